"""Attention under a causal sliding window over a KV cache: tamd_attn_fwd_window / tamd_attn_decode_window (include/tamd.h),
`window=` of the torch ops.

With off = seq_k - seq_q, key k is visible to query row s iff s + off - window + 1 <= k <= s + off (and the key-validity plane
allows it); one query row sees every key >= seq_k - window.  The bound is computed in the kernel from the row index.  Checked
through the C ABI, outputs inside sentinel-filled buffers: bit for bit against the forms that already exist where the visible
keys and the tile walk are the same (the q_start planes at seq_q == seq_k, the plain kernels under a window that covers
everything, the same call on K / V without the skipped tiles), as a gather at window 1, against the fp32 eager formula on
rectangular calls, with the keys left of the window poisoned, and for every refusal the header lists."""
import ctypes

import pytest
import torch

from conftest import max_err, record, rel_err
from transformers_amd import _cabi, ops

TAMD_E_ARG = -6
SENTINEL = -7777.0
GUARD = 64  # elements in front of and behind every output


def _guarded(shape, dtype, dev):
    """A contiguous tensor of `shape` inside a sentinel-filled buffer -> (tensor, check): check() fails when anything outside
    the tensor was written."""
    n = 1
    for x in shape:
        n *= x
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n].view(*shape)

    def check():
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "wrote outside its output"

    return view, check


def _params(q, k, v, o, lse, key_valid, scale, causal):
    ap = _cabi.AttnParams()
    ap.q, ap.k, ap.v, ap.o, ap.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
    ap.key_valid = None if key_valid is None else key_valid.data_ptr()
    ap.batch, ap.seq_q, ap.heads_q, ap.head_dim = q.shape
    ap.seq_k, ap.heads_kv = k.shape[1], k.shape[2]
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(ap, f"{name}_stride_b", t.stride(0))
        setattr(ap, f"{name}_stride_s", t.stride(1))
        setattr(ap, f"{name}_stride_h", t.stride(2))
    ap.scale, ap.causal, ap.dropout_p, ap.dropout_seed, ap.q_prescaled = scale, int(causal), 0.0, 0, 0
    ap.dtype = _cabi.TAMD_BF16 if q.dtype == torch.bfloat16 else _cabi.TAMD_F16
    return ap


def _stream(be, t):
    st = be.stream(t)
    return ctypes.c_void_p(st) if st else None


def _plane(kv):
    return None if kv is None else kv.to(torch.uint8).contiguous()


def _call(be, entry, q, k, v, kv, scale, causal=True, window=None, q_start=None):
    """One C-ABI call -> (O, lse).  entry: "fwd" / "decode"; window None: the entry without a window."""
    lib = be.lib
    o, chk_o = _guarded(q.shape, q.dtype, q.device)
    lse, chk_l = _guarded((q.shape[0], q.shape[2], q.shape[1]), torch.float32, q.device)
    kvb = _plane(kv)
    ap = _params(q, k, v, o, lse, kvb, scale, causal)
    ap.q_start = None if q_start is None else q_start.data_ptr()
    st = _stream(be, q)
    if entry == "fwd":
        code = lib.tamd_attn_fwd(ctypes.byref(ap), st) if window is None else lib.tamd_attn_fwd_window(ctypes.byref(ap), window, st)
    else:
        nbytes = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        code = (lib.tamd_attn_decode(ctypes.byref(ap), ws.data_ptr(), nbytes, st) if window is None
                else lib.tamd_attn_decode_window(ctypes.byref(ap), window, ws.data_ptr(), nbytes, st))
    lib.check(code, f"{entry} window={window}")
    if q.is_cuda:
        torch.cuda.synchronize()
    chk_o()
    chk_l()
    return o.clone(), lse.clone()


def _pieces(be, q, k):
    """The number of key pieces the split-KV plan cuts this call into (from the workspace size: pieces x rows x (d + 1) floats)."""
    o = torch.empty_like(q)
    lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=q.device)
    nbytes = be.lib.tamd_attn_decode_workspace_bytes(ctypes.byref(_params(q, k, k, o, lse, None, 1.0, True)))
    rows = q.shape[0] * q.shape[1] * q.shape[2]
    assert nbytes % (rows * (q.shape[3] + 1) * 4) == 0
    return nbytes // (rows * (q.shape[3] + 1) * 4)


def ref_window(q, k, v, scale, window, key_valid):
    """`ref_attention`'s formula (test_kernels.py: eager attention in fp32 on [B,S,H,D]) with the extra `k > q + off - W` term;
    a row without a visible key is zeros (test_kernels.py:785-789) -> (O, which rows see a key [B, Sq])."""
    b, s, h, d = q.shape
    sk, g = k.shape[1], h // k.shape[2]
    off = sk - s
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
    qi, ki = torch.arange(s, device=q.device)[:, None], torch.arange(sk, device=q.device)[None, :]
    allow = ((ki <= qi + off) & (ki > qi + off - window))[None].expand(b, -1, -1)
    if key_valid is not None:
        allow = allow & key_valid[:, None, :].bool()
    seen = allow.any(-1)
    sc = (qf @ kf.transpose(-1, -2) * scale).masked_fill(~allow[:, None], float("-inf")).masked_fill(~seen[:, None, :, None], 0.0)
    pr = torch.softmax(sc, -1) * seen[:, None, :, None]
    return (pr @ vf).permute(0, 2, 1, 3), seen


def _operands(dev, b, sq, sk, hq, hkv, d, seed, dtype=torch.bfloat16):
    torch.manual_seed(seed)
    q = torch.randn(b, sq, hq, d).to(dtype).to(dev)
    k = torch.randn(b, sk, hkv, d).to(dtype).to(dev)
    v = torch.randn(b, sk, hkv, d).to(dtype).to(dev)
    return q, k, v


def _first_tile_row(sq, sk, window):
    """64 * floor((off - W + 1) / 64), clamped at 0: the first key row of the first tile any workgroup visits."""
    return max(0, (sk - sq - window + 1) // 64 * 64)


# ---- 1. seq_q == seq_k: the bits of the plane form ----------------------------------------------------------------------
# b, s, hq, hkv, d, window, right-padded keys of batch row 0
SQUARE = [(2, 200, 4, 2, 64, 70, 0), (1, 150, 2, 1, 128, 9, 0), (2, 200, 4, 2, 64, 70, 23)]


@pytest.mark.parametrize("idx", range(len(SQUARE)))
def test_square_call_has_the_bits_of_the_plane_form(env, idx):
    """tamd_attn_fwd_window at seq_q == seq_k against tamd_attn_fwd with ops.sliding_window_q_start: the same visible keys,
    the same tile walk -- O and lse bit for bit."""
    b, s, hq, hkv, d, w, pad = SQUARE[idx]
    be = ops.backend()
    q, k, v = _operands(env.device, b, s, s, hq, hkv, d, 700 + idx)
    kv = None
    if pad:
        kv = torch.ones(b, s, dtype=torch.bool, device=env.device)
        kv[0, s - pad:] = False
    planes = ops.sliding_window_q_start(b, s, w, env.device)
    o_p, lse_p = _call(be, "fwd", q, k, v, kv, d ** -0.5, q_start=planes)
    o_w, lse_w = _call(be, "fwd", q, k, v, kv, d ** -0.5, window=w)
    assert torch.equal(o_w, o_p) and torch.equal(lse_w, lse_p), idx
    ref, _ = ref_window(q, k, v, d ** -0.5, w, kv)
    assert rel_err(o_w, ref) < 0.004, idx


# ---- 2. a window that covers everything ---------------------------------------------------------------------------------
# b, sq, sk, hq, hkv, d, window, padding
COVER = [(2, 200, 200, 4, 2, 64, 200, None), (1, 40, 300, 2, 1, 128, 1 << 40, "left"), (2, 5, 300, 4, 2, 128, 300, None),
         (2, 1, 300, 4, 2, 128, 301, "left"), (1, 1, 200, 2, 2, 64, 200, None)]


def _padding(kind, b, sk, dev):
    if kind is None:
        return None
    kv = torch.ones(b, sk, dtype=torch.bool)
    if kind == "left":
        kv[0, :37] = False
    else:  # holes
        kv[0, 3:9] = False
        kv[0, 64] = False
        kv[0, sk - 30:sk - 12:3] = False
        kv[0, sk - 5] = False
    return kv.to(dev)


@pytest.mark.parametrize("idx", range(len(COVER)))
def test_window_over_everything_is_the_plain_kernel(env, idx):
    """W >= seq_k: tamd_attn_fwd_window is tamd_attn_fwd and tamd_attn_decode_window is tamd_attn_decode, bit for bit (square
    and seq_q < seq_k; one row with and without `causal`)."""
    b, sq, sk, hq, hkv, d, w, pad = COVER[idx]
    be = ops.backend()
    q, k, v = _operands(env.device, b, sq, sk, hq, hkv, d, 720 + idx)
    kv = _padding(pad, b, sk, env.device)
    for causal in ((True, False) if sq == 1 else (True,)):
        for entry in ("fwd", "decode"):
            o0, lse0 = _call(be, entry, q, k, v, kv, d ** -0.5, causal)
            o1, lse1 = _call(be, entry, q, k, v, kv, d ** -0.5, causal, window=w)
            assert torch.equal(o1, o0) and torch.equal(lse1, lse0), (idx, entry, causal)


# ---- 3. W == 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_window_of_one_key_is_a_gather(env, d, dtype):
    """One visible key: p = 1, a row sum of 1 -- o[b, s, h] is v[b, s + off, h // group], bit for bit."""
    b, sq, sk, hq, hkv = 2, 70, 200, 4, 2
    q, k, v = _operands(env.device, b, sq, sk, hq, hkv, d, 730, dtype)
    o, lse = _call(ops.backend(), "fwd", q, k, v, None, d ** -0.5, window=1)
    want = v[:, sk - sq:].repeat_interleave(hq // hkv, 2)
    assert torch.equal(o, want)
    assert bool(torch.isfinite(lse).all())


# ---- 4. - 6. rectangular calls on the forward entry ---------------------------------------------------------------------
# b, sq, sk, hq, hkv, d, window, padding
RECT = [(2, 40, 300, 4, 2, 128, 100, None),
        (1, 150, 333, 2, 1, 64, 64, "left")]  # two query blocks, a ragged key tile, a window of one tile, a left-padded row
_RECT = {}


def _rect(env, idx):
    key = (env.name, idx)
    if key not in _RECT:
        b, sq, sk, hq, hkv, d, w, pad = RECT[idx]
        q, k, v = _operands(env.device, b, sq, sk, hq, hkv, d, 740 + idx)
        kv = _padding(pad, b, sk, env.device)
        r = {"q": q, "k": k, "v": v, "kv": kv, "w": w, "scale": d ** -0.5, "be": ops.backend()}
        r["o"], r["lse"] = _call(r["be"], "fwd", q, k, v, kv, r["scale"], window=w)
        _RECT[key] = r
    return _RECT[key]


@pytest.mark.parametrize("idx", range(len(RECT)))
def test_rectangular_call_against_fp32_eager(env, idx):
    r = _rect(env, idx)
    ref, seen = ref_window(r["q"], r["k"], r["v"], r["scale"], r["w"], r["kv"])
    e = rel_err(r["o"], ref)
    record("attn_window", f"fwd_rect{idx}_{env.name}", e)
    print(f"rect {idx}: vs fp32 {float(e):.5f}")
    assert e < 0.004, idx
    # rows without a visible key (left padding wider than the window): exactly zeros, lse = +inf
    dead = ~seen
    if idx == 1:
        assert not bool(dead.any())  # (37 padded keys, the first row's window starts at 120)
    o_rows = r["o"].permute(0, 2, 1, 3)[dead[:, None].expand(-1, r["q"].shape[2], -1)]
    assert torch.count_nonzero(o_rows) == 0
    # the split-KV entry on the same call (any number of rows through the C ABI): the project's kernel-against-kernel gates
    o_d, lse_d = _call(r["be"], "decode", r["q"], r["k"], r["v"], r["kv"], r["scale"], window=r["w"])
    assert rel_err(o_d, r["o"]) < 0.0035, idx
    assert max_err(lse_d, r["lse"]) < 2e-3, idx


def test_fully_masked_rows_under_a_window_are_zero(env):
    """A left padding wider than the window: the first rows see no key -- O = 0 and lse = +inf on both entries."""
    b, sq, sk, hq, hkv, d, w = 1, 20, 160, 2, 1, 64, 8
    q, k, v = _operands(env.device, b, sq, sk, hq, hkv, d, 745)
    kv = torch.ones(b, sk, dtype=torch.bool)
    kv[0, :sk - sq + 6] = False  # rows 0 .. 5 see padded keys only (row s: keys s + 133 .. s + 140, padded below 146)
    kv = kv.to(env.device)
    ref, seen = ref_window(q, k, v, d ** -0.5, w, kv)
    assert seen[0].tolist() == [False] * 6 + [True] * 14
    for entry, gate in (("fwd", 0.004), ("decode", 0.0045)):
        o, lse = _call(ops.backend(), entry, q, k, v, kv, d ** -0.5, window=w)
        assert torch.count_nonzero(o[:, :6]) == 0 and bool(torch.isposinf(lse[:, :, :6]).all()), entry
        assert bool(torch.isfinite(lse[:, :, 6:]).all()), entry
        assert rel_err(o, ref) < gate, entry


@pytest.mark.parametrize("idx", range(len(RECT)))
def test_skipped_tiles_are_absent_tiles(env, idx):
    """The call on K / V sliced from 64 * floor((off - W + 1) / 64): the same bound relative to the same tiles, only the
    starting index differs -- the same bits."""
    r = _rect(env, idx)
    start = _first_tile_row(r["q"].shape[1], r["k"].shape[1], r["w"])
    assert start >= 64
    kv = None if r["kv"] is None else r["kv"][:, start:]
    o, lse = _call(r["be"], "fwd", r["q"], r["k"][:, start:], r["v"][:, start:], kv, r["scale"], window=r["w"])
    assert torch.equal(o, r["o"]) and torch.equal(lse, r["lse"]), idx


def _poisoned(k, v, sq, window):
    """K / V with the rows of the tiles nobody visits set to NaN and the rows between there and the first row's bound --
    invisible to every row, but inside a visited tile, where only the mask keeps them out -- to +-1e4."""
    sk = k.shape[1]
    lo, start = sk - sq - window + 1, _first_tile_row(sq, sk, window)
    assert 0 < start < lo
    k, v = k.clone(), v.clone()
    k[:, :start], v[:, :start] = float("nan"), float("nan")
    sign = torch.where(torch.arange(lo - start, device=k.device) % 2 == 0, 1.0, -1.0).to(k.dtype)[None, :, None, None]
    k[:, start:lo], v[:, start:lo] = 1e4 * sign, -1e4 * sign
    return k, v


@pytest.mark.parametrize("idx", range(len(RECT)))
def test_keys_left_of_the_window_do_not_reach_the_result_fwd(env, idx):
    r = _rect(env, idx)
    k, v = _poisoned(r["k"], r["v"], r["q"].shape[1], r["w"])
    o, lse = _call(r["be"], "fwd", r["q"], k, v, r["kv"], r["scale"], window=r["w"])
    assert torch.equal(o, r["o"]) and torch.equal(lse, r["lse"]), idx


# ---- 7. the split-KV entry ---------------------------------------------------------------------------------------------
# b, sq, sk, hq, hkv, d, window, padding, dtype
DECODE = [(2, 5, 300, 4, 2, 128, 130, None, torch.bfloat16),
          (1, 16, 200, 2, 2, 64, 17, "holes", torch.bfloat16),   # every tile a piece of its own: two pieces see no key
          (2, 1, 300, 4, 2, 128, 100, None, torch.bfloat16),     # the re-strided form: every head row has the same bound
          (2, 5, 300, 4, 2, 128, 130, None, torch.float16)]
_DEC = {}


def _dec(env, idx):
    key = (env.name, idx)
    if key not in _DEC:
        b, sq, sk, hq, hkv, d, w, pad, dtype = DECODE[idx]
        q, k, v = _operands(env.device, b, sq, sk, hq, hkv, d, 760 + idx, dtype)
        kv = _padding(pad, b, sk, env.device)
        r = {"q": q, "k": k, "v": v, "kv": kv, "w": w, "scale": d ** -0.5, "be": ops.backend()}
        r["o"], r["lse"] = _call(r["be"], "decode", q, k, v, kv, r["scale"], window=w)
        r["o_f"], r["lse_f"] = _call(r["be"], "fwd", q, k, v, kv, r["scale"], window=w)
        _DEC[key] = r
    return _DEC[key]


@pytest.mark.parametrize("idx", range(len(DECODE)))
def test_decode_entry_against_fp32_eager_and_the_forward_entry(env, idx):
    r = _dec(env, idx)
    q, k = r["q"], r["k"]
    if idx == 1:  # one piece per 64-key tile; the first row's window starts at key 168: pieces 0 and 1 see no key
        assert _pieces(r["be"], q, k) == -(-k.shape[1] // 64) == 4
        assert (k.shape[1] - q.shape[1] - r["w"] + 1) // 64 == 2
    ref, seen = ref_window(q, k, r["v"], r["scale"], r["w"], r["kv"])
    assert bool(seen.all())
    e_ref, e_fwd, e_lse = rel_err(r["o"], ref), rel_err(r["o"], r["o_f"]), max_err(r["lse"], r["lse_f"])
    e_f = rel_err(r["o_f"], ref)
    record("attn_window", f"decode{idx}_{env.name}", e_ref)
    print(f"decode {idx}: vs fp32 {float(e_ref):.5f} (forward entry {float(e_f):.5f}) vs forward entry {float(e_fwd):.5f} lse {e_lse:.2e}")
    assert e_ref < 0.0045, idx
    assert e_f < 0.004, idx
    assert e_fwd < 0.0035, idx
    assert e_lse < 2e-3, idx


def test_one_row_sees_the_same_keys_with_and_without_causal(env):
    r = _dec(env, 2)
    for entry, want in (("decode", (r["o"], r["lse"])), ("fwd", (r["o_f"], r["lse_f"]))):
        o, lse = _call(r["be"], entry, r["q"], r["k"], r["v"], r["kv"], r["scale"], causal=False, window=r["w"])
        assert torch.equal(o, want[0]) and torch.equal(lse, want[1]), entry


@pytest.mark.parametrize("idx", [0, 2])
def test_keys_left_of_the_window_do_not_reach_the_result_decode(env, idx):
    r = _dec(env, idx)
    k, v = _poisoned(r["k"], r["v"], r["q"].shape[1], r["w"])
    o, lse = _call(r["be"], "decode", r["q"], k, v, r["kv"], r["scale"], window=r["w"])
    assert torch.equal(o, r["o"]) and torch.equal(lse, r["lse"]), idx


def test_forward_entry_in_fp16(env):
    b, sq, sk, hq, hkv, d, w, pad = RECT[0]
    q, k, v = _operands(env.device, b, sq, sk, hq, hkv, d, 770, torch.float16)
    o, _ = _call(ops.backend(), "fwd", q, k, v, None, d ** -0.5, window=w)
    ref, _ = ref_window(q, k, v, d ** -0.5, w, None)
    assert rel_err(o, ref) < 0.004


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(env):
    be = ops.backend()
    lib, dev = be.lib, env.device
    assert lib.tamd_abi_version() == 13
    q, k, v = _operands(dev, 1, 8, 160, 2, 2, 64, 780)

    def codes(q, k, v, window, causal=True, **fields):
        o = torch.empty_like(q)
        lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=dev)
        ap = _params(q, k, v, o, lse, None, 0.125, causal)
        keep = []
        for name, val in fields.items():
            if torch.is_tensor(val):
                keep.append(val)
                val = val.data_ptr()
            setattr(ap, name, val)
        nbytes = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        out = (lib.tamd_attn_fwd_window(ctypes.byref(ap), window, _stream(be, q)),
               lib.tamd_attn_decode_window(ctypes.byref(ap), window, ws.data_ptr(), max(nbytes, 16), _stream(be, q)))
        if q.is_cuda:
            torch.cuda.synchronize()
        return out

    assert codes(q, k, v, 40) == (0, 0)
    assert codes(q, k, v, 0) == (TAMD_E_ARG, TAMD_E_ARG)
    assert codes(q, k, v, -3) == (TAMD_E_ARG, TAMD_E_ARG)
    assert codes(k[:, :12], q, q, 4) == (TAMD_E_ARG, TAMD_E_ARG)                 # seq_q 12 > seq_k 8
    assert codes(q, k, v, 40, causal=False) == (TAMD_E_ARG, TAMD_E_ARG)          # several rows, not causal
    assert codes(q[:, :1], k, v, 40, causal=False) == (0, 0)                     # ... one row: served
    planes = ops.sliding_window_q_start(1, 8, 4, dev)
    assert codes(q, k[:, :8], v[:, :8], 4, q_start=planes) == (TAMD_E_ARG, TAMD_E_ARG)
    assert codes(q, k, v, 40, dropout_p=0.1) == (TAMD_E_ARG, TAMD_E_ARG)
    cnt = torch.tensor([100], dtype=torch.int32, device=dev)
    assert codes(q, k, v, 40, seq_k_dev=cnt) == (TAMD_E_ARG, TAMD_E_ARG)
    # the torch ops: inference only, and not together with what the window entries refuse
    with pytest.raises(ops.TamdError):
        ops.attention(q.clone().requires_grad_(True), k, v, 0.125, True, window=40)
    with pytest.raises(ops.TamdError):
        ops.attention(q, k, v, 0.125, True, window=0)
    with pytest.raises(ops.TamdError):
        ops.attention(q, k, v, 0.125, True, window=40, kv_len=cnt)
    with pytest.raises(ops.TamdError):
        ops.raw_attn_fwd(q, k[:, :8], v[:, :8], 0.125, True, window=4, q_start=planes)
    with pytest.raises(RuntimeError):  # (the entry point's TAMD_E_ARG through the dispatcher)
        ops.attention(q, k, v, 0.125, False, window=40)
    # the entries without a window keep their refusals
    o = torch.empty_like(q)
    lse = torch.empty(1, 2, 8, dtype=torch.float32, device=dev)
    ap = _params(q, k, v, o, lse, None, 0.125, True)
    ap.seq_k_dev = cnt.data_ptr()
    assert lib.tamd_attn_fwd(ctypes.byref(ap), _stream(be, q)) == TAMD_E_ARG


# ---- 9. the dispatcher op ----------------------------------------------------------------------------------------------
def test_dispatcher_picks_the_entry_by_shape(env):
    """At most 16 query rows over at least 128 keys: the split-KV entry; otherwise the forward entry -- the bits of the direct
    C-ABI calls."""
    r = _dec(env, 0)    # 5 rows over 300 keys
    assert torch.equal(ops.attention(r["q"], r["k"], r["v"], r["scale"], True, r["kv"], window=r["w"]), r["o"])
    o, lse = ops.raw_attn_fwd(r["q"], r["k"], r["v"], r["scale"], True, r["kv"], window=r["w"])
    assert torch.equal(o, r["o"]) and torch.equal(lse, r["lse"])
    assert not torch.equal(r["o"], r["o_f"])  # (the two schedules round differently: the comparison above tells them apart)
    r = _dec(env, 1)    # 16 rows over 200 keys, a padding mask
    o, lse = ops.raw_attn_fwd(r["q"], r["k"], r["v"], r["scale"], True, r["kv"], window=r["w"])
    assert torch.equal(o, r["o"]) and torch.equal(lse, r["lse"])
    r = _rect(env, 0)   # 40 rows
    assert torch.equal(ops.attention(r["q"], r["k"], r["v"], r["scale"], True, r["kv"], window=r["w"]), r["o"])
    o, lse = ops.raw_attn_fwd(r["q"], r["k"], r["v"], r["scale"], True, r["kv"], window=r["w"])
    assert torch.equal(o, r["o"]) and torch.equal(lse, r["lse"])
    r = _dec(env, 0)    # 5 rows over 100 keys: below the key threshold
    k, v = r["k"][:, :100], r["v"][:, :100]
    o_f, lse_f = _call(r["be"], "fwd", r["q"], k, v, None, r["scale"], window=30)
    o, lse = ops.raw_attn_fwd(r["q"], k, v, r["scale"], True, None, window=30)
    assert torch.equal(o, o_f) and torch.equal(lse, lse_f)
