"""Decode attention over a pre-allocated KV cache whose key counts live in device memory (ABI 13: tamd_attn_params.seq_k_dev,
`kv_len` of the torch ops, the third slot of `TamdMask`).

Batch row b of such a call is the problem with len_b = clamp(seq_k_dev[b], 0, seq_k) keys, exactly as if K / V had been sliced
to len_b rows: checked per row against the training kernel and the fp32 reference on sliced operands, bit for bit against
the validity-plane form of the same call (same plan, same visible keys, same tile order), and with the unused slots
poisoned -- the key tiles behind len_b are not read, so nothing they hold reaches the result."""
import ctypes

import pytest
import torch

from conftest import max_err, rel_err
from test_kernels import ref_attention
from transformers_amd import _cabi, ops

TAMD_E_ARG = -6

# b, sq, hq, hkv, d, causal, allocation, key counts, padding mask
CASES = [
    (4, 1, 4, 2, 128, True, 300, [1, 64, 130, 300], None),       # GQA re-striding; one key, a full tile, two tiles + 2, everything
    (4, 1, 4, 4, 64, True, 300, [63, 65, 0, 307], "left37"),     # tile boundary - 1 / + 1, a row without keys, a count past the allocation
    (3, 5, 4, 2, 64, True, 300, [5, 70, 260], None),             # a block of rows: the diagonal is aligned to the row's own count
    (2, 1, 2, 1, 128, False, 129, [129, 77], "holes"),           # not causal, ragged allocation, a padding mask with holes
]


def _params(q, k, v, o, lse, key_valid, scale, causal, counts=None, q_start=None):
    ap = _cabi.AttnParams()
    ap.q, ap.k, ap.v, ap.o, ap.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
    ap.key_valid = None if key_valid is None else key_valid.data_ptr()
    ap.q_start = None if q_start is None else q_start.data_ptr()
    ap.batch, ap.seq_q, ap.heads_q, ap.head_dim = q.shape
    ap.seq_k, ap.heads_kv = k.shape[1], k.shape[2]
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(ap, f"{name}_stride_b", t.stride(0))
        setattr(ap, f"{name}_stride_s", t.stride(1))
        setattr(ap, f"{name}_stride_h", t.stride(2))
    ap.scale, ap.causal, ap.dtype, ap.dropout_p, ap.dropout_seed, ap.q_prescaled = scale, int(causal), _cabi.TAMD_BF16, 0.0, 0, 0
    ap.seq_k_dev = None if counts is None else counts.data_ptr()
    return ap


def _stream(be, t):
    st = be.stream(t)
    return ctypes.c_void_p(st) if st else None


def _decode(be, q, k, v, key_valid, scale, causal, counts):
    """tamd_attn_decode through the C ABI -> (O, lse)."""
    lib = be.lib
    o = torch.empty_like(q)
    lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=q.device)
    ap = _params(q, k, v, o, lse, key_valid, scale, causal, counts)
    nbytes = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    lib.check(lib.tamd_attn_decode(ctypes.byref(ap), ws.data_ptr(), nbytes, _stream(be, q)), "decode")
    if q.is_cuda:
        torch.cuda.synchronize()
    return o, lse


def _train_fwd(be, q, k, v, key_valid, scale, causal):
    o = torch.empty_like(q)
    lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=q.device)
    ap = _params(q, k, v, o, lse, key_valid, scale, causal)
    be.lib.check(be.lib.tamd_attn_fwd(ctypes.byref(ap), _stream(be, q)), "fwd")
    if q.is_cuda:
        torch.cuda.synchronize()
    return o, lse


_RUNS = {}


def _case(env, idx):
    """Operands and the runs of one case, computed once per backend and shared (never modified) by the tests below."""
    key = (env.name, idx)
    if key in _RUNS:
        return _RUNS[key]
    b, sq, hq, hkv, d, causal, sk, counts, pad = CASES[idx]
    dev = env.device
    be = ops.backend()
    torch.manual_seed(130 + idx)
    q = torch.randn(b, sq, hq, d).bfloat16().to(dev)
    k = torch.randn(b, sk, hkv, d).bfloat16().to(dev)
    v = torch.randn(b, sk, hkv, d).bfloat16().to(dev)
    kv = None
    if pad is not None:
        kv = torch.ones(b, sk, dtype=torch.bool)
        if pad == "left37":
            kv[0, :37] = False
        else:
            kv[0, 3:9] = False
            kv[0, 64] = False
            kv[1, ::5] = False
            kv[1, 70:80] = False
        kv = kv.to(dev)
    scale = d ** -0.5
    lens = [min(max(c, 0), sk) for c in counts]
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    kvb = None if kv is None else kv.to(torch.uint8).contiguous()
    r = {"q": q, "k": k, "v": v, "kv": kv, "kvb": kvb, "scale": scale, "causal": causal, "lens": lens, "cnt": cnt, "be": be}
    r["o"], r["lse"] = _decode(be, q, k, v, kvb, scale, causal, cnt)
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_row_is_the_problem_sliced_to_its_count(env, idx):
    """Per batch row: the training kernel and the fp32 reference on K / V sliced to len_b (tolerances of
    test_attention_decode_split_kv); a row without keys is exactly zeros with lse = +inf."""
    r = _case(env, idx)
    q, k, v, kv = r["q"], r["k"], r["v"], r["kv"]
    for i, n in enumerate(r["lens"]):
        o_i, lse_i = r["o"][i:i + 1], r["lse"][i:i + 1]
        if n == 0:
            assert torch.count_nonzero(o_i) == 0 and bool(torch.isposinf(lse_i).all()), (idx, i)
            continue
        ki, vi = k[i:i + 1, :n], v[i:i + 1, :n]
        kvi = None if kv is None else kv[i:i + 1, :n]
        ref = ref_attention(q[i:i + 1], ki, vi, r["scale"], r["causal"], kvi)
        o_t, lse_t = _train_fwd(r["be"], q[i:i + 1], ki, vi, None if kvi is None else kvi.to(torch.uint8).contiguous(),
                                r["scale"], r["causal"])
        e_ref, e_trn, e_lse = rel_err(o_i, ref), rel_err(o_i, o_t), max_err(lse_i, lse_t)
        print(f"case {idx} row {i} len {n}: vs fp32 {float(e_ref):.5f} vs training kernel {float(e_trn):.5f} lse {e_lse:.2e}")
        assert e_ref < 0.0045, (idx, i)
        assert e_trn < 0.0035, (idx, i)
        assert e_lse < 2e-3, (idx, i)


def _pieces(be, q, k, causal):
    """The number of key pieces tamd_attn_decode's plan cuts this call into (from the workspace size: pieces x rows x (d + 1)
    floats)."""
    o = torch.empty_like(q)
    lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=q.device)
    nbytes = be.lib.tamd_attn_decode_workspace_bytes(ctypes.byref(_params(q, k, k, o, lse, None, 1.0, causal)))
    rows = q.shape[0] * q.shape[1] * q.shape[2]
    assert nbytes % (rows * (q.shape[3] + 1) * 4) == 0
    return nbytes // (rows * (q.shape[3] + 1) * 4)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_same_bits_as_the_form_without_the_field(env, idx):
    """seq_k_dev = NULL and a validity plane key_valid & (k < len_b) over the same allocation: the same plan, the same visible
    keys, the same tile order -- the same bits.

    That holds where a [batch, seq_k] plane can say which keys a row sees: one query row, or no causal mask (cases 0, 1, 3).
    For a causal block of rows (case 2) it cannot: under the plane the diagonal stays aligned to the ALLOCATION (row s sees
    k <= s + 300 - 5, every key below len_b), while the row's problem is the one sliced to len_b (k <= s + len_b - 5), which is
    what include/tamd.h states and test_row_is_the_problem_sliced_to_its_count checks.  The form without the field that IS the
    same problem there is the call on K / V sliced to len_b, batch row by batch row; at these shapes both plans make every
    64-key tile a piece of its own (asserted), so the pieces and the order of their merge are the same, and the bits must be."""
    r = _case(env, idx)
    be, q, k, v = r["be"], r["q"], r["k"], r["v"]
    sk = k.shape[1]
    if q.shape[1] == 1 or not r["causal"]:
        used = torch.arange(sk, device=env.device)[None] < torch.tensor(r["lens"], device=env.device)[:, None]
        plane = used if r["kv"] is None else (r["kv"] & used)
        o2, lse2 = _decode(be, q, k, v, plane.to(torch.uint8).contiguous(), r["scale"], r["causal"], None)
        assert torch.equal(o2, r["o"]), idx
        assert torch.equal(lse2, r["lse"]), idx
        return
    assert r["kv"] is None
    assert _pieces(be, q, k, r["causal"]) == -(-sk // 64)
    for i, n in enumerate(r["lens"]):
        qi, ki, vi = q[i:i + 1], k[i:i + 1, :n], v[i:i + 1, :n]
        assert _pieces(be, qi, ki, r["causal"]) == -(-n // 64)
        o2, lse2 = _decode(be, qi, ki, vi, None, r["scale"], r["causal"], None)
        assert torch.equal(o2, r["o"][i:i + 1]), (idx, i)
        assert torch.equal(lse2, r["lse"][i:i + 1]), (idx, i)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_slots_behind_the_count_are_not_read_into_the_result(env, idx):
    """K and V slots >= len_b overwritten with NaN: the same bits as the un-poisoned run."""
    r = _case(env, idx)
    k, v = r["k"].clone(), r["v"].clone()
    for i, n in enumerate(r["lens"]):
        k[i, n:] = float("nan")
        v[i, n:] = float("nan")
    o2, lse2 = _decode(r["be"], r["q"], k, v, r["kvb"], r["scale"], r["causal"], r["cnt"])
    assert torch.equal(o2, r["o"]), idx
    assert torch.equal(lse2, r["lse"]), idx


def test_entry_points_that_refuse_the_field(env):
    r = _case(env, 0)
    be = r["be"]
    lib = be.lib
    assert lib.tamd_abi_version() == 13
    q, k, v = r["q"], r["k"], r["v"]
    o = torch.empty_like(q)
    lse = torch.empty(q.shape[0], q.shape[2], q.shape[1], dtype=torch.float32, device=q.device)
    ap = _params(q, k, v, o, lse, None, r["scale"], True, r["cnt"])
    assert lib.tamd_attn_fwd(ctypes.byref(ap), _stream(be, q)) == TAMD_E_ARG
    dq, dk, dv, do = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.zeros_like(q)
    delta = torch.empty(2, *lse.shape, dtype=torch.float32, device=q.device)
    bp = _cabi.AttnBwdParams()
    bp.fwd = ap
    bp.dout, bp.dq, bp.dk, bp.dv, bp.delta = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    assert lib.tamd_attn_bwd(ctypes.byref(bp), _stream(be, q)) == TAMD_E_ARG
    # with packed-sequence bounds (which need seq_q == seq_k): refused by the decode entry point
    s = 8
    q8 = torch.randn(1, s, 2, 64).bfloat16().to(env.device)
    k8 = torch.randn(1, s, 2, 64).bfloat16().to(env.device)
    o8 = torch.empty_like(q8)
    lse8 = torch.empty(1, 2, s, dtype=torch.float32, device=env.device)
    qs = ops.packed_q_start(torch.zeros(1, s, dtype=torch.long)).to(env.device)
    cnt = torch.tensor([s], dtype=torch.int32, device=env.device)
    ap8 = _params(q8, k8, k8, o8, lse8, None, 0.125, True, cnt, q_start=qs)
    nbytes = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap8))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=env.device)
    assert lib.tamd_attn_decode(ctypes.byref(ap8), ws.data_ptr(), nbytes, _stream(be, q8)) == TAMD_E_ARG
    if q.is_cuda:
        torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_dispatcher_op_takes_the_decode_kernel(env, idx):
    r = _case(env, idx)
    o = ops.attention(r["q"], r["k"], r["v"], r["scale"], r["causal"], r["kv"], kv_len=r["cnt"])
    assert torch.equal(o, r["o"]), idx
    o2, lse2 = ops.raw_attn_fwd(r["q"], r["k"], r["v"], r["scale"], r["causal"], r["kv"], kv_len=r["cnt"])
    assert torch.equal(o2, r["o"]) and torch.equal(lse2, r["lse"]), idx


def test_dispatcher_op_below_the_decode_threshold_and_its_checks(env):
    """An allocation of 40 slots (the shape alone would take the training kernel): with kv_len it is the decode kernel."""
    torch.manual_seed(140)
    dev = env.device
    b, sk, hq, hkv, d = 2, 40, 2, 1, 64
    q = torch.randn(b, 1, hq, d).bfloat16().to(dev)
    k = torch.randn(b, sk, hkv, d).bfloat16().to(dev)
    v = torch.randn(b, sk, hkv, d).bfloat16().to(dev)
    lens = [7, 40]
    cnt = torch.tensor(lens, dtype=torch.int32, device=dev)
    scale = d ** -0.5
    o = ops.attention(q, k, v, scale, False, None, kv_len=cnt)
    o_abi, _ = _decode(ops.backend(), q, k, v, None, scale, False, cnt)
    assert torch.equal(o, o_abi)
    for i, n in enumerate(lens):
        want = ops.attention(q[i:i + 1], k[i:i + 1, :n], v[i:i + 1, :n], scale, False)  # (the training kernel: 40 < 128 keys)
        assert rel_err(o[i:i + 1], want) < 0.0035, i
        assert rel_err(o[i:i + 1], ref_attention(q[i:i + 1], k[i:i + 1, :n], v[i:i + 1, :n], scale, False, None)) < 0.0045, i
    kp, vp = k.clone(), v.clone()
    kp[0, 7:], vp[0, 7:] = float("nan"), float("nan")
    assert torch.equal(ops.attention(q, kp, vp, scale, False, None, kv_len=cnt), o)
    with pytest.raises(RuntimeError):
        ops.attention(q, k, v, scale, False, None, kv_len=cnt.long())
    with pytest.raises(RuntimeError):
        ops.attention(q, k, v, scale, False, None, kv_len=torch.zeros(b + 1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        ops.attention(q, k, v, scale, False, None, kv_len=cnt[:, None])
    with pytest.raises(RuntimeError):  # (TamdError is one)
        ops.attention(q.clone().requires_grad_(True), k, v, scale, False, None, kv_len=cnt)
    # existing positional and keyword calls are what they were
    assert torch.equal(ops.attention(q, k, v, scale, False, None, 0.0, None, None, None), ops.attention(q, k, v, scale, False))


# ---- host logic (CPU) ---------------------------------------------------------------------------------------------------
def test_mask_factory_hands_a_static_cache_decode_step_its_key_count():
    from transformers import masking_utils as mu

    from transformers_amd.attention import TamdMask, _key_valid_from_mask, _mask_kv_len, split_mask, split_mask_kv, tamd_mask

    am = torch.ones(2, 12, dtype=torch.long)
    am[1, :3] = 0
    for q_offset in (torch.tensor(11), 11):
        m = tamd_mask(2, 1, 32, q_offset=q_offset, mask_function=mu.causal_mask_function, attention_mask=am)
        assert isinstance(m, TamdMask) and m.q_start is None
        assert m.kv_len.dtype == torch.int32 and m.kv_len.tolist() == [12, 12]
        assert m.key_valid.shape == (2, 32)
        assert m.key_valid[:, :12].tolist() == am.tolist() and not bool(m.key_valid[:, 12:].any())  # the zero tail
        assert _mask_kv_len(m) == 32                      # the allocation: K / V are not sliced
    m = tamd_mask(2, 1, 32, q_offset=torch.tensor(11), mask_function=mu.causal_mask_function, device=torch.device("cpu"))
    assert isinstance(m, TamdMask) and m.key_valid is None and m.q_start is None and m.kv_len.tolist() == [12, 12]
    assert _mask_kv_len(m) is None
    assert TamdMask(am, None).kv_len is None              # the two-argument form keeps working
    # `generate` prepares the step's mask before the forward, whose own mask creation then meets it as `attention_mask`:
    # it answers what masking_utils asks of a 2-D mask and comes back from the factory unchanged
    moved = m.to(device=torch.device("cpu"), dtype=torch.bool)
    assert m.ndim == 2 and isinstance(moved, TamdMask) and moved.kv_len.tolist() == [12, 12] and moved.key_valid is None
    assert tamd_mask(2, 1, 32, q_offset=torch.tensor(11), mask_function=mu.causal_mask_function, attention_mask=m) is m
    kv, qs, n = split_mask_kv(m, 2, 32)
    assert kv is None and qs is None and n is m.kv_len
    # a block that only takes (key_valid, q_start) refuses such a mask instead of ignoring the count
    with pytest.raises(ops.TamdError):
        split_mask(m, 2, 32)
    with pytest.raises(ops.TamdError):
        _key_valid_from_mask(m, 2, 32)
    # the other branches return what they returned: the prefill into the cache is sliced on the host
    p = tamd_mask(2, 4, 32, q_offset=3, mask_function=mu.causal_mask_function, device=torch.device("cpu"))
    assert torch.is_tensor(p) and p.shape == (2, 7)
    assert tamd_mask(2, 1, 12, q_offset=11, mask_function=mu.causal_mask_function) is None  # (a dynamic cache)
