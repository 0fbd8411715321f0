"""Attention kernels, element by element (include/tamd.h "attention"): tamd_attn_fwd / _bwd / _decode / _fwd_window /
_decode_window through the C ABI, every output inside a sentinel-filled buffer, bf16 and fp16, head_dim 64 and 128, the same
shapes under the CPU execution model and on the MI355X.

Part A -- exact visibility.  q = 0 makes every score 0 and every p = exp2(0) = 1: the row sum is the COUNT n(s) of visible
keys and O[s, j] * n(s) the number of visible keys whose 0/1 code has bit j -- integers, exact in fp32.  V[b, k, h, :] is a
code of the key index (columns [0, d/2) one-hot in k mod d/2, columns [d/2, d) one-hot in (k // (d/2)) mod d/2, all rotated
by b + h), so the set of keys a row saw is decoded from (O, lse) and compared, as integers, with a mask written here from
the header's formulas (never from the kernels' helpers).  K holds arbitrary finite values.  What is NOT an integer equality:

  lse = ln n     U = the fp32 ulp of ln n.  The training kernel computes (0 + v_log_f32(n)) * ln2f: one ulp of log2 n (<= 1.39 U,
                 the binade may differ), the product's half ulp, the constant's 0.05: <= 3 U (n = 1: exactly 0).
                 The split-KV merge (attn_combine_kernel, at most 8 pieces here, asserted) takes mx + logf(sum_s expf(lse_s - mx)):
                   mx, the largest piece's lse                                   3 U
                   the argument lse_s - mx: both ends and the subtraction        3 + 3 + 0.5 U, as a relative error of w_s
                   __expf = v_exp(x * log2e): the product's rounding             0.69 U          "
                   v_exp_f32, one ulp                                            1    x 2^-23    "
                   the sum of <= 8 weights over four waves: <= 5 additions       2.5  x 2^-23    "
                   __logf = v_log * ln2 of a sum in [1, 8]                       2.4  x 2^-23
                   the last addition                                             0.5 U
                 <= 11 U + 6 x 2^-23 (ln n in [4, 8): 12.5 U); one key in all (n = 1): exactly 0.
  O = c / n      one ulp_T of round_T(c / n): the reference errs by one rounding, the kernel rounds oacc * (1 / l).

Part B -- random operands: every element of O, lse, dq, dk, dv within kernel_checks.check's gate of a float64 reference,
with `s` built in Case.s_forward / Case.s_backward from float64 reference quantities only."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import record
from kernel_checks import BF16, F16, F32, MANT, NAME, SENT, Guarded, check, rnd, ulp
from transformers_amd import _cabi, ops

OK, E_SHAPE, E_ARG = 0, -2, -6
CODE = {BF16: _cabi.TAMD_BF16, F16: _cabi.TAMD_F16}
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
TD = [pytest.param(BF16, 64, id="bf16-64"), pytest.param(BF16, 128, id="bf16-128"),
      pytest.param(F16, 64, id="fp16-64"), pytest.param(F16, 128, id="fp16-128")]
GROUP = "attn_elements"
_LSE = {}


# ---- buffers and calls ---------------------------------------------------------------------------------------------------
class Operands:
    """seq_q == seq_k: q, k, v as views of one fused [b, s, (hq + 2 hkv) d] buffer.  Otherwise k and v as views of a fused
    [b, sk, 2 hkv d] buffer and q in one of its own with a row stride of hq d + 64."""

    def __init__(self, q, k, v, dtype, dev):
        b, sq, hq, d = q.shape
        sk, hkv = k.shape[1], k.shape[2]
        if sq == sk:
            self.buf = torch.zeros(b, sk, (hq + 2 * hkv) * d, dtype=dtype, device=dev)
            self.q = self.buf[:, :, :hq * d].unflatten(-1, (hq, d))
            kv = self.buf[:, :, hq * d:]
        else:
            self.qbuf = torch.zeros(b, sq, hq * d + 64, dtype=dtype, device=dev)
            self.q = self.qbuf[:, :, :hq * d].unflatten(-1, (hq, d))
            kv = self.buf = torch.zeros(b, sk, 2 * hkv * d, dtype=dtype, device=dev)
        self.k = kv[:, :, :hkv * d].unflatten(-1, (hkv, d))
        self.v = kv[:, :, hkv * d:].unflatten(-1, (hkv, d))
        self.q.copy_(q), self.k.copy_(k), self.v.copy_(v)


class Out:
    """o [b, sq, hq, d] with a row stride of hq d + 16 and lse [b, hq, sq], each in a guarded, sentinel-filled buffer."""

    def __init__(self, b, sq, hq, d, dtype, dev):
        self.og = Guarded((b, sq, hq * d + 16), dtype, dev, 512)
        self.o = self.og.t[:, :, :hq * d].unflatten(-1, (hq, d))
        self.lg = Guarded((b, hq, sq), F32, dev, 64)
        self.lse = self.lg.t

    def intact(self):
        return self.og.intact() and self.lg.intact() and bool((self.og.t[:, :, -16:] == SENT).all())

    def untouched(self):
        return self.og.untouched() and self.lg.untouched()


def _params(q, k, v, o, lse, dtype, scale, causal, kv=None, planes=None, p=0.0, seed=0, seed_dev=None, counts=None, prescaled=0):
    ap = _cabi.AttnParams()
    ap.q, ap.k, ap.v, ap.o, ap.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
    ap.key_valid = None if kv is None else kv.data_ptr()
    ap.q_start = None if planes is None else planes.data_ptr()
    ap.batch, ap.seq_q, ap.heads_q, ap.head_dim = q.shape
    ap.seq_k, ap.heads_kv = k.shape[1], k.shape[2]
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(ap, f"{name}_stride_b", t.stride(0))
        setattr(ap, f"{name}_stride_s", t.stride(1))
        setattr(ap, f"{name}_stride_h", t.stride(2))
    ap.scale, ap.causal, ap.dtype, ap.dropout_p, ap.dropout_seed, ap.q_prescaled = scale, int(causal), CODE[dtype], p, seed, prescaled
    ap.dropout_seed_dev = None if seed_dev is None else seed_dev.data_ptr()
    ap.seq_k_dev = None if counts is None else counts.data_ptr()
    return ap


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def _stream(be, t):
    st = be.stream(t)
    return ctypes.c_void_p(st) if st else None


def _call(be, entry, ap, t, window=None):
    """One forward entry point -> its status.  The split-KV workspace is NaN-filled: a piece that is not written shows."""
    lib = be.lib
    st = _stream(be, t)
    if entry == "fwd":
        rc = lib.tamd_attn_fwd(ctypes.byref(ap), st)
    elif entry == "fwd_window":
        rc = lib.tamd_attn_fwd_window(ctypes.byref(ap), window, st)
    else:
        n = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap))
        ws = torch.full((max(n, 16) // 4,), float("nan"), dtype=F32, device=t.device)
        if entry == "decode":
            rc = lib.tamd_attn_decode(ctypes.byref(ap), ws.data_ptr(), n, st)
        else:
            rc = lib.tamd_attn_decode_window(ctypes.byref(ap), window, ws.data_ptr(), n, st)
    _sync(t)
    return rc


def _fwd(env, entry, x, dtype, scale, causal, window=None, **kw):
    """-> (O, lse) as float64 CPU tensors; every guard checked."""
    b, sq, hq, d = x.q.shape
    out = Out(b, sq, hq, d, dtype, env.device)
    ap = _params(x.q, x.k, x.v, out.o, out.lse, dtype, scale, causal, **kw)
    if entry.startswith("decode"):  # (the merged lse bound of the module docstring counts on it)
        assert host_plan(b, sq, hq, x.k.shape[2], x.k.shape[1])[0] <= 8
    rc = _call(ops.backend(), entry, ap, x.q, window)
    assert rc == OK, (entry, rc)
    assert out.intact(), entry
    return out.o.cpu().double(), out.lse.cpu().double()


class Grads:
    """dq, dk, dv as views of sentinel-filled buffers with the layout of Operands (the ABI gives them the strides of q, k, v): one
    fused buffer at seq_q == seq_k, else dk | dv fused and dq with q's padded rows; dO and O with o's padded rows; the delta
    workspace guarded."""

    def __init__(self, x, o, lse, do, dtype, dev):
        b, sq, hq, d = x.q.shape
        sk, hkv = x.k.shape[1], x.k.shape[2]
        if sq == sk:
            self.g = Guarded((b, sk, (hq + 2 * hkv) * d), dtype, dev, 4 * (hq + 2 * hkv) * d)
            self.gq, dq, kv = None, self.g.t[:, :, :hq * d], self.g.t[:, :, hq * d:]
        else:
            self.gq = Guarded((b, sq, hq * d + 64), dtype, dev, 4 * (hq * d + 64))
            self.g = Guarded((b, sk, 2 * hkv * d), dtype, dev, 8 * hkv * d)
            dq, kv = self.gq.t[:, :, :hq * d], self.g.t
        self.dq = dq.unflatten(-1, (hq, d))
        self.dk = kv[:, :, :hkv * d].unflatten(-1, (hkv, d))
        self.dv = kv[:, :, hkv * d:].unflatten(-1, (hkv, d))
        assert self.dq.stride() == x.q.stride() and self.dk.stride() == x.k.stride() and self.dv.stride() == x.v.stride()
        self.io = torch.zeros(2, b, sq, hq * d + 16, dtype=dtype, device=dev)
        self.o = self.io[0, :, :, :hq * d].unflatten(-1, (hq, d))
        self.do = self.io[1, :, :, :hq * d].unflatten(-1, (hq, d))
        self.o.copy_(o), self.do.copy_(do)
        self.lse = lse.to(F32).to(dev).contiguous()
        self.dg = Guarded((2, b, hq, sq), F32, dev, 64)

    def intact(self):
        """Guards, and the gap columns of dq's padded rows."""
        return (self.g.intact() and self.dg.intact()
                and (self.gq is None or (self.gq.intact() and bool((self.gq.t[:, :, -64:] == SENT).all()))))

    def untouched(self):
        return self.g.untouched() and self.dg.untouched() and (self.gq is None or self.gq.untouched())


def _bwd(env, x, gr, dtype, scale, causal, rope=None, **kw):
    bp = _cabi.AttnBwdParams()
    bp.fwd = _params(x.q, x.k, x.v, gr.o, gr.lse, dtype, scale, causal, **kw)
    bp.dout, bp.dq, bp.dk, bp.dv, bp.delta = gr.do.data_ptr(), gr.dq.data_ptr(), gr.dk.data_ptr(), gr.dv.data_ptr(), gr.dg.t.data_ptr()
    be = ops.backend()
    rc = be.lib.tamd_attn_bwd(ctypes.byref(bp), _stream(be, x.q))
    _sync(x.q)
    assert rc == OK, rc
    assert gr.intact()
    return gr.dq.cpu().double(), gr.dk.cpu().double(), gr.dv.cpu().double(), gr.dg.t.cpu().double()


# ---- the host mask, from the header's formulas ------------------------------------------------------------------------------
def host_mask(b, sq, sk, causal, kv=None, planes=None, window=None, lens=None):
    """bool [b, sq, sk].  causal: k <= s + off, off = len_b - seq_q; key_valid; planes: q_start[b, s] <= k <= s (with plane 1:
    s <= k_end[b, k]); window: k >= s + off - window + 1 (and k <= s + off, also for one non-causal row);
    len_b = clamp(seq_k_dev[b], 0, seq_k)."""
    s = torch.arange(sq)[:, None]
    k = torch.arange(sk)[None, :]
    m = torch.zeros(b, sq, sk, dtype=torch.bool)
    for i in range(b):
        n = sk if lens is None else min(max(int(lens[i]), 0), sk)
        off = n - sq
        a = (k < n).expand(sq, sk).clone()
        if causal or window is not None:
            a &= k <= s + off
        if window is not None:
            a &= k >= s + off - window + 1
        if planes is not None:
            a &= (planes[0, i][:, None] <= k) & (k <= s) & (s <= planes[1, i][None, :])
        if kv is not None:
            a &= kv[i].bool()[None, :]
        m[i] = a
    return m


def h_window(b, s, w):
    """masking_utils.py:92-101 as the header quotes it: q_start = max(0, q - w + 1), k_end = min(seq - 1, k + w - 1)."""
    pos = torch.arange(s)
    return torch.stack(((pos - w + 1).clamp(min=0), (pos + w - 1).clamp(max=s - 1)))[:, None].expand(2, b, s).to(torch.int32).contiguous()


def h_ids(ids):
    """Sequence (or chunk) ids [b, s] -> first / last index of each token's run of equal ids."""
    b, s = ids.shape
    out = torch.zeros(2, b, s, dtype=torch.int32)
    for i in range(b):
        lo = 0
        for j in range(s + 1):
            if j == s or (j > 0 and ids[i, j] != ids[i, j - 1]):
                out[0, i, lo:j], out[1, i, lo:j] = lo, j - 1
                lo = j
    return out


def h_chunk(b, s, chunk, left):
    """masking_utils.py:104-113: (k - left[b]) // chunk == (q - left[b]) // chunk, floor division."""
    pos = torch.arange(s)[None, :]
    return h_ids(torch.div(pos - torch.tensor(left)[:, None], chunk, rounding_mode="floor"))


def h_and(a, b):
    return torch.stack((torch.maximum(a[0], b[0]), torch.minimum(a[1], b[1]))).contiguous()


# ---- Part A operands ----------------------------------------------------------------------------------------------------------
def codes(n, d):
    m = d // 2
    c = torch.zeros(n, d, dtype=torch.float64)
    i = torch.arange(n)
    c[i, i % m] = 1.0
    c[i, m + (i // m) % m] = 1.0
    return c


def code_tensor(b, n, h, d):
    """[b, n, h, d]: the code of the row index, columns rotated by b + h."""
    c = codes(n, d)
    return torch.stack([torch.stack([torch.roll(c, i + j, 1) for j in range(h)], 1) for i in range(b)])


def assert_decodable(sk, d):
    """The precondition: every key below seq_k has a code of exactly two bits that no other key has, so removing, adding or
    exchanging one key of a row changes n or one decoded count."""
    c = codes(sk, d)
    assert sk <= (d // 2) ** 2 and bool((c.sum(1) == 2).all())
    assert torch.unique(c, dim=0).shape[0] == sk


def visibility_operands(b, sq, sk, hq, hkv, d, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(b, sk, hkv, d, generator=g) * 3.0
    return Operands(torch.zeros(b, sq, hq, d), k, code_tensor(b, sk, hkv, d), dtype, dev)


def assert_visibility(o, lse, allow, hq, hkv, d, dtype, lse_ulps, what, weight=None, dscale=1.0):
    """o, lse float64 from the kernel; allow bool [b, sq, sk] (or [b, hq, sq, sk]); weight: a dropout keep mask [b, hq, sq, sk]
    that thins the counts but not n; dscale: the fp32 keep-scale."""
    b, sq = o.shape[0], o.shape[1]
    sk = allow.shape[-1]
    assert_decodable(sk, d)
    al = (allow[:, None].expand(b, hq, sq, sk) if allow.dim() == 3 else allow).double()
    n = al.sum(-1)                                                   # [b, hq, sq]
    v = code_tensor(b, sk, hkv, d).repeat_interleave(hq // hkv, 2)  # [b, sk, hq, d]
    want = torch.einsum("bhsk,bkhj->bshj", al if weight is None else al * weight.double(), v)
    empty = n == 0
    # lse: +inf on a row without a visible key, else ln n within lse_ulps fp32 ulp (module docstring)
    assert bool(torch.isposinf(lse[empty]).all()), what
    ln = torch.log(n.clamp_min(1.0))
    assert bool(torch.isfinite(lse[~empty]).all()), what
    got_n = torch.where(empty, torch.zeros_like(n), torch.exp(torch.where(empty, torch.zeros_like(lse), lse)).round())
    bad = torch.nonzero(got_n != n)
    assert bad.numel() == 0, f"{what}: visible-key count of (b, h, s) = {bad[0].tolist()}: got {got_n[tuple(bad[0])]} want {n[tuple(bad[0])]}"
    merged = lse_ulps > 3                                            # behind attn_combine_kernel: 11 U + 6 x 2^-23, else 3 U
    diff = torch.where(empty, torch.zeros_like(ln), (torch.where(empty, ln, lse) - ln).abs())
    bound = 11.0 * ulp(ln, F32) + 6.0 * 2.0 ** -23 * (n > 1) if merged else 3.0 * ulp(ln, F32)
    worst = (diff / ulp(ln, F32))[n > 1].max().item() if bool((n > 1).any()) else 0.0
    key = f"A lse {'merged' if merged else 'training'} in fp32 ulp of ln n[{NAME[dtype]}-{d}]"
    _LSE[key] = max(_LSE.get(key, 0.0), worst)
    record(GROUP, key, _LSE[key], 12.5 if merged else 3.0)
    print(f"{what}: lse worst {worst:.2f} fp32 ulp of ln n")
    assert bool((diff <= bound).all()), (what, worst)
    # counts: integers
    nn = n.permute(0, 2, 1)[..., None]                                # [b, sq, hq, 1]
    cnt = (o * nn / dscale).round()
    bad = torch.nonzero(cnt != want)
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} counts differ; first (b, s, h, j) = {bad[0].tolist()}: "
                              f"got {cnt[tuple(bad[0])]} want {want[tuple(bad[0])]}")
    # O itself: one ulp_T of round_T(count * dscale / n); exactly 0 on an empty row
    ref = rnd(want * dscale / nn.clamp_min(1.0), dtype)
    e = ((o - ref).abs() / ulp(ref, dtype))
    assert e.max().item() <= 1.0, (what, e.max().item())
    assert bool((o[empty.permute(0, 2, 1)] == 0).all()), what


def kv_pattern(b, sk, seed):
    """A different validity pattern per batch row; never all invalid."""
    g = torch.Generator().manual_seed(seed)
    kv = torch.rand(b, sk, generator=g) > 0.3
    kv[:, sk // 2] = True
    return kv.to(torch.uint8)


# ---- A1: training forward ---------------------------------------------------------------------------------------------------------
PAIRS = [(1, 1), (31, 63), (32, 64), (33, 65), (127, 128), (128, 130), (129, 257), (1, 257), (31, 128),
         (257, 130), (129, 65), (33, 1), (128, 63), (257, 257), (127, 64), (32, 130)]


@pytest.mark.parametrize("causal,mask", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["plain", "mask", "causal", "causal-mask"])
@pytest.mark.parametrize("dtype,d", TD)
def test_forward_visibility_at_wave_and_tile_edges(env, dtype, d, causal, mask):
    """The four instantiations of attn_fwd_launch without dropout, at the edges of 32 rows per wave, 128 per workgroup and 64
    keys per tile, both orders of seq_q and seq_k (causal with seq_q > seq_k: the rows above the diagonal see nothing).
    dropout_p = 1e-5 < 2^-16 on every other pair: make_args turns it into drop_thr = 0, the SAME instantiation, no key dropped."""
    b, hq, hkv = 2, 2, 1
    for i, (sq, sk) in enumerate(PAIRS):
        x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 7 + i)
        kv = kv_pattern(b, sk, i) if mask else None
        o, lse = _fwd(env, "fwd", x, dtype, d ** -0.5, causal, kv=None if kv is None else kv.to(env.device),
                      p=1e-5 if i % 2 else 0.0, seed=99)
        assert_visibility(o, lse, host_mask(b, sq, sk, causal, kv), hq, hkv, d, dtype, 3, f"fwd {sq}x{sk} c{causal} m{mask}")


# ---- A2: padding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dtype,d", TD)
def test_padding_holes_at_tile_boundaries(env, dtype, d, causal):
    b, sq, sk, hq, hkv = 6, 70, 200, 2, 2
    kv = torch.ones(b, sk, dtype=torch.uint8)
    kv[0, 63:65] = 0        # a hole exactly at keys 63 | 64
    kv[1, 64:128] = 0       # a whole invalid tile in the middle
    kv[2, :137] = 0         # left padding
    kv[3] = 0
    kv[3, 129] = 1          # one valid key
    kv[4] = 0               # none
    kv[5, 63] = 0           # the last key of a tile; and the last key of all
    kv[5, 199] = 0
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 21)
    o, lse = _fwd(env, "fwd", x, dtype, d ** -0.5, causal, kv=kv.to(env.device))
    assert_visibility(o, lse, host_mask(b, sq, sk, causal, kv), hq, hkv, d, dtype, 3, f"padding c{causal}")


# ---- A3: bound planes -----------------------------------------------------------------------------------------------------------------
def _ids_of(lengths):
    return torch.cat([torch.full((n,), i) for i, n in enumerate(lengths)])[None]


def plane_cases():
    """name -> (planes built here, the same planes from the ops helpers, key_valid or None)."""
    c = {}
    for name, lens in (("packed-1-63-64-72", [1, 63, 64, 72]), ("packed-40-5-105", [40, 5, 105])):
        ids = _ids_of(lens)
        c[name] = (h_ids(ids), ops.packed_q_start(ids), None)
    for w, s in ((1, 200), (9, 230), (64, 260), (65, 257), (150, 240)):  # (150 of 240, 64 of 260: tiles wholly left of a bound)
        c[f"window-{w}"] = (h_window(2, s, w), ops.sliding_window_q_start(2, s, w, "cpu"), None)
    for ch, left in ((48, [0, 13]), (100, [7, 0])):
        c[f"chunk-{ch}"] = (h_chunk(2, 210, ch, left), ops.chunked_q_start(2, 210, ch, left, "cpu"), None)
    kv = torch.ones(2, 250, dtype=torch.uint8)
    kv[0, :30] = 0
    kv[1, 120:129] = 0
    both = h_and(h_window(2, 250, 70), h_chunk(2, 250, 100, [30, 0]))
    c["window-chunk-padding"] = (both, ops.intersect_q_start(ops.sliding_window_q_start(2, 250, 70, "cpu"),
                                                             ops.chunked_q_start(2, 250, 100, [30, 0], "cpu")), kv)
    return c


PLANES = plane_cases()


def test_bound_plane_helpers_give_the_header_formulas(env):
    """The ops helpers on the backend's device against the planes built here (which the kernel tests use)."""
    dev = env.device
    theirs = {}
    for name, lens in (("packed-1-63-64-72", [1, 63, 64, 72]), ("packed-40-5-105", [40, 5, 105])):
        theirs[name] = ops.packed_q_start(_ids_of(lens).to(dev))
    for w, s in ((1, 200), (9, 230), (64, 260), (65, 257), (150, 240)):
        theirs[f"window-{w}"] = ops.sliding_window_q_start(2, s, w, dev)
    for ch, left in ((48, [0, 13]), (100, [7, 0])):
        theirs[f"chunk-{ch}"] = ops.chunked_q_start(2, 210, ch, left, dev)
    theirs["window-chunk-padding"] = ops.intersect_q_start(ops.sliding_window_q_start(2, 250, 70, dev),
                                                          ops.chunked_q_start(2, 250, 100, [30, 0], dev))
    assert set(theirs) == set(PLANES)
    for name, (mine, on_cpu, _) in PLANES.items():
        assert theirs[name].dtype == torch.int32 and torch.equal(mine, theirs[name].cpu()) and torch.equal(mine, on_cpu), name
    # a tile wholly left of a workgroup's first bound: rows 128 .. of window 64 over 260 start at key 65 >= 64
    assert int(PLANES["window-64"][0][0, 0, 128]) // 64 >= 1 and int(PLANES["window-150"][0][0, 0, 239]) // 64 >= 1


@pytest.mark.parametrize("name", list(PLANES))
@pytest.mark.parametrize("dtype,d", TD)
def test_bound_planes_visibility(env, dtype, d, name):
    planes, _, kv = PLANES[name]
    _, b, s = planes.shape
    hq, hkv = 2, 1
    x = visibility_operands(b, s, s, hq, hkv, d, dtype, env.device, 31)
    o, lse = _fwd(env, "fwd", x, dtype, d ** -0.5, 1, planes=planes.to(env.device), kv=None if kv is None else kv.to(env.device))
    assert_visibility(o, lse, host_mask(b, s, s, 1, kv, planes), hq, hkv, d, dtype, 3, name)


# ---- A4: dropout ----------------------------------------------------------------------------------------------------------------------
def drop_scale(p):
    """make_args: thr = floor(p * 65536); the keep-scale is the inverse of the effective keep probability, in fp32."""
    thr = int(p * 65536.0)
    return float(np.float32(65536.0 / (65536.0 - thr)))


@pytest.mark.parametrize("p,causal", [(0.1, 1), (0.5, 0), (0.5, 1), (0.1, 0)])
@pytest.mark.parametrize("dtype,d", TD)
def test_dropout_visibility(env, dtype, d, p, causal):
    """The two DROP instantiations: a kept key contributes 1 / (1 - p_eff), a dropped one 0; lse keeps the undropped count.  Odd
    seq_q and seq_k end the 2 x 2 hash blocks ragged; the seed from device memory gives the same bits."""
    b, sq, sk, hq, hkv, seed = 2, 131, 197, 2, 1, 4242
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 41)
    kv = kv_pattern(b, sk, 5) if causal else None
    kvd = None if kv is None else kv.to(env.device)
    o, lse = _fwd(env, "fwd", x, dtype, d ** -0.5, causal, kv=kvd, p=p, seed=seed)
    keep = ops.dropout_keep_mask(seed, b, hq, sq, sk, p).cpu()
    assert_visibility(o, lse, host_mask(b, sq, sk, causal, kv), hq, hkv, d, dtype, 3, f"dropout {p} c{causal}", weight=keep,
                      dscale=drop_scale(p))
    sd = torch.tensor([seed], dtype=torch.int64, device=env.device)
    o2, lse2 = _fwd(env, "fwd", x, dtype, d ** -0.5, causal, kv=kvd, p=p, seed=1, seed_dev=sd)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


# ---- A5: decode -----------------------------------------------------------------------------------------------------------------------
def host_plan(b, sq, hq, hkv, sk):
    """decode_plan of attention.hip restated: -> (splits, tiles per split, rows, heads)."""
    g = hq // hkv
    rows, heads = (g, hkv) if (sq == 1 and g > 1) else (sq, hq)
    nkt = -(-sk // 64)
    base = -(-rows // 128) * heads * b
    splits = max(1, min(-(-768 // base), nkt, 256))
    tps = -(-nkt // splits)
    return -(-nkt // tps), tps, rows, heads


def assert_plan(x, dtype, splits, tps):
    b, sq, hq, d = x.q.shape
    sk, hkv = x.k.shape[1], x.k.shape[2]
    s, t, rows, heads = host_plan(b, sq, hq, hkv, sk)
    assert (s, t) == (splits, tps), (s, t)
    ap = _params(x.q, x.k, x.v, x.q, x.q, dtype, 1.0, 0)
    assert ops.backend().lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap)) == s * b * rows * heads * (d + 1) * 4


DECODE = [  # b, sq, hq, hkv, sk, causal, (splits, tiles per split)
    (2, 1, 4, 4, 300, 0, (5, 1)),     # group 1; one tile per split; 96 splits asked of 5 tiles
    (2, 1, 4, 2, 300, 1, (5, 1)),     # group 2: the heads become rows
    (3, 1, 8, 2, 129, 0, (3, 1)),     # group 4
    (1, 5, 2, 1, 257, 1, (5, 1)),
    (1, 5, 2, 1, 257, 0, (5, 1)),
    (2, 33, 2, 2, 130, 1, (3, 1)),
    (2, 33, 2, 1, 130, 0, (3, 1)),
]


@pytest.mark.parametrize("case", DECODE, ids=lambda c: "-".join(map(str, c[:6])))
@pytest.mark.parametrize("dtype,d", TD)
def test_decode_visibility(env, dtype, d, case):
    b, sq, hq, hkv, sk, causal, plan = case
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 51)
    assert_plan(x, dtype, *plan)
    kv = kv_pattern(b, sk, 9) if (hq + sq) % 2 else None
    o, lse = _fwd(env, "decode", x, dtype, d ** -0.5, causal, kv=None if kv is None else kv.to(env.device))
    assert_visibility(o, lse, host_mask(b, sq, sk, causal, kv), hq, hkv, d, dtype, 16, f"decode {case}")


@pytest.mark.parametrize("dtype,d", TD)
def test_decode_several_tiles_per_split(env, dtype, d):
    """8 x 32 heads x 1 query tile = 256 workgroups before the split: 3 splits of 3, 3 and 1 of the 7 key tiles -- at least two
    tiles per split, a ragged last split whose last tile has 16 keys (4 KV heads: K and V are 1.6 M elements at head_dim 128)."""
    b, sq, hq, hkv, sk = 8, 5, 32, 4, 400
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 53)
    assert_plan(x, dtype, 3, 3)
    o, lse = _fwd(env, "decode", x, dtype, d ** -0.5, 1)
    assert_visibility(o, lse, host_mask(b, sq, sk, 1), hq, hkv, d, dtype, 16, "decode 3 tiles per split")


@pytest.mark.parametrize("sq,hq,hkv,causal", [(1, 4, 2, 1), (5, 2, 2, 1), (1, 2, 2, 0)])
@pytest.mark.parametrize("dtype,d", TD)
def test_decode_key_counts_from_device_memory(env, dtype, d, sq, hq, hkv, causal):
    """seq_k_dev = [0, 1, 63, 64, 65, seq_k, seq_k + 7, -3]; the slots the header declares unread hold NaN."""
    sk = 130
    counts = [0, 1, 63, 64, 65, sk, sk + 7, -3]
    b = len(counts)
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 57)
    for i, c in enumerate(counts):
        n = min(max(c, 0), sk)
        x.k[i, n:] = float("nan")
        x.v[i, n:] = float("nan")
    cnt = torch.tensor(counts, dtype=torch.int32, device=env.device)
    o, lse = _fwd(env, "decode", x, dtype, d ** -0.5, causal, counts=cnt)
    assert_visibility(o, lse, host_mask(b, sq, sk, causal, lens=counts), hq, hkv, d, dtype, 16, f"seq_k_dev sq{sq}")


# ---- A6: the window entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sq,sk", [(1, 70), (1, 200), (1, 330), (8, 70), (8, 200), (8, 330), (70, 70), (70, 200), (70, 330)])
@pytest.mark.parametrize("dtype,d", TD)
def test_window_entry_points_visibility(env, dtype, d, sq, sk):
    b, hq, hkv = 2, 4, 2
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 61)
    kv = kv_pattern(b, sk, 11).to(env.device)
    for i, w in enumerate((1, 63, 64, 65, sk - 1, sk, sk + 5)):
        for entry in ("fwd_window", "decode_window"):
            m = kv if (i + (entry == "fwd_window")) % 2 else None
            causal = 0 if (sq == 1 and i % 2) else 1
            o, lse = _fwd(env, entry, x, dtype, d ** -0.5, causal, window=w, kv=m)
            assert_visibility(o, lse, host_mask(b, sq, sk, causal, None if m is None else m.cpu(), window=w), hq, hkv, d, dtype,
                              3 if entry == "fwd_window" else 16, f"{entry} {sq}x{sk} w{w}")


def random_operands(b, sq, sk, hq, hkv, d, dtype, dev, seed, spike=False):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, hq, d, generator=g)
    k = torch.randn(b, sk, hkv, d, generator=g)
    v = torch.randn(b, sk, hkv, d, generator=g)
    if spike:
        k[:, sk - 8:] *= 6.0  # scores late in the row exceed the running maximum by more than 2^6: the deferred rescale fires
    return Operands(q, k, v, dtype, dev)


@pytest.mark.parametrize("dtype,d", TD)
def test_window_entry_points_have_the_bits_the_header_promises(env, dtype, d):
    """Random operands.  seq_q == seq_k: tamd_attn_fwd_window == tamd_attn_fwd under the same window's planes; window >= seq_k:
    both entry points == the unwindowed ones."""
    b, s, hq, hkv = 2, 200, 2, 1
    x = random_operands(b, s, s, hq, hkv, d, dtype, env.device, 63)
    kv = kv_pattern(b, s, 13).to(env.device)
    sc = d ** -0.5
    for w in (1, 64, 65, 150):
        for m in (None, kv):
            a = _fwd(env, "fwd_window", x, dtype, sc, 1, window=w, kv=m)
            r = _fwd(env, "fwd", x, dtype, sc, 1, planes=h_window(b, s, w).to(env.device), kv=m)
            assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1]), w
    for sq in (1, 8):
        y = random_operands(b, sq, 200, 4, 2, d, dtype, env.device, 65)
        for w in (200, 205):
            for m in (None, kv):
                for entry, plain in (("fwd_window", "fwd"), ("decode_window", "decode")):
                    a = _fwd(env, entry, y, dtype, sc, 1, window=w, kv=m)
                    r = _fwd(env, plain, y, dtype, sc, 1, kv=m)
                    assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1]), (sq, w, entry)


# ---- A7: result codes -----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(env):
    """Every TAMD_E_ARG / TAMD_E_SHAPE case of the header's attention section: the status, and not one output element."""
    dtype, d, dev = BF16, 64, env.device
    be = ops.backend()
    x = random_operands(2, 8, 8, 2, 1, d, dtype, dev, 71)
    y = random_operands(2, 4, 8, 2, 1, d, dtype, dev, 72)   # seq_q < seq_k
    z = random_operands(2, 8, 4, 2, 1, d, dtype, dev, 73)   # seq_q > seq_k
    planes = h_window(2, 8, 3).to(dev)
    cnt = torch.tensor([3, 8], dtype=torch.int32, device=dev)

    def refused(entry, ops_, want, window=None, edit=None, **kw):
        out = Out(*ops_.q.shape, dtype, dev)
        ap = _params(ops_.q, ops_.k, ops_.v, out.o, out.lse, dtype, 0.125, kw.pop("causal", 1), **kw)
        if edit:
            edit(ap)
        assert _call(be, entry, ap, ops_.q, window) == want, (entry, kw, window)
        assert out.untouched(), (entry, kw, window)
        return out, ap

    def setf(**f):
        def e(ap):
            for k_, v_ in f.items():
                setattr(ap, k_, v_)
        return e

    for entry in ("fwd", "decode"):
        refused(entry, x, E_SHAPE, edit=setf(head_dim=96))
        refused(entry, x, E_SHAPE, edit=setf(heads_kv=3))          # heads_q % heads_kv
        refused(entry, x, E_SHAPE, edit=setf(seq_k=0))
        refused(entry, x, E_ARG, p=1.0)
        refused(entry, x, E_ARG, p=-0.1)
        refused(entry, x, E_ARG, planes=planes, causal=0)          # planes need causal ...
        refused(entry, y, E_ARG, planes=planes)                    # ... and seq_q == seq_k
        refused(entry, x, E_ARG, edit=setf(q_stride_s=56))         # head_dim <= stride_s
        refused(entry, x, E_ARG, edit=setf(k_stride_s=(1 << 24) + 8))
    refused("fwd", x, E_ARG, counts=cnt)                           # seq_k_dev: tamd_attn_decode only
    refused("decode", x, E_ARG, p=0.1)
    refused("decode", x, E_ARG, planes=planes)
    for entry in ("fwd_window", "decode_window"):
        refused(entry, x, E_ARG, window=0)
        refused(entry, z, E_ARG, window=4)                         # seq_q > seq_k
        refused(entry, x, E_ARG, window=4, causal=0)               # seq_q > 1 without causal
        refused(entry, x, E_ARG, window=4, planes=planes)
        refused(entry, x, E_ARG, window=4, p=0.1)
        refused(entry, x, E_ARG, window=4, counts=cnt)
        refused(entry, x, E_SHAPE, window=4, edit=setf(head_dim=32))
    # the backward: seq_k_dev, and the rotary epilogue's conditions (head_dim 128, seq_q == seq_k, rope_cos_batch 1 or batch)
    o0, l0 = _fwd(env, "fwd", x, dtype, 0.125, 1)
    x128 = random_operands(2, 8, 8, 2, 1, 128, dtype, dev, 74)
    y128 = random_operands(2, 4, 8, 2, 1, 128, dtype, dev, 75)
    for what in ("counts", "rope-d64", "shape", "rope-rect", "rope-batch"):
        xx = {"rope-rect": y128, "rope-batch": x128}.get(what, x)
        o_in = o0 if xx is x else torch.zeros(xx.q.shape, dtype=torch.float64)
        l_in = l0 if xx is x else torch.zeros(2, 2, xx.q.shape[1], dtype=torch.float64)
        gr = Grads(xx, o_in, l_in, torch.ones_like(o_in), dtype, dev)
        bp = _cabi.AttnBwdParams()
        bp.fwd = _params(xx.q, xx.k, xx.v, gr.o, gr.lse, dtype, 0.125, 1, counts=cnt if what == "counts" else None)
        bp.dout, bp.dq, bp.dk, bp.dv, bp.delta = gr.do.data_ptr(), gr.dq.data_ptr(), gr.dk.data_ptr(), gr.dv.data_ptr(), gr.dg.t.data_ptr()
        if what.startswith("rope"):  # head_dim 64; seq_q != seq_k; rope_cos_batch neither 1 nor batch
            cs = torch.ones(3, 8, 128, dtype=dtype, device=dev)
            bp.rope_cos, bp.rope_sin, bp.rope_cos_batch = cs.data_ptr(), cs.data_ptr(), 3 if what == "rope-batch" else 1
        if what == "shape":
            bp.fwd.heads_kv = 3
        assert be.lib.tamd_attn_bwd(ctypes.byref(bp), _stream(be, xx.q)) == (E_SHAPE if what == "shape" else E_ARG), what
        _sync(xx.q)
        assert gr.untouched(), what


# ---- the float64 model (reference, and the chains with the kernels' documented roundings) -------------------------------------------
class Case:
    """One problem in float64 on the STORED operands.  allow [b, hq, sq, sk] bool; drop: keep * keep-scale or None."""

    def __init__(self, x, dtype, scale, allow, drop=None, dscale=1.0, prescaled=False):
        self.dtype, self.pre, self.drop, self.dscale = dtype, prescaled, drop, dscale
        self.q, self.k, self.v = x.q.cpu().double(), x.k.cpu().double(), x.v.cpu().double()
        self.g = self.q.shape[2] // self.k.shape[2]
        self.scale = float(np.float32(scale))
        self.c32 = float(np.float32(scale) * np.float32(1.44269504088896340736))  # make_args: a.scale_log2, an fp32 product
        self.allow = allow
        self.kx, self.vx = self.k.repeat_interleave(self.g, 2), self.v.repeat_interleave(self.g, 2)

    def scores2(self, how):
        """Scores in the exp2 domain.  how: None = exact; "q" = round_T(fp32(q * c)) (scale_frag on the resident Q fragments:
        attention_fwd_kernel.inc `qf[ks] = scale_frag<T>(qf[ks], a.scale_log2, !a.q_prescaled)`, the same line in
        attention_bwd_dq_kernel.inc); "k" = the factor rides on K (attention_bwd_dkdv.hip `kf[ks] = scale_frag<T, true>(...)`)."""
        q, k = self.q, self.kx
        if self.pre:
            pass                                           # q carries the factor: no operand is scaled or rounded again
        elif how is None:
            q = q * (self.scale * LOG2E)
        elif how == "q":
            q = rnd((q * self.c32).float().double(), self.dtype)
        else:
            k = rnd((k * self.c32).float().double(), self.dtype)
        s = torch.einsum("bshd,bkhd->bhsk", q, k)
        return s.masked_fill(~self.allow, float("-inf"))

    def forward(self, how=None):
        """-> O [b, sq, hq, d], lse [b, hq, sq], P [b, hq, sq, sk] (normalised, before dropout)."""
        s2 = self.scores2(how)
        m = s2.max(-1, keepdim=True).values
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp2(s2 - m)
        l = p.sum(-1, keepdim=True)
        lse = torch.where(l > 0, (m + torch.log2(l.clamp_min(1e-300))) * LN2, torch.full_like(l, float("inf")))[..., 0]
        # forward kernel: `pack2<T>(p[...])` -- the probabilities that multiply V are rounded to T, the row sum is not
        pv = (rnd(p, self.dtype) if how else p) / l.clamp_min(1e-300)
        if self.drop is not None:
            pv = pv * self.drop
        return torch.einsum("bhsk,bkhd->bshd", pv, self.vx), lse, p / l.clamp_min(1e-300)

    def backward(self, o_in, lse_in, do, how=None):
        """Gradients as functions of the stored o, lse, dO.  how: None, "dq" (the dQ kernel) or "dkdv"."""
        s2 = self.scores2(None if how is None else ("q" if how == "dq" else "k"))
        p = torch.exp2(s2 - (lse_in * LOG2E)[..., None])      # masked: exp2(-inf) = 0; lse = +inf: 0
        p = torch.where(self.allow, p, torch.zeros_like(p))
        dp = torch.einsum("bshd,bkhd->bhsk", do, self.vx)
        delta = (do * o_in).sum(-1).permute(0, 2, 1)         # [b, hq, sq]
        if self.drop is not None:
            dp = dp * self.drop
        ds = p * (dp - delta[..., None])
        pd = p if self.drop is None else p * (self.drop != 0)
        if how:
            # both backward kernels round dS and P to T as the MFMA operands: attention_bwd_dq_kernel.inc
            # `pack_c_to_b<T>(ds, &dsf[sub * 2])`, attention_bwd_dkdv.hip `pf[op][w] = pack2<T>(p[0], p[1])`,
            # `dsf[op][w] = pack2<T>(ds[0], ds[1])`; dV's keep-scale multiplies the finished rows (store_rows_via_lds)
            ds, pd = rnd(ds, self.dtype), rnd(pd, self.dtype)
        b, hq, sq, sk = p.shape
        hkv = hq // self.g
        dq = self.scale * torch.einsum("bhsk,bkhd->bshd", ds, self.kx)
        kmul = self.scale / (self.scale * LOG2E if how is None else self.c32) if self.pre else self.scale
        dk = kmul * torch.einsum("bhsk,bshd->bkhd", ds, self.q).reshape(b, sk, hkv, self.g, -1).sum(3)
        dv = self.dscale * torch.einsum("bhsk,bshd->bkhd", pd, do).reshape(b, sk, hkv, self.g, -1).sum(3)
        return dq, dk, dv, delta, p, ds, dp

    # ---- `s`: what fp32 arithmetic and the operand roundings may add in front of the output rounding.  Float64 reference
    # quantities only.  u = 2^-(mant + 1): the relative half ulp of T.
    def eps_scores(self, lse):
        """Per (s, k), the exp2-domain score error: the half ulp of T on every product of the scaled operand (0 when q arrives
        pre-scaled), the fp32 accumulation over head_dim, and the fp32 rounding of the chain's start (-m or -lse log2 e)."""
        u = 2.0 ** -(MANT[self.dtype] + 1)
        c = 1.0 if self.pre else self.scale * LOG2E
        a = c * torch.einsum("bshd,bkhd->bhsk", self.q.abs(), self.kx.abs())
        d = self.q.shape[-1]
        fl = torch.where(torch.isfinite(lse), lse.abs(), torch.zeros_like(lse))[..., None]
        return (0.0 if self.pre else u) * a + 2.0 ** -23 * (d * a + fl * LOG2E + 8.0)

    def s_forward(self, o, lse, p):
        u = 2.0 ** -(MANT[self.dtype] + 1)
        rel = LN2 * self.eps_scores(lse) + 2.0 ** -22          # relative error of one probability (v_exp_f32: one ulp)
        rel = torch.where(self.allow, rel, torch.zeros_like(rel))
        w = p if self.drop is None else p * self.drop
        n = self.allow.sum(-1).double().permute(0, 2, 1)[..., None]
        pv = torch.einsum("bhsk,bkhd->bshd", w, self.vx.abs())
        # the rounding of P: u * sum P |V|;  a score error moves O_j by P_k |D_k V_kj - O_j| per unit (softmax derivative);
        # the fp32 sums: 2^-23 x (keys + merge / normalisation steps) x the absolute sum
        dev = torch.einsum("bhsk,bkhd->bshd", w * rel, self.vx.abs()) + torch.einsum("bhsk->bsh", p * rel)[..., None] * o.abs()
        s_o = u * pv + dev + 2.0 ** -23 * (n + 16.0) * pv
        nn = self.allow.sum(-1).double()
        fl = torch.where(torch.isfinite(lse), lse.abs(), torch.zeros_like(lse))
        s_l = rel.max(-1).values + 2.0 ** -23 * (nn + 16.0) * (fl + 8.0)  # the largest score error of the row, as it is
        return s_o, s_l

    def s_backward(self, o_in, lse_in, do, p, ds, dp):
        u = 2.0 ** -(MANT[self.dtype] + 1)
        d = self.q.shape[-1]
        rel = LN2 * self.eps_scores(lse_in) + 2.0 ** -22
        b, hq, sq, sk = p.shape
        hkv = hq // self.g
        keep = 1.0 if self.drop is None else (self.drop != 0).double()
        grp = lambda t: t.reshape(b, sk, hkv, self.g, -1).sum(3)  # noqa: E731
        # dV = sum P~ dO: P's relative error and its rounding to T; the fp32 sum over the queries of the group
        pa = torch.einsum("bhsk,bshd->bkhd", p * keep * (u + rel), do.abs())
        nq = self.allow.sum(2).double().reshape(b, hkv, self.g, sk).sum(2).permute(0, 2, 1)[..., None]
        s_dv = self.dscale * (grp(pa) + 2.0 ** -23 * (nq + 8.0) * grp(torch.einsum("bhsk,bshd->bkhd", p * keep, do.abs())))
        # dS = P (dP D - delta), rounded to T: P's relative error, the rounding, and the fp32 sums of dP and delta over head_dim
        adp = torch.einsum("bshd,bkhd->bhsk", do.abs(), self.vx.abs()) * (1.0 if self.drop is None else self.drop)
        adl = (do * o_in).abs().sum(-1).permute(0, 2, 1)[..., None]
        e_ds = ds.abs() * (rel + u) + p * 2.0 ** -23 * (d + 4.0) * (adp + adl)
        nk = self.allow.sum(-1).double().permute(0, 2, 1)[..., None]
        s_dq = self.scale * (torch.einsum("bhsk,bkhd->bshd", e_ds, self.kx.abs())
                             + 2.0 ** -23 * (nk + 8.0) * torch.einsum("bhsk,bkhd->bshd", ds.abs(), self.kx.abs()))
        kmul = 1.0 / LOG2E if self.pre else self.scale
        s_dk = kmul * (grp(torch.einsum("bhsk,bshd->bkhd", e_ds, self.q.abs()))
                       + 2.0 ** -23 * (nq + 8.0) * grp(torch.einsum("bhsk,bshd->bkhd", ds.abs(), self.q.abs())))
        return s_dq, s_dk, s_dv


# ---- Part A, backward ----------------------------------------------------------------------------------------------------------------
def _bwd_visibility(env, dtype, d, b, sq, sk, hq, hkv, causal, kv=None, planes=None, p=0.0, what=""):
    dev, seed = env.device, 808
    x = visibility_operands(b, sq, sk, hq, hkv, d, dtype, dev, 81)
    allow = host_mask(b, sq, sk, causal, kv, planes)[:, None].expand(b, hq, sq, sk)
    n = allow.sum(-1).double()                                       # [b, hq, sq]
    # dO: the code of the QUERY index, per head, times 2^floor(log2 n(s)): every term P~(s) dO lies in (1/2, 1] (x keep-scale)
    # (per head and batch row the code of a shifted query index, not rotated columns: the first code bit of every head stays in
    # columns [0, d/2), clear of the second bits, whose columns add up a whole block of d/2 queries)
    cq = codes(sq, d)
    do = torch.stack([torch.stack([cq[(torch.arange(sq) + 7 * h + 3 * i) % sq] for h in range(hq)], 1) for i in range(b)])
    do = do * torch.exp2(torch.floor(torch.log2(n.clamp_min(1.0)))).permute(0, 2, 1)[..., None]
    drop, dsc = None, 1.0
    if p:
        dsc = drop_scale(p)
        drop = ops.dropout_keep_mask(seed, b, hq, sq, sk, p).cpu().double() * dsc
    case = Case(x, dtype, d ** -0.5, allow, drop, dsc)
    o64, lse64, _ = case.forward()
    o_in, lse_in = rnd(o64, dtype), lse64.float().double()
    gr = Grads(x, o_in, lse_in, do, dtype, dev)
    kw = dict(kv=None if kv is None else kv.to(dev), planes=None if planes is None else planes.to(dev), p=p, seed=seed)
    dq, dk, dv, stats = _bwd(env, x, gr, dtype, d ** -0.5, causal, **kw)
    ref = case.backward(o_in, lse_in, do)
    chain = case.backward(o_in, lse_in, do, "dkdv")
    _, _, s_dv = case.s_backward(o_in, lse_in, do, ref[4], ref[5], ref[6])
    check(f"A dV {what}", dv, ref[2], s_dv, dtype, chain=rnd(chain[2], dtype), group=GROUP)
    # the host-side condition: dropping one visible (s, k) pair moves dV[k, first code bit of s] by one whole term P~(s) dO,
    # at least 1/2: more than the gate at every such element
    unit = ulp(ref[2], dtype) + s_dv
    own = ((rnd(chain[2], dtype) - ref[2]).abs() / unit).max().item()
    first = unit[..., :d // 2].max().item()
    assert 0.5 > 2.0 * max(0.5, own) * first, (what, own, first)
    # dK = scale dS^T Q with Q = 0: exactly zero
    assert bool((dk == 0).all()), what
    # the statistics rows: plane 1 = -lse * log2(e), one fp32 product with a constant that is within 0.16 ulp of log2(e):
    # within one fp32 ulp; a row without a visible key (lse = +inf): -inf
    want = -lse_in * LOG2E
    fin = torch.isfinite(want)
    assert bool((stats[1][~fin] == want[~fin]).all()), what
    e = ((stats[1][fin] - want[fin]).abs() / ulp(want[fin], F32)).max().item() if fin.any() else 0.0
    assert e <= 1.0, (what, e)
    # plane 0 = -rowsum(dO * O): two non-zero products per row here -- one fp32 ulp
    e0 = ((stats[0] + ref[3]).abs() / ulp(ref[3], F32)).max().item()
    assert e0 <= 1.0, (what, e0)
    assert bool(torch.isfinite(dq).all()), what


@pytest.mark.parametrize("causal,mask", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["plain", "mask", "causal", "causal-mask"])
@pytest.mark.parametrize("dtype,d", TD)
def test_backward_visibility(env, dtype, d, causal, mask):
    for (sq, sk) in ((129, 65), (65, 130)):
        _bwd_visibility(env, dtype, d, 2, sq, sk, 2, 1, causal, kv_pattern(2, sk, 3) if mask else None, what=f"{sq}x{sk} c{causal} m{mask}")


@pytest.mark.parametrize("name", ["packed-1-63-64-72", "window-65", "chunk-48", "window-chunk-padding"])
@pytest.mark.parametrize("dtype,d", TD)
def test_backward_visibility_bound_planes(env, dtype, d, name):
    planes, _, kv = PLANES[name]
    _bwd_visibility(env, dtype, d, planes.shape[1], planes.shape[2], planes.shape[2], 2, 1, 1, kv, planes, what=name)


@pytest.mark.parametrize("p,causal,packed", [(0.1, 1, 0), (0.5, 0, 0), (0.1, 1, 1)])
@pytest.mark.parametrize("dtype,d", TD)
def test_backward_visibility_dropout(env, dtype, d, p, causal, packed):
    planes = PLANES["packed-40-5-105"][0] if packed else None
    s = 150 if packed else 131
    _bwd_visibility(env, dtype, d, 1 if packed else 2, s, s if packed else 97, 2, 1, causal, planes=planes, p=p, what=f"drop {p} c{causal} pk{packed}")


# ---- Part B: random operands ------------------------------------------------------------------------------------------------------------
RANDOM = {  # name: b, sq, sk, hq, hkv, causal, mask, p, planes, prescaled, spike
    "causal-g4": (2, 129, 129, 4, 1, 1, 0, 0.0, None, 0, 0),
    "mask-g2": (2, 65, 127, 2, 1, 0, 1, 0.0, None, 0, 0),
    "causal-mask-g1": (1, 128, 63, 2, 2, 1, 1, 0.0, None, 0, 0),
    "plain-spike": (1, 64, 128, 2, 2, 0, 0, 0.0, None, 0, 1),
    "causal-drop": (2, 63, 65, 2, 1, 1, 1, 0.1, None, 0, 0),
    "plain-drop": (1, 127, 129, 2, 2, 0, 0, 0.5, None, 0, 0),
    "packed": (1, 150, 150, 2, 1, 1, 0, 0.0, "packed-40-5-105", 0, 0),
    "packed-drop": (1, 200, 200, 2, 2, 1, 0, 0.1, "packed-1-63-64-72", 0, 0),
    "prescaled": (1, 72, 72, 2, 2, 1, 0, 0.0, None, 1, 0),
}


@pytest.mark.parametrize("name", list(RANDOM))
@pytest.mark.parametrize("dtype,d", TD)
def test_random_operands_forward_and_backward(env, dtype, d, name):
    b, sq, sk, hq, hkv, causal, mask, p, pl, pre, spike = RANDOM[name]
    dev, seed, scale = env.device, 909, d ** -0.5
    x = random_operands(b, sq, sk, hq, hkv, d, dtype, dev, 91, spike)
    if pre:  # the producer's one rounding of q * scale * log2(e)
        x.q.copy_((x.q.float() * (scale * LOG2E)).to(dtype))
    kv = kv_pattern(b, sk, 17) if mask else None
    planes = PLANES[pl][0] if pl else None
    allow = host_mask(b, sq, sk, causal, kv, planes)[:, None].expand(b, hq, sq, sk)
    drop, dsc = None, 1.0
    if p:
        dsc = drop_scale(p)
        drop = ops.dropout_keep_mask(seed, b, hq, sq, sk, p).cpu().double() * dsc
    case = Case(x, dtype, scale, allow, drop, dsc, bool(pre))
    kw = dict(kv=None if kv is None else kv.to(dev), planes=None if planes is None else planes.to(dev), p=p, seed=seed, prescaled=pre)
    o, lse = _fwd(env, "fwd", x, dtype, scale, causal, **kw)
    o64, lse64, p64 = case.forward()
    oc, lc, _ = case.forward("q")
    s_o, s_l = case.s_forward(o64, lse64, p64)
    check(f"O {name}", o, o64, s_o, dtype, chain=rnd(oc, dtype), group=GROUP)
    check_lse(f"lse {name}", lse, lse64, s_l, lc.float().double())
    # the backward on the reference's own o and lse, stored as the forward stores them: independent of the forward kernel
    g = torch.Generator().manual_seed(92)
    do = rnd(torch.randn(b, sq, hq, d, generator=g).double(), dtype)
    o_in, lse_in = rnd(o64, dtype), lse64.float().double()
    gr = Grads(x, o_in, lse_in, do, dtype, dev)
    dq, dk, dv, stats = _bwd(env, x, gr, dtype, scale, causal, **kw)
    ref = case.backward(o_in, lse_in, do)
    cq, ckv = case.backward(o_in, lse_in, do, "dq"), case.backward(o_in, lse_in, do, "dkdv")
    s_dq, s_dk, s_dv = case.s_backward(o_in, lse_in, do, ref[4], ref[5], ref[6])
    check(f"dq {name}", dq, ref[0], s_dq, dtype, chain=rnd(cq[0], dtype), group=GROUP)
    check(f"dk {name}", dk, ref[1], s_dk, dtype, chain=rnd(ckv[1], dtype), group=GROUP)
    check(f"dv {name}", dv, ref[2], s_dv, dtype, chain=rnd(ckv[2], dtype), group=GROUP)
    # delta plane 0 = -rowsum(dO * O): an fp32 sum of head_dim exact products
    s_d = 2.0 ** -23 * d * (do * o_in).abs().sum(-1).permute(0, 2, 1)
    check(f"delta {name}", -stats[0], ref[3], s_d, F32, group=GROUP)


def check_lse(name, lse, ref, s, chain):
    """+inf exactly where the reference has it (a row without a visible key); every other element within the gate."""
    inf = torch.isinf(ref)
    assert torch.equal(torch.isposinf(lse), inf), name
    check(name, lse[~inf], ref[~inf], s[~inf], F32, chain=chain[~inf], group=GROUP)


DECODE_RANDOM = [  # entry, b, sq, sk, hq, hkv, causal, window
    ("decode", 2, 1, 300, 4, 2, 0, None), ("decode", 1, 5, 257, 2, 1, 1, None), ("decode", 2, 1, 130, 8, 2, 1, None),
    ("decode", 8, 5, 257, 32, 4, 1, None),   # 3 splits of 2, 2, 1 tiles (asserted)
    ("fwd_window", 1, 70, 200, 2, 1, 1, 65), ("decode_window", 2, 1, 200, 4, 2, 0, 64), ("decode_window", 1, 8, 330, 2, 2, 1, 150),
]


@pytest.mark.parametrize("case", DECODE_RANDOM, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dtype,d", TD)
def test_random_operands_decode_and_window(env, dtype, d, case):
    entry, b, sq, sk, hq, hkv, causal, w = case
    x = random_operands(b, sq, sk, hq, hkv, d, dtype, env.device, 95, spike=True)
    if b == 8:
        assert_plan(x, dtype, 3, 2)
    kv = kv_pattern(b, sk, 19)
    allow = host_mask(b, sq, sk, causal, kv, window=w)[:, None].expand(b, hq, sq, sk)
    c = Case(x, dtype, d ** -0.5, allow)
    o, lse = _fwd(env, entry, x, dtype, d ** -0.5, causal, window=w, kv=kv.to(env.device))
    o64, lse64, p64 = c.forward()
    oc, lc, _ = c.forward("q")
    s_o, s_l = c.s_forward(o64, lse64, p64)
    check(f"O {entry}", o, o64, s_o, dtype, chain=rnd(oc, dtype), group=GROUP)
    check_lse(f"lse {entry}", lse, lse64, s_l, lc.float().double())


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_rope_epilogue_has_the_bits_of_the_unfused_rotation(env, dtype):
    """rope_cos / rope_sin at head_dim 128, a ragged length: dq and dk bit-identical to tamd_rope_inplace(conj) applied to the
    plain gradients (include/tamd.h), dv untouched by it; the gradients live in a sentinel-filled fused buffer."""
    b, s, hq, hkv, d, dev = 2, 75, 2, 1, 128, env.device
    x = random_operands(b, s, s, hq, hkv, d, dtype, dev, 97)
    o, lse = ops.raw_attn_fwd(x.q, x.k, x.v, d ** -0.5, True)
    g = torch.Generator().manual_seed(98)
    do = torch.randn(b, s, hq, d, generator=g).to(dtype).to(dev)
    w = (hq + 2 * hkv) * d
    for cb in (1, b):
        ang = torch.rand(cb, s, d // 2, generator=g) * 6.28
        cos = torch.cat([ang.cos(), ang.cos()], -1).to(dtype).to(dev)
        sin = torch.cat([ang.sin(), ang.sin()], -1).to(dtype).to(dev)
        if cb == 1:
            cos, sin = cos[0], sin[0]
        bufs = []
        for rope in (None, (cos, sin)):
            gb = Guarded((b * s, w), dtype, dev, 4 * w)
            t = gb.t.view(b, s, w)
            dq, dk, dv = (t[..., :hq * d].unflatten(-1, (hq, d)), t[..., hq * d:(hq + hkv) * d].unflatten(-1, (hkv, d)),
                          t[..., (hq + hkv) * d:].unflatten(-1, (hkv, d)))
            ops.raw_attn_bwd(x.q, x.k, x.v, o, lse, do, d ** -0.5, True, dq=dq, dk=dk, dv=dv, rope=rope)
            if rope is None:
                ops.raw_rope_(gb.t, cos, sin, s, hq + hkv, d, conj=True)
            _sync(gb.t)
            assert gb.intact() and not bool((gb.t == SENT).all(-1).any())
            bufs.append(gb.t.cpu())
        assert torch.equal(bufs[0], bufs[1]), cb
