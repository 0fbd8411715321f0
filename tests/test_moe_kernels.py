"""The sparse mixture-of-experts kernels, element by element: the routing plan (tamd_moe_route), gather / combine /
combine-backward, the routed GEMM in its three modes (tamd_gemm_routed) and the differentiable op torch.ops.tamd.moe_experts,
on the SAME small shapes under the CPU execution model (`emu`) and on the MI355X (`hip`).

Geometry.  Case 1: E = 6 experts, top-2, 322 tokens whose pairs give per-expert counts of exactly [0, 1, 64, 65, 256, 258]
(an expert without rows, one row, a whole segment, one row past a segment, a whole row tile, two rows past a row tile), no
token naming an expert twice, tokens permuted by a fixed permutation.  Case 2: E = 128, top-8, 300 tokens, random ids:
2400 pairs, more than one 1024-pair chunk of the counting kernels and no multiple of 64.  The expected plan is a stable sort
on the CPU.  Sentinel variants set some ids to E (and one to -1): pos = -1 there, everything else as if those pairs did not
exist.

Values.  Operand family E of tests/test_gemm_elements.py (small integers times a power of two, every fp32 sum an integer
multiple of one unit below 2^24 units: summation order cannot matter), with the same input conditions asserted before a
kernel runs; the documented chains are then reproduced by float64 bit for bit (torch.equal).  The SwiGLU way out is checked
per element under the gate rule of test_swiglu_epilogue.  One random-normal case per GEMM mode goes through
kernel_checks.check with s = 2^-23 K sum_k |a_k b_k|.  Outputs live inside sentinel-filled buffers; refused calls leave
them untouched.  Expected values never come from another kernel."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_checks import BF16, F16, MANT, SENT, Guarded, GuardedMatrix, check, rnd, ulp
from test_gemm_elements import (U2, amplitude, floor_of, place, ptr, representable_and_ties, same, sigmoid_terms, stream_of,
                                sync)
from transformers_amd import _cabi, ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]
A_KM, B_KN = 1, 2
EPI_NONE, EPI_SWIGLU = 0, 5
E_DTYPE, E_SHAPE, E_ALIGN, E_NULL, E_ARG = -1, -2, -3, -4, -6
H, I = 128, 136  # N = 2 I = 272: the second column tile of the gate|up product is ragged


# ---------------------------------------------------------------------------------------------------- plans
def case1_index():
    pairs = [(4, 5)] * 256 + [(5, 3)] * 2 + [(2, 3)] * 63 + [(2, 1)]
    idx = torch.tensor(pairs, dtype=torch.int64)
    return idx[torch.randperm(len(pairs), generator=torch.Generator().manual_seed(322))].contiguous()


def case2_index():
    return torch.randint(0, 128, (300, 8), generator=torch.Generator().manual_seed(128), dtype=torch.int64)


def with_sentinels(idx, E):
    """every 7th pair (and pair 3 with -1) names no expert"""
    out = idx.clone().reshape(-1)
    out[5::7] = E
    out[3] = -1
    return out.view(idx.shape)


class Plan:
    """The expected plan: a stable sort by expert on the CPU."""

    def __init__(self, idx, E):
        self.idx, self.E, (self.T, self.k) = idx, E, idx.shape
        flat = idx.reshape(-1)
        valid = (flat >= 0) & (flat < E)
        order = torch.sort(torch.where(valid, flat, torch.full_like(flat, E)), stable=True).indices
        self.count = torch.bincount(flat[valid], minlength=E).to(torch.int32)
        padded = (self.count + 63) // 64 * 64
        self.offset = torch.zeros(E + 1, dtype=torch.int32)
        self.offset[1:] = torch.cumsum(padded, 0)
        pos = torch.full((flat.numel(),), -1, dtype=torch.int32)
        start = 0
        for e in range(E):
            n = int(self.count[e])
            pos[order[start:start + n]] = self.offset[e] + torch.arange(n, dtype=torch.int32)
            start += n
        self.pos = pos.view(idx.shape)
        self.rows_pad = ops.moe_rows_pad(flat.numel(), E)
        ntile = (padded + 255) // 256
        first = torch.zeros(E + 1, dtype=torch.int32)
        first[1:] = torch.cumsum(ntile, 0)
        owner = torch.full((ops.moe_tile_ints(self.rows_pad, E) - E - 1,), -1, dtype=torch.int32)
        owner[:int(first[E])] = torch.repeat_interleave(torch.arange(E, dtype=torch.int32), ntile.long())
        self.tiles = torch.cat([first, owner])
        self.used = int(self.offset[E])  # rows inside segments
        assert self.used <= self.rows_pad

    def seg(self, e):
        return slice(int(self.offset[e]), int(self.offset[e + 1]))

    def sort_rows(self, per_pair):
        """[T * k, C] float64 values per pair -> the sorted buffer [rows_pad, C] with zeros in every row no pair owns"""
        out = torch.zeros(self.rows_pad, per_pair.shape[1], dtype=torch.float64)
        p = self.pos.reshape(-1).long()
        out[p[p >= 0]] = per_pair[p >= 0]
        return out

    def dev(self, device):
        return tuple(t.to(device) for t in (self.count, self.offset, self.pos, self.tiles))


_PLANS = {}


def plan_of(name):
    if name not in _PLANS:
        base, E = (case1_index(), 6) if name.startswith("case1") else (case2_index(), 128)
        _PLANS[name] = Plan(with_sentinels(base, E) if name.endswith("sentinel") else base, E)
    return _PLANS[name]


def test_case1_counts_are_the_ones_the_kernels_must_meet():
    p = plan_of("case1")
    assert p.count.tolist() == [0, 1, 64, 65, 256, 258] and p.offset.tolist() == [0, 0, 64, 128, 256, 512, 832]
    assert all(a != b for a, b in p.idx.tolist())
    assert plan_of("case2").idx.numel() == 2400 and plan_of("case2").idx.numel() % 64 != 0
    assert (plan_of("case1_sentinel").pos == -1).sum().item() == (plan_of("case1_sentinel").idx.reshape(-1) >= 6).sum().item() + 1


@pytest.mark.parametrize("name", ["case1", "case2", "case1_sentinel", "case2_sentinel"])
def test_route_equals_a_stable_sort(env, name):
    p = plan_of(name)
    count, offset, pos, tiles = ops.raw_moe_route(p.idx.to(env.device), p.E)
    sync(env.device)
    for got, want, what in ((count, p.count, "count"), (offset, p.offset, "offset"), (pos, p.pos, "pos"), (tiles, p.tiles, "tiles")):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (name, what, got.cpu().tolist()[:16], want.tolist()[:16])
    # twice the same plan: nothing depends on what the workspace or the outputs held
    again = ops.raw_moe_route(p.idx.to(env.device), p.E)
    assert all(torch.equal(a, b) for a, b in zip(again, (count, offset, pos, tiles)))


# ---------------------------------------------------------------------------------------------------- gather / combine
def exact_rows(shape, seed, amp=16, scale=2.0 ** -3):
    return torch.randint(-amp, amp + 1, shape, generator=torch.Generator().manual_seed(seed)).double() * scale


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["case1", "case1_sentinel"])
def test_gather_combine_and_backward_are_the_documented_chains(env, name, dtype):
    """H = 72 (no multiple of 64: nine 16-byte pieces per row).  x, dout: integers of [-16, 16] times 2^-3; ys: integers of
    [-128, 128] (bf16) / [-1024, 1024] (fp16) times 2^-3 -- as wide as T holds exactly; w: integers of [1, 15] times 2^-4.
    Every product w * y is a multiple of 2^-7 below 2^11 units wide of 2^14, every sum of two of them and every row dot product
    (72 terms, multiples of 2^-6, below 2^21 units together) is exact in fp32, so
        xs = x rows, zeros elsewhere;  out = rT(sum_j w y);  dys = rT(w dout), zeros elsewhere;  dw = r_w(sum_h dout ys)
    hold bit for bit, with w in fp32 and in T -- and the sums w y need 11 (bf16) / 14 (fp16) bits: the one rounding to T decides."""
    p, dev, h = plan_of(name), env.device, 72
    count, offset, pos, _ = p.dev(dev)
    x, dout = exact_rows((p.T, h), 1), exact_rows((p.T, h), 3)
    ys = exact_rows((p.rows_pad, h), 2, amp=128 if dtype == BF16 else 1024)
    w = torch.randint(1, 16, (p.T, p.k), generator=torch.Generator().manual_seed(4)).double() * 2.0 ** -4
    for t in (x, ys, dout, w):
        assert torch.equal(t.to(dtype).double(), t)
    valid = (p.pos >= 0)
    rows = p.pos.clamp_min(0).long()
    # gather
    XS = GuardedMatrix(p.rows_pad, h, h, dtype, dev)
    ops.raw_moe_gather(x.to(dtype).to(dev), pos, count, offset, out=XS.t)
    sync(dev)
    assert XS.intact()
    same(XS.t.cpu().double(), p.sort_rows(x.repeat_interleave(p.k, 0)), (name, "gather"))  # (padding rows: exactly zero)
    # combine
    terms = w[:, :, None] * ys[rows] * valid[:, :, None]
    assert terms.abs().max().item() < 2 ** 24 * 2.0 ** -8 and torch.equal(terms.float().double(), terms)
    want = rnd(terms.sum(1), dtype)
    hard, ties = representable_and_ties(terms.sum(1), dtype)
    assert hard >= 0.15, hard  # the final rounding is exercised
    for wt in (w.float(), w.to(dtype)):
        OUT = GuardedMatrix(p.T, h, h, dtype, dev)
        ops.raw_moe_combine(ys.to(dtype).to(dev), pos, wt.to(dev), out=OUT.t)
        sync(dev)
        assert OUT.intact()
        same(OUT.t.cpu().double(), want, (name, "combine", wt.dtype))
    # unit weights: the gradient of the gather
    OUT = GuardedMatrix(p.T, h, h, dtype, dev)
    ops.raw_moe_combine(ys.to(dtype).to(dev), pos, None, out=OUT.t)
    sync(dev)
    assert OUT.intact()
    same(OUT.t.cpu().double(), rnd((ys[rows] * valid[:, :, None]).sum(1), dtype), (name, "combine, unit weights"))
    # combine backward
    dys_want = p.sort_rows(rnd(w[:, :, None] * dout[:, None, :], dtype).reshape(-1, h))
    dots = (dout[:, None, :] * ys[rows]).sum(-1) * valid
    assert 72 * 16 * (128 if dtype == BF16 else 1024) < 2 ** 24 and dots.abs().max().item() < 2 ** 24 * 2.0 ** -6
    for wt in (w.float(), w.to(dtype)):
        DYS = GuardedMatrix(p.rows_pad, h, h, dtype, dev)
        DW = Guarded((p.T, p.k), wt.dtype, dev, 64)
        ops.raw_moe_combine_bwd(dout.to(dtype).to(dev), ys.to(dtype).to(dev), pos, wt.to(dev), count, offset, dys=DYS.t, dw=DW.t)
        sync(dev)
        assert DYS.intact() and DW.intact()
        same(DYS.t.cpu().double(), dys_want, (name, "combine_bwd dys", wt.dtype))  # (padding rows: exactly zero)
        same(DW.t.cpu().double(), dots.to(wt.dtype).double(), (name, "combine_bwd dw", wt.dtype))
    if name.endswith("sentinel"):
        assert (~valid).any() and torch.equal(dots[~valid], torch.zeros_like(dots[~valid]))


# ---------------------------------------------------------------------------------------------------- routed GEMM
class RoutedProblem:
    """Exact operands of the experts' products over the segments of case 1: A [rows_pad, Ka] (zeros in rows no pair owns),
    one B per expert.  mode "rows": acc_e = A[seg_e] . B_e^T ([N, K] per expert); mode "k": acc_e = A[seg_e]^T . B2[seg_e]."""

    def __init__(self, dtype, mode, K, N, M=None, unit=2.0 ** -5, sa=2.0 ** -3):
        self.p = p = plan_of("case1")
        self.dtype, self.mode, self.K, self.N, self.M, self.u = dtype, mode, K, N, M, unit
        depth = K if mode == "rows" else 320  # the longest segment
        amp = amplitude(dtype, depth)
        assert depth * amp * amp < 2 ** 24  # (i)
        sb = unit / sa
        pairs = p.T * p.k
        for seed in range(64):
            g = torch.Generator().manual_seed(1000 * seed + 7 * K + 3 * N + (M or 0))
            if mode == "rows":
                a = p.sort_rows(torch.randint(-amp, amp + 1, (pairs, K), generator=g).double())
                b = torch.randint(-amp, amp + 1, (p.E, N, K), generator=g).double()
                acc = torch.zeros(p.rows_pad, N, dtype=torch.float64)
                for e in range(p.E):
                    acc[p.seg(e)] = a[p.seg(e)] @ b[e].t()
                live = acc[:p.used][a[:p.used].abs().sum(1) > 0]
            else:
                a = p.sort_rows(torch.randint(-amp, amp + 1, (pairs, M), generator=g).double())
                b = p.sort_rows(torch.randint(-amp, amp + 1, (pairs, N), generator=g).double())
                acc = torch.stack([a[p.seg(e)].t() @ b[p.seg(e)] for e in range(p.E)])
                live = acc[4:]  # the experts with 256 and 258 rows
            hard, ties = representable_and_ties(live, dtype)
            if hard >= 0.15 and ties >= 0.05:  # (iii): a property of the inputs alone
                break
        else:
            raise AssertionError("no operands with 15 % unrepresentable sums and 5 % ties")
        self.hard, self.ties = hard, ties
        self.A, self.B, self.acc = a * sa, b * sb, acc * unit
        assert torch.equal(self.A.to(dtype).double(), self.A) and torch.equal(self.B.to(dtype).double(), self.B)
        assert acc.abs().max().item() < 2 ** 24  # every fp32 sum is exact
        assert self.acc.abs().max().item() < float(torch.finfo(dtype).max)  # (ii)


_ROUTED = {}


def routed_problem(*key, **kw):
    k = key + tuple(sorted(kw.items()))
    if k not in _ROUTED:
        _ROUTED[k] = RoutedProblem(*key, **kw)
    return _ROUTED[k]


def routed_call(env, dtype, A, B, C, C2, plan, M, N, K, flags, epi, b_stride=None, ldc2=0, code=None, offset=None, tiles=None,
                experts=None, rows_pad=None):
    """tamd_gemm_routed through the C ABI: A / B / C / C2 are views whose row stride may exceed their width"""
    lib = ops.backend().lib
    _, off, _, til = plan
    ldb = B.stride(-2)
    st = lib.tamd_gemm_routed(ptr(A), ptr(B), ptr(C), ptr(C2), ptr(off) if offset is None else offset,
                              ptr(til) if tiles is None else tiles, A.shape[0] if rows_pad is None else rows_pad,
                              off.numel() - 1 if experts is None else experts, M, N, K, A.stride(0), ldb,
                              C.stride(0) if C is not None else 0, ldc2, (B.stride(0) if B.dim() == 3 else 0) if b_stride is None else b_stride,
                              flags, epi, ops._code(A) if code is None else code, stream_of(A))
    sync(env.device)
    return st


def place3(t64, dtype, dev, ld):
    """[E, R, C] float64 -> a device view with row stride ld, NaN in the gap columns"""
    e, r, c = t64.shape
    buf = torch.full((e, r, ld), float("nan"), dtype=dtype)
    buf[:, :, :c] = t64.to(dtype)
    return buf.to(dev)[:, :, :c]


def expect_rows(p, acc_rounded):
    """the output buffer of a rows-routed product: the chain inside the segments, the sentinel behind the last one"""
    want = torch.full_like(acc_rounded, SENT)
    want[:p.used] = acc_rounded[:p.used]
    return want


@pytest.mark.parametrize("dtype", DTYPES)
def test_routed_forward_and_dx_are_exact(env, dtype):
    """rows routed, plain way out: C[seg_e] = rT(A[seg_e] . B_e^T) with B_e row-major [N = 272, K = 128] (the forward layout)
    and C[seg_e] = rT(A[seg_e] . B_e) with B_e = [K = 128, N = 136] (TAMD_GEMM_B_KN, the dX layout); leading dimensions larger
    than the widths, NaN in the operands' gaps.  Padding rows of a segment come out as zeros (their A rows are zeros), rows
    behind the last segment are not touched."""
    dev = env.device
    for flags, N in ((0, 2 * I), (B_KN, I)):
        q = routed_problem(dtype, "rows", H, N)
        a = place(q.A, dtype, dev, H + 8)
        b = place3(q.B.transpose(1, 2).contiguous() if flags else q.B, dtype, dev, (N if flags else H) + 16)
        C = GuardedMatrix(q.p.rows_pad, N, N + 24, dtype, dev)
        assert routed_call(env, dtype, a, b, C.t, None, q.p.dev(dev), 0, N, H, flags, EPI_NONE) == 0
        assert C.intact()
        same(C.t.cpu().double(), expect_rows(q.p, rnd(q.acc, dtype)), ("rows routed", flags))


@pytest.mark.parametrize("dtype", DTYPES)
def test_routed_swiglu_way_out(env, dtype):
    """rows routed with the SwiGLU way out at I = 136: GU = rT(acc) bit-exact, ACT = rT(rT(silu(gate)) * up) per element under
    the gate rule of test_swiglu_epilogue; with GU and with GU == NULL (same ACT)."""
    dev = env.device
    amp = amplitude(dtype, H)
    sd = np.sqrt(H) * amp * (amp + 1) / 3.0
    q = routed_problem(dtype, "rows", H, 2 * I, unit=2.0 ** int(round(np.log2(2.0 / sd))))
    p = q.p
    gu = rnd(q.acc, dtype)
    g, u = gu[:p.used, :I], gu[:p.used, I:]
    assert 5.0 < g.abs().max().item() < 32.0 and (g.abs() < 1).double().mean().item() > 0.2
    sig, es = sigmoid_terms(g)
    silu = g * sig
    ref = silu * u
    s = (g.abs() * es + U2 * silu.abs() + ulp(silu, dtype)) * u.abs() + U2 * ref.abs()
    chain = rnd(rnd(silu, dtype) * u, dtype)
    f32 = rnd(torch.nn.functional.silu(g.float()).double(), dtype) * u
    a, b = place(q.A, dtype, dev, H + 8), place3(q.B, dtype, dev, H + 16)
    acts = []
    for with_gu in (True, False):
        GU = GuardedMatrix(p.rows_pad, 2 * I, 2 * I + 24, dtype, dev) if with_gu else None
        ACT = GuardedMatrix(p.rows_pad, I, I + 8, dtype, dev)
        st = routed_call(env, dtype, a, b, GU.t if with_gu else None, ACT.t, p.dev(dev), 0, 2 * I, H, 0, EPI_SWIGLU, ldc2=I + 8)
        assert st == 0 and ACT.intact() and (GU is None or GU.intact())
        if with_gu:
            same(GU.t.cpu().double(), expect_rows(p, gu), "routed swiglu GU")
        assert bool((ACT.t[p.used:] == SENT).all())
        check("routed.swiglu.act", ACT.t[:p.used], ref, s, dtype, chain=chain, group="moe_kernels", own_floor=floor_of(f32, ref, s, dtype))
        acts.append(ACT.t.cpu())
    assert torch.equal(acts[0], acts[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_routed_weight_gradients_are_exact(env, dtype):
    """K routed: dW_e = rT(A[seg_e]^T . B[seg_e]) for M = 128, N = 136, K = the expert's 0 / 64 / 64 / 128 / 256 / 320 rows;
    expert 0 (no rows) is all zeros, written by the kernel; ldc > N, the gap columns and the guard rows stay sentinel."""
    dev = env.device
    q = routed_problem(dtype, "k", 0, I, M=H)
    p = q.p
    a, b = place(q.A, dtype, dev, H + 8), place(q.B, dtype, dev, I + 16)
    C = GuardedMatrix(p.E * H, I, I + 8, dtype, dev)
    st = routed_call(env, dtype, a, b, C.t, None, p.dev(dev), H, I, 0, A_KM | B_KN, EPI_NONE)
    assert st == 0 and C.intact()
    got = C.t.cpu().double().view(p.E, H, I)
    same(got.reshape(-1, I), rnd(q.acc, dtype).reshape(-1, I), "K routed")
    assert torch.equal(got[0], torch.zeros(H, I, dtype=torch.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_routed_random_operands(env, dtype):
    """Full-mantissa operands on every mode, every element within the gate of kernel_checks.check."""
    dev, p = env.device, plan_of("case1")
    g = torch.Generator().manual_seed(17)
    pairs = p.T * p.k
    plan = p.dev(dev)
    A = p.sort_rows(torch.randn(pairs, H, generator=g).to(dtype).double())
    for flags, N, name in ((0, 2 * I, "nt"), (B_KN, I, "nn")):
        B = (torch.randn(p.E, N, H, generator=g) * 0.1).to(dtype).double()
        b = place3(B.transpose(1, 2).contiguous() if flags else B, dtype, dev, (N if flags else H) + 16)
        C = GuardedMatrix(p.rows_pad, N, N + 8, dtype, dev)
        assert routed_call(env, dtype, place(A, dtype, dev, H + 8), b, C.t, None, plan, 0, N, H, flags, EPI_NONE) == 0 and C.intact()
        for e in range(1, p.E):
            ref = A[p.seg(e)] @ B[e].t()
            check(f"routed.{name}", C.t[p.seg(e)], ref, U2 * H * (A[p.seg(e)].abs() @ B[e].abs().t()), dtype, group="moe_kernels")
    # the SwiGLU way out on random operands: GU is the plain product's chain
    B = (torch.randn(p.E, 2 * I, H, generator=g) * 0.1).to(dtype).double()
    GU, ACT = GuardedMatrix(p.rows_pad, 2 * I, 2 * I + 8, dtype, dev), GuardedMatrix(p.rows_pad, I, I + 8, dtype, dev)
    st = routed_call(env, dtype, place(A, dtype, dev, H + 8), place3(B, dtype, dev, H + 16), GU.t, ACT.t, plan, 0, 2 * I, H, 0, EPI_SWIGLU, ldc2=I + 8)
    assert st == 0 and GU.intact() and ACT.intact()
    for e in range(1, p.E):
        ref = A[p.seg(e)] @ B[e].t()
        check("routed.swiglu.gu", GU.t[p.seg(e)], ref, U2 * H * (A[p.seg(e)].abs() @ B[e].abs().t()), dtype, group="moe_kernels")
    # K routed
    B2 = p.sort_rows((torch.randn(pairs, I, generator=g) * 0.1).to(dtype).double())
    C = GuardedMatrix(p.E * H, I, I + 8, dtype, dev)
    st = routed_call(env, dtype, place(A, dtype, dev, H + 8), place(B2, dtype, dev, I + 16), C.t, None, plan, H, I, 0, A_KM | B_KN, EPI_NONE)
    assert st == 0 and C.intact()
    for e in range(p.E):
        a_e, b_e = A[p.seg(e)], B2[p.seg(e)]
        ref = a_e.t() @ b_e
        check("routed.dw", C.t[e * H:(e + 1) * H], ref, U2 * max(1, a_e.shape[0]) * (a_e.abs().t() @ b_e.abs()), dtype, group="moe_kernels")


def test_refused_calls_leave_the_buffers_untouched(env):
    """NULL, misaligned pointers, H % 64 (the products' K), I % 8, E > 256 and fp32 are reported without a launch."""
    dev, dtype, p = env.device, BF16, plan_of("case1")
    lib = ops.backend().lib
    plan = count, offset, pos, tiles = p.dev(dev)
    a = torch.zeros(p.rows_pad, H + 8, dtype=dtype, device=dev)[:, :H]
    b = torch.zeros(p.E, 2 * I, H, dtype=dtype, device=dev)
    C, C2 = GuardedMatrix(p.rows_pad, 2 * I, 2 * I + 8, dtype, dev), GuardedMatrix(p.rows_pad, I, I + 8, dtype, dev)

    def refused(want, A=a, B=b, c=C.t, c2=None, M=0, N=2 * I, K=H, flags=0, epi=EPI_NONE, **kw):
        st = routed_call(env, dtype, A, B, c, c2, plan, M, N, K, flags, epi, **kw)
        assert st == want, (st, want, kw)
        assert C.untouched() and C2.untouched()

    null = ctypes.c_void_p(0)
    refused(E_NULL, offset=null)
    refused(E_NULL, tiles=null)
    refused(E_NULL, c=None)
    refused(E_NULL, c2=None, epi=EPI_SWIGLU)
    off8 = torch.zeros(p.rows_pad * (H + 8) + 8, dtype=dtype, device=dev)[4:4 + p.rows_pad * (H + 8)].view(p.rows_pad, H + 8)[:, :H]
    refused(E_ALIGN, A=off8)  # 8 bytes past a 16-byte boundary
    c_off8 = C.full.view(-1)[4:4 + (p.rows_pad - 1) * (2 * I + 8)].view(p.rows_pad - 1, 2 * I + 8)[:, :2 * I]
    refused(E_ALIGN, c=c_off8)
    refused(E_SHAPE, K=72)                                    # the products' K: H % 64
    refused(E_SHAPE, N=2 * 132, c2=C2.t, epi=EPI_SWIGLU, ldc2=I + 8)  # I % 8
    refused(E_SHAPE, experts=257)
    refused(E_SHAPE, rows_pad=p.rows_pad + 8)
    refused(E_SHAPE, M=H + 4, N=I, flags=A_KM | B_KN)       # k-major A: M % 8
    refused(E_DTYPE, code=_cabi.TAMD_F32)
    refused(E_ARG, flags=A_KM)
    refused(E_ARG, epi=1)
    # the routing kernels
    x = torch.zeros(p.T, 72, dtype=dtype, device=dev)
    XS = GuardedMatrix(p.rows_pad, 72, 72, dtype, dev)
    s = stream_of(x)
    assert lib.tamd_moe_gather(ptr(x), ptr(pos), ptr(count), ptr(offset), ptr(XS.t), p.T, p.k, 257, 72, p.rows_pad, 0, s) == E_SHAPE
    assert lib.tamd_moe_gather(ptr(x), ptr(pos), ptr(count), ptr(offset), ptr(XS.t), p.T, p.k, p.E, 68, p.rows_pad, 0, s) == E_SHAPE
    assert lib.tamd_moe_gather(ptr(x), ptr(pos), ptr(count), ptr(offset), ptr(XS.t), p.T, p.k, p.E, 72, p.rows_pad - 64, 0, s) == E_SHAPE
    assert lib.tamd_moe_gather(ptr(x), ptr(pos), ptr(count), ptr(offset), ptr(XS.t), p.T, p.k, p.E, 72, p.rows_pad, 2, s) == E_DTYPE
    assert lib.tamd_moe_gather(ptr(x), None, ptr(count), ptr(offset), ptr(XS.t), p.T, p.k, p.E, 72, p.rows_pad, 0, s) == E_NULL
    assert lib.tamd_moe_gather(ptr(x), ptr(pos), ptr(count), ptr(offset), ptr(XS.t) + 2, p.T, p.k, p.E, 72, p.rows_pad, 0, s) == E_ALIGN
    assert lib.tamd_moe_combine(ptr(XS.t), ptr(pos), None, ptr(x), p.T, p.k, 72, 2, 2, s) == E_DTYPE
    assert lib.tamd_moe_combine(None, ptr(pos), None, ptr(x), p.T, p.k, 72, 2, 0, s) == E_NULL
    assert lib.tamd_moe_combine_bwd(ptr(x), ptr(XS.t), ptr(pos), None, ptr(count), ptr(offset), ptr(XS.t), ptr(x), p.T, p.k, p.E, 72, p.rows_pad, 2, 0, s) == E_NULL
    assert lib.tamd_moe_route(ptr(p.idx.to(dev)), ptr(count), ptr(offset), ptr(pos), ptr(tiles), None, 0, p.T, p.k, p.E, p.rows_pad, s) == E_NULL
    assert lib.tamd_moe_route_workspace_bytes(p.T, p.k, 257) == 0
    ws = torch.zeros(64, dtype=torch.int32, device=dev)
    assert lib.tamd_moe_route(ptr(p.idx.to(dev)), ptr(count), ptr(offset), ptr(pos), ptr(tiles), ptr(ws), 4, p.T, p.k, p.E, p.rows_pad, s) == -5
    sync(dev)
    assert XS.untouched() and torch.equal(count.cpu(), p.count) and torch.equal(pos.cpu(), p.pos)


# ---------------------------------------------------------------------------------------------------- the op
def experts_reference(x, idx, w, wgu, wd, dout, dtype=None):
    """The experts module and its four gradients in float64 over the plan of a stable sort: with `dtype` every point where the
    kernels round to the storage type is rounded (the composition of the documented chains), without it nothing is.
    Returns the results and, per result, the same composition on absolute values (the magnitude the roundings act on)."""
    p = Plan(idx, wgu.shape[0])
    r = (lambda t: rnd(t, dtype)) if dtype is not None else (lambda t: t)
    E, inter = wgu.shape[0], wd.shape[2]
    valid = (p.pos >= 0)
    rows = p.pos.clamp_min(0).long()
    per_expert = lambda a, b, f: torch.cat([f(a[p.seg(e)], b[e]) for e in range(E)] + [a.new_zeros(p.rows_pad - p.used, f(a[:1], b[0]).shape[1])])  # noqa: E731
    xs = p.sort_rows(x.repeat_interleave(p.k, 0))
    gu = r(per_expert(xs, wgu, lambda a, b: a @ b.t()))
    g, u = gu[:, :inter], gu[:, inter:]
    sig = torch.sigmoid(g)
    silu = r(g * sig)
    act = r(silu * u)
    ys = r(per_expert(act, wd, lambda a, b: a @ b.t()))
    out = r((w[:, :, None] * ys[rows] * valid[:, :, None]).sum(1))
    dys = p.sort_rows(r(w[:, :, None] * dout[:, None, :]).reshape(-1, x.shape[1]))
    dw = r((dout[:, None, :] * ys[rows]).sum(-1) * valid)
    dact = r(per_expert(dys, wd, lambda a, b: a @ b))
    dgate = r(r(dact * u) * (sig * (1 + g * (1 - sig))))  # tamd_swiglu_bwd: round(round(d_act * up) * silu'(gate))
    dup = r(dact * silu)
    dgu = torch.cat([dgate, dup], 1)
    dxs = r(per_expert(dgu, wgu, lambda a, b: a @ b))
    dx = r((dxs[rows] * valid[:, :, None]).sum(1))
    dwd = r(torch.stack([dys[p.seg(e)].t() @ act[p.seg(e)] for e in range(E)]))
    dwgu = r(torch.stack([dgu[p.seg(e)].t() @ xs[p.seg(e)] for e in range(E)]))
    mag = dict(
        out=(w[:, :, None] * per_expert(act.abs(), wd.abs(), lambda a, b: a @ b.t())[rows] * valid[:, :, None]).sum(1),
        dw=(dout.abs()[:, None, :] * ys.abs()[rows]).sum(-1) * valid,
        dx=(per_expert(dgu.abs(), wgu.abs(), lambda a, b: a @ b)[rows] * valid[:, :, None]).sum(1),
        dwd=torch.stack([dys[p.seg(e)].abs().t() @ act[p.seg(e)].abs() for e in range(E)]),
        dwgu=torch.stack([dgu[p.seg(e)].abs().t() @ xs[p.seg(e)].abs() for e in range(E)]))
    return dict(out=out, dw=dw, dx=dx, dwd=dwd, dwgu=dwgu), mag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["case1", "case1_sentinel"])
def test_moe_experts_op_forward_and_gradients(env, name, dtype):
    """torch.ops.tamd.moe_experts and its four gradients (x, top_k_weights, gate_up_proj, down_proj) on case 1 with H = 128,
    I = 136 (neither I nor 2 I a multiple of 64: the op extends K with zeros) against float64.  Reference: the composition
    WITHOUT any rounding.  Yardstick: the same composition with every documented rounding (chain).  Per element
        |got - ref| <= gate * (ulp_T(ref) + s),   gate = 2 * max(0.5, own),   own = the chain's own error in that unit,
    s = 6 * 2^-(mantissa + 1) * (the composition on absolute values): six storage-type roundings at most lie between the
    operands and a result (gate|up, silu, act, ys / d_act, the two of d_gate, d_xs), each moving a term by half an ulp of
    its magnitude.  The kernels differ from the chain only where fp32 sigmoid arithmetic moves a rounding."""
    dev, p = env.device, plan_of(name)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(p.T, H, generator=g).to(dtype).double()
    wgu = (torch.randn(p.E, 2 * I, H, generator=g) * 0.1).to(dtype).double()
    wd = (torch.randn(p.E, H, I, generator=g) * 0.1).to(dtype).double()
    w = torch.softmax(torch.randn(p.T, p.k, generator=g), -1).to(dtype).double()
    dout = torch.randn(p.T, H, generator=g).to(dtype).double()
    ref, mag = experts_reference(x, p.idx, w, wgu, wd, dout)
    chain, _ = experts_reference(x, p.idx, w, wgu, wd, dout, dtype)
    leaves = [t.to(dtype).to(dev).requires_grad_(True) for t in (x, w, wgu, wd)]
    out = ops.moe_experts(leaves[0], p.idx.to(dev), leaves[1], leaves[2], leaves[3])
    dx, dw, dwgu, dwd = torch.autograd.grad(out, leaves, dout.to(dtype).to(dev))
    sync(dev)
    assert torch.equal(dwd[0].cpu(), torch.zeros_like(dwd[0].cpu())) and torch.equal(dwgu[0].cpu(), torch.zeros_like(dwgu[0].cpu()))
    half_ulp = 2.0 ** -(MANT[dtype] + 1)
    for key, got in (("out", out), ("dx", dx), ("dw", dw), ("dwgu", dwgu), ("dwd", dwd)):
        check(f"moe_experts.{key}", got.reshape(ref[key].shape), ref[key], 6 * half_ulp * mag[key], dtype, chain=chain[key],
              group="moe_kernels")
    # inference: no gate|up kept, same output bits
    with torch.no_grad():
        out2 = ops.moe_experts(leaves[0], p.idx.to(dev), leaves[1], leaves[2], leaves[3])
    assert torch.equal(out2, out.detach())


def test_moe_experts_opcheck(env):
    from torch.library import opcheck

    dev = env.device
    g = torch.Generator().manual_seed(9)
    idx = torch.stack([torch.randperm(4, generator=g)[:2] for _ in range(24)])
    x = torch.randn(24, 64, generator=g).bfloat16().to(dev).requires_grad_(True)
    w = torch.softmax(torch.randn(24, 2, generator=g), -1).bfloat16().to(dev).requires_grad_(True)
    wgu = (torch.randn(4, 128, 64, generator=g) * 0.1).bfloat16().to(dev).requires_grad_(True)
    wd = (torch.randn(4, 64, 64, generator=g) * 0.1).bfloat16().to(dev).requires_grad_(True)
    opcheck(torch.ops.tamd.moe_experts, (x, idx.to(dev), w, wgu, wd, True),
            test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    count, offset, pos, tiles = ops.raw_moe_route(idx.to(dev), 4)
    xs = torch.empty(ops.moe_rows_pad(48, 4), 64, dtype=torch.bfloat16, device=dev)
    opcheck(torch.ops.tamd.moe_gather_out, (xs, x.detach(), pos, count, offset), test_utils=("test_schema",))
    opcheck(torch.ops.tamd.gemm_routed_out, (torch.empty(xs.shape[0], 128, dtype=torch.bfloat16, device=dev), None, xs, wgu.detach(),
                                             offset, tiles, ops.ROUTED_NT, True), test_utils=("test_schema",))
