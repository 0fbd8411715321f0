"""The GEMM family, element by element: the three tile kernels of csrc/gemm.hip (`pp`, `fl`, `sm`), the weight-streaming
kernels of csrc/gemv.hip, split-K with its reduction, the segmented and the grouped launch, every epilogue -- at ragged
edges in M and N, at the stage counts around the rings' depths, with leading dimensions larger than the width, on the
SAME small shapes under the CPU execution model (`emu`) and on the MI355X (`hip`).

Operand family E (exact).  A and B hold integers drawn uniformly from [-amp, amp], scaled by one power of two per tensor,
with K * amp_a * amp_b < 2^24: every product and every partial sum is an integer multiple of one unit u below 2^24 u, so
the fp32 accumulator holds the exact sum WHATEVER the summation order, MFMA shape, split or reduction.  Bias, residual and
the previous C are integer multiples of u as well.  Every documented result is then a chain of correctly rounded
operations that float64 reproduces exactly (rT: round to nearest even to the storage type, r32: to fp32):

    NONE      rT(acc)                            RESIDUAL  rT(rT(acc [+ b]) + R)
    BIAS      rT(acc + b)                        ACCUM     rT(rT(acc) + C_old)
    colscale  rT(r32((acc [+ b]) * f32(s))) on columns < scale_cols, the plain chain beyond

and the kernels' output must equal it bit for bit (torch.equal): no tolerance.  Before a kernel runs the reference is
checked for (i) K * amp_a * amp_b < 2^24 and every fp32 sum below 2^24 u, (ii) every rounding point below the type's
largest finite value, (iii) with K >= 32: at least 15 % of the exact sums are not representable in T and at least 5 % are
exact ties (round-to-nearest-EVEN decides them).  The operands of a case are the first of a fixed sequence of seeds
whose reference meets (iii) -- a property of the inputs alone.

Operand family R (random normal).  One case per kernel arm and layout, every element within gate * (ulp_T(ref) + s),
s = 2^-23 * K * sum_k |a_k b_k| (float64), gate = 2 * max(0.5, own): tests/kernel_checks.py.

Approximated epilogues (TAMD_EPI_BIAS_ACT, tamd_gemm_swiglu, tamd_gemm_swiglu_bwd): family E scaled so that the
pre-activations cover about [-6, 6]; what the ABI documents as a rounded product (GU, and the pre-activation, which the
BIAS chain pins) is bit-exact, the activation output is checked per element against float64 of the reference's formula on
that exact pre-activation: unit ulp_T(ref) + s, s = 2^-23 per elementwise fp32 operation of the reference's formula on the
magnitude it acts on (counted next to each formula below), gate = 2 * max(0.5, own), own = the larger of the float64
reference's own rounding error and the error of torch's fp32 operator on the same input, rounded to T, in that unit.

Every output lies inside a sentinel-filled buffer (four rows of ldc elements on either side, the ldc - N gap of every row):
all of it is asserted intact after every call; a refused call leaves the whole buffer untouched.  The gaps of the INPUT
operands hold NaN.  Expected values never come from another kernel, schedule or the CPU model."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_checks import BF16, F16, NAME, GuardedMatrix, check, rnd, ulp
from transformers_amd import _cabi, ops

U2 = 2.0 ** -23
A_KM, B_KN = 1, 2
PP, SM, FL = 1 << 8, 2 << 8, 3 << 8
SCHED = {"pp": PP, "sm": SM, "fl": FL, "auto": 0}
NONE, BIAS, RESIDUAL, BIAS_ACT, ACCUM = 0, 1, 2, 3, 4
E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4
SA, SB = 2.0 ** -3, 2.0 ** -2  # the operands' powers of two; u = SA * SB is the unit of every sum
U = SA * SB
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]


def amplitude(dtype, K):
    """The integers' range per (type, K), from {8, 16, 32, 64}.  The sums have a standard deviation of about
    sqrt(K) * amp^2 / 3 units: T cannot hold a sum once it exceeds 2^8 (bf16) / 2^11 (fp16) units and is odd, so the
    amplitude has to put a good share of the sums there (bf16: 16 gives 39 % unrepresentable sums and 22 % ties at K = 32;
    fp16 needs 64 up to K = 64 and 32 up to K = 704, where 16 would leave almost every sum representable), while
    K * amp^2 stays below 2^24 and the largest sum (about 7 standard deviations at most) inside fp16's 65504 units: 16 from
    K = 705 on, 8 for bf16 beyond K = 2048 (70 % / 17 % at K = 4160).  4, the smallest amplitude that still produces ties,
    is not needed at any K of this file.  ExactProduct asserts all of it on the sums themselves."""
    if dtype == BF16:
        return 16 if K <= 2048 else 8
    return 64 if K <= 64 else 32 if K <= 704 else 16


# ---------------------------------------------------------------------------------------------------- the reference
def representable_and_ties(x, dtype):
    """shares of x (float64, exact) that T cannot hold / that lie exactly between two neighbours of T"""
    d = (rnd(x, dtype) - x).abs()
    return (d != 0).double().mean().item(), (d == ulp(x, dtype) / 2).double().mean().item()


class ExactProduct:
    """One exact product [M, N] over K with its bias, residual and previous C; everything float64 on the CPU."""

    def __init__(self, dtype, M, N, K, unit, amp):
        self.dtype, self.M, self.N, self.K, self.u = dtype, M, N, K, unit
        self.amp = amp = amp or amplitude(dtype, K)
        assert K * amp * amp < 2 ** 24  # (i)
        sa = SA
        sb = unit / sa
        for seed in range(64):
            g = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K)
            ai = torch.randint(-amp, amp + 1, (M, K), generator=g).double()
            bi = torch.randint(-amp, amp + 1, (N, K), generator=g).double()
            acc = ai @ bi.t()  # integers below 2^24: exact in float64 (and in fp32, in any order)
            if K < 32:
                break
            hard, ties = representable_and_ties(acc, dtype)
            if hard >= 0.15 and ties >= 0.05:  # (iii): a property of the inputs alone
                break
        else:
            raise AssertionError(f"no operands with 15 % unrepresentable sums and 5 % ties at {M} x {N} x {K} {NAME[dtype]}")
        self.hard, self.ties = (hard, ties) if K >= 32 else (None, None)
        self.A, self.B, self.acc = ai * sa, bi * sb, acc * unit
        assert torch.equal(self.A.to(dtype).double(), self.A) and torch.equal(self.B.to(dtype).double(), self.B)
        assert acc.abs().max().item() < 2 ** 24
        # bias / residual / previous C: integers of at most 8 bits times u * 2^k, k so that they are about as large as the sums
        k = max(0, int(round(np.log2(max(1.0, np.sqrt(K) * amp * amp / 3.0 / 64.0)))))
        w = unit * 2.0 ** k
        self.bias = torch.randint(-128, 129, (N,), generator=g).double() * w
        self.R = torch.randint(-128, 129, (M, N), generator=g).double() * w
        self.C0 = torch.randint(-128, 129, (M, N), generator=g).double() * w
        for t in (self.bias, self.R, self.C0):
            assert torch.equal(t.to(dtype).double(), t)

    def _points(self, *pts):
        top = float(torch.finfo(self.dtype).max)
        for x in pts:
            m = x.abs().max().item()
            assert m < top, (m, top)  # (ii)
            assert m < 2 ** 24 * self.u, m  # the fp32 value in front of the rounding is exact

    def check_inputs(self, *pts):
        """(ii) and the exactness of every value in front of a rounding, (iii) on the sums"""
        self._points(*pts)
        if self.K >= 32:
            assert self.hard >= 0.15 and self.ties >= 0.05

    def expected(self, epi, bias=False, colscale=None):
        """the documented chain; colscale = (scale_cols, s)"""
        T = self.dtype
        pre = self.acc + self.bias if bias else self.acc
        self.check_inputs(pre)
        if colscale is not None:
            cols, s = colscale
            s = float(np.float32(s))
            scaled = (pre * s).float().double()  # one correctly rounded fp32 product: 24 x 24 bits are exact in float64
            assert scaled.abs().max().item() < float(torch.finfo(T).max)
            x = pre.clone()
            x[:, :cols] = scaled[:, :cols]
            return rnd(x, T)
        if epi in (NONE, BIAS):
            return rnd(pre, T)
        x = rnd(pre, T) + (self.R if epi == RESIDUAL else self.C0)
        self._points(x)
        return rnd(x, T)


_PROBLEMS = {}


def Problem(dtype, M, N, K, unit=U, amp=None):
    """computed once per session and shared (never modified)"""
    key = (dtype, M, N, K, unit, amp)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = ExactProduct(dtype, M, N, K, unit, amp)
    return _PROBLEMS[key]


def act_problem(dtype, M, N, K):
    """family E with the unit chosen so that the sums have a standard deviation of about 2: pre-activations over about
    [-8, 8], a third of them inside [-1, 1]"""
    amp = amplitude(dtype, K)
    sd = np.sqrt(K) * amp * (amp + 1) / 3.0
    return Problem(dtype, M, N, K, unit=2.0 ** int(round(np.log2(2.0 / sd))), amp=amp)


def place(t64, dtype, dev, ld=None):
    """[rows, cols] float64 -> a device view with row stride ld whose gap columns hold NaN"""
    rows, cols = t64.shape
    ld = ld or cols
    buf = torch.full((rows, ld), float("nan"), dtype=dtype)
    buf[:, :cols] = t64.to(dtype)
    return buf.to(dev)[:, :cols]


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream_of(t):
    sh = ops.backend().stream(t)
    return ctypes.c_void_p(sh) if sh else None


_WS = {}


def scratch(dev, nbytes):
    """a poisoned fp32 workspace (NaN): a partial tile that is read but was never written shows"""
    t = _WS.get(dev.type)
    if t is None or t.numel() * 4 < nbytes + 64:
        t = _WS[dev.type] = torch.empty((nbytes + 64) // 4 + 16, dtype=torch.float32, device=dev)
    t.fill_(float("nan"))
    return t


def operands(p, flags, dev, lda=None, ldb=None):
    a = place(p.A.t().contiguous() if flags & A_KM else p.A, p.dtype, dev, lda)
    b = place(p.B.t().contiguous() if flags & B_KN else p.B, p.dtype, dev, ldb)
    return a, b


def run(env, p, flags=0, epi=NONE, *, bias=False, sched="auto", lda=None, ldb=None, ldc=None, ldr=None, ws=None,
        colscale=None, bias_t=None, act=0):
    """One C-ABI product of Problem `p` into a guarded C.  ws: None (tamd_gemm), 'need' (tamd_gemm_ws with the size the
    library asks for, which must be > 0), or (offset bytes, size delta) to hand a misaligned / short one -- the library
    must then not split, so not one word of the (NaN-filled) workspace may be written.
    -> the [M, N] result on the CPU, float64."""
    be = ops.backend()
    lib, dev, T = be.lib, env.device, p.dtype
    M, N, K = p.M, p.N, p.K
    a, b = operands(p, flags, dev, lda, ldb)
    c = GuardedMatrix(M, N, ldc or N, T, dev, fill=p.C0.to(T) if epi == ACCUM else None)
    r = place(p.R, T, dev, ldr) if epi == RESIDUAL else None
    bv = (p.bias if bias_t is None else bias_t).to(T).to(dev) if (bias or epi in (BIAS, BIAS_ACT)) else None
    code, sh = ops._code(a), stream_of(a)
    fl = flags | SCHED[sched]
    if colscale is not None:
        st = lib.tamd_gemm_colscale(ptr(a), ptr(b), ptr(c.t), ptr(bv), M, N, K, a.stride(0), b.stride(0), c.full.stride(0),
                                    fl, colscale[0], float(colscale[1]), code, sh)
    elif ws is None:
        st = lib.tamd_gemm(ptr(a), ptr(b), ptr(c.t), ptr(bv), ptr(r), M, N, K, a.stride(0), b.stride(0), c.full.stride(0),
                           r.stride(0) if r is not None else 0, fl, epi, act, code, sh)
    else:
        need = lib.tamd_gemm_workspace_bytes(M, N, K, flags, epi)
        assert need > 0, "the case is meant to split K"
        off, delta = (0, 0) if ws == "need" else ws
        w = scratch(dev, need + 64)
        st = lib.tamd_gemm_ws(ptr(a), ptr(b), ptr(c.t), ptr(bv), ptr(r), M, N, K, a.stride(0), b.stride(0), c.full.stride(0),
                              r.stride(0) if r is not None else 0, fl, epi, act, code, w.data_ptr() + off, need + delta, sh)
    sync(dev)
    where = (NAME[T], M, N, K, flags, epi, sched, a.stride(0), b.stride(0), c.full.stride(0))
    assert st == 0, (st, where)
    if ws is not None and ws != "need":
        assert bool(w.isnan().all()), ("a workspace too short or misaligned was written: the product was split", where)
    assert c.intact(), ("guard rows or gap columns of C were written", where)
    return c.t.cpu().double()


def same(got, want, where):
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{where}: {bad.shape[0]} of {got.numel()} elements differ from the exact chain; first at {i}: "
                             f"got {got[i].item()!r} want {want[i].item()!r}; rows {sorted(set(bad[:, 0].tolist()))[:8]} "
                             f"cols {sorted(set(bad[:, 1].tolist()))[:8]}")


LAYOUTS = [0, B_KN, A_KM | B_KN, A_KM]


def layouts_of(M):
    return [f for f in LAYOUTS if not (f & A_KM) or M % 8 == 0]  # (the ABI wants M % 8 with a k-major A)


# ---------------------------------------------------------------------------------------------------- K sweeps
# pp: 32-deep stages in a ring of 4 -- 1 stage (K = 8, 24, 32: the prologue parks at j == nst), 2 (40), 3 (96), exactly the ring
# (128), 5 with an 8-wide tail (136), 5 (160), 9 (264: odd, twice round the ring);  fl / sm: 64-deep stages in 5 half-slots /
# 2 stages -- 1 .. 7 stages and 11 (odd tail of the three-barrier loop, once and twice round the slots)
K_SWEEP = {"pp": [8, 24, 32, 40, 96, 128, 136, 160, 264], "fl": [64, 128, 192, 256, 320, 384, 448, 704],
           "sm": [64, 128, 192, 320]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sched,K", [pytest.param(s, k, id=f"{s}-K{k}") for s in ("pp", "fl", "sm") for k in K_SWEEP[s]])
def test_stage_counts_on_a_ragged_tile(env, sched, K, dtype):
    """200 x 136 (ragged in M and N inside one 256 x 256 tile; two ragged 128 x 128 tiles in each direction for `sm`): every
    stage count around the ring depths, all four layouts, plain and the read-modify-write way out."""
    p = Problem(dtype, 200, 136, K)
    for flags in ([0] if sched == "sm" else LAYOUTS):
        same(run(env, p, flags, NONE, sched=sched), p.expected(NONE), (sched, K, flags, "none"))
    same(run(env, p, 0, ACCUM, sched=sched), p.expected(ACCUM), (sched, K, "accum"))


@pytest.mark.parametrize("K", [1, 7, 33, 66, 130])
def test_pp_any_k_with_both_operands_k_major(env, K):
    """dW over a ragged token count: K is a row count, zero-filled to the 32-deep stage by the loads' own bounds."""
    for dtype in (BF16, F16):
        p = Problem(dtype, 200, 136, K)
        same(run(env, p, A_KM | B_KN, NONE, sched="pp"), p.expected(NONE), ("pp", K))
        same(run(env, p, A_KM | B_KN, ACCUM, sched="pp", lda=208, ldb=144, ldc=152), p.expected(ACCUM), ("pp", K, "ld"))


# ---------------------------------------------------------------------------------------------------- shapes
# (1, 8): one row, one 8-column store; (64, 72): a last column group of exactly 8 behind a full 64-column wave piece;
# (130, 520): the second wave row holds 2 rows, three tile columns, the last 8 wide; (264, 248): a second tile row of 8 rows
# (its second wave row lies wholly past M), a last 16-byte store that ends at N; (300, 136): 44 rows in the second tile row
SHAPES = [(1, 8), (64, 72), (130, 520), (264, 248), (300, 136)]
SHAPE_K = {"pp": (40, 136), "fl": (64, 192), "sm": (64, 192)}
# the 128 x 128 tile: (72, 264) three tile columns, the last 8 wide; (130, 136): 2 rows / 8 columns in the second tiles
SM_SHAPES = [(1, 8), (72, 264), (130, 136), (264, 248)]


@pytest.mark.parametrize("sched,shape", [pytest.param(k, s, id=f"{k}-{s[0]}x{s[1]}") for k in ("pp", "fl", "sm")
                                         for s in (SM_SHAPES if k == "sm" else SHAPES)])
def test_ragged_shapes_and_layouts(env, sched, shape):
    M, N = shape
    for i, K in enumerate(SHAPE_K[sched]):
        dtype = (BF16, F16)[i]
        p = Problem(dtype, M, N, K)
        for flags in ([0] if sched == "sm" else layouts_of(M)):
            same(run(env, p, flags, NONE, sched=sched), p.expected(NONE), (sched, M, N, K, flags))
        p2 = Problem((F16, BF16)[i], M, N, K)
        same(run(env, p2, 0, BIAS, sched=sched), p2.expected(BIAS, bias=True), (sched, M, N, K, "bias"))


# ---------------------------------------------------------------------------------------------------- epilogues
def epilogue_cases(p):
    """(name, epilogue, bias?, colscale) -- scale_cols = 68: a multiple of 4 that is none of 8, inside the last wave piece"""
    s2 = 0.125 * float(np.log2(np.e))
    return [("none", NONE, False, None), ("bias", BIAS, True, None), ("residual", RESIDUAL, False, None),
            ("bias+residual", RESIDUAL, True, None), ("accum", ACCUM, False, None),
            ("colscale 2^-3", NONE, False, (68, 0.125)), ("colscale 2^-3 log2 e", NONE, False, (68, s2)),
            ("bias+colscale 2^-3 log2 e", NONE, True, (68, s2)), ("bias+colscale 4, all columns", NONE, True, (p.N, 4.0))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sched", ["pp", "fl", "sm"])
def test_every_epilogue_on_every_kernel(env, sched, dtype):
    """264 x 136 over K = 192 (ragged in both directions, a second tile row of 8 rows), dense and with lda, ldb, ldc, ldr
    larger than the widths, multiples of 8, all different.  The ACCUM chain rounds twice -- rT(rT(acc) + C_old), what
    include/tamd.h documents -- and the reference must contain elements at which rT(acc + C_old) would differ."""
    p = Problem(dtype, 264, 136, 192)
    twice, once = p.expected(ACCUM), rnd(p.acc + p.C0, dtype)
    assert (twice != once).sum().item() >= 16  # the test tells the two roundings apart
    assert (p.expected(RESIDUAL, bias=True) != rnd(p.acc + p.bias + p.R, dtype)).sum().item() >= 16
    for lds in ({}, dict(lda=200, ldb=208, ldc=152, ldr=144)):
        for name, epi, bias, cs in epilogue_cases(p):
            kw = {k: v for k, v in lds.items() if not (cs is not None and k == "ldr")}
            got = run(env, p, 0, epi, bias=bias, sched=sched, colscale=cs, **kw)
            same(got, p.expected(epi, bias=bias, colscale=cs), (sched, name, lds))
    if sched != "sm":  # the k-major layouts with leading dimensions (fused q|k|v slices, bucket views): A [K, lda], B [K, ldb]
        for flags in (B_KN, A_KM | B_KN, A_KM):
            for name, epi, bias in (("bias+residual", RESIDUAL, True), ("accum", ACCUM, False)):
                got = run(env, p, flags, epi, bias=bias, sched=sched, lda=272 if flags & A_KM else 200,
                          ldb=160 if flags & B_KN else 208, ldc=152, ldr=144)
                same(got, p.expected(epi, bias=bias), (sched, name, flags, "ld"))


# ---------------------------------------------------------------------------------------------------- default dispatch
@pytest.mark.parametrize("M", [1, 4, 5, 16, 17])
def test_default_dispatch_decode_rows(env, M):
    """Without a schedule hint: M <= 4 the VALU weight-streaming kernel, 5 .. 16 the MFMA one (csrc/gemv.hip), 17 the tile
    kernels (sm at K % 64 == 0, pp at K = 520).  Strided x, ldc > N; plain / bias / residual (+ bias): the same chains."""
    for dtype in (BF16, F16):
        for N in (72, 264):
            for K in (64, 520):
                p = Problem(dtype, M, N, K)
                for lds in ({}, dict(lda=K + 24, ldb=K + 8, ldc=N + 16, ldr=N + 8)):
                    for epi, bias in ((NONE, False), (BIAS, True), (RESIDUAL, False), (RESIDUAL, True)):
                        kw = {k: v for k, v in lds.items() if epi == RESIDUAL or k != "ldr"}
                        got = run(env, p, 0, epi, bias=bias, **kw)
                        same(got, p.expected(epi, bias=bias), (M, N, K, epi, bias, lds))


# ---------------------------------------------------------------------------------------------------- split-K
# (M, N, K, flags): 33 stages over 2 tiles -> 4 splits of 9 / 9 / 9 / 6;  130 stages over one tile -> 16 asked, 15 x 9 cover them
# ("no empty split"), the last of 4;  a forward product of 64 stages (17 rows: the tile kernels) -> 8 splits of 8
SPLITK = [(264, 136, 2112, A_KM | B_KN, 4), (264, 136, 2112, B_KN, 4), (200, 136, 8320, A_KM | B_KN, 15), (17, 264, 4096, 0, 8)]


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c[0]}x{c[1]}x{c[2]}-f{c[3]}") for c in SPLITK])
def test_split_k_and_its_reduction(env, case):
    M, N, K, flags, splits = case
    lib = ops.backend().lib
    dtype = F16 if flags == B_KN else BF16
    p = Problem(dtype, M, N, K)
    for epi, bias in ((NONE, False), (BIAS, True), (RESIDUAL, False), (RESIDUAL, True), (ACCUM, False)):
        assert lib.tamd_gemm_workspace_bytes(M, N, K, flags, epi) == splits * M * N * 4  # the split count the case is about
        lds = dict(ldc=N + 16, ldr=N + 8) if epi in (RESIDUAL, ACCUM) else {}
        if epi != RESIDUAL:
            lds.pop("ldr", None)
        got = run(env, p, flags, epi, bias=bias, ws="need", **lds)
        same(got, p.expected(epi, bias=bias), (case, epi, bias))
    if (M, flags) == (264, A_KM | B_KN):  # a workspace one byte short, or off by 8 bytes: the unsplit kernel, the same bits
        for ws in ((0, -1), (8, 0)):
            same(run(env, p, flags, ACCUM, ws=ws), p.expected(ACCUM), (case, "workspace", ws))


@pytest.mark.parametrize("env", [pytest.param("hip", id="hip", marks=pytest.mark.gpu)], indirect=True)
def test_split_k_reduction_second_grid_stride_iteration(env):
    """flags 3, 2304 x 2048 x 2048: 72 tiles cut 3 ways (11 / 11 / 10 stages); M * N / 4 = 1 179 648 vectors exceed the
    reduction's 4096 x 256 threads, so its grid-stride loop runs a second, partly filled iteration.  MI355X only: the CPU
    model would run 216 workgroups of 10 or 11 full 256 x 256 x 64 stages each, about 70 times the largest product of this
    file (seconds there), for one loop bound."""
    M, N, K = 2304, 2048, 2048
    lib = ops.backend().lib
    assert M * N // 4 > 4096 * 256
    assert lib.tamd_gemm_workspace_bytes(M, N, K, 3, NONE) == 3 * M * N * 4
    p = Problem(BF16, M, N, K)
    for epi in (NONE, ACCUM):
        same(run(env, p, A_KM | B_KN, epi, ws="need"), p.expected(epi), ("second iteration", epi))


# ---------------------------------------------------------------------------------------------------- segments, groups
@pytest.mark.parametrize("K", [320, 4096])
def test_segmented_weight_gradient(env, K):
    """tamd_gemm_seg: 512 | 256 | 264 rows, each segment in its own guarded buffer with ldc > N; unsplit (K = 320) and split
    (K = 4096), plain and accumulating."""
    lib, dev = ops.backend().lib, env.device
    rows, N, ldc = (512, 256, 264), 136, 152
    M = sum(rows)
    p = Problem(BF16, M, N, K)
    a, b = operands(p, A_KM | B_KN, dev, lda=M + 8, ldb=N + 24)
    for epi in (NONE, ACCUM):
        need = lib.tamd_gemm_workspace_bytes(M, N, K, 3, epi)
        assert (need > 0) == (K == 4096)
        segs, r0 = [], 0
        for r in rows:
            segs.append(GuardedMatrix(r, N, ldc, BF16, dev, fill=p.C0[r0:r0 + r].to(BF16) if epi == ACCUM else None))
            r0 += r
        cp = (ctypes.c_void_p * 3)(*[s.t.data_ptr() for s in segs])
        sr = (ctypes.c_int64 * 3)(*rows)
        w = scratch(dev, need)
        st = lib.tamd_gemm_seg(ptr(a), ptr(b), cp, sr, 3, N, K, a.stride(0), b.stride(0), ldc, epi, _cabi.TAMD_BF16,
                               w.data_ptr() if need else None, need, stream_of(a))
        sync(dev)
        assert st == 0
        assert all(s.intact() for s in segs), "a segment's guard rows or gap columns were written"
        same(torch.cat([s.t.cpu().double() for s in segs], 0), p.expected(epi), ("seg", K, epi))
    # refusals: a non-last segment that is no multiple of 256 rows; K % 64
    segs = [GuardedMatrix(r, N, ldc, BF16, dev) for r in (264, 512, 256)]
    cp = (ctypes.c_void_p * 3)(*[s.t.data_ptr() for s in segs])
    st = lib.tamd_gemm_seg(ptr(a), ptr(b), cp, (ctypes.c_int64 * 3)(264, 512, 256), 3, N, K, a.stride(0), b.stride(0), ldc,
                           NONE, _cabi.TAMD_BF16, None, 0, stream_of(a))
    assert st == E_SHAPE
    st2 = lib.tamd_gemm_seg(ptr(a), ptr(b), cp, (ctypes.c_int64 * 3)(512, 256, 264), 3, N, K - 32, a.stride(0), b.stride(0),
                            ldc, NONE, _cabi.TAMD_BF16, None, 0, stream_of(a))
    sync(dev)
    assert st2 == E_SHAPE and all(s.untouched() for s in segs)


def group_call(env, probs, flags, epi, dtype, ldcs, with_ws):
    lib, dev = ops.backend().lib, env.device
    ops_ = [operands(p, flags, dev) for p in probs]
    outs = [GuardedMatrix(p.M, p.N, ld, dtype, dev, fill=p.C0.to(dtype) if epi == ACCUM else None) for p, ld in zip(probs, ldcs)]
    pr = (_cabi.GemmProblem * len(probs))()
    for i, (p, (a, b), c) in enumerate(zip(probs, ops_, outs)):
        pr[i] = _cabi.GemmProblem(a.data_ptr(), b.data_ptr(), c.t.data_ptr(), p.M, p.N, p.K, a.stride(0), b.stride(0),
                                  c.full.stride(0))
    need = lib.tamd_gemm_group_workspace_bytes(ctypes.byref(pr), len(probs), flags)
    w = scratch(dev, need)
    st = lib.tamd_gemm_group(ctypes.byref(pr), len(probs), flags, epi, ops._code(ops_[0][0]),
                             w.data_ptr() if with_ws else None, need if with_ws else 0, stream_of(w))
    sync(dev)
    assert st == 0
    for i, (p, c) in enumerate(zip(probs, outs)):
        assert c.intact(), ("group member's guard rows or gap columns were written", i)
        same(c.t.cpu().double(), p.expected(epi), ("group", flags, epi, with_ws, i))
    return need


def test_grouped_launch(env):
    """tamd_gemm_group: three k-major products of 21, 17 and 32 stages (one common range length of 16: splits of 11 + 10,
    9 + 8, 16 + 16); a row-major pair; plain and accumulating; with the workspace and with NULL (unsplit); ldc > n."""
    probs = [Problem(BF16, 264, 136, 1344), Problem(BF16, 128, 72, 1088), Problem(BF16, 72, 264, 2048)]
    for epi in (NONE, ACCUM):
        assert group_call(env, probs, A_KM | B_KN, epi, BF16, (136, 88, 264), True) > 0
    group_call(env, probs[:2], A_KM | B_KN, ACCUM, BF16, (152, 72), False)
    pair = [Problem(F16, 130, 136, 1088), Problem(F16, 72, 264, 1344)]
    for epi in (NONE, ACCUM):
        assert group_call(env, pair, 0, epi, F16, (136, 280), True) > 0
        group_call(env, pair, 0, epi, F16, (144, 264), False)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(env):
    """Each unsupported argument returns its documented status before any launch; the guarded C keeps the sentinel."""
    lib, dev = ops.backend().lib, env.device
    p = Problem(BF16, 64, 72, 64)
    a, b = operands(p, 0, dev, lda=72, ldb=72)
    at, bt = operands(p, A_KM | B_KN, dev)
    r = place(p.R, BF16, dev, 80)
    bias = p.bias.to(BF16).to(dev)
    c = GuardedMatrix(64, 72, 80, BF16, dev)
    ok = dict(A=a, B=b, C=ptr(c.t), bias=None, R=None, M=64, N=72, K=64, lda=72, ldb=72, ldc=80, ldr=0, flags=0, epi=NONE)

    def status(**kw):
        v = dict(ok, **kw)
        A, B, R_, bi = (x.data_ptr() if torch.is_tensor(x) else x for x in (v["A"], v["B"], v["R"], v["bias"]))
        return lib.tamd_gemm(A, B, v["C"], bi, R_, v["M"], v["N"], v["K"], v["lda"], v["ldb"], v["ldc"], v["ldr"], v["flags"],
                             v["epi"], 0, _cabi.TAMD_BF16, stream_of(a))

    assert status(K=60) == E_SHAPE                                        # K % 8 with a row-major operand ...
    assert status(K=60, flags=B_KN, B=bt, ldb=72) == E_SHAPE              # ... with one row-major operand
    assert status(K=60, flags=A_KM, A=at, lda=64) == E_SHAPE
    assert status(N=68) == E_SHAPE                                        # N % 8
    assert status(M=60, flags=A_KM | B_KN, A=at, B=bt, lda=64) == E_SHAPE  # M % 8 with a k-major A
    for ld in ("lda", "ldb", "ldc"):
        assert status(**{ld: 76}) == E_SHAPE                              # ld % 8
    assert status(epi=RESIDUAL, R=r, ldr=76) == E_ALIGN
    assert status(A=a.data_ptr() + 8) == E_ALIGN                          # 16-byte alignment of every pointer
    assert status(B=b.data_ptr() + 8) == E_ALIGN
    assert status(C=ptr(c.t) + 8) == E_ALIGN
    assert status(epi=RESIDUAL, R=r.data_ptr() + 8, ldr=80) == E_ALIGN
    assert status(epi=BIAS, bias=bias.data_ptr() + 4) == E_ALIGN          # (the bias: 8 bytes)
    assert status(epi=RESIDUAL) == E_NULL                                 # TAMD_EPI_RESIDUAL without R
    assert status(epi=BIAS) == E_NULL
    assert status(epi=7) != 0
    assert lib.tamd_gemm_colscale(ptr(a), ptr(b), ptr(c.t), None, 64, 72, 64, 72, 72, 80, 0, 6, 0.5, _cabi.TAMD_BF16,
                                  stream_of(a)) == E_SHAPE  # scale_cols % 4
    sync(dev)
    assert c.untouched()
    assert status() == 0  # the same call without any of it runs, and writes
    sync(dev)
    assert c.intact()
    same(c.t.cpu().double(), p.expected(NONE), "the accepted call")


# ---------------------------------------------------------------------------------------------------- family R
def random_case(env, name, M, N, K, flags, sched, dtype, ws=None):
    g = torch.Generator().manual_seed(M + N + K + flags)
    A = torch.randn(M, K, generator=g).to(dtype).double()
    B = (torch.randn(N, K, generator=g) * 0.1).to(dtype).double()
    shim = type("Shim", (), dict(dtype=dtype, M=M, N=N, K=K, A=A, B=B))
    got = run(env, shim, flags, NONE, sched=sched, ws=ws, lda=(M if flags & A_KM else K) + 8, ldc=N + 8)
    ref = A @ B.t()
    s = U2 * K * (A.abs() @ B.abs().t())  # K terms in any order
    check(name, got, ref, s, dtype, group="gemm_elements")


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_operands_on_every_arm(env, dtype):
    """Full-mantissa operands (randn, as the norm-gated tests of test_kernels.py use) on every kernel arm and layout."""
    for flags in LAYOUTS:
        random_case(env, f"pp.f{flags}", 200, 136, 136, flags, "pp", dtype)
        random_case(env, f"fl.f{flags}", 200, 136, 192, flags, "fl", dtype)
    random_case(env, "sm", 130, 136, 192, 0, "sm", dtype)
    random_case(env, "gemv.valu", 4, 264, 520, 0, "auto", dtype)
    random_case(env, "gemv.mfma", 16, 264, 520, 0, "auto", dtype)
    random_case(env, "splitk", 264, 136, 2112, A_KM | B_KN, "auto", dtype, ws="need")


# ---------------------------------------------------------------------------------------------------- approximated epilogues
ACT_ERF, ACT_TANH, ACT_QUICK, ACT_SILU = 1, 2, 3, 4


def sigmoid_terms(x, c=1.0):
    """sigmoid(c x) in float64 and what fp32 may add to it: the product c x and the exponential's argument scaling move
    the argument by 2^-23 |c x| each (sigmoid' = sig (1 - sig)); the exponential, the sum and the quotient: 2^-23 sig each"""
    sig = torch.sigmoid(c * x)
    return sig, U2 * (sig * (1 - sig) * (c * x).abs() * 2 + 3 * sig)


def act_reference(act, x):
    """-> (float64 activation of the reference's formula, s, torch's fp32 operator on x)"""
    xf = x.float()
    if act == ACT_ERF:  # x * 0.5 * (1 + erf(x / sqrt 2)): the quotient moves erf by <= 2^-23 / 2, erf itself, the sum, two products
        e = torch.erf(x / np.sqrt(2.0))
        ref = x * 0.5 * (1 + e)
        s = U2 * (x.abs() / 2 * (0.5 + e.abs() + 1 + e.abs()) + 2 * ref.abs())
        f32 = torch.nn.functional.gelu(xf)
    elif act == ACT_TANH:  # 0.5 x (1 + tanh(k (x + c x^3))): five operations in the argument u, tanh, the sum, two products
        u = 0.7978845608028654 * (x + 0.044715 * x ** 3)
        t = torch.tanh(u)
        ref = 0.5 * x * (1 + t)
        s = U2 * (x.abs() / 2 * ((1 - t * t) * 5 * u.abs() + t.abs() + 1 + t.abs()) + 2 * ref.abs())
        f32 = torch.nn.functional.gelu(xf, approximate="tanh")
    else:  # x * sigmoid(c x), and the product
        c = 1.702 if act == ACT_QUICK else 1.0
        sig, es = sigmoid_terms(x, c)
        ref = x * sig
        s = x.abs() * es + U2 * ref.abs()
        f32 = xf * torch.sigmoid(c * xf) if act == ACT_QUICK else torch.nn.functional.silu(xf)
    return ref, s, f32.double()


def floor_of(f32_result, ref, s, dtype):
    """torch's fp32 operator, rounded to T, in the unit of the check"""
    return ((rnd(f32_result, dtype) - ref).abs() / (ulp(ref, dtype) + s)).max().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sched", ["pp", "fl", "sm"])
def test_bias_activation_epilogue(env, sched, dtype):
    """C = rT(act(rT(acc + b))) at 130 x 136 (ragged), K = 64, ldc > N: the pre-activation is the BIAS chain (asserted bit-exact
    through that epilogue first), the activation is checked per element on it."""
    p = act_problem(dtype, 130, 136, 64)
    bias = torch.randint(-64, 65, (p.N,), generator=torch.Generator().manual_seed(5)).double() * 2.0 ** -6
    p.check_inputs(p.acc + bias)
    pre = rnd(p.acc + bias, dtype)
    assert 5.0 < pre.abs().max().item() < 16.0 and (pre.abs() < 1).double().mean().item() > 0.2
    same(run(env, p, 0, BIAS, bias_t=bias, sched=sched, ldc=152), pre, (sched, "pre-activation"))
    for act, name in ((ACT_ERF, "gelu_erf"), (ACT_TANH, "gelu_tanh"), (ACT_QUICK, "quick_gelu"), (ACT_SILU, "silu")):
        got = run(env, p, 0, BIAS_ACT, bias_t=bias, sched=sched, act=act, ldc=152)
        ref, s, f32 = act_reference(act, pre)
        check(f"bias_act.{name}", got, ref, s, dtype, group="gemm_elements", own_floor=floor_of(f32, ref, s, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [5, 130])
def test_swiglu_epilogue(env, M, dtype):
    """tamd_gemm_swiglu at I = 72 (no multiple of the 128 features of a tile) and I = 136 (a second, 8-wide tile), M = 130
    (tile kernel, ragged) and M = 5 (the weight-streaming kernel), leading dimensions larger than the widths, with GU and
    with GU == NULL:  GU = rT(acc) bit-exact,  ACT = rT(rT(silu(gate)) * up) per element."""
    lib, dev = ops.backend().lib, env.device
    for I in (72, 136):
        K = 128
        p = act_problem(dtype, M, 2 * I, K)  # X [M, K] . [gate rows ; up rows]^T: N = 2 I
        p.check_inputs(p.acc)
        gu = rnd(p.acc, dtype)
        g, u = gu[:, :I], gu[:, I:]
        x, w = operands(p, 0, dev, lda=K + 8, ldb=K + 16)
        sig, es = sigmoid_terms(g)
        silu = g * sig
        ref = silu * u
        # silu's terms, its rounding to T (scaled by up), the product
        s = (g.abs() * es + U2 * silu.abs() + ulp(silu, dtype)) * u.abs() + U2 * ref.abs()
        chain = rnd(rnd(silu, dtype) * u, dtype)
        f32 = rnd(torch.nn.functional.silu(g.float()).double(), dtype) * u
        acts = []
        for with_gu in (True, False):
            GU = GuardedMatrix(M, 2 * I, 2 * I + 24, dtype, dev) if with_gu else None
            ACT = GuardedMatrix(M, I, I + 8, dtype, dev)
            st = lib.tamd_gemm_swiglu(ptr(x), ptr(w), ptr(GU.t) if with_gu else None, ptr(ACT.t), M, I, K, x.stride(0), w.stride(0),
                                      2 * I + 24, I + 8, ops._code(x), stream_of(x))
            sync(dev)
            assert st == 0 and ACT.intact() and (GU is None or GU.intact()), (M, I, with_gu)
            if with_gu:
                same(GU.t.cpu().double(), gu, ("swiglu GU", M, I))
            check("swiglu.act", ACT.t, ref, s, dtype, chain=chain, group="gemm_elements", own_floor=floor_of(f32, ref, s, dtype))
            acts.append(ACT.t.cpu())
        assert torch.equal(acts[0], acts[1])  # GU == NULL changes nothing about ACT


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_backward_epilogue(env, dtype):
    """tamd_gemm_swiglu_bwd at M = 130, I = 72 and 136, K = 64: d_act = rT(acc) exactly, then
    d_gate = rT(rT(d_act * up) * silu'(gate)),  d_up = rT(d_act * rT(silu(gate)))  per element; GU holds eighths over [-6, 6]."""
    lib, dev = ops.backend().lib, env.device
    M, K = 130, 64
    for I in (72, 136):
        p = act_problem(dtype, M, I, K)
        p.check_inputs(p.acc)
        d = rnd(p.acc, dtype)
        gen = torch.Generator().manual_seed(I)
        gu = torch.randint(-48, 49, (M, 2 * I), generator=gen).double() / 8
        g, u = gu[:, :I], gu[:, I:]
        dy, wd = operands(p, B_KN, dev, lda=K + 8, ldb=I + 16)
        GUd = place(gu, dtype, dev, 2 * I + 8)
        out = GuardedMatrix(M, 2 * I, 2 * I + 24, dtype, dev)
        st = lib.tamd_gemm_swiglu_bwd(ptr(dy), ptr(wd), ptr(GUd), ptr(out.t), M, I, K, dy.stride(0), wd.stride(0), GUd.stride(0),
                                      2 * I + 24, ops._code(dy), stream_of(dy))
        sync(dev)
        assert st == 0 and out.intact(), (I,)
        got = out.t.cpu().double()
        sig, es = sigmoid_terms(g)
        # d_up = d * rT(silu(g)): silu's terms and its rounding, scaled by d; the product
        silu = g * sig
        ref_up = d * silu
        s_up = (g.abs() * es + U2 * silu.abs() + ulp(silu, dtype)) * d.abs() + U2 * ref_up.abs()
        gf = g.float()
        sf = torch.sigmoid(gf)
        f_up = d * rnd((gf * sf).double(), dtype)
        check("swiglu_bwd.d_up", got[:, I:], ref_up, s_up, dtype, chain=rnd(d * rnd(silu, dtype), dtype), group="gemm_elements",
              own_floor=floor_of(f_up, ref_up, s_up, dtype))
        # d_gate = rT(d * u) * silu'(g), silu' = sig * (1 + g * (1 - sig)): 1 - sig, its product with g, the sum with 1, the
        # product with sig -- each carries what came before plus 2^-23 of its own magnitude
        oms = 1 - sig
        inner = 1 + g * oms
        ds = sig * inner
        e_oms = es + U2 * oms.abs()
        e_in = g.abs() * e_oms + U2 * (g * oms).abs() + U2 * inner.abs()
        e_ds = sig * e_in + inner.abs() * es + U2 * ds.abs()
        du = d * u  # (exact in fp32: 8 x 8 or 11 x 11 bits)
        ref_g = du * ds
        s_g = rnd(du, dtype).abs() * e_ds + ulp(du, dtype) * ds.abs() + U2 * ref_g.abs()
        f_g = rnd(du, dtype) * (sf * (1 + gf * (1 - sf))).double()
        check("swiglu_bwd.d_gate", got[:, :I], ref_g, s_g, dtype, chain=rnd(rnd(du, dtype) * ds, dtype), group="gemm_elements",
              own_floor=floor_of(f_g, ref_g, s_g, dtype))
