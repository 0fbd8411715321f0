"""The decode-step experts (csrc/gemv_moe.inc: tamd_moe_gemv_swiglu, tamd_moe_gemv_down, torch.ops.tamd.moe_experts_decode),
element by element, on the SAME small shapes under the CPU execution model (`emu`) and on the MI355X (`hip`).

Buffers are pair-major: row p = t * k + j of act / ys belongs to pair (t, j), whose expert is top_k_index[t, j].

Geometry (E = 6, top-2 unless said).  "t1": one token.  "t5": five tokens whose pairs give per-expert counts of exactly
[0, 1, 4, 5, 0, 0] -- no rows, one row, exactly one full chunk of kGemvValuRows = 4 rows, one row into a second chunk -- no token
naming an expert twice.  "t5_sentinel": the same with every 7th id set to E and one to -1.  "big": E = 128, top-8, 16 tokens,
random ids (128 pairs: two ballot words) at H = 64, I = 8.  Widths on "t5": H in {64, 128, 576} (576: a second iteration of the
512-element K step with 8 live lanes), I in {8, 136, 520} (520 as K of the down product: one live lane in the second
iteration; 8: less than one workgroup's features), ldact > I everywhere, bf16 and fp16.

Values.  Operand family E of tests/test_gemm_elements.py (integers times a power of two, every fp32 sum an integer multiple
of one unit below 2^24 units: summation order cannot matter), the same input conditions asserted before a kernel runs.
    gate|up   act = rT(rT(silu(rT(g))) * rT(u)) per element under the gate rule of test_swiglu_epilogue
    down      ys  = rT(acc) and out = rT(sum_j r32(w * f32(ys))) bit for bit (torch.equal), w in fp32 and in T
The expected values are float64 chains, never another kernel's output; the routed path's act is compared with the decode
path's as a cross-check only.  One random-normal case per product goes through kernel_checks.check with
s = 2^-23 K sum_k |a_k b_k|.  Outputs live inside sentinel-filled buffers: the rows of sentinel pairs keep the fill, refused
calls leave everything untouched."""
import numpy as np
import pytest
import torch

from kernel_checks import BF16, F16, SENT, GuardedMatrix, check, rnd, ulp
from test_gemm_elements import U2, amplitude, floor_of, place, ptr, representable_and_ties, same, sigmoid_terms, stream_of, sync
from transformers_amd import _cabi, experts, ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]
E_DTYPE, E_SHAPE, E_ALIGN, E_NULL = -1, -2, -3, -4
MAX_TOKENS = 16  # TAMD_MOE_GEMV_MAX_TOKENS (include/tamd.h)


# ---------------------------------------------------------------------------------------------------- geometries
def index_of(name):
    """-> (top_k_index int64 [T, k], E)"""
    if name == "t1":
        return torch.tensor([[4, 2]], dtype=torch.int64), 6
    if name.startswith("t5"):
        idx = torch.tensor([[2, 3], [3, 2], [3, 1], [2, 3], [3, 2]], dtype=torch.int64)
        if name.endswith("sentinel"):
            flat = idx.reshape(-1).clone()
            flat[5::7] = 6
            flat[3] = -1
            idx = flat.view(5, 2)
        return idx, 6
    assert name == "big"
    return torch.randint(0, 128, (16, 8), generator=torch.Generator().manual_seed(128), dtype=torch.int64), 128


def test_the_geometries_are_the_ones_the_kernels_must_meet():
    idx, E = index_of("t5")
    assert torch.bincount(idx.reshape(-1), minlength=E).tolist() == [0, 1, 4, 5, 0, 0]
    assert all(a != b for a, b in idx.tolist())
    s, _ = index_of("t5_sentinel")
    assert ((s < 0) | (s >= E)).sum().item() == 2 and (s == -1).sum().item() == 1
    big, _ = index_of("big")
    assert big.numel() == 128 and torch.bincount(big.reshape(-1), minlength=128).max().item() >= 3


class Case:
    """Exact operands of one product over the pairs of a geometry: A [rows, K] (gate|up: one row per TOKEN; down: one row per
    PAIR), one B [N, K] per expert; acc[p] = A[row of p] . B[e_p]^T for the valid pairs (zeros elsewhere, never compared)."""

    def __init__(self, name, dtype, K, N, per_pair, unit=None):
        self.idx, self.E = index_of(name)
        self.T, self.k = self.idx.shape
        self.S = self.T * self.k
        self.flat = self.idx.reshape(-1)
        self.valid = (self.flat >= 0) & (self.flat < self.E)
        amp = amplitude(dtype, K)
        assert K * amp * amp < 2 ** 24  # (i)
        if unit is None:  # pre-activations over about [-8, 8]
            unit = 2.0 ** int(round(np.log2(2.0 / (np.sqrt(K) * amp * (amp + 1) / 3.0))))
        sa = 2.0 ** -3
        rows = self.S if per_pair else self.T
        for seed in range(64):
            g = torch.Generator().manual_seed(1000 * seed + 7 * K + 3 * N + self.S)
            a = torch.randint(-amp, amp + 1, (rows, K), generator=g).double()
            b = torch.randint(-amp, amp + 1, (self.E, N, K), generator=g).double()
            acc = torch.zeros(self.S, N, dtype=torch.float64)
            for p in range(self.S):
                if self.valid[p]:
                    acc[p] = b[self.flat[p]] @ a[p if per_pair else p // self.k]
            live = acc[self.valid]
            hard, ties = representable_and_ties(live, dtype)
            if K < 32 or live.numel() < 512 or (hard >= 0.15 and ties >= 0.05):  # (iii): a property of the inputs alone
                break
        else:
            raise AssertionError("no operands with 15 % unrepresentable sums and 5 % ties")
        self.u, self.A, self.B, self.acc = unit, a * sa, b * (unit / sa), acc * unit
        assert torch.equal(self.A.to(dtype).double(), self.A) and torch.equal(self.B.to(dtype).double(), self.B)
        assert acc.abs().max().item() < 2 ** 24  # every fp32 sum is exact
        assert self.acc.abs().max().item() < float(torch.finfo(dtype).max)  # (ii)


_CASES = {}


def case_of(*key, **kw):
    """computed once per session and shared (never modified)"""
    k = key + tuple(sorted(kw.items()))
    if k not in _CASES:
        _CASES[k] = Case(*key, **kw)
    return _CASES[k]


def place3(t64, dtype, dev):
    return t64.to(dtype).to(dev).contiguous()


def swiglu_call(env, c, x, wgu, ACT, H, inter, ldact, *, tokens=None, experts_=None, code=None, x_ptr=None, idx_ptr=None):
    lib = ops.backend().lib
    idx = c.idx.to(env.device)
    st = lib.tamd_moe_gemv_swiglu(ptr(x) if x_ptr is None else x_ptr, ptr(idx) if idx_ptr is None else idx_ptr, ptr(wgu), ptr(ACT),
                                  c.T if tokens is None else tokens, c.k, c.E if experts_ is None else experts_, H, inter, ldact,
                                  ops._code(x) if code is None else code, stream_of(x))
    sync(env.device)
    return st


def down_call(env, c, act, wd, w, YS, OUT, H, inter, ldact, *, tokens=None, experts_=None, code=None, w_ptr=None):
    lib = ops.backend().lib
    idx = c.idx.to(env.device)
    st = lib.tamd_moe_gemv_down(ptr(act), ptr(idx), ptr(wd), ptr(w) if w_ptr is None else w_ptr, ptr(YS), ptr(OUT),
                                c.T if tokens is None else tokens, c.k, c.E if experts_ is None else experts_, H, inter, ldact,
                                ops._code(w), ops._code(act) if code is None else code, stream_of(act))
    sync(env.device)
    return st


SHAPES = [("t1", 128, 136), ("t5", 128, 136), ("t5_sentinel", 128, 136), ("big", 64, 8), ("t5", 64, 8), ("t5", 576, 136),
          ("t5", 128, 520)]


# ---------------------------------------------------------------------------------------------------- gate|up + SiLU * up
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,H,inter", SHAPES)
def test_gate_up_swiglu_per_element(env, name, H, inter, dtype):
    dev = env.device
    c = case_of(name, dtype, H, 2 * inter, False)
    gu = rnd(c.acc, dtype)[c.valid]
    g, u = gu[:, :inter], gu[:, inter:]
    assert g.abs().max().item() < 32.0
    if g.numel() >= 1000:
        assert 5.0 < g.abs().max().item() and (g.abs() < 1).double().mean().item() > 0.2
    sig, es = sigmoid_terms(g)
    silu = g * sig
    ref = silu * u
    s = (g.abs() * es + U2 * silu.abs() + ulp(silu, dtype)) * u.abs() + U2 * ref.abs()
    chain = rnd(rnd(silu, dtype) * u, dtype)
    f32 = rnd(torch.nn.functional.silu(g.float()).double(), dtype) * u
    ldact = inter + 8
    x, wgu = place(c.A, dtype, dev), place3(c.B, dtype, dev)
    ACT = GuardedMatrix(c.S, inter, ldact, dtype, dev)
    assert swiglu_call(env, c, x, wgu, ACT.t, H, inter, ldact) == 0 and ACT.intact()
    valid = c.valid.to(dev)
    assert bool((ACT.t[~valid] == SENT).all())  # the rows of sentinel pairs are not written
    check("moe_decode.act", ACT.t[valid], ref, s, dtype, chain=chain, group="moe_decode", own_floor=floor_of(f32, ref, s, dtype))
    if name == "t5_sentinel":
        assert (~c.valid).sum().item() == 2
    if name == "t5" and H % 64 == 0 and (H, inter) == (128, 136):
        # cross-check only: on exact operands the routed GEMM's way out gives the same act bits, row pos[p] for pair p
        count, offset, pos, tiles = ops.raw_moe_route(c.idx.to(dev), c.E)
        xs = ops.raw_moe_gather(x, pos, count, offset)
        _, routed = ops.raw_gemm_routed(xs, wgu, offset, tiles, mode=ops.ROUTED_SWIGLU, need_gu=False)
        sync(dev)
        assert torch.equal(routed[pos.reshape(-1).long()].cpu(), ACT.t.cpu())


# ---------------------------------------------------------------------------------------------------- down + combine
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,H,inter", SHAPES)
def test_down_and_combine_are_the_documented_chain(env, name, H, inter, dtype):
    """ys[p] = rT(act[p] . Wd[e]^T) and out[t] = rT(sum_j r32(w[t, j] * f32(ys[t k + j]))): w = integers of [1, 15] times 2^-4, so
    every product is exact in fp32 (4 + 8 / 11 bits) and every partial sum a multiple of u / 16 below 2^24 of them (asserted)."""
    dev = env.device
    c = case_of(name, dtype, inter, H, True, unit=2.0 ** -5)
    ys = rnd(c.acc, dtype)
    w = torch.randint(1, 16, (c.T, c.k), generator=torch.Generator().manual_seed(4)).double() * 2.0 ** -4
    terms = (w.reshape(-1, 1) * ys * c.valid[:, None]).view(c.T, c.k, H)
    assert torch.equal(terms.float().double(), terms) and terms.abs().sum(1).max().item() < 2 ** 24 * c.u / 16
    want = rnd(terms.sum(1), dtype)
    if inter >= 32:
        hard, _ = representable_and_ties(terms.sum(1), dtype)
        assert hard >= 0.15, hard  # the final rounding is exercised
    ldact = inter + 8
    act, wd = place(c.A, dtype, dev, ldact), place3(c.B, dtype, dev)
    valid = c.valid.to(dev)
    for wt in (w.float(), w.to(dtype)):
        YS, OUT = GuardedMatrix(c.S, H, H, dtype, dev), GuardedMatrix(c.T, H, H, dtype, dev)
        assert down_call(env, c, act, wd, wt.to(dev), YS.t, OUT.t, H, inter, ldact) == 0 and YS.intact() and OUT.intact()
        assert bool((YS.t[~valid] == SENT).all())
        same(YS.t[valid].cpu().double(), ys[c.valid], (name, "ys", wt.dtype))
        same(OUT.t.cpu().double(), want, (name, "out", wt.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_operands(env, dtype):
    """Full-mantissa operands, one case per product ("t5_sentinel", H = 128, I = 136): every element within the gate of
    kernel_checks.check with s = 2^-23 K sum |a b|; the gate|up product is read off act = silu(g) * u with up rows that make
    u = 1 exactly (a single one in x's first column), which leaves silu(g): its terms are added to s."""
    dev, (idx, E), H, inter = env.device, index_of("t5_sentinel"), 128, 136
    T, k = idx.shape
    flat = idx.reshape(-1)
    valid = (flat >= 0) & (flat < E)
    g = torch.Generator().manual_seed(23)
    c = case_of("t5_sentinel", dtype, H, 2 * inter, False)  # (for the call helper: the geometry)
    # down
    act = torch.randn(T * k, inter, generator=g).to(dtype).double()
    wd = (torch.randn(E, H, inter, generator=g) * 0.1).to(dtype).double()
    w = torch.ones(T, k)
    YS, OUT = GuardedMatrix(T * k, H, H, dtype, dev), GuardedMatrix(T, H, H, dtype, dev)
    assert down_call(env, c, place(act, dtype, dev, inter + 8), place3(wd, dtype, dev), w.to(dev), YS.t, OUT.t, H, inter, inter + 8) == 0
    assert YS.intact() and OUT.intact()
    for p in torch.nonzero(valid).reshape(-1).tolist():
        e = int(flat[p])
        check("moe_decode.down", YS.t[p:p + 1], (wd[e] @ act[p])[None], U2 * inter * (wd[e].abs() @ act[p].abs())[None], dtype,
              group="moe_decode")
    # gate|up: x[:, 0] = 1 and the up rows = e_0, so u = 1 and act = rT(rT(silu(rT(g))))
    x = torch.randn(T, H, generator=g).to(dtype).double()
    x[:, 0] = 1.0
    wgu = (torch.randn(E, 2 * inter, H, generator=g) * 0.1).to(dtype).double()
    wgu[:, inter:, :] = 0.0
    wgu[:, inter:, 0] = 1.0
    ACT = GuardedMatrix(T * k, inter, inter + 8, dtype, dev)
    assert swiglu_call(env, c, place(x, dtype, dev), place3(wgu, dtype, dev), ACT.t, H, inter, inter + 8) == 0 and ACT.intact()
    for p in torch.nonzero(valid).reshape(-1).tolist():
        e, t = int(flat[p]), p // k
        gate = wgu[e, :inter] @ x[t]
        sg = U2 * H * (wgu[e, :inter].abs() @ x[t].abs())
        gr = rnd(gate, dtype)
        sig, es = sigmoid_terms(gr)
        ref = gr * sig
        # what moves the rounded gate (s of the product + its rounding) times |silu'| <= 1.1, then silu's own terms
        s = 1.1 * (sg + ulp(gate, dtype)) + gr.abs() * es + U2 * ref.abs()
        check("moe_decode.gate", ACT.t[p:p + 1], ref[None], s[None], dtype, group="moe_decode")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refused_calls_leave_the_buffers_untouched(env):
    """T = 0, T = MAX + 1, fp32, H % 64, I % 8, E = 257, a NULL operand: the code, and no launch."""
    dev, dtype, H, inter = env.device, BF16, 128, 136
    c = case_of("t5", dtype, H, 2 * inter, False)
    ldact = inter + 8
    x = torch.zeros(MAX_TOKENS + 1, H, dtype=dtype, device=dev)
    wgu = torch.zeros(c.E, 2 * inter, H, dtype=dtype, device=dev)
    wd = torch.zeros(c.E, H, inter, dtype=dtype, device=dev)
    w = torch.ones(MAX_TOKENS + 1, c.k, device=dev)
    ACT = GuardedMatrix((MAX_TOKENS + 1) * c.k, inter, ldact, dtype, dev)
    YS, OUT = GuardedMatrix((MAX_TOKENS + 1) * c.k, H, H, dtype, dev), GuardedMatrix(MAX_TOKENS + 1, H, H, dtype, dev)
    act_in = torch.zeros((MAX_TOKENS + 1) * c.k, ldact, dtype=dtype, device=dev)[:, :inter]

    def refused(want, H_=H, inter_=inter, **kw):
        st = swiglu_call(env, c, x, wgu, ACT.t, H_, inter_, ldact, **kw)
        assert st == want, ("swiglu", st, want, kw)
        kw.pop("x_ptr", None), kw.pop("idx_ptr", None)
        st = down_call(env, c, act_in, wd, w, YS.t, OUT.t, H_, inter_, ldact, **kw)
        assert st == want, ("down", st, want, kw)
        assert ACT.untouched() and YS.untouched() and OUT.untouched()

    refused(E_SHAPE, tokens=0)
    refused(E_SHAPE, tokens=MAX_TOKENS + 1)
    refused(E_DTYPE, code=_cabi.TAMD_F32)
    refused(E_SHAPE, H_=96)
    refused(E_SHAPE, inter_=132)
    refused(E_SHAPE, experts_=257)
    lib = ops.backend().lib
    idx = c.idx.to(dev)
    s = stream_of(x)
    assert lib.tamd_moe_gemv_swiglu(None, ptr(idx), ptr(wgu), ptr(ACT.t), c.T, c.k, c.E, H, inter, ldact, 0, s) == E_NULL
    assert lib.tamd_moe_gemv_swiglu(ptr(x), None, ptr(wgu), ptr(ACT.t), c.T, c.k, c.E, H, inter, ldact, 0, s) == E_NULL
    assert lib.tamd_moe_gemv_down(ptr(act_in), ptr(idx), ptr(wd), None, ptr(YS.t), ptr(OUT.t), c.T, c.k, c.E, H, inter, ldact, 2, 0, s) == E_NULL
    assert lib.tamd_moe_gemv_down(ptr(act_in), ptr(idx), None, ptr(w), ptr(YS.t), ptr(OUT.t), c.T, c.k, c.E, H, inter, ldact, 2, 0, s) == E_NULL
    assert lib.tamd_moe_gemv_swiglu(ptr(x) + 2, ptr(idx), ptr(wgu), ptr(ACT.t), c.T, c.k, c.E, H, inter, ldact, 0, s) == E_ALIGN
    # more pairs than the scan takes (TAMD_MOE_GEMV_MAX_PAIRS = 256): 16 tokens x top-17
    assert lib.tamd_moe_gemv_swiglu(ptr(x), ptr(idx), ptr(wgu), ptr(ACT.t), 16, 17, c.E, H, inter, ldact, 0, s) == E_SHAPE
    sync(dev)
    assert ACT.untouched() and YS.untouched() and OUT.untouched()


# ---------------------------------------------------------------------------------------------------- the op and its dispatch
def op_operands(dtype, dev, T=2):
    """operands of the whole block at H = 128, I = 136, E = 6, top-2 on which both products are exact in any summation order:
    x and gate_up as in the gate|up cases; every row of down_proj holds ONE nonzero, +-1 or +-1/2, so ys[p, h] is one act
    element times a power of two; w integers of [1, 15] times 2^-4 (w * ys: 4 + 8 / 11 bits, exact in fp32)"""
    H, inter, E, k = 128, 136, 6, 2
    g = torch.Generator().manual_seed(31)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    amp = amplitude(dtype, H)
    unit = 2.0 ** int(round(np.log2(2.0 / (np.sqrt(H) * amp * (amp + 1) / 3.0))))
    x = torch.randint(-amp, amp + 1, (T, H), generator=g).double() * 2.0 ** -3
    wgu = torch.randint(-amp, amp + 1, (E, 2 * inter, H), generator=g).double() * (unit * 8)
    wd = torch.zeros(E, H, inter, dtype=torch.float64)
    col = torch.randint(0, inter, (E, H, 1), generator=g)
    val = torch.tensor([-1.0, -0.5, 0.5, 1.0], dtype=torch.float64)[torch.randint(0, 4, (E, H, 1), generator=g)]
    wd.scatter_(2, col, val)
    w = torch.randint(1, 16, (T, k), generator=g).double() * 2.0 ** -4
    return idx, x, wgu, wd, w


def op_reference(idx, x, wgu, wd, w, dtype, act):
    """the chain from the op's OWN act bits on (the SiLU is approximated: act is checked per element above): ys = rT(act . Wd^T)
    (one nonzero term per sum), out = rT(sum_j r32(w ys)) with the fp32 additions done in fp32, j ascending"""
    T, k = idx.shape
    ys = rnd(torch.stack([wd[idx.reshape(-1)[p]] @ act[p] for p in range(T * k)]), dtype)
    terms = (w.reshape(-1, 1) * ys).view(T, k, -1)
    assert torch.equal(terms.float().double(), terms)
    acc = torch.zeros(T, terms.shape[2], dtype=torch.float32)
    for j in range(k):
        acc = acc + terms[:, j].float()
    return rnd(acc.double(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_at_two_tokens(env, dtype):
    """torch.ops.tamd.moe_experts_decode at T = 2: act through tamd_moe_gemv_swiglu on the same operands (checked per element by
    the cases above), then the float64 chain of the down product and the combine on those act bits, bit for bit."""
    dev = env.device
    idx, x, wgu, wd, w = op_operands(dtype, dev)
    dx, dwgu, dwd, dw = (t.to(dtype).to(dev) for t in (x, wgu, wd, w))
    didx = idx.to(dev)
    got = torch.ops.tamd.moe_experts_decode(dx, didx, dw, dwgu, dwd)
    act = torch.empty(4, 136, dtype=dtype, device=dev)
    st = ops.backend().lib.tamd_moe_gemv_swiglu(ptr(dx), ptr(didx), ptr(dwgu), ptr(act), 2, 2, 6, 128, 136, 136, ops._code(dx), stream_of(dx))
    sync(dev)
    assert st == 0
    same(got.cpu().double(), op_reference(idx, x, wgu, wd, w, dtype, act.cpu().double()), "moe_experts_decode")
    # fp32 weights: the same bits
    assert torch.equal(torch.ops.tamd.moe_experts_decode(dx, didx, dw.float(), dwgu, dwd), got)


def test_op_opcheck(env):
    from torch.library import opcheck

    dev = env.device
    idx, x, wgu, wd, w = op_operands(BF16, dev)
    args = (x.to(BF16).to(dev), idx.to(dev)) + tuple(t.to(BF16).to(dev) for t in (w, wgu, wd))
    opcheck(torch.ops.tamd.moe_experts_decode, args, test_utils=("test_schema", "test_faketensor"))


def test_dispatch_through_moe_experts(env, monkeypatch):
    """ops.moe_experts takes the decode op at T = 2 without grad; the routed GEMM when an input requires grad, above the cut
    and under TAMD_MOE_GEMV=0 -- observed through experts.decode_call_count() -- with the same result either way (the paths
    differ in fp32 summation order only: exact operands, the same bits)."""
    dev, dtype = env.device, BF16
    assert hasattr(torch.ops.tamd, "moe_experts_decode")
    monkeypatch.delenv("TAMD_MOE_GEMV", raising=False)
    idx, x, wgu, wd, w = op_operands(dtype, dev)
    dx, dwgu, dwd, dw = (t.to(dtype).to(dev) for t in (x, wgu, wd, w))
    didx = idx.to(dev)
    experts.decode_call_count(reset=True)
    with torch.no_grad():
        a = ops.moe_experts(dx, didx, dw, dwgu, dwd)
    assert experts.decode_call_count() == 1
    # a leaf that requires grad -> the differentiable op
    xg = dx.clone().requires_grad_(True)
    b = ops.moe_experts(xg, didx, dw, dwgu, dwd)
    assert experts.decode_call_count() == 1 and b.grad_fn is not None
    # ... but not under no_grad
    with torch.no_grad():
        ops.moe_experts(xg, didx, dw, dwgu, dwd)
    assert experts.decode_call_count() == 2
    # TAMD_MOE_GEMV=0
    monkeypatch.setenv("TAMD_MOE_GEMV", "0")
    with torch.no_grad():
        c = ops.moe_experts(dx, didx, dw, dwgu, dwd)
    assert experts.decode_call_count() == 2
    monkeypatch.delenv("TAMD_MOE_GEMV")
    # above the cut
    T = ops.moe_decode_cut() + 1
    idx2, x2, _, _, w2 = op_operands(dtype, dev, T=T)
    with torch.no_grad():
        d = ops.moe_experts(x2.to(dtype).to(dev), idx2.to(dev), w2.to(dtype).to(dev), dwgu, dwd)
    assert experts.decode_call_count() == 2 and d.shape == (T, 128)
    assert 1 <= ops.moe_decode_cut() <= MAX_TOKENS
    assert torch.equal(a, b.detach()) and torch.equal(a, c)
    assert experts.decode_call_count(reset=True) == 2 and experts.decode_call_count() == 0
