"""The router kernels (csrc/moe_router.inc: tamd_moe_router_fwd, tamd_moe_router_bwd, torch.ops.tamd.moe_router), element by
element, on the SAME shapes under the CPU execution model (`emu`) and on the MI355X (`hip`).

Layout under test: one wave per token, four tokens per 256-thread workgroup, expert id = r * 64 + lane (r < 1, 2 or 4 registers
per lane).  T in {1, 5, 67}: one wave; a ragged second workgroup; many workgroups and a ragged last one.  (E, k) covers one, two
and four registers per lane, E = 64 / 65 and 255 / 256 on either side of a register boundary, k = 1, k = E and k = 16.  lde > E
everywhere (lde = E + 3: rows start at odd element offsets; the gap columns of the logits hold NaN).

Expected values are float64 evaluations of the chains of include/tamd.h from the stored logits -- never another kernel's
output; expected indices are a STABLE descending sort of the logits (ties: the lower id).  Gates:

    forward    |w - w64| <= B w64 + 2^-126 (+ half an ulp of T at w64 when the weights are stored in T)
    backward   kernel_checks.check with s = B' sum_j |g_j| w_j per row; unselected entries under `norm` exactly +0
    B  = MULT * max(2^-23, the relative error of torch's fp32 softmax -> topk -> sum -> div on the same logits against float64)
    B' = MULT * max(2^-23, the error of torch's fp32 autograd through that chain in units of sum_j |g_j| w_j)

MULT = 4: the chain rounds two exponentials (numerator, denominator: at most one unit of 2^-23 each), two divisions and the
sums of Z and s (half a unit each at the sizes here) -- four units of the fp32 format, with nothing taken from a kernel's
output.  2^-126: results under the smallest normal fp32 may be flushed.  The measured errors (reference, emu, hip) are
recorded through conftest.record (group "moe_router") and written up in profiles/moe_router_tests.md."""
import pytest
import torch

from conftest import record
from kernel_checks import BF16, F16, F32, SENT, Guarded, GuardedMatrix, check, ulp
from test_gemm_elements import place, ptr, stream_of, sync
from transformers_amd import ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]
E_DTYPE, E_SHAPE, E_ALIGN, E_NULL = -1, -2, -3, -4
GEOM = [(2, 1), (2, 2), (4, 2), (8, 2), (8, 8), (60, 4), (64, 8), (65, 8), (128, 8), (255, 16), (256, 16)]
TOKENS = (1, 5, 67)
MULT = 4.0
U23 = 2.0 ** -23
TINY = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------- float64 chains
def chain_fwd(l64, k, norm):
    """-> (w64 [T, k], idx [T, k]): include/tamd.h tamd_moe_router_fwd in float64; ties go to the lower id"""
    idx = torch.sort(l64, dim=-1, descending=True, stable=True).indices[:, :k].contiguous()
    p = torch.softmax(l64, dim=-1)
    w = p.gather(1, idx)
    if norm:
        w = w / w.sum(-1, keepdim=True)
    return w, idx


def chain_bwd(l64, idx, g64, norm):
    """-> dlogits [T, E]: float64 autograd through softmax -> gather(idx) -> renormalise"""
    l = l64.clone().requires_grad_(True)
    w = torch.softmax(l, dim=-1).gather(1, idx)
    if norm:
        w = w / w.sum(-1, keepdim=True)
    (w * g64).sum().backward()
    return l.grad


def torch_fp32(l64, idx, norm, g64=None):
    """The reference's chain as its routers run it (fp32 softmax -> topk -> sum -> div) and its autograd, on the CPU, with the
    selection given (topk rounds nothing; on the tie-free family its own choice is compared separately).
    -> (w [T, k], dlogits [T, E] or None) as float64"""
    l = l64.float().requires_grad_(g64 is not None)
    top = torch.softmax(l, dim=-1, dtype=torch.float).gather(1, idx)
    if norm:
        top = top / top.sum(-1, keepdim=True)
    if g64 is None:
        return top.detach().double(), None
    (top * g64.float()).sum().backward()
    return top.detach().double(), l.grad.double()


# ---------------------------------------------------------------------------------------------------- inputs
_INPUTS = {}


def logits_of(family, T, E, dtype):
    """float64 [T, E] holding values exact in `dtype`; computed once per session and shared (never modified)"""
    key = (family, T, E, dtype)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(7919 * T + 31 * E + (1 if dtype == F16 else 0) + 1000 * len(family))
        if family == "tiefree":  # a permutation of (i - E/2) / 16 per row: exact in bf16 and fp16, neighbours 1/16 apart
            base = (torch.arange(E, dtype=torch.float64) - E // 2) / 16.0
            t = torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)])
        else:
            scale = {"n2": 2.0, "n8": 8.0}[family]
            t = (torch.randn(T, E, generator=g, dtype=torch.float64) * scale).to(dtype).double()
        assert torch.equal(t.to(dtype).double(), t)
        _INPUTS[key] = t
    return _INPUTS[key]


def grads_of(T, k, wdt):
    g = torch.Generator().manual_seed(104729 * T + k)
    return torch.randn(T, k, generator=g, dtype=torch.float64).to(wdt).double()


# ---------------------------------------------------------------------------------------------------- calls
NULL = object()  # "pass a NULL pointer" (None means "not given" below)


def _p(default, override):
    return ptr(default) if override is None else (None if override is NULL else override)


def fwd_call(env, lg, k, norm, wdt, *, W=None, I=None, tokens=None, experts_=None, lde=None, code=None, wcode=None,
             l_ptr=None, w_ptr=None, i_ptr=None):
    """lg: a device view [T, E] with row stride lde.  -> (status, W, I): outputs inside sentinel-filled buffers"""
    T, E = lg.shape
    W = W or Guarded((T, k), wdt, env.device, 64)
    I = I or Guarded((T, k), torch.int64, env.device, 64)
    lib = ops.backend().lib
    st = lib.tamd_moe_router_fwd(_p(lg, l_ptr), _p(W.t, w_ptr), _p(I.t, i_ptr), T if tokens is None else tokens,
                                 E if experts_ is None else experts_, k, lg.stride(0) if lde is None else lde, int(norm),
                                 ops._code(W.t) if wcode is None else wcode, ops._code(lg) if code is None else code, stream_of(lg))
    sync(env.device)
    return st, W, I


def bwd_call(env, lg, idx, dw, norm, *, D=None, tokens=None, experts_=None, k=None, lde=None, code=None, wcode=None,
             l_ptr=None, i_ptr=None, g_ptr=None, d_ptr=None):
    T, E = lg.shape
    ld = lg.stride(0)
    D = D or GuardedMatrix(T, ld, ld, lg.dtype, env.device)
    lib = ops.backend().lib
    st = lib.tamd_moe_router_bwd(_p(lg, l_ptr), _p(idx, i_ptr), _p(dw, g_ptr), _p(D.t, d_ptr),
                                 T if tokens is None else tokens, E if experts_ is None else experts_,
                                 idx.shape[1] if k is None else k, ld if lde is None else lde, int(norm),
                                 ops._code(dw) if wcode is None else wcode, ops._code(lg) if code is None else code, stream_of(lg))
    sync(env.device)
    return st, D


def indices_ok(I, k, E):
    i = I.t.cpu()
    return bool(((i >= 0) & (i < E)).all()) and all(len(set(r)) == k for r in i.tolist())


# ---------------------------------------------------------------------------------------------------- the input conditions
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_tie_free_family_is_tie_free(dtype):
    """On the tie-free family torch.topk of the fp32 probabilities, of the float64 probabilities and of the logits agree, in
    order: a property of the inputs alone, asserted before any kernel runs (and again inside the kernel tests)."""
    for E, k in GEOM:
        l64 = logits_of("tiefree", 67, E, dtype)
        _assert_tie_free(l64, k)


def _assert_tie_free(l64, k):
    a = torch.topk(torch.softmax(l64.float(), dim=-1, dtype=torch.float), k, dim=-1).indices
    b = torch.topk(torch.softmax(l64, dim=-1), k, dim=-1).indices
    c = torch.topk(l64, k, dim=-1).indices
    d = torch.sort(l64, dim=-1, descending=True, stable=True).indices[:, :k]
    assert torch.equal(a, b) and torch.equal(b, c) and torch.equal(c, d)
    p32 = torch.softmax(l64.float(), dim=-1, dtype=torch.float).sort(dim=-1).values
    assert bool((p32[:, 1:] != p32[:, :-1]).all())  # all fp32 probabilities distinct


# ---------------------------------------------------------------------------------------------------- every geometry
def _check_forward(name, W, w64, wdt, B):
    got = W.t.cpu().double()
    tol = B * w64 + TINY + (0.5 * ulp(w64, wdt) if wdt != F32 else 0.0)
    bad = ~((got - w64).abs() <= tol)  # (NaN fails)
    worst = ((got - w64).abs() / w64.clamp_min(TINY)).max().item()
    if wdt == F32:
        record("moe_router", name + " fwd rel err / 2^-24", worst / 2.0 ** -24, B / 2.0 ** -24)
    print(f"{name}: forward worst relative error {worst / 2.0 ** -24:.2f} x 2^-24, gate {B / 2.0 ** -24:.2f} x 2^-24")
    assert not bool(bad.any()), (name, "first bad", torch.nonzero(bad)[0].tolist(), got[bad][0].item(), w64[bad][0].item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,k", GEOM)
def test_router_per_element(env, E, k, dtype):
    dev, lde = env.device, E + 3
    tag = f"E{E}k{k}"
    for family in ("tiefree", "n2", "n8"):
        for T in TOKENS:
            l64 = logits_of(family, T, E, dtype)
            lg = place(l64, dtype, dev, lde)
            for norm in (True, False):
                w64, idx64 = chain_fwd(l64, k, norm)
                ref32, _ = torch_fp32(l64, idx64, norm)
                if family == "tiefree":
                    _assert_tie_free(l64, k)  # the reference's own choice equals idx64 on every row
                ref_err = ((ref32 - w64).abs() / w64.clamp_min(TINY)).max().item()
                B = MULT * max(U23, ref_err)
                record("moe_router", f"{tag} {family} T{T} norm{int(norm)} reference fwd rel err / 2^-24", ref_err / 2.0 ** -24)
                for wdt in (F32, dtype):
                    name = f"{env.name} {tag} {family} T{T} norm{int(norm)} w{'32' if wdt == F32 else 'T'}"
                    st, W, I = fwd_call(env, lg, k, norm, wdt)
                    assert st == 0 and W.intact() and I.intact(), name
                    assert torch.equal(I.t.cpu(), idx64), (name, "indices")  # every row, none left out
                    _check_forward(name, W, w64, wdt, B)
                    # backward from the same logits and the expected indices
                    g64 = grads_of(T, k, wdt)
                    d64 = chain_bwd(l64, idx64, g64, norm)
                    _, d32 = torch_fp32(l64, idx64, norm, g64)
                    scale = (g64.abs() * w64).sum(-1, keepdim=True)
                    ref_b = ((d32 - d64).abs() / scale.clamp_min(TINY)).max().item()
                    Bp = MULT * max(U23, ref_b)
                    record("moe_router", f"{tag} {family} T{T} norm{int(norm)} reference bwd err / (2^-24 scale)", ref_b / 2.0 ** -24)
                    st, D = bwd_call(env, lg, idx64.to(dev), g64.to(wdt).to(dev), norm)
                    assert st == 0 and D.intact(), name
                    full = D.full.cpu()
                    assert bool((full[:, E:] == 0).all()), (name, "columns behind E are zeros")
                    got = full[:, :E]
                    if norm:
                        unsel = torch.ones(T, E, dtype=torch.bool).scatter_(1, idx64, False)
                        z = got[unsel]
                        assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), (name, "unselected entries are +0")
                    check(name + " dlogits", got, d64, (Bp * scale).expand(T, E), dtype, group="moe_router")


# ---------------------------------------------------------------------------------------------------- ties
def _tie_rows(E):
    """rows whose equal logits sit on either side of the layout's boundaries (id = r * 64 + lane)"""
    rows = []

    def row(pairs, base=-1.0):
        r = torch.full((E,), base, dtype=torch.float64)
        for i, v in pairs:
            r[i] = v
        rows.append(r)

    row([])                                    # all equal: 0 .. k-1
    if E >= 128:
        row([(67, 2.0), (5, 2.0)])             # lane 3 of register 1 against lane 5 of register 0: 5 first
        row([(67, 2.0), (3, 2.0)])             # one lane, two registers: 3 first
        row([(95, 2.0), (33, 2.0)])            # lane 31 of register 1 against lane 33 of register 0 (across the 32-lane halves)
        row([(64, 2.0), (63, 2.0), (127, 2.0)])
    if E >= 256:
        row([(200, 2.0), (9, 2.0)])            # lane 8 of register 3 against lane 9 of register 0
        row([(255, 2.0), (192, 2.0), (128, 2.0), (1, 2.0)])
    return torch.stack(rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,k", [(8, 2), (128, 8), (256, 16)])
def test_ties_go_to_the_lower_id(env, E, k, dtype):
    l64 = _tie_rows(E)
    # a tie at the k / k+1 boundary: k - 1 clear winners, then two equal candidates for the last slot
    b = torch.full((E,), -2.0, dtype=torch.float64)
    b[E - k + 1:] = torch.arange(1, k, dtype=torch.float64)
    b[E - k - 1], b[1] = 0.5, 0.5
    l64 = torch.cat([l64, b[None]])
    want = torch.sort(l64, dim=-1, descending=True, stable=True).indices[:, :k]
    assert want[0].tolist() == list(range(k)) and want[-1, -1].item() == 1
    if E >= 128:
        assert want[1, :2].tolist() == [5, 67] and want[2, :2].tolist() == [3, 67] and want[3, :2].tolist() == [33, 95]
    st, W, I = fwd_call(env, place(l64, dtype, env.device, E + 3), k, True, F32)
    assert st == 0 and W.intact() and I.intact()
    assert torch.equal(I.t.cpu(), want)


# ---------------------------------------------------------------------------------------------------- range
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,k", [(8, 2), (65, 8), (256, 16)])
def test_range(env, E, k, dtype):
    dev = env.device
    big = 60000.0 if dtype == F16 else 80.0
    rows = []
    for b in {80.0, big}:
        r = torch.full((E,), -b, dtype=torch.float64)
        r[E // 3] = b
        rows.append(r)
    r = torch.full((E,), float("-inf"), dtype=torch.float64)  # -inf in all but k - 1 entries
    r[torch.arange(k - 1) * (E // k) + 1] = torch.arange(k - 1, dtype=torch.float64) * 0.25
    rows.append(r)
    l64 = torch.stack(rows)
    for norm in (True, False):
        w64, idx64 = chain_fwd(l64, k, norm)
        st, W, I = fwd_call(env, place(l64, dtype, dev, E + 3), k, norm, F32)
        assert st == 0 and W.intact() and I.intact()
        assert torch.equal(I.t.cpu(), idx64)
        got = W.t.cpu().double()
        for i in range(len(rows) - 1):  # the largest is 1, the rest underflow
            assert got[i, 0].item() == 1.0 and bool((got[i, 1:] == 0).all())
        assert bool(((got - w64).abs() <= MULT * U23 * w64 + TINY).all())
    # a NaN somewhere, and nothing but -inf: the values are unspecified, the indices are k distinct ids in [0, E)
    bad = torch.stack([logits_of("n2", 1, E, dtype)[0].clone(), torch.full((E,), float("-inf"), dtype=torch.float64)])
    bad[0, E // 2] = float("nan")
    for norm in (True, False):
        st, W, I = fwd_call(env, place(bad, dtype, dev, E + 3), k, norm, dtype)
        assert st == 0 and W.intact() and I.intact() and indices_ok(I, k, E)
        st, D = bwd_call(env, place(bad, dtype, dev, E + 3), I.t.clone(), torch.ones(2, k, dtype=dtype, device=dev), norm)
        assert st == 0 and D.intact()


def test_backward_skips_ids_outside_the_experts(env):
    """An id outside [0, E) in top_k_index indexes nothing and contributes nothing: the result is the one of the remaining
    slots alone."""
    E, k, T, dtype, dev = 8, 3, 5, BF16, env.device
    l64 = logits_of("n2", T, E, dtype)
    lg = place(l64, dtype, dev, E + 3)
    _, idx64 = chain_fwd(l64, k, True)
    g64 = grads_of(T, k, F32)
    bad = idx64.clone()
    bad[:, 1] = torch.tensor([E, -1, 1 << 40, -(1 << 40), E + 100])
    keep = torch.tensor([0, 2])
    for norm in (True, False):
        d64 = chain_bwd(l64, idx64[:, keep], g64[:, keep], norm)
        st, D = bwd_call(env, lg, bad.to(dev), g64.float().to(dev), norm)
        assert st == 0 and D.intact()
        w, _ = chain_fwd(l64, k, False)
        sel = w[:, keep] / (w[:, keep].sum(-1, keepdim=True) if norm else 1.0)
        scale = (g64[:, keep].abs() * sel).sum(-1, keepdim=True)
        check(f"{env.name} sentinel ids norm{int(norm)}", D.full.cpu()[:, :E], d64, (MULT * U23 * scale).expand(T, E), dtype,
              group="moe_router")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(env):
    dev, E, k, T = env.device, 8, 2, 5
    l64 = logits_of("n2", T, E, BF16)
    lg = place(l64, BF16, dev, E + 3)
    big = place(torch.zeros(2, 264, dtype=torch.float64), BF16, dev, 272)
    W, I = Guarded((T, 17), F32, dev, 64), Guarded((T, 17), torch.int64, dev, 64)
    cases = [
        (E_DTYPE, dict(code=2)), (E_DTYPE, dict(wcode=1)),                       # fp32 logits; fp16 weights for bf16 logits
        (E_SHAPE, dict(k=9)), (E_SHAPE, dict(k=17, lg=big)), (E_SHAPE, dict(lg=big, experts_=257)),  # k > E, k > 16, E > 256
        (E_SHAPE, dict(tokens=0)), (E_SHAPE, dict(lde=E - 1)), (E_SHAPE, dict(k=0)),
        (E_ALIGN, dict(l_ptr=ptr(lg) + 1)), (E_ALIGN, dict(i_ptr=ptr(I.t) + 4)), (E_ALIGN, dict(w_ptr=ptr(W.t) + 2)),
        (E_NULL, dict(l_ptr=NULL)), (E_NULL, dict(w_ptr=NULL)), (E_NULL, dict(i_ptr=NULL)),
    ]
    for want, kw in cases:
        kw = dict(kw)
        st, _, _ = fwd_call(env, kw.pop("lg", lg), kw.pop("k", k), True, F32, W=W, I=I, **kw)
        assert st == want, (want, kw, st)
        assert W.untouched() and I.untouched(), kw
    idx = torch.zeros(T, k, dtype=torch.int64, device=dev)
    dw = torch.ones(T, k, dtype=F32, device=dev)
    D = GuardedMatrix(T, E + 3, E + 3, BF16, dev)
    bcases = [
        (E_DTYPE, dict(code=2)), (E_DTYPE, dict(wcode=1)), (E_SHAPE, dict(k=9)), (E_SHAPE, dict(k=17)),
        (E_SHAPE, dict(experts_=257)), (E_SHAPE, dict(tokens=0)), (E_SHAPE, dict(lde=E - 1)),
        (E_ALIGN, dict(l_ptr=ptr(lg) + 1)), (E_ALIGN, dict(d_ptr=ptr(D.t) + 1)), (E_ALIGN, dict(i_ptr=ptr(idx) + 4)),
        (E_ALIGN, dict(g_ptr=ptr(dw) + 2)),
        (E_NULL, dict(l_ptr=NULL)), (E_NULL, dict(i_ptr=NULL)), (E_NULL, dict(g_ptr=NULL)), (E_NULL, dict(d_ptr=NULL)),
    ]
    for want, kw in bcases:
        st, _ = bwd_call(env, lg, idx, dw, True, D=D, **kw)
        assert st == want, (want, kw, st)
        assert D.untouched(), kw


# ---------------------------------------------------------------------------------------------------- the op
def test_op_opcheck(env):
    from torch.library import opcheck

    dev = env.device
    lg = logits_of("n2", 5, 8, BF16).to(BF16).to(dev).requires_grad_(True)
    for norm, fp32 in ((True, True), (False, False)):
        opcheck(torch.ops.tamd.moe_router, (lg, 2, norm, fp32),
                test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    w, idx = torch.ops.tamd.moe_router(lg.detach(), 2, True, True)
    opcheck(torch.ops.tamd.moe_router_bwd, (torch.ones_like(w), lg.detach(), idx, True), test_utils=("test_schema", "test_faketensor"))
    # a [:, :E] view of a wider product (the padded-E path): the op and its backward keep the row stride
    wide = torch.zeros(5, 16, dtype=BF16, device=dev)
    wide[:, :12] = logits_of("n2", 5, 12, BF16).to(BF16).to(dev)
    view = wide[:, :12]
    opcheck(torch.ops.tamd.moe_router, (view.detach().requires_grad_(True), 4, True, False),
            test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    w, idx = torch.ops.tamd.moe_router(view, 4, True, False)
    opcheck(torch.ops.tamd.moe_router_bwd, (torch.ones_like(w), view, idx, True), test_utils=("test_schema", "test_faketensor"))
    assert torch.ops.tamd.moe_router_bwd(torch.ones_like(w), view, idx, True).stride() == (16, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fp32", [True, False], ids=["w32", "wT"])
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
def test_op_gradient_against_float64_autograd(env, norm, fp32, dtype):
    """ops.moe_router on a [:, :E] view of a wider product (the padded-gate path: row stride 16 for E = 12) and on a dense
    matrix; the gradient arrives through the op's autograd formula."""
    dev, T, E, k = env.device, 67, 12, 4
    l64 = logits_of("n2", T, E, dtype)
    w64, idx64 = chain_fwd(l64, k, norm)
    wdt = F32 if fp32 else dtype
    g64 = grads_of(T, k, wdt)
    d64 = chain_bwd(l64, idx64, g64, norm)
    scale = (g64.abs() * w64).sum(-1, keepdim=True)
    for strided in (True, False):
        wide = torch.zeros(T, 16 if strided else E, dtype=dtype, device=dev)
        wide[:, :E] = l64.to(dtype).to(dev)
        wide.requires_grad_(True)
        w, idx = ops.moe_router(wide[:, :E], k, norm, fp32)
        assert w.dtype == wdt and idx.dtype == torch.int64 and w.shape == idx.shape == (T, k) and not idx.requires_grad
        assert torch.equal(idx.cpu(), idx64)
        tol = MULT * U23 * w64 + TINY + (0.5 * ulp(w64, wdt) if wdt != F32 else 0.0)
        assert bool(((w.detach().cpu().double() - w64).abs() <= tol).all())
        (w * g64.to(wdt).to(dev)).sum().backward()
        sync(dev)
        got = wide.grad.cpu()
        assert bool((got[:, E:] == 0).all())
        check(f"{env.name} op norm{int(norm)} strided{int(strided)}", got[:, :E], d64, (MULT * U23 * scale).expand(T, E), dtype,
              group="moe_router")
