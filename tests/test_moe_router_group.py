"""The sigmoid, group-limited router kernels (csrc/moe_router_group.inc: tamd_moe_router_group_fwd / _bwd, the ops
torch.ops.tamd.moe_router_grouped and moe_gate_logits), element by element, on the SAME shapes under the CPU execution model
(`emu`) and on the MI355X (`hip`).

Layout under test: one wave per token, four tokens per 256-thread workgroup, expert id = r * 64 + lane (1, 2 or 4 registers per
lane); a group is G consecutive experts and lies across lanes and registers.  T in {1, 5, 67}: one wave; a ragged second
workgroup; many workgroups and a ragged last one.  GEOM covers one / two / four registers, no groups, G = 2 with every eligible
expert taken, G = 32 with three groups, 64 groups of 4, k = 16.  lde = E + 3 everywhere (gap columns of the logits hold NaN).

Expected values are float64 evaluations of the chain of include/tamd.h from the stored fp32 logits and bias -- never another
kernel's output.  On the tie-free family (asserted on the inputs, in float64, before any kernel runs: the group-score gap at the
topk_group boundary and every gap among the k + 1 largest eligible c are at least 8 * 2^-23 relative) the indices are compared
as ordered lists.  Gates, u = 2^-23:

    forward    |w - w64| <= MULT(k) u w64 + 2^-126
    MULT(k) = 5.5 + (k - 1) / 2:  s = 1 / (1 + exp(-l)) rounds the exponential (1 u, and x / (1 + x) <= 1 of it reaches s), the
              addition (0.5) and the division (0.5): 2 u on every s.  d carries the 2 u of its positive terms, (k - 1) / 2 for its
              k - 1 additions and 0.5 for + 1e-20; then the division and the product with scale, 0.5 each:
              2 + (2 + (k - 1) / 2 + 0.5) + 0.5 + 0.5.
    backward   |dl_e - dl64_e| <= MULTB(k) u f (|g_j| + Q) s_j + 2^-126,   f = scale / d (scale without norm), Q = sum_i |g_i| s_i / d
              (0 without norm).  The unit drops the factor (1 - s_j) on purpose: 1 - s is computed from the ROUNDED s (as the
              reference's autograd does from its saved output), an absolute error of 2.5 u s that no bound relative to 1 - s covers.
    MULTB(k) = 14.5 + 1.5 (k - 1):  f: D + 0.5 with D = 2.5 + (k - 1) / 2 (d, above); s_j: 2; the two products: 1; g_j - q in
              units of |g_j| + Q: the w_i (2 + D + 0.5), their products (0.5) and sum ((k - 1) / 2), the subtraction (0.5);
              1 - s_j in units of s_j: 2.5.
Against torch (the reference's own lines in fp32 on the same logits): index SETS per row, weights by id, the same forward gate.
The gate op's backward: the bound of include/tamd.h (one rounding of dlogits to the operands' type) + K 2^-24 sum|terms| + half an
ulp of the result.  Measured errors are recorded through conftest.record (group "moe_router_group")."""
import pytest
import torch

from conftest import record
from kernel_checks import BF16, F16, F32, Guarded, GuardedMatrix, ulp
from test_gemm_elements import place, ptr, stream_of, sync
from transformers_amd import ops

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4
GEOM = [(8, 1, 1, 2), (6, 3, 2, 4), (16, 4, 2, 4), (64, 8, 4, 6), (96, 3, 2, 8), (128, 1, 1, 8), (160, 1, 1, 8),
        (256, 8, 4, 8), (256, 64, 16, 16), (256, 1, 1, 16)]
TOKENS = (1, 5, 67)
SCALES = (1.0, 2.5)
U23 = 2.0 ** -23
TINY = 2.0 ** -126
NEG = float("-inf")


def MULT(k):
    return 5.5 + (k - 1) / 2.0


def MULTB(k):
    return 14.5 + 1.5 * (k - 1)


# ---------------------------------------------------------------------------------------------------- float64 chains
def scores64(l64, b64):
    s = torch.sigmoid(l64)
    c = s + b64
    return s, torch.where(torch.isnan(c), torch.full_like(c, NEG), c)


def eligible64(c, ng, tg):
    """-> (eligible [T, E] bool, group scores [T, ng] or None); equal group scores go to the lower group"""
    T, E = c.shape
    if ng == 1:
        return torch.ones(T, E, dtype=torch.bool), None
    gs = c.view(T, ng, E // ng).topk(2, dim=-1).values.sum(-1)
    gs = torch.where(torch.isnan(gs), torch.full_like(gs, NEG), gs)
    top = torch.sort(gs, dim=-1, descending=True, stable=True).indices[:, :tg]
    mask = torch.zeros(T, ng, dtype=torch.bool).scatter_(1, top, True)
    return mask[:, :, None].expand(T, ng, E // ng).reshape(T, E), gs


def chain_fwd(l64, b64, k, ng, tg, norm, scale):
    """-> (w64 [T, k], idx [T, k]): include/tamd.h tamd_moe_router_group_fwd in float64; ties go to the lower id"""
    s, c = scores64(l64, b64)
    elig, _ = eligible64(c, ng, tg)
    # ineligible experts sort behind every eligible one, whatever its c (-inf, a NaN): a key of two parts
    order = torch.sort(torch.where(elig, c, torch.full_like(c, NEG)), dim=-1, descending=True, stable=True).indices
    rank_elig = torch.sort((~elig.gather(1, order)).to(torch.int8), dim=-1, stable=True).indices
    idx = order.gather(1, rank_elig)[:, :k].contiguous()
    return weights64(s, idx, norm, scale), idx


def weights64(s, idx, norm, scale):
    w = s.gather(1, idx)
    if norm:
        w = w / (w.sum(-1, keepdim=True) + 1e-20)
    return w * scale


def chain_bwd(l64, idx, g64, norm, scale):
    """float64 autograd through sigmoid -> gather(idx) -> renormalise -> scale"""
    l = l64.clone().requires_grad_(True)
    (weights64(torch.sigmoid(l), idx, norm, scale) * g64).sum().backward()
    return l.grad


def torch_reference(l32, b32, k, ng, tg, norm, scale):
    """DeepseekV3TopkRouter.forward behind its gate product (modeling_deepseek_v3.py:148-169), line by line, in fp32"""
    E = l32.shape[1]
    scores = l32.sigmoid()
    scores_for_choice = scores + b32
    group_scores = scores_for_choice.view(-1, ng, E // ng).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=tg, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(-1, ng, E // ng).reshape(-1, E)
    scores_for_choice = scores_for_choice.masked_fill(~score_mask.bool(), float("-inf"))
    topk_indices = torch.topk(scores_for_choice, k=k, dim=-1, sorted=False)[1]
    topk_weights = scores.gather(1, topk_indices)
    if norm:
        topk_weights = topk_weights / (topk_weights.sum(dim=-1, keepdim=True) + 1e-20)
    return topk_weights * scale, topk_indices


# ---------------------------------------------------------------------------------------------------- inputs
_INPUTS = {}


def tie_free_ok(l64, b64, k, ng, tg):
    s, c = scores64(l64, b64)
    elig, gs = eligible64(c, ng, tg)
    if gs is not None and tg < ng:
        g = torch.sort(gs, dim=-1, descending=True).values
        if not bool(((g[:, tg - 1] - g[:, tg]) >= 8 * U23 * g[:, tg - 1].abs()).all()):
            return False
    top = torch.sort(torch.where(elig, c, torch.full_like(c, NEG)), dim=-1, descending=True).values[:, :k + 1]
    top = top[:, :min(k + 1, int(elig[0].sum()))]
    return bool(((top[:, :-1] - top[:, 1:]) >= 8 * U23 * top[:, :-1].abs()).all())


def inputs_of(T, geom, with_bias):
    """(l64 [T, E], b64 [E]) holding fp32 values; the first seed of 0 .. 31 whose rows are tie-free -- a property of the inputs
    alone; computed once per session and shared (never modified)"""
    key = (T, geom, with_bias)
    if key not in _INPUTS:
        E, ng, tg, k = geom
        for seed in range(32):
            g = torch.Generator().manual_seed(1009 * seed + 7919 * T + 31 * E + ng + (500 if with_bias else 0))
            base = (torch.arange(E, dtype=torch.float64) - E // 2) * (8.0 / E)  # logits over [-4, 4)
            l64 = torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)])
            l64 = (l64 + torch.randn(T, E, generator=g, dtype=torch.float64) * (1.0 / E)).float().double()
            b64 = (torch.rand(E, generator=g) * 0.2 - 0.1).double() if with_bias else torch.zeros(E, dtype=torch.float64)
            if tie_free_ok(l64, b64, k, ng, tg):
                break
        else:
            raise AssertionError(f"no tie-free inputs for T {T} {geom}")
        _INPUTS[key] = (l64, b64)
    return _INPUTS[key]


def grads_of(T, k):
    g = torch.Generator().manual_seed(104729 * T + k)
    return torch.randn(T, k, generator=g).double()


# ---------------------------------------------------------------------------------------------------- calls
NULL = object()


def _p(default, override):
    return ptr(default) if override is None else (None if override is NULL else override)


def fwd_call(env, lg, bias, geom, norm, scale, *, W=None, I=None, tokens=None, lde=None, l_ptr=None, b_ptr=None, w_ptr=None, i_ptr=None):
    """lg: a device view [T, E] (fp32, row stride lde); bias: a device tensor or None.  -> (status, W, I)"""
    T = lg.shape[0]
    E, ng, tg, k = geom
    W = W or Guarded((T, k), F32, env.device, 64)
    I = I or Guarded((T, k), torch.int64, env.device, 64)
    st = ops.backend().lib.tamd_moe_router_group_fwd(_p(lg, l_ptr), _p(bias, b_ptr), _p(W.t, w_ptr), _p(I.t, i_ptr),
                                                     T if tokens is None else tokens, E, k, ng, tg,
                                                     lg.stride(0) if lde is None else lde, int(norm), scale, stream_of(lg))
    sync(env.device)
    return st, W, I


def bwd_call(env, lg, idx, dw, geom, norm, scale, *, D=None, tokens=None, lde=None, l_ptr=None, i_ptr=None, g_ptr=None, d_ptr=None):
    T = lg.shape[0]
    E, ng, tg, k = geom
    ld = lg.stride(0)
    D = D or GuardedMatrix(T, ld, ld, F32, env.device)
    st = ops.backend().lib.tamd_moe_router_group_bwd(_p(lg, l_ptr), _p(idx, i_ptr), _p(dw, g_ptr), _p(D.t, d_ptr),
                                                     T if tokens is None else tokens, E, k, ng, tg, ld if lde is None else lde,
                                                     int(norm), scale, stream_of(lg))
    sync(env.device)
    return st, D


def indices_ok(I, k, E):
    i = I.t.cpu()
    return bool(((i >= 0) & (i < E)).all()) and all(len(set(r)) == k for r in i.tolist())


# ---------------------------------------------------------------------------------------------------- the input condition
@pytest.mark.parametrize("geom", GEOM, ids=str)
def test_the_tie_free_family_is_tie_free(geom):
    """A property of the inputs alone, asserted before any kernel runs (and again inside the kernel tests); on such rows the
    reference's own fp32 choice is the float64 chain's."""
    E, ng, tg, k = geom
    for with_bias in (False, True):
        l64, b64 = inputs_of(67, geom, with_bias)
        assert tie_free_ok(l64, b64, k, ng, tg)
        _, idx64 = chain_fwd(l64, b64, k, ng, tg, True, 1.0)
        _, idx32 = torch_reference(l64.float(), b64.float(), k, ng, tg, True, 1.0)
        assert torch.equal(idx32.sort(-1).values, idx64.sort(-1).values)


# ---------------------------------------------------------------------------------------------------- every geometry
def bwd_unit(l64, idx, g64, norm, scale):
    """[T, E] float64: f (|g_j| + Q) s_j at the selected entries (the module docstring), 0 elsewhere"""
    s = torch.sigmoid(l64).gather(1, idx)
    if norm:
        d = s.sum(-1, keepdim=True) + 1e-20
        f, Q = scale / d, (g64.abs() * s / d).sum(-1, keepdim=True)
    else:
        f, Q = torch.full_like(s[:, :1], scale), torch.zeros_like(s[:, :1])
    return torch.zeros_like(l64).scatter_(1, idx, f * (g64.abs() + Q) * s)


@pytest.mark.parametrize("geom", GEOM, ids=str)
def test_router_group_per_element(env, geom):
    E, ng, tg, k = geom
    dev, lde = env.device, E + 3
    worst_f = worst_b = worst_t = 0.0
    for with_bias in (False, True):
        for T in TOKENS:
            l64, b64 = inputs_of(T, geom, with_bias)
            assert tie_free_ok(l64, b64, k, ng, tg)
            lg = place(l64, F32, dev, lde)
            bias = b64.float().to(dev) if with_bias else None
            g64 = grads_of(T, k)
            for norm in (True, False):
                for scale in SCALES:
                    name = f"{env.name} {geom} T{T} bias{int(with_bias)} norm{int(norm)} scale{scale}"
                    w64, idx64 = chain_fwd(l64, b64, k, ng, tg, norm, scale)
                    st, W, I = fwd_call(env, lg, bias, geom, norm, scale)
                    assert st == 0 and W.intact() and I.intact(), name
                    assert indices_ok(I, k, E), name
                    assert torch.equal(I.t.cpu(), idx64), (name, "indices, as an ordered list")  # every row, none left out
                    got = W.t.cpu().double()
                    err = ((got - w64).abs() / w64.clamp_min(TINY)).max().item() / U23
                    worst_f = max(worst_f, err)
                    assert bool(((got - w64).abs() <= MULT(k) * U23 * w64 + TINY).all()), (name, "weights", err)
                    # against torch: the reference's own lines in fp32 on the same logits
                    wt, it = torch_reference(l64.float(), b64.float(), k, ng, tg, norm, scale)
                    assert torch.equal(it.sort(-1).values, idx64.sort(-1).values), (name, "index sets against torch")
                    by_id = torch.zeros(T, E, dtype=torch.float64).scatter_(1, it, wt.double()).gather(1, idx64)
                    errt = ((got - by_id).abs() / by_id.clamp_min(TINY)).max().item() / U23
                    worst_t = max(worst_t, errt)
                    assert bool(((got - by_id).abs() <= MULT(k) * U23 * by_id + TINY).all()), (name, "weights against torch", errt)
                    # backward from the same logits and the expected indices
                    d64 = chain_bwd(l64, idx64, g64, norm, scale)
                    st, D = bwd_call(env, lg, idx64.to(dev), g64.float().to(dev), geom, norm, scale)
                    assert st == 0 and D.intact(), name
                    full = D.full.cpu()
                    assert bool((full[:, E:] == 0).all()), (name, "columns behind E are zeros")
                    gotd = full[:, :E].double()
                    unsel = torch.ones(T, E, dtype=torch.bool).scatter_(1, idx64, False)
                    z = gotd[unsel]
                    assert bool((z == 0).all()) and not bool(torch.signbit(z).any()), (name, "unselected entries are +0")
                    unit = bwd_unit(l64, idx64, g64.float().double(), norm, scale)
                    errb = ((gotd - d64).abs() / (U23 * unit).clamp_min(TINY))[~unsel].max().item()
                    worst_b = max(worst_b, errb)
                    assert bool(((gotd - d64).abs() <= MULTB(k) * U23 * unit + TINY).all()), (name, "dlogits", errb)
    print(f"{env.name} {geom}: forward worst {worst_f:.2f} u (gate {MULT(k)}), against torch {worst_t:.2f} u, "
          f"backward worst {worst_b:.2f} u (gate {MULTB(k)})")
    record("moe_router_group", f"{env.name} {geom} fwd rel err / 2^-23", worst_f, MULT(k))
    record("moe_router_group", f"{env.name} {geom} fwd against torch / 2^-23", worst_t, MULT(k))
    record("moe_router_group", f"{env.name} {geom} bwd err / (2^-23 unit)", worst_b, MULTB(k))


# ---------------------------------------------------------------------------------------------------- the bias
def test_the_bias_steers_the_choice_and_never_the_weight(env):
    geom = (E, ng, tg, k) = (16, 4, 2, 4)
    T, dev = 5, env.device
    l64, _ = inputs_of(T, geom, False)
    l64 = l64.clone()
    l64[:, 3] = -6.0  # s = 0.0025: the smallest of its row by far
    b64 = torch.zeros(E, dtype=torch.float64)
    b64[3] = 4.0      # ... and the largest c
    lg = place(l64, F32, dev, E + 3)
    for norm in (True, False):
        _, idx0 = chain_fwd(l64, torch.zeros(E, dtype=torch.float64), k, ng, tg, norm, 2.5)
        assert not bool((idx0 == 3).any())
        w64, idx64 = chain_fwd(l64, b64, k, ng, tg, norm, 2.5)
        assert bool((idx64[:, 0] == 3).all())
        st, W, I = fwd_call(env, lg, b64.float().to(dev), geom, norm, 2.5)
        assert st == 0 and W.intact() and I.intact()
        assert torch.equal(I.t.cpu(), idx64)
        got = W.t.cpu().double()
        assert bool(((got - w64).abs() <= MULT(k) * U23 * w64 + TINY).all())
        if not norm:  # the weight of expert 3 is 2.5 * sigmoid(-6): nothing of the 4.0
            assert bool((got[:, 0] < 0.01).all())
        st, W0, I0 = fwd_call(env, lg, None, geom, norm, 2.5)  # NULL bias: zeros
        assert st == 0 and torch.equal(I0.t.cpu(), idx0)


# ---------------------------------------------------------------------------------------------------- ties
def test_ties_go_to_the_lower_id_and_the_lower_group(env):
    dev = env.device
    # equal c: ids across lanes and registers (id = r * 64 + lane), no groups
    E, k = 256, 4
    rows = []
    for pairs in ([], [(67, 2.0), (5, 2.0)], [(67, 2.0), (3, 2.0)], [(95, 2.0), (33, 2.0)], [(255, 2.0), (192, 2.0), (128, 2.0), (1, 2.0)]):
        r = torch.full((E,), -1.0, dtype=torch.float64)
        for i, v in pairs:
            r[i] = v
        rows.append(r)
    l64 = torch.stack(rows)
    want = torch.sort(l64, dim=-1, descending=True, stable=True).indices[:, :k]
    assert want[0].tolist() == [0, 1, 2, 3] and want[1, :2].tolist() == [5, 67] and want[4].tolist() == [1, 128, 192, 255]
    st, W, I = fwd_call(env, place(l64, F32, dev, E + 3), None, (E, 1, 1, k), True, 1.0)
    assert st == 0 and W.intact() and I.intact()
    assert torch.equal(I.t.cpu(), want)
    # equal group scores: four groups of 4 with the same two largest values -> groups 0 and 1; then with group 2 ahead -> 2 and 0
    E, ng, tg, k = 16, 4, 2, 4
    a = torch.tensor([1.0, 0.5, -1.0, -2.0], dtype=torch.float64)
    row0 = torch.cat([a, a.flip(0), a, a.flip(0)])
    row1 = row0.clone()
    row1[8] = 1.25
    l64 = torch.stack([row0, row1])
    st, W, I = fwd_call(env, place(l64, F32, dev, E + 3), None, (E, ng, tg, k), True, 1.0)
    assert st == 0 and W.intact() and I.intact()
    assert I.t.cpu().tolist() == [[0, 7, 1, 6], [8, 0, 1, 9]]
    w64, idx64 = chain_fwd(l64, torch.zeros(E, dtype=torch.float64), k, ng, tg, True, 1.0)
    assert idx64.tolist() == [[0, 7, 1, 6], [8, 0, 1, 9]]  # (the float64 chain breaks ties the same way)


# ---------------------------------------------------------------------------------------------------- range
@pytest.mark.parametrize("geom", [(8, 1, 1, 2), (64, 8, 4, 6), (256, 8, 4, 8)], ids=str)
def test_range(env, geom):
    E, ng, tg, k = geom
    dev = env.device
    rows = []
    for big in (30.0, 200.0):  # s saturates to exactly 1 (both) and exactly 0 (-200)
        r = torch.full((E,), -big, dtype=torch.float64)
        r[:k] = big  # (inside the first group: it is chosen, and its k large entries with it)
        rows.append(r)
    rows.append(torch.full((E,), -200.0, dtype=torch.float64))  # every s is 0
    l64 = torch.stack(rows)
    zero = torch.zeros(E, dtype=torch.float64)
    for norm in (True, False):
        w64, idx64 = chain_fwd(l64, zero, k, ng, tg, norm, 2.5)
        st, W, I = fwd_call(env, place(l64, F32, dev, E + 3), None, geom, norm, 2.5)
        assert st == 0 and W.intact() and I.intact() and indices_ok(I, k, E)
        got = W.t.cpu().double()
        assert bool(torch.isfinite(got).all())
        assert torch.equal(I.t.cpu()[:2].sort(-1).values, idx64[:2].sort(-1).values)
        exact = 2.5 / k if norm else 2.5  # k weights of s = 1
        assert bool(((got[:2] - exact).abs() <= MULT(k) * U23 * exact).all())
        assert bool((got[2] == 0).all()), "every s is 0: the weights are exactly 0, with and without norm"
        g = torch.ones(3, k, dtype=F32, device=dev)
        st, D = bwd_call(env, place(l64, F32, dev, E + 3), I.t.clone(), g, geom, norm, 2.5)
        assert st == 0 and D.intact()
        full = D.full.cpu()
        assert bool(torch.isfinite(full).all()) and bool((full[2] == 0).all())
    # a NaN logit: the values are unspecified, the indices are k distinct ids in [0, E)
    bad = inputs_of(5, geom, False)[0].clone()
    bad[0, E // 2] = float("nan")
    bad[1] = float("nan")
    for norm in (True, False):
        st, W, I = fwd_call(env, place(bad, F32, dev, E + 3), None, geom, norm, 1.0)
        assert st == 0 and W.intact() and I.intact() and indices_ok(I, k, E)
        st, D = bwd_call(env, place(bad, F32, dev, E + 3), I.t.clone(), torch.ones(5, k, dtype=F32, device=dev), geom, norm, 1.0)
        assert st == 0 and D.intact()


def test_backward_skips_ids_outside_the_experts(env):
    """An id outside [0, E) in top_k_index indexes nothing and contributes nothing: the result is the one of the remaining
    slots alone."""
    geom = (E, ng, tg, k) = (8, 1, 1, 3)
    T, dev = 5, env.device
    l64, b64 = inputs_of(T, (8, 1, 1, 2), False)
    lg = place(l64, F32, dev, E + 3)
    _, idx64 = chain_fwd(l64, b64, k, ng, tg, True, 1.0)
    g64 = grads_of(T, k).float().double()
    bad = idx64.clone()
    bad[:, 1] = torch.tensor([E, -1, 1 << 40, -(1 << 40), E + 100])
    keep = torch.tensor([0, 2])
    for norm in (True, False):
        d64 = chain_bwd(l64, idx64[:, keep], g64[:, keep], norm, 2.5)
        st, D = bwd_call(env, lg, bad.to(dev), g64.float().to(dev), geom, norm, 2.5)
        assert st == 0 and D.intact()
        unit = bwd_unit(l64, idx64[:, keep], g64[:, keep], norm, 2.5)
        assert bool(((D.full.cpu()[:, :E].double() - d64).abs() <= MULTB(k) * U23 * unit + TINY).all())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(env):
    dev, T = env.device, 5
    l64 = torch.zeros(T, 264, dtype=torch.float64)
    lg = place(l64, F32, dev, 267)
    W, I = Guarded((T, 17), F32, dev, 64), Guarded((T, 17), torch.int64, dev, 64)
    bias = torch.zeros(264, dtype=F32, device=dev)
    idx = torch.zeros(T, 17, dtype=torch.int64, device=dev)
    dw = torch.ones(T, 17, dtype=F32, device=dev)
    D = GuardedMatrix(T, 267, 267, F32, dev)
    shapes = [(264, 1, 1, 2),   # E > 256
              (16, 3, 1, 2),    # E % n_group
              (256, 128, 4, 2),  # n_group > 64
              (16, 4, 0, 2), (16, 4, 5, 2),  # topk_group outside [1, n_group]
              (16, 16, 4, 2),   # G = 1 with groups
              (16, 4, 2, 9), (256, 1, 1, 17), (16, 1, 1, 0)]  # k > topk_group * G, k > 16, k = 0
    for geom in shapes:
        st, _, _ = fwd_call(env, lg[:, :geom[0]], bias, geom, True, 1.0, W=W, I=I)
        assert st == E_SHAPE and W.untouched() and I.untouched(), geom
        st, _ = bwd_call(env, lg[:, :geom[0]], idx, dw, geom, True, 1.0, D=D)
        assert st == E_SHAPE and D.untouched(), geom
    ok = (16, 4, 2, 4)
    v = lg[:, :16]
    for want, kw in [(E_SHAPE, dict(tokens=0)), (E_SHAPE, dict(lde=15)), (E_SHAPE, dict(tokens=1 << 31)),
                     (E_ALIGN, dict(l_ptr=ptr(v) + 2)), (E_ALIGN, dict(b_ptr=ptr(bias) + 1)), (E_ALIGN, dict(w_ptr=ptr(W.t) + 2)),
                     (E_ALIGN, dict(i_ptr=ptr(I.t) + 4)),
                     (E_NULL, dict(l_ptr=NULL)), (E_NULL, dict(w_ptr=NULL)), (E_NULL, dict(i_ptr=NULL))]:
        st, _, _ = fwd_call(env, v, bias, ok, True, 1.0, W=W, I=I, **kw)
        assert st == want and W.untouched() and I.untouched(), (want, kw, st)
    for want, kw in [(E_SHAPE, dict(tokens=0)), (E_SHAPE, dict(lde=15)),
                     (E_ALIGN, dict(l_ptr=ptr(v) + 2)), (E_ALIGN, dict(d_ptr=ptr(D.t) + 2)), (E_ALIGN, dict(i_ptr=ptr(idx) + 4)),
                     (E_ALIGN, dict(g_ptr=ptr(dw) + 2)),
                     (E_NULL, dict(l_ptr=NULL)), (E_NULL, dict(i_ptr=NULL)), (E_NULL, dict(g_ptr=NULL)), (E_NULL, dict(d_ptr=NULL))]:
        st, _ = bwd_call(env, v, idx, dw, ok, True, 1.0, D=D, **kw)
        assert st == want and D.untouched(), (want, kw, st)


# ---------------------------------------------------------------------------------------------------- the ops
def test_op_opcheck(env):
    from torch.library import opcheck

    dev = env.device
    geom = (16, 4, 2, 4)
    l64, b64 = inputs_of(5, geom, True)
    lg = l64.float().to(dev).requires_grad_(True)
    bias = b64.float().to(dev)
    for b, norm, scale in ((bias, True, 2.5), (None, False, 1.0)):
        opcheck(torch.ops.tamd.moe_router_grouped, (lg, b, 4, 4, 2, norm, scale),
                test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    w, idx = torch.ops.tamd.moe_router_grouped(lg.detach(), bias, 4, 4, 2, True, 2.5)
    opcheck(torch.ops.tamd.moe_router_grouped_bwd, (torch.ones_like(w), lg.detach(), idx, 4, 2, True, 2.5),
            test_utils=("test_schema", "test_faketensor"))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 64, generator=g).to(BF16).to(dev).requires_grad_(True)
    wt = torch.randn(16, 64, generator=g).to(BF16).to(dev).requires_grad_(True)
    opcheck(torch.ops.tamd.moe_gate_logits, (x, wt), test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_op_gradient_against_float64_autograd(env):
    """ops.moe_router_grouped: the gradient arrives through the op's autograd formula; the indices carry none"""
    geom = (E, ng, tg, k) = (64, 8, 4, 6)
    T, dev = 67, env.device
    l64, b64 = inputs_of(T, geom, True)
    g64 = grads_of(T, k).float().double()
    for norm in (True, False):
        w64, idx64 = chain_fwd(l64, b64, k, ng, tg, norm, 2.5)
        lg = l64.float().to(dev).requires_grad_(True)
        w, idx = ops.moe_router_grouped(lg, b64.float().to(dev), k, ng, tg, norm, 2.5)
        assert w.dtype == F32 and idx.dtype == torch.int64 and w.shape == idx.shape == (T, k) and not idx.requires_grad
        assert torch.equal(idx.cpu(), idx64)
        (w * g64.float().to(dev)).sum().backward()
        sync(dev)
        d64 = chain_bwd(l64, idx64, g64, norm, 2.5)
        unit = bwd_unit(l64, idx64, g64, norm, 2.5)
        assert bool(((lg.grad.cpu().double() - d64).abs() <= MULTB(k) * U23 * unit + TINY).all())


@pytest.mark.parametrize("dtype", [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")])
def test_gate_op_backward(env, dtype):
    """ops.moe_gate_logits' backward: the fp32 dlogits rounded ONCE to the operands' type, then dX = dl . W and dW = dl^T . X on
    the GEMM kernels.  Per element against float64:
        |dX - dX64| <= r sum_e |dl_e W_e| + K 2^-24 sum |terms| + half an ulp of the result,  r = 2^-9 (bf16) / 2^-12 (fp16), K = E
    and likewise dW over the tokens (K = T)."""
    dev, T, E, H = env.device, 67, 72, 192
    g = torch.Generator().manual_seed(11)
    x64 = torch.randn(T, H, generator=g, dtype=torch.float64).to(dtype).double()
    w64 = (torch.randn(E, H, generator=g, dtype=torch.float64) * 0.1).to(dtype).double()
    dl64 = torch.randn(T, E, generator=g).double()  # fp32 values: what the router's backward (or a caller) hands back
    x = x64.to(dtype).to(dev).requires_grad_(True)
    w = w64.to(dtype).to(dev).requires_grad_(True)
    y = ops.moe_gate_logits(x, w)
    y.backward(dl64.float().to(dev))
    sync(dev)
    r = 2.0 ** -9 if dtype == BF16 else 2.0 ** -12
    for name, got, want, terms, K in (("dX", x.grad, dl64 @ w64, dl64.abs() @ w64.abs(), E),
                                      ("dW", w.grad, dl64.t() @ x64, dl64.abs().t() @ x64.abs(), T)):
        assert got.dtype == dtype and got.shape == want.shape
        tol = r * terms + K * 2.0 ** -24 * terms + 0.5 * ulp(want, dtype)
        err = (got.cpu().double() - want).abs()
        ratio = (err / tol).max().item()
        record("moe_router_group", f"{env.name} gate op {name} err / bound [{'bf16' if dtype == BF16 else 'fp16'}]", ratio, 1.0)
        print(f"{env.name} gate op {name}: worst err / bound {ratio:.3f}")
        assert bool((err <= tol).all()), (name, ratio)
