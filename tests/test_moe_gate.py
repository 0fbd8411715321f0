"""The gate product of the sigmoid routers (csrc/moe_gate.inc: tamd_moe_gate_f32), element by element, on the SAME shapes under
the CPU execution model (`emu`) and on the MI355X (`hip`).

logits[t, e] = sum_h f32(x[t, h]) * f32(w[e, h]) with the fp32 accumulators stored unrounded.  Two kernels behind the entry:
up to 16 tokens one 16-token block against 8 expert rows per workgroup (16 waves over H), above that 32 tokens x 64 experts per
workgroup (8 waves over H).  T in {1, 5, 16} and {17, 67, 130} are the two kernels, the cut between them and ragged token tiles;
E in {8, 64, 72, 160, 256} has one block, whole and ragged 64-expert slices; H in {64, 192, 1024} gives 2, 6 and 32 steps of 32
for 16 / 8 waves: waves without a step, one step each, several.  ldx = H + 8 and lde = E + 3 everywhere; the gap columns of
the operands hold NaN, the output lies in a sentinel-filled buffer that is checked after every call.

Exact: operands are small integers times a power of two (tests/test_gemm_elements.py's construction), every partial sum is an
integer below 2^24 units -- exact in fp32 in ANY order -- so the logits equal the float64 product bit for bit.
Random operands: |logit - float64| <= H * 2^-24 * sum_h |x_h w_h| per element, the worst-case bound of an fp32 summation of H
exact terms in any order (each of at most H - 1 additions rounds by at most 2^-24 of a partial sum of the |terms|); nothing
measured goes into it.  The largest observed ratio is recorded (conftest.record, group "moe_gate")."""
import pytest
import torch

from conftest import record
from kernel_checks import BF16, F16, F32, SENT, GuardedMatrix
from test_gemm_elements import Problem, place, ptr, stream_of, sync
from transformers_amd import ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]
E_DTYPE, E_SHAPE, E_ALIGN, E_NULL = -1, -2, -3, -4
TOKENS = (1, 5, 16, 17, 67, 130)
EXPERTS = (8, 64, 72, 160, 256)
HIDDEN = (64, 192, 1024)
NULL = object()


def _p(default, override):
    return ptr(default) if override is None else (None if override is NULL else override)


def gate_call(env, x, w, *, L=None, tokens=None, experts=None, hidden=None, ldx=None, lde=None, code=None, x_ptr=None,
              w_ptr=None, l_ptr=None):
    """x: a device view [T, H] (row stride ldx), w: [E, H] contiguous.  -> (status, L): logits inside a sentinel-filled buffer"""
    T, H = x.shape
    E = w.shape[0]
    L = L or GuardedMatrix(T, E, E + 3, F32, env.device)
    st = ops.backend().lib.tamd_moe_gate_f32(_p(x, x_ptr), _p(w, w_ptr), _p(L.t, l_ptr), T if tokens is None else tokens,
                                             E if experts is None else experts, H if hidden is None else hidden,
                                             x.stride(0) if ldx is None else ldx, L.full.stride(0) if lde is None else lde,
                                             ops._code(x) if code is None else code, stream_of(x))
    sync(env.device)
    return st, L


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HIDDEN)
def test_exact_product_bit_for_bit(env, H, dtype):
    dev = env.device
    for E in EXPERTS:
        p = Problem(dtype, max(TOKENS), E, H)  # one exact problem per (E, H); fewer tokens take its first rows
        w = p.B.to(dtype).to(dev)
        for T in TOKENS:
            x = place(p.A[:T], dtype, dev, H + 8)
            st, L = gate_call(env, x, w)
            assert st == 0 and L.intact(), (T, E, H)
            got = L.t.cpu().double()
            want = p.acc[:T]
            assert torch.equal(got, want), (T, E, H, "first bad", torch.nonzero(got != want)[0].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_operands_within_the_summation_bound(env, dtype):
    dev = env.device
    worst = 0.0
    for T, E, H in ((5, 72, 192), (16, 256, 1024), (17, 8, 64), (67, 160, 1024), (130, 64, 192)):
        g = torch.Generator().manual_seed(97 * T + 13 * E + H)
        x64 = torch.randn(T, H, generator=g, dtype=torch.float64).to(dtype).double()
        w64 = (torch.randn(E, H, generator=g, dtype=torch.float64) * 0.05).to(dtype).double()
        st, L = gate_call(env, place(x64, dtype, dev, H + 8), w64.to(dtype).to(dev))
        assert st == 0 and L.intact()
        got = L.t.cpu().double()
        want = x64 @ w64.t()
        bound = H * 2.0 ** -24 * (x64.abs() @ w64.abs().t())
        ratio = ((got - want).abs() / bound).max().item()
        worst = max(worst, ratio)
        print(f"{env.name} T{T} E{E} H{H}: worst |err| / bound {ratio:.4f}")
        assert bool(((got - want).abs() <= bound).all()), (T, E, H, ratio)
    record("moe_gate", f"{env.name} random operands |err| / (H 2^-24 sum|terms|) [{'bf16' if dtype == BF16 else 'fp16'}]", worst, 1.0)


def test_refusals_leave_the_output_untouched(env):
    dev, T, E, H = env.device, 5, 16, 128
    g = torch.Generator().manual_seed(3)
    x = place(torch.randn(T, H, generator=g, dtype=torch.float64), BF16, dev, H + 8)
    w = torch.randn(264, H, generator=g).to(BF16).to(dev)
    L = GuardedMatrix(T, 264, 267, F32, dev)
    cases = [
        (E_SHAPE, dict(experts=12)), (E_SHAPE, dict(experts=264)), (E_SHAPE, dict(experts=0)), (E_SHAPE, dict(tokens=0)),
        (E_SHAPE, dict(hidden=96)), (E_SHAPE, dict(ldx=H - 8)), (E_SHAPE, dict(lde=E - 1)), (E_SHAPE, dict(tokens=1 << 31)),
        (E_DTYPE, dict(code=2)),
        (E_NULL, dict(x_ptr=NULL)), (E_NULL, dict(w_ptr=NULL)), (E_NULL, dict(l_ptr=NULL)),
        (E_ALIGN, dict(x_ptr=ptr(x) + 2)), (E_ALIGN, dict(w_ptr=ptr(w) + 8)), (E_ALIGN, dict(l_ptr=ptr(L.t) + 2)),
        (E_ALIGN, dict(ldx=H + 4)),
    ]
    for want, kw in cases:
        kw = dict(kw)
        kw.setdefault("experts", E)
        st, _ = gate_call(env, x, w, L=L, **kw)
        assert st == want, (want, kw, st)
        assert L.untouched(), kw


def test_op_matches_the_entry(env):
    """torch.ops.tamd.moe_gate_logits: a strided view and a dense matrix give the entry's bits; fp32 [T, E] comes back"""
    dev, T, E, H = env.device, 17, 72, 192
    p = Problem(BF16, max(TOKENS), E, H)
    w = p.B.to(BF16).to(dev)
    for x in (place(p.A[:T], BF16, dev, H + 8), p.A[:T].to(BF16).to(dev)):
        y = ops.moe_gate_logits(x, w)
        sync(dev)
        assert y.dtype == F32 and y.shape == (T, E)
        assert torch.equal(y.cpu().double(), p.acc[:T])
