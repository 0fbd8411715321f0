"""gemv_fp8w_mfma_kernel (csrc/gemv_fp8.inc: 2 .. 64 rows of tamd_gemm_fp8w) where tests/test_fp8_linear.py does not look: the
workspace that 17 .. 64 rows no longer write, the instantiations its shapes do not reach (two row blocks per workgroup, a second
load round with a ragged last block) and one exact case per arithmetic mode.  Bounds: test_fp8_linear.py's docstring (streaming
form, M <= 16) and kernel_checks.check (GEMM form); which case reaches which instantiation: profiles/fp8_linear_isa.md."""
import pytest
import torch

from kernel_checks import GuardedMatrix, check, rnd, ulp
from test_fp8_linear import BIAS, DTYPES, GROUP, NONE, RESIDUAL, U2, Operands, within
from transformers_amd import ops

FILL = 0xA5


def run(env, p, epi, ld):
    """The call with a queried, FILL-ed workspace -> (y, workspace)."""
    need = ops.backend().lib.tamd_gemm_fp8w_workspace_bytes(p.M, p.N, p.K, 0)
    ws = torch.full((max(need, 16),), FILL, dtype=torch.uint8, device=env.device)
    y = GuardedMatrix(p.M, p.N, ld, p.dtype, env.device)
    assert p.call(ops.backend(), y, epi, ws if need else None, need) == 0 and y.intact()
    return y, ws


def gemm_bound(name, p, y, epi):  # (test_fp8_linear.gemm_form's reference and chain)
    pre = p.x64 @ p.wd64.t() + p.bias64
    ref, chain = (pre, None) if epi == BIAS else (pre + p.r64, rnd(rnd(pre, p.dtype) + p.r64, p.dtype))
    check(name, y.t, ref, U2 * p.K * (p.x64.abs() @ p.wd64.abs().t()), p.dtype, chain=chain, group=GROUP)


def stream_bound(name, p, y):  # (test_fp8_linear.test_streaming_form's bound under TAMD_EPI_BIAS)
    ref, s = p.x64 @ p.w64.t() + p.bias64, p.K * U2 * (p.x64.abs() @ p.w64.abs().t())
    within(name, y.t, ref, s + 0.5 * ulp(ref.abs() + s, p.dtype))


@pytest.mark.parametrize("epi", [BIAS, RESIDUAL], ids=["bias", "residual"])
@pytest.mark.parametrize("M", [17, 33, 64, 65])
@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_stays_sentinel(env, dtype, M, epi):
    """17 .. 64 rows (MT = 2, 3, 4) build Wd in registers: every workspace byte is as it was.  65 rows: the values only."""
    p = Operands(M, 136, 144, dtype, env.device)
    y, ws = run(env, p, epi, 144)
    assert M > 64 or bool((ws == FILL).all())
    gemm_bound(f"fp8w mfma {M}x136x144/{epi}", p, y, epi)


# two row blocks per workgroup from 16369 weight rows on; 16392 = 512 * 32 + 8: the last workgroup's second block lies past N.
# K = 512 U + 16: wave 0 runs a second round whose only block holds 16 values (U = 4 at M <= 16, 2 at 33 .. 48 rows).
@pytest.mark.parametrize("shape", [(M, 16392, K) for M in (5, 16) for K in (16, 144)] + [(16, 24, 2064)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_streaming_mode_instantiations(env, dtype, shape):
    p = Operands(*shape, dtype, env.device)
    y, _ = run(env, p, BIAS, shape[1] + 3)
    stream_bound("fp8w mfma stream " + "x".join(map(str, shape)), p, y)


@pytest.mark.parametrize("shape", [(40, 24, 1040)] + [(M, 16392, 16) for M in (17, 33, 64)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rounded_mode_instantiations(env, dtype, shape):
    p = Operands(*shape, dtype, env.device)
    y, ws = run(env, p, BIAS, shape[1] + 8)
    assert bool((ws == FILL).all())
    gemm_bound("fp8w mfma gemm " + "x".join(map(str, shape)), p, y, BIAS)


@pytest.mark.parametrize("M", [16, 40])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact(env, dtype, M):
    """Integers in X and W8 and a distinct power of two per scale block (2^-14 .. 2^-6 in scale row 0, 2^-5 .. 2^3 in row 1): every
    product and every partial sum is a multiple of 2^-14 below 2^10, exact in fp32 in any order, and scaling by a power of two is
    exact in T: both modes return the float64 product rounded once.  A wrong k permutation or scale block has no bound to hide in."""
    N, K = 136, 1152
    p, g = Operands(M, N, K, dtype, env.device), torch.Generator().manual_seed(M)
    x, w = torch.randint(-2, 3, (M, K), generator=g).double(), torch.randint(-4, 5, (N, K), generator=g).double()
    s = 2.0 ** (torch.arange(18.0).view(2, 9) - 14)
    p.x[:, :K], p.w8[:, :K], p.s[:, :9] = x.to(dtype), w.float().to(torch.float8_e4m3fn).view(torch.uint8), s.float()
    y, _ = run(env, p, NONE, N + 8)
    want = rnd(x @ (w * s.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K].double()).t(), dtype)
    assert torch.equal(y.t.cpu().double(), want)
