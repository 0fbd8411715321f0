"""gemm_fp8w_kernel (csrc/gemm_fp8w.inc: tamd_gemm_fp8w from 65 to 1024 rows of X), reached through the product's rule: the workspace
it no longer writes, the edges of its 128-row W tile, 64 / 128-row X tile and 128-wide K step, one exact case, and the module.
Bounds: kernel_checks.check in the GEMM form (test_fp8_linear_mfma.gemm_bound).  64 rows of X per workgroup (BM), 128 above 512
rows from 4096 weight rows on."""
import pytest
import torch
from torch import nn

import transformers_amd
from kernel_checks import check, rnd
from test_fp8_linear import BIAS, DTYPES, GROUP, NONE, RESIDUAL, U2, Operands, fp8_linear
from test_fp8_linear_mfma import FILL, gemm_bound, run
from transformers_amd.models.fp8 import TamdFP8Linear


@pytest.mark.parametrize("epi", [BIAS, RESIDUAL], ids=["bias", "residual"])
@pytest.mark.parametrize("M", [65, 129])
@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_stays_sentinel(env, dtype, M, epi):
    """Above 64 rows Wd is built in registers too: every byte of the (still demanded) workspace is as it was."""
    p = Operands(M, 136, 144, dtype, env.device)
    y, ws = run(env, p, epi, 144)
    assert bool((ws == FILL).all())
    gemm_bound(f"fp8w tile {M}x136x144/{epi}", p, y, epi)


# M: one row into a second 64-row tile, two full ones, one row into a third, a fifth.  N: fewer rows than one wave owns, a second
# workgroup with 8 live rows in the second scale row, a third.  K: one lane group live, a ragged second scale block, nine steps
# (both LDS buffers reused several times).  The last two reach BM = 128 (more than 512 rows, 4104 weight rows: 33 W tiles, the
# last with 8 live rows, in five rounds of eight with seven padding workgroups per M tile): one row into a fifth 128-row tile at one
# lane group of K, and four K steps, the last ragged.
EDGES = [(65, 8, 16), (65, 136, 144), (65, 264, 1152), (128, 136, 16), (128, 8, 1152), (129, 8, 144), (129, 136, 1152),
         (129, 264, 16), (257, 136, 144), (257, 264, 1152), (513, 4104, 16), (520, 4104, 400)]


@pytest.mark.parametrize("shape", EDGES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_edges(env, dtype, shape):
    p = Operands(*shape, dtype, env.device)
    y, ws = run(env, p, BIAS, shape[1] + 8)
    assert bool((ws == FILL).all())
    gemm_bound("fp8w tile " + "x".join(map(str, shape)), p, y, BIAS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact(env, dtype):
    """test_fp8_linear_mfma.test_exact's construction over three scale rows (2^-14 .. 2^-6, 2^-5 .. 2^3, then 2^-14 .. 2^-6 reversed,
    so that row 2 differs from row 0 block by block): integers in X and W8, every product and partial sum of an output a multiple
    of its scale row's smallest scale and below 2^19 times it -- exact in fp32 in any order, and the scaling exact in T: the
    float64 product rounded once.  A wrong k permutation, scale block, row tile or buffer phase has no bound to hide in."""
    M, N, K = 130, 264, 1152
    p, g = Operands(M, N, K, dtype, env.device), torch.Generator().manual_seed(M)
    x, w = torch.randint(-2, 3, (M, K), generator=g).double(), torch.randint(-4, 5, (N, K), generator=g).double()
    e = torch.arange(18.0).view(2, 9) - 14
    s = 2.0 ** torch.cat([e, e[:1].flip(1)])
    p.x[:, :K], p.w8[:, :K], p.s[:, :9] = x.to(dtype), w.float().to(torch.float8_e4m3fn).view(torch.uint8), s.float()
    y, _ = run(env, p, NONE, N + 8)
    want = rnd(x @ (w * s.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K].double()).t(), dtype)
    assert torch.equal(y.t.cpu().double(), want)


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module(env, dtype, has_bias):
    g = torch.Generator().manual_seed(5)
    N, K = 136, 144
    bias = torch.randn(N, generator=g).to(dtype) if has_bias else None
    lin, wd = fp8_linear(torch.randn(N, K, generator=g), bias)
    model = transformers_amd.accelerate(nn.Sequential(lin).to(env.device))
    assert type(model[0]) is TamdFP8Linear
    transformers_amd.fallback_calls(reset=True)
    x = torch.randn(2, 40, K, generator=g).to(dtype)  # 80 rows
    with torch.no_grad():
        y = model(x.to(env.device))
    assert y.shape == (2, 40, N) and y.dtype == dtype and not transformers_amd.fallback_calls()
    x64, wd64 = x.double().view(-1, K), wd.to(dtype).double()
    ref = x64 @ wd64.t() + (bias.double() if has_bias else 0.0)
    check("fp8w tile module M=80", y.view(-1, N), ref, U2 * K * (x64.abs() @ wd64.abs().t()), dtype, group=GROUP)
    transformers_amd.revert(model)
