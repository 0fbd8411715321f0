"""Linear layers over FP8 block-scaled weights (csrc/gemv_fp8.inc behind tamd_gemm_fp8w / torch.ops.tamd.linear_fp8w /
models/fp8.py), under the CPU execution model and on the MI355X; include/tamd.h's semantics restated in float64 (Operands).
Streaming form (M <= 16), per element:  |got - ref| <= e1 = s + ulp_T(|ref| + s) / 2,  s = K 2^-24 sum_k |x w|  (K fp32 operations
in any order; the rounding taken at the largest value the fp32 result can have); with a residual, the chain's second rounding on
top:  t = e1 + 2^-24 (|ref + R| + e1),  bound = t + ulp_T(|ref + R| + t) / 2.  GEMM form: kernel_checks.check with the s of
tests/test_gemm_elements.py's random operands.  Nothing is fitted; outputs sit in guarded buffers."""
import copy

import pytest
import torch
from torch import nn

import transformers_amd
from conftest import rel_err
from kernel_checks import BF16, F16, GuardedMatrix, check, rnd, ulp
from test_attn_elements import _stream, _sync
from test_attn_mla import STEPS, _reference, _stepwise
from transformers.integrations.finegrained_fp8 import FP8Linear
from transformers_amd import _cabi, ops
from transformers_amd.models.fp8 import TamdFP8Linear

CODE = {BF16: _cabi.TAMD_BF16, F16: _cabi.TAMD_F16}
NONE, BIAS, RESIDUAL = _cabi.EPI_NONE, _cabi.EPI_BIAS, _cabi.EPI_RESIDUAL
E_DTYPE, E_SHAPE, E_ARG = -1, -2, -6
U2, GROUP = 2.0 ** -24, "fp8_linear"
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="fp16")]


def expand(s, n, k):
    return s.repeat_interleave(128, 0)[:n].repeat_interleave(128, 1)[:, :k]


def scales(n, k, g):  # distinct per block: a random mantissa times a power of two in [2^-6, 2^2]
    shape = (-(-n // 128), -(-k // 128))
    return ((1 + torch.rand(shape, generator=g)) * 2.0 ** torch.randint(-6, 2, shape, generator=g)).float()


class Operands:
    """x [M, K], e4m3 w8 [N, K], s, bias [N], r [M, N] with padded rows on `dev`, and the float64 quantities of the reference."""

    def __init__(self, M, N, K, dtype, dev, seed=0):
        g = torch.Generator().manual_seed(1000 * M + N + K + seed)
        self.M, self.N, self.K, self.dtype = M, N, K, dtype
        x, w8 = torch.randn(M, K, generator=g).to(dtype), torch.randn(N, K, generator=g).to(torch.float8_e4m3fn)
        s, bias, r = scales(N, K, g), torch.randn(N, generator=g).to(dtype), torch.randn(M, N, generator=g).to(dtype)
        self.x, self.w8 = torch.zeros(M, K + 8, dtype=dtype), torch.zeros(N, K + 16, dtype=torch.uint8)
        self.x[:, :K], self.w8[:, :K] = x, w8.view(torch.uint8)
        self.s = torch.zeros(s.shape[0], s.shape[1] + 1)
        self.s[:, :-1] = s
        self.x, self.w8, self.s, self.bias, self.r = (t.to(dev) for t in (self.x, self.w8, self.s, bias, r))
        self.w64 = w8.float().double() * expand(s, N, K).double()                       # the weight, never rounded
        self.wd64 = (w8.float() * expand(s, N, K)).to(dtype).double()                   # rT(r32(f32(W8) * S))
        self.x64, self.bias64, self.r64 = x.double(), bias.double(), r.double()

    def call(self, be, y, epi, ws=None, ws_bytes=0, chunk=0, **over):
        a = dict(X=self.x.data_ptr(), W=self.w8.data_ptr(), S=self.s.data_ptr(), Y=y.t.data_ptr(),
                 bias=self.bias.data_ptr() if epi != NONE else None, R=self.r.data_ptr() if epi == RESIDUAL else None,
                 M=self.M, N=self.N, K=self.K, ldx=self.K + 8, ldw=self.K + 16, lds=self.s.shape[1], ldy=y.full.shape[1], ldr=self.N,
                 dtype=CODE[self.dtype])
        a.update(over)
        rc = be.lib.tamd_gemm_fp8w(a["X"], a["W"], a["S"], a["Y"], a["bias"], a["R"], a["M"], a["N"], a["K"], a["ldx"], a["ldw"],
                                   a["lds"], a["ldy"], a["ldr"], epi, a["dtype"], None if ws is None else ws.data_ptr(), ws_bytes,
                                   chunk, _stream(be, self.x))
        _sync(self.x)
        return rc


def test_decode_table(env):
    """Every non-NaN code (the two NaN codes replaced by 0) through dequant_fp8w: exact in bf16 and fp16, at scale 1 and 2^-3."""
    be, dev = ops.backend(), env.device
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes & 0x7f == 0x7f] = 0
    want = codes.view(torch.float8_e4m3fn).float().view(2, 128)
    w8 = codes.view(2, 128).to(dev)
    for dtype, scale in ((BF16, 1.0), (BF16, 0.125), (F16, 1.0), (F16, 0.125)):
        s = torch.full((1, 1), scale, device=dev)
        out = GuardedMatrix(2, 128, 136, dtype, dev)
        args = (w8.data_ptr(), s.data_ptr(), out.t.data_ptr(), 2, 128, 128, 1, 136, CODE[dtype], _stream(be, w8))
        assert be.lib.tamd_dequant_fp8w(*args) == 0
        _sync(w8)
        assert out.intact() and torch.equal(out.t.cpu().float(), want * scale), (dtype, scale)


def within(name, got, ref, bound):
    ratio = ((got.cpu().double() - ref).abs() / bound).max().item()
    print(f"{name}: worst {ratio:.3f} of the bound")
    assert ratio <= 1.0, (name, ratio)  # (NaN fails)


# K: one lane, a ragged second scale block, a second step of the wave.  N: fewer rows than a workgroup owns, a ragged second scale row,
# and at 16392 four rows per wave (N >= 16384, up to four rows of X) over a ragged last wave.  M: every kernel built (1, 2, 4, 8, 16).
STREAM = ([(M, N, K) for M in (1, 3, 6, 16) for N in (8, 136) for K in (16, 144, 1152)]
          + [(M, 16392, K) for M in (1, 2, 3) for K in (16, 144)])


@pytest.mark.parametrize("shape", STREAM, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_streaming_form(env, dtype, shape):
    M, N, K = shape
    p = Operands(M, N, K, dtype, env.device)
    acc = p.x64 @ p.w64.t()
    s = K * U2 * (p.x64.abs() @ p.w64.abs().t())
    for name, epi in (("none", NONE), ("bias", BIAS), ("residual", RESIDUAL)):
        pre = acc if epi == NONE else acc + p.bias64
        e1 = s + 0.5 * ulp(pre.abs() + s, dtype)
        ref, bound = pre, e1
        if epi == RESIDUAL:
            ref = pre + p.r64
            t = e1 + U2 * (ref.abs() + e1)
            bound = t + 0.5 * ulp(ref.abs() + t, dtype)
        y = GuardedMatrix(M, N, N + 3, dtype, env.device)
        assert p.call(ops.backend(), y, epi) == 0 and y.intact()
        within(f"fp8w stream {name} {M}x{N}x{K}", y.t, ref, bound)


def gemm_form(env, dtype, M, N, K, epi, chunk=0):
    be, p = ops.backend(), Operands(M, N, K, dtype, env.device)
    need = be.lib.tamd_gemm_fp8w_workspace_bytes(M, N, K, chunk)
    assert need == min(N, 128 if chunk else N) * K * 2
    ws = torch.empty(need, dtype=torch.uint8, device=env.device)
    y = GuardedMatrix(M, N, N + 8, dtype, env.device)
    assert p.call(be, y, epi, ws, need, chunk) == 0 and y.intact()
    pre = p.x64 @ p.wd64.t() + p.bias64
    ref, chain = (pre, None) if epi == BIAS else (pre + p.r64, rnd(rnd(pre, dtype) + p.r64, dtype))  # (tamd_gemm's documented chain)
    check(f"fp8w gemm {M}x{N}x{K}/{chunk}/{epi}", y.t, ref, U2 * K * (p.x64.abs() @ p.wd64.abs().t()), dtype, chain=chain, group=GROUP)


@pytest.mark.parametrize("K", [16, 144, 1152])
@pytest.mark.parametrize("N", [8, 136])
@pytest.mark.parametrize("M", [17, 40])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_form(env, dtype, M, N, K):
    gemm_form(env, dtype, M, N, K, BIAS)


@pytest.mark.parametrize("epi", [BIAS, RESIDUAL], ids=["bias", "residual"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_form_in_two_chunks(env, dtype, epi):
    gemm_form(env, dtype, 40, 136, 144, epi, chunk=128 * 144 * 2)  # (a 128-row cap: rows 0 .. 127, then 128 .. 135 into their slice)


def test_refusals_write_nothing(env):
    be, dev = ops.backend(), env.device
    p, big = Operands(4, 8, 16, BF16, dev), Operands(17, 8, 16, BF16, dev)
    ws = torch.empty(8 * 16 * 2, dtype=torch.uint8, device=dev)

    def refused(q, want, ws=None, ws_bytes=0, **over):
        y = GuardedMatrix(q.M, q.N, q.N + 8, BF16, dev)
        assert q.call(be, y, BIAS, ws, ws_bytes, **over) == want, over
        assert y.untouched(), over

    for want, over in ((E_SHAPE, dict(K=24)), (E_SHAPE, dict(M=0)), (E_SHAPE, dict(ldw=8)), (E_ARG, dict(X=None)), (E_ARG, dict(S=None)),
                       (E_ARG, dict(bias=None)), (E_ARG, dict(W=p.w8.data_ptr() + 8)), (E_ARG, dict(X=p.x.data_ptr() + 2)),
                       (E_DTYPE, dict(dtype=_cabi.TAMD_F32))):
        refused(p, want, **over)
    refused(big, E_ARG)                                   # M > 16 without a workspace
    refused(big, E_ARG, ws, ws.numel() - 1)               # ... and with one byte too few
    refused(big, E_SHAPE, ws, ws.numel(), ldy=13)
    x, w8 = p.x[:, :16].clone().requires_grad_(), p.w8[:, :16].contiguous().view(torch.float8_e4m3fn)
    for who, args in (("x", (x, w8)), ("w8", (x.detach(), w8.clone().requires_grad_()))):
        with pytest.raises(RuntimeError, match=f"`{who}` requires grad"):
            torch.ops.tamd.linear_fp8w(*args, p.s[:, :1].contiguous(), None)


def fp8_linear(weight, bias=None, block=(128, 128)):
    """An FP8Linear holding a block-wise e4m3 quantisation of `weight` (fp32 [N, K]) -> (module, dequantised fp32 weight)."""
    n, k = weight.shape
    m = FP8Linear(k, n, block_size=block, has_bias=bias is not None)
    amax = torch.stack([torch.stack([blk.abs().max() for blk in row.split(128, 1)]) for row in weight.split(128, 0)])
    s = (amax / 448.0).clamp_min(2.0 ** -20).float()
    q = (weight / expand(s, n, k)).to(torch.float8_e4m3fn)
    m.weight, m.weight_scale_inv = nn.Parameter(q, requires_grad=False), nn.Parameter(s)
    if bias is not None:
        m.bias = nn.Parameter(bias)
    return m, q.float() * expand(s, n, k)


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_module(env, dtype, has_bias):
    g = torch.Generator().manual_seed(3)
    N, K = 136, 144
    bias = torch.randn(N, generator=g).to(dtype) if has_bias else None
    lin, wd = fp8_linear(torch.randn(N, K, generator=g), bias)
    model = transformers_amd.accelerate(nn.Sequential(lin).to(env.device))
    assert type(model[0]) is TamdFP8Linear
    transformers_amd.fallback_calls(reset=True)
    b64 = bias.double() if has_bias else 0.0
    for shape in ((1, 2, K), (2, 12, K)):
        x = torch.randn(*shape, generator=g).to(dtype)
        with torch.no_grad():
            y = model(x.to(env.device))
        assert y.shape == (*shape[:-1], N) and y.dtype == dtype
        x64 = x.double().view(-1, K)
        if x64.shape[0] <= 16:
            ref, s = x64 @ wd.double().t() + b64, K * U2 * (x64.abs() @ wd.double().abs().t())
            within("fp8w module M=2", y.view(-1, N), ref, s + 0.5 * ulp(ref.abs() + s, dtype))
        else:
            wd64 = wd.to(dtype).double()
            check("fp8w module M=24", y.view(-1, N), x64 @ wd64.t() + b64, U2 * K * (x64.abs() @ wd64.abs().t()), dtype, group=GROUP)
    assert not transformers_amd.fallback_calls() and type(transformers_amd.revert(model)[0]) is FP8Linear


def test_module_leaves_other_formats_to_the_reference(env, monkeypatch):
    monkeypatch.setattr(FP8Linear, "forward", lambda self, x: "reference")
    small, _ = fp8_linear(torch.randn(8, 64), block=(64, 64))
    wide, _ = fp8_linear(torch.randn(8, 64))
    wide.weight = nn.Parameter(torch.randn(8, 64).bfloat16(), requires_grad=False)  # (a dequantised checkpoint)
    model = transformers_amd.accelerate(nn.Sequential(small, wide).to(env.device))
    transformers_amd.fallback_calls(reset=True)
    x = torch.randn(2, 64).bfloat16().to(env.device)
    with torch.no_grad():
        assert model[0](x) == "reference" and model[1](x) == "reference"
    assert transformers_amd.fallback_calls() == {"TamdFP8Linear:block_size": 1, "TamdFP8Linear:not_e4m3": 1}
    transformers_amd.revert(model)


def quantise_linears(model):
    out = {}  # attention and dense-MLP nn.Linear -> FP8Linear; {id of the new module: its dequantised fp32 weight}
    for layer in model.model.layers:
        for parent in (layer.self_attn, layer.mlp):
            for name, child in list(parent.named_children()):
                if type(child) is nn.Linear:
                    lin, wd = fp8_linear(child.weight.detach().float())
                    setattr(parent, name, lin)
                    out[id(lin)] = wd
    return out


def test_model_padded_prefill_and_cached_steps(env):
    r = _reference()  # (the two-layer DeepseekV3ForCausalLM of tests/test_attn_mla.py, its ids and its left-padded mask)
    fast, ids, am = copy.deepcopy(r["ref"]), r["ids"], r["am"]
    wd = quantise_linears(fast)
    refs = []
    for dtype in (torch.float32, torch.bfloat16):  # the eager model on the dequantised weights, in fp32 and in bf16
        ref = copy.deepcopy(fast)
        for (_, a), (_, b) in zip(ref.named_modules(), fast.named_modules()):
            if id(b) in wd:
                a.__class__, a.weight = nn.Linear, nn.Parameter(wd[id(b)])
                del a.weight_scale_inv
        refs.append(ref.to(dtype))
    l32, lref = (_stepwise(m, "dynamic", ids, am, STEPS, "cpu") for m in refs)
    fast = transformers_amd.accelerate(fast.to(env.device))
    assert sum(type(m) is TamdFP8Linear for m in fast.modules()) == len(wd)
    transformers_amd.fallback_calls(reset=True)
    got = _stepwise(fast, "dynamic", ids, am, STEPS, env.device)
    assert not any("FP8" in k for k in transformers_amd.fallback_calls()), transformers_amd.fallback_calls()
    valid, pos = am.bool(), 0
    for i, n in enumerate(STEPS):
        keep = valid[:, pos:pos + n]
        e_fast, e_ref = (rel_err(t[:, pos:pos + n][keep], l32[:, pos:pos + n][keep]) for t in (got, lref))
        print(f"{env.name} step {i} ({n} tokens at {pos}): ours {float(e_fast):.5f} reference bf16 {float(e_ref):.5f}")
        assert e_fast <= 1.1 * e_ref + 1e-3, (i, n, pos, e_fast, e_ref)
        pos += n
