"""Op-level parity: every C-ABI kernel against an fp32 restatement of the reference formula on the
SAME (storage-dtype-rounded) inputs.  The tolerance for floating-point ops is 1e-3 norm-relative
unless the op's output rounding dominates (then 2^-8 relative = one bf16 ulp); integer / index paths
(embedding gather, label handling) are bit-exact.  Each test runs twice: under the CPU execution model
(`emu`, not gpu) and on the MI355X (`hip`, gpu).

The shapes here grow with `env.big`, so the MI355X sees round shapes only and every gate is a norm.  The row kernels (norm
family, cross-entropy, column sums) are checked a second time in test_row_kernels.py, which runs identical small shapes on
both backends -- every norm geometry, ragged rows and widths -- and checks per element.  The GEMM family (tile kernels,
weight-streaming kernels, split-K, segmented and grouped launches, every epilogue) is checked bit for bit against exact
float64 chains, at ragged edges and with leading dimensions, in test_gemm_elements.py."""
import math

import pytest
import torch

from conftest import max_err, record, rel_err
from transformers_amd import ops

BF16_EPS = 2.0 ** -8


def ref_rmsnorm(x, w, eps):  # models/llama/modeling_llama.py:62-67
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return w * (xf * torch.rsqrt(var + eps)).to(x.dtype)


@pytest.mark.parametrize("cols", [64, 768, 4096])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_rmsnorm_fwd_bwd(env, cols, dtype):
    torch.manual_seed(0)
    rows = 4096 if env.big else 9
    x = torch.randn(rows, cols).to(dtype).to(env.device).requires_grad_(True)
    w = (torch.rand(cols) + 0.5).to(dtype).to(env.device).requires_grad_(True)
    y = ops.rmsnorm(x, w, 1e-5)
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    yr = ref_rmsnorm(xr, wr, 1e-5)
    # identical rounding points -> essentially bit-exact (fp32 summation order may flip a last bit)
    if dtype != torch.float32:
        assert (y != yr).float().mean().item() < 2e-3
    assert rel_err(y, yr) < 1.2e-05
    g = torch.randn_like(y)
    y.backward(g)
    yr.float().backward(g.float())
    tol = 1e-5 if dtype == torch.float32 else 6e-3
    assert rel_err(x.grad, xr.grad) < tol
    assert rel_err(w.grad, wr.grad) < (1e-4 if dtype == torch.float32 else 0.0072)


def test_rmsnorm_fused_residual(env):
    torch.manual_seed(1)
    rows, cols = (2048, 4096) if env.big else (7, 512)
    x = torch.randn(rows, cols).bfloat16().to(env.device)
    r = torch.randn(rows, cols).bfloat16().to(env.device)
    w = (torch.rand(cols) + 0.5).bfloat16().to(env.device)
    y, h, rstd = ops.raw_rmsnorm_fwd(x, w, 1e-6, residual=r)
    h_ref = x + r
    assert torch.equal(h, h_ref)  # bit-exact residual add
    assert rel_err(y, ref_rmsnorm(h_ref, w, 1e-6)) < 3.9e-05
    dy, dres = torch.randn_like(y), torch.randn_like(y)
    dx, dw = ops.raw_rmsnorm_bwd(dy, h, w, rstd, dres=dres)
    hr = h_ref.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    yr = wr * (hr * torch.rsqrt(hr.pow(2).mean(-1, keepdim=True) + 1e-6))
    yr.backward(dy.float())
    assert rel_err(dx, hr.grad + dres.float()) < 0.0034
    assert rel_err(dw, wr.grad) < 0.0051


@pytest.mark.parametrize("cols", [768, 1024])
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_fwd_bwd(env, cols, with_res):
    torch.manual_seed(2)
    rows = 4096 if env.big else 6
    dev = env.device
    x = torch.randn(rows, cols).bfloat16().to(dev).requires_grad_(True)
    r = torch.randn(rows, cols).bfloat16().to(dev).requires_grad_(True) if with_res else None
    w = (torch.rand(cols) + 0.5).bfloat16().to(dev).requires_grad_(True)
    b = torch.randn(cols).bfloat16().to(dev).requires_grad_(True)
    out = ops.layernorm(x, w, b, 1e-12, residual=r)
    y = out[0] if with_res else out
    xr, wr, br = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    rr = r.detach().clone().requires_grad_(True) if with_res else None
    hin = xr + rr if with_res else xr
    yr = torch.nn.functional.layer_norm(hin.float(), (cols,), wr.float(), br.float(), 1e-12)
    assert rel_err(y, yr) < 3e-3  # one bf16 output rounding
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float())
    assert rel_err(x.grad, xr.grad) < 4e-05
    if with_res:
        assert rel_err(r.grad, rr.grad) < 4e-05
    assert rel_err(w.grad, wr.grad) < 1.5e-2
    assert rel_err(b.grad, br.grad) < 1.5e-2


def ref_rope(q, cos, sin):  # modeling_llama.py:130-160, q [B,S,H,D], cos [B|1,S,D]
    def rot(x):
        x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
        return torch.cat((-x2, x1), dim=-1)

    c, s = cos.unsqueeze(2), sin.unsqueeze(2)
    return (q * c) + (rot(q) * s)


@pytest.mark.parametrize("d", [64, 128])
def test_rope_bit_exact_and_adjoint(env, d):
    torch.manual_seed(3)
    b, s, hq, hkv = (4, 512, 8, 2) if env.big else (2, 10, 3, 1)
    dev = env.device
    row = (hq + 2 * hkv) * d
    qkv = torch.randn(b, s, row).bfloat16().to(dev)
    inv = 1.0 / (500000.0 ** (torch.arange(0, d, 2).float() / d))
    fr = torch.arange(s).float()[:, None] * inv[None]
    emb = torch.cat((fr, fr), -1)
    cos, sin = emb.cos()[None].bfloat16().to(dev), emb.sin()[None].bfloat16().to(dev)
    out = qkv.clone()
    ops.raw_rope_(out.view(b * s, row), cos, sin, s, hq + hkv, d)
    ref = qkv.clone()
    n = (hq + hkv) * d
    ref[..., :n] = ref_rope(qkv[..., :n].view(b, s, hq + hkv, d), cos, sin).reshape(b, s, n)
    assert torch.equal(out, ref)  # same bf16 rounding points as the reference -> bit-exact; v untouched
    # adjoint: <R x, y> == <x, R^T y> (fp32 accumulate; roundings bound the slack)
    y = torch.randn(b, s, row).bfloat16().to(dev)
    rty = y.clone()
    ops.raw_rope_(rty.view(b * s, row), cos, sin, s, hq + hkv, d, conj=True)
    lhs = (out[..., :n].double() * y[..., :n].double()).sum()
    rhs = (qkv[..., :n].double() * rty[..., :n].double()).sum()
    # both sides carry independent bf16 roundings of ~2^-9 per element: compare on the scale of |x||y|
    scale = out[..., :n].double().norm() * y[..., :n].double().norm()
    assert abs(lhs - rhs).item() < 1e-3 * scale.item()


def test_embedding_bit_exact_and_scatter(env):
    torch.manual_seed(4)
    vocab, dim, n = (32000, 4096, 8192) if env.big else (50, 64, 40)
    dev = env.device
    table = torch.randn(vocab, dim).bfloat16().to(dev)
    ids = torch.randint(0, vocab, (2, n // 2)).to(dev)
    ids[0, :3] = 7  # repeated ids
    out = ops.raw_embedding_fwd(ids, table)
    assert torch.equal(out, table[ids])
    dout = torch.randn(2, n // 2, dim).bfloat16().to(dev)
    dt = ops.raw_embedding_bwd(ids, dout, vocab, padding_idx=None)
    ref = torch.zeros(vocab, dim, dtype=torch.float32, device=dev).index_add_(0, ids.view(-1), dout.view(-1, dim).float())
    assert rel_err(dt, ref) < 0.0029
    untouched = torch.ones(vocab, dtype=torch.bool, device=dev)
    untouched[ids.view(-1)] = False
    assert (dt[untouched] == 0).all()
    dt2 = ops.raw_embedding_bwd(ids, dout, vocab, padding_idx=7)
    assert (dt2[7] == 0).all()


def test_embedding_backward_long_runs(env):
    """Runs of one id longer than a 32-token segment (every BERT token has token_type 0; padding ids; frequent tokens)
    are split across waves and joined: every run / segment alignment, ignored padding rows, one id for all tokens."""
    dev = env.device
    dim = 768 if env.big else 64
    cases = []
    n = 16384 if env.big else 300
    cases.append(torch.zeros(n, dtype=torch.long))                                   # one run covering everything
    cases.append(torch.cat([torch.full((31,), 3), torch.full((33,), 5), torch.full((64,), 9), torch.full((1,), 11),
                            torch.full((n - 129,), 2)]))                             # boundaries at 31, 64, 128, 129
    cases.append(torch.randint(0, 4, (n,)))                                          # 4 long interleaved runs (after sort)
    cases.append(torch.cat([torch.arange(40), torch.full((n - 40,), 17)]))           # short runs then a long one
    # a run of more pieces than the join kernel has waves (16), over a row of more than one 256-column chunk, ragged
    cases.append(torch.cat([torch.full((5,), 1), torch.full((1200 if not env.big else 40000,), 6), torch.full((3,), 8)]))
    for ci, ids in enumerate(cases):
        torch.manual_seed(40 + ci)
        vocab = 64
        ids = ids.to(dev)
        if ci == len(cases) - 1:
            dim = 1096 if env.big else 328
        dout = torch.randn(ids.numel(), dim).bfloat16().to(dev)
        ref = torch.zeros(vocab, dim, dtype=torch.float32, device=dev).index_add_(0, ids, dout.float())
        for pad in (None, int(ids[-1])):
            dt = ops.raw_embedding_bwd(ids.view(1, -1), dout.view(1, -1, dim), vocab, padding_idx=pad)
            want = ref.clone()
            if pad is not None:
                want[pad] = 0
            assert rel_err(dt, want) < 0.0035, (ci, pad)
            assert (dt[want.abs().sum(-1) == 0] == 0).all(), (ci, pad)


def test_swiglu(env):
    torch.manual_seed(5)
    t, inter = (4096, 14336) if env.big else (5, 256)
    dev = env.device
    gu = torch.randn(t, 2 * inter).bfloat16().to(dev)
    act = ops.raw_swiglu_fwd(gu)
    g, u = gu[:, :inter], gu[:, inter:]
    ref = torch.nn.functional.silu(g) * u  # the reference's own bf16 op sequence (modeling_llama.py:175)
    assert (act != ref).float().mean().item() < 1e-3
    assert rel_err(act, torch.nn.functional.silu(g.float()) * u.float()) < 4e-3
    dact = torch.randn(t, inter).bfloat16().to(dev)
    dgu, act2 = ops.raw_swiglu_bwd(gu, dact, want_act=True)
    assert torch.equal(act2, act)
    gf, uf = g.float().requires_grad_(True), u.float().requires_grad_(True)
    (torch.nn.functional.silu(gf) * uf).backward(dact.float())
    assert rel_err(dgu[:, :inter], gf.grad) < 0.0048
    assert rel_err(dgu[:, inter:], uf.grad) < 0.0049


@pytest.mark.parametrize("act", ["gelu", "gelu_new", "quick_gelu", "silu"])
def test_bias_act(env, act):
    from transformers.activations import ACT2FN

    torch.manual_seed(6)
    rows, cols = (2048, 3072) if env.big else (5, 64)
    dev = env.device
    x = torch.randn(rows, cols).bfloat16().to(dev)
    b = torch.randn(cols).bfloat16().to(dev)
    code = ops.ACT_CODES[act]
    y = ops.raw_bias_act_fwd(x, b, code)
    zf = (x + b).float().requires_grad_(True)
    yr = ACT2FN[act](zf)
    assert rel_err(y, yr) < 0.0034
    dy = torch.randn_like(y)
    dx = ops.raw_bias_act_bwd(x, b, dy, code)
    yr.backward(dy.float())
    assert rel_err(dx, zf.grad) < 0.0036


def test_add_colsum_transpose(env):
    torch.manual_seed(7)
    rows, cols = (4096, 1024) if env.big else (72, 136)
    dev = env.device
    a = torch.randn(rows, cols).bfloat16().to(dev)
    b = torch.randn(rows, cols).bfloat16().to(dev)
    assert torch.equal(ops.raw_add(a, b), a + b)
    assert rel_err(ops.raw_colsum(a), a.float().sum(0)) < 0.0034
    assert torch.equal(ops.raw_transpose(a), a.t().contiguous())


def test_cross_entropy(env):
    torch.manual_seed(8)
    t, v = (4096, 128256) if env.big else (6, 1000)
    dev = env.device
    logits = (torch.randn(t, v) * 2).bfloat16().to(dev).requires_grad_(True)
    labels = torch.randint(0, v, (t,)).to(dev)
    labels[1] = -100
    lsum = ops.cross_entropy_sum(logits, labels, -100)
    lf = logits.detach().float().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lf, labels, ignore_index=-100, reduction="sum")
    assert abs(lsum.item() - ref.item()) < 1e-4 * abs(ref.item())
    (lsum / 5).backward()
    (ref / 5).backward()
    assert rel_err(logits.grad, lf.grad) < 0.0027
    assert (logits.grad[1] == 0).all()


GEMM_SHAPES_SMALL = [(256, 256, 64), (264, 248, 136), (130, 520, 72)]
GEMM_SHAPES_BIG = [(4096, 4096, 4096), (8192, 6144, 4096), (1000, 1032, 520), (4096, 14336, 4096)]


@pytest.mark.parametrize("layout", ["nt", "b_kn", "a_km|b_kn", "a_km"])
def test_gemm_layouts(env, layout):
    torch.manual_seed(9)
    dev = env.device
    shapes = list(GEMM_SHAPES_BIG if env.big else GEMM_SHAPES_SMALL)
    if layout == "a_km|b_kn":  # dW = dY^T.X reduces over tokens: a ragged token count (K % 8 != 0) must work
        shapes += [(4096, 1024, 8190), (1024, 4096, 4097)] if env.big else [(264, 248, 66), (256, 256, 33)]
    for (m, n, k) in shapes:
        if "a_km" in layout and m % 8:
            continue
        x = torch.randn(m, k).bfloat16().to(dev)
        w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
        ref = x.float() @ w.float().t()
        a = x.t().contiguous() if "a_km" in layout else x
        b = w.t().contiguous() if "b_kn" in layout else w
        c = ops.raw_gemm(a, b, a_km="a_km" in layout, b_kn="b_kn" in layout)
        assert rel_err(c, ref) < 0.0034, (layout, m, n, k)  # bf16 output rounding only (fp32 accumulation)


@pytest.mark.parametrize("sched", ["pp", "fl", "sm", None])
def test_gemm_schedules_agree(env, sched):
    """The three GEMM kernels (ping-pong with 32-deep stages; one-wave-per-SIMD with 64-deep full-line stages; the 128 x 128
    tile for small forward grids) and the default dispatch agree bit for bit on ragged M/N, stage counts around the ring
    size, every layout (the small tile: row-major operands) and epilogue."""
    torch.manual_seed(19)
    dev = env.device
    shapes = ([(4096, 4096, 4096), (1000, 1032, 320), (4100, 264, 832), (256, 256, 64)] if env.big else
              [(256, 256, 64), (264, 248, 128), (130, 520, 192), (72, 264, 320), (300, 136, 384), (64, 72, 704)])
    for (m, n, k) in shapes:
        x = torch.randn(m, k).bfloat16().to(dev)
        w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
        ref = x.float() @ w.float().t()
        c = ops.raw_gemm(x, w, sched=sched)
        assert rel_err(c, ref) < 0.0034, (sched, m, n, k)
        if sched is None and ops.backend().lib.tamd_gemm_workspace_bytes(m, n, k, 0, ops.EPI_NONE):
            continue  # the default dispatch splits K for this grid: fp32 summation order differs (test_gemm_split_k)
        assert torch.equal(c, ops.raw_gemm(x, w, sched="pp")), (sched, m, n, k)  # same fp32 k-order per output
    if sched not in ("pp", "sm"):  # k-major operands (the backward products)
        for (m, n, k) in ([(4096, 1024, 4096), (1000, 1032, 320), (264, 4104, 832)] if env.big else
                          [(256, 256, 64), (264, 248, 128), (136, 520, 192), (72, 264, 320), (304, 136, 384)]):
            if sched is None and ops.backend().lib.tamd_gemm_workspace_bytes(m, n, k, 0, ops.EPI_NONE):
                continue
            x = torch.randn(m, k).bfloat16().to(dev)
            w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
            xt, wt = x.t().contiguous(), w.t().contiguous()
            base = ops.raw_gemm(x, w, sched="pp")
            assert torch.equal(ops.raw_gemm(x, wt, b_kn=True, sched=sched), base), ("b_kn", m, n, k)
            assert torch.equal(ops.raw_gemm(xt, wt, a_km=True, b_kn=True, sched=sched), base), ("a_km|b_kn", m, n, k)
            assert torch.equal(ops.raw_gemm(xt, w, a_km=True, sched=sched), base), ("a_km", m, n, k)
    m, n, k = shapes[1]
    x = torch.randn(m, k).bfloat16().to(dev)
    w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
    bias = torch.randn(n).bfloat16().to(dev)
    res = torch.randn(m, n).bfloat16().to(dev)
    for kw in (dict(bias=bias, epilogue=ops.EPI_BIAS), dict(residual=res, epilogue=ops.EPI_RESIDUAL),
               dict(bias=bias, epilogue=ops.EPI_BIAS_ACT, act=ops.ACT_GELU_TANH)):
        assert torch.equal(ops.raw_gemm(x, w, sched=sched, **kw), ops.raw_gemm(x, w, sched="pp", **kw)), kw
    out = res.clone()
    ops.raw_gemm(x, w, epilogue=ops.EPI_ACCUM, out=out, sched=sched)
    out2 = res.clone()
    ops.raw_gemm(x, w, epilogue=ops.EPI_ACCUM, out=out2, sched="pp")
    assert torch.equal(out, out2)
    # f16 too
    c16 = ops.raw_gemm(x.half(), w.half(), sched=sched)
    assert rel_err(c16, x.half().float() @ w.half().float().t()) < 0.00042


def test_gemm_split_k(env):
    """Tile grids too small for the GPU are cut along K (fp32 partials + reduction): the weight-gradient products of
    narrow layers.  Same result as the unsplit kernel up to fp32 summation order; every layout, plain and accumulate."""
    torch.manual_seed(23)
    dev = env.device
    lib = ops.backend().lib
    shapes = [(768, 3072, 16384), (768, 768, 8192), (264, 520, 4096)] if env.big else [(256, 256, 4096), (264, 136, 4160)]
    assert lib.tamd_gemm_workspace_bytes(256, 256, 2048, 0, ops.EPI_NONE) == 0  # forward layout, < 64 stages: the 128 x 128 tile
    assert lib.tamd_gemm_workspace_bytes(256, 256, 2048, 3, ops.EPI_NONE) > 0   # the same product as a weight gradient: split
    for (m, n, k) in shapes:
        assert lib.tamd_gemm_workspace_bytes(m, n, k, 0, ops.EPI_NONE) > 0
        assert lib.tamd_gemm_workspace_bytes(m, n, k, 0, ops.EPI_BIAS) > 0       # (round 4: the reduction applies the epilogue)
        assert lib.tamd_gemm_workspace_bytes(m, n, k, 0, ops.EPI_BIAS_ACT) == 0  # ... except an activation
        x = torch.randn(m, k).bfloat16().to(dev)
        w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
        ref = x.float() @ w.float().t()
        xt, wt = x.t().contiguous(), w.t().contiguous()
        for kw, a, b in ((dict(), x, w), (dict(b_kn=True), x, wt), (dict(a_km=True, b_kn=True), xt, wt)):
            c = ops.raw_gemm(a, b, **kw)                     # default dispatch: split-K
            unsplit = ops.raw_gemm(a, b, sched="fl", **kw)   # a schedule hint turns it off
            assert rel_err(c, ref) < 0.0034, (m, n, k, kw)
            assert rel_err(c, unsplit) < 0.00015 and (c != unsplit).float().mean() < 0.2
        res = torch.randn(m, n).bfloat16().to(dev)
        out = res.clone()
        ops.raw_gemm(xt, wt, a_km=True, b_kn=True, epilogue=ops.EPI_ACCUM, out=out)
        assert rel_err(out, ref.bfloat16().float() + res.float()) < 0.0035
        # bias / residual (+ bias) epilogues through the split: the unsplit kernel's roundings (CLIP fc2, o_proj / down_proj of a
        # short prompt: modeling_clip.py:346-350, modeling_llama.py:280, :176)
        bias = torch.randn(n).bfloat16().to(dev)
        for kw2 in (dict(bias=bias, epilogue=ops.EPI_BIAS), dict(residual=res, epilogue=ops.EPI_RESIDUAL),
                    dict(bias=bias, residual=res, epilogue=ops.EPI_RESIDUAL)):
            c = ops.raw_gemm(x, w, **kw2)
            unsplit = ops.raw_gemm(x, w, sched="fl", **kw2)
            want = ref + (bias.float() if "bias" in kw2 else 0)
            if "residual" in kw2:
                want = want.bfloat16().float() + res.float()
            assert rel_err(c, want) < 0.0034, (m, n, k, list(kw2))
            assert rel_err(c, unsplit) < 0.00015 and (c != unsplit).float().mean() < 0.2, (m, n, k, list(kw2))
    assert lib.tamd_gemm_workspace_bytes(32768, 4096, 4096, 0, ops.EPI_NONE) == 0  # enough tiles: no split
    for (m, n, k) in [(768, 3072, 16384), (768, 768, 512), (256, 256, 2048), (2304, 768, 16384), (4096, 4096, 32768),
                      (30522, 768, 16384), (264, 136, 2560), (128, 4, 4096), (1000, 1000, 1000)]:
        for epi in (ops.EPI_NONE, ops.EPI_ACCUM, ops.EPI_BIAS, ops.EPI_RESIDUAL, ops.EPI_BIAS_ACT):  # the host-side mirror stays in step
            assert ops.gemm_workspace_bytes(m, n, k, epi) == lib.tamd_gemm_workspace_bytes(m, n, k, 0, epi), (m, n, k, epi)
            assert ops.gemm_workspace_bytes(m, n, k, epi, 3) == lib.tamd_gemm_workspace_bytes(m, n, k, 3, epi), (m, n, k, epi)


def test_gemm_epilogues(env):
    torch.manual_seed(10)
    dev = env.device
    m, n, k = (2048, 3072, 768) if env.big else (136, 264, 72)
    x = torch.randn(m, k).bfloat16().to(dev)
    w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
    bias = torch.randn(n).bfloat16().to(dev)
    res = torch.randn(m, n).bfloat16().to(dev)
    acc = x.float() @ w.float().t()
    c = ops.raw_gemm(x, w, bias=bias, epilogue=ops.EPI_BIAS)
    assert rel_err(c, acc + bias.float()) < 0.0034
    c = ops.raw_gemm(x, w, residual=res, epilogue=ops.EPI_RESIDUAL)
    assert rel_err(c, acc.bfloat16().float() + res.float()) < 0.0037
    c = ops.raw_gemm(x, w, bias=bias, epilogue=ops.EPI_BIAS_ACT, act=ops.ACT_GELU_ERF)
    assert rel_err(c, torch.nn.functional.gelu((acc + bias.float()).bfloat16().float())) < 0.0033
    out = res.clone()
    ops.raw_gemm(x, w, epilogue=ops.EPI_ACCUM, out=out)
    assert rel_err(out, acc.bfloat16().float() + res.float()) < 0.0037


def test_linear_autograd(env):
    torch.manual_seed(11)
    dev = env.device
    b, s, k, n = (4, 512, 1024, 2048) if env.big else (2, 20, 72, 136)
    x = torch.randn(b, s, k).bfloat16().to(dev).requires_grad_(True)
    w = (torch.randn(n, k) * 0.05).bfloat16().to(dev).requires_grad_(True)
    bias = torch.randn(n).bfloat16().to(dev).requires_grad_(True)
    y = ops.linear(x, w, bias, act=ops.ACT_GELU_ERF)
    xr, wr, br = (t.detach().float().requires_grad_(True) for t in (x, w, bias))
    yr = torch.nn.functional.gelu(torch.nn.functional.linear(xr, wr, br))
    assert rel_err(y, yr) < 0.0052
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float())
    assert rel_err(x.grad, xr.grad) < 0.0048
    assert rel_err(w.grad, wr.grad) < 0.0049
    assert rel_err(bias.grad, br.grad) < 0.0049


def ref_attention(q, k, v, scale, causal, key_valid, keep=None, drop_p=0.0):
    """eager_attention_forward (modeling_llama.py:191-213) in fp32 on [B,S,H,D] tensors; `keep` [B,H,Sq,Sk] is an
    explicit dropout keep mask (nn.functional.dropout semantics: dropped -> 0, kept -> / (1 - p))."""
    b, s, h, d = q.shape
    sk, hkv = k.shape[1], k.shape[2]
    g = h // hkv
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
    sc = qf @ kf.transpose(-1, -2) * scale
    mask = torch.ones(s, sk, dtype=torch.bool, device=q.device)
    if causal:
        mask = torch.tril(mask, diagonal=sk - s)
    mask = mask[None, None].expand(b, 1, s, sk).clone()
    if key_valid is not None:
        mask = mask & key_valid[:, None, None, :].bool()
    sc = sc.masked_fill(~mask, float("-inf"))
    pr = torch.softmax(sc, -1)
    if keep is not None:
        pr = pr * keep.to(pr.device).float() / (1.0 - drop_p)
    return (pr @ vf).permute(0, 2, 1, 3)


@pytest.mark.parametrize("d", [128, 64])
def test_attention_takes_prescaled_queries_from_the_rotary_kernel(env, d):
    """ABI 7 (include/tamd.h): tamd_rope_inplace multiplies the query heads by scale*log2(e) BEFORE its one rounding, and
    the attention kernels, told so (q_prescaled), skip their own scale-and-re-round of the resident operand.  Checked
    through the C ABI: the scaled rotary kernel's bits; forward and backward of both forms against the fp32 model (rotary
    embedding and eager attention in fp32); the pre-scaled form is the more accurate one (no second rounding of q)."""
    import ctypes
    from transformers_amd import _cabi
    be = ops.backend()
    lib, dev = be.lib, env.device
    torch.manual_seed(61)
    b, s, hq, hkv = (2, 1024, 8, 2) if env.big else (1, 200, 4, 2)
    row = (hq + 2 * hkv) * d
    qkv = torch.randn(b, s, row).bfloat16().to(dev)
    inv = 1.0 / (500000.0 ** (torch.arange(0, d, 2).float() / d))
    fr = torch.arange(s).float()[:, None] * inv[None]
    emb = torch.cat((fr, fr), -1)
    cos, sin = emb.cos().bfloat16().to(dev).contiguous(), emb.sin().bfloat16().to(dev).contiguous()
    scale = 1 / math.sqrt(d)
    c = scale * 1.4426950408889634
    plain, scaled = qkv.clone(), qkv.clone()
    st = be.stream(qkv)
    stream = ctypes.c_void_p(st) if st else None
    for buf, qh, qs in ((plain, 0, 1.0), (scaled, hq, c)):
        lib.check(lib.tamd_rope_inplace(buf.data_ptr(), cos.data_ptr(), sin.data_ptr(), b * s, s, row, hq + hkv, d, 1, 0,
                                        qh, qs, _cabi.TAMD_BF16, stream), "rope")
    # the scaled query heads: round((round(x cos) + round(rot(x) sin)) * c); key heads and values as before
    x = qkv[..., :hq * d].view(b, s, hq, d).float()
    rot = torch.cat((-x[..., d // 2:], x[..., :d // 2]), -1)
    cs, sn = cos.float()[None, :, None], sin.float()[None, :, None]
    want = (((x * cs).bfloat16().float() + (rot * sn).bfloat16().float()) * torch.tensor(c, dtype=torch.float32)).bfloat16()
    assert torch.equal(scaled[..., :hq * d].view(b, s, hq, d), want)
    assert torch.equal(scaled[..., hq * d:], plain[..., hq * d:])

    def views(buf):
        return (buf[..., :hq * d].view(b, s, hq, d), buf[..., hq * d:(hq + hkv) * d].view(b, s, hkv, d),
                buf[..., (hq + hkv) * d:].view(b, s, hkv, d))

    do = torch.randn(b, s, hq, d).bfloat16().to(dev)
    # the yardstick is the fp32 model: the rotary embedding WITHOUT roundings, then fp32 eager attention (against the
    # reference's rounded q the pre-scaled form would count two roundings -- its own and the yardstick's -- the
    # kernel-scaled form one)
    xk = qkv[..., hq * d:(hq + hkv) * d].view(b, s, hkv, d).float()
    rotk = torch.cat((-xk[..., d // 2:], xk[..., :d // 2]), -1)
    qr = (x * cs + rot * sn).requires_grad_(True)
    kr = (xk * cs + rotk * sn).requires_grad_(True)
    vr = views(plain)[2].detach().clone().float().requires_grad_(True)
    ref = ref_attention(qr, kr, vr, scale, True, None)
    ref.backward(do.float())
    errs = {}
    for tag, buf, flag in (("kernel-scaled", plain, 0), ("pre-scaled", scaled, 1)):
        q, k, v = views(buf)
        o = torch.empty(b, s, hq, d, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(b, hq, s, dtype=torch.float32, device=dev)
        grads = torch.zeros_like(buf)
        dq, dk, dv = views(grads)
        delta = torch.empty(2, b, hq, s, dtype=torch.float32, device=dev)
        bp = _cabi.AttnBwdParams()
        fp = bp.fwd
        fp.q, fp.k, fp.v, fp.o, fp.lse, fp.key_valid, fp.q_start = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), None, None
        fp.batch, fp.seq_q, fp.heads_q, fp.head_dim, fp.seq_k, fp.heads_kv = b, s, hq, d, s, hkv
        for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
            setattr(fp, f"{name}_stride_b", t.stride(0))
            setattr(fp, f"{name}_stride_s", t.stride(1))
            setattr(fp, f"{name}_stride_h", t.stride(2))
        fp.scale, fp.causal, fp.dtype, fp.dropout_p, fp.dropout_seed, fp.q_prescaled = scale, 1, _cabi.TAMD_BF16, 0.0, 0, flag
        bp.dout, bp.dq, bp.dk, bp.dv, bp.delta = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
        bp.rope_cos, bp.rope_sin, bp.rope_cos_batch = None, None, 1
        lib.check(lib.tamd_attn_fwd(ctypes.byref(fp), stream), "fwd")
        lib.check(lib.tamd_attn_bwd(ctypes.byref(bp), stream), "bwd")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        errs[tag] = (rel_err(o, ref), rel_err(dq, qr.grad), rel_err(dk, kr.grad), rel_err(dv, vr.grad))
        assert errs[tag][0] < 0.0052 and max(errs[tag][1:]) < 0.0065, (tag, errs[tag])   # (gradients are w.r.t. the UNSCALED q)
    # measured on the CPU model: O 0.00316 -> 0.00288, dq 0.00403 -> 0.00385, dk 0.00423 -> 0.00387, dv 0.00373 -> 0.00320
    print("prescaled-q errors (O, dq, dk, dv):", d, errs)
    for tag, e4 in errs.items():  # into the parity report (gpurun_out/parity_hip.json on MI355X)
        for nm, e in zip(("O", "dq", "dk", "dv"), e4):
            record("attn_prescaled_q", f"d{d}:{tag}:{nm}", e)
    # MI355X (profiles/r04a_parity.json), pre-scaled vs kernel-scaled (O, dq, dk, dv): head_dim 128 0.00324 / 0.00415 / 0.00418 /
    # 0.00342 vs 0.00349 / 0.00433 / 0.00448 / 0.00382; head_dim 64 0.00322 / 0.00422 / 0.00428 / 0.00343 vs 0.00349 / 0.00446 /
    # 0.00461 / 0.00393 -- ahead in every output at both head dims.  The CPU model's small head_dim-64 case (200 keys) puts dq
    # 1-3 % the other way round, hence its slack.
    slack = 1.0 if (d == 128 or env.big) else 1.03
    assert all(a <= slack * b_ for a, b_ in zip(errs["pre-scaled"], errs["kernel-scaled"])), errs
    assert errs["pre-scaled"][0] < 0.99 * slack * errs["kernel-scaled"][0], errs  # one rounding of q less


ATTN_CASES_SMALL = [
    # b, sq, sk, hq, hkv, d, causal, mask
    (1, 128, 128, 2, 1, 128, True, False),
    (1, 320, 320, 4, 2, 128, True, False),   # dK/dV: tiles without the mask test, then the diagonal ones, per wave
    (2, 200, 200, 4, 2, 64, False, True),
    (1, 130, 130, 2, 2, 128, False, False),
    (1, 577, 577, 1, 1, 64, False, False),   # CLIP-L/336: 577 tokens, no tile multiple
    (2, 192, 192, 4, 1, 128, True, True),
    (1, 96, 224, 2, 1, 64, True, False),     # seq_q != seq_k (causal offset)
]
ATTN_CASES_BIG = [
    (2, 4096, 4096, 32, 8, 128, True, False),   # Llama-3-8B shape (batch reduced)
    (4, 512, 512, 12, 12, 64, False, True),     # bert-base with padding
    (1, 577, 577, 16, 16, 64, False, False),
    (2, 1000, 1000, 8, 2, 128, True, True),
    (1, 257, 1024, 4, 4, 64, True, False),
]


def test_attention_fwd_bwd(env):
    dev = env.device
    for case in (ATTN_CASES_BIG if env.big else ATTN_CASES_SMALL):
        b, sq, sk, hq, hkv, d, causal, use_mask = case
        torch.manual_seed(12)
        q = torch.randn(b, sq, hq, d).bfloat16().to(dev).requires_grad_(True)
        k = torch.randn(b, sk, hkv, d).bfloat16().to(dev).requires_grad_(True)
        v = torch.randn(b, sk, hkv, d).bfloat16().to(dev).requires_grad_(True)
        kv = None
        if use_mask:
            kv = torch.ones(b, sk, dtype=torch.bool, device=dev)
            for i in range(b):
                kv[i, sk - 5 - 7 * i:] = False
        scale = 1 / math.sqrt(d)
        o = ops.attention(q, k, v, scale, causal, kv)
        qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ref = ref_attention(qr, kr, vr, scale, causal, kv)
        assert rel_err(o, ref) < 0.0049, case
        do = torch.randn_like(o)
        o.backward(do)
        ref.backward(do.float())
        for name, a, r in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
            assert rel_err(a, r) < 0.0057, (case, name)


def test_attention_copies_views_the_kernels_cannot_address(env):
    """The C ABI wants rows that follow each other upwards (include/tamd.h: head_dim <= stride_s <= 2^24).  An expanded operand
    (row stride 0: every key the same row) is copied by the op instead of being refused; values and gradients match the
    contiguous call bit for bit."""
    torch.manual_seed(13)
    dev = env.device
    b, s, hq, hkv, d = 1, 96, 2, 1, 64
    q = torch.randn(b, s, hq, d).bfloat16().to(dev).requires_grad_(True)
    k_row = torch.randn(b, 1, hkv, d).bfloat16().to(dev)
    v = torch.randn(b, s, hkv, d).bfloat16().to(dev).requires_grad_(True)
    k_view = k_row.expand(b, s, hkv, d)
    assert k_view.stride(1) == 0
    k_c = k_view.contiguous().requires_grad_(True)
    scale = 1 / math.sqrt(d)
    o1 = ops.attention(q, k_view, v, scale, True)
    o2 = ops.attention(q, k_c, v, scale, True)
    assert torch.equal(o1, o2)
    do = torch.randn_like(o1)
    g1 = torch.autograd.grad(o1, (q, v), do)
    g2 = torch.autograd.grad(o2, (q, v), do)
    assert all(torch.equal(a, b_) for a, b_ in zip(g1, g2))
    # a K / V expanded over HEADS (MQA written as `k.expand(b, s, H, d)`) or over the BATCH passes every stride
    # check but overlaps itself -- the backward would allocate dK with those strides and every head / batch entry would write
    # the same memory.  Copied like the row-expanded one: gradients with respect to k equal the contiguous call's, bit for bit
    # (autograd sums them over the expanded dimension on both sides).
    b, hq = 2, 2
    q = torch.randn(b, s, hq, d).bfloat16().to(dev).requires_grad_(True)
    for shape in ((b, s, 1, d), (1, s, hq, d)):
        k0 = torch.randn(shape).bfloat16().to(dev).requires_grad_(True)
        v0 = torch.randn(shape).bfloat16().to(dev).requires_grad_(True)
        k1, v1 = (t.detach().clone().requires_grad_(True) for t in (k0, v0))
        kv, vv = k0.expand(b, s, hq, d), v0.expand(b, s, hq, d)
        assert 0 in kv.stride()
        oa = ops.attention(q, kv, vv, scale, True)
        ob = ops.attention(q, k1.expand(b, s, hq, d).contiguous(), v1.expand(b, s, hq, d).contiguous(), scale, True)
        assert torch.equal(oa, ob)
        do = torch.randn_like(oa)
        ga = torch.autograd.grad(oa, (q, k0, v0), do)
        gb = torch.autograd.grad(ob, (q, k1, v1), do)
        assert all(torch.equal(x, y) for x, y in zip(ga, gb)), shape


DROPOUT_CASES_SMALL = [(1, 130, 130, 2, 1, 64, True, False, 0.1), (2, 96, 160, 2, 2, 128, False, True, 0.5),
                       (1, 67, 131, 3, 1, 64, True, False, 0.2)]  # odd lengths: the 2 x 2 hash blocks end ragged
DROPOUT_CASES_BIG = [(2, 1024, 1024, 8, 2, 128, True, False, 0.1), (4, 512, 512, 12, 12, 64, False, True, 0.1),
                     (1, 300, 777, 4, 4, 64, True, True, 0.3)]


def test_attention_dropout_matches_explicit_mask(env):
    """Dropout lives inside the kernels: the keep mask is a counter-based hash of (seed, b, h, q, k) that the host
    can rebuild (ops.dropout_keep_mask), so forward AND backward are checked against eager attention with that
    exact mask (reference: nn.functional.dropout on the softmax output, modeling_llama.py:209)."""
    dev = env.device
    for case in (DROPOUT_CASES_BIG if env.big else DROPOUT_CASES_SMALL):
        b, sq, sk, hq, hkv, d, causal, use_mask, p = case
        torch.manual_seed(21)
        q = torch.randn(b, sq, hq, d).bfloat16().to(dev).requires_grad_(True)
        k = torch.randn(b, sk, hkv, d).bfloat16().to(dev).requires_grad_(True)
        v = torch.randn(b, sk, hkv, d).bfloat16().to(dev).requires_grad_(True)
        kv = None
        if use_mask:
            kv = torch.ones(b, sk, dtype=torch.bool, device=dev)
            kv[0, sk - 9:] = False
        seed = 0x1234567 * 0x9ABCDEF1 + sq
        keep = ops.dropout_keep_mask(seed, b, hq, sq, sk, p)
        assert abs(keep.float().mean().item() - (1 - p)) < 0.02, case      # the hash is unbiased at rate p
        scale = 1 / math.sqrt(d)
        o = ops.attention(q, k, v, scale, causal, kv, dropout_p=p, seed=seed)
        qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ref = ref_attention(qr, kr, vr, scale, causal, kv, keep=keep, drop_p=p)
        assert rel_err(o, ref) < 0.0048, case
        do = torch.randn_like(o)
        o.backward(do)
        ref.backward(do.float())
        for name, a, r in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
            assert rel_err(a, r) < 0.0065, (case, name)
        # a different seed gives a different mask; the same seed repeats bit for bit
        o2 = ops.attention(q.detach(), k.detach(), v.detach(), scale, causal, kv, dropout_p=p, seed=seed)
        o3 = ops.attention(q.detach(), k.detach(), v.detach(), scale, causal, kv, dropout_p=p, seed=seed + 1)
        assert torch.equal(o2, o.detach()) and not torch.equal(o3, o2)


def test_dropout_hash_export_matches_host_mirror(env):
    """The attention-dropout mask as include/tamd.h defines it (tamd_attn_dropout_field: one hash per 2 x 2 block, 16 bits
    per element) against the vectorised host mirror, odd sizes included; the 32-bit mix does not collide on a few indices."""
    lib = ops.backend().lib
    seed = 0xDEADBEEFCAFEF00D
    for (b, h, sq, sk, p) in [(1, 1, 1, 3, 0.5), (2, 3, 5, 7, 0.1), (1, 2, 6, 4, 0.3)]:
        mask = ops.dropout_keep_mask(seed, b, h, sq, sk, p)
        thr16 = int(float(torch.tensor(p, dtype=torch.float32)) * 65536.0)
        for bh in range(b * h):
            for q in range(sq):
                for k in range(sk):
                    f = lib.tamd_attn_dropout_field(seed, bh, sq, sk, q, k)
                    assert 0 <= f < 65536 and bool(mask.view(b * h, sq, sk)[bh, q, k]) == (f >= thr16), (bh, q, k)
    big = ops.dropout_keep_mask(seed, 2, 4, 128, 256, 0.25)
    assert abs(big.float().mean().item() - 0.75) < 0.01          # unbiased at rate p ...
    for sl in (big[..., 0::2, 0::2], big[..., 1::2, 0::2], big[..., 0::2, 1::2], big[..., 1::2, 1::2]):
        assert abs(sl.float().mean().item() - 0.75) < 0.02       # ... in each of the four fields of a block
    a, c = big[..., 0::2, 0::2].float() - 0.75, big[..., 1::2, 1::2].float() - 0.75
    assert abs((a * c).mean().item()) < 0.01                     # ... which do not move together
    idx = [0, 1, 2, 12345, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17]
    assert len({lib.tamd_dropout_hash(seed, i) for i in idx}) == len(idx)


def test_attention_fp16(env):
    """The f16 instantiations of the three attention kernels (CLIP / fp16 checkpoints): forward and backward against
    the fp32 restatement on the same rounded inputs; fp16 probabilities carry 3 more mantissa bits than bf16."""
    dev = env.device
    for (b, sq, hq, hkv, d, causal) in ([(2, 1024, 8, 2, 128, True), (2, 577, 4, 4, 64, False)] if env.big
                                        else [(1, 150, 2, 1, 128, True), (1, 100, 2, 2, 64, False)]):
        torch.manual_seed(33)
        q = torch.randn(b, sq, hq, d).half().to(dev).requires_grad_(True)
        k = torch.randn(b, sq, hkv, d).half().to(dev).requires_grad_(True)
        v = torch.randn(b, sq, hkv, d).half().to(dev).requires_grad_(True)
        scale = 1 / math.sqrt(d)
        o = ops.attention(q, k, v, scale, causal, None)
        assert o.dtype == torch.float16
        qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ref = ref_attention(qr, kr, vr, scale, causal, None)
        assert rel_err(o, ref) < 0.00059, (b, sq, d)
        do = torch.randn_like(o)
        o.backward(do)
        ref.backward(do.float())
        for name, a, r in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
            assert rel_err(a, r) < 0.0007, (name, b, sq, d)


def test_attention_packed_sequences(env):
    """Packed batches (several sequences per row; block-diagonal causal mask of masking_utils.py:182-188, 728-757):
    forward and backward against eager attention with the explicit mask, and against running every sequence alone."""
    dev = env.device
    cases = ([(2, 1024, 8, 2, 128, [[300, 724], [1, 63, 64, 200, 696]]), (1, 777, 4, 4, 64, [[100, 5, 672]])] if env.big
             else [(2, 200, 4, 2, 64, [[70, 130], [1, 63, 64, 72]]), (1, 150, 2, 1, 128, [[40, 5, 105]])])
    for b, s, hq, hkv, d, lens in cases:
        torch.manual_seed(31)
        ids = torch.zeros(b, s, dtype=torch.long)
        for i, ls in enumerate(lens):
            assert sum(ls) == s
            ids[i] = torch.repeat_interleave(torch.arange(len(ls)), torch.tensor(ls))
        q_start = ops.packed_q_start(ids.to(dev))
        assert q_start.dtype == torch.int32 and q_start[0, 0, lens[0][0]].item() == lens[0][0]
        assert q_start[1, 0, 0].item() == lens[0][0] - 1 and q_start[1, 0, s - 1].item() == s - 1
        q = torch.randn(b, s, hq, d).bfloat16().to(dev).requires_grad_(True)
        k = torch.randn(b, s, hkv, d).bfloat16().to(dev).requires_grad_(True)
        v = torch.randn(b, s, hkv, d).bfloat16().to(dev).requires_grad_(True)
        scale = 1 / math.sqrt(d)
        o = ops.attention(q, k, v, scale, True, None, q_start=q_start)
        # eager reference with the explicit block-diagonal causal mask
        qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        g = hq // hkv
        qf = qr.float().permute(0, 2, 1, 3)
        kf = kr.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
        vf = vr.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
        same = (ids[:, :, None] == ids[:, None, :]).to(dev)
        allow = same & torch.tril(torch.ones(s, s, dtype=torch.bool, device=dev))
        sc = (qf @ kf.transpose(-1, -2) * scale).masked_fill(~allow[:, None], float("-inf"))
        ref = (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3)
        assert rel_err(o, ref) < 0.004, (b, s, d)
        do = torch.randn_like(o)
        o.backward(do)
        ref.backward(do.float())
        for name, x, r in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
            assert rel_err(x, r) < 0.0062, (name, b, s, d)
        # each sequence on its own gives the same rows (the kernels skip / mask whole tiles differently: tolerance)
        st = 0
        for ln in lens[0]:
            if ln >= 8:
                alone = ops.attention(q[:1, st:st + ln].detach(), k[:1, st:st + ln].detach(), v[:1, st:st + ln].detach(),
                                      scale, True, None)
                assert rel_err(o[:1, st:st + ln], alone) < 0.0038
            st += ln
    with pytest.raises(RuntimeError, match="tamd"):  # packing is a causal notion (refused by the compiled op)
        ops.attention(q.detach(), k.detach(), v.detach(), scale, False, None, q_start=q_start)


def test_attention_sliding_window_and_chunked(env):
    """The causal sliding-window and chunked masks (masking_utils.py:92-113, 134-138, 161-165) through the kernels' bound
    planes: forward and backward against eager attention with the explicit mask the reference's formulas give -- windows
    shorter than a key tile, windows over several tiles (whole tiles left of the window are skipped), chunks that do not
    align with the tiles, both overlays together, and a right-padded batch on top."""
    dev = env.device
    # (batch, seq, heads_q, heads_kv, head_dim, window, chunk, padded keys of row 0, attention dropout)
    cases = ([(2, 1024, 8, 2, 128, 300, None, 0, 0.0), (1, 777, 4, 4, 64, 37, None, 0, 0.0), (2, 640, 4, 2, 128, None, 200, 0, 0.0),
              (2, 512, 4, 1, 64, 150, 96, 40, 0.0), (2, 768, 4, 2, 64, 400, None, 0, 0.1), (1, 704, 4, 2, 128, None, 352, 0, 0.25)]
             if env.big
             else [(2, 200, 4, 2, 64, 70, None, 0, 0.0), (1, 150, 2, 1, 128, 9, None, 0, 0.0), (2, 160, 2, 2, 64, None, 48, 0, 0.0),
                   (2, 136, 2, 1, 128, 50, 40, 17, 0.0), (1, 260, 2, 1, 64, 150, None, 0, 0.2), (1, 200, 2, 2, 128, None, 100, 0, 0.1)])
    for b, s, hq, hkv, d, window, chunk, pad, p_drop in cases:
        torch.manual_seed(37)
        left = torch.tensor([(5 * i) % 7 for i in range(b)])
        bounds = None
        if window is not None:
            bounds = ops.intersect_q_start(bounds, ops.sliding_window_q_start(b, s, window, dev))
        if chunk is not None:
            bounds = ops.intersect_q_start(bounds, ops.chunked_q_start(b, s, chunk, left, dev))
        key_valid = None
        if pad:
            key_valid = torch.ones(b, s, dtype=torch.bool, device=dev)
            key_valid[0, s - pad:] = False
        q = torch.randn(b, s, hq, d).bfloat16().to(dev).requires_grad_(True)
        k = torch.randn(b, s, hkv, d).bfloat16().to(dev).requires_grad_(True)
        v = torch.randn(b, s, hkv, d).bfloat16().to(dev).requires_grad_(True)
        scale = 1 / math.sqrt(d)
        seed = 0x51D1A6 + s
        o = ops.attention(q, k, v, scale, True, key_valid, q_start=bounds, dropout_p=p_drop, seed=seed)
        qi, ki = torch.arange(s)[:, None], torch.arange(s)[None, :]
        allow = (ki <= qi)[None].expand(b, -1, -1).clone()
        if window is not None:
            allow &= (ki > qi - window)[None]
        if chunk is not None:
            allow &= torch.div(ki[None] - left[:, None, None], chunk, rounding_mode="floor") == \
                torch.div(qi[None] - left[:, None, None], chunk, rounding_mode="floor")
        allow = allow.to(dev)
        if pad:
            allow = allow & key_valid[:, None, :]
        qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        g = hq // hkv
        qf = qr.float().permute(0, 2, 1, 3)
        kf = kr.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
        vf = vr.float().permute(0, 2, 1, 3).repeat_interleave(g, 1)
        # (a query whose window / chunk holds padded keys only has no visible key: zeros, and no gradient through it --
        # test_attention_fully_masked_rows_are_zero; the eager formula gives NaN there)
        seen = allow.any(-1)[:, None, :, None]
        sc = (qf @ kf.transpose(-1, -2) * scale).masked_fill(~allow[:, None], float("-inf")).masked_fill(~seen, 0.0)
        pr = torch.softmax(sc, -1) * seen
        if p_drop:  # the kernels' counter-based keep mask, rebuilt on the host (the packed dK/dV instantiation with dropout)
            pr = pr * ops.dropout_keep_mask(seed, b, hq, s, s, p_drop).to(dev).float() / (1.0 - p_drop)
        ref = (pr @ vf).permute(0, 2, 1, 3)
        assert pad == 0 or not bool(seen.all())
        assert rel_err(o, ref) < (0.0048 if p_drop else 0.004), (b, s, d, window, chunk)
        do = torch.randn_like(o)
        o.backward(do)
        ref.backward(do.float())
        for name, x, r in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
            assert rel_err(x, r) < (0.0065 if p_drop else 0.0062), (name, b, s, d, window, chunk)


def test_attention_spike_forces_rescale(env):
    """Online-softmax rescale path: one key dominates late in the sequence (cdna guide rule 26)."""
    dev = env.device
    b, s, h, d = 1, (1024 if env.big else 256), 1, 64
    torch.manual_seed(13)
    q = torch.randn(b, s, h, d).bfloat16().to(dev)
    k = torch.randn(b, s, h, d).bfloat16().to(dev)
    v = torch.randn(b, s, h, d).bfloat16().to(dev)
    k[0, s - 20, 0] = q[0, 5, 0] * 8  # huge score for query 5 at a late key tile
    o, _ = ops.raw_attn_fwd(q, k, v, 0.125, False)
    assert rel_err(o, ref_attention(q, k, v, 0.125, False, None)) < 0.0031
    assert torch.isfinite(o.float()).all()


def test_attention_fully_masked_rows_are_zero(env):
    dev = env.device
    q = torch.randn(1, 64, 1, 64).bfloat16().to(dev)
    k = torch.randn(1, 64, 1, 64).bfloat16().to(dev)
    v = torch.randn(1, 64, 1, 64).bfloat16().to(dev)
    kv = torch.zeros(1, 64, dtype=torch.bool, device=dev)
    o, lse = ops.raw_attn_fwd(q, k, v, 0.125, False, kv)
    assert (o == 0).all() and torch.isinf(lse).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_swiglu_epilogue_is_bit_identical_to_unfused(env, dtype):
    """gate|up GEMM with the SiLU*up product in the epilogue (tamd_gemm_swiglu) against the two-kernel path (tamd_gemm,
    tamd_swiglu_fwd) it replaces in the fused Llama layer: same fp32 k-order, same rounding points -> same bits, for
    gate|up and for act; ragged token counts, feature counts that are not a multiple of the 128-feature tile, and the
    inference form that never writes gate|up."""
    torch.manual_seed(31)
    shapes = [(4096, 14336, 4096), (1000, 2816, 1024), (333, 1000, 512)] if env.big else [(130, 192, 64), (64, 72, 128)]
    for t, inter, k in shapes:
        x = torch.randn(t, k).to(dtype).to(env.device)
        wgu = (torch.randn(2 * inter, k) * k ** -0.5).to(dtype).to(env.device)
        assert ops.gemm_swiglu_supported(x, wgu)
        gu_ref = ops.raw_gemm(x, wgu)
        act_ref = ops.raw_swiglu_fwd(gu_ref)
        gu, act = ops.raw_gemm_swiglu(x, wgu, need_gu=True)
        assert torch.equal(gu, gu_ref), (t, inter, k)
        assert torch.equal(act, act_ref), (t, inter, k)
        none, act2 = ops.raw_gemm_swiglu(x, wgu, need_gu=False)
        assert none is None and torch.equal(act2, act_ref)
        # against the fp32 formula of the reference (modeling_llama.py:174-176) on the same rounded inputs
        g32, u32 = (x.float() @ wgu.float().t()).split(inter, dim=1)
        want = torch.nn.functional.silu(g32) * u32
        err = rel_err(act, want)
        record("gemm_swiglu", f"{dtype}:{t}x{inter}x{k}", err)
        assert err < 6e-3
    o, a = torch.ops.tamd.gemm_swiglu(x, wgu, True)
    assert torch.equal(o, gu_ref) and torch.equal(a, act_ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_swiglu_bwd_epilogue_is_bit_identical_to_unfused(env, dtype):
    """The down projection's dX GEMM with the SiLU*up backward as its way out (tamd_gemm_swiglu_bwd) against the two kernels it
    replaces in the fused Llama layer's backward (tamd_gemm with a k-major B, tamd_swiglu_bwd): same fp32 k-order, d_act rounded
    at the same point, the same expressions -> same bits for d_gate and d_up; ragged token counts (a partial last row tile, a
    wave whose rows lie wholly past M) and feature counts that are not a multiple of the tile.  Then against the fp32 derivative
    of the reference's expression (modeling_llama.py:174-176) on the same rounded inputs."""
    torch.manual_seed(37)
    shapes = [(4096, 14336, 4096), (1000, 2816, 1024), (333, 1000, 512)] if env.big else [(130, 200, 64), (70, 72, 128)]
    for t, inter, k in shapes:
        dy = torch.randn(t, k).to(dtype).to(env.device)
        wd = (torch.randn(k, inter) * k ** -0.5).to(dtype).to(env.device)
        gu = torch.randn(t, 2 * inter).to(dtype).to(env.device)
        assert ops.gemm_swiglu_bwd_supported(dy, wd, gu)
        d_act = ops.raw_gemm(dy, wd, b_kn=True)
        dgu_ref, _ = ops.raw_swiglu_bwd(gu, d_act)
        gu_before = gu.clone()
        dgu = ops.raw_gemm_swiglu_bwd(dy, wd, gu)
        assert torch.equal(gu, gu_before)  # (the saved activations are read, never written)
        assert torch.equal(dgu[:, :inter], dgu_ref[:, :inter]), (t, inter, k)
        assert torch.equal(dgu[:, inter:], dgu_ref[:, inter:]), (t, inter, k)
        gf = gu[:, :inter].float().requires_grad_(True)
        uf = gu[:, inter:].float().requires_grad_(True)
        (torch.nn.functional.silu(gf) * uf).backward(dy.float() @ wd.float())
        eg, eu = rel_err(dgu[:, :inter], gf.grad), rel_err(dgu[:, inter:], uf.grad)
        record("gemm_swiglu_bwd", f"{dtype}:{t}x{inter}x{k}:dgate", eg)
        record("gemm_swiglu_bwd", f"{dtype}:{t}x{inter}x{k}:dup", eu)
        assert eg < 6e-3 and eu < 6e-3, (eg, eu)
    # a grid the library's policy would split along K (or a decode-sized product) stays on the two kernels
    few = torch.randn(8, 64).to(dtype).to(env.device)
    assert not ops.gemm_swiglu_bwd_supported(few, wd[:64], gu[:8])


@pytest.mark.parametrize("cols", [128, 768, 1024])
def test_dropout_add_layernorm(env, cols):
    """LayerNorm(dropout(x, p) + residual) with the mask drawn inside the norm kernel (BertSelfOutput / BertOutput in train
    mode, modeling_bert.py:289-293): forward and backward against torch ops applied with the SAME mask, rebuilt on the
    host from the exported hash; same seed -> same bits, another seed -> another mask; keep rate ~ 1 - p."""
    torch.manual_seed(33)
    rows = 2048 if env.big else 24
    p, seed = 0.1, 0x1234_5678_9ABC
    dev = env.device
    x = torch.randn(rows, cols).bfloat16().to(dev).requires_grad_(True)
    r = torch.randn(rows, cols).bfloat16().to(dev).requires_grad_(True)
    w = (torch.rand(cols) + 0.5).bfloat16().to(dev).requires_grad_(True)
    b = (torch.randn(cols) * 0.1).bfloat16().to(dev).requires_grad_(True)
    y = ops.dropout_add_layernorm(x, r, w, b, 1e-12, p, seed)
    keep = ops.hidden_dropout_keep_mask(seed, rows, cols, p)
    assert abs(keep.float().mean().item() - (1 - p)) < (0.01 if env.big else 0.05)
    xr, rr, wr, br = (t.detach().float().cpu().requires_grad_(True) for t in (x, r, w, b))
    # the reference's bf16 op chain: dropout rounds, the add rounds, LayerNorm computes in fp32
    dropped = (xr * keep / (1 - p)).bfloat16().float()
    h = (dropped + rr).bfloat16().float()
    yr = torch.nn.functional.layer_norm(h, (cols,), wr, br, 1e-12)
    assert rel_err(y, yr) < 0.0034
    g = torch.randn(rows, cols).bfloat16()
    y.backward(g.to(dev))
    yr.backward(g.float())
    assert rel_err(r.grad, rr.grad) < 0.0034 and rel_err(x.grad, xr.grad) < 0.0034
    assert (x.grad.float().cpu()[~keep] == 0).all()  # dropped elements receive no gradient
    assert rel_err(w.grad, wr.grad) < 4e-3 and rel_err(b.grad, br.grad) < 4e-3
    y2 = ops.dropout_add_layernorm(x.detach(), r.detach(), w.detach(), b.detach(), 1e-12, p, seed)
    y3 = ops.dropout_add_layernorm(x.detach(), r.detach(), w.detach(), b.detach(), 1e-12, p, seed + 1)
    assert torch.equal(y2, y.detach()) and not torch.equal(y3, y2)
    # p = 0 is the plain fused add + LayerNorm
    y0 = ops.dropout_add_layernorm(x.detach(), r.detach(), w.detach(), b.detach(), 1e-12, 0.0, seed)
    assert torch.equal(y0, ops.layernorm(x.detach(), w.detach(), b.detach(), 1e-12, residual=r.detach())[0])


def test_attention_backward_rope_epilogue_is_bit_identical_to_unfused(env):
    """The transposed rotary embedding on dq / dk inside the attention backward kernels (tamd_attn_bwd rope_cos /
    rope_sin) gives the bits of the stored gradients followed by tamd_rope_inplace(conj): shared and per-batch cos / sin,
    GQA, ragged sequence length; dv untouched."""
    import math

    torch.manual_seed(43)
    dev = env.device
    for (b, s, hq, hkv) in ([(2, 1000, 8, 2), (1, 4096, 4, 4)] if env.big else [(2, 72, 2, 1), (1, 130, 2, 2)]):
        d = 128
        qkv = torch.randn(b * s, (hq + 2 * hkv) * d).bfloat16().to(dev)
        q = qkv[:, : hq * d].view(b, s, hq, d)
        k = qkv[:, hq * d: (hq + hkv) * d].view(b, s, hkv, d)
        v = qkv[:, (hq + hkv) * d:].view(b, s, hkv, d)
        scale = 1 / math.sqrt(d)
        o, lse = ops.raw_attn_fwd(q, k, v, scale, True)
        do = torch.randn(b, s, hq, d).bfloat16().to(dev)
        for cb in (1, b):
            ang = torch.rand(cb, s, d // 2) * 6.28
            cos = torch.cat([ang.cos(), ang.cos()], -1).bfloat16().to(dev)
            sin = torch.cat([ang.sin(), ang.sin()], -1).bfloat16().to(dev)
            if cb == 1:
                cos, sin = cos[0], sin[0]
            ref = torch.zeros_like(qkv)
            rq, rk, rv = ref[:, : hq * d].view(b, s, hq, d), ref[:, hq * d: (hq + hkv) * d].view(b, s, hkv, d), ref[:, (hq + hkv) * d:].view(b, s, hkv, d)
            ops.raw_attn_bwd(q, k, v, o, lse, do, scale, True, dq=rq, dk=rk, dv=rv)
            ops.raw_rope_(ref, cos, sin, s, hq + hkv, d, conj=True)
            got = torch.zeros_like(qkv)
            gq, gk, gv = got[:, : hq * d].view(b, s, hq, d), got[:, hq * d: (hq + hkv) * d].view(b, s, hkv, d), got[:, (hq + hkv) * d:].view(b, s, hkv, d)
            assert ops.attn_bwd_rope_supported(q, k, cos, d)
            ops.raw_attn_bwd(q, k, v, o, lse, do, scale, True, dq=gq, dk=gk, dv=gv, rope=(cos, sin))
            assert torch.equal(got, ref), (b, s, hq, hkv, cb)


def test_residual_epilogue_on_a_small_grid_goes_through_split_k(env):
    """o_proj / down_proj of a short prompt (80 tiles of 256 x 256 on 256 CUs) go through split-K, whose reduction applies the
    residual: the roundings of the one-kernel residual epilogue (the fp32 partial sums of the K ranges are added in a
    different order)."""
    torch.manual_seed(47)
    dev = env.device
    for (m, n, k) in ([(1088, 4096, 11008), (577, 1024, 4096)] if env.big else [(200, 264, 4096)]):
        x = torch.randn(m, k).bfloat16().to(dev)
        w = (torch.randn(n, k) * 0.05).bfloat16().to(dev)
        r = torch.randn(m, n).bfloat16().to(dev)
        assert ops.gemm_workspace_bytes(m, n, k, ops.EPI_RESIDUAL) > 0
        ref = ops.raw_gemm(x, w, residual=r, epilogue=ops.EPI_RESIDUAL, sched="fl")  # a schedule hint turns split-K off
        got = ops.raw_gemm(x, w, residual=r, epilogue=ops.EPI_RESIDUAL)
        # split-K sums the fp32 partials of the K ranges: not the bits of the unsplit order, but the same roundings
        assert rel_err(got, ref) < 0.00011 and (got != ref).float().mean() < 0.2
        assert rel_err(got, (x.float() @ w.float().t()).bfloat16().float() + r.float()) < 0.0036


def test_gemm_piece_placements_are_bit_identical(env):
    """The schedules of the full-line GEMM kernel -- the three-barrier loop (the product schedule of forward and dW) and the
    one-barrier ring with the early (dX) or the late LDS-DMA piece placement -- compute the same bits in every layout; the
    diagnostic entry point tamd_gemm_set_dbg(32 / 128 / 1024 / 2048) forces one of them (tools/gemm_piece_ab.py measures them)
    and refuses every other value.  The one- and three-stage products pin the prologue's park() at j == nst and the odd-count
    tail of the three-barrier loop, with ragged last tiles in M and N."""
    lib = ops.backend().lib
    if not hasattr(lib, "tamd_gemm_set_dbg"):
        pytest.skip("needs the diagnostic entry points (CPU execution model or libtamd_diag.so)")
    try:  # a retired arm is refused and the selector stays where it was
        assert lib.tamd_gemm_set_dbg(1024) == 0 and lib.tamd_gemm_get_dbg() == 1024
        assert lib.tamd_gemm_set_dbg(64) != 0 and lib.tamd_gemm_get_dbg() == 1024
    finally:
        lib.tamd_gemm_set_dbg(0)
    assert lib.tamd_gemm_get_dbg() == 0
    torch.manual_seed(61)
    dev = env.device
    for m, n, k in [(1536, 1024, 1280) if env.big else (512, 520, 768), (264, 520, 64), (264, 520, 192)]:
        x = torch.randn(m, k).bfloat16().to(dev)
        w = (torch.randn(n, k) * k ** -0.5).bfloat16().to(dev)
        layouts = [((x, w), {}), ((x, w.t().contiguous()), {"b_kn": True}),
                   ((x.t().contiguous(), w.t().contiguous()), {"a_km": True, "b_kn": True})]
        ref = x.float() @ w.float().t()
        try:
            for args, kw in layouts:
                plain = ops.raw_gemm(*args, sched="fl", **kw)
                assert rel_err(plain, ref) < 0.0036
                # (32 / 128: the ring with the early / late placement; 1024: the three-barrier loop; 2048: the ring forced where
                # three barriers are the product)
                for dbg in (32, 128, 1024, 2048):
                    assert lib.tamd_gemm_set_dbg(dbg) == 0
                    assert torch.equal(ops.raw_gemm(*args, sched="fl", **kw), plain), ((m, n, k), kw, dbg)
                    lib.tamd_gemm_set_dbg(0)
        finally:
            lib.tamd_gemm_set_dbg(0)


# ---- round 4: the bert-base fusions (pre-scaled query columns, bias gradients
# ---- accumulated by the kernels that produce the tensors they sum)
@pytest.mark.parametrize("sched", ["pp", "fl", "sm"])
def test_gemm_colscale_scales_the_query_columns_before_their_one_rounding(env, sched):
    """tamd_gemm_colscale (the q|k|v projection of BertSelfAttention, modeling_bert.py:175-177, delivering pre-scaled queries):
    columns >= scale_cols carry the bits of the plain GEMM; the scaled columns are round((acc + bias) * s) -- closer to the
    fp32 product than rounding first and scaling after, and exactly the plain result for s = 1 / a power of two."""
    import ctypes

    from transformers_amd import _cabi

    torch.manual_seed(72)
    dev = env.device
    be = ops.backend()
    lib = be.lib
    hint = {"pp": 1, "sm": 2, "fl": 3}[sched] << 8
    for (m, n, k, sc) in ([(4096, 2304, 768, 768), (1000, 1032, 320, 344)] if env.big else [(264, 248, 128, 80), (72, 264, 64, 264)]):
        x = torch.randn(m, k).bfloat16().to(dev)
        w = (torch.randn(n, k) * 0.1).bfloat16().to(dev)
        b = torch.randn(n).bfloat16().to(dev)
        plain = ops.raw_gemm(x, w, bias=b, epilogue=ops.EPI_BIAS, sched=sched)
        ref = x.float() @ w.float().t() + b.float()

        def run(s, bias=b):
            c = torch.empty(m, n, dtype=torch.bfloat16, device=dev)
            st = be.stream(x)
            lib.check(lib.tamd_gemm_colscale(x.data_ptr(), w.data_ptr(), c.data_ptr(), None if bias is None else bias.data_ptr(),
                                             m, n, k, k, k, n, hint, sc, s, _cabi.TAMD_BF16, ctypes.c_void_p(st) if st else None),
                      "gemm_colscale")
            if dev.type == "cuda":
                torch.cuda.synchronize()
            return c

        s = 0.125 * 1.4426950408889634
        c = run(s)
        assert torch.equal(c[:, sc:], plain[:, sc:])
        e_pre = rel_err(c[:, :sc], ref[:, :sc] * s)
        e_post = rel_err((plain[:, :sc].float() * s).bfloat16(), ref[:, :sc] * s)  # scale after rounding: two roundings
        assert e_pre < 0.0034 and e_pre <= e_post * 1.001, (e_pre, e_post)
        assert torch.equal(run(1.0), plain) and torch.equal(run(0.25)[:, :sc].float(), plain[:, :sc].float() * 0.25)
        assert torch.equal(run(1.0, None), ops.raw_gemm(x, w, sched=sched))  # no bias
    c2 = torch.ops.tamd.gemm_colscale(x, w, b, sc, s)
    assert torch.equal(c2, c)


@pytest.mark.parametrize("cols", [768, 1024])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layernorm_backward_accumulates_the_dense_bias_gradient(env, cols, p):
    """ABI 8: the LayerNorm backward of a post-LN block (modeling_bert.py:289-293) also returns the column sums of the
    gradient it writes for the dense output -- dx without hidden dropout, dx_drop with -- i.e. the dense bias gradient,
    without changing any other output."""
    torch.manual_seed(73)
    rows = 4096 if env.big else 37
    dev = env.device
    h = torch.randn(rows, cols).bfloat16().to(dev)
    dy = torch.randn(rows, cols).bfloat16().to(dev)
    w = (torch.rand(cols) + 0.5).bfloat16().to(dev)
    mean = h.float().mean(-1)
    rstd = (h.float().var(-1, unbiased=False) + 1e-12).rsqrt()
    T = torch.ops.tamd
    if p == 0.0:
        dx, dw, db, dc = T.layernorm_bwd(dy, h, w, mean, rstd, None, True, True)
        dx0, dw0, db0, none = T.layernorm_bwd(dy, h, w, mean, rstd, None, True, False)
        src = dx
    else:
        seed = 0x5EED_1234
        dx, dxd, dw, db, dc = T.layernorm_dropout_bwd(dy, h, w, mean, rstd, p, seed, None, True, True)
        dx0, dxd0, dw0, db0, none = T.layernorm_dropout_bwd(dy, h, w, mean, rstd, p, seed, None, True, False)
        assert torch.equal(dxd, dxd0)
        src = dxd
    assert none.numel() == 0 and torch.equal(dx, dx0) and torch.equal(dw, dw0) and torch.equal(db, db0)
    want = src.float().sum(0)
    assert rel_err(dc, want) < 0.0034  # (one output rounding; fp32 sums of the stored values)
    assert rel_err(dc, ops.raw_colsum(src)) < 0.0034


@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_bias_act_backward_accumulates_the_bias_gradient(env, act):
    """ABI 8: tamd_bias_act_bwd with dbias returns dx (the bits of the plain kernel) and its column sums in one pass."""
    torch.manual_seed(74)
    rows, cols = (4100, 3072) if env.big else (37, 136)
    dev = env.device
    x = torch.randn(rows, cols).bfloat16().to(dev)
    b = torch.randn(cols).bfloat16().to(dev)
    dy = torch.randn(rows, cols).bfloat16().to(dev)
    code = ops.ACT_CODES[act]
    for bias in (None, b):
        dx, db = ops.raw_bias_act_bwd(x, bias, dy, code, need_colsum=True)
        assert torch.equal(dx, ops.raw_bias_act_bwd(x, bias, dy, code))
        assert rel_err(db, dx.float().sum(0)) < 0.0034


DECODE_CASES_SMALL = [
    # b, sq, sk, hq, hkv, d, causal, mask
    (2, 1, 300, 4, 2, 128, True, False),    # one new token, GQA: the heads of a KV head become the rows of a query tile
    (1, 1, 200, 4, 4, 64, True, True),      # MHA, left-padded cache
    (2, 5, 260, 4, 2, 64, True, False),     # a short block of new tokens: causal inside the block
    (1, 1, 129, 2, 1, 128, False, True),    # cross-attention style (not causal), ragged key count, padding
]
DECODE_CASES_BIG = [
    (1, 1, 4096, 32, 8, 128, True, False),   # Llama-3-8B, one sequence, 4k cache
    (8, 1, 8192, 32, 8, 128, True, True),    # batch 8, 8k cache, padded
    (2, 1, 1088, 32, 32, 128, True, False),  # Llama-2-7B-shaped (LLaVA): MHA
    (4, 16, 2000, 12, 12, 64, True, False),  # 16 new rows, ragged
    (3, 7, 515, 16, 4, 64, False, True),
]


def test_attention_decode_split_kv(env):
    """tamd_attn_decode (few query rows over a KV cache: cache_utils.py:1730, 1822; modeling_llama.py:243-281): the split-KV
    schedule -- query heads of a KV head as tile rows, key range split over workgroups, fp32 partials merged -- returns what
    the training kernel returns (same roundings of P; the pieces are summed in a different order) and what fp32 eager
    attention returns, and is what `torch.ops.tamd.attention` runs for such shapes."""
    import ctypes

    from transformers_amd import _cabi

    dev = env.device
    be = ops.backend()
    lib = be.lib
    for case in (DECODE_CASES_BIG if env.big else DECODE_CASES_SMALL):
        b, sq, sk, hq, hkv, d, causal, use_mask = case
        torch.manual_seed(81)
        q = torch.randn(b, sq, hq, d).bfloat16().to(dev)
        kc = torch.randn(b, sk + 40, hkv, d).bfloat16().to(dev)  # a pre-allocated cache: the first sk slots are in use
        vc = torch.randn(b, sk + 40, hkv, d).bfloat16().to(dev)
        k, v = kc[:, :sk], vc[:, :sk]
        kv = None
        if use_mask:
            kv = torch.ones(b, sk, dtype=torch.bool, device=dev)
            kv[0, :37] = False  # left padding
        scale = d ** -0.5
        ref = ref_attention(q, k, v, scale, causal, kv)
        o = torch.empty(b, sq, hq, d, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(b, hq, sq, dtype=torch.float32, device=dev)
        ap = _cabi.AttnParams()
        ap.q, ap.k, ap.v, ap.o, ap.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
        kvb = None if kv is None else kv.to(torch.uint8).contiguous()
        ap.key_valid, ap.q_start = (None if kvb is None else kvb.data_ptr()), None
        ap.batch, ap.seq_q, ap.heads_q, ap.head_dim, ap.seq_k, ap.heads_kv = b, sq, hq, d, sk, hkv
        for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
            setattr(ap, f"{name}_stride_b", t.stride(0))
            setattr(ap, f"{name}_stride_s", t.stride(1))
            setattr(ap, f"{name}_stride_h", t.stride(2))
        ap.scale, ap.causal, ap.dtype, ap.dropout_p, ap.dropout_seed, ap.q_prescaled = scale, int(causal), _cabi.TAMD_BF16, 0.0, 0, 0
        nbytes = lib.tamd_attn_decode_workspace_bytes(ctypes.byref(ap))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st = be.stream(q)
        stream = ctypes.c_void_p(st) if st else None
        lib.check(lib.tamd_attn_decode(ctypes.byref(ap), ws.data_ptr(), nbytes, stream), "decode")
        o_train = torch.empty_like(o)
        lse_train = torch.empty_like(lse)
        ap.o, ap.lse = o_train.data_ptr(), lse_train.data_ptr()
        lib.check(lib.tamd_attn_fwd(ctypes.byref(ap), stream), "fwd")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert rel_err(o, ref) < 0.0045, case
        assert rel_err(o, o_train) < 0.0035, case       # same P roundings, another summation order (+ one output rounding)
        assert max_err(lse, lse_train) < 2e-3, case
        # the dispatcher op takes this path for cache-shaped calls
        o2 = ops.attention(q, k, v, scale, causal, kv)
        assert torch.equal(o2, o), case


def test_dropout_seed_from_device_memory_is_the_same_mask(env):
    """ABI 8: a dropout seed read from device memory (tamd_attn_params.dropout_seed_dev, `seed_dev` of the LayerNorm-dropout
    entry points: what a captured training step uses, ops.dropout_seed_tensor) gives the bits of the same seed passed by
    value -- forward and backward, attention and hidden-state dropout."""
    torch.manual_seed(91)
    dev = env.device
    seed = 0x3A5C_7E91_2B4D_6F80 & ((1 << 62) - 1)
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    b, s, hq, hkv, d = (2, 512, 12, 12, 64) if env.big else (1, 100, 2, 1, 64)
    q = torch.randn(b, s, hq, d).bfloat16().to(dev)
    k = torch.randn(b, s, hkv, d).bfloat16().to(dev)
    v = torch.randn(b, s, hkv, d).bfloat16().to(dev)
    do = torch.randn(b, s, hq, d).bfloat16().to(dev)
    o1, l1 = ops.raw_attn_fwd(q, k, v, d ** -0.5, False, dropout_p=0.1, seed=seed)
    o2, l2 = ops.raw_attn_fwd(q, k, v, d ** -0.5, False, dropout_p=0.1, seed=12345, seed_dev=sd)  # (the value is ignored)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    g1 = ops.raw_attn_bwd(q, k, v, o1, l1, do, d ** -0.5, False, dropout_p=0.1, seed=seed)
    g2 = ops.raw_attn_bwd(q, k, v, o1, l1, do, d ** -0.5, False, dropout_p=0.1, seed=0, seed_dev=sd)
    assert all(torch.equal(a, c) for a, c in zip(g1, g2))
    o3, _ = ops.raw_attn_fwd(q, k, v, d ** -0.5, False, dropout_p=0.1, seed=0, seed_dev=sd + 1)
    assert not torch.equal(o3, o1)
    rows, cols = (1024, 768) if env.big else (24, 128)
    x = torch.randn(rows, cols).bfloat16().to(dev)
    r = torch.randn(rows, cols).bfloat16().to(dev)
    w = (torch.rand(cols) + 0.5).bfloat16().to(dev)
    bb = torch.randn(cols).bfloat16().to(dev)
    f1 = ops.raw_layernorm_dropout_fwd(x, w, bb, 1e-12, r, 0.1, seed)
    f2 = ops.raw_layernorm_dropout_fwd(x, w, bb, 1e-12, r, 0.1, 777, seed_dev=sd)
    assert all(torch.equal(a, c) for a, c in zip(f1, f2))
    dy = torch.randn(rows, cols).bfloat16().to(dev)
    y, h, mean, rstd = f1
    b1 = ops.raw_layernorm_dropout_bwd(dy, h, w, mean, rstd, 0.1, seed)
    b2 = ops.raw_layernorm_dropout_bwd(dy, h, w, mean, rstd, 0.1, 0, seed_dev=sd)
    assert all(torch.equal(a, c) for a, c in zip(b1, b2))


def test_gemv_decode_projections(env):
    """M <= 16 rows against a row-major weight (the projections of a cached decode step: modeling_llama.py:254-256, 280, 174-176,
    480 with one new token per sequence) run on the weight-streaming kernel of csrc/gemv.hip: fp32 reference on the same
    bf16-rounded operands, plain / bias / residual (+ bias) epilogues with the GEMM kernels' roundings, ragged N and K, strided
    inputs (a [B, 1, H] slice of a longer buffer); a schedule hint keeps the product on the tile kernels, M = 17 is theirs anyway."""
    torch.manual_seed(101)
    dev = env.device
    shapes = ([(4096, 4096), (6144, 4096), (1032, 520), (28672, 4096), (32776, 64)] if env.big else
              [(264, 520), (72, 4104), (16, 64), (16392, 64), (32776, 64)])  # (the last two: 2 / 4 row blocks per workgroup)
    for (n, k) in shapes:
        w = (torch.randn(n, k) * 0.05).bfloat16().to(dev)
        bias = torch.randn(n).bfloat16().to(dev)
        # 1 .. 4: the VALU kernel, 5 .. 16: the MFMA one (the CPU model takes the edges of both ranges: every row count on the
        # widest shapes was 100 s of the CPU suite)
        for m in ((1, 2, 3, 4, 5, 8, 13, 16) if env.big or n < 16384 else (1, 4, 5, 16)):
            xbuf = torch.randn(m, 2 * k).bfloat16().to(dev)
            x = xbuf[:, :k]  # row stride 2k
            res = torch.randn(m, n).bfloat16().to(dev)
            ref = x.float() @ w.float().t()
            got = ops.raw_gemm(x, w)
            assert got.shape == (m, n) and rel_err(got, ref) < 0.0034, (m, n, k)
            tiles = ops.raw_gemm(x, w, sched="fl" if k % 64 == 0 else "pp")
            assert rel_err(got, tiles) < 0.004, (m, n, k)
            got = ops.raw_gemm(x, w, bias=bias, epilogue=ops.EPI_BIAS)
            assert rel_err(got, ref + bias.float()) < 0.0034, (m, n, k)
            for b in (None, bias):
                got = ops.raw_gemm(x, w, bias=b, residual=res, epilogue=ops.EPI_RESIDUAL)
                want = (ref + (b.float() if b is not None else 0)).bfloat16().float() + res.float()
                assert rel_err(got, want) < 0.0034, (m, n, k, b is not None)
        x17 = torch.randn(17, k).bfloat16().to(dev)
        assert rel_err(ops.raw_gemm(x17, w), x17.float() @ w.float().t()) < 0.0034
    x = torch.randn(2, 256).half().to(dev)
    w = (torch.randn(264, 256) * 0.05).half().to(dev)
    assert rel_err(ops.raw_gemm(x, w), x.float() @ w.float().t()) < 0.0006   # fp16
    # LlamaMLP's inner product at M = batch (tamd_gemm_swiglu -> gemv_swiglu_kernel): the bits of product + swiglu kernel
    for (m, inter, k) in ([(1, 14336, 4096), (8, 11008, 4096), (16, 14336, 4096)] if env.big else
                          [(1, 264, 128), (3, 72, 192), (8, 16, 64), (11, 72, 192), (16, 264, 128)]):
        x = torch.randn(m, k).bfloat16().to(dev)
        wgu = (torch.randn(2 * inter, k) * 0.05).bfloat16().to(dev)
        assert ops.gemm_swiglu_supported(x, wgu)
        gu, act = ops.raw_gemm_swiglu(x, wgu, need_gu=True)
        plain = ops.raw_gemm(x, wgu, sched="fl")                 # the tile kernel's gate | up
        assert rel_err(gu, plain) < 0.004
        assert torch.equal(act, ops.raw_swiglu_fwd(gu)), (m, inter, k)   # same expression on the same rounded gate | up
        assert torch.equal(ops.raw_gemm_swiglu(x, wgu, need_gu=False)[1], act)
    # the layer-level entry: ops.linear on a [B, 1, H] decode input
    h = torch.randn(3, 1, 520).bfloat16().to(dev)
    w = (torch.randn(264, 520) * 0.05).bfloat16().to(dev)
    assert rel_err(ops.linear(h, w), h.float() @ w.float().t()) < 0.0034


def test_gemm_group_weight_gradients(env):
    """tamd_gemm_group (ABI 8): the weight gradients of one layer's dense layers in ONE launch.  Groups that fit one round
    of workgroups are split along K with one common range length (fp32 partials + one grouped reduction): the single
    product's result up to fp32 summation order; groups too large to split: its bits.  Plain and accumulating, through the
    C ABI and through torch.ops.tamd.gemm_dw_group."""
    import ctypes

    from transformers_amd import _cabi

    torch.manual_seed(97)
    dev = env.device
    lib = ops.backend().lib
    if env.big:   # bert-base layer (9 + 36 + 36 + 27 tiles over 16384 tokens); a ragged pair; Llama-sized (no split: same bits)
        groups = [[(768, 768, 16384), (3072, 768, 16384), (768, 3072, 16384), (2304, 768, 16384)],
                  [(264, 520, 4096), (1000, 136, 8192)], [(4096, 4096, 2048), (1024, 4096, 2048)]]
    else:
        groups = [[(256, 128, 2048), (264, 136, 1088), (128, 520, 2048)], [(256, 256, 1024)], [(2560, 2560, 128), (256, 2816, 64)]]
    for gi, group in enumerate(groups):
        dys = [torch.randn(k, m).bfloat16().to(dev) for (m, n, k) in group]
        xs = [(torch.randn(k, n) * 0.1).bfloat16().to(dev) for (m, n, k) in group]
        single = [ops.raw_gemm(a, b, a_km=True, b_kn=True, sched="fl") for a, b in zip(dys, xs)]  # unsplit, one by one
        outs = torch.ops.tamd.gemm_dw_group(dys, xs)
        pr = (_cabi.GemmProblem * len(group))()
        acc = [torch.randn(m, n).bfloat16().to(dev) for (m, n, k) in group]
        acc0 = [a.clone() for a in acc]
        for i, (m, n, k) in enumerate(group):
            pr[i] = _cabi.GemmProblem(dys[i].data_ptr(), xs[i].data_ptr(), acc[i].data_ptr(), m, n, k, m, n, n)
        need = lib.tamd_gemm_group_workspace_bytes(ctypes.byref(pr), len(group), 3)
        tiles = sum(-(-m // 256) * -(-n // 256) for (m, n, k) in group)
        assert (need > 0) == (tiles <= 256 and max(k for (_, _, k) in group) // 64 > 16), (group, need)
        for i, (m, n, k) in enumerate(group):
            ref = dys[i].float().t() @ xs[i].float()
            assert rel_err(outs[i], ref) < 0.0034, (group, i)
            if need == 0:
                assert torch.equal(outs[i], single[i]), (group, i)
            else:
                assert rel_err(outs[i], single[i]) < 0.00015 and (outs[i] != single[i]).float().mean() < 0.2, (group, i)
        # accumulate, through the C ABI, with and without the workspace (none: unsplit, the single accumulating product's bits)
        for with_ws in (True, False):
            for a, a0 in zip(acc, acc0):
                a.copy_(a0)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            sh = ops.backend().stream(ws)
            st = lib.tamd_gemm_group(ctypes.byref(pr), len(group), 3, ops.EPI_ACCUM, _cabi.TAMD_BF16,
                                     ws.data_ptr() if with_ws else None, need if with_ws else 0,
                                     ctypes.c_void_p(sh) if sh else None)
            assert st == 0, (group, st)
            for i, (m, n, k) in enumerate(group):
                want = acc0[i].clone()
                ops.raw_gemm(dys[i], xs[i], a_km=True, b_kn=True, epilogue=ops.EPI_ACCUM, out=want, sched="fl")
                if with_ws and need > 0:
                    assert rel_err(acc[i], want) < 0.00015, (group, i)
                else:
                    assert torch.equal(acc[i], want), (group, i)
    # the row-major layout (flags 0: C_p = A_p [M, K] . B_p [N, K]^T), split (one 2-tile + one 1-tile product over 32 stages) and
    # unsplit: the single products' bits when nothing is split
    for shapes in ([(264, 136, 2048), (128, 72, 2048)], [(264, 136, 128)]):
        a_s = [torch.randn(m, k).bfloat16().to(dev) for (m, n, k) in shapes]
        b_s = [(torch.randn(n, k) * 0.1).bfloat16().to(dev) for (m, n, k) in shapes]
        c_s = [torch.full((m, n), 3.0, dtype=torch.bfloat16, device=dev) for (m, n, k) in shapes]
        pr = (_cabi.GemmProblem * len(shapes))()
        for i, (m, n, k) in enumerate(shapes):
            pr[i] = _cabi.GemmProblem(a_s[i].data_ptr(), b_s[i].data_ptr(), c_s[i].data_ptr(), m, n, k, k, k, n)
        need = lib.tamd_gemm_group_workspace_bytes(ctypes.byref(pr), len(shapes), 0)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        sh = ops.backend().stream(ws)
        st = lib.tamd_gemm_group(ctypes.byref(pr), len(shapes), 0, ops.EPI_NONE, _cabi.TAMD_BF16, ws.data_ptr(), need,
                                 ctypes.c_void_p(sh) if sh else None)
        assert st == 0, (shapes, st)
        for i, (m, n, k) in enumerate(shapes):
            single = ops.raw_gemm(a_s[i], b_s[i], sched="fl")
            assert rel_err(c_s[i], a_s[i].float() @ b_s[i].float().t()) < 0.0034, (shapes, i)
            if need == 0:
                assert torch.equal(c_s[i], single), (shapes, i)
            else:
                assert rel_err(c_s[i], single) < 0.00015, (shapes, i)
    # argument checks: more than 4 products, mixed layouts, K % 64
    pr = (_cabi.GemmProblem * 1)()
    a = torch.randn(96, 64).bfloat16().to(dev)
    pr[0] = _cabi.GemmProblem(a.data_ptr(), a.data_ptr(), a.data_ptr(), 64, 64, 96, 64, 64, 64)
    assert lib.tamd_gemm_group(ctypes.byref(pr), 1, 3, ops.EPI_NONE, _cabi.TAMD_BF16, None, 0, None) != 0   # K % 64
    assert lib.tamd_gemm_group(ctypes.byref(pr), 5, 3, ops.EPI_NONE, _cabi.TAMD_BF16, None, 0, None) != 0
    assert lib.tamd_gemm_group(ctypes.byref(pr), 1, 1, ops.EPI_NONE, _cabi.TAMD_BF16, None, 0, None) != 0   # A_KM only


def test_gemm_segmented_weight_gradient(env):
    """tamd_gemm_seg (ABI 8): dW = dY^T . X of a fused q|k|v / gate|up projection with each member's rows stored into its own
    buffer -- the bits of the one-buffer product of the same entry point, with and without split-K."""
    torch.manual_seed(93)
    dev = env.device
    cases = ([(6144, 4096, 4096, (4096, 1024, 1024)), (1536, 768, 16384, (768, 768))] if env.big else
             [(768, 128, 320, (512, 256)), (1032, 136, 4096, (512, 256, 264))])
    for (m, n, k, rows) in cases:
        dy = torch.randn(k, m).bfloat16().to(dev)
        x = torch.randn(k, n).bfloat16().to(dev)
        # the one-buffer product through the SAME entry point and split-K policy (one segment).  (The default dispatch of
        # `raw_gemm` is no longer that: since round 5 it cuts a 1.5-round product into a whole-rounds part and a split-K
        # remainder -- gemm_dw_balanced -- whose unsplit part has another fp32 summation order: compared by value below.)
        whole = torch.full((m, n), 7.0, dtype=torch.bfloat16, device=dev)
        torch.ops.tamd.gemm_dw_segments(dy, x, [whole])
        segs = [torch.full((r, n), 7.0, dtype=torch.bfloat16, device=dev) for r in rows]
        torch.ops.tamd.gemm_dw_segments(dy, x, segs)
        assert torch.equal(torch.cat(segs, 0), whole), (m, n, k, rows)
        assert rel_err(whole, ops.raw_gemm(dy, x, a_km=True, b_kn=True)) < 2e-3, (m, n, k, rows)


@pytest.mark.gpu
def test_weight_gradient_products_cut_into_whole_rounds(env):
    """Round 5: dW of the Llama-3-8B q|k|v and down projections at 32768 tokens through the default dispatch (`torch.ops.tamd.gemm`
    -> gemm_dw_balanced: a whole-rounds part + a split-K remainder, written into row / column slices of one output) against
    the same product as ONE launch of the full-line kernel: same values up to the fp32 summation order of the split part."""
    if not env.big:
        pytest.skip("Llama-3-8B weight-gradient shapes: MI355X only")
    from transformers_amd import _native

    torch.manual_seed(5)
    dev = env.device
    t = 32768
    for m, n in ((6144, 4096), (4096, 14336)):
        axis, at = _native.dw_cut(m, n, t)
        assert axis >= 0
        dy = torch.randn(t, m, device=dev).bfloat16()
        x = torch.randn(t, n, device=dev).bfloat16()
        got = ops.raw_gemm(dy, x, a_km=True, b_kn=True)
        one = ops.raw_gemm(dy, x, a_km=True, b_kn=True, sched="fl")
        assert got.shape == one.shape == (m, n)
        main = (slice(0, at), slice(None)) if axis == 0 else (slice(None), slice(0, at))
        rest = (slice(at, None), slice(None)) if axis == 0 else (slice(None), slice(at, None))
        assert torch.equal(got[main], one[main])                   # the whole-rounds part: the same kernel, the same bits
        assert rel_err(got[rest], one[rest]) < 2e-3                 # the remainder: split-K (bf16 rounding of another fp32 order)
        ref = dy[:, :64].float().t() @ x.float()
        assert rel_err(got[:64], ref) < 0.0036
        del dy, x, got, one, ref

