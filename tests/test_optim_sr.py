"""Stochastic rounding of bf16 parameters (csrc/sround.h): `ops.sr_round_bf16`, `TamdAdamW(stochastic_rounding=True)`.

A bf16 weight of magnitude 0.02 has an ulp of 2^-13; an AdamW step at lr = 2e-5 is a sixth of it and round-to-nearest puts
the weight back where it was (test 5a).  Rounded up or down with probability equal to its position between the two bf16
neighbours, the stored value is right in expectation and the steps add up (test 5b).  The random bits are a counter-based hash
that the host evaluates too (`tamd_sr_bits`), so every kernel result here is restated bit for bit."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import transformers_amd
from transformers_amd import _cabi, build, ops

HYP = dict(lr=2e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
M64 = (1 << 64) - 1


def _bits(t):
    """bf16 tensor -> its 16-bit patterns (numpy uint16, flat)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)


def _host_sr(lib, x, key, step):
    """The rounding rule restated in numpy: (bits(x) + r16) >> 16 with r16 from the host's tamd_sr_bits; inf / NaN (exponent
    field 0xFF) as round-to-nearest: inf stays inf, NaN becomes the canonical quiet NaN of its sign here (which NaN a
    conversion returns differs between torch's CPU cast, the compiler's and the hardware's: the caller compares NaN positions
    as "is a NaN").  x: fp32 CPU tensor -> uint16 [n]."""
    flat = x.detach().cpu().contiguous().reshape(-1)
    u = flat.numpy().view(np.uint32).astype(np.uint64)
    r = np.fromiter((lib.tamd_sr_bits(key & M64, step, i) for i in range(u.size)), dtype=np.uint64, count=u.size)
    assert r.size == 0 or int(r.max()) <= 0xFFFF
    out = ((u + r) >> np.uint64(16)).astype(np.uint16)
    special = (u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    out[special] = (u[special] >> np.uint64(16)).astype(np.uint16) | np.where(u[special] & np.uint64(0x7FFFFF), 0x40, 0).astype(np.uint16)
    return out


def _f32_from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


# values 0-3: already bf16 (low 16 bits zero: must not move); 4-5: +-0; 6-7: +-inf; 8: NaN; 9: the last fp32 below the largest
# bf16's upper neighbour (rounds to inf with probability 65535/65536: the rule); 10-11: denormal / tiny
SPECIALS = _f32_from_bits([0x3F800000, 0xBCC00000, 0x3C010000, 0x7F7F0000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                           0x7FC00000, 0x7F7FFFFF, 0x00000001, 0x8000FFFF])


@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (8, 0), (37, 0), (65536, 0), (65537, 0), (4097, 1)])
def test_sr_round_bits_match_the_host_function(env, n, offset):
    """1: lengths below / at one 16-byte vector and ragged, one 64 Ki block and one element more (the index continues), and a
    view one element into its buffer (misaligned storage: one element per lane -- the bits belong to the element index, not
    to the address)."""
    lib = ops.backend().lib
    seed, step, ordinal = 0x1234_5678_9ABC_DEF, 3, 5
    g = torch.Generator().manual_seed(100 + n)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 4, (n,), generator=g).float())
    k = min(n, SPECIALS.numel()) if n >= 8 else 0
    x[:k] = SPECIALS[:k]
    buf = torch.zeros(n + offset)
    buf[offset:] = x
    xd = buf.to(env.device)[offset:]
    assert xd.is_contiguous() and (xd.data_ptr() % 16 != 0) == (offset != 0)
    y = ops.sr_round_bf16(xd, seed, step=step, ordinal=ordinal)
    assert y.dtype == torch.bfloat16 and y.shape == xd.shape
    key = ops.sr_key(seed, ordinal)
    want = _host_sr(lib, x, key, step)
    got = _bits(y)
    finite = ~np.isnan(x.numpy())
    assert np.array_equal(got[finite], want[finite]), np.flatnonzero(got != want)[:8]
    assert ((got[~finite] & 0x7FFF) > 0x7F80).all() and ((want[~finite] & 0x7FFF) > 0x7F80).all()  # NaN stays NaN
    u = x.numpy().view(np.uint32)
    exact = ((u & 0xFFFF) == 0) & finite
    assert np.array_equal(got[exact], (u[exact] >> 16).astype(np.uint16))  # bf16 values (+-0, +-inf among them) do not move
    # x and -x: the results negate each other
    neg = _bits(ops.sr_round_bf16(-xd, seed, step=step, ordinal=ordinal))
    assert np.array_equal(neg[finite], got[finite] ^ np.uint16(0x8000))
    # another step, another tensor: other bits
    if n >= 65536:
        assert not np.array_equal(_bits(ops.sr_round_bf16(xd, seed, step=step + 1, ordinal=ordinal)), got)
        assert not np.array_equal(_bits(ops.sr_round_bf16(xd, seed, step=step, ordinal=ordinal + 1)), got)


def test_sr_key_is_the_seed_mix(env):
    """ops.sr_key is attn_seed_mix(seed + ordinal) as a signed int64; the host function composes with it."""
    assert ops.sr_key(0, 0) == 0 and ops.sr_key(0, 1) == ops.sr_key(1, 0) != 0
    with np.errstate(over="ignore"):  # splitmix64's finaliser restated on uint64
        z = np.uint64(2 ** 63 - 1) + np.uint64(7)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    assert ops.sr_key(2 ** 63 - 1, 7) & M64 == int(z) and -(1 << 63) <= ops.sr_key(2 ** 63 - 1, 7) < (1 << 63)
    lib = ops.backend().lib
    assert {lib.tamd_sr_bits(1, 1, i) for i in range(64)} != {lib.tamd_sr_bits(1, 2, i) for i in range(64)}


def _up_mask(env, low16, n, step):
    x = _f32_from_bits([0x3F800000 + low16]).repeat(n).to(env.device)
    b = _bits(ops.sr_round_bf16(x, 99, step=step, ordinal=2))
    assert set(np.unique(b)) <= {0x3F80, 0x3F81}
    return b == 0x3F81


@pytest.mark.parametrize("low16", [0x4000, 0x8000, 1, 65535])
def test_sr_rounding_probability(env, low16):
    """2: x = 1 + (low16 / 65536) ulp rounds up with probability p = low16 / 65536: the fraction over n elements lies within
    six binomial standard deviations of p (low16 = 1 and 65535 catch an off-by-one in the carry).  The masks of two
    consecutive steps are independent: both round up in p^2 of the positions (identical masks would give p, and bias
    training); at p = 1/2 the two masks differ in half of all positions."""
    n = 65536 if env.big else 16384
    p = low16 / 65536.0
    a, b = _up_mask(env, low16, n, 10), _up_mask(env, low16, n, 11)
    for m in (a, b):
        assert abs(m.mean() - p) <= 6.0 * math.sqrt(p * (1 - p) / n), (m.mean(), p)
    both = p * p
    assert abs((a & b).mean() - both) <= 6.0 * math.sqrt(both * (1 - both) / n), ((a & b).mean(), both)
    if low16 in (0x4000, 0x8000):
        differ = 2 * p * (1 - p)  # 0.375 of all positions at p = 1/4, one half at p = 1/2
        assert abs((a ^ b).mean() - differ) <= 6.0 * math.sqrt(differ * (1 - differ) / n)
        assert not np.array_equal(a, b)


def _sr_twin_step(env, shapes, grads, seed, fp32_moments=True, misaligned=(), **kw):
    """One step of the stochastic-rounding optimizer on bf16 parameters, and one step of the plain optimizer on fp32 copies
    with the same gradients upcast, its result rounded by ops.sr_round_bf16 with (seed, step 1, ordinal k).  With bf16
    moments (first step only: they start at zero, so both runs evaluate the same fp32 expression) each moment is the fp32
    twin's rounded to nearest.  `misaligned`: positions in `shapes` of parameters stored one element into their buffer."""
    g0 = torch.Generator().manual_seed(21)
    host = [torch.randn(s, generator=g0).bfloat16() for s in shapes]
    ps = [torch.nn.Parameter(torch.cat([t.new_zeros(1), t]).to(env.device)[1:] if k in misaligned else t.to(env.device))
          for k, t in enumerate(host)]
    assert all((p.data_ptr() % 16 == 2) == (k in misaligned) and p.is_contiguous() for k, p in enumerate(ps))
    p32 = [torch.nn.Parameter(p.detach().float().clone()) for p in ps]
    opt = transformers_amd.TamdAdamW(ps, stochastic_rounding=True, fp32_moments=fp32_moments, sr_seed=seed, **HYP, **kw)
    ref = transformers_amd.TamdAdamW(p32, **HYP, **kw)
    for p, q, g in zip(ps, p32, grads):
        p.grad = g.bfloat16().to(env.device)
        q.grad = p.grad.float()
    opt.step()
    ref.step()
    for k, (p, q) in enumerate(zip(ps, p32)):
        want = ops.sr_round_bf16(q.detach(), seed, step=1, ordinal=k)
        assert p.shape == q.shape and np.array_equal(_bits(p), _bits(want)), (k, tuple(p.shape))
        for name in ("exp_avg", "exp_avg_sq"):
            got, twin = opt.state[p][name], ref.state[q][name]
            assert got.dtype == (torch.float32 if fp32_moments else torch.bfloat16) and twin.dtype == torch.float32
            assert torch.equal(got, twin.to(got.dtype)), (k, name)
    return opt, ref, ps, p32


def test_sr_optimizer_kernel_is_the_fp32_kernel_plus_rounding(env):
    """3: both launches evaluate the same fp32 expression on the same inputs; the only difference is how the parameter is
    stored.  A 0-dim parameter, ragged tails, a multiple of the vector and a tensor of two chunks."""
    shapes = [(), (3,), (37,), (5, 13), (256, 64), (65537,)]
    g1 = torch.Generator().manual_seed(22)
    grads = [torch.randn(s, generator=g1) * 0.3 for s in shapes]
    opt, _, ps, p32 = _sr_twin_step(env, shapes, grads, seed=0x5EED)
    assert len(opt._tables) == 1
    tab = next(iter(opt._tables.values()))
    assert tab.table.numel() == 7 * len(shapes) + 1  # the key column after the plain table's words
    assert tab.table[6 * len(shapes) + 1:].tolist() == [ops.sr_key(0x5EED, k) for k in range(len(shapes))]
    # and the rounding does something: a sizeable part of the big tensor differs from round-to-nearest, by one ulp
    rn, sr = _bits(p32[-1].detach().bfloat16()).astype(np.int32), _bits(ps[-1]).astype(np.int32)
    assert 0.15 < (rn != sr).mean() < 0.35 and np.abs(rn - sr).max() == 1


def test_sr_optimizer_kernel_with_bf16_moments_is_the_fp32_kernel_plus_rounding(env):
    """3b: the same statement for bf16 moments -- eight elements per lane and a 16-byte parameter store, where test 3 (fp32
    moments) has four and eight bytes.  The shapes of test 3 and a parameter whose storage is not 16-byte aligned (one
    element per lane from start to end)."""
    shapes = [(), (3,), (37,), (5, 13), (256, 64), (65537,), (2049,)]
    g1 = torch.Generator().manual_seed(23)
    grads = [torch.randn(s, generator=g1) * 0.3 for s in shapes]
    opt, _, ps, p32 = _sr_twin_step(env, shapes, grads, seed=0xB16, fp32_moments=False, misaligned={len(shapes) - 1})
    assert len(opt._tables) == 1
    rn, sr = _bits(p32[-2].detach().bfloat16()).astype(np.int32), _bits(ps[-2]).astype(np.int32)
    assert 0.15 < (rn != sr).mean() < 0.35 and np.abs(rn - sr).max() == 1


def test_sr_bits_follow_the_parameter_not_the_table_slot(env):
    """4: [a, b, c]; at step 2 b has no gradient in one run and has one in the other.  c moves one slot up in the table of
    the first run: its bits (and a's) must not change -- the ordinal keys them."""
    results = []
    for b_has_grad in (False, True):
        g0 = torch.Generator().manual_seed(31)
        ps = [torch.nn.Parameter(torch.randn(s, generator=g0).bfloat16().to(env.device)) for s in [(40,), (24,), (300,)]]
        opt = transformers_amd.TamdAdamW(ps, stochastic_rounding=True, sr_seed=77, **HYP)
        for step in (1, 2):
            for i, p in enumerate(ps):
                p.grad = (torch.randn(p.shape, generator=g0) * 0.3).bfloat16().to(env.device)
                if step == 2 and i == 1 and not b_has_grad:
                    p.grad = None
            opt.step()
        results.append([_bits(p) for p in ps])
    (a0, b0, c0), (a1, b1, c1) = results
    assert np.array_equal(a0, a1) and np.array_equal(c0, c1)
    assert not np.array_equal(b0, b1)


def _small_step_setup(env):
    n, steps = (8192, 64) if env.big else (2048, 32)
    g0 = torch.Generator().manual_seed(41)
    p0 = (0.018 + 0.010 * torch.rand(n, generator=g0)).bfloat16()  # inside [2^-6, 2^-5) from start to end: one ulp = 2^-13
    assert float(p0.min()) - steps * 2e-5 > 2.0 ** -6 and float(p0.max()) < 2.0 ** -5
    return n, steps, p0


def test_small_steps_freeze_bf16_parameters_rounded_to_nearest(env):
    """5a, the control: lr = 2e-5 is 0.16 ulp of these weights -- after N round-to-nearest steps with a constant gradient
    the parameter is where it started, bit for bit."""
    n, steps, p0 = _small_step_setup(env)
    w = torch.nn.Parameter(p0.clone().to(env.device))
    opt = transformers_amd.TamdAdamW([w], lr=2e-5, weight_decay=0.0)
    for _ in range(steps):
        w.grad = torch.ones(n).bfloat16().to(env.device)
        opt.step()
    assert np.array_equal(_bits(w), _bits(p0))
    assert next(iter(opt._tables.values())).table.numel() == 6 + 1  # the plain table, as before


def test_small_steps_drift_correctly_with_stochastic_rounding(env):
    """5b: the same run with stochastic rounding moves the parameters, on average, as far as torch.optim.AdamW moves an fp32
    copy.  Binomial model: every step rounds an element one ulp down with probability q = lr / ulp (the update of a constant
    gradient is lr), so the displacement of one element after N steps has variance N q (1 - q) ulp^2 and the mean over n
    elements the standard error sqrt(N q (1 - q) / n) ulp -- 0.3 % of the displacement at the GPU sizes, 1 % on the CPU
    model.  Gate: six standard errors."""
    n, steps, p0 = _small_step_setup(env)
    lr, ulp = 2e-5, 2.0 ** -13
    w = torch.nn.Parameter(p0.clone().to(env.device))
    opt = transformers_amd.TamdAdamW([w], lr=lr, weight_decay=0.0, stochastic_rounding=True, sr_seed=4242)
    r = torch.nn.Parameter(p0.float())
    ref = torch.optim.AdamW([r], lr=lr, weight_decay=0.0, foreach=False)
    for _ in range(steps):
        w.grad = torch.ones(n).bfloat16().to(env.device)
        r.grad = torch.ones(n)
        opt.step()
        ref.step()
    want = (p0.double() - r.detach().double()).mean().item()
    got = (p0.double() - w.detach().cpu().double()).mean().item()
    q = lr / ulp
    se = math.sqrt(steps * q * (1 - q) / n) * ulp
    print(f"displacement: stochastic rounding {got:.6e}, fp32 AdamW {want:.6e}, standard error {se:.3e} "
          f"({(got - want) / se:+.2f} se)")
    assert abs(want - steps * lr) < 1e-3 * steps * lr
    assert se < 0.012 * want
    assert abs(got - want) <= 6.0 * se, (got, want, se)


def _run(env, p0s, seed, steps, grads, resume_at=None):
    ps = [torch.nn.Parameter(p.clone().to(env.device)) for p in p0s]
    opt = transformers_amd.TamdAdamW(ps, stochastic_rounding=True, sr_seed=seed, **HYP)
    for t in range(steps):
        if resume_at is not None and t == resume_at:
            sd = copy.deepcopy(opt.state_dict())
            ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
            opt = transformers_amd.TamdAdamW(ps, stochastic_rounding=True, sr_seed=seed + 1000, **HYP)  # (the checkpoint's wins)
            opt.load_state_dict(sd)
        for p, g in zip(ps, grads[t]):
            p.grad = g.clone().to(env.device)
        opt.step()
    return opt, [_bits(p) for p in ps]


def test_sr_is_reproducible_and_resumes(env):
    """6: same seed, same bits; another seed, other bits; a run resumed from state_dict() continues with the same bits."""
    g0 = torch.Generator().manual_seed(51)
    p0s = [torch.randn(s, generator=g0).bfloat16() for s in [(300,), (17, 5)]]
    grads = [[(torch.randn(p.shape, generator=g0) * 0.3).bfloat16() for p in p0s] for _ in range(4)]
    opt, a = _run(env, p0s, 9, 4, grads)
    _, b = _run(env, p0s, 9, 4, grads)
    _, c = _run(env, p0s, 10, 4, grads)
    opt_r, d = _run(env, p0s, 9, 4, grads, resume_at=2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not any(np.array_equal(x, y) for x, y in zip(a, c))
    assert all(np.array_equal(x, y) for x, y in zip(a, d))
    group = opt.state_dict()["param_groups"][0]
    assert group["stochastic_rounding"] is True and group["sr_seed"] == 9
    assert opt_r.param_groups[0]["sr_seed"] == 9


def test_sr_defaults_seed_and_foreign_checkpoints(env):
    """6: `sr_seed=None` reads torch's initial seed (no draw from the generator: model initialisation is undisturbed, every
    DDP rank gets the same seed after set_seed); a checkpoint without the two entries -- torch.optim.AdamW's -- loads and
    falls back to the optimizer's defaults."""
    torch.manual_seed(7)
    state = torch.get_rng_state()
    w1 = torch.nn.Parameter(torch.zeros(8).bfloat16().to(env.device))
    o1 = transformers_amd.TamdAdamW([w1], stochastic_rounding=True)
    assert torch.equal(torch.get_rng_state(), state)
    torch.randn(3)
    o2 = transformers_amd.TamdAdamW([torch.nn.Parameter(torch.zeros(8))], stochastic_rounding=True)
    assert o1.param_groups[0]["sr_seed"] == o2.param_groups[0]["sr_seed"] == 7
    off = transformers_amd.TamdAdamW([torch.nn.Parameter(torch.zeros(8))])
    assert off.param_groups[0]["stochastic_rounding"] is False and "sr_seed" in off.state_dict()["param_groups"][0]

    r = torch.nn.Parameter(torch.randn(8))
    ref = torch.optim.AdamW([r], foreach=False, **HYP)
    r.grad = torch.randn(8)
    ref.step()
    sd = copy.deepcopy(ref.state_dict())
    assert "stochastic_rounding" not in sd["param_groups"][0]
    with torch.no_grad():
        w1.copy_(r.detach().bfloat16())
    o3 = transformers_amd.TamdAdamW([w1], stochastic_rounding=True, sr_seed=5, **HYP)
    o3.load_state_dict(sd)
    g = o3.param_groups[0]
    assert g["stochastic_rounding"] is True and g["sr_seed"] == 5 and g["fp32_moments"] is False
    w1.grad = torch.randn(8).bfloat16().to(env.device)
    o3.step()
    assert float(o3.state[w1]["step"]) == 2.0 and bool(torch.isfinite(w1.detach().float()).all())


def test_sr_refusals_do_not_launch():
    """7 (no GPU): fp16 parameters are refused at the first step(); the C entry points check their arguments before any
    launch."""
    w = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    opt = transformers_amd.TamdAdamW([w], stochastic_rounding=True)
    w.grad = torch.ones(8, dtype=torch.float16)
    with pytest.raises(ValueError, match="fp16"):
        opt.step()
    assert len(opt.state[w]) == 0 and float(w.detach().abs().max()) == 0.0

    lib = _cabi.TamdLib(build.build())
    hyp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.tamd_mt_adamw_step_sr(None, 1, 1, *hyp, 1, 1.0, None, _cabi.TAMD_BF16, None) == -4  # NULL table
    words = (ctypes.c_int64 * 8)()
    table = ctypes.cast(words, ctypes.c_void_p)
    assert lib.tamd_mt_adamw_step_sr(table, 1, 1, *hyp, 0, 1.0, None, _cabi.TAMD_BF16, None) == -6  # step < 1
    assert lib.tamd_mt_adamw_step_sr(table, 1, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, 1, 1.0, None, _cabi.TAMD_F32, None) == -6
    assert lib.tamd_mt_adamw_step_sr(table, 1, 1 << 31, *hyp, 1, 1.0, None, _cabi.TAMD_BF16, None) == -6
    assert lib.tamd_mt_adamw_step_sr(table, 1, 1, *hyp, 1, 1.0, None, _cabi.TAMD_F16, None) == -1  # moments: bf16 / fp32
    assert lib.tamd_mt_adamw_step_sr(table, 0, 0, *hyp, 1, 1.0, None, _cabi.TAMD_BF16, None) == 0  # nothing to do
    assert lib.tamd_sr_round(None, None, 8, 1, 1, None) == -4
    assert lib.tamd_sr_round(table, table, -1, 1, 1, None) == -6
    assert lib.tamd_sr_round(None, None, 0, 1, 1, None) == 0
    # the host function needs no device
    assert all(0 <= lib.tamd_sr_bits(3, 1, i) <= 0xFFFF for i in range(16))
    far = 1 << 40  # the index is 64 bits wide: its high word reaches the hash
    assert [lib.tamd_sr_bits(3, 1, i) for i in range(16)] != [lib.tamd_sr_bits(3, 1, far + i) for i in range(16)]


def test_sr_combines_with_gradient_clipping(env):
    """8: max_grad_norm with the flag on == the clipped fp32 run + sr_round_bf16.  The gradients are dyadic (+-1/4 .. +-2), so
    their sum of squares is exact in fp32 whatever the order -- the norm kernels of the two dtypes read vectors of different
    widths -- and both runs apply the same coefficient."""
    shapes = [(37,), (256, 64)]
    g1 = torch.Generator().manual_seed(61)
    grads = [torch.exp2(torch.randint(-2, 2, s, generator=g1).float()) * (torch.randint(0, 2, s, generator=g1) * 2 - 1)
             for s in shapes]
    opt, ref, _, _ = _sr_twin_step(env, shapes, grads, seed=0xC11F, max_grad_norm=1.0)
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    assert norm > 50.0  # clipped for real
    assert float(opt.grad_norm) == float(ref.grad_norm) and abs(float(opt.grad_norm) - norm) <= 1e-6 * norm


def test_sr_ops_are_registered_for_the_dispatcher():
    m = torch.device("meta")
    for name in ("sr_round_bf16", "mt_adamw_step_sr_"):
        op = getattr(torch.ops.tamd, name).default
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "Meta"), name
    y = torch.ops.tamd.sr_round_bf16(torch.empty(3, 5, device=m), 1, 0)
    assert y.shape == (3, 5) and y.dtype == torch.bfloat16
