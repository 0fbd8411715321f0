"""The sigmoid, group-limited replacement routers (transformers_amd/models/moe.py: GROUPED) inside tiny models, under the CPU
execution model (`emu`) and on the MI355X (`hip`): two layers, hidden 128, 2 x 32 tokens, bf16, `experts_implementation="tamd"`,
`attn_implementation="eager"` (MLA attention stays the reference's).

    DeepSeek-V3  E = 16 in 4 groups, 2 groups chosen, top-4, scale 2.5, norm_topk_prob, one shared expert
    GLM-4-MoE    E = 24, one group, top-4, norm_topk_prob true and false

`e_score_correction_bias` holds small nonzero values in a random order (bf16-exact, so the buffer can be carried in bf16 -- what
`model.bfloat16()` leaves -- or restored to fp32 -- what `from_pretrained` keeps -- with the same numbers).

A forward hook on every router captures its input and its triple.  Per call: dtypes and shapes are those of the reference
class's own forward on the same module and input; indices match as SETS (the reference's topk(sorted=False) leaves the order
open); weights match by id against the float64 chain of include/tamd.h on the captured fp32 logits, within MULT(k) 2^-23
(tests/test_moe_router_group.py derives MULT).

A/B: the same model accelerated with `moe_router=False` -- both on the kernels, differing in the router alone.  The two gate
products sum in different orders, so the test asserts first, as a condition on the inputs -- on the reference arm's captured
logits, every row, for the model of the first seed of 0 .. 31 whose reference run on the CPU meets it -- that the group-score gap
at the topk_group boundary and every gap among the k + 1 largest eligible c are at least

    4 x 2 H 2^-24 max_e sum_h |x_h w_eh| / 4

per row: the fp32 bound of a reordered sum of H exact products, through the sigmoid (s' <= 1 / 4), doubled for two arms, times 4.
Freshly initialised routers do not meet it; `separate()` gives the routers separated logits by construction.  Then the index
sets must be identical and every quantity q (logits, loss, each parameter gradient, the gates' included; neither model family offers `output_router_logits`) agrees within

    gate(q) = 4 x max(AB_MEASURED, one bf16 flip in q)        (tests/test_moe_router_models.py: ab_gate)

Measured between the arms (profiles/moe_router_group_tests.md), both backends: logits and loss 0 -- the reference emits its
pairs in another order than ours (c descending) and tamd_moe_combine sums j ascending, yet no bf16 rounding flipped at these
sizes -- so AB_MEASURED_FWD = 0 and the flip floor gates them.  Parameter gradients: up to AB_MEASURED_GRAD = 4.4e-3
norm-relative (gate weights 1.3e-3 .. 2.9e-3, and everything upstream of a router alike).  That is the ONE rounding of dlogits
to bf16 in front of the gate's two backward products, which the reference arm runs in fp32 (include/tamd.h
tamd_moe_router_group_bwd; each dlogit moves by up to 2^-9 relative, and the terms of a sum over 64 tokens cancel);
tests/test_moe_router_group.py::test_gate_op_backward holds it to its per-element bound.
"""
import copy
import inspect

import pytest
import torch

import transformers_amd
from conftest import record, rel_err
from kernel_checks import BF16, F32
from test_moe_router_group import MULT, NEG, TINY, U23, eligible64, scores64, weights64
from test_moe_router_models import Tap, ab_gate as _ab_gate, inputs, routers
from transformers import DeepseekV3Config, DeepseekV3ForCausalLM, Glm4MoeConfig, Glm4MoeForCausalLM
from transformers.models.deepseek_v3.modeling_deepseek_v3 import DeepseekV3TopkRouter
from transformers_amd import experts
from transformers_amd.models import moe

B, S, LAYERS, H = 2, 32, 2, 128
AB_MEASURED_FWD = 0.0      # logits and loss: the largest A/B difference measured, both backends (module docstring)
AB_MEASURED_GRAD = 4.4e-3  # parameter gradients: likewise (4.34e-3 under the CPU model, 4.17e-3 on the MI355X)


def ab_gate(numel, scalar_of=None, measured=AB_MEASURED_FWD):
    return max(_ab_gate(numel, scalar_of), 4.0 * measured)


def grad_gate(numel):
    return ab_gate(numel, measured=AB_MEASURED_GRAD)


COMMON = dict(vocab_size=512, hidden_size=H, intermediate_size=128, moe_intermediate_size=64, num_hidden_layers=LAYERS,
              num_attention_heads=2, n_shared_experts=1, num_experts_per_tok=4, first_k_dense_replace=0, max_position_embeddings=256,
              attn_implementation="eager", experts_implementation="eager")


def make(family, seed=0):
    """-> (model in bf16 on the CPU, (E, n_group, topk_group, k))"""
    torch.manual_seed(seed)
    if family == "deepseek_v3":
        cfg = DeepseekV3Config(num_key_value_heads=2, n_routed_experts=16, n_group=4, topk_group=2, routed_scaling_factor=2.5,
                               norm_topk_prob=True, q_lora_rank=32, kv_lora_rank=32, qk_rope_head_dim=16, qk_nope_head_dim=16,
                               v_head_dim=32, **COMMON)
        model, geom = DeepseekV3ForCausalLM(cfg).bfloat16(), (16, 4, 2, 4)
    else:
        cfg = Glm4MoeConfig(num_key_value_heads=1, head_dim=64, n_routed_experts=24, n_group=1, topk_group=1, routed_scaling_factor=1.0,
                            norm_topk_prob=family.endswith("norm"), **COMMON)
        model, geom = Glm4MoeForCausalLM(cfg).bfloat16(), (24, 1, 1, 4)
    g = torch.Generator().manual_seed(900 + seed)
    for r in routers(model):
        # small, nonzero, exact in bf16, and -- like the logits -- apart from each other by construction: odd multiples of 2^-9
        # in a random order, |b| < 0.05
        b = ((torch.randperm(geom[0], generator=g).float() - geom[0] / 2 + 0.5) * 2.0 ** -8).bfloat16()
        r.e_score_correction_bias = b  # (a registered buffer: assignment keeps it one; bf16, as `.bfloat16()` leaves it)
    return model, geom


FAMILIES = ["deepseek_v3", "glm4_norm", "glm4_raw"]


def separate(model, E, seed):
    """Gate weights a_e * u (tests/test_moe_router_models.py: separate), a_e = (perm(e) - (E - 1) / 2) * 4 / E: every row's
    logits are a_e (u . x), over about [-5, 5], so the sigmoids keep their distance and do not saturate; the bias moves some
    choices.  u has four nonzero entries of +-1/2 (a unit vector): the margin the condition asks for grows with
    sum_h |x_h w_eh|, which a dense u makes seven times |u . x| -- too many of the 128 rows then sit inside it for any seed."""
    g = torch.Generator().manual_seed(100 + seed)
    for r in routers(model):
        u = torch.zeros(r.weight.shape[1])
        u[torch.randperm(r.weight.shape[1], generator=g)[:4]] = (torch.randint(0, 2, (4,), generator=g).float() - 0.5)
        a = (torch.randperm(E, generator=g).float() - (E - 1) / 2) * (4.0 / E)
        with torch.no_grad():
            r.weight.copy_((a[:, None] * u[None, :]).to(r.weight.dtype))


def margins_ok(calls, geom, factor=1.0):
    """the condition of the module docstring, on every row of every captured call (`factor`: that many times the margin)"""
    E, ng, tg, k = geom
    for mod, x, (logits, _w, _i) in calls:
        x64 = x.reshape(-1, H).double().cpu()
        need = factor * 4 * 2 * H * 2.0 ** -24 * 0.25 * (x64.abs() @ mod.weight.detach().double().cpu().abs().t()).max(-1).values
        s, c = scores64(logits.double().cpu(), mod.e_score_correction_bias.detach().double().cpu())
        elig, gs = eligible64(c, ng, tg)
        if gs is not None and tg < ng:
            g = torch.sort(gs, dim=-1, descending=True).values
            if not bool(((g[:, tg - 1] - g[:, tg]) >= need).all()):
                return False
        top = torch.sort(torch.where(elig, c, torch.full_like(c, NEG)), dim=-1, descending=True).values[:, :k + 1]
        if not bool(((top[:, :-1] - top[:, 1:]) >= need[:, None]).all()):
            return False
    return True


_CHOSEN = {}


def chosen(family):
    """The model of the first seed of 0 .. 31 whose reference run (bf16, eager, on the CPU) meets `margins_ok` with twice the
    margin in every layer (the arms' activations differ from that run's by bf16 roundings; the test then asserts the margin
    itself on the reference arm's own logits): a property of the inputs alone; computed once per session, shared, never modified."""
    if family not in _CHOSEN:
        ids, _ = inputs()
        for seed in range(32):
            base, geom = make(family, seed)
            separate(base, geom[0], seed)
            tap = Tap(base)
            with torch.no_grad():
                base(input_ids=ids, use_cache=False)
            if margins_ok(tap.close().calls, geom, factor=2.0):
                _CHOSEN[family] = (base, geom)
                break
        else:
            raise AssertionError("no seed of 0 .. 31 meets the margin condition")
    return _CHOSEN[family]


def accel(model, **kw):
    """`accelerate` with the attention left as built ("eager"): MLA's head sizes are not the attention kernels'"""
    return transformers_amd.accelerate(model, attn_implementation=False, **kw)


def run(model, ids, labels, **kw):
    model.zero_grad()
    tap = Tap(model)
    out = model(input_ids=ids, labels=labels, use_cache=False, **kw)
    out.loss.backward()
    return out, tap.close()


def sets(i):
    return i.cpu().sort(-1).values


# ---------------------------------------------------------------------------------------------------- the table
def test_every_class_of_the_table_has_the_reference_forward():
    """models/moe.py replaces a class only because its forward IS DeepseekV3TopkRouter.forward: an upgrade of the reference that
    changes one of them fails here."""
    ref = inspect.getsource(DeepseekV3TopkRouter.forward)
    names = {c.__name__ for c in moe.GROUPED_REPLACEMENTS}
    assert {"DeepseekV3TopkRouter", "Glm4MoeTopkRouter"} <= names
    assert names <= {n for _f, n in moe.GROUPED}
    for cls, repl in moe.GROUPED_REPLACEMENTS.items():
        assert inspect.getsource(cls.forward) == ref, cls.__name__
        assert issubclass(repl, cls) and moe.REPLACEMENTS[cls] is repl
    from transformers.models.minimax_m2.modeling_minimax_m2 import MiniMaxM2TopKRouter

    assert MiniMaxM2TopKRouter not in moe.REPLACEMENTS and inspect.getsource(MiniMaxM2TopKRouter.forward) != ref


# ---------------------------------------------------------------------------------------------------- inside the models
@pytest.mark.parametrize("bias", ["bias_bf16", "bias_fp32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_router_inside_the_model(env, family, bias):
    dev = env.device
    base, geom = chosen(family)
    E, ng, tg, k = geom
    base = copy.deepcopy(base)
    if bias == "bias_fp32":
        for r in routers(base):
            r.e_score_correction_bias = r.e_score_correction_bias.float()
    ids, labels = (t.to(dev) for t in inputs())
    fast = accel(copy.deepcopy(base).train().to(dev))
    arm = accel(copy.deepcopy(base).train().to(dev), moe_router=False)
    assert len(routers(fast)) == LAYERS and all(type(r) in moe.GROUPED_REPLACEMENTS.values() for r in routers(fast))
    assert all(type(r) in moe.GROUPED_REPLACEMENTS for r in routers(arm))
    want_bias = F32 if bias == "bias_fp32" else BF16
    assert all(r.e_score_correction_bias.dtype == want_bias for r in routers(fast))
    # ---- the reference arm first: the condition on the inputs
    o_arm, t_arm = run(arm, ids, labels)
    assert margins_ok(t_arm.calls, geom), family
    # ---- ours
    transformers_amd.fallback_calls(reset=True)
    experts.router_call_count(reset=True)
    o, tap = run(fast, ids, labels)
    assert experts.router_call_count() == LAYERS
    assert not any("Router" in key for key in transformers_amd.fallback_calls()), transformers_amd.fallback_calls()
    assert len(tap.calls) == len(t_arm.calls) == LAYERS
    moved = False  # the bias changes some choices
    for layer, ((mod, x, (logits, weights, index)), (_m, _x, (l_arm, w_arm, i_arm))) in enumerate(zip(tap.calls, t_arm.calls)):
        ref_cls = type(mod).__mro__[1]
        assert ref_cls in moe.GROUPED_REPLACEMENTS
        with torch.no_grad():
            want = ref_cls.forward(mod, x)  # the reference class's own forward on the same module and input
        for got_t, want_t in zip((logits, weights, index), want):
            assert got_t.dtype == want_t.dtype and got_t.shape == want_t.shape, (family, layer, got_t.dtype, want_t.dtype)
        assert logits.shape == (B * S, E) and logits.dtype == F32 and index.shape == (B * S, k)
        assert torch.equal(sets(index), sets(want[2])), (family, layer, "index sets against the reference's forward")
        l64 = logits.double().cpu()
        s, c = scores64(l64, mod.e_score_correction_bias.detach().double().cpu())
        elig, _ = eligible64(c, ng, tg)
        idx64 = torch.sort(torch.where(elig, c, torch.full_like(c, NEG)), dim=-1, descending=True, stable=True).indices[:, :k]
        assert torch.equal(sets(index), sets(idx64)), (family, layer)  # every row
        _, c0 = scores64(l64, torch.zeros(E, dtype=torch.float64))
        e0, _ = eligible64(c0, ng, tg)
        idx0 = torch.sort(torch.where(e0, c0, torch.full_like(c0, NEG)), dim=-1, descending=True, stable=True).indices[:, :k]
        moved = moved or not torch.equal(sets(idx0), sets(idx64))
        w64 = weights64(s, index.cpu(), bool(mod.norm_topk_prob), float(mod.routed_scaling_factor))  # by id
        err = (weights.double().cpu() - w64).abs()
        record("moe_router_group_models", f"{env.name} {family} {bias} layer {layer} weights rel err / 2^-23",
               (err / w64.clamp_min(TINY)).max().item() / U23, MULT(k))
        assert bool((err <= MULT(k) * U23 * w64 + TINY).all()), (family, layer, (err / w64).max().item())
        assert torch.equal(sets(index), sets(i_arm)), (family, layer, "the two arms route alike")
    assert moved, "the bias of the test model changes no choice"
    # ---- A/B: logits, loss, every parameter gradient
    d = rel_err(o.logits, o_arm.logits)
    record("moe_router_group_models", f"{env.name} {family} {bias} logits vs moe_router=False", d, ab_gate(o.logits.numel()))
    print(f"{env.name} {family} {bias}: logits A/B {float(d):.3e} (gate {ab_gate(o.logits.numel()):.3e})")
    assert d <= ab_gate(o.logits.numel()), (family, float(d))
    dl = abs(o.loss.item() - o_arm.loss.item()) / abs(o_arm.loss.item())
    record("moe_router_group_models", f"{env.name} {family} {bias} loss vs moe_router=False", dl, ab_gate(1, scalar_of=B * S))
    print(f"{env.name} {family} {bias}: loss A/B {dl:.3e} (gate {ab_gate(1, scalar_of=B * S):.3e})")
    assert dl <= ab_gate(1, scalar_of=B * S), (family, dl)
    g_arm = dict(arm.named_parameters())
    worst, worst_ratio, seen_gate = 0.0, 0.0, False
    fails = []
    for n, p in fast.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        dg = float(rel_err(p.grad, g_arm[n].grad))
        worst, worst_ratio = max(worst, dg), max(worst_ratio, dg / grad_gate(p.numel()))
        if n.endswith("mlp.gate.weight"):
            seen_gate = True
            record("moe_router_group_models", f"{env.name} {family} {bias} {n} gradient vs moe_router=False", dg, grad_gate(p.numel()))
            print(f"{env.name} {family} {bias}: {n} gradient A/B {dg:.3e} (gate {grad_gate(p.numel()):.3e})")
        if not dg <= grad_gate(p.numel()):
            fails.append((n, dg, grad_gate(p.numel())))
    print(f"{env.name} {family} {bias}: worst gradient A/B {worst:.3e}, worst share of its gate {worst_ratio:.3f}")
    record("moe_router_group_models", f"{env.name} {family} {bias} worst gradient vs moe_router=False / its gate", worst_ratio, 1.0)
    assert seen_gate and not fails, (family, fails)
    # ---- revert
    transformers_amd.revert(fast)
    assert all(type(r) in moe.GROUPED_REPLACEMENTS for r in routers(fast))
    assert not any("_tamd_fp32_bias" in m.__dict__ for m in fast.modules())  # the converted bias does not outlive revert


def test_generate_runs_every_step_through_the_router(env):
    dev = env.device
    base, geom = chosen("deepseek_v3")
    fast = accel(copy.deepcopy(base).eval().to(dev))
    arm = accel(copy.deepcopy(base).eval().to(dev), moe_router=False)
    ids, _ = inputs()
    prompt = ids[:, :12].to(dev)
    steps = 8
    kw = dict(max_new_tokens=steps, min_new_tokens=steps, do_sample=False, pad_token_id=0)
    experts.router_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        out = fast.generate(prompt, **kw)
    assert out.shape == (B, 12 + steps)
    assert experts.router_call_count() == LAYERS * steps, experts.router_call_count()  # the prefill (24 tokens) and every decode step (2)
    assert not any("Router" in key for key in transformers_amd.fallback_calls()), transformers_amd.fallback_calls()
    with torch.no_grad():
        want = arm.generate(prompt, **kw)
    assert torch.equal(out.cpu(), want.cpu())


# ---------------------------------------------------------------------------------------------------- refusals
def _router(E=16, ng=4, tg=2, k=4, hidden=H, dtype=BF16, seed=3):
    """one replacement router with random weights and bias, on the CPU"""
    cfg = DeepseekV3Config(**dict(COMMON, hidden_size=hidden, num_experts_per_tok=k), num_key_value_heads=2, n_routed_experts=E,
                           n_group=ng, topk_group=tg, routed_scaling_factor=2.5, norm_topk_prob=True)
    r = DeepseekV3TopkRouter(cfg)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        r.weight.copy_(torch.randn(E, hidden, generator=g) * 0.1)
    r.e_score_correction_bias = (torch.rand(E, generator=g) - 0.5) * 0.1
    r = r.to(dtype)
    r.__class__ = moe.GROUPED_REPLACEMENTS[DeepseekV3TopkRouter]
    return r


def test_refusals_are_counted(env):
    """What the kernels do not take is not approximated: the reference's forward runs, returns its result, and is counted."""
    dev = env.device
    g = torch.Generator().manual_seed(9)
    name = "TamdDeepseekV3TopkRouter"
    cases = [("dtype", _router(dtype=F32), F32, H),               # an fp32 module
             ("dtype", _router().float(), BF16, H),               # a gate kept in fp32 under bf16 activations
             ("experts", _router(E=384, ng=8, tg=4, k=8), BF16, H),   # Kimi-K2's expert count
             ("experts", _router(E=12, ng=1, tg=1, k=4), BF16, H),    # E % 8
             ("top_k", _router(E=64, ng=1, tg=1, k=17), BF16, H),
             ("groups", _router(E=16, ng=16, tg=4, k=4), BF16, H),    # groups of one expert (the reference's topk(2) raises)
             ("shape", _router(hidden=96), BF16, 96)]                 # H % 64
    for why, r, xdt, hidden in cases:
        x = torch.randn(5, hidden, generator=g).to(xdt)
        r = r.to(dev)
        experts.router_call_count(reset=True)
        transformers_amd.fallback_calls(reset=True)
        ref = copy.deepcopy(r).cpu()
        ref.__class__ = DeepseekV3TopkRouter
        with torch.no_grad():
            try:
                want = ref(x)
            except RuntimeError:
                want = None  # (groups of one: the reference itself raises)
            if want is None:
                with pytest.raises(RuntimeError):
                    r(x.to(dev))
            else:
                got = r(x.to(dev))
                assert torch.equal(sets(got[2]), sets(want[2])) and torch.allclose(got[0].cpu(), want[0], atol=1e-4)
        assert transformers_amd.fallback_calls() == {f"{name}:{why}": 1}, (why, transformers_amd.fallback_calls())
        assert experts.router_call_count() == 0, why
    # "device": a CPU module and a CPU tensor next to a GPU -- the reference's forward, the reference's result.  (Fallbacks are
    # counted for GPU tensors alone, models/common.py; under the CPU execution model a CPU tensor IS device memory.)
    if dev.type == "cuda":
        r, x = _router(), torch.randn(5, H, generator=g).bfloat16()
        ref = copy.deepcopy(r)
        ref.__class__ = DeepseekV3TopkRouter
        with torch.no_grad():
            got, want = r(x), ref(x)
        assert experts.router_call_count() == 0 and all(torch.equal(a, b) for a, b in zip(got, want))


def test_router_subclasses(env):
    """A subclass that keeps the reference's forward runs on the kernels; one that overrides it runs ITS forward and is counted
    under `subclass_forward`; `revert` gives both their classes back."""
    class Plain(DeepseekV3TopkRouter):
        pass

    class Scaled(DeepseekV3TopkRouter):
        def forward(self, hidden_states):
            logits, weights, index = super().forward(hidden_states)
            return logits, weights * 2, index

    dev = env.device
    base, geom = make("deepseek_v3")
    a, b = routers(base)
    a.__class__, b.__class__ = Plain, Scaled
    for r in (a, b):
        torch.nn.init.normal_(r.weight, std=0.1)
    ref = copy.deepcopy(base)
    model = accel(copy.deepcopy(base).eval().to(dev))
    ra, rb = routers(model)
    assert isinstance(ra, Plain) and type(ra) is not Plain and isinstance(rb, Scaled) and type(rb) is not Scaled
    x = torch.randn(5, H, generator=torch.Generator().manual_seed(8)).bfloat16()
    experts.router_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        got_a, got_b = ra(x.to(dev)), rb(x.to(dev))
        want_a, want_b = routers(ref)[0](x), routers(ref)[1](x)
    assert experts.router_call_count() == 1
    assert transformers_amd.fallback_calls() == {"TamdScaled:subclass_forward": 1}, transformers_amd.fallback_calls()
    assert got_a[0].dtype == F32 and torch.allclose(got_a[0].cpu(), want_a[0], atol=1e-4)
    assert torch.equal(sets(got_b[2]), sets(want_b[2]))
    transformers_amd.revert(model)
    assert type(ra) is Plain and type(rb) is Scaled
