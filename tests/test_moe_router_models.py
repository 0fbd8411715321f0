"""The replacement routers (transformers_amd/models/moe.py) inside tiny models of the four families, under the CPU execution
model (`emu`) and on the MI355X (`hip`): two layers, hidden 128, 64 tokens, bf16, `experts_implementation="tamd"`.

    Mixtral    E = 4,  top-2   (the padded-E path: the gate product runs over 8 rows)
    Qwen3-MoE  E = 8,  top-2,  norm_topk_prob true and false
    Qwen2-MoE  E = 12, top-4,  with its shared expert (padded to 16 rows)
    OLMoE      E = 8,  top-2

A forward hook on every router captures its input and its triple.  Indices: the stable descending sort of the CAPTURED logits,
every row.  Scores: the float64 chain of include/tamd.h on the captured logits within MULT * 2^-23 relative (tests/
test_moe_router.py explains MULT = 4), plus half an ulp of the logits' dtype where the reference rounds the scores to it.
Dtypes and shapes: those of the reference class's own forward on the same module and input.

A/B: the same model accelerated with `moe_router=False` -- both runs on the kernels, differing in the router alone.  The
reference arm's gate product is ATen's, ours the project's GEMM: a logit may differ by one bf16 ulp, so the test asserts first,
as a condition on the inputs, that every gap between neighbours among the k + 1 largest captured logits of the reference arm is
at least 4 bf16 ulps of the larger of the two -- on the model of the first seed of 0, 1, 2, ... whose eager bf16 run on the
CPU meets it; then the indices must be identical, and every quantity q (logits, loss, aux loss, router logits, each parameter
gradient, the gates' included) agrees within

    gate(q) = AB_MULT x max(AB_MEASURED, floor(q)),   AB_MULT = 4

AB_MEASURED = 2e-8: the largest difference measured between the arms (a parameter gradient; logits, loss and aux loss: 0; both
backends; profiles/moe_router_tests.md).  floor(q): ONE element of q off by one bf16 ulp, in the norm-relative metric, elements
of like magnitude: 2^-8 / sqrt(numel(q)) -- 2.2e-5 for the [64, 512] logits, 1.2e-4 for an [8, 128] gate weight; for the scalar
losses, one bf16 ulp of one of the elements they average: 2^-8 / (elements averaged).  So the arms may differ by a few flipped
roundings and by nothing more: an error of 0.1 % in a gate-weight gradient fails.  Freshly initialised routers cannot meet the
margin condition (5 - 40 of 128 rows violate it for every seed tried), so `separate()` gives the test models' routers
separated logits by construction.  Everything measured is recorded through conftest.record ("moe_router_models"), each with
its gate.
"""
import copy

import pytest
import torch

import transformers_amd
from conftest import record, rel_err
from kernel_checks import BF16, F32, ulp
from test_moe_router import MULT, TINY, U23, chain_fwd
from transformers import (MixtralConfig, MixtralForCausalLM, OlmoeConfig, OlmoeForCausalLM, Qwen2MoeConfig, Qwen2MoeForCausalLM,
                          Qwen3MoeConfig, Qwen3MoeForCausalLM)
from transformers_amd import experts
from transformers_amd.models import moe

B, S, LAYERS = 2, 32, 2
AB_MULT = 4.0
AB_MEASURED = 2e-8  # the largest A/B difference measured (module docstring)


def ab_gate(numel, scalar_of=None):
    """AB_MULT x max(what was measured, one bf16 flip in this quantity): module docstring"""
    floor = 2.0 ** -8 / scalar_of if scalar_of else 2.0 ** -8 / numel ** 0.5
    return AB_MULT * max(AB_MEASURED, floor)


COMMON = dict(vocab_size=512, hidden_size=128, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=2,
              num_key_value_heads=1, max_position_embeddings=256, rms_norm_eps=1e-5, attn_implementation="eager",
              experts_implementation="eager")


def make(family, seed=0):
    """-> (model in bf16 on the CPU, E, k)"""
    torch.manual_seed(seed)
    if family == "mixtral":
        return MixtralForCausalLM(MixtralConfig(head_dim=64, num_local_experts=4, num_experts_per_tok=2, router_jitter_noise=0.0,
                                                **COMMON)).bfloat16(), 4, 2
    if family.startswith("qwen3"):
        cfg = Qwen3MoeConfig(head_dim=64, num_experts=8, num_experts_per_tok=2, moe_intermediate_size=128, decoder_sparse_step=1,
                             mlp_only_layers=[], norm_topk_prob=family.endswith("norm"), **COMMON)
        return Qwen3MoeForCausalLM(cfg).bfloat16(), 8, 2
    if family == "qwen2":
        # (use_sliding_window with max_window_layers = the layer count: every layer is full attention, and the window the
        # reference hands its mask builder for the unused "sliding_attention" entry is a valid one)
        cfg = Qwen2MoeConfig(num_experts=12, num_experts_per_tok=4, moe_intermediate_size=128, shared_expert_intermediate_size=128,
                             decoder_sparse_step=1, mlp_only_layers=[], norm_topk_prob=False, use_sliding_window=True,
                             sliding_window=4096, max_window_layers=LAYERS, **COMMON)
        return Qwen2MoeForCausalLM(cfg).bfloat16(), 12, 4
    assert family == "olmoe"
    return OlmoeForCausalLM(OlmoeConfig(num_experts=8, num_experts_per_tok=2, norm_topk_prob=False, **COMMON)).bfloat16(), 8, 2


FAMILIES = ["mixtral", "qwen3_norm", "qwen3_raw", "qwen2", "olmoe"]


def inputs():
    alphabet = torch.randperm(512, generator=torch.Generator().manual_seed(5))[:4]
    ids = alphabet[torch.randint(0, 4, (B, S), generator=torch.Generator().manual_seed(6))]
    labels = ids.clone()
    labels[0, :4] = -100
    return ids, labels


def routers(model):
    return [m for m in model.modules() if isinstance(m, tuple(moe.REPLACEMENTS))]


class Tap:
    """every router's input and output triple, in call order"""

    def __init__(self, model):
        self.calls = []
        self.handles = [r.register_forward_hook(self._hook) for r in routers(model)]

    def _hook(self, mod, inp, out):
        self.calls.append((mod, inp[0].detach(), tuple(o.detach() for o in out)))

    def close(self):
        for h in self.handles:
            h.remove()
        return self


def margins_ok(calls, k):
    """every gap between neighbours among the k + 1 largest logits (the order inside the top k reaches the outputs too) is at
    least 4 bf16 ulps of the larger of the two logits (each may move by one)"""
    for _mod, _x, (logits, _s, _i) in calls:
        top = logits.double().cpu().sort(-1, descending=True).values
        a, b = top[:, :k], top[:, 1:k + 1]
        if not bool(((a - b) >= 4 * ulp(torch.maximum(a.abs(), b.abs()), BF16)).all()):
            return False
    return True


def separate(model, E, seed):
    """Freshly initialised routers put neighbouring logits within a bf16 ulp of each other on several of 64 tokens for every
    seed tried (5 - 40 rows of 128), and routing is discrete.  So the gate weights are set to a_e * u: u a random unit vector
    per layer, a_e = (perm(e) - (E - 1) / 2) * 2 / E.  Every row's logits are then a_e (u . x): neighbours differ by at least
    2 / (E - 1) of the larger one whatever the token, tokens with u . x > 0 and < 0 go to different experts, and the softmax stays
    unsaturated (logits of order 1)."""
    g = torch.Generator().manual_seed(100 + seed)
    for r in routers(model):
        u = torch.randn(r.weight.shape[1], generator=g)
        a = (torch.randperm(E, generator=g).float() - (E - 1) / 2) * (2.0 / E)
        with torch.no_grad():
            r.weight.copy_((a[:, None] * (u / u.norm())[None, :]).to(r.weight.dtype))


_CHOSEN = {}


def chosen(family):
    """The model of the first seed of 0, 1, 2, ... whose reference run (bf16, eager, on the CPU) meets `margins_ok` in every
    layer: a property of the inputs alone; computed once per session, shared, never modified."""
    if family not in _CHOSEN:
        ids, labels = inputs()
        for seed in range(32):
            base, E, k = make(family, seed)
            separate(base, E, seed)
            tap = Tap(base)
            with torch.no_grad():
                base(input_ids=ids, use_cache=False)
            if margins_ok(tap.close().calls, k):
                _CHOSEN[family] = (base, E, k)
                break
        else:
            raise AssertionError("no seed of 0 .. 31 meets the margin condition")
    return _CHOSEN[family]


def run(model, ids, labels, **kw):
    model.zero_grad()
    tap = Tap(model)
    out = model(input_ids=ids, labels=labels, use_cache=False, **kw)
    out.loss.backward()
    return out, tap.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_router_inside_the_model(env, family):
    dev = env.device
    base, E, k = chosen(family)
    ids, labels = inputs()
    ids, labels = ids.to(dev), labels.to(dev)
    fast = transformers_amd.accelerate(copy.deepcopy(base).train().to(dev))
    arm = transformers_amd.accelerate(copy.deepcopy(base).train().to(dev), moe_router=False)
    assert len(routers(fast)) == LAYERS and all(type(r) in moe.REPLACEMENTS.values() for r in routers(fast))
    assert all(type(r) in moe.REPLACEMENTS for r in routers(arm))
    # ---- the reference arm first: the condition on the inputs
    o_arm, t_arm = run(arm, ids, labels)
    assert margins_ok(t_arm.calls, k), family
    # ---- ours
    transformers_amd.fallback_calls(reset=True)
    experts.router_call_count(reset=True)
    o, tap = run(fast, ids, labels)
    assert experts.router_call_count() == LAYERS
    assert transformers_amd.fallback_calls() == {}, transformers_amd.fallback_calls()
    assert len(tap.calls) == len(t_arm.calls) == LAYERS
    for layer, ((mod, x, (logits, scores, index)), (_m, _x, (l_arm, s_arm, i_arm))) in enumerate(zip(tap.calls, t_arm.calls)):
        ref_cls = type(mod).__mro__[1]
        assert ref_cls in moe.REPLACEMENTS
        with torch.no_grad():
            want = ref_cls.forward(mod, x)  # the reference class's own forward on the same module and input
        for got_t, want_t in zip((logits, scores, index), want):
            assert got_t.dtype == want_t.dtype and got_t.shape == want_t.shape, (family, layer, got_t.dtype, want_t.dtype)
        assert logits.shape == (B * S, E) and index.shape == (B * S, k)
        l64 = logits.double().cpu()
        norm = True if family == "mixtral" else bool(mod.norm_topk_prob)
        w64, idx64 = chain_fwd(l64, k, norm)
        assert torch.equal(index.cpu(), idx64), (family, layer)  # every row
        tol = MULT * U23 * w64 + TINY + (0.5 * ulp(w64, scores.dtype) if scores.dtype != F32 else 0.0)
        err = (scores.double().cpu() - w64).abs()
        if scores.dtype == F32:  # (behind the reference's rounding to bf16 the figure is that rounding's)
            record("moe_router_models", f"{env.name} {family} layer {layer} scores rel err / 2^-24",
                   (err / w64).max().item() / 2.0 ** -24, MULT * 2)
        assert bool((err <= tol).all()), (family, layer, (err / w64).max().item())
        assert torch.equal(index.cpu(), i_arm.cpu()), (family, layer, "the two arms route alike")
    # ---- A/B: logits, loss, every parameter gradient
    d = rel_err(o.logits, o_arm.logits)
    record("moe_router_models", f"{env.name} {family} logits vs moe_router=False", d, ab_gate(o.logits.numel()))
    assert d <= ab_gate(o.logits.numel()), (family, float(d))
    dl = abs(o.loss.item() - o_arm.loss.item()) / abs(o_arm.loss.item())
    record("moe_router_models", f"{env.name} {family} loss vs moe_router=False", dl, ab_gate(1, scalar_of=B * S))
    assert dl <= ab_gate(1, scalar_of=B * S), (family, dl)
    g_arm = dict(arm.named_parameters())
    worst, seen_gate = 0.0, False
    for n, p in fast.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        dg = rel_err(p.grad, g_arm[n].grad)
        worst = max(worst, float(dg))
        assert dg <= ab_gate(p.numel()), (family, n, float(dg), ab_gate(p.numel()))
        if n.endswith("mlp.gate.weight"):
            record("moe_router_models", f"{env.name} {family} {n} gradient vs moe_router=False", dg, ab_gate(p.numel()))
        seen_gate = seen_gate or n.endswith("mlp.gate.weight")
    assert seen_gate
    record("moe_router_models", f"{env.name} {family} worst gradient vs moe_router=False (gates: AB_MULT = 4 x a flip)", worst)
    # ---- revert
    gates = [m.shared_expert_gate for m in fast.modules() if hasattr(m, "shared_expert_gate")]
    assert len(gates) == (LAYERS if family == "qwen2" else 0) and all(type(g) is moe.TamdSharedExpertGate for g in gates)
    transformers_amd.revert(fast)
    assert all(type(r) in moe.REPLACEMENTS for r in routers(fast))
    assert all(type(g) is torch.nn.Linear for g in gates)
    assert not any("_tamd_padded_gate" in m.__dict__ for m in fast.modules())  # the padded weights do not outlive revert


def test_output_router_logits_and_aux_loss(env):
    dev = env.device
    base, E, k = chosen("mixtral")
    ids, labels = (t.to(dev) for t in inputs())
    fast = transformers_amd.accelerate(copy.deepcopy(base).train().to(dev))
    arm = transformers_amd.accelerate(copy.deepcopy(base).train().to(dev), moe_router=False)
    experts.router_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    o, _ = run(fast, ids, labels, output_router_logits=True)
    o_arm, _ = run(arm, ids, labels, output_router_logits=True)
    assert experts.router_call_count() == LAYERS and transformers_amd.fallback_calls() == {}
    assert o.aux_loss is not None and o.router_logits is not None and len(o.router_logits) == LAYERS
    for a, b in zip(o.router_logits, o_arm.router_logits):
        assert a.shape == b.shape == (B * S, E) and a.dtype == b.dtype
        assert rel_err(a, b) <= ab_gate(a.numel())
    d = abs(o.aux_loss.item() - o_arm.aux_loss.item()) / abs(o_arm.aux_loss.item())
    aux_gate = ab_gate(1, scalar_of=LAYERS * B * S * E)
    record("moe_router_models", f"{env.name} aux_loss vs moe_router=False", d, aux_gate)
    assert d <= aux_gate
    assert abs(o.loss.item() - o_arm.loss.item()) <= ab_gate(1, scalar_of=B * S) * abs(o_arm.loss.item())


@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_generate_runs_every_step_through_the_router(env, cache):
    dev = env.device
    base, _E, _k = make("mixtral")
    fast = transformers_amd.accelerate(copy.deepcopy(base).eval().to(dev))
    ids, _ = inputs()
    prompt = ids[:, :12].to(dev)
    steps = 6
    kw = dict(max_new_tokens=steps, min_new_tokens=steps, do_sample=False, pad_token_id=0)
    if cache == "static":
        kw["cache_implementation"] = "static"
    experts.router_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        out = fast.generate(prompt, **kw)
    assert out.shape == (B, 12 + steps)
    assert experts.router_call_count() == LAYERS * steps, experts.router_call_count()  # the prefill and every decode step
    assert transformers_amd.fallback_calls() == {}, transformers_amd.fallback_calls()


def test_refusals_are_counted(env):
    """An fp32 router module and top_k > 16 are not approximated: the reference's forward runs, and is counted."""
    dev = env.device
    base, E, k = make("qwen3_norm")
    transformers_amd.accelerate(base)
    r32 = copy.deepcopy(routers(base)[0]).float().to(dev)
    torch.nn.init.normal_(r32.weight, std=0.1)
    x = torch.randn(5, 128, generator=torch.Generator().manual_seed(3))
    experts.router_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        got = r32(x.to(dev))
        want = type(r32).__mro__[1].forward(copy.deepcopy(r32).cpu(), x)
    assert transformers_amd.fallback_calls() == {"TamdQwen3MoeTopKRouter:dtype": 1}, transformers_amd.fallback_calls()
    assert torch.allclose(got[1].cpu(), want[1], atol=1e-5) and torch.equal(got[2].cpu(), want[2])
    # top_k > 16 on a patched config: 32 experts, top-17
    torch.manual_seed(4)
    cfg = Qwen3MoeConfig(head_dim=64, num_experts=32, num_experts_per_tok=17, moe_intermediate_size=128, decoder_sparse_step=1,
                         mlp_only_layers=[], norm_topk_prob=True, **COMMON)
    wide = copy.deepcopy(routers(Qwen3MoeForCausalLM(cfg).bfloat16())[0])
    wide.__class__ = moe.TamdQwen3MoeTopKRouter
    wide = wide.to(dev)
    torch.nn.init.normal_(wide.weight, std=0.1)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        _l, s, i = wide(x.bfloat16().to(dev))
    assert s.shape == i.shape == (5, 17)
    assert transformers_amd.fallback_calls() == {"TamdQwen3MoeTopKRouter:top_k": 1}, transformers_amd.fallback_calls()
    assert experts.router_call_count() == 0


def test_router_subclasses(env):
    """A subclass of a router class is not in the exact-class table: one that keeps the reference's forward runs on the
    kernels; one that overrides it runs ITS forward and is counted; `revert` gives both their classes back."""
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeTopKRouter

    class Plain(Qwen3MoeTopKRouter):
        pass

    class Scaled(Qwen3MoeTopKRouter):
        def forward(self, hidden_states):
            logits, scores, index = super().forward(hidden_states)
            return logits, scores * 2, index

    dev = env.device
    base, E, k = make("qwen3_norm")
    a, b = routers(base)
    a.__class__, b.__class__ = Plain, Scaled
    ref = copy.deepcopy(base)
    model = transformers_amd.accelerate(copy.deepcopy(base).eval().to(dev))
    ra, rb = routers(model)
    assert isinstance(ra, Plain) and type(ra) is not Plain and isinstance(rb, Scaled) and type(rb) is not Scaled
    x = torch.randn(5, 128, generator=torch.Generator().manual_seed(8)).bfloat16()
    experts.router_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        got_a, got_b = ra(x.to(dev)), rb(x.to(dev))
        want_b = routers(ref)[1](x)
    assert experts.router_call_count() == 1
    assert transformers_amd.fallback_calls() == {"TamdScaled:subclass_forward": 1}, transformers_amd.fallback_calls()
    w64, idx64 = chain_fwd(got_a[0].double().cpu(), k, True)
    assert torch.equal(got_a[2].cpu(), idx64)
    assert bool(((got_a[1].double().cpu() - w64).abs() <= MULT * U23 * w64 + 0.5 * ulp(w64, BF16)).all())
    assert torch.equal(got_b[2].cpu(), want_b[2]) and torch.allclose(got_b[1].float().cpu(), want_b[1].float(), rtol=2e-2)
    transformers_amd.revert(model)
    assert type(ra) is Plain and type(rb) is Scaled
