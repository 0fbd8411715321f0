"""A sparse mixture-of-experts model through the unchanged reference classes: MixtralForCausalLM with
`attn_implementation="tamd"` and `experts_implementation="tamd"` -- the experts of every block on the routing kernels and the
routed GEMM (transformers_amd/experts.py, torch.ops.tamd.moe_experts).

Model: two layers, hidden 128, 2 heads of 64 over 1 KV head, intermediate 128, 4 experts, top-2, vocabulary 512; batch 2 x 32
tokens, bf16.  Reference: the same weights in fp32 with eager attention and eager experts.  Yardstick: the reference's own bf16
eager run.  Gate: the rule and margins tests/test_models.py applies to its Llama cases -- logits: ours against fp32 within
1.1 x the reference's bf16 error against fp32 + 1e-3; loss within 2e-3 relative + 2e-3; every parameter gradient (the router's
included) within 1.25 x + 2e-3.

Routing is discrete: a near-tie in a router flips an expert and the comparison stops being about arithmetic.  That is a
CONDITION on the inputs, not a tolerance: the inputs are those of the first seed of the sequence 0, 1, 2, ... for which (a) the
reference's fp32 and bf16 runs choose the same top-k SET for every token in every layer and (b) the fp32 run's margin between
the k-th and the (k+1)-th router probability is at least 10 x the largest difference between the two runs' router
probabilities -- checked on the CPU, a property of the inputs alone.  That seed is SEED below (asserted).  The test then asserts
that OUR run chooses the same sets too, for every token and layer; nothing is excluded.

What that condition asks of the inputs.  With 64 tokens drawn from the whole vocabulary the 128 (token, layer) margins of a
freshly initialised router are 128 independent draws of a gap whose typical size is 0.03, while the bf16 runs move a
probability by 6e-4 .. 1e-3: the SMALLEST of 128 gaps reached 0.02 .. 2.3 x that over the seeds 0 .. 47, never 10 x (a chance
of about 1e-10 per seed).  The token ids are therefore drawn, per seed, from an alphabet of FOUR ids of the vocabulary: the
hidden state a router sees is dominated by its token's embedding, the margins cluster per (id, layer), and 8 clusters
clear 10 x the noise for one seed in some twenty.  Seed 19 is the first: margin 6.8e-3, noise 5.6e-4 (12 x).  The expert
sets it routes to: {0, 2} in layer 0, {1, 2} and {1, 3} in layer 1 -- experts without any row included; the ragged
geometries are tests/test_moe_kernels.py's business."""
import copy

import pytest
import torch

import transformers_amd
from conftest import record, rel_err
from transformers import MixtralConfig, MixtralForCausalLM
from transformers_amd import experts

SEED = 19  # the first seed of 0, 1, 2, ... that meets the routing condition (found by `chosen()`, asserted there)
B, S = 2, 32


def config():
    return MixtralConfig(vocab_size=512, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=1, head_dim=64, num_local_experts=4, num_experts_per_tok=2,
                         max_position_embeddings=256, rms_norm_eps=1e-5, attn_implementation="eager",
                         experts_implementation="eager", router_jitter_noise=0.0, output_router_logits=False)


class RouterTap:
    """Records every router's probabilities (softmax of its logits in fp32, as MixtralTopKRouter computes them) and top-k sets."""

    def __init__(self, model):
        self.probs, self.sets = [], []
        self.handles = [l.mlp.gate.register_forward_hook(self._hook) for l in model.model.layers]

    def _hook(self, _mod, _inp, out):
        logits, _scores, index = out
        self.probs.append(torch.softmax(logits.detach().float().cpu(), -1))
        self.sets.append(torch.sort(index.detach().cpu(), -1).values)

    def close(self):
        for h in self.handles:
            h.remove()
        return self


def run(model, ids, labels):
    tap = RouterTap(model)
    out = model(input_ids=ids, labels=labels, use_cache=False)
    out.loss.backward()
    return out, tap.close()


def build(seed):
    torch.manual_seed(seed)
    ref = MixtralForCausalLM(config()).bfloat16().train()
    ref32 = copy.deepcopy(ref).float()
    alphabet = torch.randperm(512, generator=torch.Generator().manual_seed(seed))[:4]
    ids = alphabet[torch.randint(0, 4, (B, S), generator=torch.Generator().manual_seed(seed + 1000))]
    labels = ids.clone()
    labels[0, :4] = -100
    return ref, ref32, ids, labels


_CHOSEN = {}


def chosen():
    """The two reference runs of the first seed that meets the routing condition (CPU; computed once, shared, never modified)."""
    if not _CHOSEN:
        for seed in range(32):
            ref, ref32, ids, labels = build(seed)
            o32, t32 = run(ref32, ids, labels)
            oref, tref = run(ref, ids, labels)
            same_sets = all(torch.equal(a, b) for a, b in zip(t32.sets, tref.sets))
            k = ref.config.num_experts_per_tok
            margin = min((p.sort(-1, descending=True).values[:, k - 1] - p.sort(-1, descending=True).values[:, k]).min().item()
                         for p in t32.probs)
            noise = max((a - b).abs().max().item() for a, b in zip(t32.probs, tref.probs))
            if same_sets and margin >= 10 * noise:
                _CHOSEN.update(seed=seed, ref=ref, ref32=ref32, ids=ids, labels=labels, o32=o32, oref=oref, t32=t32,
                               margin=margin, noise=noise)
                break
        else:
            raise AssertionError("no seed of 0 .. 31 meets the routing condition")
    assert _CHOSEN["seed"] == SEED, _CHOSEN["seed"]
    return _CHOSEN


def test_mixtral_forward_backward_parity(env):
    c = chosen()
    ref, ref32, ids, labels, o32, oref = c["ref"], c["ref32"], c["ids"], c["labels"], c["o32"], c["oref"]
    dev = env.device
    fast = copy.deepcopy(ref)
    fast.zero_grad()
    fast = fast.to(dev)
    fast.set_attn_implementation("tamd")
    fast.set_experts_implementation("tamd")
    assert fast.config._experts_implementation == "tamd" and fast.config._attn_implementation == "tamd"
    transformers_amd.fallback_calls(reset=True)
    experts.call_count(reset=True)
    o, tap = run(fast, ids.to(dev), labels.to(dev))
    assert experts.call_count() == 2  # once per layer
    assert transformers_amd.fallback_calls() == {}, transformers_amd.fallback_calls()
    # the condition: fp32, the reference's bf16 run and ours route every token of every layer to the same experts
    assert len(tap.sets) == len(c["t32"].sets) == 2
    for layer, (a, b) in enumerate(zip(tap.sets, c["t32"].sets)):
        assert torch.equal(a, b), (layer, (a != b).any(-1).sum().item())
    e_fast, e_ref = rel_err(o.logits, o32.logits), rel_err(oref.logits, o32.logits)
    record("mixtral_model", "logits", e_fast, e_ref)
    assert e_fast <= 1.1 * e_ref + 1e-3, (e_fast, e_ref)
    record("mixtral_model", "loss_abs", abs(o.loss.item() - o32.loss.item()), abs(oref.loss.item() - o32.loss.item()))
    assert abs(o.loss.item() - o32.loss.item()) <= 2e-3 * abs(o32.loss.item()) + 2e-3
    g32, gref = dict(ref32.named_parameters()), dict(ref.named_parameters())
    seen_gate = False
    for n, p in fast.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ef, er = rel_err(p.grad, g32[n].grad), rel_err(gref[n].grad, g32[n].grad)
        record("mixtral_model", n, ef, er)
        assert ef <= 1.25 * er + 2e-3, (n, ef, er)
        seen_gate = seen_gate or n.endswith("mlp.gate.weight")
    assert seen_gate


def test_accelerate_selects_the_key_and_revert_restores_it(env):
    torch.manual_seed(1)
    m = MixtralForCausalLM(config()).bfloat16().eval().to(env.device)
    before = dict(m.get_experts_implementation())
    assert before[""] == "eager"
    transformers_amd.accelerate(m)
    assert m.config._experts_implementation == "tamd" and m.config._attn_implementation == "tamd"
    ids = torch.randint(0, 512, (1, 16)).to(env.device)
    experts.call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        m(input_ids=ids, use_cache=False)
    assert experts.call_count() == 2 and transformers_amd.fallback_calls() == {}
    transformers_amd.revert(m)
    assert dict(m.get_experts_implementation()) == before
    with torch.no_grad():
        m(input_ids=ids, use_cache=False)
    assert experts.call_count() == 2  # the reference's experts again
    experts.register()  # idempotent
    from transformers.integrations.moe import ALL_EXPERTS_FUNCTIONS

    assert ALL_EXPERTS_FUNCTIONS["tamd"] is experts.tamd_experts_forward


def test_unsupported_experts_take_the_reference_path_and_are_counted(env):
    """fp32 weights and a biased experts module are not approximated: the module's own forward runs, and is counted."""
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    torch.manual_seed(2)
    cfg = config()
    cfg._experts_implementation = "tamd"
    dev = env.device
    x = torch.randn(24, 128)
    idx = torch.stack([torch.randperm(4)[:2] for _ in range(24)])
    w = torch.softmax(torch.randn(24, 2), -1)
    for what in ("dtype", "bias"):
        mod = MixtralExperts(cfg)
        torch.nn.init.normal_(mod.gate_up_proj, std=0.05)
        torch.nn.init.normal_(mod.down_proj, std=0.05)
        want_mod = copy.deepcopy(mod)
        want_mod.config = copy.deepcopy(cfg)
        want_mod.config._experts_implementation = "eager"
        if what == "bias":
            mod, want_mod = mod.bfloat16(), want_mod.bfloat16()
            mod.has_bias = True  # (what @use_experts_implementation(has_bias=True) sets)
            xin = x.bfloat16()
        else:
            xin = x
        mod = mod.to(dev)
        transformers_amd.fallback_calls(reset=True)
        experts.call_count(reset=True)
        with torch.no_grad():
            got = mod(xin.to(dev), idx.to(dev), w.to(dev))
            want = want_mod(xin, idx, w)
        assert experts.call_count() == 0
        assert transformers_amd.fallback_calls() == {f"MixtralExperts:{what}": 1}, transformers_amd.fallback_calls()
        assert torch.allclose(got.float().cpu(), want.float(), atol=1e-2 if what == "bias" else 1e-5)


def test_generate_matches_the_reference_path(env):
    c = chosen()
    ref = copy.deepcopy(c["ref"]).eval()
    fast = copy.deepcopy(ref).to(env.device)
    fast.set_attn_implementation("tamd")
    fast.set_experts_implementation("tamd")
    prompt = c["ids"][:, :12]
    kw = dict(max_new_tokens=8, do_sample=False, pad_token_id=0)
    experts.call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        want = ref.generate(prompt, **kw)
        got = fast.generate(prompt.to(env.device), **kw)
    assert experts.call_count() >= 2 * 8 and transformers_amd.fallback_calls() == {}, transformers_amd.fallback_calls()
    assert torch.equal(got.cpu(), want), (got.cpu().tolist(), want.tolist())
