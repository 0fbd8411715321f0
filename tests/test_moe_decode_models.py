"""`generate()` of a sparse mixture-of-experts model with its decode steps on the weight-streaming expert kernels
(csrc/gemv_moe.inc, torch.ops.tamd.moe_experts_decode): the tiny Mixtral of tests/test_moe_models.py -- two layers, 4 experts,
top-2, the inputs of ITS routing condition (`chosen()`: imported, the seed search is not repeated here) -- under
`attn_implementation="tamd"` + `experts_implementation="tamd"`.

A prompt of 2 x 12 tokens, 8 new tokens, greedy.  The prefill (24 tokens: above the cut) runs the experts on the routed GEMM,
each of the 7 decode steps (2 tokens) on the decode op in both layers: decode_call_count() >= 2 x 7.  Expected tokens: the
reference's own bf16 eager generate() on the CPU, token for token; nothing may fall back."""
import copy

import pytest
import torch

import transformers_amd
from test_moe_models import chosen, config
from transformers import MixtralForCausalLM
from transformers_amd import experts, ops

LAYERS, NEW, PROMPT = 2, 8, 12


@pytest.mark.parametrize("cache", [None, "static"])
def test_generate_decodes_on_the_streaming_kernels(env, cache, monkeypatch):
    monkeypatch.delenv("TAMD_MOE_GEMV", raising=False)
    c = chosen()
    ref = copy.deepcopy(c["ref"]).eval()
    fast = copy.deepcopy(ref).to(env.device)
    fast.set_attn_implementation("tamd")
    fast.set_experts_implementation("tamd")
    prompt = c["ids"][:, :PROMPT]
    assert prompt.numel() > ops.moe_decode_cut() >= prompt.shape[0]  # the prefill above the cut, a decode step below it
    kw = dict(max_new_tokens=NEW, do_sample=False, pad_token_id=0)
    more = {} if cache is None else dict(cache_implementation=cache)
    experts.call_count(reset=True)
    experts.decode_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        want = ref.generate(prompt, **kw)
        got = fast.generate(prompt.to(env.device), **kw, **more)
    assert transformers_amd.fallback_calls() == {}, transformers_amd.fallback_calls()
    assert experts.decode_call_count() >= LAYERS * (NEW - 1), experts.decode_call_count()
    assert experts.call_count() >= experts.decode_call_count() + LAYERS  # every call is counted; the prefill is not a decode call
    assert torch.equal(got.cpu(), want), (got.cpu().tolist(), want.tolist())


def test_accelerate_decodes_and_revert_stops(env, monkeypatch):
    monkeypatch.delenv("TAMD_MOE_GEMV", raising=False)
    torch.manual_seed(1)
    m = MixtralForCausalLM(config()).bfloat16().eval().to(env.device)
    ids = torch.randint(0, 512, (2, PROMPT)).to(env.device)
    kw = dict(max_new_tokens=NEW, do_sample=False, pad_token_id=0)
    transformers_amd.accelerate(m)
    experts.decode_call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        m.generate(ids, **kw)
    assert experts.decode_call_count() >= LAYERS * (NEW - 1) and transformers_amd.fallback_calls() == {}
    transformers_amd.revert(m)
    experts.decode_call_count(reset=True)
    with torch.no_grad():
        m.generate(ids, **kw)
    assert experts.decode_call_count() == 0  # the reference's experts again
