"""A decode step over a pre-allocated KV cache reads the keys in use and nothing else (ABI 13, tests/test_attn_kvlen.py):
`tamd_mask` hands the attention function the key count as a device tensor, the split-KV kernel stops at it."""
import copy

import pytest
import torch

import transformers_amd
from conftest import rel_err
from test_models import tiny_llama
from transformers import LlamaForCausalLM


@pytest.mark.parametrize("padding_side", [None, "left"])
def test_static_cache_decode_ignores_what_unused_slots_hold(env, padding_side):
    """Prefill of 11 tokens into StaticCache(max_cache_len=32), then two teacher-forced decode steps; before step t the slots
    >= 11 + t of every layer's keys and values in the accelerated model's cache are overwritten with NaN (slot 11 + t is the
    one the step writes).  The logits stay finite and within the static-cache gate of test_models.py (0.0099) of the sdpa
    reference, which runs on its own, un-poisoned cache.  With the validity plane over the whole allocation the stale slots
    took part in P.V as 0 * NaN."""
    from transformers import StaticCache

    torch.manual_seed(23)
    cfg = tiny_llama(False)
    ref = LlamaForCausalLM(cfg).bfloat16().eval()
    ref.set_attn_implementation("sdpa")
    fast = LlamaForCausalLM(copy.deepcopy(cfg)).bfloat16().eval()
    fast.load_state_dict(ref.state_dict())
    fast = transformers_amd.accelerate(fast.to(env.device))
    b, p, steps, max_len = 2, 11, 2, 32
    ids = torch.randint(1, cfg.vocab_size, (b, p + steps))
    am = torch.ones(b, p + steps, dtype=torch.long)
    if padding_side == "left":
        am[1, :4] = 0
    valid = am.bool()

    def run(model, device, poison):
        cache = StaticCache(config=model.config, max_cache_len=max_len)
        outs = []
        with torch.no_grad():
            o = model(input_ids=ids[:, :p].to(device), attention_mask=am[:, :p].to(device), past_key_values=cache,
                      use_cache=True)
            outs.append(o.logits.float().cpu())
            for t in range(steps):
                if poison:
                    for layer in cache.layers:
                        assert layer.keys.shape[2] == max_len and layer.values.shape[2] == max_len
                        layer.keys[:, :, p + t:] = float("nan")
                        layer.values[:, :, p + t:] = float("nan")
                o = model(input_ids=ids[:, p + t: p + t + 1].to(device), attention_mask=am[:, : p + t + 1].to(device),
                          past_key_values=cache, use_cache=True)
                outs.append(o.logits.float().cpu())
        return torch.cat(outs, dim=1)

    want = run(ref, "cpu", False)
    transformers_amd.fallback_calls(reset=True)
    got = run(fast, env.device, True)
    assert transformers_amd.fallback_calls() == {}
    assert got.shape == want.shape == (b, p + steps, cfg.vocab_size)
    assert bool(torch.isfinite(got).all())
    err = rel_err(got[valid], want[valid])
    print(f"static cache, poisoned unused slots ({padding_side}): rel_err {float(err):.5f}")
    assert err < 0.0099
