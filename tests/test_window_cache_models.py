"""`generate()`-style cached inference of sliding-window models through the attention registry: a Mistral-shaped decoder (2
layers, heads of 64, grouped-query attention) over the reference's own DynamicCache / StaticCache built from its config -- the
DynamicSlidingWindowLayer / StaticSlidingWindowLayer of cache_utils.py:203-277, :504-628.

Teacher-forced, step by step: a prefill shorter than the window, two decode steps, a 6-token step that crosses the window, a
decode step, a 3-token step over the cropped cache, a decode step, and a 20-token step (a second chat turn).  The multi-token
steps over the non-empty cache are the ones whose first rows no longer see the oldest keys they are handed: the kernels'
window entries (on the GPU the window is 160, so the 6- and 3-token steps take the split-KV schedule and the 20-token step the
forward kernel).  Gate at every step: the project's noise-floor rule against the reference's fp32 eager run with the same cache
class (tests/test_models.py)."""
import copy

import pytest
import torch

import transformers_amd
from conftest import record, rel_err
from transformers import MistralConfig, MistralForCausalLM

B = 2


def _window(env):
    return 160 if env.big else 20


def _steps(window):
    return [window - 5, 1, 1, 6, 1, 3, 1, 20]


def _config(window):
    return MistralConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=1, head_dim=64, max_position_embeddings=1024, sliding_window=window,
                         rms_norm_eps=1e-5, attn_implementation="eager")


def _cache(kind, model, total):
    from transformers import DynamicCache, StaticCache

    return DynamicCache(config=model.config) if kind == "dynamic" else StaticCache(config=model.config, max_cache_len=total + 4)


def _stepwise(model, kind, ids, am, steps, device):
    """Teacher-forced cached run -> the logits of every step, concatenated [B, total, V] (fp32, CPU)."""
    cache = _cache(kind, model, ids.shape[1])
    outs, pos = [], 0
    with torch.no_grad():
        for n in steps:
            kw = {} if am is None else {"attention_mask": am[:, :pos + n].to(device)}
            o = model(input_ids=ids[:, pos:pos + n].to(device), past_key_values=cache, use_cache=True, **kw)
            outs.append(o.logits.float().cpu())
            pos += n
    return torch.cat(outs, dim=1)


_REF = {}


def _reference(window, kind, padded):
    """The reference's fp32 and bf16 eager runs (CPU; computed once per case, shared, never modified)."""
    key = (window, kind, padded)
    if key not in _REF:
        torch.manual_seed(33)
        ref = MistralForCausalLM(_config(window)).bfloat16().eval()
        ref32 = copy.deepcopy(ref).float()
        steps = _steps(window)
        total = sum(steps)
        ids = torch.randint(1, 512, (B, total))
        am = None
        if padded:
            am = torch.ones(B, total, dtype=torch.long)
            am[1, :4] = 0
        _REF[key] = dict(ref=ref, ref32=ref32, ids=ids, am=am, steps=steps,
                         l32=_stepwise(ref32, kind, ids, am, steps, "cpu"), lref=_stepwise(ref, kind, ids, am, steps, "cpu"))
    return _REF[key]


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "left_padded"])
@pytest.mark.parametrize("kind", ["dynamic", "static"])
def test_cached_steps_over_a_sliding_window_cache(env, kind, padded):
    window = _window(env)
    r = _reference(window, kind, padded)
    ids, am, steps = r["ids"], r["am"], r["steps"]
    fast = transformers_amd.accelerate(copy.deepcopy(r["ref"]).to(env.device))
    assert fast.config._attn_implementation == "tamd"
    transformers_amd.fallback_calls(reset=True)
    got = _stepwise(fast, kind, ids, am, steps, env.device)
    assert not any("attn" in k.lower() for k in transformers_amd.fallback_calls()), transformers_amd.fallback_calls()
    valid = torch.ones(B, ids.shape[1], dtype=torch.bool) if am is None else am.bool()
    pos, worst = 0, 0.0
    for i, n in enumerate(steps):
        keep = valid[:, pos:pos + n]
        e_fast = rel_err(got[:, pos:pos + n][keep], r["l32"][:, pos:pos + n][keep])
        e_ref = rel_err(r["lref"][:, pos:pos + n][keep], r["l32"][:, pos:pos + n][keep])
        record("window_cache_model", f"{kind}_{'padded' if padded else 'plain'}_step{i}_{env.name}", e_fast, e_ref)
        print(f"{kind} padded={padded} step {i} ({n} tokens at {pos}): ours {float(e_fast):.5f} reference bf16 {float(e_ref):.5f}")
        assert e_fast <= 1.1 * e_ref + 1e-3, (i, n, pos, e_fast, e_ref)
        worst = max(worst, float(e_fast))
        pos += n
    # the cached steps against the same model's forward over the whole sequence without a cache (the bound planes)
    with torch.no_grad():
        kw = {} if am is None else {"attention_mask": am.to(env.device)}
        whole = fast(input_ids=ids.to(env.device), use_cache=False, **kw).logits.float().cpu()
    assert rel_err(got[valid], whole[valid]) < 1e-2
    # the window matters: without it the positions past the window come out differently
    cfg_full = copy.deepcopy(r["ref32"].config)
    cfg_full.sliding_window = None
    full32 = MistralForCausalLM(cfg_full).float().eval()
    full32.load_state_dict(r["ref32"].state_dict())
    with torch.no_grad():
        kw = {} if am is None else {"attention_mask": am}
        full = full32(input_ids=ids, use_cache=False, **kw).logits
    assert rel_err(got[0, window:], full[0, window:]) > 10 * worst


@pytest.mark.parametrize("cache_implementation", [None, "static"], ids=["default_cache", "static_cache"])
def test_generate_runs_past_the_window(env, cache_implementation):
    window = _window(env)
    torch.manual_seed(34)
    fast = transformers_amd.accelerate(MistralForCausalLM(_config(window)).bfloat16().eval().to(env.device))
    p, new = window - 8, 14
    ids = torch.randint(1, 512, (B, p))
    am = torch.ones(B, p, dtype=torch.long)
    am[1, :3] = 0
    kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=False, pad_token_id=0)
    if cache_implementation is not None:
        kw["cache_implementation"] = cache_implementation
    out = fast.generate(ids.to(env.device), attention_mask=am.to(env.device), **kw)
    assert out.shape == (B, p + new) and p + new > window
    assert torch.equal(out[:, :p].cpu(), ids)
    assert int(out.min()) >= 0 and int(out.max()) < 512


def test_mixtral_with_a_window_prefill_and_decode(env):
    """A sparse mixture-of-experts model with a sliding window: attention and experts on the kernels, one prefill past the
    window, one multi-token step over the cropped cache, one decode step."""
    from transformers import DynamicCache, MixtralConfig, MixtralForCausalLM

    from transformers_amd import experts

    torch.manual_seed(35)
    window = 16
    cfg = MixtralConfig(vocab_size=512, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=64, num_local_experts=4, num_experts_per_tok=2,
                        max_position_embeddings=256, rms_norm_eps=1e-5, attn_implementation="eager",
                        experts_implementation="eager", router_jitter_noise=0.0, sliding_window=window)
    fast = MixtralForCausalLM(cfg).bfloat16().eval().to(env.device)
    fast.set_attn_implementation("tamd")
    fast.set_experts_implementation("tamd")
    ids = torch.randint(1, 512, (B, 30)).to(env.device)
    cache = DynamicCache(config=fast.config)
    experts.call_count(reset=True)
    transformers_amd.fallback_calls(reset=True)
    outs, pos = [], 0
    with torch.no_grad():
        for n in (24, 5, 1):
            outs.append(fast(input_ids=ids[:, pos:pos + n], past_key_values=cache, use_cache=True).logits)
            pos += n
    assert experts.call_count() == 6  # two layers, three forwards
    assert transformers_amd.fallback_calls() == {}, transformers_amd.fallback_calls()
    got = torch.cat(outs, dim=1)
    assert got.shape == (B, 30, 512) and bool(torch.isfinite(got).all())


def test_attention_function_checks_what_a_window_mask_promises(env):
    """The registered attention function under a window-carrying mask: causal, at least two queries, exactly the keys the mask
    covers; and the `sliding_window` keyword alone over a longer cache stays refused."""
    from transformers_amd.attention import TamdMask, tamd_attention_forward
    from transformers_amd.ops import TamdError

    dev = env.device
    torch.manual_seed(36)
    q = torch.randn(1, 2, 4, 64).bfloat16().to(dev)     # [B, H, S, D]
    k = torch.randn(1, 1, 40, 64).bfloat16().to(dev)
    mod = torch.nn.Identity().eval()
    kv = torch.ones(1, 40, dtype=torch.bool, device=dev)
    out, _ = tamd_attention_forward(mod, q, k, k, TamdMask(kv, None, None, 10), scaling=0.125, is_causal=True, sliding_window=10)
    want = transformers_amd.ops.attention(q.transpose(1, 2), k.transpose(1, 2), k.transpose(1, 2), 0.125, True, kv, window=10)
    assert torch.equal(out, want)
    assert torch.equal(tamd_attention_forward(mod, q, k, k, TamdMask(None, None, None, 10), scaling=0.125, is_causal=True)[0], want)
    with pytest.raises(TamdError):   # a mask over fewer keys than the cache returned
        tamd_attention_forward(mod, q, k, k, TamdMask(kv[:, :30], None, None, 10), scaling=0.125, is_causal=True)
    with pytest.raises(TamdError):   # not causal
        tamd_attention_forward(mod, q, k, k, TamdMask(kv, None, None, 10), scaling=0.125, is_causal=False)
    with pytest.raises(TamdError):   # one query
        tamd_attention_forward(mod, q[:, :, :1], k, k, TamdMask(kv, None, None, 10), scaling=0.125, is_causal=True)
    with pytest.raises(TamdError):   # the keyword without a window-carrying mask: 4 queries over 40 keys
        tamd_attention_forward(mod, q, k, k, kv, scaling=0.125, is_causal=True, sliding_window=10)
