"""Attention at head_dim 256 (Gemma; csrc/attention_d256_kernel.inc behind tamd_attn_fwd / tamd_attn_decode), under the CPU
execution model and on the MI355X.

Elements: random operands with spiked scores (the deferred rescale fires early and late in a row), every element of O and lse
within kernel_checks.check's gate of the float64 reference of tests/test_attn_elements.py (Case: `s` from the reference's own
quantities, `chain` the kernel's documented roundings); q has padded rows, o and lse sit in guarded buffers.
Refusals: the status, and not one output element.  Model level: a two-layer GemmaForCausalLM through plain `accelerate`."""
import copy
import ctypes

import pytest
import torch

import transformers_amd
from conftest import rel_err
from kernel_checks import BF16, F16, check, rnd
from test_attn_elements import (E_ARG, E_SHAPE, GROUP, OK, Case, Grads, Operands, Out, _call, _params, _stream, _sync,
                                check_lse, h_window, host_mask, host_plan, kv_pattern)
from test_window_cache_models import _stepwise
from transformers import GemmaConfig, GemmaForCausalLM
from transformers_amd import _cabi, ops
from transformers_amd.attention import tamd_attention_forward

D = 256


def operands(b, sq, sk, hq, hkv, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(b, sq, hq, D, generator=g), torch.randn(b, sk, hkv, D, generator=g), torch.randn(b, sk, hkv, D, generator=g)
    k[:, 5::61] *= 6.0  # scores that exceed the running maximum by more than 2^6, early and late in a row
    return Operands(q, k, v, dtype, dev)


CASES = [  # entry, b, sq, sk, hq, hkv, causal, mask
    ("fwd", 2, 129, 129, 2, 2, 1, 0),    # one row past the 128-row workgroup tile and the 64-key tile
    ("fwd", 2, 65, 127, 2, 1, 0, 1),     # a ragged key tile, a wave with one live row, GQA
    ("fwd", 1, 5, 257, 2, 2, 1, 1),      # a multi-token step over a cache (off = 252)
    ("decode", 2, 1, 300, 8, 1, 0, 1),   # MQA (Gemma-2B): the eight heads of the KV head become rows
    ("decode", 8, 5, 257, 32, 4, 1, 1),  # several tiles per split
    ("decode", 2, 1, 300, 2, 2, 0, 1),   # one row, one tile per split
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_elements(env, dtype, case):
    entry, b, sq, sk, hq, hkv, causal, mask = case
    x = operands(b, sq, sk, hq, hkv, dtype, env.device, 7)
    kv = kv_pattern(b, sk, 19) if mask else None
    kv_dev = None if kv is None else kv.to(env.device)  # (held until the call is over: the params carry its address)
    scale = D ** -0.5
    c = Case(x, dtype, scale, host_mask(b, sq, sk, causal, kv)[:, None].expand(b, hq, sq, sk))
    out = Out(b, sq, hq, D, dtype, env.device)
    ap = _params(x.q, x.k, x.v, out.o, out.lse, dtype, scale, causal, kv=kv_dev)
    if entry == "decode":  # (the merged lse bound of tests/test_attn_elements.py counts on it)
        assert host_plan(b, sq, hq, hkv, sk)[0] <= 8
    assert _call(ops.backend(), entry, ap, x.q) == OK
    assert out.intact()
    o, lse = out.o.cpu().double(), out.lse.cpu().double()
    o64, lse64, p64 = c.forward()
    oc, lc, _ = c.forward("q")
    s_o, s_l = c.s_forward(o64, lse64, p64)
    check(f"O d256 {entry}", o, o64, s_o, dtype, chain=rnd(oc, dtype), group=GROUP)
    check_lse(f"lse d256 {entry}", lse, lse64, s_l, lc.float().double())


def test_refusals_write_nothing(env):
    dtype, dev, be = BF16, env.device, ops.backend()
    x = operands(2, 8, 8, 2, 1, dtype, dev, 71)
    z = operands(2, 8, 4, 2, 1, dtype, dev, 73)  # seq_q > seq_k
    planes = h_window(2, 8, 3).to(dev)
    cnt = torch.tensor([3, 8], dtype=torch.int32, device=dev)

    def refused(entry, x_, want, window=None, **kw):
        out = Out(*x_.q.shape, dtype, dev)
        ap = _params(x_.q, x_.k, x_.v, out.o, out.lse, dtype, 0.0625, 1, **kw)
        assert _call(be, entry, ap, x_.q, window) == want, (entry, kw)
        assert out.untouched(), (entry, kw)

    for entry in ("fwd", "decode"):
        refused(entry, x, E_ARG, p=0.1)
        refused(entry, x, E_ARG, planes=planes)
        refused(entry, x, E_ARG, counts=cnt)
        refused(entry, z, E_ARG)
    refused("fwd_window", x, E_SHAPE, window=4)
    refused("decode_window", x, E_SHAPE, window=4)
    o_in = torch.zeros(x.q.shape, dtype=torch.float64)
    gr = Grads(x, o_in, torch.zeros(2, 2, 8, dtype=torch.float64), torch.ones_like(o_in), dtype, dev)
    bp = _cabi.AttnBwdParams()
    bp.fwd = _params(x.q, x.k, x.v, gr.o, gr.lse, dtype, 0.0625, 1)
    bp.dout, bp.dq, bp.dk, bp.dv, bp.delta = gr.do.data_ptr(), gr.dq.data_ptr(), gr.dk.data_ptr(), gr.dv.data_ptr(), gr.dg.t.data_ptr()
    assert be.lib.tamd_attn_bwd(ctypes.byref(bp), _stream(be, x.q)) == E_SHAPE
    _sync(x.q)
    assert gr.untouched()
    q, k, v = (t.clone().requires_grad_() for t in (x.q, x.k, x.v))
    with pytest.raises(ops.TamdError, match="sdpa"):
        ops.attention(q, k, v, 0.0625, True)
    for d in (D, 64):  # logit soft-capping is refused at every head dim, never dropped
        t = torch.zeros(1, 2, 4, d, dtype=dtype, device=dev)
        with pytest.raises(ops.TamdError, match="soft-capping.*sdpa"):
            tamd_attention_forward(None, t, t, t, None, softcap=50.0)


# ---- model level ------------------------------------------------------------------------------------------------------------
B, STEPS = 2, (20, 1, 1, 3, 1)
_REF = {}


def _reference():
    """The reference's fp32 and bf16 eager runs on the CPU (computed once, shared, never modified)."""
    if not _REF:
        torch.manual_seed(5)
        cfg = GemmaConfig(vocab_size=512, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                          num_key_value_heads=1, head_dim=D, max_position_embeddings=256)
        ref = GemmaForCausalLM(cfg).bfloat16().eval()
        ref32 = copy.deepcopy(ref).float()
        total = sum(STEPS)
        ids = torch.randint(1, 512, (B, total))
        am = torch.ones(B, total, dtype=torch.long)
        am[1, :4] = 0
        with torch.no_grad():
            whole = [m(input_ids=ids, attention_mask=am, use_cache=False).logits.float() for m in (ref32, ref)]
        _REF.update(ref=ref, ids=ids, am=am, whole32=whole[0], whole_ref=whole[1],
                    l32=_stepwise(ref32, "dynamic", ids, am, STEPS, "cpu"), lref=_stepwise(ref, "dynamic", ids, am, STEPS, "cpu"))
    return _REF


def _fast(env):
    fast = transformers_amd.accelerate(copy.deepcopy(_reference()["ref"]).to(env.device))
    assert fast.config._attn_implementation == "tamd"
    return fast


def test_model_left_padded_forward(env):
    r = _reference()
    fast = _fast(env)
    transformers_amd.fallback_calls(reset=True)
    with torch.no_grad():
        got = fast(input_ids=r["ids"].to(env.device), attention_mask=r["am"].to(env.device), use_cache=False).logits.float().cpu()
    assert not any("attn" in k.lower() for k in transformers_amd.fallback_calls()), transformers_amd.fallback_calls()
    valid = r["am"].bool()
    e_fast, e_ref = rel_err(got[valid], r["whole32"][valid]), rel_err(r["whole_ref"][valid], r["whole32"][valid])
    print(f"{env.name}: ours {float(e_fast):.5f} reference bf16 {float(e_ref):.5f}")
    assert e_fast <= 1.1 * e_ref + 1e-3, (e_fast, e_ref)


def test_model_cached_steps_and_generate(env):
    r = _reference()
    fast = _fast(env)
    transformers_amd.fallback_calls(reset=True)
    got = _stepwise(fast, "dynamic", r["ids"], r["am"], STEPS, env.device)
    valid, pos = r["am"].bool(), 0
    for i, n in enumerate(STEPS):
        keep = valid[:, pos:pos + n]
        e_fast = rel_err(got[:, pos:pos + n][keep], r["l32"][:, pos:pos + n][keep])
        e_ref = rel_err(r["lref"][:, pos:pos + n][keep], r["l32"][:, pos:pos + n][keep])
        print(f"{env.name} step {i} ({n} tokens at {pos}): ours {float(e_fast):.5f} reference bf16 {float(e_ref):.5f}")
        assert e_fast <= 1.1 * e_ref + 1e-3, (i, n, pos, e_fast, e_ref)
        pos += n
    new = 5
    with torch.no_grad():
        out = fast.generate(r["ids"][:, :12].to(env.device), attention_mask=r["am"][:, :12].to(env.device), max_new_tokens=new,
                            min_new_tokens=new, do_sample=False, pad_token_id=0)
    assert out.shape == (B, 12 + new)
    assert not any("attn" in k.lower() for k in transformers_amd.fallback_calls()), transformers_amd.fallback_calls()
