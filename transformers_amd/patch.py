"""In-place module replacement (SURVEY.md §8b "B2").

The reference's registry route (`register_patch_mapping` + `apply_patches`,
src/transformers/monkey_patching.py:85-155, 233-297) crashes in environments without torchvision
(`dir()` on lazy alias modules, monkey_patching.py:275), so the swap is done post-construction:
`module.__class__ = Replacement` for every module whose class is in the replacement tables.  The
replacement classes subclass the originals and add no parameters, so this is exact and reversible.
"""
from __future__ import annotations

from typing import Dict, Type

import torch
from torch import nn

from . import attention, experts


def _tables(moe_router: bool = True) -> Dict[Type[nn.Module], Type[nn.Module]]:
    from .models import bert, clip, common, gpt2, llama

    table: Dict[Type[nn.Module], Type[nn.Module]] = {}
    for mod in (common, llama, bert, clip, gpt2):
        table.update(mod.REPLACEMENTS)
    moe = _moe() if moe_router else None
    if moe is not None:
        table.update(moe.REPLACEMENTS)
    return table


_MOE_MISSING = False


def _moe():
    """models/moe.py, or None -- said once -- with a reference that lacks one of the four sparse-MoE model families it
    subclasses.  Only those four imports are guarded: an error inside the project's own module is raised."""
    global _MOE_MISSING
    import importlib

    for family in ("mixtral", "qwen2_moe", "qwen3_moe", "olmoe"):
        try:
            importlib.import_module(f"transformers.models.{family}.modeling_{family}")
        except ImportError as e:
            if not _MOE_MISSING:
                import warnings

                warnings.warn(f"transformers_amd.accelerate: the reference has no {family} model ({e}); the MoE routers stay "
                              "the reference's")
                _MOE_MISSING = True
            return None
    from .models import moe

    return moe


def accelerate(model: nn.Module, attn_implementation: bool = True, fuse_loss: bool = True,
               fused_lm_head_loss: bool = False, experts_implementation: bool = True, moe_router: bool = True) -> nn.Module:
    """Switch `model` (any PreTrainedModel containing Llama / BERT / CLIP / GPT-2 blocks) to the MI355X path.

    * registers and selects `attn_implementation="tamd"` (reference API: `set_attn_implementation`,
      src/transformers/modeling_utils.py:2041-2139);
    * on a sparse mixture-of-experts model (one whose experts sit behind `@use_experts_implementation`) registers and selects
      `experts_implementation="tamd"` (reference API: `set_experts_implementation`, modeling_utils.py); `revert` restores
      what `get_experts_implementation()` returned before;
    * swaps norm / MLP / attention / layer modules for their tamd subclasses in place, and -- unless `moe_router=False` (the
      A/B switch) -- the softmax + top-k routers of Mixtral / Qwen2-MoE / Qwen3-MoE / OLMoE blocks and the sigmoid, group-limited
      routers of DeepSeek-V3 / GLM-4-MoE and their copies (models/moe.py);
    * installs the fused cross-entropy as `model.loss_function` for causal-LM heads
      (reference hook: modeling_utils.py:4652-4669);
    * `fused_lm_head_loss=True` (opt-in, Llama): training forwards with labels run the lm_head GEMM and the loss chunk by
      chunk and return `logits=None` -- no [tokens, vocab] tensor is allocated (ops.fused_linear_cross_entropy).
    Returns the same object.
    """
    attention.register()
    experts.register()
    table = _tables(moe_router)
    n = 0
    for m in model.modules():
        repl = table.get(type(m))
        if repl is not None:
            m.__class__ = repl
            n += 1
    if moe_router and _moe() is not None:
        n += _moe().swap_router_subclasses(model)
        n += _moe().swap_shared_expert_gates(model)
    model._tamd_swapped = n
    if n > 0:  # the unchanged Trainer builds DDP without bucket views and registers no hook: ddp.install_trainer_dropin
        from . import ddp

        ddp.install_trainer_dropin()
    if fused_lm_head_loss:
        import types

        from transformers.models.llama.modeling_llama import LlamaForCausalLM

        from .models.llama import fused_causal_lm_forward

        if not isinstance(model, LlamaForCausalLM):
            raise TypeError("fused_lm_head_loss=True is implemented for LlamaForCausalLM")
        model.forward = types.MethodType(fused_causal_lm_forward, model)  # instance attribute: the class is untouched
    from transformers.models.bert.modeling_bert import BertForMaskedLM

    if isinstance(model, BertForMaskedLM) and fuse_loss:
        import types

        from .models.bert import masked_lm_forward

        model.forward = types.MethodType(masked_lm_forward, model)  # instance attribute, like the fused Llama forward
    if attn_implementation and hasattr(model, "set_attn_implementation"):
        dtypes = {p.dtype for p in model.parameters() if p.is_floating_point()}
        if dtypes and not dtypes & {torch.bfloat16, torch.float16}:
            # the kernels are bf16/fp16: an fp32 model keeps the attention backend it has (under autocast the
            # registered function still accepts the fp32 q/k/v autocast leaves behind, attention.py)
            import warnings

            warnings.warn("transformers_amd.accelerate: fp32 model -- attn_implementation is left unchanged "
                          "(the MI355X kernels run bf16/fp16; load with dtype=torch.bfloat16 to use them)")
        else:
            model.set_attn_implementation(attention.ATTN_KEY)
    can_set = getattr(model, "_can_set_experts_implementation", None)
    if experts_implementation and callable(can_set) and can_set() and hasattr(model, "set_experts_implementation"):
        dtypes = {p.dtype for p in model.parameters() if p.is_floating_point()}
        if not dtypes or dtypes & {torch.bfloat16, torch.float16}:  # (an fp32 model keeps its experts, like its attention)
            if "_tamd_experts_was" not in model.__dict__:
                model.__dict__["_tamd_experts_was"] = dict(model.get_experts_implementation())
            model.set_experts_implementation(experts.EXPERTS_KEY)
    # eager weight fusion (before DDP wraps the model)
    for m in model.modules():
        fuse = getattr(m, "_fused", None)
        if callable(fuse) and all(p.is_cuda for p in m.parameters(recurse=True)):
            fuse().weight()
        pad = getattr(m, "_padded", None)
        if callable(pad) and all(p.is_cuda for p in m.parameters(recurse=True)):
            pad().buffers()
    from . import graph_stack

    graph_stack.attach(model)  # forward-only calls of a whole decoder stack replay one HIP graph (graph_stack.py)
    # `generate` with a pre-allocated cache wraps the forward in torch.compile on its own (generation/utils.py:2119-2160,
    # 2862-2863).  Our layers are opaque custom ops around host-side dispatch: the tracer gains nothing and breaks the graph in
    # every layer -- 30.8 ms per token against 5.5 without it at Llama-3-8B dimensions (profiles/r04t_decode_bench_32.jsonl).
    # The reference's own switch turns it off; a caller's explicit GenerationConfig still wins.
    gc = getattr(model, "generation_config", None)
    if gc is not None and n > 0 and not getattr(gc, "disable_compile", False):
        model.__dict__["_tamd_disable_compile_was"] = getattr(gc, "disable_compile", None)
        gc.disable_compile = True
    if fuse_loss and getattr(model, "loss_type", None) == "ForCausalLM":
        from .ops import causal_lm_loss

        model.loss_function = _LossDispatch(causal_lm_loss, model.loss_function)
    return model


class _LossDispatch:
    """GPU logits -> fused cross-entropy kernel; anything else -> the reference loss it replaced."""

    def __init__(self, fast, reference):
        self.fast, self.reference = fast, reference

    def __call__(self, logits, labels, vocab_size, **kwargs):
        from . import ops

        if logits.is_cuda or ops.backend_is_emulated():
            return self.fast(logits=logits, labels=labels, vocab_size=vocab_size, **kwargs)
        return self.reference(logits=logits, labels=labels, vocab_size=vocab_size, **kwargs)


def revert(model: nn.Module) -> nn.Module:
    """Undo `accelerate` (class swaps only; fused weight storage stays valid for the reference modules)."""
    inv = {v: k for k, v in _tables().items()}
    if _moe() is not None:
        _moe().restore(model)  # generated router subclasses, shared-expert gates, cached padded gate weights
    for m in model.modules():
        orig = inv.get(type(m))
        if orig is not None:
            m.__class__ = orig
    if isinstance(getattr(model, "loss_function", None), _LossDispatch):
        model.loss_function = model.loss_function.reference
    model.__dict__.pop("forward", None)  # the instance-level fused forward, if installed
    if "_tamd_disable_compile_was" in model.__dict__ and getattr(model, "generation_config", None) is not None:
        model.generation_config.disable_compile = model.__dict__.pop("_tamd_disable_compile_was")
    if "_tamd_experts_was" in model.__dict__:
        model.set_experts_implementation(model.__dict__.pop("_tamd_experts_was"))
    from . import graph_stack

    graph_stack.detach(model)
    return model
