"""`experts_implementation="tamd"`: the experts of a gated SiLU mixture-of-experts block on the MI355X kernels, behind the
reference's ExpertsInterface.

Boundary: `ALL_EXPERTS_FUNCTIONS` (src/transformers/integrations/moe.py, `ExpertsInterface`) maps
`config._experts_implementation` to a function that `@use_experts_implementation` calls in place of the experts module's
own forward; a registered key is accepted by `from_pretrained(..., experts_implementation=KEY)` and
`model.set_experts_implementation(KEY)` (modeling_utils.py `get_correct_experts_implementation`).  The callee signature is
the one of `grouped_mm_experts_forward`:

    fn(self, hidden_states [T, H], top_k_index [T, k] int64, top_k_weights [T, k]) -> [T, H]

with `self.gate_up_proj` [E, 2I, H] (gate rows, then up rows) and `self.down_proj` [E, H, I] (MixtralExperts,
models/mixtral/modeling_mixtral.py).  What the kernels take runs as ONE dispatcher op, `torch.ops.tamd.moe_experts`
(routing plan, gather, gate|up product with the SiLU*up way out, down product, weighted combine; the backward through the same
plan) -- no host synchronisation, deterministic, no atomics.  A decode-sized call (up to `ops.MOE_GEMV_MAX_TOKENS` tokens,
nothing to differentiate: the steps of `generate()` after the prefill) runs instead on `torch.ops.tamd.moe_experts_decode`, the
weight-streaming kernels of csrc/gemv_moe.inc, which read the weights of the chosen experts once and build no plan
(`decode_call_count()` counts those calls; TAMD_MOE_GEMV=0 in the environment keeps every call on the routed GEMM).
Everything else calls the module's ORIGINAL forward and is counted
(`transformers_amd.fallback_calls()`): it is never approximated.
"""
from __future__ import annotations

import torch

from . import ops
from .models.common import _gpu, note_fallback

EXPERTS_KEY = "tamd"
MAX_EXPERTS = 256

_calls = 0
_registered = False


def call_count(reset: bool = False) -> int:
    """Calls of `tamd_experts_forward` that ran on the kernels since the last reset."""
    global _calls
    n = _calls
    if reset:
        _calls = 0
    return n


def decode_call_count(reset: bool = False) -> int:
    """Of those calls (and of direct `ops.moe_experts` calls), the ones that took the decode op
    `torch.ops.tamd.moe_experts_decode` since the last reset."""
    return ops.moe_decode_call_count(reset)


_router_calls = 0


def router_call_count(reset: bool = False) -> int:
    """Calls of the replacement routers (models/moe.py) that ran on the kernels (gate product + `ops.moe_router`) since the
    last reset."""
    global _router_calls
    n = _router_calls
    if reset:
        _router_calls = 0
    return n


def _note_router_call() -> None:
    global _router_calls
    _router_calls += 1


def _refusal(self, hidden_states, top_k_index, top_k_weights):
    """Why this call cannot run on the kernels (None: it can)."""
    from transformers.integrations.moe import _default_apply_gate

    if not getattr(self, "has_gate", False):
        return "no_gate"
    if getattr(self, "has_bias", False):
        return "bias"
    if getattr(self, "is_transposed", False):
        return "transposed"
    if not getattr(self, "is_concatenated", True):
        return "interleaved"
    if getattr(type(self), "_apply_gate", _default_apply_gate) is not _default_apply_gate:
        return "custom_gate"
    act = getattr(self, "act_fn", None)
    if not (isinstance(act, torch.nn.SiLU) or type(act).__name__ in ("SiLUActivation", "SiLU")
            or act is torch.nn.functional.silu):
        return "activation"
    gu, dn = getattr(self, "gate_up_proj", None), getattr(self, "down_proj", None)
    if not (torch.is_tensor(gu) and torch.is_tensor(dn) and gu.dim() == 3 and dn.dim() == 3):
        return "weights"
    if hidden_states.dtype not in (torch.bfloat16, torch.float16) or gu.dtype != hidden_states.dtype or dn.dtype != gu.dtype:
        return "dtype"
    e, two_i, h = gu.shape
    if (hidden_states.dim() != 2 or hidden_states.shape[1] != h or tuple(dn.shape) != (e, h, two_i // 2) or two_i % 2
            or h % 64 or (two_i // 2) % 8 or e > MAX_EXPERTS or hidden_states.shape[0] == 0):
        return "shape"
    if top_k_index.dim() != 2 or top_k_index.shape[0] != hidden_states.shape[0] or top_k_weights.shape != top_k_index.shape:
        return "shape"
    if not (_gpu(hidden_states) and hidden_states.device == gu.device == dn.device == top_k_index.device):
        return "device"
    return None


def tamd_experts_forward(self, hidden_states, top_k_index, top_k_weights):
    """The experts function registered as "tamd" (signature of integrations/moe.py grouped_mm_experts_forward)."""
    global _calls
    why = _refusal(self, hidden_states, top_k_index, top_k_weights)
    if why is not None:
        note_fallback(self, hidden_states, why)
        return type(self).forward.__wrapped__(self, hidden_states, top_k_index, top_k_weights)  # the module's own forward
    w = top_k_weights
    if w.dtype not in (torch.float32, hidden_states.dtype):
        w = w.to(hidden_states.dtype)
    _calls += 1
    return ops.moe_experts(hidden_states, top_k_index.to(torch.int64), w, self.gate_up_proj, self.down_proj)


def register() -> None:
    """Register the key with the reference's experts registry (idempotent)."""
    global _registered
    if _registered:
        return
    from transformers.integrations.moe import ALL_EXPERTS_FUNCTIONS

    ALL_EXPERTS_FUNCTIONS.register(EXPERTS_KEY, tamd_experts_forward)
    _registered = True
