"""The routers of the sparse mixture-of-experts blocks on the MI355X kernels.

Reference: MixtralTopKRouter.forward (models/mixtral/modeling_mixtral.py), Qwen2MoeTopKRouter / Qwen3MoeTopKRouter /
OlmoeTopKRouter.forward (models/qwen2_moe, qwen3_moe, olmoe): `F.linear(hidden, weight)`, `softmax(dtype=float)`, `topk`,
`sum`, `div_`, `.to()` -- six to eight small launches per layer and call.  Here: the gate product on `ops.linear` (the
weight-streaming kernel up to 16 tokens, the tile kernels above) and ONE launch of `ops.moe_router` (csrc/moe_router.inc) for
everything behind it, forward and backward.  The triple returned has the reference's dtypes: Mixtral's scores are fp32 and
always renormalised, the other three round them to the logits' dtype and honour `norm_topk_prob`.

An expert count that is not a multiple of 8 (Qwen1.5-MoE: 60) runs the product over the gate weight zero-padded to the next
multiple of 8 rows -- cached for inference, a differentiable pad when the weight needs a gradient -- and the router kernel
reads the [:, :E] part of that product through its row stride.

What the kernels do not take (fp32 modules, CPU tensors, more than 256 experts, top_k > 16, a hidden size that is not a
multiple of 8, a subclass that overrides `forward`) calls the reference's forward -- the subclass's own -- and is counted
(`transformers_amd.fallback_calls()`); it is never approximated.

The sigmoid, group-limited routers (DeepseekV3TopkRouter.forward, models/deepseek_v3/modeling_deepseek_v3.py:144-169, and
every class of the reference whose `forward` is that text: GROUPED below) run `ops.moe_gate_logits` -- the gate product with
its fp32 accumulators kept, no fp32 copy of the weight -- and ONE launch of `ops.moe_router_grouped` in place of close to
twenty.  They return the reference's triple: fp32 logits, fp32 weights, int64 indices; the pairs come ordered by sigmoid + bias
descending where the reference's `topk(sorted=False)` leaves the order open.
Routers of another form (top-k before softmax, MiniMax-M2's, nn.Linear subclasses) are not in the table and stay the
reference's.
"""
from __future__ import annotations

import importlib

import torch
import torch.nn.functional as F
from transformers.models.mixtral.modeling_mixtral import MixtralTopKRouter
from transformers.models.olmoe.modeling_olmoe import OlmoeTopKRouter
from transformers.models.qwen2_moe.modeling_qwen2_moe import Qwen2MoeTopKRouter
from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeTopKRouter

from .. import experts, ops
from .common import TamdLinear, _gpu, note_fallback


def _refusal(self, hidden_states):
    """Why this call cannot run on the kernels (None: it can)."""
    w = self.weight
    if not torch.is_tensor(hidden_states) or not _gpu(hidden_states) or hidden_states.device != w.device:
        return "device"
    if hidden_states.dtype not in (torch.bfloat16, torch.float16) or w.dtype != hidden_states.dtype:
        return "dtype"
    e, h = w.shape
    if e > experts.MAX_EXPERTS:
        return "experts"
    if self.top_k > ops.ROUTER_MAX_TOP_K or self.top_k > e or self.top_k < 1:
        return "top_k"
    if h % 8 or hidden_states.shape[-1] != h or hidden_states.numel() == 0:
        return "shape"
    return None


def _padded_weight(self):
    """The gate weight with its rows zero-padded to a multiple of 8 (what the MFMA GEMM's row stores take)."""
    w = self.weight
    e, h = w.shape
    e_pad = -(-e // 8) * 8
    if torch.is_grad_enabled() and w.requires_grad:
        return F.pad(w, (0, 0, 0, e_pad - e))  # differentiable: the gradient of the first E rows reaches the parameter
    key = (w.data_ptr(), w._version, w.dtype, w.device)
    cached = self.__dict__.get("_tamd_padded_gate")
    if cached is None or cached[0] != key:
        buf = torch.zeros(e_pad, h, dtype=w.dtype, device=w.device)
        buf[:e].copy_(w.detach())
        cached = (key, buf)
        self.__dict__["_tamd_padded_gate"] = cached
    return cached[1]


def _forward(self, reference, hidden_states, norm: bool, scores_fp32: bool):
    why = _refusal(self, hidden_states)
    if why is not None:
        note_fallback(self, hidden_states, why)
        return reference.forward(self, hidden_states)
    x = hidden_states.reshape(-1, self.hidden_dim)
    e = self.weight.shape[0]
    if e % 8 == 0:
        router_logits = ops.linear(x, self.weight)
    else:
        router_logits = ops.linear(x, _padded_weight(self))[:, :e]
    scores, indices = ops.moe_router(router_logits, self.top_k, norm, scores_fp32)
    experts._note_router_call()
    return router_logits, scores, indices


def _replacement(reference, mixtral: bool):
    """The subclass of `reference` (no new parameters) whose forward runs on the kernels."""
    if mixtral:  # fp32 scores, always renormalised
        def forward(self, hidden_states):
            return _forward(self, reference, hidden_states, True, True)
    else:        # scores in the logits' dtype, `norm_topk_prob`
        def forward(self, hidden_states):
            return _forward(self, reference, hidden_states, bool(self.norm_topk_prob), False)
    return type("Tamd" + reference.__name__, (reference,), {"forward": forward, "__module__": __name__})


TamdMixtralTopKRouter = _replacement(MixtralTopKRouter, True)
TamdQwen2MoeTopKRouter = _replacement(Qwen2MoeTopKRouter, False)
TamdQwen3MoeTopKRouter = _replacement(Qwen3MoeTopKRouter, False)
TamdOlmoeTopKRouter = _replacement(OlmoeTopKRouter, False)

REPLACEMENTS = {MixtralTopKRouter: TamdMixtralTopKRouter, Qwen2MoeTopKRouter: TamdQwen2MoeTopKRouter,
                Qwen3MoeTopKRouter: TamdQwen3MoeTopKRouter, OlmoeTopKRouter: TamdOlmoeTopKRouter}


# ---- the sigmoid, group-limited routers ------------------------------------------------------------------------------
# Every router class of the reference whose `forward` source is textually DeepseekV3TopkRouter.forward
# (tests/test_moe_router_group_models.py asserts the identity for each class of the table, so an upgrade of the reference that
# changes one of them fails loudly).  A family the installed reference lacks is left out.
GROUPED = (("deepseek_v3", "DeepseekV3TopkRouter"), ("deepseek_v32", "DeepseekV32TopkRouter"), ("glm4_moe", "Glm4MoeTopkRouter"),
           ("glm4_moe_lite", "Glm4MoeLiteTopkRouter"), ("glm4v_moe", "Glm4vMoeTextTopkRouter"), ("glm_moe_dsa", "GlmMoeDsaTopkRouter"),
           ("dots1", "Dots1TopkRouter"), ("solar_open", "SolarOpenTopkRouter"), ("exaone_moe", "ExaoneMoeTopkRouter"),
           ("axk1", "AXK1TopkRouter"), ("mimo_v2_flash", "MiMoV2FlashTopkRouter"), ("nemotron_h", "NemotronHTopkRouter"))


def _grouped_refusal(self, hidden_states):
    """Why this call cannot run on the kernels (None: it can): the bounds of include/tamd.h tamd_moe_gate_f32 /
    tamd_moe_router_group_fwd."""
    w = self.weight
    if not torch.is_tensor(hidden_states) or not _gpu(hidden_states) or hidden_states.device != w.device:
        return "device"
    if hidden_states.dtype not in (torch.bfloat16, torch.float16) or w.dtype != hidden_states.dtype:
        return "dtype"
    e, h = w.shape
    if e > experts.MAX_EXPERTS or e % 8:
        return "experts"
    ng, tg = self.num_group, self.topk_group
    if not (1 <= ng <= ops.ROUTER_MAX_GROUPS and e % ng == 0 and 1 <= tg <= ng and (ng == 1 or e // ng >= 2)):
        return "groups"
    if not 1 <= self.top_k <= min(ops.ROUTER_MAX_TOP_K, tg * (e // ng)):
        return "top_k"
    if h % ops.GATE_HIDDEN_MULTIPLE or hidden_states.shape[-1] != h or hidden_states.numel() == 0 or self.num_experts != e:
        return "shape"
    return None


def _fp32_bias(self):
    """`e_score_correction_bias` as the kernel takes it: fp32.  `model.bfloat16()` turns the buffer into bf16 (only
    `from_pretrained` keeps it fp32); bf16 -> fp32 is exact, and the converted copy is cached like the padded gate weight."""
    b = self.e_score_correction_bias
    if b.dtype == torch.float32:
        return b
    key = (b.data_ptr(), b._version, b.dtype, b.device)
    cached = self.__dict__.get("_tamd_fp32_bias")
    if cached is None or cached[0] != key:
        cached = (key, b.detach().float())
        self.__dict__["_tamd_fp32_bias"] = cached
    return cached[1]


def _grouped_forward(self, reference, hidden_states):
    why = _grouped_refusal(self, hidden_states)
    if why is not None:
        note_fallback(self, hidden_states, why)
        return reference.forward(self, hidden_states)
    x = hidden_states.reshape(-1, self.hidden_dim)
    router_logits = ops.moe_gate_logits(x, self.weight)
    weights, indices = ops.moe_router_grouped(router_logits, _fp32_bias(self), self.top_k, self.num_group, self.topk_group,
                                              bool(self.norm_topk_prob), float(self.routed_scaling_factor))
    experts._note_router_call()
    return router_logits, weights, indices


def _grouped_replacement(reference):
    def forward(self, hidden_states):
        return _grouped_forward(self, reference, hidden_states)
    return type("Tamd" + reference.__name__, (reference,), {"forward": forward, "__module__": __name__})


GROUPED_REPLACEMENTS = {}
for _family, _name in GROUPED:
    try:
        _cls = getattr(importlib.import_module(f"transformers.models.{_family}.modeling_{_family}"), _name)
    except (ImportError, AttributeError):
        continue
    GROUPED_REPLACEMENTS[_cls] = globals()["Tamd" + _name] = _grouped_replacement(_cls)
REPLACEMENTS.update(GROUPED_REPLACEMENTS)


class TamdSharedExpertGate(TamdLinear):
    """Qwen2MoeSparseMoeBlock.shared_expert_gate, nn.Linear(hidden, 1, bias=False) (models/qwen2_moe/modeling_qwen2_moe.py: the
    sigmoid gate of the shared expert): one output row, which the GEMM's row stores do not take -- the product runs over the
    weight zero-padded to 8 rows, as a router's does, and the first column is returned.  `accelerate` installs it on the
    blocks whose router it swaps; anything else it is handed goes the way of TamdLinear."""

    def forward(self, x):
        w = self.weight
        if (self.bias is None and w.shape[0] % 8 and _gpu(x) and x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype
                and x.numel() > 0 and w.shape[1] % 8 == 0 and x.device == w.device):
            return ops.linear(x, _padded_weight(self))[..., :w.shape[0]]
        return super().forward(x)


# A subclass of one of the router classes is not in the exact-class table.  One that keeps the reference's `forward` gets
# the kernels like its parent; one that overrides `forward` computes something this package does not know: its own forward
# runs, counted under "subclass_forward".  Either way the module becomes a generated subclass of ITS class, which remembers
# the class it replaced for `revert`.
def _subclass_replacement(cls):
    reference = next(r for r in cls.__mro__ if r in REPLACEMENTS)
    if cls.forward is reference.forward:
        body = REPLACEMENTS[reference].forward
    else:
        def body(self, hidden_states):
            note_fallback(self, hidden_states, "subclass_forward")
            return cls.forward(self, hidden_states)
    return type("Tamd" + cls.__name__, (cls,), {"forward": body, "__module__": __name__, "_tamd_original": cls})


_SUBCLASSES: dict = {}


def swap_router_subclasses(model) -> int:
    """`accelerate`: routers whose class is a strict subclass of a class in REPLACEMENTS."""
    n = 0
    for m in model.modules():
        cls = type(m)
        if cls in REPLACEMENTS or cls in REPLACEMENTS.values() or "_tamd_original" in cls.__dict__:
            continue
        if isinstance(m, tuple(REPLACEMENTS)):
            if cls not in _SUBCLASSES:
                _SUBCLASSES[cls] = _subclass_replacement(cls)
            m.__class__ = _SUBCLASSES[cls]
            n += 1
    return n


def restore(model) -> None:
    """`revert`: the generated subclasses back to their classes, the shared-expert gates back to nn.Linear, the padded gate
    weights dropped."""
    for m in model.modules():
        orig = type(m).__dict__.get("_tamd_original")
        if orig is not None:
            m.__class__ = orig
        elif type(m) is TamdSharedExpertGate:
            m.__class__ = torch.nn.Linear
        m.__dict__.pop("_tamd_padded_gate", None)
        m.__dict__.pop("_tamd_fp32_bias", None)


def swap_shared_expert_gates(model) -> int:
    """`accelerate`: the shared-expert gates of the blocks whose routers were swapped."""
    n = 0
    for m in model.modules():
        g = getattr(m, "shared_expert_gate", None)
        if type(g) is TamdLinear and isinstance(getattr(m, "gate", None), tuple(REPLACEMENTS.values())):
            g.__class__ = TamdSharedExpertGate
            n += 1
    return n
