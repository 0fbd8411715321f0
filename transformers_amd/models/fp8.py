"""FP8 block-scaled linear layers on the MI355X kernels: `FP8Linear` of integrations/finegrained_fp8.py, the module the
DeepSeek-V3 / R1, Qwen3-FP8 and GLM-FP8 checkpoints load their dense projections into (e4m3 `weight`, one fp32
`weight_scale_inv` per 128 x 128 block).

The reference's forward quantises the activations per 128 values and calls a Triton kernel.  Here the activations stay
bf16 / fp16 (W8A16, include/tamd.h tamd_gemm_fp8w): a decode step streams the weight bytes once -- half the bytes of a bf16
projection, which is what such a step is bound by.  Up to 64 rows (a batch of sequences, a block of speculative tokens, a short
second turn) the same single launch streams the bytes through the matrix pipe, dequantising in registers; up to 1024 rows (a
prefill) one fused tile kernel keeps X in LDS and dequantises each weight byte once per workgroup, again in registers; more rows
dequantise row chunks in front of the GEMM kernels.
That is closer to the exact product than the reference's forward and NOT bit-identical to it.

Served: one-byte e4m3 weights, block_size (128, 128), activation_scheme "dynamic", fp32 scales, bf16 / fp16 inputs on the
kernels' backend, nothing requiring grad.  Anything else -- static activation scales, other block sizes, ue8m0 scales,
training -- calls the reference's forward and is counted (`transformers_amd.fallback_calls()`); it is never computed
differently without saying so.  FP8 experts (`FP8Experts`) are not touched."""
from __future__ import annotations

import torch
from transformers.integrations.finegrained_fp8 import FP8Linear

from .. import ops
from .common import _gpu, note_fallback


class TamdFP8Linear(FP8Linear):
    def _refusal(self, x):
        """None when the kernels serve this call, else the reason it is counted under."""
        w, s, b = self.weight, self.weight_scale_inv, self.bias
        if w.dtype != torch.float8_e4m3fn:
            return "not_e4m3"  # (a dequantised checkpoint: the reference's F.linear)
        if self.block_size is None or tuple(self.block_size) != (ops.FP8_BLOCK, ops.FP8_BLOCK):
            return "block_size"
        if self.activation_scheme != "dynamic":
            return "static_activation_scale"
        if s.dtype != torch.float32 or s.dim() != 2:
            return "scale_format"
        if not _gpu(x) or x.dtype not in (torch.bfloat16, torch.float16) or x.numel() == 0:
            return "input"
        if b is not None and b.dtype != x.dtype:
            return "bias_dtype"
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or s.requires_grad or (b is not None and b.requires_grad)):
            return "requires_grad"
        if not ops.linear_fp8w_supported(x.numel() // x.shape[-1], w.shape[0], w.shape[1]):
            return "shape"
        return None

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        reason = self._refusal(input)
        if reason is None:
            return torch.ops.tamd.linear_fp8w(input, self.weight, self.weight_scale_inv, self.bias)
        note_fallback(self, input, reason)
        return super().forward(input)


REPLACEMENTS = {FP8Linear: TamdFP8Linear}
