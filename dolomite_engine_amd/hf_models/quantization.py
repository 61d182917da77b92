"""fp8 (e4m3) weight-only linears for inference (W8A16).

A decode step streams every linear's whole weight from HBM for a handful of
rows. quantize_linears_fp8 stores the four linears of each transformer block
as e4m3 with one fp32 scale per output channel, and ops.fp8_linear reads them
as such in its HIP skinny-GEMM kernel (csrc/fp8_linear.hip) whenever a call
has at most 64 rows: the decode steps and short extend steps. Calls of up to
2048 rows (batched decode, chunked prefill) read them as fp8 in its tiled GEMM
kernel (csrc/fp8_gemm.hip); longer ones (the large prefill) take
ops.fp8_linear's dequantised route."""

import torch
import torch.nn as nn

from ..ops import fp8_linear, quantize_weight_e4m3
from .modeling import GPTDolomiteBlock, ParameterizedLinear

_BLOCK_LINEARS = (("attn", "c_attn"), ("attn", "c_proj"), ("mlp", "c_fc"), ("mlp", "c_proj"))


class Fp8Linear(nn.Module):
    """A linear with an e4m3 weight: buffers weight_q (N, K) e4m3,
    weight_scale (N,) fp32 and bias (N,) in the model dtype or None;
    y = x @ (weight_q * weight_scale[:, None])^T + bias. Inference only."""

    def __init__(self, weight_q, weight_scale, bias=None):
        super().__init__()
        self.out_features, self.in_features = weight_q.shape
        self.register_buffer("weight_q", weight_q)
        self.register_buffer("weight_scale", weight_scale)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, linear: nn.Linear) -> "Fp8Linear":
        with torch.no_grad():
            wq, scale = quantize_weight_e4m3(linear.weight.detach())
            bias = None if linear.bias is None else linear.bias.detach().clone()
        return cls(wq, scale, bias)

    def forward(self, x):
        # ops.fp8_linear raises under autograd for inputs that require grad
        return fp8_linear(x, self.weight_q, self.weight_scale, self.bias)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


def quantize_linears_fp8(model):
    """Swap, in place, c_attn / c_proj of the attention and c_fc / c_proj of
    the MLP of every GPTDolomiteBlock of `model` for Fp8Linear, freeing their
    bf16 weights, and return the model. The embedding and the LM head (which
    may be tied to it) stay as they are, as do the experts of the MoE family.
    The model must be in eval mode and not padding-free (the KV-cache paths
    that decode run on the dense model). The state dict of the result holds the
    Fp8Linear buffers: quantise after loading a checkpoint, not before."""
    if model.training:
        raise RuntimeError("quantize_linears_fp8: the model is in training mode; call model.eval() first "
                           "(fp8 linears are inference only)")
    if getattr(model, "_use_padding_free_transformer", False):
        raise RuntimeError("quantize_linears_fp8: a padding-free model has no KV cache and no decode step; "
                           "build the model without use_padding_free_transformer")
    for block in model.modules():
        if not isinstance(block, GPTDolomiteBlock):
            continue
        for parent_name, name in _BLOCK_LINEARS:
            parent = getattr(block, parent_name)
            linear = getattr(parent, name)
            if isinstance(linear, ParameterizedLinear):
                setattr(parent, name, Fp8Linear.from_linear(linear))
    return model
