"""Hot-op surface of the MI355X engine (see include/dolomite_hip.h)."""

from .functional import (
    MOE_DECODE_MAX_TOKENS,
    QKVLayout,
    adamw_step_flat,
    attention_dropout_keep_mask,
    decode_attention,
    decode_num_splits,
    draw_attention_dropout_seed,
    extend_attention,
    extend_num_splits,
    fp8_gemm_num_splits,
    fp8_linear,
    fp8_linear_num_splits,
    fused_cross_entropy,
    fused_layernorm,
    fused_rmsnorm,
    glu_activation,
    grouped_expert_gemm,
    kv_cache_append,
    moe_decode_mlp,
    moe_route,
    moe_route_topk,
    quantize_kv_e4m3,
    quantize_weight_e4m3,
    rope_packed_qkv,
    span_attention,
    varlen_attention,
)
from .hip import is_available as hip_extension_available
from .hip import so_path as hip_so_path
