"""prime_amd.ops — hand-written gfx950 HIP kernels with autograd wrappers.

Kernel inventory: flash attention fwd/bwd, RMSNorm, RoPE,
SwiGLU, fused AdamW, DiLoCo outer Nesterov step, blockwise int8
quant/dequant, fused cross-entropy. GEMMs go through hipBLASLt via
torch.nn.functional.linear (library GEMMs; everything fused is ours).
"""
from .functional import (
    apply_rope,
    invalidate_wt_cache,
    set_linear_fp8,
    set_linear_tuned,
    set_direct_wgrad,
    direct_wgrad_enabled,
    tuned_linear,
    gateup_swiglu,
    qkv_rope,
    qkv_grad_pack,
    rope_packed_fwd,
    swiglu_bwd_t,
    attn_decode,
    attn_decode_ragged,
    decode_qkv_append,
    decode_ragged_split,
    DECODE_RAGGED_CHUNK,
    fused_add_rmsnorm,
    cross_entropy,
    dequant_int8,
    doc_starts,
    flash_attention,
    fused_adamw,
    grad_sqnorm,
    mfma_probe,
    nesterov_outer,
    pseudograd,
    quant_int8,
    rmsnorm,
    swiglu,
    QBLK,
)
from . import reference
from ._lib import have_lib
from .build import build, LIB_PATH

__all__ = [
    "apply_rope",
    "attn_decode",
    "attn_decode_ragged",
    "decode_qkv_append",
    "decode_ragged_split",
    "DECODE_RAGGED_CHUNK",
    "fused_add_rmsnorm",
    "cross_entropy",
    "dequant_int8",
    "doc_starts",
    "flash_attention",
    "fused_adamw",
    "grad_sqnorm",
    "mfma_probe",
    "nesterov_outer",
    "pseudograd",
    "quant_int8",
    "rmsnorm",
    "swiglu",
    "QBLK",
    "reference",
    "have_lib",
    "build",
    "LIB_PATH",
]
