"""Autograd-wrapped fused ops.

Dispatch rule: CUDA tensors run the hand-written gfx950 HIP kernels
(mandatory — no silent eager fallback on GPU); CPU tensors run the fp32
PyTorch reference (prime_amd/ops/reference.py) so the gloo plumbing config
works without a GPU.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import torch

from . import reference as ref
from ._lib import check, lib, ptr, stream_of

# reductions that cross thread blocks store one partial per block and are
# summed here in a fixed order, never with float atomics, so a step's
# results are bit-identical from run to run
_DW_ROWS = 1024  # max blocks (= partial dw rows) of the norm backwards


def _is_hip(t: torch.Tensor) -> bool:
    return t.is_cuda


# --------------------------------------------------------------- RMSNorm
class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, eps: float):
        if not _is_hip(x):
            ctx.save_for_backward(x, w)
            ctx.eps = eps
            return ref.rmsnorm(x, w, eps)
        x = x.contiguous()
        shp = x.shape
        D = shp[-1]
        if D % 8 != 0:
            raise NotImplementedError(
                f"rmsnorm kernel needs hidden dim % 8 == 0 (got {D}): the "
                "bf16x8 vector loads require 16 B rows"
            )
        R = x.numel() // D
        y = torch.empty_like(x)
        rstd = torch.empty(R, device=x.device, dtype=torch.float32)
        check(
            lib().prime_rmsnorm_fwd(stream_of(x), ptr(x), ptr(w), ptr(y), ptr(rstd), R, D, eps),
            "rmsnorm_fwd",
        )
        ctx.save_for_backward(x, w, rstd)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        saved = ctx.saved_tensors  # read once: ckpt unpack hooks fire per access
        if len(saved) == 2:  # CPU path
            x, w = saved
            x = x.detach().float().requires_grad_(True)
            w2 = w.detach().float().requires_grad_(True)
            with torch.enable_grad():
                y = ref.rmsnorm(x, w2, ctx.eps)
            gx, gw = torch.autograd.grad(y, [x, w2], dy.float())
            return gx.to(dy.dtype), gw.to(w.dtype), None
        x, w, rstd = saved
        dy = dy.contiguous()
        D = x.shape[-1]
        R = x.numel() // D
        dx = torch.empty_like(x)
        # per-block partial dw rows, summed in a fixed order (deterministic)
        G = max(1, min(R, _DW_ROWS))
        dw = torch.empty(G, D, device=x.device, dtype=torch.float32)
        check(
            lib().prime_rmsnorm_bwd(
                stream_of(x), ptr(dy), ptr(x), ptr(w), ptr(rstd), ptr(dx), ptr(dw), R, D, G, ctx.eps
            ),
            "rmsnorm_bwd",
        )
        return dx, dw.sum(0).to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    return _RMSNorm.apply(x, w, eps)


# ------------------------------------------------------------------ RoPE
class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, pos_offset: int, pos_dev=None):
        if not _is_hip(x):
            ctx.cpu = (cos, sin, pos_offset)
            return ref.apply_rope(x, cos, sin, pos_offset)
        ctx.cpu = None
        B, S, H, D = x.shape
        if pos_dev is None and not x.is_contiguous() and _rope_view_ok(x):
            # q / k view of a packed qkv buffer: rotate straight out of it
            # (a dense copy first is a whole extra read + write)
            y = rope_packed_fwd(x, cos, sin, pos_offset)
            ctx.save_for_backward(cos, sin)
            ctx.meta = (B, S, H, D, pos_offset)
            return y
        x = x.contiguous()
        y = torch.empty_like(x)
        check(
            lib().prime_rope(
                stream_of(x), ptr(x), ptr(y), ptr(cos), ptr(sin), B * S * H,
                H, S, D, 0, pos_offset, ptr(pos_dev),
            ),
            "rope_fwd",
        )
        ctx.save_for_backward(cos, sin)
        ctx.meta = (B, S, H, D, pos_offset)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.cpu is not None:
            cos, sin, off = ctx.cpu
            # inverse rotation
            return ref.apply_rope(dy, cos, -sin, off), None, None, None, None
        cos, sin = ctx.saved_tensors
        B, S, H, D, off = ctx.meta
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(
            lib().prime_rope(
                stream_of(dy), ptr(dy), ptr(dx), ptr(cos), ptr(sin), B * S * H,
                H, S, D, 1, off, ptr(None),
            ),
            "rope_bwd",
        )
        return dx, None, None, None, None


def apply_rope(x, cos, sin, pos_offset: int = 0, pos_dev=None):
    """x: [B,S,H,D] bf16; cos/sin: [S_max, D/2] fp32 tables. `pos_dev`
    (optional int32 device scalar) overrides pos_offset at kernel time
    (hipGraph decode)."""
    return _Rope.apply(x, cos, sin, pos_offset, pos_dev)


def _rope_view_ok(x: torch.Tensor) -> bool:
    """[B,S,H,D] view the stride-aware RoPE kernel can read: heads packed
    inside each token row, one uniform token stride, 8 B aligned rows."""
    B, S, H, D = x.shape
    sb, ss, sh, sd = x.stride()
    return (sd == 1 and sh == D and D % 8 == 0 and ss % 4 == 0
            and (B == 1 or sb == S * ss) and x.storage_offset() % 4 == 0)


def rope_packed_fwd(x, cos, sin, pos_offset: int = 0) -> torch.Tensor:
    """RoPE forward (no autograd) of a [B,S,H,D] view whose heads sit inside
    wider packed token rows (q or k inside the qkv GEMM output); returns a
    contiguous [B,S,H,D] tensor, bit-identical to rotating a dense copy."""
    if not _rope_view_ok(x):
        raise NotImplementedError(
            f"rope_packed_fwd: unsupported view (shape {tuple(x.shape)}, "
            f"strides {x.stride()})")
    B, S, H, D = x.shape
    y = torch.empty(B, S, H, D, device=x.device, dtype=x.dtype)
    check(
        lib().prime_rope_strided(
            stream_of(x), ptr(x), ptr(y), ptr(cos), ptr(sin), B * S * H,
            H, S, D, x.stride(1), 0, pos_offset,
        ),
        "rope_strided",
    )
    return y


def qkv_grad_pack(dq, dk, dv, cos, sin, pos_offset: int = 0):
    """Backward of {split qkv, RoPE(q), RoPE(k)} in one pass: dq [B,S,H,D]
    and dk [B,S,Hkv,D] are gradients of the rotated q/k, dv [B,S,Hkv,D] of
    v. Returns (dqkv [M,C], dqkv^T [C,M]) with M = B*S, C = (H+2Hkv)*D."""
    B, S, H, D = dq.shape
    Hkv = dk.shape[2]
    M = B * S
    if D not in (64, 128) or M % 64 != 0:
        raise NotImplementedError(
            f"qkv_grad_pack needs head_dim in {{64, 128}} and tokens % 64 == 0 "
            f"(got head_dim={D}, tokens={M})")
    dq, dk, dv = dq.contiguous(), dk.contiguous(), dv.contiguous()
    C = (H + 2 * Hkv) * D
    dqkv = torch.empty(M, C, device=dq.device, dtype=dq.dtype)
    dqkvt = torch.empty(C, M, device=dq.device, dtype=dq.dtype)
    check(
        lib().prime_qkv_grad_pack(
            stream_of(dq), ptr(dq), ptr(dk), ptr(dv), ptr(dqkv), ptr(dqkvt),
            ptr(cos), ptr(sin), M, H, Hkv, S, D, pos_offset,
        ),
        "qkv_grad_pack",
    )
    return dqkv, dqkvt


# ---------------------------------------------------------------- SwiGLU
class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        if not _is_hip(gu):
            ctx.save_for_backward(gu)
            return ref.swiglu(gu)
        gu = gu.contiguous()
        I = gu.shape[-1] // 2
        if I % 8 != 0:
            raise NotImplementedError(
                f"swiglu kernel needs intermediate dim % 8 == 0 (got {I})"
            )
        R = gu.numel() // (2 * I)
        out = torch.empty(*gu.shape[:-1], I, device=gu.device, dtype=gu.dtype)
        check(lib().prime_swiglu_fwd(stream_of(gu), ptr(gu), ptr(out), R, I), "swiglu_fwd")
        ctx.save_for_backward(gu)
        return out

    @staticmethod
    def backward(ctx, dout):
        (gu,) = ctx.saved_tensors
        if not _is_hip(gu):
            g = gu.detach().float().requires_grad_(True)
            with torch.enable_grad():
                y = ref.swiglu(g)
            (gx,) = torch.autograd.grad(y, [g], dout.float())
            return gx.to(gu.dtype)
        dout = dout.contiguous()
        I = gu.shape[-1] // 2
        R = gu.numel() // (2 * I)
        dgu = torch.empty_like(gu)
        check(lib().prime_swiglu_bwd(stream_of(gu), ptr(dout), ptr(gu), ptr(dgu), R, I), "swiglu_bwd")
        return dgu


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    """gu: [..., 2I] (gate ‖ up) -> [..., I] = silu(gate) * up."""
    return _SwiGLU.apply(gu)


def swiglu_bwd_t(dout: torch.Tensor, gu: torch.Tensor):
    """SwiGLU backward (no autograd) that also returns dgu^T for the NN dW
    GEMM: (dgu [R,2I], dgu^T [2I,R]). One fused pass when R and I tile by
    64; otherwise the plain backward kernel plus a transpose."""
    gu = gu.contiguous()
    dout = dout.contiguous()
    I = gu.shape[-1] // 2
    R = gu.numel() // (2 * I)
    dgu = torch.empty_like(gu)
    if R % 64 == 0 and I % 64 == 0 and R > 0:
        dgut = torch.empty(2 * I, R, device=gu.device, dtype=gu.dtype)
        check(
            lib().prime_swiglu_bwd_t(stream_of(gu), ptr(dout), ptr(gu),
                                     ptr(dgu), ptr(dgut), R, I),
            "swiglu_bwd_t",
        )
        return dgu, dgut
    if I % 8 != 0:
        raise NotImplementedError(
            f"swiglu kernel needs intermediate dim % 8 == 0 (got {I})")
    check(lib().prime_swiglu_bwd(stream_of(gu), ptr(dout), ptr(gu), ptr(dgu), R, I),
          "swiglu_bwd")
    return dgu, dgu.view(R, 2 * I).t().contiguous()


# ------------------------------------------------------- flash attention
def transpose_bshd(x: torch.Tensor) -> torch.Tensor:
    """[B,S,H,D] (strided view ok) -> [B,H,D,S] contiguous, via the
    LDS-tiled transpose kernel (torch permute+contiguous is ~80 GB/s on
    this pattern)."""
    B, S, H, D = x.shape
    if not x.is_cuda or S % 64 != 0 or D % 64 != 0 or x.stride(3) != 1:
        return x.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(B, H, D, S, device=x.device, dtype=x.dtype)
    check(
        lib().prime_transpose_bshd(
            stream_of(x), ptr(x), ptr(out), B, S, H, D,
            x.stride(0), x.stride(1), x.stride(2),
        ),
        "transpose_bshd",
    )
    return out


def _bshd_ok(t: torch.Tensor) -> bool:
    """[B,S,H,D] view usable by the stride-aware kernels: last dim
    contiguous, every stride a multiple of 8 elements (16 B alignment)."""
    sb, ss, sh, sd = t.stride()
    return sd == 1 and sb % 8 == 0 and ss % 8 == 0 and sh % 8 == 0 \
        and t.storage_offset() % 8 == 0


def _check_flash_shape(S: int, D: int) -> None:
    if D not in (64, 128) or S % 64 != 0:
        raise NotImplementedError(
            f"flash attention kernels support head_dim in {{64, 128}} and "
            f"seq_len % 64 == 0 (got head_dim={D}, seq_len={S}); pad the "
            "sequence or pick a head_dim-compatible model config"
        )


def doc_starts(tokens: torch.Tensor, eos_id: int) -> torch.Tensor:
    """tokens [B,S] -> int32 [B,S]: index of the first token of the document
    each token belongs to. A token that follows an `eos_id` token starts a
    new document; the EOS itself belongs to the document it ends. Plain
    torch ops on the tokens' device, no host sync."""
    B, S = tokens.shape
    idx = torch.arange(S, device=tokens.device, dtype=torch.int32).expand(B, S)
    new_doc = torch.zeros(B, S, dtype=torch.bool, device=tokens.device)
    new_doc[:, 1:] = tokens[:, :-1] == eos_id
    return torch.where(new_doc, idx, torch.zeros_like(idx)).cummax(dim=1).values


def _doc_ends(doc_start: torch.Tensor) -> torch.Tensor:
    """Mirror of doc_start for the dK/dV kernel: exclusive end of each
    key's document (the next document's start, or S)."""
    B, S = doc_start.shape
    idx = torch.arange(S, device=doc_start.device, dtype=torch.int32).expand(B, S)
    cand = torch.where(doc_start == idx, idx, torch.full_like(idx, S))
    # first document start at or after j, then shift by one for "after j"
    nxt = cand.flip(1).cummin(dim=1).values.flip(1)
    return torch.cat([nxt[:, 1:], torch.full_like(idx[:, :1], S)], dim=1).contiguous()


_DOC_END_CACHE: list = [None, None, None]  # (weakref(doc_start), version, doc_end)


def _doc_ends_cached(doc_start: torch.Tensor) -> torch.Tensor:
    """One doc_start serves every layer of a micro-batch; derive its mirror
    once, not once per layer's backward."""
    import weakref

    ref_, ver, val = _DOC_END_CACHE
    if ref_ is not None and ref_() is doc_start and ver == doc_start._version:
        return val
    val = _doc_ends(doc_start)
    _DOC_END_CACHE[:] = [weakref.ref(doc_start), doc_start._version, val]
    return val


def _check_doc_start(doc_start, q, causal: bool) -> None:
    B, S = q.shape[0], q.shape[1]
    if not causal:
        raise ValueError("flash_attention: doc_start requires causal=True")
    if not isinstance(doc_start, torch.Tensor) or doc_start.dtype != torch.int32:
        raise TypeError(
            "flash_attention: doc_start must be an int32 tensor "
            f"(got {getattr(doc_start, 'dtype', type(doc_start))})")
    if tuple(doc_start.shape) != (B, S):
        raise ValueError(
            f"flash_attention: doc_start must have shape [B, S] = [{B}, {S}] "
            f"(got {list(doc_start.shape)})")
    if doc_start.device != q.device:
        raise ValueError(
            f"flash_attention: doc_start is on {doc_start.device}, q on {q.device}")


class _FlashAttention(torch.autograd.Function):
    """Stride-aware [B,S,H,D] domain: consumes q/k/v views of the packed
    qkv GEMM output directly (no transposes / .contiguous() on the hot
    path); only the genuinely-transposed operands (Vt/Kt/Qt/dOt, needed
    for contiguous MFMA B-fragments) are materialized."""

    @staticmethod
    def forward(ctx, q, k, v, causal: bool, scale: float, doc_start=None):
        B, S, H, D = q.shape
        _check_flash_shape(S, D)
        Hkv = k.shape[2]
        if not (_bshd_ok(q) and _bshd_ok(k) and _bshd_ok(v)):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if doc_start is not None:
            doc_start = doc_start.contiguous()
        vt = transpose_bshd(v)  # [B,Hkv,D,S]
        o = torch.empty(B, S, H, D, device=q.device, dtype=q.dtype)
        lse = torch.empty(B, S, H, device=q.device, dtype=torch.float32)
        check(
            lib().prime_flash_fwd(
                stream_of(q), ptr(q), ptr(k), ptr(vt), ptr(o), ptr(lse),
                B, H, Hkv, S, D, scale, int(causal),
                q.stride(0), q.stride(1), q.stride(2),
                k.stride(0), k.stride(1), k.stride(2), ptr(doc_start),
            ),
            "flash_fwd",
        )
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.meta = (causal, scale)
        ctx.doc_start = doc_start  # int mask, no gradient: not a saved tensor
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        causal, scale = ctx.meta
        doc_start = ctx.doc_start
        doc_end = _doc_ends_cached(doc_start) if doc_start is not None else None
        B, S, H, D = q.shape
        Hkv = k.shape[2]
        do = do.contiguous()
        delta = torch.empty(B * S * H, device=q.device, dtype=torch.float32)
        # rowc = {lse, delta} again in [B,H,S] order, for the dK/dV kernel
        rowc = torch.empty(2, B, H, S, device=q.device, dtype=torch.float32)
        # the same pass over dO also writes dO^T [B,H,D,S] for dK/dV
        dot = torch.empty(B, H, D, S, device=q.device, dtype=q.dtype)
        check(
            lib().prime_attn_delta_dot(stream_of(q), ptr(do), ptr(o), ptr(lse), ptr(delta),
                                       ptr(rowc), ptr(dot), B, S, H, D),
            "attn_delta_dot",
        )
        kt = transpose_bshd(k)  # [B,Hkv,D,S]
        dq = torch.empty(B, S, H, D, device=q.device, dtype=q.dtype)
        check(
            lib().prime_flash_bwd_dq(
                stream_of(q), ptr(q), ptr(k), ptr(v), ptr(kt), ptr(do),
                ptr(lse), ptr(delta), ptr(dq), B, H, Hkv, S, D, scale,
                int(causal),
                q.stride(0), q.stride(1), q.stride(2),
                k.stride(0), k.stride(1), k.stride(2),
                v.stride(0), v.stride(1), v.stride(2), ptr(doc_start),
            ),
            "flash_bwd_dq",
        )
        qt = transpose_bshd(q)   # [B,H,D,S]
        dk = torch.empty(B, S, Hkv, D, device=q.device, dtype=q.dtype)
        dv = torch.empty(B, S, Hkv, D, device=q.device, dtype=q.dtype)
        # the library picks the mode (see prime_flash_bwd_dkv_direct). Split:
        # the q loop is cut into `splits` slices spread across the grid, one
        # fp32 partial each. Direct: one block walks the same slices itself
        # and adds them up in the same order (same bits), parking the
        # running sum in a single slice of workspace — none for one slice.
        direct = bool(lib().prime_flash_bwd_dkv_direct(
            B, Hkv, S, D, int(causal), int(doc_end is not None)))
        env = os.environ.get("PRIME_AMD_DKV_SPLITS")
        if env:
            splits = max(1, min(int(env), S // 64))
        else:
            # measured on MI355X (10B shapes): S=2048 wants splits=2
            # (bench 14.6k at 2 vs 14.5k at 4 — workspace traffic), S=8192
            # wants 8 (12,690 vs 12,593 tok/s — causal trip imbalance
            # dominates at long context)
            splits = max(1, min(8, S // 1024, S // 64))
        ws_slices = (0 if splits == 1 else 1) if direct else splits
        ws = torch.empty(2, ws_slices, B, Hkv, S, D, device=q.device,
                         dtype=torch.float32) if ws_slices else None
        check(
            lib().prime_flash_bwd_dkv(
                stream_of(q), ptr(q), ptr(qt), ptr(k), ptr(v), ptr(do),
                ptr(dot), ptr(rowc), ptr(dk), ptr(dv),
                ptr(None if ws is None else ws[0]), ptr(None if ws is None else ws[1]), splits,
                B, H, Hkv, S, D, scale, int(causal),
                q.stride(0), q.stride(1), q.stride(2),
                k.stride(0), k.stride(1), k.stride(2),
                v.stride(0), v.stride(1), v.stride(2), ptr(doc_end),
            ),
            "flash_bwd_dkv",
        )
        return dq, dk, dv, None, None, None


def flash_attention(q, k, v, causal: bool = True, doc_start=None) -> torch.Tensor:
    """q: [B,S,H,D]; k,v: [B,S,Hkv,D] (GQA). Returns [B,S,H,D].

    doc_start: optional int32 [B,S] document mask for packed sequences
    (see `doc_starts`): query i sees key j iff doc_start[b,i] <= j <= i.
    One array per micro-batch, shared by all layers and heads."""
    if doc_start is not None:
        _check_doc_start(doc_start, q, causal)
    if not _is_hip(q):
        return ref.attention(q, k, v, causal, doc_start=doc_start)
    if doc_start is None:
        return _FlashAttention.apply(q, k, v, causal, q.shape[-1] ** -0.5)
    return _FlashAttention.apply(q, k, v, causal, q.shape[-1] ** -0.5, doc_start)


# --------------------------------------------------------- cross entropy
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index: int, need_grad: bool):
        # logits [R, V] bf16, targets [R] int32/int64. need_grad is decided
        # by the caller: Function.forward always runs under no_grad, so
        # torch.is_grad_enabled() here would be False even in training.
        R, V = logits.shape
        logits = logits.contiguous()
        t32 = targets.to(torch.int32).contiguous()
        loss = torch.empty(R, device=logits.device, dtype=torch.float32)
        # under no_grad (eval/perplexity) skip the [R,V] dlogits write —
        # at V=128k that is a full extra bf16 tensor per eval batch
        dlogits = torch.empty_like(logits) if need_grad else logits  # dummy ptr
        check(
            lib().prime_cross_entropy(
                stream_of(logits), ptr(logits), ptr(t32), ptr(loss), ptr(dlogits),
                R, V, 1.0, ignore_index, 1 if need_grad else 0,
            ),
            "cross_entropy",
        )
        n_valid = (targets != ignore_index).sum().clamp(min=1)
        if need_grad:
            ctx.save_for_backward(dlogits, n_valid)
        else:
            ctx.save_for_backward(torch.empty(0, device=logits.device,
                                              dtype=logits.dtype), n_valid)
        return loss.sum() / n_valid.float()

    @staticmethod
    def backward(ctx, grad_out):
        dlogits, n_valid = ctx.saved_tensors
        g = dlogits * (grad_out.float() / n_valid.float()).to(dlogits.dtype)
        return g, None, None, None


def cross_entropy(logits, targets, ignore_index: int = -100) -> torch.Tensor:
    """Fused CE: mean loss over non-ignored tokens; grad computed in-kernel."""
    if not _is_hip(logits):
        return ref.cross_entropy(logits, targets, ignore_index)
    need_grad = torch.is_grad_enabled() and logits.requires_grad
    return _CrossEntropy.apply(logits, targets, ignore_index, need_grad)


# ----------------------------------------------- layout-tuned linear
# Measured on MI355X (16384-token 10B shapes, fresh buffers): hipBLASLt's
# TN (dW) kernels run at ~1.0-1.2 PF and NN (dX) at ~1.3-1.4 PF while the
# NT family reaches ~1.45-1.6 PF. Re-expressing the backward GEMMs in
# faster layouts with cheap explicit transposes buys back most of the gap:
#   dX = dY @ (Wt)^T    with Wt = W^T cached per optimizer step  (NT)
#   dW = (dY^T) @ X     with dY^T via the LDS-tiled transpose    (NN)
_WT_EPOCH = 0
_WT_CACHE: dict = {}
_LINEAR_TUNED = False


def set_linear_tuned(on: bool) -> None:
    """Enable the transposed-weight dX path (Trainer: CUDA + stable param
    storage only — FSDP re-materializes weights into rotating pool buffers,
    which would alias the id()-keyed cache)."""
    global _LINEAR_TUNED
    _LINEAR_TUNED = bool(on)
    _WT_CACHE.clear()


def invalidate_wt_cache() -> None:
    """Weights changed in place (fused AdamW / outer step / load_flat_)."""
    global _WT_EPOCH
    _WT_EPOCH += 1
    _WT_CACHE.clear()
    _FP8_CACHE.clear()


def _wt_of(w: torch.Tensor):
    """Cached W^T [K,N] of a [N,K] weight; None when the shape doesn't
    tile for the transpose kernel. Keyed by (data_ptr, shape): id(w) is
    NOT stable — under activation checkpointing the saved-tensor unpack
    hands backward a fresh transient object per call, and recycled ids
    collided across different weights (caught by the 70B sizing run)."""
    N, K = w.shape
    if K % 128 or N % 64:
        return None
    key = (w.data_ptr(), N, K)
    hit = _WT_CACHE.get(key)
    if hit is not None and hit[0] == _WT_EPOCH:
        return hit[1]
    wt = transpose_bshd(w.view(1, N, K // 128, 128)).view(K, N)
    _WT_CACHE[key] = (_WT_EPOCH, wt)
    return wt


# Wgrad deferral (Megatron-style dW on a side stream, overlapping the
# backward's memory-bound kernels) was implemented and measured: the
# naive version collapsed throughput 3x — side-stream allocations split
# the caching allocator's pools at 157 GB live and every dW buffer
# forced cross-stream synchronization. Doing it right needs main-stream-
# allocated out= buffers for every intermediate (incl. an out= variant
# of the transpose kernel); parked as a documented negative in
# profiles/10b_1gpu_profile.md.
def _transpose_quant_fp8(x2: torch.Tensor, site: tuple, e5m2: bool = False):
    """[M, C] bf16 -> [C, M] fp8 in ONE pass (csrc/transpose.hip's fused
    variant): the wgrad operands x^T / dY^T are consumed only as fp8, so
    the bf16 transposed intermediate was pure HBM traffic. Falls back to
    transpose + fused quant on the bootstrap call (amax not seeded)."""
    M, C = x2.shape
    st = _FP8_ACT.get(site)
    # the one-pass variant measured 8% SLOWER end-to-end (10B fp8 bench
    # 20.1k vs 21.9k): its 8-byte fp8 stores halve the store width and
    # the per-element conversion sits in the store loop — the separate
    # LDS-tiled transpose + fused quant pair wins. Kept opt-in for
    # further tuning (PRIME_AMD_FUSED_TQ=1).
    import os

    fused_ok = os.environ.get("PRIME_AMD_FUSED_TQ", "0") == "1"
    if st is None or M % 64 or C % 128 or not fused_ok:
        xt = transpose_bshd(x2.view(1, M, C // 128, 128)).view(C, M)
        return _quant_act_fp8(xt, site, e5m2=e5m2)
    dt8 = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
    xt8 = torch.empty(C, M, device=x2.device, dtype=dt8)
    st["next"].zero_()
    check(
        lib().prime_transpose_fp8(
            stream_of(x2), ptr(x2), ptr(xt8), 1, M, C // 128, 128,
            x2.stride(0) * M, x2.stride(0), 128,
            ptr(st["amax"]), ptr(st["next"]), ptr(st["sinv"]), 1 if e5m2 else 0,
        ),
        "transpose_fp8",
    )
    st["amax"], st["next"] = st["next"], st["amax"]
    return xt8, st["sinv"]


# Direct wgrad: a FlatParamSpace makes p.grad a view of its flat gradient,
# so autograd's accumulate turns every dW into {GEMM writes a temporary;
# grad += temporary} on top of the per-step zero fill — three writes of a
# weight-sized tensor where one is needed. A space registers the grad view
# of each untied PrimeLinear weight here; while a slot is armed (between
# the space's zero_grad() and the weight's first gradient of the step) the
# dW GEMM writes straight into the view and backward hands autograd None.
# Later gradients in the same step (grad accumulation) go through autograd
# as before, so accumulated values do not change.
_DIRECT_WGRAD = False
# (data_ptr, N, K) -> [grad_view, armed, owner_ref, autograd_pending]
_WGRAD_SLOTS: dict = {}


def set_direct_wgrad(on: bool) -> None:
    """Let dW GEMMs write into registered flat-gradient views (Trainer:
    CUDA + FlatParamSpace; bare modules keep autograd's accumulate)."""
    global _DIRECT_WGRAD
    _DIRECT_WGRAD = bool(on)


def direct_wgrad_enabled() -> bool:
    return _DIRECT_WGRAD


def register_wgrad_slot(w: torch.Tensor, grad_view: torch.Tensor, owner):
    """Called by FlatParamSpace; `owner` is a weakref to the space. Returns
    the slot (the space arms/disarms it by setting slot[1]; slot[3] asks
    it to zero the view instead of arming at its next zero_grad())."""
    slot = [grad_view, False, owner, False]
    _WGRAD_SLOTS[(w.data_ptr(), *w.shape)] = slot
    return slot


def unregister_wgrad_slots(owner) -> None:
    for k in [k for k, s in _WGRAD_SLOTS.items() if s[2] is owner]:
        del _WGRAD_SLOTS[k]


def _wgrad_take(w: torch.Tensor):
    """The flat-gradient view to write w's dW into, if this is the first
    gradient of the step for a registered weight; else None."""
    if not _WGRAD_SLOTS:
        return None
    slot = _WGRAD_SLOTS.get((w.data_ptr(), *w.shape))
    if slot is None or not slot[1]:
        return None
    if slot[2]() is None:  # owning space is gone
        del _WGRAD_SLOTS[(w.data_ptr(), *w.shape)]
        return None
    slot[1] = False
    return slot[0]


def _wgrad_release(w: torch.Tensor) -> None:
    """w's gradient will reach its grad view through autograd's accumulate
    (a forward that does not lead to _compute_dw): give the view the zero
    it expects — now if the step has started, else at its zero_grad()."""
    if not _WGRAD_SLOTS:
        return
    out = _wgrad_take(w)
    if out is not None:
        out.zero_()
    elif torch.is_grad_enabled():
        slot = _WGRAD_SLOTS.get((w.data_ptr(), *w.shape))
        if slot is not None:
            slot[3] = True


def _compute_dw(x2, w, dy2, dyt=None):
    """dW = dY^T @ X. `dyt` is dY^T when the producer of dY already emitted
    it (fused swiglu / qkv-pack backward). Returns None when the GEMM wrote
    the registered flat-gradient view directly."""
    N, K = w.shape
    M = x2.shape[0]
    out = _wgrad_take(w)
    if out is not None and not (out.dtype == x2.dtype == dy2.dtype):
        out.zero_()  # mixed dtypes: leave the accumulate to autograd
        out = None
    if N % 128 == 0 and M % 64 == 0 and M >= 4096:
        if (_LINEAR_FP8_WGRAD and K % 128 == 0 and M % 16 == 0
                and x2.dtype == torch.bfloat16):
            xt8, xtinv = _transpose_quant_fp8(
                x2, ("xT", w.data_ptr(), *w.shape))
            dyt8, dytinv = _transpose_quant_fp8(
                dy2, ("dyT", w.data_ptr(), *w.shape), e5m2=True)
            g = torch._scaled_mm(xt8, dyt8.t(), scale_a=xtinv,
                                 scale_b=dytinv, out_dtype=x2.dtype)
            dw = transpose_bshd(g.view(1, K, N // 128, 128)).view(N, K)
            if out is not None:
                out.copy_(dw)
                return None
            return dw
        if dyt is None:
            dyt = transpose_bshd(dy2.view(1, M, N // 128, 128)).view(N, M)
        dw = torch.mm(dyt, x2, out=out)
    else:
        dw = torch.mm(dyt if dyt is not None else dy2.t(), x2, out=out)
    return None if out is not None else dw


def _linear_backward(x2, w, dy):
    """Shared layout-tuned backward for the bf16 and fp8-forward paths."""
    N, K = w.shape
    M = x2.shape[0]
    dy2 = dy.reshape(-1, N).contiguous()
    # dX as NT against the per-step transposed weight
    wt = _wt_of(w) if _LINEAR_TUNED else None
    if (_LINEAR_FP8_DGRAD and wt is not None and M % 16 == 0
            and dy2.dtype == torch.bfloat16):
        # fp8 dgrad: e5m2 gradients (grad dynamic range) x e4m3 weights.
        # Per-tensor delayed scaling here: hipBLASLt's rowwise _scaled_mm
        # path is only validated for e4m3 x e4m3 (the forward), and mixing
        # a rowwise scale_a with a scalar scale_b is rejected.
        dy8, dyinv = _quant_act_fp8(dy2, ("dy", w.data_ptr(), *w.shape),
                                    e5m2=True)
        wt8, wtinv = _w8_of(wt, skey=("wt", w.data_ptr(), *w.shape))
        dx = torch._scaled_mm(dy8, wt8.t(), scale_a=dyinv, scale_b=wtinv,
                              out_dtype=dy2.dtype)
    elif wt is not None:
        dx = torch.matmul(dy2, wt.t())
    else:
        dx = torch.matmul(dy2, w)
    # dW: NN-via-dY^T rewrite + the fp8 wgrad tier live in _compute_dw
    return dx.view(*dy.shape[:-1], K), _compute_dw(x2, w, dy2)


class _TunedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x2 = x.reshape(-1, x.shape[-1])
        y = torch.matmul(x2, w.t())
        ctx.save_for_backward(x2, w)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        return _linear_backward(x2, w, dy)


# ----------------------------------------------- fp8 forward (opt-in)
# hipBLASLt's OCP-e4m3 scaled GEMM measured 2449 TF/s vs 1372 bf16 on the
# 16k-token qkv shape (1.78x). Opt-in mixed mode: FORWARD linears compute
# in fp8 with per-tensor dynamic scaling (activations) and a per-step
# cached fp8 weight; master weights, gradients and the whole backward
# stay bf16/fp32. The headline bench contract stays bf16 - this mode is
# measured and reported separately (bench.py --fp8).
_FP8_CACHE: dict = {}
_LINEAR_FP8 = False
_FP8_MAX = 448.0  # OCP e4m3 finite max


_LINEAR_FP8_DGRAD = False
_LINEAR_FP8_WGRAD = False


def set_linear_fp8(on: bool, dgrad: bool = False, wgrad: bool = False) -> None:
    global _LINEAR_FP8, _LINEAR_FP8_DGRAD, _LINEAR_FP8_WGRAD
    _LINEAR_FP8 = bool(on)
    _LINEAR_FP8_DGRAD = bool(on and dgrad)
    _LINEAR_FP8_WGRAD = bool(on and dgrad and wgrad)
    _FP8_CACHE.clear()
    _FP8_ACT.clear()


def _w8_of(w: torch.Tensor, rowwise: bool = False, skey: tuple | None = None):
    # skey: stable identity for tensors whose storage churns per step
    # (the cached W^T) — keying state by their data_ptr re-bootstraps the
    # delayed-scaling amax every step (measured ~237 extra torch
    # abs+amax launches/step) and leaks stale _FP8_ACT/_FP8_CACHE
    # entries as the allocator rotates blocks.
    key = ((skey if skey is not None else (w.data_ptr(), *w.shape))
           + (rowwise,))
    hit = _FP8_CACHE.get(key)
    if hit is not None and hit[0] == _WT_EPOCH:
        return hit[1], hit[2]
    if rowwise:
        # per-output-channel weight scales, cached per optimizer step;
        # consumed transposed, so the row vector becomes scale_b=[1,N]
        w8, sinv = _quant_rowwise_fp8(w.reshape(w.shape[0], -1))
        w8 = w8.view(w.shape)
        _FP8_CACHE[key] = (_WT_EPOCH, w8, sinv.view(1, -1))
        return w8, sinv.view(1, -1)
    # per-step weight re-quantization ALSO goes through the fused kernel
    # (torch's abs+amax+mul+cast chain measured 126 ms/step over the 10B
    # weights); weights drift slowly, so last step's amax is the right
    # delayed scale
    w8, sinv = _quant_act_fp8(w.reshape(-1), ("w8",) + key)
    w8 = w8.view(w.shape)
    _FP8_CACHE[key] = (_WT_EPOCH, w8, sinv)
    return w8, sinv


# Rowwise scaling (opt-in, FORWARD GEMM only): one workgroup per row
# computes the row's amax and casts in a second L2-hot pass — no
# cross-step state, no outlier saturation on the activation path;
# torch._scaled_mm consumes the vectors as scale_a=[M,1] / scale_b=[1,N]
# (e4m3 x e4m3). dgrad/wgrad keep per-tensor delayed scaling: the e5m2
# rowwise _scaled_mm path is unvalidated on hipBLASLt, and the wgrad
# operands are already produced transposed by the fused transpose+quant
# kernel. Measured A/B at 10B: delayed 21.3k tok/s vs rowwise-fwd
# 21.0k (-1.5%, the extra per-row amax pass), convergence identical
# (Zipf-150m 2.1503 rowwise / 2.1518 delayed / 2.1537 bf16) — so the
# faster delayed path is the default; PRIME_AMD_FP8_ROWWISE=1 opts in
# per-row scales for models with activation outliers (also removes the
# cross-step amax state, which is not checkpointed).
def _fp8_rowwise_on() -> bool:
    import os

    return os.environ.get("PRIME_AMD_FP8_ROWWISE", "0") == "1"


def _quant_rowwise_fp8(x2: torch.Tensor, e5m2: bool = False):
    dt8 = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
    R, C = x2.shape
    x8 = torch.empty(R, C, device=x2.device, dtype=dt8)
    sinv = torch.empty(R, 1, device=x2.device, dtype=torch.float32)
    check(
        lib().prime_rowwise_quant_fp8(
            stream_of(x2), ptr(x2), ptr(x8), ptr(sinv), R, C,
            1 if e5m2 else 0,
        ),
        "rowwise_quant_fp8",
    )
    return x8, sinv


# per-site delayed-scaling state for activations: the fused quant kernel
# (csrc/quant_fp8.hip) casts with the PREVIOUS step's amax in ONE pass
# (outliers saturate for one step, TransformerEngine-style) and records
# this step's amax for the next — vs the 3-pass amax/mul/cast torch path
_FP8_ACT: dict = {}


def _quant_act_fp8(x2: torch.Tensor, site: tuple, e5m2: bool = False):
    dt8 = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
    fmax8 = 57344.0 if e5m2 else _FP8_MAX
    st = _FP8_ACT.get(site)
    if st is None:
        # bootstrap: dynamic 2-pass scaling, seed the amax state
        ax = x2.abs().amax().float().clamp(min=1e-12)
        sx = fmax8 / ax
        x8 = (x2 * sx.to(x2.dtype)).to(dt8)
        _FP8_ACT[site] = {
            "amax": ax.reshape(1).contiguous(),
            "next": torch.zeros(1, device=x2.device),
            "sinv": (1.0 / sx).reshape(1).contiguous(),
        }
        return x8, _FP8_ACT[site]["sinv"]
    x8 = torch.empty(x2.shape, device=x2.device, dtype=dt8)
    st["next"].zero_()
    check(
        lib().prime_quant_fp8(
            stream_of(x2), ptr(x2), ptr(x8), ptr(st["amax"]), ptr(st["next"]),
            ptr(st["sinv"]), x2.numel(), 1 if e5m2 else 0,
        ),
        "quant_fp8",
    )
    st["amax"], st["next"] = st["next"], st["amax"]
    return x8, st["sinv"]


class _Fp8Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        rw = _fp8_rowwise_on()
        if rw:
            x8, sxinv = _quant_rowwise_fp8(x2)
        else:
            x8, sxinv = _quant_act_fp8(x2, (w.data_ptr(), *w.shape))
        w8, swinv = _w8_of(w, rowwise=rw)
        y = torch._scaled_mm(x8, w8.t(), scale_a=sxinv, scale_b=swinv,
                             out_dtype=x.dtype)
        ctx.save_for_backward(x2, w)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        return _linear_backward(x2, w, dy)


def tuned_linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """F.linear (no bias) routed through layout-tuned GEMMs on HIP.
    The layout rewrites were measured at training-sized M (16k tokens);
    skinny decode GEMMs (M < 1024) keep the F.linear dispatch, which
    measured faster there (decode A/B: 2881 vs 2688 graph tok/s)."""
    if not _is_hip(x) or x.numel() // x.shape[-1] < 1024:
        _wgrad_release(w)  # dW will come through autograd's accumulate
        return torch.nn.functional.linear(x, w)
    if _LINEAR_FP8 and x.shape[-1] % 16 == 0 and w.shape[0] % 16 == 0:
        return _Fp8Linear.apply(x, w)
    return _TunedLinear.apply(x, w)


# ------------------------------------- fused projection + layout producers
# The gate/up and qkv projections feed kernels of ours on both sides, so
# the backward of those kernels can emit dY^T (the NN dW GEMM's operand)
# while it still holds dY in registers, instead of a separate transpose
# pass re-reading what was just written. The GEMMs see the same operands
# as tuned_linear's, so results match the composed ops bit for bit.
def _fused_layout_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """Same conditions under which _compute_dw takes its dY^T branch, on
    the plain bf16 tuned path (Trainer, non-FSDP, fp8 off)."""
    if not (_LINEAR_TUNED and not _LINEAR_FP8 and _is_hip(x)):
        return False
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or w.dim() != 2:
        return False
    M = x.numel() // x.shape[-1]
    return w.shape[0] % 128 == 0 and M % 64 == 0 and M >= 4096


def _dx_of(dy2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    wt = _wt_of(w) if _LINEAR_TUNED else None
    return torch.matmul(dy2, wt.t()) if wt is not None else torch.matmul(dy2, w)


class _GateUpSwiGLU(torch.autograd.Function):
    """swiglu(x @ W_gateup^T) as one node; saves {x, w, gu} like the
    composed ops. Backward: one kernel writes dgu and dgu^T."""

    @staticmethod
    def forward(ctx, x, w):
        x2 = x.reshape(-1, x.shape[-1])
        gu = torch.matmul(x2, w.t())
        I = w.shape[0] // 2
        out = torch.empty(x2.shape[0], I, device=x.device, dtype=x.dtype)
        check(lib().prime_swiglu_fwd(stream_of(gu), ptr(gu), ptr(out),
                                     x2.shape[0], I), "swiglu_fwd")
        ctx.save_for_backward(x2, w, gu)
        ctx.xshape = x.shape
        return out.view(*x.shape[:-1], I)

    @staticmethod
    def backward(ctx, dout):
        x2, w, gu = ctx.saved_tensors
        dgu, dgut = swiglu_bwd_t(dout.reshape(-1, dout.shape[-1]), gu)
        dx = _dx_of(dgu, w)
        return dx.view(ctx.xshape), _compute_dw(x2, w, dgu, dyt=dgut)


def gateup_swiglu(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up of the packed projection x @ w^T, w: [2I, K]."""
    if _fused_layout_ok(x, w):
        return _GateUpSwiGLU.apply(x, w)
    return swiglu(tuned_linear(x, w))


class _QkvRope(torch.autograd.Function):
    """(RoPE(q), RoPE(k), v) of the packed projection x @ W_qkv^T. q and k
    are rotated straight out of the GEMM output; v is a view of it.
    Backward packs dq/dk/dv into dqkv and dqkv^T in one kernel."""

    @staticmethod
    def forward(ctx, x, w, cos, sin, H, Hkv, D, pos_offset):
        B, S, K = x.shape
        x2 = x.reshape(-1, K)
        qkv = torch.matmul(x2, w.t()).view(B, S, -1)
        q = rope_packed_fwd(qkv[..., : H * D].view(B, S, H, D), cos, sin,
                            pos_offset)
        k = rope_packed_fwd(
            qkv[..., H * D : (H + Hkv) * D].view(B, S, Hkv, D), cos, sin,
            pos_offset)
        v = qkv[..., (H + Hkv) * D :].view(B, S, Hkv, D)
        ctx.save_for_backward(x2, w, cos, sin)
        ctx.meta = (B, S, K, H, Hkv, D, pos_offset)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x2, w, cos, sin = ctx.saved_tensors
        B, S, K, H, Hkv, D, off = ctx.meta
        # missing grads become dense zeros
        if dq is None:
            dq = x2.new_zeros(B, S, H, D)
        if dk is None:
            dk = x2.new_zeros(B, S, Hkv, D)
        if dv is None:
            dv = x2.new_zeros(B, S, Hkv, D)
        dqkv, dqkvt = qkv_grad_pack(dq, dk, dv, cos, sin, off)
        dx = _dx_of(dqkv, w)
        return (dx.view(B, S, K), _compute_dw(x2, w, dqkv, dyt=dqkvt),
                None, None, None, None, None, None)


def qkv_rope(x, w, cos, sin, n_heads: int, n_kv_heads: int, head_dim: int,
             pos_offset: int = 0):
    """x [B,S,K] @ w^T -> (RoPE(q) [B,S,H,D], RoPE(k) [B,S,Hkv,D],
    v [B,S,Hkv,D]); w: [(H+2Hkv)*D, K]."""
    H, Hkv, D = n_heads, n_kv_heads, head_dim
    if (x.dim() == 3 and D in (64, 128) and w.shape[0] == (H + 2 * Hkv) * D
            and _fused_layout_ok(x, w)):
        return _QkvRope.apply(x, w, cos, sin, H, Hkv, D, pos_offset)
    B, S = x.shape[0], x.shape[1]
    qkv = tuned_linear(x, w)
    q, k, v = qkv.split([H * D, Hkv * D, Hkv * D], dim=-1)
    q = apply_rope(q.view(B, S, H, D), cos, sin, pos_offset=pos_offset)
    k = apply_rope(k.view(B, S, Hkv, D), cos, sin, pos_offset=pos_offset)
    return q, k, v.view(B, S, Hkv, D)


# ------------------------------------------------- raw (non-autograd) ops
def fused_adamw(p32, p16, grad, m, v, *, lr, beta1, beta2, eps, wd, step,
                gscale=None):
    """One-pass AdamW; optional fused gradient clip via a 1-element device
    scalar `gscale` (grads are multiplied in-register, never rewritten)."""
    check(
        lib().prime_adamw(
            stream_of(p32), ptr(p32), ptr(p16), ptr(grad), ptr(m), ptr(v),
            ptr(gscale), p32.numel(), lr, beta1, beta2, eps, wd, step,
        ),
        "adamw",
    )


def grad_sqnorm(grad: torch.Tensor, out: torch.Tensor) -> None:
    """out (1-elem fp32, pre-zeroed) += sum(grad^2), single bf16 pass."""
    # per-block partials added up in a fixed order: the clip scale, and so
    # every weight update, is bit-identical from run to run
    part = torch.zeros(lib().prime_grad_sqnorm_partials(), device=grad.device,
                       dtype=torch.float32)
    check(lib().prime_grad_sqnorm(stream_of(grad), ptr(grad), ptr(part),
                                  grad.numel(), part.numel()),
          "grad_sqnorm")
    out.add_(part.sum())


def pseudograd(outer32, master32, out_delta):
    check(
        lib().prime_pseudograd(
            stream_of(outer32), ptr(outer32), ptr(master32), ptr(out_delta), outer32.numel()
        ),
        "pseudograd",
    )


QBLK = 1024


def quant_int8(x32: torch.Tensor):
    n = x32.numel()
    nblk = (n + QBLK - 1) // QBLK
    q = torch.empty(n, device=x32.device, dtype=torch.int8)
    scales = torch.empty(nblk, device=x32.device, dtype=torch.float32)
    check(lib().prime_quant_int8(stream_of(x32), ptr(x32), ptr(q), ptr(scales), n), "quant_int8")
    return q, scales


def dequant_int8(q, scales, out, accumulate: bool = False):
    check(
        lib().prime_dequant_int8(
            stream_of(out), ptr(q), ptr(scales), ptr(out), q.numel(), int(accumulate)
        ),
        "dequant_int8",
    )
    return out


def nesterov_outer(theta32, master32, inner16, buf32, delta32, *, lr, mu):
    check(
        lib().prime_nesterov_outer(
            stream_of(theta32), ptr(theta32), ptr(master32), ptr(inner16), ptr(buf32),
            ptr(delta32), theta32.numel(), lr, mu,
        ),
        "nesterov_outer",
    )


def mfma_probe(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """16x16x32 bf16 MFMA single-tile matmul (layout verification)."""
    C = torch.empty(16, 16, device=A.device, dtype=torch.float32)
    check(lib().prime_mfma_probe(stream_of(A), ptr(A), ptr(B), ptr(C)), "mfma_probe")
    return C


# ----------------------------------------------- fused residual + RMSNorm
class _AddRMSNorm(torch.autograd.Function):
    """(x, res) -> (y, s): s = x (+ res) is the new residual stream,
    y = rmsnorm(s) * w. One fused pass instead of {add; norm} (and the
    backward folds the residual-branch grad into the norm dx pass)."""

    @staticmethod
    def forward(ctx, x, res, w, eps: float):
        if not _is_hip(x):
            s = x if res is None else x + res
            y = ref.rmsnorm(s, w, eps)
            ctx.save_for_backward(s, w)
            ctx.eps = eps
            ctx.cpu = True
            return y, s
        x = x.contiguous()
        res = res.contiguous() if res is not None else None
        D = x.shape[-1]
        R = x.numel() // D
        s = torch.empty_like(x)
        y = torch.empty_like(x)
        rstd = torch.empty(R, device=x.device, dtype=torch.float32)
        check(
            lib().prime_add_rmsnorm_fwd(
                stream_of(x), ptr(x), ptr(res), ptr(w), ptr(s), ptr(y),
                ptr(rstd), R, D, eps,
            ),
            "add_rmsnorm_fwd",
        )
        ctx.save_for_backward(s, w, rstd)
        ctx.eps = eps
        ctx.cpu = False
        ctx.has_res = res is not None
        return y, s

    @staticmethod
    def backward(ctx, dy, ds_res):
        saved = ctx.saved_tensors
        if ctx.cpu:
            s, w = saved
            s2 = s.detach().float().requires_grad_(True)
            w2 = w.detach().float().requires_grad_(True)
            with torch.enable_grad():
                y = ref.rmsnorm(s2, w2, ctx.eps)
            gs, gw = torch.autograd.grad(y, [s2, w2], dy.float())
            if ds_res is not None:
                gs = gs + ds_res.float()
            gs = gs.to(dy.dtype)
            return gs, (gs if ctx.needs_input_grad[1] else None), gw.to(w.dtype), None
        s, w, rstd = saved
        dy = dy.contiguous()
        D = s.shape[-1]
        R = s.numel() // D
        ds = torch.empty_like(s)
        G = max(1, min(R, _DW_ROWS))
        dw = torch.empty(G, D, device=s.device, dtype=torch.float32)
        dres_in = ds_res.contiguous() if ds_res is not None else None
        check(
            lib().prime_add_rmsnorm_bwd(
                stream_of(s), ptr(dy), ptr(dres_in), ptr(s), ptr(w), ptr(rstd),
                ptr(ds), ptr(dw), R, D, G, ctx.eps,
            ),
            "add_rmsnorm_bwd",
        )
        return ds, (ds if ctx.needs_input_grad[1] else None), dw.sum(0).to(w.dtype), None


def fused_add_rmsnorm(x, res, w, eps: float = 1e-5):
    """Returns (y, s): y = rmsnorm(x + res) * w, s = x + res."""
    return _AddRMSNorm.apply(x, res, w, eps)


# ------------------------------------------------------- decode attention
def attn_decode(q, k_cache, v_cache, length: int, len_dev=None) -> torch.Tensor:
    """Single-token decode: q [B,H,D] (or [B,1,H,D]) against the first
    `length` rows of k/v caches [B,Smax,Hkv,D]. Returns [B,H,D]. `len_dev`
    (optional int32 device scalar) overrides `length` at kernel time
    (hipGraph decode)."""
    if q.dim() == 4:
        q = q.squeeze(1)
    B, H, D = q.shape
    _, Smax, Hkv, _ = k_cache.shape
    if not _is_hip(q):
        qs = q.unsqueeze(1)  # [B,1,H,D]
        o = ref.attention(qs, k_cache[:, :length], v_cache[:, :length], causal=False)
        return o.squeeze(1)
    q = q.contiguous()
    o = torch.empty_like(q)
    check(
        lib().prime_attn_decode(
            stream_of(q), ptr(q), ptr(k_cache), ptr(v_cache), ptr(o),
            B, H, Hkv, Smax, length, D, D**-0.5, ptr(len_dev),
        ),
        "attn_decode",
    )
    return o


# ------------------------------------------------ ragged (batched) decode
# Internal boundaries of the ragged decode kernel: the online softmax walks
# the cache in chunks of DECODE_RAGGED_CHUNK keys, and each (batch, kv head)
# is split along the sequence into ranges of decode_ragged_split(...) rows.
DECODE_RAGGED_CHUNK = 256
_RAGGED_GROUPS = (1, 2, 4, 8)
_RAGGED_WS: dict = {}  # (B, Hkv, G, D, nsplit, device) -> fp32 partials


def decode_ragged_split(B: int, Hkv: int, Smax: int, n_cu: int = 256) -> int:
    """Rows per sequence split of attn_decode_ragged for a cache shape: a
    multiple of DECODE_RAGGED_CHUNK aiming at ~4 workgroups per CU. Depends
    on the launch shape only, never on the lengths, so it is stable under
    graph replay. The number of splits is ceil(Smax / rows)."""
    chunks = -(-Smax // DECODE_RAGGED_CHUNK)
    want = max(1, min(chunks, -(-4 * n_cu // (B * Hkv))))
    return -(-chunks // want) * DECODE_RAGGED_CHUNK


def _n_cu(dev) -> int:
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _check_ragged_shape(H: int, Hkv: int, D: int) -> None:
    if D not in (64, 128) or H % Hkv != 0 or H // Hkv not in _RAGGED_GROUPS:
        raise NotImplementedError(
            f"attn_decode_ragged needs head_dim in {{64, 128}} and a GQA group "
            f"size in {_RAGGED_GROUPS} (got head_dim={D}, heads={H}, "
            f"kv_heads={Hkv})")


def attn_decode_ragged(q, k_cache, v_cache, lens, split_rows=None) -> torch.Tensor:
    """Single-token decode with per-sequence lengths: q [B,H,D] (or
    [B,1,H,D]); sequence b attends to rows [0, lens[b]) of its own caches
    [B,Smax,Hkv,D]. `lens` is an int32 [B] tensor on q's device, read at
    kernel time and clamped to [0, Smax]; lens[b] == 0 is an idle slot whose
    output row is exactly zero and whose cache is not read. `split_rows`
    overrides decode_ragged_split (a multiple of DECODE_RAGGED_CHUNK)."""
    if q.dim() == 4:
        q = q.squeeze(1)
    B, H, D = q.shape
    _, Smax, Hkv, _ = k_cache.shape
    if lens.dtype != torch.int32 or lens.shape != (B,) or lens.device != q.device:
        raise ValueError("lens must be an int32 [B] tensor on q's device")
    if not _is_hip(q):
        o = torch.zeros_like(q)
        for b, n in enumerate(lens.tolist()):
            n = min(max(n, 0), Smax)
            if n > 0:
                o[b] = ref.attention(q[b:b + 1].unsqueeze(1), k_cache[b:b + 1, :n],
                                     v_cache[b:b + 1, :n], causal=False)[0, 0]
        return o
    _check_ragged_shape(H, Hkv, D)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("attn_decode_ragged needs contiguous KV caches")
    if split_rows is None:
        split_rows = decode_ragged_split(B, Hkv, Smax, _n_cu(q.device))
    if split_rows <= 0 or split_rows % DECODE_RAGGED_CHUNK != 0:
        raise ValueError(f"split_rows must be a positive multiple of "
                         f"{DECODE_RAGGED_CHUNK} (got {split_rows})")
    nsplit = -(-Smax // split_rows)
    G = H // Hkv
    # one workspace per shape, reused: a captured graph sees stable pointers
    key = (B, Hkv, G, D, nsplit, q.device.index)
    ws = _RAGGED_WS.get(key)
    if ws is None:
        ws = _RAGGED_WS[key] = torch.empty(
            B * Hkv, nsplit, G * (D + 2), device=q.device, dtype=torch.float32)
    q = q.contiguous()
    o = torch.empty_like(q)
    check(
        lib().prime_attn_decode_ragged(
            stream_of(q), ptr(q), ptr(k_cache), ptr(v_cache), ptr(o), ptr(ws),
            ptr(lens), B, H, Hkv, Smax, D, split_rows, D**-0.5,
        ),
        "attn_decode_ragged",
    )
    return o


def decode_qkv_append(qkv, cos, sin, k_cache, v_cache, pos, n_heads: int,
                      n_kv_heads: int) -> torch.Tensor:
    """Decode-step prep in one launch: qkv [B, (H+2Hkv)*D] is the packed
    projection of one new token per sequence; rotates q and k at pos[b]
    (bit-identical to apply_rope(..., pos_offset=pos[b])), writes k and v to
    row pos[b] of the caches [B,Smax,Hkv,D] and returns the rotated q
    [B,H,D]. `pos` is an int32 [B] device tensor; a slot with pos[b] < 0 or
    pos[b] >= min(Smax, len(cos)) is idle: nothing is written for it and its
    q is zeros."""
    B = qkv.shape[0]
    H, Hkv = n_heads, n_kv_heads
    _, Smax, Hkv_c, D = k_cache.shape
    T = cos.shape[0]
    if qkv.dim() != 2 or qkv.shape[1] != (H + 2 * Hkv) * D or Hkv_c != Hkv:
        raise ValueError(f"decode_qkv_append: qkv {tuple(qkv.shape)} does not "
                         f"match heads={H}, kv_heads={Hkv}, head_dim={D}")
    if pos.dtype != torch.int32 or pos.shape != (B,) or pos.device != qkv.device:
        raise ValueError("pos must be an int32 [B] tensor on qkv's device")
    if not _is_hip(qkv):
        q = torch.zeros(B, H, D, dtype=qkv.dtype, device=qkv.device)
        x = qkv.view(B, 1, H + 2 * Hkv, D)
        for b, p in enumerate(pos.tolist()):
            if not 0 <= p < min(Smax, T):
                continue
            q[b] = ref.apply_rope(x[b:b + 1, :, :H], cos, sin, p)[0, 0]
            k_cache[b, p] = ref.apply_rope(x[b:b + 1, :, H:H + Hkv], cos, sin, p)[0, 0]
            v_cache[b, p] = x[b, 0, H + Hkv:]
        return q
    if D not in (64, 128):
        raise NotImplementedError(
            f"decode_qkv_append needs head_dim in {{64, 128}} (got {D})")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("decode_qkv_append needs contiguous KV caches")
    qkv = qkv.contiguous()
    q = torch.empty(B, H, D, dtype=qkv.dtype, device=qkv.device)
    check(
        lib().prime_decode_qkv_append(
            stream_of(qkv), ptr(qkv), ptr(q), ptr(k_cache), ptr(v_cache),
            ptr(cos), ptr(sin), ptr(pos), B, H, Hkv, D, Smax, T,
        ),
        "decode_qkv_append",
    )
    return q


# ------------------------------------------------------------ fp8 KV cache
class KVCacheFp8(NamedTuple):
    """One layer's fp8 KV cache. k, v: float8_e4m3fn [B,Smax,Hkv,D];
    k_scale, v_scale: fp32 [B,Smax,Hkv], the dequantisation factor of each
    (sequence, row, kv head) vector. For a vector x: m = max(max|x|, 1e-12),
    s = 448 / m, sinv = m / 448 (fp32), byte = e4m3_rne(clamp(x * s, -448,
    448)), scale = sinv; the stored value is float(byte) * sinv. A zero
    vector gives zero bytes and sinv = 1e-12 / 448."""
    k: torch.Tensor
    v: torch.Tensor
    k_scale: torch.Tensor
    v_scale: torch.Tensor


_E4M3_MAX = 448.0


def kv_cache_fp8(B: int, Smax: int, Hkv: int, D: int, device=None) -> KVCacheFp8:
    """A zeroed fp8 KV cache for one layer."""
    def z(*shape, dtype):
        return torch.zeros(*shape, dtype=dtype, device=device)

    return KVCacheFp8(z(B, Smax, Hkv, D, dtype=torch.float8_e4m3fn),
                      z(B, Smax, Hkv, D, dtype=torch.float8_e4m3fn),
                      z(B, Smax, Hkv, dtype=torch.float32),
                      z(B, Smax, Hkv, dtype=torch.float32))


def kv_cache_dequant(cache: KVCacheFp8):
    """The values an fp8 cache holds, as fp32 (k, v) [B,Smax,Hkv,D]: the
    executable definition of the format."""
    return (cache.k.float() * cache.k_scale.unsqueeze(-1),
            cache.v.float() * cache.v_scale.unsqueeze(-1))


def _kv_quant(x: torch.Tensor):
    """x [..., D] -> (e4m3 [..., D], sinv fp32 [...]) by the KVCacheFp8 rule,
    in plain torch."""
    xf = x.float()
    m = xf.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12)
    fm = torch.tensor(_E4M3_MAX, dtype=torch.float32, device=x.device)
    q = (xf * (fm / m)).clamp(-_E4M3_MAX, _E4M3_MAX)
    return q.to(torch.float8_e4m3fn), (m / fm).squeeze(-1)


def _check_fp8_cache(cache, what: str) -> None:
    if not isinstance(cache, KVCacheFp8):
        raise TypeError(f"{what} needs a KVCacheFp8 (got {type(cache).__name__})")
    k, v, ks, vs = cache
    if k.dim() != 4 or v.shape != k.shape or ks.shape != k.shape[:3] \
            or vs.shape != k.shape[:3]:
        raise ValueError(f"{what}: inconsistent KVCacheFp8 shapes")
    if k.dtype != torch.float8_e4m3fn or v.dtype != torch.float8_e4m3fn \
            or ks.dtype != torch.float32 or vs.dtype != torch.float32:
        raise ValueError(f"{what}: KVCacheFp8 needs float8_e4m3fn k/v and "
                         "fp32 scales")


def _fp8_cache_contiguous(cache, what: str) -> None:
    # a view of the leading slots (cache[:n]) is contiguous too
    if not all(t.is_contiguous() for t in cache):
        raise ValueError(f"{what} needs a contiguous KVCacheFp8")


def kv_store_fp8(cache: KVCacheFp8, k, v, pos: int) -> None:
    """Prefill store: quantise k, v [B,S,Hkv,D] per head row into rows
    [pos, pos+S) of the first B sequences of `cache` ([B',Smax,Hkv,D],
    B <= B'). Other rows and slots are left as they are."""
    _check_fp8_cache(cache, "kv_store_fp8")
    Bc, Smax, Hkv, D = cache.k.shape
    if k.dim() != 4 or v.shape != k.shape or k.shape[2:] != (Hkv, D) \
            or k.shape[0] > Bc:
        raise ValueError(f"kv_store_fp8: k/v {tuple(k.shape)} do not fit a "
                         f"cache {tuple(cache.k.shape)}")
    B, S = k.shape[:2]
    if pos < 0 or pos + S > Smax:
        raise ValueError(f"kv_store_fp8: rows [{pos}, {pos + S}) outside a "
                         f"cache of {Smax} rows")
    if B == 0 or S == 0:
        return
    if not _is_hip(k):
        for x, c, sc in ((k, cache.k, cache.k_scale), (v, cache.v, cache.v_scale)):
            q, sinv = _kv_quant(x)
            c[:B, pos:pos + S] = q
            sc[:B, pos:pos + S] = sinv
        return
    if D not in (64, 128):
        raise NotImplementedError(
            f"kv_store_fp8 needs head_dim in {{64, 128}} (got {D})")
    _fp8_cache_contiguous(cache, "kv_store_fp8")
    k, v = k.contiguous(), v.contiguous()
    check(
        lib().prime_kv_store_fp8(
            stream_of(k), ptr(k), ptr(v), ptr(cache.k), ptr(cache.v),
            ptr(cache.k_scale), ptr(cache.v_scale), B, S, Hkv, D, Smax, pos,
        ),
        "kv_store_fp8",
    )


def decode_qkv_append_fp8(qkv, cos, sin, cache: KVCacheFp8, pos, n_heads: int,
                          n_kv_heads: int) -> torch.Tensor:
    """decode_qkv_append into an fp8 cache: the same inputs, idle rule and
    rotated q (bit-identical); k (rotated, rounded to qkv's dtype) and v are
    quantised per head row into row pos[b] of `cache`."""
    _check_fp8_cache(cache, "decode_qkv_append_fp8")
    B = qkv.shape[0]
    H, Hkv = n_heads, n_kv_heads
    _, Smax, Hkv_c, D = cache.k.shape
    T = cos.shape[0]
    if qkv.dim() != 2 or qkv.shape[1] != (H + 2 * Hkv) * D or Hkv_c != Hkv:
        raise ValueError(f"decode_qkv_append_fp8: qkv {tuple(qkv.shape)} does "
                         f"not match heads={H}, kv_heads={Hkv}, head_dim={D}")
    if pos.dtype != torch.int32 or pos.shape != (B,) or pos.device != qkv.device:
        raise ValueError("pos must be an int32 [B] tensor on qkv's device")
    if not _is_hip(qkv):
        q = torch.zeros(B, H, D, dtype=qkv.dtype, device=qkv.device)
        x = qkv.view(B, 1, H + 2 * Hkv, D)
        for b, p in enumerate(pos.tolist()):
            if not 0 <= p < min(Smax, T):
                continue
            q[b] = ref.apply_rope(x[b:b + 1, :, :H], cos, sin, p)[0, 0]
            kq, ks = _kv_quant(
                ref.apply_rope(x[b:b + 1, :, H:H + Hkv], cos, sin, p)[0, 0])
            vq, vs = _kv_quant(x[b, 0, H + Hkv:])
            cache.k[b, p], cache.k_scale[b, p] = kq, ks
            cache.v[b, p], cache.v_scale[b, p] = vq, vs
        return q
    if D not in (64, 128):
        raise NotImplementedError(
            f"decode_qkv_append_fp8 needs head_dim in {{64, 128}} (got {D})")
    _fp8_cache_contiguous(cache, "decode_qkv_append_fp8")
    qkv = qkv.contiguous()
    q = torch.empty(B, H, D, dtype=qkv.dtype, device=qkv.device)
    check(
        lib().prime_decode_qkv_append_fp8(
            stream_of(qkv), ptr(qkv), ptr(q), ptr(cache.k), ptr(cache.v),
            ptr(cache.k_scale), ptr(cache.v_scale), ptr(cos), ptr(sin),
            ptr(pos), B, H, Hkv, D, Smax, T,
        ),
        "decode_qkv_append_fp8",
    )
    return q


def attn_decode_ragged_fp8(q, cache: KVCacheFp8, lens, split_rows=None) -> torch.Tensor:
    """attn_decode_ragged over an fp8 cache: the same lens / idle / clamp
    rules and split_rows contract; the values attended to are
    kv_cache_dequant(cache)."""
    _check_fp8_cache(cache, "attn_decode_ragged_fp8")
    if q.dim() == 4:
        q = q.squeeze(1)
    B, H, D = q.shape
    _, Smax, Hkv, _ = cache.k.shape
    if lens.dtype != torch.int32 or lens.shape != (B,) or lens.device != q.device:
        raise ValueError("lens must be an int32 [B] tensor on q's device")
    if not _is_hip(q):
        o = torch.zeros_like(q)
        for b, n in enumerate(lens.tolist()):
            n = min(max(n, 0), Smax)
            if n > 0:
                kf, vf = kv_cache_dequant(KVCacheFp8(
                    *(t[b:b + 1, :n] for t in cache)))
                o[b] = ref.attention(q[b:b + 1].unsqueeze(1), kf, vf,
                                     causal=False)[0, 0]
        return o
    _check_ragged_shape(H, Hkv, D)
    _fp8_cache_contiguous(cache, "attn_decode_ragged_fp8")
    if split_rows is None:
        split_rows = decode_ragged_split(B, Hkv, Smax, _n_cu(q.device))
    if split_rows <= 0 or split_rows % DECODE_RAGGED_CHUNK != 0:
        raise ValueError(f"split_rows must be a positive multiple of "
                         f"{DECODE_RAGGED_CHUNK} (got {split_rows})")
    nsplit = -(-Smax // split_rows)
    G = H // Hkv
    # the bf16 op's workspace: same shape key, and the ops run in stream order
    key = (B, Hkv, G, D, nsplit, q.device.index)
    ws = _RAGGED_WS.get(key)
    if ws is None:
        ws = _RAGGED_WS[key] = torch.empty(
            B * Hkv, nsplit, G * (D + 2), device=q.device, dtype=torch.float32)
    q = q.contiguous()
    o = torch.empty_like(q)
    check(
        lib().prime_attn_decode_ragged_fp8(
            stream_of(q), ptr(q), ptr(cache.k), ptr(cache.v),
            ptr(cache.k_scale), ptr(cache.v_scale), ptr(o), ptr(ws), ptr(lens),
            B, H, Hkv, Smax, D, split_rows, D**-0.5,
        ),
        "attn_decode_ragged_fp8",
    )
    return o


def mfma_probe32(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """32x32x16 bf16 MFMA single-tile matmul (layout verification)."""
    C = torch.empty(32, 32, device=A.device, dtype=torch.float32)
    check(lib().prime_mfma_probe32(stream_of(A), ptr(A), ptr(B), ptr(C)), "mfma_probe32")
    return C
