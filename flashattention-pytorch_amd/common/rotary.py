"""Rotary position embedding for training and prefill, in FlashAttention's names, argument order and defaults
(`flash_attn.layers.rotary`), over the HIP library's `fa_rotary_apply` (include/fa_mi355x.h):

    apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None) -> x'
    apply_rotary_emb_qkv_(qkv, cos, sin, interleaved=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None,
                          num_heads_q=None) -> qkv (rotated in place)

x: (B, S, heads, d), or packed (total, heads, d) with cu_seqlens (int32 (B + 1,) on the device) and max_seqlen; float16 or
bfloat16 on the GPU.  cos, sin: (seqlen_ro, rotary_dim / 2) in x's dtype, the tables `flash_attn_with_kvcache(..., rotary_cos=,
rotary_sin=)` takes; rotary_dim a multiple of 16 in [16, d], head dims at and past it pass through.  interleaved pairs elements
(2j, 2j + 1) (GPT-J), otherwise (j, j + rotary_dim / 2) (GPT-NeoX).  seqlen_offsets: an int, or an int32 (B,) device tensor (never
read on the host): token i of sequence b is rotated at table row seqlen_offsets[b] + i, and passes through unrotated when that is
not a row of the tables.  The arithmetic is the decode call's to the bit, so a key rotated here at position p has the bits
`flash_attn_with_kvcache` stores for it at position p: prefill and decode fill one cache with one rounding.

Both functions are differentiable in x / qkv; tables and offsets take no gradient.  The backward is the conjugate rotation (by
-sin) of the incoming gradient, one launch; the incoming gradient itself is never modified.  No CPU path, and fp32 tensors are
refused, as the KV-cache calls refuse them.
"""
from __future__ import annotations

import torch


def _saved_offsets(ctx, seqlen_offsets, cu_seqlens, cos, sin):
    tensors = [cos, sin]
    ctx.offsets_saved = isinstance(seqlen_offsets, torch.Tensor)
    ctx.cu_saved = cu_seqlens is not None
    if ctx.offsets_saved:
        tensors.append(seqlen_offsets)
    else:
        ctx.seqlen_offsets = seqlen_offsets
    if ctx.cu_saved:
        tensors.append(cu_seqlens)
    ctx.save_for_backward(*tensors)


def _restored_offsets(ctx):
    saved = list(ctx.saved_tensors)
    cos, sin = saved[:2]
    rest = saved[2:]
    seqlen_offsets = rest.pop(0) if ctx.offsets_saved else ctx.seqlen_offsets
    cu_seqlens = rest.pop(0) if ctx.cu_saved else None
    return cos, sin, seqlen_offsets, cu_seqlens


class _ApplyRotaryEmb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, interleaved, inplace, seqlen_offsets, cu_seqlens, max_seqlen):
        import flashattention_lab_cuda as ext

        out = ext.rotary_apply(x, cos, sin, out=x if inplace else None, interleaved=interleaved, seqlen_offsets=seqlen_offsets,
                               cu_seqlens=cu_seqlens, max_seqlen=max_seqlen)
        if inplace:
            ctx.mark_dirty(x)
        _saved_offsets(ctx, seqlen_offsets, cu_seqlens, cos, sin)
        ctx.interleaved, ctx.max_seqlen = interleaved, max_seqlen
        return out

    @staticmethod
    def backward(ctx, do):
        import flashattention_lab_cuda as ext

        cos, sin, seqlen_offsets, cu_seqlens = _restored_offsets(ctx)
        kw = dict(interleaved=ctx.interleaved, conjugate=True, seqlen_offsets=seqlen_offsets, cu_seqlens=cu_seqlens,
                  max_seqlen=ctx.max_seqlen)
        try:     # the gradient as it lies in memory (a token-strided view is addressed as it is); it is only read
            dx = ext.rotary_apply(do, cos, sin, **kw)
        except ValueError:
            dx = ext.rotary_apply(do.contiguous(), cos, sin, **kw)
        return (dx,) + (None,) * 7


def apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None):
    """x with the first rotary_dim head dims of every head rotated (see the head of this module).  inplace=True rotates x itself
    and returns it (x is marked dirty for autograd); otherwise a new dense tensor is returned and x is only read."""
    return _ApplyRotaryEmb.apply(x, cos, sin, bool(interleaved), bool(inplace), seqlen_offsets, cu_seqlens, max_seqlen)


def _qk_view(who, qkv, packed, num_heads_q):
    """The q and k heads of a fused projection as one (.., heads, d) view of qkv's memory (never a copy)."""
    lead = 1 if packed else 2      # (total,) or (B, S)
    if num_heads_q is None:
        if qkv.dim() != lead + 3 or qkv.shape[lead] != 3:
            shape = "(total, 3, H, d)" if packed else "(B, S, 3, H, d)"
            raise ValueError(f"{who}: qkv must be {shape} (or pass num_heads_q for the (.., H_q + 2 H_kv, d) layout); got "
                             f"{tuple(qkv.shape)}")
        h, d = qkv.shape[-2:]
        try:     # (.., 2, H, d) -> (.., 2 H, d): a view exactly when the k heads follow the q heads at the head stride
            return qkv[..., :2, :, :].view(*qkv.shape[:lead], 2 * h, d)
        except RuntimeError:
            raise ValueError(f"{who}: the q and k heads of qkv must be adjacent in memory (strides {tuple(qkv.stride())}); qkv is "
                             f"never copied") from None
    hq = int(num_heads_q)
    if qkv.dim() != lead + 2 or hq < 1 or qkv.shape[-2] <= hq or (qkv.shape[-2] - hq) % 2 != 0:
        shape = "(total, H_q + 2 H_kv, d)" if packed else "(B, S, H_q + 2 H_kv, d)"
        raise ValueError(f"{who}: with num_heads_q = {num_heads_q} qkv must be {shape}, H_kv >= 1; got {tuple(qkv.shape)}")
    return qkv[..., :hq + (qkv.shape[-2] - hq) // 2, :]


class _ApplyRotaryEmbQKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, interleaved, seqlen_offsets, cu_seqlens, max_seqlen, num_heads_q):
        import flashattention_lab_cuda as ext

        qk = _qk_view("apply_rotary_emb_qkv_", qkv, cu_seqlens is not None, num_heads_q)
        ext.rotary_apply(qk, cos, sin, out=qk, interleaved=interleaved, seqlen_offsets=seqlen_offsets, cu_seqlens=cu_seqlens,
                         max_seqlen=max_seqlen)
        ctx.mark_dirty(qkv)
        _saved_offsets(ctx, seqlen_offsets, cu_seqlens, cos, sin)
        ctx.interleaved, ctx.max_seqlen, ctx.num_heads_q = interleaved, max_seqlen, num_heads_q
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        import flashattention_lab_cuda as ext

        cos, sin, seqlen_offsets, cu_seqlens = _restored_offsets(ctx)
        dqkv = dqkv.clone(memory_format=torch.contiguous_format)     # the incoming gradient is never modified: v's part is the copy
        dqk = _qk_view("apply_rotary_emb_qkv_", dqkv, cu_seqlens is not None, ctx.num_heads_q)
        ext.rotary_apply(dqk, cos, sin, out=dqk, interleaved=ctx.interleaved, conjugate=True, seqlen_offsets=seqlen_offsets,
                         cu_seqlens=cu_seqlens, max_seqlen=ctx.max_seqlen)
        return (dqkv,) + (None,) * 7


def apply_rotary_emb_qkv_(qkv, cos, sin, interleaved=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None, num_heads_q=None):
    """Rotates q and k of a fused projection in place, in one launch, and leaves v untouched; returns qkv.  Without num_heads_q:
    qkv (B, S, 3, H, d), or (total, 3, H, d) with cu_seqlens.  With num_heads_q (GQA): qkv (B, S, H_q + 2 H_kv, d), or
    (total, H_q + 2 H_kv, d) with cu_seqlens, the q heads first, then k, then v."""
    return _ApplyRotaryEmbQKV.apply(qkv, cos, sin, bool(interleaved), seqlen_offsets, cu_seqlens, max_seqlen, num_heads_q)
