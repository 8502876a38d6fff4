"""Merge of partial attention results, the update step of ring / context-parallel attention, of cascade (shared-prefix) inference
and of attention over key chunks that do not fit one call:

    merge_attention_states(o_a, lse_a, o_b, lse_b, *, layout="bhnd", out=None) -> (o, lse)

(o_a, lse_a) and (o_b, lse_b) are attention of the same queries over two DISJOINT key sets, as the library's calls return them
(lse: the natural-log normaliser of each row, float32, -inf for a row without a visible key).  The result is attention over the
union:  lse = logaddexp(lse_a, lse_b),  o = exp(lse_a - lse) o_a + exp(lse_b - lse) o_b,  one HIP launch (fa_merge_states,
include/fa_mi355x.h), fp64 arithmetic from the stored values and one rounding to fp32 and the tensor dtype.  A side with lse = -inf
has weight 0 and its o is not used, even if it holds NaN; both -inf give o = 0, lse = -inf.  Merging is associative, so more than two
chunks fold left to right.

Layouts, each taken from the views' own strides without a copy (a slice of a wider tensor is fine):

    "bhnd"   o (B, H, N, d) or (BH, N, d),  lse (B, H, N) or (BH, N)      flash_attention_ex(..., return_lse=True)
    "bnhd"   o (B, N, H, d),                lse (B, H, N)                 flash_attn_with_kvcache(..., return_softmax_lse=True)
    "thd"    o (T, H, d),                   lse (H, T)                    flash_attention_varlen(..., return_softmax_lse=True),
                                                                          flash_attn_with_kvcache with cu_seqlens_q

o_a, o_b: float16, bfloat16 (d a multiple of 8) or float32 (any d), up to d = 256.  Differentiable in all four inputs (one backward
launch, fa_merge_states_backward, deterministic); chained with the differentiable lse of flash_attention_ex / flash_attention_varlen
the gradients are those of the single call over all the keys.  out = (o, lse) writes into given tensors and is allowed only outside
autograd; it may be (o_a, lse_a) themselves, the accumulate step of a ring loop under torch.no_grad().

Which chunk calls make up a causal call: the library aligns `causal` bottom-right, so the chunk keys[j0:j1] of a causal call over
Nk keys is `causal=False, window_size=(left', Nk - j1)` on the chunk (left' = the full call's left bound less Nk - j1, or -1), and
the last chunk is plain `causal=True`; with sinks, pass `sinks` to exactly one chunk.  ALiBi across chunks is not expressible and is
out of scope.  See flash_attention_ex's docstring.

The merge works at o's width, whatever it is, so chunked MLA prefill composes with it: (o, lse) pairs of flash_attention_ex /
flash_attention_varlen calls whose v is narrower than q and k (192 + 128) merge as any others, gradients included.  Those calls take
no window_size; the chunking they can express is the usual one of prefill behind a prefix — the keys every row sees whole as one
`causal=False` chunk, the trailing Nq keys as the `causal=True` chunk.

Errors: mismatched shapes, dtypes or devices RuntimeError; an unknown layout, or a view the kernel cannot address (a last dim that
is not contiguous, 16-bit tensors that are not 16-byte aligned with strides that are multiples of 8 elements) ValueError — nothing is
copied silently.  No CPU path.
"""
from __future__ import annotations

import torch


class _MergeStatesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o_a, lse_a, o_b, lse_b, layout):
        import flashattention_lab_cuda as ext

        ctx.set_materialize_grads(False)
        ctx.layout = layout
        o, lse = ext.merge_states(o_a, lse_a, o_b, lse_b, layout)
        ctx.save_for_backward(o_a, lse_a, o_b, lse_b)
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        import flashattention_lab_cuda as ext

        if do is None and dlse is None:
            return None, None, None, None, None
        o_a, lse_a, o_b, lse_b = ctx.saved_tensors
        do = torch.zeros_like(o_a, memory_format=torch.contiguous_format) if do is None else do.contiguous()
        do_a, do_b, dlse_a, dlse_b = ext.merge_states_backward(o_a, lse_a, o_b, lse_b, do, None if dlse is None else dlse.contiguous(),
                                                               ctx.layout)
        return do_a, dlse_a, do_b, dlse_b, None


def merge_attention_states(o_a, lse_a, o_b, lse_b, *, layout="bhnd", out=None):
    import flashattention_lab_cuda as ext

    if layout not in ext.MERGE_LAYOUTS:
        raise ValueError(f"merge_attention_states: layout must be one of {ext.MERGE_LAYOUTS}, got {layout!r}")
    tensors = (o_a, lse_a, o_b, lse_b)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError("merge_attention_states: out must be a pair (o, lse) of tensors")
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (*tensors, *out)):
            raise RuntimeError("merge_attention_states: out= is allowed only outside autograd (an input requires grad; call it under "
                               "torch.no_grad(), or let the call allocate its result)")
        with torch.no_grad():
            return ext.merge_states(o_a, lse_a, o_b, lse_b, layout, out=out)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        return _MergeStatesFn.apply(o_a, lse_a, o_b, lse_b, layout)
    return ext.merge_states(o_a, lse_a, o_b, lse_b, layout)
