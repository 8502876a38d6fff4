"""The MXFP4 KV cache at head dims 64, 128 and 256 (C ABI: fa_fp4_kvcache_append_hdim, fa_fp4_forward_kvcache_hdim,
fa_fp4_forward_varlen_hdim): the cache of common.fp4_kvcache at the width of the model, with the sliding
window, the softcap and the sinks on both readers.  gpt-oss (sinks, a 128-token window) has heads of 64, Gemma-2 / 3 (a softcap, an
alternating window) heads of 256.

    mxfp4_append     16-bit k, v (B, N_new, H_kv, d) -> e2m1 codes and E8M0 scales at cache_seqlens[b] + i, in place
    mxfp4_decode     e4m3 q (B, Nq, H_q, d) over that cache: split-KV decoding, mxfp4_attn_with_kvcache's keywords
    mxfp4_prefill    packed e4m3 q (total_q, H_q, d) over the paged cache: chunked prefill, mxfp4_attn_varlen_func's keywords

The cache per K/V head at d in {64, 128, 256} (at 128 byte for byte common.fp4_kvcache's):
    k_cache  uint8 (.., H_kv, d / 2): two e2m1 codes a byte, the low nibble the even channel
    k_scale  uint8 (.., H_kv, d / 32): one E8M0 byte per 32 channels, value 2^(byte - 127)
    v_cache  as k_cache;  v_scale uint8 (.., H_kv): ONE E8M0 byte per (token, head), its maximum taken over all d channels
67 bytes a token and head at d = 64 against 128 in e4m3, 265 at d = 256 against 512.  Code rows are 16-byte aligned, k_scale rows
d / 32-byte aligned.  d is read from q (or k) and every array must agree with it.  softmax_scale defaults to d ** -0.5.  The
exponent and tie rules, the descales, the trust rules and graph replay are common.fp4_kvcache's.  Refused by name
(NotImplementedError): cache_leftpad, qv, rotary tables, ALiBi, a bias, 16-bit q, head dims such as 96 / 192; packed queries on the
decode call (they are mxfp4_prefill's).  No gradient."""
from __future__ import annotations

import torch

from .fp4_kvcache import _det, _window

_REFUSED = dict(
    cache_leftpad="cache_leftpad", qv="qv (MLA)", rotary_cos="rotary embedding", rotary_sin="rotary embedding", alibi_slopes="ALiBi",
    attn_bias="an additive bias", cu_seqlens_q="packed queries (mxfp4_prefill takes them)", max_seqlen_q="packed queries (mxfp4_prefill "
    "takes them)", cu_seqlens_k_new="packed new keys", cache_batch_idx="cache_batch_idx", cache_seqlens="cache_seqlens (cu_seqlens_k "
    "holds the lengths)")


def _refuse(who, unsupported):
    for name, val in unsupported.items():
        if name not in _REFUSED:
            raise TypeError(f"{who}() got an unexpected keyword argument '{name}'")
        if isinstance(val, torch.Tensor) or val not in (None, False, 0, 0.0):
            raise NotImplementedError(f"{who}: {name} is not supported: the MXFP4 cache calls take no {_REFUSED[name]}")


def mxfp4_append(k, v, k_cache, k_scale, v_cache, v_scale, *, cache_seqlens, block_table=None, cache_batch_idx=None, k_descale=None,
                 v_descale=None, **unsupported):
    """Append k, v (B, N_new, H_kv, d) float16 / bfloat16, d in {64, 128, 256}, to the MXFP4 cache of that width at positions
    cache_seqlens[b] + i (the lengths BEFORE the append; clamped on the device, not modified): mxfp4_kvcache_append's rule with K's
    blocks of 32 channels and V's one block of all d.  A token outside the cache is dropped.  Returns None."""
    who = "mxfp4_append"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        ext.fp4_kvcache_append(_det(k), _det(v), k_cache, k_scale, v_cache, v_scale, cache_seqlens, block_table, cache_batch_idx,
                               _det(k_descale), _det(v_descale), hdim=True)


def mxfp4_decode(q, k_cache, k_scale, v_cache, v_scale, *, cache_seqlens=None, block_table=None, cache_batch_idx=None, q_descale=None,
                 k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0, sinks=None,
                 num_splits=0, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """mxfp4_attn_with_kvcache at head dim d in {64, 128, 256}: q (B, Nq, H_q, d) torch.float8_e4m3fn over the cache of that width, with
    its window_size, softcap, sinks, GQA, cache_seqlens, block_table or cache_batch_idx and num_splits.  Returns o (B, Nq, H_q, d) in
    out_dtype, with return_softmax_lse also lse (B, H_q, Nq) float32."""
    who = "mxfp4_decode"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp4_kvcache_forward(_det(q), k_cache, k_scale, v_cache, v_scale, cache_seqlens, block_table, cache_batch_idx,
                                         _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal), num_splits,
                                         out_dtype, window=_window(who, window_size), softcap=softcap, sinks=_det(sinks), hdim=True)
    return (o, lse) if return_softmax_lse else o


def mxfp4_prefill(q, k_cache, k_scale, v_cache, v_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, block_table,
                  q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                  sinks=None, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """mxfp4_attn_varlen_func at head dim d in {64, 128, 256}: q (total_q, H_q, d) torch.float8_e4m3fn packed by cu_seqlens_q over the
    pools (num_blocks, ps, H_kv, ..) of that width under block_table, ps % 16 == 0, one launch, no workspace.  Returns o (total_q,
    H_q, d) in out_dtype, with return_softmax_lse also lse (H_q, total_q) float32."""
    who = "mxfp4_prefill"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp4_varlen_forward(_det(q), k_cache, k_scale, v_cache, v_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                        block_table, _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal),
                                        out_dtype, window=_window(who, window_size), softcap=softcap, sinks=_det(sinks), hdim=True)
    return (o, lse) if return_softmax_lse else o
