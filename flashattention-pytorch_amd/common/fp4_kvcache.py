"""An MXFP4 KV cache under an fp8 query (C ABI: fa_fp4_kvcache_append, fa_fp4_forward_kvcache, fa_fp4_forward_varlen and their _mod
forms; DESIGN.md sections 9zg, 9zh and 9zi): half the bytes of the e4m3 cache per cached token, read by the matrix instruction in its own format.

    mxfp4_kvcache_append                  16-bit k, v -> e2m1 codes and E8M0 scales at cache_seqlens[b] + i, in place
    fp8_attn_with_mxfp4_kvcache           e4m3 q over that cache: split-KV decoding, fp8_attn_with_kvcache's contract
    fp8_attn_varlen_with_mxfp4_kvcache    packed e4m3 q over the paged cache: chunked prefill, fp8_attn_varlen_func(block_table=)'s
                                          contract, a workgroup of four waves sharing each key tile
    mxfp4_attn_with_kvcache               the decode call with window_size, softcap and sinks (flash_attn_fp8_with_kvcache's semantics)
    mxfp4_attn_varlen_func                the prefill call with the same three: a workgroup walks the key tiles of its band alone

The cache, per K/V head at d = 128:
    k_cache  uint8 (B_cache, cap, H_kv, 64), or a pool (num_blocks, ps, H_kv, 64): two e2m1 codes a byte, the low nibble the even
             channel; code s eem, magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6
    k_scale  uint8 (.., H_kv, 4): one E8M0 byte per 32 channels (an OCP MX block), value 2^(byte - 127)
    v_cache  as k_cache;  v_scale uint8 (.., H_kv): one E8M0 byte per (token, head)
torch.float4_e2m1fn_x2 / torch.float8_e8m0fnu tensors are taken as well where torch has them.  Views at any batch / page / token
strides are used in place (code rows 16-byte aligned, k_scale rows 4-byte aligned).  k_descale / v_descale (and q_descale) are the
float32 (B, H_kv) or (H_kv,) scales of the fp8 calls and carry the global magnitude: value = code * 2^(scale byte - 127) * descale.

Lengths, block_table and cache_batch_idx are untrusted device memory, never read on the host: a captured append + decode replays
after they changed in place.  Refused by name (NotImplementedError) by every call: cache_leftpad, qv, rotary tables, ALiBi, a bias,
head dims other than 128, 16-bit q; by the three older ones also window_size, softcap and sinks (the two mxfp4_attn_* calls take them).  The decode call also refuses cu_seqlens_q / max_seqlen_q
(packed queries are fp8_attn_varlen_with_mxfp4_kvcache's) and block_table with cache_batch_idx; the packed call refuses
cache_batch_idx and cache_seqlens (its lengths are cu_seqlens_k) and needs block_table.  No gradient."""
from __future__ import annotations

import torch

_REFUSED = dict(
    window_size="a sliding window", softcap="a softcap", sinks="attention sinks", cu_seqlens_q="packed queries",
    max_seqlen_q="packed queries", cu_seqlens_k_new="packed new keys", cache_leftpad="cache_leftpad", qv="qv (MLA)",
    rotary_cos="rotary embedding", rotary_sin="rotary embedding", alibi_slopes="ALiBi", attn_bias="an additive bias",
    cache_batch_idx="cache_batch_idx", cache_seqlens="cache_seqlens")


def _refuse(who, unsupported):
    # (the older decode and prefill wrappers name the call that takes the three features; the append has none to name)
    newer = dict(fp8_attn_with_mxfp4_kvcache="mxfp4_attn_with_kvcache", fp8_attn_varlen_with_mxfp4_kvcache="mxfp4_attn_varlen_func").get(who)
    _FEATURED = dict.fromkeys(("window_size", "softcap", "sinks"), newer) if newer else {}
    for name, val in unsupported.items():
        if name not in _REFUSED:
            raise TypeError(f"{who}() got an unexpected keyword argument '{name}'")
        if isinstance(val, torch.Tensor) or val not in (None, False, 0, 0.0, (-1, -1), (None, None)):
            if _REFUSED[name] == "packed queries":
                raise NotImplementedError(f"{who}: {name} is not supported: packed queries over the MXFP4 cache are "
                                          f"fp8_attn_varlen_with_mxfp4_kvcache's (chunked prefill over the paged cache)")
            if name in _FEATURED:
                raise NotImplementedError(f"{who}: {name} is not supported: {_FEATURED[name]} takes {_REFUSED[name]} over the MXFP4 cache")
            raise NotImplementedError(f"{who}: {name} is not supported: the MXFP4 cache calls take no {_REFUSED[name]} (the e4m3 cache "
                                      f"calls of common.fp8_attention do)")


def _det(t):
    return t.detach() if isinstance(t, torch.Tensor) else t


def mxfp4_kvcache_append(k, v, k_cache, k_scale, v_cache, v_scale, *, cache_seqlens, block_table=None, cache_batch_idx=None,
                         k_descale=None, v_descale=None, **unsupported):
    """Append k, v (B, N_new, H_kv, 128) float16 / bfloat16 to the MXFP4 cache at positions cache_seqlens[b] + i (the lengths BEFORE
    the append: int32 (B,) on the device or an int; clamped to [0, capacity] there and not modified).  Per block (32 channels of K,
    the 128 of V) with x' = x * (1 / descale) in float32: e = the smallest integer with 6 * 2^e >= max |x'| in [-64, 64] (0 for an
    all-zero block), scale byte e + 127, code = x' * 2^-e rounded to e2m1 (nearest, ties to the even code).  A token whose position,
    page or cache row falls outside the cache is dropped.  Returns None; the four arrays are written in place."""
    who = "mxfp4_kvcache_append"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        ext.fp4_kvcache_append(_det(k), _det(v), k_cache, k_scale, v_cache, v_scale, cache_seqlens, block_table, cache_batch_idx,
                               _det(k_descale), _det(v_descale))


def fp8_attn_with_mxfp4_kvcache(q, k_cache, k_scale, v_cache, v_scale, *, cache_seqlens=None, block_table=None, cache_batch_idx=None,
                                q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False, num_splits=0,
                                out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """o = softmax(softmax_scale q_descale k_descale q8 (k4 2^ek)^T [causal, bottom-right]) (v4 2^ev v_descale): q (B, Nq, H_q, 128)
    torch.float8_e4m3fn over the MXFP4 cache.  GQA, cache_seqlens (None: full), block_table (ps % 16 == 0) or cache_batch_idx,
    num_splits (0: the library's rule) as in fp8_attn_with_kvcache.  Returns o (B, Nq, H_q, 128) in out_dtype, with
    return_softmax_lse also lse (B, H_q, Nq) float32.  A row without a visible key gives o = 0, lse = -inf."""
    who = "fp8_attn_with_mxfp4_kvcache"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp4_kvcache_forward(_det(q), k_cache, k_scale, v_cache, v_scale, cache_seqlens, block_table, cache_batch_idx,
                                         _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal), num_splits,
                                         out_dtype)
    return (o, lse) if return_softmax_lse else o


def fp8_attn_varlen_with_mxfp4_kvcache(q, k_cache, k_scale, v_cache, v_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *,
                                       block_table, q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False,
                                       out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """Chunked prefill over the paged MXFP4 cache, one launch: q (total_q, H_q, 128) torch.float8_e4m3fn packed by cu_seqlens_q (a
    view such as qkv8[:, 0] is used in place) over the pools (num_blocks, ps, H_kv, ..) mxfp4_kvcache_append fills, under block_table
    int32 (B, max_blocks), ps % 16 == 0.  Sequence b has cu_seqlens_q[b + 1] - cu_seqlens_q[b] queries and cu_seqlens_k[b + 1] -
    cu_seqlens_k[b] keys (slots 0 .. of its pages), both clamped on the device; causal is the bottom-right diagonal of that sequence
    alone; sequences may be empty.  Returns o (total_q, H_q, 128) in out_dtype, with return_softmax_lse also lse (H_q, total_q)
    float32; a row without a visible key gives o = 0, lse = -inf, a row of no sequence is not written.  A contiguous (B, cap, H_kv, ..)
    cache with cap % ps == 0 is already such a pool: pass its arrays as .view(B * cap // ps, ps, H_kv, -1) with block_table =
    arange(B * cap // ps).view(B, -1).  Below about 32 / (H_q / H_kv) query tokens a sequence fp8_attn_with_mxfp4_kvcache, which
    splits the keys, is the faster call."""
    who = "fp8_attn_varlen_with_mxfp4_kvcache"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp4_varlen_forward(_det(q), k_cache, k_scale, v_cache, v_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                        block_table, _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal),
                                        out_dtype)
    return (o, lse) if return_softmax_lse else o


def _window(who, window_size):
    try:
        left, right = window_size
    except (TypeError, ValueError):
        raise RuntimeError(f"{who}: window_size must be a pair (left, right), got {window_size!r}") from None
    return (-1 if left is None else left, -1 if right is None else right)


def mxfp4_attn_with_kvcache(q, k_cache, k_scale, v_cache, v_scale, *, cache_seqlens=None, block_table=None, cache_batch_idx=None,
                            q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1),
                            softcap=0.0, sinks=None, num_splits=0, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """fp8_attn_with_mxfp4_kvcache with a sliding window, a softcap and attention sinks (flash_attn_fp8_with_kvcache's semantics):
    window_size (left, right), -1 = unbounded, bottom-right aligned per sequence: key j is visible to query token i iff i + (len_b -
    Nq) - left <= j <= i + (len_b - Nq) + right (causal sets right = 0); softcap * tanh(s / softcap) on the scaled score before the
    mask (0.0 = off); sinks float32 (H_q,) on q's device, one logit per query head in natural-log units: an extra softmax column
    with a zero value, never capped.  lse contains the sink; a row without a visible key gives o = 0, lse = sink (-inf without
    sinks).  With none of the three the call is fp8_attn_with_mxfp4_kvcache, launch for launch."""
    who = "mxfp4_attn_with_kvcache"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp4_kvcache_forward(_det(q), k_cache, k_scale, v_cache, v_scale, cache_seqlens, block_table, cache_batch_idx,
                                         _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal), num_splits,
                                         out_dtype, window=_window(who, window_size), softcap=softcap, sinks=_det(sinks))
    return (o, lse) if return_softmax_lse else o


def mxfp4_attn_varlen_func(q, k_cache, k_scale, v_cache, v_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, block_table,
                           q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1),
                           softcap=0.0, sinks=None, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """fp8_attn_varlen_with_mxfp4_kvcache with window_size, softcap and sinks as mxfp4_attn_with_kvcache takes them, per sequence (the
    band is aligned to that sequence's own bottom-right corner).  A workgroup reads the key tiles of its rows' band alone, so a
    window of w keys costs O(N w) tiles a sequence.  With none of the three the call is fp8_attn_varlen_with_mxfp4_kvcache."""
    who = "mxfp4_attn_varlen_func"
    _refuse(who, unsupported)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp4_varlen_forward(_det(q), k_cache, k_scale, v_cache, v_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                        block_table, _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal),
                                        out_dtype, window=_window(who, window_size), softcap=softcap, sinks=_det(sinks))
    return (o, lse) if return_softmax_lse else o
