"""The fp8 (e4m3) attention calls at head dims 64, 128 and 256 (C ABI: fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim,
fa_fp8_forward_kvcache_hdim), and what a continuous-batching engine calls once per step (C ABI:
fa_fp8_forward_kvcache_varlen, fa_fp8_kvcache_step_varlen).

    fp8_attn_func                  flash_attn_fp8_func's signature           padded q, k, v
    fp8_attn_varlen_func           flash_attn_fp8_varlen_func's signature    packed q with packed or paged k, v
    fp8_attn_with_kvcache          flash_attn_fp8_with_kvcache's signature   split-KV decoding over an e4m3 cache
    fp8_attn_with_kvcache_varlen   the same with packed queries (cu_seqlens_q, max_seqlen_q): a ragged batch in one call
    fp8_attn_kvcache_step          flash_attn_fp8_kvcache_step's signature   append + rotary + quantise q + attend, at 64 / 128 / 256,
                                   with packed queries and packed or padded new keys (cu_seqlens_q, cu_seqlens_k_new)

The packed calls follow FlashAttention-3's convention as flash_attn_with_kvcache(cu_seqlens_q=) states it: q is (total_q, H_q, d),
sequence b owns tokens [cu_seqlens_q[b], cu_seqlens_q[b + 1]), at most max_seqlen_q, and gets bit for bit what the padded call
returns for it alone; o is (total_q, H_q, d), lse (H_q, total_q); rows no sequence owns keep their contents.  A chunk of n tokens
reads its keys ceil(n * G / 32) times: for long prefill chunks fp8_attn_varlen_func(block_table=) is the call.

Each is its namesake in common/attention_ex.py, whose docstring holds with the head dim d in {64, 128, 256} where it says 128:
q, k and v (or q and the caches) agree in their last extent, softmax_scale defaults to d ** -0.5, o is d wide.  The sliding
window, the softcap and the sinks, GQA, Nq != Nk with the bottom-right diagonal, strided views, paging, cache_batch_idx,
split-KV and graph replay are what they are at 128.  At d = 128 the result is the older function's to the bit (the library runs
the same launches); the older functions keep refusing every other head dim.  gpt-oss (sinks, a 128-token window) has d = 64,
Gemma-2 / 3 (a softcap, an alternating window) d = 256.

A d = 64 / 256 cache is filled by flash_attn_with_kvcache(..., k=, v=, k_descale=, v_descale=), q comes from quantize_fp8: both
take these widths.  Refused by name (NotImplementedError): head dims other than 64, 128, 256 (96 and 192 among them), 16-bit or
float32 inputs, out_dtype other than bfloat16 / float16, and everything the namesake refuses; q, k, v of different head dims are a
RuntimeError that names them.  The older fused decode step flash_attn_fp8_kvcache_step, fa3_attention(fp8=True) and the MLA /
indexer calls stay at their own head dims.  Still refused by name: cache_leftpad, qv, alibi_slopes, attn_bias, mask, dropout_p,
head dims 96 / 192, block_table together with cache_batch_idx.  No gradient."""
from __future__ import annotations

import torch

from common import attention_ex as _ex

HEAD_DIMS = (64, 128, 256)


def _check(who, hint, **tensors):
    """the refusals that come before the shim's: tensors, e4m3, one head dim of HEAD_DIMS"""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype in (torch.float16, torch.bfloat16, torch.float32):
            raise NotImplementedError(f"{who}: 16-bit inputs are not supported: {name} is {t.dtype}, torch.float8_e4m3fn expected "
                                      f"({hint})")
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
    dims = {name: t.shape[-1] for name, t in tensors.items() if t.dim() >= 1}
    if len(set(dims.values())) > 1:
        raise RuntimeError(f"{who}: mixed head dims: " + ", ".join(f"{name} has {d}" for name, d in dims.items()) +
                           " (q, k and v must agree in their last extent)")
    for d in dims.values():
        if d not in HEAD_DIMS:
            raise NotImplementedError(f"{who}: head_dim {d} is not supported (64, 128 or 256)")


def _out_dtype(who, out_dtype):
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")


def _det(t):
    return t.detach() if isinstance(t, torch.Tensor) else t


def fp8_attn_func(q, k, v, *, q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False,
                  window_size=(-1, -1), softcap=0.0, sinks=None, out_dtype=torch.bfloat16, layout="bhnd", return_lse=False,
                  **unsupported):
    """flash_attn_fp8_func at head dims 64, 128 and 256: q (B, H_q, Nq, d), k and v (B, H_kv, Nk, d) in torch.float8_e4m3fn
    (layout="bnhd": (B, N, H, d)).  Returns o in `layout` and out_dtype, with return_lse also lse (B, H_q, Nq) float32."""
    who = "fp8_attn_func"
    _ex._fp8_refuse(who, tuple(n for n in _ex._FP8_REFUSED if n not in _ex._FP8_MOD_ARGS), unsupported, "call")
    mod = _ex._fp8_mod_args(who, window_size, softcap, sinks)
    _check(who, "quantise first (quantize_fp8_qkv), or use flash_attention_ex", q=q, k=k, v=v)
    _out_dtype(who, out_dtype)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp8_forward(q.detach(), k.detach(), v.detach(), bool(causal), softmax_scale, _det(q_descale), _det(k_descale),
                                 _det(v_descale), out_dtype, layout, hdim=True, **mod)
    return (o, lse) if return_lse else o


def fp8_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, block_table=None, q_descale=None,
                         k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                         sinks=None, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """flash_attn_fp8_varlen_func at head dims 64, 128 and 256: q (total_q, H_q, d) e4m3 packed by cu_seqlens_q; k and v
    (total_k, H_kv, d), or with block_table the pools (num_blocks, ps, H_kv, d).  Returns o (total_q, H_q, d) in out_dtype, with
    return_softmax_lse also lse (H_q, total_q) float32."""
    who = "fp8_attn_varlen_func"
    _ex._fp8_refuse(who, tuple(n for n in _ex._FP8_VARLEN_REFUSED if n not in _ex._FP8_MOD_ARGS), unsupported, "call")
    mod = _ex._fp8_mod_args(who, window_size, softcap, sinks)
    _check(who, "quantise first (quantize_fp8_qkv), or use flash_attention_varlen", q=q, k=k, v=v)
    _out_dtype(who, out_dtype)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        raise RuntimeError(f"{who}: forward only — q, k or v requires grad and the fp8 call has no backward (call it under "
                           f"torch.no_grad(), or detach the tensors)")
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp8_varlen_forward(q.detach(), k.detach(), v.detach(), cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                        bool(causal), softmax_scale, _det(q_descale), _det(k_descale), _det(v_descale), out_dtype,
                                        block_table, hdim=True, **mod)
    return (o, lse) if return_softmax_lse else o


def fp8_attn_with_kvcache(q, k_cache, v_cache, *, cache_seqlens=None, block_table=None, cache_batch_idx=None, q_descale=None,
                          k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                          sinks=None, num_splits=0, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """flash_attn_fp8_with_kvcache at head dims 64, 128 and 256: q (B, Nq, H_q, d) e4m3 over the e4m3 caches
    (B_cache, cache_len, H_kv, d), or with block_table the pools (num_blocks, ps, H_kv, d).  Returns o (B, Nq, H_q, d) in
    out_dtype, with return_softmax_lse also lse (B, H_q, Nq) float32."""
    who = "fp8_attn_with_kvcache"
    _ex._fp8_refuse(who, tuple(n for n in _ex._FP8_KVCACHE_REFUSED if n not in _ex._FP8_MOD_ARGS), unsupported, "decode call")
    mod = _ex._fp8_mod_args(who, window_size, softcap, sinks)
    _check(who, "a 16-bit q over an e4m3 cache is flash_attn_with_kvcache(..., k_descale=, v_descale=)", q=q, k_cache=k_cache,
           v_cache=v_cache)
    if block_table is not None and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    _out_dtype(who, out_dtype)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp8_kvcache_forward(q.detach(), k_cache.detach(), v_cache.detach(), cache_seqlens, block_table, cache_batch_idx,
                                         _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal), num_splits,
                                         out_dtype, hdim=True, **mod)
    return (o, lse) if return_softmax_lse else o


_PACKED_NAMES = ("cu_seqlens_q", "max_seqlen_q", "cu_seqlens_k_new")


def fp8_attn_with_kvcache_varlen(q, k_cache, v_cache, *, cu_seqlens_q, max_seqlen_q, cache_seqlens=None, block_table=None,
                                 cache_batch_idx=None, q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False,
                                 window_size=(-1, -1), softcap=0.0, sinks=None, num_splits=0, out_dtype=torch.bfloat16,
                                 return_softmax_lse=False, **unsupported):
    """fp8_attn_with_kvcache on packed queries: q (total_q, H_q, d) e4m3, a view such as qkv[:, 0] used at its own token stride;
    cu_seqlens_q int32 (B + 1,) on the device (untrusted, clamped there, never read on the host), max_seqlen_q an int.  Sequence b
    attends over len_b = clamp(cache_seqlens[b], 0, capacity) cached keys with the causal diagonal len_b - nq_b, exactly as
    fp8_attn_with_kvcache on it alone with the same num_splits.  num_splits=0 is the rule over the dense max_seqlen_q grid, which
    cannot see the lengths: a step of many one-token rows beside one long chunk gets too few splits and should pass num_splits.  Returns o
    (total_q, H_q, d) in out_dtype, with return_softmax_lse also lse (H_q, total_q) float32."""
    who = "fp8_attn_with_kvcache_varlen"
    _ex._fp8_refuse(who, tuple(n for n in _ex._FP8_KVCACHE_REFUSED if n not in _ex._FP8_MOD_ARGS + _PACKED_NAMES), unsupported, "decode call")
    mod = _ex._fp8_mod_args(who, window_size, softcap, sinks)
    _check(who, "a 16-bit q over an e4m3 cache is flash_attn_with_kvcache(..., k_descale=, v_descale=)", q=q, k_cache=k_cache,
           v_cache=v_cache)
    if cu_seqlens_q is None:
        raise RuntimeError(f"{who}: cu_seqlens_q is required (padded queries: fp8_attn_with_kvcache)")
    if block_table is not None and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    _out_dtype(who, out_dtype)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp8_kvcache_forward(q.detach(), k_cache.detach(), v_cache.detach(), cache_seqlens, block_table, cache_batch_idx,
                                         _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal), num_splits,
                                         out_dtype, hdim=True, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, **mod)
    return (o, lse) if return_softmax_lse else o


def fp8_attn_kvcache_step(q, k_cache, v_cache, k, v, *, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, cache_seqlens,
                          block_table=None, cache_batch_idx=None, q_descale=None, k_descale=None, v_descale=None, softmax_scale=None,
                          causal=False, window_size=(-1, -1), softcap=0.0, sinks=None, num_splits=0, out_dtype=None, q8_out=None,
                          return_softmax_lse=False, cu_seqlens_q=None, max_seqlen_q=None, cu_seqlens_k_new=None, **unsupported):
    """flash_attn_fp8_kvcache_step at head dims 64, 128 and 256, with packed queries and new keys; its docstring holds with d where
    it says 128 (rotary_dim up to d, softmax_scale defaults to d ** -0.5).  cu_seqlens_q (with max_seqlen_q): q is (total_q, H_q, d),
    q8_out and o likewise, lse (H_q, total_q).  cu_seqlens_k_new (needs cu_seqlens_q): k, v are (total_k_new, H_kv, d); without it
    they are padded (B, N_new, H_kv, d).  Per sequence L_b = clamp(cache_seqlens[b], 0, capacity - nnew_b), new key n sits (and is
    rotated) at L_b + n, q token i is rotated at L_b + i when causal or a window bound is given, else at L_b; a sequence without
    query tokens still appends, one without new keys appends nothing.  Both offset arrays are untrusted device memory.  Without the
    three packed arguments at d = 128 the call IS flash_attn_fp8_kvcache_step, launch for launch."""
    who = "fp8_attn_kvcache_step"
    _ex._fp8_refuse(who, tuple(n for n in _ex._FP8_STEP_REFUSED if n not in _PACKED_NAMES), unsupported, "decode step")
    if k is None or v is None:
        raise NotImplementedError(f"{who}: k / v missing: the step appends new tokens (attention over the cache as it is: "
                                  f"fp8_attn_with_kvcache_varlen)")
    tensors = dict(q=q, k=k, v=v, k_cache=k_cache, v_cache=v_cache)
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    dims = {name: t.shape[-1] for name, t in tensors.items() if t.dim() >= 1}
    if len(set(dims.values())) > 1:
        raise RuntimeError(f"{who}: mixed head dims: " + ", ".join(f"{name} has {d}" for name, d in dims.items()) +
                           " (q, k, v and the caches must agree in their last extent)")
    for d in dims.values():
        if d not in HEAD_DIMS:
            raise NotImplementedError(f"{who}: head_dim {d} is not supported (64, 128 or 256)")
    if q.dtype not in (torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (float16, bfloat16 or torch.float8_e4m3fn)")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise NotImplementedError(f"{who}: mixed dtypes are not supported: q, k, v must be all float16, all bfloat16 or all "
                                  f"torch.float8_e4m3fn (got {q.dtype}, {k.dtype}, {v.dtype})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
    if q.dtype == torch.float8_e4m3fn:
        for name, val in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin), ("q8_out", q8_out)):
            if val is not None:
                raise NotImplementedError(f"{who}: {name} is not supported with torch.float8_e4m3fn q, k, v (the codes are used as they are)")
    if block_table is not None and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    if out_dtype is not None:
        _out_dtype(who, out_dtype)
    mod = _ex._fp8_mod_args(who, window_size, softcap, sinks)
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp8_kvcache_step(q.detach(), k_cache.detach(), v_cache.detach(), k.detach(), v.detach(), cache_seqlens, block_table,
                                      cache_batch_idx, _det(q_descale), _det(k_descale), _det(v_descale), softmax_scale, bool(causal),
                                      num_splits, out_dtype, rotary_cos=_det(rotary_cos), rotary_sin=_det(rotary_sin),
                                      rotary_interleaved=bool(rotary_interleaved), q8_out=_det(q8_out), cu_seqlens_q=cu_seqlens_q,
                                      max_seqlen_q=max_seqlen_q, cu_seqlens_k_new=cu_seqlens_k_new, hdim=True, **mod)
    return (o, lse) if return_softmax_lse else o
