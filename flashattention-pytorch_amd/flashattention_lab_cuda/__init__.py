"""`flashattention_lab_cuda` — the extension module the reference's wrappers look up by name
(`/root/reference/src/fa2/cuda/impl.py:10`), re-created as a thin ctypes shim over the C-ABI
library `libfa_mi355x.so` (declared in `include/fa_mi355x.h`, built from `csrc/`).

Exports exactly the six names of `/root/reference/csrc/common/torch.extension.cpp:73-83` with the
same positional signatures:

    fa1_forward / forward (q, k, v, causal, softmax_scale, br, bc)              -> (o, lse)
    fa1_backward / backward (q, k, v, o, do_, lse, causal, softmax_scale, br, bc) -> (dq, dk, dv)
    fa3_forward (q, k, v, causal, softmax_scale, br, bc, stages, fp8)           -> (o, lse)
    fa3_backward(q, k, v, o, do_, lse, causal, softmax_scale, br, bc, stages, fp8) -> (dq, dk, dv)

As in the reference (`csrc/fa2/fa2_fwd.cu:38-54`, `fa2_bwd.cu:112-115`): inputs are (BH, N, d) device
tensors, `o` and the gradients come back in the input dtype, `lse` is float32, nothing is recorded by
autograd, inputs are never modified, and shape errors raise RuntimeError.  PyTorch is used only to
allocate the outputs / workspace and to name the current HIP stream; all compute is in the HIP library.
There is NO CPU fallback: a missing library or a non-device tensor is an error.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import os
import operator

import torch

from .workspace import WorkspaceCache, plan_backward_workspace

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libfa_mi355x.so")

_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

EXPORTED_C_SYMBOLS = (
    "fa1_forward", "fa1_backward", "fa2_forward", "fa2_backward", "fa3_forward", "fa3_backward",
    "fa_backward_workspace_bytes", "fa_backward_workspace_bytes_fast", "fa3_forward_workspace_bytes", "fa3_backward_workspace_bytes", "fa_last_error", "fa_version",
    "fa_set_kernel_mode", "fa_set_option", "fa_debug_trace_buffer", "fa_device_is_gfx950", "fa_profile_enable", "fa_profile_report", "fa_route_count",
    "fa_ex_forward", "fa_ex_backward", "fa_ex_backward_workspace_bytes", "fa_ex_backward_workspace_bytes_fast",
    "fa_ex_forward_grouped", "fa_ex_backward_grouped", "fa_ex_backward_workspace_bytes_grouped",
    "fa_ex_backward_workspace_bytes_fast_grouped", "fa_ex_forward_window", "fa_ex_backward_window",
    "fa_ex_forward_varlen", "fa_ex_backward_varlen", "fa_ex_backward_workspace_bytes_varlen",
    "fa_ex_forward_scoremod", "fa_ex_backward_scoremod", "fa_ex_forward_varlen_scoremod", "fa_ex_backward_varlen_scoremod",
    "fa_ex_forward_kvcache", "fa_ex_kvcache_workspace_bytes", "fa_ex_forward_kvcache_paged", "fa_ex_forward_kvcache_rotary",
    "fa_ex_forward_kvcache_fp8",
    "fa_ex_forward_sink", "fa_ex_backward_sink", "fa_ex_forward_varlen_sink", "fa_ex_backward_varlen_sink",
    "fa_ex_forward_kvcache_sink", "fa_ex_kvcache_workspace_bytes_sink",
    "fa_ex_forward_kvcache_varlen", "fa_ex_kvcache_workspace_bytes_varlen",
    "fa_ex_forward_kvcache_qv", "fa_ex_kvcache_workspace_bytes_qv",
    "fa_ex_forward_varlen_paged", "fa_ex_forward_varlen_paged_fp8",
    "fa_rotary_apply",
    "fa_ex_backward_dlse", "fa_ex_backward_varlen_dlse", "fa_merge_states", "fa_merge_states_backward",
    "fa_mla_sparse_forward", "fa_mla_sparse_workspace_bytes",
    "fa_mla_fp8_forward", "fa_mla_fp8_workspace_bytes", "fa_mla_fp8_pack",
    "fa_indexer_pack", "fa_indexer_logits", "fa_indexer_topk",
    "fa_ex_forward_vdim", "fa_ex_backward_vdim", "fa_ex_forward_varlen_vdim", "fa_ex_backward_varlen_vdim",
    "fa_ex_forward_bias", "fa_ex_backward_bias", "fa_ex_backward_workspace_bytes_bias",
    "fa_fp8_forward", "fa_fp8_forward_workspace_bytes",
    "fa_fp8_forward_varlen", "fa_fp8_forward_varlen_workspace_bytes",
    "fa_fp8_forward_kvcache", "fa_fp8_forward_kvcache_workspace_bytes",
    "fa_fp8_forward_mod", "fa_fp8_forward_varlen_mod", "fa_fp8_forward_kvcache_mod", "fa_fp8_forward_kvcache_workspace_bytes_mod",
    "fa_fp8_quantize", "fa_fp8_quantize_workspace_bytes",
    "fa_fp8_kvcache_step", "fa_fp8_kvcache_step_workspace_bytes",
    "fa_fp8_forward_hdim", "fa_fp8_forward_varlen_hdim", "fa_fp8_forward_kvcache_hdim",
    "fa_fp8_forward_hdim_workspace_bytes", "fa_fp8_forward_varlen_hdim_workspace_bytes", "fa_fp8_forward_kvcache_hdim_workspace_bytes",
    "fa_fp8_forward_kvcache_varlen", "fa_fp8_forward_kvcache_varlen_workspace_bytes",
    "fa_fp8_kvcache_step_varlen", "fa_fp8_kvcache_step_varlen_workspace_bytes",
)


# ---- the C signatures (include/fa_mi355x.h): for each exported function its return type and its ordered (field, ctype) parameters,
# composed from named groups.  An argument group a feature adds is one new group here, appended where the header has it.
_TYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int64, "c": ctypes.c_int, "d": ctypes.c_double, "u": ctypes.c_uint64, "z": ctypes.c_size_t,
          "s": ctypes.c_char_p}


def _fields(spec):
    """'p:q,k i:bh' -> (("q", c_void_p), ("k", c_void_p), ("bh", c_int64))"""
    return tuple((name, _TYPES[group[0]]) for group in spec.split() for name in group[2:].split(","))


_FWD = _fields("p:q,k,v,o,lse")
_BWD = _fields("p:q,k,v,o,do_,lse,dq,dk,dv")                 # the nine backward pointers
_STREAM = _fields("p:stream")
_WS = _fields("p:workspace z:workspace_bytes p:stream")
_BHND = _fields("i:bh,n,d c:dtype")
_PLAIN = _BHND + _fields("c:causal d:softmax_scale i:br,bc")   # fa1 / fa2 / fa3
_FA3 = _fields("i:stages c:fp8")
_GROUP = _fields("i:kv_group")
_EXDIMS = _fields("i:nq,nk,d c:dtype")
_WINDOW = _fields("i:window_left,window_right")
_SCALE = _fields("d:softmax_scale")
_MOD = _fields("d:softcap p:alibi_slopes i:alibi_heads,alibi_batch_stride")
_MODH = _fields("d:softcap p:alibi_slopes i:alibi_batch_stride")   # varlen and KV-cache: one slope per query head
_SINK = _fields("p:sinks i:sink_heads")
_DSINK = _fields("p:dsinks")
_DLSE = _fields("p:dlse")                                     # the gradient of lse, after the sink group
_VDIM = _fields("i:d_v")                                      # the width of v, o, do_, dv (0: d), after the sink / dlse group
_BIAS = _fields("p:bias i:bias_heads,bias_batch_stride,bias_head_stride,bias_row_stride")   # an additive bias, after d_v
_DBIAS = _fields("p:dbias i:dbias_batch_stride,dbias_head_stride,dbias_row_stride")          # its gradient (backward)
_MASKS = _fields("p:mask i:mask_bh_stride p:block_mask i:br,bc")
_DROPOUT = _fields("d:dropout_p u:dropout_seed")
_VARLEN = _fields("p:cu_seqlens_q,cu_seqlens_k i:batch,heads_q,heads_kv,total_q,total_k,max_seqlen_q,max_seqlen_k,d c:dtype "
                  "i:q_stride,k_stride,v_stride c:causal") + _WINDOW + _SCALE
_VPAGED = _fields("p:block_table i:max_blocks_per_seq,num_blocks,page_block_size,k_page_stride,v_page_stride")
_FP8 = _fields("c:cache_dtype p:k_descale,v_descale i:descale_batch_stride")
_KV = _fields("p:q,k_cache,v_cache,k_new,v_new,cache_seqlens,o,lse i:batch,heads_q,heads_kv,seqlen_q,seqlen_new,cache_len,d c:dtype "
              "i:q_batch_stride,q_token_stride,k_cache_batch_stride,k_cache_token_stride,v_cache_batch_stride,v_cache_token_stride,"
              "k_new_batch_stride,k_new_token_stride,v_new_batch_stride,v_new_token_stride c:causal") + _WINDOW + _SCALE + _MODH + \
    _fields("i:num_splits")
_PAGED = _fields("p:block_table i:block_table_row_stride,num_blocks,page_block_size,max_blocks_per_seq p:cache_batch_idx i:cache_batch "
                 "p:cache_leftpad")
_ROTARY = _fields("p:rotary_cos,rotary_sin i:rotary_cos_row_stride,rotary_sin_row_stride,seqlen_ro,rotary_dim c:rotary_interleaved")
_KVVARLEN = _fields("p:cu_seqlens_q,cu_seqlens_k_new i:total_q,max_seqlen_q,total_k_new")
_KVQV = _fields("p:qv i:qv_batch_stride,qv_token_stride,d_v")
_KVWS = _fields("i:batch,heads_q,heads_kv,seqlen_q,cache_len,d,num_splits")
_ROXY = _fields("p:x,y i:batch,seqlen,heads,d c:dtype i:x_batch_stride,x_token_stride,y_batch_stride,y_token_stride")
_ROPOS = _fields("c:conjugate i:seqlen_offset p:seqlen_offsets,cu_seqlens i:total,max_seqlen")
_MDIMS = _fields("i:batch,heads,rows,d c:dtype")


def _strides(*tensors):
    """the (batch, head, row) stride triple of each named tensor of the merge calls"""
    return sum((_fields(f"i:{t}_batch_stride,{t}_head_stride,{t}_row_stride") for t in tensors), ())


_SIGNATURES = {}


def _sig(names, fields, restype=ctypes.c_int):
    for name in names.split():
        _SIGNATURES[name] = (restype, fields)


def _ex_sig(ptrs, tail, group=(), window=(), mod=()):
    return ptrs + _fields("i:bh") + group + _EXDIMS + _fields("c:causal") + window + _SCALE + mod + _MASKS + _DROPOUT + tail


_SIZE = ctypes.c_size_t
_sig("fa1_forward fa2_forward", _FWD + _PLAIN + _STREAM)
_sig("fa1_backward fa2_backward", _BWD + _PLAIN + _WS)
_sig("fa3_forward", _FWD + _PLAIN + _FA3 + _WS)
_sig("fa3_backward", _BWD + _PLAIN + _FA3 + _WS)
_sig("fa_backward_workspace_bytes", _BHND, _SIZE)
_sig("fa_backward_workspace_bytes_fast", _BHND + _fields("c:causal"), _SIZE)
_sig("fa3_forward_workspace_bytes fa3_backward_workspace_bytes", _BHND + _fields("c:fp8"), _SIZE)
_sig("fa_last_error fa_version", (), ctypes.c_char_p)
_sig("fa_set_kernel_mode", _fields("c:mode"))
_sig("fa_set_option", _fields("s:name c:value"))
_sig("fa_debug_trace_buffer", _fields("p:device_ptr"))
_sig("fa_device_is_gfx950", _fields("c:device"))
_sig("fa_profile_enable", _fields("c:on"))
_sig("fa_profile_report", _fields("s:buf z:cap"))
_sig("fa_route_count", _fields("s:name"), ctypes.c_int64)
for _dir, _ptrs, _tail, _ds in (("forward", _FWD, _STREAM, ()), ("backward", _BWD, _WS, _DSINK)):
    _sig(f"fa_ex_{_dir}", _ex_sig(_ptrs, _tail))
    _sig(f"fa_ex_{_dir}_grouped", _ex_sig(_ptrs, _tail, _GROUP))
    _sig(f"fa_ex_{_dir}_window", _ex_sig(_ptrs, _tail, _GROUP, _WINDOW))
    _sig(f"fa_ex_{_dir}_scoremod", _ex_sig(_ptrs, _tail, _GROUP, _WINDOW, _MOD))
    _sig(f"fa_ex_{_dir}_sink", _ex_sig(_ptrs, _tail, _GROUP, _WINDOW, _MOD + _SINK + _ds))
    _sig(f"fa_ex_{_dir}_varlen", _ptrs + _VARLEN + _DROPOUT + _tail)
    _sig(f"fa_ex_{_dir}_varlen_scoremod", _ptrs + _VARLEN + _MODH + _DROPOUT + _tail)
    _sig(f"fa_ex_{_dir}_varlen_sink", _ptrs + _VARLEN + _MODH + _SINK + _ds + _DROPOUT + _tail)
_sig("fa_ex_backward_dlse", _ex_sig(_BWD, _WS, _GROUP, _WINDOW, _MOD + _SINK + _DSINK + _DLSE))
_sig("fa_ex_backward_varlen_dlse", _BWD + _VARLEN + _MODH + _SINK + _DSINK + _DLSE + _DROPOUT + _WS)
_sig("fa_ex_forward_vdim", _ex_sig(_FWD, _STREAM, _GROUP, _WINDOW, _MOD + _SINK + _VDIM))
_sig("fa_ex_backward_vdim", _ex_sig(_BWD, _WS, _GROUP, _WINDOW, _MOD + _SINK + _DSINK + _DLSE + _VDIM))
_sig("fa_ex_forward_varlen_vdim", _FWD + _VARLEN + _MODH + _SINK + _VDIM + _DROPOUT + _STREAM)
_sig("fa_ex_backward_varlen_vdim", _BWD + _VARLEN + _MODH + _SINK + _DSINK + _DLSE + _VDIM + _DROPOUT + _WS)
_sig("fa_ex_forward_bias", _ex_sig(_FWD, _STREAM, _GROUP, _WINDOW, _MOD + _SINK + _VDIM + _BIAS))
_sig("fa_ex_backward_bias", _ex_sig(_BWD, _WS, _GROUP, _WINDOW, _MOD + _SINK + _DSINK + _DLSE + _VDIM + _BIAS + _DBIAS))
_sig("fa_ex_backward_workspace_bytes_bias", _fields("i:bh") + _GROUP + _EXDIMS + _fields("c:dbias_reduced"), _SIZE)
_sig("fa_ex_forward_varlen_paged", _FWD + _VARLEN + _MODH + _SINK + _VPAGED + _STREAM)
_sig("fa_ex_forward_varlen_paged_fp8", _FWD + _VARLEN + _MODH + _SINK + _VPAGED + _FP8 + _STREAM)
_sig("fa_ex_backward_workspace_bytes", _fields("i:bh") + _EXDIMS, _SIZE)
_sig("fa_ex_backward_workspace_bytes_fast", _fields("i:bh") + _EXDIMS + _fields("c:causal,extras"), _SIZE)
_sig("fa_ex_backward_workspace_bytes_grouped", _fields("i:bh") + _GROUP + _EXDIMS, _SIZE)
_sig("fa_ex_backward_workspace_bytes_fast_grouped", _fields("i:bh") + _GROUP + _EXDIMS + _fields("c:causal,extras"), _SIZE)
_sig("fa_ex_backward_workspace_bytes_varlen", _fields("i:heads_q,heads_kv,total_q,total_k,d c:dtype"), _SIZE)
_kv = _KV   # each KV-cache entry point: the one before it and one more group, in front of the workspace
for _suffix, _added in (("", ()), ("_paged", _PAGED), ("_rotary", _ROTARY), ("_fp8", _FP8), ("_sink", _SINK), ("_varlen", _KVVARLEN),
                        ("_qv", _KVQV)):
    _kv += _added
    _sig("fa_ex_forward_kvcache" + _suffix, _kv + _WS)
_sig("fa_ex_kvcache_workspace_bytes fa_ex_kvcache_workspace_bytes_sink", _KVWS, _SIZE)
_sig("fa_rotary_apply", _ROXY + _ROTARY + _ROPOS + _STREAM)
_sig("fa_merge_states", _fields("p:o_a,lse_a,o_b,lse_b,o,lse") + _MDIMS + _strides("o_a", "lse_a", "o_b", "lse_b", "o", "lse") + _STREAM)
_sig("fa_merge_states_backward", _fields("p:o_a,lse_a,o_b,lse_b,do_,dlse,do_a,do_b,dlse_a,dlse_b") + _MDIMS +
     _strides("o_a", "lse_a", "o_b", "lse_b", "do", "dlse", "do_a", "do_b", "dlse_a", "dlse_b") + _STREAM)
_sig("fa_mla_sparse_forward", _fields(
    "p:q,qv,k_cache,v_cache,indices,cache_seqlens,o,lse i:batch,heads_q,heads_kv,seqlen_q,cache_len,topk,d,d_v c:dtype "
    "i:q_batch_stride,q_token_stride,qv_batch_stride,qv_token_stride,k_cache_batch_stride,k_cache_token_stride,v_cache_batch_stride,"
    "v_cache_token_stride,indices_batch_stride,indices_token_stride,indices_head_stride c:causal d:softmax_scale i:num_splits "
    "p:block_table i:block_table_row_stride,num_blocks,page_block_size,max_blocks_per_seq p:cache_batch_idx i:cache_batch") + _WS)
_sig("fa_mla_sparse_workspace_bytes", _fields("i:batch,heads_q,heads_kv,seqlen_q,topk,num_splits"), _SIZE)
_F8POOL = _fields("i:page_stride_bytes,token_stride_bytes")
_F8PAGES = _fields("i:block_table_row_stride,num_blocks,page_block_size,max_blocks_per_seq")
_sig("fa_mla_fp8_forward", _fields(
    "p:q,qv,kv_cache,indices,cache_seqlens,block_table,o,lse i:batch,heads_q,heads_kv,seqlen_q,topk,d,d_v c:dtype "
    "i:q_batch_stride,q_token_stride,q_head_stride,qv_batch_stride,qv_token_stride,qv_head_stride") + _F8POOL + _fields("i:indices_batch_stride,indices_token_stride") +
     _F8PAGES + _fields("c:causal d:softmax_scale i:num_splits") + _WS)
_sig("fa_mla_fp8_workspace_bytes", _fields("i:batch,heads_q,heads_kv,seqlen_q,cache_len,topk c:with_indices i:num_splits"), _SIZE)
_sig("fa_mla_fp8_pack", _fields(
    "p:latent_new,rope_new,kv_cache,cache_seqlens,block_table i:batch,seqlen_new,latent_batch_stride,latent_token_stride,"
    "rope_batch_stride,rope_token_stride") + _F8POOL + _F8PAGES + _fields("c:scale_pow2") + _STREAM)
_sig("fa_indexer_pack", _fields("p:k_new,k_cache,cache_seqlens,block_table i:batch,seqlen_new,d,k_new_batch_stride,k_new_token_stride") +
     _F8POOL + _F8PAGES + _fields("c:scale_pow2") + _STREAM)
_sig("fa_indexer_logits", _fields(
    "p:q,weights,k_cache,cache_seqlens,block_table,logits i:batch,seqlen_q,heads,d,width,q_batch_stride,q_token_stride,q_head_stride,"
    "weights_batch_stride,weights_token_stride,logits_batch_stride,logits_row_stride") + _F8POOL + _F8PAGES + _fields("c:causal") + _STREAM)
_sig("fa_indexer_topk", _fields("p:logits,cache_seqlens,indices i:batch,seqlen_q,width,topk,logits_batch_stride,logits_row_stride,"
                                "indices_batch_stride,indices_token_stride c:causal") + _STREAM)
_sig("fa_fp8_forward", _fields("p:q,k,v,o,lse,q_descale,k_descale,v_descale i:batch,heads_q,heads_kv,seqlen_q,seqlen_k,d c:dtype "
                               "i:q_batch_stride,q_head_stride,q_token_stride,k_batch_stride,k_head_stride,k_token_stride,v_batch_stride,"
                               "v_head_stride,v_token_stride,o_batch_stride,o_head_stride,o_token_stride,q_descale_batch_stride,"
                               "k_descale_batch_stride,v_descale_batch_stride c:causal d:softmax_scale") + _WS)
_sig("fa_fp8_forward_workspace_bytes", _fields("i:batch,heads_kv,seqlen_k,d"), _SIZE)
_sig("fa_fp8_forward_varlen", _fields(
    "p:q,k,v,o,lse,q_descale,k_descale,v_descale,cu_seqlens_q,cu_seqlens_k,block_table "
    "i:batch,heads_q,heads_kv,total_q,total_k,max_seqlen_q,max_seqlen_k,d c:dtype "
    "i:q_token_stride,q_head_stride,k_token_stride,k_head_stride,v_token_stride,v_head_stride,max_blocks_per_seq,num_blocks,"
    "page_block_size,k_page_stride,v_page_stride,q_descale_batch_stride,k_descale_batch_stride,v_descale_batch_stride "
    "c:causal d:softmax_scale") + _WS)
_sig("fa_fp8_forward_varlen_workspace_bytes", _fields("i:batch,heads_kv,total_k,max_seqlen_k,max_blocks_per_seq,page_block_size,d"), _SIZE)
_sig("fa_fp8_forward_kvcache", _fields(
    "p:q,k_cache,v_cache,o,lse,q_descale,k_descale,v_descale,cache_seqlens,block_table,cache_batch_idx "
    "i:batch,heads_q,heads_kv,seqlen_q,cache_len,cache_batch,d c:dtype,q_dtype,cache_dtype "
    "i:q_batch_stride,q_token_stride,k_batch_stride,k_token_stride,v_batch_stride,v_token_stride,block_table_row_stride,num_blocks,"
    "page_block_size,q_descale_batch_stride,k_descale_batch_stride,v_descale_batch_stride c:causal d:softmax_scale i:num_splits") + _WS)
_sig("fa_fp8_forward_kvcache_workspace_bytes", _KVWS, _SIZE)
# a window, a softcap and sinks on the three fp8 calls: the parent's arguments, then one more group
_FP8MOD = _WINDOW + _fields("d:softcap") + _SINK
for _name in ("fa_fp8_forward", "fa_fp8_forward_varlen", "fa_fp8_forward_kvcache"):
    _sig(_name + "_mod", _SIGNATURES[_name][1] + _FP8MOD)
_sig("fa_fp8_forward_kvcache_workspace_bytes_mod", _KVWS + _fields("c:causal") + _WINDOW + _fields("c:with_sinks"), _SIZE)
_sig("fa_fp8_quantize", _fields("p:x,out,descale,descale_out,cu_seqlens") + _ROTARY + _fields(
    "i:seqlen_offset p:seqlen_offsets i:batch,heads,seqlen,d,heads_per_scale,total,max_seqlen c:dtype "
    "i:x_batch_stride,x_head_stride,x_token_stride,out_batch_stride,out_head_stride,out_token_stride,descale_batch_stride "
    "c:scale_pow2") + _WS)
_sig("fa_fp8_quantize_workspace_bytes", _fields("i:batch,heads,heads_per_scale"), _SIZE)
# the fp8 decode step: fa_fp8_forward_kvcache_mod's arguments, then the new tokens, in_dtype, the q8 buffer and the rotary group
_sig("fa_fp8_kvcache_step", _SIGNATURES["fa_fp8_forward_kvcache_mod"][1] + _fields(
    "p:k_new,v_new i:seqlen_new,k_new_batch_stride,k_new_token_stride,v_new_batch_stride,v_new_token_stride c:in_dtype "
    "p:q8_out i:q8_batch_stride,q8_token_stride") + _ROTARY)
_sig("fa_fp8_kvcache_step_workspace_bytes", _KVWS + _fields("c:causal") + _WINDOW + _fields("c:with_sinks,in_dtype,with_q8_out"), _SIZE)
# head dims 64 / 128 / 256: each _mod entry point's list (and the workspace functions' lists) with d under the name head_dim
def _hdim_fields(fields):
    return tuple(("head_dim" if field == "d" else field, ctype) for field, ctype in fields)


for _name in ("fa_fp8_forward", "fa_fp8_forward_varlen", "fa_fp8_forward_kvcache"):
    _sig(_name + "_hdim", _hdim_fields(_SIGNATURES[_name + "_mod"][1]))
_sig("fa_fp8_forward_hdim_workspace_bytes", _hdim_fields(_SIGNATURES["fa_fp8_forward_workspace_bytes"][1]), _SIZE)
_sig("fa_fp8_forward_varlen_hdim_workspace_bytes", _hdim_fields(_SIGNATURES["fa_fp8_forward_varlen_workspace_bytes"][1]), _SIZE)
_sig("fa_fp8_forward_kvcache_hdim_workspace_bytes", _hdim_fields(_SIGNATURES["fa_fp8_forward_kvcache_workspace_bytes_mod"][1]), _SIZE)
# packed queries (and new keys) on the fp8 decode call and the step: the _hdim / step list with head_dim, then the packed group
_sig("fa_fp8_forward_kvcache_varlen", _SIGNATURES["fa_fp8_forward_kvcache_hdim"][1] + _fields("p:cu_seqlens_q i:total_q,max_seqlen_q"))
_sig("fa_fp8_forward_kvcache_varlen_workspace_bytes",
     _fields("i:batch,heads_q,heads_kv,total_q,max_seqlen_q,cache_len,head_dim,num_splits c:causal") + _WINDOW + _fields("c:with_sinks"), _SIZE)
_sig("fa_fp8_kvcache_step_varlen", _hdim_fields(_SIGNATURES["fa_fp8_kvcache_step"][1]) +
     _fields("p:cu_seqlens_q i:total_q,max_seqlen_q p:cu_seqlens_k_new i:total_k_new"))
_sig("fa_fp8_kvcache_step_varlen_workspace_bytes",
     _hdim_fields(_SIGNATURES["fa_fp8_kvcache_step_workspace_bytes"][1]) + _fields("i:total_q,max_seqlen_q"), _SIZE)
_KVWSV = _fields("i:batch,heads_q,heads_kv,total_q,max_seqlen_q,cache_len,d,num_splits c:with_sinks")
_sig("fa_ex_kvcache_workspace_bytes_varlen", _KVWSV, _SIZE)
_sig("fa_ex_kvcache_workspace_bytes_qv", _KVWSV + _fields("i:d_v"), _SIZE)


def _load_library() -> ctypes.CDLL:
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} not found: build it with `make -C flashattention-pytorch_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`)"
        )
    lib = ctypes.CDLL(_LIB_PATH)
    for name in EXPORTED_C_SYMBOLS:
        restype, fields = _SIGNATURES[name]
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [ctype for _field, ctype in fields], restype
    return lib


_lib = _load_library()
LIBRARY_PATH = _LIB_PATH
_CALLS = {}   # name -> (the C function, a getter of its arguments from the widest entry point's, their count): see _call


def _family(widest, narrower):
    """The entry points of a family take the widest one's arguments less the groups they were defined before; each gets a getter
    of its own arguments from a tuple of the widest one's (a field the widest one lacks is a ValueError here, at import)."""
    wide = [field for field, _ctype in _SIGNATURES[widest][1]]
    for name in (widest, *narrower):
        own = operator.itemgetter(*[wide.index(field) for field, _ctype in _SIGNATURES[name][1]])
        _CALLS[name] = (getattr(_lib, name), own, len(wide))


_family("fa_ex_forward_sink", ["fa_ex_forward" + _suffix for _suffix in ("", "_grouped", "_window", "_scoremod")])
_family("fa_ex_forward_varlen_sink", ["fa_ex_forward_varlen", "fa_ex_forward_varlen_scoremod"])
_family("fa_ex_backward_dlse", ["fa_ex_backward" + _suffix for _suffix in ("", "_grouped", "_window", "_scoremod", "_sink")])
_family("fa_ex_backward_varlen_dlse", ["fa_ex_backward_varlen" + _suffix for _suffix in ("", "_scoremod", "_sink")])
# a v of its own width: each entry point takes the widest member above plus d_v and is called with exactly its own arguments, so
# the four families above, and what their members are handed, stay what they were
for _name in ("fa_ex_forward_vdim", "fa_ex_backward_vdim", "fa_ex_forward_varlen_vdim", "fa_ex_backward_varlen_vdim"):
    _family(_name, [])
# an additive bias: likewise a family of one each, called with exactly its own arguments
for _name in ("fa_ex_forward_bias", "fa_ex_backward_bias"):
    _family(_name, [])
_family("fa_ex_forward_varlen_paged_fp8", ["fa_ex_forward_varlen_paged"])
_family("fa_rotary_apply", [])
_family("fa_merge_states", [])
_family("fa_merge_states_backward", [])
_family("fa_mla_sparse_forward", [])
_family("fa_mla_fp8_forward", [])
_family("fa_mla_fp8_pack", [])
_family("fa_indexer_pack", [])
_family("fa_indexer_logits", [])
_family("fa_indexer_topk", [])
_family("fa_fp8_forward", [])
_family("fa_fp8_forward_varlen", [])
_family("fa_fp8_forward_kvcache", [])
# a window, a softcap and sinks: each entry point takes its parent's arguments plus one group and is called with exactly its own
for _name in ("fa_fp8_forward_mod", "fa_fp8_forward_varlen_mod", "fa_fp8_forward_kvcache_mod"):
    _family(_name, [])
# head dims 64 / 128 / 256: again a family of one each
for _name in ("fa_fp8_forward_hdim", "fa_fp8_forward_varlen_hdim", "fa_fp8_forward_kvcache_hdim"):
    _family(_name, [])
_family("fa_fp8_quantize", [])
_family("fa_fp8_kvcache_step", [])
# packed queries / new keys and the step at 64 / 256: a family of one each, called with exactly its own arguments
_family("fa_fp8_forward_kvcache_varlen", [])
_family("fa_fp8_kvcache_step_varlen", [])
_family("fa_ex_forward_kvcache_qv", ["fa_ex_forward_kvcache" + _suffix for _suffix in ("", "_paged", "_rotary", "_fp8", "_sink", "_varlen")])


def version() -> str:
    return _lib.fa_version().decode()


def set_kernel_mode(mode: int) -> int:
    """0 = auto (16-bit MFMA kernels where they apply), 1 = force the exact-f32 kernels. Returns the old mode."""
    return _lib.fa_set_kernel_mode(int(mode))


def set_option(name: str, value: int) -> None:
    """Tuning knob for sweeps / A-B runs (fwd_kb, fwd_stag, fwd_tpw, dq_tpw, dkdv_tpw, ...); see csrc/fa_kernels.h."""
    _check(_lib.fa_set_option(name.encode(), int(value)))


def debug_trace_buffer(t) -> None:
    """Debug: register a CUDA int64 tensor of >= 4096 elements for the staggered forward's phase timestamps (None = off)."""
    _check(_lib.fa_debug_trace_buffer(ctypes.c_void_p(t.data_ptr() if t is not None else 0)))


def profile_enable(on: bool) -> None:
    """Start (and clear) or stop per-kernel HIP-event timing inside the library."""
    _lib.fa_profile_enable(int(bool(on)))


def profile_report() -> dict:
    """{kernel_name: (launches, total_ms)} for the launches since profile_enable(True); waits for the events."""
    buf = ctypes.create_string_buffer(4096)
    n = _lib.fa_profile_report(buf, 4096)
    if n < 0:
        raise RuntimeError(_lib.fa_last_error().decode())
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out


def route_count(name: str) -> int:
    """Launches of the named kernel route since the library was loaded ("dkdv_stream", "dkdv_lean": include/fa_mi355x.h)."""
    n = _lib.fa_route_count(name.encode())
    if n < 0:
        raise RuntimeError(_lib.fa_last_error().decode())
    return n


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(_lib.fa_last_error().decode())


def _call(name, values) -> None:
    """Call the C function `name`.  values: the arguments of the widest entry point of its family, in that one's order; a narrower
    entry point is passed the ones it takes.  RuntimeError with the library's text on an error code."""
    fn, own, count = _CALLS[name]
    if len(values) != count:
        raise TypeError(f"{name}: {len(values)} values for the {count} arguments of its family")
    if fn(*own(values)) != 0:
        raise RuntimeError(_lib.fa_last_error().decode())


def _ptr(t) -> int:
    return t.data_ptr() if t is not None else 0


def _contiguous(t):
    return t.contiguous() if t is not None else None


def _check_inputs(who, *tensors):
    t0 = tensors[0]
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if t0.dim() != 3:
        raise RuntimeError(f"{who}: q must be 3-D (BH, N, d), got {tuple(t0.shape)}")  # fa2_fwd.cu:40
    for t in tensors:
        if t.shape != t0.shape or t.dtype != t0.dtype or t.device != t0.device:
            raise RuntimeError(f"{who}: q, k, v (o, do) must share shape, dtype and device")  # fa2_fwd.cu:41-45
    if t0.dtype not in _DTYPE_CODE:
        raise RuntimeError(f"{who}: unsupported dtype {t0.dtype}")
    return _DTYPE_CODE[t0.dtype]


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# ---- workspace: one grow-only buffer per (device, stream), see workspace.py ----
_workspaces = WorkspaceCache(lambda nbytes, device: torch.empty((nbytes,), dtype=torch.uint8, device=device))


def _workspace(device, nbytes: int):
    """The buffer a call on `device`'s current stream works in.  Inside a graph capture it is a plain allocation of the
    capture's own pool (a cached buffer allocated during capture would outlive the pool it came from)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)
    return _workspaces.get(device, _stream_ptr(device), nbytes)


def _device_headroom(device) -> int:
    """Bytes the device could still give this process: driver-free memory + what torch's allocator holds unused."""
    free, _total = torch.cuda.mem_get_info(device)
    return int(free) + max(0, torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device))


def release_workspace(device=None) -> int:
    """Give the shim's workspace buffers back to torch's allocator (all devices if None).  Returns the bytes released.
    Call it between phases of a program that no longer runs attention backward; the next call allocates again."""
    if device is not None:
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
    return _workspaces.release(device)


def workspace_stats() -> dict:
    return {"bytes": _workspaces.total_bytes(), "allocations": _workspaces.allocations, "hits": _workspaces.hits}


def _forward(cfn, who, q, k, v, causal, softmax_scale, br, bc, extra=None):
    code = _check_inputs(who, q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    bh, n, d = q.shape
    with torch.cuda.device(q.device):
        o = torch.empty_like(q)
        lse = torch.empty((bh, n), dtype=torch.float32, device=q.device)
        args = [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), bh, n, d, code,
                int(bool(causal)), float(softmax_scale), int(br), int(bc)]
        ws = None
        if extra is not None:
            stages, fp8 = extra
            nbytes = _lib.fa3_forward_workspace_bytes(bh, n, d, code, int(bool(fp8)))
            ws = _workspace(q.device, nbytes)
            args += [int(stages), int(bool(fp8)), ws.data_ptr(), int(nbytes)]
        args.append(_stream_ptr(q.device))
        _check(cfn(*args))
    return o, lse


def _backward(cfn, who, q, k, v, o, do_, lse, causal, softmax_scale, br, bc, extra=None):
    code = _check_inputs(who, q, k, v, o, do_)
    q, k, v, o, do_ = (t.contiguous() for t in (q, k, v, o, do_))
    bh, n, d = q.shape
    if lse.shape != (bh, n) or lse.dtype != torch.float32 or not lse.is_cuda:
        raise RuntimeError(f"{who}: lse must be a float32 device tensor of shape (BH, N)")
    lse = lse.contiguous()
    with torch.cuda.device(q.device):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        # minimum = row constants (+ FA3's round-tripped Q, K); fast = + room for the dS tiles where the hand-over serves the
        # call (bounded by the library's chunk size whatever BH is).  The size only selects speed: with the minimum the
        # library runs its recomputing dQ pass.
        small = int(_lib.fa_backward_workspace_bytes(bh, n, d, code))
        fast = int(_lib.fa_backward_workspace_bytes_fast(bh, n, d, code, int(bool(causal))))
        if extra is not None:
            fp8_slabs = int(_lib.fa3_backward_workspace_bytes(bh, n, d, code, int(bool(extra[1])))) - small
            small, fast = small + fp8_slabs, fast + fp8_slabs
        capturing = torch.cuda.is_current_stream_capturing()
        have = 0 if capturing else _workspaces.capacity(q.device, _stream_ptr(q.device))
        # (no device query while a graph is being captured: the buffer then comes from the capture's pool anyway)
        nbytes = plan_backward_workspace(small, fast, have, None if (have >= fast or capturing) else _device_headroom(q.device))
        ws = _workspace(q.device, nbytes)
        nbytes = max(nbytes, 0 if capturing else _workspaces.capacity(q.device, _stream_ptr(q.device)))
        args = [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do_.data_ptr(), lse.data_ptr(),
                dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), bh, n, d, code, int(bool(causal)),
                float(softmax_scale), int(br), int(bc)]
        if extra is not None:
            stages, fp8 = extra
            args += [int(stages), int(bool(fp8))]
        args += [ws.data_ptr(), nbytes, _stream_ptr(q.device)]
        _check(cfn(*args))
    return dq, dk, dv


# ---- the six names of csrc/common/torch.extension.cpp:73-83 ----

def fa1_forward(q, k, v, causal, softmax_scale, br, bc):
    return _forward(_lib.fa1_forward, "fa1_forward", q, k, v, causal, softmax_scale, br, bc)


def fa1_backward(q, k, v, o, do_, lse, causal, softmax_scale, br, bc):
    return _backward(_lib.fa1_backward, "fa1_backward", q, k, v, o, do_, lse, causal, softmax_scale, br, bc)


def forward(q, k, v, causal, softmax_scale, br, bc):
    return _forward(_lib.fa2_forward, "forward", q, k, v, causal, softmax_scale, br, bc)


def backward(q, k, v, o, do_, lse, causal, softmax_scale, br, bc):
    return _backward(_lib.fa2_backward, "backward", q, k, v, o, do_, lse, causal, softmax_scale, br, bc)


def fa3_forward(q, k, v, causal, softmax_scale, br, bc, stages, fp8):
    return _forward(_lib.fa3_forward, "fa3_forward", q, k, v, causal, softmax_scale, br, bc, extra=(stages, fp8))


def fa3_backward(q, k, v, o, do_, lse, causal, softmax_scale, br, bc, stages, fp8):
    return _backward(_lib.fa3_backward, "fa3_backward", q, k, v, o, do_, lse, causal, softmax_scale, br, bc,
                     extra=(stages, fp8))


# ---- extended attention (include/fa_mi355x.h: fa_ex_forward / fa_ex_backward) ----

def _dlse_arg(who, dlse, lse, form):
    """dlse, the gradient of lse, contiguous: float32 with exactly lse's shape on lse's device; None passes through"""
    if dlse is None:
        return None
    if not isinstance(dlse, torch.Tensor) or dlse.dtype != torch.float32 or dlse.shape != lse.shape or dlse.device != lse.device:
        got = f"{tuple(dlse.shape)} {dlse.dtype} on {dlse.device}" if isinstance(dlse, torch.Tensor) else type(dlse).__name__
        raise RuntimeError(f"{who}: dlse must be a {form} float32 tensor on lse's device, lse's shape {tuple(lse.shape)}; got {got}")
    return dlse.contiguous()


def _ex_common(who, q, k, v, mask, block_mask, br, bc):
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    # grouped-query attention: k and v may hold fewer units than q, BH / kv_group, query unit u reading K/V unit u // kv_group
    if (q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or v.shape[:2] != k.shape[:2] or q.shape[2] != k.shape[2] or
            (k.shape[0] == 0 and q.shape[0] != 0) or (k.shape[0] > 0 and q.shape[0] % k.shape[0] != 0)):
        raise RuntimeError(f"{who}: q must be (BH, Nq, d), k (BH / kv_group, Nk, d) and v (BH / kv_group, Nk, d_v); got {tuple(q.shape)}, "
                           f"{tuple(k.shape)}, {tuple(v.shape)}")
    if q.dtype not in _DTYPE_CODE or k.dtype != q.dtype or v.dtype != q.dtype:
        raise RuntimeError(f"{who}: q, k, v must share a supported dtype")
    bh, nq, d = q.shape
    nk = k.shape[1]
    mptr, mstride = 0, 0
    if mask is not None:
        mask = mask.to(device=q.device, dtype=torch.uint8).contiguous()   # 0 = masked
        if tuple(mask.shape) == (nq, nk):
            mstride = 0
        elif tuple(mask.shape) == (bh, nq, nk):
            mstride = nq * nk
        else:
            raise RuntimeError(f"{who}: mask must be (Nq, Nk) or (BH, Nq, Nk), got {tuple(mask.shape)}")
        mptr = mask.data_ptr()
    bptr = 0
    if block_mask is not None:
        block_mask = block_mask.to(device=q.device, dtype=torch.uint8).contiguous()
        br, bc = max(int(br), 1), max(int(bc), 1)   # (an empty side: Br = min(block_size, 0))
        want = ((nq + br - 1) // br, (nk + bc - 1) // bc)
        if tuple(block_mask.shape) != want:
            raise RuntimeError(f"{who}: block_sparse_mask must be {want} for br={br}, bc={bc}, got {tuple(block_mask.shape)}")
        bptr = block_mask.data_ptr()
    kv_group = bh // k.shape[0] if k.shape[0] > 0 else 1
    return bh, nq, nk, d, _DTYPE_CODE[q.dtype], mask, mptr, mstride, block_mask, bptr, kv_group


def window_arg(who, window):
    """`window` as (left, right) ints, -1 = unbounded on that side (FlashAttention-2's window_size); the C layer's error text
    for anything else."""
    try:
        left, right = window
    except (TypeError, ValueError):
        raise RuntimeError(f"{who}: window must be a pair (left, right) of ints, got {window!r}") from None
    try:
        if isinstance(left, bool) or isinstance(right, bool):
            raise TypeError
        left, right = operator.index(left), operator.index(right)
    except TypeError:
        raise RuntimeError(f"{who}: window must be a pair (left, right) of ints, got {window!r}") from None
    if left < -1 or right < -1:
        raise RuntimeError(f"{who}: window ({left}, {right}): each bound must be >= 0, or -1 for unbounded")
    return left, right


def window_effective(nq, nk, causal, window) -> bool:
    """Does `window` bound anything once the C layer has canonicalised it (fa_capi.hip: window_canon)?"""
    left, right = window
    if left >= nk - 1:
        left = -1
    if right >= nq - 1 or (causal and right >= 0):
        right = -1
    if not causal and right == 0:
        right = -1   # (the causal mask)
    return left >= 0 or right >= 0


def softcap_arg(who, softcap) -> float:
    """softcap as a float, finite and >= 0 (0 = off); the C layer's error text for anything else."""
    if isinstance(softcap, bool) or not isinstance(softcap, numbers.Real):
        raise RuntimeError(f"{who}: softcap must be a finite number >= 0 (got {softcap!r})")
    c = float(softcap)
    if not (math.isfinite(c) and c >= 0.0):
        raise RuntimeError(f"{who}: softcap must be a finite number >= 0 (got {c!r})")
    return c


def alibi_arg(who, slopes, device, units, heads=None):
    """(pointer, alibi_heads, alibi_batch_stride, tensor) of ALiBi slopes (FlashAttention-2's alibi_slopes): float32 on `device`,
    (heads,) or (units / heads, heads) with a unit last-dim stride — contiguous, or a (B, H) view of an (H,) vector (row stride 0).
    heads=None (the 3-D calls, (BH, N, d)): one slope per unit, (BH,), or (B, H) with B * H = BH.  (0, 1, 0, None) without slopes."""
    if slopes is None:
        return 0, 1, 0, None
    if not isinstance(slopes, torch.Tensor):
        raise RuntimeError(f"{who}: alibi_slopes must be a float32 tensor")
    if slopes.dtype != torch.float32:
        raise RuntimeError(f"{who}: alibi_slopes must be float32, got {slopes.dtype}")
    if slopes.device != device:
        raise RuntimeError(f"{who}: alibi_slopes must be on q's device ({device}), got {slopes.device}")
    if heads is None:
        forms = f"({units},) or (B, H) with B * H = {units}"
        ok = (slopes.dim() == 1 and slopes.shape[0] == units) or (slopes.dim() == 2 and slopes.shape[0] * slopes.shape[1] == units)
    else:
        forms = f"({heads},) or ({units // max(heads, 1)}, {heads})"
        ok = (slopes.dim() == 1 and slopes.shape[0] == heads) or (slopes.dim() == 2 and tuple(slopes.shape) == (units // heads, heads))
    if not ok:
        raise RuntimeError(f"{who}: alibi_slopes must be {forms}, got {tuple(slopes.shape)}")
    if slopes.dim() == 1:
        if not slopes.is_contiguous():
            raise RuntimeError(f"{who}: alibi_slopes must be contiguous")
        return slopes.data_ptr(), slopes.shape[0], 0, slopes
    if slopes.shape[1] > 1 and slopes.stride(1) != 1 or (slopes.shape[0] > 1 and slopes.stride(0) not in (0, slopes.shape[1])):
        raise RuntimeError(f"{who}: alibi_slopes must be contiguous (or a (B, H) view of an (H,) vector)")
    bstride = slopes.stride(0) if slopes.shape[0] > 1 else 0
    return slopes.data_ptr(), slopes.shape[1], bstride, slopes


def sinks_arg(who, sinks, device, units, heads=None):
    """(pointer, sink_heads, tensor) of attention sinks: a contiguous float32 (sink_heads,) tensor on `device`, one logit per head
    that joins each row's softmax as an extra column with a zero value (-inf = no sink for that head).  heads=None (the 3-D
    calls, (BH, N, d)): sink_heads = len(sinks) must divide the BH units, unit u takes sinks[u % sink_heads]; otherwise
    (the 4-D, varlen and KV-cache calls) sinks must be (heads,), one per query head.  (0, 1, None) without sinks."""
    if sinks is None:
        return 0, 1, None
    if not isinstance(sinks, torch.Tensor):
        raise RuntimeError(f"{who}: sinks must be a float32 tensor")
    if sinks.dtype != torch.float32:
        raise RuntimeError(f"{who}: sinks must be float32, got {sinks.dtype}")
    if sinks.device != device:
        raise RuntimeError(f"{who}: sinks must be on q's device ({device}), got {sinks.device}")
    if heads is None:
        ok = sinks.dim() == 1 and sinks.shape[0] >= 1 and units % sinks.shape[0] == 0
        forms = f"(sink_heads,) with sink_heads dividing {units}"
    else:
        ok = sinks.dim() == 1 and sinks.shape[0] == heads
        forms = f"({heads},)"
    if not ok:
        raise RuntimeError(f"{who}: sinks must be {forms}, got {tuple(sinks.shape)}")
    if not sinks.is_contiguous():
        raise RuntimeError(f"{who}: sinks must be contiguous")
    return sinks.data_ptr(), sinks.shape[0], sinks


def bias_refuse(who, **carried):
    """NotImplementedError naming the first argument in `carried` (name=truthy) that a call with attn_bias does not take"""
    for name, on in carried.items():
        if on:
            hint = ": fold it into attn_bias as -inf" if name == "mask" else ""
            raise NotImplementedError(f"{who}: {name} is not supported with attn_bias{hint}")


def bias_arg(who, bias, q, nq, nk, units, heads=None, need_dbias=False, **carried):
    """(pointer, bias_heads, batch stride, head stride, row stride, tensor) of an additive attention bias: q's dtype on q's device,
    (Bb, Hb, Rb, Nk) with Bb in {1, B}, Hb in {1, H}, Rb in {1, Nq} and B * H = `units`, or (Ub, Rb, Nk) with Ub in {1, units}
    (one bias per unit).  heads=None (the 3-D calls): H is the bias's own Hb (H = 1 with Hb = 1 and Bb = 1, units / Bb with Hb = 1).
    It is passed by strides, never copied: the last dim contiguous, the data 16-byte aligned, every stride of a dimension that is
    not broadcast a multiple of 8, the storage of a row reaching to Nk rounded up to 8 — ValueError otherwise, which says how to
    allocate it.  Then NotImplementedError naming the first argument in `carried` (name=truthy) the bias kernels do not take, and
    a gradient for a row-broadcast bias.  (0, 1, 0, 0, 0, None) without a bias."""
    if bias is None:
        return 0, 1, 0, 0, 0, None
    if not isinstance(bias, torch.Tensor):
        raise RuntimeError(f"{who}: attn_bias must be a tensor of q's dtype")
    if bias.dtype != q.dtype:
        raise RuntimeError(f"{who}: attn_bias must have q's dtype ({q.dtype}), got {bias.dtype}")
    if bias.device != q.device:
        raise RuntimeError(f"{who}: attn_bias must be on q's device ({q.device}), got {bias.device}")
    shape = tuple(bias.shape)
    if bias.dim() == 3:
        forms = f"({units} or 1, {nq} or 1, {nk})"
        ok = shape[0] in (1, units) and shape[1] in (1, nq) and shape[2] == nk
        h = 1
        sizes, strides = (shape[0], 1, shape[1]), (bias.stride(0), 0, bias.stride(1))
    else:
        if heads is None and bias.dim() == 4:
            heads = shape[1] if shape[1] > 1 else (1 if shape[0] == 1 else max(units // max(shape[0], 1), 1))
        h = heads if heads else 1
        forms = f"(B or 1, H or 1, {nq} or 1, {nk}) with B * H = {units}" + (f", H = {h}" if heads else "")
        ok = (bias.dim() == 4 and units % h == 0 and shape[0] in (1, units // h) and shape[1] in (1, h) and shape[2] in (1, nq) and
              shape[3] == nk)
        sizes, strides = shape[:3], bias.stride()[:3]
    if not ok:
        raise RuntimeError(f"{who}: attn_bias must be {forms}, got {shape}")
    bias_refuse(who, **carried)
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{who}: attn_bias needs float16 or bfloat16 tensors, got dtype {q.dtype} (no exact-f32 kernels with a bias)")
    d = q.shape[-1]
    if d > 128 or d % 8 != 0:
        raise NotImplementedError(f"{who}: attn_bias needs d <= 128 and d % 8 == 0, got d={d} (no exact-f32 kernels with a bias)")
    if need_dbias and sizes[2] == 1 and nq > 1:
        raise NotImplementedError(f"{who}: a gradient for a row-broadcast attn_bias (shape {shape}, Nq={nq}) is not supported")
    pad = "allocate the last dim padded to a multiple of 8 and pass the slice, bias_padded[..., :Nk]; the library never copies a bias"
    if nk > 1 and bias.stride(-1) != 1:
        raise ValueError(f"{who}: attn_bias must have a contiguous last dim (stride {bias.stride(-1)}); {pad}")
    bs, hs, rs = (st if n > 1 else 0 for n, st in zip(sizes, strides))
    if bs % 8 or hs % 8 or rs % 8 or bs < 0 or hs < 0 or rs < 0:
        raise ValueError(f"{who}: attn_bias of shape {shape} has strides {tuple(bias.stride())}: every stride of a dimension that is not "
                         f"broadcast must be a multiple of 8 elements; {pad}")
    nkp = (nk + 7) // 8 * 8
    last = bias.storage_offset() + (sizes[0] - 1) * bs + (sizes[1] - 1) * hs + (sizes[2] - 1) * rs
    if nk > 0 and (last + nkp) * bias.element_size() > bias.untyped_storage().nbytes():
        raise ValueError(f"{who}: the storage of attn_bias (shape {shape}) ends before Nk = {nk} rounded up to {nkp} in its last row; {pad}")
    if bias.data_ptr() % 16 != 0:
        raise ValueError(f"{who}: attn_bias must be 16-byte aligned; {pad}")
    return bias.data_ptr(), h, bs, hs, rs, bias


def _dbias_alloc(bias, nk):
    """dbias for `bias`: the bias's own shape, a slice of a buffer whose last dim is padded to 8, and its three strides (0 = a
    dimension of one: broadcast).  The call writes every element of the slice and nothing of the padding."""
    lead = tuple(bias.shape[:-1])
    dbias = torch.empty(lead + ((nk + 7) // 8 * 8,), dtype=bias.dtype, device=bias.device)[..., :nk]
    st = dbias.stride()
    if bias.dim() == 3:
        return dbias, (st[0] if lead[0] > 1 else 0, 0, st[1] if lead[1] > 1 else 0)
    return dbias, tuple(s if n > 1 else 0 for n, s in zip(lead, st[:3]))


def vdim_arg(who, d, d_v, dtype, **carried):
    """The width of v as the library takes it: 0 where v is as wide as q and k (the call without the argument), else d_v after the
    rules of fa_ex_*_vdim in the library's order — NotImplementedError naming the first one broken: the widths, the dtype, then
    each argument in `carried` (name=truthy) that the two-width kernels do not take."""
    if d_v == d:
        return 0
    if d_v > d:
        raise NotImplementedError(f"{who}: v wider than q and k (d_v={d_v} > d={d}) is not supported")
    if d % 8 != 0 or d_v % 8 != 0 or d_v < 8:
        raise NotImplementedError(f"{who}: d_v != d needs d and d_v to be positive multiples of 8 (got d={d}, d_v={d_v})")
    if d > 192:
        raise NotImplementedError(f"{who}: d_v != d needs d <= 192 (got d={d})")
    if d_v > 128:
        raise NotImplementedError(f"{who}: d_v != d needs d_v <= 128 (got d_v={d_v})")
    if dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{who}: d_v != d needs float16 or bfloat16 tensors, got dtype {dtype} (no exact-f32 kernels with two widths)")
    for name, on in carried.items():
        if on:
            raise NotImplementedError(f"{who}: {name} is not supported with d_v != d (v of shape (..., {d_v}), q and k (..., {d}))")
    return d_v


def _ex_variant(sinks, mod, window, grouped=False, dlse=False, vdim=False) -> str:
    """the narrowest entry point of a family that takes what the call carries: each one adds a group of arguments to the one before"""
    return "_vdim" if vdim else "_dlse" if dlse else "_sink" if sinks else "_scoremod" if mod else "_window" if window else "_grouped" if grouped else ""


def ex_forward(q, k, v, causal, softmax_scale, mask=None, block_mask=None, br=128, bc=128, dropout_p=0.0, seed=0, window=(-1, -1),
               softcap=0.0, alibi_slopes=None, *, attn_bias=None, sinks=None):
    """(o, lse) of attention with Nq != Nk (causal aligned bottom-right), dense mask (0 = masked), block-sparse mask
    (0 = tile skipped) and dropout; see include/fa_mi355x.h.  k and v with BH / g units (g query heads per K/V head) make
    it grouped-query attention.  window = (left, right): key j is visible to row i only within
    [i + Nk - Nq - left, i + Nk - Nq + right], -1 = unbounded (fa_ex_forward_window).  softcap > 0 caps the scores at
    softcap * tanh(s / softcap); alibi_slopes (float32 (BH,), or (B, H) with B * H = BH) subtract slope * |i + Nk - Nq - j|
    (fa_ex_forward_scoremod).  sinks (float32 (sink_heads,), sink_heads dividing BH: unit u takes sinks[u % sink_heads]) adds one
    column exp(sink) with a zero value to each row's softmax; lse contains it (fa_ex_forward_sink).
    v may be narrower than q and k, (BH / g, Nk, d_v) with 8 <= d_v < d <= 192, d_v <= 128, both multiples of 8, float16 / bfloat16
    (fa_ex_forward_vdim; MLA prefill: 192 + 128): o is then (BH, Nq, d_v).  It goes with causal, GQA and softmax_scale only: mask,
    block_sparse_mask, dropout_p, window_size, softcap, alibi_slopes and sinks raise NotImplementedError with the name (vdim_arg).
    attn_bias (keyword-only; q's dtype, (Bb, Hb, Rb, Nk) or (BH or 1, Rb, Nk), broadcast by size 1, passed by strides: bias_arg) is
    added to the scaled scores, -inf = masked (fa_ex_forward_bias).  It goes with causal, GQA and softmax_scale only as well."""
    wl, wr = window_arg("ex_forward", window)
    cap = softcap_arg("ex_forward", softcap)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    bh, nq, nk, d, code, mask, mptr, mstride, block_mask, bptr, g = _ex_common("ex_forward", q, k, v, mask, block_mask, br, bc)
    aptr, aheads, astride, alibi_slopes = alibi_arg("ex_forward", alibi_slopes, q.device, bh)
    sptr, sheads, sinks = sinks_arg("ex_forward", sinks, q.device, bh)
    bias = bias_arg("ex_forward", attn_bias, q, nq, nk, bh, mask=mask is not None, block_sparse_mask=block_mask is not None,
                    dropout_p=dropout_p > 0.0, window_size=(wl, wr) != (-1, -1), softcap=cap > 0.0, alibi_slopes=aptr, sinks=sptr,
                    **{"d_v != d": v.shape[2] != d})
    d_v = vdim_arg("ex_forward", d, v.shape[2], q.dtype, mask=mask is not None, block_sparse_mask=block_mask is not None,
                   dropout_p=dropout_p > 0.0, window_size=(wl, wr) != (-1, -1), softcap=cap > 0.0, alibi_slopes=aptr, sinks=sptr)
    with torch.cuda.device(q.device):
        o = torch.empty((bh, nq, v.shape[2]), dtype=q.dtype, device=q.device)
        lse = torch.empty((bh, nq), dtype=torch.float32, device=q.device)
        if bias[0]:
            _call("fa_ex_forward_bias", (
                q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), bh, g, nq, nk, d, code, int(bool(causal)), wl, wr,
                float(softmax_scale), cap, aptr, aheads, astride, sptr, sheads, 0, *bias[:5], mptr, mstride, bptr, int(br), int(bc),
                float(dropout_p), int(seed) & (2 ** 64 - 1), _stream_ptr(q.device)))
            return o, lse
        _call("fa_ex_forward" + _ex_variant(sptr, cap > 0.0 or aptr, (wl, wr) != (-1, -1), g > 1, vdim=d_v), (
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), bh, g, nq, nk, d, code, int(bool(causal)), wl, wr,
            float(softmax_scale), cap, aptr, aheads, astride, sptr, sheads, *((d_v,) if d_v else ()), mptr, mstride, bptr, int(br), int(bc), float(dropout_p),
            int(seed) & (2 ** 64 - 1), _stream_ptr(q.device)))
    return o, lse


def ex_backward(q, k, v, o, do_, lse, causal, softmax_scale, mask=None, block_mask=None, br=128, bc=128, dropout_p=0.0, seed=0,
                window=(-1, -1), softcap=0.0, alibi_slopes=None, *, dlse=None, attn_bias=None, need_dbias=False, sinks=None):
    """(dq, dk, dv) of ex_forward; with sinks (and the lse ex_forward returned with them) also dsinks, float32 (sink_heads,), as a
    fourth result (fa_ex_backward_sink).  dlse: the gradient of lse, float32 (BH, Nq) on q's device, or None
    (fa_ex_backward_dlse); rows whose lse is -inf ignore it.  dlse is keyword-only, and sinks with it: sinks stays the last parameter.
    With a v of its own width (ex_forward) o and do_ are (BH, Nq, d_v) and dv comes back in v's shape (fa_ex_backward_vdim).
    attn_bias: the bias of the forward (fa_ex_backward_bias); with need_dbias its gradient dS = P (dP - delta + dlse) comes back as an
    extra last result, in the bias's own shape and dtype (the fp32 sum in unit order, rounded once, over a batch or head dimension
    of size 1); a row-broadcast bias has no gradient here (NotImplementedError)."""
    wl, wr = window_arg("ex_backward", window)
    cap = softcap_arg("ex_backward", softcap)
    q, k, v, o, do_, lse = (t.contiguous() for t in (q, k, v, o, do_, lse))
    bh, nq, nk, d, code, mask, mptr, mstride, block_mask, bptr, g = _ex_common("ex_backward", q, k, v, mask, block_mask, br, bc)
    aptr, aheads, astride, alibi_slopes = alibi_arg("ex_backward", alibi_slopes, q.device, bh)
    sptr, sheads, sinks = sinks_arg("ex_backward", sinks, q.device, bh)
    mod = cap > 0.0 or aptr != 0 or sptr != 0
    bias = bias_arg("ex_backward", attn_bias, q, nq, nk, bh, need_dbias=bool(need_dbias), mask=mask is not None,
                    block_sparse_mask=block_mask is not None, dropout_p=dropout_p > 0.0, window_size=(wl, wr) != (-1, -1),
                    softcap=cap > 0.0, alibi_slopes=aptr, sinks=sptr, **{"d_v != d": v.shape[2] != d})
    if need_dbias and not bias[0]:
        raise RuntimeError("ex_backward: need_dbias without attn_bias")
    d_v = vdim_arg("ex_backward", d, v.shape[2], q.dtype, mask=mask is not None, block_sparse_mask=block_mask is not None,
                   dropout_p=dropout_p > 0.0, window_size=(wl, wr) != (-1, -1), softcap=cap > 0.0, alibi_slopes=aptr, sinks=sptr)
    if o.shape != (bh, nq, v.shape[2]) or do_.shape != o.shape or lse.shape != (bh, nq) or lse.dtype != torch.float32:
        raise RuntimeError("ex_backward: o, do must be (BH, Nq, d_v) (v's width) and lse (BH, Nq) float32")
    dlse = _dlse_arg("ex_backward", dlse, lse, "(BH, Nq)")
    with torch.cuda.device(q.device):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        if bias[0]:
            dbias, dstr = _dbias_alloc(bias[5], nk) if need_dbias else (None, (0, 0, 0))
            reduced = int(need_dbias and ((dstr[0] == 0 and bh // bias[1] > 1) or (dstr[1] == 0 and bias[1] > 1)))
            nbytes = int(_lib.fa_ex_backward_workspace_bytes_bias(bh, g, nq, nk, d, code, reduced))
            ws = _workspace(q.device, nbytes)
            _call("fa_ex_backward_bias", (
                q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do_.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                dv.data_ptr(), bh, g, nq, nk, d, code, int(bool(causal)), wl, wr, float(softmax_scale), cap, aptr, aheads, astride, sptr,
                sheads, 0, _ptr(dlse), 0, *bias[:5], _ptr(dbias), *dstr, mptr, mstride, bptr, int(br), int(bc), float(dropout_p),
                int(seed) & (2 ** 64 - 1), ws.data_ptr(), nbytes, _stream_ptr(q.device)))
            return (dq, dk, dv, dbias) if need_dbias else (dq, dk, dv)
        extras = int(mask is not None or block_mask is not None or dropout_p > 0.0 or mod or dlse is not None or d_v != 0 or
                     window_effective(nq, nk, bool(causal), (wl, wr)))   # (the dS hand-over serves neither a window nor a modifier,
        #                                                                    nor a gradient of lse)
        if g > 1 or (wl, wr) != (-1, -1) or mod or d_v:   # (+ the per-query-head dK / dV partials the library sums over each group)
            small = int(_lib.fa_ex_backward_workspace_bytes_grouped(bh, g, nq, nk, d, code))
            fast = int(_lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, g, nq, nk, d, code, int(bool(causal)), extras))
        else:
            small = int(_lib.fa_ex_backward_workspace_bytes(bh, nq, nk, d, code))
            fast = int(_lib.fa_ex_backward_workspace_bytes_fast(bh, nq, nk, d, code, int(bool(causal)), extras))
        capturing = torch.cuda.is_current_stream_capturing()
        have = 0 if capturing else _workspaces.capacity(q.device, _stream_ptr(q.device))
        nbytes = plan_backward_workspace(small, fast, have, None if (have >= fast or capturing) else _device_headroom(q.device))
        ws = _workspace(q.device, nbytes)
        nbytes = max(nbytes, 0 if capturing else _workspaces.capacity(q.device, _stream_ptr(q.device)))
        dsinks = torch.empty((sheads,), dtype=torch.float32, device=q.device) if sptr else None
        _call("fa_ex_backward" + _ex_variant(sptr, mod, (wl, wr) != (-1, -1), g > 1, dlse is not None, vdim=d_v), (
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do_.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
            dv.data_ptr(), bh, g, nq, nk, d, code, int(bool(causal)), wl, wr, float(softmax_scale), cap, aptr, aheads, astride, sptr,
            sheads, _ptr(dsinks), _ptr(dlse), *((d_v,) if d_v else ()), mptr, mstride, bptr, int(br), int(bc), float(dropout_p), int(seed) & (2 ** 64 - 1), ws.data_ptr(),
            nbytes, _stream_ptr(q.device)))
    return (dq, dk, dv, dsinks) if sptr else (dq, dk, dv)


# ---- variable-length (packed) sequences (include/fa_mi355x.h: fa_ex_forward_varlen / fa_ex_backward_varlen) ----

def _token_stride(who, name, t, heads, d):
    """Token stride (elements) of a (total, heads, d) tensor whose heads are adjacent at stride d, last dim contiguous."""
    if t.stride(2) != 1:
        raise RuntimeError(f"{who}: {name} must have a contiguous last dim")
    if t.shape[0] > 0 and heads > 1 and t.stride(1) != d:
        raise RuntimeError(f"{who}: the heads of {name} must be adjacent (head stride d = {d}, got {t.stride(1)})")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), heads * d)


def _varlen_common(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    for t in (q, k, v, cu_seqlens_q, cu_seqlens_k):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or v.shape[:2] != k.shape[:2] or q.shape[2] != k.shape[2]:
        raise RuntimeError(f"{who}: q must be (total_q, H_q, d), k (total_k, H_kv, d) and v (total_k, H_kv, d_v); got {tuple(q.shape)}, "
                           f"{tuple(k.shape)}, {tuple(v.shape)}")
    if q.dtype not in _DTYPE_CODE or k.dtype != q.dtype or v.dtype != q.dtype:
        raise RuntimeError(f"{who}: q, k, v must share a supported dtype")
    if len({q.device, k.device, v.device, cu_seqlens_q.device, cu_seqlens_k.device}) != 1:
        raise RuntimeError(f"{who}: all tensors must be on one device")
    for name, c in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if c.dtype != torch.int32 or c.dim() != 1 or c.shape[0] < 2:
            raise RuntimeError(f"{who}: {name} must be a 1-D int32 tensor of batch + 1 >= 2 offsets")
    if cu_seqlens_q.shape != cu_seqlens_k.shape:
        raise RuntimeError(f"{who}: cu_seqlens_q and cu_seqlens_k must have the same length (batch + 1)")
    total_q, hq, d = q.shape
    total_k, hkv = k.shape[0], k.shape[1]
    if hkv == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: the query heads ({hq}) must be a multiple of the K/V heads ({hkv})")
    mq, mk = operator.index(max_seqlen_q), operator.index(max_seqlen_k)
    if mq < 0 or mk < 0:
        raise RuntimeError(f"{who}: max_seqlen_q, max_seqlen_k must be >= 0")
    sq = _token_stride(who, "q", q, hq, d)
    sk = _token_stride(who, "k", k, hkv, d)
    sv = _token_stride(who, "v", v, hkv, v.shape[2])   # (v's own width: its heads adjacent at stride d_v)
    cu_q, cu_k = cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous()
    return (cu_q, cu_k, cu_q.shape[0] - 1, hq, hkv, total_q, total_k, mq, mk, d, _DTYPE_CODE[q.dtype], sq, sk, sv)


def _varlen_pool_e4m3(who, q, k, v, k_descale, v_descale):
    """Are k and v torch.float8_e4m3fn pools?  The float8 rules of flash_attn_with_kvcache, for ex_varlen_forward."""
    for name, t in (("k", k), ("v", v)):
        if isinstance(t, torch.Tensor) and t.dtype in _FLOAT8_DTYPES and t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (an 8-bit cache is torch.float8_e4m3fn)")
    e4m3 = k.dtype == torch.float8_e4m3fn and v.dtype == torch.float8_e4m3fn
    if (k.dtype == torch.float8_e4m3fn or v.dtype == torch.float8_e4m3fn) and \
            (not e4m3 or q.dtype not in (torch.float16, torch.bfloat16)):
        raise RuntimeError(f"{who}: q must have a 16-bit dtype (float16 or bfloat16) and k, v both q's dtype or both "
                           f"torch.float8_e4m3fn, got {q.dtype}, {k.dtype}, {v.dtype}")
    if not e4m3 and (k_descale is not None or v_descale is not None):
        raise RuntimeError(f"{who}: k_descale / v_descale need torch.float8_e4m3fn pools (k, v are {k.dtype})")
    return e4m3


def _varlen_paged_forward(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, dropout_p, wl, wr,
                          cap, alibi_slopes, sinks, block_table, k_descale=None, v_descale=None):
    """ex_varlen_forward with a block_table (fa_ex_forward_varlen_paged, fa_ex_forward_varlen_paged_fp8 for e4m3 pools), its
    arguments checked"""
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32:
        dt = block_table.dtype if isinstance(block_table, torch.Tensor) else type(block_table).__name__
        raise NotImplementedError(f"{who}: block_table of dtype {dt} is not supported (int32 tensor expected)")
    if float(dropout_p) > 0.0:
        raise ValueError(f"{who}: dropout_p > 0 is not supported with block_table (an inference path)")
    for t in (q, k, v, cu_seqlens_q, cu_seqlens_k, block_table):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if len({q.device, k.device, v.device, cu_seqlens_q.device, cu_seqlens_k.device, block_table.device}) != 1:
        raise RuntimeError(f"{who}: all tensors must be on one device")
    if q.dim() != 3 or k.dim() != 4 or v.shape != k.shape or q.shape[2] != k.shape[3]:
        raise RuntimeError(f"{who}: with block_table q must be (total_q, H_q, d), k and v pools (num_blocks, page_block_size, H_kv, d); "
                           f"got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    e4m3 = _varlen_pool_e4m3(who, q, k, v, k_descale, v_descale)
    if not e4m3 and (q.dtype not in _DTYPE_CODE or k.dtype != q.dtype or v.dtype != q.dtype):
        raise RuntimeError(f"{who}: q, k, v must share a supported dtype")
    for name, c in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if c.dtype != torch.int32 or c.dim() != 1 or c.shape[0] < 2:
            raise RuntimeError(f"{who}: {name} must be a 1-D int32 tensor of batch + 1 >= 2 offsets")
    if cu_seqlens_q.shape != cu_seqlens_k.shape:
        raise RuntimeError(f"{who}: cu_seqlens_q and cu_seqlens_k must have the same length (batch + 1)")
    b = cu_seqlens_q.shape[0] - 1
    total_q, hq, d = q.shape
    nblk, ps, hkv = k.shape[0], k.shape[1], k.shape[2]
    if hkv == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: the query heads ({hq}) must be a multiple of the K/V heads ({hkv})")
    if ps < 16 or ps % 16 != 0:
        raise RuntimeError(f"{who}: page_block_size must be a positive multiple of 16, got {ps}")
    if block_table.dim() != 2 or block_table.shape[0] != b:
        raise RuntimeError(f"{who}: block_table must be an int32 (batch, max_blocks_per_seq) tensor, batch = {b}; got "
                           f"{tuple(block_table.shape)}")
    mq, mk = operator.index(max_seqlen_q), operator.index(max_seqlen_k)
    if mq < 0 or mk < 0:
        raise RuntimeError(f"{who}: max_seqlen_q, max_seqlen_k must be >= 0")
    sq = _token_stride(who, "q", q, hq, d)
    kps, kts = _kv_strides(who, "k", k, hkv, d, True)   # (ValueError on a pool view that would need a copy)
    vps, vts = _kv_strides(who, "v", v, hkv, d, True)
    cu_q, cu_k, block_table = cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous(), block_table.contiguous()
    aptr, _h, astride, alibi_slopes = alibi_arg(who, alibi_slopes, q.device, b * hq, heads=hq)
    sptr, sheads, sinks = sinks_arg(who, sinks, q.device, b * hq, heads=hq)
    kdp, vdp, dsc_bs, _scales = _kv_descales(who, k_descale, v_descale, q, b, hkv)
    with torch.cuda.device(q.device):
        o = torch.empty((total_q, hq, d), dtype=q.dtype, device=q.device)
        lse = torch.empty((hq, total_q), dtype=torch.float32, device=q.device)
        _call("fa_ex_forward_varlen_paged_fp8" if e4m3 else "fa_ex_forward_varlen_paged", (
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), b, hq, hkv,
            total_q, 0, mq, mk, d, _DTYPE_CODE[q.dtype], sq, kts, vts, int(bool(causal)), wl, wr, float(softmax_scale), cap, aptr,
            astride, sptr, sheads, block_table.data_ptr(), block_table.shape[1], nblk, ps, kps, vps, _E4M3_CODE, kdp, vdp, dsc_bs,
            _stream_ptr(q.device)))
    return o, lse


def ex_varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, dropout_p=0.0, seed=0,
                      window=(-1, -1), softcap=0.0, alibi_slopes=None, *, block_table=None, k_descale=None, v_descale=None, sinks=None):
    """(o, lse) of attention over packed sequences (FlashAttention-2's varlen layout): q (total_q, H_q, d), k and v
    (total_k, H_kv, d) — strided views along the token dim allowed — cu_seqlens_* int32 (batch + 1,) device offsets.  o is
    (total_q, H_q, d), lse (H_q, total_q) float32.  Never synchronises: cu_seqlens are clamped in the kernels.  softcap and
    alibi_slopes (float32 (H_q,) or (batch, H_q)) as in ex_forward, per sequence (fa_ex_forward_varlen_scoremod).  sinks: float32
    (H_q,), one extra softmax column per query head (fa_ex_forward_varlen_sink).
    block_table (keyword-only, as sinks now is: sinks stays the last parameter) int32 (batch, max_blocks_per_seq): k and v are pools (num_blocks, page_block_size, H_kv, d), page_block_size a
    multiple of 16, and key t of sequence b lives at pool[block_table[b, t // ps], t % ps]; len_k[b] = cu_seqlens_k[b + 1] -
    cu_seqlens_k[b], clamped to min(max_seqlen_k, max_blocks_per_seq * ps).  The pools may be strided views (their own page and
    token strides; a view that would need a copy raises ValueError) and are only read; no dropout.  Each sequence gets the bits
    of the call on the same tokens gathered into packed k, v.  See fa_ex_forward_varlen_paged.
    With block_table the pools may both be torch.float8_e4m3fn (OCP e4m3; q and o stay 16-bit), the cache of flash_attn_with_kvcache:
    a stored byte c of K head h of sequence b stands for e4m3(c) * k_descale[b, h] (V: v_descale), float32 (batch, H_kv) or (H_kv,)
    on q's device, None = 1.0.  The score is softmax_scale * k_descale * (q . k_stored), v_descale multiplies the normalised output
    once.  Other float8 dtypes raise NotImplementedError, scales without e4m3 pools and e4m3 pools without block_table RuntimeError.
    See fa_ex_forward_varlen_paged_fp8.
    Without block_table v may be narrower than q and k, (total_k, H_kv, d_v) as in ex_forward (fa_ex_forward_varlen_vdim): o is
    (total_q, H_q, d_v); dropout_p, window_size, softcap, alibi_slopes, sinks, block_table and k_descale / v_descale then raise
    NotImplementedError with the name.  The heads of v must be adjacent at stride d_v (as k's at d): a slice of a wider projection
    whose head stride is not d_v raises RuntimeError like any k the library cannot take without a copy."""
    who = "ex_varlen_forward"
    wl, wr = window_arg(who, window)
    cap = softcap_arg(who, softcap)
    if isinstance(k, torch.Tensor) and isinstance(v, torch.Tensor) and isinstance(q, torch.Tensor) and k.dim() == v.dim() and \
            k.dim() in (3, 4) and v.shape[:-1] == k.shape[:-1] and v.shape[-1] != k.shape[-1]:
        # a v of its own width goes with neither a paged cache nor an e4m3 one: refused by name, before the checks of those paths
        vdim_arg(who, k.shape[-1], v.shape[-1], q.dtype, block_table=block_table is not None, k_descale=k_descale is not None,
                 v_descale=v_descale is not None)
    if block_table is not None:
        return _varlen_paged_forward(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale,
                                     dropout_p, wl, wr, cap, alibi_slopes, sinks, block_table, k_descale, v_descale)
    if isinstance(k, torch.Tensor) and isinstance(v, torch.Tensor) and isinstance(q, torch.Tensor) and \
            _varlen_pool_e4m3(who, q, k, v, k_descale, v_descale):
        raise RuntimeError(f"{who}: torch.float8_e4m3fn k, v are pools of a paged cache and need block_table")
    cu_q, cu_k, *dims = _varlen_common(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    b, hq, _hkv, total_q, *_ = dims
    d = q.shape[2]
    aptr, _h, astride, alibi_slopes = alibi_arg(who, alibi_slopes, q.device, b * hq, heads=hq)
    sptr, sheads, sinks = sinks_arg(who, sinks, q.device, b * hq, heads=hq)
    d_v = vdim_arg(who, d, v.shape[2], q.dtype, dropout_p=dropout_p > 0.0, window_size=(wl, wr) != (-1, -1), softcap=cap > 0.0,
                   alibi_slopes=aptr, sinks=sptr, k_descale=k_descale is not None, v_descale=v_descale is not None)
    with torch.cuda.device(q.device):
        o = torch.empty((total_q, hq, v.shape[2]), dtype=q.dtype, device=q.device)
        lse = torch.empty((hq, total_q), dtype=torch.float32, device=q.device)
        _call("fa_ex_forward_varlen" + _ex_variant(sptr, cap > 0.0 or aptr, False, vdim=d_v), (
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), *dims,
            int(bool(causal)), wl, wr, float(softmax_scale), cap, aptr, astride, sptr, sheads, *((d_v,) if d_v else ()), float(dropout_p),
            int(seed) & (2 ** 64 - 1), _stream_ptr(q.device)))
    return o, lse


def ex_varlen_backward(q, k, v, o, do_, lse, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale,
                       dropout_p=0.0, seed=0, window=(-1, -1), softcap=0.0, alibi_slopes=None, *, dlse=None, sinks=None):
    """(dq, dk, dv) of ex_varlen_forward: dq in q's (total_q, H_q, d) shape, dk and dv in k's and v's (dense); with sinks also
    dsinks, float32 (H_q,), as a fourth result.  dlse: the gradient of lse, float32 (H_q, total_q), or None
    (fa_ex_backward_varlen_dlse).  With a v of its own width o and do_ are (total_q, H_q, d_v) and dv is (total_k, H_kv, d_v)
    (fa_ex_backward_varlen_vdim)."""
    who = "ex_varlen_backward"
    wl, wr = window_arg(who, window)
    cap = softcap_arg(who, softcap)
    cu_q, cu_k, *dims = _varlen_common(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    b, hq, hkv, total_q, total_k, _mq, _mk, d, code = dims[:9]
    aptr, _h, astride, alibi_slopes = alibi_arg(who, alibi_slopes, q.device, b * hq, heads=hq)
    sptr, sheads, sinks = sinks_arg(who, sinks, q.device, b * hq, heads=hq)
    d_v = vdim_arg(who, d, v.shape[2], q.dtype, dropout_p=dropout_p > 0.0, window_size=(wl, wr) != (-1, -1), softcap=cap > 0.0,
                   alibi_slopes=aptr, sinks=sptr)
    for name, t in (("o", o), ("do", do_)):
        if not t.is_cuda or t.shape != (total_q, hq, v.shape[2]) or t.dtype != q.dtype:
            raise RuntimeError(f"{who}: {name} must be a (total_q, H_q, d_v) device tensor of q's dtype (d_v: v's width)")
    if not lse.is_cuda or lse.shape != (hq, total_q) or lse.dtype != torch.float32:
        raise RuntimeError(f"{who}: lse must be a (H_q, total_q) float32 device tensor")
    dlse = _dlse_arg(who, dlse, lse, "(H_q, total_q)")
    o, do_, lse = o.contiguous(), do_.contiguous(), lse.contiguous()
    with torch.cuda.device(q.device):
        dq = torch.empty((total_q, hq, d), dtype=q.dtype, device=q.device)
        dk = torch.empty((total_k, hkv, d), dtype=q.dtype, device=q.device)
        dv = torch.empty((total_k, hkv, v.shape[2]), dtype=q.dtype, device=q.device)
        nbytes = int(_lib.fa_ex_backward_workspace_bytes_varlen(hq, hkv, total_q, total_k, d, code))
        ws = _workspace(q.device, nbytes)
        nbytes = max(nbytes, 0 if torch.cuda.is_current_stream_capturing() else _workspaces.capacity(q.device, _stream_ptr(q.device)))
        dsinks = torch.empty((sheads,), dtype=torch.float32, device=q.device) if sptr else None
        _call("fa_ex_backward_varlen" + _ex_variant(sptr, cap > 0.0 or aptr, False, False, dlse is not None, vdim=d_v), (
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do_.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
            dv.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), *dims, int(bool(causal)), wl, wr, float(softmax_scale), cap, aptr, astride,
            sptr, sheads, _ptr(dsinks), _ptr(dlse), *((d_v,) if d_v else ()), float(dropout_p), int(seed) & (2 ** 64 - 1), ws.data_ptr(), nbytes,
            _stream_ptr(q.device)))
    return (dq, dk, dv, dsinks) if sptr else (dq, dk, dv)


# ---- KV-cache decoding with split-KV (include/fa_mi355x.h: fa_ex_forward_kvcache) ----

_E4M3_CODE = 3   # FA_DTYPE_E4M3
_FLOAT8_DTYPES = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz")
                       if hasattr(torch, n))


def _kv_descale(who, name, t, q, b, hkv):
    """(pointer, batch stride, the tensor to keep alive) of a float32 (B, H_kv) or (H_kv,) scale on q's device; None: (0, 0, None)"""
    if t is None:
        return 0, 0, None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
        raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (float32 tensor expected)")
    if t.device != q.device:
        raise RuntimeError(f"{who}: {name} must be on q's device ({q.device}), got {t.device}")
    if t.shape == (hkv,):
        if t.stride(0) != 1 and hkv > 1:
            raise RuntimeError(f"{who}: {name} of shape (H_kv,) must be contiguous")
        return t.data_ptr(), 0, t
    if t.shape != (b, hkv):
        raise RuntimeError(f"{who}: {name} must be float32 of shape (B, H_kv) = ({b}, {hkv}) or (H_kv,), got {tuple(t.shape)}")
    if hkv > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{who}: {name} must have a contiguous last dim")
    bs = t.stride(0) if b > 1 else max(t.stride(0), hkv)
    if bs < hkv:   # an expanded row: the (H_kv,) form
        if bs != 0:
            raise RuntimeError(f"{who}: {name} has overlapping rows (stride {bs} < H_kv = {hkv})")
    return t.data_ptr(), bs, t


def _kv_descales(who, k_descale, v_descale, q, b, hkv):
    """(k_descale pointer, v_descale pointer, descale_batch_stride, the tensors to keep alive) of an e4m3 cache's two scales.
    The C entry points have ONE batch stride for both.  Scales of the same form, the usual case, are passed as they are; in mixed
    forms, one (H_kv,) and one (B, H_kv), the (H_kv,) one is copied into (B, H_kv) rows here: one small copy kernel in front of the
    attention kernel, on the call's stream, captured and replayed with it (a replay reads the caller's tensor again, so changed
    scale values are seen)."""
    if k_descale is None and v_descale is None:
        return 0, 0, 0, None
    kdp, kds, k_descale = _kv_descale(who, "k_descale", k_descale, q, b, hkv)
    vdp, vds, v_descale = _kv_descale(who, "v_descale", v_descale, q, b, hkv)
    if kdp and vdp and kds != vds:
        if kds == 0:
            k_descale = k_descale.expand(b, hkv).contiguous()
            kdp, kds = k_descale.data_ptr(), hkv
        elif vds == 0:
            v_descale = v_descale.expand(b, hkv).contiguous()
            vdp, vds = v_descale.data_ptr(), hkv
        else:
            k_descale, v_descale = k_descale.contiguous(), v_descale.contiguous()
            kdp, kds, vdp, vds = k_descale.data_ptr(), hkv, v_descale.data_ptr(), hkv
    return kdp, vdp, kds if kdp else vds, (k_descale, v_descale)


def _kv_strides(who, name, t, heads, d, cache):
    """(batch stride, token stride) of a (B, N, heads, d) tensor whose heads are adjacent at stride d, last dim contiguous."""
    if t.stride(3) != 1 or (heads > 1 and t.stride(2) != d):
        if cache:   # a copy would silently lose the in-place append
            raise ValueError(f"{who}: {name} must have a contiguous last dim and its heads at stride d = {d} "
                             f"(got strides {tuple(t.stride())}); the cache is never copied")
        raise RuntimeError(f"{who}: {name} has an unsupported layout")
    b, n = t.shape[0], t.shape[1]
    ts = t.stride(1) if n > 1 else max(t.stride(1), heads * d)
    bs = t.stride(0) if b > 1 else max(t.stride(0), (n - 1) * ts + heads * d)
    return bs, ts


def _rotary_tables(rotary_cos, rotary_sin, rdim, rotary_interleaved):
    """(the tables to keep alive, the seven rotary arguments of the KV-cache entry points); rows at an even stride, 4-byte aligned:
    otherwise a dense copy.  Without tables: all 0."""
    if rotary_cos is None:
        return None, (0,) * len(_ROTARY)
    tabs = []
    for t in (rotary_cos, rotary_sin):
        if t.stride(1) != 1 or (t.shape[0] > 1 and (t.stride(0) < t.shape[1] or t.stride(0) % 2)) or t.data_ptr() % 4:
            t = t.clone(memory_format=torch.contiguous_format)
        tabs.append(t)
    c, s_ = tabs
    return tabs, (c.data_ptr(), s_.data_ptr(), c.stride(0) if c.shape[0] > 1 else c.shape[1],
                  s_.stride(0) if s_.shape[0] > 1 else s_.shape[1], c.shape[0], rdim, int(bool(rotary_interleaved)))


# what the entry points after fa_ex_forward_kvcache add, for a call it serves: it takes none of them (see _call), any value does
_KV_NOTHING_ADDED = (0,) * (len(_SIGNATURES["fa_ex_forward_kvcache_qv"][1]) - len(_SIGNATURES["fa_ex_forward_kvcache"][1]))


def ex_kvcache_forward(q, k_cache, v_cache, k_new=None, v_new=None, cache_seqlens=None, causal=False, softmax_scale=None,
                       window=(-1, -1), softcap=0.0, alibi_slopes=None, num_splits=0, block_table=None, cache_batch_idx=None,
                       cache_leftpad=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, *, cu_seqlens_q=None,
                       cu_seqlens_k_new=None, max_seqlen_q=None, qv=None, sinks=None, k_descale=None, v_descale=None):
    """(o, lse) of a decode step over a KV cache (FlashAttention-2's flash_attn_with_kvcache, forward): q (B, Nq, H_q, d);
    k_cache, v_cache (B, cache_len, H_kv, d), used in place (strided views such as kv.unbind(2) allowed, never copied);
    k_new, v_new (B, N_new, H_kv, d) are written into the caches at cache_seqlens[b] first; cache_seqlens int32 (B,) on the
    device, or an int.  o (B, Nq, H_q, d) in q's dtype, lse (B, H_q, Nq) float32.  See fa_ex_forward_kvcache.
    block_table int32 (B, max_blocks_per_seq): k_cache, v_cache are pools (num_blocks, page_block_size, H_kv, d) and token t of
    sequence b lives at pool[block_table[b, t // ps], t % ps]; the capacity is max_blocks_per_seq * ps.  cache_batch_idx int32
    (B,): sequence b uses cache row idx[b] of a (B_cache, cache_len, H_kv, d) cache.  cache_leftpad int32 (B,): the keys of
    sequence b start at cache position leftpad[b].  The last two combine; neither goes with block_table.  All on q's device,
    never read on the host.  See fa_ex_forward_kvcache_paged.
    rotary_cos, rotary_sin (seqlen_ro, rotary_dim / 2) in q's dtype on q's device, rotary_dim a multiple of 16 in [16, d]: k_new
    is rotated at its position in the sequence before it is written to the cache, and the kernel's copy of q at the position
    of its token (causal or a window bound given) or of the first new token (neither); pairs (2j, 2j + 1) with
    rotary_interleaved, else (j, j + rotary_dim / 2).  Needs k_new, v_new, cache_seqlens and seqlen_ro >= capacity +
    max(0, Nq - N_new).  See fa_ex_forward_kvcache_rotary.
    k_cache and v_cache may both be torch.float8_e4m3fn (OCP e4m3) while q, k_new, v_new and o stay 16-bit: a stored byte c of
    K head h of sequence b stands for e4m3(c) * k_descale[b, h] (V: v_descale).  k_descale, v_descale: float32 (B, H_kv) (last
    dim contiguous, the row stride is passed through) or contiguous (H_kv,), on q's device, read by the kernels only; None means
    1.0; they must be finite and > 0.  The scale follows the sequence b of the call, not the cache row or page.  k_new / v_new
    are quantised on the append: clamp(float(x) * (1.0f / descale), -448, 448) in fp32, rounded to nearest even.  An e4m3 cache
    view must have strides that are multiples of 8 and an 8-byte aligned address (ValueError otherwise; never copied).  See
    fa_ex_forward_kvcache_fp8.
    sinks: float32 (H_q,) on q's device, one extra softmax column per query head with a zero value; it joins where the splits are
    combined, so such a call runs at least two splits.  lse contains it.  See fa_ex_forward_kvcache_sink.
    sinks, k_descale and v_descale are keyword-only; the two scales stay the trailing keywords.  So are the three below.
    cu_seqlens_q int32 (B + 1,) on q's device with max_seqlen_q (an int, required): q is packed (total_q, H_q, d) — a view with
    a token stride such as qkv[:, 0] is taken as it is — and sequence b owns tokens [cu_seqlens_q[b], cu_seqlens_q[b + 1]), at
    most max_seqlen_q of them, none allowed.  o is then (total_q, H_q, d) and lse (H_q, total_q).  cu_seqlens_k_new int32
    (B + 1,), only with k_new, v_new and cu_seqlens_q: k_new, v_new are packed (total_k_new, H_kv, d) and sequence b appends
    its own count of tokens, independent of its count of q tokens; cu_seqlens_q also goes with padded (B, N_new, H_kv, d) new
    keys, or with none.  Each sequence gets what the padded call returns for it alone (its causal diagonal is len_k_b - nq_b); a
    sequence without q tokens still appends; rows of o and lse that no sequence owns are left as allocated.  Neither array is
    read on the host: the kernels clamp them, as they clamp cache_seqlens, so no content reads or writes out of bounds.  Rotary
    needs seqlen_ro >= capacity + max_seqlen_q.  A 4-D q with cu_seqlens_q, a missing max_seqlen_q and a packed q that would need
    a copy raise ValueError.  See fa_ex_forward_kvcache_varlen.
    qv (keyword-only; FlashAttention-3's): a second query operand (B, Nq, H_q, 512) in q's dtype for K and V of different widths,
    multi-head latent attention at decode time.  q and k_cache are then 64 wide, v_cache (.., H_kv, 512), o (B, Nq, H_q, 512), the
    score is softmax_scale * (q . k + qv . v) and softmax_scale defaults to (64 + 512) ** -0.5.  k_cache and v_cache may be the two
    slices of one (.., 576) pool: each view's own page and token strides are taken, never a copy (ValueError where that is not
    possible); a token-strided qv is taken as it is.  Goes with cache_seqlens, cache_batch_idx, block_table, causal, window,
    softmax_scale and num_splits; other widths, k_new / v_new, cu_seqlens_k_new, rotary_cos / rotary_sin, an e4m3 cache with
    k_descale / v_descale, softcap, alibi_slopes, sinks, cu_seqlens_q and cache_leftpad raise NotImplementedError with the name.
    See fa_ex_forward_kvcache_qv."""
    who = "ex_kvcache_forward"
    if qv is not None:
        for name, val in (("k / v (new tokens to append)", k_new if k_new is not None else v_new), ("cu_seqlens_k_new", cu_seqlens_k_new),
                          ("rotary_cos / rotary_sin", rotary_cos if rotary_cos is not None else rotary_sin),
                          ("k_descale / v_descale", k_descale if k_descale is not None else v_descale),
                          ("softcap", softcap or None), ("alibi_slopes", alibi_slopes), ("sinks", sinks), ("cu_seqlens_q", cu_seqlens_q),
                          ("cache_leftpad", cache_leftpad)):
            if val is not None:
                raise NotImplementedError(f"{who}: qv cannot be combined with {name}")
    wl, wr = window_arg(who, window)
    cap = softcap_arg(who, softcap)
    packed = cu_seqlens_q is not None
    if cu_seqlens_k_new is not None and not packed:
        raise ValueError(f"{who}: cu_seqlens_k_new needs cu_seqlens_q")
    if max_seqlen_q is not None and not packed:
        raise ValueError(f"{who}: max_seqlen_q needs cu_seqlens_q")
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)) + ((("qv", qv),) if qv is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a GPU (HIP device) tensor; there is no CPU path")
        if t.device != q.device:
            raise RuntimeError(f"{who}: {name} must be on q's device ({q.device}), got {t.device}")
        if packed and name == "q":
            if t.dim() != 3:
                raise ValueError(f"{who}: with cu_seqlens_q q must be packed (total_q, H_q, d), got {tuple(t.shape)}")
        elif t.dim() != 4:
            raise RuntimeError(f"{who}: {name} must be 4-D (B, N, H, d), got {tuple(t.shape)}")
    total_q = total_kn = mq = 0
    if packed:
        if max_seqlen_q is None:
            raise ValueError(f"{who}: cu_seqlens_q needs max_seqlen_q")
        for name, t in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k_new", cu_seqlens_k_new)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
                raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (int32 tensor expected)")
            if t.device != q.device or t.dim() != 1 or t.shape[0] < 2 or t.shape != cu_seqlens_q.shape:
                raise RuntimeError(f"{who}: {name} must be an int32 (B + 1,) tensor on q's device, B >= 1, both of one length")
        total_q, mq = q.shape[0], operator.index(max_seqlen_q)
        if mq < 0 or mq > total_q:
            raise ValueError(f"{who}: max_seqlen_q = {mq} must lie in [0, total_q = {total_q}]")
        q = q.unsqueeze(0)   # (1, total_q, H_q, d) for the shape checks below; never copied
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype in _FLOAT8_DTYPES and t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (an 8-bit cache is torch.float8_e4m3fn)")
    e4m3 = k_cache.dtype == torch.float8_e4m3fn and v_cache.dtype == torch.float8_e4m3fn
    if q.dtype not in (torch.float16, torch.bfloat16) or k_cache.dtype != v_cache.dtype or (not e4m3 and k_cache.dtype != q.dtype):
        raise RuntimeError(f"{who}: q must have a 16-bit dtype (float16 or bfloat16) and k_cache, v_cache both q's dtype or both "
                           f"torch.float8_e4m3fn, got {q.dtype}, {k_cache.dtype}, {v_cache.dtype}")
    if not e4m3 and (k_descale is not None or v_descale is not None):
        raise RuntimeError(f"{who}: k_descale / v_descale need a torch.float8_e4m3fn cache (the caches are {k_cache.dtype})")
    b, nq, hq, d = q.shape
    if packed:
        b, nq = cu_seqlens_q.shape[0] - 1, mq
    cap_len, hkv = k_cache.shape[1], k_cache.shape[2]
    dv = d   # the width of v_cache and o
    if qv is not None:
        if e4m3:
            raise NotImplementedError(f"{who}: qv cannot be combined with an e4m3 cache (k_descale / v_descale)")
        dv = v_cache.shape[3]
        if (d, dv) != (64, 512):
            raise NotImplementedError(f"{who}: qv is supported for q, k_cache of head dim 64 with v_cache of head dim 512 only "
                                      f"(got {d}, {dv})")
        if qv.dtype != q.dtype or qv.shape != (b, nq, hq, dv):
            raise RuntimeError(f"{who}: qv must be a (B, Nq, H_q, {dv}) = ({b}, {nq}, {hq}, {dv}) tensor of q's dtype, got "
                               f"{qv.dtype}, {tuple(qv.shape)}")
    for name, t, shape in (("block_table", block_table, "(B, max_blocks_per_seq)"), ("cache_batch_idx", cache_batch_idx, "(B,)"),
                           ("cache_leftpad", cache_leftpad, "(B,)")):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != q.device or \
                t.dim() != (2 if name == "block_table" else 1) or t.shape[0] != b or t.numel() == 0:
            raise RuntimeError(f"{who}: {name} must be an int32 {shape} tensor on q's device, B = {b}")
    if block_table is not None and (cache_batch_idx is not None or cache_leftpad is not None):
        raise RuntimeError(f"{who}: block_table cannot be combined with cache_batch_idx or cache_leftpad")
    units = b   # leading dim of the caches: pages, cache rows, or batch elements
    if block_table is not None:
        units = k_cache.shape[0]
        if cap_len < 16 or cap_len % 16 != 0:
            raise RuntimeError(f"{who}: page_block_size (k_cache.shape[1]) must be a positive multiple of 16, got {cap_len}")
    elif cache_batch_idx is not None:
        units = k_cache.shape[0]
    if units == 0 or k_cache.shape != (units, cap_len, hkv, d) or v_cache.shape != (units, cap_len, hkv, dv):
        what = "(num_blocks, page_block_size, H_kv, d)" if block_table is not None else \
            "(B_cache, cache_len, H_kv, d)" if cache_batch_idx is not None else "(B, cache_len, H_kv, d)"
        raise RuntimeError(f"{who}: k_cache and v_cache must be {what} = ({units}, ., ., {d}); got "
                           f"{tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    if d % 8 != 0 or not 8 <= d <= 256:
        raise RuntimeError(f"{who}: head dim must be a multiple of 8 in [8, 256], got {d}")
    if hkv == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: the query heads ({hq}) must be a multiple of the K/V heads ({hkv})")
    if (k_new is None) != (v_new is None):
        raise RuntimeError(f"{who}: k and v must be given together")
    if (rotary_cos is None) != (rotary_sin is None):
        raise RuntimeError(f"{who}: rotary_cos and rotary_sin must be given together")
    rdim = 0
    if rotary_cos is not None:
        for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != q.dtype or t.device != q.device or t.dim() != 2 or \
                    t.shape != rotary_cos.shape or t.numel() == 0:
                raise RuntimeError(f"{who}: {name} must be a (seqlen_ro, rotary_dim / 2) tensor of q's dtype on q's device, "
                                   f"rotary_cos and rotary_sin of one shape")
        rdim = 2 * rotary_cos.shape[1]
        if rdim % 16 != 0 or not 16 <= rdim <= d:
            raise RuntimeError(f"{who}: rotary_dim = 2 * rotary_cos.shape[1] must be a multiple of 16 in [16, d = {d}], got {rdim}")
        if k_new is None or cache_seqlens is None:
            raise RuntimeError(f"{who}: rotary_cos / rotary_sin need k, v (the new tokens) and cache_seqlens")
    kvb, kvt = _kv_strides(who, "k_cache", k_cache, hkv, d, True)
    vvb, vvt = _kv_strides(who, "v_cache", v_cache, hkv, dv, True)
    kdp, vdp, dsc_bs, _scales = _kv_descales(who, k_descale, v_descale, q, b, hkv)
    if e4m3:
        for name, t, bs_, ts_ in (("k_cache", k_cache, kvb, kvt), ("v_cache", v_cache, vvb, vvt)):
            if bs_ % 8 != 0 or ts_ % 8 != 0 or t.data_ptr() % 8 != 0:
                raise ValueError(f"{who}: an e4m3 {name} must be 8-byte aligned with batch and token strides that are multiples "
                                 f"of 8 elements (got address % 8 = {t.data_ptr() % 8}, strides {tuple(t.stride())}); the cache "
                                 f"is never copied")
    nnew = 0
    knb = knt = vnb = vnt = 0
    if cu_seqlens_k_new is not None:
        if k_new is None:
            raise ValueError(f"{who}: cu_seqlens_k_new needs k and v")
        for name, t in (("k", k_new), ("v", v_new)):
            if not isinstance(t, torch.Tensor) or t.device != q.device or t.dtype != q.dtype or t.dim() != 3 or \
                    t.shape[1:] != (hkv, d) or t.shape != k_new.shape:
                raise RuntimeError(f"{who}: with cu_seqlens_k_new {name} must be a packed (total_k_new, H_kv, d) tensor of q's "
                                   f"dtype and device")
        total_kn = k_new.shape[0]
        nnew = min(total_kn, 1)   # (for the checks below: new tokens or none)
        k_new, v_new = k_new.contiguous().unsqueeze(0), v_new.contiguous().unsqueeze(0)
        _kb, knt = _kv_strides(who, "k", k_new, hkv, d, False)
        _vb, vnt = _kv_strides(who, "v", v_new, hkv, d, False)
    elif k_new is not None:
        for name, t in (("k", k_new), ("v", v_new)):
            if not isinstance(t, torch.Tensor) or t.device != q.device or t.dtype != q.dtype or t.dim() != 4 or \
                    t.shape[0] != b or t.shape[2:] != (hkv, d) or t.shape != k_new.shape:
                raise RuntimeError(f"{who}: {name} must be a (B, N_new, H_kv, d) tensor of q's dtype and device")
        nnew = k_new.shape[1]
        k_new, v_new = k_new.contiguous(), v_new.contiguous()
        knb, knt = _kv_strides(who, "k", k_new, hkv, d, False)
        vnb, vnt = _kv_strides(who, "v", v_new, hkv, d, False)
    if rotary_cos is not None:
        capacity = cap_len * (block_table.shape[1] if block_table is not None else 1)
        # the library's bound: every position a clamped length can give is a table row
        need = capacity + (mq if packed else max(0, nq - nnew))
        if rotary_cos.shape[0] < need:
            raise RuntimeError(f"{who}: rotary_cos / rotary_sin have {rotary_cos.shape[0]} rows; the capacity {capacity} + "
                               f"{'max_seqlen_q' if packed else 'max(0, Nq - N_new)'} = {need} are needed")
    if packed:   # a token-strided view is taken as it is; anything else would need a copy
        if q.stride(3) != 1 or (hq > 1 and q.stride(2) != d) or (total_q > 1 and (q.stride(1) < hq * d or q.stride(1) % 8)) or \
                q.data_ptr() % 16:
            raise ValueError(f"{who}: a packed q must have a contiguous last dim, its heads at stride d = {d}, a token stride that "
                             f"is a multiple of 8 and >= H_q d, and a 16-byte aligned address (got strides {tuple(q.stride()[1:])}); "
                             f"it is never copied")
    else:
        q = q.contiguous()
    qb, qt = _kv_strides(who, "q", q, hq, d, False)
    qvb = qvt = 0
    if qv is not None:   # a view whose heads are adjacent is taken as it is (a token-strided one, say); anything else is copied
        if qv.stride(3) != 1 or (hq > 1 and qv.stride(2) != dv) or qv.stride(1) % 8 or qv.stride(0) % 8 or qv.data_ptr() % 16 or \
                (nq > 1 and qv.stride(1) < hq * dv) or (b > 1 and qv.stride(0) < (nq - 1) * qv.stride(1) + hq * dv):
            qv = qv.contiguous()
        qvb, qvt = _kv_strides(who, "qv", qv, hq, dv, False)
    scale = (d + (dv if qv is not None else 0)) ** -0.5 if softmax_scale is None else float(softmax_scale)
    aptr, _h, astride, alibi_slopes = alibi_arg(who, alibi_slopes, q.device, b * hq, heads=hq)
    sptr, sheads, sinks = sinks_arg(who, sinks, q.device, b * hq, heads=hq)
    with torch.cuda.device(q.device):
        if cache_seqlens is not None and not isinstance(cache_seqlens, torch.Tensor):
            cache_seqlens = torch.full((b,), operator.index(cache_seqlens), dtype=torch.int32, device=q.device)
        if cache_seqlens is not None:
            if cache_seqlens.device != q.device or cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (b,):
                raise RuntimeError(f"{who}: cache_seqlens must be an int32 ({b},) tensor on q's device, or an int")
            cache_seqlens = cache_seqlens.contiguous()
        # the narrowest entry point that takes what the call carries (each adds a group of arguments to the one before), its
        # workspace query, and those groups: marshalled in one place, and not at all for a call that carries none of them
        variant = "_qv" if qv is not None else "_varlen" if packed else "_sink" if sptr else "_fp8" if e4m3 else "_rotary" if rotary_cos is not None else \
            "_paged" if (block_table is not None or cache_batch_idx is not None or cache_leftpad is not None) else ""
        code, capacity, added = _DTYPE_CODE[q.dtype], cap_len, _KV_NOTHING_ADDED
        if variant:
            cu_q, cu_kn = _contiguous(cu_seqlens_q), _contiguous(cu_seqlens_k_new)
            cache_batch_idx, cache_leftpad = _contiguous(cache_batch_idx), _contiguous(cache_leftpad)
            paged = (0, 0, 0, 0, 0)   # block_table, its row stride, num_blocks, page_block_size, max_blocks_per_seq
            if block_table is not None:
                if block_table.stride(1) != 1:
                    block_table = block_table.contiguous()
                capacity = block_table.shape[1] * cap_len
                paged = (block_table.data_ptr(), block_table.stride(0) if b > 1 else max(block_table.stride(0), block_table.shape[1]),
                         units, cap_len, block_table.shape[1])
            _tabs, rotary = _rotary_tables(rotary_cos, rotary_sin, rdim, rotary_interleaved)
            added = (*paged, _ptr(cache_batch_idx), 0 if cache_batch_idx is None else units, _ptr(cache_leftpad), *rotary,
                     _E4M3_CODE if e4m3 else code, kdp, vdp, dsc_bs, sptr, sheads, _ptr(cu_q), _ptr(cu_kn), total_q, mq, total_kn,
                     _ptr(qv), qvb, qvt, dv if qv is not None else 0)
        if packed:
            o = torch.empty((total_q, hq, d), dtype=q.dtype, device=q.device)
            lse = torch.empty((hq, total_q), dtype=torch.float32, device=q.device)
            nbytes = int(_lib.fa_ex_kvcache_workspace_bytes_varlen(b, hq, hkv, total_q, mq, capacity, d, int(num_splits), int(bool(sptr))))
        elif qv is not None:
            o = torch.empty((b, nq, hq, dv), dtype=q.dtype, device=q.device)
            lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
            nbytes = int(_lib.fa_ex_kvcache_workspace_bytes_qv(b, hq, hkv, b * nq, nq, capacity, d, int(num_splits), 0, dv))
        else:
            o = torch.empty((b, nq, hq, d), dtype=q.dtype, device=q.device)
            lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
            ws_bytes = _lib.fa_ex_kvcache_workspace_bytes_sink if sptr else _lib.fa_ex_kvcache_workspace_bytes
            nbytes = int(ws_bytes(b, hq, hkv, nq, capacity, d, int(num_splits)))
        ws = _workspace(q.device, nbytes) if nbytes > 0 else None
        _call("fa_ex_forward_kvcache" + variant, (
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_new.data_ptr() if k_new is not None else 0,
            v_new.data_ptr() if v_new is not None else 0, cache_seqlens.data_ptr() if cache_seqlens is not None else 0, o.data_ptr(), lse.data_ptr(),
            b, hq, hkv, 0 if packed else nq, 0 if cu_seqlens_k_new is not None else nnew, cap_len, d, code,
            0 if packed else qb, qt, kvb, kvt, vvb, vvt, knb, knt, vnb, vnt,
            int(bool(causal)), wl, wr, scale, cap, aptr, astride, int(num_splits), *added,
            ws.data_ptr() if ws is not None else 0, nbytes, _stream_ptr(q.device)))
    return o, lse


def _index_strides(indices, b, nq, hkv, topk):
    """(indices, batch stride, token stride, head stride) of the lists of a sparse call as the library addresses them: the topk
    entries of a list adjacent, head stride 0 for a (B, Nq, topk) tensor or a view expanded over the K/V heads, lists that do not
    overlap.  Any other view is copied (the lists are only read)."""
    def strides(t):
        ixh = t.stride(2) if t.dim() == 4 and hkv > 1 else 0
        span = (hkv - 1) * ixh + topk if ixh else topk                 # entries of one token's lists
        ixt = t.stride(1) if nq > 1 else span
        ixb = t.stride(0) if b > 1 else (nq - 1) * ixt + span
        ok = (ixh == 0 or ixh >= topk) and ixt >= span and ixb >= (nq - 1) * ixt + span
        return ok, ixb, ixt, ixh
    if indices.numel() == 0:
        return indices, 0, 0, 0
    ok, ixb, ixt, ixh = strides(indices)
    if not ok or indices.stride(-1) != 1 or indices.data_ptr() % 4:
        indices = indices.contiguous()
        ok, ixb, ixt, ixh = strides(indices)
    return indices, ixb, ixt, ixh


def ex_mla_sparse_forward(q, qv, k_cache, v_cache, indices, cache_seqlens=None, causal=False, softmax_scale=None, block_table=None,
                          cache_batch_idx=None, num_splits=0):
    """(o, lse) of sparse MLA decoding: ex_kvcache_forward(q, k_cache, v_cache, qv=qv, ...) over a list of cached tokens per query
    token.  q (B, Nq, H_q, 64), qv (B, Nq, H_q, 512), k_cache (.., H_kv, 64), v_cache (.., H_kv, 512) as that call takes them
    (contiguous, cache_batch_idx rows, or pools under block_table; cache views are never copied); indices int32 (B, Nq, topk) or
    (B, Nq, H_kv, topk) on q's device: entry j is a token position of sequence b, a key iff 0 <= entry < cache_seqlens[b] (and
    <= cache_seqlens[b] - Nq + i if causal); anything else is skipped and never read.  Never read on the host.  o (B, Nq, H_q, 512)
    in q's dtype, lse (B, H_q, Nq) float32; softmax_scale defaults to (64 + 512) ** -0.5.  See fa_mla_sparse_forward."""
    who = "ex_mla_sparse_forward"
    for name, t in (("q", q), ("qv", qv), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a GPU (HIP device) tensor; there is no CPU path")
        if t.device != q.device:
            raise RuntimeError(f"{who}: {name} must be on q's device ({q.device}), got {t.device}")
        if t.dim() != 4:
            raise RuntimeError(f"{who}: {name} must be 4-D (B, N, H, d), got {tuple(t.shape)}")
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32:
        dt = indices.dtype if isinstance(indices, torch.Tensor) else type(indices).__name__
        raise NotImplementedError(f"{who}: indices of dtype {dt} is not supported (int32 tensor expected)")
    if q.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q.dtype for t in (qv, k_cache, v_cache)):
        raise RuntimeError(f"{who}: q, qv, k_cache and v_cache must share a 16-bit dtype (float16 or bfloat16), got {q.dtype}, "
                           f"{qv.dtype}, {k_cache.dtype}, {v_cache.dtype}")
    b, nq, hq, d = q.shape
    cap_len, hkv, dv = k_cache.shape[1], k_cache.shape[2], v_cache.shape[3]
    if (d, dv) != (64, 512):
        raise NotImplementedError(f"{who}: supported for q, k_cache of head dim 64 with v_cache of head dim 512 only (got {d}, {dv})")
    if qv.shape != (b, nq, hq, dv):
        raise RuntimeError(f"{who}: qv must be a (B, Nq, H_q, {dv}) = ({b}, {nq}, {hq}, {dv}) tensor, got {tuple(qv.shape)}")
    if hkv == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: the query heads ({hq}) must be a multiple of the K/V heads ({hkv})")
    for name, t, shape in (("block_table", block_table, "(B, max_blocks_per_seq)"), ("cache_batch_idx", cache_batch_idx, "(B,)")):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != q.device or \
                t.dim() != (2 if name == "block_table" else 1) or t.shape[0] != b or t.numel() == 0:
            raise RuntimeError(f"{who}: {name} must be an int32 {shape} tensor on q's device, B = {b}")
    if block_table is not None and cache_batch_idx is not None:
        raise RuntimeError(f"{who}: block_table cannot be combined with cache_batch_idx")
    units = b if block_table is None and cache_batch_idx is None else k_cache.shape[0]
    if block_table is not None and (cap_len < 16 or cap_len % 16 != 0):
        raise RuntimeError(f"{who}: page_block_size (k_cache.shape[1]) must be a positive multiple of 16, got {cap_len}")
    if units == 0 or cap_len == 0 or k_cache.shape != (units, cap_len, hkv, d) or v_cache.shape != (units, cap_len, hkv, dv):
        what = "(num_blocks, page_block_size, H_kv, .)" if block_table is not None else \
            "(B_cache, cache_len, H_kv, .)" if cache_batch_idx is not None else "(B, cache_len, H_kv, .)"
        raise RuntimeError(f"{who}: k_cache and v_cache must be {what} = ({units}, ., ., {d} | {dv}); got "
                           f"{tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    if indices.device != q.device or indices.dim() not in (3, 4) or indices.shape[:2] != (b, nq) or \
            (indices.dim() == 4 and indices.shape[2] != hkv):
        raise RuntimeError(f"{who}: indices must be an int32 (B, Nq, topk) or (B, Nq, H_kv, topk) = ({b}, {nq}, [{hkv},] topk) tensor on "
                           f"q's device, got {tuple(indices.shape)} on {indices.device}")
    topk = indices.shape[-1]
    indices, ixb, ixt, ixh = _index_strides(indices, b, nq, hkv, topk)
    kvb, kvt = _kv_strides(who, "k_cache", k_cache, hkv, d, True)
    vvb, vvt = _kv_strides(who, "v_cache", v_cache, hkv, dv, True)
    q = q.contiguous()
    qb, qt = _kv_strides(who, "q", q, hq, d, False)
    if qv.stride(3) != 1 or (hq > 1 and qv.stride(2) != dv) or qv.stride(1) % 8 or qv.stride(0) % 8 or qv.data_ptr() % 16 or \
            (nq > 1 and qv.stride(1) < hq * dv) or (b > 1 and qv.stride(0) < (nq - 1) * qv.stride(1) + hq * dv):
        qv = qv.contiguous()   # a view whose heads are adjacent (a token-strided one, say) is taken as it is
    qvb, qvt = _kv_strides(who, "qv", qv, hq, dv, False)
    scale = (d + dv) ** -0.5 if softmax_scale is None else float(softmax_scale)
    with torch.cuda.device(q.device):
        if cache_seqlens is not None and not isinstance(cache_seqlens, torch.Tensor):
            cache_seqlens = torch.full((b,), operator.index(cache_seqlens), dtype=torch.int32, device=q.device)
        if cache_seqlens is not None:
            if cache_seqlens.device != q.device or cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (b,):
                raise RuntimeError(f"{who}: cache_seqlens must be an int32 ({b},) tensor on q's device, or an int")
            cache_seqlens = cache_seqlens.contiguous()
        cache_batch_idx = _contiguous(cache_batch_idx)
        paged = (0, 0, 0, 0, 0)   # block_table, its row stride, num_blocks, page_block_size, max_blocks_per_seq
        if block_table is not None:
            if block_table.stride(1) != 1:
                block_table = block_table.contiguous()
            paged = (block_table.data_ptr(), block_table.stride(0) if b > 1 else max(block_table.stride(0), block_table.shape[1]),
                     units, cap_len, block_table.shape[1])
        o = torch.empty((b, nq, hq, dv), dtype=q.dtype, device=q.device)
        lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
        nbytes = int(_lib.fa_mla_sparse_workspace_bytes(b, hq, hkv, nq, topk, int(num_splits))) if b and nq and hq else 0
        ws = _workspace(q.device, nbytes) if nbytes > 0 else None
        _call("fa_mla_sparse_forward", (
            q.data_ptr(), qv.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), indices.data_ptr(), _ptr(cache_seqlens), o.data_ptr(),
            lse.data_ptr(), b, hq, hkv, nq, cap_len, topk, d, dv, _DTYPE_CODE[q.dtype], qb, qt, qvb, qvt, kvb, kvt, vvb, vvt, ixb, ixt, ixh,
            int(bool(causal)), scale, int(num_splits), *paged, _ptr(cache_batch_idx), 0 if cache_batch_idx is None else units,
            ws.data_ptr() if ws is not None else 0, nbytes, _stream_ptr(q.device)))
    return o, lse


# ---- the packed 8-bit latent cache (include/fa_mi355x.h: fa_mla_fp8_forward, fa_mla_fp8_pack) ----
MLA_FP8_TOKEN_BYTES = 656   # 512 e4m3 | 4 float32 scales | 64 bf16


def _f8_pool(who, kv_cache, device):
    """(the pool as bytes, page stride, token stride, num_blocks, page_block_size) of a packed (num_blocks, page_block_size, 1, 656)
    uint8 / float8_e4m3fn cache; a view of a wider allocation keeps its strides, nothing is copied"""
    if not isinstance(kv_cache, torch.Tensor) or kv_cache.dtype not in (torch.uint8, torch.float8_e4m3fn):
        dt = kv_cache.dtype if isinstance(kv_cache, torch.Tensor) else type(kv_cache).__name__
        raise NotImplementedError(f"{who}: kv_cache of dtype {dt} is not supported (torch.uint8 or torch.float8_e4m3fn bytes expected)")
    if not kv_cache.is_cuda or kv_cache.device != device:
        raise RuntimeError(f"{who}: kv_cache must be a GPU (HIP device) tensor on q's device; there is no CPU path")
    if kv_cache.dim() != 4 or kv_cache.shape[2:] != (1, MLA_FP8_TOKEN_BYTES) or kv_cache.shape[0] == 0:
        raise RuntimeError(f"{who}: kv_cache must be (num_blocks, page_block_size, 1, {MLA_FP8_TOKEN_BYTES}), got {tuple(kv_cache.shape)}")
    nblk, ps = kv_cache.shape[:2]
    if ps < 16 or ps % 16 != 0:
        raise RuntimeError(f"{who}: page_block_size (kv_cache.shape[1]) must be a positive multiple of 16, got {ps}")
    tsb = kv_cache.stride(1)
    psb = kv_cache.stride(0) if nblk > 1 else max(kv_cache.stride(0), (ps - 1) * tsb + MLA_FP8_TOKEN_BYTES)
    if kv_cache.stride(3) != 1 or tsb < MLA_FP8_TOKEN_BYTES or tsb % 16 or psb % 16 or psb < (ps - 1) * tsb + MLA_FP8_TOKEN_BYTES or \
            kv_cache.data_ptr() % 16:
        raise ValueError(f"{who}: kv_cache must have contiguous 656-byte tokens at a stride that is a multiple of 16, pages that do not "
                         f"overlap at a stride that is a multiple of 16, and a 16-byte aligned address (got strides "
                         f"{tuple(kv_cache.stride())}); it is never copied")
    return kv_cache, psb, tsb, nblk, ps


def _f8_table(who, block_table, cache_seqlens, b, device, need_lens):
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32:
        dt = block_table.dtype if isinstance(block_table, torch.Tensor) else type(block_table).__name__
        raise NotImplementedError(f"{who}: block_table of dtype {dt} is not supported (int32 tensor expected)")
    if block_table.device != device or block_table.dim() != 2 or block_table.shape[0] != b or block_table.numel() == 0:
        raise RuntimeError(f"{who}: block_table must be an int32 (B, max_blocks_per_seq) tensor on q's device, B = {b}")
    if cache_seqlens is None and need_lens:
        raise RuntimeError(f"{who}: cache_seqlens must be an int32 ({b},) tensor on the device, or an int")
    if cache_seqlens is not None and not isinstance(cache_seqlens, (torch.Tensor, numbers.Integral)):
        raise NotImplementedError(f"{who}: cache_seqlens of type {type(cache_seqlens).__name__} is not supported (int32 tensor or int expected)")
    if isinstance(cache_seqlens, torch.Tensor):
        if cache_seqlens.dtype != torch.int32:
            raise NotImplementedError(f"{who}: cache_seqlens of dtype {cache_seqlens.dtype} is not supported (int32 tensor expected)")
        if cache_seqlens.device != device or cache_seqlens.shape != (b,):
            raise RuntimeError(f"{who}: cache_seqlens must be an int32 ({b},) tensor on q's device, or an int")


def _f8_table_args(block_table, cache_seqlens, b, device):
    """(cache_seqlens, block_table, its row stride, max_blocks_per_seq) as handed to the library; inside torch.cuda.device"""
    if cache_seqlens is not None and not isinstance(cache_seqlens, torch.Tensor):
        cache_seqlens = torch.full((b,), operator.index(cache_seqlens), dtype=torch.int32, device=device)
    cache_seqlens = _contiguous(cache_seqlens)
    if block_table.stride(1) != 1:
        block_table = block_table.contiguous()
    trs = block_table.stride(0) if b > 1 else max(block_table.stride(0), block_table.shape[1])
    return cache_seqlens, block_table, trs, block_table.shape[1]


def _f8_rows(who, name, t, heads, width):
    """(batch, token, head) strides of a (B, N, heads, width) bf16 view as the packed calls address it; anything they cannot
    address is copied (the tensor is only read)"""
    def ok(t):
        b, n = t.shape[:2]
        hs = t.stride(2) if heads > 1 else width
        tok = (heads - 1) * hs + width
        ts = t.stride(1) if n > 1 else tok
        bs = t.stride(0) if b > 1 else (n - 1) * ts + tok
        good = t.stride(3) == 1 and hs >= width and ts >= tok and bs >= (n - 1) * ts + tok and not (hs % 8 or ts % 8 or bs % 8 or t.data_ptr() % 16)
        return good, bs, ts, hs
    good, bs, ts, hs = ok(t)
    if not good:
        t = t.contiguous()
        good, bs, ts, hs = ok(t)
    return t, bs, ts, hs


def ex_mla_fp8_forward(q, qv, kv_cache, block_table, cache_seqlens=None, indices=None, causal=False, softmax_scale=None, num_splits=0):
    """(o, lse) of MLA decoding from a packed 8-bit latent cache (FlashMLA's 656-byte token: 512 e4m3 | 4 float32 tile scales | 64
    bf16): q (B, Nq, H_q, 64) and qv (B, Nq, H_q, 512) bfloat16 — views such as the two column ranges of one (B, Nq, H_q, 576)
    tensor are used with their own strides; kv_cache (num_blocks, page_block_size, 1, 656) torch.uint8 or torch.float8_e4m3fn,
    read as bytes, a view of a wider allocation with its own strides, never copied; block_table int32 (B, max_blocks_per_seq);
    cache_seqlens int32 (B,), an int or None (the capacity); indices None (every cached token: ex_kvcache_forward(..., qv=qv) on
    the dequantised pool, to the bit) or int32 (B, Nq, topk) (ex_mla_sparse_forward on it, to the bit).  o (B, Nq, H_q, 512)
    bfloat16, lse (B, H_q, Nq) float32; softmax_scale defaults to (64 + 512) ** -0.5.  See fa_mla_fp8_forward."""
    who = "ex_mla_fp8_forward"
    for name, t in (("q", q), ("qv", qv)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a GPU (HIP device) tensor; there is no CPU path")
        if t.device != q.device:
            raise RuntimeError(f"{who}: {name} must be on q's device ({q.device}), got {t.device}")
        if t.dim() != 4:
            raise RuntimeError(f"{who}: {name} must be 4-D (B, Nq, H_q, d), got {tuple(t.shape)}")
    if q.dtype != torch.bfloat16 or qv.dtype != torch.bfloat16:
        raise NotImplementedError(f"{who}: q and qv of dtype {q.dtype}, {qv.dtype} are not supported (torch.bfloat16 expected: the rotary "
                                  f"part of a packed token is bfloat16)")
    if indices is not None and not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int32):
        dt = indices.dtype if isinstance(indices, torch.Tensor) else type(indices).__name__
        raise NotImplementedError(f"{who}: indices of dtype {dt} is not supported (int32 tensor expected)")
    b, nq, hq, d = q.shape
    dv = qv.shape[3]
    if (d, dv) != (64, 512):
        raise NotImplementedError(f"{who}: supported for q of head dim 64 with qv of head dim 512 only (got {d}, {dv})")
    if qv.shape != (b, nq, hq, dv):
        raise RuntimeError(f"{who}: qv must be a (B, Nq, H_q, {dv}) = ({b}, {nq}, {hq}, {dv}) tensor, got {tuple(qv.shape)}")
    kv_cache, psb, tsb, nblk, ps = _f8_pool(who, kv_cache, q.device)
    _f8_table(who, block_table, cache_seqlens, b, q.device, False)
    topk = ixb = ixt = 0
    if indices is not None:
        if indices.device != q.device or indices.dim() != 3 or indices.shape[:2] != (b, nq):
            raise RuntimeError(f"{who}: indices must be an int32 (B, Nq, topk) = ({b}, {nq}, topk) tensor on q's device, got "
                               f"{tuple(indices.shape)} on {indices.device}")
        topk = indices.shape[-1]
        indices, ixb, ixt, _ixh = _index_strides(indices, b, nq, 1, topk)
        if indices.numel() == 0:   # (a non-null address selects the list call; nothing is read through it)
            indices = torch.zeros((1,), dtype=torch.int32, device=q.device) if b and nq else indices
    q, qb, qt, qh = _f8_rows(who, "q", q, hq, d)
    qv, qvb, qvt, qvh = _f8_rows(who, "qv", qv, hq, dv)
    scale = (d + dv) ** -0.5 if softmax_scale is None else float(softmax_scale)
    with torch.cuda.device(q.device):
        cache_seqlens, block_table, trs, mb = _f8_table_args(block_table, cache_seqlens, b, q.device)
        o = torch.empty((b, nq, hq, dv), dtype=q.dtype, device=q.device)
        lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
        nbytes = int(_lib.fa_mla_fp8_workspace_bytes(b, hq, 1, nq, mb * ps, topk, int(indices is not None), int(num_splits))) if b and nq and hq else 0
        ws = _workspace(q.device, nbytes) if nbytes > 0 else None
        _call("fa_mla_fp8_forward", (
            q.data_ptr(), qv.data_ptr(), kv_cache.data_ptr(), _ptr(indices), _ptr(cache_seqlens), block_table.data_ptr(), o.data_ptr(),
            lse.data_ptr(), b, hq, 1, nq, topk, d, dv, _DTYPE_CODE[q.dtype], qb, qt, qh, qvb, qvt, qvh, psb, tsb, ixb, ixt, trs, nblk, ps, mb,
            int(bool(causal)), scale, int(num_splits), ws.data_ptr() if ws is not None else 0, nbytes, _stream_ptr(q.device)))
    return o, lse


def ex_mla_fp8_pack(latent_new, rope_new, kv_cache, cache_seqlens, block_table, scale_pow2=False):
    """Quantise and append new tokens to a packed 8-bit latent cache, in place (fa_mla_fp8_pack): latent_new (B, N_new, 512) and
    rope_new (B, N_new, 64) bfloat16 on the GPU — the two column ranges of one (B, N_new, 576) tensor are used as they are —
    go to positions cache_seqlens[b] .. + N_new of sequence b (cache_seqlens: int32 (B,) lengths before the append, or an int)
    through block_table; a token whose position or page falls outside the table or the pool is dropped.  Returns None."""
    who = "ex_mla_fp8_pack"
    for name, t, w in (("latent_new", latent_new, 512), ("rope_new", rope_new, 64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a GPU (HIP device) tensor; there is no CPU path")
        if t.dtype != torch.bfloat16:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.bfloat16 expected)")
        if t.device != latent_new.device or t.dim() != 3 or t.shape[2] != w or t.shape[:2] != latent_new.shape[:2]:
            raise RuntimeError(f"{who}: latent_new and rope_new must be (B, N_new, 512) and (B, N_new, 64) on one device, got "
                               f"{tuple(latent_new.shape)}, {tuple(rope_new.shape)}")
    b, nnew = latent_new.shape[:2]
    dev = latent_new.device
    kv_cache, psb, tsb, nblk, ps = _f8_pool(who, kv_cache, dev)
    _f8_table(who, block_table, cache_seqlens, b, dev, True)
    latent_new, lb, lt, _h = _f8_rows(who, "latent_new", latent_new.unsqueeze(2), 1, 512)
    rope_new, rb, rt, _h = _f8_rows(who, "rope_new", rope_new.unsqueeze(2), 1, 64)
    with torch.cuda.device(dev):
        cache_seqlens, block_table, trs, mb = _f8_table_args(block_table, cache_seqlens, b, dev)
        _call("fa_mla_fp8_pack", (
            latent_new.data_ptr(), rope_new.data_ptr(), kv_cache.data_ptr(), cache_seqlens.data_ptr(), block_table.data_ptr(), b, nnew,
            lb, lt, rb, rt, psb, tsb, trs, nblk, ps, mb, int(bool(scale_pow2)), _stream_ptr(dev)))


# ---- the lightning indexer (include/fa_mi355x.h: fa_indexer_pack, fa_indexer_logits, fa_indexer_topk) ----
INDEXER_TOKEN_BYTES = 132   # 128 e4m3 | 1 float32 scale
INDEXER_DIM = 128


def _idx_pool(who, k_cache, device):
    """(page stride, token stride, num_blocks, page_block_size) in bytes of a (num_blocks, page_block_size, 1, W >= 132) uint8 /
    float8_e4m3fn index-key pool; a view of a wider allocation keeps its strides, nothing is copied"""
    if not isinstance(k_cache, torch.Tensor) or k_cache.dtype not in (torch.uint8, torch.float8_e4m3fn):
        dt = k_cache.dtype if isinstance(k_cache, torch.Tensor) else type(k_cache).__name__
        raise NotImplementedError(f"{who}: k_cache of dtype {dt} is not supported (torch.uint8 or torch.float8_e4m3fn bytes expected)")
    if not k_cache.is_cuda or k_cache.device != device:
        raise RuntimeError(f"{who}: k_cache must be a GPU (HIP device) tensor on the other tensors' device; there is no CPU path")
    if k_cache.dim() != 4 or k_cache.shape[2] != 1 or k_cache.shape[3] < INDEXER_TOKEN_BYTES or k_cache.shape[0] == 0:
        raise RuntimeError(f"{who}: k_cache must be (num_blocks, page_block_size, 1, W >= {INDEXER_TOKEN_BYTES}), got {tuple(k_cache.shape)}")
    nblk, ps = k_cache.shape[:2]
    if ps < 16 or ps % 16 != 0:
        raise RuntimeError(f"{who}: page_block_size (k_cache.shape[1]) must be a positive multiple of 16, got {ps}")
    tsb = k_cache.stride(1)
    psb = k_cache.stride(0) if nblk > 1 else max(k_cache.stride(0), ((ps - 1) * tsb + INDEXER_TOKEN_BYTES + 15) // 16 * 16)
    if k_cache.stride(3) != 1 or tsb < INDEXER_TOKEN_BYTES or tsb % 16 or psb % 16 or psb < (ps - 1) * tsb + INDEXER_TOKEN_BYTES or \
            k_cache.data_ptr() % 16:
        raise ValueError(f"{who}: k_cache must have contiguous 132-byte tokens at a stride that is a multiple of 16, pages that do not "
                         f"overlap at a stride that is a multiple of 16, and a 16-byte aligned address (got strides "
                         f"{tuple(k_cache.stride())}); it is never copied")
    return psb, tsb, nblk, ps


def _idx_lens(who, cache_seqlens, b, device):
    if isinstance(cache_seqlens, numbers.Integral):
        return
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32:
        dt = cache_seqlens.dtype if isinstance(cache_seqlens, torch.Tensor) else type(cache_seqlens).__name__
        raise NotImplementedError(f"{who}: cache_seqlens of dtype {dt} is not supported (int32 tensor or int expected)")
    if cache_seqlens.device != device or cache_seqlens.shape != (b,):
        raise RuntimeError(f"{who}: cache_seqlens must be an int32 ({b},) tensor on the other tensors' device, or an int")


def _idx_out(who, name, out, shape, dtype, device):
    """a caller's output: the right shape, dtype and device, last dim contiguous; its (batch, row) strides"""
    if not isinstance(out, torch.Tensor) or out.dtype != dtype:
        dt = out.dtype if isinstance(out, torch.Tensor) else type(out).__name__
        raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported ({dtype} expected)")
    if out.device != device or tuple(out.shape) != tuple(shape):
        raise RuntimeError(f"{who}: {name} must be a {tuple(shape)} tensor on {device}, got {tuple(out.shape)} on {out.device}")
    b, n, w = shape
    rs = out.stride(1) if n > 1 else max(out.stride(1), w)
    bs = out.stride(0) if b > 1 else max(out.stride(0), (n - 1) * rs + w)
    if (w > 1 and out.stride(2) != 1) or rs < w or bs < (n - 1) * rs + w:
        raise ValueError(f"{who}: {name} must have a contiguous last dim and rows that do not overlap (got strides {tuple(out.stride())}); "
                         f"it is never copied")
    return bs, rs


def ex_indexer_pack(k_new, k_cache, cache_seqlens, block_table, scale_pow2=False):
    """Quantise and append new index keys to an fp8 index-key pool, in place (fa_indexer_pack): k_new (B, N_new, 128) bfloat16 on the
    GPU goes to positions cache_seqlens[b] .. + N_new of sequence b (int32 (B,) lengths before the append, or an int) through
    block_table; a token whose position or page falls outside the table or the pool is dropped.  Returns None."""
    who = "ex_indexer_pack"
    if not isinstance(k_new, torch.Tensor) or not k_new.is_cuda:
        raise RuntimeError(f"{who}: k_new must be a GPU (HIP device) tensor; there is no CPU path")
    if k_new.dtype != torch.bfloat16:
        raise NotImplementedError(f"{who}: k_new of dtype {k_new.dtype} is not supported (torch.bfloat16 expected)")
    if k_new.dim() != 3:
        raise RuntimeError(f"{who}: k_new must be (B, N_new, 128), got {tuple(k_new.shape)}")
    if k_new.shape[2] != INDEXER_DIM:
        raise NotImplementedError(f"{who}: k_new of width {k_new.shape[2]} is not supported (128 expected)")
    b, nnew = k_new.shape[:2]
    dev = k_new.device
    psb, tsb, nblk, ps = _idx_pool(who, k_cache, dev)
    _f8_table(who, block_table, cache_seqlens, b, dev, True)
    k_new, kb, kt, _h = _f8_rows(who, "k_new", k_new.unsqueeze(2), 1, INDEXER_DIM)
    with torch.cuda.device(dev):
        cache_seqlens, block_table, trs, mb = _f8_table_args(block_table, cache_seqlens, b, dev)
        _call("fa_indexer_pack", (
            k_new.data_ptr(), k_cache.data_ptr(), cache_seqlens.data_ptr(), block_table.data_ptr(), b, nnew, INDEXER_DIM, kb, kt, psb, tsb,
            trs, nblk, ps, mb, int(bool(scale_pow2)), _stream_ptr(dev)))


def _idx_q(who, q, weights):
    """q as bytes with its (batch, token, head) byte strides, weights with its (batch, token) strides; what the call cannot
    address is copied (both are only read)"""
    if not isinstance(q, torch.Tensor) or not q.is_cuda:
        raise RuntimeError(f"{who}: q must be a GPU (HIP device) tensor; there is no CPU path")
    if q.dtype not in (torch.float8_e4m3fn, torch.uint8):
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (torch.float8_e4m3fn, or its bytes as torch.uint8, expected: "
                                  f"the caller quantises q)")
    if q.dim() != 4:
        raise RuntimeError(f"{who}: q must be 4-D (B, Nq, H_I, 128), got {tuple(q.shape)}")
    b, nq, h, d = q.shape
    if d != INDEXER_DIM:
        raise NotImplementedError(f"{who}: q of width {d} is not supported (128 expected)")
    if h not in (32, 64):
        raise NotImplementedError(f"{who}: q with {h} index heads is not supported (32 or 64 expected)")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
        dt = weights.dtype if isinstance(weights, torch.Tensor) else type(weights).__name__
        raise NotImplementedError(f"{who}: weights of dtype {dt} is not supported (torch.float32 expected)")
    if weights.device != q.device or tuple(weights.shape) != (b, nq, h):
        raise RuntimeError(f"{who}: weights must be a (B, Nq, H_I) = ({b}, {nq}, {h}) tensor on q's device, got {tuple(weights.shape)} on "
                           f"{weights.device}")

    def ok(t):
        hs = t.stride(2)
        tok = (h - 1) * hs + d
        ts = t.stride(1) if nq > 1 else max(t.stride(1), tok)
        bs = t.stride(0) if b > 1 else max(t.stride(0), (nq - 1) * ts + tok)
        good = t.stride(3) == 1 and hs >= d and ts >= tok and bs >= (nq - 1) * ts + tok and not (hs % 16 or ts % 16 or bs % 16 or t.data_ptr() % 16)
        return good, bs, ts, hs
    good, qb, qt, qh = ok(q)
    if not good:
        q = q.contiguous()
        good, qb, qt, qh = ok(q)
    if weights.stride(2) != 1 or (nq > 1 and weights.stride(1) < h) or (b > 1 and weights.stride(0) < (nq - 1) * weights.stride(1) + h):
        weights = weights.contiguous()
    wt = weights.stride(1) if nq > 1 else max(weights.stride(1), h)
    wb = weights.stride(0) if b > 1 else max(weights.stride(0), (nq - 1) * wt + h)
    return q, qb, qt, qh, weights, wb, wt


def ex_indexer_logits(q, weights, k_cache, cache_seqlens, block_table, causal=True, out=None, width=None):
    """The index logits (fa_indexer_logits): q (B, Nq, H_I, 128) e4m3, weights (B, Nq, H_I) float32, k_cache the index-key pool;
    returns float32 (B, Nq, width), width defaulting to max_blocks_per_seq * page_block_size.  Only visible entries are written: a
    fresh result is torch.empty elsewhere."""
    who = "ex_indexer_logits"
    q, qb, qt, qh, weights, wb, wt = _idx_q(who, q, weights)
    b, nq, h, d = q.shape
    dev = q.device
    psb, tsb, nblk, ps = _idx_pool(who, k_cache, dev)
    _f8_table(who, block_table, cache_seqlens, b, dev, True)
    width = block_table.shape[1] * ps if width is None else operator.index(width)
    if width < 1:
        raise RuntimeError(f"{who}: width must be >= 1, got {width}")
    with torch.cuda.device(dev):
        cache_seqlens, block_table, trs, mb = _f8_table_args(block_table, cache_seqlens, b, dev)
        if out is None:
            out = torch.empty((b, nq, width), dtype=torch.float32, device=dev)
        lb, lr = _idx_out(who, "out", out, (b, nq, width), torch.float32, dev)
        _call("fa_indexer_logits", (
            q.data_ptr(), weights.data_ptr(), k_cache.data_ptr(), cache_seqlens.data_ptr(), block_table.data_ptr(), out.data_ptr(),
            b, nq, h, d, width, qb, qt, qh, wb, wt, lb, lr, psb, tsb, trs, nblk, ps, mb, int(bool(causal)), _stream_ptr(dev)))
    return out


def ex_indexer_topk(logits, cache_seqlens, topk, seqlen_q=None, causal=True, out=None):
    """The selection (fa_indexer_topk): logits float32 (B, Nq, width); returns int32 (B, Nq, topk), per row the positions of the
    topk largest visible logits in ascending order, then -1."""
    who = "ex_indexer_topk"
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise RuntimeError(f"{who}: logits must be a GPU (HIP device) tensor; there is no CPU path")
    if logits.dtype != torch.float32:
        raise NotImplementedError(f"{who}: logits of dtype {logits.dtype} is not supported (torch.float32 expected)")
    if logits.dim() != 3 or logits.shape[2] < 1:
        raise RuntimeError(f"{who}: logits must be (B, Nq, width >= 1), got {tuple(logits.shape)}")
    b, nq, width = logits.shape
    if seqlen_q is not None and operator.index(seqlen_q) != nq:
        raise RuntimeError(f"{who}: seqlen_q = {seqlen_q} is not logits.shape[1] = {nq}")
    topk = operator.index(topk)
    if topk < 1 or topk > 1 << 20:
        raise RuntimeError(f"{who}: topk must lie in [1, 2^20], got {topk}")
    dev = logits.device
    _idx_lens(who, cache_seqlens, b, dev)
    lb, lr = _idx_out(who, "logits", logits, (b, nq, width), torch.float32, dev)
    with torch.cuda.device(dev):
        if not isinstance(cache_seqlens, torch.Tensor):
            cache_seqlens = torch.full((b,), operator.index(cache_seqlens), dtype=torch.int32, device=dev)
        cache_seqlens = cache_seqlens.contiguous()
        if out is None:
            out = torch.empty((b, nq, topk), dtype=torch.int32, device=dev)
        ib, it = _idx_out(who, "out", out, (b, nq, topk), torch.int32, dev)
        _call("fa_indexer_topk", (
            logits.data_ptr(), cache_seqlens.data_ptr(), out.data_ptr(), b, nq, width, topk, lb, lr, ib, it, int(bool(causal)),
            _stream_ptr(dev)))
    return out


def ex_lightning_indexer(q, weights, k_cache, cache_seqlens, block_table, topk, causal=True):
    """ex_indexer_topk(ex_indexer_logits(..)) with the logits in the shim's workspace: no allocation but the result's after the
    first call of a shape."""
    who = "ex_lightning_indexer"
    _idx_q(who, q, weights)                                   # (the refusals first: nothing has run yet)
    _idx_pool(who, k_cache, q.device)
    b, nq = q.shape[:2]
    _f8_table(who, block_table, cache_seqlens, b, q.device, True)
    width = block_table.shape[1] * k_cache.shape[1]
    if b * nq == 0:
        return ex_indexer_topk(ex_indexer_logits(q, weights, k_cache, cache_seqlens, block_table, causal), cache_seqlens, topk, None, causal)
    with torch.cuda.device(q.device):
        ws = _workspace(q.device, b * nq * width * 4)
    logits = ws[:b * nq * width * 4].view(torch.float32).view(b, nq, width)
    ex_indexer_logits(q, weights, k_cache, cache_seqlens, block_table, causal, logits, width)
    return ex_indexer_topk(logits, cache_seqlens, topk, nq, causal)


# ---- rotary embedding for training and prefill (include/fa_mi355x.h: fa_rotary_apply) ----

def _rotary_view(who, name, t, packed):
    """(batch stride, token stride) of a (B, S, heads, d) or packed (total, heads, d) view as fa_rotary_apply addresses it: last
    dim contiguous, heads adjacent at stride d, strides multiples of 8, 16-byte aligned.  Anything else raises: the tensor may be
    the target of the call, and a copy would silently lose the write."""
    heads, d = t.shape[-2], t.shape[-1]
    tokens = t.shape[-3]
    ts = t.stride(-3) if tokens > 1 else max(t.stride(-3), heads * d)
    bs = 0
    if not packed:
        bs = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), (tokens - 1) * ts + heads * d)
    if t.stride(-1) != 1 or (heads > 1 and t.stride(-2) != d) or ts < heads * d or ts % 8 or bs % 8 or t.data_ptr() % 16 or \
            (not packed and t.shape[0] > 1 and bs < (tokens - 1) * ts + heads * d):
        raise ValueError(f"{who}: {name} must have a contiguous last dim, its heads at stride d = {d}, token and batch strides that "
                         f"are multiples of 8 and do not overlap, and a 16-byte aligned address (got strides {tuple(t.stride())}); "
                         f"it is never copied")
    return bs, ts


def rotary_apply(x, cos, sin, out=None, interleaved=False, conjugate=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None):
    """Rotary position embedding of the first rotary_dim = 2 * cos.shape[1] head dims of every head of x, one launch
    (fa_rotary_apply).  x: (B, S, heads, d) float16 / bfloat16 on the GPU, or packed (total, heads, d) with cu_seqlens (int32
    (B + 1,) on x's device) and max_seqlen (an int, required); a strided view whose heads are adjacent (qkv[:, :, :2].reshape(B, S,
    2 * H, d) of a (B, S, 3, H, d) projection) is addressed as it is.  cos, sin: (seqlen_ro, rotary_dim / 2) in x's dtype on x's
    device, rotary_dim a multiple of 16 in [16, d].  out: None allocates a dense result; `out is x` (or a view of the same memory
    and strides) rotates in place, and the head dims at and past rotary_dim are then not touched; any other tensor of x's shape,
    dtype and device receives the result.  interleaved: pairs (2j, 2j + 1), else (j, j + rotary_dim / 2).  conjugate: rotate by
    -sin, the backward of the forward map.  seqlen_offsets: an int, or an int32 (B,) tensor on x's device that is read by the
    kernel only; token i of sequence b sits at seqlen_offsets[b] + i and is rotated iff that is a row of the tables, otherwise it
    passes through.  Nothing is read on the host, so the call can be captured and replayed with changed offsets and cu_seqlens.
    A layout the kernel cannot address raises ValueError; nothing is copied.  Returns out."""
    who = "rotary_apply"
    packed = cu_seqlens is not None
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{who}: x must be a GPU (HIP device) tensor; there is no CPU path")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"{who}: x must have a 16-bit dtype (float16 or bfloat16), got {x.dtype}")
    if max_seqlen is not None and not packed:
        raise ValueError(f"{who}: max_seqlen needs cu_seqlens")
    if packed:
        if x.dim() != 3:
            raise ValueError(f"{who}: with cu_seqlens x must be packed (total, heads, d), got {tuple(x.shape)}")
        if max_seqlen is None:
            raise ValueError(f"{who}: cu_seqlens needs max_seqlen")
        if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32:
            dt = cu_seqlens.dtype if isinstance(cu_seqlens, torch.Tensor) else type(cu_seqlens).__name__
            raise NotImplementedError(f"{who}: cu_seqlens of dtype {dt} is not supported (int32 tensor expected)")
        if cu_seqlens.device != x.device or cu_seqlens.dim() != 1 or cu_seqlens.shape[0] < 2:
            raise RuntimeError(f"{who}: cu_seqlens must be an int32 (B + 1,) tensor on x's device, B >= 1")
        total, heads, d = x.shape
        b, seqlen, mx = cu_seqlens.shape[0] - 1, 0, operator.index(max_seqlen)
        if mx < 0 or mx > total:
            raise ValueError(f"{who}: max_seqlen = {mx} must lie in [0, total = {total}]")
    else:
        if x.dim() != 4:
            raise RuntimeError(f"{who}: x must be 4-D (B, S, heads, d), or packed (total, heads, d) with cu_seqlens; got {tuple(x.shape)}")
        b, seqlen, heads, d = x.shape
        total = mx = 0
    if d % 8 != 0 or not 8 <= d <= 256:
        raise RuntimeError(f"{who}: head dim must be a multiple of 8 in [8, 256], got {d}")
    for name, t in (("cos", cos), ("sin", sin)):
        if not isinstance(t, torch.Tensor) or t.dtype != x.dtype or t.device != x.device or t.dim() != 2 or \
                t.shape != cos.shape or t.numel() == 0:
            raise RuntimeError(f"{who}: {name} must be a (seqlen_ro, rotary_dim / 2) tensor of x's dtype on x's device, cos and sin "
                               f"of one shape")
    rdim = 2 * cos.shape[1]
    if rdim % 16 != 0 or not 16 <= rdim <= d:
        raise RuntimeError(f"{who}: rotary_dim = 2 * cos.shape[1] must be a multiple of 16 in [16, d = {d}], got {rdim}")
    off0, offs = 0, None
    if isinstance(seqlen_offsets, torch.Tensor):
        if seqlen_offsets.dtype != torch.int32 or seqlen_offsets.device != x.device or seqlen_offsets.shape != (b,):
            raise RuntimeError(f"{who}: seqlen_offsets must be an int, or an int32 ({b},) tensor on x's device")
        offs = seqlen_offsets.contiguous()
    else:
        off0 = operator.index(seqlen_offsets)
        if abs(off0) >= 2 ** 31:
            raise ValueError(f"{who}: |seqlen_offsets| must be < 2^31, got {off0}")
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
        raise RuntimeError(f"{who}: out must be a tensor of x's shape, dtype and device")
    if b == 0 or heads == 0 or (total if packed else seqlen) == 0 or (packed and mx == 0):
        return out
    xb, xt = _rotary_view(who, "x", x, packed)
    yb, yt = _rotary_view(who, "out", out, packed)
    if out.data_ptr() == x.data_ptr() and (xb, xt) != (yb, yt):
        raise ValueError(f"{who}: out shares x's address with other strides; in place needs the same view")
    with torch.cuda.device(x.device):
        _tabs, rotary = _rotary_tables(cos, sin, rdim, interleaved)
        cu = cu_seqlens.contiguous() if packed else None
        _call("fa_rotary_apply", (x.data_ptr(), out.data_ptr(), b, seqlen, heads, d, _DTYPE_CODE[x.dtype], xb, xt, yb, yt, *rotary,
                                  int(bool(conjugate)), off0, _ptr(offs), _ptr(cu), total, mx, _stream_ptr(x.device)))
    return out


# ---- the fp8 quantiser (include/fa_mi355x.h: fa_fp8_quantize) ----

FP8_QUANT_LAYOUTS = ("bhnd", "bnhd", "thd")


def _fp8_quant_view(who, name, t, layout, unit):
    """(batch, heads, tokens, d, (batch, head, token) strides) of x or out under `layout`: (B, H, N, d), (B, N, H, d) or packed
    (total, H, d).  Strides in elements of t (out: bytes), each a multiple of `unit` (16 bytes), the start 16-byte aligned, the last
    dim contiguous; the stride of an extent-1 dim is handed on as 0.  ValueError for a view that would need a copy: it is never
    copied (out is the target of the call)."""
    want = 3 if layout == "thd" else 4
    if t.dim() != want:
        shape = {"bhnd": "(B, H, N, d)", "bnhd": "(B, N, H, d)", "thd": "(total, H, d) with cu_seqlens"}[layout]
        raise RuntimeError(f"{who}: {name} must be {want}-D {shape} under layout {layout!r}, got {tuple(t.shape)}")
    d = t.shape[-1]
    if layout == "thd":
        b, h, n, st = 1, t.shape[1], t.shape[0], (0, t.stride(1), t.stride(0))
    elif layout == "bhnd":
        b, h, n, st = t.shape[0], t.shape[1], t.shape[2], (t.stride(0), t.stride(1), t.stride(2))
    else:
        b, h, n, st = t.shape[0], t.shape[2], t.shape[1], (t.stride(0), t.stride(2), t.stride(1))
    st = tuple(s if e > 1 else 0 for s, e in zip(st, (b, h, n)))
    if t.numel() and (t.stride(-1) != 1 or t.data_ptr() % 16 != 0 or any(s % unit != 0 or s < 0 for s in st)):
        raise ValueError(f"{who}: {name} is a view the kernel cannot address: a contiguous last dim, a 16-byte aligned start and "
                         f"non-negative strides that are multiples of 16 bytes are needed (strides {tuple(t.stride())}); it is never copied")
    return b, h, n, d, st


def fp8_quantize(x, heads_per_scale=1, descale=None, layout="bnhd", out=None, out_layout=None, descale_out=None, scale_pow2=False,
                 cu_seqlens=None, max_seqlen=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, seqlen_offsets=0):
    """(x8, descale): a float16 / bfloat16 tensor as torch.float8_e4m3fn codes plus the float32 descales (B, H / heads_per_scale) the
    fp8 calls read (fa_fp8_quantize), on the shim's persistent workspace.  x: (B, N, H, d) under layout "bnhd", (B, H, N, d) under
    "bhnd", packed (total, H, d) under "thd" with cu_seqlens (int32 (B + 1,) on x's device) and max_seqlen; d a multiple of 16 in
    [16, 256]; any view with a contiguous last dim and strides that are multiples of 8 is addressed as it is (a slice of a fused qkv
    projection).  One descale covers heads_per_scale adjacent heads, all tokens of a sequence and all of d: H_q / H_kv for q, 1 for k
    and v.  descale None: amax / 448 per unit (scale_pow2: rounded up to a power of two), 1 for an all-zero or empty unit.  descale
    given (float32 (B, H / g) or (H / g,), read on the device only): the static mode, one launch; the returned descale is that
    tensor.  Codes: e4m3_rne(clamp(x / descale, +-448)) by the e4m3 cache append's arithmetic, so with the same descale the bytes
    are the cache's.  out: an e4m3 tensor in out_layout (default: layout) at its own strides (multiples of 16 bytes), e.g. the
    [:, :N] prefix of a (B, capacity, H, d) cache; None allocates a dense one.  descale_out: float32 (B, H / g) contiguous, or None.
    rotary_cos / rotary_sin (seqlen_ro, rotary_dim / 2) in x's dtype rotate the first rotary_dim head dims first, by rotary_apply's
    rules (rotary_interleaved, seqlen_offsets an int or int32 (B,)), with rotary_apply's bits.  Nothing is read on the host: the
    call can be captured and replayed.  NotImplementedError for dtypes and head dims, ValueError for views that would need a copy."""
    who = "fp8_quantize"
    if layout not in FP8_QUANT_LAYOUTS:
        raise ValueError(f"{who}: layout must be one of {FP8_QUANT_LAYOUTS}, got {layout!r}")
    out_layout = layout if out_layout is None else out_layout
    if out_layout not in FP8_QUANT_LAYOUTS or (out_layout == "thd") != (layout == "thd"):
        raise ValueError(f"{who}: out_layout must be one of {FP8_QUANT_LAYOUTS} and packed exactly when layout is, got {out_layout!r} "
                         f"for layout {layout!r}")
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float16, torch.bfloat16):
        dt = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
        raise NotImplementedError(f"{who}: x of dtype {dt} is not supported (torch.float16 or torch.bfloat16)")
    if x.dim() >= 1 and (x.shape[-1] % 16 != 0 or not 16 <= x.shape[-1] <= 256):
        raise NotImplementedError(f"{who}: head_dim {x.shape[-1]} is not supported (a multiple of 16 in [16, 256])")
    if not x.is_cuda:
        raise RuntimeError(f"{who}: x must be on the GPU (HIP device); there is no CPU path")
    packed = layout == "thd"
    if packed != (cu_seqlens is not None):
        raise ValueError(f"{who}: layout 'thd' and cu_seqlens go together")
    if max_seqlen is not None and not packed:
        raise ValueError(f"{who}: max_seqlen needs cu_seqlens")
    b, heads, n, d, sx = _fp8_quant_view(who, "x", x, layout, 8)
    total = mx = 0
    if packed:
        if max_seqlen is None:
            raise ValueError(f"{who}: cu_seqlens needs max_seqlen")
        if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32:
            dt = cu_seqlens.dtype if isinstance(cu_seqlens, torch.Tensor) else type(cu_seqlens).__name__
            raise NotImplementedError(f"{who}: cu_seqlens of dtype {dt} is not supported (int32 tensor expected)")
        if cu_seqlens.device != x.device or cu_seqlens.dim() != 1 or cu_seqlens.shape[0] < 2:
            raise RuntimeError(f"{who}: cu_seqlens must be an int32 (B + 1,) tensor on x's device, B >= 1")
        b, total, n, mx = cu_seqlens.shape[0] - 1, n, 0, operator.index(max_seqlen)
        if mx < 0 or mx > total:
            raise ValueError(f"{who}: max_seqlen = {mx} must lie in [0, total = {total}]")
    g = operator.index(heads_per_scale)
    if b < 1 or heads < 1:
        raise RuntimeError(f"{who}: x needs at least one batch element and one head, got {tuple(x.shape)}")
    if g < 1 or heads % g != 0:
        raise RuntimeError(f"{who}: heads_per_scale = {g} must be >= 1 and divide H = {heads}")
    nj = heads // g
    rdim = 0
    if (rotary_cos is None) != (rotary_sin is None):
        raise RuntimeError(f"{who}: rotary_cos and rotary_sin must both be given")
    off0, offs = 0, None
    if rotary_cos is not None:
        for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != x.dtype or t.device != x.device or t.dim() != 2 or \
                    t.shape != rotary_cos.shape or t.numel() == 0:
                raise RuntimeError(f"{who}: {name} must be a (seqlen_ro, rotary_dim / 2) tensor of x's dtype on x's device, cos and "
                                   f"sin of one shape")
        rdim = 2 * rotary_cos.shape[1]
        if rdim % 16 != 0 or not 16 <= rdim <= d:
            raise RuntimeError(f"{who}: rotary_dim = 2 * rotary_cos.shape[1] must be a multiple of 16 in [16, d = {d}], got {rdim}")
        if isinstance(seqlen_offsets, torch.Tensor):
            if seqlen_offsets.dtype != torch.int32 or seqlen_offsets.device != x.device or seqlen_offsets.shape != (b,):
                raise RuntimeError(f"{who}: seqlen_offsets must be an int, or an int32 ({b},) tensor on x's device")
            offs = seqlen_offsets.contiguous()
        else:
            off0 = operator.index(seqlen_offsets)
            if abs(off0) >= 2 ** 31:
                raise ValueError(f"{who}: |seqlen_offsets| must be < 2^31, got {off0}")
    dp, dbs, keep = _kv_descale(who, "descale", descale, x, b, nj)
    with torch.cuda.device(x.device):
        shape_out = (total, heads, d) if packed else (b, heads, n, d) if out_layout == "bhnd" else (b, n, heads, d)
        if out is None:
            out = torch.empty(shape_out, dtype=torch.float8_e4m3fn, device=x.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float8_e4m3fn:
            dt = out.dtype if isinstance(out, torch.Tensor) else type(out).__name__
            raise NotImplementedError(f"{who}: out of dtype {dt} is not supported (torch.float8_e4m3fn expected)")
        elif tuple(out.shape) != shape_out or out.device != x.device:
            raise RuntimeError(f"{who}: out must have shape {shape_out} under layout {out_layout!r} on x's device, got {tuple(out.shape)}")
        _b, _h, _n, _d, so = _fp8_quant_view(who, "out", out, out_layout, 16)
        if descale_out is not None:
            if not isinstance(descale_out, torch.Tensor) or descale_out.dtype != torch.float32 or descale_out.device != x.device or \
                    tuple(descale_out.shape) != (b, nj) or not descale_out.is_contiguous():
                raise RuntimeError(f"{who}: descale_out must be a contiguous float32 ({b}, {nj}) tensor on x's device")
        elif descale is None:
            descale_out = torch.empty((b, nj), dtype=torch.float32, device=x.device)
        _tabs, rotary = _rotary_tables(rotary_cos, rotary_sin, rdim, rotary_interleaved)
        cu = cu_seqlens.contiguous() if packed else None
        need = int(_lib.fa_fp8_quantize_workspace_bytes(b, heads, g))
        ws = _workspace(x.device, need)
        # a tensor without elements has no address: the call addresses nothing of it then, and any aligned pointer stands in
        _call("fa_fp8_quantize", (x.data_ptr() or ws.data_ptr(), out.data_ptr() or ws.data_ptr(), dp, _ptr(descale_out), _ptr(cu), *rotary, off0, _ptr(offs), b, heads, n,
                                  d, g, total, mx, _DTYPE_CODE[x.dtype], *sx, *so, dbs, int(bool(scale_pow2)), ws.data_ptr(), ws.numel(),
                                  _stream_ptr(x.device)))
    del keep
    return out, (descale if descale is not None else descale_out)


# ---- merge of two partial attention results (include/fa_mi355x.h: fa_merge_states / fa_merge_states_backward) ----

MERGE_LAYOUTS = ("bhnd", "bnhd", "thd")


def _merge_views(who, layout, o_likes, lse_likes):
    """The (batch, heads, rows, d) of a merge call and each tensor's (batch, head, row) stride triple, from the views themselves.
    o_likes / lse_likes: (name, tensor) pairs, the first of each the model for the others' shape, dtype and device.  layout:
    "bhnd" o (B, H, N, d) or (BH, N, d) with lse (B, H, N) or (BH, N); "bnhd" o (B, N, H, d) with lse (B, H, N); "thd" o (T, H, d)
    with lse (H, T).  RuntimeError on mismatched shapes, dtypes or devices, ValueError on a view the kernel cannot address."""
    if layout not in MERGE_LAYOUTS:
        raise ValueError(f"{who}: layout must be one of {MERGE_LAYOUTS}, got {layout!r}")
    o0, l0 = o_likes[0][1], lse_likes[0][1]
    for name, t in (*o_likes, *lse_likes):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a tensor on the GPU (HIP device); there is no CPU path")
        if t.device != o0.device:
            raise RuntimeError(f"{who}: all tensors must be on one device ({name} is on {t.device}, {o_likes[0][0]} on {o0.device})")
    if o0.dtype not in _DTYPE_CODE:
        raise RuntimeError(f"{who}: unsupported dtype {o0.dtype}")
    for name, t in o_likes:
        if t.shape != o0.shape or t.dtype != o0.dtype:
            raise RuntimeError(f"{who}: {name} must have the shape and dtype of {o_likes[0][0]} ({tuple(o0.shape)}, {o0.dtype}); got "
                               f"{tuple(t.shape)}, {t.dtype}")
    for name, t in lse_likes:
        if t.shape != l0.shape or t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32 of shape {tuple(l0.shape)}; got {tuple(t.shape)}, {t.dtype}")
    if layout == "bhnd" and o0.dim() == 3:
        want, dims = (o0.shape[0], o0.shape[1]), (1, o0.shape[0], o0.shape[1])
        o_tr = lambda t: (0, t.stride(0), t.stride(1))
        l_tr = lambda t: (0, t.stride(0), t.stride(1))
    elif layout == "bhnd" and o0.dim() == 4:
        b, h, n, d = o0.shape
        want, dims = (b, h, n), (b, h, n)
        o_tr = lambda t: (t.stride(0), t.stride(1), t.stride(2))
        l_tr = lambda t: (t.stride(0), t.stride(1), t.stride(2))
    elif layout == "bnhd" and o0.dim() == 4:
        b, n, h, d = o0.shape
        want, dims = (b, h, n), (b, h, n)
        o_tr = lambda t: (t.stride(0), t.stride(2), t.stride(1))
        l_tr = lambda t: (t.stride(0), t.stride(1), t.stride(2))
    elif layout == "thd" and o0.dim() == 3:
        n, h, d = o0.shape
        want, dims = (h, n), (1, h, n)
        o_tr = lambda t: (0, t.stride(1), t.stride(0))
        l_tr = lambda t: (0, t.stride(0), t.stride(1))
    else:
        raise RuntimeError(f"{who}: layout {layout!r} does not take {o_likes[0][0]} of shape {tuple(o0.shape)}")
    if tuple(l0.shape) != tuple(want):
        raise RuntimeError(f"{who}: with layout {layout!r} and {o_likes[0][0]} of shape {tuple(o0.shape)}, {lse_likes[0][0]} must be "
                           f"{tuple(want)}; got {tuple(l0.shape)}")
    d = o0.shape[-1]
    if d < 1 or d > 256 or (o0.dtype != torch.float32 and d % 8 != 0):
        raise RuntimeError(f"{who}: head_dim must lie in [1, 256], a multiple of 8 for 16-bit tensors (got {d})")
    strides = []
    for name, t in o_likes:
        if d > 1 and t.stride(-1) != 1:
            raise ValueError(f"{who}: {name} must have a contiguous last dim (a view that would need a copy)")
        tr = o_tr(t)
        if t.dtype != torch.float32 and t.numel() > 0 and (t.data_ptr() % 16 != 0 or any(x % 8 != 0 for x, n_ in zip(tr, dims) if n_ > 1)):
            raise ValueError(f"{who}: {name} is a view the kernel cannot address: 16-bit tensors need a 16-byte aligned start and "
                             f"strides that are multiples of 8 elements (strides {tr})")
        strides.append(tr)
    for name, t in lse_likes:
        strides.append(l_tr(t))
    for tr in strides:
        if any(x < 0 for x in tr):
            raise ValueError(f"{who}: negative strides cannot be addressed")
    # (a stride of an extent-1 dim is not used: hand 0 on, so that the C layer's alignment rule sees only the strides that address)
    strides = [tuple(x if n_ > 1 else 0 for x, n_ in zip(tr, dims)) for tr in strides]
    return dims, d, _DTYPE_CODE[o0.dtype], strides


def merge_states(o_a, lse_a, o_b, lse_b, layout="bhnd", out=None):
    """(o, lse) of attention over the union of two disjoint key sets from the two partial results (fa_merge_states):
    lse = logaddexp(lse_a, lse_b), o = exp(lse_a - lse) o_a + exp(lse_b - lse) o_b.  Strides come from the views; nothing is
    copied.  out = (o, lse) to write into given tensors, which may be (o_a, lse_a) themselves (in place).  Nothing is recorded by
    autograd."""
    who = "merge_states"
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError(f"{who}: out must be a pair (o, lse) of tensors")
        o, lse = out
    _merge_views(who, layout, (("o_a", o_a), ("o_b", o_b)), (("lse_a", lse_a), ("lse_b", lse_b)))
    with torch.cuda.device(o_a.device):
        if out is None:
            o = torch.empty(o_a.shape, dtype=o_a.dtype, device=o_a.device)
            lse = torch.empty(lse_a.shape, dtype=torch.float32, device=o_a.device)
        dims, d, code, st = _merge_views(who, layout, (("o_a", o_a), ("o_b", o_b), ("o", o)), (("lse_a", lse_a), ("lse_b", lse_b), ("lse", lse)))
        s_oa, s_ob, s_o, s_la, s_lb, s_l = st
        _call("fa_merge_states", (o_a.data_ptr(), lse_a.data_ptr(), o_b.data_ptr(), lse_b.data_ptr(), o.data_ptr(), lse.data_ptr(), *dims, d,
                                  code, *s_oa, *s_la, *s_ob, *s_lb, *s_o, *s_l, _stream_ptr(o_a.device)))
    return o, lse


def merge_states_backward(o_a, lse_a, o_b, lse_b, do_, dlse=None, layout="bhnd"):
    """(do_a, do_b, dlse_a, dlse_b) of merge_states from the gradients of its o and lse (dlse None: zero), one launch
    (fa_merge_states_backward).  The results are new contiguous tensors of the inputs' shapes."""
    who = "merge_states_backward"
    o_likes = [("o_a", o_a), ("o_b", o_b), ("do", do_)]
    lse_likes = [("lse_a", lse_a), ("lse_b", lse_b)] + ([("dlse", dlse)] if dlse is not None else [])
    _merge_views(who, layout, o_likes, lse_likes)
    with torch.cuda.device(o_a.device):
        do_a, do_b = (torch.empty(o_a.shape, dtype=o_a.dtype, device=o_a.device) for _ in range(2))
        dlse_a, dlse_b = (torch.empty(lse_a.shape, dtype=torch.float32, device=o_a.device) for _ in range(2))
        dims, d, code, st = _merge_views(who, layout, o_likes + [("do_a", do_a), ("do_b", do_b)],
                                         lse_likes + [("dlse_a", dlse_a), ("dlse_b", dlse_b)])
        s_oa, s_ob, s_do, s_doa, s_dob = st[:5]
        s_la, s_lb = st[5:7]
        s_dl = st[7] if dlse is not None else (0, 0, 0)
        s_dla, s_dlb = st[-2:]
        _call("fa_merge_states_backward", (
            o_a.data_ptr(), lse_a.data_ptr(), o_b.data_ptr(), lse_b.data_ptr(), do_.data_ptr(), _ptr(dlse), do_a.data_ptr(),
            do_b.data_ptr(), dlse_a.data_ptr(), dlse_b.data_ptr(), *dims, d, code, *s_oa, *s_la, *s_ob, *s_lb, *s_do, *s_dl, *s_doa,
            *s_dob, *s_dla, *s_dlb, _stream_ptr(o_a.device)))
    return do_a, do_b, dlse_a, dlse_b



# ---- e4m3 q, k, v with per-head descales (include/fa_mi355x.h: fa_fp8_forward) ----

FP8_LAYOUTS = ("bhnd", "bnhd")


FP8_HEAD_DIMS = (64, 128, 256)   # of the _hdim entry points (hdim=True below); every other call: 128


def _fp8_head_dim(who, hdim, **tensors):
    """The head dim of an fp8 call: 128 (the callers' own checks refuse the rest), or with hdim the one last extent of all
    `tensors`, 64, 128 or 256: RuntimeError names tensors that disagree, NotImplementedError any other width."""
    if not hdim:
        return 128
    dims = {name: t.shape[-1] for name, t in tensors.items() if t.dim() >= 1}
    if len(set(dims.values())) > 1:
        raise RuntimeError(f"{who}: mixed head dims: " + ", ".join(f"{name} has {d}" for name, d in dims.items()) +
                           " (q, k and v must agree in their last extent)")
    d = next(iter(dims.values()), 128)
    if d not in FP8_HEAD_DIMS:
        raise NotImplementedError(f"{who}: head_dim {d} is not supported (64, 128 or 256)")
    return d


def _fp8_view(who, name, t, layout, d=128):
    """(batch, heads, rows, (batch, head, token) strides in elements) of a 4-D (.., d) tensor under `layout`; a stride of an extent-1
    dim is handed on as 0 (token: d), so that the C layer's rules see only the strides that address"""
    if t.dim() != 4 or t.shape[3] != d:
        if t.dim() == 4:
            raise NotImplementedError(f"{who}: head_dim {t.shape[3]} is not supported (128 only); got {name} of shape {tuple(t.shape)}")
        raise RuntimeError(f"{who}: {name} must be 4-D ({f'B, H, N, {d}' if layout == 'bhnd' else f'B, N, H, {d}'}), got {tuple(t.shape)}")
    if t.stride(3) != 1:
        raise ValueError(f"{who}: {name} must have a contiguous last dim (a view that would need a copy)")
    b, h, n = (t.shape[0], t.shape[1], t.shape[2]) if layout == "bhnd" else (t.shape[0], t.shape[2], t.shape[1])
    hs, ts = (t.stride(1), t.stride(2)) if layout == "bhnd" else (t.stride(2), t.stride(1))
    st = (t.stride(0) if b > 1 else 0, hs if h > 1 else 0, ts if n > 1 else d)
    unit = 16 // t.element_size()
    if t.numel() and (t.data_ptr() % 16 != 0 or any(x % unit != 0 or x < 0 for x in st)):
        raise ValueError(f"{who}: {name} is a view the kernel cannot address: a 16-byte aligned start and non-negative strides that are "
                         f"multiples of 16 bytes are needed (strides {st})")
    return b, h, n, st


def _fp8_mod(who, q, hq, window, softcap, sinks, hdim=False):
    """(the entry point's suffix, its trailing (window_left, window_right, softcap, sinks, sink_heads), the tensor to keep alive) of
    a window, a softcap and sinks on an fp8 call with hq query heads; ("", (), None) when none of the three is given: such a call
    goes through its parent entry point with the parent's arguments.  hdim: the suffix is "_hdim" and the trailing group is always
    there (the _hdim entry points take it; at its defaults it is no feature)"""
    try:
        wl, wr = window
        if isinstance(wl, bool) or isinstance(wr, bool):
            raise TypeError
        wl, wr = operator.index(wl), operator.index(wr)
    except (TypeError, ValueError):
        raise RuntimeError(f"{who}: window must be a pair (left, right) of ints, got {window!r}") from None
    if wl < -1 or wr < -1:
        raise RuntimeError(f"{who}: window ({wl}, {wr}): each bound must be >= 0, or -1 for unbounded")
    cap = float(softcap)
    if not (math.isfinite(cap) and cap >= 0.0):
        raise RuntimeError(f"{who}: softcap must be a finite number >= 0 (got {cap})")
    if sinks is not None:
        if not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32:
            dt = sinks.dtype if isinstance(sinks, torch.Tensor) else type(sinks).__name__
            raise RuntimeError(f"{who}: sinks of dtype {dt} is not supported (a float32 tensor expected; pass a 16-bit parameter as p.float())")
        if tuple(sinks.shape) != (hq,):
            raise RuntimeError(f"{who}: sinks must be (H_q,) = ({hq},), one per query head, got {tuple(sinks.shape)}")
        if sinks.device != q.device:
            raise RuntimeError(f"{who}: sinks must be on q's device ({q.device}), got {sinks.device}")
        sinks = sinks.contiguous()
    featured = wl >= 0 or wr >= 0 or cap > 0.0 or sinks is not None
    if hdim:
        return "_hdim", (wl, wr, cap, _ptr(sinks), hq if sinks is not None else 0), sinks
    return ("_mod", (wl, wr, cap, _ptr(sinks), hq if sinks is not None else 0), sinks) if featured else ("", (), None)


def fp8_forward(q, k, v, causal, softmax_scale, q_descale=None, k_descale=None, v_descale=None, out_dtype=torch.bfloat16, layout="bhnd",
                *, window=(-1, -1), softcap=0.0, sinks=None, hdim=False):
    """(o, lse) of FlashAttention-3's fp8 call (fa_fp8_forward): q (B, H_q, Nq, 128), k and v (B, H_kv, Nk, 128) in torch.float8_e4m3fn
    (layout "bnhd": (B, N, H, 128)), used at their own strides, never copied; q_descale, k_descale, v_descale float32 (B, H_kv) or
    (H_kv,) on q's device, None = 1.  o comes back contiguous in `layout` and out_dtype (bfloat16 / float16), lse float32
    (B, H_q, Nq).  The V^T workspace is the shim's persistent one.  Nothing is recorded by autograd.
    window (left, right; -1 = unbounded), softcap (0 = off) and sinks (float32 (H_q,) on q's device) are fa_fp8_forward_mod's; a call
    with none of them goes through fa_fp8_forward.  hdim=True: the call goes through fa_fp8_forward_hdim, whatever its other arguments,
    and the last extent of q, k, v may be 64, 128 or 256 (softmax_scale None: d ** -0.5); at 128 that entry point is fa_fp8_forward_mod."""
    who = "fp8_forward"
    if layout not in FP8_LAYOUTS:
        raise ValueError(f"{who}: layout must be one of {FP8_LAYOUTS}, got {layout!r}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float8_e4m3fn:
            dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (torch.float8_e4m3fn expected; 16-bit tensors go to "
                                      f"fa3_forward(fp8=1) or flash_attention_ex)")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
        if t.device != q.device:
            raise RuntimeError(f"{who}: q, k, v must be on one device ({name} is on {t.device}, q on {q.device})")
    d = _fp8_head_dim(who, hdim, q=q, k=k, v=v)
    b, hq, nq, sq = _fp8_view(who, "q", q, layout, d)
    bk, hkv, nk, sk = _fp8_view(who, "k", k, layout, d)
    bv, hv, nv, sv = _fp8_view(who, "v", v, layout, d)
    if (bk, bv) != (b, b) or (hv, nv) != (hkv, nk):
        raise RuntimeError(f"{who}: k and v must share (B, H_kv, Nk) and q's batch; got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    if min(b, hq, hkv, nq, nk) < 1:
        raise RuntimeError(f"{who}: empty tensors are not supported (q {tuple(q.shape)}, k {tuple(k.shape)})")
    if hq % hkv != 0:
        raise RuntimeError(f"{who}: H_q = {hq} must be a multiple of H_kv = {hkv}")
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise RuntimeError(f"{who}: softmax_scale must be finite and > 0 (got {scale})")
    qdp, qds, keep_q = _kv_descale(who, "q_descale", q_descale, q, b, hkv)
    kdp, kds, keep_k = _kv_descale(who, "k_descale", k_descale, q, b, hkv)
    vdp, vds, keep_v = _kv_descale(who, "v_descale", v_descale, q, b, hkv)
    mod, tail, keep_s = _fp8_mod(who, q, hq, window, softcap, sinks, hdim)
    with torch.cuda.device(q.device):
        o = torch.empty((b, hq, nq, d) if layout == "bhnd" else (b, nq, hq, d), dtype=out_dtype, device=q.device)
        lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
        _b, _h, _n, so = _fp8_view(who, "o", o, layout, d)
        need = int((_lib.fa_fp8_forward_hdim_workspace_bytes if hdim else _lib.fa_fp8_forward_workspace_bytes)(b, hkv, nk, d))
        ws = _workspace(q.device, need)
        _call("fa_fp8_forward" + mod, (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), qdp, kdp, vdp, b, hq, hkv, nq,
                                       nk, d, _DTYPE_CODE[out_dtype], *sq, *sk, *sv, *so, qds, kds, vds, int(bool(causal)), scale,
                                       ws.data_ptr(), ws.numel(), _stream_ptr(q.device), *tail))
    del keep_q, keep_k, keep_v, keep_s
    return o, lse


def _fp8_rows(who, name, t, heads, d=128):
    """(token stride, head stride) in bytes of an e4m3 (.., heads, d) tensor's last three dims; ValueError on a view the kernels
    cannot address without a copy"""
    if t.stride(-1) != 1:
        raise ValueError(f"{who}: {name} must have a contiguous last dim (a view that would need a copy)")
    n = t.shape[-3]
    ts = t.stride(-3) if n > 1 else max(t.stride(-3), d)
    hs = t.stride(-2) if heads > 1 else 0
    if t.numel() and (t.data_ptr() % 16 != 0 or ts % 16 != 0 or hs % 16 != 0 or ts < d or hs < 0):
        raise ValueError(f"{who}: {name} is a view the kernel cannot address: a 16-byte aligned start and non-negative strides that are "
                         f"multiples of 16 bytes are needed (token stride {ts}, head stride {hs})")
    return ts, hs


def fp8_varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, q_descale=None,
                       k_descale=None, v_descale=None, out_dtype=torch.bfloat16, block_table=None, *, window=(-1, -1), softcap=0.0,
                       sinks=None, hdim=False):
    """(o, lse) of the packed / paged fp8 call (fa_fp8_forward_varlen): q (total_q, H_q, 128) in torch.float8_e4m3fn at its own token
    and head strides; k and v (total_k, H_kv, 128) e4m3, or with block_table (int32 (B, max_blocks_per_seq)) the pools
    (num_blocks, ps, H_kv, 128) at their own page and token strides; nothing is copied.  cu_seqlens_* int32 (B + 1,) on the device;
    descales float32 (B, H_kv) or (H_kv,), None = 1.  o (total_q, H_q, 128) in out_dtype, lse float32 (H_q, total_q); rows no
    sequence owns hold unspecified values.  Nothing is read on the host; the V^T workspace is the shim's persistent one.
    window, softcap and sinks (float32 (H_q,)) are fa_fp8_forward_varlen_mod's; a call with none of them goes through
    fa_fp8_forward_varlen.  hdim=True: through fa_fp8_forward_varlen_hdim, with a last extent of 64, 128 or 256 (fp8_forward has the rest)."""
    who = "fp8_varlen_forward"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float8_e4m3fn:
            dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (torch.float8_e4m3fn expected; 16-bit tensors go to "
                                      f"flash_attention_varlen)")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    paged = block_table is not None
    if paged and not (isinstance(block_table, torch.Tensor) and block_table.dtype == torch.int32):
        dt = block_table.dtype if isinstance(block_table, torch.Tensor) else type(block_table).__name__
        raise NotImplementedError(f"{who}: block_table of dtype {dt} is not supported (int32 tensor expected)")
    kdim = 4 if paged else 3
    if q.dim() != 3 or k.dim() != kdim or v.shape != k.shape:
        raise RuntimeError(f"{who}: q must be (total_q, H_q, 128) and k, v " +
                           ("pools (num_blocks, page_block_size, H_kv, 128)" if paged else "(total_k, H_kv, 128)") +
                           f"; got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    d = _fp8_head_dim(who, hdim, q=q, k=k, v=v)
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.shape[-1] != d:
            raise NotImplementedError(f"{who}: head_dim {t.shape[-1]} is not supported (128 only); got {name} of shape {tuple(t.shape)}")
    tensors = (q, k, v, cu_seqlens_q, cu_seqlens_k) + ((block_table,) if paged else ())
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f"{who}: all tensors must be on one device")
    for name, c in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if c.dtype != torch.int32 or c.dim() != 1 or c.shape[0] < 2:
            raise RuntimeError(f"{who}: {name} must be a 1-D int32 tensor of batch + 1 >= 2 offsets")
    if cu_seqlens_q.shape != cu_seqlens_k.shape:
        raise RuntimeError(f"{who}: cu_seqlens_q and cu_seqlens_k must have the same length (batch + 1)")
    b = cu_seqlens_q.shape[0] - 1
    total_q, hq = q.shape[0], q.shape[1]
    hkv = k.shape[-2]
    if hkv == 0 or hq == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: H_q = {hq} must be a multiple of H_kv = {hkv}")
    mq, mk = operator.index(max_seqlen_q), operator.index(max_seqlen_k)
    if mq < 0 or mk < 0:
        raise RuntimeError(f"{who}: max_seqlen_q, max_seqlen_k must be >= 0")
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise RuntimeError(f"{who}: softmax_scale must be finite and > 0 (got {scale})")
    qts, qhs = _fp8_rows(who, "q", q, hq, d)
    kts, khs = _fp8_rows(who, "k", k, hkv, d)
    vts, vhs = _fp8_rows(who, "v", v, hkv, d)
    if paged:
        nblk, ps = k.shape[0], k.shape[1]
        if ps < 16 or ps % 16 != 0:
            raise RuntimeError(f"{who}: page_block_size must be a positive multiple of 16, got {ps}")
        if block_table.dim() != 2 or block_table.shape[0] != b:
            raise RuntimeError(f"{who}: block_table must be an int32 (batch, max_blocks_per_seq) tensor, batch = {b}; got "
                               f"{tuple(block_table.shape)}")
        if nblk < 1:
            raise RuntimeError(f"{who}: the pools must hold at least one page")
        block_table = block_table.contiguous()
        mblk = block_table.shape[1]
        kps, vps = (t.stride(0) if nblk > 1 else max(t.stride(0), 0) for t in (k, v))
        if kps % 16 != 0 or vps % 16 != 0 or kps < 0 or vps < 0:
            raise ValueError(f"{who}: the page strides of k, v ({kps}, {vps}) must be non-negative multiples of 16 bytes")
        total_k, pages = 0, (mblk, nblk, ps, kps, vps)
    else:
        total_k, mblk, ps, pages = k.shape[0], 0, 0, (0, 0, 0, 0, 0)
    cu_q, cu_k = cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous()
    qdp, qds, keep_q = _kv_descale(who, "q_descale", q_descale, q, b, hkv)
    kdp, kds, keep_k = _kv_descale(who, "k_descale", k_descale, q, b, hkv)
    vdp, vds, keep_v = _kv_descale(who, "v_descale", v_descale, q, b, hkv)
    mod, tail, keep_s = _fp8_mod(who, q, hq, window, softcap, sinks, hdim)
    with torch.cuda.device(q.device):
        o = torch.empty((total_q, hq, d), dtype=out_dtype, device=q.device)
        lse = torch.empty((hq, total_q), dtype=torch.float32, device=q.device)
        if total_q == 0:
            return o, lse
        need = int((_lib.fa_fp8_forward_varlen_hdim_workspace_bytes if hdim else _lib.fa_fp8_forward_varlen_workspace_bytes)(
            b, hkv, total_k, mk, mblk, ps, d))
        ws = _workspace(q.device, need)
        _call("fa_fp8_forward_varlen" + mod, (
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), qdp, kdp, vdp, cu_q.data_ptr(), cu_k.data_ptr(),
            block_table.data_ptr() if paged else 0, b, hq, hkv, total_q, total_k, mq, mk, d, _DTYPE_CODE[out_dtype], qts, qhs, kts, khs,
            vts, vhs, *pages, qds, kds, vds, int(bool(causal)), scale, ws.data_ptr(), ws.numel(), _stream_ptr(q.device), *tail))
    del keep_q, keep_k, keep_v, keep_s
    return o, lse


def fp8_kvcache_forward(q, k_cache, v_cache, cache_seqlens=None, block_table=None, cache_batch_idx=None, q_descale=None, k_descale=None,
                        v_descale=None, softmax_scale=None, causal=False, num_splits=0, out_dtype=torch.bfloat16, *, window=(-1, -1),
                        softcap=0.0, sinks=None, hdim=False, cu_seqlens_q=None, max_seqlen_q=None):
    """(o, lse) of fp8 KV-cache decoding (fa_fp8_forward_kvcache): q (B, Nq, H_q, 128) in torch.float8_e4m3fn at its own batch and
    token strides over the e4m3 caches (B_cache, cache_len, H_kv, 128), or with block_table (int32 (B, max_blocks_per_seq)) the pools
    (num_blocks, ps, H_kv, 128), at their own batch / page and token strides; nothing is copied.  cache_seqlens int32 (B,) on the
    device, an int, or None (full); cache_batch_idx int32 (B,), contiguous form only; descales float32 (B, H_kv) or (H_kv,), None =
    1.  o (B, Nq, H_q, 128) in out_dtype, lse float32 (B, H_q, Nq).  Nothing is read on the host; the partials live in the shim's
    persistent workspace.  window, softcap and sinks (float32 (H_q,)) are fa_fp8_forward_kvcache_mod's; a call with none of them goes
    through fa_fp8_forward_kvcache.  hdim=True: through fa_fp8_forward_kvcache_hdim, with a last extent of 64, 128 or 256 (fp8_forward
    has the rest).  cu_seqlens_q (int32 (B + 1,) on the device, never read on the host) with max_seqlen_q (an int): packed queries
    through fa_fp8_forward_kvcache_varlen under the hdim rules; q is (total_q, H_q, d), o likewise and lse (H_q, total_q)."""
    who = "fp8_kvcache_forward"
    if cu_seqlens_q is not None or max_seqlen_q is not None:
        return _fp8_kvcache_packed(who, q, k_cache, v_cache, None, None, cache_seqlens, block_table, cache_batch_idx, q_descale, k_descale,
                                   v_descale, softmax_scale, causal, num_splits, out_dtype, window, softcap, sinks, cu_seqlens_q,
                                   max_seqlen_q, None, None, None, False, None)
    if isinstance(q, torch.Tensor) and q.dtype in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (torch.float8_e4m3fn expected; a 16-bit q over an e4m3 "
                                  f"cache is flash_attn_with_kvcache(..., k_descale=, v_descale=))")
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float8_e4m3fn:
            dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (torch.float8_e4m3fn expected)")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    paged = block_table is not None
    if paged and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    for name, t in (("block_table", block_table), ("cache_batch_idx", cache_batch_idx)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32):
            dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (int32 tensor expected)")
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise RuntimeError(f"{who}: q must be (B, Nq, H_q, 128) and k_cache, v_cache " +
                           ("pools (num_blocks, page_block_size, H_kv, 128)" if paged else "(B_cache, cache_len, H_kv, 128)") +
                           f" of one shape; got {tuple(q.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    d = _fp8_head_dim(who, hdim, q=q, k_cache=k_cache, v_cache=v_cache)
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if t.shape[-1] != d:
            raise NotImplementedError(f"{who}: head_dim {t.shape[-1]} is not supported (128 only); got {name} of shape {tuple(t.shape)}")
    b, nq, hq = q.shape[0], q.shape[1], q.shape[2]
    hkv = k_cache.shape[2]
    if hkv == 0 or hq == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: H_q = {hq} must be a multiple of H_kv = {hkv}")
    if isinstance(cache_seqlens, int) and not isinstance(cache_seqlens, bool):
        cache_seqlens = torch.full((b,), cache_seqlens, dtype=torch.int32, device=q.device)
    if cache_seqlens is not None and not (isinstance(cache_seqlens, torch.Tensor) and cache_seqlens.dtype == torch.int32 and
                                          cache_seqlens.shape == (b,)):
        raise RuntimeError(f"{who}: cache_seqlens must be an int32 tensor of shape (B,) = ({b},), an int or None")
    tensors = [t for t in (q, k_cache, v_cache, cache_seqlens, block_table, cache_batch_idx) if t is not None]
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f"{who}: all tensors must be on one device")
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise RuntimeError(f"{who}: softmax_scale must be finite and > 0 (got {scale})")
    ns = operator.index(num_splits)
    if ns < 0 or ns > 256:
        raise RuntimeError(f"{who}: num_splits must lie in [0, 256] (got {ns})")
    for name, t, heads in (("q", q, hq), ("k_cache", k_cache, hkv), ("v_cache", v_cache, hkv)):
        if t.numel() and ((heads > 1 and t.stride(2) != d) or t.stride(3) != 1):
            raise ValueError(f"{who}: {name} must have adjacent heads with a contiguous last dim (strides {t.stride()})")
        if t.numel() and (t.data_ptr() % 16 != 0 or t.stride(0) % 16 != 0 or t.stride(1) % 16 != 0 or t.stride(0) < 0 or
                          (t.shape[1] > 1 and t.stride(1) < heads * d)):
            raise ValueError(f"{who}: {name} is a view the kernel cannot address: a 16-byte aligned start, batch and token strides that "
                             f"are multiples of 16 bytes and rows that do not overlap are needed (strides {t.stride()})")
    tstride = lambda t, heads: t.stride(1) if t.shape[1] > 1 else heads * d   # noqa: E731
    if paged:
        nblk, ps = k_cache.shape[0], k_cache.shape[1]
        if ps < 16 or ps % 16 != 0:
            raise RuntimeError(f"{who}: page_block_size must be a positive multiple of 16, got {ps}")
        if block_table.dim() != 2 or block_table.shape[0] != b or block_table.shape[1] < 1:
            raise RuntimeError(f"{who}: block_table must be an int32 (B, max_blocks_per_seq >= 1) tensor, B = {b}; got "
                               f"{tuple(block_table.shape)}")
        if nblk < 1:
            raise RuntimeError(f"{who}: the pools must hold at least one page")
        if block_table.stride(1) != 1 and block_table.shape[1] > 1:
            block_table = block_table.contiguous()
        cap, cbatch = block_table.shape[1] * ps, 0
        pages = (max(block_table.stride(0), block_table.shape[1]), nblk, ps)
    else:
        cap = k_cache.shape[1]
        if cap < 1:
            raise RuntimeError(f"{who}: the caches must hold at least one token")
        if cache_batch_idx is not None:
            if cache_batch_idx.shape != (b,):
                raise RuntimeError(f"{who}: cache_batch_idx must be an int32 tensor of shape (B,) = ({b},)")
            cache_batch_idx = cache_batch_idx.contiguous()
            cbatch = k_cache.shape[0]
        elif k_cache.shape[0] != b:
            raise RuntimeError(f"{who}: the caches hold {k_cache.shape[0]} rows for a batch of {b} (pass cache_batch_idx to select rows)")
        else:
            cbatch = 0
        pages = (0, 0, 0)
    if cache_seqlens is not None:
        cache_seqlens = cache_seqlens.contiguous()
    qdp, qds, keep_q = _kv_descale(who, "q_descale", q_descale, q, b, hkv)
    kdp, kds, keep_k = _kv_descale(who, "k_descale", k_descale, q, b, hkv)
    vdp, vds, keep_v = _kv_descale(who, "v_descale", v_descale, q, b, hkv)
    mod, tail, keep_s = _fp8_mod(who, q, hq, window, softcap, sinks, hdim)
    with torch.cuda.device(q.device):
        o = torch.empty((b, nq, hq, d), dtype=out_dtype, device=q.device)
        lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
        if b == 0 or nq == 0:
            return o, lse
        if hdim:
            need = int(_lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(b, hq, hkv, nq, cap, d, ns, int(bool(causal)), tail[0], tail[1],
                                                                        int(sinks is not None)))
        elif mod:
            need = int(_lib.fa_fp8_forward_kvcache_workspace_bytes_mod(b, hq, hkv, nq, cap, 128, ns, int(bool(causal)), tail[0], tail[1],
                                                                       int(sinks is not None)))
        else:
            need = int(_lib.fa_fp8_forward_kvcache_workspace_bytes(b, hq, hkv, nq, cap, 128, ns))
        ws = _workspace(q.device, need)
        _call("fa_fp8_forward_kvcache" + mod, (
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), o.data_ptr(), lse.data_ptr(), qdp, kdp, vdp,
            cache_seqlens.data_ptr() if cache_seqlens is not None else 0, block_table.data_ptr() if paged else 0,
            cache_batch_idx.data_ptr() if cache_batch_idx is not None else 0, b, hq, hkv, nq, cap, cbatch, d, _DTYPE_CODE[out_dtype],
            _E4M3_CODE, _E4M3_CODE, max(q.stride(0), 0) if b > 1 else 0, tstride(q, hq),
            k_cache.stride(0) if k_cache.shape[0] > 1 else 0, tstride(k_cache, hkv),
            v_cache.stride(0) if v_cache.shape[0] > 1 else 0, tstride(v_cache, hkv), *pages, qds, kds, vds, int(bool(causal)), scale, ns,
            ws.data_ptr() if need else 0, ws.numel() if need else 0, _stream_ptr(q.device), *tail))
    del keep_q, keep_k, keep_v, keep_s
    return o, lse


def fp8_kvcache_step(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table=None, cache_batch_idx=None, q_descale=None,
                     k_descale=None, v_descale=None, softmax_scale=None, causal=False, num_splits=0, out_dtype=None, *, window=(-1, -1),
                     softcap=0.0, sinks=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q8_out=None, cu_seqlens_q=None,
                     max_seqlen_q=None, cu_seqlens_k_new=None, hdim=False):
    """(o, lse) of the fp8 decode step (fa_fp8_kvcache_step): the new tokens k_new, v_new (B, N_new, H_kv, 128) are appended to the
    e4m3 caches at cache_seqlens[b] (the lengths BEFORE the append: int32 (B,) on the device, or an int), q (B, Nq, H_q, 128) is
    rotated and quantised, and fp8_kvcache_forward's attention runs over the caches with the new tokens in them.  q, k_new, v_new are
    all float16, all bfloat16 (quantised with 1 / descale; k_new and q rotated when rotary_cos / rotary_sin, (seqlen_ro, rotary_dim / 2)
    in their dtype, are given) or all torch.float8_e4m3fn (copied and used as they are; no rotary, no q8_out).  q and the caches follow
    fp8_kvcache_forward's view rules (their own strides, never copied), the new tokens and the tables ex_kvcache_forward's (a dense
    copy where the kernel cannot address them).  q8_out: an e4m3 (B, Nq, H_q, 128) tensor that receives q's codes (16-bit mode),
    else they stay in the workspace.  out_dtype defaults to q's dtype, bfloat16 for an e4m3 q.  Nothing is read on the host.
    cu_seqlens_q with max_seqlen_q, cu_seqlens_k_new (int32 (B + 1,) device tensors, never read on the host) or hdim=True: through
    fa_fp8_kvcache_step_varlen, at a last extent of 64, 128 or 256; with cu_seqlens_q q is packed (total_q, H_q, d), o and q8_out
    likewise, lse (H_q, total_q); with cu_seqlens_k_new the new tokens are packed (total_k_new, H_kv, d).  Without any of the four the
    function is what it was."""
    who = "fp8_kvcache_step"
    if cu_seqlens_q is not None or max_seqlen_q is not None or cu_seqlens_k_new is not None or hdim:
        return _fp8_kvcache_packed(who, q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, cache_batch_idx, q_descale, k_descale,
                                   v_descale, softmax_scale, causal, num_splits, out_dtype, window, softcap, sinks, cu_seqlens_q,
                                   max_seqlen_q, cu_seqlens_k_new, rotary_cos, rotary_sin, rotary_interleaved, q8_out)
    for name, t in (("q", q), ("k", k_new), ("v", v_new), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if q.dtype not in (torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (float16, bfloat16 or torch.float8_e4m3fn)")
    if k_new.dtype != q.dtype or v_new.dtype != q.dtype:
        raise NotImplementedError(f"{who}: mixed dtypes are not supported: q, k, v must be all float16, all bfloat16 or all "
                                  f"torch.float8_e4m3fn (got {q.dtype}, {k_new.dtype}, {v_new.dtype})")
    e4 = q.dtype == torch.float8_e4m3fn
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
    if e4 and (rotary_cos is not None or rotary_sin is not None):
        raise NotImplementedError(f"{who}: rotary_cos / rotary_sin are not supported with torch.float8_e4m3fn q, k, v (codes cannot be rotated)")
    if e4 and q8_out is not None:
        raise NotImplementedError(f"{who}: q8_out is not supported with a torch.float8_e4m3fn q (it is used in place)")
    if out_dtype is None:
        out_dtype = torch.bfloat16 if e4 else q.dtype
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    paged = block_table is not None
    if paged and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    for name, t in (("block_table", block_table), ("cache_batch_idx", cache_batch_idx)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32):
            dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (int32 tensor expected)")
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise RuntimeError(f"{who}: q must be (B, Nq, H_q, 128) and k_cache, v_cache " +
                           ("pools (num_blocks, page_block_size, H_kv, 128)" if paged else "(B_cache, cache_len, H_kv, 128)") +
                           f" of one shape; got {tuple(q.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache), ("k", k_new), ("v", v_new)):
        if t.shape[-1] != 128:
            raise NotImplementedError(f"{who}: head_dim {t.shape[-1]} is not supported (128 only); got {name} of shape {tuple(t.shape)}")
    b, nq, hq = q.shape[0], q.shape[1], q.shape[2]
    hkv = k_cache.shape[2]
    if hkv == 0 or hq == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: H_q = {hq} must be a multiple of H_kv = {hkv}")
    if k_new.dim() != 4 or k_new.shape[0] != b or k_new.shape[1] < 1 or k_new.shape[2] != hkv or v_new.shape != k_new.shape:
        raise RuntimeError(f"{who}: k and v must be (B, N_new >= 1, H_kv, 128) = ({b}, ., {hkv}, 128) tensors of one shape; got "
                           f"{tuple(k_new.shape)}, {tuple(v_new.shape)}")
    nnew = k_new.shape[1]
    if cache_seqlens is None:
        raise RuntimeError(f"{who}: cache_seqlens is required (the lengths before the append: an int32 (B,) tensor or an int)")
    if isinstance(cache_seqlens, int) and not isinstance(cache_seqlens, bool):
        cache_seqlens = torch.full((b,), cache_seqlens, dtype=torch.int32, device=q.device)
    if not (isinstance(cache_seqlens, torch.Tensor) and cache_seqlens.dtype == torch.int32 and cache_seqlens.shape == (b,)):
        raise RuntimeError(f"{who}: cache_seqlens must be an int32 tensor of shape (B,) = ({b},) or an int")
    rot = rotary_cos is not None or rotary_sin is not None
    rdim = 0
    if rot:
        if rotary_cos is None or rotary_sin is None:
            raise RuntimeError(f"{who}: rotary_cos and rotary_sin must be given together")
        for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != q.dtype or t.dim() != 2 or t.shape != rotary_cos.shape or t.numel() == 0:
                raise RuntimeError(f"{who}: {name} must be a (seqlen_ro, rotary_dim / 2) tensor of q's dtype, rotary_cos and rotary_sin of "
                                   f"one shape")
        rdim = 2 * rotary_cos.shape[1]
        if rdim % 16 != 0 or not 16 <= rdim <= 128:
            raise RuntimeError(f"{who}: rotary_dim = 2 * rotary_cos.shape[1] must be a multiple of 16 in [16, 128], got {rdim}")
    if q8_out is not None and not (isinstance(q8_out, torch.Tensor) and q8_out.dtype == torch.float8_e4m3fn and q8_out.shape == q.shape):
        raise RuntimeError(f"{who}: q8_out must be a torch.float8_e4m3fn tensor of q's shape {tuple(q.shape)}")
    tensors = [t for t in (q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, cache_batch_idx, rotary_cos, rotary_sin, q8_out)
               if t is not None]
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f"{who}: all tensors must be on one device")
    scale = 128 ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise RuntimeError(f"{who}: softmax_scale must be finite and > 0 (got {scale})")
    ns = operator.index(num_splits)
    if ns < 0 or ns > 256:
        raise RuntimeError(f"{who}: num_splits must lie in [0, 256] (got {ns})")
    views = [("q", q, hq), ("k_cache", k_cache, hkv), ("v_cache", v_cache, hkv)] + ([("q8_out", q8_out, hq)] if q8_out is not None else [])
    for name, t, heads in views:
        unit = 16 // t.element_size()
        if t.numel() and ((heads > 1 and t.stride(2) != 128) or t.stride(3) != 1):
            raise ValueError(f"{who}: {name} must have adjacent heads with a contiguous last dim (strides {t.stride()})")
        if t.numel() and (t.data_ptr() % 16 != 0 or t.stride(0) % unit != 0 or t.stride(1) % unit != 0 or t.stride(0) < 0 or
                          (t.shape[1] > 1 and t.stride(1) < heads * 128)):
            raise ValueError(f"{who}: {name} is a view the kernel cannot address: a 16-byte aligned start, batch and token strides that "
                             f"are multiples of 16 bytes and rows that do not overlap are needed (strides {t.stride()})")
    # (batch stride, token stride) in bytes of a view checked above
    bstride = lambda t: (max(t.stride(0), 0) if t.shape[0] > 1 else 0) * t.element_size()   # noqa: E731
    tstride = lambda t, heads: (t.stride(1) if t.shape[1] > 1 else heads * 128) * t.element_size()   # noqa: E731
    if paged:
        nblk, ps = k_cache.shape[0], k_cache.shape[1]
        if ps < 16 or ps % 16 != 0:
            raise RuntimeError(f"{who}: page_block_size must be a positive multiple of 16, got {ps}")
        if block_table.dim() != 2 or block_table.shape[0] != b or block_table.shape[1] < 1:
            raise RuntimeError(f"{who}: block_table must be an int32 (B, max_blocks_per_seq >= 1) tensor, B = {b}; got "
                               f"{tuple(block_table.shape)}")
        if nblk < 1:
            raise RuntimeError(f"{who}: the pools must hold at least one page")
        if block_table.stride(1) != 1 and block_table.shape[1] > 1:
            block_table = block_table.contiguous()
        cap, cbatch = block_table.shape[1] * ps, 0
        pages = (max(block_table.stride(0), block_table.shape[1]), nblk, ps)
    else:
        cap = k_cache.shape[1]
        if cap < 1:
            raise RuntimeError(f"{who}: the caches must hold at least one token")
        if cache_batch_idx is not None:
            if cache_batch_idx.shape != (b,):
                raise RuntimeError(f"{who}: cache_batch_idx must be an int32 tensor of shape (B,) = ({b},)")
            cache_batch_idx = cache_batch_idx.contiguous()
            cbatch = k_cache.shape[0]
        elif k_cache.shape[0] != b:
            raise RuntimeError(f"{who}: the caches hold {k_cache.shape[0]} rows for a batch of {b} (pass cache_batch_idx to select rows)")
        else:
            cbatch = 0
        pages = (0, 0, 0)
    if nnew > cap:
        raise RuntimeError(f"{who}: N_new = {nnew} new tokens do not fit the capacity {cap}")
    if rot and rotary_cos.shape[0] < cap + max(0, nq - nnew):
        raise RuntimeError(f"{who}: rotary_cos / rotary_sin have {rotary_cos.shape[0]} rows; the capacity {cap} + max(0, Nq - N_new) = "
                           f"{cap + max(0, nq - nnew)} are needed")
    cache_seqlens = cache_seqlens.contiguous()
    k_new, v_new = k_new.contiguous(), v_new.contiguous()
    esz = q.element_size()
    knb, knt = (x * esz for x in _kv_strides(who, "k", k_new, hkv, 128, False))
    vnb, vnt = (x * esz for x in _kv_strides(who, "v", v_new, hkv, 128, False))
    qdp, qds, keep_q = _kv_descale(who, "q_descale", q_descale, q, b, hkv)
    kdp, kds, keep_k = _kv_descale(who, "k_descale", k_descale, q, b, hkv)
    vdp, vds, keep_v = _kv_descale(who, "v_descale", v_descale, q, b, hkv)
    mod, tail, keep_s = _fp8_mod(who, q, hq, window, softcap, sinks)
    if not mod:
        tail = (-1, -1, 0.0, 0, 0)
    code = _E4M3_CODE if e4 else _DTYPE_CODE[q.dtype]
    with torch.cuda.device(q.device):
        o = torch.empty((b, nq, hq, 128), dtype=out_dtype, device=q.device)
        lse = torch.empty((b, hq, nq), dtype=torch.float32, device=q.device)
        if b == 0:
            return o, lse
        _tabs, rotary = _rotary_tables(rotary_cos, rotary_sin, rdim, rotary_interleaved)
        need = int(_lib.fa_fp8_kvcache_step_workspace_bytes(b, hq, hkv, nq, cap, 128, ns, int(bool(causal)), tail[0], tail[1],
                                                            int(sinks is not None), code, int(q8_out is not None)))
        ws = _workspace(q.device, need)
        q8 = (q8_out.data_ptr(), bstride(q8_out), tstride(q8_out, hq)) if q8_out is not None else (0, 0, 0)
        _call("fa_fp8_kvcache_step", (
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), o.data_ptr(), lse.data_ptr(), qdp, kdp, vdp, cache_seqlens.data_ptr(),
            block_table.data_ptr() if paged else 0, cache_batch_idx.data_ptr() if cache_batch_idx is not None else 0, b, hq, hkv, nq, cap,
            cbatch, 128, _DTYPE_CODE[out_dtype], code, _E4M3_CODE, bstride(q), tstride(q, hq), bstride(k_cache), tstride(k_cache, hkv),
            bstride(v_cache), tstride(v_cache, hkv), *pages, qds, kds, vds, int(bool(causal)), scale, ns, ws.data_ptr(), ws.numel(),
            _stream_ptr(q.device), *tail, k_new.data_ptr(), v_new.data_ptr(), nnew, knb, knt, vnb, vnt, code, *q8, *rotary))
    del keep_q, keep_k, keep_v, keep_s, _tabs
    return o, lse


def _fp8_kvcache_packed(who, q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, cache_batch_idx, q_descale, k_descale, v_descale,
                        softmax_scale, causal, num_splits, out_dtype, window, softcap, sinks, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new,
                        rotary_cos, rotary_sin, rotary_interleaved, q8_out):
    """fp8_kvcache_forward (k_new is None) and fp8_kvcache_step through the _varlen entry points: packed queries (cu_seqlens_q), packed
    or padded new keys, head dims 64 / 128 / 256.  The offsets are int32 (B + 1,) device tensors and are never read on the host."""
    step = k_new is not None
    tensors = [("q", q), ("k_cache", k_cache), ("v_cache", v_cache)] + ([("k", k_new), ("v", v_new)] if step else [])
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    packed = cu_seqlens_q is not None
    if max_seqlen_q is not None and not packed:
        raise RuntimeError(f"{who}: max_seqlen_q goes with cu_seqlens_q")
    if cu_seqlens_k_new is not None and not packed:
        raise RuntimeError(f"{who}: cu_seqlens_k_new needs cu_seqlens_q (packed new keys go with packed queries)")
    if packed and (isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int)):
        raise RuntimeError(f"{who}: max_seqlen_q (an int, the most query tokens of one sequence) is required with cu_seqlens_q")
    if step:
        if q.dtype not in (torch.float16, torch.bfloat16, torch.float8_e4m3fn):
            raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (float16, bfloat16 or torch.float8_e4m3fn)")
        if k_new.dtype != q.dtype or v_new.dtype != q.dtype:
            raise NotImplementedError(f"{who}: mixed dtypes are not supported: q, k, v must be all float16, all bfloat16 or all "
                                      f"torch.float8_e4m3fn (got {q.dtype}, {k_new.dtype}, {v_new.dtype})")
    elif q.dtype != torch.float8_e4m3fn:
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (torch.float8_e4m3fn expected)")
    e4 = q.dtype == torch.float8_e4m3fn
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
    if e4 and (rotary_cos is not None or rotary_sin is not None):
        raise NotImplementedError(f"{who}: rotary_cos / rotary_sin are not supported with torch.float8_e4m3fn q, k, v (codes cannot be rotated)")
    if e4 and q8_out is not None:
        raise NotImplementedError(f"{who}: q8_out is not supported with a torch.float8_e4m3fn q (it is used in place)")
    if out_dtype is None:
        out_dtype = torch.bfloat16 if e4 else q.dtype
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    paged = block_table is not None
    if paged and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    for name, t in (("block_table", block_table), ("cache_batch_idx", cache_batch_idx), ("cu_seqlens_q", cu_seqlens_q),
                    ("cu_seqlens_k_new", cu_seqlens_k_new)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32):
            dt = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (int32 tensor expected)")
    qdim = 3 if packed else 4
    if q.dim() != qdim or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise RuntimeError(f"{who}: q must be " + ("packed (total_q, H_q, d)" if packed else "(B, Nq, H_q, d)") + " and k_cache, v_cache " +
                           ("pools (num_blocks, page_block_size, H_kv, d)" if paged else "(B_cache, cache_len, H_kv, d)") +
                           f" of one shape; got {tuple(q.shape)}, {tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    d = _fp8_head_dim(who, True, **dict(tensors))
    hq, hkv = q.shape[-2], k_cache.shape[2]
    if hkv == 0 or hq == 0 or hq % hkv != 0:
        raise RuntimeError(f"{who}: H_q = {hq} must be a multiple of H_kv = {hkv}")
    if packed:
        if cu_seqlens_q.dim() != 1 or cu_seqlens_q.shape[0] < 1:
            raise RuntimeError(f"{who}: cu_seqlens_q must be an int32 (B + 1,) tensor, got {tuple(cu_seqlens_q.shape)}")
        b, total_q, nq = cu_seqlens_q.shape[0] - 1, q.shape[0], 0
        if max_seqlen_q < 0 or max_seqlen_q > total_q:
            raise RuntimeError(f"{who}: max_seqlen_q = {max_seqlen_q} must lie in [0, total_q = {total_q}]")
    else:
        b, total_q, nq, max_seqlen_q = q.shape[0], 0, q.shape[1], 0
    packed_kn = cu_seqlens_k_new is not None
    nnew = total_kn = 0
    if step:
        if packed_kn:
            if cu_seqlens_k_new.shape != (b + 1,):
                raise RuntimeError(f"{who}: cu_seqlens_k_new must be an int32 (B + 1,) = ({b + 1},) tensor, got {tuple(cu_seqlens_k_new.shape)}")
            if k_new.dim() != 3 or k_new.shape[1] != hkv or v_new.shape != k_new.shape:
                raise RuntimeError(f"{who}: k and v must be packed (total_k_new, H_kv, d) = (., {hkv}, {d}) tensors of one shape; got "
                                   f"{tuple(k_new.shape)}, {tuple(v_new.shape)}")
            total_kn = k_new.shape[0]
        else:
            if k_new.dim() != 4 or k_new.shape[0] != b or k_new.shape[1] < 1 or k_new.shape[2] != hkv or v_new.shape != k_new.shape:
                raise RuntimeError(f"{who}: k and v must be (B, N_new >= 1, H_kv, d) = ({b}, ., {hkv}, {d}) tensors of one shape; got "
                                   f"{tuple(k_new.shape)}, {tuple(v_new.shape)}")
            nnew = k_new.shape[1]
        if cache_seqlens is None:
            raise RuntimeError(f"{who}: cache_seqlens is required (the lengths before the append: an int32 (B,) tensor or an int)")
    if isinstance(cache_seqlens, int) and not isinstance(cache_seqlens, bool):
        cache_seqlens = torch.full((b,), cache_seqlens, dtype=torch.int32, device=q.device)
    if cache_seqlens is not None and not (isinstance(cache_seqlens, torch.Tensor) and cache_seqlens.dtype == torch.int32 and
                                          cache_seqlens.shape == (b,)):
        raise RuntimeError(f"{who}: cache_seqlens must be an int32 tensor of shape (B,) = ({b},), an int or None")
    rot = rotary_cos is not None or rotary_sin is not None
    rdim = 0
    if rot:
        if rotary_cos is None or rotary_sin is None:
            raise RuntimeError(f"{who}: rotary_cos and rotary_sin must be given together")
        for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
            if not isinstance(t, torch.Tensor) or t.dtype != q.dtype or t.dim() != 2 or t.shape != rotary_cos.shape or t.numel() == 0:
                raise RuntimeError(f"{who}: {name} must be a (seqlen_ro, rotary_dim / 2) tensor of q's dtype, rotary_cos and rotary_sin of "
                                   f"one shape")
        rdim = 2 * rotary_cos.shape[1]
        if rdim % 16 != 0 or not 16 <= rdim <= d:
            raise RuntimeError(f"{who}: rotary_dim = 2 * rotary_cos.shape[1] must be a multiple of 16 in [16, {d}], got {rdim}")
    if q8_out is not None and not (isinstance(q8_out, torch.Tensor) and q8_out.dtype == torch.float8_e4m3fn and q8_out.shape == q.shape):
        raise RuntimeError(f"{who}: q8_out must be a torch.float8_e4m3fn tensor of q's shape {tuple(q.shape)}")
    every = [t for t in (q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, cache_batch_idx, cu_seqlens_q, cu_seqlens_k_new,
                         rotary_cos, rotary_sin, q8_out) if t is not None]
    for t in every:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensors must be on the GPU (HIP device); there is no CPU path")
    if len({t.device for t in every}) != 1:
        raise RuntimeError(f"{who}: all tensors must be on one device")
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise RuntimeError(f"{who}: softmax_scale must be finite and > 0 (got {scale})")
    ns = operator.index(num_splits)
    if ns < 0 or ns > 256:
        raise RuntimeError(f"{who}: num_splits must lie in [0, 256] (got {ns})")
    # views: (tensor, heads, the dim of its tokens); a batch dim, where there is one, is dim 0
    views = [("q", q, hq, qdim - 3), ("k_cache", k_cache, hkv, 1), ("v_cache", v_cache, hkv, 1)]
    if q8_out is not None:
        views.append(("q8_out", q8_out, hq, qdim - 3))
    for name, t, heads, tdim in views:
        unit = 16 // t.element_size()
        if t.numel() and ((heads > 1 and t.stride(-2) != d) or t.stride(-1) != 1):
            raise ValueError(f"{who}: {name} must have adjacent heads with a contiguous last dim (strides {t.stride()})")
        if t.numel() and (t.data_ptr() % 16 != 0 or any(t.stride(i) % unit != 0 or t.stride(i) < 0 for i in range(tdim + 1)) or
                          (t.shape[tdim] > 1 and t.stride(tdim) < heads * d)):
            raise ValueError(f"{who}: {name} is a view the kernel cannot address: a 16-byte aligned start, batch and token strides that "
                             f"are multiples of 16 bytes and rows that do not overlap are needed (strides {t.stride()})")
    bstride = lambda t: (max(t.stride(0), 0) if t.dim() == 4 and t.shape[0] > 1 else 0) * t.element_size()   # noqa: E731
    tstride = lambda t, heads: (t.stride(-3) if t.shape[-3] > 1 else heads * d) * t.element_size()   # noqa: E731
    if paged:
        nblk, ps = k_cache.shape[0], k_cache.shape[1]
        if ps < 16 or ps % 16 != 0:
            raise RuntimeError(f"{who}: page_block_size must be a positive multiple of 16, got {ps}")
        if block_table.dim() != 2 or block_table.shape[0] != b or block_table.shape[1] < 1:
            raise RuntimeError(f"{who}: block_table must be an int32 (B, max_blocks_per_seq >= 1) tensor, B = {b}; got "
                               f"{tuple(block_table.shape)}")
        if nblk < 1:
            raise RuntimeError(f"{who}: the pools must hold at least one page")
        if block_table.stride(1) != 1 and block_table.shape[1] > 1:
            block_table = block_table.contiguous()
        cap, cbatch = block_table.shape[1] * ps, 0
        pages = (max(block_table.stride(0), block_table.shape[1]), nblk, ps)
    else:
        cap = k_cache.shape[1]
        if cap < 1:
            raise RuntimeError(f"{who}: the caches must hold at least one token")
        if cache_batch_idx is not None:
            if cache_batch_idx.shape != (b,):
                raise RuntimeError(f"{who}: cache_batch_idx must be an int32 tensor of shape (B,) = ({b},)")
            cache_batch_idx = cache_batch_idx.contiguous()
            cbatch = k_cache.shape[0]
        elif k_cache.shape[0] != b:
            raise RuntimeError(f"{who}: the caches hold {k_cache.shape[0]} rows for a batch of {b} (pass cache_batch_idx to select rows)")
        else:
            cbatch = 0
        pages = (0, 0, 0)
    if step and not packed_kn and nnew > cap:
        raise RuntimeError(f"{who}: N_new = {nnew} new tokens do not fit the capacity {cap}")
    ro_need = cap + (max_seqlen_q if packed else max(0, nq - nnew))
    if rot and rotary_cos.shape[0] < ro_need:
        raise RuntimeError(f"{who}: rotary_cos / rotary_sin have {rotary_cos.shape[0]} rows; the capacity {cap} + " +
                           ("max_seqlen_q" if packed else "max(0, Nq - N_new)") + f" = {ro_need} are needed")
    if cache_seqlens is not None:
        cache_seqlens = cache_seqlens.contiguous()
    if packed:
        cu_seqlens_q = cu_seqlens_q.contiguous()
    if packed_kn:
        cu_seqlens_k_new = cu_seqlens_k_new.contiguous()
    qdp, qds, keep_q = _kv_descale(who, "q_descale", q_descale, q, b, hkv)
    kdp, kds, keep_k = _kv_descale(who, "k_descale", k_descale, q, b, hkv)
    vdp, vds, keep_v = _kv_descale(who, "v_descale", v_descale, q, b, hkv)
    _mod, tail, keep_s = _fp8_mod(who, q, hq, window, softcap, sinks, True)
    code = _E4M3_CODE if e4 else _DTYPE_CODE[q.dtype]
    with torch.cuda.device(q.device):
        o = torch.empty((total_q, hq, d) if packed else (b, nq, hq, d), dtype=out_dtype, device=q.device)
        lse = torch.empty((hq, total_q) if packed else (b, hq, nq), dtype=torch.float32, device=q.device)
        if b == 0 or (not step and (total_q == 0 or max_seqlen_q == 0 if packed else nq == 0)):
            return o, lse
        head = (q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), o.data_ptr(), lse.data_ptr(), qdp, kdp, vdp,
                cache_seqlens.data_ptr() if cache_seqlens is not None else 0, block_table.data_ptr() if paged else 0,
                cache_batch_idx.data_ptr() if cache_batch_idx is not None else 0, b, hq, hkv, nq, cap, cbatch, d, _DTYPE_CODE[out_dtype], code,
                _E4M3_CODE, bstride(q), tstride(q, hq), bstride(k_cache), tstride(k_cache, hkv), bstride(v_cache), tstride(v_cache, hkv),
                *pages, qds, kds, vds, int(bool(causal)), scale, ns)
        group = (cu_seqlens_q.data_ptr() if packed else 0, total_q, max_seqlen_q)
        if not step:
            if packed:
                need = int(_lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(b, hq, hkv, total_q, max_seqlen_q, cap, d, ns, int(bool(causal)),
                                                                              tail[0], tail[1], int(sinks is not None)))
            else:
                need = int(_lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(b, hq, hkv, nq, cap, d, ns, int(bool(causal)), tail[0], tail[1],
                                                                            int(sinks is not None)))
            ws = _workspace(q.device, need)
            _call("fa_fp8_forward_kvcache_varlen", (*head, ws.data_ptr() if need else 0, ws.numel() if need else 0, _stream_ptr(q.device),
                                                    *tail, *group))
        else:
            k_new, v_new = k_new.contiguous(), v_new.contiguous()
            esz = q.element_size()
            if packed_kn:
                knb = vnb = 0
                knt = vnt = hkv * d * esz
            else:
                knb, knt = (x * esz for x in _kv_strides(who, "k", k_new, hkv, d, False))
                vnb, vnt = (x * esz for x in _kv_strides(who, "v", v_new, hkv, d, False))
            _tabs, rotary = _rotary_tables(rotary_cos, rotary_sin, rdim, rotary_interleaved)
            need = int(_lib.fa_fp8_kvcache_step_varlen_workspace_bytes(b, hq, hkv, nq, cap, d, ns, int(bool(causal)), tail[0], tail[1],
                                                                       int(sinks is not None), code, int(q8_out is not None), total_q,
                                                                       max_seqlen_q))
            ws = _workspace(q.device, need)
            q8 = (q8_out.data_ptr(), bstride(q8_out), tstride(q8_out, hq)) if q8_out is not None else (0, 0, 0)
            _call("fa_fp8_kvcache_step_varlen", (*head, ws.data_ptr(), ws.numel(), _stream_ptr(q.device), *tail, k_new.data_ptr(),
                                                 v_new.data_ptr(), nnew, knb, knt, vnb, vnt, code, *q8, *rotary, *group,
                                                 cu_seqlens_k_new.data_ptr() if packed_kn else 0, total_kn))
            del _tabs
    del keep_q, keep_k, keep_v, keep_s
    return o, lse
