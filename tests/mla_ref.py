"""fp64 CPU reference of KV-cache decoding with a second query operand (include/fa_mi355x.h: fa_ex_forward_kvcache_qv):
for query head h reading K/V head h // G

    s[i, j] = scale * (q[i, h, :] . k[j, hk, :] + qv[i, h, :] . v[j, hk, :]),   o[i, h, :] = sum_j softmax_j(s)[i, j] v[j, hk, :]

per sequence, with the band mask of tests/kvcache_full_ref.dense_attention (causal / window aligned bottom-right) and the paged
gather of tests/kvcache_paged_ref.paged_tokens (a page outside the pool: zero keys with zero values, which still take part in
the softmax with score 0).  CPU tensors only; it never imports the extension."""
import math

import torch

from tests.kvcache_paged_ref import paged_tokens

NEG_INF = -math.inf


def mla_attention(qd, qvd, kd, vd, causal, window, scale):
    """(o (nq, H_q, d_v), lse (H_q, nq)) of one sequence in fp64: qd (nq, H_q, d), qvd (nq, H_q, d_v), kd (lk, H_kv, d), vd
    (lk, H_kv, d_v).  Row i sees key j inside [i + lk - nq - wl, i + lk - nq + wr] (causal: wr = 0); a row without a visible key
    gives o = 0 and lse = -inf."""
    nq, hq, _d = qd.shape
    lk, dv = kd.shape[0], vd.shape[2]
    o = torch.zeros((nq, hq, dv), dtype=torch.float64)
    lse = torch.full((hq, nq), NEG_INF, dtype=torch.float64)
    if lk == 0:
        return o, lse
    g = hq // kd.shape[1]
    diag = torch.arange(nq).view(-1, 1) + (lk - nq)
    j = torch.arange(lk).view(1, -1)
    wl, wr = window
    vis = torch.ones((nq, lk), dtype=torch.bool)
    if causal:
        vis &= j <= diag
    if wl >= 0:
        vis &= j >= diag - wl
    if wr >= 0:
        vis &= j <= diag + wr
    for h in range(hq):
        hk = h // g
        s = scale * (qd[:, h] @ kd[:, hk].T + qvd[:, h] @ vd[:, hk].T)      # (nq, lk)
        s = s.masked_fill(~vis, NEG_INF)
        for i in range(nq):
            if not vis[i].any():
                continue
            m = s[i].max()
            e = torch.exp(s[i] - m)
            tot = e.sum()
            lse[h, i] = m + torch.log(tot)
            o[i, h] = (e / tot) @ vd[:, hk]
    return o, lse


def lengths(cache_seqlens, bsz, cap):
    """the clamped length of every sequence: None = the capacity, an int for all, or one per sequence"""
    if cache_seqlens is None:
        return [cap] * bsz
    if isinstance(cache_seqlens, int):
        return [min(max(cache_seqlens, 0), cap)] * bsz
    return [min(max(int(x), 0), cap) for x in cache_seqlens]


def mla_reference(q, qv, k_cache, v_cache, cache_seqlens=None, causal=False, window=(-1, -1), softmax_scale=None, block_table=None,
                  cache_batch_idx=None):
    """(o (B, Nq, H_q, d_v), lse (B, H_q, Nq)) in fp64 of flash_attn_with_kvcache(q, k_cache, v_cache, qv=qv, ...).  The caches are
    (B, cap, H_kv, .) tensors, rows picked by cache_batch_idx (an index outside the cache: zero keys with zero values), or pools
    (num_blocks, ps, H_kv, .) under block_table."""
    bsz, nq, hq, d = q.shape
    dv = qv.shape[3]
    ps = k_cache.shape[1]
    cap = block_table.shape[1] * ps if block_table is not None else ps
    scale = (d + dv) ** -0.5 if softmax_scale is None else float(softmax_scale)
    lens = lengths(cache_seqlens, bsz, cap)
    o = torch.zeros((bsz, nq, hq, dv), dtype=torch.float64)
    lse = torch.full((bsz, hq, nq), NEG_INF, dtype=torch.float64)
    for b in range(bsz):
        lk = lens[b]
        if block_table is not None:
            kt, vt = paged_tokens(k_cache, block_table[b], lk, ps), paged_tokens(v_cache, block_table[b], lk, ps)
        else:
            row = int(cache_batch_idx[b]) if cache_batch_idx is not None else b
            if 0 <= row < k_cache.shape[0]:
                kt, vt = k_cache[row, :lk], v_cache[row, :lk]
            else:   # a row outside the cache reads as zeros, as without qv (tests/kvcache_full_ref.py): o = 0, lse = log(keys in the band)
                kt, vt = torch.zeros((lk,) + tuple(k_cache.shape[2:]), dtype=k_cache.dtype), torch.zeros((lk,) + tuple(v_cache.shape[2:]), dtype=v_cache.dtype)
        o[b], lse[b] = mla_attention(q[b].double(), qv[b].double(), kt.double(), vt.double(), bool(causal), window, scale)
    return o, lse
