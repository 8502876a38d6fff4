"""fp64 CPU reference of sparse MLA decoding (include/fa_mi355x.h: fa_mla_sparse_forward): for sequence b, query token i, query head h
reading K/V head hk = h // G and the list I = indices[b, i, hk, :]

    visible(j)  <=>  0 <= I[j] < len_b  and, if causal,  I[j] <= len_b - Nq + i
    s[j] = scale * (q[b, i, h, :] . k[I[j], hk, :] + qv[b, i, h, :] . v[I[j], hk, :])      over the visible j
    o[b, i, h, :] = sum_j softmax_j(s)[j] v[I[j], hk, :],    lse[b, h, i] = logsumexp_j s[j]

per sequence.  Every list position is a key (a token named twice counts twice); a row without a visible entry gives o = 0 and
lse = -inf.  Token positions are resolved as tests/mla_ref.py resolves them: the lengths of mla_ref.lengths, the pages of
tests/kvcache_paged_ref.paged_tokens (a page outside the pool: zero keys with zero values that still take part in the softmax
with score 0), and cache rows through cache_batch_idx (a row outside the cache likewise).  CPU tensors only; it never imports
the extension."""
import math

import torch

from tests.kvcache_paged_ref import paged_tokens
from tests.mla_ref import lengths

NEG_INF = -math.inf


def visible_entries(row, lk, bound):
    """the entries of one list that are keys, in list order: 0 <= entry < lk and entry <= bound"""
    return [int(t) for t in row.tolist() if 0 <= int(t) < lk and int(t) <= bound]


def mla_sparse_reference(q, qv, k_cache, v_cache, indices, cache_seqlens=None, causal=False, softmax_scale=None, block_table=None,
                         cache_batch_idx=None):
    """(o (B, Nq, H_q, d_v), lse (B, H_q, Nq)) in fp64 of flash_mla_sparse_attn(q, qv, k_cache, v_cache, indices, ...).  indices is
    (B, Nq, topk) or (B, Nq, H_kv, topk); the caches are (B, cap, H_kv, .) tensors, rows picked by cache_batch_idx, or pools
    (num_blocks, ps, H_kv, .) under block_table."""
    bsz, nq, hq, d = q.shape
    dv = qv.shape[3]
    ps, hkv = k_cache.shape[1], k_cache.shape[2]
    g = hq // hkv
    cap = block_table.shape[1] * ps if block_table is not None else ps
    scale = (d + dv) ** -0.5 if softmax_scale is None else float(softmax_scale)
    lens = lengths(cache_seqlens, bsz, cap)
    if indices.dim() == 3:
        indices = indices.unsqueeze(2).expand(-1, -1, hkv, -1)
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
            else:
                kt = torch.zeros((lk,) + tuple(k_cache.shape[2:]), dtype=k_cache.dtype)
                vt = torch.zeros((lk,) + tuple(v_cache.shape[2:]), dtype=v_cache.dtype)
        kt, vt = kt.double(), vt.double()
        for i in range(nq):
            bound = lk - nq + i if causal else lk - 1
            for hk in range(hkv):
                keys = visible_entries(indices[b, i, hk], lk, bound)
                if not keys:
                    continue
                ks, vs = kt[keys, hk], vt[keys, hk]                       # (n, d), (n, d_v)
                hs = slice(hk * g, (hk + 1) * g)
                s = scale * (q[b, i, hs].double() @ ks.T + qv[b, i, hs].double() @ vs.T)      # (G, n)
                m = s.max(dim=1, keepdim=True).values
                e = torch.exp(s - m)
                tot = e.sum(dim=1, keepdim=True)
                lse[b, hs, i] = (m + torch.log(tot)).squeeze(1)
                o[b, i, hs] = (e / tot) @ vs
    return o, lse
