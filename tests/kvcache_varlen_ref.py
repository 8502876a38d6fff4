"""Helpers for the packed-query KV-cache tests (include/fa_mi355x.h: fa_ex_forward_kvcache_varlen).

A pure-Python model of the device clamp (csrc/fa_decode.hip: kv_cu_range) and of how a split-kernel wave finds its rows of the
packed tensors, and the per-sequence fp64 reference: every sequence of a packed call is by definition the padded call on that
sequence alone, so the reference loops over the sequences with tests/kvcache_paged_ref.reference (tests/sink_ref with sinks).
CPU tensors only."""
import math

import torch

from tests.kvcache_paged_ref import reference

ROWS = 16   # query rows of a split-kernel tile


def cu_range(cu, b, total, bound):
    """(start, n) of sequence b in a packed tensor of `total` tokens, from untrusted offsets: start = clamp(cu[b], 0, total),
    n = clamp(cu[b + 1] - cu[b], 0, min(bound, total - start)).  bound: max_seqlen_q for q, the capacity for k_new."""
    c0, c1 = int(cu[b]), int(cu[b + 1])
    start = min(max(c0, 0), total)
    return start, min(max(c1 - c0, 0), min(bound, total - start))


def row_tiles(max_seqlen_q, g):
    """grid row tiles of a call: ceil(max_seqlen_q * G / 16)"""
    return (max_seqlen_q * g + ROWS - 1) // ROWS


def tile_rows(cu, b, rt, total_q, max_seqlen_q, g):
    """The (packed token, head in the group) rows that the wave of (sequence b, row tile rt) loads and stores, in lane order;
    None when it leaves before its first load (the tile starts at or past the sequence's G * nq_b rows)."""
    start, nq = cu_range(cu, b, total_q, max_seqlen_q)
    rows = g * nq
    if ROWS * rt >= rows:
        return None
    return [(start + pr // g, pr % g) for pr in range(ROWS * rt, min(ROWS * rt + ROWS, rows))]


def well_formed(cu, total, bound):
    return cu[0] >= 0 and cu[-1] <= total and all(0 <= y - x <= bound for x, y in zip(cu[:-1], cu[1:]))


def lengths_to_cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def packed_reference(q, cu_q, ks, vs, causal, window, scale, softcap=0.0, slopes=None, sinks=None):
    """o (total_q, H_q, d) fp64 and lse (H_q, total_q) float64 of a packed call with well-formed cu_q: sequence b's tokens
    q[cu_q[b]:cu_q[b + 1]] (q: any float dtype, e.g. already rotated in fp64) over its keys ks[b], vs[b] ((len_k_b, H_kv, d)).
    slopes: (H_q,) or (B, H_q).  Rows no sequence owns: o = 0, lse = nan."""
    total_q, hq, d = q.shape
    o = torch.zeros((total_q, hq, d), dtype=torch.float64)
    lse = torch.full((hq, total_q), math.nan, dtype=torch.float64)
    for b in range(len(cu_q) - 1):
        lo, hi = int(cu_q[b]), int(cu_q[b + 1])
        if hi <= lo:
            continue
        qb = q[lo:hi]
        if sinks is not None:
            from tests import sink_ref as sr

            assert slopes is None
            if ks[b].shape[0] == 0:   # no key: o = 0, lse = the sink
                lse[:, lo:hi] = sinks.detach().cpu().double().view(hq, 1)
                continue
            r = sr.sink_reference(qb.transpose(0, 1), ks[b].transpose(0, 1), vs[b].transpose(0, 1), None, sinks, causal, scale,
                                  window=window, softcap=softcap)
            o[lo:hi], lse[:, lo:hi] = r[0].transpose(0, 1), r[1].double()
        else:
            sl = None if slopes is None else (slopes[b] if slopes.dim() == 2 else slopes)
            ob, lb = reference(qb.unsqueeze(0), [ks[b]], [vs[b]], causal, window, scale, softcap, sl)
            o[lo:hi], lse[:, lo:hi] = ob[0], lb[0]
    return o, lse
