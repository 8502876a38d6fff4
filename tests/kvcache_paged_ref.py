"""fp64 reference for the paged / indexed / left-padded KV-cache tests: per batch element, gather the sequence's tokens (through
a block table, a cache row index or a left pad), then attention over them with an explicit visibility mask — the form of
tests/test_kvcache_gpu.py's reference, on lists of per-sequence token tensors.  CPU tensors only."""
import math

import torch


def paged_tokens(pool, table_row, n, ps):
    """(n, H_kv, d): tokens [0, n) of one sequence, token t from pool[table_row[t // ps], t % ps]; a page number outside
    [0, num_blocks) reads as zeros"""
    out = torch.zeros((n,) + tuple(pool.shape[2:]), dtype=pool.dtype)
    for j in range((n + ps - 1) // ps):
        pg = int(table_row[j])
        lo, hi = j * ps, min(n, (j + 1) * ps)
        if 0 <= pg < pool.shape[0]:
            out[lo:hi] = pool[pg, :hi - lo]
    return out


def paged_append(pool, table, lens, new, ps):
    """write new[b, n] to token lens[b] + n of sequence b through the table, in place; an append to a page outside the pool is
    dropped"""
    for b in range(new.shape[0]):
        for n in range(new.shape[1]):
            t = int(lens[b]) + n
            pg = int(table[b, t // ps])
            if 0 <= pg < pool.shape[0]:
                pool[pg, t % ps] = new[b, n]


def reference(q, ks, vs, causal, window, scale, softcap=0.0, slopes=None):
    """o (B, Nq, H_q, d) fp64 and lse (B, H_q, Nq): sequence b attends over the tokens ks[b], vs[b] ((len_k, H_kv, d) each)"""
    b_, nq, hq, d = q.shape
    o = torch.zeros((b_, nq, hq, d), dtype=torch.float64)
    lse = torch.full((b_, hq, nq), -math.inf, dtype=torch.float64)
    wl, wr = window
    for b in range(b_):
        lk = ks[b].shape[0]
        if lk == 0:
            continue
        g = hq // ks[b].shape[1]
        qq = q[b].double().permute(1, 0, 2)                              # (H_q, Nq, d)
        kk = ks[b].double().permute(1, 0, 2).repeat_interleave(g, 0)    # (H_q, lk, d)
        vv = vs[b].double().permute(1, 0, 2).repeat_interleave(g, 0)
        s = scale * qq @ kk.transpose(1, 2)
        if softcap > 0:
            s = softcap * torch.tanh(s / softcap)
        i = torch.arange(nq).view(-1, 1)
        j = torch.arange(lk).view(1, -1)
        diag = i + lk - nq
        if slopes is not None:
            sl = (slopes[b] if slopes.dim() == 2 else slopes).double().cpu().view(-1, 1, 1)
            s = s - sl * (diag - j).abs().double()
        vis = torch.ones((nq, lk), dtype=torch.bool)
        if causal:
            vis &= j <= diag
        if wl >= 0:
            vis &= j >= diag - wl
        if wr >= 0:
            vis &= j <= diag + wr
        s = s.masked_fill(~vis, -math.inf)
        l = torch.logsumexp(s, -1)
        p = torch.exp(s - l.unsqueeze(-1)).nan_to_num(0.0)
        o[b] = (p @ vv).permute(1, 0, 2)
        lse[b] = l
    return o, lse
