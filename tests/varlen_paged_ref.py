"""Helpers for the paged varlen forward tests (flash_attention_varlen with block_table): scatter per-sequence K/V into a pool
behind a shuffled block table, gather a sequence back through a table (an out-of-pool page gives zeros), and a model of the
kernel's piece -> page arithmetic.  Device-agnostic: the tensors stay where the caller made them."""
import torch

from tests.kvcache_paged_ref import paged_tokens


def build_pool(ks, vs, ps, spare=3, seed=0, max_blocks=None, fill=float("nan")):
    """(k_pool, v_pool, table): the tokens of sequence b, ks[b] / vs[b] of shape (len_b, H_kv, d), on pages of `ps` tokens handed
    out in a shuffled order from a pool with `spare` pages more than are used.  Everything no token was written to holds `fill`
    (NaN: a read of it would show); table entries past ceil(len_b / ps) are -1."""
    g = torch.Generator().manual_seed(seed)
    need = [(k.shape[0] + ps - 1) // ps for k in ks]
    nblk = sum(need) + spare
    mb = max(need + [1]) if max_blocks is None else max_blocks
    order = torch.randperm(nblk, generator=g).tolist()
    kp = torch.full((nblk, ps) + tuple(ks[0].shape[1:]), fill, dtype=ks[0].dtype)
    vp = torch.full_like(kp, fill)
    table = torch.full((len(ks), mb), -1, dtype=torch.int32)
    for b, (k, v) in enumerate(zip(ks, vs)):
        for j in range(need[b]):
            pg = order.pop()
            table[b, j] = pg
            lo, hi = j * ps, min(k.shape[0], (j + 1) * ps)
            kp[pg, :hi - lo] = k[lo:hi]
            vp[pg, :hi - lo] = v[lo:hi]
    return kp, vp, table


def gather(pool, table_row, n, ps):
    """(n, H_kv, d): tokens [0, n) of one sequence through its table row; a page outside the pool reads as zeros"""
    return paged_tokens(pool, table_row, n, ps)


def piece_fetches(D, ps, length, tile0):
    """The 128-key tile at `tile0` of a sequence of `length` keys as the MFMA kernel stages it: 1-KiB pieces of 512 / D rows, wave
    w of 8 issuing pieces w, w + 8, ..  Per piece: (first key, rows below `length`, table slot), the slot clamped to the last one
    in use as the kernel does (a piece past the sequence fetches nothing, so its slot is never dereferenced for data)."""
    rpp = 512 // D
    last = (max(length, 1) - 1) // ps
    out = []
    for w in range(8):
        for j in range(128 // rpp // 8):
            key = tile0 + rpp * (w + 8 * j)
            rows = min(rpp, length - key)
            slot = min(pg_slot(key, ps), last)
            out.append((key, max(rows, 0), slot))
    return out


def pg_slot(t, ps):
    """t // ps as the kernels compute it: (t >> 4) * ceil(2^32 / (ps / 16)) >> 32 (a plain shift for ps = 16)"""
    g = ps // 16
    if g <= 1:
        return t >> 4
    m = ((1 << 32) + g - 1) // g
    return ((t >> 4) * m) >> 32
