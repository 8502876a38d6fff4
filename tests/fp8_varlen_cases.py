"""The packed and the paged form of the fp8 call (fa_fp8_forward_varlen, flash_attention_fp8_varlen): pure-Python
models of the two device rules the host cannot see — where a sequence's V^T tiles start, and what descriptor a 1-KiB K piece gets —
and the builders of the GPU tests (tests/test_fp8_varlen_gpu.py).  tests/test_fp8_varlen_cpu.py proves the models.

Sequence shapes (len_q, len_k) of the GPU sweep, four to a call so that B <= 4 and the shapes mix:
    SET_A  (1, 1)       one row, one key
           (40, 0)      an empty key sequence: every row dead
           (0, 40)      an empty query sequence: nothing is written
           (300, 40)    under the mask the whole first query tile is dead (the diagonal is shifted by -260)
    SET_B  (257, 129)   one row in the second query tile, one key in the second key tile; nb = 3 is odd
           (64, 300)    a ragged third key tile
           (256, 128)   whole tiles
           (17, 191)    an odd 64-block count: the second half of the last V^T tile is the zeroed one
Page sizes: 16, 48 (does not divide the 128-key tile), 256 (exceeds it).  Table variants: "shuffled" pages, "shared" (the first
page of the last sequence with a page is also the first page of another one), "strided" (pool views with padded page and token
strides, K and V padded differently)."""
import torch

SET_A = ((1, 1), (40, 0), (0, 40), (300, 40))
SET_B = ((257, 129), (64, 300), (256, 128), (17, 191))
SETS = {"A": SET_A, "B": SET_B}
PAGE_SIZES = (16, 48, 256)
TABLES = ("shuffled", "shared", "strided")
SENTINEL = 0x7F
D = 128


# ---- the models

def seq_span(cu, b, total, max_len):
    """fa_ex_common.h, seq_span: (start, len) of sequence b from untrusted offsets"""
    a = min(max(int(cu[b]), 0), total)
    e = min(max(int(cu[b + 1]), a), total)
    return a, min(e - a, max_len)


def paged_len(cu, b, cap):
    """fa_ex_common.h, paged_len"""
    return min(max(int(cu[b + 1]) - int(cu[b]), 0), cap)


def packed_tiles_per_head(batch, total_k):
    return total_k // 128 + batch


def paged_cap(max_k, max_blocks, ps):
    return min(max_k, max_blocks * ps)


def paged_tiles_per_head(batch, max_k, max_blocks, ps):
    return batch * ((paged_cap(max_k, max_blocks, ps) + 127) // 128)


def workspace_bytes(batch, hkv, total_k, max_k, max_blocks=0, ps=0):
    """include/fa_mi355x.h, fa_fp8_forward_varlen_workspace_bytes (ps > 0: the paged form)"""
    tiles = paged_tiles_per_head(batch, max_k, max_blocks, ps) if ps else packed_tiles_per_head(batch, total_k)
    return hkv * tiles * 128 * 128 + 256


def packed_regions(cu, total_k, max_k):
    """[(first tile, tiles)] of every sequence of a packed call inside one head's part of the workspace
    (csrc/fa_fp8_inputs.hip, fp8in_tile_start: floor(start / 128) + b)"""
    out = []
    for b in range(len(cu) - 1):
        start, n = seq_span(cu, b, total_k, max_k)
        out.append((start // 128 + b, (n + 127) // 128))
    return out


def paged_regions(cu, max_k, max_blocks, ps):
    cap = paged_cap(max_k, max_blocks, ps)
    nt_seq = (cap + 127) // 128
    return [(b * nt_seq, (paged_len(cu, b, cap) + 127) // 128) for b in range(len(cu) - 1)]


def piece(key, nk, ps, table_row, num_blocks):
    """The descriptor of the 1-KiB K piece that starts at key `key` (a multiple of 8) of a sequence of nk keys
    (fwd_fp8in_varlen_kernel, `stage`): (slot read from the table, page, first row inside the page, rows = num_records / row bytes).
    rows == 0: the piece lands as zeros (past the end, or a page outside the pool)."""
    assert key % 8 == 0 and ps % 16 == 0
    last = max(nk - 1, 0) // ps
    slot = min(key // ps, last)
    page = int(table_row[slot])
    rows = min(8, nk - key)
    ok = rows > 0 and 0 <= page < num_blocks
    return slot, page, key - slot * ps, rows if ok else 0


def stage_tile(t, nk, ps, table_row, pool):
    """(128, d) bytes of K tile t of a sequence staged piece by piece through `piece` from pool (num_blocks, ps, d), and the set of
    table slots read"""
    out = torch.zeros((128,) + tuple(pool.shape[2:]), dtype=pool.dtype)
    slots = set()
    for pc in range(16):
        key = 128 * t + 8 * pc
        slot, page, row, rows = piece(key, nk, ps, table_row, pool.shape[0])
        slots.add(slot)
        if rows:
            out[8 * pc:8 * pc + rows] = pool[page, row:row + rows]
    return out, slots


def gather(pool, table_row, nk, ps):
    """(nk, ...) the keys of a sequence through its table row; a page outside the pool reads as zeros"""
    out = torch.zeros((nk,) + tuple(pool.shape[2:]), dtype=pool.dtype)
    for t in range(nk):
        page = int(table_row[t // ps])
        if 0 <= page < pool.shape[0]:
            out[t] = pool[page, t % ps]
    return out


# ---- the builders of the GPU tests (CPU tensors)

def codes(shape, g):
    """finite e4m3 codes of unit normals"""
    return torch.randn(shape, generator=g).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def descales(batch, hkv, g):
    """three (batch, hkv) float32 descales in [0.25, 4] with odd mantissas"""
    out = []
    for _ in range(3):
        x = (0.25 * 16.0 ** torch.rand((batch, hkv), generator=g)).float().contiguous()
        out.append((x.view(torch.int32) | 1).view(torch.float32).clamp(0.25, 4.0))
    return out


def build_paged(seqs, hq, hkv, ps, table, seed):
    """A paged call: dict with q8 (total_q, hq, 128), the pools pool_k / pool_v (num_blocks, ps, hkv, 128) uint8, block_table
    (B, max_blocks) int32 whose entries past a sequence's last page hold garbage, cu_q, cu_k, the three descales, and per sequence
    the gathered tokens k8[b], v8[b] (len_k, hkv, 128).  Pool bytes no live token owns are 0x7F (e4m3 NaN)."""
    g = torch.Generator().manual_seed(seed)
    B = len(seqs)
    need = [(lk + ps - 1) // ps for _lq, lk in seqs]
    max_blocks = max(need) + 2
    num_blocks = sum(need) + 3
    perm = torch.randperm(num_blocks, generator=g).tolist()
    bt = torch.randint(-5, num_blocks + 5, (B, max_blocks), generator=g, dtype=torch.int32)   # garbage past the live entries
    for b in range(B):
        for s in range(need[b]):
            bt[b, s] = perm.pop()
    if table == "shared":
        users = [b for b in range(B) if need[b] > 0]
        bt[users[-1], 0] = bt[users[0], 0]
    pool_k, pool_v = codes((num_blocks, ps, hkv, D), g), codes((num_blocks, ps, hkv, D), g)
    live = torch.zeros((num_blocks, ps), dtype=torch.bool)
    for b, (_lq, lk) in enumerate(seqs):
        for t in range(lk):
            live[int(bt[b, t // ps]), t % ps] = True
    pool_k[~live] = SENTINEL
    pool_v[~live] = SENTINEL
    k8 = [gather(pool_k, bt[b], lk, ps) for b, (_lq, lk) in enumerate(seqs)]
    v8 = [gather(pool_v, bt[b], lk, ps) for b, (_lq, lk) in enumerate(seqs)]
    lq = [s[0] for s in seqs]
    cu_q = torch.tensor([0] + torch.tensor(lq).cumsum(0).tolist(), dtype=torch.int32)
    base = 1000                                                                                 # (absolute offsets mean nothing for a pool)
    cu_k = torch.tensor([base] + [base + x for x in torch.tensor([s[1] for s in seqs]).cumsum(0).tolist()], dtype=torch.int32)
    qd, kd, vd = descales(B, hkv, g)
    return dict(seqs=tuple(seqs), hq=hq, hkv=hkv, ps=ps, q8=codes((sum(lq), hq, D), g), pool_k=pool_k, pool_v=pool_v, block_table=bt,
                cu_q=cu_q, cu_k=cu_k, q_descale=qd, k_descale=kd, v_descale=vd, k8=k8, v8=v8, max_q=max(lq),
                max_k=max(s[1] for s in seqs), strided=table == "strided")


def packed_kv(call):
    """(k8, v8 (total_k, hkv, 128), cu_k) of the packed call on the same tokens"""
    k8, v8 = torch.cat(call["k8"]), torch.cat(call["v8"])
    cu_k = torch.tensor([0] + torch.tensor([s[1] for s in call["seqs"]]).cumsum(0).tolist(), dtype=torch.int32)
    return k8, v8, cu_k


def padded_call(call, b, causal, dtype):
    """sequence b alone as the dict tests/fp8_inputs_ref.py takes (B = 1)"""
    lq, lk = call["seqs"][b]
    qs = int(call["cu_q"][b])
    return dict(B=1, hq=call["hq"], hkv=call["hkv"], nq=lq, nk=lk, causal=causal, dtype=dtype, scale=D ** -0.5,
                q8=call["q8"][qs:qs + lq].transpose(0, 1)[None].contiguous(), k8=call["k8"][b].transpose(0, 1)[None].contiguous(),
                v8=call["v8"][b].transpose(0, 1)[None].contiguous(),
                **{n: call[n][b:b + 1] for n in ("q_descale", "k_descale", "v_descale")})
