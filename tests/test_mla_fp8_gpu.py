"""GPU: the packed 8-bit latent cache (mla_fp8_pack_cache, flash_mla_with_kvcache(is_fp8_kvcache=True); fa_mla_fp8_pack,
fa_mla_fp8_forward).  The append byte for byte against tests/mla_fp8_ref.pack_rows / scatter_rows; the decode bit for bit against
the 16-bit calls (flash_attn_with_kvcache(qv=), flash_mla_sparse_attn) on the pool that unpack_rows gives, with the same table,
lengths and num_splits, and within the tolerances of tests/test_kvcache_gpu.py::check of the fp64 references on those values;
append + decode on one stream; graph replay; the 16-bit route of flash_mla_with_kvcache.  Every quantised value has a magnitude
in [2^-6, 8] (or is an exact zero), so no product of the contract is fp32-subnormal.  At most 80 packed rows and 200 cached tokens."""
import functools

import pytest
import torch

from tests import mla_fp8_ref as ref
from tests.mla_ref import mla_reference
from tests.mla_sparse_ref import mla_sparse_reference
from tests.test_kvcache_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SCALE = 576 ** -0.5
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LENS = (0, 1, 33, 100)


def fm(*args, **kw):
    from common.attention_ex import flash_mla_with_kvcache

    return flash_mla_with_kvcache(*args, **kw)


def qv_call(q, pool16, table, lens, **kw):
    from common.attention_ex import flash_attn_with_kvcache

    return flash_attn_with_kvcache(q[..., 512:], pool16[..., 512:], pool16[..., :512], cache_seqlens=lens, block_table=table,
                                   softmax_scale=SCALE, return_softmax_lse=True, qv=q[..., :512], **kw)


def sparse_call(q, pool16, ix, table, lens, **kw):
    from common.attention_ex import flash_mla_sparse_attn

    return flash_mla_sparse_attn(q[..., 512:], q[..., :512], pool16[..., 512:], pool16[..., :512], ix, cache_seqlens=lens,
                                 block_table=table, softmax_scale=SCALE, return_softmax_lse=True, **kw)


def values(shape, seed):
    """bf16, magnitudes 2^u with u uniform in [-6, 3] (so every e4m3 binade of a tile is hit), random signs, |x| in [2^-6, 8]"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(shape, generator=g) * 9 - 6)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    x = (mag * sign).to(BF16)
    assert (x.abs() >= 2 ** -6).all() and (x.abs() <= 8).all()
    return x


def special_tiles(lat):
    """(.., 512) latent rows: an all-zero tile in the first row, a tile whose amax is 7 = 448 * 2^-6 in the last"""
    flat = lat.reshape(-1, 512)
    flat[0, 128:256] = 0
    flat[-1, 256:384] = flat[-1, 256:384].clamp(-3.5, 3.5)
    flat[-1, 300] = 7.0
    return lat


@functools.lru_cache(maxsize=None)
def pools(ps):
    """CPU: a packed pool (wide: tokens 672 bytes apart, the 16 bytes between them 0xA5), the same pool with 656-byte tokens, the
    bf16 pool the read contract gives, and a (4, mb) table whose rows share pages, with one page outside the pool inside sequence 3's
    length and a negative one inside sequence 2's.  ps = 16: 9 pages, capacity 112; ps = 48: 4 pages, capacity 144."""
    nblk, mb = (9, 7) if ps == 16 else (4, 3)
    lat = special_tiles(values((nblk, ps, 1, 512), ps))
    rows = ref.pack_rows(lat, values((nblk, ps, 1, 64), ps + 1), scale_pow2=(ps == 48))
    wide = torch.full((nblk, ps, 1, 672), 0xA5, dtype=torch.uint8)
    wide[..., :656] = rows
    g = torch.Generator().manual_seed(ps)
    table = torch.stack([torch.randperm(nblk, generator=g).repeat(3)[:mb] for _ in range(4)]).to(torch.int32)
    table[3, 1] = nblk + 5
    table[2, 0] = -1
    return wide, rows, ref.unpack_pool(rows), table


@functools.lru_cache(maxsize=None)
def queries(hq, nq):
    g = torch.Generator().manual_seed(100 * hq + nq)
    return torch.randn((4, nq, hq, 576), generator=g).to(BF16)


@functools.lru_cache(maxsize=None)
def dense_expected(ps, hq, nq, lens, causal):
    _wide, _rows, pool16, table = pools(ps)
    q = queries(hq, nq)
    return mla_reference(q[..., 512:], q[..., :512], pool16[..., 512:], pool16[..., :512], torch.tensor(lens, dtype=torch.int32), causal,
                         (-1, -1), SCALE, table)


def make_lists(lens, nq, topk, cap, seed, causal):
    """(4, Nq, topk) int32: visible tokens at random list positions, one of them named twice, -1 padding, and entries that are no
    keys: the length itself, a position past it, above the causal bound of the row (its own last visible token + 1), INT_MIN,
    INT_MAX, -7"""
    g = torch.Generator().manual_seed(seed)
    ix = torch.full((4, nq, topk), -1, dtype=torch.int64)
    for b in range(4):
        for i in range(nq):
            pos = torch.randperm(topk, generator=g).tolist()
            if lens[b] == 0:
                ix[b, i] = torch.randint(0, cap, (topk,), generator=g)
                continue
            n = int(torch.randint(2, topk - 7, (1,), generator=g))
            ix[b, i, pos[:n]] = torch.randint(0, lens[b], (n,), generator=g)
            ix[b, i, pos[1]] = ix[b, i, pos[0]]
            junk = [lens[b], int(torch.randint(lens[b], cap + 50, (1,), generator=g)), INT_MIN, INT_MAX, -7, lens[b] - 1]
            if causal and i < nq - 1:
                junk[-1] = max(lens[b] - nq + i + 1, 0)     # the first token above this row's bound (below the length: visible without causal)
            for p, val in zip(pos[n:], junk):
                ix[b, i, p] = val
    return ix.to(torch.int32)


# ---- 1. the append, byte for byte

def _new_tokens(nnew, seed):
    new = torch.cat([special_tiles(values((3, nnew, 512), seed)), values((3, nnew, 64), seed + 1)], dim=-1)
    return new.contiguous()


PACK_TABLE = ((0, 1), (2, 3), (4, 5))      # 6 pages of 16 tokens, 2 a sequence: capacity 32


def _pack_and_compare(new, lens, table, pow2, sliced=True, wide=True):
    from common.attention_ex import mla_fp8_pack_cache

    pool = torch.full((6, 16, 1, 672 if wide else 656), 0xA5, dtype=torch.uint8)
    lens_t, table_t = torch.tensor(lens, dtype=torch.int32), torch.tensor(table, dtype=torch.int32)
    want, dropped = ref.scatter_rows(pool, ref.pack_rows(new[..., :512], new[..., 512:], pow2), lens_t, table_t)
    dpool, dnew = pool.to(DEV), new.to(DEV)
    lat, rope = (dnew[..., :512], dnew[..., 512:]) if sliced else (dnew[..., :512].contiguous(), dnew[..., 512:].contiguous())
    mla_fp8_pack_cache(lat, rope, dpool[..., :656], lens_t.to(DEV), table_t.to(DEV), scale_pow2=pow2)
    got = dpool.cpu()
    bad = (got != want).any(-1).nonzero().tolist()
    assert not bad, bad[:8]
    assert torch.equal(got, want)                      # every byte of a row not written, and past a token's 656, is still 0xA5
    return want, dropped


@pytest.mark.parametrize("sliced", (True, False), ids=("one_tensor", "two_tensors"))
@pytest.mark.parametrize("pow2", (False, True), ids=("amax", "pow2"))
@pytest.mark.parametrize("nnew", (1, 5))
def test_pack_matches_the_reference_byte_for_byte(nnew, pow2, sliced):
    """lengths before the append 0, 15 (five tokens cross the 16-token page) and 17; an all-zero tile and a tile with amax = 448 *
    2^-6 among the new tokens; 672-byte token stride, so the 16 bytes behind every token must stay"""
    new = _new_tokens(nnew, 10 * nnew + pow2)
    want, dropped = _pack_and_compare(new, (0, 15, 17), PACK_TABLE, pow2, sliced)
    assert not dropped and int((want[..., 0, :656] != 0xA5).any(-1).sum()) == 3 * nnew
    # the quantised values come back within 2^-4 of the tile's amax, and within the exact bound of the format derived in
    # tests/test_mla_fp8_cpu.py::test_round_trip_error_bound: 1 / 28 (scale_pow2: 1 / 17) for the quantiser + 2^-9 for the bf16 read
    back, rope = ref.unpack_rows(want[0, :nnew, 0])
    assert torch.equal(rope.view(torch.int16), new[0, :, 512:].view(torch.int16))
    x = new[0, :, :512].double().reshape(nnew, 4, 128)
    err, amax = (back.double().reshape(nnew, 4, 128) - x).abs(), x.abs().amax(-1, keepdim=True)
    assert (err <= 2 ** -4 * amax).all()
    assert (err <= ((1 / 17 if pow2 else 1 / 28) + 2 ** -9 + 2 ** -20) * amax).all()


@pytest.mark.parametrize("lens,table,n_dropped", (
    ((0, 15, 17), ((0, 1), (2, -1), (4, 5)), 4),          # sequence 1: token 15 is written, 16 .. 19 sit on page -1
    ((0, 15, 17), ((6, 1), (2, 3), (4, 5)), 5),           # sequence 0: page 6 of a pool of 6
    ((0, 15, 30), ((0, 1), (2, 3), (4, 5)), 3),           # sequence 2: positions 30, 31 are written, 32 .. 34 are past the capacity
    ((-1, 32, 2 ** 31 - 3), ((0, 1), (2, 3), (4, 5)), 15),    # a negative length, a full table, a length whose sum leaves int32
    ((0, 15, 17), ((INT_MIN, 1), (2, INT_MAX), (4, 5)), 9),
), ids=("page_-1", "page_past_the_pool", "past_the_capacity", "bad_lengths", "int_extremes"))
def test_pack_drops_exactly_the_tokens_without_a_slot(lens, table, n_dropped):
    new = _new_tokens(5, 77)
    _want, dropped = _pack_and_compare(new, lens, table, False, wide=False)
    assert len(dropped) == n_dropped


# ---- 2. and 4. dense decode: the 16-bit call's bits, and the fp64 reference

# H_q x Nq = 1, 16, 17 and 80 packed rows: one wave with a partial and an exact tile, two waves, four waves (the prefetch) over two
# workgroups of rows
DENSE = [(1, 1, 16), (16, 1, 16), (17, 1, 48), (40, 2, 16), (80, 1, 48)]


@pytest.mark.parametrize("hq,nq,ps", DENSE, ids=[f"hq{h}_nq{n}_ps{p}" for h, n, p in DENSE])
def test_dense_decode_has_the_bits_of_the_16_bit_call(hq, nq, ps):
    wide, rows, pool16, table = pools(ps)
    q, d8, d16, dtab = queries(hq, nq).to(DEV), rows.to(DEV), pool16.to(DEV), table.to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    ro, rlse = dense_expected(ps, hq, nq, LENS, False)
    for splits in (1, 2, 5, 0):
        o, lse = fm(q, d8, dtab, lens, is_fp8_kvcache=True, num_splits=splits)
        assert o.shape == (4, nq, hq, 512) and o.dtype == BF16 and lse.shape == (4, hq, nq) and lse.dtype == torch.float32
        o16, lse16 = qv_call(q, d16, dtab, lens, num_splits=splits)
        assert torch.equal(o, o16) and torch.equal(lse, lse16), splits
        check(o, lse, ro, rlse, BF16)
        o2, lse2 = fm(q, d8, dtab, lens, is_fp8_kvcache=True, num_splits=splits)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), splits
    assert (o[0] == 0).all() and (lse[0] == -float("inf")).all() and torch.isfinite(lse[1:]).all()
    # tokens 672 bytes apart, and the pool as torch.float8_e4m3fn: the same bits
    o3, lse3 = fm(q, wide.to(DEV)[..., :656].view(torch.float8_e4m3fn), dtab, lens, is_fp8_kvcache=True)
    assert torch.equal(o, o3) and torch.equal(lse, lse3)


@pytest.mark.parametrize("hq,ps", ((5, 16), (20, 48)), ids=("hq5_ps16", "hq20_ps48"))
def test_dense_causal_with_rows_without_a_key_and_lengths_beyond_the_capacity(hq, ps):
    """causal with Nq = 3: length 0 has no key for any row, length 1 none for rows 0 and 1; a length beyond the capacity is the
    capacity"""
    nq = 3
    _wide, rows, pool16, table = pools(ps)
    cap = table.shape[1] * ps
    q, d8, d16, dtab = queries(hq, nq).to(DEV), rows.to(DEV), pool16.to(DEV), table.to(DEV)
    for lens, clamped in ((LENS, LENS), ((1, 2, 10 ** 6, INT_MAX), (1, 2, cap, cap))):
        dl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        ro, rlse = dense_expected(ps, hq, nq, clamped, True)
        for splits in (0, 2):
            o, lse = fm(q, d8, dtab, dl, is_fp8_kvcache=True, causal=True, num_splits=splits)
            o16, lse16 = qv_call(q, d16, dtab, dl, causal=True, num_splits=splits)
            assert torch.equal(o, o16) and torch.equal(lse, lse16), (lens, splits)
            check(o, lse, ro, rlse, BF16)
    o, lse = fm(q, d8, dtab, torch.tensor(LENS, dtype=torch.int32, device=DEV), is_fp8_kvcache=True, causal=True)
    assert (lse[0] == -float("inf")).all() and (lse[1, :, :2] == -float("inf")).all() and torch.isfinite(lse[1, :, 2]).all()
    assert (o[1, :2] == 0).all()
    # cache_seqlens=None is the capacity
    o, lse = fm(q, d8, dtab, None, is_fp8_kvcache=True, causal=True)
    o16, lse16 = qv_call(q, d16, dtab, None, causal=True)
    assert torch.equal(o, o16) and torch.equal(lse, lse16)


# ---- 3. and 4. decode over a list: flash_mla_sparse_attn's bits, and the fp64 reference

SPARSE = [(1, 1, 16, False), (16, 1, 48, False), (17, 2, 16, True), (40, 2, 48, True), (80, 1, 16, False)]


@pytest.mark.parametrize("hq,nq,ps,causal", SPARSE, ids=[f"hq{h}_nq{n}_ps{p}{'_causal' if c else ''}" for h, n, p, c in SPARSE])
def test_sparse_decode_has_the_bits_of_the_16_bit_call(hq, nq, ps, causal):
    wide, rows, pool16, table = pools(ps)
    cap = table.shape[1] * ps
    ix = make_lists(LENS, nq, 40, cap, 7 * hq + ps, causal)
    q = queries(hq, nq)
    sl = torch.tensor(LENS, dtype=torch.int32)
    ro, rlse = mla_sparse_reference(q[..., 512:], q[..., :512], pool16[..., 512:], pool16[..., :512], ix, sl, causal, SCALE, table)
    dq, d8, d16, dtab, dix, dl = q.to(DEV), rows.to(DEV), pool16.to(DEV), table.to(DEV), ix.to(DEV), sl.to(DEV)
    for splits in (1, 2, 5, 0):
        o, lse = fm(dq, d8, dtab, dl, is_fp8_kvcache=True, indices=dix, causal=causal, num_splits=splits)
        o16, lse16 = sparse_call(dq, d16, dix, dtab, dl, causal=causal, num_splits=splits)
        assert torch.equal(o, o16) and torch.equal(lse, lse16), splits
        check(o, lse, ro, rlse, BF16)
        o2, lse2 = fm(dq, d8, dtab, dl, is_fp8_kvcache=True, indices=dix, causal=causal, num_splits=splits)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), splits
    assert (o[0] == 0).all() and (lse[0] == -float("inf")).all() and torch.isfinite(lse[3]).any()
    if causal:   # the bound cuts something: an entry above it is visible without it
        o4, _ = fm(dq, d8, dtab, dl, is_fp8_kvcache=True, indices=dix)
        assert not torch.equal(o[3, 0], o4[3, 0])
    o3, lse3 = fm(dq, wide.to(DEV)[..., :656], dtab, dl, is_fp8_kvcache=True, indices=dix, causal=causal)
    assert torch.equal(o, o3) and torch.equal(lse, lse3)
    # topk = 0: no key
    empty = torch.empty((4, nq, 0), dtype=torch.int32, device=DEV)
    o0, lse0 = fm(dq, d8, dtab, dl, is_fp8_kvcache=True, indices=empty)
    o16, lse16 = sparse_call(dq, d16, empty, dtab, dl)
    assert (o0 == 0).all() and (lse0 == -float("inf")).all() and torch.equal(o0, o16) and torch.equal(lse0, lse16)


# ---- 5. append and decode on one stream

def own_pages(table, before, nnew, ps):
    """the table with a page of its own under every position that an append of nnew tokens at the lengths `before` writes (two
    tokens on one slot are undefined); the other entries, shared and invalid pages among them, stay"""
    t, taken, nxt = table.clone(), set(), 0
    for b, ln in enumerate(before):
        for pos in range(ln, ln + nnew):
            j = pos // ps
            if j < t.shape[1] and (b, j) not in taken:
                taken.add((b, j))
                t[b, j] = nxt
                nxt += 1
    assert nxt <= 9
    return t


@pytest.mark.parametrize("with_lists", (False, True), ids=("dense", "lists"))
def test_pack_then_decode_is_decode_on_the_reference_bytes(with_lists):
    from common.attention_ex import mla_fp8_pack_cache

    hq, nq, ps, nnew = 16, 2, 16, 5
    _wide, rows, _pool16, table = pools(ps)
    before = torch.tensor((0, 15, 33, 110), dtype=torch.int32)
    table = own_pages(table, before.tolist(), nnew, ps)
    new = torch.cat([values((4, nnew, 512), 5), values((4, nnew, 64), 6)], dim=-1)
    want, dropped = ref.scatter_rows(rows, ref.pack_rows(new[..., :512], new[..., 512:]), before, table)
    assert dropped == [(3, 2), (3, 3), (3, 4)]        # positions 112 .. 114 are past the capacity
    after = before + nnew
    ix = make_lists(tuple(after.tolist()), nq, 40, table.shape[1] * ps, 3, True).to(DEV) if with_lists else None
    q, dtab, dbefore, dafter, dnew = queries(hq, nq).to(DEV), table.to(DEV), before.to(DEV), after.to(DEV), new.to(DEV)
    dpool = rows.to(DEV)
    mla_fp8_pack_cache(dnew[..., :512], dnew[..., 512:], dpool, dbefore, dtab)
    o, lse = fm(q, dpool, dtab, dafter, is_fp8_kvcache=True, indices=ix, causal=True)
    assert torch.equal(dpool.cpu(), want)
    o2, lse2 = fm(q, want.to(DEV), dtab, dafter, is_fp8_kvcache=True, indices=ix, causal=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o3, _ = fm(q, rows.to(DEV), dtab, dafter, is_fp8_kvcache=True, indices=ix, causal=True)
    assert not torch.equal(o[1], o3[1])          # the new tokens are seen


# ---- 6. graph replay

def test_graph_replay_with_changed_lengths_tables_and_contents():
    from common.attention_ex import mla_fp8_pack_cache

    hq, nq, ps, nnew = 16, 1, 16, 2
    _wide, rows, _pool16, table = pools(ps)
    q = queries(hq, nq).to(DEV)
    dpool, dtab = rows.to(DEV), own_pages(table, (0, 15, 33, 95), nnew, ps).to(DEV)
    dbefore = torch.tensor((0, 15, 33, 95), dtype=torch.int32, device=DEV)
    dnew = torch.cat([values((4, nnew, 512), 8), values((4, nnew, 64), 9)], dim=-1).to(DEV)

    def step():
        mla_fp8_pack_cache(dnew[..., :512], dnew[..., 512:], dpool, dbefore, dtab)
        return fm(q, dpool, dtab, dbefore + nnew, is_fp8_kvcache=True, causal=True)

    step()   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.Generator().manual_seed(4)
    for seed, lens in ((20, (40, 0, 110, 7)), (30, (111, 64, 1, 16))):     # 110 + 2 and 111 + 2: the last token(s) past the capacity 112
        new_table = torch.stack([torch.randperm(9, generator=g).repeat(3)[:7] for _ in range(4)]).to(torch.int32)
        new_table = own_pages(new_table, lens, nnew, ps)
        new_table[seed // 10 - 2, 5] = 9                                   # a page outside the pool, read as zeros
        new = torch.cat([values((4, nnew, 512), seed), values((4, nnew, 64), seed + 1)], dim=-1)
        start = ref.pack_rows(values((9, ps, 1, 512), seed + 2), values((9, ps, 1, 64), seed + 3))
        before = torch.tensor(lens, dtype=torch.int32)
        dtab.copy_(new_table)
        dnew.copy_(new)
        dpool.copy_(start)
        dbefore.copy_(before)
        q.copy_(torch.randn(q.shape, generator=g).to(BF16))
        graph.replay()
        torch.cuda.synchronize()
        want, _dropped = ref.scatter_rows(start, ref.pack_rows(new[..., :512], new[..., 512:]), before, new_table)
        assert torch.equal(dpool.cpu(), want)
        after = (before + nnew).to(DEV)
        eager = fm(q, want.to(DEV), dtab, after, is_fp8_kvcache=True, causal=True)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        p16 = ref.unpack_pool(want)
        ro, rlse = mla_reference(q.cpu()[..., 512:], q.cpu()[..., :512], p16[..., 512:], p16[..., :512], before + nnew, True, (-1, -1),
                                 SCALE, new_table)
        check(out[0], out[1], ro, rlse, BF16)


# ---- 7. the 16-bit route

@pytest.mark.parametrize("dtype", (BF16, torch.float16), ids=("bf16", "f16"))
def test_the_16_bit_route_is_the_two_existing_calls(dtype):
    hq, nq, ps = 17, 2, 16
    _wide, _rows, pool16, table = pools(ps)
    q, d16, dtab = queries(hq, nq).to(dtype).to(DEV), pool16.to(dtype).to(DEV), table.to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    o, lse = fm(q, d16, dtab, lens, causal=True, num_splits=2)
    o16, lse16 = qv_call(q, d16, dtab, lens, causal=True, num_splits=2)
    assert o.dtype == dtype and torch.equal(o, o16) and torch.equal(lse, lse16)
    ix = make_lists(LENS, nq, 40, 112, 1, True).to(DEV)
    o, lse = fm(q, d16, dtab, lens, indices=ix, causal=True)
    o16, lse16 = sparse_call(q, d16, ix, dtab, lens, causal=True)
    assert torch.equal(o, o16) and torch.equal(lse, lse16)
    # explicit and default scale agree; another scale does not
    o2, _ = fm(q, d16, dtab, lens, indices=ix, causal=True, softmax_scale=SCALE)
    o3, _ = fm(q, d16, dtab, lens, indices=ix, causal=True, softmax_scale=0.11)
    assert torch.equal(o, o2) and not torch.equal(o, o3)
