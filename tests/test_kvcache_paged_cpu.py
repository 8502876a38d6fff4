"""CPU: the paged KV cache, cache_batch_idx and cache_leftpad of KV-cache decoding (include/fa_mi355x.h:
fa_ex_forward_kvcache_paged) — declared, exported, every host-side validation before any HIP call, all-null equal to
fa_ex_forward_kvcache, the Python wrappers' checks, and a model of token -> (page, slot) -> element offset."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_kvcache_cpu import BAD, BASE, ORDER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

# the arguments fa_ex_forward_kvcache_paged adds, between num_splits and the workspace
EXTRA = ("table", "trs", "nblk", "ps", "mb", "bidx", "bcache", "leftpad")
NONE = dict(table=None, trs=0, nblk=0, ps=0, mb=0, bidx=None, bcache=0, leftpad=None)
PORDER = ORDER[:ORDER.index("ws")] + EXTRA + ("ws", "wsb")
# a paged call: 9 pages of 16 tokens, 4 a sequence (capacity 64); the cache "batch" strides are page strides
PAGED = dict(table=P, trs=4, nblk=9, ps=16, mb=4, kcb=16 * 128, vcb=16 * 128)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **NONE)
    a.update(kw)
    rc = ext._lib.fa_ex_forward_kvcache_paged(*[a[n] for n in PORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def _old(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **kw)
    rc = ext._lib.fa_ex_forward_kvcache(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbol():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bfa_ex_forward_kvcache_paged\s*\(", src)
    assert hasattr(ctypes.CDLL(ext.LIBRARY_PATH), "fa_ex_forward_kvcache_paged")
    assert "fa_ex_forward_kvcache_paged" in ext.EXPORTED_C_SYMBOLS


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_all_null_answers_as_the_old_entry_point(kw, what):
    rc, msg = _call(**kw)
    rc0, msg0 = _old(**kw)
    assert rc == rc0 == INVALID_ARGUMENT and what in msg
    assert msg == msg0.replace("fa_ex_forward_kvcache:", "fa_ex_forward_kvcache_paged:")


def test_all_null_reaches_the_null_pointer_check():
    rc, msg = _call(o=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg


PAGED_BAD = [
    (dict(ps=0), INVALID_ARGUMENT, "page_block_size"), (dict(ps=-16), INVALID_ARGUMENT, "page_block_size"),
    (dict(ps=8), INVALID_ARGUMENT, "page_block_size"), (dict(ps=24), INVALID_ARGUMENT, "page_block_size"),
    (dict(nblk=0), INVALID_ARGUMENT, "num_blocks"), (dict(nblk=-3), INVALID_ARGUMENT, "num_blocks"),
    (dict(mb=0, trs=4), INVALID_ARGUMENT, "max_blocks_per_seq"),
    (dict(mb=2 ** 24 + 1, trs=2 ** 24 + 1), UNSUPPORTED, "beyond 2^28"),          # capacity 2^28 + 16
    (dict(ps=48, mb=(2 ** 28) // 48 + 1, trs=2 ** 27, kcb=48 * 128, vcb=48 * 128), UNSUPPORTED, "beyond 2^28"),
    (dict(table=ctypes.c_void_p(4098)), INVALID_ARGUMENT, "4-byte aligned"),
    (dict(trs=3), INVALID_ARGUMENT, "block_table_row_stride"), (dict(trs=0), INVALID_ARGUMENT, "block_table_row_stride"),
    (dict(bidx=P, bcache=2), INVALID_ARGUMENT, "cannot be combined"), (dict(leftpad=P), INVALID_ARGUMENT, "cannot be combined"),
    # strides as for caches: token stride >= H_kv d; page stride >= (ps - 1) token stride + H_kv d; multiples of 8
    (dict(kct=64), INVALID_ARGUMENT, "strides of k_cache"), (dict(vcb=15 * 128), INVALID_ARGUMENT, "strides of v_cache"),
    (dict(kcb=16 * 128 + 4), INVALID_ARGUMENT, "multiples of 8"),
    # a page spanning 2^31 bytes or more: 16 tokens, the span is 15 token strides + 128 elements of 2 bytes
    (dict(kct=2 ** 27, kcb=2 ** 31), UNSUPPORTED, "beyond 32-bit offsets"),
    (dict(vct=2 ** 26 + 2 ** 23, vcb=2 ** 31), UNSUPPORTED, "beyond 32-bit offsets"),
    (dict(nnew=65), INVALID_ARGUMENT, "seqlen_new"),                                # above the capacity 4 * 16
]


@pytest.mark.parametrize("kw,code,what", PAGED_BAD, ids=[str(i) for i in range(len(PAGED_BAD))])
def test_paged_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _call(**dict(PAGED, **kw), cap=0)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_ex_forward_kvcache_paged:"), (kw, msg)


def test_valid_paged_arguments_reach_the_null_pointer_check():
    # cache_len is ignored with a table: 0, the capacity and nonsense all pass
    for cap in (0, 64, -5, 2 ** 40):
        rc, msg = _call(**PAGED, cap=cap, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg
    # ps not a power of two; one page only (its stride is free); a padded table row; pool.unbind(1) strides
    for kw in (dict(ps=48, kcb=48 * 128, vcb=48 * 128), dict(nblk=1, kcb=0, vcb=0), dict(trs=100),
               dict(kcb=2 * 16 * 128, vcb=2 * 16 * 128), dict(kct=2 ** 26, kcb=2 ** 30)):   # the last: a page just below 2^31 bytes
        rc, msg = _call(**dict(PAGED, **kw), o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
    # the capacity bounds seqlen_new and sizes the num_splits = 0 rule: 2^28 tokens is accepted
    rc, msg = _call(**dict(PAGED, mb=2 ** 24, trs=2 ** 24), o=None, splits=1)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg
    # window bounds canonicalise against the capacity
    rc, msg = _call(**PAGED, wl=2 ** 40, wr=2 ** 62, o=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg


def test_table_integers_must_be_zero_without_a_table():
    for kw in (dict(trs=4), dict(nblk=9), dict(ps=16), dict(mb=4)):
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and "without block_table" in msg, (kw, msg)


def test_cache_batch_idx_and_leftpad_arguments():
    for kw, what in ((dict(bidx=P, bcache=0), "cache_batch"), (dict(bidx=P, bcache=-1), "cache_batch"), (dict(bcache=3), "cache_batch"),
                     (dict(bidx=ctypes.c_void_p(4098), bcache=2), "4-byte aligned"),
                     (dict(leftpad=ctypes.c_void_p(4097)), "4-byte aligned"),
                     # B_cache = 3 rows need the batch stride even with batch = 1
                     (dict(b=1, bidx=P, bcache=3, kcb=0), "strides of k_cache")):
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and what in msg, (kw, msg)
    for kw in (dict(bidx=P, bcache=5), dict(bidx=P, bcache=1), dict(leftpad=P), dict(bidx=P, bcache=2, leftpad=P),
               dict(b=1, kcb=0, vcb=0, leftpad=P)):
        rc, msg = _call(**kw, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)


def test_python_wrapper_rejections():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    q = torch.zeros((2, 1, 4, 64), dtype=torch.bfloat16)
    kc = torch.zeros((2, 16, 2, 64), dtype=torch.bfloat16)
    for name in ("block_table", "cache_batch_idx", "cache_leftpad"):
        for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int64), [0, 1], 3):
            with pytest.raises(NotImplementedError, match=name + r" of dtype .* \(int32 tensor expected\)"):
                flash_attn_with_kvcache(q, kc, kc, **{name: bad})
    for name in ("rotary_cos", "rotary_sin"):
        with pytest.raises(NotImplementedError, match=name):
            flash_attn_with_kvcache(q, kc, kc, **{name: torch.zeros(1)})

    class FakeCuda(torch.Tensor):   # the wrapper's checks run before anything touches the device
        @property
        def is_cuda(self):
            return True

    fq, fk = q.as_subclass(FakeCuda), kc.as_subclass(FakeCuda)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)   # noqa: E731
    # wrong shapes of int32 tensors: RuntimeError, through flash_attn_with_kvcache too
    for kw in (dict(block_table=i32(2)), dict(block_table=i32(3, 4)), dict(block_table=i32(2, 0)), dict(cache_batch_idx=i32(3)),
               dict(cache_batch_idx=i32(2, 1)), dict(cache_leftpad=i32(1)), dict(cache_leftpad=i32(2, 2))):
        with pytest.raises(RuntimeError, match=next(iter(kw)) + " must be an int32"):
            ext.ex_kvcache_forward(fq, fk, fk, **kw)
        with pytest.raises(RuntimeError, match=next(iter(kw)) + " must be an int32"):
            flash_attn_with_kvcache(fq, fk, fk, **kw)
    with pytest.raises(RuntimeError, match="must be an int32"):
        ext.ex_kvcache_forward(fq, fk, fk, block_table=torch.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="on q's device"):
        ext.ex_kvcache_forward(fq, fk, fk, cache_leftpad=i32(2).to("meta"))
    for other in ("cache_batch_idx", "cache_leftpad"):
        with pytest.raises(RuntimeError, match="cannot be combined"):
            ext.ex_kvcache_forward(fq, fk, fk, block_table=i32(2, 4), **{other: i32(2)})
    # a page size that is not a multiple of 16; pools whose shapes disagree; a pool view that would need a copy
    pool24 = torch.zeros((5, 24, 2, 64), dtype=torch.bfloat16).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ext.ex_kvcache_forward(fq, pool24, pool24, block_table=i32(2, 4))
    pool = torch.zeros((5, 16, 2, 64), dtype=torch.bfloat16).as_subclass(FakeCuda)
    pool7 = torch.zeros((7, 16, 2, 64), dtype=torch.bfloat16).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="num_blocks, page_block_size"):
        ext.ex_kvcache_forward(fq, pool, pool7, block_table=i32(2, 4))
    strided = torch.zeros((5, 16, 2, 128), dtype=torch.bfloat16)[..., ::2].as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="never copied"):
        ext.ex_kvcache_forward(fq, strided, pool, block_table=i32(2, 4))
    heads_apart = torch.zeros((5, 16, 64, 2), dtype=torch.bfloat16).transpose(2, 3).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="never copied"):
        ext.ex_kvcache_forward(fq, pool, heads_apart, block_table=i32(2, 4))
    # without cache_batch_idx the cache's batch dim must be q's
    with pytest.raises(RuntimeError, match=r"\(B, cache_len, H_kv, d\)"):
        ext.ex_kvcache_forward(fq, pool, pool)
    with pytest.raises(RuntimeError, match=r"\(B, cache_len, H_kv, d\)"):
        ext.ex_kvcache_forward(fq, pool, pool, cache_leftpad=i32(2))


# ---- model of the documented addressing: token t of sequence b -> pool[table[b, t // ps], t % ps]
def element_offset(table_row, t, ps, page_stride, token_stride, head, d, i):
    return table_row[t // ps] * page_stride + (t % ps) * token_stride + head * d + i


def tile_walk(kbeg, kend, ps):
    """csrc/fa_decode.hip's walk: the page j0 and slot s0 of each 32-key tile's first key are carried from tile to tile, and a
    lane's key kbeg + 32 n + l is at most two pages further on.  Yields (key, page index, slot)."""
    j0, s0 = divmod(kbeg, ps)
    for k0 in range(kbeg, kend, 32):
        for lane in range(32):
            j, sl = j0, s0 + lane
            if sl >= ps:
                sl -= ps
                j += 1
            if sl >= ps:
                sl -= ps
                j += 1
            if k0 + lane < kend:
                yield k0 + lane, j, sl
        s0 += 32
        for _ in range(2):
            if s0 >= ps:
                s0 -= ps
                j0 += 1
        assert 0 <= s0 < ps


@pytest.mark.parametrize("ps", [16, 48, 80, 256, 272])
def test_token_to_page_slot_offset_model(ps):
    hkv, d = 2, 64
    nblk, mb = 11, 5
    g = torch.Generator().manual_seed(ps)
    for page_stride, token_stride, base in ((ps * hkv * d, hkv * d, 0),                       # a dense pool
                                            (2 * ps * hkv * d, hkv * d, ps * hkv * d),        # the V half of pool.unbind(1)
                                            (ps * 3 * hkv * d + 64, 3 * hkv * d, 8)):         # padded tokens and pages
        storage = torch.arange(base + nblk * page_stride, dtype=torch.int64)
        pool = storage.as_strided((nblk, ps, hkv, d), (page_stride, token_stride, d, 1), base)
        table = torch.randperm(nblk, generator=g)[:mb].tolist()
        for t in (0, 1, ps - 1, ps, ps + 1, 2 * ps - 1, 2 * ps, mb * ps - 1):
            for head, i in ((0, 0), (1, 5), (hkv - 1, d - 1)):
                off = element_offset(table, t, ps, page_stride, token_stride, head, d, i)
                assert int(pool[table[t // ps], t % ps, head, i]) == base + off
                assert 0 <= (t % ps) * token_stride + head * d + i < page_stride   # inside the page: the 32-bit part
    # the kernel's tile walk, from any band start (tiles are cut from the band's first key, not from a page boundary)
    for kbeg in (0, 1, 15, 16, 17, ps - 1, ps, ps + 5, 3 * ps - 7):
        for kend in (kbeg, kbeg + 1, kbeg + 31, kbeg + 32, kbeg + 33, kbeg + 5 * ps + 3):
            seen = list(tile_walk(kbeg, kend, ps))
            assert [k for k, _, _ in seen] == list(range(kbeg, kend))
            assert all((j, sl) == divmod(k, ps) for k, j, sl in seen)
