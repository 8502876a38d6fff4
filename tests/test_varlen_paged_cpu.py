"""CPU: the paged K/V cache of the varlen forward (flash_attention_varlen with block_table; include/fa_mi355x.h:
fa_ex_forward_varlen_paged) — declared and exported, every host-side validation before any HIP call, the Python wrappers'
errors, the test helper's gather / scatter, and a model of the kernel's piece -> page arithmetic."""
import ctypes
import os
import re

import pytest
import torch

from tests.varlen_paged_ref import build_pool, gather, pg_slot, piece_fetches

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

ORDER = ("q", "k", "v", "o", "lse", "cu_q", "cu_k", "batch", "hq", "hkv", "total_q", "total_k", "max_q", "max_k", "d", "dtype", "sq", "sk",
         "sv", "causal", "wl", "wr", "scale", "softcap", "alibi", "abs", "sinks", "sheads", "table", "mb", "nblk", "ps", "kps", "vps")
# 2 sequences, 4 query heads over 2 K/V heads of d = 64, bf16; 9 pages of 16 tokens, 4 a sequence
BASE = dict(q=P, k=P, v=P, o=P, lse=P, cu_q=P, cu_k=P, batch=2, hq=4, hkv=2, total_q=40, total_k=0, max_q=32, max_k=64, d=64, dtype=2,
            sq=256, sk=128, sv=128, causal=1, wl=-1, wr=-1, scale=0.125, softcap=0.0, alibi=None, abs=0, sinks=None, sheads=1, table=P,
            mb=4, nblk=9, ps=16, kps=16 * 128, vps=16 * 128)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **kw)
    rc = ext._lib.fa_ex_forward_varlen_paged(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbol():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bfa_ex_forward_varlen_paged\s*\(", src)
    assert hasattr(ctypes.CDLL(ext.LIBRARY_PATH), "fa_ex_forward_varlen_paged")
    assert "fa_ex_forward_varlen_paged" in ext.EXPORTED_C_SYMBOLS


BAD = [
    (dict(ps=0), "page_block_size"), (dict(ps=8), "page_block_size"), (dict(ps=24), "page_block_size"), (dict(ps=-16), "page_block_size"),
    (dict(table=None), "null block_table"), (dict(table=ctypes.c_void_p(4098)), "4-byte aligned"),
    (dict(nblk=-1), "num_blocks"), (dict(mb=-2), "max_blocks_per_seq"),
    (dict(sk=64), "token strides"), (dict(sv=127), "token strides"), (dict(sq=255), "token strides"),
    (dict(kps=15 * 128), "page strides"), (dict(vps=15 * 128 + 127), "page strides"), (dict(sk=256, kps=16 * 128), "page strides"),
    (dict(cu_k=None), "null cu_seqlens"), (dict(hkv=3), "heads_q"), (dict(wl=-2), "window"), (dict(softcap=-1.0), "softcap"),
    (dict(sinks=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(scale=float("nan")), "softmax_scale"),
]


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_arguments_are_rejected_before_any_hip_call(kw, what):
    rc, msg = _call(**kw)
    assert rc == INVALID_ARGUMENT and what in msg and msg.startswith("fa_ex_forward_varlen_paged:"), (kw, msg)


def test_too_large_pages_are_unsupported():
    for kw in (dict(ps=65536 + 16, kps=(65536 + 16) * 128, vps=(65536 + 16) * 128), dict(sk=2 ** 27, kps=2 ** 31)):
        rc, msg = _call(**kw)
        assert rc == UNSUPPORTED and "page" in msg, (kw, msg)


def test_valid_arguments_reach_the_null_pointer_check_or_return():
    # total_k is not used; one page only: its stride is free; ps no power of two; strided pools (K|V interleaved)
    for kw in (dict(total_k=-5), dict(total_k=2 ** 40), dict(nblk=1, kps=0, vps=0), dict(ps=48, kps=48 * 128, vps=48 * 128),
               dict(sk=128, kps=2 * 16 * 128, sv=128, vps=2 * 16 * 128), dict(wl=2 ** 40, wr=2 ** 62)):
        rc, msg = _call(**kw, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
    # nothing to do: no query token (before any pointer is looked at)
    for kw in (dict(total_q=0), dict(max_q=0)):
        rc, msg = _call(**kw, o=None)
        assert rc == OK, (kw, msg)


def test_python_wrapper_rejections():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_varlen

    bf = torch.bfloat16
    q = torch.zeros((40, 4, 64), dtype=bf)
    pool = torch.zeros((9, 16, 2, 64), dtype=bf)
    cu = torch.tensor([0, 8, 40], dtype=torch.int32)
    table = torch.zeros((2, 4), dtype=torch.int32)
    args = (cu, cu, 32, 64)
    for bad in (torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int64), [[0, 1]], 3):
        with pytest.raises(NotImplementedError, match=r"block_table of dtype .* \(int32 tensor expected\)"):
            flash_attention_varlen(q, pool, pool, *args, block_table=bad)
    with pytest.raises(ValueError, match="dropout_p > 0 is not supported with block_table"):
        flash_attention_varlen(q, pool, pool, *args, dropout_p=0.1, block_table=table)
    for who in range(3):
        t = [x.clone() for x in (q, pool, pool)]
        t[who].requires_grad_(True)
        with pytest.raises(RuntimeError, match="block_table"):
            flash_attention_varlen(*t, *args, block_table=table)
        with torch.no_grad(), pytest.raises(RuntimeError, match="CUDA tensors"):   # grad mode off: on to the device check
            flash_attention_varlen(*t, *args, block_table=table)

    class FakeCuda(torch.Tensor):   # the wrapper's checks run before anything touches the device
        @property
        def is_cuda(self):
            return True

    fq, fpool, fcu, ftab = (t.as_subclass(FakeCuda) for t in (q, pool, cu, table))
    # a pool view that would need a copy: elements of a head apart, heads not adjacent
    strided = torch.zeros((9, 16, 2, 128), dtype=bf)[..., ::2].as_subclass(FakeCuda)
    heads_apart = torch.zeros((9, 16, 64, 2), dtype=bf).transpose(2, 3).as_subclass(FakeCuda)
    for k, v in ((strided, fpool), (fpool, heads_apart)):
        with pytest.raises(ValueError, match="never copied"):
            ext.ex_varlen_forward(fq, k, v, fcu, fcu, 32, 64, True, 0.125, block_table=ftab)
        with pytest.raises(ValueError, match="never copied"):
            flash_attention_varlen(fq, k, v, fcu, fcu, 32, 64, causal=True, block_table=ftab)
    with pytest.raises(ValueError, match="dropout_p"):
        ext.ex_varlen_forward(fq, fpool, fpool, fcu, fcu, 32, 64, True, 0.125, 0.5, block_table=ftab)
    with pytest.raises(NotImplementedError, match="int32 tensor expected"):
        ext.ex_varlen_forward(fq, fpool, fpool, fcu, fcu, 32, 64, True, 0.125, block_table=ftab.long())
    # shapes: a packed k with a table, a page size off the 16 grid, a table of another batch
    with pytest.raises(RuntimeError, match="num_blocks, page_block_size"):
        ext.ex_varlen_forward(fq, fq, fq, fcu, fcu, 32, 64, True, 0.125, block_table=ftab)
    pool24 = torch.zeros((9, 24, 2, 64), dtype=bf).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ext.ex_varlen_forward(fq, pool24, pool24, fcu, fcu, 32, 64, True, 0.125, block_table=ftab)
    with pytest.raises(RuntimeError, match="block_table must be an int32"):
        ext.ex_varlen_forward(fq, fpool, fpool, fcu, fcu, 32, 64, True, 0.125, block_table=torch.zeros((3, 4), dtype=torch.int32).as_subclass(FakeCuda))


@pytest.mark.parametrize("ps", [16, 48, 256])
def test_gather_of_scatter_is_the_identity(ps):
    g = torch.Generator().manual_seed(ps)
    lens = [0, 1, 16, 127, 129, 300]
    ks = [torch.randn((n, 2, 8), generator=g) for n in lens]
    vs = [torch.randn((n, 2, 8), generator=g) for n in lens]
    kp, vp, table = build_pool(ks, vs, ps, spare=3, seed=ps)
    used = table[table >= 0]
    assert used.numel() == sum((n + ps - 1) // ps for n in lens) == len(set(used.tolist())) and kp.shape[0] == used.numel() + 3
    assert sorted(used.tolist()) != used.tolist()   # shuffled
    for b, n in enumerate(lens):
        assert torch.equal(gather(kp, table[b], n, ps), ks[b]) and torch.equal(gather(vp, table[b], n, ps), vs[b])
    # a page outside the pool reads as zeros, on either side of the range
    row = table[5].clone()
    row[0], row[1] = -1, kp.shape[0]
    got = gather(kp, row, 300, ps)
    assert torch.count_nonzero(got[:min(300, 2 * ps)]) == 0 and torch.equal(got[2 * ps:], ks[5][2 * ps:])


@pytest.mark.parametrize("ps", [16, 48, 64, 256, 272, 65536])
def test_slot_arithmetic_is_exact(ps):
    ts = list(range(0, 4 * ps + 17)) + [2 ** 24 - 1, 2 ** 24 - ps, 2 ** 24 - ps - 1, 2 ** 23 + 5]
    assert all(pg_slot(t, ps) == t // ps for t in ts)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("ps", [16, 48, 64, 256])
def test_no_piece_straddles_a_page_and_every_key_is_fetched_once(D, ps):
    rpp = 512 // D
    for length in (1, 15, 16, 17, 127, 128, 129, 300, 2 * ps, 2 * ps + 1, 3 * ps - 1, 5 * 128):
        seen, top = [], -1
        for tile0 in range(0, length, 128):
            pieces = piece_fetches(D, ps, length, tile0)
            assert sorted(k for k, _r, _s in pieces) == list(range(tile0, tile0 + 128, rpp))   # the tile is fully written
            for key, rows, slot in pieces:
                if rows == 0:
                    assert key >= length
                    continue
                assert key // ps == (key + rows - 1) // ps == slot, (D, ps, length, key)   # inside one page
                assert (key % ps) + rows <= ps
                seen += list(range(key, key + rows))
                top = max(top, slot)
            assert max(s for _k, _r, s in pieces) <= (length - 1) // ps   # no slot past the last one in use, fetched or not
        assert sorted(seen) == list(range(length))
        assert top == (length + ps - 1) // ps - 1
