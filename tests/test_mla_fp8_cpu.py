"""CPU: the packed 8-bit latent cache (include/fa_mi355x.h: fa_mla_fp8_forward, fa_mla_fp8_workspace_bytes, fa_mla_fp8_pack;
FlashMLA's 656-byte token) — declared, exported, the signature rows, every bad argument rejected before any HIP call in the
documented order, the workspace query against the qv and the sparse one, the Python wrappers' checks and what they hand to the
library, and the reference itself (tests/mla_fp8_ref.py): scales, zero tiles, the rotary bytes, the round-trip error bound."""
import contextlib
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mla_fp8_ref as ref
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_mla_fp8_forward", "fa_mla_fp8_workspace_bytes", "fa_mla_fp8_pack")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

ORDER = ("q", "qv", "kv", "ix", "seqlens", "table", "o", "lse", "b", "hq", "hkv", "nq", "topk", "d", "dv", "dtype", "qb", "qt", "qh", "qvb",
         "qvt", "qvh", "psb", "tsb", "ixb", "ixt", "trs", "nblk", "ps", "mb", "causal", "scale", "splits", "ws", "wsb")
# B = 2, H_q = 8, Nq = 3, bf16, q and qv the two column ranges of one (2, 3, 8, 576) tensor, 9 pages of 16 tokens of 656 bytes, 4
# table entries a sequence, every cached token (no indices), one split
BASE = dict(q=P, qv=P, kv=P, ix=None, seqlens=P, table=P, o=P, lse=P, b=2, hq=8, hkv=1, nq=3, topk=0, d=64, dv=512, dtype=2,
            qb=3 * 8 * 576, qt=8 * 576, qh=576, qvb=3 * 8 * 576, qvt=8 * 576, qvh=576, psb=16 * 656, tsb=656, ixb=0, ixt=0, trs=4, nblk=9,
            ps=16, mb=4, causal=0, scale=576 ** -0.5, splits=1, ws=None, wsb=0)
LISTS = dict(ix=P, topk=40, ixb=3 * 40, ixt=40)   # the same over a list of 40 entries a query token

PACK_ORDER = ("lat", "rope", "kv", "seqlens", "table", "b", "nnew", "lb", "lt", "rb", "rt", "psb", "tsb", "trs", "nblk", "ps", "mb", "pow2")
# B = 2, five new tokens, latent and rope the two column ranges of one (2, 5, 576) tensor
PACK = dict(lat=P, rope=P, kv=P, seqlens=P, table=P, b=2, nnew=5, lb=5 * 576, lt=576, rb=5 * 576, rt=576, psb=16 * 656, tsb=656, trs=4,
            nblk=9, ps=16, mb=4, pow2=0)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **kw)
    rc = ext._lib.fa_mla_fp8_forward(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def _pack(**kw):
    import flashattention_lab_cuda as ext

    a = dict(PACK, **kw)
    rc = ext._lib.fa_mla_fp8_pack(*[a[n] for n in PACK_ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS
    assert hasattr(ext, "ex_mla_fp8_forward") and hasattr(ext, "ex_mla_fp8_pack")


def test_signature_rows_and_a_family_of_its_own():
    import flashattention_lab_cuda as ext

    names = PROTOTYPES["fa_mla_fp8_forward"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_mla_fp8_forward"][1]] == names and len(names) == len(ORDER) + 1   # (ORDER: all but the stream)
    assert names[:8] == ["q", "qv", "kv_cache", "indices", "cache_seqlens", "block_table", "o", "lse"]
    assert names[-3:] == ["workspace", "workspace_bytes", "stream"]
    at = names.index("page_stride_bytes")
    assert names[at:at + 2] == ["page_stride_bytes", "token_stride_bytes"] and PROTOTYPES["fa_mla_fp8_forward"][1][at:at + 2] == [ctypes.c_int64] * 2
    pnames = PROTOTYPES["fa_mla_fp8_pack"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_mla_fp8_pack"][1]] == pnames and len(pnames) == len(PACK_ORDER) + 1
    assert pnames[:5] == ["latent_new", "rope_new", "kv_cache", "cache_seqlens", "block_table"] and pnames[-2:] == ["scale_pow2", "stream"]
    assert PROTOTYPES["fa_mla_fp8_workspace_bytes"][2] == ["batch", "heads_q", "heads_kv", "seqlen_q", "cache_len", "topk", "with_indices", "num_splits"]
    assert PROTOTYPES["fa_mla_fp8_workspace_bytes"][0] is ctypes.c_size_t
    # each the only and widest member of its family; no entry point is as wide as another family's widest one
    for name, count in (("fa_mla_fp8_forward", len(names)), ("fa_mla_fp8_pack", len(pnames))):
        assert ext._CALLS[name][2] == count
        assert [n for n, c in ext._CALLS.items() if c[2] == count] == [name]
    assert ext._CALLS["fa_ex_forward_kvcache_qv"][2] == 67
    sparse = len(PROTOTYPES["fa_mla_sparse_forward"][2])
    assert [n for n, c in ext._CALLS.items() if c[2] == sparse] == ["fa_mla_sparse_forward"]


# every row is rejected before any HIP call: there is no GPU here, and the pointers are fake.  In the documented order: a later
# rule's breach does not hide an earlier one (the rows with two breaches).
BAD = [
    # (0) the shape's signs
    (dict(b=-1), INVALID_ARGUMENT, "batch, seqlen_q and heads_q must be >= 0"),
    (dict(nq=-2, q=None), INVALID_ARGUMENT, "batch, seqlen_q and heads_q must be >= 0"),
    # (1) null pointers, before the widths
    (dict(q=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(qv=None, dv=256), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(kv=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(o=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(lse=None, dtype=1), INVALID_ARGUMENT, "null tensor pointer"),
    # (2) widths: 64 + 512 only, with both numbers; before the dtype
    (dict(dv=256), UNSUPPORTED, "head_dim = 64, d_v = 256"),
    (dict(d=128, dtype=1), UNSUPPORTED, "head_dim = 128, d_v = 512"),
    (dict(d=576, dv=512), UNSUPPORTED, "head_dim = 576, d_v = 512"),
    # (3) dtype: bf16, f16 refused by name; then heads_kv, block_table and the ranges
    (dict(dtype=1), UNSUPPORTED, "f16 is not supported"),
    (dict(dtype=1, hkv=2), UNSUPPORTED, "f16 is not supported"),
    (dict(dtype=0), INVALID_ARGUMENT, "dtype must be bf16 (got code 0)"),
    (dict(dtype=3, table=None), INVALID_ARGUMENT, "dtype must be bf16 (got code 3)"),
    (dict(hkv=2), UNSUPPORTED, "heads_kv must be 1"),
    (dict(hkv=0, table=None), UNSUPPORTED, "heads_kv must be 1"),
    (dict(table=None), INVALID_ARGUMENT, "block_table is required"),
    (dict(table=None, tsb=640), INVALID_ARGUMENT, "block_table is required"),
    (dict(scale=0.0), INVALID_ARGUMENT, "softmax_scale must be > 0"),
    (dict(scale=float("nan")), INVALID_ARGUMENT, "softmax_scale must be finite"),
    (dict(splits=257), INVALID_ARGUMENT, "num_splits must lie in [0, 256]"),
    (dict(splits=-1, tsb=8), INVALID_ARGUMENT, "num_splits must lie in [0, 256]"),
    (dict(hq=65536 * 2), UNSUPPORTED, "problem too large"),
    (dict(b=2 ** 20, nq=2 ** 12), UNSUPPORTED, "problem too large"),
    (dict(b=65536), UNSUPPORTED, "problem too large"),            # the sequences along grid z without indices
    # (4) strides and alignment of q and qv, then the pool's two strides and its address
    (dict(qh=56), INVALID_ARGUMENT, "head stride of q must lie in [64"),
    (dict(qvh=64, tsb=8), INVALID_ARGUMENT, "head stride of qv must lie in [512"),
    (dict(qt=7 * 576 + 56), INVALID_ARGUMENT, "strides of q too small"),
    (dict(qb=2 * 8 * 576, topk=-1), INVALID_ARGUMENT, "strides of q too small"),
    (dict(qvt=8 * 512), INVALID_ARGUMENT, "strides of qv too small"),
    (dict(qvb=2 * 8 * 576), INVALID_ARGUMENT, "strides of qv too small"),
    (dict(qvt=8 * 576 + 4, qvb=4 * 8 * 576), INVALID_ARGUMENT, "strides of qv must be multiples of 8"),
    (dict(qh=580, qt=8 * 580, qb=3 * 8 * 580), INVALID_ARGUMENT, "strides of q must be multiples of 8"),
    (dict(tsb=655), INVALID_ARGUMENT, "token_stride_bytes must be >= 656 and a multiple of 16 (got 655)"),
    (dict(tsb=640, psb=8), INVALID_ARGUMENT, "token_stride_bytes must be >= 656"),
    (dict(tsb=664, psb=16 * 664), INVALID_ARGUMENT, "token_stride_bytes must be >= 656 and a multiple of 16 (got 664)"),
    (dict(tsb=2 ** 31, psb=2 ** 36), UNSUPPORTED, "token_stride_bytes"),
    (dict(psb=15 * 656 + 640), INVALID_ARGUMENT, "page_stride_bytes must be >= (page_block_size - 1) * token_stride_bytes + 656 = 10496"),
    (dict(psb=16 * 656 + 8), INVALID_ARGUMENT, "page_stride_bytes must be"),
    (dict(tsb=672, psb=16 * 656, kv=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "page_stride_bytes must be >= (page_block_size - 1) * token_stride_bytes + 656 = 10736"),
    (dict(psb=-16), INVALID_ARGUMENT, "page_stride_bytes must be"),
    (dict(kv=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "kv_cache must be 16-byte aligned"),
    (dict(kv=ctypes.c_void_p(4096 + 8), ps=24), INVALID_ARGUMENT, "page_stride_bytes must be"),    # (24 tokens need a longer page)
    (dict(q=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "tensors must be 16-byte aligned"),
    (dict(qv=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "tensors must be 16-byte aligned"),
    (dict(o=ctypes.c_void_p(4096 + 4), mb=0), INVALID_ARGUMENT, "tensors must be 16-byte aligned"),
    (dict(lse=ctypes.c_void_p(4096 + 1)), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (dict(seqlens=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (dict(table=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (dict(LISTS, ix=ctypes.c_void_p(4096 + 2), ixt=8), INVALID_ARGUMENT, "must be 4-byte aligned"),
    # (5) the lists, before the page geometry
    (dict(LISTS, topk=-1), INVALID_ARGUMENT, "topk must lie in [0, 2^30] (got -1)"),
    (dict(LISTS, topk=2 ** 30 + 1), INVALID_ARGUMENT, "topk must lie in"),
    (dict(LISTS, ixt=39), INVALID_ARGUMENT, "strides of indices"),
    (dict(LISTS, ixb=119), INVALID_ARGUMENT, "strides of indices"),
    (dict(LISTS, ixb=-120), INVALID_ARGUMENT, "strides of indices"),
    (dict(LISTS, ixt=8, nblk=0), INVALID_ARGUMENT, "strides of indices"),
    (dict(topk=40), INVALID_ARGUMENT, "must be 0 without indices"),
    (dict(ixt=40, ps=8, psb=2 ** 20), INVALID_ARGUMENT, "must be 0 without indices"),
    # (6) the page geometry, before the workspace
    (dict(ps=24, psb=24 * 656), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 24)"),
    (dict(ps=0, splits=4), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 0)"),
    (dict(nblk=0), INVALID_ARGUMENT, "num_blocks must lie in [1, 2^31)"),
    (dict(mb=0), INVALID_ARGUMENT, "max_blocks_per_seq must be >= 1"),
    (dict(mb=2 ** 24 + 1, trs=2 ** 25), UNSUPPORTED, "beyond 2^28 tokens"),
    (dict(trs=3, splits=4), INVALID_ARGUMENT, "block_table_row_stride=3 must be >= max_blocks_per_seq=4"),
    # (7) the workspace
    (dict(splits=4, ws=P, wsb=0), INVALID_ARGUMENT, "workspace of"),
    (dict(LISTS, splits=4, ws=None, wsb=2 ** 40), INVALID_ARGUMENT, "workspace of"),
    (dict(splits=2, ws=ctypes.c_void_p(4096 + 8), wsb=2 ** 40), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
    (dict(LISTS, b=2 ** 12, nq=2 ** 12, hq=4, qb=2 ** 12 * 4 * 576, qt=4 * 576, qvb=2 ** 12 * 4 * 576, qvt=4 * 576, ixb=40 * 2 ** 12, splits=2, ws=P,
          wsb=2 ** 50), UNSUPPORTED, "rows are too many to combine 2 splits"),
]


@pytest.mark.parametrize("kw,code,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _call(**kw)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_mla_fp8_forward:"), (kw, msg)


PACK_BAD = [
    (dict(b=-1), INVALID_ARGUMENT, "batch and seqlen_new must be >= 0"),
    (dict(nnew=-1, lat=None), INVALID_ARGUMENT, "batch and seqlen_new must be >= 0"),
    (dict(lat=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(rope=None, lt=8), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(kv=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(seqlens=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(table=None, tsb=8), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(b=2 ** 20, nnew=2 ** 12), UNSUPPORTED, "problem too large"),
    (dict(lt=504), INVALID_ARGUMENT, "strides of latent_new too small"),
    (dict(lb=4 * 576 + 504, rt=8), INVALID_ARGUMENT, "strides of latent_new too small"),
    (dict(rt=56), INVALID_ARGUMENT, "strides of rope_new too small"),
    (dict(rb=-8), INVALID_ARGUMENT, "strides of rope_new too small"),
    (dict(rt=580, rb=5 * 580, tsb=8), INVALID_ARGUMENT, "strides of rope_new must be multiples of 8"),
    (dict(tsb=648), INVALID_ARGUMENT, "token_stride_bytes must be >= 656 and a multiple of 16 (got 648)"),
    (dict(tsb=688, psb=16 * 656), INVALID_ARGUMENT, "page_stride_bytes must be >= (page_block_size - 1) * token_stride_bytes + 656 = 10976"),
    (dict(kv=ctypes.c_void_p(4096 + 4)), INVALID_ARGUMENT, "kv_cache must be 16-byte aligned"),
    (dict(lat=ctypes.c_void_p(4096 + 8), ps=8), INVALID_ARGUMENT, "tensors must be 16-byte aligned"),
    (dict(rope=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "tensors must be 16-byte aligned"),
    (dict(seqlens=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (dict(ps=32, psb=32 * 656, nblk=0), INVALID_ARGUMENT, "num_blocks must lie in [1, 2^31)"),
    (dict(ps=8), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 8)"),
    (dict(mb=0), INVALID_ARGUMENT, "max_blocks_per_seq must be >= 1"),
    (dict(trs=3), INVALID_ARGUMENT, "block_table_row_stride=3 must be >= max_blocks_per_seq=4"),
]


@pytest.mark.parametrize("kw,code,what", PACK_BAD, ids=[str(i) for i in range(len(PACK_BAD))])
def test_pack_bad_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _pack(**kw)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_mla_fp8_pack:"), (kw, msg)


def test_an_empty_call_is_ok_before_anything_is_looked_at():
    for kw in (dict(b=0), dict(nq=0), dict(hq=0)):
        rc, msg = _call(**kw, q=None, qv=None, kv=None, o=None, lse=None, table=None, d=7, dtype=9, topk=-5, ps=3, tsb=1)
        assert rc == OK, (kw, msg)
    for kw in (dict(b=0), dict(nnew=0)):
        rc, msg = _pack(**kw, lat=None, rope=None, kv=None, seqlens=None, table=None, ps=3, tsb=1)
        assert rc == OK, (kw, msg)


def test_workspace_query_is_the_qv_and_the_sparse_one():
    """the same shape gives the same splits, hence the same bytes, as the 16-bit calls"""
    import flashattention_lab_cuda as ext

    f, qvq, spq = ext._lib.fa_mla_fp8_workspace_bytes, ext._lib.fa_ex_kvcache_workspace_bytes_qv, ext._lib.fa_mla_sparse_workspace_bytes
    seen = set()
    for b, hq, nq, cap, topk in ((32, 128, 1, 4096, 2048), (32, 16, 1, 4096, 2048), (1, 128, 2, 8192, 512), (1, 16, 1, 2 ** 20, 2 ** 20),
                                 (3, 40, 2, 160, 160), (4, 17, 1, 112, 40), (4, 1, 1, 112, 0), (2, 80, 1, 144, 97), (1, 1, 1, 16, 1)):
        for splits in (0, 1, 2, 7, 256):
            dense = f(b, hq, 1, nq, cap, 0, 0, splits)
            assert dense == qvq(b, hq, 1, b * nq, nq, cap, 64, splits, 0, 512), (b, hq, nq, cap, splits)
            lists = f(b, hq, 1, nq, cap, topk, 1, splits)
            assert lists == spq(b, hq, 1, nq, topk, splits), (b, hq, nq, topk, splits)
            seen.update((dense, lists))
    assert len(seen) > 10 and f(32, 128, 1, 1, 4096, 0, 0, 0) > 0
    assert f(32, 16, 1, 1, 4096, 0, 0, 4) == 32 * 16 * 4 * 513 * 4
    for bad in ((0, 8, 1, 1, 64, 0, 0, 2), (1, 8, 2, 1, 64, 0, 0, 2), (1, 8, 1, 0, 64, 0, 0, 2), (1, 8, 1, 1, 64, -1, 1, 2), (1, 8, 1, 1, 64, 40, 0, 2),
                (1, 8, 1, 1, 64, 0, 0, 257), (1, 8, 1, 1, -1, 0, 0, 2)):
        assert f(*bad) == 0, bad
    # the call asks for what the query answers
    need = f(2, 8, 1, 3, 64, 0, 0, 4)
    rc, msg = _call(splits=4, ws=P, wsb=need - 1)
    assert need > 0 and rc == INVALID_ARGUMENT and "workspace" in msg and str(need) in msg


class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def test_python_wrappers_errors():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_mla_with_kvcache, mla_fp8_pack_cache

    q, pool8, pool16 = _fake(2, 3, 8, 576), _fake(9, 16, 1, 656, dtype=torch.uint8), _fake(9, 16, 1, 576)
    table, lens = _fake(2, 4, dtype=torch.int32), _fake(2, dtype=torch.int32)
    ix = _fake(2, 3, 40, dtype=torch.int32)
    fm = flash_mla_with_kvcache
    params = inspect.signature(fm).parameters
    assert [p.name for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == ["q", "k_cache", "block_table", "cache_seqlens", "head_dim_v"]
    assert params["head_dim_v"].default == 512 and params["is_fp8_kvcache"].default is False and params["indices"].default is None
    assert params["causal"].default is False and params["num_splits"].default == 0 and params["softmax_scale"].default is None
    # by name: head_dim_v, dtypes
    with pytest.raises(NotImplementedError, match="head_dim_v = 256"):
        fm(q, pool8, table, lens, 256, is_fp8_kvcache=True)
    with pytest.raises(NotImplementedError, match="q of dtype torch.float32"):
        fm(q.float(), pool16, table, lens)
    with pytest.raises(NotImplementedError, match="q of dtype torch.float16 is not supported with is_fp8_kvcache"):
        fm(q.half(), pool8, table, lens, is_fp8_kvcache=True)
    with pytest.raises(NotImplementedError, match="k_cache of dtype torch.bfloat16"):
        fm(q, pool16, table, lens, is_fp8_kvcache=True)
    with pytest.raises(NotImplementedError, match="k_cache of dtype torch.uint8"):
        fm(q, pool8, table, lens)
    with pytest.raises(NotImplementedError, match="k_cache of dtype torch.float16"):
        fm(q, pool16.half(), table, lens)
    with pytest.raises(NotImplementedError, match="block_table of dtype torch.int64"):
        fm(q, pool8, table.long(), lens, is_fp8_kvcache=True)
    with pytest.raises(NotImplementedError, match="block_table of dtype NoneType"):
        fm(q, pool8, None, lens, is_fp8_kvcache=True)
    with pytest.raises(NotImplementedError, match="indices of dtype torch.int64"):
        fm(q, pool8, table, lens, is_fp8_kvcache=True, indices=ix.long())
    with pytest.raises(NotImplementedError, match="cache_seqlens of dtype torch.int64"):
        fm(q, pool8, table, lens.long(), is_fp8_kvcache=True)
    # shapes and devices
    with pytest.raises(RuntimeError, match="must be GPU"):
        fm(torch.zeros((2, 3, 8, 576), dtype=torch.bfloat16), pool8, table, lens, is_fp8_kvcache=True)
    with pytest.raises(RuntimeError, match=r"q must be \(B, Nq, H_q, 576\)"):
        fm(_fake(2, 3, 8, 512), pool8, table, lens, is_fp8_kvcache=True)
    with pytest.raises(RuntimeError, match=r"k_cache must be \(num_blocks, page_block_size, 1, 656\)"):
        fm(q, _fake(9, 16, 1, 576, dtype=torch.uint8), table, lens, is_fp8_kvcache=True)
    with pytest.raises(RuntimeError, match=r"k_cache must be \(num_blocks, page_block_size, 1, 576\)"):
        fm(q, _fake(9, 16, 2, 576), table, lens)
    with pytest.raises(RuntimeError, match=r"indices must be an int32 \(B, Nq, topk\)"):
        fm(q, pool8, table, lens, is_fp8_kvcache=True, indices=_fake(2, 2, 40, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="page_block_size .* multiple of 16"):
        fm(q, _fake(9, 24, 1, 656, dtype=torch.uint8), table, lens, is_fp8_kvcache=True)
    with pytest.raises(RuntimeError, match="block_table must be an int32"):
        fm(q, pool8, _fake(3, 4, dtype=torch.int32), lens, is_fp8_kvcache=True)
    with pytest.raises(RuntimeError, match="cache_seqlens must be an int32"):
        fm(q, pool8, table, _fake(3, dtype=torch.int32), is_fp8_kvcache=True)
    with pytest.raises(ValueError, match="never copied"):    # tokens at a stride that is no multiple of 16
        fm(q, _fake(9, 16, 1, 664, dtype=torch.uint8)[..., :656], table, lens, is_fp8_kvcache=True)
    # the extension's own call: q and qv by name and shape
    with pytest.raises(NotImplementedError, match="q and qv of dtype torch.float16"):
        ext.ex_mla_fp8_forward(_fake(2, 3, 8, 64, dtype=torch.float16), _fake(2, 3, 8, 512, dtype=torch.float16), pool8, table, lens)
    with pytest.raises(NotImplementedError, match=r"head dim 64 with qv of head dim 512 only \(got 64, 256\)"):
        ext.ex_mla_fp8_forward(_fake(2, 3, 8, 64), _fake(2, 3, 8, 256), pool8, table, lens)
    with pytest.raises(RuntimeError, match=r"qv must be a \(B, Nq, H_q, 512\)"):
        ext.ex_mla_fp8_forward(_fake(2, 3, 8, 64), _fake(2, 3, 4, 512), pool8, table, lens)
    with pytest.raises(NotImplementedError, match="kv_cache of dtype torch.int8"):
        ext.ex_mla_fp8_forward(_fake(2, 3, 8, 64), _fake(2, 3, 8, 512), pool8.to(torch.int8), table, lens)
    # the append
    new = _fake(2, 5, 576)
    for fn in (mla_fp8_pack_cache, ext.ex_mla_fp8_pack):
        with pytest.raises(NotImplementedError, match="latent_new of dtype torch.float16"):
            fn(new.half()[..., :512], new[..., 512:], pool8, lens, table)
        with pytest.raises(NotImplementedError, match="rope_new of dtype torch.float32"):
            fn(new[..., :512], new.float()[..., 512:], pool8, lens, table)
        with pytest.raises(NotImplementedError, match="kv_cache of dtype torch.bfloat16"):
            fn(new[..., :512], new[..., 512:], pool16, lens, table)
        with pytest.raises(NotImplementedError, match="block_table of dtype torch.int64"):
            fn(new[..., :512], new[..., 512:], pool8, lens, table.long())
        with pytest.raises(NotImplementedError, match="cache_seqlens of dtype torch.int64"):
            fn(new[..., :512], new[..., 512:], pool8, lens.long(), table)
        with pytest.raises(RuntimeError, match="must be a GPU"):
            fn(torch.zeros((2, 5, 512), dtype=torch.bfloat16), new[..., 512:], pool8, lens, table)
        with pytest.raises(RuntimeError, match=r"latent_new and rope_new must be \(B, N_new, 512\) and \(B, N_new, 64\)"):
            fn(new[..., :512], new[:, :4, 512:], pool8, lens, table)
        with pytest.raises(RuntimeError, match=r"latent_new and rope_new must be"):
            fn(new[..., :256], new[..., 512:], pool8, lens, table)
        with pytest.raises(RuntimeError, match=r"kv_cache must be \(num_blocks, page_block_size, 1, 656\)"):
            fn(new[..., :512], new[..., 512:], _fake(9, 16, 656, dtype=torch.uint8), lens, table)
        with pytest.raises(RuntimeError, match="cache_seqlens must be an int32"):
            fn(new[..., :512], new[..., 512:], pool8, None, table)
    assert inspect.signature(mla_fp8_pack_cache).parameters["scale_pow2"].kind is inspect.Parameter.KEYWORD_ONLY


def test_views_strides_and_the_default_scale_as_handed_to_the_library(monkeypatch):
    """q[..., :512] goes as qv and q[..., 512:] as q, with the head stride 576 and no copy; the pool's own byte strides; the 16-bit
    route ends in the two existing calls on the pool's two slices: caught at the wrappers' call into the library"""
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_mla_with_kvcache, mla_fp8_pack_cache

    seen = []
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ext, "_stream_ptr", lambda dev: 0)
    monkeypatch.setattr(ext, "_call", lambda name, values: seen.append((name, values)))

    def got(want):
        name, values = seen[-1]
        fields = [f for f, _t in ext._SIGNATURES[name][1]]
        assert name == want and len(values) == len(fields)
        return dict(zip(fields, values))

    q = _fake(2, 3, 8, 576)
    wide = _fake(9, 16, 1, 672, dtype=torch.uint8)
    pool8 = wide[..., :656]
    table, lens = _fake(2, 4, dtype=torch.int32), _fake(2, dtype=torch.int32)
    o, lse = flash_mla_with_kvcache(q, pool8, table, lens, is_fp8_kvcache=True, num_splits=1)
    a = got("fa_mla_fp8_forward")
    assert o.shape == (2, 3, 8, 512) and o.dtype == torch.bfloat16 and lse.shape == (2, 8, 3) and lse.dtype == torch.float32
    assert a["softmax_scale"] == 576 ** -0.5 and (a["q"], a["qv"]) == (q.data_ptr() + 1024, q.data_ptr())
    assert (a["q_head_stride"], a["q_token_stride"], a["q_batch_stride"]) == (576, 8 * 576, 3 * 8 * 576)
    assert (a["qv_head_stride"], a["qv_token_stride"], a["qv_batch_stride"]) == (576, 8 * 576, 3 * 8 * 576)
    assert (a["kv_cache"], a["page_stride_bytes"], a["token_stride_bytes"]) == (wide.data_ptr(), 16 * 672, 672)
    assert (a["indices"], a["topk"], a["indices_batch_stride"], a["indices_token_stride"]) == (0, 0, 0, 0)
    assert (a["block_table"], a["block_table_row_stride"], a["num_blocks"], a["page_block_size"], a["max_blocks_per_seq"]) == (table.data_ptr(), 4, 9, 16, 4)
    assert (a["cache_seqlens"], a["heads_q"], a["heads_kv"], a["d"], a["d_v"], a["dtype"], a["causal"], a["num_splits"], a["workspace_bytes"]) == \
        (lens.data_ptr(), 8, 1, 64, 512, 2, 0, 1, 0)
    ix = _fake(2, 3, 64, dtype=torch.int32)
    flash_mla_with_kvcache(q, pool8.view(torch.float8_e4m3fn), table, None, is_fp8_kvcache=True, indices=ix[..., 8:48], causal=True,
                           softmax_scale=0.25, num_splits=1)
    a = got("fa_mla_fp8_forward")
    assert (a["indices"], a["topk"], a["indices_batch_stride"], a["indices_token_stride"]) == (ix.data_ptr() + 32, 40, 192, 64)
    assert (a["softmax_scale"], a["causal"], a["cache_seqlens"], a["kv_cache"]) == (0.25, 1, 0, wide.data_ptr())
    # the append: the two column ranges of one tensor, as they are
    new = _fake(2, 5, 576)
    assert mla_fp8_pack_cache(new[..., :512], new[..., 512:], pool8, lens, table, scale_pow2=True) is None
    a = got("fa_mla_fp8_pack")
    assert (a["latent_new"], a["rope_new"]) == (new.data_ptr(), new.data_ptr() + 1024)
    assert (a["latent_batch_stride"], a["latent_token_stride"], a["rope_batch_stride"], a["rope_token_stride"]) == (5 * 576, 576, 5 * 576, 576)
    assert (a["batch"], a["seqlen_new"], a["scale_pow2"], a["page_stride_bytes"], a["token_stride_bytes"]) == (2, 5, 1, 16 * 672, 672)
    assert (a["cache_seqlens"], a["block_table"], a["max_blocks_per_seq"]) == (lens.data_ptr(), table.data_ptr(), 4)
    # the 16-bit route: the existing calls on the pool's two slices, scale 576 ** -0.5
    pool16 = _fake(9, 16, 1, 576)
    flash_mla_with_kvcache(q, pool16, table, lens, num_splits=1)
    a = got("fa_ex_forward_kvcache_qv")
    assert (a["k_cache"], a["v_cache"], a["d"], a["d_v"], a["softmax_scale"]) == (pool16.data_ptr() + 1024, pool16.data_ptr(), 64, 512, 576 ** -0.5)
    assert (a["k_cache_token_stride"], a["v_cache_token_stride"], a["block_table"]) == (576, 576, table.data_ptr())
    flash_mla_with_kvcache(q, pool16, table, lens, indices=ix[..., :40], num_splits=1)
    a = got("fa_mla_sparse_forward")
    assert (a["k_cache"], a["v_cache"], a["topk"], a["softmax_scale"]) == (pool16.data_ptr() + 1024, pool16.data_ptr(), 40, 576 ** -0.5)


# ---- the reference itself

def _values(shape, seed):
    """bf16 values with |x| in [2^-6, 8], random signs"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(shape, generator=g) * (8 - 2 ** -6) + 2 ** -6
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    x = (mag * sign).to(torch.bfloat16)
    assert (x.abs() >= 2 ** -6).all() and (x.abs() <= 8).all()
    return x


@pytest.mark.parametrize("pow2", (False, True))
def test_reference_scales_zero_tiles_and_rope_bytes(pow2):
    lat, rope = _values((6, 5, 512), 1), _values((6, 5, 64), 2)
    lat[0, 0, 128:256] = 0                      # an all-zero tile
    lat[1, 2, :128] *= 0.25
    lat[1, 2, 7] = 7.0                          # amax = 448 * 2^-6: scale 2^-6 exactly
    lat[2, 1, 384:] = (lat[2, 1, 384:].float() * 2 ** -7).to(torch.bfloat16)   # a small tile
    rows = ref.pack_rows(lat, rope, pow2)
    assert rows.shape == (6, 5, 656) and rows.dtype == torch.uint8
    scales = rows[..., 512:528].contiguous().view(torch.float32)
    # every scale as specified, against numpy's IEEE fp32 division
    amax = lat.float().reshape(6, 5, 4, 128).abs().amax(-1).numpy()
    want = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    if pow2:
        m, e = np.frexp(want)
        want = np.where(m == 0.5, want, np.ldexp(np.float32(1.0), e)).astype(np.float32)
        assert (np.frexp(want)[0] == 0.5).all() and (want >= np.where(amax > 0, amax / np.float32(448.0), 1)).all()
        assert (want < 2 * np.where(amax > 0, amax / np.float32(448.0), 1)).all()
    assert np.array_equal(scales.numpy().view(np.uint32), want.view(np.uint32))
    assert scales[0, 0, 1] == 1.0 and (rows[0, 0, 128:256] == 0).all()
    assert scales[1, 2, 0] == 2 ** -6
    # the bytes, against numpy's division and torch's e4m3fn rounding
    y = np.clip(lat.float().reshape(6, 5, 4, 128).numpy() / want[..., None], -448, 448).astype(np.float32)
    assert torch.equal(rows[..., :512], torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).reshape(6, 5, 512))
    assert (rows[..., :512] & 0x7f).max() <= 0x7e                       # never the NaN code
    if not pow2:                                                         # the tile's largest element is +-448
        assert ((rows[..., :512].reshape(6, 5, 4, 128) & 0x7f).amax(-1)[torch.from_numpy(amax > 0)] == 0x7e).all()
    # the rotary bytes verbatim
    assert torch.equal(rows[..., 528:].contiguous().view(torch.bfloat16), rope)
    lat2, rope2 = ref.unpack_rows(rows)
    assert torch.equal(rope2.view(torch.int16), rope.view(torch.int16)) and (lat2[0, 0, 128:256] == 0).all()
    # a wider token stride carries the same rows
    wide = torch.full((6, 5, 672), 0xA5, dtype=torch.uint8)
    wide[..., :656] = rows
    assert torch.equal(ref.unpack_rows(wide)[0].view(torch.int16), lat2.view(torch.int16))


@pytest.mark.parametrize("pow2", (False, True))
def test_round_trip_error_bound(pow2):
    """Every element of unpack(pack(x)) is within 2^-4 * amax of x, amax the largest magnitude of its 128-wide tile, for both
    quantisers.  The exact bounds, asserted beside it: let R = amax / scale, so that y = x / scale has |y| <= R (up to one fp32
    rounding, 2^-23 relative, then the clamp).  e4m3 has 3 mantissa bits: its step is 32 in the top binade [256, 448] and at most
    16 below 256, so |q - y| <= 8 for |y| <= 256 and <= min(16, R - 256) above (up to 272 the neighbours are 256 and 288, and y
    cannot pass R).  Relative to amax = R * scale that is 8 / R or min(16, R - 256) / R.
      * scale = amax / 448: R = 448, the error of the quantiser is at most 16 / 448 = 1 / 28 of amax.
      * scale_pow2: the scale is rounded up by less than 2, R lies in (224, 448]; 8 / R < 1 / 28, and min(16, R - 256) / R is largest
        at R = 272: 16 / 272 = 1 / 17 of amax (attained: amax = 4.25 gives scale 2^-6 and y = 272, a tie that rounds to 256).
    The read contract then rounds q * scale (|.| <= amax (1 + 2^-22)) once to bf16, 8 significant bits: another 2^-9 * amax.  With
    2^-20 * amax for the fp32 roundings: (1 / 28 + 2^-9 + 2^-20) amax = 0.0377 amax and (1 / 17 + 2^-9 + 2^-20) amax = 0.0608 amax,
    both below 2^-4 amax = 0.0625 amax."""
    lat = _values((8, 16, 512), 3 + pow2)
    small = lat[0, :, :256].float() * 2 ** -3          # tiles of a smaller range, still within [2^-6, 8]
    lat[0, :, :256] = torch.where(small.abs() < 2 ** -6, torch.full_like(small, 2 ** -6), small).to(torch.bfloat16)
    # tiles with R = 272 under scale_pow2 (amax = 272 * 2^-6, 2^-7): the worst case of the derivation, the amax itself on the tie
    lat[1, :, :128] = lat[1, :, :128].clamp(-4.25, 4.25)
    lat[1, :, 5] = 4.25
    lat[1, :, 128:256] = lat[1, :, 128:256].clamp(-2.125, 2.125)
    lat[1, :, 130] = -2.125
    rope = _values((8, 16, 64), 5)
    back, _rope = ref.unpack_rows(ref.pack_rows(lat, rope, pow2))
    x = lat.double().reshape(8, 16, 4, 128)
    err = (back.double().reshape(8, 16, 4, 128) - x).abs()
    amax = x.abs().amax(-1, keepdim=True)
    print("round trip, scale_pow2 =", pow2, ": largest error / amax =", float((err / amax).max()))
    assert (err <= 2 ** -4 * amax).all(), float((err / amax).max())
    tight = (1 / 17 if pow2 else 1 / 28) + 2 ** -9 + 2 ** -20
    assert (err <= tight * amax).all(), float((err / amax).max())
    if pow2:   # the worst case is reached: 4.25 comes back as 4.0
        assert float(back[1, 0, 5]) == 4.0 and float(back[1, 0, 130]) == -2.0 and float((err / amax).max()) == 1 / 17
    assert float((err / amax).max()) > 2 ** -7       # (the bound is not vacuous: errors of this order do occur)


def test_scatter_rows_maps_positions_and_drops():
    pool = torch.full((4, 16, 1, 672), 0xA5, dtype=torch.uint8)
    rows = torch.arange(3 * 2 * 656, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(3, 2, 656)
    table = torch.tensor([[2, 0], [1, 7], [3, -1]], dtype=torch.int32)
    out, dropped = ref.scatter_rows(pool, rows, torch.tensor([15, 16, 31]), table)
    # sequence 0: positions 15, 16 -> page 2 slot 15, page 0 slot 0; sequence 1: position 16, 17 on page 7: outside the pool;
    # sequence 2: position 31 on page -1, position 32 past the capacity
    assert dropped == [(1, 0), (1, 1), (2, 0), (2, 1)]
    assert torch.equal(out[2, 15, 0, :656], rows[0, 0]) and torch.equal(out[0, 0, 0, :656], rows[0, 1])
    changed = (out != pool).any(-1).nonzero().tolist()
    assert changed == [[0, 0, 0], [2, 15, 0]] and (out[..., 656:] == 0xA5).all()
    _out, dropped = ref.scatter_rows(pool, rows, torch.tensor([-1, 0, 0]), table)
    assert dropped == [(0, 0), (0, 1)]
