"""CPU: sparse MLA decoding (include/fa_mi355x.h: fa_mla_sparse_forward, fa_mla_sparse_workspace_bytes; attention over a per-query
list of cached tokens) — declared, exported, the signature rows, every bad argument rejected before any HIP call in the
documented order, the workspace formula and the launch rule at hand-computed points, the Python wrappers' checks, the default
scale as handed to the library, and the fp64 reference (tests/mla_sparse_ref.py) against the dense one (tests/mla_ref.py)."""
import contextlib
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests import mla_ref
from tests.mla_sparse_ref import mla_sparse_reference
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_mla_sparse_forward", "fa_mla_sparse_workspace_bytes")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

ORDER = ("q", "qv", "kc", "vc", "ix", "seqlens", "o", "lse", "b", "hq", "hkv", "nq", "cap", "topk", "d", "dv", "dtype", "qb", "qt", "qvb", "qvt",
         "kcb", "kct", "vcb", "vct", "ixb", "ixt", "ixh", "causal", "scale", "splits", "table", "trs", "nblk", "ps", "mb", "bidx", "bcache",
         "ws", "wsb")
# B = 2, H_q = 8, H_kv = 2, Nq = 3, cache_len = 64, topk = 40, bf16, one list per (token, K/V head), one split
BASE = dict(q=P, qv=P, kc=P, vc=P, ix=P, seqlens=P, o=P, lse=P, b=2, hq=8, hkv=2, nq=3, cap=64, topk=40, d=64, dv=512, dtype=2,
            qb=3 * 8 * 64, qt=8 * 64, qvb=3 * 8 * 512, qvt=8 * 512, kcb=64 * 2 * 64, kct=2 * 64, vcb=64 * 2 * 512, vct=2 * 512,
            ixb=3 * 2 * 40, ixt=2 * 40, ixh=40, causal=0, scale=576 ** -0.5, splits=1, table=None, trs=0, nblk=0, ps=0, mb=0, bidx=None,
            bcache=0, ws=None, wsb=0)
# the same over pools of 9 pages of 16 tokens, 4 table entries a sequence
PAGED = dict(table=P, trs=4, nblk=9, ps=16, mb=4, kcb=16 * 2 * 64, vcb=16 * 2 * 512)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **kw)
    rc = ext._lib.fa_mla_sparse_forward(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


def test_signature_rows_and_a_family_of_its_own():
    import flashattention_lab_cuda as ext

    names = PROTOTYPES["fa_mla_sparse_forward"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_mla_sparse_forward"][1]] == names and len(names) == len(ORDER) + 1   # (ORDER: all but the stream)
    assert names[:8] == ["q", "qv", "k_cache", "v_cache", "indices", "cache_seqlens", "o", "lse"]
    assert names[-3:] == ["workspace", "workspace_bytes", "stream"]
    at = names.index("indices_batch_stride")
    assert names[at:at + 3] == ["indices_batch_stride", "indices_token_stride", "indices_head_stride"]
    assert PROTOTYPES["fa_mla_sparse_forward"][1][at:at + 3] == [ctypes.c_int64] * 3
    assert PROTOTYPES["fa_mla_sparse_workspace_bytes"][2] == ["batch", "heads_q", "heads_kv", "seqlen_q", "topk", "num_splits"]
    assert PROTOTYPES["fa_mla_sparse_workspace_bytes"][0] is ctypes.c_size_t
    assert [f for f, _t in ext._SIGNATURES["fa_mla_sparse_workspace_bytes"][1]] == PROTOTYPES["fa_mla_sparse_workspace_bytes"][2]
    # the only and widest member of its family; the kv-cache family is what it was
    assert ext._CALLS["fa_mla_sparse_forward"][2] == len(names)
    assert [n for n, c in ext._CALLS.items() if c[2] == len(names)] == ["fa_mla_sparse_forward"]
    assert ext._CALLS["fa_ex_forward_kvcache_qv"][2] == 67


# every row is rejected before any HIP call: there is no GPU here, and the pointers are fake.  In the documented order: a later
# rule's breach does not hide an earlier one (the rows with two breaches).
BAD = [
    # (0) the shape's signs
    (dict(b=-1), INVALID_ARGUMENT, "batch, seqlen_q and heads_q must be >= 0"),
    (dict(nq=-2, q=None), INVALID_ARGUMENT, "batch, seqlen_q and heads_q must be >= 0"),
    # (1) null pointers, before the widths
    (dict(q=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(qv=None, dv=256), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(kc=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(vc=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(o=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(lse=None, dtype=0), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(ix=None), INVALID_ARGUMENT, "null tensor pointer"),
    # (2) widths: 64 + 512 only, with both numbers; before the dtype
    (dict(dv=256), UNSUPPORTED, "head_dim = 64, d_v = 256"),
    (dict(d=128, dtype=0), UNSUPPORTED, "head_dim = 128, d_v = 512"),
    (dict(d=576, dv=512), UNSUPPORTED, "head_dim = 576, d_v = 512"),
    (dict(dv=0), UNSUPPORTED, "head_dim = 64, d_v = 0"),
    # (3) dtype, then the ranges
    (dict(dtype=0), INVALID_ARGUMENT, "dtype must be f16 or bf16 (got code 0)"),
    (dict(dtype=3, qt=8), INVALID_ARGUMENT, "dtype must be f16 or bf16 (got code 3)"),
    (dict(hkv=3), INVALID_ARGUMENT, "heads_q=8 must be a positive multiple of heads_kv=3"),
    (dict(hkv=0), INVALID_ARGUMENT, "positive multiple of heads_kv=0"),
    (dict(scale=0.0), INVALID_ARGUMENT, "softmax_scale must be > 0"),
    (dict(scale=float("nan")), INVALID_ARGUMENT, "softmax_scale must be finite"),
    (dict(splits=257), INVALID_ARGUMENT, "num_splits must lie in [0, 256]"),
    (dict(splits=-1), INVALID_ARGUMENT, "num_splits must lie in [0, 256]"),
    (dict(cap=0), INVALID_ARGUMENT, "cache_len must be >= 1"),
    (dict(bidx=P, bcache=0), INVALID_ARGUMENT, "cache_batch must lie in [1, 2^31)"),
    (dict(bcache=4), INVALID_ARGUMENT, "cache_batch must be 0 without cache_batch_idx"),
    (dict(PAGED, bidx=P, bcache=4), INVALID_ARGUMENT, "block_table cannot be combined with cache_batch_idx"),
    (dict(hq=65536 * 2), UNSUPPORTED, "problem too large"),
    (dict(b=2 ** 20, nq=2 ** 12), UNSUPPORTED, "problem too large"),
    # (4) strides and alignment of every tensor, before the indices
    (dict(qt=8 * 64 - 8), INVALID_ARGUMENT, "strides of q too small"),
    (dict(qb=3 * 8 * 64 - 8, topk=-1), INVALID_ARGUMENT, "strides of q too small"),
    (dict(qvt=8 * 64), INVALID_ARGUMENT, "strides of qv too small"),
    (dict(qvb=2 * 8 * 512), INVALID_ARGUMENT, "strides of qv too small"),
    (dict(qvt=8 * 512 + 4, qvb=4 * 8 * 512), INVALID_ARGUMENT, "strides of qv must be multiples of 8"),
    (dict(kct=64), INVALID_ARGUMENT, "strides of k_cache too small"),
    (dict(kcb=63 * 2 * 64), INVALID_ARGUMENT, "strides of k_cache too small"),
    (dict(vct=2 * 64), INVALID_ARGUMENT, "strides of v_cache too small"),
    (dict(vcb=63 * 2 * 512), INVALID_ARGUMENT, "strides of v_cache too small"),
    (dict(vcb=-8), INVALID_ARGUMENT, "strides of v_cache too small"),
    (dict(PAGED, vcb=15 * 2 * 512), INVALID_ARGUMENT, "strides of v_cache too small"),       # a page holds page_block_size tokens
    (dict(bidx=P, bcache=4, kcb=8), INVALID_ARGUMENT, "strides of k_cache too small"),       # cache_batch rows
    (dict(cap=2 ** 21 + 1, vcb=2 ** 32, kcb=2 ** 32), UNSUPPORTED, "one batch element of v_cache spans"),
    (dict(q=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "16-byte aligned"),
    (dict(qv=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "16-byte aligned"),
    (dict(kc=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "16-byte aligned"),
    (dict(vc=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "16-byte aligned"),
    (dict(o=ctypes.c_void_p(4096 + 4)), INVALID_ARGUMENT, "16-byte aligned"),
    (dict(ix=ctypes.c_void_p(4096 + 2), ixh=8), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (dict(lse=ctypes.c_void_p(4096 + 1)), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (dict(seqlens=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "must be 4-byte aligned"),
    # (5) the lists, before the page geometry
    (dict(topk=-1), INVALID_ARGUMENT, "topk must lie in [0, 2^30] (got -1)"),
    (dict(topk=2 ** 30 + 1), INVALID_ARGUMENT, "topk must lie in"),
    (dict(ixh=39), INVALID_ARGUMENT, "strides of indices"),
    (dict(ixh=-40), INVALID_ARGUMENT, "strides of indices"),
    (dict(ixt=79), INVALID_ARGUMENT, "strides of indices"),
    (dict(ixh=0, ixt=39), INVALID_ARGUMENT, "strides of indices"),
    (dict(ixb=3 * 80 - 1), INVALID_ARGUMENT, "strides of indices"),
    (dict(ixb=-240), INVALID_ARGUMENT, "strides of indices"),
    (dict(PAGED, ixt=8, ps=24, vcb=24 * 2 * 512, kcb=24 * 2 * 64), INVALID_ARGUMENT, "strides of indices"),
    # (6) the page geometry, before the workspace
    (dict(PAGED, ps=24, vcb=24 * 2 * 512, kcb=24 * 2 * 64), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 24)"),
    (dict(PAGED, ps=0, splits=4), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 0)"),
    (dict(PAGED, nblk=0), INVALID_ARGUMENT, "num_blocks must lie in [1, 2^31)"),
    (dict(PAGED, mb=0), INVALID_ARGUMENT, "max_blocks_per_seq must be >= 1"),
    (dict(PAGED, mb=2 ** 24 + 1, trs=2 ** 25), UNSUPPORTED, "beyond 2^28 tokens"),
    (dict(PAGED, trs=3), INVALID_ARGUMENT, "block_table_row_stride=3 must be >= max_blocks_per_seq=4"),
    (dict(ps=16), INVALID_ARGUMENT, "must be 0 without block_table"),
    (dict(trs=4, splits=4), INVALID_ARGUMENT, "must be 0 without block_table"),
    # (7) the workspace
    (dict(splits=4, ws=P, wsb=0), INVALID_ARGUMENT, "workspace of"),
    (dict(splits=4, ws=None, wsb=2 ** 40), INVALID_ARGUMENT, "workspace of"),
    (dict(splits=2, ws=ctypes.c_void_p(4096 + 8), wsb=2 ** 40), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
    (dict(b=2 ** 12, nq=2 ** 12, hq=4, hkv=1, qb=2 ** 20, qt=256, qvb=2 ** 23, qvt=2048, kct=64, kcb=64 * 64, vct=512, vcb=64 * 512,
          ixh=0, ixt=40, ixb=40 * 2 ** 12, splits=2, ws=P, wsb=2 ** 50), UNSUPPORTED, "rows are too many to combine 2 splits"),
]


@pytest.mark.parametrize("kw,code,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _call(**kw)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_mla_sparse_forward:"), (kw, msg)


def test_an_empty_call_is_ok_before_anything_is_looked_at():
    for kw in (dict(b=0), dict(nq=0), dict(hq=0)):
        rc, msg = _call(**kw, q=None, qv=None, kc=None, vc=None, ix=None, o=None, lse=None, d=7, dtype=9, topk=-5, ps=3)
        assert rc == OK, (kw, msg)


def _ws_model(rows, s):
    if s <= 1:
        return 0
    r256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    return r256(rows * s * 512 * 4) + r256(rows * s * 4)


def _splits_model(units, hkv, group, topk):
    """csrc/fa_mla.hip: mla_waves and mla_sparse_num_splits"""
    nw = 1 if group <= 16 else 2 if group <= 32 else 4
    wgs = units * hkv * -(-group // (16 * nw))
    if wgs <= 0 or topk <= 0:
        return 1
    s = -(-256 * (4 // nw) // wgs)
    return max(1, min(s, -(-topk // 128), 256))


def test_workspace_bytes_formula_and_launch_rule():
    import flashattention_lab_cuda as ext

    f = ext._lib.fa_mla_sparse_workspace_bytes
    # hand-computed points of the rule: fill 256 CUs once at 4 / waves workgroups a CU, no split shorter than 128 entries, at most 256
    assert _splits_model(32, 1, 128, 2048) == 4        # 64 workgroups of four waves, one a CU: 256 / 64
    assert _splits_model(32, 1, 16, 2048) == 16        # 32 workgroups of one wave, four a CU: 1024 / 32 = 32, but 2048 / 128 = 16
    assert _splits_model(512, 1, 128, 2048) == 1       # 1024 workgroups: the chip is full
    assert _splits_model(1, 1, 16, 2 ** 20) == 256     # the combine's weight row
    assert _splits_model(1, 1, 1, 100) == 1 and _splits_model(3, 1, 40, 160) == 2 and _splits_model(1, 1, 16, 0) == 1
    for b, hq, hkv, nq, topk in ((32, 128, 1, 1, 2048), (32, 16, 1, 1, 2048), (1, 128, 1, 512, 2048), (1, 16, 1, 1, 2 ** 20), (3, 40, 1, 2, 160),
                                 (3, 8, 2, 2, 97), (2, 64, 2, 1, 1024), (1, 1, 1, 1, 0)):
        s = _splits_model(b * nq, hkv, hq // hkv, topk)
        assert f(b, hq, hkv, nq, topk, 0) == _ws_model(b * hq * nq, s), (b, hq, hkv, nq, topk, s)
        for given in (1, 2, 7, 256):
            assert f(b, hq, hkv, nq, topk, given) == _ws_model(b * hq * nq, given)
    assert f(32, 128, 1, 1, 2048, 0) == 32 * 128 * 4 * 513 * 4
    for bad in ((0, 8, 8, 1, 64, 2), (1, 8, 3, 1, 64, 2), (1, 8, 8, 0, 64, 2), (1, 8, 8, 1, -1, 2), (1, 8, 8, 1, 64, 257), (1, 8, 8, 1, 64, -1)):
        assert f(*bad) == 0, bad
    # the call asks for what the query answers
    need = _ws_model(2 * 8 * 3, 4)
    rc, msg = _call(splits=4, ws=P, wsb=need - 1)
    assert rc == INVALID_ARGUMENT and "workspace" in msg and str(need) in msg


class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def _wrappers():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_mla_sparse_attn

    return ((flash_mla_sparse_attn, True), (ext.ex_mla_sparse_forward, False))


def test_python_wrappers_errors():
    q, qv, kc, vc = _fake(2, 3, 8, 64), _fake(2, 3, 8, 512), _fake(2, 32, 2, 64), _fake(2, 32, 2, 512)
    ix = _fake(2, 3, 2, 40, dtype=torch.int32)
    for fn, public in _wrappers():
        for bad in (ix.long(), ix.to(torch.int16), ix.float(), [[1, 2]], None):
            with pytest.raises(NotImplementedError, match="indices of dtype .* is not supported"):
                fn(q, qv, kc, vc, bad)
        if public:   # block_table and cache_batch_idx of another dtype, by name; and the arguments after indices are keyword-only
            with pytest.raises(NotImplementedError, match="block_table of dtype torch.int64"):
                fn(q, qv, kc, vc, ix, block_table=torch.zeros((2, 4), dtype=torch.int64))
            with pytest.raises(NotImplementedError, match="cache_batch_idx of dtype torch.int64"):
                fn(q, qv, kc, vc, ix, cache_batch_idx=torch.zeros((2,), dtype=torch.int64))
            params = inspect.signature(fn).parameters
            assert [p.name for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == ["q", "qv", "k_cache", "v_cache", "indices"]
            assert params["causal"].default is False and params["num_splits"].default == 0 and params["return_softmax_lse"].default is False
        # widths other than 64 + 512, with both numbers
        with pytest.raises(NotImplementedError, match=r"head dim 64 with v_cache of head dim 512 only \(got 64, 256\)"):
            fn(q, _fake(2, 3, 8, 256), kc, _fake(2, 32, 2, 256), ix)
        with pytest.raises(NotImplementedError, match=r"\(got 128, 512\)"):
            fn(_fake(2, 3, 8, 128), qv, _fake(2, 32, 2, 128), vc, ix)
        # shapes and devices: RuntimeError before anything touches the device
        with pytest.raises(RuntimeError, match="must be a GPU"):
            fn(q, torch.zeros((2, 3, 8, 512), dtype=torch.bfloat16), kc, vc, ix)
        with pytest.raises(RuntimeError, match="q must be 4-D"):
            fn(_fake(6, 8, 64), qv, kc, vc, ix)
        with pytest.raises(RuntimeError, match="share a 16-bit dtype"):
            fn(q, _fake(2, 3, 8, 512, dtype=torch.float16), kc, vc, ix)
        with pytest.raises(RuntimeError, match=r"qv must be a \(B, Nq, H_q, 512\)"):
            fn(q, _fake(2, 3, 4, 512), kc, vc, ix)
        with pytest.raises(RuntimeError, match="multiple of the K/V heads"):
            fn(q, qv, _fake(2, 32, 3, 64), _fake(2, 32, 3, 512), ix)
        with pytest.raises(RuntimeError, match="k_cache and v_cache must be"):
            fn(q, qv, kc, _fake(2, 16, 2, 512), ix)
        with pytest.raises(RuntimeError, match="k_cache and v_cache must be"):
            fn(q, qv, _fake(3, 32, 2, 64), _fake(3, 32, 2, 512), ix)          # three cache rows for B = 2, no cache_batch_idx
        for bad in (_fake(2, 40, dtype=torch.int32), _fake(3, 3, 2, 40, dtype=torch.int32), _fake(2, 1, 2, 40, dtype=torch.int32),
                    _fake(2, 3, 4, 40, dtype=torch.int32), _fake(2, 3, 2, 2, 40, dtype=torch.int32)):
            with pytest.raises(RuntimeError, match=r"indices must be an int32 \(B, Nq, topk\) or \(B, Nq, H_kv, topk\)"):
                fn(q, qv, kc, vc, bad)
        with pytest.raises(RuntimeError, match="indices must be an int32"):
            fn(q, qv, kc, vc, torch.zeros((2, 3, 40), dtype=torch.int32, device="meta"))
        kw = dict(block_table=_fake(2, 4, dtype=torch.int32), cache_batch_idx=_fake(2, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="block_table cannot be combined with cache_batch_idx"):
            fn(q, qv, kc, vc, ix, **kw)
        with pytest.raises(RuntimeError, match="block_table must be an int32"):
            fn(q, qv, kc, vc, ix, block_table=_fake(3, 4, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="page_block_size .* multiple of 16"):
            fn(q, qv, _fake(5, 24, 2, 64), _fake(5, 24, 2, 512), ix, block_table=_fake(2, 4, dtype=torch.int32))
        # a cache view that would need a copy: the two slices of a (.., H_kv = 2, 576) pool have their heads 576 apart
        pool = _fake(2, 32, 2, 576)
        with pytest.raises(ValueError, match="never copied"):
            fn(q, qv, pool[..., 512:], pool[..., :512], ix)


def test_default_scale_strides_and_lists_as_handed_to_the_library(monkeypatch):
    """softmax_scale=None is (64 + 512) ** -0.5; the caches' own strides and the lists' layout reach the library as they are:
    caught at the wrapper's call into it (there is no GPU here)"""
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_mla_sparse_attn

    seen = []
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ext, "_stream_ptr", lambda dev: 0)
    monkeypatch.setattr(ext, "_call", lambda name, values: seen.append((name, values)))
    fields = [f for f, _t in ext._SIGNATURES["fa_mla_sparse_forward"][1]]

    def got():
        name, values = seen[-1]
        assert name == "fa_mla_sparse_forward" and len(values) == len(fields)
        return dict(zip(fields, values))

    q, qv, kc, vc = _fake(2, 3, 8, 64), _fake(2, 3, 8, 512), _fake(2, 32, 1, 64), _fake(2, 32, 1, 512)
    ix3 = _fake(2, 3, 40, dtype=torch.int32)
    o, lse = flash_mla_sparse_attn(q, qv, kc, vc, ix3, num_splits=1, return_softmax_lse=True)
    a = got()
    assert a["softmax_scale"] == (64 + 512) ** -0.5 and o.shape == (2, 3, 8, 512) and lse.shape == (2, 8, 3) and lse.dtype == torch.float32
    assert (a["d"], a["d_v"], a["topk"], a["cache_len"], a["causal"], a["num_splits"]) == (64, 512, 40, 32, 0, 1)
    assert (a["indices"], a["indices_batch_stride"], a["indices_token_stride"], a["indices_head_stride"]) == (ix3.data_ptr(), 120, 40, 0)
    assert (a["cache_seqlens"], a["block_table"], a["cache_batch_idx"], a["cache_batch"], a["workspace_bytes"]) == (0, 0, 0, 0, 0)
    assert isinstance(flash_mla_sparse_attn(q, qv, kc, vc, ix3, num_splits=1, softmax_scale=0.25, causal=True), torch.Tensor)
    a = got()
    assert a["softmax_scale"] == 0.25 and a["causal"] == 1
    # (B, Nq, H_kv, topk): a list per K/V head; a view expanded over the heads is the shared list again; a sliced one keeps its strides
    kc2, vc2 = _fake(2, 32, 2, 64), _fake(2, 32, 2, 512)
    ix4 = _fake(2, 3, 2, 40, dtype=torch.int32)
    ext.ex_mla_sparse_forward(q, qv, kc2, vc2, ix4, num_splits=1)
    a = got()
    assert (a["indices_batch_stride"], a["indices_token_stride"], a["indices_head_stride"], a["heads_kv"]) == (240, 80, 40, 2)
    ext.ex_mla_sparse_forward(q, qv, kc2, vc2, ix3.unsqueeze(2).expand(-1, -1, 2, -1), num_splits=1)
    a = got()
    assert (a["indices"], a["indices_batch_stride"], a["indices_token_stride"], a["indices_head_stride"]) == (ix3.data_ptr(), 120, 40, 0)
    wide = _fake(2, 3, 2, 64, dtype=torch.int32)
    ext.ex_mla_sparse_forward(q, qv, kc2, vc2, wide[..., 8:48], num_splits=1)
    a = got()
    assert (a["indices"], a["indices_batch_stride"], a["indices_token_stride"], a["indices_head_stride"], a["topk"]) == \
        (wide.data_ptr() + 32, 384, 128, 64, 40)
    # the two slices of one (B, cap, 1, 576) pool: each view's own strides and address, no copy; a token-strided qv as it is
    pool = _fake(2, 32, 1, 576)
    wqv = _fake(2, 3, 3, 8, 512)
    ext.ex_mla_sparse_forward(q, wqv[:, :, 1], pool[..., 512:], pool[..., :512], ix3, num_splits=1)
    a = got()
    assert (a["k_cache"], a["v_cache"]) == (pool.data_ptr() + 1024, pool.data_ptr())
    assert (a["k_cache_token_stride"], a["v_cache_token_stride"], a["k_cache_batch_stride"], a["v_cache_batch_stride"]) == (576, 576, 32 * 576, 32 * 576)
    assert (a["qv"], a["qv_token_stride"], a["qv_batch_stride"]) == (wqv.data_ptr() + 2 * 8 * 512, 3 * 8 * 512, 9 * 8 * 512)
    # pools and a table; cache rows
    table = _fake(2, 4, dtype=torch.int32)
    ext.ex_mla_sparse_forward(q, qv, _fake(9, 16, 1, 64), _fake(9, 16, 1, 512), ix3, 17, block_table=table, num_splits=1)
    a = got()
    assert (a["block_table"], a["block_table_row_stride"], a["num_blocks"], a["page_block_size"], a["max_blocks_per_seq"]) == (table.data_ptr(), 4, 9, 16, 4)
    bidx = _fake(2, dtype=torch.int32)
    ext.ex_mla_sparse_forward(q, qv, _fake(5, 32, 1, 64), _fake(5, 32, 1, 512), ix3, cache_batch_idx=bidx, num_splits=1)
    a = got()
    assert (a["cache_batch_idx"], a["cache_batch"], a["block_table"]) == (bidx.data_ptr(), 5, 0)


# ---- the reference against the dense one (tests/mla_ref.py)

def _ref_problem(seed, b=3, nq=2, hq=4, hkv=2, cap=40):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((b, nq, hq, 64), generator=g), torch.randn((b, nq, hq, 512), generator=g),
            torch.randn((b, cap, hkv, 64), generator=g), torch.randn((b, cap, hkv, 512), generator=g), g)


def _close(got, want):
    (o, lse), (ro, rlse) = got, want
    torch.testing.assert_close(o, ro, rtol=1e-11, atol=1e-11)
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin)
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-11, atol=1e-11)


def _full_lists(lens, b, nq, topk, causal):
    """arange(len) (causal: up to each row's bound) padded with -1"""
    ix = torch.full((b, nq, topk), -1, dtype=torch.int32)
    for s in range(b):
        for i in range(nq):
            n = max(0, lens[s] - nq + i + 1) if causal else lens[s]
            ix[s, i, :n] = torch.arange(n, dtype=torch.int32)
    return ix


@pytest.mark.parametrize("causal", (False, True))
def test_reference_with_every_token_listed_is_the_dense_reference(causal):
    q, qv, kc, vc, _g = _ref_problem(1)
    lens = [40, 0, 17]
    sl = torch.tensor(lens, dtype=torch.int32)
    want = mla_ref.mla_reference(q, qv, kc, vc, sl, causal)
    ix = _full_lists(lens, 3, 2, 48, causal)
    _close(mla_sparse_reference(q, qv, kc, vc, ix, sl, causal), want)
    # without the causal cut in the list, the mask makes it
    _close(mla_sparse_reference(q, qv, kc, vc, _full_lists(lens, 3, 2, 48, False), sl, causal), want)
    # a list per K/V head
    _close(mla_sparse_reference(q, qv, kc, vc, ix.unsqueeze(2).repeat(1, 1, 2, 1), sl, causal), want)


def test_reference_does_not_depend_on_the_order_of_a_list():
    q, qv, kc, vc, g = _ref_problem(2)
    lens = [40, 1, 17]
    sl = torch.tensor(lens, dtype=torch.int32)
    ix = _full_lists(lens, 3, 2, 48, False)
    perm = torch.stack([torch.stack([ix[s, i, torch.randperm(48, generator=g)] for i in range(2)]) for s in range(3)])
    assert not torch.equal(perm, ix)
    _close(mla_sparse_reference(q, qv, kc, vc, perm, sl), mla_ref.mla_reference(q, qv, kc, vc, sl))


def test_reference_counts_a_duplicated_entry_twice():
    """a list that names token 5 twice is the dense call on the cache with that token repeated"""
    q, qv, kc, vc, _g = _ref_problem(3, b=1, cap=24)
    n = 20
    ix = torch.full((1, 2, 32), -1, dtype=torch.int32)
    ix[0, :, :n] = torch.arange(n)
    ix[0, :, n] = 5
    kd, vd = torch.cat([kc[:, :n], kc[:, 5:6]], 1), torch.cat([vc[:, :n], vc[:, 5:6]], 1)
    want = mla_ref.mla_reference(q, qv, kd, vd, n + 1)
    got = mla_sparse_reference(q, qv, kc, vc, ix, n)
    _close(got, want)
    assert not torch.allclose(got[1], mla_ref.mla_reference(q, qv, kc, vc, n)[1])


def test_reference_skips_invalid_entries_and_gathers_pages_and_rows():
    q, qv, kc, vc, g = _ref_problem(4)
    lens = [33, 0, 9]
    sl = torch.tensor(lens, dtype=torch.int32)
    clean = torch.full((3, 2, 24), -1, dtype=torch.int32)
    for s in (0, 2):
        for i in range(2):
            clean[s, i, :8] = torch.randint(0, lens[s], (8,), generator=g)
    dirty = torch.full((3, 2, 40), -1, dtype=torch.int32)
    dirty[:, :, 0:16:2] = clean[:, :, :8]                        # the same keys in the same order, with invalid entries between them
    dirty[:, :, 1] = torch.tensor(lens).view(3, 1)               # the first position past each sequence
    dirty[:, :, 3], dirty[:, :, 5], dirty[:, :, 7], dirty[:, :, 20] = 39, -2 ** 31, 2 ** 31 - 1, -7
    dirty[0, :, 9] = 36                                           # inside the cache, past the length
    want = mla_sparse_reference(q, qv, kc, vc, clean, sl)
    got = mla_sparse_reference(q, qv, kc, vc, dirty, sl)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[0][1] == 0).all() and (got[1][1] == -float("inf")).all() and torch.isfinite(got[1][0]).all()
    # causal: an entry above the row's bound is no key (row 0 of sequence 2 sees tokens [0, 8), row 1 [0, 9))
    top = torch.tensor([3, 8, 7, -1], dtype=torch.int32).expand(3, 2, 4).contiguous()
    c = mla_sparse_reference(q, qv, kc, vc, top, sl, True)
    cut = top.clone()
    cut[2, 0, 1] = -1
    c2 = mla_sparse_reference(q, qv, kc, vc, cut, sl, True)
    assert torch.equal(c[0], c2[0]) and torch.equal(c[1], c2[1]) and not torch.equal(c[0][2, 0], c[0][2, 1])
    # pages: token t of sequence b at pool[table[b, t // ps], t % ps], a page outside the pool a zero key with a zero value
    kp, vp = torch.randn((5, 16, 2, 64), generator=g), torch.randn((5, 16, 2, 512), generator=g)
    table = torch.tensor([[3, 1, 9], [0, 0, 0], [4, 4, 2]], dtype=torch.int32)
    from tests.kvcache_paged_ref import paged_tokens
    kg = torch.stack([paged_tokens(kp, table[s], 48, 16) for s in range(3)])
    vg = torch.stack([paged_tokens(vp, table[s], 48, 16) for s in range(3)])
    pl = torch.tensor([40, 3, 48], dtype=torch.int32)
    lists = torch.randint(-3, 50, (3, 2, 2, 24), generator=g).to(torch.int32)
    a = mla_sparse_reference(q, qv, kp, vp, lists, pl, False, None, table)
    b_ = mla_sparse_reference(q, qv, kg, vg, lists, pl)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    # cache rows: a row outside the cache reads zero keys with zero values: o = 0, lse = log(visible entries)
    rows = torch.tensor([2, 7, 0], dtype=torch.int32)
    r = mla_sparse_reference(q, qv, kc, vc, clean, 30, False, 0.1, None, rows)
    s0 = mla_sparse_reference(q[:1], qv[:1], kc[2:], vc[2:], clean[:1], 30, False, 0.1)
    assert torch.equal(r[0][0], s0[0][0]) and (r[0][1] == 0).all()
    nvis = sum(1 for t in clean[1, 0].tolist() if 0 <= t < 30)
    assert nvis == 0 and (r[1][1] == -float("inf")).all()
