"""CPU: the lightning indexer (include/fa_mi355x.h: fa_indexer_pack, fa_indexer_logits, fa_indexer_topk; common/indexer.py) —
declared, exported, the signature rows, every bad argument rejected before any HIP call in the documented order, the empty calls, the
wrappers' refusals, and the reference itself (tests/indexer_ref.py): the baseline without rounding is the reference, the pairwise
table and its bands, the selection model against a brute-force definition, every mutant told apart, the quantiser by hand."""
import ctypes
import functools
import inspect
import itertools
import os
import re

import pytest
import torch

from tests import indexer_ref as ir
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_indexer_pack", "fa_indexer_logits", "fa_indexer_topk")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

PACK_ORDER = ("k", "pool", "seqlens", "table", "b", "nnew", "d", "kb", "kt", "psb", "tsb", "trs", "nblk", "ps", "mb", "pow2")
# B = 2, five new tokens, dense 144-byte tokens, 9 pages of 16, 4 table entries a sequence
PACK = dict(k=P, pool=P, seqlens=P, table=P, b=2, nnew=5, d=128, kb=5 * 128, kt=128, psb=16 * 144, tsb=144, trs=4, nblk=9, ps=16, mb=4, pow2=0)
LOGITS_ORDER = ("q", "w", "pool", "seqlens", "table", "out", "b", "nq", "h", "d", "width", "qb", "qt", "qh", "wb", "wt", "lb", "lr", "psb", "tsb",
                "trs", "nblk", "ps", "mb", "causal")
# B = 2, Nq = 3, 64 heads, width = the capacity 64
LOGITS = dict(q=P, w=P, pool=P, seqlens=P, table=P, out=P, b=2, nq=3, h=64, d=128, width=64, qb=3 * 64 * 128, qt=64 * 128, qh=128, wb=3 * 64,
              wt=64, lb=3 * 64, lr=64, psb=16 * 144, tsb=144, trs=4, nblk=9, ps=16, mb=4, causal=1)
TOPK_ORDER = ("logits", "seqlens", "ix", "b", "nq", "width", "topk", "lb", "lr", "ib", "it", "causal")
TOPK = dict(logits=P, seqlens=P, ix=P, b=2, nq=3, width=64, topk=16, lb=3 * 64, lr=64, ib=3 * 16, it=16, causal=1)
CALLS = dict(fa_indexer_pack=(PACK_ORDER, PACK), fa_indexer_logits=(LOGITS_ORDER, LOGITS), fa_indexer_topk=(TOPK_ORDER, TOPK))


def _call(name, **kw):
    import flashattention_lab_cuda as ext

    order, base = CALLS[name]
    a = dict(base, **kw)
    rc = getattr(ext._lib, name)(*[a[n] for n in order], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS
    for name in ("ex_indexer_pack", "ex_indexer_logits", "ex_indexer_topk", "ex_lightning_indexer"):
        assert hasattr(ext, name), name


def test_signature_rows_and_families_of_their_own():
    import flashattention_lab_cuda as ext

    for name in NAMES:
        names = PROTOTYPES[name][2]
        assert [f for f, _t in ext._SIGNATURES[name][1]] == names and len(names) == len(CALLS[name][0]) + 1   # (all but the stream)
        assert names[-1] == "stream" and PROTOTYPES[name][0] is ctypes.c_int
        assert ext._CALLS[name][2] == len(names)
        assert [n for n, c in ext._CALLS.items() if c[2] == len(names)] == [name]     # no other family is as wide
    assert PROTOTYPES["fa_indexer_pack"][2][:4] == ["k_new", "k_cache", "cache_seqlens", "block_table"]
    assert PROTOTYPES["fa_indexer_logits"][2][:6] == ["q", "weights", "k_cache", "cache_seqlens", "block_table", "logits"]
    assert PROTOTYPES["fa_indexer_topk"][2][:3] == ["logits", "cache_seqlens", "indices"]
    for name in NAMES[:2]:   # the pool and the pages as the packed latent cache names them: one table serves both
        names = PROTOTYPES[name][2]
        at = names.index("page_stride_bytes")
        assert names[at:at + 6] == ["page_stride_bytes", "token_stride_bytes", "block_table_row_stride", "num_blocks", "page_block_size",
                                    "max_blocks_per_seq"]


# every row is rejected before any HIP call: there is no GPU here, and the pointers are fake.  In the documented order: a later
# rule's breach does not hide an earlier one (the rows with two breaches).
A8 = ctypes.c_void_p(4096 + 8)
A2 = ctypes.c_void_p(4096 + 2)
BAD = [
    # ---- fa_indexer_pack
    ("fa_indexer_pack", dict(b=-1), INVALID_ARGUMENT, "batch and seqlen_new must be >= 0"),
    ("fa_indexer_pack", dict(nnew=-1, k=None), INVALID_ARGUMENT, "batch and seqlen_new must be >= 0"),
    ("fa_indexer_pack", dict(k=None, d=64), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_pack", dict(pool=None), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_pack", dict(seqlens=None), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_pack", dict(table=None, tsb=8), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_pack", dict(d=64, kt=8), UNSUPPORTED, "head_dim = 128 only (got 64)"),
    ("fa_indexer_pack", dict(d=512), UNSUPPORTED, "head_dim = 128 only (got 512)"),
    ("fa_indexer_pack", dict(b=2 ** 20, nnew=2 ** 12), UNSUPPORTED, "problem too large"),
    ("fa_indexer_pack", dict(kt=120), INVALID_ARGUMENT, "strides of k_new too small"),
    ("fa_indexer_pack", dict(kb=4 * 128 + 120, tsb=8), INVALID_ARGUMENT, "strides of k_new too small"),
    ("fa_indexer_pack", dict(kb=-8), INVALID_ARGUMENT, "strides of k_new too small"),
    ("fa_indexer_pack", dict(kt=132, kb=5 * 132, tsb=8), INVALID_ARGUMENT, "strides of k_new must be multiples of 8"),
    ("fa_indexer_pack", dict(tsb=132), INVALID_ARGUMENT, "token_stride_bytes must be >= 132 and a multiple of 16 (got 132)"),
    ("fa_indexer_pack", dict(tsb=128, psb=8), INVALID_ARGUMENT, "token_stride_bytes must be >= 132 and a multiple of 16 (got 128)"),
    ("fa_indexer_pack", dict(tsb=2 ** 31, psb=2 ** 36), UNSUPPORTED, "token_stride_bytes"),
    ("fa_indexer_pack", dict(psb=15 * 144 + 128), INVALID_ARGUMENT, "page_stride_bytes must be >= (page_block_size - 1) * token_stride_bytes + 132 = 2292"),
    ("fa_indexer_pack", dict(tsb=208, psb=16 * 144, pool=A8), INVALID_ARGUMENT, "token_stride_bytes + 132 = 3252"),
    ("fa_indexer_pack", dict(psb=16 * 144 + 8), INVALID_ARGUMENT, "page_stride_bytes must be"),
    ("fa_indexer_pack", dict(pool=A8), INVALID_ARGUMENT, "k_cache must be 16-byte aligned"),
    ("fa_indexer_pack", dict(k=A8, ps=8), INVALID_ARGUMENT, "k_new must be 16-byte aligned"),
    ("fa_indexer_pack", dict(seqlens=A2), INVALID_ARGUMENT, "must be 4-byte aligned"),
    ("fa_indexer_pack", dict(table=A2, nblk=0), INVALID_ARGUMENT, "must be 4-byte aligned"),
    ("fa_indexer_pack", dict(ps=8), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 8)"),
    ("fa_indexer_pack", dict(ps=32, psb=32 * 144, nblk=0), INVALID_ARGUMENT, "num_blocks must lie in [1, 2^31)"),
    ("fa_indexer_pack", dict(mb=0), INVALID_ARGUMENT, "max_blocks_per_seq must be >= 1"),
    ("fa_indexer_pack", dict(mb=2 ** 24 + 1, trs=2 ** 25), UNSUPPORTED, "beyond 2^28 tokens"),
    ("fa_indexer_pack", dict(trs=3), INVALID_ARGUMENT, "block_table_row_stride=3 must be >= max_blocks_per_seq=4"),
    # ---- fa_indexer_logits
    ("fa_indexer_logits", dict(b=-1), INVALID_ARGUMENT, "batch and seqlen_q must be >= 0"),
    ("fa_indexer_logits", dict(nq=-2, q=None), INVALID_ARGUMENT, "batch and seqlen_q must be >= 0"),
    # (1) null pointers, before the widths
    ("fa_indexer_logits", dict(q=None, d=64), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_logits", dict(w=None, h=16), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_logits", dict(pool=None), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_logits", dict(seqlens=None), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_logits", dict(table=None), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_logits", dict(out=None, width=0), INVALID_ARGUMENT, "null tensor pointer"),
    # (2) d, then the heads, each with its number
    ("fa_indexer_logits", dict(d=64, h=16), UNSUPPORTED, "head_dim = 128 only (got 64)"),
    ("fa_indexer_logits", dict(d=576), UNSUPPORTED, "head_dim = 128 only (got 576)"),
    ("fa_indexer_logits", dict(h=16, width=0), UNSUPPORTED, "32 or 64 index heads only (got 16)"),
    ("fa_indexer_logits", dict(h=128, qt=128 * 128, qb=3 * 128 * 128, wt=128, wb=3 * 128), UNSUPPORTED, "32 or 64 index heads only (got 128)"),
    ("fa_indexer_logits", dict(h=0), UNSUPPORTED, "32 or 64 index heads only (got 0)"),
    # (3) the width and the launch
    ("fa_indexer_logits", dict(width=0, qh=8), INVALID_ARGUMENT, "width must lie in [1, 2^28] (got 0)"),
    ("fa_indexer_logits", dict(width=2 ** 28 + 1, lr=2 ** 29, lb=2 ** 31), INVALID_ARGUMENT, "width must lie in [1, 2^28]"),
    ("fa_indexer_logits", dict(b=65536), UNSUPPORTED, "problem too large"),
    ("fa_indexer_logits", dict(nq=2 ** 22 + 1, qh=8), UNSUPPORTED, "problem too large"),
    # (4) q, weights, logits, then the pool's two strides and its address, then the alignment
    ("fa_indexer_logits", dict(qh=112), INVALID_ARGUMENT, "head stride of q must lie in [128"),
    ("fa_indexer_logits", dict(qt=63 * 128 + 112, wt=8), INVALID_ARGUMENT, "strides of q too small"),
    ("fa_indexer_logits", dict(qb=2 * 64 * 128), INVALID_ARGUMENT, "strides of q too small"),
    ("fa_indexer_logits", dict(qh=136, qt=64 * 136, qb=3 * 64 * 136), INVALID_ARGUMENT, "strides of q must be multiples of 16"),
    ("fa_indexer_logits", dict(wt=63), INVALID_ARGUMENT, "strides of weights"),
    ("fa_indexer_logits", dict(wb=2 * 64 + 63, lr=8), INVALID_ARGUMENT, "strides of weights"),
    ("fa_indexer_logits", dict(lr=63), INVALID_ARGUMENT, "strides of logits"),
    ("fa_indexer_logits", dict(lb=2 * 64 + 63, tsb=8), INVALID_ARGUMENT, "strides of logits"),
    ("fa_indexer_logits", dict(lb=-64), INVALID_ARGUMENT, "strides of logits"),
    ("fa_indexer_logits", dict(out=A2), INVALID_ARGUMENT, "logits must be 4-byte aligned"),
    ("fa_indexer_logits", dict(tsb=136), INVALID_ARGUMENT, "token_stride_bytes must be >= 132 and a multiple of 16 (got 136)"),
    ("fa_indexer_logits", dict(psb=15 * 144 + 128, q=A8), INVALID_ARGUMENT, "page_stride_bytes must be"),
    ("fa_indexer_logits", dict(pool=A8, q=A8), INVALID_ARGUMENT, "k_cache must be 16-byte aligned"),
    ("fa_indexer_logits", dict(q=A8, ps=8), INVALID_ARGUMENT, "q must be 16-byte aligned"),
    ("fa_indexer_logits", dict(w=A2), INVALID_ARGUMENT, "must be 4-byte aligned"),
    ("fa_indexer_logits", dict(seqlens=A2), INVALID_ARGUMENT, "must be 4-byte aligned"),
    ("fa_indexer_logits", dict(table=A2, mb=0), INVALID_ARGUMENT, "must be 4-byte aligned"),
    # (5) the page geometry
    ("fa_indexer_logits", dict(ps=24, psb=24 * 144), INVALID_ARGUMENT, "page_block_size must be a positive multiple of 16 (got 24)"),
    ("fa_indexer_logits", dict(nblk=0), INVALID_ARGUMENT, "num_blocks must lie in [1, 2^31)"),
    ("fa_indexer_logits", dict(mb=0), INVALID_ARGUMENT, "max_blocks_per_seq must be >= 1"),
    ("fa_indexer_logits", dict(trs=3), INVALID_ARGUMENT, "block_table_row_stride=3 must be >= max_blocks_per_seq=4"),
    # ---- fa_indexer_topk
    ("fa_indexer_topk", dict(b=-1), INVALID_ARGUMENT, "batch and seqlen_q must be >= 0"),
    ("fa_indexer_topk", dict(nq=-1, ix=None), INVALID_ARGUMENT, "batch and seqlen_q must be >= 0"),
    ("fa_indexer_topk", dict(logits=None, topk=0), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_topk", dict(seqlens=None), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_topk", dict(ix=None, width=0), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_indexer_topk", dict(topk=0, width=0), INVALID_ARGUMENT, "topk must lie in [1, 2^20] (got 0)"),
    ("fa_indexer_topk", dict(topk=2 ** 20 + 1, it=2 ** 21, ib=2 ** 23), INVALID_ARGUMENT, "topk must lie in [1, 2^20]"),
    ("fa_indexer_topk", dict(width=0, lr=8), INVALID_ARGUMENT, "width must be >= 1 (got 0)"),
    ("fa_indexer_topk", dict(width=2 ** 28 + 1, lr=2 ** 29, lb=2 ** 31), UNSUPPORTED, "beyond 2^28 keys a row"),
    ("fa_indexer_topk", dict(b=65536, lr=8), UNSUPPORTED, "problem too large"),
    ("fa_indexer_topk", dict(lr=63, it=8), INVALID_ARGUMENT, "strides of logits"),
    ("fa_indexer_topk", dict(lb=2 * 64 + 63), INVALID_ARGUMENT, "strides of logits"),
    ("fa_indexer_topk", dict(logits=A2, it=8), INVALID_ARGUMENT, "logits must be 4-byte aligned"),
    ("fa_indexer_topk", dict(it=15), INVALID_ARGUMENT, "strides of indices"),
    ("fa_indexer_topk", dict(ib=2 * 16 + 15), INVALID_ARGUMENT, "strides of indices"),
    ("fa_indexer_topk", dict(ib=-48, ix=A2), INVALID_ARGUMENT, "strides of indices"),
    ("fa_indexer_topk", dict(ix=A2), INVALID_ARGUMENT, "indices and cache_seqlens must be 4-byte aligned"),
    ("fa_indexer_topk", dict(seqlens=A2), INVALID_ARGUMENT, "indices and cache_seqlens must be 4-byte aligned"),
]


@pytest.mark.parametrize("name,kw,code,what", BAD, ids=[f"{b[0][11:]}{i}" for i, b in enumerate(BAD)])
def test_bad_arguments_are_rejected_before_any_hip_call(name, kw, code, what):
    rc, msg = _call(name, **kw)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith(name + ":"), (kw, msg)


def test_an_empty_call_is_ok_before_anything_is_looked_at():
    for kw in (dict(b=0), dict(nnew=0)):
        rc, msg = _call("fa_indexer_pack", **kw, k=None, pool=None, seqlens=None, table=None, d=7, ps=3, tsb=1)
        assert rc == OK, (kw, msg)
    for kw in (dict(b=0), dict(nq=0)):
        rc, msg = _call("fa_indexer_logits", **kw, q=None, w=None, pool=None, out=None, table=None, d=7, h=5, width=-1, ps=3, tsb=1)
        assert rc == OK, (kw, msg)
        rc, msg = _call("fa_indexer_topk", **kw, logits=None, ix=None, seqlens=None, topk=-5, width=0)
        assert rc == OK, (kw, msg)


class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def test_python_wrappers_refuse_before_anything_runs():
    from common import indexer as ix

    F8, U8, I32, F32 = torch.float8_e4m3fn, torch.uint8, torch.int32, torch.float32
    q, w, pool = _fake(2, 3, 64, 128, dtype=U8).view(F8), _fake(2, 3, 64, dtype=F32), _fake(9, 16, 1, 144, dtype=U8)
    lens, table = _fake(2, dtype=I32), _fake(2, 4, dtype=I32)
    cases = [
        (NotImplementedError, "q of dtype torch.bfloat16", lambda: ix.indexer_logits(_fake(2, 3, 64, 128), w, pool, lens, table)),
        (NotImplementedError, "q of dtype torch.float16", lambda: ix.lightning_indexer(_fake(2, 3, 64, 128, dtype=torch.float16), w, pool, lens, table, 8)),
        (NotImplementedError, "q of dtype torch.float8_e5m2", lambda: ix.indexer_logits(_fake(2, 3, 64, 128, dtype=U8).view(torch.float8_e5m2), w, pool, lens, table)),
        (NotImplementedError, "q of width 64", lambda: ix.indexer_logits(_fake(2, 3, 64, 64, dtype=U8).view(F8), w, pool, lens, table)),
        (NotImplementedError, "16 index heads", lambda: ix.indexer_logits(_fake(2, 3, 16, 128, dtype=U8).view(F8), _fake(2, 3, 16, dtype=F32), pool, lens, table)),
        (NotImplementedError, "weights of dtype torch.bfloat16", lambda: ix.indexer_logits(q, _fake(2, 3, 64), pool, lens, table)),
        (NotImplementedError, "k_cache of dtype torch.bfloat16", lambda: ix.indexer_logits(q, w, _fake(9, 16, 1, 144), lens, table)),
        (NotImplementedError, "cache_seqlens of dtype torch.int64", lambda: ix.indexer_logits(q, w, pool, _fake(2, dtype=torch.int64), table)),
        (NotImplementedError, "block_table of dtype torch.int64", lambda: ix.indexer_logits(q, w, pool, lens, _fake(2, 4, dtype=torch.int64))),
        (NotImplementedError, "block_table of dtype torch.int64", lambda: ix.indexer_pack_cache(_fake(2, 5, 128), pool, lens, _fake(2, 4, dtype=torch.int64))),
        (NotImplementedError, "k_new of dtype torch.float16", lambda: ix.indexer_pack_cache(_fake(2, 5, 128, dtype=torch.float16), pool, lens, table)),
        (NotImplementedError, "k_new of width 512", lambda: ix.indexer_pack_cache(_fake(2, 5, 512), pool, lens, table)),
        (NotImplementedError, "cache_seqlens of dtype torch.int64", lambda: ix.indexer_pack_cache(_fake(2, 5, 128), pool, _fake(2, dtype=torch.int64), table)),
        (NotImplementedError, "logits of dtype torch.bfloat16", lambda: ix.indexer_topk(_fake(2, 3, 64), lens, 8)),
        (NotImplementedError, "cache_seqlens of dtype torch.int64", lambda: ix.indexer_topk(_fake(2, 3, 64, dtype=F32), _fake(2, dtype=torch.int64), 8)),
        (RuntimeError, "q must be 4-D", lambda: ix.indexer_logits(_fake(2, 3, 64 * 128, dtype=U8).view(F8), w, pool, lens, table)),
        (RuntimeError, "weights must be a (B, Nq, H_I)", lambda: ix.indexer_logits(q, _fake(2, 3, 32, dtype=F32), pool, lens, table)),
        (RuntimeError, "k_cache must be (num_blocks", lambda: ix.indexer_logits(q, w, _fake(9, 16, 1, 128, dtype=U8), lens, table)),
        (RuntimeError, "page_block_size", lambda: ix.indexer_logits(q, w, _fake(9, 24, 1, 144, dtype=U8), lens, table)),
        (RuntimeError, "block_table must be", lambda: ix.indexer_logits(q, w, pool, lens, _fake(3, 4, dtype=I32))),
        (RuntimeError, "cache_seqlens must be", lambda: ix.indexer_logits(q, w, pool, _fake(3, dtype=I32), table)),
        (RuntimeError, "must be a GPU", lambda: ix.indexer_logits(torch.zeros((2, 3, 64, 128), dtype=U8).view(F8), w, pool, lens, table)),
        (RuntimeError, "must be a GPU", lambda: ix.indexer_pack_cache(torch.zeros((2, 5, 128), dtype=torch.bfloat16), pool, lens, table)),
        (RuntimeError, "must be a GPU", lambda: ix.indexer_topk(torch.zeros((2, 3, 64)), lens, 8)),
        (RuntimeError, "k_new must be (B, N_new, 128)", lambda: ix.indexer_pack_cache(_fake(2, 5, 1, 128), pool, lens, table)),
        (RuntimeError, "logits must be (B, Nq, width", lambda: ix.indexer_topk(_fake(2, 64, dtype=F32), lens, 8)),
        (RuntimeError, "topk must lie in", lambda: ix.indexer_topk(_fake(2, 3, 64, dtype=F32), lens, 0)),
        (RuntimeError, "seqlen_q = 4", lambda: ix.indexer_topk(_fake(2, 3, 64, dtype=F32), lens, 8, seqlen_q=4)),
        (ValueError, "k_cache must have contiguous 132-byte tokens", lambda: ix.indexer_logits(q, w, _fake(9, 16, 1, 264, dtype=U8)[..., ::2], lens, table)),
    ]
    for exc, what, fn in cases:
        with pytest.raises(exc) as e:
            fn()
        assert what in str(e.value), (what, str(e.value))
    for fn, names in ((ix.indexer_pack_cache, ("scale_pow2",)), (ix.indexer_logits, ("causal", "out", "width")),
                      (ix.indexer_topk, ("seqlen_q", "causal", "out")), (ix.lightning_indexer, ("causal",))):
        for n in names:
            assert inspect.signature(fn).parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(ix.indexer_logits).parameters["causal"].default is True


# ---- the reference itself
@functools.lru_cache(maxsize=None)
def _case(i):
    call = ir.build_call(ir.CASES[i], 100 + i)
    return call, ir.reference(call), ir.baseline(call)


SMALL = [i for i, c in enumerate(ir.CASES) if c["nq"] * c["heads"] * max(c["lens"]) <= 5 * 64 * 1000]   # (the rest: the GPU file's time)


def test_the_table_covers_every_pair_under_its_cap():
    assert len(ir.CASES) <= ir.MAX_CASES and ir.CASES == ir.generate()          # a fixed seed: the same table everywhere
    for a, b in itertools.combinations(ir.AXES, 2):
        assert {(c[a], c[b]) for c in ir.CASES} == set(itertools.product(ir.AXES[a], ir.AXES[b])), (a, b)
    assert {n for c in ir.CASES for n in c["lens"]} == {0, 1, 31, 32, 33, 130, 257, 1000}
    assert any(min(c["lens"]) < c["nq"] for c in ir.CASES) and all(min(c["lens"]) < max(c["nq"], 2) for c in ir.CASES)


@pytest.mark.parametrize("i", SMALL)
def test_the_baseline_without_rounding_is_the_reference_and_no_band_degenerates(i):
    call, ref, base = _case(i)
    b64 = ir.baseline(call, torch.float64, rounding=False)
    vis = ir.visible(call)
    assert torch.equal(torch.isnan(ref), ~vis) and torch.equal(torch.isnan(b64), ~vis) and torch.equal(torch.isnan(base), ~vis)
    assert (b64[vis] - ref[vis]).abs().max().item() <= 1e-10
    assert call["w"].min() < 0 < call["w"].max()                                 # weights of mixed sign
    norms = ir.fp8_ref.e4m3_value(call["k8"]).norm(dim=-1) * call["ks"]
    assert bool((norms[:, -1] > 4 * norms[:, 0]).all())                          # keys whose norm grows along the sequence
    bands = ir.band_errors(base, ref, call["lens"])
    assert len(bands) == sum(-(-n // ir.BAND) for n in call["lens"])
    for _b, _band, err, big in bands:
        assert 0.0 < err < float("inf") and big > 0.0                            # the bound is never the eps term alone
    assert not ir.sharp_bar(base, ref, base, call["lens"])


def test_head_order_is_a_partition_of_the_heads():
    for h in (32, 64):
        a, b = ir.head_order(h, 0), ir.head_order(h, 1)
        assert sorted(a + b) == list(range(h)) and a[:5] == [0, 1, 2, 3, 8] and b[:5] == [4, 5, 6, 7, 12]


def _brute(bits, n, topk):
    """the definition, without a sort: a position is selected iff fewer than topk visible positions beat it"""
    key = [ir.order_key(b) for b in bits[:n]]
    chosen = [j for j in range(n) if sum(1 for m in range(n) if key[m] > key[j] or (key[m] == key[j] and m < j)) < topk]
    return chosen + [-1] * (topk - len(chosen))


def _rows(seed):
    g = torch.Generator().manual_seed(seed)
    sp = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x3F800000, 0xBF800000]
    yield torch.randn(90, generator=g).view(torch.int32).tolist()
    yield torch.randint(-1, 2, (90,), generator=g).float().view(torch.int32).tolist()        # tie-heavy
    yield [0x3F400000] * 90                                                                  # all equal
    yield [sp[int(j)] for j in torch.randint(0, len(sp), (90,), generator=g)]


def test_select_is_the_brute_force_definition():
    for seed in range(3):
        for bits in _rows(seed):
            bits = [b & 0xFFFFFFFF for b in bits]
            for n in (0, 1, 17, 89, 90):
                for topk in (1, 16, 17, 18, 200):
                    assert ir.select(bits, n, topk) == _brute(bits, n, topk), (seed, n, topk)
    assert ir.order_key(0x80000000) < ir.order_key(0) < ir.order_key(0x7F800000) < ir.order_key(0x7FC00000)
    assert ir.order_key(0xFFC00000) < ir.order_key(0xFF800000) < ir.order_key(0xBF800000) < ir.order_key(0x80000000)


def test_select_all_is_select_row_by_row():
    g = torch.Generator().manual_seed(9)
    logits = torch.randint(-2, 3, (3, 4, 70), generator=g).float()
    logits[0, 0, :10] = torch.tensor([0.0, -0.0] * 5)
    logits[1, 1, 5], logits[1, 1, 6] = float("nan"), float("-inf")
    lens = [70, 33, 2]
    for causal in (True, False):
        for topk in (1, 8, 31, 70, 80):
            got = ir.select_all(logits, lens, topk, causal)
            bits = logits.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            for b in range(3):
                for i in range(4):
                    n = ir.visible_count(lens[b], 4, i, causal, 70)
                    assert got[b, i].tolist() == ir.select(bits[b, i].tolist(), n, topk), (causal, topk, b, i)


@pytest.mark.parametrize("mutant", ir.LOGIT_MUTANTS)
def test_every_logit_mutant_fails_the_bar_on_some_case(mutant):
    failed = []
    for i in SMALL:
        call, ref, base = _case(i)
        if ir.sharp_bar(ir.baseline(call, mutant=mutant), ref, base, call["lens"]):
            failed.append(i)
    assert failed, mutant


@pytest.mark.parametrize("mutant", ir.SELECT_MUTANTS)
def test_every_select_mutant_fails_the_exact_comparison(mutant):
    rows = {"ties_to_highest": ([0x3F800000] * 6, 6, 3), "zeros_equal": ([0x80000000, 0x00000000, 0x80000000, 0x00000000], 4, 2),
            "pad_zero": ([0x3F800000] * 3, 3, 5)}
    bits, n, topk = rows[mutant]
    assert ir.select(bits, n, topk, mutant) != ir.select(bits, n, topk)
    assert ir.select([0x80000000, 0, 0x80000000, 0], 4, 2) == [1, 3] and ir.select([0x3F800000] * 6, 6, 3) == [0, 1, 2]
    assert ir.select([5, 6, 7], 3, 5) == [0, 1, 2, -1, -1]
    assert set(ir.MUTANTS) == set(ir.LOGIT_MUTANTS) | set(ir.SELECT_MUTANTS) and len(ir.MUTANTS) == 9


def test_the_quantiser_by_hand():
    x = torch.zeros((4, 128), dtype=torch.bfloat16)
    x[1, 3], x[1, 4], x[1, 5] = 7.0, -3.5, 0.0546875            # amax = 7 = 448 * 2^-6: scale 2^-6 either way
    x[2, 0], x[2, 1] = 3.0, -1.0                                # amax = 3: scale 3 / 448, up to 2^-7 as a power of two
    x[3, 127] = -448.0                                          # amax = 448: scale 1
    codes, scale = ir.pack(x)
    assert scale.tolist() == [1.0, 2.0 ** -6, torch.tensor(3.0).div(torch.tensor(448.0)).item(), 1.0]
    assert bool((codes[0] == 0).all())
    val = ir.fp8_ref.e4m3_value(codes)
    assert val[1, 3] == 448.0 and val[1, 4] == -224.0 and val[1, 5] == 3.5 and val[3, 127] == -448.0
    assert val[2, 0] == 448.0 and val[2, 1] == -144.0           # -149.33 rounds to the e4m3 neighbour -144 (step 16)
    codes2, scale2 = ir.pack(x, scale_pow2=True)
    assert scale2.tolist() == [1.0, 2.0 ** -6, 2.0 ** -7, 1.0]
    val2 = ir.fp8_ref.e4m3_value(codes2)
    assert val2[2, 0] == 384.0 and val2[2, 1] == -128.0 and torch.equal(codes2[1], codes[1])
    tok = ir.token_bytes(codes, scale)
    assert tok.shape == (4, 132) and tok[1, 128:].tolist() == [0, 0, 0x80, 0x3C] and torch.equal(tok[:, :128], codes)
    # scatter: the drop rules
    pool = torch.full((3, 16, 1, 144), 0x7F, dtype=torch.uint8)
    table = torch.tensor([[2, 0], [1, 7]], dtype=torch.int32)
    ir.scatter(pool, tok.view(2, 2, 132), [15, 31], table, 16)
    assert torch.equal(pool[2, 15, 0, :132], tok[0]) and torch.equal(pool[0, 0, 0, :132], tok[1])     # across a page boundary
    assert bool((pool[1] == 0x7F).all()) and bool((pool[..., 132:] == 0x7F).all())                    # page 7, then the capacity
    assert int((pool != 0x7F).any(-1).sum()) == 2
