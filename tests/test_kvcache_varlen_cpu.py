"""CPU: packed (variable-length) queries and new keys in KV-cache decoding (include/fa_mi355x.h: fa_ex_forward_kvcache_varlen,
fa_ex_kvcache_workspace_bytes_varlen) — declared, exported, null arrays equal to fa_ex_forward_kvcache_sink, every host-side
rejection before any HIP call, the workspace formula, the Python wrappers' checks, and the model of the device clamp and of a
wave's rows (tests/kvcache_varlen_ref.py) checked exhaustively on small shapes."""
import ctypes
import inspect
import itertools
import os
import re

import pytest
import torch

from tests import kvcache_varlen_ref as vr
from tests.test_kvcache_cpu import BAD, BASE
from tests.test_kvcache_paged_cpu import NONE as PNONE
from tests.test_kvcache_paged_cpu import PAGED
from tests.test_kvcache_rotary_cpu import NONE as RNONE
from tests.test_kvcache_rotary_cpu import RORDER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_ex_forward_kvcache_varlen", "fa_ex_kvcache_workspace_bytes_varlen")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

# the sink entry point's arguments (cache_dtype 2 = bf16, BASE's dtype), then the five this one adds before the workspace
SORDER = RORDER[:RORDER.index("ws")] + ("cdt", "kd", "vd", "dbs", "sinks", "sheads", "ws", "wsb")
VORDER = SORDER[:SORDER.index("ws")] + ("cuq", "cukn", "tq", "mq", "tkn", "ws", "wsb")
SNONE = dict(cdt=2, kd=None, vd=None, dbs=0, sinks=None, sheads=1)
VNONE = dict(cuq=None, cukn=None, tq=0, mq=0, tkn=0)
# a packed call on BASE's shapes: 5 q tokens at stride H_q d = 512, at most 3 a sequence; 2 new tokens at stride 128
VQ = dict(cuq=P, tq=5, mq=3, nq=0, qb=0)
VK = dict(VQ, cukn=P, tkn=2, nnew=0, knb=0, vnb=0)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **PNONE, **RNONE, **SNONE, **VNONE)
    a.update(kw)
    rc = ext._lib.fa_ex_forward_kvcache_varlen(*[a[n] for n in VORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def _sink(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **PNONE, **RNONE, **SNONE)
    a.update(kw)
    rc = ext._lib.fa_ex_forward_kvcache_sink(*[a[n] for n in SORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_null_arrays_answer_as_the_sink_entry_point(kw, what):
    rc, msg = _call(**kw)
    rc0, msg0 = _sink(**kw)
    assert rc == rc0 == INVALID_ARGUMENT and what in msg
    assert msg == msg0.replace("fa_ex_forward_kvcache_sink:", "fa_ex_forward_kvcache_varlen:")


def test_null_arrays_reach_the_null_pointer_check():
    rc, msg = _call(o=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg
    rc, msg = _call(**PAGED, sinks=P, sheads=8, splits=0, ws=P, wsb=2 ** 40, lse=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg


def _ws_model(hq, total_q, d, s):
    if s <= 1:
        return 0
    rows = total_q * hq * s
    r256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    return r256(rows * d * 4) + r256(rows * 4)   # S * total_q * H_q * (d + 1) floats, each part rounded up to 256 bytes


VARLEN_BAD = [
    # integers without their array
    (dict(tq=5), INVALID_ARGUMENT, "without cu_seqlens_q"), (dict(mq=1), INVALID_ARGUMENT, "without cu_seqlens_q"),
    (dict(tq=-1), INVALID_ARGUMENT, "without cu_seqlens_q"),
    (dict(tkn=2), INVALID_ARGUMENT, "without cu_seqlens_k_new"), (dict(VQ, tkn=2), INVALID_ARGUMENT, "without cu_seqlens_k_new"),
    # cu_seqlens_k_new without cu_seqlens_q, or without the new keys
    (dict(cukn=P, tkn=2), INVALID_ARGUMENT, "cu_seqlens_k_new needs cu_seqlens_q"),
    (dict(VK, kn=None), INVALID_ARGUMENT, "cu_seqlens_k_new needs k_new and v_new"),
    (dict(VK, vn=None), INVALID_ARGUMENT, "cu_seqlens_k_new needs k_new and v_new"),
    (dict(VK, seqlens=None), INVALID_ARGUMENT, "needs cache_seqlens"),
    # max_seqlen_q outside [0, total_q]; totals outside [0, 2^31)
    (dict(VQ, mq=-1), INVALID_ARGUMENT, "max_seqlen_q"), (dict(VQ, mq=6), INVALID_ARGUMENT, "max_seqlen_q"),
    (dict(VQ, tq=0, mq=1), INVALID_ARGUMENT, "max_seqlen_q"),
    (dict(VQ, tq=-3, mq=0), INVALID_ARGUMENT, "total_q"), (dict(VQ, tq=2 ** 31), INVALID_ARGUMENT, "total_q"),
    (dict(VK, tkn=-1), INVALID_ARGUMENT, "total_k_new"), (dict(VK, tkn=2 ** 31), INVALID_ARGUMENT, "total_k_new"),
    (dict(VQ, cuq=ctypes.c_void_p(4098)), INVALID_ARGUMENT, "4-byte aligned"),
    (dict(VK, cukn=ctypes.c_void_p(4097)), INVALID_ARGUMENT, "4-byte aligned"),
    # the token stride of a packed q; one sequence's tokens (max_seqlen_q of them) past 32-bit byte offsets
    (dict(VQ, qt=504), INVALID_ARGUMENT, "strides of q"), (dict(VQ, qt=516), INVALID_ARGUMENT, "multiples of 8"),
    (dict(VQ, tq=2 ** 20, mq=2 ** 12 + 1, qt=2 ** 18), UNSUPPORTED, "beyond 32-bit offsets"),
    (dict(VK, knt=64), INVALID_ARGUMENT, "strides of k_new"),
    # the rotary table bound is capacity + max_seqlen_q
    (dict(VK, rcos=P, rsin=P, rcs=32, rss=32, sro=64 + 2, rdim=64), INVALID_ARGUMENT, "capacity + max_seqlen_q = 67"),
    (dict(VQ, rcos=P, rsin=P, rcs=32, rss=32, sro=64 + 2, rdim=64), INVALID_ARGUMENT, "capacity + max_seqlen_q = 67"),
    # the workspace of a split call is sized by total_q
    (dict(VQ, splits=4, ws=P, wsb=_ws_model(8, 5, 64, 4) - 1), INVALID_ARGUMENT, "workspace"),
    # heads_q * total_q rows are too many for one combine launch (one split: no combine, fine)
    (dict(VQ, tq=2 ** 23, mq=1, splits=2, ws=P, wsb=2 ** 62), UNSUPPORTED, "too many to combine"),
]


@pytest.mark.parametrize("kw,code,what", VARLEN_BAD, ids=[str(i) for i in range(len(VARLEN_BAD))])
def test_varlen_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _call(**kw)   # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_ex_forward_kvcache_varlen:"), (kw, msg)


def test_valid_varlen_arguments_reach_the_null_pointer_check():
    for kw in (VQ, VK, dict(VQ, mq=5), dict(VQ, mq=0), dict(VK, tkn=0), dict(VK, tkn=1000),      # more new tokens than the capacity
               dict(VQ, nq=77, qb=-8), dict(VK, nnew=-4, knb=3, vnb=-1),                          # the padded integers are not used
               dict(VQ, nnew=0, kn=None, vn=None, seqlens=None, knb=0, knt=0, vnb=0, vnt=0),      # packed q without new keys
               dict(VQ, qt=3 * 512),                                                              # qkv[:, 0]
               dict(VQ, tq=2 ** 20, mq=2 ** 12, qt=2 ** 18),                                      # one sequence just below 2^31 bytes
               dict(VQ, tq=2 ** 23, mq=1, splits=1),
               dict(VK, rcos=P, rsin=P, rcs=32, rss=32, sro=64 + 3, rdim=64),
               dict(VQ, **PAGED), dict(VK, sinks=P, sheads=8, splits=0, ws=P, wsb=2 ** 40),
               dict(VQ, splits=4, ws=P, wsb=_ws_model(8, 5, 64, 4))):
        rc, msg = _call(**kw, kc=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
    # without a q token q, o and lse may be null (an append-only call): the cache pointers are still checked
    rc, msg = _call(**dict(VK, tq=0, mq=0), q=None, o=None, lse=None, vc=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg
    # no q token and nothing to append: nothing is launched
    rc, msg = _call(**dict(VK, tq=0, mq=0, tkn=0), q=None, o=None, lse=None)
    assert rc == OK, msg
    rc, msg = _call(**dict(VQ, mq=0), nnew=0, kn=None, vn=None, seqlens=None, knb=0, knt=0, vnb=0, vnt=0)
    assert rc == OK, msg


def test_workspace_bytes_formula():
    import flashattention_lab_cuda as ext

    f = ext._lib.fa_ex_kvcache_workspace_bytes_varlen
    old = ext._lib.fa_ex_kvcache_workspace_bytes
    for b, hq, hkv, tq, mq, cap, d, s in itertools.product((1, 64), (8, 32), (1, 8), (5, 200), (1, 5), (100, 32768), (64, 96),
                                                           (1, 2, 7, 256)):
        assert f(b, hq, hkv, tq, mq, cap, d, s, 0) == _ws_model(hq, tq, d, s)
        assert f(b, hq, hkv, tq, mq, cap, d, s, 1) == _ws_model(hq, tq, d, max(s, 2))
    # num_splits = 0: the padded rule on max_seqlen_q's row tiles, the partials for total_q tokens
    for b, hq, hkv, tq, mq, cap, d in ((64, 32, 8, 191, 128, 8192, 128), (4, 8, 8, 4, 1, 32768, 64), (1, 8, 8, 3, 3, 32, 128)):
        padded = old(b, hq, hkv, mq, cap, d, 0)
        s = 1 if padded == 0 else next(s for s in range(2, 257) if old(b, hq, hkv, mq, cap, d, s) == padded)
        assert f(b, hq, hkv, tq, mq, cap, d, 0, 0) == _ws_model(hq, tq, d, s)
        assert f(b, hq, hkv, tq, mq, cap, d, 0, 1) == _ws_model(hq, tq, d, max(s, 2))
    assert f(1, 8, 8, 3, 3, 32, 128, 0, 0) == 0          # one key tile never splits
    for bad in ((0, 8, 8, 5, 1, 100, 64, 2, 0), (1, 8, 3, 5, 1, 100, 64, 2, 0), (1, 8, 8, 5, 1, 100, 64, 300, 0),
                (1, 8, 8, 0, 0, 100, 64, 2, 0), (1, 8, 8, 5, 0, 100, 64, 2, 0), (1, 8, 8, 5, 6, 100, 64, 2, 0)):
        assert f(*bad) == 0, bad


def test_python_wrapper_rejections():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    q = torch.zeros((5, 4, 64), dtype=torch.bfloat16)
    kc = torch.zeros((2, 16, 2, 64), dtype=torch.bfloat16)
    for name in ("cu_seqlens_q", "cu_seqlens_k_new"):
        for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.int64), [0, 1, 5], 3):
            with pytest.raises(NotImplementedError, match=name + r" of dtype .* \(int32 tensor expected\)"):
                flash_attn_with_kvcache(q, kc, kc, **{name: bad}, max_seqlen_q=1)

    class FakeCuda(torch.Tensor):   # the wrapper's checks run before anything touches the device
        @property
        def is_cuda(self):
            return True

    fq, fk, fq4 = q.as_subclass(FakeCuda), kc.as_subclass(FakeCuda), q.view(1, 5, 4, 64).as_subclass(FakeCuda)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    kn = torch.zeros((3, 2, 64), dtype=torch.bfloat16)
    for fn in (ext.ex_kvcache_forward, flash_attn_with_kvcache):
        with pytest.raises(ValueError, match=r"packed \(total_q, H_q, d\)"):      # a 4-D q with cu_seqlens_q
            fn(fq4, fk, fk, cu_seqlens_q=cu, max_seqlen_q=3)
        with pytest.raises(ValueError, match="needs max_seqlen_q"):
            fn(fq, fk, fk, cu_seqlens_q=cu)
        with pytest.raises(ValueError, match="max_seqlen_q"):
            fn(fq, fk, fk, cu_seqlens_q=cu, max_seqlen_q=6)
        with pytest.raises(ValueError, match="cu_seqlens_k_new needs cu_seqlens_q"):
            fn(fq4, fk, fk, cu_seqlens_k_new=cu)
        with pytest.raises(ValueError, match="max_seqlen_q needs cu_seqlens_q"):
            fn(fq4, fk, fk, max_seqlen_q=3)
        with pytest.raises(ValueError, match="cu_seqlens_k_new needs k and v"):
            fn(fq, fk, fk, cu_seqlens_q=cu, cu_seqlens_k_new=cu, max_seqlen_q=3)
        with pytest.raises(RuntimeError, match=r"int32 \(B \+ 1,\)"):               # lengths that disagree; a single offset
            fn(fq, fk, fk, cu_seqlens_q=cu, cu_seqlens_k_new=cu[:2], max_seqlen_q=3)
        with pytest.raises(RuntimeError, match=r"int32 \(B \+ 1,\)"):
            fn(fq, fk, fk, cu_seqlens_q=cu[:1], max_seqlen_q=3)
        with pytest.raises(RuntimeError, match=r"packed \(total_k_new, H_kv, d\)"):
            fn(fq, fk, fk, kn.view(1, 3, 2, 64), kn.view(1, 3, 2, 64), cu_seqlens_q=cu, cu_seqlens_k_new=cu, max_seqlen_q=3)
        # a packed q the library cannot take without a copy: a strided last dim, heads apart, an odd token stride, a misaligned view
        for bad in (torch.zeros((5, 4, 128), dtype=torch.bfloat16)[..., ::2], torch.zeros((5, 64, 4), dtype=torch.bfloat16).transpose(1, 2),
                    torch.zeros((5, 4 * 64 + 4), dtype=torch.bfloat16)[:, :256].view(5, 4, 64),
                    torch.zeros((5 * 256 + 4,), dtype=torch.bfloat16)[4:].view(5, 4, 64)):
            with pytest.raises(ValueError, match="never copied"):
                fn(bad.as_subclass(FakeCuda), fk, fk, cu_seqlens_q=cu, max_seqlen_q=3)
        # the cache's batch dim is B = len(cu_seqlens_q) - 1, not total_q
        with pytest.raises(RuntimeError, match=r"\(B, cache_len, H_kv, d\)"):
            fn(fq, fk, fk, cu_seqlens_q=torch.tensor([0, 1, 2, 5], dtype=torch.int32), max_seqlen_q=3)
    # keyword-only, behind FlashAttention-2's positional order; the e4m3 scales stay the trailing keywords
    for fn in (ext.ex_kvcache_forward, flash_attn_with_kvcache):
        params = inspect.signature(fn).parameters
        for name in ("cu_seqlens_q", "cu_seqlens_k_new", "max_seqlen_q"):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None


# ---- the model of the device clamp and of a wave's rows, exhaustively
def _arrays(b, total):
    vals = (-2 ** 31, -1) + tuple(range(total + 2)) + (2 ** 31 - 1,)
    return itertools.product(vals, repeat=b + 1)


def test_clamp_and_row_model_exhaustive():
    checked = formed = 0
    for b, total_q, g in itertools.product((1, 2, 3), range(7), (1, 4)):
        for max_q in range(min(4, total_q) + 1):
            tiles = vr.row_tiles(max_q, g)
            assert tiles == -(-max_q * g // 16)
            for cu in _arrays(b, total_q):
                ok = vr.well_formed(cu, total_q, max_q)
                for seq in range(b):
                    start, nq = vr.cu_range(cu, seq, total_q, max_q)
                    assert 0 <= start <= total_q and 0 <= nq <= max_q and start + nq <= total_q
                    got = []
                    for rt in range(tiles):
                        rows = vr.tile_rows(cu, seq, rt, total_q, max_q, g)
                        if rows is None:                        # the early exit: nothing of this tile exists
                            assert 16 * rt >= g * nq
                            continue
                        assert 0 < len(rows) <= 16
                        got.extend(rows)
                    assert all(0 <= t < total_q and 0 <= h < g for t, h in got)      # every packed row inside q / o / lse
                    assert len(set(got)) == len(got) == g * nq                        # the grid covers the sequence, once
                    if ok:   # well-formed offsets are reproduced exactly
                        assert (start, nq) == (cu[seq], cu[seq + 1] - cu[seq])
                        assert got == [(t, h) for t in range(cu[seq], cu[seq + 1]) for h in range(g)]
                    checked += 1
                formed += ok
    assert checked > 10 ** 5 and formed > 100


def test_clamp_of_new_keys_against_the_capacity():
    # the same clamp with the capacity for a bound: nnew_b <= capacity, so L_b = clamp(seqlens, 0, capacity - nnew_b) >= 0
    for cap, total in itertools.product((1, 3, 16), (0, 2, 5, 40)):
        for cu in _arrays(2, min(total, 4)):
            for seq in range(2):
                start, n = vr.cu_range(cu, seq, total, cap)
                assert 0 <= start <= total and 0 <= n <= min(cap, total - start)
                for seqlen in (-5, 0, cap - 1, cap, cap + 7):
                    L = min(max(seqlen, 0), cap - n)
                    assert 0 <= L and L + n <= cap
    assert vr.lengths_to_cu([1, 0, 5, 20, 3]) == [0, 1, 1, 6, 26, 29]
