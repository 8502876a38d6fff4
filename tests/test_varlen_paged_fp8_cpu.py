"""CPU: an e4m3 pool under the paged varlen forward (flash_attention_varlen with block_table, k_descale, v_descale;
include/fa_mi355x.h: fa_ex_forward_varlen_paged_fp8) — declared and exported, every host-side validation before any HIP call,
cache_dtype == dtype as the parent call, the Python wrappers' errors, and a model of the MFMA kernel's e4m3 staging: a block of
16 keys per wave, which no page boundary cuts."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.test_varlen_paged_cpu import BASE, INVALID_ARGUMENT, OK, ORDER, P, UNSUPPORTED
from tests.varlen_paged_ref import pg_slot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
E4M3_CODE = 3
# the parent call's arguments, then cache_dtype, k_descale, v_descale, descale_batch_stride (in front of stream)
BASE8 = dict(BASE, cache=E4M3_CODE, kd=P, vd=P, dbs=2)
ORDER8 = ORDER + ("cache", "kd", "vd", "dbs")


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE8, **kw)
    rc = ext._lib.fa_ex_forward_varlen_paged_fp8(*[a[n] for n in ORDER8], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbol():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bfa_ex_forward_varlen_paged_fp8\s*\(([^;]*)\)\s*;", src)
    assert m and re.search(r"int cache_dtype,\s*const float\*\s*k_descale,\s*const float\*\s*v_descale,\s*int64_t descale_batch_stride,\s*void\*\s*stream$",
                           " ".join(m.group(1).split()))
    assert hasattr(ctypes.CDLL(ext.LIBRARY_PATH), "fa_ex_forward_varlen_paged_fp8")
    assert "fa_ex_forward_varlen_paged_fp8" in ext.EXPORTED_C_SYMBOLS


BAD = [
    (dict(cache=1), "cache_dtype"), (dict(cache=0), "cache_dtype"), (dict(cache=7), "cache_dtype"),
    (dict(cache=2), "need an e4m3 pool"), (dict(cache=2, kd=None), "need an e4m3 pool"),           # a scale with a 16-bit pool
    (dict(cache=2, kd=None, vd=None), "descale_batch_stride must be 0 with a 16-bit pool"),
    (dict(dbs=-1), "descale_batch_stride"), (dict(dbs=1), "descale_batch_stride"),                  # negative; non-zero below heads_kv
    (dict(kd=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(vd=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(k=ctypes.c_void_p(4100)), "8-byte aligned"), (dict(v=ctypes.c_void_p(4098)), "8-byte aligned"),
    (dict(dtype=0), "dtype must be f16 or bf16"),
    (dict(d=20, sq=80, sk=40, sv=40, kps=640, vps=640), "multiple of 8"),
    (dict(sk=132, kps=16 * 132), "multiples of 8"), (dict(kps=16 * 128 + 4), "multiples of 8"),
    # the parent's list still holds
    (dict(ps=24), "page_block_size"), (dict(table=None), "null block_table"), (dict(sk=64), "token strides"),
    (dict(kps=15 * 128), "page strides"), (dict(hkv=3, dbs=0), "heads_q"), (dict(scale=float("nan")), "softmax_scale"),
]


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_arguments_are_rejected_before_any_hip_call(kw, what):
    rc, msg = _call(**kw)
    assert rc == INVALID_ARGUMENT and what in msg and msg.startswith("fa_ex_forward_varlen_paged_fp8:"), (kw, msg)


def test_the_page_limit_is_on_bytes():
    # a page of 15 * 2^27 + 128 elements: beyond 2^31 bytes as bf16, below as e4m3
    big = dict(sk=2 ** 27, sv=2 ** 27, kps=2 ** 31, vps=2 ** 31, o=None)
    rc, msg = _call(**big)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg
    rc, msg = _call(**big, cache=2, kd=None, vd=None, dbs=0)
    assert rc == UNSUPPORTED and "page" in msg, msg
    rc, msg = _call(**dict(big, sk=2 ** 28, kps=2 ** 32))
    assert rc == UNSUPPORTED and "page" in msg, msg


def test_valid_arguments_reach_the_null_pointer_check_or_return():
    # null scales (1.0); the (H_kv,) form; 8- but not 16-byte aligned pools; strides that are multiples of 8 only; ps no power of two
    for kw in (dict(kd=None, vd=None, dbs=0), dict(kd=None), dict(dbs=0), dict(dbs=2 ** 20), dict(k=ctypes.c_void_p(4104), v=ctypes.c_void_p(4104)),
               dict(sk=136, kps=16 * 136 + 8), dict(ps=48, kps=48 * 128, vps=48 * 128), dict(dtype=1)):
        rc, msg = _call(**kw, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
    for kw in (dict(total_q=0), dict(max_q=0)):
        rc, msg = _call(**kw, o=None)
        assert rc == OK, (kw, msg)


def test_cache_dtype_equal_to_dtype_is_the_parent_call():
    import flashattention_lab_cuda as ext

    def parent(**kw):
        a = dict(BASE, **kw)
        rc = ext._lib.fa_ex_forward_varlen_paged(*[a[n] for n in ORDER], None)
        return rc, ext._lib.fa_last_error().decode()

    same = dict(kd=None, vd=None, dbs=0)
    for kw in (dict(o=None), dict(ps=8), dict(table=None), dict(sv=127), dict(kps=15 * 128), dict(dtype=7), dict(dtype=0, o=None),
               dict(d=20, sq=80, sk=40, sv=40, kps=640, vps=640, o=None), dict(k=ctypes.c_void_p(4100), o=None), dict(total_q=0),
               dict(ps=65536 + 16, kps=(65536 + 16) * 128, vps=(65536 + 16) * 128), dict(sk=2 ** 27, kps=2 ** 31)):
        rc0, msg0 = parent(**kw)
        rc1, msg1 = _call(**kw, cache=kw.get("dtype", BASE["dtype"]), **same)
        assert rc0 == rc1 and msg0.split(":", 1)[1:] == msg1.split(":", 1)[1:], (kw, msg0, msg1)


def test_keywords_of_the_public_functions():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_varlen

    for fn in (flash_attention_varlen, ext.ex_varlen_forward):
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps[-4:]] == ["block_table", "k_descale", "v_descale", "sinks"]
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None for p in ps[-4:])


def test_python_wrapper_rejections():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_varlen

    class FakeCuda(torch.Tensor):   # the wrapper's checks run before anything touches the device
        @property
        def is_cuda(self):
            return True

    bf = torch.bfloat16
    q = torch.zeros((40, 4, 64), dtype=bf).as_subclass(FakeCuda)
    pool = torch.zeros((9, 16, 2, 64), dtype=bf).as_subclass(FakeCuda)
    pool8 = torch.zeros((9, 16, 2, 64), dtype=torch.uint8).view(torch.float8_e4m3fn).as_subclass(FakeCuda)
    cu = torch.tensor([0, 8, 40], dtype=torch.int32).as_subclass(FakeCuda)
    table = torch.zeros((2, 4), dtype=torch.int32).as_subclass(FakeCuda)
    sc = torch.ones((2, 2)).as_subclass(FakeCuda)
    calls = (lambda k, v, **kw: ext.ex_varlen_forward(q, k, v, cu, cu, 32, 64, True, 0.125, **kw),
             lambda k, v, **kw: flash_attention_varlen(q, k, v, cu, cu, 32, 64, causal=True, **kw))
    for call in calls:
        # other float8 dtypes: the decode call's text
        for name in ("float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz"):
            if not hasattr(torch, name):
                continue
            other = torch.zeros((9, 16, 2, 64), dtype=torch.uint8).view(getattr(torch, name)).as_subclass(FakeCuda)
            with pytest.raises(NotImplementedError, match=r"is not supported \(an 8-bit cache is torch.float8_e4m3fn\)"):
                call(other, other, block_table=table)
            with pytest.raises(NotImplementedError, match=r"is not supported \(an 8-bit cache is torch.float8_e4m3fn\)"):
                call(pool8, other, block_table=table)
        # K and V both e4m3, or neither
        for k, v in ((pool8, pool), (pool, pool8)):
            with pytest.raises(RuntimeError, match="both"):
                call(k, v, block_table=table)
        # scales without e4m3 pools
        for kw in (dict(k_descale=sc), dict(v_descale=sc)):
            with pytest.raises(RuntimeError, match="k_descale / v_descale need"):
                call(pool, pool, block_table=table, **kw)
            with pytest.raises(RuntimeError, match="k_descale / v_descale need"):
                call(q, q, **kw)
        # an e4m3 pool without block_table
        with pytest.raises(RuntimeError, match="need block_table"):
            call(pool8, pool8)
        # the scales: dtype and shape by the decode call's helper
        with pytest.raises(NotImplementedError, match=r"k_descale of dtype .* \(float32 tensor expected\)"):
            call(pool8, pool8, block_table=table, k_descale=sc.double())
        with pytest.raises(RuntimeError, match=r"v_descale must be float32 of shape \(B, H_kv\) = \(2, 2\) or \(H_kv,\)"):
            call(pool8, pool8, block_table=table, v_descale=torch.ones((3, 2)).as_subclass(FakeCuda))
        # a pool view that would need a copy
        strided = torch.zeros((9, 16, 2, 128), dtype=torch.uint8).view(torch.float8_e4m3fn)[..., ::2].as_subclass(FakeCuda)
        with pytest.raises(ValueError, match="never copied"):
            call(strided, pool8, block_table=table)
    # q must be 16-bit with e4m3 pools
    with pytest.raises(RuntimeError, match="16-bit dtype"):
        ext.ex_varlen_forward(q.float(), pool8, pool8, cu, cu, 32, 64, True, 0.125, block_table=table)


def block_fetches(D, ps, length, tile0):
    """The 128-key tile at `tile0` of a sequence of `length` keys as the MFMA kernel stages an e4m3 pool: wave w of 8 owns the block of
    16 keys at tile0 + 16 w (one table entry, one descriptor) and moves it as 16 D / 256 loads of 256 / D rows each.  Per load:
    (first key, rows below `length`, table slot), the slot clamped to the last one in use as the kernel does."""
    rpi = 256 // D
    last = (max(length, 1) - 1) // ps
    out = []
    for w in range(8):
        key0 = tile0 + 16 * w
        rows = max(min(16, length - key0), 0)        # the descriptor's num_records cuts the block here
        slot = min(pg_slot(key0, ps), last)
        for j in range(16 // rpi):
            out.append((key0 + rpi * j, max(min(rpi, rows - rpi * j), 0), slot))
    return out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("ps", [16, 48, 256])
def test_no_block_straddles_a_page_and_every_key_is_fetched_once(D, ps):
    rpi = 256 // D
    for length in (1, 15, 16, 17, 127, 128, 129, 300, 2 * ps, 2 * ps + 1, 3 * ps - 1, 5 * 128):
        seen, top = [], -1
        for tile0 in range(0, length, 128):
            loads = block_fetches(D, ps, length, tile0)
            assert sorted(k for k, _r, _s in loads) == list(range(tile0, tile0 + 128, rpi))   # the staging area is fully written
            for key, rows, slot in loads:
                if rows == 0:
                    assert key >= length
                    continue
                block = key - (key - tile0) % 16
                assert block // ps == (block + 15) // ps == slot, (D, ps, length, key)   # the whole block inside one page
                seen += list(range(key, key + rows))
                top = max(top, slot)
            assert max(s for _k, _r, s in loads) <= (length - 1) // ps
        assert sorted(seen) == list(range(length))
        assert top == (length + ps - 1) // ps - 1
