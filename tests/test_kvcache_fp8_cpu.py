"""CPU: the e4m3 KV cache of KV-cache decoding (include/fa_mi355x.h: fa_ex_forward_kvcache_fp8) — that every finite e4m3 value is
exact in float16 and bfloat16 (the kernels' dequantisation rests on it), the append's quantisation recipe of
tests/kvcache_fp8_ref.py against the correctly rounded quantisation on the GPU tests' own inputs, and the C layer's argument
checks that need no device."""
import ctypes
import os
import re

import pytest
import torch

from tests.kvcache_fp8_ref import E4M3, FIXED_SCALES, absmax_scales, dequantize, neighbours, quantize, quantize_exact, randn16
from tests.test_kvcache_cpu import BASE
from tests.test_kvcache_paged_cpu import NONE as PNONE
from tests.test_kvcache_rotary_cpu import NONE as RNONE
from tests.test_kvcache_rotary_cpu import RORDER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
INVALID_ARGUMENT = -1
E4M3_CODE = 3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

# the arguments fa_ex_forward_kvcache_fp8 adds, between rotary_interleaved and the workspace
EXTRA = ("cdt", "kd", "vd", "dbs")
FORDER = RORDER[:RORDER.index("ws")] + EXTRA + ("ws", "wsb")
# BASE: bf16, 2 sequences, 2 K/V heads, d = 64, cache_len = 64; as an e4m3 cache its strides (elements) are bytes
FP8 = dict(cdt=E4M3_CODE, kd=P, vd=P, dbs=2)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **PNONE, **RNONE, cdt=BASE["dtype"], kd=None, vd=None, dbs=0)
    a.update(kw)
    rc = ext._lib.fa_ex_forward_kvcache_fp8(*[a[n] for n in FORDER], None)
    return rc, ext._lib.fa_last_error().decode()


# ---- 1. representability

FINITE = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)


def test_every_finite_code_is_exact_in_both_16_bit_dtypes():
    assert FINITE.numel() == 254
    vals = FINITE.view(E4M3)
    assert torch.isfinite(vals.float()).all() and vals.float().abs().max() == 448.0
    for dtype in (torch.float16, torch.bfloat16):
        wide = vals.to(dtype)
        assert torch.equal(wide.double(), vals.double()), dtype            # exact on the way up
        assert torch.equal(wide.to(E4M3).view(torch.uint8), FINITE), dtype   # and the same byte on the way back
    nz = vals.double().abs()[vals.double() != 0]
    assert nz.min() == 2.0 ** -9 and nz.max() == 448.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_quantize_saturates_and_keeps_the_sign_of_zero(dtype):
    x = torch.tensor([1e4, -1e4, 449.0, -449.0, 6e4, -6e4, 0.0, -0.0, 448.0, -448.0, 1.0], dtype=dtype).view(1, 1, 1, -1)
    for ds in (1.0, 2.0 ** -5, 1e-4, 0.0137):
        c = quantize(x, torch.tensor([ds])).view(-1)
        assert (c & 0x7f != 0x7f).all(), ds                                 # never the NaN code
        assert c[:6].tolist() == [0x7e, 0xfe] * 3, (ds, c.tolist())
        assert c[6].item() == 0x00 and c[7].item() == 0x80
    ds = torch.tensor([1e-3, 1.0])
    sign = torch.where(randn16((1, 50, 2, 64), dtype, 1) >= 0, 1.0, -1.0)
    big = (sign * 1e4 * ds.view(1, 1, 2, 1)).to(dtype)                    # |x| = 10^4 descale: |x / descale| far above 448
    c = quantize(big, ds)
    assert torch.equal(c, torch.where(sign > 0, 0x7e, 0xfe).to(torch.uint8))


# ---- 2. the recipe against the correctly rounded quantisation, on the GPU tests' inputs

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_recipe_is_within_the_cap_of_the_exact_rounding(dtype):
    """The GPU test allows the kernel's bytes to differ from quantize() on 1 element in 10^3.  quantize() itself (fp32 multiply
    by the rounded reciprocal) differs from the correctly rounded quotient on well under that share, and always returns one of
    the two codes that bracket the exact quotient."""
    x = randn16((4, 300, 2, 128), dtype, 77)
    scales = [absmax_scales(x), absmax_scales(x, per_batch=False)] + [torch.full((2,), s) for s in FIXED_SCALES]
    for ds in scales:
        got, exact = quantize(x, ds), quantize_exact(x, ds)
        lo, hi = neighbours(x, ds)
        assert bool(((got == lo) | (got == hi)).all()), ds
        assert bool(((exact == lo) | (exact == hi)).all()), ds
        share = (got != exact).double().mean().item()
        print(f"{dtype} scale {ds.flatten()[:2].tolist()}: quantize != quantize_exact on {share:.2e} of {x.numel()} elements")
        assert share <= 1e-3, (ds, share)
        # the dequantised value is within half a step of x (relative 2^-4 for normal codes) unless saturated
        back = dequantize(got, ds)
        sat = (got & 0x7f) == 0x7e
        err = (back - x.double()).abs()[~sat]
        bound = (x.double().abs() * 2.0 ** -4 + 2.0 ** -10 * float(ds.max()))[~sat]
        assert bool((err <= bound).all())


# ---- 3. the C layer

def test_header_declares_and_library_exports_the_symbol():
    import flashattention_lab_cuda as ext

    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bfa_ex_forward_kvcache_fp8\s*\(", src)
    assert re.search(r"#define\s+FA_DTYPE_E4M3\s+3\b", text)
    assert hasattr(ctypes.CDLL(ext.LIBRARY_PATH), "fa_ex_forward_kvcache_fp8")
    assert "fa_ex_forward_kvcache_fp8" in ext.EXPORTED_C_SYMBOLS


FP8_BAD = [
    (dict(kd=P), "k_descale"), (dict(vd=P), "k_descale"), (dict(kd=P, vd=P, dbs=2), "k_descale"),           # scales, 16-bit cache
    (dict(dbs=2), "descale_batch_stride"),                                                                 # a stride, 16-bit cache
    (dict(cdt=1), "cache_dtype"), (dict(cdt=0), "cache_dtype"), (dict(cdt=4), "cache_dtype"), (dict(cdt=-1), "cache_dtype"),
    (dict(FP8, dbs=-1), "descale_batch_stride"), (dict(FP8, dbs=-2 ** 40), "descale_batch_stride"),
    (dict(FP8, dbs=1), "descale_batch_stride"),                                                            # 0 < stride < heads_kv
    (dict(FP8, kc=ctypes.c_void_p(4100)), "8-byte aligned"), (dict(FP8, vc=ctypes.c_void_p(4097)), "8-byte aligned"),
    (dict(FP8, kd=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(FP8, vd=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(FP8, kct=132, kcb=64 * 132), "multiples of 8"),
]


@pytest.mark.parametrize("kw,what", FP8_BAD, ids=[str(i) for i in range(len(FP8_BAD))])
def test_fp8_arguments_are_rejected_before_any_hip_call(kw, what):
    rc, msg = _call(**kw)   # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == INVALID_ARGUMENT, (kw, msg)
    assert what in msg and msg.startswith("fa_ex_forward_kvcache_fp8:"), (kw, msg)


def test_valid_fp8_arguments_reach_the_null_pointer_check():
    for kw in (dict(), dict(FP8), dict(FP8, dbs=0), dict(FP8, kd=None), dict(FP8, kd=None, vd=None, dbs=0), dict(FP8, dbs=7),
               dict(FP8, kc=ctypes.c_void_p(4104), vc=ctypes.c_void_p(4096 + 64 * 128))):   # 8-byte, not 16-byte, aligned
        rc, msg = _call(**kw, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)


def test_16_bit_cache_dtype_answers_as_the_rotary_entry_point():
    import flashattention_lab_cuda as ext

    for kw in (dict(d=60), dict(kct=64), dict(splits=300), dict(o=None)):
        rc, msg = _call(**kw)
        a = dict(BASE, **PNONE, **RNONE)
        a.update(kw)
        rc0 = ext._lib.fa_ex_forward_kvcache_rotary(*[a[n] for n in RORDER], None)
        msg0 = ext._lib.fa_last_error().decode()
        assert rc == rc0 == INVALID_ARGUMENT
        assert msg == msg0.replace("fa_ex_forward_kvcache_rotary:", "fa_ex_forward_kvcache_fp8:")


def test_span_limit_is_in_bytes():
    """A batch element of 2^30 + 2^29 elements: beyond 32-bit offsets at 2 bytes an element, inside them at 1."""
    tokens = 3 * 2 ** 21
    big = dict(cap=tokens, kcb=tokens * 256, vcb=tokens * 256, kct=256, vct=256, hkv=4, hq=8, knb=256, knt=256, vnb=256, vnt=256)   # 4 heads x 64
    rc, msg = _call(**big, o=None)
    assert rc != 0 and "spans" in msg and "k_cache" in msg, msg
    rc, msg = _call(**dict(FP8, **big, dbs=4), o=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg
    huge = dict(big, cap=2 * tokens, kcb=2 * tokens * 256, vcb=2 * tokens * 256)
    rc, msg = _call(**dict(FP8, **huge, dbs=4), o=None)
    assert rc != 0 and "spans" in msg, msg


def test_python_signatures_take_the_scales_as_trailing_keywords():
    import inspect

    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    for fn in (ext.ex_kvcache_forward, flash_attn_with_kvcache):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["k_descale", "v_descale"], names
