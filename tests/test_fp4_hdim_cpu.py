"""No GPU: the argument checks of the MXFP4 cache calls at head dims 64 / 128 / 256 (fa_fp4_*_hdim, the shim's hdim=True,
common.mxfp4_attention).  Every refusal here happens before a launch."""
import ctypes

import pytest
import torch

import flashattention_lab_cuda as ext

E4 = torch.float8_e4m3fn


def arrays(d, lead=(2, 16), hkv=2):
    return [torch.zeros((*lead, hkv, *w), dtype=torch.uint8) for w in ((d // 2,), (d // 32,), (d // 2,), ())]


@pytest.mark.parametrize("d", (96, 192))
def test_entry_points_refuse_other_head_dims(d):
    """the C layer, called with host pointers it never follows: the head dim is its first rule after the null checks"""
    lib, want = ext._lib, f"head_dim {d} is not supported (64, 128 or 256)".encode()
    buf = ctypes.addressof(ctypes.create_string_buffer(64)) + 15 & ~15
    a = lib.fa_fp4_kvcache_append_hdim(buf, buf, buf, buf, buf, buf, buf, 0, 0, 0, 0, 1, 1, 1, 16, 0, d, 2, *([0] * 16), 0)
    assert a != 0 and want in lib.fa_last_error()
    kv = lib.fa_fp4_forward_kvcache_hdim(*([buf] * 7), *([0] * 6), 1, 1, 1, 1, 16, 0, d, 2, *([0] * 16), 0, 1.0, 1, 0, 0, 0, -1, -1, 0.0, 0, 0)
    assert kv != 0 and want in lib.fa_last_error()
    vl = lib.fa_fp4_forward_varlen_hdim(*([buf] * 7), 0, 0, 0, buf, buf, buf, 1, 1, 1, 1, 1, 16, d, 2, *([0] * 15), 0, 1.0, 0, -1, -1, 0.0, 0, 0)
    assert vl != 0 and want in lib.fa_last_error()
    assert lib.fa_fp4_forward_kvcache_hdim_workspace_bytes(4, 8, 2, 1, 4096, d, 4, 0, -1, -1, 0) == 0


@pytest.mark.parametrize("shape", ((4, 8, 2, 1, 4096, 4, 0, -1, -1, 0), (2, 8, 2, 9, 65536, 0, 1, 128, -1, 1)))
def test_workspace_at_128_is_the_mod_one(shape):
    b, hq, hkv, nq, cap, *rest = shape
    at = lambda d: ext._lib.fa_fp4_forward_kvcache_hdim_workspace_bytes(b, hq, hkv, nq, cap, d, *rest)   # noqa: E731
    assert at(128) == ext._lib.fa_fp4_forward_kvcache_workspace_bytes_mod(b, hq, hkv, nq, cap, 128, *rest)
    if rest[0] > 1:
        assert 0 < at(64) < at(128) < at(256)


def test_mixed_widths_are_named_and_other_dims_refused():
    from common.mxfp4_attention import mxfp4_append, mxfp4_decode, mxfp4_prefill

    kc, ks, vc, vs = arrays(64)
    q = torch.zeros((2, 1, 8, 64)).to(E4)
    with pytest.raises(RuntimeError, match=r"q 64, k_cache 64, k_scale 256, v_cache 64"):
        mxfp4_decode(q, kc, arrays(256)[1], vc, vs)
    with pytest.raises(RuntimeError, match=r"k_new 256, k_cache 64, k_scale 64, v_cache 64"):
        mxfp4_append(torch.zeros((2, 1, 2, 256), dtype=torch.bfloat16), torch.zeros((2, 1, 2, 256), dtype=torch.bfloat16), kc, ks, vc, vs, cache_seqlens=0)
    cu = torch.tensor([0, 1, 2], dtype=torch.int32)
    for d in (96, 192):
        with pytest.raises(NotImplementedError, match=f"head_dim {d} is not supported \\(64, 128 or 256\\)"):
            mxfp4_prefill(torch.zeros((2, 8, d)).to(E4), *arrays(d), cu, cu, 1, 16, block_table=torch.zeros((2, 1), dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="q of dtype torch.bfloat16"):
        mxfp4_decode(q.bfloat16(), kc, ks, vc, vs)
    for name in ("cache_leftpad", "qv", "rotary_cos", "alibi_slopes", "attn_bias"):
        with pytest.raises(NotImplementedError, match=name):
            mxfp4_decode(q, kc, ks, vc, vs, **{name: torch.zeros(1)})


def test_the_old_wrappers_still_refuse_64():
    import common.fp4_kvcache as old

    kc, ks, vc, vs = arrays(64)
    q, cu = torch.zeros((2, 1, 8, 64)).to(E4), torch.tensor([0, 1, 2], dtype=torch.int32)
    k = torch.zeros((2, 1, 2, 64), dtype=torch.bfloat16)
    table = torch.zeros((2, 1), dtype=torch.int32)
    calls = [lambda: old.mxfp4_kvcache_append(k, k, kc, ks, vc, vs, cache_seqlens=0),
             lambda: old.fp8_attn_with_mxfp4_kvcache(q, kc, ks, vc, vs), lambda: old.mxfp4_attn_with_kvcache(q, kc, ks, vc, vs),
             lambda: old.fp8_attn_varlen_with_mxfp4_kvcache(q[:, 0], kc, ks, vc, vs, cu, cu, 1, 16, block_table=table),
             lambda: old.mxfp4_attn_varlen_func(q[:, 0], kc, ks, vc, vs, cu, cu, 1, 16, block_table=table)]
    for call in calls:
        with pytest.raises(NotImplementedError, match="head_dim 64 is not supported"):
            call()


def test_signatures_resolve():
    for name in ("fa_fp4_kvcache_append_hdim", "fa_fp4_forward_kvcache_hdim", "fa_fp4_forward_kvcache_hdim_workspace_bytes", "fa_fp4_forward_varlen_hdim"):
        fields = [f for f, _c in ext._SIGNATURES[name][1]]
        assert name in ext.EXPORTED_C_SYMBOLS and "head_dim" in fields and "d" not in fields and getattr(ext._lib, name).argtypes
