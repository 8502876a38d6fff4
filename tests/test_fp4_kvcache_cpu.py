"""CPU: the MXFP4 KV cache calls (include/fa_mi355x.h: fa_fp4_kvcache_append, fa_fp4_forward_kvcache) — what the
Python wrappers refuse, by name, before anything touches a device; the workspace formula; mismatched code / scale tensors."""
import pytest
import torch

from common.fp4_kvcache import fp8_attn_with_mxfp4_kvcache, mxfp4_kvcache_append

B, CAP, HKV = 2, 32, 2


def cache(**shape):
    s = dict(k_cache=(B, CAP, HKV, 64), k_scale=(B, CAP, HKV, 4), v_cache=(B, CAP, HKV, 64), v_scale=(B, CAP, HKV))
    s.update(shape)
    return [torch.zeros(s[n], dtype=torch.uint8) for n in ("k_cache", "k_scale", "v_cache", "v_scale")]


def q8(d=128):
    return torch.zeros((B, 1, 8, d), dtype=torch.float8_e4m3fn)


REFUSED = [("window_size", (128, 0)), ("softcap", 30.0), ("sinks", torch.zeros(8)), ("cu_seqlens_q", torch.zeros(3, dtype=torch.int32)),
           ("max_seqlen_q", 4), ("cache_leftpad", torch.zeros(B, dtype=torch.int32)), ("qv", torch.zeros(1))]


@pytest.mark.parametrize("name,value", REFUSED, ids=[n for n, _ in REFUSED])
def test_decode_refuses_by_name(name, value):
    with pytest.raises(NotImplementedError, match=name):
        fp8_attn_with_mxfp4_kvcache(q8(), *cache(), **{name: value})
    fp4 = dict(window_size=(-1, -1), softcap=0.0, sinks=None)   # the defaults of the e4m3 call are not a refusal
    with pytest.raises(RuntimeError, match="GPU"):
        fp8_attn_with_mxfp4_kvcache(q8(), *cache(), **fp4)
    with pytest.raises(TypeError, match="unexpected keyword"):
        fp8_attn_with_mxfp4_kvcache(q8(), *cache(), no_such_argument=1)


def test_head_dims_and_dtypes_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        fp8_attn_with_mxfp4_kvcache(q8(64), *cache())
    with pytest.raises(NotImplementedError, match="head_dim 256"):
        fp8_attn_with_mxfp4_kvcache(q8(), *cache(k_cache=(B, CAP, HKV, 128), v_cache=(B, CAP, HKV, 128)))
    with pytest.raises(NotImplementedError, match="q of dtype torch.bfloat16"):
        fp8_attn_with_mxfp4_kvcache(q8().to(torch.bfloat16), *cache())
    with pytest.raises(NotImplementedError, match="k_scale of dtype torch.float32"):
        kc, ks, vc, vs = cache()
        fp8_attn_with_mxfp4_kvcache(q8(), kc, ks.float(), vc, vs)
    new = torch.zeros((B, 1, HKV, 64), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        mxfp4_kvcache_append(new, new, *cache(), cache_seqlens=0)
    with pytest.raises(NotImplementedError, match="rotary_cos"):
        mxfp4_kvcache_append(new, new, *cache(), cache_seqlens=0, rotary_cos=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="block_table together with cache_batch_idx"):
        fp8_attn_with_mxfp4_kvcache(q8(), *cache(), block_table=torch.zeros((B, 2), dtype=torch.int32), cache_batch_idx=torch.zeros(B, dtype=torch.int32))


MISMATCHED = [("k_scale", (B, CAP, HKV, 2)), ("k_scale", (B, CAP, HKV)), ("v_cache", (B, CAP + 1, HKV, 64)), ("v_scale", (B, CAP, HKV, 4)),
              ("v_scale", (B, CAP, HKV + 1))]


@pytest.mark.parametrize("name,shape", MISMATCHED, ids=[f"{n}{s}" for n, s in MISMATCHED])
def test_codes_and_scales_must_match(name, shape):
    new = torch.zeros((B, 1, HKV, 128), dtype=torch.float16)
    for call in (lambda c: fp8_attn_with_mxfp4_kvcache(q8(), *c), lambda c: mxfp4_kvcache_append(new, new, *c, cache_seqlens=0)):
        with pytest.raises(RuntimeError, match=f"{name} of shape .* does not match k_cache"):
            call(cache(**{name: shape}))


@pytest.mark.parametrize("splits", (1, 3))
def test_workspace_bytes_are_the_decode_layout(splits):
    import flashattention_lab_cuda as ext

    b, hq, hkv, nq, cap = 2, 8, 2, 9, 256
    rows = b * hq * nq * splits
    want = 0 if splits == 1 else ((rows * 128 * 4 + 255) & ~255) + ((rows * 4 + 255) & ~255)   # kv_workspace_bytes at d = 128
    assert ext._lib.fa_fp4_forward_kvcache_workspace_bytes(b, hq, hkv, nq, cap, 128, splits) == want
    assert ext._lib.fa_fp4_forward_kvcache_workspace_bytes(b, hq, hkv, nq, cap, 128, splits) == \
        ext._lib.fa_fp8_forward_kvcache_workspace_bytes(b, hq, hkv, nq, cap, 128, splits)
    assert ext._lib.fa_fp4_forward_kvcache_workspace_bytes(b, hq, hkv, nq, cap, 64, splits) == 0   # a head dim the call refuses
