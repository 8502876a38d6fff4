"""CPU: a sliding window, a softcap and sinks over the MXFP4 KV cache (include/fa_mi355x.h: fa_fp4_forward_kvcache_mod,
fa_fp4_forward_varlen_mod) — what the two new wrappers take and still refuse, by name, before anything touches a
device; the C-ABI checks that fail before any launch; the workspace formula."""
import pytest
import torch

import flashattention_lab_cuda as ext
from common.fp4_kvcache import mxfp4_attn_varlen_func, mxfp4_attn_with_kvcache

B, CAP, PS, HQ, HKV = 2, 32, 16, 8, 2
FEATURES = dict(window_size=(17, 0), softcap=30.0, sinks=torch.zeros(HQ))


def decode(**kw):
    cache = [torch.zeros(s, dtype=torch.uint8) for s in ((B, CAP, HKV, 64), (B, CAP, HKV, 4), (B, CAP, HKV, 64), (B, CAP, HKV))]
    return mxfp4_attn_with_kvcache(torch.zeros((B, 1, HQ, 128), dtype=torch.float8_e4m3fn), *cache, **kw)


def prefill(**kw):
    pool = [torch.zeros(s, dtype=torch.uint8) for s in ((4, PS, HKV, 64), (4, PS, HKV, 4), (4, PS, HKV, 64), (4, PS, HKV))]
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    kw.setdefault("block_table", torch.zeros((B, 2), dtype=torch.int32))
    return mxfp4_attn_varlen_func(torch.zeros((8, HQ, 128), dtype=torch.float8_e4m3fn), *pool, cu, cu, 5, 5, **kw)


REFUSED = [(decode, "cu_seqlens_q", torch.zeros(3, dtype=torch.int32)), (decode, "cache_leftpad", torch.zeros(B, dtype=torch.int32)),
           (decode, "qv", torch.zeros(1)), (decode, "rotary_cos", torch.zeros(1)), (prefill, "cache_batch_idx", torch.zeros(B, dtype=torch.int32)),
           (prefill, "cache_seqlens", torch.zeros(B, dtype=torch.int32)), (prefill, "alibi_slopes", torch.zeros(HQ)), (prefill, "attn_bias", torch.zeros(1))]


@pytest.mark.parametrize("call,name,value", REFUSED, ids=[f"{c.__name__}-{n}" for c, n, _ in REFUSED])
def test_the_new_wrappers_take_the_three_and_refuse_the_rest(call, name, value):
    with pytest.raises(RuntimeError, match="GPU"):                # accepted: the call gets as far as asking for a device
        call(**FEATURES)
    with pytest.raises(NotImplementedError, match=name):
        call(**FEATURES, **{name: value})
    with pytest.raises(TypeError, match="unexpected keyword"):
        call(no_such_argument=1)


def abi_args(name):
    fields = [f for f, _ in ext._SIGNATURES[name][1]]
    args = dict.fromkeys(fields, 0)
    args.update({f: 4096 for f in fields[:13]}, batch=B, heads_q=HQ, heads_kv=HKV, cache_len=2 * PS, d=128, dtype=ext._DTYPE_CODE[torch.bfloat16],
                q_token_stride=HQ * 128, k_batch_stride=PS * HKV * 64, k_token_stride=HKV * 64, k_scale_batch_stride=PS * HKV * 4,
                k_scale_token_stride=HKV * 4, v_batch_stride=PS * HKV * 64, v_token_stride=HKV * 64, v_scale_batch_stride=PS * HKV,
                v_scale_token_stride=HKV, block_table_row_stride=2, num_blocks=4, page_block_size=PS, softmax_scale=0.1,
                q_descale=0, k_descale=0, v_descale=0, window_left=-1, window_right=-1)
    if "seqlen_q" in args:                                        # the decode call: a paged cache, one split, no workspace
        args.update(seqlen_q=1, cache_batch_idx=0, num_splits=1)
    else:
        args.update(total_q=8, max_seqlen_q=5)
    return fields, args


ABI = [(dict(softcap=-1.0), "FA_ERR_INVALID_ARGUMENT", "softcap must be a finite number >= 0"),
       (dict(window_left=-2), "FA_ERR_INVALID_ARGUMENT", "each bound must be >= 0, or -1 for unbounded"),
       (dict(sinks=4096, sink_heads=3), "FA_ERR_INVALID_ARGUMENT", "sink_heads=3 must be 1 or heads_q=8"),
       (dict(sinks=0, sink_heads=HQ), "FA_ERR_INVALID_ARGUMENT", "sink_heads must be 0 without sinks"),
       (dict(sinks=4098, sink_heads=1), "FA_ERR_INVALID_ARGUMENT", "sinks must be 4-byte aligned"),
       (dict(d=64), "FA_ERR_UNSUPPORTED", "head_dim 64 is not supported"),       # default trailing arguments: the parent's error
       (dict(batch=0), "FA_OK", None)]                                           # ... and the parent's FA_OK


@pytest.mark.parametrize("name", ("fa_fp4_forward_kvcache_mod", "fa_fp4_forward_varlen_mod"))
@pytest.mark.parametrize("change,code,text", ABI, ids=["-".join(c[0]) for c in ABI])
def test_c_abi_checks_fail_before_any_launch(name, change, code, text):
    fields, args = abi_args(name)
    args.update(change)
    rc = getattr(ext._lib, name)(*[args[f] for f in fields])
    assert rc == dict(FA_OK=0, FA_ERR_INVALID_ARGUMENT=-1, FA_ERR_UNSUPPORTED=-2)[code]     # (include/fa_mi355x.h)
    if text:
        assert name + ": " in ext._lib.fa_last_error().decode() and text in ext._lib.fa_last_error().decode()


@pytest.mark.parametrize("splits,window,sinks", ((1, (-1, -1), 0), (1, (-1, -1), 1), (0, (128, -1), 0), (0, (-1, -1), 0), (3, (17, 1), 1)))
def test_workspace_bytes_are_the_e4m3_featured_call_s(splits, window, sinks):
    args = (64, 32, 8, 1, 32768, 128, splits, 1, *window, sinks)
    want = ext._lib.fa_fp8_forward_kvcache_workspace_bytes_mod(*args)
    assert ext._lib.fa_fp4_forward_kvcache_workspace_bytes_mod(*args) == want
    assert splits == 0 or (want > 0) == (splits > 1 or bool(sinks))   # (sinks raise one split to two: the sink joins in the combine)
    assert ext._lib.fa_fp4_forward_kvcache_workspace_bytes_mod(64, 32, 8, 1, 32768, 64, splits, 1, *window, sinks) == 0   # a head dim the call refuses
