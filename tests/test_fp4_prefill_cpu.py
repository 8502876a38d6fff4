"""CPU: chunked prefill over the MXFP4 KV cache (include/fa_mi355x.h: fa_fp4_forward_varlen) — what the Python wrapper
refuses, by name, before anything touches a device, and the C-ABI checks that fail before any launch."""
import pytest
import torch

import flashattention_lab_cuda as ext
from common.fp4_kvcache import fp8_attn_varlen_with_mxfp4_kvcache

NB, PS, HKV = 4, 16, 2


def call(d=128, **kw):
    pool = [torch.zeros(s, dtype=torch.uint8) for s in ((NB, PS, HKV, 64), (NB, PS, HKV, 4), (NB, PS, HKV, 64), (NB, PS, HKV))]
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    kw.setdefault("block_table", torch.zeros((2, 2), dtype=torch.int32))
    return fp8_attn_varlen_with_mxfp4_kvcache(torch.zeros((8, 8, d), dtype=torch.float8_e4m3fn), *pool, cu, cu, 5, 5, **kw)


REFUSED = [("window_size", (128, 0)), ("softcap", 30.0), ("sinks", torch.zeros(8)), ("cache_leftpad", torch.zeros(2, dtype=torch.int32)),
           ("cache_batch_idx", torch.zeros(2, dtype=torch.int32)), ("qv", torch.zeros(1)), ("rotary_cos", torch.zeros(1)),
           ("alibi_slopes", torch.zeros(8)), ("attn_bias", torch.zeros(1))]


@pytest.mark.parametrize("name,value", REFUSED, ids=[n for n, _ in REFUSED])
def test_prefill_refuses_by_name(name, value):
    with pytest.raises(NotImplementedError, match=name):
        call(**{name: value})


def test_what_else_the_wrappers_say():
    with pytest.raises(TypeError, match="unexpected keyword"):
        call(no_such_argument=1)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        call(d=64)
    with pytest.raises(RuntimeError, match="block_table is required"):
        call(block_table=None)
    with pytest.raises(RuntimeError, match="GPU"):                # (the defaults of the e4m3 call are not a refusal)
        call(window_size=(-1, -1), softcap=0.0, sinks=None)


ABI = [(dict(d=64), "FA_ERR_UNSUPPORTED", "head_dim 64 is not supported"),
       (dict(k_token_stride=HKV * 64 + 8), "FA_ERR_INVALID_ARGUMENT", "the strides of k_cache"),
       (dict(block_table=0), "FA_ERR_INVALID_ARGUMENT", "block_table is required"),
       (dict(total_q=0), "FA_OK", None)]


@pytest.mark.parametrize("change,code,text", ABI, ids=[next(iter(c[0])) for c in ABI])
def test_c_abi_checks_fail_before_any_launch(change, code, text):
    fields = [f for f, _ in ext._SIGNATURES["fa_fp4_forward_varlen"][1]]
    args = dict.fromkeys(fields, 0)
    args.update({f: 4096 for f in fields[:13]}, batch=2, heads_q=8, heads_kv=HKV, total_q=8, max_seqlen_q=5, cache_len=2 * PS, d=128,
                dtype=ext._DTYPE_CODE[torch.bfloat16], q_token_stride=8 * 128, k_batch_stride=PS * HKV * 64, k_token_stride=HKV * 64,
                k_scale_batch_stride=PS * HKV * 4, k_scale_token_stride=HKV * 4, v_batch_stride=PS * HKV * 64, v_token_stride=HKV * 64,
                v_scale_batch_stride=PS * HKV, v_scale_token_stride=HKV, block_table_row_stride=2, num_blocks=NB, page_block_size=PS,
                softmax_scale=0.1)
    args.update(q_descale=0, k_descale=0, v_descale=0, **change)
    rc = ext._lib.fa_fp4_forward_varlen(*[args[f] for f in fields])
    assert rc == dict(FA_OK=0, FA_ERR_INVALID_ARGUMENT=-1, FA_ERR_UNSUPPORTED=-2)[code]     # (include/fa_mi355x.h)
    if text:
        assert text in ext._lib.fa_last_error().decode()
