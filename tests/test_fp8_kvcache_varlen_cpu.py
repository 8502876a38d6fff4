"""CPU: packed queries and new keys on the fp8 decode call and the fp8 decode step, and the step at head dims 64 / 256
(include/fa_mi355x.h: fa_fp8_forward_kvcache_varlen, fa_fp8_kvcache_step_varlen and their size functions; common/fp8_attention.py:
fp8_attn_with_kvcache_varlen, fp8_attn_kvcache_step): the declarations, the host's refusals in their documented
order, the workspace sizes against the stated expressions, the wrappers' refusals, and the proofs behind
tests/test_fp8_kvcache_varlen_gpu.py: the d- and offset-parameterised model is the padded step's model on uniform lengths, its
clamp is the 16-bit call's, and the clamp lets nothing out of a tensor."""
import ctypes
import itertools

import pytest
import torch

from tests import fp8_step_ref as sr
from tests import fp8_step_varlen_ref as vr
from tests import kvcache_varlen_ref as kv
from tests.test_abi_signatures_cpu import PROTOTYPES

E4 = torch.float8_e4m3fn
OK, INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails
ODD = ctypes.c_void_p(4104)   # 8-byte aligned only
ODD2 = ctypes.c_void_p(4098)  # 2-byte aligned only
E4M3, BF16 = 3, 2
DECODE_FN, STEP_FN = "fa_fp8_forward_kvcache_varlen", "fa_fp8_kvcache_step_varlen"
DECODE_WS, STEP_WS = DECODE_FN + "_workspace_bytes", STEP_FN + "_workspace_bytes"
TAIL = dict(window_left=-1, window_right=-1, softcap=0.0, sinks=None, sink_heads=0)


def align(x):
    return (x + 255) & ~255


def partials(s, total_q, hq, d):
    """S * total_q * H_q * (d + 1) floats, each of the two parts rounded up to 256 bytes; 0 for one split"""
    return align(s * total_q * hq * d * 4) + align(s * total_q * hq * 4) if s > 1 and total_q > 0 else 0


# packed decode: B = 3, H_q = 8, H_kv = 2, ten packed query tokens, at most four a sequence, caches of 1000 tokens, four splits
DECODE = dict(q=P, k_cache=P, v_cache=P, o=P, lse=P, q_descale=P, k_descale=P, v_descale=P, cache_seqlens=P, block_table=None,
              cache_batch_idx=None, batch=3, heads_q=8, heads_kv=2, seqlen_q=0, cache_len=1000, cache_batch=0, head_dim=64, dtype=2,
              q_dtype=E4M3, cache_dtype=E4M3, q_batch_stride=0, q_token_stride=512, k_batch_stride=256000, k_token_stride=256,
              v_batch_stride=256000, v_token_stride=256, block_table_row_stride=0, num_blocks=0, page_block_size=0,
              q_descale_batch_stride=2, k_descale_batch_stride=2, v_descale_batch_stride=2, causal=1, softmax_scale=0.125, num_splits=4,
              workspace=P, workspace_bytes=2 ** 40, stream=None, **TAIL, cu_seqlens_q=P, total_q=10, max_seqlen_q=4)
# the packed step in bf16: six packed new keys, the q codes in the workspace, no rotary
STEP = dict(DECODE, q_dtype=BF16, q_token_stride=1024, k_new=P, v_new=P, seqlen_new=0, k_new_batch_stride=0, k_new_token_stride=256,
            v_new_batch_stride=0, v_new_token_stride=256, in_dtype=BF16, q8_out=None, q8_batch_stride=0, q8_token_stride=0,
            rotary_cos=None, rotary_sin=None, rotary_cos_row_stride=0, rotary_sin_row_stride=0, seqlen_ro=0, rotary_dim=0,
            rotary_interleaved=0, cu_seqlens_k_new=P, total_k_new=6)
ROTARY = dict(rotary_cos=P, rotary_sin=P, rotary_cos_row_stride=16, rotary_sin_row_stride=16, seqlen_ro=1004, rotary_dim=32)
PADDED_Q = dict(cu_seqlens_q=None, total_q=0, max_seqlen_q=0, seqlen_q=2, q_batch_stride=2048)   # on STEP: q (B, 2, H_q, 64) bf16
STEP_NEED = align(3 * 4) + align(10 * 8 * 64) + partials(4, 10, 8, 64)


def invoke(name, base, **kw):
    """(return code, message) of the C function on base's arguments by the header's parameter names"""
    import flashattention_lab_cuda as ext

    a = dict(base, **kw)
    names = PROTOTYPES[name][2]
    assert set(names) == set(a), set(names) ^ set(a)
    rc = getattr(ext._lib, name)(*[a[n] for n in names])
    return rc, ext._lib.fa_last_error().decode()


def test_the_entry_points_are_declared_exported_and_extend_their_parents_lists():
    import flashattention_lab_cuda as ext
    from common import attention_ex, fp8_attention

    for name in (DECODE_FN, STEP_FN, DECODE_WS, STEP_WS):
        assert name in PROTOTYPES and name in ext.EXPORTED_C_SYMBOLS and hasattr(ext._lib, name)
    renamed = lambda names: ["head_dim" if n == "d" else n for n in names]   # noqa: E731
    assert PROTOTYPES[DECODE_FN][2] == PROTOTYPES["fa_fp8_forward_kvcache_hdim"][2] + ["cu_seqlens_q", "total_q", "max_seqlen_q"]
    assert PROTOTYPES[STEP_FN][2] == renamed(PROTOTYPES["fa_fp8_kvcache_step"][2]) + \
        ["cu_seqlens_q", "total_q", "max_seqlen_q", "cu_seqlens_k_new", "total_k_new"]
    assert PROTOTYPES[STEP_WS][2] == renamed(PROTOTYPES["fa_fp8_kvcache_step_workspace_bytes"][2]) + ["total_q", "max_seqlen_q"]
    assert PROTOTYPES[DECODE_WS][2] == ["batch", "heads_q", "heads_kv", "total_q", "max_seqlen_q", "cache_len", "head_dim", "num_splits",
                                        "causal", "window_left", "window_right", "with_sinks"]
    for name in (DECODE_FN, STEP_FN):       # a family of one each: called with exactly its own arguments
        _fn, own, count = ext._CALLS[name]
        assert count == len(PROTOTYPES[name][2]) and list(own(tuple(PROTOTYPES[name][2]))) == PROTOTYPES[name][2]
    for fn in ("fp8_attn_with_kvcache_varlen", "fp8_attn_kvcache_step"):
        assert getattr(attention_ex, fn) is getattr(fp8_attention, fn)
    for route in ("fp8kv_split_varlen", "fp8kv_step_prep_varlen"):
        assert ext.route_count(route) >= 0


# Every row breaks one rule and, where it can, a LATER one as well, which must not be the one reported; no row passes validation (a
# call that did would launch on the fake pointers).  The order: the parents' rules (1) .. (9) and the window / softcap / sinks rules,
# the packed group (P1) .. (P8), the workspace.
REFUSALS = [
    (DECODE_FN, DECODE, dict(q=None, head_dim=96), INVALID_ARGUMENT, "null tensor pointer"),
    (DECODE_FN, DECODE, dict(head_dim=96, heads_kv=3), UNSUPPORTED, "head_dim 96 is not supported (64, 128 or 256)"),
    (DECODE_FN, DECODE, dict(head_dim=192, heads_kv=3), UNSUPPORTED, "head_dim 192 is not supported (64, 128 or 256)"),
    (DECODE_FN, DECODE, dict(q_dtype=2, heads_kv=3), UNSUPPORTED, "q_dtype must be FA_DTYPE_E4M3"),
    (DECODE_FN, DECODE, dict(heads_kv=3, batch=70000), INVALID_ARGUMENT, "multiple of heads_kv"),
    (DECODE_FN, DECODE, dict(batch=70000, q_token_stride=8), INVALID_ARGUMENT, "batch must lie"),
    (DECODE_FN, DECODE, dict(q_token_stride=256, num_splits=300), INVALID_ARGUMENT, "the token stride >= heads * 64 = 512"),
    (DECODE_FN, DECODE, dict(head_dim=256, num_splits=300), INVALID_ARGUMENT, "the token stride >= heads * 256 = 2048"),
    (DECODE_FN, DECODE, dict(num_splits=300, max_seqlen_q=11), INVALID_ARGUMENT, "num_splits"),
    (DECODE_FN, DECODE, dict(window_right=-5, max_seqlen_q=11), INVALID_ARGUMENT, "window (-1, -5)"),
    (DECODE_FN, DECODE, dict(cu_seqlens_q=None, seqlen_q=2, q_batch_stride=1024, workspace=None), INVALID_ARGUMENT,
     "total_q and max_seqlen_q must be 0 without cu_seqlens_q"),
    (DECODE_FN, DECODE, dict(max_seqlen_q=11, total_q=10, cu_seqlens_q=ODD2), INVALID_ARGUMENT, "max_seqlen_q=11 must lie in [0, total_q=10]"),
    (DECODE_FN, DECODE, dict(max_seqlen_q=-1, cu_seqlens_q=ODD2), INVALID_ARGUMENT, "max_seqlen_q=-1 must lie in [0, total_q=10]"),
    (DECODE_FN, DECODE, dict(total_q=2 ** 31, cu_seqlens_q=ODD2), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    (DECODE_FN, DECODE, dict(total_q=2 ** 20, max_seqlen_q=2 ** 20, q_token_stride=4096), UNSUPPORTED, "span limit: max_seqlen_q * token stride of q"),
    (DECODE_FN, DECODE, dict(total_q=2 ** 19, max_seqlen_q=2 ** 19, cu_seqlens_q=ODD2), INVALID_ARGUMENT,
     "(heads_q / heads_kv) * max_seqlen_q = 4 * 524288 must be <= 2^20"),
    (DECODE_FN, DECODE, dict(cu_seqlens_q=ODD2, workspace=None), INVALID_ARGUMENT, "cu_seqlens_q and cu_seqlens_k_new must be 4-byte aligned"),
    (DECODE_FN, DECODE, dict(workspace=None), WORKSPACE, DECODE_WS),
    (DECODE_FN, DECODE, dict(workspace_bytes=1000), WORKSPACE, f"need {partials(4, 10, 8, 64)}"),
    (DECODE_FN, DECODE, dict(workspace=ODD), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
    (STEP_FN, STEP, dict(k_new=None, head_dim=96), INVALID_ARGUMENT, "null tensor pointer (k_new, v_new)"),
    (STEP_FN, STEP, dict(cache_seqlens=None, head_dim=96), INVALID_ARGUMENT, "cache_seqlens is required"),
    (STEP_FN, STEP, dict(head_dim=96, in_dtype=1), UNSUPPORTED, "head_dim 96 is not supported (64, 128 or 256)"),
    (STEP_FN, STEP, dict(head_dim=192, in_dtype=1), UNSUPPORTED, "head_dim 192 is not supported (64, 128 or 256)"),
    (STEP_FN, STEP, dict(in_dtype=1, heads_kv=3), UNSUPPORTED, "mixed dtypes"),
    (STEP_FN, STEP, dict(heads_kv=3, q_token_stride=512), INVALID_ARGUMENT, "multiple of heads_kv"),
    (STEP_FN, STEP, dict(cu_seqlens_k_new=None, total_k_new=0, seqlen_new=0, q_token_stride=512), INVALID_ARGUMENT, "seqlen_new=0 must lie in [1, cache_len=1000]"),
    (STEP_FN, STEP, dict(q_token_stride=512, num_splits=300), INVALID_ARGUMENT, "the token stride >= heads * 64 = 1024"),
    (STEP_FN, STEP, dict(k_new_token_stride=128, num_splits=300), INVALID_ARGUMENT, "strides of k_new"),
    (STEP_FN, STEP, dict(head_dim=256, q_token_stride=4096, num_splits=300), INVALID_ARGUMENT, "strides of k_cache"),
    (STEP_FN, STEP, dict(q8_out=P, q8_token_stride=256, num_splits=300), INVALID_ARGUMENT, "the token stride >= heads_q * 64 = 512"),
    (STEP_FN, STEP, dict(ROTARY, rotary_dim=128, num_splits=300), INVALID_ARGUMENT, "rotary_dim must be a multiple of 16 in [16, 64] (got 128)"),
    (STEP_FN, STEP, dict(num_splits=300, max_seqlen_q=11), INVALID_ARGUMENT, "num_splits"),
    (STEP_FN, STEP, dict(softcap=-1.0, max_seqlen_q=11), INVALID_ARGUMENT, "softcap must be a finite number"),
    (STEP_FN, STEP, dict(PADDED_Q, total_q=10, workspace=None), INVALID_ARGUMENT, "total_q and max_seqlen_q must be 0 without cu_seqlens_q"),
    (STEP_FN, STEP, dict(cu_seqlens_k_new=None, seqlen_new=1, k_new_batch_stride=256, v_new_batch_stride=256, max_seqlen_q=11), INVALID_ARGUMENT,
     "total_k_new must be 0 without cu_seqlens_k_new"),
    (STEP_FN, STEP, dict(PADDED_Q, workspace=None), INVALID_ARGUMENT, "cu_seqlens_k_new needs cu_seqlens_q"),
    (STEP_FN, STEP, dict(max_seqlen_q=11, total_k_new=-1), INVALID_ARGUMENT, "max_seqlen_q=11 must lie in [0, total_q=10]"),
    (STEP_FN, STEP, dict(total_k_new=2 ** 31, cu_seqlens_k_new=ODD2), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    (STEP_FN, STEP, dict(total_k_new=-1, cu_seqlens_k_new=ODD2), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    (STEP_FN, STEP, dict(total_q=2 ** 20, max_seqlen_q=2 ** 20, q8_out=P, q8_token_stride=4096), UNSUPPORTED,
     "span limit: max_seqlen_q * token stride of q8_out"),
    (STEP_FN, STEP, dict(total_q=2 ** 19, max_seqlen_q=2 ** 19, cu_seqlens_q=ODD2), INVALID_ARGUMENT, "must be <= 2^20"),
    (STEP_FN, STEP, dict(ROTARY, seqlen_ro=1003, cu_seqlens_k_new=ODD2), INVALID_ARGUMENT, "seqlen_ro=1003 must be >= capacity + max_seqlen_q = 1004"),
    (STEP_FN, STEP, dict(cu_seqlens_k_new=ODD2, workspace=None), INVALID_ARGUMENT, "must be 4-byte aligned"),
    (STEP_FN, STEP, dict(workspace=None), WORKSPACE, STEP_WS),
    (STEP_FN, STEP, dict(workspace_bytes=1000), WORKSPACE, f"need {STEP_NEED}"),
    (STEP_FN, STEP, dict(total_q=0, max_seqlen_q=0, workspace_bytes=255), WORKSPACE, "need 256"),     # no query token: len_b alone
    (STEP_FN, STEP, dict(workspace=ODD), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("name,base,kw,code,what", REFUSALS,
                         ids=[f"{i:02d}-{'step' if r[0] == STEP_FN else 'decode'}-{r[4][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_in_the_documented_order_before_any_hip_call(name, base, kw, code, what):
    rc, msg = invoke(name, base, **kw)
    assert rc == code, (rc, msg)
    assert what in msg and msg.startswith(name + ":"), msg


def test_the_empty_calls_are_ok_before_anything_is_looked_at():
    for kw in (dict(batch=0), dict(total_q=0, max_seqlen_q=0), dict(max_seqlen_q=0), dict(cu_seqlens_q=None, total_q=0, max_seqlen_q=0)):
        rc, msg = invoke(DECODE_FN, DECODE, q=None, head_dim=96, **kw)
        assert rc == OK, msg
    rc, msg = invoke(STEP_FN, STEP, q=None, head_dim=96, batch=0)
    assert rc == OK, msg


def test_with_a_null_packed_group_the_parents_rules_and_texts_hold():
    padded = dict(DECODE, cu_seqlens_q=None, total_q=0, max_seqlen_q=0, seqlen_q=2, q_batch_stride=1024)
    rc, msg = invoke(DECODE_FN, padded, q_batch_stride=8)
    assert rc == INVALID_ARGUMENT and "the strides of q (batch 8, token 512) must be multiples of 16 bytes" in msg
    rc, msg = invoke(DECODE_FN, padded, seqlen_q=2 ** 20 + 1)
    assert rc == INVALID_ARGUMENT and "(heads_q / heads_kv) * seqlen_q" in msg
    rc, msg = invoke(DECODE_FN, padded, workspace_bytes=1000)
    hdim = dict((k, v) for k, v in padded.items() if k not in ("cu_seqlens_q", "total_q", "max_seqlen_q"))
    rc2, msg2 = invoke("fa_fp8_forward_kvcache_hdim", hdim, workspace_bytes=1000)
    assert rc == rc2 == WORKSPACE and msg.split("need ")[1].split(":")[0] == msg2.split("need ")[1].split(":")[0]
    # with cu_seqlens_q the two are not looked at
    rc, msg = invoke(DECODE_FN, DECODE, seqlen_q=-5, q_batch_stride=8, workspace=None)
    assert rc == WORKSPACE, msg
    step = dict(STEP, **PADDED_Q, cu_seqlens_k_new=None, total_k_new=0, seqlen_new=1, k_new_batch_stride=256, v_new_batch_stride=256)
    rc, msg = invoke(STEP_FN, step, **dict(ROTARY, seqlen_ro=1000))
    assert rc == INVALID_ARGUMENT and "seqlen_ro=1000 must be >= capacity + max(0, seqlen_q - seqlen_new) = 1001" in msg
    rc, msg = invoke(STEP_FN, step, workspace_bytes=1000)
    assert rc == WORKSPACE and f"need {align(3 * 4) + align(3 * 2 * 8 * 64) + partials(4, 3 * 2, 8, 64)}" in msg
    # with cu_seqlens_k_new seqlen_new and the batch strides of the new keys are not looked at
    rc, msg = invoke(STEP_FN, STEP, seqlen_new=-3, k_new_batch_stride=8, v_new_batch_stride=-16, workspace=None)
    assert rc == WORKSPACE, msg


def splits_rule(batch, hq, hkv, max_q, cache_len, num_splits, causal, wl, wr, sinks):
    """the host split rule: num_splits = 0 takes ceil(4096 / units) over ceil(max_seqlen_q * G / 32) row tiles, at most one split a
    128 keys of the keys a window can show, in [1, 256]; sinks raise 1 to 2"""
    if num_splits > 0:
        s = num_splits
    else:
        length = cache_len if wl < 0 else min(cache_len, wl + (0 if causal or wr < 0 else wr) + max_q)
        units = batch * hkv * ((max_q * (hq // hkv) + 31) // 32)
        s = 1 if units <= 0 or length <= 0 else max(1, min((4096 + units - 1) // units, (length + 127) // 128, 256))
    return max(s, 2) if sinks else s


def test_the_workspace_sizes():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for d in vr.HEAD_DIMS:
        for (b, hq, hkv, tq, mq, cap), (ns, causal, wl, wr, snk) in itertools.product(
                ((5, 8, 2, 29, 20, 384), (3, 8, 2, 10, 4, 1000), (64, 8, 8, 191, 128, 8192), (1, 4, 4, 1, 1, 100000)),
                ((4, 1, -1, -1, 0), (1, 1, -1, -1, 0), (1, 0, 128, -1, 1), (7, 0, -1, -1, 1), (0, 1, -1, -1, 0), (0, 0, 128, 5, 0), (0, 1, 20, -1, 1))):
            s = splits_rule(b, hq, hkv, mq, cap, ns, causal, wl, wr, snk)
            want = partials(s, tq, hq, d)
            assert lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(b, hq, hkv, tq, mq, cap, d, ns, causal, wl, wr, snk) == want
            for code, q8o in ((BF16, 0), (1, 1), (E4M3, 0)):
                prep = align(b * 4) + (align(tq * hq * d) if code != E4M3 and not q8o else 0)
                assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(b, hq, hkv, 0, cap, d, ns, causal, wl, wr, snk, code, q8o, tq, mq) == prep + want
        # the padded step at this width: the _hdim partials behind len_b and the codes
        for code, q8o in ((BF16, 0), (BF16, 1), (E4M3, 0)):
            prep = align(3 * 4) + (align(3 * 2 * 8 * d) if code != E4M3 and not q8o else 0)
            assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 2, 1000, d, 4, 1, -1, -1, 0, code, q8o, 0, 0) == \
                prep + lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(3, 8, 2, 2, 1000, d, 4, 1, -1, -1, 0) > prep
    assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 2, 1000, 128, 0, 1, 64, -1, 1, BF16, 0, 0, 0) == \
        lib.fa_fp8_kvcache_step_workspace_bytes(3, 8, 2, 2, 1000, 128, 0, 1, 64, -1, 1, BF16, 0) > 0
    # one split, no query token: nothing for the decode call, len_b alone for the step
    assert lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(3, 8, 2, 10, 4, 1000, 64, 1, 1, -1, -1, 0) == 0
    assert lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(3, 8, 2, 0, 0, 1000, 64, 4, 1, -1, -1, 0) == 0
    assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 0, 1000, 64, 4, 1, -1, -1, 0, E4M3, 0, 0, 0) == 256
    # refused arguments: 0
    for bad in (dict(d=96), dict(d=192), dict(hkv=3), dict(mq=11), dict(mq=-1), dict(tq=2 ** 31), dict(ns=300), dict(wl=-2), dict(b=0),
                dict(cap=0), dict(mq=2 ** 19, tq=2 ** 19)):
        a = dict(dict(b=3, hq=8, hkv=2, tq=10, mq=4, cap=1000, d=64, ns=4, wl=-1), **bad)
        assert lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(a["b"], a["hq"], a["hkv"], a["tq"], a["mq"], a["cap"], a["d"], a["ns"], 1,
                                                                 a["wl"], -1, 0) == 0, bad
        assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(a["b"], a["hq"], a["hkv"], 0, a["cap"], a["d"], a["ns"], 1, a["wl"], -1, 0, BF16,
                                                              0, a["tq"], a["mq"]) == 0, bad
    assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 0, 1000, 64, 4, 1, -1, -1, 0, E4M3, 1, 10, 4) == 0     # q8_out with e4m3
    assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 0, 1000, 64, 4, 1, -1, -1, 0, 0, 0, 10, 4) == 0        # float32
    assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 2, 1000, 64, 4, 1, -1, -1, 0, BF16, 0, 10, 4) == 0     # both forms
    assert lib.fa_fp8_kvcache_step_varlen_workspace_bytes(3, 8, 2, 2, 1000, 96, 4, 1, -1, -1, 0, BF16, 0, 0, 0) == 0
    # the older size functions still answer 0 at 64 and 256
    for d in (64, 256):
        assert lib.fa_fp8_kvcache_step_workspace_bytes(3, 8, 2, 2, 1000, d, 4, 1, -1, -1, 0, BF16, 0) == 0


def _f8(*shape):
    return torch.zeros(shape, dtype=torch.uint8).view(E4)


def test_the_new_wrappers_refuse_by_name():
    from common.fp8_attention import fp8_attn_kvcache_step, fp8_attn_with_kvcache_varlen

    cu = torch.tensor([0, 1, 4], dtype=torch.int32)
    decode = lambda d, dk=None, **kw: fp8_attn_with_kvcache_varlen(   # noqa: E731
        _f8(4, 2, d), _f8(2, 16, 2, dk or d), _f8(2, 16, 2, dk or d), **dict(dict(cu_seqlens_q=cu, max_seqlen_q=3), **kw))
    step = lambda d, dk=None, dt=torch.bfloat16, **kw: fp8_attn_kvcache_step(   # noqa: E731
        torch.zeros((4, 2, d), dtype=dt), _f8(2, 16, 2, dk or d), _f8(2, 16, 2, dk or d), torch.zeros((4, 2, d), dtype=dt),
        torch.zeros((4, 2, d), dtype=dt), **dict(dict(cache_seqlens=3, cu_seqlens_q=cu, max_seqlen_q=3, cu_seqlens_k_new=cu), **kw))
    with pytest.raises(TypeError):
        fp8_attn_with_kvcache_varlen(_f8(4, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64))          # cu_seqlens_q, max_seqlen_q: required
    for fn in (decode, step):
        with pytest.raises(RuntimeError, match="mixed head dims: q has"):
            fn(64, 128)
        for d in (96, 192, 32, 512):
            with pytest.raises(NotImplementedError, match=rf"head_dim {d} is not supported \(64, 128 or 256\)"):
                fn(d)
        for name, val in (("cache_leftpad", torch.zeros(2, dtype=torch.int32)), ("qv", _f8(4, 2, 64)), ("alibi_slopes", torch.zeros(2)),
                          ("attn_bias", torch.zeros(1)), ("mask", torch.zeros(1)), ("dropout_p", 0.1)):
            with pytest.raises(NotImplementedError, match=f"{name} is not supported"):
                fn(64, **{name: val})
        with pytest.raises(TypeError, match="unexpected keyword argument"):
            fn(64, no_such_argument=1)
        with pytest.raises(NotImplementedError, match="block_table together with cache_batch_idx"):
            fn(64, block_table=torch.zeros((2, 1), dtype=torch.int32), cache_batch_idx=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(NotImplementedError, match="out_dtype torch.float32 is not supported"):
            fn(64, out_dtype=torch.float32)
        with pytest.raises(RuntimeError, match="window"):
            fn(256, window_size=(-2, 0))
        with pytest.raises(NotImplementedError, match="cu_seqlens_q of dtype torch.int64 is not supported"):
            fn(64, cu_seqlens_q=cu.long())
        with pytest.raises(RuntimeError, match=r"max_seqlen_q \(an int"):
            fn(64, max_seqlen_q=None)
        with pytest.raises(RuntimeError, match=r"max_seqlen_q \(an int"):
            fn(64, max_seqlen_q=torch.tensor(3))
        with pytest.raises(RuntimeError, match=r"max_seqlen_q = 5 must lie in \[0, total_q = 4\]"):
            fn(64, max_seqlen_q=5)
        for d in vr.HEAD_DIMS:              # everything passes: the call gets as far as the device check
            with pytest.raises(RuntimeError, match="must be on the GPU"):
                fn(d)
    with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: q is"):
        fp8_attn_with_kvcache_varlen(torch.zeros((4, 2, 64), dtype=torch.bfloat16), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), cu_seqlens_q=cu,
                                     max_seqlen_q=3)
    with pytest.raises(RuntimeError, match="cu_seqlens_q is required"):
        decode(64, cu_seqlens_q=None)
    with pytest.raises(RuntimeError, match="q must be packed"):
        fp8_attn_with_kvcache_varlen(_f8(1, 4, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), cu_seqlens_q=cu, max_seqlen_q=3)
    with pytest.raises(RuntimeError, match="cu_seqlens_k_new needs cu_seqlens_q"):
        step(64, cu_seqlens_q=None, max_seqlen_q=None)
    with pytest.raises(RuntimeError, match="max_seqlen_q goes with cu_seqlens_q"):
        step(64, cu_seqlens_q=None, cu_seqlens_k_new=None)
    with pytest.raises(NotImplementedError, match="mixed dtypes"):
        fp8_attn_kvcache_step(torch.zeros((4, 2, 64), dtype=torch.bfloat16), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64),
                              torch.zeros((4, 2, 64), dtype=torch.float16), torch.zeros((4, 2, 64), dtype=torch.bfloat16), cache_seqlens=3,
                              cu_seqlens_q=cu, max_seqlen_q=3, cu_seqlens_k_new=cu)
    with pytest.raises(NotImplementedError, match="rotary_cos is not supported with torch.float8_e4m3fn"):
        fp8_attn_kvcache_step(_f8(4, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), _f8(4, 2, 64), _f8(4, 2, 64), cache_seqlens=3, cu_seqlens_q=cu,
                              max_seqlen_q=3, cu_seqlens_k_new=cu, rotary_cos=torch.zeros((32, 8)), rotary_sin=torch.zeros((32, 8)))
    with pytest.raises(NotImplementedError, match="k / v missing"):
        fp8_attn_kvcache_step(_f8(4, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), None, None, cache_seqlens=3)
    with pytest.raises(RuntimeError, match=r"rotary_dim = 2 \* rotary_cos.shape\[1\] must be a multiple of 16 in \[16, 64\], got 128"):
        step(64, rotary_cos=torch.zeros((32, 64), dtype=torch.bfloat16), rotary_sin=torch.zeros((32, 64), dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match=r"k and v must be packed \(total_k_new, H_kv, d\)"):
        fp8_attn_kvcache_step(torch.zeros((4, 2, 64), dtype=torch.bfloat16), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64),
                              torch.zeros((2, 2, 2, 64), dtype=torch.bfloat16), torch.zeros((2, 2, 2, 64), dtype=torch.bfloat16), cache_seqlens=3,
                              cu_seqlens_q=cu, max_seqlen_q=3, cu_seqlens_k_new=cu)
    # the padded step at 64 / 256 and padded new keys with packed queries pass as far as the device check
    for d in vr.HEAD_DIMS:
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            fp8_attn_kvcache_step(torch.zeros((2, 1, 2, d), dtype=torch.float16), _f8(2, 16, 2, d), _f8(2, 16, 2, d),
                                  torch.zeros((2, 1, 2, d), dtype=torch.float16), torch.zeros((2, 1, 2, d), dtype=torch.float16), cache_seqlens=3)
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            fp8_attn_kvcache_step(torch.zeros((4, 2, d), dtype=torch.float16), _f8(2, 16, 2, d), _f8(2, 16, 2, d),
                                  torch.zeros((2, 1, 2, d), dtype=torch.float16), torch.zeros((2, 1, 2, d), dtype=torch.float16), cache_seqlens=3,
                                  cu_seqlens_q=cu, max_seqlen_q=3)


def test_the_shim_keywords():
    import flashattention_lab_cuda as ext

    cu = torch.tensor([0, 1, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="max_seqlen_q goes with cu_seqlens_q"):
        ext.fp8_kvcache_forward(_f8(2, 2, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), max_seqlen_q=3)
    with pytest.raises(RuntimeError, match=r"max_seqlen_q \(an int"):
        ext.fp8_kvcache_forward(_f8(4, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), cu_seqlens_q=cu)
    with pytest.raises(NotImplementedError, match=r"head_dim 96 is not supported \(64, 128 or 256\)"):   # the hdim rules
        ext.fp8_kvcache_forward(_f8(4, 2, 96), _f8(2, 16, 2, 96), _f8(2, 16, 2, 96), cu_seqlens_q=cu, max_seqlen_q=3)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ext.fp8_kvcache_forward(_f8(4, 2, 256), _f8(2, 16, 2, 256), _f8(2, 16, 2, 256), cu_seqlens_q=cu, max_seqlen_q=3)
    with pytest.raises(TypeError):
        ext.fp8_kvcache_forward(_f8(4, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), None, None, None, None, None, None, None, False, 0,
                                torch.bfloat16, cu, 3)                                               # keyword-only
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16)   # noqa: E731
    with pytest.raises(RuntimeError, match="cu_seqlens_k_new needs cu_seqlens_q"):
        ext.fp8_kvcache_step(bf(2, 1, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), bf(3, 2, 64), bf(3, 2, 64), 3, cu_seqlens_k_new=cu)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ext.fp8_kvcache_step(bf(2, 1, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), bf(2, 1, 2, 64), bf(2, 1, 2, 64), 3, hdim=True)
    with pytest.raises(NotImplementedError, match=r"head_dim 64 is not supported \(128 only\)"):       # without the keywords: what it was
        ext.fp8_kvcache_step(bf(2, 1, 2, 64), _f8(2, 16, 2, 64), _f8(2, 16, 2, 64), bf(2, 1, 2, 64), bf(2, 1, 2, 64), 3)


def test_the_older_wrappers_still_refuse_the_three_names():
    from common.attention_ex import flash_attention_fp8_kvcache, flash_attn_fp8_kvcache_step, flash_attn_fp8_with_kvcache
    from common.fp8_attention import fp8_attn_with_kvcache

    cu = torch.tensor([0, 1], dtype=torch.int32)
    for fn in (flash_attention_fp8_kvcache, flash_attn_fp8_with_kvcache, fp8_attn_with_kvcache):
        for name, val in (("cu_seqlens_q", cu), ("max_seqlen_q", 1), ("cu_seqlens_k_new", cu)):
            with pytest.raises(NotImplementedError, match=f"{name} is not supported by the fp8 decode call"):
                fn(_f8(1, 1, 2, 128), _f8(1, 16, 2, 128), _f8(1, 16, 2, 128), **{name: val})
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16)   # noqa: E731
    for name, val in (("cu_seqlens_q", cu), ("max_seqlen_q", 1), ("cu_seqlens_k_new", cu)):
        with pytest.raises(NotImplementedError, match=f"{name} is not supported by the fp8 decode step"):
            flash_attn_fp8_kvcache_step(bf(1, 1, 2, 128), _f8(1, 16, 2, 128), _f8(1, 16, 2, 128), bf(1, 1, 2, 128), bf(1, 1, 2, 128),
                                        cache_seqlens=3, **{name: val})


# ---- the model

@pytest.mark.parametrize("i", range(len(sr.TABLE)), ids=[sr.case_id(i) for i in range(len(sr.TABLE))])
def test_at_128_with_uniform_lengths_the_model_is_the_padded_steps_bit_for_bit(i):
    call = sr.build_call(i)
    ka, va, q8, len_eff = sr.model(call)
    mk, mv, mq8, mlen, owned = vr.model(vr.from_padded(call))
    assert torch.equal(mk, ka) and torch.equal(mv, va) and mlen == len_eff and bool(owned.all())
    assert torch.equal(mq8, q8.reshape(mq8.shape))


def test_the_clamp_is_the_16_bit_calls_and_lets_nothing_out():
    values = list(range(-3, 10)) + [-2 ** 31, 2 ** 31 - 1]
    for total in range(0, 7):
        for bound in range(0, 5):
            for c0, c1 in itertools.product(values, values):
                start, n = vr.cu_range([c0, c1], 0, total, bound)
                assert (start, n) == kv.cu_range([c0, c1], 0, total, bound)
                assert 0 <= start <= total and 0 <= n <= bound and start + n <= total
                if 0 <= c0 <= c1 <= total and c1 - c0 <= bound:
                    assert (start, n) == (c0, c1 - c0)             # well-formed offsets are taken as they are
    for name, cu in vr.BAD_OFFSETS.items():
        assert not kv.well_formed(cu, 29, 20), name
        for b in range(5):
            start, n = vr.cu_range(cu, b, 29, 20)
            assert 0 <= start and n >= 0 and start + n <= 29 and n <= 20


def test_the_problem_of_the_gpu_tests():
    p = vr.PROBLEM
    assert sum(p["nq"]) == 29 and max(p["nq"]) == 20 and sum(p["nnew"]) == 11 and p["capacity"] % 16 == 0 and p["capacity"] % 48 == 0
    assert (20 * 4 + 31) // 32 == 3 and (20 * 1 + 31) // 32 == 1                      # G = 4: nq = 20 spans three 32-row tiles
    call = vr.problem(64, 4, "ps48", rot=(False, 32))
    ka, va, q8, len_eff, owned = vr.model(call)
    assert len_eff == [301, 17, 5, 66, 132] and bool(owned.all()) and q8.shape == (29, 8, 64)
    changed = (ka != call["k_cache"]).any(-1).any(-1)
    assert int(changed.sum()) <= 11                                                    # no byte outside the appended slots
    padded = vr.problem(64, 4, "bidx", packed_kn=False)
    _ka, _va, _q8, len_eff, _o = vr.model(padded)
    assert len_eff == [305, 22, 5, 69, 134]                                           # every sequence appends max nnew = 5
