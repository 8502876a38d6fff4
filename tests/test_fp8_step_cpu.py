"""CPU: the fp8 decode step (include/fa_mi355x.h: fa_fp8_kvcache_step, fa_fp8_kvcache_step_workspace_bytes) —
declared, exported, the signature rows and a family of its own; every rule of the header's list through raw ctypes with fake
pointers; the workspace's three parts; the wrapper's refusals by name; and the model (tests/fp8_step_ref.py): its append is
kvcache_full_ref.front_half's, the right model passes the sharp bar on every case of the table, and each of five wrong rules built
into it fails that bar somewhere."""
import ctypes
import os
import re

import pytest
import torch

from tests import fp8_kvcache_ref as fk
from tests import fp8_step_ref as ref
from tests.kvcache_full_ref import front_half
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_fp8_kvcache_step", "fa_fp8_kvcache_step_workspace_bytes")
OK, INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails
F16, BF16, E4M3 = 1, 2, 3

ORDER = ("q", "kc", "vc", "o", "lse", "qd", "kd", "vd", "lens", "bt", "bidx", "b", "hq", "hkv", "nq", "cap", "cb", "d", "dtype", "qdt", "cdt",
         "qb", "qt", "kb", "kt", "vb", "vt", "trs", "nb", "ps", "qdb", "kdb", "vdb", "causal", "scale", "ns", "ws", "wsb", "stream",
         "wl", "wr", "softcap", "sinks", "sh", "kn", "vn", "nnew", "knb", "knt", "vnb", "vnt", "idt", "q8", "q8b", "q8t",
         "cos", "sin", "crs", "srs", "ro", "rdim", "inter")
# contiguous, 16-bit mode: B = 3, H_q = 8, H_kv = 2, 2 query tokens (bf16: a token of 8 heads is 2048 bytes), 2 new tokens (512 bytes a
# token), caches of 1000 tokens with interleaved K and V, 4 splits, NeoX tables of rotary_dim 64 with 1000 rows, an ample workspace
BASE = dict(q=P, kc=P, vc=P, o=P, lse=P, qd=P, kd=P, vd=P, lens=P, bt=None, bidx=None, b=3, hq=8, hkv=2, nq=2, cap=1000, cb=0, d=128, dtype=2,
            qdt=BF16, cdt=E4M3, qb=8192, qt=4096, kb=512000, kt=512, vb=512000, vt=512, trs=0, nb=0, ps=0, qdb=2, kdb=2, vdb=2, causal=1,
            scale=128 ** -0.5, ns=4, ws=P, wsb=2 ** 40, stream=None, wl=-1, wr=-1, softcap=0.0, sinks=None, sh=0, kn=P, vn=P, nnew=2,
            knb=1024, knt=512, vnb=2048, vnt=1024, idt=BF16, q8=P, q8b=2048, q8t=1024, cos=P, sin=P, crs=32, srs=32, ro=1000, rdim=64,
            inter=0)
NOROT = dict(cos=None, sin=None, crs=0, srs=0, ro=0, rdim=0, inter=0)
# e4m3 mode: q, k_new, v_new hold codes (a token of 8 heads is 1024 bytes), no q8_out, no tables
F8 = dict(BASE, qdt=E4M3, idt=E4M3, qb=2048, qt=1024, knb=512, knt=256, vnb=512, vnt=256, q8=None, q8b=0, q8t=0, **NOROT)
PAGED = dict(BASE, bt=P, cap=960, trs=24, nb=64, ps=48, kb=48 * 512, vb=48 * 512 + 256, ro=960)


def _call(base=BASE, **kw):
    import flashattention_lab_cuda as ext

    a = dict(base, **kw)
    rc = ext._lib.fa_fp8_kvcache_step(*[a[n] for n in ORDER])
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext
    from common import attention_ex

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS
    assert hasattr(ext, "fp8_kvcache_step") and hasattr(attention_ex, "flash_attn_fp8_kvcache_step")
    assert ext.route_count("fp8kv_step_prep") >= 0            # (a known route: an unknown name raises)


def test_signature_rows_and_a_family_of_its_own():
    import flashattention_lab_cuda as ext

    names = PROTOTYPES["fa_fp8_kvcache_step"][2]
    parent = PROTOTYPES["fa_fp8_forward_kvcache_mod"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_fp8_kvcache_step"][1]] == names and len(names) == len(ORDER)
    assert names[:len(parent)] == parent                      # fa_fp8_forward_kvcache_mod's arguments, then the new groups
    assert names[len(parent):] == ["k_new", "v_new", "seqlen_new", "k_new_batch_stride", "k_new_token_stride", "v_new_batch_stride",
                                   "v_new_token_stride", "in_dtype", "q8_out", "q8_batch_stride", "q8_token_stride"] + \
        PROTOTYPES["fa_ex_forward_kvcache_rotary"][2][-10:-3]  # the rotary group as fa_ex_forward_kvcache_rotary spells it
    assert PROTOTYPES["fa_fp8_kvcache_step_workspace_bytes"][2] == PROTOTYPES["fa_fp8_forward_kvcache_workspace_bytes_mod"][2] + \
        ["in_dtype", "with_q8_out"]
    assert PROTOTYPES["fa_fp8_kvcache_step_workspace_bytes"][0] is ctypes.c_size_t
    _fn, own, count = ext._CALLS["fa_fp8_kvcache_step"]
    assert count == len(names) and list(own(tuple(names))) == names
    # the parents' rows and families are what they were
    assert ext._CALLS["fa_fp8_forward_kvcache_mod"][2] == len(parent) and ext._CALLS["fa_fp8_forward_kvcache"][2] == len(parent) - 5


def test_the_empty_call_is_ok_before_anything_is_looked_at():
    rc, _ = _call(q=None, kc=None, d=64, hkv=3, b=0)
    assert rc == OK


# every rule in the header's order: each row breaks one rule and, where it can, also a LATER one, which must not be the one reported.
# (No row passes validation: a call that did would launch on the fake pointers.)
REFUSALS = [
    (BASE, dict(q=None, d=64), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(kn=None, d=64), INVALID_ARGUMENT, "null tensor pointer (k_new, v_new)"),
    (BASE, dict(vn=None, lens=None), INVALID_ARGUMENT, "null tensor pointer (k_new, v_new)"),
    (BASE, dict(lens=None, d=64), INVALID_ARGUMENT, "cache_seqlens is required"),
    (BASE, dict(d=64, hkv=3), UNSUPPORTED, "head_dim 64"),
    (BASE, dict(qdt=0, idt=0, hkv=3), UNSUPPORTED, "q_dtype must be f16, bf16 or FA_DTYPE_E4M3"),
    (BASE, dict(idt=F16, hkv=3), UNSUPPORTED, "mixed dtypes"),
    (BASE, dict(idt=E4M3, hkv=3), UNSUPPORTED, "mixed dtypes"),
    (F8, dict(idt=BF16, hkv=3), UNSUPPORTED, "mixed dtypes"),
    (BASE, dict(cdt=2, hkv=3), UNSUPPORTED, "cache_dtype must be FA_DTYPE_E4M3"),
    (BASE, dict(dtype=0, hkv=3), UNSUPPORTED, "dtype (of o)"),
    (BASE, dict(hkv=3, b=70000), INVALID_ARGUMENT, "multiple of heads_kv"),
    (BASE, dict(b=70000, qt=8), INVALID_ARGUMENT, "batch must lie"),
    (BASE, dict(nq=0, qt=8), INVALID_ARGUMENT, "seqlen_q must be >= 1"),
    (BASE, dict(cap=0, qt=8), INVALID_ARGUMENT, "cache_len must be >= 1"),
    (BASE, dict(nnew=0, qt=8), INVALID_ARGUMENT, "seqlen_new=0 must lie in [1, cache_len=1000]"),
    (BASE, dict(nnew=1001, qt=8), INVALID_ARGUMENT, "seqlen_new=1001 must lie"),
    (BASE, dict(scale=0.0, qt=8), INVALID_ARGUMENT, "softmax_scale"),
    (BASE, dict(cb=5, qt=8), INVALID_ARGUMENT, "cache_batch must be 0 without"),
    (BASE, dict(q=ctypes.c_void_p(4104), qdb=1), INVALID_ARGUMENT, "16-byte aligned"),
    (BASE, dict(kn=ctypes.c_void_p(4104), qdb=1), INVALID_ARGUMENT, "k_new and v_new must be 16-byte aligned"),
    (BASE, dict(qt=2032, qdb=1), INVALID_ARGUMENT, "strides of q"),             # a bf16 token of 8 heads is 2048 bytes
    (BASE, dict(qt=1024, qdb=1), INVALID_ARGUMENT, "strides of q"),             # (1024 would do for e4m3 codes)
    (F8, dict(qt=512, qdb=1), INVALID_ARGUMENT, "strides of q"),
    (BASE, dict(kt=128, qdb=1), INVALID_ARGUMENT, "strides of k_cache"),
    (BASE, dict(knt=256, qdb=1), INVALID_ARGUMENT, "strides of k_new"),
    (BASE, dict(vnt=520, qdb=1), INVALID_ARGUMENT, "strides of v_new"),
    (BASE, dict(vnb=-16, qdb=1), INVALID_ARGUMENT, "strides of v_new"),
    (F8, dict(q8=P, qdb=1), INVALID_ARGUMENT, "q8_out goes with a 16-bit q only"),
    (BASE, dict(q8=ctypes.c_void_p(4104), qdb=1), INVALID_ARGUMENT, "q8_out must be 16-byte aligned"),
    (BASE, dict(q8t=512, qdb=1), INVALID_ARGUMENT, "strides of q8_out"),
    (BASE, dict(q8=None, qdb=1), INVALID_ARGUMENT, "must be 0 without q8_out"),
    (BASE, dict(qdb=1, ps=16), INVALID_ARGUMENT, "q_descale_batch_stride"),
    (BASE, dict(kd=None, ps=16), INVALID_ARGUMENT, "k_descale_batch_stride must be 0 without"),
    (BASE, dict(ps=16, rdim=8), INVALID_ARGUMENT, "must be 0 without block_table"),
    (PAGED, dict(bidx=P, cb=7, rdim=8), INVALID_ARGUMENT, "cannot be combined with cache_batch_idx"),
    (PAGED, dict(ps=40, rdim=8), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    (PAGED, dict(trs=19, rdim=8), INVALID_ARGUMENT, "block_table_row_stride"),
    (BASE, dict(cap=2 ** 20, kt=2048, kb=2 ** 32, rdim=8), UNSUPPORTED, "span limit"),
    (BASE, dict(nnew=900, knt=2 ** 22, knb=2 ** 40, rdim=8), UNSUPPORTED, "of k_new"),
    (BASE, dict(nq=2 ** 10, qb=2 ** 30, q8t=2 ** 22, q8b=2 ** 40, rdim=8), UNSUPPORTED, "of q8_out"),
    (BASE, dict(sin=None, ns=300), INVALID_ARGUMENT, "rotary_cos and rotary_sin must be given together"),
    (F8, dict(cos=P, sin=P, crs=32, srs=32, ro=1000, rdim=64, ns=300), INVALID_ARGUMENT, "go with 16-bit q, k_new, v_new only"),
    (BASE, dict(rdim=24, ns=300), INVALID_ARGUMENT, "rotary_dim must be a multiple of 16 in [16, 128]"),
    (BASE, dict(rdim=144, crs=72, srs=72, ns=300), INVALID_ARGUMENT, "rotary_dim must be a multiple of 16"),
    (BASE, dict(ro=999, ns=300), INVALID_ARGUMENT, "seqlen_ro=999 must be >= capacity + max(0, seqlen_q - seqlen_new) = 1000"),
    (BASE, dict(nq=5, qb=5 * 4096, q8b=5 * 1024, ns=300), INVALID_ARGUMENT, "= 1003"),
    (BASE, dict(crs=30, ns=300), INVALID_ARGUMENT, "rotary row strides (30, 32) must be >= rotary_dim / 2"),
    (BASE, dict(srs=33, ns=300), INVALID_ARGUMENT, "must be even"),
    (BASE, dict(cos=ctypes.c_void_p(4098), ns=300), INVALID_ARGUMENT, "rotary_cos and rotary_sin must be 4-byte aligned"),
    (BASE, dict(NOROT, rdim=64, ns=300), INVALID_ARGUMENT, "must be 0 without rotary_cos / rotary_sin"),
    (BASE, dict(ns=300, wl=-2), INVALID_ARGUMENT, "num_splits"),
    (BASE, dict(wl=-2, ws=None), INVALID_ARGUMENT, "window"),
    (BASE, dict(softcap=-1.0, ws=None), INVALID_ARGUMENT, "softcap"),
    (BASE, dict(sinks=P, sh=3, ws=None), INVALID_ARGUMENT, "sink_heads"),
    (BASE, dict(ws=None), WORKSPACE, "fa_fp8_kvcache_step_workspace_bytes"),
    (BASE, dict(ns=1, ws=None), WORKSPACE, "workspace"),                        # one split still needs len_eff
    (BASE, dict(wsb=1000), WORKSPACE, "too small"),
    (BASE, dict(ws=ctypes.c_void_p(4104)), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("base,kw,code,what", REFUSALS, ids=[f"{i:02d}-{r[3][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_rejected_before_any_hip_call(base, kw, code, what):
    rc, msg = _call(base, **kw)
    assert rc == code, (rc, msg)
    assert what in msg and msg.startswith("fa_fp8_kvcache_step:"), msg


def test_the_workspace_is_the_sum_of_its_three_parts():
    import flashattention_lab_cuda as ext

    ws = ext._lib.fa_fp8_kvcache_step_workspace_bytes
    parent = ext._lib.fa_fp8_forward_kvcache_workspace_bytes_mod
    al = lambda x: (x + 255) & ~255   # noqa: E731
    # (batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits, causal, window_left, window_right, with_sinks) of the parent
    for args in ((3, 8, 2, 2, 1000, 128, 4, 1, -1, -1, 0), (3, 8, 2, 2, 1000, 128, 1, 0, -1, -1, 0), (3, 8, 2, 2, 1000, 128, 1, 0, 20, -1, 1),
                 (32, 32, 8, 1, 8192, 128, 0, 1, -1, -1, 0), (70, 40, 1, 5, 300, 128, 0, 0, 17, 1, 0)):
        b, hq, _hkv, nq = args[:4]
        part = parent(*args)
        assert ws(*args, BF16, 0) == al(4 * b) + al(b * nq * hq * 128) + part          # len_eff, the q codes, the partials
        assert ws(*args, F16, 0) == ws(*args, BF16, 0)
        assert ws(*args, BF16, 1) == al(4 * b) + part                                   # the caller's q8_out
        assert ws(*args, E4M3, 0) == al(4 * b) + part                                   # q is used in place
    assert parent(3, 8, 2, 2, 1000, 128, 1, 0, -1, -1, 0) == 0 and ws(3, 8, 2, 2, 1000, 128, 1, 0, -1, -1, 0, BF16, 0) == 256 + 6144
    # arguments the call would refuse
    good = (3, 8, 2, 2, 1000, 128, 4, 1, -1, -1, 0)
    for i, bad in ((0, 0), (2, 3), (5, 64), (6, 257), (4, -1), (8, -2)):
        args = list(good)
        args[i] = bad
        assert ws(*args, BF16, 0) == 0
    assert ws(*good, 0, 0) == 0 and ws(*good, E4M3, 1) == 0


# ---- the wrapper's refusals by name

def _tensors(dtype=torch.bfloat16):
    q = torch.zeros((2, 1, 4, 128), dtype=dtype)
    k = torch.zeros((2, 1, 2, 128), dtype=dtype)
    kc = torch.zeros((2, 64, 2, 128), dtype=torch.float8_e4m3fn)
    return q, kc, kc.clone(), k, k.clone()


def test_the_wrapper_refuses_by_name():
    from common.attention_ex import flash_attn_fp8_kvcache_step as fn

    q, kc, vc, k, v = _tensors()
    t = torch.zeros(1)
    for name, val in (("cache_leftpad", t), ("cu_seqlens_q", t), ("cu_seqlens_k_new", t), ("qv", t), ("alibi_slopes", t), ("attn_bias", t),
                      ("dropout_p", 0.1)):
        with pytest.raises(NotImplementedError, match=rf"flash_attn_fp8_kvcache_step: {name} is not supported"):
            fn(q, kc, vc, k, v, cache_seqlens=3, **{name: val})
    with pytest.raises(NotImplementedError, match="k / v missing.*flash_attn_fp8_with_kvcache"):
        fn(q, kc, vc, None, None, cache_seqlens=3)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        fn(q[..., :64], kc[..., :64], vc[..., :64], k[..., :64], v[..., :64], cache_seqlens=3)
    with pytest.raises(NotImplementedError, match="block_table together with cache_batch_idx"):
        fn(q, kc, vc, k, v, cache_seqlens=3, block_table=torch.zeros((2, 4), dtype=torch.int32), cache_batch_idx=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="mixed dtypes"):
        fn(q, kc, vc, k.to(torch.float16), v, cache_seqlens=3)
    with pytest.raises(NotImplementedError, match="mixed dtypes"):
        fn(q, kc, vc, k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn), cache_seqlens=3)
    with pytest.raises(NotImplementedError, match="q of dtype torch.float32"):
        fn(q.float(), kc, vc, k.float(), v.float(), cache_seqlens=3)
    with pytest.raises(NotImplementedError, match="k_cache of dtype torch.bfloat16"):
        fn(q, kc.to(torch.bfloat16), vc, k, v, cache_seqlens=3)
    q8, _kc, _vc, k8, v8 = _tensors(torch.float8_e4m3fn)
    cos = torch.zeros((70, 16), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="rotary_cos is not supported with torch.float8_e4m3fn"):
        fn(q8, kc, vc, k8, v8, cache_seqlens=3, rotary_cos=cos, rotary_sin=cos)
    with pytest.raises(NotImplementedError, match="q8_out is not supported with torch.float8_e4m3fn"):
        fn(q8, kc, vc, k8, v8, cache_seqlens=3, q8_out=torch.zeros_like(q8))
    with pytest.raises(NotImplementedError, match="out_dtype"):
        fn(q, kc, vc, k, v, cache_seqlens=3, out_dtype=torch.float32)
    with pytest.raises(TypeError, match="unexpected keyword"):
        fn(q, kc, vc, k, v, cache_seqlens=3, no_such_argument=1)
    with pytest.raises(TypeError, match="cache_seqlens"):
        fn(q, kc, vc, k, v)
    with pytest.raises(RuntimeError, match="cache_seqlens is required"):
        fn(q, kc, vc, k, v, cache_seqlens=None)
    # valid calls in both modes get as far as the device check: there is no CPU path
    for args, kw in (((q, kc, vc, k, v), dict(rotary_cos=cos, rotary_sin=cos, q8_out=torch.zeros_like(q8))), ((q8, kc, vc, k8, v8), {})):
        with pytest.raises(RuntimeError, match="tensors must be on the GPU"):
            fn(*args, cache_seqlens=3, cache_leftpad=None, dropout_p=0.0, window_size=(20, -1), softcap=30.0, causal=True, **kw)


def test_the_older_wrappers_keep_their_refusals():
    from common.attention_ex import flash_attention_fp8_kvcache, flash_attn_fp8_with_kvcache

    q8, kc, vc, k8, _v8 = _tensors(torch.float8_e4m3fn)
    for fn in (flash_attention_fp8_kvcache, flash_attn_fp8_with_kvcache):
        for name in ("k", "v", "rotary_cos"):
            with pytest.raises(NotImplementedError, match=f"{name} is not supported by the fp8 decode call"):
                fn(q8, kc, vc, **{name: k8})


# ---- the model

_CACHE = {}


def _built(i):
    """(call, model, reference, rounded baseline) of case i, computed once and shared, never modified"""
    if i not in _CACHE:
        call = ref.build_call(i)
        m = ref.model(call)
        _CACHE[i] = (call, m, ref.reference(call), fk.rounded(ref.baseline(call), call["dtype"]))
    return _CACHE[i]


IDS = [ref.case_id(i) for i in range(len(ref.TABLE))]


def test_the_table_covers_the_issue():
    t = ref.TABLE
    assert {c["heads"] for c in t} == {(4, 2), (8, 1)} and {c["nq"] for c in t} == {1, 3} and {c["nnew"] for c in t} == {1, 3}
    assert {c["layout"] for c in t} == {"contig", "bidx", "paged", "paged_hole", "strided"}
    assert {x for c in t for x in c["lens"]} == {0, 17, 63, 64, "full", ref.CAPACITY + 5, -3}
    assert {c["dtype"] for c in t} == {"bf16", "f16"} and {c["splits"] for c in t} == {1, 3, 0}
    assert {c["rot"] for c in t} == {None, (False, 32), (False, 128), (True, 32), (True, 128)}
    assert (True, 32) in {c["rot"] for c in t if c["dtype"] == "f16"} or (True, 128) in {c["rot"] for c in t if c["dtype"] == "f16"}
    assert {(c["causal"], c["mod"]) for c in t} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c["scales"] for c in t} >= {"bbb", "hhh", "-hb"}     # (B, H_kv), (H_kv,) and None descales


@pytest.mark.parametrize("i", range(len(ref.TABLE)), ids=IDS)
def test_the_models_append_is_front_halfs(i):
    """the clamp, the slot and the codes: kvcache_full_ref.front_half on k_new as the model rotated it (in fp32) writes the same bytes,
    and nothing but the slots it lists"""
    call, (ka, va, q8, len_eff), _want, _base = _built(i)
    L = ref.clamped(call)
    k16 = call["k_new"]
    if call["rotary_cos"] is not None:
        k16 = ref.rotate32(k16, call["rotary_cos"], call["rotary_sin"], L, call["rotary_interleaved"])
    e = torch.float8_e4m3fn
    fc, _seqs = front_half(call["q"], call["k_cache"].view(e), call["v_cache"].view(e), k16, call["v_new"], call["cache_seqlens"],
                           block_table=call["block_table"], cache_batch_idx=call["cache_batch_idx"], k_descale=call["k_descale"],
                           v_descale=call["v_descale"])
    assert fc.L == L and len_eff == [x + call["nnew"] for x in L]
    assert torch.equal(fc.k_cache.view(torch.uint8), ka) and torch.equal(fc.v_cache.view(torch.uint8), va)
    assert torch.equal(ka[~fc.k_mask], call["k_cache"][~fc.k_mask]) and torch.equal(va[~fc.v_mask], call["v_cache"][~fc.v_mask])
    dropped = call["B"] * call["nnew"] - len(fc.slots)
    assert dropped == (call["nnew"] if call["layout"] in ("bidx", "paged_hole") else 0)
    assert q8.shape == call["q"].shape and q8.dtype == torch.uint8


def test_the_right_model_passes_the_bar_on_every_case():
    for i in range(len(ref.TABLE)):
        call, _m, want, base = _built(i)
        assert bool(torch.isfinite(want.o).all()) and not bool(torch.isnan(want.lse).any())
        bad, _ = fk.tile_bar(base, want, base, call["dtype"])
        assert not bad, (i, bad)


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_every_wrong_rule_fails_the_bar_somewhere(wrong):
    applies, caught = 0, []
    for i in range(len(ref.TABLE)):
        call, _m, want, base = _built(i)
        r = ref.reference(call, wrong)
        if r is None:
            continue
        applies += 1
        bad, _ratio = fk.tile_bar(fk.rounded(r, call["dtype"]), want, base, call["dtype"])
        if bad or not torch.equal(torch.isfinite(r.lse), torch.isfinite(want.lse)):
            caught.append(i)
    assert applies >= 1 and caught, (wrong, applies)
