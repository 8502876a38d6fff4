"""CPU: fp8 KV-cache decoding (include/fa_mi355x.h: fa_fp8_forward_kvcache, fa_fp8_forward_kvcache_workspace_bytes) —
declared, exported, the signature rows and a family of its own; every refusal in the header's order through raw ctypes with fake
pointers; the empty call; the workspace formula and the split rule at hand-computed points; the wrappers' refusals by name; and the
reference itself (tests/fp8_kvcache_ref.py): it is fp8_inputs_ref.reference and kvcache_paged_ref.reference on every sequence, the
unrounded baseline is the reference, the reference is finite on the whole table, growing keys make a wave rescale several times, and
every mutant put in the kernel's place fails the sharp bar somewhere."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import fp8_inputs_ref, kvcache_paged_ref
from tests import fp8_kvcache_cases as cases
from tests import fp8_kvcache_ref as ref
from tests.fp8_ref import e4m3_value
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_fp8_forward_kvcache", "fa_fp8_forward_kvcache_workspace_bytes")
OK, INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails
E4M3 = 3

ORDER = ("q", "kc", "vc", "o", "lse", "qd", "kd", "vd", "lens", "bt", "bidx", "b", "hq", "hkv", "nq", "cap", "cb", "d", "dtype", "qdt", "cdt",
         "qb", "qt", "kb", "kt", "vb", "vt", "trs", "nb", "ps", "qdb", "kdb", "vdb", "causal", "scale", "ns", "ws", "wsb")
# contiguous: B = 3, H_q = 8, H_kv = 2, 2 query tokens a slice of a fused projection (token stride 2048), caches of 1000 tokens with
# interleaved K and V (token stride 512), bf16 out, (B, H_kv) descales, 4 splits, an ample workspace
BASE = dict(q=P, kc=P, vc=P, o=P, lse=P, qd=P, kd=P, vd=P, lens=P, bt=None, bidx=None, b=3, hq=8, hkv=2, nq=2, cap=1000, cb=0, d=128, dtype=2,
            qdt=E4M3, cdt=E4M3, qb=4096, qt=2048, kb=512000, kt=512, vb=512000, vt=512, trs=0, nb=0, ps=0, qdb=2, kdb=2, vdb=2, causal=1,
            scale=128 ** -0.5, ns=4, ws=P, wsb=2 ** 40)
# paged: 64 pages of 48 tokens, capacity 20 pages a sequence, a table row of 24 entries
PAGED = dict(BASE, bt=P, cap=960, trs=24, nb=64, ps=48, kb=48 * 512, vb=48 * 512 + 256)
BIDX = dict(BASE, bidx=P, cb=7)


def _call(base=BASE, **kw):
    import flashattention_lab_cuda as ext

    a = dict(base, **kw)
    rc = ext._lib.fa_fp8_forward_kvcache(*[a[n] for n in ORDER], None)
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
    assert hasattr(ext, "fp8_kvcache_forward") and hasattr(attention_ex, "flash_attention_fp8_kvcache")


def test_signature_rows_and_a_family_of_its_own():
    import flashattention_lab_cuda as ext

    names = PROTOTYPES["fa_fp8_forward_kvcache"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_fp8_forward_kvcache"][1]] == names and len(names) == len(ORDER) + 1   # (all but the stream)
    assert names[:11] == ["q", "k_cache", "v_cache", "o", "lse", "q_descale", "k_descale", "v_descale", "cache_seqlens", "block_table",
                          "cache_batch_idx"]
    assert names[11:21] == ["batch", "heads_q", "heads_kv", "seqlen_q", "cache_len", "cache_batch", "d", "dtype", "q_dtype", "cache_dtype"]
    assert names[-6:] == ["causal", "softmax_scale", "num_splits", "workspace", "workspace_bytes", "stream"]
    assert PROTOTYPES["fa_fp8_forward_kvcache_workspace_bytes"][2] == ["batch", "heads_q", "heads_kv", "seqlen_q", "cache_len", "d", "num_splits"]
    assert PROTOTYPES["fa_fp8_forward_kvcache_workspace_bytes"][0] is ctypes.c_size_t
    fn, own, count = ext._CALLS["fa_fp8_forward_kvcache"]
    assert count == len(names) and list(own(tuple(names))) == names
    # the 16-bit-q call's rows and family are what they were
    assert ext._CALLS["fa_ex_forward_kvcache_fp8"][2] == ext._CALLS["fa_ex_forward_kvcache_qv"][2]


def test_the_empty_call_is_ok_before_anything_is_looked_at():
    for kw in (dict(b=0), dict(nq=0)):
        rc, _ = _call(q=None, kc=None, d=64, hkv=3, **kw)
        assert rc == OK


# every rule in the header's order: each row breaks one rule and, where it can, also a LATER one, which must not be the one reported.
# (No row passes validation: a call that did would launch on the fake pointers.)
REFUSALS = [
    (BASE, dict(q=None, d=64), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(lse=None), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(d=64, hkv=3), UNSUPPORTED, "head_dim 64"),
    (BASE, dict(qdt=2, hkv=3), UNSUPPORTED, "q_dtype must be FA_DTYPE_E4M3"),
    (BASE, dict(qdt=1), UNSUPPORTED, "fa_ex_forward_kvcache_fp8"),
    (BASE, dict(cdt=2, hkv=3), UNSUPPORTED, "cache_dtype must be FA_DTYPE_E4M3"),
    (BASE, dict(dtype=0, hkv=3), UNSUPPORTED, "dtype (of o)"),
    (BASE, dict(hkv=3, b=70000), INVALID_ARGUMENT, "multiple of heads_kv"),
    (BASE, dict(hkv=0), INVALID_ARGUMENT, "multiple of heads_kv"),
    (BASE, dict(b=70000, qt=8), INVALID_ARGUMENT, "batch must lie"),
    (BASE, dict(b=-1), INVALID_ARGUMENT, "batch must lie"),
    (BASE, dict(nq=-2), INVALID_ARGUMENT, "seqlen_q must be >= 1"),
    (BASE, dict(cap=0, qt=8), INVALID_ARGUMENT, "cache_len must be >= 1"),
    (BASE, dict(nq=2 ** 19, qt=8), INVALID_ARGUMENT, "<= 2^20"),
    (BASE, dict(scale=float("nan"), qt=8), INVALID_ARGUMENT, "softmax_scale"),
    (BASE, dict(scale=0.0), INVALID_ARGUMENT, "softmax_scale"),
    (BASE, dict(cb=5, qt=8), INVALID_ARGUMENT, "cache_batch must be 0 without"),
    (BIDX, dict(cb=0, qt=8), INVALID_ARGUMENT, "cache_batch must lie"),
    (BASE, dict(q=ctypes.c_void_p(4104), qdb=1), INVALID_ARGUMENT, "16-byte aligned"),
    (BASE, dict(lens=ctypes.c_void_p(4098), qdb=1), INVALID_ARGUMENT, "4-byte aligned"),
    (BASE, dict(qt=2056, qdb=1), INVALID_ARGUMENT, "strides of q"),
    (BASE, dict(qt=512, qdb=1), INVALID_ARGUMENT, "strides of q"),
    (BASE, dict(kt=128, qdb=1), INVALID_ARGUMENT, "strides of k_cache"),
    (BASE, dict(vb=-16, qdb=1), INVALID_ARGUMENT, "strides of v_cache"),
    (BASE, dict(kb=2 ** 45, qdb=1), INVALID_ARGUMENT, "strides of k_cache"),
    (BASE, dict(qdb=1, ps=16), INVALID_ARGUMENT, "q_descale_batch_stride"),
    (BASE, dict(kd=None, ps=16), INVALID_ARGUMENT, "k_descale_batch_stride must be 0 without"),
    (BASE, dict(vd=ctypes.c_void_p(4098), ps=16), INVALID_ARGUMENT, "v_descale must be 4-byte aligned"),
    (BASE, dict(vdb=-2, ps=16), INVALID_ARGUMENT, "v_descale_batch_stride"),
    (BASE, dict(ps=16, ns=300), INVALID_ARGUMENT, "must be 0 without block_table"),
    (BASE, dict(trs=5, ns=300), INVALID_ARGUMENT, "must be 0 without block_table"),
    (PAGED, dict(bidx=P, cb=7, ns=300), INVALID_ARGUMENT, "cannot be combined with cache_batch_idx"),
    (PAGED, dict(ps=40, ns=300), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    (PAGED, dict(ps=0, ns=300), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    (PAGED, dict(cap=1000, ns=300), INVALID_ARGUMENT, "multiple of page_block_size"),
    (PAGED, dict(nb=0, ns=300), INVALID_ARGUMENT, "num_blocks"),
    (PAGED, dict(trs=19, ns=300), INVALID_ARGUMENT, "block_table_row_stride"),
    (BASE, dict(nq=2 ** 12, qb=2 ** 40, qt=2 ** 19, ns=300), UNSUPPORTED, "span limit"),
    (BASE, dict(cap=2 ** 20, kt=2048, kb=2 ** 32, ns=300), UNSUPPORTED, "span limit"),
    (PAGED, dict(ps=65536, cap=65536 * 4, vt=2 ** 15, vb=2 ** 31, ns=300), UNSUPPORTED, "span limit"),
    (PAGED, dict(cap=48 * (2 ** 28 // 48 + 1), trs=2 ** 24, ns=300), UNSUPPORTED, "span limit"),
    (BASE, dict(ns=300, ws=None), INVALID_ARGUMENT, "num_splits"),
    (BASE, dict(ns=-1, ws=None), INVALID_ARGUMENT, "num_splits"),
    (BASE, dict(ws=None), WORKSPACE, "workspace"),
    (BASE, dict(wsb=1000), WORKSPACE, "too small"),
    (BASE, dict(ws=ctypes.c_void_p(4104)), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("base,kw,code,what", REFUSALS, ids=[f"{i:02d}-{r[3][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_rejected_before_any_hip_call(base, kw, code, what):
    rc, msg = _call(base, **kw)
    assert rc == code, (rc, msg)
    assert what in msg and msg.startswith("fa_fp8_forward_kvcache:"), msg


def test_the_workspace_formula_and_the_split_rule_at_hand_computed_points():
    import flashattention_lab_cuda as ext

    ws = ext._lib.fa_fp8_forward_kvcache_workspace_bytes
    al = lambda x: (x + 255) & ~255   # noqa: E731
    # explicit splits: rows = B H_q Nq S; O partials of 128 floats and lse partials, each rounded up to 256 bytes
    assert ws(3, 8, 2, 2, 1000, 128, 4) == al(3 * 8 * 2 * 4 * 512) + al(3 * 8 * 2 * 4 * 4) == 98304 + 768
    assert ws(3, 8, 2, 2, 1000, 128, 1) == 0
    # the rule: units = B H_kv ceil(G Nq / 32); S = min(ceil(4096 / units), ceil(cap / 128), 256), at least 1
    #   B 32, H 32 / 8, Nq 1, 8192 keys: units = 256, ceil(4096 / 256) = 16, ceil(8192 / 128) = 64 -> 16
    assert ws(32, 32, 8, 1, 8192, 128, 0) == al(32 * 32 * 16 * 512) + al(32 * 32 * 16 * 4)
    #   B 1, 65536 keys: units = 8, 512 -> capped at 256
    assert ws(1, 32, 8, 1, 65536, 128, 0) == al(32 * 256 * 512) + al(32 * 256 * 4)
    #   (40, 1) heads and 5 tokens: 200 rows = 7 tiles a head; B 3 -> units 21, ceil(4096 / 21) = 196, ceil(300 / 128) = 3 -> 3
    assert ws(3, 40, 1, 5, 300, 128, 0) == al(3 * 40 * 5 * 3 * 512) + al(3 * 40 * 5 * 3 * 4)
    #   a cache of 100 keys: one split
    assert ws(3, 8, 2, 2, 100, 128, 0) == 0
    # arguments the call would refuse
    for bad in ((0, 8, 2, 2, 1000, 128, 4), (3, 8, 3, 2, 1000, 128, 4), (3, 8, 2, 2, 1000, 64, 4), (3, 8, 2, 2, 1000, 128, 257), (3, 8, 2, 2, -1, 128, 4)):
        assert ws(*bad) == 0
    # the Python model of the rule and of the formula (tests/fp8_kvcache_ref.py) on the table
    for i, c in enumerate(cases.CASES):
        call = cases.build_call(c, i)
        assert ws(call["B"], call["hq"], call["hkv"], call["nq"], ref.capacity(call), 128, call["num_splits"]) == ref.workspace_bytes(call)


def test_split_ranges_cover_the_keys_once_in_whole_tiles():
    call = dict(B=1, hq=8, hkv=2, nq=5, causal=True, num_splits=3, block_table=None, k_cache=torch.zeros((1, 400, 2, 128), dtype=torch.uint8))
    # 20 rows, one tile; causal over 300 keys: every key visible to the last token: 5 tiles of 64 cut 1 / 2 / 2
    assert ref.split_ranges(call, 300, 0) == [(0, 64), (64, 192), (192, 300)]
    # 3 keys under the mask with 5 tokens: hi = 3, one tile; splits 0 and 1 are empty
    assert ref.split_ranges(call, 3, 0) == [(0, 0), (0, 0), (0, 3)]
    many = ref.split_ranges(dict(call, causal=False, num_splits=64), 129, 0)                 # more splits than tiles: 61 are empty
    assert sum(1 for a, b in many if a >= b) == 61 and sorted((a, b) for a, b in many if a < b) == [(0, 64), (64, 128), (128, 129)]


# ---- the wrappers' refusals by name

def _tensors():
    q = torch.zeros((2, 1, 4, 128), dtype=torch.float8_e4m3fn)
    kc = torch.zeros((2, 64, 2, 128), dtype=torch.float8_e4m3fn)
    return q, kc, kc.clone()


def test_the_wrapper_refuses_by_name():
    from common.attention_ex import flash_attention_fp8_kvcache as fn

    q, kc, vc = _tensors()
    with pytest.raises(NotImplementedError, match="q of dtype torch.bfloat16.*flash_attn_with_kvcache"):
        fn(q.to(torch.bfloat16), kc, vc)
    with pytest.raises(NotImplementedError, match="k_cache of dtype torch.float16"):
        fn(q, kc.to(torch.float16), vc)
    with pytest.raises(NotImplementedError, match="v_cache of dtype torch.float8_e5m2"):
        fn(q, kc, vc.to(torch.float32).to(torch.float8_e5m2))
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        fn(q[..., :64], kc[..., :64], vc[..., :64])
    t = torch.zeros(1)
    for name, val in (("k", t), ("v", t), ("rotary_cos", t), ("rotary_sin", t), ("window_size", (4, 0)), ("softcap", 30.0), ("alibi_slopes", t),
                      ("sinks", t), ("cache_leftpad", t), ("cu_seqlens_q", t), ("qv", t)):
        with pytest.raises(NotImplementedError, match=rf"flash_attention_fp8_kvcache: {name} is not supported"):
            fn(q, kc, vc, **{name: val})
    with pytest.raises(NotImplementedError, match="fill|filled"):
        fn(q, kc, vc, k=t)
    with pytest.raises(NotImplementedError, match="block_table together with cache_batch_idx"):
        fn(q, kc, vc, block_table=torch.zeros((2, 4), dtype=torch.int32), cache_batch_idx=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="out_dtype"):
        fn(q, kc, vc, out_dtype=torch.float32)
    with pytest.raises(TypeError, match="unexpected keyword"):
        fn(q, kc, vc, no_such_argument=1)
    # the defaults of the refused arguments pass the gate (the call then stops at the device check: there is no CPU path)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fn(q, kc, vc, k=None, window_size=(-1, -1), softcap=0.0, sinks=None)


def test_the_shim_refuses_by_name():
    import flashattention_lab_cuda as ext

    q, kc, vc = _tensors()
    with pytest.raises(NotImplementedError, match="flash_attn_with_kvcache"):
        ext.fp8_kvcache_forward(q.to(torch.float16), kc, vc)
    with pytest.raises(NotImplementedError, match="k_cache of dtype"):
        ext.fp8_kvcache_forward(q, kc.to(torch.bfloat16), vc)
    with pytest.raises(NotImplementedError, match="block_table of dtype torch.int64"):
        ext.fp8_kvcache_forward(q, kc, vc, block_table=torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="multiple of H_kv"):
        ext.fp8_kvcache_forward(q[:, :, :3], kc, vc)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ext.fp8_kvcache_forward(q, kc, vc)


# ---- the reference itself

TABLE = [(i, c) for i, c in enumerate(cases.CASES)]
_CACHE = {}


def _built(i):
    """(call, reference, rounded baseline) of case i, computed once and shared, never modified"""
    if i not in _CACHE:
        call = cases.build_call(cases.CASES[i], i)
        tr = []
        _CACHE[i] = (call, ref.reference(call), ref.rounded(ref.baseline(call, trace=tr), call["dtype"]), tr)
    return _CACHE[i]


def _seq_call(call, b, k8, v8):
    """sequence b alone as the dict tests/fp8_inputs_ref.py takes (B = 1)"""
    ds = {n: (None if call[n] is None else call[n] if call[n].dim() == 1 else call[n][b:b + 1]) for n in ("q_descale", "k_descale", "v_descale")}
    return dict(B=1, hq=call["hq"], hkv=call["hkv"], nq=call["nq"], nk=k8.shape[0], causal=call["causal"], dtype=call["dtype"],
                scale=call["scale"], q8=call["q8"][b].transpose(0, 1)[None].contiguous(), k8=k8.transpose(0, 1)[None].contiguous(),
                v8=v8.transpose(0, 1)[None].contiguous(), **ds)


@pytest.mark.parametrize("i", range(len(cases.CASES)), ids=[cases.case_id(c, i) for i, c in TABLE])
def test_reference_is_the_padded_fp8_reference_and_the_kvcache_reference_per_sequence(i):
    call, want, _base, _tr = _built(i)
    o, lse = ref.unpack(want, call)
    assert bool(torch.isfinite(o).all()) and not bool(torch.isnan(lse).any())          # finite on every case of the table
    seqs = ref.sequences(call)
    qd, kd, vd = fp8_inputs_ref.descales(call)
    g = call["hq"] // call["hkv"]
    qf = e4m3_value(call["q8"]).double() * qd.double().repeat_interleave(g, 1)[:, None, :, None]
    ks = [e4m3_value(k).double() * kd[b].double()[None, :, None] for b, (k, _v) in enumerate(seqs)]
    vs = [e4m3_value(v).double() * vd[b].double()[None, :, None] for b, (_k, v) in enumerate(seqs)]
    o2, lse2 = kvcache_paged_ref.reference(qf, ks, vs, call["causal"], (-1, -1), call["scale"])
    fin = torch.isfinite(lse)
    assert torch.equal(fin, torch.isfinite(lse2))
    assert (o - o2).abs().max().item() <= 1e-12 * max(1.0, o.abs().max().item())
    assert (lse[fin] - lse2[fin]).abs().max().item() <= 1e-12 * max(1.0, lse[fin].abs().max().item()) if fin.any() else True
    for b, (k8, v8) in enumerate(seqs):
        if k8.shape[0] == 0:
            assert bool((o[b] == 0).all()) and bool((lse[b] == -math.inf).all())
            continue
        r = fp8_inputs_ref.reference(_seq_call(call, b, k8, v8))                           # (H_q, Nq, .)
        ob, lb = o[b].transpose(0, 1), lse[b]
        fb = torch.isfinite(lb)
        assert torch.equal(fb, torch.isfinite(r.lse))
        assert (ob - r.o).abs().max().item() <= 1e-12 * max(1.0, ob.abs().max().item())
        if fb.any():
            assert (lb[fb] - r.lse[fb]).abs().max().item() <= 1e-12 * max(1.0, lb[fb].abs().max().item())


@pytest.mark.parametrize("i", range(len(cases.CASES)), ids=[cases.case_id(c, i) for i, c in TABLE])
def test_unrounded_baseline_is_the_reference(i):
    call, want, _base, _tr = _built(i)
    b64 = ref.baseline(call, torch.float64, rounding=False)
    fin = torch.isfinite(want.lse)
    assert torch.equal(fin, torch.isfinite(b64.lse))
    assert (b64.o - want.o).abs().max().item() <= 1e-10 * max(1.0, want.o.abs().max().item())
    if fin.any():
        assert (b64.lse[fin] - want.lse[fin]).abs().max().item() <= 1e-10 * max(1.0, want.lse[fin].abs().max().item())


def test_the_table_keeps_every_axis_value_and_rows_without_a_key():
    assert len(cases.CASES) <= 40
    for a, vals in cases.AXES.items():
        assert {c[a] for c in cases.CASES} == set(vals), a
    # causal with Nq > len: some live sequence has rows without a key
    hit = 0
    for i, c in TABLE:
        if c["mask"] == "causal" and c["nq"] > 1 and 1 in cases.LENS[c["lens"]]:
            call, want, _b, _t = _built(i)
            _o, lse = ref.unpack(want, call)
            b = cases.LENS[c["lens"]].index(1)
            if call["cache_batch_idx"] is None or 0 <= int(call["cache_batch_idx"][b]) < call["k_cache"].shape[0]:
                assert bool((lse[b] == -math.inf).any()) and bool(torch.isfinite(lse[b]).any())
                hit += 1
    assert hit >= 1


def test_growing_keys_make_a_wave_rescale_several_times():
    """the baseline's trace: in the growing cases some wave moves its running maximum on three tiles or more of one split"""
    most = 0
    for i, c in TABLE:
        if c["values"] != "growing":
            continue
        moves = {}
        for b, hk, rt, s, _t, gw in _built(i)[3]:
            moves[(b, hk, rt, s)] = moves.get((b, hk, rt, s), 0) + int(gw)
        most = max(most, max(moves.values(), default=0))
    assert most >= 3, most


@pytest.mark.parametrize("name", ref.MUTANTS)
def test_every_mutant_fails_the_sharp_bar_somewhere(name):
    applies, caught = 0, []
    for i, c in TABLE:
        call, want, base, _tr = _built(i)
        m = ref.mutant(call, name)
        if m is None:
            continue
        applies += 1
        bad, _ratio = ref.tile_bar(ref.rounded(m, call["dtype"]), want, base, call["dtype"])
        # the -inf pattern is part of what the GPU test holds
        if bad or not torch.equal(torch.isfinite(m.lse), torch.isfinite(want.lse)):
            caught.append(i)
    assert applies >= 1 and caught, (name, applies)


def test_the_baseline_itself_passes_the_bar_it_sets():
    for i, _c in TABLE[:6]:
        call, want, base, _tr = _built(i)
        bad, _ = ref.tile_bar(base, want, base, call["dtype"])
        assert not bad
