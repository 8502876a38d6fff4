"""CPU: a sliding window, a softcap and attention sinks on the three fp8 calls (include/fa_mi355x.h: fa_fp8_forward_mod,
fa_fp8_forward_varlen_mod, fa_fp8_forward_kvcache_mod, fa_fp8_forward_kvcache_workspace_bytes_mod) — the proofs
behind tests/test_fp8_mod_gpu.py and tests/test_fp8_kvcache_mod_gpu.py (the written-out fp64 form and the baseline without rounding
are the project's fp64 reference; every mutant fails the sharp bar on some table case), the new wrappers' refusals and acceptances,
the old wrappers' refusals, the host's validation texts and the decode split rule with a window."""
import ctypes
import functools
import itertools

import pytest
import torch

from tests import fp8_kvcache_mod_ref as km
from tests import fp8_kvcache_ref as fk
from tests import fp8_mod_ref as fm
from tests.fp8_ref import tiled_sharp_bar

E4M3 = torch.float8_e4m3fn
PADDED = [(i, cap, snk) for i in range(len(fm.TABLE)) for cap in (False, True) for snk in (False, True)]
PADDED_IDS = [f"{i}-{'x'.join(map(str, fm.TABLE[i]['n']))}{'-cap' if cap else ''}{'-sinks' if snk else ''}" for i, cap, snk in PADDED]
DECODE_IDS = [km.case_id(i) for i in range(len(km.TABLE))]


@functools.lru_cache(maxsize=None)
def padded_case(i, cap, snk):
    """(call in bf16, fp64 reference, float32 baseline before o's rounding to a dtype) — shared with the GPU tests, never changed"""
    call = fm.build_call(i, cap, snk)
    return call, fm.reference(call), fm.baseline(dict(call, dtype=None))


def padded_base(i, cap, snk, dtype):
    """the baseline of the case with o rounded to dtype (the rounding is the baseline's last step)"""
    call, ref, raw = padded_case(i, cap, snk)
    return dict(call, dtype=dtype), ref, raw._replace(o=raw.o.to(dtype).float())


@functools.lru_cache(maxsize=None)
def decode_case(i):
    call = km.build_call(i)
    return call, km.reference(call), km.baseline(call)


def _close(a, b, tol=1e-10):
    fin = torch.isfinite(b.lse)
    assert torch.equal(torch.isfinite(a.lse), fin) and torch.equal(a.lse[~fin], b.lse[~fin])
    assert float((a.o - b.o).abs().max()) <= tol * max(1.0, float(b.o.abs().max()))
    assert float((a.lse[fin] - b.lse[fin]).abs().max()) <= tol * max(1.0, float(b.lse[fin].abs().max()))


@pytest.mark.parametrize("i,cap,snk", PADDED, ids=PADDED_IDS)
def test_padded_written_out_form_and_unrounded_baseline_are_the_reference(i, cap, snk):
    call, ref, _raw = padded_case(i, cap, snk)
    _close(fm.evaluate(call), ref)
    _close(fm.baseline(call, torch.float64, rounding=False), ref)
    if snk:      # a row without a visible key: o = 0 and lse = the sink; -inf without one
        dead = ~fm.band(call).any(-1)
        want = call["sinks"].double().repeat(call["B"])[:, None].expand_as(ref.lse)
        assert torch.equal(ref.lse[:, dead], want[:, dead]) and bool((ref.o[:, dead] == 0).all())


@pytest.mark.parametrize("i", range(len(km.TABLE)), ids=DECODE_IDS)
def test_decode_written_out_form_and_unrounded_baseline_are_the_reference(i):
    call, ref, _base = decode_case(i)
    _close(km.evaluate(call), ref)
    _close(km.baseline(call, torch.float64, rounding=False), ref)


def test_the_baselines_pass_their_own_bar_with_finite_sinks_at_1e4():
    for i, cap, snk in PADDED:
        call, ref, base = padded_base(i, cap, snk, torch.bfloat16)
        assert bool(torch.isfinite(base.o).all()) and not bool(torch.isnan(base.lse).any())
        bad, _r = tiled_sharp_bar(base, ref, base, torch.bfloat16)
        assert not bad, bad
    for i in range(len(km.TABLE)):
        call, ref, base = decode_case(i)
        assert bool(torch.isfinite(base.o).all()) and not bool(torch.isnan(base.lse).any())
        bad, _r = fk.tile_bar(base, ref, base, call["dtype"])
        assert not bad, bad


@pytest.mark.parametrize("name", fm.MUTANTS)
def test_every_mutant_fails_the_sharp_bar_on_some_case(name):
    caught = []
    for key, (i, cap, snk) in zip(PADDED_IDS, PADDED):
        call, ref, base = padded_base(i, cap, snk, torch.bfloat16)
        mut = fm.evaluate(call, name)
        if mut is not None and tiled_sharp_bar(mut, ref, base, torch.bfloat16)[0]:
            caught.append("padded " + key)
    for i in range(len(km.TABLE)):
        call, ref, base = decode_case(i)
        mut = km.evaluate(call, name)
        if mut is not None and fk.tile_bar(mut, ref, base, call["dtype"])[0]:
            caught.append("decode " + DECODE_IDS[i])
    print(name, caught)
    assert caught, f"{name} passes the sharp bar on every case it applies to"


def test_no_case_is_skipped_by_every_mutant():
    """A table case is a shape with its window; it runs bare, capped, with sinks and with both.  The bare run of (300, 300) with
    the right bound alone is out of every listed bug's reach (square, no left bound, no causal flag), so the padded table is
    counted per case over its four runs; every decode case is within reach as it stands."""
    for i in range(len(fm.TABLE)):
        assert any(fm.applies(padded_case(i, cap, snk)[0], m) for m in fm.MUTANTS for cap in (False, True) for snk in (False, True)), i
    for i in range(len(km.TABLE)):
        assert any(km.applies(decode_case(i)[0], m) for m in fm.MUTANTS), i


def test_the_varlen_case_is_the_padded_call_per_sequence():
    v = fm.varlen_case(True, (20, -1), True, True)
    assert v["cu_q"].tolist() == [0, 5, 6, 43, 83, 83] and v["cu_k"].tolist() == [0, 0, 1, 38, 338, 467]
    o, lse = fm.varlen_expected(v, fm.reference)
    assert torch.equal(lse[:, :5], v["sinks"].double()[:, None].expand(4, 5)) and bool((o[:5] == 0).all())   # no key: the sink
    c = v["calls"][2]
    assert torch.equal(v["q8"][6:43], c["q8"][0].transpose(0, 1)) and torch.equal(v["k8"][1:38], c["k8"][0].transpose(0, 1))


# ---- the Python wrappers

def _q8(*shape):
    return torch.zeros(shape, dtype=E4M3)


def test_the_new_wrappers_refuse_by_name_and_take_the_three_arguments():
    from common.attention_ex import flash_attn_fp8_func, flash_attn_fp8_varlen_func, flash_attn_fp8_with_kvcache

    cu = torch.tensor([0, 16, 32], dtype=torch.int32)
    calls = {
        "flash_attn_fp8_func": (flash_attn_fp8_func, (_q8(2, 2, 16, 128),) * 3,
                                dict(alibi_slopes=torch.ones(2), attn_bias=torch.zeros(16, 16), mask=torch.ones(16, 16),
                                     block_sparse_mask=torch.ones(1, 1), dropout_p=0.1)),
        "flash_attn_fp8_varlen_func": (flash_attn_fp8_varlen_func, (_q8(32, 2, 128),) * 3 + (cu, cu, 16, 16),
                                       dict(alibi_slopes=torch.ones(2), attn_bias=torch.zeros(16, 16), mask=torch.ones(16, 16),
                                            dropout_p=0.1, seqused_k=cu[:2], cache_leftpad=cu[:2], rotary_cos=torch.zeros(4, 4))),
        "flash_attn_fp8_with_kvcache": (flash_attn_fp8_with_kvcache, (_q8(2, 1, 2, 128), _q8(2, 64, 2, 128), _q8(2, 64, 2, 128)),
                                        dict(k=_q8(2, 1, 2, 128), v=_q8(2, 1, 2, 128), rotary_cos=torch.zeros(4, 4), alibi_slopes=torch.ones(2),
                                             cache_leftpad=cu[:2], cu_seqlens_q=cu, qv=_q8(2, 1, 2, 128), attn_bias=torch.zeros(1, 64),
                                             dropout_p=0.1)),
    }
    mod = dict(window_size=(8, 0), softcap=30.0, sinks=torch.zeros(2))
    for who, (fn, args, refused) in calls.items():
        for name, val in refused.items():
            with pytest.raises(NotImplementedError, match=f"{who}: {name} is not supported"):
                fn(*args, **{name: val})
        with pytest.raises(TypeError, match="unexpected keyword argument 'nonsense'"):
            fn(*args, nonsense=1)
        with pytest.raises(NotImplementedError, match="torch.float8_e4m3fn expected"):
            fn(args[0].to(torch.bfloat16), *args[1:], **mod)
        with pytest.raises(NotImplementedError, match="head_dim 64 is not supported"):
            fn(*(t[..., :64] for t in args[:3]), *args[3:], **mod)
        with pytest.raises(NotImplementedError, match="out_dtype torch.float32 is not supported"):
            fn(*args, out_dtype=torch.float32, **mod)
        # the three arguments are taken: the call gets as far as the shim, which has no CPU path
        for kw in (mod, dict(window_size=(8, 0)), dict(softcap=30.0), dict(sinks=torch.zeros(2)), {}):
            with pytest.raises(RuntimeError, match="tensors must be on the GPU"):
                fn(*args, **kw)
        with pytest.raises(RuntimeError, match=f"{who}: window \\(-2, 0\\): each bound must be >= 0, or -1 for unbounded"):
            fn(*args, window_size=(-2, 0))
        with pytest.raises(RuntimeError, match=f"{who}: window_size must be a pair"):
            fn(*args, window_size=5)
        for bad in (-1.0, float("nan"), float("inf"), "x"):
            with pytest.raises(RuntimeError, match=f"{who}: softcap must be a finite number >= 0"):
                fn(*args, softcap=bad)
        with pytest.raises(RuntimeError, match=f"{who}: sinks must be a float32 tensor"):
            fn(*args, sinks=torch.zeros(2, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="block_table together with cache_batch_idx"):
        flash_attn_fp8_with_kvcache(*calls["flash_attn_fp8_with_kvcache"][1], block_table=torch.zeros((2, 4), dtype=torch.int32),
                                    cache_batch_idx=cu[:2], **mod)


def test_the_old_wrappers_still_refuse_and_name_the_new_function():
    from common.attention_ex import flash_attention_fp8, flash_attention_fp8_kvcache, flash_attention_fp8_varlen

    cu = torch.tensor([0, 16, 32], dtype=torch.int32)
    old = (("flash_attention_fp8", flash_attention_fp8, (_q8(2, 2, 16, 128),) * 3, "call", "flash_attn_fp8_func"),
           ("flash_attention_fp8_varlen", flash_attention_fp8_varlen, (_q8(32, 2, 128),) * 3 + (cu, cu, 16, 16), "call",
            "flash_attn_fp8_varlen_func"),
           ("flash_attention_fp8_kvcache", flash_attention_fp8_kvcache, (_q8(2, 1, 2, 128), _q8(2, 64, 2, 128), _q8(2, 64, 2, 128)),
            "decode call", "flash_attn_fp8_with_kvcache"))
    for who, fn, args, what, new in old:
        for name, val in (("window_size", (8, 0)), ("softcap", 30.0), ("sinks", torch.zeros(2))):
            with pytest.raises(NotImplementedError) as e:
                fn(*args, **{name: val})
            assert str(e.value) == f"{who}: {name} is not supported by the fp8 {what} ({new} takes it)"
        with pytest.raises(NotImplementedError) as e:
            fn(*args, alibi_slopes=torch.ones(2))
        assert str(e.value) == f"{who}: alibi_slopes is not supported by the fp8 {what}"
    with pytest.raises(NotImplementedError) as e:
        flash_attention_fp8_kvcache(*old[2][2], k=_q8(2, 1, 2, 128))
    assert str(e.value).endswith("decode call (the cache is filled by flash_attn_with_kvcache's append, or by the caller)")


def test_the_shim_checks_the_three_arguments_after_the_device():
    import flashattention_lab_cuda as ext

    q = _q8(2, 2, 16, 128)
    assert ext._fp8_mod("who", q, 2, (-1, -1), 0.0, None) == ("", (), None)
    mod, tail, keep = ext._fp8_mod("who", q, 2, (8, -1), 0.0, None)
    assert (mod, tail, keep) == ("_mod", (8, -1, 0.0, 0, 0), None)
    s = torch.zeros(2)
    mod, tail, keep = ext._fp8_mod("who", q, 2, (-1, -1), 0.0, s)
    assert mod == "_mod" and tail == (-1, -1, 0.0, s.data_ptr(), 2) and keep is s
    with pytest.raises(RuntimeError, match=r"who: sinks must be \(H_q,\) = \(2,\), one per query head, got \(3,\)"):
        ext._fp8_mod("who", q, 2, (-1, -1), 0.0, torch.zeros(3))
    with pytest.raises(RuntimeError, match="who: window \\(-1, -3\\)"):
        ext._fp8_mod("who", q, 2, (-1, -3), 0.0, None)
    with pytest.raises(RuntimeError, match="who: softcap must be a finite number >= 0"):
        ext._fp8_mod("who", q, 2, (-1, -1), float("inf"), None)
    with pytest.raises(RuntimeError, match="tensors must be on the GPU"):
        ext.fp8_forward(q, q, q, False, None, window=(4, 0), softcap=5.0, sinks=s)


# ---- the C layer: every row is rejected before any HIP call (there is no GPU here, and the pointers are fake)

P = ctypes.c_void_p(4096)
INVALID_ARGUMENT = -1
PAD = (P, P, P, P, P, P, P, P, 2, 4, 2, 300, 500, 128, 2, 4 * 300 * 128, 300 * 128, 128, 2 * 500 * 128, 500 * 128, 128, 2 * 500 * 128,
       500 * 128, 128, 4 * 300 * 128, 300 * 128, 128, 2, 2, 2, 1, 128 ** -0.5, P, 2 ** 40, None)
VAR = (P, P, P, P, P, P, P, P, P, P, None, 2, 4, 2, 600, 1000, 300, 500, 128, 2, 4 * 128, 128, 2 * 128, 128, 2 * 128, 128, 0, 0, 0, 0, 0,
       2, 2, 2, 1, 128 ** -0.5, P, 2 ** 40, None)
KV = (P, P, P, P, P, P, P, P, P, None, None, 2, 4, 2, 1, 1024, 0, 128, 2, 3, 3, 512, 512, 1024 * 256, 256, 1024 * 256, 256, 0, 0, 0, 2, 2,
      2, 1, 128 ** -0.5, 1, None, 0, None)
BAD = [
    ((-2, 0, 0.0, None, 0), "window (-2, 0): each bound must be >= 0, or -1 for unbounded"),
    ((0, -5, 0.0, None, 0), "window (0, -5): each bound must be >= 0, or -1 for unbounded"),
    ((-1, -1, -1.0, None, 0), "softcap must be a finite number >= 0 (got -1)"),
    ((-1, -1, float("nan"), None, 0), "softcap must be a finite number >= 0 (got nan)"),
    ((-1, -1, float("inf"), None, 0), "softcap must be a finite number >= 0 (got inf)"),
    ((-1, -1, 0.0, P, 2), "sink_heads=2 must be heads_q=4 (one sink per query head)"),
    ((-1, -1, 0.0, P, 0), "sink_heads=0 must be heads_q=4 (one sink per query head)"),
    ((-1, -1, 0.0, None, 4), "sink_heads must be 0 without sinks (got 4)"),
    ((-1, -1, 0.0, ctypes.c_void_p(4098), 4), "sinks must be 4-byte aligned"),
]


@pytest.mark.parametrize("entry,args", [("fa_fp8_forward_mod", PAD), ("fa_fp8_forward_varlen_mod", VAR), ("fa_fp8_forward_kvcache_mod", KV)])
def test_the_host_validates_the_three_arguments_by_name(entry, args):
    import flashattention_lab_cuda as ext

    fn = getattr(ext._lib, entry)
    assert len(args) + 5 == len(ext._SIGNATURES[entry][1]) and len(args) == len(ext._SIGNATURES[entry[:-4]][1])
    for tail, text in BAD:
        assert fn(*args, *tail) == INVALID_ARGUMENT
        assert ext._lib.fa_last_error().decode() == f"{entry}: {text}"
    # the parent's rules come first and keep their texts
    assert fn(None, *args[1:], -2, 0, 0.0, None, 0) == INVALID_ARGUMENT
    assert ext._lib.fa_last_error().decode() == f"{entry}: null tensor pointer"


def test_the_decode_split_rule_with_a_window():
    """fa_fp8_forward_kvcache_workspace_bytes_mod against the model of tests/fp8_kvcache_mod_ref.py: with a left bound the rule takes
    min(cache_len, L + max(R, 0) + Nq) (causal: R = 0) for cache_len, sinks raise one split to two, and without a window or sinks
    the need is the parent's"""
    import flashattention_lab_cuda as ext

    def need(b, hq, hkv, nq, cap, ns, causal, wl, wr, snk):
        return int(ext._lib.fa_fp8_forward_kvcache_workspace_bytes_mod(b, hq, hkv, nq, cap, 128, ns, causal, wl, wr, snk))

    def model(b, hq, hkv, nq, cap, ns, causal, wl, wr, snk):
        call = dict(B=b, hq=hq, hkv=hkv, nq=nq, num_splits=ns, causal=bool(causal), window=(wl, wr), sinks=torch.zeros(hq) if snk else None,
                    block_table=None, k_cache=torch.empty((1, cap, 0, 0)))
        s = km.num_splits(call)
        rows = b * hq * nq * s
        return s, (0 if s <= 1 else ((rows * 128 * 4 + 255) & ~255) + ((rows * 4 + 255) & ~255))

    shapes = [(32, 32, 8, 1, 32768), (4, 8, 2, 3, 1024), (1, 8, 8, 1, 100000), (2, 16, 2, 5, 4096)]
    for (b, hq, hkv, nq, cap), ns, causal, wl, wr, snk in itertools.product(shapes, (0, 1, 3), (0, 1), (-1, 0, 17, 128, 1023, 2000), (-1, 0, 40),
                                                                           (0, 1)):
        s, want = model(b, hq, hkv, nq, cap, ns, causal, wl, wr, snk)
        assert need(b, hq, hkv, nq, cap, ns, causal, wl, wr, snk) == want, (b, hq, hkv, nq, cap, ns, causal, wl, wr, snk, s)
        if wl < 0 and not snk:
            assert want == int(ext._lib.fa_fp8_forward_kvcache_workspace_bytes(b, hq, hkv, nq, cap, 128, ns))
    # the issue's decode row: a window of 1023 over 32768 cached keys is split as 1024 keys are, not as 32768
    assert km.num_splits(dict(B=1, hq=8, hkv=8, nq=1, num_splits=0, causal=True, window=(1023, -1), sinks=None, block_table=None,
                              k_cache=torch.empty((1, 32768, 0, 0)))) == 8
    assert km.num_splits(dict(B=1, hq=8, hkv=8, nq=1, num_splits=0, causal=True, window=(-1, -1), sinks=None, block_table=None,
                              k_cache=torch.empty((1, 32768, 0, 0)))) == 256
    assert need(2, 4, 2, 1, 1024, 0, 0, -2, 0, 0) == 0 and need(2, 4, 2, 1, 1024, 0, 0, 0, 0, 0) >= 0
    # the kernel's ranges: splits cut [lo, hi), lo the first 64-key tile a row of the tile sees, and cover it exactly once
    call = dict(km.build_call(1), num_splits=3)
    for lk in (0, 1, 65, 1000):
        for rt in range(1):
            r = km.split_ranges(call, lk, rt)
            lo = max(0, lk - 3 - 17) // 64 * 64
            assert r[0][0] == lo and all(a % 64 == 0 for a, _z in r)
            covered = sorted(j for a, z in r for j in range(a, z))
            assert covered == list(range(lo, lk))
