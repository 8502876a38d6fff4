"""GPU: the all-pairs sweep of KV-cache decoding (ex_kvcache_forward).  One test per case of tests/kvcache_sweep_cases.py: the inputs
are built on the CPU from the case's seed, the call runs once on caches cut out of the middle of larger buffers, and o, lse and
the caches are held to tests/kvcache_full_ref.full_reference — the whole call in fp64, which reads the keys as it appended them
itself.  The bars are the ones every decode test uses: tests.helpers.dtype_tolerances for o, rtol = atol = 1e-3 for finite lse,
the -inf pattern and o == 0 on rows without a visible key exact; every cache element outside the reference's write mask keeps
its bits; appended elements are k_new / v_new's own bits, or judged by the rotary (kvcache_rotary_ref.check_caches) and e4m3
(test_kvcache_fp8_gpu.check_appended) tests' rules.  The cases with a head dim or group size no other test runs also run at
fixed split counts: 1 and 5 against the reference, and a packed call bitwise against the padded call on each sequence alone.

Every case, and every fixed-split extra, is also held to the sharp bar (sharp_out): tests/ex_full_ref.sharp_bar's inequality against
tests/decode_baseline.kv_baseline, the rounding model of the decode kernels, per call and per sequence.  Reference and baseline of
that bar attend over the cache contents the call left behind, read back from the device: the append is judged by
check_caches_after, whose rules let a rotated or quantised element differ from the reference's by one step, and that step is
neither charged to the attention kernel nor used to excuse it.  tests/test_decode_sharp_cpu.py proves on the CPU that this bar
rejects the decode bugs the bars above let through; profiles/decode_sweep.md records the measured ratios."""
import functools

import pytest
import torch

from tests import decode_baseline as db
from tests import kvcache_sweep_cases as sc
from tests.helpers import dtype_tolerances
from tests.kvcache_full_ref import full_reference
from tests.kvcache_fp8_ref import E4M3
from tests.kvcache_rotary_ref import check_caches

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [sc.case_id(i) for i in range(len(sc.CASES))]


def bits(t):
    return t.view(torch.uint8) if t.dtype == E4M3 else t.view(torch.int16)


def to_dev(t):
    """a CPU tensor on the device; e4m3 travels as its bytes"""
    return t.view(torch.uint8).to(DEV).view(E4M3) if t.dtype == E4M3 else t.to(DEV)


def run(kw, **over):
    """the call kw on the device, on fresh copies of the canary buffers: (o, lse, k_big, v_big) with the last two on the CPU"""
    return run_on(kw, to_dev(kw["k_big"]), to_dev(kw["v_big"]), **over)


def check_out(o, lse, r, dtype, what=""):
    """o within dtype_tolerances, finite lse at rtol = atol = 1e-3, the -inf pattern exact, o == 0 exactly on rows without a visible
    key, nothing NaN; rows that no sequence owns are not compared"""
    o, lse = o.double(), lse.double()
    if r.lse.dim() == 2:      # packed: (total_q, H_q, d), (H_q, total_q)
        o, lse, ro, rlse = o[r.own].permute(1, 0, 2), lse[:, r.own], r.o[r.own].permute(1, 0, 2), r.lse[:, r.own]
    else:                     # (B, Nq, H_q, d), (B, H_q, Nq)
        o, ro, rlse = o.permute(0, 2, 1, 3), r.o.permute(0, 2, 1, 3), r.lse
    assert not torch.isnan(o).any() and not torch.isnan(lse).any(), what
    fin = torch.isfinite(rlse)
    print(f"{what} max |o - ref| = {(o - ro).abs().max().item() if o.numel() else 0.0:.3e}, "
          f"max |lse - ref| = {(lse[fin] - rlse[fin]).abs().max().item() if fin.any() else 0.0:.3e}")
    torch.testing.assert_close(o, ro, **dtype_tolerances(dtype), msg=lambda m: f"o {what}: {m}")
    assert torch.equal(torch.isfinite(lse), fin), f"lse -inf pattern {what}"
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-3, atol=1e-3, msg=lambda m: f"lse {what}: {m}")
    novis = r.novis[r.own].unsqueeze(0).expand(rlse.shape) if r.lse.dim() == 2 else r.novis.unsqueeze(1).expand(rlse.shape)
    assert (o[novis] == 0).all(), f"o != 0 on rows without a visible key {what}"


AFTER = {}


def after_the_call(key, kw, k_big, v_big, splits):
    """(reference, baseline at `splits` splits; None: the call's own) of the call kw over the caches it left behind, computed once
    per problem (key) and split count: the append does not depend on the split count, and a repeated call leaves the same bits"""
    caches = (k_big[1:-1], v_big[1:-1])
    hit = AFTER.get(key)
    if hit is None or not (torch.equal(bits(hit["caches"][0]), bits(caches[0])) and torch.equal(bits(hit["caches"][1]), bits(caches[1]))):
        AFTER[key] = hit = dict(caches=caches, r=full_reference(**sc.call_keywords(kw), caches_after=caches), base={})
    if splits not in hit["base"]:
        hit["base"][splits] = db.kv_baseline(sc.call_keywords(kw), splits, caches_after=caches)
    return hit["r"], hit["base"][splits]


def family(kw, splits):
    """the split kernel instantiation a call launches and how its results are finished (csrc/fa_decode.hip: kv_dispatch, kv_launch)"""
    d = kw["q"].shape[-1]
    feat = (1 if kw["rotary_cos"] is not None else 0) | (2 if kw["k_cache"].dtype == E4M3 else 0)   # kKvRot | kKvQ8
    end = "kv_combine_kernel<SINK>" if kw["sinks"] is not None else "kv_combine_kernel" if splits > 1 else "direct"
    return f"kv_split_kernel<D={64 if d <= 64 else 128 if d <= 128 else 256},{'paged' if kw['block_table'] is not None else 'contig'},FEAT={feat}>+{end}"


def sharp_out(o, lse, kw, r, base, what=""):
    """tests/ex_full_ref.sharp_bar on o and lse — max |kernel - fp64| <= 2 * max |baseline - fp64| + eps * max |fp64|, eps of the
    tensor dtype for o and of float32 for lse — over the call's owned rows and over each sequence's rows alone (a case holds
    lengths 0, 1, 33, 100 and full side by side, and the short rows, where |o| ~ |v|, would otherwise set the maximum for the
    192-key rows).  A sequence without a visible key stays under check_out's exact rules only; no other (case, sequence) is left
    out.  r and base: after_the_call's."""
    bad, ratios, used = db.sharp_rows(o, lse, r.o, r.lse, base.o, base.lse, kw["q"].dtype, db.kv_groups(r))
    top = lambda t: max([g[t] for n, g in ratios.items() if n != "call" and t in g], default=0.0)   # noqa: E731
    print(f"decode_sweep_ratio {what} o={ratios['call'].get('o', 0.0):.3f} lse={ratios['call'].get('lse', 0.0):.3f} per sequence o={top('o'):.3f} "
          f"lse={top('lse'):.3f} used={used:.3f} family={family(kw, base.splits)}")
    assert not bad, f"sharp bar {what}: " + "; ".join(bad)


def padded_new(per_seq, hkv, d, dtype):
    """(B, max nnew_b, H_kv, d): the per-sequence new tokens side by side (the append helpers index [b, n])"""
    out = torch.zeros((len(per_seq), max(1, max(t.shape[0] for t in per_seq)), hkv, d), dtype=dtype)
    for b, t in enumerate(per_seq):
        out[b, :t.shape[0]] = t
    return out


def check_caches_after(kw, r, k_big, v_big, what=""):
    from tests.test_kvcache_fp8_gpu import check_appended

    c_e4m3, rotary = kw["k_cache"].dtype == E4M3, kw["rotary_cos"] is not None
    # 1. nothing outside the write mask moved, the canary margins included
    for name, got, before, mask in (("K", k_big, kw["k_big"], r.k_mask), ("V", v_big, kw["v_big"], r.v_mask)):
        keep = torch.ones(before.shape, dtype=torch.bool)
        keep[1:-1] = ~mask
        assert torch.equal(bits(got)[keep], bits(before)[keep]), f"{name} cache changed outside the appended tokens {what}"
    if not r.slots:
        return
    kc, vc = k_big[1:-1], v_big[1:-1]
    hkv, d = kc.shape[2], kc.shape[3]
    dtype = kw["q"].dtype
    k16, v16 = padded_new(r.k_new16, hkv, d, dtype), padded_new(r.v_new16, hkv, d, dtype)
    if not c_e4m3 and not rotary:     # 2. plain append: the new tokens' own bits
        for b, n, unit, pos in r.slots:
            assert torch.equal(bits(kc[unit, pos]), bits(k16[b, n])) and torch.equal(bits(vc[unit, pos]), bits(v16[b, n])), (what, b, n)
    elif not c_e4m3:                  # 3. rotated: the rotary tests' rule
        raw = padded_new([kw["k_new"][b] if kw["cu_seqlens_k_new"] is None else
                          kw["k_new"][int(kw["cu_seqlens_k_new"][b]):int(kw["cu_seqlens_k_new"][b + 1])] for b in range(sc.B)], hkv, d, dtype)
        check_caches(kc, vc, r.k_cache, r.v_cache, r.k_exact, r.L, raw, 2 * kw["rotary_cos"].shape[1], kw["block_table"], kw["cache_batch_idx"])
    else:                             # 4. quantised: the e4m3 tests' rules
        ones = torch.ones((sc.B, hkv), dtype=torch.float32)
        kd = kw["k_descale"] if kw["k_descale"] is not None else ones
        vd = kw["v_descale"] if kw["v_descale"] is not None else ones
        gk, gv = kc.view(torch.uint8), vc.view(torch.uint8)
        check_appended(gv, kw["v_cache"].view(torch.uint8), v16, vd, r.slots)
        if not rotary:
            check_appended(gk, kw["k_cache"].view(torch.uint8), k16, kd, r.slots)
        else:   # against quantize(the reference's rotation): at most 2 bytes in 1000 differ (test_rotary_with_an_e4m3_cache)
            want = r.k_cache.view(torch.uint8)
            mism = sum(int((gk[u, p] != want[u, p]).sum()) for _b, _n, u, p in r.slots)
            assert mism * 1000 <= 2 * len(r.slots) * hkv * d, f"{mism} appended K bytes differ from quantize(rotated reference) {what}"


@functools.lru_cache(maxsize=None)
def case_and_reference(i, packed_variant=False):
    c = sc.CASES[i]
    if packed_variant and not c["queries"].startswith("packed"):
        c = dict(c, queries="packed7" if int(c["queries"][2:]) <= 7 else "packed18")
    kw = sc.build_inputs(i, c)
    r = full_reference(**sc.call_keywords(kw))
    return kw, r


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_case(i):
    kw, r = case_and_reference(i)
    o, lse, k_big, v_big = run(kw)
    assert o.shape == r.o.shape and lse.shape == r.lse.shape and lse.dtype == torch.float32 and o.dtype == kw["q"].dtype
    check_out(o, lse, r, kw["q"].dtype, IDS[i])
    check_caches_after(kw, r, k_big, v_big, IDS[i])
    sharp_out(o, lse, kw, *after_the_call(i, kw, k_big, v_big, None), IDS[i])


EXTRA = sc.fixed_split_cases()


@pytest.mark.parametrize("i", EXTRA, ids=[IDS[i] for i in EXTRA])
def test_fixed_splits_match_the_reference(i):
    kw, r = case_and_reference(i)
    for splits in (1, 5):
        o, lse, k_big, v_big = run(kw, num_splits=splits)
        check_out(o, lse, r, kw["q"].dtype, f"{IDS[i]} S={splits}")
        check_caches_after(kw, r, k_big, v_big, f"{IDS[i]} S={splits}")
        sharp_out(o, lse, kw, *after_the_call(i, kw, k_big, v_big, splits), f"{IDS[i]} S={splits}")


@pytest.mark.parametrize("i", EXTRA, ids=[IDS[i] for i in EXTRA])
def test_packed_call_is_bitwise_the_padded_call_on_each_sequence(i):
    """the case with packed queries (as it is, or with its queries packed): every sequence's rows of o and lse and its appended
    tokens are the bits of the padded call on that sequence alone, at one and at five splits.  A sequence without q tokens has
    no rows; one that appends nothing while rotary is on has no padded call (rotary needs new keys)."""
    kw, r = case_and_reference(i, True)
    cu = [int(x) for x in kw["cu_seqlens_q"]]
    ckn = [int(x) for x in kw["cu_seqlens_k_new"]] if kw["cu_seqlens_k_new"] is not None else None
    whole = kw["block_table"] is not None or kw["cache_batch_idx"] is not None      # the padded call takes the whole pool / cache
    compared = 0
    for splits in (1, 5):
        o, lse, k_big, v_big = run(kw, num_splits=splits)
        check_out(o, lse, r, kw["q"].dtype, f"{IDS[i]} packed S={splits}")
        for b in range(sc.B):
            lo, hi = cu[b], cu[b + 1]
            if hi == lo or (kw["rotary_cos"] is not None and r.nnew[b] == 0):
                continue
            one = dict(kw, q=kw["q"][lo:hi].unsqueeze(0), cu_seqlens_q=None, cu_seqlens_k_new=None, max_seqlen_q=None,
                       cache_seqlens=kw["cache_seqlens"][b:b + 1], k_new=None, v_new=None)
            if r.nnew[b]:
                one.update(k_new=kw["k_new"][ckn[b]:ckn[b + 1]].unsqueeze(0), v_new=kw["v_new"][ckn[b]:ckn[b + 1]].unsqueeze(0))
            for name in ("block_table", "cache_batch_idx", "cache_leftpad", "k_descale", "v_descale"):
                if kw[name] is not None:
                    one[name] = kw[name][b:b + 1]
            if kw["alibi_slopes"] is not None and kw["alibi_slopes"].dim() == 2:
                one["alibi_slopes"] = kw["alibi_slopes"][b:b + 1]
            over = dict(num_splits=splits)
            kb, vb = to_dev(kw["k_big"]), to_dev(kw["v_big"])
            if not whole:
                over.update(k_cache=kb[1 + b:2 + b], v_cache=vb[1 + b:2 + b])
            o1, lse1, k1, v1 = run_on(one, kb, vb, **over)
            assert torch.equal(o[lo:hi], o1[0]) and torch.equal(lse[:, lo:hi], lse1[0]), (IDS[i], splits, b)
            for bb, _n, unit, pos in r.slots:
                if bb == b:
                    assert torch.equal(bits(k_big[1 + unit, pos]), bits(k1[1 + unit, pos])), (IDS[i], splits, b)
                    assert torch.equal(bits(v_big[1 + unit, pos]), bits(v1[1 + unit, pos])), (IDS[i], splits, b)
            compared += 1
    assert compared >= 2


def run_on(kw, k_big, v_big, **over):
    """run() on device buffers the caller made"""
    import flashattention_lab_cuda as ext

    args = {k: (to_dev(v) if isinstance(v, torch.Tensor) else v) for k, v in sc.call_keywords(kw).items() if k not in ("k_cache", "v_cache")}
    args.update(k_cache=k_big[1:-1], v_cache=v_big[1:-1])
    args.update(over)
    o, lse = ext.ex_kvcache_forward(**args)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), k_big.cpu(), v_big.cpu()
