"""CPU: the proof that the sharp bar of the decode sweeps bites (tests/decode_baseline.py; the bar runs on the GPU in
tests/test_kvcache_sweep_gpu.py and tests/test_mla_routes_gpu.py).

  * the transcriptions of kv_num_splits and mla_split_rule against the library's host-only workspace-size entry points;
  * the baseline in fp64 without rounding is the reference again — kvcache_full_ref.full_reference on every case of the table at 1, 2
    and 5 splits, mla_reference and mla_sparse_reference on the route test's problem — at the 1e-10 tests/test_ex_sweep_cpu.py uses for the
    same statement about ex_full_ref.baseline; in fp32 with rounding it passes the decode tests' bar (check_out) and, rounded as a
    kernel returns results, the sharp bar at ratio <= 1;
  * mutants: each plausible decode bug, built into the fp64 evaluation and rounded as a kernel returns results, fails the sharp bar
    on every (case, S) it changes, and at least half of them pass the decode tests' bar somewhere: the gap, written down.

"Changes" is measured on the unrounded mutant: some tensor of some row group (the call, or one sequence) lies more than 1.5 bounds
from the reference.  The final rounding moves a result by at most eps / 2 of its size, and a bound is at least eps * max |fp64|, so
past 1.5 bounds the rounded mutant is past one bound whatever the rounding does; between 1 and 1.5 the rounding decides, and below
1 the bug is inside what the bar allows a correct kernel — there the case does not carry the bug (a seam key of negligible weight,
say), and the table printed per mutant says how many such cases there were.  The split mutants run at the case's own number of
splits and at five.

The first ten mutants are the ones the sweep was asked to reject, as stated.  On this table, with randn values and a sequence of 1
or 33 keys in every case, seven of them move o by more than 5e-2 somewhere in every case they touch, so they do not show the gap.
Five sharper ones of the same kinds were added, not swapped in — a scale, slope or partial that went through 16 bits on its way:
softmax_scale_as_bf16, k_descale_as_bf16, v_descale_as_bf16, alibi_slope_as_bf16 (a scale-side slip of at most 2^-9 relative) and
lse_partials_as_f16 (a combine weight that is slightly off).  They move o by well under 5e-2 and lse by under 1e-3 (1 + |lse|) on
many cases and are far outside the sharp bar on all they change."""
import functools

import pytest
import torch

from tests import decode_baseline as db
from tests import kvcache_sweep_cases as sc
from tests import test_mla_routes_gpu as routes
from tests.kvcache_full_ref import full_reference
from tests.mla_ref import mla_reference
from tests.mla_sparse_ref import mla_sparse_reference
from tests.test_kvcache_gpu import check
from tests.test_kvcache_sweep_gpu import check_out

IDS = [sc.case_id(i) for i in range(len(sc.CASES))]
CHANGED = 1.5
SPLIT_MUTANTS = ("seam_key_dropped", "tile_counted_from_zero", "sink_in_every_split", "combine_weight_from_split0", "lse_partials_as_f16")


@functools.lru_cache(maxsize=None)
def problem(i):
    kw = sc.call_keywords(sc.build_inputs(i))
    return kw, full_reference(**kw)


@functools.lru_cache(maxsize=None)
def base32(i, splits):
    return db.kv_baseline(problem(i)[0], splits)


# ---- the number of splits

def test_the_split_rules_are_the_librarys():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    seen = set()
    for i in range(len(sc.CASES)):
        kw = problem(i)[0]
        bsz, hq, hkv, nq, cap, d, total_q = db.kv_shape(kw)
        s, sink = db.kv_splits(kw), int(kw["sinks"] is not None)
        if total_q is not None:
            got = lib.fa_ex_kvcache_workspace_bytes_varlen(bsz, hq, hkv, total_q, nq, cap, d, kw["num_splits"], sink)
            want = db.workspace_bytes(hq * total_q, d, s)
        else:
            got = (lib.fa_ex_kvcache_workspace_bytes_sink if sink else lib.fa_ex_kvcache_workspace_bytes)(bsz, hq, hkv, nq, cap, d, kw["num_splits"])
            want = db.workspace_bytes(bsz * hq * nq, d, s)
        assert got == want, (IDS[i], s)
        if kw["num_splits"] == 0:
            seen.add(s)
    assert seen == {2}, seen      # a capacity of 192 keys and few workgroups: two splits of at least 128 keys
    # the rule itself, away from the table's one capacity, and the MLA forms' rule
    for bsz, (hq, hkv), nq, cap in ((1, (8, 8), 1, 32768), (3, (32, 8), 5, 1000), (64, (8, 1), 16, 4096), (2, (40, 2), 18, 100000)):
        s = db.kv_num_splits(bsz, hkv, ((hq // hkv) * nq + 15) // 16, cap)
        assert lib.fa_ex_kvcache_workspace_bytes(bsz, hq, hkv, nq, cap, 64, 0) == db.workspace_bytes(bsz * hq * nq, 64, s), (bsz, hq, hkv, nq, cap)
    for bsz, (hq, hkv), nq, keys in ((2, (16, 1), 1, 112), (2, (33, 1), 1, 112), (1, (17, 1), 1, 4096), (4, (128, 1), 2, 32768), (3, (64, 2), 1, 700)):
        s = db.mla_split_rule(bsz, hkv, (hq // hkv) * nq, keys)
        assert lib.fa_ex_kvcache_workspace_bytes_qv(bsz, hq, hkv, bsz * nq, nq, keys, 64, 0, 0, 512) == db.workspace_bytes(bsz * hq * nq, 512, s)
        s = db.mla_split_rule(bsz * nq, hkv, hq // hkv, keys)
        assert lib.fa_mla_sparse_workspace_bytes(bsz, hq, hkv, nq, keys, 0) == db.workspace_bytes(bsz * hq * nq, 512, s)
        assert lib.fa_mla_fp8_workspace_bytes(bsz, hq, 1, nq, 9999, keys, 1, 0) == db.workspace_bytes(bsz * hq * nq, 512, db.mla_split_rule(bsz * nq, 1, hq, keys))


# ---- the baseline against the references

def close64(o, lse, ro, rlse, what):
    torch.testing.assert_close(o, ro, rtol=1e-10, atol=1e-10, msg=lambda m: f"o {what}: {m}")
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin), what
    assert torch.equal(torch.isnan(lse), torch.isnan(rlse)) and bool((lse[~fin & ~torch.isnan(rlse)] == -float("inf")).all()), what
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-10, atol=1e-10, msg=lambda m: f"lse {what}: {m}")


def sharp(o, lse, r, base, dtype):
    return db.sharp_rows(o, lse, r.o, r.lse, base.o, base.lse, dtype, db.kv_groups(r))


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_the_baseline_of_the_case(i):
    kw, r = problem(i)
    dtype = kw["q"].dtype
    for splits in sorted({1, 2, 5, db.kv_splits(kw)}):
        what = f"{IDS[i]} S={splits}"
        b64 = db.kv_baseline(kw, splits, compute=torch.float64, tensor_dtype=None)
        close64(b64.o, b64.lse, r.o, r.lse, what)
        b32 = base32(i, splits)
        assert b32.o.dtype == torch.float32 and torch.equal(b32.o.to(dtype).float(), b32.o), what
        check_out(b32.o.to(dtype), b32.lse, r, dtype, what)
        bad, ratios, used = sharp(b32.o.to(dtype), b32.lse, r, b32, dtype)
        assert not bad and used <= 1.0 and all(v <= 1.0 for g in ratios.values() for v in g.values()), (what, bad, ratios)


MLA_PROBLEMS = [(form, dtype, hq, s) for form, splits in (("dense", (1, 3)), ("lists", (1, 2))) for dtype in (routes.BF16, routes.F16)
                for hq in routes.WAVES for s in splits]


def mla_baseline(form, dtype, hq, splits, **kw):
    pool, _cont = routes.caches(dtype)
    q, table, sl = routes.queries(dtype, hq), routes.pools()[2], torch.tensor(routes.LENS, dtype=torch.int32)
    if form == "dense":
        return db.mla_dense_baseline(q[..., 512:], q[..., :512], pool[..., 512:], pool[..., :512], sl, False, (-1, -1), routes.SCALE, table,
                                     splits=splits, **kw)
    return db.mla_list_baseline(q[..., 512:], q[..., :512], pool[..., 512:], pool[..., :512], routes.lists(), sl, False, routes.SCALE, table,
                                splits=splits, **kw)


@functools.lru_cache(maxsize=None)
def mla_base32(form, dtype, hq, splits):
    return mla_baseline(form, dtype, hq, splits)


def mla_sharp(o, lse, form, dtype, hq, splits):
    ro, rlse = routes.expected(form, dtype, hq)
    bo, bl = mla_base32(form, dtype, hq, splits)
    return db.sharp_rows(o, lse, ro, rlse, bo, bl, dtype, db.mla_groups(routes.LENS))


@pytest.mark.parametrize("form,dtype,hq,splits", MLA_PROBLEMS, ids=[routes.ident(*c) for c in MLA_PROBLEMS])
def test_the_mla_baseline_of_the_route_problem(form, dtype, hq, splits):
    ro, rlse = routes.expected(form, dtype, hq)
    o, lse = mla_baseline(form, dtype, hq, splits, compute=torch.float64, tensor_dtype=None)
    close64(o, lse, ro, rlse, routes.ident(form, dtype, hq, splits))
    o, lse = mla_base32(form, dtype, hq, splits)
    check(o.to(dtype), lse, ro, rlse, dtype)
    bad, _ratios, used = mla_sharp(o.to(dtype), lse, form, dtype, hq, splits)
    assert not bad and used <= 1.0


def test_the_mla_baseline_under_the_mask_and_with_more_heads():
    """what the route problem does not hold: several query tokens under the causal mask, a window, two K/V heads, a contiguous cache"""
    g = torch.Generator().manual_seed(11)
    q = torch.randn((2, 3, 6, 576), generator=g).to(routes.BF16)
    cache = torch.randn((2, 112, 2, 576), generator=g).to(routes.BF16)
    sl = torch.tensor([100, 37], dtype=torch.int32)
    ix = torch.randint(-1, 112, (2, 3, 2, 70), generator=g).to(torch.int32)
    for causal, window, splits in ((True, (-1, -1), 1), (True, (-1, -1), 3), (False, (40, 1), 2)):
        ro, rlse = mla_reference(q[..., 512:], q[..., :512], cache[..., 512:], cache[..., :512], sl, causal, window, routes.SCALE)
        o, lse = db.mla_dense_baseline(q[..., 512:], q[..., :512], cache[..., 512:], cache[..., :512], sl, causal, window, routes.SCALE,
                                       splits=splits, compute=torch.float64, tensor_dtype=None)
        close64(o, lse, ro, rlse, f"dense {causal} {window} {splits}")
    for causal, splits in ((False, 1), (True, 2), (True, 3)):
        ro, rlse = mla_sparse_reference(q[..., 512:], q[..., :512], cache[..., 512:], cache[..., :512], ix, sl, causal, routes.SCALE)
        o, lse = db.mla_list_baseline(q[..., 512:], q[..., :512], cache[..., 512:], cache[..., :512], ix, sl, causal, routes.SCALE,
                                      splits=splits, compute=torch.float64, tensor_dtype=None)
        close64(o, lse, ro, rlse, f"lists {causal} {splits}")


# ---- mutants

def carries(mutant, c, splits):
    """does case c at `splits` splits hold the feature the mutant breaks?"""
    e4m3 = c["cache"] == "e4m3"
    return {"v_from_next_slot": c["addr"].startswith("paged"),
            "v_descale_of_next_head": e4m3 and c["heads"][1] > 1,
            "k_descale_after_softcap": e4m3 and "softcap" in c["mods"],
            "seam_key_dropped": splits >= 2,
            "tile_counted_from_zero": sc.window_of(c["mask"])[0] >= 0,
            "sink_in_every_split": c["sinks"],
            "combine_weight_from_split0": splits >= 2,
            "tail_head_dims_zero": c["d"] in db.TAIL_DIMS,
            "k_descale_as_bf16": e4m3, "v_descale_as_bf16": e4m3, "alibi_slope_as_bf16": "alibi" in c["mods"],
            "lse_partials_as_f16": splits >= 2}.get(mutant, True)


def passes_check_out(o, lse, r, dtype):
    try:
        check_out(o, lse, r, dtype)
    except AssertionError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def mutant_record(mutant):
    """(carried, changed, failed the sharp bar, changed and passed the decode tests' bar, changed but survived) over the (case, S)"""
    carried = changed = failed = passed_project = 0
    survivors = []
    for i, c in enumerate(sc.CASES):
        kw, r = problem(i)
        dtype = kw["q"].dtype
        own = db.kv_splits(kw)
        for splits in sorted({own, 5} if mutant in SPLIT_MUTANTS else {own}):
            if not carries(mutant, c, splits):
                continue
            carried += 1
            m = db.kv_baseline(kw, splits, compute=torch.float64, tensor_dtype=None, mutant=mutant)
            base = base32(i, splits)
            if sharp(m.o, m.lse, r, base, dtype)[2] <= CHANGED:
                continue
            changed += 1
            o, lse = m.o.to(dtype), m.lse.float()      # as a kernel returns results (ex_full_ref.rounded)
            if sharp(o, lse, r, base, dtype)[0]:
                failed += 1
            else:
                survivors.append(f"{IDS[i]} S={splits}")
            passed_project += passes_check_out(o, lse, r, dtype)
    return carried, changed, failed, passed_project, survivors


@pytest.mark.parametrize("mutant", db.MUTANTS)
def test_the_sharp_bar_kills_the_mutant(mutant):
    carried, changed, failed, passed_project, survivors = mutant_record(mutant)
    print(f"mutant {mutant}: {carried} (case, S) carry the feature, {changed} are changed by more than the bound; the sharp bar fails "
          f"{failed} of them, the decode tests' bar passes {passed_project} of them")
    assert carried >= 3 and changed >= 3, f"{mutant}: {carried} carried, {changed} changed"
    assert failed == changed, f"{mutant} survives the sharp bar on {survivors}"


def test_the_decode_tests_bar_lets_half_of_the_mutants_through():
    rec = {m: mutant_record(m) for m in db.MUTANTS}
    through = [m for m, (_c, _ch, _f, passed, _s) in rec.items() if passed]
    print(f"mutants that pass check_out on a case they change: {len(through)} / {len(db.MUTANTS)}: {', '.join(through)}")
    assert 2 * len(through) >= len(db.MUTANTS), through


def test_the_gpu_files_sharp_out_passes_the_baseline_and_rejects_a_mutant():
    """the functions the GPU tests call, fed on the CPU: the rounded baseline in the kernel's place passes, a mutant does not"""
    from tests import test_kvcache_sweep_gpu as sweep

    i = next(i for i, c in enumerate(sc.CASES) if c["cache"] == "e4m3" and c["nnew"] and c["splits"] != 1)
    kw, r = sweep.case_and_reference(i)
    dtype = kw["q"].dtype
    k_big, v_big = kw["k_big"].clone(), kw["v_big"].clone()
    k_big[1:-1], v_big[1:-1] = r.k_cache, r.v_cache                       # the caches as the reference's append leaves them
    for splits in (None, 5):
        ra, ba = sweep.after_the_call(("cpu", i), kw, k_big, v_big, splits)
        sweep.sharp_out(ba.o.to(dtype), ba.lse, kw, ra, ba, IDS[i])
        m = db.kv_baseline(sc.call_keywords(kw), splits, compute=torch.float64, tensor_dtype=None, mutant="lse_partials_as_f16")
        sweep.check_out(m.o.to(dtype), m.lse.float(), r, dtype, IDS[i])
        with pytest.raises(AssertionError, match="sharp bar"):
            sweep.sharp_out(m.o.to(dtype), m.lse.float(), kw, ra, ba, IDS[i])
    form, dtype, hq, splits = "lists", routes.BF16, 17, 2
    what = "paged against contiguous: " + ", ".join(routes.routes(form, dtype, hq))
    o, lse = routes.baseline(form, dtype, hq, splits)
    routes.sharp_out(o.to(dtype), lse, form, dtype, hq, splits, what)
    o, lse = mla_baseline(form, dtype, hq, splits, compute=torch.float64, tensor_dtype=None, mutant="lse_plus_2e-4")
    check(o.to(dtype), lse.float(), *routes.expected(form, dtype, hq), dtype)
    with pytest.raises(AssertionError, match="sharp bar"):
        routes.sharp_out(o.to(dtype), lse.float(), form, dtype, hq, splits, what)


def mla_carries(mutant, form, splits):
    return {"list_tail_dropped": form == "lists", "seam_key_dropped": splits >= 2, "combine_weight_from_split0": splits >= 2}.get(mutant, True)


@pytest.mark.parametrize("mutant", db.MLA_MUTANTS)
def test_the_sharp_bar_kills_the_mla_mutant(mutant):
    carried = changed = failed = passed_project = 0
    for form, dtype, hq, splits in MLA_PROBLEMS:
        if not mla_carries(mutant, form, splits):
            continue
        carried += 1
        ro, rlse = routes.expected(form, dtype, hq)
        o, lse = mla_baseline(form, dtype, hq, splits, compute=torch.float64, tensor_dtype=None, mutant=mutant)
        if mla_sharp(o, lse, form, dtype, hq, splits)[2] <= CHANGED:
            continue
        changed += 1
        o, lse = o.to(dtype), lse.float()
        bad = mla_sharp(o, lse, form, dtype, hq, splits)[0]
        failed += bool(bad)
        try:
            check(o, lse, ro, rlse, dtype)
            passed_project += 1
        except AssertionError:
            pass
    print(f"MLA mutant {mutant}: {carried} route problems carry the feature, {changed} are changed by more than the bound; the sharp bar "
          f"fails {failed} of them, the decode tests' bar passes {passed_project} of them")
    assert carried >= 3 and changed >= 3 and failed == changed
