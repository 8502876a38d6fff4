"""CPU: the table of the plain-path sweep (tests/hot_cases.py), the baseline models of its routes (tests/ex_full_ref.Model) and the
hot-path mutants (ex_full_ref.HOT_MUTANTS) — everything tests/test_hot_sweep_gpu.py relies on that needs no GPU."""
import functools
import itertools

import pytest
import torch

from tests import ex_full_ref as fr
from tests import ex_sweep_cases as sc
from tests import hot_cases as hc


# ---- the table

def test_table_is_deterministic_and_within_its_cap():
    assert len(hc.CASES) <= hc.MAX_CASES
    assert hc.generate() == hc.CASES
    assert len({hc.case_name(c) for c in hc.CASES}) == len(hc.CASES)


def test_every_legal_pair_is_covered_and_every_case_is_legal():
    covered = set()
    for c in hc.CASES:
        assert hc.case_legal(c), c
        covered |= hc.pairs_of(c)
    assert hc.all_pairs() <= covered
    for axis, values in hc.AXES.items():
        assert {c[axis] for c in hc.CASES} == set(values), axis


def test_the_shapes_are_the_small_ones_of_the_issue():
    for bh, nq, nk in hc.AXES["shape"]:
        assert bh == (5 if max(nq, nk) <= 130 else 3) and max(nq, nk) <= 1100
    assert {s[1] for s in hc.ALL5} == {31, 130, 512, 513, 1100}
    assert {s[1:] for s in hc.NQNK} == {(300, 1100), (1100, 300), (1, 513)}
    assert not any(c["mask"] == "causal" and c["shape"][1] > c["shape"][2] for c in hc.CASES)
    assert all(c["dtype"] != "f32" or hc.route_of(c)["fwd"] == "fwd_generic" for c in hc.CASES)       # f32 on the exact routes only
    assert all(c["d"] != 20 or hc.route_of(c)["fwd"] == "fwd_generic" for c in hc.CASES)


# what each route is in the table for: a predicate on route_of that at least one of its cases must meet
def _has(kernel):
    return lambda ro: kernel in ro["fwd"] or any(kernel in k for k in ro["bwd"])


REACHES = {
    "auto": [_has("fwd_mfma_kernel<128,KB=4,TPW=1,W4>"), _has("fwd_mfma_kernel<64,KB=4,TPW=1,W4>"), _has("fwd_mfma_kernel<256,KB=2"),
             _has("bwd_dq_mfma_kernel<256"), _has("bwd_dkdv_mfma_kernel<256"), _has("bwd_dq_mfma_kernel<128,KT=1,TPW=2,PAD>"),
             _has("bwd_dkdv_mfma_kernel<64,TPW=2,PAD>"), lambda ro: ro["chunks"] == 1],
    "sg1": [_has("fwd_mfma_kernel<64,KB=2,TPW=1>"), _has("fwd_mfma_kernel<64,KB=4,TPW=2,PAD>"), _has("fwd_mfma_stag_kernel<128,KB=4,RD=4,KA,PAD>"),
            _has("fwd_mfma_kernel<256,KB=2,TPW=1,PAD>"), _has("fwd_mfma_kernel<256,KB=2,TPW=1>"), _has("fwd_mfma_stag_kernel<128,KB=4,RD=4,KA>")],
    "sg2": [_has("fwd_mfma_kernel<128,KB=4,TPW=1,W4>"), _has("fwd_mfma_kernel<64,KB=4,TPW=1,W4>"), _has("bwd_dq_mfma_kernel<128,KT=1,TPW=2,W4>"),
            _has("bwd_dkdv_mfma_kernel<128,TPW=1,W4>"), _has("bwd_dkdv_mfma_kernel<64,TPW=1,W4>")],
    "lock128": [_has("fwd_mfma_kernel<128,KB=4,TPW=1>"), _has("fwd_mfma_kernel<128,KB=4,TPW=2>"), _has("fwd_mfma_kernel<128,KB=4,TPW=1,PAD>")],
    "stag128": [_has("fwd_mfma_stag_kernel<128,KB=4,RD=4,KA>"), _has("fwd_mfma_stag_kernel<64,KB=4,two-buffer>")],
    "stag64": [_has("fwd_mfma_stag_kernel<128,KB=2,two-buffer>")],
    "two_buffer": [_has("fwd_mfma_stag_kernel<128,KB=4,two-buffer>")],
    "fwd_kb1": [_has("fwd_mfma_kernel<128,KB=1,")],
    "fwd_kb2": [_has("fwd_mfma_kernel<128,KB=2,"), _has("fwd_mfma_kernel<64,KB=2,")],
    "fwd_tpw1": [_has("fwd_mfma_kernel<128,KB=4,TPW=1>"), _has("fwd_mfma_kernel<64,KB=4,TPW=1>")],
    "fwd_tpw2": [_has("fwd_mfma_kernel<128,KB=4,TPW=2>")],
    "fwd_eager": [_has("fwd_mfma_kernel<128,KB=4,EAGER>")],
    "fwd_hs": [_has("fwd_mfma_kernel<128,KB=4,HS>")],
    "fwd_rs": [_has("fwd_mfma_kernel<128,KB=4,RS>")],
    "fwd_rd6": [_has("fwd_mfma_stag_kernel<128,KB=4,RD=6>")],
    "fwd_rd8": [_has("fwd_mfma_stag_kernel<128,KB=4,RD=8>")],
    "fwd_w2": [_has("fwd_mfma_stag_kernel<128,KB=4,RD=6,W2>")],
    "handover": [_has("bwd_dq_ds_kernel<NW=4>"), _has(",DS>"), lambda ro: ro["chunks"] == 1],
    "handover_w4": [_has("bwd_dq_ds_kernel<NW=4>")],
    "handover_chunk4": [lambda ro: ro["chunks"] == 3],
    "handover_chunk1": [lambda ro: ro["chunks"] > 1],
    "recompute": [lambda ro: ro["bwd"] == ("bwd_dq_w4_kernel", "bwd_dkdv_w4_kernel<KR=3>")],
    "w8": [_has("bwd_dq_mfma_kernel<128,KT=1,TPW=2>"), _has("bwd_dkdv_mfma_kernel<128,TPW=1,STG>"), _has("bwd_dkdv_mfma_kernel<128,TPW=2>"),
           lambda ro: ro["bwd"][0] == "bwd_prep_kernel" and "bwd_dkdv_mfma_kernel<64,TPW=" in ro["bwd"][1]],
    "dkdv4": [_has("bwd_mfma_kernel<128>")],
    "atomic": [_has("bwd_mfma_kernel<128,FUSED_DQ>"), _has("dq_convert_kernel")],
    "dq_tpw1": [_has("bwd_dq_mfma_kernel<128,KT=1,TPW=1>")],
    "dq_tpw2": [_has("bwd_dq_mfma_kernel<128,KT=1,TPW=2>")],
    "dkdv_tpw1": [_has("bwd_dkdv_mfma_kernel<128,TPW=1,STG>")],
    "dkdv_tpw2": [_has("bwd_dkdv_mfma_kernel<128,TPW=2>")],
    "dq_nlf": [_has("bwd_dq_mfma_kernel<128,KT=1,TPW=2,NLF>")],
    "dq_w4": [_has("bwd_dq_mfma_kernel<128,KT=1,TPW=2,W4>")],
    "dq_kt2": [_has("bwd_dq_mfma_kernel<128,KT=2,TPW=1>")],
    "dkdv_kreg1": [_has("bwd_dkdv_mfma_kernel<64,KREG,TPW=1>")],
    "dkdv_kreg2": [_has("bwd_dkdv_w4_kernel<KR=0")],
    "dkdv_kreg3": [_has("bwd_dkdv_w4_kernel<KR=1")],
    "dkdv_kreg4": [_has("bwd_dkdv_w4_kernel<KR=2")],
    "dkdv_stg1": [_has("bwd_dkdv_mfma_kernel<64,TPW=1,STG>")],
    "dkdv_stg2": [_has("bwd_dkdv_mfma_kernel<128,TPW=1>")],
    "f32": [_has("fwd_generic")],
    "d20": [_has("fwd_generic")],
    "misaligned": [_has("fwd_generic")],
    "mode1": [_has("fwd_generic")],
    "nqnk": [_has("fwd_mfma_stag_kernel<128,KB=4,RD=4,KA>"), lambda ro: ro["bwd"] == ("bwd_dq_w4_kernel", "bwd_dkdv_w4_kernel<KR=3>"),
             lambda ro: ro["chunks"] == 1],
    "nqnk_handover": [lambda ro: ro["chunks"] == 1],
}


def test_every_route_is_the_route_of_a_case():
    assert set(REACHES) == set(hc.ROUTES)
    for route, wants in REACHES.items():
        ros = [hc.route_of(c) for c in hc.CASES if c["route"] == route]
        assert ros, route
        for n, want in enumerate(wants):
            assert any(want(ro) for ro in ros), (route, n, [(ro["fwd"], ro["bwd"]) for ro in ros])


def test_the_options_of_a_route_decide_its_kernels_on_a_case_of_it():
    """a route whose options the dispatch ignored would run another route's kernels under its name: against the same case without
    the options that make the route what it is (on `auto`, or on `sg1` where the route carries small_grid = 1; `nqnk` for the
    Nq != Nk hand-over), route_of differs on at least one case of every route.  (Not on every case: small_grid = 2, fwd_stag = 2 and
    dq = 6 force what the rules themselves pick for some of the table's launches.)"""
    for route, r in hc.ROUTES.items():
        if route in ("auto", "sg1", "f32", "d20", "misaligned", "mode1", "nqnk") or r["mode"]:
            continue
        other = "nqnk" if route == "nqnk_handover" else "sg1" if r["opts"].get("small_grid") == 1 else "auto"
        differs = []
        for c in (c for c in hc.CASES if c["route"] == route):
            a, b = hc.route_of(c), hc.route_of(dict(c, route=other))
            differs.append((a["fwd"], a["bwd"], a["chunks"]) != (b["fwd"], b["bwd"], b["chunks"]))
        if route == "handover_w4":      # below 160 workgroups the rule picks the 4-wave product itself: the option decides at bh = 160
            big = dict(route=route, dtype="bf16", mask="none", d=128, shape=(160, 1100, 1100), scale="default")
            differs.append(hc.route_of(big)["bwd"] != hc.route_of(dict(big, route="handover"))["bwd"])
        assert any(differs), route


def test_no_two_routes_are_the_same_call():
    sig = lambda r: (tuple(sorted(r["opts"].items())), r["mode"], r["api"], r["misaligned"],   # noqa: E731
                     r["dtypes"] if not r["opts"] else None, r["d"] if not r["opts"] else None)
    sigs = [sig(r) for r in hc.ROUTES.values()]
    assert len(set(sigs)) == len(sigs)
    for r in hc.ROUTES.values():
        assert r["why"] and ".hip" in r["why"]


def test_every_option_of_design_6b_that_computes_the_function_has_its_values_in_the_table():
    want = {"fwd_kb": {1, 2}, "fwd_stag": {1, 2, 3, 4}, "fwd_tpw": {1, 2}, "dq_tpw": {1, 2}, "dkdv_tpw": {1, 2}, "fwd_rs": {1}, "fwd_eager": {1},
            "fwd_hs": {1}, "dq_kt": {2}, "dq_nlf": {1}, "dq_w4": {1, 3}, "small_grid": {1, 2}, "dkdv": {4, 5, 8}, "dq": {5, 6, 8},
            "dkdv_kreg": {1, 2, 3, 4}, "dkdv_stg": {1, 2}, "fwd_rd": {6, 8}, "fwd_w2": {1}}
    have = {}
    for r in hc.ROUTES.values():
        for k, v in r["opts"].items():
            have.setdefault(k, set()).add(v)
    assert "ds_chunk_mb" in have
    have.pop("ds_chunk_mb")
    assert have == want
    assert {r["mode"] for r in hc.ROUTES.values()} == {0, 1, 2}


def test_the_default_rules_reach_the_headline_kernels_at_a_real_launch_size():
    big = dict(route="auto", dtype="bf16", d=128, shape=(160, 1100, 1100), scale="default")
    a, b = hc.route_of(dict(big, mask="none")), hc.route_of(dict(big, mask="causal"))
    assert a["fwd"] == "fwd_mfma_stag_kernel<128,KB=4,RD=4,KA>" and b["fwd"] == "fwd_mfma_kernel<128,KB=4,TPW=2>"
    for ro in (a, b):
        assert ro["bwd"] == ("bwd_prep_kernel", "bwd_dkdv_w4_kernel<KR=3,DS>", "bwd_dq_ds_kernel<NW=8>") and ro["chunks"] == 1
    assert not any("NW=8" in k for c in hc.CASES for k in hc.route_of(c)["bwd"])      # the table's launches are too small for it


# ---- the baseline and its models

def test_the_default_model_is_the_baseline_of_the_extended_sweep():
    """The defaults of Model are the rounding points baseline had before it took a model: the same results bit for bit on three
    sweep cases (16-bit packed with dropout, ALiBi, sinks and dlse; 16-bit padded with a mask and a softcap; float32 padded) whether
    the model is left out, passed as Model() or spelled out — and the default path performs none of the operations the models
    added (no exp2, no fused multiply-add, no rounding of P for the row sum)."""
    assert fr.DEFAULT_MODEL == fr.Model() == fr.Model(key_tile=64, lazy_rescale=False, exp2=False, rowsum_rounded_p=False,
                                                      dk_ds_from_rounded_p=False, f32_inside=False, fma_chain=False)
    for i in (1, 3, 21):
        call = sc.build_inputs(i)
        a = fr.baseline(call)
        real_exp2, real_fma = torch.exp2, fr._fma

        def forbidden(*_a, **_k):
            raise AssertionError("the default model took a path of the plain-path models")
        had_softcap = call["softcap"] > 0.0
        try:
            fr._fma = forbidden
            if not had_softcap:                 # (the softcap's tanh is an exp2 of its own: mod_softcap)
                torch.exp2 = forbidden
            b = fr.baseline(call, model=fr.Model(key_tile=64, lazy_rescale=False, exp2=False, rowsum_rounded_p=False,
                                                 dk_ds_from_rounded_p=False, f32_inside=False, fma_chain=False))
        finally:
            torch.exp2, fr._fma = real_exp2, real_fma
        for n in fr.TENSORS:
            x, y = getattr(a, n), getattr(b, n)
            assert (x is None and y is None) or torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0)), (i, n)


MODELS = sorted({hc.route_of(c)["model"] for c in hc.CASES} | {fr.Model(key_tile=128, lazy_rescale=True, exp2=True)})


def test_the_models_of_the_table():
    assert fr.Model(key_tile=128, lazy_rescale=True, exp2=True) in MODELS                                       # the hot forward
    assert {m.key_tile for m in MODELS} == {32, 64, 128}
    assert any(m.rowsum_rounded_p for m in MODELS) and any(m.dk_ds_from_rounded_p for m in MODELS) and any(not m.lazy_rescale and m.exp2 for m in MODELS)
    assert any(m.f32_inside and m.fma_chain for m in MODELS)


@pytest.mark.parametrize("model", MODELS, ids=lambda m: "-".join(str(int(x)) for x in m))
@pytest.mark.parametrize("mask", hc.BOTH)
def test_every_model_in_fp64_without_rounding_is_the_reference(model, mask):
    for key in (((5, 130, 130), 64, "bf16", mask, 0.37), ((3, 300, 513), 128, "f16", mask, "default")):
        call = hc.build_call(key)
        ref = fr.full_reference(call)
        got = fr.baseline(call, compute=torch.float64, tensor_dtype=None, model=model)
        for n in ("o", "lse", "dq", "dk", "dv"):
            err = (getattr(got, n) - getattr(ref, n)).abs().max().item()
            assert err <= 1e-10 * max(1.0, getattr(ref, n).abs().max().item()), (n, err)


def test_the_lazy_rescale_and_the_exp2_domain_round_elsewhere():
    """the fields are not decoration: in float32 each moves the result's last bits"""
    call = hc.build_call(((3, 513, 513), 128, "bf16", "causal", "default"))
    a = fr.baseline(call, model=fr.Model(key_tile=128))
    for m in (fr.Model(key_tile=128, lazy_rescale=True), fr.Model(key_tile=128, exp2=True), fr.Model(key_tile=128, rowsum_rounded_p=True)):
        assert not torch.equal(a.lse, fr.baseline(call, model=m).lse), m
    b = fr.baseline(call, model=fr.Model(key_tile=128, dk_ds_from_rounded_p=True))
    assert torch.equal(a.dq, b.dq) and torch.equal(a.dv, b.dv) and not torch.equal(a.dk, b.dk)


# ---- mutants

MUTANT_CASES = [i for i, c in enumerate(hc.CASES) if c["dtype"] != "f32" and c["d"] in (128, 64) and hc.ROUTES[c["route"]]["api"] == "plain"
                and hc.route_of(c)["fwd"] != "fwd_generic"]
CAUSAL_ONLY = ("causal_tail_keys_dropped", "diagonal_mask_shifted")


@functools.lru_cache(maxsize=None)
def refs(key):
    call = hc.build_call(key)
    return call, fr.full_reference(call)


@functools.lru_cache(maxsize=None)
def base(key, model):
    return fr.baseline(refs(key)[0], model=model)


@functools.lru_cache(maxsize=None)
def mutated(key, mutant):
    call, ref = refs(key)
    return fr.rounded(fr.hot_mutant(call, ref, mutant), call["dtype"])


@functools.lru_cache(maxsize=None)
def mutant_record(mutant):
    """(cases tried, cases failing the sharp bar whole or per band, cases failing the whole-tensor sharp bar, cases failing
    dtype_tolerances alone, cases failing the project's whole bar)"""
    tried, sharp, whole, tol_only, project = 0, [], [], [], []
    for i in MUTANT_CASES:
        c = hc.CASES[i]
        if mutant in CAUSAL_ONLY and c["mask"] != "causal":
            continue
        key = hc.problem_key(c)
        (call, ref), b, got = refs(key), base(key, hc.route_of(c)["model"]), mutated(key, mutant)
        tried += 1
        w = bool(fr.sharp_bar(got, ref, b, call["dtype"])[0])
        if w:
            whole.append(i)
        if w or (call["causal"] and fr.banded_sharp_bar(got, ref, b, call["dtype"])[0]):
            sharp.append(i)
        if fr.project_bar(got, ref, call["dtype"], only_tolerances=True):
            tol_only.append(i)
        if fr.project_bar(got, ref, call["dtype"]):
            project.append(i)
    return tried, sharp, whole, tol_only, project


@pytest.mark.parametrize("mutant", fr.HOT_MUTANTS)
def test_the_sharp_bar_kills_the_hot_mutant(mutant):
    tried, sharp, whole, tol_only, project = mutant_record(mutant)
    print(f"hot mutant {mutant}: {tried} cases; the sharp bar (whole or per band) fails {len(sharp)}, whole tensors alone {len(whole)}, "
          f"dtype_tolerances alone {len(tol_only)}, the project's whole bar {len(project)}")
    assert tried >= 3 and sharp, f"{mutant} survives the sharp bar on all {tried} cases"


def test_count_the_hot_mutants_each_bar_kills():
    rec = {m: mutant_record(m) for m in fr.HOT_MUTANTS}
    for m in fr.HOT_MUTANTS:
        tried, sharp, whole, tol_only, project = rec[m]
        print(f"  {m}: cases {tried}, sharp {len(sharp)}, sharp whole-tensor {len(whole)}, dtype_tolerances {len(tol_only)}, whole project bar {len(project)}")
    assert all(rec[m][1] for m in fr.HOT_MUTANTS)
    # scale slips and the lse offset pass the project's bar on cases where the sharp bar fails them (profiles/hot_sweep.md has the counts;
    # delta over half of d is outside dtype_tolerances on this table's shapes: |o| reaches 0.3 and the half-row constant moves dq by 0.054)
    for m in ("o_times_1.02", "dq_times_1.1", "lse_plus_2e-4", "pv_block_rescaled_twice"):
        assert set(rec[m][1]) - set(rec[m][4]), m


def test_the_kernel_in_the_baselines_place_passes_both_bars():
    """the other direction: a result with the model's rounding points and nothing else — the baseline of another model of the
    same route family — is inside the sharp bar of the case's own model, whole and per band"""
    for key in (((3, 513, 513), 128, "bf16", "causal", "default"), ((5, 130, 130), 64, "f16", "none", 0.37)):
        call, ref = refs(key)
        own = base(key, fr.Model(key_tile=128, lazy_rescale=True, exp2=True))
        other = fr.rounded(base(key, fr.Model(key_tile=64, lazy_rescale=False, exp2=True))._replace(
            dead_rows=ref.dead_rows, dead_keys=ref.dead_keys), call["dtype"])
        assert not fr.project_bar(other, ref, call["dtype"])
        assert not fr.sharp_bar(other, ref, own, call["dtype"])[0]
        if call["causal"]:
            assert not fr.banded_sharp_bar(other, ref, own, call["dtype"])[0]


def test_band_edges():
    assert fr.band_edges(1100, 1100) == ([(0, 64), (64, 256), (256, 1100)], [(0, 844), (844, 1036), (1036, 1100)])
    assert fr.band_edges(31, 31) == ([(0, 31)], [(0, 31)])
    assert fr.band_edges(130, 130) == ([(0, 64), (64, 130)], [(0, 66), (66, 130)])
    assert fr.band_edges(1, 513) == ([(0, 1)], [(0, 257), (257, 449), (449, 513)])
    assert list(itertools.chain(*fr.band_edges(512, 512)[0])) == [0, 64, 64, 256, 256, 512]
