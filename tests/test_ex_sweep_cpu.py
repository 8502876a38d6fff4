"""CPU: the extended forward / backward sweep without a GPU — the case table (tests/ex_sweep_cases.py) is deterministic, legal, covers
every allowed pair and stays within its cap; the whole-call reference (tests/ex_full_ref.py) agrees to fp64 round-off with each
single-feature reference the project has and with its own closed-form backward; every case has a row that sees a key and nothing
NaN, and the table as a whole has dead rows, dead keys and sink-only rows; and the two bars of the sweep are measured against nine
mutants of the reference — every one must fail the sharp bar on at least one case, and the number that tests.helpers.dtype_tolerances
alone would have caught is printed (profiles/ex_sweep.md has the figures)."""
import functools

import pytest
import torch

from oracle import attention_oracle as orc
from tests import ex_full_ref as fr
from tests import ex_sweep_cases as sc
from tests import merge_ref
from tests import sink_ref as sr
from tests.vdim_ref import vdim_reference

TIGHT = dict(rtol=1e-12, atol=1e-12)
IDS = [sc.case_id(i) for i in range(len(sc.CASES))]


# ---- the table

def test_table_is_deterministic_and_within_its_cap():
    assert sc.generate() == sc.CASES
    assert 0 < len(sc.CASES) <= sc.MAX_CASES <= 120
    assert len(set(IDS)) == len(IDS)


def test_every_allowed_pair_is_covered_and_every_value_appears():
    covered = set()
    for c in sc.CASES:
        assert sc.case_legal(c)
        covered |= sc.pairs_of(c)
    assert sc.all_pairs() <= covered
    for (a, va), (b, vb) in covered:
        assert sc.pair_legal(a, va, b, vb)
    for n in sc.NAMES:
        assert {c[n] for c in sc.CASES} == set(sc.AXES[n]), n


def test_the_rules_leave_out_what_the_issue_names():
    legal = sc.pair_legal
    assert not legal("path", "mfma_only", "dtype", "f32") and not legal("path", "mfma_only", "widths", (136, 136))
    assert not legal("path", "mfma_only", "widths", (20, 20)) and legal("path", "mfma_only", "widths", (192, 128))
    assert not legal("dtype", "f32", "widths", (72, 40))
    for axis, v in (("dense", "mask"), ("dense", "block64"), ("dropout", 0.1), ("mask", "causal+window0"), ("mask", "window30_10"),
                    ("mods", "softcap"), ("mods", "alibi"), ("sinks", True)):
        assert not legal("widths", (64, 32), axis, v), (axis, v)
    assert legal("widths", (64, 32), "mask", "causal") and legal("widths", (64, 32), "dlse", True)
    for layout in ("packed", "packed_qk", "packed_strided"):
        assert not legal("layout", layout, "dense", "mask") and not legal("layout", layout, "dense", "block32")
        assert legal("layout", layout, "widths", (192, 128))


def test_packed_lengths_hold_what_they_promise():
    for lens in sc.PACKED:
        assert len(lens) == sc.SEQS and 0 in lens and 1 in lens and any(n > 128 and n % 32 for n in lens)
    for lq, lk in sc.PACKED_QK:
        assert len(lq) == len(lk) == sc.SEQS and 0 in lq and 1 in lq
        assert any(a > b > 0 for a, b in zip(lq, lk)) and any(a > 0 and b == 0 for a, b in zip(lq, lk))
        assert any(n > 128 and n % 32 for n in lq + lk)


# ---- the reference on every case

@functools.lru_cache(maxsize=None)
def case_refs(i):
    call = sc.build_inputs(i)
    return call, fr.full_reference(call), fr.baseline(call)


def owned(name, t, ref):
    return fr._owned(name, t, ref)


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_reference_of_the_case(i):
    """nothing NaN, a row that sees a key, the shapes of the raw entry points; the closed-form backward in fp64 without rounding is
    the autograd reference; the reference passes both bars against itself"""
    c = sc.CASES[i]
    call, ref, base = case_refs(i)
    hq, hkv = c["heads"]
    d, dv = c["widths"]
    assert call["q"].shape[-1] == d and call["v"].shape[-1] == dv and call["q"].dtype == sc.DTYPES[c["dtype"]]
    assert ref.o.shape == call["q"].shape[:2] + (dv,) and ref.dq.shape == call["q"].shape and ref.dk.shape == call["k"].shape
    assert ref.dv.shape == call["v"].shape and (ref.dsinks is None) == (not c["sinks"])
    if c["layout"] == "padded":
        assert call["q"].shape[0] == sc.B * hq and call["k"].shape[0] == sc.B * hkv and ref.lse.shape == call["q"].shape[:2]
    else:
        assert call["q"].shape[1] == hq and call["k"].shape[1] == hkv and ref.lse.shape == (hq, call["q"].shape[0])
        assert int(ref.unowned_q.sum()) == 2 and int(ref.unowned_k.sum()) == 2 and torch.isnan(ref.lse[:, ref.unowned_q]).all()
        if c["layout"] == "packed_strided":
            assert call["q"].stride(0) == 3 * hq * d and call["k"].stride(0) == 3 * hq * d and call["k"].stride(1) == d
    for name in fr.TENSORS:
        t = getattr(ref, name)
        if t is not None:
            assert not torch.isnan(owned(name, t, ref)).any(), name
    assert bool(torch.isfinite(owned("lse", ref.lse, ref)).any()) and not bool(owned("lse", ref.dead_rows, ref).all())
    exact = fr.baseline(call, compute=torch.float64, tensor_dtype=None)
    for name in fr.TENSORS:
        t = getattr(ref, name)
        if t is None:
            continue
        a, b = owned(name, getattr(exact, name), ref), owned(name, t, ref)
        if name == "lse":
            assert torch.equal(torch.isfinite(a), torch.isfinite(b))
            a, b = a[torch.isfinite(b)], b[torch.isfinite(b)]
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10, msg=lambda m, n=name: f"closed form {n}: {m}")
    dtype = call["dtype"]
    assert fr.project_bar(fr.rounded(ref, dtype), ref, dtype) == []
    assert fr.sharp_bar(fr.rounded(ref, dtype), ref, base, dtype)[0] == []
    shaped = ref._replace(o=base.o, lse=base.lse, dq=base.dq, dk=base.dk, dv=base.dv, dsinks=base.dsinks)
    miss = fr.project_bar(fr.rounded(shaped, dtype), ref, dtype)
    if miss:      # (a measure, not a bar: where the rounding points of a 16-bit kernel alone spend the project's 5e-2)
        print(f"baseline outside the project's bar {IDS[i]}: {miss}")
    assert not [m for m in miss if "outside" not in m], miss       # NaN, the -inf pattern and the exact zeros hold for it too


def test_the_table_has_dead_rows_dead_keys_and_sink_only_rows():
    rows = keys = sink_only = 0
    for i in range(len(sc.CASES)):
        _call, ref, _base = case_refs(i)
        rows += bool(ref.dead_rows.any())
        keys += bool(ref.dead_keys.any())
        sink_only += bool(ref.sink_rows.any())
    print(f"cases with dead rows {rows}, with dead keys {keys}, with sink-only rows {sink_only}")
    assert rows >= 3 and keys >= 3 and sink_only >= 3


# ---- the reference against the single-feature references

def close(a, b, what):
    torch.testing.assert_close(a, b, **TIGHT, msg=lambda m: f"{what}: {m}")


def close_lse(a, b, what):
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), what
    close(a[fin], b[fin].double(), what)


def variants(pred, change, limit):
    """(index, case) of up to `limit` table cases that pass pred, with the axes in `change` replaced, where that is legal"""
    out = []
    for i, c in enumerate(sc.CASES):
        v = dict(c, **change)
        if pred(v) and sc.case_legal(v):
            out.append((i, v))
    return out[:limit]


def test_against_the_extended_oracle():
    """padded, no GQA, masks and dropout only: oracle.attention_oracle.extended_attention_backward"""
    picked = variants(lambda c: c["layout"] == "padded" and c["widths"][0] == c["widths"][1] and c["mask"] in ("none", "causal"),
                      dict(heads=(4, 4), mods="none", sinks=False, dlse=False), 12)
    assert len(picked) >= 8 and {c["dense"] for _i, c in picked} >= {"mask", "mask_bh", "block32", "block64"}
    for i, c in picked:
        call = sc.build_inputs(i, c)
        ref = fr.full_reference(call)
        dq, dk, dv, o, lse = orc.extended_attention_backward(call["q"].double(), call["k"].double(), call["v"].double(), call["do"].double(),
                                                             causal=call["causal"], softmax_scale=call["scale"], mask=call["mask"],
                                                             block_mask=call["block_mask"], br=call["br"], bc=call["bc"],
                                                             dropout_p=call["dropout_p"], seed=call["seed"])
        for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            close(getattr(ref, name), torch.nan_to_num(t, nan=0.0) if name == "o" else t, f"{sc.case_id(i)} {name}")
        fin = torch.isfinite(ref.lse)
        assert torch.equal(torch.isfinite(lse), fin)
        torch.testing.assert_close(ref.lse[fin].float(), lse[fin], rtol=1e-6, atol=1e-6)      # (the oracle returns lse in float32)


def test_against_the_sink_reference_and_its_dlse_form():
    """padded, v as wide as q: sink_ref.sink_reference (GQA, window, masks, dropout, softcap, ALiBi, sinks) and, with a gradient of
    lse, merge_ref.attention_grads"""
    picked = variants(lambda c: c["layout"] == "padded" and c["widths"][0] == c["widths"][1], {}, 200)
    assert len(picked) >= 30
    for i, c in picked:
        call, ref, _base = case_refs(i)
        kw = dict(softcap=call["softcap"], slopes=None if call["alibi_slopes"] is None else call["alibi_slopes"].reshape(-1),
                  window=call["window"], mask=call["mask"], block_mask=call["block_mask"], br=call["br"], bc=call["bc"],
                  dropout_p=call["dropout_p"], seed=call["seed"])
        if call["dlse"] is None:
            o, lse, dq, dk, dv, ds = sr.sink_reference(call["q"], call["k"], call["v"], call["do"], call["sinks"], call["causal"], call["scale"], **kw)
        else:
            o, lse, dq, dk, dv, ds = merge_ref.attention_grads(call["q"], call["k"], call["v"], call["do"], call["dlse"], call["sinks"],
                                                               call["causal"], call["scale"], **kw)
        for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            close(getattr(ref, name), t, f"{IDS[i]} {name}")
        if call["dlse"] is None:
            fin = torch.isfinite(ref.lse)
            assert torch.equal(torch.isfinite(lse), fin)
            torch.testing.assert_close(ref.lse[fin].float(), lse[fin], rtol=1e-6, atol=1e-6)  # (sink_reference returns lse in float32)
        else:
            close_lse(ref.lse, lse, f"{IDS[i]} lse")
        if ds is not None:
            close(ref.dsinks, ds, f"{IDS[i]} dsinks")


def test_against_the_vdim_reference():
    """the two-width cases, padded one batch element at a time and packed one sequence at a time: vdim_ref.vdim_reference"""
    n = 0
    for i, c in enumerate(sc.CASES):
        if c["widths"][0] == c["widths"][1]:
            continue
        call, ref, _base = case_refs(i)
        hq, hkv = c["heads"]
        if c["layout"] == "padded":
            spans = [((slice(b * hq, (b + 1) * hq), slice(b * hkv, (b + 1) * hkv)), lambda t: t, lambda t: t) for b in range(sc.B)]
        else:
            cu_q, cu_k = call["cu_seqlens_q"].tolist(), call["cu_seqlens_k"].tolist()
            spans = [((slice(cu_q[b], cu_q[b + 1]), slice(cu_k[b], cu_k[b + 1])), lambda t: t.transpose(0, 1), lambda t: t.transpose(0, 1))
                     for b in range(sc.SEQS) if cu_q[b + 1] > cu_q[b]]
        for (sq, sk), tin, _tout in spans:
            dl = None
            if call["dlse"] is not None:
                dl = call["dlse"][sq] if c["layout"] == "padded" else call["dlse"][:, sq]
            o, lse, (dq, dk, dv) = vdim_reference(tin(call["q"][sq]), tin(call["k"][sk]), tin(call["v"][sk]), call["causal"], call["scale"],
                                                  tin(call["do"][sq]), dl)
            close(tin(ref.o[sq]), o, f"{IDS[i]} o")
            close_lse(ref.lse[sq] if c["layout"] == "padded" else ref.lse[:, sq], lse, f"{IDS[i]} lse")
            close(tin(ref.dq[sq]), dq, f"{IDS[i]} dq")
            close(tin(ref.dk[sk]), dk, f"{IDS[i]} dk")
            close(tin(ref.dv[sk]), dv, f"{IDS[i]} dv")
        n += 1
    assert n >= 6


def test_against_the_varlen_helper_of_the_sink_tests():
    """packed with cu_q == cu_k, causal / window / GQA / sinks only: tests.test_sinks_gpu._varlen_reference on the owned tokens"""
    from tests.test_sinks_gpu import _varlen_reference

    picked = variants(lambda c: c["layout"] in ("packed", "packed_strided") and c["widths"][0] == c["widths"][1],
                      dict(mods="none", dropout=0.0, dlse=False), 8)
    assert len(picked) >= 6 and any(c["sinks"] for _i, c in picked) and any(not c["sinks"] for _i, c in picked)
    for i, c in picked:
        call = sc.build_inputs(i, c)
        ref = fr.full_reference(call)
        lens, _ = sc.lengths_of(c)
        own = slice(1, -1)
        o, lse, dq, dk, dv, ds = _varlen_reference(call["q"][own], call["k"][own], call["v"][own], call["do"][own], call["sinks"], lens,
                                                   call["causal"], call["scale"], call["window"])
        for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            close(getattr(ref, name)[own], t, f"{sc.case_id(i)} {name}")
        rl = ref.lse[:, own]
        fin = torch.isfinite(rl)
        assert torch.equal(torch.isfinite(lse), fin)
        torch.testing.assert_close(rl[fin].float(), lse[fin], rtol=1e-6, atol=1e-6)           # (the helper returns lse in float32)
        if call["sinks"] is not None:
            close(ref.dsinks, ds, f"{sc.case_id(i)} dsinks")


# ---- discriminating power: mutants of the reference against the two bars

RELEVANT = {
    "window_left_off_by_one": lambda c: sc.window_of(c["mask"])[0] >= 0,
    "alibi_without_shift": lambda c: "alibi" in c["mods"],
    "sink_not_in_lse": lambda c: c["sinks"],
    "kv_head_modulo": lambda c: c["heads"] == (4, 2),
    "tail_keys_dropped": lambda c: True,
    "causal_top_left": lambda c: c["mask"].startswith("causal"),
    "dlse_ignored": lambda c: c["dlse"],
    "softcap_after_alibi": lambda c: c["mods"] == "alibi_b+softcap",
    "dropout_unscaled": lambda c: c["dropout"] > 0.0,
}


@functools.lru_cache(maxsize=None)
def mutant_record(mutant):
    """(cases tried, cases failing the sharp bar, cases failing dtype_tolerances alone, cases failing the project's whole bar)"""
    tried, sharp, tol_only, project = 0, [], [], []
    for i, c in enumerate(sc.CASES):
        if not RELEVANT[mutant](c):
            continue
        call, ref, base = case_refs(i)
        got = fr.rounded(fr.full_reference(call, mutant=mutant), call["dtype"])
        tried += 1
        if fr.sharp_bar(got, ref, base, call["dtype"])[0]:
            sharp.append(i)
        if fr.project_bar(got, ref, call["dtype"], only_tolerances=True):
            tol_only.append(i)
        if fr.project_bar(got, ref, call["dtype"]):
            project.append(i)
    return tried, sharp, tol_only, project


@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_the_sharp_bar_kills_the_mutant(mutant):
    tried, sharp, tol_only, project = mutant_record(mutant)
    print(f"mutant {mutant}: {tried} cases carry the feature; the sharp bar fails {len(sharp)}, dtype_tolerances alone {len(tol_only)}, "
          f"the project's whole bar (lse and exact zeros included) {len(project)}")
    assert tried >= 3 and sharp, f"{mutant} survives the sharp bar on all {tried} cases that carry its feature"


def test_count_the_mutants_each_bar_kills():
    rec = {m: mutant_record(m) for m in fr.MUTANTS}
    by_sharp = [m for m in fr.MUTANTS if rec[m][1]]
    by_tol = [m for m in fr.MUTANTS if rec[m][2]]
    by_project = [m for m in fr.MUTANTS if rec[m][3]]
    print(f"mutants killed: sharp bar {len(by_sharp)} / {len(fr.MUTANTS)}, dtype_tolerances alone {len(by_tol)} / {len(fr.MUTANTS)} "
          f"({', '.join(by_tol)}), the project's whole bar {len(by_project)} / {len(fr.MUTANTS)}")
    for m in fr.MUTANTS:
        tried, sharp, tol_only, project = rec[m]
        print(f"  {m}: cases {tried}, sharp {len(sharp)}, dtype_tolerances {len(tol_only)}, whole project bar {len(project)}")
    assert len(by_sharp) == len(fr.MUTANTS)
