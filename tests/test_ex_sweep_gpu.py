"""GPU: the all-pairs sweep of the extended forward and backward (ex_forward / ex_backward, ex_varlen_forward / ex_varlen_backward).
One test per case of tests/ex_sweep_cases.py: the inputs are built on the CPU from the case's seed, the raw entry points run forward
then backward under the case's ex_path, and the results are held to tests/ex_full_ref.py twice:

  * the project's bar, unchanged (ex_full_ref.project_bar): o, dq, dk, dv, dsinks within tests.helpers.dtype_tolerances of fp64, finite
    lse at rtol = atol = 1e-3 (which is also "lse = the sink" on sink-only rows), the -inf pattern exact, nothing NaN, o = dq = 0 on
    rows without a visible key and dk = dv = 0 on keys no row sees, exactly; tokens no sequence owns are not compared;
  * the sharp bar (ex_full_ref.sharp_bar), per tensor in the max norm: max |kernel - fp64| <= 2 * max |baseline - fp64| +
    eps(dtype) * max |fp64| (float32's eps for lse), the baseline being the same function with a flash kernel's rounding points.
    Factor 2: what a correct kernel adds to those points is of their own size; the bugs the sweep is after are off by a large
    fraction of the output.  A kernel outside the bar has a rounding point the baseline lacks — it is then added there, with its
    file and function — or a bug; the factor is not raised.  The ratio kernel error / baseline error is printed per case and
    tensor ("ex_sweep_ratio ..."); profiles/ex_sweep.md records the largest, and how close the float32 cases run to the bar.

A case the table calls legal and the library refuses fails here: the rule in ex_sweep_cases.pair_legal is then wrong.

The packed cases under ex_path 3 without dropout are also compared bit for bit with the padded call on each sequence alone — DESIGN.md
§9d: "each sequence of a varlen call is bit-identical to the same sequence run alone through fa_ex_*_window (ex_path 3, no dropout: the
tests check o, lse, dq, dk and dv)", read with the wider entry points that came after it (softcap, ALiBi, sinks, a gradient of lse,
a v of its own width: each sequence takes its own row of (B, H_q) slopes and its own columns of dlse).  Left out, because the design
does not promise them: ex_path 1 (the exact-f32 kernels), dropout (the padded call on one sequence has other counters), dsinks (one
sum over all sequences) and a sequence without keys (the padded call launches nothing)."""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import ex_full_ref as fr
from tests import ex_sweep_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [sc.case_id(i) for i in range(len(sc.CASES))]


@functools.lru_cache(maxsize=None)
def case_and_references(i):
    """(call, fp64 reference, baseline, dlse with NaN where the reference's lse is -inf), computed once and never changed"""
    call = sc.build_inputs(i)
    ref, base = fr.full_reference(call), fr.baseline(call)
    dlse = None
    if call["dlse"] is not None:
        dlse = torch.where(ref.lse == fr.NEG_INF, torch.full_like(call["dlse"], float("nan")), call["dlse"])
    return call, ref, base, dlse


def family(c):
    """the kernel family launch_ex routes case c to (csrc/fa_ex.hip), for the record of error ratios"""
    (d, dv), packed = c["widths"], c["layout"] != "padded"
    if d != dv:
        return "vdim"
    mfma = c["dtype"] != "f32" and d <= 128 and d % 8 == 0
    bare = (c["mask"] in ("none", "causal") and c["dense"] == "none" and c["dropout"] == 0.0 and c["mods"] == "none" and not c["sinks"]
            and not c["dlse"])
    if c["path"] == "auto" and not packed and bare:
        if mfma and (c["lengths"][0] == c["lengths"][1] or d == 128):
            return "plain"
        if not mfma and c["lengths"][0] == c["lengths"][1] and c["heads"][0] == c["heads"][1]:
            return "generic"
    kind = "mfma" if mfma and c["path"] != "exact" else "exact"
    return kind + ("_varlen" if packed else "")


def dev(t):
    return None if t is None else t.to(DEV)


def run_padded(call, q, k, v, do, dlse, slopes):
    """(o, lse, dq, dk, dv, dsinks) of ex_forward + ex_backward on device tensors, under the call's ex_path"""
    import flashattention_lab_cuda as ext

    kw = dict(mask=dev(call["mask"]), block_mask=dev(call["block_mask"]), br=call["br"], bc=call["bc"], dropout_p=call["dropout_p"],
              seed=call["seed"], window=call["window"], softcap=call["softcap"], alibi_slopes=slopes)
    sinks = dev(call["sinks"])
    ext.set_option("ex_path", call["path"])
    try:
        o, lse = ext.ex_forward(q, k, v, call["causal"], call["scale"], sinks=sinks, **kw)
        grads = ext.ex_backward(q, k, v, o, do, lse, call["causal"], call["scale"], dlse=dlse, sinks=sinks, **kw)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return (o, lse) + tuple(grads) + ((None,) if sinks is None else ())


def run_case(call, dlse):
    import flashattention_lab_cuda as ext

    if call["layout"] == "padded":
        slopes = call["alibi_slopes"]
        if slopes is not None:      # (H_q,) travels as the (B, H_q) view of the vector
            slopes = slopes[0].contiguous().to(DEV).view(1, -1).expand(slopes.shape[0], -1) if slopes.stride(0) == 0 else slopes.to(DEV)
        return run_padded(call, dev(call["q"]), dev(call["k"]), dev(call["v"]), dev(call["do"]), dev(dlse), slopes)
    if call["layout"] == "packed_strided":
        qkv = call["qkv"].to(DEV)
        hkv = call["heads"][1]
        q, k = qkv[:, 0], qkv[:, 1, :hkv]
        v = qkv[:, 2, :hkv] if call["v"].shape[2] == call["q"].shape[2] else call["v"].to(DEV)
        assert q.stride(0) == 3 * q.shape[1] * q.shape[2] and k.stride(0) == q.stride(0)
    else:
        q, k, v = dev(call["q"]), dev(call["k"]), dev(call["v"])
    cu_q, cu_k = dev(call["cu_seqlens_q"]), dev(call["cu_seqlens_k"])
    args = (cu_q, cu_k, call["max_seqlen_q"], call["max_seqlen_k"], call["causal"], call["scale"])
    kw = dict(dropout_p=call["dropout_p"], seed=call["seed"], window=call["window"], softcap=call["softcap"],
              alibi_slopes=dev(call["alibi_slopes"]))
    sinks = dev(call["sinks"])
    ext.set_option("ex_path", call["path"])
    try:
        o, lse = ext.ex_varlen_forward(q, k, v, *args, sinks=sinks, **kw)
        grads = ext.ex_varlen_backward(q, k, v, o, dev(call["do"]), lse, *args, dlse=dev(dlse), sinks=sinks, **kw)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return (o, lse) + tuple(grads) + ((None,) if sinks is None else ())


def as_result(out):
    return SimpleNamespace(**{n: (None if t is None else t.cpu()) for n, t in zip(fr.TENSORS, out)})


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_case(i):
    call, ref, base, dlse = case_and_references(i)
    got = as_result(run_case(call, dlse))
    dtype = call["dtype"]
    # shapes and dtypes as documented
    for name in ("o", "dq", "dk", "dv"):
        t = getattr(got, name)
        assert t.shape == getattr(ref, name).shape and t.dtype == dtype, name
    assert got.lse.shape == ref.lse.shape and got.lse.dtype == torch.float32
    if call["sinks"] is None:
        assert got.dsinks is None
    else:
        assert got.dsinks.shape == call["sinks"].shape and got.dsinks.dtype == torch.float32
    errs = fr.errors(got, ref)
    print(f"ex_sweep_error {IDS[i]} " + " ".join(f"{n}={e:.3e}" for n, (e, _big) in errs.items()))
    project = fr.project_bar(got, ref, dtype)
    sharp, ratio = fr.sharp_bar(got, ref, base, dtype)
    print(f"ex_sweep_ratio {IDS[i]} family={family(sc.CASES[i])} " + " ".join(f"{n}={r:.3f}" for n, r in ratio.items()))
    assert not project, f"{IDS[i]}: the project's bar: {project}"
    assert not sharp, f"{IDS[i]}: the sharp bar: {sharp}"


BITWISE = [i for i, c in enumerate(sc.CASES) if c["layout"] != "padded" and c["path"] == "mfma_only" and c["dropout"] == 0.0]


@pytest.mark.parametrize("i", BITWISE, ids=[IDS[i] for i in BITWISE])
def test_packed_call_is_bitwise_the_padded_call_on_each_sequence(i):
    call, _ref, _base, dlse = case_and_references(i)
    o, lse, dq, dk, dv, _ds = run_case(call, dlse)
    cu_q, cu_k = call["cu_seqlens_q"].tolist(), call["cu_seqlens_k"].tolist()
    slopes = call["alibi_slopes"]
    compared = 0
    for b in range(sc.SEQS):
        (q0, q1), (k0, k1) = cu_q[b:b + 2], cu_k[b:b + 2]
        if q1 == q0 or k1 == k0:
            continue
        one = dict(call, layout="padded")
        qb, kb, vb, dob = (dev(t).transpose(0, 1).contiguous() for t in (call["q"][q0:q1], call["k"][k0:k1], call["v"][k0:k1], call["do"][q0:q1]))
        dlb = None if dlse is None else dlse[:, q0:q1].contiguous().to(DEV)
        slb = None if slopes is None else (slopes[b] if slopes.dim() == 2 else slopes).contiguous().to(DEV)
        ob, lb, dqb, dkb, dvb, _ = run_padded(one, qb, kb, vb, dob, dlb, slb)
        assert torch.equal(o[q0:q1], ob.transpose(0, 1)) and torch.equal(lse[:, q0:q1], lb), (IDS[i], b, "o / lse")
        assert torch.equal(dq[q0:q1], dqb.transpose(0, 1)), (IDS[i], b, "dq")
        assert torch.equal(dk[k0:k1], dkb.transpose(0, 1)) and torch.equal(dv[k0:k1], dvb.transpose(0, 1)), (IDS[i], b, "dk / dv")
        compared += 1
    assert compared >= 1


def test_the_bitwise_extras_are_not_empty():
    assert len(BITWISE) >= 6
