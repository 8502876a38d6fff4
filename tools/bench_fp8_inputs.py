"""Forward-only timing of the fp8-inputs call (flash_attention_fp8 / fa_fp8_forward) at tools/bench_fp8.py's
shape (B = 1, H = 16, N = 16384, d = 128, causal and not), interleaved in one process with the bf16 forward and with
fa3_forward(fp8 = 1) on the same 16-bit data; the new call runs on tensors quantised ONCE outside the timed region (one absmax descale
per (batch, K/V head)).  HIP-event kernel times per call from the library's profiler, median and spread over the rounds.  Further
rows: GQA (H_q = 32, H_kv = 8, N = 8192), chunked prefill (Nq = 2048, Nk = 16384, causal) against the bf16 extended forward, and the
V transposer's time over its byte floor (2 * units * Nk * 128 bytes at the 8 TB/s HBM peak).
`--accuracy`: max |o - fp64| over the sweep of tests/fp8_inputs_cases.py, rows seeing < 256 keys and the rest, beside the 16-bit
extended forward on the dequantised tensors, and the kernel / baseline error ratio of every case."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-pytorch_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import flashattention_lab_cuda as ext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--accuracy", action="store_true")
args = ap.parse_args()
D, CALLS, HBM_PEAK = 128, 10, 8.0e12
E4M3 = torch.float8_e4m3fn


def quantise(x):
    """x (B, H, N, d) 16-bit -> (e4m3 codes, descale (B, H) float32 = absmax / 448)"""
    descale = (x.float().abs().amax(dim=(2, 3)) / 448.0).clamp_min(1e-12)
    return (x.float() / descale[:, :, None, None]).clamp(-448.0, 448.0).to(E4M3), descale


def timed(fn):
    ext.profile_enable(True)
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    prof = ext.profile_report()
    ext.profile_enable(False)
    return sum(ms for _c, ms in prof.values()) / CALLS, {kn: ms / CALLS for kn, (_c, ms) in prof.items()}


def interleave(variants):
    """{name: (median ms, min, max, kernels of the last round)} over args.rounds rounds after one warm-up round"""
    acc, kern = {n: [] for n in variants}, {}
    for rnd in range(args.rounds + 1):
        for name, fn in variants.items():
            tot, ks = timed(fn)
            if rnd:
                acc[name].append(tot)
                kern[name] = ks
    return {n: dict(median_ms=statistics.median(a), min_ms=min(a), max_ms=max(a), kernels_ms=kern[n]) for n, a in acc.items()}


def problem(b, hq, hkv, nq, nk, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn((b, hq, nq, D), device="cuda", dtype=torch.bfloat16, generator=g)
    k, v = (torch.randn((b, hkv, nk, D), device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    return q, k, v


def flops(b, hq, nq, nk, causal):
    pairs = nq * nk - (nq * (nq - 1) // 2 if causal else 0)
    return 4.0 * b * hq * pairs * D


def time_rows():
    res = {}
    b, h, n = 1, 16, 16384
    q, k, v = problem(b, h, h, n, n, 0)
    (q8, qd), (k8, kd), (v8, vd) = quantise(q), quantise(k), quantise(v)
    q3, k3, v3 = (t.reshape(b * h, n, D) for t in (q, k, v))
    for causal in (False, True):
        r = interleave({
            "bf16": lambda: ext.fa3_forward(q3, k3, v3, causal, D ** -0.5, 64, 128, 2, False),
            "fa3_fp8": lambda: ext.fa3_forward(q3, k3, v3, causal, D ** -0.5, 64, 128, 2, True),
            "fp8_inputs": lambda: ext.fp8_forward(q8, k8, v8, causal, D ** -0.5, qd, kd, vd),
        })
        fl = flops(b, h, n, n, causal)
        for name, x in r.items():
            x["tflops"] = fl / x["median_ms"] / 1e9
        old, new = r["fa3_fp8"], r["fp8_inputs"]
        r["expectation"] = dict(bound_ms=old["median_ms"] + (old["max_ms"] - old["min_ms"]), met=new["median_ms"] <= old["median_ms"] + (old["max_ms"] - old["min_ms"]))
        vt = new["kernels_ms"].get("fp8in_vt", 0.0)
        floor = 2.0 * b * h * n * D / HBM_PEAK * 1e3
        r["transposer"] = dict(ms=vt, byte_floor_ms=floor, over_floor=vt / floor if floor else None)
        res["causal" if causal else "full"] = r
    b, hq, hkv, n = 1, 32, 8, 8192
    q, k, v = problem(b, hq, hkv, n, n, 1)
    (q8, qd), (k8, kd), (v8, vd) = quantise(q), quantise(k), quantise(v)
    qd = qd.reshape(b, hkv, hq // hkv).amax(-1)                     # one q descale per K/V head
    q8 = (q.float() / qd.repeat_interleave(hq // hkv, dim=1)[:, :, None, None]).clamp(-448.0, 448.0).to(E4M3)
    for causal in (False, True):
        r = interleave({
            "bf16_ex": lambda: ext.ex_forward(q.reshape(b * hq, n, D), k.reshape(b * hkv, n, D), v.reshape(b * hkv, n, D), causal, D ** -0.5),
            "fp8_inputs": lambda: ext.fp8_forward(q8, k8, v8, causal, D ** -0.5, qd, kd, vd),
        })
        for x in r.values():
            x["tflops"] = flops(b, hq, n, n, causal) / x["median_ms"] / 1e9
        res[f"gqa_32_8_n8192_{'causal' if causal else 'full'}"] = r
    b, h, nq, nk = 1, 16, 2048, 16384
    q, k, v = problem(b, h, h, nq, nk, 2)
    (q8, qd), (k8, kd), (v8, vd) = quantise(q), quantise(k), quantise(v)
    r = interleave({
        "bf16_ex": lambda: ext.ex_forward(q.reshape(b * h, nq, D), k.reshape(b * h, nk, D), v.reshape(b * h, nk, D), True, D ** -0.5),
        "fp8_inputs": lambda: ext.fp8_forward(q8, k8, v8, True, D ** -0.5, qd, kd, vd),
    })
    for x in r.values():
        x["tflops"] = flops(b, h, nq, nk, True) / x["median_ms"] / 1e9
    res["chunked_prefill_2048_16384_causal"] = r
    return res


def accuracy_rows():
    from tests import fp8_inputs_cases as fc
    from tests import fp8_inputs_ref as fr
    from tests.fp8_ref import tiled_sharp_bar

    worst = {"fp8_short": 0.0, "fp8_rest": 0.0, "bit16_short": 0.0, "bit16_rest": 0.0}
    ratios = {}
    for i, c in enumerate(fc.CASES):
        call = fc.build_call(c, i)
        ref, base = fr.reference(call), fr.baseline(call)
        q, k, v = (call[n].view(E4M3).cuda() for n in ("q8", "k8", "v8"))
        ds = [None if call[n] is None else call[n].cuda() for n in ("q_descale", "k_descale", "v_descale")]
        o, lse = ext.fp8_forward(q, k, v, call["causal"], call["scale"], *ds, call["dtype"])
        got = fr._result(o.reshape(-1, call["nq"], D).cpu(), lse.reshape(-1, call["nq"]).cpu())
        ratios[fc.case_id(c, i)] = {k_: round(v_, 3) for k_, v_ in tiled_sharp_bar(got, ref, base, call["dtype"])[1].items()}
        qd, kd, vd = (t.to(call["dtype"]).cuda() for t in fr.dequantised(call))
        o16, _ = ext.ex_forward(qd, kd, vd, call["causal"], call["scale"])
        seen = fr.visible(call).sum(-1)
        short = (seen < 256) & (seen > 0)
        for name, out in (("fp8", got.o), ("bit16", o16.cpu())):
            err = (out.double() - ref.o).abs().amax(dim=(0, 2))
            if short.any():
                worst[name + "_short"] = max(worst[name + "_short"], float(err[short].max()))
            if (~short).any():
                worst[name + "_rest"] = max(worst[name + "_rest"], float(err[~short].max()))
    return {"max_abs_err_vs_fp64": worst, "kernel_over_baseline": ratios}


out = accuracy_rows() if args.accuracy else time_rows()
print(json.dumps({"config": f"d={D}, median of {args.rounds} interleaved rounds x {CALLS} calls" if not args.accuracy else "sweep of tests/fp8_inputs_cases.py",
                  "results": out}, indent=1))
