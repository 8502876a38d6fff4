"""Forward-only timing of the featured fp8 prefill call (flash_attn_fp8_func / fa_fp8_forward_mod: a sliding window, a softcap, sinks;
DESIGN.md section 9zc) at tools/bench_fp8_inputs.py's shape (B = 1, H = 16, N = 16384, d = 128, causal), with that tool's method: the
variants interleaved in one process, HIP-event kernel times per call from the library's profiler, median and spread over the rounds,
tensors quantised once outside the timed region.
  window   a causal window of 1023 keys against the same call without a window (the parent kernel) and against the bf16 extended
           forward with the same window; the attention kernel's time beside the transposer's, which still transposes every key
  softcap, sinks   each on the unwindowed causal row, against the parent kernel on that row"""
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
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--window", type=int, default=1023)
args = ap.parse_args()
D, CALLS = 128, 10
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


b, h, n, w = 1, 16, args.n, args.window
g = torch.Generator(device="cuda").manual_seed(0)
q, k, v = (torch.randn((b, h, n, D), device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
(q8, qd), (k8, kd), (v8, vd) = quantise(q), quantise(k), quantise(v)
q3, k3, v3 = (t.reshape(b * h, n, D) for t in (q, k, v))
sinks = torch.randn((h,), dtype=torch.float32, device="cuda", generator=g)
fp8 = lambda **kw: ext.fp8_forward(q8, k8, v8, True, D ** -0.5, qd, kd, vd, **kw)   # noqa: E731
res = interleave({
    "fp8_causal": fp8,
    f"fp8_causal_window_{w}": lambda: fp8(window=(w, -1)),
    f"bf16_ex_causal_window_{w}": lambda: ext.ex_forward(q3, k3, v3, True, D ** -0.5, window=(w, -1)),
    "fp8_causal_softcap_30": lambda: fp8(softcap=30.0),
    "fp8_causal_sinks": lambda: fp8(sinks=sinks),
})
pairs_full = n * (n + 1) // 2
pairs_win = sum(min(i, w) + 1 for i in range(n))
for name, x in res.items():
    x["tflops"] = 4.0 * b * h * (pairs_win if "window" in name else pairs_full) * D / x["median_ms"] / 1e9
print(json.dumps({"config": f"B={b} H={h} N={n} d={D} causal, median of {args.rounds} interleaved rounds x {CALLS} calls", "results": res},
                 indent=1))
