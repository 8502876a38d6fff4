"""Forward-only timing of the fp8 calls at head dims 64, 128 and 256 (fp8_attn_func / fa_fp8_forward_hdim, fp8_attn_with_kvcache /
fa_fp8_forward_kvcache_hdim) with tools/bench_fp8_mod.py's method: the variants interleaved in one process,
HIP-event kernel times per call from the library's profiler, median and spread over the rounds, tensors quantised once outside the
timed region (the decode rows: HIP events around 50 back-to-back eager calls).
  prefill  B = 1, H = 16, N = 16384 (the d = 128 profile's shape), causal and not: the e4m3 call against the 16-bit call
           (flash_attention_ex's kernels through ex_forward) at the same shape, per head dim
  decode   B = 32, H_q = 32, H_kv = 8, one token over 8192 cached keys: the e4m3 call against flash_attn_with_kvcache's widening
           kernel (a bf16 q) on the same e4m3 cache, per head dim
  d = 128  the same call through the older entry point and through the _hdim one, side by side: the same kernels, so their
           difference is the run-to-run noise of the method"""
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
ap.add_argument("--cache-len", type=int, default=8192)
ap.add_argument("--head-dim", type=int, nargs="*", default=[64, 128, 256])
args = ap.parse_args()
CALLS = 10
E4M3 = torch.float8_e4m3fn


def quantise(x, dims):
    """16-bit x -> (e4m3 codes, float32 descale = absmax / 448 over dims)"""
    descale = (x.float().abs().amax(dim=dims, keepdim=True) / 448.0).clamp_min(1e-12)
    return (x.float() / descale).clamp(-448.0, 448.0).to(E4M3), descale.reshape([s for i, s in enumerate(descale.shape) if i not in dims])


def timed(fn):
    ext.profile_enable(True)
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    prof = ext.profile_report()
    ext.profile_enable(False)
    return sum(ms for _c, ms in prof.values()) / CALLS, {kn: ms / CALLS for kn, (_c, ms) in prof.items()}


def timed_events(fn, calls=50):
    """the decode calls: two events around `calls` back-to-back eager calls (the 16-bit decode kernels have no profile scope)"""
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / calls, {}


def interleave(variants, timed=timed):
    """{name: median / min / max ms and the kernels of the last round} over args.rounds rounds after one warm-up round"""
    acc, kern = {n: [] for n in variants}, {}
    for rnd in range(args.rounds + 1):
        for name, fn in variants.items():
            tot, ks = timed(fn)
            if rnd:
                acc[name].append(tot)
                kern[name] = ks
    return {n: dict(median_ms=statistics.median(a), min_ms=min(a), max_ms=max(a), kernels_ms=kern[n]) for n, a in acc.items()}


out = {}
g = torch.Generator(device="cuda").manual_seed(0)
for d in args.head_dim:
    b, h, n = 1, 16, args.n
    q, k, v = (torch.randn((b, h, n, d), device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    (q8, qd), (k8, kd), (v8, vd) = (quantise(t, (2, 3)) for t in (q, k, v))
    q3, k3, v3 = (t.reshape(b * h, n, d) for t in (q, k, v))
    variants = {}
    for causal in (True, False):
        tag = "causal" if causal else "full"
        variants[f"fp8_{tag}"] = lambda c=causal: ext.fp8_forward(q8, k8, v8, c, d ** -0.5, qd, kd, vd, hdim=True)
        variants[f"bf16_{tag}"] = lambda c=causal: ext.ex_forward(q3, k3, v3, c, d ** -0.5)
        if d == 128:
            variants[f"fp8_{tag}_older_entry"] = lambda c=causal: ext.fp8_forward(q8, k8, v8, c, d ** -0.5, qd, kd, vd)
    res = interleave(variants)
    for name, x in res.items():
        pairs = n * (n + 1) // 2 if "causal" in name else n * n
        x["tflops"] = 4.0 * b * h * pairs * d / x["median_ms"] / 1e9
    out[f"prefill d={d} B={b} H={h} N={n}"] = res
    print(json.dumps({f"prefill d={d}": res}), flush=True)
    del q, k, v, q8, k8, v8, q3, k3, v3

    from common.attention_ex import flash_attn_with_kvcache  # noqa: E402

    nb, hq, hkv, cap = 32, 32, 8, args.cache_len
    qn = torch.randn((nb, 1, hq, d), device="cuda", dtype=torch.bfloat16, generator=g)
    kc, vc = (torch.randn((nb, cap, hkv, d), device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    qn8, qnd = quantise(qn.reshape(nb, 1, hkv, hq // hkv, d), (1, 3, 4))
    qn8 = qn8.reshape(nb, 1, hq, d)
    (kc8, kcd), (vc8, vcd) = (quantise(t, (1, 3)) for t in (kc, vc))
    lens = torch.full((nb,), cap, dtype=torch.int32, device="cuda")
    variants = {
        "fp8_decode": lambda: ext.fp8_kvcache_forward(qn8, kc8, vc8, lens, None, None, qnd, kcd, vcd, d ** -0.5, True, 0, hdim=True),
        "bf16_q_on_e4m3_cache": lambda: flash_attn_with_kvcache(qn, kc8, vc8, cache_seqlens=lens, k_descale=kcd, v_descale=vcd, causal=True),
    }
    if d == 128:
        variants["fp8_decode_older_entry"] = lambda: ext.fp8_kvcache_forward(qn8, kc8, vc8, lens, None, None, qnd, kcd, vcd, d ** -0.5, True, 0)
    res = interleave(variants, timed_events)
    for x in res.values():
        x["cache_gb_s"] = 2.0 * nb * cap * hkv * d / x["median_ms"] / 1e6
    out[f"decode d={d} B={nb} H_q={hq} H_kv={hkv} L={cap}"] = res
    print(json.dumps({f"decode d={d}": res}), flush=True)
    del qn, kc, vc, kc8, vc8
print(json.dumps({"method": f"median of {args.rounds} interleaved rounds x {CALLS} calls, HIP-event kernel times", "results": out}, indent=1))
