#!/usr/bin/env python3
"""Time the fp8 quantiser (common.attention_ex.quantize_fp8, fa_fp8_quantize) against its byte floor and against the PyTorch
composition it replaces, and the chain 3 x quantise + flash_attention_fp8 against fa3_forward(fp8=1) and the bf16 forward.

    python tools/bench_fp8_quantize.py [--out profiles/fp8_quantize.md] [--skip-chain]

Rows (bf16): B H 16 x N 16384 x d 128 (DESIGN 9w's shape, g = 1, two-pass); the q slice of a packed (4096, 32 + 8 + 8, 128)
projection (g = 4, one sequence, read in place); the decode q (32, 1, 32, 128) with g = 4 (fused).  Per row, interleaved in one
process: the dynamic call, the static call, and the torch composition abs().amax / division / clamp / cast on the same tensor.
Byte floors at 6.3 TB/s: dynamic two-pass 2 reads of 2 B + 1 write of 1 B an element, fused and static 1 read + 1 write.
Times are HIP-event medians of groups of calls after warm-up.  Accuracy: max and RMS error of the chain against fp64 attention of
the original 16-bit tensors (a 512-row slice), beside fa3_forward(fp8=1)'s on the same inputs."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-pytorch_amd"))
import flashattention_lab_cuda as ext  # noqa: E402
from common.attention_ex import flash_attention_fp8, quantize_fp8, quantize_fp8_qkv  # noqa: E402

COPY_TBS = 6.3


def timed_interleaved(fns, warmup, iters, reps):
    """{name: median us} of the callables, their groups of `iters` calls interleaved rep by rep"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / iters * 1e3)
    return {k: statistics.median(v) for k, v in out.items()}


def torch_quantise(x, g):
    """(B, N, H, d) -> codes, descale (B, H / g) in PyTorch ops"""
    b, n, h, d = x.shape
    amax = x.abs().reshape(b, n, h // g, g * d).amax(dim=(1, 3)).float()
    ds = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    y = (x.float() * (1.0 / ds).repeat_interleave(g, dim=1)[:, None, :, None]).clamp(-448.0, 448.0)
    return y.to(torch.float8_e4m3fn), ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, dtype = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=gen, device=dev, dtype=torch.float32).to(dtype)   # noqa: E731
    lines = [f"# The fp8 quantiser: time, byte floor, the torch composition ({torch.cuda.get_device_name(0)})", "",
             f"`tools/bench_fp8_quantize.py`: bf16, HIP events, medians of {a.reps} interleaved groups of {a.iters} calls after {a.warmup} "
             f"warm-up calls; byte floors at {COPY_TBS} TB/s.", "",
             "| row | route | call us | floor us | call / floor | static us | torch ops us | call / torch |", "|---|---|---|---|---|---|---|---|"]
    proj = rnd(1, 4096, 48, 128)
    rows = [("B H 16 x N 16384 x d 128, g 1", rnd(1, 16384, 16, 128), 1), ("q of a packed (4096, 32 + 8 + 8, 128) projection, g 4", proj[:, :, :32], 4),
            ("decode q (32, 1, 32, 128), g 4", rnd(32, 1, 32, 128), 4)]
    for name, x, g in rows:
        before = [ext.route_count(r) for r in ("fp8_quant_fused", "fp8_quant_two_pass")]
        x8, ds = quantize_fp8(x, g)
        fused = ext.route_count("fp8_quant_fused") > before[0]
        ref8, refds = torch_quantise(x, g)
        # the composition is the same function up to how torch divides on the device: its dequantised values must agree closely
        err = (x8.float() * ds.repeat_interleave(g, dim=1)[:, None, :, None] - ref8.float() * refds.repeat_interleave(g, dim=1)[:, None, :, None]).abs().max()
        assert err.item() <= 2.0 ** -3 * x.float().abs().max().item(), (name, err.item())
        out, dso = torch.empty_like(x8), torch.empty_like(ds)
        t = timed_interleaved({"call": lambda: quantize_fp8(x, g, out=out, descale_out=dso),
                               "static": lambda: quantize_fp8(x, g, ds, out=out),
                               "torch": lambda: torch_quantise(x, g)}, a.warmup, a.iters, a.reps)
        floor = x.numel() * (3 if fused else 5) / (COPY_TBS * 1e6)
        lines.append(f"| {name} | {'fused' if fused else 'two-pass'} | {t['call']:.1f} | {floor:.1f} | {t['call'] / floor:.2f} | {t['static']:.1f} | "
                     f"{t['torch']:.1f} | {t['call'] / t['torch']:.3f} |")
    if not a.skip_chain:
        bh, n, d = 16, 16384, 128
        q, k, v = rnd(1, n, bh, d), rnd(1, n, bh, d), rnd(1, n, bh, d)
        q3, k3, v3 = (t[0].transpose(0, 1).contiguous() for t in (q, k, v))            # (BH, N, d) for the fa3 call
        scale = d ** -0.5

        def chain():
            q8, k8, v8, qd, kd, vd = quantize_fp8_qkv(q, k, v)
            return flash_attention_fp8(q8, k8, v8, q_descale=qd, k_descale=kd, v_descale=vd, layout="bnhd")

        t = timed_interleaved({"chain": chain, "fa3 fp8": lambda: ext.fa3_forward(q3, k3, v3, False, scale, 128, 128, 2, 1),
                               "bf16": lambda: ext.fa3_forward(q3, k3, v3, False, scale, 128, 128, 2, 0)}, a.warmup, max(1, a.iters // 2), a.reps)
        lines += ["", f"## End to end at B H {bh} x N {n} x d {d}, no mask", "", "| what | ms |", "|---|---|",
                  f"| 3 x quantize_fp8 + flash_attention_fp8 | {t['chain'] / 1e3:.3f} |", f"| fa3_forward(fp8=1) | {t['fa3 fp8'] / 1e3:.3f} |",
                  f"| fa3_forward(fp8=0), bf16 | {t['bf16'] / 1e3:.3f} |"]
        rows_ = 512
        ref = torch.softmax((q3[:, :rows_].double() @ k3.double().transpose(1, 2)) * scale, dim=-1) @ v3.double()
        o_chain = chain()[0].transpose(0, 1)[:, :rows_].double()
        o_fa3 = ext.fa3_forward(q3, k3, v3, False, scale, 128, 128, 2, 1)[0][:, :rows_].double()
        lines += ["", f"Accuracy against fp64 attention of the bf16 tensors (first {rows_} rows of every head):", "", "| what | max error | RMS error |",
                  "|---|---|---|"]
        for name, o in (("3 x quantize_fp8 + flash_attention_fp8", o_chain), ("fa3_forward(fp8=1)", o_fa3)):
            lines.append(f"| {name} | {(o - ref).abs().max().item():.3e} | {(o - ref).pow(2).mean().sqrt().item():.3e} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
