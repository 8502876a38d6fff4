#!/usr/bin/env python3
"""Time the rotary embedding kernel (flashattention_lab_cuda.rotary_apply, fa_rotary_apply) against a copy of the same bytes and
against the same function composed of PyTorch ops.

    python tools/bench_rotary.py [--shape 8 4096 40 128] [--dtype bf16] [--out profiles/rotary_bandwidth.md]

For the shape (B, S, H, d) in bf16 (default (8, 4096, 40, 128): 335 MB, beyond the 256 MB Infinity Cache) and rotary_dim = d, both
pairings, on one run:
  kernel, out of place : rotary_apply(x, cos, sin)               reads x, writes y
  kernel, in place     : rotary_apply(x, cos, sin, out=x)        reads x, writes x
  copy                 : y.copy_(x) of the same view             the same bytes read and written
  torch ops            : the rotation as elementwise PyTorch ops on the 16-bit tensor (the composition a user writes without
                         the kernel: slice or unflatten, two multiplies and an add per half, cat or stack), checked against the
                         kernel to one 16-bit step before it is timed
Times are HIP-event medians after warm-up; effective bandwidth counts x's bytes once read and once written.  The two ratios
reported are kernel / copy and kernel / torch ops."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-pytorch_amd"))
import flashattention_lab_cuda as ext  # noqa: E402


def timed(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)   # us
    return statistics.median(out)


def torch_rotary(x, cos, sin, interleaved):
    """the rotation in PyTorch ops on the 16-bit tensor; cos, sin (S, d / 2)"""
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    if interleaved:
        x1, x2 = x[..., 0::2], x[..., 1::2]
        return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 4096, 40, 128])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    b, s, h, d = a.shape
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((b, s, h, d), generator=g, device=dev, dtype=torch.float32).to(dtype)
    y = torch.empty_like(x)
    inv = 10000.0 ** (-torch.arange(0, d, 2, dtype=torch.float64) / d)
    ang = torch.arange(s, dtype=torch.float64).view(-1, 1) * inv.view(1, -1)
    cos, sin = torch.cos(ang).to(dtype).to(dev), torch.sin(ang).to(dtype).to(dev)
    nbytes = 2 * x.numel() * x.element_size()
    rows = []
    copy_us = timed(lambda: y.copy_(x), a.warmup, a.iters, a.reps)
    rows.append(("copy (y.copy_(x))", copy_us, None, None))
    for inter in (False, True):
        name = "GPT-J (interleaved)" if inter else "GPT-NeoX"
        ref = torch_rotary(x, cos, sin, inter)
        got = ext.rotary_apply(x, cos, sin, out=y, interleaved=inter)
        # the composition rounds each product to 16 bits: one step of the format, not bitwise
        err = (got.float() - ref.float()).abs().max().item()
        assert err <= 2.0 ** -6 * max(1.0, x.float().abs().max().item()), err
        del ref, got
        oop = timed(lambda: ext.rotary_apply(x, cos, sin, out=y, interleaved=inter), a.warmup, a.iters, a.reps)
        xin = x.clone()
        inp = timed(lambda: ext.rotary_apply(xin, cos, sin, out=xin, interleaved=inter), a.warmup, a.iters, a.reps)
        del xin
        tor = timed(lambda: torch_rotary(x, cos, sin, inter), a.warmup, max(1, a.iters // 4), a.reps)
        copy2 = timed(lambda: y.copy_(x), a.warmup, a.iters, a.reps)          # again, beside this pairing's figures
        rows.append((f"kernel, out of place, {name}", oop, oop / copy2, oop / tor))
        rows.append((f"kernel, in place, {name}", inp, inp / copy2, inp / tor))
        rows.append((f"torch ops, {name}", tor, tor / copy2, None))
        rows.append((f"copy, beside {name}", copy2, None, None))
    lines = [f"# Rotary embedding kernel: time and effective bandwidth ({torch.cuda.get_device_name(0)})", "",
             f"`tools/bench_rotary.py --shape {b} {s} {h} {d} --dtype {a.dtype}`: x ({b}, {s}, {h}, {d}) {a.dtype}, "
             f"{x.numel() * x.element_size() / 1e6:.0f} MB, rotary_dim = {d}; HIP events, median of {a.reps} groups of {a.iters} calls "
             f"after {a.warmup} warm-up calls.  Effective bandwidth = (bytes of x read + bytes of x written) / time.", "",
             "| what | us | TB/s | / copy | / torch ops |", "|---|---|---|---|---|"]
    for name, us, rc, rt in rows:
        lines.append(f"| {name} | {us:.1f} | {nbytes / us / 1e6:.2f} | {'' if rc is None else f'{rc:.2f}'} | {'' if rt is None else f'{rt:.3f}'} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
