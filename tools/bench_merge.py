#!/usr/bin/env python3
"""Time the merge of two partial attention results (flashattention_lab_cuda.merge_states / merge_states_backward,
fa_merge_states / fa_merge_states_backward) against torch.add of the same tensors and against the merge composed of PyTorch ops.

    python tools/bench_merge.py [--shape 8 40 4096 128] [--dtype bf16] [--out profiles/merge_states.md]

For o of shape (B, H, N, d) (default (8, 40, 4096, 128) bf16: 336 MB per tensor, beyond the 256 MB Infinity Cache), on one run:
  add                  : torch.add(o_a, o_b, out=o)             reads two tensors, writes one: the forward's bytes (less the lse)
  kernel, forward      : merge_states(o_a, lse_a, o_b, lse_b, out=(o, lse))
  kernel, in place     : merge_states(..., out=(o_a, lse_a))
  kernel, backward     : merge_states_backward(o_a, lse_a, o_b, lse_b, dO, dlse): reads three o-like tensors, writes two: 5 / 3
                         of the forward's bytes
  torch ops, forward   : the merge as elementwise PyTorch ops in fp32 (the composition a user writes without the kernel), checked
                         against the kernel to one 16-bit step before it is timed
  torch ops, backward  : the closed-form backward as PyTorch ops in fp32
Times are HIP-event medians after warm-up; effective bandwidth counts the o-like tensors a call must read and write once each
(3 forward, 5 backward) plus the float32 lse-like ones.  Ratios: / add in the same run; backward / forward beside its byte ratio."""
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


def torch_merge(o_a, lse_a, o_b, lse_b):
    lse = torch.logaddexp(lse_a, lse_b)
    wa, wb = torch.exp(lse_a - lse).unsqueeze(-1), torch.exp(lse_b - lse).unsqueeze(-1)
    return (wa * o_a.float() + wb * o_b.float()).to(o_a.dtype), lse


def torch_merge_backward(o_a, lse_a, o_b, lse_b, do, dlse):
    lse = torch.logaddexp(lse_a, lse_b)
    wa, wb = torch.exp(lse_a - lse), torch.exp(lse_b - lse)
    dof = do.float()
    t = (dof * (o_a.float() - o_b.float())).sum(-1)
    return ((wa.unsqueeze(-1) * dof).to(do.dtype), (wb.unsqueeze(-1) * dof).to(do.dtype), wa * (dlse + wb * t), wb * (dlse - wa * t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 40, 4096, 128])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    b, h, n, d = a.shape
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    o_a, o_b, do = (torch.randn((b, h, n, d), generator=g, device=dev, dtype=torch.float32).to(dtype) for _ in range(3))
    lse_a, lse_b, dlse = (2.0 * torch.randn((b, h, n), generator=g, device=dev) for _ in range(3))
    o, lse = torch.empty_like(o_a), torch.empty_like(lse_a)
    ob, lb = o_a.numel() * o_a.element_size(), lse_a.numel() * 4
    fwd_bytes, bwd_bytes = 3 * ob + 3 * lb, 5 * ob + 5 * lb

    ref_o, ref_lse = torch_merge(o_a, lse_a, o_b, lse_b)
    ext.merge_states(o_a, lse_a, o_b, lse_b, out=(o, lse))
    err = (o.float() - ref_o.float()).abs().max().item()     # the composition rounds w to fp32: one step of the format at most
    assert err <= 2.0 ** (-6 if dtype != torch.float32 else -20) * max(1.0, ref_o.float().abs().max().item()), err
    assert (lse - ref_lse).abs().max().item() <= 1e-5
    del ref_o, ref_lse

    rows = []
    add_us = timed(lambda: torch.add(o_a, o_b, out=o), a.warmup, a.iters, a.reps)
    fwd = timed(lambda: ext.merge_states(o_a, lse_a, o_b, lse_b, out=(o, lse)), a.warmup, a.iters, a.reps)
    acc_o, acc_l = o_a.clone(), lse_a.clone()
    inp = timed(lambda: ext.merge_states(acc_o, acc_l, o_b, lse_b, out=(acc_o, acc_l)), a.warmup, a.iters, a.reps)
    del acc_o, acc_l
    bwd = timed(lambda: ext.merge_states_backward(o_a, lse_a, o_b, lse_b, do, dlse), a.warmup, a.iters, a.reps)
    tfw = timed(lambda: torch_merge(o_a, lse_a, o_b, lse_b), a.warmup, max(1, a.iters // 4), a.reps)
    tbw = timed(lambda: torch_merge_backward(o_a, lse_a, o_b, lse_b, do, dlse), a.warmup, max(1, a.iters // 4), a.reps)
    add2 = timed(lambda: torch.add(o_a, o_b, out=o), a.warmup, a.iters, a.reps)       # again, at the end of the run
    rows.append(("torch.add(o_a, o_b, out=o)", add_us, 3 * ob, None, None))
    rows.append(("kernel, forward", fwd, fwd_bytes, fwd / add_us, fwd / tfw))
    rows.append(("kernel, forward in place", inp, fwd_bytes, inp / add_us, inp / tfw))
    rows.append(("kernel, backward", bwd, bwd_bytes, bwd / add_us, bwd / tbw))
    rows.append(("torch ops, forward", tfw, fwd_bytes, tfw / add_us, None))
    rows.append(("torch ops, backward", tbw, bwd_bytes, tbw / add_us, None))
    rows.append(("torch.add again, at the end", add2, 3 * ob, None, None))
    lines = [f"# Merge of partial attention results: time and effective bandwidth ({torch.cuda.get_device_name(0)})", "",
             f"`tools/bench_merge.py --shape {b} {h} {n} {d} --dtype {a.dtype}`: o ({b}, {h}, {n}, {d}) {a.dtype}, {ob / 1e6:.0f} MB per "
             f"tensor; HIP events, median of {a.reps} groups of {a.iters} calls after {a.warmup} warm-up calls.  Effective bandwidth = "
             f"(bytes the call must read + write once) / time: 3 o-like tensors forward, 5 backward.", "",
             "| what | us | TB/s | / add | / torch ops |", "|---|---|---|---|---|"]
    for name, us, nbytes, rc, rt in rows:
        lines.append(f"| {name} | {us:.1f} | {nbytes / us / 1e6:.2f} | {'' if rc is None else f'{rc:.2f}'} | {'' if rt is None else f'{rt:.3f}'} |")
    lines += ["", f"backward / forward = {bwd / fwd:.2f} (bytes: {bwd_bytes / fwd_bytes:.2f})"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
