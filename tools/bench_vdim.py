"""Interleaved A/B of attention with v narrower than q and k (fa_ex_*_vdim: MLA prefill, 192 + 128) against the two yardsticks of
DESIGN §9s, in ONE process, the variants alternating inside every round as tools/ab.py does it:

  vdim   flash_attention_ex(q192, k192, v128)                       the two-width 16-bit MFMA kernels (fa_ex_mfma_vdim.hip)
  pad    flash_attention_ex(q192, k192, pad(v128 -> 192))[..., :128] the only route before them: V (and with it dO and o)
                                                                    zero-padded to 192; the padded copy of V, the slice of o and
                                                                    autograd's padding of dO are inside the timed window.  A
                                                                    square call without extras is the plain path, whose 16-bit
                                                                    MFMA kernels pad d = 192 into 256-wide tiles; with Nq != Nk
                                                                    (--cross) the call stays in the extended family, whose MFMA
                                                                    kernels stop at d = 128: the exact-f32 kernels of fa_ex.hip
  d128   flash_attention_ex(q128, k128, v128)                       the existing 16-bit MFMA call at d = d_v = 128, same BH and N
  d128x  the same with option ex_path = 3                           ... on the extended MFMA kernels (the bodies the two-width
                                                                    kernels were derived from) instead of the plain tuned ones

Times are device-event times around `reps` calls, a warm-up round first; median (min) over the rounds.  Executed FLOPs, counted
from the shapes with the MFMA tiles' zero padding left out and the pairs the bottom-right causal mask leaves:
  forward    2 Nq Nk (d + d_v) per unit         192 + 128 against 128 + 128: 1.25
  backward   dK/dV pass 2 Nq Nk (2 d + 2 d_v)  [S, dP, dV, dK]  +  dQ pass 2 Nq Nk (2 d + d_v)  [S, dP, dQ]  =  2 Nq Nk (4 d + 3 d_v)
             4 * 192 + 3 * 128 = 1152 against 7 * 128 = 896: 1.286; forward + backward 1472 against 1152: 1.278
The result rows go to stdout as a markdown table; the results of `vdim` and `pad` are compared once per shape (max |diff|).

    python tools/bench_vdim.py [--bh 128] [--seqlens 4096 8192] [--cross 2048:8192] [--rounds 5] [--reps 2] [--skip-pad]
"""
import argparse
import statistics
import sys

sys.path.insert(0, "flashattention-pytorch_amd")
import torch
import torch.nn.functional as F

import flashattention_lab_cuda as ext
from common.attention_ex import flash_attention_ex

D, DV = 192, 128


def flops(nq, nk, d, dv, causal, backward):
    pairs = sum(min(nk, max(0, i + nk - nq + 1)) for i in range(nq)) if causal else nq * nk
    return 2.0 * pairs * ((d + dv) if not backward else (d + dv) + (4 * d + 3 * dv))


def make_variant(name, q, k, v, do, causal):
    """a callable that runs one forward (+ backward) of the variant and returns o"""
    if name == "pad":
        def run(backward):
            vp = F.pad(v, (0, D - DV))
            o = flash_attention_ex(q, k, vp, causal=causal)[..., :DV]
            if backward:
                o.backward(do)
            return o
    else:
        def run(backward):
            o = flash_attention_ex(q, k, v, causal=causal)
            if backward:
                o.backward(do)
            return o
    return run


def timed(fn, backward, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn(backward)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bh", type=int, default=128)
    ap.add_argument("--seqlens", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--cross", nargs="*", default=["2048:8192"], help="Nq:Nk shapes with Nq != Nk (prefill behind a prefix)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-pad", action="store_true", help="leave the zero-padding yardstick out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vdim.py needs the GPU: there is no fall-back"
    print(f"device: {torch.cuda.get_device_name(0)} | library {ext.version()} | bf16, BH={args.bh}, rounds={args.rounds}, reps={args.reps}")
    print("| Nq x Nk | causal | pass | vdim ms | pad ms | d128 ms | d128x ms | pad / vdim | vdim / d128 | vdim / d128x | FLOP ratio | vdim TFLOP/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    gen = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(n, n) for n in args.seqlens] + [tuple(int(x) for x in c.split(":")) for c in args.cross]
    for nq, nk in shapes:
        def t(rows, width):
            return torch.randn((args.bh, rows, width), device="cuda", dtype=torch.bfloat16, generator=gen).requires_grad_(True)
        q, k, v, q1, k1 = t(nq, D), t(nk, D), t(nk, DV), t(nq, DV), t(nk, DV)
        do = torch.randn((args.bh, nq, DV), device="cuda", dtype=torch.bfloat16, generator=gen)
        for causal in (True, False):
            variants = [("vdim", make_variant("vdim", q, k, v, do, causal), 0)]
            if not args.skip_pad:
                variants.append(("pad", make_variant("pad", q, k, v, do, causal), 0))
            variants += [("d128", make_variant("d128", q1, k1, v, do, causal), 0), ("d128x", make_variant("d128x", q1, k1, v, do, causal), 3)]
            if not args.skip_pad:   # the two routes compute the same thing
                with torch.no_grad():
                    oa, ob = variants[0][1](False).float(), variants[1][1](False).float()
                print(f"<!-- {nq} x {nk} causal={causal}: max |o_vdim - o_pad| = {(oa - ob).abs().max().item():.3e}, mean |o_vdim| = "
                      f"{oa.abs().mean().item():.3e}, elements that differ: {int((oa != ob).sum().item())} of {oa.numel()} -->")
                del oa, ob
            for backward in (False, True):
                res = {name: [] for name, _f, _p in variants}
                for rnd in range(args.rounds + 1):
                    for name, fn, path in variants:
                        ext.set_option("ex_path", path)
                        for x in (q, k, v, q1, k1):
                            x.grad = None
                        ms = timed(fn, backward, args.reps)
                        if rnd:
                            res[name].append(ms)
                ext.set_option("ex_path", 0)
                med = {name: statistics.median(xs) for name, xs in res.items()}
                cell = lambda name: f"{med[name]:.3f} ({min(res[name]):.3f})" if name in med else "-"
                fr = flops(nq, nk, D, DV, causal, backward) / flops(nq, nk, DV, DV, causal, backward)
                tf = args.bh * flops(nq, nk, D, DV, causal, backward) / (med["vdim"] * 1e-3) / 1e12
                print(f"| {nq} x {nk} | {causal} | {'fwd+bwd' if backward else 'fwd'} | {cell('vdim')} | {cell('pad')} | {cell('d128')} | {cell('d128x')} | "
                      f"{(med['pad'] / med['vdim']) if 'pad' in med else float('nan'):.2f} | {med['vdim'] / med['d128']:.2f} | "
                      f"{med['vdim'] / med['d128x']:.2f} | {fr:.3f} | {tf:.0f} |", flush=True)
        del q, k, v, q1, k1, do
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
