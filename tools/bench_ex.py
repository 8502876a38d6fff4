"""Forward / backward time of the extended attention path (fa_ex_forward / fa_ex_backward) per feature and per kernel
family (16-bit MFMA kernels, csrc/fa_ex_mfma.hip; exact-f32 kernels, csrc/fa_ex.hip), with the visible fraction of the
score matrix accounted for (algorithmic FLOPs = 4 / 10 x visible (q, key) pairs x d).

    python tools/bench_ex.py [--bh 32] [--nq 2048] [--nk 4096] [--head-dim 128] [--dtype bf16] [--paths default,mfma,exact]

Grouped-query attention (--kv-heads 8,1): B x H_q query heads (--batch, --q-heads, --nq = --nk) against each listed K/V head
count, causal and not.  Per row: the grouped call (fa_ex_*_grouped), the same call with H_kv = H_q, and the repeat_interleave
route (K and V expanded by torch, autograd sums their gradients); forward and backward alone for the first two, the whole
autograd step (flash_attention_ex forward + backward) for all three, and the group-sum kernel's share of the backward.

    python tools/bench_ex.py --kv-heads 8,1 [--batch 8] [--q-heads 32] [--nq 4096] [--head-dim 128]

Sliding window (--window L,R; -1 = unbounded, bottom-right aligned as the causal flag; --causal for a causal window): three calls
on the same kernel family (--paths, one of them; default mfma), timed alternately in one process — the native window
(fa_ex_*_window), the same window as one shared dense mask, and the full causal call — forward and backward, with visible-pair
TFLOP/s (4 / 10 x visible pairs x d, the pairs counted from the shapes).

    python tools/bench_ex.py --window 1024,0 --causal [--bh 32] [--nq 16384] [--nk 16384] [--head-dim 128] [--rounds 3]

Packed sequences (--varlen LENS: NxB = B sequences of N tokens, or mix:COUNT:LO:HI = a seeded (--seed) mix of COUNT lengths in
[LO, HI]): the varlen call (fa_ex_*_varlen, --q-heads, --kv-heads one count, default = --q-heads; --causal) timed alternately in
one process against, with equal lengths, the same tensors in (B*H, N, d) layout through the extended MFMA kernels (ex_path 3);
with a mix, (a) padding to the longest with a key-padding mask through flash_attention_ex's entry points and (b) one call per
sequence.  Forward and backward, visible-pair TFLOP/s (4 / 10 x visible pairs x d).

    python tools/bench_ex.py --varlen 4096x8 [--causal] [--q-heads 32] [--head-dim 128] [--rounds 3]
    python tools/bench_ex.py --varlen mix:16:256:8192 --causal --q-heads 32 --kv-heads 8 [--seed 0]

Score modifiers (--softcap C and / or --alibi: the standard slopes 2^(-8 (h + 1) / H), shape (H,)): B x H query heads, N = --nq
(square), timed alternately in one process — the modified call (fa_ex_*_scoremod), the same call without modifiers on the same
kernel family (ex_path 3: the extended MFMA kernels), and without modifiers as the library routes it (ex_path 0: the plain
kernels for a square call) — forward and backward.

    python tools/bench_ex.py --softcap 30 --alibi [--causal] [--batch 8] [--q-heads 32] [--nq 4096] [--head-dim 128] [--rounds 3]
Attention sinks (--sinks: one logit per head, shape (H,)): the same shapes, optionally with --window L,R; the call with sinks
against the call without on the extended MFMA kernels (ex_path 3) and on the default path, alternated --rounds times:
    python tools/bench_ex.py --sinks --causal [--window 1024,-1] [--batch 8] [--q-heads 32] [--nq 4096] [--head-dim 128] [--rounds 3]
An additive bias (--bias: attn_bias, randn * 2 in the tensor dtype): BH = --bh units as B = BH / --q-heads batches of --q-heads heads,
Nq = --nq, Nk = --nk.  Alternated --rounds times in one process: the call with a full (B, H, Nq, Nk) bias and with a (1, H, Nq, Nk)
bias, forward and backward with and without dbias; the same call without a bias on the extended MFMA kernels (ex_path 3) and as the
library routes it; and the call with a random dense mask (half the pairs).  Beside the times the bytes the bias adds per pass:
    python tools/bench_ex.py --bias [--causal] [--bh 32] [--q-heads 8] [--nq 2048] [--nk 4096] [--head-dim 128] [--rounds 3]
"""
import argparse
import json
import sys

sys.path.insert(0, "flashattention-pytorch_amd")   # (run from the repository root)
import torch
import flashattention_lab_cuda as ext


def timed(fn, iters=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bh", type=int, default=32)
    ap.add_argument("--nq", type=int, default=2048)
    ap.add_argument("--nk", type=int, default=4096)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--paths", default="mfma,exact")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kv-heads", default="", help="comma-separated K/V head counts: time grouped-query attention instead")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--q-heads", type=int, default=32)
    ap.add_argument("--window", default="", help="L,R: time a sliding window against its dense mask and the causal call")
    ap.add_argument("--causal", action="store_true", help="(--window) the causal flag with the window")
    ap.add_argument("--rounds", type=int, default=3, help="(--window) alternations of the three calls")
    ap.add_argument("--varlen", default="", help="NxB or mix:COUNT:LO:HI: time packed sequences")
    ap.add_argument("--seed", type=int, default=0, help="(--varlen mix) the lengths' seed")
    ap.add_argument("--softcap", type=float, default=0.0, help="time the softcap (and --alibi) against the call without")
    ap.add_argument("--alibi", action="store_true", help="time ALiBi slopes (and --softcap) against the call without")
    ap.add_argument("--sinks", action="store_true", help="time attention sinks ((H,) logits) against the call without")
    ap.add_argument("--bias", action="store_true", help="time an additive attn_bias (and its dbias) against the call without")
    args = ap.parse_args()
    if args.bias:
        return bench_bias(args)
    if args.sinks:
        return bench_sinks(args)
    if args.softcap > 0.0 or args.alibi:
        return bench_scoremod(args)
    if args.varlen:
        return bench_varlen(args)
    if args.kv_heads:
        return bench_gqa(args)
    if args.window:
        return bench_window(args)
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    bh, nq, nk, d = args.bh, args.nq, args.nk, args.head_dim
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((bh, nq, d), device="cuda", dtype=dt, generator=g)
    k, v = (torch.randn((bh, nk, d), device="cuda", dtype=dt, generator=g) for _ in range(2))
    do = torch.randn((bh, nq, d), device="cuda", dtype=dt, generator=g)
    qi, kj = torch.arange(nq, device="cuda").unsqueeze(1), torch.arange(nk, device="cuda").unsqueeze(0)
    dense = (torch.rand((nq, nk), device="cuda", generator=g) < 0.5).to(torch.uint8)
    dense[:, 0] = 1
    bm = (torch.rand(((nq + 127) // 128, (nk + 127) // 128), device="cuda", generator=g) < 0.25).to(torch.uint8)
    bm[:, 0] = 1
    cases = {
        "plain (Nq != Nk)": dict(),
        "causal, bottom-right aligned": dict(causal=True),
        "dense mask, half the pairs": dict(mask=dense),
        "the causal mask handed over as a dense one": dict(mask=(kj <= qi + (nk - nq)).to(torch.uint8)),
        "block-sparse 128x128, a quarter of the tiles": dict(block_mask=bm, br=128, bc=128),
        "dropout 0.1": dict(dropout_p=0.1, seed=1),
        "causal + dropout 0.1": dict(causal=True, dropout_p=0.1, seed=1),
    }
    rows = []
    paths = ["exact"] if args.dtype == "fp32" else args.paths.split(",")
    for path in paths:
      ext.set_option("ex_path", {"mfma": 3, "exact": 1}.get(path, 0))   # 3: the extended MFMA kernels even where the plain ones would do; default: the library's own choice
      for name, kw in cases.items():
        kw = dict(kw)
        causal = kw.pop("causal", False)
        vis = torch.ones((nq, nk), dtype=torch.bool, device="cuda")
        if causal:
            vis &= kj <= qi + (nk - nq)
        if "mask" in kw:
            vis &= kw["mask"] != 0
        if "block_mask" in kw:
            vis &= kw["block_mask"].repeat_interleave(128, 0)[:nq].repeat_interleave(128, 1)[:, :nk] != 0
        frac = vis.float().mean().item()
        o, lse = ext.ex_forward(q, k, v, causal, d ** -0.5, **kw)
        tf = timed(lambda: ext.ex_forward(q, k, v, causal, d ** -0.5, **kw), args.iters)
        tb = timed(lambda: ext.ex_backward(q, k, v, o, do, lse, causal, d ** -0.5, **kw), args.iters)
        pairs = bh * nq * nk * frac
        rows.append(dict(kernels=path, case=name, visible_fraction=round(frac, 4), fwd_ms=round(tf, 3), bwd_ms=round(tb, 3),
                         fwd_tflops=round(4 * pairs * d / tf / 1e9, 2), bwd_tflops=round(10 * pairs * d / tb / 1e9, 2)))
    ext.set_option("ex_path", 0)
    print(json.dumps(dict(shape=dict(bh=bh, nq=nq, nk=nk, d=d, dtype=args.dtype),
                          kernels="mfma: v_mfma_f32_32x32x16 (peak 2500 TFLOP/s); exact: v_mfma_f32_16x16x4_f32 (peak 157 TFLOP/s)",
                          rows=rows), indent=1))


def bench_gqa(args):
    from common.attention_ex import flash_attention_ex

    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    b, hq, n, d = args.batch, args.q_heads, args.nq, args.head_dim
    scale = d ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((b * hq, n, d), device="cuda", dtype=dt, generator=g)
    do = torch.randn((b * hq, n, d), device="cuda", dtype=dt, generator=g)
    kf, vf = (torch.randn((b * hq, n, d), device="cuda", dtype=dt, generator=g) for _ in range(2))   # H_kv = H_q
    rows = []
    for hkv in (int(x) for x in args.kv_heads.split(",")):
        grp = hq // hkv
        k, v = kf[: b * hkv].clone(), vf[: b * hkv].clone()
        for causal in (False, True):
            row = dict(h_q=hq, h_kv=hkv, causal=causal)
            for name, kk, vv in (("grouped", k, v), ("ungrouped", kf, vf)):
                o, lse = ext.ex_forward(q, kk, vv, causal, scale)
                row[name + "_fwd_ms"] = round(timed(lambda: ext.ex_forward(q, kk, vv, causal, scale), args.iters), 3)
                row[name + "_bwd_ms"] = round(timed(lambda: ext.ex_backward(q, kk, vv, o, do, lse, causal, scale), args.iters), 3)
                if name == "grouped":
                    ext.profile_enable(True)
                    ext.ex_backward(q, kk, vv, o, do, lse, causal, scale)
                    torch.cuda.synchronize()
                    prof = ext.profile_report()
                    ext.profile_enable(False)
                    row["kv_group_sum_ms"] = round(prof.get("kv_group_sum", (0, 0.0))[1], 3)
            leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
            full = [t.detach().clone().requires_grad_(True) for t in (kf, vf)]

            def step(route):
                if route == "grouped":
                    o = flash_attention_ex(leaves[0], leaves[1], leaves[2], causal=causal, softmax_scale=scale)
                elif route == "ungrouped":
                    o = flash_attention_ex(leaves[0], full[0], full[1], causal=causal, softmax_scale=scale)
                else:   # expand K and V by torch; autograd sums the gradients of each group
                    o = flash_attention_ex(leaves[0], leaves[1].repeat_interleave(grp, 0), leaves[2].repeat_interleave(grp, 0),
                                           causal=causal, softmax_scale=scale)
                o.backward(do)

            for route in ("grouped", "ungrouped", "repeat_interleave"):
                row[route + "_step_ms"] = round(timed(lambda: step(route), args.iters), 3)
            rows.append(row)
            del leaves, full
    print(json.dumps(dict(shape=dict(batch=b, q_heads=hq, n=n, d=d, dtype=args.dtype), rows=rows), indent=1))


def window_pairs(nq, nk, causal, wl, wr):
    """Visible (query, key) pairs of one (b,h) under the window, counted row by row from the shapes."""
    c, total = nk - nq, 0
    for i in range(nq):
        lo = 0 if wl < 0 else max(0, i + c - wl)
        hi = nk - 1 if wr < 0 else min(nk - 1, i + c + wr)
        if causal:
            hi = min(hi, i + c)
        total += max(0, hi - lo + 1)
    return total


def bench_window(args):
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    bh, nq, nk, d = args.bh, args.nq, args.nk, args.head_dim
    wl, wr = (int(x) for x in args.window.split(","))
    path = args.paths.split(",")[0]
    scale = d ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((bh, nq, d), device="cuda", dtype=dt, generator=g)
    k, v = (torch.randn((bh, nk, d), device="cuda", dtype=dt, generator=g) for _ in range(2))
    do = torch.randn((bh, nq, d), device="cuda", dtype=dt, generator=g)
    qi, kj = torch.arange(nq, device="cuda").unsqueeze(1), torch.arange(nk, device="cuda").unsqueeze(0)
    vis = torch.ones((nq, nk), dtype=torch.bool, device="cuda")
    if wl >= 0:
        vis &= kj >= qi + (nk - nq) - wl
    if wr >= 0:
        vis &= kj <= qi + (nk - nq) + wr
    if args.causal:
        vis &= kj <= qi + (nk - nq)
    calls = {
        "window": (args.causal, dict(window=(wl, wr))),
        "dense_mask": (False, dict(mask=vis.to(torch.uint8))),
        "causal": (True, dict()),
    }
    pairs = {"window": window_pairs(nq, nk, args.causal, wl, wr), "causal": window_pairs(nq, nk, True, -1, -1)}
    pairs["dense_mask"] = pairs["window"]
    assert pairs["window"] == int(vis.sum().item())
    ext.set_option("ex_path", {"mfma": 3, "exact": 1}.get(path, 0))
    times = {name: ([], []) for name in calls}
    try:
        outs = {}
        for name, (causal, kw) in calls.items():
            outs[name] = ext.ex_forward(q, k, v, causal, scale, **kw)
        for _ in range(args.rounds):
            for name, (causal, kw) in calls.items():
                o, lse = outs[name]
                times[name][0].append(timed(lambda: ext.ex_forward(q, k, v, causal, scale, **kw), args.iters))
                times[name][1].append(timed(lambda: ext.ex_backward(q, k, v, o, do, lse, causal, scale, **kw), args.iters))
    finally:
        ext.set_option("ex_path", 0)
    rows = []
    for name in calls:
        tf, tb = sorted(times[name][0])[len(times[name][0]) // 2], sorted(times[name][1])[len(times[name][1]) // 2]
        p = bh * pairs[name]
        rows.append(dict(call=name, visible_pairs_per_bh=pairs[name], fwd_ms=round(tf, 3), bwd_ms=round(tb, 3),
                         fwd_bwd_ms=round(tf + tb, 3), fwd_tflops=round(4 * p * d / tf / 1e9, 1),
                         bwd_tflops=round(10 * p * d / tb / 1e9, 1), fwd_ms_all=[round(x, 3) for x in times[name][0]],
                         bwd_ms_all=[round(x, 3) for x in times[name][1]]))
    by = {r["call"]: r for r in rows}
    summary = dict(
        window_over_causal_time=round(by["window"]["fwd_bwd_ms"] / by["causal"]["fwd_bwd_ms"], 3),
        dense_mask_over_window_time=round(by["dense_mask"]["fwd_bwd_ms"] / by["window"]["fwd_bwd_ms"], 2),
        window_over_causal_pairs=round(pairs["window"] / pairs["causal"], 4),
        window_over_causal_pair_rate=round((pairs["window"] / (by["window"]["fwd_bwd_ms"])) /
                                           (pairs["causal"] / by["causal"]["fwd_bwd_ms"]), 3))
    print(json.dumps(dict(shape=dict(bh=bh, nq=nq, nk=nk, d=d, dtype=args.dtype, window=[wl, wr], causal=args.causal,
                                     kernels=path, iters=args.iters, rounds=args.rounds), rows=rows, summary=summary), indent=1))


def varlen_lengths(spec, seed):
    if spec.startswith("mix:"):
        _, count, lo, hi = spec.split(":")
        g = torch.Generator().manual_seed(seed)
        return torch.randint(int(lo), int(hi) + 1, (int(count),), generator=g).tolist()
    n, b = spec.lower().split("x")
    return [int(n)] * int(b)


def bench_varlen(args):
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    lens = varlen_lengths(args.varlen, args.seed)
    hq = args.q_heads
    hkv = int(args.kv_heads) if args.kv_heads else hq
    d, causal, scale, B = args.head_dim, args.causal, args.head_dim ** -0.5, len(lens)
    total, mx = sum(lens), max(lens)
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn((total, hq, d), device="cuda", dtype=dt, generator=g)
    k, v = (torch.randn((total, hkv, d), device="cuda", dtype=dt, generator=g) for _ in range(2))
    do = torch.randn((total, hq, d), device="cuda", dtype=dt, generator=g)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
    pairs = sum(hq * (n * (n + 1) // 2 if causal else n * n) for n in lens)
    calls = {}
    o, lse = ext.ex_varlen_forward(q, k, v, cu, cu, mx, mx, causal, scale)
    calls["varlen"] = (lambda: ext.ex_varlen_forward(q, k, v, cu, cu, mx, mx, causal, scale),
                       lambda: ext.ex_varlen_backward(q, k, v, o, do, lse, cu, cu, mx, mx, causal, scale), pairs)

    def heads_first(t, n):   # (B*n, H, d) -> (B*H, n, d)
        return t.view(-1, n, t.shape[1], d).transpose(1, 2).reshape(-1, n, d).contiguous()

    if len(set(lens)) == 1:   # the same tensors in (B*H, N, d) layout
        n = lens[0]
        q3, k3, v3, do3 = (heads_first(t, n) for t in (q, k, v, do))
        o3, lse3 = ext.ex_forward(q3, k3, v3, causal, scale)
        calls["bhnd"] = (lambda: ext.ex_forward(q3, k3, v3, causal, scale),
                         lambda: ext.ex_backward(q3, k3, v3, o3, do3, lse3, causal, scale), pairs)
    else:
        # (a) padded to the longest, keys past each sequence masked: (B*H, max, max) mask bytes
        qp, kp, vp, dop = (torch.zeros((B * t.shape[1], mx, d), device="cuda", dtype=dt) for t in (q, k, v, do))
        kpm = torch.zeros((B, mx), dtype=torch.uint8, device="cuda")
        s0 = 0
        for b, n in enumerate(lens):
            for src, dst in ((q, qp), (k, kp), (v, vp), (do, dop)):
                h = src.shape[1]
                dst[b * h:(b + 1) * h, :n] = src[s0:s0 + n].transpose(0, 1)
            kpm[b, :n] = 1
            s0 += n
        mask = kpm[:, None, None, :].expand(B, hq, mx, mx).reshape(B * hq, mx, mx).contiguous()
        op, lsep = ext.ex_forward(qp, kp, vp, causal, scale, mask=mask)
        calls["padded_mask"] = (lambda: ext.ex_forward(qp, kp, vp, causal, scale, mask=mask),
                                lambda: ext.ex_backward(qp, kp, vp, op, dop, lsep, causal, scale, mask=mask), pairs)
        # (b) one call per sequence
        seqs, s0 = [], 0
        for n in lens:
            qs, ks, vs, dos = (t[s0:s0 + n].transpose(0, 1).contiguous() for t in (q, k, v, do))
            os_, ls_ = ext.ex_forward(qs, ks, vs, causal, scale)
            seqs.append((qs, ks, vs, dos, os_, ls_))
            s0 += n
        calls["per_sequence"] = (lambda: [ext.ex_forward(a[0], a[1], a[2], causal, scale) for a in seqs],
                                 lambda: [ext.ex_backward(a[0], a[1], a[2], a[4], a[3], a[5], causal, scale) for a in seqs], pairs)
    times = {name: ([], []) for name in calls}
    ext.set_option("ex_path", 3 if len(set(lens)) == 1 else 0)   # equal lengths: the extended MFMA kernels on both sides
    try:
        for _ in range(args.rounds):
            for name, (f, b, _p) in calls.items():
                times[name][0].append(timed(f, args.iters))
                times[name][1].append(timed(b, args.iters))
    finally:
        ext.set_option("ex_path", 0)
    rows = []
    for name, (_f, _b, p) in calls.items():
        tf, tb = sorted(times[name][0])[len(times[name][0]) // 2], sorted(times[name][1])[len(times[name][1]) // 2]
        rows.append(dict(call=name, fwd_ms=round(tf, 3), bwd_ms=round(tb, 3), fwd_bwd_ms=round(tf + tb, 3),
                         fwd_tflops=round(4 * p * d / tf / 1e9, 1), bwd_tflops=round(10 * p * d / tb / 1e9, 1),
                         fwd_ms_all=[round(x, 3) for x in times[name][0]], bwd_ms_all=[round(x, 3) for x in times[name][1]]))
    print(json.dumps(dict(shape=dict(lens=lens, total=total, q_heads=hq, kv_heads=hkv, d=d, dtype=args.dtype, causal=causal,
                                     visible_pairs=pairs, iters=args.iters, rounds=args.rounds), rows=rows), indent=1))


def bench_scoremod(args):
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    b, h, n, d, causal = args.batch, args.q_heads, args.nq, args.head_dim, args.causal
    bh, scale = b * h, args.head_dim ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, do = (torch.randn((bh, n, d), device="cuda", dtype=dt, generator=g) for _ in range(4))
    slopes = None
    if args.alibi:   # (H,) as a (B, H) view: one slope per head, shared by the batch
        slopes = torch.tensor([2.0 ** (-8.0 * (i + 1) / h) for i in range(h)], dtype=torch.float32, device="cuda")
        slopes = slopes.unsqueeze(0).expand(b, h)
    mod = dict(softcap=args.softcap, alibi_slopes=slopes)
    pairs = bh * (n * (n + 1) // 2 if causal else n * n)
    o, lse = ext.ex_forward(q, k, v, causal, scale, **mod)
    o0, lse0 = ext.ex_forward(q, k, v, causal, scale)
    calls = {   # name: (ex_path, forward, backward)
        "scoremod": (0, lambda: ext.ex_forward(q, k, v, causal, scale, **mod),
                     lambda: ext.ex_backward(q, k, v, o, do, lse, causal, scale, **mod)),
        "none_ex_mfma": (3, lambda: ext.ex_forward(q, k, v, causal, scale),
                         lambda: ext.ex_backward(q, k, v, o0, do, lse0, causal, scale)),
        "none_auto": (0, lambda: ext.ex_forward(q, k, v, causal, scale),
                      lambda: ext.ex_backward(q, k, v, o0, do, lse0, causal, scale)),
    }
    times = {name: ([], []) for name in calls}
    try:
        for _ in range(args.rounds):
            for name, (path, f, bw) in calls.items():
                ext.set_option("ex_path", path)
                times[name][0].append(timed(f, args.iters))
                times[name][1].append(timed(bw, args.iters))
    finally:
        ext.set_option("ex_path", 0)
    med = {name: (sorted(t[0])[len(t[0]) // 2], sorted(t[1])[len(t[1]) // 2]) for name, t in times.items()}
    rows = []
    for name, (tf, tb) in med.items():
        rows.append(dict(call=name, fwd_ms=round(tf, 3), bwd_ms=round(tb, 3), fwd_bwd_ms=round(tf + tb, 3),
                         fwd_tflops=round(4 * pairs * d / tf / 1e9, 1), bwd_tflops=round(10 * pairs * d / tb / 1e9, 1),
                         fwd_vs_ex=round(tf / med["none_ex_mfma"][0], 3), bwd_vs_ex=round(tb / med["none_ex_mfma"][1], 3),
                         fwd_ms_all=[round(x, 3) for x in times[name][0]], bwd_ms_all=[round(x, 3) for x in times[name][1]]))
    print(json.dumps(dict(shape=dict(batch=b, q_heads=h, n=n, d=d, dtype=args.dtype, causal=causal, softcap=args.softcap,
                                     alibi=args.alibi, iters=args.iters, rounds=args.rounds), rows=rows)))


def bench_sinks(args):
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    b, h, n, d, causal = args.batch, args.q_heads, args.nq, args.head_dim, args.causal
    bh, scale = b * h, args.head_dim ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, do = (torch.randn((bh, n, d), device="cuda", dtype=dt, generator=g) for _ in range(4))
    sinks = torch.randn((h,), device="cuda", generator=g)
    kw = {}
    if args.window:
        kw["window"] = tuple(int(x) for x in args.window.split(","))
    o, lse = ext.ex_forward(q, k, v, causal, scale, sinks=sinks, **kw)
    o0, lse0 = ext.ex_forward(q, k, v, causal, scale, **kw)
    calls = {   # name: (ex_path, forward, backward)
        "sinks": (0, lambda: ext.ex_forward(q, k, v, causal, scale, sinks=sinks, **kw),
                  lambda: ext.ex_backward(q, k, v, o, do, lse, causal, scale, sinks=sinks, **kw)),
        "none_ex_mfma": (3, lambda: ext.ex_forward(q, k, v, causal, scale, **kw),
                         lambda: ext.ex_backward(q, k, v, o0, do, lse0, causal, scale, **kw)),
        "none_auto": (0, lambda: ext.ex_forward(q, k, v, causal, scale, **kw),
                      lambda: ext.ex_backward(q, k, v, o0, do, lse0, causal, scale, **kw)),
    }
    times = {name: ([], []) for name in calls}
    try:
        for _ in range(args.rounds):
            for name, (path, f, bw) in calls.items():
                ext.set_option("ex_path", path)
                times[name][0].append(timed(f, args.iters))
                times[name][1].append(timed(bw, args.iters))
    finally:
        ext.set_option("ex_path", 0)
    med = {name: (sorted(t[0])[len(t[0]) // 2], sorted(t[1])[len(t[1]) // 2]) for name, t in times.items()}
    rows = []
    for name, (tf, tb) in med.items():
        rows.append(dict(call=name, fwd_ms=round(tf, 3), bwd_ms=round(tb, 3), fwd_bwd_ms=round(tf + tb, 3),
                         fwd_vs_ex=round(tf / med["none_ex_mfma"][0], 3), bwd_vs_ex=round(tb / med["none_ex_mfma"][1], 3),
                         fwd_ms_all=[round(x, 3) for x in times[name][0]], bwd_ms_all=[round(x, 3) for x in times[name][1]]))
    print(json.dumps(dict(shape=dict(batch=b, q_heads=h, n=n, d=d, dtype=args.dtype, causal=causal, window=args.window, sinks=True,
                                     iters=args.iters, rounds=args.rounds), rows=rows)))


def bench_bias(args):
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    bh, nq, nk, d, causal = args.bh, args.nq, args.nk, args.head_dim, args.causal
    h = args.q_heads if bh % args.q_heads == 0 else 1
    b, scale = bh // h, d ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q, do = (torch.randn((bh, nq, d), device="cuda", dtype=dt, generator=g) for _ in range(2))
    k, v = (torch.randn((bh, nk, d), device="cuda", dtype=dt, generator=g) for _ in range(2))
    nkp = (nk + 7) // 8 * 8
    full = (torch.randn((b, h, nq, nkp), device="cuda", generator=g) * 2).to(dt)[..., :nk]
    one_h = (torch.randn((1, h, nq, nkp), device="cuda", generator=g) * 2).to(dt)[..., :nk]
    mask = (torch.rand((nq, nk), device="cuda", generator=g) < 0.5).to(torch.uint8)
    mask[:, 0] = 1
    o0, l0 = ext.ex_forward(q, k, v, causal, scale)
    of, lf = ext.ex_forward(q, k, v, causal, scale, attn_bias=full)
    oh, lh = ext.ex_forward(q, k, v, causal, scale, attn_bias=one_h)
    om, lm = ext.ex_forward(q, k, v, causal, scale, mask=mask)

    def bwd(o, lse, **kw):
        return lambda: ext.ex_backward(q, k, v, o, do, lse, causal, scale, **kw)
    calls = {   # name: (ex_path, forward, backward, backward with dbias)
        "bias_full": (0, lambda: ext.ex_forward(q, k, v, causal, scale, attn_bias=full), bwd(of, lf, attn_bias=full),
                      bwd(of, lf, attn_bias=full, need_dbias=True)),
        "bias_1h": (0, lambda: ext.ex_forward(q, k, v, causal, scale, attn_bias=one_h), bwd(oh, lh, attn_bias=one_h),
                    bwd(oh, lh, attn_bias=one_h, need_dbias=True)),
        "none_ex_mfma": (3, lambda: ext.ex_forward(q, k, v, causal, scale), bwd(o0, l0), None),
        "none_auto": (0, lambda: ext.ex_forward(q, k, v, causal, scale), bwd(o0, l0), None),
        "dense_mask": (0, lambda: ext.ex_forward(q, k, v, causal, scale, mask=mask), bwd(om, lm, mask=mask), None),
    }
    times = {name: ([], [], []) for name in calls}
    try:
        for _ in range(args.rounds):
            for name, (path, f, bw, bwd_db) in calls.items():
                ext.set_option("ex_path", path)
                times[name][0].append(timed(f, args.iters))
                times[name][1].append(timed(bw, args.iters))
                if bwd_db is not None:
                    times[name][2].append(timed(bwd_db, args.iters))
    finally:
        ext.set_option("ex_path", 0)
    med = lambda t: round(sorted(t)[len(t) // 2], 3) if t else None   # noqa: E731
    rows = [dict(call=name, fwd_ms=med(t[0]), bwd_ms=med(t[1]), bwd_dbias_ms=med(t[2]), fwd_ms_all=[round(x, 3) for x in t[0]],
                 bwd_ms_all=[round(x, 3) for x in t[1]], bwd_dbias_ms_all=[round(x, 3) for x in t[2]]) for name, t in times.items()]
    print(json.dumps(dict(shape=dict(bh=bh, batch=b, q_heads=h, nq=nq, nk=nk, d=d, dtype=args.dtype, causal=causal, bias=True, iters=args.iters,
                                     rounds=args.rounds),
                          bias_bytes_per_pass=bh * nq * nk * 2, dbias_bytes=bh * nq * nk * 2, rows=rows)))


if __name__ == "__main__":
    main()
