"""Timing of the lightning indexer (common/indexer.py; profiles/indexer.md) in one process, the variants of a row
interleaved round by round, HIP-event times around CALLS back-to-back calls (call times: they contain the host's enqueue where that
is the slower side), median and min / max over the rounds after one warm-up round; beside them the kernels' own times from the
library's per-launch events (fa_profile_enable).  Rows: decode, B = 32, Nq = 1 and 2, H_I = 64, 8192 and 65 536 cached tokens, page
64, topk 2048; prefill, B = 1, Nq = 2048 against 16 384 keys, causal.  Yardsticks, all measured in the same run:
  logits     the byte floor (cache bytes read + logits bytes written at the 6.3 TB/s the HBM streams at, MI355X_MICROARCH.md) and the
             torch path a user has without the library: gather through the table, dequantise to bf16, einsum, ReLU, weighted sum
  selection  torch.topk + sort on the same logits, with the masking it needs
  chain      beside the sparse attention call it feeds (flash_mla_with_kvcache(..., indices=), H_q = 128, bf16 cache) at the same shape
`--out FILE` also writes the JSON there."""
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
from common import indexer as ix  # noqa: E402
from common.attention_ex import flash_mla_with_kvcache  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--rows", default="decode,prefill")
args = ap.parse_args()
DEV, STREAM_RATE, H, D, PAGE, TOPK, TOKEN = "cuda", 6.3e12, 64, 128, 64, 2048, 144
E4M3, BF16 = torch.float8_e4m3fn, torch.bfloat16


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / args.calls * 1e3   # us a call


def kernel_times(fn):
    """{kernel: us a launch} from the library's own HIP events around each launch (no host time between the launches in it)"""
    ext.profile_enable(True)
    for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    prof = ext.profile_report()
    ext.profile_enable(False)
    return {k: ms / c * 1e3 for k, (c, ms) in prof.items()}


def interleave(variants):
    acc = {n: [] for n in variants}
    for rnd in range(args.rounds + 1):
        for name, fn in variants.items():
            t = timed(fn)
            if rnd:
                acc[name].append(t)
    return {n: dict(median_us=statistics.median(a), min_us=min(a), max_us=max(a)) for n, a in acc.items()}


def problem(b, nq, length, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mb = length // PAGE
    nblk = b * mb
    k = torch.randn((b, length, D), device=DEV, dtype=BF16, generator=g)
    pool = torch.zeros((nblk, PAGE, 1, TOKEN), dtype=torch.uint8, device=DEV)
    table = torch.randperm(nblk, device=DEV, generator=g).to(torch.int32).view(b, mb)
    ix.indexer_pack_cache(k, pool, 0, table)
    q = torch.randn((b, nq, H, D), device=DEV, generator=g).to(E4M3)
    w = torch.randn((b, nq, H), device=DEV, generator=g) * (H ** -0.5 * D ** -0.5)
    lens = torch.full((b,), length, dtype=torch.int32, device=DEV)
    return q, w, pool, lens, table


def torch_logits(q, w, pool, table):
    b, mb = table.shape
    toks = pool[table.long()].view(b, mb * PAGE, TOKEN)                       # the gather through the table
    scale = toks[..., 128:132].contiguous().view(torch.float32)               # (B, L, 1)
    k = (toks[..., :128].contiguous().view(E4M3).to(BF16) * scale.to(BF16))   # dequantised to bf16
    p = torch.einsum("bihd,bjd->bihj", q.to(BF16), k)
    return (p.relu_() * w.to(BF16).unsqueeze(-1)).sum(2, dtype=torch.float32)


def torch_select(logits, lens, causal):
    b, nq, width = logits.shape
    n = lens.view(b, 1) - (nq - 1 - torch.arange(nq, device=DEV)).view(1, nq) if causal else lens.view(b, 1).expand(b, nq)
    masked = logits.masked_fill(torch.arange(width, device=DEV).view(1, 1, width) >= n.unsqueeze(-1), float("-inf"))
    return masked.topk(min(TOPK, width), dim=-1).indices.sort(-1).values.to(torch.int32)


def spread(r):
    return (r["max_us"] - r["min_us"]) / r["median_us"]


def row(kind, b, nq, length, seed, attention=True):
    q, w, pool, lens, table = problem(b, nq, length, seed)
    logits = ix.indexer_logits(q, w, pool, lens, table, causal=True)
    variants = {
        "logits": lambda: ix.indexer_logits(q, w, pool, lens, table, causal=True, out=logits),
        "torch_logits": lambda: torch_logits(q, w, pool, table),
        "topk": lambda: ix.indexer_topk(logits, lens, TOPK, causal=True),
        "torch_topk_sort": lambda: torch_select(logits, lens, True),
        "chain": lambda: ix.lightning_indexer(q, w, pool, lens, table, TOPK, causal=True),
    }
    if attention:
        g = torch.Generator(device=DEV).manual_seed(seed + 1)
        qa = torch.randn((b, nq, 128, 576), device=DEV, dtype=BF16, generator=g)
        kv = torch.randn((pool.shape[0], PAGE, 1, 576), device=DEV, dtype=BF16, generator=g)
        lists = ix.lightning_indexer(q, w, pool, lens, table, TOPK, causal=True)
        variants["sparse_attention"] = lambda: flash_mla_with_kvcache(qa, kv, table, lens, causal=True, indices=lists)
    r = interleave(variants)
    kern = kernel_times(variants["chain"])
    floor_bytes = b * length * 132 + b * nq * length * 4
    floor_us = floor_bytes / STREAM_RATE * 1e6
    out = dict(kind=kind, B=b, Nq=nq, H_I=H, keys=length, page=PAGE, topk=TOPK, times=r, byte_floor_us=floor_us,
               logits_over_floor=r["logits"]["median_us"] / floor_us, kernels_us=kern,
               logits_kernel_over_floor=kern.get("idx_logits", 0.0) / floor_us,
               logits_vs_torch=r["torch_logits"]["median_us"] / r["logits"]["median_us"],
               topk_vs_torch=r["torch_topk_sort"]["median_us"] / r["topk"]["median_us"],
               spread={n: spread(x) for n, x in r.items()})
    # the gap to torch lies outside the spread when the slowest kernel round beats the fastest torch round
    out["logits_beats_torch"] = r["logits"]["max_us"] < r["torch_logits"]["min_us"]
    out["topk_beats_torch"] = r["topk"]["max_us"] < r["torch_topk_sort"]["min_us"]
    if kind == "prefill":
        pairs = nq * length - nq * (nq - 1) // 2
        out["logits_tflops"] = 2.0 * b * H * pairs * D / r["logits"]["median_us"] / 1e6
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_indexer: no GPU")
    res = []
    kinds = args.rows.split(",")
    if "decode" in kinds:
        for length in (8192, 65536):
            for nq in (1, 2):
                res.append(row("decode", 32, nq, length, 10 * nq + length % 7))
                torch.cuda.empty_cache()
    if "prefill" in kinds:
        res.append(row("prefill", 1, 2048, 16384, 3, attention=False))
    text = json.dumps(dict(rounds=args.rounds, calls=args.calls, stream_rate_bytes_per_s=STREAM_RATE, rows=res), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
