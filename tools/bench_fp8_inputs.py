"""Forward-only timing of the fp8-inputs call (flash_attention_fp8 / fa_fp8_forward) at tools/bench_fp8.py's
shape (B = 1, H = 16, N = 16384, d = 128, causal and not), interleaved in one process with the bf16 forward and with
fa3_forward(fp8 = 1) on the same 16-bit data; the new call runs on tensors quantised ONCE outside the timed region (one absmax descale
per (batch, K/V head)).  HIP-event kernel times per call from the library's profiler, median and spread over the rounds.  Further
rows: GQA (H_q = 32, H_kv = 8, N = 8192), chunked prefill (Nq = 2048, Nk = 16384, causal) against the bf16 extended forward, and the
V transposer's time over its byte floor (2 * units * Nk * 128 bytes at the 8 TB/s HBM peak).
`--accuracy`: max |o - fp64| over the sweep of tests/fp8_inputs_cases.py, rows seeing < 256 keys and the rest, beside the 16-bit
extended forward on the dequantised tensors, and the kernel / baseline error ratio of every case.
`--varlen`: the packed and the paged form (flash_attention_fp8_varlen / fa_fp8_forward_varlen, section 9y) — uniform lengths against
the padded call on the same tokens with that call's round-to-round spread, chunked prefill over an e4m3 paged cache against the
widening 16-bit call of section 9n, and a ragged batch against the uniform one of the same total."""
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
ap.add_argument("--varlen", action="store_true", help="the packed and the paged form (flash_attention_fp8_varlen, DESIGN.md section 9y)")
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


def varlen_problem(lens_q, lens_k, hq, hkv, seed):
    """packed e4m3 q, k, v of the sequences, their offsets and (B, H_kv) descales"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda n, h: torch.randn((n, h, D), device="cuda", dtype=torch.bfloat16, generator=g).to(E4M3)   # noqa: E731
    q, k, v = mk(sum(lens_q), hq), mk(sum(lens_k), hkv), mk(sum(lens_k), hkv)
    cu = lambda lens: torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device="cuda")   # noqa: E731
    ds = [torch.full((len(lens_q), hkv), x, dtype=torch.float32, device="cuda") for x in (0.5, 0.75, 1.25)]
    return q, k, v, cu(lens_q), cu(lens_k), ds


def paged_from(k, v, lens_k, ps, seed):
    """the pools (num_blocks, ps, H_kv, d) and a shuffled table that hold the packed tokens"""
    need = [(n + ps - 1) // ps for n in lens_k]
    nblk, mblk = sum(need), max(need)
    perm = torch.randperm(nblk, generator=torch.Generator().manual_seed(seed))
    table = torch.zeros((len(lens_k), mblk), dtype=torch.int32)
    pk, pv = (torch.zeros((nblk, ps) + tuple(t.shape[1:]), dtype=torch.uint8, device="cuda") for t in (k, v))
    start, used = 0, 0
    for b, n in enumerate(lens_k):
        pages = perm[used:used + need[b]]
        table[b, :need[b]] = pages.to(torch.int32)
        for src, pool in ((k, pk), (v, pv)):
            pad = torch.zeros((need[b] * ps,) + tuple(src.shape[1:]), dtype=torch.uint8, device="cuda")
            pad[:n] = src[start:start + n].view(torch.uint8)
            pool[pages.cuda()] = pad.reshape(need[b], ps, *src.shape[1:])
        start, used = start + n, used + need[b]
    return pk.view(E4M3), pv.view(E4M3), table.cuda()


def varlen_flops(lens_q, lens_k, hq, causal):
    return sum(flops(1, hq, a, b, causal) for a, b in zip(lens_q, lens_k))


def varlen_rows():
    """the packed and the paged call against the padded call on the same tokens (uniform lengths), against the widening 16-bit prefill
    over an e4m3 paged cache (chunked prefill), and a ragged batch against the uniform one of the same total"""
    res = {}

    def uniform(b, h, n, causal, seed):
        lens = [n] * b
        q, k, v, cu_q, cu_k, ds = varlen_problem(lens, lens, h, h, seed)
        qp, kp, vp = (t.reshape(b, n, h, D) for t in (q, k, v))
        variants = {
            "padded": lambda: ext.fp8_forward(qp, kp, vp, causal, D ** -0.5, *ds, torch.bfloat16, "bnhd"),
            "packed": lambda: ext.fp8_varlen_forward(q, k, v, cu_q, cu_k, n, n, causal, D ** -0.5, *ds),
        }
        for ps in (16, 256):
            pk, pv, table = paged_from(k, v, lens, ps, seed)
            variants[f"paged_ps{ps}"] = (lambda pk=pk, pv=pv, table=table:
                                         ext.fp8_varlen_forward(q, pk, pv, cu_q, cu_k, n, n, causal, D ** -0.5, *ds, block_table=table))
        r = interleave(variants)
        base = r["padded"]
        for name, x in r.items():
            x["tflops"] = varlen_flops(lens, lens, h, causal) / x["median_ms"] / 1e9
            x["over_padded"] = x["median_ms"] / base["median_ms"]
        r["padded_spread"] = (base["max_ms"] - base["min_ms"]) / base["median_ms"]
        return r

    for n in (16384, 8192):
        for causal in (False, True):
            res[f"uniform_b2_h8_n{n}_{'causal' if causal else 'full'}"] = uniform(2, 8, n, causal, n + causal)
    # chunked prefill: 2048 new queries against 16384 cached keys, GQA 32 / 8, an e4m3 paged cache
    hq, hkv, nq, nk, ps = 32, 8, 2048, 16384, 256
    q, k, v, cu_q, cu_k, ds = varlen_problem([nq], [nk], hq, hkv, 5)
    pk, pv, table = paged_from(k, v, [nk], ps, 5)
    q16 = q.to(torch.bfloat16)
    r = interleave({
        "bf16_widening": lambda: ext.ex_varlen_forward(q16, pk, pv, cu_q, cu_k, nq, nk, True, D ** -0.5, block_table=table, k_descale=ds[1],
                                                       v_descale=ds[2]),
        "fp8_paged": lambda: ext.fp8_varlen_forward(q, pk, pv, cu_q, cu_k, nq, nk, True, D ** -0.5, *ds, block_table=table),
    })
    for x in r.values():
        x["tflops"] = flops(1, hq, nq, nk, True) / x["median_ms"] / 1e9
    r["speedup"] = r["bf16_widening"]["median_ms"] / r["fp8_paged"]["median_ms"]
    res["chunked_prefill_2048_16384_causal_gqa_32_8_ps256"] = r
    # a ragged batch: 8 sequences, the total of 8 x 4096, lengths drawn once
    b, h, n = 8, 2, 4096
    cuts = sorted(torch.randint(1, b * n // 64, (b - 1,), generator=torch.Generator().manual_seed(11)).mul(64).tolist())
    ragged = [hi - lo for lo, hi in zip([0] + cuts, cuts + [b * n])]
    for causal in (False, True):
        row = {}
        for name, lens in (("uniform", [n] * b), ("ragged", ragged)):
            q, k, v, cu_q, cu_k, ds = varlen_problem(lens, lens, h, h, 9)
            pk, pv, table = paged_from(k, v, lens, 256, 9)
            m = max(lens)
            row[name] = (lens, {
                f"{name}_packed": lambda q=q, k=k, v=v, cu_q=cu_q, cu_k=cu_k, ds=ds, m=m: ext.fp8_varlen_forward(q, k, v, cu_q, cu_k, m, m, causal, D ** -0.5, *ds),
                f"{name}_paged_ps256": lambda q=q, pk=pk, pv=pv, cu_q=cu_q, cu_k=cu_k, ds=ds, m=m, table=table:
                    ext.fp8_varlen_forward(q, pk, pv, cu_q, cu_k, m, m, causal, D ** -0.5, *ds, block_table=table),
            })
        r = interleave({**row["uniform"][1], **row["ragged"][1]})
        for name, x in r.items():
            lens = row[name.split("_")[0]][0]
            x["tflops"] = varlen_flops(lens, lens, h, causal) / x["median_ms"] / 1e9
            x["grid_tiles"] = b * h * ((max(lens) + 255) // 256)
            x["live_tiles"] = h * sum((n_ + 255) // 256 for n_ in lens)
        r["lengths"] = ragged
        res[f"ragged_b8_h2_total{b * n}_{'causal' if causal else 'full'}"] = r
    return res


out = accuracy_rows() if args.accuracy else varlen_rows() if args.varlen else time_rows()
print(json.dumps({"config": f"d={D}, median of {args.rounds} interleaved rounds x {CALLS} calls" if not args.accuracy else "sweep of tests/fp8_inputs_cases.py",
                  "results": out}, indent=1))
