#!/usr/bin/env python3
"""Time a KV-cache decode step (flashattention_lab_cuda.ex_kvcache_forward) against the same decode through ex_forward.

    python tools/bench_kvcache.py [--d 128] [--dtype bf16] [--nq 1] [--page-size 16 --page-size 256] [--rotary] [--cache-dtype e4m3]
                                  [--json out.json]

Rows: B in {1, 8, 32}, H_q = 32, H_kv in {8, 32}, cache length in {1k, 8k, 32k, 128k}, plus one mixed-length batch.  The
largest row (B = 32, 128k keys, H_kv = 32) holds 68 GB of cache and as much again in ex_forward's layout; --max-tokens drops
rows with B * len above it on smaller devices.  Each row reports the median time per call of
  kv      : the new path without append (cache_seqlens = len),
  kv_app  : the new path appending one token (cache_seqlens = len - 1),
  ex      : ex_forward with GQA on (B * H_q, 1, d) q and (B * H_kv, len, d) K/V (the layout it needs, copied once outside the timing),
  paged_<ps> (one per --page-size): the paged call without append over a pool that holds the same tokens, its pages assigned to
            the sequences in shuffled order (block_table; flashattention_lab_cuda.ex_kvcache_forward(..., block_table=...)),
  kv_app_rot, unfused_rot (--rotary): kv_app with rotary_cos / rotary_sin (rotary_dim = d, not interleaved), the rotation of q and
            of the new key fused into the call; and the same step with q and k_new rotated by torch elementwise ops on the device
            in front of kv_app (checked against the fused call before it is timed),
and the effective bandwidth of kv: bytes of K and V read (sum over b of len_b * H_kv * d * 2 * 2) / time, against 6.3 TB/s.
--cache-dtype e4m3: the caches (and pools) are quantised once, outside the timed region, to torch.float8_e4m3fn with scales
absmax / 448 per (b, head), and every kv / kv_app / paged / rotary call runs on them with k_descale / v_descale; the bytes of K
and V are then 1 an element.  ex_forward and the unfused rotation keep the 16-bit tensors.
--varlen: instead of the grid, the packed call (cu_seqlens_q) on an 8k-key paged cache (page 16), H_q = 32, H_kv = 8:
  uniform : B = 32 sequences of --nq tokens through cu_seqlens_q against the padded call on the same tensors (the same kernels:
            the ratio should be 1), parent-comparable;
  mixed   : 63 sequences of 1 token and one chunk of n tokens (--chunks, default 16 .. 512) in one packed call, against the two
            padded calls that serve the same step (63 x 1 token, 1 x n tokens), with the share of the packed grid's waves that
            leave empty, 1 - sum_b ceil(nq_b G / 16) / (B ceil(max_seqlen_q G / 16)); and the chunk alone through
            ex_varlen_forward on its gathered keys (the gather timed apart), the call that overtakes this path on long chunks.
--prefill: one prefill chunk of n new tokens (--prefill-chunks, default 16, 64, 128, 512, 2048) against a paged cache (page 16) of
  8k and 32k tokens (--prefill-lens), H_q = 32, H_kv = 8 (G = 4), causal, the chunk's own keys being the cache's last n, three ways:
  (a) decode_us        : the packed decode call (ex_kvcache_forward with cu_seqlens_q), which re-reads the keys ceil(n G / 16) times,
  (b) paged_varlen_us  : ex_varlen_forward(..., block_table=), the prefill kernel reading the pool through the table,
  (c) gather_varlen_us : the pages gathered into packed k, v by torch indexing, then ex_varlen_forward (the gather alone: gather_us).
  and, on an e4m3 copy of the same tokens (one absmax scale per K/V head; k_descale, v_descale):
  (a8) decode_e4m3_us       : the packed decode call on the e4m3 pools, the only route to an e4m3 cache before (b8) existed,
  (b8) paged_varlen_e4m3_us : ex_varlen_forward(..., block_table=, k_descale=, v_descale=), the prefill kernel on the e4m3 pools
  ((b) itself is the 16-bit context for (b8): the same tokens on the same kernel without the widening pass).
  All are timed in turn, --rounds times over, so that clock and cache state drift hits all alike; each figure is the median
  of the rounds (each round itself the median of --reps groups).  (b) is checked to be bitwise (c) before anything is timed.
  --parent-check: only the packed ex_varlen_forward without a table at B H = 64, 4096 tokens, d = 128 (B = 2 sequences of 4096,
  32 heads, causal): the figure to compare between two checkouts, with the spread of its rounds.
--mla: the call with a second query operand (qv=; q, k_cache 64 wide, qv, v_cache, o 512 wide) at (B, H_q, H_kv, Nq, len) =
  (32, 128, 1, 1, 8192), (32, 16, 1, 1, 8192), (4, 128, 1, 2, 32768), bf16, the two caches as the slices of one (.., 576) pool,
  contiguous and paged (page 64, shuffled; checked bitwise against the contiguous call first): the median time over --rounds
  rounds with their spread, the split count the launch rule takes, and the cache bytes read per second with the cache counted
  once per sequence, B * len * 576 * 2.  In the same run, the plain split kernel at d = 256, H_q / H_kv = 8 on a cache of the same
  B and len (its bytes: B * len * H_kv * 256 * 2 * 2), from the unchanged code path.
--mla-sparse: the sparse call (ex_mla_sparse_forward: topk = 2048 listed tokens per query token) at (B, H_q, Nq) = (32, 128, 1),
  (32, 16, 1), (1, 128, 512) (a prefill chunk), H_kv = 1, bf16, over caches of len 8192 and 65536 (the two slices of one
  (.., 576) pool), contiguous and paged (page 64, shuffled; checked bitwise against the contiguous call first), with uniformly
  random lists and with the same lists sorted.  The yardstick, in the same run: the dense qv call on a cache of len = topk (the
  same number of keys and the same matrix work, every row read in order), and that call through a page table (page 64, pages
  in order), whose copy path the sparse kernel shares.  Per figure the median over --rounds rounds with their
  spread, the ratio to the dense call, and the listed bytes gathered per second, B * Nq * topk * 576 * 2 (a list counted once: at
  H_q = 128 two workgroups gather it).
--mla-fp8: the packed 8-bit latent cache (ex_mla_fp8_forward: 656-byte tokens, 512 e4m3 + 4 scales + 64 bf16) against the 16-bit
  paged call on the same tokens through the same table (page 64, shuffled), in the same run: --mla's three rows, and --mla-sparse's
  (32, 128, 1) row at len 8192 with random lists; per figure the median over --rounds rounds with their spread, the bytes of the
  tokens read per second in each format, and the ratio packed / 16-bit.  Then the append (ex_mla_fp8_pack) of 1, 512 and 8192 new
  tokens to each of 32 sequences, with and without power-of-two scales, against the bytes it moves (1152 read + 656 written a
  token): eager calls, and the same calls replayed from one captured graph (without the wrapper and the launch path).
`--fp8-q`: fp8 KV-cache decoding (fp8_kvcache_forward: e4m3 q on the e4m3 matrix instruction) against the yardstick, the e4m3-cache
  call with a 16-bit q on the same cache, interleaved in one process: B 32 / H 32:8 / L 8192 / Nq 1, B 1 / L 65536, B 8 / Nq 4 causal /
  L 4096, each contiguous and paged with ps 16 and 256.  Per row the median of `--rounds` (at least 5) interleaved rounds of both
  calls, the yardstick's own spread over its rounds, and the cache bytes moved over the time against the copy rate.
Timing: HIP events around `--iters` back-to-back calls after `--warmup` calls; the median of `--reps` such groups.
`--fp8-mod`: the featured fp8 decode call (a window, a softcap, sinks: DESIGN.md section 9zc) at B 32, H_q 32, H_kv 8, Nq 1, interleaved
rounds: a causal window of 1023 over 32768 cached keys against its floor (the unwindowed fp8 call over a 1024-key cache: the same
visible keys) and against the 16-bit-q call with the same window on the same e4m3 cache; then the cost of a softcap and of sinks on the
unwindowed 32768-key row.
`--fp8-step`: the fp8 decode step (fp8_kvcache_step: append, rotary-free q quantise and attention in one call)
at B 1 and 32, H 32:8, Nq = N_new = 1 over 8192 cached keys, contiguous and paged (ps 16), interleaved rounds: the step; its parent,
fp8_kvcache_forward alone on the pre-filled cache (the difference is the prep launch); what gives the same effect without the step,
the e4m3-cache call with a 16-bit q and the append; and the prep launch by its own profile scope against the bytes it moves.
`--md PATH` writes the table as markdown.
`--fp8-varlen`: packed queries on the fp8 decode call and the step, H 32:8, 8192 cached keys, contiguous e4m3
caches, interleaved rounds, three row kinds: `uniform`, the packed call on B = 32 sequences of Nq = 1 and of Nq = 4 tokens against
the padded call on the same tokens (d = 128); `mixed`, one step of 63 one-token sequences plus one chunk of 128 tokens, as one packed
fp8 step (num_splits by the rule, and 8) against the two padded fp8 steps that serve it today (d = 128); `step_hdim`, the fused step at d = 64 and 256 (B = 32, Nq =
N_new = 1) against the three calls that served these widths: the e4m3-cache call with a 16-bit q and k=, v= (the only append there
was; its own attention comes with it), quantize_fp8 on q, the fp8 decode call."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-pytorch_amd"))
import flashattention_lab_cuda as ext  # noqa: E402

COPY_RATE = 6.3e12


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


def quantise(x):
    """(e4m3 tensor, float32 (B, H_kv) scales) of a (B, N, H_kv, d) 16-bit tensor: scale = absmax / 448 per (b, head); one batch
    element at a time, so the fp32 copy stays small"""
    out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty((x.shape[0], x.shape[2]), dtype=torch.float32, device=x.device)
    for bb in range(x.shape[0]):
        xf = x[bb].float()
        sc = (xf.abs().amax(dim=(0, 2)) / 448.0).clamp_min(2.0 ** -20)
        out[bb] = (xf * (1.0 / sc).view(1, -1, 1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        scales[bb] = sc
    return out, scales


def row(b, hq, hkv, lens, d, dtype, args):
    cap = max(lens)
    dev = "cuda"
    q = torch.randn((b, args.nq, hq, d), device=dev, dtype=dtype)
    kc = torch.randn((b, cap, hkv, d), device=dev, dtype=dtype)   # (generated in the 16-bit dtype: B = 32 x 128k x 32 heads is 34 GB)
    vc = torch.randn((b, cap, hkv, d), device=dev, dtype=dtype)
    kn = torch.randn((b, 1, hkv, d), device=dev, dtype=dtype)
    vn = torch.randn((b, 1, hkv, d), device=dev, dtype=dtype)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    sl1 = sl - 1
    kc16, vc16, dsc = kc, vc, {}
    if args.cache_dtype == "e4m3":
        (kc, kd), (vc, vd) = quantise(kc16), quantise(vc16)
        dsc = dict(k_descale=kd, v_descale=vd)
        if len(set(lens)) != 1 or args.no_ex:
            del kc16, vc16
            kc16 = vc16 = None
    t_kv = timed(lambda: ext.ex_kvcache_forward(q, kc, vc, None, None, sl, True, None, **dsc), args.warmup, args.iters, args.reps)
    t_app = timed(lambda: ext.ex_kvcache_forward(q, kc, vc, kn, vn, sl1, True, None, **dsc), args.warmup, args.iters, args.reps)
    snk = {}
    if args.sinks:   # the call with sinks (always through the combine) against the call without, alternated twice
        sinks = torch.randn((hq,), device=dev)
        with_s = lambda: ext.ex_kvcache_forward(q, kc, vc, None, None, sl, True, None, sinks=sinks, **dsc)   # noqa: E731
        without = lambda: ext.ex_kvcache_forward(q, kc, vc, None, None, sl, True, None, **dsc)              # noqa: E731
        ts = [timed(with_s, args.warmup, args.iters, args.reps), timed(without, args.warmup, args.iters, args.reps),
              timed(with_s, args.warmup, args.iters, args.reps), timed(without, args.warmup, args.iters, args.reps)]
        snk = dict(kv_sinks_us=[round(ts[0], 2), round(ts[2], 2)], kv_again_us=[round(ts[1], 2), round(ts[3], 2)],
                   sinks_vs_kv=round((ts[0] + ts[2]) / (ts[1] + ts[3]), 3), sinks_extra_us=round((ts[0] + ts[2] - ts[1] - ts[3]) / 2, 2))
    rot = {}
    if args.rotary:
        half = d // 2
        inv = 10000.0 ** (-torch.arange(0, d, 2, dtype=torch.float64, device=dev) / d)
        ang = torch.arange(cap + max(0, args.nq - 1), dtype=torch.float64, device=dev).view(-1, 1) * inv
        cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
        qi = torch.arange(args.nq, device=dev)

        def rotate(x, pos):   # x (B, N, H, d), pos (B, N): GPT-NeoX pairs (j, j + d / 2), fp32, one rounding
            c, s_ = cos[pos].float().unsqueeze(2), sin[pos].float().unsqueeze(2)
            x1, x2 = x[..., :half].float(), x[..., half:].float()
            return torch.cat((x1 * c - x2 * s_, x1 * s_ + x2 * c), -1).to(dtype)

        def unfused():
            pos = sl1.long().view(-1, 1)
            return ext.ex_kvcache_forward(rotate(q, pos + qi), kc, vc, rotate(kn, pos), vn, sl1, True, None, **dsc)

        def fused():
            return ext.ex_kvcache_forward(q, kc, vc, kn, vn, sl1, True, None, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False,
                                          **dsc)

        torch.testing.assert_close(fused()[0].float(), unfused()[0].float(), rtol=2e-2, atol=2e-2)
        rot = dict(kv_app_rot_us=round(timed(fused, args.warmup, args.iters, args.reps), 2),
                   unfused_rot_us=round(timed(unfused, args.warmup, args.iters, args.reps), 2))
        del cos, sin, ang
    paged = {}
    for ps in args.page_size:
        mb = (cap + ps - 1) // ps
        g = torch.Generator(device="cpu").manual_seed(ps)
        table = torch.randperm(b * mb, generator=g).view(b, mb).to(torch.int32).to(dev)
        kp = torch.empty((b * mb, ps, hkv, d), device=dev, dtype=kc.dtype)
        vp = torch.empty((b * mb, ps, hkv, d), device=dev, dtype=vc.dtype)
        pad = mb * ps - cap
        for bb in range(b):   # the same tokens, page by page (the tail of a last partial page is never read)
            rows = table[bb].long()
            kp.view(torch.uint8 if dsc else dtype)[rows] = torch.nn.functional.pad(
                kc[bb].view(torch.uint8 if dsc else dtype), (0, 0, 0, 0, 0, pad)).view(mb, ps, hkv, d)
            vp.view(torch.uint8 if dsc else dtype)[rows] = torch.nn.functional.pad(
                vc[bb].view(torch.uint8 if dsc else dtype), (0, 0, 0, 0, 0, pad)).view(mb, ps, hkv, d)
        o_c = ext.ex_kvcache_forward(q, kc, vc, None, None, sl, True, None, **dsc)[0]
        o_p = ext.ex_kvcache_forward(q, kp, vp, None, None, sl, True, None, block_table=table, **dsc)[0]
        assert torch.equal(o_c, o_p), "paged and contiguous calls disagree"
        paged[ps] = timed(lambda: ext.ex_kvcache_forward(q, kp, vp, None, None, sl, True, None, block_table=table, **dsc),
                          args.warmup, args.iters, args.reps)
        del kp, vp, table
    t_ex = None
    if len(set(lens)) == 1 and not args.no_ex:
        q3 = q.permute(0, 2, 1, 3).reshape(b * hq, args.nq, d).contiguous()
        k3 = kc16.permute(0, 2, 1, 3).reshape(b * hkv, cap, d).contiguous()
        v3 = vc16.permute(0, 2, 1, 3).reshape(b * hkv, cap, d).contiguous()
        t_ex = timed(lambda: ext.ex_forward(q3, k3, v3, True, d ** -0.5), args.warmup, args.iters, args.reps)
        del q3, k3, v3
    kv_bytes = sum(lens) * hkv * d * 2 * (1 if dsc else 2)
    r = dict(cache_dtype=args.cache_dtype, B=b, Hq=hq, Hkv=hkv, len=lens[0] if len(set(lens)) == 1 else "mixed", lens=None if len(set(lens)) == 1 else lens,
             kv_us=round(t_kv, 2), kv_append_us=round(t_app, 2), ex_forward_us=None if t_ex is None else round(t_ex, 2),
             speedup=None if t_ex is None else round(t_ex / t_kv, 2), kv_TBps=round(kv_bytes / t_kv / 1e6, 3),
             frac_copy_rate=round(kv_bytes / t_kv / 1e6 / (COPY_RATE / 1e12), 3))
    r.update(rot)
    r.update(snk)
    for ps, t in paged.items():
        r[f"paged_{ps}_us"] = round(t, 2)
        r[f"paged_{ps}_TBps"] = round(kv_bytes / t / 1e6, 3)
        r[f"paged_{ps}_vs_kv"] = round(t / t_kv, 3)
    del q, kc, vc, kc16, vc16, kn, vn
    torch.cuda.empty_cache()
    return r


def varlen_rows(args, dtype):
    dev, hq, hkv, d, ps, cap = "cuda", 32, 8, args.d, 16, 8192
    g = hq // hkv
    rows = []

    def pool(b):
        mb = cap // ps
        table = torch.randperm(b * mb, generator=torch.Generator().manual_seed(b)).view(b, mb).to(torch.int32).to(dev)
        return torch.randn((b * mb, ps, hkv, d), device=dev, dtype=dtype), torch.randn((b * mb, ps, hkv, d), device=dev, dtype=dtype), table

    def cu(lens):
        return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)

    t = lambda fn: timed(fn, args.warmup, args.iters, args.reps)   # noqa: E731
    # uniform lengths: the packed call against the padded call on the same tensors, alternated twice
    b = 32
    kp, vp, table = pool(b)
    sl = torch.full((b,), cap, dtype=torch.int32, device=dev)
    q = torch.randn((b, args.nq, hq, d), device=dev, dtype=dtype)
    cu_q = cu([args.nq] * b)
    padded = lambda: ext.ex_kvcache_forward(q, kp, vp, None, None, sl, True, None, block_table=table)   # noqa: E731
    packed = lambda: ext.ex_kvcache_forward(q.view(b * args.nq, hq, d), kp, vp, None, None, sl, True, None, block_table=table,   # noqa: E731
                                            cu_seqlens_q=cu_q, max_seqlen_q=args.nq)
    assert torch.equal(padded()[0].view(b * args.nq, hq, d), packed()[0]), "packed and padded calls disagree"
    ts = [t(packed), t(padded), t(packed), t(padded)]
    rows.append(dict(kind="uniform", B=b, nq=args.nq, len=cap, packed_us=[round(ts[0], 2), round(ts[2], 2)],
                     padded_us=[round(ts[1], 2), round(ts[3], 2)], packed_vs_padded=round((ts[0] + ts[2]) / (ts[1] + ts[3]), 3)))
    print(json.dumps(rows[-1]), flush=True)
    del kp, vp, table, q
    # a mixed step: 63 decoding sequences and one prefill chunk
    b = 64
    kp, vp, table = pool(b)
    for n in args.chunks:
        lens = [1] * 63 + [n]
        sl = torch.full((b,), cap, dtype=torch.int32, device=dev)   # (the chunk's own keys are the cache's last n: no append is timed)
        q = torch.randn((63 + n, hq, d), device=dev, dtype=dtype)
        cu_q = cu(lens)
        q1, qn = q[:63].view(63, 1, hq, d), q[63:].view(1, n, hq, d)
        packed = lambda: ext.ex_kvcache_forward(q, kp, vp, None, None, sl, True, None, block_table=table, cu_seqlens_q=cu_q,   # noqa: E731
                                                max_seqlen_q=n)

        def two():
            ext.ex_kvcache_forward(q1, kp, vp, None, None, sl[:63], True, None, block_table=table[:63])
            return ext.ex_kvcache_forward(qn, kp, vp, None, None, sl[63:], True, None, block_table=table[63:])

        torch.testing.assert_close(packed()[0][63:].float(), two()[0][0].float(), rtol=2e-2, atol=2e-2)
        # the chunk through the training path: its keys gathered from the pool, then one packed sequence
        gather = lambda: (kp[table[63].long()].view(cap, hkv, d), vp[table[63].long()].view(cap, hkv, d))   # noqa: E731
        kg, vg = gather()
        cq, ck = cu([n]), cu([cap])
        vl = lambda: ext.ex_varlen_forward(qn[0], kg, vg, cq, ck, n, cap, True, d ** -0.5)   # noqa: E731
        torch.testing.assert_close(vl()[0].float(), two()[0][0].float(), rtol=2e-2, atol=2e-2)
        tiles = (n * g + 15) // 16
        live = sum((x * g + 15) // 16 for x in lens)
        r = dict(kind="mixed", B=b, chunk=n, len=cap, packed_us=round(t(packed), 2), two_padded_us=round(t(two), 2),
                 chunk_varlen_us=round(t(vl), 2), gather_us=round(t(gather), 2), empty_wave_share=round(1 - live / (b * tiles), 4))
        r["packed_vs_two"] = round(r["packed_us"] / r["two_padded_us"], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del q, kg, vg
    return rows


def prefill_rows(args, dtype):
    dev, hq, hkv, d, ps = "cuda", 32, 8, args.d, 16
    rows = []
    t = lambda fn: timed(fn, args.warmup, args.iters, args.reps)   # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)   # noqa: E731
    for cap in args.prefill_lens:
        mb = cap // ps
        nblk = mb + 64
        table = torch.randperm(nblk, generator=torch.Generator().manual_seed(cap))[:mb].view(1, mb).to(torch.int32).to(dev)
        kp = torch.randn((nblk, ps, hkv, d), device=dev, dtype=dtype)
        vp = torch.randn((nblk, ps, hkv, d), device=dev, dtype=dtype)
        sl = i32([cap])
        # the same tokens as e4m3 pools: one scale per K/V head over the whole pool, the (H_kv,) form
        kd = (kp.float().abs().amax(dim=(0, 1, 3)) / 448.0).clamp_min(2.0 ** -20)
        vd = (vp.float().abs().amax(dim=(0, 1, 3)) / 448.0).clamp_min(2.0 ** -20)
        kp8 = (kp.float() / kd.view(1, 1, -1, 1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        vp8 = (vp.float() / vd.view(1, 1, -1, 1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        for n in args.prefill_chunks:
            q = torch.randn((n, hq, d), device=dev, dtype=dtype)
            cq, ck = i32([0, n]), i32([0, cap])
            decode = lambda: ext.ex_kvcache_forward(q, kp, vp, None, None, sl, True, None, block_table=table, cu_seqlens_q=cq,   # noqa: E731
                                                    max_seqlen_q=n)
            paged = lambda: ext.ex_varlen_forward(q, kp, vp, cq, ck, n, cap, True, d ** -0.5, block_table=table)   # noqa: E731
            gather = lambda: (kp[table[0].long()].view(cap, hkv, d), vp[table[0].long()].view(cap, hkv, d))   # noqa: E731

            def gathered():
                kg, vg = gather()
                return ext.ex_varlen_forward(q, kg, vg, cq, ck, n, cap, True, d ** -0.5)

            ob, oc = paged(), gathered()
            assert torch.equal(ob[0], oc[0]) and torch.equal(ob[1], oc[1]), "the paged call and the gathered call disagree"
            torch.testing.assert_close(decode()[0].float(), ob[0].float(), rtol=2e-2, atol=2e-2)
            decode8 = lambda: ext.ex_kvcache_forward(q, kp8, vp8, None, None, sl, True, None, block_table=table, cu_seqlens_q=cq,   # noqa: E731
                                                     max_seqlen_q=n, k_descale=kd, v_descale=vd)
            paged8 = lambda: ext.ex_varlen_forward(q, kp8, vp8, cq, ck, n, cap, True, d ** -0.5, block_table=table, k_descale=kd,   # noqa: E731
                                                   v_descale=vd)
            torch.testing.assert_close(paged8()[0].float(), decode8()[0].float(), rtol=2e-2, atol=2e-2)
            ta, tb, tc, tg, ta8, tb8 = [], [], [], [], [], []
            for _ in range(args.rounds):
                ta.append(t(decode))
                tb.append(t(paged))
                tc.append(t(gathered))
                tg.append(t(gather))
                ta8.append(t(decode8))
                tb8.append(t(paged8))
            med = statistics.median
            r = dict(kind="prefill", len=cap, chunk=n, decode_us=round(med(ta), 2), paged_varlen_us=round(med(tb), 2),
                     gather_varlen_us=round(med(tc), 2), gather_us=round(med(tg), 2), decode_reads=(n * (hq // hkv) + 15) // 16,
                     varlen_reads=(n + 255) // 256, paged_vs_decode=round(med(tb) / med(ta), 3),
                     paged_vs_gathered=round(med(tb) / med(tc), 3), rounds=dict(decode=[round(x, 2) for x in ta], paged=[round(x, 2) for x in tb],
                                                                             gathered=[round(x, 2) for x in tc]))
            r.update(decode_e4m3_us=round(med(ta8), 2), paged_varlen_e4m3_us=round(med(tb8), 2),
                     paged_e4m3_vs_decode_e4m3=round(med(tb8) / med(ta8), 3), paged_e4m3_vs_paged=round(med(tb8) / med(tb), 3))
            r["rounds"].update(decode_e4m3=[round(x, 2) for x in ta8], paged_e4m3=[round(x, 2) for x in tb8])
            rows.append(r)
            print(json.dumps(r), flush=True)
        del kp, vp, kp8, vp8
    return rows


def mla_rows(args):
    dev, dtype, d, dv, ps = "cuda", torch.bfloat16, 64, 512, 64
    rows = []
    t = lambda fn: [timed(fn, args.warmup, args.iters, args.reps) for _ in range(args.rounds)]   # noqa: E731
    med = statistics.median

    def figures(ts, nbytes):
        return dict(us=round(med(ts), 2), rounds=[round(x, 2) for x in ts], spread=round((max(ts) - min(ts)) / med(ts), 4),
                    TBps=round(nbytes / med(ts) / 1e6, 3))

    for b, hq, hkv, nq, L in ((32, 128, 1, 1, 8192), (32, 16, 1, 1, 8192), (4, 128, 1, 2, 32768)):
        q = torch.randn((b, nq, hq, d), device=dev, dtype=dtype)
        qv = torch.randn((b, nq, hq, dv), device=dev, dtype=dtype)
        pool = torch.randn((b, L, hkv, d + dv), device=dev, dtype=dtype)
        sl = torch.full((b,), L, dtype=torch.int32, device=dev)
        kc, vc = pool[..., dv:], pool[..., :dv]
        mb = L // ps
        table = torch.randperm(b * mb, generator=torch.Generator().manual_seed(b)).view(b, mb).to(torch.int32).to(dev)
        ppool = torch.empty((b * mb, ps, hkv, d + dv), device=dev, dtype=dtype)
        for bb in range(b):
            ppool[table[bb].long()] = pool[bb].view(mb, ps, hkv, d + dv)
        kp, vp = ppool[..., dv:], ppool[..., :dv]
        cont = lambda: ext.ex_kvcache_forward(q, kc, vc, None, None, sl, True, None, qv=qv)                       # noqa: E731
        paged = lambda: ext.ex_kvcache_forward(q, kp, vp, None, None, sl, True, None, block_table=table, qv=qv)   # noqa: E731
        oc, op = cont(), paged()
        assert torch.equal(oc[0], op[0]) and torch.equal(oc[1], op[1]), "paged and contiguous calls disagree"
        nbytes = b * L * (d + dv) * 2
        splits = next((s_ for s_ in range(2, 257) if ext._lib.fa_ex_kvcache_workspace_bytes_qv(b, hq, hkv, b * nq, nq, L, d, s_, 0, dv) ==
                       ext._lib.fa_ex_kvcache_workspace_bytes_qv(b, hq, hkv, b * nq, nq, L, d, 0, 0, dv)), 1)
        r = dict(kind="mla", B=b, Hq=hq, Hkv=hkv, nq=nq, len=L, splits=splits, cache_bytes=nbytes, contiguous=figures(t(cont), nbytes),
                 paged_64=figures(t(paged), nbytes))
        del pool, ppool, kc, vc, kp, vp
        # the plain split kernel on a cache of the same B and len: d = 256, H_q / H_kv = 8
        hq2, hkv2, d2 = 8, 1, 256
        q2 = torch.randn((b, nq, hq2, d2), device=dev, dtype=dtype)
        k2 = torch.randn((b, L, hkv2, d2), device=dev, dtype=dtype)
        v2 = torch.randn((b, L, hkv2, d2), device=dev, dtype=dtype)
        plain = lambda: ext.ex_kvcache_forward(q2, k2, v2, None, None, sl, True, None)   # noqa: E731
        r["plain_d256_g8"] = figures(t(plain), b * L * hkv2 * d2 * 2 * 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del q2, k2, v2
        torch.cuda.empty_cache()
    return rows


def mla_sparse_rows(args):
    dev, dtype, d, dv, ps, topk, hkv = "cuda", torch.bfloat16, 64, 512, 64, 2048, 1
    rows = []
    t = lambda fn: [timed(fn, args.warmup, args.iters, args.reps) for _ in range(args.rounds)]   # noqa: E731
    med = statistics.median

    def figures(ts, nbytes, base=None):
        f = dict(us=round(med(ts), 2), rounds=[round(x, 2) for x in ts], spread=round((max(ts) - min(ts)) / med(ts), 4),
                 TBps=round(nbytes / med(ts) / 1e6, 3))
        if base is not None:
            f["vs_dense"] = round(med(ts) / base, 3)
        return f

    def splits_of(query, *a):
        return next((s_ for s_ in range(2, 257) if query(*a[:-1], s_, *a[-1]) == query(*a[:-1], 0, *a[-1])), 1)

    for b, hq, nq in ((32, 128, 1), (32, 16, 1), (1, 128, 512)):
        q = torch.randn((b, nq, hq, d), device=dev, dtype=dtype)
        qv = torch.randn((b, nq, hq, dv), device=dev, dtype=dtype)
        # the yardstick: the dense call over topk keys (no causal cut: every row sees them all)
        dpool = torch.randn((b, topk, hkv, d + dv), device=dev, dtype=dtype)
        dense = lambda: ext.ex_kvcache_forward(q, dpool[..., dv:], dpool[..., :dv], None, None, topk, False, None, qv=qv)   # noqa: E731
        gathered = b * nq * hkv * topk * (d + dv) * 2
        td = t(dense)
        base = med(td)
        # the same keys through the dense call's paged copy (page 64, in order): the copy path the sparse kernel derives from
        dtable = torch.arange(b * topk // ps, dtype=torch.int32, device=dev).view(b, topk // ps)
        dpp = dpool.view(b * topk // ps, ps, hkv, d + dv)
        dense_paged = lambda: ext.ex_kvcache_forward(q, dpp[..., dv:], dpp[..., :dv], None, None, topk, False, None, block_table=dtable, qv=qv)   # noqa: E731
        tdp = t(dense_paged)
        dsplits = splits_of(ext._lib.fa_ex_kvcache_workspace_bytes_qv, b, hq, hkv, b * nq, nq, topk, d, (0, dv))
        for L in (8192, 65536):
            pool = torch.randn((b, L, hkv, d + dv), device=dev, dtype=dtype)
            kc, vc = pool[..., dv:], pool[..., :dv]
            mb = L // ps
            table = torch.randperm(b * mb, generator=torch.Generator().manual_seed(b)).view(b, mb).to(torch.int32).to(dev)
            ppool = torch.empty((b * mb, ps, hkv, d + dv), device=dev, dtype=dtype)
            for bb in range(b):
                ppool[table[bb].long()] = pool[bb].view(mb, ps, hkv, d + dv)
            kp, vp = ppool[..., dv:], ppool[..., :dv]
            rnd = torch.randint(0, L, (b, nq, topk), device=dev, dtype=torch.int32)
            r = dict(kind="mla_sparse", B=b, Hq=hq, Hkv=hkv, nq=nq, len=L, topk=topk, cache_bytes=b * L * (d + dv) * 2, listed_bytes=gathered,
                     splits=splits_of(ext._lib.fa_mla_sparse_workspace_bytes, b, hq, hkv, nq, topk, ()),
                     dense_len_topk=dict(figures(td, b * topk * (d + dv) * 2), splits=dsplits),
                     dense_paged_64_len_topk=figures(tdp, b * topk * (d + dv) * 2, base))
            for order, ix in (("random", rnd), ("sorted", rnd.sort(dim=-1).values.contiguous())):
                cont = lambda: ext.ex_mla_sparse_forward(q, qv, kc, vc, ix, L)                           # noqa: E731
                paged = lambda: ext.ex_mla_sparse_forward(q, qv, kp, vp, ix, L, block_table=table)       # noqa: E731
                oc, op = cont(), paged()
                assert torch.equal(oc[0], op[0]) and torch.equal(oc[1], op[1]), "paged and contiguous calls disagree"
                r[order] = dict(contiguous=figures(t(cont), gathered, base), paged_64=figures(t(paged), gathered, base))
            rows.append(r)
            print(json.dumps(r), flush=True)
            del pool, ppool, kc, vc, kp, vp
            torch.cuda.empty_cache()
    return rows


def mla_fp8_rows(args):
    """--mla-fp8: the packed 8-bit latent cache (656-byte tokens) against the 16-bit paged call on the same tokens and table"""
    dev, dtype, d, dv, ps, hkv, tok8 = "cuda", torch.bfloat16, 64, 512, 64, 1, 656
    rows = []
    t = lambda fn: [timed(fn, args.warmup, args.iters, args.reps) for _ in range(args.rounds)]   # noqa: E731
    med = statistics.median

    def figures(ts, nbytes, base=None):
        f = dict(us=round(med(ts), 2), rounds=[round(x, 2) for x in ts], spread=round((max(ts) - min(ts)) / med(ts), 4),
                 TBps=round(nbytes / med(ts) / 1e6, 3))
        if base is not None:
            f["vs_16bit"] = round(med(ts) / base, 3)
        return f

    def pools(b, L):
        """a bf16 (b, L, 1, 576) cache, the same tokens paged (page 64, shuffled), and packed through the same table"""
        pool = torch.randn((b, L, hkv, dv + d), device=dev, dtype=dtype)
        mb = L // ps
        table = torch.randperm(b * mb, generator=torch.Generator().manual_seed(b)).view(b, mb).to(torch.int32).to(dev)
        p16 = torch.empty((b * mb, ps, hkv, dv + d), device=dev, dtype=dtype)
        for bb in range(b):
            p16[table[bb].long()] = pool[bb].view(mb, ps, hkv, dv + d)
        p8 = torch.zeros((b * mb, ps, hkv, tok8), device=dev, dtype=torch.uint8)
        ext.ex_mla_fp8_pack(pool[:, :, 0, :dv], pool[:, :, 0, dv:], p8, 0, table)
        return pool, p16, p8, table

    for b, hq, nq, L, topk in ((32, 128, 1, 8192, 0), (32, 16, 1, 8192, 0), (4, 128, 2, 32768, 0), (32, 128, 1, 8192, 2048)):
        q = torch.randn((b, nq, hq, dv + d), device=dev, dtype=dtype)
        qr, ql = q[..., dv:], q[..., :dv]               # the packed call takes the views; the 16-bit calls get their own copies
        qr16, ql16 = qr.contiguous(), ql.contiguous()
        pool, p16, p8, table = pools(b, L)
        del pool
        sl = torch.full((b,), L, dtype=torch.int32, device=dev)
        if topk:
            ix = torch.randint(0, L, (b, nq, topk), device=dev, dtype=torch.int32)
            ref16 = lambda: ext.ex_mla_sparse_forward(qr16, ql16, p16[..., dv:], p16[..., :dv], ix, sl, False, None, table)   # noqa: E731
            packed = lambda: ext.ex_mla_fp8_forward(qr, ql, p8, table, sl, ix)                                            # noqa: E731
            tokens = b * nq * topk
        else:
            ref16 = lambda: ext.ex_kvcache_forward(qr16, p16[..., dv:], p16[..., :dv], None, None, sl, True, None, block_table=table, qv=ql16)   # noqa: E731
            packed = lambda: ext.ex_mla_fp8_forward(qr, ql, p8, table, sl, None, True)                                    # noqa: E731
            tokens = b * L
        o16, o8 = ref16()[0].float(), packed()[0].float()
        assert torch.isfinite(o8).all() and (o8 - o16).abs().max() < 0.25, "the packed call is far from the 16-bit one"
        t16 = t(ref16)
        r = dict(kind="mla_fp8", B=b, Hq=hq, nq=nq, len=L, topk=topk, bytes_16bit=tokens * (d + dv) * 2, bytes_packed=tokens * tok8,
                 paged_64_16bit=figures(t16, tokens * (d + dv) * 2), paged_64_packed=figures(t(packed), tokens * tok8, med(t16)))
        rows.append(r)
        print(json.dumps(r), flush=True)
        del p16, p8
        torch.cuda.empty_cache()
    # the append: 32 sequences, 1, 512 and 8192 new tokens each, against the bytes it moves (576 * 2 read, 656 written a token).
    # Eager calls carry the wrapper and the launch (about 19 us); the same calls replayed from one captured graph do not
    b, L = 32, 8192
    mb = L // ps
    table = torch.randperm(b * mb, generator=torch.Generator().manual_seed(b)).view(b, mb).to(torch.int32).to(dev)
    p8 = torch.zeros((b * mb, ps, hkv, tok8), device=dev, dtype=torch.uint8)

    def graphed(fn):
        """us a call of args.iters calls captured once and replayed: median of args.reps replays, of args.rounds rounds"""
        fn()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
            for _ in range(args.iters):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        return [timed(graph.replay, args.warmup, 1, args.reps) / args.iters for _ in range(args.rounds)]

    for nnew in (1, 512, 8192):
        new = torch.randn((b, nnew, dv + d), device=dev, dtype=dtype)
        sl = torch.full((b,), min(4096, L - nnew), dtype=torch.int32, device=dev)
        for pow2 in (False, True):
            fn = lambda: ext.ex_mla_fp8_pack(new[..., :dv], new[..., dv:], p8, sl, table, pow2)   # noqa: E731
            moved = b * nnew * ((d + dv) * 2 + tok8)
            r = dict(kind="mla_fp8_pack", B=b, n_new=nnew, scale_pow2=pow2, bytes_moved=moved, pack=figures(t(fn), moved),
                     pack_graph=figures(graphed(fn), moved))
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def fp8q_rows(args, dtype):
    """--fp8-q: see the module docstring"""
    dev, rounds = "cuda", max(args.rounds, 5)
    rows = []
    for b, nq, L, causal in ((32, 1, 8192, False), (1, 1, 65536, False), (8, 4, 4096, True)):
        hq, hkv = 32, 8
        q16 = torch.randn((b, nq, hq, 128), device=dev, dtype=dtype)
        (kc, kd), (vc, vd) = (quantise(torch.randn((b, L, hkv, 128), device=dev, dtype=dtype)) for _ in range(2))
        q8 = q16.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        qd = torch.ones((b, hkv), dtype=torch.float32, device=dev)
        sl = torch.full((b,), L, dtype=torch.int32, device=dev)
        nbytes = 2 * b * L * hkv * 128
        for ps in (0, 16, 256):
            if ps:
                nblk = b * L // ps
                perm = torch.randperm(nblk, device=dev)
                table = perm.view(b, L // ps).to(torch.int32)
                kk, vv = torch.empty_like(kc).view(nblk, ps, hkv, 128), torch.empty_like(vc).view(nblk, ps, hkv, 128)
                kk[perm] = kc.view(nblk, ps, hkv, 128)
                vv[perm] = vc.view(nblk, ps, hkv, 128)
            else:
                table, kk, vv = None, kc, vc
            old = lambda: ext.ex_kvcache_forward(q16, kk, vv, None, None, sl, causal, None, block_table=table, k_descale=kd,   # noqa: E731
                                                 v_descale=vd)
            new = lambda: ext.fp8_kvcache_forward(q8, kk, vv, sl, table, None, qd, kd, vd, None, causal, 0, dtype)   # noqa: E731
            t_old, t_new = [], []
            for _ in range(rounds):
                t_old.append(timed(old, args.warmup, args.iters, 1))
                t_new.append(timed(new, args.warmup, args.iters, 1))
            m_old, m_new = statistics.median(t_old), statistics.median(t_new)
            rows.append(dict(b=b, nq=nq, L=L, causal=causal, page_size=ps, yardstick_us=round(m_old, 2), fp8q_us=round(m_new, 2),
                             ratio=round(m_new / m_old, 3), yardstick_spread=round((max(t_old) - min(t_old)) / m_old, 3),
                             fp8q_spread=round((max(t_new) - min(t_new)) / m_new, 3),
                             yardstick_TBps=round(nbytes / m_old / 1e6, 3), fp8q_TBps=round(nbytes / m_new / 1e6, 3),
                             fp8q_of_copy_rate=round(nbytes / m_new * 1e6 / COPY_RATE, 3)))
            print(json.dumps(rows[-1]), flush=True)
        del kc, vc
    return rows


def fp8_mod_rows(args, dtype):
    """--fp8-mod: see the module docstring"""
    dev, rounds = "cuda", max(args.rounds, 5)
    b, hq, hkv, L, w = 32, 32, 8, 32768, 1023
    q16 = torch.randn((b, 1, hq, 128), device=dev, dtype=dtype)
    (kc, kd), (vc, vd) = (quantise(torch.randn((b, L, hkv, 128), device=dev, dtype=dtype)) for _ in range(2))
    q8 = q16.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    qd = torch.ones((b, hkv), dtype=torch.float32, device=dev)
    sl, sl_short = (torch.full((b,), n, dtype=torch.int32, device=dev) for n in (L, w + 1))
    sinks = torch.randn((hq,), dtype=torch.float32, device=dev)
    ks, vs = kc[:, :w + 1].contiguous(), vc[:, :w + 1].contiguous()          # the floor: the same visible keys in a 1024-key cache
    fp8 = lambda k_, v_, s_, **kw: ext.fp8_kvcache_forward(q8, k_, v_, s_, None, None, qd, kd, vd, None, True, 0, dtype, **kw)   # noqa: E731
    variants = {
        "fp8_window_1023_of_32768": lambda: fp8(kc, vc, sl, window=(w, -1)),
        "fp8_floor_1024_keys": lambda: fp8(ks, vs, sl_short),
        "q16_window_1023_of_32768": lambda: ext.ex_kvcache_forward(q16, kc, vc, None, None, sl, True, None, window=(w, -1), k_descale=kd,
                                                                   v_descale=vd),
        "fp8_unwindowed_32768": lambda: fp8(kc, vc, sl),
        "fp8_unwindowed_32768_softcap": lambda: fp8(kc, vc, sl, softcap=30.0),
        "fp8_unwindowed_32768_sinks": lambda: fp8(kc, vc, sl, sinks=sinks),
    }
    ts = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            ts[n].append(timed(fn, args.warmup, args.iters, 1))
    rows = []
    for n, t in ts.items():
        m = statistics.median(t)
        rows.append(dict(kind="fp8_mod", b=b, hq=hq, hkv=hkv, variant=n, us=round(m, 2), spread=round((max(t) - min(t)) / m, 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def fp8_step_rows(args, dtype):
    """--fp8-step: see the module docstring"""
    dev, rounds = "cuda", max(args.rounds, 5)
    hq, hkv, L, cap = 32, 8, 8192, 8192 + 256
    rows = []
    for b in (1, 32):
        q16 = torch.randn((b, 1, hq, 128), device=dev, dtype=dtype)
        kn, vn = (torch.randn((b, 1, hkv, 128), device=dev, dtype=dtype) for _ in range(2))
        (kc, kd), (vc, vd) = (quantise(torch.randn((b, cap, hkv, 128), device=dev, dtype=dtype)) for _ in range(2))
        qd = torch.full((b, hkv), 2.0 ** -5, dtype=torch.float32, device=dev)
        q8 = (q16.float() * 32.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        sl, sl1 = (torch.full((b,), n, dtype=torch.int32, device=dev) for n in (L, L + 1))
        # the prep launch: q and the new tokens in, their codes and the lengths out
        prep_bytes = b * (hq * 128 * (2 + 1) + 2 * hkv * 128 * (2 + 1) + 8)
        for ps in (0, 16):
            if ps:
                nblk = b * cap // ps
                perm = torch.randperm(nblk, device=dev)
                table = perm.view(b, cap // ps).to(torch.int32)
                kk, vv = torch.empty_like(kc).view(nblk, ps, hkv, 128), torch.empty_like(vc).view(nblk, ps, hkv, 128)
                kk[perm] = kc.view(nblk, ps, hkv, 128)
                vv[perm] = vc.view(nblk, ps, hkv, 128)
            else:
                table, kk, vv = None, kc, vc
            variants = {
                "step": lambda: ext.fp8_kvcache_step(q16, kk, vv, kn, vn, sl, table, None, qd, kd, vd, None, False, 0, dtype),
                "parent_fp8_decode": lambda: ext.fp8_kvcache_forward(q8, kk, vv, sl1, table, None, qd, kd, vd, None, False, 0, dtype),
                "q16_call_with_append": lambda: ext.ex_kvcache_forward(q16, kk, vv, kn, vn, sl, False, None, block_table=table, k_descale=kd,
                                                                       v_descale=vd),
            }
            ts = {n: [] for n in variants}
            for _ in range(rounds):
                for n, fn in variants.items():
                    ts[n].append(timed(fn, args.warmup, args.iters, 1))
            # the same calls replayed from one captured graph each: the device's time without the wrapper and the launch path
            graphed = {}
            for n in ("step", "parent_fp8_decode"):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(args.iters):
                        variants[n]()
                graphed[n] = statistics.median([timed(gr.replay, 1, 1, 1) / args.iters for _ in range(rounds)])
            ext.profile_enable(True)
            for _ in range(args.iters):
                variants["step"]()
            torch.cuda.synchronize()
            count, ms = ext.profile_report().get("fp8kv_step_prep", (0, 0.0))
            ext.profile_enable(False)
            med = {n: statistics.median(t) for n, t in ts.items()}
            prep_us = ms * 1e3 / max(count, 1)
            rows.append(dict(kind="fp8_step", b=b, hq=hq, hkv=hkv, L=L, page_size=ps, step_us=round(med["step"], 2),
                             parent_us=round(med["parent_fp8_decode"], 2), step_minus_parent_us=round(med["step"] - med["parent_fp8_decode"], 2),
                             q16_append_us=round(med["q16_call_with_append"], 2), step_graph_us=round(graphed["step"], 2),
                             parent_graph_us=round(graphed["parent_fp8_decode"], 2),
                             spread={n: round((max(t) - min(t)) / med[n], 3) for n, t in ts.items()}, prep_kernel_us=round(prep_us, 2),
                             prep_bytes=prep_bytes, prep_floor_us=round(prep_bytes / COPY_RATE * 1e6, 4)))
            print(json.dumps(rows[-1]), flush=True)
        del kc, vc
    return rows


def fp8_step_markdown(rows, args):
    out = ["# The fp8 decode step: measured on an MI355X", "",
           f"`tools/bench_kvcache.py --fp8-step --dtype {args.dtype}`: H 32 / 8, Nq = N_new = 1, 8192 cached keys, num_splits by the rule; the median "
           f"of {max(args.rounds, 5)} interleaved rounds of {args.iters} back-to-back calls (microseconds a call, host path included); the prep "
           "kernel by its own profile scope (events on the stream, which cost about as much as the kernel); its floor is its bytes at the copy rate.  "
           "`graph`: the same calls replayed from one captured graph, the device's time without the wrapper and the launch path.", "",
           "| B | layout | step | fp8 decode alone | step - alone | 16-bit q call + append | step, graph | alone, graph | prep kernel | prep bytes | prep floor |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['b']} | {'ps ' + str(r['page_size']) if r['page_size'] else 'contiguous'} | {r['step_us']} | {r['parent_us']} | "
                   f"{r['step_minus_parent_us']} | {r['q16_append_us']} | {r['step_graph_us']} | {r['parent_graph_us']} | {r['prep_kernel_us']} | {r['prep_bytes']} | {r['prep_floor_us']} |")
    out += ["", "Spread of the rounds (max - min over the median): " +
            "; ".join(f"B {r['b']} {'ps16' if r['page_size'] else 'contig'} " + ", ".join(f"{k} {v}" for k, v in r["spread"].items()) for r in rows), ""]
    return "\n".join(out)


def fp8_varlen_rows(args, dtype):
    """--fp8-varlen: see the module docstring"""
    dev, rounds = "cuda", max(args.rounds, 5)
    hq, hkv, L, cap = 32, 8, 8192, 8192 + 256
    rows = []

    def measure(kind, variants, **what):
        ts = {n: [] for n in variants}
        for _ in range(rounds):
            for n, fn in variants.items():
                ts[n].append(timed(fn, args.warmup, args.iters, 1))
        med = {n: statistics.median(t) for n, t in ts.items()}
        rows.append(dict(kind=kind, hq=hq, hkv=hkv, L=L, **what, us={n: round(v, 2) for n, v in med.items()},
                         spread={n: round((max(t) - min(t)) / med[n], 3) for n, t in ts.items()}))
        print(json.dumps(rows[-1]), flush=True)

    def caches(b, d):
        (kc, kd), (vc, vd) = (quantise(torch.randn((b, cap, hkv, d), device=dev, dtype=dtype)) for _ in range(2))
        return kc, vc, kd, vd, torch.full((b, hkv), 2.0 ** -5, dtype=torch.float32, device=dev)

    def codes(x):
        return (x.float() * 32.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)

    # uniform lengths: the packed call against the padded call on the same tokens
    b, d = 32, 128
    kc, vc, kd, vd, qd = caches(b, d)
    sl = torch.full((b,), L, dtype=torch.int32, device=dev)
    for nq in (1, 4):
        q8 = codes(torch.randn((b, nq, hq, d), device=dev, dtype=dtype))
        qp = q8.view(b * nq, hq, d)
        cu = torch.arange(0, b * nq + 1, nq, dtype=torch.int32, device=dev)
        measure("uniform", {
            "padded": lambda: ext.fp8_kvcache_forward(q8, kc, vc, sl, None, None, qd, kd, vd, None, True, 0, dtype),
            "packed": lambda: ext.fp8_kvcache_forward(qp, kc, vc, sl, None, None, qd, kd, vd, None, True, 0, dtype, cu_seqlens_q=cu,
                                                      max_seqlen_q=nq)}, b=b, nq=nq, d=d)
    del kc, vc
    # the mixed step: 63 one-token decodes and one chunk of 128 tokens, one packed step against two padded steps
    b, chunk = 64, 128
    kc, vc, kd, vd, qd = caches(b, d)
    sl = torch.full((b,), L, dtype=torch.int32, device=dev)
    total = b - 1 + chunk
    q16, kn, vn = (torch.randn((total, h, d), device=dev, dtype=dtype) for h in (hq, hkv, hkv))
    cu = torch.tensor(list(range(b)) + [total], dtype=torch.int32, device=dev)
    idx1, idx2 = torch.arange(b - 1, dtype=torch.int32, device=dev), torch.full((1,), b - 1, dtype=torch.int32, device=dev)
    q1, k1, v1 = (t[:b - 1].view(b - 1, 1, -1, d) for t in (q16, kn, vn))
    q2, k2, v2 = (t[b - 1:].view(1, chunk, -1, d) for t in (q16, kn, vn))

    def two_padded():
        ext.fp8_kvcache_step(q1, kc, vc, k1, v1, sl[:b - 1], None, idx1, qd[:b - 1], kd[:b - 1], vd[:b - 1], None, True, 0, dtype)
        ext.fp8_kvcache_step(q2, kc, vc, k2, v2, sl[b - 1:], None, idx2, qd[b - 1:], kd[b - 1:], vd[b - 1:], None, True, 0, dtype)

    measure("mixed", {
        "two_padded_steps": two_padded,
        "one_packed_step": lambda: ext.fp8_kvcache_step(q16, kc, vc, kn, vn, sl, None, None, qd, kd, vd, None, True, 0, dtype, cu_seqlens_q=cu,
                                                        max_seqlen_q=chunk, cu_seqlens_k_new=cu),
        # the rule counts the dense grid (B x ceil(max_seqlen_q G / 32) row tiles, most of which leave at once) and gives one split here
        "one_packed_step_8_splits": lambda: ext.fp8_kvcache_step(q16, kc, vc, kn, vn, sl, None, None, qd, kd, vd, None, True, 8, dtype,
                                                                 cu_seqlens_q=cu, max_seqlen_q=chunk, cu_seqlens_k_new=cu)},
        b=b, chunk=chunk, d=d)
    del kc, vc
    # the fused step at 64 / 256 against the three calls that served these widths
    b = 32
    for d in (64, 256):
        kc, vc, kd, vd, qd = caches(b, d)
        sl, sl1 = (torch.full((b,), n, dtype=torch.int32, device=dev) for n in (L, L + 1))
        q16 = torch.randn((b, 1, hq, d), device=dev, dtype=dtype)
        kn, vn = (torch.randn((b, 1, hkv, d), device=dev, dtype=dtype) for _ in range(2))
        q8 = torch.empty((b, 1, hq, d), dtype=torch.float8_e4m3fn, device=dev)

        def chain():
            ext.ex_kvcache_forward(q16, kc, vc, kn, vn, sl, False, None, k_descale=kd, v_descale=vd)   # (the append's call)
            ext.fp8_quantize(q16, hq // hkv, qd, "bnhd", q8)
            ext.fp8_kvcache_forward(q8, kc, vc, sl1, None, None, qd, kd, vd, None, False, 0, dtype, hdim=True)

        measure("step_hdim", {
            "append_quantize_decode": chain,
            "fused_step": lambda: ext.fp8_kvcache_step(q16, kc, vc, kn, vn, sl, None, None, qd, kd, vd, None, False, 0, dtype, hdim=True)},
            b=b, nq=1, d=d)
        del kc, vc
    return rows


def parent_check(args, dtype):
    dev, b, h, n, d = "cuda", 2, 32, 4096, 128
    q, k, v = (torch.randn((b * n, h, d), device=dev, dtype=dtype) for _ in range(3))
    cu = torch.tensor([0, n, 2 * n], dtype=torch.int32, device=dev)
    fn = lambda: ext.ex_varlen_forward(q, k, v, cu, cu, n, n, True, d ** -0.5)   # noqa: E731
    ts = [timed(fn, args.warmup, args.iters, args.reps) for _ in range(max(args.rounds, 5))]
    r = dict(kind="parent_check", BH=b * h, n=n, d=d, varlen_fwd_us=round(statistics.median(ts), 2), rounds=[round(x, 2) for x in ts],
             spread=round((max(ts) - min(ts)) / statistics.median(ts), 4), version=ext.version())
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--nq", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-tokens", type=int, default=1 << 22, help="skip rows with B * len above this")
    ap.add_argument("--page-size", type=int, action="append", default=[], help="also time the paged call with this page size (repeatable)")
    ap.add_argument("--no-ex", action="store_true", help="skip the ex_forward column")
    ap.add_argument("--rotary", action="store_true", help="also time the append with fused rotary embedding, and with torch rotating first")
    ap.add_argument("--cache-dtype", default="16", choices=("16", "e4m3"),
                    help="16: the caches in --dtype; e4m3: quantised once to float8_e4m3fn with per-(b, head) scales")
    ap.add_argument("--sinks", action="store_true", help="also time the call with attention sinks ((H_q,) logits) against the call without")
    ap.add_argument("--lens", default="1024,8192,32768,131072", help="the grid's cache lengths")
    ap.add_argument("--varlen", action="store_true", help="time the packed call (cu_seqlens_q) instead of the grid: see the module docstring")
    ap.add_argument("--chunks", default="16,32,64,128,256,512", help="--varlen: the chunk lengths of the mixed step")
    ap.add_argument("--prefill", action="store_true", help="time one prefill chunk against a paged cache three ways: see the module docstring")
    ap.add_argument("--prefill-chunks", default="16,64,128,512,2048")
    ap.add_argument("--prefill-lens", default="8192,32768")
    ap.add_argument("--rounds", type=int, default=3, help="--prefill / --parent-check: interleaved rounds per figure")
    ap.add_argument("--parent-check", action="store_true", help="time only the packed varlen forward at B H = 64, 4096 tokens, d = 128")
    ap.add_argument("--mla", action="store_true", help="time the call with qv (64 + 512 head dims): see the module docstring")
    ap.add_argument("--mla-sparse", action="store_true", help="time the sparse MLA call against the dense qv call at equal keys: see the module docstring")
    ap.add_argument("--mla-fp8", action="store_true", help="time the packed 8-bit latent cache against the 16-bit paged call, and the append: see the module docstring")
    ap.add_argument("--fp8-q", action="store_true", help="time fp8 KV-cache decoding (e4m3 q) against the e4m3-cache call with a 16-bit q: see the module docstring")
    ap.add_argument("--fp8-mod", action="store_true", help="time the windowed fp8 decode call, its floor and the 16-bit-q call with the same window: see the module docstring")
    ap.add_argument("--fp8-step", action="store_true", help="time the fp8 decode step against its parent and the 16-bit-q call with the append: see the module docstring")
    ap.add_argument("--fp8-varlen", action="store_true", help="time the packed fp8 decode call and step, and the step at d 64 / 256: see the module docstring")
    ap.add_argument("--md", default=None, help="--fp8-step: write the table as markdown to this path")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    args.chunks = [int(x) for x in args.chunks.split(",")]
    args.prefill_chunks = [int(x) for x in args.prefill_chunks.split(",")]
    args.prefill_lens = [int(x) for x in args.prefill_lens.split(",")]
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    # bring the clocks up before the first row (a second of large decode steps)
    wq = torch.randn((8, 1, 32, args.d), device="cuda", dtype=dtype)
    wk = torch.randn((8, 32768, 8, args.d), device="cuda", dtype=dtype)
    wl = torch.full((8,), 32768, dtype=torch.int32, device="cuda")
    for _ in range(2000):
        ext.ex_kvcache_forward(wq, wk, wk, None, None, wl, True, None)
    torch.cuda.synchronize()
    del wq, wk
    if args.fp8_varlen:
        rows = fp8_varlen_rows(args, dtype)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(fp8_varlen=True, dtype=args.dtype, version=ext.version(), rows=rows), f, indent=1)
        return
    if args.fp8_step:
        rows = fp8_step_rows(args, dtype)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(fp8_step=True, dtype=args.dtype, version=ext.version(), copy_rate_TBps=COPY_RATE / 1e12, rows=rows), f, indent=1)
        if args.md:
            with open(args.md, "w") as f:
                f.write(fp8_step_markdown(rows, args))
        return
    if args.fp8_mod:
        rows = fp8_mod_rows(args, dtype)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(fp8_mod=True, dtype=args.dtype, version=ext.version(), rows=rows), f, indent=1)
        return
    if args.fp8_q:
        rows = fp8q_rows(args, dtype)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(fp8_q=True, dtype=args.dtype, version=ext.version(), copy_rate_TBps=COPY_RATE / 1e12, rows=rows), f, indent=1)
        return
    if args.mla_fp8:
        rows = mla_fp8_rows(args)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(mla_fp8=True, version=ext.version(), rows=rows), f, indent=1)
        return
    if args.mla or args.mla_sparse:
        rows = mla_sparse_rows(args) if args.mla_sparse else mla_rows(args)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(mla=True, sparse=bool(args.mla_sparse), version=ext.version(), rows=rows), f, indent=1)
        return
    if args.prefill or args.parent_check:
        rows = parent_check(args, dtype) if args.parent_check else prefill_rows(args, dtype)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(d=args.d, dtype=args.dtype, prefill=True, rows=rows), f, indent=1)
        return
    if args.varlen:
        rows = varlen_rows(args, dtype)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(d=args.d, dtype=args.dtype, nq=args.nq, varlen=True, rows=rows), f, indent=1)
        return
    rows = []
    for b in (1, 8, 32):
        for hkv in (8, 32):
            for L in (int(x) for x in args.lens.split(",")):
                if b * L > args.max_tokens:
                    continue
                rows.append(row(b, 32, hkv, [L] * b, args.d, dtype, args))
                print(json.dumps(rows[-1]), flush=True)
    g = torch.Generator().manual_seed(0)
    mixed = [int(x) for x in torch.randint(64, 32768, (8,), generator=g)]
    rows.append(row(8, 32, 8, mixed, args.d, dtype, args))
    print(json.dumps(rows[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(d=args.d, dtype=args.dtype, nq=args.nq, page_sizes=args.page_size, rotary=args.rotary, cache_dtype=args.cache_dtype,
                           copy_rate_TBps=COPY_RATE / 1e12, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
