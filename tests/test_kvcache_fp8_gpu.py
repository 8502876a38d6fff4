"""GPU: an e4m3 KV cache with per-(sequence, K/V head) scales in flash_attn_with_kvcache / fa_ex_forward_kvcache_fp8.  The cache
is quantised on the CPU by tests/kvcache_fp8_ref.quantize; the reference is fp64 attention over dequantize(cache) per batch
element with an explicit visibility mask (tests/kvcache_paged_ref.reference).  Tolerances are the 16-bit decode path's:
tests.helpers.dtype_tolerances for o, rtol = atol = 1e-3 for finite lse — dequantisation is exact and only two fp32 multiplies
are added.  Appended bytes must be one of the two codes that bracket the exact quotient on every element and quantize()'s byte
on all but 1 in 10^3 (tests/test_kvcache_fp8_cpu.py shows quantize() itself is that close to the exact rounding); every other
byte of the caches is compared bitwise."""
import itertools

import pytest
import torch

from tests.helpers import dtype_tolerances
from tests.kvcache_fp8_ref import E4M3, FIXED_SCALES, absmax_scales, neighbours, quantize, randn16
from tests.kvcache_paged_ref import paged_tokens, reference
from tests.kvcache_rotary_ref import rotate64, round_once, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
U8 = torch.uint8


def check(o, lse, ro, rlse, dtype):
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    torch.testing.assert_close(o.double().cpu(), ro, **dtype_tolerances(dtype))
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse.cpu()), fin)
    torch.testing.assert_close(lse.double().cpu()[fin], rlse[fin], rtol=1e-3, atol=1e-3)
    assert (o.cpu().double().permute(0, 2, 1, 3)[~fin] == 0).all()


def dev(t):
    return None if t is None else t.to(DEV)


def dev8(codes):
    """uint8 codes (CPU) -> an e4m3 tensor on the device"""
    return codes.to(DEV).view(E4M3)


def alibi(hq):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / hq) for h in range(hq)], dtype=torch.float32)


def make(b, cap, hq, hkv, nq, d, dtype, seed, nnew=0, scales="absmax"):
    """CPU: q, the quantised caches (uint8), their scales (float32 (B, H_kv) or (H_kv,)), k_new, v_new"""
    q = randn16((b, nq, hq, d), dtype, seed)
    k16, v16 = randn16((b, cap, hkv, d), dtype, seed + 1), randn16((b, cap, hkv, d), dtype, seed + 2)
    kn = randn16((b, nnew, hkv, d), dtype, seed + 3) if nnew else None
    vn = randn16((b, nnew, hkv, d), dtype, seed + 4) if nnew else None
    if scales == "absmax":
        kd, vd = absmax_scales(k16), absmax_scales(v16)
    elif scales == "heads":
        kd, vd = absmax_scales(k16, per_batch=False), absmax_scales(v16, per_batch=False)
    else:   # the fixed, non-power-of-two scales, a different one per (b, head)
        fs = torch.tensor(FIXED_SCALES, dtype=torch.float32)
        kd = fs[torch.arange(b * hkv) % 5].view(b, hkv).contiguous()
        vd = fs[(torch.arange(b * hkv) + 2) % 5].view(b, hkv).contiguous()
    return q, quantize(k16, kd), quantize(v16, vd), kd, vd, kn, vn


def make_units(b, units, n, hq, hkv, nq, d, dtype, seed, nnew, owner, factors):
    """CPU, for pools and indexed caches of `units` pages or rows of n tokens: as make(), with per-sequence scales
    kd[b] = (absmax / 448 per head) * factors[b], and unit u quantised with the scale of its sequence owner[u] (factor 1 where
    owner[u] < 0), so that the dequantised cache every sequence reads is about unit scale while the scales differ by sequence."""
    q = randn16((b, nq, hq, d), dtype, seed)
    k16, v16 = randn16((units, n, hkv, d), dtype, seed + 1), randn16((units, n, hkv, d), dtype, seed + 2)
    kn, vn = randn16((b, nnew, hkv, d), dtype, seed + 3), randn16((b, nnew, hkv, d), dtype, seed + 4)
    f = torch.tensor(factors, dtype=torch.float32).view(-1, 1)
    fu = torch.tensor([factors[o] if o >= 0 else 1.0 for o in owner], dtype=torch.float32).view(-1, 1)
    bk, bv = absmax_scales(k16, per_batch=False).view(1, -1), absmax_scales(v16, per_batch=False).view(1, -1)
    return q, quantize(k16, bk * fu), quantize(v16, bv * fu), (bk * f).contiguous(), (bv * f).contiguous(), kn, vn


def deq_tokens(codes, ds, bb, hkv):
    """fp64 (n, H_kv, d): the tokens `codes` (n, H_kv, d) of sequence bb under its scales"""
    row = ds if ds.dim() == 1 else ds[bb]
    return codes.view(E4M3).double() * row.double().view(1, hkv, 1)


def check_appended(got, before, new16, ds, slots, cap_num=1, cap_den=1000):
    """got / before: a cache's uint8 codes after / before the call (CPU); slots: [(bb, n, unit, pos)] of the appended tokens that
    landed.  Appended elements: one of the two bracketing codes, quantize()'s byte on all but cap_num / cap_den; the rest unchanged.
    Returns (mismatches, elements)."""
    want = quantize(new16, ds)
    lo, hi = neighbours(new16, ds)
    expect = before.clone()
    mism = total = 0
    for bb, n, unit, pos in slots:
        g = got[unit, pos]
        assert bool(((g == lo[bb, n]) | (g == hi[bb, n])).all()), f"sequence {bb}, new token {n}: not a neighbour of the exact quotient"
        mism += int((g != want[bb, n]).sum())
        total += g.numel()
        expect[unit, pos] = g
    assert torch.equal(got, expect), "bytes outside the appended slots changed"
    assert mism * cap_den <= total * cap_num, f"{mism} of {total} appended bytes differ from quantize()"
    return mism, total


# ---- 1. parity, read-only and appending

PARITY = []
_i = 0
for _dtype, _d in itertools.product((torch.bfloat16, torch.float16), (8, 40, 64, 96, 128, 256)):
    for (_hq, _hkv), _nq in itertools.product(((8, 8), (8, 2), (8, 1)), (1, 5, 16, 130)):
        if (_i + _i // 12) % 4 == 0 or (_d, _hkv, _nq) in ((128, 2, 1), (256, 1, 130), (8, 8, 5)):   # thinned: every d x nq, every d x heads
            PARITY.append((_dtype, _d, _hq, _hkv, _nq, ("absmax", "heads", "fixed")[len(PARITY) % 3]))
        _i += 1


@pytest.mark.parametrize("dtype,d,hq,hkv,nq,scales", PARITY, ids=lambda x: str(x).replace("torch.", ""))
def test_parity(dtype, d, hq, hkv, nq, scales):
    from common.attention_ex import flash_attn_with_kvcache

    b, cap = 4, 300
    nnew = 1 if nq <= 2 else 0
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, nq, d, dtype, 100 + d + hkv + nq, nnew, scales)
    assert (kd.dim() == 1) == (scales == "heads")
    lens = torch.tensor([0, 1, cap - nnew, 137], dtype=torch.int32)
    sl = alibi(hq)
    variants = [(False, (-1, -1), 0.0, None), (True, (-1, -1), 0.0, None), (False, (40, 3), 0.0, None), (True, (64, -1), 30.0, None),
                (False, (-1, -1), 0.0, sl), (True, (-1, -1), 5.0, sl),
                (True, (-1, -1), 0.0, sl.unsqueeze(0) * torch.arange(1, b + 1).view(-1, 1).float())]
    # read-only: the dequantised tokens are the same for every variant
    ks = [deq_tokens(k8[bb, :lens[bb]], kd, bb, hkv) for bb in range(b)]
    vs = [deq_tokens(v8[bb, :lens[bb]], vd, bb, hkv) for bb in range(b)]
    qd, knd, vnd, kdd, vdd, lensd = dev(q), dev(kn), dev(vn), dev(kd), dev(vd), dev(lens)
    for vi, (causal, window, softcap, slopes) in enumerate(variants):
        for s in ((1, 4, 0) if vi in (0, 3) else ((1, 4, 0)[vi % 3],)):
            kc, vc = dev8(k8), dev8(v8)
            o, lse = flash_attn_with_kvcache(qd, kc, vc, knd, vnd, cache_seqlens=lensd, causal=causal, window_size=window,
                                             softcap=softcap, alibi_slopes=dev(slopes), num_splits=s, return_softmax_lse=True,
                                             k_descale=kdd, v_descale=vdd)
            if nnew:   # the append may differ from quantize() on rare elements (test_append_bytes): attend over what is there
                gk, gv = kc.view(U8).cpu(), vc.view(U8).cpu()
                ks = [deq_tokens(gk[bb, :lens[bb] + nnew], kd, bb, hkv) for bb in range(b)]
                vs = [deq_tokens(gv[bb, :lens[bb] + nnew], vd, bb, hkv) for bb in range(b)]
            ro, rlse = reference(q, ks, vs, causal, window, d ** -0.5, softcap, slopes)
            check(o, lse, ro, rlse, dtype)
            if not nnew:   # sequence 0 is empty: every row dead
                assert torch.isneginf(lse[0]).all() and (o[0] == 0).all()


# ---- 2. the bytes the append writes

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("scales", ["absmax", "heads", "fixed"])
def test_append_bytes(dtype, scales):
    import flashattention_lab_cuda as ext

    b, cap, hq, hkv, nq, d, nnew = 4, 300, 8, 2, 3, 128, 3
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, nq, d, dtype, 900, nnew, scales)
    seqlens = torch.tensor([-5, 10, cap + 100, 137], dtype=torch.int32)
    L = seqlens.clamp(0, cap - nnew)
    kc, vc = dev8(k8), dev8(v8)
    o, lse = ext.ex_kvcache_forward(dev(q), kc, vc, dev(kn), dev(vn), dev(seqlens), True, None, k_descale=dev(kd), v_descale=dev(vd))
    slots = [(bb, n, bb, int(L[bb]) + n) for bb in range(b) for n in range(nnew)]
    gk, gv = kc.view(U8).cpu(), vc.view(U8).cpu()
    mk, tk = check_appended(gk, k8, kn, kd, slots)
    mv, tv = check_appended(gv, v8, vn, vd, slots)
    print(f"append {dtype} {scales}: K {mk} of {tk}, V {mv} of {tv} bytes differ from quantize()")
    ks = [deq_tokens(gk[bb, :L[bb] + nnew], kd, bb, hkv) for bb in range(b)]
    vs = [deq_tokens(gv[bb, :L[bb] + nnew], vd, bb, hkv) for bb in range(b)]
    ro, rlse = reference(q, ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_append_saturates(dtype):
    import flashattention_lab_cuda as ext

    b, cap, hq, hkv, d = 2, 64, 4, 2, 64
    q, k8, v8, _, _, _, _ = make(b, cap, hq, hkv, 1, d, dtype, 950, 0, "fixed")
    kd = torch.tensor([[1.0, 2.0 ** -5], [0.0137, 3.7]])
    vd = torch.tensor([[3.7, 1.0], [2.0 ** -5, 0.0137]])
    sign = torch.where(randn16((b, 1, hkv, d), dtype, 951) >= 0, 1.0, -1.0)
    kn = (sign * 1e4 * kd.view(b, 1, hkv, 1)).to(dtype)        # |x| = 10^4 descale
    vn = (-sign * 1e4 * vd.view(b, 1, hkv, 1)).to(dtype)
    assert torch.isfinite(kn.float()).all() and torch.isfinite(vn.float()).all()
    kc, vc = dev8(k8), dev8(v8)
    lens = torch.tensor([5, 63], dtype=torch.int32)
    o, lse = ext.ex_kvcache_forward(dev(q), kc, vc, dev(kn), dev(vn), dev(lens), False, None, k_descale=dev(kd), v_descale=dev(vd))
    gk, gv = kc.view(U8).cpu(), vc.view(U8).cpu()
    for bb in range(b):
        assert torch.equal(gk[bb, lens[bb]], torch.where(sign[bb, 0] > 0, 0x7e, 0xfe).to(U8))
        assert torch.equal(gv[bb, lens[bb]], torch.where(sign[bb, 0] > 0, 0xfe, 0x7e).to(U8))
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    ks = [deq_tokens(gk[bb, :lens[bb] + 1], kd, bb, hkv) for bb in range(b)]
    vs = [deq_tokens(gv[bb, :lens[bb] + 1], vd, bb, hkv) for bb in range(b)]
    ro, rlse = reference(q, ks, vs, False, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, dtype)


# ---- 3. paged, indexed, left-padded

@pytest.mark.parametrize("ps,d,hkv,nq", [(16, 128, 2, 1), (48, 64, 8, 5), (256, 256, 1, 1), (16, 40, 2, 16)])
def test_paged_equals_contiguous_and_reference(ps, d, hkv, nq):
    import flashattention_lab_cuda as ext

    mb = {16: 20, 48: 7, 256: 3}[ps]
    b, cap, hq, nnew = 4, mb * ps, 8, 1
    g = torch.Generator().manual_seed(ps + d)
    nblk = b * mb + 3
    table = torch.randperm(nblk, generator=g)[:b * mb].view(b, mb).to(torch.int32)
    idx = table.long()
    owner = [-1] * nblk
    for bb in range(b):
        for pg in table[bb].tolist():
            owner[pg] = bb
    q, kp8, vp8, kd, vd, kn, vn = make_units(b, nblk, ps, hq, hkv, nq, d, BF16, 300 + ps, nnew, owner, (1.0, 1.5, 2.3, 3.1))
    lens = torch.tensor([cap - nnew, 2 * ps + 7, 0, cap - 33], dtype=torch.int32)
    args = dict(k_descale=dev(kd), v_descale=dev(vd))
    for (causal, window), s in zip(((True, (-1, -1)), (False, (37, 2)), (False, (-1, -1))), (1, 4, 0)):
        kc, vc = dev8(kp8[idx].reshape(b, cap, hkv, d).contiguous()), dev8(vp8[idx].reshape(b, cap, hkv, d).contiguous())
        oc, lc = ext.ex_kvcache_forward(dev(q), kc, vc, dev(kn), dev(vn), dev(lens), causal, None, window=window, num_splits=s, **args)
        kp, vp = dev8(kp8), dev8(vp8)
        op, lp = ext.ex_kvcache_forward(dev(q), kp, vp, dev(kn), dev(vn), dev(lens), causal, None, window=window, num_splits=s,
                                        block_table=dev(table), **args)
        assert torch.equal(op, oc) and torch.equal(lp, lc), (causal, window, s)
        gk, gv = kp.view(U8).cpu(), vp.view(U8).cpu()
        assert torch.equal(gk[idx].reshape(b, cap, hkv, d), kc.view(U8).cpu()) and torch.equal(gv[idx].reshape(b, cap, hkv, d), vc.view(U8).cpu())
        slots = [(bb, 0, int(table[bb, int(lens[bb]) // ps]), int(lens[bb]) % ps) for bb in range(b)]
        check_appended(gk, kp8, kn, kd, slots)
        check_appended(gv, vp8, vn, vd, slots)
        ks = [deq_tokens(paged_tokens(gk, table[bb], int(lens[bb]) + nnew, ps), kd, bb, hkv) for bb in range(b)]
        vs = [deq_tokens(paged_tokens(gv, table[bb], int(lens[bb]) + nnew, ps), vd, bb, hkv) for bb in range(b)]
        ro, rlse = reference(q, ks, vs, causal, window, d ** -0.5)
        check(op, lp, ro, rlse, BF16)


def test_paged_prefix_sharing_and_out_of_range_page():
    import flashattention_lab_cuda as ext

    b, ps, mb, hq, hkv, d, nblk = 3, 16, 6, 8, 2, 128, 12
    # sequences 0 and 1 share their first two pages (read only) and therefore their scales; sequence 2 appends to a page
    # outside the pool and reads one
    table = torch.tensor([[3, 7, 1, 0, 0, 0], [3, 7, 9, 4, 0, 0], [5, -1, nblk, 2, 0, 0]], dtype=torch.int32)
    owner = [-1] * nblk
    for pg, bb in ((3, 0), (7, 0), (1, 0), (9, 1), (4, 1), (5, 2), (2, 2)):
        owner[pg] = bb
    q, kp8, vp8, kd, vd, kn, vn = make_units(b, nblk, ps, hq, hkv, 1, d, torch.float16, 41, 1, owner, (1.5, 1.5, 2.3))
    lens = torch.tensor([40, 55, 35], dtype=torch.int32)   # the appends go to pages 1 (token 40), 4 (token 55) and nblk (token 35: dropped)
    for s in (1, 4, 0):
        kp, vp = dev8(kp8), dev8(vp8)
        o, lse = ext.ex_kvcache_forward(dev(q), kp, vp, dev(kn), dev(vn), dev(lens), True, None, num_splits=s, block_table=dev(table),
                                        k_descale=dev(kd), v_descale=dev(vd))
        gk, gv = kp.view(U8).cpu(), vp.view(U8).cpu()
        slots = [(0, 0, 1, 40 % ps), (1, 0, 4, 55 % ps)]     # sequence 2's append is dropped: the pool keeps its bytes there
        check_appended(gk, kp8, kn, kd, slots)
        check_appended(gv, vp8, vn, vd, slots)
        ks = [deq_tokens(paged_tokens(gk, table[bb], int(lens[bb]) + 1, ps), kd, bb, hkv) for bb in range(b)]   # bad pages: zeros
        vs = [deq_tokens(paged_tokens(gv, table[bb], int(lens[bb]) + 1, ps), vd, bb, hkv) for bb in range(b)]
        assert (ks[2][16:48] == 0).all()
        ro, rlse = reference(q, ks, vs, True, (-1, -1), d ** -0.5)
        check(o, lse, ro, rlse, torch.float16)


@pytest.mark.parametrize("leftpad", [False, True], ids=["idx", "idx-leftpad"])
def test_cache_batch_idx_leftpad_and_scales_follow_the_sequence(leftpad):
    import flashattention_lab_cuda as ext

    b, bc, cap, hq, hkv, d, nq = 4, 6, 300, 8, 2, 128, 2
    # per-sequence scales that differ (by up to 3.1), and a permuting index with one entry out of range: the scale used is that of
    # sequence b, not of cache row idx[b] — a row read with another sequence's scale would be off by a factor of 1.35 to 3.1
    bidx = torch.tensor([4, 0, bc, 2], dtype=torch.int32)
    owner = [-1] * bc
    for bb in (0, 1, 3):
        owner[int(bidx[bb])] = bb
    q, k8, v8, kd, vd, kn, vn = make_units(b, bc, cap, hq, hkv, nq, d, BF16, 61, 1, owner, (1.0, 1.5, 2.3, 3.1))
    pad = torch.tensor([3, 37, -3, 500], dtype=torch.int32) if leftpad else None
    lens = torch.tensor([0, 77, 150, 201], dtype=torch.int32)
    P = [min(max(int(pad[i]), 0), int(lens[i])) if leftpad else 0 for i in range(b)]
    for s in (1, 4, 0):
        kc, vc = dev8(k8), dev8(v8)
        o, lse = ext.ex_kvcache_forward(dev(q), kc, vc, dev(kn), dev(vn), dev(lens), True, None, num_splits=s, cache_batch_idx=dev(bidx),
                                        cache_leftpad=dev(pad), k_descale=dev(kd), v_descale=dev(vd))
        gk, gv = kc.view(U8).cpu(), vc.view(U8).cpu()
        slots = [(bb, 0, int(bidx[bb]), int(lens[bb])) for bb in range(b) if int(bidx[bb]) < bc]
        check_appended(gk, k8, kn, kd, slots)
        check_appended(gv, v8, vn, vd, slots)
        ks, vs = [], []
        for bb in range(b):
            n = int(lens[bb]) + 1
            if int(bidx[bb]) < bc:
                ks.append(deq_tokens(gk[int(bidx[bb]), P[bb]:n], kd, bb, hkv))
                vs.append(deq_tokens(gv[int(bidx[bb]), P[bb]:n], vd, bb, hkv))
            else:   # a row outside the cache reads as zeros
                ks.append(torch.zeros((n - P[bb], hkv, d), dtype=torch.float64))
                vs.append(torch.zeros((n - P[bb], hkv, d), dtype=torch.float64))
        ro, rlse = reference(q, ks, vs, True, (-1, -1), d ** -0.5)
        check(o, lse, ro, rlse, BF16)


# ---- 4. rotary

@pytest.mark.parametrize("interleaved", [True, False], ids=["gptj", "neox"])
@pytest.mark.parametrize("dtype,d,rdim,hkv,nq,s", [(torch.bfloat16, 128, 16, 2, 1, 0), (torch.float16, 128, 128, 2, 3, 4),
                                                   (torch.bfloat16, 64, 64, 8, 3, 1), (torch.float16, 256, 16, 1, 2, 0)])
def test_rotary_with_an_e4m3_cache(dtype, d, rdim, hkv, nq, s, interleaved):
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, nnew = 4, 320, 8, nq
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, nq, d, dtype, 700 + d + rdim, nnew, "absmax")
    lens = torch.tensor([0, 77, cap + 50, 201], dtype=torch.int32)
    pad = torch.tensor([3, 37, -3, 130], dtype=torch.int32)
    L = [min(max(int(x), 0), cap - nnew) for x in lens]
    P = [min(max(int(pad[i]), 0), L[i]) for i in range(b)]
    cos, sin = tables(cap, rdim, dtype)
    kc, vc = dev8(k8), dev8(v8)
    o, lse = flash_attn_with_kvcache(dev(q), kc, vc, dev(kn), dev(vn), rotary_cos=dev(cos), rotary_sin=dev(sin),
                                     rotary_interleaved=interleaved, cache_seqlens=dev(lens), cache_leftpad=dev(pad), causal=True,
                                     num_splits=s, return_softmax_lse=True, k_descale=dev(kd), v_descale=dev(vd))
    # the reference's rotation, rounded once to 16 bits, then quantised
    kr = torch.stack([round_once(rotate64(kn[bb], cos, sin, [L[bb] - P[bb] + n for n in range(nnew)], interleaved), dtype) for bb in range(b)])
    qr = torch.stack([round_once(rotate64(q[bb], cos, sin, [L[bb] - P[bb] + i for i in range(nq)], interleaved), dtype) for bb in range(b)])
    gk, gv = kc.view(U8).cpu(), vc.view(U8).cpu()
    slots = [(bb, n, bb, L[bb] + n) for bb in range(b) for n in range(nnew)]
    want = quantize(kr, kd)
    mism = sum(int((gk[u, p] != want[bb, n]).sum()) for bb, n, u, p in slots)
    total = len(slots) * hkv * d
    print(f"rotary {dtype} d={d} rdim={rdim}: {mism} of {total} appended K bytes differ from quantize(rotated reference)")
    assert mism * 1000 <= 2 * total
    expect = k8.clone()
    for bb, n, u, p in slots:
        expect[u, p] = gk[u, p]
    assert torch.equal(gk, expect)
    check_appended(gv, v8, vn, vd, slots)
    ks = [deq_tokens(gk[bb, P[bb]:L[bb] + nnew], kd, bb, hkv) for bb in range(b)]
    vs = [deq_tokens(gv[bb, P[bb]:L[bb] + nnew], vd, bb, hkv) for bb in range(b)]
    ro, rlse = reference(qr, ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, dtype)


# ---- 5. strided and odd layouts

def test_unbound_kv_views_and_wide_token_stride():
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hkv, hq, d, nq = 3, 200, 2, 8, 128, 1
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, nq, d, BF16, 81, 1, "absmax")
    lens = torch.tensor([5, 100, 199], dtype=torch.int32)
    kv = torch.stack([k8, v8], dim=2).to(DEV).view(E4M3)                    # (B, cap, 2, H_kv, d)
    wide = torch.zeros((2, b, cap, hkv * d + 24), dtype=U8)                 # token stride H_kv d + 24
    wide[0, :, :, :hkv * d], wide[1, :, :, :hkv * d] = k8.view(b, cap, -1), v8.view(b, cap, -1)
    wide = wide.to(DEV).view(E4M3)
    for kc, vc, buf in ((*kv.unbind(2), kv), (wide[0, :, :, :hkv * d].view(b, cap, hkv, d), wide[1, :, :, :hkv * d].view(b, cap, hkv, d), wide)):
        assert not kc.is_contiguous()
        before = buf.view(U8).clone()
        o, lse = flash_attn_with_kvcache(dev(q), kc, vc, dev(kn), dev(vn), cache_seqlens=dev(lens), causal=True, return_softmax_lse=True,
                                         k_descale=dev(kd), v_descale=dev(vd))
        gk, gv = kc.view(U8).cpu(), vc.view(U8).cpu()
        slots = [(bb, 0, bb, int(lens[bb])) for bb in range(b)]
        check_appended(gk, k8, kn, kd, slots)
        check_appended(gv, v8, vn, vd, slots)
        changed = (buf.view(U8) != before).sum().item()
        assert changed <= 2 * b * hkv * d                                   # nothing but the appended tokens
        ks = [deq_tokens(gk[bb, :lens[bb] + 1], kd, bb, hkv) for bb in range(b)]
        vs = [deq_tokens(gv[bb, :lens[bb] + 1], vd, bb, hkv) for bb in range(b)]
        ro, rlse = reference(q, ks, vs, True, (-1, -1), d ** -0.5)
        check(o, lse, ro, rlse, BF16)


def test_misaligned_view_raises_and_leaves_the_cache_alone():
    import flashattention_lab_cuda as ext

    b, cap, hkv, hq, d = 2, 64, 2, 8, 64
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, 1, d, BF16, 85, 1, "absmax")
    flat = torch.zeros(b * cap * hkv * d + 16, dtype=U8, device=DEV)
    flat[4:4 + k8.numel()] = k8.to(DEV).view(-1)
    kc = flat[4:4 + k8.numel()].view(b, cap, hkv, d).view(E4M3)            # 4 bytes off an 8-byte boundary
    vc = dev8(v8)
    assert kc.data_ptr() % 8 == 4
    before = flat.clone()
    with pytest.raises(ValueError, match="8-byte aligned"):
        ext.ex_kvcache_forward(dev(q), kc, vc, dev(kn), dev(vn), dev(torch.tensor([3, 9], dtype=torch.int32)), True, None,
                               k_descale=dev(kd), v_descale=dev(vd))
    odd = torch.zeros((b, cap, hkv * d + 4), dtype=U8, device=DEV).view(E4M3)   # a token stride that is no multiple of 8
    with pytest.raises(ValueError, match="multiples of 8"):
        ext.ex_kvcache_forward(dev(q), odd[:, :, :hkv * d].view(b, cap, hkv, d), vc, None, None, None, True, None)
    torch.cuda.synchronize()
    assert torch.equal(flat, before) and torch.equal(vc.view(U8).cpu(), v8)


# ---- 6. the 16-bit call on the same values

@pytest.mark.parametrize("dtype,d,hkv,nq", [(torch.bfloat16, 128, 2, 1), (torch.float16, 64, 8, 5), (torch.bfloat16, 256, 1, 16),
                                            (torch.float16, 96, 2, 1)])
def test_unit_scales_match_the_16_bit_call(dtype, d, hkv, nq):
    import flashattention_lab_cuda as ext

    b, cap, hq = 4, 300, 8
    q, k8, v8, _, _, _, _ = make(b, cap, hq, hkv, nq, d, dtype, 91, 0, "heads")
    one = torch.ones((b, hkv), dtype=torch.float32, device=DEV)
    lens = dev(torch.tensor([0, 1, cap, 137], dtype=torch.int32))
    kc, vc = dev8(k8), dev8(v8)
    k16, v16 = kc.to(dtype), vc.to(dtype)
    assert torch.equal(k16.double().cpu(), k8.view(E4M3).double())           # the device's widening cast is exact too
    for s in (1, 4, 0):
        o8, l8 = ext.ex_kvcache_forward(dev(q), kc, vc, None, None, lens, True, None, num_splits=s, k_descale=one, v_descale=one)
        on, ln = ext.ex_kvcache_forward(dev(q), kc, vc, None, None, lens, True, None, num_splits=s)      # null scales are 1.0
        o16, l16 = ext.ex_kvcache_forward(dev(q), k16, v16, None, None, lens, True, None, num_splits=s)
        assert torch.equal(o8, on) and torch.equal(l8, ln)
        print(f"{dtype} d={d} S={s}: e4m3 call bitwise equal to the 16-bit call: o {torch.equal(o8, o16)}, lse {torch.equal(l8, l16)}")
        torch.testing.assert_close(o8.float(), o16.float(), **dtype_tolerances(dtype))
        fin = torch.isfinite(l16)
        assert torch.equal(torch.isfinite(l8), fin)
        torch.testing.assert_close(l8[fin], l16[fin], rtol=1e-3, atol=1e-3)


# ---- 7. graph capture

def test_graph_capture_appending_step():
    """One captured appending step, replayed with cache_seqlens and the scales changed on the device.  One stream, no parallel
    branches."""
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, d = 2, 512, 8, 2, 128
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, 1, d, BF16, 21, 1, "absmax")
    kc, vc = dev8(k8), dev8(v8)
    qd, knd, vnd, kdd, vdd = dev(q), dev(kn), dev(vn), dev(kd), dev(vd)
    lens = torch.tensor([10, 300], dtype=torch.int32, device=DEV)
    kw = dict(cache_seqlens=lens, causal=True, num_splits=0, return_softmax_lse=True, k_descale=kdd, v_descale=vdd)
    flash_attn_with_kvcache(qd, kc, vc, knd, vnd, **kw)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            out = flash_attn_with_kvcache(qd, kc, vc, knd, vnd, **kw)
    torch.cuda.current_stream().wait_stream(st)
    for new_lens, mul in (([11, 301], 1.0), ([200, 5], 1.37)):
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32))
        kdd.mul_(mul)                                    # changed on the device between replays
        vdd.mul_(1.0 / mul)
        k_before, v_before = kc.view(U8).clone(), vc.view(U8).clone()
        graph.replay()
        torch.cuda.synchronize()
        o_g, l_g, k_g, v_g = out[0].clone(), out[1].clone(), kc.view(U8).clone(), vc.view(U8).clone()
        kc.view(U8).copy_(k_before)
        vc.view(U8).copy_(v_before)
        o_e, l_e = flash_attn_with_kvcache(qd, kc, vc, knd, vnd, **kw)
        assert torch.equal(o_g, o_e) and torch.equal(l_g, l_e)
        assert torch.equal(k_g, kc.view(U8)) and torch.equal(v_g, vc.view(U8))
        kdc, vdc, gk, gv = kdd.cpu(), vdd.cpu(), k_g.cpu(), v_g.cpu()
        slots = [(bb, 0, bb, new_lens[bb]) for bb in range(b)]
        check_appended(gk, k_before.cpu(), kn, kdc, slots)
        check_appended(gv, v_before.cpu(), vn, vdc, slots)
        ks = [deq_tokens(gk[bb, :new_lens[bb] + 1], kdc, bb, hkv) for bb in range(b)]
        vs = [deq_tokens(gv[bb, :new_lens[bb] + 1], vdc, bb, hkv) for bb in range(b)]
        ro, rlse = reference(q, ks, vs, True, (-1, -1), d ** -0.5)
        check(o_g, l_g, ro, rlse, BF16)


# ---- 8. errors through Python, and the unchanged 16-bit call

def test_python_errors_and_the_16_bit_call_is_unchanged():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, d = 3, 64, 8, 2, 64
    q, k8, v8, kd, vd, kn, vn = make(b, cap, hq, hkv, 1, d, BF16, 99, 1, "absmax")
    qd, kc, vc, kdd, vdd = dev(q), dev8(k8), dev8(v8), dev(kd), dev(vd)
    k16, v16 = kc.to(BF16), vc.to(BF16)
    lens = torch.tensor([3, 9, 60], dtype=torch.int32, device=DEV)
    before = kc.view(U8).clone()
    for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(NotImplementedError):
            flash_attn_with_kvcache(qd, kc.view(bad), vc.view(bad), cache_seqlens=lens)
        with pytest.raises(NotImplementedError):
            ext.ex_kvcache_forward(qd, kc.view(bad), vc.view(bad), None, None, lens)
    with pytest.raises(RuntimeError, match="both q's dtype or both"):
        flash_attn_with_kvcache(qd, kc, v16, cache_seqlens=lens)
    with pytest.raises(RuntimeError, match="need a torch.float8_e4m3fn cache"):
        flash_attn_with_kvcache(qd, k16, v16, cache_seqlens=lens, k_descale=kdd)
    with pytest.raises(RuntimeError, match="need a torch.float8_e4m3fn cache"):
        ext.ex_kvcache_forward(qd, k16, v16, None, None, lens, v_descale=vdd)
    with pytest.raises(NotImplementedError, match="float32"):
        flash_attn_with_kvcache(qd, kc, vc, cache_seqlens=lens, k_descale=kdd.double())
    with pytest.raises(NotImplementedError, match="float32"):
        ext.ex_kvcache_forward(qd, kc, vc, None, None, lens, v_descale=vdd.half())
    with pytest.raises(RuntimeError, match=r"\(B, H_kv\)"):
        flash_attn_with_kvcache(qd, kc, vc, cache_seqlens=lens, k_descale=torch.ones(b, device=DEV))
    with pytest.raises(RuntimeError, match="q's device"):
        flash_attn_with_kvcache(qd, kc, vc, cache_seqlens=lens, v_descale=vd)
    torch.cuda.synchronize()
    assert torch.equal(kc.view(U8), before)
    # the 16-bit call with the new keywords left at None: the same bits as without them
    for s in (1, 0):
        ka, va, kb_, vb = k16.clone(), v16.clone(), k16.clone(), v16.clone()
        o0, l0 = ext.ex_kvcache_forward(qd, ka, va, dev(kn), dev(vn), lens, True, None, num_splits=s)
        o1, l1 = ext.ex_kvcache_forward(qd, kb_, vb, dev(kn), dev(vn), lens, True, None, num_splits=s, k_descale=None, v_descale=None)
        assert torch.equal(o0, o1) and torch.equal(l0, l1) and torch.equal(ka, kb_) and torch.equal(va, vb)
