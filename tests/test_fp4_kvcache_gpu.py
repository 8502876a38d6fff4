"""GPU: the MXFP4 KV cache (csrc/fa_fp4_decode.hip) through common.fp4_kvcache.

  * the append bit for bit against the rule restated here in torch, untouched bytes included;
  * decoding against fp64 attention on code * 2^e * descale, held to the sharp bar (tests/ex_full_ref.sharp_bar, factor 2) with the
    merged e4m3 call on the exactly widened cache as the baseline; V exponents far from 0 and far apart; untrusted lengths, table
    entries and cache rows with guarded outputs; append + decode replayed from one graph.
The kernel / baseline ratios are printed per case (profiles/fp4_kvcache.md records a run)."""
import math

import pytest
import torch

from tests.ex_full_ref import Result, sharp_bar

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
MAGS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
E2M1 = torch.cat((MAGS, -MAGS))                                  # code s eem
B, HQ, HKV, CAP, PS = 2, 8, 2, 256, 16


def values(codes, scale):
    """(.., H, 64) code bytes and (.., H, nb) E8M0 bytes -> (.., H, 128) float64 code * 2^(byte - 127), nb blocks a head"""
    x = E2M1[torch.stack((codes & 15, codes >> 4), -1).flatten(-2).long()]
    e = (scale.double() - 127.0).reshape(*codes.shape[:-1], -1)
    return x * torch.exp2(e).repeat_interleave(128 // e.shape[-1], -1)


def append_model(x, descale, block):
    """the append rule: x (.., H, 128) 16-bit, descale float32 broadcastable to (.., H, 1) -> (codes (.., H, 64), bytes (.., H, 128 / block))"""
    xp = (x.float() * (1.0 / descale.float())).reshape(*x.shape[:-1], 128 // block, block)
    amax = xp.abs().amax(-1)
    m, ex = torch.frexp(amax)                                    # amax = m 2^ex, m in [.5, 1): 6 * 2^e = .75 * 2^(e + 3)
    e = torch.where(amax == 0, torch.zeros_like(ex), ex - 3 + (m > 0.75).int()).clamp(-64, 64)
    y = xp.double() * torch.exp2(-e.double()).unsqueeze(-1)
    near = (y.abs().unsqueeze(-1) - MAGS).abs()
    is_min = near == near.amin(-1, keepdim=True)                 # a tie: two codes, the even one wins
    code = (is_min * torch.tensor([2, 1] * 4)).argmax(-1) + 8 * (y < 0)
    code = code.reshape(*x.shape[:-1], 64, 2)
    return (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8), (e + 127).to(torch.uint8)


def lay_out(layout, arrays, seed):
    """the (B, CAP, ..) arrays as the call takes them: as they are, in rows (2, 0) of a 3-row cache behind cache_batch_idx, or in a
    shuffled pool of PS-token pages; -> (arrays, keywords)"""
    if layout == "contig":
        return arrays, {}
    if layout == "bidx":
        idx = torch.tensor([2, 0], dtype=torch.int32)
        out = [torch.zeros((3, *a.shape[1:]), dtype=a.dtype) for a in arrays]
        for o, a in zip(out, arrays):
            o[idx.long()] = a
        return out, dict(cache_batch_idx=idx.to(DEV))
    nb = CAP // PS
    table = torch.randperm(B * nb + 3, generator=torch.Generator().manual_seed(seed))[:B * nb].reshape(B, nb).to(torch.int32)
    out = [torch.zeros((B * nb + 3, PS, *a.shape[2:]), dtype=a.dtype) for a in arrays]
    for o, a in zip(out, arrays):
        o[table.reshape(-1).long()] = a.reshape(B * nb, PS, *a.shape[2:])
    return out, dict(block_table=table.to(DEV))


def reference(q8, kval, vval, lens, scale, qd, kd, vd, causal):
    """fp64 attention per sequence: q8 (B, Nq, HQ, 128) e4m3, kval / vval (B, CAP, HKV, 128) float64 without the descales"""
    nq, g = q8.shape[1], HQ // HKV
    o = torch.zeros((B, nq, HQ, 128), dtype=torch.float64)
    lse = torch.full((B, HQ, nq), -math.inf, dtype=torch.float64)
    for b in range(B):
        n = lens[b]
        for h in range(HQ if n else 0):
            hk = h // g
            s = scale * qd[b, hk].double() * kd[b, hk].double() * (q8[b, :, h].double() @ kval[b, :n, hk].T)
            if causal:
                s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(nq)[:, None] + n - nq, -math.inf)
            lse[b, h] = torch.logsumexp(s, -1)
            o[b, :, h] = torch.nan_to_num(torch.exp(s - lse[b, h][:, None])) @ (vval[b, :n, hk] * vd[b, hk].double())
    return o, lse


def check(nq, lens, splits, layout, dtype, ek=None, ev=None, base_shift=0, causal=False, seed=0, call_lens=None, spoil=None):
    """one decode call against fp64 and the e4m3 baseline.  ek / ev: the exponents (default: drawn from [-5, 5]); base_shift: the
    baseline's V exponents are ev + base_shift with v_descale * 2^-base_shift; call_lens: what the call is handed (default lens);
    spoil(keywords, kval, vval): makes table entries or indices untrusted and the reference to match."""
    from common.fp4_kvcache import fp8_attn_with_mxfp4_kvcache
    from common.fp8_attention import fp8_attn_with_kvcache

    g = torch.Generator().manual_seed(1000 * nq + 10 * splits + seed)
    q8 = (torch.randn((B, nq, HQ, 128), generator=g) * 1.5).to(E4)
    kc, vc = (torch.randint(0, 256, (B, CAP, HKV, 64), generator=g, dtype=torch.uint8) for _ in range(2))
    ks = (127 + (torch.randint(-5, 6, (B, CAP, HKV, 4), generator=g) if ek is None else ek)).to(torch.uint8)
    vs = (127 + (torch.randint(-5, 6, (B, CAP, HKV), generator=g) if ev is None else ev)).to(torch.uint8)
    qd, kd, vd = (0.2 + 0.3 * torch.rand((B, HKV), generator=g) for _ in range(3))
    kval, vval = values(kc, ks), values(vc, vs)
    k8, v8 = kval.to(E4), (vval * 2.0 ** base_shift).to(E4)       # the widening must be exact
    assert torch.equal(k8.double(), kval) and torch.equal(v8.double(), vval * 2.0 ** base_shift)
    (kc, ks, vc, vs, k8, v8), kw = lay_out(layout, (kc, ks, vc, vs, k8.view(torch.uint8), v8.view(torch.uint8)), seed)
    if spoil is not None:
        spoil(kw, kval, vval)
    kw.update(cache_seqlens=torch.tensor(call_lens or lens, dtype=torch.int32, device=DEV), q_descale=qd.to(DEV), k_descale=kd.to(DEV),
              causal=causal, num_splits=splits, out_dtype=dtype, return_softmax_lse=True)
    o, lse = fp8_attn_with_mxfp4_kvcache(q8.to(DEV), kc.to(DEV), ks.to(DEV), vc.to(DEV), vs.to(DEV), v_descale=vd.to(DEV), **kw)
    ob, lb = fp8_attn_with_kvcache(q8.to(DEV), k8.to(DEV).view(E4), v8.to(DEV).view(E4), v_descale=(vd * 2.0 ** -base_shift).to(DEV), **kw)
    ro, rl = reference(q8, kval, vval, lens, 128 ** -0.5, qd, kd, vd, causal)
    pack = lambda o_, l_: Result(o_.cpu().reshape(-1, 128), l_.cpu().reshape(B * HQ, nq), *[None] * 9)   # noqa: E731
    dead = rl == -math.inf
    assert torch.equal(lse.cpu() == -math.inf, dead) and bool((o.cpu().transpose(1, 2)[dead] == 0).all())
    assert bool(torch.isfinite(o).all())
    bad, ratio = sharp_bar(pack(o, lse), pack(ro, rl), pack(ob, lb), dtype)
    print(f"RATIO nq={nq} lens={lens} S={splits} {layout} {dtype} shift={base_shift} " + " ".join(f"{k}={v:.3f}" for k, v in ratio.items()))
    assert not bad, bad
    return o, lse


# ---- 1. the append, bit for bit

@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=("f16", "bf16"))
@pytest.mark.parametrize("nnew", (1, 5))
@pytest.mark.parametrize("layout", ("bidx", "ps16"))
def test_append_bits(layout, nnew, dtype):
    """lengths (0, 13) of capacity 16: with 5 new tokens the last two of sequence 1 fall past the capacity and are dropped.  Token 0
    of head 0 holds, in its first K blocks and in V: an all-zero block, then a block of amax exactly 6 * 2^1 with the ties 2.5 * 2^1,
    5 * 2^1 and 0.25 * 2^1 (k_descale = v_descale = 0.5 there, so x' = 2 x)."""
    from common.fp4_kvcache import mxfp4_kvcache_append

    cap, lens = 16, (0, 13)
    g = torch.Generator().manual_seed(nnew)
    k, v = ((torch.randn((B, nnew, HKV, 128), generator=g) * 3.0).to(dtype) for _ in range(2))
    k[0, 0, 0, :32] = 0.0
    k[0, 0, 0, 32:64] = torch.tensor([6.0, 2.5, 5.0, 0.25, -2.5, -0.25, -5.0, 0.75] * 4)
    v[0, 0, 0] = torch.tensor([6.0, 2.5, 5.0, 0.25, -2.5, -0.25, -5.0, 0.75] * 16)
    v[1, 0, 1] = 0.0
    kd = torch.tensor([[0.5, 0.3], [1.7, 2.0]])
    vd = torch.tensor([[0.5, 1.1], [0.7, 3.0]])
    kcode, kbyte = append_model(k, kd[:, None, :, None], 32)
    vcode, vbyte = append_model(v, vd[:, None, :, None], 128)
    assert kbyte[0, 0, 0, 0] == 127 and kbyte[0, 0, 0, 1] == 128 and vbyte[0, 0, 0, 0] == 128 and vbyte[1, 0, 1, 0] == 127
    rows, kw = (2, 0), dict(cache_batch_idx=torch.tensor([2, 0], dtype=torch.int32, device=DEV))
    shapes = [(3, cap, HKV, 64), (3, cap, HKV, 4), (3, cap, HKV, 64), (3, cap, HKV)]
    if layout == "ps16":
        rows, kw = (3, 1), dict(block_table=torch.tensor([[3], [1]], dtype=torch.int32, device=DEV))
        shapes = [(5, PS, HKV, 64), (5, PS, HKV, 4), (5, PS, HKV, 64), (5, PS, HKV)]
    before = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in shapes]
    want = [t.clone() for t in before]
    for b in range(B):
        for i in range(nnew):
            if lens[b] + i < cap:
                for t, new in zip(want, (kcode, kbyte, vcode, vbyte[..., 0])):
                    t[rows[b], lens[b] + i] = new[b, i]
    got = [t.to(DEV) for t in before]
    mxfp4_kvcache_append(k.to(DEV), v.to(DEV), *got, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), k_descale=kd.to(DEV),
                         v_descale=vd.to(DEV), **kw)
    for name, a, w in zip(("k_cache", "k_scale", "v_cache", "v_scale"), got, want):
        assert torch.equal(a.cpu(), w), (name, (a.cpu() != w).nonzero()[:4])


# ---- 2. decoding against fp64

CASES = [(nq, (65, 200), s, layout, torch.float16 if (nq, s, layout) == (9, 3, "contig") else torch.bfloat16)
         for nq in (1, 9) for s in (1, 3) for layout in ("contig", "bidx", "ps16")]
CASES += [(9, (1, 64), 3, "ps16", torch.bfloat16), (1, (1, 64), 1, "contig", torch.bfloat16)]


@pytest.mark.parametrize("nq,lens,splits,layout,dtype", CASES, ids=[f"nq{c[0]}-{c[1][0]}_{c[1][1]}-S{c[2]}-{c[3]}-{str(c[4])[6:]}" for c in CASES])
def test_decode_against_fp64(nq, lens, splits, layout, dtype):
    check(nq, lens, splits, layout, dtype, causal=nq > 1)


# ---- 3. the range of V's scale

@pytest.mark.parametrize("splits", (1, 3))
@pytest.mark.parametrize("which", ("all_minus_20", "alternating"))
def test_v_scale_range(which, splits):
    """every ev = -20: P' must still peak at 1 (a kernel that folds ev without the joint maximum flushes all of P to zero); ev
    alternating -6 / +5 with unit K scales: both kinds of key in one tile."""
    if which == "all_minus_20":
        check(1, (65, 200), splits, "contig", torch.bfloat16, ev=torch.full((B, CAP, HKV), -20), base_shift=20)
    else:
        ev = torch.where(torch.arange(CAP) % 2 == 0, -6, 5)[None, :, None].expand(B, CAP, HKV)
        check(1, (65, 200), splits, "contig", torch.bfloat16, ek=torch.zeros((B, CAP, HKV, 4), dtype=torch.int64), ev=ev)


# ---- 4. untrusted inputs, outputs inside guard bytes

def test_untrusted_lengths_table_and_rows():
    def bad_page(kw, kval, vval):                                 # keys 32 .. 47 of sequence 1 on a page outside the pool: zeros
        kw["block_table"][1, 2] = 10 ** 6
        kw["block_table"][0, 1] = -1
        kval[1, 32:48], vval[1, 32:48], kval[0, 16:32], vval[0, 16:32] = 0.0, 0.0, 0.0, 0.0

    def bad_row(kw, kval, vval):
        kw["cache_batch_idx"][1] = 3

    check(1, (CAP, 0), 3, "contig", torch.bfloat16, call_lens=(CAP + 50, -3))
    check(9, (65, 200), 1, "ps16", torch.bfloat16, causal=True, spoil=bad_page)
    check(1, (65, 0), 1, "bidx", torch.bfloat16, call_lens=(65, 200), spoil=bad_row)
    # the outputs inside guard bytes: the call writes its tensors and nothing beside them
    import flashattention_lab_cuda as ext
    g = torch.Generator().manual_seed(4)
    q8 = torch.randn((B, 9, HQ, 128), generator=g).to(E4).to(DEV)
    kc, vc = (torch.randint(0, 256, (B, CAP, HKV, 64), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    ks, vs = torch.full((B, CAP, HKV, 4), 127, dtype=torch.uint8, device=DEV), torch.full((B, CAP, HKV), 0xFF, dtype=torch.uint8, device=DEV)
    lens = torch.tensor([2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    for splits in (1, 3):
        n_o, n_l, pad = B * 9 * HQ * 128, B * HQ * 9, 4096
        buf_o = torch.full((n_o + 2 * pad,), -7.0, dtype=torch.bfloat16, device=DEV)
        buf_l = torch.full((n_l + 2 * pad,), -7.0, dtype=torch.float32, device=DEV)
        out = (buf_o[pad:pad + n_o].view(B, 9, HQ, 128), buf_l[pad:pad + n_l].view(B, HQ, 9))
        ext.fp4_kvcache_forward(q8, kc, ks, vc, vs, lens, causal=True, num_splits=splits, out=out)   # (0xFF scales: any numbers, no fault)
        torch.cuda.synchronize()
        for buf, n in ((buf_o, n_o), (buf_l, n_l)):
            assert bool((buf[:pad] == -7.0).all()) and bool((buf[pad + n:] == -7.0).all())
        assert bool((out[0][1] == 0).all()) and bool((out[1][1] == -math.inf).all())


# ---- 5. append + decode from one graph

def test_graph_replay_after_the_state_changed():
    from common.fp4_kvcache import fp8_attn_with_mxfp4_kvcache, mxfp4_kvcache_append

    g = torch.Generator().manual_seed(5)
    nb, nnew = CAP // PS, 5
    pool = [torch.randint(0, 256, (B * nb, PS, HKV, 64), generator=g, dtype=torch.uint8), torch.randint(122, 133, (B * nb, PS, HKV, 4), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (B * nb, PS, HKV, 64), generator=g, dtype=torch.uint8), torch.randint(122, 133, (B * nb, PS, HKV), generator=g, dtype=torch.uint8)]
    state = lambda s: (torch.tensor(((13, 60), (77, 190))[s], dtype=torch.int32), (torch.randn((B, nnew, HKV, 128), generator=g) * (1 + s)).bfloat16(),   # noqa: E731
                       (torch.randn((B, nnew, HKV, 128), generator=g) * (2 - s)).bfloat16(),
                       torch.randperm(B * nb, generator=g).reshape(B, nb).to(torch.int32))
    first, second = state(0), state(1)
    lens, k, v, table = (t.to(DEV) for t in first)
    q8 = torch.randn((B, 1, HQ, 128), generator=g).to(E4).to(DEV)
    dev_pool = [t.to(DEV) for t in pool]

    def step():
        mxfp4_kvcache_append(k, v, *dev_pool, cache_seqlens=lens, block_table=table)
        return fp8_attn_with_mxfp4_kvcache(q8, *dev_pool, cache_seqlens=lens + nnew, block_table=table, num_splits=3, return_softmax_lse=True)

    step()                                                        # (the workspace and the lazy initialisations happen outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g = step()
    for new in (second, first, second):
        for dst, src in zip((lens, k, v, table, *dev_pool), (*new, *pool)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o_g.clone(), lse_g.clone(), *[t.clone() for t in dev_pool]]
        for dst, src in zip(dev_pool, pool):
            dst.copy_(src)
        eager = [*step(), *dev_pool]
        for a, b_ in zip(replayed, eager):
            assert torch.equal(a, b_)
