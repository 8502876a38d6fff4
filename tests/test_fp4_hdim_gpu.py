"""GPU: the MXFP4 KV cache at head dims 64 and 256 (csrc/fa_fp4_decode.hip, csrc/fa_fp4_prefill.hip) through common.mxfp4_attention.

  * the append bit for bit against the rule restated here in torch at width d, untouched bytes included;
  * decode and prefill against fp64 attention on code * 2^e * descale, held to the sharp bar (tests/ex_full_ref.sharp_bar, factor 2)
    with the e4m3 call of common.fp8_attention at the same d on the exactly widened cache as the baseline;
  * untrusted lengths, table entries, rows and scale bytes with guarded outputs; append + decode replayed from one graph.
The kernel / baseline ratios are printed per case (profiles/fp4_hdim.md records a run)."""
import math

import pytest
import torch

from tests.ex_full_ref import Result, sharp_bar
from tests.test_fp4_kvcache_gpu import lay_out
from tests.test_fp4_mod_gpu import attention
from tests.test_fp4_prefill_gpu import SEQS, cu_of

pytestmark = pytest.mark.gpu
DEV, E4 = "cuda", torch.float8_e4m3fn
MAGS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
E2M1 = torch.cat((MAGS, -MAGS))                                  # code s eem
B, HQ, HKV, CAP, PS, PAD = 2, 8, 2, 256, 16, 4096
DIMS = pytest.mark.parametrize("d", (64, 256))
TIES = [6.0, 2.5, 5.0, 0.25, -2.5, -0.25, -5.0, 0.75]             # amax 6 (x' = 12 = 6 * 2^1 under a descale of 0.5) and the three ties


def values(codes, scale):
    """(.., H, d / 2) code bytes and (.., H, nb) E8M0 bytes -> (.., H, d) float64 code * 2^(byte - 127), nb blocks a head"""
    x = E2M1[torch.stack((codes & 15, codes >> 4), -1).flatten(-2).long()]
    e = (scale.double() - 127.0).reshape(*codes.shape[:-1], -1)
    return x * torch.exp2(e).repeat_interleave(x.shape[-1] // e.shape[-1], -1)


def append_model(x, descale, block):
    """the append rule: x (.., H, d) 16-bit, descale broadcastable to (.., H, 1) -> (codes (.., H, d / 2), bytes (.., H, d / block))"""
    d = x.shape[-1]
    xp = (x.float() * (1.0 / descale.float())).reshape(*x.shape[:-1], d // block, block)
    amax = xp.abs().amax(-1)
    m, ex = torch.frexp(amax)                                    # amax = m 2^ex, m in [.5, 1): 6 * 2^e = .75 * 2^(e + 3)
    e = torch.where(amax == 0, torch.zeros_like(ex), ex - 3 + (m > 0.75).int()).clamp(-64, 64)
    y = xp.double() * torch.exp2(-e.double()).unsqueeze(-1)
    near = (y.abs().unsqueeze(-1) - MAGS).abs()
    is_min = near == near.amin(-1, keepdim=True)                 # a tie: two codes, the even one wins
    code = ((is_min * torch.tensor([2, 1] * 4)).argmax(-1) + 8 * (y < 0)).reshape(*x.shape[:-1], d // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8), (e + 127).to(torch.uint8)


def cache(g, b, hkv, d, ek=None, ev=None, shift=0):
    """random codes with scale exponents from [-5, 5] (or ek / ev): the four arrays and the exactly widened e4m3 caches (V's by
    2^shift) as (b, CAP, ..) uint8, and the fp64 values"""
    kc, vc = (torch.randint(0, 256, (b, CAP, hkv, d // 2), generator=g, dtype=torch.uint8) for _ in range(2))
    ks = (127 + (torch.randint(-5, 6, (b, CAP, hkv, d // 32), generator=g) if ek is None else ek)).to(torch.uint8)
    vs = (127 + (torch.randint(-5, 6, (b, CAP, hkv), generator=g) if ev is None else ev)).to(torch.uint8)
    kval, vval = values(kc, ks), values(vc, vs)
    k8, v8 = kval.to(E4), (vval * 2.0 ** shift).to(E4)
    assert torch.equal(k8.double(), kval) and torch.equal(v8.double(), vval * 2.0 ** shift)   # the widening must be exact
    return (kc, ks, vc, vs, k8.view(torch.uint8), v8.view(torch.uint8)), kval, vval


def judge(tag, d, o, lse, ro, rl, ob, lb, sink_rows=None, dtype=torch.bfloat16):
    """dead rows, finiteness and the sharp bar on rows-major tensors: o (.., d), lse (..); sink_rows: each row's sink, or None"""
    dead = torch.isinf(rl) if sink_rows is None else rl == sink_rows.double()
    want = torch.full_like(lse, -math.inf) if sink_rows is None else sink_rows
    assert bool((o[dead] == 0).all()) and torch.equal(lse[dead], want[dead]) and bool(torch.isfinite(o).all())
    pack = lambda o_, l_: Result(o_.reshape(-1, d), l_.reshape(1, -1), *[None] * 9)   # noqa: E731
    bad, ratio = sharp_bar(pack(o, lse), pack(ro, rl), pack(ob, lb), dtype)
    print(f"RATIO d={d} {tag} " + " ".join(f"{k}={v:.3f}" for k, v in ratio.items()))
    assert not bad, bad


# ---- 1. the append, bit for bit

@DIMS
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=("f16", "bf16"))
@pytest.mark.parametrize("nnew", (1, 5))
@pytest.mark.parametrize("layout", ("bidx", "ps16"))
def test_append_bits(layout, nnew, dtype, d):
    """lengths (0, 13) of capacity 16: with 5 new tokens the last two of sequence 1 are dropped.  Token 0 of head 0 holds an all-zero
    first K block, the TIES block next, and in V the TIES block LAST among small values (at 256 a maximum over four lanes misses it);
    head 1's first V block is large, and must not reach head 0's scale (at 64 its lanes are the next two)."""
    from common.mxfp4_attention import mxfp4_append

    cap, lens, nb = 16, (0, 13), d // 32
    g = torch.Generator().manual_seed(nnew)
    k, v = ((torch.randn((B, nnew, HKV, d), generator=g) * 3.0).to(dtype) for _ in range(2))
    k[0, 0, 0, :32] = 0.0
    k[0, 0, 0, 32:64] = torch.tensor(TIES * 4)
    v[0, 0, 0] = 0.125 * torch.randn(d, generator=g)
    v[0, 0, 0, -32:] = torch.tensor(TIES * 4)
    v[0, 0, 1, :32] = 100.0
    v[1, 0, 1] = 0.0
    kd, vd = torch.tensor([[0.5, 0.3], [1.7, 2.0]]), torch.tensor([[0.5, 1.1], [0.7, 3.0]])
    kcode, kbyte = append_model(k, kd[:, None, :, None], 32)
    vcode, vbyte = append_model(v, vd[:, None, :, None], d)
    assert kbyte[0, 0, 0, 0] == 127 and kbyte[0, 0, 0, 1] == 128 and vbyte[0, 0, 0, 0] == 128 and vbyte[1, 0, 1, 0] == 127
    rows, kw = (2, 0), dict(cache_batch_idx=torch.tensor([2, 0], dtype=torch.int32, device=DEV))
    lead = (3, cap)
    if layout == "ps16":
        rows, kw, lead = (3, 1), dict(block_table=torch.tensor([[3], [1]], dtype=torch.int32, device=DEV)), (5, PS)
    before = [torch.randint(0, 256, (*lead, HKV, *w), generator=g, dtype=torch.uint8) for w in ((d // 2,), (nb,), (d // 2,), ())]
    want = [t.clone() for t in before]
    for b in range(B):
        for i in range(nnew):
            if lens[b] + i < cap:
                for t, new in zip(want, (kcode, kbyte, vcode, vbyte[..., 0])):
                    t[rows[b], lens[b] + i] = new[b, i]
    got = [t.to(DEV) for t in before]
    mxfp4_append(k.to(DEV), v.to(DEV), *got, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), k_descale=kd.to(DEV),
                 v_descale=vd.to(DEV), **kw)
    for name, a, w in zip(("k_cache", "k_scale", "v_cache", "v_scale"), got, want):
        assert torch.equal(a.cpu(), w), (name, (a.cpu() != w).nonzero()[:4])


# ---- 2. decode against fp64

def decode(d, nq, lens, splits, layout, dtype=torch.bfloat16, causal=False, window=(-1, -1), softcap=0.0, nsink=0, ek=None, ev=None,
           shift=0, seed=0, call_lens=None, spoil=None):
    """one decode call against fp64 and the e4m3 baseline.  shift: the baseline's V is widened by 2^shift under v_descale * 2^-shift;
    nsink: 0, or the sinks tensor's length (1 or HQ); call_lens: what the call is handed; spoil(keywords, kval, vval)."""
    from common.fp8_attention import fp8_attn_with_kvcache
    from common.mxfp4_attention import mxfp4_decode

    g = torch.Generator().manual_seed(1000 * nq + 10 * splits + seed + d)
    q8 = (torch.randn((B, nq, HQ, d), generator=g) * 0.25).to(E4)
    arrays, kval, vval = cache(g, B, HKV, d, ek, ev, shift)
    qd, kd, vd = (0.2 + 0.3 * torch.rand((B, HKV), generator=g) for _ in range(3))
    sinks = (torch.randn(HQ, generator=g) * 2.0).float()
    arrays, kw = lay_out(layout, arrays, seed)
    if spoil is not None:
        spoil(kw, kval, vval)
    arrays = [a.to(DEV) for a in arrays]
    kw.update(cache_seqlens=torch.tensor(call_lens or lens, dtype=torch.int32, device=DEV), q_descale=qd.to(DEV), k_descale=kd.to(DEV),
              causal=causal, window_size=window, softcap=softcap, sinks=sinks.to(DEV) if nsink else None, num_splits=splits, out_dtype=dtype,
              return_softmax_lse=True)
    o, lse = mxfp4_decode(q8.to(DEV), *arrays[:4], v_descale=vd.to(DEV), **kw)
    ob, lb = fp8_attn_with_kvcache(q8.to(DEV), arrays[4].view(E4), arrays[5].view(E4), v_descale=(vd * 2.0 ** -shift).to(DEV), **kw)
    ro, rl = torch.zeros((B, HQ, nq, d), dtype=torch.float64), torch.zeros((B, HQ, nq), dtype=torch.float64)
    for b in range(B):
        for h in range(HQ):
            hk = h // (HQ // HKV)
            ro[b, h], rl[b, h] = attention(q8[b, :, h].double(), kval[b, :lens[b], hk], vval[b, :lens[b], hk] * vd[b, hk].double(),
                                           d ** -0.5 * qd[b, hk].double() * kd[b, hk].double(), window, causal, softcap, sinks[h] if nsink else None)
    judge(f"decode nq={nq} lens={lens} S={splits} {layout} w={window} cap={softcap} sinks={nsink} shift={shift}", d, o.cpu().transpose(1, 2),
          lse.cpu(), ro, rl, ob.cpu().transpose(1, 2), lb.cpu(), sinks[None, :, None].expand(B, HQ, nq) if nsink else None, dtype)


CASES = [(nq, (65, 200), s, layout, torch.float16 if (nq, s, layout) == (9, 3, "contig") else torch.bfloat16)
         for nq in (1, 9) for s in (1, 3) for layout in ("contig", "bidx", "ps16")]
CASES += [(9, (1, 64), 3, "ps16", torch.bfloat16), (1, (1, 64), 1, "contig", torch.bfloat16)]


@DIMS
@pytest.mark.parametrize("nq,lens,splits,layout,dtype", CASES, ids=[f"nq{c[0]}-{c[1][0]}_{c[1][1]}-S{c[2]}-{c[3]}-{str(c[4])[6:]}" for c in CASES])
def test_decode_against_fp64(nq, lens, splits, layout, dtype, d):
    decode(d, nq, lens, splits, layout, dtype, causal=nq > 1)


@DIMS
@pytest.mark.parametrize("which", ("all_minus_20", "alternating", "window", "softcap", "sinks1", "sinks3", "scale_row"))
def test_decode_scales_and_features(which, d):
    """every ev = -20: P' must still peak at 1; ev alternating -6 / +5 under unit K scales: both kinds of key in a tile; one case a
    feature ((17, -1): the left edge inside a tile; sinks at S = 1, raised to 2 by the library, and at S = 3); scale_row: K exponents
    +4 in the first half of a head's blocks and -4 in the second (at 256, blocks 4 - 7 lie in the row's second dword)."""
    nb = d // 32
    if which == "all_minus_20":
        decode(d, 1, (65, 200), 3, "contig", ev=torch.full((B, CAP, HKV), -20), shift=20)
    elif which == "alternating":
        ev = torch.where(torch.arange(CAP) % 2 == 0, -6, 5)[None, :, None].expand(B, CAP, HKV)
        decode(d, 1, (65, 200), 1, "contig", ek=torch.zeros((B, CAP, HKV, nb), dtype=torch.int64), ev=ev)
    elif which == "window":
        decode(d, 9, (65, 200), 3, "ps16", causal=True, window=(17, -1))
    elif which == "softcap":
        decode(d, 9, (65, 200), 1, "bidx", causal=True, softcap=30.0)
    elif which in ("sinks1", "sinks3"):
        decode(d, 9, (65, 200), int(which[-1]), "ps16", causal=True, nsink=HQ)
    else:
        ek = torch.where(torch.arange(nb) < nb // 2, 4, -4).expand(B, CAP, HKV, nb)
        decode(d, 1, (65, 200), 1, "contig", ek=ek)


# ---- 3. prefill against fp64

PREFILL = [((-1, -1), False, False, 8, 2), ((-1, -1), True, False, 8, 2), ((-1, -1), True, False, 2, 2), ((-1, -1), False, False, 2, 2),
           ((70, -1), True, False, 8, 2), ((-1, -1), True, True, 8, 2)]


@DIMS
@pytest.mark.parametrize("window,causal,with_sinks,hq,hkv", PREFILL, ids=[f"w{c[0][0]}-c{int(c[1])}-sink{int(c[2])}-H{c[3]}_{c[4]}" for c in PREFILL])
def test_prefill_against_fp64(window, causal, with_sinks, hq, hkv, d):
    """test_fp4_prefill_gpu's sequences in a shuffled pool of 16-token pages; the call writes into -7-filled buffers with three rows
    of no sequence at the end"""
    from common.fp8_attention import fp8_attn_varlen_func
    from common.mxfp4_attention import mxfp4_prefill
    import flashattention_lab_cuda as ext

    g = torch.Generator().manual_seed(hq + d)
    nseq, nb = len(SEQS), CAP // PS
    q8 = (torch.randn((sum(s[0] for s in SEQS), hq, d), generator=g) * 0.25).to(E4)
    arrays, kval, vval = cache(g, nseq, hkv, d)
    qd, kd, vd = (0.2 + 0.3 * torch.rand((nseq, hkv), generator=g) for _ in range(3))
    sinks = (torch.randn(hq, generator=g) * 2.0).float()
    table = torch.randperm(nseq * nb + 3, generator=g)[:nseq * nb].reshape(nseq, nb).to(torch.int32)
    pools = []
    for a in arrays:
        pool = torch.zeros((nseq * nb + 3, PS, *a.shape[2:]), dtype=torch.uint8)
        pool[table.reshape(-1).long()] = a.reshape(nseq * nb, PS, *a.shape[2:])
        pools.append(pool.to(DEV))
    cu = [torch.tensor(cu_of([s[i] for s in SEQS]), dtype=torch.int32, device=DEV) for i in (0, 1)]
    kw = dict(block_table=table.to(DEV), q_descale=qd.to(DEV), k_descale=kd.to(DEV), v_descale=vd.to(DEV), causal=causal, window_size=window,
              sinks=sinks.to(DEV) if with_sinks else None, return_softmax_lse=True)
    total, spare, max_q = q8.shape[0], 3, max(s[0] for s in SEQS)
    buf_o = torch.full(((total + spare) * hq * d + 2 * PAD,), -7.0, dtype=torch.bfloat16, device=DEV)
    buf_l = torch.full((hq * (total + spare) + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    o, lse = buf_o[PAD:-PAD].view(total + spare, hq, d), buf_l[PAD:-PAD].view(hq, total + spare)
    qpad = torch.cat((q8.to(DEV), torch.zeros((spare, hq, d), dtype=E4, device=DEV)))
    ext.fp4_varlen_forward(qpad, *pools[:4], *cu, max_q, CAP, kw["block_table"], kw["q_descale"], kw["k_descale"], kw["v_descale"], None, causal,
                           out=(o, lse), window=window, sinks=kw["sinks"], hdim=True)
    o2, lse2 = mxfp4_prefill(q8.to(DEV), *pools[:4], *cu, max_q, CAP, **kw)
    ob, lb = fp8_attn_varlen_func(q8.to(DEV), pools[4].view(E4), pools[5].view(E4), *cu, max_q, CAP, **kw)
    torch.cuda.synchronize()
    assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))   # nothing beside the outputs
    assert bool((o[total:] == -7.0).all()) and bool((lse[:, total:] == -7.0).all())                              # rows of no sequence
    assert torch.equal(o[:total], o2) and torch.equal(lse[:, :total], lse2)                                      # the module is the shim call
    ro, rl, st = torch.zeros((hq, total, d), dtype=torch.float64), torch.zeros((hq, total), dtype=torch.float64), 0
    for b, (nq, nk) in enumerate(SEQS):
        for h in range(hq):
            hk = h // (hq // hkv)
            ro[h, st:st + nq], rl[h, st:st + nq] = attention(q8[st:st + nq, h].double(), kval[b, :nk, hk], vval[b, :nk, hk] * vd[b, hk].double(),
                                                             d ** -0.5 * qd[b, hk].double() * kd[b, hk].double(), window, causal, 0.0,
                                                             sinks[h] if with_sinks else None)
        st += nq
    judge(f"prefill w={window} causal={causal} sinks={with_sinks} H={hq}/{hkv}", d, o[:total].cpu().transpose(0, 1), lse[:, :total].cpu(), ro, rl,
          ob.cpu().transpose(0, 1), lb.cpu(), sinks[:, None].expand(hq, total) if with_sinks else None)


# ---- 4. untrusted inputs with guarded outputs, and append + decode from one graph

@DIMS
def test_decode_untrusted_inputs(d):
    def bad_page(kw, kval, vval):                                 # pages outside the pool: zero codes, unit scales
        kw["block_table"][1, 2], kw["block_table"][0, 1] = 10 ** 6, -1
        kval[1, 32:48], vval[1, 32:48], kval[0, 16:32], vval[0, 16:32] = 0.0, 0.0, 0.0, 0.0

    def bad_row(kw, kval, vval):
        kw["cache_batch_idx"][1] = 3

    decode(d, 1, (CAP, 0), 3, "contig", call_lens=(CAP + 50, -3))
    decode(d, 9, (65, 200), 1, "ps16", causal=True, spoil=bad_page)
    decode(d, 1, (65, 0), 1, "bidx", call_lens=(65, 200), spoil=bad_row)
    import flashattention_lab_cuda as ext
    g = torch.Generator().manual_seed(4)
    q8 = torch.randn((B, 9, HQ, d), generator=g).to(E4).to(DEV)
    kc, vc = (torch.randint(0, 256, (B, CAP, HKV, d // 2), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    ks, vs = torch.full((B, CAP, HKV, d // 32), 0xFF, dtype=torch.uint8, device=DEV), torch.full((B, CAP, HKV), 0xFF, dtype=torch.uint8, device=DEV)
    lens = torch.tensor([2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    for splits in (1, 3):
        n_o, n_l = B * 9 * HQ * d, B * HQ * 9
        buf_o = torch.full((n_o + 2 * PAD,), -7.0, dtype=torch.bfloat16, device=DEV)
        buf_l = torch.full((n_l + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
        out = (buf_o[PAD:-PAD].view(B, 9, HQ, d), buf_l[PAD:-PAD].view(B, HQ, 9))
        ext.fp4_kvcache_forward(q8, kc, ks, vc, vs, lens, causal=True, num_splits=splits, out=out, hdim=True)   # (0xFF scales: any numbers)
        torch.cuda.synchronize()
        assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))
        assert bool((out[0][1] == 0).all()) and bool((out[1][1] == -math.inf).all())


@DIMS
def test_prefill_untrusted_inputs(d):
    """offsets past the packed tokens and backwards, lengths past the capacity, table entries -1 and 10^6, 0xFF scale bytes: any
    numbers, nothing written beside the outputs"""
    import flashattention_lab_cuda as ext
    g = torch.Generator().manual_seed(6)
    nb, total, hq = CAP // PS, 70, 8
    q8 = torch.randn((total, hq, d), generator=g).to(E4).to(DEV)
    kc, vc = (torch.randint(0, 256, (2 * nb, PS, HKV, d // 2), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    ks, vs = torch.full((2 * nb, PS, HKV, d // 32), 0xFF, dtype=torch.uint8, device=DEV), torch.full((2 * nb, PS, HKV), 0xFF, dtype=torch.uint8, device=DEV)
    table = torch.arange(2 * nb, dtype=torch.int32).reshape(2, nb)
    table[0, 1], table[1, 0] = -1, 10 ** 6
    cu_q = torch.tensor([0, 40, 4000], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0, 10 ** 6, 10 ** 6 - 5], dtype=torch.int32, device=DEV)
    buf_o = torch.full((total * hq * d + 2 * PAD,), -7.0, dtype=torch.bfloat16, device=DEV)
    buf_l = torch.full((hq * total + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    ext.fp4_varlen_forward(q8, kc, ks, vc, vs, cu_q, cu_k, 64, CAP, table.to(DEV), causal=True, window=(70, -1),
                           out=(buf_o[PAD:-PAD].view(total, hq, d), buf_l[PAD:-PAD].view(hq, total)), hdim=True)
    torch.cuda.synchronize()
    assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))


@DIMS
def test_append_untrusted_inputs(d):
    """lengths past the capacity and negative, table entries -1 and 10^6, a row outside the cache: those tokens are dropped and no byte
    outside the slots of the two tokens that fit (sequence 1 at length 14 of 16) changes"""
    from common.mxfp4_attention import mxfp4_append
    g = torch.Generator().manual_seed(7)
    k, v = (torch.randn((B, 3, HKV, d), generator=g).bfloat16().to(DEV) for _ in range(2))
    for kw, lead in ((dict(cache_batch_idx=torch.tensor([7, 1], dtype=torch.int32)), (3, 16)), (dict(block_table=torch.tensor([[-1], [10 ** 6]], dtype=torch.int32)), (4, PS))):
        before = [torch.randint(0, 256, (*lead, HKV, *w), generator=g, dtype=torch.uint8) for w in ((d // 2,), (d // 32,), (d // 2,), ())]
        for lens in ((5, 2 ** 31 - 1), (-2 ** 31, 14)):
            got = [t.to(DEV) for t in before]
            mxfp4_append(k, v, *got, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), **{n: t.to(DEV) for n, t in kw.items()})
            for a, w in zip(got, before):
                a, w = a.cpu(), w.clone()
                if "cache_batch_idx" in kw and lens[1] < 16:      # sequence 1 -> row 1, positions max(len, 0) ..: the one place a token may land
                    a[1, max(lens[1], 0):max(lens[1], 0) + 3], w[1, max(lens[1], 0):max(lens[1], 0) + 3] = 0, 0
                assert torch.equal(a, w)


@DIMS
def test_graph_replay_after_the_state_changed(d):
    from common.mxfp4_attention import mxfp4_append, mxfp4_decode

    g = torch.Generator().manual_seed(5)
    nb, nnew = CAP // PS, 5
    pool = [torch.randint(*r, (B * nb, PS, HKV, *w), generator=g, dtype=torch.uint8)
            for r, w in (((0, 256), (d // 2,)), ((122, 133), (d // 32,)), ((0, 256), (d // 2,)), ((122, 133), ()))]
    state = lambda s: (torch.tensor(((13, 60), (77, 190))[s], dtype=torch.int32), (torch.randn((B, nnew, HKV, d), generator=g) * (1 + s)).bfloat16(),   # noqa: E731
                       (torch.randn((B, nnew, HKV, d), generator=g) * (2 - s)).bfloat16(),
                       torch.randperm(B * nb, generator=g).reshape(B, nb).to(torch.int32))
    first, second = state(0), state(1)
    lens, k, v, table = (t.to(DEV) for t in first)
    q8 = torch.randn((B, 1, HQ, d), generator=g).to(E4).to(DEV)
    dev_pool = [t.to(DEV) for t in pool]

    def step():
        mxfp4_append(k, v, *dev_pool, cache_seqlens=lens, block_table=table)
        return mxfp4_decode(q8, *dev_pool, cache_seqlens=lens + nnew, block_table=table, num_splits=3, window_size=(70, -1), return_softmax_lse=True)

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
