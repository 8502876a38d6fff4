"""GPU: a sliding window, a softcap and attention sinks over the MXFP4 KV cache (csrc/fa_fp4_decode.hip fp4kv_split_mod_kernel,
csrc/fa_fp4_prefill.hip fp4kv_prefill_mod_kernel) through common.fp4_kvcache's mxfp4_attn_with_kvcache and
mxfp4_attn_varlen_func: against plain fp64 attention per sequence on code * 2^e * descale with the band, the cap and the sink column
written out, held to the sharp bar (tests/ex_full_ref.sharp_bar, factor 2) with the merged e4m3 featured call on the exactly widened
cache as the baseline.  q is drawn at 0.25 (rows that sum over many keys: §9zh).  Ratios are printed (profiles/fp4_mod.md)."""
import math

import pytest
import torch

from tests.ex_full_ref import Result, sharp_bar
from tests.test_fp4_kvcache_gpu import lay_out, values
from tests.test_fp4_prefill_gpu import SEQS, cu_of

pytestmark = pytest.mark.gpu
DEV, E4 = "cuda", torch.float8_e4m3fn
B, HQ, HKV, CAP, PAD = 2, 8, 2, 256, 4096
ALT = "alternating"                                               # V exponents -6 / +5 by key parity, unit K scales


def attention(q, k, v, scale, window, causal, softcap, sink):
    """one head of one sequence in fp64: q (nq, 128), k, v (nk, 128), sink a float or None -> (o, lse)"""
    nq, nk = q.shape[0], k.shape[0]
    s = scale * (q @ k.T)
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    off = torch.arange(nk)[None, :] - (torch.arange(nq)[:, None] + nk - nq)       # j - (i + nk - nq)
    left, right = window[0], 0 if causal else window[1]
    s = s.masked_fill((off < -left if left >= 0 else off < -2 ** 40) | (off > right if right >= 0 else off > 2 ** 40), -math.inf)
    if sink is not None:
        s = torch.cat((s, torch.full((nq, 1), float(sink), dtype=torch.float64)), 1)
    lse = torch.logsumexp(s, -1)
    return torch.nan_to_num(torch.exp(s - lse[:, None]))[:, :nk] @ v, lse


def cache(g, b, hkv, ev):
    """random codes and scale bytes (b, CAP, hkv, ..), their fp64 values and the exactly widened e4m3 caches"""
    kc, vc = (torch.randint(0, 256, (b, CAP, hkv, 64), generator=g, dtype=torch.uint8) for _ in range(2))
    ks = (127 + (torch.randint(-5, 6, (b, CAP, hkv, 4), generator=g) if ev != ALT else torch.zeros((b, CAP, hkv, 4), dtype=torch.int64))).to(torch.uint8)
    evs = torch.randint(-5, 6, (b, CAP, hkv), generator=g) if ev != ALT else torch.where(torch.arange(CAP) % 2 == 0, -6, 5)[None, :, None].expand(b, CAP, hkv)
    vs = (127 + evs).to(torch.uint8)
    kval, vval = values(kc, ks), values(vc, vs)
    k8, v8 = kval.to(E4), vval.to(E4)
    assert torch.equal(k8.double(), kval) and torch.equal(v8.double(), vval)   # the widening must be exact
    return (kc, ks, vc, vs, k8.view(torch.uint8), v8.view(torch.uint8)), kval, vval


def judge(tag, o, lse, ro, rl, ob, lb, sinks_rows, dtype=torch.bfloat16):
    """dead rows, finiteness and the sharp bar; rows-major tensors: o (rows, 128), lse (rows,); sinks_rows: each row's sink or None"""
    dead = torch.isinf(rl) if sinks_rows is None else rl == sinks_rows.double()   # (a sink row with visible keys has lse > sink)
    want = torch.full_like(lse, -math.inf) if sinks_rows is None else sinks_rows
    assert bool((o[dead] == 0).all()) and torch.equal(lse[dead], want[dead]) and bool(torch.isfinite(o).all())
    pack = lambda o_, l_: Result(o_.reshape(-1, 128), l_.reshape(1, -1), *[None] * 9)   # noqa: E731
    bad, ratio = sharp_bar(pack(o, lse), pack(ro, rl), pack(ob, lb), dtype)
    print(f"RATIO {tag} " + " ".join(f"{k}={v:.3f}" for k, v in ratio.items()))
    assert not bad, bad


# ---- decode: B 2, H 8 / 2, capacity 256, lengths (65, 250)

def decode_inputs(nq, layout, ev, seed, lens=(65, 250)):
    g = torch.Generator().manual_seed(seed)
    q8 = (torch.randn((B, nq, HQ, 128), generator=g) * 0.25).to(E4)
    arrays, kval, vval = cache(g, B, HKV, ev)
    qd, kd, vd = (0.2 + 0.3 * torch.rand((B, HKV), generator=g) for _ in range(3))
    arrays, kw = lay_out(layout, arrays, seed)
    kw.update(cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), q_descale=qd.to(DEV), k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    return q8, [a.to(DEV) for a in arrays], kw, kval, vval, (qd, kd, vd), (torch.randn(HQ, generator=g) * 2.0).float()


#        nq S  layout  window      causal cap  sinks ev
DECODE = [(1, 1, "bidx", (0, -1), True, 0.0, False, None), (3, 3, "ps16", (17, -1), True, 0.0, False, None),
          (1, 0, "ps16", (70, -1), True, 0.0, False, None), (3, 1, "bidx", (70, -1), True, 30.0, False, None),
          (3, 0, "bidx", (2000, -1), True, 0.0, True, None), (1, 3, "bidx", (17, 1), False, 0.0, True, None),
          (3, 1, "ps16", (17, 1), False, 30.0, True, None), (3, 3, "ps16", (-1, -1), True, 30.0, True, None),
          (1, 1, "ps16", (-1, -1), False, 30.0, False, None), (3, 3, "bidx", (70, -1), True, 0.0, False, ALT),
          (1, 1, "bidx", (17, -1), True, 0.0, False, ALT), (3, 0, "ps16", (0, -1), True, 0.0, True, None)]


@pytest.mark.parametrize("nq,splits,layout,window,causal,softcap,with_sinks,ev", DECODE, ids=[
    f"nq{c[0]}-S{c[1]}-{c[2]}-w{c[3][0]}_{c[3][1]}-c{int(c[4])}-cap{int(c[5])}-sink{int(c[6])}{'-alt' if c[7] else ''}" for c in DECODE])
def test_decode_against_fp64(nq, splits, layout, window, causal, softcap, with_sinks, ev):
    """(17, -1): the left edge inside a tile; (70, -1): lo in a later tile than 0; (2000, -1): wider than the cache; (17, 1) without
    causal: a right bound.  ALT: a masked key of ev = +5 lies just left of the band and must not move the joint maximum."""
    import flashattention_lab_cuda as ext
    from common.fp8_attention import fp8_attn_with_kvcache

    lens = (65, 250)
    q8, arrays, kw, kval, vval, (qd, kd, vd), sinks = decode_inputs(nq, layout, ev, 100 * nq + splits)
    feat = dict(softcap=softcap, sinks=sinks.to(DEV) if with_sinks else None)
    buf_o = torch.full((B * nq * HQ * 128 + 2 * PAD,), -7.0, dtype=torch.bfloat16, device=DEV)
    buf_l = torch.full((B * HQ * nq + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    o, lse = ext.fp4_kvcache_forward(q8.to(DEV), *arrays[:4], kw["cache_seqlens"], kw.get("block_table"), kw.get("cache_batch_idx"), kw["q_descale"],
                                     kw["k_descale"], kw["v_descale"], None, causal, splits, out=(buf_o[PAD:-PAD].view(B, nq, HQ, 128),
                                     buf_l[PAD:-PAD].view(B, HQ, nq)), window=window, **feat)
    ob, lb = fp8_attn_with_kvcache(q8.to(DEV), arrays[4].view(E4), arrays[5].view(E4), causal=causal, window_size=window, num_splits=splits,
                                   return_softmax_lse=True, **kw, **feat)
    torch.cuda.synchronize()
    assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))   # nothing beside the outputs
    ro, rl = torch.zeros((B, HQ, nq, 128), dtype=torch.float64), torch.zeros((B, HQ, nq), dtype=torch.float64)
    for b in range(B):
        for h in range(HQ):
            hk = h // (HQ // HKV)
            ro[b, h], rl[b, h] = attention(q8[b, :, h].double(), kval[b, :lens[b], hk], vval[b, :lens[b], hk] * vd[b, hk].double(),
                                           128 ** -0.5 * qd[b, hk].double() * kd[b, hk].double(), window, causal, softcap, sinks[h] if with_sinks else None)
    rows = sinks[None, :, None].expand(B, HQ, nq) if with_sinks else None
    judge(f"decode nq={nq} S={splits} {layout} w={window} causal={causal} cap={softcap} sinks={with_sinks} ev={ev}", o.cpu().transpose(1, 2), lse.cpu(),
          ro, rl, ob.cpu().transpose(1, 2), lb.cpu(), rows)


# ---- prefill: test_fp4_prefill_gpu.SEQS, ps 16

#          window     causal cap  sinks H_q H_kv
PREFILL = [((0, -1), True, 0.0, False, 8, 2), ((17, -1), True, 0.0, False, 8, 2), ((70, -1), True, 0.0, False, 8, 2),
           ((70, -1), True, 0.0, False, 2, 2), ((2000, -1), True, 0.0, True, 8, 2), ((17, 1), False, 0.0, False, 8, 2),
           ((-1, -1), True, 30.0, False, 8, 2), ((-1, -1), False, 0.0, True, 2, 2), ((17, 1), False, 30.0, True, 8, 2),
           ((70, -1), True, 30.0, True, 2, 2)]


def prefill_inputs(hq, hkv, seed, ev=None):
    g = torch.Generator().manual_seed(seed)
    nseq, ps = len(SEQS), 16
    nb = CAP // ps
    q8 = (torch.randn((sum(s[0] for s in SEQS), hq, 128), generator=g) * 0.25).to(E4)
    arrays, kval, vval = cache(g, nseq, hkv, ev)
    qd, kd, vd = (0.2 + 0.3 * torch.rand((nseq, hkv), generator=g) for _ in range(3))
    table = torch.randperm(nseq * nb + 3, generator=g)[:nseq * nb].reshape(nseq, nb).to(torch.int32)   # a shuffled pool with spare pages
    pools = []
    for a in arrays:
        pool = torch.zeros((nseq * nb + 3, ps, *a.shape[2:]), dtype=torch.uint8)
        pool[table.reshape(-1).long()] = a.reshape(nseq * nb, ps, *a.shape[2:])
        pools.append(pool.to(DEV))
    cu = [torch.tensor(cu_of([s[i] for s in SEQS]), dtype=torch.int32, device=DEV) for i in (0, 1)]
    kw = dict(block_table=table.to(DEV), q_descale=qd.to(DEV), k_descale=kd.to(DEV), v_descale=vd.to(DEV), return_softmax_lse=True)
    return q8, pools, cu, kw, kval, vval, (qd, kd, vd), (torch.randn(hq, generator=g) * 2.0).float()


@pytest.mark.parametrize("window,causal,softcap,with_sinks,hq,hkv", PREFILL, ids=[
    f"w{c[0][0]}_{c[0][1]}-c{int(c[1])}-cap{int(c[2])}-sink{int(c[3])}-H{c[4]}_{c[5]}" for c in PREFILL])
def test_prefill_against_fp64(window, causal, softcap, with_sinks, hq, hkv):
    """(70, -1) on the (129, 200) sequence: the waves of a workgroup start at different tiles; (17, 1) without causal: kend and whi
    follow the right bound.  The call writes into -7-filled buffers with three rows of no sequence at the end."""
    import flashattention_lab_cuda as ext
    from common.fp8_attention import fp8_attn_varlen_func

    q8, pools, cu, kw, kval, vval, (qd, kd, vd), sinks = prefill_inputs(hq, hkv, hq)
    total, spare, max_q = q8.shape[0], 3, max(s[0] for s in SEQS)
    feat = dict(softcap=softcap, sinks=sinks.to(DEV) if with_sinks else None)
    buf_o = torch.full(((total + spare) * hq * 128 + 2 * PAD,), -7.0, dtype=torch.bfloat16, device=DEV)
    buf_l = torch.full((hq * (total + spare) + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    o, lse = buf_o[PAD:-PAD].view(total + spare, hq, 128), buf_l[PAD:-PAD].view(hq, total + spare)
    qpad = torch.cat((q8.to(DEV), torch.zeros((spare, hq, 128), dtype=E4, device=DEV)))
    ext.fp4_varlen_forward(qpad, *pools[:4], *cu, max_q, CAP, kw["block_table"], kw["q_descale"], kw["k_descale"], kw["v_descale"], None, causal,
                           out=(o, lse), window=window, **feat)
    ob, lb = fp8_attn_varlen_func(q8.to(DEV), pools[4].view(E4), pools[5].view(E4), *cu, max_q, CAP, causal=causal, window_size=window, **kw, **feat)
    torch.cuda.synchronize()
    assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))   # nothing beside the outputs
    assert bool((o[total:] == -7.0).all()) and bool((lse[:, total:] == -7.0).all())                              # rows of no sequence
    ro, rl, st = torch.zeros((hq, total, 128), dtype=torch.float64), torch.zeros((hq, total), dtype=torch.float64), 0
    for b, (nq, nk) in enumerate(SEQS):
        for h in range(hq):
            hk = h // (hq // hkv)
            ro[h, st:st + nq], rl[h, st:st + nq] = attention(q8[st:st + nq, h].double(), kval[b, :nk, hk], vval[b, :nk, hk] * vd[b, hk].double(),
                                                             128 ** -0.5 * qd[b, hk].double() * kd[b, hk].double(), window, causal, softcap,
                                                             sinks[h] if with_sinks else None)
        st += nq
    rows = sinks[:, None].expand(hq, total) if with_sinks else None
    judge(f"prefill w={window} causal={causal} cap={softcap} sinks={with_sinks} H={hq}/{hkv}", o[:total].cpu().transpose(0, 1), lse[:, :total].cpu(),
          ro, rl, ob.cpu().transpose(0, 1), lb.cpu(), rows)


# ---- what both calls share

def test_sink_edges_and_the_default_arguments():
    """every sink head at -inf: the bits of the call without sinks (decode: at the same split count); +-1e4: finite o and lse; the
    default arguments through the new functions: the bits and the routes of the older wrappers"""
    import flashattention_lab_cuda as ext
    from common.fp4_kvcache import (fp8_attn_varlen_with_mxfp4_kvcache, fp8_attn_with_mxfp4_kvcache, mxfp4_attn_varlen_func,
                                    mxfp4_attn_with_kvcache)

    q8, arrays, kw, *_ = decode_inputs(3, "ps16", None, 7)
    dec = lambda f, **more: f(q8.to(DEV), *arrays[:4], causal=True, num_splits=3, return_softmax_lse=True, **kw, **more)   # noqa: E731
    p8, pools, cu, pkw, *_ = prefill_inputs(8, 2, 8)
    pre = lambda f, **more: f(p8.to(DEV), *pools[:4], *cu, 129, CAP, causal=True, **pkw, **more)                            # noqa: E731
    total = p8.shape[0]
    for call, new, old, routes in ((dec, mxfp4_attn_with_kvcache, fp8_attn_with_mxfp4_kvcache, (b"fp4kv_split", b"fp4kv_split_mod")),
                                   (pre, mxfp4_attn_varlen_func, fp8_attn_varlen_with_mxfp4_kvcache, (b"fp4kv_prefill", b"fp4kv_prefill_mod"))):
        plain = call(new, window_size=(70, -1), softcap=30.0)
        gone = call(new, window_size=(70, -1), softcap=30.0, sinks=torch.full((HQ,), -math.inf, device=DEV))
        assert all(torch.equal(a, b_) for a, b_ in zip(plain, gone))
        for big in (1e4, -1e4):
            o, lse = call(new, window_size=(70, -1), sinks=torch.full((HQ,), big, device=DEV))
            assert bool(torch.isfinite(o[:total]).all()) and bool(torch.isfinite(lse[..., :total] if call is pre else lse).all())
        before = [ext._lib.fa_route_count(r) for r in routes]
        same = call(new, window_size=(-1, -1), softcap=0.0, sinks=None)
        assert [ext._lib.fa_route_count(r) for r in routes] == [before[0] + 1, before[1]]
        assert all(torch.equal(a, b_) for a, b_ in zip(same, call(old)))


def test_graph_replay_after_the_state_changed():
    """append + windowed decode with sinks from one graph, replayed after lengths, table and sink values changed in place"""
    from common.fp4_kvcache import mxfp4_attn_with_kvcache, mxfp4_kvcache_append

    g = torch.Generator().manual_seed(5)
    ps, nnew = 16, 5
    nb = CAP // ps
    pool = [torch.randint(0, 256, (B * nb, ps, HKV, 64), generator=g, dtype=torch.uint8), torch.randint(122, 133, (B * nb, ps, HKV, 4), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (B * nb, ps, HKV, 64), generator=g, dtype=torch.uint8), torch.randint(122, 133, (B * nb, ps, HKV), generator=g, dtype=torch.uint8)]
    state = lambda s: (torch.tensor(((13, 60), (77, 190))[s], dtype=torch.int32), (torch.randn((B, nnew, HKV, 128), generator=g) * (1 + s)).bfloat16(),   # noqa: E731
                       (torch.randn((B, nnew, HKV, 128), generator=g) * (2 - s)).bfloat16(),
                       torch.randperm(B * nb, generator=g).reshape(B, nb).to(torch.int32), torch.randn(HQ, generator=g) * (1 + 2 * s))
    first, second = state(0), state(1)
    lens, k, v, table, sinks = (t.to(DEV) for t in first)
    q8 = (torch.randn((B, 3, HQ, 128), generator=g) * 0.25).to(E4).to(DEV)
    dev_pool = [t.to(DEV) for t in pool]

    def step():
        mxfp4_kvcache_append(k, v, *dev_pool, cache_seqlens=lens, block_table=table)
        return mxfp4_attn_with_kvcache(q8, *dev_pool, cache_seqlens=lens + nnew, block_table=table, causal=True, window_size=(70, -1),
                                       sinks=sinks, num_splits=3, return_softmax_lse=True)

    step()                                                        # (the workspace and the lazy initialisations happen outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g = step()
    for new in (second, first, second):
        for dst, src in zip((lens, k, v, table, sinks, *dev_pool), (*new, *pool)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o_g.clone(), lse_g.clone(), *[t.clone() for t in dev_pool]]
        for dst, src in zip(dev_pool, pool):
            dst.copy_(src)
        for a, b_ in zip(replayed, [*step(), *dev_pool]):
            assert torch.equal(a, b_)
