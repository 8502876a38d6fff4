"""GPU: chunked prefill over the paged MXFP4 KV cache (csrc/fa_fp4_prefill.hip) against fp64 attention per sequence
on code * 2^e * descale, held to the sharp bar (tests/ex_full_ref.sharp_bar, factor 2) with the merged fp8_attn_varlen_func(block_table=)
on the exactly widened e4m3 pool as the baseline, outputs inside -7-filled guard buffers; ratios printed (profiles/fp4_prefill.md)."""
import math

import pytest
import torch

from tests.ex_full_ref import Result, sharp_bar
from tests.test_fp4_kvcache_gpu import values

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
# (nq, nk): one row; across a wave and a key tile; across a workgroup's rows and a ragged page; no query; no key; dead causal rows
SEQS = ((1, 1), (33, 65), (129, 200), (0, 40), (40, 0), (50, 20))
B, CAP, PAD = len(SEQS), 256, 4096


def cu_of(lens):
    return [0] + torch.tensor(lens).cumsum(0).tolist()


def cu_range(cu, b, total, cap):   # kv_cu_range (csrc/fa_decode_common.h): the clamp of one sequence's untrusted offsets
    start = min(max(cu[b], 0), total)
    return start, min(max(cu[b + 1] - cu[b], 0), min(cap, total - start))


def check(causal, hq=8, hkv=2, ps=16, dtype=torch.bfloat16, ek=None, ev=None, base_shift=0, cu_q=None, cu_k=None, total_q=None,
          bad_pages=(), seed=0):
    """one call against fp64 and the e4m3 baseline.  ek / ev, base_shift: as in test_fp4_kvcache_gpu.check; cu_q / cu_k / total_q: the
    untrusted offsets (the baseline gets their clamped form); bad_pages: ((b, page, entry), ..) table entries outside the pool."""
    import flashattention_lab_cuda as ext
    from common.fp8_attention import fp8_attn_varlen_func

    g = torch.Generator().manual_seed(seed)
    cu_q, cu_k = cu_q or cu_of([s[0] for s in SEQS]), cu_k or cu_of([s[1] for s in SEQS])
    total_q, nb, max_q = total_q or cu_q[-1], CAP // ps, max(s[0] for s in SEQS)
    qs = [cu_range(cu_q, b, total_q, max_q) for b in range(B)]                 # (start, nq) and nk, clamped as the device clamps them
    nks = [cu_range(cu_k, b, 2 ** 31 - 1, CAP)[1] for b in range(B)]
    # q at 0.25: scores of about one nat of spread, every row a sum over many keys.  (Drawn at 1.5 the rows are one-hot; the largest
    # error of either kernel is then ONE rounding of one late key's P, up to 2^-4 |o| under the lazy rescale both share, and the ratio
    # of two such maxima is luck: profiles/fp4_prefill.md.)
    qkv8 = (torch.randn((total_q, 3, hq, 128), generator=g) * 0.25).to(E4)
    kc, vc = (torch.randint(0, 256, (B, CAP, hkv, 64), generator=g, dtype=torch.uint8) for _ in range(2))
    ks = (127 + (torch.randint(-5, 6, (B, CAP, hkv, 4), generator=g) if ek is None else ek)).to(torch.uint8)
    vs = (127 + (torch.randint(-5, 6, (B, CAP, hkv), generator=g) if ev is None else ev)).to(torch.uint8)
    qd, kd, vd = (0.2 + 0.3 * torch.rand((B, hkv), generator=g) for _ in range(3))
    kval, vval = values(kc, ks), values(vc, vs)
    k8, v8 = kval.to(E4), (vval * 2.0 ** base_shift).to(E4)                    # the widening must be exact
    assert torch.equal(k8.double(), kval) and torch.equal(v8.double(), vval * 2.0 ** base_shift)
    table = torch.randperm(B * nb + 3, generator=g)[:B * nb].reshape(B, nb).to(torch.int32)   # a shuffled pool with spare pages
    pools = []
    for a in (kc, ks, vc, vs, k8.view(torch.uint8), v8.view(torch.uint8)):
        pool = torch.zeros((B * nb + 3, ps, *a.shape[2:]), dtype=torch.uint8)
        pool[table.reshape(-1).long()] = a.reshape(B * nb, ps, *a.shape[2:])
        pools.append(pool.to(DEV))
    call_table = table.clone()
    for b, page, entry in bad_pages:
        call_table[b, page] = entry
        kval[b, page * ps:(page + 1) * ps], vval[b, page * ps:(page + 1) * ps] = 0.0, 0.0
        for pool in pools[4:]:
            pool[table[b, page]] = 0
    ro = torch.zeros((total_q, hq, 128), dtype=torch.float64)
    rl = torch.full((hq, total_q), -math.inf, dtype=torch.float64)
    owned = torch.zeros(total_q, dtype=torch.bool)
    for b, ((st, nq), nk) in enumerate(zip(qs, nks)):
        owned[st:st + nq] = True
        for h in range(hq if nq and nk else 0):
            hk = h // (hq // hkv)
            s = 128 ** -0.5 * qd[b, hk].double() * kd[b, hk].double() * (qkv8[st:st + nq, 0, h].double() @ kval[b, :nk, hk].T)
            if causal:
                s = s.masked_fill(torch.arange(nk)[None, :] > torch.arange(nq)[:, None] + nk - nq, -math.inf)
            rl[h, st:st + nq] = torch.logsumexp(s, -1)
            ro[st:st + nq, h] = torch.nan_to_num(torch.exp(s - rl[h, st:st + nq, None])) @ (vval[b, :nk, hk] * vd[b, hk].double())

    dev = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)              # noqa: E731
    buf_o = torch.full((total_q * hq * 128 + 2 * PAD,), -7.0, dtype=dtype, device=DEV)
    buf_l = torch.full((hq * total_q + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    o, lse = buf_o[PAD:-PAD].view(total_q, hq, 128), buf_l[PAD:-PAD].view(hq, total_q)
    kw = dict(q_descale=qd.to(DEV), k_descale=kd.to(DEV), causal=causal, out_dtype=dtype)
    ext.fp4_varlen_forward(qkv8.to(DEV)[:, 0], *pools[:4], dev(cu_q), dev(cu_k), max_q, CAP, call_table.to(DEV), v_descale=vd.to(DEV),
                           out=(o, lse), **kw)
    rows = torch.cat([torch.arange(st, st + nq) for st, nq in qs])               # the owned tokens in sequence order: the baseline's packing
    ob, lb = fp8_attn_varlen_func(qkv8[:, 0][rows].contiguous().to(DEV), pools[4].view(E4), pools[5].view(E4), dev(cu_of([n for _, n in qs])), dev(cu_of(nks)),
                                  max_q, CAP, block_table=table.to(DEV), v_descale=(vd * 2.0 ** -base_shift).to(DEV),
                                  return_softmax_lse=True, **kw)
    torch.cuda.synchronize()
    assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))   # nothing beside the outputs
    assert bool((o.cpu()[~owned] == -7.0).all()) and bool((lse.cpu()[:, ~owned] == -7.0).all())
    o, lse, ro, rl, ob, lb = o.cpu()[rows], lse.cpu()[:, rows], ro[rows], rl[:, rows], ob.cpu(), lb.cpu()
    dead = rl == -math.inf                                                       # (rl, ro: fp64 attention per sequence)
    assert torch.equal(lse == -math.inf, dead) and bool((o.transpose(0, 1)[dead] == 0).all()) and bool(torch.isfinite(o).all())
    pack = lambda o_, l_: Result(o_.reshape(-1, 128), l_, *[None] * 9)         # noqa: E731
    bad, ratio = sharp_bar(pack(o, lse), pack(ro, rl), pack(ob, lb), dtype)
    print(f"RATIO causal={causal} H={hq}/{hkv} ps={ps} {dtype} shift={base_shift} " + " ".join(f"{k}={v:.3f}" for k, v in ratio.items()))
    assert not bad, bad


CASES = [(False, 8, 2, 16, torch.bfloat16), (True, 8, 2, 16, torch.bfloat16), (True, 8, 2, 16, torch.float16), (True, 2, 2, 16, torch.bfloat16),
         (True, 8, 2, 64, torch.bfloat16)]


@pytest.mark.parametrize("causal,hq,hkv,ps,dtype", CASES, ids=[f"causal{int(c[0])}-H{c[1]}_{c[2]}-ps{c[3]}-{str(c[4])[6:]}" for c in CASES])
def test_prefill_against_fp64(causal, hq, hkv, ps, dtype):
    check(causal, hq, hkv, ps, dtype)


@pytest.mark.parametrize("which", ("all_minus_20", "alternating"))
def test_v_scale_range(which):
    """every ev = -20 (without the joint maximum all of P flushes to zero); ev alternating -6 / +5 with unit K scales"""
    if which == "all_minus_20":
        check(True, ev=torch.full((B, CAP, 2), -20), base_shift=20)
    else:
        ev = torch.where(torch.arange(CAP) % 2 == 0, -6, 5)[None, :, None].expand(B, CAP, 2)
        check(True, ek=torch.zeros((B, CAP, 2, 4), dtype=torch.int64), ev=ev)


def test_untrusted_offsets_table_and_scale_bytes():
    """rows 0 .. 2 of no sequence; sequence 4's offsets run past total_q (94 rows left), sequence 5's decrease (empty); cu_seqlens_k
    decreases (sequence 3: no key), runs past the capacity (sequence 4: CAP keys); table entries -1 and 10^6 are zero keys."""
    check(True, cu_q=[3, 4, 37, 166, 166, 999, 990], total_q=260, cu_k=[0, 1, 66, 266, 200, 10 ** 6, 10 ** 6 + 20],
          bad_pages=((2, 1, -1), (2, 5, 10 ** 6), (1, 0, 10 ** 6)))
    # 0xFF scale bytes: any numbers, no fault, nothing written beside o and lse
    import flashattention_lab_cuda as ext
    g = torch.Generator().manual_seed(4)
    q8 = torch.randn((253, 8, 128), generator=g).to(E4).to(DEV)
    kc, vc = (torch.randint(0, 256, (B * 16, 16, 2, 64), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    ks, vs = (torch.full(s, 0xFF, dtype=torch.uint8, device=DEV) for s in ((B * 16, 16, 2, 4), (B * 16, 16, 2)))
    cu = [torch.tensor(cu_of([s[i] for s in SEQS]), dtype=torch.int32, device=DEV) for i in (0, 1)]
    buf_o = torch.full((253 * 8 * 128 + 2 * PAD,), -7.0, dtype=torch.bfloat16, device=DEV)
    buf_l = torch.full((8 * 253 + 2 * PAD,), -7.0, dtype=torch.float32, device=DEV)
    ext.fp4_varlen_forward(q8, kc, ks, vc, vs, *cu, 129, CAP, torch.arange(B * 16, dtype=torch.int32, device=DEV).view(B, 16), causal=True,
                           out=(buf_o[PAD:-PAD].view(253, 8, 128), buf_l[PAD:-PAD].view(8, 253)))
    torch.cuda.synchronize()
    assert all(bool((buf[:PAD] == -7.0).all()) and bool((buf[-PAD:] == -7.0).all()) for buf in (buf_o, buf_l))
    assert bool((buf_l[PAD:-PAD].view(8, 253)[:, 163:203] == -math.inf).all())   # (sequence 4 has no key)


def test_graph_replay_after_the_state_changed():
    """append + prefill from one graph, replayed after the state changed in place: bit for bit the eager run"""
    from common.fp4_kvcache import fp8_attn_varlen_with_mxfp4_kvcache, mxfp4_kvcache_append

    g = torch.Generator().manual_seed(5)
    b, hq, hkv, ps, nb, nnew, total = 2, 8, 2, 16, 16, 40, 80
    pool = [torch.randint(0, 256, (b * nb, ps, hkv, 64), generator=g, dtype=torch.uint8), torch.randint(122, 133, (b * nb, ps, hkv, 4), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (b * nb, ps, hkv, 64), generator=g, dtype=torch.uint8), torch.randint(122, 133, (b * nb, ps, hkv), generator=g, dtype=torch.uint8)]

    def state(s):
        lens, nq = ((13, 60), (77, 190))[s], ((40, 40), (7, 33))[s]
        return (torch.tensor(lens, dtype=torch.int32), torch.tensor(cu_of(nq), dtype=torch.int32),
                torch.tensor(cu_of([n + nnew for n in lens]), dtype=torch.int32), (torch.randn((b, nnew, hkv, 128), generator=g) * (1 + s)).bfloat16(),
                (torch.randn((b, nnew, hkv, 128), generator=g) * (2 - s)).bfloat16(), torch.randperm(b * nb, generator=g).reshape(b, nb).to(torch.int32),
                0.5 + torch.rand((b, hkv), generator=g))
    first, second = state(0), state(1)
    lens, cu_q, cu_k, k, v, table, kd = (t.to(DEV) for t in first)
    q8 = torch.randn((total, hq, 128), generator=g).to(E4).to(DEV)
    dev_pool = [t.to(DEV) for t in pool]

    def step():
        mxfp4_kvcache_append(k, v, *dev_pool, cache_seqlens=lens, block_table=table)
        return fp8_attn_varlen_with_mxfp4_kvcache(q8, *dev_pool, cu_q, cu_k, 40, nb * ps, block_table=table, k_descale=kd, causal=True,
                                                  return_softmax_lse=True)

    step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g = step()
    for new in (second, first, second):
        for dst, src in zip((lens, cu_q, cu_k, k, v, table, kd, *dev_pool), (*new, *pool)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        n = int(new[1][-1])                                      # (rows past the last sequence are not written: uninitialised)
        replayed = [o_g[:n].clone(), lse_g[:, :n].clone(), *[t.clone() for t in dev_pool]]
        for dst, src in zip(dev_pool, pool):
            dst.copy_(src)
        o_e, lse_e = step()
        for a, b_ in zip(replayed, [o_e[:n], lse_e[:, :n], *dev_pool]):
            assert torch.equal(a, b_)
