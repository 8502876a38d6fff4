"""GPU: KV-cache decoding with split-KV (fa_ex_forward_kvcache; common/attention_ex.py: flash_attn_with_kvcache) against an fp64
reference computed per batch element on the [:len_k] slice with an explicit visibility mask; the in-place append, the splits,
the existing extended path, dead rows, strided and large caches, and graph capture."""
import itertools
import math

import pytest
import torch

from tests.helpers import dtype_tolerances

pytestmark = pytest.mark.gpu
DEV = "cuda"


def reference(q, kc, vc, lens_k, causal, window, scale, softcap=0.0, slopes=None):
    """o (B, Nq, H_q, d) fp64 and lse (B, H_q, Nq) of attention over keys [0, lens_k[b]) of the (already appended) caches"""
    b_, nq, hq, d = q.shape
    hkv = kc.shape[2]
    g = hq // hkv
    o = torch.zeros((b_, nq, hq, d), dtype=torch.float64)
    lse = torch.full((b_, hq, nq), -math.inf, dtype=torch.float64)
    wl, wr = window
    for b in range(b_):
        lk = int(lens_k[b])
        if lk == 0:
            continue
        qq = q[b].double().permute(1, 0, 2)                                   # (H_q, Nq, d)
        kk = kc[b, :lk].double().permute(1, 0, 2).repeat_interleave(g, 0)    # (H_q, lk, d)
        vv = vc[b, :lk].double().permute(1, 0, 2).repeat_interleave(g, 0)
        s = scale * qq @ kk.transpose(1, 2)
        if softcap > 0:
            s = softcap * torch.tanh(s / softcap)
        i = torch.arange(nq).view(-1, 1)
        j = torch.arange(lk).view(1, -1)
        diag = i + lk - nq
        if slopes is not None:
            sl = (slopes[b] if slopes.dim() == 2 else slopes).double().cpu().view(-1, 1, 1)
            s = s - sl * (diag - j).abs().double()
        vis = torch.ones((nq, lk), dtype=torch.bool)
        if causal:
            vis &= j <= diag
        if wl >= 0:
            vis &= j >= diag - wl
        if wr >= 0:
            vis &= j <= diag + wr
        s = s.masked_fill(~vis, -math.inf)
        l = torch.logsumexp(s, -1)
        p = torch.exp(s - l.unsqueeze(-1)).nan_to_num(0.0)
        o[b] = (p @ vv).permute(1, 0, 2)
        lse[b] = l
    return o, lse


def make(b, cap, hq, hkv, nq, d, dtype, seed, nnew=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((b, nq, hq, d), generator=g).to(dtype).to(DEV)
    kc = torch.randn((b, cap, hkv, d), generator=g).to(dtype).to(DEV)
    vc = torch.randn((b, cap, hkv, d), generator=g).to(dtype).to(DEV)
    kn = torch.randn((b, nnew, hkv, d), generator=g).to(dtype).to(DEV) if nnew else None
    vn = torch.randn((b, nnew, hkv, d), generator=g).to(dtype).to(DEV) if nnew else None
    return q, kc, vc, kn, vn


def check(o, lse, ro, rlse, dtype):
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    torch.testing.assert_close(o.double().cpu(), ro, **dtype_tolerances(dtype))
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse.cpu()), fin)
    torch.testing.assert_close(lse.double().cpu()[fin], rlse[fin], rtol=1e-3, atol=1e-3)
    assert (o.cpu().double().permute(0, 2, 1, 3)[~fin] == 0).all()


def alibi(hq):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / hq) for h in range(hq)], dtype=torch.float32, device=DEV)


CASES = []
for dtype, d in itertools.product((torch.bfloat16, torch.float16), (64, 96, 128, 256)):
    for (hq, hkv), nq in itertools.product(((8, 8), (8, 2), (8, 1)), (1, 2, 5, 16, 130)):
        CASES.append((dtype, d, hq, hkv, nq))


@pytest.mark.parametrize("dtype,d,hq,hkv,nq", CASES, ids=lambda x: str(x).replace("torch.", ""))
def test_parity(dtype, d, hq, hkv, nq):
    from common.attention_ex import flash_attn_with_kvcache

    cap = 300
    b = 4
    seed = hash((d, hq, hkv, nq)) & 0xffff
    q, kc, vc, kn, vn = make(b, cap, hq, hkv, nq, d, dtype, seed, nnew=1 if nq <= 2 else 0)
    nnew = 0 if kn is None else kn.shape[1]
    lens = torch.tensor([0, 1, cap - nnew, 137][:b], dtype=torch.int32)
    scale = d ** -0.5
    variants = [(False, (-1, -1), 0.0, None), (True, (-1, -1), 0.0, None), (False, (40, 3), 0.0, None), (True, (64, -1), 30.0, None),
                (False, (-1, -1), 0.0, alibi(hq)), (True, (-1, -1), 5.0, alibi(hq)),
                (True, (-1, -1), 0.0, alibi(hq).unsqueeze(0) * torch.arange(1, b + 1, device=DEV).view(-1, 1).float())]   # (B, H_q)
    k0, v0 = kc.clone(), vc.clone()
    for causal, window, softcap, slopes in variants:
        kc.copy_(k0)
        vc.copy_(v0)
        o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens.to(DEV), causal=causal, window_size=window,
                                         softcap=softcap, alibi_slopes=slopes, return_softmax_lse=True)
        kref, vref = k0.cpu().clone(), v0.cpu().clone()
        if nnew:
            for bb in range(b):
                kref[bb, lens[bb]:lens[bb] + nnew] = kn[bb].cpu()
                vref[bb, lens[bb]:lens[bb] + nnew] = vn[bb].cpu()
        assert torch.equal(kc.cpu(), kref) and torch.equal(vc.cpu(), vref)
        ro, rlse = reference(q.cpu(), kref, vref, lens + nnew, causal, window, scale, softcap, slopes)
        check(o, lse, ro, rlse, dtype)


@pytest.mark.parametrize("causal", [False, True])
def test_huge_window_bounds_mean_unbounded(causal):
    import flashattention_lab_cuda as ext

    q, kc, vc, _, _ = make(3, 500, 8, 2, 3, 128, torch.bfloat16, 13)
    lens = torch.tensor([500, 37, 260], dtype=torch.int32, device=DEV)
    for s in (1, 4):
        o0, l0 = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, causal, None, num_splits=s)
        for window in ((2 ** 32, -1), (-1, 2 ** 31 - 1), (2 ** 63 - 1, 2 ** 63 - 1), (499, 2)):
            o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, causal, None, window=window, num_splits=s)
            assert torch.equal(o, o0) and torch.equal(lse, l0), window
    ro, rlse = reference(q.cpu(), kc.cpu(), vc.cpu(), lens.cpu(), causal, (-1, -1), 128 ** -0.5)
    check(o0, l0, ro, rlse, torch.bfloat16)


def test_append_exact_and_clamped():
    import flashattention_lab_cuda as ext

    b, cap, hq, hkv, nq, d, nnew = 5, 64, 4, 2, 2, 128, 3
    q, kc, vc, kn, vn = make(b, cap, hq, hkv, nq, d, torch.bfloat16, 7, nnew=nnew)
    # guard values around each cache: a bigger buffer whose middle is the cache
    big_k = torch.randn((b + 2, cap, hkv, d), dtype=torch.float32).to(torch.bfloat16).to(DEV)
    big_v = torch.randn((b + 2, cap, hkv, d), dtype=torch.float32).to(torch.bfloat16).to(DEV)
    kcache, vcache = big_k[1:b + 1], big_v[1:b + 1]
    before_k, before_v = big_k.clone(), big_v.clone()
    seqlens = torch.tensor([-5, 0, 10, cap - nnew, cap + 100], dtype=torch.int32)
    o, lse = ext.ex_kvcache_forward(q, kcache, vcache, kn, vn, seqlens.to(DEV), False, None)
    L = seqlens.clamp(0, cap - nnew)
    ek, ev = before_k.clone(), before_v.clone()
    for bb in range(b):
        ek[bb + 1, L[bb]:L[bb] + nnew] = kn[bb]
        ev[bb + 1, L[bb]:L[bb] + nnew] = vn[bb]
    assert torch.equal(big_k, ek) and torch.equal(big_v, ev)
    ro, rlse = reference(q.cpu(), kcache.cpu(), vcache.cpu(), L + nnew, False, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, torch.bfloat16)


def test_splits_agree_and_repeat_bitwise():
    import flashattention_lab_cuda as ext

    b, cap, hq, hkv, nq, d = 3, 2000, 8, 2, 1, 128
    q, kc, vc, _, _ = make(b, cap, hq, hkv, nq, d, torch.bfloat16, 11)
    lens = torch.tensor([2000, 1, 777], dtype=torch.int32, device=DEV)
    outs = {}
    for s in (1, 2, 7, 0):
        outs[s] = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=s)
        again = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=s)
        assert torch.equal(outs[s][0], again[0]) and torch.equal(outs[s][1], again[1])
    ro, rlse = reference(q.cpu(), kc.cpu(), vc.cpu(), lens.cpu(), True, (-1, -1), d ** -0.5)
    for s, (o, lse) in outs.items():
        check(o, lse, ro, rlse, torch.bfloat16)
        torch.testing.assert_close(o.float(), outs[1][0].float(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("causal", [False, True])
def test_matches_ex_forward_gqa(causal):
    import flashattention_lab_cuda as ext

    b, L, hq, hkv, nq, d = 2, 1024, 8, 2, 4, 128
    q, kc, vc, _, _ = make(b, L, hq, hkv, nq, d, torch.bfloat16, 3)
    o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, None, causal, None)
    q3 = q.permute(0, 2, 1, 3).reshape(b * hq, nq, d)
    k3 = kc.permute(0, 2, 1, 3).reshape(b * hkv, L, d)
    v3 = vc.permute(0, 2, 1, 3).reshape(b * hkv, L, d)
    oe, lsee = ext.ex_forward(q3, k3, v3, causal, d ** -0.5)
    torch.testing.assert_close(o.permute(0, 2, 1, 3).reshape(b * hq, nq, d).float(), oe.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.reshape(b * hq, nq), lsee, rtol=1e-3, atol=1e-3)


def test_dead_rows():
    import flashattention_lab_cuda as ext

    b, cap, hq, hkv, nq, d = 2, 100, 4, 4, 3, 64
    q, kc, vc, _, _ = make(b, cap, hq, hkv, nq, d, torch.float16, 5)
    for s in (1, 3):
        # len_k = 0: every row dead
        o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, torch.zeros(b, dtype=torch.int32, device=DEV), False, None, num_splits=s)
        assert (o == 0).all() and torch.isneginf(lse).all()
        # causal with len_k = 1 < Nq = 3: coff = -2, rows 0 and 1 see no key
        lens = torch.full((b,), 1, dtype=torch.int32, device=DEV)
        o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=s)
        ro, rlse = reference(q.cpu(), kc.cpu(), vc.cpu(), lens.cpu(), True, (-1, -1), d ** -0.5)
        check(o, lse, ro, rlse, torch.float16)
        assert torch.isneginf(lse[:, :, :2]).all() and (o[:, :2] == 0).all()


def test_window_hides_every_key():
    import flashattention_lab_cuda as ext

    # Nq = 4 over len_k = 2: coff = -2; window (0, 0) puts row i's band at key i - 2: rows 0, 1 see nothing, rows 2, 3 one key each
    q, kc, vc, _, _ = make(1, 50, 2, 1, 4, 64, torch.bfloat16, 9)
    lens = torch.tensor([2], dtype=torch.int32, device=DEV)
    for s in (1, 2):
        o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, False, None, window=(0, 0), num_splits=s)
        ro, rlse = reference(q.cpu(), kc.cpu(), vc.cpu(), lens.cpu(), False, (0, 0), 64 ** -0.5)
        check(o, lse, ro, rlse, torch.bfloat16)
        assert torch.isneginf(lse[0, :, :2]).all() and (o[0, :2] == 0).all() and not torch.isnan(o).any()


def test_unbound_kv_views():
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hkv, hq, d, nq = 3, 200, 2, 8, 128, 1
    kv = torch.randn((b, cap, 2, hkv, d), dtype=torch.float32).to(torch.bfloat16).to(DEV)
    kc, vc = kv.unbind(2)
    q = torch.randn((b, nq, hq, d)).to(torch.bfloat16).to(DEV)
    kn = torch.randn((b, 1, hkv, d)).to(torch.bfloat16).to(DEV)
    vn = torch.randn((b, 1, hkv, d)).to(torch.bfloat16).to(DEV)
    lens = torch.tensor([5, 100, 199], dtype=torch.int32, device=DEV)
    before = kv.clone()
    o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, causal=True, return_softmax_lse=True)
    for bb in range(b):
        before[bb, lens[bb], 0] = kn[bb, 0]
        before[bb, lens[bb], 1] = vn[bb, 0]
    assert torch.equal(kv, before)
    ro, rlse = reference(q.cpu(), kc.cpu(), vc.cpu(), (lens + 1).cpu(), True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, torch.bfloat16)


def test_cache_larger_than_2gib():
    import flashattention_lab_cuda as ext

    b, cap, hkv, hq, d = 17, 65536, 8, 8, 128   # 128 MiB per batch element: each cache 2.125 GiB, the last element past 2^31 B
    kc = torch.empty((b, cap, hkv, d), dtype=torch.bfloat16, device=DEV)
    vc = torch.empty((b, cap, hkv, d), dtype=torch.bfloat16, device=DEV)
    kc.normal_()
    vc.normal_()
    assert kc.numel() * 2 + vc.numel() * 2 > 2 ** 31
    q = torch.randn((b, 1, hq, d)).to(torch.bfloat16).to(DEV)
    lens = torch.full((b,), 3000, dtype=torch.int32, device=DEV)
    o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, False, None)
    last = slice(b - 1, b)
    ro, rlse = reference(q[last].cpu(), kc[last, :3000].cpu(), vc[last, :3000].cpu(), [3000], False, (-1, -1), d ** -0.5)
    check(o[last], lse[last], ro, rlse, torch.bfloat16)
    del kc, vc
    torch.cuda.empty_cache()


def test_graph_capture_decode_step():
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, d, nq = 2, 512, 8, 2, 128, 1
    q, kc, vc, kn, vn = make(b, cap, hq, hkv, nq, d, torch.bfloat16, 21, nnew=1)
    lens = torch.tensor([10, 300], dtype=torch.int32, device=DEV)
    flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, causal=True)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, causal=True, return_softmax_lse=True)
    torch.cuda.current_stream().wait_stream(s)
    for step, new_lens in enumerate(([11, 301], [0, 511], [200, 5])):
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32))
        q.copy_(torch.randn(q.shape).to(q.dtype))
        kn.copy_(torch.randn(kn.shape).to(kn.dtype))
        k_before, v_before = kc.clone(), vc.clone()
        graph.replay()
        torch.cuda.synchronize()
        kref, vref = k_before.cpu(), v_before.cpu()
        for bb in range(b):
            kref[bb, new_lens[bb]] = kn[bb, 0].cpu()
            vref[bb, new_lens[bb]] = vn[bb, 0].cpu()
        assert torch.equal(kc.cpu(), kref) and torch.equal(vc.cpu(), vref)
        ro, rlse = reference(q.cpu(), kref, vref, [x + 1 for x in new_lens], True, (-1, -1), d ** -0.5)
        check(out[0], out[1], ro, rlse, torch.bfloat16)
