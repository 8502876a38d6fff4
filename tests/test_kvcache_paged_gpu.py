"""GPU: the paged KV cache (block_table), cache_batch_idx and cache_leftpad of flash_attn_with_kvcache /
fa_ex_forward_kvcache_paged against the fp64 reference of tests/kvcache_paged_ref.py (per batch element: gather the sequence's
tokens, explicit visibility mask), bitwise against the contiguous call, the append through the table, untrusted table entries
and cache indices, prefix sharing, strided and > 4 GiB pools, and graph capture.  Tolerances: tests.helpers.dtype_tolerances for
o, rtol = atol = 1e-3 for lse, as in tests/test_kvcache_gpu.py; bitwise checks use torch.equal."""
import itertools

import pytest
import torch

from tests.helpers import dtype_tolerances
from tests.kvcache_paged_ref import paged_append, paged_tokens, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def check(o, lse, ro, rlse, dtype):
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    torch.testing.assert_close(o.double().cpu(), ro, **dtype_tolerances(dtype))
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse.cpu()), fin)
    torch.testing.assert_close(lse.double().cpu()[fin], rlse[fin], rtol=1e-3, atol=1e-3)
    assert (o.cpu().double().permute(0, 2, 1, 3)[~fin] == 0).all()


def alibi(hq):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / hq) for h in range(hq)], dtype=torch.float32, device=DEV)


def randn(shape, g, dtype):
    return torch.randn(shape, generator=g).to(dtype).to(DEV)


def make_paged(b, mb, ps, hq, hkv, nq, d, dtype, seed, nnew=0, spare=3):
    """q, K pool, V pool (b * mb + spare pages), k_new, v_new and a (b, mb) table of distinct pages in shuffled order"""
    g = torch.Generator().manual_seed(seed)
    nblk = b * mb + spare
    q = randn((b, nq, hq, d), g, dtype)
    kp, vp = randn((nblk, ps, hkv, d), g, dtype), randn((nblk, ps, hkv, d), g, dtype)
    kn = randn((b, nnew, hkv, d), g, dtype) if nnew else None
    vn = randn((b, nnew, hkv, d), g, dtype) if nnew else None
    table = torch.randperm(nblk, generator=g)[:b * mb].view(b, mb).to(torch.int32)
    return q, kp, vp, kn, vn, table


def to_contiguous(kp, vp, table, ps):
    """the same tokens as a (B, mb * ps, H_kv, d) cache"""
    idx = table.long().to(kp.device)
    b, mb = table.shape
    return (kp[idx].reshape(b, mb * ps, *kp.shape[2:]).contiguous(), vp[idx].reshape(b, mb * ps, *vp.shape[2:]).contiguous())


MB = {16: 13, 48: 5, 256: 3}   # pages a sequence: capacities 208, 240 and 768 tokens (at least three pages)
NQ_D = tuple(itertools.product((1, 2, 5, 16, 130), (64, 96, 128, 256)))
CASES = [(dtype, d, hq, hkv, nq, ps)
         for dtype, (nq, d), (hq, hkv), ps in itertools.product((BF16, torch.float16), NQ_D, ((8, 8), (8, 2), (8, 1)), (16, 48, 256))]


@pytest.mark.parametrize("dtype,d,hq,hkv,nq,ps", CASES, ids=lambda x: str(x).replace("torch.", ""))
def test_parity(dtype, d, hq, hkv, nq, ps):
    from common.attention_ex import flash_attn_with_kvcache

    mb = MB[ps]
    cap = mb * ps
    NNEW = 2
    # lengths before the append: 0, 1, a page boundary and its neighbours, two pages and a bit, the capacity
    base = [0, 1, ps, ps - 1, ps + 1, 2 * ps + 5, cap]
    b = len(base)
    seed = hash((d, hq, hkv, nq, ps)) & 0xffff
    q, kp, vp, kn, vn, table = make_paged(b, mb, ps, hq, hkv, nq, d, dtype, seed, nnew=NNEW)
    scale = d ** -0.5
    variants = [(False, (-1, -1), 0.0, None), (True, (-1, -1), 0.0, None), (False, (40, 3), 0.0, None), (True, (64, -1), 30.0, None),
                (False, (-1, -1), 0.0, alibi(hq)), (True, (-1, -1), 5.0, alibi(hq)),
                (True, (-1, -1), 0.0, alibi(hq).unsqueeze(0) * torch.arange(1, b + 1, device=DEV).view(-1, 1).float())]   # (B, H_q)
    k0, v0 = kp.clone(), vp.clone()
    tdev = table.to(DEV)
    for vi, (causal, window, softcap, slopes) in enumerate(variants):
        nnew = NNEW if vi % 2 else 0            # with and without an append, in every case
        lens = torch.tensor([min(x, cap - nnew) for x in base], dtype=torch.int32)
        assert max(int(x) + nnew for x in lens) >= 2 * ps   # translation really crosses pages
        kp.copy_(k0)
        vp.copy_(v0)
        o, lse = flash_attn_with_kvcache(q, kp, vp, kn if nnew else None, vn if nnew else None, cache_seqlens=lens.to(DEV),
                                         block_table=tdev, causal=causal, window_size=window, softcap=softcap, alibi_slopes=slopes,
                                         return_softmax_lse=True)
        kref, vref = k0.cpu().clone(), v0.cpu().clone()
        if nnew:
            paged_append(kref, table, lens, kn.cpu(), ps)
            paged_append(vref, table, lens, vn.cpu(), ps)
        assert torch.equal(kp.cpu(), kref) and torch.equal(vp.cpu(), vref)
        ks = [paged_tokens(kref, table[bb], int(lens[bb]) + nnew, ps) for bb in range(b)]
        vs = [paged_tokens(vref, table[bb], int(lens[bb]) + nnew, ps) for bb in range(b)]
        ro, rlse = reference(q.cpu(), ks, vs, causal, window, scale, softcap, slopes)
        check(o, lse, ro, rlse, dtype)


@pytest.mark.parametrize("ps", [16, 48, 256])
@pytest.mark.parametrize("d,hq,hkv,nq", [(128, 8, 2, 1), (64, 8, 1, 5), (256, 8, 8, 3), (96, 4, 2, 20)])
def test_paged_equals_contiguous_bitwise(ps, d, hq, hkv, nq):
    import flashattention_lab_cuda as ext

    mb = {16: 40, 48: 14, 256: 3}[ps]
    b, cap = 4, mb * ps
    q, kp, vp, _, _, table = make_paged(b, mb, ps, hq, hkv, nq, d, BF16, 100 + ps + d)
    kc, vc = to_contiguous(kp, vp, table, ps)
    lens = torch.tensor([cap, 2 * ps + 7, 1, cap - 33], dtype=torch.int32, device=DEV)
    tdev = table.to(DEV)
    # (ps + 9, 0): with Nq = 1 the band of the full sequence starts at key cap - 1 - (ps + 9), nine keys before a page boundary
    for (causal, window), s in itertools.product(((False, (-1, -1)), (True, (-1, -1)), (True, (ps + 9, 0)), (False, (37, 2))), (1, 4, 0)):
        oc, lc = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, causal, None, window=window, num_splits=s)
        op, lp = ext.ex_kvcache_forward(q, kp, vp, None, None, lens, causal, None, window=window, num_splits=s, block_table=tdev)
        assert torch.equal(oc, op) and torch.equal(lc, lp), (causal, window, s)
    assert not torch.isnan(op).any()


def test_append_through_the_table_changes_only_its_slots():
    import flashattention_lab_cuda as ext

    ps, mb, b, hq, hkv, nq, d, nnew = 16, 4, 4, 4, 2, 3, 128, 3
    q, _, _, kn, vn, _ = make_paged(b, mb, ps, hq, hkv, nq, d, BF16, 41, nnew=nnew)
    nblk, guard = b * mb + 5, 2
    g = torch.Generator().manual_seed(42)
    big_k, big_v = randn((nblk + 2 * guard, ps, hkv, d), g, BF16), randn((nblk + 2 * guard, ps, hkv, d), g, BF16)
    kp, vp = big_k[guard:guard + nblk], big_v[guard:guard + nblk]     # the pools: the middle slices
    table = torch.randperm(nblk, generator=g)[:b * mb].view(b, mb).to(torch.int32)   # five pages that no table names
    # L = ps - 1: the three new tokens cross a page boundary; clamped lengths; an append into the last page
    seqlens = torch.tensor([ps - 1, -4, 10 ** 6, 2 * ps], dtype=torch.int32)
    L = seqlens.clamp(0, mb * ps - nnew)
    before_k, before_v = big_k.clone(), big_v.clone()
    o, lse = ext.ex_kvcache_forward(q, kp, vp, kn, vn, seqlens.to(DEV), True, None, block_table=table.to(DEV))
    ek, ev = before_k.cpu(), before_v.cpu()
    paged_append(ek[guard:guard + nblk], table, L, kn.cpu(), ps)
    paged_append(ev[guard:guard + nblk], table, L, vn.cpu(), ps)
    assert torch.equal(big_k.cpu(), ek) and torch.equal(big_v.cpu(), ev)
    assert not torch.equal(ek, before_k.cpu())
    ks = [paged_tokens(ek[guard:guard + nblk], table[bb], int(L[bb]) + nnew, ps) for bb in range(b)]
    vs = [paged_tokens(ev[guard:guard + nblk], table[bb], int(L[bb]) + nnew, ps) for bb in range(b)]
    ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)


def test_table_entries_past_the_used_range_are_not_read():
    import flashattention_lab_cuda as ext

    ps, mb, b, hq, hkv, nq, d = 48, 6, 3, 8, 2, 2, 128
    q, kp, vp, kn, vn, table = make_paged(b, mb, ps, hq, hkv, nq, d, BF16, 51, nnew=1)
    lens = torch.tensor([0, ps - 1, 3 * ps + 1], dtype=torch.int32)   # len_k = 1, ps, 3 ps + 2: 1, 1 and 4 pages used
    dirty = table.clone()
    for bb, used in enumerate((1, 1, 4)):
        dirty[bb, used:] = torch.tensor([2 ** 31 - 1, -7] * mb, dtype=torch.int32)[:mb - used]
    k0, v0 = kp.clone(), vp.clone()
    outs = []
    for t in (table, dirty):
        kp.copy_(k0)
        vp.copy_(v0)
        for s in (1, 3, 0):
            outs.append(ext.ex_kvcache_forward(q, kp, vp, kn, vn, lens.to(DEV), True, None, num_splits=s, block_table=t.to(DEV)))
        outs.append((kp.clone(), vp.clone()))
    half = len(outs) // 2
    for (a0, a1), (b0, b1) in zip(outs[:half], outs[half:]):
        assert torch.equal(a0, b0) and torch.equal(a1, b1)


def test_pages_outside_the_pool_read_as_zeros_and_drop_the_append():
    """Entries -1 and num_blocks inside the used range.  The pools are the middle of larger buffers, so the pages a wrong
    implementation would reach (one before, one after the pool) are allocated guard pages.  Run once."""
    import flashattention_lab_cuda as ext

    ps, mb, b, hq, hkv, nq, d, nnew = 16, 5, 2, 4, 2, 2, 64, 2
    q, _, _, kn, vn, _ = make_paged(b, mb, ps, hq, hkv, nq, d, BF16, 61, nnew=nnew)
    nblk, guard = 12, 2
    g = torch.Generator().manual_seed(62)
    big_k, big_v = randn((nblk + 2 * guard, ps, hkv, d), g, BF16), randn((nblk + 2 * guard, ps, hkv, d), g, BF16)
    kp, vp = big_k[guard:guard + nblk], big_v[guard:guard + nblk]
    table = torch.tensor([[3, -1, 7, 0, 5], [9, 2, nblk, 11, 4]], dtype=torch.int32)
    # sequence 0 appends at tokens 31, 32: the first into the dropped page 1; sequence 1 at 46, 47: both into its dropped page 2
    lens = torch.tensor([2 * ps - 1, 3 * ps - 2], dtype=torch.int32)
    before_k, before_v = big_k.clone(), big_v.clone()
    o, lse = ext.ex_kvcache_forward(q, kp, vp, kn, vn, lens.to(DEV), True, None, block_table=table.to(DEV))
    ek, ev = before_k.cpu(), before_v.cpu()
    paged_append(ek[guard:guard + nblk], table, lens, kn.cpu(), ps)
    paged_append(ev[guard:guard + nblk], table, lens, vn.cpu(), ps)
    assert torch.equal(big_k.cpu(), ek) and torch.equal(big_v.cpu(), ev)          # guards included
    assert torch.equal(big_k[:guard], before_k[:guard]) and torch.equal(big_k[guard + nblk:], before_k[guard + nblk:])
    ks = [paged_tokens(ek[guard:guard + nblk], table[bb], int(lens[bb]) + nnew, ps) for bb in range(b)]
    vs = [paged_tokens(ev[guard:guard + nblk], table[bb], int(lens[bb]) + nnew, ps) for bb in range(b)]
    assert (ks[0][ps:2 * ps] == 0).all() and (ks[1][2 * ps:3 * ps] == 0).all()
    ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)


def test_prefix_sharing():
    import flashattention_lab_cuda as ext

    ps, mb, hq, hkv, nq, d = 16, 8, 8, 2, 1, 128
    q, kp, vp, _, _, table = make_paged(2, mb, ps, hq, hkv, nq, d, BF16, 71)
    table[1, :3] = table[0, :3]            # the first three pages are shared
    lens = torch.tensor([5 * ps + 3, 7 * ps], dtype=torch.int32, device=DEV)
    tdev = table.to(DEV)
    o, lse = ext.ex_kvcache_forward(q, kp, vp, None, None, lens, True, None, block_table=tdev)
    for bb in range(2):
        o1, l1 = ext.ex_kvcache_forward(q[bb:bb + 1], kp, vp, None, None, lens[bb:bb + 1], True, None, block_table=tdev[bb:bb + 1])
        # (num_splits = 0 reads the batch size: pin the split count to compare bits)
        ob, lb = ext.ex_kvcache_forward(q, kp, vp, None, None, lens, True, None, num_splits=2, block_table=tdev)
        o2, l2 = ext.ex_kvcache_forward(q[bb:bb + 1], kp, vp, None, None, lens[bb:bb + 1], True, None, num_splits=2,
                                        block_table=tdev[bb:bb + 1])
        assert torch.equal(ob[bb:bb + 1], o2) and torch.equal(lb[bb:bb + 1], l2)
        torch.testing.assert_close(o[bb:bb + 1].float(), o1.float(), **dtype_tolerances(BF16))
    ks = [paged_tokens(kp.cpu(), table[bb], int(lens[bb]), ps) for bb in range(2)]
    vs = [paged_tokens(vp.cpu(), table[bb], int(lens[bb]), ps) for bb in range(2)]
    assert torch.equal(ks[0][:3 * ps], ks[1][:3 * ps])
    ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)


def test_unbound_pool_views():
    from common.attention_ex import flash_attn_with_kvcache

    ps, mb, b, hq, hkv, nq, d = 48, 4, 3, 8, 2, 1, 128
    nblk = b * mb + 2
    g = torch.Generator().manual_seed(81)
    kv = randn((nblk, 2, ps, hkv, d), g, BF16)
    kp, vp = kv.unbind(1)
    q, kn, vn = randn((b, nq, hq, d), g, BF16), randn((b, 1, hkv, d), g, BF16), randn((b, 1, hkv, d), g, BF16)
    table = torch.randperm(nblk, generator=g)[:b * mb].view(b, mb).to(torch.int32)
    lens = torch.tensor([5, ps - 1, 4 * ps - 1], dtype=torch.int32)
    expect = kv.cpu().clone()
    o, lse = flash_attn_with_kvcache(q, kp, vp, kn, vn, cache_seqlens=lens.to(DEV), block_table=table.to(DEV), causal=True,
                                     return_softmax_lse=True)
    paged_append(expect[:, 0], table, lens, kn.cpu(), ps)
    paged_append(expect[:, 1], table, lens, vn.cpu(), ps)
    assert torch.equal(kv.cpu(), expect)
    ks = [paged_tokens(expect[:, 0], table[bb], int(lens[bb]) + 1, ps) for bb in range(b)]
    vs = [paged_tokens(expect[:, 1], table[bb], int(lens[bb]) + 1, ps) for bb in range(b)]
    ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)


def test_pools_larger_than_4gib():
    import flashattention_lab_cuda as ext

    ps, hkv, hq, d, nblk = 256, 8, 8, 128, 8704      # 512 KiB a page: each pool 4.25 GiB
    kp = torch.empty((nblk, ps, hkv, d), dtype=BF16, device=DEV)
    vp = torch.empty((nblk, ps, hkv, d), dtype=BF16, device=DEV)
    assert kp.numel() * 2 > 2 ** 32 and vp.numel() * 2 > 2 ** 32
    kp[:16].normal_()
    vp[:16].normal_()
    kp[-16:].normal_()
    vp[-16:].normal_()
    b, mb, n = 2, 12, 2900
    table = torch.stack([torch.arange(mb), torch.arange(nblk - 1, nblk - 1 - mb, -1)]).to(torch.int32)   # the last pages, backwards
    q = torch.randn((b, 1, hq, d)).to(BF16).to(DEV)
    kn, vn = torch.randn((b, 1, hkv, d)).to(BF16).to(DEV), torch.randn((b, 1, hkv, d)).to(BF16).to(DEV)
    lens = torch.full((b,), n, dtype=torch.int32)
    o, lse = ext.ex_kvcache_forward(q, kp, vp, kn, vn, lens.to(DEV), False, None, block_table=table.to(DEV))
    pg, slot = int(table[1, n // ps]), n % ps
    assert pg * ps * hkv * d * 2 > 2 ** 32          # the appended token lies beyond 4 GiB
    assert torch.equal(kp[pg, slot], kn[1, 0]) and torch.equal(vp[pg, slot], vn[1, 0])
    # the checked sequence: only its pages go to the host
    sub_k, sub_v = kp[table[1].long().to(DEV)].cpu(), vp[table[1].long().to(DEV)].cpu()
    ident = torch.arange(mb)
    ks, vs = [paged_tokens(sub_k, ident, n + 1, ps)], [paged_tokens(sub_v, ident, n + 1, ps)]
    ro, rlse = reference(q[1:].cpu(), ks, vs, False, (-1, -1), d ** -0.5)
    check(o[1:], lse[1:], ro, rlse, BF16)
    del kp, vp, sub_k, sub_v
    torch.cuda.empty_cache()


def test_graph_capture_decode_step_with_a_growing_table():
    from common.attention_ex import flash_attn_with_kvcache

    ps, mb, b, hq, hkv, d, nq = 16, 6, 2, 8, 2, 128, 1
    q, kp, vp, kn, vn, full = make_paged(b, mb, ps, hq, hkv, nq, d, BF16, 91, nnew=1)
    cur = [ps - 2, 3 * ps - 1]                      # sequence 1 crosses into a new page at once, sequence 0 two steps later
    table = torch.full((b, mb), -1, dtype=torch.int32)
    for bb in range(b):
        used = cur[bb] // ps + 1
        table[bb, :used] = full[bb, :used]
    tdev, lens = table.to(DEV), torch.tensor(cur, dtype=torch.int32, device=DEV)
    flash_attn_with_kvcache(q, kp, vp, kn, vn, cache_seqlens=lens, block_table=tdev, causal=True)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = flash_attn_with_kvcache(q, kp, vp, kn, vn, cache_seqlens=lens, block_table=tdev, causal=True, return_softmax_lse=True)
    torch.cuda.current_stream().wait_stream(s)
    grew = 0
    for step in range(4):
        cur = [x + 1 for x in cur]
        for bb in range(b):
            if cur[bb] % ps == 0:                   # the token to append opens a page: the allocator names it in the table
                table[bb, cur[bb] // ps] = full[bb, cur[bb] // ps]
                grew += 1
        tdev.copy_(table)
        lens.copy_(torch.tensor(cur, dtype=torch.int32))
        q.copy_(torch.randn(q.shape).to(q.dtype))
        kn.copy_(torch.randn(kn.shape).to(kn.dtype))
        vn.copy_(torch.randn(vn.shape).to(vn.dtype))
        kref, vref = kp.cpu().clone(), vp.cpu().clone()
        graph.replay()
        torch.cuda.synchronize()
        paged_append(kref, table, cur, kn.cpu(), ps)
        paged_append(vref, table, cur, vn.cpu(), ps)
        assert torch.equal(kp.cpu(), kref) and torch.equal(vp.cpu(), vref)
        ks = [paged_tokens(kref, table[bb], cur[bb] + 1, ps) for bb in range(b)]
        vs = [paged_tokens(vref, table[bb], cur[bb] + 1, ps) for bb in range(b)]
        ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
        check(out[0], out[1], ro, rlse, BF16)
    assert grew == 2


# ---- cache_batch_idx, cache_leftpad (contiguous caches)

def make_cache(bc, cap, hkv, d, dtype, g):
    return randn((bc, cap, hkv, d), g, dtype), randn((bc, cap, hkv, d), g, dtype)


@pytest.mark.parametrize("bc,idx", [(4, [2, 0, 3, 1]), (7, [5, 0, 6])], ids=["permutation", "subset"])
def test_cache_batch_idx(bc, idx):
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, nq, d, nnew = len(idx), 200, 8, 2, 2, 128, 2
    g = torch.Generator().manual_seed(101 + bc)
    kc, vc = make_cache(bc, cap, hkv, d, BF16, g)
    q, kn, vn = randn((b, nq, hq, d), g, BF16), randn((b, nnew, hkv, d), g, BF16), randn((b, nnew, hkv, d), g, BF16)
    lens = torch.tensor([0, 77, cap - nnew, 130][:b], dtype=torch.int32)
    ek, ev = kc.cpu().clone(), vc.cpu().clone()
    for s in (1, 0):
        kc.copy_(ek)
        vc.copy_(ev)
        o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens.to(DEV), causal=True, num_splits=s,
                                         cache_batch_idx=torch.tensor(idx, dtype=torch.int32, device=DEV), return_softmax_lse=True)
        rk, rv = ek.clone(), ev.clone()
        for bb, row in enumerate(idx):
            rk[row, lens[bb]:lens[bb] + nnew] = kn[bb].cpu()
            rv[row, lens[bb]:lens[bb] + nnew] = vn[bb].cpu()
        assert torch.equal(kc.cpu(), rk) and torch.equal(vc.cpu(), rv)          # the rows no index names are untouched
        ks = [rk[row, :int(lens[bb]) + nnew] for bb, row in enumerate(idx)]
        vs = [rv[row, :int(lens[bb]) + nnew] for bb, row in enumerate(idx)]
        ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
        check(o, lse, ro, rlse, BF16)


def test_cache_batch_idx_outside_the_cache_reads_zeros_and_drops_the_append():
    """Indices -1 and B_cache; the cache is the middle of a larger buffer, so the rows a wrong implementation would reach are
    allocated guard rows.  Run once."""
    import flashattention_lab_cuda as ext

    bc, cap, hq, hkv, nq, d, nnew = 3, 96, 4, 2, 1, 64, 1
    g = torch.Generator().manual_seed(111)
    big_k, big_v = make_cache(bc + 2, cap, hkv, d, BF16, g)
    kc, vc = big_k[1:1 + bc], big_v[1:1 + bc]
    idx = [-1, 1, bc]
    b = len(idx)
    q, kn, vn = randn((b, nq, hq, d), g, BF16), randn((b, nnew, hkv, d), g, BF16), randn((b, nnew, hkv, d), g, BF16)
    lens = torch.tensor([40, 50, 60], dtype=torch.int32)
    before_k, before_v = big_k.cpu().clone(), big_v.cpu().clone()
    o, lse = ext.ex_kvcache_forward(q, kc, vc, kn, vn, lens.to(DEV), False, None,
                                    cache_batch_idx=torch.tensor(idx, dtype=torch.int32, device=DEV))
    before_k[2, 50], before_v[2, 50] = kn[1, 0].cpu(), vn[1, 0].cpu()             # cache row 1 of the middle slice
    assert torch.equal(big_k.cpu(), before_k) and torch.equal(big_v.cpu(), before_v)
    zk = torch.zeros((int(lens[0]) + nnew, hkv, d), dtype=BF16)
    ks = [zk, before_k[2, :51], torch.zeros((61, hkv, d), dtype=BF16)]
    vs = [zk, before_v[2, :51], torch.zeros((61, hkv, d), dtype=BF16)]
    ro, rlse = reference(q.cpu(), ks, vs, False, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)
    assert (o[0] == 0).all() and (o[2] == 0).all()


@pytest.mark.parametrize("variant", ["causal", "window", "alibi"])
@pytest.mark.parametrize("nq,nnew", [(1, 1), (3, 0), (20, 2)])
def test_cache_leftpad(variant, nq, nnew):
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, d = 5, 260, 8, 2, 128
    g = torch.Generator().manual_seed(121 + nq)
    kc, vc = make_cache(b, cap, hkv, d, BF16, g)
    q = randn((b, nq, hq, d), g, BF16)
    kn = randn((b, nnew, hkv, d), g, BF16) if nnew else None
    vn = randn((b, nnew, hkv, d), g, BF16) if nnew else None
    lens = torch.tensor([cap - nnew, 100, 33, 200, 64], dtype=torch.int32)
    pad = torch.tensor([0, 37, 32, -3, 1], dtype=torch.int32)          # (-3 clamps to 0)
    causal, window, slopes = {"causal": (True, (-1, -1), None), "window": (False, (45, 2), None),
                              "alibi": (True, (-1, -1), alibi(hq))}[variant]
    rk, rv = kc.cpu().clone(), vc.cpu().clone()
    for s in (1, 3, 0):
        kc.copy_(rk)
        vc.copy_(rv)
        o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens.to(DEV), cache_leftpad=pad.to(DEV), causal=causal,
                                         window_size=window, alibi_slopes=slopes, num_splits=s, return_softmax_lse=True)
        ek, ev = rk.clone(), rv.clone()
        for bb in range(b):
            if nnew:
                ek[bb, lens[bb]:lens[bb] + nnew] = kn[bb].cpu()         # still written at L_b
                ev[bb, lens[bb]:lens[bb] + nnew] = vn[bb].cpu()
        assert torch.equal(kc.cpu(), ek) and torch.equal(vc.cpu(), ev)
        P = [min(max(int(pad[bb]), 0), int(lens[bb])) for bb in range(b)]
        ks = [ek[bb, P[bb]:int(lens[bb]) + nnew] for bb in range(b)]
        vs = [ev[bb, P[bb]:int(lens[bb]) + nnew] for bb in range(b)]
        ro, rlse = reference(q.cpu(), ks, vs, causal, window, d ** -0.5, 0.0, slopes)
        check(o, lse, ro, rlse, BF16)


def test_cache_leftpad_past_the_length_and_with_cache_batch_idx():
    import flashattention_lab_cuda as ext

    bc, cap, hq, hkv, nq, d = 4, 150, 8, 2, 2, 128
    g = torch.Generator().manual_seed(131)
    kc, vc = make_cache(bc, cap, hkv, d, BF16, g)
    # leftpad >= L_b, no append: no key at all
    q = randn((bc, nq, hq, d), g, BF16)
    lens = torch.tensor([10, 0, cap, 77], dtype=torch.int32, device=DEV)
    pad = torch.tensor([10, 5, cap + 9, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    for s in (1, 2):
        o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=s, cache_leftpad=pad)
        assert (o == 0).all() and torch.isneginf(lse).all()
    # combined with cache_batch_idx, with an append
    idx, nnew = [3, 1], 1
    b = len(idx)
    q, kn, vn = randn((b, nq, hq, d), g, BF16), randn((b, nnew, hkv, d), g, BF16), randn((b, nnew, hkv, d), g, BF16)
    lens = torch.tensor([120, 40], dtype=torch.int32)
    pad = torch.tensor([17, 40], dtype=torch.int32)       # sequence 1: only the appended token is a key
    ek, ev = kc.cpu().clone(), vc.cpu().clone()
    o, lse = ext.ex_kvcache_forward(q, kc, vc, kn, vn, lens.to(DEV), True, None,
                                    cache_batch_idx=torch.tensor(idx, dtype=torch.int32, device=DEV), cache_leftpad=pad.to(DEV))
    for bb, row in enumerate(idx):
        ek[row, lens[bb]] = kn[bb, 0].cpu()
        ev[row, lens[bb]] = vn[bb, 0].cpu()
    assert torch.equal(kc.cpu(), ek) and torch.equal(vc.cpu(), ev)
    ks = [ek[row, int(pad[bb]):int(lens[bb]) + nnew] for bb, row in enumerate(idx)]
    vs = [ev[row, int(pad[bb]):int(lens[bb]) + nnew] for bb, row in enumerate(idx)]
    ro, rlse = reference(q.cpu(), ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)


def test_identity_index_and_zero_leftpad_equal_the_plain_call_bitwise():
    import flashattention_lab_cuda as ext

    b, cap, hq, hkv, nq, d = 3, 700, 8, 2, 1, 128
    g = torch.Generator().manual_seed(141)
    kc, vc = make_cache(b, cap, hkv, d, BF16, g)
    q = randn((b, nq, hq, d), g, BF16)
    lens = torch.tensor([700, 1, 333], dtype=torch.int32, device=DEV)
    ident, zero = torch.arange(b, dtype=torch.int32, device=DEV), torch.zeros(b, dtype=torch.int32, device=DEV)
    for s in (1, 4, 0):
        o0, l0 = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=s)
        o1, l1 = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=s, cache_batch_idx=ident, cache_leftpad=zero)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
