"""GPU: sparse MLA decoding (flash_mla_sparse_attn; fa_mla_sparse_forward: attention over a per-query list of cached tokens, q and
k_cache 64 wide, qv, v_cache and o 512 wide) against the fp64 reference of tests/mla_sparse_ref.py, with the tolerances of
tests/test_kvcache_gpu.py::check: one, two and four waves a workgroup, a partial and an exact row tile, more than one workgroup
of heads, two K/V heads, every topk around the 32-entry tile, dead sequences and dead lists, invalid entries of every kind, the
splits, NaN in every cache row that no visible entry names, the causal bound, pages, the two caches as slices of one pool,
cache_batch_idx, a shared list against a list per K/V head, and graph replay.  Inputs are randn rounded to the 16-bit dtype; a
reference is computed once per problem and shared."""
import functools

import pytest
import torch

from tests.kvcache_paged_ref import paged_tokens
from tests.mla_sparse_ref import mla_sparse_reference, visible_entries
from tests.test_kvcache_gpu import check
from tests.test_kvcache_qv_gpu import paged_problem, problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
D, DV, CAP = 64, 512, 304
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def sparse(*args, **kw):
    from common.attention_ex import flash_mla_sparse_attn

    return flash_mla_sparse_attn(*args, return_softmax_lse=True, **kw)


def on_dev(*ts):
    return [t.to(DEV) for t in ts]


def make_indices(lens, nq, hkv, topk, seed, cap=CAP, dead_list=True):
    """(B, Nq, H_kv, topk) int32 on the CPU: per list n draws from [0, len) at random list positions (so tokens repeat), n between
    1 and topk - 5 (topk < 8: topk), -1 elsewhere, and five of the -1 replaced by entries that are no keys: len, another position
    in [len, cap + 50), INT_MIN, INT_MAX, -7.  The lists of a dead sequence hold positions of the cache, none visible.  dead_list: the last list of
    the last live sequence is all -1."""
    g = torch.Generator().manual_seed(seed)
    b = len(lens)
    ix = torch.full((b, nq, hkv, topk), -1, dtype=torch.int64)
    for s in range(b):
        for i in range(nq):
            for hk in range(hkv):
                pos = torch.randperm(topk, generator=g)
                if lens[s] == 0:
                    ix[s, i, hk] = torch.randint(0, cap, (topk,), generator=g)
                    continue
                n = int(torch.randint(1, (topk if topk < 8 else topk - 5) + 1, (1,), generator=g))
                ix[s, i, hk, pos[:n]] = torch.randint(0, lens[s], (n,), generator=g)
                junk = [lens[s], int(torch.randint(lens[s], cap + 50, (1,), generator=g)), INT_MIN, INT_MAX, -7]
                for p, val in zip(pos[n:].tolist(), junk):
                    ix[s, i, hk, p] = val
    if dead_list:
        live = max(s for s in range(b) if lens[s] > 0)
        ix[live, nq - 1, hkv - 1] = -1
    return ix.to(torch.int32)


def lists_for(ix, hkv):
    """the tensor handed to the call: (B, Nq, topk) for one K/V head, (B, Nq, H_kv, topk) otherwise"""
    return ix[:, :, 0].contiguous() if hkv == 1 else ix


@functools.lru_cache(maxsize=None)
def case(dtype, hq, hkv, nq, topk, lens, causal=False):
    """CPU tensors (q, qv, k_cache, v_cache, indices) of a B = 3 problem and its fp64 reference"""
    q, qv, kc, vc = problem(dtype, 3, hq, hkv, nq)
    ix = lists_for(make_indices(lens, nq, hkv, topk, 100 * hq + topk), hkv)
    ref = mla_sparse_reference(q, qv, kc, vc, ix, torch.tensor(lens, dtype=torch.int32), causal)
    return (q, qv, kc, vc, ix), ref


# (H_q, H_kv, Nq), topk, lengths: one wave with a partial and an exact row tile, G = 3 with three tokens, four waves with an idle one
# (G = 40), two K/V heads, two workgroups of four waves (G = 128), and two waves (G = 24); every topk of {1, 31, 32, 33, 97, 160} and
# every length of {0, 1, 33, 97, 300}; every case has a dead sequence and a live one with a list that is all -1
SHAPES = [((1, 1, 1), 1, (0, 33, 300)), ((3, 1, 3), 31, (1, 97, 0)), ((16, 1, 1), 32, (33, 0, 300)), ((40, 1, 2), 33, (97, 300, 0)),
          ((8, 2, 2), 97, (0, 97, 33)), ((128, 1, 1), 160, (300, 0, 1)), ((24, 1, 2), 160, (0, 300, 97))]


@pytest.mark.parametrize("dtype", (BF16, F16), ids=("bf16", "f16"))
@pytest.mark.parametrize("shape,topk,lens", SHAPES, ids=[f"hq{s[0]}_hkv{s[1]}_nq{s[2]}_topk{t}" for s, t, _l in SHAPES])
def test_reference_parity(dtype, shape, topk, lens):
    hq, hkv, nq = shape
    (q, qv, kc, vc, ix), (ro, rlse) = case(dtype, hq, hkv, nq, topk, lens)
    o, lse = sparse(*on_dev(q, qv, kc, vc, ix), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert o.shape == (3, nq, hq, DV) and o.dtype == dtype and lse.shape == (3, hq, nq) and lse.dtype == torch.float32
    check(o, lse, ro, rlse, dtype)
    dead = lens.index(0)
    assert (o[dead] == 0).all() and (lse[dead] == -float("inf")).all()
    live = max(s for s in range(3) if lens[s] > 0)                 # its last list is all -1: the heads of the last K/V head
    g = hq // hkv
    assert (o[live, nq - 1, hq - g:] == 0).all() and (lse[live, hq - g:, nq - 1] == -float("inf")).all()
    assert torch.isfinite(lse[3 - dead - live]).any()


def test_topk_zero_gives_zeros():
    q, qv, kc, vc = on_dev(*problem(BF16, 3, 16, 1, 1))
    o, lse = sparse(q, qv, kc, vc, torch.empty((3, 1, 0), dtype=torch.int32, device=DEV), cache_seqlens=200)
    assert (o == 0).all() and (lse == -float("inf")).all()


@pytest.mark.parametrize("shape", ((16, 1, 1), (40, 1, 2)), ids=("hq16_nq1", "hq40_nq2"))
def test_every_split_count_is_within_tolerance_and_deterministic(shape):
    hq, hkv, nq = shape
    lens = (33, 0, 300)
    (q, qv, kc, vc, ix), (ro, rlse) = case(BF16, hq, hkv, nq, 160, lens)
    dq, dqv, dkc, dvc, dix = on_dev(q, qv, kc, vc, ix)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for splits in (1, 2, 5, 0):
        o, lse = sparse(dq, dqv, dkc, dvc, dix, cache_seqlens=sl, num_splits=splits)
        check(o, lse, ro, rlse, BF16)
        o2, lse2 = sparse(dq, dqv, dkc, dvc, dix, cache_seqlens=sl, num_splits=splits)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), splits
    # more splits than tiles (topk = 33: two tiles): the empty ones carry no weight
    (q, qv, kc, vc, ix), (ro, rlse) = case(BF16, 40, 1, 2, 33, (97, 300, 0))
    o, lse = sparse(*on_dev(q, qv, kc, vc, ix), cache_seqlens=torch.tensor((97, 300, 0), dtype=torch.int32, device=DEV), num_splits=5)
    check(o, lse, ro, rlse, BF16)


@pytest.mark.parametrize("shape,topk,splits", (((16, 1, 1), 97, 1), ((8, 2, 2), 160, 3), ((128, 1, 1), 33, 0)),
                         ids=("hq16_topk97", "hq8_hkv2_nq2_topk160_s3", "hq128_topk33"))
def test_nothing_outside_the_lists_reaches_the_result(shape, topk, splits):
    """every cache row that no visible entry names holds NaN — the rows at and past each length, which the invalid entries point
    at, among them: o and lse stay finite and within tolerance"""
    hq, hkv, nq = shape
    lens = (97, 0, 300)
    (q, qv, kc, vc, ix), (ro, rlse) = case(BF16, hq, hkv, nq, topk, lens)
    ix4 = ix if ix.dim() == 4 else ix.unsqueeze(2)
    named = torch.zeros((3, CAP, hkv), dtype=torch.bool)
    for s in range(3):
        for i in range(nq):
            for hk in range(hkv):
                named[s, visible_entries(ix4[s, i, hk], lens[s], lens[s] - 1), hk] = True
    assert named.any() and not named[1].any() and not named[0, 97:].any() and (ix4[0] == 97).any()
    kn, vn = kc.clone(), vc.clone()
    kn[~named] = float("nan")
    vn[~named] = float("nan")
    o, lse = sparse(*on_dev(q, qv, kn, vn, ix), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), num_splits=splits)
    assert torch.isfinite(o).all() and not torch.isnan(lse).any()
    check(o, lse, ro, rlse, BF16)


@pytest.mark.parametrize("splits", (1, 3))
def test_causal_bound(splits):
    """causal with Nq = 3: row i of a sequence sees tokens up to len - 3 + i, and every list names the last token of its sequence,
    which is above the bound of rows 0 and 1.  With lengths 1 and 2 rows 0, 1 (and 0) have no key: o = 0, lse = -inf"""
    hq, hkv, nq, topk, lens = 5, 1, 3, 33, (1, 300, 2)
    q, qv, kc, vc = problem(F16, 3, hq, hkv, nq)
    ix = make_indices(lens, nq, hkv, topk, 9, dead_list=False)[:, :, 0].contiguous()
    ix[:, :, 7] = torch.tensor(lens, dtype=torch.int32).view(3, 1) - 1
    ix[:, :, 8] = 0
    sl = torch.tensor(lens, dtype=torch.int32)
    ro, rlse = mla_sparse_reference(q, qv, kc, vc, ix, sl, True)
    o, lse = sparse(*on_dev(q, qv, kc, vc, ix), cache_seqlens=sl.to(DEV), causal=True, num_splits=splits)
    check(o, lse, ro, rlse, F16)
    assert (lse[0, :, :2] == -float("inf")).all() and (o[0, :2] == 0).all() and torch.isfinite(lse[0, :, 2]).all()
    assert (lse[2, :, 0] == -float("inf")).all() and (o[2, 0] == 0).all() and torch.isfinite(lse[2, :, 1:]).all()
    # the bound cuts something: the call without it differs in the middle sequence
    o2, _ = sparse(*on_dev(q, qv, kc, vc, ix), cache_seqlens=sl.to(DEV), num_splits=splits)
    assert not torch.equal(o[1, 0], o2[1, 0]) and torch.equal(o[1, 2], o2[1, 2])


@pytest.mark.parametrize("ps", (16, 48))
@pytest.mark.parametrize("splits", (0, 2))
def test_paged_is_the_contiguous_call_on_the_gathered_tokens(ps, splits):
    """pools of 9 pages whose table rows share pages and name a page outside the pool inside sequence 1's length (a zero key with a
    zero value that takes part) and a negative one"""
    dtype, hq, hkv, nq, topk = BF16, 20, 2, 2, 97
    q, qv, kp, vp, table = paged_problem(dtype, ps, hq, hkv, nq, 7 + ps)
    mb = table.shape[1]
    lens = (97, 300, 33)
    sl = torch.tensor(lens, dtype=torch.int32)
    ix = make_indices(lens, nq, hkv, topk, 40 + ps, cap=mb * ps)
    ix[1, 0, 0, :4] = torch.tensor([ps, 2 * ps - 1, ps + 3, ps])          # the page outside the pool, by name
    ro, rlse = mla_sparse_reference(q, qv, kp, vp, ix, sl, True, None, table)
    dq, dqv, dkp, dvp, dtab, dsl, dix = on_dev(q, qv, kp, vp, table, sl, ix)
    o, lse = sparse(dq, dqv, dkp, dvp, dix, cache_seqlens=dsl, block_table=dtab, causal=True, num_splits=splits)
    check(o, lse, ro, rlse, dtype)
    # the same tokens in a contiguous cache of the same capacity
    kc = torch.stack([paged_tokens(kp, table[b], mb * ps, ps) for b in range(3)])
    vc = torch.stack([paged_tokens(vp, table[b], mb * ps, ps) for b in range(3)])
    o2, lse2 = sparse(dq, dqv, kc.to(DEV), vc.to(DEV), dix, cache_seqlens=dsl, causal=True, num_splits=splits)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_the_two_caches_as_slices_of_one_pool_and_a_token_strided_qv(paged):
    dtype, hq, nq, ps, topk = F16, 16, 2, 32, 40
    g = torch.Generator().manual_seed(3)
    units = 7 if paged else 3
    pool = torch.randn((units, ps if paged else 100, 1, D + DV), generator=g).to(dtype).to(DEV)
    keep = pool.clone()
    q, qv = on_dev(torch.randn((3, nq, hq, D), generator=g).to(dtype), torch.randn((3, nq, hq, DV), generator=g).to(dtype))
    lens = (100, 33, 64)
    ix = make_indices(lens, nq, 1, topk, 5, cap=128 if paged else 100)[:, :, 0].contiguous().to(DEV)
    kw = dict(cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=True)
    if paged:
        kw["block_table"] = torch.tensor([[6, 0, 3, 1], [2, 2, 5, 4], [1, 3, 0, 6]], dtype=torch.int32, device=DEV)
    kview, vview = pool[..., DV:], pool[..., :DV]
    assert kview.data_ptr() == pool.data_ptr() + 2 * DV and vview.data_ptr() == pool.data_ptr() and not kview.is_contiguous()
    o, lse = sparse(q, qv, kview, vview, ix, **kw)
    o2, lse2 = sparse(q, qv, kview.contiguous(), vview.contiguous(), ix, **kw)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(pool, keep)
    table = kw["block_table"].cpu() if paged else None
    ro, rlse = mla_sparse_reference(q.cpu(), qv.cpu(), kview.cpu(), vview.cpu(), ix.cpu(), kw["cache_seqlens"].cpu(), True, None, table)
    check(o, lse, ro, rlse, dtype)
    # a token-strided qv (the rows of a wider projection) is taken as it is, and gives the same bits
    wide = torch.zeros((3, nq, 3, hq, DV), dtype=dtype, device=DEV)
    wide[:, :, 1] = qv
    o3, lse3 = sparse(q, wide[:, :, 1], kview, vview, ix, **kw)
    assert torch.equal(o, o3) and torch.equal(lse, lse3)


def test_cache_batch_idx_permutes_and_an_index_outside_the_cache_reads_zero_rows():
    dtype, hq, hkv, nq, topk = BF16, 16, 1, 1, 97
    lens = (97, 300, 33)
    q, qv, kc, vc = problem(dtype, 3, hq, hkv, nq)
    ix = make_indices(lens, nq, hkv, topk, 12, dead_list=False)[:, :, 0].contiguous()
    rows = torch.tensor([2, 5, 0], dtype=torch.int32)            # sequence 1 names a row the cache does not have
    sl = torch.tensor(lens, dtype=torch.int32)
    ro, rlse = mla_sparse_reference(q, qv, kc, vc, ix, sl, False, None, None, rows)
    dq, dqv, dkc, dvc, dix = on_dev(q, qv, kc, vc, ix)
    o, lse = sparse(dq, dqv, dkc, dvc, dix, cache_seqlens=sl.to(DEV), cache_batch_idx=rows.to(DEV))
    check(o, lse, ro, rlse, dtype)
    # that sequence holds no data: its visible entries are zero keys with zero values, so o = 0 exactly and lse = log(their number)
    nvis = len(visible_entries(ix[1, 0], 300, 299))
    assert (o[1] == 0).all() and torch.allclose(lse[1].cpu(), torch.full((hq, 1), float(torch.tensor(float(nvis)).log())))
    straight, _ = sparse(dq[:1], dqv[:1], dkc[2:], dvc[2:], dix[:1], cache_seqlens=sl[:1].to(DEV))
    assert torch.equal(o[0], straight[0])


def test_a_shared_list_is_the_list_repeated_per_kv_head():
    dtype, hq, hkv, nq, topk = BF16, 8, 2, 2, 97
    lens = (0, 97, 33)
    q, qv, kc, vc = on_dev(*problem(dtype, 3, hq, hkv, nq))
    ix3 = make_indices(lens, nq, 1, topk, 31)[:, :, 0].contiguous().to(DEV)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = sparse(q, qv, kc, vc, ix3, cache_seqlens=sl)
    for ix4 in (ix3.unsqueeze(2).repeat(1, 1, hkv, 1), ix3.unsqueeze(2).expand(-1, -1, hkv, -1)):
        o2, lse2 = sparse(q, qv, kc, vc, ix4, cache_seqlens=sl)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)
    ro, rlse = mla_sparse_reference(q.cpu(), qv.cpu(), kc.cpu(), vc.cpu(), ix3.cpu(), sl.cpu())
    check(o, lse, ro, rlse, dtype)
    # the order of a list changes the result by rounding only
    perm = torch.randperm(topk, generator=torch.Generator().manual_seed(1)).to(DEV)
    o3, lse3 = sparse(q, qv, kc, vc, ix3[:, :, perm].contiguous(), cache_seqlens=sl)
    check(o3, lse3, ro, rlse, dtype)


def test_graph_replay_with_changed_indices_lengths_and_table():
    dtype, hq, hkv, nq, ps, topk = BF16, 16, 1, 1, 16, 97
    q, qv, kp, vp, table = paged_problem(dtype, ps, hq, hkv, nq, 23)
    cap = table.shape[1] * ps
    dq, dqv, dkp, dvp = on_dev(q, qv, kp, vp)
    tdev = table.to(DEV)
    lens = torch.tensor([40, 17, 300], dtype=torch.int32, device=DEV)
    dix = make_indices((40, 17, 300), nq, hkv, topk, 1, cap=cap)[:, :, 0].contiguous().to(DEV)
    sparse(dq, dqv, dkp, dvp, dix, cache_seqlens=lens, block_table=tdev, causal=True)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = sparse(dq, dqv, dkp, dvp, dix, cache_seqlens=lens, block_table=tdev, causal=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.Generator().manual_seed(2)
    for seed, new_lens in ((2, (300, 0, 33)), (3, (1, 336, 97))):
        table = torch.stack([torch.randperm(9, generator=g).repeat(3)[:table.shape[1]] for _ in range(3)]).to(torch.int32)
        ix = make_indices(new_lens, nq, hkv, topk, seed, cap=cap)[:, :, 0].contiguous()
        tdev.copy_(table)
        dix.copy_(ix)
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32))
        dq.copy_(torch.randn(q.shape, generator=g).to(dtype))
        dqv.copy_(torch.randn(qv.shape, generator=g).to(dtype))
        graph.replay()
        torch.cuda.synchronize()
        eager = sparse(dq, dqv, dkp, dvp, dix, cache_seqlens=lens, block_table=tdev, causal=True)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        ro, rlse = mla_sparse_reference(dq.cpu(), dqv.cpu(), kp, vp, ix, lens.cpu(), True, None, table)
        check(out[0], out[1], ro, rlse, dtype)


def test_default_scale_and_an_explicit_one():
    hq, hkv, nq, topk, lens = 16, 1, 1, 32, (33, 0, 300)
    (q, qv, kc, vc, ix), _ref = case(BF16, hq, hkv, nq, topk, lens)
    dev = on_dev(q, qv, kc, vc, ix)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = sparse(*dev, cache_seqlens=sl)
    o2, lse2 = sparse(*dev, cache_seqlens=sl, softmax_scale=(D + DV) ** -0.5)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o3, lse3 = sparse(*dev, cache_seqlens=sl, softmax_scale=0.11)
    ro, rlse = mla_sparse_reference(q, qv, kc, vc, ix, sl.cpu(), False, 0.11)
    check(o3, lse3, ro, rlse, BF16)
    assert not torch.equal(o, o3)
