"""GPU: KV-cache decoding with a second query operand (flash_attn_with_kvcache(.., qv=); fa_ex_forward_kvcache_qv: q, k_cache 64
wide, qv, v_cache, o 512 wide — multi-head latent attention at decode time) against the fp64 reference of tests/mla_ref.py, with
the tolerances of tests/test_kvcache_gpu.py::check: partial, exact and several row tiles, G with two K/V heads, dead sequences,
the splits, the band, pages, the two caches as slices of one pool, cache_batch_idx, graph replay, and the call without qv.
Inputs are randn rounded to the 16-bit dtype; a reference is computed once per problem and shared."""
import functools

import pytest
import torch

from tests import mla_ref
from tests.kvcache_paged_ref import paged_tokens
from tests.test_kvcache_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
D, DV, CAP = 64, 512, 304


def kvcache(*args, **kw):
    from common.attention_ex import flash_attn_with_kvcache

    return flash_attn_with_kvcache(*args, return_softmax_lse=True, **kw)


@functools.lru_cache(maxsize=None)
def problem(dtype, b, hq, hkv, nq, cap=CAP, seed=0):
    """CPU tensors q, qv, k_cache, v_cache"""
    g = torch.Generator().manual_seed(1000 * hq + 10 * nq + seed)
    return (torch.randn((b, nq, hq, D), generator=g).to(dtype), torch.randn((b, nq, hq, DV), generator=g).to(dtype),
            torch.randn((b, cap, hkv, D), generator=g).to(dtype), torch.randn((b, cap, hkv, DV), generator=g).to(dtype))


@functools.lru_cache(maxsize=None)
def expected(dtype, b, hq, hkv, nq, lens, causal=False, window=(-1, -1), cap=CAP, seed=0):
    q, qv, kc, vc = problem(dtype, b, hq, hkv, nq, cap, seed)
    return mla_ref.mla_reference(q, qv, kc, vc, torch.tensor(lens, dtype=torch.int32), causal, window)


def on_dev(*ts):
    return [t.to(DEV) for t in ts]


# (H_q, H_kv, Nq): 1, 9, 16, 80 and 8 packed rows — a partial tile, an exact one, more than one workgroup of rows, G with two K/V
# heads; every length of {0, 1, 31, 32, 33, 97, 300} appears, and every case has a dead sequence
SHAPES = [((1, 1, 1), (0, 33, 300)), ((3, 1, 3), (1, 97, 0)), ((16, 1, 1), (31, 0, 300)), ((40, 1, 2), (32, 300, 0)), ((8, 2, 2), (0, 97, 33))]


@pytest.mark.parametrize("dtype", (BF16, F16), ids=("bf16", "f16"))
@pytest.mark.parametrize("shape,lens", SHAPES, ids=[f"hq{s[0]}_hkv{s[1]}_nq{s[2]}" for s, _l in SHAPES])
def test_reference_parity_contiguous(dtype, shape, lens):
    hq, hkv, nq = shape
    q, qv, kc, vc = on_dev(*problem(dtype, 3, hq, hkv, nq))
    o, lse = kvcache(q, kc, vc, qv=qv, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert o.shape == (3, nq, hq, DV) and o.dtype == dtype and lse.shape == (3, hq, nq) and lse.dtype == torch.float32
    ro, rlse = expected(dtype, 3, hq, hkv, nq, lens)
    check(o, lse, ro, rlse, dtype)
    dead = lens.index(0)
    assert (o[dead] == 0).all() and (lse[dead] == -float("inf")).all()


@pytest.mark.parametrize("shape", ((16, 1, 1), (40, 1, 2)), ids=("hq16_nq1", "hq40_nq2"))
def test_every_split_count_is_within_tolerance_and_deterministic(shape):
    hq, hkv, nq = shape
    lens = (33, 300)
    q, qv, kc, vc = on_dev(*problem(BF16, 2, hq, hkv, nq))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ro, rlse = expected(BF16, 2, hq, hkv, nq, lens)
    for splits in (1, 2, 5, 0):
        o, lse = kvcache(q, kc, vc, qv=qv, cache_seqlens=sl, num_splits=splits)
        check(o, lse, ro, rlse, BF16)
        o2, lse2 = kvcache(q, kc, vc, qv=qv, cache_seqlens=sl, num_splits=splits)
        assert torch.equal(o, o2) and torch.equal(lse, lse2), splits


BANDS = [(True, (-1, -1)), (False, (5, 0)), (False, (-1, 2)), (True, (1, -1))]


@pytest.mark.parametrize("causal,window", BANDS, ids=("causal", "w5_0", "w-1_2", "causal_w1"))
@pytest.mark.parametrize("splits", (1, 3))
def test_band(causal, window, splits):
    """causal with Nq = 3 (multi-token prediction), windows, and lengths 1 and 2 under the causal mask: rows 0, 1 (and 0) of those
    sequences have no key and give o = 0, lse = -inf"""
    hq, hkv, nq, lens = 5, 1, 3, (1, 300, 2)
    q, qv, kc, vc = on_dev(*problem(F16, 3, hq, hkv, nq))
    o, lse = kvcache(q, kc, vc, qv=qv, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=causal, window_size=window,
                     num_splits=splits)
    ro, rlse = expected(F16, 3, hq, hkv, nq, lens, causal, window)
    check(o, lse, ro, rlse, F16)
    if causal:
        assert (lse[0, :, :2] == -float("inf")).all() and (o[0, :2] == 0).all() and torch.isfinite(lse[0, :, 2]).all()
        assert (lse[2, :, 0] == -float("inf")).all() and (o[2, 0] == 0).all()


def paged_problem(dtype, ps, hq, hkv, nq, seed):
    """pools of 9 pages, a table of mb = 336 / ps rows' worth whose rows share pages (in another order) and name one page outside
    the pool; CPU tensors"""
    mb, nblk, b = 336 // ps, 9, 3
    g = torch.Generator().manual_seed(seed)
    q, qv = torch.randn((b, nq, hq, D), generator=g).to(dtype), torch.randn((b, nq, hq, DV), generator=g).to(dtype)
    kp, vp = torch.randn((nblk, ps, hkv, D), generator=g).to(dtype), torch.randn((nblk, ps, hkv, DV), generator=g).to(dtype)
    table = torch.stack([torch.randperm(nblk, generator=g).repeat(3)[:mb] for _ in range(b)]).to(torch.int32)
    table[1, 1] = nblk + 5      # inside sequence 1's length
    table[2, 0] = -1
    return q, qv, kp, vp, table


@pytest.mark.parametrize("ps", (16, 48))
@pytest.mark.parametrize("splits", (0, 2))
def test_paged_is_the_contiguous_call_on_the_gathered_tokens(ps, splits):
    dtype, hq, hkv, nq = BF16, 20, 2, 2
    q, qv, kp, vp, table = paged_problem(dtype, ps, hq, hkv, nq, 7 + ps)
    mb = table.shape[1]
    lens = (97, 300, 33)
    sl = torch.tensor(lens, dtype=torch.int32)
    ro, rlse = mla_ref.mla_reference(q, qv, kp, vp, sl, True, (-1, -1), None, table)
    dq, dqv, dkp, dvp, dtab, dsl = on_dev(q, qv, kp, vp, table, sl)
    o, lse = kvcache(dq, dkp, dvp, qv=dqv, cache_seqlens=dsl, block_table=dtab, causal=True, num_splits=splits)
    check(o, lse, ro, rlse, dtype)
    # the same tokens in a contiguous cache of the same capacity (a page outside the pool: a zero key with a zero value)
    kc = torch.stack([paged_tokens(kp, table[b], mb * ps, ps) for b in range(3)])
    vc = torch.stack([paged_tokens(vp, table[b], mb * ps, ps) for b in range(3)])
    o2, lse2 = kvcache(dq, kc.to(DEV), vc.to(DEV), qv=dqv, cache_seqlens=dsl, causal=True, num_splits=splits)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_the_two_caches_as_slices_of_one_pool(paged):
    dtype, hq, nq, ps = F16, 16, 2, 32
    g = torch.Generator().manual_seed(3)
    units = 7 if paged else 3
    pool = torch.randn((units, ps if paged else 100, 1, D + DV), generator=g).to(dtype).to(DEV)
    keep = pool.clone()
    q, qv = on_dev(torch.randn((3, nq, hq, D), generator=g).to(dtype), torch.randn((3, nq, hq, DV), generator=g).to(dtype))
    kw = dict(cache_seqlens=torch.tensor([100, 33, 64], dtype=torch.int32, device=DEV), causal=True)
    if paged:
        kw["block_table"] = torch.tensor([[6, 0, 3, 1], [2, 2, 5, 4], [1, 3, 0, 6]], dtype=torch.int32, device=DEV)
    kview, vview = pool[..., DV:], pool[..., :DV]
    assert kview.data_ptr() == pool.data_ptr() + 2 * DV and vview.data_ptr() == pool.data_ptr() and not kview.is_contiguous()
    o, lse = kvcache(q, kview, vview, qv=qv, **kw)
    o2, lse2 = kvcache(q, kview.contiguous(), vview.contiguous(), qv=qv, **kw)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(pool, keep)
    table = kw["block_table"].cpu() if paged else None
    ro, rlse = mla_ref.mla_reference(q.cpu(), qv.cpu(), kview.cpu(), vview.cpu(), kw["cache_seqlens"].cpu(), True, (-1, -1), None, table)
    check(o, lse, ro, rlse, dtype)
    # a token-strided qv (the rows of a wider projection) is taken as it is, and gives the same bits
    wide = torch.zeros((3, nq, 3, hq, DV), dtype=dtype, device=DEV)
    wide[:, :, 1] = qv
    o3, lse3 = kvcache(q, kview, vview, qv=wide[:, :, 1], **kw)
    assert torch.equal(o, o3) and torch.equal(lse, lse3)


def test_cache_batch_idx_permutes_and_an_index_outside_the_cache_reads_zero_rows():
    dtype, hq, hkv, nq = BF16, 16, 1, 1
    lens = (97, 300, 33)
    q, qv, kc, vc = problem(dtype, 3, hq, hkv, nq)
    idx = torch.tensor([2, 5, 0], dtype=torch.int32)            # sequence 1 names a row the cache does not have
    ro, rlse = mla_ref.mla_reference(q, qv, kc, vc, torch.tensor(lens, dtype=torch.int32), False, (-1, -1), None, None, idx)
    dq, dqv, dkc, dvc = on_dev(q, qv, kc, vc)
    o, lse = kvcache(dq, dkc, dvc, qv=dqv, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), cache_batch_idx=idx.to(DEV))
    check(o, lse, ro, rlse, dtype)
    # as without qv, that sequence holds no data: its keys read as zero rows (score 0, value 0), so o = 0 exactly
    assert (o[1] == 0).all()
    straight, _ = kvcache(dq[:1], dkc[2:], dvc[2:], qv=dqv[:1], cache_seqlens=torch.tensor(lens[:1], dtype=torch.int32, device=DEV))
    assert torch.equal(o[0], straight[0])


def test_graph_replay_with_changed_lengths_and_table():
    dtype, hq, hkv, nq, ps = BF16, 16, 1, 1, 16
    q, qv, kp, vp, table = paged_problem(dtype, ps, hq, hkv, nq, 23)
    dq, dqv, dkp, dvp = on_dev(q, qv, kp, vp)
    tdev = table.to(DEV)
    lens = torch.tensor([40, 17, 300], dtype=torch.int32, device=DEV)
    kvcache(dq, dkp, dvp, qv=dqv, cache_seqlens=lens, block_table=tdev, causal=True)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = kvcache(dq, dkp, dvp, qv=dqv, cache_seqlens=lens, block_table=tdev, causal=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.Generator().manual_seed(2)
    for new_lens in ((300, 0, 33), (1, 336, 97)):
        table = torch.stack([torch.randperm(9, generator=g).repeat(3)[:table.shape[1]] for _ in range(3)]).to(torch.int32)
        tdev.copy_(table)
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32))
        dq.copy_(torch.randn(q.shape, generator=g).to(dtype))
        dqv.copy_(torch.randn(qv.shape, generator=g).to(dtype))
        graph.replay()
        torch.cuda.synchronize()
        eager = kvcache(dq, dkp, dvp, qv=dqv, cache_seqlens=lens, block_table=tdev, causal=True)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        ro, rlse = mla_ref.mla_reference(dq.cpu(), dqv.cpu(), kp, vp, lens.cpu(), True, (-1, -1), None, table)
        check(out[0], out[1], ro, rlse, dtype)


def test_default_scale_and_an_explicit_one():
    hq, hkv, nq, lens = 16, 1, 1, (31, 0, 300)
    q, qv, kc, vc = on_dev(*problem(BF16, 3, hq, hkv, nq))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = kvcache(q, kc, vc, qv=qv, cache_seqlens=sl)
    o2, lse2 = kvcache(q, kc, vc, qv=qv, cache_seqlens=sl, softmax_scale=(D + DV) ** -0.5)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o3, lse3 = kvcache(q, kc, vc, qv=qv, cache_seqlens=sl, softmax_scale=0.11)
    cq, cqv, ckc, cvc = problem(BF16, 3, hq, hkv, nq)
    ro, rlse = mla_ref.mla_reference(cq, cqv, ckc, cvc, torch.tensor(lens, dtype=torch.int32), False, (-1, -1), 0.11)
    check(o3, lse3, ro, rlse, BF16)
    assert not torch.equal(o, o3)


@pytest.mark.parametrize("splits", (0, 1, 3))
def test_without_qv_the_call_is_the_varlen_entry_point_bit_for_bit(splits):
    """the family's prefix property for the new member: a plain d = 64 decode call through the Python wrapper, through
    fa_ex_forward_kvcache_qv with its group absent, and through fa_ex_forward_kvcache_varlen called directly"""
    import flashattention_lab_cuda as ext

    b, hq, hkv, nq, cap = 2, 8, 2, 3, 160
    g = torch.Generator().manual_seed(20)
    q, kc, vc = on_dev(torch.randn((b, nq, hq, D), generator=g).to(BF16), torch.randn((b, cap, hkv, D), generator=g).to(BF16),
                       torch.randn((b, cap, hkv, D), generator=g).to(BF16))
    lens = torch.tensor([100, 160], dtype=torch.int32, device=DEV)
    want = kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=splits)
    stream = torch.cuda.current_stream().cuda_stream
    for name, group, query in (("fa_ex_forward_kvcache_varlen", [], (ext._lib.fa_ex_kvcache_workspace_bytes_varlen, [])),
                               ("fa_ex_forward_kvcache_qv", [None, 0, 0, 0], (ext._lib.fa_ex_kvcache_workspace_bytes_qv, [0]))):
        nbytes = int(query[0](b, hq, hkv, b * nq, nq, cap, D, splits, 0, *query[1]))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=DEV)
        o, lse = torch.empty_like(q), torch.empty((b, hq, nq), dtype=torch.float32, device=DEV)
        a = [q.data_ptr(), kc.data_ptr(), vc.data_ptr(), None, None, lens.data_ptr(), o.data_ptr(), lse.data_ptr(), b, hq, hkv, nq, 0, cap, D, 2]
        for t in (q, kc, vc):
            a += [t.stride(0), t.stride(1)]
        a += [0, 0, 0, 0, 1, -1, -1, D ** -0.5, 0.0, None, 0, splits]
        a += [None, 0, 0, 0, 0, None, 0, None] + [None, None, 0, 0, 0, 0, 0] + [2, None, None, 0] + [None, 1] + [None, None, 0, 0, 0] + group
        rc = getattr(ext._lib, name)(*a, ws.data_ptr(), nbytes, stream)
        assert rc == 0, ext._lib.fa_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(o, want[0]) and torch.equal(lse, want[1]), name
