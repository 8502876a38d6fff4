"""GPU: flash_attention_varlen over a paged K/V cache (block_table; fa_ex_forward_varlen_paged).  The paged kernels differ from the
packed ones only in where a K/V tile's rows come from, so every sequence of a paged call must have the bits of the packed call
on the same tokens gathered into packed k, v — torch.equal on o and lse, no tolerance — on the MFMA kernels and on the exact-f32
fallback; a few cases also go against the fp64 oracle of tests/test_varlen_gpu.py.  Then the table as an untrusted input, prefix
sharing, strided pools, a pool above 4 GiB and graph replay.  The pools are filled with NaN wherever no token lives: a read past
a sequence's keys or from a page it does not own would show in the result."""
import functools
import itertools
import math

import pytest
import torch

from tests.test_varlen_gpu import _cu, check_against_oracle, oracle_varlen
from tests.varlen_paged_ref import build_pool, gather

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# mixed lengths in one batch: empty sides, one key, a page, a tile minus / plus one, several tiles; len_q > len_k (257 > 129)
LENS = {
    "A": ([257, 1, 40, 0, 40], [129, 0, 300, 16, 127]),
    "B": ([1, 257, 0, 40, 40], [1, 300, 129, 16, 0]),
}
MASKS = {"none": (False, (-1, -1)), "causal": (True, (-1, -1)), "win5_0": (False, (5, 0)), "causal_win130": (True, (130, -1))}
MODS = ("none", "softcap_alibi", "sinks")


def _pairwise(dims):
    """a small set of tuples of the product of `dims` in which every pair of values of two dims occurs (greedy)"""
    todo = {(i, a, j, b) for i, j in itertools.combinations(range(len(dims)), 2) for a in dims[i] for b in dims[j]}
    out = []
    prod = list(itertools.product(*dims))
    while todo:
        best = max(prod, key=lambda t: sum((i, t[i], j, t[j]) in todo for i, j in itertools.combinations(range(len(dims)), 2)))
        todo -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(dims)), 2)}
        out.append(best)
    return out


CASES = _pairwise([("bf16", "f16"), (64, 128, 40, 72), ((4, 4), (4, 2), (6, 2)), (16, 48, 256), tuple(MASKS), MODS, tuple(LENS)])
assert len(CASES) <= 60
DT = {"bf16": BF16, "f16": F16, "f32": F32}


def _mods(mod, b, hq, seed):
    g = torch.Generator().manual_seed(seed)
    if mod == "softcap_alibi":
        return dict(softcap=9.0, alibi_slopes=(torch.rand((b, hq), generator=g) * 0.3).to(DEV))
    if mod == "sinks":
        s = torch.randn((hq,), generator=g)
        s[1] = -math.inf
        return dict(sinks=s.to(DEV))
    return {}


def _tokens(lens_q, lens_k, hq, hkv, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((sum(lens_q), hq, d), generator=g).to(dtype)
    ks = [torch.randn((n, hkv, d), generator=g).to(dtype) for n in lens_k]
    vs = [torch.randn((n, hkv, d), generator=g).to(dtype) for n in lens_k]
    return q, ks, vs


def _packed(ks):
    return torch.cat(ks).to(DEV) if sum(k.shape[0] for k in ks) else torch.zeros((0,) + tuple(ks[0].shape[1:]), dtype=ks[0].dtype, device=DEV)


def _both(q, ks, vs, lens_q, lens_k, ps, causal, window, mods, path=0, seed=0, junk=1000):
    """((o, lse) of the paged call, (o, lse) of the packed call on the gathered tokens, the device pools and table)"""
    import flashattention_lab_cuda as ext

    d = q.shape[2]
    kp, vp, table = build_pool(ks, vs, ps, seed=seed)
    kp, vp, table, qd = kp.to(DEV), vp.to(DEV), table.to(DEV), q.to(DEV)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    mq, mk = max(lens_q), max(lens_k)
    ext.set_option("ex_path", path)
    try:
        # (only the differences of cu_seqlens_k count for a pool: shifted by `junk`)
        got = ext.ex_varlen_forward(qd, kp, vp, cu_q, cu_k + junk, mq, mk, causal, d ** -0.5, window=window, block_table=table, **mods)
        ref = ext.ex_varlen_forward(qd, _packed(ks), _packed(vs), cu_q, cu_k, mq, mk, causal, d ** -0.5, window=window, **mods)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return got, ref, (kp, vp, table)


def _same(got, ref, what=""):
    assert torch.equal(got[0], ref[0]), f"o differs {what}: max |diff| {(got[0].float() - ref[0].float()).abs().max().item()}"
    assert torch.equal(got[1], ref[1]), f"lse differs {what}"
    assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), f"NaN {what}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-d{c[1]}-h{c[2][0]}_{c[2][1]}-ps{c[3]}-{c[4]}-{c[5]}-{c[6]}")
def test_paged_is_bitwise_the_packed_call_on_the_gathered_tokens(case):
    dt, d, (hq, hkv), ps, mask, mod, lens = case
    lens_q, lens_k = LENS[lens]
    causal, window = MASKS[mask]
    q, ks, vs = _tokens(lens_q, lens_k, hq, hkv, d, DT[dt], seed=d + ps)
    got, ref, _ = _both(q, ks, vs, lens_q, lens_k, ps, causal, window, _mods(mod, len(lens_q), hq, d), path=3, seed=ps + d)
    _same(got, ref, str(case))


FALLBACK = [("f32", 64, (4, 2), 48, "causal", "softcap_alibi", "A"), ("bf16", 136, (4, 4), 16, "causal_win130", "sinks", "B"),
            ("bf16", 20, (6, 2), 256, "win5_0", "none", "A"), ("f32", 64, (4, 4), 16, "none", "none", "B")]


@pytest.mark.parametrize("case", FALLBACK, ids=lambda c: f"{c[0]}-d{c[1]}-ps{c[3]}-{c[4]}-{c[5]}")
def test_fallback_is_bitwise_the_packed_call_on_the_gathered_tokens(case):
    dt, d, (hq, hkv), ps, mask, mod, lens = case
    lens_q, lens_k = LENS[lens]
    causal, window = MASKS[mask]
    q, ks, vs = _tokens(lens_q, lens_k, hq, hkv, d, DT[dt], seed=d)
    got, ref, _ = _both(q, ks, vs, lens_q, lens_k, ps, causal, window, _mods(mod, len(lens_q), hq, d), path=0, seed=d)
    _same(got, ref, str(case))


def test_exact_path_option_takes_the_fallback_for_a_shape_the_mfma_kernels_take():
    lens_q, lens_k = LENS["A"]
    q, ks, vs = _tokens(lens_q, lens_k, 4, 2, 64, BF16, seed=5)
    got, ref, _ = _both(q, ks, vs, lens_q, lens_k, 48, True, (-1, -1), {}, path=1, seed=5)
    _same(got, ref)


ORACLE = [("bf16", 128, (4, 2), 48, "causal", "A", 3), ("f16", 64, (6, 2), 16, "causal_win130", "B", 3),
          ("bf16", 72, (4, 4), 256, "none", "A", 3), ("f32", 64, (4, 2), 48, "win5_0", "B", 0)]


@pytest.mark.parametrize("case", ORACLE, ids=lambda c: f"{c[0]}-d{c[1]}-ps{c[3]}-{c[4]}")
def test_paged_matches_the_fp64_oracle(case):
    dt, d, (hq, hkv), ps, mask, lens, path = case
    lens_q, lens_k = LENS[lens]
    causal, window = MASKS[mask]
    q, ks, vs = _tokens(lens_q, lens_k, hq, hkv, d, DT[dt], seed=d + 1)
    got, _ref, _ = _both(q, ks, vs, lens_q, lens_k, ps, causal, window, {}, path=path, seed=d)
    k, v = torch.cat(ks), torch.cat(vs)
    ref = oracle_varlen(q, k, v, torch.zeros_like(q), lens_q, lens_k, causal, window, d ** -0.5)
    # forward only: the oracle's own gradients stand in for the three backward results
    check_against_oracle((got[0], got[1]) + tuple(ref[2:]), ref, lens_q, lens_k, DT[dt], str(case))


# ---- the table is untrusted
@functools.lru_cache(maxsize=None)
def _base(d=128, ps=16, dtype=BF16):
    lens_q, lens_k = [40, 257, 3], [100, 300, 17]
    q, ks, vs = _tokens(lens_q, lens_k, 4, 2, d, dtype, seed=77)
    kp, vp, table = build_pool(ks, vs, ps, seed=3, max_blocks=24)
    return lens_q, lens_k, q.to(DEV), ks, vs, kp, vp, table


def _call(q, kp, vp, table, cu_q, cu_k, mq, mk, causal=True, **kw):
    import flashattention_lab_cuda as ext

    out = ext.ex_varlen_forward(q, kp, vp, cu_q, cu_k, mq, mk, causal, q.shape[2] ** -0.5, block_table=table, **kw)
    torch.cuda.synchronize()
    return out


def _canaries(kp, vp):
    """the pools cut out of larger buffers of a sentinel, and a check that neither the pools nor their surroundings changed"""
    bufs, views = [], []
    for p in (kp, vp):
        n = p.numel()
        buf = torch.full((n + 8192,), 7.0, dtype=p.dtype, device=DEV)
        view = buf[4096:4096 + n].view(p.shape)
        view.copy_(p)
        bufs.append(buf)
        views.append(view)
    before = [b.clone() for b in bufs]

    def unchanged():
        # NaN-filled pools: compare the bits
        return all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(bufs, before))
    return views[0], views[1], unchanged


def test_pages_outside_the_pool_read_as_zeros():
    import flashattention_lab_cuda as ext

    lens_q, lens_k, q, ks, vs, kp, vp, table = _base()
    ps = 16
    kc, vc, unchanged = _canaries(kp, vp)
    bad = table.clone()
    bad[1, 2], bad[1, 9] = -1, kp.shape[0]
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    got = _call(q, kc, vc, bad.to(DEV), cu_q, cu_k, 257, 300)
    kz = [gather(kp, bad[b], n, ps) for b, n in enumerate(lens_k)]
    vz = [gather(vp, bad[b], n, ps) for b, n in enumerate(lens_k)]
    assert torch.count_nonzero(kz[1][32:48]) == 0 and torch.count_nonzero(vz[1][144:160]) == 0
    ref = ext.ex_varlen_forward(q, _packed(kz), _packed(vz), cu_q, cu_k, 257, 300, True, 128 ** -0.5)
    _same(got, ref)
    assert unchanged()


def test_table_entries_past_the_length_are_never_read():
    lens_q, lens_k, q, ks, vs, kp, vp, table = _base()
    kc, vc, unchanged = _canaries(kp, vp)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    want = _call(q, kc, vc, table.to(DEV), cu_q, cu_k, 257, 300)
    wild = table.clone()
    for b, n in enumerate(lens_k):
        wild[b, (n + 15) // 16:] = 2 ** 31 - 1 - b
    _same(_call(q, kc, vc, wild.to(DEV), cu_q, cu_k, 257, 300), want)
    # ... which for a page number means: as if the table ended there (a huge number inside the length reads as zeros instead)
    assert unchanged()


def test_lengths_are_clamped_to_the_table_and_to_max_seqlen_k():
    lens_q, lens_k, q, ks, vs, kp, vp, table = _base()
    kc, vc, unchanged = _canaries(kp, vp)
    cu_q = _cu(lens_q).to(DEV)
    # every page of the short table is full of real tokens: the first 6 pages = 96 keys of sequences 0 and 1
    short = table[:, :6].contiguous()
    short[2, 1:] = short[2, 0]   # (sequence 2 claims more than it has: its first, full page over and over)
    claim = torch.tensor([0, 5000, 5000 + 2 ** 30, 2 ** 31 - 1], dtype=torch.int32).to(DEV)
    got = _call(q, kc, vc, short.to(DEV), cu_q, claim, 257, 10 ** 6)
    want = _call(q, kc, vc, short.to(DEV), cu_q, _cu([96, 96, 96]).to(DEV), 257, 96)
    _same(got, want)
    # max_seqlen_k below the lengths: the first 50 keys of each sequence
    got = _call(q, kc, vc, table.to(DEV), cu_q, _cu(lens_k).to(DEV), 257, 50, causal=False)
    want = _call(q, kc, vc, table.to(DEV), cu_q, _cu([50, 50, 17]).to(DEV), 257, 50, causal=False)
    _same(got, want)
    # negative and decreasing offsets: no keys (o = 0, lse = -inf)
    neg = torch.tensor([100, 0, -7, -2 ** 31], dtype=torch.int32).to(DEV)
    o, lse = _call(q, kc, vc, table.to(DEV), cu_q, neg, 257, 300)
    assert torch.count_nonzero(o) == 0 and torch.isinf(lse).all()
    assert unchanged()


def test_prefix_sharing():
    import flashattention_lab_cuda as ext

    ps, d = 16, 128
    lens_q, lens_k = [40, 130, 7], [100, 180, 64]
    q, ks, vs = _tokens(lens_q, lens_k, 4, 2, d, F16, seed=9)
    for b in (1, 2):   # the first 64 tokens (4 pages) of every sequence are sequence 0's
        ks[b][:64], vs[b][:64] = ks[0][:64], vs[0][:64]
    kp, vp, table = build_pool(ks, vs, ps, seed=4)
    table[1, :4] = table[0, :4]
    table[2, :4] = table[0, :4]
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    got = _call(q.to(DEV), kp.to(DEV), vp.to(DEV), table.to(DEV), cu_q, cu_k, 130, 180)
    ref = ext.ex_varlen_forward(q.to(DEV), _packed(ks), _packed(vs), cu_q, cu_k, 130, 180, True, d ** -0.5)
    _same(got, ref)


@pytest.mark.parametrize("path", [3, 1], ids=["mfma", "exact"])
def test_strided_pools(path):
    import flashattention_lab_cuda as ext

    lens_q, lens_k, q, ks, vs, kp, vp, table = _base(64, 48, F16)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    tab = table.to(DEV)
    ext.set_option("ex_path", path)
    try:
        want = _call(q, kp.to(DEV), vp.to(DEV), tab, cu_q, cu_k, 257, 300)
        # K and V as the two halves of one (num_blocks, 2, ps, H_kv, d) allocation
        kv = torch.stack([kp, vp], 1).to(DEV)
        assert kv[:, 0].stride(0) == 2 * kp.stride(0) and not kv[:, 0].is_contiguous()
        _same(_call(q, kv[:, 0], kv[:, 1], tab, cu_q, cu_k, 257, 300), want)
        # pools sliced in the head dimension: H_kv = 2 of 5 heads, K and V at different places
        wide_k = torch.full((kp.shape[0], 48, 5, 64), float("nan"), dtype=F16)
        wide_v = torch.full((kp.shape[0], 48, 5, 64), float("nan"), dtype=F16)
        wide_k[:, :, 1:3], wide_v[:, :, 3:5] = kp, vp
        wk, wv = wide_k.to(DEV)[:, :, 1:3], wide_v.to(DEV)[:, :, 3:5]
        assert wk.stride(1) == 5 * 64
        _same(_call(q, wk, wv, tab, cu_q, cu_k, 257, 300), want)
    finally:
        ext.set_option("ex_path", 0)


def test_pool_larger_than_4gib():
    ps, hkv, hq, d, nblk = 256, 8, 8, 128, 8704      # 512 KiB a page: each pool 4.25 GiB
    lens_q, lens_k = [70, 300], [600, 1000]
    q, ks, vs = _tokens(lens_q, lens_k, hq, hkv, d, BF16, seed=12)
    small_k, small_v, table = build_pool(ks, vs, ps, seed=1)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    want = _call(q.to(DEV), small_k.to(DEV), small_v.to(DEV), table.to(DEV), cu_q, cu_k, 300, 1000)
    kp = torch.empty((nblk, ps, hkv, d), dtype=BF16, device=DEV)
    vp = torch.empty((nblk, ps, hkv, d), dtype=BF16, device=DEV)
    assert kp.numel() * 2 > 2 ** 32 and vp.numel() * 2 > 2 ** 32
    big = table.clone()
    big[0, :3] = torch.tensor([5, 8500, 17])                     # sequence 0 on both sides of the 4 GiB mark
    big[1, :4] = torch.tensor([8703, 8400, 8650, 8300])          # sequence 1 beyond it, the last page included
    assert 8300 * ps * hkv * d * 2 > 2 ** 32
    for b, n in enumerate(lens_k):
        for j in range((n + ps - 1) // ps):
            kp[int(big[b, j])] = small_k[int(table[b, j])].to(DEV)
            vp[int(big[b, j])] = small_v[int(table[b, j])].to(DEV)
    got = _call(q.to(DEV), kp, vp, big.to(DEV), cu_q, cu_k, 300, 1000)
    _same(got, want)
    del kp, vp
    torch.cuda.empty_cache()


def test_graph_capture_replays_a_changed_table_and_changed_offsets():
    import flashattention_lab_cuda as ext

    lens_q, lens_k, q, ks, vs, kp, vp, table = _base()
    kpd, vpd = kp.to(DEV), vp.to(DEV)
    tab = table.to(DEV)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)

    def call(t, a, b):
        return ext.ex_varlen_forward(q, kpd, vpd, a, b, 257, 300, True, 128 ** -0.5, window=(200, -1), block_table=t)
    call(tab, cu_q, cu_k)   # warm-up (modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = call(tab, cu_q, cu_k)
    torch.cuda.current_stream().wait_stream(s)
    # the same total_q: other splits of the tokens, other lengths, sequences trading their pages
    for lq, lk, perm in (([257, 40, 3], [300, 100, 17], [1, 0, 2]), ([0, 200, 100], [17, 90, 290], [2, 0, 1]), (lens_q, lens_k, [0, 1, 2])):
        tab.copy_(table[perm].to(DEV))
        cu_q.copy_(_cu(lq).to(DEV))
        cu_k.copy_(_cu(lk).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = call(tab.clone(), cu_q.clone(), cu_k.clone())
        torch.cuda.synchronize()
        _same(out, want, str((lq, lk)))


def test_flash_attention_varlen_takes_the_table():
    from common.attention_ex import flash_attention_varlen

    lens_q, lens_k, q, ks, vs, kp, vp, table = _base()
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    sinks = torch.tensor([0.5, -math.inf, 1.0, -2.0], device=DEV)
    kw = dict(causal=True, window_size=(64, -1), softcap=20.0, sinks=sinks)
    o = flash_attention_varlen(q, kp.to(DEV), vp.to(DEV), cu_q, cu_k, 257, 300, block_table=table.to(DEV), **kw)
    ref = flash_attention_varlen(q, _packed(ks), _packed(vs), cu_q, cu_k, 257, 300, **kw)
    assert not o.requires_grad and torch.equal(o, ref)
    # a token-strided q view (the q of a packed qkv projection)
    qkv = torch.zeros((q.shape[0], 3, 4, 128), dtype=BF16, device=DEV)
    qkv[:, 0] = q
    o2 = flash_attention_varlen(qkv[:, 0], kp.to(DEV), vp.to(DEV), cu_q, cu_k, 257, 300, block_table=table.to(DEV), **kw)
    assert torch.equal(o2, o)
