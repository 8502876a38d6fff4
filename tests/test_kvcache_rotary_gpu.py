"""GPU: rotary embedding fused into flash_attn_with_kvcache / fa_ex_forward_kvcache_rotary, against the reference of
tests/kvcache_rotary_ref.py: q and k_new rotated in fp64 by the documented formulas, rounded once, then the fp64 attention of
tests/kvcache_paged_ref.py.  Tolerances are the decode path's existing ones: tests.helpers.dtype_tolerances for o, rtol = atol =
1e-3 for finite lse.  The rotated K the kernel writes to the cache must be one of the two dtype neighbours of the exact value on
every element, and the reference's rounding on all but 1 in 10^4 (tests/test_kvcache_rotary_cpu.py shows an fp32 evaluation
gives 0 mismatches on these inputs); V, the pass-through head dims and every other byte of the caches are compared bitwise."""
import pytest
import torch

from tests.helpers import dtype_tolerances
from tests.kvcache_paged_ref import reference
from tests.kvcache_rotary_ref import (CASES, case_id, case_inputs, case_reference, check_caches, rotary_reference, rotate64, round_once,
                                      tables)

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


def dev(t):
    return None if t is None else t.to(DEV)


def device_caches(r):
    """the case's caches on the device (paged256: the two halves of one buffer, pool.unbind(1))"""
    if r["kv"] is not None:
        return dev(r["kv"]).unbind(1)
    return dev(r["kc"]), dev(r["vc"])


def run_case(r, kc, vc, num_splits=None, **over):
    from common.attention_ex import flash_attn_with_kvcache

    kw = dict(rotary_cos=dev(r["cos"]), rotary_sin=dev(r["sin"]), rotary_interleaved=r["inter"], cache_seqlens=dev(r["seqlens"]),
              cache_batch_idx=dev(r["bidx"]), cache_leftpad=dev(r["leftpad"]), block_table=dev(r["table"]), causal=r["causal"],
              window_size=r["window"], softcap=r["softcap"], alibi_slopes=dev(r["slopes"]),
              num_splits=r["splits"] if num_splits is None else num_splits, return_softmax_lse=True)
    kw.update(over)
    return flash_attn_with_kvcache(dev(r["q"]), kc, vc, dev(r["kn"]), dev(r["vn"]), **kw)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_parity_and_cache_contents(idx):
    r = case_inputs(idx)
    if r["wide_tables"]:
        assert r["cos"].stride(0) > r["cos"].shape[1]
    kc, vc = device_caches(r)
    q_before = r["q"].clone()
    o, lse = run_case(r, kc, vc)
    ro, rlse, ek, ev, exact, L, _ = case_reference(r)
    check(o, lse, ro, rlse, r["dtype"])
    assert L[2] == r["cap"] - r["nnew"] and L[0] == 0                     # a clamped length and an empty sequence
    mism = check_caches(kc.cpu(), vc.cpu(), ek, ev, exact, L, r["kn"], r["rdim"], r["table"], r["bidx"])
    print(f"case {idx}: {mism} rotated K elements differ from the fp64 rounding")
    assert torch.equal(r["q"], q_before)


def _plain(b, cap, hq, hkv, nq, nnew, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, generator=g).to(dtype)   # noqa: E731
    return rn(b, nq, hq, d), rn(b, cap, hkv, d), rn(b, cap, hkv, d), rn(b, nnew, hkv, d), rn(b, nnew, hkv, d)


@pytest.mark.parametrize("interleaved", [True, False], ids=["gptj", "neox"])
@pytest.mark.parametrize("d,rdim,hkv,nq", [(128, 128, 2, 1), (64, 32, 8, 3), (256, 256, 1, 20), (96, 48, 2, 2)])
def test_identity_tables_equal_the_non_rotary_call_bitwise(d, rdim, hkv, nq, interleaved):
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq = 3, 700, 8
    q, kc0, vc0, kn, vn = (dev(t) for t in _plain(b, cap, hq, hkv, nq, nq, d, BF16, 300 + d))
    lens = torch.tensor([699 - nq, 0, 333], dtype=torch.int32, device=DEV)
    cos = torch.ones((cap, rdim // 2), dtype=BF16, device=DEV)
    sin = torch.zeros((cap, rdim // 2), dtype=BF16, device=DEV)
    for s in (1, 4, 0):
        outs = []
        for rot in (dict(), dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)):
            kc, vc = kc0.clone(), vc0.clone()
            o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, causal=True, num_splits=s, return_softmax_lse=True,
                                             **rot)
            outs.append((o, lse, kc, vc))
        for x, y in zip(*outs):
            assert torch.equal(x, y), s
        assert not torch.equal(outs[0][2], kc0)


def test_second_step_without_rotary_reads_the_rotated_cache():
    """Step 1 appends with rotary.  Step 2 passes no rotary arguments: the test rotates its q and k_new itself.  The reference of
    step 2 attends over the reference's cache of step 1, so it only agrees if the rotated K is what step 1 left in the cache."""
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, d, rdim = 3, 400, 8, 2, 128, 64
    q1, kc0, vc0, kn1, vn1 = _plain(b, cap, hq, hkv, 1, 1, d, BF16, 401)
    q2, _, _, kn2, vn2 = _plain(b, cap, hq, hkv, 1, 1, d, BF16, 402)
    lens = torch.tensor([0, 131, 398], dtype=torch.int32)
    cos, sin = tables(cap, rdim, BF16)
    kc, vc = dev(kc0), dev(vc0)
    flash_attn_with_kvcache(dev(q1), kc, vc, dev(kn1), dev(vn1), rotary_cos=dev(cos), rotary_sin=dev(sin), rotary_interleaved=False,
                            cache_seqlens=dev(lens), causal=True)
    _, _, ek, ev, exact, L, _ = rotary_reference(q1, kc0, vc0, kn1, vn1, lens, cos, sin, False, True, (-1, -1), d ** -0.5)
    check_caches(kc.cpu(), vc.cpu(), ek, ev, exact, L, kn1, rdim)
    lens2 = lens + 1
    rot = lambda x: torch.stack([round_once(rotate64(x[bb], cos, sin, [int(lens2[bb])], False), BF16) for bb in range(b)])   # noqa: E731
    q2r, kn2r = rot(q2), rot(kn2)
    o, lse = flash_attn_with_kvcache(dev(q2r), kc, vc, dev(kn2r), dev(vn2), cache_seqlens=dev(lens2), causal=True, return_softmax_lse=True)
    ks, vs = [], []
    for bb in range(b):
        n = int(lens2[bb])
        ek[bb, n], ev[bb, n] = kn2r[bb, 0], vn2[bb, 0]
        ks.append(ek[bb, :n + 1])
        vs.append(ev[bb, :n + 1])
    ro, rlse = reference(q2r, ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, BF16)
    got_k, got_v = kc.cpu(), vc.cpu()
    for bb in range(b):       # step 2 wrote what it was given, bit for bit, and left step 1's rotated token alone
        n = int(lens2[bb])
        assert torch.equal(got_k[bb, n], kn2r[bb, 0]) and torch.equal(got_v[bb, n], vn2[bb, 0])
        got_k[bb, n], got_v[bb, n] = kc0[bb, n], vc0[bb, n]
        ek[bb, n], ev[bb, n] = kc0[bb, n], vc0[bb, n]
    check_caches(got_k, got_v, ek, ev, exact, L, kn1, rdim)


@pytest.mark.parametrize("ps", [16, 256])
@pytest.mark.parametrize("d,rdim,hkv,nq,interleaved", [(128, 64, 2, 1, False), (64, 64, 1, 5, True), (256, 128, 8, 3, False)])
def test_repeatable_and_paged_equals_contiguous_bitwise(ps, d, rdim, hkv, nq, interleaved):
    import flashattention_lab_cuda as ext

    mb = {16: 40, 256: 3}[ps]
    b, cap, hq, nnew = 4, mb * ps, 8, nq
    g = torch.Generator().manual_seed(500 + ps + d)
    nblk = b * mb + 3
    rn = lambda *shape: torch.randn(shape, generator=g).to(BF16).to(DEV)   # noqa: E731
    q, kp0, vp0, kn, vn = rn(b, nq, hq, d), rn(nblk, ps, hkv, d), rn(nblk, ps, hkv, d), rn(b, nnew, hkv, d), rn(b, nnew, hkv, d)
    table = torch.randperm(nblk, generator=g)[:b * mb].view(b, mb).to(torch.int32).to(DEV)
    idx = table.long()
    kc0 = kp0[idx].reshape(b, cap, hkv, d).contiguous()
    vc0 = vp0[idx].reshape(b, cap, hkv, d).contiguous()
    lens = torch.tensor([cap - nnew, 2 * ps + 7, 0, cap - 33], dtype=torch.int32, device=DEV)
    cos, sin = (t.to(DEV) for t in tables(cap, rdim, BF16))
    rot = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
    for (causal, window), s in ((x, y) for x in ((True, (-1, -1)), (False, (37, 2)), (False, (-1, -1))) for y in (1, 4, 0)):
        runs = []
        for _ in range(2):
            kc, vc = kc0.clone(), vc0.clone()
            o, lse = ext.ex_kvcache_forward(q, kc, vc, kn, vn, lens, causal, None, window=window, num_splits=s, **rot)
            runs.append((o, lse, kc, vc))
        for x, y in zip(*runs):
            assert torch.equal(x, y), "not repeatable"
        kp, vp = kp0.clone(), vp0.clone()
        op, lp = ext.ex_kvcache_forward(q, kp, vp, kn, vn, lens, causal, None, window=window, num_splits=s, block_table=table, **rot)
        assert torch.equal(op, runs[0][0]) and torch.equal(lp, runs[0][1]), (causal, window, s)
        assert torch.equal(kp[idx].reshape(b, cap, hkv, d), runs[0][2]) and torch.equal(vp[idx].reshape(b, cap, hkv, d), runs[0][3])
    assert not torch.isnan(op).any()


def test_graph_capture_multi_step_decode():
    """One captured call, replayed: cache_seqlens is advanced on the device between replays.  One stream, no parallel branches."""
    from common.attention_ex import flash_attn_with_kvcache

    b, cap, hq, hkv, d, rdim, steps = 2, 64, 8, 2, 128, 128, 6
    g = torch.Generator().manual_seed(601)
    rn = lambda *shape: torch.randn(shape, generator=g).to(BF16)   # noqa: E731
    qs, kns, vns = rn(steps, b, 1, hq, d), rn(steps, b, 1, hkv, d), rn(steps, b, 1, hkv, d)
    cos, sin = tables(cap, rdim, BF16)
    kc, vc = torch.zeros((b, cap, hkv, d), dtype=BF16, device=DEV), torch.zeros((b, cap, hkv, d), dtype=BF16, device=DEV)
    q, kn, vn = dev(qs[0]).clone(), dev(kns[0]).clone(), dev(vns[0]).clone()
    lens = torch.zeros(b, dtype=torch.int32, device=DEV)
    one = torch.ones(b, dtype=torch.int32, device=DEV)
    kw = dict(rotary_cos=dev(cos), rotary_sin=dev(sin), rotary_interleaved=True, cache_seqlens=lens, causal=True, return_softmax_lse=True)
    flash_attn_with_kvcache(q, kc, vc, kn, vn, **kw)   # warm-up (workspace, modules); its token is overwritten by step 0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = flash_attn_with_kvcache(q, kc, vc, kn, vn, **kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ek = torch.zeros((b, cap, hkv, d), dtype=BF16)
    ev = torch.zeros((b, cap, hkv, d), dtype=BF16)
    for step in range(steps):
        q.copy_(qs[step])
        kn.copy_(kns[step])
        vn.copy_(vns[step])
        graph.replay()
        lens.add_(one)                                  # advanced on the device
        torch.cuda.synchronize()
        ro, rlse, ek, ev, _, _, _ = rotary_reference(qs[step], ek, ev, kns[step], vns[step], [step] * b, cos, sin, True, True, (-1, -1),
                                                     d ** -0.5)
        check(out[0], out[1], ro, rlse, BF16)
    # the cache's K: the whole sequence rotated at positions 0 .. steps - 1
    whole = torch.stack([round_once(rotate64(kns[:, bb, 0], cos, sin, range(steps), True), BF16) for bb in range(b)])
    got = kc.cpu()
    mism = int((got[:, :steps].double() != whole.double()).sum())
    assert mism * 10 ** 4 <= b * steps * hkv * rdim, mism
    assert torch.equal(ek[:, :steps], whole) and (got[:, steps:] == 0).all()
    assert torch.equal(vc.cpu()[:, :steps], vns[:, :, 0].transpose(0, 1))
