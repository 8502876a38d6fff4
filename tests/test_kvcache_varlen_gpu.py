"""GPU: packed (variable-length) queries and new keys in KV-cache decoding (flash_attn_with_kvcache with cu_seqlens_q /
cu_seqlens_k_new; fa_ex_forward_kvcache_varlen).  Every sequence of a packed call is by definition the padded call on that
sequence alone: bitwise where the split count is fixed, against the per-sequence fp64 reference everywhere
(tests/kvcache_varlen_ref.py); the append, a token-strided q, graph replay with changed offsets, offsets that lie, and calls
without a token.  One base batch holds an empty sequence, a one-row tile, a partial second tile and a five-tile sequence."""
import functools

import pytest
import torch

from tests import kvcache_varlen_ref as vr
from tests.helpers import dtype_tolerances
from tests.kvcache_fp8_ref import E4M3, absmax_scales, quantize
from tests.kvcache_paged_ref import paged_tokens
from tests.kvcache_rotary_ref import rotate64, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
HQ, CAP = 8, 384
NQ = [1, 0, 5, 20, 3]
LENS = [300, 17, 0, 64, 129]
NNEW = [1, 0, 5, 2, 3]
B, TOTAL_Q, MAX_Q = len(NQ), sum(NQ), max(NQ)
CU_Q, CU_KN = vr.lengths_to_cu(NQ), vr.lengths_to_cu(NNEW)
# one case per head dim, both dtypes at d = 128; the K/V head counts 1, 2, 8 spread over them
SHAPES = [(torch.bfloat16, 64, 8), (torch.float16, 96, 1), (torch.bfloat16, 128, 2), (torch.float16, 128, 2), (torch.bfloat16, 256, 1)]
SHAPE_IDS = ["bf16-64-8", "f16-96-1", "bf16-128-2", "f16-128-2", "bf16-256-1"]
SINKS = (0.6, -1.5, 2.5, 0.0, float("-inf"), 1.0, -0.5, 3.0)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def inputs(dtype, d, hkv, seed=0):
    """CPU tensors, made once per shape and never modified: packed q, contiguous caches, packed new keys"""
    g = torch.Generator().manual_seed(1234 + seed + d + 7 * hkv)
    rn = lambda *shape: torch.randn(shape, generator=g).to(dtype)   # noqa: E731
    return rn(TOTAL_Q, HQ, d), rn(B, CAP, hkv, d), rn(B, CAP, hkv, d), rn(sum(NNEW), hkv, d), rn(sum(NNEW), hkv, d)


def make_pool(kc, vc, ps, seed=1):
    """(k pool, v pool, table) holding the contiguous caches on shuffled pages, five spare pages"""
    mb = CAP // ps
    nblk = B * mb + 5
    table = torch.randperm(nblk, generator=torch.Generator().manual_seed(seed))[:B * mb].view(B, mb).to(torch.int32)
    kp, vp = torch.zeros((nblk, ps) + tuple(kc.shape[2:]), dtype=kc.dtype), torch.zeros((nblk, ps) + tuple(kc.shape[2:]), dtype=kc.dtype)
    kp[table.reshape(-1).long()] = kc.reshape(B * mb, ps, *kc.shape[2:])
    vp[table.reshape(-1).long()] = vc.reshape(B * mb, ps, *vc.shape[2:])
    return kp, vp, table


def check(o, lse, ro, rlse, dtype, what=""):
    """dtype_tolerances for o, rtol = atol = 1e-3 for finite lse, the -inf pattern exact; rows no sequence owns (nan in the
    reference's lse) are not compared"""
    own = ~torch.isnan(rlse[0])
    o, lse = o.cpu().double()[own], lse.cpu().double()[:, own]
    ro, rlse = ro[own], rlse[:, own]
    assert not torch.isnan(o).any() and not torch.isnan(lse).any(), what
    torch.testing.assert_close(o, ro, **dtype_tolerances(dtype), msg=lambda m: f"o {what}: {m}")
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin), f"lse -inf pattern {what}"
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-3, atol=1e-3, msg=lambda m: f"lse {what}: {m}")
    assert (o.permute(1, 0, 2)[~fin] == 0).all(), what


@pytest.mark.parametrize("mode", ["contig", "ps16", "ps48"])
@pytest.mark.parametrize("dtype,d,hkv", SHAPES, ids=SHAPE_IDS)
def test_bitwise_against_the_padded_call(dtype, d, hkv, mode):
    import flashattention_lab_cuda as ext

    q, kc, vc, _, _ = inputs(dtype, d, hkv)
    causal = d != 96
    table = None
    if mode != "contig":
        kc, vc, table = make_pool(kc, vc, int(mode[2:]))
    ks = [(paged_tokens(kc, table[b], n, kc.shape[1]) if table is not None else kc[b, :n]) for b, n in enumerate(LENS)]
    vs = [(paged_tokens(vc, table[b], n, vc.shape[1]) if table is not None else vc[b, :n]) for b, n in enumerate(LENS)]
    ro, rlse = vr.packed_reference(q, CU_Q, ks, vs, causal, (-1, -1), d ** -0.5)
    qd, kd, vd, lens, cu = q.to(DEV), kc.to(DEV), vc.to(DEV), i32(LENS), i32(CU_Q)
    td = table.to(DEV) if table is not None else None
    for splits in (1, 4, 0):
        o, lse = ext.ex_kvcache_forward(qd, kd, vd, None, None, lens, causal, None, num_splits=splits, block_table=td,
                                        cu_seqlens_q=cu, max_seqlen_q=MAX_Q)
        assert o.shape == (TOTAL_Q, HQ, d) and lse.shape == (HQ, TOTAL_Q) and lse.dtype == torch.float32
        check(o, lse, ro, rlse, dtype, f"S={splits}")
        if splits == 0:
            continue
        for b in range(B):   # the padded call on sequence b alone: the same arithmetic in the same order, other addresses
            lo, hi = CU_Q[b], CU_Q[b + 1]
            if hi == lo:
                continue
            o1, lse1 = ext.ex_kvcache_forward(qd[lo:hi].unsqueeze(0), kd if td is not None else kd[b:b + 1],
                                              vd if td is not None else vd[b:b + 1], None, None, lens[b:b + 1], causal, None,
                                              num_splits=splits, block_table=td[b:b + 1] if td is not None else None)
            assert torch.equal(o[lo:hi], o1[0]) and torch.equal(lse[:, lo:hi], lse1[0]), (splits, b)


FEATURES = ["causal", "window70", "window32", "softcap", "alibi", "idxpad", "rotary-causal-gptj", "rotary-neox", "e4m3", "sinks",
            "paged-rotary-e4m3-sinks"]


@pytest.mark.parametrize("name", FEATURES)
def test_composition(name):
    from common.attention_ex import flash_attn_with_kvcache

    dtype, d, hkv = torch.bfloat16, 128, 2
    q, kc, vc, kn, vn = inputs(dtype, d, hkv)
    scale = d ** -0.5
    causal = name in ("causal", "idxpad", "rotary-causal-gptj", "sinks", "paged-rotary-e4m3-sinks")
    window = {"window70": (7, 0), "window32": (3, 2)}.get(name, (-1, -1))
    softcap = 15.0 if name == "softcap" else 0.0
    kw, ref_kw = {}, {}
    pad, nnew, rows = [0] * B, [0] * B, list(range(B))
    kq, vq = kc, vc                                   # the caches as the call gets them
    table = kd = vd = None
    if name == "alibi":
        slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / HQ) for h in range(HQ)]).view(1, HQ) * torch.arange(1, B + 1).view(B, 1).float()
        kw["alibi_slopes"], ref_kw["slopes"] = slopes.to(DEV), slopes
    if name == "idxpad":
        g = torch.Generator().manual_seed(5)
        kq, vq = torch.randn((B + 2, CAP, hkv, d), generator=g).to(dtype), torch.randn((B + 2, CAP, hkv, d), generator=g).to(dtype)
        rows, pad = [4, 0, 5, 2, 6], [3, 5, 0, 10, 100]
        kw.update(cache_batch_idx=i32(rows), cache_leftpad=i32(pad))
    if "sinks" in name:
        kw["sinks"] = torch.tensor(SINKS, device=DEV)
        ref_kw["sinks"] = torch.tensor(SINKS)
    if "e4m3" in name:
        kd, vd = absmax_scales(kc), absmax_scales(vc)                      # (B, H_kv): the scale follows the sequence
        kq, vq = quantize(kc, kd), quantize(vc, vd)                        # uint8 codes
        kw.update(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    if "paged" in name:
        kq, vq, table = make_pool(kq, vq, 16)
        kw["block_table"] = table.to(DEV)
    if "rotary" in name:
        nnew = NNEW
        cos, sin = tables(CAP + MAX_Q, 64, dtype)
        inter = "neox" not in name
        kw.update(rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=inter, cu_seqlens_k_new=i32(CU_KN))
    kdev, vdev = kq.to(DEV), vq.to(DEV)
    if "e4m3" in name:
        kdev, vdev = kdev.view(E4M3), vdev.view(E4M3)
    for splits in (0, 1, 3):
        k2, v2 = kdev.clone(), vdev.clone()
        o, lse = flash_attn_with_kvcache(q.to(DEV), k2, v2, kn.to(DEV) if "rotary" in name else None, vn.to(DEV) if "rotary" in name else None,
                                         cache_seqlens=i32(LENS), causal=causal, window_size=window, softcap=softcap, num_splits=splits,
                                         return_softmax_lse=True, cu_seqlens_q=i32(CU_Q), max_seqlen_q=MAX_Q, **kw)
        # the sequence's keys as the caches hold them after the call (the appended ones rotated and quantised by it)
        ka, va = k2.cpu(), v2.cpu()
        if "e4m3" in name:
            ka, va = ka.view(torch.uint8), va.view(torch.uint8)
        ks, vs = [], []
        for b in range(B):
            n = LENS[b] + nnew[b]
            kb = paged_tokens(ka, table[b], n, 16) if table is not None else ka[rows[b], pad[b]:n]
            vb = paged_tokens(va, table[b], n, 16) if table is not None else va[rows[b], pad[b]:n]
            if "e4m3" in name:
                kb = kb.view(E4M3).double() * kd[b].double().view(1, hkv, 1)
                vb = vb.view(E4M3).double() * vd[b].double().view(1, hkv, 1)
            ks.append(kb)
            vs.append(vb)
        qr = q
        if "rotary" in name:   # q token i of sequence b at position L_b - P_b + i (causal), else at L_b - P_b
            pos = [LENS[b] + (i if causal else 0) for b in range(B) for i in range(NQ[b])]
            qr = rotate64(q, cos, sin, pos, inter)
        ro, rlse = vr.packed_reference(qr, CU_Q, ks, vs, causal, window, scale, softcap, **ref_kw)
        check(o, lse, ro, rlse, dtype, f"{name} S={splits}")


@pytest.mark.parametrize("mode", ["contig", "ps16", "rotary-e4m3"])
def test_append(mode):
    import flashattention_lab_cuda as ext

    dtype, d, hkv = torch.bfloat16, 128, 2
    q, kc, vc, kn, vn = inputs(dtype, d, hkv)
    seqlens = [300, 17, 0, 64, 1000]                       # the last one too large: clamped to capacity - nnew_b
    L = [min(max(x, 0), CAP - n) for x, n in zip(seqlens, NNEW)]
    kw, table = {}, None
    kq, vq = kc, vc
    if mode == "ps16":
        kq, vq, table = make_pool(kc, vc, 16)
        kw["block_table"] = table.to(DEV)
    if mode == "rotary-e4m3":
        kd, vd = absmax_scales(kc), absmax_scales(vc)
        kq, vq = quantize(kc, kd).view(E4M3), quantize(vc, vd).view(E4M3)
        cos, sin = tables(CAP + MAX_Q, 64, dtype)
        kw.update(k_descale=kd.to(DEV), v_descale=vd.to(DEV), rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=False)
    k2, v2 = kq.to(DEV), vq.to(DEV)
    o, lse = ext.ex_kvcache_forward(q.to(DEV), k2, v2, kn.to(DEV), vn.to(DEV), i32(seqlens), True, None, num_splits=2,
                                    cu_seqlens_q=i32(CU_Q), cu_seqlens_k_new=i32(CU_KN), max_seqlen_q=MAX_Q, **kw)
    if mode == "rotary-e4m3":
        # the rotated, quantised bits are those of the padded call on each sequence alone; it also gives o and lse
        k1, v1 = kq.to(DEV), vq.to(DEV)
        for b in range(B):
            if NNEW[b] == 0:
                continue
            kwb = dict(kw, k_descale=kw["k_descale"][b:b + 1], v_descale=kw["v_descale"][b:b + 1])
            qb = q[CU_Q[b]:CU_Q[b + 1]].unsqueeze(0).to(DEV)
            o1, lse1 = ext.ex_kvcache_forward(qb, k1[b:b + 1], v1[b:b + 1], kn[CU_KN[b]:CU_KN[b + 1]].unsqueeze(0).to(DEV),
                                              vn[CU_KN[b]:CU_KN[b + 1]].unsqueeze(0).to(DEV), i32(seqlens[b:b + 1]), True, None, num_splits=2,
                                              **kwb)
            assert torch.equal(o[CU_Q[b]:CU_Q[b + 1]], o1[0]) and torch.equal(lse[:, CU_Q[b]:CU_Q[b + 1]], lse1[0]), b
        assert not torch.equal(k1.view(torch.uint8), kq.to(DEV).view(torch.uint8))
        assert torch.equal(k2.view(torch.uint8), k1.view(torch.uint8)) and torch.equal(v2.view(torch.uint8), v1.view(torch.uint8))
        return
    ek, ev = kq.clone(), vq.clone()
    for b in range(B):
        for n in range(NNEW[b]):
            unit, slot = (int(table[b, (L[b] + n) // 16]), (L[b] + n) % 16) if table is not None else (b, L[b] + n)
            ek[unit, slot], ev[unit, slot] = kn[CU_KN[b] + n], vn[CU_KN[b] + n]
    assert torch.equal(k2.cpu(), ek) and torch.equal(v2.cpu(), ev)          # nothing but the appended slots changed
    ks = [(paged_tokens(ek, table[b], L[b] + NNEW[b], 16) if table is not None else ek[b, :L[b] + NNEW[b]]) for b in range(B)]
    vs = [(paged_tokens(ev, table[b], L[b] + NNEW[b], 16) if table is not None else ev[b, :L[b] + NNEW[b]]) for b in range(B)]
    ro, rlse = vr.packed_reference(q, CU_Q, ks, vs, True, (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, dtype, mode)


def test_padded_new_keys_with_packed_queries():
    from common.attention_ex import flash_attn_with_kvcache

    dtype, d, hkv, nnew = torch.float16, 64, 8, 2
    q, kc, vc, kn, vn = inputs(dtype, d, hkv)
    kn, vn = kn[:B * nnew].view(B, nnew, hkv, d), vn[:B * nnew].view(B, nnew, hkv, d)
    k2, v2 = kc.to(DEV), vc.to(DEV)
    o, lse = flash_attn_with_kvcache(q.to(DEV), k2, v2, kn.to(DEV), vn.to(DEV), cache_seqlens=i32(LENS), causal=True,
                                     return_softmax_lse=True, cu_seqlens_q=i32(CU_Q), max_seqlen_q=MAX_Q)
    ek, ev = kc.clone(), vc.clone()
    for b in range(B):
        ek[b, LENS[b]:LENS[b] + nnew], ev[b, LENS[b]:LENS[b] + nnew] = kn[b], vn[b]
    assert torch.equal(k2.cpu(), ek) and torch.equal(v2.cpu(), ev)
    ro, rlse = vr.packed_reference(q, CU_Q, [ek[b, :LENS[b] + nnew] for b in range(B)], [ev[b, :LENS[b] + nnew] for b in range(B)], True,
                                   (-1, -1), d ** -0.5)
    check(o, lse, ro, rlse, dtype)


def test_strided_packed_q_equals_the_contiguous_call_bitwise():
    import flashattention_lab_cuda as ext

    dtype, d, hkv = torch.bfloat16, 128, 2
    q, kc, vc, _, _ = inputs(dtype, d, hkv)
    qkv = torch.randn((TOTAL_Q, 3, HQ, d)).to(dtype).to(DEV)
    qkv[:, 0] = q.to(DEV)
    view = qkv[:, 0]
    assert not view.is_contiguous() and view.stride(0) == 3 * HQ * d
    kd, vd, before = kc.to(DEV), vc.to(DEV), qkv.clone()
    for splits in (1, 4):
        a = ext.ex_kvcache_forward(view, kd, vd, None, None, i32(LENS), True, None, num_splits=splits, cu_seqlens_q=i32(CU_Q), max_seqlen_q=MAX_Q)
        c = ext.ex_kvcache_forward(q.to(DEV), kd, vd, None, None, i32(LENS), True, None, num_splits=splits, cu_seqlens_q=i32(CU_Q),
                                   max_seqlen_q=MAX_Q)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert torch.equal(qkv, before)


def test_graph_capture_replays_changed_offsets():
    from common.attention_ex import flash_attn_with_kvcache

    dtype, d, hkv = torch.bfloat16, 128, 2
    q, kc, vc, kn, vn = inputs(dtype, d, hkv)
    qd, knd, vnd = q.to(DEV), kn.to(DEV), vn.to(DEV)
    k0, v0 = kc.to(DEV), vc.to(DEV)
    kg, vg = k0.clone(), v0.clone()
    cu_q, cu_kn, lens = i32(CU_Q), i32(CU_KN), i32(LENS)
    call = lambda k, v, a, b, c: flash_attn_with_kvcache(qd, k, v, knd, vnd, cache_seqlens=c, causal=True, return_softmax_lse=True,   # noqa: E731
                                                         cu_seqlens_q=a, cu_seqlens_k_new=b, max_seqlen_q=MAX_Q)
    call(kg, vg, cu_q, cu_kn, lens)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = call(kg, vg, cu_q, cu_kn, lens)
    torch.cuda.current_stream().wait_stream(s)
    # the same total_q, max_seqlen_q and total_k_new; other lengths, other sequences empty
    for nq, nnew, ln in ((NQ, NNEW, LENS), ([20, 3, 0, 1, 5], [0, 4, 2, 5, 0], [10, 380, 300, 0, 64]), ([0, 9, 0, 20, 0], [11, 0, 0, 0, 0], [1, 2, 3, 4, 5])):
        assert sum(nq) == TOTAL_Q and sum(nnew) == sum(NNEW)
        cu_q.copy_(i32(vr.lengths_to_cu(nq)))
        cu_kn.copy_(i32(vr.lengths_to_cu(nnew)))
        lens.copy_(i32(ln))
        kg.copy_(k0)
        vg.copy_(v0)
        graph.replay()
        torch.cuda.synchronize()
        ke, ve = k0.clone(), v0.clone()
        oe, lsee = call(ke, ve, cu_q.clone(), cu_kn.clone(), lens.clone())
        assert torch.equal(out[0], oe) and torch.equal(out[1], lsee)
        assert torch.equal(kg, ke) and torch.equal(vg, ve) and not torch.equal(kg, k0)


# ---- the C entry point on o / lse / workspace cut out of the middle of canary-filled buffers
CANARY = -7.0


def raw_call(q, kc, vc, lens, cu_q, max_q, splits):
    """(o, lse, the three guarded buffers): fa_ex_forward_kvcache_varlen on a contiguous cache without new keys, causal; o, lse and
    the workspace each the middle third of a buffer filled with CANARY, so the margins hold at least total_q rows"""
    import flashattention_lab_cuda as ext

    total_q, hq, d = q.shape
    hkv = kc.shape[2]
    code = {torch.float16: 1, torch.bfloat16: 2}[q.dtype]
    o_big = torch.full((3 * total_q, hq, d), CANARY, dtype=q.dtype, device=DEV)
    lse_big = torch.full((3, hq, total_q), CANARY, dtype=torch.float32, device=DEV)
    nbytes = int(ext._lib.fa_ex_kvcache_workspace_bytes_varlen(len(lens), hq, hkv, total_q, max_q, kc.shape[1], d, splits, 0))
    ws_big = torch.full((3, max(nbytes, 256) // 4), CANARY, dtype=torch.float32, device=DEV)
    o, lse = o_big[total_q:2 * total_q], lse_big[1]
    rc = ext._lib.fa_ex_forward_kvcache_varlen(
        q.data_ptr(), kc.data_ptr(), vc.data_ptr(), 0, 0, lens.data_ptr(), o.data_ptr(), lse.data_ptr(),
        len(lens), hq, hkv, 0, 0, kc.shape[1], d, code, 0, q.stride(0), kc.stride(0), kc.stride(1), vc.stride(0), vc.stride(1), 0, 0, 0, 0,
        1, -1, -1, d ** -0.5, 0.0, 0, 0, splits,
        0, 0, 0, 0, 0, 0, 0, 0,            # no table, cache_batch_idx or cache_leftpad
        0, 0, 0, 0, 0, 0, 0,               # no rotary
        code, 0, 0, 0, 0, 1,               # a 16-bit cache, no sinks
        cu_q.data_ptr(), 0, total_q, max_q, 0,
        ws_big[1].data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, ext._lib.fa_last_error().decode()
    torch.cuda.synchronize()
    return o, lse, (o_big, lse_big, ws_big)


def margins_intact(guards):
    o_big, lse_big, ws_big = guards
    n = o_big.shape[0] // 3
    return all(bool((t == CANARY).all()) for t in (o_big[:n], o_big[2 * n:], lse_big[0], lse_big[2], ws_big[0], ws_big[2]))


@pytest.mark.parametrize("splits", [1, 4])
def test_untrusted_offsets_stay_inside_the_tensors(splits):
    dtype, d, hkv = torch.bfloat16, 128, 2
    q, kc, vc, _, _ = inputs(dtype, d, hkv)
    qd, kd, vd, lens = q.to(DEV), kc.to(DEV), vc.to(DEV), i32(LENS)
    good_o, good_lse, guards = raw_call(qd, kd, vd, lens, i32(CU_Q), MAX_Q, splits)
    assert margins_intact(guards)
    ks, vs = [kc[b, :n] for b, n in enumerate(LENS)], [vc[b, :n] for b, n in enumerate(LENS)]
    ro, rlse = vr.packed_reference(q, CU_Q, ks, vs, True, (-1, -1), d ** -0.5)
    check(good_o, good_lse, ro, rlse, dtype)
    # (offsets, max_seqlen_q, the sequences whose offsets are well formed, packed rows that no sequence owns after the clamp)
    cases = [
        (CU_Q, 5, (0, 2, 4), range(11, 26)),                          # sequence 3 longer than max_seqlen_q: cut to 5 tokens
        (CU_Q[:-1] + [TOTAL_Q + 20], MAX_Q, (0, 2, 3, 4), ()),        # an end past total_q: cut to the 3 tokens that exist
        ([0, 1, 6, 1, 26, 29], MAX_Q, (0, 4), range(21, 26)),         # a decreasing pair: sequences 1 and 3 overlap, 2 is empty
        ([-25, 1, 1, 6, 2 ** 31 - 1, -2 ** 31], MAX_Q, (), range(26, 29)),    # negative, huge, a difference past 32 bits
    ]
    for cu, max_q, formed, unowned in cases:
        o, lse, guards = raw_call(qd, kd, vd, lens, i32(cu), max_q, splits)
        assert margins_intact(guards), cu                # a missing clamp lands here, not outside the allocation
        for b in formed:
            lo, hi = CU_Q[b], CU_Q[b + 1]
            assert torch.equal(o[lo:hi], good_o[lo:hi]) and torch.equal(lse[:, lo:hi], good_lse[:, lo:hi]), (cu, b)
        for t in unowned:                                # rows of no sequence are not written
            assert bool((o[t] == CANARY).all()) and bool((lse[:, t] == CANARY).all()), (cu, t)


@pytest.mark.parametrize("splits", [1, 4])
def test_all_empty_call_touches_nothing(splits):
    from common.attention_ex import flash_attn_with_kvcache

    dtype, d, hkv = torch.bfloat16, 128, 2
    q, kc, vc, kn, vn = inputs(dtype, d, hkv)
    kd, vd = kc.to(DEV), vc.to(DEV)
    o, lse, guards = raw_call(q.to(DEV), kd, vd, i32(LENS), i32([0] * (B + 1)), MAX_Q, splits)
    assert all(bool((g == CANARY).all()) for g in guards[:2])
    o, lse, guards = raw_call(q.to(DEV), kd, vd, i32(LENS), i32([7] * (B + 1)), 0, splits)        # max_seqlen_q = 0: no launch at all
    assert all(bool((g == CANARY).all()) for g in guards)
    # no q token at all, and the new keys are still appended
    o, lse = flash_attn_with_kvcache(q[:0].to(DEV), kd, vd, kn.to(DEV), vn.to(DEV), cache_seqlens=i32(LENS), causal=True, num_splits=splits,
                                     return_softmax_lse=True, cu_seqlens_q=i32([0] * (B + 1)), cu_seqlens_k_new=i32(CU_KN), max_seqlen_q=0)
    assert o.shape == (0, HQ, d) and lse.shape == (HQ, 0)
    ek, ev = kc.clone(), vc.clone()
    for b in range(B):
        ek[b, LENS[b]:LENS[b] + NNEW[b]], ev[b, LENS[b]:LENS[b] + NNEW[b]] = kn[CU_KN[b]:CU_KN[b + 1]], vn[CU_KN[b]:CU_KN[b + 1]]
    assert torch.equal(kd.cpu(), ek) and torch.equal(vd.cpu(), ev)
