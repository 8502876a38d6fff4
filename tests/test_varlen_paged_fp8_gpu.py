"""GPU: flash_attention_varlen over an e4m3 paged K/V cache (block_table + k_descale / v_descale; fa_ex_forward_varlen_paged_fp8).
Widening e4m3 to q's dtype is exact and the kernels keep their 16-bit loop, so
  1. with null scales o and lse have the bits of the 16-bit paged call on the pools widened to q's dtype,
  2. with power-of-two scales unit (b, hk) has the bits of that call at softmax_scale * k_descale[b, hk], o times v_descale,
  3. with arbitrary scales the call meets the fp64 oracle on the dequantised tokens at the 16-bit kernel's own bars,
  4. the cache flash_attn_with_kvcache appended to (quantising) is the cache this call reads, with the same scales,
  5. the table stays untrusted, the pools may be views, and a captured call replays changed tables, offsets and scale values.
The pools hold the e4m3 NaN code 0x7f wherever no token lives: a stray read shows in the result.
v_descale is checked bitwise in bf16 only (o == o_ref * v_descale): bf16 has fp32's exponent range, while f16 subnormals would make
the product inexact; the oracle test covers v_descale in f16."""
import functools
import math

import pytest
import torch

from tests.kvcache_fp8_ref import E4M3, FIXED_SCALES, dequantize, quantize
from tests.test_varlen_gpu import _cu, check_against_oracle, oracle_varlen
from tests.test_varlen_paged_gpu import LENS, MASKS, MODS, _mods, _pairwise, _same, _tokens
from tests.varlen_paged_ref import build_pool, gather

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DT = {"bf16": BF16, "f16": F16}
NAN8 = 0x7F
# (head_dim, ex_path): the MFMA kernels or fail; the exact-f32 fallback for d > 128 and by option
DP = ((64, 3), (128, 3), (40, 3), (72, 3), (136, 1), (200, 1), (64, 1))
CASES = _pairwise([("bf16", "f16"), DP, ((4, 4), (4, 2), (6, 2)), (16, 48, 256), tuple(MASKS), MODS, tuple(LENS)])
assert len(CASES) <= 40, len(CASES)
POW2 = (2.0 ** -3, 2.0 ** -1, 1.0, 2.0, 4.0)


def _ids(c):
    return f"{c[0]}-d{c[1][0]}-p{c[1][1]}-h{c[2][0]}_{c[2][1]}-ps{c[3]}-{c[4]}-{c[5]}-{c[6]}"


def _pools8(ks, vs, ps, seed, kq=None, vq=None, **kw):
    """(k_pool, v_pool, table) of uint8 e4m3 codes: sequence b quantised with the scales kq[b] / vq[b] ((H_kv,) each; None: 1.0),
    scattered behind a shuffled table, 0x7f everywhere else"""
    k8 = [quantize(k[None], 1.0 if kq is None else kq[b])[0] for b, k in enumerate(ks)]
    v8 = [quantize(v[None], 1.0 if vq is None else vq[b])[0] for b, v in enumerate(vs)]
    return build_pool(k8, v8, ps, seed=seed, fill=NAN8, **kw)


def _widen(pool8, dtype):
    return pool8.view(E4M3).to(dtype)   # exact: every e4m3 value is an f16 and a bf16 number (0x7f stays NaN)


def _run(path, q, kp, vp, table, cu_q, cu_k, mq, mk, causal, window, scale=None, **kw):
    import flashattention_lab_cuda as ext

    ext.set_option("ex_path", path)
    try:
        out = ext.ex_varlen_forward(q, kp, vp, cu_q, cu_k, mq, mk, causal, q.shape[2] ** -0.5 if scale is None else scale,
                                    window=window, block_table=table, **kw)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _case(case):
    """the inputs of one case of the table on the device, shared by the bitwise tests"""
    dt, (d, path), (hq, hkv), ps, mask, mod, lens = case
    lens_q, lens_k = LENS[lens]
    q, ks, vs = _tokens(lens_q, lens_k, hq, hkv, d, DT[dt], seed=d + ps)
    kp8, vp8, table = _pools8(ks, vs, ps, seed=ps + d)
    dev = dict(q=q.to(DEV), k8=kp8.to(DEV).view(E4M3), v8=vp8.to(DEV).view(E4M3), k16=_widen(kp8, DT[dt]).to(DEV),
               v16=_widen(vp8, DT[dt]).to(DEV), table=table.to(DEV), cu_q=_cu(lens_q).to(DEV), cu_k=_cu(lens_k).to(DEV))
    return dev, lens_q, lens_k


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_null_scales_have_the_bits_of_the_16_bit_call_on_the_widened_pools(case):
    dt, (d, path), (hq, hkv), ps, mask, mod, lens = case
    t, lens_q, lens_k = _case(case)
    causal, window = MASKS[mask]
    mods = _mods(mod, len(lens_q), hq, d)
    args = (t["table"], t["cu_q"], t["cu_k"], max(lens_q), max(lens_k), causal, window)
    got = _run(path, t["q"], t["k8"], t["v8"], *args, **mods)
    ref = _run(path, t["q"], t["k16"], t["v16"], *args, **mods)
    _same(got, ref, str(case))


# softcap + ALiBi and sinks among them, both paths, both scale forms ((B, H_kv), and (H_kv,) where `row` is set)
POW2_CASES = [(c, row) for c, row in zip([c for c in CASES if c[5] != "none"][:5] + [c for c in CASES if c[5] == "none"][:3],
                                         (False, True, False, True, False, False, True, False))]
assert len(POW2_CASES) >= 6 and {c[5] for c, _ in POW2_CASES} == set(MODS) and {c[1][1] for c, _ in POW2_CASES} == {1, 3}


@pytest.mark.parametrize("case,row", POW2_CASES, ids=lambda x: _ids(x) if isinstance(x, tuple) else ("Hkv" if x else "BHkv"))
def test_power_of_two_scales_have_the_bits_of_the_16_bit_call_at_the_scaled_softmax_scale(case, row):
    dt, (d, path), (hq, hkv), ps, mask, mod, lens = case
    t, lens_q, lens_k = _case(case)
    causal, window = MASKS[mask]
    b, g = len(lens_q), hq // hkv
    mods = _mods(mod, b, hq, d)
    gen = torch.Generator().manual_seed(d + ps + hq)
    shape = (hkv,) if row else (b, hkv)
    kd = torch.tensor(POW2)[torch.randint(0, len(POW2), shape, generator=gen)]
    vd = torch.tensor(POW2)[torch.randint(0, len(POW2), shape, generator=gen)] if dt == "bf16" else None   # (bf16 only: the module docstring)
    tail = (t["table"], t["cu_q"], t["cu_k"], max(lens_q), max(lens_k), causal, window)
    o, lse = _run(path, t["q"], t["k8"], t["v8"], *tail, k_descale=kd.to(DEV), v_descale=None if vd is None else vd.to(DEV), **mods)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    kd2 = kd.expand(b, hkv)
    vd2 = None if vd is None else vd.expand(b, hkv)
    starts = _cu(lens_q).tolist()
    for hk in range(hkv):
        heads = slice(hk * g, (hk + 1) * g)
        sub = {}
        if "alibi_slopes" in mods:
            sub = dict(softcap=mods["softcap"], alibi_slopes=mods["alibi_slopes"][:, heads].contiguous())
        if "sinks" in mods:
            sub = dict(sinks=mods["sinks"][heads].contiguous())
        for s in sorted(set(kd2[:, hk].tolist())):
            # one reference call per distinct scale value and head: that K/V head's query heads over that head of the widened pools
            ro, rlse = _run(path, t["q"][:, heads], t["k16"][:, :, hk:hk + 1], t["v16"][:, :, hk:hk + 1], *tail, scale=d ** -0.5 * s, **sub)
            for bi in range(b):
                if kd2[bi, hk].item() != s:
                    continue
                tok = slice(starts[bi], starts[bi + 1])
                want = ro[tok] if vd2 is None else (ro[tok].float() * vd2[bi, hk].item()).to(ro.dtype)
                assert torch.equal(o[tok, heads], want), f"o of unit ({bi}, {hk}) at k_descale {s}: {case}"
                assert torch.equal(lse[heads, tok], rlse[:, tok]), f"lse of unit ({bi}, {hk}) at k_descale {s}: {case}"


def _fixed_scales(b, hkv, shift):
    return torch.tensor([[FIXED_SCALES[(shift + 2 * bi + h) % len(FIXED_SCALES)] for h in range(hkv)] for bi in range(b)], dtype=torch.float32)


# dtype, d, heads, ps, mask, lens, ex_path: the bars are those of tests/test_varlen_paged_gpu.py::test_paged_matches_the_fp64_oracle
ORACLE = [("bf16", 128, (4, 2), 48, "causal", "A", 3), ("f16", 64, (6, 2), 16, "causal_win130", "B", 3),
          ("f16", 72, (4, 4), 256, "none", "A", 3), ("bf16", 40, (4, 2), 16, "win5_0", "B", 3),
          ("bf16", 136, (4, 2), 48, "causal", "B", 1), ("f16", 128, (4, 4), 16, "none", "A", 1)]


@pytest.mark.parametrize("case", ORACLE, ids=lambda c: f"{c[0]}-d{c[1]}-ps{c[3]}-{c[4]}-p{c[6]}")
def test_arbitrary_scales_match_the_fp64_oracle_on_the_dequantised_tokens(case):
    dt, d, (hq, hkv), ps, mask, lens, path = case
    lens_q, lens_k = LENS[lens]
    causal, window = MASKS[mask]
    b = len(lens_q)
    q, ks, vs = _tokens(lens_q, lens_k, hq, hkv, d, DT[dt], seed=d + 1)
    kd, vd = _fixed_scales(b, hkv, 0), _fixed_scales(b, hkv, 3)
    # (the tokens are quantised for the scales they are read with: the dequantised values are the randn tokens, rounded)
    kp8, vp8, table = _pools8(ks, vs, ps, seed=d, kq=kd, vq=vd)
    o, lse = _run(path, q.to(DEV), kp8.to(DEV).view(E4M3), vp8.to(DEV).view(E4M3), table.to(DEV), _cu(lens_q).to(DEV), _cu(lens_k).to(DEV),
                  max(lens_q), max(lens_k), causal, window, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    k64 = torch.cat([dequantize(gather(kp8, table[bi], n, ps)[None], kd[bi])[0] for bi, n in enumerate(lens_k)])
    v64 = torch.cat([dequantize(gather(vp8, table[bi], n, ps)[None], vd[bi])[0] for bi, n in enumerate(lens_k)])
    ref = oracle_varlen(q, k64, v64, torch.zeros_like(q), lens_q, lens_k, causal, window, d ** -0.5)
    check_against_oracle((o, lse) + tuple(ref[2:]), ref, lens_q, lens_k, DT[dt], str(case))


def test_one_cache_two_calls_append_then_prefill():
    from common.attention_ex import flash_attn_with_kvcache, flash_attention_varlen

    d, hq, hkv, ps, n_new, dtype = 128, 4, 2, 16, 24, BF16
    have = [100, 0, 37]                      # tokens in the cache before the append
    b, mb = len(have), 12
    g = torch.Generator().manual_seed(21)
    kd, vd = _fixed_scales(b, hkv, 1), _fixed_scales(b, hkv, 2)
    old_k = [torch.randn((n, hkv, d), generator=g).to(dtype) for n in have]
    old_v = [torch.randn((n, hkv, d), generator=g).to(dtype) for n in have]
    # pages for the tokens to come as well: the table of build_pool on full-length placeholders, the tail bytes zeroed
    full_k = [torch.cat([k, torch.zeros((n_new, hkv, d), dtype=dtype)]) for k in old_k]
    full_v = [torch.cat([v, torch.zeros((n_new, hkv, d), dtype=dtype)]) for v in old_v]
    kp8, vp8, table = _pools8(full_k, full_v, ps, seed=8, kq=kd, vq=vd, max_blocks=mb)
    kpool, vpool = kp8.to(DEV).view(E4M3), vp8.to(DEV).view(E4M3)
    q = torch.randn((b, n_new, hq, d), generator=g).to(dtype).to(DEV)
    k_new = torch.randn((b, n_new, hkv, d), generator=g).to(dtype).to(DEV)
    v_new = torch.randn((b, n_new, hkv, d), generator=g).to(dtype).to(DEV)
    tab, kdd, vdd = table.to(DEV), kd.to(DEV), vd.to(DEV)
    flash_attn_with_kvcache(q, kpool, vpool, k_new, v_new, cache_seqlens=torch.tensor(have, dtype=torch.int32, device=DEV),
                            block_table=tab, causal=True, k_descale=kdd, v_descale=vdd)
    torch.cuda.synchronize()
    lens_k = [n + n_new for n in have]
    lens_q = [n_new] * b
    qp = q.reshape(b * n_new, hq, d)
    o = flash_attention_varlen(qp, kpool, vpool, _cu(lens_q).to(DEV), _cu(lens_k).to(DEV), n_new, max(lens_k), causal=True,
                               block_table=tab, k_descale=kdd, v_descale=vdd)
    torch.cuda.synchronize()
    k_after, v_after = kpool.view(torch.uint8).cpu(), vpool.view(torch.uint8).cpu()
    k64 = torch.cat([dequantize(gather(k_after, table[bi], n, ps)[None], kd[bi])[0] for bi, n in enumerate(lens_k)])
    v64 = torch.cat([dequantize(gather(v_after, table[bi], n, ps)[None], vd[bi])[0] for bi, n in enumerate(lens_k)])
    assert not torch.isnan(k64).any() and k64[have[0]:lens_k[0]].abs().sum() > 0      # the append landed in the pages read here
    ref = oracle_varlen(qp.cpu(), k64, v64, torch.zeros_like(qp.cpu()), lens_q, lens_k, True, (-1, -1), d ** -0.5)
    lse = ref[1].float()   # (the public function returns o alone: the oracle's lse stands in)
    check_against_oracle((o, lse) + tuple(ref[2:]), ref, lens_q, lens_k, dtype, "append then prefill")


# ---- the table is untrusted, the pools may be views
@functools.lru_cache(maxsize=None)
def _base(d=128, ps=16, dtype=BF16):
    lens_q, lens_k = [40, 257, 3], [100, 300, 17]
    q, ks, vs = _tokens(lens_q, lens_k, 4, 2, d, dtype, seed=77)
    kp8, vp8, table = _pools8(ks, vs, ps, seed=3, max_blocks=24)
    return lens_q, lens_k, q.to(DEV), kp8, vp8, table


def _call(q, kp, vp, table, cu_q, cu_k, mq, mk, causal=True, **kw):
    return _run(0, q, kp, vp, table, cu_q, cu_k, mq, mk, causal, (-1, -1), **kw)


def _canaries(*pools):
    """the e4m3 pools (whole allocations, as bytes) cut out of larger byte buffers of a sentinel, and a check that neither the pools
    nor their surroundings changed"""
    bufs, views = [], []
    for p in pools:
        n = p.numel()
        buf = torch.full((n + 8192,), 0x55, dtype=torch.uint8, device=DEV)
        view = buf[4096:4096 + n].view(p.shape)
        view.copy_(p)
        bufs.append(buf)
        views.append(view.view(E4M3))
    before = [x.clone() for x in bufs]
    return (*views, lambda: all(torch.equal(x, y) for x, y in zip(bufs, before)))


def test_untrusted_table_with_e4m3_pools():
    import flashattention_lab_cuda as ext

    lens_q, lens_k, q, kp8, vp8, table = _base()
    ps = 16
    kc, vc, unchanged = _canaries(kp8, vp8)
    k16, v16 = _widen(kp8, BF16), _widen(vp8, BF16)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    # a page outside the pool reads as zeros: the packed 16-bit call on the tokens gathered with zero pages
    bad = table.clone()
    bad[1, 2], bad[1, 9] = -1, kp8.shape[0]
    got = _call(q, kc, vc, bad.to(DEV), cu_q, cu_k, 257, 300)
    kz = torch.cat([gather(k16, bad[b], n, ps) for b, n in enumerate(lens_k)]).to(DEV)
    vz = torch.cat([gather(v16, bad[b], n, ps) for b, n in enumerate(lens_k)]).to(DEV)
    assert torch.count_nonzero(kz[100 + 32:100 + 48]) == 0
    _same(got, ext.ex_varlen_forward(q, kz, vz, cu_q, cu_k, 257, 300, True, 128 ** -0.5))
    # entries past the length are never read
    want = _call(q, kc, vc, table.to(DEV), cu_q, cu_k, 257, 300)
    wild = table.clone()
    for b, n in enumerate(lens_k):
        wild[b, (n + 15) // 16:] = 2 ** 31 - 1 - b
    _same(_call(q, kc, vc, wild.to(DEV), cu_q, cu_k, 257, 300), want)
    # lengths are clamped to the table and to max_seqlen_k; negative and decreasing offsets give no keys
    short = table[:, :6].contiguous()
    short[2, 1:] = short[2, 0]
    claim = torch.tensor([0, 5000, 5000 + 2 ** 30, 2 ** 31 - 1], dtype=torch.int32).to(DEV)
    _same(_call(q, kc, vc, short.to(DEV), cu_q, claim, 257, 10 ** 6), _call(q, kc, vc, short.to(DEV), cu_q, _cu([96, 96, 96]).to(DEV), 257, 96))
    _same(_call(q, kc, vc, table.to(DEV), cu_q, cu_k, 257, 50, causal=False),
          _call(q, kc, vc, table.to(DEV), cu_q, _cu([50, 50, 17]).to(DEV), 257, 50, causal=False))
    o, lse = _call(q, kc, vc, table.to(DEV), cu_q, torch.tensor([100, 0, -7, -2 ** 31], dtype=torch.int32).to(DEV), 257, 300)
    assert torch.count_nonzero(o) == 0 and torch.isinf(lse).all()
    assert unchanged()


def test_prefix_sharing_with_e4m3_pools():
    ps, d = 16, 128
    lens_q, lens_k = [40, 130, 7], [100, 180, 64]
    q, ks, vs = _tokens(lens_q, lens_k, 4, 2, d, F16, seed=9)
    for b in (1, 2):   # the first 64 tokens (4 pages) of every sequence are sequence 0's
        ks[b][:64], vs[b][:64] = ks[0][:64], vs[0][:64]
    kp8, vp8, table = _pools8(ks, vs, ps, seed=4)
    own = table.clone()
    table[1, :4] = table[0, :4]
    table[2, :4] = table[0, :4]
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    kd = torch.tensor([[2.0, 0.5], [1.0, 4.0], [0.125, 2.0]]).to(DEV)   # the scale is the sequence's, not the page's
    kc, vc, unchanged = _canaries(kp8, vp8)
    args = (q.to(DEV), kc, vc)
    _same(_call(*args, table.to(DEV), cu_q, cu_k, 130, 180, k_descale=kd), _call(*args, own.to(DEV), cu_q, cu_k, 130, 180, k_descale=kd))
    assert unchanged()


@pytest.mark.parametrize("path", [3, 1], ids=["mfma", "exact"])
def test_strided_e4m3_pools(path):
    lens_q, lens_k, q, kp8, vp8, table = _base(72, 48, F16)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    tab = table.to(DEV)
    kd = torch.tensor([2.0, 0.5]).to(DEV)
    tail = (tab, cu_q, cu_k, 257, 300, True, (-1, -1))
    want = _run(path, q, kp8.to(DEV).view(E4M3), vp8.to(DEV).view(E4M3), *tail, k_descale=kd)
    # K and V as the two halves of one (num_blocks, 2, ps, H_kv, d) allocation; pools sliced in the head dimension: H_kv = 2 of 5
    # heads of 72 bytes, K at byte 72 of a token (8- but not 16-byte aligned)
    wide_k = torch.full((kp8.shape[0], 48, 5, 72), NAN8, dtype=torch.uint8)
    wide_v = torch.full((kp8.shape[0], 48, 5, 72), NAN8, dtype=torch.uint8)
    wide_k[:, :, 1:3], wide_v[:, :, 3:5] = kp8, vp8
    kv, wide_k, wide_v, unchanged = _canaries(torch.stack([kp8, vp8], 1), wide_k, wide_v)
    assert kv[:, 0].stride(0) == 2 * kp8.stride(0) and not kv[:, 0].is_contiguous()
    _same(_run(path, q, kv[:, 0], kv[:, 1], *tail, k_descale=kd), want)
    wk, wv = wide_k[:, :, 1:3], wide_v[:, :, 3:5]
    assert wk.stride(1) == 5 * 72 and wk.data_ptr() % 16 == 8 and wv.data_ptr() % 16 == 8
    _same(_run(path, q, wk, wv, *tail, k_descale=kd), want)
    assert unchanged()


def test_graph_capture_replays_changed_table_offsets_and_scale_values():
    import flashattention_lab_cuda as ext

    lens_q, lens_k, q, kp8, vp8, table = _base()
    kpd, vpd, unchanged = _canaries(kp8, vp8)
    tab = table.to(DEV)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    kd, vd = torch.ones((3, 2), device=DEV), torch.ones((3, 2), device=DEV)

    def call(t, a, b, sk, sv):
        return ext.ex_varlen_forward(q, kpd, vpd, a, b, 257, 300, True, 128 ** -0.5, window=(200, -1), block_table=t, k_descale=sk,
                                     v_descale=sv)
    call(tab, cu_q, cu_k, kd, vd)   # warm-up (modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = call(tab, cu_q, cu_k, kd, vd)
    torch.cuda.current_stream().wait_stream(s)
    seen = []
    for i, (lq, lk, perm) in enumerate((([257, 40, 3], [300, 100, 17], [1, 0, 2]), ([0, 200, 100], [17, 90, 290], [2, 0, 1]),
                                        (lens_q, lens_k, [0, 1, 2]))):
        tab.copy_(table[perm].to(DEV))
        cu_q.copy_(_cu(lq).to(DEV))
        cu_k.copy_(_cu(lk).to(DEV))
        kd.copy_(_fixed_scales(3, 2, i).to(DEV))
        vd.copy_(_fixed_scales(3, 2, i + 2).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = call(tab.clone(), cu_q.clone(), cu_k.clone(), kd.clone(), vd.clone())
        torch.cuda.synchronize()
        _same(out, want, str((lq, lk)))
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[2])
    assert unchanged()
