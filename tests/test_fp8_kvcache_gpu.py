"""GPU: fp8 KV-cache decoding (csrc/fa_fp8_decode.hip: fp8kv_split_kernel) through flash_attention_fp8_kvcache.

  * the sharp bar of §9l-2 on o and lse per 32-row tile over the table of tests/fp8_kvcache_cases.py, against the fp64 reference and
    the baseline of tests/fp8_kvcache_ref.py; the exact zeros / -inf of rows without a key; dtype_tolerances as the project bar;
  * the V path exactly: a one-hot probability hands every (key, column) code of V through the on-chip transposition bit for bit;
  * bit identities at a fixed num_splits; untrusted lengths, table entries and dead cache bytes; graph replay.
The largest kernel / baseline ratios are printed per case (profiles/fp8_kvcache.md records a run)."""
import math

import pytest
import torch

from tests import fp8_kvcache_cases as cases
from tests import fp8_kvcache_ref as ref
from tests.fp8_ref import e4m3_value
from tests.helpers import dtype_tolerances

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn


def _fn():
    from common.attention_ex import flash_attention_fp8_kvcache
    return flash_attention_fp8_kvcache


def _f8(t):
    return t.to(DEV).view(E4)


def _dev(t):
    return None if t is None else t.to(DEV)


def run_call(call, **over):
    kw = dict(cache_seqlens=_dev(call["cache_seqlens"]), block_table=_dev(call["block_table"]),
              cache_batch_idx=_dev(call["cache_batch_idx"]), q_descale=_dev(call["q_descale"]), k_descale=_dev(call["k_descale"]),
              v_descale=_dev(call["v_descale"]), softmax_scale=call["scale"], causal=call["causal"], num_splits=call["num_splits"],
              out_dtype=call["dtype"], return_softmax_lse=True)
    kw.update(over)
    o, lse = _fn()(_f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"]), **kw)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("i", range(len(cases.CASES)), ids=[cases.case_id(c, i) for i, c in enumerate(cases.CASES)])
def test_sharp_bar(i):
    call = cases.build_call(cases.CASES[i], i)
    o, lse = run_call(call)
    got = ref.pack(o, lse, call)
    want = ref.reference(call)
    base = ref.rounded(ref.baseline(call), call["dtype"])
    # rows without a key: exact zeros and -inf; everything else finite
    dead = want.lse == -math.inf
    assert torch.equal(got.lse == -math.inf, dead)
    assert bool((got.o[dead] == 0).all())
    assert bool(torch.isfinite(got.o).all()) and bool(torch.isfinite(got.lse[~dead]).all())
    bad, ratio = ref.tile_bar(got, want, base, call["dtype"])
    top = sorted(ratio.items(), key=lambda kv: -kv[1])[:2]
    print(f"RATIO {cases.case_id(cases.CASES[i], i)} " + " ".join(f"{k}={v:.3f}" for k, v in top))
    assert not bad, bad
    tol = dtype_tolerances(call["dtype"])
    torch.testing.assert_close(got.o.double(), want.o, **tol)
    torch.testing.assert_close(got.lse[~dead].double(), want.lse[~dead], rtol=1e-3, atol=1e-3)


# ---- the V path, exactly

def _codes_distinct(nkeys):
    """(nkeys, 128) uint8: a distinct non-NaN e4m3 code per (key, column) as far as 254 codes go: no two neighbours in a row or a
    column alike, and every 4 x 4 block of (key, column) holds 16 different codes"""
    j, c = torch.arange(nkeys)[:, None], torch.arange(128)[None, :]
    x = (j * 37 + c * 5 + (j // 4) * 3) % 254                       # 0 .. 253
    code = torch.where(x >= 127, x + 1, x)                          # skip 0x7F; 0xFF is not reached
    return code.to(torch.uint8)


@pytest.mark.parametrize("paged", (False, True), ids=("contig", "ps16"))
@pytest.mark.parametrize("splits", (1, 3))
def test_one_hot_v_path(splits, paged):
    """q = 448 e_0, k[j*] = 448 e_0, every other key zero, unit descales: the raw score of j* is 448^2 and every other one 0, so every
    other probability is exp2 of about -25000, exactly 0, and o is the widened row v[j*] bit for bit.  softmax_scale is the float32
    x near 0.125 / log2(e) for which the kernel's factor f = x * 1.4426950408889634f is exactly 0.125: then 448^2 * f = 25088 is
    exact, the exp2's fma leaves 0 and p = 1 to the last bit (with 128 ** -0.5 the product rounds, p = 1.0006, and the f16 o is one
    ulp off v: arithmetic, not the V path).  One sequence per j* over every position of two key tiles (128 sequences, one call)."""
    import numpy as np
    log2e = np.float32(1.4426950408889634)
    x = np.float32(0.125 / 1.4426950408889634)
    cands = [x]
    for _ in range(4):
        cands = [np.nextafter(cands[0], np.float32(0)), *cands, np.nextafter(cands[-1], np.float32(1))]
    scale = float(next(c for c in cands if np.float32(c * log2e) == np.float32(0.125)))
    n = 128
    B, hkv = n, 1
    q8 = torch.zeros((B, 1, 1, 128), dtype=torch.uint8)
    q8[..., 0] = 0x7E                                              # 448
    kc = torch.zeros((B, n, hkv, 128), dtype=torch.uint8)
    kc[torch.arange(B), torch.arange(B), 0, 0] = 0x7E
    v = _codes_distinct(n)
    vc = v[None, :, None, :].expand(B, n, hkv, 128).contiguous()
    table = None
    if paged:
        ps, nb = 16, n // 16
        perm = torch.randperm(B * nb, generator=torch.Generator().manual_seed(5))
        table = perm.reshape(B, nb).to(torch.int32)
        pk, pv = torch.zeros((B * nb, ps, hkv, 128), dtype=torch.uint8), torch.zeros((B * nb, ps, hkv, 128), dtype=torch.uint8)
        pk[table.reshape(-1).long()] = kc.reshape(B * nb, ps, hkv, 128)
        pv[table.reshape(-1).long()] = vc.reshape(B * nb, ps, hkv, 128)
        kc, vc = pk, pv
    for dt in (torch.bfloat16, torch.float16):
        o, lse = _fn()(_f8(q8), _f8(kc), _f8(vc), block_table=_dev(table), softmax_scale=scale, num_splits=splits, out_dtype=dt,
                       return_softmax_lse=True)
        want = e4m3_value(v).to(dt)                                # (key j*, 128): exact in both dtypes
        assert torch.equal(o.cpu()[:, 0, 0], want), (o.cpu()[:, 0, 0].float() - want.float()).abs().max()
        assert torch.allclose(lse.cpu(), torch.full((B, 1, 1), 25088.0 * math.log(2.0)), rtol=1e-6)


# ---- bit identities at a fixed num_splits

def _case(**kw):
    c = dict(dtype="bf16", heads=(8, 2), nq=2, lens="e", mask="causal", layout="ps16", splits=2, descales="bhkv", values="normal")
    c.update(kw)
    return c


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _gathered(call):
    """the contiguous call on the tokens the call's sequences own"""
    seqs = ref.sequences(call)
    cap = max(k.shape[0] for k, _ in seqs) + 3
    kc = torch.full((call["B"], cap, call["hkv"], 128), cases.SENTINEL, dtype=torch.uint8)
    vc = kc.clone()
    for b, (k, v) in enumerate(seqs):
        kc[b, :k.shape[0]], vc[b, :k.shape[0]] = k, v
    lens = torch.tensor([k.shape[0] for k, _ in seqs], dtype=torch.int32)
    return dict(call, k_cache=kc, v_cache=vc, block_table=None, cache_batch_idx=None, cache_seqlens=lens)


@pytest.mark.parametrize("splits", (1, 2))
def test_bit_identities(splits):
    call = cases.build_call(_case(splits=splits), 100)
    a = run_call(call)
    _same(a, run_call(call))                                       # two runs
    _same(a, run_call(_gathered(call)))                            # paged = contiguous on the gathered tokens
    # permuted pages: the pool reversed, the table following it
    nb = call["k_cache"].shape[0]
    rev = dict(call, k_cache=call["k_cache"].flip(0).contiguous(), v_cache=call["v_cache"].flip(0).contiguous(),
               block_table=(nb - 1 - call["block_table"]).to(torch.int32))
    _same(a, run_call(rev))
    # shared pages: sequence 1 (64 keys) reads the first pages of sequence 0
    sh = dict(call, block_table=call["block_table"].clone())
    sh["block_table"][1, :4] = call["block_table"][0, :4]
    shc = _gathered(sh)
    _same(run_call(sh), run_call(shc))
    # each batch element alone = its slice
    for b in range(call["B"]):
        one = dict(call, B=1, q8=call["q8"][b:b + 1], cache_seqlens=call["cache_seqlens"][b:b + 1], block_table=call["block_table"][b:b + 1],
                   **{n: call[n][b:b + 1] for n in ("q_descale", "k_descale", "v_descale")})
        ob, lb = run_call(one)
        assert torch.equal(ob[0], a[0][b]) and torch.equal(lb[0], a[1][b])
    # a strided q view = its contiguous copy
    wide = torch.zeros((call["B"], call["nq"] * 2, call["hq"] * 2, 128), dtype=torch.uint8)
    wide[:, ::2, :call["hq"]] = call["q8"]
    qv = wide.to(DEV).view(E4)[:, ::2, :call["hq"]]
    assert not qv.is_contiguous()
    kw = dict(cache_seqlens=_dev(call["cache_seqlens"]), block_table=_dev(call["block_table"]), q_descale=_dev(call["q_descale"]),
              k_descale=_dev(call["k_descale"]), v_descale=_dev(call["v_descale"]), causal=True, num_splits=splits, return_softmax_lse=True)
    o, lse = _fn()(qv, _f8(call["k_cache"]), _f8(call["v_cache"]), **kw)
    _same(a, (o.cpu(), lse.cpu()))


@pytest.mark.parametrize("splits", (1, 2))
def test_cache_batch_idx_is_the_gathered_cache(splits):
    call = cases.build_call(_case(layout="bidx", splits=splits), 101)
    _same(run_call(call), run_call(_gathered(call)))


def test_gqa_is_the_call_with_heads_repeated():
    call = cases.build_call(_case(mask="none", layout="contig", heads=(8, 2), nq=2), 102)
    a = run_call(call)
    g = call["hq"] // call["hkv"]
    rep = dict(call, hkv=call["hq"], k_cache=call["k_cache"].repeat_interleave(g, 2), v_cache=call["v_cache"].repeat_interleave(g, 2),
               **{n: call[n].repeat_interleave(g, 1) for n in ("q_descale", "k_descale", "v_descale")})
    _same(a, run_call(rep))


def test_power_of_two_descales_fold_into_the_scale():
    call = cases.build_call(_case(descales="none", layout="contig"), 103)
    a_, b_, c_ = 3, -2, 4
    ones = torch.ones((call["B"], call["hkv"]))
    o1, l1 = run_call(dict(call, q_descale=ones * 2.0 ** a_, k_descale=ones * 2.0 ** b_, v_descale=ones * 2.0 ** c_))
    o2, l2 = run_call(dict(call, scale=call["scale"] * 2.0 ** (a_ + b_)))
    assert torch.equal(o1, (o2.float() * 2.0 ** c_).to(o2.dtype)) and torch.equal(l1, l2)


# ---- untrusted inputs

def test_untrusted_lengths_table_and_dead_bytes():
    c = _case(layout="ps16", lens="e", splits=2)
    call = cases.build_call(c, 104)                                # dead pool bytes are 0x7F already; the table's tail is garbage
    want = run_call(_gathered(call))
    bt = call["block_table"].clone()
    nb, ps = call["k_cache"].shape[0], 16
    for b, n in enumerate(cases.LENS["e"]):
        bt[b, (n + ps - 1) // ps:] = torch.tensor([-1, nb, 2 ** 30] * 8, dtype=torch.int32)[:bt.shape[1] - (n + ps - 1) // ps]
    _same(want, run_call(dict(call, block_table=bt)))
    # lengths -5 and capacity + 7: empty, and clamped to the capacity
    full = cases.build_call(_case(layout="contig", lens="e", splits=2), 105)
    cap = full["k_cache"].shape[1]
    full["k_cache"][:, :] = cases.build_call(_case(layout="contig", lens="e", splits=2), 105)["k_cache"][0:1, :1]   # finite everywhere
    full["v_cache"][:, :] = full["k_cache"]
    over = run_call(dict(full, cache_seqlens=torch.tensor([-5, cap + 7, cap], dtype=torch.int32)))
    exact = run_call(dict(full, cache_seqlens=torch.tensor([0, cap, cap], dtype=torch.int32)))
    _same(over, exact)
    assert bool((over[0][0] == 0).all()) and bool((over[1][0] == -math.inf).all())
    # a page outside the pool inside the live range: zero K and V with score 0 — the gathered cache holds zeros there
    hole = dict(call, block_table=call["block_table"].clone())
    hole["block_table"][0, 1] = nb
    _same(run_call(hole), run_call(_gathered(hole)))


def test_outputs_cut_out_of_sentinel_buffers():
    """the C call with o, lse and the workspace inside sentinel buffers: the call's own bytes are the wrapper's result, and the
    surroundings (512 elements on either side, and the workspace past the bytes the size query names) stay intact"""
    import flashattention_lab_cuda as ext

    call = cases.build_call(_case(splits=2), 106)
    B, nq, hq, hkv = call["B"], call["nq"], call["hq"], call["hkv"]
    q, kc, vc = _f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"])
    lens, bt = _dev(call["cache_seqlens"]), _dev(call["block_table"])
    qd, kd, vd = (_dev(call[n]).contiguous() for n in ("q_descale", "k_descale", "v_descale"))
    want_o, want_lse = run_call(call)
    pad, no, nl = 512, B * nq * hq * 128, B * hq * nq
    obuf = torch.full((pad + no + pad,), -768.0, dtype=call["dtype"], device=DEV)
    lbuf = torch.full((pad + nl + pad,), 12345.0, dtype=torch.float32, device=DEV)
    cap = bt.shape[1] * kc.shape[1]
    need = int(ext._lib.fa_fp8_forward_kvcache_workspace_bytes(B, hq, hkv, nq, cap, 128, 2))
    assert need > 0
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    ext._call("fa_fp8_forward_kvcache", (
        q.data_ptr(), kc.data_ptr(), vc.data_ptr(), obuf[pad:].data_ptr(), lbuf[pad:].data_ptr(), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(),
        lens.data_ptr(), bt.data_ptr(), 0, B, hq, hkv, nq, cap, 0, 128, ext._DTYPE_CODE[call["dtype"]], 3, 3, q.stride(0), q.stride(1),
        kc.stride(0), kc.stride(1), vc.stride(0), vc.stride(1), bt.stride(0), kc.shape[0], kc.shape[1], hkv, hkv, hkv, 1, call["scale"], 2,
        ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(obuf[pad:pad + no].cpu().reshape(want_o.shape), want_o)
    assert torch.equal(lbuf[pad:pad + nl].cpu().reshape(want_lse.shape), want_lse)
    for buf, n, fill in ((obuf, no, -768.0), (lbuf, nl, 12345.0)):
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all())
    assert bool((ws[need:] == 0x5A).all())


# ---- graph

def test_graph_replays_after_inputs_change_in_place():
    call = cases.build_call(_case(splits=2), 107)
    q, kc, vc = _f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"])
    lens, bt = _dev(call["cache_seqlens"]), _dev(call["block_table"])
    ds = [_dev(call[n]).clone() for n in ("q_descale", "k_descale", "v_descale")]
    kw = dict(cache_seqlens=lens, block_table=bt, q_descale=ds[0], k_descale=ds[1], v_descale=ds[2], causal=True, num_splits=2,
              return_softmax_lse=True)
    fn = _fn()
    fn(q, kc, vc, **kw)                                            # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = fn(q, kc, vc, **kw)
    lens.copy_(torch.tensor([200, 17, 0], dtype=torch.int32))
    bt[1, 0] = bt[0, 2]
    for d in ds:
        d.mul_(1.37)
    graph.replay()
    torch.cuda.synchronize()
    o2, lse2 = fn(q, kc, vc, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
