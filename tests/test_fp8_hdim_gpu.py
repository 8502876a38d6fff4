"""GPU: the fp8 calls at head dims 64 and 256 (fp8_attn_func, fp8_attn_varlen_func, fp8_attn_with_kvcache in common/fp8_attention.py;
fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim, fa_fp8_forward_kvcache_hdim).

Acceptance is what the d = 128 tests apply to the same quantities, with their helpers unchanged: the sharp bar (kernel error
against the fp64 definition at most twice the error of the float32 baseline with the kernel's rounding points; ex_full_ref.sharp_bar)
per 256-row tile for the prefill calls (fp8_ref.tiled_sharp_bar, as tests/test_fp8_mod_gpu.py) and per 32-row tile for the decode
call (fp8_kvcache_ref.tile_bar, as tests/test_fp8_kvcache_mod_gpu.py); exact zeros and the exact sink / -inf on rows without a
visible key; bit equality of every packed or paged sequence with the padded call on it alone; bit equality at d = 128 with the
_mod functions.  None of those bars is stated per head dim.  The reference and the baseline are tests/fp8_hdim_ref.py's, which
tests/test_fp8_hdim_cpu.py ties to the pinned d = 128 models.

Shapes: the smallest that cross the boundaries of the geometry.  Padded Nq = 260, Nk = 300: two query tiles, three 128-key tiles, an
odd count of 64-key blocks (the zeroed half tile of the transposer), Nq != Nk.  Packed q (1, 70, 189) on k (130, 5, 300): the
middle sequence has causal rows without a visible key.  Paged ps = 16 with a shuffled table and one page outside the pool."""
import functools
import math

import pytest
import torch

from tests import fp8_hdim_ref as hr
from tests import fp8_inputs_ref as fr
from tests import fp8_kvcache_mod_ref as km
from tests import fp8_kvcache_ref as fk
from tests import fp8_mod_ref as fm
from tests.fp8_ref import SENTINEL, tiled_sharp_bar

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
HQ, HKV = 4, 2
NEW_ROUTES = ("fp8in_fwd_hdim", "fp8in_fwd_varlen_hdim", "fp8kv_split_hdim")
OLD_ROUTES = ("fp8in_fwd_mod", "fp8in_fwd_varlen_mod", "fp8kv_split_mod")
MODES = {"bare": dict(causal=False), "causal": dict(causal=True),
         "window-cap-sinks": dict(causal=False, window=(40, 0), softcap=30.0, sinks=True)}
SEQ_Q, SEQ_K = (1, 70, 189), (130, 5, 300)


def _api():
    from common import fp8_attention
    return fp8_attention


def routes(names=NEW_ROUTES + OLD_ROUTES):
    import flashattention_lab_cuda as ext
    return tuple(ext.route_count(n) for n in names)


def dev(t):
    return None if t is None else t.to(DEV)


def mode_call(d, mode, dtype, n, batch, seed):
    m = MODES[mode]
    return hr.make_call(d, n, m["causal"], m.get("window", (-1, -1)), m.get("softcap", 0.0), hr.the_sinks(HQ) if m.get("sinks") else None,
                        dtype, batch=batch, hq=HQ, hkv=HKV, seed=seed)


def call_kwargs(call):
    return dict(q_descale=dev(call["q_descale"]), k_descale=dev(call["k_descale"]), v_descale=dev(call["v_descale"]),
                softmax_scale=call["scale"], causal=call["causal"], out_dtype=call["dtype"], window_size=call["window"],
                softcap=call["softcap"], sinks=dev(call["sinks"]))


def run_padded(call, strided=False):
    """fp8_attn_func on the call as a Result with units (B * H_q, Nq, .) on the CPU.  strided: layout "bnhd" views, k and v the
    [:, :Nk] prefix of a larger cache whose other bytes are e4m3 NaN codes"""
    d, nq, nk = call["d"], call["nq"], call["nk"]
    if strided:
        q = call["q8"].transpose(1, 2).contiguous().view(E4).to(DEV)                       # (B, Nq, H_q, d)
        kbuf, vbuf = (torch.full((call["B"], nk + 37, HKV, d), SENTINEL, dtype=torch.uint8) for _ in range(2))
        kbuf[:, :nk], vbuf[:, :nk] = call["k8"].transpose(1, 2), call["v8"].transpose(1, 2)
        k, v = kbuf.view(E4).to(DEV)[:, :nk], vbuf.view(E4).to(DEV)[:, :nk]
        assert not k.is_contiguous()
        o, lse = _api().fp8_attn_func(q, k, v, layout="bnhd", return_lse=True, **call_kwargs(call))
        o = o.transpose(1, 2)
    else:
        q, k, v = (call[n].view(E4).to(DEV) for n in ("q8", "k8", "v8"))
        o, lse = _api().fp8_attn_func(q, k, v, layout="bhnd", return_lse=True, **call_kwargs(call))
    torch.cuda.synchronize()
    assert o.dtype == call["dtype"] and lse.dtype == torch.float32 and o.shape[-1] == d
    return fr._result(o.reshape(-1, nq, d).cpu(), lse.reshape(-1, nq).cpu())


def check_dead_rows(got, call, dead):
    """rows without a visible key: exact zeros and the exact sink (-inf without one); everything finite elsewhere"""
    assert not bool(torch.isnan(got.lse).any()) and bool(torch.isfinite(got.o.float()).all())
    assert bool((got.o[dead] == 0).all())
    if call["sinks"] is not None:
        want = call["sinks"].repeat(call["B"])[:, None].expand_as(got.lse)
        assert torch.equal(got.lse[dead], want[dead])
    else:
        assert torch.equal(got.lse == float("-inf"), dead)


@functools.lru_cache(maxsize=None)
def padded_case(d, mode, dt):
    call = mode_call(d, mode, DTYPES[dt], (260, 300), 2, seed=d)
    return call, hr.reference(call), hr.baseline(call)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", [64, 256])
def test_padded_meets_the_sharp_bar(d, mode, dt):
    call, ref, base = padded_case(d, mode, dt)
    before = routes()
    got = run_padded(call, strided=True)
    assert routes() == (before[0] + 1,) + before[1:]          # the new route once, the d = 128 routes not at all
    check_dead_rows(got, call, ~fm.band(call).any(-1)[None, :].expand_as(ref.lse))
    bad, ratio = tiled_sharp_bar(got, ref, base, call["dtype"])
    print(f"RATIO padded d={d} {mode} {dt} " + " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
    assert not bad, bad
    plain = run_padded(call, strided=False)                   # the contiguous "bhnd" tensors: the same bits
    assert torch.equal(got.o, plain.o) and torch.equal(got.lse, plain.lse)
    if call["sinks"] is not None:                             # the head whose sink is -inf has the bits of the call without sinks
        bare = run_padded(dict(call, sinks=None))
        u = torch.arange(call["B"]) * HQ + 1
        assert torch.equal(got.o[u], bare.o[u]) and torch.equal(got.lse[u], bare.lse[u])


# ---- packed and paged: three sequences cut from one padded set of tensors

@functools.lru_cache(maxsize=None)
def varlen_case(d, mode, dt, zero_page):
    """(the B = 3 pool of tensors, per sequence the padded call on it alone, reference and baseline as (o (total_q, H_q, d),
    lse (H_q, total_q))); zero_page: ps, whose third page of the last sequence reads as zero bytes (a page outside the pool)"""
    pool = mode_call(d, mode, DTYPES[dt], (max(SEQ_Q), max(SEQ_K)), 3, seed=1000 + d)
    calls = [hr.sequence_call(pool, b, nq, nk, (2 * zero_page, 3 * zero_page) if zero_page and b == 2 else None)
             for b, (nq, nk) in enumerate(zip(SEQ_Q, SEQ_K))]
    out = []
    for fn in (hr.reference, hr.baseline):
        rs = [fn(c) for c in calls]
        out.append((torch.cat([r.o.double().transpose(0, 1) for r in rs]), torch.cat([r.lse.double() for r in rs], dim=1)))
    return pool, calls, out[0], out[1]


def run_varlen(pool, calls, ps):
    d = pool["d"]
    cu = lambda lens: torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32).to(DEV)   # noqa: E731
    q = torch.cat([c["q8"][0].transpose(0, 1) for c in calls])                             # (total_q, H_q, d)
    buf = torch.zeros((q.shape[0], 3, HQ, d), dtype=torch.uint8)                           # a slice of a fused projection
    buf[:, 1] = q
    q = buf.view(E4).to(DEV)[:, 1]
    assert not q.is_contiguous()
    kw = call_kwargs(pool)
    if ps == 0:
        k, v = (torch.cat([pool[n][b, :, :nk].transpose(0, 1) for b, nk in enumerate(SEQ_K)]).contiguous().view(E4).to(DEV) for n in ("k8", "v8"))
    else:
        need = [(n + ps - 1) // ps for n in SEQ_K]
        nblk, mblk = sum(need) + 2, max(need) + 1
        g = torch.Generator().manual_seed(3)
        perm = torch.randperm(nblk, generator=g).tolist()
        table = torch.randint(-3, nblk + 3, (3, mblk), generator=g, dtype=torch.int32)
        kp, vp = (torch.full((nblk, ps, HKV, d), SENTINEL, dtype=torch.uint8) for _ in range(2))
        for b, n in enumerate(SEQ_K):
            for j in range(need[b]):
                pg = perm.pop()
                table[b, j] = pg
                m = min(ps, n - j * ps)
                kp[pg, :m] = pool["k8"][b, :, j * ps:j * ps + m].transpose(0, 1)
                vp[pg, :m] = pool["v8"][b, :, j * ps:j * ps + m].transpose(0, 1)
        table[2, 2] = nblk + 7                                                             # a page outside the pool
        k, v, kw["block_table"] = kp.view(E4).to(DEV), vp.view(E4).to(DEV), table.to(DEV)
    o, lse = _api().fp8_attn_varlen_func(q, k, v, cu(SEQ_Q), cu(SEQ_K), max(SEQ_Q), max(SEQ_K), return_softmax_lse=True, **kw)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("form", ["packed", "ps16"])
@pytest.mark.parametrize("d", [64, 256])
def test_packed_and_paged_meet_the_sharp_bar_and_the_padded_bits(d, form, mode, dt):
    ps = 16 if form == "ps16" else 0
    pool, calls, ref, base = varlen_case(d, mode, dt, ps)
    before = routes()
    o, lse = run_varlen(pool, calls, ps)
    assert routes() == (before[0], before[1] + 1) + before[2:]
    assert not bool(torch.isnan(lse).any()) and bool(torch.isfinite(o.float()).all())
    a = 0
    for c in calls:                                           # every sequence: the bits of the padded call on it alone
        one = run_padded(c)
        z = a + c["nq"]
        assert torch.equal(o[a:z].transpose(0, 1), one.o) and torch.equal(lse[:, a:z], one.lse), (form, a)
        check_dead_rows(one, c, ~fm.band(c).any(-1)[None, :].expand_as(one.lse))
        a = z
    if mode != "bare":                                        # the middle sequence: 65 rows above the diagonal of its 5 keys
        assert int((~fm.band(calls[1]).any(-1)).sum()) == 65
    got, want, model = (fr._result(x.transpose(0, 1), y) for x, y in ((o, lse), ref, base))
    bad, ratio = tiled_sharp_bar(got, want, model, pool["dtype"])
    print(f"RATIO {form} d={d} {mode} {dt} " + " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
    assert not bad, bad


# ---- decode
# heads, Nq, layout, lengths (the last sequence of a "bidx" call loses its cache row: an index out of range), num_splits, featured
LENS = {"a": (63, 192, 64), "b": (0, 63, 192), "c": (192, 0, 64), "d": (64, 192, 63)}
DECODE = (
    dict(heads=(8, 2), nq=1, layout="bidx", lens="a", splits=1, feat=False, dt="bf16"),
    dict(heads=(8, 2), nq=3, layout="ps16", lens="b", splits=3, feat=True, dt="bf16"),
    dict(heads=(4, 4), nq=3, layout="bidx", lens="c", splits=0, feat=True, dt="f16"),
    dict(heads=(4, 4), nq=1, layout="ps16", lens="d", splits=0, feat=False, dt="f16"),
    dict(heads=(8, 2), nq=3, layout="ps16", lens="c", splits=1, feat=True, dt="f16"),      # sinks raise one split to two
    dict(heads=(4, 4), nq=1, layout="bidx", lens="b", splits=3, feat=False, dt="bf16"),
    dict(heads=(8, 2), nq=3, layout="bidx", lens="d", splits=3, feat=False, dt="bf16"),    # bare, causal over three tokens
)
DECODE_IDS = [f"h{c['heads'][0]}-{c['heads'][1]}-nq{c['nq']}-{c['layout']}-{c['lens']}-S{c['splits']}-{'feat' if c['feat'] else 'bare'}" for c in DECODE]


@functools.lru_cache(maxsize=None)
def decode_case(d, i):
    c = DECODE[i]
    call = hr.decode_call(d, c["heads"], c["nq"], LENS[c["lens"]], c["layout"], c["splits"], (128, -1) if c["feat"] else (-1, -1),
                          c["feat"], causal=True, dtype=DTYPES[c["dt"]], seed=10 * i + d)
    return call, hr.decode_reference(call), hr.decode_baseline(call)


def decode_kwargs(call):
    return dict(cache_seqlens=dev(call["cache_seqlens"]), block_table=dev(call["block_table"]), cache_batch_idx=dev(call["cache_batch_idx"]),
                q_descale=dev(call["q_descale"]), k_descale=dev(call["k_descale"]), v_descale=dev(call["v_descale"]),
                softmax_scale=call["scale"], causal=call["causal"], num_splits=call["num_splits"], out_dtype=call["dtype"],
                return_softmax_lse=True, window_size=call["window"], softcap=call["softcap"], sinks=dev(call["sinks"]))


def run_decode(call):
    q, kc_, vc_ = (call[n].to(DEV).view(E4) for n in ("q8", "k_cache", "v_cache"))
    o, lse = _api().fp8_attn_with_kvcache(q, kc_, vc_, **decode_kwargs(call))
    torch.cuda.synchronize()
    assert o.shape == (call["B"], call["nq"], call["hq"], call["d"]) and o.dtype == call["dtype"]
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("i", range(len(DECODE)), ids=DECODE_IDS)
@pytest.mark.parametrize("d", [64, 256])
def test_decode_meets_the_sharp_bar(d, i):
    call, want, base = decode_case(d, i)
    before = routes()
    o, lse = run_decode(call)
    assert routes() == before[:2] + (before[2] + 1,) + before[3:]
    got = hr.pack(o, lse, call)
    dead = torch.stack([~km.visible(call, k8.shape[0]).any(-1) for k8, _v8 in fk.sequences(call)]).repeat_interleave(call["hkv"], dim=0)
    assert torch.equal(got.lse[dead], want.lse[dead].float()) and bool((got.o[dead] == 0).all())
    assert not bool(torch.isnan(got.lse).any()) and bool(torch.isfinite(got.o.float()).all())
    assert torch.equal(got.lse == -math.inf, want.lse == -math.inf) and torch.equal(got.lse == math.inf, want.lse == math.inf)
    bad, ratio = fk.tile_bar(got, want, base, call["dtype"])
    top = sorted(ratio.items(), key=lambda kv: -kv[1])[:2]
    print(f"RATIO decode d={d} {DECODE_IDS[i]} " + " ".join(f"{k}={v:.3f}" for k, v in top))
    assert not bad, bad
    o2, lse2 = run_decode(call)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


# ---- d = 128 through the new functions is the _mod call

def test_head_dim_128_is_the_mod_call_bit_for_bit():
    from common.attention_ex import flash_attn_fp8_func, flash_attn_fp8_varlen_func, flash_attn_fp8_with_kvcache

    before = routes()
    # padded, featured
    call = fm.build_call(0, softcap=True, sinks=True)
    q, k, v = (call[n].view(E4).to(DEV) for n in ("q8", "k8", "v8"))
    kw = dict(call_kwargs(call), return_lse=True)
    new, old = _api().fp8_attn_func(q, k, v, **kw), flash_attn_fp8_func(q, k, v, **kw)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    # packed, bare: the parent's lean kernels, no featured route at all
    vc = fm.varlen_case(True, (-1, -1), False, False)
    args = tuple(vc[n].view(E4).to(DEV) for n in ("q8", "k8", "v8")) + (vc["cu_q"].to(DEV), vc["cu_k"].to(DEV), max(fm.SEQ_Q), max(fm.SEQ_K))
    kw = dict(q_descale=dev(vc["q_descale"]), k_descale=dev(vc["k_descale"]), v_descale=dev(vc["v_descale"]), causal=True, return_softmax_lse=True)
    new, old = _api().fp8_attn_varlen_func(*args, **kw), flash_attn_fp8_varlen_func(*args, **kw)
    tq = int(vc["cu_q"][-1])
    assert torch.equal(new[0][:tq], old[0][:tq]) and torch.equal(new[1][:, :tq], old[1][:, :tq])
    # decode, featured
    dc = km.build_call(6)
    dq, dk, dv = (dc[n].to(DEV).view(E4) for n in ("q8", "k_cache", "v_cache"))
    kw = decode_kwargs(dc)
    new, old = _api().fp8_attn_with_kvcache(dq, dk, dv, **kw), flash_attn_fp8_with_kvcache(dq, dk, dv, **kw)
    torch.cuda.synchronize()
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    after = routes()
    assert after[:3] == before[:3]                            # none of the new routes
    assert after[3:] == (before[3] + 2, before[4], before[5] + 2)   # the parent's: featured padded and decode twice each, bare packed none


# ---- end to end: quantise, append, decode at d = 64

def test_quantise_append_decode_at_head_dim_64():
    from common.attention_ex import flash_attn_with_kvcache, quantize_fp8_qkv

    d, nb, hq, hkv, cap, nnew = 64, 2, 8, 2, 96, 70
    g = torch.Generator().manual_seed(64)
    q16 = torch.randn((nb, 1, hq, d), generator=g).to(torch.bfloat16).to(DEV)
    k16, v16 = (torch.randn((nb, nnew, hkv, d), generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    q8, _k8, _v8, qd, kd, vd = quantize_fp8_qkv(q16, k16, v16, layout="bnhd")
    kc_, vc_ = (torch.full((nb, cap, hkv, d), SENTINEL, dtype=torch.uint8, device=DEV).view(E4) for _ in range(2))
    lens = torch.zeros(nb, dtype=torch.int32, device=DEV)
    flash_attn_with_kvcache(q16, kc_, vc_, k16, v16, cache_seqlens=lens, k_descale=kd, v_descale=vd)      # the append
    assert torch.equal(kc_.view(torch.uint8)[:, :nnew], _k8.view(torch.uint8))
    lens = torch.full((nb,), nnew, dtype=torch.int32, device=DEV)
    o, lse = _api().fp8_attn_with_kvcache(q8, kc_, vc_, cache_seqlens=lens, q_descale=qd, k_descale=kd, v_descale=vd, causal=True,
                                          num_splits=2, return_softmax_lse=True)
    torch.cuda.synchronize()
    call = dict(B=nb, hq=hq, hkv=hkv, nq=1, d=d, causal=True, dtype=torch.bfloat16, scale=d ** -0.5, num_splits=2,
                q8=q8.view(torch.uint8).cpu(), k_cache=kc_.view(torch.uint8).cpu(), v_cache=vc_.view(torch.uint8).cpu(),
                cache_seqlens=lens.cpu(), block_table=None, cache_batch_idx=None, q_descale=qd.cpu(), k_descale=kd.cpu(), v_descale=vd.cpu(),
                window=(-1, -1), softcap=0.0, sinks=None)
    bad, _ratio = fk.tile_bar(hr.pack(o.cpu(), lse.cpu(), call), hr.decode_reference(call), hr.decode_baseline(call), torch.bfloat16)
    assert not bad, bad


# ---- graph capture: one decode call at d = 64, replayed after the lengths and the descales changed in place

def test_graph_replay_at_head_dim_64():
    call, _want, _base = decode_case(64, 1)                   # nq 3, paged, three splits, window and sinks
    q, kc_, vc_ = (call[n].to(DEV).view(E4) for n in ("q8", "k_cache", "v_cache"))
    kw = decode_kwargs(call)
    fn = _api().fp8_attn_with_kvcache
    fn(q, kc_, vc_, **kw)                                     # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = fn(q, kc_, vc_, **kw)
    torch.cuda.current_stream().wait_stream(s)
    kw["cache_seqlens"].copy_(torch.tensor([40, 1, 700], dtype=torch.int32))
    for n in ("q_descale", "k_descale", "v_descale"):
        kw[n].mul_(1.75)
    graph.replay()
    torch.cuda.synchronize()
    eager = fn(q, kc_, vc_, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    changed = dict(call, cache_seqlens=kw["cache_seqlens"].cpu(), **{n: kw[n].cpu() for n in ("q_descale", "k_descale", "v_descale")})
    bad, _ratio = fk.tile_bar(hr.pack(out[0].cpu(), out[1].cpu(), changed), hr.decode_reference(changed), hr.decode_baseline(changed),
                              call["dtype"])
    assert not bad, bad
