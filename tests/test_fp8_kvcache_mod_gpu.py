"""GPU: a sliding window, a softcap and attention sinks on fp8 KV-cache decoding (csrc/fa_fp8_decode.hip: fp8kv_split_mod_kernel;
flash_attn_fp8_with_kvcache).

  * the sharp bar on o and lse per 32-row tile over the table of tests/fp8_kvcache_mod_ref.py, against the project's fp64
    reference and that module's baseline; rows without a key give zeros and the sink (-inf without one);
  * nothing below the window's first tile is read: a cache whose bytes there are e4m3 NaN codes gives the clean cache's bits;
  * the bits depend on num_splits and the window alone; default trailing arguments are the parent call; the route counters;
  * a graph replay after cache_seqlens and the sink values changed in place."""
import math

import pytest
import torch

from tests import fp8_kvcache_mod_ref as km
from tests import fp8_kvcache_ref as fk
from tests.test_fp8_mod_cpu import DECODE_IDS, decode_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn


def _fn():
    from common.attention_ex import flash_attn_fp8_with_kvcache
    return flash_attn_fp8_with_kvcache


def _f8(t):
    return t.to(DEV).view(E4)


def _dev(t):
    return None if t is None else t.to(DEV)


def kwargs(call, **over):
    kw = dict(cache_seqlens=_dev(call["cache_seqlens"]), block_table=_dev(call["block_table"]),
              cache_batch_idx=_dev(call["cache_batch_idx"]), q_descale=_dev(call["q_descale"]), k_descale=_dev(call["k_descale"]),
              v_descale=_dev(call["v_descale"]), softmax_scale=call["scale"], causal=call["causal"], num_splits=call["num_splits"],
              out_dtype=call["dtype"], return_softmax_lse=True, window_size=call["window"], softcap=call["softcap"],
              sinks=_dev(call["sinks"]))
    kw.update(over)
    return kw


def run_call(call, **over):
    o, lse = _fn()(_f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"]), **kwargs(call, **over))
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def routes():
    import flashattention_lab_cuda as ext

    return tuple(ext.route_count(n) for n in ("fp8in_fwd_mod", "fp8in_fwd_varlen_mod", "fp8kv_split_mod"))


@pytest.mark.parametrize("i", range(len(km.TABLE)), ids=DECODE_IDS)
def test_sharp_bar(i):
    call, want, base = decode_case(i)
    before = routes()
    o, lse = run_call(call)
    assert routes() == (before[0], before[1], before[2] + 1)
    got = fk.pack(o, lse, call)
    # rows without a key: exact zeros, and the sink (-inf without one or for the head at -inf); everything else finite
    dead = torch.stack([~km.visible(call, k8.shape[0]).any(-1) for k8, _v8 in fk.sequences(call)]).repeat_interleave(call["hkv"], dim=0)
    assert torch.equal(got.lse[dead], want.lse[dead].float()) and bool((got.o[dead] == 0).all())
    assert not bool(torch.isnan(got.lse).any()) and bool(torch.isfinite(got.o.float()).all())
    assert torch.equal(got.lse == -math.inf, want.lse == -math.inf) and torch.equal(got.lse == math.inf, want.lse == math.inf)
    bad, ratio = fk.tile_bar(got, want, base, call["dtype"])
    top = sorted(ratio.items(), key=lambda kv: -kv[1])[:2]
    print(f"RATIO {DECODE_IDS[i]} " + " ".join(f"{k}={v:.3f}" for k, v in top))
    assert not bad, bad
    o2, lse2 = run_call(call)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("i", [1, 2, 6, 10], ids=[DECODE_IDS[i] for i in (1, 2, 6, 10)])
def test_nothing_below_the_windows_first_tile_is_read(i):
    """every cache byte of a sequence below lo, the first 64-key tile a row of the tile sees, becomes an e4m3 NaN code (paged: the
    whole pages below lo, which no other sequence shares).  Every key there is masked for every row, so a kernel that read them
    would still give 0 x NaN = NaN through P V: the result is finite and has the clean cache's bits"""
    call, _want, _base = decode_case(i)
    clean = run_call(call)
    kc_, vc_ = call["k_cache"].clone(), call["v_cache"].clone()
    poisoned = 0
    for b, (k8, _v8) in enumerate(fk.sequences(call)):
        lo = max(0, k8.shape[0] - call["nq"] - call["window"][0]) // 64 * 64
        poisoned += lo
        if call["block_table"] is not None:
            ps = kc_.shape[1]
            for j in range(lo // ps):
                pg = int(call["block_table"][b, j])
                kc_[pg], vc_[pg] = 0x7F, 0x7F
        elif lo:
            row = int(call["cache_batch_idx"][b])
            kc_[row, :lo], vc_[row, :lo] = 0x7F, 0x7F
    assert poisoned >= 64
    dirty = run_call(dict(call, k_cache=kc_, v_cache=vc_))
    assert bool(torch.isfinite(dirty[0].float()).all()) and not bool(torch.isnan(dirty[1]).any())
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[1], clean[1])


def test_the_bits_depend_on_num_splits_and_the_window_alone():
    """a sequence of the batch called alone (another grid, other neighbours, its own row of the table) has the bits it has in the
    batch, at a fixed num_splits and window"""
    call, _want, _base = decode_case(1)                       # nq 3, L 17, causal, S 3, paged
    o, lse = run_call(call)
    for b in (1, 3):
        one = dict(call, B=1, q8=call["q8"][b:b + 1], cache_seqlens=call["cache_seqlens"][b:b + 1], block_table=call["block_table"][b:b + 1],
                   **{n: call[n][b:b + 1] for n in ("q_descale", "k_descale", "v_descale")})
        o1, lse1 = run_call(one)
        assert torch.equal(o1[0], o[b]) and torch.equal(lse1[0], lse[b])


def test_default_trailing_arguments_are_the_parent_call():
    from common.attention_ex import flash_attention_fp8_kvcache

    call, _want, _base = decode_case(1)
    kw = kwargs(call)
    for n in ("window_size", "softcap", "sinks"):
        kw.pop(n)
    before = routes()
    parent = flash_attention_fp8_kvcache(_f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"]), **kw)
    new = _fn()(_f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"]), **kw)
    torch.cuda.synchronize()
    assert routes() == before
    assert torch.equal(new[0], parent[0]) and torch.equal(new[1], parent[1])


def test_graph_replay_with_changed_lengths_and_sinks():
    call, _want, _base = decode_case(6)                       # nq 3, L 128, causal, S 3, paged, sinks
    q, kc_, vc_ = _f8(call["q8"]), _f8(call["k_cache"]), _f8(call["v_cache"])
    kw = kwargs(call)
    _fn()(q, kc_, vc_, **kw)                                  # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = _fn()(q, kc_, vc_, **kw)
    torch.cuda.current_stream().wait_stream(s)
    kw["cache_seqlens"].copy_(torch.tensor([1, 0, 40, 700], dtype=torch.int32))
    kw["sinks"].copy_(torch.tensor([0.5, -1.0, float("-inf"), 3.0, 1.0e4, -2.0, 0.0, -1.0e4]))
    graph.replay()
    torch.cuda.synchronize()
    eager = _fn()(q, kc_, vc_, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    changed = dict(call, cache_seqlens=kw["cache_seqlens"].cpu(), sinks=kw["sinks"].cpu())
    got = fk.pack(out[0].cpu(), out[1].cpu(), changed)
    bad, _ratio = fk.tile_bar(got, km.reference(changed), km.baseline(changed), call["dtype"])
    assert not bad, bad
