"""GPU: the fp8 decode step (csrc/fa_fp8_step.hip: fp8kv_step_prep_kernel; flash_attn_fp8_kvcache_step) over the
table of tests/fp8_step_ref.py.  Every case runs the step once, on caches of its own, and is held to:

  * the cache bytes of flash_attn_with_kvcache(q16, ..., k=, v=, rotary, k_descale=, v_descale=) on a copy: the parent's append is
    the yardstick (contiguous, cache_batch_idx with an index out of range, paged, a table entry outside the pool, strided pools);
  * q8_out = the model's codes in every byte; no cache byte but the appended slots changes (the model's caches, byte for byte);
  * o, lse = flash_attn_fp8_with_kvcache(q8_out, caches after, cache_seqlens = len_eff, ...) bit for bit;
  * o, lse under fp8_kvcache_ref.tile_bar against the fp64 reference and the baseline on the GPU's own q8 and caches;
and beside the table: e4m3 mode, a graph replay after everything a replay may change changed in place, the route counters."""
import pytest
import torch

from tests import fp8_kvcache_mod_ref as fm
from tests import fp8_kvcache_ref as fk
from tests import fp8_step_ref as ref
from tests.kvcache_fp8_ref import quantize
from tests.test_fp8_step_cpu import IDS, _built

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
CASES = range(len(ref.TABLE))


def _dev(t):
    return None if t is None else t.to(DEV)


def caches(call):
    """(k_cache, v_cache, the allocation they live in) as uint8 device tensors; strided: the K and V pools are the two halves of
    one (num_blocks, ps, 2, H_kv, 128) allocation, so a token of one lies between two tokens of the other"""
    kc, vc = call["k_cache"], call["v_cache"]
    if call["layout"] == "strided":
        both = torch.stack([kc, vc], dim=2).to(DEV)
        return both[:, :, 0], both[:, :, 1], both
    both = torch.stack([kc, vc]).to(DEV)
    return both[0], both[1], both


def common_kw(call):
    return dict(block_table=_dev(call["block_table"]), cache_batch_idx=_dev(call["cache_batch_idx"]), k_descale=_dev(call["k_descale"]),
                v_descale=_dev(call["v_descale"]), softmax_scale=call["scale"], causal=call["causal"], window_size=call["window"],
                softcap=call["softcap"], sinks=_dev(call["sinks"]), num_splits=call["num_splits"], return_softmax_lse=True)


def run_step(call, kc, vc, **over):
    from common.attention_ex import flash_attn_fp8_kvcache_step

    kw = dict(common_kw(call), cache_seqlens=_dev(call["cache_seqlens"]), q_descale=_dev(call["q_descale"]),
              rotary_cos=_dev(call["rotary_cos"]), rotary_sin=_dev(call["rotary_sin"]), rotary_interleaved=call["rotary_interleaved"])
    kw.update(over)
    return flash_attn_fp8_kvcache_step(_dev(call["q"]), kc.view(E4), vc.view(E4), _dev(call["k_new"]), _dev(call["v_new"]), **kw)


_RUNS = {}


def ran(i):
    """case i on the GPU, once: the step (with q8_out) on caches A, the 16-bit call with the append on caches B, the fp8 decode call
    on the step's q8_out and caches A with cache_seqlens = len_eff"""
    if i in _RUNS:
        return _RUNS[i]
    from common.attention_ex import flash_attn_fp8_with_kvcache, flash_attn_with_kvcache

    call = _built(i)[0]
    ka, va, alloc_a = caches(call)
    kb, vb, alloc_b = caches(call)
    q8 = torch.full(call["q"].shape, 0x7F, dtype=torch.uint8, device=DEV)
    o, lse = run_step(call, ka, va, q8_out=q8.view(E4))
    kw = common_kw(call)
    flash_attn_with_kvcache(_dev(call["q"]), kb.view(E4), vb.view(E4), k=_dev(call["k_new"]), v=_dev(call["v_new"]),
                            rotary_cos=_dev(call["rotary_cos"]), rotary_sin=_dev(call["rotary_sin"]),
                            rotary_interleaved=call["rotary_interleaved"], cache_seqlens=_dev(call["cache_seqlens"]), **kw)
    len_eff = torch.tensor([x + call["nnew"] for x in ref.clamped(call)], dtype=torch.int32, device=DEV)
    o2, lse2 = flash_attn_fp8_with_kvcache(q8.view(E4), ka.view(E4), va.view(E4), cache_seqlens=len_eff, q_descale=_dev(call["q_descale"]),
                                           out_dtype=call["dtype"], **kw)
    torch.cuda.synchronize()
    _RUNS[i] = dict(o=o.cpu(), lse=lse.cpu(), o2=o2.cpu(), lse2=lse2.cpu(), q8=q8.cpu(), ka=ka.cpu(), va=va.cpu(), alloc_a=alloc_a.cpu(),
                    alloc_b=alloc_b.cpu())
    return _RUNS[i]


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_cache_bytes_are_the_16_bit_calls_append(i):
    r = ran(i)
    assert torch.equal(r["alloc_a"], r["alloc_b"])
    call = _built(i)[0]
    assert not torch.equal(r["ka"], call["k_cache"]) and not torch.equal(r["va"], call["v_cache"])   # (something was appended)


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_q8_is_the_models_in_every_byte(i):
    _call, (_ka, _va, q8, _len), _want, _base = _built(i)
    assert torch.equal(ran(i)["q8"], q8)


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_no_byte_but_the_appended_slots_is_written(i):
    """the model writes the slots kvcache_full_ref.front_half lists and nothing else (tests/test_fp8_step_cpu.py): every other byte is
    the 0xA5 fill or the older token it was, and a dropped token (a row outside the cache, a page outside the pool) wrote nowhere"""
    call, (ka, va, _q8, _len), _want, _base = _built(i)
    r = ran(i)
    assert torch.equal(r["ka"], ka) and torch.equal(r["va"], va)
    changed = int((r["ka"] != call["k_cache"]).any(-1).any(-1).sum())
    dropped = call["nnew"] if call["layout"] in ("bidx", "paged_hole") else 0
    assert 0 < changed <= call["B"] * call["nnew"] - dropped


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_attention_is_the_fp8_decode_call_bit_for_bit(i):
    r = ran(i)
    assert torch.equal(r["o"], r["o2"]) and torch.equal(r["lse"], r["lse2"])
    assert r["o"].dtype == _built(i)[0]["dtype"]


@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_sharp_bar_against_fp64(i):
    call = _built(i)[0]
    r = ran(i)
    att = ref.attention_call(call, r["ka"], r["va"], r["q8"], [x + call["nnew"] for x in ref.clamped(call)])
    want, base = fm.reference(att), fk.rounded(fm.baseline(att), call["dtype"])
    got = fk.pack(r["o"], r["lse"], att)
    assert not bool(torch.isnan(got.lse).any()) and bool(torch.isfinite(got.o.float()).all())
    assert torch.equal(torch.isfinite(got.lse), torch.isfinite(want.lse))
    bad, ratio = fk.tile_bar(got, want, base, call["dtype"])
    top = sorted(ratio.items(), key=lambda kv: -kv[1])[:2]
    print(f"RATIO {IDS[i]} " + " ".join(f"{k}={v:.3f}" for k, v in top))
    assert not bad, bad


@pytest.mark.parametrize("i", [0, 3, 6, 8], ids=[IDS[i] for i in (0, 3, 6, 8)])
def test_the_workspace_q8_gives_the_bits_of_q8_out(i):
    """without q8_out the codes live in the call's workspace: the same o, lse and cache bytes"""
    call = _built(i)[0]
    ka, va, _alloc = caches(call)
    o, lse = run_step(call, ka, va)
    r = ran(i)
    assert torch.equal(o.cpu(), r["o"]) and torch.equal(lse.cpu(), r["lse"]) and torch.equal(ka.cpu(), r["ka"]) and torch.equal(va.cpu(), r["va"])


@pytest.mark.parametrize("i", [1, 2, 4, 9], ids=[IDS[i] for i in (1, 2, 4, 9)])
def test_e4m3_mode_copies_the_bytes_and_uses_q_in_place(i):
    """q, k, v as codes: the new bytes land as they are (the model's slots), q is used in place, o is the decode call's on the appended
    cache; q8_out and rotary are refused by name"""
    from common.attention_ex import flash_attn_fp8_kvcache_step, flash_attn_fp8_with_kvcache

    call, (_ka, _va, q8_m, len_eff), _want, _base = _built(i)
    k8 = quantize(call["k_new"], ref.scales_bh(call["k_descale"], call["B"], call["hkv"]))   # (no rotary in this mode)
    v8 = quantize(call["v_new"], ref.scales_bh(call["v_descale"], call["B"], call["hkv"]))
    plain = dict(call, rotary_cos=None, rotary_sin=None)
    ka_w, va_w, _q, _l = ref.model(plain)
    ka, va, _alloc = caches(call)
    kw = dict(common_kw(call), q_descale=_dev(call["q_descale"]))
    q8 = q8_m.to(DEV).view(E4)
    o, lse = flash_attn_fp8_kvcache_step(q8, ka.view(E4), va.view(E4), k8.to(DEV).view(E4), v8.to(DEV).view(E4),
                                         cache_seqlens=_dev(call["cache_seqlens"]), **kw)
    assert o.dtype == torch.bfloat16                                  # the default in e4m3 mode
    assert torch.equal(ka.cpu(), ka_w) and torch.equal(va.cpu(), va_w)
    assert torch.equal(q8.view(torch.uint8).cpu(), q8_m)
    o2, lse2 = flash_attn_fp8_with_kvcache(q8, ka.view(E4), va.view(E4), cache_seqlens=torch.tensor(len_eff, dtype=torch.int32, device=DEV),
                                           **kw)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    with pytest.raises(NotImplementedError, match="q8_out is not supported"):
        flash_attn_fp8_kvcache_step(q8, ka.view(E4), va.view(E4), k8.to(DEV).view(E4), v8.to(DEV).view(E4),
                                    cache_seqlens=_dev(call["cache_seqlens"]), q8_out=torch.empty_like(q8), **kw)
    assert torch.equal(ka.cpu(), ka_w)


@pytest.mark.parametrize("i", [8, 5], ids=[IDS[8], IDS[5]])
def test_a_graph_replays_after_its_inputs_changed_in_place(i):
    """one captured step; then cache_seqlens, k, v, q, a table row (paged) and the descales change in place: the replay equals the
    eager call on the new values, in o, lse, q8_out and every cache byte"""
    call = _built(i)[0]
    g = torch.Generator().manual_seed(77 + i)
    st = {n: _dev(call[n]) for n in ("q", "k_new", "v_new", "cache_seqlens", "block_table", "q_descale", "k_descale", "v_descale")}
    ka, va, alloc = caches(call)
    start = alloc.clone()
    q8 = torch.zeros(call["q"].shape, dtype=torch.uint8, device=DEV)

    cos, sin = _dev(call["rotary_cos"]), _dev(call["rotary_sin"])

    from common.attention_ex import flash_attn_fp8_kvcache_step
    kw = dict(common_kw(call), cache_seqlens=st["cache_seqlens"], block_table=st["block_table"], q_descale=st["q_descale"],
              k_descale=st["k_descale"], v_descale=st["v_descale"], rotary_cos=cos, rotary_sin=sin,
              rotary_interleaved=call["rotary_interleaved"], q8_out=q8.view(E4))

    def step():   # on the static tensors (no host copy inside): the call that is captured, and the eager call it is compared with
        return flash_attn_fp8_kvcache_step(st["q"], ka.view(E4), va.view(E4), st["k_new"], st["v_new"], **kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # the warm-up sizes the shim's workspace before the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    alloc.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step()
    # everything a replay may change, in place
    st["cache_seqlens"].copy_(torch.tensor([40, ref.CAPACITY + 9, 5], dtype=torch.int32))
    for n in ("q", "k_new", "v_new"):
        st[n].copy_((1.5 * torch.randn(call[n].shape, generator=g)).to(call["dtype"]))
    for n in ("q_descale", "k_descale", "v_descale"):
        st[n].mul_(1.75)
    if st["block_table"] is not None:
        st["block_table"][0].copy_(st["block_table"][0].flip(0))
    alloc.copy_(start)
    graph.replay()
    torch.cuda.synchronize()
    got = (o.cpu(), lse.cpu(), q8.cpu(), alloc.cpu())
    alloc.copy_(start)
    q8.zero_()
    o_e, lse_e = step()
    torch.cuda.synchronize()
    assert torch.equal(got[0], o_e.cpu()) and torch.equal(got[1], lse_e.cpu())
    assert torch.equal(got[2], q8.cpu()) and torch.equal(got[3], alloc.cpu())
    assert not torch.equal(got[3], start.cpu()) and bool((got[2] != 0).any())


def test_route_counters():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_fp8_with_kvcache

    names = ("fp8kv_step_prep", "fp8kv_split_mod")
    for i, mod in ((0, 0), (4, 1)):                                # a bare call, and one with window + softcap + sinks
        call = _built(i)[0]
        assert bool(call["sinks"] is not None) == bool(mod)
        ka, va, _alloc = caches(call)
        before = tuple(ext.route_count(n) for n in names)
        run_step(call, ka, va)
        assert tuple(ext.route_count(n) for n in names) == (before[0] + 1, before[1] + mod)
        before = tuple(ext.route_count(n) for n in names)
        q8 = torch.zeros(call["q"].shape, dtype=torch.uint8, device=DEV).view(E4)
        flash_attn_fp8_with_kvcache(q8, ka.view(E4), va.view(E4), cache_seqlens=_dev(call["cache_seqlens"]).clamp(0, ref.CAPACITY),
                                    q_descale=_dev(call["q_descale"]), **common_kw(call))
        assert tuple(ext.route_count(n) for n in names) == (before[0], before[1] + mod)   # the parent alone counts no prep
    torch.cuda.synchronize()
