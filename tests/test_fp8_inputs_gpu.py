"""GPU: FlashAttention-3's fp8 call (csrc/fa_fp8_inputs.hip; flash_attention_fp8) on the table of
tests/fp8_inputs_cases.py: the V^T bytes of the transposer, every case at the sharp bar per 256-row tile against the fp64 reference
with the baseline of tests/fp8_inputs_ref.py, the descale, GQA, layout and batch bit identities, and a graph replay with changed
descales.  The proofs that reference, baseline and mutants are what they claim run on the CPU (tests/test_fp8_inputs_cpu.py)."""
import pytest
import torch

from common.attention_ex import flash_attention_fp8
from tests import fp8_inputs_cases as fc
from tests import fp8_inputs_ref as fr
from tests.fp8_ref import SENTINEL, tiled_sharp_bar
from tests.test_fp8_inputs_cpu import IDS, _case

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4M3 = torch.float8_e4m3fn


def device_tensors(call, layout=None):
    """q, k, v on the device as `layout` (default: the call's) wants them, and the layout string of the wrapper.  "prefix": K and V
    are the [:, :Nk] views of (B, Nk + 37, H_kv, 128) buffers filled with the e4m3 NaN byte"""
    layout = layout or call["layout"]
    q, k, v = (call[n].view(E4M3) for n in ("q8", "k8", "v8"))
    if layout == "bhnd":
        return q.to(DEV), k.to(DEV), v.to(DEV), "bhnd"
    q = q.transpose(1, 2).contiguous().to(DEV)
    if layout == "bnhd":
        return q, k.transpose(1, 2).contiguous().to(DEV), v.transpose(1, 2).contiguous().to(DEV), "bnhd"
    assert layout == "prefix"
    nk = call["nk"]
    views = []
    for t in (k, v):
        buf = torch.full((call["B"], nk + fc.PREFIX_EXTRA, call["hkv"], 128), SENTINEL, dtype=torch.uint8, device=DEV)
        buf[:, :nk] = t.view(torch.uint8).transpose(1, 2).to(DEV)
        views.append(buf.view(E4M3)[:, :nk])
    return q, views[0], views[1], "bnhd"


def on_dev(t):
    return None if t is None else t.to(DEV)


def run(call, layout=None, **over):
    """the call on the GPU as a Result with units (B * H_q, Nq, .) on the CPU"""
    q, k, v, lay = device_tensors(call, layout)
    kw = dict(q_descale=on_dev(call["q_descale"]), k_descale=on_dev(call["k_descale"]), v_descale=on_dev(call["v_descale"]),
              softmax_scale=call["scale"], causal=call["causal"], out_dtype=call["dtype"], layout=lay, return_lse=True)
    kw.update(over)
    o, lse = flash_attention_fp8(q, k, v, **kw)
    torch.cuda.synchronize()
    assert o.dtype == kw["out_dtype"] and lse.dtype == torch.float32 and o.is_contiguous()
    if lay == "bnhd":
        o = o.transpose(1, 2)
    return fr._result(o.reshape(-1, call["nq"], 128).cpu(), lse.reshape(-1, call["nq"]).cpu())


def same_bits(a, b):
    return torch.equal(a.o.view(torch.int16), b.o.view(torch.int16)) and torch.equal(a.lse.view(torch.int32), b.lse.view(torch.int32))


@pytest.mark.parametrize("i", [2, 6, 8, 9], ids=[IDS[i] for i in (2, 6, 8, 9)])
def test_the_transposer_writes_the_expected_bytes_and_nothing_else(i, monkeypatch):
    """V^T in a caller workspace cut out of a 0x7F buffer: the expected bytes exactly, the pad and the surroundings untouched"""
    import flashattention_lab_cuda as ext

    call = _case(i)[0]
    need = fr.workspace_bytes(call)
    buf = torch.full((need + 8192,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = buf[4096:4096 + need]
    monkeypatch.setattr(ext, "_workspace", lambda device, nbytes: ws if nbytes == need else None)
    run(call)
    got = buf.cpu()
    assert torch.equal(got[4096:4096 + need - 256], fr.expected_v8t(call).reshape(-1))
    assert bool((got[:4096] == SENTINEL).all()) and bool((got[4096 + need - 256:] == SENTINEL).all())


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_every_case_meets_the_sharp_bar(i):
    call, ref, base, _trace = _case(i)
    got = run(call)
    dead = ~torch.isfinite(ref.lse)
    assert not bool(torch.isnan(got.lse).any()) and torch.equal(got.lse == float("-inf"), dead)
    assert bool(torch.isfinite(got.lse[~dead]).all()) and bool(torch.isfinite(got.o.float()).all())
    assert bool((got.o[dead] == 0).all())
    bad, ratio = tiled_sharp_bar(got, ref, base, call["dtype"])
    print(IDS[i], " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
    assert not bad, bad
    assert same_bits(got, run(call))        # the same bits on a second run


def test_a_query_tile_without_any_visible_key():
    """(Nq, Nk) = (300, 40) under the mask: the diagonal is shifted by -260, so the whole first query tile is dead (the workgroup
    stages no key tile at all: fwd_fp8in_kernel, `ntiles == 0`) and the second has 4 dead rows beside its 40 live ones"""
    c = dict(heads=(4, 2), n=(300, 40), mask="causal", dtype="bf16", layout="prefix", descale="bh", input="normal")
    call = fc.build_call(c, 99)
    ref, base = fr.reference(call), fr.baseline(call)
    got = run(call)
    dead = ~torch.isfinite(ref.lse)
    assert int(dead[0].sum()) == 260 and bool(dead[:, :256].all())
    assert torch.equal(got.lse == float("-inf"), dead) and bool((got.o[dead] == 0).all()) and bool(torch.isfinite(got.o.float()).all())
    bad, _ratio = tiled_sharp_bar(got, ref, base, call["dtype"])
    assert not bad, bad


def _pick(**want):
    """the first case of the table with these axis values"""
    for i, c in enumerate(fc.CASES):
        if all(c[k] == v for k, v in want.items()):
            return _case(i)[0]
    raise AssertionError(want)


def test_power_of_two_q_and_k_descales_are_the_softmax_scale():
    call = dict(_pick(heads=(4, 2), mask="causal", descale="none"))
    plain = run(call, softmax_scale=call["scale"] * 2.0 ** (3 - 5))
    qd = torch.full((call["B"], call["hkv"]), 8.0)
    kd = torch.full((call["hkv"],), 2.0 ** -5)
    assert same_bits(run(call, q_descale=qd.to(DEV), k_descale=kd.to(DEV)), plain)


def test_a_power_of_two_v_descale_scales_o_exactly():
    call = dict(_pick(dtype="bf16", descale="none", input="normal"))
    plain = run(call)
    vd = torch.exp2(torch.arange(call["B"] * call["hkv"], dtype=torch.float32) - 2.0).reshape(call["B"], call["hkv"])
    got = run(call, v_descale=vd.to(DEV))
    per_unit = vd.reshape(-1)[fr.kv_unit(call)][:, None, None]
    assert torch.equal(got.o.float(), plain.o.float() * per_unit) and torch.equal(got.lse, plain.lse)


@pytest.mark.parametrize("heads", [(4, 2), (3, 1)])
def test_gqa_is_the_ungrouped_call_on_repeated_heads(heads):
    call = dict(_pick(heads=heads, descale="bh"))
    g = heads[0] // heads[1]
    wide = dict(call, hkv=heads[0], k8=call["k8"].repeat_interleave(g, dim=1), v8=call["v8"].repeat_interleave(g, dim=1),
                **{n: call[n].repeat_interleave(g, dim=1) for n in ("q_descale", "k_descale", "v_descale")})
    assert same_bits(run(call, "bhnd"), run(wide, "bhnd"))


@pytest.mark.parametrize("i", [4, 16, 19], ids=[IDS[i] for i in (4, 16, 19)])
def test_views_and_batch_slices_give_the_contiguous_call_bits(i):
    call = _case(i)[0]
    plain = run(call, "bhnd")
    assert same_bits(run(call, "bnhd"), plain)
    assert same_bits(run(call, "prefix"), plain)
    hq = call["hq"]
    for b in range(call["B"]):
        one = dict(call, B=1, q8=call["q8"][b:b + 1], k8=call["k8"][b:b + 1], v8=call["v8"][b:b + 1],
                   **{n: (call[n] if call[n] is None or call[n].dim() == 1 else call[n][b:b + 1]) for n in ("q_descale", "k_descale", "v_descale")})
        got = run(one, "bhnd")
        assert torch.equal(got.o, plain.o[b * hq:(b + 1) * hq]) and torch.equal(got.lse, plain.lse[b * hq:(b + 1) * hq])


def test_graph_replay_with_changed_descales():
    call = _pick(heads=(4, 2), descale="bh", mask="causal")
    q, k, v, lay = device_tensors(call, "bnhd")
    ds = {n: call[n].to(DEV) for n in ("q_descale", "k_descale", "v_descale")}
    kw = dict(softmax_scale=call["scale"], causal=True, out_dtype=call["dtype"], layout=lay, return_lse=True, **ds)
    flash_attention_fp8(q, k, v, **kw)          # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = flash_attention_fp8(q, k, v, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        for t in ds.values():
            t.copy_(0.25 + 3.0 * torch.rand(t.shape, generator=g))
        graph.replay()
        torch.cuda.synchronize()
        eager = flash_attention_fp8(q, k, v, **kw)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    changed = dict(call, **{n: t.cpu() for n, t in ds.items()})
    ref, base = fr.reference(changed), fr.baseline(changed)
    got = fr._result(out[0].transpose(1, 2).reshape(-1, call["nq"], 128).cpu(), out[1].reshape(-1, call["nq"]).cpu())
    bad, _ratio = tiled_sharp_bar(got, ref, base, call["dtype"])
    assert not bad, bad
