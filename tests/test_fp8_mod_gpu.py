"""GPU: a sliding window, a softcap and attention sinks on the padded, packed and paged fp8 calls (fwd_fp8in_mod_kernel in
csrc/fa_fp8_inputs.hip; flash_attn_fp8_func, flash_attn_fp8_varlen_func).  Every table case of tests/fp8_mod_ref.py,
bare, capped, with sinks and with both, in bf16 and f16, at the sharp bar per 256-row tile against the project's fp64 reference with
the baseline of tests/fp8_mod_ref.py; the bit identities (a head whose sink is -inf, default trailing arguments, every packed or
paged sequence against the padded call on it alone); the route counters.  The proofs that reference, baseline and mutants are what
they claim run on the CPU (tests/test_fp8_mod_cpu.py)."""
import pytest
import torch

from common.attention_ex import flash_attention_fp8, flash_attention_fp8_varlen, flash_attn_fp8_func, flash_attn_fp8_varlen_func
from tests import fp8_inputs_ref as fr
from tests import fp8_mod_ref as fm
from tests.fp8_ref import tiled_sharp_bar
from tests.test_fp8_mod_cpu import PADDED, PADDED_IDS, padded_base

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4M3 = torch.float8_e4m3fn
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def on_dev(t):
    return None if t is None else t.to(DEV)


def run(call, **over):
    """the padded call on the GPU as a Result with units (B * H_q, Nq, .) on the CPU"""
    q, k, v = (call[n].view(E4M3).to(DEV) for n in ("q8", "k8", "v8"))
    kw = dict(q_descale=on_dev(call["q_descale"]), k_descale=on_dev(call["k_descale"]), v_descale=on_dev(call["v_descale"]),
              softmax_scale=call["scale"], causal=call["causal"], out_dtype=call["dtype"], layout="bhnd", return_lse=True,
              window_size=call["window"], softcap=call["softcap"], sinks=on_dev(call["sinks"]))
    kw.update(over)
    o, lse = flash_attn_fp8_func(q, k, v, **kw)
    torch.cuda.synchronize()
    assert o.dtype == kw["out_dtype"] and lse.dtype == torch.float32 and o.is_contiguous()
    return fr._result(o.reshape(-1, call["nq"], 128).cpu(), lse.reshape(-1, call["nq"]).cpu())


def same_bits(a, b):
    return torch.equal(a.o.view(torch.int16), b.o.view(torch.int16)) and torch.equal(a.lse.view(torch.int32), b.lse.view(torch.int32))


def routes():
    import flashattention_lab_cuda as ext

    return tuple(ext.route_count(n) for n in ("fp8in_fwd_mod", "fp8in_fwd_varlen_mod", "fp8kv_split_mod"))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("i,cap,snk", PADDED, ids=PADDED_IDS)
def test_every_padded_case_meets_the_sharp_bar(i, cap, snk, dt):
    call, ref, base = padded_base(i, cap, snk, DTYPES[dt])
    before = routes()
    got = run(call)
    assert routes() == (before[0] + 1, before[1], before[2])
    dead = ~fm.band(call).any(-1)[None, :].expand_as(ref.lse)
    assert not bool(torch.isnan(got.lse).any()) and bool(torch.isfinite(got.o.float()).all())
    assert bool((got.o[dead] == 0).all())
    if snk:          # a row without a visible key: lse = the sink exactly (-inf for the head at -inf); +-1e4 stay finite
        want = call["sinks"].repeat(call["B"])[:, None].expand_as(got.lse)
        assert torch.equal(got.lse[dead], want[dead])
        assert bool(torch.isfinite(got.lse[call["sinks"].repeat(call["B"]) > float("-inf")]).all())
    else:
        assert torch.equal(got.lse == float("-inf"), dead)
    bad, ratio = tiled_sharp_bar(got, ref, base, call["dtype"])
    print(PADDED_IDS[PADDED.index((i, cap, snk))], dt, " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
    assert not bad, bad
    if snk:          # the head whose sink is -inf has the bits of the same call without sinks
        bare = run(call, sinks=None)
        u = torch.arange(call["B"]) * call["hq"] + 1
        assert float(call["sinks"][1]) == float("-inf")
        assert torch.equal(got.o[u], bare.o[u]) and torch.equal(got.lse[u], bare.lse[u])


def test_default_trailing_arguments_are_the_parent_call(monkeypatch):
    """flash_attn_fp8_func without the three, and fa_fp8_forward_mod itself with (-1, -1, 0.0, NULL, 0), launch the parent's kernels:
    the parent's bits, no count on the featured route"""
    import flashattention_lab_cuda as ext

    call = dict(fm.build_call(0), window=(-1, -1))
    q, k, v = (call[n].view(E4M3).to(DEV) for n in ("q8", "k8", "v8"))
    kw = dict(q_descale=on_dev(call["q_descale"]), k_descale=on_dev(call["k_descale"]), v_descale=on_dev(call["v_descale"]),
              softmax_scale=call["scale"], causal=True, return_lse=True)
    before = routes()
    parent = flash_attention_fp8(q, k, v, **kw)
    new = flash_attn_fp8_func(q, k, v, **kw)
    monkeypatch.setattr(ext, "_fp8_mod", lambda *a: ("_mod", (-1, -1, 0.0, 0, 0), None))
    through_mod = flash_attention_fp8(q, k, v, **kw)
    torch.cuda.synchronize()
    assert routes() == before
    for got in (new, through_mod):
        assert torch.equal(got[0], parent[0]) and torch.equal(got[1], parent[1])


# ---- packed and paged

def _zero_keys(call, a, z):
    """the padded call with keys [a, z) of K and V as zero bytes (what a page outside the pool reads as)"""
    k8, v8 = call["k8"].clone(), call["v8"].clone()
    k8[:, :, a:z], v8[:, :, a:z] = 0, 0
    return dict(call, k8=k8, v8=v8)


def _varlen_run(v, ps=0, bad_page=None, strided_q=False):
    """(o (total_q, H_q, 128), lse (H_q, total_q)) on the CPU of flash_attn_fp8_varlen_func on the case; ps > 0: K and V as pools
    behind a block table (bad_page = (sequence, slot): that entry points outside the pool)"""
    q = v["q8"].view(E4M3).to(DEV)
    if strided_q:        # a head- and token-strided view: a slice of a fused projection
        buf = torch.zeros((q.shape[0], 3, q.shape[1], 128), dtype=torch.uint8, device=DEV).view(E4M3)
        buf[:, 1] = q
        q = buf[:, 1]
        assert not q.is_contiguous()
    kw = dict(q_descale=on_dev(v["q_descale"]), k_descale=on_dev(v["k_descale"]), v_descale=on_dev(v["v_descale"]),
              softmax_scale=v["scale"], causal=v["causal"], out_dtype=v["dtype"], return_softmax_lse=True, window_size=v["window"],
              softcap=v["softcap"], sinks=on_dev(v["sinks"]))
    cu_q, cu_k = v["cu_q"].to(DEV), v["cu_k"].to(DEV)
    if ps == 0:
        k, vv = v["k8"].view(E4M3).to(DEV), v["v8"].view(E4M3).to(DEV)
    else:
        need = [(n + ps - 1) // ps for n in fm.SEQ_K]
        nblk, mblk = sum(need) + 2, max(need) + 1
        g = torch.Generator().manual_seed(3)
        perm = torch.randperm(nblk, generator=g).tolist()
        table = torch.randint(-3, nblk + 3, (v["B"], mblk), generator=g, dtype=torch.int32)
        kp = torch.full((nblk, ps, fm.HKV, 128), 0x7F, dtype=torch.uint8)
        vp = torch.full((nblk, ps, fm.HKV, 128), 0x7F, dtype=torch.uint8)
        for b, n in enumerate(fm.SEQ_K):
            k0 = int(v["cu_k"][b])
            for j in range(need[b]):
                pg = perm.pop()
                table[b, j] = pg
                m = min(ps, n - j * ps)
                kp[pg, :m], vp[pg, :m] = v["k8"][k0 + j * ps:k0 + j * ps + m], v["v8"][k0 + j * ps:k0 + j * ps + m]
        if bad_page is not None:
            table[bad_page[0], bad_page[1]] = nblk + 7
        k, vv, kw["block_table"] = kp.view(E4M3).to(DEV), vp.view(E4M3).to(DEV), table.to(DEV)
    o, lse = flash_attn_fp8_varlen_func(q, k, vv, cu_q, cu_k, max(fm.SEQ_Q), max(fm.SEQ_K), **kw)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize("form", ["packed", "ps16", "ps64"])
@pytest.mark.parametrize("causal,window,cap,snk", [(True, (20, -1), True, True), (False, (30, 9), False, True), (True, (0, -1), True, False)],
                         ids=["causal-L20-cap-sinks", "L30R9-sinks", "causal-L0-cap"])
def test_every_sequence_is_the_padded_call_on_it_alone(form, causal, window, cap, snk):
    v = fm.varlen_case(causal, window, cap, snk)
    ps = 0 if form == "packed" else int(form[2:])
    bad_page = None
    if ps:               # one entry of the 300-key sequence points outside the pool: its keys read as zero bytes
        bad_page = (3, 2)
        v = dict(v, calls=[c if b != 3 else _zero_keys(c, 2 * ps, 3 * ps) for b, c in enumerate(v["calls"])])
    before = routes()
    o, lse = _varlen_run(v, ps, bad_page, strided_q=(form != "ps64"))
    assert routes() == (before[0], before[1] + 1, before[2])
    assert not bool(torch.isnan(lse).any()) and bool(torch.isfinite(o.float()).all())
    # every sequence: the bits of the padded call
    for b, c in enumerate(v["calls"]):
        a, z = int(v["cu_q"][b]), int(v["cu_q"][b + 1])
        if z == a:
            continue
        if c is None:    # no key at all: o = 0, lse = the sink (-inf without one)
            want = torch.full((fm.HQ,), float("-inf")) if v["sinks"] is None else v["sinks"]
            assert bool((o[a:z] == 0).all()) and torch.equal(lse[:, a:z], want[:, None].expand(fm.HQ, z - a))
            continue
        one = run(c)
        assert torch.equal(o[a:z].transpose(0, 1), one.o) and torch.equal(lse[:, a:z], one.lse), (form, b)
    # the whole against the sharp bar
    ro, rl = fm.varlen_expected(v, fm.reference)
    bo, bl = fm.varlen_expected(v, fm.baseline)
    got, ref, base = (fr._result(x.transpose(0, 1), y) for x, y in ((o, lse), (ro, rl), (bo, bl)))
    bad, _ratio = tiled_sharp_bar(got, ref, base, v["dtype"])
    assert not bad, bad


def test_varlen_default_trailing_arguments_are_the_parent_call():
    v = fm.varlen_case(True, (-1, -1), False, False)
    q, k, vv = (v[n].view(E4M3).to(DEV) for n in ("q8", "k8", "v8"))
    args = (q, k, vv, v["cu_q"].to(DEV), v["cu_k"].to(DEV), max(fm.SEQ_Q), max(fm.SEQ_K))
    kw = dict(q_descale=on_dev(v["q_descale"]), k_descale=on_dev(v["k_descale"]), v_descale=on_dev(v["v_descale"]), causal=True,
              return_softmax_lse=True)
    before = routes()
    parent = flash_attention_fp8_varlen(*args, **kw)
    new = flash_attn_fp8_varlen_func(*args, **kw)
    torch.cuda.synchronize()
    assert routes() == before
    tq = int(v["cu_q"][-1])
    assert torch.equal(new[0][:tq], parent[0][:tq]) and torch.equal(new[1][:, :tq], parent[1][:, :tq])
