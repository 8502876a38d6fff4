"""GPU: the lean form of the dS-storing dK/dV stream kernel (csrc/fa_bwd_dkdv_w4.hip, template flag LEAN) against the general form
forced by option dkdv_lean = 2, on the same inputs.  The lean form loads the row constants once per block and reads its operands
through immediates of one block body per tile buffer; every accumulation chain keeps its order, so dK, dV and the stored dS — which
dQ is made from — are the general form's bit for bit.  Shapes: the smallest that reach one buffer, the unroll's remainders 1 and 3,
the wrap-around of the four buffers, and two key tiles.  Which form ran is read back from the library (fa_route_count)."""
import functools

import pytest
import torch

from tests import ex_full_ref as fr
from tests import hot_cases as hc
from tests import test_hot_sweep_gpu as hs

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPTIONS = ("small_grid", "dq", "dkdv_lean")

# (bh, query rows, keys): 1, 3, 5 and 9 blocks of 32 queries over one key tile; two key tiles
LEAN_SHAPES = [(3, 32, 256), (3, 96, 256), (3, 160, 256), (3, 288, 256), (2, 512, 512)]


@functools.lru_cache(maxsize=None)
def problem(key):
    call = hc.build_call(key)
    return call, fr.full_reference(call)


def run(opts, q, k, v, do, causal, scale):
    """(o, lse, dq, dk, dv) and the launches of (general, lean) form the call made; Nq != Nk or grouped K/V: the extended entry"""
    import flashattention_lab_cuda as ext

    before = (ext.route_count("dkdv_stream"), ext.route_count("dkdv_lean"))
    try:
        for name, val in opts.items():
            ext.set_option(name, val)
        if q.shape[1] != k.shape[1] or q.shape[0] != k.shape[0]:
            o, lse = ext.ex_forward(q, k, v, causal, scale)
            dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, causal, scale)
        else:
            o, lse = ext.forward(q, k, v, causal, scale, 128, 128)
            dq, dk, dv = ext.backward(q, k, v, o, do, lse, causal, scale, 128, 128)
    finally:
        for name in OPTIONS:
            ext.set_option(name, 0)
    torch.cuda.synchronize()
    return (o, lse, dq, dk, dv), (ext.route_count("dkdv_stream") - before[0], ext.route_count("dkdv_lean") - before[1])


def both_forms(call, base_opts):
    dev = tuple(call[n].to(DEV) for n in ("q", "k", "v", "do"))
    new, took_new = run(base_opts, *dev, call["causal"], call["scale"])
    old, took_old = run(dict(base_opts, dkdv_lean=2), *dev, call["causal"], call["scale"])
    return new, took_new, old, took_old


def assert_same_bits(new, old, what):
    for name, x, y in zip(hs.NAMES5, new, old):
        assert torch.equal(x, y), (what, name, (x.float() - y.float()).abs().max().item())


@pytest.mark.parametrize("dtype", hc.B16)
@pytest.mark.parametrize("shape", LEAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lean_form_is_bitwise_the_general_form_and_inside_the_bars(shape, dtype):
    key = (shape, 128, dtype, "none", "default")
    call, ref = problem(key)
    ro = hc.route_of(dict(route="sg1" if shape[1] == shape[2] else "nqnk", dtype=dtype, mask="none", d=128, shape=shape, scale="default"))
    assert ro["chunks"] == 1 and any(",DS>" in kern for kern in ro["bwd"])      # the hand-over: the dS-storing kernel
    new, took_new, old, took_old = both_forms(call, {"small_grid": 1})
    assert took_new == (0, 1), f"the default took (general, lean) = {took_new} launches"
    assert took_old == (1, 0), f"dkdv_lean = 2 took (general, lean) = {took_old} launches"
    assert_same_bits(new, old, shape)
    base = fr.baseline(call, model=ro["model"])
    hs.hold_to_the_bars(f"lean-{'x'.join(map(str, shape))}-{dtype}", hs.as_result(new), call, ref, base, "route=lean")


@pytest.mark.parametrize("dtype", hc.B16)
def test_grouped_keys_through_the_extended_entry(dtype):
    """kv_group = 2: four query units over two K/V units, five blocks over one key tile"""
    g = torch.Generator(device="cpu").manual_seed(7)
    dt = hc.DTYPES[dtype]
    q, do = (torch.randn((4, 160, 128), generator=g).to(dt) for _ in range(2))
    k, v = (torch.randn((2, 256, 128), generator=g).to(dt) for _ in range(2))
    call = dict(q=q, k=k, v=v, do=do, causal=False, scale=128 ** -0.5)
    new, took_new, old, took_old = both_forms(call, {"small_grid": 1})
    assert took_new == (0, 1) and took_old == (1, 0), (took_new, took_old)
    assert new[3].shape == k.shape and new[4].shape == v.shape
    assert_same_bits(new, old, "grouped")


@pytest.mark.parametrize("what,shape,mask,opts", [("ragged key tile", (3, 96, 320), "none", {"small_grid": 1}),
                                                  ("causal", (2, 512, 512), "causal", {"small_grid": 1, "dq": 6})], ids=["nk320", "causal"])
def test_launches_that_can_need_the_mask_keep_the_general_form(what, shape, mask, opts):
    call, _ref = problem((shape, 128, "bf16", mask, "default"))
    new, took_new, old, took_old = both_forms(call, opts)
    assert took_new == (1, 0), f"{what}: the default took (general, lean) = {took_new} launches"
    assert took_old == (1, 0)
    assert_same_bits(new, old, what)
