"""The production instantiation of the staggered forward (no debug word, no trace stamps, the masked block behind a branch, the
in-stream DMA state advanced in scalar registers) against the debug instantiation, which is the kernel as it was: the two
perform the same operations in the same order, so `o` and `lse` must be BITWISE equal.  The debug one is forced with
fwd_abl = 64 (which wave half lags: changes no value); fwd_stag = 3 selects the staggered kernel with the default schedule on
both sides, so the shapes can be the smallest at which it can go wrong: 9 tiles with a ragged last one and out-of-range DMA
pieces, the padded head dim, per-wave tile counts that differ under the mask, and Nk != Nq through the extended path."""
import pytest
import torch

import flashattention_lab_cuda as ext

pytestmark = pytest.mark.gpu


def _production_and_debug(fn):
    outs = []
    try:
        ext.set_option("fwd_stag", 3)
        for abl in (0, 64):
            ext.set_option("fwd_abl", abl)
            outs.append(fn())
            torch.cuda.synchronize()
    finally:
        ext.set_option("fwd_abl", 0)
        ext.set_option("fwd_stag", 0)
    return outs


def _same(a, b):
    (o1, l1), (o2, l2) = a, b
    assert torch.isfinite(o1.float()).all() and torch.isfinite(l1).all()
    assert torch.isfinite(o2.float()).all() and torch.isfinite(l2).all()
    assert torch.equal(o1, o2)
    assert torch.equal(l1, l2)


def _qkv(bh, nq, nk, d, dtype, device):
    g = torch.Generator(device=device).manual_seed(bh + nq + nk + d)
    q = torch.randn((bh, nq, d), device=device, dtype=dtype, generator=g)
    k, v = (torch.randn((bh, nk, d), device=device, dtype=dtype, generator=g) for _ in range(2))
    return q, k, v


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bh,n,d,causal", [(160, 1100, 128, False), (160, 1100, 128, True), (160, 1100, 96, False),
                                           (160, 1100, 96, True), (8, 8292, 128, True)])
def test_production_equals_debug_instantiation(dtype, bh, n, d, causal, device):
    q, k, v = _qkv(bh, n, n, d, dtype, device)
    _same(*_production_and_debug(lambda: ext.forward(q, k, v, causal, d ** -0.5, 64, 128)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [False, True])
def test_production_equals_debug_instantiation_nq_ne_nk(dtype, causal, device):
    q, k, v = _qkv(32, 2048, 4096, 128, dtype, device)
    _same(*_production_and_debug(lambda: ext.ex_forward(q, k, v, causal, 128 ** -0.5)))


def test_default_dispatch_is_the_production_kernel_again_after_a_debug_run(device):
    """No option set (the default dispatch picks the staggered kernel at this shape), then fwd_abl set and taken back: the
    same bits every time, and the same as the debug instantiation's."""
    d = 128
    q, k, v = _qkv(160, 1100, 1100, d, torch.bfloat16, device)
    before = ext.forward(q, k, v, False, d ** -0.5, 64, 128)
    prod, dbg = _production_and_debug(lambda: ext.forward(q, k, v, False, d ** -0.5, 64, 128))
    after = ext.forward(q, k, v, False, d ** -0.5, 64, 128)
    torch.cuda.synchronize()
    _same(before, dbg)
    _same(before, prod)
    _same(before, after)
