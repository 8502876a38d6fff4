"""The forward's default schedule at 128-key tiles (K three buffers, V two, LDS-DMA inside the matrix phases) against the
two-buffer schedule it replaced (option fwd_stag = 4): the two perform the same operations in the same order inside every
accumulation chain, so `o` and `lse` must be BITWISE equal — dense and causal, bf16 and f16, full and ragged rows, the
padded head dim, and Nk != Nq through the extended path."""
import pytest
import torch

import flashattention_lab_cuda as ext

pytestmark = pytest.mark.gpu


def _both(fn):
    outs = []
    for stag in (0, 4):
        ext.set_option("fwd_stag", stag)
        try:
            outs.append(fn())
            torch.cuda.synchronize()
        finally:
            ext.set_option("fwd_stag", 0)
    return outs


# sizes at which the dispatch picks the staggered kernel (causal, d = 128: rows of 8192 and more, or of 4096 from 3072 row
# tiles on; the padded head dims always)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,d,bh,causal", [(4096, 128, 48, False), (4096, 128, 192, True), (1100, 128, 160, False),
                                           (8292, 128, 8, True), (1100, 96, 160, False), (1100, 96, 160, True)])
def test_default_equals_two_buffer_schedule(dtype, n, d, bh, causal, device):
    g = torch.Generator(device=device).manual_seed(n + d + int(causal))
    q, k, v = (torch.randn((bh, n, d), device=device, dtype=dtype, generator=g) for _ in range(3))
    (o1, l1), (o2, l2) = _both(lambda: ext.forward(q, k, v, causal, d ** -0.5, 64, 128))
    assert torch.isfinite(o1.float()).all()
    assert torch.equal(o1, o2)
    assert torch.equal(l1, l2)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("nq,nk", [(2048, 4096), (1100, 1500)])
def test_extended_path_nq_ne_nk(causal, nq, nk, device):
    bh, d = 32, 128
    g = torch.Generator(device=device).manual_seed(nq + nk)
    q = torch.randn((bh, nq, d), device=device, dtype=torch.bfloat16, generator=g)
    k, v = (torch.randn((bh, nk, d), device=device, dtype=torch.bfloat16, generator=g) for _ in range(2))
    (o1, l1), (o2, l2) = _both(lambda: ext.ex_forward(q, k, v, causal, d ** -0.5))
    assert torch.isfinite(o1.float()).all()
    assert torch.equal(o1, o2)
    assert torch.equal(l1, l2)
