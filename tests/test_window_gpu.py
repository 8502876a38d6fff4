"""GPU: sliding-window (local) attention (fa_ex_forward_window / fa_ex_backward_window through ex_forward / ex_backward and
flash_attention_ex's window_size).  The reference is the fp64 oracle with the window expressed as a dense mask (for GQA on K/V
repeated over each group, dK / dV summed over the group), on the extended MFMA kernels (ex_path 3), the exact-f32 kernels
(ex_path 1) and the default routing (ex_path 0)."""
import pytest
import torch

from oracle import attention_oracle as orc
from tests.helpers import dtype_tolerances

pytestmark = pytest.mark.gpu

PATHS = {"auto": 0, "exact": 1, "mfma_only": 3}


def window_mask(nq, nk, causal, window):
    """True = visible: the window in the causal flag's coordinates (bottom-right aligned)."""
    wl, wr = window
    i = torch.arange(nq).unsqueeze(1)
    j = torch.arange(nk).unsqueeze(0)
    c = nk - nq
    m = torch.ones((nq, nk), dtype=torch.bool)
    if wl >= 0:
        m &= j >= i + c - wl
    if wr >= 0:
        m &= j <= i + c + wr
    if causal:
        m &= j <= i + c
    return m


def _case(bh, bh_kv, nq, nk, d, dtype, seed, mask_kind=None, block=None, density=0.7):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((bh, nq, d), generator=g).to(dtype)
    k = torch.randn((bh_kv, nk, d), generator=g).to(dtype)
    v = torch.randn((bh_kv, nk, d), generator=g).to(dtype)
    do = torch.randn((bh, nq, d), generator=g).to(dtype)
    mask = bmask = None
    if mask_kind == "per_bh":
        mask = (torch.rand((bh, nq, nk), generator=g) < density).to(torch.uint8)
    if block is not None:
        br, bc = block
        bmask = (torch.rand(((nq + br - 1) // br, (nk + bc - 1) // bc), generator=g) < density).to(torch.uint8)
    return q, k, v, do, mask, bmask


def _oracle(q, k, v, do, g, causal, window, mask, **kw):
    """fp64 oracle with the window folded into the dense mask (no causal flag: the mask carries it)."""
    nq, nk = q.shape[1], k.shape[1]
    wm = window_mask(nq, nk, causal, window)
    m = wm.to(torch.uint8) if mask is None else (mask.bool() & wm).to(torch.uint8)
    qf, kf, vf = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o, lse = orc.extended_attention(qf, kf.repeat_interleave(g, 0), vf.repeat_interleave(g, 0), causal=False, mask=m, **kw)
    (o * do.double()).sum().backward()
    return qf.grad.to(q.dtype), kf.grad.to(q.dtype), vf.grad.to(q.dtype), o.detach().to(q.dtype), lse.detach().float()


def _run(ext, q, k, v, do, causal, scale, path=0, **kw):
    ext.set_option("ex_path", path)
    try:
        o, lse = ext.ex_forward(q, k, v, causal, scale, **kw)
        dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, causal, scale, **kw)
    finally:
        ext.set_option("ex_path", 0)
    return o, lse, dq, dk, dv


ORACLE_CASES = [
    # bh, g, nq, nk, d, causal, window, mask_kind, block, p, dtype, path
    (4, 1, 1024, 1024, 128, True, (256, 0), None, None, 0.0, torch.bfloat16, "mfma_only"),     # (L, 0) with causal, edge on a tile
    (4, 1, 1024, 1024, 128, False, (255, 100), None, None, 0.0, torch.float16, "mfma_only"),   # bidirectional
    (2, 1, 1024, 1536, 64, True, (1000, -1), None, None, 0.0, torch.bfloat16, "auto"),         # Nq < Nk
    (2, 1, 1280, 1024, 128, False, (-1, 100), None, None, 0.0, torch.bfloat16, "mfma_only"),   # Nq > Nk: dead rows at the top
    (2, 1, 1024, 1024, 64, False, (0, 0), None, None, 0.0, torch.float16, "mfma_only"),        # the diagonal alone
    (2, 1, 1024, 1100, 128, False, (17, 5), None, None, 0.0, torch.bfloat16, "auto"),          # inside one 32-block
    (2, 1, 1024, 1024, 128, False, (257, 30), "per_bh", None, 0.1, torch.bfloat16, "mfma_only"),  # + per-(b,h) mask, dropout
    (2, 1, 1024, 1100, 64, True, (100, -1), None, (32, 64), 0.0, torch.float16, "mfma_only"),  # + block-sparse
    (2, 1, 1056, 1056, 128, True, (1000, -1), None, (64, 32), 0.1, torch.bfloat16, "mfma_only"),  # block-sparse + dropout
    (8, 4, 1024, 1024, 128, True, (256, -1), None, None, 0.0, torch.bfloat16, "mfma_only"),    # g = 4 GQA
    (8, 4, 1024, 1200, 64, False, (300, 3), "per_bh", None, 0.1, torch.float16, "auto"),       # GQA, mask and dropout
    (2, 1, 300, 400, 40, False, (100, 30), None, None, 0.0, torch.bfloat16, "auto"),           # d = 40: the exact family
    (2, 1, 520, 520, 64, True, (255, -1), None, None, 0.0, torch.float32, "auto"),             # fp32: exact
    (2, 1, 1100, 1100, 128, True, (1000, 0), None, (64, 64), 0.0, torch.bfloat16, "exact"),
    (4, 2, 600, 700, 128, False, (256, 256), None, None, 0.1, torch.float16, "exact"),
    (2, 1, 700, 500, 32, False, (-1, 20), "per_bh", None, 0.0, torch.float32, "exact"),        # dead rows on the exact kernels
]


@pytest.mark.parametrize("bh,g,nq,nk,d,causal,window,mask_kind,block,p,dtype,path", ORACLE_CASES)
def test_window_matches_the_oracle(bh, g, nq, nk, d, causal, window, mask_kind, block, p, dtype, path, device):
    import flashattention_lab_cuda as ext

    q, k, v, do, mask, bmask = _case(bh, bh // g, nq, nk, d, dtype, seed=nq + nk + d + window[0], mask_kind=mask_kind, block=block)
    br, bc = block if block is not None else (128, 128)
    scale, seed = d ** -0.5, 3 + nk
    rq, rk, rv, ro, rlse = _oracle(q, k, v, do, g, causal, window, mask, softmax_scale=scale, block_mask=bmask, br=br, bc=bc,
                                   dropout_p=p, seed=seed)
    dev = lambda t: None if t is None else t.to(device)
    o, lse, dq, dk, dv = _run(ext, dev(q), dev(k), dev(v), dev(do), causal, scale, PATHS[path], mask=dev(mask), block_mask=dev(bmask),
                              br=br, bc=bc, dropout_p=p, seed=seed, window=window)
    assert dk.shape == k.shape and dv.shape == v.shape
    tol = dtype_tolerances(dtype)
    torch.testing.assert_close(o.cpu(), ro, **tol)
    live = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse.cpu()), live)
    torch.testing.assert_close(lse.cpu()[live], rlse[live], rtol=1e-3, atol=1e-3)
    for name, a, r in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        assert torch.isfinite(a.float()).all(), name
        torch.testing.assert_close(a.cpu(), r, **tol, msg=name)


def _bitwise(a, b):
    for x, y, name in zip(a, b, ("o", "lse", "dq", "dk", "dv")):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("path", ["auto", "mfma_only"])
@pytest.mark.parametrize("causal", [False, True])
def test_a_window_that_bounds_nothing_is_the_call_without_one(path, causal, device):
    """auto: the square 16-bit call takes the plain kernels (and their dS hand-over) either way; mfma_only: the extended ones."""
    import flashattention_lab_cuda as ext

    n, d = 1024, 128
    q, k, v, do = (t.to(device) for t in _case(4, 4, n, n, d, torch.bfloat16, seed=7)[:4])
    ref = _run(ext, q, k, v, do, causal, d ** -0.5, PATHS[path])
    for window in ((n - 1, n - 1), (n + 50, -1), (-1, n - 1), (n - 1, 3 if causal else n)):
        _bitwise(_run(ext, q, k, v, do, causal, d ** -0.5, PATHS[path], window=window), ref)


@pytest.mark.parametrize("path", ["auto", "mfma_only"])
def test_noncausal_right_bound_zero_is_the_causal_call(path, device):
    import flashattention_lab_cuda as ext

    for nq, nk in ((1024, 1024), (768, 1024)):
        q, k, v, do = (t.to(device) for t in _case(4, 4, nq, nk, 128, torch.float16, seed=nq)[:4])
        ref = _run(ext, q, k, v, do, True, 0.1, PATHS[path])
        _bitwise(_run(ext, q, k, v, do, False, 0.1, PATHS[path], window=(-1, 0)), ref)
        ref = _run(ext, q, k, v, do, True, 0.1, PATHS[path], window=(300, -1))
        _bitwise(_run(ext, q, k, v, do, False, 0.1, PATHS[path], window=(300, 0)), ref)
        _bitwise(_run(ext, q, k, v, do, True, 0.1, PATHS[path], window=(300, 7)), ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window,causal", [((300, 40), False), ((1000, 0), True), ((20, -1), True)])
def test_native_window_against_the_same_window_as_a_dense_mask(window, causal, dtype, device):
    import flashattention_lab_cuda as ext

    n, d = 1024, 128
    q, k, v, do = (t.to(device) for t in _case(4, 4, n, n, d, dtype, seed=n + window[0])[:4])
    native = _run(ext, q, k, v, do, causal, d ** -0.5, 3, window=window)
    dense = _run(ext, q, k, v, do, False, d ** -0.5, 3, mask=window_mask(n, n, causal, window).to(torch.uint8).to(device))
    tol = dtype_tolerances(dtype)
    same = []
    for x, y, name in zip(native, dense, ("o", "lse", "dq", "dk", "dv")):
        torch.testing.assert_close(x, y, **tol, msg=name)
        same.append(f"{name}={'bitwise' if torch.equal(x, y) else 'differs'}")
    print(f"window {window} causal={causal} {dtype}: native vs dense mask:", " ".join(same))


@pytest.mark.parametrize("path", ["mfma_only", "exact"])
def test_dead_rows_and_keys_are_exact_zeros(path, device):
    import flashattention_lab_cuda as ext

    for nq, nk, causal, window in ((512, 1024, True, (100, -1)), (1024, 512, False, (-1, 50)), (600, 900, False, (40, -1))):
        q, k, v, do = (t.to(device) for t in _case(2, 2, nq, nk, 64, torch.bfloat16, seed=nq + 1)[:4])
        o, lse, dq, dk, dv = _run(ext, q, k, v, do, causal, 0.125, PATHS[path], window=window)
        vis = window_mask(nq, nk, causal, window).to(device)
        dead_rows, dead_keys = ~vis.any(1), ~vis.any(0)
        assert dead_rows.any() or dead_keys.any()
        assert torch.equal(torch.isinf(lse), dead_rows.expand_as(lse)) and bool((lse[:, dead_rows] < 0).all())
        assert bool((o[:, dead_rows] == 0).all()) and bool((dq[:, dead_rows] == 0).all())
        assert bool((dk[:, dead_keys] == 0).all()) and bool((dv[:, dead_keys] == 0).all())
        assert bool((o[:, ~dead_rows].abs().sum(-1) > 0).all())


def test_windowed_dropout_is_reproducible_from_the_seed(device):
    import flashattention_lab_cuda as ext

    q, k, v, do = (t.to(device) for t in _case(4, 4, 1024, 1024, 128, torch.bfloat16, seed=99)[:4])
    kw = dict(window=(200, 10), dropout_p=0.1)
    a = _run(ext, q, k, v, do, False, 0.09, 3, seed=17, **kw)
    _bitwise(_run(ext, q, k, v, do, False, 0.09, 3, seed=17, **kw), a)
    assert not torch.equal(_run(ext, q, k, v, do, False, 0.09, 3, seed=18, **kw)[0], a[0])
    # the kept elements are oracle.dropout_keep's: with every kept probability, o is the oracle's
    rq, rk, rv, ro, rlse = _oracle(*(t.cpu() for t in (q, k, v, do)), 1, False, (200, 10), None, softmax_scale=0.09, dropout_p=0.1,
                                   seed=17)
    torch.testing.assert_close(a[0].cpu(), ro, **dtype_tolerances(torch.bfloat16))
    torch.testing.assert_close(a[2].cpu(), rq, **dtype_tolerances(torch.bfloat16))


def test_flash_attention_ex_window_size_autograd_gqa(device):
    from common.attention_ex import flash_attention_ex

    b, h, hkv, n, d = 2, 8, 2, 1024, 64
    g = torch.Generator().manual_seed(5)
    q = torch.randn((b, h, n, d), generator=g).to(torch.bfloat16)
    k = torch.randn((b, hkv, n, d), generator=g).to(torch.bfloat16)
    v = torch.randn((b, hkv, n, d), generator=g).to(torch.bfloat16)
    do = torch.randn((b, h, n, d), generator=g).to(torch.bfloat16)
    qd, kd, vd = (t.to(device).requires_grad_(True) for t in (q, k, v))
    o = flash_attention_ex(qd, kd, vd, window_size=(200, 0))
    (o * do.to(device)).sum().backward()
    assert kd.grad.shape == k.shape and vd.grad.shape == v.shape and o.shape == q.shape
    rq, rk, rv, ro, _ = _oracle(q.reshape(b * h, n, d), k.reshape(b * hkv, n, d), v.reshape(b * hkv, n, d), do.reshape(b * h, n, d),
                                h // hkv, True, (200, -1), None, softmax_scale=d ** -0.5)
    tol = dtype_tolerances(torch.bfloat16)
    torch.testing.assert_close(o.detach().cpu().reshape(b * h, n, d), ro, **tol)
    torch.testing.assert_close(qd.grad.cpu().reshape(b * h, n, d), rq, **tol)
    torch.testing.assert_close(kd.grad.cpu().reshape(b * hkv, n, d), rk, **tol)
    torch.testing.assert_close(vd.grad.cpu().reshape(b * hkv, n, d), rv, **tol)
