"""GPU: grouped-query attention (fa_ex_forward_grouped / fa_ex_backward_grouped through ex_forward / ex_backward and
flash_attention_ex): k and v with B*H_kv units against q's B*H_q, query unit u reading K/V unit u // (H_q / H_kv).

The reference result is the oracle on K and V repeated over each group, with dK and dV summed over the group in fp64
(autograd through repeat_interleave).  The sharp checks hold the grouped call to the ungrouped call on the expanded K/V: the
same kernels run on the same units, so o, lse and dq must be the same bits, and dk, dv the fp32 sum of the expanded call's."""
import pytest
import torch

from oracle import attention_oracle as orc
from tests.helpers import dtype_tolerances

pytestmark = pytest.mark.gpu


def _case(b, hq, hkv, nq, nk, d, dtype, seed, mask_kind=None, block=None, density=0.6):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((b * hq, nq, d), generator=g).to(dtype)
    k = torch.randn((b * hkv, nk, d), generator=g).to(dtype)
    v = torch.randn((b * hkv, nk, d), generator=g).to(dtype)
    do = torch.randn((b * hq, nq, d), generator=g).to(dtype)
    mask = bmask = None
    if mask_kind == "shared":
        mask = (torch.rand((nq, nk), generator=g) < density).to(torch.uint8)
    elif mask_kind == "per_bh":
        mask = (torch.rand((b * hq, nq, nk), generator=g) < density).to(torch.uint8)
    if block is not None:
        br, bc = block
        bmask = (torch.rand(((nq + br - 1) // br, (nk + bc - 1) // bc), generator=g) < density).to(torch.uint8)
    return q, k, v, do, mask, bmask


def _oracle(q, k, v, do, g, **kw):
    """fp64: attention on the repeated K/V; the gradients of k and v are the fp64 sums over each group."""
    qf, kf, vf = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o, lse = orc.extended_attention(qf, kf.repeat_interleave(g, 0), vf.repeat_interleave(g, 0), **kw)
    (o * do.double()).sum().backward()
    return qf.grad.to(q.dtype), kf.grad.to(q.dtype), vf.grad.to(q.dtype), o.detach().to(q.dtype), lse.detach().float()


ORACLE_CASES = [
    # b, hq, hkv, nq, nk, d, causal, mask_kind, block, p, dtype, path
    (2, 8, 4, 300, 300, 128, False, None, None, 0.0, torch.bfloat16, "auto"),          # g = 2: the plain kernels
    (2, 8, 4, 300, 300, 128, True, None, None, 0.0, torch.float16, "auto"),
    (1, 8, 2, 256, 384, 128, True, None, None, 0.0, torch.float16, "auto"),            # g = 4, Nq != Nk
    (1, 8, 1, 200, 200, 128, True, None, None, 0.0, torch.bfloat16, "auto"),           # MQA (g = H_q = 8)
    (1, 16, 2, 257, 257, 128, True, None, None, 0.0, torch.bfloat16, "mfma_only"),     # g = 8 on the extended MFMA kernels
    (2, 4, 2, 128, 160, 128, False, "per_bh", None, 0.1, torch.bfloat16, "mfma_only"),  # dense mask + dropout
    (2, 4, 2, 130, 190, 64, True, "per_bh", None, 0.0, torch.bfloat16, "mfma_only"),    # d = 64, per-(b,h) mask alone
    (1, 8, 1, 100, 100, 40, False, None, (32, 32), 0.2, torch.float16, "mfma_only"),    # d = 40, MQA, block-sparse + dropout
    (2, 4, 1, 120, 96, 64, False, None, (32, 64), 0.0, torch.bfloat16, "mfma_only"),     # block-sparse alone
    (2, 4, 2, 90, 120, 64, False, None, None, 0.3, torch.float16, "mfma_only"),          # dropout alone
    (2, 4, 1, 70, 90, 36, True, "per_bh", (32, 64), 0.1, torch.bfloat16, "exact"),       # d = 36: everything at once
    (2, 6, 2, 65, 65, 64, False, None, None, 0.0, torch.float32, "auto"),              # fp32 square without extras: exact kernels
    (1, 8, 2, 100, 140, 128, True, "shared", None, 0.1, torch.float32, "exact"),
    (1, 8, 8, 64, 64, 32, True, None, None, 0.0, torch.bfloat16, "auto"),              # g = 1 through the same wrapper
]


@pytest.mark.parametrize("b,hq,hkv,nq,nk,d,causal,mask_kind,block,p,dtype,path", ORACLE_CASES)
def test_grouped_forward_and_backward_match_the_oracle(b, hq, hkv, nq, nk, d, causal, mask_kind, block, p, dtype, path, device):
    import flashattention_lab_cuda as ext

    g = hq // hkv
    q, k, v, do, mask, bmask = _case(b, hq, hkv, nq, nk, d, dtype, seed=11 + nq + nk + d + g, mask_kind=mask_kind, block=block)
    br, bc = block if block is not None else (128, 128)
    scale, seed = d ** -0.5, 5 + nq
    kw = dict(causal=causal, softmax_scale=scale, mask=mask, block_mask=bmask, br=br, bc=bc, dropout_p=p, seed=seed)
    rq, rk, rv, ro, rlse = _oracle(q, k, v, do, g, **kw)
    dev = lambda t: None if t is None else t.to(device)
    ext.set_option("ex_path", {"auto": 0, "mfma_only": 3, "exact": 1}[path])
    try:
        o, lse = ext.ex_forward(dev(q), dev(k), dev(v), causal, scale, dev(mask), dev(bmask), br, bc, p, seed)
        dq, dk, dv = ext.ex_backward(dev(q), dev(k), dev(v), o, dev(do), lse, causal, scale, dev(mask), dev(bmask), br, bc, p, seed)
    finally:
        ext.set_option("ex_path", 0)
    assert dk.shape == k.shape and dv.shape == v.shape and dq.shape == q.shape
    tol = dtype_tolerances(dtype)
    torch.testing.assert_close(o.cpu(), ro, **tol)
    live = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse.cpu()), live)
    torch.testing.assert_close(lse.cpu()[live], rlse[live], rtol=1e-3, atol=1e-3)
    for name, a, r in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        assert torch.isfinite(a.float()).all(), name
        torch.testing.assert_close(a.cpu(), r, **tol, msg=name)


def _run(ext, q, k, v, do, causal, scale, **kw):
    o, lse = ext.ex_forward(q, k, v, causal, scale, **kw)
    dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, causal, scale, **kw)
    return o, lse, dq, dk, dv


def _group_sum(t, g):
    """fp32 sum over each group of the expanded call's per-head gradients, member 0 first, rounded once."""
    u = t.float().reshape(-1, g, *t.shape[1:])
    acc = u[:, 0].clone()
    for m in range(1, g):
        acc += u[:, m]
    return acc.to(t.dtype)


def _assert_sharp(grouped, expanded, g):
    o, lse, dq, dk, dv = grouped
    eo, else_, edq, edk, edv = expanded
    assert torch.equal(o, eo) and torch.equal(lse, else_), "grouped forward differs from the expanded call"
    assert torch.equal(dq, edq), "grouped dq differs from the expanded call"
    for a, e in ((dk, edk), (dv, edv)):
        s = _group_sum(e, g)
        assert a.shape == s.shape
        ulp = torch.finfo(a.dtype).eps
        assert bool(((a.float() - s.float()).abs() <= ulp * s.float().abs()).all()), (a.float() - s.float()).abs().max()


# backward variants, pinned by option: each grouped call against the expanded call under the same options (matched variants)
VARIANTS = {
    "default": {},                                # hand-over where the workspace allows it (the library's default)
    "stream": {"dq": 5, "dkdv": 5},               # the one-wave-per-SIMD dQ and dK/dV kernels, no hand-over
    "eight_wave": {"dq": 8, "dkdv": 8},           # the 8-wave dQ / dK/dV kernels
    "small_grid": {"small_grid": 2, "dq": 8, "dkdv": 8},   # the 4-wave (128-row / 128-key) forms
}


# square: every variant; Nq != Nk runs the stream kernels only (with and without the hand-over)
SHARP_CASES = [(2, 32, 8, 1024, 1024, c, var) for c in (False, True) for var in VARIANTS] + \
              [(4, 16, 2, 1024, 1536, c, var) for c in (False, True) for var in ("default", "stream")]


@pytest.mark.parametrize("b,hq,hkv,nq,nk,causal,variant", SHARP_CASES)
def test_grouped_d128_runs_the_tuned_kernels_bit_for_bit(b, hq, hkv, nq, nk, causal, variant, device):
    """16-bit, d = 128, no extras: the grouped call takes the plain path's kernels (square and Nq != Nk) and reproduces the
    ungrouped call on repeat-interleaved K/V: o, lse and dq bit for bit, dk and dv as the fp32 group sum of its dk and dv."""
    import flashattention_lab_cuda as ext

    opts = VARIANTS[variant]
    g = hq // hkv
    q, k, v, do, _, _ = _case(b, hq, hkv, nq, nk, 128, torch.bfloat16, seed=7 + nk)
    q, k, v, do = (t.to(device) for t in (q, k, v, do))
    scale = 128 ** -0.5
    for name, val in opts.items():
        ext.set_option(name, val)
    try:
        ext.profile_enable(True)
        grouped = _run(ext, q, k, v, do, causal, scale)
        torch.cuda.synchronize()
        prof = ext.profile_report()
        ext.profile_enable(False)
        expanded = _run(ext, q, k.repeat_interleave(g, 0), v.repeat_interleave(g, 0), do, causal, scale)
    finally:
        for name in opts:
            ext.set_option(name, 0)
        ext.profile_enable(False)
    assert "fwd_mfma" in prof and "ex_fwd" not in prof and "ex_bwd" not in prof, prof
    assert prof["kv_group_sum"][0] == 1, prof
    _assert_sharp(grouped, expanded, g)
    ext.release_workspace()


def test_grouped_extended_kernels_match_the_expanded_call(device):
    """The same on the extended MFMA kernels (a mask and dropout) and on the exact-f32 kernels."""
    import flashattention_lab_cuda as ext

    for dtype, path, d in ((torch.bfloat16, 3, 64), (torch.float16, 3, 128), (torch.bfloat16, 1, 72)):
        b, hq, hkv, nq, nk = 2, 8, 2, 200, 260
        g = hq // hkv
        q, k, v, do, mask, bmask = _case(b, hq, hkv, nq, nk, d, dtype, seed=3 + d, mask_kind="per_bh", block=(32, 64))
        q, k, v, do, mask, bmask = (t.to(device) for t in (q, k, v, do, mask, bmask))
        kw = dict(mask=mask, block_mask=bmask, br=32, bc=64, dropout_p=0.15, seed=42)
        ext.set_option("ex_path", path)
        try:
            grouped = _run(ext, q, k, v, do, True, d ** -0.5, **kw)
            expanded = _run(ext, q, k.repeat_interleave(g, 0), v.repeat_interleave(g, 0), do, True, d ** -0.5, **kw)
        finally:
            ext.set_option("ex_path", 0)
        _assert_sharp(grouped, expanded, g)


def test_grouped_handover_in_chunks_of_whole_groups(device):
    """A dS bound of 1 MiB fits 8 units of 128 KiB: chunks of 8 ungrouped, rounded down to 6 for groups of 3 (8 is not a
    multiple of 3), so a chunk that started inside a group would read the wrong K/V unit."""
    import flashattention_lab_cuda as ext

    b, hq, hkv, n, d = 2, 12, 4, 256, 128
    g = hq // hkv
    q, k, v, do, _, _ = _case(b, hq, hkv, n, n, d, torch.bfloat16, seed=21)
    q, k, v, do = (t.to(device) for t in (q, k, v, do))
    scale = d ** -0.5
    ext.set_option("ds_chunk_mb", 1)
    try:
        o, lse = ext.ex_forward(q, k, v, False, scale)
        ext.profile_enable(True)
        dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, False, scale)
        torch.cuda.synchronize()
        prof = ext.profile_report()
        ext.profile_enable(False)
        ke, ve = k.repeat_interleave(g, 0), v.repeat_interleave(g, 0)
        eo, else_ = ext.ex_forward(q, ke, ve, False, scale)
        edq, edk, edv = ext.ex_backward(q, ke, ve, eo, do, else_, False, scale)
    finally:
        ext.set_option("ds_chunk_mb", 0)
        ext.profile_enable(False)
    assert prof["bwd_mfma"][0] == 4 and prof["bwd_dq_mfma"][0] == 4, prof   # 24 units in chunks of 6
    _assert_sharp((o, lse, dq, dk, dv), (eo, else_, edq, edk, edv), g)
    rq, rk, rv, _, _ = _oracle(q.cpu(), k.cpu(), v.cpu(), do.cpu(), g, softmax_scale=scale)
    tol = dtype_tolerances(torch.bfloat16)
    for a, r in ((dq, rq), (dk, rk), (dv, rv)):
        torch.testing.assert_close(a.cpu(), r, **tol)
    ext.release_workspace()


@pytest.mark.parametrize("path", [0, 3, 1])
def test_grouped_backward_is_deterministic(path, device):
    import flashattention_lab_cuda as ext

    b, hq, hkv, n, d = 2, 16, 1, 512, 128
    q, k, v, do, _, _ = _case(b, hq, hkv, n, n, d, torch.bfloat16, seed=9)
    q, k, v, do = (t.to(device) for t in (q, k, v, do))
    ext.set_option("ex_path", path)
    try:
        o, lse = ext.ex_forward(q, k, v, True, 0.09)
        one = ext.ex_backward(q, k, v, o, do, lse, True, 0.09)
        two = ext.ex_backward(q, k, v, o, do, lse, True, 0.09)
    finally:
        ext.set_option("ex_path", 0)
    for a, c in zip(one, two):
        assert torch.equal(a, c)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grouped_empty_sides(dtype, device):
    import flashattention_lab_cuda as ext

    b, hq, hkv, d = 2, 8, 2, 64
    # Nq = 0: dk = dv = 0, shaped like k
    q = torch.randn((b * hq, 0, d), dtype=dtype, device=device)
    k = torch.randn((b * hkv, 50, d), dtype=dtype, device=device)
    v = torch.randn((b * hkv, 50, d), dtype=dtype, device=device)
    o, lse = ext.ex_forward(q, k, v, False, 0.1)
    dq, dk, dv = ext.ex_backward(q, k, v, o, q.clone(), lse, False, 0.1)
    assert dk.shape == k.shape and dv.shape == v.shape and dq.shape == q.shape
    assert not dk.any() and not dv.any()
    # Nk = 0: o = 0, lse = -inf, dq = 0
    q = torch.randn((b * hq, 30, d), dtype=dtype, device=device)
    k = torch.randn((b * hkv, 0, d), dtype=dtype, device=device)
    o, lse = ext.ex_forward(q, k, k.clone(), False, 0.1)
    assert not o.any() and bool(torch.isneginf(lse).all())
    dq, dk, dv = ext.ex_backward(q, k, k.clone(), o, torch.randn_like(q), lse, False, 0.1)
    assert not dq.any() and dk.shape == k.shape and dv.shape == k.shape


@pytest.mark.parametrize("causal,dtype", [(False, torch.bfloat16), (True, torch.float16), (True, torch.float32)])
def test_flash_attention_ex_with_4d_gqa_tensors(causal, dtype, device):
    """(B, H_q, N, d) against (B, H_kv, N, d): the same o and q/k/v gradients as the call on repeat-interleaved heads through
    torch autograd; a (B, H_q, Nq, Nk) mask still broadcasts against q's heads."""
    from common.attention_ex import flash_attention_ex

    b, hq, hkv, nq, nk, d = 2, 8, 2, 96, 130, 64
    g = hq // hkv
    gen = torch.Generator().manual_seed(4)
    q0 = torch.randn((b, hq, nq, d), generator=gen).to(dtype)
    k0 = torch.randn((b, hkv, nk, d), generator=gen).to(dtype)
    v0 = torch.randn((b, hkv, nk, d), generator=gen).to(dtype)
    do = torch.randn((b, hq, nq, d), generator=gen).to(dtype).to(device)
    mask = (torch.rand((b, hq, nq, nk), generator=gen) < 0.7).to(device)
    leaves = [t.to(device).requires_grad_(True) for t in (q0, k0, v0)]
    o = flash_attention_ex(*leaves, mask=mask, causal=causal, dropout_p=0.1, seed=3)
    assert o.shape == q0.shape
    (o * do).sum().backward()
    ref = [t.to(device).requires_grad_(True) for t in (q0, k0, v0)]
    ro = flash_attention_ex(ref[0], ref[1].repeat_interleave(g, 1), ref[2].repeat_interleave(g, 1), mask=mask, causal=causal,
                            dropout_p=0.1, seed=3)
    (ro * do).sum().backward()
    tol = dtype_tolerances(dtype)
    torch.testing.assert_close(o, ro, **tol)
    for a, r in zip(leaves, ref):
        assert a.grad.shape == a.shape
        torch.testing.assert_close(a.grad, r.grad, **tol)


def test_head_counts_that_do_not_group_are_refused(device):
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_ex

    q = torch.randn((2, 6, 16, 32), device=device)
    k = torch.randn((2, 4, 16, 32), device=device)
    with pytest.raises(RuntimeError):
        flash_attention_ex(q, k, k.clone())
    with pytest.raises(RuntimeError):
        ext.ex_forward(q.reshape(12, 16, 32), k.reshape(8, 16, 32), k.reshape(8, 16, 32), False, 0.1)
    with pytest.raises(RuntimeError):   # k and v must still agree
        ext.ex_forward(q.reshape(12, 16, 32), k.reshape(8, 16, 32)[:4], k.reshape(8, 16, 32)[:6], False, 0.1)
    o, lse = ext.ex_forward(q.reshape(12, 16, 32), k.reshape(8, 16, 32)[:4], k.reshape(8, 16, 32)[:4], False, 0.1)   # g = 3
    with pytest.raises(RuntimeError):
        ext.ex_backward(q.reshape(12, 16, 32), k.reshape(8, 16, 32)[:4], k.reshape(8, 16, 32)[:4], o, o, lse[:6], False, 0.1)
