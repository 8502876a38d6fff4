"""CPU: the score-modifier entry points (include/fa_mi355x.h, fa_ex_*_scoremod: FlashAttention-2's softcap and alibi_slopes) —
declared, exported, argument validation before any HIP call, the Python wrappers' checks — and the fp64 reference the GPU tests
(tests/test_scoremod_gpu.py) hold the kernels to, checked on a case small enough to work out by hand."""
import ctypes
import math
import os
import re

import pytest
import torch

from oracle import attention_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
SCOREMOD = ("fa_ex_forward_scoremod", "fa_ex_backward_scoremod", "fa_ex_forward_varlen_scoremod", "fa_ex_backward_varlen_scoremod")
OK, INVALID_ARGUMENT = 0, -1


def window_visible(nq, nk, causal, window):
    """(nq, nk) boolean of the causal flag and the window, bottom-right aligned."""
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


def scoremod_reference(q, k, v, do, causal, scale, softcap=0.0, slopes=None, window=(-1, -1), mask=None, block_mask=None, br=128,
                       bc=128, dropout_p=0.0, seed=0):
    """(o, lse, dq, dk, dv) in fp64 of q (BH, Nq, d), k, v (BH / g, Nk, d) (GQA: K / V repeated over each group), do (BH, Nq, d):
        s = scale q.k;  s' = softcap tanh(s / softcap) if softcap > 0;  s'' = s' - slope[u] |i + Nk - Nq - j| with slopes (BH,)
    P = softmax of s'' over the visible keys (oracle.extended_visible and the window), dropout by oracle.dropout_keep; a row without
    a visible key: o = 0, lse = -inf.  The slopes take no gradient."""
    bh, nq, d = q.shape
    nk = k.shape[1]
    g = bh // k.shape[0]
    qd = q.detach().cpu().double().requires_grad_(True)
    kd = k.detach().cpu().double().requires_grad_(True)
    vd = v.detach().cpu().double().requires_grad_(True)
    kr, vr = kd.repeat_interleave(g, 0), vd.repeat_interleave(g, 0)
    s = qd @ kr.transpose(1, 2) * scale
    if softcap > 0.0:
        s = softcap * torch.tanh(s / softcap)
    if slopes is not None:
        dist = (torch.arange(nq).unsqueeze(1) + (nk - nq) - torch.arange(nk).unsqueeze(0)).abs().double()
        s = s - slopes.detach().cpu().double().reshape(bh, 1, 1) * dist
    vis = orc.extended_visible(bh, nq, nk, False, None if mask is None else mask.cpu(), None if block_mask is None else block_mask.cpu(),
                               br, bc)
    vis = vis & window_visible(nq, nk, causal, window).unsqueeze(0)
    live = vis.any(-1, keepdim=True)
    sm = torch.where(vis, s, torch.tensor(float("-inf"), dtype=torch.float64))
    sm = torch.where(live, sm, torch.zeros((), dtype=torch.float64))
    p = torch.softmax(sm, -1) * live
    lse = torch.where(live.squeeze(-1), torch.logsumexp(sm, -1), torch.tensor(float("-inf"), dtype=torch.float64))
    if dropout_p > 0.0:
        keep = orc.dropout_keep(bh, nq, nk, dropout_p, seed)
        p = p * keep / (1.0 - dropout_p)
    o = p @ vr
    if do is not None:
        (o * do.detach().cpu().double()).sum().backward()
        return o.detach(), lse.detach().float(), qd.grad, kd.grad, vd.grad
    return o.detach(), lse.detach().float(), None, None, None


def test_header_declares_and_library_exports_the_scoremod_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in SCOREMOD:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


def _fwd(lib, bh, cap=0.0, slopes=None, heads=1, stride=0):
    return lib.fa_ex_forward_scoremod(None, None, None, None, None, bh, 1, 64, 64, 128, 2, 0, -1, -1, 0.125, cap, slopes, heads, stride,
                                      None, 0, None, 128, 128, 0.0, 0, None)


def _bwd(lib, bh, cap=0.0, slopes=None, heads=1, stride=0):
    return lib.fa_ex_backward_scoremod(None, None, None, None, None, None, None, None, None, bh, 1, 64, 64, 128, 2, 0, -1, -1, 0.125,
                                       cap, slopes, heads, stride, None, 0, None, 128, 128, 0.0, 0, None, 0, None)


def _vfwd(lib, batch, cap=0.0, slopes=None, stride=0):
    return lib.fa_ex_forward_varlen_scoremod(None, None, None, None, None, None, None, batch, 4, 4, 0, 0, 0, 0, 64, 2, 256, 256, 256, 0,
                                             -1, -1, 0.125, cap, slopes, stride, 0.0, 0, None)


def _vbwd(lib, batch, cap=0.0, slopes=None, stride=0):
    return lib.fa_ex_backward_varlen_scoremod(None, None, None, None, None, None, None, None, None, None, None, batch, 4, 4, 0, 0, 0, 0,
                                              64, 2, 256, 256, 256, 0, -1, -1, 0.125, cap, slopes, stride, 0.0, 0, None, 0, None)


def test_invalid_modifiers_are_rejected_before_any_hip_call():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    fake = 0x1000   # never dereferenced: the checks come first
    for call in (_fwd, _bwd):
        for cap in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert call(lib, 8, cap=cap) == INVALID_ARGUMENT, (call.__name__, cap)
            assert b"softcap" in lib.fa_last_error()
            assert call(lib, 0, cap=cap) == INVALID_ARGUMENT   # (before the empty-problem shortcut)
        assert call(lib, 8, slopes=fake, heads=0) == INVALID_ARGUMENT and b"alibi_heads" in lib.fa_last_error()
        assert call(lib, 8, slopes=fake, heads=-3) == INVALID_ARGUMENT and b"alibi_heads" in lib.fa_last_error()
        assert call(lib, 8, slopes=fake, heads=3) == INVALID_ARGUMENT and b"alibi_heads=3 does not divide BH=8" in lib.fa_last_error()
        assert call(lib, 8, slopes=fake, heads=4, stride=-1) == INVALID_ARGUMENT and b"alibi_batch_stride" in lib.fa_last_error()
        assert call(lib, 0, stride=-4) == INVALID_ARGUMENT and b"alibi_batch_stride" in lib.fa_last_error()
        # valid modifiers get past their checks to the null-pointer check; an empty problem is a no-op
        for cap, slopes, heads, stride in ((0.0, None, 1, 0), (30.0, None, 1, 0), (0.0, fake, 4, 0), (5.0, fake, 4, 4), (1.0, fake, 8, 0)):
            assert call(lib, 8, cap, slopes, heads, stride) == INVALID_ARGUMENT and b"null" in lib.fa_last_error()
            assert call(lib, 0, cap, slopes, heads, stride) == OK
        assert call(lib, 0, slopes=None, heads=0) == OK   # (alibi_heads is only read with slopes)
    for call in (_vfwd, _vbwd):
        assert call(lib, 2, cap=-2.0) == INVALID_ARGUMENT and b"softcap" in lib.fa_last_error()
        assert call(lib, 2, cap=float("nan")) == INVALID_ARGUMENT and b"softcap" in lib.fa_last_error()
        assert call(lib, 2, slopes=fake, stride=-4) == INVALID_ARGUMENT and b"alibi_batch_stride" in lib.fa_last_error()
        assert call(lib, 2, cap=50.0, slopes=fake, stride=4) == OK   # no token at all


def test_python_wrappers_reject_bad_slopes_and_softcap():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_ex, flash_attention_varlen

    q = torch.zeros((8, 16, 32))
    lse = torch.zeros((8, 16))
    for cap in (-1.0, float("nan"), float("inf"), "3", True, None):
        with pytest.raises(RuntimeError, match="softcap must be a finite number >= 0"):
            ext.ex_forward(q, q, q, False, 0.25, softcap=cap)
        with pytest.raises(RuntimeError, match="softcap"):
            ext.ex_backward(q, q, q, q, q, lse, False, 0.25, softcap=cap)
        with pytest.raises(RuntimeError, match="softcap"):
            ext.ex_varlen_forward(q, q, q, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 4, 4, False, 0.25,
                                  softcap=cap)
    # the slopes' checks run after the tensors' own (there is no CPU path): fake a device with the meta tensors' help is not
    # possible, so the helper is driven directly
    dev = torch.device("cpu")
    good = torch.zeros(8)
    assert ext.alibi_arg("t", None, dev, 8) == (0, 1, 0, None)
    assert ext.alibi_arg("t", good, dev, 8)[1:3] == (8, 0)
    assert ext.alibi_arg("t", torch.zeros(2, 4), dev, 8)[1:3] == (4, 4)
    assert ext.alibi_arg("t", torch.zeros(4).unsqueeze(0).expand(2, 4), dev, 8)[1:3] == (4, 0)
    assert ext.alibi_arg("t", torch.zeros(4), dev, 8, heads=4)[1:3] == (4, 0)
    assert ext.alibi_arg("t", torch.zeros(2, 4), dev, 8, heads=4)[1:3] == (4, 4)
    with pytest.raises(RuntimeError, match="float32"):
        ext.alibi_arg("t", torch.zeros(8, dtype=torch.float64), dev, 8)
    with pytest.raises(RuntimeError, match="float32"):
        ext.alibi_arg("t", [0.0] * 8, dev, 8)
    with pytest.raises(RuntimeError, match="device"):
        ext.alibi_arg("t", good, torch.device("meta"), 8)
    for bad in (torch.zeros(7), torch.zeros(3, 3), torch.zeros(8, 1, 1), torch.zeros(())):
        with pytest.raises(RuntimeError, match="alibi_slopes must be"):
            ext.alibi_arg("t", bad, dev, 8)
    for bad in (torch.zeros(8), torch.zeros(3, 4), torch.zeros(4, 2)):
        with pytest.raises(RuntimeError, match="alibi_slopes must be"):
            ext.alibi_arg("t", bad, dev, 8, heads=4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.alibi_arg("t", torch.zeros(16)[::2], dev, 8)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.alibi_arg("t", torch.zeros(4, 2).t(), dev, 8)
    # the autograd wrappers check the shape against q's heads before anything reaches the device
    q4 = torch.zeros((2, 4, 16, 32))
    with pytest.raises(RuntimeError, match="CUDA"):
        flash_attention_ex(q4, q4, q4, softcap=5.0, alibi_slopes=torch.zeros(4))
    with pytest.raises(RuntimeError, match="CUDA"):
        flash_attention_varlen(q, q, q, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 4, 4, softcap=1.0)


def test_reference_matches_a_hand_computed_two_key_case():
    """One query, two keys (Nq = 1, Nk = 2: coff = 1, distances |0 + 1 - j| = 1, 0), d = 1, softcap 2, slope 0.5."""
    q = torch.tensor([[[2.0]]])
    k = torch.tensor([[[1.5], [-1.0]]])
    v = torch.tensor([[[3.0], [-2.0]]])
    do = torch.tensor([[[1.0]]])
    scale, cap, slope = 0.5, 2.0, 0.5
    s = [scale * 2.0 * 1.5, scale * 2.0 * -1.0]                     # 1.5, -1.0
    t = [math.tanh(x / cap) for x in s]
    s2 = [cap * t[0] - slope * 1, cap * t[1] - slope * 0]
    lse = math.log(math.exp(s2[0]) + math.exp(s2[1]))
    p = [math.exp(x - lse) for x in s2]
    o = p[0] * 3.0 + p[1] * -2.0
    dp = [3.0, -2.0]                                                  # do . v_j
    ds = [p[j] * (dp[j] - o) * (1 - t[j] ** 2) for j in range(2)]    # delta = do . o = o
    dq = scale * (ds[0] * 1.5 + ds[1] * -1.0)
    dk = [scale * ds[0] * 2.0, scale * ds[1] * 2.0]
    ro, rlse, rdq, rdk, rdv = scoremod_reference(q, k, v, do, False, scale, softcap=cap, slopes=torch.tensor([slope]))
    assert abs(ro.item() - o) < 1e-12 and abs(rlse.item() - lse) < 1e-6
    assert abs(rdq.item() - dq) < 1e-12
    assert torch.allclose(rdk.flatten(), torch.tensor(dk, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(rdv.flatten(), torch.tensor(p, dtype=torch.float64), atol=1e-12)
    # the causal flag hides key 1 from nothing here (row 0 + coff = 1 >= both keys); with Nq = Nk = 1 ... a dead row instead:
    ro, rlse, rdq, _, _ = scoremod_reference(q, k[:, :1], v[:, :1], do, True, scale, softcap=cap, slopes=torch.tensor([slope]),
                                             window=(-1, -1), mask=torch.zeros((1, 1), dtype=torch.uint8))
    assert ro.item() == 0.0 and rlse.item() == float("-inf") and rdq.item() == 0.0
