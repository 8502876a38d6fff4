"""CPU: the sliding-window entry points (include/fa_mi355x.h, fa_ex_forward_window / fa_ex_backward_window) — declared, exported,
argument validation before any HIP call, the Python wrappers' checks — and a model of the 16-bit kernels' window tile ranges
(csrc/fa_ex_mfma_kernels.h, FEAT bit 2), checked exhaustively on small shapes: every visible element is computed, every computed tile
holds a visible element, and the per-element thresholds keep exactly the visible elements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
WINDOW = ("fa_ex_forward_window", "fa_ex_backward_window")
OK, INVALID_ARGUMENT = 0, -1


def test_header_declares_and_library_exports_the_window_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in WINDOW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


def _fwd(lib, bh, wl, wr, g=1):
    return lib.fa_ex_forward_window(None, None, None, None, None, bh, g, 64, 64, 128, 2, 0, wl, wr, 0.125, None, 0, None, 128, 128,
                                    0.0, 0, None)


def _bwd(lib, bh, wl, wr, g=1):
    return lib.fa_ex_backward_window(None, None, None, None, None, None, None, None, None, bh, g, 64, 64, 128, 2, 0, wl, wr, 0.125,
                                     None, 0, None, 128, 128, 0.0, 0, None, 0, None)


def test_windows_below_minus_one_are_invalid():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for wl, wr in ((-2, -1), (-1, -2), (-5, 3), (7, -100), (-2, -2)):
        for call in (_fwd, _bwd):
            assert call(lib, 8, wl, wr) == INVALID_ARGUMENT, (call.__name__, wl, wr)
            assert b"window" in lib.fa_last_error()
            assert call(lib, 0, wl, wr) == INVALID_ARGUMENT   # (before the empty-problem shortcut)
    # a valid window gets past the window check to the null-pointer check; an empty problem is a no-op
    for wl, wr in ((-1, -1), (0, 0), (3, -1), (-1, 5), (1000, 1000)):
        for call in (_fwd, _bwd):
            assert call(lib, 8, wl, wr) == INVALID_ARGUMENT and b"null" in lib.fa_last_error()
            assert call(lib, 0, wl, wr) == OK
            assert call(lib, 0, wl, wr, g=4) == OK


def test_python_wrappers_reject_malformed_windows():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_ex

    q = torch.zeros((2, 8, 16))
    bad = [(-2, 0), (0, -3), (1,), (1, 2, 3), "ab", 5, None, (1.5, 2), (True, 1), (0, False)]
    for w in bad:
        with pytest.raises(RuntimeError, match="window"):
            ext.ex_forward(q, q, q, False, 0.25, window=w)
        with pytest.raises(RuntimeError, match="window"):
            ext.ex_backward(q, q, q, q, q, torch.zeros((2, 8)), False, 0.25, window=w)
        with pytest.raises(RuntimeError, match="window"):
            flash_attention_ex(q, q, q, window_size=w)
    with pytest.raises(RuntimeError, match=r"window \(-2, 0\): each bound must be >= 0, or -1 for unbounded"):
        ext.ex_forward(q, q, q, False, 0.25, window=(-2, 0))
    # a well-formed window reaches the tensor checks (CPU tensors: there is no CPU path)
    with pytest.raises(RuntimeError, match="GPU|CUDA"):
        ext.ex_forward(q, q, q, False, 0.25, window=(np.int64(3), 0))
    with pytest.raises(RuntimeError, match="CUDA"):
        flash_attention_ex(q, q, q, window_size=[4, -1])


def _canon(nq, nk, causal, wl, wr):
    """fa_capi.hip: window_canon."""
    if wl >= nk - 1:
        wl = -1
    if wr >= nq - 1:
        wr = -1
    if causal and wr >= 0:
        wr = -1
    if not causal and wr == 0:
        causal, wr = True, -1
    return causal, wl, wr


def test_window_effective_follows_the_c_canonicalisation():
    import flashattention_lab_cuda as ext

    for nq, nk in ((1, 1), (5, 9), (9, 5), (64, 64)):
        for causal in (False, True):
            for wl in (-1, 0, 1, nk - 2, nk - 1, nk + 3):
                for wr in (-1, 0, 1, nq - 2, nq - 1, nq + 3):
                    if wl < -1 or wr < -1:
                        continue
                    c, l, r = _canon(nq, nk, causal, wl, wr)
                    assert ext.window_effective(nq, nk, causal, (wl, wr)) == (l >= 0 or r >= 0)
                    if not causal and wr == 0 and nq > 1:
                        assert c and r == -1   # (-1, 0) without the causal flag is the causal call


# ---- model of the tile ranges of exm_fwd_kernel / exm_dq_kernel (query on the lane) and exm_dkdv_kernel (key on the lane)
BIG = 1 << 30


def _params(nq, nk, causal, wl, wr):
    causal, wl, wr = _canon(nq, nk, causal, wl, wr)
    pwl = wl if wl >= 0 else BIG
    pwr = 0 if causal else (wr if wr >= 0 else BIG)
    return pwl, pwr


def _visible(nq, nk, pwl, pwr):
    i = np.arange(nq)[:, None]
    j = np.arange(nk)[None, :]
    c = nk - nq
    return (j >= i + c - pwl) & (j <= i + c + pwr)


def _check_query_on_lane(nq, nk, pwl, pwr, BN, KBW):
    """Forward (BN = 128, mask blocks of BN) and dQ (BN = 64, mask blocks of 32): KBW = keys per need_mask decision."""
    BM, coff = 256, nk - nq
    vis = _visible(nq, nk, pwl, pwr)
    covered = np.zeros_like(vis)
    for q0 in range(0, nq, BM):
        kend = max(0, min(nk, min(q0 + BM, nq) + coff + pwr))
        ntiles = (kend + BN - 1) // BN
        t_lo = max(0, q0 + coff - pwl) // BN
        for t in range(t_lo, ntiles):   # the workgroup's tiles: each holds a visible element of its rows
            assert vis[q0:q0 + BM, t * BN:(t + 1) * BN].any(), (q0, t)
        for w in range(8):
            r0 = q0 + 32 * w
            kend_w = max(0, min(nk, min(r0 + 32, nq) + coff + pwr)) if r0 < nq else 0
            ntiles_w = (kend_w + BN - 1) // BN
            t_lo_w = max(0, r0 + coff - pwl) // BN
            assert t_lo_w >= t_lo and ntiles_w <= ntiles
            for t in range(max(t_lo_w, t_lo), ntiles_w):
                assert vis[r0:r0 + 32, t * BN:(t + 1) * BN].any(), (q0, w, t)
                for kb0 in range(t * BN, (t + 1) * BN, KBW):
                    need = (kb0 + KBW - 1 > r0 + coff + pwr) or (kb0 + KBW > nk) or (kb0 < r0 + 31 + coff - pwl)
                    for row in range(r0, min(r0 + 32, nq)):
                        keys = np.arange(kb0, kb0 + KBW)
                        if need:
                            lim = min(row + coff + pwr, nk - 1)
                            kept = (keys <= lim) & (keys >= row + coff - pwl)
                        else:
                            kept = np.ones(KBW, dtype=bool)
                        inside = keys < nk
                        assert not kept[~inside].any()
                        assert np.array_equal(kept[inside], vis[row, keys[inside]]), (row, kb0)
                        covered[row, keys[inside]] |= kept[inside]
    assert np.array_equal(covered, vis)


def _check_key_on_lane(nq, nk, pwl, pwr):
    BK, BQ, coff = 256, 64, nk - nq
    vis = _visible(nq, nk, pwl, pwr)
    covered = np.zeros_like(vis)
    for key0 in range(0, nk, BK):
        qs_first = (max(0, key0 - coff - pwr) // BQ) * BQ
        qend = min(nq, min(key0 + BK, nk) - coff + pwl)
        ntile = (qend - qs_first + BQ - 1) // BQ if qs_first < qend else 0
        for it in range(ntile):
            r = qs_first + it * BQ
            assert vis[r:r + BQ, key0:key0 + BK].any(), (key0, it)
        for w in range(8):
            kw0 = key0 + 32 * w
            it_first = max(0, kw0 - coff - pwr) // BQ - qs_first // BQ
            it_last = min(ntile, (max(0, min(nq, min(kw0 + 32, nk) - coff + pwl)) + BQ - 1) // BQ - qs_first // BQ) if kw0 < nk else 0
            for it in range(max(0, it_first), it_last):
                qs = qs_first + it * BQ
                assert vis[qs:qs + BQ, kw0:kw0 + 32].any(), (key0, w, it)
                for rb0 in (qs, qs + 32):
                    need = (kw0 + 31 - coff - pwr > rb0) or (kw0 + 32 > nk) or (rb0 + 31 > kw0 - coff + pwl)
                    rows = np.arange(rb0, rb0 + 32)
                    for key in range(kw0, min(kw0 + 32, nk)):
                        if need:
                            kept = (rows >= key - coff - pwr) & (rows <= key - coff + pwl)
                        else:
                            kept = np.ones(32, dtype=bool)
                        inside = rows < nq
                        assert np.array_equal(kept[inside], vis[rows[inside], key]), (key, rb0)
                        covered[rows[inside], key] |= kept[inside]
    assert np.array_equal(covered, vis)


SHAPES = [(300, 300), (256, 512), (520, 260), (64, 700), (700, 64), (1, 300), (300, 1)]
WINDOWS = [(0, 0), (5, 3), (31, -1), (100, 0), (-1, 40), (255, 256), (257, -1), (-1, 0), (0, -1), (600, 17)]


@pytest.mark.parametrize("nq,nk", SHAPES)
def test_window_tile_ranges_cover_the_band_and_nothing_else(nq, nk):
    for causal in (False, True):
        for wl, wr in WINDOWS:
            pwl, pwr = _params(nq, nk, causal, wl, wr)
            _check_query_on_lane(nq, nk, pwl, pwr, 128, 128)   # forward
            _check_query_on_lane(nq, nk, pwl, pwr, 64, 32)     # dQ
            _check_key_on_lane(nq, nk, pwl, pwr)               # dK / dV
