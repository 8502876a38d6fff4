"""CPU: KV-cache decoding with split-KV (include/fa_mi355x.h: fa_ex_forward_kvcache, fa_ex_kvcache_workspace_bytes) — declared,
exported, every host-side validation before any HIP call, the workspace formula, the Python wrappers' checks — and models of the
device split rule (csrc/fa_decode.hip: kv_split_range) and of the combine, checked exhaustively on small shapes."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_ex_forward_kvcache", "fa_ex_kvcache_workspace_bytes")
OK, INVALID_ARGUMENT = 0, -1
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails


def test_header_declares_and_library_exports_the_kvcache_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


# B = 2, H_q = 8, H_kv = 2, Nq = 1, N_new = 1, cache_len = 64, d = 64, bf16; dense strides
BASE = dict(q=P, kc=P, vc=P, kn=P, vn=P, seqlens=P, o=P, lse=P, b=2, hq=8, hkv=2, nq=1, nnew=1, cap=64, d=64, dtype=2,
            qb=512, qt=512, kcb=64 * 128, kct=128, vcb=64 * 128, vct=128, knb=128, knt=128, vnb=128, vnt=128,
            causal=0, wl=-1, wr=-1, scale=0.125, softcap=0.0, alibi=None, abs_=0, splits=1, ws=None, wsb=0)
ORDER = ("q", "kc", "vc", "kn", "vn", "seqlens", "o", "lse", "b", "hq", "hkv", "nq", "nnew", "cap", "d", "dtype", "qb", "qt", "kcb",
         "kct", "vcb", "vct", "knb", "knt", "vnb", "vnt", "causal", "wl", "wr", "scale", "softcap", "alibi", "abs_", "splits", "ws", "wsb")


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **kw)
    rc = ext._lib.fa_ex_forward_kvcache(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


BAD = [
    (dict(dtype=0), "dtype"), (dict(dtype=7), "dtype"),
    (dict(d=4), "head_dim"), (dict(d=60), "head_dim"), (dict(d=264), "head_dim"),
    (dict(hq=7), "multiple"), (dict(hkv=0), "multiple"), (dict(hq=0), "multiple"),
    (dict(nq=0), "seqlen_q"), (dict(nnew=-1), "seqlen_new"), (dict(nnew=65), "seqlen_new"),
    (dict(qt=504), "strides of q"), (dict(qb=256), "strides of q"), (dict(kct=64), "strides of k_cache"),
    (dict(vcb=63 * 128), "strides of v_cache"), (dict(knt=64), "strides of k_new"), (dict(vnb=8), "strides of v_new"),
    (dict(seqlens=None), "needs cache_seqlens"), (dict(kn=None), "needs cache_seqlens"), (dict(vn=None), "needs cache_seqlens"),
    (dict(wl=-2), "window"), (dict(wr=-5), "window"),
    (dict(scale=float("nan")), "softmax_scale"), (dict(scale=float("inf")), "softmax_scale"),
    (dict(softcap=float("inf")), "softcap"), (dict(softcap=-1.0), "softcap"), (dict(softcap=float("nan")), "softcap"),
    (dict(splits=-1), "num_splits"), (dict(splits=257), "num_splits"),
    (dict(splits=4, ws=P, wsb=10), "workspace"), (dict(splits=4), "workspace"),
    (dict(q=None), "null"), (dict(kc=None), "null"), (dict(vc=None), "null"), (dict(o=None), "null"), (dict(lse=None), "null"),
]


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_invalid_arguments_are_rejected_before_any_hip_call(kw, what):
    rc, msg = _call(**kw)   # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == INVALID_ARGUMENT, (kw, msg)
    assert what in msg, (kw, msg)


def test_valid_arguments_reach_the_null_pointer_check():
    rc, msg = _call(o=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg
    # without new tokens k_new / v_new / cache_seqlens may be null and their strides are not checked
    rc, msg = _call(nnew=0, kn=None, vn=None, seqlens=None, knb=0, knt=0, vnb=0, vnt=0, lse=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg
    # unbound (B, L, 2, H, d) views: token stride 2 H d, batch stride L 2 H d
    rc, msg = _call(kct=256, kcb=64 * 256, vct=256, vcb=64 * 256, q=None)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg


def test_too_many_rows_to_combine_is_rejected():
    # B * H_q * Nq = 65 * 64 * 16383 >= 2^26 rows: fine with one split (no combine), refused with two
    big = dict(b=65, hq=64, hkv=1, nq=16383, nnew=0, kn=None, vn=None, seqlens=None, knb=0, knt=0, vnb=0, vnt=0, qt=4096,
               qb=16383 * 4096, kcb=64 * 64, kct=64, vcb=64 * 64, vct=64, q=None)
    rc, msg = _call(**big, splits=2)
    assert rc == -2 and "too many to combine" in msg, msg
    rc, msg = _call(**big, splits=1)
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg


def test_window_bounds_of_any_size_reach_the_null_pointer_check():
    for wl, wr in ((2 ** 32, -1), (-1, 2 ** 31 - 1), (2 ** 63 - 1, 2 ** 63 - 1), (63, 0)):
        rc, msg = _call(wl=wl, wr=wr, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg


def _ws_model(b, hq, nq, d, s):
    if s <= 1:
        return 0
    rows = b * hq * nq * s
    r256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    return r256(rows * d * 4) + r256(rows * 4)


def test_workspace_bytes_formula():
    import flashattention_lab_cuda as ext

    f = ext._lib.fa_ex_kvcache_workspace_bytes
    for b, hq, hkv, nq, cap, d, s in itertools.product((1, 3), (8, 32), (1, 8), (1, 5), (100, 32768), (64, 96), (1, 2, 7, 256)):
        assert f(b, hq, hkv, nq, cap, d, s) == _ws_model(b, hq, nq, d, s)
    assert f(4, 32, 8, 1, 1024, 128, 1) == 0
    # num_splits = 0: the library's rule, from shapes only; one key tile per cache never splits
    assert f(1, 8, 8, 1, 32, 128, 0) == 0
    assert f(1, 32, 8, 1, 32768, 128, 0) > 0
    assert f(0, 8, 8, 1, 100, 64, 2) == 0 and f(1, 8, 3, 1, 100, 64, 2) == 0 and f(1, 8, 8, 1, 100, 64, 300) == 0


def test_python_wrapper_rejections():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    q = torch.zeros((1, 1, 4, 64), dtype=torch.bfloat16)
    kc = torch.zeros((1, 16, 2, 64), dtype=torch.bfloat16)
    for name in ("rotary_cos", "rotary_sin", "cache_batch_idx", "cache_leftpad", "block_table"):
        with pytest.raises(NotImplementedError, match=name):
            flash_attn_with_kvcache(q, kc, kc, **{name: torch.zeros(1)})

    class FakeCuda(torch.Tensor):   # the wrapper's checks run before anything touches the device
        @property
        def is_cuda(self):
            return True

    fq = q.as_subclass(FakeCuda)
    fk = kc.as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="16-bit"):
        ext.ex_kvcache_forward(q.float().as_subclass(FakeCuda), kc.float().as_subclass(FakeCuda), kc.float().as_subclass(FakeCuda))
    odd_q = torch.zeros((1, 1, 4, 60), dtype=torch.bfloat16).as_subclass(FakeCuda)
    odd_k = torch.zeros((1, 16, 2, 60), dtype=torch.bfloat16).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.ex_kvcache_forward(odd_q, odd_k, odd_k)
    strided = torch.zeros((1, 16, 2, 128), dtype=torch.bfloat16)[..., ::2].as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="never copied"):
        ext.ex_kvcache_forward(fq, strided, fk)
    heads_apart = torch.zeros((1, 16, 64, 2), dtype=torch.bfloat16).transpose(2, 3).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="never copied"):
        ext.ex_kvcache_forward(fq, fk, heads_apart)


# ---- model of kv_split_range (csrc/fa_decode.hip)
KT = 32
NONE = 1 << 30


def split_range(lk, nq, qlo, qhi, causal, wl, wr, s, S):
    wl = wl if wl >= 0 else NONE
    wr = 0 if causal else (wr if wr >= 0 else NONE)
    coff = lk - nq
    lo, hi = max(0, qlo + coff - wl), min(lk, qhi + coff + wr + 1)
    nt = (hi - lo + KT - 1) // KT if hi > lo else 0
    t0, t1 = s * nt // S, (s + 1) * nt // S
    return lo + t0 * KT, min(hi, lo + t1 * KT)


def visible(lk, nq, i, j, causal, wl, wr):
    diag = i + lk - nq
    return 0 <= j < lk and (not causal or j <= diag) and (wl < 0 or j >= diag - wl) and (wr < 0 or j <= diag + wr)


def test_split_rule_partitions_the_visible_band():
    for lk, nq, S, causal, (wl, wr) in itertools.product((0, 1, 31, 32, 33, 95, 200), (1, 2, 5), (1, 2, 3, 7, 16),
                                                        (False, True), ((-1, -1), (0, 0), (3, -1), (-1, 2), (40, 5))):
        for qlo, qhi in ((a, b) for a in range(nq) for b in range(a, nq)):   # every row tile's token range
            band = {j for i in range(qlo, qhi + 1) for j in range(lk) if visible(lk, nq, i, j, causal, wl, wr)}
            spans = [split_range(lk, nq, qlo, qhi, causal, wl, wr, s, S) for s in range(S)]
            covered = []
            for a, b in spans:
                if a < b:   # a split the kernel's key loop enters: only keys some row of the tile sees
                    assert set(range(a, b)) <= band
                    covered.extend(range(a, b))
                # else: empty (a >= b) — the loop does not run, the split writes lse = -inf, the combine gives it weight 0
            assert len(covered) == len(set(covered)), "splits overlap"
            assert set(covered) == band, "the splits together are not exactly the visible band"
            nonempty = [b - a for a, b in spans if a < b]
            assert len(nonempty) == min(S, -(-len(band) // KT))
            assert not nonempty or max(nonempty) - min(nonempty) <= KT


# ---- model of the split kernel's row packing (csrc/fa_decode_kernels.h: pr0, qlo, qhi, qi, h) for any G = H_q / H_kv: row
# pr = token * G + head in the group, 16 rows a tile.  G need not divide 16 (a tile then starts in the middle of a token) and may
# exceed it (one token's heads then span several tiles).
ROWS = 16


def tile_tokens(rt, g, nq):
    """(qlo, qhi): the first and last query token with a row in row tile rt; None when the tile lies past the G * nq rows"""
    rows, pr0 = g * nq, ROWS * rt
    if pr0 >= rows:
        return None
    return pr0 // g, (min(pr0 + ROWS, rows) - 1) // g


def tile_rows(rt, g, nq):
    """[(token, head in the group)] of the valid lanes of row tile rt, in lane order"""
    return [(pr // g, pr % g) for pr in range(ROWS * rt, min(ROWS * rt + ROWS, g * nq))]


def row_band(lk, nq, i, causal, wl, wr):
    return {j for j in range(lk) if visible(lk, nq, i, j, causal, wl, wr)}


def check_group_arithmetic(g, nq, lk, causal, wl, wr, S):
    """every (token, head) row is in exactly one tile, and over that tile's splits the keys [kbeg, kend) cut to the row's band
    (the kernel's rlo / rhi) are the row's band, each key once"""
    seen = []
    for rt in range((g * nq + ROWS - 1) // ROWS):
        qlo, qhi = tile_tokens(rt, g, nq)
        rows = tile_rows(rt, g, nq)
        assert {t for t, _ in rows} == set(range(qlo, qhi + 1)), "qlo / qhi are not the tile's tokens"
        seen.extend(rows)
        spans = [split_range(lk, nq, qlo, qhi, causal, wl, wr, s, S) for s in range(S)]
        for i in sorted({t for t, _ in rows}):
            band = row_band(lk, nq, i, causal, wl, wr)
            got = [j for a, b in spans if a < b for j in range(a, b) if j in band]
            assert len(got) == len(set(got)), "a key of the row's band is in two splits"
            assert set(got) == band, (g, nq, lk, causal, wl, wr, S, rt, i)
    assert tile_tokens((g * nq + ROWS - 1) // ROWS, g, nq) is None
    assert sorted(seen) == [(t, h) for t in range(nq) for h in range(g)] and len(seen) == len(set(seen))


def test_group_arithmetic_for_any_group_size():
    for g, nq in itertools.product((1, 3, 5, 6, 8, 12, 16, 17, 20, 32), (1, 2, 3, 7, 18)):
        for lk, S, causal, (wl, wr) in itertools.product((0, 1, 33, 100), (1, 2, 5), (False, True), ((-1, -1), (5, 0), (40, 2), (33, -1))):
            check_group_arithmetic(g, nq, lk, causal, wl, wr, S)


def combine(parts):
    """the kv_combine_kernel merge: parts = [(o_s (rows, d), lse_s (rows,))] in split order"""
    los = np.stack([l for _, l in parts])
    m = los.max(0)
    o = np.zeros_like(parts[0][0])
    tot = np.zeros_like(m)
    for o_s, l_s in parts:
        w = np.where(np.isneginf(l_s), 0.0, np.exp(np.where(np.isneginf(l_s), 0.0, l_s - np.where(np.isneginf(m), 0.0, m))))
        tot += w
        o += w[:, None] * np.nan_to_num(o_s)
    live = tot > 0
    o = np.where(live[:, None], o / np.where(live, tot, 1.0)[:, None], 0.0)
    lse = np.where(live, m + np.log(np.where(live, tot, 1.0)), -np.inf)
    return o, lse


def test_combine_model_matches_one_shot_softmax():
    rng = np.random.default_rng(0)
    for S, n, dead in itertools.product((1, 2, 5), (7, 64), (False, True)):
        s = rng.standard_normal((3, n)) * 3
        v = rng.standard_normal((n, 4))
        if dead:
            s[1] = -np.inf          # a row without any visible key
        s[2, : n // 2] = -np.inf     # splits that are all -inf for this row
        cuts = np.linspace(0, n, S + 1).astype(int)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ss = s[:, a:b]
            with np.errstate(invalid="ignore", divide="ignore"):
                m = ss.max(1, initial=-np.inf)
                e = np.exp(ss - np.where(np.isneginf(m), 0.0, m)[:, None])
                l = e.sum(1)
                o_s = np.where(l[:, None] > 0, e @ v[a:b] / np.where(l > 0, l, 1)[:, None], np.nan)   # empty: garbage, never read
                lse_s = np.where(l > 0, m + np.log(np.where(l > 0, l, 1)), -np.inf)
            parts.append((o_s, lse_s))
        o, lse = combine(parts)
        with np.errstate(divide="ignore", invalid="ignore"):
            mm = s.max(1)
            ref_l = np.where(np.isneginf(mm), -np.inf, mm + np.log(np.exp(s - np.where(np.isneginf(mm), 0, mm)[:, None]).sum(1)))
            p = np.where(np.isneginf(ref_l)[:, None], 0.0, np.exp(s - np.where(np.isneginf(ref_l), 0, ref_l)[:, None]))
        assert not np.isnan(o).any()
        np.testing.assert_allclose(o, p @ v, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(np.isneginf(lse), np.isneginf(ref_l))
        fin = np.isfinite(ref_l)
        np.testing.assert_allclose(lse[fin], ref_l[fin], rtol=1e-12)
        assert math.isinf(lse[1]) == dead
