"""CPU: the variable-length (packed) sequence entry points (include/fa_mi355x.h, fa_ex_forward_varlen / fa_ex_backward_varlen) —
declared, exported, every host-side validation before any HIP call, the Python wrappers' checks — and a model of the kernels'
per-sequence tile ranges with the cu_seqlens clamps (csrc/fa_ex_common.h: seq_span; fa_ex_mfma_kernels.h: FEAT bit 3), checked
exhaustively on small length sets: every visible (sequence, row, key) is computed, no computed tile leaves its sequence, and
malformed offsets stay inside [0, total)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
VARLEN = ("fa_ex_forward_varlen", "fa_ex_backward_varlen", "fa_ex_backward_workspace_bytes_varlen")
OK, INVALID_ARGUMENT = 0, -1
CU = ctypes.c_void_p(16)   # a non-null cu_seqlens address: never dereferenced when validation fails


def test_header_declares_and_library_exports_the_varlen_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in VARLEN:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


BASE = dict(cu_q=CU, cu_k=CU, batch=2, hq=8, hkv=2, total_q=100, total_k=120, max_q=64, max_k=80, d=64, dtype=2, sq=512, sk=128,
            sv=128, causal=0, wl=-1, wr=-1, scale=0.125, p=0.0, seed=0)


def _args(**kw):
    a = dict(BASE, **kw)
    return [a[n] for n in ("cu_q", "cu_k", "batch", "hq", "hkv", "total_q", "total_k", "max_q", "max_k", "d", "dtype", "sq", "sk", "sv",
                           "causal", "wl", "wr", "scale", "p", "seed")]


def _fwd(lib, **kw):
    return lib.fa_ex_forward_varlen(None, None, None, None, None, *_args(**kw), None)


def _bwd(lib, **kw):
    return lib.fa_ex_backward_varlen(None, None, None, None, None, None, None, None, None, *_args(**kw), None, 0, None)


BAD = [
    (dict(batch=0), "batch"), (dict(batch=-3), "batch"),
    (dict(hq=6, hkv=4), "multiple"), (dict(hkv=0), "multiple"), (dict(hq=0), "multiple"),
    (dict(sq=8 * 64 - 1), "stride"), (dict(sk=2 * 64 - 8), "stride"), (dict(sv=64), "stride"),
    (dict(max_q=-1), "shape"), (dict(max_k=-5), "shape"), (dict(total_q=-1), "shape"), (dict(d=0), "shape"),
    (dict(cu_q=None), "cu_seqlens"), (dict(cu_k=None), "cu_seqlens"),
    (dict(wl=-2), "window"), (dict(wr=-7), "window"),
    (dict(dtype=5), "dtype"), (dict(scale=float("nan")), "NaN"), (dict(p=1.0), "dropout"), (dict(p=-0.1), "dropout"),
    (dict(batch=1 << 20, hq=1 << 10, hkv=1, max_q=1 << 4, sq=1 << 16), "2^32"),
]


@pytest.mark.parametrize("kw,msg", BAD, ids=[str(k) for k, _ in BAD])
def test_host_validation_rejects_before_any_hip_call(kw, msg):
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for call in (_fwd, _bwd):
        assert call(lib, **kw) == INVALID_ARGUMENT, (call.__name__, kw)
        assert msg.encode() in lib.fa_last_error(), lib.fa_last_error()


def test_valid_arguments_reach_the_null_pointer_check_and_empty_calls_are_no_ops():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for call in (_fwd, _bwd):
        for kw in ({}, dict(wl=0, wr=0), dict(causal=1, wl=10), dict(hkv=8, sk=512, sv=1024), dict(p=0.5)):
            assert call(lib, **kw) == INVALID_ARGUMENT and b"null" in lib.fa_last_error(), kw
        # nothing to do: no query rows (and for the backward no keys either); null cu_seqlens are fine with a zero total
        assert call(lib, total_q=0, total_k=0, cu_q=None, cu_k=None) == OK
        assert call(lib, max_q=0, max_k=0) == OK
    assert _fwd(lib, total_q=0, cu_q=None) == OK


def test_workspace_bytes():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    ws = lib.fa_ex_backward_workspace_bytes_varlen
    base = ws(8, 8, 1000, 1200, 128, 2)
    assert base == lib.fa_ex_backward_workspace_bytes(8, 1000, 1200, 128, 2)   # the row constants (heads_q, total_q)
    slab = (1200 * 8 * 128 * 2 + 255) // 256 * 256
    assert ws(8, 2, 1000, 1200, 128, 2) == base + 2 * slab                         # + the per-query-head dK / dV partials
    assert ws(8, 2, 1000, 1200, 128, 0) == base + 2 * ((1200 * 8 * 128 * 4 + 255) // 256 * 256)


def test_python_wrappers_check_shapes_and_dtypes():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_varlen

    q = torch.zeros((10, 4, 16))
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU|CUDA"):
        ext.ex_varlen_forward(q, q, q, cu, cu, 6, 6, False, 0.25)
    with pytest.raises(RuntimeError, match="GPU|CUDA"):
        ext.ex_varlen_backward(q, q, q, q, q, torch.zeros((4, 10)), cu, cu, 6, 6, False, 0.25)
    with pytest.raises(RuntimeError, match="CUDA"):
        flash_attention_varlen(q, q, q, cu, cu, 6, 6)
    with pytest.raises(RuntimeError, match="window"):
        ext.ex_varlen_forward(q, q, q, cu, cu, 6, 6, False, 0.25, window=(-3, 0))
    with pytest.raises(RuntimeError, match="window"):
        flash_attention_varlen(q, q, q, cu, cu, 6, 6, window_size=(1,))


def test_python_wrapper_argument_checks(monkeypatch):
    """The checks after the device test, run on CPU tensors that claim to be on the GPU."""
    import flashattention_lab_cuda as ext

    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    q = torch.zeros((10, 4, 16), dtype=torch.bfloat16)
    kv = torch.zeros((10, 2, 16), dtype=torch.bfloat16)
    chk = ext._varlen_common
    dims = chk("t", q, kv, kv, cu, cu, 6, 6)
    assert dims[2:] == (2, 4, 2, 10, 10, 6, 6, 16, 2, 64, 32, 32)
    with pytest.raises(RuntimeError, match="multiple"):
        chk("t", q, torch.zeros((10, 3, 16), dtype=torch.bfloat16), torch.zeros((10, 3, 16), dtype=torch.bfloat16), cu, cu, 6, 6)
    with pytest.raises(RuntimeError, match="dtype"):
        chk("t", q, kv.float(), kv.float(), cu, cu, 6, 6)
    with pytest.raises(RuntimeError, match="int32"):
        chk("t", q, kv, kv, cu.long(), cu, 6, 6)
    with pytest.raises(RuntimeError, match="int32"):
        chk("t", q, kv, kv, cu.view(1, 3), cu, 6, 6)
    with pytest.raises(RuntimeError, match="same length"):
        chk("t", q, kv, kv, cu, torch.tensor([0, 10], dtype=torch.int32), 6, 6)
    with pytest.raises(RuntimeError, match="total_q, H_q, d"):
        chk("t", q.view(10, 64), kv, kv, cu, cu, 6, 6)
    with pytest.raises(RuntimeError, match=">= 0"):
        chk("t", q, kv, kv, cu, cu, -1, 6)
    with pytest.raises(RuntimeError, match="contiguous last dim"):
        chk("t", q.transpose(1, 2).contiguous().transpose(1, 2), kv, kv, cu, cu, 6, 6)
    with pytest.raises(RuntimeError, match="adjacent"):
        chk("t", torch.zeros((10, 4, 32), dtype=torch.bfloat16)[:, :, :16], kv, kv, cu, cu, 6, 6)
    # unbind views of a (total, 3, H, d) projection: token stride 3 H d, no copy
    qkv = torch.zeros((10, 3, 4, 16), dtype=torch.bfloat16)
    qq, kk, vv = qkv.unbind(1)
    assert chk("t", qq, kk, vv, cu, cu, 6, 6)[-3:] == (192, 192, 192)
    with pytest.raises(RuntimeError, match="o must be"):
        ext.ex_varlen_backward(q, kv, kv, q[:5], q, torch.zeros((4, 10)), cu, cu, 6, 6, False, 0.25)
    with pytest.raises(RuntimeError, match="lse must be"):
        ext.ex_varlen_backward(q, kv, kv, q, q, torch.zeros((10, 4)), cu, cu, 6, 6, False, 0.25)


# ---- model of the kernels' per-sequence ranges: seq_span's clamps, then the padded grid's tiles narrowed to the sequence
def seq_span(cu, b, total, max_len):
    a = min(max(cu[b], 0), total)
    e = min(max(cu[b + 1], a), total)
    return a, min(e - a, max_len)


def _visible(nq, nk, causal):
    i = np.arange(nq)[:, None]
    j = np.arange(nk)[None, :]
    return (j <= i + nk - nq) if causal else np.ones((nq, nk), dtype=bool)


def _check_call(cu_q, cu_k, total_q, total_k, max_q, max_k, causal, wellformed):
    """Walk every workgroup of the padded grids (forward / dQ: 256 query rows, dK / dV: 256 keys) like the kernels do."""
    B = len(cu_q) - 1
    cov = np.zeros((total_q, total_k), dtype=np.int64)   # visible (row, key) pairs computed, by global token
    for b in range(B):
        sq0, lq = seq_span(cu_q, b, total_q, max_q)
        sk0, lk = seq_span(cu_k, b, total_k, max_k)
        assert 0 <= sq0 and sq0 + lq <= total_q and 0 <= sk0 and sk0 + lk <= total_k
        assert lq >= 0 and lk >= 0 and lq <= max_q and lk <= max_k
        vis = _visible(lq, lk, causal)
        for q0 in range(0, max_q, 256):   # query-on-the-lane kernels: leave when the tile starts past the sequence
            if q0 >= lq:
                continue
            rows = np.arange(q0, min(q0 + 256, lq))
            assert rows.max() < lq   # rows past lq are neither loaded (buffer range) nor stored (row < nq)
            cov[sq0 + rows[:, None], sk0 + np.arange(lk)[None, :]] += vis[rows]
        keys_done = np.zeros(lk, dtype=bool)
        for k0 in range(0, max_k, 256):   # dK / dV: every key of the sequence is written (zeros where no row sees it)
            if k0 >= lk:
                continue
            keys = np.arange(k0, min(k0 + 256, lk))
            keys_done[keys] = True
        assert keys_done.all()
    if wellformed:   # every visible (sequence, row, key) computed exactly once, nothing across sequences
        want = np.zeros_like(cov)
        for b in range(B):
            sq0, lq = cu_q[b], cu_q[b + 1] - cu_q[b]
            sk0, lk = cu_k[b], cu_k[b + 1] - cu_k[b]
            want[sq0:sq0 + lq, sk0:sk0 + lk] = _visible(lq, lk, causal)
        assert np.array_equal(cov, want)


LENS = [0, 1, 2, 255, 256, 257, 300]


@pytest.mark.parametrize("causal", [False, True])
def test_tile_ranges_cover_every_sequence_and_nothing_else(causal):
    for lens_q in itertools.product([0, 1, 257], repeat=3):
        for lens_k in ([0, 1, 257], [256, 2, 1], list(lens_q)):
            cu_q = np.concatenate([[0], np.cumsum(lens_q)]).tolist()
            cu_k = np.concatenate([[0], np.cumsum(lens_k)]).tolist()
            for extra in (0, 3, 300):
                _check_call(cu_q, cu_k, cu_q[-1], cu_k[-1], max(lens_q) + extra, max(lens_k) + extra, causal, True)
    for lens in itertools.combinations(LENS, 3):
        cu = np.concatenate([[0], np.cumsum(lens)]).tolist()
        _check_call(cu, cu, cu[-1], cu[-1], max(lens), max(lens), causal, True)


def test_malformed_offsets_stay_inside_the_packed_tensors():
    rng = np.random.default_rng(0)
    for _ in range(400):
        B = int(rng.integers(1, 6))
        total_q, total_k = int(rng.integers(0, 700)), int(rng.integers(0, 700))
        cu_q = rng.integers(-800, 1500, B + 1).tolist()
        cu_k = rng.integers(-800, 1500, B + 1).tolist()
        max_q, max_k = int(rng.integers(0, 600)), int(rng.integers(0, 600))
        _check_call(cu_q, cu_k, total_q, total_k, max_q, max_k, bool(rng.integers(0, 2)), False)
    # the extremes of int32
    big = [-(1 << 31), (1 << 31) - 1, 0, (1 << 31) - 1, -(1 << 31)]
    _check_call(big, big[::-1], 500, 300, 1 << 24, 1 << 24, True, False)
