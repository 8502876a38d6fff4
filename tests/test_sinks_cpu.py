"""CPU: attention sinks (include/fa_mi355x.h, fa_ex_*_sink) — the fp64 reference's identities (tests/sink_ref.py), the decode
combine formula as a small torch model, the entry points declared and exported, argument validation before any HIP call in the C
layer and in the Python wrappers, and the `sinks` keyword of the wrappers and public functions."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from tests import sink_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
SINK_SYMBOLS = ("fa_ex_forward_sink", "fa_ex_backward_sink", "fa_ex_forward_varlen_sink", "fa_ex_backward_varlen_sink",
                "fa_ex_forward_kvcache_sink", "fa_ex_kvcache_workspace_bytes_sink")
OK, INVALID_ARGUMENT = 0, -1
NEG_INF = float("-inf")


def _inputs(bh, bh_kv, nq, nk, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((bh, nq, d), generator=g)
    k = torch.randn((bh_kv, nk, d), generator=g)
    v = torch.randn((bh_kv, nk, d), generator=g)
    do = torch.randn((bh, nq, d), generator=g)
    return q, k, v, do


# ---- the reference's identities

@pytest.mark.parametrize("kw", [dict(), dict(window=(5, 0)), dict(softcap=3.0, dropout_p=0.2, seed=3)], ids=["plain", "window", "cap+drop"])
def test_minus_inf_sinks_are_the_reference_without_the_column(kw):
    q, k, v, do = _inputs(4, 2, 12, 9, 8, 1)
    off = torch.full((2,), NEG_INF)
    a = sr.sink_reference(q, k, v, do, off, True, 0.3, **kw)
    b = sr.sink_reference(q, k, v, do, None, True, 0.3, **kw)
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    assert torch.equal(a[5], torch.zeros(2, dtype=torch.float64)) and b[5] is None
    # Nq > Nk under the causal mask: rows 0 .. 2 see no key; o = 0, lse = -inf there without a sink
    assert torch.equal(a[0][:, :3], torch.zeros((4, 3, 8), dtype=torch.float64)) and bool((a[1][:, :3] == NEG_INF).all())


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_analytic_dsink_equals_autograd(p):
    """dsink[h] = - sum exp(sink_h - lse) * rowsum(dO * O), also under dropout: the sink column is never dropped and has dP = 0."""
    q, k, v, do = _inputs(6, 3, 10, 14, 8, 2)
    sinks = torch.tensor([0.7, NEG_INF, -2.0])
    for causal, window in ((False, (-1, -1)), (True, (4, -1))):
        o, lse, _dq, _dk, _dv, ds = sr.sink_reference(q, k, v, do, sinks, causal, 0.4, window=window, dropout_p=p, seed=11, softcap=5.0)
        term = sr.dsink_terms(o, do, lse.double(), sinks)
        want = sr.dsink_sum(term, 3)
        assert ds[1] == 0.0 and want[1] == 0.0
        torch.testing.assert_close(ds, want, rtol=1e-6, atol=1e-9)   # (lse went through float32)
        assert ds[0].abs() > 1e-3


def test_dead_rows_and_a_hand_computed_case():
    """One query, one key, d = 1: s = 0.5 * 2 * 1.5 = 1.5, sink 0.5: p = e^1.5 / (e^1.5 + e^0.5), o = 3 p, lse = log(e^1.5 + e^0.5);
    dsink = -(e^0.5 / (e^1.5 + e^0.5)) * (do * o) with do = 1."""
    q, k, v, do = torch.tensor([[[2.0]]]), torch.tensor([[[1.5]]]), torch.tensor([[[3.0]]]), torch.tensor([[[1.0]]])
    o, lse, dq, dk, dv, ds = sr.sink_reference(q, k, v, do, torch.tensor([0.5]), False, 0.5)
    z = math.exp(1.5) + math.exp(0.5)
    pk, ps = math.exp(1.5) / z, math.exp(0.5) / z
    assert abs(o.item() - 3 * pk) < 1e-12 and abs(lse.item() - math.log(z)) < 1e-6
    assert abs(ds.item() + ps * 3 * pk) < 1e-12
    assert abs(dv.item() - pk) < 1e-12 and abs(dq.item() - 0.5 * pk * (3.0 - 3 * pk) * 1.5) < 1e-12
    # no visible key: o = 0, lse = the sink, every gradient 0
    o, lse, dq, dk, dv, ds = sr.sink_reference(q, k, v, do, torch.tensor([0.5]), False, 0.5, mask=torch.zeros((1, 1), dtype=torch.uint8))
    assert o.item() == 0.0 and lse.item() == 0.5 and dq.item() == 0.0 and ds.item() == 0.0
    # huge sinks stay finite: +1e4 takes all the weight, -1e4 none
    o, lse, *_ = sr.sink_reference(q, k, v, do, torch.tensor([1e4]), False, 0.5)
    assert o.item() == 0.0 and lse.item() == 1e4
    o, lse, *_ = sr.sink_reference(q, k, v, do, torch.tensor([-1e4]), False, 0.5)
    assert o.item() == 3.0 and abs(lse.item() - 1.5) < 1e-6


# ---- the decode combine: merging per-split (O_s, lse_s) with the extra column

def _row(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g, dtype=torch.float64) * 3, torch.randn((n, d), generator=g, dtype=torch.float64)


def _partials(s, v, cuts):
    """per-split normalised outputs and lse of keys [cuts[i], cuts[i + 1]); an empty split: lse = -inf, O = garbage (NaN)"""
    po, pl = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == b:
            po.append(torch.full((v.shape[1],), float("nan"), dtype=torch.float64))
            pl.append(torch.tensor(NEG_INF, dtype=torch.float64))
        else:
            po.append(torch.softmax(s[a:b], 0) @ v[a:b])
            pl.append(torch.logsumexp(s[a:b], 0))
    return torch.stack(po), torch.stack(pl)


@pytest.mark.parametrize("cuts", [(0, 40), (0, 17, 40), (0, 0, 40), (0, 40, 40), (0, 5, 5, 23, 40), (0, 1, 2, 40)])
@pytest.mark.parametrize("sink", [0.3, -4.0, 12.0, 1e4, -1e4, NEG_INF])
def test_combine_model_matches_the_softmax_with_the_sink_column(cuts, sink):
    s, v = _row(40, 6, len(cuts))
    po, pl = _partials(s, v, cuts)
    o, lse = sr.combine_model(po, pl, sink)
    full = torch.cat([s, torch.tensor([sink], dtype=torch.float64)])
    want_o = torch.softmax(full, 0)[:40] @ v
    want_lse = torch.logsumexp(full, 0).item()
    torch.testing.assert_close(o, want_o, rtol=1e-12, atol=1e-12)
    assert abs(lse - want_lse) <= 1e-12 * max(1.0, abs(want_lse))
    assert torch.isfinite(o).all() and math.isfinite(lse)


def test_combine_model_on_an_all_empty_row():
    po = torch.full((3, 4), float("nan"), dtype=torch.float64)
    pl = torch.full((3,), NEG_INF, dtype=torch.float64)
    o, lse = sr.combine_model(po, pl, -0.75)
    assert torch.equal(o, torch.zeros(4, dtype=torch.float64)) and lse == -0.75      # o = 0, lse = the sink exactly
    o, lse = sr.combine_model(po, pl, NEG_INF)
    assert torch.equal(o, torch.zeros(4, dtype=torch.float64)) and lse == NEG_INF   # without a sink: -inf


# ---- the C layer

def test_header_declares_and_library_exports_the_sink_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in SINK_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


FAKE = 0x1000   # never dereferenced: the checks come first


def _fwd(lib, bh, sinks=FAKE, heads=4, nq=64):
    return lib.fa_ex_forward_sink(None, None, None, None, None, bh, 1, nq, 64, 128, 2, 1, 32, -1, 0.125, 0.0, None, 1, 0, sinks, heads,
                                  None, 0, None, 128, 128, 0.0, 0, None)


def _bwd(lib, bh, sinks=FAKE, heads=4, dsinks=FAKE, nq=64):
    return lib.fa_ex_backward_sink(None, None, None, None, None, None, None, None, None, bh, 1, nq, 64, 128, 2, 1, 32, -1, 0.125, 0.0,
                                   None, 1, 0, sinks, heads, dsinks, None, 0, None, 128, 128, 0.0, 0, None, 0, None)


def _vfwd(lib, hq, sinks=FAKE, heads=4, total=0):
    return lib.fa_ex_forward_varlen_sink(None, None, None, None, None, FAKE, FAKE, 2, hq, 4, total, total, total, total, 64, 2,
                                         hq * 64, 256, 256, 0, -1, -1, 0.125, 0.0, None, 0, sinks, heads, 0.0, 0, None)


def _vbwd(lib, hq, sinks=FAKE, heads=4, dsinks=FAKE, total=64):
    return lib.fa_ex_backward_varlen_sink(None, None, None, None, None, None, None, None, None, FAKE, FAKE, 2, hq, 4, total, total,
                                          total, total, 64, 2, hq * 64, 256, 256, 0, -1, -1, 0.125, 0.0, None, 0, sinks, heads, dsinks,
                                          0.0, 0, None, 0, None)


def _kv(lib, sinks=FAKE, heads=8, splits=0, ws_bytes=1 << 30):
    """B = 2, H_q = 8, H_kv = 2, Nq = 1, no append, cache_len = 64, d = 64, bf16, dense strides; null tensors"""
    return lib.fa_ex_forward_kvcache_sink(None, None, None, None, None, None, None, None, 2, 8, 2, 1, 0, 64, 64, 2, 8 * 64, 8 * 64,
                                          64 * 2 * 64, 2 * 64, 64 * 2 * 64, 2 * 64, 0, 0, 0, 0, 0, -1, -1, 0.125, 0.0, None, 0, splits,
                                          None, 0, 0, 0, 0, None, 0, None, None, None, 0, 0, 0, 0, 0, 2, None, None, 0, sinks, heads,
                                          FAKE, ws_bytes, None)


def test_invalid_sinks_are_rejected_before_any_hip_call():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    err = lib.fa_last_error
    for call in (_fwd, _bwd):
        assert call(lib, 8, sinks=FAKE + 2) == INVALID_ARGUMENT and b"4-byte aligned" in err()
        for heads in (0, -4):
            assert call(lib, 8, heads=heads) == INVALID_ARGUMENT and b"sink_heads must be >= 1" in err()
        assert call(lib, 8, heads=3) == INVALID_ARGUMENT and b"sink_heads=3 does not divide the 8 query units" in err()
        # valid sinks get past their checks to the null-pointer check
        for heads in (1, 2, 4, 8):
            assert call(lib, 8, heads=heads) == INVALID_ARGUMENT and b"null tensor pointer" in err()
        # null sinks: the score-modifier call (sink_heads is not read)
        assert call(lib, 8, sinks=None, heads=0) == INVALID_ARGUMENT and b"null tensor pointer" in err()
    assert _fwd(lib, 0) == OK and _fwd(lib, 8, nq=0) == OK     # the empty forward is a no-op
    assert _bwd(lib, 8, dsinks=None) == INVALID_ARGUMENT and b"sinks without dsinks" in err()
    assert _bwd(lib, 8, dsinks=FAKE + 1) == INVALID_ARGUMENT and b"4-byte aligned" in err()
    # packed sequences and decoding: indexed by query head
    for call in (_vfwd, _vbwd):
        assert call(lib, 8, sinks=FAKE + 3) == INVALID_ARGUMENT and b"4-byte aligned" in err()
        assert call(lib, 8, heads=0) == INVALID_ARGUMENT and b"sink_heads must be >= 1" in err()
        assert call(lib, 8, heads=3) == INVALID_ARGUMENT and b"sink_heads=3 does not divide the 8 query units" in err()
    assert _vfwd(lib, 8, heads=8) == OK                          # no token at all
    assert _vbwd(lib, 8, heads=8) == INVALID_ARGUMENT and b"null tensor pointer" in err()
    assert _vbwd(lib, 8, dsinks=None) == INVALID_ARGUMENT and b"sinks without dsinks" in err()
    assert _kv(lib, sinks=FAKE + 2) == INVALID_ARGUMENT and b"4-byte aligned" in err()
    assert _kv(lib, heads=0) == INVALID_ARGUMENT and b"sink_heads must be >= 1" in err()
    assert _kv(lib, heads=3) == INVALID_ARGUMENT and b"sink_heads=3 does not divide the 8 query units" in err()
    assert _kv(lib) == INVALID_ARGUMENT and b"null tensor pointer" in err()
    assert _kv(lib, sinks=None, heads=0) == INVALID_ARGUMENT and b"null tensor pointer" in err()


def test_a_sink_decode_call_needs_the_workspace_of_two_splits():
    """The sink joins in the combine, so one split becomes two: the sink-aware size query, and the call's own check."""
    import flashattention_lab_cuda as ext

    lib = ext._lib
    args = (2, 8, 2, 1, 64, 64)
    two = lib.fa_ex_kvcache_workspace_bytes(*args, 2)
    assert lib.fa_ex_kvcache_workspace_bytes(*args, 1) == 0 and two > 0
    assert lib.fa_ex_kvcache_workspace_bytes_sink(*args, 1) == two
    assert lib.fa_ex_kvcache_workspace_bytes_sink(*args, 2) == two
    for s in (0, 4, 7):
        assert lib.fa_ex_kvcache_workspace_bytes_sink(*args, s) == max(two, lib.fa_ex_kvcache_workspace_bytes(*args, s))
    assert lib.fa_ex_kvcache_workspace_bytes_sink(2, 8, 3, 1, 64, 64, 1) == 0          # invalid shapes: 0, as the sibling
    assert _kv(lib, splits=1, ws_bytes=two - 1) == INVALID_ARGUMENT and b"workspace of" in lib.fa_last_error()
    assert _kv(lib, splits=1, ws_bytes=two) == INVALID_ARGUMENT and b"null tensor pointer" in lib.fa_last_error()
    assert _kv(lib, sinks=None, splits=1, ws_bytes=0) == INVALID_ARGUMENT and b"null tensor pointer" in lib.fa_last_error()


# ---- the Python layers

def test_sinks_arg_rejects_bad_tensors():
    import flashattention_lab_cuda as ext

    dev = torch.device("cpu")
    assert ext.sinks_arg("t", None, dev, 8) == (0, 1, None)
    good = torch.zeros(4)
    assert ext.sinks_arg("t", good, dev, 8)[:2] == (good.data_ptr(), 4)
    assert ext.sinks_arg("t", torch.zeros(8), dev, 8)[1] == 8 and ext.sinks_arg("t", torch.zeros(1), dev, 8)[1] == 1
    assert ext.sinks_arg("t", good, dev, 8, heads=4)[1] == 4
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="sinks must be float32"):
            ext.sinks_arg("t", bad, dev, 8)
    with pytest.raises(RuntimeError, match="float32 tensor"):
        ext.sinks_arg("t", [0.0] * 4, dev, 8)
    with pytest.raises(RuntimeError, match="device"):
        ext.sinks_arg("t", good, torch.device("meta"), 8)
    for bad in (torch.zeros(3), torch.zeros(16), torch.zeros(0), torch.zeros(2, 4), torch.zeros(())):   # 3-D calls: a divisor of BH
        with pytest.raises(RuntimeError, match="sinks must be"):
            ext.sinks_arg("t", bad, dev, 8)
    for bad in (torch.zeros(2), torch.zeros(8), torch.zeros(1, 4)):                                    # heads known: exactly (H,)
        with pytest.raises(RuntimeError, match=r"sinks must be \(4,\)"):
            ext.sinks_arg("t", bad, dev, 8, heads=4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.sinks_arg("t", torch.zeros(8)[::2], dev, 8)


def test_wrappers_and_public_functions_take_the_sinks_keyword():
    """Without the feature every call below is a TypeError (unexpected keyword argument)."""
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_ex, flash_attention_varlen, flash_attn_with_kvcache

    q = torch.zeros((8, 16, 32))
    lse = torch.zeros((8, 16))
    cu = torch.zeros(2, dtype=torch.int32)
    s = torch.zeros(4)
    # (there is no CPU path: with the keyword accepted, the tensors' own check answers)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.ex_forward(q, q, q, False, 0.25, sinks=s)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.ex_backward(q, q, q, q, q, lse, False, 0.25, sinks=s)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.ex_varlen_forward(q, q, q, cu, cu, 4, 4, False, 0.25, sinks=s)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.ex_varlen_backward(q, q, q, q, q, lse, cu, cu, 4, 4, False, 0.25, sinks=s)
    q4 = torch.zeros((2, 4, 16, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        ext.ex_kvcache_forward(q4, q4, q4, sinks=s)
    with pytest.raises(RuntimeError, match="CUDA"):
        flash_attention_ex(q4, q4, q4, sinks=s)
    with pytest.raises(RuntimeError, match="CUDA"):
        flash_attention_varlen(q, q, q, cu, cu, 4, 4, sinks=s)
    with pytest.raises(RuntimeError, match="GPU"):
        flash_attn_with_kvcache(q4, q4, q4, sinks=s)
    # keyword-only, behind FlashAttention-2's positional order (which ends at return_softmax_lse); the e4m3 scales stay the
    # trailing keywords (tests/test_kvcache_fp8_cpu.py pins that)
    for fn in (flash_attn_with_kvcache, ext.ex_kvcache_forward):
        params = inspect.signature(fn).parameters
        assert params["sinks"].kind is inspect.Parameter.KEYWORD_ONLY and params["sinks"].default is None
        assert list(params)[-3:] == ["sinks", "k_descale", "v_descale"]
    params = list(inspect.signature(flash_attn_with_kvcache).parameters.values())
    assert [p.name for p in params[:5]] == ["q", "k_cache", "v_cache", "k", "v"]
    positional = [p.name for p in params if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional[-1] == "return_softmax_lse" and "sinks" not in positional
    for fn in (flash_attention_ex, flash_attention_varlen, ext.ex_forward, ext.ex_backward, ext.ex_varlen_forward, ext.ex_varlen_backward):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "sinks" and last.default is None
