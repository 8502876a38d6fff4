"""CPU: the differentiable lse and the merge of partial attention results (include/fa_mi355x.h: fa_ex_backward_dlse,
fa_ex_backward_varlen_dlse, fa_merge_states, fa_merge_states_backward; common/merge_states.py).  The fp64 references of
tests/merge_ref.py against torch.autograd — merged key chunks are the full call in o, lse and every gradient — the declarations,
exports and signature groups, the C layer's validation before any HIP call, and the shim's and wrappers' errors."""
import ctypes
import os
import re

import pytest
import torch

from tests import merge_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
INVALID_ARGUMENT, UNSUPPORTED = -1, -2
NEW_SYMBOLS = ("fa_ex_backward_dlse", "fa_ex_backward_varlen_dlse", "fa_merge_states", "fa_merge_states_backward")
TOL = dict(rtol=1e-12, atol=1e-12)


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------- the maths, fp64

# (causal, Nq, Nk, split, GQA group, sinks): the split is no tile multiple; causal Nq = Nk leaves chunk b rows without a key
CHUNK_CASES = [(False, 24, 40, 17, 1, False), (True, 40, 40, 17, 1, False), (True, 9, 40, 17, 2, False), (False, 24, 40, 17, 2, True),
               (True, 40, 40, 17, 1, True)]


@pytest.mark.parametrize("causal,nq,nk,split,g,with_sinks", CHUNK_CASES)
def test_merged_chunks_are_the_full_call_in_o_lse_and_every_gradient(causal, nq, nk, split, g, with_sinks):
    bh, d, scale = 4, 8, 0.3
    q, k, v = _rand(bh, nq, d, seed=1), _rand(bh // g, nk, d, seed=2), _rand(bh // g, nk, d, seed=3)
    do, dlse = _rand(bh, nq, d, seed=4), _rand(bh, nq, seed=5)
    sinks = _rand(2, seed=6) if with_sinks else None
    o_f, lse_f, dq_f, dk_f, dv_f, ds_f = ref.attention_grads(q, k, v, do, dlse, sinks, causal, scale)

    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    sd = None if sinks is None else sinks.clone().requires_grad_(True)
    # the chunk rule: keys[:split] is causal=False with window (-1, Nk - split); the last chunk is plain causal; sinks on one chunk
    wa = (-1, nk - split) if causal else (-1, -1)
    o_a, lse_a = ref.attention(qd, kd[:, :split], vd[:, :split], sd, False, scale, window=wa)
    o_b, lse_b = ref.attention(qd, kd[:, split:], vd[:, split:], None, causal, scale)
    if causal and nq == nk:
        assert (lse_b[:, : split] == ref.NEG_INF).all()          # chunk b's first rows see none of its keys
    o, lse = ref.merge(o_a, lse_a, o_b, lse_b)
    torch.testing.assert_close(o, o_f, **TOL)
    torch.testing.assert_close(lse, lse_f, **TOL)
    ((o * do).sum() + ref.lse_loss(lse, dlse)).backward()
    torch.testing.assert_close(qd.grad, dq_f, **TOL)
    torch.testing.assert_close(kd.grad, dk_f, **TOL)
    torch.testing.assert_close(vd.grad, dv_f, **TOL)
    if with_sinks:
        torch.testing.assert_close(sd.grad, ds_f, **TOL)


@pytest.mark.parametrize("causal,nq,nk,g,with_sinks,window", [(False, 24, 40, 1, False, (-1, -1)), (True, 40, 24, 2, True, (-1, -1)),
                                                               (True, 24, 40, 1, True, (9, -1)), (False, 24, 40, 2, False, (5, 3))])
def test_closed_form_dlse_backward_is_autograd(causal, nq, nk, g, with_sinks, window):
    """dS = P (dP - delta + dlse), dV unchanged, dsinks from the same row constant; rows at lse = -inf ignore a NaN dlse"""
    bh, d, scale = 4, 8, 0.3
    q, k, v = _rand(bh, nq, d, seed=1), _rand(bh // g, nk, d, seed=2), _rand(bh // g, nk, d, seed=3)
    do, dlse = _rand(bh, nq, d, seed=4), _rand(bh, nq, seed=5)
    sinks = _rand(2, seed=6) if with_sinks else None
    if sinks is not None:
        sinks[1] = ref.NEG_INF
    _o, lse, dq, dk, dv, ds = ref.attention_grads(q, k, v, do, dlse, sinks, causal, scale, window=window)
    dlse = torch.where(torch.isfinite(lse), dlse, torch.full_like(dlse, float("nan")))
    if causal and nq > nk:
        assert torch.isnan(dlse).any()
    cq, ck, cv, cs = ref.closed_form_backward(q, k, v, do, dlse, sinks, causal, scale, window=window)
    for a, b in ((cq, dq), (ck, dk), (cv, dv)):
        torch.testing.assert_close(a, b, **TOL)
    if with_sinks:
        torch.testing.assert_close(cs, ds, **TOL)
    # dv does not depend on dlse
    torch.testing.assert_close(ref.closed_form_backward(q, k, v, do, None, sinks, causal, scale, window=window)[2], cv, **TOL)


def _merge_inputs(rows=11, d=8):
    o_a, o_b = _rand(3, rows, d, seed=1), _rand(3, rows, d, seed=2)
    lse_a, lse_b = 3 * _rand(3, rows, seed=3), 3 * _rand(3, rows, seed=4)
    lse_a[:, 0] = ref.NEG_INF                       # a dead, b dead, both dead; the dead side's o is NaN
    lse_b[:, 1] = ref.NEG_INF
    lse_a[:, 2] = lse_b[:, 2] = ref.NEG_INF
    lse_b[:, 3] = lse_a[:, 3] - 800.0               # exp underflows: weight exactly 0
    o_a[:, 0] = o_b[:, 1] = o_a[:, 2] = o_b[:, 2] = o_b[:, 3] = float("nan")
    return o_a, lse_a, o_b, lse_b


def test_merge_and_its_closed_form_backward_with_infinite_rows():
    o_a, lse_a, o_b, lse_b = _merge_inputs()
    do, dlse = _rand(*o_a.shape, seed=5), _rand(*lse_a.shape, seed=6)
    o, lse = ref.merge(o_a, lse_a, o_b, lse_b)
    assert torch.isfinite(o).all()
    assert torch.equal(o[:, 0], o_b[:, 0]) and torch.equal(o[:, 1], o_a[:, 1]) and torch.equal(o[:, 3], o_a[:, 3])
    assert torch.equal(lse[:, 0], lse_b[:, 0]) and torch.equal(lse[:, 1], lse_a[:, 1])
    assert (o[:, 2] == 0).all() and (lse[:, 2] == ref.NEG_INF).all()
    live = torch.isfinite(lse_a) & torch.isfinite(lse_b)
    torch.testing.assert_close(lse[live], torch.logaddexp(lse_a, lse_b)[live], **TOL)
    # autograd through the differentiable form, NaN replaced where the side is dead (autograd would carry 0 * NaN)
    ta, tb = (torch.nan_to_num(t, nan=0.0).requires_grad_(True) for t in (o_a, o_b))
    la, lb = lse_a.clone().requires_grad_(True), lse_b.clone().requires_grad_(True)
    o2, lse2 = ref.merge(ta, la, tb, lb)
    ((o2 * do).sum() + ref.lse_loss(lse2, dlse)).backward()
    dlse_nan = dlse.clone()
    dlse_nan[:, 2] = float("nan")                   # a row with both sides dead does not read its dlse
    do_a, do_b, dla, dlb = ref.merge_backward(o_a, lse_a, o_b, lse_b, do, dlse_nan)
    for got, want in ((do_a, ta.grad), (do_b, tb.grad), (dla, la.grad), (dlb, lb.grad)):
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, torch.nan_to_num(want, nan=0.0), **TOL)
    assert (do_a[:, 0] == 0).all() and (dla[:, 0] == 0).all() and (do_b[:, 1] == 0).all() and (dlb[:, 3] == 0).all()
    for t in (do_a[:, 2], do_b[:, 2], dla[:, 2], dlb[:, 2]):
        assert (t == 0).all()
    # dlse absent means zero
    for got, want in zip(ref.merge_backward(o_a, lse_a, o_b, lse_b, do), ref.merge_backward(o_a, lse_a, o_b, lse_b, do, torch.zeros_like(dlse))):
        assert torch.equal(got, want)


def test_merge_is_associative_over_three_chunks():
    q, k, v = _rand(2, 7, 8, seed=1), _rand(2, 30, 8, seed=2), _rand(2, 30, 8, seed=3)
    full = ref.attention(q, k, v, None, False, 0.3)
    parts = [ref.attention(q, k[:, a:b], v[:, a:b], None, False, 0.3) for a, b in ((0, 11), (11, 12), (12, 30))]
    left = ref.merge(*ref.merge(*parts[0], *parts[1]), *parts[2])
    right = ref.merge(*parts[0], *ref.merge(*parts[1], *parts[2]))
    for got in (left, right):
        torch.testing.assert_close(got[0], full[0], **TOL)
        torch.testing.assert_close(got[1], full[1], **TOL)


def test_varlen_reference_is_the_dense_one_per_sequence():
    cu = [0, 5, 5, 12]
    q, k, v = _rand(12, 4, 8, seed=1), _rand(12, 2, 8, seed=2), _rand(12, 2, 8, seed=3)
    o, lse = ref.varlen_attention(q, k, v, None, cu, cu, True, 0.3)
    assert o.shape == (12, 4, 8) and lse.shape == (4, 12)
    o1, lse1 = ref.attention(q[5:].transpose(0, 1), k[5:].transpose(0, 1), v[5:].transpose(0, 1), None, True, 0.3)
    assert torch.equal(o[5:], o1.transpose(0, 1)) and torch.equal(lse[:, 5:], lse1)


# ---------------------------------------------------------------------------------------------- declarations

def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS and name in ext._CALLS


def test_signature_rows_are_composed_from_groups():
    import flashattention_lab_cuda as ext

    sig = lambda name: ext._SIGNATURES[name][1]
    # dlse: one named group, after the sink group and before the masks / dropout group; nothing else differs from the sink calls
    for wide, narrow, after in (("fa_ex_backward_dlse", "fa_ex_backward_sink", ext._MASKS), ("fa_ex_backward_varlen_dlse", "fa_ex_backward_varlen_sink", ext._DROPOUT)):
        w, n = sig(wide), sig(narrow)
        at = w.index(ext._DLSE[0])
        assert w[:at] + w[at + 1:] == n
        assert w[at - 1] == ext._DSINK[0] and w[at + 1: at + 1 + len(after)] == after
        assert ext._CALLS[wide][2] == len(w) == len(n) + 1      # the widest of its family
        assert ext._CALLS[narrow][2] == len(w)
    # the forward families are unchanged
    assert ext._CALLS["fa_ex_forward"][2] == len(sig("fa_ex_forward_sink"))
    assert ext._CALLS["fa_ex_forward_varlen"][2] == len(sig("fa_ex_forward_varlen_sink"))
    # merge: pointers, dims, one stride triple per pointer in the pointers' order, stream
    for name, ptrs in (("fa_merge_states", 6), ("fa_merge_states_backward", 10)):
        s = sig(name)
        assert len(s) == ptrs + len(ext._MDIMS) + 3 * ptrs + 1
        assert s[ptrs: ptrs + len(ext._MDIMS)] == ext._MDIMS and s[-1:] == ext._STREAM
        for i in range(ptrs):
            tensor = s[i][0].rstrip("_")
            assert [f for f, _ in s[ptrs + 5 + 3 * i: ptrs + 8 + 3 * i]] == [f"{tensor}_{x}_stride" for x in ("batch", "head", "row")]


def test_ex_variant_picks_the_narrowest_entry_point():
    import flashattention_lab_cuda as ext

    assert ext._ex_variant(0, False, False) == "" and ext._ex_variant(1, True, True, True) == "_sink"
    assert ext._ex_variant(0, False, False, False, True) == "_dlse" and ext._ex_variant(1, True, True, True, True) == "_dlse"


# ---------------------------------------------------------------------------------------------- C-layer validation, no GPU

P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(10)]   # non-null, 16-byte aligned, never dereferenced
DENSE = (3 * 5 * 64, 5 * 64, 64)                            # (2, 3, 5, 64) contiguous
LDENSE = (15, 5, 1)


def _fwd(ptrs=None, dims=(2, 3, 5, 64), dtype=2, strides=None):
    import flashattention_lab_cuda as ext

    ptrs = list(P[:6]) if ptrs is None else ptrs
    strides = [DENSE, LDENSE, DENSE, LDENSE, DENSE, LDENSE] if strides is None else strides
    rc = ext._lib.fa_merge_states(*ptrs, *dims, dtype, *[x for s in strides for x in s], None)
    return rc, ext._lib.fa_last_error().decode()


def _bwd(ptrs=None, dims=(2, 3, 5, 64), dtype=2, strides=None):
    import flashattention_lab_cuda as ext

    ptrs = list(P[:10]) if ptrs is None else ptrs
    strides = [DENSE, LDENSE, DENSE, LDENSE, DENSE, LDENSE, DENSE, DENSE, LDENSE, LDENSE] if strides is None else strides
    rc = ext._lib.fa_merge_states_backward(*ptrs, *dims, dtype, *[x for s in strides for x in s], None)
    return rc, ext._lib.fa_last_error().decode()


def _with(seq, i, value):
    out = list(seq)
    out[i] = value
    return out


def test_merge_validation_codes():
    six = [DENSE, LDENSE, DENSE, LDENSE, DENSE, LDENSE]
    bad = [
        (dict(dtype=3), INVALID_ARGUMENT, "dtype"), (dict(dtype=-1), INVALID_ARGUMENT, "dtype"),
        (dict(dims=(2, 3, 5, 0)), INVALID_ARGUMENT, "bad shape"), (dict(dims=(-1, 3, 5, 64)), INVALID_ARGUMENT, "bad shape"),
        (dict(dims=(2, 3, 2 ** 31, 64)), INVALID_ARGUMENT, "bad shape"),
        (dict(dims=(2, 3, 5, 264)), UNSUPPORTED, "head_dim"),
        (dict(dims=(2, 3, 5, 60)), INVALID_ARGUMENT, "multiple of 8"), (dict(dims=(2, 3, 5, 60), dtype=1), INVALID_ARGUMENT, "multiple of 8"),
        (dict(ptrs=_with(P[:6], 0, None)), INVALID_ARGUMENT, "null tensor pointer (o_a)"),
        (dict(ptrs=_with(P[:6], 3, None)), INVALID_ARGUMENT, "null tensor pointer (lse_b)"),
        (dict(ptrs=_with(P[:6], 5, None)), INVALID_ARGUMENT, "null tensor pointer (lse)"),
        (dict(ptrs=_with(P[:6], 2, ctypes.c_void_p(4104))), INVALID_ARGUMENT, "o_b must be 16-byte aligned"),
        (dict(ptrs=_with(P[:6], 1, ctypes.c_void_p(4098))), INVALID_ARGUMENT, "lse_a must be 4-byte aligned"),
        (dict(strides=_with(six, 0, (3 * 5 * 64, 5 * 64, 68))), INVALID_ARGUMENT, "multiples of 8"),
        (dict(strides=_with(six, 4, (3 * 5 * 64 + 4, 5 * 64, 64))), INVALID_ARGUMENT, "multiples of 8"),
        (dict(strides=_with(six, 2, (3 * 5 * 64, -320, 64))), INVALID_ARGUMENT, ">= 0"),
        (dict(strides=_with(six, 1, (2 ** 59, 5, 1))), INVALID_ARGUMENT, "2^58"),
        (dict(strides=_with(six, 3, (15, 5, 2 ** 57))), INVALID_ARGUMENT, "2^58"),
        # in place with other strides than the input's
        (dict(ptrs=_with(P[:6], 4, P[0]), strides=_with(six, 4, (3 * 5 * 128, 5 * 128, 128))), INVALID_ARGUMENT, "in place"),
        (dict(ptrs=_with(P[:6], 5, P[1]), strides=_with(six, 5, (30, 10, 2))), INVALID_ARGUMENT, "in place"),
    ]
    for kw, code, what in bad:
        rc, msg = _fwd(**kw)
        assert rc == code and what in msg and msg.startswith("fa_merge_states:"), (kw, rc, msg)
    # fp32 takes any d and any 4-byte aligned view (it falls back to 4-byte accesses); only the 4-byte rule remains
    rc, msg = _fwd(dtype=0, dims=(2, 3, 5, 40), ptrs=_with(P[:6], 0, ctypes.c_void_p(4098)))
    assert rc == INVALID_ARGUMENT and "o_a must be 4-byte aligned" in msg
    # the backward: the same rules over its ten tensors; dlse alone may be null
    ten = [DENSE, LDENSE, DENSE, LDENSE, DENSE, LDENSE, DENSE, DENSE, LDENSE, LDENSE]
    for kw, code, what in [(dict(dtype=7), INVALID_ARGUMENT, "dtype"), (dict(dims=(2, 3, 5, 12)), INVALID_ARGUMENT, "multiple of 8"),
                           (dict(ptrs=_with(P, 4, None)), INVALID_ARGUMENT, "null tensor pointer (do_)"),
                           (dict(ptrs=_with(P, 9, None)), INVALID_ARGUMENT, "null tensor pointer (dlse_b)"),
                           (dict(ptrs=_with(P, 6, ctypes.c_void_p(4100))), INVALID_ARGUMENT, "do_a must be 16-byte aligned"),
                           (dict(ptrs=_with(P, 5, ctypes.c_void_p(4097))), INVALID_ARGUMENT, "dlse must be 4-byte aligned"),
                           (dict(strides=_with(ten, 7, (3 * 5 * 64, 5 * 64, 65))), INVALID_ARGUMENT, "multiples of 8")]:
        rc, msg = _bwd(**kw)
        assert rc == code and what in msg and msg.startswith("fa_merge_states_backward:"), (kw, rc, msg)


def test_the_first_broken_rule_names_itself():
    for kw, what in ((dict(dtype=9, dims=(2, 3, 5, 60)), "dtype"), (dict(dims=(2, 3, -5, 60)), "bad shape"),
                     (dict(dims=(2, 3, 5, 60), ptrs=_with(P[:6], 0, None)), "multiple of 8"),
                     (dict(ptrs=_with(_with(P[:6], 0, None), 2, ctypes.c_void_p(4104))), "null tensor pointer"),
                     (dict(ptrs=_with(P[:6], 2, ctypes.c_void_p(4104)), strides=[DENSE, (2 ** 59, 5, 1), DENSE, LDENSE, DENSE, LDENSE]), "16-byte")):
        rc, msg = _fwd(**kw)
        assert rc == INVALID_ARGUMENT and what in msg, (kw, msg)


def test_a_call_without_rows_is_ok_without_a_launch():
    """no row: FA_OK, nothing launched (there is no device here), and the pointers are not looked at (an empty tensor has none)"""
    for dims in ((0, 3, 5, 64), (2, 0, 5, 64), (2, 3, 0, 64)):
        assert _fwd(dims=dims)[0] == 0
        assert _fwd(dims=dims, ptrs=[None] * 6)[0] == 0
        assert _bwd(dims=dims, ptrs=[None] * 10)[0] == 0
    assert _fwd(dims=(2, 3, 0, 60))[0] == INVALID_ARGUMENT      # validation of the shape still comes first


def test_dlse_alignment_is_checked_before_any_hip_call():
    import flashattention_lab_cuda as ext

    p = P[0]
    odd = ctypes.c_void_p(4098)
    rc = ext._lib.fa_ex_backward_dlse(p, p, p, p, p, p, p, p, p, 4, 1, 16, 16, 64, 2, 0, -1, -1, 0.125, 0.0, None, 1, 0, None, 1, None, odd,
                                      None, 0, None, 0, 0, 0.0, 0, p, 1 << 20, None)
    assert rc == INVALID_ARGUMENT and "fa_ex_backward_dlse: dlse must be 4-byte aligned" in ext._lib.fa_last_error().decode()
    rc = ext._lib.fa_ex_backward_varlen_dlse(p, p, p, p, p, p, p, p, p, p, p, 2, 4, 2, 16, 16, 8, 8, 64, 2, 256, 128, 128, 0, -1, -1, 0.125,
                                             0.0, None, 0, None, 1, None, odd, 0.0, 0, p, 1 << 20, None)
    assert rc == INVALID_ARGUMENT and "fa_ex_backward_varlen_dlse: dlse must be 4-byte aligned" in ext._lib.fa_last_error().decode()
    # an empty problem with a dlse is still an empty problem
    assert ext._lib.fa_ex_backward_dlse(p, p, p, p, p, p, p, p, p, 0, 1, 16, 16, 64, 2, 0, -1, -1, 0.125, 0.0, None, 1, 0, None, 1, None, p,
                                        None, 0, None, 0, 0, 0.0, 0, p, 1 << 20, None) == 0


# ---------------------------------------------------------------------------------------------- shim and wrapper errors

class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def test_shim_rejects_a_wrong_dlse():
    import flashattention_lab_cuda as ext

    q, lse = _fake(4, 16, 64), _fake(4, 16, dtype=torch.float32)
    for dlse in (_fake(4, 15, dtype=torch.float32), _fake(16, 4, dtype=torch.float32), _fake(4, 16, 1, dtype=torch.float32),
                 _fake(4, 16, dtype=torch.bfloat16), _fake(4, 16, dtype=torch.float64), 1.0):
        with pytest.raises(RuntimeError, match=r"ex_backward: dlse must be a \(BH, Nq\) float32 tensor"):
            ext.ex_backward(q, q, q, q, q, lse, False, 0.125, dlse=dlse)
    cu = torch.tensor([0, 7, 16], dtype=torch.int32).as_subclass(FakeCuda)
    qv, lsev = _fake(16, 4, 64), _fake(4, 16, dtype=torch.float32)
    for dlse in (_fake(16, 4, dtype=torch.float32), _fake(4, 16, dtype=torch.float16)):
        with pytest.raises(RuntimeError, match=r"ex_varlen_backward: dlse must be a \(H_q, total_q\) float32 tensor"):
            ext.ex_varlen_backward(qv, qv, qv, qv, qv, lsev, cu, cu, 9, 9, True, 0.125, dlse=dlse)


def test_wrapper_errors():
    from common.merge_states import merge_attention_states

    o, lse = _fake(2, 3, 5, 64), _fake(2, 3, 5, dtype=torch.float32)
    with pytest.raises(ValueError, match="layout"):
        merge_attention_states(o, lse, o, lse, layout="bshd")
    # out= under grad
    og = _fake(2, 3, 5, 64).requires_grad_(True)
    with pytest.raises(RuntimeError, match="only outside autograd"):
        merge_attention_states(og, lse, o, lse, out=(o, lse))
    # mismatched shapes, dtypes
    for args in ((o, lse, _fake(2, 3, 5, 32), lse), (o, lse, _fake(2, 3, 5, 64, dtype=torch.float16), lse), (o, lse, o, _fake(2, 3, 4, dtype=torch.float32)),
                 (o, _fake(2, 3, 5, dtype=torch.bfloat16), o, lse), (o, _fake(2, 5, 3, dtype=torch.float32), o, _fake(2, 5, 3, dtype=torch.float32)),
                 (_fake(2, 3, 5, 60), lse, _fake(2, 3, 5, 60), lse)):
        with pytest.raises(RuntimeError):
            merge_attention_states(*args)
    with pytest.raises(RuntimeError, match="layout 'thd' does not take"):
        merge_attention_states(o, lse, o, lse, layout="thd")
    with pytest.raises(RuntimeError, match="no CPU path"):
        merge_attention_states(torch.zeros(2, 3, 5, 64), lse, o, lse)
    # views the kernel cannot address: a last dim that is not contiguous, strides that are no multiple of 8, a misaligned start
    wide = _fake(2, 3, 5, 128)
    with pytest.raises(ValueError, match="contiguous last dim"):
        merge_attention_states(wide[..., ::2], lse, o, lse)
    with pytest.raises(ValueError, match="cannot address"):
        merge_attention_states(_fake(2, 3, 5, 68)[..., :64], lse, o, lse)
    with pytest.raises(ValueError, match="cannot address"):
        merge_attention_states(_fake(2, 3, 5, 72)[..., 4:68], lse, o, lse)
    with pytest.raises(RuntimeError, match="out must be a pair"):
        with torch.no_grad():
            merge_attention_states(o, lse, o, lse, out=o)
