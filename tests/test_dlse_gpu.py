"""GPU: the differentiable lse (fa_ex_backward_dlse, fa_ex_backward_varlen_dlse; flash_attention_ex(..., return_lse=True),
flash_attention_varlen(..., return_softmax_lse=True)) and its composition with merge_attention_states, against the fp64 references
of tests/merge_ref.py.  Bars: tests/helpers.py dtype_tolerances for o and every gradient, rtol = atol = 1e-3 on finite lse (as
tests/test_sinks_gpu.py).  Shapes: 320 rows and keys cross a 256-row workgroup tile and a 128-key tile; the key split 136 is no
tile multiple."""
import functools

import pytest
import torch

from tests import merge_ref as ref
from tests.helpers import dtype_tolerances, max_abs

pytestmark = pytest.mark.gpu

PATHS = {"auto": 0, "exact": 1, "mfma_only": 3}
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


class on_path:
    def __init__(self, path):
        self.path = PATHS[path]

    def __enter__(self):
        import flashattention_lab_cuda as ext

        ext.set_option("ex_path", self.path)

    def __exit__(self, *exc):
        import flashattention_lab_cuda as ext

        ext.set_option("ex_path", 0)
        return False


def _randn(shape, seed, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _close(name, got, want, dtype):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), name
    print(f"{name}: max |got - fp64| = {(got - want).abs().max().item():.3e}")
    torch.testing.assert_close(got, want, **dtype_tolerances(dtype), msg=lambda m: f"{name}: {m}")


def _close_lse(got, want):
    got = got.detach().double().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin) and (got[~fin] == ref.NEG_INF).all()
    torch.testing.assert_close(got[fin], want[fin], rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------------------------------------- low level: ex_backward(dlse=)

FEATURES = {
    "plain": dict(), "causal": dict(causal=True), "gqa2": dict(g=2),
    "window": dict(window=(70, 40)), "mask": dict(mask=True), "dropout": dict(dropout_p=0.1, seed=5), "softcap": dict(softcap=15.0),
    "sinks": dict(sinks=True, causal=True),
}
KINDS = [(BF16, 64, "mfma_only"), (BF16, 128, "mfma_only"), (F16, 64, "mfma_only"), (F16, 128, "mfma_only"), (F32, 40, "exact")]
LOW = [(k, f) for k in KINDS for f in ("plain", "causal", "gqa2")] + \
      [(KINDS[1], "window"), (KINDS[0], "mask"), (KINDS[3], "dropout"), (KINDS[1], "softcap"), (KINDS[1], "sinks"), (KINDS[4], "sinks"),
       (KINDS[4], "window")]


@functools.lru_cache(maxsize=None)
def _low_case(dtype, d, feature, nq=320, nk=320):
    """the inputs of a low-level case and its fp64 gradients, computed once"""
    f = dict(FEATURES[feature])
    bh, g = 4, f.pop("g", 1)
    q, k, v = _randn((bh, nq, d), 1, dtype), _randn((bh // g, nk, d), 2, dtype), _randn((bh // g, nk, d), 3, dtype)
    do, dlse = _randn((bh, nq, d), 4, dtype), _randn((bh, nq), 5)
    sinks = torch.tensor([0.5, -1.0]) if f.pop("sinks", False) else None
    mask = (_randn((nq, nk), 6) > -1.0) if f.pop("mask", False) else None
    if mask is not None:
        mask[:, 0] = True
    causal = f.pop("causal", False)
    scale = d ** -0.5
    kw = dict(f)
    if mask is not None:
        kw["mask"] = mask.to(torch.uint8)
    want = ref.attention_grads(q, k, v, do, dlse, sinks, causal, scale, **kw)
    return q, k, v, do, dlse, sinks, mask, causal, scale, f, want


@pytest.mark.parametrize("kind,feature", LOW, ids=[f"{str(k[0])[6:]}-d{k[1]}-{f}" for k, f in LOW])
def test_ex_backward_with_dlse_against_fp64(device, kind, feature):
    import flashattention_lab_cuda as ext

    dtype, d, path = kind
    q, k, v, do, dlse, sinks, mask, causal, scale, f, want = _low_case(dtype, d, feature)
    o64, lse64, dq64, dk64, dv64, ds64 = want
    qd, kd, vd, dod, dlsed = (t.to(device) for t in (q, k, v, do, dlse))
    kw = dict(window=f.get("window", (-1, -1)), softcap=f.get("softcap", 0.0), dropout_p=f.get("dropout_p", 0.0), seed=f.get("seed", 0),
              mask=None if mask is None else mask.to(device), sinks=None if sinks is None else sinks.to(device))
    with on_path(path):
        o, lse = ext.ex_forward(qd, kd, vd, causal, scale, **kw)
        grads = ext.ex_backward(qd, kd, vd, o, dod, lse, causal, scale, dlse=dlsed, **kw)
        plain = ext.ex_backward(qd, kd, vd, o, dod, lse, causal, scale, **kw)
    _close("o", o, o64, dtype)
    _close_lse(lse, lse64)
    for name, got, w in zip(("dq", "dk", "dv"), grads, (dq64, dk64, dv64)):
        _close(name, got, w, dtype)
    assert torch.equal(grads[2], plain[2])                 # dV does not depend on dlse
    assert not torch.equal(grads[0], plain[0])             # ... and dQ does
    if sinks is not None:
        _close("dsinks", grads[3], ds64, dtype)


@pytest.mark.parametrize("dtype,d,path", [(BF16, 128, "mfma_only"), (F16, 64, "mfma_only"), (F32, 40, "exact")])
def test_ex_varlen_backward_with_dlse_against_fp64(device, dtype, d, path):
    import flashattention_lab_cuda as ext

    lens, hq, hkv, scale = (37, 0, 200), 4, 2, d ** -0.5
    cu = [0, 37, 37, 237]
    total = cu[-1]
    q, k, v = _randn((total, hq, d), 1, dtype), _randn((total, hkv, d), 2, dtype), _randn((total, hkv, d), 3, dtype)
    do, dlse = _randn((total, hq, d), 4, dtype), _randn((hq, total), 5)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o64, lse64 = ref.varlen_attention(qr, kr, vr, None, cu, cu, True, scale)
    ((o64 * do.double()).sum() + ref.lse_loss(lse64, dlse.double())).backward()
    cud = torch.tensor(cu, dtype=torch.int32, device=device)
    qd, kd, vd, dod, dlsed = (t.to(device) for t in (q, k, v, do, dlse))
    with on_path(path):
        o, lse = ext.ex_varlen_forward(qd, kd, vd, cud, cud, max(lens), max(lens), True, scale)
        dq, dk, dv = ext.ex_varlen_backward(qd, kd, vd, o, dod, lse, cud, cud, max(lens), max(lens), True, scale, dlse=dlsed)
    _close("o", o, o64.detach(), dtype)
    _close_lse(lse, lse64.detach())
    for name, got, w in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        _close(name, got, w, dtype)


# ---------------------------------------------------------------------------------------------- unchanged behaviour

@pytest.mark.parametrize("feature,nq,nk", [("plain", 320, 320), ("causal", 256, 384), ("sinks", 320, 320), ("gqa2", 320, 320)])
def test_a_null_dlse_through_the_new_entry_point_gives_the_old_bits(device, monkeypatch, feature, nq, nk):
    import flashattention_lab_cuda as ext

    q, k, v, do, _dlse, sinks, _mask, causal, scale, _f, _want = _low_case(BF16, 128, feature, nq, nk)
    qd, kd, vd, dod = (t.to(device) for t in (q, k, v, do))
    kw = dict(sinks=None if sinks is None else sinks.to(device))
    o, lse = ext.ex_forward(qd, kd, vd, causal, scale, **kw)
    old = ext.ex_backward(qd, kd, vd, o, dod, lse, causal, scale, **kw)
    called = []
    real = ext._call
    monkeypatch.setattr(ext, "_ex_variant", lambda *a, **k_: "_dlse")        # the widest entry point, dlse = NULL
    monkeypatch.setattr(ext, "_call", lambda name, values: (called.append(name), real(name, values))[1])
    new = ext.ex_backward(qd, kd, vd, o, dod, lse, causal, scale, **kw)
    assert called == ["fa_ex_backward_dlse"]
    for a, b in zip(old, new):
        assert torch.equal(a, b)


def test_a_null_dlse_through_the_new_varlen_entry_point_gives_the_old_bits(device, monkeypatch):
    import flashattention_lab_cuda as ext

    cu = torch.tensor([0, 37, 37, 237], dtype=torch.int32, device=device)
    q, k, v, do = (_randn((237, h, 128), s, BF16).to(device) for s, h in ((1, 4), (2, 2), (3, 2), (4, 4)))
    o, lse = ext.ex_varlen_forward(q, k, v, cu, cu, 200, 200, True, 0.1)
    old = ext.ex_varlen_backward(q, k, v, o, do, lse, cu, cu, 200, 200, True, 0.1)
    called = []
    real = ext._call
    monkeypatch.setattr(ext, "_ex_variant", lambda *a, **k_: "_dlse")
    monkeypatch.setattr(ext, "_call", lambda name, values: (called.append(name), real(name, values))[1])
    new = ext.ex_varlen_backward(q, k, v, o, do, lse, cu, cu, 200, 200, True, 0.1)
    assert called == ["fa_ex_backward_varlen_dlse"]
    for a, b in zip(old, new):
        assert torch.equal(a, b)


@pytest.mark.parametrize("four_d,with_sinks", [(True, False), (False, True)])
def test_return_lse_leaves_o_and_the_gradients_of_an_o_only_loss_bitwise(device, four_d, with_sinks):
    from common.attention_ex import flash_attention_ex

    shape_q, shape_k = ((2, 4, 320, 128), (2, 2, 320, 128)) if four_d else ((8, 320, 128), (4, 320, 128))
    q, k, v = _randn(shape_q, 1, BF16).to(device), _randn(shape_k, 2, BF16).to(device), _randn(shape_k, 3, BF16).to(device)
    g = _randn(shape_q, 4, BF16).to(device)
    sinks = torch.tensor([0.5, -1.0, 0.0, 2.0], device=device) if with_sinks else None
    outs = []
    for return_lse in (False, True):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)] + ([sinks.clone().requires_grad_(True)] if with_sinks else [])
        r = flash_attention_ex(*leaves[:3], causal=True, sinks=leaves[3] if with_sinks else None, return_lse=return_lse)
        o = r[0] if return_lse else r
        if return_lse:
            assert r[1].shape == shape_q[:-1] and r[1].dtype == F32 and r[1].requires_grad
        (o * g).sum().backward()
        outs.append([o.detach()] + [t.grad for t in leaves])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- rows without a visible key

@pytest.mark.parametrize("dtype,d,path", [(BF16, 128, "mfma_only"), (F16, 64, "mfma_only"), (F32, 40, "exact")])
def test_rows_at_minus_inf_ignore_a_nan_dlse(device, dtype, d, path):
    import flashattention_lab_cuda as ext

    q, k, v, do, dlse, _s, _m, causal, scale, _f, want = _low_case(dtype, d, "causal", 320, 200)
    o64, lse64, dq64, dk64, dv64, _ds = want
    dead = ~torch.isfinite(lse64)
    assert dead[:, :120].all() and not dead[:, 120:].any()                  # the first Nq - Nk rows see no key
    dlse = torch.where(dead, torch.full_like(dlse, float("nan")), dlse)
    qd, kd, vd, dod, dlsed = (t.to(device) for t in (q, k, v, do, dlse))
    with on_path(path):
        o, lse = ext.ex_forward(qd, kd, vd, causal, scale)
        dq, dk, dv = ext.ex_backward(qd, kd, vd, o, dod, lse, causal, scale, dlse=dlsed)
    _close_lse(lse, lse64)
    assert (dq.cpu()[dead] == 0).all()
    for name, got, w in (("dq", dq, dq64), ("dk", dk, dk64), ("dv", dv, dv64)):
        _close(name, got, w, dtype)


# ---------------------------------------------------------------------------------------------- composition with the merge

SPLIT = 136
COMPOSE = [("noncausal", 320, 320, False, False), ("causal", 320, 320, True, False), ("causal-short-q", 64, 320, True, False),
           ("sinks", 320, 320, True, True), ("noncausal-sinks", 64, 320, False, True)]


@pytest.mark.parametrize("name,nq,nk,causal,with_sinks", COMPOSE, ids=[c[0] for c in COMPOSE])
def test_two_merged_key_chunks_are_the_full_call(device, name, nq, nk, causal, with_sinks):
    """forward and dq, dk, dv (dsinks) through autograd, against the fp64 reference of the FULL call"""
    from common.attention_ex import flash_attention_ex
    from common.merge_states import merge_attention_states

    b, h, hkv, d, dtype = 1, 4, 2, 128, BF16
    q, k, v, g = _randn((b, h, nq, d), 1, dtype), _randn((b, hkv, nk, d), 2, dtype), _randn((b, hkv, nk, d), 3, dtype), _randn((b, h, nq, d), 4, dtype)
    gl = _randn((b, h, nq), 5)
    sinks = torch.tensor([0.5, -1.0, 0.0, 2.0]) if with_sinks else None
    o64, lse64, dq64, dk64, dv64, ds64 = ref.attention_grads(q.reshape(b * h, nq, d), k.reshape(b * hkv, nk, d), v.reshape(b * hkv, nk, d),
                                                              g.reshape(b * h, nq, d), gl.reshape(b * h, nq), sinks, causal, d ** -0.5)
    ql, kl, vl = (t.to(device).requires_grad_(True) for t in (q, k, v))
    sl = None if sinks is None else sinks.to(device).requires_grad_(True)
    # chunk a = keys[:SPLIT]: causal=False with the window (-1, Nk - SPLIT); chunk b = the rest: plain causal; sinks on chunk a only
    o_a, lse_a = flash_attention_ex(ql, kl[:, :, :SPLIT], vl[:, :, :SPLIT], causal=False, window_size=(-1, nk - SPLIT) if causal else (-1, -1),
                                    sinks=sl, return_lse=True)
    o_b, lse_b = flash_attention_ex(ql, kl[:, :, SPLIT:], vl[:, :, SPLIT:], causal=causal, return_lse=True)
    if causal and nq == nk:
        assert (lse_b[:, :, :SPLIT] == ref.NEG_INF).all() and torch.isfinite(lse_b[:, :, SPLIT:]).all()
    o, lse = merge_attention_states(o_a, lse_a, o_b, lse_b)
    ((o * g.to(device)).sum() + (lse * gl.to(device)).sum()).backward()
    with torch.no_grad():
        full = flash_attention_ex(ql, kl, vl, causal=causal, sinks=sl)
    print(f"max |merged - the library's full call| = {max_abs(o.detach().cpu(), full.cpu()):.3e}")
    _close("o", o.reshape(b * h, nq, d), o64, dtype)
    _close_lse(lse.reshape(b * h, nq), lse64)
    _close("dq", ql.grad.reshape(b * h, nq, d), dq64, dtype)
    _close("dk", kl.grad.reshape(b * hkv, nk, d), dk64, dtype)
    _close("dv", vl.grad.reshape(b * hkv, nk, d), dv64, dtype)
    if with_sinks:
        _close("dsinks", sl.grad, ds64, dtype)


def test_two_merged_key_chunks_are_the_full_varlen_call(device):
    """packed sequences through the "thd" layout: each sequence's keys split in two, non-causal"""
    from common.attention_ex import flash_attention_varlen
    from common.merge_states import merge_attention_states

    hq, hkv, d, dtype = 4, 2, 128, BF16
    cu, splits = [0, 37, 37, 237], (20, 0, 136)
    total = cu[-1]
    ia = [t for b, s in enumerate(splits) for t in range(cu[b], cu[b] + s)]
    ib = [t for b, s in enumerate(splits) for t in range(cu[b] + s, cu[b + 1])]
    cu_a = [0, 20, 20, 156]
    cu_b = [0, 17, 17, 81]
    q, k, v, g = _randn((total, hq, d), 1, dtype), _randn((total, hkv, d), 2, dtype), _randn((total, hkv, d), 3, dtype), _randn((total, hq, d), 4, dtype)
    gl = _randn((hq, total), 5)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o64, lse64 = ref.varlen_attention(qr, kr, vr, None, cu, cu, False, d ** -0.5)
    ((o64 * g.double()).sum() + ref.lse_loss(lse64, gl.double())).backward()
    dev_cu = lambda c: torch.tensor(c, dtype=torch.int32, device=device)
    ql, kl, vl = (t.to(device).requires_grad_(True) for t in (q, k, v))
    parts = []
    for idx, cu_k in ((ia, cu_a), (ib, cu_b)):
        sel = torch.tensor(idx, device=device)
        parts += flash_attention_varlen(ql, kl[sel], vl[sel], dev_cu(cu), dev_cu(cu_k), 200, 200, return_softmax_lse=True)
    assert parts[1].shape == (hq, total) and parts[1].requires_grad
    o, lse = merge_attention_states(*parts, layout="thd")
    ((o * g.to(device)).sum() + (lse * gl.to(device)).sum()).backward()
    with torch.no_grad():
        full = flash_attention_varlen(ql, kl, vl, dev_cu(cu), dev_cu(cu), 200, 200)
    print(f"max |merged - the library's full call| = {max_abs(o.detach().cpu(), full.cpu()):.3e}")
    _close("o", o, o64.detach(), dtype)
    _close_lse(lse, lse64.detach())
    _close("dq", ql.grad, qr.grad, dtype)
    _close("dk", kl.grad, kr.grad, dtype)
    _close("dv", vl.grad, vr.grad, dtype)


def test_varlen_return_softmax_lse_with_block_table_has_no_gradient(device):
    from common.attention_ex import flash_attention_varlen

    hq, hkv, d, ps = 4, 2, 128, 16
    cu = torch.tensor([0, 5, 12], dtype=torch.int32, device=device)
    cu_k = torch.tensor([0, 20, 50], dtype=torch.int32, device=device)
    q = _randn((12, hq, d), 1, BF16).to(device)
    pool_k, pool_v = _randn((4, ps, hkv, d), 2, BF16).to(device), _randn((4, ps, hkv, d), 3, BF16).to(device)
    table = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=device)
    o, lse = flash_attention_varlen(q, pool_k, pool_v, cu, cu_k, 7, 30, causal=True, block_table=table, return_softmax_lse=True)
    o2 = flash_attention_varlen(q, pool_k, pool_v, cu, cu_k, 7, 30, causal=True, block_table=table)
    assert torch.equal(o, o2) and lse.shape == (hq, 12) and lse.dtype == F32 and not lse.requires_grad
    assert torch.isfinite(lse).all()


# ---------------------------------------------------------------------------------------------- cascade decode

def test_cascade_decode_prefix_and_suffix_merge_to_one_causal_call(device):
    from common.attention_ex import flash_attn_with_kvcache
    from common.merge_states import merge_attention_states

    b, nq, hq, hkv, d, dtype = 2, 3, 4, 2, 128, BF16
    npre, nsuf = 200, 72
    q = _randn((b, nq, hq, d), 1, dtype)
    kp, vp = _randn((b, npre, hkv, d), 2, dtype), _randn((b, npre, hkv, d), 3, dtype)
    ks, vs = _randn((b, 128, hkv, d), 4, dtype), _randn((b, 128, hkv, d), 5, dtype)
    kn, vn = _randn((b, nq, hkv, d), 6, dtype), _randn((b, nq, hkv, d), 7, dtype)
    qd = q.to(device)
    o_p, lse_p = flash_attn_with_kvcache(qd, kp.to(device), vp.to(device), causal=False, return_softmax_lse=True)
    lens = torch.full((b,), nsuf, dtype=torch.int32, device=device)
    o_s, lse_s = flash_attn_with_kvcache(qd, ks.to(device), vs.to(device), k=kn.to(device), v=vn.to(device), cache_seqlens=lens, causal=True,
                                         return_softmax_lse=True)
    o, lse = merge_attention_states(o_p, lse_p, o_s, lse_s, layout="bnhd")
    assert o.shape == (b, nq, hq, d) and lse.shape == (b, hq, nq)
    for i in range(b):
        kk = torch.cat([kp[i], ks[i, :nsuf], kn[i]]).transpose(0, 1).double()        # (H_kv, 275, d)
        vv = torch.cat([vp[i], vs[i, :nsuf], vn[i]]).transpose(0, 1).double()
        o64, lse64 = ref.attention(q[i].transpose(0, 1).double(), kk, vv, None, True, d ** -0.5)
        _close(f"o[{i}]", o[i].transpose(0, 1), o64, dtype)
        _close_lse(lse[i], lse64)


# ---------------------------------------------------------------------------------------------- autograd plumbing

def test_a_loss_on_o_and_lse_against_fp64_autograd(device):
    """gradcheck is of no use at 16 bits; fp32, d = 40, N = 48 on the exact kernels, loss sum(o * g) + sum(lse * h), at 1e-4"""
    from common.attention_ex import flash_attention_ex

    bh, n, d = 4, 48, 40
    q, k, v, g = (_randn((bh, n, d), s) for s in (1, 2, 3, 4))
    h = _randn((bh, n), 5)
    _o, _l, dq64, dk64, dv64, _ds = ref.attention_grads(q, k, v, g, h, None, True, d ** -0.5)
    leaves = [t.to(device).requires_grad_(True) for t in (q, k, v)]
    with on_path("exact"):
        o, lse = flash_attention_ex(*leaves, causal=True, return_lse=True)
        ((o * g.to(device)).sum() + (lse * h.to(device)).sum()).backward()
    for name, leaf, want in zip(("dq", "dk", "dv"), leaves, (dq64, dk64, dv64)):
        torch.testing.assert_close(leaf.grad.double().cpu(), want, rtol=1e-4, atol=1e-4, msg=lambda m: f"{name}: {m}")
    # a loss on lse alone: autograd materialises no dO, the Function makes the zeros
    leaves = [t.to(device).requires_grad_(True) for t in (q, k, v)]
    with on_path("exact"):
        (flash_attention_ex(*leaves, causal=True, return_lse=True)[1] * h.to(device)).sum().backward()
    want = ref.attention_grads(q, k, v, None, h, None, True, d ** -0.5)
    for name, leaf, w in zip(("dq", "dk", "dv"), leaves, want[2:5]):
        torch.testing.assert_close(leaf.grad.double().cpu(), w, rtol=1e-4, atol=1e-4, msg=lambda m: f"{name}: {m}")
