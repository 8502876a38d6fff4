"""GPU: attention sinks (fa_ex_*_sink; the `sinks` keyword of flashattention_lab_cuda and common/attention_ex.py) against the fp64
reference of tests/sink_ref.py: forward and backward on the 16-bit MFMA kernels and the exact-f32 ones, packed sequences, the
sink's own gradient, rows without a visible key, huge and switched-off sinks, autograd, and KV-cache decoding with its
combinations.  B = 2, H = 4 throughout the extended path (sinks are (H,), unit u = b H + h takes sinks[h])."""
import pytest
import torch

from tests import sink_ref as sr
from tests.helpers import dtype_tolerances

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = {"auto": 0, "exact": 1, "mfma_only": 3}
NEG_INF = float("-inf")
B, H = 2, 4
SINKS = (0.6, -1.5, 2.5, 0.0)


def make(bh, bh_kv, nq, nk, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((bh, nq, d), generator=g).to(dtype).to(DEV)
    k = torch.randn((bh_kv, nk, d), generator=g).to(dtype).to(DEV)
    v = torch.randn((bh_kv, nk, d), generator=g).to(dtype).to(DEV)
    do = torch.randn((bh, nq, d), generator=g).to(dtype).to(DEV)
    return q, k, v, do


def run(ext, path, q, k, v, do, sinks, causal, scale, **kw):
    """(o, lse, dq, dk, dv, dsinks); sinks=None: the call without the keyword, dsinks None"""
    ext.set_option("ex_path", PATHS[path])
    try:
        if sinks is None:
            o, lse = ext.ex_forward(q, k, v, causal, scale, **kw)
            got = ext.ex_backward(q, k, v, o, do, lse, causal, scale, **kw) + (None,)
        else:
            o, lse = ext.ex_forward(q, k, v, causal, scale, sinks=sinks, **kw)
            got = ext.ex_backward(q, k, v, o, do, lse, causal, scale, sinks=sinks, **kw)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return (o, lse) + tuple(got)


def check(got, ref, dtype, what="", dsinks=True):
    tol = dtype_tolerances(dtype)
    o, lse, dq, dk, dv = (t.cpu() for t in got[:5])
    ro, rlse, rdq, rdk, rdv, rds = ref
    torch.testing.assert_close(o.double(), ro, **tol, msg=lambda m: f"o {what}: {m}")
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin), f"lse -inf pattern {what}"
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-3, atol=1e-3, msg=lambda m: f"lse {what}: {m}")
    for name, a, b in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        torch.testing.assert_close(a.double(), b, **tol, msg=lambda m, n=name: f"{n} {what}: {m}")
    if dsinks:
        ds = got[5].cpu()
        assert ds.dtype == torch.float32 and ds.shape == rds.shape
        print(f"dsinks {what}: got {ds.tolist()} ref {rds.tolist()} max |diff| {(ds.double() - rds).abs().max().item():.3e}")
        torch.testing.assert_close(ds.double(), rds, **tol, msg=lambda m: f"dsinks {what}: {m}")


def check_dsinks_against_own_outputs(got, do, sinks, what=""):
    """The new kernel alone: the formula in fp64 from the kernel's own o, lse and the do it was given; within
    1e-4 * sum |term| + 1e-6 (fp32 delta over d <= 256 products, one exp and a tree sum over <= 600 rows: a few 1e-6 each)."""
    term = sr.dsink_terms(got[0], do, got[1], sinks)
    want = sr.dsink_sum(term, sinks.shape[0])
    bound = 1e-4 * sr.dsink_sum(term.abs(), sinks.shape[0]) + 1e-6
    err = (got[5].cpu().double() - want).abs()
    print(f"dsinks vs own outputs {what}: err {err.tolist()} bound {bound.tolist()}")
    assert bool((err <= bound).all()), f"{what}: {err.tolist()} > {bound.tolist()}"


# ---- parity grid

PAIRS = [(160, 160), (1, 200), (48, 16), (300, 300)]
GRID = [(dt, d, hkv, pair) for dt in (torch.bfloat16, torch.float16) for d in (64, 128) for hkv in (4, 2, 1) for pair in PAIRS]
GRID += [(torch.float32, 64, (4, 2, 1, 2)[i], pair) for i, pair in enumerate(PAIRS)]   # the exact-f32 kernels
GRID += [(torch.bfloat16, 256, 2, (300, 300))]                                          # d = 256: exact f32 on 16-bit tensors


@pytest.mark.parametrize("dtype,d,hkv,pair", GRID, ids=lambda x: str(x).replace("torch.", ""))
def test_forward_and_backward_match_the_reference(dtype, d, hkv, pair):
    import flashattention_lab_cuda as ext

    nq, nk = pair
    q, k, v, do = make(B * H, B * hkv, nq, nk, d, dtype, seed=nq + d + hkv)
    sinks = torch.tensor(SINKS, device=DEV)
    scale = d ** -0.5
    got = run(ext, "auto", q, k, v, do, sinks, False, scale)
    ref = sr.sink_reference(q, k, v, do, sinks, False, scale)
    what = f"{dtype} d={d} hkv={hkv} {pair}"
    check(got, ref, dtype, what)
    check_dsinks_against_own_outputs(got, do, sinks, what)


def _feature(name, nq, nk, bh):
    g = torch.Generator().manual_seed(7)
    if name == "causal":
        return True, {}, {}
    if name == "window":
        return True, dict(window=(64, 0)), dict(window=(64, 0))
    if name == "mask":
        m = (torch.rand((bh, nq, nk), generator=g) > 0.3).to(torch.uint8)
        m[0, :5] = 0   # rows without a visible key
        return False, dict(mask=m.to(DEV)), dict(mask=m)
    if name == "block":
        bm = (torch.rand(((nq + 63) // 64, (nk + 63) // 64), generator=g) > 0.35).to(torch.uint8)
        bm[0, 0] = 1
        return False, dict(block_mask=bm.to(DEV), br=64, bc=64), dict(block_mask=bm, br=64, bc=64)
    if name == "dropout":
        return False, dict(dropout_p=0.1, seed=41), dict(dropout_p=0.1, seed=41)
    if name == "softcap":
        return False, dict(softcap=30.0), dict(softcap=30.0)
    if name == "alibi":
        sl = torch.tensor([2.0 ** (-8.0 * (i % H + 1) / H) for i in range(bh)], dtype=torch.float32)
        return False, dict(alibi_slopes=sl.to(DEV)), dict(slopes=sl)
    assert name == "combined"   # window + GQA + softcap + sinks, the gpt-oss shape of a call
    return True, dict(window=(64, -1), softcap=30.0), dict(window=(64, -1), softcap=30.0)


@pytest.mark.parametrize("path,dtype", [("mfma_only", torch.bfloat16), ("exact", torch.float32)], ids=["mfma", "exact"])
@pytest.mark.parametrize("name", ["causal", "window", "mask", "block", "dropout", "softcap", "alibi", "combined"])
def test_features_with_sinks(name, path, dtype):
    import flashattention_lab_cuda as ext

    nq = nk = 300
    d = 128 if dtype != torch.float32 else 64
    hkv = 1 if name == "combined" else H
    q, k, v, do = make(B * H, B * hkv, nq, nk, d, dtype, seed=len(name))
    sinks = torch.tensor(SINKS, device=DEV)
    causal, kw, rkw = _feature(name, nq, nk, B * H)
    scale = d ** -0.5
    got = run(ext, path, q, k, v, do, sinks, causal, scale, **kw)
    ref = sr.sink_reference(q, k, v, do, sinks, causal, scale, **rkw)
    check(got, ref, dtype, f"{name} {path}")
    check_dsinks_against_own_outputs(got, do, sinks, f"{name} {path}")


# ---- packed sequences

def _varlen_inputs(lens, hq, hkv, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    total = sum(lens)
    q = torch.randn((total, hq, d), generator=g).to(dtype).to(DEV)
    k = torch.randn((total, hkv, d), generator=g).to(dtype).to(DEV)
    v = torch.randn((total, hkv, d), generator=g).to(dtype).to(DEV)
    do = torch.randn((total, hq, d), generator=g).to(dtype).to(DEV)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    return q, k, v, do, cu


def _varlen_reference(q, k, v, do, sinks, lens, causal, scale, window):
    """per sequence through sink_reference; o, dq (total, hq, d), dk, dv (total, hkv, d), lse (hq, total), dsinks (hq,)"""
    total, hq, d = q.shape
    o = torch.zeros((total, hq, d), dtype=torch.float64)
    dq, dk, dv = torch.zeros_like(o), torch.zeros(tuple(k.shape), dtype=torch.float64), torch.zeros(tuple(k.shape), dtype=torch.float64)
    lse = torch.zeros((hq, total))
    ds = torch.zeros((hq,), dtype=torch.float64)
    t0 = 0
    for n in lens:
        if n:
            sl = slice(t0, t0 + n)
            r = sr.sink_reference(q[sl].transpose(0, 1), k[sl].transpose(0, 1), v[sl].transpose(0, 1), do[sl].transpose(0, 1), sinks,
                                  causal, scale, window=window)
            o[sl], dq[sl], dk[sl], dv[sl] = (x.transpose(0, 1) for x in (r[0], r[2], r[3], r[4]))
            lse[:, sl] = r[1]
            if r[5] is not None:
                ds += r[5]
        t0 += n
    return o, lse, dq, dk, dv, ds


@pytest.mark.parametrize("path,dtype,d", [("auto", torch.bfloat16, 128), ("auto", torch.float16, 64), ("exact", torch.float32, 64)])
def test_varlen_with_gqa_causal_and_window(path, dtype, d):
    import flashattention_lab_cuda as ext

    lens, hq, hkv = (0, 1, 37, 130), 4, 2
    q, k, v, do, cu = _varlen_inputs(lens, hq, hkv, d, dtype, seed=d)
    sinks = torch.tensor(SINKS, device=DEV)
    scale = d ** -0.5
    kw = dict(window=(20, -1))
    ext.set_option("ex_path", PATHS[path])
    try:
        o, lse = ext.ex_varlen_forward(q, k, v, cu, cu, 130, 130, True, scale, sinks=sinks, **kw)
        dq, dk, dv, ds = ext.ex_varlen_backward(q, k, v, o, do, lse, cu, cu, 130, 130, True, scale, sinks=sinks, **kw)
        ds2 = ext.ex_varlen_backward(q, k, v, o, do, lse, cu, cu, 130, 130, True, scale, sinks=sinks, **kw)[3]
        off = torch.full((hq,), NEG_INF, device=DEV)
        o_off, lse_off = ext.ex_varlen_forward(q, k, v, cu, cu, 130, 130, True, scale, sinks=off, **kw)
        ds_off = ext.ex_varlen_backward(q, k, v, o_off, do, lse_off, cu, cu, 130, 130, True, scale, sinks=off, **kw)[3]
        o_no, lse_no = ext.ex_varlen_forward(q, k, v, cu, cu, 130, 130, True, scale, **kw)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    ref = _varlen_reference(q, k, v, do, sinks, lens, True, scale, (20, -1))
    check((o, lse, dq, dk, dv, ds), ref, dtype, f"varlen {path} {dtype}")
    assert torch.equal(ds, ds2)
    # sinks at -inf: the call without sinks, bit for bit, and a zero gradient
    assert torch.equal(o_off, o_no) and torch.equal(lse_off, lse_no)
    assert torch.equal(ds_off, torch.zeros_like(ds_off))


# ---- rows without a visible key, the range of the sink, -inf

@pytest.mark.parametrize("path,dtype,d", [("mfma_only", torch.bfloat16, 128), ("mfma_only", torch.float16, 64), ("exact", torch.float32, 64)])
def test_rows_without_a_visible_key(path, dtype, d):
    """Causal with (Nq, Nk) = (48, 16): rows 0 .. 31 see no key — o = 0 and lse = the head's sink exactly, dq = 0."""
    import flashattention_lab_cuda as ext

    nq, nk = 48, 16
    q, k, v, do = make(B * H, B * H, nq, nk, d, dtype, seed=5)
    sinks = torch.tensor(SINKS, device=DEV)
    got = run(ext, path, q, k, v, do, sinks, True, d ** -0.5)
    o, lse, dq = got[0].cpu(), got[1].cpu(), got[2].cpu()
    assert torch.equal(o[:, :32], torch.zeros_like(o[:, :32]))
    assert torch.equal(lse[:, :32], torch.tensor(SINKS).repeat(B).view(B * H, 1).expand(B * H, 32))
    assert torch.equal(dq[:, :32], torch.zeros_like(dq[:, :32]))
    check(got, sr.sink_reference(q, k, v, do, sinks, True, d ** -0.5), dtype, f"dead rows {path}")


@pytest.mark.parametrize("path,dtype,d", [("mfma_only", torch.bfloat16, 128), ("exact", torch.float32, 64)])
def test_huge_sinks_stay_finite(path, dtype, d):
    import flashattention_lab_cuda as ext

    q, k, v, do = make(B * H, B * H, 160, 160, d, dtype, seed=9)
    sinks = torch.tensor([-1e4, 1e4, 0.3, -3.0], device=DEV)
    got = run(ext, path, q, k, v, do, sinks, True, d ** -0.5)
    for t in got:
        assert bool(torch.isfinite(t).all())
    check(got, sr.sink_reference(q, k, v, do, sinks, True, d ** -0.5), dtype, f"huge {path}")
    o, lse = got[0].cpu(), got[1].cpu()
    assert torch.equal(o[1::H], torch.zeros_like(o[1::H]))                 # +1e4 takes all the weight: o rounds to 0
    torch.testing.assert_close(lse[1::H], torch.full_like(lse[1::H], 1e4), rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("path,dtype,d,kw", [
    ("mfma_only", torch.bfloat16, 128, {}), ("mfma_only", torch.float16, 64, dict(dropout_p=0.1, seed=3)),
    ("auto", torch.bfloat16, 128, dict(window=(64, -1))), ("exact", torch.float32, 64, {}), ("exact", torch.bfloat16, 64, dict(softcap=20.0))],
    ids=["mfma", "mfma-drop", "auto-window", "exact", "exact-cap"])
def test_minus_inf_is_the_call_without_sinks(path, dtype, d, kw):
    """Heads at -inf: o and lse are the bits of the call without sinks (on the same kernel family), dsinks exactly 0."""
    import flashattention_lab_cuda as ext

    q, k, v, do = make(B * H, B * 2, 300, 300, d, dtype, seed=13)
    base = run(ext, path, q, k, v, do, None, True, d ** -0.5, **kw)
    off = run(ext, path, q, k, v, do, torch.full((H,), NEG_INF, device=DEV), True, d ** -0.5, **kw)
    assert torch.equal(off[0], base[0]) and torch.equal(off[1], base[1])
    assert torch.equal(off[5], torch.zeros_like(off[5]))
    for a, b in zip(off[2:5], base[2:5]):
        assert torch.equal(a, b)
    # two heads off, two on: the heads that are off keep the bits, the others change
    mixed = torch.tensor([NEG_INF, 0.5, NEG_INF, -1.0], device=DEV)
    part = run(ext, path, q, k, v, do, mixed, True, d ** -0.5, **kw)
    for h in (0, 2):
        assert torch.equal(part[0][h::H], base[0][h::H]) and torch.equal(part[1][h::H], base[1][h::H])
        assert part[5][h].item() == 0.0
    assert not torch.equal(part[1][1::H], base[1][1::H]) and part[5][1].item() != 0.0
    assert bool(torch.isfinite(part[5]).all())


@pytest.mark.parametrize("path,dtype,d", [("mfma_only", torch.bfloat16, 128), ("exact", torch.float32, 64)])
def test_dsinks_are_deterministic(path, dtype, d):
    import flashattention_lab_cuda as ext

    q, k, v, do = make(B * H, B * H, 300, 300, d, dtype, seed=17)
    sinks = torch.tensor(SINKS, device=DEV)
    a = run(ext, path, q, k, v, do, sinks, True, d ** -0.5, dropout_p=0.1, seed=5)
    b = run(ext, path, q, k, v, do, sinks, True, d ** -0.5, dropout_p=0.1, seed=5)
    assert torch.equal(a[5], b[5]) and bool((a[5] != 0).all())


# ---- autograd

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_autograd_gives_sinks_a_float32_gradient(dtype):
    from common.attention_ex import flash_attention_ex, flash_attention_varlen

    d, nq, nk = 64, 160, 160
    g = torch.Generator().manual_seed(23)
    q = torch.randn((B, H, nq, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    k = torch.randn((B, 2, nk, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    v = torch.randn((B, 2, nk, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    do = torch.randn((B, H, nq, d), generator=g).to(dtype).to(DEV)
    sinks = torch.tensor(SINKS, device=DEV, requires_grad=True)
    o = flash_attention_ex(q, k, v, causal=True, window_size=(64, -1), sinks=sinks)
    (o * do).sum().backward()
    ref = sr.sink_reference(q.reshape(B * H, nq, d), k.reshape(B * 2, nk, d), v.reshape(B * 2, nk, d), do.reshape(B * H, nq, d), sinks,
                            True, d ** -0.5, window=(64, -1))
    tol = dtype_tolerances(dtype)
    assert sinks.grad.dtype == torch.float32 and sinks.grad.shape == (H,)
    torch.testing.assert_close(o.detach().cpu().double().reshape(B * H, nq, d), ref[0], **tol)
    torch.testing.assert_close(sinks.grad.cpu().double(), ref[5], **tol)
    torch.testing.assert_close(q.grad.cpu().double().reshape(B * H, nq, d), ref[2], **tol)
    torch.testing.assert_close(k.grad.cpu().double().reshape(B * 2, nk, d), ref[3], **tol)
    # a bf16 parameter passed as p.float() receives its gradient through the cast
    p = torch.tensor(SINKS, device=DEV).to(torch.bfloat16).requires_grad_(True)
    o2 = flash_attention_ex(q.detach(), k.detach(), v.detach(), causal=True, window_size=(64, -1), sinks=p.float())
    (o2 * do).sum().backward()
    assert p.grad is not None and p.grad.dtype == torch.bfloat16 and bool((p.grad != 0).any())
    ref2 = sr.sink_reference(q.reshape(B * H, nq, d), k.reshape(B * 2, nk, d), v.reshape(B * 2, nk, d), do.reshape(B * H, nq, d),
                             p.detach().float(), True, d ** -0.5, window=(64, -1))
    torch.testing.assert_close(p.grad.cpu().double(), ref2[5], rtol=5e-2, atol=5e-2)
    # packed sequences
    lens = (0, 1, 37, 130)
    qv, kv, vv, dov, cu = _varlen_inputs(lens, H, 2, d, dtype, seed=29)
    qv.requires_grad_(True)
    sv = torch.tensor(SINKS, device=DEV, requires_grad=True)
    ov = flash_attention_varlen(qv, kv, vv, cu, cu, 130, 130, causal=True, sinks=sv)
    (ov * dov).sum().backward()
    rv = _varlen_reference(qv.detach(), kv, vv, dov, sv.detach(), lens, True, d ** -0.5, (-1, -1))
    assert sv.grad.dtype == torch.float32
    torch.testing.assert_close(ov.detach().cpu().double(), rv[0], **tol)
    torch.testing.assert_close(sv.grad.cpu().double(), rv[5], **tol)
    torch.testing.assert_close(qv.grad.cpu().double(), rv[2], **tol)


# ---- KV-cache decoding

KB, KHQ, KHKV, KD, KCAP = 3, 8, 2, 128, 300
KLENS = (0, 17, 290)
KSINKS = (0.6, -1.5, 2.5, 0.0, NEG_INF, 1.0, -0.5, 3.0)


def _kv_inputs(nq, nnew, dtype, seed, cap=KCAP):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((KB, nq, KHQ, KD), generator=g).to(dtype).to(DEV)
    kc = torch.randn((KB, cap, KHKV, KD), generator=g).to(dtype).to(DEV)
    vc = torch.randn((KB, cap, KHKV, KD), generator=g).to(dtype).to(DEV)
    kn = torch.randn((KB, nnew, KHKV, KD), generator=g).to(dtype).to(DEV) if nnew else None
    vn = torch.randn((KB, nnew, KHKV, KD), generator=g).to(dtype).to(DEV) if nnew else None
    return q, kc, vc, kn, vn


def _kv_reference(q, ks, vs, sinks, causal, window, scale, softcap=0.0):
    """o (B, Nq, H_q, d) fp64 and lse (B, H_q, Nq): sequence b over the tokens ks[b], vs[b] ((len_k, H_kv, d) each), by sink_ref"""
    b, nq, hq, d = q.shape
    o = torch.zeros((b, nq, hq, d), dtype=torch.float64)
    lse = torch.zeros((b, hq, nq))
    for bb in range(b):
        if ks[bb].shape[0] == 0:   # no key: o = 0, lse = the sink
            lse[bb] = sinks.detach().cpu().float().view(hq, 1).expand(hq, nq)
            continue
        r = sr.sink_reference(q[bb].transpose(0, 1), ks[bb].transpose(0, 1), vs[bb].transpose(0, 1), None, sinks, causal, scale,
                              window=window, softcap=softcap)
        o[bb], lse[bb] = r[0].transpose(0, 1), r[1]
    return o, lse


def _kv_check(o, lse, ro, rlse, dtype, what=""):
    torch.testing.assert_close(o.cpu().double(), ro, **dtype_tolerances(dtype), msg=lambda m: f"o {what}: {m}")
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse.cpu()), fin), f"lse -inf pattern {what}"
    torch.testing.assert_close(lse.cpu()[fin], rlse[fin], rtol=1e-3, atol=1e-3, msg=lambda m: f"lse {what}: {m}")


@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("nnew", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_decode_matches_the_reference(dtype, nnew, nq):
    import flashattention_lab_cuda as ext

    q, kc, vc, kn, vn = _kv_inputs(nq, nnew, dtype, seed=nq + 10 * nnew)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    sinks = torch.tensor(KSINKS, device=DEV)
    kref, vref = kc.cpu().clone(), vc.cpu().clone()
    for bb, n in enumerate(KLENS):
        if nnew:
            kref[bb, n:n + nnew], vref[bb, n:n + nnew] = kn[bb].cpu(), vn[bb].cpu()
    ks = [kref[bb, :n + nnew] for bb, n in enumerate(KLENS)]
    vs = [vref[bb, :n + nnew] for bb, n in enumerate(KLENS)]
    ro, rlse = _kv_reference(q.cpu(), ks, vs, sinks, True, (-1, -1), KD ** -0.5)
    for splits in (0, 1, 2, 4):   # (a request of 1 still runs the combine, on two splits)
        k2, v2 = kc.clone(), vc.clone()
        o, lse = ext.ex_kvcache_forward(q, k2, v2, kn, vn, lens, True, None, num_splits=splits, sinks=sinks)
        torch.cuda.synchronize()
        _kv_check(o, lse, ro, rlse, dtype, f"nq={nq} nnew={nnew} S={splits}")
        assert torch.equal(k2.cpu(), kref) and torch.equal(v2.cpu(), vref)
        if nnew == 0:   # the empty sequence has no key: o = 0 and lse = the sink exactly (-inf for the head without one)
            assert torch.equal(o[0], torch.zeros_like(o[0]))
            assert torch.equal(lse[0].cpu(), torch.tensor(KSINKS).view(KHQ, 1).expand(KHQ, nq))


@pytest.mark.parametrize("splits", [2, 4])
def test_decode_minus_inf_is_the_call_without_sinks(splits):
    import flashattention_lab_cuda as ext

    q, kc, vc, _, _ = _kv_inputs(3, 0, torch.bfloat16, seed=31)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    o0, lse0 = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=splits)
    o1, lse1 = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, num_splits=splits,
                                      sinks=torch.full((KHQ,), NEG_INF, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)


def test_decode_paged():
    import flashattention_lab_cuda as ext

    ps, dtype = 16, torch.bfloat16
    q, kc, vc, kn, vn = _kv_inputs(1, 1, dtype, seed=37, cap=304)      # 19 pages a sequence
    mb = 304 // ps
    nblk = KB * mb + 5
    table = torch.randperm(nblk, generator=torch.Generator().manual_seed(1))[:KB * mb].view(KB, mb).to(torch.int32)
    kp = torch.zeros((nblk, ps, KHKV, KD), dtype=dtype, device=DEV)
    vp = torch.zeros_like(kp)
    idx = table.reshape(-1).long().to(DEV)
    kp[idx] = kc.reshape(KB * mb, ps, KHKV, KD)
    vp[idx] = vc.reshape(KB * mb, ps, KHKV, KD)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    sinks = torch.tensor(KSINKS, device=DEV)
    o, lse = ext.ex_kvcache_forward(q, kp, vp, kn, vn, lens, True, None, block_table=table.to(DEV), sinks=sinks)
    torch.cuda.synchronize()
    ks = [torch.cat([kc[bb, :n].cpu(), kn[bb].cpu()]) for bb, n in enumerate(KLENS)]
    vs = [torch.cat([vc[bb, :n].cpu(), vn[bb].cpu()]) for bb, n in enumerate(KLENS)]
    ro, rlse = _kv_reference(q.cpu(), ks, vs, sinks, True, (-1, -1), KD ** -0.5)
    _kv_check(o, lse, ro, rlse, dtype, "paged")


def test_decode_leftpad_and_window():
    import flashattention_lab_cuda as ext

    dtype = torch.float16
    q, kc, vc, _, _ = _kv_inputs(3, 0, dtype, seed=41)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    pad = (0, 5, 100)
    sinks = torch.tensor(KSINKS, device=DEV)
    ks = [kc[bb, p:n].cpu() for bb, (p, n) in enumerate(zip(pad, KLENS))]
    vs = [vc[bb, p:n].cpu() for bb, (p, n) in enumerate(zip(pad, KLENS))]
    o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, cache_leftpad=torch.tensor(pad, dtype=torch.int32, device=DEV),
                                    sinks=sinks)
    ro, rlse = _kv_reference(q.cpu(), ks, vs, sinks, True, (-1, -1), KD ** -0.5)
    _kv_check(o, lse, ro, rlse, dtype, "leftpad")
    ks = [kc[bb, :n].cpu() for bb, n in enumerate(KLENS)]
    vs = [vc[bb, :n].cpu() for bb, n in enumerate(KLENS)]
    o, lse = ext.ex_kvcache_forward(q, kc, vc, None, None, lens, True, None, window=(40, -1), softcap=20.0, sinks=sinks)
    ro, rlse = _kv_reference(q.cpu(), ks, vs, sinks, True, (40, -1), KD ** -0.5, softcap=20.0)
    _kv_check(o, lse, ro, rlse, dtype, "window")


def test_decode_rotary():
    import flashattention_lab_cuda as ext
    from tests.kvcache_rotary_ref import rotate64, tables

    dtype, nq = torch.bfloat16, 1
    q, kc, vc, kn, vn = _kv_inputs(nq, 1, dtype, seed=43)
    cos, sin = tables(KCAP + 8, 64, dtype)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    sinks = torch.tensor(KSINKS, device=DEV)
    o, lse = ext.ex_kvcache_forward(q, kc, vc, kn, vn, lens, True, None, rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV),
                                    rotary_interleaved=True, sinks=sinks)
    torch.cuda.synchronize()
    # the gathered cache after the call holds the rotated new key; q token i is rotated at position L_b + i
    ks = [kc[bb, :n + 1].cpu() for bb, n in enumerate(KLENS)]
    vs = [vc[bb, :n + 1].cpu() for bb, n in enumerate(KLENS)]
    qr = torch.stack([rotate64(q[bb].cpu(), cos, sin, [n + i for i in range(nq)], True) for bb, n in enumerate(KLENS)])
    ro, rlse = _kv_reference(qr, ks, vs, sinks, True, (-1, -1), KD ** -0.5)
    _kv_check(o, lse, ro, rlse, dtype, "rotary")


def test_decode_e4m3_cache():
    import flashattention_lab_cuda as ext
    from tests.kvcache_fp8_ref import E4M3, absmax_scales, dequantize, quantize

    dtype = torch.bfloat16
    q, kc, vc, _, _ = _kv_inputs(3, 0, dtype, seed=47)
    kd, vd = absmax_scales(kc.cpu()), absmax_scales(vc.cpu())
    k8, v8 = quantize(kc.cpu(), kd), quantize(vc.cpu(), vd)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    sinks = torch.tensor(KSINKS, device=DEV)
    o, lse = ext.ex_kvcache_forward(q, k8.to(DEV).view(E4M3), v8.to(DEV).view(E4M3), None, None, lens, True, None, k_descale=kd.to(DEV),
                                    v_descale=vd.to(DEV), sinks=sinks)
    kdq, vdq = dequantize(k8, kd), dequantize(v8, vd)
    ro, rlse = _kv_reference(q.cpu(), [kdq[bb, :n] for bb, n in enumerate(KLENS)], [vdq[bb, :n] for bb, n in enumerate(KLENS)], sinks,
                             True, (-1, -1), KD ** -0.5)
    _kv_check(o, lse, ro, rlse, dtype, "e4m3")


def test_decode_graph_capture_with_changing_sinks():
    from common.attention_ex import flash_attn_with_kvcache

    dtype = torch.bfloat16
    q, kc, vc, _, _ = _kv_inputs(1, 0, dtype, seed=53)
    lens = torch.tensor(KLENS, dtype=torch.int32, device=DEV)
    sinks = torch.tensor(KSINKS, device=DEV)
    flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, sinks=sinks)   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, sinks=sinks)
    torch.cuda.current_stream().wait_stream(s)
    ks = [kc[bb, :n].cpu() for bb, n in enumerate(KLENS)]
    vs = [vc[bb, :n].cpu() for bb, n in enumerate(KLENS)]
    for new in (KSINKS, tuple(-x for x in KSINKS[:4]) + (2.0, NEG_INF, 1e4, -1e4)):
        sinks.copy_(torch.tensor(new))
        graph.replay()
        torch.cuda.synchronize()
        ro, rlse = _kv_reference(q.cpu(), ks, vs, sinks, True, (-1, -1), KD ** -0.5)
        _kv_check(out[0], out[1], ro, rlse, dtype, f"graph {new}")
        assert bool(torch.isfinite(out[0]).all())
