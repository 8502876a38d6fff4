"""GPU: score modifiers (softcap, ALiBi slopes) on the extended path — fa_ex_*_scoremod through flashattention_lab_cuda and the
autograd wrappers — against the fp64 reference of tests/test_scoremod_cpu.py, on the 16-bit MFMA kernels (FEAT bit 4) and the
exact-f32 ones."""
import ctypes

import pytest
import torch

from tests.helpers import dtype_tolerances
from tests.test_scoremod_cpu import scoremod_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = {"auto": 0, "exact": 1, "mfma_only": 3}


def alibi_standard(h):
    """The standard ALiBi slopes 2^(-8 (i + 1) / H)."""
    return torch.tensor([2.0 ** (-8.0 * (i + 1) / h) for i in range(h)], dtype=torch.float32)


def make(bh, bh_kv, nq, nk, d, dtype, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((bh, nq, d), generator=g) * amp).to(dtype).to(DEV)
    k = torch.randn((bh_kv, nk, d), generator=g).to(dtype).to(DEV)
    v = torch.randn((bh_kv, nk, d), generator=g).to(dtype).to(DEV)
    do = torch.randn((bh, nq, d), generator=g).to(dtype).to(DEV)
    return q, k, v, do


def run(ext, path, q, k, v, do, causal, scale, **kw):
    ext.set_option("ex_path", PATHS[path])
    try:
        o, lse = ext.ex_forward(q, k, v, causal, scale, **kw)
        dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, causal, scale, **kw)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def check(got, ref, dtype, what=""):
    tol = dtype_tolerances(dtype)
    o, lse, dq, dk, dv = (t.cpu() for t in got)
    ro, rlse, rdq, rdk, rdv = ref
    torch.testing.assert_close(o.double(), ro, **tol, msg=lambda m: f"o {what}: {m}")
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin), f"lse -inf pattern {what}"
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-3, atol=1e-3, msg=lambda m: f"lse {what}: {m}")
    for name, a, b in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        torch.testing.assert_close(a.double(), b, **tol, msg=lambda m, n=name: f"{n} {what}: {m}")


CASES = [
    # bh, g, nq, nk, d, dtype, causal, softcap, alibi, extra, path
    (4, 1, 300, 300, 128, torch.bfloat16, True, 20.0, False, {}, "mfma_only"),
    (4, 1, 200, 333, 64, torch.float16, False, 0.0, True, {}, "auto"),
    (4, 1, 400, 260, 128, torch.bfloat16, True, 10.0, True, {}, "mfma_only"),                     # Nq > Nk: dead rows
    (4, 1, 260, 400, 96, torch.bfloat16, False, 8.0, True, {"window": (64, 32)}, "mfma_only"),
    (2, 1, 256, 320, 64, torch.float16, False, 15.0, True, {"mask": "bh"}, "mfma_only"),
    (2, 1, 300, 300, 128, torch.bfloat16, True, 12.0, True, {"block": 64}, "mfma_only"),
    (4, 1, 257, 300, 128, torch.bfloat16, True, 25.0, True, {"dropout_p": 0.2, "seed": 77}, "mfma_only"),
    (8, 4, 300, 300, 128, torch.bfloat16, True, 9.0, True, {}, "auto"),                           # GQA g = 4
    (8, 4, 200, 280, 64, torch.float16, False, 6.0, True, {"window": (90, -1), "dropout_p": 0.1, "seed": 5}, "mfma_only"),
    (4, 1, 300, 300, 128, torch.bfloat16, False, 7.0, True, {}, "exact"),
    (4, 1, 200, 280, 64, torch.float32, True, 5.0, True, {}, "auto"),
    (4, 4, 150, 170, 36, torch.float16, False, 4.0, True, {"window": (40, 10)}, "auto"),         # d = 36: exact f32
    (2, 1, 130, 200, 256, torch.bfloat16, True, 30.0, True, {"dropout_p": 0.1, "seed": 9}, "auto"),  # d = 256: exact f32
    (2, 2, 140, 120, 256, torch.float32, False, 0.0, True, {"mask": "bh"}, "auto"),
    (4, 1, 257, 300, 64, torch.float16, True, 3.0, False, {"block": 32}, "exact"),
]


def _extra(extra, bh, nq, nk, seed):
    kw, ref = {}, {}
    g = torch.Generator().manual_seed(seed + 100)
    if "window" in extra:
        kw["window"] = ref["window"] = extra["window"]
    if extra.get("mask") == "bh":
        m = (torch.rand((bh, nq, nk), generator=g) > 0.3).to(torch.uint8)
        m[0, :5] = 0   # dead rows
        m[1 % bh, :, 7] = 0
        kw["mask"], ref["mask"] = m.to(DEV), m
    if "block" in extra:
        blk = extra["block"]
        bm = (torch.rand(((nq + blk - 1) // blk, (nk + blk - 1) // blk), generator=g) > 0.35).to(torch.uint8)
        bm[0, 0] = 1
        kw.update(block_mask=bm.to(DEV), br=blk, bc=blk)
        ref.update(block_mask=bm, br=blk, bc=blk)
    if "dropout_p" in extra:
        kw.update(dropout_p=extra["dropout_p"], seed=extra["seed"])
        ref.update(dropout_p=extra["dropout_p"], seed=extra["seed"])
    return kw, ref


@pytest.mark.parametrize("case", CASES)
def test_scoremod_matches_the_reference(case):
    import flashattention_lab_cuda as ext

    bh, g, nq, nk, d, dtype, causal, cap, alibi, extra, path = case
    q, k, v, do = make(bh, bh // g, nq, nk, d, dtype, seed=nq + d)
    slopes = (alibi_standard(bh) * 4.0).to(DEV) if alibi else None
    kw, rkw = _extra(extra, bh, nq, nk, nq)
    scale = d ** -0.5
    got = run(ext, path, q, k, v, do, causal, scale, softcap=cap, alibi_slopes=slopes, **kw)
    ref = scoremod_reference(q, k, v, do, causal, scale, softcap=cap, slopes=slopes, **rkw)
    check(got, ref, dtype, f"{case}")


@pytest.mark.parametrize("path,dtype,d", [("mfma_only", torch.bfloat16, 128), ("mfma_only", torch.float16, 64),
                                          ("exact", torch.float32, 128)])
def test_saturating_softcap(path, dtype, d):
    """|s| about 20 against softcap 5: tanh saturates (2^x overflows to inf, or underflows to 0, in the 16-bit kernels' form)."""
    import flashattention_lab_cuda as ext

    q, k, v, do = make(4, 4, 256, 300, d, dtype, seed=3, amp=20.0)
    scale = d ** -0.5
    for causal in (False, True):
        got = run(ext, path, q, k, v, do, causal, scale, softcap=5.0)
        ref = scoremod_reference(q, k, v, do, causal, scale, softcap=5.0)
        assert ref[0].abs().max() > 0 and (q.float().cpu() @ k.float().cpu().transpose(1, 2) * scale).abs().max() > 15
        check(got, ref, dtype, f"saturating {causal}")


@pytest.mark.parametrize("path,dtype,d", [("mfma_only", torch.bfloat16, 64), ("auto", torch.float16, 128), ("exact", torch.bfloat16, 64)])
def test_large_alibi_slopes_both_sides_of_the_diagonal(path, dtype, d):
    """Non-causal, N = 2048, slopes up to 0.5: the bias reaches about -1000 on both sides of the diagonal, and the running max
    moves by far more than the lazy rescale's threshold from tile to tile."""
    import flashattention_lab_cuda as ext

    bh, n = 2, 2048
    q, k, v, do = make(bh, bh, n, n, d, dtype, seed=21)
    slopes = torch.tensor([0.5, 0.05], dtype=torch.float32, device=DEV)
    scale = d ** -0.5
    got = run(ext, path, q, k, v, do, False, scale, alibi_slopes=slopes, softcap=0.0)
    ref = scoremod_reference(q, k, v, do, False, scale, slopes=slopes)
    check(got, ref, dtype, "large alibi")


@pytest.mark.parametrize("path", ["mfma_only", "auto"])
def test_no_modifiers_is_the_window_call_bit_for_bit(path):
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_ex

    lib = ext._lib
    for dtype, d, causal, nq, nk in ((torch.bfloat16, 128, True, 300, 300), (torch.float16, 64, False, 200, 333),
                                     (torch.float32, 64, True, 130, 130)):
        if dtype == torch.float32 and path == "mfma_only":
            continue   # (f32 tensors have no MFMA kernels: ex_path 3 fails them, with or without modifiers)
        q, k, v, _ = make(4, 4, nq, nk, d, dtype, seed=d)
        code = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dtype]
        outs = []
        ext.set_option("ex_path", PATHS[path])
        try:
            for fn in ("window", "scoremod"):
                o, lse = torch.empty_like(q), torch.empty((4, nq), dtype=torch.float32, device=DEV)
                ptrs = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), 4, 1, nq, nk, d, code, int(causal), -1, -1,
                        d ** -0.5)
                if fn == "window":
                    rc = lib.fa_ex_forward_window(*ptrs, None, 0, None, 128, 128, 0.0, 0, None)
                else:
                    rc = lib.fa_ex_forward_scoremod(*ptrs, 0.0, None, 1, 0, None, 0, None, 128, 128, 0.0, 0, None)
                assert rc == 0, lib.fa_last_error()
                torch.cuda.synchronize()
                outs.append((o, lse))
        finally:
            ext.set_option("ex_path", 0)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        # through the autograd wrapper, forward and backward
        grads = []
        ext.set_option("ex_path", PATHS[path])
        try:
            for kw in ({}, {"softcap": 0.0, "alibi_slopes": None}):
                qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
                o = flash_attention_ex(qg, kg, vg, causal=causal, **kw)
                o.backward(torch.ones_like(o))
                grads.append((o.detach(), qg.grad, kg.grad, vg.grad))
        finally:
            ext.set_option("ex_path", 0)
        for a, b in zip(*grads):
            assert torch.equal(a, b)


@pytest.mark.parametrize("path", ["mfma_only", "exact"])
def test_dead_rows_and_keys_and_dropout_repeatability(path):
    import flashattention_lab_cuda as ext

    bh, nq, nk, d, dtype = 2, 300, 200, 128, torch.bfloat16
    q, k, v, do = make(bh, bh, nq, nk, d, dtype, seed=8)
    mask = torch.ones((nq, nk), dtype=torch.uint8)
    mask[:, 50] = 0    # a key no row sees
    slopes = torch.tensor([-0.02, 0.3], dtype=torch.float32, device=DEV)   # (a negative slope as well)
    kw = dict(softcap=6.0, alibi_slopes=slopes, mask=mask.to(DEV), dropout_p=0.25, seed=4242)
    a = run(ext, path, q, k, v, do, True, d ** -0.5, **kw)
    b = run(ext, path, q, k, v, do, True, d ** -0.5, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    o, lse, dq, dk, dv = a
    dead = nq - nk   # causal with Nq > Nk: rows i < Nq - Nk see no key
    assert torch.all(o[:, :dead] == 0) and torch.all(lse[:, :dead] == float("-inf")) and torch.all(dq[:, :dead] == 0)
    assert torch.all(dk[:, 50] == 0) and torch.all(dv[:, 50] == 0)
    assert all(torch.isfinite(t).all() for t in (o, dq, dk, dv))
    ref = scoremod_reference(q, k, v, do, True, d ** -0.5, softcap=6.0, slopes=slopes, mask=mask, dropout_p=0.25, seed=4242)
    check(a, ref, dtype, "dead rows / dropout")


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _varlen_reference(q, k, v, do, lens_q, lens_k, causal, scale, cap, slopes_bh):
    """Sequence by sequence through scoremod_reference; slopes_bh (batch, H_q)."""
    hq = q.shape[1]
    out = [torch.zeros(q.shape, dtype=torch.float64), torch.full((hq, q.shape[0]), float("-inf")),
           torch.zeros(q.shape, dtype=torch.float64), torch.zeros(k.shape, dtype=torch.float64), torch.zeros(v.shape, dtype=torch.float64)]
    sq = sk = 0
    for b, (lq, lk) in enumerate(zip(lens_q, lens_k)):
        if lq > 0 and lk > 0:
            qb, kb, vb, dob = (t.transpose(0, 1) for t in (q[sq:sq + lq], k[sk:sk + lk], v[sk:sk + lk], do[sq:sq + lq]))
            o, lse, dq, dk, dv = scoremod_reference(qb, kb, vb, dob, causal, scale, softcap=cap, slopes=slopes_bh[b])
            out[0][sq:sq + lq] = o.transpose(0, 1)
            out[1][:, sq:sq + lq] = lse
            out[2][sq:sq + lq] = dq.transpose(0, 1)
            out[3][sk:sk + lk] = dk.transpose(0, 1)
            out[4][sk:sk + lk] = dv.transpose(0, 1)
        sq += lq
        sk += lk
    return out


@pytest.mark.parametrize("path,dtype,d,hkv", [("mfma_only", torch.bfloat16, 128, 2), ("auto", torch.float16, 64, 4),
                                              ("exact", torch.bfloat16, 64, 1), ("auto", torch.float32, 40, 2)])
def test_varlen_scoremod(path, dtype, d, hkv):
    import flashattention_lab_cuda as ext

    lens_q, lens_k, hq = [255, 0, 1, 300, 130], [300, 7, 40, 300, 0], 4
    g = torch.Generator().manual_seed(d)
    q = torch.randn((sum(lens_q), hq, d), generator=g).to(dtype).to(DEV)
    k = torch.randn((sum(lens_k), hkv, d), generator=g).to(dtype).to(DEV)
    v = torch.randn((sum(lens_k), hkv, d), generator=g).to(dtype).to(DEV)
    do = torch.randn((sum(lens_q), hq, d), generator=g).to(dtype).to(DEV)
    slopes = (torch.rand((len(lens_q), hq), generator=g) * 0.5).to(DEV)   # (B, H)
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)
    scale, cap = d ** -0.5, 8.0
    for causal in (True, False):
        ext.set_option("ex_path", PATHS[path])
        try:
            o, lse = ext.ex_varlen_forward(q, k, v, cu_q, cu_k, max(lens_q), max(lens_k), causal, scale, softcap=cap, alibi_slopes=slopes)
            dq, dk, dv = ext.ex_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max(lens_q), max(lens_k), causal, scale, softcap=cap,
                                                alibi_slopes=slopes)
        finally:
            ext.set_option("ex_path", 0)
        torch.cuda.synchronize()
        ref = _varlen_reference(q.cpu(), k.cpu().repeat_interleave(hq // hkv, 1), v.cpu().repeat_interleave(hq // hkv, 1), do.cpu(),
                                lens_q, lens_k, causal, scale, cap, slopes.cpu())
        g_ = hq // hkv
        ref[3] = ref[3].reshape(-1, hkv, g_, d).sum(2)
        ref[4] = ref[4].reshape(-1, hkv, g_, d).sum(2)
        check((o, lse, dq, dk, dv), ref, dtype, f"varlen {causal}")
        if path != "mfma_only":
            continue
        # every sequence equals the same sequence alone through fa_ex_*_scoremod with its batch row of slopes, bit for bit
        sq = sk = 0
        for b, (lq, lk) in enumerate(zip(lens_q, lens_k)):
            if lq > 0 and lk > 0:
                qb, kb, vb, dob = (t.transpose(0, 1).contiguous() for t in (q[sq:sq + lq], k[sk:sk + lk], v[sk:sk + lk], do[sq:sq + lq]))
                ext.set_option("ex_path", 3)
                try:
                    ob, lb = ext.ex_forward(qb, kb, vb, causal, scale, softcap=cap, alibi_slopes=slopes[b].contiguous())
                    dqb, dkb, dvb = ext.ex_backward(qb, kb, vb, ob, dob, lb, causal, scale, softcap=cap, alibi_slopes=slopes[b].contiguous())
                finally:
                    ext.set_option("ex_path", 0)
                assert torch.equal(o[sq:sq + lq], ob.transpose(0, 1)), (b, "o")
                assert torch.equal(lse[:, sq:sq + lq], lb), (b, "lse")
                assert torch.equal(dq[sq:sq + lq], dqb.transpose(0, 1)), (b, "dq")
                assert torch.equal(dk[sk:sk + lk], dkb.transpose(0, 1)), (b, "dk")
                assert torch.equal(dv[sk:sk + lk], dvb.transpose(0, 1)), (b, "dv")
            sq += lq
            sk += lk


def test_flash_attention_ex_autograd_gqa_bh_slopes():
    from common.attention_ex import flash_attention_ex

    b, h, hkv, n, d, dtype, tau, cap = 2, 8, 2, 300, 128, torch.bfloat16, 0.7, 10.0
    g = torch.Generator().manual_seed(12)
    q = torch.randn((b, h, n, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    k = torch.randn((b, hkv, n, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    v = torch.randn((b, hkv, n, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    do = torch.randn((b, h, n, d), generator=g).to(dtype).to(DEV)
    slopes = (alibi_standard(h).repeat(b, 1) * torch.tensor([[1.0], [2.0]])).to(DEV).requires_grad_(True)   # (B, H)
    o = flash_attention_ex(q, k, v, tau=tau, causal=True, softcap=cap, alibi_slopes=slopes)
    o.backward(do)
    assert slopes.grad is None
    scale = tau / d ** 0.5
    ref = scoremod_reference(q.reshape(b * h, n, d), k.reshape(b * hkv, n, d), v.reshape(b * hkv, n, d), do.reshape(b * h, n, d), True,
                             scale, softcap=cap, slopes=slopes.reshape(-1))
    tol = dtype_tolerances(dtype)
    torch.testing.assert_close(o.detach().cpu().double().reshape(b * h, n, d), ref[0], **tol)
    for a, r in ((q.grad, ref[2]), (k.grad, ref[3]), (v.grad, ref[4])):
        torch.testing.assert_close(a.cpu().double().reshape(r.shape), r, **tol)
    # (H,) slopes: the same as the (B, H) tensor of identical rows
    q.grad = k.grad = v.grad = None
    s1 = alibi_standard(h).to(DEV)
    o1 = flash_attention_ex(q, k, v, tau=tau, causal=True, softcap=cap, alibi_slopes=s1)
    o2 = flash_attention_ex(q, k, v, tau=tau, causal=True, softcap=cap, alibi_slopes=s1.repeat(b, 1))
    assert torch.equal(o1, o2)


def test_flash_attention_varlen_autograd_h_slopes():
    from common.attention_ex import flash_attention_varlen

    lens, hq, hkv, d, dtype = [300, 1, 200, 256], 8, 2, 128, torch.bfloat16
    g = torch.Generator().manual_seed(4)
    t = sum(lens)
    q = torch.randn((t, hq, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    k = torch.randn((t, hkv, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    v = torch.randn((t, hkv, d), generator=g).to(dtype).to(DEV).requires_grad_(True)
    do = torch.randn((t, hq, d), generator=g).to(dtype).to(DEV)
    slopes = alibi_standard(hq).to(DEV).requires_grad_(True)   # (H,)
    cu = _cu(lens)
    o = flash_attention_varlen(q, k, v, cu, cu, max(lens), max(lens), causal=True, softcap=20.0, alibi_slopes=slopes)
    o.backward(do)
    assert slopes.grad is None
    ref = _varlen_reference(q.detach().cpu(), k.detach().cpu().repeat_interleave(hq // hkv, 1),
                            v.detach().cpu().repeat_interleave(hq // hkv, 1), do.cpu(), lens, lens, True, d ** -0.5, 20.0,
                            slopes.detach().cpu().repeat(len(lens), 1))
    tol = dtype_tolerances(dtype)
    torch.testing.assert_close(o.detach().cpu().double(), ref[0], **tol)
    torch.testing.assert_close(q.grad.cpu().double(), ref[2], **tol)
    torch.testing.assert_close(k.grad.cpu().double(), ref[3].reshape(t, hkv, hq // hkv, d).sum(2), **tol)
    torch.testing.assert_close(v.grad.cpu().double(), ref[4].reshape(t, hkv, hq // hkv, d).sum(2), **tol)
