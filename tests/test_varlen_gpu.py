"""GPU: variable-length (packed) sequences (fa_ex_forward_varlen / fa_ex_backward_varlen through ex_varlen_forward /
ex_varlen_backward and flash_attention_varlen).  The reference is the fp64 oracle (orc.extended_attention) run sequence by sequence
on the (H, len, d) slices, with the causal flag and the window as a dense mask and, for GQA, K/V repeated over each group and dK / dV
summed over it; on the extended MFMA kernels (ex_path 3), the exact-f32 kernels (ex_path 1) and the default routing (ex_path 0)."""
import ctypes

import pytest
import torch

from oracle import attention_oracle as orc
from tests.helpers import dtype_tolerances

pytestmark = pytest.mark.gpu

PATHS = {"auto": 0, "exact": 1, "mfma_only": 3}
DEV = "cuda"


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def window_mask(nq, nk, causal, window):
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


def make_case(lens_q, lens_k, hq, hkv, d, dtype, seed, packed=False):
    """q (total_q, hq, d), k, v (total_k, hkv, d) and do; packed=True: q, k, v are unbind(1) views of one (total, 3, H, d)
    projection (needs hq == hkv and equal lengths) — token stride 3 H d."""
    g = torch.Generator().manual_seed(seed)
    tq, tk = sum(lens_q), sum(lens_k)
    if packed:
        assert hq == hkv and tq == tk
        qkv = torch.randn((tq, 3, hq, d), generator=g).to(dtype).to(DEV)
        q, k, v = qkv.unbind(1)
    else:
        q = torch.randn((tq, hq, d), generator=g).to(dtype).to(DEV)
        k = torch.randn((tk, hkv, d), generator=g).to(dtype).to(DEV)
        v = torch.randn((tk, hkv, d), generator=g).to(dtype).to(DEV)
    do = torch.randn((tq, hq, d), generator=g).to(dtype).to(DEV)
    return q, k, v, do


def oracle_varlen(q, k, v, do, lens_q, lens_k, causal, window, scale, dropout_p=0.0, seed=0, max_q=None, max_k=None):
    """(o, lse, dq, dk, dv) in the packed layouts (lse (H_q, total_q)), sequence by sequence in fp64."""
    hq, hkv = q.shape[1], k.shape[1]
    g = hq // hkv
    q, k, v, do = (t.detach().cpu() for t in (q, k, v, do))
    o = torch.zeros(q.shape, dtype=torch.float64)
    dq = torch.zeros(q.shape, dtype=torch.float64)
    dk = torch.zeros(k.shape, dtype=torch.float64)
    dv = torch.zeros(v.shape, dtype=torch.float64)
    lse = torch.full((hq, q.shape[0]), float("-inf"), dtype=torch.float64)
    keep_all = None
    if dropout_p > 0.0:
        keep_all = orc.dropout_keep(len(lens_q) * hq, max_q, max_k, dropout_p, seed)
    sq = sk = 0
    for b, (lq, lk) in enumerate(zip(lens_q, lens_k)):
        if lq > 0 and lk > 0:
            qb = q[sq:sq + lq].transpose(0, 1).double().requires_grad_(True)
            kb = k[sk:sk + lk].transpose(0, 1).double().requires_grad_(True)
            vb = v[sk:sk + lk].transpose(0, 1).double().requires_grad_(True)
            m = window_mask(lq, lk, causal, window).to(torch.uint8)
            kw = {}
            saved = orc.dropout_keep
            if keep_all is not None:
                kw = dict(dropout_p=dropout_p, seed=seed)
                sl = keep_all[b * hq:(b + 1) * hq, :lq, :lk]
                orc.dropout_keep = lambda *_a, **_k: sl
            try:
                ob, lb = orc.extended_attention(qb, kb.repeat_interleave(g, 0), vb.repeat_interleave(g, 0), causal=False,
                                                softmax_scale=scale, mask=m, **kw)
            finally:
                orc.dropout_keep = saved
            (ob * do[sq:sq + lq].transpose(0, 1).double()).sum().backward()
            o[sq:sq + lq] = ob.detach().transpose(0, 1)
            lse[:, sq:sq + lq] = lb.detach()
            dq[sq:sq + lq] = qb.grad.transpose(0, 1)
            dk[sk:sk + lk] = kb.grad.transpose(0, 1)
            dv[sk:sk + lk] = vb.grad.transpose(0, 1)
        sq += lq
        sk += lk
    return o, lse.float(), dq, dk, dv


def run_varlen(ext, q, k, v, do, cu_q, cu_k, max_q, max_k, causal, scale, window, path=0, dropout_p=0.0, seed=0):
    ext.set_option("ex_path", path)
    try:
        o, lse = ext.ex_varlen_forward(q, k, v, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed, window=window)
        dq, dk, dv = ext.ex_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed,
                                            window=window)
    finally:
        ext.set_option("ex_path", 0)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def check_against_oracle(got, ref, lens_q, lens_k, dtype, what=""):
    tol = dtype_tolerances(dtype)
    o, lse, dq, dk, dv = (t.cpu() for t in got)
    ro, rlse, rdq, rdk, rdv = ref
    # only tokens covered by a sequence are specified (here: all of them)
    torch.testing.assert_close(o.double(), ro, **tol, msg=lambda m: f"o {what}: {m}")
    fin = torch.isfinite(rlse)
    assert torch.equal(torch.isfinite(lse), fin), f"lse -inf pattern {what}"
    torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-3, atol=1e-3, msg=lambda m: f"lse {what}: {m}")
    for name, a, b in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        torch.testing.assert_close(a.double(), b, **tol, msg=lambda m, n=name: f"{n} {what}: {m}")


ORACLE_CASES = [
    # lens_q, lens_k, hq, hkv, d, dtype, causal, window, packed, max_extra, path
    ([255, 0, 1, 257, 256], None, 4, 4, 128, torch.bfloat16, True, (-1, -1), False, 0, "mfma_only"),
    ([300, 17, 513], [200, 40, 513], 4, 1, 64, torch.float16, True, (-1, -1), False, 0, "auto"),       # len_q > len_k, MQA
    ([100, 256, 3], [400, 257, 90], 8, 2, 128, torch.bfloat16, False, (-1, -1), False, 5, "auto"),    # len_q < len_k, GQA 4
    ([257, 600, 1], None, 4, 4, 128, torch.bfloat16, False, (100, 0), False, 0, "mfma_only"),          # (L, 0) = causal window
    ([300, 520, 64], [333, 500, 64], 4, 4, 64, torch.float16, False, (70, 40), False, 0, "mfma_only"),  # (L, R)
    ([256, 300, 0, 41], None, 2, 2, 128, torch.bfloat16, True, (-1, -1), True, 100, "mfma_only"),     # unbind views, max > max
    ([300, 17, 513], [200, 40, 513], 4, 1, 40, torch.float16, True, (-1, -1), False, 0, "auto"),      # d = 40: exact kernels
    ([130, 77, 256], [90, 300, 256], 4, 2, 64, torch.float32, True, (50, -1), False, 0, "auto"),       # f32
    ([255, 1, 257], [300, 2, 100], 4, 2, 128, torch.bfloat16, True, (64, -1), False, 0, "exact"),
    ([200, 0, 129], [0, 50, 129], 2, 2, 64, torch.float16, False, (-1, -1), False, 0, "exact"),         # empty sides
    ([256, 300, 0, 41], None, 2, 2, 40, torch.float32, False, (-1, -1), True, 3, "exact"),            # f32 views, d = 40
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: f"{c[5]}-d{c[4]}-g{c[2] // c[3]}-{c[10]}".replace("torch.", ""))
def test_varlen_matches_the_oracle(case):
    import flashattention_lab_cuda as ext

    lens_q, lens_k, hq, hkv, d, dtype, causal, window, packed, extra, path = case
    lens_k = lens_q if lens_k is None else lens_k
    q, k, v, do = make_case(lens_q, lens_k, hq, hkv, d, dtype, seed=len(lens_q) * 7 + d, packed=packed)
    if packed:
        assert q.stride(0) == 3 * hq * d and not q.is_contiguous()
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    mq, mk = max(lens_q) + extra, max(lens_k) + extra
    scale = d ** -0.5
    got = run_varlen(ext, q, k, v, do, cu_q, cu_k, mq, mk, causal, scale, window, PATHS[path])
    ref = oracle_varlen(q, k, v, do, lens_q, lens_k, causal, window, scale)
    check_against_oracle(got, ref, lens_q, lens_k, dtype, str(case))


BIT_CASES = [
    # lens_q, lens_k, hq, hkv, d, dtype, causal, window
    ([255, 1, 257, 640], None, 4, 4, 128, torch.bfloat16, True, (-1, -1)),
    ([300, 64, 700], [200, 90, 513], 4, 1, 64, torch.float16, False, (-1, -1)),
    ([300, 600], [350, 600], 8, 2, 128, torch.bfloat16, True, (100, -1)),
]


@pytest.mark.parametrize("case", BIT_CASES)
def test_varlen_is_bit_identical_to_each_sequence_alone(case):
    """ex_path 3, no dropout: every sequence of a varlen call equals fa_ex_*_window on that sequence alone in (H, n, d) layout."""
    import flashattention_lab_cuda as ext

    lens_q, lens_k, hq, hkv, d, dtype, causal, window = case
    lens_k = lens_q if lens_k is None else lens_k
    q, k, v, do = make_case(lens_q, lens_k, hq, hkv, d, dtype, seed=11)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    scale = d ** -0.5
    o, lse, dq, dk, dv = run_varlen(ext, q, k, v, do, cu_q, cu_k, max(lens_q), max(lens_k), causal, scale, window, 3)
    sq = sk = 0
    for lq, lk in zip(lens_q, lens_k):
        qb, kb, vb, dob = (t.transpose(0, 1).contiguous() for t in (q[sq:sq + lq], k[sk:sk + lk], v[sk:sk + lk], do[sq:sq + lq]))
        ext.set_option("ex_path", 3)
        try:
            ob, lb = ext.ex_forward(qb, kb, vb, causal, scale, window=window)
            dqb, dkb, dvb = ext.ex_backward(qb, kb, vb, ob, dob, lb, causal, scale, window=window)
        finally:
            ext.set_option("ex_path", 0)
        assert torch.equal(o[sq:sq + lq], ob.transpose(0, 1)), (lq, lk, "o")
        assert torch.equal(lse[:, sq:sq + lq], lb), (lq, lk, "lse")
        assert torch.equal(dq[sq:sq + lq], dqb.transpose(0, 1)), (lq, lk, "dq")
        assert torch.equal(dk[sk:sk + lk], dkb.transpose(0, 1)), (lq, lk, "dk")
        assert torch.equal(dv[sk:sk + lk], dvb.transpose(0, 1)), (lq, lk, "dv")
        sq += lq
        sk += lk


@pytest.mark.parametrize("path", ["mfma_only", "exact"])
@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_varlen_dropout_uses_the_padded_calls_keep_mask(path, dtype, d):
    import flashattention_lab_cuda as ext

    lens_q, lens_k, hq, hkv = [257, 40, 300], [300, 40, 129], 4, 2
    q, k, v, do = make_case(lens_q, lens_k, hq, hkv, d, dtype, seed=5)
    cu_q, cu_k = _cu(lens_q).to(DEV), _cu(lens_k).to(DEV)
    mq, mk, p, seed, scale = 320, 310, 0.15, 1234, d ** -0.5
    for causal, window in ((True, (-1, -1)), (False, (80, 20))):
        got = run_varlen(ext, q, k, v, do, cu_q, cu_k, mq, mk, causal, scale, window, PATHS[path], dropout_p=p, seed=seed)
        ref = oracle_varlen(q, k, v, do, lens_q, lens_k, causal, window, scale, dropout_p=p, seed=seed, max_q=mq, max_k=mk)
        check_against_oracle(got, ref, lens_q, lens_k, dtype, f"dropout {causal} {window}")


def test_flash_attention_varlen_autograd():
    from common.attention_ex import flash_attention_varlen

    lens, hq, hkv, d, dtype = [300, 1, 200, 256], 8, 2, 128, torch.bfloat16
    q, k, v, do = make_case(lens, lens, hq, hkv, d, dtype, seed=3)
    cu = _cu(lens).to(DEV)
    qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention_varlen(qg, kg, vg, cu, cu, max(lens), max(lens), causal=True, window_size=(128, -1))
    o.backward(do)
    assert kg.grad.shape == k.shape and vg.grad.shape == v.shape and qg.grad.shape == q.shape
    ro, _rl, rdq, rdk, rdv = oracle_varlen(q, k, v, do, lens, lens, True, (128, -1), d ** -0.5)
    tol = dtype_tolerances(dtype)
    torch.testing.assert_close(o.detach().cpu().double(), ro, **tol)
    for a, b in ((qg.grad, rdq), (kg.grad, rdk), (vg.grad, rdv)):
        torch.testing.assert_close(a.cpu().double(), b, **tol)


SENT = 7.0


@pytest.mark.parametrize("path", ["mfma_only", "exact"])
def test_malformed_cu_seqlens_stay_inside_the_packed_tensors(path):
    """Offsets that decrease, run past total or exceed max_seqlen.  Every tensor is a view into the middle of a sentinel-filled
    allocation with PAD tokens of slack on each side, more than any unclamped offset here could reach, so the check is that the
    clamps hold (the slack keeps its sentinels), not a fault."""
    import flashattention_lab_cuda as ext

    hq, hkv, d, dtype, total, mx, PAD = 4, 2, 128, torch.bfloat16, 300, 128, 1024
    cu = torch.tensor([-40, 100, 60, 290, 420, 600], dtype=torch.int32, device=DEV)
    batch = cu.shape[0] - 1
    lib = ext._lib

    def slab(h):
        big = torch.full((total + 2 * PAD, h, d), SENT, dtype=dtype, device=DEV)
        return big, big[PAD:PAD + total]

    g = torch.Generator().manual_seed(9)
    (qb, q), (kb, k), (vb, v), (ob, o), (dob, do), (dqb, dq), (dkb, dk), (dvb, dv) = (
        slab(h) for h in (hq, hkv, hkv, hq, hq, hq, hkv, hkv))
    for t in (q, k, v, do):
        t.copy_(torch.randn(t.shape, generator=g).to(dtype).to(DEV))
    lseb = torch.full((hq * total + 2 * PAD * hq,), SENT, dtype=torch.float32, device=DEV)
    lse = lseb[PAD * hq:PAD * hq + hq * total]
    wsn = int(lib.fa_ex_backward_workspace_bytes_varlen(hq, hkv, total, total, d, 2))
    ws = torch.empty((wsn,), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    before = {n: t.clone() for n, t in (("q", qb), ("k", kb), ("v", vb), ("do", dob))}
    ext.set_option("ex_path", PATHS[path])
    try:
        for causal in (0, 1):
            rc = lib.fa_ex_forward_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(),
                                          batch, hq, hkv, total, total, mx, mx, d, 2, hq * d, hkv * d, hkv * d, causal, -1, -1,
                                          d ** -0.5, 0.1, 5, ctypes.c_void_p(st))
            assert rc == 0, lib.fa_last_error()
            rc = lib.fa_ex_backward_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),
                                           dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), cu.data_ptr(), cu.data_ptr(), batch, hq, hkv,
                                           total, total, mx, mx, d, 2, hq * d, hkv * d, hkv * d, causal, -1, -1, d ** -0.5, 0.1, 5,
                                           ws.data_ptr(), wsn, ctypes.c_void_p(st))
            assert rc == 0, lib.fa_last_error()
            torch.cuda.synchronize()
    finally:
        ext.set_option("ex_path", 0)
    for name, big in (("o", ob), ("dq", dqb), ("dk", dkb), ("dv", dvb)):
        for part in (big[:PAD], big[PAD + total:]):
            assert bool((part == SENT).all()), f"{name}: a write left the packed tensor"
    for part in (lseb[:PAD * hq], lseb[PAD * hq + hq * total:]):
        assert bool((part == SENT).all()), "lse: a write left the packed tensor"
    for name, big in (("q", qb), ("k", kb), ("v", vb), ("do", dob)):
        assert torch.equal(big, before[name]), f"{name} was written"
    # the in-range part of the first (clamped) sequence is well defined: tokens [0, 100) -> its first 100 rows only
    assert bool(torch.isfinite(o[:100].float()).all())
