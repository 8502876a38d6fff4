"""GPU: the FA3 fp8 path (fa3_cuda(..., fp8=True)) pinned to the reference's fixtures, and at the edges of its quantisation.

A. The reference's own fp8 cases (tests/test_correctness_fa3.py:12-34, 64-92) on its committed fixtures, at its per-element bar
   (rtol = atol = 1e-1) for o, dq, dk, dv.  lse cannot meet its 1e-3 once e4m3 really rounds (its fp8 mode rounds nothing,
   SURVEY D7): it is held to the oracle's e4m3 model at 2e-2 and to the stored exact value at 1e-1.
B. BH > 65535 (the quantisation kernels once put BH in gridDim.y).
C. d = 128: the backward differentiates attention of the V~ the forward used (power-of-two scales where the all-e4m3 kernel runs).
D. Edge values: Q = 0, all-zero and tiny blocks, large magnitudes, ragged N next to a much larger neighbouring unit.

Model tolerances are those of tests/test_parity_gpu.py for the same kernels: 3e-2 where P.V is 16-bit, 8e-2 where the all-e4m3
kernel rounds P (the model has its error statistics, not its bits)."""
import pytest
import torch

from oracle import attention_oracle as orc
from tests.helpers import dtype_tolerances, golden_tags, load_golden, make_qkv, max_abs

pytestmark = pytest.mark.gpu

FA3_TAGS = golden_tags("fa3_*")


def _fa3(q, k, v, causal, scale, do=None, fp8=True):
    from fa3.cuda.impl import fa3_cuda
    from fa3.spec import pick_fa3_spec

    if do is not None:
        q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o, lse = fa3_cuda(q, k, v, causal, scale, pick_fa3_spec(q.shape[-1]), fp8)
    if do is None:
        return o.detach(), lse.detach()
    (o * do).sum().backward()
    return o.detach(), lse.detach(), q.grad, k.grad, v.grad


def _e4m3_kernel(n, d):
    """does the all-e4m3 kernel (e4m3 P, power-of-two V scales) serve the call?  d = 128, N > 256, option fp8_pv at 0"""
    return d == 128 and n > 256


def _fp8_model(q, k, v, causal, scale):
    """(o, lse, tol) of the model of what fa3_forward(fp8) computes at the default options, row by row: under the causal mask
    the first 256 query rows take the 16-bit P.V even where the all-e4m3 kernel serves the rest, on the same V~"""
    n, d = q.shape[-2], q.shape[-1]
    e4 = _e4m3_kernel(n, d)
    mo, mlse = orc.fp8_attention(q, k, v, causal, scale, 64, 64, p_e4m3=e4)
    if e4 and causal:
        m16, _ = orc.fp8_attention(q, k, v, causal, scale, 64, 64, p_e4m3=False, v_pow2=True)
        mo = torch.cat([m16[:, :256], mo[:, 256:]], dim=1)
    return mo, mlse, (8e-2 if e4 else 3e-2)


def _per_element(a, b, what):
    """the reference's per-element fp8 bar, |a - b| <= 1e-1 + 1e-1 |b|; returns the worst share of it used"""
    a, b = a.detach().cpu().double(), b.double()
    ratio = (a - b).abs() / (1e-1 + 1e-1 * b.abs())
    worst = ratio.max().item()
    print(f"{what}: worst share of the per-element bar {worst:.3f}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements past the per-element 1e-1 bar, worst ratio {worst:.3f}"
    torch.testing.assert_close(a.float(), b.float(), rtol=1e-1, atol=1e-1)
    return worst


# ------------------------------------------------------------------------------------------------------------ A. fixtures


@pytest.mark.parametrize("tag", FA3_TAGS)
def test_fp8_matches_the_reference_fixture(tag, device):
    """fp8=True on the reference's fa3 fixtures.  fp16: real e4m3 (the output differs from fp8=False), o / dq / dk / dv at the
    reference's per-element 1e-1 against the stored exact values, lse against the model at 2e-2 and the stored value at 1e-1 —
    a departure from the reference's lse bar of 1e-3, which its fp8 mode meets only because it rounds nothing (the model, on the
    CPU, is 3.1e-2 - 5.7e-2 off the stored lse on these cases).  fp32: fp8 is ignored, bit for bit, at the fp32 bar."""
    meta, g = load_golden(tag)
    causal, scale = meta["causal"], meta["softmax_scale"]
    q, k, v = (g[x].to(device) for x in "qkv")
    do = g["do"].to(device) if "do" in g else None
    r8 = _fa3(q, k, v, causal, scale, do=do, fp8=True)
    r16 = _fa3(q, k, v, causal, scale, do=do, fp8=False)
    names = ("o", "lse", "dq", "dk", "dv")
    if g["q"].dtype == torch.float32:
        for name, a, b in zip(names, r8, r16):
            assert torch.equal(a, b), name
        tol = dtype_tolerances(torch.float32)
        torch.testing.assert_close(r8[0].cpu(), g["o"], **tol)
        torch.testing.assert_close(r8[1].cpu(), g["lse"], rtol=1e-3, atol=1e-3)
        for name, a in zip(names[2:], r8[2:]):
            torch.testing.assert_close(a.cpu(), g[name], **tol)
        return
    assert not torch.equal(r8[0], r16[0])   # e4m3 really ran
    o, lse = r8[0], r8[1]
    _per_element(o, g["o"], f"{tag} o")
    mo, mlse = orc.fp8_attention(g["q"], g["k"], g["v"], causal, scale, 64, 64)
    torch.testing.assert_close(o.cpu().float(), mo.float(), rtol=3e-2, atol=3e-2)
    assert max_abs(lse.cpu(), mlse) < 2e-2
    assert max_abs(lse.cpu(), g["lse"]) < 1e-1
    if do is not None:
        mg = orc.fp8_attention_backward(g["q"], g["k"], g["v"], g["do"], causal, scale, 64, 64)[:3]
        for name, a, m in zip(names[2:], r8[2:], mg):
            assert a.dtype == g[name].dtype
            _per_element(a, g[name], f"{tag} {name}")
            torch.testing.assert_close(a.cpu().float(), m.float(), rtol=3e-2, atol=3e-2)


# ------------------------------------------------------------------------------------------------------------ B. BH > 65535

BIG_BH = 65537
UNITS = [0, 65534, 65535, 65536]


def _big_inputs(n, d, dtype, seed, device, with_do):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return [torch.randn((BIG_BH, n, d), generator=g, device=device, dtype=torch.float32).to(dtype) for _ in range(4 if with_do else 3)]


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,d,causal,backward", [(100, 64, False, True), (100, 64, True, True), (64, 128, True, True),
                                                 (64, 128, False, True), (260, 128, False, False), (260, 128, True, False)])
def test_fp8_with_more_than_65535_units(n, d, causal, backward, device):
    """BH = 65537 with fp8: d = 64 (round trip ahead of the 16-bit kernels, ragged last block), d = 128 at N = 64 (e4m3 Q, K and the
    round-tripped V, forward and backward) and at N = 260 (the all-e4m3 kernel and its V quantisation, forward).  Units on both
    sides of 65535 and the last one against the model of that unit."""
    bf = torch.bfloat16
    scale = d ** -0.5
    ts = _big_inputs(n, d, bf, 4000 + n + d, device, backward)
    q, k, v = ts[:3]
    if backward:
        o, lse, dq, dk, dv = _fa3(q, k, v, causal, scale, do=ts[3])
    else:
        o, lse = _fa3(q, k, v, causal, scale)
    sel = torch.tensor(UNITS, device=device)
    cpu = [t.index_select(0, sel).cpu() for t in ts]
    out = [t.index_select(0, sel).cpu() for t in ((o, lse, dq, dk, dv) if backward else (o, lse))]
    del ts, q, k, v, o, lse
    if backward:
        del dq, dk, dv
    _free()
    mo, mlse, tol = _fp8_model(cpu[0], cpu[1], cpu[2], causal, scale)
    assert torch.isfinite(out[0].float()).all()
    torch.testing.assert_close(out[0].float(), mo.float(), rtol=tol, atol=tol)
    assert max_abs(out[1], mlse) < 2e-2
    if backward:
        mg = orc.fp8_attention_backward(cpu[0], cpu[1], cpu[2], cpu[3], causal, scale, 64, 64, v_pow2=_e4m3_kernel(n, d))[:3]
        for name, a, m in zip(("dq", "dk", "dv"), out[2:], mg):
            torch.testing.assert_close(a.float(), m.float(), rtol=3e-2, atol=3e-2, msg=lambda s: f"{name}: {s}")


def test_bf16_with_more_than_65535_units(device):
    """the 16-bit control at BH = 65537: forward and backward against the exact result at the reference's bf16 bar"""
    n, d = 100, 64
    scale = d ** -0.5
    ts = _big_inputs(n, d, torch.bfloat16, 4242, device, True)
    o, lse, dq, dk, dv = _fa3(ts[0], ts[1], ts[2], True, scale, do=ts[3], fp8=False)
    sel = torch.tensor(UNITS, device=device)
    cpu = [t.index_select(0, sel).cpu() for t in ts]
    out = [t.index_select(0, sel).cpu() for t in (o, lse, dq, dk, dv)]
    del ts, o, lse, dq, dk, dv
    _free()
    rq, rk, rv, ro, rlse = orc.exact_attention_backward(*cpu, True, scale, math_dtype=torch.float64)
    tol = dtype_tolerances(torch.bfloat16)
    torch.testing.assert_close(out[0], ro, **tol)
    torch.testing.assert_close(out[1], rlse, rtol=1e-3, atol=1e-3)
    for a, b in zip(out[2:], (rq, rk, rv)):
        torch.testing.assert_close(a, b, **tol)


# ------------------------------------------------------------------------------------------------------------ C. one V~


@pytest.mark.parametrize("pv", [0, 1], ids=["all-e4m3", "pv16"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("n", [333, 1000, 2100])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fp8_backward_differentiates_the_forwards_v(dtype, n, causal, pv, device):
    """d = 128: dQ and dK are the gradients of attention of the V~ the forward used — power-of-two block scales where the
    all-e4m3 kernel runs (option fp8_pv = 0, N > 256: every row, the causal first tile included), absmax / 448 ones otherwise.
    Every case is bounded against the matching model; where the two V~ give clearly different gradients (causal, N >= 1000,
    about 0.1 apart on the CPU) the error against the matching model must also be at most 1/3 of that against the other."""
    import flashattention_lab_cuda as ext

    d = 128
    q, k, v, do = make_qkv(2, n, d, dtype, seed=900 + n)
    scale = d ** -0.5
    ext.set_option("fp8_pv", pv)
    try:
        o, lse, dq, dk, dv = _fa3(q.to(device), k.to(device), v.to(device), causal, scale, do=do.to(device))
    finally:
        ext.set_option("fp8_pv", 0)
    pow2 = pv == 0 and n > 256
    match = orc.fp8_attention_backward(q, k, v, do, causal, scale, 64, 64, v_pow2=pow2)
    other = orc.fp8_attention_backward(q, k, v, do, causal, scale, 64, 64, v_pow2=not pow2)
    tol = 8e-2 if pow2 else 3e-2
    for name, a, m, x in (("dq", dq, match[0], other[0]), ("dk", dk, match[1], other[1])):
        a = a.cpu()
        assert torch.isfinite(a.float()).all()
        torch.testing.assert_close(a.float(), m.float(), rtol=tol, atol=tol, msg=lambda s: f"{name}: {s}")
        if causal and n >= 1000:
            e_match, e_other = max_abs(a, m), max_abs(a, x)
            assert e_match <= e_other / 3, f"{name}: error against the forward's V~ {e_match:.4f}, against the other V~ {e_other:.4f}"
    torch.testing.assert_close(dv.cpu().float(), match[2].float(), rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------------------ D. edge values

EDGE_D = [32, 40, 64, 128, 256]
EDGE_N = 300     # d = 128: the all-e4m3 kernel, and under the mask its first tile on the 16-bit P.V; five 64-row blocks, the last partial


def _visible_vmax(v, causal):
    """per (unit, query row): the largest |v| of the keys the row sees"""
    m = v.float().abs().amax(dim=-1)
    m = torch.cummax(m, dim=-1).values if causal else m.amax(dim=-1, keepdim=True).expand_as(m)
    return m[..., None]


def _check_fwd(o, lse, q, k, v, causal, scale, what, scaled=False):
    """o and lse against the model; scaled=True: the bar on o is relative to the magnitude of the V the row sees
    (values near 6e4 carry 16-bit rounding far above an absolute 3e-2)"""
    o, lse = o.cpu(), lse.cpu()
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), what
    mo, mlse, tol = _fp8_model(q, k, v, causal, scale)
    if scaled:
        err = (o.double() - mo.double()).abs()
        bar = tol * _visible_vmax(v, causal).double()
        assert (err <= bar).all(), f"{what}: {int((err > bar).sum())} elements past {tol} x the visible |v|"
    else:
        torch.testing.assert_close(o.float(), mo.float(), rtol=tol, atol=tol, msg=lambda s: f"{what}: {s}")
    assert max_abs(lse, mlse) < 2e-2, what


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", EDGE_D)
def test_fp8_zero_q(d, dtype, causal, device):
    """Q = 0: S = 0, P uniform, o = the mean of V~ over the visible keys (prefix means under the mask); the V quantisation in
    isolation, every block's absmax element included (it must come back as +-448 x scale, not as NaN)."""
    q, k, v = make_qkv(2, EDGE_N, d, dtype, seed=70 + d, with_do=False)
    q = torch.zeros_like(q)
    o, lse = _fa3(q.to(device), k.to(device), v.to(device), causal, d ** -0.5)
    _check_fwd(o, lse, q, k, v, causal, d ** -0.5, "q = 0")
    # and the model is what the docstring says: prefix means of V~
    vt = orc.fp8_roundtrip(q, k, v, 64, 64, v_pow2=_e4m3_kernel(EDGE_N, d))[2].double()
    cnt = torch.arange(1, EDGE_N + 1, dtype=torch.float64)[:, None]
    mean = vt.cumsum(dim=1) / cnt if causal else vt.mean(dim=1, keepdim=True).expand_as(vt)
    torch.testing.assert_close(o.cpu().float(), mean.float(), rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", EDGE_D)
def test_fp8_zero_and_tiny_blocks(d, dtype, causal, device):
    """a 64-row block of V and one of K all zero, and one of each with absmax below the 1e-6 eps of the scale"""
    q, k, v = make_qkv(2, EDGE_N, d, dtype, seed=80 + d, with_do=False)
    v[:, 64:128] = 0
    k[:, 128:192] = 0
    v[:, 192:256] = (v[:, 192:256].float() * 1e-7).to(dtype)
    k[:, 0:64] = (k[:, 0:64].float() * 1e-7).to(dtype)
    o, lse = _fa3(q.to(device), k.to(device), v.to(device), causal, d ** -0.5)
    _check_fwd(o, lse, q, k, v, causal, d ** -0.5, "zero / tiny blocks")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", EDGE_D)
def test_fp8_large_magnitudes(d, dtype, causal, device):
    """fp16: V with values up to 6e4 (near the format's 65504).  bf16: V blocks around 1e-3 next to blocks around 1e4 (the first
    block small, so that under the mask the first rows see only small values)."""
    q, k, v = make_qkv(2, EDGE_N, d, dtype, seed=90 + d, with_do=False)
    vf = v.float()
    if dtype == torch.float16:
        vf = vf.clamp(-3, 3) * 2e4
        vf[:, 5, 0] = 6e4
    else:
        blk = torch.arange(EDGE_N) // 64
        vf = vf * torch.where(blk % 2 == 0, 1e-3, 1e4)[None, :, None]
    v = vf.to(dtype)
    o, lse = _fa3(q.to(device), k.to(device), v.to(device), causal, d ** -0.5)
    _check_fwd(o, lse, q, k, v, causal, d ** -0.5, "large magnitudes", scaled=True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [65, 100, 130])
@pytest.mark.parametrize("d", EDGE_D)
def test_fp8_ragged_n_keeps_units_apart(d, n, dtype, device):
    """BH = 3, ragged N: a partial last block that read past N would take the next unit's first rows into its absmax.  The first
    16 rows of V in units 1 and 2 are 1e4 x larger than the rest (a float format rounds a block 100x larger almost as it
    rounds this one: only a ratio this large pushes unit 0's last block into e4m3's subnormals under a borrowed scale), and
    unit 0's queries attend mostly to its own last block.  Each unit must match the model computed on that unit alone.  (With the
    attention on a few keys, one V element rounded to the neighbouring e4m3 value shows: these cases caught the quantisers
    computing x * (448 / absmax), whose last-bit error flips bf16 inputs that lie exactly halfway between two e4m3 values.)"""
    q, k, v = make_qkv(3, n, d, dtype, seed=60 + n + d, with_do=False)
    last = (n - 1) // 64 * 64
    q[0] = (q[0].float() + 1.0).to(dtype)                    # S gains sqrt(d) on unit 0's last-block keys
    k[0, last:] = (k[0, last:].float() + 1.0).to(dtype)
    vf = v.float()
    vf[1:, :16] *= 1e4
    v = vf.to(dtype)
    for causal in (False, True):
        o, lse = _fa3(q.to(device), k.to(device), v.to(device), causal, d ** -0.5)
        for b in range(3):
            _check_fwd(o[b:b + 1], lse[b:b + 1], q[b:b + 1], k[b:b + 1], v[b:b + 1], causal, d ** -0.5, f"unit {b} causal={causal}",
                       scaled=b > 0)
