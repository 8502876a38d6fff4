"""The oracle's e4m3 model (oracle.fp8_attention*) against the reference's own fp8 fixtures, on the CPU.

The GPU tests in tests/test_fp8_gpu.py hold the HIP fp8 path to the reference's fixtures and to this model; this file makes sure
a change to the model that would break that pin fails without a GPU.  The bars are the reference's (tests/test_correctness_fa3.py:
31-32, 89: rtol = atol = 1e-1 per element) for o, dq, dk, dv.  lse is held to 1e-1 against the stored exact value, not to the
reference's 1e-3: the reference's fp8 mode rounds nothing, real e4m3 moves lse by 3e-2 - 6e-2 on these cases."""
import pytest
import torch

from oracle import attention_oracle as orc
from tests.helpers import golden_tags, load_golden, make_qkv, max_abs

FP8_TAGS = [t for t in golden_tags("fa3_*") if load_golden(t)[0]["dtype"] != "fp32"]


def per_element_ratio(a, b):
    """largest |a - b| / (1e-1 + 1e-1 |b|): <= 1 is the reference's per-element fp8 bar"""
    a, b = a.double(), b.double()
    return ((a - b).abs() / (1e-1 + 1e-1 * b.abs())).max().item()


def test_the_five_fp16_fixtures_are_there():
    assert len(FP8_TAGS) == 5, FP8_TAGS


@pytest.mark.parametrize("tag", FP8_TAGS)
def test_fp8_model_meets_the_reference_bar_on_its_fixtures(tag):
    meta, g = load_golden(tag)
    causal, scale = meta["causal"], meta["softmax_scale"]
    mo, mlse = orc.fp8_attention(g["q"], g["k"], g["v"], causal, scale, 64, 64)
    torch.testing.assert_close(mo.float(), g["o"].float(), rtol=1e-1, atol=1e-1)
    assert per_element_ratio(mo, g["o"]) < 0.97
    err_lse = max_abs(mlse, g["lse"])
    # real rounding: lse moves by far more than the reference's 1e-3, and stays well inside 1e-1
    assert 1e-2 < err_lse < 1e-1, err_lse
    ro, rlse = orc.exact_attention(g["q"].double(), g["k"].double(), g["v"].double(), causal, scale)
    assert not torch.equal(mo.double(), ro.to(mo.dtype).double())   # the model really rounds
    if "do" in g:
        grads = orc.fp8_attention_backward(g["q"], g["k"], g["v"], g["do"], causal, scale, 64, 64)[:3]
        for name, a in zip(("dq", "dk", "dv"), grads):
            torch.testing.assert_close(a.float(), g[name].float(), rtol=1e-1, atol=1e-1, msg=lambda m: f"{name}: {m}")
            assert per_element_ratio(a, g[name]) < 0.7, name


def test_pow2_v_scales_are_powers_of_two_that_fit_e4m3():
    x = make_qkv(3, 200, 64, torch.float32, seed=3, with_do=False)[0] * torch.tensor([1e-8, 1.0, 3e4])[:, None, None]
    xq, sc = orc.quantize_e4m3_blockwise_pow2(x, 64)
    amax = orc.block_absmax_scale(x, 64)
    assert torch.equal(torch.exp2(torch.log2(sc.double()).round()), sc.double())
    assert (amax / sc <= orc.E4M3_MAX).all() and (amax / sc > orc.E4M3_MAX / 2).all()
    assert torch.isfinite(xq).all()


@pytest.mark.parametrize("causal", [False, True])
def test_fp8_model_v_pow2_flag(causal):
    """v_pow2 picks V's scales independently of p_e4m3, forward and backward; dV does not depend on V~, dQ and dK do."""
    q, k, v, do = make_qkv(2, 150, 128, torch.bfloat16, seed=5)
    s = 128 ** -0.5
    qd, kd, vp = orc.fp8_roundtrip(q, k, v, 64, 64, v_pow2=True)
    va = orc.fp8_roundtrip(q, k, v, 64, 64, v_pow2=False)[2]
    assert not torch.equal(vp, va)
    o, lse = orc.fp8_attention(q, k, v, causal, s, 64, 64, p_e4m3=False, v_pow2=True)
    ro, rlse = orc.exact_attention(qd, kd, vp, causal, s)
    torch.testing.assert_close(o, ro.to(o.dtype), rtol=0, atol=0)
    # the defaults are unchanged: v_pow2 follows p_e4m3
    for p8 in (False, True):
        a = orc.fp8_attention(q, k, v, causal, s, 64, 64, p_e4m3=p8)[0]
        b = orc.fp8_attention(q, k, v, causal, s, 64, 64, p_e4m3=p8, v_pow2=p8)[0]
        assert torch.equal(a, b)
    gp = orc.fp8_attention_backward(q, k, v, do, causal, s, 64, 64, v_pow2=True)
    ga = orc.fp8_attention_backward(q, k, v, do, causal, s, 64, 64)
    assert torch.equal(gp[2], ga[2])
    assert max_abs(gp[0], ga[0]) > 0 and max_abs(gp[1], ga[1]) > 0
    ex = orc.exact_attention_backward(qd, kd, vp, do, causal, s, math_dtype=torch.float64)
    for a, b in zip(gp, ex):
        assert torch.equal(a, b)
