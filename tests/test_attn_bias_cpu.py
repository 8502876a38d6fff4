"""An additive attention bias (fa_ex_forward_bias / fa_ex_backward_bias; ex_forward(attn_bias=); flash_attention_ex(attn_bias=)), the
part that needs no GPU: the entry points and their signatures, the C layer's argument rules (refused before any HIP call: the pointers
here are fake), the wrappers' rules on fake-CUDA tensors, and tests/bias_ref.py against itself and against its mutants."""
import inspect

import pytest
import torch

import flashattention_lab_cuda as ext
from common.attention_ex import flash_attention_ex
from tests import bias_ref as br
from tests import ex_full_ref as xr

INVALID_ARGUMENT, UNSUPPORTED = -1, -2
P = 0x10000      # a fake, 16-byte aligned pointer: every call below is refused before anything is read


# ---- 1. the three symbols

def test_symbols_and_signatures():
    for name in ("fa_ex_forward_bias", "fa_ex_backward_bias", "fa_ex_backward_workspace_bytes_bias"):
        assert name in ext.EXPORTED_C_SYMBOLS and name in ext._SIGNATURES and hasattr(ext._lib, name)
    fwd = [f for f, _t in ext._SIGNATURES["fa_ex_forward_bias"][1]]
    vd = [f for f, _t in ext._SIGNATURES["fa_ex_forward_vdim"][1]]
    group = ["bias", "bias_heads", "bias_batch_stride", "bias_head_stride", "bias_row_stride"]
    i = vd.index("d_v") + 1
    assert fwd == vd[:i] + group + vd[i:]
    bwd = [f for f, _t in ext._SIGNATURES["fa_ex_backward_bias"][1]]
    vdb = [f for f, _t in ext._SIGNATURES["fa_ex_backward_vdim"][1]]
    i = vdb.index("d_v") + 1
    assert bwd == vdb[:i] + group + ["dbias", "dbias_batch_stride", "dbias_head_stride", "dbias_row_stride"] + vdb[i:]
    # the workspace: the grouped one, plus BH * Nq * (Nk padded to 8) * 2 bytes of per-unit dS for a broadcast dbias
    base = ext._lib.fa_ex_backward_workspace_bytes_grouped(8, 2, 70, 300, 64, 2)
    assert ext._lib.fa_ex_backward_workspace_bytes_bias(8, 2, 70, 300, 64, 2, 0) == base
    assert ext._lib.fa_ex_backward_workspace_bytes_bias(8, 2, 70, 300, 64, 2, 1) == base + 8 * 70 * 304 * 2


# ---- 2. the C layer's rules

def _c_call(backward=False, **kw):
    a = dict(q=P, k=P, v=P, o=P, do_=P, lse=P, dq=P, dk=P, dv=P, bh=8, kv_group=1, nq=16, nk=24, d=64, dtype=2, causal=0, window_left=-1,
             window_right=-1, softmax_scale=0.125, softcap=0.0, alibi_slopes=0, alibi_heads=1, alibi_batch_stride=0, sinks=0, sink_heads=1,
             dsinks=0, dlse=0, d_v=0, bias=P, bias_heads=4, bias_batch_stride=4 * 16 * 24, bias_head_stride=16 * 24, bias_row_stride=24,
             dbias=0, dbias_batch_stride=0, dbias_head_stride=0, dbias_row_stride=0, mask=0, mask_bh_stride=0, block_mask=0, br=0, bc=0,
             dropout_p=0.0, dropout_seed=0, workspace=P, workspace_bytes=1 << 30, stream=0)
    a.update(kw)
    name = "fa_ex_backward_bias" if backward else "fa_ex_forward_bias"
    rc = getattr(ext._lib, name)(*[a[f] for f, _t in ext._SIGNATURES[name][1]])
    return rc, ext._lib.fa_last_error().decode()


@pytest.mark.parametrize("backward", [False, True])
def test_c_rules_in_their_order(backward):
    c = lambda **kw: _c_call(backward, **kw)   # noqa: E731
    rc, msg = c(bias=0)                                                    # (1) null bias with strides
    assert rc == INVALID_ARGUMENT and "bias is null" in msg
    rc, msg = c(bias=P + 8)                                                # (2) misaligned
    assert rc == UNSUPPORTED and "16-byte aligned" in msg
    rc, msg = c(bias_row_stride=20)                                        # (3) a stride that is no multiple of 8
    assert rc == UNSUPPORTED and "multiple of 8" in msg and "padded" in msg and "20" in msg
    rc, msg = c(bias_heads=3)                                              # (4) bias_heads not dividing bh
    assert rc == INVALID_ARGUMENT and "bias_heads=3 does not divide BH=8" in msg
    rc, msg = c(bias=P + 8, bias_row_stride=20, bias_heads=3, mask=P)      # the first broken rule is the one named
    assert rc == UNSUPPORTED and "16-byte aligned" in msg
    for kw, name in ((dict(mask=P), "mask"), (dict(block_mask=P, br=32, bc=32), "block_sparse_mask"), (dict(dropout_p=0.1), "dropout_p > 0"),
                     (dict(window_left=3), "window_size"), (dict(softcap=30.0), "softcap"), (dict(alibi_slopes=P), "alibi_slopes"),
                     (dict(sinks=P, dsinks=P), "sinks"), (dict(d_v=32), "d_v != d")):
        rc, msg = c(**kw)
        assert rc == UNSUPPORTED and f": {name} is not supported with a bias" in msg, (kw, msg)
    assert "fold it into the bias as -inf" in c(mask=P)[1]
    rc, msg = c(dtype=0)
    assert rc == UNSUPPORTED and "f16 or bf16" in msg and "no exact-f32 kernels with a bias" in msg
    for d in (136, 60):
        rc, msg = c(d=d)
        assert rc == UNSUPPORTED and "d <= 128" in msg and f"d={d}" in msg
    rc, msg = c(softmax_scale=0.0)
    assert rc == UNSUPPORTED and "softmax_scale > 0" in msg
    if backward:
        rc, msg = c(dbias=P, dbias_row_stride=24, bias_row_stride=0)        # (5) a gradient for a row-broadcast bias
        assert rc == UNSUPPORTED and "row-broadcast" in msg
        rc, msg = c(dbias=P + 4, dbias_row_stride=24)
        assert rc == UNSUPPORTED and "16-byte aligned" in msg
        rc, msg = c(dbias=P, dbias_row_stride=12)
        assert rc == UNSUPPORTED and "multiple of 8" in msg
        rc, msg = c(bias=0, bias_batch_stride=0, bias_head_stride=0, bias_row_stride=0, dbias=P)
        assert rc == INVALID_ARGUMENT and "bias is null" in msg


# ---- 3. the wrappers, on tensors that only claim to be on the GPU

class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def test_wrapper_refusals_and_layout_rules():
    q, k = _fake(8, 16, 64), _fake(8, 24, 64)
    lse = _fake(8, 16, dtype=torch.float32)
    bias = _fake(2, 4, 16, 24)
    calls = (lambda **kw: ext.ex_forward(q, k, k, False, 0.125, **kw),
             lambda **kw: ext.ex_backward(q, k, k, q, q, lse, False, 0.125, **kw))
    for call in calls:
        for kw, name in ((dict(mask=torch.ones(16, 24)), "mask"), (dict(block_mask=torch.ones(1, 1), br=32, bc=32), "block_sparse_mask"),
                         (dict(dropout_p=0.1), "dropout_p"), (dict(window=(3, -1)), "window_size"), (dict(softcap=30.0), "softcap"),
                         (dict(alibi_slopes=_fake(8, dtype=torch.float32)), "alibi_slopes"), (dict(sinks=_fake(4, dtype=torch.float32)), "sinks")):
            with pytest.raises(NotImplementedError, match=f"{name} is not supported with attn_bias"):
                call(attn_bias=bias, **kw)
        with pytest.raises(NotImplementedError, match="fold it into attn_bias as -inf"):
            call(attn_bias=bias, mask=torch.ones(16, 24))
        with pytest.raises(ValueError, match="padded to a multiple of 8"):          # contiguous, Nk = 20
            ext.ex_forward(q, _fake(8, 20, 64), _fake(8, 20, 64), False, 0.125, attn_bias=_fake(2, 4, 16, 20))
        with pytest.raises(ValueError, match="ends before Nk = 20 rounded up to 24"):  # every stride broadcast, the storage still too short
            ext.ex_forward(q, _fake(8, 20, 64), _fake(8, 20, 64), False, 0.125, attn_bias=_fake(1, 1, 1, 20))
        with pytest.raises(RuntimeError, match="must have q's dtype"):
            call(attn_bias=_fake(2, 4, 16, 24, dtype=torch.float16))
        with pytest.raises(RuntimeError, match=r"attn_bias must be .*got \(2, 4, 16, 23\)"):
            call(attn_bias=_fake(2, 4, 16, 23))
        with pytest.raises(RuntimeError, match=r"attn_bias must be .*got \(3, 16, 24\)"):
            call(attn_bias=_fake(3, 16, 24))
        with pytest.raises(RuntimeError, match="must be on q's device"):
            call(attn_bias=torch.zeros((2, 4, 16, 24), dtype=torch.bfloat16, device="meta"))
    with pytest.raises(NotImplementedError, match="d_v != d is not supported with attn_bias"):
        ext.ex_forward(q, k, _fake(8, 24, 32), False, 0.125, attn_bias=bias)
    q40 = _fake(8, 16, 132)
    with pytest.raises(NotImplementedError, match="d <= 128"):
        ext.ex_forward(q40, _fake(8, 24, 132), _fake(8, 24, 132), False, 0.1, attn_bias=bias)
    f32 = _fake(8, 16, 64, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="float16 or bfloat16"):
        ext.ex_forward(f32, _fake(8, 24, 64, dtype=torch.float32), _fake(8, 24, 64, dtype=torch.float32), False, 0.1,
                       attn_bias=_fake(2, 4, 16, 24, dtype=torch.float32))
    with pytest.raises(NotImplementedError, match="row-broadcast"):
        ext.ex_backward(q, k, k, q, q, lse, False, 0.125, attn_bias=_fake(2, 1, 1, 24), need_dbias=True)
    with pytest.raises(RuntimeError, match="need_dbias without attn_bias"):
        ext.ex_backward(q, k, k, q, q, lse, False, 0.125, need_dbias=True)
    # the public call: refusals by name before anything runs, the shapes of a 4-D and of a 3-D q
    q4, k4 = _fake(2, 4, 16, 64), _fake(2, 4, 24, 64)
    for kw, name in ((dict(mask=torch.ones(16, 24)), "mask"), (dict(dropout_p=0.2), "dropout_p"), (dict(window_size=(4, 0)), "window_size"),
                     (dict(softcap=20.0), "softcap"), (dict(alibi_slopes=_fake(4, dtype=torch.float32)), "alibi_slopes"),
                     (dict(sinks=_fake(4, dtype=torch.float32)), "sinks"), (dict(block_sparse_mask=torch.ones(1, 1)), "block_sparse_mask")):
        with pytest.raises(NotImplementedError, match=f"{name} is not supported with attn_bias"):
            flash_attention_ex(q4, k4, k4, attn_bias=bias, **kw)
    with pytest.raises(RuntimeError, match=r"attn_bias must be \(1 or 2, 1 or 4, 1 or 16, 24\), got \(2, 2, 16, 24\)"):
        flash_attention_ex(q4, k4, k4, attn_bias=_fake(2, 2, 16, 24))
    with pytest.raises(RuntimeError, match=r"attn_bias must be \(1 or 8, 1 or 16, 24\), got \(2, 4, 16, 24\)"):
        flash_attention_ex(q, k, k, attn_bias=bias)


def test_attn_bias_is_keyword_only_and_before_sinks():
    for fn in (ext.ex_forward, ext.ex_backward, flash_attention_ex):
        params = inspect.signature(fn).parameters
        assert params["attn_bias"].kind is inspect.Parameter.KEYWORD_ONLY and params["attn_bias"].default is None
        assert list(params)[-1] == "sinks" and list(params).index("attn_bias") < list(params).index("sinks")
    assert inspect.signature(ext.ex_backward).parameters["need_dbias"].default is False


# ---- 4. the reference against itself

def _maxdiff(a, b):
    out = 0.0
    for name in ("o", "lse", "dq", "dk", "dv", "dbias"):
        x, y = getattr(a, name), getattr(b, name)
        if x is None:
            continue
        fin = torch.isfinite(y.double())
        assert torch.equal(torch.isfinite(x.double()), fin)
        out = max(out, (x.double()[fin] - y.double()[fin]).abs().max().item())
    return out


@pytest.mark.parametrize("shape,causal,inf", [("full", False, 0.0), ((1, 0, 0), True, 0.0), ((0, 1, 0), False, 0.3), ((1, 1, 0), True, 0.2)])
def test_fp64_baseline_is_the_reference(shape, causal, inf):
    call = br.make_call(2, 4, 2, 37, 70, 16, torch.bfloat16, causal, shape, seed=3, with_dlse=True, inf_frac=inf, dead_rows=2 if inf else 0)
    ref = br.bias_reference(call)
    base = br.bias_baseline(call, compute=torch.float64, tensor_dtype=None)
    assert _maxdiff(base, ref) < 1e-10
    assert ref.dbias.shape == call["bias"].shape


def _sweep_call(call, **kw):
    bh, nq = call["q"].shape[:2]
    d = dict(layout="padded", q=call["q"], k=call["k"], v=call["v"], do=call["do"], dlse=call["dlse"], heads=call["heads"], causal=call["causal"],
             scale=call["scale"], dtype=call["dtype"], window=(-1, -1), mask=None, block_mask=None, br=0, bc=0, dropout_p=0.0, seed=0,
             softcap=0.0, alibi_slopes=None, sinks=None)
    d.update(kw)
    return d


def test_bias_reproduces_alibi_and_the_causal_flag():
    b, hq, nq, nk = 2, 4, 19, 45
    call = br.make_call(b, hq, 2, nq, nk, 16, torch.float16, False, seed=5, with_dlse=True)
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625]).repeat(b)
    dist = (torch.arange(nq).unsqueeze(1) + nk - nq - torch.arange(nk).unsqueeze(0)).abs().double()
    call["bias"] = -(slopes.double().reshape(b, hq, 1, 1) * dist)                       # exact in fp64: the reference widens to it
    ref = br.bias_reference(call)
    want = xr.full_reference(_sweep_call(call, alibi_slopes=slopes.float()))
    assert _maxdiff(br.BiasResult(want.o, want.lse, want.dq, want.dk, want.dv, None, *[None] * 6), ref) < 1e-12
    # -inf above the shifted diagonal is the causal flag, dead rows included (Nq > Nk: the first Nq - Nk rows see nothing)
    for nq, nk in ((19, 45), (45, 19)):
        call = br.make_call(b, hq, 4, nq, nk, 16, torch.bfloat16, False, seed=6, with_dlse=True)
        above = torch.arange(nk).unsqueeze(0) > torch.arange(nq).unsqueeze(1) + nk - nq
        call["bias"] = torch.zeros((1, 1, nq, nk), dtype=torch.float64).masked_fill(above, br.NEG_INF)
        ref = br.bias_reference(call)
        want = xr.full_reference(_sweep_call(call, causal=True))
        got = br.BiasResult(want.o, want.lse, want.dq, want.dk, want.dv, None, *[None] * 6)
        assert _maxdiff(got, ref) < 1e-12
        assert torch.equal(ref.dead_rows, want.dead_rows) and torch.equal(ref.dead_keys, want.dead_keys)
        assert not torch.isnan(ref.dq).any() and bool((ref.dbias[..., above] == 0).all())


# ---- 5. the mutants: each fails the sharp bar that the baseline passes, on inputs fixed here

MUTANT_CALLS = {
    "bias_times_scale": dict(hkv=4, nq=40, nk=72, causal=False, shape="full"),
    "head_is_u_div_hq": dict(hkv=4, nq=40, nk=72, causal=False, shape="full"),
    "bias_by_kv_head": dict(hkv=2, nq=40, nk=72, causal=False, shape="full"),
    "block_transposed": dict(hkv=4, nq=40, nk=72, causal=False, shape="full"),
    "dbias_under_causal": dict(hkv=4, nq=40, nk=72, causal=True, shape="full"),
    "dbias_from_batch0": dict(hkv=4, nq=40, nk=72, causal=False, shape=(1, 0, 0)),
    "padding_read_as_keys": dict(hkv=4, nq=40, nk=69, causal=False, shape="full"),
}


@pytest.mark.parametrize("mutant", br.BIAS_MUTANTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mutants_fail_the_sharp_bar(mutant, dtype):
    c = MUTANT_CALLS[mutant]
    call = br.make_call(2, 4, c["hkv"], c["nq"], c["nk"], 32, dtype, c["causal"], c["shape"], seed=11, with_dlse=True)
    ref = br.bias_reference(call)
    base = br.rounded(br.bias_baseline(call), dtype)
    bad, _ratio = br.sharp_bar(base, ref, base, dtype)
    assert not bad and not br.project_bar(base._replace(dead_rows=None), ref, dtype) and not br.dbias_zeros(base, call)
    wrong = br.rounded(br.bias_reference(call, mutant=mutant), dtype)
    bad, _ratio = br.sharp_bar(wrong, ref, base, dtype)
    assert bad, mutant
