"""An additive attention bias and its gradient on the GPU (fa_ex_forward_bias / fa_ex_backward_bias), against tests/bias_ref.py at the
project's bar and at the sharp bar.  The tile edges of the kernels are 32 (block), 64 (forward key step, dK/dV query tile) and 256 (rows
per forward / dQ workgroup, keys per dK/dV workgroup); the shapes are the smallest that cross them.  B = 2, H_q = 4, the bias randn * 2
in the tensor dtype, every bias row padded to 8 with NaN, every dbias read back from the call's own buffer."""
import pytest
import torch

import flashattention_lab_cuda as ext
from common.attention_ex import flash_attention_ex
from common.merge_states import merge_attention_states
from tests import bias_ref as br

pytestmark = pytest.mark.gpu
B, HQ = 2, 4
BF, F16 = torch.bfloat16, torch.float16


def _padded(t, device, fill=float("nan")):
    """t (.., Nk) on the device as a slice of a buffer whose last dim is padded to 8 and filled with `fill`"""
    nk = t.shape[-1]
    buf = torch.full(tuple(t.shape[:-1]) + ((nk + 7) // 8 * 8,), fill, dtype=t.dtype, device=device)
    buf[..., :nk] = t.to(device)
    return buf[..., :nk]


def _run(call, device, need_dbias=True, bias_d=None):
    q, k, v, do = (call[n].to(device) for n in ("q", "k", "v", "do"))
    bias_d = _padded(call["bias"], device) if bias_d is None else bias_d
    dlse = None if call["dlse"] is None else call["dlse"].to(device)
    o, lse = ext.ex_forward(q, k, v, call["causal"], call["scale"], attn_bias=bias_d)
    grads = ext.ex_backward(q, k, v, o, do, lse, call["causal"], call["scale"], dlse=dlse, attn_bias=bias_d, need_dbias=need_dbias)
    torch.cuda.synchronize()
    dbias = grads[3].cpu() if need_dbias else None
    return br.BiasResult(o.cpu(), lse.cpu(), grads[0].cpu(), grads[1].cpu(), grads[2].cpu(), dbias, None, None, None, None, None, None)


def _check(got, call, zeros=True):
    ref = br.bias_reference(call)
    if got.dbias is None:
        ref = ref._replace(dbias=None)
    base = br.rounded(br.bias_baseline(call), call["dtype"])
    for t in (got.o, got.lse, got.dq, got.dk, got.dv) + (() if got.dbias is None else (got.dbias,)):
        assert not torch.isnan(t).any()
    assert not br.project_bar(got, ref, call["dtype"])
    bad, ratio = br.sharp_bar(got, ref, base, call["dtype"])
    assert not bad, (bad, ratio)
    if zeros and got.dbias is not None:
        assert not br.dbias_zeros(got, call)
    return ref


SHAPES = [(3, 5, False), (40, 72, False), (70, 300, False), (260, 100, False), (257, 264, False), (100, 260, True), (260, 100, True)]


@pytest.mark.parametrize("dtype,d,hkv", [(BF, 64, 4), (F16, 128, 2), (BF, 128, 2), (F16, 64, 4)])
@pytest.mark.parametrize("nq,nk,causal", SHAPES)
def test_forward_backward_dbias(device, nq, nk, causal, dtype, d, hkv):
    call = br.make_call(B, HQ, hkv, nq, nk, d, dtype, causal, seed=nq + nk, with_dlse=True)
    got = _run(call, device)
    ref = _check(got, call)
    if causal and nq > nk:      # the first Nq - Nk rows see no key
        dead = nq - nk
        assert bool(ref.dead_rows[:, :dead].all()) and bool((got.lse[:, :dead] == br.NEG_INF).all())
        assert bool((got.o[:, :dead] == 0).all()) and bool((got.dq[:, :dead] == 0).all()) and bool((got.dbias[:, :, :dead] == 0).all())


def test_head_dim_40(device):
    call = br.make_call(B, HQ, 2, 70, 300, 40, BF, True, seed=40, with_dlse=True)
    _check(_run(call, device), call)


@pytest.mark.parametrize("flags", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)])
@pytest.mark.parametrize("dtype", [BF, F16])
def test_broadcast_dbias_in_the_bias_shape(device, flags, dtype):
    call = br.make_call(B, HQ, 2, 70, 300, 64, dtype, False, flags, seed=7, with_dlse=True)
    got = _run(call, device)
    assert got.dbias.shape == call["bias"].shape
    _check(got, call)
    if flags != (0, 0, 0):      # the sum in unit order, no atomics: the same bits on every run
        assert torch.equal(_run(call, device).dbias, got.dbias)


def test_row_broadcast_key_padding_bias(device):
    nq, nk = 70, 300
    call = br.make_call(B, HQ, 2, nq, nk, 64, BF, False, (0, 1, 1), seed=9)
    call["bias"][0, :, :, 250:] = br.NEG_INF         # a key-padding bias: the tail of each batch element's keys masked
    call["bias"][1, :, :, 290:] = br.NEG_INF
    got = _run(call, device, need_dbias=False)
    _check(got, call)
    assert bool((got.dk.reshape(B, 2, nk, 64)[0, :, 250:] == 0).all()) and bool((got.dv.reshape(B, 2, nk, 64)[1, :, 290:] == 0).all())
    with pytest.raises(NotImplementedError, match="row-broadcast"):
        _run(call, device, need_dbias=True)


@pytest.mark.parametrize("causal", [False, True])
def test_minus_inf_entries(device, causal):
    call = br.make_call(B, HQ, 4, 70, 300, 64, F16, causal, seed=13, with_dlse=True, inf_frac=0.3, dead_rows=0)
    call["bias"][:, :, 5] = br.NEG_INF
    call["bias"][1, 2, 33:40] = br.NEG_INF
    got = _run(call, device)
    ref = _check(got, call)
    assert torch.equal(got.lse == br.NEG_INF, ref.lse == br.NEG_INF) and bool((got.lse[:, 5] == br.NEG_INF).all())
    assert bool((got.o[ref.dead_rows] == 0).all()) and bool((got.dq[ref.dead_rows] == 0).all())
    assert bool((got.dbias[call["bias"] == br.NEG_INF] == 0).all())


def test_padding_sentinel_and_skipped_tiles_are_written(device):
    """causal with Nk > Nq + 256: whole key tiles right of the diagonal are skipped, and still every element [:Nq, :Nk] is written
    into a buffer that held NaN, while the padding columns keep their sentinel"""
    nq, nk = 40, 333
    call = br.make_call(B, HQ, 4, nq, nk, 64, BF, True, seed=17)
    q, k, v, do = (call[n].to(device) for n in ("q", "k", "v", "do"))
    bias_d = _padded(call["bias"], device)
    o, lse = ext.ex_forward(q, k, v, True, call["scale"], attn_bias=bias_d)
    nkp = (nk + 7) // 8 * 8
    buf = torch.full((B, HQ, nq, nkp), float("nan"), dtype=BF, device=device)
    buf[..., nk:] = 7.0
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty((int(ext._lib.fa_ex_backward_workspace_bytes_bias(B * HQ, 1, nq, nk, 64, 2, 0)),), dtype=torch.uint8, device=device)
    a = _raw_args(q, k, v, o, lse, do, dq, dk, dv, ws, call, bias_d, buf, (HQ * nq * nkp, nq * nkp, nkp))
    assert _raw("fa_ex_backward_bias", a) == 0, ext._lib.fa_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[..., nk:] == 7.0).all()) and not torch.isnan(buf[..., :nk]).any()
    got = br.BiasResult(o.cpu(), lse.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), buf[..., :nk].cpu(), None, None, None, None, None, None)
    _check(got, call)
    above = torch.arange(nk).unsqueeze(0) > torch.arange(nq).unsqueeze(1) + nk - nq
    assert bool((got.dbias[..., above] == 0).all())


def test_strided_bias_view_gives_the_bits_of_its_copy(device):
    nq, nk = 70, 100
    call = br.make_call(B, HQ, 2, nq, nk, 64, F16, False, seed=19)
    wide = torch.full((B, HQ + 3, nq, 104), float("nan"), dtype=F16, device=device)
    wide[:, 2:2 + HQ, :, :nk] = call["bias"].to(device)
    view = wide[:, 2:2 + HQ, :, :nk]                                    # a head slice of a wider buffer: batch stride (H + 3) Nq 104
    a, b = _run(call, device, bias_d=view), _run(call, device)
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)


def _raw_args(q, k, v, o, lse, do, dq, dk, dv, ws, call, bias_d=None, dbias=None, dstr=(0, 0, 0), dlse=None):
    bh, nq, d = q.shape
    g = bh // k.shape[0]
    code = {F16: 1, BF: 2}[q.dtype]
    bs = (0, 1, 0, 0, 0) if bias_d is None else (bias_d.data_ptr(), HQ, bias_d.stride(0), bias_d.stride(1), bias_d.stride(2))
    return dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), do_=do.data_ptr(), dq=dq.data_ptr(),
                dk=dk.data_ptr(), dv=dv.data_ptr(), bh=bh, kv_group=g, nq=nq, nk=k.shape[1], d=d, dtype=code, causal=int(call["causal"]),
                window_left=-1, window_right=-1, softmax_scale=call["scale"], softcap=0.0, alibi_slopes=0, alibi_heads=1,
                alibi_batch_stride=0, sinks=0, sink_heads=1, dsinks=0, dlse=0 if dlse is None else dlse.data_ptr(), d_v=0, bias=bs[0],
                bias_heads=bs[1] if bias_d is not None else 0, bias_batch_stride=bs[2], bias_head_stride=bs[3], bias_row_stride=bs[4],
                dbias=0 if dbias is None else dbias.data_ptr(), dbias_batch_stride=dstr[0], dbias_head_stride=dstr[1],
                dbias_row_stride=dstr[2], mask=0, mask_bh_stride=0, block_mask=0, br=0, bc=0, dropout_p=0.0, dropout_seed=0,
                workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=torch.cuda.current_stream().cuda_stream)


def _raw(name, a):
    return getattr(ext._lib, name)(*[a[f] for f, _t in ext._SIGNATURES[name][1]])


@pytest.mark.parametrize("nq,nk,causal", [(128, 128, True), (70, 300, False)])
def test_null_bias_is_the_vdim_call_bit_for_bit(device, nq, nk, causal):
    call = br.make_call(B, HQ, 2, nq, nk, 128, BF, causal, seed=23)
    q, k, v, do = (call[n].to(device) for n in ("q", "k", "v", "do"))
    ws = torch.empty((int(ext._lib.fa_ex_backward_workspace_bytes_bias(B * HQ, 2, nq, nk, 128, 2, 0)),), dtype=torch.uint8, device=device)
    outs = []
    for suffix in ("_vdim", "_bias"):
        o, lse = torch.empty_like(q), torch.empty((B * HQ, nq), dtype=torch.float32, device=device)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        a = _raw_args(q, k, v, o, lse, do, dq, dk, dv, ws, call)
        assert _raw("fa_ex_forward" + suffix, a) == 0 and _raw("fa_ex_backward" + suffix, a) == 0, ext._lib.fa_last_error().decode()
        torch.cuda.synchronize()
        outs.append((o, lse, dq, dk, dv))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_zero_bias_and_need_dbias_false(device):
    call = br.make_call(B, HQ, 2, 70, 300, 64, BF, True, seed=29, with_dlse=True)
    with_dbias = _run(call, device)
    without = _run(call, device, need_dbias=False)
    for n in ("dq", "dk", "dv"):        # storing dS changes nothing else
        assert torch.equal(getattr(with_dbias, n), getattr(without, n))
    call["bias"] = torch.zeros_like(call["bias"])
    got = _run(call, device)
    q, k, v, do = (call[n].to(device) for n in ("q", "k", "v", "do"))
    o, lse = ext.ex_forward(q, k, v, True, call["scale"])
    dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, True, call["scale"], dlse=call["dlse"].to(device))
    plain = br.BiasResult(o.cpu(), lse.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), None, None, None, None, None, None, None)
    ref = br.bias_reference(call)._replace(dbias=None)
    base = br.rounded(br.bias_baseline(call), BF)
    for res in (plain, got._replace(dbias=None)):      # the call without a bias and the call with a zero bias: the same function
        bad, ratio = br.sharp_bar(res, ref, base, BF)
        assert not bad, (bad, ratio)


def test_autograd_with_lse_loss(device):
    b, nq, nk, d = B, 70, 300, 64
    call = br.make_call(b, HQ, 2, nq, nk, d, BF, True, seed=31, with_dlse=True)
    q4 = call["q"].reshape(b, HQ, nq, d).to(device).requires_grad_(True)
    k4 = call["k"].reshape(b, 2, nk, d).to(device).requires_grad_(True)
    v4 = call["v"].reshape(b, 2, nk, d).to(device).requires_grad_(True)
    p = _padded(call["bias"], device).detach().requires_grad_(True)
    o, lse = flash_attention_ex(q4, k4, v4, causal=True, return_lse=True, attn_bias=p)
    loss = (o.float() * call["do"].reshape(b, HQ, nq, d).to(device).float()).sum() + (lse * call["dlse"].reshape(b, HQ, nq).to(device)).sum()
    loss.backward()
    assert p.grad.shape == p.shape and p.grad.dtype == BF
    got = br.BiasResult(o.detach().reshape(b * HQ, nq, d).cpu(), lse.detach().reshape(b * HQ, nq).cpu(), q4.grad.reshape(b * HQ, nq, d).cpu(),
                        k4.grad.reshape(b * 2, nk, d).cpu(), v4.grad.reshape(b * 2, nk, d).cpu(), p.grad.cpu(), None, None, None, None, None, None)
    _check(got, call)
    # without a gradient of the bias the same call returns no dbias and the same dq
    q5 = q4.detach().clone().requires_grad_(True)
    o2 = flash_attention_ex(q5, k4.detach(), v4.detach(), causal=True, attn_bias=p.detach())
    assert torch.equal(o2, o.detach())


def test_merged_chunks_carry_the_dbias_of_the_whole_call(device):
    b, nq, nk, d, cut = B, 70, 300, 64, 136
    call = br.make_call(b, HQ, 4, nq, nk, d, BF, False, seed=37)
    q4, k4, v4 = (call[n].reshape(b, HQ, -1, d).to(device) for n in ("q", "k", "v"))
    q4 = q4.requires_grad_(True)
    pa = _padded(call["bias"][..., :cut], device).detach().requires_grad_(True)
    pb = _padded(call["bias"][..., cut:], device).detach().requires_grad_(True)
    oa, la = flash_attention_ex(q4, k4[:, :, :cut], v4[:, :, :cut], return_lse=True, attn_bias=pa)
    ob, lb = flash_attention_ex(q4, k4[:, :, cut:], v4[:, :, cut:], return_lse=True, attn_bias=pb)
    o, _lse = merge_attention_states(oa, la, ob, lb)
    (o.float() * call["do"].reshape(b, HQ, nq, d).to(device).float()).sum().backward()
    dbias = torch.cat([pa.grad, pb.grad], -1).cpu()
    ref = br.bias_reference(call)
    base = br.rounded(br.bias_baseline(call), BF)
    err = (dbias.double() - ref.dbias).abs().max().item()
    eb = (base.dbias.double() - ref.dbias).abs().max().item()
    assert err <= 2.0 * eb + torch.finfo(BF).eps * ref.dbias.abs().max().item(), (err, eb)
