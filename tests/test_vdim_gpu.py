"""GPU: attention with v narrower than q and k (fa_ex_*_vdim; MLA prefill, 192 + 128 head dims) through flash_attention_ex,
flash_attention_varlen and the raw C ABI, against the fp64 reference of tests/vdim_ref.py on the 16-bit-rounded inputs.

Bars: tests/helpers.py::dtype_tolerances for o, dq, dk, dv; rtol = atol = 1e-3 on finite lse (as tests/test_dlse_gpu.py), -inf rows
compare as -inf.  The shapes are small and cross every tile edge of the kernels: 32-row / 32-key blocks, the 64-key tiles of the
forward and dQ kernels, the 256-row / 256-key workgroup tiles and the 32-row query tiles of the dK/dV kernel.

Measured on the MI355X (profiles/vdim.md), max |error| against fp64 over test 1's shapes, the bar being 5e-2:
    bf16  o 7.7e-3  dq 1.24e-2  dk 1.02e-2  dv 1.07e-2        f16  o 9.1e-4  dq 1.1e-3  dk 1.4e-3  dv 1.7e-3        lse 5.9e-7 (bar 1e-3)"""
import ctypes
import functools

import pytest
import torch

from tests.helpers import dtype_tolerances
from tests.vdim_ref import vdim_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
LSE_TOL = {"rtol": 1e-3, "atol": 1e-3}


def _randn(gen, *shape, dtype=torch.bfloat16):
    return torch.randn(shape, generator=gen).to(dtype)


def _close(name, got, want, dtype, errs=None):
    got = got.detach().double().cpu()
    err = (got - want).abs().max().item() if got.numel() else 0.0
    if errs is not None:
        errs[name] = max(errs.get(name, 0.0), err)
    print(f"{name}: max |err| = {err:.3e}")
    torch.testing.assert_close(got, want, **dtype_tolerances(dtype), msg=lambda m: f"{name}: {m}")


def _close_lse(got, want):
    got = got.detach().double().cpu()
    dead = torch.isneginf(want)
    assert torch.equal(torch.isneginf(got), dead), "lse: the rows without a visible key differ"
    if bool((~dead).any()):
        print(f"lse: max |err| = {(got[~dead] - want[~dead]).abs().max().item():.3e}")
    torch.testing.assert_close(got[~dead], want[~dead], **LSE_TOL)


def _problem(seed, h, hkv, nq, nk, d, dv, dtype):
    gen = torch.Generator().manual_seed(seed)
    return (_randn(gen, 1, h, nq, d, dtype=dtype), _randn(gen, 1, hkv, nk, d, dtype=dtype), _randn(gen, 1, hkv, nk, dv, dtype=dtype),
            _randn(gen, 1, h, nq, dv, dtype=dtype))


def _run(q, k, v, do, causal, **kw):
    """(o, dq, dk, dv) of flash_attention_ex on the device"""
    from common.attention_ex import flash_attention_ex

    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o = flash_attention_ex(qd, kd, vd, causal=causal, **kw)
    o.backward(do.to(DEV))
    return o, qd.grad, kd.grad, vd.grad


def _check(q, k, v, do, causal, dtype, errs=None):
    d = q.shape[-1]
    o, dq, dk, dv = _run(q, k, v, do, causal)
    assert o.shape == q.shape[:-1] + (v.shape[-1],) and dv.shape == v.shape and dk.shape == k.shape and dq.shape == q.shape
    ro, _rlse, (rdq, rdk, rdv) = vdim_reference(q[0], k[0], v[0], causal, d ** -0.5, do[0])   # the default scale: q's width
    _close("o", o[0], ro, dtype, errs)
    _close("dq", dq[0], rdq, dtype, errs)
    _close("dk", dk[0], rdk, dtype, errs)
    _close("dv", dv[0], rdv, dtype, errs)
    return o, dq, dk, dv


# ---- 1. the MLA widths against fp64, forward and backward
MLA_CASES = [(300, 300, True), (300, 300, False), (77, 333, True), (333, 77, True), (1, 1, True), (1, 1, False), (257, 129, False),
             (257, 129, True)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("nq,nk,causal", MLA_CASES)
def test_mla_widths_match_fp64_forward_and_backward(device, nq, nk, causal, dtype):
    """On the commit before the feature this raises RuntimeError (v.shape != k.shape)."""
    q, k, v, do = _problem(1, 2, 2, nq, nk, 192, 128, dtype)
    o, dq, _dk, _dv = _check(q, k, v, do, causal, dtype)
    if causal and nq > nk:   # rows with no visible key: o = 0 and no gradient from them
        assert not bool(o[0, :, :nq - nk].any()) and not bool(dq[0, :, :nq - nk].any())


# ---- 2. other width pairs: the padding of both widths must not leak
@pytest.mark.parametrize("d,dv", [(72, 40), (192, 8), (136, 128), (64, 32)])
def test_other_width_pairs(device, d, dv):
    q, k, v, do = _problem(2, 2, 2, 130, 130, d, dv, torch.bfloat16)
    _check(q, k, v, do, True, torch.bfloat16)


# ---- 3. GQA: dk and dv summed per group, each at its own width
@pytest.mark.parametrize("hkv", [1, 2])
def test_gqa(device, hkv):
    q, k, v, do = _problem(3, 4, hkv, 200, 200, 192, 128, torch.bfloat16)
    _check(q, k, v, do, True, torch.bfloat16)


# ---- 4. packed sequences
LENS_Q, LENS_K = [0, 1, 130, 300], [5, 1, 130, 260]


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _packed():
    gen = torch.Generator().manual_seed(4)
    tq, tk, h = sum(LENS_Q), sum(LENS_K), 2
    qkv = _randn(gen, tq, 3, h, 192)               # q is the token-strided view qkv[:, 1]
    return qkv, _randn(gen, tk, h, 192), _randn(gen, tk, h, 128), _randn(gen, tq, h, 128)


@pytest.mark.parametrize("causal", [True, False])
def test_packed_sequences_match_fp64_each_alone(device, causal):
    from common.attention_ex import flash_attention_varlen

    qkv, k, v, do = _packed()
    qkv_d = qkv.to(DEV).requires_grad_(True)
    kd, vd = k.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    qd = qkv_d[:, 1]
    assert qd.stride(0) == 3 * 2 * 192
    o = flash_attention_varlen(qd, kd, vd, _cu(LENS_Q).to(DEV), _cu(LENS_K).to(DEV), max(LENS_Q), max(LENS_K), causal=causal)
    assert o.shape == (sum(LENS_Q), 2, 128)
    o.backward(do.to(DEV))
    dq, dk, dv = qkv_d.grad[:, 1], kd.grad, vd.grad
    assert dk.shape == k.shape and dv.shape == v.shape
    q0 = k0 = 0
    for lq, lk in zip(LENS_Q, LENS_K):
        sl_q, sl_k = slice(q0, q0 + lq), slice(k0, k0 + lk)
        ro, _rl, (rdq, rdk, rdv) = vdim_reference(qkv[sl_q, 1].transpose(0, 1), k[sl_k].transpose(0, 1), v[sl_k].transpose(0, 1), causal,
                                                  192 ** -0.5, do[sl_q].transpose(0, 1))
        _close("o", o[sl_q].transpose(0, 1), ro, torch.bfloat16)
        _close("dq", dq[sl_q].transpose(0, 1), rdq, torch.bfloat16)
        _close("dk", dk[sl_k].transpose(0, 1), rdk, torch.bfloat16)
        _close("dv", dv[sl_k].transpose(0, 1), rdv, torch.bfloat16)
        q0, k0 = q0 + lq, k0 + lk


def test_cu_seqlens_past_total_are_clamped_on_the_device_without_a_host_sync(device):
    """DESIGN §9d's rule: offsets are untrusted and clamped in the kernels.  The call is captured in a graph (a host
    synchronisation would fail the capture), the offsets are then overwritten on the device with ones that run past total, and the
    replay must leave the rows of the sequences that are still valid as they were and write nothing outside o."""
    import flashattention_lab_cuda as ext

    qkv, k, v, _do = _packed()
    tq, tk, PAD, SENT = sum(LENS_Q), sum(LENS_K), 512, 7.0
    q = qkv[:, 1].contiguous().to(DEV)

    def slab(t):
        big = torch.full((t.shape[0] + 2 * PAD,) + tuple(t.shape[1:]), SENT, dtype=t.dtype, device=DEV)
        big[PAD:PAD + t.shape[0]] = t.to(DEV)
        return big, big[PAD:PAD + t.shape[0]]
    (kb, kd), (vb, vd) = slab(k), slab(v)
    cu_q, cu_k = _cu(LENS_Q).to(DEV), _cu(LENS_K).to(DEV)
    want, _ = ext.ex_varlen_forward(q, kd, vd, cu_q, cu_k, max(LENS_Q), max(LENS_K), True, 192 ** -0.5)   # (and the warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out, lse = ext.ex_varlen_forward(q, kd, vd, cu_q, cu_k, max(LENS_Q), max(LENS_K), True, 192 ** -0.5)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # the last sequence's end runs far past both totals (written on the device, never read on the host)
    bad_q, bad_k = _cu(LENS_Q), _cu(LENS_K)
    bad_q[-1] += 100000
    bad_k[-1] += 100000
    cu_q.copy_(bad_q.to(DEV))
    cu_k.copy_(bad_k.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    owned = tq - LENS_Q[-1]                     # the rows of the sequences whose offsets are still what they were
    assert torch.equal(out[:owned], want[:owned])
    # clamped to total the last sequence is the one it was: same tokens, same lengths
    assert torch.equal(out, want)
    assert bool((kb[:PAD] == SENT).all()) and bool((kb[PAD + tk:] == SENT).all()) and bool((vb[PAD + tk:] == SENT).all())
    assert bool(torch.isfinite(out.float()).all())


# ---- 5. lse
def test_return_lse_with_a_loss_on_o_and_lse(device):
    from common.attention_ex import flash_attention_ex

    q, k, v, do = _problem(5, 2, 2, 200, 150, 192, 128, torch.bfloat16)   # causal with Nq > Nk: 50 rows whose lse is -inf
    dlse = torch.randn((1, 2, 200), generator=torch.Generator().manual_seed(55))
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o, lse = flash_attention_ex(qd, kd, vd, causal=True, return_lse=True)
    assert lse.shape == (1, 2, 200) and lse.dtype == torch.float32
    finite = torch.isfinite(lse)
    loss = (o.float() * do.to(DEV).float()).sum() + (torch.where(finite, lse, torch.zeros_like(lse)) * dlse.to(DEV)).sum()
    loss.backward()
    ro, rlse, (rdq, rdk, rdv) = vdim_reference(q[0], k[0], v[0], True, 192 ** -0.5, do[0], dlse[0])
    _close("o", o[0], ro, torch.bfloat16)
    _close_lse(lse[0], rlse)
    _close("dq", qd.grad[0], rdq, torch.bfloat16)
    _close("dk", kd.grad[0], rdk, torch.bfloat16)
    _close("dv", vd.grad[0], rdv, torch.bfloat16)


def test_two_key_chunks_merge_into_the_one_causal_call(device):
    """Chunked MLA prefill composes with merge_attention_states: 100 new tokens behind a 200-token prefix.  The prefix, which every
    row sees whole, is a causal=False call, the trailing 100 keys the causal=True call; merged they are the causal call over
    the 300 keys, gradients included."""
    from common.attention_ex import flash_attention_ex
    from common.merge_states import merge_attention_states

    q, k, v, do = _problem(6, 2, 2, 100, 300, 192, 128, torch.bfloat16)
    one = _run(q, k, v, do, True)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    oa, la = flash_attention_ex(qd, kd[:, :, :200], vd[:, :, :200], causal=False, return_lse=True, softmax_scale=192 ** -0.5)
    ob, lb = flash_attention_ex(qd, kd[:, :, 200:], vd[:, :, 200:], causal=True, return_lse=True, softmax_scale=192 ** -0.5)
    o, _lse = merge_attention_states(oa, la, ob, lb)
    o.backward(do.to(DEV))
    for name, got, want in zip(("o", "dq", "dk", "dv"), (o, qd.grad, kd.grad, vd.grad), one):
        _close(name, got, want.detach().double().cpu(), torch.bfloat16)


# ---- 6. nothing old moved: the new entry points with d_v = 0 and d_v = d give the bits of the widest existing member
D0, N0, BH0, CODE = 64, 96, 4, 2
NOMASK = [None, 0, None, 0, 0, 0.0, 0]   # mask, mask_bh_stride, block_mask, br, bc, dropout_p, dropout_seed
MODS = [0.0, None, 1, 0, None, 1]        # softcap, alibi_slopes, alibi_heads, alibi_batch_stride, sinks, sink_heads


def _ok(rc):
    import flashattention_lab_cuda as ext

    assert rc == 0, ext._lib.fa_last_error().decode()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ex_raw(d_v):
    """(o, lse, dq, dk, dv) through fa_ex_forward_sink / fa_ex_backward_dlse (d_v None) or the _vdim entry points"""
    import flashattention_lab_cuda as ext

    lib = ext._lib
    gen = torch.Generator().manual_seed(61)
    q, k, v, do = (_randn(gen, BH0, N0, D0).to(DEV) for _ in range(4))
    o, lse = torch.empty_like(q), torch.empty((BH0, N0), dtype=torch.float32, device=DEV)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dims = [BH0, 1, N0, N0, D0, CODE, 1, -1, -1, D0 ** -0.5]
    extra = [] if d_v is None else [d_v]
    fwd = lib.fa_ex_forward_sink if d_v is None else lib.fa_ex_forward_vdim
    bwd = lib.fa_ex_backward_dlse if d_v is None else lib.fa_ex_backward_vdim
    _ok(fwd(*[t.data_ptr() for t in (q, k, v, o, lse)], *dims, *MODS, *extra, *NOMASK, _stream()))
    nbytes = int(lib.fa_ex_backward_workspace_bytes_grouped(BH0, 1, N0, N0, D0, CODE))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    _ok(bwd(*[t.data_ptr() for t in (q, k, v, o, do, lse, dq, dk, dv)], *dims, *MODS, None, None, *extra, *NOMASK, ws.data_ptr(), nbytes,
            _stream()))
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def _varlen_raw(d_v):
    import flashattention_lab_cuda as ext

    lib = ext._lib
    gen = torch.Generator().manual_seed(62)
    hq, hkv, lens = 4, 2, (N0, N0)
    total = sum(lens)
    q, do = _randn(gen, total, hq, D0).to(DEV), _randn(gen, total, hq, D0).to(DEV)
    k, v = _randn(gen, total, hkv, D0).to(DEV), _randn(gen, total, hkv, D0).to(DEV)
    cu = _cu(lens).to(DEV)
    o, lse = torch.empty_like(q), torch.empty((hq, total), dtype=torch.float32, device=DEV)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dims = [cu.data_ptr(), cu.data_ptr(), len(lens), hq, hkv, total, total, N0, N0, D0, CODE, hq * D0, hkv * D0, hkv * D0, 1, -1, -1, D0 ** -0.5]
    mods = [0.0, None, 0, None, 1]      # softcap, alibi_slopes, alibi_batch_stride, sinks, sink_heads
    extra = [] if d_v is None else [d_v]
    fwd = lib.fa_ex_forward_varlen_sink if d_v is None else lib.fa_ex_forward_varlen_vdim
    bwd = lib.fa_ex_backward_varlen_dlse if d_v is None else lib.fa_ex_backward_varlen_vdim
    _ok(fwd(*[t.data_ptr() for t in (q, k, v, o, lse)], *dims, *mods, *extra, 0.0, 0, _stream()))
    nbytes = int(lib.fa_ex_backward_workspace_bytes_varlen(hq, hkv, total, total, D0, CODE))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    _ok(bwd(*[t.data_ptr() for t in (q, k, v, o, do, lse, dq, dk, dv)], *dims, *mods, None, None, *extra, 0.0, 0, ws.data_ptr(), nbytes,
            _stream()))
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("raw", [_ex_raw, _varlen_raw], ids=["padded", "varlen"])
@pytest.mark.parametrize("d_v", [0, D0])
def test_new_entry_points_without_a_second_width_give_the_old_bits(device, raw, d_v):
    for name, got, want in zip(("o", "lse", "dq", "dk", "dv"), raw(d_v), raw(None)):
        assert torch.equal(got, want), name


# ---- 7. repeatability
def test_two_runs_are_bit_equal(device):
    q, k, v, do = _problem(1, 2, 2, 300, 300, 192, 128, torch.bfloat16)
    first, second = _run(q, k, v, do, True), _run(q, k, v, do, True)
    for name, a, b in zip(("o", "dq", "dk", "dv"), first, second):
        assert torch.equal(a, b), name
