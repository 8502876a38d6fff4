"""CPU: FlashAttention-3's fp8 call (include/fa_mi355x.h: fa_fp8_forward, fa_fp8_forward_workspace_bytes) — declared,
exported, the signature rows and a family of its own, every bad argument rejected before any HIP call in the documented order, the
workspace formula, the Python wrappers' refusals by name, and the proofs behind tests/test_fp8_inputs_gpu.py: the reference is
ex_full_ref's on the dequantised tensors, the baseline without rounding is the reference, every mutant fails the sharp bar
somewhere while the baseline passes everywhere, and the growing input exercises the lazy rescale."""
import ctypes
import functools
import os
import re

import pytest
import torch

from tests import ex_full_ref as ex
from tests import fp8_inputs_cases as fc
from tests import fp8_inputs_ref as fr
from tests.fp8_ref import tiled_sharp_bar
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_fp8_forward", "fa_fp8_forward_workspace_bytes")
OK, INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

ORDER = ("q", "k", "v", "o", "lse", "qd", "kd", "vd", "b", "hq", "hkv", "nq", "nk", "d", "dtype", "qb", "qh", "qt", "kb", "kh", "kt", "vb", "vh",
         "vt", "ob", "oh", "ot", "qdb", "kdb", "vdb", "causal", "scale", "ws", "wsb")
# B = 2, H_q = 4, H_kv = 2, Nq = 300, Nk = 500, bf16 out, contiguous (B, H, N, 128) tensors, (B, H_kv) descales, an ample workspace
BASE = dict(q=P, k=P, v=P, o=P, lse=P, qd=P, kd=P, vd=P, b=2, hq=4, hkv=2, nq=300, nk=500, d=128, dtype=2, qb=4 * 300 * 128, qh=300 * 128,
            qt=128, kb=2 * 500 * 128, kh=500 * 128, kt=128, vb=2 * 500 * 128, vh=500 * 128, vt=128, ob=4 * 300 * 128, oh=300 * 128, ot=128,
            qdb=2, kdb=2, vdb=2, causal=1, scale=128 ** -0.5, ws=P, wsb=2 ** 40)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **kw)
    rc = ext._lib.fa_fp8_forward(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext
    from common import attention_ex

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS
    assert hasattr(ext, "fp8_forward") and hasattr(attention_ex, "flash_attention_fp8")


def test_signature_rows_and_a_family_of_its_own():
    import flashattention_lab_cuda as ext

    names = PROTOTYPES["fa_fp8_forward"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_fp8_forward"][1]] == names and len(names) == len(ORDER) + 1   # (ORDER: all but the stream)
    assert names[:8] == ["q", "k", "v", "o", "lse", "q_descale", "k_descale", "v_descale"]
    assert names[8:15] == ["batch", "heads_q", "heads_kv", "seqlen_q", "seqlen_k", "d", "dtype"]
    assert names[-5:] == ["causal", "softmax_scale", "workspace", "workspace_bytes", "stream"]
    assert PROTOTYPES["fa_fp8_forward"][1][15:30] == [ctypes.c_int64] * 15
    assert PROTOTYPES["fa_fp8_forward_workspace_bytes"][2] == ["batch", "heads_kv", "seqlen_k", "d"]
    assert PROTOTYPES["fa_fp8_forward_workspace_bytes"][0] is ctypes.c_size_t
    # the only member of its family, handed exactly its own arguments; fa3_forward's row is what it was
    fn, own, count = ext._CALLS["fa_fp8_forward"]
    assert count == len(names) and list(own(tuple(names))) == names
    assert [f for f, _t in ext._SIGNATURES["fa3_forward"][1]][-5:] == ["stages", "fp8", "workspace", "workspace_bytes", "stream"]


# every row is rejected before any HIP call: there is no GPU here, and the pointers are fake.  In the documented order: a later
# rule's breach does not hide an earlier one (the rows with two breaches).
BAD = [
    # (1) null pointers, before the dims
    (dict(q=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(k=None, b=0), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(v=None, d=64), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(o=None), INVALID_ARGUMENT, "null tensor pointer"),
    (dict(lse=None, dtype=0), INVALID_ARGUMENT, "null tensor pointer"),
    # (2) dims > 0, before the head dim
    (dict(b=0), INVALID_ARGUMENT, "must be > 0"),
    (dict(hq=0, d=64), INVALID_ARGUMENT, "must be > 0"),
    (dict(hkv=-1), INVALID_ARGUMENT, "must be > 0"),
    (dict(nq=0), INVALID_ARGUMENT, "must be > 0"),
    (dict(nk=0, dtype=7), INVALID_ARGUMENT, "must be > 0"),
    (dict(d=0), INVALID_ARGUMENT, "must be > 0"),
    # (3) d == 128, before the heads ratio
    (dict(d=64), UNSUPPORTED, "head_dim 64 is not supported (128 only)"),
    (dict(d=256, hq=3), UNSUPPORTED, "head_dim 256 is not supported"),
    # (4) the heads ratio, before the dtype
    (dict(hq=3), INVALID_ARGUMENT, "heads_q=3 must be a multiple of heads_kv=2"),
    (dict(hq=2, hkv=4, dtype=0), INVALID_ARGUMENT, "heads_q=2 must be a multiple of heads_kv=4"),
    # (5) dtype, scale, descale strides, before the alignment
    (dict(dtype=0), INVALID_ARGUMENT, "dtype (of o) must be f16 or bf16 (got code 0)"),
    (dict(dtype=3, q=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "dtype (of o) must be f16 or bf16 (got code 3)"),
    (dict(scale=0.0), INVALID_ARGUMENT, "softmax_scale must be finite and > 0"),
    (dict(scale=float("nan"), qt=100), INVALID_ARGUMENT, "softmax_scale must be finite and > 0"),
    (dict(scale=float("inf")), INVALID_ARGUMENT, "softmax_scale must be finite and > 0"),
    (dict(qdb=1), INVALID_ARGUMENT, "q_descale_batch_stride=1 must be 0 or >= heads_kv=2"),
    (dict(kdb=-2), INVALID_ARGUMENT, "k_descale_batch_stride=-2 must be 0 or >= heads_kv=2"),
    (dict(vd=None), INVALID_ARGUMENT, "v_descale_batch_stride must be 0 without v_descale"),
    (dict(kd=ctypes.c_void_p(4096 + 2), kt=8), INVALID_ARGUMENT, "k_descale must be 4-byte aligned"),
    # (6) alignment and strides, before the span limit
    (dict(q=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "q, k, v and o must be 16-byte aligned"),
    (dict(v=ctypes.c_void_p(4096 + 4), kt=2 ** 30), INVALID_ARGUMENT, "q, k, v and o must be 16-byte aligned"),
    (dict(lse=ctypes.c_void_p(4096 + 2)), INVALID_ARGUMENT, "lse must be 4-byte aligned"),
    (dict(qt=136), INVALID_ARGUMENT, "the strides of q (153600, 38400, 136) must be multiples of 16 elements"),
    (dict(kh=500 * 128 + 8), INVALID_ARGUMENT, "the strides of k"),
    (dict(vb=2 * 500 * 128 + 4, ws=None), INVALID_ARGUMENT, "the strides of v"),
    (dict(ot=132), INVALID_ARGUMENT, "the strides of o (153600, 38400, 132) must be multiples of 8 elements"),
    (dict(kt=64), INVALID_ARGUMENT, "the token stride >= 128"),
    (dict(qb=-16), INVALID_ARGUMENT, "must be >= 0"),
    # (7) the span limit, by name, before the workspace
    (dict(kt=2 ** 22), UNSUPPORTED, "span limit: round_up(rows, 256) * token stride of k is 2147483648 bytes"),
    (dict(qt=2 ** 23, ws=None), UNSUPPORTED, "span limit: round_up(rows, 256) * token stride of q"),
    (dict(b=2 ** 20, hq=2 ** 11, hkv=2 ** 11, qdb=2 ** 11, kdb=2 ** 11, vdb=2 ** 11), INVALID_ARGUMENT, "descale_batch_stride"),
    (dict(b=2 ** 20, hq=2 ** 11, hkv=2 ** 11, qd=None, kd=None, vd=None, qdb=0, kdb=0, vdb=0), UNSUPPORTED, "span limit: batch * heads * tiles"),
    # (8) the workspace
    (dict(ws=None), WORKSPACE, "workspace of 0 bytes is too small (need 262400"),
    (dict(wsb=262399), WORKSPACE, "workspace of 262399 bytes is too small (need 262400"),
    (dict(ws=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("kw,code,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _call(**kw)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_fp8_forward:"), (kw, msg)


def test_strides_of_extent_one_dims_are_not_looked_at():
    """B = H = N = 1 with odd strides passes every rule up to the workspace"""
    rc, msg = _call(b=1, hq=1, hkv=1, nq=1, nk=1, qb=7, qh=3, qt=5, kb=1, kh=1, kt=1, vb=9, vh=9, vt=9, ob=3, oh=3, ot=3, ws=None)
    assert rc == WORKSPACE and "need 16640" in msg, msg


def test_the_workspace_formula():
    import flashattention_lab_cuda as ext

    f = ext._lib.fa_fp8_forward_workspace_bytes
    for b, hkv, nk in ((1, 1, 1), (2, 2, 500), (2, 1, 128), (3, 8, 129), (2, 2, 16384)):
        assert f(b, hkv, nk, 128) == b * hkv * ((nk + 127) // 128) * 16384 + 256
    assert f(2, 2, 500, 128) == 262400
    for bad in ((0, 1, 1, 128), (1, 0, 1, 128), (1, 1, 0, 128), (1, 1, 1, 64), (-1, 1, 1, 128)):
        assert f(*bad) == 0
    for i, c in enumerate(fc.CASES[:6]):
        call = fc.build_call(c, i)
        assert f(call["B"], call["hkv"], call["nk"], 128) == fr.workspace_bytes(call)


def test_the_wrappers_refuse_by_name():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_fp8

    q8 = torch.zeros((2, 2, 16, 128), dtype=torch.float8_e4m3fn)
    q16 = torch.zeros((2, 2, 16, 128), dtype=torch.bfloat16)
    for name, val in (("window_size", (8, 0)), ("softcap", 30.0), ("alibi_slopes", torch.ones(2)), ("sinks", torch.zeros(2)),
                      ("attn_bias", torch.zeros(16, 16)), ("mask", torch.ones(16, 16)), ("block_sparse_mask", torch.ones(1, 1)),
                      ("dropout_p", 0.1)):
        with pytest.raises(NotImplementedError, match=f"flash_attention_fp8: {name} is not supported"):
            flash_attention_fp8(q8, q8, q8, **{name: val})
    with pytest.raises(TypeError, match="unexpected keyword argument 'nonsense'"):
        flash_attention_fp8(q8, q8, q8, nonsense=1)
    with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: q is torch.bfloat16"):
        flash_attention_fp8(q16, q8, q8)
    with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: v is torch.bfloat16"):
        flash_attention_fp8(q8, q8, q16)
    with pytest.raises(NotImplementedError, match="k of dtype torch.uint8 is not supported"):
        flash_attention_fp8(q8, q8.view(torch.uint8), q8)
    with pytest.raises(NotImplementedError, match="head_dim 64 is not supported"):
        flash_attention_fp8(q8[..., :64], q8[..., :64], q8[..., :64])
    with pytest.raises(NotImplementedError, match="out_dtype torch.float32 is not supported"):
        flash_attention_fp8(q8, q8, q8, out_dtype=torch.float32)
    # the defaults of the refused arguments pass through to the shim, which has no CPU path
    with pytest.raises(RuntimeError, match="tensors must be on the GPU"):
        flash_attention_fp8(q8, q8, q8, window_size=(-1, -1), softcap=0.0, dropout_p=0.0, sinks=None)
    with pytest.raises(NotImplementedError, match="fp8_forward: q of dtype torch.bfloat16 is not supported"):
        ext.fp8_forward(q16, q8, q8, False, None)
    with pytest.raises(ValueError, match="layout must be one of"):
        ext.fp8_forward(q8, q8, q8, False, None, layout="thd")
    with pytest.raises(NotImplementedError, match="out_dtype torch.float32"):
        ext.fp8_forward(q8, q8, q8, False, None, out_dtype=torch.float32)


# ---- the proofs behind the GPU sweep

@functools.lru_cache(maxsize=None)
def _case(i):
    call = fc.build_call(fc.CASES[i], i)
    trace = []
    return call, fr.reference(call), fr.baseline(call, trace=trace), trace


IDS = [fc.case_id(c, i) for i, c in enumerate(fc.CASES)]


def test_the_table_covers_every_pair_under_its_cap():
    import itertools

    assert len(fc.CASES) <= fc.MAX_CASES
    for a, b in itertools.combinations(fc.AXES, 2):
        assert {(c[a], c[b]) for c in fc.CASES} == set(itertools.product(fc.AXES[a], fc.AXES[b])), (a, b)


def test_the_inputs_are_finite_e4m3_and_use_the_clamp():
    for i in range(len(fc.CASES)):
        call = _case(i)[0]
        for name in ("q8", "k8", "v8"):
            assert not bool(((call[name] & 0x7F) == 0x7F).any()), (i, name)      # no NaN code
    assert torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all()   # why build_call clamps


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_reference_is_the_full_reference_on_the_dequantised_tensors(i):
    call, ref, _base, _trace = _case(i)
    full = ex.full_reference(fr.ex_call(call))
    torch.testing.assert_close(ref.o, full.o, rtol=1e-12, atol=1e-12)
    assert torch.equal(torch.isfinite(ref.lse), torch.isfinite(full.lse)) and torch.equal(ref.lse == ex.NEG_INF, full.dead_rows)
    fin = torch.isfinite(ref.lse)
    torch.testing.assert_close(ref.lse[fin], full.lse[fin], rtol=1e-12, atol=1e-12)
    assert bool((ref.o[~fin] == 0).all())


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_baseline_without_rounding_is_the_reference(i):
    call, ref, base, _trace = _case(i)
    b64 = fr.baseline(call, compute=torch.float64, rounding=False)
    fin = torch.isfinite(ref.lse)
    assert torch.equal(torch.isfinite(b64.lse), fin) and bool((b64.lse[~fin] == ex.NEG_INF).all())
    assert float((b64.o - ref.o).abs().max()) <= 1e-10 * max(1.0, float(ref.o.abs().max()))
    if fin.any():
        assert float((b64.lse[fin] - ref.lse[fin]).abs().max()) <= 1e-10 * max(1.0, float(ref.lse[fin].abs().max()))
    # and the rounded baseline is finite, -inf / 0 exactly on the dead rows, and passes its own bar
    assert torch.equal(torch.isfinite(base.lse), fin) and bool((base.o[~fin] == 0).all()) and bool(torch.isfinite(base.o).all())
    bad, _ratio = tiled_sharp_bar(fr.rounded(base, call["dtype"]), ref, base, call["dtype"])
    assert not bad, bad


@pytest.mark.parametrize("name", fr.MUTANTS)
def test_every_mutant_fails_the_sharp_bar_somewhere(name):
    applied, caught = 0, []
    for i in range(len(fc.CASES)):
        call, ref, base, _trace = _case(i)
        mut = fr.mutant(call, name)
        if mut is None:
            continue
        applied += 1
        got = fr.rounded(mut, call["dtype"])
        bad, _ratio = tiled_sharp_bar(got, ref, base, call["dtype"])
        dead = ~torch.isfinite(ref.lse)
        if bad or not torch.equal(~torch.isfinite(got.lse), dead) or bool((got.o[dead] != 0).any()) or bool(torch.isnan(got.o).any()):
            caught.append(IDS[i])
    assert applied > 0, name
    assert caught, (name, applied)


def test_the_growing_input_exercises_the_lazy_rescale():
    """on the baseline's own trace: some wave rescales at least three times, and at some tile after the first some wave keeps a row on
    a stale max (its own max grew, by no more than 2^8) while another wave of the same launch moves"""
    most, stale_beside_move = 0, False
    for i, c in enumerate(fc.CASES):
        if c["input"] != "growing":
            continue
        trace = _case(i)[3]
        count = {}
        for t, r0, moved, stale in trace:
            w = moved[:, ::32]                                         # one flag per wave
            count[r0] = count.get(r0, 0) + w.to(torch.int64)
            if t > 0 and bool(stale.any()) and bool(moved.any()):
                stale_beside_move = True
        most = max([most] + [int(v.max()) for v in count.values()])
    assert most >= 3, most
    assert stale_beside_move


def test_expected_v8t_inverts_to_v_and_zeroes_the_pads():
    from tests.fp8_ref import decode_v8t

    for i in (2, 6, 8):
        call = _case(i)[0]
        nk, units = call["nk"], call["B"] * call["hkv"]
        v8t = fr.expected_v8t(call)
        assert v8t.numel() + 256 == fr.workspace_bytes(call)
        dec = decode_v8t(v8t.reshape(-1), units, nk)
        assert torch.equal(dec[:, :nk], call["v8"].reshape(units, nk, 128)) and bool((dec[:, nk:] == 0).all())
