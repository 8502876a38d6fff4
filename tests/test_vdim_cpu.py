"""CPU: attention with v narrower than q and k (include/fa_mi355x.h: fa_ex_forward_vdim, fa_ex_backward_vdim,
fa_ex_forward_varlen_vdim, fa_ex_backward_varlen_vdim) — declared, exported, the signature rows and families, every refusal raised
by name from Python, the first-broken-rule error texts of the four *_impl functions before any HIP call, d_v = 0 / d_v = d falling
through to the checks of the call without the argument, and the fp64 reference (tests/vdim_ref.py) against a direct computation."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_abi_signatures_cpu import PROTOTYPES
from tests.vdim_ref import vdim_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_ex_forward_vdim", "fa_ex_backward_vdim", "fa_ex_forward_varlen_vdim", "fa_ex_backward_varlen_vdim")
WIDEST_BEFORE = {"fa_ex_forward_vdim": "fa_ex_forward_sink", "fa_ex_backward_vdim": "fa_ex_backward_dlse",
                 "fa_ex_forward_varlen_vdim": "fa_ex_forward_varlen_sink", "fa_ex_backward_varlen_vdim": "fa_ex_backward_varlen_dlse"}
AFTER = {"fa_ex_forward_vdim": "sink_heads", "fa_ex_backward_vdim": "dlse", "fa_ex_forward_varlen_vdim": "sink_heads",
         "fa_ex_backward_varlen_vdim": "dlse"}
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


@pytest.mark.parametrize("name", NAMES)
def test_one_argument_after_the_widest_member_and_a_family_of_its_own(name):
    import flashattention_lab_cuda as ext

    names, old = PROTOTYPES[name][2], PROTOTYPES[WIDEST_BEFORE[name]][2]
    at = names.index("d_v")
    assert names[at - 1] == AFTER[name] and PROTOTYPES[name][1][at] is ctypes.c_int64
    assert names[:at] + names[at + 1:] == old                       # the widest existing member plus the one argument
    assert [f for f, _t in ext._SIGNATURES[name][1]] == names
    assert ext._CALLS[name][2] == len(names)
    # a family of its own: the existing families, and what their members are handed, are what they were
    assert [n for n, c in ext._CALLS.items() if c[2] == len(names) and "d_v" in PROTOTYPES[n][2] and PROTOTYPES[n][2] == names] == [name]
    assert ext._CALLS[WIDEST_BEFORE[name]][2] == len(old)


# ---- the Python surface: every refusal by name, before anything touches a device
def _qkv(d=192, dv=128, dtype=torch.bfloat16, four_d=True):
    shape = (1, 2, 16) if four_d else (2, 16)
    return torch.zeros(shape + (d,), dtype=dtype), torch.zeros(shape + (d,), dtype=dtype), torch.zeros(shape + (dv,), dtype=dtype)


EX_REFUSED = [
    ("mask", dict(mask=torch.ones(16, 16))),
    ("block_sparse_mask", dict(block_sparse_mask=torch.ones(1, 1), block_size=16)),
    ("dropout_p", dict(dropout_p=0.1)),
    ("window_size", dict(window_size=(4, -1))),
    ("softcap", dict(softcap=30.0)),
    ("alibi_slopes", dict(alibi_slopes=torch.ones(2))),
    ("sinks", dict(sinks=torch.zeros(2))),
]


@pytest.mark.parametrize("name,kw", EX_REFUSED, ids=[n for n, _ in EX_REFUSED])
@pytest.mark.parametrize("four_d", [True, False])
def test_flash_attention_ex_refuses_by_name(name, kw, four_d):
    from common.attention_ex import flash_attention_ex

    with pytest.raises(NotImplementedError, match=name):
        flash_attention_ex(*_qkv(four_d=four_d), causal=True, **kw)


VARLEN_REFUSED = [
    ("dropout_p", dict(dropout_p=0.1)),
    ("window_size", dict(window_size=(-1, 8))),
    ("softcap", dict(softcap=30.0)),
    ("alibi_slopes", dict(alibi_slopes=torch.ones(2))),
    ("sinks", dict(sinks=torch.zeros(2))),
    ("block_table", dict(block_table=torch.zeros((1, 1), dtype=torch.int32))),
    ("k_descale", dict(k_descale=torch.ones(2))),
    ("v_descale", dict(v_descale=torch.ones(2))),
]


@pytest.mark.parametrize("name,kw", VARLEN_REFUSED, ids=[n for n, _ in VARLEN_REFUSED])
def test_flash_attention_varlen_refuses_by_name(name, kw):
    from common.attention_ex import flash_attention_varlen

    q, k, v = _qkv(four_d=False)
    q, k, v = q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1)      # (total, H, d)
    cu = torch.tensor([0, 16], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match=name):
        flash_attention_varlen(q, k, v, cu, cu, 16, 16, causal=True, **kw)


def test_block_table_with_pools_of_two_widths_is_refused_by_name():
    from common.attention_ex import flash_attention_varlen

    q = torch.zeros((16, 2, 192), dtype=torch.bfloat16)
    kp, vp = torch.zeros((2, 16, 2, 192), dtype=torch.bfloat16), torch.zeros((2, 16, 2, 128), dtype=torch.bfloat16)
    cu = torch.tensor([0, 16], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="block_table"):
        flash_attention_varlen(q, kp, vp, cu, cu, 16, 16, block_table=torch.zeros((1, 1), dtype=torch.int32))


WIDTHS_REFUSED = [
    (dict(d=128, dv=192), r"d_v=192 > d=128"),
    (dict(d=192, dv=100), "multiples of 8"),
    (dict(d=100, dv=64), "multiples of 8"),
    (dict(d=200, dv=128), r"d <= 192 \(got d=200\)"),
    (dict(d=192, dv=136), r"d_v <= 128 \(got d_v=136\)"),
    (dict(d=256, dv=192), r"d <= 192"),                      # the first broken rule: d before d_v
    (dict(d=192, dv=128, dtype=torch.float32), "float16 or bfloat16"),
    (dict(d=200, dv=128, dtype=torch.float32), r"d <= 192"),  # widths before the dtype
]


@pytest.mark.parametrize("kw,text", WIDTHS_REFUSED)
def test_widths_and_dtype_are_refused_by_name(kw, text):
    from common.attention_ex import flash_attention_ex, flash_attention_varlen

    with pytest.raises(NotImplementedError, match=text):
        flash_attention_ex(*_qkv(**kw))
    q, k, v = (t.transpose(0, 1) for t in _qkv(four_d=False, **kw))
    cu = torch.tensor([0, 16], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match=text):
        flash_attention_varlen(q, k, v, cu, cu, 16, 16)


def test_the_rules_come_in_the_librarys_order_and_equal_widths_pass():
    import flashattention_lab_cuda as ext

    assert ext.vdim_arg("t", 128, 128, torch.float32, sinks=True) == 0          # d_v == d: the call without the argument
    assert ext.vdim_arg("t", 192, 128, torch.bfloat16, sinks=False, mask=0) == 128
    assert ext.vdim_arg("t", 16, 8, torch.float16) == 8
    with pytest.raises(NotImplementedError, match="mask"):                       # the first carried argument, in the order given
        ext.vdim_arg("t", 192, 128, torch.bfloat16, mask=True, sinks=True)
    with pytest.raises(NotImplementedError, match="float16 or bfloat16"):        # the dtype before any feature
        ext.vdim_arg("t", 192, 128, torch.float32, mask=True)
    assert ext._ex_variant(True, True, True, True, True, vdim=128) == "_vdim" and ext._ex_variant(0, 0, 0) == ""


def test_the_wrappers_without_a_second_width_reach_their_old_checks():
    from common.attention_ex import flash_attention_ex

    q, k, v = _qkv(d=64, dv=64)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        flash_attention_ex(q, k, v, sinks=torch.zeros(2))
    with pytest.raises(RuntimeError, match="CUDA tensors"):    # a v of its own width that breaks no rule goes on to the device check
        flash_attention_ex(*_qkv())


# ---- the C ABI: the first broken rule, before any HIP call (there is no GPU here and the pointers are fake)
EX_ORDER = ("bh", "g", "nq", "nk", "d", "dtype", "causal", "wl", "wr", "scale", "softcap", "alibi", "aheads", "abs", "sinks", "sheads")
EX_BASE = dict(bh=4, g=1, nq=40, nk=50, d=192, dtype=2, causal=1, wl=-1, wr=-1, scale=192 ** -0.5, softcap=0.0, alibi=None, aheads=1,
               abs=0, sinks=None, sheads=1, dsinks=None, dlse=None, d_v=128, mask=None, mbs=0, bmask=None, br=0, bc=0, p=0.0, seed=0)
EX_TAIL = ("d_v", "mask", "mbs", "bmask", "br", "bc", "p", "seed")
VAR_ORDER = ("batch", "hq", "hkv", "tq", "tk", "mq", "mk", "d", "dtype", "sq", "sk", "sv", "causal", "wl", "wr", "scale", "softcap", "alibi",
             "abs", "sinks", "sheads")
VAR_BASE = dict(batch=2, hq=4, hkv=2, tq=60, tk=70, mq=40, mk=50, d=192, dtype=2, sq=4 * 192, sk=2 * 192, sv=2 * 128, causal=1, wl=-1,
                wr=-1, scale=192 ** -0.5, softcap=0.0, alibi=None, abs=0, sinks=None, sheads=1, dsinks=None, dlse=None, d_v=128, p=0.0,
                seed=0)


def _call(entry, **kw):
    import flashattention_lab_cuda as ext

    lib = ext._lib
    if entry in ("fa_ex_forward_vdim", "fa_ex_backward_vdim"):
        a = dict(EX_BASE, **kw)
        back = entry == "fa_ex_backward_vdim"
        args = [P] * (9 if back else 5) + [a[n] for n in EX_ORDER] + ([a["dsinks"], a["dlse"]] if back else []) + [a[n] for n in EX_TAIL]
    else:
        a = dict(VAR_BASE, **kw)
        back = entry == "fa_ex_backward_varlen_vdim"
        args = [P] * (9 if back else 5) + [P, P] + [a[n] for n in VAR_ORDER] + ([a["dsinks"], a["dlse"]] if back else []) + \
            [a["d_v"], a["p"], a["seed"]]
    args += [P, 1 << 30, None] if back else [None]
    rc = getattr(lib, entry)(*args)
    return rc, lib.fa_last_error().decode()


# (what the row breaks, the code, a piece of the text).  Rows with two breaches: a later rule's does not hide an earlier one.
BAD = [
    (dict(d_v=-8), INVALID_ARGUMENT, "d_v must be >= 0"),
    (dict(d=128, d_v=192), UNSUPPORTED, "d_v=192 > d=128"),
    (dict(d=128, d_v=136, dtype=0), UNSUPPORTED, "d_v=136 > d=128"),
    (dict(d_v=100), UNSUPPORTED, "multiples of 8 (got d=192, d_v=100)"),
    (dict(d=100, d_v=64), UNSUPPORTED, "multiples of 8 (got d=100, d_v=64)"),
    (dict(d=200, d_v=128), UNSUPPORTED, "d <= 192 (got d=200)"),
    (dict(d=256, d_v=192), UNSUPPORTED, "d <= 192 (got d=256)"),
    (dict(d_v=136), UNSUPPORTED, "d_v <= 128 (got d_v=136)"),
    (dict(dtype=0), UNSUPPORTED, "needs f16 or bf16 tensors (dtype code 0)"),
    (dict(dtype=0, sinks=P), UNSUPPORTED, "needs f16 or bf16 tensors"),
    (dict(p=0.25), UNSUPPORTED, "dropout_p > 0 is not supported with d_v != d"),
    (dict(wl=16), UNSUPPORTED, "window_size is not supported with d_v != d"),
    (dict(wr=0, softcap=20.0), UNSUPPORTED, "window_size is not supported with d_v != d"),
    (dict(softcap=20.0), UNSUPPORTED, "softcap is not supported with d_v != d"),
    (dict(alibi=P), UNSUPPORTED, "alibi_slopes is not supported with d_v != d"),
    (dict(sinks=P, dsinks=P), UNSUPPORTED, "sinks is not supported with d_v != d"),
    (dict(scale=0.0), UNSUPPORTED, "needs softmax_scale > 0"),
    (dict(scale=-1.0, sinks=P), UNSUPPORTED, "sinks is not supported"),
]
BAD_PADDED = [
    (dict(mask=P), UNSUPPORTED, "mask is not supported with d_v != d"),
    (dict(bmask=P, br=32, bc=32), UNSUPPORTED, "block_sparse_mask is not supported with d_v != d"),
    (dict(mask=P, p=0.5, softcap=1.0), UNSUPPORTED, "mask is not supported"),
]


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("kw,code,text", BAD)
def test_first_broken_rule_of_every_impl(entry, kw, code, text):
    rc, err = _call(entry, **kw)
    assert rc == code and text in err and err.startswith(entry + ":"), err


@pytest.mark.parametrize("entry", NAMES[:2])
@pytest.mark.parametrize("kw,code,text", BAD_PADDED)
def test_first_broken_rule_of_the_padded_impls(entry, kw, code, text):
    rc, err = _call(entry, **kw)
    assert rc == code and text in err and err.startswith(entry + ":"), err


@pytest.mark.parametrize("entry", NAMES[2:])
def test_layout_rules_of_the_packed_impls(entry):
    """(every row here is refused by validation: a call whose fake pointers passed it would be launched where there is a device)"""
    rc, err = _call(entry, sv=2 * 128 + 4)
    assert rc == UNSUPPORTED and "token strides that are multiples of 8" in err
    rc, err = _call(entry, sv=2 * 128 - 8)        # v's rows are heads_kv * d_v wide
    assert rc == INVALID_ARGUMENT and "token strides" in err


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("d_v", [0, 64])
def test_no_second_width_is_the_call_without_the_argument(entry, d_v):
    """d_v = 0 and d_v = d never meet the new rules: features the two-width kernels lack pass the checks (f32 tensors with a
    window and dropout here), and the old checks answer as they did."""
    kw = dict(d=64, d_v=d_v, dtype=0, wl=8, p=0.5, sq=4 * 64, sk=2 * 64, sv=2 * 64, scale=64 ** -0.5)
    rc, err = _call(entry, **kw, bh=-1, batch=0)
    assert rc == INVALID_ARGUMENT and "d_v" not in err.split(":", 1)[1]
    rc, err = _call(entry, **dict(kw, p=1.5))
    assert rc == INVALID_ARGUMENT and "dropout_p must lie in [0, 1)" in err


# ---- the fp64 reference against a direct computation
def test_reference_matches_a_direct_softmax_and_finite_differences():
    gen = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(s, generator=gen).to(torch.bfloat16) for s in ((4, 5, 16), (2, 7, 16), (2, 7, 8), (4, 5, 8)))
    o, lse, (dq, dk, dv) = vdim_reference(q, k, v, True, 0.25, do)
    qd, kd, vd = q.double(), k.double().repeat_interleave(2, 0), v.double().repeat_interleave(2, 0)
    s = 0.25 * qd @ kd.transpose(1, 2)
    s = s.masked_fill(torch.arange(7).view(1, -1) > torch.arange(5).view(-1, 1) + 2, float("-inf"))
    assert torch.allclose(o, torch.softmax(s, -1) @ vd, atol=1e-12) and torch.allclose(lse, torch.logsumexp(s, -1), atol=1e-12)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    # dv = P^T dO summed over the group
    want_dv = (torch.softmax(s, -1).transpose(1, 2) @ do.double()).view(2, 2, 7, 8).sum(1)
    assert torch.allclose(dv, want_dv, atol=1e-12)
    # rows without a visible key: o = 0, lse = -inf, no gradient (Nq > Nk under the causal mask)
    o2, lse2, (dq2, _dk2, _dv2) = vdim_reference(q, k[:, :3], v[:, :3], True, 0.25, do, torch.ones(4, 5))
    assert not bool(o2[:, :2].any()) and bool(torch.isneginf(lse2[:, :2]).all()) and not bool(dq2[:, :2].any())
    assert bool(torch.isfinite(lse2[:, 2:]).all()) and bool(torch.isfinite(dq2).all())
