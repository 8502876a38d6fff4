"""CPU: the fp8 quantiser (include/fa_mi355x.h: fa_fp8_quantize; flashattention_lab_cuda.fp8_quantize; common.attention_ex:
quantize_fp8, quantize_fp8_qkv) — declared and exported, every host-side rule reached in the header's order through raw ctypes
with fake pointers (there is no GPU here), the workspace formula, the wrappers' refusals by name, and the properties of the CPU
model (tests/fp8_quantize_ref.py) that can be derived from the number formats."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.fp8_quantize_ref import (VALUES, descale_of, make_x, odd_mantissa, pow2_up, quantize_model, rotate32, span, static_descales,
                                    tables, unit_amax)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = ctypes.c_void_p(4096)     # non-null, 16-byte aligned, never dereferenced: validation fails first, or nothing is launched
Q = ctypes.c_void_p(8192)

ORDER = ("x", "out", "ds", "dso", "cu", "rcos", "rsin", "rcs", "rss", "sro", "rdim", "rint", "off", "offs", "batch", "heads", "seqlen",
         "d", "g", "total", "maxs", "dtype", "xb", "xh", "xt", "ob", "oh", "ot", "dsb", "pow2", "ws", "wsb")
# a valid static call without tokens and without descale_out: (2, 0, 4, 64) bf16 "bnhd", g = 2.  It passes every rule and launches
# nothing, so each BAD entry breaks exactly one rule of an otherwise valid call.
BASE = dict(x=P, out=Q, ds=P, dso=None, cu=None, rcos=None, rsin=None, rcs=0, rss=0, sro=0, rdim=0, rint=0, off=0, offs=None, batch=2,
            heads=4, seqlen=0, d=64, g=2, total=0, maxs=0, dtype=2, xb=5 * 256, xh=64, xt=256, ob=5 * 256, oh=64, ot=256, dsb=2, pow2=0,
            ws=None, wsb=0)
TOKENS = dict(seqlen=5)       # a call that would launch: only for rules that fail before that
ROT = dict(rcos=P, rsin=P, rcs=16, rss=16, sro=8, rdim=32)
PACKED = dict(cu=P, total=9, maxs=0, xb=0, ob=0)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE)
    a.update(kw)
    rc = ext._lib.fa_fp8_quantize(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in ("fa_fp8_quantize", "fa_fp8_quantize_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src)
        assert hasattr(lib, name)
        assert name in ext.EXPORTED_C_SYMBOLS and name in ext._SIGNATURES
    fields = [f for f, _ in ext._SIGNATURES["fa_fp8_quantize"][1]]
    assert len(fields) == len(ORDER) + 1 and fields[-1] == "stream"
    assert fields[5:12] == [f for f, _ in ext._ROTARY]          # the rotary group, verbatim
    assert ext._CALLS["fa_fp8_quantize"][2] == len(fields)
    assert ext._lib.fa_fp8_quantize_workspace_bytes.restype is ctypes.c_size_t
    for route in ("fp8_quant_fused", "fp8_quant_two_pass", "fp8_quant_static"):
        assert ext.route_count(route) >= 0                       # the library knows the names


def test_the_base_call_is_valid_and_launches_nothing():
    assert _call() == (0, _call()[1])
    assert _call(**PACKED)[0] == 0
    assert _call(**ROT)[0] == 0
    assert _call(batch=1, xb=3, ob=-7)[0] == 0                   # batch 1 and the packed form do not look at the batch strides
    assert _call(**dict(PACKED, xb=3, ob=-7))[0] == 0
    assert _call(dsb=0)[0] == 0                                  # one (heads / g,) row for every batch element


BAD = [
    (dict(dtype=0), "dtype"), (dict(dtype=3), "dtype"),
    (dict(d=0), "head_dim"), (dict(d=8), "head_dim"), (dict(d=72), "head_dim"), (dict(d=272), "head_dim"),
    (dict(batch=0), "batch must be >= 1"),
    (dict(heads=0), "heads must be >= 1"), (dict(heads=2 ** 31), "heads must be >= 1"),
    (dict(g=0), "heads_per_scale"), (dict(g=3), "heads_per_scale"), (dict(g=8), "heads_per_scale"),
    (dict(batch=2 ** 31, g=4), "must be < 2^31"),
    (dict(seqlen=-1), "seqlen must lie"), (dict(seqlen=2 ** 31), "seqlen must lie"),
    (dict(x=None), "null tensor pointer"), (dict(out=None), "null tensor pointer"),
    (dict(x=ctypes.c_void_p(4104)), "16-byte aligned"), (dict(out=ctypes.c_void_p(8200)), "16-byte aligned"),
    (dict(ds=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(dso=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(PACKED, cu=ctypes.c_void_p(4099)), "4-byte aligned"), (dict(offs=ctypes.c_void_p(4098)), "4-byte aligned"),
    (dict(ds=None), "needs descale_out"),
    (dict(PACKED, total=-1), "total must lie"), (dict(PACKED, total=2 ** 31), "total must lie"),
    (dict(PACKED, maxs=-1), "max_seqlen"), (dict(PACKED, maxs=10), "max_seqlen"),
    (dict(PACKED, seqlen=5), "seqlen must be 0"),
    (dict(total=9), "without cu_seqlens"), (dict(maxs=5), "without cu_seqlens"),
    (dict(TOKENS, xt=252), "strides of x"), (dict(TOKENS, xh=-64), "strides of x"), (dict(TOKENS, xb=1284), "strides of x"),
    (dict(TOKENS, xt=2 ** 57), "strides of x"),
    (dict(TOKENS, ot=264), "strides of out"), (dict(TOKENS, oh=-64), "strides of out"), (dict(TOKENS, ob=1288), "strides of out"),
    (dict(TOKENS, ob=2 ** 59), "strides of out"),
    (dict(TOKENS, oh=48), "rows of out overlap"), (dict(TOKENS, ot=128), "rows of out overlap"),
    (dict(TOKENS, oh=128, ot=64), "rows of out overlap"),         # tokens inside heads: the head stride must span the 5 tokens
    (dict(TOKENS, ob=4 * 256 + 192), "batch stride"),
    (dict(dsb=1), "descale_batch_stride"), (dict(dsb=-2), "descale_batch_stride"), (dict(dsb=2 ** 41), "descale_batch_stride"),
    (dict(ROT, rcos=None), "both be given"), (dict(ROT, rsin=None), "both be given"),
    (dict(ROT, rcos=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(ROT, rsin=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(ROT, rdim=0), "rotary_dim"), (dict(ROT, rdim=8), "rotary_dim"), (dict(ROT, rdim=24), "rotary_dim"), (dict(ROT, rdim=80), "rotary_dim"),
    (dict(ROT, rcs=15), "row strides"), (dict(ROT, rss=8), "row strides"), (dict(ROT, rcs=2 ** 31 + 2), "row strides"),
    (dict(ROT, rcs=17), "even"), (dict(ROT, rss=19), "even"),
    (dict(ROT, sro=0), "seqlen_ro"), (dict(ROT, sro=2 ** 31), "seqlen_ro"),
    (dict(ROT, off=2 ** 31), "seqlen_offset"), (dict(ROT, off=-2 ** 31), "seqlen_offset"),
]


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_rule_is_checked_before_any_hip_call(kw, what):
    rc, msg = _call(**kw)    # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == INVALID_ARGUMENT, (kw, msg)
    assert what in msg and msg.startswith("fa_fp8_quantize:"), (kw, msg)


def test_unit_size_and_workspace_come_last():
    # a unit of 2^28 tokens x 2 heads x 8 chunks = 2^32 chunks
    rc, msg = _call(seqlen=2 ** 28, batch=1, xt=256, ot=256)
    assert rc == UNSUPPORTED and "beyond 2^31" in msg
    # dynamic, 129 tokens x 2 heads x 8 chunks = 2064 > 1024 items: the two-pass route, which needs its scratch
    big = dict(ds=None, dso=P, seqlen=129, xb=129 * 256, ob=129 * 256)
    rc, msg = _call(**big)
    assert rc == WORKSPACE and "workspace of 256 bytes needed, 0 given" in msg
    rc, msg = _call(**dict(big, ws=Q, wsb=255))
    assert rc == WORKSPACE and "256 bytes needed, 255 given" in msg
    rc, msg = _call(**dict(big, ws=ctypes.c_void_p(8200), wsb=256))
    assert rc == WORKSPACE and "16-byte aligned" in msg
    rc, msg = _call(**dict(big, ws=P, wsb=256))
    assert rc == WORKSPACE and "must not be descale_out" in msg
    # validation still comes first
    assert _call(**dict(big, d=72))[0] == INVALID_ARGUMENT


def test_the_first_broken_rule_names_itself():
    """two broken rules: the one that comes first in the header's list answers"""
    for kw, what in ((dict(dtype=0, d=72), "dtype"), (dict(d=72, batch=0), "head_dim"), (dict(batch=0, heads=0), "batch must be"),
                     (dict(heads=0, g=0), "heads must be"), (dict(g=3, seqlen=-1), "heads_per_scale"), (dict(seqlen=-1, x=None), "seqlen"),
                     (dict(x=None, ds=ctypes.c_void_p(4098)), "null tensor pointer"), (dict(out=ctypes.c_void_p(8200), ds=None), "16-byte"),
                     (dict(ds=None, total=9), "needs descale_out"), (dict(total=9, dsb=1), "without cu_seqlens"),
                     (dict(TOKENS, xt=252, ot=264), "strides of x"), (dict(TOKENS, ot=264, dsb=1), "strides of out"),
                     (dict(TOKENS, oh=48, dsb=1), "rows of out overlap"), (dict(ROT, dsb=1, rdim=8), "descale_batch_stride"),
                     (dict(ROT, rdim=8, sro=0), "rotary_dim"), (dict(ROT, sro=0, off=2 ** 31), "seqlen_ro")):
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and what in msg, (kw, msg)


def test_workspace_formula():
    import flashattention_lab_cuda as ext

    ws = ext._lib.fa_fp8_quantize_workspace_bytes
    assert ws(1, 1, 1) == 256 and ws(2, 8, 2) == 256 and ws(8, 8, 1) == 256 and ws(8, 9, 1) == 512       # 4 bytes a unit, up to 256
    assert ws(32, 32, 4) == 32 * 8 * 4 and ws(4096, 48, 1) == 4096 * 48 * 4
    for bad in ((0, 8, 1), (2, 0, 1), (2, 8, 0), (2, 8, 3), (-1, 8, 1), (2 ** 31, 8, 2)):
        assert ws(*bad) == 0


class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def test_shim_rejections():
    import flashattention_lab_cuda as ext

    x = _fake(2, 5, 4, 64)
    with pytest.raises(ValueError, match="layout must be one of"):
        ext.fp8_quantize(x, layout="hbnd")
    with pytest.raises(ValueError, match="out_layout"):
        ext.fp8_quantize(x, out_layout="thd")
    for bad in (_fake(2, 5, 4, 64, dtype=torch.float32), _fake(2, 5, 4, 64, dtype=torch.float8_e4m3fn), [1.0]):
        with pytest.raises(NotImplementedError, match="x of dtype"):
            ext.fp8_quantize(bad)
    for d in (8, 72, 264, 512):
        with pytest.raises(NotImplementedError, match=f"head_dim {d} is not supported"):
            ext.fp8_quantize(_fake(2, 5, 4, d))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.fp8_quantize(torch.zeros((2, 5, 4, 64), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="go together"):
        ext.fp8_quantize(x, cu_seqlens=torch.zeros(3, dtype=torch.int32), max_seqlen=5)
    with pytest.raises(ValueError, match="go together"):
        ext.fp8_quantize(_fake(9, 4, 64), layout="thd")
    with pytest.raises(ValueError, match="max_seqlen needs cu_seqlens"):
        ext.fp8_quantize(x, max_seqlen=5)
    with pytest.raises(ValueError, match="needs max_seqlen"):
        ext.fp8_quantize(_fake(9, 4, 64), layout="thd", cu_seqlens=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="cu_seqlens of dtype"):
        ext.fp8_quantize(_fake(9, 4, 64), layout="thd", cu_seqlens=torch.zeros(3, dtype=torch.int64), max_seqlen=5)
    with pytest.raises(ValueError, match=r"max_seqlen = 10 must lie in \[0, total = 9\]"):
        ext.fp8_quantize(_fake(9, 4, 64), layout="thd", cu_seqlens=torch.zeros(3, dtype=torch.int32), max_seqlen=10)
    with pytest.raises(RuntimeError, match="must be 4-D"):
        ext.fp8_quantize(_fake(5, 4, 64))
    with pytest.raises(RuntimeError, match="heads_per_scale = 3"):
        ext.fp8_quantize(x, heads_per_scale=3)
    with pytest.raises(NotImplementedError, match="descale of dtype"):
        ext.fp8_quantize(x, descale=torch.ones((2, 4), dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"descale must be float32 of shape"):
        ext.fp8_quantize(x, heads_per_scale=2, descale=torch.ones((2, 4)))
    with pytest.raises(RuntimeError, match="both be given"):
        ext.fp8_quantize(x, rotary_cos=_fake(8, 16))
    with pytest.raises(RuntimeError, match="multiple of 16 in"):
        ext.fp8_quantize(x, rotary_cos=_fake(8, 12), rotary_sin=_fake(8, 12))
    with pytest.raises(RuntimeError, match="seqlen_offsets must be an int"):
        ext.fp8_quantize(x, rotary_cos=_fake(8, 16), rotary_sin=_fake(8, 16), seqlen_offsets=torch.zeros(3, dtype=torch.int32))
    # views that would need a copy raise for x and are never copied
    last_strided = _fake(2, 5, 4, 128)[..., ::2]
    odd_stride = _fake(2, 5, 4, 68)[..., :64]
    misaligned = _fake(2 * 5 * 4 * 64 + 8)[4:-4].view(2, 5, 4, 64)
    for bad in (last_strided, odd_stride, misaligned):
        with pytest.raises(ValueError, match="never copied"):
            ext.fp8_quantize(bad)


def test_module_rejections():
    from common.attention_ex import quantize_fp8, quantize_fp8_qkv

    with pytest.raises(NotImplementedError, match="x of dtype"):
        quantize_fp8(_fake(2, 5, 4, 64, dtype=torch.float32))
    with pytest.raises(NotImplementedError, match="head_dim 72"):
        quantize_fp8(_fake(2, 5, 4, 72))
    with pytest.raises(ValueError, match="never copied"):
        quantize_fp8(_fake(2, 5, 4, 128)[..., ::2])
    q, k = _fake(2, 5, 6, 64), _fake(2, 5, 4, 64)
    with pytest.raises(RuntimeError, match="H_q = 6 must be a multiple of H_kv = 4"):
        quantize_fp8_qkv(q, k, k)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        quantize_fp8_qkv(q, None, k)


# ---- the model's derived properties
def _dequant(codes, descale, g):
    return codes.view(torch.float8_e4m3fn).double() * descale.double().repeat_interleave(g, dim=1)[:, None, :, None]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", VALUES)
@pytest.mark.parametrize("pow2", [False, True], ids=["plain", "pow2"])
def test_model_error_bound_and_top_element(dtype, kind, pow2):
    g = 2
    x = make_x(kind, (2, 37, 4, 64), g, dtype, seed=11)
    codes, ds = quantize_model(x, g, scale_pow2=pow2)
    amax = unit_amax(x, g)
    # the division is IEEE: numpy's float32 division gives the same bits
    want = np.where(amax.numpy() > 0, amax.numpy() / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    plain = descale_of(amax)
    assert np.array_equal(plain.numpy().view(np.uint32), want.view(np.uint32))
    if pow2:
        assert bool(((ds >= plain) & (ds < 2 * plain)).all())                    # rounded UP, by less than a factor of two
        assert bool(((ds.view(torch.int32) & 0x007FFFFF) == 0).all())
    deq = _dequant(codes, ds, g)
    xd = x.double()
    # half an e4m3 step (2^-4 relative; the (1 + 2^-20) covers the two fp32 roundings of inv and of the product) plus half the
    # subnormal step 2^-9 in units of the descale
    bound = 2.0 ** -4 * xd.abs() * (1 + 2.0 ** -20) + 2.0 ** -10 * ds.double().repeat_interleave(g, dim=1)[:, None, :, None]
    assert bool(((deq - xd).abs() <= bound).all())
    if not pow2:
        # the element that sets a unit's amax comes back as amax within 2^-23 relative: it quantises to +-448 exactly
        top = deq.abs().reshape(2, 37, 2, g * 64).amax(dim=(1, 3))
        live = amax > 0
        assert bool(((top - amax.double()).abs()[live] <= 2.0 ** -23 * amax.double()[live]).all())
    zero = amax == 0
    assert bool((ds[zero] == 1).all())
    u = codes.reshape(2, 37, 2, g * 64)
    for b in range(2):
        for j in range(2):
            if zero[b, j]:
                assert int(u[b, :, j].max()) == 0                                # an all-zero unit: descale 1, codes 0


def test_model_ties_round_to_even():
    x = make_x("ties", (1, 16, 2, 64), 1, torch.bfloat16, seed=3)
    codes, ds = quantize_model(x, 1)
    assert bool((ds == 1).all())
    f = x.float()
    back = codes.view(torch.float8_e4m3fn).float()
    step = torch.where(f.abs() < 2.0 ** -6, torch.full_like(f, 2.0 ** -9), torch.exp2(torch.floor(torch.log2(f.abs())) - 3))
    tie = (f.abs() / step) % 1 == 0.5
    assert int(tie.sum()) > 100
    assert bool(((back[tie].abs() / step[tie]) % 2 == 0).all())                  # every tie went to the even neighbour
    assert bool(((back - f).abs()[tie] == step[tie] / 2).all())


def test_model_static_mode_and_pow2_rule():
    x = make_x("normal", (2, 9, 4, 32), 2, torch.float16, seed=5)
    ds = static_descales((2, 2), seed=6)
    assert bool(((ds.view(torch.int32) & 1) == 1).all())
    codes, got = quantize_model(x, 2, descale=ds)
    assert torch.equal(got, ds)
    row, _ = quantize_model(x, 2, descale=ds[0])                               # the (H / g,) form: one row for every batch element
    assert torch.equal(row[0], codes[0])
    # a dynamic call's own descale, handed back statically, gives the dynamic codes
    dyn, dds = quantize_model(x, 2)
    assert torch.equal(quantize_model(x, 2, descale=dds)[0], dyn)
    p = pow2_up(torch.tensor([1.0, 1.5, 0.75, 2.0 ** -20, 3.0e-3, 448.0 / 448.0]))
    assert p.tolist() == [1.0, 2.0, 1.0, 2.0 ** -20, 2.0 ** -8, 1.0]
    assert odd_mantissa(torch.tensor([1.0])).item() == 1.0 + 2.0 ** -23


def test_model_rotation_is_the_fp64_rotation_rounded_once():
    """on these inputs the fp32 evaluation rounds exactly as the fp64 reference of the rotary tests does (tests/rotary_ref.py)"""
    from tests.rotary_ref import reference64, round_once

    for dtype in (torch.bfloat16, torch.float16):
        for inter in (False, True):
            g = torch.Generator().manual_seed(17)
            x = torch.randn((2, 9, 3, 64), generator=g).to(dtype)
            cos, sin = tables(12, 32, dtype)
            got = rotate32(x, cos, sin, [-2, 7], inter)
            exact, rotated = reference64(x, cos, sin, [-2, 7], inter, False)
            assert rotated.tolist()[0][:3] == [False, False, True] and rotated.tolist()[1][4:6] == [True, False]
            assert torch.equal(got[~rotated], x[~rotated]) and torch.equal(got[..., 32:], x[..., 32:])
            want = round_once(exact, dtype)
            differ = int((got.double() != want.double()).sum())
            assert differ * 10 ** 4 <= got.numel(), differ                     # double rounding through fp32: rotary_ref's own cap


def test_span_is_the_varlen_clamp():
    assert span([0, 3, 9], 1, 9, 5) == (3, 5)
    assert span([0, 9, 3], 1, 9, 9) == (9, 0)          # decreasing
    assert span([0, 50, 60], 0, 9, 9) == (0, 9)        # oversized
    assert span([-4, 2, 2], 0, 9, 9) == (0, 2)
