"""CPU: a second query operand and K, V of different widths in KV-cache decoding (include/fa_mi355x.h: fa_ex_forward_kvcache_qv,
fa_ex_kvcache_workspace_bytes_qv; FlashAttention-3's qv, multi-head latent attention at decode time) — declared, exported, the
signature rows, the group absent equal to fa_ex_forward_kvcache_varlen, every unsupported combination and width rejected before
any HIP call with its name, the workspace formula and the launch rule, the Python wrappers' checks, and the fp64 reference
(tests/mla_ref.py) against tests/kvcache_full_ref.dense_attention on the concatenated operands."""
import ctypes
import inspect
import itertools
import os
import re

import pytest
import torch

from tests import mla_ref
from tests.kvcache_full_ref import dense_attention
from tests.test_abi_signatures_cpu import PROTOTYPES
from tests.test_kvcache_cpu import BAD, BASE
from tests.test_kvcache_paged_cpu import NONE as PNONE
from tests.test_kvcache_paged_cpu import PAGED
from tests.test_kvcache_rotary_cpu import NONE as RNONE
from tests.test_kvcache_varlen_cpu import SNONE, VARLEN_BAD, VNONE, VORDER, VQ

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_ex_forward_kvcache_qv", "fa_ex_kvcache_workspace_bytes_qv")
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

QV_PARAMS = PROTOTYPES["fa_ex_forward_kvcache_qv"][2]   # the header's parameter names of the new entry point
# the varlen entry point's arguments, then the four this one adds before the workspace
QORDER = VORDER[:VORDER.index("ws")] + ("qv", "qvb", "qvt", "dv", "ws", "wsb")
QNONE = dict(qv=None, qvb=0, qvt=0, dv=0)
# an MLA call on BASE's shapes (B = 2, H_q = 8, H_kv = 2, Nq = 1, cache_len = 64, bf16): q, k_cache 64 wide, v_cache, qv 512 wide, nothing to append
MLA = dict(qv=P, qvb=8 * 512, qvt=8 * 512, dv=512, vct=2 * 512, vcb=64 * 2 * 512, nnew=0, kn=None, vn=None, knb=0, knt=0, vnb=0, vnt=0)


def _call(name="fa_ex_forward_kvcache_qv", **kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **PNONE, **RNONE, **SNONE, **VNONE, **QNONE)
    a.update(kw)
    order = QORDER if name.endswith("_qv") else VORDER
    rc = getattr(ext._lib, name)(*[a[n] for n in order], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


def test_signature_rows_are_the_varlen_ones_plus_the_group():
    import flashattention_lab_cuda as ext

    group = ["qv", "qv_batch_stride", "qv_token_stride", "d_v"]
    varlen, qv = PROTOTYPES["fa_ex_forward_kvcache_varlen"][2], QV_PARAMS
    at = varlen.index("workspace")
    assert qv == varlen[:at] + group + varlen[at:] and len(qv) == 67 == len(QORDER) + 1   # (QORDER: all but the stream)
    assert PROTOTYPES["fa_ex_forward_kvcache_qv"][1][at:at + 4] == [ctypes.c_void_p] + [ctypes.c_int64] * 3
    assert [f for f, _t in ext._SIGNATURES["fa_ex_forward_kvcache_qv"][1]] == qv
    assert PROTOTYPES["fa_ex_kvcache_workspace_bytes_qv"][2] == PROTOTYPES["fa_ex_kvcache_workspace_bytes_varlen"][2] + ["d_v"]
    assert [f for f, _t in ext._SIGNATURES["fa_ex_kvcache_workspace_bytes_qv"][1]] == PROTOTYPES["fa_ex_kvcache_workspace_bytes_qv"][2]
    # the widest entry point of the family: every narrower one is handed its own arguments of these
    assert ext._CALLS["fa_ex_forward_kvcache_varlen"][2] == ext._CALLS["fa_ex_forward_kvcache_qv"][2] == 67


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_group_absent_answers_as_the_varlen_entry_point(kw, what):
    rc, msg = _call(**kw)
    rc0, msg0 = _call("fa_ex_forward_kvcache_varlen", **kw)
    assert rc == rc0 == INVALID_ARGUMENT and what in msg
    assert msg == msg0.replace("fa_ex_forward_kvcache_varlen:", "fa_ex_forward_kvcache_qv:")


@pytest.mark.parametrize("kw,code,what", VARLEN_BAD, ids=[str(i) for i in range(len(VARLEN_BAD))])
def test_group_absent_rejects_what_the_varlen_entry_point_rejects(kw, code, what):
    rc, msg = _call(**kw)
    rc0, msg0 = _call("fa_ex_forward_kvcache_varlen", **kw)
    assert rc == rc0 == code and what in msg
    assert msg == msg0.replace("fa_ex_forward_kvcache_varlen:", "fa_ex_forward_kvcache_qv:")


def test_group_absent_reaches_the_null_pointer_check_and_the_empty_call():
    for kw in (dict(o=None), dict(VQ, kc=None), dict(VQ, **PAGED, kc=None)):
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
    rc, msg = _call(**dict(VQ, mq=0), nnew=0, kn=None, vn=None, seqlens=None, knb=0, knt=0, vnb=0, vnt=0)   # nothing to launch
    assert rc == OK, msg
    for kw in (dict(qvb=8), dict(qvt=8), dict(dv=512), dict(dv=-1)):   # the group's integers without qv
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and "must be 0 without qv" in msg, (kw, msg)


QV_BAD = [
    # widths: only head_dim = 64 with d_v = 512; the text names both numbers
    (dict(MLA, dv=256, vct=2 * 256, vcb=64 * 2 * 256, qvb=8 * 256, qvt=8 * 256), UNSUPPORTED, "head_dim = 64, d_v = 256"),
    (dict(MLA, dv=64, vct=128, vcb=64 * 128, qvb=512, qvt=512), UNSUPPORTED, "head_dim = 64, d_v = 64"),
    (dict(MLA, d=128, qb=1024, qt=1024, kcb=64 * 256, kct=256), UNSUPPORTED, "head_dim = 128, d_v = 512"),
    (dict(MLA, dv=0), UNSUPPORTED, "head_dim = 64, d_v = 0"),
    (dict(MLA, dv=-512), UNSUPPORTED, "d_v = -512"),
    # what qv does not go with, each by its name
    (dict(MLA, nnew=1, kn=P, vn=P, knb=128, knt=128, vnb=128, vnt=128), UNSUPPORTED, "qv cannot be combined with k_new / v_new"),
    (dict(MLA, kn=P, vn=P), UNSUPPORTED, "qv cannot be combined with k_new / v_new"),
    (dict(MLA, cuq=P, tq=2, mq=1, nq=0, qb=0, cukn=P, tkn=0, kn=P, vn=P, knt=128, vnt=128), UNSUPPORTED, "qv cannot be combined with k_new / v_new"),
    (dict(MLA, cdt=3, kd=P, vd=P), UNSUPPORTED, "qv cannot be combined with an e4m3 cache (cache_dtype, k_descale, v_descale)"),
    (dict(MLA, cdt=3), UNSUPPORTED, "qv cannot be combined with an e4m3 cache"),
    (dict(MLA, softcap=30.0), UNSUPPORTED, "qv cannot be combined with softcap"),
    (dict(MLA, alibi=P), UNSUPPORTED, "qv cannot be combined with alibi_slopes"),
    (dict(MLA, sinks=P, sheads=8, splits=2, ws=P, wsb=2 ** 40), UNSUPPORTED, "qv cannot be combined with sinks"),
    (dict(MLA, cuq=P, tq=2, mq=1, nq=0, qb=0), UNSUPPORTED, "qv cannot be combined with cu_seqlens_q"),
    (dict(MLA, leftpad=P), UNSUPPORTED, "qv cannot be combined with cache_leftpad"),
    # v_cache is d_v wide under qv: its strides are checked at that width (an existing check, at its place)
    (dict(MLA, vct=2 * 64), INVALID_ARGUMENT, "strides of v_cache"),
    (dict(MLA, vcb=63 * 2 * 512), INVALID_ARGUMENT, "strides of v_cache"),
    # qv's own layout
    (dict(MLA, qvt=8 * 512 - 8), INVALID_ARGUMENT, "strides of qv too small"),
    (dict(MLA, qvb=8 * 512 - 8), INVALID_ARGUMENT, "strides of qv too small"),
    (dict(MLA, qvt=8 * 512 + 4), INVALID_ARGUMENT, "strides of qv must be multiples of 8"),
    (dict(MLA, nq=2 ** 10 + 1, qt=512, qb=2 ** 20, qvt=2 ** 20, qvb=2 ** 31), UNSUPPORTED, "one batch element of qv spans"),
    (dict(MLA, qv=ctypes.c_void_p(4096 + 8)), INVALID_ARGUMENT, "16-byte aligned"),
    # the workspace of a split call holds d_v-wide partials
    (dict(MLA, splits=4, ws=P, wsb=0), INVALID_ARGUMENT, "workspace"),
]
# the rotary tables need new tokens, which qv does not take: the existing check answers first, by its own text
QV_BAD.append((dict(MLA, rcos=P, rsin=P, rcs=32, rss=32, sro=65, rdim=64), INVALID_ARGUMENT, "rotary needs seqlen_new > 0"))


@pytest.mark.parametrize("kw,code,what", QV_BAD, ids=[str(i) for i in range(len(QV_BAD))])
def test_qv_arguments_are_rejected_before_any_hip_call(kw, code, what):
    rc, msg = _call(**kw)   # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_ex_forward_kvcache_qv:"), (kw, msg)


def _ws_model(rows, dv, s):
    if s <= 1:
        return 0
    r256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    return r256(rows * s * dv * 4) + r256(rows * s * 4)


def test_workspace_of_a_split_call_is_sized_at_d_v():
    need = _ws_model(2 * 8 * 1, 512, 4)
    rc, msg = _call(**dict(MLA, splits=4, ws=P, wsb=need - 1))
    assert rc == INVALID_ARGUMENT and "workspace" in msg and str(need) in msg
    rc, msg = _call(**dict(MLA, splits=4, ws=P, wsb=need), kc=None)      # enough: on to the null pointer check
    assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, msg


def test_valid_qv_arguments_reach_the_null_pointer_check():
    for kw in (MLA, dict(MLA, causal=1), dict(MLA, wl=5, wr=0), dict(MLA, seqlens=None), dict(MLA, splits=0, ws=P, wsb=2 ** 40),
               {**MLA, **PAGED, "vcb": 16 * 2 * 512}, dict(MLA, hkv=1, hq=16, qb=1024, qt=1024, kct=64, kcb=64 * 64, vct=512, vcb=64 * 512, qvb=16 * 512, qvt=16 * 512),
               # the two caches as the column ranges of one (B, cap, 1, 576) allocation; a token-strided qv
               dict(MLA, hkv=1, kct=576, kcb=64 * 576, vct=576, vcb=64 * 576, qvt=3 * 8 * 512, qvb=3 * 8 * 512)):
        rc, msg = _call(**kw, kc=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
        rc, msg = _call(**kw, q=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)


def _mla_splits_model(b, hkv, rows, cap):
    """csrc/fa_mla.hip: mla_waves and mla_num_splits"""
    nw = 1 if rows <= 16 else 2 if rows <= 32 else 4
    units = b * hkv * -(-rows // (16 * nw))
    s = -(-256 * (4 // nw) // units)
    return max(1, min(s, -(-cap // 128), 256))


def test_workspace_bytes_formula_and_launch_rule():
    import flashattention_lab_cuda as ext

    f, varlen = ext._lib.fa_ex_kvcache_workspace_bytes_qv, ext._lib.fa_ex_kvcache_workspace_bytes_varlen
    for b, hq, hkv, nq, cap, s in itertools.product((1, 32), (16, 128), (1, 2), (1, 3), (100, 8192), (1, 2, 7, 256)):
        assert f(b, hq, hkv, b * nq, nq, cap, 64, s, 0, 512) == _ws_model(b * hq * nq, 512, s)
        assert f(b, hq, hkv, b * nq, nq, cap, 64, s, 1, 0) == varlen(b, hq, hkv, b * nq, nq, cap, 64, s, 1)   # d_v = 0: that query
        assert f(b, hq, hkv, b * nq, nq, cap, 64, s, 0, 0) == varlen(b, hq, hkv, b * nq, nq, cap, 64, s, 0)
    # num_splits = 0: the rule of the workgroups this kernel launches (rows per workgroup differ from the plain kernel's)
    for b, hq, hkv, nq, cap in ((32, 128, 1, 1, 8192), (32, 16, 1, 1, 8192), (4, 128, 1, 2, 32768), (3, 40, 1, 2, 304), (1, 16, 1, 1, 100),
                                (2, 8, 2, 2, 4096), (1, 1, 1, 1, 2 ** 20)):
        s = _mla_splits_model(b, hkv, (hq // hkv) * nq, cap)
        assert f(b, hq, hkv, b * nq, nq, cap, 64, 0, 0, 512) == _ws_model(b * hq * nq, 512, s), (b, hq, hkv, nq, cap, s)
    assert _mla_splits_model(32, 1, 16, 8192) == 32 and _mla_splits_model(32, 1, 128, 8192) == 4 and _mla_splits_model(1, 1, 16, 100) == 1
    for bad in ((0, 8, 8, 5, 1, 100, 64, 2, 0, 512), (1, 8, 3, 5, 1, 100, 64, 2, 0, 512), (1, 8, 8, 5, 1, 100, 64, 300, 0, 512),
                (1, 8, 8, 5, 6, 100, 64, 2, 0, 512), (1, 8, 8, 5, 1, 100, 64, 2, 0, -512)):
        assert f(*bad) == 0, bad


class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16).as_subclass(FakeCuda)


def test_python_wrappers_raise_not_implemented_with_the_name():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    q, qv, kc, vc = _fake(2, 1, 8, 64), _fake(2, 1, 8, 512), _fake(2, 32, 1, 64), _fake(2, 32, 1, 512)
    i32 = torch.zeros((2,), dtype=torch.int32)
    f32 = torch.ones((8,), dtype=torch.float32)
    tab = _fake(64, 16)
    new = dict(flash=dict(k=_fake(2, 1, 1, 64), v=_fake(2, 1, 1, 512)), ex=dict(k_new=_fake(2, 1, 1, 64), v_new=_fake(2, 1, 1, 512)))
    for fn, which, win in ((flash_attn_with_kvcache, "flash", "window_size"), (ext.ex_kvcache_forward, "ex", "window")):
        cases = [(new[which], r"k / v \(new tokens"), (dict(cu_seqlens_k_new=torch.zeros((3,), dtype=torch.int32)), "cu_seqlens_k_new"),
                 (dict(rotary_cos=tab, rotary_sin=tab), "rotary_cos / rotary_sin"), (dict(k_descale=f32[:1]), "k_descale / v_descale"),
                 (dict(v_descale=f32[:1]), "k_descale / v_descale"), (dict(softcap=20.0), "softcap"), (dict(alibi_slopes=f32), "alibi_slopes"),
                 (dict(sinks=f32), "sinks"), (dict(cu_seqlens_q=torch.zeros((3,), dtype=torch.int32), max_seqlen_q=1), "cu_seqlens_q"),
                 (dict(cache_leftpad=i32), "cache_leftpad")]
        for kw, name in cases:
            with pytest.raises(NotImplementedError, match="qv cannot be combined with " + name):
                fn(q, kc, vc, qv=qv, **kw)
        # widths other than 64 + 512, with both numbers; an e4m3 cache
        with pytest.raises(NotImplementedError, match=r"head dim 64 with v_cache of head dim 512 only \(got 64, 256\)"):
            fn(q, kc, _fake(2, 32, 1, 256), qv=_fake(2, 1, 8, 256))
        with pytest.raises(NotImplementedError, match=r"\(got 128, 512\)"):
            fn(_fake(2, 1, 8, 128), _fake(2, 32, 1, 128), vc, qv=qv)
        e4 = torch.zeros((2, 32, 1, 64), dtype=torch.float8_e4m3fn).as_subclass(FakeCuda)
        with pytest.raises(NotImplementedError, match="qv cannot be combined with an e4m3 cache"):
            fn(q, e4, torch.zeros((2, 32, 1, 512), dtype=torch.float8_e4m3fn).as_subclass(FakeCuda), qv=qv)
        # shapes: qv is (B, Nq, H_q, 512) in q's dtype; v_cache has the cache's units and tokens
        with pytest.raises(RuntimeError, match=r"qv must be a \(B, Nq, H_q, 512\)"):
            fn(q, kc, vc, qv=_fake(2, 1, 4, 512))
        with pytest.raises(RuntimeError, match="qv must be a"):
            fn(q, kc, vc, qv=torch.zeros((2, 1, 8, 512), dtype=torch.float16).as_subclass(FakeCuda))
        with pytest.raises(RuntimeError, match="k_cache and v_cache must be"):
            fn(q, kc, _fake(2, 16, 1, 512), qv=qv)
        with pytest.raises(RuntimeError, match="k_cache and v_cache must be"):   # without qv the two widths still have to agree
            fn(q, kc, vc)
        # a cache view that would need a copy: the two slices of a (.., H_kv = 2, 576) pool have their heads 576 apart
        pool = _fake(2, 32, 2, 576)
        with pytest.raises(ValueError, match="never copied"):
            fn(q, pool[..., 512:], pool[..., :512], qv=qv)
        params = inspect.signature(fn).parameters
        assert params["qv"].kind is inspect.Parameter.KEYWORD_ONLY and params["qv"].default is None
        positional = [p.name for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert "qv" not in positional
    with pytest.raises(NotImplementedError, match="qv of type list"):
        flash_attn_with_kvcache(q, kc, vc, qv=[1.0])


def test_default_scale_is_q_width_plus_qv_width(monkeypatch):
    """softmax_scale=None is (64 + 512) ** -0.5 with qv (FlashAttention-3's rule) and d ** -0.5 without: what the wrapper hands the
    library, caught at its call into it (there is no GPU here)."""
    import contextlib

    import flashattention_lab_cuda as ext

    seen = []
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ext, "_stream_ptr", lambda dev: 0)
    monkeypatch.setattr(ext, "_call", lambda name, values: seen.append((name, values)))
    q, qv, kc, vc = _fake(2, 1, 8, 64), _fake(2, 1, 8, 512), _fake(2, 32, 1, 64), _fake(2, 32, 1, 512)
    fields = [f for f, _t in ext._SIGNATURES["fa_ex_forward_kvcache_qv"][1]]
    o, lse = ext.ex_kvcache_forward(q, kc, vc, qv=qv, num_splits=1)
    name, values = seen[-1]
    got = dict(zip(fields, values))
    assert name == "fa_ex_forward_kvcache_qv" and len(values) == len(fields)
    assert got["softmax_scale"] == (64 + 512) ** -0.5
    assert (got["d"], got["d_v"], got["qv_token_stride"], got["v_cache_token_stride"], got["k_cache_token_stride"]) == (64, 512, 8 * 512, 512, 64)
    assert got["qv"] == qv.data_ptr() and o.shape == (2, 1, 8, 512) and lse.shape == (2, 8, 1)
    ext.ex_kvcache_forward(q, kc, vc, qv=qv, num_splits=1, softmax_scale=0.25)
    assert dict(zip(fields, seen[-1][1]))["softmax_scale"] == 0.25
    # the two slices of one (B, cap, 1, 576) pool: each view's own strides and address, no copy
    pool = _fake(2, 32, 1, 576)
    ext.ex_kvcache_forward(q, pool[..., 512:], pool[..., :512], qv=qv, num_splits=1)
    got = dict(zip(fields, seen[-1][1]))
    assert (got["k_cache"], got["v_cache"]) == (pool.data_ptr() + 1024, pool.data_ptr())
    assert (got["k_cache_token_stride"], got["v_cache_token_stride"], got["k_cache_batch_stride"], got["v_cache_batch_stride"]) == \
        (576, 576, 32 * 576, 32 * 576)
    # without qv: the narrowest entry point, d ** -0.5, and nothing of the group
    ext.ex_kvcache_forward(q, kc, kc, num_splits=1)
    name, values = seen[-1]
    got = dict(zip(fields, values))
    assert name == "fa_ex_forward_kvcache" and got["softmax_scale"] == 64 ** -0.5 and (got["qv"], got["d_v"]) == (0, 0)


@pytest.mark.parametrize("causal,window", [(False, (-1, -1)), (True, (-1, -1)), (False, (5, 0)), (False, (-1, 2)), (False, (2, 1))])
def test_reference_is_dense_attention_on_the_concatenated_operands(causal, window):
    g = torch.Generator().manual_seed(11)
    hq, hkv, nq, d, dv = 6, 2, 3, 64, 512
    scale = (d + dv) ** -0.5
    for lk in (1, 3, 33, 70):
        q, qv = torch.randn((nq, hq, d), generator=g).double(), torch.randn((nq, hq, dv), generator=g).double()
        k, v = torch.randn((lk, hkv, d), generator=g).double(), torch.randn((lk, hkv, dv), generator=g).double()
        o, lse = mla_ref.mla_attention(q, qv, k, v, causal, window, scale)
        # dense_attention returns (.., d of its q) columns of p @ v: pad v to the operands' width and cut
        vpad = torch.cat([torch.zeros((lk, hkv, d), dtype=torch.float64), v], -1)
        ro, rlse, novis = dense_attention(torch.cat([q, qv], -1), torch.cat([k, v], -1), vpad, causal, window, scale)
        torch.testing.assert_close(o, ro[..., d:], rtol=1e-12, atol=1e-12)
        fin = torch.isfinite(rlse)
        assert torch.equal(torch.isfinite(lse), fin) and torch.equal(~fin[0], novis)
        torch.testing.assert_close(lse[fin], rlse[fin], rtol=1e-12, atol=1e-12)
        assert (o[novis] == 0).all()


def test_reference_gathers_pages_rows_and_lengths():
    g = torch.Generator().manual_seed(5)
    b, hq, nq, ps, nblk = 3, 2, 2, 16, 7
    q, qv = torch.randn((b, nq, hq, 64), generator=g), torch.randn((b, nq, hq, 512), generator=g)
    kp, vp = torch.randn((nblk, ps, 1, 64), generator=g), torch.randn((nblk, ps, 1, 512), generator=g)
    table = torch.tensor([[3, 1, 6], [0, 99, 2], [5, 5, -1]], dtype=torch.int32)
    lens = torch.tensor([40, 33, 0], dtype=torch.int32)
    o, lse = mla_ref.mla_reference(q, qv, kp, vp, lens, True, (-1, -1), None, table)
    assert (o[2] == 0).all() and (lse[2] == -float("inf")).all()
    for s in range(2):
        kt = torch.cat([kp[p] if 0 <= p < nblk else torch.zeros_like(kp[0]) for p in table[s].tolist()])[:int(lens[s])]
        vt = torch.cat([vp[p] if 0 <= p < nblk else torch.zeros_like(vp[0]) for p in table[s].tolist()])[:int(lens[s])]
        ro, rlse = mla_ref.mla_attention(q[s].double(), qv[s].double(), kt.double(), vt.double(), True, (-1, -1), 576 ** -0.5)
        assert torch.equal(o[s], ro) and torch.equal(lse[s], rlse)
    # contiguous rows through cache_batch_idx: an index outside the cache reads zero keys with zero values
    kc, vc = torch.randn((2, 48, 1, 64), generator=g), torch.randn((2, 48, 1, 512), generator=g)
    o, lse = mla_ref.mla_reference(q, qv, kc, vc, 20, False, (-1, -1), 0.1, None, torch.tensor([1, 7, 0], dtype=torch.int32))
    ro, rlse = mla_ref.mla_attention(q[0].double(), qv[0].double(), kc[1, :20].double(), vc[1, :20].double(), False, (-1, -1), 0.1)
    assert torch.equal(o[0], ro) and torch.equal(lse[0], rlse)
    assert (o[1] == 0).all() and torch.allclose(lse[1], torch.full_like(lse[1], torch.log(torch.tensor(20.0)).item()))
    assert mla_ref.lengths(None, 2, 48) == [48, 48] and mla_ref.lengths(torch.tensor([-3, 99]), 2, 48) == [0, 48]
