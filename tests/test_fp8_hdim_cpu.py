"""CPU: head dims 64 and 256 beside 128 on the fp8 calls (include/fa_mi355x.h: fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim,
fa_fp8_forward_kvcache_hdim and their three workspace functions; common/fp8_attention.py): the declarations, the host's
refusals in the parents' order with the head dim in their texts, the workspace sizes against the formulas of tests/fp8_hdim_ref.py,
the wrappers' refusals, and the proofs behind tests/test_fp8_hdim_gpu.py: the d-parameterised model is the pinned d = 128 model bit
for bit, and without rounding it is the fp64 definition at 64 and 256."""
import ctypes

import pytest
import torch

from tests import fp8_hdim_ref as hr
from tests import fp8_kvcache_mod_ref as km
from tests import fp8_kvcache_ref as fk
from tests import fp8_mod_ref as fm
from tests.fp8_ref import tiled_sharp_bar
from tests.test_abi_signatures_cpu import PROTOTYPES

E4 = torch.float8_e4m3fn
OK, INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails
ODD = ctypes.c_void_p(4104)
E4M3 = 3
CALLS = ("fa_fp8_forward_hdim", "fa_fp8_forward_varlen_hdim", "fa_fp8_forward_kvcache_hdim")
SIZES = ("fa_fp8_forward_hdim_workspace_bytes", "fa_fp8_forward_varlen_hdim_workspace_bytes", "fa_fp8_forward_kvcache_hdim_workspace_bytes")
TAIL = dict(window_left=-1, window_right=-1, softcap=0.0, sinks=None, sink_heads=0)

# padded: B = 2, H_q = 4, H_kv = 2, 300 x 300 tokens in the (B, N, H, 64) layout, (B, H_kv) descales, an ample workspace
PADDED = dict(q=P, k=P, v=P, o=P, lse=P, q_descale=P, k_descale=P, v_descale=P, batch=2, heads_q=4, heads_kv=2, seqlen_q=300, seqlen_k=300,
              head_dim=64, dtype=2, q_batch_stride=300 * 256, q_head_stride=64, q_token_stride=256, k_batch_stride=300 * 128,
              k_head_stride=64, k_token_stride=128, v_batch_stride=300 * 128, v_head_stride=64, v_token_stride=128,
              o_batch_stride=300 * 256, o_head_stride=64, o_token_stride=256, q_descale_batch_stride=2, k_descale_batch_stride=2,
              v_descale_batch_stride=2, causal=1, softmax_scale=0.125, workspace=P, workspace_bytes=2 ** 40, stream=None, **TAIL)
# packed: three sequences, 500 query and 700 key tokens
PACKED = dict(q=P, k=P, v=P, o=P, lse=P, q_descale=P, k_descale=P, v_descale=P, cu_seqlens_q=P, cu_seqlens_k=P, block_table=None, batch=3,
              heads_q=4, heads_kv=2, total_q=500, total_k=700, max_seqlen_q=300, max_seqlen_k=400, head_dim=64, dtype=2, q_token_stride=256,
              q_head_stride=64, k_token_stride=128, k_head_stride=64, v_token_stride=128, v_head_stride=64, max_blocks_per_seq=0,
              num_blocks=0, page_block_size=0, k_page_stride=0, v_page_stride=0, q_descale_batch_stride=2, k_descale_batch_stride=2,
              v_descale_batch_stride=2, causal=1, softmax_scale=0.125, workspace=P, workspace_bytes=2 ** 40, stream=None, **TAIL)
PAGED = dict(PACKED, block_table=P, total_k=0, max_blocks_per_seq=30, num_blocks=64, page_block_size=16, k_page_stride=16 * 128,
             v_page_stride=16 * 128)
# decode: B = 3, H_q = 8, H_kv = 2, two query tokens, caches of 1000 tokens, four splits
DECODE = dict(q=P, k_cache=P, v_cache=P, o=P, lse=P, q_descale=P, k_descale=P, v_descale=P, cache_seqlens=P, block_table=None,
              cache_batch_idx=None, batch=3, heads_q=8, heads_kv=2, seqlen_q=2, cache_len=1000, cache_batch=0, head_dim=64, dtype=2,
              q_dtype=E4M3, cache_dtype=E4M3, q_batch_stride=2048, q_token_stride=1024, k_batch_stride=256000, k_token_stride=256,
              v_batch_stride=256000, v_token_stride=256, block_table_row_stride=0, num_blocks=0, page_block_size=0,
              q_descale_batch_stride=2, k_descale_batch_stride=2, v_descale_batch_stride=2, causal=1, softmax_scale=0.125, num_splits=4,
              workspace=P, workspace_bytes=2 ** 40, stream=None, **TAIL)


def invoke(name, base, **kw):
    """(return code, message) of the C function on base's arguments by the header's parameter names"""
    import flashattention_lab_cuda as ext

    a = dict(base, **kw)
    names = PROTOTYPES[name][2]
    assert set(names) == set(a), set(names) ^ set(a)
    rc = getattr(ext._lib, name)(*[a[n] for n in names])
    return rc, ext._lib.fa_last_error().decode()


def test_the_entry_points_are_declared_exported_and_take_their_mod_parents_lists():
    import flashattention_lab_cuda as ext
    from common import attention_ex, fp8_attention

    for name in CALLS + SIZES:
        assert name in PROTOTYPES and name in ext.EXPORTED_C_SYMBOLS and hasattr(ext._lib, name)
    renamed = lambda names: ["head_dim" if n == "d" else n for n in names]   # noqa: E731
    for name in CALLS:
        parent = name.replace("_hdim", "_mod")
        assert PROTOTYPES[name][:2] == PROTOTYPES[parent][:2] and PROTOTYPES[name][2] == renamed(PROTOTYPES[parent][2])
        _fn, own, count = ext._CALLS[name]
        assert count == len(PROTOTYPES[name][2]) and list(own(tuple(PROTOTYPES[name][2]))) == PROTOTYPES[name][2]
    for name, parent in zip(SIZES, ("fa_fp8_forward_workspace_bytes", "fa_fp8_forward_varlen_workspace_bytes",
                                    "fa_fp8_forward_kvcache_workspace_bytes_mod")):
        assert PROTOTYPES[name][:2] == PROTOTYPES[parent][:2] and PROTOTYPES[name][2] == renamed(PROTOTYPES[parent][2])
    for fn in ("fp8_attn_func", "fp8_attn_varlen_func", "fp8_attn_with_kvcache"):
        assert getattr(attention_ex, fn) is getattr(fp8_attention, fn)             # exported where the older ones are
    for route in ("fp8in_fwd_hdim", "fp8in_fwd_varlen_hdim", "fp8kv_split_hdim"):
        assert ext.route_count(route) >= 0


# Every row breaks one rule and, where it can, a LATER one as well, which must not be the one reported; no row passes validation (a
# call that did would launch on the fake pointers).
REFUSALS = [
    ("fa_fp8_forward_hdim", PADDED, dict(q=None, head_dim=96), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_fp8_forward_hdim", PADDED, dict(batch=0, head_dim=96), INVALID_ARGUMENT, "must be > 0"),
    ("fa_fp8_forward_hdim", PADDED, dict(head_dim=96, heads_kv=3), UNSUPPORTED, "head_dim 96 is not supported (64, 128 or 256)"),
    ("fa_fp8_forward_hdim", PADDED, dict(head_dim=192, dtype=0), UNSUPPORTED, "head_dim 192 is not supported (64, 128 or 256)"),
    ("fa_fp8_forward_hdim", PADDED, dict(head_dim=32, dtype=0), UNSUPPORTED, "head_dim 32 is not supported (64, 128 or 256)"),
    ("fa_fp8_forward_hdim", PADDED, dict(heads_kv=3, dtype=0), INVALID_ARGUMENT, "multiple of heads_kv"),
    ("fa_fp8_forward_hdim", PADDED, dict(dtype=0, window_left=-2), INVALID_ARGUMENT, "dtype (of o)"),
    ("fa_fp8_forward_hdim", PADDED, dict(window_left=-2, q=ODD), INVALID_ARGUMENT, "window (-2, -1)"),
    ("fa_fp8_forward_hdim", PADDED, dict(sink_heads=4, q=ODD), INVALID_ARGUMENT, "sink_heads must be 0 without sinks"),
    ("fa_fp8_forward_hdim", PADDED, dict(q=ODD, q_token_stride=48), INVALID_ARGUMENT, "16-byte aligned"),
    ("fa_fp8_forward_hdim", PADDED, dict(k_token_stride=48, workspace=None), INVALID_ARGUMENT, "the token stride >= 64"),
    ("fa_fp8_forward_hdim", PADDED, dict(head_dim=256, workspace=None), INVALID_ARGUMENT, "the token stride >= 256"),
    ("fa_fp8_forward_hdim", PADDED, dict(head_dim=128, v_token_stride=64, workspace=None), INVALID_ARGUMENT, "the token stride >= 128"),
    ("fa_fp8_forward_hdim", PADDED, dict(seqlen_q=2 ** 20, q_token_stride=4096, workspace=None), UNSUPPORTED, "span limit"),
    ("fa_fp8_forward_hdim", PADDED, dict(workspace=None), WORKSPACE, "fa_fp8_forward_hdim_workspace_bytes"),
    ("fa_fp8_forward_hdim", PADDED, dict(workspace_bytes=2 * 2 * 3 * 64 * 128 + 255), WORKSPACE, f"need {2 * 2 * 3 * 64 * 128 + 256}"),
    ("fa_fp8_forward_hdim", PADDED, dict(workspace=ODD), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(cu_seqlens_q=None, head_dim=96), INVALID_ARGUMENT, "null cu_seqlens pointer"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(total_q=-1, head_dim=96), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(head_dim=96, heads_kv=3), UNSUPPORTED, "head_dim 96 is not supported (64, 128 or 256)"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(heads_kv=3, dtype=0), INVALID_ARGUMENT, "multiple of heads_kv"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(softcap=-1.0, page_block_size=16), INVALID_ARGUMENT, "softcap must be a finite number"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(page_block_size=16, q_token_stride=48), INVALID_ARGUMENT, "must be 0 without block_table"),
    ("fa_fp8_forward_varlen_hdim", PAGED, dict(page_block_size=24, q_token_stride=48), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(q_token_stride=48, workspace=None), INVALID_ARGUMENT, "the token stride >= 64"),
    ("fa_fp8_forward_varlen_hdim", PAGED, dict(head_dim=256, workspace=None), INVALID_ARGUMENT, "the token stride >= 256"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(max_seqlen_q=2 ** 20, q_token_stride=4096, workspace=None), UNSUPPORTED, "span limit"),
    ("fa_fp8_forward_varlen_hdim", PACKED, dict(workspace=None), WORKSPACE, "fa_fp8_forward_varlen_hdim_workspace_bytes"),
    ("fa_fp8_forward_varlen_hdim", PAGED, dict(workspace_bytes=1000), WORKSPACE, f"need {2 * 3 * 4 * 64 * 128 + 256}"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(q=None, head_dim=96), INVALID_ARGUMENT, "null tensor pointer"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(head_dim=96, heads_kv=3), UNSUPPORTED, "head_dim 96 is not supported (64, 128 or 256)"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(q_dtype=2, heads_kv=3), UNSUPPORTED, "q_dtype must be FA_DTYPE_E4M3"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(heads_kv=3, batch=70000), INVALID_ARGUMENT, "multiple of heads_kv"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(batch=70000, q_token_stride=8), INVALID_ARGUMENT, "batch must lie"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(q_token_stride=256, num_splits=300), INVALID_ARGUMENT, "the token stride >= heads * 64 = 512"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(head_dim=256, num_splits=300), INVALID_ARGUMENT, "the token stride >= heads * 256 = 2048"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(k_token_stride=64, num_splits=300), INVALID_ARGUMENT, "strides of k_cache"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(num_splits=300, workspace=None), INVALID_ARGUMENT, "num_splits"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(window_right=-5, workspace=None), INVALID_ARGUMENT, "window (-1, -5)"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(workspace=None), WORKSPACE, "fa_fp8_forward_kvcache_hdim_workspace_bytes"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(workspace_bytes=1000), WORKSPACE, f"need {hr.kvcache_workspace_bytes(3, 8, 2, 64, 4)}"),
    ("fa_fp8_forward_kvcache_hdim", DECODE, dict(workspace=ODD), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("name,base,kw,code,what", REFUSALS, ids=[f"{i:02d}-{r[0][11:-5]}-{r[4][:20].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_in_the_parents_order_before_any_hip_call(name, base, kw, code, what):
    rc, msg = invoke(name, base, **kw)
    assert rc == code, (rc, msg)
    assert what in msg and msg.startswith(name + ":"), msg


def test_the_older_entry_points_refuse_what_they_refused():
    for name, base in (("fa_fp8_forward_mod", PADDED), ("fa_fp8_forward_varlen_mod", PACKED), ("fa_fp8_forward_kvcache_mod", DECODE)):
        a = dict(base)
        a["d"] = a.pop("head_dim")
        for d in (64, 256):
            rc, msg = invoke(name, a, d=d)
            assert rc == UNSUPPORTED and f"head_dim {d} is not supported (128 only)" in msg, msg


def test_the_empty_decode_call_is_ok_before_anything_is_looked_at():
    for kw in (dict(batch=0), dict(seqlen_q=0)):
        rc, _ = invoke("fa_fp8_forward_kvcache_hdim", DECODE, q=None, head_dim=96, **kw)
        assert rc == OK


def test_the_workspace_sizes():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for d in hr.HEAD_DIMS:
        for b, hkv, nk in ((2, 2, 300), (1, 3, 128), (5, 1, 129)):
            assert lib.fa_fp8_forward_hdim_workspace_bytes(b, hkv, nk, d) == hr.forward_workspace_bytes(b, hkv, nk, d)
        for b, hkv, tk, mk, mb, ps in ((3, 2, 700, 400, 0, 0), (3, 2, 0, 400, 30, 16), (2, 1, 127, 127, 0, 0), (4, 2, 0, 10 ** 6, 5, 48)):
            assert lib.fa_fp8_forward_varlen_hdim_workspace_bytes(b, hkv, tk, mk, mb, ps, d) == hr.varlen_workspace_bytes(b, hkv, tk, mk, mb, ps, d)
        for ns, causal, wl, wr, snk, want in ((4, 1, -1, -1, 0, 4), (1, 1, -1, -1, 0, 1), (1, 0, 128, -1, 1, 2), (7, 0, -1, -1, 1, 7)):
            assert lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(3, 8, 2, 2, 1000, d, ns, causal, wl, wr, snk) == \
                hr.kvcache_workspace_bytes(3, 8, 2, d, want)
        # the split rule (num_splits = 0) counts keys, not bytes: the same number of splits at every head dim
        auto = lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(1, 8, 2, 1, 8192, d, 0, 1, -1, -1, 0)
        call = dict(B=1, hq=8, hkv=2, nq=1, num_splits=0, causal=True, window=(-1, -1), sinks=None, block_table=None,
                    k_cache=torch.empty((1, 8192, 0, 0)))
        assert auto == hr.kvcache_workspace_bytes(1, 8, 1, d, km.num_splits(call)) and km.num_splits(call) > 1
    # d = 128: the parents' sizes
    assert lib.fa_fp8_forward_hdim_workspace_bytes(2, 2, 300, 128) == lib.fa_fp8_forward_workspace_bytes(2, 2, 300, 128) > 0
    assert lib.fa_fp8_forward_varlen_hdim_workspace_bytes(3, 2, 700, 400, 0, 0, 128) == lib.fa_fp8_forward_varlen_workspace_bytes(3, 2, 700, 400, 0, 0, 128) > 0
    assert lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(3, 8, 2, 2, 1000, 128, 0, 1, 64, -1, 1) == \
        lib.fa_fp8_forward_kvcache_workspace_bytes_mod(3, 8, 2, 2, 1000, 128, 0, 1, 64, -1, 1) > 0
    # refused arguments: 0
    for d in (96, 192, 0, 32, 512):
        assert lib.fa_fp8_forward_hdim_workspace_bytes(2, 2, 300, d) == 0
        assert lib.fa_fp8_forward_varlen_hdim_workspace_bytes(3, 2, 700, 400, 0, 0, d) == 0
        assert lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(3, 8, 2, 2, 1000, d, 4, 1, -1, -1, 0) == 0
    assert lib.fa_fp8_forward_hdim_workspace_bytes(0, 2, 300, 64) == 0
    assert lib.fa_fp8_forward_varlen_hdim_workspace_bytes(3, 2, 0, 400, 30, 24, 64) == 0
    assert lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(3, 8, 3, 2, 1000, 64, 4, 1, -1, -1, 0) == 0
    assert lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(3, 8, 2, 2, 1000, 64, 4, 1, -2, -1, 0) == 0
    # and the older ones still answer 0 at 64 and 256
    for d in (64, 256):
        assert lib.fa_fp8_forward_workspace_bytes(2, 2, 300, d) == 0
        assert lib.fa_fp8_forward_kvcache_workspace_bytes_mod(3, 8, 2, 2, 1000, d, 4, 1, -1, -1, 0) == 0


def _f8(*shape):
    return torch.zeros(shape, dtype=torch.uint8).view(E4)


def test_the_wrappers_refuse_by_name():
    from common.fp8_attention import fp8_attn_func, fp8_attn_varlen_func, fp8_attn_with_kvcache

    cu = torch.tensor([0, 4], dtype=torch.int32)
    padded = lambda dq, dk, dv, **kw: fp8_attn_func(_f8(1, 2, 4, dq), _f8(1, 2, 4, dk), _f8(1, 2, 4, dv), **kw)   # noqa: E731
    packed = lambda dq, dk, dv, **kw: fp8_attn_varlen_func(_f8(4, 2, dq), _f8(4, 2, dk), _f8(4, 2, dv), cu, cu, 4, 4, **kw)   # noqa: E731
    decode = lambda dq, dk, dv, **kw: fp8_attn_with_kvcache(_f8(1, 1, 2, dq), _f8(1, 16, 2, dk), _f8(1, 16, 2, dv), **kw)   # noqa: E731
    for fn in (padded, packed, decode):
        for dims in ((64, 128, 64), (64, 64, 256), (256, 64, 64)):
            with pytest.raises(RuntimeError, match="mixed head dims: q has"):
                fn(*dims)
        for d in (96, 192, 32, 512):
            with pytest.raises(NotImplementedError, match=rf"head_dim {d} is not supported \(64, 128 or 256\)"):
                fn(d, d, d)
        with pytest.raises(NotImplementedError, match="out_dtype torch.float32 is not supported"):
            fn(64, 64, 64, out_dtype=torch.float32)
        with pytest.raises(NotImplementedError, match="alibi_slopes is not supported"):
            fn(64, 64, 64, alibi_slopes=torch.zeros(2))
        with pytest.raises(TypeError, match="unexpected keyword argument"):
            fn(64, 64, 64, no_such_argument=1)
        with pytest.raises(RuntimeError, match="window"):
            fn(256, 256, 256, window_size=(-2, 0))
        for d in hr.HEAD_DIMS:              # the head dim passes: the call gets as far as the device check
            with pytest.raises(RuntimeError, match="must be on the GPU"):
                fn(d, d, d)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: q is"):
            fp8_attn_func(torch.zeros((1, 2, 4, 64), dtype=dt), _f8(1, 2, 4, 64), _f8(1, 2, 4, 64))
        with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: v is"):
            fp8_attn_varlen_func(_f8(4, 2, 64), _f8(4, 2, 64), torch.zeros((4, 2, 64), dtype=dt), cu, cu, 4, 4)
        with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: q is"):
            fp8_attn_with_kvcache(torch.zeros((1, 1, 2, 64), dtype=dt), _f8(1, 16, 2, 64), _f8(1, 16, 2, 64))
    with pytest.raises(NotImplementedError, match="block_table together with cache_batch_idx"):
        decode(64, 64, 64, block_table=torch.zeros((1, 1), dtype=torch.int32), cache_batch_idx=torch.zeros(1, dtype=torch.int32))


def test_the_older_wrappers_and_the_shim_without_hdim_still_refuse_64_and_256():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_fp8_func, flash_attn_fp8_with_kvcache

    for d in (64, 256):
        with pytest.raises(NotImplementedError, match=rf"head_dim {d} is not supported \(128 only\)"):
            flash_attn_fp8_func(_f8(1, 2, 4, d), _f8(1, 2, 4, d), _f8(1, 2, 4, d))
        with pytest.raises(NotImplementedError, match=rf"head_dim {d} is not supported \(128 only\)"):
            flash_attn_fp8_with_kvcache(_f8(1, 1, 2, d), _f8(1, 16, 2, d), _f8(1, 16, 2, d))
    assert ext._fp8_head_dim("x", False, q=_f8(1, 64)) == 128 and ext._fp8_head_dim("x", True, q=_f8(1, 64), k=_f8(3, 64)) == 64


# ---- the model

def _close(a, b, tol=1e-10):
    fin = torch.isfinite(b.lse)
    assert torch.equal(torch.isfinite(a.lse), fin) and torch.equal(a.lse[~fin], b.lse[~fin])
    assert float((a.o - b.o).abs().max()) <= tol * max(1.0, float(b.o.abs().max()))
    assert float((a.lse[fin] - b.lse[fin]).abs().max()) <= tol * max(1.0, float(b.lse[fin].abs().max()))


def _bits(a, b):
    return torch.equal(a.o.float().view(torch.int32), b.o.float().view(torch.int32)) and \
        torch.equal(a.lse.float().view(torch.int32), b.lse.float().view(torch.int32))


def test_at_128_the_prefill_model_is_the_pinned_one_bit_for_bit():
    call = fm.build_call(1, softcap=True, sinks=True)         # (130, 400), window (50, 30), capped, sinks
    mine = dict(call, d=128)
    assert hr.key_tile(128) == 128 and hr.key_tile(64) == 128 and hr.key_tile(256) == 64
    assert _bits(hr.baseline(mine), fm.baseline(call))
    _close(hr.reference(mine), fm.reference(call))
    bare = dict(fm.build_call(3), window=(-1, -1))            # (260, 200) causal: dead rows
    assert _bits(hr.baseline(dict(bare, d=128)), fm.baseline(bare))


def test_at_128_the_decode_model_is_the_pinned_one_bit_for_bit():
    for i in (1, 6):                                          # nq 3, paged, three splits; with sinks
        call = km.build_call(i)
        mine = dict(call, d=128)
        assert _bits(hr.decode_baseline(mine), km.baseline(call))
        _close(hr.decode_reference(mine), km.reference(call))
        got = km.baseline(call)
        o, lse = fk.unpack(got, call)
        assert _bits(hr.pack(o, lse, mine), got)


@pytest.mark.parametrize("d", [64, 256])
def test_without_rounding_the_model_is_the_fp64_definition(d):
    call = hr.make_call(d, (150, 70), False, (40, 0), 30.0, hr.the_sinks(4), batch=1, seed=5)
    ref = hr.reference(call)
    _close(hr.baseline(call, torch.float64, rounding=False), ref)
    base = hr.baseline(call)
    bad, _r = tiled_sharp_bar(base, ref, base, call["dtype"])
    assert not bad, bad
    dead = ~fm.band(call).any(-1)
    assert bool(dead.any()) and bool((ref.o[:, dead] == 0).all())
    dc = hr.decode_call(d, (8, 2), 3, (0, 63, 192), "ps16", 3, (128, -1), True, seed=d)
    dref = hr.decode_reference(dc)
    _close(hr.decode_baseline(dc, torch.float64, rounding=False), dref)
    dbase = hr.decode_baseline(dc)
    bad, _r = fk.tile_bar(dbase, dref, dbase, dc["dtype"])
    assert not bad, bad
    assert dref.o.shape[-1] == d
    g = 4                                                     # the empty first sequence: o = 0 and lse = the sink of the row's head
    want = torch.stack([hr.the_sinks(8).double()[hk * g + torch.arange(3 * g) % g] for hk in range(2)])
    assert torch.equal(dref.lse[:2], want) and bool((dref.o[:2] == 0).all())
