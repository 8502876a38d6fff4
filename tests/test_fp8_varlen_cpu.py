"""CPU: the packed and the paged form of the fp8 call (include/fa_mi355x.h: fa_fp8_forward_varlen,
fa_fp8_forward_varlen_workspace_bytes) — declared, exported, the signature rows and a family of its own, every bad
argument rejected before any HIP call in the documented order, the workspace formula against the Python model, the wrappers'
refusals by name, and the two device rules of tests/fp8_varlen_cases.py: the V^T regions of the sequences never overlap and fit the
workspace, and the per-piece descriptors stage what a gather through the table gives."""
import ctypes
import os
import random
import re

import pytest
import torch

from tests import fp8_varlen_cases as vc
from tests.test_abi_signatures_cpu import PROTOTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
NAMES = ("fa_fp8_forward_varlen", "fa_fp8_forward_varlen_workspace_bytes")
OK, INVALID_ARGUMENT, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

ORDER = ("q", "k", "v", "o", "lse", "qd", "kd", "vd", "cuq", "cuk", "bt", "b", "hq", "hkv", "tq", "tk", "mq", "mk", "d", "dtype", "qt", "qh",
         "kt", "kh", "vt", "vh", "mb", "nb", "ps", "kp", "vp", "qdb", "kdb", "vdb", "causal", "scale", "ws", "wsb")
# packed: B = 3, H_q = 4, H_kv = 2, 700 query and 900 key tokens, q a slice of a fused projection (token stride 512), k and v
# interleaved halves (token stride 256), bf16 out, (B, H_kv) descales, an ample workspace
BASE = dict(q=P, k=P, v=P, o=P, lse=P, qd=P, kd=P, vd=P, cuq=P, cuk=P, bt=None, b=3, hq=4, hkv=2, tq=700, tk=900, mq=300, mk=500, d=128,
            dtype=2, qt=512, qh=128, kt=256, kh=128, vt=256, vh=128, mb=0, nb=0, ps=0, kp=0, vp=0, qdb=2, kdb=2, vdb=2, causal=1,
            scale=128 ** -0.5, ws=P, wsb=2 ** 40)
# paged: 64 pages of 48 tokens, 10 table entries a sequence
PAGED = dict(BASE, bt=P, tk=0, mb=10, nb=64, ps=48, kp=48 * 256, vp=48 * 256 + 512)


def _call(base=BASE, **kw):
    import flashattention_lab_cuda as ext

    a = dict(base, **kw)
    rc = ext._lib.fa_fp8_forward_varlen(*[a[n] for n in ORDER], None)
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
    assert hasattr(ext, "fp8_varlen_forward") and hasattr(attention_ex, "flash_attention_fp8_varlen")


def test_signature_rows_and_a_family_of_its_own():
    import flashattention_lab_cuda as ext

    names = PROTOTYPES["fa_fp8_forward_varlen"][2]
    assert [f for f, _t in ext._SIGNATURES["fa_fp8_forward_varlen"][1]] == names and len(names) == len(ORDER) + 1   # (all but the stream)
    assert names[:11] == ["q", "k", "v", "o", "lse", "q_descale", "k_descale", "v_descale", "cu_seqlens_q", "cu_seqlens_k", "block_table"]
    assert names[11:20] == ["batch", "heads_q", "heads_kv", "total_q", "total_k", "max_seqlen_q", "max_seqlen_k", "d", "dtype"]
    assert names[-5:] == ["causal", "softmax_scale", "workspace", "workspace_bytes", "stream"]
    assert PROTOTYPES["fa_fp8_forward_varlen"][1][20:34] == [ctypes.c_int64] * 14
    assert PROTOTYPES["fa_fp8_forward_varlen_workspace_bytes"][2] == ["batch", "heads_kv", "total_k", "max_seqlen_k", "max_blocks_per_seq",
                                                                       "page_block_size", "d"]
    assert PROTOTYPES["fa_fp8_forward_varlen_workspace_bytes"][0] is ctypes.c_size_t
    fn, own, count = ext._CALLS["fa_fp8_forward_varlen"]
    assert count == len(names) and list(own(tuple(names))) == names
    # the padded call's row and family are what they were
    assert len(ext._SIGNATURES["fa_fp8_forward"][1]) == 35 and ext._CALLS["fa_fp8_forward"][2] == 35


A8 = ctypes.c_void_p(4096 + 8)
A2 = ctypes.c_void_p(4096 + 2)
# every row is rejected before any HIP call: there is no GPU here, and the pointers are fake.  In the documented order: a later
# rule's breach does not hide an earlier one (the rows with two breaches).
BAD = [
    # (1) null pointers, before the dims
    (BASE, dict(q=None), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(k=None, b=0), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(v=None, d=64), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(o=None), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(lse=None, dtype=0), INVALID_ARGUMENT, "null tensor pointer"),
    (BASE, dict(cuq=None, hq=0), INVALID_ARGUMENT, "null cu_seqlens pointer"),
    (PAGED, dict(cuk=None, ps=8), INVALID_ARGUMENT, "null cu_seqlens pointer"),
    # (2) dims, before the head dim
    (BASE, dict(b=0), INVALID_ARGUMENT, "batch, heads_q, heads_kv and d must be > 0"),
    (BASE, dict(hq=0, d=64), INVALID_ARGUMENT, "must be > 0"),
    (BASE, dict(hkv=-1), INVALID_ARGUMENT, "must be > 0"),
    (BASE, dict(d=0), INVALID_ARGUMENT, "must be > 0"),
    (BASE, dict(tq=-1, d=64), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    (BASE, dict(tk=2 ** 31), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    (BASE, dict(mq=-5), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    (PAGED, dict(mk=2 ** 31, hq=3), INVALID_ARGUMENT, "must lie in [0, 2^31)"),
    # (3) d == 128, before the heads ratio
    (BASE, dict(d=64), UNSUPPORTED, "head_dim 64 is not supported (128 only)"),
    (PAGED, dict(d=256, hq=3), UNSUPPORTED, "head_dim 256 is not supported"),
    # (4) the heads ratio, before the dtype
    (BASE, dict(hq=3), INVALID_ARGUMENT, "heads_q=3 must be a multiple of heads_kv=2"),
    (BASE, dict(hq=2, hkv=4, dtype=0), INVALID_ARGUMENT, "heads_q=2 must be a multiple of heads_kv=4"),
    # (5) dtype and scale, before the pages
    (BASE, dict(dtype=0), INVALID_ARGUMENT, "dtype (of o) must be f16 or bf16 (got code 0)"),
    (PAGED, dict(dtype=3, ps=8), INVALID_ARGUMENT, "dtype (of o) must be f16 or bf16 (got code 3)"),
    (BASE, dict(scale=0.0), INVALID_ARGUMENT, "softmax_scale must be finite and > 0"),
    (PAGED, dict(scale=float("nan"), nb=0), INVALID_ARGUMENT, "softmax_scale must be finite and > 0"),
    (BASE, dict(scale=float("inf")), INVALID_ARGUMENT, "softmax_scale must be finite and > 0"),
    # (6) the pages, before the descale strides
    (PAGED, dict(ps=8), INVALID_ARGUMENT, "page_block_size must be a multiple of 16 in [16, 65536] (got 8)"),
    (PAGED, dict(ps=40, qdb=1), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    (PAGED, dict(ps=2 ** 17), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    (PAGED, dict(ps=0), INVALID_ARGUMENT, "page_block_size must be a multiple of 16"),
    (PAGED, dict(nb=0), INVALID_ARGUMENT, "num_blocks must lie in [1, 2^31) (got 0)"),
    (PAGED, dict(mb=-1), INVALID_ARGUMENT, "batch * max_blocks_per_seq must lie in [0, 2^31)"),
    (PAGED, dict(mb=2 ** 30, vd=None), INVALID_ARGUMENT, "batch * max_blocks_per_seq must lie in [0, 2^31)"),
    (BASE, dict(ps=16), INVALID_ARGUMENT, "must be 0 without block_table"),
    (BASE, dict(kp=4096, kdb=1), INVALID_ARGUMENT, "must be 0 without block_table"),
    # (7) the descale strides, before the alignment
    (BASE, dict(qdb=1), INVALID_ARGUMENT, "q_descale_batch_stride=1 must be 0 or >= heads_kv=2"),
    (BASE, dict(kdb=-2), INVALID_ARGUMENT, "k_descale_batch_stride=-2 must be 0 or >= heads_kv=2"),
    (PAGED, dict(vd=None), INVALID_ARGUMENT, "v_descale_batch_stride must be 0 without v_descale"),
    (BASE, dict(kd=A2, kt=8), INVALID_ARGUMENT, "k_descale must be 4-byte aligned"),
    # (8) alignment and strides, before the span limits
    (BASE, dict(q=A8), INVALID_ARGUMENT, "q, k, v and o must be 16-byte aligned"),
    (BASE, dict(v=ctypes.c_void_p(4096 + 4), kt=2 ** 30), INVALID_ARGUMENT, "q, k, v and o must be 16-byte aligned"),
    (BASE, dict(lse=A2), INVALID_ARGUMENT, "lse, cu_seqlens_q, cu_seqlens_k and block_table must be 4-byte aligned"),
    (BASE, dict(cuk=A2), INVALID_ARGUMENT, "lse, cu_seqlens_q, cu_seqlens_k and block_table must be 4-byte aligned"),
    (PAGED, dict(bt=A2, ws=None), INVALID_ARGUMENT, "lse, cu_seqlens_q, cu_seqlens_k and block_table must be 4-byte aligned"),
    (BASE, dict(qt=520), INVALID_ARGUMENT, "the strides of q (token 520, head 128, page 0) must be multiples of 16 bytes"),
    (BASE, dict(kh=136), INVALID_ARGUMENT, "the strides of k"),
    (PAGED, dict(vp=48 * 256 + 8, ws=None), INVALID_ARGUMENT, "the strides of v (token 256, head 128, page 12296) must be multiples of 16 bytes"),
    (BASE, dict(kt=64), INVALID_ARGUMENT, "the token stride >= 128"),
    (BASE, dict(qh=-16), INVALID_ARGUMENT, "must be >= 0"),
    (PAGED, dict(kp=-4096), INVALID_ARGUMENT, "must be >= 0"),
    # (9) the span limits, by name, before the workspace
    (BASE, dict(qt=2 ** 22), UNSUPPORTED, "span limit: round_up(max_seqlen_q, 256) * token stride of q is 2147483648 bytes"),
    (BASE, dict(kt=2 ** 22, ws=None), UNSUPPORTED, "span limit: round_up(max_seqlen_k, 256) * token stride of k is 2147483648 bytes"),
    (PAGED, dict(kt=2 ** 22, ps=512), UNSUPPORTED, "span limit: page_block_size * token stride of k is 2147483648 bytes"),
    (PAGED, dict(vt=2 ** 22, ps=512, ws=None), UNSUPPORTED, "span limit: page_block_size * token stride of v"),
    (PAGED, dict(mk=2 ** 24, mb=2 ** 20, ps=16), UNSUPPORTED, "is at or above 2^24"),
    (BASE, dict(b=2 ** 20, hq=2 ** 11, hkv=2 ** 11, qd=None, kd=None, vd=None, qdb=0, kdb=0, vdb=0), UNSUPPORTED,
     "span limit: batch * heads * tiles"),
    # (10) the workspace
    (BASE, dict(ws=None), WORKSPACE, "workspace of 0 bytes is too small (need 327936"),
    (BASE, dict(wsb=327935), WORKSPACE, "workspace of 327935 bytes is too small (need 327936"),
    (PAGED, dict(wsb=393471), WORKSPACE, "workspace of 393471 bytes is too small (need 393472"),
    (PAGED, dict(ws=A8), INVALID_ARGUMENT, "workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("base,kw,code,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments_are_rejected_before_any_hip_call(base, kw, code, what):
    rc, msg = _call(base, **kw)
    assert rc == code, (kw, msg)
    assert what in msg and msg.startswith("fa_fp8_forward_varlen:"), (kw, msg)


def test_head_strides_of_one_head_are_not_looked_at():
    rc, msg = _call(hq=1, hkv=1, qh=7, kh=3, vh=5, qdb=1, kdb=1, vdb=1, ws=None)
    assert rc == WORKSPACE and f"need {vc.workspace_bytes(3, 1, 900, 500)}" in msg, msg


def test_the_workspace_formula_is_the_model():
    import flashattention_lab_cuda as ext

    f = ext._lib.fa_fp8_forward_varlen_workspace_bytes
    for b, hkv, total_k, max_k in ((1, 1, 1, 1), (3, 2, 900, 500), (4, 1, 128, 128), (4, 2, 127, 40), (2, 8, 0, 0), (16, 1, 16 * 16384, 16384)):
        assert f(b, hkv, total_k, max_k, 0, 0, 128) == vc.workspace_bytes(b, hkv, total_k, max_k)
        assert f(b, hkv, total_k, max_k, 7, 0, 128) == vc.workspace_bytes(b, hkv, total_k, max_k)   # (page_block_size 0: packed)
    assert f(3, 2, 900, 500, 0, 0, 128) == 2 * (7 + 3) * 16384 + 256
    for b, hkv, max_k, mb, ps in ((1, 1, 1, 1, 16), (3, 2, 500, 10, 48), (3, 2, 500, 11, 48), (4, 2, 129, 1, 256), (2, 1, 300, 0, 16), (16, 1, 16384, 64, 256)):
        assert f(b, hkv, 12345, max_k, mb, ps, 128) == vc.workspace_bytes(b, hkv, 0, max_k, mb, ps)
    assert f(3, 2, 0, 500, 10, 48, 128) == 2 * 3 * 4 * 16384 + 256
    for bad in ((0, 1, 1, 1, 0, 0, 128), (1, 0, 1, 1, 0, 0, 128), (1, 1, -1, 1, 0, 0, 128), (1, 1, 1, 1, 0, 0, 64), (1, 1, 1, 1, 4, 24, 128),
                (1, 1, 1, -1, 0, 0, 128)):
        assert f(*bad) == 0


def test_the_wrappers_refuse_by_name():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attention_fp8_varlen

    q8 = torch.zeros((32, 2, 128), dtype=torch.float8_e4m3fn)
    q16 = torch.zeros((32, 2, 128), dtype=torch.bfloat16)
    cu = torch.tensor([0, 16, 32], dtype=torch.int32)
    args = (cu, cu, 16, 16)
    for name, val in (("window_size", (8, 0)), ("softcap", 30.0), ("alibi_slopes", torch.ones(2)), ("sinks", torch.zeros(2)),
                      ("attn_bias", torch.zeros(16, 16)), ("mask", torch.ones(16, 16)), ("block_sparse_mask", torch.ones(1, 1)),
                      ("dropout_p", 0.1), ("seqused_q", cu[:2]), ("seqused_k", cu[:2]), ("cache_leftpad", cu[:2]), ("cache_batch_idx", cu[:2])):
        with pytest.raises(NotImplementedError, match=f"flash_attention_fp8_varlen: {name} is not supported"):
            flash_attention_fp8_varlen(q8, q8, q8, *args, **{name: val})
    with pytest.raises(TypeError, match="unexpected keyword argument 'nonsense'"):
        flash_attention_fp8_varlen(q8, q8, q8, *args, nonsense=1)
    with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: q is torch.bfloat16"):
        flash_attention_fp8_varlen(q16, q8, q8, *args)
    with pytest.raises(NotImplementedError, match="16-bit inputs are not supported: v is torch.bfloat16"):
        flash_attention_fp8_varlen(q8, q8, q16, *args)
    with pytest.raises(NotImplementedError, match="k of dtype torch.uint8 is not supported"):
        flash_attention_fp8_varlen(q8, q8.view(torch.uint8), q8, *args)
    with pytest.raises(NotImplementedError, match="head_dim 64 is not supported"):
        flash_attention_fp8_varlen(q8[..., :64], q8[..., :64], q8[..., :64], *args)
    with pytest.raises(NotImplementedError, match="out_dtype torch.float32 is not supported"):
        flash_attention_fp8_varlen(q8, q8, q8, *args, out_dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="block_table of dtype torch.int64 is not supported"):
        flash_attention_fp8_varlen(q8, q8.reshape(2, 16, 2, 128), q8.reshape(2, 16, 2, 128), *args, block_table=torch.zeros((2, 1), dtype=torch.int64))
    qg = torch.zeros((32, 2, 128), dtype=torch.bfloat16, requires_grad=True).to(torch.float8_e4m3fn)
    assert qg.requires_grad
    with pytest.raises(RuntimeError, match="forward only"):
        flash_attention_fp8_varlen(qg, q8, q8, *args)
    # the defaults of the refused arguments pass through to the shim, which has no CPU path
    with pytest.raises(RuntimeError, match="tensors must be on the GPU"):
        flash_attention_fp8_varlen(q8, q8, q8, *args, window_size=(-1, -1), softcap=0.0, dropout_p=0.0, sinks=None, seqused_k=None)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="tensors must be on the GPU"):
            flash_attention_fp8_varlen(qg, q8, q8, *args)
    with pytest.raises(NotImplementedError, match="fp8_varlen_forward: q of dtype torch.bfloat16 is not supported"):
        ext.fp8_varlen_forward(q16, q8, q8, *args, False, None)
    with pytest.raises(RuntimeError, match=r"pools \(num_blocks, page_block_size, H_kv, 128\)"):
        ext.fp8_varlen_forward(q8, q8, q8, *args, False, None, block_table=torch.zeros((2, 1), dtype=torch.int32))
    # the padded call, the 16-bit packed call and the decode call refuse what they refused
    from common.attention_ex import flash_attention_fp8, flash_attention_varlen

    with pytest.raises(NotImplementedError, match="flash_attention_fp8: cu_seqlens_q is not supported by the fp8 call"):
        flash_attention_fp8(q8[None], q8[None], q8[None], cu_seqlens_q=cu)
    with pytest.raises(RuntimeError, match="torch.float8_e4m3fn k, v are pools of a paged cache and need block_table"):
        flash_attention_varlen(q16, q8, q8, *args)


# ---- where a sequence's V^T tiles start

def _offsets(rng, batch, total_rem):
    """a monotone offset list of `batch` sequences, empty ones included, whose total has the wanted remainder mod 128"""
    lens = [rng.choice((0, 0, 1, 63, 64, 65, 127, 128, 129, 300, rng.randrange(0, 700))) for _ in range(batch)]
    lens[-1] += (total_rem - sum(lens)) % 128
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


@pytest.mark.parametrize("total_rem", [0, 1, 127, 77])
def test_packed_regions_never_overlap_and_fit_the_workspace(total_rem):
    rng = random.Random(1000 + total_rem)
    for _ in range(300):
        batch = rng.randrange(1, 9)
        cu = _offsets(rng, batch, total_rem)
        total = cu[-1]
        assert total % 128 == total_rem
        lens = [cu[b + 1] - cu[b] for b in range(batch)]
        max_k = max(lens) if rng.random() < 0.7 else rng.randrange(0, max(lens) + 1)     # (a max below a length clamps it)
        regions = vc.packed_regions(cu, total, max_k)
        tiles = vc.packed_tiles_per_head(batch, total)
        end = 0
        for b, (first, n) in enumerate(regions):
            assert n == (min(lens[b], max_k) + 127) // 128
            assert first >= end, (cu, b)                       # in order, no overlap (an empty region may share its start)
            end = first + n
        assert end <= tiles, (cu, tiles)
        assert vc.workspace_bytes(batch, 3, total, max_k) == 3 * tiles * 16384 + 256


def test_untrusted_packed_offsets_stay_inside_the_workspace():
    rng = random.Random(7)
    for _ in range(300):
        batch, total = rng.randrange(1, 7), rng.randrange(0, 2000)
        cu = [rng.randrange(-500, 3000) for _ in range(batch + 1)]
        max_k = rng.randrange(0, 1000)
        for first, n in vc.packed_regions(cu, total, max_k):
            assert 0 <= first and first + n <= vc.packed_tiles_per_head(batch, total)


def test_paged_regions_never_overlap_and_fit_the_workspace():
    rng = random.Random(11)
    for _ in range(300):
        batch, ps = rng.randrange(1, 7), rng.choice(vc.PAGE_SIZES)
        max_blocks, max_k = rng.randrange(0, 9), rng.randrange(0, 900)
        base = rng.randrange(-100, 100)
        lens = [rng.randrange(-50, 1200) for _ in range(batch)]
        cu = [base]
        for n in lens:
            cu.append(cu[-1] + n)
        cap = vc.paged_cap(max_k, max_blocks, ps)
        end = 0
        for b, (first, n) in enumerate(vc.paged_regions(cu, max_k, max_blocks, ps)):
            assert n == (min(max(lens[b], 0), cap) + 127) // 128 and first >= end
            end = first + n
        assert end <= vc.paged_tiles_per_head(batch, max_k, max_blocks, ps)


# ---- what a 1-KiB K piece reads

@pytest.mark.parametrize("ps", vc.PAGE_SIZES)
def test_the_piece_rule_stages_what_a_gather_gives(ps):
    g = torch.Generator().manual_seed(ps)
    num_blocks, max_blocks = 12, 6
    pool = torch.randint(1, 120, (num_blocks, ps, 4), generator=g, dtype=torch.uint8)
    edges = sorted({n for e in (8, 16, ps, 2 * ps, 128, 256) for n in (e - 1, e, e + 1) if 0 < n <= max_blocks * ps} | {1, max_blocks * ps})
    for nk in edges:
        need = (nk + ps - 1) // ps
        row = torch.full((max_blocks,), 10 ** 6, dtype=torch.int32)            # past the live entries: never a valid page
        row[:need] = torch.randperm(num_blocks, generator=g)[:need].to(torch.int32)
        for bad_page in (None, -1, num_blocks):
            r = row.clone()
            if bad_page is not None:
                r[need // 2] = bad_page                                         # an entry outside the pool inside the live sequence
            want = vc.gather(pool, r, nk, ps)
            for t in range((nk + 127) // 128 + 1):                              # (one tile past the end: all zeros)
                got, slots = vc.stage_tile(t, nk, ps, r, pool)
                lo, hi = 128 * t, min(128 * t + 128, nk)
                assert torch.equal(got[:max(hi - lo, 0)], want[lo:hi]), (ps, nk, t)
                assert bool((got[max(hi - lo, 0):] == 0).all())
                assert max(slots) < need, (ps, nk, t, slots)                    # no entry past ceil(nk / ps) is read
            for key in range(0, nk + 16, 8):
                slot, _page, first, rows = vc.piece(key, nk, ps, r, num_blocks)
                assert 0 <= first and (rows == 0 or first + rows <= ps)         # a piece never straddles a page
    assert vc.piece(0, 0, ps, torch.zeros(1, dtype=torch.int32), num_blocks)[3] == 0
