"""CPU: rotary embedding for training and prefill (include/fa_mi355x.h: fa_rotary_apply; common/rotary.py) — declared and
exported, every host-side validation rule before any HIP call, the Python wrappers' layout and argument errors, a model of the
kernel's thread-to-chunk map that proves the in-place form free of races, the packed clamp, and the check that on the GPU
tests' own inputs an fp32 evaluation of the rotation (plain and conjugate) rounds exactly as the fp64 reference does."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from tests.rotary_ref import (BATCH, CASES, SEQLEN_RO, case_id, case_inputs, pairs, positions, reference64, round_once, span,
                              unit_count, unit_model)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
INVALID_ARGUMENT = -1
P = ctypes.c_void_p(4096)     # non-null, 16-byte aligned, never dereferenced: validation fails first, or no token is launched
Q = ctypes.c_void_p(8192)

ORDER = ("x", "y", "batch", "seqlen", "heads", "d", "dtype", "xb", "xt", "yb", "yt", "rcos", "rsin", "rcs", "rss", "sro", "rdim",
         "rint", "conj", "off", "offs", "cu", "total", "maxs")
# a valid padded call: (2, 5, 4, 64) bf16, dense, rotary_dim 32
BASE = dict(x=P, y=Q, batch=2, seqlen=5, heads=4, d=64, dtype=2, xb=5 * 256, xt=256, yb=5 * 256, yt=256, rcos=P, rsin=P, rcs=16,
            rss=16, sro=8, rdim=32, rint=0, conj=0, off=0, offs=None, cu=None, total=0, maxs=0)
PACKED = dict(seqlen=0, cu=P, total=9, maxs=5, xb=0, yb=0)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE)
    a.update(kw)
    rc = ext._lib.fa_rotary_apply(*[a[n] for n in ORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbol():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bfa_rotary_apply\s*\(", src)
    assert hasattr(ctypes.CDLL(ext.LIBRARY_PATH), "fa_rotary_apply")
    assert "fa_rotary_apply" in ext.EXPORTED_C_SYMBOLS
    assert [f for f, _ in ext._SIGNATURES["fa_rotary_apply"][1]][11:18] == [f for f, _ in ext._ROTARY]   # the group, verbatim


BAD = [
    (dict(dtype=0), "dtype"), (dict(dtype=3), "dtype"),
    (dict(d=0), "head_dim"), (dict(d=60), "head_dim"), (dict(d=264), "head_dim"),
    (dict(batch=0), "batch"), (dict(batch=65536), "batch"),
    (dict(heads=0), "heads"), (dict(heads=-1), "heads"), (dict(heads=2 ** 31), "heads"),
    (dict(seqlen=-1), "seqlen"), (dict(seqlen=2 ** 31), "seqlen"),
    (dict(x=None), "null tensor pointer"), (dict(y=None), "null tensor pointer"),
    (dict(x=ctypes.c_void_p(4104)), "16-byte aligned"), (dict(y=ctypes.c_void_p(8194)), "16-byte aligned"),
    (dict(offs=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(PACKED, cu=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(xt=248), "token strides"), (dict(yt=0), "token strides"), (dict(xt=-256), "token strides"), (dict(yt=2 ** 31 + 8), "token strides"),
    (dict(xb=4 * 256 + 248), "batch strides"), (dict(yb=0), "batch strides"), (dict(xb=-8), "batch strides"),
    (dict(xt=260, xb=5 * 260), "multiple of 8"), (dict(yt=257, yb=2000), "multiple of 8"), (dict(xb=5 * 256 + 4), "multiple of 8"),
    (dict(y=P, yt=512, yb=5 * 512), "equal strides"), (dict(y=P, yb=6 * 256), "equal strides"),
    (dict(rcos=None), "both be given"), (dict(rsin=None), "both be given"),
    (dict(rcos=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(rsin=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(rdim=0), "rotary_dim"), (dict(rdim=8), "rotary_dim"), (dict(rdim=24), "rotary_dim"), (dict(rdim=80), "rotary_dim"),
    (dict(rcs=15), "row strides"), (dict(rss=8), "row strides"), (dict(rcs=-16), "row strides"),
    (dict(rcs=17), "even"), (dict(rss=19), "even"),
    (dict(sro=0), "seqlen_ro"), (dict(sro=-4), "seqlen_ro"),
    (dict(off=2 ** 31), "seqlen_offset"), (dict(off=-2 ** 31), "seqlen_offset"),
    # the packed form
    (dict(PACKED, total=-1), "total"), (dict(PACKED, total=2 ** 31), "total"),
    (dict(PACKED, maxs=-1), "max_seqlen"), (dict(PACKED, maxs=10), "max_seqlen"),
    (dict(PACKED, seqlen=5), "seqlen must be 0"),
    (dict(total=9), "without cu_seqlens"), (dict(maxs=5), "without cu_seqlens"),
]


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_rule_is_checked_before_any_hip_call(kw, what):
    rc, msg = _call(**kw)    # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == INVALID_ARGUMENT, (kw, msg)
    assert what in msg and msg.startswith("fa_rotary_apply:"), (kw, msg)


def test_the_first_broken_rule_names_itself():
    """two broken rules: the one that comes first in the header's list answers"""
    for kw, what in ((dict(dtype=0, d=60), "dtype"), (dict(d=60, batch=0), "head_dim"), (dict(batch=0, x=None), "batch"),
                     (dict(x=None, rdim=8), "null tensor pointer"), (dict(xt=248, rdim=8), "token strides"),
                     (dict(rdim=8, sro=0), "rotary_dim"), (dict(sro=0, off=2 ** 31), "seqlen_ro")):
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and what in msg, (kw, msg)


def test_a_call_without_tokens_is_ok_without_a_launch():
    """valid arguments and no token: FA_OK, and nothing was launched (there is no device here to launch on)"""
    for kw in (dict(seqlen=0), dict(seqlen=0, xb=0, yb=0, batch=1), dict(PACKED, maxs=0), dict(PACKED, total=0, maxs=0),
               dict(seqlen=0, y=P), dict(seqlen=0, off=2 ** 31 - 1, offs=P), dict(seqlen=0, off=-(2 ** 31) + 1)):
        rc, msg = _call(**kw)
        assert rc == 0, (kw, msg)
    # the packed form does not look at the batch strides, the padded form with batch = 1 neither
    assert _call(**dict(PACKED, maxs=0, xb=3, yb=-7))[0] == 0
    assert _call(seqlen=0, batch=1, xb=3, yb=-7)[0] == 0
    # validation still comes first
    assert _call(seqlen=0, rdim=8)[0] == INVALID_ARGUMENT


class FakeCuda(torch.Tensor):   # the wrappers' checks run before anything touches the device
    @property
    def is_cuda(self):
        return True


def _fake(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)


def test_shim_rejections():
    import flashattention_lab_cuda as ext

    x, cos = _fake(2, 5, 4, 64), _fake(8, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.rotary_apply(torch.zeros((2, 5, 4, 64), dtype=torch.bfloat16), cos, cos)
    with pytest.raises(RuntimeError, match="16-bit dtype"):                         # fp32 is refused, as the KV-cache calls refuse it
        ext.rotary_apply(_fake(2, 5, 4, 64, dtype=torch.float32), cos, cos)
    with pytest.raises(RuntimeError, match="must be 4-D"):
        ext.rotary_apply(_fake(5, 4, 64), cos, cos)
    with pytest.raises(ValueError, match="packed"):
        ext.rotary_apply(x, cos, cos, cu_seqlens=torch.zeros(3, dtype=torch.int32), max_seqlen=5)
    with pytest.raises(ValueError, match="needs max_seqlen"):
        ext.rotary_apply(_fake(9, 4, 64), cos, cos, cu_seqlens=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs cu_seqlens"):
        ext.rotary_apply(x, cos, cos, max_seqlen=5)
    with pytest.raises(NotImplementedError, match="cu_seqlens of dtype"):
        ext.rotary_apply(_fake(9, 4, 64), cos, cos, cu_seqlens=torch.zeros(3, dtype=torch.int64), max_seqlen=5)
    with pytest.raises(ValueError, match=r"max_seqlen = 10 must lie in \[0, total = 9\]"):
        ext.rotary_apply(_fake(9, 4, 64), cos, cos, cu_seqlens=torch.zeros(3, dtype=torch.int32), max_seqlen=10)
    with pytest.raises(RuntimeError, match="head dim"):
        ext.rotary_apply(_fake(2, 5, 4, 60), cos, cos)
    for bad in (torch.zeros((8, 16)), _fake(8), _fake(8, 16, 1), [1.0]):
        with pytest.raises(RuntimeError, match=r"must be a \(seqlen_ro, rotary_dim / 2\) tensor"):
            ext.rotary_apply(x, bad, bad)
    with pytest.raises(RuntimeError, match="of one shape"):
        ext.rotary_apply(x, cos, _fake(8, 8))
    for half in (4, 12, 40):
        with pytest.raises(RuntimeError, match="multiple of 16 in"):
            ext.rotary_apply(x, _fake(8, half), _fake(8, half))
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="seqlen_offsets must be an int"):
            ext.rotary_apply(x, cos, cos, seqlen_offsets=bad)
    with pytest.raises(ValueError, match="2\\^31"):
        ext.rotary_apply(x, cos, cos, seqlen_offsets=2 ** 31)
    with pytest.raises(TypeError):
        ext.rotary_apply(x, cos, cos, seqlen_offsets=1.5)
    for bad in (_fake(2, 5, 4, 32), _fake(2, 5, 4, 64, dtype=torch.float16), [0]):
        with pytest.raises(RuntimeError, match="out must be a tensor of x's shape"):
            ext.rotary_apply(x, cos, cos, out=bad)
    # layouts the kernel cannot address raise for x and for out alike: nothing is copied
    heads_apart = _fake(2, 4, 5, 64).transpose(1, 2)                      # (2, 5, 4, 64) with the heads at stride 5 * 64
    odd_stride = _fake(2, 5, 4, 68)[..., :64]                             # head stride 68
    last_strided = _fake(2, 5, 4, 128)[..., ::2]
    misaligned = _fake(2 * 5 * 4 * 64 + 8)[4:-4].view(2, 5, 4, 64)        # 8 bytes off a 16-byte boundary
    overlapping = _fake(2, 5, 4, 64).as_strided((2, 5, 4, 64), (256, 256, 64, 1))
    for bad in (heads_apart, odd_stride, last_strided, misaligned, overlapping):
        with pytest.raises(ValueError, match="never copied"):
            ext.rotary_apply(bad, cos, cos)
        with pytest.raises(ValueError, match="never copied"):
            ext.rotary_apply(x, cos, cos, out=bad)
    # no tokens: returns out without a call
    empty = _fake(2, 0, 4, 64)
    assert ext.rotary_apply(empty, cos, cos, out=empty) is empty
    assert ext.rotary_apply(empty, cos, cos).shape == (2, 0, 4, 64)


def test_module_rejections():
    from common.rotary import apply_rotary_emb, apply_rotary_emb_qkv_

    cos = _fake(8, 16)
    with pytest.raises(RuntimeError, match="16-bit dtype"):
        apply_rotary_emb(_fake(2, 5, 4, 64, dtype=torch.float32), cos, cos)
    with pytest.raises(ValueError, match="never copied"):
        apply_rotary_emb(_fake(2, 4, 5, 64).transpose(1, 2), cos, cos, inplace=True)
    for bad in (_fake(2, 5, 2, 4, 64), _fake(2, 5, 4, 64), _fake(2, 5, 3, 64)):
        with pytest.raises(ValueError, match=r"qkv must be \(B, S, 3, H, d\)"):
            apply_rotary_emb_qkv_(bad, cos, cos)
    cu = torch.zeros(3, dtype=torch.int32)
    for bad in (_fake(2, 5, 3, 4, 64), _fake(9, 2, 4, 64)):
        with pytest.raises(ValueError, match=r"qkv must be \(total, 3, H, d\)"):
            apply_rotary_emb_qkv_(bad, cos, cos, cu_seqlens=cu, max_seqlen=5)
    for bad, hq in ((_fake(2, 5, 7, 64), 4), (_fake(2, 5, 4, 64), 4), (_fake(2, 5, 3, 6, 64), 4), (_fake(2, 5, 6, 64), 0)):
        with pytest.raises(ValueError, match=r"qkv must be \(B, S, H_q \+ 2 H_kv, d\)"):
            apply_rotary_emb_qkv_(bad, cos, cos, num_heads_q=hq)
    with pytest.raises(ValueError, match=r"qkv must be \(total, H_q \+ 2 H_kv, d\)"):
        apply_rotary_emb_qkv_(_fake(2, 5, 6, 64), cos, cos, cu_seqlens=cu, max_seqlen=5, num_heads_q=4)
    with pytest.raises(ValueError, match="adjacent in memory"):           # q, k, v planes that are not one after the other
        apply_rotary_emb_qkv_(_fake(2, 5, 4, 3, 64).transpose(2, 3), cos, cos)


# ---- the thread-to-chunk map: each rotated element is written exactly once, by a unit that read both members of its pair, and no
# other unit reads or writes either member.  With y == x that excludes every read-after-write and write-after-write between
# threads: the in-place proof.
SHAPES = sorted({(c["d"], c["rdim"]) for c in CASES})


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("d,rdim", SHAPES)
def test_unit_map_owns_whole_pairs(d, rdim, interleaved):
    partner = {}
    for a, b in pairs(rdim, interleaved):
        partner[a], partner[b] = b, a
    for inplace in (False, True):
        n = unit_count(d, rdim, interleaved, inplace)
        writers, readers = {}, {}
        for u in range(n):
            kind, reads, writes = unit_model(u, d, rdim, interleaved, inplace)
            assert len(reads) == len(set(reads)) and sorted(reads) == sorted(writes)        # every element read once, then written
            for c in reads:
                for e in range(8 * c, 8 * c + 8):
                    readers.setdefault(e, []).append(u)
            for c in writes:
                for e in range(8 * c, 8 * c + 8):
                    writers.setdefault(e, []).append(u)
                    assert (e < rdim) == (kind == "rotate")
        for e in range(rdim):
            assert len(writers[e]) == 1, (e, writers[e])                    # written exactly once
            u = writers[e][0]
            assert readers[e] == [u] and readers[partner[e]] == [u]         # its writer, and nobody else, read both members
            assert writers[partner[e]] == [u]
        for e in range(rdim, d):                                            # pass-through: one copy, or untouched in place
            assert writers.get(e, []) == readers.get(e, []) and len(writers.get(e, [])) == (0 if inplace else 1)
        assert max(8 * c + 7 for u in range(n) for c in unit_model(u, d, rdim, interleaved, inplace)[1]) < d
    # the table words a unit loads are 4-byte aligned entries of one row
    for u in range(unit_count(d, rdim, interleaved, True)):
        first = 4 * u if interleaved else 8 * u
        assert first % 2 == 0 and first + (4 if interleaved else 8) <= rdim // 2


def test_packed_clamp_keeps_every_span_inside_the_tensor():
    total, mx = 11, 6
    vals = (-5, 0, 3, 6, 11, 12, 2 ** 31 - 1, -2 ** 31)
    for c0, c1 in itertools.product(vals, vals):
        start, n = span([c0, c1], 0, total, mx)
        assert 0 <= start <= total and 0 <= n <= mx and start + n <= total
    assert span([2, 7], 0, total, mx) == (2, 5) and span([7, 2], 0, total, mx) == (7, 0) and span([3, 30], 0, total, mx) == (3, 6)


def test_positions_are_formed_without_wrapping():
    """a host offset and a device offset near 2^31 each: the 64-bit sum is far outside the tables, a 32-bit sum would be inside"""
    off, dev = 2 ** 31 - 1, 2 ** 31 - 1
    pos = positions(off + dev, 4)
    assert all(p >= SEQLEN_RO for p in pos)
    wrapped = [((p + 2 ** 31) % 2 ** 32) - 2 ** 31 for p in pos]
    assert any(0 <= p < SEQLEN_RO for p in wrapped)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_fp32_rotation_rounds_as_the_fp64_reference_on_the_gpu_cases(idx):
    """The GPU test allows the kernel's rounding to differ from the reference's on 1 element in 10^4; on these inputs an fp32
    evaluation (plain, and with the second product fused into the sum) does not differ at all, for either sign of sin."""
    r = case_inputs(idx)
    x, dtype = r["x"], r["dtype"]
    for conj in (False, True):
        exact, rotated = reference64(x, r["cos"], r["sin"], r["pos0"], r["inter"], conj)
        want = round_once(exact, dtype)
        c32, s32 = r["cos"].float(), (-r["sin"] if conj else r["sin"]).float()
        for bb in range(BATCH):
            keep = torch.nonzero(rotated[bb]).flatten()
            if keep.numel() == 0:
                assert torch.equal(want[bb].view(torch.int16), x[bb].view(torch.int16))
                continue
            rows = torch.tensor(positions(r["pos0"][bb], x.shape[1]))[keep]
            xf = x[bb, keep].float()
            plain, fused = xf.clone(), xf.clone()
            for j, (a, b) in enumerate(pairs(r["rdim"], r["inter"])):
                cj, sj = c32[rows, j].view(-1, 1), s32[rows, j].view(-1, 1)
                plain[:, :, a] = xf[:, :, a] * cj - xf[:, :, b] * sj
                plain[:, :, b] = xf[:, :, a] * sj + xf[:, :, b] * cj
                fused[:, :, a] = torch.addcmul(xf[:, :, a] * cj, xf[:, :, b], -sj)
                fused[:, :, b] = torch.addcmul(xf[:, :, a] * sj, xf[:, :, b], cj)
            assert torch.equal(plain.to(dtype).view(torch.int16), want[bb, keep].view(torch.int16))
            assert torch.equal(fused.to(dtype).view(torch.int16), want[bb, keep].view(torch.int16))
