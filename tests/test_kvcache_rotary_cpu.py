"""CPU: rotary embedding in KV-cache decoding (include/fa_mi355x.h: fa_ex_forward_kvcache_rotary) — declared, exported, every
host-side validation before any HIP call (the seqlen_ro bound that replaces a device check at its edge), null tables equal to
fa_ex_forward_kvcache_paged, the Python wrappers' checks, models of the kernels' chunk addressing and of the position rule, and
the check that on the GPU tests' own inputs an fp32 evaluation of the rotation rounds exactly as the fp64 reference does."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from tests.kvcache_rotary_ref import CASES, case_id, case_inputs, clamps, pairs, rotate64, round_once, tables
from tests.test_kvcache_cpu import BAD, BASE
from tests.test_kvcache_paged_cpu import NONE as PNONE
from tests.test_kvcache_paged_cpu import PAGED, PORDER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
INVALID_ARGUMENT = -1
P = ctypes.c_void_p(4096)   # a non-null, aligned address: never dereferenced when validation fails

# the arguments fa_ex_forward_kvcache_rotary adds, between cache_leftpad and the workspace
EXTRA = ("rcos", "rsin", "rcs", "rss", "sro", "rdim", "rint")
NONE = dict(rcos=None, rsin=None, rcs=0, rss=0, sro=0, rdim=0, rint=0)
RORDER = PORDER[:PORDER.index("ws")] + EXTRA + ("ws", "wsb")
# BASE has d = 64, cache_len = 64, seqlen_q = seqlen_new = 1: 64 table rows are exactly enough
ROT = dict(rcos=P, rsin=P, rcs=32, rss=32, sro=64, rdim=64, rint=1)


def _call(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **PNONE, **NONE)
    a.update(kw)
    rc = ext._lib.fa_ex_forward_kvcache_rotary(*[a[n] for n in RORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def _paged(**kw):
    import flashattention_lab_cuda as ext

    a = dict(BASE, **PNONE)
    a.update(kw)
    rc = ext._lib.fa_ex_forward_kvcache_paged(*[a[n] for n in PORDER], None)
    return rc, ext._lib.fa_last_error().decode()


def test_header_declares_and_library_exports_the_symbol():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bfa_ex_forward_kvcache_rotary\s*\(", src)
    assert hasattr(ctypes.CDLL(ext.LIBRARY_PATH), "fa_ex_forward_kvcache_rotary")
    assert "fa_ex_forward_kvcache_rotary" in ext.EXPORTED_C_SYMBOLS


@pytest.mark.parametrize("kw,what", BAD, ids=[str(i) for i in range(len(BAD))])
def test_null_tables_answer_as_the_paged_entry_point(kw, what):
    rc, msg = _call(**kw)
    rc0, msg0 = _paged(**kw)
    assert rc == rc0 == INVALID_ARGUMENT and what in msg
    assert msg == msg0.replace("fa_ex_forward_kvcache_paged:", "fa_ex_forward_kvcache_rotary:")


def test_null_tables_reach_the_null_pointer_check():
    for kw in (dict(), dict(PAGED, cap=0), dict(bidx=P, bcache=2, leftpad=P)):
        rc, msg = _call(**kw, o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)


ROT_BAD = [
    (dict(rsin=None), "given together"), (dict(rcos=None), "given together"),
    (dict(rdim=0), "rotary_dim"), (dict(rdim=8), "rotary_dim"), (dict(rdim=24), "rotary_dim"), (dict(rdim=80), "rotary_dim"),
    (dict(rdim=-16), "rotary_dim"), (dict(rdim=72), "rotary_dim"),
    (dict(sro=63), "seqlen_ro"), (dict(sro=0), "seqlen_ro"), (dict(sro=-1), "seqlen_ro"),
    (dict(rcs=31), "row strides"), (dict(rss=16), "row strides"), (dict(rcs=0), "row strides"), (dict(rss=-32), "row strides"),
    (dict(rcs=33), "even"), (dict(rss=35), "even"),
    (dict(rcos=ctypes.c_void_p(4098)), "4-byte aligned"), (dict(rsin=ctypes.c_void_p(4097)), "4-byte aligned"),
    (dict(nnew=0, kn=None, vn=None, knb=0, knt=0, vnb=0, vnt=0), "rotary needs"), (dict(seqlens=None, nnew=0), "rotary needs"),
]


@pytest.mark.parametrize("kw,what", ROT_BAD, ids=[str(i) for i in range(len(ROT_BAD))])
def test_rotary_arguments_are_rejected_before_any_hip_call(kw, what):
    rc, msg = _call(**dict(ROT, **kw))   # no HIP call can have happened: there is no GPU here, and the pointers are fake
    assert rc == INVALID_ARGUMENT, (kw, msg)
    assert what in msg and msg.startswith("fa_ex_forward_kvcache_rotary:"), (kw, msg)


def test_rotary_integers_must_be_zero_without_tables():
    for kw in (dict(rcs=32), dict(rss=32), dict(sro=64), dict(rdim=64), dict(rint=1)):
        rc, msg = _call(**kw)
        assert rc == INVALID_ARGUMENT and "without rotary_cos" in msg, (kw, msg)


def test_valid_rotary_arguments_reach_the_null_pointer_check():
    for kw in (dict(), dict(rint=0), dict(rdim=16, rcs=8, rss=8), dict(rdim=32, rcs=16, rss=40), dict(rcs=2 ** 20, sro=2 ** 30),
               dict(causal=1), dict(wl=3, wr=0), dict(wl=2 ** 40), dict(leftpad=P), dict(bidx=P, bcache=3)):
        rc, msg = _call(**dict(ROT, **kw), o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)


def test_seqlen_ro_bound_at_its_edge():
    """seqlen_ro >= capacity + max(0, seqlen_q - seqlen_new): equal is accepted, one less refused"""
    contiguous = dict()                                                     # capacity 64, Nq = N_new = 1: 64
    paged = dict(PAGED, cap=0)                                              # capacity 4 * 16 = 64 (cache_len ignored): 64
    paged_big = dict(PAGED, cap=10 ** 6, mb=6, trs=6)                       # capacity 96, whatever cache_len says
    longer_q = dict(nq=5, qb=5 * 512)                                       # 64 + (5 - 1) = 68
    longer_q_paged = dict(PAGED, cap=0, nq=7, qb=7 * 512, nnew=3, knb=3 * 128, vnb=3 * 128)   # 64 + (7 - 3) = 68
    more_new = dict(nnew=4, knb=4 * 128, vnb=4 * 128)                       # Nq < N_new: 64
    for kw, need in ((contiguous, 64), (paged, 64), (paged_big, 96), (longer_q, 68), (longer_q_paged, 68), (more_new, 64)):
        rc, msg = _call(**dict(ROT, **kw, sro=need), o=None)
        assert rc == INVALID_ARGUMENT and "null tensor pointer" in msg, (kw, msg)
        rc, msg = _call(**dict(ROT, **kw, sro=need - 1), o=None)
        assert rc == INVALID_ARGUMENT and "seqlen_ro" in msg and f"= {need}" in msg, (kw, msg)


def test_python_wrapper_rejections():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_with_kvcache

    bf = torch.bfloat16
    q = torch.zeros((2, 1, 4, 64), dtype=bf)
    kc = torch.zeros((2, 16, 2, 64), dtype=bf)
    kn = torch.zeros((2, 1, 2, 64), dtype=bf)
    lens = torch.zeros(2, dtype=torch.int32)
    # a table of another dtype (or no tensor at all): refused at the top of flash_attn_with_kvcache, on any device
    for name in ("rotary_cos", "rotary_sin"):
        for bad in (torch.zeros(1), torch.zeros((16, 32)), torch.zeros((16, 32), dtype=torch.float16), [1.0], 1.0):
            with pytest.raises(NotImplementedError, match=name + r" of dtype .* \(q's dtype expected\)"):
                flash_attn_with_kvcache(q, kc, kc, kn, kn, **{name: bad}, cache_seqlens=lens)

    class FakeCuda(torch.Tensor):   # the wrapper's checks run before anything touches the device
        @property
        def is_cuda(self):
            return True

    fq, fk, fn, fl = (t.as_subclass(FakeCuda) for t in (q, kc, kn, lens))
    tab = lambda *shape: torch.zeros(shape, dtype=bf).as_subclass(FakeCuda)   # noqa: E731
    for fn_ in (lambda **kw: ext.ex_kvcache_forward(fq, fk, fk, fn, fn, fl, **kw),
                lambda **kw: flash_attn_with_kvcache(fq, fk, fk, fn, fn, cache_seqlens=fl, **kw)):
        with pytest.raises(RuntimeError, match="given together"):
            fn_(rotary_cos=tab(16, 32))
        with pytest.raises(RuntimeError, match="given together"):
            fn_(rotary_sin=tab(16, 32))
        for shape in ((16,), (16, 32, 1), (1, 16, 32)):
            with pytest.raises(RuntimeError, match=r"must be a \(seqlen_ro, rotary_dim / 2\) tensor"):
                fn_(rotary_cos=tab(*shape), rotary_sin=tab(*shape))
        with pytest.raises(RuntimeError, match="of one shape"):
            fn_(rotary_cos=tab(16, 32), rotary_sin=tab(16, 16))
        for half in (4, 12, 40):       # rotary_dim 8, 24 and 80 > d
            with pytest.raises(RuntimeError, match="multiple of 16 in"):
                fn_(rotary_cos=tab(16, half), rotary_sin=tab(16, half))
        with pytest.raises(RuntimeError, match="on q's device"):
            fn_(rotary_cos=tab(16, 32), rotary_sin=torch.zeros((16, 32), dtype=bf, device="meta"))
        with pytest.raises(RuntimeError, match="16 are needed"):          # too short a table: the capacity is 16
            fn_(rotary_cos=tab(15, 32), rotary_sin=tab(15, 32))
    with pytest.raises(RuntimeError, match="q's dtype"):                   # ex_kvcache_forward itself on a float32 table
        ext.ex_kvcache_forward(fq, fk, fk, fn, fn, fl, rotary_cos=torch.zeros((16, 32)), rotary_sin=torch.zeros((16, 32)))
    # rotary without the new tokens, or without cache_seqlens
    with pytest.raises(RuntimeError, match="need k, v"):
        ext.ex_kvcache_forward(fq, fk, fk, None, None, fl, rotary_cos=tab(16, 32), rotary_sin=tab(16, 32))
    with pytest.raises(RuntimeError, match="need k, v"):
        ext.ex_kvcache_forward(fq, fk, fk, fn, fn, None, rotary_cos=tab(16, 32), rotary_sin=tab(16, 32))
    # a paged call: the capacity is max_blocks_per_seq * page_block_size = 48, and Nq - N_new = 2 more rows
    fq3 = torch.zeros((2, 3, 4, 64), dtype=bf).as_subclass(FakeCuda)
    table = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="50 are needed"):
        ext.ex_kvcache_forward(fq3, fk, fk, fn, fn, fl, block_table=table, rotary_cos=tab(49, 32), rotary_sin=tab(49, 32))


# ---- model of the kernels' chunk addressing (csrc/fa_decode.hip: kv_rot_partner, kv_rotate_chunk)
def chunk_model(c, rotary_dim, interleaved):
    """What the lane that holds the 16-byte chunk c (head dims 8 c .. 8 c + 7, below rotary_dim) uses: (partner chunk or None,
    the table column of each of its 8 elements, for each element whether it is the x of its pair, else the y)."""
    col, half = 8 * c, rotary_dim // 2
    if interleaved:   # pairs (2 j, 2 j + 1) inside the chunk: entries 4 c .. 4 c + 3, element e is x when even
        return None, [(col >> 1) + e // 2 for e in range(8)], [e % 2 == 0 for e in range(8)]
    is_x = col < half
    j0 = col if is_x else col - half
    return (col + half) // 8 if is_x else (col - half) // 8, [j0 + e for e in range(8)], [is_x] * 8


def rotate_by_chunks(row, cos_row, sin_row, rotary_dim, interleaved):
    """row (d,) float64: out = own * cos + sgn * partner * sin, chunk by chunk as the kernels do"""
    out = row.clone()
    for c in range(rotary_dim // 8):
        partner, cols, is_x = chunk_model(c, rotary_dim, interleaved)
        for e in range(8):
            own = row[8 * c + e]
            if interleaved:
                par = row[8 * c + (e ^ 1)]           # the other element of the pair, in the same chunk
            else:
                par = row[8 * partner + e]
            sgn = -1.0 if is_x[e] else 1.0
            out[8 * c + e] = own * cos_row[cols[e]] + sgn * par * sin_row[cols[e]]
    return out


@pytest.mark.parametrize("d", [64, 96, 128, 256])
def test_chunk_addressing_model(d):
    g = torch.Generator().manual_seed(d)
    for rotary_dim, interleaved in itertools.product(sorted({16, (d // 2) // 16 * 16, d // 16 * 16}), (True, False)):
        cos, sin = tables(9, rotary_dim, torch.bfloat16)
        x = torch.randn((9, 1, d), generator=g).to(torch.bfloat16)
        want = rotate64(x, cos, sin, range(9), interleaved)
        for t in range(9):
            got = rotate_by_chunks(x[t, 0].double(), cos[t].double(), sin[t].double(), rotary_dim, interleaved)
            assert torch.equal(got, want[t, 0]), (rotary_dim, interleaved, t)
            assert torch.equal(got[rotary_dim:], x[t, 0].double()[rotary_dim:])
        # every chunk below rotary_dim has a partner below rotary_dim, the partner's partner is the chunk, columns stay in the table
        for c in range(rotary_dim // 8):
            partner, cols, is_x = chunk_model(c, rotary_dim, interleaved)
            assert all(0 <= j < rotary_dim // 2 for j in cols)
            assert cols[0] % 4 == 0          # the lane's first entry is 4-byte aligned in a row of 16-bit entries
            if not interleaved:
                assert 0 <= partner < rotary_dim // 8 and chunk_model(partner, rotary_dim, False)[0] == c
                assert chunk_model(partner, rotary_dim, False)[2][0] != is_x[0]
        # the pairs the chunks cover are exactly the documented ones
        seen = set()
        for c in range(rotary_dim // 8):
            partner, cols, is_x = chunk_model(c, rotary_dim, interleaved)
            for e in range(8):
                mine = 8 * c + e
                other = 8 * c + (e ^ 1) if interleaved else 8 * partner + e
                seen.add((cols[e], (mine, other) if is_x[e] else (other, mine)))
        assert seen == set(enumerate(pairs(rotary_dim, interleaved)))


def test_position_rule_stays_below_the_host_bound():
    """new key n at L_b - P_b + n, q token i at L_b - P_b + (i if causal or a window is given else 0): for every cache_seqlens
    and cache_leftpad value, clamped as the kernels clamp them, inside [0, capacity + max(0, Nq - N_new))"""
    cap = 12
    for nq, nnew in itertools.product((1, 2, 5), (1, 2, 4, 12)):
        bound = cap + max(0, nq - nnew)
        for sl, lp, per_token in itertools.product(range(-3, cap + 4), (None, *range(-2, cap + 3)), (False, True)):
            (L,), (Pb,) = clamps([sl], None if lp is None else [lp], cap, nnew)
            assert 0 <= Pb <= L <= cap - nnew
            lk = L + nnew - Pb
            kpos = [L - Pb + n for n in range(nnew)]
            qpos = [L - Pb + (i if per_token else 0) for i in range(nq)]
            assert kpos == list(range(lk - nnew, lk))          # the new tokens' indices in the sequence's key coordinates
            assert all(0 <= x < cap for x in kpos) and all(0 <= x < bound for x in qpos)
            if per_token and nq == nnew:                       # q token i sits on the diagonal: the position of new key i
                assert qpos == [i + lk - nq for i in range(nq)] == kpos
    # the bound is tight: the longest clamped sequence with Nq > N_new reaches its last row
    (L,), (Pb,) = clamps([10 ** 6], None, cap, 1)
    assert L - Pb + (5 - 1) == cap + (5 - 1) - 1


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_fp32_rotation_rounds_as_the_fp64_reference_on_the_gpu_cases(idx):
    """The GPU test allows the kernel's rounding to differ from the reference's on 1 element in 10^4; on these inputs an fp32
    evaluation (plain, and with the second product fused into the sum) does not differ at all."""
    r = case_inputs(idx)
    dtype, cap, nnew, nq = r["dtype"], r["cap"], r["nnew"], r["nq"]
    L, Pb = clamps(r["seqlens"], r["leftpad"], cap, nnew)
    per_token = r["causal"] or r["window"] != (-1, -1)
    c32, s32 = r["cos"].float(), r["sin"].float()
    for x, npos in ((r["kn"], nnew), (r["q"], nq)):
        for bb in range(r["b"]):
            first = L[bb] - Pb[bb]
            pos = [first + n for n in range(npos)] if x is r["kn"] else [first + (i if per_token else 0) for i in range(npos)]
            assert max(pos) < r["cos"].shape[0]
            want = round_once(rotate64(x[bb], r["cos"], r["sin"], pos, r["inter"]), dtype)
            xf = x[bb].float()
            plain, fused = xf.clone(), xf.clone()
            rows = torch.tensor(pos)
            for j, (a, b) in enumerate(pairs(r["rdim"], r["inter"])):
                cj, sj = c32[rows, j].view(-1, 1), s32[rows, j].view(-1, 1)
                plain[:, :, a] = xf[:, :, a] * cj - xf[:, :, b] * sj
                plain[:, :, b] = xf[:, :, a] * sj + xf[:, :, b] * cj
                fused[:, :, a] = torch.addcmul(xf[:, :, a] * cj, xf[:, :, b], -sj)
                fused[:, :, b] = torch.addcmul(xf[:, :, a] * sj, xf[:, :, b], cj)
            assert torch.equal(plain.to(dtype).view(torch.int16), want.view(torch.int16))
            assert torch.equal(fused.to(dtype).view(torch.int16), want.view(torch.int16))
