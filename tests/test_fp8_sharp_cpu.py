"""CPU: the proofs behind tests/test_fp8_sharp_gpu.py.  The workspace of every d = 128 case is made by the
transcriptions of tests/fp8_ref.py alone (expected_ws), so nothing here needs a GPU:

  * the baseline without rounding is the reference (1e-10), and on the "growing" input its own trace shows the lazy rescale at work;
  * the transcriptions agree with the oracle's quantisers (scales and unrotated codes exactly; rotated codes within one e4m3 step:
    the oracle rotates by a matrix product, the kernel by a butterfly);
  * the v8t decoder inverts an encoder written from the kernel's store indices;
  * the workspace layout is consistent at every table shape;
  * the near-tie counts of the chosen seeds stay within the cap of 8 per tensor;
  * every mutant fails the sharp bar on a case where it changes the result, while o x 1.2, o + 0.05 and lse + 1.5e-2 pass today's
    bars (tests/test_fp8_gpu.py: 3e-2 / 8e-2 on o, 2e-2 on lse against oracle.fp8_attention) on every all-e4m3 unit-normal case."""
import functools

import pytest
import torch

from oracle import attention_oracle as orc
from tests import fp8_cases as fc
from tests import fp8_ref as fr

IDS = [fc.case_id(c, i) for i, c in enumerate(fc.CASES)]


@functools.lru_cache(maxsize=None)
def _case(i):
    """(call, ws by the transcriptions, reference, baseline rounded as the kernel returns it) of case i, computed once"""
    call = fc.build_call(fc.CASES[i], i)
    ws = fr.expected_ws(call)
    return call, ws, fr.reference(ws, call), fr.rounded(fr.baseline(ws, call), call["dtype"])


def test_the_tables_are_within_their_caps_and_cover_every_pair():
    import itertools
    for cases, axes, cap in ((fc.CASES, fc.AXES, fc.MAX_CASES), (fc.RT_CASES, fc.RT_AXES, fc.MAX_RT_CASES)):
        assert len(cases) <= cap
        for a, b in itertools.combinations(axes, 2):
            assert {(c[a], c[b]) for c in cases} == set(itertools.product(axes[a], axes[b]))
    assert fc.CASES == fc.generate(fc.AXES, fc.SEED)          # a fixed seed: the same table everywhere


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_the_baseline_without_rounding_is_the_reference(i):
    call, ws, ref, _base = _case(i)
    b = fr.baseline(ws, call, compute=torch.float64, rounding=False)
    assert torch.isfinite(ref.o).all() and torch.isfinite(ref.lse).all()
    assert (b.o - ref.o).abs().max().item() <= 1e-10 and (b.lse - ref.lse).abs().max().item() <= 1e-10


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_the_baseline_itself_is_inside_the_bar(i):
    """the rounded baseline put in the kernel's place passes (ratio 1 by construction) and has the reference's -inf / NaN pattern"""
    call, _ws, ref, base = _case(i)
    bad, ratio = fr.tiled_sharp_bar(base, ref, base, call["dtype"])
    assert not bad and all(r <= 1.0 for r in ratio.values())
    assert torch.isfinite(base.o.float()).all() and torch.isfinite(base.lse).all()


def test_the_growing_input_exercises_the_lazy_rescale():
    """on the baseline's own trace: some wave rescales at least three times, and at some tile after the first some wave keeps a row
    on a stale max (its own max grew, by no more than 2^8) while another wave of the same launch moves"""
    most, stale_beside_move = 0, False
    for i, c in enumerate(fc.CASES):
        if c["input"] != "growing":
            continue
        call, ws, _ref, _base = _case(i)
        trace = []
        fr.baseline(ws, call, trace=trace)
        count = {}
        for kernel, t, r0, moved, stale in trace:
            w = moved[:, ::32]                                         # one flag per wave
            count[(kernel, r0)] = count.get((kernel, r0), 0) + w.to(torch.int64)
            if t > 0 and bool(stale.any()) and bool(moved.any()):
                stale_beside_move = True
        most = max([most] + [int(v.max()) for v in count.values()])
    assert most >= 3, most
    assert stale_beside_move


def test_normal_inputs_rescale_on_the_first_tile_only():
    """the reason the growing input exists"""
    for i, c in enumerate(fc.CASES):
        if c["input"] == "normal":
            call, ws, _ref, _base = _case(i)
            trace = []
            fr.baseline(ws, call, trace=trace)
            assert not any(bool(moved.any()) for _k, t, _r0, moved, _s in trace if t > 0)
            return


# ---- the transcriptions against the oracle's quantisers

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,d", [(300, 128), (130, 40), (65, 64), (257, 256)])
def test_transcriptions_agree_with_the_oracle(n, d, dtype):
    g = torch.Generator().manual_seed(n + d)
    x = torch.randn((3, n, d), generator=g).to(dtype)
    q = fr.quantise(x, rot=False, kernel="roundtrip")
    oq, osc = orc.quantize_e4m3_blockwise(x, 64)
    assert torch.equal(q["scale"], osc) and torch.equal(q["codes"], fr.e4m3_code(oq))
    q2 = fr.quantise(x, rot=False, pow2=True, kernel="roundtrip")
    oq2, osc2 = orc.quantize_e4m3_blockwise_pow2(x, 64)
    assert torch.equal(q2["scale"], osc2) and torch.equal(q2["codes"], fr.e4m3_code(oq2))
    qv = fr.quantise_v(x)
    assert torch.equal(qv["codes"], q2["codes"]) and torch.equal(qv["scale"], q2["scale"])
    assert torch.equal(fr.rot_sign(d), orc.incoherent_signs(d))
    # the unrotated round trip: the oracle's, rounded to the dtype
    rt = fr.roundtrip(x, False)
    assert torch.equal(rt["out"], orc.fp8_roundtrip(x, x, x, 64, 64, rotate=False)[2].to(dtype))
    if d & (d - 1) == 0:
        for kernel in ("quant", "roundtrip") if d == 128 else ("roundtrip",):
            qr = fr.quantise(x, rot=True, kernel=kernel)
            orq, orsc = orc.quantize_e4m3_blockwise(orc.incoherent_rotate(x), 64)
            torch.testing.assert_close(qr["scale"], orsc, rtol=1e-5, atol=0)
            assert int(fr.code_steps(qr["codes"], fr.e4m3_code(orq)).max()) <= 1
            assert float((qr["codes"] != fr.e4m3_code(orq)).float().mean()) < 1e-3
        # and the butterfly is the rotation: fp64 both ways
        torch.testing.assert_close(fr.rotation64(x), orc.incoherent_rotate(x.double().float()).double(), rtol=0, atol=1e-5)
        torch.testing.assert_close(fr.inverse_rotation64(fr.rotation64(x)), x.double(), rtol=0, atol=1e-12)


# ---- the v8t layout

def _encode_v8t(codes, n):
    """(bh, n, 128) codes -> the v8t region, written from fp8_quant_v_kernel's store indices: block blk of 64 keys; key `key` of the
    block goes to position pos = 32 (key >> 5) + 16 ((wlo >> 2) & 1) + (wlo & 3) + 4 (wlo >> 3), wlo = key & 31, of the d row's 64
    bytes in `tr`; d row r of the block is stored at [tile blk / 2][r][64 (blk & 1) ..]; an odd block count zeroes the second half
    of the last tile"""
    bh = codes.shape[0]
    nb, ntile = (n + 63) // 64, (n + 127) // 128
    out = torch.full((bh, ntile, 128, 128), fr.SENTINEL, dtype=torch.uint8)
    for blk in range(nb):
        tr = torch.zeros((bh, 128, 64), dtype=torch.uint8)             # rows >= N were loaded as zeros: code 0
        for key in range(64):
            wlo = key & 31
            pos = 32 * (key >> 5) + 16 * ((wlo >> 2) & 1) + (wlo & 3) + 4 * (wlo >> 3)
            if blk * 64 + key < n:
                tr[:, :, pos] = codes[:, blk * 64 + key, :]
        out[:, blk >> 1, :, 64 * (blk & 1):64 * (blk & 1) + 64] = tr
        if (nb & 1) and blk == nb - 1:
            out[:, blk >> 1, :, 64:] = 0
    return out.reshape(-1)


@pytest.mark.parametrize("n", [64, 257, 300, 384])
def test_the_v8t_decoder_inverts_the_encoder(n):
    g = torch.Generator().manual_seed(n)
    codes = torch.randint(0, 256, (2, n, 128), generator=g, dtype=torch.uint8)
    region = _encode_v8t(codes, n)
    assert not bool((region == fr.SENTINEL).all()) and region.numel() == 2 * ((n + 127) // 128) * 128 * 128
    dec = fr.decode_v8t(region, 2, n)
    assert torch.equal(dec[:, :n], codes)
    assert bool((dec[:, n:] == 0).all())          # keys >= N, the second half of the last tile at odd nb included


# ---- the layout helper

@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_the_workspace_layout_is_consistent(direction):
    shapes = {(c["n"], 128, c["dtype"]) for c in fc.CASES} | {(c["n"], c["d"], c["dtype"]) for c in fc.RT_CASES}
    for n, d, dname in sorted(shapes):
        lay = fr.ws_layout(fc.BH, n, d, fc.DTYPES[dname], direction, plain_bytes=512)
        regions = sorted((o, s, name) for name, (o, s) in ((k, v) for k, v in lay.items() if k != "total"))
        end = 0
        for o, s, name in regions:
            assert o >= end, (name, n, d)                              # disjoint, in order
            end = o + s
        assert end <= lay["total"]
        for name in ("qt", "kt", "vt", "q8", "sq", "v8t", "plain"):    # where the code aligns: slabs, the e4m3 workspace, its scale and V^T parts
            if name in lay:
                assert lay[name][0] % 256 == 0, (name, n, d)
        if direction == "forward" and d == 128:
            assert lay["total"] - (lay["v8t"][0] + lay["v8t"][1]) == 256
            assert lay["k8"][0] == lay["q8"][0] + lay["q8"][1] and lay["sk"][0] == lay["sq"][0] + lay["sq"][1]
            assert lay["svexp"][0] == lay["sk"][0] + lay["sk"][1]
        assert fr.untouched(torch.zeros(lay["total"], dtype=torch.uint8), lay).numel() == lay["total"] - sum(s for _o, s, _n in regions)


# ---- near ties

def test_the_near_tie_counts_stay_within_the_cap():
    """by the transcription alone: at most 8 elements per tensor whose inexact quotient lies within 4 float ulps of an e4m3 midpoint"""
    worst = 0
    for i in range(len(fc.CASES)):
        call, ws, _ref, _base = _case(i)
        counts = [int(fr.near_ties(q).sum()) for q in ws["quant"]]
        if fr.vrows(call):
            counts.append(int(fr.near_ties(fr.roundtrip(call["v"][:, :fr.vrows(call)], False, pow2=fr.v_pow2(call))["q"]).sum()))
        for name in ("q", "k", "v"):       # the backward's round trips
            counts.append(int(fr.near_ties(fr.roundtrip(call[name], name != "v" and call["fp8_rot"] != 2, pow2=name == "v" and fr.v_pow2(call))["q"]).sum()))
        assert max(counts) <= 8, (fc.case_id(fc.CASES[i], i), counts)
        worst = max(worst, max(counts))
    for i, c in enumerate(fc.RT_CASES):
        call = fc.build_call(c, i)
        rot = c["d"] & (c["d"] - 1) == 0
        counts = [int(fr.near_ties(fr.roundtrip(call[name], rot and name != "v")["q"]).sum()) for name in ("q", "k", "v")]
        assert max(counts) <= 8, (fc.case_id(c, i), counts)
        worst = max(worst, max(counts))
    print(f"near ties: at most {worst} per tensor")


# ---- the mutants

def _old_model(call):
    """tests/test_fp8_gpu.py's _fp8_model on the call's own options"""
    e4 = fr.v_pow2(call)
    rot = call["fp8_rot"] != 2
    mo, mlse = orc.fp8_attention(call["q"], call["k"], call["v"], call["causal"], call["scale"], 64, 64, rotate=rot, p_e4m3=e4)
    if e4 and call["causal"]:
        m16, _ = orc.fp8_attention(call["q"], call["k"], call["v"], call["causal"], call["scale"], 64, 64, rotate=rot, p_e4m3=False, v_pow2=True)
        mo = torch.cat([m16[:, :256], mo[:, 256:]], dim=1)
    return mo, mlse


def _same_pattern(got, ref):
    return bool(torch.isfinite(got.o.float()).all()) and torch.equal(torch.isfinite(got.lse), torch.isfinite(ref.lse))


def test_every_mutant_fails_the_sharp_bar_and_three_pass_todays():
    table = {}
    for name in fr.MUTANTS:
        applies = fails = passes_old = e4_normal = e4_normal_old = e4_normal_fails = 0
        for i, c in enumerate(fc.CASES):
            call, ws, ref, base = _case(i)
            m = fr.mutant(ws, call, name)
            if m is None:
                continue
            got = fr.rounded(m, call["dtype"])
            exact = fr.rounded(ref, call["dtype"])
            if torch.equal(got.o, exact.o) and torch.equal(got.lse, exact.lse):
                continue                                               # the bug changes nothing here
            applies += 1
            bad, _ratio = fr.tiled_sharp_bar(got, ref, base, call["dtype"]) if _same_pattern(got, ref) else (["NaN / inf pattern"], {})
            fails += bool(bad)
            old = _same_pattern(got, ref) and fr.old_bars(got, *_old_model(call), call)
            passes_old += old
            if fr.v_pow2(call) and c["input"] == "normal":
                e4_normal += 1
                e4_normal_old += old
                e4_normal_fails += bool(bad)
        table[name] = (applies, fails, passes_old, e4_normal, e4_normal_old, e4_normal_fails)
        print(f"{name:30s} changes {applies:2d} cases: fails the sharp bar on {fails:2d}, passes today's bars on {passes_old:2d}")
    for name, (applies, fails, _old, _n, _o, _f) in table.items():
        assert applies > 0 and fails > 0, name
    for name in fr.MUTANTS[:3]:        # the finding: kept on record
        applies, fails, _old, e4n, e4n_old, e4n_fails = table[name]
        assert e4n > 0 and e4n_old == e4n and e4n_fails == e4n, (name, table[name])      # today's bars pass where the sharp bar fails
