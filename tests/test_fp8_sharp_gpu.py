"""GPU: the FA3 fp8 path cut at the caller's workspace (tests/fp8_ref.py, tests/fp8_cases.py; the proofs are in
tests/test_fp8_sharp_cpu.py).  Every call goes through the raw entry points with a workspace cut out of a larger byte buffer filled
with 0x7F — NaN as e4m3, 3.4e38 as a float scale or a 16-bit value — so that a stray read shows in o, and the pads, the 256-byte
tail and the bytes around the workspace can be checked afterwards.

  * quantisers, bit for bit: q8, k8, sq, sk, svexp, v8t (layout, permutation and the zeros past N included) and the V~ slab against
    the float32 transcriptions; an element may differ only where the transcription's quotient is a near tie (fp8_ref.compare_codes);
  * round trips (Q~, K~, V~ of the backward, and of the forward at d != 128): bit for bit, the rotated ones too — the derived bar
    |Q~ - Q~_64| <= eps/2 |Q~_64| + 2^-18 ||row|| is kept for the rows a near tie lets differ; at d = 128 the backward's Q~, K~ rotated
    in fp64 lie within (eps/2 + 2^-18) ||row|| of the forward's q8 sq, k8 sk;
  * attention on the quantised bytes: o and lse against fp8_ref.reference of the workspace as read back, at ex_full_ref.sharp_bar
    (factor 2) per tensor and per 256-row query tile, every value finite; the baseline's model of the e4m3 matrix instruction,
    which does not sum exactly, is held to the instruction itself on the rows that see a single key;
  * bit identities: fa3_forward(fp8 = 1) at d != 128 and fa3_backward(fp8 = 1) at every d have the bits of the fp8 = 0 call on the
    Q~, K~, V~ read back from their workspace (those kernels are under §9l-3's bar); every call twice gives the same bits."""
import contextlib
import functools

import pytest
import torch

import flashattention_lab_cuda as ext
from tests import fp8_cases as fc
from tests import fp8_ref as fr

pytestmark = pytest.mark.gpu
GUARD = 4096
MUTANT = None        # a name of fp8_ref.MUTANTS: that bug, rounded as the kernel returns it, takes the kernel's place in the attention test
IDS = [fc.case_id(c, i) for i, c in enumerate(fc.CASES)]
RT_IDS = [fc.case_id(c, i) for i, c in enumerate(fc.RT_CASES)]
ALL = [("d128", i) for i in range(len(fc.CASES))] + [("rt", i) for i in range(len(fc.RT_CASES))]
ALL_IDS = ["d128-" + s for s in IDS] + ["rt-" + s for s in RT_IDS]


@contextlib.contextmanager
def _options(call):
    ext.set_option("fp8_pv", call["fp8_pv"])
    ext.set_option("fp8_rot", call["fp8_rot"])
    try:
        yield
    finally:
        ext.set_option("fp8_pv", 0)
        ext.set_option("fp8_rot", 0)


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _buffer(device, nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), fr.SENTINEL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes):
    b = buf.cpu()
    return bool((b[:GUARD] == fr.SENTINEL).all()) and bool((b[GUARD + nbytes:] == fr.SENTINEL).all())


def _code(dtype):
    return {torch.float16: 1, torch.bfloat16: 2}[dtype]


def _forward(call, device, q, k, v, fp8):
    """(o, lse, workspace bytes on the CPU or None, guards intact) of one raw fa3_forward"""
    bh, n, d = q.shape
    nbytes = int(ext._lib.fa3_forward_workspace_bytes(bh, n, d, _code(call["dtype"]), 1)) if fp8 else 0
    buf, ws = _buffer(device, nbytes)
    o = torch.full_like(q, float("nan"))
    lse = torch.full((bh, n), float("nan"), dtype=torch.float32, device=device)
    with _options(call):
        rc = ext._lib.fa3_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), bh, n, d, _code(call["dtype"]),
                                  int(call["causal"]), float(call["scale"]), 64, 128, 2, int(fp8), ws.data_ptr() if fp8 else None, nbytes,
                                  _stream(device))
    assert rc == 0, ext._lib.fa_last_error().decode()
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), (ws.cpu() if fp8 else None), _guards_intact(buf, nbytes)


def _backward(call, device, q, k, v, o, do, lse, fp8, nbytes):
    """(dq, dk, dv, workspace bytes on the CPU, guards intact) of one raw fa3_backward with a workspace of exactly nbytes"""
    bh, n, d = q.shape
    buf, ws = _buffer(device, nbytes)
    dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
    with _options(call):
        rc = ext._lib.fa3_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                   dk.data_ptr(), dv.data_ptr(), bh, n, d, _code(call["dtype"]), int(call["causal"]), float(call["scale"]),
                                   64, 128, 2, int(fp8), ws.data_ptr(), nbytes, _stream(device))
    assert rc == 0, ext._lib.fa_last_error().decode()
    torch.cuda.synchronize()
    return dq.cpu(), dk.cpu(), dv.cpu(), ws.cpu(), _guards_intact(buf, nbytes)


def _call_of(kind, i):
    return fc.build_call((fc.CASES if kind == "d128" else fc.RT_CASES)[i], i)


@functools.lru_cache(maxsize=None)
def _fwd_run(kind, i, device):
    """the forward of a case, twice: dict(call, o, lse, ws, guards, again = the second call's (o, lse, ws))"""
    call = _call_of(kind, i)
    q, k, v = (call[x].to(device) for x in "qkv")
    o, lse, ws, guards = _forward(call, device, q, k, v, 1)
    o2, lse2, ws2, _g = _forward(call, device, q, k, v, 1)
    return dict(call=call, o=o, lse=lse, ws=ws, guards=guards, again=(o2, lse2, ws2))


def _slabs(ws, call, direction):
    """Q~, K~, V~ of a [Q~][K~][V~].. workspace"""
    bh, n, d, dt = call["bh"], call["n"], call["d"], call["dtype"]
    lay = fr.ws_layout(bh, n, d, dt, direction)
    return [ws[lay[x][0]:lay[x][0] + lay[x][1]].clone().view(dt).reshape(bh, n, d) for x in ("qt", "kt", "vt")]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _e4m3_step(q, n):
    """per element: one e4m3 step at the element's code, times its block scale (float64)"""
    val = fr.e4m3_value(q["codes"]).abs().double()
    return torch.exp2(torch.floor(torch.log2(val.clamp_min(2.0 ** -6))) - 3.0) * fr.per_row(q["scale"].double(), n)


def _check_roundtrip(got, x, rot, pow2, what):
    """a round-tripped tensor against the float32 transcription: bit for bit, rotated tensors included (the first run on the
    MI355X showed rsqrtf(d) correctly rounded and no contraction on the way back: profiles/fp8_sweep.md).  The near-tie rule:
    a row may differ only if it holds a near-tie element (fp8_ref.near_ties), at most 8 rows per tensor, and then stays inside the
    derived bar |x~ - x~_64| <= eps/2 |x~_64| + 2^-18 ||row|| plus one e4m3 step of each near-tie element (seen through the
    rotation: step / sqrt(d)).  Returns the number of elements whose bits differ."""
    rt = fr.roundtrip(x, rot, pow2)
    diff = _bits(got) != _bits(rt["out"])
    differ = int(diff.sum())
    if differ:
        n, d = x.shape[1], x.shape[2]
        near = fr.near_ties(rt["q"])
        rows = diff.any(-1)
        assert int(rows.sum()) <= 8 and not bool((rows & ~near.any(-1)).any()), \
            f"{what}: {differ} elements in {int(rows.sum())} rows differ from the transcription bit for bit, {int((rows & ~near.any(-1)).sum())} rows without a near tie"
        want = rt["out64"]
        slack = (near.double() * _e4m3_step(rt["q"], n)).sum(-1, keepdim=True) / (d ** 0.5 if rot else 1.0)
        bound = 0.5 * torch.finfo(x.dtype).eps * want.abs() + 2.0 ** -18 * want.norm(dim=-1, keepdim=True) + slack
        err = (got.double() - want).abs()
        assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements outside the derived bar, worst ratio {(err / bound).max().item():.3f}"
    return differ


# ---------------------------------------------------------------------------------------------------------------- sizes

def test_the_layout_helper_gives_the_librarys_workspace_sizes(device):
    shapes = {(c["n"], 128, c["dtype"]) for c in fc.CASES} | {(c["n"], c["d"], c["dtype"]) for c in fc.RT_CASES}
    for n, d, dname in sorted(shapes):
        dt = fc.DTYPES[dname]
        assert fr.ws_layout(fc.BH, n, d, dt, "forward")["total"] == int(ext._lib.fa3_forward_workspace_bytes(fc.BH, n, d, _code(dt), 1)), (n, d)
        plain = int(ext._lib.fa_backward_workspace_bytes(fc.BH, n, d, _code(dt)))
        assert fr.ws_layout(fc.BH, n, d, dt, "backward", plain)["total"] == int(ext._lib.fa3_backward_workspace_bytes(fc.BH, n, d, _code(dt), 1)), (n, d)


# ---------------------------------------------------------------------------------------------------------------- d = 128 forward

@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_quantisers_bit_for_bit(i, device):
    run = _fwd_run("d128", i, str(device))
    call, ws = run["call"], run["ws"]
    bh, n, d = call["bh"], call["n"], call["d"]
    lay = fr.ws_layout(bh, n, d, call["dtype"], "forward")
    assert run["guards"], "bytes around the workspace were written"
    assert bool((fr.untouched(ws, lay) == fr.SENTINEL).all()), "a pad or the 256-byte tail of the workspace was written"
    got, want = fr.parse_forward_ws(ws, call), fr.expected_ws(call)
    bad, near = [], {}
    for name, codes, q in (("q8", got["q8"], want["quant"][0]), ("k8", got["k8"], want["quant"][1])):
        b, near[name] = fr.compare_codes(codes, q, name)
        bad += b
    for name in ("sq", "sk", "svexp"):
        if not torch.equal(got[name].view(torch.int32), want[name].view(torch.int32)):
            bad.append(f"{name}: differs from the transcription as bits")
    if not torch.equal(got["v8"], want["v8"]):           # layout, permutation, the zeros of keys >= N (odd nb: half a tile of them)
        bad.append(f"v8t: {int((got['v8'] != want['v8']).sum())} bytes differ from the transcription")
    if fr.v_pow2(call):
        assert bool((got["v8"][:, n:] == 0).all())
    if not torch.equal(_bits(got["vt"]), _bits(want["vt"])):   # rows >= vrows: still the sentinel
        bad.append(f"V~ slab: {int((_bits(got['vt']) != _bits(want['vt'])).sum())} elements differ from the transcription (sentinel rows included)")
    print(f"{IDS[i]}: codes off the transcription {near}")
    assert not bad, bad


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_attention_on_the_quantised_bytes(i, device):
    run = _fwd_run("d128", i, str(device))
    call = run["call"]
    ws = fr.parse_forward_ws(run["ws"], call)
    ref = fr.reference(ws, call)
    base = fr.rounded(fr.baseline(ws, call), call["dtype"])
    got = fr._result(run["o"], run["lse"])
    if MUTANT is not None and fr.mutant(ws, call, MUTANT) is not None:
        got = fr.rounded(fr.mutant(ws, call, MUTANT), call["dtype"])
    assert bool(torch.isfinite(got.o.float()).all()) and bool(torch.isfinite(got.lse).all()), "NaN or inf in o or lse"
    bad, ratio = fr.tiled_sharp_bar(got, ref, base, call["dtype"])
    r16 = fr.rows16(call)
    kern = {k: ("fwd_fp8_kernel" if int(k.split("[")[1].split(":")[0]) < r16 else "fwd_fp8v_kernel") for k in ratio}
    print(f"{IDS[i]}: kernel / baseline error " + ", ".join(f"{k} ({kern[k]}) {v:.2f}" for k, v in ratio.items()))
    assert not bad, (bad, ratio)


CAUSAL = [i for i, c in enumerate(fc.CASES) if c["mask"] == "causal"]


@pytest.mark.parametrize("i", CAUSAL, ids=[IDS[i] for i in CAUSAL])
def test_the_matrix_instruction_model_on_single_key_rows(i, device):
    """Under the mask row 0 sees key 0 alone: p = 1, l = 1 and lse = fl(fl(sacc * f) * ln2f), so lse / (ln2f * f) is the raw
    score the two e4m3 matrix instructions gave, to the three float32 roundings in between (bound: 4 * 2^-24 relative).  It must be
    fp8_ref._mfma_f8's value — the measurement behind that model, kept as a test.  (The exact sum of the 128 products lies up to
    2.8 away at values near 1e5, where the bound is 0.05 at most.)"""
    run = _fwd_run("d128", i, str(device))
    call = run["call"]
    ws = fr.parse_forward_ws(run["ws"], call)
    q8, k8 = fr.e4m3_value(ws["q8"][:, :1]), fr.e4m3_value(ws["k8"][:, :1])
    want = fr._mfma_f8(q8, k8.transpose(1, 2), torch.float32, torch.zeros((call["bh"], 1, 1)), True).double().reshape(-1)
    exact = (q8.double() * k8.double()).sum(-1).reshape(-1)
    c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(fr.LOG2E_F, dtype=torch.float32)
    f = ((ws["sq"][:, 0] * c_log2) * ws["sk"][:, 0]).double()
    got = run["lse"][:, 0].double() / float(torch.tensor(fr.LN2_F, dtype=torch.float32)) / f
    print(f"{IDS[i]}: raw score of row 0: instruction {got.tolist()}, model {want.tolist()}, exact sum {exact.tolist()}")
    assert bool(((got - want).abs() <= 4 * 2.0 ** -24 * want.abs()).all()), (got, want, exact)


@pytest.mark.parametrize("i", range(len(fc.CASES)), ids=IDS)
def test_the_forward_twice_gives_the_same_bits(i, device):
    run = _fwd_run("d128", i, str(device))
    o2, lse2, ws2 = run["again"]
    assert torch.equal(_bits(run["o"]), _bits(o2)) and torch.equal(run["lse"].view(torch.int32), lse2.view(torch.int32))
    assert torch.equal(run["ws"], ws2)


# ---------------------------------------------------------------------------------------------------------------- other head dims, forward

@pytest.mark.parametrize("i", range(len(fc.RT_CASES)), ids=RT_IDS)
def test_forward_round_trip_and_bit_identity(i, device):
    run = _fwd_run("rt", i, str(device))
    call, ws = run["call"], run["ws"]
    d = call["d"]
    lay = fr.ws_layout(call["bh"], call["n"], d, call["dtype"], "forward")
    assert run["guards"] and bool((fr.untouched(ws, lay) == fr.SENTINEL).all())
    qt, kt, vt = _slabs(ws, call, "forward")
    rot = d & (d - 1) == 0
    differ = [_check_roundtrip(t, call[x], rot and x != "v", False, f"{x}~") for t, x in ((qt, "q"), (kt, "k"), (vt, "v"))]
    print(f"{RT_IDS[i]}: elements off the float32 transcription bit for bit (q~, k~, v~) {differ}")
    # the 16-bit kernels on the round-tripped tensors: the same bits
    o0, lse0, _ws, _g = _forward(call, device, qt.to(device), kt.to(device), vt.to(device), 0)
    assert torch.equal(_bits(run["o"]), _bits(o0)) and torch.equal(run["lse"].view(torch.int32), lse0.view(torch.int32))
    assert bool(torch.isfinite(run["o"].float()).all()) and bool(torch.isfinite(run["lse"]).all())
    o2, lse2, ws2 = run["again"]
    assert torch.equal(_bits(run["o"]), _bits(o2)) and torch.equal(run["lse"].view(torch.int32), lse2.view(torch.int32)) and torch.equal(ws, ws2)


# ---------------------------------------------------------------------------------------------------------------- backward, every d

@pytest.mark.parametrize("kind,i", ALL, ids=ALL_IDS)
def test_backward_round_trip_and_bit_identity(kind, i, device):
    run = _fwd_run(kind, i, str(device))
    call = run["call"]
    bh, n, d, dt = call["bh"], call["n"], call["d"], call["dtype"]
    q, k, v, do = (call[x].to(device) for x in ("q", "k", "v", "do"))
    o, lse = run["o"].to(device), run["lse"].to(device)
    total = int(ext._lib.fa3_backward_workspace_bytes(bh, n, d, _code(dt), 1))
    slab = fr.slab_bytes(bh, n, d)
    dq, dk, dv, ws, guards = _backward(call, device, q, k, v, o, do, lse, 1, total)
    assert guards, "bytes around the workspace were written"
    for t in (dq, dk, dv):
        assert bool(torch.isfinite(t.float()).all())
    qt, kt, vt = _slabs(ws, call, "backward")
    rot = d & (d - 1) == 0 and call["fp8_rot"] != 2
    differ = [_check_roundtrip(t, call[x], rot and x != "v", x == "v" and fr.v_pow2(call), f"{x}~") for t, x in ((qt, "q"), (kt, "k"), (vt, "v"))]
    print(f"{ALL_IDS[ALL.index((kind, i))]}: backward, elements off the float32 transcription bit for bit (q~, k~, v~) {differ}")
    if d == 128:
        # forward and backward on the same codes: R(Q~_backward) against q8 sq of the forward's workspace
        fws = fr.parse_forward_ws(run["ws"], call)
        for t, codes, sc, x in ((qt, fws["q8"], fws["sq"], "q"), (kt, fws["k8"], fws["sk"], "k")):
            want = fr.dequant(codes, sc)
            back = fr.rotation64(t) if rot else t.double()
            qrec = fr.quantise(call[x], rot, kernel="quant")
            qrec2 = fr.quantise(call[x], rot, kernel="roundtrip")
            slack = sum((fr.near_ties(r).double() * _e4m3_step(r, n)).sum(-1, keepdim=True) for r in (qrec, qrec2))
            bound = (0.5 * torch.finfo(dt).eps + 2.0 ** -18) * want.norm(dim=-1, keepdim=True) + slack
            err = (back - want).abs()
            assert bool((err <= bound).all()), f"{x}: backward's round trip against the forward's codes, worst ratio {(err / bound).max().item():.3f}"
    # the plain backward on the round-tripped tensors with the workspace that is left: the same bits
    dq0, dk0, dv0, _ws, g0 = _backward(call, device, qt.to(device), kt.to(device), vt.to(device), o, do, lse, 0, total - 3 * slab)
    assert g0
    for name, a, b in (("dq", dq, dq0), ("dk", dk, dk0), ("dv", dv, dv0)):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: fp8 = 1 differs from fp8 = 0 on the round-tripped tensors"
    dq2, dk2, dv2, ws2, _g = _backward(call, device, q, k, v, o, do, lse, 1, total)
    assert torch.equal(_bits(dq), _bits(dq2)) and torch.equal(_bits(dk), _bits(dk2)) and torch.equal(_bits(dv), _bits(dv2))
    assert torch.equal(ws[:3 * slab], ws2[:3 * slab])
