"""GPU: the sweep of the plain path — the kernels behind `forward` / `backward` that bench.py measures, every route and variant of
DESIGN.md 6b, and the Nq != Nk calls of `ex_forward` / `ex_backward` that land on the same kernels.  One test per case of
tests/hot_cases.py: the route's options are set, forward then backward run, every option is reset, and the results are held to
tests/ex_full_ref.py three times:

  * the project's bar, unchanged (ex_full_ref.project_bar);
  * the sharp bar, unchanged (ex_full_ref.sharp_bar): max |kernel - fp64| <= 2 * max |baseline - fp64| + eps * max |fp64| per tensor,
    the baseline being ex_full_ref.baseline under the model hot_cases.route_of names for the kernels the case runs;
  * under the mask the same bar on each band of ex_full_ref.band_edges alone, so that the first rows, where |o| ~ |v|, do not set
    the maximum for the long ones (banded_sharp_bar: the same function on slices, the same factor).

A kernel outside the sharp bar has a rounding point the model lacks — it is then added to ex_full_ref.Model with its file and
function — or a bug; the factor is not raised.  "hot_sweep_ratio ..." lines print kernel error / baseline error per case and
tensor; profiles/hot_sweep.md records the largest.

Where fa_profile_report tells routes apart the case asserts the kernel names it shows (route_of's `profile`): bwd_delta on the
hand-over and the d <= 64 / 4-wave-file routes and never on the recomputing d = 128 routes, bwd_dq_cvt on the atomic backward,
fwd_f32 on the exact routes.  Then the bit identities the code promises, once each on the table's shapes, and the default rules
at a real launch size with no option set."""
import functools
import time
from types import SimpleNamespace

import pytest
import torch

from tests import ex_full_ref as fr
from tests import hot_cases as hc

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [hc.case_id(i) for i in range(len(hc.CASES))]
ALL_OPTIONS = sorted({name for r in hc.ROUTES.values() for name in r["opts"]})
NAMES5 = ("o", "lse", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def problem(key):
    """(call, fp64 reference) of a problem, computed once and never changed; the routes that share a problem share them"""
    call = hc.build_call(key)
    return call, fr.full_reference(call)


@functools.lru_cache(maxsize=None)
def baseline_of(key, model):
    return fr.baseline(problem(key)[0], model=model)


def misaligned(t):
    """t on the device at a storage offset of 8 bytes (four 16-bit elements): contiguous, not 16-byte aligned"""
    buf = torch.empty((t.numel() + 8,), dtype=t.dtype, device=DEV)
    out = buf[4:4 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous()
    return out


def run_route(route, q, k, v, do, causal, scale, profile=False):
    """(o, lse, dq, dk, dv) and the kernel names fa_profile_report shows, on device tensors, under the route's options; every
    option and the kernel mode are reset whatever happens"""
    import flashattention_lab_cuda as ext

    r = hc.ROUTES[route] if isinstance(route, str) else dict(opts=route, mode=0, api="plain")     # (or a bare dict of options)
    old_mode = ext.set_kernel_mode(r["mode"])
    shown = None
    try:
        for name, val in r["opts"].items():
            ext.set_option(name, val)
        if profile:
            ext.profile_enable(True)
        if r["api"] == "ex":
            o, lse = ext.ex_forward(q, k, v, causal, scale)
            dq, dk, dv = ext.ex_backward(q, k, v, o, do, lse, causal, scale)
        else:
            o, lse = ext.forward(q, k, v, causal, scale, 128, 128)
            dq, dk, dv = ext.backward(q, k, v, o, do, lse, causal, scale, 128, 128)
        if profile:
            shown = {name for name, (count, _ms) in ext.profile_report().items() if count > 0}
    finally:
        if profile:
            ext.profile_enable(False)
        for name in ALL_OPTIONS:
            ext.set_option(name, 0)
        ext.set_kernel_mode(old_mode)
    torch.cuda.synchronize()
    return (o, lse, dq, dk, dv), shown


def on_device(c, call):
    put = misaligned if hc.ROUTES[c["route"]]["misaligned"] else (lambda t: t.to(DEV))
    return tuple(put(call[n]) for n in ("q", "k", "v", "do"))


def as_result(out):
    return SimpleNamespace(**{n: t.cpu() for n, t in zip(NAMES5, out)}, dsinks=None)


def hold_to_the_bars(what, got, call, ref, base, route_text):
    """prints the ratios, then asserts the three bars"""
    dtype = call["dtype"]
    for name in ("o", "dq", "dk", "dv"):
        t = getattr(got, name)
        assert t.shape == getattr(ref, name).shape and t.dtype == dtype, name
    assert got.lse.shape == ref.lse.shape and got.lse.dtype == torch.float32
    project = fr.project_bar(got, ref, dtype)
    sharp, ratio = fr.sharp_bar(got, ref, base, dtype)
    print(f"hot_sweep_ratio {what} {route_text} " + " ".join(f"{n}={r:.3f}" for n, r in ratio.items()))
    eg, eb = fr.errors(got, ref), fr.errors(base, ref)      # how much of the sharp bar's bound each tensor uses (the record's "nearest")
    used = {n: e / (2.0 * eb[n][0] + torch.finfo(torch.float32 if n == "lse" else dtype).eps * big) for n, (e, big) in eg.items() if big > 0.0}
    print(f"hot_sweep_used {what} " + " ".join(f"{n}={u:.3f}" for n, u in used.items()))
    banded = []
    if call["causal"]:
        banded, bratio = fr.banded_sharp_bar(got, ref, base, dtype)
        print(f"hot_sweep_band {what} " + " ".join(f"{n}={r:.3f}" for n, r in bratio.items()))
    assert not project, f"{what}: the project's bar: {project}"
    assert not sharp, f"{what}: the sharp bar: {sharp}"
    assert not banded, f"{what}: the sharp bar per band: {banded}"


@pytest.mark.parametrize("i", range(len(hc.CASES)), ids=IDS)
def test_case(i):
    c = hc.CASES[i]
    ro = hc.route_of(c)
    key = hc.problem_key(c)
    call, ref = problem(key)
    base = baseline_of(key, ro["model"])
    out, shown = run_route(c["route"], *on_device(c, call), call["causal"], call["scale"], profile=True)
    assert shown == ro["profile"], f"{IDS[i]}: fa_profile_report shows {sorted(shown)}, route_of expects {sorted(ro['profile'])}"
    hold_to_the_bars(IDS[i], as_result(out), call, ref, base, f"route={c['route']} family={hc.family(c)}")


# ---- bit identities the code promises

SQUARE_128 = [(s, m, t) for s in hc.ALL5 for m in hc.BOTH for t in hc.B16]


def _inputs(shape, d, dtype, mask):
    call, _ref = problem((shape, d, dtype, mask, "default"))
    return call, tuple(call[n].to(DEV) for n in ("q", "k", "v", "do"))


def _forward(route, q, k, v, causal, scale):
    import flashattention_lab_cuda as ext

    try:
        for name, val in hc.ROUTES[route]["opts"].items():
            ext.set_option(name, val)
        out = ext.forward(q, k, v, causal, scale, 128, 128)
    finally:
        for name in ALL_OPTIONS:
            ext.set_option(name, 0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape,mask,dtype", SQUARE_128, ids=lambda v: str(v).replace(" ", ""))
def test_staggered_forward_is_bitwise_the_lock_step_forward(shape, mask, dtype):
    """fa_fwd_mfma.hip, launch_fwd_kb: "bitwise the same results, it performs the same operations in the same order" """
    c = dict(dtype=dtype, mask=mask, d=128, shape=shape, scale="default")
    assert "stag_kernel<128,KB=4" in hc.route_of(dict(c, route="stag128"))["fwd"]
    assert hc.route_of(dict(c, route="lock128"))["fwd"].startswith("fwd_mfma_kernel<128,KB=4,TPW")
    call, (q, k, v, _do) = _inputs(shape, 128, dtype, mask)
    o1, l1 = _forward("stag128", q, k, v, call["causal"], call["scale"])
    o2, l2 = _forward("lock128", q, k, v, call["causal"], call["scale"])
    assert torch.equal(o1, o2) and torch.equal(l1, l2), ((o1.float() - o2.float()).abs().max().item(), (l1 - l2).abs().max().item())


@pytest.mark.parametrize("shape,mask,dtype", [t for t in SQUARE_128 if t[0] in hc.THREE], ids=lambda v: str(v).replace(" ", ""))
def test_dv_of_the_stream_kernel_is_bitwise_the_8wave_kernels(shape, mask, dtype):
    """fa_bwd_dkdv_w4.hip forms the same P in the same order as the 8-wave kernel: dV bit for bit, every form of the
    stream kernel's K registers included — while both read the row constants of the same maker.  (Under the hand-over the
    constants are bwd_prep_kernel's, -lse * (1 / scale) (fa_bwd_mfma.hip:62), where the dQ kernels make -lse / scale
    (fa_bwd_dq_mfma.hip:80): P then differs in its last float32 bit in places and dV by one unit of the tensor dtype, which the
    first run of this sweep measured: 2^-9 at bf16.  That is a rounding point, held by the bars, and no identity.)"""
    call, dev = _inputs(shape, 128, dtype, mask)
    a, _ = run_route({"small_grid": 1, "dkdv": 8}, *dev, call["causal"], call["scale"])
    for kreg in (0, 2, 3, 4):
        b, _ = run_route({"small_grid": 1, "dkdv": 5, "dkdv_kreg": kreg}, *dev, call["causal"], call["scale"])
        assert torch.equal(a[4], b[4]), (kreg, (a[4].float() - b[4].float()).abs().max().item())
        assert torch.equal(a[2], b[2]), "dq: the same dQ kernel on both sides"


FIRST_OF_ROUTE = {}
for _i, _c in enumerate(hc.CASES):
    FIRST_OF_ROUTE.setdefault(_c["route"], _i)


@pytest.mark.parametrize("route", [r for r in hc.ROUTES if r != "atomic"])
def test_a_deterministic_route_gives_the_same_bits_twice(route):
    i = FIRST_OF_ROUTE[route]
    c = hc.CASES[i]
    assert hc.route_of(c)["deterministic"]
    call, _ref = problem(hc.problem_key(c))
    dev = on_device(c, call)
    a, _ = run_route(route, *dev, call["causal"], call["scale"])
    b, _ = run_route(route, *dev, call["causal"], call["scale"])
    for name, x, y in zip(NAMES5, a, b):
        assert torch.equal(x, y), (IDS[i], name)


def test_the_atomic_route_is_the_one_that_is_not_deterministic():
    assert [r for r in hc.ROUTES if any(not hc.route_of(c)["deterministic"] for c in hc.CASES if c["route"] == r)] == ["atomic"]


ALONE = [(r, d, s, m) for r, d in (("sg2", 128), ("lock128", 128), ("stag128", 128), ("sg1", 64), ("sg2", 64), ("sg1", 96), ("sg1", 192))
         for s in (hc.S513, hc.S1100) for m in hc.BOTH]


@pytest.mark.parametrize("route,d,shape,mask", ALONE, ids=lambda v: str(v).replace(" ", ""))
def test_a_unit_alone_is_bitwise_the_unit_inside_the_launch(route, d, shape, mask):
    """forward: a (b, h) unit's rows depend on nothing but the unit (under options that pin the kernel whatever the launch size)"""
    c = dict(route=route, dtype="bf16", mask=mask, d=d, shape=shape, scale="default")
    assert hc.route_of(c)["fwd"] == hc.route_of(dict(c, shape=(1,) + shape[1:]))["fwd"]
    call, (q, k, v, _do) = _inputs(shape, d, "bf16", mask)
    o, lse = _forward(route, q, k, v, call["causal"], call["scale"])
    for u in range(shape[0]):
        ou, lu = _forward(route, q[u:u + 1].contiguous(), k[u:u + 1].contiguous(), v[u:u + 1].contiguous(), call["causal"], call["scale"])
        assert torch.equal(o[u:u + 1], ou) and torch.equal(lse[u:u + 1], lu), u


# ---- the default rules at a real launch size, no option set

REAL = [(d, t, m) for d in (128, 64) for t in hc.B16 for m in hc.BOTH]


@pytest.mark.parametrize("d,dtype,mask", REAL, ids=lambda v: str(v))
def test_the_default_rules_at_a_real_launch_size(d, dtype, mask):
    """8 distinct units x 20 copies (bh = 160; 10 copies, bh = 80, at d = 64) at N = 1100: by the rules themselves the staggered
    forward (no mask), the lock-step pairs (mask) and the hand-over with the 512-row dQ product in both maskings at d = 128, the
    64-key lock-step forward and the 8-wave backward with its preparation launch at d = 64.  Copies are bitwise equal; the distinct
    units are held to both bars."""
    copies = 20 if d == 128 else 10
    big = dict(route="auto", dtype=dtype, mask=mask, d=d, shape=(8 * copies, 1100, 1100), scale="default")
    ro = hc.route_of(big)
    if d == 128:
        assert ro["fwd"] == ("fwd_mfma_kernel<128,KB=4,TPW=2>" if mask == "causal" else "fwd_mfma_stag_kernel<128,KB=4,RD=4,KA>")
        assert ro["bwd"][0] == "bwd_prep_kernel" and ro["bwd"][1].startswith("bwd_dkdv_w4_kernel") and ro["bwd"][2] == "bwd_dq_ds_kernel<NW=8>"
        assert ro["chunks"] == 1
    else:
        assert ro["fwd"] == ("fwd_mfma_kernel<64,KB=4,TPW=2>" if mask == "causal" else "fwd_mfma_kernel<64,KB=2,TPW=1>")
        assert ro["bwd"] == ("bwd_prep_kernel", f"bwd_dkdv_mfma_kernel<64,TPW={2 if mask == 'causal' else 1}>",
                             f"bwd_dq_mfma_kernel<64,KT=1,TPW={2 if mask == 'causal' else 1}>")
    key = ((8, 1100, 1100), d, dtype, mask, "default")
    call, ref = problem(key)
    base = baseline_of(key, ro["model"])
    dev = tuple(call[n].to(DEV).repeat(copies, 1, 1) for n in ("q", "k", "v", "do"))      # unit u is distinct unit u % 8
    t0 = time.perf_counter()
    out, shown = run_route("auto", *dev, call["causal"], call["scale"], profile=True)
    print(f"hot_sweep_real d={d} {dtype} {mask}: forward + backward {1e3 * (time.perf_counter() - t0):.1f} ms, kernels {sorted(shown)}")
    assert shown == ro["profile"]
    for name, t in zip(NAMES5, out):
        first = t[:8]
        for cpy in range(1, copies):
            assert torch.equal(t[8 * cpy:8 * cpy + 8], first), (name, cpy)
    got = as_result(tuple(t[:8] for t in out))
    hold_to_the_bars(f"real-d{d}-{dtype}-{mask}", got, call, ref, base, f"route=auto family={hc.family(big)}")
