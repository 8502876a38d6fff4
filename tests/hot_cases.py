"""The case table of the plain-path sweep (tests/test_hot_sweep_gpu.py runs it, tests/test_hot_sweep_cpu.py checks it): the kernels
behind `forward` / `backward` — the ones bench.py measures — one route at a time, and the Nq != Nk calls of `ex_forward` /
`ex_backward` that land on the same kernels.

A ROUTE is a dict of set_option values (and a kernel mode, an entry point, a misaligned storage offset) under which the dispatch
takes one kernel pair; ROUTES lists for each the head dims, masks, dtypes and shapes on which its options still decide the kernels,
with the line of flashattention-pytorch_amd/csrc that says so.  route_of(case) transcribes the dispatch itself (small_grid,
launch_fwd_mfma / launch_fwd_kb / launch_fwd_t, launch_bwd_t, bwd_ds_path, launch_bwd_dkdv_mfma, launch_bwd_dq_mfma, launch_ex_one)
and returns the kernels a case runs, the kernel names fa_profile_report shows for it and the baseline model of its rounding points
(tests/ex_full_ref.Model).  Line numbers are those of the files at the commit that added this module.

CASES comes from the greedy covering-array generator of tests/ex_sweep_cases.py (over this module's axes, the route chosen first)
with a fixed seed: every legal pair of values of two axes is in a case, and there are at most MAX_CASES.  A new kernel variant or
option adds its route here.

Shapes are the smallest at which these kernels can still go wrong: bh = 3 (5 at N <= 130), N in {31, 130, 512, 513, 1100} — less than a
tile; two 64-row tiles with a ragged end; an even number of 256-row tiles exactly; the same plus one row; nine 128-key tiles with a
ragged last one and an odd number of 256-row tiles, so that the causal heavy + light pairing leaves the middle tile alone.  The cap
binds on route x shape, so the routes that only pin a variant of a kernel a main route already runs at all five sizes take three
of them (130, 513, 1100): values of `shape` were dropped there, none of `route`."""
import itertools
import random
import zlib

import torch

from tests.ex_full_ref import Model

MAX_CASES = 200
SEED = 4242
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

# (bh, Nq, Nk)
S31, S130, S512, S513, S1100 = (5, 31, 31), (5, 130, 130), (3, 512, 512), (3, 513, 513), (3, 1100, 1100)
X1, X2, X3 = (3, 300, 1100), (3, 1100, 300), (3, 1, 513)
ALL5 = (S31, S130, S512, S513, S1100)
THREE = (S130, S513, S1100)
NQNK = (X1, X2, X3)
SMALL3 = (S31, S130, S513)      # the exact routes: 64-row workgroups and 32-key tiles — 513 is nine and seventeen of them, ragged; their baseline
#                                 (every product a float32 fma chain, term by term) takes 10 s and more at N = 1100
BOTH = ("none", "causal")
B16 = ("bf16", "f16")
WIDE = (128, 64, 96, 40, 192, 256)


def _r(opts=None, d=(128,), masks=BOTH, shapes=THREE, dtypes=B16, mode=0, api="plain", misaligned=False, why=""):
    return dict(opts=dict(opts or {}), d=tuple(d), masks=tuple(masks), shapes=tuple(shapes), dtypes=tuple(dtypes), mode=mode, api=api,
                misaligned=misaligned, why=why)


# name -> route.  `why`: where csrc says that the options decide the kernels on exactly these values.
ROUTES = {
    # ---- the rows of DESIGN 6b by the rules themselves, at every head dim
    "auto": _r({}, d=WIDE, shapes=ALL5, why="no option: small_grid (fa_fwd_mfma.hip:983-988) is true at every table shape, so d = 128 / 64 "
               "take launch_fwd_w4 (:1037-1040); the backward takes bwd_ds_path's rule (fa_bwd_mfma.hip:376-393)"),
    "sg1": _r({"small_grid": 1}, d=WIDE, shapes=ALL5, why="small_grid = 1 (fa_fwd_mfma.hip:985): launch_fwd_kb's own rule (:991-1015) — d = 64 "
              "without the mask on 64-key tiles (:1013), padded d on the 64- / 128-wide kernels (:1029-1034, staggered at d > 64), "
              "d > 128 on the 256-wide 4-wave kernel (:1025-1028); the split backward at padded and 256-wide d (fa_bwd_mfma.hip:439)"),
    "sg2": _r({"small_grid": 2}, d=(128, 64), shapes=ALL5, why="small_grid = 2 (fa_fwd_mfma.hip:986): launch_fwd_w4 at d = 128 / 64 only "
              "(:1029 sends other d past it); backward: bwd_ds_path false (fa_bwd_mfma.hip:384), the 4-wave forms of launch_dq_t "
              "(fa_bwd_dq_mfma.hip:273) and launch_bwd_dkdv_mfma (fa_bwd_dkdv_mfma.hip:322) under the mask or at d = 64"),
    # ---- forward variants
    "lock128": _r({"small_grid": 1, "fwd_stag": 2}, d=(128, 96), shapes=ALL5, why="fwd_stag = 2 is not `sweeping` (fa_fwd_mfma.hip:1035: "
                  "fwd_stag & 1), so small_grid = 1 keeps the call off launch_fwd_w4; launch_fwd_kb:1005-1014 then ends in "
                  "launch_fwd_t<D, 4> lock step; d = 96: :1031 `fwd_stag != 2`.  At d = 64 :1013 takes 64-key tiles instead"),
    "stag128": _r({"fwd_stag": 3}, d=(128, 64), shapes=ALL5, why="fa_fwd_mfma.hip:1005: so == 3 at D = 128 and D = 64; :1035 makes it "
                  "`sweeping`, past small_grid"),
    "stag64": _r({"fwd_stag": 1}, why="fa_fwd_mfma.hip:1006-1007: D == 128 && so == 1 only"),
    "two_buffer": _r({"small_grid": 1, "fwd_stag": 4}, masks=("none",), shapes=(S1100,), why="fa_fwd_mfma.hip:998, 1004-1005: so = 4 is "
                     "so_default, staggered only off short_rows: N >= 1024 without the mask; :887 ka = false -> the two-buffer kernel"),
    "fwd_kb1": _r({"fwd_kb": 1}, why="fa_fwd_mfma.hip:1008: kb == 1 && D == 128"),
    "fwd_kb2": _r({"fwd_kb": 2}, d=(128, 64), why="fa_fwd_mfma.hip:1009"),
    "fwd_tpw1": _r({"fwd_tpw": 1}, d=(128, 64), why="fa_fwd_mfma.hip:999 other_sweep -> :1014 launch_fwd_t<D, 4>, :941 tpw"),
    "fwd_tpw2": _r({"fwd_tpw": 2}, d=(128, 64), why="fa_fwd_mfma.hip:941-947"),
    "fwd_eager": _r({"fwd_eager": 1}, d=(128, 64), why="fa_fwd_mfma.hip:915, 920: !PAD && D != 256"),
    "fwd_hs": _r({"fwd_hs": 1}, d=(128, 64), why="fa_fwd_mfma.hip:915, 922"),
    "fwd_rs": _r({"fwd_rs": 1}, d=(128, 64), why="fa_fwd_mfma.hip:915-919"),
    "fwd_rd6": _r({"fwd_stag": 3, "fwd_rd": 6}, why="fa_fwd_mfma.hip:898-903: ka_ok (D == 128, KB == 4), !PAD; fwd_stag = 3 brings the "
                  "table's small launches to the staggered kernel (:1005)"),
    "fwd_rd8": _r({"fwd_stag": 3, "fwd_rd": 8}, why="fa_fwd_mfma.hip:904"),
    "fwd_w2": _r({"fwd_stag": 3, "fwd_w2": 1}, why="fa_fwd_mfma.hip:902"),
    # ---- backward variants
    "handover": _r({"dq": 6}, shapes=ALL5, why="fa_bwd_mfma.hip:383: dq == 6 -> the hand-over, under the mask and at every size; "
                   ":378 d = 128 only.  fa_bwd_dq_ds.hip:179: below 160 workgroups (every table shape) the 256-row dQ product"),
    "handover_w4": _r({"dq": 6, "dq_w4": 3}, why="fa_bwd_mfma.hip:381 lets dq_w4 = 3 through; fa_bwd_dq_ds.hip:179 forces the 4-wave form"),
    "handover_chunk4": _r({"dq": 6, "ds_chunk_mb": 4}, shapes=(S1100,), why="fa_bwd_mfma.hip:368-375, 419: dS of one unit at N = 1100 is "
                          "35 * 40 * 2 KiB = 2.73 MiB (fa_kernels.h:96-98), one unit a chunk: the loop runs three times"),
    "handover_chunk1": _r({"dq": 6, "ds_chunk_mb": 1}, shapes=(S512, S513), why="fa_bwd_mfma.hip:368-375, 419 as above: 0.5 MiB a unit at N = 512 (chunks of 2 + 1), "
                          "0.8 MiB at 513 (1 + 1 + 1); at N = 1100 one unit is over the chunk (:382) and the path is left"),
    "recompute": _r({"dq": 5, "dkdv": 5}, shapes=ALL5, why="fa_bwd_mfma.hip:380; fa_bwd_dq_mfma.hip:284 dq == 5; fa_bwd_dkdv_mfma.hip:312 "
                    "dkdv == 5; d = 128 (bwd_dq_w4_supported)"),
    "w8": _r({"small_grid": 1, "dq": 8, "dkdv": 8}, d=(128, 64), shapes=ALL5, why="fa_bwd_dq_mfma.hip:284, 273-275 and "
             "fa_bwd_dkdv_mfma.hip:312, 322-327 with small_grid = 1: the 8-wave forms; d = 64: launch_bwd_t's preparation launch "
             "(fa_bwd_mfma.hip:462-471, dq_makes_row_constants)"),
    "dkdv4": _r({"dkdv": 4}, d=(128, 64), why="fa_bwd_mfma.hip:455: split = false at unpadded d, bwd_mfma_kernel<.., FUSED = false> (:495)"),
    "atomic": _r({}, d=(128, 64), shapes=ALL5, mode=2, why="fa_capi.hip:93-96, fa_bwd_mfma.hip:444: fused at unpadded d, :494, dq_convert_kernel :502"),
    "dq_tpw1": _r({"dq_tpw": 1}, d=(128, 64), why="fa_bwd_mfma.hip:381; fa_bwd_dq_mfma.hip:283 sweeping, :273 not the 4-wave form, :237"),
    "dq_tpw2": _r({"dq_tpw": 2}, d=(128, 64), why="fa_bwd_dq_mfma.hip:237, 253"),
    "dkdv_tpw1": _r({"dkdv_tpw": 1}, d=(128, 64), why="fa_bwd_mfma.hip:381; fa_bwd_dkdv_mfma.hip:311 sweeping, :322 not the 4-wave form, :276"),
    "dkdv_tpw2": _r({"dkdv_tpw": 2}, d=(128, 64), why="fa_bwd_dkdv_mfma.hip:276, 294"),
    "dq_nlf": _r({"small_grid": 1, "dq_nlf": 1}, d=(128, 64), why="fa_bwd_dq_mfma.hip:263-264: KT == 1 && !PAD; small_grid = 1 for the 8-wave form"),
    "dq_w4": _r({"small_grid": 1, "dq_w4": 1}, d=(128, 64), why="fa_bwd_dq_mfma.hip:273-274; small_grid = 1: the rule would not pick the 4-wave form itself"),
    "dq_kt2": _r({"dq_kt": 2}, d=(128, 64), why="fa_bwd_dq_mfma.hip:275"),
    "dkdv_kreg1": _r({"dkdv_kreg": 1}, d=(64,), why="fa_bwd_dkdv_mfma.hip:288-292: D == 64 && !PAD && !W4"),
    "dkdv_kreg2": _r({"small_grid": 1, "dkdv_kreg": 2}, why="fa_bwd_dkdv_w4.hip:681-682, the stream kernel (d = 128); small_grid = 1 keeps "
                     "the masked table launches on it (fa_bwd_dkdv_mfma.hip:312)"),
    "dkdv_kreg3": _r({"small_grid": 1, "dkdv_kreg": 3}, why="fa_bwd_dkdv_w4.hip:681-682"),
    "dkdv_kreg4": _r({"small_grid": 1, "dkdv_kreg": 4}, why="fa_bwd_dkdv_w4.hip:681-682"),
    "dkdv_stg1": _r({"small_grid": 1, "dkdv": 8, "dkdv_stg": 1}, d=(128, 64), masks=("none",), why="fa_bwd_dkdv_mfma.hip:297-301: read "
                    "only at tpw == 1 (:294; under the mask :277 makes it 2) on the 8-wave form"),
    "dkdv_stg2": _r({"small_grid": 1, "dkdv": 8, "dkdv_stg": 2}, d=(128, 64), masks=("none",), why="fa_bwd_dkdv_mfma.hip:297-302"),
    # ---- exact
    "f32": _r({}, d=(128, 64, 40, 20), shapes=SMALL3, dtypes=("f32",), why="fa_fwd_mfma.hip:340 / fa_bwd_mfma.hip:348: dtype 1 or 2 only -> fa_generic.hip (fa_capi.hip:138, 157)"),
    "d20": _r({}, d=(20,), shapes=SMALL3, why="fa_fwd_mfma.hip:340: d % 8 == 0"),
    "misaligned": _r({}, d=(128, 64), shapes=SMALL3, misaligned=True, why="fa_capi.hip:101-110: aligned16"),
    "mode1": _r({}, d=(128, 40), shapes=SMALL3, dtypes=("bf16", "f16", "f32"), mode=1, why="fa_capi.hip:108: FA_MODE_F32_GENERIC"),
    # ---- Nq != Nk on the plain kernels
    "nqnk": _r({"small_grid": 1}, shapes=NQNK, api="ex", why="fa_ex.hip:915-936 after nqnk_mfma_supported (fa_fwd_mfma.hip:1017-1019: d == 128, "
               "!small_grid): launch_fwd_nqnk and launch_bwd_handover / the stream kernels with a.nk"),
    "nqnk_handover": _r({"small_grid": 1, "dq": 6}, shapes=NQNK, api="ex", why="fa_ex.hip:931-933 with bwd_ds_path's dq == 6 (fa_bwd_mfma.hip:383): "
                        "the hand-over under the shifted diagonal too"),
}

AXES = {
    "route": tuple(ROUTES),
    "dtype": ("bf16", "f16", "f32"),
    "mask": BOTH,
    "d": (128, 64, 96, 40, 192, 256, 20),
    "shape": ALL5 + NQNK,
    "scale": ("default", 0.37),
}
NAMES = tuple(AXES)
_FIELD = {"dtype": "dtypes", "mask": "masks", "d": "d", "shape": "shapes"}


def _route_takes(r, axis, value):
    return axis == "scale" or value in ROUTES[r][_FIELD[axis]]


def pair_legal(a, va, b, vb):
    """may axis a = va go with axis b = vb in one case?  A route goes with the values ROUTES lists for it (each entry cites its lines);
    two values of other axes go together where some route takes both, and never Nq > Nk under the mask."""
    p = {a: va, b: vb}
    if p.get("mask") == "causal" and "shape" in p and p["shape"][1] > p["shape"][2]:
        return False    # fa_fwd_mfma.hip:1018 nqnk_mfma_supported: `!causal || nk >= nq` (the kernels assume that every row sees key 0)
    if "route" in p:
        other = b if a == "route" else a
        return _route_takes(p["route"], other, p[other])
    return any(_route_takes(r, a, va) and _route_takes(r, b, vb) for r in ROUTES)


def case_legal(c):
    return all(pair_legal(a, c[a], b, c[b]) for a, b in itertools.combinations(NAMES, 2))


def all_pairs():
    out = set()
    for a, b in itertools.combinations(NAMES, 2):
        for va, vb in itertools.product(AXES[a], AXES[b]):
            if pair_legal(a, va, b, vb):
                out.add(((a, va), (b, vb)))
    return out


def pairs_of(c):
    return {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(NAMES, 2)}


# Triples the issue names that all-pairs alone does not promise: each is completed by the generator before it starts on the pairs.
MUST = (
    dict(route="auto", d=128, mask="none"), dict(route="auto", d=128, mask="causal"), dict(route="auto", d=64, mask="none"),
    dict(route="auto", d=40, mask="causal"), dict(route="auto", d=192, mask="causal"), dict(route="sg1", d=256, mask="causal"),
    dict(route="sg1", d=64, mask="none"), dict(route="sg1", d=64, mask="causal"), dict(route="sg1", d=128, mask="none", shape=S1100),
    dict(route="sg1", d=128, mask="causal", shape=S1100),
    dict(route="sg2", d=128, mask="causal"), dict(route="sg2", d=128, mask="none"), dict(route="sg2", d=64, mask="causal"),
    dict(route="lock128", d=128, mask="none"), dict(route="lock128", d=128, mask="causal"), dict(route="lock128", d=96, mask="none"),
    dict(route="stag128", d=128, mask="causal", shape=S1100), dict(route="stag128", d=64, mask="none"),
    dict(route="handover", d=128, mask="causal", shape=S1100), dict(route="handover", d=128, mask="none", shape=S513),
    dict(route="w8", d=128, mask="none"), dict(route="w8", d=128, mask="causal"), dict(route="w8", d=64, mask="none"), dict(route="w8", d=64, mask="causal"),
    dict(route="atomic", d=128, mask="causal"), dict(route="recompute", d=128, mask="causal", shape=S1100),
)


def _complete(c, rng, uncovered):
    """the greedy fill of tests/ex_sweep_cases.generate, the route first among the axes still open: every other axis depends on
    the route alone, so a candidate always completes"""
    c = dict(c)
    rest = [n for n in NAMES if n not in c and n != "route"]
    rng.shuffle(rest)
    if "route" not in c:
        rest.insert(0, "route")
    for n in rest:
        scored = []
        for v in AXES[n]:
            if not all(pair_legal(n, v, m, c[m]) for m in c):
                continue
            gain = sum(1 for m in c if (((n, v), (m, c[m])) if NAMES.index(n) < NAMES.index(m) else ((m, c[m]), (n, v))) in uncovered)
            scored.append((gain, rng.random(), v))
        c[n] = max(scored, key=lambda t: t[:2])[2]
    return c


def generate(seed=SEED, tries=40):
    """tests/ex_sweep_cases.generate over this module's axes, after the cases of MUST"""
    rng = random.Random(seed)
    uncovered = all_pairs()
    cases = []
    for partial in MUST:
        c = _complete(partial, rng, uncovered)
        cases.append({n: c[n] for n in NAMES})
        uncovered -= pairs_of(c)
    while uncovered:
        best, best_gain = None, -1
        for _ in range(tries):
            (a, va), (b, vb) = rng.choice(sorted(uncovered, key=repr))
            c = _complete({a: va, b: vb}, rng, uncovered)
            gain = len(pairs_of(c) & uncovered)
            if gain > best_gain:
                best, best_gain = c, gain
        cases.append({n: best[n] for n in NAMES})
        uncovered -= pairs_of(best)
    return cases


CASES = generate()


def case_name(c):
    bh, nq, nk = c["shape"]
    return f"{c['route']}-{c['dtype']}-{c['mask']}-d{c['d']}-{bh}x{nq}" + (f"x{nk}" if nk != nq else "") + f"-{c['scale']}"


def case_id(i):
    return f"{i:03d}-" + case_name(CASES[i])


# ---- the dispatch, transcribed

def _small_grid(opt, bh, n, backward, d=128):
    """fa_fwd_mfma.hip:983-988"""
    o = opt("small_grid")
    if o == 1:
        return False
    if o == 2:
        return True
    return bh * ((n + 255) // 256) <= (256 if backward or d <= 64 else 128)


def _fwd_t(opt, D, KB, pad, causal, want_stag=False):
    """fa_fwd_mfma.hip:865-956 launch_fwd_t -> (kernel name, key tile, eager, row sum on the matrix pipe)"""
    p = ",PAD" if pad else ""
    if D in (128, 64) and KB in (2, 4) and want_stag:                                           # :884-913
        if D == 128 and KB == 4 and opt("fwd_stag") != 4:                                       # :886-887 ka
            if not pad:
                if opt("fwd_w2") == 1:
                    return f"fwd_mfma_stag_kernel<128,KB=4,RD=6,W2{p}>", 128, False, False       # :902
                if opt("fwd_rd") in (6, 8):
                    return f"fwd_mfma_stag_kernel<128,KB=4,RD={opt('fwd_rd')}{p}>", 128, False, False    # :903-904
            return f"fwd_mfma_stag_kernel<128,KB=4,RD=4,KA{p}>", 128, False, False               # :909 (the production build)
        return f"fwd_mfma_stag_kernel<{D},KB={KB},two-buffer{p}>", 32 * KB, False, False         # :912
    if not pad and D != 256:                                                                    # :915-924
        if opt("fwd_rs"):
            return f"fwd_mfma_kernel<{D},KB={KB},RS>", 32 * KB, False, True
        if opt("fwd_eager"):
            return f"fwd_mfma_kernel<{D},KB={KB},EAGER>", 32 * KB, True, False
        if opt("fwd_hs"):
            return f"fwd_mfma_kernel<{D},KB={KB},HS>", 32 * KB, False, False
    if KB == 4:                                                                                 # :938-954
        tpw = opt("fwd_tpw") or (2 if causal or D == 64 else 1)
        if D == 256:
            tpw = 1
        if tpw == 2:
            return f"fwd_mfma_kernel<{D},KB=4,TPW=2{p}>", 128, False, False
    return f"fwd_mfma_kernel<{D},KB={KB},TPW=1{p}>", 32 * KB, False, False                       # :955


def _fwd(opt, d, bh, n, causal):
    """fa_fwd_mfma.hip:1024-1043 launch_fwd_mfma and :991-1015 launch_fwd_kb"""
    if d > 128:
        return _fwd_t(opt, 256, 2, d != 256, causal)                                            # :1025-1028
    if d not in (64, 128):                                                                      # :1029-1034
        stag = d > 64 and opt("fwd_stag") != 2 and not _small_grid(opt, bh, n, False, d)
        return _fwd_t(opt, 128 if d > 64 else 64, 4, True, causal, stag)
    sweeping = (opt("fwd_kb") or (opt("fwd_stag") & 1) or opt("fwd_rs") or opt("fwd_eager") or opt("fwd_hs") or opt("fwd_tpw")
                or opt("fwd_abl"))                                                              # :1035-1036
    if not sweeping and _small_grid(opt, bh, n, False, d):                                      # :1037-1040 launch_fwd_w4 (:959-975)
        return f"fwd_mfma_kernel<{d},KB=4,TPW=1,W4>", 128, False, False
    D, kb, so = d, opt("fwd_kb"), opt("fwd_stag")
    other_sweep = kb or opt("fwd_rs") or opt("fwd_eager") or opt("fwd_hs") or opt("fwd_tpw") or opt("fwd_abl")    # :999
    tiles = bh * ((n + 255) // 256)
    short_rows = (not (n >= 8192 or (n >= 4096 and tiles >= 3072))) if causal else n < 1024     # :1004
    if (D == 128 and (so == 3 or (so in (0, 4) and not other_sweep and not short_rows))) or (D == 64 and so == 3):    # :1005
        return _fwd_t(opt, D, 4, False, causal, True)
    if D == 128 and so == 1:                                                                    # :1006-1007
        return _fwd_t(opt, D, 2, False, causal, True)
    if kb == 1 and D == 128:                                                                    # :1008
        return _fwd_t(opt, D, 1, False, causal)
    if kb == 2:                                                                                 # :1009
        return _fwd_t(opt, D, 2, False, causal)
    if D == 64 and kb == 0 and not causal and not other_sweep:                                  # :1013
        return _fwd_t(opt, D, 2, False, causal)
    return _fwd_t(opt, D, 4, False, causal)                                                     # :1014


def _ds_unit_bytes(nq, nk):
    """fa_kernels.h:96-98 ds_workspace_bytes(1, nq, nk)"""
    return ((nq + 31) // 32) * (8 * ((nk + 255) // 256)) * 2048


def _chunk_units(opt, bh, nq, nk):
    """fa_bwd_mfma.hip:362-375 ds_chunk_bytes, ds_chunk_units (kv_group = 1)"""
    cb = (opt("ds_chunk_mb") << 20) if opt("ds_chunk_mb") > 0 else 4 << 30
    fit = cb // _ds_unit_bytes(nq, nk)
    if fit >= bh:
        return bh
    if fit < 1:
        return 0
    nch = (bh + fit - 1) // fit
    return (bh + nch - 1) // nch


def _ds_path(opt, d, bh, n, nk, causal, atomic):
    """fa_bwd_mfma.hip:376-393 bwd_ds_path"""
    dq, dkdv = opt("dq"), opt("dkdv")
    if atomic or d != 128:                                                                      # :378
        return False
    if (dkdv not in (0, 5)) if dq == 6 else (dq != 0 or dkdv != 0):                              # :380
        return False
    if opt("dq_kt") or opt("dq_tpw") or opt("dq_nlf") or (opt("dq_w4") and opt("dq_w4") != 3) or opt("dkdv_tpw"):    # :381
        return False
    if _ds_unit_bytes(n, nk) > ((opt("ds_chunk_mb") << 20) if opt("ds_chunk_mb") > 0 else 4 << 30):    # :382
        return False
    if dq == 6:                                                                                 # :383
        return True
    if opt("small_grid") == 2:                                                                  # :384
        return False
    if causal:                                                                                  # :391
        return (n >= 4096 or bh * ((n + 255) // 256) >= 160) and _chunk_units(opt, bh, n, nk) >= min(bh, 16)
    return True


def _dq_kt(opt, D, KT, pad, w4, causal):
    """fa_bwd_dq_mfma.hip:229-267 launch_dq_kt"""
    tpw = opt("dq_tpw") or (2 if KT == 1 and (causal or D == 128) else 1)                       # :237-238
    if KT != 1 or D == 256:
        tpw = 1                                                                                 # :239
    nlf = D == 256 or (KT == 1 and not pad and opt("dq_nlf") == 1)                              # :262-265
    return f"bwd_dq_mfma_kernel<{D},KT={KT},TPW={tpw}" + (",PAD" if pad else "") + (",NLF" if nlf else "") + (",W4" if w4 else "") + ">"


def _dq(opt, d, bh, n, causal):
    """fa_bwd_dq_mfma.hip:278-296 launch_bwd_dq_mfma and :271-276 launch_dq_t"""
    sweeping = opt("dq_kt") or opt("dq_tpw") or opt("dq_nlf") or opt("dq_w4")                   # :283
    if d == 128 and (opt("dq") == 5 or (opt("dq") == 0 and not sweeping and (not _small_grid(opt, bh, n, True) or not causal))):    # :284
        return "bwd_dq_w4_kernel"
    if d > 128:
        return _dq_kt(opt, 256, 1, d != 256, False, causal)                                     # :286-289
    if d not in (64, 128):
        return _dq_kt(opt, 128 if d > 64 else 64, 1, True, False, causal)                       # :290-293
    if opt("dq_w4") == 1 or (opt("dq_w4") == 0 and opt("dq_kt") == 0 and opt("dq_tpw") == 0 and _small_grid(opt, bh, n, True)):    # :273
        return _dq_kt(opt, d, 1, False, True, causal)
    return _dq_kt(opt, d, 2 if opt("dq_kt") == 2 else 1, False, False, causal)                  # :275


def _stream_dkdv(opt, dtype, causal, ds):
    """fa_bwd_dkdv_w4.hip:658-744 launch_dkdv_w4_t: the K rows kept in registers"""
    kro = opt("dkdv_kreg")
    kr = {2: 0, 3: 1, 4: 2}.get(kro, 3)                                                         # :681-682
    if ds and causal and kr == 3 and dtype == "f16":
        kr = 2                                                                                  # :698
    return f"bwd_dkdv_w4_kernel<KR={kr}" + (",DS" if ds else "") + ">"


def _dkdv_t(opt, D, pad, w4, causal):
    """fa_bwd_dkdv_mfma.hip:269-303 launch_dkdv_t"""
    tail = (",PAD" if pad else "") + (",W4" if w4 else "")
    tpw = opt("dkdv_tpw") or (2 if causal and not w4 else 1)                                    # :276-277
    if D == 64 and not pad and not w4 and opt("dkdv_kreg") == 1:                                # :288-292
        return "bwd_dkdv_mfma_kernel<64,KREG,TPW=1>"
    if tpw == 2:
        return f"bwd_dkdv_mfma_kernel<{D},TPW=2{tail}>"                                         # :294-295
    so = opt("dkdv_stg")
    stg = (so == 1 or (so == 0 and D == 128)) and not pad and not w4                            # :297-301
    return f"bwd_dkdv_mfma_kernel<{D},TPW=1{tail}" + (",STG" if stg else "") + ">"


def _dkdv(opt, dtype, d, bh, n, causal):
    """fa_bwd_dkdv_mfma.hip:305-328 launch_bwd_dkdv_mfma"""
    dk = opt("dkdv")
    sweeping = opt("dkdv_kreg") == 1 or opt("dkdv_tpw") or opt("dkdv_stg")                      # :311
    if d == 128 and (dk == 5 or (dk == 0 and not sweeping and (not _small_grid(opt, bh, n, True) if causal else True))):    # :312
        return _stream_dkdv(opt, dtype, causal, False)
    if d > 128:
        return _dkdv_t(opt, 256, d != 256, False, causal)                                       # :314-317
    if d not in (64, 128):
        return _dkdv_t(opt, 128 if d > 64 else 64, True, False, causal)                         # :318-321
    if opt("dkdv_kreg") != 1 and opt("dkdv_tpw") == 0 and _small_grid(opt, bh, n, True):        # :322-325
        return _dkdv_t(opt, d, False, True, causal)
    return _dkdv_t(opt, d, False, False, causal)                                                # :326-327


def _handover(opt, dtype, bh, nq, nk, causal):
    """fa_bwd_mfma.hip:407-430 run_handover_t; fa_bwd_dq_ds.hip:172-194 launch_dq_ds_t"""
    step = _chunk_units(opt, bh, nq, nk)
    chunks = (bh + step - 1) // step
    nqt8 = (nq + 511) // 512
    nw = 4 if (opt("dq_w4") == 3 or ((nqt8 + 1) // 2 if causal else nqt8) * step < 160) else 8    # :179 (a.bh is the chunk's there)
    return ("bwd_prep_kernel", _stream_dkdv(opt, dtype, causal, True), f"bwd_dq_ds_kernel<NW={nw}>"), chunks


def route_of(c):
    """What the dispatch does with case c: dict(fwd, bwd (kernels in launch order), chunks (of the dS hand-over, 0 without it),
    profile (the kernel names fa_profile_report shows for the forward + backward), model (ex_full_ref.Model), deterministic)."""
    r = ROUTES[c["route"]]
    opt = lambda name: r["opts"].get(name, 0)   # noqa: E731
    dtype, d, causal = c["dtype"], c["d"], c["mask"] == "causal"
    bh, nq, nk = c["shape"]
    # fa_capi.hip:107-114 use_mfma_fwd / use_mfma_bwd (the scale and slab sizes of the table always pass)
    if r["mode"] == 1 or r["misaligned"] or dtype == "f32" or d % 8 or d < 8:
        # fa_generic.hip:539-582: the exact-f32 kernels; everything in fp32, every product an fma chain (ex_full_ref._mm, chunk 1)
        return dict(fwd="fwd_generic", bwd=("bwd_delta_generic", "bwd_dkdv_generic", "bwd_dq_generic"), chunks=0,
                    profile={"fwd_f32", "bwd_delta", "bwd_dkdv_f32", "bwd_dq_f32"}, model=Model(key_tile=32, f32_inside=True, fma_chain=True), deterministic=True)
    if r["api"] == "ex":
        # fa_ex.hip:915-936: needs !small_grid(bh, min(nq, nk)) (fa_fwd_mfma.hip:1018); launch_fwd_nqnk = launch_fwd_t<128, 4>(stag) :1020-1022
        assert d == 128 and not _small_grid(opt, bh, min(nq, nk), False, d) and (not causal or nk >= nq)
        fwd, tile, eager, rs = _fwd_t(opt, 128, 4, False, causal, True)
        if _ds_path(opt, d, bh, nq, nk, causal, False):                                         # :931-933
            bwd, chunks = _handover(opt, dtype, bh, nq, nk, causal)
            prof = {"bwd_delta", "bwd_mfma", "bwd_dq_mfma"}
        else:                                                                                   # :934-936
            bwd, chunks, prof = ("bwd_dq_w4_kernel", _stream_dkdv(opt, dtype, causal, False)), 0, {"bwd_mfma", "bwd_dq_mfma"}
        return dict(fwd=fwd, bwd=bwd, chunks=chunks, profile=prof | {"fwd_mfma"}, deterministic=True,
                    model=Model(key_tile=tile, lazy_rescale=not eager, exp2=True, rowsum_rounded_p=rs))
    n = nq
    fwd, tile, eager, rs = _fwd(opt, d, bh, n, causal)
    # fa_bwd_mfma.hip:435-507 launch_bwd_t
    D = 256 if d > 128 else (128 if d > 64 else 64)
    pad = d != D or D == 256                                                                    # :439
    fused = r["mode"] == 2 and not pad                                                          # :444
    split = pad or (not fused and opt("dkdv") != 4)                                             # :455
    chunks = 0
    if not pad and _ds_path(opt, d, bh, n, n, causal, fused):                                   # :456-461 (the Python layer gives the room)
        bwd, chunks = _handover(opt, dtype, bh, n, n, causal)
        prof = {"bwd_delta", "bwd_mfma", "bwd_dq_mfma"}
    elif split and d > 64:                                                                      # :462-466 dq first: it makes the row constants
        bwd, prof = (_dq(opt, d, bh, n, causal), _dkdv(opt, dtype, d, bh, n, causal)), {"bwd_mfma", "bwd_dq_mfma"}
    elif split:                                                                                 # :467-478
        bwd, prof = ("bwd_prep_kernel", _dkdv(opt, dtype, d, bh, n, causal), _dq(opt, d, bh, n, causal)), {"bwd_delta", "bwd_mfma", "bwd_dq_mfma"}
    elif fused:                                                                                 # :494, 499-504
        bwd, prof = ("bwd_prep_kernel", f"bwd_mfma_kernel<{D},FUSED_DQ>", "dq_convert_kernel"), {"bwd_delta", "bwd_mfma", "bwd_dq_cvt"}
    else:                                                                                       # :495, 498 (dkdv = 4)
        bwd, prof = ("bwd_prep_kernel", f"bwd_mfma_kernel<{D}>", _dq(opt, d, bh, n, causal)), {"bwd_delta", "bwd_mfma", "bwd_dq_mfma"}
    rounded_p = any(k.startswith("bwd_dkdv_mfma_kernel") for k in bwd)
    return dict(fwd=fwd, bwd=bwd, chunks=chunks, profile=prof | {"fwd_mfma"}, deterministic=not fused,
                model=Model(key_tile=tile, lazy_rescale=not eager, exp2=True, rowsum_rounded_p=rs, dk_ds_from_rounded_p=rounded_p))


def family(c):
    """the row of the record's ratio table a case belongs to"""
    ro = route_of(c)
    if ro["fwd"] == "fwd_generic":
        return "exact"
    if ROUTES[c["route"]]["api"] == "ex":
        return "nqnk"
    bwd = ro["bwd"]
    back = ("handover" if ro["chunks"] else "atomic" if not ro["deterministic"] else "stream" if any("w4_kernel" in k for k in bwd) and
            not any("mfma_kernel" in k for k in bwd) else "8wave/4wave")
    return ("stag" if "stag" in ro["fwd"] else "w4" if "W4" in ro["fwd"] else "lock") + "+" + back


# ---- inputs

def problem_key(c):
    return (c["shape"], c["d"], c["dtype"], c["mask"], c["scale"])


def build_call(key):
    """The plain call of a problem as the dict tests/ex_full_ref.py reads (layout padded, heads (1, 1), no feature), seeded by the
    problem like tests.helpers.make_qkv: q, k, v, do from one CPU generator, in that order.  Under scale 0.37 q has the deviation
    d^-0.5 / 0.37, as in tests/ex_sweep_cases.build_inputs and for its reason: the logits keep unit variance."""
    (bh, nq, nk), d, dtype, mask, scale = key
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(repr(key).encode()))
    dt = DTYPES[dtype]
    qstd = 1.0 if scale == "default" else d ** -0.5 / float(scale)
    q = (torch.randn((bh, nq, d), generator=g, dtype=torch.float32) * qstd).to(dt)
    k, v = (torch.randn((bh, nk, d), generator=g, dtype=torch.float32).to(dt) for _ in range(2))
    do = torch.randn((bh, nq, d), generator=g, dtype=torch.float32).to(dt)
    return dict(layout="padded", dtype=dt, path=0, heads=(1, 1), q=q, k=k, v=v, do=do, causal=mask == "causal",
                scale=d ** -0.5 if scale == "default" else float(scale), window=(-1, -1), softcap=0.0, alibi_slopes=None, sinks=None,
                dlse=None, dropout_p=0.0, seed=0, mask=None, block_mask=None, br=128, bc=128, cu_seqlens_q=None, cu_seqlens_k=None,
                max_seqlen_q=None, max_seqlen_k=None)
