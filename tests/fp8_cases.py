"""The table of the fp8 sweep: tests/test_fp8_sharp_cpu.py proves the reference, baseline and mutants of
tests/fp8_ref.py on it, tests/test_fp8_sharp_gpu.py runs it on the kernels.  BH = 3 everywhere, so that `bh * nb` indexing counts.

d = 128 (the e4m3 MFMA kernels), CASES.  Every N names the edge of csrc/fa_fwd_fp8.hip it crosses:
     64   one 64-row quantisation block, one key tile, one (partial) query tile; fwd_fp8_kernel
    256   the last N that fwd_fp8_kernel serves alone (launch_fp8_t: fp8_v_pow2 is N > 256); four blocks, one whole query tile
    257   the smallest all-e4m3 call: nb = 5 (odd: the zeroed half tile of v8t, b1 clamped to nb - 1), one key in the last 128-key
          tile and in the last 64-row block, one row in the second query tile
    300   nb = 5 with a ragged block (44 rows) and a ragged 128-key tile
    384   even nb = 6, whole 128-key tiles, a half query tile
    520   nb = 9, three query tiles; under the mask tile 0 on fwd_fp8_kernel and tiles 1 - 2 on fwd_fp8v_kernel
options: default, fp8_pv = 1 (S on e4m3, P.V 16-bit at every N), fp8_rot = 2 (no rotation before the quantisation).
inputs: unit normal at scale d^-0.5, and "growing": the keys' norm rises 13-fold along the sequence so that the logits' running max
climbs by more than 2^8 several times (the lazy rescale is otherwise only ever taken on the first tile), and V is 2.5 times larger
on every second 64-key block (the two exponents of a 128-key V tile then differ).  Every 64-row block of q, k and v gets an absmax
with an odd mantissa (plant_block_maxima): the near-tie count of the bitwise rule then stays at what chance gives.  DATA_SEED is
chosen so that today's bars let o x 1.2 through on every all-e4m3 unit-normal case (tests/test_fp8_sharp_cpu.py asserts it; one
row with a single dominant key, |o| > 0.67, and they would not).

Other head dims (the round trip ahead of the 16-bit kernels), RT_CASES: d in {32, 64, 256} rotated, {40, 96, 192} not; N in {65 (a
one-row second block), 130 (two blocks and two rows), 300 (a ragged fifth block; two query tiles)}.

Both tables come from §9l's greedy pairwise generator (tests/ex_sweep_cases.generate) with a fixed seed, under caps of 60 and 40."""
import itertools
import random

import torch

BH = 3
SEED = 8128            # of the tables
DATA_SEED = 3          # of the tensors (build_call)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
AXES = {
    "dtype": ("bf16", "f16"),
    "mask": ("none", "causal"),
    "n": (64, 256, 257, 300, 384, 520),
    "opt": ("default", "fp8_pv=1", "fp8_rot=2"),
    "input": ("normal", "growing"),
}
RT_AXES = {
    "dtype": ("bf16", "f16"),
    "mask": ("none", "causal"),
    "n": (65, 130, 300),
    "d": (32, 64, 256, 40, 96, 192),
}
MAX_CASES, MAX_RT_CASES = 60, 40


def generate(axes, seed, tries=40):
    """Greedy, as tests/ex_sweep_cases.generate (every pair of axis values is legal here): each new case is the best of `tries`
    candidates; a candidate starts from an uncovered pair and takes, axis by axis in a shuffled order, the value that covers the
    most uncovered pairs with the values already chosen."""
    names = tuple(axes)
    rng = random.Random(seed)
    pairs_of = lambda c: {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(names, 2)}   # noqa: E731
    uncovered = {((a, va), (b, vb)) for a, b in itertools.combinations(names, 2) for va, vb in itertools.product(axes[a], axes[b])}
    cases = []
    while uncovered:
        best, best_gain = None, -1
        for _ in range(tries):
            (a, va), (b, vb) = rng.choice(sorted(uncovered, key=repr))
            c = {a: va, b: vb}
            rest = [n for n in names if n not in c]
            rng.shuffle(rest)
            for n in rest:
                scored = []
                for v in axes[n]:
                    gain = sum(1 for m in c if (((n, v), (m, c[m])) if names.index(n) < names.index(m) else ((m, c[m]), (n, v))) in uncovered)
                    scored.append((gain, rng.random(), v))
                c[n] = max(scored, key=lambda t: t[:2])[2]
            gain = len(pairs_of(c) & uncovered)
            if gain > best_gain:
                best, best_gain = c, gain
        cases.append({n: best[n] for n in names})
        uncovered -= pairs_of(best)
    return cases


CASES = generate(AXES, SEED)
RT_CASES = generate(RT_AXES, SEED + 1)
assert len(CASES) <= MAX_CASES and len(RT_CASES) <= MAX_RT_CASES


def case_id(c, i):
    return f"{i:02d}-" + "-".join(str(v) for v in c.values())


def plant_block_maxima(x, g):
    """x (16-bit) with one element of every 64-row block of every unit replaced by the block's maximum-to-be: +-a 2^e with a an ODD
    mantissa of the dtype's width (8 bits bf16, 11 bits f16), one or two (rarely a few) steps of the dtype above the block's own
    absmax, so that the tensor stays what it was statistically.  Why: an unrotated 16-bit tensor
    whose block absmax has a mantissa divisible by 4 holds dozens of elements x = 3 absmax / 2^j, whose exact quotient
    x / (absmax / 448) = 21 * 2^k is the midpoint of two e4m3 values, and the float quotient then lies within an ulp of it.  With an
    odd mantissa (not a multiple of 7: then absmax / 448 and every quotient are exact) no element of the dtype can sit there, and
    the near-tie count of tests/fp8_ref.near_ties stays at the few elements chance puts there."""
    bh, n, d = x.shape
    bits = 8 if x.dtype == torch.bfloat16 else 11
    xf = x.float()
    for b in range(bh):
        for r0 in range(0, n, 64):
            blk = xf[b, r0:r0 + 64]
            top = float(blk.abs().max())
            e = int(torch.floor(torch.log2(torch.tensor(top))))
            a = int(round(top / 2.0 ** (e + 1 - bits)))               # the absmax's mantissa as an integer in [2^(bits-1), 2^bits)
            a += 1 if a % 2 == 0 else 2
            while a % 7 == 0:
                a += 2
            if a >= 2 ** bits:
                a, e = 2 ** (bits - 1) + 1, e + 1
            pos = int(torch.randint(0, blk.numel(), (1,), generator=g))
            sign = 1.0 if pos % 2 else -1.0
            blk.view(-1)[pos] = sign * a * 2.0 ** (e + 1 - bits)
    out = xf.to(x.dtype)
    assert torch.equal(out.float(), xf)
    return out


def build_call(c, i):
    """the call of case c (index i in its table) as CPU tensors: bh, n, d, dtype, causal, scale, the option values fp8_pv and fp8_rot,
    q, k, v and do"""
    d = c.get("d", 128)
    n, dt = c["n"], DTYPES[c["dtype"]]
    g = torch.Generator(device="cpu")
    g.manual_seed(DATA_SEED + 1000 * d + i)
    q, k, v, do = (torch.randn((BH, n, d), generator=g, dtype=torch.float32) for _ in range(4))
    if c.get("input") == "growing":
        k = k * (1.0 + 12.0 * torch.arange(n, dtype=torch.float32) / n)[None, :, None]
        # and V 2.5 times larger on every second 64-key block, so that the two power-of-two exponents of a 128-key V tile differ
        v = v * (1.0 + 1.5 * ((torch.arange(n) // 64) % 2).float())[None, :, None]
    opt = c.get("opt", "default")
    q, k, v = (plant_block_maxima(t.to(dt), g) for t in (q, k, v))
    return dict(bh=BH, n=n, d=d, dtype=dt, causal=c["mask"] == "causal", scale=d ** -0.5, fp8_pv=1 if opt == "fp8_pv=1" else 0,
                fp8_rot=2 if opt == "fp8_rot=2" else 0, q=q.to(dt), k=k.to(dt), v=v.to(dt), do=do.to(dt), input=c.get("input", "normal"))
