"""The all-pairs case table of the KV-cache decoding sweep (tests/test_kvcache_sweep_gpu.py runs it, tests/test_kvcache_sweep_cpu.py
checks it) and the inputs of a case, as CPU tensors in the keywords of ex_kvcache_forward.

AXES lists the features a decode call combines.  CASES comes from a greedy covering-array generator with a fixed seed: every
pair of values of two different axes that the C layer accepts together (pair_legal: rotary needs new keys and a rotary_dim in
[16, d]) is in at least one case, every case is legal, and there are at most MAX_CASES of them.  A new decode feature adds its
axis here.  Sizes: four sequences over a capacity of 192 (a multiple of both page sizes), cached lengths from {0, 1, 33, 100,
capacity - nnew}, one sequence empty and one full in every case — several 32-key tiles, several splits and page crossings inside
a tile, nothing larger."""
import itertools
import random

import torch

from tests.kvcache_fp8_ref import E4M3, quantize
from tests.kvcache_rotary_ref import tables
from tests.kvcache_varlen_ref import lengths_to_cu

B, CAP = 4, 192
MAX_CASES = 120
SEED = 20240
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
AXES = {
    "dtype": ("bf16", "f16"),
    "d": (8, 24, 40, 64, 72, 96, 128, 136, 200, 256),
    "heads": ((8, 8), (8, 2), (6, 2), (5, 1), (12, 2), (12, 1), (32, 1), (40, 2)),                  # (H_q, H_kv)
    "queries": ("nq1", "nq3", "nq7", "nq18", "packed7", "packed18"),                                # packed: max_seqlen_q
    "nnew": (0, 1, 3),
    "addr": ("contig", "bidx", "leftpad", "bidx+leftpad", "paged16", "paged48"),
    "cache": ("16bit", "e4m3"),
    "rotary": ("off", "gptj", "neox"),              # gptj: interleaved, rotary_dim = d rounded down to 16; neox: 16 or 32, < d
    "mask": ("none", "causal", "window5_0", "window40_2", "causal+window33"),
    "mods": ("none", "softcap", "alibi", "alibi_b+softcap"),
    "sinks": (False, True),
    "splits": (0, 1, 2, 5),
}
# values no other decode test runs
BOLD = {"d": (8, 24, 40, 72, 136, 200), "heads": ((6, 2), (5, 1), (12, 2), (12, 1), (32, 1), (40, 2))}
NAMES = tuple(AXES)


def rotary_dim(kind, d):
    """rotary_dim of a rotary axis value at head dim d; 0 where there is none that the C layer accepts"""
    if kind == "gptj":
        return d // 16 * 16
    if kind == "neox":
        return 32 if d > 32 else (16 if d > 16 else 0)
    return 0


def pair_legal(a, va, b, vb):
    """may axis a = va go with axis b = vb in one call?  (fa_capi.hip, kvcache_impl: rotary needs seqlen_new > 0 and
    16 <= rotary_dim <= head_dim.  paged against cache_batch_idx / cache_leftpad and packed new keys without packed queries
    cannot be written down in these axes.)"""
    p = {a: va, b: vb}
    if p.get("rotary", "off") != "off":
        if p.get("nnew") == 0:
            return False
        if "d" in p and rotary_dim(p["rotary"], p["d"]) == 0:
            return False
    return True


def case_legal(c):
    return all(pair_legal(a, c[a], b, c[b]) for a, b in itertools.combinations(NAMES, 2))


def all_pairs():
    """every legal ((axis, value), (axis, value)) with the axes in NAMES order"""
    out = set()
    for a, b in itertools.combinations(NAMES, 2):
        for va, vb in itertools.product(AXES[a], AXES[b]):
            if pair_legal(a, va, b, vb):
                out.add(((a, va), (b, vb)))
    return out


def pairs_of(c):
    return {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(NAMES, 2)}


def generate(seed=SEED, tries=40):
    """Greedy: each new case is the best of `tries` candidates; a candidate starts from an uncovered pair and takes, axis by
    axis in a shuffled order, the legal value that covers the most uncovered pairs with the values already chosen."""
    rng = random.Random(seed)
    uncovered = all_pairs()
    cases = []
    while uncovered:
        best, best_gain = None, -1
        for _ in range(tries):
            (a, va), (b, vb) = rng.choice(sorted(uncovered, key=repr))
            c = {a: va, b: vb}
            rest = [n for n in NAMES if n not in c]
            rng.shuffle(rest)
            for n in rest:
                scored = []
                for v in AXES[n]:
                    if not all(pair_legal(n, v, m, c[m]) for m in c):
                        continue
                    gain = sum(1 for m in c if (((n, v), (m, c[m])) if NAMES.index(n) < NAMES.index(m) else ((m, c[m]), (n, v))) in uncovered)
                    scored.append((gain, rng.random(), v))
                c[n] = max(scored, key=lambda t: t[:2])[2]
            gain = len(pairs_of(c) & uncovered)
            if gain > best_gain:
                best, best_gain = c, gain
        cases.append({n: best[n] for n in NAMES})
        uncovered -= pairs_of(best)
    return cases


CASES = generate()


def case_id(i):
    c = CASES[i]
    return f"{i:03d}-" + "-".join(str(c[n]).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") for n in NAMES)


def fixed_split_cases():
    """the cases of the fixed-split extras: for every bold value the first case that holds it (about ten)"""
    out = []
    for axis, vals in BOLD.items():
        for v in vals:
            i = next(i for i, c in enumerate(CASES) if c[axis] == v and i not in out)
            out.append(i)
    return sorted(out)


def window_of(mask):
    return {"window5_0": (5, 0), "window40_2": (40, 2), "causal+window33": (33, -1)}.get(mask, (-1, -1))


def shape_of(c, i):
    """the per-sequence counts of case c (index i seeds the choice): nq, nnew, cached lengths as passed and clamped"""
    rng = random.Random(SEED + 1000 + i)
    packed = c["queries"].startswith("packed")
    if packed:
        mq = int(c["queries"][6:])
        nq = [mq, 0, 3 if mq == 7 else 5, 1]               # a full-length, an empty, a partial-tile and a one-token sequence
        rng.shuffle(nq)
        nnew = {0: [0, 0, 0, 0], 1: [1, 0, 1, 1], 3: [3, 0, 1, 2]}[c["nnew"]]
        rng.shuffle(nnew)
    else:
        nq, nnew = [int(c["queries"][2:])] * B, [c["nnew"]] * B
    order = [0, 1, 2, 3]
    rng.shuffle(order)
    lens = [0] * B
    lens[order[0]] = 0                                      # the empty sequence
    lens[order[1]] = CAP - nnew[order[1]]                   # the full one
    lens[order[2]], lens[order[3]] = rng.choice([1, 33, 100]), rng.choice([33, 100])
    raw = list(lens)
    if i % 2:
        raw[order[1]] = CAP + 5                             # above the capacity: clamped to the same length
    return packed, nq, nnew, raw, lens


def build_inputs(i, case=None):
    """The call of case i as {keyword of ex_kvcache_forward: CPU tensor or value}, seeded by i; k_cache and v_cache are views of
    the middle of the canary buffers under "k_big" / "v_big" (not keywords of the call).  An e4m3 cache is torch.float8_e4m3fn."""
    c = CASES[i] if case is None else case
    g = torch.Generator().manual_seed(SEED + i)
    dtype, d, (hq, hkv) = DTYPES[c["dtype"]], c["d"], c["heads"]
    rn = lambda *shape: torch.randn(shape, generator=g).to(dtype)   # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)   # noqa: E731
    packed, nq, nnew, raw, lens = shape_of(c, i)
    kw = dict(causal=c["mask"] in ("causal", "causal+window33"), softmax_scale=None, window=window_of(c["mask"]), softcap=0.0,
              alibi_slopes=None, num_splits=c["splits"], block_table=None, cache_batch_idx=None, cache_leftpad=None, rotary_cos=None,
              rotary_sin=None, rotary_interleaved=True, cu_seqlens_q=None, cu_seqlens_k_new=None, max_seqlen_q=None, sinks=None,
              k_descale=None, v_descale=None, k_new=None, v_new=None, cache_seqlens=i32(raw))
    # ---- queries and new keys
    if packed:
        cu = [x + 1 for x in lengths_to_cu(nq)]            # token 0 and the last token belong to no sequence
        kw["q"] = rn(cu[-1] + 1, hq, d)
        kw["cu_seqlens_q"], kw["max_seqlen_q"] = i32(cu), max(nq)
        if c["nnew"]:
            kw["k_new"], kw["v_new"] = rn(sum(nnew), hkv, d), rn(sum(nnew), hkv, d)
            kw["cu_seqlens_k_new"] = i32(lengths_to_cu(nnew))
    else:
        kw["q"] = rn(B, nq[0], hq, d)
        if c["nnew"]:
            kw["k_new"], kw["v_new"] = rn(B, c["nnew"], hkv, d), rn(B, c["nnew"], hkv, d)
    # ---- the caches, cut out of the middle of a larger buffer
    paged = c["addr"].startswith("paged")
    if paged:
        ps = int(c["addr"][5:])
        mb = CAP // ps
        units, n = B * mb + 3, ps
        table = torch.randperm(units, generator=g)[:B * mb].view(B, mb).to(torch.int32)
        if i % 4 == 1:                                      # one page outside the pool: reads as zeros, its append is dropped
            table[int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, mb, (1,), generator=g))] = units + 5
        kw["block_table"] = table
    else:
        units, n = (B + 2 if "bidx" in c["addr"] else B), CAP
        if "bidx" in c["addr"]:
            rows = torch.randperm(units, generator=g)[:B].tolist()
            if i % 4 == 0:                                  # one row outside the cache
                rows[int(torch.randint(0, B, (1,), generator=g))] = units + 3
            kw["cache_batch_idx"] = i32(rows)
        if "leftpad" in c["addr"]:
            kw["cache_leftpad"] = i32([(0, 5, 40, 1000)[int(x)] for x in torch.randperm(4, generator=g)])   # 1000: clamped to L_b
    k_big, v_big = rn(units + 2, n, hkv, d), rn(units + 2, n, hkv, d)
    if c["cache"] == "e4m3":
        # the stored codes: unit-scale values under one scale per head; sequence b reads and appends them under its own scale,
        # a factor away (the smallest factor makes the largest new keys saturate)
        base_k = (k_big.float().abs().amax(dim=(0, 1, 3)) / 448.0).float()
        base_v = (v_big.float().abs().amax(dim=(0, 1, 3)) / 448.0).float()
        k_big, v_big = quantize(k_big, base_k).view(E4M3), quantize(v_big, base_v).view(E4M3)
        f = torch.tensor([0.75, 1.0, 1.5, 2.0])[torch.randint(0, 4, (B, hkv), generator=g)]
        kw["k_descale"], kw["v_descale"] = (base_k.view(1, hkv) * f).contiguous(), (base_v.view(1, hkv) * f.flip(0)).contiguous()
    kw["k_big"], kw["v_big"] = k_big, v_big
    kw["k_cache"], kw["v_cache"] = k_big[1:units + 1], v_big[1:units + 1]
    # ---- rotary, modifiers, sinks
    if c["rotary"] != "off":
        ro_rows = CAP + (max(nq) if packed else max(0, nq[0] - c["nnew"]))
        kw["rotary_cos"], kw["rotary_sin"] = tables(ro_rows, rotary_dim(c["rotary"], d), dtype)
        kw["rotary_interleaved"] = c["rotary"] == "gptj"
    if "softcap" in c["mods"]:
        kw["softcap"] = 15.0 if c["mods"] == "softcap" else 30.0
    if "alibi" in c["mods"]:
        sl = torch.tensor([2.0 ** (-8.0 * (h + 1) / hq) for h in range(hq)], dtype=torch.float32)
        kw["alibi_slopes"] = sl if c["mods"] == "alibi" else (sl.view(1, hq) * torch.arange(1, B + 1).view(B, 1).float()).contiguous()
    if c["sinks"]:
        sk = torch.randn((hq,), generator=g)
        sk[1 % hq], sk[3 % hq] = float("-inf"), 6.0          # one sink that adds nothing, one that outweighs the keys
        kw["sinks"] = sk
    return kw


def call_keywords(kw):
    """kw without the canary buffers: what ex_kvcache_forward and tests.kvcache_full_ref.full_reference take"""
    return {k: v for k, v in kw.items() if k not in ("k_big", "v_big")}
