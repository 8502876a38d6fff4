"""CPU reference of the lightning indexer (include/fa_mi355x.h: fa_indexer_pack, fa_indexer_logits, fa_indexer_topk;
flashattention-pytorch_amd/csrc/fa_indexer.hip).  Torch on CPU tensors only; it never imports the extension.

A call is a dict: q8 uint8 (B, Nq, H, 128) e4m3 codes, w float32 (B, Nq, H), k8 uint8 (B, L, 128) and ks float32 (B, L) the
sequences' keys and scales in token order (what the pool holds behind the table; a key on a page outside the pool is a zero row with
scale 0), lens (the clamped lengths), causal.  Key j of sequence b is visible to token i iff 0 <= j < len_b and, if causal,
j <= len_b - Nq + i.

    reference(call)   float64 (B, Nq, L):  sum_h w[h] * max(0, q[h] . (e4m3_value(k8) * ks)), every product and sum in fp64
    baseline(call)    the same closed form with the kernel's rounding points, in the kernel's order.  Each step names its line of
                      idx_logits_kernel (csrc/fa_indexer.hip, the tags [L1] .. [L5] of its header comment and of the code):
        [L1]  p[h] = q[h] . k8: fp8_ref._mfma_f8, two 64-term instructions over bytes 0 .. 63 and 64 .. 127, its truncation, the fp32
              accumulator from 0.  (A lane's register bytes are bytes 64 M + 32 kk + 16 c .. of the row: the instruction's groups of 8
              consecutive k are 8 consecutive bytes of the row, the grouping of order=None.)
        [L2]  r[h] = max(p[h], 0)
        [L3]  for each lane half c = 0, 1: s_c = 0; s_c = fma(w[h], r[h], s_c) in fp32 over h = 32 hb + (i & 3) + 8 (i >> 2) + 4 c,
              hb = 0 .. H / 32 - 1 outside, i = 0 .. 15 inside
        [L4]  t = s_0 + s_1, one fp32 add
        [L5]  logit = t * ks, one fp32 multiply: the scale once, after the head sum
      baseline(call, torch.float64, rounding=False) is the reference in another order of summation.
    select(bits, n, topk)   the exact model of the selection: a sort of (key, position) pairs
    pack(x, scale_pow2)     the quantiser of the append, bit for bit
    MUTANTS                 wrong kernels the tests must tell from the right one

Both results hold NaN where the entry is not visible (the kernel does not write there)."""
import itertools
import random

import torch

from tests import fp8_ref

D, TOKEN_BYTES, SCALE_AT = 128, 132, 128
E4M3_MAX = 448.0
BAND = 256   # the sharp bar is taken per (sequence, 256-key band)


def head_order(heads, half):
    """the heads lane half `half` sums, in its order ([L3])"""
    return [32 * hb + (i & 3) + 8 * (i >> 2) + 4 * half for hb in range(heads // 32) for i in range(16)]


def visible(call, bound_shift=0, top_left=False):
    """bool (B, Nq, L)"""
    b, nq = call["q8"].shape[:2]
    cap = call["k8"].shape[1]
    j = torch.arange(cap).view(1, 1, cap)
    i = torch.arange(nq).view(1, nq, 1)
    lens = torch.tensor(call["lens"]).view(b, 1, 1)
    vis = (j < lens).expand(b, nq, cap).clone()
    if call["causal"]:
        vis &= (j <= i + bound_shift) if top_left else (j <= lens - nq + i + bound_shift)
    return vis


def reference(call):
    q = fp8_ref.e4m3_value(call["q8"]).double()                                  # (B, Nq, H, 128)
    k = fp8_ref.e4m3_value(call["k8"]).double() * call["ks"].double().unsqueeze(-1)   # (B, L, 128)
    p = torch.einsum("bihd,bjd->bihj", q, k)
    out = (call["w"].double().unsqueeze(-1) * p.clamp_min(0.0)).sum(2)
    return torch.where(visible(call), out, torch.full_like(out, float("nan")))


def _products(call, ct, rounding, rows=64):
    """[L1]: (B, Nq, H, L) in ct"""
    q = fp8_ref.e4m3_value(call["q8"])
    k = fp8_ref.e4m3_value(call["k8"])
    b, nq, h, _d = q.shape
    cap = k.shape[1]
    out = torch.empty((b, nq, h, cap), dtype=ct)
    for bi in range(b):
        kt = k[bi].t().contiguous()                                             # (128, L)
        qa = q[bi].reshape(nq * h, D)
        res = out[bi].view(nq * h, cap)
        for r0 in range(0, nq * h, rows):
            a = qa[r0:r0 + rows]
            res[r0:r0 + rows] = fp8_ref._mfma_f8(a, kt, ct, torch.zeros((a.shape[0], cap), dtype=ct), truncate=rounding)
    return out


def baseline(call, compute=torch.float32, rounding=True, mutant=None):
    ct = compute
    h = call["q8"].shape[2]
    p = _products(call, ct, rounding)                                           # [L1]
    w = call["w"].to(ct)
    ks = call["ks"].to(ct)
    if mutant == "scale_of_previous_token":
        ks = torch.cat([ks[:, :1], ks[:, :-1]], dim=1)
    halves = []
    for c in range(2):
        s = torch.zeros_like(p[:, :, 0, :])
        for hd in head_order(h, c):                                             # [L3]
            wh = w[:, :, hd % 32 if mutant == "weight_of_head_mod_32" else hd].unsqueeze(-1)
            r = p[:, :, hd, :] if mutant == "relu_after_sum" else p[:, :, hd, :].clamp_min(0.0)   # [L2]
            s = (wh.double() * r.double() + s.double()).to(ct)                  # (the product is exact in fp64: one rounding to ct)
        halves.append(s)
    t = (halves[0].double() + halves[1].double()).to(ct)                        # [L4]
    if mutant == "relu_after_sum":
        t = t.clamp_min(0.0)
    out = (t.double() * ks.unsqueeze(1).double()).to(ct)                        # [L5]
    vis = visible(call)
    if mutant == "bound_off_by_one":
        vis = visible(call, bound_shift=-1)
    elif mutant == "bound_top_left":
        vis = visible(call, top_left=True)
    elif mutant == "tail_dropped":
        lens = torch.tensor(call["lens"]).view(-1, 1, 1)
        vis = vis & (torch.arange(call["k8"].shape[1]).view(1, 1, -1) < lens - lens % 32)
    return torch.where(vis, out, torch.full_like(out, float("nan")))


LOGIT_MUTANTS = ("relu_after_sum", "weight_of_head_mod_32", "scale_of_previous_token", "bound_off_by_one", "bound_top_left", "tail_dropped")
SELECT_MUTANTS = ("ties_to_highest", "zeros_equal", "pad_zero")
MUTANTS = LOGIT_MUTANTS + SELECT_MUTANTS


def band_errors(x, ref, lens):
    """[(sequence, band, max |x - ref|, max |ref|)] over the visible entries of every (sequence, 256-key band); an entry that is
    visible in one and not in the other counts as an infinite error; one entry a band"""
    out = []
    for b, n in enumerate(lens):
        for k0 in range(0, n, BAND):
            xs, rs = x[b, :, k0:min(k0 + BAND, n)].double(), ref[b, :, k0:min(k0 + BAND, n)]
            vis = ~torch.isnan(rs)
            big = rs[vis].abs().max().item() if bool(vis.any()) else 0.0
            if bool((torch.isnan(xs) != ~vis).any()):
                out.append((b, k0 // BAND, float("inf"), big))
            else:
                out.append((b, k0 // BAND, (xs[vis] - rs[vis]).abs().max().item() if bool(vis.any()) else 0.0, big))
    return out


def sharp_bar(got, ref, base, lens):
    """failures of  max |got - fp64| <= 2 * max |baseline - fp64| + eps_f32 * max |fp64|  per (sequence, 256-key band): the rule of
    tests/ex_full_ref.sharp_bar with float32's eps"""
    eps = torch.finfo(torch.float32).eps
    bad = []
    for (b, band, err, big), (_b, _band, eb, _big) in zip(band_errors(got, ref, lens), band_errors(base, ref, lens)):
        bound = 2.0 * eb + eps * big
        if not err <= bound:
            bad.append(f"sequence {b} band {band}: max |got - fp64| = {err:.3e} > 2 * {eb:.3e} (baseline) + {eps:.1e} * {big:.3e} = {bound:.3e}")
    return bad


# ---- the selection
def order_key(bits):
    """the unsigned order key of float32 bit patterns (int64 tensor or int)"""
    bits = bits & 0xFFFFFFFF
    return bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)


def select(row_bits, n, topk, mutant=None):
    """indices (list of topk ints) of one row: row_bits the float32 bit patterns (ints) of at least n entries, the visible keys being
    0 .. n - 1.  The min(topk, n) largest by (key descending, position ascending), in ascending position order, then -1."""
    def key(j):
        k = order_key(int(row_bits[j]))
        if mutant == "zeros_equal" and k == order_key(0x80000000):
            k = order_key(0)
        return k
    take = min(topk, n)
    if n <= topk:
        chosen = list(range(n))
    else:
        order = sorted(range(n), key=lambda j: (-key(j), -j if mutant == "ties_to_highest" else j))
        chosen = sorted(order[:take])
    return chosen + [0 if mutant == "pad_zero" else -1] * (topk - take)


def visible_count(length, nq, i, causal, width):
    n = min(max(int(length), 0), width)
    return min(max(n - nq + i + 1, 0), n) if causal else n


def select_all(logits, lens, topk, causal, mutant=None):
    """int32 (B, Nq, topk) of float32 logits (B, Nq, width): `select` row by row -- for a row with more visible keys than topk and no
    mutant through a stable descending torch.sort of the keys, which leaves equal keys in ascending position order (the CPU tests
    hold it against `select`)"""
    b, nq, width = logits.shape
    bits = logits.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    keys = bits ^ torch.where((bits >> 31) != 0, torch.full_like(bits, 0xFFFFFFFF), torch.full_like(bits, 0x80000000))
    out = torch.full((b, nq, topk), -1, dtype=torch.int32)
    for bi in range(b):
        for i in range(nq):
            n = visible_count(lens[bi], nq, i, causal, width)
            if mutant is not None:
                out[bi, i] = torch.tensor(select(bits[bi, i, :n].tolist(), n, topk, mutant), dtype=torch.int32)
            elif n <= topk:
                out[bi, i, :n] = torch.arange(n, dtype=torch.int32)
            else:
                order = torch.sort(keys[bi, i, :n], descending=True, stable=True).indices[:topk]
                out[bi, i] = torch.sort(order).values.to(torch.int32)
    return out


# ---- the append
def pack(x, scale_pow2=False):
    """(uint8 (.., 128) codes, float32 (..,) scales) of bf16 (.., 128) rows: scale = amax / 448 (1 for a zero row; scale_pow2: up to
    the next power of two), byte = e4m3_rne(clamp(x / scale, +-448)), in fp32 from the exact bf16 values.  Every division has a
    tensor divisor: the IEEE fp32 division element by element."""
    assert x.dtype == torch.bfloat16 and x.shape[-1] == D
    xf = x.float()
    amax = xf.abs().amax(-1)
    scale = torch.where(amax > 0, amax / torch.full_like(amax, E4M3_MAX), torch.ones_like(amax))
    if scale_pow2:
        m, e = torch.frexp(scale)                       # scale = m * 2^e, m in [0.5, 1)
        scale = torch.where(m == 0.5, scale, torch.ldexp(torch.ones_like(scale), e))
    y = (xf / scale.unsqueeze(-1).expand_as(xf)).clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), scale


def token_bytes(codes, scale):
    """uint8 (.., 132) tokens"""
    out = torch.empty((*codes.shape[:-1], TOKEN_BYTES), dtype=torch.uint8)
    out[..., :SCALE_AT] = codes
    out[..., SCALE_AT:] = scale.contiguous().view(torch.uint8).reshape(*scale.shape, 4)
    return out


def scatter(pool, tokens, lens_before, table, page):
    """the append's mapping: pool uint8 (num_blocks, page, 1, W) (modified in place and returned), tokens uint8 (B, N_new, 132); a
    negative length, a position at or past the table's capacity or a page outside the pool drops the token"""
    nblk = pool.shape[0]
    b, nnew = tokens.shape[:2]
    for bi in range(b):
        for i in range(nnew):
            ln = int(lens_before[bi])
            pos = ln + i
            if ln < 0 or pos >= table.shape[1] * page:
                continue
            pg = int(table[bi, pos // page])
            if 0 <= pg < nblk:
                pool[pg, pos % page, 0, :TOKEN_BYTES] = tokens[bi, i]
    return pool


# ---- the sweep (the pairwise generator of tests/kvcache_sweep_cases.py: greedy, best of `tries` candidates, a fixed seed)
# lens: three lengths from {0, 1, 31, 32, 33, 130, 257, 1000}; each triple has one below most Nq, and (1000, 0, 33) one below every Nq
AXES = dict(heads=(32, 64), nq=(1, 2, 5, 70), lens=((1000, 0, 33), (257, 1, 130), (31, 32, 1)), page=(16, 48, 256), causal=(True, False),
            stride=(144, 208))
NAMES = tuple(AXES)
SEED, MAX_CASES = 20251, 16


def generate(axes=AXES, seed=SEED, tries=40):
    rng = random.Random(seed)
    names = tuple(axes)
    uncovered = {((a, va), (b, vb)) for a, b in itertools.combinations(names, 2) for va in axes[a] for vb in axes[b]}
    cases = []

    def pair(a, va, b, vb):   # the two in the axes' order
        return ((a, va), (b, vb)) if names.index(a) < names.index(b) else ((b, vb), (a, va))

    while uncovered:
        best, best_gain = None, -1
        for _ in range(tries):
            (a, va), (b, vb) = rng.choice(sorted(uncovered, key=repr))
            c = {a: va, b: vb}
            rest = [n for n in names if n not in c]
            rng.shuffle(rest)
            for n in rest:
                vals = list(axes[n])
                rng.shuffle(vals)
                c[n] = max(vals, key=lambda v: sum(pair(n, v, m, c[m]) in uncovered for m in c))
            gain = sum(((a2, c[a2]), (b2, c[b2])) in uncovered for a2, b2 in itertools.combinations(names, 2))
            if gain > best_gain:
                best, best_gain = c, gain
        cases.append({n: best[n] for n in names})
        uncovered -= {((a2, best[a2]), (b2, best[b2])) for a2, b2 in itertools.combinations(names, 2)}
    return cases


CASES = generate()
B = 3


def build_call(case, seed):
    """The call of a case: q from a normal draw quantised to e4m3, weights of mixed sign around H^-1/2 d^-1/2, keys whose norm grows
    along the sequence quantised by `pack`.  The capacity is the longest length rounded up to whole pages."""
    g = torch.Generator().manual_seed(seed)
    h, nq, page = case["heads"], case["nq"], case["page"]
    lens = list(case["lens"])
    cap = max(page, -(-max(lens) // page) * page)
    q = torch.randn((B, nq, h, D), generator=g).clamp(-E4M3_MAX, E4M3_MAX)
    q8 = fp8_ref.e4m3_code(q)
    w = torch.randn((B, nq, h), generator=g) * (h ** -0.5 * D ** -0.5)
    grow = 0.25 + 4.0 * torch.arange(cap).float() / max(cap - 1, 1)
    k = (torch.randn((B, cap, D), generator=g) * grow.view(1, cap, 1)).to(torch.bfloat16)
    k8, ks = pack(k)
    return dict(q8=q8, w=w, k8=k8, ks=ks, lens=lens, causal=case["causal"], k_bf16=k, page=page, stride=case["stride"], cap=cap)


def paged(call, seed, extra_pages=2):
    """(pool uint8 (num_blocks, page, 1, stride) filled with 0x7F outside the tokens' 132 bytes, table int32 (B, max_blocks)): the
    call's keys on shuffled pages"""
    rng = random.Random(seed)
    page, cap, stride = call["page"], call["cap"], call["stride"]
    mb = cap // page
    nblk = B * mb + extra_pages
    ids = list(range(nblk))
    rng.shuffle(ids)
    table = torch.tensor(ids[:B * mb], dtype=torch.int32).view(B, mb)
    pool = torch.full((nblk, page, 1, stride), 0x7F, dtype=torch.uint8)
    toks = token_bytes(call["k8"], call["ks"])                                   # (B, cap, 132)
    for b in range(B):
        for j in range(mb):
            pool[int(table[b, j]), :, 0, :TOKEN_BYTES] = toks[b, j * page:(j + 1) * page]
    return pool, table
