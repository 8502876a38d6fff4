"""fp64 reference for the rotary KV-cache tests: q and k_new are rotated by the documented formulas, written out with index
arithmetic, rounded once to the tensors' dtype, K is placed in a copy of the cache and tests/kvcache_paged_ref.reference does
the attention.  CPU tensors only.

The finite values of a 16-bit dtype are few enough to list, so the two dtype neighbours of an fp64 value come from a search in
the sorted list: no conversion is involved in that check."""
import torch

from tests.kvcache_paged_ref import paged_tokens, reference

_VALUES = {}


def dtype_values(dtype):
    """every finite value of a 16-bit dtype, ascending, as float64 (-0 and +0 are one entry)"""
    if dtype not in _VALUES:
        bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
        vals = bits.view(dtype).double()
        keep = torch.isfinite(vals) & (bits != -32768)          # drop -0: +0 stands for both
        vals = vals[keep]
        order = torch.argsort(vals)
        _VALUES[dtype] = vals[order].contiguous()
    return _VALUES[dtype]


def neighbours(exact, dtype):
    """(lo, hi) float64: the largest dtype value <= exact and the smallest >= exact"""
    vals = dtype_values(dtype)
    flat = exact.reshape(-1).contiguous()
    hi_i = torch.searchsorted(vals, flat).clamp(max=vals.numel() - 1)
    lo_i = torch.where(vals[hi_i] == flat, hi_i, (hi_i - 1).clamp(min=0))
    return vals[lo_i].view(exact.shape), vals[hi_i].view(exact.shape)


def round_once(exact, dtype):
    """fp64 -> dtype by torch's conversion, which goes through float32.  For bf16 that is the correctly rounded value.  For
    f16 the step through float32 can move an fp64 value onto an f16 tie: about 1 element in 3 * 10^4 of these tests' inputs then
    rounds to the other neighbour than a direct rounding would, and so does every fp32 evaluation of the rotation (its
    products are exact, its sum is the float32 rounding of the fp64 sum).  Both roundings are dtype neighbours of the exact
    value, which is what the tests require of every element."""
    return exact.to(dtype)


def tables(seqlen_ro, rotary_dim, dtype, base=10000.0):
    """cos, sin (seqlen_ro, rotary_dim / 2) of the usual base-10000 frequencies, rounded to dtype"""
    inv = base ** (-torch.arange(0, rotary_dim, 2, dtype=torch.float64) / rotary_dim)
    ang = torch.arange(seqlen_ro, dtype=torch.float64).view(-1, 1) * inv.view(1, -1)
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def pairs(rotary_dim, interleaved):
    """[(index of x, index of y)] of table entry j = 0 .. rotary_dim / 2 - 1"""
    half = rotary_dim // 2
    return [(2 * j, 2 * j + 1) if interleaved else (j, j + half) for j in range(half)]


def rotate64(x, cos, sin, pos, interleaved):
    """x (T, H, d) in the 16-bit dtype, token t at table row pos[t]: the exact rotation in float64 (x' = x c - y s,
    y' = x s + y c); elements at and past rotary_dim pass through"""
    xd = x.double()
    out = xd.clone()
    rows = torch.tensor(list(pos), dtype=torch.long)
    c, s = cos.double()[rows], sin.double()[rows]            # (T, rotary_dim / 2)
    for j, (a, b) in enumerate(pairs(2 * cos.shape[1], interleaved)):
        cj, sj = c[:, j].view(-1, 1), s[:, j].view(-1, 1)
        out[:, :, a] = xd[:, :, a] * cj - xd[:, :, b] * sj
        out[:, :, b] = xd[:, :, a] * sj + xd[:, :, b] * cj
    return out


def clamps(seqlens, leftpad, cap, nnew):
    """L_b and P_b of DESIGN 9f / 9g"""
    L = [min(max(int(x), 0), cap - nnew) for x in seqlens]
    P = [min(max(int(leftpad[i]), 0), L[i]) if leftpad is not None else 0 for i in range(len(L))]
    return L, P


def rotary_reference(q, kc, vc, kn, vn, seqlens, cos, sin, interleaved, causal, window, scale, softcap=0.0, slopes=None,
                     table=None, bidx=None, leftpad=None):
    """The call's o (fp64), lse, the caches after it, and per batch element the exact fp64 rotation of k_new (nnew, H_kv, d).
    kc / vc: (B, cap, H_kv, d), (B_cache, cap, H_kv, d) with bidx, or pools (num_blocks, ps, H_kv, d) with table."""
    b, nq = q.shape[:2]
    nnew, dtype, ps = kn.shape[1], q.dtype, kc.shape[1]
    cap = table.shape[1] * ps if table is not None else kc.shape[1]
    L, P = clamps(seqlens, leftpad, cap, nnew)
    per_token = causal or window[0] >= 0 or window[1] >= 0
    ek, ev = kc.clone(), vc.clone()
    qr = torch.empty_like(q)
    exact = []
    for bb in range(b):
        first = L[bb] - P[bb]
        ex = rotate64(kn[bb], cos, sin, [first + n for n in range(nnew)], interleaved)
        exact.append(ex)
        kr = round_once(ex, dtype)
        qr[bb] = round_once(rotate64(q[bb], cos, sin, [first + (i if per_token else 0) for i in range(nq)], interleaved), dtype)
        for n in range(nnew):
            unit, slot = slot_of(bb, L[bb] + n, table, bidx, ps)
            if 0 <= unit < ek.shape[0]:
                ek[unit, slot] = kr[n]
                ev[unit, slot] = vn[bb, n]
    ks, vs = [], []
    for bb in range(b):
        if table is not None:
            ks.append(paged_tokens(ek, table[bb], L[bb] + nnew, ps))
            vs.append(paged_tokens(ev, table[bb], L[bb] + nnew, ps))
        else:
            row = int(bidx[bb]) if bidx is not None else bb
            ks.append(ek[row, P[bb]:L[bb] + nnew])
            vs.append(ev[row, P[bb]:L[bb] + nnew])
    ro, rlse = reference(qr, ks, vs, causal, window, scale, softcap, slopes)
    return ro, rlse, ek, ev, exact, L, P


def slot_of(bb, t, table, bidx, ps):
    """(cache row or page, position in it) of token t of sequence bb"""
    if table is not None:
        return int(table[bb, t // ps]), t % ps
    return (int(bidx[bb]) if bidx is not None else bb), t


def check_caches(kc, vc, ek, ev, exact, L, kn, rotary_dim, table=None, bidx=None):
    """kc, vc: the caches after the call (CPU).  V and everything in K outside the appended tokens: the expected bits.  The
    appended K: every element one of the two dtype neighbours of the exact value; equal to the reference's rounding except
    on at most 1 in 10^4 of the rotated elements; the pass-through elements k_new's own bits.  Returns the mismatch count."""
    dtype, ps = kc.dtype, kc.shape[1]
    assert torch.equal(vc.view(torch.int16), ev.view(torch.int16)), "V cache"
    same = kc.view(torch.int16) == ek.view(torch.int16)
    inside = torch.zeros(kc.shape[:2], dtype=torch.bool)
    mismatch = rotated = 0
    for bb, ex in enumerate(exact):
        for n in range(ex.shape[0]):
            unit, slot = slot_of(bb, L[bb] + n, table, bidx, ps)
            if not 0 <= unit < kc.shape[0]:
                continue
            inside[unit, slot] = True
            got = kc[unit, slot]
            lo, hi = neighbours(ex[n], dtype)
            gd = got.double()
            assert bool(((gd == lo) | (gd == hi)).all()), f"sequence {bb}, new token {n}: not a neighbour of the exact value"
            assert torch.equal(got[:, rotary_dim:].view(torch.int16), kn[bb, n][:, rotary_dim:].view(torch.int16)), "pass-through"
            mismatch += int((gd[:, :rotary_dim] != ek[unit, slot].double()[:, :rotary_dim]).sum())
            rotated += got.shape[0] * rotary_dim
    assert bool(same[~inside].all()), "K cache outside the appended tokens"
    assert mismatch * 10 ** 4 <= rotated, f"{mismatch} of {rotated} rotated elements differ from the fp64 rounding"
    return mismatch


# ---- the parity cases, shared by the GPU test (which runs them) and the CPU test (which checks on the same inputs that an fp32
# evaluation of the rotation rounds as the fp64 reference does)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
HQ = 8


def _cases():
    out, i = [], 0
    for dt in ("bf16", "f16"):
        for d in (64, 96, 128, 256):
            for rdim in (16, (d // 2) // 16 * 16, d // 16 * 16):
                n = (1, 3, 20)[(i // 2) % 3]
                out.append(dict(dtype=dt, d=d, rdim=rdim, inter=i % 2 == 0, variant=("causal", "window", "none")[i % 3], nq=n, nnew=n,
                                hkv=(8, 2, 1)[(i // 3) % 3], splits=(1, 4, 0)[(i + i // 3) % 3],
                                mode=("contig", "paged16", "idxpad", "paged256")[i % 4], softcap=0.0, alibi=False,
                                spare_rows=7 * (i % 2), wide_tables=i % 5 == 0))
                i += 1
    base = dict(dtype="bf16", d=128, rdim=64, inter=False, variant="causal", nq=1, nnew=1, hkv=2, splits=0, mode="contig", softcap=0.0,
                alibi=False, spare_rows=0, wide_tables=False)
    out.append(dict(base, nq=5, nnew=2))                                   # more q tokens than new keys: positions past the capacity
    out.append(dict(base, nq=2, nnew=6, inter=True, variant="none", mode="paged16", dtype="f16"))
    out.append(dict(base, softcap=30.0, inter=True, splits=4))
    out.append(dict(base, softcap=5.0, variant="window", mode="idxpad", nq=3, nnew=3))
    out.append(dict(base, alibi=True, splits=4, mode="idxpad"))
    out.append(dict(base, alibi=True, inter=True, variant="none", mode="paged256", dtype="f16", nq=3, nnew=3))
    return out


CASES = _cases()
WINDOW = (45, 2)


def case_id(c):
    return "-".join(str(c[k]) for k in ("dtype", "d", "rdim", "variant", "nq", "nnew", "hkv", "splits", "mode")) + \
        ("-gptj" if c["inter"] else "-neox") + ("-cap" if c["softcap"] else "") + ("-alibi" if c["alibi"] else "")


def case_inputs(idx):
    """CPU tensors of parity case idx (seeded by idx).  Four sequences: empty, mid-length, one whose length is above the capacity
    (clamped) and one more; `kv` is the buffer kc and vc are views of (paged256: pool.unbind(1)), else None."""
    c = CASES[idx]
    g = torch.Generator().manual_seed(1000 + idx)
    dtype, d, hkv, nq, nnew = DTYPES[c["dtype"]], c["d"], c["hkv"], c["nq"], c["nnew"]
    rn = lambda *shape: torch.randn(shape, generator=g).to(dtype)   # noqa: E731
    b = 4
    r = dict(c, dtype=dtype, table=None, bidx=None, leftpad=None, kv=None, b=b)
    if c["mode"] in ("paged16", "paged256"):
        ps, mb = (16, 20) if c["mode"] == "paged16" else (256, 2)
        nblk = b * mb + 3
        cap = ps * mb
        if c["mode"] == "paged256":
            r["kv"] = rn(nblk, 2, ps, hkv, d)
            r["kc"], r["vc"] = r["kv"].unbind(1)
        else:
            r["kc"], r["vc"] = rn(nblk, ps, hkv, d), rn(nblk, ps, hkv, d)
        r["table"] = torch.randperm(nblk, generator=g)[:b * mb].view(b, mb).to(torch.int32)      # shuffled pages
    elif c["mode"] == "idxpad":
        cap = 320
        r["kc"], r["vc"] = rn(b + 2, cap, hkv, d), rn(b + 2, cap, hkv, d)
        r["bidx"] = torch.tensor([4, 0, 5, 2], dtype=torch.int32)
        r["leftpad"] = torch.tensor([3, 37, -3, 130], dtype=torch.int32)     # above L_0 = 0 (clamped to it), inside, negative, inside
    else:
        cap = 320
        r["kc"], r["vc"] = rn(b, cap, hkv, d), rn(b, cap, hkv, d)
    r["cap"] = cap
    r["q"], r["kn"], r["vn"] = rn(b, nq, HQ, d), rn(b, nnew, hkv, d), rn(b, nnew, hkv, d)
    r["seqlens"] = torch.tensor([0, 77, cap + 50, 201], dtype=torch.int32)
    seqlen_ro = cap + max(0, nq - nnew) + c["spare_rows"]
    cos, sin = tables(seqlen_ro, c["rdim"], dtype)
    if c["wide_tables"]:     # rows at a stride above rotary_dim / 2
        wide = torch.zeros((2, seqlen_ro, c["rdim"] // 2 + 8), dtype=dtype)
        wide[0, :, :c["rdim"] // 2], wide[1, :, :c["rdim"] // 2] = cos, sin
        cos, sin = wide[0, :, :c["rdim"] // 2], wide[1, :, :c["rdim"] // 2]
    r["cos"], r["sin"] = cos, sin
    r["causal"] = c["variant"] == "causal"
    r["window"] = WINDOW if c["variant"] == "window" else (-1, -1)
    r["slopes"] = torch.tensor([2.0 ** (-8.0 * (h + 1) / HQ) for h in range(HQ)], dtype=torch.float32) if c["alibi"] else None
    return r


def case_reference(r):
    return rotary_reference(r["q"], r["kc"], r["vc"], r["kn"], r["vn"], r["seqlens"], r["cos"], r["sin"], r["inter"], r["causal"],
                            r["window"], r["d"] ** -0.5, r["softcap"], r["slopes"], r["table"], r["bidx"], r["leftpad"])
