"""fp64 reference and shared cases for the rotary tests (fa_rotary_apply, common/rotary.py): the rotation written out with index
arithmetic in float64 (tests/kvcache_rotary_ref.rotate64), tokens whose position is not a table row passed through, the
conjugate as a rotation by -sin, the result rounded once to the tensor's dtype.  CPU tensors only.

The parity cases are shared by the GPU test, which runs them, and the CPU test, which shows on the same inputs that an fp32
evaluation of the rotation rounds as the fp64 reference does.  Tolerances: every element must be one of the two dtype neighbours
of the exact value (that is what one correct rounding of anything computed from exact products can give at worst through a
float32 sum), and at most 1 in 10^4 of the rotated elements may differ from round_once(fp64), the cap check_caches uses."""
import torch

from tests.kvcache_rotary_ref import neighbours, pairs, rotate64, round_once, tables  # noqa: F401  (re-exported to the tests)

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
BATCH = 3
SEQLEN_RO = 50
EXTRA_HEADS = 2          # heads of the strided buffer that are not part of x (the "v" of a fused projection)
VECTOR_OFFSETS = (-3, 40, 7)     # a negative entry; one that carries a sequence of 37 tokens past SEQLEN_RO = 50


def positions(offset, n):
    return [int(offset) + i for i in range(n)]


def reference64(x, cos, sin, offsets, interleaved, conjugate):
    """x (B, S, H, d) 16-bit; offsets: one position of token 0 per sequence.  Returns (exact fp64 (B, S, H, d), rotated (B, S)
    bool): token i of sequence b is rotated at table row offsets[b] + i iff that is a row of the tables."""
    b, s = x.shape[:2]
    ro = cos.shape[0]
    sgn = -sin if conjugate else sin          # exact in a 16-bit dtype
    exact = x.double().clone()
    rotated = torch.zeros((b, s), dtype=torch.bool)
    for bb in range(b):
        pos = positions(offsets[bb], s)
        keep = [i for i, p in enumerate(pos) if 0 <= p < ro]
        if keep:
            exact[bb, keep] = rotate64(x[bb, keep], cos, sgn, [pos[i] for i in keep], interleaved)
            rotated[bb, keep] = True
    return exact, rotated


def check_rotated(got, x, exact, rotated, rdim):
    """got, x: (B, S, H, d) CPU tensors of one 16-bit dtype.  Every element a dtype neighbour of the exact value; the
    pass-through head dims and the unrotated tokens x's own bits; at most 1 in 10^4 of the rotated elements off the reference's
    rounding.  Returns that mismatch count."""
    dtype = x.dtype
    lo, hi = neighbours(exact, dtype)
    gd = got.double()
    assert bool(((gd == lo) | (gd == hi)).all()), "an element is not a dtype neighbour of the exact value"
    gi, xi = got.view(torch.int16), x.view(torch.int16)
    assert torch.equal(gi[..., rdim:], xi[..., rdim:]), "pass-through head dims"
    assert torch.equal(gi[~rotated], xi[~rotated]), "tokens outside the tables must come back bit-identical"
    want = round_once(exact, dtype)
    mismatch = int((gd[rotated][..., :rdim] != want.double()[rotated][..., :rdim]).sum())
    count = int(rotated.sum()) * x.shape[2] * rdim
    assert mismatch * 10 ** 4 <= count, f"{mismatch} of {count} rotated elements differ from the fp64 rounding"
    return mismatch


def _cases():
    out, i = [], 0
    for dt in ("bf16", "f16"):
        for d in (64, 96, 128, 256):
            for rdim in (16, (d // 2) // 16 * 16, d // 16 * 16):
                for inter in (False, True):
                    for conj in (False, True):
                        out.append(dict(dtype=dt, d=d, rdim=rdim, inter=inter, conj=conj, seqlen=(1, 5, 37)[i % 3],
                                        heads=(1, 3, 8)[(i // 3) % 3], offsets=("zero", "eleven", "vector")[(i + i // 9) % 3],
                                        wide_tables=i % 5 == 0, strided=i % 2 == 1))
                        i += 1
    # every offsets form at the long sequence, where the vector carries tokens past the table, in both layouts
    base = dict(dtype="bf16", d=128, rdim=64, inter=False, conj=False, seqlen=37, heads=3, offsets="vector", wide_tables=False,
                strided=True)
    out.append(base)
    out.append(dict(base, inter=True, conj=True, dtype="f16", strided=False, wide_tables=True))
    out.append(dict(base, offsets="eleven", heads=8, d=256, rdim=256))
    return out


CASES = _cases()


def case_id(c):
    return "-".join(str(c[k]) for k in ("dtype", "d", "rdim", "seqlen", "heads", "offsets")) + ("-gptj" if c["inter"] else "-neox") + \
        ("-conj" if c["conj"] else "") + ("-wide" if c["wide_tables"] else "") + ("-strided" if c["strided"] else "")


def case_inputs(idx):
    """CPU tensors of parity case idx (seeded by idx): `buf` (B, S, heads + EXTRA_HEADS, d) when strided, x = buf[:, :, :heads],
    else x dense; cos / sin (wide: slices of rows 8 entries longer); offsets: an int or an int32 (B,) tensor; pos0: per sequence."""
    c = CASES[idx]
    g = torch.Generator().manual_seed(7000 + idx)
    dtype, d, heads, s = DTYPES[c["dtype"]], c["d"], c["heads"], c["seqlen"]
    r = dict(c, dtype=dtype)
    if c["strided"]:
        r["buf"] = torch.randn((BATCH, s, heads + EXTRA_HEADS, d), generator=g).to(dtype)
        r["x"] = r["buf"][:, :, :heads]
    else:
        r["buf"] = None
        r["x"] = torch.randn((BATCH, s, heads, d), generator=g).to(dtype)
    cos, sin = tables(SEQLEN_RO, c["rdim"], dtype)
    if c["wide_tables"]:
        wide = torch.zeros((2, SEQLEN_RO, c["rdim"] // 2 + 8), dtype=dtype)
        wide[0, :, :c["rdim"] // 2], wide[1, :, :c["rdim"] // 2] = cos, sin
        r["wide"] = wide
        cos, sin = wide[0, :, :c["rdim"] // 2], wide[1, :, :c["rdim"] // 2]
    r["cos"], r["sin"] = cos, sin
    if c["offsets"] == "vector":
        r["offsets"] = torch.tensor(VECTOR_OFFSETS, dtype=torch.int32)
        r["pos0"] = list(VECTOR_OFFSETS)
    else:
        r["offsets"] = 0 if c["offsets"] == "zero" else 11
        r["pos0"] = [r["offsets"]] * BATCH
    return r


# ---- a model of the kernel's thread-to-chunk map (csrc/fa_rotary.hip: a unit is what one thread moves per step)
def unit_model(u, d, rdim, interleaved, inplace):
    """Unit u of a head row: (kind, the chunks it reads, the chunks it writes); a chunk c is head dims 8 c .. 8 c + 7.  Rotating
    units come first (interleaved: one self-contained chunk; otherwise the chunk below rotary_dim / 2 and its partner), then,
    out of place only, one copying unit per pass-through chunk."""
    nrot = rdim // 8 if interleaved else rdim // 16
    units = nrot + (0 if inplace else (d - rdim) // 8)
    assert 0 <= u < units
    if u >= nrot:
        c = rdim // 8 + (u - nrot)
        return "copy", [c], [c]
    if interleaved:
        return "rotate", [u], [u]
    return "rotate", [u, u + rdim // 16], [u, u + rdim // 16]


def unit_count(d, rdim, interleaved, inplace):
    return (rdim // 8 if interleaved else rdim // 16) + (0 if inplace else (d - rdim) // 8)


def span(cu, b, total, max_seqlen):
    """(start, len) of sequence b of a packed tensor: the clamp of the varlen forward, which the kernel restates"""
    a = min(max(int(cu[b]), 0), total)
    e = min(max(int(cu[b + 1]), a), total)
    return a, min(e - a, max_seqlen)
