"""The contract of the fp8 quantiser (include/fa_mi355x.h: fa_fp8_quantize; common.attention_ex.quantize_fp8) in torch on the CPU,
in float32 with IEEE operations only, so that the GPU result must agree with it bit for bit:

    amax[b, j]    = max |float(x)| over heads [j g, (j + 1) g) x the tokens of sequence b x d        (exact)
    descale[b, j] = amax > 0 ? amax / 448 : 1                                                          (one IEEE division)
    pow2          : a descale whose mantissa is not zero goes to the next exponent, in the bit pattern
    inv           = 1 / descale                                                                        (one IEEE division)
    code          = e4m3_rne(clamp(float(x) * inv, -448, 448))        (one IEEE product; torch's cast rounds to nearest even)

and the fused rotation in fp32 from the 16-bit inputs, rounded once to x's dtype before anything else looks at it.  Both products
of a rotated element are exact in fp32 (8 x 8 or 11 x 11 significant bits), so their float32 sum is the correctly rounded exact
value whichever way it is evaluated.  CPU tensors only; the canonical layout is (B, N, H, d)."""
import torch

E4M3_MAX = 448.0


def span(cu, b, total, max_seqlen):
    """(start, len) of sequence b of a packed tensor: seq_span (csrc/fa_ex_common.h), the clamp of the varlen forward"""
    a = min(max(int(cu[b]), 0), total)
    e = min(max(int(cu[b + 1]), a), total)
    return a, min(e - a, max_seqlen)


def pow2_up(descale):
    """fa_mla_fp8_pack's rule, restated: the next power of two at or above a positive normal float32, in the bit pattern"""
    bits = descale.contiguous().view(torch.int32)
    up = (bits & 0x7F800000) + 0x00800000
    return torch.where((bits & 0x007FFFFF) != 0, up, bits).view(torch.float32)


def descale_of(amax, scale_pow2=False):
    amax = amax.float()
    ds = torch.where(amax > 0, amax / torch.full_like(amax, E4M3_MAX), torch.ones_like(amax))
    return pow2_up(ds) if scale_pow2 else ds


def unit_amax(x, g):
    """x (B, N, H, d) -> float32 (B, H / g): the maximum of |x| over each scale unit; 0 for a unit without tokens"""
    b, n, h, d = x.shape
    if n == 0:
        return torch.zeros((b, h // g), dtype=torch.float32)
    return x.float().abs().reshape(b, n, h // g, g * d).amax(dim=(1, 3))


def codes_of(x, descale, g):
    """uint8 e4m3 codes of x (B, N, H, d) under descale (B, H / g)"""
    inv = torch.ones_like(descale) / descale
    y = x.float() * inv.repeat_interleave(g, dim=1)[:, None, :, None]
    return y.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def quantize_model(x, g=1, descale=None, scale_pow2=False):
    """(codes uint8 (B, N, H, d), descale float32 (B, H / g)) of a 16-bit x (B, N, H, d); descale given ((B, H / g) or (H / g,)):
    the static mode"""
    b, _n, h, _d = x.shape
    if descale is None:
        descale = descale_of(unit_amax(x, g), scale_pow2)
    else:
        descale = descale.float().expand(b, h // g).contiguous()
    return codes_of(x, descale, g), descale


def rotate32(x, cos, sin, pos0, interleaved):
    """x (B, N, H, d) 16-bit, cos / sin (seqlen_ro, rotary_dim / 2) in x's dtype, pos0: the position of token 0 per sequence.  Token
    i of sequence b is rotated at table row pos0[b] + i iff that is a row of the tables, else passed through; fp32 arithmetic, one
    rounding to x's dtype."""
    b, n = x.shape[:2]
    ro, half = cos.shape
    rdim = 2 * half
    out = x.clone()
    for bb in range(b):
        pos = torch.arange(n) + int(pos0[bb])
        keep = (pos >= 0) & (pos < ro)
        if not bool(keep.any()):
            continue
        xs = x[bb, keep].float()                                   # (n', H, d)
        c, s = cos[pos[keep]].float()[:, None, :], sin[pos[keep]].float()[:, None, :]
        if interleaved:
            a, p = xs[..., 0:rdim:2], xs[..., 1:rdim:2]
        else:
            a, p = xs[..., :half], xs[..., half:rdim]
        ra, rp = a * c - p * s, a * s + p * c
        rot = xs.clone()
        if interleaved:
            rot[..., 0:rdim:2], rot[..., 1:rdim:2] = ra, rp
        else:
            rot[..., :half], rot[..., half:rdim] = ra, rp
        out[bb, keep] = rot.to(x.dtype)
    return out


def tables(seqlen_ro, rdim, dtype, base=10000.0):
    inv_freq = 1.0 / (base ** (torch.arange(0, rdim, 2, dtype=torch.float64) / rdim))
    ang = torch.arange(seqlen_ro, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return ang.cos().to(dtype), ang.sin().to(dtype)


# ---- inputs
VALUES = ("normal", "outlier", "zero_units", "ties")


def make_x(kind, shape, g, dtype, seed):
    """x (B, N, H, d) of one value pattern.  normal: randn.  outlier: one element of every scale unit 1000 times larger, which
    sends most of the rest into e4m3's subnormals and zeros.  zero_units: every other unit all zero (descale 1, codes 0).  ties:
    (1 + m / 16) 2^e with e in [-10, 7], both signs, and one 448 per unit, so that descale = inv = 1 exactly and every value with an
    odd m sits exactly half way between two e4m3 codes (the subnormal ones included): round to nearest EVEN decides each of them."""
    b, n, h, d = shape
    gen = torch.Generator().manual_seed(seed)
    if kind == "ties":
        m = torch.randint(0, 16, shape, generator=gen).float()
        e = torch.randint(-10, 8, shape, generator=gen).float()
        sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
        x = sign * (1 + m / 16) * torch.exp2(e)
    else:
        x = torch.randn(shape, generator=gen)
    u = x.reshape(b, n, h // g, g, d)
    for bb in range(b):
        for j in range(h // g):
            if n == 0:
                continue
            i, hh, e = (int(torch.randint(0, k, (1,), generator=gen)) for k in (n, g, d))
            if kind == "outlier":
                u[bb, i, j, hh, e] *= 1000.0
            elif kind == "zero_units" and (bb + j) % 2 == 0:
                u[bb, :, j] = 0.0
            elif kind == "ties":
                u[bb, i, j, hh, e] = E4M3_MAX
    return x.to(dtype)


def odd_mantissa(x):
    """float32 x with the last mantissa bit set: a descale whose reciprocal and quotients are not exact"""
    return (x.float().contiguous().view(torch.int32) | 1).view(torch.float32)


def static_descales(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return odd_mantissa(2.0 ** -7 * 16.0 ** torch.rand(shape, generator=gen))
