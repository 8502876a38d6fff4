"""CPU helpers for the e4m3 KV-cache tests (include/fa_mi355x.h: fa_ex_forward_kvcache_fp8): the append's quantisation recipe
in torch CPU ops, the correctly rounded quantisation by search over the code list, the two codes that bracket the exact
quotient, and the dequantisation to fp64.  Bytes are uint8 throughout; a scale has the shape (B, H_kv) or (H_kv,) and applies
to tensors (B, N, H_kv, d).  CPU tensors only.

The 127 non-negative finite e4m3 values are few enough to list, so the exact rounding is a search in the sorted list: no
conversion is involved in that check."""
import torch

E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
FIXED_SCALES = (1.0, 2.0 ** -5, 0.0137, 3.7, 11.3)

_POS = torch.arange(0, 127, dtype=torch.uint8).view(E4M3).double()      # codes 0x00 .. 0x7e ascending: 0 .. 448


def _rows(descale, x):
    """the scale of every element of x (B, N, H_kv, d): (B, 1, H_kv, 1) or (1, 1, H_kv, 1), float32"""
    ds = torch.as_tensor(descale, dtype=torch.float32)
    if ds.dim() == 0:
        return ds.view(1, 1, 1, 1)
    return ds.view(1, 1, -1, 1) if ds.dim() == 1 else ds.view(ds.shape[0], 1, ds.shape[1], 1)


def absmax_scales(x16, per_batch=True):
    """float32 (B, H_kv) (or (H_kv,)): absmax / 448 of every (b, head) of x16 (B, N, H_kv, d)"""
    a = x16.float().abs().amax(dim=(1, 3) if per_batch else (0, 1, 3))
    return (a / E4M3_MAX).clamp_min(2.0 ** -20).float()


def quantize(x16, descale):
    """uint8 codes by the library's recipe: inv = 1.0f / descale; y = clamp(float(x) * inv, -448, 448) in fp32; e4m3(y) to
    nearest even (torch's cast; past 448 it would give NaN, which the clamp rules out)"""
    inv = torch.tensor(1.0, dtype=torch.float32) / _rows(descale, x16)
    y = (x16.float() * inv).clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(E4M3).view(torch.uint8)


def _exact_quotient(x16, descale):
    return x16.double() / _rows(descale, x16).double()


def neighbours(x16, descale):
    """(lo, hi) uint8: the codes of the largest e4m3 value <= and the smallest >= the exact quotient x / descale, the
    quotient clamped to [-448, 448] first (zero carries the sign of x)"""
    qd = _exact_quotient(x16, descale).clamp(-E4M3_MAX, E4M3_MAX)
    neg = torch.signbit(x16.float())
    mag = qd.abs().reshape(-1).contiguous()
    up = torch.searchsorted(_POS, mag).clamp(max=126)
    dn = torch.where(_POS[up] == mag, up, (up - 1).clamp(min=0))
    sign = (neg.to(torch.uint8) * 128).reshape(-1)
    # for a negative quotient the larger magnitude is the smaller value
    lo = torch.where(neg.reshape(-1), up, dn).to(torch.uint8) | sign
    hi = torch.where(neg.reshape(-1), dn, up).to(torch.uint8) | sign
    return lo.view(x16.shape), hi.view(x16.shape)


def quantize_exact(x16, descale):
    """uint8 codes: the fp64 quotient rounded to nearest, ties to the even code, over the 127 non-negative finite values by
    search; sign restored"""
    qd = _exact_quotient(x16, descale).clamp(-E4M3_MAX, E4M3_MAX)
    mag = qd.abs().reshape(-1).contiguous()
    up = torch.searchsorted(_POS, mag).clamp(max=126)
    dn = torch.where(_POS[up] == mag, up, (up - 1).clamp(min=0))
    d_up, d_dn = _POS[up] - mag, mag - _POS[dn]
    pick = torch.where(d_up < d_dn, up, torch.where(d_dn < d_up, dn, torch.where(up % 2 == 0, up, dn)))
    sign = torch.signbit(x16.float()).to(torch.uint8).reshape(-1) * 128
    return (pick.to(torch.uint8) | sign).view(x16.shape)


def dequantize(cache_u8, descale):
    """fp64: e4m3(c) * descale, for a cache (B, N, H_kv, d) of uint8 codes"""
    return cache_u8.view(E4M3).double() * _rows(descale, cache_u8).double()


def randn16(shape, dtype, seed):
    """seeded randn rounded to the 16-bit dtype: the K / V values the GPU tests quantise"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
