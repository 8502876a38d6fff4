"""CPU reference of the packed 8-bit latent cache (include/fa_mi355x.h: fa_mla_fp8_pack, fa_mla_fp8_forward), FlashMLA's 656-byte
token

    byte   0 .. 511   512 x float8_e4m3fn   the latent, quantised per 128-wide tile
    byte 512 .. 527   4 x float32           one scale per tile:  value = float(e4m3) * scale
    byte 528 .. 655   64 x bfloat16         the rotary part, not quantised

pack_rows is the quantiser of the append, unpack_rows the read contract of the decode kernels, scatter_rows the append's mapping of
new tokens to pool slots with its drop rules.  Torch on CPU tensors only; it never imports the extension.  Every division has a
tensor divisor, so that it is the IEEE fp32 division element by element (tests/test_mla_fp8_cpu.py checks it against numpy)."""
import torch

LATENT, ROPE, TILE, TOKEN_BYTES = 512, 64, 128, 656
SCALES_AT, ROPE_AT = 512, 528
E4M3_MAX = 448.0


def tile_scales(latent, scale_pow2=False):
    """float32 (.., 4): amax / 448 of every 128-wide tile of a bf16 (.., 512) latent, 1 for an all-zero tile; scale_pow2: rounded up
    to the next power of two"""
    x = latent.float().reshape(*latent.shape[:-1], LATENT // TILE, TILE)
    amax = x.abs().amax(-1)
    scale = torch.where(amax > 0, amax / torch.full_like(amax, E4M3_MAX), torch.ones_like(amax))
    if scale_pow2:
        m, e = torch.frexp(scale)                       # scale = m * 2^e, m in [0.5, 1)
        scale = torch.where(m == 0.5, scale, torch.ldexp(torch.ones_like(scale), e))
    return scale


def pack_rows(latent, rope, scale_pow2=False):
    """uint8 (.., 656) of bf16 latent (.., 512) and rope (.., 64): byte = e4m3_rne(clamp(x / scale, +-448)) in fp32 from the exact
    bf16 values, the four scales, the rope bytes as they are"""
    assert latent.dtype == torch.bfloat16 and rope.dtype == torch.bfloat16
    assert latent.shape[-1] == LATENT and rope.shape[-1] == ROPE and latent.shape[:-1] == rope.shape[:-1]
    lead = latent.shape[:-1]
    scale = tile_scales(latent, scale_pow2)
    x = latent.float().reshape(*lead, LATENT // TILE, TILE)
    y = (x / scale.unsqueeze(-1).expand_as(x)).clamp(-E4M3_MAX, E4M3_MAX)
    out = torch.empty((*lead, TOKEN_BYTES), dtype=torch.uint8)
    out[..., :SCALES_AT] = y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(*lead, LATENT)
    out[..., SCALES_AT:ROPE_AT] = scale.contiguous().view(torch.uint8).reshape(*lead, 16)
    out[..., ROPE_AT:] = rope.contiguous().view(torch.uint8).reshape(*lead, 2 * ROPE)
    return out


def unpack_rows(rows):
    """(latent bf16 (.., 512), rope bf16 (.., 64)) of uint8 (.., >= 656) rows by the read contract: bf16_rne(float(e4m3) * scale),
    one fp32 multiply and one rounding; the rope as stored"""
    assert rows.dtype == torch.uint8 and rows.shape[-1] >= TOKEN_BYTES
    lead = rows.shape[:-1]
    c = rows[..., :SCALES_AT].contiguous().view(torch.float8_e4m3fn).float().reshape(*lead, LATENT // TILE, TILE)
    scale = rows[..., SCALES_AT:ROPE_AT].contiguous().view(torch.float32).reshape(*lead, LATENT // TILE)
    latent = (c * scale.unsqueeze(-1)).to(torch.bfloat16).reshape(*lead, LATENT)
    rope = rows[..., ROPE_AT:TOKEN_BYTES].contiguous().view(torch.bfloat16).reshape(*lead, ROPE)
    return latent, rope


def unpack_pool(pool):
    """bf16 (num_blocks, page, 1, 576) [latent | rope] of a packed uint8 (num_blocks, page, 1, >= 656) pool: the 16-bit pool whose
    slices [..., 512:] and [..., :512] are k_cache and v_cache of the 16-bit calls"""
    latent, rope = unpack_rows(pool)
    return torch.cat([latent, rope], dim=-1)


def scatter_rows(pool, rows, cache_seqlens, block_table):
    """Write rows (B, N_new, 656) uint8 into a copy of pool (num_blocks, page, 1, >= 656): token i of sequence b at position
    cache_seqlens[b] + i, slot pos % page of page block_table[b, pos // page].  Dropped, nothing written: a negative length, a
    position at or past the table's capacity, a page outside the pool.  Returns (the new pool, the list of dropped (b, i))."""
    out = pool.clone()
    nblk, ps = pool.shape[:2]
    mb = block_table.shape[1]
    dropped = []
    for b in range(rows.shape[0]):
        for i in range(rows.shape[1]):
            ln = int(cache_seqlens[b])
            pos = ln + i
            if ln < 0 or pos >= mb * ps:
                dropped.append((b, i))
                continue
            pg = int(block_table[b, pos // ps])
            if not 0 <= pg < nblk:
                dropped.append((b, i))
                continue
            out[pg, pos % ps, 0, :TOKEN_BYTES] = rows[b, i]
    return out, dropped
