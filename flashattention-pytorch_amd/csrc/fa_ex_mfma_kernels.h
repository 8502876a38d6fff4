// The three kernels of the extended 16-bit MFMA family and the device helpers they use, for the three translation units that
// instantiate them (fa_ex_mfma.hip: every 16-bit call; fa_ex_mfma_kv8.hip: the kFeatKv8 instantiations of the forward;
// fa_ex_mfma_bias.hip: the kFeatBias instantiations of all three, whose header says what the bit changes):
//   exm_fwd_kernel<Tag, D, FEAT>, exm_dkdv_kernel<Tag, D, FEAT, M16>, exm_dq_kernel<Tag, D, FEAT>.
// fa_ex_mfma.hip's header says what each FEAT bit stands for.  The parameter block (ExB<FEAT>) and the type K and V are addressed
// by (ExKV<FEAT>) are functions of FEAT alone, so every instantiation is one function of its own, as when each parameter block
// had a __global__ shell around a textually included body; a feature a FEAT lacks is a discarded `if constexpr` branch.
// The existing instantiations are touchy about how this text is written (profiles/exm_refactor.md): flags go into plain ternaries,
// not into lambdas, and the dma_wait_all(); __syncthreads(); pairs of the 16-bit pools stay literal.  tools/kernel_diff.py
// compares the instruction text of two builds.
#pragma once
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_ex_mfma_feat.h"
#include "fa_kernels.h"

namespace fa {

namespace {

// Which tiles does the block-sparse mask leave alive?  A workgroup walks tiles along ONE axis (key tiles of T keys in
// the forward and dQ kernels, query tiles of T rows in the dK/dV kernel) against a fixed range of the other axis.  One
// probe = one byte load per lane + a ballot, and covers TP = 64 / E consecutive tiles, E = block-mask entries a tile can
// touch (at most 32: tiles are at most 256 x 128, blocks at least 32 x 32); the window is kept in scalar registers, so
// next() costs a probe only every TP tiles (128 x 128 blocks: every 32 key tiles).  All results are wave-uniform.
template <bool KEYS_VARY, int T>
struct LiveScan {
    const uint8_t* bm;
    int nbc, blk_var, blk_fix;     // block size along the walked / the fixed axis
    int fb0, nfix;                 // first block and number of blocks of the fixed range
    int nvar, E, TP;               // blocks of the walked axis a tile can touch; entries per tile; tiles per probe
    int origin, alim, ntiles;      // tile t covers [origin + t T, origin + (t + 1) T) clipped to alim
    int base;                      // first tile of the cached window (-1: none)
    unsigned long long bits;
    int lane;

    __device__ __forceinline__ void init(const ExParams& p, int f0, int f1, int origin_, int alim_, int ntiles_, int lane_) {
        bm = p.bmask; nbc = p.nbc;
        blk_var = KEYS_VARY ? p.bc : p.br;
        blk_fix = KEYS_VARY ? p.br : p.bc;
        fb0 = f0 / blk_fix;
        nfix = (f1 - 1) / blk_fix - fb0 + 1;
        nvar = (T % blk_var == 0) ? T / blk_var : ((blk_var % T == 0 && origin_ % T == 0) ? 1 : (T - 1) / blk_var + 2);
        E = nfix * nvar;
        TP = 64 / E;
        origin = origin_; alim = alim_; ntiles = ntiles_; lane = lane_;
        base = -1; bits = 0;
    }
    __device__ __forceinline__ void probe(int t0) {
        const int tau = lane / E, e = lane - tau * E;
        const int iv = e / nfix, jf = e - iv * nfix;
        const int tile = t0 + tau;
        bool hit = false;
        if (tau < TP && tile < ntiles) {
            const int a0 = origin + tile * T;
            const int vb0 = a0 / blk_var, vb1 = (min(a0 + T, alim) - 1) / blk_var;
            if (vb0 + iv <= vb1) hit = (KEYS_VARY ? bm[(fb0 + jf) * nbc + vb0 + iv] : bm[(vb0 + iv) * nbc + fb0 + jf]) != 0;
        }
        bits = __ballot(hit);
        base = t0;
    }
    // first live tile >= t (ntiles if none)
    __device__ __forceinline__ int next(int t) {
        const unsigned long long emask = E >= 64 ? ~0ull : ((1ull << E) - 1ull);
        while (t < ntiles) {
            if (base < 0 || t < base || t >= base + TP) probe(t);
            if ((bits >> ((t - base) * E)) & emask) return t;
            ++t;
        }
        return t;
    }
};

struct MaskSrc {
    buf_rsrc_t rs;
    bool on, dwords, quads;
};
__device__ __forceinline__ MaskSrc make_mask_src(const ExParams& p, int bh) {
    MaskSrc m;
    m.on = p.mask != nullptr;
    const uint8_t* base = m.on ? p.mask + (size_t)bh * p.mask_bh : nullptr;
    m.rs = make_rsrc(base, m.on ? (unsigned)p.nq * (unsigned)p.nk : 0u);
    m.dwords = m.on && (p.nk & 3) == 0 && (p.mask_bh & 3) == 0 && (((uintptr_t)p.mask) & 3) == 0;
    m.quads = m.on && (p.nk & 15) == 0 && (p.mask_bh & 15) == 0 && (((uintptr_t)p.mask) & 15) == 0;
    return m;
}
__device__ __forceinline__ unsigned mask_load_b32(const MaskSrc& m, int off) { return __builtin_amdgcn_raw_buffer_load_b32(m.rs, off, 0, 0); }
__device__ __forceinline__ unsigned mask_load_b8(const MaskSrc& m, int off) { return (unsigned)(__builtin_amdgcn_raw_buffer_load_b8(m.rs, off, 0, 0) & 0xff); }

// 16-bit visibility mask (bit i = register i visible) of one 32 x 32 block for a lane of a query-on-the-lane kernel:
// the lane's row is `row`, register i holds key kcol + rc(i)
__device__ __forceinline__ void mask_words_q(const MaskSrc& m, int row, int nk, int kcol, unsigned (&wd)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) wd[g] = mask_load_b32(m, row * nk + kcol + 8 * g);
}
// The same words from ONE 16-byte load per lane (round 3; Nk, pointer and (b,h) stride multiples of 16): the two lanes of a row
// (r, h = 0 / 1) fetch bytes 16 h .. 16 h + 15 of the row's 32 and trade the dwords the other one's registers stand for — lane
// (r, 0) holds keys 0-3, 8-11, 16-19, 24-27 of the block, lane (r, 1) keys 4-7, 12-15, 20-23, 28-31 — with two
// v_permlane32_swap (upper half of the first operand <-> lower half of the second).  A quarter of the load instructions, the
// same cache lines: the address unit walks 64 lanes per instruction either way.
__device__ __forceinline__ void mask_words_q16(const MaskSrc& m, int row, int nk, int kblk, int h, unsigned (&wd)[4]) {
    const u32x4 w = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(m.rs, row * nk + kblk + 16 * h, 0, 0));
    const auto s01 = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);   // [0]: lo own w0 | hi <- lo's w1;  [1]: lo <- hi's w0 | hi own w1
    const auto s23 = __builtin_amdgcn_permlane32_swap(w[2], w[3], false, false);
    wd[0] = s01[0]; wd[1] = s23[0]; wd[2] = s01[1]; wd[3] = s23[1];
}
__device__ __forceinline__ unsigned bits_of_words(const unsigned (&wd)[4]) {
    // Structured masks (a causal or windowed mask handed over as a dense one) are all-visible or all-masked over most
    // 32 x 32 blocks: two wave-uniform tests on the words save the per-byte work there (6 instructions per element)
    unsigned zero_byte = 0;   // bit 7 of every byte that is 0
#pragma unroll
    for (int g = 0; g < 4; ++g) zero_byte |= (wd[g] - 0x01010101u) & ~wd[g] & 0x80808080u;
    if (__all(zero_byte == 0)) return 0xffffu;
    if (__all((wd[0] | wd[1] | wd[2] | wd[3]) == 0)) return 0u;
    // bit 4 g + j = byte j of word g is non-zero.  Branch-free on the whole word (round 3; was a shift, mask, compare and select
    // per byte): bit 7 of every non-zero byte, then the four bits gathered with three shifts — 11 instructions per four
    // elements instead of 16.
    unsigned bits = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const unsigned nz = (((wd[g] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | wd[g]) & 0x80808080u;
        bits |= (((nz >> 7) | (nz >> 14) | (nz >> 21) | (nz >> 28)) & 0xfu) << (4 * g);
    }
    return bits;
}
// s where bit i of `vis` is set, -inf where it is not: a sign-extended one-bit field as the select mask of a bit-field insert
// (two instructions, no compare / VCC round trip)
__device__ __forceinline__ float keep_or_minus_inf(float s, unsigned vis, int i) {
    const int m = ((int)(vis << (31 - i))) >> 31;                     // v_bfe_i32: 0 or -1
    return __uint_as_float((__float_as_uint(s) & (unsigned)m) | (0xff800000u & ~(unsigned)m));   // v_bfi_b32
}
__device__ __forceinline__ unsigned dense_bits_q(const MaskSrc& m, int row, int nk, int kcol /* block's first key + 4 h */, int h) {
    if (m.quads) {
        unsigned wd[4];
        mask_words_q16(m, row, nk, kcol - 4 * h, h, wd);
        return bits_of_words(wd);
    }
    if (m.dwords) {
        unsigned wd[4];
        mask_words_q(m, row, nk, kcol, wd);
        return bits_of_words(wd);
    }
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) bits |= mask_load_b8(m, row * nk + kcol + rc_of(i)) ? (1u << i) : 0u;
    return bits;
}
// the same for a lane of the key-on-the-lane kernel: the lane's key is `key`, register i holds row rb0 + 4 h + rc(i)
__device__ __forceinline__ unsigned dense_bits_k(const MaskSrc& m, int rrow, int nk, int key) {
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) bits |= mask_load_b8(m, (rrow + rc_of(i)) * nk + key) ? (1u << i) : 0u;
    return bits;
}

// The same through LDS (round 3; Nk, pointer and (b,h) stride multiples of 16): the block's 32 x 32 mask bytes are exactly one
// 16-byte load per lane (lane l: row l >> 1, bytes 16 (l & 1) ..), written to a 1 KiB image [row][32 bytes] of the wave's own,
// from which the lane reads its key's column — 16 byte reads from LDS instead of 16 byte loads from memory.  Structured masks
// leave on the words as loaded: all bytes set / all bytes clear over the wave are decided before the round trip.  A wave's
// LDS instructions execute in order, so the reads see the wave's own writes without a barrier.
__device__ __forceinline__ unsigned dense_bits_k_lds(const MaskSrc& m, int rb0, int nk, int kw0, int lane, char* img /* this wave's 1 KiB */) {
    asm volatile("" : "+v"(lane));   // the lane-constant addresses below are made per call: hoisted, they are three registers this kernel does not have
    const u32x4 w = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(m.rs, (rb0 + (lane >> 1)) * nk + kw0 + 16 * (lane & 1), 0, 0));
    unsigned zero_byte = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) zero_byte |= (w[g] - 0x01010101u) & ~w[g] & 0x80808080u;
    if (__all(zero_byte == 0)) return 0xffffu;
    if (__all((w[0] | w[1] | w[2] | w[3]) == 0)) return 0u;
    *reinterpret_cast<u32x4*>(img + 16 * lane) = w;
    const int c = lane & 31, h = lane >> 5;
    unsigned bits = 0;
    const char* col = img + 128 * h + c;   // row 4 h + rc(i), rc(i) = (i & 3) + 8 (i >> 2): immediate offsets from one address
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= (*reinterpret_cast<const volatile uint8_t*>(col + 32 * (j + 8 * g)) ? 1u : 0u) << (4 * g + j);
        asm volatile("" : "+v"(bits));   // four reads in flight at a time: the kernel has no registers to spare
    }
    return bits;
}

// keep bits (bit i = register i kept) of one 32 x 32 block.  Query on the lane: row fixed, keys kcol + rc(i) — registers
// 4g+0, 4g+1 are one key pair, 4g+2, 4g+3 the next: 8 values per block.
__device__ __forceinline__ unsigned keep_bits_q(const ExParams& p, unsigned hi, int row, int kcol) {
    unsigned bits = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const unsigned long long z = ex_hash(hi, (unsigned)(kcol + 8 * g + 2 * pr) >> 1, p.seedmix);
            const unsigned wd = (row & 1) ? (unsigned)(z >> 32) : (unsigned)z;
            bits |= ((wd & 0xffffu) >= p.drop_thr) ? (1u << (4 * g + 2 * pr)) : 0u;
            bits |= ((wd >> 16) >= p.drop_thr) ? (1u << (4 * g + 2 * pr + 1)) : 0u;
        }
    return bits;
}
// Key on the lane: key fixed, rows rrow + rc(i) — registers 4g+0, 4g+1 are one row pair
// Score modifiers (FEAT bit 4): mod_softcap / mod_alibi (fa_ex_common.h, shared with the decode kernels of fa_decode.hip)
// the modifiers of a kFeatScore instantiation's ExParamsS (a call dependent on FEAT: the bodies the plain entries include name it
// only in discarded `if constexpr (SC)` branches)
template <int FEAT, typename P> __device__ __forceinline__ const ExScore& sc_of(const P& p) { return p.sc; }
// the same for the sinks of a kFeatSink instantiation's ExParamsK
template <int FEAT, typename P> __device__ __forceinline__ const ExSink& sink_of(const P& p) { return p.snk; }
// the same for the pages of a kFeatPaged instantiation's ExParamsPg
template <int FEAT, typename P> __device__ __forceinline__ const ExPage& pg_of(const P& p) { return p.pg; }
// this unit's al (0 without ALiBi), the same product in every kernel
__device__ __forceinline__ float alibi_k(const ExScore& sc, int bh) { return ex_slope(sc, bh) * sc.al_k; }

// ---- Additive bias (FEAT bit 8, always on the kFeatScore body): s = scale q.k + bias[b, h, i, j], in the raw-score domain of these
// kernels fma(bias, 1 / scale, q.k), the bias widened exactly.  The bias group of a kFeatBias instantiation's ExParamsB:
template <int FEAT, typename P> __device__ __forceinline__ const ExBias& bias_of(const P& p) { return p.bs; }
// This unit's bias as a range-checked buffer (rows i * b_rs, b_rs = 0: one row for every query), sized to the unit's span with the
// last row's keys rounded up to 8: the C layer asks for that much storage, and a load is then wholly inside or wholly outside the
// range.  Reads past it (rows >= nq) return 0.  A key >= nk of an earlier row reads padding, whatever it holds: the kernels make such
// a key invisible with a select after the sum, so it reaches no result.  ds: the unit's dS rows (null: none asked for).
struct BiasSrc {
    buf_rsrc_t rs;
    uint16_t* ds;
    int b_rs, s_rs;
    float binv;
};
__device__ __forceinline__ BiasSrc make_bias_src(const ExBias& bs, int bh, int nq, int nk) {
    BiasSrc s;
    const int b = bh / bs.heads, hh = bh - b * bs.heads;
    s.rs = make_rsrc(bs.bias + b * bs.b_bs + hh * bs.b_hs, ((unsigned)(nq - 1) * (unsigned)bs.b_rs + (unsigned)((nk + 7) & ~7)) * 2u);
    s.ds = bs.ds ? bs.ds + b * bs.s_bs + hh * bs.s_hs : nullptr;
    s.b_rs = bs.b_rs; s.s_rs = bs.s_rs;
    s.binv = bs.inv_scale;
    return s;
}
// Query on the lane: the lane's row is `row`, registers 4 g .. 4 g + 3 hold keys kcol + 8 g .. + 3 — four 8-byte loads per block
__device__ __forceinline__ void bias_load_q(const BiasSrc& s, int row, int kcol, u32x2 (&bw)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) bw[g] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(s.rs, (row * s.b_rs + kcol + 8 * g) * 2, 0, 0));
}
template <typename Tag>
__device__ __forceinline__ void bias_add_q(f32x16& sacc, const u32x2 (&bw)[4], float binv) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        sacc[4 * g + 0] = fmaf(unpack_lo<Tag>(bw[g][0]), binv, sacc[4 * g + 0]);
        sacc[4 * g + 1] = fmaf(unpack_hi<Tag>(bw[g][0]), binv, sacc[4 * g + 1]);
        sacc[4 * g + 2] = fmaf(unpack_lo<Tag>(bw[g][1]), binv, sacc[4 * g + 2]);
        sacc[4 * g + 3] = fmaf(unpack_hi<Tag>(bw[g][1]), binv, sacc[4 * g + 3]);
    }
}
// Key on the lane: a lane needs 16 rows of one key column.  The block's 32 x 32 values are 2 KiB, two 16-byte loads per lane (lane
// l: row l >> 1, bytes 32 (l & 1) ..), written to a 2 KiB image [row][64 bytes] of the wave's own, from which the lane reads its
// key's column (dense_bits_k_lds does the same with the mask's bytes; a wave's LDS instructions execute in order, so the reads see
// the wave's own writes without a barrier, and the next block's writes come after this block's reads).
__device__ __forceinline__ void bias_load_k(const BiasSrc& s, int rb0, int kw0, int lane, u32x4& w0, u32x4& w1) {
    asm volatile("" : "+v"(lane));   // (the lane-constant part of the address is made per call, as in dense_bits_k_lds)
    const int off = ((rb0 + (lane >> 1)) * s.b_rs + kw0 + 16 * (lane & 1)) * 2;
    w0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(s.rs, off, 0, 0));
    w1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(s.rs, off + 16, 0, 0));
}
template <typename Tag>
__device__ __forceinline__ void bias_add_k(f32x16& sacc, const u32x4& w0, const u32x4& w1, int lane, char* img /* this wave's 2 KiB */, float binv) {
    asm volatile("" : "+v"(lane));
    *reinterpret_cast<volatile u32x4*>(img + 32 * lane) = w0;
    *reinterpret_cast<volatile u32x4*>(img + 32 * lane + 16) = w1;
    const char* col = img + 256 * (lane >> 5) + 2 * (lane & 31);   // row 4 h + rc(i): immediate offsets from one address
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const volatile uint16_t*>(col + 64 * (j + 8 * g));
#pragma unroll
        for (int j = 0; j < 4; ++j) sacc[4 * g + j] = fmaf(unpack_lo<Tag>(v[j]), binv, sacc[4 * g + j]);   // four reads in flight at a time
    }
}
// dS out (the dQ kernel): the 16-bit words a lane packs for its MFMA are 4 consecutive keys of its row per register group, 8
// bytes; the row's last group stores its keys below nk one by one, so nothing past column nk is written
__device__ __forceinline__ void bias_ds_store(uint16_t* row, int col, int nk, unsigned lo, unsigned hi) {
    if (col + 4 <= nk) {
        u32x2 v;
        v[0] = lo; v[1] = hi;
        *reinterpret_cast<u32x2*>(row + col) = v;
    } else {
        if (col + 0 < nk) row[col + 0] = (uint16_t)(lo & 0xffffu);
        if (col + 1 < nk) row[col + 1] = (uint16_t)(lo >> 16);
        if (col + 2 < nk) row[col + 2] = (uint16_t)(hi & 0xffffu);
        if (col + 3 < nk) row[col + 3] = (uint16_t)(hi >> 16);
    }
}

__device__ __forceinline__ unsigned keep_bits_k(const ExParams& p, unsigned hi_bh, int rrow, int key) {
    unsigned bits = 0;
    const int sh = 16 * (key & 1);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const unsigned long long z = ex_hash(hi_bh + ((unsigned)(rrow + 8 * g + 2 * pr) >> 1), (unsigned)key >> 1, p.seedmix);
            bits |= ((((unsigned)z >> sh) & 0xffffu) >= p.drop_thr) ? (1u << (4 * g + 2 * pr)) : 0u;
            bits |= ((((unsigned)(z >> 32) >> sh) & 0xffffu) >= p.drop_thr) ? (1u << (4 * g + 2 * pr + 1)) : 0u;
        }
    return bits;
}

// Varlen (FEAT bit 3): the workgroup's unit bh = b * hq + h and its tile come from the padded grid (nq, nk = the maxima).  This is
// sequence b of the unit: where it starts in q and k, its lengths (seq_span) and its heads.  The caller narrows nq, nk, coff to it
// and leaves before its first barrier when its tile starts past the sequence; bases, buffer ranges and row strides become the
// sequence's, DR stays the column bound.  (It only reads p, and the caller writes: a function that narrows p through a reference
// changes the scalar prologue of the packed backward kernels.)
// (kFeatPaged: the keys are no span of a packed tensor — sk0 stays 0, the length is paged_len, ub names the table row)
struct ExmUnit {
    int sq0 = 0, sk0 = 0, hh = 0, hk = 0, ub = 0;   // first token of q / k, query head, K/V head, table row
    int lq = 0, lk = 0;                             // rows and keys of the sequence
};
template <int FEAT, typename P>
__device__ __forceinline__ ExmUnit exm_varlen_unit(const P& p, int bh, int nq, int nk) {
    ExmUnit u;
    const int b = bh / p.hq;
    u.hh = bh - b * p.hq;
    u.hk = kv_unit(u.hh, p.kvg);
    seq_span(p.cu_q, b, p.total_q, nq, u.sq0, u.lq);
    if constexpr ((FEAT & kFeatPaged) != 0) { u.ub = b; u.lk = paged_len(p.cu_k, b, nk); }
    else seq_span(p.cu_k, b, p.total_k, nk, u.sk0, u.lk);
    return u;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ forward
// kFeatKv8: k and v address the e4m3 bytes of the pools.  A tile's bytes come by LDS-DMA into a staging area behind the two tile
// buffers (dma_stage_kv_paged8: a block of 16 keys per wave, dword granularity) and at the tile boundary every wave widens its own
// block into the 16-bit TileSwz image (`land`; kv8_widen_block, exact), so the key loop reads what it reads from a 16-bit pool.
// k_descale joins the constants that carry softmax_scale, v_descale the epilogue's normaliser.
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_fwd_kernel(const uint16_t* __restrict__ q, const ExKV<FEAT>* __restrict__ k,
                                                         const ExKV<FEAT>* __restrict__ v, uint16_t* __restrict__ o,
                                                         float* __restrict__ lse, ExB<FEAT> p, float c_log2) {
    static_assert((FEAT & kFeatSink) == 0 || (FEAT & kFeatScore) != 0, "a sink forward is a score-modifier instantiation");
    static_assert((FEAT & kFeatPaged) == 0 || (FEAT & (kFeatVarlen | kFeatMask | kFeatDrop)) == kFeatVarlen, "paged K/V: varlen, no mask, no dropout");
    static_assert((FEAT & kFeatKv8) == 0 || (FEAT & kFeatPaged) != 0, "an e4m3 pool is paged");
    constexpr int NW = 8, BM = 32 * NW, KB = 4, BN = 32 * KB, NKS = D / 16, NDV = D / 32, TILE_BYTES = BN * D * 2;
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0, SC = (FEAT & kFeatScore) != 0, SNK = (FEAT & kFeatSink) != 0;
    constexpr bool PG = (FEAT & kFeatPaged) != 0;   // k, v are pools read through a block table: only `stage` differs
    constexpr bool KV8 = (FEAT & kFeatKv8) != 0;    // ... of e4m3 bytes: `stage` and `land` differ
    constexpr bool BIAS = (FEAT & kFeatBias) != 0;  // an additive bias joins the scores where ALiBi does
    static_assert(!BIAS || (FEAT & ~kFeatBias) == kFeatScore, "a bias instantiation is the score-modifier body and nothing else");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K tile | V tile]; kFeatKv8: then [K | V] e4m3 bytes of one tile
    const int DR = p.d;
    int nq = p.nq, nk = p.nk;
    const int nqt = (nq + BM - 1) / BM;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;
    const int q0 = (L - bh * nqt) * BM;
    ExmUnit u;
    if constexpr (VAR) {
        u = exm_varlen_unit<FEAT>(p, bh, nq, nk);
        nq = u.lq; nk = u.lk; p.coff = u.lk - u.lq;
        if (q0 >= nq) return;
    }
    // kFeatKv8: the scales of (sequence, K/V head), one scalar load each.  k_descale multiplies the score, so it joins every constant
    // that carries softmax_scale or its reciprocal: fp32 multiplications or divisions, exact for a power of two, the identity for 1.0
    [[maybe_unused]] float vdsc = 1.f;
    if constexpr (KV8) {
        const float kdsc = kv8_scale(p.q8.kd, p.q8.bs, u.ub, u.hk);
        vdsc = kv8_scale(p.q8.vd, p.q8.bs, u.ub, u.hk);
        p.scale *= kdsc;
        c_log2 *= kdsc;
        if constexpr (SC) {
            p.sc.cap_k *= kdsc;
            p.sc.cap_a /= kdsc;
            p.sc.al_k /= kdsc;
        }
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const size_t qbase = VAR ? (size_t)u.sq0 * p.sq + u.hh * DR : (size_t)bh * nq * DR;
    const size_t kbase = VAR ? (size_t)u.sk0 * p.sk + u.hk * DR : (size_t)kv_unit(bh, p.kvg) * nk * DR;
    const size_t vbase = VAR ? (size_t)u.sk0 * p.sv + u.hk * DR : kbase;
    const size_t obase = VAR ? ((size_t)u.sq0 * p.hq + u.hh) * DR : qbase;
    const size_t lbase = VAR ? (size_t)u.hh * p.total_q + u.sq0 : (size_t)bh * nq;
    const int qrow = q0 + 32 * w + r;

    const buf_rsrc_t q_rs = make_rsrc(q + qbase, VAR ? span_bytes(nq, DR, p.sq) : (unsigned)nq * DR * 2);
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = buf_load_frag(q_rs, frag_off<VAR>(qrow, 16 * ks + 8 * h, DR, true, VAR ? p.sq : DR));

    const rsrc_s_t k_rs = make_rsrc_s(k + kbase, VAR ? span_bytes(nk, DR, p.sk) : (unsigned)nk * DR * 2);
    const rsrc_s_t v_rs = make_rsrc_s(v + vbase, VAR ? span_bytes(nk, DR, p.sv) : (unsigned)nk * DR * 2);
    const int dma_voff = KV8 ? dma_lane_voff8<D>(lane, DR, p.sk) : dma_lane_voff<D, VAR>(lane, w, DR, VAR ? p.sk : DR);
    const int dma_voff_v = KV8 ? dma_lane_voff8<D>(lane, DR, p.sv) : (VAR ? dma_lane_voff<D, VAR>(lane, w, DR, p.sv) : dma_voff);
    [[maybe_unused]] const int* pg_row = nullptr;   // kFeatPaged: this sequence's table row and its last slot in use
    [[maybe_unused]] int pg_last = 0;
    if constexpr (PG) {
        pg_row = pg_of<FEAT>(p).table + (size_t)u.ub * pg_of<FEAT>(p).max_blocks;
        pg_last = pg_slot(pg_of<FEAT>(p), max(nk, 1) - 1);
    }
    // (kFeatKv8: every tile goes through the one staging area, whichever buffer it is for: `land` empties it before the next is staged)
    constexpr int KSTAGE = 4 * TILE_BYTES, VSTAGE = KSTAGE + BN * D;
    auto stage = [&](int buf, int k0) {
        char* kb_ = smem + buf * 2 * TILE_BYTES;
        if constexpr (KV8) {
            dma_stage_kv_paged8<D, BN, NW>(pg_of<FEAT>(p), pg_row, pg_last, reinterpret_cast<const char*>(k + kbase), reinterpret_cast<const char*>(v + vbase),
                                           smem + KSTAGE, smem + VSTAGE, k0, nk, dma_voff, dma_voff_v, w, DR, p.sk, p.sv);
        } else if constexpr (PG) {
            dma_stage_kv_paged<D, BN, NW>(pg_of<FEAT>(p), pg_row, pg_last, k + kbase, v + vbase, kb_, kb_ + TILE_BYTES, k0, nk, dma_voff,
                                          dma_voff_v, w, DR, p.sk, p.sv);
        } else {
            dma_stage_tile<D, BN, NW, VAR>(k_rs, kb_, k0, dma_voff, w, DR, 0, VAR ? p.sk : DR);
            dma_stage_tile<D, BN, NW, VAR>(v_rs, kb_ + TILE_BYTES, k0, dma_voff_v, w, DR, 0, VAR ? p.sv : DR);
        }
    };
    // kFeatKv8: the staged tile arrives in buffer `buf` for every wave.  `fresh` (uniform over the workgroup): a tile was staged
    // since the last call.  Its bytes are in the staging area, and LDS-DMA data is ordered for a ds_read only by the issuing wave's
    // vmcnt and a barrier the reader has passed, its own wave included — so one more barrier, then every wave widens its block.
    // (The 16-bit pools keep their literal dma_wait_all(); __syncthreads(); pairs: see the file header.)
    [[maybe_unused]] auto land = [&](int buf, bool fresh) {
        dma_wait_all();
        if (fresh) {
            __syncthreads();
            kv8_widen_block<Tag, D>(smem + KSTAGE, smem + buf * 2 * TILE_BYTES, w, lane);
            kv8_widen_block<Tag, D>(smem + VSTAGE, smem + buf * 2 * TILE_BYTES + TILE_BYTES, w, lane);
        }
        __syncthreads();
    };
    const MaskSrc msk = make_mask_src(p, bh);
    const bool use_bm = (FEAT & kFeatMask) && p.bmask != nullptr;
    const bool drop = (FEAT & kFeatDrop) && p.p_drop > 0.f;
    const unsigned hi = (unsigned)bh * p.nqh + ((unsigned)qrow >> 1);
    const int rbw = min(q0 + 32 * w, nq - 1) / p.br;   // block row of this wave's 32 rows (br is a multiple of 32)
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = alibi_k(sc_of<FEAT>(p), bh);
    [[maybe_unused]] float snk = -INFINITY;   // this unit's sink logit (kFeatSink): workgroup-uniform, one scalar load
    if constexpr (SNK) snk = ex_sink(sink_of<FEAT>(p), bh);
    [[maybe_unused]] BiasSrc bsrc;
    if constexpr (BIAS) bsrc = make_bias_src(bias_of<FEAT>(p), bh, nq, nk);

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // keys past the last row's diagonal are masked for every row of the tile (of the wave)
    constexpr bool WIN = (FEAT & kFeatWindow) != 0;
    // window: the band's right edge takes the diagonal's place (wr = 0 under the causal mask), and keys left of the first
    // row's left edge are masked for every row as well: tiles [t_lo, ntiles) for the workgroup, [t_lo_w, ntiles_w) per wave,
    // both bounded by the last row < nq (a wave without one computes nothing)
    const int kend = WIN ? max(0, min(nk, min(q0 + BM, nq) + p.coff + p.wr)) : (p.causal ? max(0, min(nk, q0 + BM + p.coff)) : nk);
    const int kend_w = WIN ? (q0 + 32 * w < nq ? max(0, min(nk, min(q0 + 32 * w + 32, nq) + p.coff + p.wr)) : 0)
                           : (p.causal ? max(0, min(nk, q0 + 32 * w + 32 + p.coff)) : nk);
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const int t_lo = WIN ? max(0, q0 + p.coff - p.wl) / BN : 0;
    const int t_lo_w = WIN ? max(0, q0 + 32 * w + p.coff - p.wl) / BN : 0;
    LiveScan<true, BN> scan;   // (tiles keep their absolute index: the scan's first probe is at t_lo)
    if (use_bm) scan.init(p, q0, min(q0 + BM, nq), 0, nk, ntiles, lane);
    auto next_live = [&](int t) { return use_bm ? scan.next(t) : t; };
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int t = next_live(t_lo), cur = 0;
    if (t < ntiles) stage(0, t * BN);
    if constexpr (KV8) land(0, t < ntiles);
    else { dma_wait_all(); __syncthreads(); }
    if constexpr (WIN) {
        // leading feed-only tiles: left of this wave's band, inside the workgroup's
        while (t < min(t_lo_w, ntiles)) {
            const int tn = next_live(t + 1);
            if (tn < ntiles) stage(cur ^ 1, tn * BN);
            if constexpr (KV8) land(cur ^ 1, tn < ntiles);
            else { dma_wait_all(); __syncthreads(); }
            cur ^= 1;
            t = tn;
        }
    }
    // two loops instead of an `if` inside one (a conditional accumulate makes hipcc carry the accumulators through
    // copies): tiles this wave computes, then the ones it only helps to load
    // Dense mask: its loads are ordinary VMEM loads, and VMEM returns in order — were the next tile's LDS-DMA issued
    // first, the wait for the mask words would also be a wait for that whole tile.  So the DMA goes out when the mask has
    // been read (it still has the tile's products to land).  Fetching the words a tile ahead instead (16 more live
    // registers) was measured slower: 1.15 vs 1.08 ms forward at BH 64, N 4096, half the pairs masked.
    // (the bias words are VMEM loads as well: a kFeatBias instantiation always stages late)
    const bool late_stage = BIAS || ((FEAT & kFeatMask) && msk.on);
    while (t < ntiles_w) {
        const int tn = next_live(t + 1);
        if (!late_stage && tn < ntiles) stage(cur ^ 1, tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * 2 * TILE_BYTES;
        const char* Vt = Kt + TILE_BYTES;
        {
            // visibility / keep bits of this lane's 4 x 16 elements, requested ahead of the S MFMAs
            unsigned vis[KB], kp[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                vis[kb] = 0xffffu;
                kp[kb] = 0xffffu;
                if constexpr (FEAT & kFeatMask) {
                    if (msk.on) vis[kb] = dense_bits_q(msk, qrow, nk, k0 + 32 * kb + 4 * h, h);
                    if (use_bm && p.bmask[rbw * p.nbc + min(k0 + 32 * kb, nk - 1) / p.bc] == 0) vis[kb] = 0;
                }
                if constexpr (FEAT & kFeatDrop) {
                    if (drop) kp[kb] = keep_bits_q(p, hi, qrow, k0 + 32 * kb + 4 * h);
                }
            }
            // a tile of which this wave sees nothing (the upper triangle of a causal mask handed over as a dense one, the
            // dead blocks of a block-sparse tile) is not computed: wave-uniform
            bool any_vis = true;
            if constexpr (FEAT & kFeatMask) {
                unsigned all = 0;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) all |= vis[kb];
                any_vis = __any(all != 0) != 0;
                if (late_stage && tn < ntiles) stage(cur ^ 1, tn * BN);   // the mask words have arrived
            }
            [[maybe_unused]] u32x2 bw[KB][4];   // kFeatBias: this lane's 4 x 16 bias values, requested ahead of the S MFMAs
            if constexpr (BIAS) {
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) bias_load_q(bsrc, qrow, k0 + 32 * kb + 4 * h, bw[kb]);
                if (tn < ntiles) stage(cur ^ 1, tn * BN);   // behind the bias loads: VMEM returns in order
            }
            if (any_vis) {
            f32x16 sacc[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const s16x8 a = *reinterpret_cast<const s16x8*>(Kt + TileSwz<D>::off(32 * kb + r, 2 * ks + h));
                    sacc[kb] = mfma32<Tag>(a, qf[ks], sacc[kb]);
                }
            }
            if constexpr (SC) {   // ---- score modifiers (wave-uniform switches), before every mask
                if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int i = 0; i < 16; ++i) { float dt; sacc[kb][i] = mod_softcap(sacc[kb][i], sc_of<FEAT>(p), dt); }
                }
                if (sc_of<FEAT>(p).alibi) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) {
                        const float fb = (float)(qrow + p.coff - (k0 + 32 * kb + 4 * h));   // dist of register i: fb - rc(i)
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[kb][i] = mod_alibi(sacc[kb][i], al, fb - (float)rc_of(i));
                    }
                }
                if constexpr (BIAS) {   // a key >= nk may have added padding, NaN included: the select below takes it out
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) bias_add_q<Tag>(sacc[kb], bw[kb], bsrc.binv);
                }
            }
            // ---- causal diagonal / ragged last tile: key index of register i is k0 + 32 kb + 4 h + rc(i)
            const bool need_mask = WIN ? ((k0 + BN - 1 > q0 + 32 * w + p.coff + p.wr) || (k0 + BN > nk) ||
                                          (k0 < q0 + 32 * w + 31 + p.coff - p.wl))   // + the band's left edge
                                       : ((p.causal && (k0 + BN - 1 > q0 + 32 * w + p.coff)) || (k0 + BN > nk));
            if (need_mask) {
                // last visible key of this lane's row
                const int lim = WIN ? min(qrow + p.coff + p.wr, nk - 1) : (p.causal ? min(qrow + p.coff, nk - 1) : nk - 1);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const int thr = lim - (k0 + 32 * kb + 4 * h);
                    if constexpr (WIN) {
                        const int thl = qrow + p.coff - p.wl - (k0 + 32 * kb + 4 * h);   // the row's first visible key
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            if (rc_of(i) > thr || rc_of(i) < thl) sacc[kb][i] = -INFINITY;
                    } else {
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            if (rc_of(i) > thr) sacc[kb][i] = -INFINITY;
                    }
                }
            }
            if constexpr (FEAT & kFeatMask) {
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
                    if (__any(vis[kb] != 0xffffu)) {   // wave-uniform
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[kb][i] = keep_or_minus_inf(sacc[kb][i], vis[kb], i);
                    }
            }
            // ---- online softmax (fa_fwd_mfma.hip), with rows that have not met a visible key yet (m = -inf)
            float mx = sacc[0][0];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
            mx = fmaxf(mx, wave_half_swap(mx));
            const float m_new = fmaxf(m_run, mx);
            float mc;
            // lazy rescale: keep the stale max while no row has grown past it by more than 2^8; -inf - -inf = NaN counts
            // as "rescale", so a wave with a dead row takes the exact path
            const bool rescale = __any(!((m_new - m_run) * c_log2 <= 8.0f)) != 0;
            if (rescale) {
                const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
                const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * c_log2);
                mc = m_use * c_log2;
                m_run = m_new;
#pragma unroll
                for (int t2 = 0; t2 < NDV; ++t2)
#pragma unroll
                    for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
                l_run *= alpha;
            } else {
                mc = m_run * c_log2;
            }
            float rs = 0.f;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float pe = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], c_log2, -mc));
                    rs += pe;   // the denominator counts every visible key, dropped or not
                    if constexpr (FEAT & kFeatDrop) pe = ((kp[kb] >> i) & 1u) ? pe * p.keep_scale : 0.f;
                    sacc[kb][i] = pe;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4 pk;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pk[j] = pack2<Tag>(sacc[kb][8 * s + 2 * j], sacc[kb][8 * s + 2 * j + 1]);
                    const s16x8 pb = *reinterpret_cast<s16x8*>(&pk);
                    const int key_a = 32 * kb + 16 * s + 4 * h + tq;
#pragma unroll
                    for (int dvb = 0; dvb < NDV; ++dvb) {
                        const int ch = 4 * dvb + 2 * g16 + (tp >> 1);
                        const s16x4 lo = lds_tr16(Vt + TileSwz<D>::off(key_a, ch) + 8 * (tp & 1));
                        const s16x4 hi4 = lds_tr16(Vt + TileSwz<D>::off(key_a + 8, ch) + 8 * (tp & 1));
                        oacc[dvb] = mfma32<Tag>(cat8(lo, hi4), pb, oacc[dvb]);
                    }
                }
            }
            l_run += rs;
            }   // any_vis
        }
        if constexpr (KV8) land(cur ^ 1, tn < ntiles);
        else { dma_wait_all(); __syncthreads(); }
        cur ^= 1;
        t = tn;
    }
    while (t < ntiles) {
        const int tn = next_live(t + 1);
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        if constexpr (KV8) land(cur ^ 1, tn < ntiles);
        else { dma_wait_all(); __syncthreads(); }
        cur ^= 1;
        t = tn;
    }

    // ---- epilogue: normalise, store O and lse.  Every wave is past the last barrier and nothing is in flight: each wave
    // stages its rows in 32 x D x 2 bytes of buffer 0
    const float l_tot = l_run + wave_half_swap(l_run);
    float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    [[maybe_unused]] float lse_k = 0.f;
    if constexpr (SNK) {   // the sink column (a head at -inf keeps the formulas of the call without sinks: the same bits)
        lse_k = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
        if (snk != -INFINITY) ex_sink_norm(l_tot > 0.f ? m_run * p.scale : -INFINITY, l_tot, snk, inv, lse_k);
    }
    // v_descale, once, in fp32, in front of the single rounding: with 1.0 the products below are the 16-bit kernel's
    if constexpr (KV8) inv *= vdsc;
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vals[4 * dvb + g][0] = pack2_rn<Tag>(oacc[dvb][4 * g + 0] * inv, oacc[dvb][4 * g + 1] * inv);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(oacc[dvb][4 * g + 2] * inv, oacc[dvb][4 * g + 3] * inv);
        }
    store_rows_via_lds<D, VAR>(smem + w * 32 * D * 2, vals, o + obase, q0 + 32 * w, nq, lane, DR, -1, p.hq * DR);
    if constexpr (SNK) {
        if (qrow < nq && h == 0) lse[lbase + qrow] = lse_k;
    } else {
        if (qrow < nq && h == 0) lse[lbase + qrow] = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ dK / dV
// M16: the dense mask (if any) is 16-byte aligned in every respect — its bytes come through the wave's LDS image
// (dense_bits_k_lds); a separate instantiation, not a run-time choice: with both loaders in one kernel the masked form spills
template <typename Tag, int D, int FEAT, bool M16 = false>
__global__ __launch_bounds__(512, 2) void exm_dkdv_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                          const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                          const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                          uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, ExB<FEAT> p,
                                                          float c_log2) {
    static_assert((FEAT & (kFeatSink | kFeatPaged | kFeatKv8)) == 0, "forward-only bits");
    constexpr int NW = 8, BK = 32 * NW, BQ = 64, NKS = D / 16, NDB = D / 32;
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0, SC = (FEAT & kFeatScore) != 0;
    constexpr bool BIAS = (FEAT & kFeatBias) != 0;   // + 8 x 2 KiB behind the row constants: the waves' bias images
    static_assert(!BIAS || ((FEAT & ~kFeatBias) == kFeatScore && !M16), "a bias instantiation is the score-modifier body and nothing else");
    constexpr int K_BYTES = BK * D * 2, Q_BYTES = BQ * D * 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                      // [256][D]
    char* Qs = Ks + K_BYTES;              // [2][64][D]
    char* Os = Qs + 2 * Q_BYTES;          // [2][64][D]   (dO)
    float* Ls = reinterpret_cast<float*>(Os + 2 * Q_BYTES);  // [2][ 64 x -lse/scale | 64 x -delta ]
    const int DR = p.d;
    int nq = p.nq, nk = p.nk;
    const int nkt = (nk + BK - 1) / BK;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nkt;
    const int key0 = (L - bh * nkt) * BK;
    ExmUnit u;
    if constexpr (VAR) {
        u = exm_varlen_unit<FEAT>(p, bh, nq, nk);
        nq = u.lq; nk = u.lk; p.coff = u.lk - u.lq;
        if (key0 >= nk) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const size_t qbase = VAR ? (size_t)u.sq0 * p.sq + u.hh * DR : (size_t)bh * nq * DR;
    const size_t kbase = VAR ? (size_t)u.sk0 * p.sk + u.hk * DR : (size_t)kv_unit(bh, p.kvg) * nk * DR;
    const size_t vbase = VAR ? (size_t)u.sk0 * p.sv + u.hk * DR : kbase;
    const size_t obase = VAR ? ((size_t)u.sq0 * p.hq + u.hh) * DR : qbase;
    const size_t rbase = VAR ? (size_t)u.hh * p.total_q + u.sq0 : (size_t)bh * nq;
    const int kw0 = key0 + 32 * w, key = kw0 + r;

    const rsrc_s_t k_rs = make_rsrc_s(k + kbase, VAR ? span_bytes(nk, DR, p.sk) : (unsigned)nk * DR * 2);
    const rsrc_s_t q_rs = make_rsrc_s(q + qbase, VAR ? span_bytes(nq, DR, p.sq) : (unsigned)nq * DR * 2);
    const rsrc_s_t o_rs = make_rsrc_s(dout + obase, VAR ? span_bytes(nq, DR, p.hq * DR) : (unsigned)nq * DR * 2);
    const rsrc_s_t l_rs = make_rsrc_s(nlse + rbase, (unsigned)nq * 4);
    const rsrc_s_t d_rs = make_rsrc_s(ndelta + rbase, (unsigned)nq * 4);
    const buf_rsrc_t v_rs = make_rsrc(v + vbase, VAR ? span_bytes(nk, DR, p.sv) : (unsigned)nk * DR * 2);
    const int dma_voff = dma_lane_voff<D, VAR>(lane, w, DR, VAR ? p.sq : DR);
    const int dma_voff_o = VAR ? dma_lane_voff<D, VAR>(lane, w, DR, p.hq * DR) : dma_voff;
    auto stage = [&](int buf, int qs) {
        dma_stage_tile<D, BQ, NW, VAR>(q_rs, Qs + buf * Q_BYTES, qs, dma_voff, w, DR, 0, VAR ? p.sq : DR);
        dma_stage_tile<D, BQ, NW, VAR>(o_rs, Os + buf * Q_BYTES, qs, dma_voff_o, w, DR, 0, VAR ? p.hq * DR : DR);
        // row constants: 64 floats each, one 4-byte LDS-DMA per lane (rows >= nq read as 0: harmless, their dO is 0)
        if (w == 0) dma4_issue(l_rs, lds_addr_of(Ls + buf * 128), lane * 4, __builtin_amdgcn_readfirstlane(qs * 4));
        if (w == 1) dma4_issue(d_rs, lds_addr_of(Ls + buf * 128 + 64), lane * 4, __builtin_amdgcn_readfirstlane(qs * 4));
    };
    const MaskSrc msk = make_mask_src(p, bh);
    const bool use_bm = (FEAT & kFeatMask) && p.bmask != nullptr;
    const bool drop = (FEAT & kFeatDrop) && p.p_drop > 0.f;
    const int cbw = min(kw0, nk - 1) / p.bc;   // block column of this wave's 32 keys (bc is a multiple of 32)
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = alibi_k(sc_of<FEAT>(p), bh);
    [[maybe_unused]] BiasSrc bsrc;
    if constexpr (BIAS) bsrc = make_bias_src(bias_of<FEAT>(p), bh, nq, nk);

    if constexpr (VAR) dma_stage_tile<D, BK, NW, VAR>(k_rs, Ks, key0, dma_lane_voff<D, VAR>(lane, w, DR, p.sk), w, DR, 0, p.sk);
    else dma_stage_tile<D, BK, NW>(k_rs, Ks, key0, dma_voff, w, DR);
    s16x8 vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) vf[ks] = buf_load_frag(v_rs, frag_off<VAR>(key, 16 * ks + 8 * h, DR, true, VAR ? p.sv : DR));

    f32x16 dka[NDB], dva[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { dka[t][i] = 0.f; dva[t][i] = 0.f; }

    // key j is visible from row j - coff on: earlier query tiles see none of this workgroup's (this wave's) keys
    constexpr bool WIN = (FEAT & kFeatWindow) != 0;
    // window: key j is visible from row j - coff - wr to row j - coff + wl; rows past the last key's band see none of
    // the workgroup's (query tiles [0, ntile)) or of this wave's keys (iterations [it_first, it_last) compute)
    const int qs_first = WIN ? (max(0, key0 - p.coff - p.wr) / BQ) * BQ : (p.causal ? (max(0, key0 - p.coff) / BQ) * BQ : 0);
    const int qend = WIN ? min(nq, min(key0 + BK, nk) - p.coff + p.wl) : nq;
    const int ntile = qs_first < qend ? (qend - qs_first + BQ - 1) / BQ : 0;
    const int it_first = WIN ? max(0, kw0 - p.coff - p.wr) / BQ - qs_first / BQ
                             : (p.causal ? max(0, kw0 - p.coff) / BQ - qs_first / BQ : 0);
    const int it_last = WIN ? (kw0 < nk ? min(ntile, (max(0, min(nq, min(kw0 + 32, nk) - p.coff + p.wl)) + BQ - 1) / BQ - qs_first / BQ) : 0)
                            : ntile;
    LiveScan<false, BQ> scan;
    if (use_bm) scan.init(p, key0, min(key0 + BK, nk), qs_first, nq, ntile, lane);   // (window: over the band's tiles)
    auto next_live = [&](int it) { return use_bm ? scan.next(it) : it; };
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int it = next_live(0), cur = 0;
    if (it < ntile) stage(0, qs_first + it * BQ);
    dma_wait_all();
    __syncthreads();
    // feed-only iterations first (tiles before this wave's first visible row), then the computing ones
    while (it < min(it_first, ntile)) {
        const int itn = next_live(it + 1);
        if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        it = itn;
    }
    while (it < it_last) {
        const int itn = next_live(it + 1);
        if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
        const int qs = qs_first + it * BQ;
        const char* Qt = Qs + cur * Q_BYTES;
        const char* Ot = Os + cur * Q_BYTES;
        const float* Lt = Ls + cur * 128;
#pragma unroll
        for (int qb = 0; qb < BQ / 32; ++qb) {
            const int rb0 = qs + 32 * qb;              // first row of the block; register i holds row rb0 + 4 h + rc(i)
            unsigned vis = 0xffffu, kp = 0xffffu;
            if constexpr (FEAT & kFeatMask) {
                if constexpr (M16) { if (msk.on) vis = dense_bits_k_lds(msk, rb0, nk, kw0, lane, reinterpret_cast<char*>(Ls + 2 * 128) + 1024 * w); }
                else if (msk.on) vis = dense_bits_k(msk, rb0 + 4 * h, nk, key);
                if (use_bm && p.bmask[(min(rb0, nq - 1) / p.br) * p.nbc + cbw] == 0) vis = 0;
            }
            if constexpr (FEAT & kFeatDrop) {
                if (drop) kp = keep_bits_k(p, (unsigned)bh * p.nqh, rb0 + 4 * h, key);
            }
            // a block of which this wave sees nothing is not computed (wave-uniform; see the forward kernel)
            if ((FEAT & kFeatMask) && !__any(vis != 0)) continue;
            // masked: the row precedes the key's first visible row (causal), or the key lies past nk: rc(i) < thr;
            // window: also the row follows the key's last visible row, rc(i) > thh
            const bool need_mask = WIN ? ((kw0 + 31 - p.coff - p.wr > rb0) || (kw0 + 32 > nk) || (rb0 + 31 > kw0 - p.coff + p.wl))
                                       : ((p.causal && (kw0 + 31 - p.coff > rb0)) || (kw0 + 32 > nk));
            const int thr = WIN ? (!need_mask ? -1 : (key >= nk ? 64 : key - p.coff - p.wr - rb0 - 4 * h))
                                : (!need_mask ? -1 : (key >= nk ? 64 : (p.causal ? key - p.coff - rb0 - 4 * h : -1)));
            [[maybe_unused]] const int thh = WIN && need_mask ? key - p.coff + p.wl - rb0 - 4 * h : 64;
            int kofs = 32 * w * 2 * D;
            asm volatile("" : "+v"(kofs));
            u32x4 pp[2], sp[2];
            [[maybe_unused]] u32x4 pu[2];   // dropout: the un-dropped 16-bit P (dS = P (dP_drop - delta)); score modifiers: P (1 - t^2)
            [[maybe_unused]] float dt[16];  // score modifiers: the softcap's derivative 1 - t^2
            [[maybe_unused]] u32x4 bq0, bq1;   // kFeatBias: this lane's 32 bytes of the block's bias, requested ahead of the S MFMAs
            if constexpr (BIAS) bias_load_k(bsrc, rb0, kw0, lane, bq0, bq1);
            {
                f32x16 sacc;
                // seeded with -lse / scale; with a score modifier S starts at 0, is modified, and then -lse / scale is added
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(Lt + 32 * qb + 8 * g + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (SC) sacc[4 * g + j] = 0.f;
                        else sacc[4 * g + j] = a[j];
                    }
                }
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const int ro = TileSwz<D>::off(r, 2 * ks + h);
                    const s16x8 qa = *reinterpret_cast<const s16x8*>(Qt + 32 * qb * 2 * D + ro);
                    const s16x8 kf = *reinterpret_cast<const s16x8*>(Ks + ro + kofs);
                    sacc = mfma32<Tag>(qa, kf, sacc);
                }
                if constexpr (SC) {
                    if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[i] = mod_softcap(sacc[i], sc_of<FEAT>(p), dt[i]);
                    }
                    if (sc_of<FEAT>(p).alibi) {
                        const float fb = (float)(rb0 + 4 * h + p.coff - key);   // dist of register i: fb + rc(i)
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[i] = mod_alibi(sacc[i], al, fb + (float)rc_of(i));
                    }
                    if constexpr (BIAS) bias_add_k<Tag>(sacc, bq0, bq1, lane, reinterpret_cast<char*>(Ls + 2 * 128) + 2048 * w, bsrc.binv);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(Lt + 32 * qb + 8 * g + 4 * h);
#pragma unroll
                        for (int j = 0; j < 4; ++j) sacc[4 * g + j] += a[j];
                    }
                }
                // wave-uniform: blocks that every lane sees whole (most of a structured mask) skip the selects
                // (score modifiers: the rows past nq of the last tile are masked as well — a zero dO no longer makes them
                // harmless, since a negative slope can make their modified score, taken against lse = 0, overflow exp2)
                const bool plain = !need_mask && (!(FEAT & kFeatMask) || !__any(vis != 0xffffu)) && (!SC || rb0 + 32 <= nq);
                if (plain) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) sacc[i] = __builtin_amdgcn_exp2f(sacc[i] * c_log2);
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        bool dead = rc_of(i) < thr;
                        if constexpr (WIN) dead = dead || rc_of(i) > thh;
                        if constexpr (SC) dead = dead || rc_of(i) >= nq - rb0 - 4 * h;
                        if constexpr (FEAT & kFeatMask) dead = dead || !((vis >> i) & 1u);
                        sacc[i] = dead ? 0.f : __builtin_amdgcn_exp2f(sacc[i] * c_log2);
                    }
                }
                if constexpr (SC) {
                    // the dS side of P: P (1 - t^2), multiplied in fp32 and packed once (dS = [P (1 - t^2)] (dP - delta), the
                    // product rounded to 16 bits where P alone is otherwise) — so dt does not live on across the dP product
                    if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                        for (int s = 0; s < 2; ++s)
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                pu[s][j] = pack2<Tag>(sacc[8 * s + 2 * j] * dt[8 * s + 2 * j], sacc[8 * s + 2 * j + 1] * dt[8 * s + 2 * j + 1]);
                    } else {
#pragma unroll
                        for (int s = 0; s < 2; ++s)
#pragma unroll
                            for (int j = 0; j < 4; ++j) pu[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
                    }
                    if constexpr (FEAT & kFeatDrop) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[i] = ((kp >> i) & 1u) ? sacc[i] * p.keep_scale : 0.f;
                    }
                } else if constexpr (FEAT & kFeatDrop) {
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int j = 0; j < 4; ++j) pu[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
#pragma unroll
                    for (int i = 0; i < 16; ++i) sacc[i] = ((kp >> i) & 1u) ? sacc[i] * p.keep_scale : 0.f;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) pp[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
            }
            {
                f32x16 pacc;
                f32x4 ndv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) ndv[g] = *reinterpret_cast<const f32x4*>(Lt + 64 + 32 * qb + 8 * g + 4 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) pacc[4 * g + j] = (FEAT & kFeatDrop) ? 0.f : ndv[g][j];
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const s16x8 oa = *reinterpret_cast<const s16x8*>(Ot + 32 * qb * 2 * D + TileSwz<D>::off(r, 2 * ks + h));
                    pacc = mfma32<Tag>(oa, vf[ks], pacc);
                }
                if constexpr (FEAT & kFeatDrop) {   // dP' = keep / (1 - p) * (dO V^T) - delta
#pragma unroll
                    for (int i = 0; i < 16; ++i) pacc[i] = (((kp >> i) & 1u) ? pacc[i] * p.keep_scale : 0.f) + ndv[i >> 2][i & 3];
                }
                if constexpr (std::is_same<Tag, f16_tag>::value) mfma_result_fence(pacc);   // mul_pack<f16> reads pacc from asm
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        sp[s][j] = mul_pack<Tag>(((FEAT & kFeatDrop) || SC) ? pu[s][j] : pp[s][j], pacc[8 * s + 2 * j], pacc[8 * s + 2 * j + 1]);
                if constexpr (std::is_same<Tag, f16_tag>::value) asm volatile("s_nop 1" : "+v"(sp[0]), "+v"(sp[1]));
            }
            if (D > 64) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const s16x8 pb = *reinterpret_cast<s16x8*>(&pp[s]);
                const s16x8 sb = *reinterpret_cast<s16x8*>(&sp[s]);
                const int qa_ = 32 * qb + 16 * s + 4 * h + tq;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const int ch = 4 * db + 2 * g16 + (tp >> 1);
                    const int o1 = TileSwz<D>::off(qa_, ch) + 8 * (tp & 1);
                    const int o2 = TileSwz<D>::off(qa_ + 8, ch) + 8 * (tp & 1);
                    const s16x8 doT = cat8(lds_tr16(Ot + o1), lds_tr16(Ot + o2));
                    dva[db] = mfma32<Tag>(doT, pb, dva[db]);
                    const s16x8 qT = cat8(lds_tr16(Qt + o1), lds_tr16(Qt + o2));
                    dka[db] = mfma32<Tag>(qT, sb, dka[db]);
                }
                if (D > 64) __builtin_amdgcn_sched_barrier(0);
            }
        }
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        it = itn;
    }
    if constexpr (WIN) {
        // trailing feed-only iterations: rows past this wave's keys' band, inside the workgroup's
        while (it < ntile) {
            const int itn = next_live(it + 1);
            if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
            dma_wait_all();
            __syncthreads();
            cur ^= 1;
            it = itn;
        }
    }

    if (key < nk) {
        // dK / dV rows: per query head (grouped: the partials kv_group_sum adds up)
        // (varlen: rows of (total_k, hq, d) — the partials, or dk / dv themselves when hq = hkv)
        const size_t krow = VAR ? ((size_t)(u.sk0 + key) * p.hq + u.hh) * DR : ((size_t)bh * nk + key) * DR;
        uint16_t* dkrow = dk + krow;
        uint16_t* dvrow = dv + krow;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 a, b;
                a[0] = pack2_rn<Tag>(dka[db][4 * g + 0] * p.scale, dka[db][4 * g + 1] * p.scale);
                a[1] = pack2_rn<Tag>(dka[db][4 * g + 2] * p.scale, dka[db][4 * g + 3] * p.scale);
                b[0] = pack2_rn<Tag>(dva[db][4 * g + 0], dva[db][4 * g + 1]);
                b[1] = pack2_rn<Tag>(dva[db][4 * g + 2], dva[db][4 * g + 3]);
                if (32 * db + 8 * g + 4 * h >= DR) continue;   // padded columns (DR is a multiple of 8)
                *reinterpret_cast<u32x2*>(dkrow + 32 * db + 8 * g + 4 * h) = a;
                *reinterpret_cast<u32x2*>(dvrow + 32 * db + 8 * g + 4 * h) = b;
            }
    }
}

// ------------------------------------------------------------------------------------------------ dQ
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_dq_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                        const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                        const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                        uint16_t* __restrict__ dq, ExB<FEAT> p, float c_log2) {
    static_assert((FEAT & (kFeatSink | kFeatPaged | kFeatKv8)) == 0, "forward-only bits");
    constexpr int NW = 8, BM = 32 * NW, BN = 64, NKS = D / 16, NDB = D / 32, TILE_BYTES = BN * D * 2;
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0, SC = (FEAT & kFeatScore) != 0;
    constexpr bool BIAS = (FEAT & kFeatBias) != 0;   // the bias joins the scores; this kernel also stores dS where it is asked for
    static_assert(!BIAS || (FEAT & ~kFeatBias) == kFeatScore, "a bias instantiation is the score-modifier body and nothing else");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][K tile | V tile]
    const int DR = p.d;
    int nq = p.nq, nk = p.nk;
    const int nqt = (nq + BM - 1) / BM;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;
    const int q0 = (L - bh * nqt) * BM;
    ExmUnit u;
    if constexpr (VAR) {
        u = exm_varlen_unit<FEAT>(p, bh, nq, nk);
        nq = u.lq; nk = u.lk; p.coff = u.lk - u.lq;
        if (q0 >= nq) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const size_t qbase = VAR ? (size_t)u.sq0 * p.sq + u.hh * DR : (size_t)bh * nq * DR;
    const size_t kbase = VAR ? (size_t)u.sk0 * p.sk + u.hk * DR : (size_t)kv_unit(bh, p.kvg) * nk * DR;
    const size_t vbase = VAR ? (size_t)u.sk0 * p.sv + u.hk * DR : kbase;
    const size_t obase = VAR ? ((size_t)u.sq0 * p.hq + u.hh) * DR : qbase;
    const size_t rbase = VAR ? (size_t)u.hh * p.total_q + u.sq0 : (size_t)bh * nq;
    const int ostr = VAR ? p.hq * DR : DR;   // rows of dout and dq
    const int qrow = q0 + 32 * w + r;
    const bool live_row = qrow < nq;

    const buf_rsrc_t q_rs = make_rsrc(q + qbase, VAR ? span_bytes(nq, DR, p.sq) : (unsigned)nq * DR * 2);
    const buf_rsrc_t o_rs = make_rsrc(dout + obase, VAR ? span_bytes(nq, DR, ostr) : (unsigned)nq * DR * 2);
    s16x8 qf[NKS], of[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        qf[ks] = buf_load_frag(q_rs, frag_off<VAR>(qrow, 16 * ks + 8 * h, DR, true, VAR ? p.sq : DR));
        of[ks] = buf_load_frag(o_rs, frag_off<VAR>(qrow, 16 * ks + 8 * h, DR, true, ostr));
    }
    const float nl = live_row ? nlse[rbase + qrow] : 0.f;
    const float nd = live_row ? ndelta[rbase + qrow] : 0.f;

    const rsrc_s_t k_rs = make_rsrc_s(k + kbase, VAR ? span_bytes(nk, DR, p.sk) : (unsigned)nk * DR * 2);
    const rsrc_s_t v_rs = make_rsrc_s(v + vbase, VAR ? span_bytes(nk, DR, p.sv) : (unsigned)nk * DR * 2);
    const int dma_voff = dma_lane_voff<D, VAR>(lane, w, DR, VAR ? p.sk : DR);
    const int dma_voff_v = VAR ? dma_lane_voff<D, VAR>(lane, w, DR, p.sv) : dma_voff;
    auto stage = [&](int buf, int k0) {
        char* kb_ = smem + buf * 2 * TILE_BYTES;
        dma_stage_tile<D, BN, NW, VAR>(k_rs, kb_, k0, dma_voff, w, DR, 0, VAR ? p.sk : DR);
        dma_stage_tile<D, BN, NW, VAR>(v_rs, kb_ + TILE_BYTES, k0, dma_voff_v, w, DR, 0, VAR ? p.sv : DR);
    };
    const MaskSrc msk = make_mask_src(p, bh);
    const bool use_bm = (FEAT & kFeatMask) && p.bmask != nullptr;
    const bool drop = (FEAT & kFeatDrop) && p.p_drop > 0.f;
    const unsigned hi = (unsigned)bh * p.nqh + ((unsigned)qrow >> 1);
    const int rbw = min(q0 + 32 * w, nq - 1) / p.br;
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = alibi_k(sc_of<FEAT>(p), bh);
    [[maybe_unused]] BiasSrc bsrc;
    [[maybe_unused]] uint16_t* dsrow = nullptr;   // this lane's row of dS (null: none to store)
    if constexpr (BIAS) {
        bsrc = make_bias_src(bias_of<FEAT>(p), bh, nq, nk);
        if (bsrc.ds && live_row) dsrow = bsrc.ds + (size_t)qrow * bsrc.s_rs;
    }

    f32x16 dqa[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dqa[t][i] = 0.f;

    constexpr bool WIN = (FEAT & kFeatWindow) != 0;   // (the tile ranges of the forward kernel)
    const int kend = WIN ? max(0, min(nk, min(q0 + BM, nq) + p.coff + p.wr)) : (p.causal ? max(0, min(nk, q0 + BM + p.coff)) : nk);
    const int kend_w = WIN ? (q0 + 32 * w < nq ? max(0, min(nk, min(q0 + 32 * w + 32, nq) + p.coff + p.wr)) : 0)
                           : (p.causal ? max(0, min(nk, q0 + 32 * w + 32 + p.coff)) : nk);
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const int t_lo = WIN ? max(0, q0 + p.coff - p.wl) / BN : 0;
    const int t_lo_w = WIN ? max(0, q0 + 32 * w + p.coff - p.wl) / BN : 0;
    LiveScan<true, BN> scan;
    if (use_bm) scan.init(p, q0, min(q0 + BM, nq), 0, nk, ntiles, lane);
    auto next_live = [&](int t) { return use_bm ? scan.next(t) : t; };
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int t = next_live(t_lo), cur = 0;
    if (t < ntiles) stage(0, t * BN);
    dma_wait_all();
    __syncthreads();
    if constexpr (WIN) {
        while (t < min(t_lo_w, ntiles)) {   // leading feed-only tiles
            const int tn = next_live(t + 1);
            if (tn < ntiles) stage(cur ^ 1, tn * BN);
            dma_wait_all();
            __syncthreads();
            cur ^= 1;
            t = tn;
        }
    }
    const bool late_stage = BIAS || ((FEAT & kFeatMask) && msk.on);   // see the forward kernel
    while (t < ntiles_w) {
        const int tn = next_live(t + 1);
        if (!late_stage && tn < ntiles) stage(cur ^ 1, tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * 2 * TILE_BYTES;
        const char* Vt = Kt + TILE_BYTES;
        u32x4 dsb[2][2];
        unsigned visw[2] = {0xffffu, 0xffffu};
        if constexpr (FEAT & kFeatMask) {
            if (msk.on) {
                visw[0] = dense_bits_q(msk, qrow, nk, k0 + 4 * h, h);
                visw[1] = dense_bits_q(msk, qrow, nk, k0 + 32 + 4 * h, h);
                if (tn < ntiles) stage(cur ^ 1, tn * BN);
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
                if (use_bm && p.bmask[rbw * p.nbc + min(k0 + 32 * kb, nk - 1) / p.bc] == 0) visw[kb] = 0;
        }
        [[maybe_unused]] u32x2 bw[2][4];   // kFeatBias: this lane's 2 x 16 bias values
        if constexpr (BIAS) {
            bias_load_q(bsrc, qrow, k0 + 4 * h, bw[0]);
            bias_load_q(bsrc, qrow, k0 + 32 + 4 * h, bw[1]);
            if (tn < ntiles) stage(cur ^ 1, tn * BN);
        }
        // a tile of which this wave sees nothing is not computed (wave-uniform; see the forward kernel)
        const bool any_vis = !(FEAT & kFeatMask) || __any((visw[0] | visw[1]) != 0) != 0;
        if (any_vis) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            unsigned vis = visw[kb], kp = 0xffffu;
            if constexpr (FEAT & kFeatDrop) {
                if (drop) kp = keep_bits_q(p, hi, qrow, k0 + 32 * kb + 4 * h);
            }
            f32x16 sacc, pacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if constexpr (SC) sacc[i] = 0.f;
                else sacc[i] = nl;
                pacc[i] = (FEAT & kFeatDrop) ? 0.f : nd;
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int off = TileSwz<D>::off(32 * kb + r, 2 * ks + h);
                const s16x8 ka = *reinterpret_cast<const s16x8*>(Kt + off);
                sacc = mfma32<Tag>(ka, qf[ks], sacc);
                const s16x8 va = *reinterpret_cast<const s16x8*>(Vt + off);
                pacc = mfma32<Tag>(va, of[ks], pacc);
            }
            [[maybe_unused]] float dt[16];
            if constexpr (SC) {   // modify S from 0, then add -lse / scale (the dK/dV kernel's order)
                if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        // dS = P (dP - delta) (1 - t^2) in fp32: without dropout dP - delta is final here, so dt goes in at once
                        float d;
                        sacc[i] = mod_softcap(sacc[i], sc_of<FEAT>(p), d);
                        if constexpr (FEAT & kFeatDrop) dt[i] = d;
                        else pacc[i] *= d;
                    }
                }
                if (sc_of<FEAT>(p).alibi) {
                    const float fb = (float)(qrow + p.coff - (k0 + 32 * kb + 4 * h));
#pragma unroll
                    for (int i = 0; i < 16; ++i) sacc[i] = mod_alibi(sacc[i], al, fb - (float)rc_of(i));
                }
                if constexpr (BIAS) bias_add_q<Tag>(sacc, bw[kb], bsrc.binv);
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[i] += nl;
            }
            const bool need_mask = WIN ? ((k0 + 32 * kb + 31 > q0 + 32 * w + p.coff + p.wr) || (k0 + 32 * kb + 32 > nk) ||
                                          (k0 + 32 * kb < q0 + 32 * w + 31 + p.coff - p.wl))
                                       : ((p.causal && (k0 + 32 * kb + 31 > q0 + 32 * w + p.coff)) || (k0 + 32 * kb + 32 > nk));
            const int lim = WIN ? min(qrow + p.coff + p.wr, nk - 1) : (p.causal ? min(qrow + p.coff, nk - 1) : nk - 1);
            const int thr = need_mask ? lim - (k0 + 32 * kb + 4 * h) : 64;
            [[maybe_unused]] const int thl = WIN && need_mask ? qrow + p.coff - p.wl - (k0 + 32 * kb + 4 * h) : -64;
            // wave-uniform (not in the dropout build: two copies of its selects cost registers it does not have)
            const bool plain = !(FEAT & kFeatDrop) && !need_mask && (!(FEAT & kFeatMask) || !__any(vis != 0xffffu));
            if (plain) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float dpv = pacc[i];
                    if constexpr (FEAT & kFeatDrop) dpv = (((kp >> i) & 1u) ? dpv * p.keep_scale : 0.f) + nd;
                    pacc[i] = __builtin_amdgcn_exp2f(sacc[i] * c_log2) * dpv;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    bool dead = rc_of(i) > thr;
                    if constexpr (WIN) dead = dead || rc_of(i) < thl;
                    if constexpr (FEAT & kFeatMask) dead = dead || !((vis >> i) & 1u);
                    float dpv = pacc[i];
                    if constexpr (FEAT & kFeatDrop) dpv = (((kp >> i) & 1u) ? dpv * p.keep_scale : 0.f) + nd;
                    pacc[i] = dead ? 0.f : __builtin_amdgcn_exp2f(sacc[i] * c_log2) * dpv;
                }
            }
            if constexpr (SC && (FEAT & kFeatDrop)) {   // dS *= 1 - t^2 in fp32, before the pack
                if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) pacc[i] *= dt[i];
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) dsb[kb][s][j] = pack2<Tag>(pacc[8 * s + 2 * j], pacc[8 * s + 2 * j + 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (BIAS) {   // dS out: the words of the MFMA below, group g = registers 4 g .. 4 g + 3 = words 2 (g & 1), + 1 of half g >> 1
            if (dsrow) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        bias_ds_store(dsrow, k0 + 32 * kb + 4 * h + 8 * g, nk, dsb[kb][g >> 1][2 * (g & 1)], dsb[kb][g >> 1][2 * (g & 1) + 1]);
            }
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const s16x8 sb = *reinterpret_cast<s16x8*>(&dsb[kb][s]);
                const int key_a = 32 * kb + 16 * s + 4 * h + tq;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const int ch = 4 * db + 2 * g16 + (tp >> 1);
                    const s16x8 a = cat8(lds_tr16(Kt + TileSwz<D>::off(key_a, ch) + 8 * (tp & 1)),
                                         lds_tr16(Kt + TileSwz<D>::off(key_a + 8, ch) + 8 * (tp & 1)));
                    dqa[db] = mfma32<Tag>(a, sb, dqa[db]);
                }
            }
        }   // any_vis
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    while (t < ntiles) {
        const int tn = next_live(t + 1);
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    if constexpr (BIAS) {
        // dS of the keys right of the tiles this wave computed (under the causal diagonal; a dead row computes none): zeros, so that
        // every element [:nq, :nk] is written by the call.  Row by row, the lanes across the row's keys.
        if (bsrc.ds) {
            for (int rr = 0; rr < 32 && q0 + 32 * w + rr < nq; ++rr) {
                uint16_t* zrow = bsrc.ds + (size_t)(q0 + 32 * w + rr) * bsrc.s_rs;
                for (int c = ntiles_w * BN + 4 * lane; c < nk; c += 256) bias_ds_store(zrow, c, nk, 0u, 0u);
            }
        }
    }
    if (live_row) {
        uint16_t* drow = dq + obase + (size_t)qrow * ostr;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (32 * db + 8 * g + 4 * h >= DR) continue;
                u32x2 val;
                val[0] = pack2_rn<Tag>(dqa[db][4 * g + 0] * p.scale, dqa[db][4 * g + 1] * p.scale);
                val[1] = pack2_rn<Tag>(dqa[db][4 * g + 2] * p.scale, dqa[db][4 * g + 3] * p.scale);
                *reinterpret_cast<u32x2*>(drow + 32 * db + 8 * g + 4 * h) = val;
            }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The forward launch of an instantiation.  LDS: two buffers of a K and a V tile; kFeatKv8: and the staging area, half a buffer.
template <typename Tag, int D, int FEAT>
static hipError_t exm_fwd_t(const ExArgs& a, hipStream_t st) {
    const size_t smem = 2 * 2 * 128 * D * 2 + ((FEAT & kFeatKv8) != 0 ? 2 * 128 * D : 0);
    auto kern = exm_fwd_kernel<Tag, D, FEAT>;
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((a.nq + 255) / 256) * a.bh));
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, grid, dim3(512), smem, st, (const uint16_t*)a.q, (const ExKV<FEAT>*)a.k, (const ExKV<FEAT>*)a.v,
                       (uint16_t*)a.o, a.lse, make_exm_block<FEAT>(a), a.scale * 1.4426950408889634f);
    return hipGetLastError();
}

// The backward launches of an instantiation, dense or packed (kFeatVarlen: a.cu_q is set): the pre-pass (fa_ex_mfma.hip), dK/dV, dQ.  FEAT never carries kFeatSink here: the backward
// of a sink call runs the kernels of the call without sinks, and ex_dsink_kernel for the sinks' gradient.
// workspace: [-lse/scale | -delta], one float per row each: (bh, nq), packed (heads_q, total_q)
template <typename Tag, int D, int FEAT>
static hipError_t exm_bwd_t(const ExArgs& a, hipStream_t st) {
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0;
    const long long rows = VAR ? (long long)a.heads_q * a.total_q : (long long)a.bh * a.nq;
    float* nlse = reinterpret_cast<float*>(a.workspace);
    float* ndelta = nlse + ((rows + 63) & ~63ll);
    const ExB<FEAT> p = make_exm_block<FEAT>(a);
    const float c = a.scale * 1.4426950408889634f;
    ProfScope ps(K_EX_BWD, st);
    hipError_t e = launch_exm_prep(a, a.d, nlse, ndelta, st);
    if (e != hipSuccess) return e;
    if (a.sinks) {   // the sink's gradient from the caller's lse and the -delta just written (packed: at (head, token), as lse)
        e = launch_ex_dsink(a, ndelta, VAR ? a.total_q : 0, 1, -1.f, st);
        if (e != hipSuccess) return e;
    }
    if (a.nk > 0) {
        const bool m16 = (FEAT & kFeatMask) && p.mask != nullptr && (p.nk & 15) == 0 && (p.mask_bh & 15) == 0 && (((uintptr_t)p.mask) & 15) == 0;
        const size_t smem = (size_t)256 * D * 2 + 4 * 64 * D * 2 + 2 * 128 * sizeof(float) + (m16 ? 8 * 1024 : 0)   // + the waves' mask images
                            + ((FEAT & kFeatBias) != 0 ? 8 * 2048 : 0);                                              // or their bias images
        auto kern = m16 ? exm_dkdv_kernel<Tag, D, FEAT, (FEAT & kFeatMask) != 0> : exm_dkdv_kernel<Tag, D, FEAT, false>;
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e != hipSuccess) return e;
        dim3 grid((unsigned)(((a.nk + 255) / 256) * a.bh));
        hipLaunchKernelGGL(kern, grid, dim3(512), smem, st, (const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v,
                           (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta, (uint16_t*)a.dk, (uint16_t*)a.dv, p, c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.nq > 0) {
        const size_t smem = 2 * 2 * 64 * D * 2;
        auto kern = exm_dq_kernel<Tag, D, FEAT>;
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e != hipSuccess) return e;
        dim3 grid((unsigned)(((a.nq + 255) / 256) * a.bh));
        hipLaunchKernelGGL(kern, grid, dim3(512), smem, st, (const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v,
                           (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta, (uint16_t*)a.dq, p, c);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace fa
