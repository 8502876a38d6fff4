// Extended attention on the 16-bit MFMA (bf16 / f16 tensors, head_dim a multiple of 8 up to 128): the notebook model's
// extras (fa_ex.hip has the list and the reference lines) on the decomposition of the plain kernels —
//   forward   (fa_fwd_mfma.hip)      : 8 waves x 32 query rows, K/V tiles of 128 keys by LDS-DMA, S^T = K Q^T with the query on
//                                      the lane, online softmax in registers, O^T += V^T P^T;
//   dK/dV     (fa_bwd_dkdv_mfma.hip) : 8 waves x 32 keys, Q/dO tiles of 64 rows, the key on the lane;
//   dQ        (fa_bwd_dq_mfma.hip)   : 8 waves x 32 query rows, K/V tiles of 64 keys, the query on the lane;
// with Nq != Nk (separate row counts, causal diagonal shifted by Nk - Nq), and per element
//   FEAT bit 0  dense mask and / or block-sparse mask (either pointer may be null at run time),
//   FEAT bit 1  dropout (counter-based, fa_ex_common.h: a lane makes one splitmix64 value per two of its elements),
//   FEAT bit 2  sliding window: row i sees keys [i + coff - wl, i + coff + wr].  The workgroup walks only the tiles of its
//               band; a wave computes the tiles of its own 32 rows (keys) and only helps to load the others, before
//               and after its own (feed-only); edge tiles mask per element against a lower and an upper threshold.
//               Without the bit the instantiations are the ones of the causal / unmasked kernels, unchanged.
//   FEAT bit 3  packed (varlen) sequences: the padded call's grid, each workgroup narrowed to its sequence (EXM_VARLEN_UNIT; the
//               fields in ExParams, fa_ex_common.h), token strides for q, k, v; combinable with bits 1 and 2, never with bit 0.
//   FEAT bit 4  score modifiers (softcap, ALiBi slopes): the parameter block grows by ExScore (ExParamsS), and the raw scores are
//               modified right after the S MFMAs, before any mask (mod_softcap / mod_alibi; on / off are wave-uniform run-time
//               switches).  The backward kernels then start S at 0 and add -lse / scale after the modifier, and dS takes the
//               softcap's 1 - t^2 in fp32 before its 16-bit pack.  Combinable with every other bit.
//   FEAT bit 5  attention sinks (forward only, always with bit 4): the parameter block grows once more (ExParamsK) and the
//               epilogue's normaliser takes the unit's sink logit as one more column (ex_sink_norm).  The key loop is bit 4's.
//               The backward of a sink call runs the kernels of the call without sinks and ex_dsink_kernel (fa_ex.hip).
//   FEAT bit 6  paged K/V (forward only, always with bit 3, never with bits 0 and 1): k and v are pools of pages and a sequence's
//               keys are found through a block table (ExPage: the parameter block grows by it, ExParamsPg).  Only the staging of
//               a K/V tile differs (dma_stage_kv_paged): each 1-KiB piece takes its page from one scalar table load and gets a
//               buffer descriptor of its own; everything after the staging is the text of the packed kernel, so a sequence gets
//               the bits of the packed call on the same tokens.  Kernels of their own (exm_fwd_paged_kernel).
//   FEAT bit 7  an e4m3 pool (always with bits 3 and 6): fa_ex_mfma_kv8.hip, a translation unit of its own.
// Dense mask bytes are fetched with range-checked buffer loads (rows / bytes past the mask read as 0 = masked); when Nk, the
// mask pointer and the (b,h) stride are multiples of 4 a lane of the query-on-the-lane kernels takes the 4 keys of a
// register group with one dword load.  The block-sparse mask needs br, bc multiples of 32 here (a wave's 32 x 32 block
// then has ONE entry; other block shapes take the exact-f32 kernels): tiles without a live entry are skipped before
// they are loaded, live tiles mask their dead 32 x 32 blocks.  A row without a visible key: o = 0, lse = -inf, dQ = 0.
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

}  // namespace

// ------------------------------------------------------------------------------------------------ forward
// Varlen (FEAT bit 3): the workgroup's unit bh = b * hq + h and its tile T0 come from the padded grid (nq, nk = the maxima); it
// narrows nq, nk, coff to sequence b (seq_span) and leaves before its first barrier when its tile starts past the sequence.
// Bases, buffer ranges and row strides become the sequence's; DR stays the column bound.
// (kFeatPaged: the keys are no span of a packed tensor — sk0 stays 0, the length is paged_len, ub names the table row)
#define EXM_VARLEN_UNIT(T0, N0)                                                                                         \
    [[maybe_unused]] int sq0 = 0, sk0 = 0, hh = 0, hk = 0, ub = 0;                                                      \
    if constexpr (VAR) {                                                                                                \
        const int b = bh / p.hq;                                                                                        \
        hh = bh - b * p.hq;                                                                                             \
        hk = kv_unit(hh, p.kvg);                                                                                        \
        int lq, lk;                                                                                                     \
        seq_span(p.cu_q, b, p.total_q, nq, sq0, lq);                                                                    \
        if constexpr ((FEAT & kFeatPaged) != 0) { ub = b; lk = paged_len(p.cu_k, b, nk); }                              \
        else seq_span(p.cu_k, b, p.total_k, nk, sk0, lk);                                                               \
        nq = lq; nk = lk; p.coff = lk - lq;                                                                             \
        if ((T0) >= (N0)) return;                                                                                       \
    }

template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_fwd_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                         const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                                                         float* __restrict__ lse, ExParams p, float c_log2) {
#include "fa_ex_mfma_fwd.inc"
}
// FEAT with kFeatScore: the parameter block grows by the modifiers (ExParamsS)
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_fwd_score_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                               const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                                                               float* __restrict__ lse, ExParamsS p, float c_log2) {
#include "fa_ex_mfma_fwd.inc"
}
// FEAT with kFeatSink (and kFeatScore): the parameter block grows by the sinks (ExParamsK)
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_fwd_sink_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                              const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                                                              float* __restrict__ lse, ExParamsK p, float c_log2) {
#include "fa_ex_mfma_fwd.inc"
}

// FEAT with kFeatPaged (and kFeatVarlen): the parameter block of the instantiation without the bit grows by the pages (ExParamsPg)
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_fwd_paged_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                               const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                                                               float* __restrict__ lse, ExParamsPg<ExP<FEAT>> p, float c_log2) {
#include "fa_ex_mfma_fwd.inc"
}

// ------------------------------------------------------------------------------------------------ row constants
// nlse = -lse / scale (0 for a row without a visible key: every element of such a row is masked by a select, and an
// infinite initial accumulator would only make NaNs on the way), ndelta = -rowsum(dO * O).  16 lanes per row.
// dlse != null (fa_ex_backward_dlse): ndelta = dlse - rowsum(dO * O), the gradient of the row's lse, which is all a gradient of lse
// does to the backward (dS = P (dP + ndelta)); a row whose lse is -inf ignores its dlse.
template <typename Tag>
__global__ __launch_bounds__(256) void exm_prep_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ dout,
                                                       const float* __restrict__ lse, float* __restrict__ nlse,
                                                       float* __restrict__ ndelta, long long rows, int d, float inv_scale,
                                                       const float* __restrict__ dlse) {
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    float s = 0.f;
    if (row < rows && 8 * sub < d) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(o + row * d + 8 * sub);
        const u32x4 b = *reinterpret_cast<const u32x4*>(dout + row * d + 8 * sub);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += unpack_lo<Tag>(a[j]) * unpack_lo<Tag>(b[j]) + unpack_hi<Tag>(a[j]) * unpack_hi<Tag>(b[j]);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (row < rows && sub == 0) {
        const float l = lse[row];
        nlse[row] = (l == -INFINITY) ? 0.f : -l * inv_scale;
        ndelta[row] = (dlse && l != -INFINITY) ? dlse[row] - s : -s;
    }
}

// the same for packed sequences: o, dout (total_q, hq, d); lse and the two outputs (hq, total_q).  Workgroup x: head x / tph,
// tokens 16 (x % tph) ..  Tokens no sequence covers get constants of their unspecified lse (no kernel reads them).
template <typename Tag>
__global__ __launch_bounds__(256) void exm_prep_varlen_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ dout,
                                                              const float* __restrict__ lse, float* __restrict__ nlse,
                                                              float* __restrict__ ndelta, int total_q, int tph, int hq, int d,
                                                              float inv_scale, const float* __restrict__ dlse) {
    const int hd = blockIdx.x / tph;
    const int tok = (blockIdx.x - hd * tph) * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    const size_t row = ((size_t)tok * hq + hd) * d;
    float s = 0.f;
    if (tok < total_q && 8 * sub < d) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(o + row + 8 * sub);
        const u32x4 b = *reinterpret_cast<const u32x4*>(dout + row + 8 * sub);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += unpack_lo<Tag>(a[j]) * unpack_lo<Tag>(b[j]) + unpack_hi<Tag>(a[j]) * unpack_hi<Tag>(b[j]);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (tok < total_q && sub == 0) {
        const size_t i = (size_t)hd * total_q + tok;
        const float l = lse[i];
        nlse[i] = (l == -INFINITY) ? 0.f : -l * inv_scale;
        ndelta[i] = (dlse && l != -INFINITY) ? dlse[i] - s : -s;
    }
}

// ------------------------------------------------------------------------------------------------ dK / dV
// M16: the dense mask (if any) is 16-byte aligned in every respect — its bytes come through the wave's LDS image
// (dense_bits_k_lds); a separate instantiation, not a run-time choice: with both loaders in one kernel the masked form spills
template <typename Tag, int D, int FEAT, bool M16 = false>
__global__ __launch_bounds__(512, 2) void exm_dkdv_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                          const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                          const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                          uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, ExParams p,
                                                          float c_log2) {
#include "fa_ex_mfma_dkdv.inc"
}
template <typename Tag, int D, int FEAT, bool M16 = false>
__global__ __launch_bounds__(512, 2) void exm_dkdv_score_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                                const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                                const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                                uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, ExParamsS p,
                                                                float c_log2) {
#include "fa_ex_mfma_dkdv.inc"
}
// ------------------------------------------------------------------------------------------------ dQ
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_dq_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                        const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                        const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                        uint16_t* __restrict__ dq, ExParams p, float c_log2) {
#include "fa_ex_mfma_dq.inc"
}
template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_dq_score_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                              const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                              const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                              uint16_t* __restrict__ dq, ExParamsS p, float c_log2) {
#include "fa_ex_mfma_dq.inc"
}
// ------------------------------------------------------------------------------------------------ host side
bool ex_mfma_supported(const ExArgs& a) {
    if (a.dtype != 1 && a.dtype != 2) return false;
    if (a.d < 8 || a.d > 128 || a.d % 8 != 0) return false;
    if (!(a.scale > 0.f)) return false;                       // the running max is taken on the raw scores
    if (a.block_mask && (a.br % 32 != 0 || a.bc % 32 != 0)) return false;
    if (a.mask && a.nq * a.nk >= ((int64_t)1 << 31)) return false;   // 32-bit byte offsets into one (b,h)'s mask
    if (a.bh * ((a.nq + 1) / 2) >= ((int64_t)1 << 32)) return false;  // the generator's row-pair counter
    return true;
}

// the kernel entry of an instantiation: exm_*_score_kernel with kFeatScore
template <typename Tag, int D, int FEAT> static auto exm_fwd_entry() {
    if constexpr ((FEAT & kFeatSink) != 0) return exm_fwd_sink_kernel<Tag, D, FEAT>;
    else if constexpr ((FEAT & kFeatScore) != 0) return exm_fwd_score_kernel<Tag, D, FEAT>;
    else return exm_fwd_kernel<Tag, D, FEAT>;
}
template <typename Tag, int D, int FEAT, bool M16> static auto exm_dkdv_entry() {
    if constexpr ((FEAT & kFeatScore) != 0) return exm_dkdv_score_kernel<Tag, D, FEAT, M16>;
    else return exm_dkdv_kernel<Tag, D, FEAT, M16>;
}
template <typename Tag, int D, int FEAT> static auto exm_dq_entry() {
    if constexpr ((FEAT & kFeatScore) != 0) return exm_dq_score_kernel<Tag, D, FEAT>;
    else return exm_dq_kernel<Tag, D, FEAT>;
}

template <typename Tag, int D, int FEAT>
static hipError_t exm_fwd_t(const ExArgs& a, hipStream_t st) {
    const size_t smem = 2 * 2 * 128 * D * 2;
    auto kern = exm_fwd_entry<Tag, D, FEAT>();
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((a.nq + 255) / 256) * a.bh));
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, grid, dim3(512), smem, st, (const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v,
                       (uint16_t*)a.o, a.lse, make_exm_params<FEAT>(a), a.scale * 1.4426950408889634f);
    return hipGetLastError();
}

// (FEAT never carries kFeatSink here: the backward of a sink call runs the kernels of the call without sinks)
template <typename Tag, int D, int FEAT>
static hipError_t exm_bwd_t(const ExArgs& a, hipStream_t st) {
    const long long rows = (long long)a.bh * a.nq;
    float* nlse = reinterpret_cast<float*>(a.workspace);
    float* ndelta = nlse + ((rows + 63) & ~63ll);
    const ExP<FEAT> p = make_exm_params<FEAT>(a);
    const float c = a.scale * 1.4426950408889634f;
    ProfScope ps(K_EX_BWD, st);
    hipLaunchKernelGGL(exm_prep_kernel<Tag>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, (const uint16_t*)a.o,
                       (const uint16_t*)a.dout, (const float*)a.lse, nlse, ndelta, rows, (int)a.d, 1.f / a.scale, a.dlse);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.sinks) {   // the sink's gradient from the caller's lse and the -delta just written
        e = launch_ex_dsink(a, ndelta, 0, 1, -1.f, st);
        if (e != hipSuccess) return e;
    }
    if (a.nk > 0) {
        const bool m16 = (FEAT & kFeatMask) && p.mask != nullptr && (p.nk & 15) == 0 && (p.mask_bh & 15) == 0 && (((uintptr_t)p.mask) & 15) == 0;
        const size_t smem = (size_t)256 * D * 2 + 4 * 64 * D * 2 + 2 * 128 * sizeof(float) + (m16 ? 8 * 1024 : 0);   // + the waves' mask images
        auto kern = m16 ? exm_dkdv_entry<Tag, D, FEAT, (FEAT & kFeatMask) != 0>() : exm_dkdv_entry<Tag, D, FEAT, false>();
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
        auto kern = exm_dq_entry<Tag, D, FEAT>();
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e != hipSuccess) return e;
        dim3 grid((unsigned)(((a.nq + 255) / 256) * a.bh));
        hipLaunchKernelGGL(kern, grid, dim3(512), smem, st, (const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v,
                           (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta, (uint16_t*)a.dq, p, c);
        e = hipGetLastError();
    }
    return e;
}

// The row-constant pre-pass for the kernels of another translation unit (fa_ex_mfma_vdim.hip): exm_prep_kernel /
// exm_prep_varlen_kernel as exm_bwd_t and exm_varlen_t launch them, with d_row the row width of o and dout.
hipError_t launch_exm_prep(const ExArgs& a, int64_t d_row, float* nlse, float* ndelta, hipStream_t st) {
    const bool bf = a.dtype == 2;
    if (a.cu_q) {
        const int tph = (int)((a.total_q + 15) / 16);
        auto kern = bf ? exm_prep_varlen_kernel<bf16_tag> : exm_prep_varlen_kernel<f16_tag>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(tph * a.heads_q)), dim3(256), 0, st, (const uint16_t*)a.o, (const uint16_t*)a.dout,
                           (const float*)a.lse, nlse, ndelta, (int)a.total_q, tph, (int)a.heads_q, (int)d_row, 1.f / a.scale, a.dlse);
    } else {
        const long long rows = (long long)a.bh * a.nq;
        auto kern = bf ? exm_prep_kernel<bf16_tag> : exm_prep_kernel<f16_tag>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, (const uint16_t*)a.o, (const uint16_t*)a.dout,
                           (const float*)a.lse, nlse, ndelta, rows, (int)d_row, 1.f / a.scale, a.dlse);
    }
    return hipGetLastError();
}

// S: 0, or kFeatScore for a call with a score modifier (every other feature combination once more with it)
template <typename Tag, int D, int S>
static hipError_t exm_by_feat_s(const ExArgs& a, bool backward, hipStream_t st) {
    const bool masks = a.mask || a.block_mask, drop = a.dropout_p > 0.0;
    if (ex_windowed(a)) {
        if (drop) return backward ? exm_bwd_t<Tag, D, S | 7>(a, st) : exm_fwd_t<Tag, D, S | 7>(a, st);
        if (masks) return backward ? exm_bwd_t<Tag, D, S | 5>(a, st) : exm_fwd_t<Tag, D, S | 5>(a, st);
        return backward ? exm_bwd_t<Tag, D, S | 4>(a, st) : exm_fwd_t<Tag, D, S | 4>(a, st);
    }
    if (drop) return backward ? exm_bwd_t<Tag, D, S | 3>(a, st) : exm_fwd_t<Tag, D, S | 3>(a, st);
    if (masks) return backward ? exm_bwd_t<Tag, D, S | 1>(a, st) : exm_fwd_t<Tag, D, S | 1>(a, st);
    return backward ? exm_bwd_t<Tag, D, S>(a, st) : exm_fwd_t<Tag, D, S>(a, st);
}
// the forward of a sink call: one sink entry per feature combination, on the score-modifier body
template <typename Tag, int D>
static hipError_t exm_fwd_sink(const ExArgs& a, hipStream_t st) {
    constexpr int S = kFeatScore | kFeatSink;
    const bool masks = a.mask || a.block_mask, drop = a.dropout_p > 0.0;
    if (ex_windowed(a)) {
        if (drop) return exm_fwd_t<Tag, D, S | 7>(a, st);
        if (masks) return exm_fwd_t<Tag, D, S | 5>(a, st);
        return exm_fwd_t<Tag, D, S | 4>(a, st);
    }
    if (drop) return exm_fwd_t<Tag, D, S | 3>(a, st);
    if (masks) return exm_fwd_t<Tag, D, S | 1>(a, st);
    return exm_fwd_t<Tag, D, S>(a, st);
}
template <typename Tag, int D>
static hipError_t exm_by_feat(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.sinks && !backward) return exm_fwd_sink<Tag, D>(a, st);
    return ex_scoremod(a) ? exm_by_feat_s<Tag, D, kFeatScore>(a, backward, st) : exm_by_feat_s<Tag, D, 0>(a, backward, st);
}

// ---- packed sequences: the varlen kernels on the padded grid (a.bh = batch * heads_q units, a.nq / a.nk = the maxima)
bool ex_mfma_varlen_supported(const ExArgs& a) {
    if (!ex_mfma_supported(a)) return false;
    if (a.stride_q % 8 != 0 || a.stride_k % 8 != 0 || a.stride_v % 8 != 0) return false;   // 16-byte rows
    const void* ptrs[] = {a.q, a.k, a.v, a.o, a.dout, a.dq, a.dk, a.dv};
    for (const void* ptr : ptrs)
        if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) return false;
    int64_t smax = a.heads_q * a.d;   // o, dout, dq rows
    if (a.stride_q > smax) smax = a.stride_q;
    if (a.stride_k > smax) smax = a.stride_k;
    if (a.stride_v > smax) smax = a.stride_v;
    const int64_t nmax = a.nq > a.nk ? a.nq : a.nk;
    return nmax * smax * 2 < ((int64_t)1 << 31);   // the 32-bit buffer offsets inside one sequence
}

template <typename Tag, int D, int FEAT>
static hipError_t exm_varlen_fwd_t(const ExArgs& a, hipStream_t st) {
    const ExP<FEAT> p = make_exm_params<FEAT>(a);
    const float c = a.scale * 1.4426950408889634f;
    const size_t smem = 2 * 2 * 128 * D * 2;
    auto kern = exm_fwd_entry<Tag, D, FEAT | kFeatVarlen>();
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nq + 255) / 256) * a.bh)), dim3(512), smem, st, (const uint16_t*)a.q,
                       (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.o, a.lse, p, c);
    return hipGetLastError();
}

template <typename Tag, int D, int FEAT>
static hipError_t exm_varlen_t(const ExArgs& a, bool backward, hipStream_t st) {
    if (!backward) return exm_varlen_fwd_t<Tag, D, FEAT>(a, st);
    const ExP<FEAT> p = make_exm_params<FEAT>(a);
    const float c = a.scale * 1.4426950408889634f;
    hipError_t e;
    // workspace: [-lse/scale | -delta], (heads_q, total_q) each
    const long long rows = (long long)a.heads_q * a.total_q;
    float* nlse = reinterpret_cast<float*>(a.workspace);
    float* ndelta = nlse + ((rows + 63) & ~63ll);
    const int tph = (int)((a.total_q + 15) / 16);
    ProfScope ps(K_EX_BWD, st);
    hipLaunchKernelGGL(exm_prep_varlen_kernel<Tag>, dim3((unsigned)(tph * a.heads_q)), dim3(256), 0, st, (const uint16_t*)a.o,
                       (const uint16_t*)a.dout, (const float*)a.lse, nlse, ndelta, (int)a.total_q, tph, (int)a.heads_q, (int)a.d,
                       1.f / a.scale, a.dlse);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.sinks) {   // (-delta at (head, token), as lse)
        e = launch_ex_dsink(a, ndelta, a.total_q, 1, -1.f, st);
        if (e != hipSuccess) return e;
    }
    {
        const size_t smem = (size_t)256 * D * 2 + 4 * 64 * D * 2 + 2 * 128 * sizeof(float);
        auto kern = exm_dkdv_entry<Tag, D, FEAT | kFeatVarlen, false>();
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nk + 255) / 256) * a.bh)), dim3(512), smem, st, (const uint16_t*)a.q,
                           (const uint16_t*)a.k, (const uint16_t*)a.v, (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta,
                           (uint16_t*)a.dk, (uint16_t*)a.dv, p, c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const size_t smem = 2 * 2 * 64 * D * 2;
    auto kern = exm_dq_entry<Tag, D, FEAT | kFeatVarlen>();
    e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nq + 255) / 256) * a.bh)), dim3(512), smem, st, (const uint16_t*)a.q,
                       (const uint16_t*)a.k, (const uint16_t*)a.v, (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta,
                       (uint16_t*)a.dq, p, c);
    return hipGetLastError();
}

template <typename Tag, int D, int S>
static hipError_t exm_varlen_by_feat_s(const ExArgs& a, bool backward, hipStream_t st) {
    const bool drop = a.dropout_p > 0.0;
    if (ex_windowed(a)) return drop ? exm_varlen_t<Tag, D, S | kFeatWindow | kFeatDrop>(a, backward, st) : exm_varlen_t<Tag, D, S | kFeatWindow>(a, backward, st);
    return drop ? exm_varlen_t<Tag, D, S | kFeatDrop>(a, backward, st) : exm_varlen_t<Tag, D, S>(a, backward, st);
}
template <typename Tag, int D>
static hipError_t exm_varlen_by_feat(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.sinks && !backward) {   // the forward of a sink call
        constexpr int S = kFeatScore | kFeatSink;
        const bool drop = a.dropout_p > 0.0;
        if (ex_windowed(a)) return drop ? exm_varlen_fwd_t<Tag, D, S | kFeatWindow | kFeatDrop>(a, st) : exm_varlen_fwd_t<Tag, D, S | kFeatWindow>(a, st);
        return drop ? exm_varlen_fwd_t<Tag, D, S | kFeatDrop>(a, st) : exm_varlen_fwd_t<Tag, D, S>(a, st);
    }
    return ex_scoremod(a) ? exm_varlen_by_feat_s<Tag, D, kFeatScore>(a, backward, st) : exm_varlen_by_feat_s<Tag, D, 0>(a, backward, st);
}

// ---- paged K/V (a.block_table != null): the varlen forward with kFeatPaged, {window} x {plain, score, score + sink}
bool ex_mfma_paged_supported(const ExArgs& a) {
    if (!ex_mfma_supported(a) || a.dropout_p > 0.0) return false;
    if (a.stride_q % 8 != 0 || a.stride_k % 8 != 0 || a.stride_v % 8 != 0 || a.page_stride_k % 8 != 0 || a.page_stride_v % 8 != 0) return false;
    const void* ptrs[] = {a.q, a.k, a.v, a.o};
    for (const void* ptr : ptrs)
        if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) return false;
    const int64_t sq = a.stride_q > a.heads_q * a.d ? a.stride_q : a.heads_q * a.d;
    const int64_t skv = a.stride_k > a.stride_v ? a.stride_k : a.stride_v;
    // the 32-bit buffer offsets: inside one sequence of q and o, inside one piece (at most 8 rows) of a page
    return a.nq * sq * 2 < ((int64_t)1 << 31) && 8 * skv * 2 < ((int64_t)1 << 31);
}

template <typename Tag, int D, int FEAT>
static hipError_t exm_paged_fwd_t(const ExArgs& a, hipStream_t st) {
    ExParamsPg<ExP<FEAT>> p;
    static_cast<ExP<FEAT>&>(p) = make_exm_params<FEAT>(a);
    p.pg = make_ex_page(a);
    const size_t smem = 2 * 2 * 128 * D * 2;
    auto kern = exm_fwd_paged_kernel<Tag, D, FEAT | kFeatVarlen | kFeatPaged>;
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nq + 255) / 256) * a.bh)), dim3(512), smem, st, (const uint16_t*)a.q,
                       (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.o, a.lse, p, a.scale * 1.4426950408889634f);
    return hipGetLastError();
}
template <typename Tag, int D>
static hipError_t exm_paged_by_feat(const ExArgs& a, hipStream_t st) {
    const bool win = ex_windowed(a);
    if (a.sinks) return win ? exm_paged_fwd_t<Tag, D, kFeatScore | kFeatSink | kFeatWindow>(a, st) : exm_paged_fwd_t<Tag, D, kFeatScore | kFeatSink>(a, st);
    if (ex_scoremod(a)) return win ? exm_paged_fwd_t<Tag, D, kFeatScore | kFeatWindow>(a, st) : exm_paged_fwd_t<Tag, D, kFeatScore>(a, st);
    return win ? exm_paged_fwd_t<Tag, D, kFeatWindow>(a, st) : exm_paged_fwd_t<Tag, D, 0>(a, st);
}
// (the caller has checked ex_mfma_paged_supported, and that max_seqlen_q and the key cap are > 0)
hipError_t launch_ex_mfma_varlen_paged(const ExArgs& a, hipStream_t st) {
    if (a.dtype == 2) return a.d > 64 ? exm_paged_by_feat<bf16_tag, 128>(a, st) : exm_paged_by_feat<bf16_tag, 64>(a, st);
    return a.d > 64 ? exm_paged_by_feat<f16_tag, 128>(a, st) : exm_paged_by_feat<f16_tag, 64>(a, st);
}

// (the caller has checked ex_mfma_varlen_supported, and that max_seqlen_q, max_seqlen_k, total_q, total_k are > 0)
hipError_t launch_ex_mfma_varlen(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.dtype == 2) return a.d > 64 ? exm_varlen_by_feat<bf16_tag, 128>(a, backward, st) : exm_varlen_by_feat<bf16_tag, 64>(a, backward, st);
    return a.d > 64 ? exm_varlen_by_feat<f16_tag, 128>(a, backward, st) : exm_varlen_by_feat<f16_tag, 64>(a, backward, st);
}

hipError_t launch_ex_mfma(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.dtype == 2) return a.d > 64 ? exm_by_feat<bf16_tag, 128>(a, backward, st) : exm_by_feat<bf16_tag, 64>(a, backward, st);
    return a.d > 64 ? exm_by_feat<f16_tag, 128>(a, backward, st) : exm_by_feat<f16_tag, 64>(a, backward, st);
}

}  // namespace fa
