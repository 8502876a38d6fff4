// What the two readers of the MXFP4 KV cache share at the head dims D = 64 and 256 (fp4kv_split_hdim_kernel in fa_fp4_decode.hip,
// fp4kv_prefill_hdim_kernel in fa_fp4_prefill.hip): the per-width facts, and one 64-key tile of a wave from its operands on.  One
// definition each; the operand orders, the softmax and the V^T image are argued in fa_fp4_decode.hip's header.  The two 128 kernels
// keep their own inline text and use nothing of this file but fp4h_width (why: profiles/fp4_merge.md).
#pragma once
#include "fa_kvq_common.h"

namespace fa {

namespace {

// The per-width facts                               D = 64   (128)   D = 256
//   NM     S^T instructions a 32-key block             1       2         4
//   NDV    O^T instructions a tile, 32 channels each   2       4         8
//   HB     code bytes a key and head                  32      64       128
//   SB     k_scale bytes a key and head (a row)        2       4         8    read as a ushort, (a dword,) two dwords
//   VT     bytes of the V^T image, vt4_off(D)       2176    4352      8704
//   KROW   a key's row in the prefill K stage         48      80       144    HB + SB padded to an ODD multiple of 16
//   WAVES  a SIMD                                      2       2         1
// One wave a SIMD at 256: O^T is 8 x 16 = 128 fp32 accumulators, q four operands (32), a tile's scores and exponents 64 more:
// beyond the 256 registers of two waves a SIMD.  Both readers run ONE wave a SIMD there (512 registers, the accumulators in
// AGPRs), as the e4m3 kernel does at 256.  The other way, the value channels split over two waves, reads K and runs S twice or
// hands P' through LDS behind a barrier a tile; the decode wave has no barrier today and is bound by the cache bytes it pulls,
// which the split count, not the occupancy, spreads over the chip.  No kernel of the two files uses scratch.
template <int D> struct Fp4Hd {
    static_assert(D == 64 || D == 256, "the 128 readers have their own text");
    static constexpr int KT = 64, NM = D / 64, NDV = D / 32, HB = D / 2, SB = D / 32;   // HB / SB: code / k_scale bytes a key and head
    static constexpr int VT = 34 * D;                      // the V^T image: vt4_off(D)
    static constexpr int KROW = D == 64 ? 48 : 144;        // a key's row in the prefill K stage
    static constexpr int WAVES = D == 256 ? 1 : 2;         // a SIMD
};

// a key's k_scale row (D / 32 bytes, global or LDS) as two words (the second is read at D = 256 alone)
template <int D> __device__ __forceinline__ void fp4h_scale_row(const void* sp, uint32_t (&w)[2]) {
    if constexpr (D == 64) {
        w[0] = *reinterpret_cast<const uint16_t*>(sp);
        w[1] = 0u;
    } else {
        const u32x2 x = *reinterpret_cast<const u32x2*>(sp);
        w[0] = x[0];
        w[1] = x[1];
    }
}

// the lane's e4m3 q operands: qp = the row's D bytes + 16 h
// (an 8-bit operand's byte 16 g + x of lane half h is k = 32 g + 16 h + x: the two 16-byte halves lie 32 channels apart)
template <int NM> __device__ __forceinline__ void fp4h_load_q(const uint8_t* qp, bool valid, i32x8_t (&qb)[NM]) {
#pragma unroll
    for (int M = 0; M < NM; ++M) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(qp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(qp + 64 * M + 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qb[M][i] = valid ? (int)a0[i] : 0;
            qb[M][4 + i] = valid ? (int)a1[i] : 0;
        }
    }
}

// S^T of one 32-key block: a[M] the lane's 16 code bytes at 32 M + 16 h, w its key's scale row; instruction M's block is 2 M + h
template <int NM> __device__ __forceinline__ f32x16 fp4h_scores(const u32x4 (&a)[NM], const uint32_t (&w)[2], int h, const i32x8_t (&qb)[NM]) {
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int M = 0; M < NM; ++M) {
        const i32x8_t ka = {(int)a[M][0], (int)a[M][1], (int)a[M][2], (int)a[M][3], 0, 0, 0, 0};
        const int sc = (int)((w[M >> 1] >> (16 * (M & 1) + 8 * h)) & 0xffu);
        s = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb[M], s, kFp4, 0, 0, sc, 0, 127);
    }
    return s;
}

// what the softmax of a lane's row needs beside the scores
struct Fp4hRow {
    bool valid, capped;
    int rhi, rlo;                         // the row sees keys [rlo, rhi] (rlo: a window alone)
    float fe, ck, cap2;                   // fe: the factor of what the accumulators hold after the cap; ck = f cap_k
};

// One 64-key tile from its scores on: evb the tile's 64 V exponents by key, vtb its V^T image.
//   softcap (before the mask): the capped score in log2 units, cap2 (1 - 2 r) with r = 1 / (2^(ck s) + 1), replaces s f: one exp2
//   and one rcp an element.
//   the mask, t = (s f or the capped score) + ev, the row maximum over t.  The selects run only where need_mask / need_lo say
//   that a row's upper bound, the end, or with a window a row's lower bound lies inside this key tile (wave-uniform).  A masked
//   key's score is -inf BEFORE ev is added: its ev never reaches the joint maximum.
//   the lazy rescale (threshold 8) under the joint running maximum, P' rounded to e4m3, l from the unrounded ldexp, and
//   O^T += V^T P'^T: the lane's 16 key bytes (32 keys) of channel 32 dvb + r out of the image.
template <int D>
__device__ __forceinline__ void fp4h_softmax_pv(f32x16 (&sacc)[2], const int* evb, const char* vtb, f32x16 (&oacc)[D / 32], float& m_run,
                                                float& l_run, const Fp4hRow& rw, int k0, int r, int h, bool need_mask, bool need_lo) {
    if (rw.capped) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * rw.ck) + 1.f);
                sacc[kb][i] = fmaf(rr, -2.f * rw.cap2, rw.cap2);
            }
    }
    int ev[2][16];
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i32x4_t e4 = *reinterpret_cast<const i32x4_t*>(evb + 32 * kb + 4 * h + 8 * j);
#pragma unroll
            for (int c = 0; c < 4; ++c) ev[kb][4 * j + c] = e4[c];
        }
        if (need_mask) {
            const int thr = rw.rhi - (k0 + 32 * kb + 4 * h);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
        }
        if (need_lo) {
            const int thr = rw.rlo - (k0 + 32 * kb + 4 * h);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((i & 3) + 8 * (i >> 2) < thr) sacc[kb][i] = -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sacc[kb][i] = fmaf(sacc[kb][i], rw.fe, (float)ev[kb][i]);   // (a masked key stays -inf whatever its ev: fe > 0)
            mx = fmaxf(mx, sacc[kb][i]);
        }
    }
    mx = fmaxf(mx, wave_half_swap(mx));
    const float m_new = fmaxf(m_run, mx);
    float m_use;
    if (__any(rw.valid && m_new - m_run > 8.0f) != 0) {   // lazy rescale on the real rows; a row's first visible key: inf > 8
        m_use = m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int t2 = 0; t2 < D / 32; ++t2)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
    } else {
        m_use = m_run;
    }
    if (m_use == -INFINITY) m_use = 0.f;      // a row without a visible key so far: p = exp2(-inf) = 0, not exp2(-inf + inf)
    float rs = 0.f;
    i32x8_t pb;                               // P'^T as the accumulators hold it, rounded to e4m3 (RNE)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float pe = __builtin_amdgcn_exp2f(sacc[kb][i] - m_use);
            sacc[kb][i] = pe;
            rs += __builtin_ldexpf(pe, -ev[kb][i]);          // the key's share of l: exp2(s f - M), V's scale taken out again
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int wd = 0;
            wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 0], sacc[kb][4 * j + 1], wd, false);
            wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 2], sacc[kb][4 * j + 3], wd, true);
            pb[4 * kb + j] = wd;
        }
    }
    l_run += rs;
#pragma unroll
    for (int dvb = 0; dvb < D / 32; ++dvb) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(vtb + vt4_off(32 * dvb + r) + 16 * h);
        const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], 0, 0, 0, 0};
        oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], kFp4, 0, 0, 127, 0, 127);
    }
}

// a lane's row of O^T out: register i of block dvb is channel 32 dvb + 4 h + (i & 3) + 8 (i >> 2); scaled by inv, zeros if dead
template <typename Tag, int NDV> __device__ __forceinline__ void fp4h_store_o(uint16_t* orow, const f32x16 (&oacc)[NDV], float inv, bool dead, int h) {
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
            u32x2 v;
            v[0] = pack2_rn<Tag>(y[0], y[1]);
            v[1] = pack2_rn<Tag>(y[2], y[3]);
            *reinterpret_cast<u32x2*>(orow + 32 * dvb + 8 * g + 4 * h) = v;
        }
}

// four keys' dwords (eight channels each) to the even-channel and odd-channel dwords of key pairs (0, 1) and (2, 3), two keys a byte
__device__ __forceinline__ void fp4h_pair_nibbles(const uint32_t (&x)[4], uint32_t& e01, uint32_t& o01, uint32_t& e23, uint32_t& o23) {
    constexpr uint32_t LO = 0x0f0f0f0fu;
    e01 = (x[0] & LO) | ((x[1] & LO) << 4);
    o01 = ((x[0] >> 4) & LO) | (x[1] & ~LO);
    e23 = (x[2] & LO) | ((x[3] & LO) << 4);
    o23 = ((x[2] >> 4) & LO) | (x[3] & ~LO);
}

// f(std::integral_constant<int, d>) for d in {64, 128, 256} (the launchers have refused any other)
template <typename F> inline void fp4h_width(int64_t d, F&& f) {
    if (d == 64) f(std::integral_constant<int, 64>{});
    else if (d == 128) f(std::integral_constant<int, 128>{});
    else f(std::integral_constant<int, 256>{});
}

}  // namespace

}  // namespace fa
