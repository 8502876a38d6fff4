// Extended attention forward / backward for gfx950: the extras the reference's notebook model wires around its tiled
// attention (src/fa3/torch/flashattention_pytorch.py), as kernel features behind one entry point:
//   * Nq != Nk with the causal mask aligned bottom-right: key j is visible to query i iff j <= i + (Nk - Nq)
//     (look_ahead_mask_, flashattention_pytorch.py:176-190);
//   * a dense mask [Nq][Nk] of bytes, 0 = masked (scores.masked_fill(mask == 0, -inf), :139-141), shared by all (b,h) or
//     one per (b,h);
//   * a block-sparse mask [ceil(Nq/br)][ceil(Nk/bc)], 0 = the tile is skipped (Algorithm 5, line 8: :123-125);
//   * dropout on the attention probabilities, in-kernel: keep where rnd > p, scale 1/(1-p) (src/common/dropout.py:9-15,
//     flashattention_pytorch.py:85-87), with a counter-based generator so that the backward regenerates the mask from
//     (seed, b*h, i, j) instead of storing it; `tau` (:134) folds into softmax_scale;
//   * a sliding window (no reference counterpart; FlashAttention-2's window_size): key j is visible to query i only if
//     i + (Nk - Nq) - wl <= j <= i + (Nk - Nq) + wr (ExParams: wr = 0 under the causal mask, kWinNone when unbounded); the
//     key (query) tile ranges of every kernel are cut to the band at both ends.
//   * packed (varlen) sequences (FlashAttention-2's flash_attn_varlen_func): each workgroup of the padded call's grid works inside
//     its own sequence, in entries of their own (ex_*_varlen_kernel) around the bodies the other kernels share.
//   * a paged K/V cache under the packed forward (FlashAttention-2's block_table of flash_attn_varlen_func): k and v are pools of
//     pages and a sequence's keys are found through a table (ExPage), one lookup per row of a K/V tile (ex_load_tile_paged); entries
//     of their own again (ex_fwd_varlen_paged_kernel: the forward body with ExParamsPg).
//   * score modifiers (FlashAttention-2's softcap and alibi_slopes): x = scale q.k becomes softcap tanh(x / softcap), then
//     x - slope |i + coff - j|, before the visibility rule; the backward multiplies dS by 1 - tanh^2.  Entries of their own
//     (ex_*_score_kernel: the bodies with ExParamsS), so the kernels without a modifier keep their code.
// Exact-f32 math on the f32-input MFMA (any dtype in, head_dim <= 256), the structure of fa_generic.hip: forward by
// query tile with online softmax over the visible keys; backward = delta pre-pass + dK/dV kernel + dQ kernel, no
// atomics.  Rows without any visible key get o = 0, lse = -inf (the reference's softmax of an all -inf row is NaN).
// Dropout is the standard one — O = dropout(softmax(S)) V, the denominator counts every visible key — as in the model's
// dense branch (:85-87); its tiled branch renormalises by the sum of the KEPT probabilities (:155-163), which is a
// different function and is not reproduced.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"

namespace fa {

#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// rows r0 .. r0 + rows - 1 of a (n, d) matrix into an f32 LDS tile, zero-filled past n and d; `vec` (wave-uniform: d % 4 == 0 and
// the tensor aligned for it): four elements per load (16 bytes of f32, 8 bytes of 16-bit elements) and one 16-byte LDS store
// (STRIDED: the rows of src are `ld` elements apart, the token stride of a packed tensor, instead of d)
template <typename T, int DP, int LD, int NTHREADS, bool STRIDED = false>
__device__ __forceinline__ void ex_load_tile(float* __restrict__ dst, const T* __restrict__ src, int r0, int rows, int n,
                                             int d, bool vec, int ld = 0) {
    if (vec) {
        for (int idx = threadIdx.x; idx < rows * (DP / 4); idx += NTHREADS) {
            const int r = idx / (DP / 4), c = 4 * (idx - r * (DP / 4));
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < n && c < d) {
                if constexpr (sizeof(T) == 4) {
                    x = *reinterpret_cast<const f32x4*>(src + (size_t)(r0 + r) * (STRIDED ? ld : d) + c);
                } else {
                    T t[4];
                    *reinterpret_cast<u32x2*>(t) = *reinterpret_cast<const u32x2*>(src + (size_t)(r0 + r) * (STRIDED ? ld : d) + c);
                    x = f32x4{to_f32<T>(t[0]), to_f32<T>(t[1]), to_f32<T>(t[2]), to_f32<T>(t[3])};
                }
            }
            *reinterpret_cast<f32x4*>(dst + r * LD + c) = x;
        }
        return;
    }
    for (int idx = threadIdx.x; idx < rows * DP; idx += NTHREADS) {
        const int r = idx / DP, c = idx - r * DP;
        float x = 0.f;
        if (r0 + r < n && c < d) x = to_f32<T>(src[(size_t)(r0 + r) * (STRIDED ? ld : d) + c]);
        dst[r * LD + c] = x;
    }
}
// The same tile through a block table (ExPage; the paged varlen forward): row r0 + r of the sequence is row t % ps of page
// trow[t / ps] of the pool behind src (page stride `pstride`, token stride `ld`, 64-bit offsets).  A page outside the pool gives
// zeros like a row past n; only the entries of rows < n are read.
template <typename T, int DP, int LD, int NTHREADS>
__device__ __forceinline__ void ex_load_tile_paged(float* __restrict__ dst, const T* __restrict__ src, const ExPage& pg,
                                                   const int* __restrict__ trow, long long pstride, int r0, int rows, int n, int d,
                                                   bool vec, int ld) {
    if (vec) {
        for (int idx = threadIdx.x; idx < rows * (DP / 4); idx += NTHREADS) {
            const int r = idx / (DP / 4), c = 4 * (idx - r * (DP / 4));
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < n && c < d) {
                const int slot = pg_slot(pg, r0 + r), page = trow[slot];
                if ((unsigned)page < (unsigned)pg.num_blocks) {
                    const T* at = src + (size_t)page * (size_t)pstride + (size_t)(r0 + r - slot * pg.ps) * ld + c;
                    if constexpr (sizeof(T) == 4) {
                        x = *reinterpret_cast<const f32x4*>(at);
                    } else {
                        T t[4];
                        *reinterpret_cast<u32x2*>(t) = *reinterpret_cast<const u32x2*>(at);
                        x = f32x4{to_f32<T>(t[0]), to_f32<T>(t[1]), to_f32<T>(t[2]), to_f32<T>(t[3])};
                    }
                }
            }
            *reinterpret_cast<f32x4*>(dst + r * LD + c) = x;
        }
        return;
    }
    for (int idx = threadIdx.x; idx < rows * DP; idx += NTHREADS) {
        const int r = idx / DP, c = idx - r * DP;
        float x = 0.f;
        if (r0 + r < n && c < d) {
            const int slot = pg_slot(pg, r0 + r), page = trow[slot];
            if ((unsigned)page < (unsigned)pg.num_blocks)
                x = to_f32<T>(src[(size_t)page * (size_t)pstride + (size_t)(r0 + r - slot * pg.ps) * ld + c]);
        }
        dst[r * LD + c] = x;
    }
}
// The same from an e4m3 pool (ExKv8; fa_ex_forward_varlen_paged_fp8): src addresses bytes, pstride and ld are bytes, and a byte
// widens exactly to f32 (v_cvt_f32_fp8).  The scales are not applied here: they are two fp32 multiplies in the body.
template <int DP, int LD, int NTHREADS>
__device__ __forceinline__ void ex_load_tile_paged_q8(float* __restrict__ dst, const uint8_t* __restrict__ src, const ExPage& pg,
                                                      const int* __restrict__ trow, long long pstride, int r0, int rows, int n, int d,
                                                      bool vec, int ld) {
    if (vec) {   // (d % 4 == 0, the pool and its strides multiples of 4 bytes: one dword = four elements)
        for (int idx = threadIdx.x; idx < rows * (DP / 4); idx += NTHREADS) {
            const int r = idx / (DP / 4), c = 4 * (idx - r * (DP / 4));
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < n && c < d) {
                const int slot = pg_slot(pg, r0 + r), page = trow[slot];
                if ((unsigned)page < (unsigned)pg.num_blocks) {
                    const int u = *reinterpret_cast<const int*>(src + (size_t)page * (size_t)pstride + (size_t)(r0 + r - slot * pg.ps) * ld + c);
                    x = f32x4{__builtin_amdgcn_cvt_f32_fp8(u, 0), __builtin_amdgcn_cvt_f32_fp8(u, 1), __builtin_amdgcn_cvt_f32_fp8(u, 2),
                              __builtin_amdgcn_cvt_f32_fp8(u, 3)};
                }
            }
            *reinterpret_cast<f32x4*>(dst + r * LD + c) = x;
        }
        return;
    }
    for (int idx = threadIdx.x; idx < rows * DP; idx += NTHREADS) {
        const int r = idx / DP, c = idx - r * DP;
        float x = 0.f;
        if (r0 + r < n && c < d) {
            const int slot = pg_slot(pg, r0 + r), page = trow[slot];
            if ((unsigned)page < (unsigned)pg.num_blocks)
                x = __builtin_amdgcn_cvt_f32_fp8((int)src[(size_t)page * (size_t)pstride + (size_t)(r0 + r - slot * pg.ps) * ld + c], 0);
        }
        dst[r * LD + c] = x;
    }
}
// score modifiers of one element in the exact kernels' domain (ExScore; x = scale q.k, dist = i + coff - j); dt = 1 - t^2, the
// softcap's derivative (1 without one).  The forward and both backward bodies evaluate it with these same operations.
__device__ __forceinline__ float ex_score_mod(const ExScore& sc, float slope, float x, int dist, float& dt) {
    dt = 1.f;
    if (sc.softcap > 0.f) {
        const float t = tanhf(x / sc.softcap);
        dt = fmaf(-t, t, 1.f);
        x = sc.softcap * t;
    }
    if (sc.alibi) x = fmaf(-slope, fabsf((float)dist), x);
    return x;
}
template <typename P> constexpr bool ex_has_score() { return std::is_base_of<ExParamsS, P>::value; }
template <typename P> constexpr bool ex_has_sink() { return std::is_base_of<ExParamsK, P>::value; }
template <typename P> struct ex_is_paged : std::false_type {};
template <typename B> struct ex_is_paged<ExParamsPg<B>> : std::true_type {};
template <typename B> struct ex_is_paged<ExParamsPg8<B>> : std::true_type {};
template <typename P> struct ex_is_kv8 : std::false_type {};   // (paged, from an e4m3 pool)
template <typename B> struct ex_is_kv8<ExParamsPg8<B>> : std::true_type {};

template <typename T> __device__ __forceinline__ bool ex_quad_ok(int d, const void* a, const void* b, const void* c, const void* e) {
    return d % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                           reinterpret_cast<uintptr_t>(e)) % (4 * sizeof(T))) == 0;
}
// Operand reads (as fa_generic.hip, round 2): the contraction index of the 16x16x4 MFMA is permuted so that a lane's operands for
// four consecutive MFMAs are one 16-byte LDS read — lane (lr, lq), step j of super-step S: k = 16 S + 4 lq + j (A and B agree; the
// sum stays an f32 fma chain).  The P / dS staging areas are wave-private: no workgroup barrier between writing and reading them.

// ---- forward: one workgroup = NW waves = 16 NW query rows of one (b,h); key tiles of 32
// VAR: packed sequences (ExParams' varlen fields; the ex_*_varlen_kernel entries): the tile of unit bh = b * hq + h of the padded
// grid, inside sequence b.  q rows at token stride sq (k, v: sk, sv), o / dq / dk / dv rows at hq * d, lse at (h, token), delta at
// (token, h).
// P: ExParams, or ExParamsS for the score-modifier entries (the same for the backward bodies), or ExParamsK for the sink entries
// (forward only: the sink joins the row's normaliser in the epilogue, the key loop does not know it), or ExParamsPg of one of them
// for the paged entries (forward only, VAR: the K/V tiles come through the block table, nothing else differs)
template <typename T, int DP, int NW, bool WIN, bool VAR, typename P>
__device__ __forceinline__ void ex_fwd_body(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ o,
                                            float* __restrict__ lse, P& p) {
    constexpr bool SC = ex_has_score<P>(), SNK = ex_has_sink<P>(), PG = ex_is_paged<P>::value, Q8 = ex_is_kv8<P>::value;
    static_assert(!PG || VAR, "the paged entries are varlen entries");
    constexpr int LD = DP + 4, BM = 16 * NW, BN = 32, NT = DP / 16, PLD = BN + 4, NTH = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ks = Qs + BM * LD;
    float* Vs = Ks + BN * LD;
    float* Ps = Vs + BN * LD;
    const int ntile = (p.nq + BM - 1) / BM;
    const int bh = blockIdx.x / ntile;
    const int q0 = (blockIdx.x - bh * ntile) * BM;
    [[maybe_unused]] int sq0 = 0, sk0 = 0, hh = 0, hk = 0;
    [[maybe_unused]] const int* pg_row = nullptr;   // paged: this sequence's table row
    if constexpr (VAR) {   // packed sequences: narrow the padded call to sequence b (fa_ex_mfma_kernels.h: exm_varlen_unit)
        const int b = bh / p.hq;
        hh = bh - b * p.hq;
        hk = kv_unit(hh, p.kvg);
        int lq, lk;
        seq_span(p.cu_q, b, p.total_q, p.nq, sq0, lq);
        if constexpr (PG) {   // (the keys are no span of a packed tensor: sk0 stays 0)
            lk = paged_len(p.cu_k, b, p.nk);
            pg_row = p.pg.table + (size_t)b * p.pg.max_blocks;
        } else {
            seq_span(p.cu_k, b, p.total_k, p.nk, sk0, lk);
        }
        p.nq = lq; p.nk = lk; p.coff = lk - lq;
        if (q0 >= p.nq) return;
    }
    [[maybe_unused]] float vdsc = 1.0f;
    if constexpr (Q8) {   // the scales of (sequence, K/V head): the score is scale * k_descale * (q . k_stored), before softcap and ALiBi
        p.scale *= kv8_scale(p.q8.kd, p.q8.bs, bh / p.hq, hk);
        vdsc = kv8_scale(p.q8.vd, p.q8.bs, bh / p.hq, hk);
    }
    const size_t qbase = VAR ? (size_t)sq0 * p.sq + (size_t)hh * p.d : (size_t)bh * p.nq * p.d;
    const size_t kbase = VAR ? (size_t)sk0 * p.sk + (size_t)hk * p.d : (size_t)kv_unit(bh, p.kvg) * p.nk * p.d;
    const size_t vbase = VAR ? (size_t)sk0 * p.sv + (size_t)hk * p.d : kbase;
    const size_t obase = VAR ? ((size_t)sq0 * p.hq + hh) * p.d : qbase;
    const size_t ostr = VAR ? (size_t)p.hq * p.d : (size_t)p.d;
    const size_t lbase = VAR ? (size_t)hh * p.total_q + sq0 : (size_t)bh * p.nq;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;

    bool vec = ex_quad_ok<T>(p.d, q, k, v, q) && (!VAR || (p.sq | p.sk | p.sv) % 4 == 0);
    if constexpr (PG) vec = vec && (p.pg.kps | p.pg.vps) % 4 == 0;
    [[maybe_unused]] bool vec8 = false;   // e4m3 pools: dwords of four bytes
    if constexpr (Q8) vec8 = p.d % 4 == 0 && ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) % 4) == 0 &&
                             (p.sk | p.sv) % 4 == 0 && (p.pg.kps | p.pg.vps) % 4 == 0;
    ex_load_tile<T, DP, LD, NTH, VAR>(Qs, q + qbase, q0, BM, p.nq, p.d, vec, VAR ? p.sq : 0);
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; l[i] = 0.f; }
    // keys past the last row's diagonal / band are masked for every row of the tile, and keys before the first row's band
    const int kend = WIN ? max(0, min(p.nk, q0 + BM + p.coff + p.wr)) : (p.causal ? max(0, min(p.nk, q0 + BM + p.coff)) : p.nk);
    const int kstart = WIN ? (max(0, q0 + p.coff - p.wl) / BN) * BN : 0;   // (wr = 0 under the causal mask)
    float* Pw = Ps + w * 16 * PLD;
    [[maybe_unused]] float slope = 0.f;
    if constexpr (SC) slope = ex_slope(p.sc, bh);
    [[maybe_unused]] float snk = -INFINITY;
    if constexpr (SNK) snk = ex_sink(p.snk, bh);

    for (int k0 = kstart; k0 < kend; k0 += BN) {
        if (!VAR && !ex_tile_live(p, q0, min(q0 + BM, p.nq), k0, min(k0 + BN, p.nk))) continue;   // block-sparse skip (uniform)
        __syncthreads();
        if constexpr (Q8) {
            ex_load_tile_paged_q8<DP, LD, NTH>(Ks, reinterpret_cast<const uint8_t*>(k) + kbase, p.pg, pg_row, p.pg.kps, k0, BN, p.nk, p.d, vec8, p.sk);
            ex_load_tile_paged_q8<DP, LD, NTH>(Vs, reinterpret_cast<const uint8_t*>(v) + vbase, p.pg, pg_row, p.pg.vps, k0, BN, p.nk, p.d, vec8, p.sv);
        } else if constexpr (PG) {
            ex_load_tile_paged<T, DP, LD, NTH>(Ks, k + kbase, p.pg, pg_row, p.pg.kps, k0, BN, p.nk, p.d, vec, p.sk);
            ex_load_tile_paged<T, DP, LD, NTH>(Vs, v + vbase, p.pg, pg_row, p.pg.vps, k0, BN, p.nk, p.d, vec, p.sv);
        } else {
            ex_load_tile<T, DP, LD, NTH, VAR>(Ks, k + kbase, k0, BN, p.nk, p.d, vec, VAR ? p.sk : 0);
            ex_load_tile<T, DP, LD, NTH, VAR>(Vs, v + vbase, k0, BN, p.nk, p.d, vec, VAR ? p.sv : 0);
        }
        __syncthreads();
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int S = 0; S < DP / 16; ++S) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(Qs + (w * 16 + lr) * LD + 16 * S + 4 * lq);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(Ks + lr * LD + 16 * S + 4 * lq);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(Ks + (16 + lr) * LD + 16 * S + 4 * lq);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s0 = MFMA_F32(a[j], b0[j], s0);
                s1 = MFMA_F32(a[j], b1[j], s1);
            }
        }
        const int key0 = k0 + lr, key1 = k0 + 16 + lr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = q0 + w * 16 + lq * 4 + i;
            float x0, x1;
            if constexpr (SC) {
                float dt;
                x0 = ex_visible<WIN, VAR>(p, bh, row, key0) ? ex_score_mod(p.sc, slope, s0[i] * p.scale, row + p.coff - key0, dt) : -INFINITY;
                x1 = ex_visible<WIN, VAR>(p, bh, row, key1) ? ex_score_mod(p.sc, slope, s1[i] * p.scale, row + p.coff - key1, dt) : -INFINITY;
            } else {
                x0 = ex_visible<WIN, VAR>(p, bh, row, key0) ? s0[i] * p.scale : -INFINITY;
                x1 = ex_visible<WIN, VAR>(p, bh, row, key1) ? s1[i] * p.scale : -INFINITY;
            }
            float mx = fmaxf(x0, x1);
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
            const float mn = fmaxf(m[i], mx);
            const float msafe = (mn == -INFINITY) ? 0.f : mn;
            const float alpha = expf(m[i] - msafe);
            float p0 = expf(x0 - msafe), p1 = expf(x1 - msafe);
            float rs = p0 + p1;     // the softmax denominator counts every visible key, dropped or not
            rs += __shfl_xor(rs, 1, 64);
            rs += __shfl_xor(rs, 2, 64);
            rs += __shfl_xor(rs, 4, 64);
            rs += __shfl_xor(rs, 8, 64);
            l[i] = l[i] * alpha + rs;
            m[i] = mn;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][i] *= alpha;
            if (p.p_drop > 0.f) {
                p0 = ex_keep(p, bh, row, key0) ? p0 * p.keep_scale : 0.f;
                p1 = ex_keep(p, bh, row, key1) ? p1 * p.keep_scale : 0.f;
            }
            Pw[(lq * 4 + i) * PLD + lr] = p0;
            Pw[(lq * 4 + i) * PLD + 16 + lr] = p1;
        }
#pragma unroll
        for (int S = 0; S < BN / 16; ++S) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(Pw + lr * PLD + 16 * S + 4 * lq);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = MFMA_F32(a[j], Vs[(16 * S + 4 * lq + j) * LD + 16 * t + lr], acc[t]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = q0 + w * 16 + lq * 4 + i;
        if (row < p.nq) {
            float inv = l[i] > 0.f ? 1.f / l[i] : 0.f;   // a row without a visible key: o = 0, lse = -inf
            [[maybe_unused]] float lse_k = 0.f;
            if constexpr (SNK) {   // (a head at -inf keeps the formulas of the call without sinks: the same bits)
                lse_k = l[i] > 0.f ? m[i] + logf(l[i]) : -INFINITY;
                if (snk != -INFINITY) ex_sink_norm(m[i], l[i], snk, inv, lse_k);
            }
            [[maybe_unused]] const float invv = inv * vdsc;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = 16 * t + lr;
                if constexpr (Q8) {   // v_descale joins the normaliser (above): one fp32 product in front of the single rounding
                    if (c < p.d) o[obase + (size_t)row * ostr + c] = from_f32<T>(acc[t][i] * invv);
                } else {
                    if (c < p.d) o[obase + (size_t)row * ostr + c] = from_f32<T>(acc[t][i] * inv);
                }
            }
            if constexpr (SNK) {
                if (lr == 0) lse[lbase + row] = lse_k;
            } else {
                if (lr == 0) lse[lbase + row] = l[i] > 0.f ? m[i] + logf(l[i]) : -INFINITY;
            }
        }
    }
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                         const T* __restrict__ v, T* __restrict__ o,
                                                         float* __restrict__ lse, ExParams p) {
    ex_fwd_body<T, DP, NW, WIN, false>(q, k, v, o, lse, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_fwd_varlen_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                const T* __restrict__ v, T* __restrict__ o,
                                                                float* __restrict__ lse, ExParams p) {
    ex_fwd_body<T, DP, NW, WIN, true>(q, k, v, o, lse, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_fwd_score_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                               const T* __restrict__ v, T* __restrict__ o,
                                                               float* __restrict__ lse, ExParamsS p) {
    ex_fwd_body<T, DP, NW, WIN, false>(q, k, v, o, lse, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_fwd_varlen_score_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                      const T* __restrict__ v, T* __restrict__ o,
                                                                      float* __restrict__ lse, ExParamsS p) {
    ex_fwd_body<T, DP, NW, WIN, true>(q, k, v, o, lse, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_fwd_sink_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                              const T* __restrict__ v, T* __restrict__ o,
                                                              float* __restrict__ lse, ExParamsK p) {
    ex_fwd_body<T, DP, NW, WIN, false>(q, k, v, o, lse, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_fwd_varlen_sink_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                     const T* __restrict__ v, T* __restrict__ o,
                                                                     float* __restrict__ lse, ExParamsK p) {
    ex_fwd_body<T, DP, NW, WIN, true>(q, k, v, o, lse, p);
}
// paged K/V: P = ExParamsPg<ExParams | ExParamsS | ExParamsK>
template <typename T, int DP, int NW, bool WIN, typename P>
__global__ __launch_bounds__(NW * 64) void ex_fwd_varlen_paged_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                      const T* __restrict__ v, T* __restrict__ o,
                                                                      float* __restrict__ lse, P p) {
    ex_fwd_body<T, DP, NW, WIN, true>(q, k, v, o, lse, p);
}

// dlse != null (fa_ex_backward_dlse): the gradient of the row's lse leaves the row constant, delta - dlse, so that the kernels'
// dS = P (dP - delta) becomes P (dP - delta + dlse); a row whose lse is -inf (no visible key) ignores its dlse.  lse and dlse are
// indexed by the row, or (hq > 0: packed sequences, rows in (token, head) order) at [head * total_q + token].
template <typename T>
__global__ __launch_bounds__(256) void ex_delta_kernel(const T* __restrict__ o, const T* __restrict__ dout,
                                                       float* __restrict__ delta, long long rows, int d,
                                                       const float* __restrict__ lse, const float* __restrict__ dlse, long long hq,
                                                       long long total_q) {
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    float s = 0.f;
    if (row < rows)
        for (int c = sub; c < d; c += 16) s += to_f32<T>(o[row * d + c]) * to_f32<T>(dout[row * d + c]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (row < rows && sub == 0) {
        if (dlse) {
            const long long li = hq > 0 ? (row % hq) * total_q + row / hq : row;
            if (lse[li] != -INFINITY) s -= dlse[li];
        }
        delta[row] = s;
    }
}

// ---- backward dK/dV: one workgroup = 16 NW keys resident in LDS; loops over 32-row query tiles
//      dV = P_drop^T dO,  dP = keep/(1-p) * (dO V^T),  dS = P (dP - delta),  dK = scale dS^T Q
template <typename T, int DP, int NW, bool WIN, bool VAR, typename P>
__device__ __forceinline__ void ex_dkdv_body(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                             const T* __restrict__ dout, const float* __restrict__ lse,
                                             const float* __restrict__ delta, T* __restrict__ dk, T* __restrict__ dv, P& p) {
    constexpr bool SC = ex_has_score<P>();
    constexpr int LD = DP + 4, BK = 16 * NW, BQ = 32, NT = DP / 16, PLD = BQ + 4, NTH = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = Ks + BK * LD;
    float* Qs = Vs + BK * LD;
    float* Os = Qs + BQ * LD;
    float* Pt = Os + BQ * LD;
    float* St = Pt + NW * 16 * PLD;
    float* Ls = St + NW * 16 * PLD;
    const int ntile = (p.nk + BK - 1) / BK;
    const int bh = blockIdx.x / ntile;
    const int k0 = (blockIdx.x - bh * ntile) * BK;
    [[maybe_unused]] int sq0 = 0, sk0 = 0, hh = 0, hk = 0;
    if constexpr (VAR) {   // packed sequences: narrow the padded call to sequence b (fa_ex_mfma_kernels.h: exm_varlen_unit)
        const int b = bh / p.hq;
        hh = bh - b * p.hq;
        hk = kv_unit(hh, p.kvg);
        int lq, lk;
        seq_span(p.cu_q, b, p.total_q, p.nq, sq0, lq);
        seq_span(p.cu_k, b, p.total_k, p.nk, sk0, lk);
        p.nq = lq; p.nk = lk; p.coff = lk - lq;
        if (k0 >= p.nk) return;
    }
    const size_t qbase = VAR ? (size_t)sq0 * p.sq + (size_t)hh * p.d : (size_t)bh * p.nq * p.d;
    const size_t kbase = VAR ? (size_t)sk0 * p.sk + (size_t)hk * p.d : (size_t)kv_unit(bh, p.kvg) * p.nk * p.d;
    const size_t vbase = VAR ? (size_t)sk0 * p.sv + (size_t)hk * p.d : kbase;
    const size_t obase = VAR ? ((size_t)sq0 * p.hq + hh) * p.d : qbase;   // dO
    const size_t ostr = VAR ? (size_t)p.hq * p.d : (size_t)p.d;           // rows of dO, dK, dV
    const size_t lbase = VAR ? (size_t)hh * p.total_q + sq0 : (size_t)bh * p.nq;
    const size_t dbase = VAR ? (size_t)sq0 * p.hq + hh : (size_t)bh * p.nq, dstep = VAR ? p.hq : 1;   // delta
    // dK / dV rows: per query head (grouped: the partials kv_group_sum adds up)
    const size_t dkbase = VAR ? ((size_t)sk0 * p.hq + hh) * p.d : (size_t)bh * p.nk * p.d;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;

    const bool vec = ex_quad_ok<T>(p.d, q, k, v, dout) && (!VAR || (p.sq | p.sk | p.sv) % 4 == 0);
    ex_load_tile<T, DP, LD, NTH, VAR>(Ks, k + kbase, k0, BK, p.nk, p.d, vec, VAR ? p.sk : 0);
    ex_load_tile<T, DP, LD, NTH, VAR>(Vs, v + vbase, k0, BK, p.nk, p.d, vec, VAR ? p.sv : 0);
    f32x4 dka[NT], dva[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { dka[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dva[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    float* Pw = Pt + w * 16 * PLD;
    float* Sw = St + w * 16 * PLD;
    [[maybe_unused]] float slope = 0.f;
    if constexpr (SC) slope = ex_slope(p.sc, bh);
    // rows before the tile's first key's diagonal see none of it: key k0 is visible from row k0 - coff - wr on (wr = 0
    // under the causal mask); with a left bound the tile's last key is visible up to row kl - coff + wl
    const int qstart = WIN ? (max(0, k0 - p.coff - p.wr) / BQ) * BQ : (p.causal ? (max(0, k0 - p.coff) / BQ) * BQ : 0);
    const int qend = WIN ? min(p.nq, min(k0 + BK, p.nk) - p.coff + p.wl) : p.nq;
    for (int r0 = qstart; r0 < qend; r0 += BQ) {
        if (!VAR && !ex_tile_live(p, r0, min(r0 + BQ, p.nq), k0, min(k0 + BK, p.nk))) continue;
        __syncthreads();
        ex_load_tile<T, DP, LD, NTH, VAR>(Qs, q + qbase, r0, BQ, p.nq, p.d, vec, VAR ? p.sq : 0);
        ex_load_tile<T, DP, LD, NTH, VAR>(Os, dout + obase, r0, BQ, p.nq, p.d, vec, VAR ? (int)ostr : 0);
        if (threadIdx.x < BQ) {
            const int r = r0 + threadIdx.x;
            Ls[threadIdx.x] = r < p.nq ? lse[lbase + r] : 0.f;
            Ls[BQ + threadIdx.x] = r < p.nq ? delta[dbase + r * dstep] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int S = 0; S < DP / 16; ++S) {
                const f32x4 ak = *reinterpret_cast<const f32x4*>(Ks + (w * 16 + lr) * LD + 16 * S + 4 * lq);
                const f32x4 av = *reinterpret_cast<const f32x4*>(Vs + (w * 16 + lr) * LD + 16 * S + 4 * lq);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(Qs + (qb * 16 + lr) * LD + 16 * S + 4 * lq);
                const f32x4 bo = *reinterpret_cast<const f32x4*>(Os + (qb * 16 + lr) * LD + 16 * S + 4 * lq);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    st = MFMA_F32(ak[j], bq[j], st);
                    dpt = MFMA_F32(av[j], bo[j], dpt);
                }
            }
            const int row = r0 + qb * 16 + lr;   // query index (MFMA column)
            const float lq_ = Ls[qb * 16 + lr], dl_ = Ls[BQ + qb * 16 + lr];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + w * 16 + lq * 4 + i;
                if constexpr (SC) {   // dS = P (dP - delta) (1 - t^2)
                    float dt;
                    const float x = ex_score_mod(p.sc, slope, st[i] * p.scale, row + p.coff - key, dt);
                    const float pr = ex_visible<WIN, VAR>(p, bh, row, key) ? expf(x - lq_) : 0.f;
                    const float ks_ = (p.p_drop > 0.f) ? (ex_keep(p, bh, row, key) ? p.keep_scale : 0.f) : 1.f;
                    Pw[(lq * 4 + i) * PLD + qb * 16 + lr] = pr * ks_;
                    Sw[(lq * 4 + i) * PLD + qb * 16 + lr] = pr * (dpt[i] * ks_ - dl_) * dt;
                } else {
                    const float pr = ex_visible<WIN, VAR>(p, bh, row, key) ? expf(st[i] * p.scale - lq_) : 0.f;
                    const float ks_ = (p.p_drop > 0.f) ? (ex_keep(p, bh, row, key) ? p.keep_scale : 0.f) : 1.f;
                    Pw[(lq * 4 + i) * PLD + qb * 16 + lr] = pr * ks_;                       // P_drop^T (feeds dV)
                    Sw[(lq * 4 + i) * PLD + qb * 16 + lr] = pr * (dpt[i] * ks_ - dl_);      // dS^T
                }
            }
        }
#pragma unroll
        for (int S = 0; S < BQ / 16; ++S) {
            const f32x4 ap = *reinterpret_cast<const f32x4*>(Pw + lr * PLD + 16 * S + 4 * lq);
            const f32x4 as = *reinterpret_cast<const f32x4*>(Sw + lr * PLD + 16 * S + 4 * lq);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dva[t] = MFMA_F32(ap[j], Os[(16 * S + 4 * lq + j) * LD + 16 * t + lr], dva[t]);
                    dka[t] = MFMA_F32(as[j], Qs[(16 * S + 4 * lq + j) * LD + 16 * t + lr], dka[t]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = k0 + w * 16 + lq * 4 + i;
        if (key < p.nk) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = 16 * t + lr;
                if (c < p.d) {
                    dk[dkbase + (size_t)key * ostr + c] = from_f32<T>(dka[t][i] * p.scale);
                    dv[dkbase + (size_t)key * ostr + c] = from_f32<T>(dva[t][i]);
                }
            }
        }
    }
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dkdv_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                          const T* __restrict__ v, const T* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          T* __restrict__ dk, T* __restrict__ dv, ExParams p) {
    ex_dkdv_body<T, DP, NW, WIN, false>(q, k, v, dout, lse, delta, dk, dv, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dkdv_varlen_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                 const T* __restrict__ v, const T* __restrict__ dout,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 T* __restrict__ dk, T* __restrict__ dv, ExParams p) {
    ex_dkdv_body<T, DP, NW, WIN, true>(q, k, v, dout, lse, delta, dk, dv, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dkdv_score_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                const T* __restrict__ v, const T* __restrict__ dout,
                                                                const float* __restrict__ lse, const float* __restrict__ delta,
                                                                T* __restrict__ dk, T* __restrict__ dv, ExParamsS p) {
    ex_dkdv_body<T, DP, NW, WIN, false>(q, k, v, dout, lse, delta, dk, dv, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dkdv_varlen_score_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                       const T* __restrict__ v, const T* __restrict__ dout,
                                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                                       T* __restrict__ dk, T* __restrict__ dv, ExParamsS p) {
    ex_dkdv_body<T, DP, NW, WIN, true>(q, k, v, dout, lse, delta, dk, dv, p);
}

// ---- backward dQ: one workgroup = 16 NW query rows; loops over 32-key tiles (S and dP recomputed: deterministic)
template <typename T, int DP, int NW, bool WIN, bool VAR, typename P>
__device__ __forceinline__ void ex_dq_body(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                           const T* __restrict__ dout, const float* __restrict__ lse,
                                           const float* __restrict__ delta, T* __restrict__ dq, P& p) {
    constexpr bool SC = ex_has_score<P>();
    constexpr int LD = DP + 4, BM = 16 * NW, BN = 32, NT = DP / 16, PLD = BN + 4, NTH = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Os = Qs + BM * LD;
    float* Ks = Os + BM * LD;
    float* Vs = Ks + BN * LD;
    float* Ss = Vs + BN * LD;
    const int ntile = (p.nq + BM - 1) / BM;
    const int bh = blockIdx.x / ntile;
    const int q0 = (blockIdx.x - bh * ntile) * BM;
    [[maybe_unused]] int sq0 = 0, sk0 = 0, hh = 0, hk = 0;
    if constexpr (VAR) {   // packed sequences: narrow the padded call to sequence b (fa_ex_mfma_kernels.h: exm_varlen_unit)
        const int b = bh / p.hq;
        hh = bh - b * p.hq;
        hk = kv_unit(hh, p.kvg);
        int lq, lk;
        seq_span(p.cu_q, b, p.total_q, p.nq, sq0, lq);
        seq_span(p.cu_k, b, p.total_k, p.nk, sk0, lk);
        p.nq = lq; p.nk = lk; p.coff = lk - lq;
        if (q0 >= p.nq) return;
    }
    const size_t qbase = VAR ? (size_t)sq0 * p.sq + (size_t)hh * p.d : (size_t)bh * p.nq * p.d;
    const size_t kbase = VAR ? (size_t)sk0 * p.sk + (size_t)hk * p.d : (size_t)kv_unit(bh, p.kvg) * p.nk * p.d;
    const size_t vbase = VAR ? (size_t)sk0 * p.sv + (size_t)hk * p.d : kbase;
    const size_t obase = VAR ? ((size_t)sq0 * p.hq + hh) * p.d : qbase;   // dO, dQ
    const size_t ostr = VAR ? (size_t)p.hq * p.d : (size_t)p.d;
    const size_t lbase = VAR ? (size_t)hh * p.total_q + sq0 : (size_t)bh * p.nq;
    const size_t dbase = VAR ? (size_t)sq0 * p.hq + hh : (size_t)bh * p.nq, dstep = VAR ? p.hq : 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;

    const bool vec = ex_quad_ok<T>(p.d, q, k, v, dout) && (!VAR || (p.sq | p.sk | p.sv) % 4 == 0);
    ex_load_tile<T, DP, LD, NTH, VAR>(Qs, q + qbase, q0, BM, p.nq, p.d, vec, VAR ? p.sq : 0);
    ex_load_tile<T, DP, LD, NTH, VAR>(Os, dout + obase, q0, BM, p.nq, p.d, vec, VAR ? (int)ostr : 0);
    float lrow[4], drow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = q0 + w * 16 + lq * 4 + i;
        lrow[i] = row < p.nq ? lse[lbase + row] : 0.f;
        drow[i] = row < p.nq ? delta[dbase + row * dstep] : 0.f;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* Sw = Ss + w * 16 * PLD;
    [[maybe_unused]] float slope = 0.f;
    if constexpr (SC) slope = ex_slope(p.sc, bh);
    const int kend = WIN ? max(0, min(p.nk, q0 + BM + p.coff + p.wr)) : (p.causal ? max(0, min(p.nk, q0 + BM + p.coff)) : p.nk);
    const int kstart = WIN ? (max(0, q0 + p.coff - p.wl) / BN) * BN : 0;   // (the forward kernel's tile range)
    for (int k0 = kstart; k0 < kend; k0 += BN) {
        if (!VAR && !ex_tile_live(p, q0, min(q0 + BM, p.nq), k0, min(k0 + BN, p.nk))) continue;
        __syncthreads();
        ex_load_tile<T, DP, LD, NTH, VAR>(Ks, k + kbase, k0, BN, p.nk, p.d, vec, VAR ? p.sk : 0);
        ex_load_tile<T, DP, LD, NTH, VAR>(Vs, v + vbase, k0, BN, p.nk, p.d, vec, VAR ? p.sv : 0);
        __syncthreads();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int S = 0; S < DP / 16; ++S) {
                const f32x4 aq = *reinterpret_cast<const f32x4*>(Qs + (w * 16 + lr) * LD + 16 * S + 4 * lq);
                const f32x4 ao = *reinterpret_cast<const f32x4*>(Os + (w * 16 + lr) * LD + 16 * S + 4 * lq);
                const f32x4 bk = *reinterpret_cast<const f32x4*>(Ks + (nb * 16 + lr) * LD + 16 * S + 4 * lq);
                const f32x4 bv = *reinterpret_cast<const f32x4*>(Vs + (nb * 16 + lr) * LD + 16 * S + 4 * lq);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s = MFMA_F32(aq[j], bk[j], s);
                    dp = MFMA_F32(ao[j], bv[j], dp);
                }
            }
            const int key = k0 + nb * 16 + lr;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = q0 + w * 16 + lq * 4 + i;
                if constexpr (SC) {
                    float dt;
                    const float x = ex_score_mod(p.sc, slope, s[i] * p.scale, row + p.coff - key, dt);
                    const float pr = ex_visible<WIN, VAR>(p, bh, row, key) ? expf(x - lrow[i]) : 0.f;
                    const float ks_ = (p.p_drop > 0.f) ? (ex_keep(p, bh, row, key) ? p.keep_scale : 0.f) : 1.f;
                    Sw[(lq * 4 + i) * PLD + nb * 16 + lr] = pr * (dp[i] * ks_ - drow[i]) * dt;
                } else {
                    const float pr = ex_visible<WIN, VAR>(p, bh, row, key) ? expf(s[i] * p.scale - lrow[i]) : 0.f;
                    const float ks_ = (p.p_drop > 0.f) ? (ex_keep(p, bh, row, key) ? p.keep_scale : 0.f) : 1.f;
                    Sw[(lq * 4 + i) * PLD + nb * 16 + lr] = pr * (dp[i] * ks_ - drow[i]);
                }
            }
        }
#pragma unroll
        for (int S = 0; S < BN / 16; ++S) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(Sw + lr * PLD + 16 * S + 4 * lq);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = MFMA_F32(a[j], Ks[(16 * S + 4 * lq + j) * LD + 16 * t + lr], acc[t]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = q0 + w * 16 + lq * 4 + i;
        if (row < p.nq) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = 16 * t + lr;
                if (c < p.d) dq[obase + (size_t)row * ostr + c] = from_f32<T>(acc[t][i] * p.scale);
            }
        }
    }
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dq_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                        const T* __restrict__ v, const T* __restrict__ dout,
                                                        const float* __restrict__ lse, const float* __restrict__ delta,
                                                        T* __restrict__ dq, ExParams p) {
    ex_dq_body<T, DP, NW, WIN, false>(q, k, v, dout, lse, delta, dq, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dq_varlen_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                               const T* __restrict__ v, const T* __restrict__ dout,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               T* __restrict__ dq, ExParams p) {
    ex_dq_body<T, DP, NW, WIN, true>(q, k, v, dout, lse, delta, dq, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dq_score_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                              const T* __restrict__ v, const T* __restrict__ dout,
                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                              T* __restrict__ dq, ExParamsS p) {
    ex_dq_body<T, DP, NW, WIN, false>(q, k, v, dout, lse, delta, dq, p);
}
template <typename T, int DP, int NW, bool WIN>
__global__ __launch_bounds__(NW * 64) void ex_dq_varlen_score_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                     const T* __restrict__ v, const T* __restrict__ dout,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                                     T* __restrict__ dq, ExParamsS p) {
    ex_dq_body<T, DP, NW, WIN, true>(q, k, v, dout, lse, delta, dq, p);
}

// ---- the sink's gradient: dsinks[h] = -sum over the rows of head h of exp(sink_h - lse) delta, delta = rowsum(dO * O) as the
// backward's pre-pass left it in the workspace (dsign = -1 where that holds -delta).  One workgroup per head and a fixed order:
// thread t adds its rows t, t + 1024, .. of segment after segment (a segment = the nq rows of one unit of the head, or the rows
// of one packed sequence under one query head: only rows some sequence covers have an lse), then the wave adds by shuffles, then wave 0 adds the 16
// wave sums from LDS.  No atomics: the same bits on every run.  exp(sink - lse) <= 1 because lse contains the sink.
struct DsinkParams {
    const int* cu_q;               // varlen: the sequences' token offsets (untrusted); null otherwise
    long long l_hstride, d_hstride, d_tstride;   // varlen: lse[h * l_hstride + t], delta[h * d_hstride + t * d_tstride]
    int nseg, nq, heads, total_q, hq;   // segments per head (units / heads, or the batch); rows per unit (varlen: max_seqlen_q)
    float dsign;
};
__global__ __launch_bounds__(1024) void ex_dsink_kernel(const float* __restrict__ lse, const float* __restrict__ delta,
                                                         const float* __restrict__ sinks, float* __restrict__ dsinks, DsinkParams p) {
    __shared__ float part[16];
    const int h = blockIdx.x;
    const float snk = sinks[h];
    if (snk == -INFINITY) {   // no sink for this head: gradient 0 (uniform over the workgroup)
        if (threadIdx.x == 0) dsinks[h] = 0.f;
        return;
    }
    float acc = 0.f;
    if (p.cu_q) {   // packed sequences: the query heads h, h + heads, .. share the sink; sequence after sequence
        for (int hh = h; hh < p.hq; hh += p.heads)
            for (int b = 0; b < p.nseg; ++b) {
                int start, len;
                seq_span(p.cu_q, b, p.total_q, p.nq, start, len);
                const long long lb = (long long)hh * p.l_hstride + start;
                const long long db = (long long)hh * p.d_hstride + (long long)start * p.d_tstride;
                for (int i = threadIdx.x; i < len; i += 1024) acc += expf(snk - lse[lb + i]) * delta[db + i * p.d_tstride];
            }
    } else {
        for (int sgm = 0; sgm < p.nseg; ++sgm) {   // units h, h + heads, ..
            const long long base = ((long long)sgm * p.heads + h) * p.nq;
            for (int i = threadIdx.x; i < p.nq; i += 1024) acc += expf(snk - lse[base + i]) * delta[base + i];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        float t = threadIdx.x < 16 ? part[threadIdx.x] : 0.f;
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
        if (threadIdx.x == 0) dsinks[h] = -p.dsign * t;
    }
}
hipError_t launch_ex_dsink(const ExArgs& a, const float* delta, long long d_hstride, long long d_tstride, float dsign, hipStream_t st) {
    DsinkParams p;
    p.cu_q = a.cu_q;
    p.l_hstride = a.total_q; p.d_hstride = d_hstride; p.d_tstride = d_tstride;
    p.heads = (int)a.sink_heads;
    p.nseg = a.cu_q ? (int)(a.bh / a.heads_q) : (int)(a.bh / a.sink_heads);
    p.nq = (int)a.nq; p.total_q = (int)a.total_q; p.hq = (int)a.heads_q;
    p.dsign = dsign;
    hipLaunchKernelGGL(ex_dsink_kernel, dim3((unsigned)a.sink_heads), dim3(1024), 0, st, (const float*)a.lse, delta, a.sinks, a.dsinks, p);
    return hipGetLastError();
}
// the lse of a sink call's rows when no sequence has a key: the sink itself
__global__ __launch_bounds__(256) void ex_sink_fill_kernel(float* __restrict__ lse, const float* __restrict__ sinks, int heads, long long nq,
                                                           long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) lse[i] = sinks[(i / nq) % heads];
}
hipError_t launch_ex_sink_fill(float* lse, const float* sinks, int64_t sink_heads, int64_t units, int64_t nq, hipStream_t st) {
    const long long total = (long long)units * nq;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(ex_sink_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, lse, sinks, (int)sink_heads,
                       (long long)nq, total);
    return hipGetLastError();
}

// ---- host launchers
// SC: a call with a score modifier (the *_score_kernel entries, ExParamsS); SK: a forward with sinks (the *_sink_kernel entries,
// ExParamsK; always with SC)
template <typename T, int DP, int NW, bool WIN, bool VAR, bool SC, bool SK = false> static auto ex_fwd_entry() {
    if constexpr (SK) return VAR ? ex_fwd_varlen_sink_kernel<T, DP, NW, WIN> : ex_fwd_sink_kernel<T, DP, NW, WIN>;
    else if constexpr (SC) return VAR ? ex_fwd_varlen_score_kernel<T, DP, NW, WIN> : ex_fwd_score_kernel<T, DP, NW, WIN>;
    else return VAR ? ex_fwd_varlen_kernel<T, DP, NW, WIN> : ex_fwd_kernel<T, DP, NW, WIN>;
}
template <typename T, int DP, int NW, bool WIN, bool VAR, bool SC> static auto ex_dkdv_entry() {
    if constexpr (SC) return VAR ? ex_dkdv_varlen_score_kernel<T, DP, NW, WIN> : ex_dkdv_score_kernel<T, DP, NW, WIN>;
    else return VAR ? ex_dkdv_varlen_kernel<T, DP, NW, WIN> : ex_dkdv_kernel<T, DP, NW, WIN>;
}
template <typename T, int DP, int NW, bool WIN, bool VAR, bool SC> static auto ex_dq_entry() {
    if constexpr (SC) return VAR ? ex_dq_varlen_score_kernel<T, DP, NW, WIN> : ex_dq_score_kernel<T, DP, NW, WIN>;
    else return VAR ? ex_dq_varlen_kernel<T, DP, NW, WIN> : ex_dq_kernel<T, DP, NW, WIN>;
}
template <bool SC, bool SK = false> static auto ex_params(const ExArgs& a) {
    if constexpr (SK) return make_ex_params_k(a);
    else if constexpr (SC) return make_ex_params_s(a);
    else return make_ex_params(a);
}

template <typename T, int DP, int NW, bool WIN, bool VAR = false, bool SC = false, bool SK = false>
static hipError_t ex_fwd_t(const ExArgs& a, hipStream_t st) {
    constexpr int LD = DP + 4;
    const size_t smem = sizeof(float) * ((16 * NW + 64) * LD + NW * 16 * 36);
    auto kern = ex_fwd_entry<T, DP, NW, WIN, VAR, SC, SK>();
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((a.nq + 16 * NW - 1) / (16 * NW)) * a.bh));
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), smem, st, (const T*)a.q, (const T*)a.k, (const T*)a.v, (T*)a.o, a.lse,
                       ex_params<SC, SK>(a));
    return hipGetLastError();
}

template <typename T, int DP, int NW, bool WIN, bool VAR = false, bool SC = false>
static hipError_t ex_bwd_t(const ExArgs& a, hipStream_t st) {
    constexpr int LD = DP + 4;
    float* delta = reinterpret_cast<float*>(a.workspace);
    const long long rows = VAR ? (long long)a.total_q * a.heads_q : (long long)a.bh * a.nq;   // (varlen: (token, head) order)
    const auto p = ex_params<SC>(a);
    ProfScope ps(K_EX_BWD, st);
    hipLaunchKernelGGL(ex_delta_kernel<T>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, (const T*)a.o,
                       (const T*)a.dout, delta, rows, (int)a.d, (const float*)a.lse, a.dlse, VAR ? (long long)a.heads_q : 0LL,
                       (long long)a.total_q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.sinks) {   // (delta rows: (unit, row), varlen (token, head))
        e = launch_ex_dsink(a, delta, 1, a.heads_q, 1.f, st);
        if (e != hipSuccess) return e;
    }
    {
        const size_t smem = sizeof(float) * ((2 * 16 * NW + 64) * LD + 2 * NW * 16 * 36 + 64);
        auto kern = ex_dkdv_entry<T, DP, NW, WIN, VAR, SC>();
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e != hipSuccess) return e;
        dim3 grid((unsigned)(((a.nk + 16 * NW - 1) / (16 * NW)) * a.bh));
        hipLaunchKernelGGL(kern, grid, dim3(NW * 64), smem, st, (const T*)a.q, (const T*)a.k, (const T*)a.v, (const T*)a.dout,
                           (const float*)a.lse, (const float*)delta, (T*)a.dk, (T*)a.dv, p);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    {
        const size_t smem = sizeof(float) * ((2 * 16 * NW + 64) * LD + NW * 16 * 36);
        auto kern = ex_dq_entry<T, DP, NW, WIN, VAR, SC>();
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e != hipSuccess) return e;
        dim3 grid((unsigned)(((a.nq + 16 * NW - 1) / (16 * NW)) * a.bh));
        hipLaunchKernelGGL(kern, grid, dim3(NW * 64), smem, st, (const T*)a.q, (const T*)a.k, (const T*)a.v, (const T*)a.dout,
                           (const float*)a.lse, (const float*)delta, (T*)a.dq, p);
        e = hipGetLastError();
    }
    return e;
}

// (SK: the forward's sink entries; the backward of a sink call runs the kernels of the call without sinks, on the lse that contains
// the sink, and ex_dsink_kernel beside them)
template <typename T, bool WIN, bool VAR = false, bool SC = false, bool SK = false>
static hipError_t ex_by_d(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.d <= 64) return backward ? ex_bwd_t<T, 64, 4, WIN, VAR, SC>(a, st) : ex_fwd_t<T, 64, 4, WIN, VAR, SC, SK>(a, st);
    if (a.d <= 128) return backward ? ex_bwd_t<T, 128, 4, WIN, VAR, SC>(a, st) : ex_fwd_t<T, 128, 4, WIN, VAR, SC, SK>(a, st);
    return backward ? ex_bwd_t<T, 256, 2, WIN, VAR, SC>(a, st) : ex_fwd_t<T, 256, 4, WIN, VAR, SC, SK>(a, st);
}
template <typename T, bool SC, bool SK = false>
static hipError_t ex_by_d_s(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.cu_q) return ex_windowed(a) ? ex_by_d<T, true, true, SC, SK>(a, backward, st) : ex_by_d<T, false, true, SC, SK>(a, backward, st);
    return ex_windowed(a) ? ex_by_d<T, true, false, SC, SK>(a, backward, st) : ex_by_d<T, false, false, SC, SK>(a, backward, st);
}
template <typename T>
static hipError_t ex_by_d(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.sinks && !backward) return ex_by_d_s<T, true, true>(a, false, st);
    return ex_scoremod(a) ? ex_by_d_s<T, true>(a, backward, st) : ex_by_d_s<T, false>(a, backward, st);
}

// Grouped-query attention (a.kv_group > 1) reaches every family below except the plain path's exact-f32 kernels (fa_generic.hip):
// those calls take this file's kernels.  The K/V unit enters the kernels' K/V addresses only; a backward writes per-query-head
// dK / dV partials that launch_ex adds up.
static hipError_t launch_ex_one(const ExArgs& a, bool backward, hipStream_t st) {
    const int path = option(OPT_EX_PATH);   // 0: MFMA kernels where they apply, 1: always these, 2: MFMA or fail, 3: MFMA, never the plain kernels
    // an additive bias: kernels of their own, or nothing (the C layer has refused by name what they do not take) — never the plain
    // kernels, the dS hand-over or the exact-f32 kernels, which know no bias
    if (a.bias) return ex_mfma_bias_supported(a) ? launch_ex_mfma_bias(a, backward, st) : hipErrorInvalidConfiguration;
    // no extras at all on a square problem: this IS the plain path — hand it to the tuned kernels (same results contract;
    // the workspace of fa_ex_backward_workspace_bytes covers their row constants)
    // (a window that bounds something never leaves this file's families: the plain, nq != nk and fa_generic kernels know no band)
    // (nor does a score modifier: the plain, Nq != Nk and fa_generic kernels and the dS hand-over know none)
    // (nor do sinks)
    // (nor does a gradient of lse: the plain kernels make their row constants inside the matrix kernels or hand dS over; a call with
    // dlse takes the recomputing kernels, whose pre-pass is a launch of its own — DESIGN.md 9p)
    const bool win = ex_windowed(a), mod = ex_scoremod(a) || a.sinks != nullptr || a.dlse != nullptr;
    const bool plain = (path == 0 || path == 2) && !win && !mod && !a.mask && !a.block_mask && a.dropout_p <= 0.0 && a.scale > 0.f;
    if (plain && a.nq == a.nk && (backward ? bwd_mfma_supported(a.dtype, a.d) : fwd_mfma_supported(a.dtype, a.d))) {
        if (!backward) {
            FwdArgs f{a.q, a.k, a.v, a.o, a.lse, a.bh, a.nq, a.d, a.dtype, a.causal, a.scale};
            f.kv_group = a.kv_group;
            return launch_fwd_mfma(f, st);
        }
        // (with a workspace of fa_ex_backward_workspace_bytes_fast the plain backward hands dS over as it does behind fa2_backward)
        BwdArgs b{a.q, a.k, a.v, a.o, a.dout, a.lse, a.dq, a.dk, a.dv, a.bh, a.nq, a.d, a.dtype, a.causal, a.scale,
                  a.workspace, a.workspace_bytes > ex_backward_workspace_bytes(a.bh, a.nq) ? a.workspace_bytes : ex_backward_workspace_bytes(a.bh, a.nq), 0};
        b.kv_group = a.kv_group;
        return launch_bwd_mfma(b, st);
    }
    // the same for what the 16-bit kernels do not take (fp32 tensors, head dims that are not a multiple of 8): the plain path's
    // exact-f32 kernels (fa_generic.hip: register fragments, 16-byte operand reads — 2.5 x the rate of the kernels below)
    if ((path == 0) && a.kv_group == 1 && !win && !mod && !a.mask && !a.block_mask && a.dropout_p <= 0.0 && a.nq == a.nk && a.d <= 256 &&
        !(backward ? bwd_mfma_supported(a.dtype, a.d) : fwd_mfma_supported(a.dtype, a.d))) {
        if (!backward) return launch_fwd_generic(FwdArgs{a.q, a.k, a.v, a.o, a.lse, a.bh, a.nq, a.d, a.dtype, a.causal, a.scale}, st);
        return launch_bwd_generic(BwdArgs{a.q, a.k, a.v, a.o, a.dout, a.lse, a.dq, a.dk, a.dv, a.bh, a.nq, a.d, a.dtype, a.causal, a.scale,
                                          a.workspace, ex_backward_workspace_bytes(a.bh, a.nq), 0}, st);
    }
    // Nq != Nk without masks or dropout (cross attention; a cached prefix under the causal mask): the d = 128 kernels of the plain
    // path take separate row counts.  Under the causal mask only with Nk >= Nq: they assume that every query row sees key 0.
    if (plain && a.nq != a.nk && nqnk_mfma_supported(a.dtype, a.d, a.bh, a.nq, a.nk, a.causal)) {
        if (!backward) {
            FwdArgs f{a.q, a.k, a.v, a.o, a.lse, a.bh, a.nq, a.d, a.dtype, a.causal, a.scale};
            f.nk = a.nk;
            f.kv_group = a.kv_group;
            return launch_fwd_nqnk(f, st);
        }
        BwdArgs b{a.q, a.k, a.v, a.o, a.dout, a.lse, a.dq, a.dk, a.dv, a.bh, a.nq, a.d, a.dtype, a.causal, a.scale, a.workspace,
                  ex_backward_workspace_bytes(a.bh, a.nq), 0};
        b.nk = a.nk;
        b.kv_group = a.kv_group;
        float* nlse = reinterpret_cast<float*>(a.workspace);
        float* ndelta = nlse + (size_t)a.bh * a.nq;
        // with room for the dS tiles behind the row constants the dK/dV kernel hands dS to the dQ product kernel,
        // as the square backward does and by its rule — since round 3 also under the (shifted) causal diagonal
        const size_t base = (ex_backward_workspace_bytes(a.bh, a.nq) + 255) & ~(size_t)255;
        const size_t extra = bwd_ds_extra_bytes(a.bh, a.nq, a.d, a.dtype, a.causal != 0, false, a.nk, a.kv_group);
        if (extra && a.workspace_bytes >= base + extra)
            return launch_bwd_handover(b, nlse, ndelta, reinterpret_cast<char*>(a.workspace) + base, st);
        hipError_t e = launch_bwd_dq_w4(b, nlse, ndelta, st);   // makes the row constants on its way
        if (e != hipSuccess) return e;
        return launch_bwd_dkdv_w4(b, nlse, ndelta, st);
    }
    if (path != 1 && ex_mfma_supported(a)) return launch_ex_mfma(a, backward, st);
    if (path >= 2) return hipErrorInvalidConfiguration;
    switch (a.dtype) {
        case 0: return ex_by_d<float>(a, backward, st);
        case 1: return ex_by_d<__half>(a, backward, st);
        default: return ex_by_d<__hip_bfloat16>(a, backward, st);
    }
}

// The paged varlen forward (a.block_table != null) on the exact kernels (Q8: from an e4m3 pool, a.kv_e4m3)
template <typename T, int DP, bool WIN, bool SC, bool SK, bool Q8 = false>
static hipError_t ex_paged_fwd_t(const ExArgs& a, hipStream_t st) {
    constexpr int NW = 4, LD = DP + 4;
    using B = decltype(ex_params<SC, SK>(a));
    typename std::conditional<Q8, ExParamsPg8<B>, ExParamsPg<B>>::type p;
    static_cast<B&>(p) = ex_params<SC, SK>(a);
    p.pg = make_ex_page(a);
    if constexpr (Q8) p.q8 = make_ex_kv8(a);
    const size_t smem = sizeof(float) * ((16 * NW + 64) * LD + NW * 16 * 36);
    auto kern = ex_fwd_varlen_paged_kernel<T, DP, NW, WIN, decltype(p)>;
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(((a.nq + 16 * NW - 1) / (16 * NW)) * a.bh));
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), smem, st, (const T*)a.q, (const T*)a.k, (const T*)a.v, (T*)a.o, a.lse, p);
    return hipGetLastError();
}
template <typename T, bool WIN, bool SC, bool SK>
static hipError_t ex_paged_by_d(const ExArgs& a, hipStream_t st) {
    if (a.kv_e4m3) {
        if constexpr (sizeof(T) == 2) {
            if (a.d <= 64) return ex_paged_fwd_t<T, 64, WIN, SC, SK, true>(a, st);
            if (a.d <= 128) return ex_paged_fwd_t<T, 128, WIN, SC, SK, true>(a, st);
            return ex_paged_fwd_t<T, 256, WIN, SC, SK, true>(a, st);
        } else {
            return hipErrorInvalidValue;   // (the C layer takes an e4m3 pool with f16 / bf16 queries only)
        }
    }
    if (a.d <= 64) return ex_paged_fwd_t<T, 64, WIN, SC, SK>(a, st);
    if (a.d <= 128) return ex_paged_fwd_t<T, 128, WIN, SC, SK>(a, st);
    return ex_paged_fwd_t<T, 256, WIN, SC, SK>(a, st);
}
template <typename T>
static hipError_t ex_paged(const ExArgs& a, hipStream_t st) {
    const bool win = ex_windowed(a);
    if (a.sinks) return win ? ex_paged_by_d<T, true, true, true>(a, st) : ex_paged_by_d<T, false, true, true>(a, st);
    if (ex_scoremod(a)) return win ? ex_paged_by_d<T, true, true, false>(a, st) : ex_paged_by_d<T, false, true, false>(a, st);
    return win ? ex_paged_by_d<T, true, false, false>(a, st) : ex_paged_by_d<T, false, false, false>(a, st);
}
static hipError_t launch_ex_varlen_paged(const ExArgs& a, hipStream_t st) {
    const int path = option(OPT_EX_PATH);
    if (a.kv_e4m3) {
        if (path != 1 && ex_mfma_paged_kv8_supported(a)) return launch_ex_mfma_varlen_paged_kv8(a, st);
    } else if (path != 1 && ex_mfma_paged_supported(a)) {
        return launch_ex_mfma_varlen_paged(a, st);
    }
    if (path >= 2) return hipErrorInvalidConfiguration;
    switch (a.dtype) {
        case 0: return ex_paged<float>(a, st);
        case 1: return ex_paged<__half>(a, st);
        default: return ex_paged<__hip_bfloat16>(a, st);
    }
}

// Packed sequences (a.cu_q != null; the C layer has handled the calls with an empty side): the extended kernels only — 16-bit MFMA
// where they take the call, exact f32 otherwise (option ex_path as for the other calls: 1 = exact f32, 2 / 3 = MFMA or fail).
static hipError_t launch_ex_varlen_one(const ExArgs& a, bool backward, hipStream_t st) {
    const int path = option(OPT_EX_PATH);
    if (path != 1 && ex_mfma_varlen_supported(a)) return launch_ex_mfma_varlen(a, backward, st);
    if (path >= 2) return hipErrorInvalidConfiguration;
    switch (a.dtype) {
        case 0: return ex_by_d<float>(a, backward, st);
        case 1: return ex_by_d<__half>(a, backward, st);
        default: return ex_by_d<__hip_bfloat16>(a, backward, st);
    }
}

hipError_t launch_ex(const ExArgs& a, bool backward, hipStream_t st) {
    // V narrower than Q / K: kernels of their own, or nothing (the C layer has refused by name what they do not take)
    if (a.d_v != 0) return ex_vdim_supported(a) ? launch_ex_vdim(a, backward, st) : hipErrorInvalidConfiguration;
    if (a.cu_q) {
        if (a.block_table) return backward ? hipErrorInvalidValue : launch_ex_varlen_paged(a, st);   // (forward only)
        if (!backward || a.kv_group <= 1) return launch_ex_varlen_one(a, backward, st);
        // grouped: per-query-head partials (total_k, heads_q, d) in front of the row constants, then the group sum over units of
        // d elements — unit t * heads_kv + j adds partial rows t * heads_q + j * g + m, m = 0 .. g-1, in that order
        const size_t slab = kv_partial_bytes(a.total_k * a.heads_q, 1, a.d, a.dtype);
        if (a.workspace_bytes < 2 * slab) return hipErrorInvalidValue;
        ExArgs g = a;
        g.dk = a.workspace;
        g.dv = reinterpret_cast<char*>(a.workspace) + slab;
        g.workspace = reinterpret_cast<char*>(a.workspace) + 2 * slab;
        g.workspace_bytes = a.workspace_bytes - 2 * slab;
        hipError_t e = launch_ex_varlen_one(g, true, st);
        if (e != hipSuccess) return e;
        return launch_kv_group_sum(g.dk, g.dv, a.dk, a.dv, a.total_k * (a.heads_q / a.kv_group), a.kv_group, 1, a.d, a.dtype, st);
    }
    if (!backward || a.kv_group <= 1) return launch_ex_one(a, backward, st);
    // Grouped backward.  Workspace: [dK partials][dV partials][what the ungrouped call of bh query units takes]; the kernels write
    // one dK / dV unit per query head into the partials (their indexing and launch geometry as ungrouped), then the group sum.
    const size_t slab = kv_partial_bytes(a.bh, a.nk, a.d, a.dtype);
    if (a.workspace_bytes < 2 * slab) return hipErrorInvalidValue;
    ExArgs g = a;
    g.dk = a.workspace;
    g.dv = reinterpret_cast<char*>(a.workspace) + slab;
    g.workspace = reinterpret_cast<char*>(a.workspace) + 2 * slab;
    g.workspace_bytes = a.workspace_bytes - 2 * slab;
    hipError_t e = launch_ex_one(g, true, st);
    if (e != hipSuccess) return e;
    return launch_kv_group_sum(g.dk, g.dv, a.dk, a.dv, a.bh / a.kv_group, a.kv_group, a.nk, a.d, a.dtype, st);
}
// [-lse/scale | -delta] for the MFMA kernels (the exact kernels keep delta alone in the first half)
size_t ex_backward_workspace_bytes(int64_t bh, int64_t nq) { return sizeof(float) * 2 * (((size_t)bh * (size_t)nq + 63) & ~(size_t)63) + 256; }

}  // namespace fa
