// FlashAttention-3's fp8 call for gfx950: q, k, v arrive ALREADY in OCP e4m3 (float8_e4m3fn) with one float32 descale per (batch,
// K/V head) for each of them, and both products run on v_mfma_scale_f32_32x32x64_f8f6f4 with unit hardware scales.  Forward only,
// head_dim 128, o in f16 / bf16, lse float32.  (include/fa_mi355x.h: fa_fp8_forward)
//
//     o = softmax(softmax_scale * q_descale * k_descale * q8 k8^T [causal, bottom-right aligned]) (v8 * v_descale)
//
// Two launches:
//   fp8in_vt_kernel     V -> V^T in the image fwd_fp8v_kernel (fa_fwd_fp8.hip) reads: [K/V unit][128-key tile][d row][128 key bytes],
//                       every 64-key group in fp8_quant_v_kernel's key permutation (byte 32 hi + 16 h + jj of a group is key
//                       32 hi + 4 h + (jj & 3) + 8 (jj >> 2)), zeros for keys >= Nk including the second half of an odd last tile.  A
//                       byte permutation through LDS: no arithmetic, no scales.  It reads v at the caller's strides and writes the
//                       caller's workspace.
//   fwd_fp8in_kernel    fwd_fp8v_kernel's structure (512 threads, 256 query rows a workgroup, 128-key tiles, double-buffered LDS-DMA
//                       of K8 and V8^T) with: separate nq / nk and the causal diagonal shifted by nk - nq in the tile bound, the
//                       per-wave bound and the mask; the K/V unit from the GQA rule (query head h reads K/V head h / (H_q / H_kv));
//                       ONE score factor per workgroup, f = softmax_scale * log2(e) * q_descale * k_descale, instead of per-block
//                       scale loads; v_descale applied once in the epilogue together with 1 / l; a guard for rows without a visible
//                       key (o = 0, lse = -inf, where 1 / l would give NaN); q, k and o at the caller's strides.
//
// Arithmetic, in the order tests/fp8_inputs_ref.py (baseline) transcribes it:
//   * raw scores: two 64-term instructions over the 128 head-dim bytes, f32 accumulation;
//   * row maxima on the raw products, times f once (f > 0); p = exp2(fma(s, f, -m)) with the lazy rescale (the running max moves
//     only on a tile where some row of the wave's 32 grew by more than 8 in log2 units);
//   * P rounded to e4m3 (RNE) on EVERY row; l and lse from the unrounded p;
//   * o = RNE(acc * (v_descale * (1 / l))), lse = (m + log2 l) * ln 2.
// There is NO 16-bit-P route for short rows.  fa3_forward(fp8 = 1) keeps one (fa_fwd_fp8.hip, launch_fp8_t) because its backward takes
// delta from o; this call has no backward, and FlashAttention-3 rounds P everywhere.  The cost: 2^-4 relative per probability, which
// averages out over a row's keys but stands in full on a row that sees a couple of keys (up to 6 % of |v| on a row that sees two).
//
// Bytes outside [0, Nk) of a view never reach a result: K rows >= Nk are cut off by the buffer descriptor's range check (they
// arrive as zeros), their scores are masked to -inf, and the transposer writes zeros for them; likewise q rows >= Nq.  So the
// [:, :Nk] prefix of a cache with a larger capacity can be passed as it is, whatever the rest holds (e4m3 NaN bytes included).
// NaN codes inside the view propagate.
//
// Span limit: q and k are addressed through 32-bit buffer descriptors and 32-bit offsets per (batch, head) unit, so
// round_up(rows, 256) * token_stride_bytes must stay below 2^31 for both (fa_capi.hip checks it; batch and head offsets are 64-bit).
//
// The packed and the paged form of the call (fa_fp8_forward_varlen) follow the padded one below: fp8in_vt_varlen_kernel,
// fwd_fp8in_varlen_kernel.
// A sliding window, a softcap and attention sinks (fa_fp8_forward_mod, fa_fp8_forward_varlen_mod) are a
// kernel of their own after those, fwd_fp8in_mod_kernel, for all three forms: a call without them launches the kernels
// above as before.
// Head dims 64 and 256 (fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim) are the last part of the file:
// fwd_fp8in_hdim_kernel and fp8in_vt_hdim_kernel serve every call at those widths; everything before them stays d = 128.
#include <algorithm>

#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"

namespace fa {

// one workgroup = one 64-key block of one K/V unit (blockIdx.x = unit * nb + block: gridDim.y stops at 65535)
__global__ __launch_bounds__(256) void fp8in_vt_kernel(const uint8_t* __restrict__ v, uint8_t* __restrict__ v8t, int nk, int nb,
                                                       int ntile, int hkv, long long v_bs, long long v_hs, long long v_ts) {
    constexpr int D = 128, CPR = D / 16, PER = (64 * CPR) / 256;   // 16-byte chunks per row / per thread
    __shared__ __attribute__((aligned(16))) uint8_t tr[D * 64];   // [d row][permuted key position]
    const int unit = blockIdx.x / nb, blk = blockIdx.x - unit * nb, row0 = blk * 64;
    const int b = unit / hkv, hk = unit - b * hkv;
    const uint8_t* src = v + (size_t)b * v_bs + (size_t)hk * v_hs;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + 256 * i, key = c / CPR, ch = c % CPR;   // key within the 64-key block
        u32x4 x = u32x4{0u, 0u, 0u, 0u};
        if (row0 + key < nk) x = *reinterpret_cast<const u32x4*>(src + (size_t)(row0 + key) * v_ts + 16 * ch);
        const int wlo = key & 31, pos = 32 * (key >> 5) + 16 * ((wlo >> 2) & 1) + (wlo & 3) + 4 * (wlo >> 3);
#pragma unroll
        for (int j = 0; j < 16; ++j) tr[(16 * ch + j) * 64 + pos] = (uint8_t)((x[j >> 2] >> (8 * (j & 3))) & 0xff);
    }
    __syncthreads();
    // d row r of the block: 64 bytes at [tile blk / 2][r][64 (blk & 1) ...]; a thread stores half a row
    const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
    uint8_t* dst = v8t + (((size_t)unit * ntile + (blk >> 1)) * D + r) * 128 + 64 * (blk & 1) + 32 * half;
    const u32x4* s4 = reinterpret_cast<const u32x4*>(tr + r * 64 + 32 * half);
    reinterpret_cast<u32x4*>(dst)[0] = s4[0];
    reinterpret_cast<u32x4*>(dst)[1] = s4[1];
    // an odd block count leaves the second half of the last tile unwritten by any block: zero it (those keys lie past Nk)
    if ((nb & 1) && blk == nb - 1) {
        reinterpret_cast<u32x4*>(dst + 64)[0] = u32x4{0u, 0u, 0u, 0u};
        reinterpret_cast<u32x4*>(dst + 64)[1] = u32x4{0u, 0u, 0u, 0u};
    }
}

struct Fp8InKernelArgs {
    const uint8_t *q, *k, *v8t;
    uint16_t* o;
    float* lse;
    const float *qds, *kds, *vds;          // (B, H_kv) descales at their batch strides; null: 1
    int qds_bs, kds_bs, vds_bs;
    int nq, nk, hq, hkv, group, nqt, ntile;
    int q_ts, k_ts, o_ts;                  // token strides: q and k in bytes, o in elements
    long long q_bs, q_hs, k_bs, k_hs, o_bs, o_hs;
    float c_log2;                          // float(softmax_scale) * log2(e)
};

template <typename Tag, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void fwd_fp8in_kernel(const Fp8InKernelArgs a) {
    constexpr int D = 128, BM = 256, BN = 128, KB = 4, NM = D / 32, NDV = D / 32;
    constexpr int TILE = BN * D;                         // bytes of a K tile and of a V^T tile alike
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K8 tile | V8^T tile]
    typedef int i32x8_t __attribute__((ext_vector_type(8)));

    const int nq = a.nq, nk = a.nk;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / a.nqt;                            // query unit b * H_q + head
    int qt = L - bh * a.nqt;
    if (CAUSAL) qt = a.nqt - 1 - qt;
    const int b = bh / a.hq, hd = bh - b * a.hq, hk = hd / a.group;
    const int ukv = b * a.hkv + hk;                      // the GQA rule: query head hd reads K/V head hd / (H_q / H_kv)
    const int q0 = qt * BM;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int qrow = q0 + 32 * w + r;
    const int shift = nk - nq;                           // row i sees key j <= i + shift

    // q rows >= nq and k rows >= nk lie outside the descriptors: they read as zeros, whatever the memory behind them holds
    const buf_rsrc_t q_rs = make_rsrc(a.q + (size_t)b * a.q_bs + (size_t)hd * a.q_hs, (unsigned)(nq - 1) * (unsigned)a.q_ts + D);
    u32x4 qf[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) qf[m] = __builtin_amdgcn_raw_buffer_load_b128(q_rs, qrow * a.q_ts + 32 * m + 16 * h, 0, 0);
    const float qd = a.qds ? a.qds[(size_t)b * a.qds_bs + hk] : 1.f;
    const float kd = a.kds ? a.kds[(size_t)b * a.kds_bs + hk] : 1.f;
    const float vd = a.vds ? a.vds[(size_t)b * a.vds_bs + hk] : 1.f;
    const float f = (a.c_log2 * qd) * kd;                // the one score factor of this workgroup, > 0

    const int kend = CAUSAL ? max(0, min(nk, q0 + BM + shift)) : nk;
    const int ntiles = (kend + BN - 1) / BN;             // 0: no row of this tile sees a key
    const rsrc_s_t k_rs = make_rsrc_s(a.k + (size_t)b * a.k_bs + (size_t)hk * a.k_hs, (unsigned)(nk - 1) * (unsigned)a.k_ts + D);
    const rsrc_s_t v_rs = make_rsrc_s(a.v8t + (size_t)ukv * a.ntile * TILE, (unsigned)a.ntile * TILE);
    const int kstride = a.k_ts >> 1;                     // the STRIDED helpers count 2-byte elements
    const int voff_k = dma_lane_voff<64, true>(lane, w, 64, kstride);   // 128-byte rows: the geometry of a 16-bit d = 64 tile
    const int voff_v = dma_lane_voff<64>(lane, w);
    auto stage = [&](int buf, int t) {
        char* b_ = smem + buf * 2 * TILE;
        dma_stage_tile<64, BN, 8, true>(k_rs, b_, t * BN, voff_k, w, 64, 0, kstride);
        dma_stage_tile<64, BN, 8>(v_rs, b_ + TILE, t * BN, voff_v, w);   // V^T tile t = rows 128 t .. of the [tile][d row] matrix
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                // running max in log2 units of the scaled score

    if (ntiles > 0) {
        stage(0, 0);
        dma_wait_all();
        __syncthreads();
    }
    const int last_w = q0 + 32 * w + 31 + shift;         // the last key the wave's last row sees under the mask
    const int ntiles_w = CAUSAL ? (last_w < 0 ? 0 : min(ntiles, last_w / BN + 1)) : ntiles;

    for (int t = 0; t < ntiles_w; ++t) {
        const int k0 = t * BN, cur = t & 1;
        if (t + 1 < ntiles) stage(cur ^ 1, t + 1);
        const char* Kt = smem + cur * 2 * TILE;
        const char* Vt = Kt + TILE;
        f32x16 sacc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int M = 0; M < NM / 2; ++M) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<64>::off(32 * kb + r, 4 * M + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<64>::off(32 * kb + r, 4 * M + 2 + h));
                const i32x8_t ka = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                const u32x4 b0_ = qf[2 * M], b1_ = qf[2 * M + 1];
                const i32x8_t qb = {(int)b0_[0], (int)b0_[1], (int)b0_[2], (int)b0_[3], (int)b1_[0], (int)b1_[1], (int)b1_[2], (int)b1_[3]};
                sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb, sacc[kb], 0, 0, 0, 127, 0, 127);
            }
        }
        // mask and row maximum on the RAW products; f > 0 is applied to the maximum once and to every element inside the exp2
        // argument's fma
        const bool need_mask = (CAUSAL && (k0 + BN - 1 > q0 + 32 * w + shift)) || (k0 + BN > nk);
        const int lim = CAUSAL ? min(qrow + shift, nk - 1) : nk - 1;   // (negative: the row sees no key)
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            if (need_mask) {
                const int thr = lim - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
        }
        mx = mx * f;
        mx = fmaxf(mx, wave_half_swap(mx));
        const float m_new = fmaxf(m_run, mx);
        float m_use;
        if (__any(m_new - m_run > 8.0f) != 0) {   // lazy rescale (fa_fwd_mfma.hip); a row's first visible key: inf > 8
            m_use = m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int t2 = 0; t2 < NDV; ++t2)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
        } else {
            m_use = m_run;
        }
        if (m_use == -INFINITY) m_use = 0.f;      // a row without a visible key so far: p = exp2(-inf) = 0, not exp2(-inf + inf)
        float rs = 0.f;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            i32x8_t pb;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int kb = 2 * g + kk;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], f, -m_use));   // (-inf stays -inf: f > 0)
                    sacc[kb][i] = p;
                    rs += p;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int wd = 0;
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 0], sacc[kb][4 * j + 1], wd, false);
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 2], sacc[kb][4 * j + 3], wd, true);
                    pb[4 * kk + j] = wd;
                }
            }
#pragma unroll
            for (int dvb = 0; dvb < NDV; ++dvb) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * g + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * g + 2 + h));
                const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], 0, 0, 0, 127, 0, 127);
            }
        }
        l_run += rs;
        dma_wait_all();
        __syncthreads();
    }
    for (int t = ntiles_w; t < ntiles; ++t) {
        if (t + 1 < ntiles) stage((t & 1) ^ 1, t + 1);
        dma_wait_all();
        __syncthreads();
    }

    // every wave is past the last barrier (the tile loops end with one): the K / V buffers are dead and each wave turns its
    // row-on-the-lane tile into whole-row stores through 8 KiB of them (fa_fwd_mfma.hip's epilogue)
    const float l_tot = l_run + wave_half_swap(l_run);
    const bool dead = l_tot == 0.f;                      // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
    const float inv = vd * (1.f / l_tot);                // v_descale once, with 1 / l
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
            vals[4 * dvb + g][0] = pack2_rn<Tag>(y[0], y[1]);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(y[2], y[3]);
        }
    store_rows_via_lds<D, true>(smem + w * 32 * D * 2, vals, a.o + (size_t)b * a.o_bs + (size_t)hd * a.o_hs, q0 + 32 * w, nq, lane, D, -1,
                                a.o_ts);
    if (qrow < nq && h == 0) a.lse[(size_t)bh * nq + qrow] = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
}

size_t fp8in_workspace_bytes(int64_t units_kv, int64_t nk, int64_t d) {
    return (size_t)units_kv * (size_t)((nk + 127) / 128) * (size_t)d * 128 + 256;   // V^T tiles (d rows of 128 key bytes) and a pad
}

// the transposer's launch and the attention kernel's arguments: what fa_fp8_forward and fa_fp8_forward_mod share on the host
static hipError_t fp8in_launch_vt(const Fp8InArgs& c, hipStream_t st) {
    const int nb = (int)((c.nk + 63) / 64), ntile = (int)((c.nk + 127) / 128);
    const int64_t units_kv = c.batch * c.heads_kv;
    {
        ProfScope ps(K_FP8IN_VT, st);
        hipLaunchKernelGGL(fp8in_vt_kernel, dim3((unsigned)(units_kv * nb)), dim3(256), 0, st, (const uint8_t*)c.v, (uint8_t*)c.workspace,
                           (int)c.nk, nb, ntile, (int)c.heads_kv, (long long)c.v_bs, (long long)c.v_hs, (long long)c.v_ts);
    }
    return hipGetLastError();
}

static Fp8InKernelArgs fp8in_kernel_args(const Fp8InArgs& c) {
    Fp8InKernelArgs a;
    a.q = (const uint8_t*)c.q; a.k = (const uint8_t*)c.k; a.v8t = (const uint8_t*)c.workspace;
    a.o = (uint16_t*)c.o; a.lse = c.lse;
    a.qds = c.q_descale; a.kds = c.k_descale; a.vds = c.v_descale;
    a.qds_bs = (int)c.qds_bs; a.kds_bs = (int)c.kds_bs; a.vds_bs = (int)c.vds_bs;
    a.nq = (int)c.nq; a.nk = (int)c.nk; a.hq = (int)c.heads_q; a.hkv = (int)c.heads_kv; a.group = (int)(c.heads_q / c.heads_kv);
    a.nqt = (int)((c.nq + 255) / 256); a.ntile = (int)((c.nk + 127) / 128);
    a.q_ts = (int)c.q_ts; a.k_ts = (int)c.k_ts; a.o_ts = (int)c.o_ts;
    a.q_bs = c.q_bs; a.q_hs = c.q_hs; a.k_bs = c.k_bs; a.k_hs = c.k_hs; a.o_bs = c.o_bs; a.o_hs = c.o_hs;
    a.c_log2 = c.scale * 1.4426950408889634f;
    return a;
}

hipError_t launch_fp8_inputs(const Fp8InArgs& c, hipStream_t st) {
    const hipError_t e = fp8in_launch_vt(c, st);
    if (e != hipSuccess) return e;
    const Fp8InKernelArgs a = fp8in_kernel_args(c);
    const size_t smem = 2 * 2 * 128 * 128;
    const unsigned grid = (unsigned)(c.batch * c.heads_q * a.nqt);
    ProfScope ps(K_FP8IN_FWD, st);
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e2 = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), smem, st, a);
        return hipGetLastError();
    };
    if (c.dtype == 2) return c.causal ? launch(fwd_fp8in_kernel<bf16_tag, true>) : launch(fwd_fp8in_kernel<bf16_tag, false>);
    return c.causal ? launch(fwd_fp8in_kernel<f16_tag, true>) : launch(fwd_fp8in_kernel<f16_tag, false>);
}

// ---- The packed and the paged form (include/fa_mi355x.h: fa_fp8_forward_varlen) --------------------------
// q is (total_q, H_q, 128) packed by cu_seqlens_q; k and v are (total_k, H_kv, 128) packed by cu_seqlens_k, or, with a block
// table, pools (num_blocks, ps, H_kv, 128) in which key t of sequence b is row t % ps of page table[b][t / ps].  Every sequence
// gets the bits of fa_fp8_forward on that sequence alone: the loop below is fwd_fp8in_kernel's text from the first `stage` call to
// the epilogue, DUPLICATED rather than shared (a shared device function must not change fwd_fp8in_kernel's instructions, and the
// two kernels differ in every value that text closes over), and the transposer writes fp8in_vt_kernel's image per sequence.
//
// The V^T workspace is [K/V head][tile][d row][128 key bytes] with `nt_head` tiles a head.  Sequence b's tiles start at
//   packed   floor(start_b / 128) + b      start_b its clamped first key; floor((s + l) / 128) - floor(s / 128) + 1 >= ceil(l / 128), so
//                                          the regions of consecutive sequences do not overlap and end inside
//                                          nt_head = floor(total_k / 128) + B tiles
//   paged    b * nt_seq                    nt_seq = ceil(cap / 128), cap = min(max_seqlen_k, max_blocks * ps); nt_head = B * nt_seq
// both computable on the device from the offsets alone, and the size on the host from shapes alone.
// Offsets and table are untrusted: lengths are clamped (seq_span / paged_len, fa_ex_common.h), a page outside [0, num_blocks) reads
// as zero bytes for K and V, and no table entry past ceil(len_k / ps) is read.
struct Fp8InVarKernelArgs {
    const uint8_t *q, *k, *v8t;
    uint16_t* o;
    float* lse;                            // (H_q, total_q)
    const float *qds, *kds, *vds;          // (B, H_kv) descales at their batch strides; null: 1
    int qds_bs, kds_bs, vds_bs;
    const int *cu_q, *cu_k;                // [B + 1] untrusted offsets
    int total_q, total_k, max_q, max_k;    // max_k: the cap on a sequence's keys (paged: min(max_seqlen_k, max_blocks * ps))
    int hq, hkv, group, nqt, nt_head, nt_seq;
    int q_ts, k_ts, o_ts;                  // token strides: q and k in bytes, o in elements
    long long q_hs, k_hs, o_hs;
    ExPage pg;                             // PAGED: table, K page stride in kps (bytes); vps is not used here
    float c_log2;
};

// tiles before sequence b's in a head's part of the workspace; ks: its clamped first key (packed)
template <bool PAGED> __device__ __forceinline__ int fp8in_tile_start(int b, int ks, int nt_seq) {
    return PAGED ? b * nt_seq : (ks >> 7) + b;
}

// one workgroup = one 64-key block of one (sequence, K/V head); the grid is padded to the cap on a sequence's keys, and a block
// past its sequence's last one has no tile half of its own to write (the last block zeroes the other half of an odd last tile)
template <bool PAGED>
__global__ __launch_bounds__(256) void fp8in_vt_varlen_kernel(const uint8_t* __restrict__ v, uint8_t* __restrict__ v8t,
                                                              const int* __restrict__ cu_k, int total_k, int max_k, int nbmax,
                                                              int nt_head, int nt_seq, int hkv, long long v_hs, long long v_ts,
                                                              const ExPage pg) {
    constexpr int D = 128, CPR = D / 16, PER = (64 * CPR) / 256;   // 16-byte chunks per row / per thread
    __shared__ __attribute__((aligned(16))) uint8_t tr[D * 64];   // [d row][permuted key position]
    const int unit = blockIdx.x / nbmax, blk = blockIdx.x - unit * nbmax, row0 = blk * 64;
    const int b = unit / hkv, hk = unit - b * hkv;
    int ks = 0, nk;
    if (PAGED) nk = paged_len(cu_k, b, max_k);
    else seq_span(cu_k, b, total_k, max_k, ks, nk);
    const int nb = (nk + 63) >> 6;
    if (blk >= nb) return;
    const uint8_t* src = v + (size_t)hk * v_hs + (PAGED ? (size_t)0 : (size_t)ks * v_ts);
    [[maybe_unused]] const int* trow = PAGED ? pg.table + (size_t)b * pg.max_blocks : nullptr;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + 256 * i, key = c / CPR, ch = c % CPR;   // key within the 64-key block
        u32x4 x = u32x4{0u, 0u, 0u, 0u};
        if (row0 + key < nk) {
            if (PAGED) {
                // a 16-key group never straddles a page (ps % 16 == 0): one entry serves it, and key < nk keeps the slot below
                // ceil(nk / ps)
                const int slot = pg_slot(pg, row0 + key), page = trow[slot];
                if ((unsigned)page < (unsigned)pg.num_blocks)
                    x = *reinterpret_cast<const u32x4*>(src + (size_t)page * pg.vps + (size_t)(row0 + key - slot * pg.ps) * v_ts + 16 * ch);
            } else {
                x = *reinterpret_cast<const u32x4*>(src + (size_t)(row0 + key) * v_ts + 16 * ch);
            }
        }
        const int wlo = key & 31, pos = 32 * (key >> 5) + 16 * ((wlo >> 2) & 1) + (wlo & 3) + 4 * (wlo >> 3);
#pragma unroll
        for (int j = 0; j < 16; ++j) tr[(16 * ch + j) * 64 + pos] = (uint8_t)((x[j >> 2] >> (8 * (j & 3))) & 0xff);
    }
    __syncthreads();
    const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
    const size_t tile = (size_t)hk * nt_head + fp8in_tile_start<PAGED>(b, ks, nt_seq) + (blk >> 1);
    uint8_t* dst = v8t + (tile * D + r) * 128 + 64 * (blk & 1) + 32 * half;
    const u32x4* s4 = reinterpret_cast<const u32x4*>(tr + r * 64 + 32 * half);
    reinterpret_cast<u32x4*>(dst)[0] = s4[0];
    reinterpret_cast<u32x4*>(dst)[1] = s4[1];
    if ((nb & 1) && blk == nb - 1) {
        reinterpret_cast<u32x4*>(dst + 64)[0] = u32x4{0u, 0u, 0u, 0u};
        reinterpret_cast<u32x4*>(dst + 64)[1] = u32x4{0u, 0u, 0u, 0u};
    }
}

// One K tile of a paged call: dma_stage_kv_paged's pieces (fa_ex_common.h) for K alone, with e4m3 rows.  A 1-KiB piece is 8 rows,
// 8 | 16 | ps, so a piece lies inside one page and one wave-uniform table entry serves it.  Each piece gets a descriptor of its
// own in SGPRs: the 64-bit address of its first row and as num_records the bytes of its rows below nk, 0 for a piece past the end
// or on a page outside the pool (every lane fails the range check and lands as zero).  No branch around the DMA: the image is
// always fully written.  make_rsrc_s's v_readfirstlane writes stand right before dma16_issue, whose s_mov m0 + s_nop 3 are the
// wait states the buffer instruction needs after them.  The table is not written while the kernel runs, and its entry is read
// through the constant address space so that it is a scalar load: as a plain global pointer it became a vector load (the DMA's
// asm statements clobber memory, so hipcc does not prove the table unchanged) whose whole latency stood in front of every tile
// (profiles/fp8_varlen.md).
// Head dim D (fwd_fp8in_mod_kernel at 64 and 256): a piece is RPP = 1024 / D rows, 16 or 4, which still divide 16 | ps, and a
// wave issues D / 64 of them; the pieces of a wave lie 8 RPP rows apart, a multiple of 16, so one voff_k serves them all.
typedef const int __attribute__((address_space(4)))* fp8in_const_int_p;
template <int D = 128>
__device__ __forceinline__ void fp8in_stage_k_paged(const ExPage& pg, const int* __restrict__ trow, int last, const uint8_t* kh, char* ktile,
                                                    int row0, int nk, int voff_k, int w, int k_ts) {
    constexpr int RPP = 1024 / D;
    const unsigned tk = lds_addr_of(ktile);
#pragma unroll
    for (int j = 0; j < D / 64; ++j) {
        const int pc = w + 8 * j;
        const int key = __builtin_amdgcn_readfirstlane(row0 + RPP * pc);
        const int rows = min(RPP, nk - key);             // <= 0: the piece lies past the sequence
        const int slot = min(pg_slot(pg, key), last);    // no entry past ceil(nk / ps) is read
        const int page = ((fp8in_const_int_p)trow)[slot];
        const bool ok = rows > 0 && (unsigned)page < (unsigned)pg.num_blocks;
        const long long ko = ok ? (long long)page * pg.kps + (long long)(key - slot * pg.ps) * k_ts : 0ll;
        dma16_issue(make_rsrc_s(kh + ko, ok ? (unsigned)(rows - 1) * (unsigned)k_ts + (unsigned)D : 0u), tk + pc * 1024, voff_k, 0);
    }
}

template <typename Tag, bool CAUSAL, bool PAGED>
__global__ __launch_bounds__(512, 2) void fwd_fp8in_varlen_kernel(const Fp8InVarKernelArgs a) {
    constexpr int D = 128, BM = 256, BN = 128, KB = 4, NM = D / 32, NDV = D / 32;
    constexpr int TILE = BN * D;                         // bytes of a K tile and of a V^T tile alike
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K8 tile | V8^T tile]
    typedef int i32x8_t __attribute__((ext_vector_type(8)));

    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / a.nqt;                            // b * H_q + head
    int qt = L - bh * a.nqt;
    if (CAUSAL) qt = a.nqt - 1 - qt;
    const int b = bh / a.hq, hd = bh - b * a.hq, hk = hd / a.group;
    int qs, nq, ks = 0, nk;                              // this sequence's clamped spans
    seq_span(a.cu_q, b, a.total_q, a.max_q, qs, nq);
    if (PAGED) nk = paged_len(a.cu_k, b, a.max_k);
    else seq_span(a.cu_k, b, a.total_k, a.max_k, ks, nk);
    const int q0 = qt * BM;
    if (q0 >= nq) return;                                // the padded grid: no row of this tile belongs to the sequence
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int qrow = q0 + 32 * w + r;
    const int shift = nk - nq;                           // row i sees key j <= i + shift

    const buf_rsrc_t q_rs = make_rsrc(a.q + (size_t)qs * a.q_ts + (size_t)hd * a.q_hs, (unsigned)(nq - 1) * (unsigned)a.q_ts + D);
    u32x4 qf[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) qf[m] = __builtin_amdgcn_raw_buffer_load_b128(q_rs, qrow * a.q_ts + 32 * m + 16 * h, 0, 0);
    const float qd = a.qds ? a.qds[(size_t)b * a.qds_bs + hk] : 1.f;
    const float kd = a.kds ? a.kds[(size_t)b * a.kds_bs + hk] : 1.f;
    const float vd = a.vds ? a.vds[(size_t)b * a.vds_bs + hk] : 1.f;
    const float f = (a.c_log2 * qd) * kd;                // the one score factor of this workgroup, > 0

    const int kend = CAUSAL ? max(0, min(nk, q0 + BM + shift)) : nk;
    const int ntiles = (kend + BN - 1) / BN;             // 0: no row of this tile sees a key
    const int ntile_b = (nk + BN - 1) / BN;              // this sequence's V^T tiles
    const uint8_t* kh = a.k + (size_t)hk * a.k_hs + (PAGED ? (size_t)0 : (size_t)ks * a.k_ts);
    [[maybe_unused]] const rsrc_s_t k_rs = make_rsrc_s(kh, nk > 0 ? (unsigned)(nk - 1) * (unsigned)a.k_ts + D : 0u);
    const rsrc_s_t v_rs = make_rsrc_s(a.v8t + ((size_t)hk * a.nt_head + fp8in_tile_start<PAGED>(b, ks, a.nt_seq)) * TILE,
                                      (unsigned)ntile_b * TILE);
    const int kstride = a.k_ts >> 1;                     // the STRIDED helpers count 2-byte elements
    const int voff_k = dma_lane_voff<64, true>(lane, w, 64, kstride);   // 128-byte rows: the geometry of a 16-bit d = 64 tile
    const int voff_v = dma_lane_voff<64>(lane, w);
    [[maybe_unused]] const int* trow = PAGED ? a.pg.table + (size_t)b * a.pg.max_blocks : nullptr;
    [[maybe_unused]] const int pg_last = PAGED ? pg_slot(a.pg, max(nk - 1, 0)) : 0;   // no entry past ceil(nk / ps) is read
    auto stage = [&](int buf, int t) {
        char* b_ = smem + buf * 2 * TILE;
        if constexpr (PAGED) {
            fp8in_stage_k_paged(a.pg, trow, pg_last, kh, b_, t * BN, nk, voff_k, w, a.k_ts);
        } else {
            dma_stage_tile<64, BN, 8, true>(k_rs, b_, t * BN, voff_k, w, 64, 0, kstride);
        }
        dma_stage_tile<64, BN, 8>(v_rs, b_ + TILE, t * BN, voff_v, w);   // V^T tile t = rows 128 t .. of the [tile][d row] matrix
    };

    // ---- from here to the stores: fwd_fp8in_kernel's text
    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                // running max in log2 units of the scaled score

    if (ntiles > 0) {
        stage(0, 0);
        dma_wait_all();
        __syncthreads();
    }
    const int last_w = q0 + 32 * w + 31 + shift;         // the last key the wave's last row sees under the mask
    const int ntiles_w = CAUSAL ? (last_w < 0 ? 0 : min(ntiles, last_w / BN + 1)) : ntiles;

    for (int t = 0; t < ntiles_w; ++t) {
        const int k0 = t * BN, cur = t & 1;
        if (t + 1 < ntiles) stage(cur ^ 1, t + 1);
        const char* Kt = smem + cur * 2 * TILE;
        const char* Vt = Kt + TILE;
        f32x16 sacc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int M = 0; M < NM / 2; ++M) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<64>::off(32 * kb + r, 4 * M + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<64>::off(32 * kb + r, 4 * M + 2 + h));
                const i32x8_t ka = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                const u32x4 b0_ = qf[2 * M], b1_ = qf[2 * M + 1];
                const i32x8_t qb = {(int)b0_[0], (int)b0_[1], (int)b0_[2], (int)b0_[3], (int)b1_[0], (int)b1_[1], (int)b1_[2], (int)b1_[3]};
                sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb, sacc[kb], 0, 0, 0, 127, 0, 127);
            }
        }
        const bool need_mask = (CAUSAL && (k0 + BN - 1 > q0 + 32 * w + shift)) || (k0 + BN > nk);
        const int lim = CAUSAL ? min(qrow + shift, nk - 1) : nk - 1;   // (negative: the row sees no key)
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            if (need_mask) {
                const int thr = lim - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
        }
        mx = mx * f;
        mx = fmaxf(mx, wave_half_swap(mx));
        const float m_new = fmaxf(m_run, mx);
        float m_use;
        if (__any(m_new - m_run > 8.0f) != 0) {   // lazy rescale; a row's first visible key: inf > 8
            m_use = m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int t2 = 0; t2 < NDV; ++t2)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
        } else {
            m_use = m_run;
        }
        if (m_use == -INFINITY) m_use = 0.f;      // a row without a visible key so far: p = exp2(-inf) = 0, not exp2(-inf + inf)
        float rs = 0.f;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            i32x8_t pb;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int kb = 2 * g + kk;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], f, -m_use));   // (-inf stays -inf: f > 0)
                    sacc[kb][i] = p;
                    rs += p;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int wd = 0;
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 0], sacc[kb][4 * j + 1], wd, false);
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 2], sacc[kb][4 * j + 3], wd, true);
                    pb[4 * kk + j] = wd;
                }
            }
#pragma unroll
            for (int dvb = 0; dvb < NDV; ++dvb) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * g + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * g + 2 + h));
                const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], 0, 0, 0, 127, 0, 127);
            }
        }
        l_run += rs;
        dma_wait_all();
        __syncthreads();
    }
    for (int t = ntiles_w; t < ntiles; ++t) {
        if (t + 1 < ntiles) stage((t & 1) ^ 1, t + 1);
        dma_wait_all();
        __syncthreads();
    }

    const float l_tot = l_run + wave_half_swap(l_run);
    const bool dead = l_tot == 0.f;                      // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
    const float inv = vd * (1.f / l_tot);                // v_descale once, with 1 / l
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
            vals[4 * dvb + g][0] = pack2_rn<Tag>(y[0], y[1]);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(y[2], y[3]);
        }
    // the sequence's rows of o (total_q, H_q, 128) and of lse (H_q, total_q): rows >= nq are not stored
    store_rows_via_lds<D, true>(smem + w * 32 * D * 2, vals, a.o + (size_t)qs * a.o_ts + (size_t)hd * a.o_hs, q0 + 32 * w, nq, lane, D, -1,
                                a.o_ts);
    if (qrow < nq && h == 0) a.lse[(size_t)hd * a.total_q + qs + qrow] = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
}

int64_t fp8in_varlen_tiles_per_head(const Fp8InVarArgs& c) {
    if (c.page_size > 0) return c.batch * ((std::min(c.max_k, c.max_blocks * c.page_size) + 127) / 128);   // (0: the packed form)
    return c.total_k / 128 + c.batch;
}

size_t fp8in_varlen_workspace_bytes(const Fp8InVarArgs& c) {
    return (size_t)c.heads_kv * (size_t)fp8in_varlen_tiles_per_head(c) * (size_t)c.d * 128 + 256;   // V^T tiles and a pad
}

// the transposer of the head dims 64 and 256 (at the end of the file)
struct Fp8InVtArgs {
    const uint8_t* v;
    uint8_t* v8t;
    const int* cu_k;
    int nk, total_k, max_k, nb, ntile, nt_head, nt_seq, hkv;   // nb: the grid's 64-key blocks a (sequence, K/V head)
    long long v_bs, v_hs, v_ts;
    ExPage pg;
};
static Fp8InVtArgs fp8in_vt_hdim_args(const Fp8InVarArgs& c, const ExPage& pg, int cap, int nbmax, int nt_head, int nt_seq);
template <int MODE> static hipError_t fp8in_launch_vt_hdim(const Fp8InVtArgs& a, int d, unsigned grid, hipStream_t st);

// the transposer's launch and the attention kernel's arguments: what fa_fp8_forward_varlen and fa_fp8_forward_varlen_mod share
// on the host (c.max_q > 0)
template <bool PAGED> static hipError_t fp8in_varlen_front(const Fp8InVarArgs& c, hipStream_t st, Fp8InVarKernelArgs& a) {
    const int64_t cap = PAGED ? std::min(c.max_k, c.max_blocks * c.page_size) : c.max_k;
    const int nbmax = (int)((cap + 63) / 64), nqt = (int)((c.max_q + 255) / 256);
    const int nt_head = (int)fp8in_varlen_tiles_per_head(c), nt_seq = (int)((cap + 127) / 128);
    ExPage pg{};
    if (PAGED) {
        pg.table = c.block_table; pg.kps = c.k_ps; pg.vps = c.v_ps;
        pg.max_blocks = (int)c.max_blocks; pg.num_blocks = (int)c.num_blocks; pg.ps = (int)c.page_size;
        pg.ps16m = kv_magic((int)(c.page_size / 16));
    }
    if (nbmax > 0 && c.d != 128) {                        // (fa_fp8_forward_varlen_hdim: the transposer at the end of the file)
        const hipError_t e = fp8in_launch_vt_hdim<PAGED ? 2 : 1>(fp8in_vt_hdim_args(c, pg, (int)cap, nbmax, nt_head, nt_seq), (int)c.d,
                                                                 (unsigned)(c.batch * c.heads_kv * nbmax), st);
        if (e != hipSuccess) return e;
    } else if (nbmax > 0) {
        ProfScope ps(K_FP8IN_VT_VARLEN, st);
        hipLaunchKernelGGL(fp8in_vt_varlen_kernel<PAGED>, dim3((unsigned)(c.batch * c.heads_kv * nbmax)), dim3(256), 0, st,
                           (const uint8_t*)c.v, (uint8_t*)c.workspace, c.cu_k, (int)c.total_k, (int)cap, nbmax, nt_head, nt_seq,
                           (int)c.heads_kv, (long long)c.v_hs, (long long)c.v_ts, pg);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    a.q = (const uint8_t*)c.q; a.k = (const uint8_t*)c.k; a.v8t = (const uint8_t*)c.workspace;
    a.o = (uint16_t*)c.o; a.lse = c.lse;
    a.qds = c.q_descale; a.kds = c.k_descale; a.vds = c.v_descale;
    a.qds_bs = (int)c.qds_bs; a.kds_bs = (int)c.kds_bs; a.vds_bs = (int)c.vds_bs;
    a.cu_q = c.cu_q; a.cu_k = c.cu_k;
    a.total_q = (int)c.total_q; a.total_k = (int)c.total_k; a.max_q = (int)c.max_q; a.max_k = (int)cap;
    a.hq = (int)c.heads_q; a.hkv = (int)c.heads_kv; a.group = (int)(c.heads_q / c.heads_kv);
    a.nqt = nqt; a.nt_head = nt_head; a.nt_seq = nt_seq;
    a.q_ts = (int)c.q_ts; a.k_ts = (int)c.k_ts; a.o_ts = (int)(c.heads_q * c.d);
    a.q_hs = c.q_hs; a.k_hs = c.k_hs; a.o_hs = c.d;
    a.pg = pg;
    a.c_log2 = c.scale * 1.4426950408889634f;
    return hipSuccess;
}

template <bool PAGED> static hipError_t launch_fp8_inputs_varlen_t(const Fp8InVarArgs& c, hipStream_t st) {
    if (c.max_q == 0) return hipSuccess;                 // no sequence has a query: nothing is written
    Fp8InVarKernelArgs a;
    const hipError_t e = fp8in_varlen_front<PAGED>(c, st, a);
    if (e != hipSuccess) return e;
    const size_t smem = 2 * 2 * 128 * 128;
    const unsigned grid = (unsigned)(c.batch * c.heads_q * a.nqt);
    ProfScope ps(K_FP8IN_FWD_VARLEN, st);
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e2 = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), smem, st, a);
        return hipGetLastError();
    };
    if (c.dtype == 2)
        return c.causal ? launch(fwd_fp8in_varlen_kernel<bf16_tag, true, PAGED>) : launch(fwd_fp8in_varlen_kernel<bf16_tag, false, PAGED>);
    return c.causal ? launch(fwd_fp8in_varlen_kernel<f16_tag, true, PAGED>) : launch(fwd_fp8in_varlen_kernel<f16_tag, false, PAGED>);
}

hipError_t launch_fp8_inputs_varlen(const Fp8InVarArgs& c, hipStream_t st) {
    return c.block_table ? launch_fp8_inputs_varlen_t<true>(c, st) : launch_fp8_inputs_varlen_t<false>(c, st);
}

// ---- A sliding window, a softcap and sinks (fa_fp8_forward_mod, fa_fp8_forward_varlen_mod) -------------
// One kernel of its own for the padded (MODE 0), the packed (1) and the paged (2) form, so that a call without the three
// features launches fwd_fp8in_kernel / fwd_fp8in_varlen_kernel as before.  The three features are wave-uniform run-time
// switches.  The transposers are the ones above and still transpose every key of a sequence.
//   window   row i of a sequence sits at pos = i + len_k - len_q and sees key j iff pos - wl <= j <= pos + wr and 0 <= j < len_k
//            (kWinNone: unbounded; causal is wr = 0).  The workgroup's tile loop, with its double-buffered staging, runs over
//            the 128-key tiles [t_lo, t_hi) that some row of its 256 sees: O(N w) work.  A wave computes on the tiles
//            [tw_lo, tw_hi) some row of its 32 sees and only takes part in the barriers of the others.  The mask compares
//            with an upper and a lower threshold, each only on a tile that edge crosses.
//   softcap  s~ = C tanh(s / C) with s = softmax_scale q_descale k_descale (q8 . k8), BEFORE the mask, as mod_softcap has it:
//            in log2 units s~ = cap2 (1 - 2 r), r = 1 / (2^(ck raw) + 1), ck = f (2 / C), cap2 = C log2(e), f the workgroup's
//            score factor.  The capped score replaces the raw product in the accumulator and the factor of what follows is 1.
//   sinks    one float32 per QUERY head in natural-log units, an extra softmax column with a zero value, never capped or
//            masked.  It enters in the epilogue after the half-wave sum of l, by ex_sink_norm (finite at +-1e4).  A row
//            without a visible key gives o = 0, lse = sink; a head at -inf takes the epilogue of a call without sinks.
struct Fp8InModKernelArgs {
    Fp8InKernelArgs pad;                   // MODE 0
    Fp8InVarKernelArgs var;                // MODE 1, 2
    int wl, wr;                            // kWinNone: unbounded
    int rev;                               // causal: the long query tiles first
    float cap_k, cap2;                     // 2 / softcap, softcap * log2(e); cap2 == 0: no softcap
    const float* sinks;                    // (H_q,) or null
};

template <typename Tag, int MODE>
__global__ __launch_bounds__(512, 2) void fwd_fp8in_mod_kernel(const Fp8InModKernelArgs am) {
    constexpr bool VAR = MODE != 0, PAGED = MODE == 2;
    constexpr int D = 128, BM = 256, BN = 128, KB = 4, NM = D / 32, NDV = D / 32;
    constexpr int TILE = BN * D;                         // bytes of a K tile and of a V^T tile alike
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K8 tile | V8^T tile]
    typedef int i32x8_t __attribute__((ext_vector_type(8)));

    // ---- the sequence and its tensors: fwd_fp8in_kernel's (MODE 0) or fwd_fp8in_varlen_kernel's prologue
    const int nqt = VAR ? am.var.nqt : am.pad.nqt, hq = VAR ? am.var.hq : am.pad.hq, group = VAR ? am.var.group : am.pad.group;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;                              // b * H_q + head
    int qt = L - bh * nqt;
    if (am.rev) qt = nqt - 1 - qt;
    const int b = bh / hq, hd = bh - b * hq, hk = hd / group;
    const int q0 = qt * BM;
    int nq, nk, qs = 0, ks = 0;
    if constexpr (VAR) {
        seq_span(am.var.cu_q, b, am.var.total_q, am.var.max_q, qs, nq);
        if (PAGED) nk = paged_len(am.var.cu_k, b, am.var.max_k);
        else seq_span(am.var.cu_k, b, am.var.total_k, am.var.max_k, ks, nk);
        if (q0 >= nq) return;                            // the padded grid: no row of this tile belongs to the sequence
    } else {
        nq = am.pad.nq; nk = am.pad.nk;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int qrow = q0 + 32 * w + r;
    const int shift = nk - nq;                           // row i sits at key position i + shift
    const int q_ts = VAR ? am.var.q_ts : am.pad.q_ts, k_ts = VAR ? am.var.k_ts : am.pad.k_ts, o_ts = VAR ? am.var.o_ts : am.pad.o_ts;
    const uint8_t* qbase;
    const uint8_t* kh;                                   // the K rows of this K/V head (PAGED: of page 0)
    const uint8_t* vbase;
    uint16_t* obase;
    const float *qds, *kds, *vds;
    int qds_bs, kds_bs, vds_bs, ntile_b;
    if constexpr (VAR) {
        qbase = am.var.q + (size_t)qs * q_ts + (size_t)hd * am.var.q_hs;
        kh = am.var.k + (size_t)hk * am.var.k_hs + (PAGED ? (size_t)0 : (size_t)ks * k_ts);
        ntile_b = (nk + BN - 1) / BN;
        vbase = am.var.v8t + ((size_t)hk * am.var.nt_head + fp8in_tile_start<PAGED>(b, ks, am.var.nt_seq)) * TILE;
        obase = am.var.o + (size_t)qs * o_ts + (size_t)hd * am.var.o_hs;
        qds = am.var.qds; kds = am.var.kds; vds = am.var.vds;
        qds_bs = am.var.qds_bs; kds_bs = am.var.kds_bs; vds_bs = am.var.vds_bs;
    } else {
        qbase = am.pad.q + (size_t)b * am.pad.q_bs + (size_t)hd * am.pad.q_hs;
        kh = am.pad.k + (size_t)b * am.pad.k_bs + (size_t)hk * am.pad.k_hs;
        ntile_b = am.pad.ntile;
        vbase = am.pad.v8t + (size_t)(b * am.pad.hkv + hk) * am.pad.ntile * TILE;
        obase = am.pad.o + (size_t)b * am.pad.o_bs + (size_t)hd * am.pad.o_hs;
        qds = am.pad.qds; kds = am.pad.kds; vds = am.pad.vds;
        qds_bs = am.pad.qds_bs; kds_bs = am.pad.kds_bs; vds_bs = am.pad.vds_bs;
    }

    // q rows >= nq and k rows >= nk lie outside the descriptors: they read as zeros, whatever the memory behind them holds
    const buf_rsrc_t q_rs = make_rsrc(qbase, (unsigned)(nq - 1) * (unsigned)q_ts + D);
    u32x4 qf[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) qf[m] = __builtin_amdgcn_raw_buffer_load_b128(q_rs, qrow * q_ts + 32 * m + 16 * h, 0, 0);
    const float qd = qds ? qds[(size_t)b * qds_bs + hk] : 1.f;
    const float kd = kds ? kds[(size_t)b * kds_bs + hk] : 1.f;
    const float vd = vds ? vds[(size_t)b * vds_bs + hk] : 1.f;
    const float f = ((VAR ? am.var.c_log2 : am.pad.c_log2) * qd) * kd;   // the one score factor of this workgroup, > 0
    const bool capped = am.cap2 != 0.f;
    const float ck = f * am.cap_k, cap2 = am.cap2;
    const float fe = capped ? 1.f : f;                   // the factor of what the accumulators hold after the cap

    // the 128-key tiles [t_lo, t_hi) some row of the workgroup sees, from its first row's lower and its last row's upper bound
    const int wl = am.wl, wr = am.wr;
    const int kfirst = max(0, q0 + shift - wl), kend = max(0, min(nk, q0 + BM + shift + wr));
    const int t_lo = kfirst / BN, t_hi = kend > kfirst ? (kend + BN - 1) / BN : t_lo;
    [[maybe_unused]] const rsrc_s_t k_rs = make_rsrc_s(kh, nk > 0 ? (unsigned)(nk - 1) * (unsigned)k_ts + D : 0u);
    const rsrc_s_t v_rs = make_rsrc_s(vbase, (unsigned)ntile_b * TILE);
    const int kstride = k_ts >> 1;                       // the STRIDED helpers count 2-byte elements
    const int voff_k = dma_lane_voff<64, true>(lane, w, 64, kstride);   // 128-byte rows: the geometry of a 16-bit d = 64 tile
    const int voff_v = dma_lane_voff<64>(lane, w);
    [[maybe_unused]] const int* trow = PAGED ? am.var.pg.table + (size_t)b * am.var.pg.max_blocks : nullptr;
    [[maybe_unused]] const int pg_last = PAGED ? pg_slot(am.var.pg, max(nk - 1, 0)) : 0;   // no entry past ceil(nk / ps) is read
    auto stage = [&](int buf, int t) {
        char* b_ = smem + buf * 2 * TILE;
        if constexpr (PAGED) {
            fp8in_stage_k_paged(am.var.pg, trow, pg_last, kh, b_, t * BN, nk, voff_k, w, k_ts);
        } else {
            dma_stage_tile<64, BN, 8, true>(k_rs, b_, t * BN, voff_k, w, 64, 0, kstride);
        }
        dma_stage_tile<64, BN, 8>(v_rs, b_ + TILE, t * BN, voff_v, w);   // V^T tile t = rows 128 t .. of the [tile][d row] matrix
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                // running max in log2 units of the (capped) scaled score

    if (t_hi > t_lo) {
        stage(0, t_lo);
        dma_wait_all();
        __syncthreads();
    }
    // the tiles some row of the wave sees: its first row's lower bound, its last row's upper bound
    const int pos_w = q0 + 32 * w + shift;               // the position of the wave's first row
    const int last_w = pos_w + 31 + wr;
    const int tw_lo = max(t_lo, max(0, pos_w - wl) / BN), tw_hi = last_w < 0 ? t_lo : min(t_hi, last_w / BN + 1);
    const int lim_hi = min(qrow + shift + wr, nk - 1), lim_lo = qrow + shift - wl;   // this row sees keys [lim_lo, lim_hi]

    for (int t = t_lo; t < t_hi; ++t) {
        const int k0 = t * BN, cur = (t - t_lo) & 1;
        if (t + 1 < t_hi) stage(cur ^ 1, t + 1);
        if (t >= tw_lo && t < tw_hi) {                   // (wave-uniform)
        const char* Kt = smem + cur * 2 * TILE;
        const char* Vt = Kt + TILE;
        f32x16 sacc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int M = 0; M < NM / 2; ++M) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<64>::off(32 * kb + r, 4 * M + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<64>::off(32 * kb + r, 4 * M + 2 + h));
                const i32x8_t ka = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                const u32x4 b0_ = qf[2 * M], b1_ = qf[2 * M + 1];
                const i32x8_t qb = {(int)b0_[0], (int)b0_[1], (int)b0_[2], (int)b0_[3], (int)b1_[0], (int)b1_[1], (int)b1_[2], (int)b1_[3]};
                sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb, sacc[kb], 0, 0, 0, 127, 0, 127);
            }
        }
        // the softcap first (before the mask), in log2 units: one exp2 and one rcp an element
        if (capped) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * ck) + 1.f);
                    sacc[kb][i] = fmaf(rr, -2.f * cap2, cap2);
                }
        }
        // the mask, only where a band edge or the end of the keys crosses this tile for some row of the wave
        const bool need_hi = (k0 + BN - 1 > pos_w + wr) || (k0 + BN > nk);
        const bool need_lo = k0 < pos_w + 31 - wl;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            if (need_hi) {
                const int thr = lim_hi - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
            }
            if (need_lo) {
                const int thr = lim_lo - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) < thr) sacc[kb][i] = -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
        }
        mx = mx * fe;
        mx = fmaxf(mx, wave_half_swap(mx));
        const float m_new = fmaxf(m_run, mx);
        float m_use;
        if (__any(m_new - m_run > 8.0f) != 0) {   // lazy rescale (fwd_fp8in_kernel); a row's first visible key: inf > 8
            m_use = m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int t2 = 0; t2 < NDV; ++t2)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
        } else {
            m_use = m_run;
        }
        if (m_use == -INFINITY) m_use = 0.f;      // a row without a visible key so far: p = exp2(-inf) = 0, not exp2(-inf + inf)
        float rs = 0.f;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            i32x8_t pb;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int kb = 2 * g + kk;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], fe, -m_use));   // (-inf stays -inf: fe > 0)
                    sacc[kb][i] = p;
                    rs += p;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int wd = 0;
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 0], sacc[kb][4 * j + 1], wd, false);
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 2], sacc[kb][4 * j + 3], wd, true);
                    pb[4 * kk + j] = wd;
                }
            }
#pragma unroll
            for (int dvb = 0; dvb < NDV; ++dvb) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * g + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * g + 2 + h));
                const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], 0, 0, 0, 127, 0, 127);
            }
        }
        l_run += rs;
        }
        dma_wait_all();
        __syncthreads();
    }

    // every wave is past the last barrier: the K / V buffers are dead (fwd_fp8in_kernel's epilogue).  The sink joins here.
    const float l_tot = l_run + wave_half_swap(l_run);
    const float snk = am.sinks ? am.sinks[hd] : -INFINITY;   // (workgroup-uniform)
    bool dead;
    float inv, lse_v;
    if (snk != -INFINITY) {
        float iv;
        ex_sink_norm(m_run * 0.6931471805599453f, l_tot, snk, iv, lse_v);
        dead = false;                                    // (no visible key: iv = 0, lse = sink)
        inv = vd * iv;
    } else {
        dead = l_tot == 0.f;                             // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
        inv = vd * (1.f / l_tot);                        // v_descale once, with 1 / l
        lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    }
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
            vals[4 * dvb + g][0] = pack2_rn<Tag>(y[0], y[1]);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(y[2], y[3]);
        }
    store_rows_via_lds<D, true>(smem + w * 32 * D * 2, vals, obase, q0 + 32 * w, nq, lane, D, -1, o_ts);
    if (qrow < nq && h == 0) {
        if constexpr (VAR) am.var.lse[(size_t)hd * am.var.total_q + qs + qrow] = lse_v;
        else am.pad.lse[(size_t)bh * nq + qrow] = lse_v;
    }
}

static void fp8in_mod_fill(Fp8InModKernelArgs& a, const Fp8Mod& m, bool causal) {
    a.wl = m.window_left >= 0 ? (int)std::min<int64_t>(m.window_left, kWinNone) : kWinNone;
    a.wr = causal ? 0 : (m.window_right >= 0 ? (int)std::min<int64_t>(m.window_right, kWinNone) : kWinNone);
    a.rev = causal;
    a.cap_k = m.softcap > 0.0 ? (float)(2.0 / m.softcap) : 0.f;
    a.cap2 = m.softcap > 0.0 ? (float)(m.softcap * 1.4426950408889634) : 0.f;
    a.sinks = m.sinks;
}

template <int MODE> static hipError_t launch_fp8in_mod(const Fp8InModKernelArgs& a, int dtype, unsigned grid, hipStream_t st) {
    const size_t smem = 2 * 2 * 128 * 128;
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e2 = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), smem, st, a);
        return hipGetLastError();
    };
    return dtype == 2 ? launch(fwd_fp8in_mod_kernel<bf16_tag, MODE>) : launch(fwd_fp8in_mod_kernel<f16_tag, MODE>);
}

hipError_t launch_fp8_inputs_mod(const Fp8InArgs& c, const Fp8Mod& m, hipStream_t st) {
    if (!m.any()) return launch_fp8_inputs(c, st);       // the parent call, launch for launch
    const hipError_t e = fp8in_launch_vt(c, st);
    if (e != hipSuccess) return e;
    Fp8InModKernelArgs a{};
    a.pad = fp8in_kernel_args(c);
    fp8in_mod_fill(a, m, c.causal != 0);
    route_hit(ROUTE_FP8IN_FWD_MOD);
    ProfScope ps(K_FP8IN_FWD_MOD, st);
    return launch_fp8in_mod<0>(a, c.dtype, (unsigned)(c.batch * c.heads_q * a.pad.nqt), st);
}

hipError_t launch_fp8_inputs_varlen_mod(const Fp8InVarArgs& c, const Fp8Mod& m, hipStream_t st) {
    if (!m.any()) return launch_fp8_inputs_varlen(c, st);
    if (c.max_q == 0) return hipSuccess;                 // no sequence has a query: nothing is written
    Fp8InModKernelArgs a{};
    const hipError_t e = c.block_table ? fp8in_varlen_front<true>(c, st, a.var) : fp8in_varlen_front<false>(c, st, a.var);
    if (e != hipSuccess) return e;
    fp8in_mod_fill(a, m, c.causal != 0);
    route_hit(ROUTE_FP8IN_FWD_VARLEN_MOD);
    ProfScope ps(K_FP8IN_FWD_VARLEN_MOD, st);
    const unsigned grid = (unsigned)(c.batch * c.heads_q * a.var.nqt);
    return c.block_table ? launch_fp8in_mod<2>(a, c.dtype, grid, st) : launch_fp8in_mod<1>(a, c.dtype, grid, st);
}

// ---- Head dims 64 and 256 (fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim) --------------------------------
// Every call at d = 64 / 256, with or without a window, a softcap or sinks, runs fwd_fp8in_hdim_kernel<Tag, MODE, D>:
// fwd_fp8in_mod_kernel's text (DUPLICATED rather than given a head-dim parameter: as one template its d = 128 instantiation kept
// its instructions but not their order, and d = 128 runs the code it ran) with NM = NDV = D / 32 fragments and accumulators, D / 64 score instructions a 32-key block in ascending head-dim order,
// a K tile of 128 rows of D bytes (TileSwz<D / 2> and the LDS-DMA geometry of a 16-bit tile of D / 2 elements) and a V^T tile of D
// rows of 128 key bytes, in which the key permutation of a row is what it is at 128.  Two buffers of both are 32 KiB at 64 and
// 128 KiB at 256: one workgroup a CU there, which the registers ask for as well (eight waves a workgroup are two a SIMD, 256
// registers each).  At 256 the 128 output accumulators, 64 score accumulators and 32 q registers do not fit them (68 bytes of
// scratch), so the softmax step is a 64-key half of the staged tile (KBS = 2: 32 score accumulators, no scratch); the
// arithmetic is that of a 64-key tile (profiles/fp8_hdim.md has the register report of both choices).
// The transposer is one kernel for the three forms: fp8in_vt_kernel's / fp8in_vt_varlen_kernel's loads and key permutation, D
// rows in LDS, and the block's D x 64 bytes leave as 4 D 16-byte chunks over the 256 threads.
template <typename Tag, int MODE, int D>
__global__ __launch_bounds__(512, 2) void fwd_fp8in_hdim_kernel(const Fp8InModKernelArgs am) {
    constexpr bool VAR = MODE != 0, PAGED = MODE == 2;
    constexpr int BM = 256, BN = 128, KB = 4, NM = D / 32, NDV = D / 32;
    constexpr int KBS = D == 256 ? 2 : KB, BNS = 32 * KBS;   // key blocks and keys of a softmax step
    constexpr int TILE = BN * D;                         // bytes of a K tile and of a V^T tile alike
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K8 tile | V8^T tile]
    typedef int i32x8_t __attribute__((ext_vector_type(8)));

    // ---- the sequence and its tensors: fwd_fp8in_kernel's (MODE 0) or fwd_fp8in_varlen_kernel's prologue
    const int nqt = VAR ? am.var.nqt : am.pad.nqt, hq = VAR ? am.var.hq : am.pad.hq, group = VAR ? am.var.group : am.pad.group;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;                              // b * H_q + head
    int qt = L - bh * nqt;
    if (am.rev) qt = nqt - 1 - qt;
    const int b = bh / hq, hd = bh - b * hq, hk = hd / group;
    const int q0 = qt * BM;
    int nq, nk, qs = 0, ks = 0;
    if constexpr (VAR) {
        seq_span(am.var.cu_q, b, am.var.total_q, am.var.max_q, qs, nq);
        if (PAGED) nk = paged_len(am.var.cu_k, b, am.var.max_k);
        else seq_span(am.var.cu_k, b, am.var.total_k, am.var.max_k, ks, nk);
        if (q0 >= nq) return;                            // the padded grid: no row of this tile belongs to the sequence
    } else {
        nq = am.pad.nq; nk = am.pad.nk;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int qrow = q0 + 32 * w + r;
    const int shift = nk - nq;                           // row i sits at key position i + shift
    const int q_ts = VAR ? am.var.q_ts : am.pad.q_ts, k_ts = VAR ? am.var.k_ts : am.pad.k_ts, o_ts = VAR ? am.var.o_ts : am.pad.o_ts;
    const uint8_t* qbase;
    const uint8_t* kh;                                   // the K rows of this K/V head (PAGED: of page 0)
    const uint8_t* vbase;
    uint16_t* obase;
    const float *qds, *kds, *vds;
    int qds_bs, kds_bs, vds_bs, ntile_b;
    if constexpr (VAR) {
        qbase = am.var.q + (size_t)qs * q_ts + (size_t)hd * am.var.q_hs;
        kh = am.var.k + (size_t)hk * am.var.k_hs + (PAGED ? (size_t)0 : (size_t)ks * k_ts);
        ntile_b = (nk + BN - 1) / BN;
        vbase = am.var.v8t + ((size_t)hk * am.var.nt_head + fp8in_tile_start<PAGED>(b, ks, am.var.nt_seq)) * TILE;
        obase = am.var.o + (size_t)qs * o_ts + (size_t)hd * am.var.o_hs;
        qds = am.var.qds; kds = am.var.kds; vds = am.var.vds;
        qds_bs = am.var.qds_bs; kds_bs = am.var.kds_bs; vds_bs = am.var.vds_bs;
    } else {
        qbase = am.pad.q + (size_t)b * am.pad.q_bs + (size_t)hd * am.pad.q_hs;
        kh = am.pad.k + (size_t)b * am.pad.k_bs + (size_t)hk * am.pad.k_hs;
        ntile_b = am.pad.ntile;
        vbase = am.pad.v8t + (size_t)(b * am.pad.hkv + hk) * am.pad.ntile * TILE;
        obase = am.pad.o + (size_t)b * am.pad.o_bs + (size_t)hd * am.pad.o_hs;
        qds = am.pad.qds; kds = am.pad.kds; vds = am.pad.vds;
        qds_bs = am.pad.qds_bs; kds_bs = am.pad.kds_bs; vds_bs = am.pad.vds_bs;
    }

    // q rows >= nq and k rows >= nk lie outside the descriptors: they read as zeros, whatever the memory behind them holds
    const buf_rsrc_t q_rs = make_rsrc(qbase, (unsigned)(nq - 1) * (unsigned)q_ts + D);
    u32x4 qf[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) qf[m] = __builtin_amdgcn_raw_buffer_load_b128(q_rs, qrow * q_ts + 32 * m + 16 * h, 0, 0);
    const float qd = qds ? qds[(size_t)b * qds_bs + hk] : 1.f;
    const float kd = kds ? kds[(size_t)b * kds_bs + hk] : 1.f;
    const float vd = vds ? vds[(size_t)b * vds_bs + hk] : 1.f;
    const float f = ((VAR ? am.var.c_log2 : am.pad.c_log2) * qd) * kd;   // the one score factor of this workgroup, > 0
    const bool capped = am.cap2 != 0.f;
    const float ck = f * am.cap_k, cap2 = am.cap2;
    const float fe = capped ? 1.f : f;                   // the factor of what the accumulators hold after the cap

    // the 128-key tiles [t_lo, t_hi) some row of the workgroup sees, from its first row's lower and its last row's upper bound
    const int wl = am.wl, wr = am.wr;
    const int kfirst = max(0, q0 + shift - wl), kend = max(0, min(nk, q0 + BM + shift + wr));
    const int t_lo = kfirst / BN, t_hi = kend > kfirst ? (kend + BN - 1) / BN : t_lo;
    [[maybe_unused]] const rsrc_s_t k_rs = make_rsrc_s(kh, nk > 0 ? (unsigned)(nk - 1) * (unsigned)k_ts + D : 0u);
    const rsrc_s_t v_rs = make_rsrc_s(vbase, (unsigned)ntile_b * TILE);
    const int kstride = k_ts >> 1;                       // the STRIDED helpers count 2-byte elements
    const int voff_k = dma_lane_voff<D / 2, true>(lane, w, D / 2, kstride);   // D-byte rows: the geometry of a 16-bit d = D / 2 tile
    const int voff_v = dma_lane_voff<64>(lane, w);
    [[maybe_unused]] const int* trow = PAGED ? am.var.pg.table + (size_t)b * am.var.pg.max_blocks : nullptr;
    [[maybe_unused]] const int pg_last = PAGED ? pg_slot(am.var.pg, max(nk - 1, 0)) : 0;   // no entry past ceil(nk / ps) is read
    auto stage = [&](int buf, int t) {
        char* b_ = smem + buf * 2 * TILE;
        if constexpr (PAGED) {
            fp8in_stage_k_paged<D>(am.var.pg, trow, pg_last, kh, b_, t * BN, nk, voff_k, w, k_ts);
        } else {
            dma_stage_tile<D / 2, BN, 8, true>(k_rs, b_, t * BN, voff_k, w, D / 2, 0, kstride);
        }
        dma_stage_tile<64, D, 8>(v_rs, b_ + TILE, t * D, voff_v, w);   // V^T tile t = rows D t .. of the [tile][d row] matrix
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                // running max in log2 units of the (capped) scaled score

    if (t_hi > t_lo) {
        stage(0, t_lo);
        dma_wait_all();
        __syncthreads();
    }
    // the tiles some row of the wave sees: its first row's lower bound, its last row's upper bound
    const int pos_w = q0 + 32 * w + shift;               // the position of the wave's first row
    const int last_w = pos_w + 31 + wr;
    const int tw_lo = max(t_lo, max(0, pos_w - wl) / BN), tw_hi = last_w < 0 ? t_lo : min(t_hi, last_w / BN + 1);
    const int lim_hi = min(qrow + shift + wr, nk - 1), lim_lo = qrow + shift - wl;   // this row sees keys [lim_lo, lim_hi]

    for (int t = t_lo; t < t_hi; ++t) {
        const int k0 = t * BN, cur = (t - t_lo) & 1;
        if (t + 1 < t_hi) stage(cur ^ 1, t + 1);
        if (t >= tw_lo && t < tw_hi) {                   // (wave-uniform)
        const char* Kt = smem + cur * 2 * TILE;
        const char* Vt = Kt + TILE;
        // the softmax step: the whole staged tile (KBS = KB, one trip), at D = 256 its two 64-key halves one after the other
        // (kept a loop: unrolled, hipcc hoists the second half's operand reads over the first and spills 448 bytes)
#pragma nounroll
        for (int sub = 0; sub < KB / KBS; ++sub) {
        const int kbo = KBS * sub, k0s = k0 + 32 * kbo;  // the step's first key block and first key
        f32x16 sacc[KBS];
#pragma unroll
        for (int kb = 0; kb < KBS; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int M = 0; M < NM / 2; ++M) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<D / 2>::off(32 * (kbo + kb) + r, 4 * M + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Kt + TileSwz<D / 2>::off(32 * (kbo + kb) + r, 4 * M + 2 + h));
                const i32x8_t ka = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                const u32x4 b0_ = qf[2 * M], b1_ = qf[2 * M + 1];
                const i32x8_t qb = {(int)b0_[0], (int)b0_[1], (int)b0_[2], (int)b0_[3], (int)b1_[0], (int)b1_[1], (int)b1_[2], (int)b1_[3]};
                sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb, sacc[kb], 0, 0, 0, 127, 0, 127);
            }
        }
        // the softcap first (before the mask), in log2 units: one exp2 and one rcp an element
        if (capped) {
#pragma unroll
            for (int kb = 0; kb < KBS; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * ck) + 1.f);
                    sacc[kb][i] = fmaf(rr, -2.f * cap2, cap2);
                }
        }
        // the mask, only where a band edge or the end of the keys crosses this tile for some row of the wave
        const bool need_hi = (k0s + BNS - 1 > pos_w + wr) || (k0s + BNS > nk);
        const bool need_lo = k0s < pos_w + 31 - wl;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KBS; ++kb) {
            if (need_hi) {
                const int thr = lim_hi - (k0s + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
            }
            if (need_lo) {
                const int thr = lim_lo - (k0s + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) < thr) sacc[kb][i] = -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
        }
        mx = mx * fe;
        mx = fmaxf(mx, wave_half_swap(mx));
        const float m_new = fmaxf(m_run, mx);
        float m_use;
        if (__any(m_new - m_run > 8.0f) != 0) {   // lazy rescale (fwd_fp8in_kernel); a row's first visible key: inf > 8
            m_use = m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int t2 = 0; t2 < NDV; ++t2)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
        } else {
            m_use = m_run;
        }
        if (m_use == -INFINITY) m_use = 0.f;      // a row without a visible key so far: p = exp2(-inf) = 0, not exp2(-inf + inf)
        float rs = 0.f;
#pragma unroll
        for (int g = 0; g < KBS / 2; ++g) {
            const int gt = kbo / 2 + g;                  // the 64-key group of the staged tile
            i32x8_t pb;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int kb = 2 * g + kk;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], fe, -m_use));   // (-inf stays -inf: fe > 0)
                    sacc[kb][i] = p;
                    rs += p;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int wd = 0;
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 0], sacc[kb][4 * j + 1], wd, false);
                    wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 2], sacc[kb][4 * j + 3], wd, true);
                    pb[4 * kk + j] = wd;
                }
            }
#pragma unroll
            for (int dvb = 0; dvb < NDV; ++dvb) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * gt + h));
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(Vt + TileSwz<64>::off(32 * dvb + r, 4 * gt + 2 + h));
                const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
                oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], 0, 0, 0, 127, 0, 127);
            }
        }
        l_run += rs;
        }
        }
        dma_wait_all();
        __syncthreads();
    }

    // every wave is past the last barrier: the K / V buffers are dead (fwd_fp8in_mod_kernel's epilogue).  The sink joins here.
    const float l_tot = l_run + wave_half_swap(l_run);
    const float snk = am.sinks ? am.sinks[hd] : -INFINITY;   // (workgroup-uniform)
    bool dead;
    float inv, lse_v;
    if (snk != -INFINITY) {
        float iv;
        ex_sink_norm(m_run * 0.6931471805599453f, l_tot, snk, iv, lse_v);
        dead = false;                                    // (no visible key: iv = 0, lse = sink)
        inv = vd * iv;
    } else {
        dead = l_tot == 0.f;                             // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
        inv = vd * (1.f / l_tot);                        // v_descale once, with 1 / l
        lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    }
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
            vals[4 * dvb + g][0] = pack2_rn<Tag>(y[0], y[1]);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(y[2], y[3]);
        }
    store_rows_via_lds<D, true>(smem + w * 32 * D * 2, vals, obase, q0 + 32 * w, nq, lane, D, -1, o_ts);
    if (qrow < nq && h == 0) {
        if constexpr (VAR) am.var.lse[(size_t)hd * am.var.total_q + qs + qrow] = lse_v;
        else am.pad.lse[(size_t)bh * nq + qrow] = lse_v;
    }
}

template <int MODE, int D>
static hipError_t launch_fp8in_hdim(const Fp8InModKernelArgs& a, int dtype, unsigned grid, hipStream_t st) {
    const size_t smem = 2 * 2 * 128 * D;
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e2 = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), smem, st, a);
        return hipGetLastError();
    };
    return dtype == 2 ? launch(fwd_fp8in_hdim_kernel<bf16_tag, MODE, D>) : launch(fwd_fp8in_hdim_kernel<f16_tag, MODE, D>);
}

template <int D, int MODE>
__global__ __launch_bounds__(256) void fp8in_vt_hdim_kernel(const Fp8InVtArgs a) {
    constexpr bool VAR = MODE != 0, PAGED = MODE == 2;
    constexpr int CPR = D / 16, PER = (64 * CPR) / 256;   // 16-byte chunks per row / per thread
    __shared__ __attribute__((aligned(16))) uint8_t tr[D * 64];   // [d row][permuted key position]
    const int unit = blockIdx.x / a.nb, blk = blockIdx.x - unit * a.nb, row0 = blk * 64;
    const int b = unit / a.hkv, hk = unit - b * a.hkv;
    int ks = 0, nk = a.nk;
    if constexpr (VAR) {
        if (PAGED) nk = paged_len(a.cu_k, b, a.max_k);
        else seq_span(a.cu_k, b, a.total_k, a.max_k, ks, nk);
    }
    const int nb = (nk + 63) >> 6;
    if (blk >= nb) return;                               // (the padded grid of the packed and the paged form)
    const uint8_t* src = a.v + (size_t)hk * a.v_hs + (VAR ? (PAGED ? (size_t)0 : (size_t)ks * a.v_ts) : (size_t)b * a.v_bs);
    [[maybe_unused]] const int* trow = PAGED ? a.pg.table + (size_t)b * a.pg.max_blocks : nullptr;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = threadIdx.x + 256 * i, key = c / CPR, ch = c % CPR;   // key within the 64-key block
        u32x4 x = u32x4{0u, 0u, 0u, 0u};
        if (row0 + key < nk) {
            if constexpr (PAGED) {
                // a 16-key group never straddles a page (ps % 16 == 0), and key < nk keeps the slot below ceil(nk / ps)
                const int slot = pg_slot(a.pg, row0 + key), page = trow[slot];
                if ((unsigned)page < (unsigned)a.pg.num_blocks)
                    x = *reinterpret_cast<const u32x4*>(src + (size_t)page * a.pg.vps + (size_t)(row0 + key - slot * a.pg.ps) * a.v_ts + 16 * ch);
            } else {
                x = *reinterpret_cast<const u32x4*>(src + (size_t)(row0 + key) * a.v_ts + 16 * ch);
            }
        }
        const int wlo = key & 31, pos = 32 * (key >> 5) + 16 * ((wlo >> 2) & 1) + (wlo & 3) + 4 * (wlo >> 3);
#pragma unroll
        for (int j = 0; j < 16; ++j) tr[(16 * ch + j) * 64 + pos] = (uint8_t)((x[j >> 2] >> (8 * (j & 3))) & 0xff);
    }
    __syncthreads();
    const size_t tile = VAR ? (size_t)hk * a.nt_head + fp8in_tile_start<PAGED>(b, ks, a.nt_seq) + (blk >> 1)
                            : (size_t)unit * a.ntile + (blk >> 1);
#pragma unroll
    for (int i = 0; i < D / 64; ++i) {
        const int c = threadIdx.x + 256 * i, r = c >> 2, q4 = c & 3;   // d row r, 16-byte quarter q4 of its 64 key bytes
        uint8_t* dst = a.v8t + (tile * D + r) * 128 + 64 * (blk & 1) + 16 * q4;
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(tr + r * 64 + 16 * q4);
        // an odd block count leaves the second half of the last tile unwritten by any block: zero it (those keys lie past nk)
        if ((nb & 1) && blk == nb - 1) *reinterpret_cast<u32x4*>(dst + 64) = u32x4{0u, 0u, 0u, 0u};
    }
}

static Fp8InVtArgs fp8in_vt_hdim_args(const Fp8InVarArgs& c, const ExPage& pg, int cap, int nbmax, int nt_head, int nt_seq) {
    Fp8InVtArgs a{};
    a.v = (const uint8_t*)c.v; a.v8t = (uint8_t*)c.workspace; a.cu_k = c.cu_k;
    a.total_k = (int)c.total_k; a.max_k = cap; a.nb = nbmax; a.nt_head = nt_head; a.nt_seq = nt_seq; a.hkv = (int)c.heads_kv;
    a.v_hs = c.v_hs; a.v_ts = c.v_ts; a.pg = pg;
    return a;
}

template <int MODE> static hipError_t fp8in_launch_vt_hdim(const Fp8InVtArgs& a, int d, unsigned grid, hipStream_t st) {
    ProfScope ps(MODE == 0 ? K_FP8IN_VT : K_FP8IN_VT_VARLEN, st);
    if (d == 64) hipLaunchKernelGGL((fp8in_vt_hdim_kernel<64, MODE>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((fp8in_vt_hdim_kernel<256, MODE>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fp8_inputs_hdim(const Fp8InArgs& c, const Fp8Mod& m, hipStream_t st) {
    if (c.d == 128) return launch_fp8_inputs_mod(c, m, st);   // the parent call, launch for launch
    const int nb = (int)((c.nk + 63) / 64);
    Fp8InVtArgs v{};
    v.v = (const uint8_t*)c.v; v.v8t = (uint8_t*)c.workspace;
    v.nk = (int)c.nk; v.nb = nb; v.ntile = (int)((c.nk + 127) / 128); v.hkv = (int)c.heads_kv;
    v.v_bs = c.v_bs; v.v_hs = c.v_hs; v.v_ts = c.v_ts;
    const hipError_t e = fp8in_launch_vt_hdim<0>(v, (int)c.d, (unsigned)(c.batch * c.heads_kv * nb), st);
    if (e != hipSuccess) return e;
    Fp8InModKernelArgs a{};
    a.pad = fp8in_kernel_args(c);
    fp8in_mod_fill(a, m, c.causal != 0);
    route_hit(ROUTE_FP8IN_FWD_HDIM);
    ProfScope ps(K_FP8IN_FWD_HDIM, st);
    const unsigned grid = (unsigned)(c.batch * c.heads_q * a.pad.nqt);
    return c.d == 64 ? launch_fp8in_hdim<0, 64>(a, c.dtype, grid, st) : launch_fp8in_hdim<0, 256>(a, c.dtype, grid, st);
}

hipError_t launch_fp8_inputs_varlen_hdim(const Fp8InVarArgs& c, const Fp8Mod& m, hipStream_t st) {
    if (c.d == 128) return launch_fp8_inputs_varlen_mod(c, m, st);
    if (c.max_q == 0) return hipSuccess;                 // no sequence has a query: nothing is written
    Fp8InModKernelArgs a{};
    const hipError_t e = c.block_table ? fp8in_varlen_front<true>(c, st, a.var) : fp8in_varlen_front<false>(c, st, a.var);
    if (e != hipSuccess) return e;
    fp8in_mod_fill(a, m, c.causal != 0);
    route_hit(ROUTE_FP8IN_FWD_VARLEN_HDIM);
    ProfScope ps(K_FP8IN_FWD_VARLEN_HDIM, st);
    const unsigned grid = (unsigned)(c.batch * c.heads_q * a.var.nqt);
    if (c.d == 64) return c.block_table ? launch_fp8in_hdim<2, 64>(a, c.dtype, grid, st) : launch_fp8in_hdim<1, 64>(a, c.dtype, grid, st);
    return c.block_table ? launch_fp8in_hdim<2, 256>(a, c.dtype, grid, st) : launch_fp8in_hdim<1, 256>(a, c.dtype, grid, st);
}

}  // namespace fa
