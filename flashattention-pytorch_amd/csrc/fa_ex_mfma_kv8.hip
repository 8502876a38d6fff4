// The paged varlen forward of fa_ex_mfma.hip on an e4m3 pool (fa_ex_forward_varlen_paged_fp8): FEAT bit 7, kFeatKv8, always with
// bits 3 (varlen) and 6 (paged), never with bits 0 and 1 (mask, dropout).  k and v address OCP e4m3 bytes, strides are bytes, and
// the parameter block grows by the two scale pointers (ExKv8, ExParamsPg8).  Only how a K/V tile reaches LDS differs from
// exm_fwd_paged_kernel: the pool's bytes come by LDS-DMA into a staging area behind the two tile buffers (dma_stage_kv_paged8: a
// block of 16 keys per wave, dword granularity) and at the tile boundary every wave widens its own block into the 16-bit TileSwz
// image (kv8_widen_block; exact), so the loop — ds_read_b128 of K, lds_tr16 of V, the S and P V MFMAs, the softmax — is the text
// of fa_ex_mfma_fwd.inc without its mask and dropout branches and reads what it reads from a 16-bit pool.  k_descale joins the
// constants that carry softmax_scale, v_descale the epilogue's normaliser.
// A translation unit of its own: hipcc allocates the registers of a kernel differently when other kernels join its module, and
// the kernels of fa_ex_mfma.hip are to stay the instructions they were.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_ex_mfma_feat.h"
#include "fa_kernels.h"

namespace fa {

template <typename Tag, int D, int FEAT>
__global__ __launch_bounds__(512, 2) void exm_fwd_paged_kv8_kernel(const uint16_t* __restrict__ q, const uint8_t* __restrict__ k,
                                                                   const uint8_t* __restrict__ v, uint16_t* __restrict__ o,
                                                                   float* __restrict__ lse, ExParamsPg8<ExP<FEAT>> p, float c_log2) {
    static_assert((FEAT & (kFeatVarlen | kFeatPaged | kFeatKv8)) == (kFeatVarlen | kFeatPaged | kFeatKv8), "an e4m3 pool is paged and varlen");
    constexpr int NW = 8, BM = 32 * NW, KB = 4, BN = 32 * KB, NKS = D / 16, NDV = D / 32, TILE_BYTES = BN * D * 2;
    constexpr bool WIN = (FEAT & kFeatWindow) != 0, SC = (FEAT & kFeatScore) != 0, SNK = (FEAT & kFeatSink) != 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K tile | V tile], then [K | V] e4m3 bytes of one tile
    char* const kstage = smem + 4 * TILE_BYTES;
    char* const vstage = kstage + BN * D;
    const int DR = p.d;
    int nq = p.nq, nk = p.nk;
    const int nqt = (nq + BM - 1) / BM;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;
    const int q0 = (L - bh * nqt) * BM;
    // the workgroup's sequence b (the table row) and heads; it leaves before its first barrier when its tile starts past the sequence
    const int b = bh / p.hq, hh = bh - b * p.hq, hk = kv_unit(hh, p.kvg);
    int sq0;
    {
        int lq;
        seq_span(p.cu_q, b, p.total_q, nq, sq0, lq);
        nk = paged_len(p.cu_k, b, nk);
        nq = lq; p.coff = nk - lq;
        if (q0 >= nq) return;
    }
    // the scales of (sequence, K/V head), one scalar load each.  k_descale multiplies the score, so it joins every constant that
    // carries softmax_scale or its reciprocal: fp32 multiplications or divisions, exact for a power of two, the identity for 1.0
    const float kdsc = kv8_scale(p.q8.kd, p.q8.bs, b, hk), vdsc = kv8_scale(p.q8.vd, p.q8.bs, b, hk);
    p.scale *= kdsc;
    c_log2 *= kdsc;
    if constexpr (SC) {
        p.sc.cap_k *= kdsc;
        p.sc.cap_a /= kdsc;
        p.sc.al_k /= kdsc;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const size_t qbase = (size_t)sq0 * p.sq + hh * DR;
    const int qrow = q0 + 32 * w + r;

    const buf_rsrc_t q_rs = make_rsrc(q + qbase, span_bytes(nq, DR, p.sq));
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = buf_load_frag(q_rs, frag_off<true>(qrow, 16 * ks + 8 * h, DR, true, p.sq));

    const int dma_voff = dma_lane_voff8<D>(lane, DR, p.sk), dma_voff_v = dma_lane_voff8<D>(lane, DR, p.sv);
    const int* pg_row = p.pg.table + (size_t)b * p.pg.max_blocks;   // this sequence's table row and its last slot in use
    const int pg_last = pg_slot(p.pg, max(nk, 1) - 1);
    // (every tile goes through the one staging area: `land` empties it before the next is staged)
    auto stage = [&](int k0) {
        dma_stage_kv_paged8<D, BN, NW>(p.pg, pg_row, pg_last, reinterpret_cast<const char*>(k) + hk * DR, reinterpret_cast<const char*>(v) + hk * DR,
                                       kstage, vstage, k0, nk, dma_voff, dma_voff_v, w, DR, p.sk, p.sv);
    };
    // the staged tile arrives in buffer `buf` for every wave.  `fresh` (uniform over the workgroup): a tile was staged since the
    // last call.  Its bytes are in the staging area, and LDS-DMA data is ordered for a ds_read only by the issuing wave's vmcnt and
    // a barrier the reader has passed, its own wave included — so one more barrier, then every wave widens its block
    auto land = [&](int buf, bool fresh) {
        dma_wait_all();
        if (fresh) {
            __syncthreads();
            kv8_widen_block<Tag, D>(kstage, smem + buf * 2 * TILE_BYTES, w, lane);
            kv8_widen_block<Tag, D>(vstage, smem + buf * 2 * TILE_BYTES + TILE_BYTES, w, lane);
        }
        __syncthreads();
    };
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = ex_slope(p.sc, bh) * p.sc.al_k;
    [[maybe_unused]] float snk = -INFINITY;   // this unit's sink logit (kFeatSink): workgroup-uniform, one scalar load
    if constexpr (SNK) snk = ex_sink(p.snk, bh);

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // tiles [t_lo, ntiles) for the workgroup, [t_lo_w, ntiles_w) per wave (fa_ex_mfma_fwd.inc)
    const int kend = WIN ? max(0, min(nk, min(q0 + BM, nq) + p.coff + p.wr)) : (p.causal ? max(0, min(nk, q0 + BM + p.coff)) : nk);
    const int kend_w = WIN ? (q0 + 32 * w < nq ? max(0, min(nk, min(q0 + 32 * w + 32, nq) + p.coff + p.wr)) : 0)
                           : (p.causal ? max(0, min(nk, q0 + 32 * w + 32 + p.coff)) : nk);
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const int t_lo = WIN ? max(0, q0 + p.coff - p.wl) / BN : 0;
    const int t_lo_w = WIN ? max(0, q0 + 32 * w + p.coff - p.wl) / BN : 0;
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int t = t_lo, cur = 0;
    if (t < ntiles) stage(t * BN);
    land(0, t < ntiles);
    if constexpr (WIN) {
        // leading feed-only tiles: left of this wave's band, inside the workgroup's
        while (t < min(t_lo_w, ntiles)) {
            const int tn = t + 1;
            if (tn < ntiles) stage(tn * BN);
            land(cur ^ 1, tn < ntiles);
            cur ^= 1;
            t = tn;
        }
    }
    // two loops instead of an `if` inside one (a conditional accumulate makes hipcc carry the accumulators through
    // copies): tiles this wave computes, then the ones it only helps to load
    while (t < ntiles_w) {
        const int tn = t + 1;
        if (tn < ntiles) stage(tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * 2 * TILE_BYTES;
        const char* Vt = Kt + TILE_BYTES;
        {
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
                if (p.sc.cap_a > 0.f) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int i = 0; i < 16; ++i) { float dt; sacc[kb][i] = mod_softcap(sacc[kb][i], p.sc, dt); }
                }
                if (p.sc.alibi) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) {
                        const float fb = (float)(qrow + p.coff - (k0 + 32 * kb + 4 * h));   // dist of register i: fb - rc(i)
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[kb][i] = mod_alibi(sacc[kb][i], al, fb - (float)rc_of(i));
                    }
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
                    const float pe = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], c_log2, -mc));
                    rs += pe;
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
        }
        land(cur ^ 1, tn < ntiles);
        cur ^= 1;
        t = tn;
    }
    while (t < ntiles) {
        const int tn = t + 1;
        if (tn < ntiles) stage(tn * BN);
        land(cur ^ 1, tn < ntiles);
        cur ^= 1;
        t = tn;
    }

    // ---- epilogue: normalise, store O and lse.  Every wave is past the last barrier and nothing is in flight: each wave
    // stages its rows in 32 x D x 2 bytes of buffer 0
    const float l_tot = l_run + wave_half_swap(l_run);
    float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    float lse_k = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if constexpr (SNK) {   // the sink column (a head at -inf keeps the formulas of the call without sinks: the same bits)
        if (snk != -INFINITY) ex_sink_norm(l_tot > 0.f ? m_run * p.scale : -INFINITY, l_tot, snk, inv, lse_k);
    }
    // v_descale, once, in fp32, in front of the single rounding: with 1.0 the products below are the 16-bit kernel's
    const float invv = inv * vdsc;
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vals[4 * dvb + g][0] = pack2_rn<Tag>(oacc[dvb][4 * g + 0] * invv, oacc[dvb][4 * g + 1] * invv);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(oacc[dvb][4 * g + 2] * invv, oacc[dvb][4 * g + 3] * invv);
        }
    const size_t obase = ((size_t)sq0 * p.hq + hh) * DR;
    const size_t lbase = (size_t)hh * p.total_q + sq0;
    store_rows_via_lds<D, true>(smem + w * 32 * D * 2, vals, o + obase, q0 + 32 * w, nq, lane, DR, -1, p.hq * DR);
    if (qrow < nq && h == 0) lse[lbase + qrow] = lse_k;
}

// ------------------------------------------------------------------------------------------------ launch
// Dword DMA and 8-byte staging reads: what the C layer checked of the pools (8-byte alignment, strides % 8) will do; q and o as in
// ex_mfma_paged_supported
bool ex_mfma_paged_kv8_supported(const ExArgs& a) {
    if (!ex_mfma_supported(a) || a.dropout_p > 0.0) return false;
    if (a.stride_q % 8 != 0 || ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.o)) & 15) != 0) return false;
    if (a.stride_k % 4 != 0 || a.stride_v % 4 != 0 || a.page_stride_k % 4 != 0 || a.page_stride_v % 4 != 0) return false;
    if (((reinterpret_cast<uintptr_t>(a.k) | reinterpret_cast<uintptr_t>(a.v)) & 3) != 0) return false;
    const int64_t sq = a.stride_q > a.heads_q * a.d ? a.stride_q : a.heads_q * a.d;
    const int64_t skv = a.stride_k > a.stride_v ? a.stride_k : a.stride_v;
    // the 32-bit buffer offsets: inside one sequence of q and o, inside one block of 16 rows of a page (bytes)
    return a.nq * sq * 2 < ((int64_t)1 << 31) && 16 * skv < ((int64_t)1 << 31);
}

// two tile buffers and the staging area, half a buffer
template <typename Tag, int D, int FEAT>
static hipError_t exm_paged_kv8_fwd_t(const ExArgs& a, hipStream_t st) {
    ExParamsPg8<ExP<FEAT>> p;
    static_cast<ExP<FEAT>&>(p) = make_exm_params<FEAT>(a);
    p.pg = make_ex_page(a);
    p.q8 = make_ex_kv8(a);
    const size_t smem = 2 * 2 * 128 * D * 2 + 2 * 128 * D;
    auto kern = exm_fwd_paged_kv8_kernel<Tag, D, FEAT | kFeatVarlen | kFeatPaged | kFeatKv8>;
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)smem);
    if (e != hipSuccess) return e;
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nq + 255) / 256) * a.bh)), dim3(512), smem, st, (const uint16_t*)a.q,
                       (const uint8_t*)a.k, (const uint8_t*)a.v, (uint16_t*)a.o, a.lse, p, a.scale * 1.4426950408889634f);
    return hipGetLastError();
}
template <typename Tag, int D>
static hipError_t exm_paged_kv8_by_feat(const ExArgs& a, hipStream_t st) {
    const bool win = ex_windowed(a);
    if (a.sinks) return win ? exm_paged_kv8_fwd_t<Tag, D, kFeatScore | kFeatSink | kFeatWindow>(a, st) : exm_paged_kv8_fwd_t<Tag, D, kFeatScore | kFeatSink>(a, st);
    if (ex_scoremod(a)) return win ? exm_paged_kv8_fwd_t<Tag, D, kFeatScore | kFeatWindow>(a, st) : exm_paged_kv8_fwd_t<Tag, D, kFeatScore>(a, st);
    return win ? exm_paged_kv8_fwd_t<Tag, D, kFeatWindow>(a, st) : exm_paged_kv8_fwd_t<Tag, D, 0>(a, st);
}
// (the caller has checked ex_mfma_paged_kv8_supported, and that max_seqlen_q and the key cap are > 0)
hipError_t launch_ex_mfma_varlen_paged_kv8(const ExArgs& a, hipStream_t st) {
    if (a.dtype == 2) return a.d > 64 ? exm_paged_kv8_by_feat<bf16_tag, 128>(a, st) : exm_paged_kv8_by_feat<bf16_tag, 64>(a, st);
    return a.d > 64 ? exm_paged_kv8_by_feat<f16_tag, 128>(a, st) : exm_paged_kv8_by_feat<f16_tag, 64>(a, st);
}

}  // namespace fa
