// fp8 KV-cache decoding with split-KV for gfx950 (fa_fp8_forward_kvcache; include/fa_mi355x.h): q, k_cache
// and v_cache arrive in OCP e4m3 with one float32 descale per (batch, K/V head) for each of them, and both products run on
// v_mfma_scale_f32_32x32x64_f8f6f4 with unit hardware scales.  head_dim 128, o in f16 / bf16, lse float32.
//
//     o = softmax(softmax_scale * q_descale * k_descale * q8 k8^T [causal, bottom-right aligned]) (v8 * v_descale)
//
// Two launches on the caller's stream, the second for S > 1 only:
//   fp8kv_split_kernel<Tag, PAGED>  one wave per (split, row tile x K/V head, batch element), as kv_split_kernel (fa_decode.hip) maps:
//                       the G = H_q / H_kv query heads that share a K/V head, times the Nq query tokens, are packed into 32-row tiles
//                       (row = token * G + head in the group), and each wave reads its cache bytes exactly once.
//   kv_combine_kernel<Tag, false>   fa_decode.hip's combine, unchanged, over fp32 partials in kv_workspace_bytes' layout.
// fa_fp8_forward_kvcache_mod (a sliding window, a softcap, attention sinks) launches fp8kv_split_mod_kernel
// instead, and with sinks kv_combine_kernel<Tag, true>; a call without the three launches the two above as before.
// fa_fp8_forward_kvcache_varlen (packed queries, cu_seqlens_q) launches fp8kv_split_mod_kernel's packed
// instantiation (one more kernel argument, Fp8KvPacked) at every head dim, featured or not: sequence b owns the tokens kv_cu_range
// gives it, rows = G nq_b, and a wave whose row tile lies past them leaves before its first load; for S > 1 a memset of the lse
// partials (kPlseFill) and kv_combine_kernel in its packed mode, which leaves the rows that no sequence owns unwritten.
//
// One 64-key tile of a wave, lane l = (r = l & 31, h = l >> 5):
//   S^T = K Q^T     A = K as it lies in memory: key k0 + 32 kb + r, head-dim bytes 64 M + 32 h .. + 31 (two 16-byte loads), B = the
//                   same bytes of the lane's query row.  Accumulator register i of block kb is key k0 + 32 kb + 4 h + (i & 3) + 8 (i >> 2).
//   softmax         fwd_fp8in_kernel's (fa_fp8_inputs.hip): mask and row maximum on the RAW products, one factor per wave
//                   f = softmax_scale * log2(e) * q_descale * k_descale, p = exp2(fma(s, f, -m)) with the lazy rescale, P rounded to
//                   e4m3 (RNE) on every row, l from the unrounded p.
//   O^T = V^T P^T   B = P^T as the accumulators hold it: k = 32 h + 16 kb + 4 j + c is key 32 kb + 4 h + 8 j + c (fp8_ref._PV_KEY_OF_K).
//                   A = V^T in the same key order, TRANSPOSED ON CHIP: the lane loads the 4 bytes at head dims 4 r .. 4 r + 3 of the 16
//                   keys 32 kb + 4 h + 8 j + c (one dword each; 32 lanes cover a key's 128-byte row), turns each group of four keys
//                   (c = 0 .. 3) into four dwords of one head dim each with 8 v_perm_b32 (a 4 x 4 byte transpose), and writes head dim
//                   4 r + dd as one 16-byte LDS chunk (j = 0 .. 3) at row 4 r + dd, byte 32 h + 16 kb.  An LDS row is the 64 key bytes
//                   of one head dim; 16 bytes of padding after every four rows keep both the writes and the reads off each other's
//                   banks.  The A operand of d block dvb is then the lane's 32 contiguous bytes at row 32 dvb + r, byte 32 h.
//   v_descale enters once, in the epilogue, with 1 / l.  A row without a visible key gives o = 0, lse = -inf (l == 0).
//
// What is untrusted: cache_seqlens, block_table, cache_batch_idx, cu_seqlens_q and the descales are read on the device only.  len_b =
// clamp(cache_seqlens[b], 0, capacity); a cache_batch_idx outside [0, B_cache) makes the sequence empty; a page outside
// [0, num_blocks) reads as zero K and zero V and takes part with score 0; no table entry past ceil(len_b / ps) is read (a 16-key
// group never straddles a page, ps % 16 == 0, and a group is looked up only if its first key lies below the split's end).  Bytes
// of keys at or past the split's end are never loaded: K reads as zero there and its score is masked by a select, V reads as
// zero, so that p = 0 meets 0 and not a NaN code.
//
// Addressing: 64-bit bases per 16-key group (batch element or page, first token of the group), 32-bit offsets inside them.
// A tile that lies whole below the split's end on pages inside the pool takes a wave-uniform path without the per-lane selects and
// without the mask: with them on every tile the loads of a tile were not issued together (profiles/fp8_kvcache.md, 2.6 x the time).
#include <algorithm>

#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"
#include "fa_decode_common.h"   // kv_cu_range, kPlseFill: the packed calls

namespace fa {

namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef long long i64x4_t __attribute__((ext_vector_type(4)));   // four group bases, held as values (an array becomes an indexed scratch slot)

struct Fp8KvParams {
    const uint8_t *q, *kc, *vc;
    uint16_t* o;
    float *lse, *po, *plse;               // po / plse: the partials of S > 1 ((b, h_q, token)-major rows, then split)
    const float *qds, *kds, *vds;         // (B, H_kv) descales at their batch strides; null: 1
    long long qds_bs, kds_bs, vds_bs;
    const int *seqlens, *table, *bidx;    // untrusted device memory, or null
    long long tbl_rs;
    int nblk, ps, bcache;
    long long q_bs, kc_bs, vc_bs;         // batch (or page) strides in bytes
    int q_ts, kc_ts, vc_ts;               // token strides in bytes
    int hq, hkv, G, nq, cap, rows, causal;
    float c_log2;                         // float(softmax_scale) * log2(e)
};

// 4 x 4 byte transpose: x[c] holds bytes (d0, d1, d2, d3) of key c; t[dd] gets byte dd of keys 0 .. 3 (key 0 in the low byte).
// v_perm_b32 selects bytes 0 .. 3 from its second source and 4 .. 7 from its first.
__device__ __forceinline__ void transpose4x4(const uint32_t (&x)[4], uint32_t (&t)[4]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(x[1], x[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(x[1], x[0], 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(x[3], x[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(x[3], x[2], 0x07030602u);
    t[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    t[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    t[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// byte offset of 16-byte chunk ch of head-dim row `row` in the V^T image: 64-byte rows, 16 bytes of padding after every four
// Head dims 64 and 256 (fp8kv_split_mod_kernel<Tag, PAGED, D>) KEEP this padding rule: the image is D such
// rows, the d = 64 lanes write 8-byte halves of a chunk and the d = 256 lanes two rows 128 apart, both at the same row offsets.
constexpr int kVtRowBytes = 64 + 4;                      // a head dim's share of the image: D rows take kVtRowBytes * D bytes
constexpr int kVtBytes = kVtRowBytes * 128;
__device__ __forceinline__ int vt_off(int row, int ch) { return 64 * row + 16 * (row >> 2) + 16 * ch; }

template <typename Tag, bool PAGED>
__global__ __launch_bounds__(64, 2) void fp8kv_split_kernel(const Fp8KvParams p) {
    constexpr int D = 128, KT = 64, NDV = D / 32;
    __shared__ __attribute__((aligned(16))) char vt[kVtBytes];   // V^T tile, [head dim][64 key bytes in P's key order]
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int nq = p.nq, rows = p.rows, G = p.G;
    const int pr0 = 32 * rt, pr = pr0 + r;                        // (the grid has ceil(rows / 32) row tiles: pr0 < rows)

    // the sequence: its length, and the cache row its keys lie in (contiguous)
    int lk = p.seqlens ? min(max(p.seqlens[b], 0), p.cap) : p.cap;
    long long crow = b;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; lk = 0; }   // an index outside the cache: an empty sequence
    }
    const int coff = lk - nq;                                     // causal: token i sees key j <= i + coff
    const int qlo = pr0 / G, qhi = (min(pr0 + 32, rows) - 1) / G;
    // the split's keys [kbeg, kend): the tile's visible keys [0, hi) cut into 64-key tiles, tiles [s nt / S, (s + 1) nt / S)
    const int hi = p.causal ? max(0, min(lk, qhi + coff + 1)) : lk;
    const int nt = (hi + KT - 1) / KT;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    const int kbeg = t0 * KT, kend = min(hi, t1 * KT);

    // this lane's query row: token qi, query head hd; its last visible key rhi (padding rows of the tile: none)
    const bool valid = pr < rows;
    // (a padding row takes the tile's first token: its scores are masked like a real row's, and nothing of it is stored)
    const int qi = valid ? pr / G : qlo, hd = hk * G + (valid ? pr - qi * G : 0);
    const int rhi = min(p.causal ? qi + coff : lk - 1, kend - 1);

    i32x8_t qb[2];
    {
        const uint8_t* qp = p.q + (long long)b * p.q_bs + (long long)qi * p.q_ts + hd * D + 32 * h;
#pragma unroll
        for (int M = 0; M < 2; ++M) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(qp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(qp + 64 * M + 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qb[M][i] = valid ? (int)a0[i] : 0;
                qb[M][4 + i] = valid ? (int)a1[i] : 0;
            }
        }
    }
    const float qd = p.qds ? p.qds[b * p.qds_bs + hk] : 1.f;
    const float kd = p.kds ? p.kds[b * p.kds_bs + hk] : 1.f;
    const float vd = p.vds ? p.vds[b * p.vds_bs + hk] : 1.f;
    const float f = (p.c_log2 * qd) * kd;                         // the one score factor of this wave, > 0

    // byte offsets of the first token of the 16-key groups of the tile at k0 in the two caches, -1: the group reads as zeros
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    auto group_bases = [&](int k0, i64x4_t& kb_, i64x4_t& vb_) {
        int j0 = 0, s0 = 0;
        if (PAGED) { j0 = k0 / p.ps; s0 = k0 - j0 * p.ps; }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int key0 = k0 + 16 * g4;
            kb_[g4] = -1; vb_[g4] = -1;
            if (key0 < kend) {
                if (PAGED) {
                    int j = j0, sl = s0 + 16 * g4;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (sl >= p.ps) { sl -= p.ps; ++j; }
                    const int pg = tbl[j];
                    if ((unsigned)pg < (unsigned)p.nblk) {
                        kb_[g4] = pg * p.kc_bs + (long long)sl * p.kc_ts;
                        vb_[g4] = pg * p.vc_bs + (long long)sl * p.vc_ts;
                    }
                } else {
                    kb_[g4] = crow * p.kc_bs + (long long)key0 * p.kc_ts;
                    vb_[g4] = crow * p.vc_bs + (long long)key0 * p.vc_ts;
                }
            }
        }
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                         // running max in log2 units of the scaled score
    const uint8_t* nowhere = p.q;                                 // readable, for a load whose value is selected away

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        i64x4_t kbase, vbase;
        group_bases(k0, kbase, vbase);

        // a whole tile below the split's end on pages inside the pool: no lane needs a select on its addresses or its bytes
        // (wave-uniform; the general form below is the same text with them)
        const bool full = k0 + KT <= kend && kbase[0] >= 0 && kbase[1] >= 0 && kbase[2] >= 0 && kbase[3] >= 0;
        f32x16 sacc[2];
        auto front = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        // ---- S^T = K Q^T: K rows as they lie in memory
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const long long base_lo = kbase[2 * kb], base_hi = kbase[2 * kb + 1];
            const long long base = (r >> 4) ? base_hi : base_lo;
            const bool ok = FULL || (base >= 0 && k0 + 32 * kb + r < kend);
            const uint8_t* kp = ok ? p.kc + base + (r & 15) * p.kc_ts + hk * D + 32 * h : nowhere;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int M = 0; M < 2; ++M) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(kp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(kp + 64 * M + 16);
                i32x8_t ka;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ka[i] = ok ? (int)a0[i] : 0;
                    ka[4 + i] = ok ? (int)a1[i] : 0;
                }
                sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb[M], sacc[kb], 0, 0, 0, 127, 0, 127);
            }
        }

        // ---- V -> V^T through registers: 16 keys x 4 head dims a lane and key block, four 4 x 4 byte transposes, one 16-byte chunk
        // a head dim (the previous tile's operand reads were issued before these writes: one wave, LDS in order)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            uint32_t t[4][4];                                     // [j][dd]: head dim 4 r + dd of keys 32 kb + 4 h + 8 j + (0 .. 3)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long base = vbase[2 * kb + (j >> 1)];  // wave-uniform
                uint32_t x[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int pos = 4 * h + 8 * (j & 1) + c;      // the key's place in its 16-key group
                    const bool ok = FULL || (base >= 0 && k0 + 32 * kb + 16 * (j >> 1) + pos < kend);
                    const uint8_t* vp = ok ? p.vc + base + pos * p.vc_ts + hk * D + 4 * r : nowhere;
                    const uint32_t y = *reinterpret_cast<const uint32_t*>(vp);
                    x[c] = ok ? y : 0u;
                }
                transpose4x4(x, t[j]);
            }
#pragma unroll
            for (int dd = 0; dd < 4; ++dd)
                *reinterpret_cast<u32x4*>(vt + vt_off(4 * r + dd, 2 * h + kb)) = u32x4{t[0][dd], t[1][dd], t[2][dd], t[3][dd]};
        }
        };
        if (full) front(std::true_type{});
        else front(std::false_type{});

        // ---- mask and row maximum on the RAW products; f > 0 goes to the maximum once and to every element inside the exp2's fma
        // (the mask only where a row of the tile can end inside this key tile: wave-uniform)
        const bool need_mask = !full || (p.causal && k0 + KT - 1 > qlo + coff);
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (need_mask) {
                const int thr = rhi - (k0 + 32 * kb + 4 * h);
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
        if (__any(valid && m_new - m_run > 8.0f) != 0) {   // lazy rescale (fwd_fp8in_kernel) on the real rows; a row's first visible key: inf > 8
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
        i32x8_t pb;                               // P^T as the accumulators hold it, rounded to e4m3 (RNE)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float pe = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], f, -m_use));   // (-inf stays -inf: f > 0)
                sacc[kb][i] = pe;
                rs += pe;
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

        // ---- O^T = V^T P^T: the lane's 32 key bytes of head dim 32 dvb + r
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(vt + vt_off(32 * dvb + r, 2 * h));
            const u32x4 a1 = *reinterpret_cast<const u32x4*>(vt + vt_off(32 * dvb + r, 2 * h + 1));
            const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
            oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], 0, 0, 0, 127, 0, 127);
        }
    }

    // ---- epilogue: O^T register i of block dvb is head dim 32 dvb + 4 h + (i & 3) + 8 (i >> 2) of the lane's query row
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    const bool dead = l_tot == 0.f;                      // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
    const float inv = vd * (1.f / l_tot);                // v_descale once, with 1 / l
    const float lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    const size_t row_id = ((size_t)b * p.hq + hd) * nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + (((size_t)b * nq + qi) * p.hq + hd) * D;
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
        if (h == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * D;
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
                *reinterpret_cast<f32x4*>(prow + 32 * dvb + 8 * g + 4 * h) = y;
            }
        if (h == 0) p.plse[row_id * S + s] = lse_v;
    }
}


// What fp8kv_split_mod_kernel takes beside Fp8KvParams (fa_fp8_forward_kvcache_mod)
struct Fp8KvMod {
    int wl, wr;                           // token i sees keys [i + coff - wl, i + coff + wr]; kWinNone: unbounded, wr = 0 if causal
    float cap_k, cap2;                    // 2 / softcap, softcap * log2(e); cap2 == 0: no softcap
};

// fp8kv_split_kernel's text (DUPLICATED rather than shared: as one body with the features in discarded `if constexpr` branches
// fp8kv_split_kernel's instructions changed) with, as wave-uniform run-time switches:
//   window   the tile's keys are [lo, hi) with lo the first 64-key tile some row of the 32 sees, and the splits cut [lo, hi): no
//            table entry, K byte or V byte below lo is read.  The mask takes the row's lower bound beside its upper one on a
//            tile that bound crosses.
//   softcap  fwd_fp8in_mod_kernel's (fa_fp8_inputs.hip): the capped score, in log2 units, replaces the raw product before the
//            mask, and the factor of what follows is 1.
// Sinks are not this kernel's: they join in kv_combine_kernel<Tag, true>, once per row.
//
// PACKED (fa_fp8_forward_kvcache_varlen): the kernel takes one more argument, Packed = (Fp8KvPacked), and
// PACKED is "that argument is there" (an argument pack, as kv_combine_kernel's Sink: the padded instantiations keep their argument
// list, and with it their instructions).  q and o are (total_q, H_q, D), lse and the partials (H_q, total_q)-major; sequence b owns
// the nq_b tokens from tok0 that kv_cu_range gives it, and is the padded call on b alone: rows = G nq_b, coff = len_b - nq_b.  The
// grid is sized for max_seqlen_q; a wave whose row tile starts at or past rows leaves before its first load.  Wave-uniform scalars.
struct Fp8KvPacked {
    const int* cu_q;                      // (B + 1,) untrusted device offsets
    int total_q, max_q;
};

template <typename Tag, bool PAGED, int D = 128, typename... Packed>
__global__ __launch_bounds__(64, D == 256 ? 1 : 2) void fp8kv_split_mod_kernel(const Fp8KvParams p, const Fp8KvMod md, const Packed... pk) {
    constexpr bool PACKED = sizeof...(Packed) != 0;
    static_assert(sizeof...(Packed) <= 1, "PACKED: (Fp8KvPacked) follows");
    constexpr int KT = 64, NDV = D / 32, NMQ = D / 64;
    __shared__ __attribute__((aligned(16))) char vt[kVtRowBytes * D];   // V^T tile, [head dim][64 key bytes in P's key order]
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    int nq = p.nq, rows = p.rows;
    const int G = p.G;
    const int pr0 = 32 * rt, pr = pr0 + r;                        // (the grid has ceil(rows / 32) row tiles: pr0 < rows)
    [[maybe_unused]] long long tok0 = 0;                          // PACKED: the sequence's first token of q, o and lse
    [[maybe_unused]] int total_q = 0;
    if constexpr (PACKED) {
        const Fp8KvPacked& pq = (pk, ...);
        int st;
        nq = kv_cu_range(pq.cu_q, b, pq.total_q, pq.max_q, st);
        tok0 = st;
        total_q = pq.total_q;
        rows = G * nq;
        if (pr0 >= rows) return;                                  // (wave-uniform) a tile past the sequence's rows: nothing loaded, nothing stored
    }

    // the sequence: its length, and the cache row its keys lie in (contiguous)
    int lk = p.seqlens ? min(max(p.seqlens[b], 0), p.cap) : p.cap;
    long long crow = b;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; lk = 0; }   // an index outside the cache: an empty sequence
    }
    const int coff = lk - nq;                                     // causal: token i sees key j <= i + coff
    const int qlo = pr0 / G, qhi = (min(pr0 + 32, rows) - 1) / G;
    // the split's keys [kbeg, kend): the tile's visible keys [0, hi) cut into 64-key tiles, tiles [s nt / S, (s + 1) nt / S)
    const int hi = max(0, min(lk, qhi + coff + md.wr + 1));
    const int lo = max(0, qlo + coff - md.wl) & ~(KT - 1);       // the first 64-key tile some row sees (whole 16-key groups)
    const int nt = hi > lo ? (hi - lo + KT - 1) / KT : 0;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    const int kbeg = lo + t0 * KT, kend = min(hi, lo + t1 * KT);

    // this lane's query row: token qi, query head hd; its last visible key rhi (padding rows of the tile: none)
    const bool valid = pr < rows;
    // (a padding row takes the tile's first token: its scores are masked like a real row's, and nothing of it is stored)
    const int qi = valid ? pr / G : qlo, hd = hk * G + (valid ? pr - qi * G : 0);
    const int rhi = min(min(qi + coff + md.wr, lk - 1), kend - 1), rlo = qi + coff - md.wl;   // the row sees keys [rlo, rhi]

    i32x8_t qb[NMQ];
    {
        const uint8_t* qp = p.q + (PACKED ? tok0 * p.q_ts : (long long)b * p.q_bs) + (long long)qi * p.q_ts + hd * D + 32 * h;
#pragma unroll
        for (int M = 0; M < NMQ; ++M) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(qp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(qp + 64 * M + 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qb[M][i] = valid ? (int)a0[i] : 0;
                qb[M][4 + i] = valid ? (int)a1[i] : 0;
            }
        }
    }
    const float qd = p.qds ? p.qds[b * p.qds_bs + hk] : 1.f;
    const float kd = p.kds ? p.kds[b * p.kds_bs + hk] : 1.f;
    const float vd = p.vds ? p.vds[b * p.vds_bs + hk] : 1.f;
    const float f = (p.c_log2 * qd) * kd;                         // the one score factor of this wave, > 0
    const bool capped = md.cap2 != 0.f;
    const float ck = f * md.cap_k;
    const float fe = capped ? 1.f : f;                            // the factor of what the accumulators hold after the cap

    // byte offsets of the first token of the 16-key groups of the tile at k0 in the two caches, -1: the group reads as zeros
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    auto group_bases = [&](int k0, i64x4_t& kb_, i64x4_t& vb_) {
        int j0 = 0, s0 = 0;
        if (PAGED) { j0 = k0 / p.ps; s0 = k0 - j0 * p.ps; }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int key0 = k0 + 16 * g4;
            kb_[g4] = -1; vb_[g4] = -1;
            if (key0 < kend) {
                if (PAGED) {
                    int j = j0, sl = s0 + 16 * g4;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (sl >= p.ps) { sl -= p.ps; ++j; }
                    const int pg = tbl[j];
                    if ((unsigned)pg < (unsigned)p.nblk) {
                        kb_[g4] = pg * p.kc_bs + (long long)sl * p.kc_ts;
                        vb_[g4] = pg * p.vc_bs + (long long)sl * p.vc_ts;
                    }
                } else {
                    kb_[g4] = crow * p.kc_bs + (long long)key0 * p.kc_ts;
                    vb_[g4] = crow * p.vc_bs + (long long)key0 * p.vc_ts;
                }
            }
        }
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                         // running max in log2 units of the scaled score
    const uint8_t* nowhere = p.q;                                 // readable, for a load whose value is selected away

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        i64x4_t kbase, vbase;
        group_bases(k0, kbase, vbase);

        // a whole tile below the split's end on pages inside the pool: no lane needs a select on its addresses or its bytes
        // (wave-uniform; the general form below is the same text with them)
        const bool full = k0 + KT <= kend && kbase[0] >= 0 && kbase[1] >= 0 && kbase[2] >= 0 && kbase[3] >= 0;
        f32x16 sacc[2];
        auto front = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        // ---- S^T = K Q^T: K rows as they lie in memory
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const long long base_lo = kbase[2 * kb], base_hi = kbase[2 * kb + 1];
            const long long base = (r >> 4) ? base_hi : base_lo;
            const bool ok = FULL || (base >= 0 && k0 + 32 * kb + r < kend);
            const uint8_t* kp = ok ? p.kc + base + (r & 15) * p.kc_ts + hk * D + 32 * h : nowhere;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int M = 0; M < NMQ; ++M) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(kp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(kp + 64 * M + 16);
                i32x8_t ka;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ka[i] = ok ? (int)a0[i] : 0;
                    ka[4 + i] = ok ? (int)a1[i] : 0;
                }
                sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb[M], sacc[kb], 0, 0, 0, 127, 0, 127);
            }
        }

        // ---- V -> V^T through registers: 16 keys x 4 head dims a lane and key block, four 4 x 4 byte transposes, one 16-byte chunk
        // a head dim (the previous tile's operand reads were issued before these writes: one wave, LDS in order).
        // D = 256: 32 lanes cover half a key row, so a lane takes the dwords at head dims 4 r and 128 + 4 r (DW = 2 rounds).
        // D = 64: 16 lanes cover a key row; lane r takes head dims 4 (r & 15) of the key groups j = 2 (r >> 4), 2 (r >> 4) + 1
        // only, and writes that half (8 bytes) of the head dim's chunk: all 64 lanes load, no key byte twice.
        constexpr int DW = D == 256 ? 2 : 1, NJ = D == 64 ? 2 : 4;
        const int rd = D == 64 ? (r & 15) : r, j0 = D == 64 ? 2 * (r >> 4) : 0;
#pragma unroll
        for (int dw = 0; dw < DW; ++dw)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            uint32_t t[NJ][4];                                    // [j][dd]: head dim 128 dw + 4 rd + dd of keys 32 kb + 4 h + 8 (j0 + j) + (0 .. 3)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = j0 + jj;
                const long long base = D == 64 ? ((j >> 1) ? vbase[2 * kb + 1] : vbase[2 * kb]) : vbase[2 * kb + (jj >> 1)];   // (D != 64: wave-uniform)
                uint32_t x[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int pos = 4 * h + 8 * (j & 1) + c;      // the key's place in its 16-key group
                    const bool ok = FULL || (base >= 0 && k0 + 32 * kb + 16 * (j >> 1) + pos < kend);
                    const uint8_t* vp = ok ? p.vc + base + pos * p.vc_ts + hk * D + 128 * dw + 4 * rd : nowhere;
                    const uint32_t y = *reinterpret_cast<const uint32_t*>(vp);
                    x[c] = ok ? y : 0u;
                }
                transpose4x4(x, t[jj]);
            }
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                char* chunk = vt + vt_off(128 * dw + 4 * rd + dd, 2 * h + kb);
                if constexpr (D == 64) *reinterpret_cast<u32x2*>(chunk + 4 * j0) = u32x2{t[0][dd], t[1][dd]};
                else *reinterpret_cast<u32x4*>(chunk) = u32x4{t[0][dd], t[1][dd], t[2][dd], t[3][dd]};
            }
        }
        };
        if (full) front(std::true_type{});
        else front(std::false_type{});

        // ---- mask and row maximum on the RAW products; f > 0 goes to the maximum once and to every element inside the exp2's fma
        // (the mask only where a row of the tile can end inside this key tile: wave-uniform)
        if (capped) {                             // the softcap first (before the mask): one exp2 and one rcp an element
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * ck) + 1.f);
                    sacc[kb][i] = fmaf(rr, -2.f * md.cap2, md.cap2);
                }
        }
        const bool need_mask = !full || k0 + KT - 1 > qlo + coff + md.wr;
        const bool need_lo = k0 < qhi + coff - md.wl;   // some row's lower bound lies inside or past this tile
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (need_mask) {
                const int thr = rhi - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
            }
            if (need_lo) {
                const int thr = rlo - (k0 + 32 * kb + 4 * h);
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
        if (__any(valid && m_new - m_run > 8.0f) != 0) {   // lazy rescale (fwd_fp8in_kernel) on the real rows; a row's first visible key: inf > 8
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
        i32x8_t pb;                               // P^T as the accumulators hold it, rounded to e4m3 (RNE)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float pe = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], fe, -m_use));   // (-inf stays -inf: fe > 0)
                sacc[kb][i] = pe;
                rs += pe;
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

        // ---- O^T = V^T P^T: the lane's 32 key bytes of head dim 32 dvb + r
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(vt + vt_off(32 * dvb + r, 2 * h));
            const u32x4 a1 = *reinterpret_cast<const u32x4*>(vt + vt_off(32 * dvb + r, 2 * h + 1));
            const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
            oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], 0, 0, 0, 127, 0, 127);
        }
    }

    // ---- epilogue: O^T register i of block dvb is head dim 32 dvb + 4 h + (i & 3) + 8 (i >> 2) of the lane's query row
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    const bool dead = l_tot == 0.f;                      // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
    const float inv = vd * (1.f / l_tot);                // v_descale once, with 1 / l
    const float lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    // (PACKED: kv_combine_row's packed layout, row = h * total_q + packed token)
    const size_t row_id = PACKED ? (size_t)hd * total_q + (size_t)(tok0 + qi) : ((size_t)b * p.hq + hd) * nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + (PACKED ? (size_t)(tok0 + qi) * p.hq + hd : ((size_t)b * nq + qi) * p.hq + hd) * D;
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
        if (h == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * D;
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
                *reinterpret_cast<f32x4*>(prow + 32 * dvb + 8 * g + 4 * h) = y;
            }
        if (h == 0) p.plse[row_id * S + s] = lse_v;
    }
}

}  // namespace

int fp8kv_row_tiles(int64_t heads_q, int64_t heads_kv, int64_t seqlen_q) { return (int)(((heads_q / heads_kv) * seqlen_q + 31) / 32); }

// kv_num_splits (fa_decode.hip) over this kernel's 32-row tiles: the same constants, the same rule
int fp8kv_num_splits(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len) {
    return kv_num_splits(batch, heads_kv, fp8kv_row_tiles(heads_q, heads_kv, seqlen_q), cache_len);
}

int64_t fp8kv_split_len(int64_t cache_len, int64_t seqlen_q, int causal, const Fp8Mod& m) {
    if (m.window_left < 0) return cache_len;
    const int64_t right = causal || m.window_right < 0 ? 0 : m.window_right;
    return std::min(cache_len, std::min<int64_t>(m.window_left, kWinNone) + std::min<int64_t>(right, kWinNone) + seqlen_q);
}

// md: null for fa_fp8_forward_kvcache; else the featured call's kernel arguments, with its sinks (null: none)
static hipError_t launch_fp8_kvcache_t(const Fp8KvArgs& a, const Fp8KvMod* md, const float* sinks, int sink_heads, hipStream_t st) {
    Fp8KvParams p;
    p.q = (const uint8_t*)a.q; p.kc = (const uint8_t*)a.k_cache; p.vc = (const uint8_t*)a.v_cache;
    p.o = (uint16_t*)a.o; p.lse = a.lse;
    p.qds = a.q_descale; p.kds = a.k_descale; p.vds = a.v_descale;
    p.qds_bs = a.qds_bs; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.seqlens = a.cache_seqlens; p.table = a.block_table; p.bidx = a.cache_batch_idx;
    p.tbl_rs = a.table_row_stride; p.nblk = (int)a.num_blocks; p.ps = (int)a.page_size; p.bcache = (int)a.cache_batch;
    p.q_bs = a.q_bs; p.kc_bs = a.kc_bs; p.vc_bs = a.vc_bs;
    p.q_ts = (int)a.q_ts; p.kc_ts = (int)a.kc_ts; p.vc_ts = (int)a.vc_ts;
    p.hq = (int)a.heads_q; p.hkv = (int)a.heads_kv; p.G = (int)(a.heads_q / a.heads_kv);
    p.nq = (int)a.seqlen_q; p.cap = (int)a.cache_len; p.rows = p.G * p.nq; p.causal = a.causal != 0;
    p.c_log2 = a.scale * 1.4426950408889634f;
    const int S = (int)a.num_splits;
    // workspace (S > 1): the O partials, then the lse partials, each rounded up to 256 bytes (kv_workspace_bytes)
    const size_t q_rows = (size_t)a.batch * a.heads_q * a.seqlen_q;
    p.po = (float*)a.workspace;
    p.plse = S > 1 ? (float*)((char*)a.workspace + ((q_rows * S * (size_t)a.d * 4 + 255) & ~(size_t)255)) : nullptr;
    const dim3 grid((unsigned)S, (unsigned)(fp8kv_row_tiles(a.heads_q, a.heads_kv, a.seqlen_q) * p.hkv), (unsigned)a.batch);
    if (a.d != 128) {                                    // launch_fp8_kvcache_hdim: md is never null here
        route_hit(ROUTE_FP8KV_SPLIT_HDIM);
        ProfScope ps(K_FP8KV_SPLIT_HDIM, st);
        const bool paged = a.block_table != nullptr;
        auto launch = [&](auto d_c) {
            constexpr int DD = decltype(d_c)::value;
            if (a.dtype == 2) {
                if (paged) hipLaunchKernelGGL((fp8kv_split_mod_kernel<bf16_tag, true, DD>), grid, dim3(64), 0, st, p, *md);
                else hipLaunchKernelGGL((fp8kv_split_mod_kernel<bf16_tag, false, DD>), grid, dim3(64), 0, st, p, *md);
            } else {
                if (paged) hipLaunchKernelGGL((fp8kv_split_mod_kernel<f16_tag, true, DD>), grid, dim3(64), 0, st, p, *md);
                else hipLaunchKernelGGL((fp8kv_split_mod_kernel<f16_tag, false, DD>), grid, dim3(64), 0, st, p, *md);
            }
        };
        if (a.d == 64) launch(std::integral_constant<int, 64>{});
        else launch(std::integral_constant<int, 256>{});
    } else if (md) {
        route_hit(ROUTE_FP8KV_SPLIT_MOD);
        ProfScope ps(K_FP8KV_SPLIT_MOD, st);
        const bool paged = a.block_table != nullptr;
        if (a.dtype == 2) {
            if (paged) hipLaunchKernelGGL((fp8kv_split_mod_kernel<bf16_tag, true>), grid, dim3(64), 0, st, p, *md);
            else hipLaunchKernelGGL((fp8kv_split_mod_kernel<bf16_tag, false>), grid, dim3(64), 0, st, p, *md);
        } else {
            if (paged) hipLaunchKernelGGL((fp8kv_split_mod_kernel<f16_tag, true>), grid, dim3(64), 0, st, p, *md);
            else hipLaunchKernelGGL((fp8kv_split_mod_kernel<f16_tag, false>), grid, dim3(64), 0, st, p, *md);
        }
    } else {
        ProfScope ps(K_FP8KV_SPLIT, st);
        const bool paged = a.block_table != nullptr;
        if (a.dtype == 2) {
            if (paged) hipLaunchKernelGGL((fp8kv_split_kernel<bf16_tag, true>), grid, dim3(64), 0, st, p);
            else hipLaunchKernelGGL((fp8kv_split_kernel<bf16_tag, false>), grid, dim3(64), 0, st, p);
        } else {
            if (paged) hipLaunchKernelGGL((fp8kv_split_kernel<f16_tag, true>), grid, dim3(64), 0, st, p);
            else hipLaunchKernelGGL((fp8kv_split_kernel<f16_tag, false>), grid, dim3(64), 0, st, p);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || S == 1) return e;
    if (sinks) return launch_kv_combine_sink(a.o, a.lse, p.po, p.plse, a.batch, a.heads_q, a.seqlen_q, a.d, a.dtype, S, sinks, sink_heads, st);
    return launch_kv_combine(a.o, a.lse, p.po, p.plse, a.batch, a.heads_q, a.seqlen_q, a.d, a.dtype, S, st);
}

hipError_t launch_fp8_kvcache(const Fp8KvArgs& a, hipStream_t st) { return launch_fp8_kvcache_t(a, nullptr, nullptr, 0, st); }

// the featured kernel's arguments of an Fp8Mod (one that is not any(): no window, no cap)
static Fp8KvMod fp8kv_mod_args(const Fp8KvArgs& a, const Fp8Mod& m) {
    Fp8KvMod md;
    md.wl = m.window_left >= 0 ? (int)std::min<int64_t>(m.window_left, kWinNone) : kWinNone;
    md.wr = a.causal ? 0 : (m.window_right >= 0 ? (int)std::min<int64_t>(m.window_right, kWinNone) : kWinNone);
    md.cap_k = m.softcap > 0.0 ? (float)(2.0 / m.softcap) : 0.f;
    md.cap2 = m.softcap > 0.0 ? (float)(m.softcap * 1.4426950408889634) : 0.f;
    return md;
}

hipError_t launch_fp8_kvcache_mod(const Fp8KvArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (!m.any()) return launch_fp8_kvcache(a, st);     // the parent call, launch for launch
    if (m.sinks && a.num_splits < 2) return hipErrorInvalidValue;   // (the C layer raises a sink call's S to 2: the sink joins in the combine)
    const Fp8KvMod md = fp8kv_mod_args(a, m);
    return launch_fp8_kvcache_t(a, &md, m.sinks, (int)(m.sink_heads > 0 ? m.sink_heads : 1), st);
}

// Head dims 64 and 256 (fa_fp8_forward_kvcache_hdim): every such call, featured or not, runs
// fp8kv_split_mod_kernel<Tag, PAGED, D>, then kv_combine_kernel at d.  d = 128 is the call above.
hipError_t launch_fp8_kvcache_hdim(const Fp8KvArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (a.d == 128) return launch_fp8_kvcache_mod(a, m, st);
    if (m.sinks && a.num_splits < 2) return hipErrorInvalidValue;
    const Fp8KvMod md = fp8kv_mod_args(a, m);
    return launch_fp8_kvcache_t(a, &md, m.sinks, (int)(m.sink_heads > 0 ? m.sink_heads : 1), st);
}

// Packed queries (fa_fp8_forward_kvcache_varlen): a.cu_seqlens_q non-null, q / o (total_q, H_q, d), lse
// (H_q, total_q).  Every call, featured or not, at every head dim runs fp8kv_split_mod_kernel<Tag, PAGED, D, Fp8KvPacked> on a grid
// sized for max_seqlen_q; for S > 1 the lse partials are filled with kPlseFill bytes first (a memset node: rows that no sequence
// owns keep it) and kv_combine_kernel runs in its packed mode.  The workspace is kv_workspace_bytes(1, H_q, total_q, d, S).
hipError_t launch_fp8_kvcache_varlen(const Fp8KvArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (!a.cu_seqlens_q) return launch_fp8_kvcache_hdim(a, m, st);
    if (a.total_q <= 0 || a.max_seqlen_q <= 0) return hipSuccess;
    const int S = (int)a.num_splits;
    if (m.sinks && S < 2) return hipErrorInvalidValue;
    Fp8KvArgs pa = a;
    pa.seqlen_q = a.max_seqlen_q;                        // what the window's right bound is canonicalised against (fp8kv_mod_args)
    const Fp8KvMod md = fp8kv_mod_args(pa, m);
    Fp8KvParams p;
    p.q = (const uint8_t*)a.q; p.kc = (const uint8_t*)a.k_cache; p.vc = (const uint8_t*)a.v_cache;
    p.o = (uint16_t*)a.o; p.lse = a.lse;
    p.qds = a.q_descale; p.kds = a.k_descale; p.vds = a.v_descale;
    p.qds_bs = a.qds_bs; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.seqlens = a.cache_seqlens; p.table = a.block_table; p.bidx = a.cache_batch_idx;
    p.tbl_rs = a.table_row_stride; p.nblk = (int)a.num_blocks; p.ps = (int)a.page_size; p.bcache = (int)a.cache_batch;
    p.q_bs = 0; p.kc_bs = a.kc_bs; p.vc_bs = a.vc_bs;
    p.q_ts = (int)a.q_ts; p.kc_ts = (int)a.kc_ts; p.vc_ts = (int)a.vc_ts;
    p.hq = (int)a.heads_q; p.hkv = (int)a.heads_kv; p.G = (int)(a.heads_q / a.heads_kv);
    p.nq = (int)a.max_seqlen_q; p.cap = (int)a.cache_len; p.rows = p.G * p.nq; p.causal = a.causal != 0;   // (nq, rows: the kernel takes its own)
    p.c_log2 = a.scale * 1.4426950408889634f;
    const size_t q_rows = (size_t)a.total_q * a.heads_q;
    p.po = (float*)a.workspace;
    p.plse = S > 1 ? (float*)((char*)a.workspace + ((q_rows * S * (size_t)a.d * 4 + 255) & ~(size_t)255)) : nullptr;
    const Fp8KvPacked pk{a.cu_seqlens_q, (int)a.total_q, (int)a.max_seqlen_q};
    if (S > 1) {
        const hipError_t e = hipMemsetAsync(p.plse, kPlseFill, q_rows * S * 4, st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)S, (unsigned)(fp8kv_row_tiles(a.heads_q, a.heads_kv, a.max_seqlen_q) * p.hkv), (unsigned)a.batch);
    {
        route_hit(ROUTE_FP8KV_SPLIT_VARLEN);
        ProfScope ps(K_FP8KV_SPLIT_VARLEN, st);
        const bool paged = a.block_table != nullptr;
        auto launch = [&](auto d_c) {
            constexpr int DD = decltype(d_c)::value;
            if (a.dtype == 2) {
                if (paged) hipLaunchKernelGGL((fp8kv_split_mod_kernel<bf16_tag, true, DD, Fp8KvPacked>), grid, dim3(64), 0, st, p, md, pk);
                else hipLaunchKernelGGL((fp8kv_split_mod_kernel<bf16_tag, false, DD, Fp8KvPacked>), grid, dim3(64), 0, st, p, md, pk);
            } else {
                if (paged) hipLaunchKernelGGL((fp8kv_split_mod_kernel<f16_tag, true, DD, Fp8KvPacked>), grid, dim3(64), 0, st, p, md, pk);
                else hipLaunchKernelGGL((fp8kv_split_mod_kernel<f16_tag, false, DD, Fp8KvPacked>), grid, dim3(64), 0, st, p, md, pk);
            }
        };
        if (a.d == 64) launch(std::integral_constant<int, 64>{});
        else if (a.d == 128) launch(std::integral_constant<int, 128>{});
        else launch(std::integral_constant<int, 256>{});
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || S == 1) return e;
    return launch_kv_combine_packed(a.o, a.lse, p.po, p.plse, a.cu_seqlens_q, a.heads_q, a.total_q, a.d, a.dtype, S, m.sinks,
                                    (int)(m.sink_heads > 0 ? m.sink_heads : 1), st);
}

}  // namespace fa
