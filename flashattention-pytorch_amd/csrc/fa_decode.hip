// KV-cache decoding with split-KV (fa_ex_forward_kvcache; include/fa_mi355x.h): a few query tokens per sequence over a long
// per-sequence cache.  Three launches on the caller's stream, none of which the host has to wait for:
//   kv_append_kernel : k_new / v_new -> k_cache / v_cache at L_b = clamp(cache_seqlens[b], 0, cache_len - N_new) (16 bytes a lane)
//   kv_split_kernel  : one wave per (split, row tile x K/V head, batch element).  The G = H_q / H_kv query heads that share a K/V
//                      head, times the Nq query tokens, are packed into the 16 rows of a tile (row r = token * G + head in the
//                      group), so the cache is read once per K/V head and row tile.  S^T = K Q^T and O^T = V^T P^T on
//                      v_mfma_f32_16x16x32_{bf16,f16}: K fragments come straight from the cache into registers (8 consecutive
//                      d per lane, the A operand as it lies in memory), V goes through a wave-private LDS tile and is read
//                      transposed with ds_read_b64_tr_b16 (the TileSwz image of the forward kernels).  Online softmax in fp32
//                      on the lane of its query row.  One split writes o / lse directly; more write fp32 partials.
//   kv_combine_kernel: S > 1 only — one wave per (b, h_q, row) merges the S partials in split order.
// Split ranges come from len_k on the device (kv_split_range), S from the shapes on the host (fa_capi.hip): the call never
// synchronises and never allocates, so it can be captured in a graph.  Keys are addressed per 32-key tile from one base per
// (batch element, K/V head).  fa_ex_forward_kvcache_paged adds three ways to move that base, all in per-sequence key coordinates, so
// the split rule, the masks and the combine do not change:
//   cache_batch_idx : the base is cache row idx[b]; an index outside [0, B_cache) gives an empty buffer range (zeros, no append).
//   cache_leftpad   : the base moves on by P_b = clamp(leftpad[b], 0, L_b) tokens and len_k = L_b + N_new - P_b.
//   block_table     : kv_split_kernel<.., true>.  Per tile, lane l looks up the page of key k0 + (l & 31) (one 4-byte read, the next
//                     tile's issued a tile ahead) and keeps the 64-bit element offsets page * page stride + slot * token stride of K
//                     and of V; the lane that loads a key row takes its offset by a lane shuffle and reads with a global load at a
//                     32-bit offset inside the page.  A key past the split's end or on a page outside [0, num_blocks) has offset -1
//                     and reads as zeros without touching memory.  The contiguous instantiations hold none of this.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"
#include <algorithm>

namespace fa {

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <typename Tag> __device__ __forceinline__ f32x4_t mfma16(s16x8 a, s16x8 b, f32x4_t c);
template <> __device__ __forceinline__ f32x4_t mfma16<bf16_tag>(s16x8 a, s16x8 b, f32x4_t c) {
    typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf8*>(&a), *reinterpret_cast<bf8*>(&b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_t mfma16<f16_tag>(s16x8 a, s16x8 b, f32x4_t c) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<h8*>(&a), *reinterpret_cast<h8*>(&b), c, 0, 0, 0);
}

struct KvParams {
    const uint16_t *q;
    uint16_t *kc, *vc;                 // the caches (written by the append kernel only)
    const uint16_t *kn, *vn;
    uint16_t *o;
    float *lse, *po, *plse;          // po / plse: the partials of S > 1 ((b, h_q, token)-major rows, then split)
    const int* seqlens;              // null: L_b = cache_len (and N_new = 0)
    const int *table, *bidx, *leftpad;   // block_table (paged), cache_batch_idx, cache_leftpad: untrusted device memory, or null
    long long tbl_rs;                // table row stride (entries)
    int nblk, ps, bcache;            // pages in the pools, tokens a page, rows of a contiguous cache (bidx)
    const float* alibi;
    long long q_bs, kc_bs, vc_bs, kn_bs, vn_bs;   // batch strides (elements)
    int q_ts, kc_ts, vc_ts, kn_ts, vn_ts;         // token strides (elements)
    int hq, hkv, G, nq, nnew, cap, d, rows;       // rows = G * nq
    int wl, wr;                                   // band [i + coff - wl, i + coff + wr]; kWinNone = unbounded, wr = 0 if causal
    int al_bs;
    float scale, c_log2;
    ExScore sc;                                   // cap_k / cap_a (softcap > 0) and al_k, as the extended kernels take them
};

// L_b (the cache_seqlens clamp), P_b (the cache_leftpad clamp: the sequence's first cache position) and len_k = L_b + N_new - P_b
__device__ __forceinline__ int kv_len_k(const KvParams& p, int b, int& L, int& P) {
    L = p.seqlens ? min(max(p.seqlens[b], 0), p.cap - p.nnew) : p.cap;
    P = p.leftpad ? min(max(p.leftpad[b], 0), L) : 0;
    return L + p.nnew - P;
}

// Keys [kbeg, kend) of split s of S for the row tile whose query tokens are [qlo, qhi]: the union of the rows' bands,
// [max(0, qlo + coff - wl), min(len_k, qhi + coff + wr + 1)), cut into 32-key tiles from its start, tiles
// [floor(s nt / S), floor((s + 1) nt / S)) to split s.  Empty (kbeg >= kend) when the band is, or nt < S for some s.
// tests/test_kvcache_cpu.py models this rule.
__device__ __forceinline__ void kv_split_range(const KvParams& p, int lk, int qlo, int qhi, int s, int S, int& kbeg, int& kend) {
    constexpr int KT = 32;
    const int coff = lk - p.nq;
    const int lo = max(0, qlo + coff - p.wl), hi = min(lk, qhi + coff + p.wr + 1);
    const int nt = hi > lo ? (hi - lo + KT - 1) / KT : 0;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    kbeg = lo + t0 * KT;
    kend = min(hi, lo + t1 * KT);
}

// Token L_b + n of batch element b goes to cache row (bidx ? bidx[b] : b) at position L_b + n, or through the table to
// pool[table[b, (L_b + n) / ps], (L_b + n) % ps]; a row or page outside the cache / pool drops the token.
__global__ __launch_bounds__(256) void kv_append_kernel(KvParams p) {
    const int cpr = p.d / 8;                                      // 16-byte chunks per head row
    const long long per_b = (long long)p.nnew * p.hkv * cpr;
    const int b = blockIdx.y;
    int L, P;
    kv_len_k(p, b, L, P);
    long long row = b;
    if (p.bidx) {
        const int ix = p.bidx[b];
        if ((unsigned)ix >= (unsigned)p.bcache) return;
        row = ix;
    }
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < per_b; t += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(t % cpr);
        const long long r = t / cpr;
        const int h = (int)(r % p.hkv), n = (int)(r / p.hkv);
        const size_t col = (size_t)h * p.d + 8 * c;
        int pos = L + n;
        long long unit = row;
        if (p.table) {
            const int j = pos / p.ps;
            const int pg = p.table[b * p.tbl_rs + j];
            if ((unsigned)pg >= (unsigned)p.nblk) continue;
            pos -= j * p.ps;
            unit = pg;
        }
        const u32x4 kx = *reinterpret_cast<const u32x4*>(p.kn + b * p.kn_bs + (size_t)n * p.kn_ts + col);
        const u32x4 vx = *reinterpret_cast<const u32x4*>(p.vn + b * p.vn_bs + (size_t)n * p.vn_ts + col);
        *reinterpret_cast<u32x4*>(p.kc + unit * p.kc_bs + (size_t)pos * p.kc_ts + col) = kx;
        *reinterpret_cast<u32x4*>(p.vc + unit * p.vc_bs + (size_t)pos * p.vc_ts + col) = vx;
    }
}

// One wave: split blockIdx.x of gridDim.x, row tile blockIdx.y / hkv and K/V head blockIdx.y % hkv, batch element blockIdx.z.
// Lane l: query row r = l & 15 of the tile (S^T's column, O^T's column), lane group g = l >> 4 (4 keys of each 16-key block
// of S^T, 4 head-dim elements of each 16-wide block of O^T).  D: the padded tile width (64 | 128 | 256), p.d <= D.
// PAGED: keys are reached through p.table (see the head of this file); otherwise through one buffer range per wave.
template <typename Tag, int D, bool PAGED>
__global__ __launch_bounds__(64) void kv_split_kernel(KvParams p) {
    constexpr int KT = 32, NKS = D / 32, NDB = D / 16, CPR = D / 8, VLD = KT * CPR / 64;
    __shared__ __attribute__((aligned(16))) char vs[KT * D * 2];   // V tile, [key][D] in the TileSwz<D> image
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int DR = p.d;
    int L_b, P_b;
    const int lk = kv_len_k(p, b, L_b, P_b), coff = lk - p.nq;
    const int pr0 = 16 * rt, pr = pr0 + r;
    const int qlo = pr0 / p.G, qhi = (min(pr0 + 16, p.rows) - 1) / p.G;
    int kbeg, kend;
    kv_split_range(p, lk, qlo, qhi, s, S, kbeg, kend);

    // this lane's query row: token qi, query head h; its visible keys [rlo, rhi] (padding rows of the tile: none)
    const bool valid = pr < p.rows;
    const int qi = valid ? pr / p.G : qlo, h = hk * p.G + (valid ? pr - qi * p.G : 0);
    const int rlo = max(qi + coff - p.wl, kbeg);
    const int rhi = valid ? min(min(qi + coff + p.wr, lk - 1), kend - 1) : -1;
    float al = 0.f;
    if (p.alibi && valid) al = p.alibi[(size_t)b * p.al_bs + h] * p.sc.al_k;

    const buf_rsrc_t q_rs = make_rsrc(p.q + b * p.q_bs, (unsigned)(((p.nq - 1) * p.q_ts + p.hq * DR) * 2));
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int col = 32 * ks + 8 * g;
        qf[ks] = buf_load_frag(q_rs, (valid && col < DR) ? (qi * p.q_ts + h * DR + col) * 2 : kOobOff);
    }
    // contiguous: the sequence's keys start P_b tokens into cache row (bidx ? bidx[b] : b); a row outside the cache is an empty range
    long long crow = b;
    int ctok = PAGED ? 0 : p.cap - P_b;   // tokens the buffer range holds
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; ctok = 0; }
    }
    const buf_rsrc_t k_rs = make_rsrc(p.kc + crow * p.kc_bs + (long long)P_b * p.kc_ts,
                                      ctok > 0 ? (unsigned)(((ctok - 1) * p.kc_ts + p.hkv * DR) * 2) : 0u);
    const buf_rsrc_t v_rs = make_rsrc(p.vc + crow * p.vc_bs + (long long)P_b * p.vc_ts,
                                      ctok > 0 ? (unsigned)(((ctok - 1) * p.vc_ts + p.hkv * DR) * 2) : 0u);
    // paged: the table row, and the page j0 and slot s0 of the tile's first key (a 32-key tile spans at most three pages)
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    int j0 = 0, s0 = 0, pg = -1;
    auto page_of = [&](int jt, int st, int kt) {   // the table entry of key kt + (lane & 31), or -1 past the split's end
        int j = jt, sl = st + (lane & 31);
        if (sl >= p.ps) { sl -= p.ps; ++j; }
        if (sl >= p.ps) ++j;
        return kt + (lane & 31) < kend ? tbl[j] : -1;
    };
    if (PAGED && kbeg < kend) {
        j0 = kbeg / p.ps;
        s0 = kbeg - j0 * p.ps;
        pg = page_of(j0, s0, kbeg);
    }

    f32x4_t oacc[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t) oacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const int q4 = r >> 2, p4 = r & 3;   // ds_read_b64_tr_b16: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p + 3

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        // K fragments (A of S^T = K Q^T: key k0 + 16 kb + r, head dims 32 ks + 8 g ..) and this lane's share of the V tile;
        // keys past the split's end read as zeros (the cache behind them may hold anything)
        s16x8 kf[2][NKS];
        u32x4 vr[VLD];
        if constexpr (PAGED) {
            // this lane's key k0 + (lane & 31): element offsets of its token in the two pools, -1 = reads as zeros
            long long ko = -1, vo = -1;
            {
                int sl = s0 + (lane & 31);
                if (sl >= p.ps) sl -= p.ps;
                if (sl >= p.ps) sl -= p.ps;
                if ((unsigned)pg < (unsigned)p.nblk) {
                    ko = pg * p.kc_bs + (long long)sl * p.kc_ts;
                    vo = pg * p.vc_bs + (long long)sl * p.vc_ts;
                }
            }
            s0 += KT;
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (k0 + KT < kend) pg = page_of(j0, s0, k0 + KT);   // the next tile's lookup, a tile ahead of its use
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const long long ro = __shfl(ko, 16 * kb + r, 64);
                const uint16_t* kp = p.kc + ro + hk * DR + 8 * g;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bool ok = ro >= 0 && 32 * ks + 8 * g < DR;
                    const s16x8 x = *reinterpret_cast<const s16x8*>(ok ? kp + 32 * ks : p.q);
                    kf[kb][ks] = ok ? x : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
            }
#pragma unroll
            for (int i = 0; i < VLD; ++i) {
                const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR;
                const long long ro = __shfl(vo, row, 64);
                const bool ok = ro >= 0 && 8 * ch < DR;
                const u32x4 x = *reinterpret_cast<const u32x4*>(ok ? p.vc + ro + hk * DR + 8 * ch : p.q);
                vr[i] = ok ? x : u32x4{0u, 0u, 0u, 0u};
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int key = k0 + 16 * kb + r;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const int col = 32 * ks + 8 * g;
                    kf[kb][ks] = buf_load_frag(k_rs, (key < kend && col < DR) ? (key * p.kc_ts + hk * DR + col) * 2 : kOobOff);
                }
            }
#pragma unroll
            for (int i = 0; i < VLD; ++i) {
                const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR, key = k0 + row;
                vr[i] = __builtin_amdgcn_raw_buffer_load_b128(v_rs, (key < kend && 8 * ch < DR) ? (key * p.vc_ts + hk * DR + 8 * ch) * 2 : kOobOff,
                                                              0, 0);
            }
        }
        f32x4_t sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) sacc[kb] = mfma16<Tag>(kf[kb][ks], qf[ks], sacc[kb]);
        }
        // (the previous tile's transposed reads were issued before these writes: one wave, LDS in order)
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR;
            *reinterpret_cast<u32x4*>(vs + TileSwz<D>::off(row, ch)) = vr[i];
        }
        // score modifiers (before any mask, as in the extended kernels), then the row's band: register i of block kb holds key
        // k0 + 16 kb + 4 g + i
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 16 * kb + 4 * g + i;
                float x = sacc[kb][i];
                if (p.sc.cap_a > 0.f) { float dt; x = mod_softcap(x, p.sc, dt); }
                if (p.alibi) x = mod_alibi(x, al, (float)(qi + coff - key));
                x = (key >= rlo && key <= rhi) ? x : -INFINITY;
                sacc[kb][i] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * p.c_log2);
        const float mc = m_use * p.c_log2;
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int t = 0; t < NDB; ++t) oacc[t] *= alpha;
        // P^T as the B operand of O^T = V^T P^T: k-slot 8 g + j is key 4 g + j (j < 4) and 16 + 4 g + j - 4 (j >= 4)
        u32x4 pk;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float e0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][2 * j], p.c_log2, -mc));
                const float e1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][2 * j + 1], p.c_log2, -mc));
                l_run += e0 + e1;
                pk[2 * kb + j] = pack2<Tag>(e0, e1);
            }
        const s16x8 pb = *reinterpret_cast<s16x8*>(&pk);
        // V^T operand, the same k-slots: rows (keys) 4 g + q and 16 + 4 g + q, head dims 16 t + 4 p ..
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int ch = 2 * t + (p4 >> 1), bo = 8 * (p4 & 1);
            const s16x4 lo = lds_tr16(vs + TileSwz<D>::off(4 * g + q4, ch) + bo);
            const s16x4 hi = lds_tr16(vs + TileSwz<D>::off(16 + 4 * g + q4, ch) + bo);
            oacc[t] = mfma16<Tag>(cat8(lo, hi), pb, oacc[t]);
        }
    }

    // ---- epilogue: the row's sum over the four lane groups; O^T register i of block t is head dim 16 t + 4 g + i
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const float lse_v = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if (!valid) return;
    const size_t row_id = ((size_t)b * p.hq + h) * p.nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + (((size_t)b * p.nq + qi) * p.hq + h) * DR;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int col = 16 * t + 4 * g;
            if (col < DR) {
                u32x2 v;
                v[0] = pack2_rn<Tag>(oacc[t][0] * inv, oacc[t][1] * inv);
                v[1] = pack2_rn<Tag>(oacc[t][2] * inv, oacc[t][3] * inv);
                *reinterpret_cast<u32x2*>(orow + col) = v;
            }
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * DR;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int col = 16 * t + 4 * g;
            if (col < DR) *reinterpret_cast<f32x4_t*>(prow + col) = oacc[t] * inv;
        }
        if (g == 0) p.plse[row_id * S + s] = lse_v;
    }
}

// One wave per (b, h_q, token) row, four rows per workgroup.  The lanes read the S lse partials side by side (lane c: splits
// c, c + 64, ..), reduce max and weight sum over the wave in a fixed shuffle order, and park the weights in LDS; then lane c adds
// head dims 4c .. 4c + 3 of the O partials in split order, eight loads in flight, branch-free: a split with lse_s = -inf (empty,
// or no visible key) has weight 0 and its O partial, which it never wrote, is selected away.  A row without any visible key gives
// o = 0, lse = -inf.  Same bits on every run.
template <typename Tag>
__global__ __launch_bounds__(256) void kv_combine_kernel(KvParams p, int S, long long nrows) {
    __shared__ float wsh[4][256];
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63, DR = p.d;
    const long long row = (long long)blockIdx.x * 4 + wv;
    if (row >= nrows) return;   // (wave-uniform; the LDS rows are wave-private, no barrier)
    const float* pl = p.plse + row * S;
    float m = -INFINITY;
    for (int s = c; s < S; s += 64) m = fmaxf(m, pl[s]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int s = c; s < S; s += 64) {
        const float ls = pl[s];
        const float w = (ls == -INFINITY) ? 0.f : __expf(ls - m);
        wsh[wv][s] = w;
        sum += w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (4 * c < DR) {
        const float* po = p.po + row * S * DR + 4 * c;
#pragma unroll 8
        for (int s = 0; s < S; ++s) {
            const float w = wsh[wv][s];
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(po + (size_t)s * DR);
            acc += (w != 0.f) ? w * x : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
    // row = (b * hq + h) * nq + qi  ->  o (b, qi, h)
    const long long bh = row / p.nq;
    const int qi = (int)(row - bh * p.nq), h = (int)(bh % p.hq);
    const long long b = bh / p.hq;
    if (4 * c < DR) {
        u32x2 v;
        v[0] = pack2_rn<Tag>(acc[0] * inv, acc[1] * inv);
        v[1] = pack2_rn<Tag>(acc[2] * inv, acc[3] * inv);
        *reinterpret_cast<u32x2*>(p.o + ((b * p.nq + qi) * p.hq + h) * DR + 4 * c) = v;
    }
    if (c == 0) p.lse[row] = sum > 0.f ? m + logf(sum) : -INFINITY;
}

template <typename Tag, int D>
hipError_t launch_split(const KvParams& p, int S, int row_tiles, int batch, hipStream_t st) {
    if (p.table)
        hipLaunchKernelGGL((kv_split_kernel<Tag, D, true>), dim3((unsigned)S, (unsigned)(row_tiles * p.hkv), (unsigned)batch), dim3(64), 0, st, p);
    else
        hipLaunchKernelGGL((kv_split_kernel<Tag, D, false>), dim3((unsigned)S, (unsigned)(row_tiles * p.hkv), (unsigned)batch), dim3(64), 0, st, p);
    return hipGetLastError();
}

template <typename Tag>
hipError_t launch_kv_t(const KvParams& p, int S, int row_tiles, int batch, hipStream_t st) {
    hipError_t e;
    if (p.d <= 64) e = launch_split<Tag, 64>(p, S, row_tiles, batch, st);
    else if (p.d <= 128) e = launch_split<Tag, 128>(p, S, row_tiles, batch, st);
    else e = launch_split<Tag, 256>(p, S, row_tiles, batch, st);
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = (long long)batch * p.hq * p.nq;
    hipLaunchKernelGGL((kv_combine_kernel<Tag>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, p, S, nrows);
    return hipGetLastError();
}

}  // namespace

int kv_num_splits(int64_t batch, int64_t heads_kv, int64_t row_tiles, int64_t cache_len) {
    constexpr int64_t kCUs = 256, kWavesPerCU = 16, kMinKeys = 128;   // MI355X; one wave per workgroup
    const int64_t units = batch * heads_kv * row_tiles;
    if (units <= 0 || cache_len <= 0) return 1;
    int64_t s = (kCUs * kWavesPerCU + units - 1) / units;
    s = std::min<int64_t>(s, (cache_len + kMinKeys - 1) / kMinKeys);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, 256));
}

size_t kv_workspace_bytes(int64_t batch, int64_t heads_q, int64_t seqlen_q, int64_t d, int splits) {
    if (splits <= 1 || batch <= 0 || heads_q <= 0 || seqlen_q <= 0 || d <= 0) return 0;
    const size_t rows = (size_t)batch * heads_q * seqlen_q * splits;
    return ((rows * d * 4 + 255) & ~(size_t)255) + ((rows * 4 + 255) & ~(size_t)255);
}

hipError_t launch_kvcache(const KvArgs& a, hipStream_t st) {
    KvParams p;
    p.q = (const uint16_t*)a.q; p.kc = (uint16_t*)a.k_cache; p.vc = (uint16_t*)a.v_cache;
    p.kn = (const uint16_t*)a.k_new; p.vn = (const uint16_t*)a.v_new;
    p.o = (uint16_t*)a.o; p.lse = a.lse;
    p.seqlens = a.cache_seqlens;
    p.table = a.block_table; p.bidx = a.cache_batch_idx; p.leftpad = a.cache_leftpad;
    p.tbl_rs = a.table_row_stride; p.nblk = (int)a.num_blocks; p.ps = (int)a.page_size; p.bcache = (int)a.cache_batch;
    p.alibi = a.alibi;
    p.q_bs = a.q_bs; p.kc_bs = a.kc_bs; p.vc_bs = a.vc_bs; p.kn_bs = a.kn_bs; p.vn_bs = a.vn_bs;
    p.q_ts = (int)a.q_ts; p.kc_ts = (int)a.kc_ts; p.vc_ts = (int)a.vc_ts; p.kn_ts = (int)a.kn_ts; p.vn_ts = (int)a.vn_ts;
    p.hq = (int)a.heads_q; p.hkv = (int)a.heads_kv; p.G = (int)(a.heads_q / a.heads_kv);
    p.nq = (int)a.seqlen_q; p.nnew = (int)a.seqlen_new; p.cap = (int)a.cache_len; p.d = (int)a.d;
    p.rows = p.G * p.nq;
    p.wl = a.window_left >= 0 ? (int)a.window_left : kWinNone;
    p.wr = a.causal ? 0 : (a.window_right >= 0 ? (int)a.window_right : kWinNone);
    p.al_bs = (int)a.alibi_bstride;
    p.scale = a.scale;
    p.c_log2 = a.scale * 1.4426950408889634f;
    // the extended kernels' modifier constants (fa_ex_common.h: make_ex_params_s)
    const double cap = a.softcap > 0.0 ? a.softcap : 0.0, sc = a.scale;
    p.sc.alibi = a.alibi; p.sc.al_heads = 1; p.sc.al_bstride = 0;
    p.sc.softcap = (float)cap;
    p.sc.cap_k = cap > 0.0 ? (float)(2.0 * 1.4426950408889634 * sc / cap) : 0.f;
    p.sc.cap_a = cap > 0.0 ? (float)(cap / sc) : 0.f;
    p.sc.al_k = (float)(1.0 / sc);
    const int S = (int)a.num_splits;
    p.po = (float*)a.workspace;
    // workspace (S > 1): the O partials, then the lse partials, each rounded up to 256 bytes (kv_workspace_bytes)
    p.plse = S > 1 ? (float*)((char*)a.workspace + (((size_t)a.batch * a.heads_q * a.seqlen_q * S * a.d * 4 + 255) & ~(size_t)255))
                   : nullptr;
    const int batch = (int)a.batch;
    if (p.nnew > 0) {
        const long long per_b = (long long)p.nnew * p.hkv * (p.d / 8);
        const unsigned gx = (unsigned)std::min<long long>((per_b + 255) / 256, 1024);
        hipLaunchKernelGGL(kv_append_kernel, dim3(gx, (unsigned)batch), dim3(256), 0, st, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int row_tiles = (p.rows + 15) / 16;
    return a.dtype == 1 ? launch_kv_t<f16_tag>(p, S, row_tiles, batch, st) : launch_kv_t<bf16_tag>(p, S, row_tiles, batch, st);
}

}  // namespace fa
