// KV-cache decoding with a second query operand and K and V of different widths (fa_ex_forward_kvcache_qv; FlashAttention-3's
// qv): multi-head latent attention at decode time.  Every cached token is a 64-wide rotary row k (k_cache) and a 512-wide latent
// row v (v_cache); for query head h reading K/V head hk = h / G
//   s[i, j] = scale * (q[i, h, :] . k[j, hk, :] + qv[i, h, :] . v[j, hk, :]),   o[i, h, :] = sum_j softmax_j(s)[i, j] v[j, hk, :]
// so the latent row is the score operand and the value operand.  It is fetched from memory once per workgroup:
//   mla_split_kernel  : NW waves (1 | 2 | 4), wave w the row tile NW * blockIdx.y' + w of 16 packed rows (row = token * G + head,
//                       the mapping of kv_split_kernel).  Per 32-key tile the workgroup copies the 32 x 512 latent rows and the
//                       32 x 64 rotary rows into LDS (36 KiB, 16 bytes a lane and step, through registers; with four waves the
//                       loads of tile t + 1 are issued before tile t is computed on), the latent in the swizzled image MlaSwz.  S^T = K Q^T reads that image row-wise (ds_read_b128: 8 consecutive head dims a
//                       lane, 2 + 16 k-steps of v_mfma_f32_16x16x32 per 16 keys against the q and qv fragments the wave keeps in
//                       registers); O^T = V^T P^T reads the same bytes transposed (ds_read_b64_tr_b16), 32 MFMAs into a 16 x 512
//                       fp32 accumulator.  Online softmax in fp32 on the lane of its query row, as in kv_split_kernel.
//   mla_combine_kernel: S > 1 only — kv_combine_kernel with a loop over the two 256-column halves of a 512-wide row.
// Lengths, pages, cache rows, split ranges and masks are kv_len_k, kv_split_range and the page rules of fa_decode.hip
// (fa_decode_common.h): the split range of a workgroup is the union of its row tiles' bands, every row masks its own band.
// Small launches: the wave count follows the packed rows (mla_waves: 16 rows -> one wave a workgroup), so no wave of a
// workgroup is without rows unless the last row tile of a larger call is; the launch rule (mla_num_splits) then cuts the keys
// into more splits, and the partial results meet in mla_combine_kernel in the fixed split order.  That is the merge a
// workgroup-internal key split would need a second, LDS-resident copy of; here it is the one the split path already has.
// Sparse form (fa_mla_sparse_forward): mla_sparse_kernel below, the same tile pipeline over a per-query list of token positions.
#include "fa_decode_common.h"
#include <algorithm>

namespace fa {

namespace {

constexpr int kMlaDk = 64, kMlaDv = 512, kMlaKT = 32;
constexpr int kMlaLatBytes = kMlaKT * kMlaDv * 2, kMlaLdsBytes = kMlaLatBytes + kMlaKT * kMlaDk * 2;

// the latent tile [32][512]: 1024-byte rows, the 16-chunk pattern of TileSwz<256> repeating (a chunk's bank is its index mod 16)
struct MlaSwz {
    static __device__ __forceinline__ int off(int row, int ch) { return 1024 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
};

struct MlaParams {
    KvParams p;            // p.d = 64: q, k_cache; v_cache, o and the partials are 512 wide
    const uint16_t* qv;    // (batch, nq, hq, 512): batch stride qv_bs, token stride qv_ts
    long long qv_bs;
    int qv_ts;
};

template <typename Tag, int NW, bool PAGED>
__global__ __launch_bounds__(64 * NW) void mla_split_kernel(MlaParams mp) {
    constexpr int KT = kMlaKT, DK = kMlaDk, DV = kMlaDv, NDB = DV / 16, T = 64 * NW;
    constexpr int LCH = KT * (DV / 8) / T, RCH = KT * (DK / 8) / T;   // 16-byte chunks a thread moves per tile: latent, rotary
    static_assert(LCH * T == KT * DV / 8 && RCH >= 1, "tile copy");
    __shared__ __attribute__((aligned(16))) char lds[kMlaLdsBytes];
    char* const lat = lds;
    char* const rop = lds + kMlaLatBytes;
    const KvParams& p = mp.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, wt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int nq = p.nq, rows = p.rows;
    const long long tok0 = (long long)b * nq;
    int L_b, P_b;
    const int lk = kv_len_k(p, b, 0, L_b, P_b), coff = lk - nq;
    // the workgroup's rows [wr0, wr1) and the key range of their bands' union; wr0 < rows by the grid
    const int wr0 = 16 * NW * wt, wr1 = min(wr0 + 16 * NW, rows);
    int kbeg, kend;
    kv_split_range(p, lk, nq, wr0 / p.G, (wr1 - 1) / p.G, s, S, kbeg, kend);

    // this wave's row tile (none: the wave only copies), this lane's query row and its visible keys [rlo, rhi]
    const int pr0 = wr0 + 16 * w, pr = pr0 + r;
    const bool active = pr0 < rows, valid = pr < rows;
    const int qlo = min(pr0, rows - 1) / p.G;
    const int qi = valid ? pr / p.G : qlo, h = hk * p.G + (valid ? pr - qi * p.G : 0);
    const int rlo = max(qi + coff - p.wl, kbeg);
    const int rhi = valid ? min(min(qi + coff + p.wr, lk - 1), kend - 1) : -1;

    s16x8 qf[DK / 32], qvf[DV / 32];
    {
        const buf_rsrc_t q_rs = make_rsrc(p.q + b * p.q_bs, (unsigned)(((nq - 1) * p.q_ts + p.hq * DK) * 2));
        const buf_rsrc_t qv_rs = make_rsrc(mp.qv + b * mp.qv_bs, (unsigned)(((nq - 1) * mp.qv_ts + p.hq * DV) * 2));
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks) qf[ks] = buf_load_frag(q_rs, valid ? (qi * p.q_ts + h * DK + 32 * ks + 8 * g) * 2 : kOobOff);
#pragma unroll
        for (int ks = 0; ks < DV / 32; ++ks) qvf[ks] = buf_load_frag(qv_rs, valid ? (qi * mp.qv_ts + h * DV + 32 * ks + 8 * g) * 2 : kOobOff);
    }
    // contiguous: cache row (bidx ? bidx[b] : b); a row outside the cache is an empty range (kv_split_kernel's rule)
    long long crow = b;
    int ctok = PAGED ? 0 : p.cap;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; ctok = 0; }
    }
    const buf_rsrc_t k_rs = make_rsrc(p.kc + crow * p.kc_bs, ctok > 0 ? (unsigned)(((ctok - 1) * p.kc_ts + p.hkv * DK) * 2) : 0u);
    const buf_rsrc_t v_rs = make_rsrc(p.vc + crow * p.vc_bs, ctok > 0 ? (unsigned)(((ctok - 1) * p.vc_ts + p.hkv * DV) * 2) : 0u);
    // paged: kv_split_kernel's lookup, done by every wave for itself (lane l: key k0 + (l & 31), the next tile's a tile ahead)
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    int j0 = 0, s0 = 0, pg = -1;
    auto page_of = [&](int jt, int st, int kt) {
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
    const int q4 = r >> 2, p4 = r & 3;

    // One tile's copy, loads and LDS writes apart: chunk idx = T i + tid of the latent rows (row idx / 64 = (T / 64) i + w, the
    // same for the whole wave; chunk idx % 64 = lane), then of the rotary rows (idx / 8, idx % 8).  Keys past the split's end,
    // on a page outside the pool or in a row outside the cache are zeros.  Paged: this lane's key kt + (lane & 31) has element
    // offsets ko / vo in the two pools, -1 = reads as zeros.  Four waves (PRE): a thread holds a whole tile's share, 9 chunks,
    // and the loads of tile k0 + 32 are in flight while tile k0 is computed on.  Fewer waves move 18 or 36 chunks a thread,
    // eight at a time between the barriers; there the other workgroups of the CU cover the latency.
    constexpr bool PRE = LCH <= 8;
    constexpr int LB = PRE ? LCH : 8;
    static_assert(LCH % LB == 0, "tile copy");
    u32x4 xl[LB], xr[RCH];
    long long ko = -1, vo = -1;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    auto offsets = [&](int kt) {
        if constexpr (PAGED) {
            int sl = s0 + (lane & 31);
            if (sl >= p.ps) sl -= p.ps;
            if (sl >= p.ps) sl -= p.ps;
            ko = vo = -1;
            if ((unsigned)pg < (unsigned)p.nblk) {
                ko = pg * p.kc_bs + (long long)sl * p.kc_ts;
                vo = pg * p.vc_bs + (long long)sl * p.vc_ts;
            }
            s0 += KT;
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (kt + KT < kend) pg = page_of(j0, s0, kt + KT);   // the next tile's lookup, a tile ahead of its use
        }
    };
    auto load_lat = [&](int kt, int i0) {
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            const int row = (T / 64) * (i0 + i) + wu;
            if constexpr (PAGED) {
                const long long ro = ((long long)__builtin_amdgcn_readlane((int)(vo >> 32), row) << 32) |
                                     (unsigned)__builtin_amdgcn_readlane((int)vo, row);   // (wave-uniform: a scalar base)
                const bool ok = ro >= 0;
                const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? p.vc + ro + hk * DV + 8 * lane : p.q);
                xl[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
            } else {
                const int key = kt + row;
                xl[i] = __builtin_amdgcn_raw_buffer_load_b128(v_rs, key < kend ? (key * p.vc_ts + hk * DV + 8 * lane) * 2 : kOobOff, 0, 0);
            }
        }
    };
    auto store_lat = [&](int i0) {
#pragma unroll
        for (int i = 0; i < LB; ++i) *reinterpret_cast<u32x4*>(lat + MlaSwz::off((T / 64) * (i0 + i) + wu, lane)) = xl[i];
    };
    auto load_rot = [&](int kt) {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid, row = idx >> 3, ch = idx & 7;
            if constexpr (PAGED) {
                const long long ro = __shfl(ko, row, 64);
                const bool ok = ro >= 0;
                const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? p.kc + ro + hk * DK + 8 * ch : p.q);
                xr[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
            } else {
                const int key = kt + row;
                xr[i] = __builtin_amdgcn_raw_buffer_load_b128(k_rs, key < kend ? (key * p.kc_ts + hk * DK + 8 * ch) * 2 : kOobOff, 0, 0);
            }
        }
    };
    auto store_rot = [&]() {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid;
            *reinterpret_cast<u32x4*>(rop + TileSwz<64>::off(idx >> 3, idx & 7)) = xr[i];
        }
    };
    if (PRE && kbeg < kend) {
        offsets(kbeg);
        load_lat(kbeg, 0);
        load_rot(kbeg);
    }

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        if constexpr (!PRE) offsets(k0);
        __syncthreads();   // every wave has read the previous tile
        if constexpr (PRE) {
            store_lat(0);
        } else {
#pragma unroll 1
            for (int i0 = 0; i0 < LCH; i0 += LB) {
                load_lat(k0, i0);
                store_lat(i0);
            }
            load_rot(k0);
        }
        store_rot();
        __syncthreads();
        if (PRE && k0 + KT < kend) {
            offsets(k0 + KT);
            load_lat(k0 + KT, 0);
            load_rot(k0 + KT);
        }
        if (!active) continue;   // (wave-uniform; the wave still takes part in the copies and the barriers)

        // S^T = K Q^T: A = key 16 kb + r, head dims 32 ks + 8 g .. of the rotary row, then of the latent row
        f32x4_t sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < DK / 32; ++ks)
                sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(rop + TileSwz<64>::off(16 * kb + r, 4 * ks + g)), qf[ks], sacc[kb]);
#pragma unroll
            for (int ks = 0; ks < DV / 32; ++ks) {
                // (four operand reads in flight: hipcc would otherwise hoist all of a tile's reads and spill)
                if (ks % 4 == 0) __builtin_amdgcn_sched_barrier(0);
                sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(lat + MlaSwz::off(16 * kb + r, 4 * ks + g)), qvf[ks], sacc[kb]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // both score tiles live in VGPRs at one point (kv_split_kernel: the second chain must not end in the first one's registers)
        asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
        // the row's band: register i of block kb holds key k0 + 16 kb + 4 g + i
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 16 * kb + 4 * g + i;
                const float x = (key >= rlo && key <= rhi) ? sacc[kb][i] : -INFINITY;
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
        // V^T operand from the same latent image: rows (keys) 4 g + q and 16 + 4 g + q, head dims 16 t + 4 p ..
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            if (t % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            const int ch = 2 * t + (p4 >> 1), bo = 8 * (p4 & 1);
            const s16x4 lo = lds_tr16(lat + MlaSwz::off(4 * g + q4, ch) + bo);
            const s16x4 hi = lds_tr16(lat + MlaSwz::off(16 + 4 * g + q4, ch) + bo);
            oacc[t] = mfma16<Tag>(cat8(lo, hi), pb, oacc[t]);
        }
    }

    // ---- epilogue (kv_split_kernel's): O^T register i of block t is head dim 16 t + 4 g + i
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const float lse_v = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if (!valid) return;
    const size_t row_id = ((size_t)b * p.hq + h) * nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + ((size_t)(tok0 + qi) * p.hq + h) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            u32x2 v;
            v[0] = pack2_rn<Tag>(oacc[t][0] * inv, oacc[t][1] * inv);
            v[1] = pack2_rn<Tag>(oacc[t][2] * inv, oacc[t][3] * inv);
            *reinterpret_cast<u32x2*>(orow + 16 * t + 4 * g) = v;
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) *reinterpret_cast<f32x4_t*>(prow + 16 * t + 4 * g) = oacc[t] * inv;
        if (g == 0) p.plse[row_id * S + s] = lse_v;
    }
}

// kv_combine_kernel for 512-wide rows: one wave per (b, h_q, token) row, four rows a workgroup; the weights as there, then lane c
// adds head dims 256 j + 4 c .. + 3 (j = 0, 1) of the O partials in split order.  A split with lse_s = -inf has weight 0 and its
// O partial, which it never wrote, is selected away; a row without any visible key gives o = 0, lse = -inf.  Same bits on every run.
template <typename Tag>
__global__ __launch_bounds__(256) void mla_combine_kernel(KvParams p, int S, long long nrows) {
    constexpr int DV = kMlaDv;
    __shared__ float wsh[4][256];
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + wv;
    if (row >= nrows) return;   // (wave-uniform; the LDS rows are wave-private, no barrier)
    const float* pl = p.plse + row * S;
    int h;
    long long orow;
    if (!kv_combine_row(p, row, pl, h, orow)) return;
    float m = -INFINITY;
    for (int s = c; s < S; s += 64) m = fmaxf(m, pl[s]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int s = c; s < S; s += 64) {
        const float ls = pl[s];
        const float wgt = (ls == -INFINITY) ? 0.f : __expf(ls - m);
        wsh[wv][s] = wgt;
        sum += wgt;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
    for (int j = 0; j < DV / 256; ++j) {
        const int col = 256 * j + 4 * c;
        const float* po = p.po + row * S * DV + col;
        f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int s = 0; s < S; ++s) {
            const float wgt = wsh[wv][s];
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(po + (size_t)s * DV);
            acc += (wgt != 0.f) ? wgt * x : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        u32x2 v;
        v[0] = pack2_rn<Tag>(acc[0] * inv, acc[1] * inv);
        v[1] = pack2_rn<Tag>(acc[2] * inv, acc[3] * inv);
        *reinterpret_cast<u32x2*>(p.o + orow * DV + col) = v;
    }
    if (c == 0) p.lse[row] = sum > 0.f ? m + logf(sum) : -INFINITY;
}

template <typename Tag, int NW>
hipError_t launch_mla_split(const MlaParams& mp, int S, int batch, hipStream_t st) {
    const int wg_tiles = (mp.p.rows + 16 * NW - 1) / (16 * NW);
    const dim3 grid((unsigned)S, (unsigned)(wg_tiles * mp.p.hkv), (unsigned)batch);
    if (mp.p.table) hipLaunchKernelGGL((mla_split_kernel<Tag, NW, true>), grid, dim3(64 * NW), 0, st, mp);
    else hipLaunchKernelGGL((mla_split_kernel<Tag, NW, false>), grid, dim3(64 * NW), 0, st, mp);
    return hipGetLastError();
}

template <typename Tag>
hipError_t launch_mla_t(const MlaParams& mp, int S, int batch, hipStream_t st) {
    const int nw = mla_waves(mp.p.rows);
    hipError_t e = nw == 1 ? launch_mla_split<Tag, 1>(mp, S, batch, st)
                 : nw == 2 ? launch_mla_split<Tag, 2>(mp, S, batch, st) : launch_mla_split<Tag, 4>(mp, S, batch, st);
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = (long long)batch * mp.p.hq * mp.p.nq;
    hipLaunchKernelGGL((mla_combine_kernel<Tag>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, mp.p, S, nrows);
    return hipGetLastError();
}

// ---- sparse MLA (fa_mla_sparse_forward): the keys of a (sequence b, query token i, K/V head hk) are the topk entries of a list
// of token positions.  mla_sparse_kernel is mla_split_kernel with another producer of ko / vo: a workgroup serves one list
// (blockIdx.x = b * nq + i; its rows are the G heads of hk, 16 a wave), a tile is 32 list positions, and from ko / vo on the copy
// is the PAGED branch of load_lat / load_rot there (wave-uniform latent row through v_readlane, 16 bytes a lane, MlaSwz image).
// Lane l holds entry j0 + (l & 31): one coalesced 128-byte read two tiles ahead of its use; a tile ahead the lane decides
// visibility (0 <= entry < len_b, and <= len_b - nq + i if causal) and, paged, looks up its page.  An entry that is not visible
// is never turned into an address: its row is zeros in LDS and its score is -inf by the tile's 32-bit ballot of the per-key flag.
// A visible entry on a page outside the pool or in a cache row outside the cache is a zero row too, with score 0 (the page rule
// of fa_decode.hip).  Splits cut the list positions [0, topk) into ranges of whole tiles; partials and mla_combine_kernel as above.
struct MlaSparseParams {
    MlaParams mp;          // mp.p.nq: the query tokens of a sequence (the window fields are not used)
    const int* idx;        // entry j of (b, i, hk): idx[b * ix_bs + i * ix_ts + hk * ix_hs + j]; untrusted device memory
    long long ix_bs, ix_ts, ix_hs;
    int topk, causal;
};

template <typename Tag, int NW, bool PAGED>
__global__ __launch_bounds__(64 * NW) void mla_sparse_kernel(MlaSparseParams sp) {
    constexpr int KT = kMlaKT, DK = kMlaDk, DV = kMlaDv, NDB = DV / 16, T = 64 * NW;
    constexpr int LCH = KT * (DV / 8) / T, RCH = KT * (DK / 8) / T;
    static_assert(LCH * T == KT * DV / 8 && RCH >= 1, "tile copy");
    __shared__ __attribute__((aligned(16))) char lds[kMlaLdsBytes];
    char* const lat = lds;
    char* const rop = lds + kMlaLatBytes;
    const KvParams& p = sp.mp.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int s = blockIdx.y, S = gridDim.y;
    const int hk = blockIdx.z % p.hkv, wt = blockIdx.z / p.hkv;
    const int nq = p.nq, b = blockIdx.x / nq, qi = blockIdx.x - b * nq;
    int L_b, P_b;
    const int lk = kv_len_k(p, b, 0, L_b, P_b);
    // visible token positions: [0, tlim)
    const int thi = sp.causal ? lk - nq + qi : lk - 1;
    const unsigned tlim = thi >= 0 ? (unsigned)thi + 1u : 0u;
    // list positions [jbeg, jend) of split s: whole tiles
    const int nt = (sp.topk + KT - 1) / KT;
    const int jbeg = (int)((long long)s * nt / S) * KT, jend = min(sp.topk, (int)((long long)(s + 1) * nt / S) * KT);

    // this wave's row tile of the G heads (none: the wave only copies) and this lane's head
    const int pr0 = 16 * NW * wt + 16 * w, pr = pr0 + r;
    const bool active = pr0 < p.G, valid = pr < p.G;
    const int h = hk * p.G + (valid ? pr : 0);

    s16x8 qf[DK / 32], qvf[DV / 32];
    {
        const buf_rsrc_t q_rs = make_rsrc(p.q + b * p.q_bs, (unsigned)(((nq - 1) * p.q_ts + p.hq * DK) * 2));
        const buf_rsrc_t qv_rs = make_rsrc(sp.mp.qv + b * sp.mp.qv_bs, (unsigned)(((nq - 1) * sp.mp.qv_ts + p.hq * DV) * 2));
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks) qf[ks] = buf_load_frag(q_rs, valid ? (qi * p.q_ts + h * DK + 32 * ks + 8 * g) * 2 : kOobOff);
#pragma unroll
        for (int ks = 0; ks < DV / 32; ++ks) qvf[ks] = buf_load_frag(qv_rs, valid ? (qi * sp.mp.qv_ts + h * DV + 32 * ks + 8 * g) * 2 : kOobOff);
    }
    // contiguous: cache row (bidx ? bidx[b] : b); a row outside the cache holds zero rows
    long long crow = b;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = (unsigned)ix < (unsigned)p.bcache ? ix : -1;
    }
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    const int* il = sp.idx + b * sp.ix_bs + qi * sp.ix_ts + hk * sp.ix_hs;

    // The list pipeline of lane l (list position + (l & 31) of a tile): e2 the raw entry of the tile after next; s1 the next
    // tile's visible entry as its token position (contiguous) or its slot in its page pg1 (paged), -1 = not visible.
    int e2 = -1, s1 = -1, pg1 = -1;
    auto entry = [&](int jt) {
        const int pos = jt + (lane & 31);
        return pos < jend ? il[pos] : -1;
    };
    auto advance = [&](int jt) {   // e2 -> s1 (pg1); e2 = the entries of the tile at jt
        const bool vis = (unsigned)e2 < tlim;
        if constexpr (PAGED) {
            const unsigned j = (unsigned)e2 / (unsigned)p.ps;   // (< max_blocks_per_seq: e2 < len_b <= the capacity)
            s1 = vis ? (int)((unsigned)e2 - j * (unsigned)p.ps) : -1;
            pg1 = vis ? tbl[j] : -1;
        } else {
            s1 = vis ? e2 : -1;
        }
        e2 = entry(jt);
    };
    if (jbeg < jend) {
        e2 = entry(jbeg);
        advance(jbeg + KT);
    }

    f32x4_t oacc[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t) oacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const int q4 = r >> 2, p4 = r & 3;

    // One tile's copy, as in mla_split_kernel<.., PAGED = true>: this lane's key has element offsets ko / vo in the two caches,
    // -1 = not fetched, zeros in LDS.  offsets() returns the tile's visibility flags, bit k = list position kt + k.
    constexpr bool PRE = LCH <= 8;
    constexpr int LB = PRE ? LCH : 8;
    static_assert(LCH % LB == 0, "tile copy");
    u32x4 xl[LB], xr[RCH];
    long long ko = -1, vo = -1;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    auto offsets = [&](int kt) {
        ko = vo = -1;
        if constexpr (PAGED) {
            if (s1 >= 0 && (unsigned)pg1 < (unsigned)p.nblk) {
                ko = pg1 * p.kc_bs + (long long)s1 * p.kc_ts;
                vo = pg1 * p.vc_bs + (long long)s1 * p.vc_ts;
            }
        } else if (s1 >= 0 && crow >= 0) {
            ko = crow * p.kc_bs + (long long)s1 * p.kc_ts;
            vo = crow * p.vc_bs + (long long)s1 * p.vc_ts;
        }
        const unsigned vm = (unsigned)__ballot(s1 >= 0);
        advance(kt + 2 * KT);
        return vm;
    };
    auto load_lat = [&](int i0) {
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            const int row = (T / 64) * (i0 + i) + wu;
            const long long ro = ((long long)__builtin_amdgcn_readlane((int)(vo >> 32), row) << 32) |
                                 (unsigned)__builtin_amdgcn_readlane((int)vo, row);   // (wave-uniform: a scalar base)
            const bool ok = ro >= 0;
            const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? p.vc + ro + hk * DV + 8 * lane : p.q);
            xl[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_lat = [&](int i0) {
#pragma unroll
        for (int i = 0; i < LB; ++i) *reinterpret_cast<u32x4*>(lat + MlaSwz::off((T / 64) * (i0 + i) + wu, lane)) = xl[i];
    };
    auto load_rot = [&]() {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid, row = idx >> 3, ch = idx & 7;
            const long long ro = __shfl(ko, row, 64);
            const bool ok = ro >= 0;
            const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? p.kc + ro + hk * DK + 8 * ch : p.q);
            xr[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_rot = [&]() {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid;
            *reinterpret_cast<u32x4*>(rop + TileSwz<64>::off(idx >> 3, idx & 7)) = xr[i];
        }
    };
    unsigned vm_next = 0u;
    if (PRE && jbeg < jend) {
        vm_next = offsets(jbeg);
        load_lat(0);
        load_rot();
    }

    for (int k0 = jbeg; k0 < jend; k0 += KT) {
        unsigned vm = vm_next;
        if constexpr (!PRE) vm = offsets(k0);
        __syncthreads();   // every wave has read the previous tile
        if constexpr (PRE) {
            store_lat(0);
        } else {
#pragma unroll 1
            for (int i0 = 0; i0 < LCH; i0 += LB) {
                load_lat(i0);
                store_lat(i0);
            }
            load_rot();
        }
        store_rot();
        __syncthreads();
        if (PRE && k0 + KT < jend) {
            vm_next = offsets(k0 + KT);
            load_lat(0);
            load_rot();
        }
        if (!active) continue;   // (wave-uniform; the wave still takes part in the copies and the barriers)

        // S^T = K Q^T, as in mla_split_kernel
        f32x4_t sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < DK / 32; ++ks)
                sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(rop + TileSwz<64>::off(16 * kb + r, 4 * ks + g)), qf[ks], sacc[kb]);
#pragma unroll
            for (int ks = 0; ks < DV / 32; ++ks) {
                if (ks % 4 == 0) __builtin_amdgcn_sched_barrier(0);
                sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(lat + MlaSwz::off(16 * kb + r, 4 * ks + g)), qvf[ks], sacc[kb]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
        // the list's flags: register i of block kb holds list position k0 + 16 kb + 4 g + i
        const unsigned vg = valid ? vm >> (4 * g) : 0u;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = ((vg >> (16 * kb + i)) & 1u) ? sacc[kb][i] : -INFINITY;
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
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            if (t % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            const int ch = 2 * t + (p4 >> 1), bo = 8 * (p4 & 1);
            const s16x4 lo = lds_tr16(lat + MlaSwz::off(4 * g + q4, ch) + bo);
            const s16x4 hi = lds_tr16(lat + MlaSwz::off(16 + 4 * g + q4, ch) + bo);
            oacc[t] = mfma16<Tag>(cat8(lo, hi), pb, oacc[t]);
        }
    }

    // ---- epilogue (mla_split_kernel's)
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const float lse_v = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if (!valid) return;
    const size_t row_id = ((size_t)b * p.hq + h) * nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + ((size_t)blockIdx.x * p.hq + h) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            u32x2 v;
            v[0] = pack2_rn<Tag>(oacc[t][0] * inv, oacc[t][1] * inv);
            v[1] = pack2_rn<Tag>(oacc[t][2] * inv, oacc[t][3] * inv);
            *reinterpret_cast<u32x2*>(orow + 16 * t + 4 * g) = v;
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) *reinterpret_cast<f32x4_t*>(prow + 16 * t + 4 * g) = oacc[t] * inv;
        if (g == 0) p.plse[row_id * S + s] = lse_v;
    }
}

template <typename Tag, int NW>
hipError_t launch_mla_sparse_split(const MlaSparseParams& sp, int S, long long units, hipStream_t st) {
    const int wg_tiles = (sp.mp.p.G + 16 * NW - 1) / (16 * NW);
    const dim3 grid((unsigned)units, (unsigned)S, (unsigned)(wg_tiles * sp.mp.p.hkv));
    if (sp.mp.p.table) hipLaunchKernelGGL((mla_sparse_kernel<Tag, NW, true>), grid, dim3(64 * NW), 0, st, sp);
    else hipLaunchKernelGGL((mla_sparse_kernel<Tag, NW, false>), grid, dim3(64 * NW), 0, st, sp);
    return hipGetLastError();
}

template <typename Tag>
hipError_t launch_mla_sparse_t(const MlaSparseParams& sp, int S, long long units, hipStream_t st) {
    const int nw = mla_waves(sp.mp.p.G);
    hipError_t e = nw == 1 ? launch_mla_sparse_split<Tag, 1>(sp, S, units, st)
                 : nw == 2 ? launch_mla_sparse_split<Tag, 2>(sp, S, units, st) : launch_mla_sparse_split<Tag, 4>(sp, S, units, st);
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = units * sp.mp.p.hq;
    hipLaunchKernelGGL((mla_combine_kernel<Tag>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, sp.mp.p, S, nrows);
    return hipGetLastError();
}

}  // namespace

// Waves a workgroup: one per 16-row tile of the rows = G * Nq packed rows of a (sequence, K/V head), at most four (one per SIMD)
int mla_waves(int64_t rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : 4; }

// kv_num_splits for mla_split_kernel.  A unit is a workgroup of mla_waves(rows) waves over 16 * waves rows, not a wave over 16.
// The 16 x 512 fp32 accumulator beside the q and qv fragments takes a wave past 256 registers, so one wave runs per SIMD and a
// CU holds 4 / waves workgroups (36 KiB of LDS each).  Enough splits to fill the 256 CUs once, none shorter than 128 keys, at
// most 256 (the combine's weight row).
int mla_num_splits(int64_t batch, int64_t heads_kv, int64_t rows, int64_t cache_len) {
    constexpr int64_t kCUs = 256, kMinKeys = 128;
    if (rows <= 0) return 1;
    const int64_t nw = mla_waves(rows), per_cu = 4 / nw;
    const int64_t units = batch * heads_kv * ((rows + 16 * nw - 1) / (16 * nw));
    if (units <= 0 || cache_len <= 0) return 1;
    int64_t s = (kCUs * per_cu + units - 1) / units;
    s = std::min<int64_t>(s, (cache_len + kMinKeys - 1) / kMinKeys);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, 256));
}

// mla_num_splits for mla_sparse_kernel, with its constants.  A unit is a workgroup of mla_waves(group) waves over 16 * waves of the
// group heads of one list (units = batch * seqlen_q lists a K/V head); the splits cut the topk list positions, none shorter than
// 128 entries.
int mla_sparse_num_splits(int64_t units, int64_t heads_kv, int64_t group, int64_t topk) {
    constexpr int64_t kCUs = 256, kMinKeys = 128;
    if (group <= 0) return 1;
    const int64_t nw = mla_waves(group), per_cu = 4 / nw;
    const int64_t wgs = units * heads_kv * ((group + 16 * nw - 1) / (16 * nw));
    if (wgs <= 0 || topk <= 0) return 1;
    int64_t s = (kCUs * per_cu + wgs - 1) / wgs;
    s = std::min<int64_t>(s, (topk + kMinKeys - 1) / kMinKeys);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, 256));
}

hipError_t launch_mla_sparse(const MlaSparseArgs& a, hipStream_t st) {
    const KvArgs& kv = a.kv;
    if (kv.d != kMlaDk || kv.d_v != kMlaDv) return hipErrorInvalidValue;   // (the C layer's check)
    MlaSparseParams sp;
    sp.mp.p = kv_make_params(kv);
    sp.mp.qv = (const uint16_t*)kv.qv; sp.mp.qv_bs = kv.qv_bs; sp.mp.qv_ts = (int)kv.qv_ts;
    sp.idx = a.indices; sp.ix_bs = a.ix_bs; sp.ix_ts = a.ix_ts; sp.ix_hs = a.ix_hs;
    sp.topk = (int)a.topk; sp.causal = kv.causal;
    const int S = (int)kv.num_splits;
    // workspace (S > 1): kv_workspace_bytes at d_v, the O partials and then the lse partials
    const size_t q_rows = (size_t)kv.batch * kv.heads_q * kv.seqlen_q;
    sp.mp.p.po = (float*)kv.workspace;
    sp.mp.p.plse = S > 1 ? (float*)((char*)kv.workspace + ((q_rows * S * kMlaDv * 4 + 255) & ~(size_t)255)) : nullptr;
    const long long units = (long long)kv.batch * kv.seqlen_q;
    return kv.dtype == 1 ? launch_mla_sparse_t<f16_tag>(sp, S, units, st) : launch_mla_sparse_t<bf16_tag>(sp, S, units, st);
}

hipError_t launch_kvcache_mla(const KvArgs& a, hipStream_t st) {
    if (a.d != kMlaDk || a.d_v != kMlaDv) return hipErrorInvalidValue;   // (the C layer's check)
    MlaParams mp;
    mp.p = kv_make_params(a);
    mp.qv = (const uint16_t*)a.qv; mp.qv_bs = a.qv_bs; mp.qv_ts = (int)a.qv_ts;
    const int S = (int)a.num_splits;
    // workspace (S > 1): kv_workspace_bytes at d_v, the O partials and then the lse partials
    const size_t q_rows = (size_t)a.batch * a.heads_q * a.seqlen_q;
    mp.p.po = (float*)a.workspace;
    mp.p.plse = S > 1 ? (float*)((char*)a.workspace + ((q_rows * S * kMlaDv * 4 + 255) & ~(size_t)255)) : nullptr;
    return a.dtype == 1 ? launch_mla_t<f16_tag>(mp, S, (int)a.batch, st) : launch_mla_t<bf16_tag>(mp, S, (int)a.batch, st);
}

// ---- the packed 8-bit latent cache (fa_mla_fp8_forward, fa_mla_fp8_pack): FlashMLA's 656-byte token
//   byte 0 .. 511: 512 e4m3 (the latent, quantised per 128-wide tile) | 512 .. 527: 4 float32 scales | 528 .. 655: 64 bf16 (rotary)
// in a paged pool, token t of sequence b at pool + page * page_sb + (t % ps) * tok_sb bytes (64-bit), one K/V head, bf16 only.
// mla_f8_kernel<NW, SPARSE> is mla_split_kernel<bf16_tag, NW, true> (SPARSE: mla_sparse_kernel<bf16_tag, NW, true>) with another
// copy into the same 36 KiB LDS image; from the barrier after the copy on the two are the same text, so a call on a pool gives
// the bits of the 16-bit call on the pool's dequantised rows.  The copy: row tid / TPR of the tile belongs to TPR = T / 32
// threads; a thread loads the row's four scales (one 16-byte load) and its 16-byte chunks c = tid % TPR + TPR i of e4m3 (16 head
// dims of the 128-wide tile c / 8), and writes for each the two MlaSwz chunks 2c, 2c + 1 of
//   bf16_rne(fp32(e4m3) * scale)    (one exact widening, one fp32 multiply, one rounding to nearest even).
// The rotary 128 bytes are 8 chunks, copied as there.  A row that is not fetched (its loads are redirected to the first bytes of
// q and their results selected away, as in the 16-bit kernels: no address is formed from the key) has zero bytes and zero
// scales: zeros.  Four waves: a thread holds 4 + 1 + 1 chunks of tile t + 1 while tile t is computed on.
// The text shared with mla_split_kernel / mla_sparse_kernel carries their comments; a change to the loop there belongs here too
// (tests/test_mla_fp8_gpu.py holds the two to the same bits).
namespace {

constexpr int kF8Scales = 512, kF8Rope = 528;   // byte offsets in a token (656 bytes)

struct MlaF8Params {
    MlaSparseParams sp;    // sp.mp.p.kc / vc are not used; sp.idx, topk: SPARSE only
    const unsigned char* pool;
    long long page_sb;     // bytes from page to page
    int tok_sb;            // bytes from token to token of a page
    int q_hs, qv_hs;       // head strides of q and qv (elements): the two column ranges of one (.., 576) tensor are 576 apart
};

// 16 e4m3 bytes times one scale -> the two 16-byte chunks of bf16 they fill
__device__ __forceinline__ void mla_f8_widen(u32x4 x, float sc, u32x4& lo, u32x4& hi) {
    uint32_t out[8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[d], false);
        const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[d], true);
        out[2 * d] = pack2<bf16_tag>(a[0] * sc, a[1] * sc);
        out[2 * d + 1] = pack2<bf16_tag>(b[0] * sc, b[1] * sc);
    }
    lo = u32x4{out[0], out[1], out[2], out[3]};
    hi = u32x4{out[4], out[5], out[6], out[7]};
}

template <int NW, bool SPARSE>
__global__ __launch_bounds__(64 * NW) void mla_f8_kernel(MlaF8Params fp) {
    using Tag = bf16_tag;
    constexpr int KT = kMlaKT, DK = kMlaDk, DV = kMlaDv, NDB = DV / 16, T = 64 * NW;
    constexpr int TPR = T / KT, FCH = (DV / 16) / TPR, RCH = KT * (DK / 8) / T;   // threads a latent row; 16-byte chunks a thread: e4m3, rotary
    static_assert(TPR * FCH * 16 == DV && 8 % TPR == 0 && RCH >= 1, "tile copy");
    __shared__ __attribute__((aligned(16))) char lds[kMlaLdsBytes];
    char* const lat = lds;
    char* const rop = lds + kMlaLatBytes;
    const MlaSparseParams& sp = fp.sp;
    const KvParams& p = sp.mp.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int s = SPARSE ? blockIdx.y : blockIdx.x, S = SPARSE ? gridDim.y : gridDim.x;
    const int wt = SPARSE ? blockIdx.z : blockIdx.y;
    const int nq = p.nq, b = SPARSE ? blockIdx.x / nq : blockIdx.z;
    int L_b, P_b;
    const int lk = kv_len_k(p, b, 0, L_b, P_b);   // (one K/V head: hk = 0 throughout)

    // the positions [kbeg, kend) of this split (keys, SPARSE: list positions), this wave's row tile (none: the wave only
    // copies), this lane's query row: mla_split_kernel's, SPARSE mla_sparse_kernel's
    int kbeg, kend, qi, h, rlo = 0, rhi = -1;
    bool active, valid;
    unsigned tlim = 0u;
    if constexpr (SPARSE) {
        qi = blockIdx.x - b * nq;
        // visible token positions: [0, tlim)
        const int thi = sp.causal ? lk - nq + qi : lk - 1;
        tlim = thi >= 0 ? (unsigned)thi + 1u : 0u;
        // list positions [kbeg, kend) of split s: whole tiles
        const int nt = (sp.topk + KT - 1) / KT;
        kbeg = (int)((long long)s * nt / S) * KT;
        kend = min(sp.topk, (int)((long long)(s + 1) * nt / S) * KT);
        // this wave's row tile of the G heads (none: the wave only copies) and this lane's head
        const int pr0 = 16 * NW * wt + 16 * w, pr = pr0 + r;
        active = pr0 < p.G;
        valid = pr < p.G;
        h = valid ? pr : 0;
    } else {
        const int rows = p.rows, coff = lk - nq;
        // the workgroup's rows [wr0, wr1) and the key range of their bands' union; wr0 < rows by the grid
        const int wr0 = 16 * NW * wt, wr1 = min(wr0 + 16 * NW, rows);
        kv_split_range(p, lk, nq, wr0 / p.G, (wr1 - 1) / p.G, s, S, kbeg, kend);
        // this wave's row tile (none: the wave only copies), this lane's query row and its visible keys [rlo, rhi]
        const int pr0 = wr0 + 16 * w, pr = pr0 + r;
        active = pr0 < rows;
        valid = pr < rows;
        const int qlo = min(pr0, rows - 1) / p.G;
        qi = valid ? pr / p.G : qlo;
        h = valid ? pr - qi * p.G : 0;
        rlo = max(qi + coff - p.wl, kbeg);
        rhi = valid ? min(min(qi + coff + p.wr, lk - 1), kend - 1) : -1;
    }

    s16x8 qf[DK / 32], qvf[DV / 32];
    {
        const buf_rsrc_t q_rs = make_rsrc(p.q + b * p.q_bs, (unsigned)(((nq - 1) * p.q_ts + (p.hq - 1) * fp.q_hs + DK) * 2));
        const buf_rsrc_t qv_rs = make_rsrc(sp.mp.qv + b * sp.mp.qv_bs, (unsigned)(((nq - 1) * sp.mp.qv_ts + (p.hq - 1) * fp.qv_hs + DV) * 2));
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks) qf[ks] = buf_load_frag(q_rs, valid ? (qi * p.q_ts + h * fp.q_hs + 32 * ks + 8 * g) * 2 : kOobOff);
#pragma unroll
        for (int ks = 0; ks < DV / 32; ++ks) qvf[ks] = buf_load_frag(qv_rs, valid ? (qi * sp.mp.qv_ts + h * fp.qv_hs + 32 * ks + 8 * g) * 2 : kOobOff);
    }
    const int* tbl = p.table + b * p.tbl_rs;

    // The producer of this lane's key (position + (lane & 31) of a tile).  Dense: kv_split_kernel's page lookup, done by every
    // wave for itself, the next tile's a tile ahead.  SPARSE: the list pipeline of mla_sparse_kernel: e2 the raw entry of the
    // tile after next (one coalesced 128-byte read), s1 the next tile's visible entry as its slot in its page pg1, -1 = not
    // visible: an entry that is not visible is never turned into an address.
    int j0 = 0, s0 = 0, pg = -1;
    int e2 = -1, s1 = -1, pg1 = -1;
    const int* il = nullptr;
    auto page_of = [&](int jt, int st, int kt) {
        int j = jt, sl = st + (lane & 31);
        if (sl >= p.ps) { sl -= p.ps; ++j; }
        if (sl >= p.ps) ++j;
        return kt + (lane & 31) < kend ? tbl[j] : -1;
    };
    auto entry = [&](int jt) {
        const int pos = jt + (lane & 31);
        return pos < kend ? il[pos] : -1;
    };
    auto advance = [&](int jt) {   // e2 -> s1, pg1; e2 = the entries of the tile at jt
        const bool vis = (unsigned)e2 < tlim;
        const unsigned j = (unsigned)e2 / (unsigned)p.ps;   // (< max_blocks_per_seq: e2 < len_b <= the capacity)
        s1 = vis ? (int)((unsigned)e2 - j * (unsigned)p.ps) : -1;
        pg1 = vis ? tbl[j] : -1;
        e2 = entry(jt);
    };
    if constexpr (SPARSE) {
        il = sp.idx + b * sp.ix_bs + qi * sp.ix_ts;
        if (kbeg < kend) {
            e2 = entry(kbeg);
            advance(kbeg + KT);
        }
    } else if (kbeg < kend) {
        j0 = kbeg / p.ps;
        s0 = kbeg - j0 * p.ps;
        pg = page_of(j0, s0, kbeg);
    }

    f32x4_t oacc[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t) oacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const int q4 = r >> 2, p4 = r & 3;

    // One tile's copy, loads and LDS writes apart.  to: the byte offset of this lane's token in the pool, -1 = reads as zeros
    // (past the split's end, not visible, or on a page outside the pool); offsets() returns the SPARSE tile's visibility flags.
    constexpr bool PRE = NW == 4;
    constexpr int FB = FCH < 8 ? FCH : 8;
    static_assert(FCH % FB == 0, "tile copy");
    u32x4 xl[FB], xs, xr[RCH];
    long long to = -1, lro = -1;
    const int lrow = tid / TPR, lc0 = tid % TPR;
    auto offsets = [&](int kt) {
        to = -1;
        unsigned vm = 0u;
        if constexpr (SPARSE) {
            if (s1 >= 0 && (unsigned)pg1 < (unsigned)p.nblk) to = pg1 * fp.page_sb + (long long)s1 * fp.tok_sb;
            vm = (unsigned)__ballot(s1 >= 0);
            advance(kt + 2 * KT);
        } else {
            int sl = s0 + (lane & 31);
            if (sl >= p.ps) sl -= p.ps;
            if (sl >= p.ps) sl -= p.ps;
            if ((unsigned)pg < (unsigned)p.nblk) to = pg * fp.page_sb + (long long)sl * fp.tok_sb;
            s0 += KT;
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (kt + KT < kend) pg = page_of(j0, s0, kt + KT);   // the next tile's lookup, a tile ahead of its use
        }
        return vm;
    };
    auto load_lat = [&](int i0) {
        if (i0 == 0) {
            lro = __shfl(to, lrow, 64);
            const u32x4 y = *reinterpret_cast<const u32x4*>(lro >= 0 ? fp.pool + lro + kF8Scales : (const unsigned char*)p.q);
            xs = lro >= 0 ? y : u32x4{0u, 0u, 0u, 0u};
        }
        const bool ok = lro >= 0;
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? fp.pool + lro + 16 * (lc0 + TPR * (i0 + i)) : (const unsigned char*)p.q);
            xl[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_lat = [&](int i0) {
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            const int c = lc0 + TPR * (i0 + i), tile = (TPR * (i0 + i)) >> 3;
            const uint32_t sb = tile == 0 ? xs[0] : tile == 1 ? xs[1] : tile == 2 ? xs[2] : xs[3];
            u32x4 lo, hi;
            mla_f8_widen(xl[i], __uint_as_float(sb), lo, hi);
            *reinterpret_cast<u32x4*>(lat + MlaSwz::off(lrow, 2 * c)) = lo;
            *reinterpret_cast<u32x4*>(lat + MlaSwz::off(lrow, 2 * c + 1)) = hi;
        }
    };
    auto load_rot = [&]() {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid, row = idx >> 3, ch = idx & 7;
            const long long ro = __shfl(to, row, 64);
            const bool ok = ro >= 0;
            const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? fp.pool + ro + kF8Rope + 16 * ch : (const unsigned char*)p.q);
            xr[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_rot = [&]() {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid;
            *reinterpret_cast<u32x4*>(rop + TileSwz<64>::off(idx >> 3, idx & 7)) = xr[i];
        }
    };
    unsigned vm_next = 0u;
    if (PRE && kbeg < kend) {
        vm_next = offsets(kbeg);
        load_lat(0);
        load_rot();
    }

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        unsigned vm = vm_next;
        if constexpr (!PRE) vm = offsets(k0);
        __syncthreads();   // every wave has read the previous tile
        if constexpr (PRE) {
            store_lat(0);
        } else {
#pragma unroll 1
            for (int i0 = 0; i0 < FCH; i0 += FB) {
                load_lat(i0);
                store_lat(i0);
            }
            load_rot();
        }
        store_rot();
        __syncthreads();
        if (PRE && k0 + KT < kend) {
            vm_next = offsets(k0 + KT);
            load_lat(0);
            load_rot();
        }
        if (!active) continue;   // (wave-uniform; the wave still takes part in the copies and the barriers)

        // ---- from here to the end: mla_split_kernel's text (SPARSE: mla_sparse_kernel's mask)
        // S^T = K Q^T: A = key 16 kb + r, head dims 32 ks + 8 g .. of the rotary row, then of the latent row
        f32x4_t sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < DK / 32; ++ks)
                sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(rop + TileSwz<64>::off(16 * kb + r, 4 * ks + g)), qf[ks], sacc[kb]);
#pragma unroll
            for (int ks = 0; ks < DV / 32; ++ks) {
                // (four operand reads in flight: hipcc would otherwise hoist all of a tile's reads and spill)
                if (ks % 4 == 0) __builtin_amdgcn_sched_barrier(0);
                sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(lat + MlaSwz::off(16 * kb + r, 4 * ks + g)), qvf[ks], sacc[kb]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // both score tiles live in VGPRs at one point (kv_split_kernel: the second chain must not end in the first one's registers)
        asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
        // register i of block kb holds position k0 + 16 kb + 4 g + i: the row's band [rlo, rhi], SPARSE the list's flags
        const unsigned vg = valid ? vm >> (4 * g) : 0u;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bool vis;
                if constexpr (SPARSE) {
                    vis = (vg >> (16 * kb + i)) & 1u;
                } else {
                    const int key = k0 + 16 * kb + 4 * g + i;
                    vis = key >= rlo && key <= rhi;
                }
                const float x = vis ? sacc[kb][i] : -INFINITY;
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
        // V^T operand from the same latent image: rows (keys) 4 g + q and 16 + 4 g + q, head dims 16 t + 4 p ..
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            if (t % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            const int ch = 2 * t + (p4 >> 1), bo = 8 * (p4 & 1);
            const s16x4 lo = lds_tr16(lat + MlaSwz::off(4 * g + q4, ch) + bo);
            const s16x4 hi = lds_tr16(lat + MlaSwz::off(16 + 4 * g + q4, ch) + bo);
            oacc[t] = mfma16<Tag>(cat8(lo, hi), pb, oacc[t]);
        }
    }

    // ---- epilogue (kv_split_kernel's): O^T register i of block t is head dim 16 t + 4 g + i
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const float lse_v = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if (!valid) return;
    const size_t row_id = ((size_t)b * p.hq + h) * nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + (((size_t)b * nq + qi) * p.hq + h) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            u32x2 v;
            v[0] = pack2_rn<Tag>(oacc[t][0] * inv, oacc[t][1] * inv);
            v[1] = pack2_rn<Tag>(oacc[t][2] * inv, oacc[t][3] * inv);
            *reinterpret_cast<u32x2*>(orow + 16 * t + 4 * g) = v;
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) *reinterpret_cast<f32x4_t*>(prow + 16 * t + 4 * g) = oacc[t] * inv;
        if (g == 0) p.plse[row_id * S + s] = lse_v;
    }
}

template <int NW>
hipError_t launch_mla_f8_split(const MlaF8Params& fp, bool sparse, int S, int batch, hipStream_t st) {
    const KvParams& p = fp.sp.mp.p;
    if (sparse) {
        const dim3 grid((unsigned)(batch * p.nq), (unsigned)S, (unsigned)((p.G + 16 * NW - 1) / (16 * NW)));
        hipLaunchKernelGGL((mla_f8_kernel<NW, true>), grid, dim3(64 * NW), 0, st, fp);
    } else {
        const dim3 grid((unsigned)S, (unsigned)((p.rows + 16 * NW - 1) / (16 * NW)), (unsigned)batch);
        hipLaunchKernelGGL((mla_f8_kernel<NW, false>), grid, dim3(64 * NW), 0, st, fp);
    }
    return hipGetLastError();
}

// fa_mla_fp8_pack: one wave a new token.  Lane l holds 8 latent elements of tile l / 16: amax over the tile's 16 lanes,
// scale = amax > 0 ? amax / 448 : 1 (pow2: rounded up to a power of two), byte = e4m3_rne(clamp(x / scale, +-448)) with both
// divisions IEEE-rounded; 8 bytes a lane, the four scales one 16-byte store of lane 0, the rotary 128 bytes by lanes 0 .. 7.
// The token goes to position cache_seqlens[b] + i through the table; a negative length, a position at or past the table's
// capacity or a page outside the pool drops it: nothing is written.  The power of two is taken in the bit pattern (a mantissa
// that is not zero: the next exponent), exact for every normal scale below 2^127; a subnormal scale would go to 2^-126 and one
// in the top binade to +inf, where tests/mla_fp8_ref.py (frexp / ldexp) differs: amax below 448 * 2^-126 or above 448 * 2^127,
// outside the contract as NaN and infinity are (values in [2^-6, 8] give scales in [2^-15, 2^-5]).
struct MlaF8PackParams {
    const uint16_t *lat, *rope;
    unsigned char* pool;
    const int *seqlens, *table;
    long long lat_bs, lat_ts, rope_bs, rope_ts, page_sb, tok_sb, tbl_rs, tokens;
    int nnew, nblk, ps, mb, pow2;
};

__global__ __launch_bounds__(256) void mla_f8_pack_kernel(MlaF8PackParams a) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.tokens) return;   // (wave-uniform, as everything up to the loads)
    const long long b = t / a.nnew;
    const int i = (int)(t - b * a.nnew);
    const int len = a.seqlens[b];
    const long long pos = (long long)len + i;
    if (len < 0 || pos >= (long long)a.mb * a.ps) return;
    const int j = (int)(pos / a.ps), slot = (int)(pos - (long long)j * a.ps);
    const int pg = a.table[b * a.tbl_rs + j];
    if ((unsigned)pg >= (unsigned)a.nblk) return;
    unsigned char* dst = a.pool + pg * a.page_sb + slot * a.tok_sb;

    const u32x4 x = *reinterpret_cast<const u32x4*>(a.lat + b * a.lat_bs + i * a.lat_ts + 8 * lane);
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = unpack_lo<bf16_tag>(x[k]);
        v[2 * k + 1] = unpack_hi<bf16_tag>(x[k]);
    }
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(v[k]));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    float scale = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
    if (a.pow2) {
        uint32_t bits = __float_as_uint(scale);
        if (bits & 0x007fffffu) bits = (bits & 0x7f800000u) + 0x00800000u;
        scale = __uint_as_float(bits);
    }
    float y[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = fminf(fmaxf(__fdiv_rn(v[k], scale), -448.f), 448.f);
    u32x2 q8;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * k], y[4 * k + 1], 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * k + 2], y[4 * k + 3], c, true);
        q8[k] = (uint32_t)c;
    }
    *reinterpret_cast<u32x2*>(dst + 8 * lane) = q8;
    u32x4 sc;
#pragma unroll
    for (int k = 0; k < 4; ++k) sc[k] = __float_as_uint(__shfl(scale, 16 * k, 64));
    if (lane == 0) *reinterpret_cast<u32x4*>(dst + kF8Scales) = sc;
    if (lane < 8)
        *reinterpret_cast<u32x4*>(dst + kF8Rope + 16 * lane) = *reinterpret_cast<const u32x4*>(a.rope + b * a.rope_bs + i * a.rope_ts + 8 * lane);
}

}  // namespace

hipError_t launch_mla_f8(const MlaF8Args& a, hipStream_t st) {
    const KvArgs& kv = a.sa.kv;
    if (kv.d != kMlaDk || kv.d_v != kMlaDv || kv.dtype != 2 || kv.heads_kv != 1 || !kv.block_table) return hipErrorInvalidValue;   // (the C layer's checks)
    const bool sparse = a.sa.indices != nullptr;
    MlaF8Params fp;
    fp.sp.mp.p = kv_make_params(kv);
    fp.sp.mp.qv = (const uint16_t*)kv.qv; fp.sp.mp.qv_bs = kv.qv_bs; fp.sp.mp.qv_ts = (int)kv.qv_ts;
    fp.sp.idx = a.sa.indices; fp.sp.ix_bs = a.sa.ix_bs; fp.sp.ix_ts = a.sa.ix_ts; fp.sp.ix_hs = 0;
    fp.sp.topk = (int)a.sa.topk; fp.sp.causal = kv.causal;
    fp.pool = (const unsigned char*)a.pool; fp.page_sb = a.page_sb; fp.tok_sb = (int)a.tok_sb;
    fp.q_hs = (int)a.q_hs; fp.qv_hs = (int)a.qv_hs;
    const int S = (int)kv.num_splits;
    KvParams& p = fp.sp.mp.p;
    const size_t q_rows = (size_t)kv.batch * kv.heads_q * kv.seqlen_q;
    p.po = (float*)kv.workspace;
    p.plse = S > 1 ? (float*)((char*)kv.workspace + ((q_rows * S * kMlaDv * 4 + 255) & ~(size_t)255)) : nullptr;
    const int nw = mla_waves(sparse ? p.G : p.rows);
    hipError_t e = nw == 1 ? launch_mla_f8_split<1>(fp, sparse, S, (int)kv.batch, st)
                 : nw == 2 ? launch_mla_f8_split<2>(fp, sparse, S, (int)kv.batch, st) : launch_mla_f8_split<4>(fp, sparse, S, (int)kv.batch, st);
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = (long long)q_rows;
    hipLaunchKernelGGL((mla_combine_kernel<bf16_tag>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, p, S, nrows);
    return hipGetLastError();
}

hipError_t launch_mla_f8_pack(const MlaF8PackArgs& a, hipStream_t st) {
    MlaF8PackParams k;
    k.lat = (const uint16_t*)a.latent; k.rope = (const uint16_t*)a.rope; k.pool = (unsigned char*)a.pool;
    k.seqlens = a.cache_seqlens; k.table = a.block_table;
    k.lat_bs = a.lat_bs; k.lat_ts = a.lat_ts; k.rope_bs = a.rope_bs; k.rope_ts = a.rope_ts;
    k.page_sb = a.page_sb; k.tok_sb = a.tok_sb; k.tbl_rs = a.table_row_stride; k.tokens = a.batch * a.seqlen_new;
    k.nnew = (int)a.seqlen_new; k.nblk = (int)a.num_blocks; k.ps = (int)a.page_size; k.mb = (int)a.max_blocks; k.pow2 = a.scale_pow2 ? 1 : 0;
    hipLaunchKernelGGL(mla_f8_pack_kernel, dim3((unsigned)((k.tokens + 3) / 4)), dim3(256), 0, st, k);
    return hipGetLastError();
}

}  // namespace fa
