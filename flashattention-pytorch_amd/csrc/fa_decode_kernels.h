// The append and split kernels of KV-cache decoding (fa_decode.hip has the layout and what each feature means):
// kv_append_kernel<Tag, FEAT> and kv_split_kernel<Tag, D, PAGED, FEAT>, ordinary function bodies.  FEAT is a set of the bits
// below; the kernel's one argument, KvB<FEAT>, is KvParams, then KvRot with kKvRot, then KvQ8 with kKvQ8 (no struct changes
// layout), so an instantiation is one function of its own and a feature its FEAT lacks is a discarded `if constexpr` branch.
// Packed queries and new keys (fa_ex_forward_kvcache_varlen) are run-time null tests on p.cu_q / p.cu_kn in every instantiation.
#pragma once
#include <type_traits>

#include "fa_decode_common.h"

namespace fa {

namespace {

constexpr int kKvRot = 1, kKvQ8 = 2;   // rotary embedding of q and k_new (KvRot); an e4m3 cache with per-head scales (KvQ8)

// Rotary embedding (fa_ex_forward_kvcache_rotary)
struct KvRot {
    const uint16_t *cos, *sin;   // (seqlen_ro, rdim / 2) in q's dtype, 4-byte aligned, rows at the even strides cos_rs / sin_rs
    long long cos_rs, sin_rs;
    int rdim, inter, qseq;       // qseq: q token i at position L_b - P_b + i (causal or a window bound given), else all at L_b - P_b
};

// e4m3 cache (fa_ex_forward_kvcache_fp8).  The scale of (b, K/V head) is kd[b * bs + hk] (vd likewise); null = 1.0.  The
// KvParams cache pointers then address bytes, and the cache strides are in bytes as well.
struct KvQ8 {
    const float *kd, *vd;
    long long bs;
};

template <typename P> struct KvWithRot : P { KvRot ro; };
template <typename P> struct KvWithQ8 : P { KvQ8 q8; };
template <int FEAT> using KvBR = typename std::conditional<(FEAT & kKvRot) != 0, KvWithRot<KvParams>, KvParams>::type;
template <int FEAT> using KvB = typename std::conditional<(FEAT & kKvQ8) != 0, KvWithQ8<KvBR<FEAT>>, KvBR<FEAT>>::type;
// what a cache stride counts
template <int FEAT> using KvCacheT = typename std::conditional<(FEAT & kKvQ8) != 0, uint8_t, uint16_t>::type;
static_assert(sizeof(KvParams) % 8 == 0 && sizeof(KvB<kKvRot>) == sizeof(KvParams) + 48 &&
                  sizeof(KvB<kKvQ8>) == sizeof(KvParams) + 24 && sizeof(KvB<kKvRot | kKvQ8>) == sizeof(KvParams) + 72,
              "KvB layout: each group behind every field of the one before, as when they were separate kernel arguments");

// the first head dim of the chunk that holds the other halves of the pairs of the chunk at col (col < rdim); not interleaved only
__device__ __forceinline__ int kv_rot_partner(const KvRot& ro, int col) {
    const int half = ro.rdim >> 1;
    return col < half ? col + half : col - half;
}

// The chunk at head dims col .. col + 7 (col < rdim) of a token at table row pos, rotated: own = the chunk, par = its partner
// chunk (not interleaved; unused otherwise).  See the head of fa_decode.hip.
template <typename Tag>
__device__ __forceinline__ u32x4 kv_rotate_chunk(const KvRot& ro, long long pos, int col, u32x4 own, u32x4 par) {
    u32x4 out;
    if (ro.inter) {
        const uint32_t* cp = reinterpret_cast<const uint32_t*>(ro.cos + pos * ro.cos_rs + (col >> 1));
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(ro.sin + pos * ro.sin_rs + (col >> 1));
        const uint32_t c2[2] = {cp[0], cp[1]}, s2[2] = {sp[0], sp[1]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = unpack_lo<Tag>(own[i]), y = unpack_hi<Tag>(own[i]);
            const float c = (i & 1) ? unpack_hi<Tag>(c2[i >> 1]) : unpack_lo<Tag>(c2[i >> 1]);
            const float sn = (i & 1) ? unpack_hi<Tag>(s2[i >> 1]) : unpack_lo<Tag>(s2[i >> 1]);
            out[i] = pack2_rn<Tag>(x * c - y * sn, x * sn + y * c);
        }
    } else {
        const int half = ro.rdim >> 1;
        const bool is_x = col < half;
        const int j0 = is_x ? col : col - half;
        const uint32_t* cp = reinterpret_cast<const uint32_t*>(ro.cos + pos * ro.cos_rs + j0);
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(ro.sin + pos * ro.sin_rs + j0);
        const float sgn = is_x ? -1.f : 1.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c2 = cp[i], s2 = sp[i];
            out[i] = pack2_rn<Tag>(unpack_lo<Tag>(own[i]) * unpack_lo<Tag>(c2) + unpack_lo<Tag>(par[i]) * (sgn * unpack_lo<Tag>(s2)),
                                   unpack_hi<Tag>(own[i]) * unpack_hi<Tag>(c2) + unpack_hi<Tag>(par[i]) * (sgn * unpack_hi<Tag>(s2)));
        }
    }
    return out;
}

// (kv_q8_widen, 8 e4m3 bytes -> 8 values of q's 16-bit dtype: fa_ex_common.h, shared with the paged varlen forward)
// 8 values of q's 16-bit dtype -> 8 e4m3 bytes: y = clamp(float(x) * inv, -448, 448) in fp32, then round to nearest even
// (v_cvt_pk_fp8_f32; after the clamp its saturation mode cannot matter, and a finite x never gives the NaN code)
template <typename Tag> __device__ __forceinline__ u32x2 kv_q8_quant(u32x4 x, float inv) {
    float y[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        y[2 * i] = fminf(fmaxf(unpack_lo<Tag>(x[i]) * inv, -448.f), 448.f);
        y[2 * i + 1] = fminf(fmaxf(unpack_hi<Tag>(x[i]) * inv, -448.f), 448.f);
    }
    u32x2 out;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        int v = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w], y[4 * w + 1], 0, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w + 2], y[4 * w + 3], v, true);
        out[w] = (uint32_t)v;
    }
    return out;
}

// A chunk of 8 head dims of the cache as 8 values of q's 16-bit dtype: 16 bytes as they lie, or 8 e4m3 bytes widened
// (kv_q8_widen).  From a buffer range at byte offset off (kOobOff or past the range: zeros) ..
template <typename Tag, bool Q8> __device__ __forceinline__ u32x4 kv_chunk_buf(buf_rsrc_t rs, int off) {
    if constexpr (Q8) return kv_q8_widen<Tag>(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
    else return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
}
// .. or from an address (paged); !ok: at is some readable address and the chunk is zeros
// (V: u32x4, or s16x8 for an MFMA operand; the 16-bit select is done in V)
template <typename Tag, bool Q8, typename V> __device__ __forceinline__ V kv_chunk_at(const void* at, bool ok) {
    if constexpr (Q8) {
        const u32x2 x = *reinterpret_cast<const u32x2*>(at);
        return __builtin_bit_cast(V, kv_q8_widen<Tag>(ok ? x : u32x2{0u, 0u}));
    } else {
        const V x = *reinterpret_cast<const V*>(at);
        return ok ? x : V{};
    }
}

// Token L_b + n of batch element b (k_new[b, n], or row cu_k_new[b] + n of a packed k_new) goes to cache row
// (bidx ? bidx[b] : b) at position L_b + n, or through the table to
// pool[table[b, (L_b + n) / ps], (L_b + n) % ps]; a row or page outside the cache / pool drops the token.
// kKvRot: k_new[b, n] is rotated at position L_b - P_b + n on the way.  kKvQ8: the (rotated, rounded) 16-bit values are
// quantised, one 8-byte store a chunk.  Tag is k_new's dtype; FEAT 0 only copies 16 bytes and is instantiated once, with
// bf16_tag, for both dtypes (kv_launch).
template <typename Tag, int FEAT>
__global__ __launch_bounds__(256) void kv_append_kernel(KvB<FEAT> p) {
    constexpr bool ROT = (FEAT & kKvRot) != 0, Q8 = (FEAT & kKvQ8) != 0;
    const int cpr = p.d / 8;                                      // 16-byte chunks per head row
    const int b = blockIdx.y;
    int kn0, L, P;
    const int nnew = kv_seq_new(p, b, kn0);                       // packed k_new: nnew_b tokens from row kn0 (else N_new, 0)
    const long long per_b = (long long)nnew * p.hkv * cpr;
    kv_len_k(p, b, nnew, L, P);
    const long long kn_b = p.cu_kn ? (long long)kn0 * p.kn_ts : b * p.kn_bs, vn_b = p.cu_kn ? (long long)kn0 * p.vn_ts : b * p.vn_bs;
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
        u32x4 kx = *reinterpret_cast<const u32x4*>(p.kn + kn_b + (size_t)n * p.kn_ts + col);
        if constexpr (ROT) {
            if (8 * c < p.ro.rdim) {
                u32x4 par = kx;
                if (!p.ro.inter)
                    par = *reinterpret_cast<const u32x4*>(p.kn + kn_b + (size_t)n * p.kn_ts + (size_t)h * p.d +
                                                          kv_rot_partner(p.ro, 8 * c));
                kx = kv_rotate_chunk<Tag>(p.ro, L - P + n, 8 * c, kx, par);
            }
        }
        const u32x4 vx = *reinterpret_cast<const u32x4*>(p.vn + vn_b + (size_t)n * p.vn_ts + col);
        if constexpr (Q8) {
            const float kinv = 1.0f / (p.q8.kd ? p.q8.kd[b * p.q8.bs + h] : 1.0f);
            const float vinv = 1.0f / (p.q8.vd ? p.q8.vd[b * p.q8.bs + h] : 1.0f);
            uint8_t* kc8 = reinterpret_cast<uint8_t*>(p.kc);
            uint8_t* vc8 = reinterpret_cast<uint8_t*>(p.vc);
            *reinterpret_cast<u32x2*>(kc8 + unit * p.kc_bs + (size_t)pos * p.kc_ts + col) = kv_q8_quant<Tag>(kx, kinv);
            *reinterpret_cast<u32x2*>(vc8 + unit * p.vc_bs + (size_t)pos * p.vc_ts + col) = kv_q8_quant<Tag>(vx, vinv);
        } else {
            *reinterpret_cast<u32x4*>(p.kc + unit * p.kc_bs + (size_t)pos * p.kc_ts + col) = kx;
            *reinterpret_cast<u32x4*>(p.vc + unit * p.vc_bs + (size_t)pos * p.vc_ts + col) = vx;
        }
    }
}

// One wave: split blockIdx.x of gridDim.x, row tile blockIdx.y / hkv and K/V head blockIdx.y % hkv, batch element blockIdx.z.
// Lane l: query row r = l & 15 of the tile (S^T's column, O^T's column), lane group g = l >> 4 (4 keys of each 16-key block
// of S^T, 4 head-dim elements of each 16-wide block of O^T).  D: the padded tile width (64 | 128 | 256), p.d <= D.
// PAGED: keys are reached through p.table (see the head of fa_decode.hip); otherwise through one buffer range per wave.
// kKvRot: the q fragments are rotated (p.ro) before the key loop.
// kKvQ8: the cache holds e4m3 (p.q8: the scales of (b, hk)) and is addressed in bytes; each lane loads 8 bytes where it loaded
// 16 and widens them on their way into the 16-bit loop (kv_chunk_buf, kv_chunk_at).
template <typename Tag, int D, bool PAGED, int FEAT>
__global__ __launch_bounds__(64) void kv_split_kernel(KvB<FEAT> p) {
    constexpr bool ROT = (FEAT & kKvRot) != 0, Q8 = (FEAT & kKvQ8) != 0;
    constexpr int EB = Q8 ? 1 : 2;   // bytes a cache element
    constexpr int KT = 32, NKS = D / 32, NDB = D / 16, CPR = D / 8, VLD = KT * CPR / 64;
    __shared__ __attribute__((aligned(16))) char vs[KT * D * 2];   // V tile, [key][D] in the TileSwz<D> image
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int DR = p.d;
    // packed queries (p.cu_q): the sequence's nq_b tokens start at packed token tok0 and the grid is sized for max_seqlen_q, so
    // a wave whose row tile lies past the sequence's rows leaves before its first load.  Wave-uniform, scalar.
    long long tok0;
    const int nq = kv_seq_q(p, b, tok0), rows = p.G * nq;
    const int pr0 = 16 * rt, pr = pr0 + r;
    if (pr0 >= rows) return;
    int kn0, L_b, P_b;
    const int lk = kv_len_k(p, b, kv_seq_new(p, b, kn0), L_b, P_b), coff = lk - nq;
    const int qlo = pr0 / p.G, qhi = (min(pr0 + 16, rows) - 1) / p.G;
    int kbeg, kend;
    kv_split_range(p, lk, nq, qlo, qhi, s, S, kbeg, kend);

    // this lane's query row: token qi, query head h; its visible keys [rlo, rhi] (padding rows of the tile: none)
    const bool valid = pr < rows;
    const int qi = valid ? pr / p.G : qlo, h = hk * p.G + (valid ? pr - qi * p.G : 0);
    const int rlo = max(qi + coff - p.wl, kbeg);
    const int rhi = valid ? min(min(qi + coff + p.wr, lk - 1), kend - 1) : -1;
    float al = 0.f;
    if (p.alibi && valid) al = p.alibi[(size_t)b * p.al_bs + h] * p.sc.al_k;

    const buf_rsrc_t q_rs = make_rsrc(p.q + (p.cu_q ? tok0 * p.q_ts : b * p.q_bs), (unsigned)(((nq - 1) * p.q_ts + p.hq * DR) * 2));
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int col = 32 * ks + 8 * g;
        qf[ks] = buf_load_frag(q_rs, (valid && col < DR) ? (qi * p.q_ts + h * DR + col) * 2 : kOobOff);
    }
    if constexpr (ROT) {
        // fragment ks of this lane is the chunk at head dims 32 ks + 8 g of row (qi, h); rdim <= DR
        const long long qpos = L_b - P_b + (p.ro.qseq ? qi : 0);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int col = 32 * ks + 8 * g;
            if (valid && col < p.ro.rdim) {
                const u32x4 own = __builtin_bit_cast(u32x4, qf[ks]);
                u32x4 par = own;
                if (!p.ro.inter)
                    par = __builtin_bit_cast(u32x4, buf_load_frag(q_rs, (qi * p.q_ts + h * DR + kv_rot_partner(p.ro, col)) * 2));
                qf[ks] = __builtin_bit_cast(s16x8, kv_rotate_chunk<Tag>(p.ro, qpos, col, own, par));
            }
        }
    }
    // contiguous: the sequence's keys start P_b tokens into cache row (bidx ? bidx[b] : b); a row outside the cache is an empty range
    long long crow = b;
    int ctok = PAGED ? 0 : p.cap - P_b;   // tokens the buffer range holds
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; ctok = 0; }
    }
    const KvCacheT<FEAT>* kc = reinterpret_cast<const KvCacheT<FEAT>*>(p.kc);
    const KvCacheT<FEAT>* vc = reinterpret_cast<const KvCacheT<FEAT>*>(p.vc);
    [[maybe_unused]] float kdsc = 1.0f, vdsc = 1.0f;
    if constexpr (Q8) {
        kdsc = p.q8.kd ? p.q8.kd[b * p.q8.bs + hk] : 1.0f;
        vdsc = p.q8.vd ? p.q8.vd[b * p.q8.bs + hk] : 1.0f;
    }
    const buf_rsrc_t k_rs = make_rsrc(kc + crow * p.kc_bs + (long long)P_b * p.kc_ts,
                                      ctok > 0 ? (unsigned)(((ctok - 1) * p.kc_ts + p.hkv * DR) * EB) : 0u);
    const buf_rsrc_t v_rs = make_rsrc(vc + crow * p.vc_bs + (long long)P_b * p.vc_ts,
                                      ctok > 0 ? (unsigned)(((ctok - 1) * p.vc_ts + p.hkv * DR) * EB) : 0u);
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
            const KvCacheT<FEAT>* nowhere = reinterpret_cast<const KvCacheT<FEAT>*>(p.q);   // readable, for a chunk that is zeros
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const long long to = __shfl(ko, 16 * kb + r, 64);
                const KvCacheT<FEAT>* kp = kc + to + hk * DR + 8 * g;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bool ok = to >= 0 && 32 * ks + 8 * g < DR;
                    kf[kb][ks] = kv_chunk_at<Tag, Q8, s16x8>(ok ? kp + 32 * ks : nowhere, ok);
                }
            }
#pragma unroll
            for (int i = 0; i < VLD; ++i) {
                const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR;
                const long long to = __shfl(vo, row, 64);
                const bool ok = to >= 0 && 8 * ch < DR;
                vr[i] = kv_chunk_at<Tag, Q8, u32x4>(ok ? vc + to + hk * DR + 8 * ch : nowhere, ok);
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int key = k0 + 16 * kb + r;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const int col = 32 * ks + 8 * g;
                    const int off = (key < kend && col < DR) ? (key * p.kc_ts + hk * DR + col) * EB : kOobOff;
                    kf[kb][ks] = __builtin_bit_cast(s16x8, kv_chunk_buf<Tag, Q8>(k_rs, off));
                }
            }
#pragma unroll
            for (int i = 0; i < VLD; ++i) {
                const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR, key = k0 + row;
                vr[i] = kv_chunk_buf<Tag, Q8>(v_rs, (key < kend && 8 * ch < DR) ? (key * p.vc_ts + hk * DR + 8 * ch) * EB : kOobOff);
            }
        }
        f32x4_t sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) sacc[kb] = mfma16<Tag>(kf[kb][ks], qf[ks], sacc[kb]);
        }
        // both score tiles live in VGPRs at one point: without this hipcc ends the second chain in the first one's registers
        // (a[0:3] = .. + a[4:7]), a C operand that is not the destination, which tools/mfma_hazard_audit.py R1 does not pass
        // (the e4m3 kernels always did that; with the packed-query prologue the contiguous 16-bit D = 128 ones do as well)
        asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
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
                if constexpr (Q8) x *= kdsc;   // s = softmax_scale * k_descale * (q . k_stored): before softcap and ALiBi
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
    auto fin = [&](auto x) {   // an accumulator (or four) normalised, and descaled for an e4m3 V
        if constexpr (Q8) return x * inv * vdsc;
        else return x * inv;
    };
    // o row (token, h) of the (packed or padded) token tok0 + qi; lse / partials row (b, h, qi), packed (h, token)
    const size_t row_id = p.cu_q ? (size_t)h * p.total_q + tok0 + qi : ((size_t)b * p.hq + h) * p.nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + ((size_t)(tok0 + qi) * p.hq + h) * DR;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int col = 16 * t + 4 * g;
            if (col < DR) {
                u32x2 v;
                v[0] = pack2_rn<Tag>(fin(oacc[t][0]), fin(oacc[t][1]));
                v[1] = pack2_rn<Tag>(fin(oacc[t][2]), fin(oacc[t][3]));
                *reinterpret_cast<u32x2*>(orow + col) = v;
            }
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * DR;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int col = 16 * t + 4 * g;
            if (col < DR) *reinterpret_cast<f32x4_t*>(prow + col) = fin(oacc[t]);
        }
        if (g == 0) p.plse[row_id * S + s] = lse_v;
    }
}

}  // namespace

}  // namespace fa
