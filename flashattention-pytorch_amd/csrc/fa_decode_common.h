// What the KV-cache decode kernels share (fa_decode.hip and fa_mla.hip): the kernel parameter block, the clamps of the untrusted
// device lengths and offsets, the split rule and the combine's row lookup.  One definition, so that a split, a mask or a clamp
// is the same function in every kernel of the family.
#pragma once
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"

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
    // fa_ex_forward_kvcache_varlen (null: the padded call): untrusted device offsets of the packed q / k_new tokens
    const int *cu_q, *cu_kn;
    int total_q, max_q, total_kn;                 // tokens of q / o, the host's bound on nq_b, tokens of k_new / v_new
};

// One sequence's share of a packed tensor of total tokens, from untrusted offsets: its first token start = clamp(cu[b], 0, total)
// and its n = clamp(cu[b + 1] - cu[b], 0, min(cap, total - start)) tokens, so start + n <= total whatever cu holds.
// tests/kvcache_varlen_ref.py models this clamp.
__device__ __forceinline__ int kv_cu_range(const int* cu, int b, int total, int cap, int& start) {
    const long long c0 = cu[b], c1 = cu[b + 1];
    start = (int)min(max(c0, 0LL), (long long)total);
    return (int)min(max(c1 - c0, 0LL), (long long)min(cap, total - start));
}

// nq_b and the sequence's first packed q token (cu_seqlens_q), or the call's seqlen_q and token b * seqlen_q
__device__ __forceinline__ int kv_seq_q(const KvParams& p, int b, long long& start) {
    if (p.cu_q) {
        int st;
        const int n = kv_cu_range(p.cu_q, b, p.total_q, p.max_q, st);
        start = st;
        return n;
    }
    start = (long long)b * p.nq;
    return p.nq;
}

// nnew_b and the sequence's first packed k_new token (cu_seqlens_k_new), or the call's seqlen_new
__device__ __forceinline__ int kv_seq_new(const KvParams& p, int b, int& start) {
    if (p.cu_kn) return kv_cu_range(p.cu_kn, b, p.total_kn, p.cap, start);
    start = 0;
    return p.nnew;
}

// L_b (the cache_seqlens clamp), P_b (the cache_leftpad clamp: the sequence's first cache position) and len_k = L_b + nnew_b - P_b
// (nnew: the sequence's new tokens, kv_seq_new)
__device__ __forceinline__ int kv_len_k(const KvParams& p, int b, int nnew, int& L, int& P) {
    L = p.seqlens ? min(max(p.seqlens[b], 0), p.cap - nnew) : p.cap;
    P = p.leftpad ? min(max(p.leftpad[b], 0), L) : 0;
    return L + nnew - P;
}

// Keys [kbeg, kend) of split s of S for the row tile whose query tokens are [qlo, qhi]: the union of the rows' bands,
// [max(0, qlo + coff - wl), min(len_k, qhi + coff + wr + 1)) with coff = len_k - nq_b, cut into 32-key tiles from its start, tiles
// [floor(s nt / S), floor((s + 1) nt / S)) to split s.  Empty (kbeg >= kend) when the band is, or nt < S for some s.
// tests/test_kvcache_cpu.py models this rule.
__device__ __forceinline__ void kv_split_range(const KvParams& p, int lk, int nq, int qlo, int qhi, int s, int S, int& kbeg, int& kend) {
    constexpr int KT = 32;
    const int coff = lk - nq;
    const int lo = max(0, qlo + coff - p.wl), hi = min(lk, qhi + coff + p.wr + 1);
    const int nt = hi > lo ? (hi - lo + KT - 1) / KT : 0;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    kbeg = lo + t0 * KT;
    kend = min(hi, lo + t1 * KT);
}

// The combine's row -> its query head h and the index of its (token, head) row of o.  Padded: row = (b * hq + h) * nq + qi.
// Packed (cu_q): row = h * total_q + packed token, no sequence index; the host fills plse with kPlseFill bytes before the split
// kernel runs, every wave of which writes the lse partial of each row it owns, so a row whose first partial still holds the
// fill belongs to no sequence: false, and the wave leaves without writing.
constexpr int kPlseFill = 0xff;
__device__ __forceinline__ bool kv_combine_row(const KvParams& p, long long row, const float* pl, int& h, long long& orow) {
    if (p.cu_q) {
        h = (int)(row / p.total_q);
        orow = (row - (long long)h * p.total_q) * p.hq + h;
        return __float_as_uint(pl[0]) != 0xffffffffu;
    }
    const long long bh = row / p.nq;
    const int qi = (int)(row - bh * p.nq);
    h = (int)(bh % p.hq);
    orow = ((bh / p.hq) * p.nq + qi) * p.hq + h;
    return true;
}


// The kernel parameters of a call, all but the workspace pointers (po, plse), which depend on the width of o
inline KvParams kv_make_params(const KvArgs& a) {
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
    p.cu_q = a.cu_seqlens_q; p.cu_kn = a.cu_seqlens_k_new;
    p.total_q = (int)a.total_q; p.max_q = (int)a.max_seqlen_q; p.total_kn = (int)a.total_k_new;
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
    p.po = nullptr; p.plse = nullptr;
    return p;
}

}  // namespace

}  // namespace fa
