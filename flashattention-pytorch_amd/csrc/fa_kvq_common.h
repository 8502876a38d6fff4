// What the readers of a quantised KV cache share (fa_fp8_decode.hip, fa_fp4_decode.hip, fa_fp4_prefill.hip): the operand vector
// types, the 4 x 4 byte transpose, the MXFP4 V^T image, the featured kernel arguments with the one function that fills them, and
// the dtype x paged launch ladder.  One definition each.
#pragma once
#include <algorithm>
#include <type_traits>

#include "fa_decode_common.h"   // kv_cu_range, kPlseFill: the packed calls

namespace fa {

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef long long i64x4_t __attribute__((ext_vector_type(4)));   // four group bases, held as values (an array becomes an indexed scratch slot)

constexpr int kFp4 = 4;                                  // v_mfma_scale_f32_32x32x64_f8f6f4's format selector of e2m1 (0: e4m3)

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

// the MXFP4 V^T image: 32 key bytes a channel row, 16 bytes of padding after every eight rows (the bank argument: the header of
// fa_fp4_decode.hip; its size at head dim D: Fp4Hd<D>::VT, fa_fp4_common.h)
constexpr int kVt4Bytes = 32 * 128 + 16 * 16;           // at head dim 128
__device__ __forceinline__ int vt4_off(int row) { return 32 * row + 16 * (row >> 3); }

// What a featured instantiation takes beside its kernel's parameter block (the _mod calls; DESIGN.md sections 9zc, 9zi).  It is
// the kernel's argument pack Mod...: the plain instantiation has no such argument, and with its argument list keeps its instructions.
struct KvqMod {
    int wl, wr;                           // token i sees keys [i + coff - wl, i + coff + wr]; kWinNone: unbounded, wr = 0 if causal
    float cap_k, cap2;                    // 2 / softcap, softcap * log2(e); cap2 == 0: no softcap
};
// fp4kv_prefill_kernel's: it has no combine for the sinks to join in
struct KvqModSinks : KvqMod {
    const float* sinks;                   // one logit a query head (natural-log units), sinks[h % sink_heads]; null: none
    int sink_heads;
};

// the first argument of a kernel's pack Mod..., or for the plain instantiation (an empty pack) a value that nothing reads
template <typename M> __device__ __forceinline__ M kvq_mod_of() { return M{}; }
template <typename M, typename... Rest> __device__ __forceinline__ M kvq_mod_of(const M& m, const Rest&...) { return m; }

// the featured kernel arguments of an Fp8Mod (one that is not any(): no window, no cap)
inline KvqMod kvq_mod_args(const Fp8Mod& m, bool causal) {
    KvqMod md;
    md.wl = m.window_left >= 0 ? (int)std::min<int64_t>(m.window_left, kWinNone) : kWinNone;
    md.wr = causal ? 0 : (m.window_right >= 0 ? (int)std::min<int64_t>(m.window_right, kWinNone) : kWinNone);
    md.cap_k = m.softcap > 0.0 ? (float)(2.0 / m.softcap) : 0.f;
    md.cap2 = m.softcap > 0.0 ? (float)(m.softcap * 1.4426950408889634) : 0.f;
    return md;
}

// ---- the MXFP4 cache kernels' parameter blocks (fa_fp4_decode.hip, fa_fp4_prefill.hip) and what fills them from
// the launch arguments: one definition each, whatever the head dim of the kernel that takes it
struct Fp4KvParams {
    const uint8_t *q, *kc, *ksc, *vc, *vsc;
    uint16_t* o;
    float *lse, *po, *plse;               // po / plse: the partials of S > 1 ((b, h_q, token)-major rows, then split)
    const float *qds, *kds, *vds;         // (B, H_kv) descales at their batch strides; null: 1
    long long qds_bs, kds_bs, vds_bs;
    const int *seqlens, *table, *bidx;    // untrusted device memory, or null
    long long tbl_rs;
    int nblk, ps, bcache;
    long long q_bs, kc_bs, ks_bs, vc_bs, vs_bs;   // batch (or page) strides in bytes
    int q_ts, kc_ts, ks_ts, vc_ts, vs_ts;         // token strides in bytes
    int hq, hkv, G, nq, cap, rows, causal;
    float c_log2;                         // float(softmax_scale) * log2(e)
};

// d: the head dim, which sizes the partials of S > 1
inline Fp4KvParams fp4_kv_params(const Fp4KvArgs& a, int d) {
    Fp4KvParams p;
    p.q = (const uint8_t*)a.q; p.kc = (const uint8_t*)a.c.k_cache; p.ksc = (const uint8_t*)a.c.k_scale;
    p.vc = (const uint8_t*)a.c.v_cache; p.vsc = (const uint8_t*)a.c.v_scale;
    p.o = (uint16_t*)a.o; p.lse = a.lse;
    p.qds = a.q_descale; p.kds = a.k_descale; p.vds = a.v_descale;
    p.qds_bs = a.qds_bs; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.seqlens = a.c.cache_seqlens; p.table = a.c.block_table; p.bidx = a.c.cache_batch_idx;
    p.tbl_rs = a.c.table_row_stride; p.nblk = (int)a.c.num_blocks; p.ps = (int)a.c.page_size; p.bcache = (int)a.c.cache_batch;
    p.q_bs = a.q_bs; p.kc_bs = a.c.kc_bs; p.ks_bs = a.c.ks_bs; p.vc_bs = a.c.vc_bs; p.vs_bs = a.c.vs_bs;
    p.q_ts = (int)a.q_ts; p.kc_ts = (int)a.c.kc_ts; p.ks_ts = (int)a.c.ks_ts; p.vc_ts = (int)a.c.vc_ts; p.vs_ts = (int)a.c.vs_ts;
    p.hq = (int)a.heads_q; p.hkv = (int)a.c.heads_kv; p.G = (int)(a.heads_q / a.c.heads_kv);
    p.nq = (int)a.seqlen_q; p.cap = (int)a.c.cache_len; p.rows = p.G * p.nq; p.causal = a.causal != 0;
    p.c_log2 = a.scale * 1.4426950408889634f;
    const int S = (int)a.num_splits;
    // workspace (S > 1): the O partials, then the lse partials, each rounded up to 256 bytes (kv_workspace_bytes)
    const size_t q_rows = (size_t)a.batch * a.heads_q * a.seqlen_q;
    p.po = (float*)a.workspace;
    p.plse = S > 1 ? (float*)((char*)a.workspace + ((q_rows * S * (size_t)d * 4 + 255) & ~(size_t)255)) : nullptr;
    return p;
}

struct Fp4AppendParams {
    const uint8_t *kn, *vn;
    uint8_t *kc, *ksc, *vc, *vsc;
    const float *kds, *vds;
    long long kds_bs, vds_bs;
    const int *seqlens, *table, *bidx;
    long long tbl_rs;
    int nblk, ps, bcache, cap, nnew, hkv;
    long long kn_bs, kn_ts, vn_bs, vn_ts;         // strides in bytes
    long long kc_bs, ks_bs, vc_bs, vs_bs;
    int kc_ts, ks_ts, vc_ts, vs_ts;
};

// the smallest integer e with 6 * 2^e >= amax, in [-64, 64]; 0 for amax = 0.  amax = m 2^x with m in [1, 2): 6 * 2^e = 1.5 *
// 2^(e + 2), so e = x - 2 for m <= 1.5 and x - 1 above.
__device__ __forceinline__ int fp4_block_exponent(float amax) {
    if (amax == 0.f) return 0;
    const uint32_t bits = __float_as_uint(amax);
    const int e = (int)((bits >> 23) & 0xffu) - 129 + ((bits & 0x7fffffu) > 0x400000u ? 1 : 0);
    return min(max(e, -64), 64);
}

// y to its e2m1 code: magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6 are codes 0 .. 7; nearest, a tie to the even code, past 6: 6
__device__ __forceinline__ uint32_t fp4_code(float y) {
    const float a = fabsf(y);
    const uint32_t mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return mag | (y < 0.f ? 8u : 0u);
}

inline Fp4AppendParams fp4_append_params(const Fp4AppendArgs& a) {
    Fp4AppendParams p;
    p.kn = (const uint8_t*)a.k_new; p.vn = (const uint8_t*)a.v_new;
    p.kc = (uint8_t*)a.c.k_cache; p.ksc = (uint8_t*)a.c.k_scale; p.vc = (uint8_t*)a.c.v_cache; p.vsc = (uint8_t*)a.c.v_scale;
    p.kds = a.k_descale; p.vds = a.v_descale; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.seqlens = a.c.cache_seqlens; p.table = a.c.block_table; p.bidx = a.c.cache_batch_idx;
    p.tbl_rs = a.c.table_row_stride; p.nblk = (int)a.c.num_blocks; p.ps = (int)a.c.page_size; p.bcache = (int)a.c.cache_batch;
    p.cap = (int)a.c.cache_len; p.nnew = (int)a.seqlen_new; p.hkv = (int)a.c.heads_kv;
    p.kn_bs = a.kn_bs; p.kn_ts = a.kn_ts; p.vn_bs = a.vn_bs; p.vn_ts = a.vn_ts;
    p.kc_bs = a.c.kc_bs; p.ks_bs = a.c.ks_bs; p.vc_bs = a.c.vc_bs; p.vs_bs = a.c.vs_bs;
    p.kc_ts = (int)a.c.kc_ts; p.ks_ts = (int)a.c.ks_ts; p.vc_ts = (int)a.c.vc_ts; p.vs_ts = (int)a.c.vs_ts;
    return p;
}

struct Fp4PrefillParams {
    const uint8_t *q, *kc, *ksc, *vc, *vsc;
    uint16_t* o;
    float* lse;
    const float *qds, *kds, *vds;         // (B, H_kv) descales at their batch strides; null: 1
    long long qds_bs, kds_bs, vds_bs;
    const int *cu_q, *cu_k, *table;       // untrusted device memory
    long long tbl_rs;
    int nblk, ps, cap;
    long long q_ts, kc_bs, ks_bs, vc_bs, vs_bs;   // q's token stride and the page strides in bytes
    int kc_ts, ks_ts, vc_ts, vs_ts;               // token strides in bytes
    int hq, G, total_q, max_q, causal;
    float c_log2;                         // float(softmax_scale) * log2(e)
};

inline Fp4PrefillParams fp4_prefill_params(const Fp4VarlenArgs& a) {
    Fp4PrefillParams p;
    p.q = (const uint8_t*)a.q; p.kc = (const uint8_t*)a.c.k_cache; p.ksc = (const uint8_t*)a.c.k_scale;
    p.vc = (const uint8_t*)a.c.v_cache; p.vsc = (const uint8_t*)a.c.v_scale;
    p.o = (uint16_t*)a.o; p.lse = a.lse;
    p.qds = a.q_descale; p.kds = a.k_descale; p.vds = a.v_descale;
    p.qds_bs = a.qds_bs; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k; p.table = a.c.block_table;
    p.tbl_rs = a.c.table_row_stride; p.nblk = (int)a.c.num_blocks; p.ps = (int)a.c.page_size; p.cap = (int)a.c.cache_len;
    p.q_ts = a.q_ts; p.kc_bs = a.c.kc_bs; p.ks_bs = a.c.ks_bs; p.vc_bs = a.c.vc_bs; p.vs_bs = a.c.vs_bs;
    p.kc_ts = (int)a.c.kc_ts; p.ks_ts = (int)a.c.ks_ts; p.vc_ts = (int)a.c.vc_ts; p.vs_ts = (int)a.c.vs_ts;
    p.hq = (int)a.heads_q; p.G = (int)(a.heads_q / a.c.heads_kv);
    p.total_q = (int)a.total_q; p.max_q = (int)a.max_seqlen_q; p.causal = a.causal != 0;
    p.c_log2 = a.scale * 1.4426950408889634f;
    return p;
}

// the launch ladder: f(tag, paged) with o's dtype as bf16_tag{} / f16_tag{} and paged as std::true_type{} / std::false_type{}
template <typename F> inline void kvq_dispatch(int dtype, bool paged, F&& f) {
    if (dtype == 2) {
        if (paged) f(bf16_tag{}, std::true_type{});
        else f(bf16_tag{}, std::false_type{});
    } else {
        if (paged) f(f16_tag{}, std::true_type{});
        else f(f16_tag{}, std::false_type{});
    }
}

}  // namespace

}  // namespace fa
