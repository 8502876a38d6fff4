// The fp8 decode step for gfx950 (fa_fp8_kvcache_step; include/fa_mi355x.h): what a serving loop does to an
// e4m3 KV cache between two tokens, in front of fp8 KV-cache decoding (fa_fp8_decode.hip), as one memory-bound launch.
//
//   fp8kv_step_prep_kernel<Tag, FEAT>   grid (K/V blocks + q blocks, batch element), 256 threads, a 16-byte chunk a thread and turn:
//     blocks [0, kv_blocks)   the K/V scatter.  Token n of sequence b goes to position L_b + n, L_b = clamp(cache_seqlens[b], 0,
//                             capacity - N_new), of cache row (bidx ? bidx[b] : b), or through the table to
//                             pool[table[b, pos / ps], pos % ps]; a row or page outside the cache / pool drops the token.  16-bit
//                             mode: a chunk is 8 head dims, K rotated on the way with kStepRot (a non-interleaved pair reads its
//                             partner chunk), both quantised with 1 / descale[b, hk], one 8-byte store each.  kStepE4: a chunk is
//                             16 bytes of codes, copied.
//     blocks [kv_blocks, ..)  the q pass (16-bit mode only).  Token i of head h, rotated at L_b + i (qseq) or L_b, rounded once to
//                             its dtype, quantised with 1 / q_descale[b, h / G], one 8-byte store a chunk into the q8 buffer at
//                             that buffer's own strides.
//     block 0, thread 0       len_eff[b] = L_b + N_new.
//   The rotation, the rounding and the quantisation are kv_append_kernel's device functions (fa_decode_kernels.h:
//   kv_rotate_chunk, kv_q8_quant), so the cache bytes are the ones fa_ex_forward_kvcache_fp8's append stores.
//   fp8kv_step_prep_varlen_kernel<Tag, FEAT, D>   the same work for packed tokens (cu_seqlens_q, cu_seqlens_k_new) and for the head dims
//     64 / 128 / 256 (fa_fp8_kvcache_step_varlen), followed by launch_fp8_kvcache_varlen: see the kernel.
// Then launch_fp8_kvcache_mod, unchanged, with q = the q8 buffer and cache_seqlens = len_eff: its clamp to [0, capacity] is the
// identity on len_eff, and a cache_batch_idx outside the cache is an empty sequence there as it is a dropped append here.
//
// What is untrusted: cache_seqlens, block_table and cache_batch_idx, read on the device only and clamped as above.  After the
// clamp pos = L_b + n < capacity, so a table column is below capacity / ps <= the row stride and a contiguous position inside
// the row; the rotary rows L_b + n and L_b + i lie below capacity + max(0, Nq - N_new) <= seqlen_ro, which the C layer requires.
// Addressing: 64-bit batch, row and page offsets, 32-bit offsets inside one batch element or page (the C layer's span limits).
#include <algorithm>

#include "fa_decode_kernels.h"

namespace fa {

namespace {

constexpr int kStepRot = 1, kStepE4 = 2;   // rotary tables given (16-bit mode); e4m3 q, k_new, v_new

struct Fp8StepParams {
    const uint8_t *q, *kn, *vn;           // the caller's q and new tokens, strides in bytes
    uint8_t *kc, *vc, *q8;                // the e4m3 caches and the q8 buffer
    int* len_eff;
    const float *qds, *kds, *vds;         // (B, H_kv) descales at their batch strides; null: 1
    long long qds_bs, kds_bs, vds_bs;
    const int *seqlens, *table, *bidx;    // untrusted device memory; table and bidx may be null
    long long tbl_rs;
    int nblk, ps, bcache;
    long long q_bs, kn_bs, vn_bs, kc_bs, vc_bs, q8_bs;   // batch (or page) strides in bytes
    int q_ts, kn_ts, vn_ts, kc_ts, vc_ts, q8_ts;         // token strides in bytes
    int hq, hkv, G, nq, nnew, cap;
    int kv_blocks, q_blocks;              // the two sections of blockIdx.x
    KvRot ro;                             // kStepRot
};

template <typename Tag, int FEAT>
__global__ __launch_bounds__(256) void fp8kv_step_prep_kernel(const Fp8StepParams p) {
    constexpr bool ROT = (FEAT & kStepRot) != 0, E4 = (FEAT & kStepE4) != 0;
    constexpr int CPR = E4 ? 8 : 16;      // 16-byte chunks of the source per head row
    constexpr int HB = E4 ? 128 : 256;    // bytes of a head row of the source
    const int b = blockIdx.y;
    const int L = min(max(p.seqlens[b], 0), p.cap - p.nnew);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.len_eff[b] = L + p.nnew;
    if ((int)blockIdx.x < p.kv_blocks) {
        long long row = b;
        if (p.bidx) {
            const int ix = p.bidx[b];
            if ((unsigned)ix >= (unsigned)p.bcache) return;
            row = ix;
        }
        const uint8_t* kn = p.kn + b * p.kn_bs;
        const uint8_t* vn = p.vn + b * p.vn_bs;
        const long long per_b = (long long)p.nnew * p.hkv * CPR;
        for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < per_b; t += (long long)p.kv_blocks * blockDim.x) {
            const int c = (int)(t % CPR);
            const long long r = t / CPR;
            const int h = (int)(r % p.hkv), n = (int)(r / p.hkv);
            int pos = L + n;
            long long unit = row;
            if (p.table) {
                const int j = pos / p.ps;
                const int pg = p.table[b * p.tbl_rs + j];
                if ((unsigned)pg >= (unsigned)p.nblk) continue;
                pos -= j * p.ps;
                unit = pg;
            }
            const uint8_t* krow = kn + (size_t)n * p.kn_ts + (size_t)h * HB;
            u32x4 kx = *reinterpret_cast<const u32x4*>(krow + 16 * c);
            const u32x4 vx = *reinterpret_cast<const u32x4*>(vn + (size_t)n * p.vn_ts + (size_t)h * HB + 16 * c);
            uint8_t* kdst = p.kc + unit * p.kc_bs + (size_t)pos * p.kc_ts + (size_t)h * 128;
            uint8_t* vdst = p.vc + unit * p.vc_bs + (size_t)pos * p.vc_ts + (size_t)h * 128;
            if constexpr (E4) {
                *reinterpret_cast<u32x4*>(kdst + 16 * c) = kx;
                *reinterpret_cast<u32x4*>(vdst + 16 * c) = vx;
            } else {
                if constexpr (ROT) {
                    if (8 * c < p.ro.rdim) {
                        u32x4 par = kx;
                        if (!p.ro.inter) par = *reinterpret_cast<const u32x4*>(krow + 2 * kv_rot_partner(p.ro, 8 * c));
                        kx = kv_rotate_chunk<Tag>(p.ro, L + n, 8 * c, kx, par);
                    }
                }
                const float kinv = 1.0f / (p.kds ? p.kds[b * p.kds_bs + h] : 1.0f);
                const float vinv = 1.0f / (p.vds ? p.vds[b * p.vds_bs + h] : 1.0f);
                *reinterpret_cast<u32x2*>(kdst + 8 * c) = kv_q8_quant<Tag>(kx, kinv);
                *reinterpret_cast<u32x2*>(vdst + 8 * c) = kv_q8_quant<Tag>(vx, vinv);
            }
        }
    } else if constexpr (!E4) {
        const uint8_t* q = p.q + b * p.q_bs;
        uint8_t* q8 = p.q8 + b * p.q8_bs;
        const int xb = (int)blockIdx.x - p.kv_blocks;
        const long long per_b = (long long)p.nq * p.hq * CPR;
        for (long long t = (long long)xb * blockDim.x + threadIdx.x; t < per_b; t += (long long)p.q_blocks * blockDim.x) {
            const int c = (int)(t % CPR);
            const long long r = t / CPR;
            const int h = (int)(r % p.hq), i = (int)(r / p.hq);
            const uint8_t* qrow = q + (size_t)i * p.q_ts + (size_t)h * HB;
            u32x4 qx = *reinterpret_cast<const u32x4*>(qrow + 16 * c);
            if constexpr (ROT) {
                if (8 * c < p.ro.rdim) {
                    u32x4 par = qx;
                    if (!p.ro.inter) par = *reinterpret_cast<const u32x4*>(qrow + 2 * kv_rot_partner(p.ro, 8 * c));
                    qx = kv_rotate_chunk<Tag>(p.ro, L + (p.ro.qseq ? i : 0), 8 * c, qx, par);
                }
            }
            const float qinv = 1.0f / (p.qds ? p.qds[b * p.qds_bs + h / p.G] : 1.0f);
            *reinterpret_cast<u32x2*>(q8 + (size_t)i * p.q8_ts + (size_t)h * 128 + 8 * c) = kv_q8_quant<Tag>(qx, qinv);
        }
    }
}

// fp8kv_step_prep_kernel's sibling for packed tokens and for the head dims 64 / 128 / 256 (fa_fp8_kvcache_step_varlen; DESIGN.md
// section 9zf): every packed call and every call at d != 128 runs it; the padded d = 128 step keeps the kernel above.
// Per sequence, from untrusted device memory: nnew_b and its first source row start_b (kv_cu_range over cu_kn with the capacity as
// bound; cu_kn null: seqlen_new rows of batch element b), nq_b and its first token tok0 (kv_cu_range over cu_q with max_seqlen_q;
// cu_q null: seqlen_q tokens of batch element b), L_b = clamp(cache_seqlens[b], 0, capacity - nnew_b), len_eff[b] = L_b + nnew_b.
// The loop bounds come from these; the grid is sized on the host from the totals.  Chunk geometry by width: a 16-bit head row is
// 2 D bytes in D / 8 chunks, an e4m3 row D bytes in D / 16 chunks, the destination head offset h D.  Source rows are addressed in
// 64 bits.  The rotation, rounding and quantisation are the same device functions, at the same positions (new key n at L_b + n, q
// token i at L_b + i with qseq, else L_b), so the bytes are the padded step's and fa_ex_forward_kvcache_fp8's.
struct Fp8StepVarParams {
    Fp8StepParams s;                      // nq / nnew: the padded extents (used where the offsets are null)
    const int *cu_q, *cu_kn;              // untrusted device offsets (B + 1,), or null
    int total_q, max_q, total_kn;
};

template <typename Tag, int FEAT, int D>
__global__ __launch_bounds__(256) void fp8kv_step_prep_varlen_kernel(const Fp8StepVarParams v) {
    constexpr bool ROT = (FEAT & kStepRot) != 0, E4 = (FEAT & kStepE4) != 0;
    constexpr int CPR = E4 ? D / 16 : D / 8;   // 16-byte chunks of the source per head row
    constexpr int HB = E4 ? D : 2 * D;         // bytes of a head row of the source
    const Fp8StepParams& p = v.s;
    const int b = blockIdx.y;
    int kst = 0, nnew = p.nnew;
    if (v.cu_kn) nnew = kv_cu_range(v.cu_kn, b, v.total_kn, p.cap, kst);
    const int L = min(max(p.seqlens[b], 0), p.cap - nnew);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.len_eff[b] = L + nnew;
    if ((int)blockIdx.x < p.kv_blocks) {
        long long row = b;
        if (p.bidx) {
            const int ix = p.bidx[b];
            if ((unsigned)ix >= (unsigned)p.bcache) return;
            row = ix;
        }
        const uint8_t* kn = p.kn + (v.cu_kn ? (long long)kst * p.kn_ts : b * p.kn_bs);
        const uint8_t* vn = p.vn + (v.cu_kn ? (long long)kst * p.vn_ts : b * p.vn_bs);
        const long long per_b = (long long)nnew * p.hkv * CPR;
        for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < per_b; t += (long long)p.kv_blocks * blockDim.x) {
            const int c = (int)(t % CPR);
            const long long r = t / CPR;
            const int h = (int)(r % p.hkv), n = (int)(r / p.hkv);
            int pos = L + n;
            long long unit = row;
            if (p.table) {
                const int j = pos / p.ps;
                const int pg = p.table[b * p.tbl_rs + j];
                if ((unsigned)pg >= (unsigned)p.nblk) continue;
                pos -= j * p.ps;
                unit = pg;
            }
            const uint8_t* krow = kn + (size_t)n * p.kn_ts + (size_t)h * HB;
            u32x4 kx = *reinterpret_cast<const u32x4*>(krow + 16 * c);
            const u32x4 vx = *reinterpret_cast<const u32x4*>(vn + (size_t)n * p.vn_ts + (size_t)h * HB + 16 * c);
            uint8_t* kdst = p.kc + unit * p.kc_bs + (size_t)pos * p.kc_ts + (size_t)h * D;
            uint8_t* vdst = p.vc + unit * p.vc_bs + (size_t)pos * p.vc_ts + (size_t)h * D;
            if constexpr (E4) {
                *reinterpret_cast<u32x4*>(kdst + 16 * c) = kx;
                *reinterpret_cast<u32x4*>(vdst + 16 * c) = vx;
            } else {
                if constexpr (ROT) {
                    if (8 * c < p.ro.rdim) {
                        u32x4 par = kx;
                        if (!p.ro.inter) par = *reinterpret_cast<const u32x4*>(krow + 2 * kv_rot_partner(p.ro, 8 * c));
                        kx = kv_rotate_chunk<Tag>(p.ro, L + n, 8 * c, kx, par);
                    }
                }
                const float kinv = 1.0f / (p.kds ? p.kds[b * p.kds_bs + h] : 1.0f);
                const float vinv = 1.0f / (p.vds ? p.vds[b * p.vds_bs + h] : 1.0f);
                *reinterpret_cast<u32x2*>(kdst + 8 * c) = kv_q8_quant<Tag>(kx, kinv);
                *reinterpret_cast<u32x2*>(vdst + 8 * c) = kv_q8_quant<Tag>(vx, vinv);
            }
        }
    } else if constexpr (!E4) {
        int qst = 0, nq = p.nq;
        if (v.cu_q) nq = kv_cu_range(v.cu_q, b, v.total_q, v.max_q, qst);
        const uint8_t* q = p.q + (v.cu_q ? (long long)qst * p.q_ts : b * p.q_bs);
        uint8_t* q8 = p.q8 + (v.cu_q ? (long long)qst * p.q8_ts : b * p.q8_bs);
        const int xb = (int)blockIdx.x - p.kv_blocks;
        const long long per_b = (long long)nq * p.hq * CPR;
        for (long long t = (long long)xb * blockDim.x + threadIdx.x; t < per_b; t += (long long)p.q_blocks * blockDim.x) {
            const int c = (int)(t % CPR);
            const long long r = t / CPR;
            const int h = (int)(r % p.hq), i = (int)(r / p.hq);
            const uint8_t* qrow = q + (size_t)i * p.q_ts + (size_t)h * HB;
            u32x4 qx = *reinterpret_cast<const u32x4*>(qrow + 16 * c);
            if constexpr (ROT) {
                if (8 * c < p.ro.rdim) {
                    u32x4 par = qx;
                    if (!p.ro.inter) par = *reinterpret_cast<const u32x4*>(qrow + 2 * kv_rot_partner(p.ro, 8 * c));
                    qx = kv_rotate_chunk<Tag>(p.ro, L + (p.ro.qseq ? i : 0), 8 * c, qx, par);
                }
            }
            const float qinv = 1.0f / (p.qds ? p.qds[b * p.qds_bs + h / p.G] : 1.0f);
            *reinterpret_cast<u32x2*>(q8 + (size_t)i * p.q8_ts + (size_t)h * D + 8 * c) = kv_q8_quant<Tag>(qx, qinv);
        }
    }
}

constexpr size_t step_align(size_t x) { return (x + 255) & ~(size_t)255; }

template <typename Tag, int FEAT>
void step_prep_varlen_launch(int d, dim3 grid, hipStream_t st, const Fp8StepVarParams& v) {
    if (d == 64) hipLaunchKernelGGL((fp8kv_step_prep_varlen_kernel<Tag, FEAT, 64>), grid, dim3(256), 0, st, v);
    else if (d == 128) hipLaunchKernelGGL((fp8kv_step_prep_varlen_kernel<Tag, FEAT, 128>), grid, dim3(256), 0, st, v);
    else hipLaunchKernelGGL((fp8kv_step_prep_varlen_kernel<Tag, FEAT, 256>), grid, dim3(256), 0, st, v);
}

}  // namespace

size_t fp8kv_step_prep_bytes(int64_t batch, int64_t heads_q, int64_t seqlen_q, bool q8_in_workspace) {
    return step_align((size_t)batch * 4) + (q8_in_workspace ? step_align((size_t)batch * seqlen_q * heads_q * 128) : 0);
}

hipError_t launch_fp8_kvcache_step(const Fp8StepArgs& s, const Fp8Mod& m, hipStream_t st) {
    const Fp8KvArgs& a = s.kv;
    const bool e4 = s.in_dtype == 3, rot = s.rotary_cos != nullptr;
    if (!a.cache_seqlens || !a.workspace || (e4 && (rot || s.q8_out))) return hipErrorInvalidValue;
    char* ws = (char*)a.workspace;
    Fp8StepParams p;
    p.q = (const uint8_t*)a.q; p.kn = (const uint8_t*)s.k_new; p.vn = (const uint8_t*)s.v_new;
    p.kc = (uint8_t*)const_cast<void*>(a.k_cache); p.vc = (uint8_t*)const_cast<void*>(a.v_cache);
    p.len_eff = (int*)ws;
    ws += step_align((size_t)a.batch * 4);
    Fp8KvArgs att = a;
    if (e4) {                  // q is used in place
        p.q8 = nullptr; p.q8_bs = 0; p.q8_ts = 0;
    } else if (s.q8_out) {
        p.q8 = (uint8_t*)s.q8_out; p.q8_bs = s.q8_bs; p.q8_ts = (int)s.q8_ts;
    } else {
        p.q8 = (uint8_t*)ws; p.q8_ts = (int)(a.heads_q * 128); p.q8_bs = a.seqlen_q * a.heads_q * 128;
        ws += step_align((size_t)a.batch * a.seqlen_q * a.heads_q * 128);
    }
    if (!e4) { att.q = p.q8; att.q_bs = p.q8_bs; att.q_ts = p.q8_ts; }
    att.cache_seqlens = p.len_eff;
    att.workspace = ws;
    p.qds = a.q_descale; p.kds = a.k_descale; p.vds = a.v_descale;
    p.qds_bs = a.qds_bs; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.seqlens = a.cache_seqlens; p.table = a.block_table; p.bidx = a.cache_batch_idx;
    p.tbl_rs = a.table_row_stride; p.nblk = (int)a.num_blocks; p.ps = (int)a.page_size; p.bcache = (int)a.cache_batch;
    p.q_bs = a.q_bs; p.kn_bs = s.kn_bs; p.vn_bs = s.vn_bs; p.kc_bs = a.kc_bs; p.vc_bs = a.vc_bs;
    p.q_ts = (int)a.q_ts; p.kn_ts = (int)s.kn_ts; p.vn_ts = (int)s.vn_ts; p.kc_ts = (int)a.kc_ts; p.vc_ts = (int)a.vc_ts;
    p.hq = (int)a.heads_q; p.hkv = (int)a.heads_kv; p.G = (int)(a.heads_q / a.heads_kv);
    p.nq = (int)a.seqlen_q; p.nnew = (int)s.seqlen_new; p.cap = (int)a.cache_len;
    p.ro.cos = (const uint16_t*)s.rotary_cos; p.ro.sin = (const uint16_t*)s.rotary_sin;
    p.ro.cos_rs = s.rotary_cos_rs; p.ro.sin_rs = s.rotary_sin_rs;
    p.ro.rdim = (int)s.rotary_dim; p.ro.inter = s.rotary_interleaved; p.ro.qseq = s.rotary_q_per_token;
    // a 16-byte chunk a thread: at most 1024 blocks a section, the threads stride over what is left
    const long long kv_chunks = (long long)s.seqlen_new * a.heads_kv * (e4 ? 8 : 16), q_chunks = e4 ? 0 : (long long)a.seqlen_q * a.heads_q * 16;
    p.kv_blocks = (int)std::min<long long>((kv_chunks + 255) / 256, 1024);
    p.q_blocks = (int)std::min<long long>((q_chunks + 255) / 256, 1024);
    const dim3 grid((unsigned)(p.kv_blocks + p.q_blocks), (unsigned)a.batch);
    {
        route_hit(ROUTE_FP8KV_STEP_PREP);
        ProfScope ps(K_FP8KV_STEP_PREP, st);
        if (e4) hipLaunchKernelGGL((fp8kv_step_prep_kernel<bf16_tag, kStepE4>), grid, dim3(256), 0, st, p);   // bytes only: one kernel
        else if (s.in_dtype == 2) {
            if (rot) hipLaunchKernelGGL((fp8kv_step_prep_kernel<bf16_tag, kStepRot>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((fp8kv_step_prep_kernel<bf16_tag, 0>), grid, dim3(256), 0, st, p);
        } else {
            if (rot) hipLaunchKernelGGL((fp8kv_step_prep_kernel<f16_tag, kStepRot>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((fp8kv_step_prep_kernel<f16_tag, 0>), grid, dim3(256), 0, st, p);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_fp8_kvcache_mod(att, m, st);
}

size_t fp8kv_step_prep_bytes_varlen(int64_t batch, int64_t q_tokens, int64_t heads_q, int64_t d, bool q8_in_workspace) {
    return step_align((size_t)batch * 4) + (q8_in_workspace ? step_align((size_t)q_tokens * heads_q * d) : 0);
}

hipError_t launch_fp8_kvcache_step_varlen(const Fp8StepArgs& s, const Fp8Mod& m, hipStream_t st) {
    const Fp8KvArgs& a = s.kv;
    const bool packed = a.cu_seqlens_q != nullptr;
    if (!packed && !s.cu_seqlens_k_new && a.d == 128) return launch_fp8_kvcache_step(s, m, st);   // the padded step, launch for launch
    const bool e4 = s.in_dtype == 3, rot = s.rotary_cos != nullptr;
    if (!a.cache_seqlens || !a.workspace || (e4 && (rot || s.q8_out)) || (s.cu_seqlens_k_new && !packed)) return hipErrorInvalidValue;
    const int64_t d = a.d;
    const int64_t q_tokens = packed ? a.total_q : a.batch * a.seqlen_q;
    char* ws = (char*)a.workspace;
    Fp8StepVarParams v;
    Fp8StepParams& p = v.s;
    p.q = (const uint8_t*)a.q; p.kn = (const uint8_t*)s.k_new; p.vn = (const uint8_t*)s.v_new;
    p.kc = (uint8_t*)const_cast<void*>(a.k_cache); p.vc = (uint8_t*)const_cast<void*>(a.v_cache);
    p.len_eff = (int*)ws;
    ws += step_align((size_t)a.batch * 4);
    Fp8KvArgs att = a;
    if (e4) {                  // q is used in place
        p.q8 = nullptr; p.q8_bs = 0; p.q8_ts = 0;
    } else if (s.q8_out) {
        p.q8 = (uint8_t*)s.q8_out; p.q8_bs = packed ? 0 : s.q8_bs; p.q8_ts = (int)s.q8_ts;
    } else {
        p.q8 = (uint8_t*)ws; p.q8_ts = (int)(a.heads_q * d); p.q8_bs = packed ? 0 : a.seqlen_q * a.heads_q * d;
        ws += step_align((size_t)q_tokens * a.heads_q * d);
    }
    if (!e4) { att.q = p.q8; att.q_bs = p.q8_bs; att.q_ts = p.q8_ts; }
    att.cache_seqlens = p.len_eff;
    att.workspace = ws;
    p.qds = a.q_descale; p.kds = a.k_descale; p.vds = a.v_descale;
    p.qds_bs = a.qds_bs; p.kds_bs = a.kds_bs; p.vds_bs = a.vds_bs;
    p.seqlens = a.cache_seqlens; p.table = a.block_table; p.bidx = a.cache_batch_idx;
    p.tbl_rs = a.table_row_stride; p.nblk = (int)a.num_blocks; p.ps = (int)a.page_size; p.bcache = (int)a.cache_batch;
    p.q_bs = packed ? 0 : a.q_bs; p.kn_bs = s.kn_bs; p.vn_bs = s.vn_bs; p.kc_bs = a.kc_bs; p.vc_bs = a.vc_bs;
    p.q_ts = (int)a.q_ts; p.kn_ts = (int)s.kn_ts; p.vn_ts = (int)s.vn_ts; p.kc_ts = (int)a.kc_ts; p.vc_ts = (int)a.vc_ts;
    p.hq = (int)a.heads_q; p.hkv = (int)a.heads_kv; p.G = (int)(a.heads_q / a.heads_kv);
    p.nq = packed ? 0 : (int)a.seqlen_q; p.nnew = s.cu_seqlens_k_new ? 0 : (int)s.seqlen_new; p.cap = (int)a.cache_len;
    p.ro.cos = (const uint16_t*)s.rotary_cos; p.ro.sin = (const uint16_t*)s.rotary_sin;
    p.ro.cos_rs = s.rotary_cos_rs; p.ro.sin_rs = s.rotary_sin_rs;
    p.ro.rdim = (int)s.rotary_dim; p.ro.inter = s.rotary_interleaved; p.ro.qseq = s.rotary_q_per_token;
    v.cu_q = a.cu_seqlens_q; v.cu_kn = s.cu_seqlens_k_new;
    v.total_q = (int)a.total_q; v.max_q = (int)a.max_seqlen_q; v.total_kn = (int)s.total_k_new;
    // a 16-byte chunk a thread: at most 1024 blocks a section (one sequence has at most total_k_new new keys and max_seqlen_q
    // query tokens; the kernel's loop bounds come from the device), the threads stride over what is left.  At least one block
    // writes len_eff.
    const long long cpr = e4 ? d / 16 : d / 8;
    const long long kv_chunks = (s.cu_seqlens_k_new ? s.total_k_new : s.seqlen_new) * a.heads_kv * cpr;
    const long long q_chunks = e4 ? 0 : (packed ? a.max_seqlen_q : a.seqlen_q) * a.heads_q * cpr;
    p.kv_blocks = (int)std::max<long long>(1, std::min<long long>((kv_chunks + 255) / 256, 1024));
    p.q_blocks = (int)std::min<long long>((q_chunks + 255) / 256, 1024);
    const dim3 grid((unsigned)(p.kv_blocks + p.q_blocks), (unsigned)a.batch);
    {
        route_hit(ROUTE_FP8KV_STEP_PREP_VARLEN);
        ProfScope ps(K_FP8KV_STEP_PREP_VARLEN, st);
        if (e4) step_prep_varlen_launch<bf16_tag, kStepE4>((int)d, grid, st, v);   // bytes only: one kernel a width
        else if (s.in_dtype == 2) {
            if (rot) step_prep_varlen_launch<bf16_tag, kStepRot>((int)d, grid, st, v);
            else step_prep_varlen_launch<bf16_tag, 0>((int)d, grid, st, v);
        } else {
            if (rot) step_prep_varlen_launch<f16_tag, kStepRot>((int)d, grid, st, v);
            else step_prep_varlen_launch<f16_tag, 0>((int)d, grid, st, v);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_fp8_kvcache_varlen(att, m, st);   // (padded at 64 / 256: launch_fp8_kvcache_hdim; without a query token: nothing)
}

}  // namespace fa
