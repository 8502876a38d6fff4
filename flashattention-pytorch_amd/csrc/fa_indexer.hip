// DeepSeek-V3.2's lightning indexer for gfx950: the step that makes the token lists sparse MLA attends over
// (include/fa_mi355x.h: fa_indexer_pack, fa_indexer_logits, fa_indexer_topk).  For query token t and cached
// token s
//     I[t, s] = sum_h  w[t, h] * relu(q_I[t, h] . k_I[s])
// over H_I = 32 | 64 index heads, 128 wide, q_I and k_I in e4m3, and per token the topk largest I[t, .] among the tokens t sees.
//
// The index-key cache is a paged pool of 132-byte tokens [128 e4m3 | 1 float32 scale], slot s of page p at pool + p * page_sb +
// s * tok_sb bytes (tok_sb >= 132, a multiple of 16: 144 dense).  Lengths and table are untrusted, under the rules of fa_mla.hip.
//
// Three kernels:
//   idx_pack_kernel     16 lanes a new token (8 bf16 each): mla_f8_pack_kernel's quantiser (fa_mla.hip) on one 128-wide tile.  The
//                       rule is written out again here rather than shared: that kernel's instructions stay what they were.
//   idx_logits_kernel   <H, CAUSAL>: a workgroup of 4 waves owns 256 consecutive keys of one sequence and walks up to 64 query tokens.
//                       Each wave keeps its 64 keys (two 32-key blocks) in registers for the whole walk, as the SECOND operand of
//                       v_mfma_scale_f32_32x32x64_f8f6f4 (unit scales): the key is on the lane.  The FIRST operand is 32 heads of one
//                       token's q from LDS (TileSwz<64> image, staged four tokens at a time together with their weights), read once
//                       for both key blocks.  So a lane holds, per key block, the products of ITS key with 16 heads
//                       (register i: head 32 hb + (i & 3) + 8 (i >> 2) + 4 (lane >> 5)), and the head sum is in-lane.
//   idx_topk_kernel     one workgroup a row: an 8-bit radix select (4 histogram passes, integer LDS atomics) for the threshold
//                       key, then an ordered compaction in position order.
//
// The logits' arithmetic, in the order tests/indexer_ref.py (baseline) transcribes it -- weights may be negative, the head sum
// cancels, and nothing here may be reordered without that module following:
//   [L1] p[h] = q[h] . k8: two 64-term instructions over the 128 bytes, bytes 0 .. 63 first, fp32 accumulator from 0;
//   [L2] r[h] = max(p[h], 0);
//   [L3] per lane half c = lane >> 5: s_c = 0, then s_c = fma(w[h], r[h], s_c) over its heads in the order
//        hb = 0 .. H/32 - 1, i = 0 .. 15, h = 32 hb + (i & 3) + 8 (i >> 2) + 4 c;
//   [L4] t = s_0 + s_1 (one fp32 add; commutative, so both halves hold the same bits);
//   [L5] logit = t * k_scale (one fp32 multiply, after the head sum).
#include "fa_common.h"
#include "fa_kernels.h"
#include <algorithm>

namespace fa {
namespace {

constexpr int kIdxD = 128, kIdxScaleAt = 128;   // a token: 128 codes, then its scale
typedef float idx_f32x4 __attribute__((ext_vector_type(4)));

// ---- the append ---------------------------------------------------------------------------------------------------------------
struct IdxPackParams {
    const uint16_t* k;
    unsigned char* pool;
    const int *seqlens, *table;
    long long k_bs, k_ts, page_sb, tok_sb, tbl_rs, tokens;
    int nnew, nblk, ps, mb, pow2;
};

__global__ __launch_bounds__(256) void idx_pack_kernel(IdxPackParams a) {
    const int sub = threadIdx.x & 15;
    const long long t = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (t >= a.tokens) return;   // (uniform over the token's 16 lanes, as everything up to the loads: the shuffles stay inside them)
    const long long b = t / a.nnew;
    const int i = (int)(t - b * a.nnew);
    const int len = a.seqlens[b];
    const long long pos = (long long)len + i;
    if (len < 0 || pos >= (long long)a.mb * a.ps) return;
    const int j = (int)(pos / a.ps), slot = (int)(pos - (long long)j * a.ps);
    const int pg = a.table[b * a.tbl_rs + j];
    if ((unsigned)pg >= (unsigned)a.nblk) return;
    unsigned char* dst = a.pool + pg * a.page_sb + slot * a.tok_sb;

    const u32x4 x = *reinterpret_cast<const u32x4*>(a.k + b * a.k_bs + i * a.k_ts + 8 * sub);
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
    if (a.pow2) {   // the next power of two, in the bit pattern (exact for every normal scale below 2^127)
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
    *reinterpret_cast<u32x2*>(dst + 8 * sub) = q8;
    if (sub == 0) *reinterpret_cast<float*>(dst + kIdxScaleAt) = scale;
}

// ---- the logits ---------------------------------------------------------------------------------------------------------------
constexpr int kIdxKeys = 256;    // keys a workgroup
constexpr int kIdxTokens = 64;   // query tokens a workgroup walks
constexpr int kIdxStage = 4;     // tokens staged in LDS at a time

struct IdxLogitsParams {
    const uint8_t *q, *pool;
    const float* w;
    const int *seqlens, *table;
    float* out;
    long long q_bs, q_ts, q_hs, w_bs, w_ts, page_sb, tbl_rs, out_bs, out_rs;
    int tok_sb, nq, nblk, ps, cap, width;   // cap: min(max_blocks * page, width)
};

template <int H, bool CAUSAL>
__global__ __launch_bounds__(256) void idx_logits_kernel(const IdxLogitsParams p) {
    constexpr int HB = H / 32, QTOK = H * kIdxD;           // head blocks; bytes of one token's q image
    __shared__ __attribute__((aligned(16))) char qs[kIdxStage * QTOK];
    __shared__ __attribute__((aligned(16))) float ws[kIdxStage * H];
    typedef int i32x8_t __attribute__((ext_vector_type(8)));

    const int b = blockIdx.z, k0 = blockIdx.x * kIdxKeys, i0 = blockIdx.y * kIdxTokens;
    const int len = min(max(p.seqlens[b], 0), p.cap);
    if (k0 >= len) return;                                 // (workgroup-uniform, as every return and loop bound below)
    const int i1 = min(p.nq, i0 + kIdxTokens);
    const int shift = len - p.nq;                          // token i sees key j <= i + shift
    int ifirst = i0;
    if (CAUSAL) {
        if (k0 > i1 - 1 + shift) return;                   // no token of the workgroup sees a key of the tile: not loaded
        ifirst = max(i0, k0 - shift);                      // the tokens before it see none of it
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;

    // the wave's 64 keys: key block kb, key kw + 32 kb + r; chunk c of a lane is bytes 32 c + 16 h .. of its key (the second
    // operand's half of every 32 bytes), an invisible key or one on a page outside the pool a zero row with scale 0
    const int kw = k0 + 64 * wv;
    u32x4 kf[2][4];
    float ksc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int j = kw + 32 * kb + r;
        const unsigned char* src = nullptr;
        if (j < len) {                                     // (so no table entry past ceil(len / page) is read)
            const int blk = j / p.ps;
            const int pg = p.table[b * p.tbl_rs + blk];
            if ((unsigned)pg < (unsigned)p.nblk) src = p.pool + pg * p.page_sb + (long long)(j - blk * p.ps) * p.tok_sb;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            kf[kb][c] = src ? *reinterpret_cast<const u32x4*>(src + 32 * c + 16 * h) : u32x4{0u, 0u, 0u, 0u};
        ksc[kb] = src ? *reinterpret_cast<const float*>(src + kIdxScaleAt) : 0.f;
    }
    const int jout = kw + lane;                            // the key whose logit the lane stores: block h, key r
    float* orow = p.out + b * p.out_bs + jout;
    const uint8_t* qb_ = p.q + b * p.q_bs;
    const float* wb_ = p.w + b * p.w_bs;

    for (int g0 = ifirst; g0 < i1; g0 += kIdxStage) {
        const int cnt = min(kIdxStage, i1 - g0);
        __syncthreads();                                   // the previous group's reads are done
        for (int c = tid; c < cnt * H * 8; c += 256) {     // q: 16-byte chunks, 8 a head
            const int tk = c / (H * 8), rem = c - tk * (H * 8), hd = rem >> 3, ch = rem & 7;
            *reinterpret_cast<u32x4*>(qs + tk * QTOK + TileSwz<64>::off(hd, ch)) =
                *reinterpret_cast<const u32x4*>(qb_ + (g0 + tk) * p.q_ts + hd * p.q_hs + 16 * ch);
        }
        for (int c = tid; c < cnt * H; c += 256) {
            const int tk = c / H;
            ws[c] = wb_[(g0 + tk) * p.w_ts + (c - tk * H)];
        }
        __syncthreads();
        for (int tk = 0; tk < cnt; ++tk) {
            const int i = g0 + tk, bound = CAUSAL ? min(i + shift, len - 1) : len - 1;   // the last key token i sees
            if (bound < kw) continue;                      // (wave-uniform: no barrier below)
            const char* qt = qs + tk * QTOK;
            float s[2] = {0.f, 0.f};
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                f32x16 acc[2];
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[kb][e] = 0.f;
#pragma unroll
                for (int M = 0; M < 2; ++M) {              // [L1]
                    const u32x4 a0 = *reinterpret_cast<const u32x4*>(qt + TileSwz<64>::off(32 * hb + r, 4 * M + h));
                    const u32x4 a1 = *reinterpret_cast<const u32x4*>(qt + TileSwz<64>::off(32 * hb + r, 4 * M + 2 + h));
                    const i32x8_t qa = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) {
                        const u32x4 b0 = kf[kb][2 * M], b1 = kf[kb][2 * M + 1];
                        const i32x8_t kk = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
                        acc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(qa, kk, acc[kb], 0, 0, 0, 127, 0, 127);
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const idx_f32x4 wg = *reinterpret_cast<const idx_f32x4*>(ws + tk * H + 32 * hb + 8 * g + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int kb = 0; kb < 2; ++kb) s[kb] = fmaf(wg[e], fmaxf(acc[kb][4 * g + e], 0.f), s[kb]);   // [L2] [L3]
                }
            }
            const float t0 = s[0] + wave_half_swap(s[0]), t1 = s[1] + wave_half_swap(s[1]);   // [L4]
            const float val = h ? t1 * ksc[1] : t0 * ksc[0];                                   // [L5]
            if (jout <= bound) orow[i * p.out_rs] = val;
        }
    }
}

// ---- the selection ------------------------------------------------------------------------------------------------------------
struct IdxTopkParams {
    const float* logits;
    const int* seqlens;
    int* out;
    long long lg_bs, lg_rs, ix_bs, ix_ts;
    int nq, width, topk, causal;
};

// the order key: a total order on bit patterns, compared as unsigned (-0 < +0, a positive NaN above +inf)
__device__ __forceinline__ unsigned idx_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }

constexpr int kTopkThreads = 1024, kTopkBatch = 8;   // loads a thread keeps in flight

__global__ __launch_bounds__(kTopkThreads) void idx_topk_kernel(const IdxTopkParams p) {
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[2];                     // the chosen digit, and what remains to take at and below it
    __shared__ unsigned wtot[2][kTopkThreads / 64];  // per wave: count(key > T) | count(key == T) << 16, double-buffered
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int len = min(max(p.seqlens[b], 0), p.width);
    const int n = p.causal ? min(max(len - p.nq + i + 1, 0), len) : len;   // the visible keys are 0 .. n - 1
    int* out = p.out + b * p.ix_bs + i * p.ix_ts;
    if (n <= p.topk) {                               // every visible key is selected: the logits are not read
        for (int j = tid; j < p.topk; j += kTopkThreads) out[j] = j < n ? j : -1;
        return;
    }
    const unsigned* row = reinterpret_cast<const unsigned*>(p.logits + b * p.lg_bs + i * p.lg_rs);

    // the threshold key T: the topk-th largest, a digit of 8 bits a pass among the keys that share the digits found so far
    unsigned prefix = 0, mask = 0, remaining = (unsigned)p.topk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int j0 = 0; j0 < n; j0 += kTopkThreads * kTopkBatch) {
            unsigned v[kTopkBatch];
#pragma unroll
            for (int u = 0; u < kTopkBatch; ++u) {
                const int j = j0 + u * kTopkThreads + tid;
                v[u] = j < n ? row[j] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kTopkBatch; ++u) {
                const unsigned key = idx_key(v[u]);
                if (j0 + u * kTopkThreads + tid < n && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (wv == 0) {                               // lane l: digits 4 l .. 4 l + 3; the keys above a digit, by a suffix scan
            unsigned c[4], tot = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { c[e] = hist[4 * lane + e]; tot += c[e]; }
            unsigned x = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned y = __shfl_down(x, o, 64);
                if (lane + o < 64) x += y;
            }
            unsigned above = x - tot;
#pragma unroll
            for (int e = 3; e >= 0; --e) {
                if (above < remaining && above + c[e] >= remaining) { pick[0] = 4 * lane + e; pick[1] = remaining - above; }
                above += c[e];
            }
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        mask |= 255u << shift;
        remaining = pick[1];
    }
    const unsigned T = prefix, need = remaining;      // take every key > T, and the first `need` positions with key == T

    // the compaction, in position order: a selected position's place is the count of selected positions before it
    unsigned gt_base = 0, eq_base = 0;
    int buf = 0;
    for (int j0 = 0; j0 < n; j0 += kTopkThreads * kTopkBatch) {
        unsigned v[kTopkBatch];
#pragma unroll
        for (int u = 0; u < kTopkBatch; ++u) {
            const int j = j0 + u * kTopkThreads + tid;
            v[u] = j < n ? row[j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kTopkBatch; ++u) {
            const int jc = j0 + u * kTopkThreads;    // (uniform)
            if (jc >= n) break;
            const int j = jc + tid;
            const unsigned key = idx_key(v[u]);
            const bool gt = j < n && key > T, eq = j < n && key == T;
            const unsigned long long bg = __ballot(gt), be = __ballot(eq), below = (1ull << lane) - 1ull;
            if (lane == 0) wtot[buf][wv] = (unsigned)__popcll(bg) | ((unsigned)__popcll(be) << 16);
            __syncthreads();
            unsigned before = 0, all = 0;
#pragma unroll
            for (int x = 0; x < kTopkThreads / 64; ++x) {
                const unsigned c = wtot[buf][x];
                all += c;
                before += x < wv ? c : 0u;
            }
            const unsigned gt_before = gt_base + (before & 0xffffu) + (unsigned)__popcll(bg & below);
            const unsigned eq_before = eq_base + (before >> 16) + (unsigned)__popcll(be & below);
            if (gt || (eq && eq_before < need)) {
                const unsigned at = gt_before + min(eq_before, need);
                if (at < (unsigned)p.topk) out[at] = j;
            }
            gt_base += all & 0xffffu;
            eq_base += all >> 16;
            buf ^= 1;   // (the next write of this buffer lies behind the next barrier, which every reader of it has then passed)
        }
    }
}

}  // namespace

hipError_t launch_indexer_pack(const IndexerPackArgs& a, hipStream_t st) {
    IdxPackParams k;
    k.k = (const uint16_t*)a.k_new; k.pool = (unsigned char*)a.pool; k.seqlens = a.cache_seqlens; k.table = a.block_table;
    k.k_bs = a.k_bs; k.k_ts = a.k_ts; k.page_sb = a.page_sb; k.tok_sb = a.tok_sb; k.tbl_rs = a.table_row_stride;
    k.tokens = a.batch * a.seqlen_new;
    k.nnew = (int)a.seqlen_new; k.nblk = (int)a.num_blocks; k.ps = (int)a.page_size; k.mb = (int)a.max_blocks; k.pow2 = a.scale_pow2 ? 1 : 0;
    ProfScope ps(K_IDX_PACK, st);
    hipLaunchKernelGGL(idx_pack_kernel, dim3((unsigned)((k.tokens + 15) / 16)), dim3(256), 0, st, k);
    return hipGetLastError();
}

hipError_t launch_indexer_logits(const IndexerLogitsArgs& a, hipStream_t st) {
    if (a.heads != 32 && a.heads != 64) return hipErrorInvalidValue;   // (the C layer's check)
    IdxLogitsParams k;
    k.q = (const uint8_t*)a.q; k.pool = (const uint8_t*)a.pool; k.w = a.weights; k.seqlens = a.cache_seqlens; k.table = a.block_table;
    k.out = a.logits;
    k.q_bs = a.q_bs; k.q_ts = a.q_ts; k.q_hs = a.q_hs; k.w_bs = a.w_bs; k.w_ts = a.w_ts; k.page_sb = a.page_sb;
    k.tbl_rs = a.table_row_stride; k.out_bs = a.lg_bs; k.out_rs = a.lg_rs;
    k.tok_sb = (int)a.tok_sb; k.nq = (int)a.seqlen_q; k.nblk = (int)a.num_blocks; k.ps = (int)a.page_size;
    k.cap = (int)std::min<int64_t>(a.max_blocks * a.page_size, a.width); k.width = (int)a.width;
    const dim3 grid((unsigned)((k.cap + kIdxKeys - 1) / kIdxKeys), (unsigned)((a.seqlen_q + kIdxTokens - 1) / kIdxTokens), (unsigned)a.batch);
    ProfScope ps(K_IDX_LOGITS, st);
    if (a.heads == 64) {
        if (a.causal) hipLaunchKernelGGL((idx_logits_kernel<64, true>), grid, dim3(256), 0, st, k);
        else hipLaunchKernelGGL((idx_logits_kernel<64, false>), grid, dim3(256), 0, st, k);
    } else {
        if (a.causal) hipLaunchKernelGGL((idx_logits_kernel<32, true>), grid, dim3(256), 0, st, k);
        else hipLaunchKernelGGL((idx_logits_kernel<32, false>), grid, dim3(256), 0, st, k);
    }
    return hipGetLastError();
}

hipError_t launch_indexer_topk(const IndexerTopkArgs& a, hipStream_t st) {
    IdxTopkParams k;
    k.logits = a.logits; k.seqlens = a.cache_seqlens; k.out = a.indices;
    k.lg_bs = a.lg_bs; k.lg_rs = a.lg_rs; k.ix_bs = a.ix_bs; k.ix_ts = a.ix_ts;
    k.nq = (int)a.seqlen_q; k.width = (int)a.width; k.topk = (int)a.topk; k.causal = a.causal ? 1 : 0;
    ProfScope ps(K_IDX_TOPK, st);
    hipLaunchKernelGGL(idx_topk_kernel, dim3((unsigned)a.seqlen_q, (unsigned)a.batch), dim3(kTopkThreads), 0, st, k);
    return hipGetLastError();
}

}  // namespace fa
