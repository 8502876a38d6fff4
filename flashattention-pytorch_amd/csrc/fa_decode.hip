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
// fa_ex_forward_kvcache_sink (attention sinks) changes the last launch only: kv_combine_sink_kernel merges the partials with one
// more column, the head's sink logit with a zero value vector, so such a call always has S >= 2 (the C layer raises 1 to 2; the
// second split of a short cache is empty, lse_s = -inf, and is selected away).  The append and split kernels are the ones above.
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
// fa_ex_forward_kvcache_rotary adds rotary position embedding (KvRot) in kernels of their own, kv_append_rot_kernel and
// kv_split_rot_kernel; the kernels above keep their instruction text.  A 16-byte chunk (head dims 8 c .. 8 c + 7) is the unit both
// kernels already move: the append's lane copies one, a q fragment of the split kernel is one (c = 4 ks + g).
//   interleaved     : the chunk holds pairs (x, y) = (2 j, 2 j + 1), j = 4 c .. 4 c + 3: four table entries, no partner.
//   not interleaved : with half = rotary_dim / 2 (a multiple of 8), the chunk at 8 c < half holds x of pairs j = 8 c .. 8 c + 7 and
//                     its partner, half / 8 chunks further on, their y; the chunk at half <= 8 c < rotary_dim holds y of pairs
//                     j = 8 c - half .., its partner half / 8 chunks back their x.  The lane reads the partner chunk from k_new / q
//                     as well.  Either way out = own * cos[j] + sgn * partner * sin[j], sgn = -1 for an x chunk, +1 for a y chunk.
//   Chunks at and past rotary_dim pass through.  fp32 from the 16-bit inputs (the products are exact), one rounding to 16 bits.
//   Positions are in the sequence's key coordinates: new key n at L_b - P_b + n (the rotated value is what the cache gets), q
//   token i at L_b - P_b + i when causal or a window bound was given (qseq), else at L_b - P_b.  q is rotated in the prologue, after
//   the fragments are loaded; nothing of it lives into the key loop.  The tables are read without a device check: the C layer
//   requires seqlen_ro >= capacity + max(0, seqlen_q - seqlen_new), and L_b <= capacity - seqlen_new after the clamp.
// fa_ex_forward_kvcache_varlen packs the queries and the new keys (KvParams::cu_q, cu_kn; null = the padded call): q and o
// are (total_q, H_q, d), lse and the partials (H_q, total_q)-major, k_new / v_new (total_k_new, H_kv, d).  Sequence b owns the
// tokens kv_cu_range gives it (untrusted offsets, clamped so that no content leaves the tensors): nq_b query tokens, nnew_b new
// keys, len_k = L_b + nnew_b - P_b and coff = len_k - nq_b as if it were the padded call on b alone.  The split grid is sized for
// max_seqlen_q; a wave whose row tile lies past G * nq_b leaves before its first load.  The append takes its loop bound and its
// source rows from the device.  The combine runs per (packed token, h_q) without a sequence index; tokens that no sequence
// owns are told by the fill the host puts into the lse partials (kv_combine_row) and stay unwritten.  All of it is wave-uniform
// scalar work in the existing instantiations, a null test on cu_q / cu_kn as for bidx / leftpad.
#include "fa_decode_common.h"
#include <algorithm>

namespace fa {

namespace {

// Rotary embedding (fa_ex_forward_kvcache_rotary): the second argument of the *_rot kernels
struct KvRot {
    const uint16_t *cos, *sin;   // (seqlen_ro, rdim / 2) in q's dtype, 4-byte aligned, rows at the even strides cos_rs / sin_rs
    long long cos_rs, sin_rs;
    int rdim, inter, qseq;       // qseq: q token i at position L_b - P_b + i (causal or a window bound given), else all at L_b - P_b
};

// the first head dim of the chunk that holds the other halves of the pairs of the chunk at col (col < rdim); not interleaved only
__device__ __forceinline__ int kv_rot_partner(const KvRot& ro, int col) {
    const int half = ro.rdim >> 1;
    return col < half ? col + half : col - half;
}

// The chunk at head dims col .. col + 7 (col < rdim) of a token at table row pos, rotated: own = the chunk, par = its partner
// chunk (not interleaved; unused otherwise).  See the head of this file.
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

// e4m3 cache (fa_ex_forward_kvcache_fp8): the last argument of the *_q8 kernels.  The scale of (b, K/V head) is kd[b * bs + hk]
// (vd likewise); null = 1.0.  The KvParams cache pointers then address bytes, and the cache strides are in bytes as well.
struct KvQ8 {
    const float *kd, *vd;
    long long bs;
};

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

// kv_append_kernel and kv_split_kernel, then the same source with the rotation compiled in: kv_append_rot_kernel and
// kv_split_rot_kernel, which take a KvRot beside the KvParams; then both again for an e4m3 cache (KV_Q8): kv_append_q8_kernel,
// kv_split_q8_kernel, kv_append_rot_q8_kernel and kv_split_rot_q8_kernel, which take a KvQ8 as well
#define KV_Q8 0
#define KV_ROT 0
#include "fa_decode_kernels.inc"
#undef KV_ROT
#define KV_ROT 1
#include "fa_decode_kernels.inc"
#undef KV_ROT
#undef KV_Q8
#define KV_Q8 1
#define KV_ROT 0
#include "fa_decode_kernels.inc"
#undef KV_ROT
#define KV_ROT 1
#include "fa_decode_kernels.inc"
#undef KV_ROT
#undef KV_Q8

// One wave per (b, h_q, token) row (packed queries: per (h_q, packed token)), four rows per workgroup.  The lanes read the S
// lse partials side by side (lane c: splits
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
    if (4 * c < DR) {
        u32x2 v;
        v[0] = pack2_rn<Tag>(acc[0] * inv, acc[1] * inv);
        v[1] = pack2_rn<Tag>(acc[2] * inv, acc[3] * inv);
        *reinterpret_cast<u32x2*>(p.o + orow * DR + 4 * c) = v;
    }
    if (c == 0) p.lse[row] = sum > 0.f ? m + logf(sum) : -INFINITY;
}

// kv_combine_kernel with the sink column (a kernel of its own: the one above keeps its instruction text).  Head h takes
// snk = sinks[h % sink_heads] and
//   m = max(max_s lse_s, snk),  denom = sum_s exp(lse_s - m) + exp(snk - m),  o = sum_s exp(lse_s - m) O_s / denom,
//   lse = m + log(denom)
// so a row without any visible key gives o = 0, lse = snk exactly (denom = 1).  snk = -inf adds nothing anywhere: the bits of
// kv_combine_kernel.  The sink is added to the denominator after the wave's reduction, in a fixed place.
template <typename Tag>
__global__ __launch_bounds__(256) void kv_combine_sink_kernel(KvParams p, int S, long long nrows, const float* __restrict__ sinks,
                                                              int sink_heads) {
    __shared__ float wsh[4][256];
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63, DR = p.d;
    const long long row = (long long)blockIdx.x * 4 + wv;
    if (row >= nrows) return;   // (wave-uniform; the LDS rows are wave-private, no barrier)
    const float* pl = p.plse + row * S;
    int h;
    long long orow;
    if (!kv_combine_row(p, row, pl, h, orow)) return;
    const float snk = sinks[h % sink_heads];
    float m = -INFINITY;
    for (int s = c; s < S; s += 64) m = fmaxf(m, pl[s]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    m = fmaxf(m, snk);
    float sum = 0.f;
    for (int s = c; s < S; s += 64) {
        const float ls = pl[s];
        const float w = (ls == -INFINITY) ? 0.f : __expf(ls - m);
        wsh[wv][s] = w;
        sum += w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    sum += (snk == -INFINITY) ? 0.f : __expf(snk - m);
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
    if (4 * c < DR) {
        u32x2 v;
        v[0] = pack2_rn<Tag>(acc[0] * inv, acc[1] * inv);
        v[1] = pack2_rn<Tag>(acc[2] * inv, acc[3] * inv);
        *reinterpret_cast<u32x2*>(p.o + orow * DR + 4 * c) = v;
    }
    if (c == 0) p.lse[row] = sum > 0.f ? m + logf(sum) : -INFINITY;
}

template <typename Tag, int D>
hipError_t launch_split(const KvParams& p, const KvRot& ro, const KvQ8* q8, int S, int row_tiles, int batch, hipStream_t st) {
    const dim3 grid((unsigned)S, (unsigned)(row_tiles * p.hkv), (unsigned)batch);
    if (q8) {
        if (ro.cos) {
            if (p.table) hipLaunchKernelGGL((kv_split_rot_q8_kernel<Tag, D, true>), grid, dim3(64), 0, st, p, ro, *q8);
            else hipLaunchKernelGGL((kv_split_rot_q8_kernel<Tag, D, false>), grid, dim3(64), 0, st, p, ro, *q8);
        } else if (p.table)
            hipLaunchKernelGGL((kv_split_q8_kernel<Tag, D, true>), grid, dim3(64), 0, st, p, *q8);
        else
            hipLaunchKernelGGL((kv_split_q8_kernel<Tag, D, false>), grid, dim3(64), 0, st, p, *q8);
    } else if (ro.cos) {
        if (p.table) hipLaunchKernelGGL((kv_split_rot_kernel<Tag, D, true>), grid, dim3(64), 0, st, p, ro);
        else hipLaunchKernelGGL((kv_split_rot_kernel<Tag, D, false>), grid, dim3(64), 0, st, p, ro);
    } else if (p.table)
        hipLaunchKernelGGL((kv_split_kernel<Tag, D, true>), grid, dim3(64), 0, st, p);
    else
        hipLaunchKernelGGL((kv_split_kernel<Tag, D, false>), grid, dim3(64), 0, st, p);
    return hipGetLastError();
}

// sinks != null (S >= 2 then): the combine with the sink column
template <typename Tag>
hipError_t launch_kv_t(const KvParams& p, const KvRot& ro, const KvQ8* q8, int S, int row_tiles, int batch, hipStream_t st,
                       const float* sinks, int sink_heads) {
    hipError_t e = hipSuccess;
    if (p.cu_kn ? p.total_kn > 0 : p.nnew > 0) {
        // (packed k_new: a sequence has at most total_kn tokens; the kernel's loop takes its bound from the device)
        const long long per_b = (long long)(p.cu_kn ? p.total_kn : p.nnew) * p.hkv * (p.d / 8);
        const dim3 grid((unsigned)std::min<long long>((per_b + 255) / 256, 1024), (unsigned)batch);
        if (q8 && ro.cos) hipLaunchKernelGGL(kv_append_rot_q8_kernel<Tag>, grid, dim3(256), 0, st, p, ro, *q8);
        else if (q8) hipLaunchKernelGGL(kv_append_q8_kernel<Tag>, grid, dim3(256), 0, st, p, *q8);
        else if (ro.cos) hipLaunchKernelGGL(kv_append_rot_kernel<Tag>, grid, dim3(256), 0, st, p, ro);
        else hipLaunchKernelGGL(kv_append_kernel, grid, dim3(256), 0, st, p);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (row_tiles == 0) return e;   // packed queries without a token: the append was the call
    if (p.cu_q && S > 1) {          // rows that no sequence owns keep this fill: kv_combine_row
        e = hipMemsetAsync(p.plse, kPlseFill, (size_t)p.total_q * p.hq * S * 4, st);
        if (e != hipSuccess) return e;
    }
    if (p.d <= 64) e = launch_split<Tag, 64>(p, ro, q8, S, row_tiles, batch, st);
    else if (p.d <= 128) e = launch_split<Tag, 128>(p, ro, q8, S, row_tiles, batch, st);
    else e = launch_split<Tag, 256>(p, ro, q8, S, row_tiles, batch, st);
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = p.cu_q ? (long long)p.total_q * p.hq : (long long)batch * p.hq * p.nq;
    if (sinks)
        hipLaunchKernelGGL((kv_combine_sink_kernel<Tag>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, p, S, nrows, sinks, sink_heads);
    else
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
    if (a.qv) return launch_kvcache_mla(a, st);   // K and V of different widths with a second query operand: fa_mla.hip
    KvParams p = kv_make_params(a);
    const int S = (int)a.num_splits;
    if (a.sinks && S < 2) return hipErrorInvalidValue;   // (the C layer raises a sink call's S to 2: the sink joins in the combine)
    p.po = (float*)a.workspace;
    // workspace (S > 1): the O partials, then the lse partials, each rounded up to 256 bytes (kv_workspace_bytes)
    const size_t q_rows = a.cu_seqlens_q ? (size_t)a.total_q * a.heads_q : (size_t)a.batch * a.heads_q * a.seqlen_q;
    p.plse = S > 1 ? (float*)((char*)a.workspace + ((q_rows * S * a.d * 4 + 255) & ~(size_t)255)) : nullptr;
    KvRot ro{};
    ro.cos = (const uint16_t*)a.rotary_cos; ro.sin = (const uint16_t*)a.rotary_sin;
    ro.cos_rs = a.rotary_cos_rs; ro.sin_rs = a.rotary_sin_rs;
    ro.rdim = (int)a.rotary_dim; ro.inter = a.rotary_interleaved; ro.qseq = a.rotary_q_per_token;
    const KvQ8 q8{a.k_descale, a.v_descale, (long long)a.descale_bstride};
    const KvQ8* q8p = a.cache_e4m3 ? &q8 : nullptr;
    const int batch = (int)a.batch;
    const int row_tiles = ((a.cu_seqlens_q ? p.G * p.max_q : p.rows) + 15) / 16;
    const int sink_heads = (int)(a.sink_heads > 0 ? a.sink_heads : 1);
    return a.dtype == 1 ? launch_kv_t<f16_tag>(p, ro, q8p, S, row_tiles, batch, st, a.sinks, sink_heads)
                        : launch_kv_t<bf16_tag>(p, ro, q8p, S, row_tiles, batch, st, a.sinks, sink_heads);
}

}  // namespace fa
