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
// The family is laid out once.  fa_decode_kernels.h has kv_append_kernel<Tag, FEAT> and kv_split_kernel<Tag, D, PAGED, FEAT>:
// FEAT is a set of the bits kKvRot and kKvQ8, and the kernel's one argument KvB<FEAT> is KvParams + KvRot + KvQ8 as far as the
// bits go.  kv_combine_kernel<Tag, SINK> below is the one combine.  kv_dispatch is the one function from a call to its
// instantiation, and KvFeats the list of what the family instantiates.  A feature an instantiation lacks is a discarded
// `if constexpr` branch in it; that a change leaves the other instantiations' instructions alone is shown with
// tools/kernel_diff.py, not kept by copying.
// fa_ex_forward_kvcache_sink (attention sinks) changes the last launch only: kv_combine_kernel<Tag, true> merges the partials with
// one more column, the head's sink logit with a zero value vector, so such a call always has S >= 2 (the C layer raises 1 to 2;
// the second split of a short cache is empty, lse_s = -inf, and is selected away).
// Split ranges come from len_k on the device (kv_split_range), S from the shapes on the host (fa_capi.hip): the call never
// synchronises and never allocates, so it can be captured in a graph.  Keys are addressed per 32-key tile from one base per
// (batch element, K/V head).  fa_ex_forward_kvcache_paged adds three ways to move that base, all in per-sequence key coordinates, so
// the split rule, the masks and the combine do not change:
//   cache_batch_idx : the base is cache row idx[b]; an index outside [0, B_cache) gives an empty buffer range (zeros, no append).
//   cache_leftpad   : the base moves on by P_b = clamp(leftpad[b], 0, L_b) tokens and len_k = L_b + N_new - P_b.
//   block_table     : kv_split_kernel<.., PAGED = true, ..>.  Per tile, lane l looks up the page of key k0 + (l & 31) (one 4-byte
//                     read, the next tile's issued a tile ahead) and keeps the 64-bit element offsets page * page stride + slot *
//                     token stride of K and of V; the lane that loads a key row takes its offset by a lane shuffle and reads with
//                     a global load at a 32-bit offset inside the page.  A key past the split's end or on a page outside
//                     [0, num_blocks) has offset -1 and reads as zeros without touching memory.  The contiguous instantiations
//                     hold none of this.
// fa_ex_forward_kvcache_rotary adds rotary position embedding (kKvRot, KvRot) to the append and the split kernel.  A 16-byte chunk
// (head dims 8 c .. 8 c + 7) is the unit both kernels already move: the append's lane copies one, a q fragment of the split
// kernel is one (c = 4 ks + g).
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
// fa_ex_forward_kvcache_fp8 is an e4m3 cache with per-head scales (kKvQ8, KvQ8): the cache is addressed in bytes, a chunk of 8
// head dims is 8 bytes, K and V chunks are widened to q's 16-bit dtype in registers (kv_q8_widen) on their way into the 16-bit
// loop, k_descale joins on the score and v_descale in the epilogue, and the append quantises (kv_q8_quant).
// fa_ex_forward_kvcache_varlen packs the queries and the new keys (KvParams::cu_q, cu_kn; null = the padded call): q and o
// are (total_q, H_q, d), lse and the partials (H_q, total_q)-major, k_new / v_new (total_k_new, H_kv, d).  Sequence b owns the
// tokens kv_cu_range gives it (untrusted offsets, clamped so that no content leaves the tensors): nq_b query tokens, nnew_b new
// keys, len_k = L_b + nnew_b - P_b and coff = len_k - nq_b as if it were the padded call on b alone.  The split grid is sized for
// max_seqlen_q; a wave whose row tile lies past G * nq_b leaves before its first load.  The append takes its loop bound and its
// source rows from the device.  The combine runs per (packed token, h_q) without a sequence index; tokens that no sequence
// owns are told by the fill the host puts into the lse partials (kv_combine_row) and stay unwritten.  All of it is wave-uniform
// scalar work in every instantiation, a null test on cu_q / cu_kn as for bidx / leftpad.
#include "fa_decode_kernels.h"
#include <algorithm>

namespace fa {

namespace {

// One wave per (b, h_q, token) row (packed queries: per (h_q, packed token)), four rows per workgroup.  The lanes read the S
// lse partials side by side (lane c: splits c, c + 64, ..), reduce max and weight sum over the wave in a fixed shuffle order, and
// park the weights in LDS; then lane c adds head dims 4c .. 4c + 3 of the O partials in split order, eight loads in flight,
// branch-free: a split with lse_s = -inf (empty, or no visible key) has weight 0 and its O partial, which it never wrote, is
// selected away.  A row without any visible key gives o = 0, lse = -inf.  Same bits on every run.
// SINK: head h takes snk = sinks[h % sink_heads] as one more column with a zero value vector:
//   m = max(max_s lse_s, snk),  denom = sum_s exp(lse_s - m) + exp(snk - m),  o = sum_s exp(lse_s - m) O_s / denom,
//   lse = m + log(denom)
// so a row without any visible key gives o = 0, lse = snk exactly (denom = 1), and snk = -inf adds nothing anywhere.
// SINK: the kernel takes two more arguments, Sink = (const float* __restrict__ sinks, int sink_heads), the argument list the
// sink combine had as a kernel of its own (without the __restrict__ hipcc loads the pointer with the row count in one go).
// (mla_combine_kernel has this weight phase once more: as a shared device function it changed the instructions of all three
// kernels and did not hold the timing bar on every row, profiles/decode_refactor.md.)
__device__ __forceinline__ float kv_sink_of(int h, const float* sinks, int sink_heads) { return sinks[h % sink_heads]; }

template <typename Tag, bool SINK, typename... Sink>
__global__ __launch_bounds__(256) void kv_combine_kernel(KvParams p, int S, long long nrows, Sink... sink) {
    static_assert(sizeof...(Sink) == (SINK ? 2 : 0), "SINK: (const float* sinks, int sink_heads) follow");
    __shared__ float wsh[4][256];
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63, DR = p.d;
    const long long row = (long long)blockIdx.x * 4 + wv;
    if (row >= nrows) return;   // (wave-uniform; the LDS rows are wave-private, no barrier)
    const float* pl = p.plse + row * S;
    int h;
    long long orow;
    if (!kv_combine_row(p, row, pl, h, orow)) return;
    float snk = -INFINITY;
    if constexpr (SINK) snk = kv_sink_of(h, sink...);
    float m = -INFINITY;
    for (int s = c; s < S; s += 64) m = fmaxf(m, pl[s]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if constexpr (SINK) m = fmaxf(m, snk);
    float sum = 0.f;
    for (int s = c; s < S; s += 64) {
        const float ls = pl[s];
        const float w = (ls == -INFINITY) ? 0.f : __expf(ls - m);
        wsh[wv][s] = w;
        sum += w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if constexpr (SINK) sum += (snk == -INFINITY) ? 0.f : __expf(snk - m);   // after the wave's reduction, in a fixed place
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

// One call's launches: what the host made of the KvArgs
struct KvCall {
    KvParams p;
    KvRot ro;
    KvQ8 q8;
    int S, row_tiles, batch;
    const float* sinks;   // != null (S >= 2 then): the combine with the sink column
    int sink_heads;
    hipStream_t st;
};

// The launches of one call on its instantiation
template <typename Tag, int D, bool PAGED, int FEAT>
hipError_t kv_launch(const KvCall& c) {
    const KvParams& p = c.p;
    const int S = c.S;
    KvB<FEAT> blk;
    static_cast<KvParams&>(blk) = p;
    if constexpr ((FEAT & kKvRot) != 0) blk.ro = c.ro;
    if constexpr ((FEAT & kKvQ8) != 0) blk.q8 = c.q8;
    hipError_t e = hipSuccess;
    if (p.cu_kn ? p.total_kn > 0 : p.nnew > 0) {
        // (packed k_new: a sequence has at most total_kn tokens; the kernel's loop takes its bound from the device)
        const long long per_b = (long long)(p.cu_kn ? p.total_kn : p.nnew) * p.hkv * (p.d / 8);
        const dim3 grid((unsigned)std::min<long long>((per_b + 255) / 256, 1024), (unsigned)c.batch);
        using ATag = typename std::conditional<FEAT == 0, bf16_tag, Tag>::type;   // FEAT 0 copies bytes: one kernel for both dtypes
        hipLaunchKernelGGL((kv_append_kernel<ATag, FEAT>), grid, dim3(256), 0, c.st, blk);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (c.row_tiles == 0) return e;   // packed queries without a token: the append was the call
    if (p.cu_q && S > 1) {            // rows that no sequence owns keep this fill: kv_combine_row
        e = hipMemsetAsync(p.plse, kPlseFill, (size_t)p.total_q * p.hq * S * 4, c.st);
        if (e != hipSuccess) return e;
    }
    const dim3 sgrid((unsigned)S, (unsigned)(c.row_tiles * p.hkv), (unsigned)c.batch);
    hipLaunchKernelGGL((kv_split_kernel<Tag, D, PAGED, FEAT>), sgrid, dim3(64), 0, c.st, blk);
    e = hipGetLastError();
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = p.cu_q ? (long long)p.total_q * p.hq : (long long)c.batch * p.hq * p.nq;
    const dim3 grid((unsigned)((nrows + 3) / 4));
    if (c.sinks) {
        auto kernel = kv_combine_kernel<Tag, true, const float* __restrict__, int>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c.st, p, S, nrows, c.sinks, c.sink_heads);
    } else {
        hipLaunchKernelGGL((kv_combine_kernel<Tag, false>), grid, dim3(256), 0, c.st, p, S, nrows);
    }
    return hipGetLastError();
}

// The FEAT values the family instantiates: every subset of {kKvRot, kKvQ8}
template <int... F> struct KvFeatList {};
using KvFeats = KvFeatList<0, kKvRot, kKvQ8, kKvRot | kKvQ8>;

// From a call to its instantiation, one axis a function: the dtype (1 = f16, else bf16), head_dim (padded to 64 | 128 | 256),
// paged = table != null, and FEAT = kKvRot if cos != null, | kKvQ8 if cache_e4m3.  A FEAT outside KvFeats is
// hipErrorInvalidValue, never another kernel.
template <typename Tag, int D, bool PAGED, int... F>
hipError_t kv_walk(KvFeatList<F...>, int feat, const KvCall& c) {
    hipError_t e = hipErrorInvalidValue;
    (void)((feat == F && ((e = kv_launch<Tag, D, PAGED, F>(c)), true)) || ...);
    return e;
}
template <typename Tag, int D>
hipError_t kv_dispatch_d(bool paged, int feat, const KvCall& c) {
    return paged ? kv_walk<Tag, D, true>(KvFeats{}, feat, c) : kv_walk<Tag, D, false>(KvFeats{}, feat, c);
}
template <typename Tag>
hipError_t kv_dispatch_t(int d, bool paged, int feat, const KvCall& c) {
    if (d <= 64) return kv_dispatch_d<Tag, 64>(paged, feat, c);
    return d <= 128 ? kv_dispatch_d<Tag, 128>(paged, feat, c) : kv_dispatch_d<Tag, 256>(paged, feat, c);
}
hipError_t kv_dispatch(int dtype, int d, bool paged, bool rotary, bool e4m3, const KvCall& c) {
    const int feat = (rotary ? kKvRot : 0) | (e4m3 ? kKvQ8 : 0);
    return dtype == 1 ? kv_dispatch_t<f16_tag>(d, paged, feat, c) : kv_dispatch_t<bf16_tag>(d, paged, feat, c);
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

hipError_t launch_kv_combine(void* o, float* lse, float* po, float* plse, int64_t batch, int64_t heads_q, int64_t seqlen_q, int64_t d,
                             int dtype, int splits, hipStream_t st) {
    KvParams p{};
    p.o = (uint16_t*)o; p.lse = lse; p.po = po; p.plse = plse;
    p.hq = (int)heads_q; p.nq = (int)seqlen_q; p.d = (int)d;
    const long long nrows = (long long)batch * heads_q * seqlen_q;
    const dim3 grid((unsigned)((nrows + 3) / 4));
    if (dtype == 1) hipLaunchKernelGGL((kv_combine_kernel<f16_tag, false>), grid, dim3(256), 0, st, p, splits, nrows);
    else hipLaunchKernelGGL((kv_combine_kernel<bf16_tag, false>), grid, dim3(256), 0, st, p, splits, nrows);
    return hipGetLastError();
}

hipError_t launch_kv_combine_sink(void* o, float* lse, float* po, float* plse, int64_t batch, int64_t heads_q, int64_t seqlen_q, int64_t d,
                                  int dtype, int splits, const float* sinks, int sink_heads, hipStream_t st) {
    KvParams p{};
    p.o = (uint16_t*)o; p.lse = lse; p.po = po; p.plse = plse;
    p.hq = (int)heads_q; p.nq = (int)seqlen_q; p.d = (int)d;
    const long long nrows = (long long)batch * heads_q * seqlen_q;
    const dim3 grid((unsigned)((nrows + 3) / 4));
    if (dtype == 1) {
        auto kernel = kv_combine_kernel<f16_tag, true, const float* __restrict__, int>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, p, splits, nrows, sinks, sink_heads);
    } else {
        auto kernel = kv_combine_kernel<bf16_tag, true, const float* __restrict__, int>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, p, splits, nrows, sinks, sink_heads);
    }
    return hipGetLastError();
}

hipError_t launch_kv_combine_packed(void* o, float* lse, float* po, float* plse, const int* cu_seqlens_q, int64_t heads_q, int64_t total_q,
                                    int64_t d, int dtype, int splits, const float* sinks, int sink_heads, hipStream_t st) {
    KvParams p{};
    p.o = (uint16_t*)o; p.lse = lse; p.po = po; p.plse = plse;
    p.hq = (int)heads_q; p.d = (int)d;
    p.cu_q = cu_seqlens_q; p.total_q = (int)total_q;   // (the combine tests cu_q against null and never reads it)
    const long long nrows = (long long)total_q * heads_q;
    const dim3 grid((unsigned)((nrows + 3) / 4));
    if (sinks) {
        if (dtype == 1) {
            auto kernel = kv_combine_kernel<f16_tag, true, const float* __restrict__, int>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, p, splits, nrows, sinks, sink_heads);
        } else {
            auto kernel = kv_combine_kernel<bf16_tag, true, const float* __restrict__, int>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, p, splits, nrows, sinks, sink_heads);
        }
    } else if (dtype == 1) hipLaunchKernelGGL((kv_combine_kernel<f16_tag, false>), grid, dim3(256), 0, st, p, splits, nrows);
    else hipLaunchKernelGGL((kv_combine_kernel<bf16_tag, false>), grid, dim3(256), 0, st, p, splits, nrows);
    return hipGetLastError();
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
    KvCall c{};
    c.ro.cos = (const uint16_t*)a.rotary_cos; c.ro.sin = (const uint16_t*)a.rotary_sin;
    c.ro.cos_rs = a.rotary_cos_rs; c.ro.sin_rs = a.rotary_sin_rs;
    c.ro.rdim = (int)a.rotary_dim; c.ro.inter = a.rotary_interleaved; c.ro.qseq = a.rotary_q_per_token;
    c.q8 = KvQ8{a.k_descale, a.v_descale, (long long)a.descale_bstride};
    c.S = S;
    c.batch = (int)a.batch;
    c.row_tiles = ((a.cu_seqlens_q ? p.G * p.max_q : p.rows) + 15) / 16;
    c.sinks = a.sinks;
    c.sink_heads = (int)(a.sink_heads > 0 ? a.sink_heads : 1);
    c.st = st;
    c.p = p;
    return kv_dispatch((int)a.dtype, p.d, p.table != nullptr, c.ro.cos != nullptr, a.cache_e4m3 != 0, c);
}

}  // namespace fa
