// Merge of two partial attention results (fa_merge_states / fa_merge_states_backward; include/fa_mi355x.h): (o_a, lse_a) and
// (o_b, lse_b) are attention of the same queries over two disjoint key sets, and
//     lse = logaddexp(lse_a, lse_b),   w_x = exp(lse_x - lse),   o = w_a o_a + w_b o_b
// is attention over their union.  Two memory-bound kernels, forward and backward, each one launch.
//   addressing   : every tensor by (batch, head, row) through its own stride triple (elements), 64-bit offsets; the d elements of
//                  an o-like row are contiguous.  That covers (B, H, N, d), (B, N, H, d) and packed (T, H, d) with lse (B, H, N) or
//                  (H, T) without a copy.
//   lanes        : 8 lanes own one row.  Lane c moves the 16-byte chunks c, c + 8, .. of the row (CPL of them at most: 8 16-bit
//                  or 4 fp32 elements each; fp32 rows that 16-byte accesses cannot address take 4-byte chunks).  A wave takes
//                  64 consecutive rows per step (a workgroup of 256 threads 256 rows): lane l alone reads lse_a, lse_b (and
//                  dlse) of row base + l, forms that row's weights once, in fp64 around the larger lse, and alone writes its lse;
//                  then eight passes of eight rows, the eight lanes of a row fetching its weights from the lane that formed
//                  them by a shuffle.  So the fp64 exp / log run on full waves, once per row.
//   arithmetic   : a 16-bit or fp32 element times an fp64 weight is exact in fp64, so w_a o_a + w_b o_b carries one fp64 rounding
//                  (2^-53, also under cancellation of the two terms, where fp32 weights would leave an error of 2^-24 of the larger
//                  term); it is then rounded to fp32 and, for 16-bit tensors, to the tensor dtype, to nearest even.  A side with
//                  weight 0 (lse_x = -inf, or exp underflow) is not used: its elements are replaced by 0 before the product, so NaN
//                  or garbage there never reaches the result and the other side comes back with its own bits.  Both -inf: o = 0,
//                  lse = -inf.
//   in place     : o == o_a and lse == lse_a (equal strides) is allowed: a chunk is loaded by the lane that stores it, before that
//                  store, and a row's lse is read and written by one lane only.
//   backward     : t = <dO, o_a - o_b> per row as an fp32 sum: each lane over its chunks in order, then xor-shuffles 1, 2, 4 inside
//                  the row's lanes: a fixed order, the same bits on every run.  dO_x = w_x dO, dlse_a = w_a (dlse + w_b t),
//                  dlse_b = w_b (dlse - w_a t); a side with weight 0 gets zeros and t is not used (it may hold that side's NaN);
//                  both -inf: zeros everywhere.  dO stays in registers between the two uses.
// Grid: (x, y), y over the (batch, head) units and x over a unit's 256-row groups, about 2048 workgroups in all, grid-stride loops
// in both.  No LDS, no scratch.  Nothing is read on the host.
#include "fa_common.h"
#include "fa_kernels.h"
#include <algorithm>

namespace fa {

namespace {

constexpr int kMergeLanes = 8;                        // lanes per row
constexpr int kMergeRowsPerPass = 64 / kMergeLanes;   // rows a wave moves at once
constexpr int kMergeRows = 256;                       // rows per workgroup and step: 64 per wave, in 8 passes

struct MgT {
    void* p;
    long long bs, hs, rs;
};
struct MgParams {
    MgT o_a, lse_a, o_b, lse_b, o, lse, dout, dlse, do_a, do_b, dlse_a, dlse_b;
    long long units, heads, rows;
    int nchunks;   // chunks per row
};

struct f32_tag {};

// one chunk of a row: VEC elements, read and written at once
template <typename Tag, int VEC> struct MgChunk;
template <typename Tag> struct MgChunk<Tag, 8> {   // eight 16-bit elements
    typedef uint16_t elem;
    u32x4 v;
    __device__ __forceinline__ void load(const elem* p) { v = *reinterpret_cast<const u32x4*>(p); }
    __device__ __forceinline__ void store(elem* p) const { *reinterpret_cast<u32x4*>(p) = v; }
    __device__ __forceinline__ float get(int j) const { return (j & 1) ? unpack_hi<Tag>(v[j >> 1]) : unpack_lo<Tag>(v[j >> 1]); }
    template <typename F> __device__ __forceinline__ void fill(F f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = pack2_rn<Tag>(f(2 * j), f(2 * j + 1));
    }
};
template <> struct MgChunk<f32_tag, 4> {
    typedef float elem;
    float4 v;
    __device__ __forceinline__ void load(const elem* p) { v = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ void store(elem* p) const { *reinterpret_cast<float4*>(p) = v; }
    __device__ __forceinline__ float get(int j) const { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
    template <typename F> __device__ __forceinline__ void fill(F f) { v.x = f(0); v.y = f(1); v.z = f(2); v.w = f(3); }
};
template <> struct MgChunk<f32_tag, 1> {
    typedef float elem;
    float v;
    __device__ __forceinline__ void load(const elem* p) { v = *p; }
    __device__ __forceinline__ void store(elem* p) const { *p = v; }
    __device__ __forceinline__ float get(int) const { return v; }
    template <typename F> __device__ __forceinline__ void fill(F f) { v = f(0); }
};

__device__ __forceinline__ long long mg_off(const MgT& t, long long b, long long h, long long i) { return b * t.bs + h * t.hs + i * t.rs; }

// the weights of a row from its two lse, formed around the larger one; l: the merged lse
__device__ __forceinline__ void mg_weights(float la, float lb, double& wa, double& wb, float& l) {
    const float m = fmaxf(la, lb);
    if (m == -INFINITY) {   // no visible key on either side
        wa = 0.0; wb = 0.0; l = -INFINITY;
        return;
    }
    const double ea = exp((double)la - (double)m), eb = exp((double)lb - (double)m), s = ea + eb;   // the larger side's is 1
    wa = ea / s;
    wb = eb / s;
    l = (float)((double)m + log(s));
}

// A wave takes 64 consecutive rows of a unit per step: lane l forms the weights of row base + l (and writes that row's lse, or
// holds its dlse), then eight passes of eight rows each, the eight lanes of a row fetching the row's weights by a shuffle.
template <typename Tag, int VEC, int CPL>
__global__ __launch_bounds__(256) void merge_fwd_kernel(MgParams p) {
    typedef MgChunk<Tag, VEC> C;
    typedef typename C::elem E;
    constexpr int L = kMergeLanes, PASSES = 64 / kMergeRowsPerPass;
    const int wl = threadIdx.x & 63, lane = wl & (L - 1), sub = wl / L;
    for (long long u = blockIdx.y; u < p.units; u += gridDim.y) {
        const long long b = u / p.heads, h = u - b * p.heads;
        for (long long base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < p.rows; base += (long long)gridDim.x * kMergeRows) {
            double wa = 0.0, wb = 0.0;
            if (base + wl < p.rows) {   // this lane's row: read both lse, write the merged one
                float l;
                mg_weights(reinterpret_cast<const float*>(p.lse_a.p)[mg_off(p.lse_a, b, h, base + wl)],
                           reinterpret_cast<const float*>(p.lse_b.p)[mg_off(p.lse_b, b, h, base + wl)], wa, wb, l);
                reinterpret_cast<float*>(p.lse.p)[mg_off(p.lse, b, h, base + wl)] = l;
            }
            for (int pass = 0; pass < PASSES; ++pass) {
                const int src = pass * kMergeRowsPerPass + sub;
                const double ra = __shfl(wa, src, 64), rb = __shfl(wb, src, 64);
                const long long i = base + src;
                if (i >= p.rows) continue;
                const E* xa = reinterpret_cast<const E*>(p.o_a.p) + mg_off(p.o_a, b, h, i);
                const E* xb = reinterpret_cast<const E*>(p.o_b.p) + mg_off(p.o_b, b, h, i);
                E* y = reinterpret_cast<E*>(p.o.p) + mg_off(p.o, b, h, i);
                C ca[CPL], cb[CPL];
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int c = lane + k * L;
                    if (c < p.nchunks) {
                        ca[k].load(xa + (long long)c * VEC);
                        cb[k].load(xb + (long long)c * VEC);
                    }
                }
                const bool use_a = ra > 0.0, use_b = rb > 0.0;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int c = lane + k * L;
                    if (c < p.nchunks) {
                        C out;
                        out.fill([&](int j) {
                            const double a = use_a ? (double)ca[k].get(j) : 0.0, bb = use_b ? (double)cb[k].get(j) : 0.0;
                            return (float)fma(ra, a, rb * bb);
                        });
                        out.store(y + (long long)c * VEC);
                    }
                }
            }
        }
    }
}

template <typename Tag, int VEC, int CPL>
__global__ __launch_bounds__(256) void merge_bwd_kernel(MgParams p) {
    typedef MgChunk<Tag, VEC> C;
    typedef typename C::elem E;
    constexpr int L = kMergeLanes, PASSES = 64 / kMergeRowsPerPass;
    const int wl = threadIdx.x & 63, lane = wl & (L - 1), sub = wl / L;
    for (long long u = blockIdx.y; u < p.units; u += gridDim.y) {
        const long long b = u / p.heads, h = u - b * p.heads;
        for (long long base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < p.rows; base += (long long)gridDim.x * kMergeRows) {
            double wa = 0.0, wb = 0.0, g = 0.0;
            if (base + wl < p.rows) {
                float l;
                mg_weights(reinterpret_cast<const float*>(p.lse_a.p)[mg_off(p.lse_a, b, h, base + wl)],
                           reinterpret_cast<const float*>(p.lse_b.p)[mg_off(p.lse_b, b, h, base + wl)], wa, wb, l);
                if (p.dlse.p && l != -INFINITY) g = (double)reinterpret_cast<const float*>(p.dlse.p)[mg_off(p.dlse, b, h, base + wl)];
            }
            for (int pass = 0; pass < PASSES; ++pass) {
                const int src = pass * kMergeRowsPerPass + sub;
                const double ra = __shfl(wa, src, 64), rb = __shfl(wb, src, 64), rg = __shfl(g, src, 64);
                const long long i = base + src;
                const bool live = i < p.rows;
                const bool both = live && ra > 0.0 && rb > 0.0;   // t only matters where both sides count; a dead side may hold NaN
                const long long ii = live ? i : 0;
                const E* xa = reinterpret_cast<const E*>(p.o_a.p) + mg_off(p.o_a, b, h, ii);
                const E* xb = reinterpret_cast<const E*>(p.o_b.p) + mg_off(p.o_b, b, h, ii);
                const E* xg = reinterpret_cast<const E*>(p.dout.p) + mg_off(p.dout, b, h, ii);
                C cg[CPL];
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int c = lane + k * L;
                    if (live && c < p.nchunks) {
                        cg[k].load(xg + (long long)c * VEC);
                        if (both) {
                            C ca, cb;
                            ca.load(xa + (long long)c * VEC);
                            cb.load(xb + (long long)c * VEC);
#pragma unroll
                            for (int j = 0; j < VEC; ++j) t += cg[k].get(j) * (ca.get(j) - cb.get(j));
                        }
                    }
                }
                t += __shfl_xor(t, 1, 64);   // (the row's eight lanes are neighbours; every lane of the wave is here)
                t += __shfl_xor(t, 2, 64);
                t += __shfl_xor(t, 4, 64);
                if (!live) continue;
                E* ya = reinterpret_cast<E*>(p.do_a.p) + mg_off(p.do_a, b, h, i);
                E* yb = reinterpret_cast<E*>(p.do_b.p) + mg_off(p.do_b, b, h, i);
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int c = lane + k * L;
                    if (c < p.nchunks) {
                        C out;
                        out.fill([&](int j) { return (float)(ra * (double)cg[k].get(j)); });
                        out.store(ya + (long long)c * VEC);
                        out.fill([&](int j) { return (float)(rb * (double)cg[k].get(j)); });
                        out.store(yb + (long long)c * VEC);
                    }
                }
                if (lane == 0) {
                    const double tt = both ? (double)t : 0.0;
                    reinterpret_cast<float*>(p.dlse_a.p)[mg_off(p.dlse_a, b, h, i)] = ra > 0.0 ? (float)(ra * (rg + rb * tt)) : 0.f;
                    reinterpret_cast<float*>(p.dlse_b.p)[mg_off(p.dlse_b, b, h, i)] = rb > 0.0 ? (float)(rb * (rg - ra * tt)) : 0.f;
                }
            }
        }
    }
}

MgT mg_t(const MergeTensor& t) { return MgT{const_cast<void*>(t.p), (long long)t.bs, (long long)t.hs, (long long)t.rs}; }

template <typename Tag, int VEC, int CPL>
hipError_t merge_launch(const MgParams& p, bool backward, dim3 grid, hipStream_t st) {
    if (backward)
        hipLaunchKernelGGL((merge_bwd_kernel<Tag, VEC, CPL>), grid, dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL((merge_fwd_kernel<Tag, VEC, CPL>), grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

// CPL: the chunks a lane moves per row, the next power of two
template <typename Tag, int VEC, int MAXCPL>
hipError_t merge_by_cpl(const MgParams& p, bool backward, dim3 grid, hipStream_t st) {
    const int cpl = (p.nchunks + kMergeLanes - 1) / kMergeLanes;
    if (cpl <= 1) return merge_launch<Tag, VEC, 1>(p, backward, grid, st);
    if (cpl <= 2) return merge_launch<Tag, VEC, 2>(p, backward, grid, st);
    if (cpl <= 4) return merge_launch<Tag, VEC, 4>(p, backward, grid, st);
    if constexpr (MAXCPL >= 8)
        if (cpl <= 8) return merge_launch<Tag, VEC, 8>(p, backward, grid, st);
    if constexpr (MAXCPL >= 32) {
        if (cpl <= 16) return merge_launch<Tag, VEC, 16>(p, backward, grid, st);
        if (cpl <= 32) return merge_launch<Tag, VEC, 32>(p, backward, grid, st);
    }
    return hipErrorInvalidValue;   // (d > 256: the C layer refuses it)
}

}  // namespace

hipError_t launch_merge(const MergeArgs& a, bool backward, hipStream_t st) {
    MgParams p;
    p.o_a = mg_t(a.o_a); p.lse_a = mg_t(a.lse_a); p.o_b = mg_t(a.o_b); p.lse_b = mg_t(a.lse_b);
    p.o = mg_t(a.o); p.lse = mg_t(a.lse); p.dout = mg_t(a.dout); p.dlse = mg_t(a.dlse);
    p.do_a = mg_t(a.do_a); p.do_b = mg_t(a.do_b); p.dlse_a = mg_t(a.dlse_a); p.dlse_b = mg_t(a.dlse_b);
    p.units = a.batch * a.heads; p.heads = a.heads; p.rows = a.rows;
    if (p.units <= 0 || p.rows <= 0) return hipSuccess;
    const long long want = (p.rows + kMergeRows - 1) / kMergeRows;
    const long long gy = std::min<long long>(p.units, 2048), gx = std::min(want, std::max<long long>(1, 2048 / gy));
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (a.dtype == 0) {
        if (a.vec) {
            p.nchunks = (int)(a.d / 4);
            return merge_by_cpl<f32_tag, 4, 8>(p, backward, grid, st);
        }
        p.nchunks = (int)a.d;
        return merge_by_cpl<f32_tag, 1, 32>(p, backward, grid, st);
    }
    p.nchunks = (int)(a.d / 8);
    return a.dtype == 2 ? merge_by_cpl<bf16_tag, 8, 4>(p, backward, grid, st) : merge_by_cpl<f16_tag, 8, 4>(p, backward, grid, st);
}

}  // namespace fa
