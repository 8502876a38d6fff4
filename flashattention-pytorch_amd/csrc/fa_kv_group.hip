// Grouped-query attention, backward: the sum of the dK / dV partials over the query heads of a group.
//
// A grouped backward (kv_group = g > 1) runs the dK / dV kernels as they are, with one output unit per query head: they write
// (bh, nk, d) partial slabs into the workspace.  This kernel adds the g partials of every K/V unit, member 0 first, in fp32 and
// rounds once to the tensor dtype: the result does not depend on the launch, the same bits on every run.  One launch does dK and
// dV: the first half of the grid reads the dK slab, the second half the dV slab.  A lane owns 16 bytes of one output unit (8
// 16-bit or 4 fp32 elements) and reads them with one 16-byte load per member; where a unit's nk * d elements are not a multiple
// of that, or a tensor is not 16-byte aligned, lanes go element by element.
#include "fa_common.h"
#include "fa_kernels.h"

namespace fa {

template <typename T>
__global__ __launch_bounds__(256) void kv_group_sum_kernel(const T* __restrict__ pk, const T* __restrict__ pv, T* __restrict__ dk,
                                                           T* __restrict__ dv, long long per_unit, long long cpu, long long nchunk,
                                                           int g, int vec_ok) {
    constexpr int VEC = 16 / (int)sizeof(T);
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // [0, nchunk): dK chunks, [nchunk, 2 nchunk): dV chunks
    if (i >= 2 * nchunk) return;
    const bool second = i >= nchunk;
    if (second) i -= nchunk;
    const T* src = second ? pv : pk;
    T* dst = second ? dv : dk;
    const long long u = i / cpu, off = (i - u * cpu) * VEC;    // K/V unit, first element of the chunk in it
    const T* s0 = src + (u * g) * per_unit + off;               // member m of the group: s0 + m * per_unit
    T* d0 = dst + u * per_unit + off;
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    if (vec_ok) {
        for (int m = 0; m < g; ++m) {
            const uint4 x = *reinterpret_cast<const uint4*>(s0 + (long long)m * per_unit);
            const T* e = reinterpret_cast<const T*>(&x);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += to_f32<T>(e[j]);
        }
        uint4 y;
        T* e = reinterpret_cast<T*>(&y);
#pragma unroll
        for (int j = 0; j < VEC; ++j) e[j] = from_f32<T>(acc[j]);
        *reinterpret_cast<uint4*>(d0) = y;
        return;
    }
    const int cnt = per_unit - off < VEC ? (int)(per_unit - off) : VEC;   // the unit's last chunk may be short
    for (int m = 0; m < g; ++m)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (j < cnt) acc[j] += to_f32<T>(s0[(long long)m * per_unit + j]);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (j < cnt) d0[j] = from_f32<T>(acc[j]);
}

template <typename T>
static hipError_t kv_group_sum_t(const void* pk, const void* pv, void* dk, void* dv, int64_t bh_kv, int64_t g, int64_t nk, int64_t d,
                                 hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const long long per_unit = (long long)nk * d;
    const long long cpu = (per_unit + VEC - 1) / VEC;   // chunks per unit
    const long long nchunk = cpu * bh_kv;
    if (nchunk == 0) return hipSuccess;
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const int vec_ok = per_unit % VEC == 0 && a16(pk) && a16(pv) && a16(dk) && a16(dv);
    const long long blocks = (2 * nchunk + 255) / 256;
    if (blocks * 256 >= ((long long)1 << 32)) return hipErrorInvalidConfiguration;   // work-items per launch
    ProfScope ps(K_KV_GROUP_SUM, st);
    hipLaunchKernelGGL(kv_group_sum_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)pk, (const T*)pv, (T*)dk, (T*)dv,
                       per_unit, cpu, nchunk, (int)g, vec_ok);
    return hipGetLastError();
}

// One tensor alone (dK and dV of different widths: fa_ex_mfma_vdim.hip): the same sum, member 0 first, fp32, one rounding.
template <typename T>
__global__ __launch_bounds__(256) void kv_group_sum_one_kernel(const T* __restrict__ src, T* __restrict__ dst, long long per_unit,
                                                               long long cpu, long long nchunk, int g, int vec_ok) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    const long long u = i / cpu, off = (i - u * cpu) * VEC;
    const T* s0 = src + (u * g) * per_unit + off;
    T* d0 = dst + u * per_unit + off;
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    if (vec_ok) {
        for (int m = 0; m < g; ++m) {
            const uint4 x = *reinterpret_cast<const uint4*>(s0 + (long long)m * per_unit);
            const T* e = reinterpret_cast<const T*>(&x);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += to_f32<T>(e[j]);
        }
        uint4 y;
        T* e = reinterpret_cast<T*>(&y);
#pragma unroll
        for (int j = 0; j < VEC; ++j) e[j] = from_f32<T>(acc[j]);
        *reinterpret_cast<uint4*>(d0) = y;
        return;
    }
    const int cnt = per_unit - off < VEC ? (int)(per_unit - off) : VEC;
    for (int m = 0; m < g; ++m)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (j < cnt) acc[j] += to_f32<T>(s0[(long long)m * per_unit + j]);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (j < cnt) d0[j] = from_f32<T>(acc[j]);
}

template <typename T>
static hipError_t kv_group_sum_one_t(const void* src, void* dst, int64_t bh_kv, int64_t g, int64_t nk, int64_t d, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const long long per_unit = (long long)nk * d;
    const long long cpu = (per_unit + VEC - 1) / VEC;
    const long long nchunk = cpu * bh_kv;
    if (nchunk == 0) return hipSuccess;
    const int vec_ok = per_unit % VEC == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const long long blocks = (nchunk + 255) / 256;
    if (blocks * 256 >= ((long long)1 << 32)) return hipErrorInvalidConfiguration;
    ProfScope ps(K_KV_GROUP_SUM, st);
    hipLaunchKernelGGL(kv_group_sum_one_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)src, (T*)dst, per_unit, cpu,
                       nchunk, (int)g, vec_ok);
    return hipGetLastError();
}

hipError_t launch_kv_group_sum_one(const void* src, void* dst, int64_t bh_kv, int64_t g, int64_t nk, int64_t d, int dtype,
                                   hipStream_t st) {
    switch (dtype) {
        case 0: return kv_group_sum_one_t<float>(src, dst, bh_kv, g, nk, d, st);
        case 1: return kv_group_sum_one_t<__half>(src, dst, bh_kv, g, nk, d, st);
        default: return kv_group_sum_one_t<__hip_bfloat16>(src, dst, bh_kv, g, nk, d, st);
    }
}

hipError_t launch_kv_group_sum(const void* pk, const void* pv, void* dk, void* dv, int64_t bh_kv, int64_t g, int64_t nk, int64_t d,
                               int dtype, hipStream_t st) {
    switch (dtype) {
        case 0: return kv_group_sum_t<float>(pk, pv, dk, dv, bh_kv, g, nk, d, st);
        case 1: return kv_group_sum_t<__half>(pk, pv, dk, dv, bh_kv, g, nk, d, st);
        default: return kv_group_sum_t<__hip_bfloat16>(pk, pv, dk, dv, bh_kv, g, nk, d, st);
    }
}

}  // namespace fa
