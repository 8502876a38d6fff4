// The fp8 quantiser (fa_fp8_quantize; include/fa_mi355x.h): one 16-bit tensor x -> e4m3 codes and one float32 descale per scale
// unit (b, j) = heads [j g, (j + 1) g) x the tokens of sequence b x d, the producer of the tensors the fp8 calls read.  Memory bound.
//   item        : what one thread moves per step, fa_rotary.hip's unit.  Without tables, and for head dims at and past rotary_dim:
//                 one 16-byte chunk of 8 head dims.  Interleaved tables: one chunk, four pairs, self-contained.  Not interleaved:
//                 the chunk at 8 u < half AND its partner at 8 u + half, so the thread that owns a pair loads both members.
//                 Item t of a unit: u = t % units, head j g + (t / units) % g, token t / units / g, so consecutive lanes read
//                 consecutive chunks of a head row and then of the next head of the group.
//   rotation    : kv_rotate_chunk's arithmetic as fa_rotary.hip restates it: fp32 from the 16-bit inputs, own * cos + partner *
//                 (sgn * sin), both products exact, ONE rounding to nearest even to x's dtype (pack2_rn).  amax and codes are taken
//                 from those 16-bit values, so the call equals itself without tables on fa_rotary_apply's result.
//   codes       : the e4m3 append's arithmetic (fa_decode_kernels.h: kv_q8_quant, kinv), restated: inv = 1 / descale (IEEE),
//                 y = min(max(float(x) * inv, -448), 448), v_cvt_pk_fp8_f32 (nearest even); one 8-byte store a chunk.
//   descale     : amax > 0 ? amax / 448 (IEEE) : 1; pow2: fa_mla_fp8_pack's rule, restated (a mantissa that is not zero: the next
//                 exponent, in the bit pattern).
//   amax        : |.| and max into one register a thread, __shfl_xor over the wave, four floats through LDS, and between the
//                 workgroups of a unit atomicMax on the uint bits of the non-negative float (a vector atomic; the bits of
//                 non-negative floats order as the floats do) into a scratch that a small kernel zeroes first.  A maximum
//                 does not depend on the order: the same bits on every run and on every route.
// Kernels: fp8q_kernel<Tag, MODE>.  kAmax: pass one of the two-pass route.  kQuant: pass two (descale from the scratch) or the
// static call (descale from the caller).  kFused: one workgroup a unit of at most kFp8QuantFused items, held in registers between
// the maximum and the codes.  Grid: (unit, workgroup of the unit) folded into gridDim.x, about 2048 workgroups of 256 threads in
// all and a stride loop over the unit's items.  Offsets are 64-bit; packed sequences come from seq_span, so nothing outside x and
// out is addressed whatever cu_seqlens holds.  Nothing is read on the host.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"
#include <algorithm>

namespace fa {

namespace {

enum { kAmax = 0, kQuant = 1, kFused = 2 };
constexpr int kThreads = 256;
constexpr int kHeld = (int)(kFp8QuantFused / kThreads);   // items a thread of the fused kernel holds

struct Q8Params {
    const uint16_t* x;
    uint8_t* out;
    const float* ds;               // static descales, or null
    float* ds_out;                 // or null (static only)
    unsigned* amax;                // the scratch of the two-pass route: one word a unit
    const uint16_t *cos, *sin;     // null: no rotation
    const int *offs, *cu;          // seqlen_offsets (batch,), cu_seqlens (batch + 1,): untrusted device memory, or null
    long long x_bs, x_hs, x_ts, o_bs, o_hs, o_ts, ds_bs, cos_rs, sin_rs, ro_len, off0;
    int S, total;                  // tokens a sequence has at most (seqlen, or max_seqlen); tokens of a packed tensor
    int g, nj, d, rdim, inter, pow2;
    int nrot, units;               // rotating items per head row, all items per head row
    int nchunk;                    // workgroups a unit (kFused: 1)
};

typedef u32x4 chunk_t;

// the sequence and the heads of a unit
struct Q8Unit {
    long long xb, ob, pos0;
    int len, h0;
    unsigned items;
};

__device__ __forceinline__ Q8Unit q8_unit(const Q8Params& p, unsigned unit) {
    const int b = (int)(unit / (unsigned)p.nj), j = (int)(unit - (unsigned)b * (unsigned)p.nj);
    int start = 0, len = p.S;
    if (p.cu) seq_span(p.cu, b, p.total, p.S, start, len);
    Q8Unit s;
    s.len = len;
    s.h0 = j * p.g;
    s.xb = p.cu ? (long long)start * p.x_ts : b * p.x_bs;
    s.ob = p.cu ? (long long)start * p.o_ts : b * p.o_bs;
    s.pos0 = p.off0 + (p.offs ? (long long)p.offs[b] : 0LL);
    s.items = (unsigned)len * (unsigned)p.g * (unsigned)p.units;   // < 2^31: checked on the host against S
    return s;
}

// an item: its 16-bit values after the rotation (b: the partner chunk of a non-interleaved pair) and where its codes go
struct Q8Item {
    chunk_t a, b;
    long long o;     // byte offset of chunk a in out; chunk b at o + rdim / 2
    bool two;
};

template <typename Tag> __device__ __forceinline__ Q8Item q8_load(const Q8Params& p, const Q8Unit& s, unsigned t) {
    const unsigned r = t / (unsigned)p.units;
    const int u = (int)(t - r * (unsigned)p.units);
    const unsigned i = r / (unsigned)p.g;                           // the sequence's token
    const int h = s.h0 + (int)(r - i * (unsigned)p.g);
    const uint16_t* xr = p.x + s.xb + h * p.x_hs + (long long)i * p.x_ts;
    const long long orow = s.ob + h * p.o_hs + (long long)i * p.o_ts;
    Q8Item it;
    it.two = false;
    if (u >= p.nrot) {                                              // no rotation for these head dims (or for any)
        const int col = p.rdim + 8 * (u - p.nrot);
        it.a = *reinterpret_cast<const chunk_t*>(xr + col);
        it.b = it.a;
        it.o = orow + col;
        return it;
    }
    const long long pos = s.pos0 + i;
    const bool rot = pos >= 0 && pos < p.ro_len;
    const int col = 8 * u;
    it.o = orow + col;
    if (p.inter) {
        const chunk_t own = *reinterpret_cast<const chunk_t*>(xr + col);
        it.a = own;
        if (rot) {
            const uint32_t* cp = reinterpret_cast<const uint32_t*>(p.cos + pos * p.cos_rs + (col >> 1));
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(p.sin + pos * p.sin_rs + (col >> 1));
            const uint32_t c2[2] = {cp[0], cp[1]}, s2[2] = {sp[0], sp[1]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xv = unpack_lo<Tag>(own[e]), yv = unpack_hi<Tag>(own[e]);
                const float c = (e & 1) ? unpack_hi<Tag>(c2[e >> 1]) : unpack_lo<Tag>(c2[e >> 1]);
                const float sn = (e & 1) ? unpack_hi<Tag>(s2[e >> 1]) : unpack_lo<Tag>(s2[e >> 1]);
                it.a[e] = pack2_rn<Tag>(xv * c - yv * sn, xv * sn + yv * c);
            }
        }
        it.b = it.a;
    } else {
        const int half = p.rdim >> 1;
        const chunk_t xs = *reinterpret_cast<const chunk_t*>(xr + col), ys = *reinterpret_cast<const chunk_t*>(xr + col + half);
        it.a = xs;
        it.b = ys;
        it.two = true;
        if (rot) {
            const uint32_t* cp = reinterpret_cast<const uint32_t*>(p.cos + pos * p.cos_rs + col);
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(p.sin + pos * p.sin_rs + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t c2 = cp[e], s2 = sp[e];
                const float clo = unpack_lo<Tag>(c2), chi = unpack_hi<Tag>(c2), slo = unpack_lo<Tag>(s2), shi = unpack_hi<Tag>(s2);
                // own * cos + partner * (sgn * sin): sgn = -1 for the x chunk, +1 for the y chunk
                it.a[e] = pack2_rn<Tag>(unpack_lo<Tag>(xs[e]) * clo + unpack_lo<Tag>(ys[e]) * (-1.f * slo),
                                        unpack_hi<Tag>(xs[e]) * chi + unpack_hi<Tag>(ys[e]) * (-1.f * shi));
                it.b[e] = pack2_rn<Tag>(unpack_lo<Tag>(ys[e]) * clo + unpack_lo<Tag>(xs[e]) * (1.f * slo),
                                        unpack_hi<Tag>(ys[e]) * chi + unpack_hi<Tag>(xs[e]) * (1.f * shi));
            }
        }
    }
    return it;
}

template <typename Tag> __device__ __forceinline__ float q8_chunk_amax(chunk_t v, float m) {
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(unpack_lo<Tag>(v[e])), fabsf(unpack_hi<Tag>(v[e]))));
    return m;
}
template <typename Tag> __device__ __forceinline__ float q8_item_amax(const Q8Item& it, float m) {
    m = q8_chunk_amax<Tag>(it.a, m);
    return it.two ? q8_chunk_amax<Tag>(it.b, m) : m;
}

// 8 values of x's dtype -> 8 e4m3 bytes (the append quantiser's arithmetic, restated)
template <typename Tag> __device__ __forceinline__ u32x2 q8_codes(chunk_t x, float inv) {
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
template <typename Tag> __device__ __forceinline__ void q8_store(const Q8Params& p, const Q8Item& it, float inv) {
    *reinterpret_cast<u32x2*>(p.out + it.o) = q8_codes<Tag>(it.a, inv);
    if (it.two) *reinterpret_cast<u32x2*>(p.out + it.o + (p.rdim >> 1)) = q8_codes<Tag>(it.b, inv);
}

__device__ __forceinline__ float q8_descale(float amax, int pow2) {
    float scale = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
    if (pow2) {   // the next power of two, in the bit pattern
        uint32_t bits = __float_as_uint(scale);
        if (bits & 0x007fffffu) bits = (bits & 0x7f800000u) + 0x00800000u;
        scale = __uint_as_float(bits);
    }
    return scale;
}

// the workgroup's maximum, in every thread
__device__ __forceinline__ float q8_block_max(float m, float* red) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <typename Tag, int MODE>
__global__ __launch_bounds__(kThreads) void fp8q_kernel(Q8Params p) {
    __shared__ float red[kThreads / 64];
    const unsigned unit = MODE == kFused ? blockIdx.x : blockIdx.x / (unsigned)p.nchunk;
    const unsigned chunk = MODE == kFused ? 0u : blockIdx.x - unit * (unsigned)p.nchunk;
    const Q8Unit s = q8_unit(p, unit);
    const unsigned t0 = chunk * kThreads + threadIdx.x, step = (unsigned)p.nchunk * kThreads;
    if constexpr (MODE == kFused) {
        Q8Item held[kHeld];
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < kHeld; ++k) {
            const unsigned t = threadIdx.x + k * kThreads;
            if (t < s.items) {
                held[k] = q8_load<Tag>(p, s, t);
                m = q8_item_amax<Tag>(held[k], m);
            }
        }
        const float scale = q8_descale(q8_block_max(m, red), p.pow2);
        const float inv = __fdiv_rn(1.f, scale);
        if (threadIdx.x == 0) p.ds_out[unit] = scale;
#pragma unroll
        for (int k = 0; k < kHeld; ++k)
            if (threadIdx.x + k * kThreads < s.items) q8_store<Tag>(p, held[k], inv);
    } else if constexpr (MODE == kAmax) {
        float m = 0.f;
        for (unsigned t = t0; t < s.items; t += step) m = q8_item_amax<Tag>(q8_load<Tag>(p, s, t), m);
        m = q8_block_max(m, red);
        if (threadIdx.x == 0 && m > 0.f) atomicMax(p.amax + unit, __float_as_uint(m));
    } else {
        float scale;
        if (p.ds) {
            const unsigned b = unit / (unsigned)p.nj;
            scale = p.ds[(long long)b * p.ds_bs + (unit - b * (unsigned)p.nj)];
        } else {
            scale = q8_descale(__uint_as_float(p.amax[unit]), p.pow2);
        }
        const float inv = __fdiv_rn(1.f, scale);
        if (chunk == 0 && threadIdx.x == 0 && p.ds_out) p.ds_out[unit] = scale;
        for (unsigned t = t0; t < s.items; t += step) q8_store<Tag>(p, q8_load<Tag>(p, s, t), inv);
    }
}

// The scratch is zeroed by a kernel of the call's own, in stream order ahead of the maxima.  (A 16-byte hipMemsetAsync node left
// the low word of every 8 bytes holding other bits when a captured call was replayed; a kernel node has no such form.)
__global__ __launch_bounds__(kThreads) void fp8q_zero_kernel(unsigned* amax, unsigned units) {
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    if (i < units) amax[i] = 0u;
}

int q8_items_per_row(const Fp8QuantArgs& a) {
    const int64_t rdim = a.rotary_cos ? a.rotary_dim : 0;
    return (int)((a.rotary_interleaved ? rdim / 8 : rdim / 16) + (a.d - rdim) / 8);
}

template <int MODE> hipError_t q8_launch(const Q8Params& p, int dtype, unsigned blocks, hipStream_t st) {
    if (dtype == 2)
        hipLaunchKernelGGL((fp8q_kernel<bf16_tag, MODE>), dim3(blocks), dim3(kThreads), 0, st, p);
    else
        hipLaunchKernelGGL((fp8q_kernel<f16_tag, MODE>), dim3(blocks), dim3(kThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace

int64_t fp8_quant_unit_items(const Fp8QuantArgs& a) {
    return (a.cu_seqlens ? a.max_seqlen : a.seqlen) * a.heads_per_scale * q8_items_per_row(a);
}

size_t fp8_quant_workspace_bytes(int64_t batch, int64_t heads, int64_t heads_per_scale) {
    return ((size_t)(batch * (heads / heads_per_scale)) * 4 + 255) & ~(size_t)255;
}

hipError_t launch_fp8_quantize(const Fp8QuantArgs& a, hipStream_t st) {
    Q8Params p;
    p.x = (const uint16_t*)a.x; p.out = (uint8_t*)a.out; p.ds = a.descale; p.ds_out = a.descale_out; p.amax = (unsigned*)a.workspace;
    const bool rot = a.rotary_cos != nullptr;
    p.cos = (const uint16_t*)a.rotary_cos; p.sin = (const uint16_t*)a.rotary_sin;
    p.offs = rot ? a.seqlen_offsets : nullptr; p.cu = a.cu_seqlens;
    p.x_bs = a.x_bs; p.x_hs = a.x_hs; p.x_ts = a.x_ts; p.o_bs = a.o_bs; p.o_hs = a.o_hs; p.o_ts = a.o_ts; p.ds_bs = a.descale_bs;
    p.cos_rs = a.rotary_cos_rs; p.sin_rs = a.rotary_sin_rs; p.ro_len = rot ? a.seqlen_ro : 0; p.off0 = rot ? a.seqlen_offset : 0;
    p.S = (int)(a.cu_seqlens ? a.max_seqlen : a.seqlen); p.total = (int)a.total;
    p.g = (int)a.heads_per_scale; p.nj = (int)(a.heads / a.heads_per_scale); p.d = (int)a.d;
    p.rdim = rot ? (int)a.rotary_dim : 0; p.inter = a.rotary_interleaved ? 1 : 0; p.pow2 = a.scale_pow2 ? 1 : 0;
    p.nrot = p.inter ? p.rdim / 8 : p.rdim / 16;
    p.units = q8_items_per_row(a);
    const int64_t units = a.batch * p.nj, items = fp8_quant_unit_items(a);
    const int64_t want = std::max<int64_t>(1, (items + kThreads - 1) / kThreads), room = std::max<int64_t>(1, 2048 / units);
    p.nchunk = (int)std::min(want, room);
    if (a.descale) {
        route_hit(ROUTE_FP8Q_STATIC);
        ProfScope ps(K_FP8Q_QUANT, st);
        return q8_launch<kQuant>(p, a.dtype, (unsigned)(units * p.nchunk), st);
    }
    if (!fp8_quant_two_pass(a)) {
        route_hit(ROUTE_FP8Q_FUSED);
        p.nchunk = 1;
        ProfScope ps(K_FP8Q_FUSED, st);
        return q8_launch<kFused>(p, a.dtype, (unsigned)units, st);
    }
    route_hit(ROUTE_FP8Q_TWO_PASS);
    hipError_t e;
    {
        ProfScope ps(K_FP8Q_AMAX, st);
        hipLaunchKernelGGL(fp8q_zero_kernel, dim3((unsigned)((units + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, p.amax, (unsigned)units);
        e = hipGetLastError();
        if (e == hipSuccess) e = q8_launch<kAmax>(p, a.dtype, (unsigned)(units * p.nchunk), st);
    }
    if (e != hipSuccess) return e;
    ProfScope ps(K_FP8Q_QUANT, st);
    return q8_launch<kQuant>(p, a.dtype, (unsigned)(units * p.nchunk), st);
}

}  // namespace fa
