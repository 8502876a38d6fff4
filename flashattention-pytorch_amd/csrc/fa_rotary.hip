// Rotary position embedding for training and prefill (fa_rotary_apply; include/fa_mi355x.h): one memory-bound launch rotates the
// first rotary_dim head dims of every head of one 16-bit tensor x (batch, seqlen, heads, d) into y, forward or conjugate (the
// transpose of the forward map, which is the whole backward), in place (y == x) or out of place, padded or packed (cu_seqlens).
// Tables, pairings and arithmetic are those of the decode call (fa_decode.hip: KvRot, kv_rotate_chunk), restated here so that the
// decode translation unit keeps its text: fp32 from the 16-bit inputs, own * cos + partner * (sgn * sin), one rounding to nearest
// even.  Both products are exact in fp32 (8 x 8 or 11 x 11 significant bits), so the sum rounds once whether or not the compiler
// contracts it into an FMA, and this kernel gives the bits the decode append stores.
//   unit           : what one thread moves per step.  Interleaved (pairs (2 j, 2 j + 1)): one 16-byte chunk, head dims 8 u .. 8 u + 7,
//                    four pairs and four table entries, self-contained.  Not interleaved (pairs (j, j + half), half =
//                    rotary_dim / 2, a multiple of 8): the chunk at 8 u < half AND its partner chunk at 8 u + half.  The thread
//                    loads both, rotates both and stores both, so every element is read once, by the thread that writes it,
//                    before that write: no other thread touches the pair, which is what makes y == x safe (the decode append
//                    reads the partner chunk from another thread's chunk; it is out of place).  tests/test_rotary_cpu.py models
//                    this map.
//   pass-through   : head dims at and past rotary_dim.  Out of place they are further one-chunk units that copy; in place they
//                    are no units at all (neither read nor written).
//   position       : token i of sequence b is at pos = seqlen_offset + (seqlen_offsets ? seqlen_offsets[b] : 0) + i, formed in 64
//                    bits from untrusted device memory.  Rotated iff 0 <= pos < seqlen_ro; any other token passes through (copied
//                    out of place, untouched in place), so no table row outside the table is ever addressed.
//   packed         : sequence b owns the tokens seq_span gives it (the clamp of the varlen forward), positions count from its
//                    own first token, the grid is that of the padded (batch, max_seqlen) call and threads past the sequence's end
//                    leave.  Tokens no sequence owns are not visited.
// Grid: (x, batch) with about 2048 blocks of 256 threads in all and a grid-stride loop over a sequence's units; 64-bit element
// offsets throughout.  Nothing is read on the host.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"
#include <algorithm>

namespace fa {

namespace {

struct RoParams {
    const uint16_t* x;
    uint16_t* y;
    const uint16_t *cos, *sin;     // (ro_len, rdim / 2), rows at the even strides cos_rs / sin_rs, 4-byte aligned
    const int *offs, *cu;          // seqlen_offsets (batch,), cu_seqlens (batch + 1,): untrusted device memory, or null
    long long x_bs, x_ts, y_bs, y_ts, cos_rs, sin_rs, ro_len, off0;
    int S, total;                  // tokens a sequence has at most (seqlen, or max_seqlen); tokens of a packed tensor
    int heads, d, rdim, inter, conj, inplace;
    int nrot, units;               // rotating units per head row, all units per head row (nrot + the copying ones)
};

typedef u32x4 chunk_t;

__device__ __forceinline__ chunk_t ro_load(const uint16_t* p) { return *reinterpret_cast<const chunk_t*>(p); }
__device__ __forceinline__ void ro_store(uint16_t* p, chunk_t v) { *reinterpret_cast<chunk_t*>(p) = v; }

template <typename Tag>
__global__ __launch_bounds__(256) void rotary_kernel(RoParams p) {
    const int b = blockIdx.y;
    int start = 0, len = p.S;
    if (p.cu) seq_span(p.cu, b, p.total, p.S, start, len);
    const long long per_b = (long long)len * p.heads * p.units;
    const long long xb = p.cu ? (long long)start * p.x_ts : b * p.x_bs;
    const long long yb = p.cu ? (long long)start * p.y_ts : b * p.y_bs;
    const long long pos0 = p.off0 + (p.offs ? (long long)p.offs[b] : 0LL);
    const int half = p.rdim >> 1;
    const float sg = p.conj ? -1.f : 1.f;                        // the conjugate rotates by -sin: an exact sign flip
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < per_b; t += (long long)gridDim.x * blockDim.x) {
        const int u = (int)(t % p.units);
        const long long r = t / p.units;
        const int h = (int)(r % p.heads);
        const long long i = r / p.heads;                         // the sequence's token
        const uint16_t* xr = p.x + xb + i * p.x_ts + (long long)h * p.d;
        uint16_t* yr = p.y + yb + i * p.y_ts + (long long)h * p.d;
        if (u >= p.nrot) {                                       // a pass-through chunk (out of place only)
            const int col = p.rdim + 8 * (u - p.nrot);
            ro_store(yr + col, ro_load(xr + col));
            continue;
        }
        const long long pos = pos0 + i;
        const bool rot = pos >= 0 && pos < p.ro_len;
        if (!rot && p.inplace) continue;
        const int col = 8 * u;
        if (p.inter) {
            const chunk_t own = ro_load(xr + col);
            chunk_t out = own;
            if (rot) {
                const uint32_t* cp = reinterpret_cast<const uint32_t*>(p.cos + pos * p.cos_rs + (col >> 1));
                const uint32_t* sp = reinterpret_cast<const uint32_t*>(p.sin + pos * p.sin_rs + (col >> 1));
                const uint32_t c2[2] = {cp[0], cp[1]}, s2[2] = {sp[0], sp[1]};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xv = unpack_lo<Tag>(own[e]), yv = unpack_hi<Tag>(own[e]);
                    const float c = (e & 1) ? unpack_hi<Tag>(c2[e >> 1]) : unpack_lo<Tag>(c2[e >> 1]);
                    const float sn = sg * ((e & 1) ? unpack_hi<Tag>(s2[e >> 1]) : unpack_lo<Tag>(s2[e >> 1]));
                    out[e] = pack2_rn<Tag>(xv * c - yv * sn, xv * sn + yv * c);
                }
            }
            ro_store(yr + col, out);
        } else {
            const chunk_t xs = ro_load(xr + col), ys = ro_load(xr + col + half);   // both halves of pairs j = col .. col + 7
            chunk_t ox = xs, oy = ys;
            if (rot) {
                const uint32_t* cp = reinterpret_cast<const uint32_t*>(p.cos + pos * p.cos_rs + col);
                const uint32_t* sp = reinterpret_cast<const uint32_t*>(p.sin + pos * p.sin_rs + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t c2 = cp[e], s2 = sp[e];
                    const float clo = unpack_lo<Tag>(c2), chi = unpack_hi<Tag>(c2);
                    const float slo = sg * unpack_lo<Tag>(s2), shi = sg * unpack_hi<Tag>(s2);
                    // own * cos + partner * (sgn * sin): sgn = -1 for the x chunk, +1 for the y chunk
                    ox[e] = pack2_rn<Tag>(unpack_lo<Tag>(xs[e]) * clo + unpack_lo<Tag>(ys[e]) * (-1.f * slo),
                                          unpack_hi<Tag>(xs[e]) * chi + unpack_hi<Tag>(ys[e]) * (-1.f * shi));
                    oy[e] = pack2_rn<Tag>(unpack_lo<Tag>(ys[e]) * clo + unpack_lo<Tag>(xs[e]) * (1.f * slo),
                                          unpack_hi<Tag>(ys[e]) * chi + unpack_hi<Tag>(xs[e]) * (1.f * shi));
                }
            }
            ro_store(yr + col, ox);
            ro_store(yr + col + half, oy);
        }
    }
}

}  // namespace

hipError_t launch_rotary(const RotaryArgs& a, hipStream_t st) {
    RoParams p;
    p.x = (const uint16_t*)a.x; p.y = (uint16_t*)a.y;
    p.cos = (const uint16_t*)a.rotary_cos; p.sin = (const uint16_t*)a.rotary_sin;
    p.offs = a.seqlen_offsets; p.cu = a.cu_seqlens;
    p.x_bs = a.x_bs; p.x_ts = a.x_ts; p.y_bs = a.y_bs; p.y_ts = a.y_ts;
    p.cos_rs = a.rotary_cos_rs; p.sin_rs = a.rotary_sin_rs; p.ro_len = a.seqlen_ro; p.off0 = a.seqlen_offset;
    p.S = (int)(a.cu_seqlens ? a.max_seqlen : a.seqlen); p.total = (int)a.total;
    p.heads = (int)a.heads; p.d = (int)a.d; p.rdim = (int)a.rotary_dim;
    p.inter = a.rotary_interleaved ? 1 : 0; p.conj = a.conjugate ? 1 : 0;
    p.inplace = a.x == a.y ? 1 : 0;
    p.nrot = p.inter ? p.rdim / 8 : p.rdim / 16;
    p.units = p.nrot + (p.inplace ? 0 : (p.d - p.rdim) / 8);
    const long long per_b = (long long)p.S * p.heads * p.units;
    if (per_b <= 0) return hipSuccess;
    const long long want = (per_b + 255) / 256, room = std::max<long long>(1, 2048 / a.batch);
    const dim3 grid((unsigned)std::min(want, room), (unsigned)a.batch);
    if (a.dtype == 2)
        hipLaunchKernelGGL(rotary_kernel<bf16_tag>, grid, dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(rotary_kernel<f16_tag>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace fa
