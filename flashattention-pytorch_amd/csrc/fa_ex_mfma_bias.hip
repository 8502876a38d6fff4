// An additive bias on the scores (fa_ex_forward_bias / fa_ex_backward_bias): FEAT bit 8, kFeatBias, always with bit 4 (the
// score-modifier body, where the bias joins as ALiBi does) and with no other bit.  For query unit u = b * heads + h, row i, key j:
//   s[i, j] = scale q_i . k_j + bias[b, h, i, j]        (bias in q's dtype, widened exactly, added in fp32, not scaled; -inf = masked)
// and the softmax, o and lse are those of s.  The kernels are the kFeatBias instantiations of exm_fwd_kernel, exm_dkdv_kernel and
// exm_dq_kernel (fa_ex_mfma_kernels.h); the parameter block grows by ExBias (ExParamsB).  What the bit changes in them:
//   forward, dQ   (the query on the lane) a lane holds 4 groups of 4 consecutive keys of its row per 32 x 32 block: four 8-byte
//                 range-checked buffer loads (bias_load_q), issued in front of the next tile's LDS-DMA (VMEM returns in order);
//   dK/dV         (the key on the lane) a lane needs 16 rows of one key column: the block's 2 KiB go through an LDS image of the
//                 wave's own, two 16-byte loads per lane (bias_load_k / bias_add_k), 8 x 2 KiB behind the row constants;
//   dS out        dbias[b, h, i, j] = dS[i, j] = P (dP - delta + dlse_i), the 16-bit words the dQ kernel packs for its own MFMA,
//                 stored from there 8 bytes per register group (bias_ds_store); the same kernel writes the zeros of the tiles it
//                 skips under the causal diagonal, so every element [:nq, :nk] is written and nothing past column nk is.
// A key >= nk may read padding of the bias row, NaN included: every kernel turns it invisible with a select after the sum.
// A dbias that is broadcast over the batch or the heads is the sum of the per-unit dS: the kernels then write (bh, nq, nk padded to 8)
// 16-bit dS into the workspace and exm_dbias_sum_kernel adds them in fp32 in unit order and rounds once — the same bits on every run.
// A translation unit of its own for the reason fa_ex_mfma_kv8.hip gives: the kernels of fa_ex_mfma.hip stay the instructions they were.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_ex_mfma_feat.h"
#include "fa_ex_mfma_kernels.h"
#include "fa_kernels.h"

namespace fa {

// ------------------------------------------------------------------------------------------------ the broadcast sum
// ws: (B, H, nq, nkp) 16-bit per-unit dS, nkp = nk rounded up to 8 (the columns nk .. nkp - 1 are never written and never stored
// from).  out[bo, ho, i, j] = round(sum over the units (b, h) that broadcast onto (bo, ho), b outer and h inner = unit order, in
// fp32).  A thread owns 8 keys of one output row: one 16-byte load per unit, one 16-byte store (the row's last chunk: key by key).
template <typename Tag>
__global__ __launch_bounds__(256) void exm_dbias_sum_kernel(const uint16_t* __restrict__ ws, uint16_t* __restrict__ out, int B, int H,
                                                            int nq, int nk, int nkp, int red_b, int red_h, long long o_bs,
                                                            long long o_hs, long long o_rs, long long nchunk) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunk) return;
    const int cpr = nkp / 8;
    const long long rowi = i / cpr;
    const int c = (int)(i - rowi * cpr);
    const long long uo = rowi / nq;
    const int r = (int)(rowi - uo * nq);
    const int Ho = red_h ? 1 : H;
    const int bo = (int)(uo / Ho), ho = (int)(uo - (long long)bo * Ho);
    const int b0 = red_b ? 0 : bo, b1 = red_b ? B : bo + 1;
    const int h0 = red_h ? 0 : ho, h1 = red_h ? H : ho + 1;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int b = b0; b < b1; ++b)
        for (int h = h0; h < h1; ++h) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(ws + (((size_t)b * H + h) * nq + r) * nkp + 8 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[2 * j] += unpack_lo<Tag>(x[j]);
                acc[2 * j + 1] += unpack_hi<Tag>(x[j]);
            }
        }
    u32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = pack2_rn<Tag>(acc[2 * j], acc[2 * j + 1]);
    uint16_t* dst = out + bo * o_bs + ho * o_hs + r * o_rs + 8 * c;
    if (8 * c + 8 <= nk) {
        *reinterpret_cast<u32x4*>(dst) = y;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (8 * c + j < nk) dst[j] = (uint16_t)(y[j >> 1] >> (16 * (j & 1)));
    }
}

// ------------------------------------------------------------------------------------------------ launch
// What the C layer checked of the bias and of dbias (16-byte aligned, the last dim contiguous, every stride a multiple of 8) will do
// for the 8- and 16-byte accesses; here once more, with the 32-bit offsets inside one unit (rows up to the last tile's end).
bool ex_mfma_bias_supported(const ExArgs& a) {
    if (!a.bias || !ex_mfma_supported(a) || a.d_v != 0 || a.cu_q) return false;
    if (a.mask || a.block_mask || a.dropout_p > 0.0 || ex_windowed(a) || ex_scoremod(a) || a.sinks) return false;
    if (a.bias_heads < 1 || a.bh % a.bias_heads != 0) return false;
    const int64_t strides[] = {a.bias_bstride, a.bias_hstride, a.bias_rstride, a.dbias_bstride, a.dbias_hstride, a.dbias_rstride};
    for (const int64_t s : strides)
        if (s < 0 || s % 8 != 0) return false;
    if (((reinterpret_cast<uintptr_t>(a.bias) | reinterpret_cast<uintptr_t>(a.dbias)) & 15) != 0) return false;
    const int64_t nkp = (a.nk + 7) & ~(int64_t)7;
    const int64_t rmax = a.bias_rstride > a.dbias_rstride ? a.bias_rstride : a.dbias_rstride;
    return ((a.nq + 256) * rmax + nkp + 256) * 2 < ((int64_t)1 << 31);
}

// (the caller has checked ex_mfma_bias_supported, and that nq, nk > 0)
hipError_t launch_ex_mfma_bias(const ExArgs& a, bool backward, hipStream_t st) {
    ExArgs g = a;
    const int64_t nkp = (a.nk + 7) & ~(int64_t)7, B = a.bh / a.bias_heads, H = a.bias_heads;
    if (!backward) g.dbias = nullptr;
    const bool red = g.dbias && ex_bias_reduced(a.bh, a.bias_heads, a.dbias_bstride, a.dbias_hstride);
    if (red) {   // the per-unit dS behind the row constants
        const size_t rows = ex_backward_workspace_bytes(a.bh, a.nq);
        if (a.workspace_bytes < rows + ex_bias_ds_bytes(a.bh, a.nq, a.nk)) return hipErrorInvalidValue;
        g.dbias = reinterpret_cast<char*>(a.workspace) + rows;
        g.dbias_rstride = nkp;
        g.dbias_hstride = a.nq * nkp;
        g.dbias_bstride = H * a.nq * nkp;
    }
    hipError_t e = exm_dispatch<ExmBiasFeats>(g, exm_feat_of(kExmBias, g, backward), [&](auto tag, auto d, auto feat) -> hipError_t {
        using Tag = decltype(tag);
        constexpr int D = decltype(d)::value, FEAT = decltype(feat)::value;
        return backward ? exm_bwd_t<Tag, D, FEAT>(g, st) : exm_fwd_t<Tag, D, FEAT>(g, st);
    });
    if (e != hipSuccess || !red) return e;
    const int red_b = a.dbias_bstride == 0 && B > 1, red_h = a.dbias_hstride == 0 && H > 1;
    const long long nchunk = (long long)(red_b ? 1 : B) * (red_h ? 1 : H) * a.nq * (nkp / 8);
    const long long blocks = (nchunk + 255) / 256;
    if (blocks >= ((long long)1 << 31)) return hipErrorInvalidConfiguration;
    auto kern = a.dtype == 2 ? exm_dbias_sum_kernel<bf16_tag> : exm_dbias_sum_kernel<f16_tag>;
    ProfScope ps(K_EX_BWD, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, st, (const uint16_t*)g.dbias, (uint16_t*)a.dbias, (int)B, (int)H, (int)a.nq,
                       (int)a.nk, (int)nkp, red_b, red_h, (long long)a.dbias_bstride, (long long)a.dbias_hstride, (long long)a.dbias_rstride,
                       nchunk);
    return hipGetLastError();
}

}  // namespace fa
