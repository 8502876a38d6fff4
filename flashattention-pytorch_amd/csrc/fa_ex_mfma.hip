// Extended attention on the 16-bit MFMA (bf16 / f16 tensors, head_dim a multiple of 8 up to 128): the notebook model's
// extras (fa_ex.hip has the list and the reference lines) on the decomposition of the plain kernels —
//   forward   (fa_fwd_mfma.hip)      : 8 waves x 32 query rows, K/V tiles of 128 keys by LDS-DMA, S^T = K Q^T with the query on
//                                      the lane, online softmax in registers, O^T += V^T P^T;
//   dK/dV     (fa_bwd_dkdv_mfma.hip) : 8 waves x 32 keys, Q/dO tiles of 64 rows, the key on the lane;
//   dQ        (fa_bwd_dq_mfma.hip)   : 8 waves x 32 query rows, K/V tiles of 64 keys, the query on the lane;
// with Nq != Nk (separate row counts, causal diagonal shifted by Nk - Nq), and per element
//   FEAT bit 0  dense mask and / or block-sparse mask (either pointer may be null at run time),
//   FEAT bit 1  dropout (counter-based, fa_ex_common.h: a lane makes one splitmix64 value per two of its elements),
//   FEAT bit 2  sliding window: row i sees keys [i + coff - wl, i + coff + wr].  The workgroup walks only the tiles of its
//               band; a wave computes the tiles of its own 32 rows (keys) and only helps to load the others, before
//               and after its own (feed-only); edge tiles mask per element against a lower and an upper threshold.
//               Without the bit the instantiations are the ones of the causal / unmasked kernels, unchanged.
//   FEAT bit 3  packed (varlen) sequences: the padded call's grid, each workgroup narrowed to its sequence (exm_varlen_unit; the
//               fields in ExParams, fa_ex_common.h), token strides for q, k, v; combinable with bits 1 and 2, never with bit 0.
//   FEAT bit 4  score modifiers (softcap, ALiBi slopes): the parameter block grows by ExScore (ExParamsS), and the raw scores are
//               modified right after the S MFMAs, before any mask (mod_softcap / mod_alibi; on / off are wave-uniform run-time
//               switches).  The backward kernels then start S at 0 and add -lse / scale after the modifier, and dS takes the
//               softcap's 1 - t^2 in fp32 before its 16-bit pack.  Combinable with every other bit.
//   FEAT bit 5  attention sinks (forward only, always with bit 4): the parameter block grows once more (ExParamsK) and the
//               epilogue's normaliser takes the unit's sink logit as one more column (ex_sink_norm).  The key loop is bit 4's.
//               The backward of a sink call runs the kernels of the call without sinks and ex_dsink_kernel (fa_ex.hip).
//   FEAT bit 6  paged K/V (forward only, always with bit 3, never with bits 0 and 1): k and v are pools of pages and a sequence's
//               keys are found through a block table (ExPage: the parameter block grows by it, ExParamsPg).  Only the staging of
//               a K/V tile differs (dma_stage_kv_paged): each 1-KiB piece takes its page from one scalar table load and gets a
//               buffer descriptor of its own; everything after the staging is the text of the packed kernel, so a sequence gets
//               the bits of the packed call on the same tokens.
//   FEAT bit 7  an e4m3 pool (always with bits 3 and 6): instantiated by fa_ex_mfma_kv8.hip, a translation unit of its own.
//   FEAT bit 8  an additive bias (always with bit 4 and with no other): instantiated by fa_ex_mfma_bias.hip, a translation unit of
//               its own, whose header has the loaders and where dS is stored.
// One kernel template per pass (fa_ex_mfma_kernels.h: the bodies and their device helpers; the parameter block is a function of
// FEAT), one forward and one backward launcher, one function from a call to its FEAT and one list of the FEAT values a call family
// may instantiate (fa_ex_mfma_feat.h).  This file holds the row-constant pre-pass, the support checks and the launches.
// Dense mask bytes are fetched with range-checked buffer loads (rows / bytes past the mask read as 0 = masked); when Nk, the
// mask pointer and the (b,h) stride are multiples of 4 a lane of the query-on-the-lane kernels takes the 4 keys of a
// register group with one dword load.  The block-sparse mask needs br, bc multiples of 32 here (a wave's 32 x 32 block
// then has ONE entry; other block shapes take the exact-f32 kernels): tiles without a live entry are skipped before
// they are loaded, live tiles mask their dead 32 x 32 blocks.  A row without a visible key: o = 0, lse = -inf, dQ = 0.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_ex_mfma_feat.h"
#include "fa_ex_mfma_kernels.h"
#include "fa_kernels.h"

namespace fa {

// ------------------------------------------------------------------------------------------------ row constants
// nlse = -lse / scale (0 for a row without a visible key: every element of such a row is masked by a select, and an
// infinite initial accumulator would only make NaNs on the way), ndelta = -rowsum(dO * O).  16 lanes per row.
// dlse != null (fa_ex_backward_dlse): ndelta = dlse - rowsum(dO * O), the gradient of the row's lse, which is all a gradient of lse
// does to the backward (dS = P (dP + ndelta)); a row whose lse is -inf ignores its dlse.
template <typename Tag>
__global__ __launch_bounds__(256) void exm_prep_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ dout,
                                                       const float* __restrict__ lse, float* __restrict__ nlse,
                                                       float* __restrict__ ndelta, long long rows, int d, float inv_scale,
                                                       const float* __restrict__ dlse) {
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    float s = 0.f;
    if (row < rows && 8 * sub < d) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(o + row * d + 8 * sub);
        const u32x4 b = *reinterpret_cast<const u32x4*>(dout + row * d + 8 * sub);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += unpack_lo<Tag>(a[j]) * unpack_lo<Tag>(b[j]) + unpack_hi<Tag>(a[j]) * unpack_hi<Tag>(b[j]);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (row < rows && sub == 0) {
        const float l = lse[row];
        nlse[row] = (l == -INFINITY) ? 0.f : -l * inv_scale;
        ndelta[row] = (dlse && l != -INFINITY) ? dlse[row] - s : -s;
    }
}

// the same for packed sequences: o, dout (total_q, hq, d); lse and the two outputs (hq, total_q).  Workgroup x: head x / tph,
// tokens 16 (x % tph) ..  Tokens no sequence covers get constants of their unspecified lse (no kernel reads them).
template <typename Tag>
__global__ __launch_bounds__(256) void exm_prep_varlen_kernel(const uint16_t* __restrict__ o, const uint16_t* __restrict__ dout,
                                                              const float* __restrict__ lse, float* __restrict__ nlse,
                                                              float* __restrict__ ndelta, int total_q, int tph, int hq, int d,
                                                              float inv_scale, const float* __restrict__ dlse) {
    const int hd = blockIdx.x / tph;
    const int tok = (blockIdx.x - hd * tph) * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    const size_t row = ((size_t)tok * hq + hd) * d;
    float s = 0.f;
    if (tok < total_q && 8 * sub < d) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(o + row + 8 * sub);
        const u32x4 b = *reinterpret_cast<const u32x4*>(dout + row + 8 * sub);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += unpack_lo<Tag>(a[j]) * unpack_lo<Tag>(b[j]) + unpack_hi<Tag>(a[j]) * unpack_hi<Tag>(b[j]);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (tok < total_q && sub == 0) {
        const size_t i = (size_t)hd * total_q + tok;
        const float l = lse[i];
        nlse[i] = (l == -INFINITY) ? 0.f : -l * inv_scale;
        ndelta[i] = (dlse && l != -INFINITY) ? dlse[i] - s : -s;
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool ex_mfma_supported(const ExArgs& a) {
    if (a.dtype != 1 && a.dtype != 2) return false;
    if (a.d < 8 || a.d > 128 || a.d % 8 != 0) return false;
    if (!(a.scale > 0.f)) return false;                       // the running max is taken on the raw scores
    if (a.block_mask && (a.br % 32 != 0 || a.bc % 32 != 0)) return false;
    if (a.mask && a.nq * a.nk >= ((int64_t)1 << 31)) return false;   // 32-bit byte offsets into one (b,h)'s mask
    if (a.bh * ((a.nq + 1) / 2) >= ((int64_t)1 << 32)) return false;  // the generator's row-pair counter
    return true;
}

// The row-constant pre-pass, the only place that launches exm_prep_kernel / exm_prep_varlen_kernel (for this unit's backward and
// for fa_ex_mfma_vdim.hip's): d_row is the row width of o and dout, the packed form goes by a.cu_q.
hipError_t launch_exm_prep(const ExArgs& a, int64_t d_row, float* nlse, float* ndelta, hipStream_t st) {
    const bool bf = a.dtype == 2;
    if (a.cu_q) {
        const int tph = (int)((a.total_q + 15) / 16);
        auto kern = bf ? exm_prep_varlen_kernel<bf16_tag> : exm_prep_varlen_kernel<f16_tag>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(tph * a.heads_q)), dim3(256), 0, st, (const uint16_t*)a.o, (const uint16_t*)a.dout,
                           (const float*)a.lse, nlse, ndelta, (int)a.total_q, tph, (int)a.heads_q, (int)d_row, 1.f / a.scale, a.dlse);
    } else {
        const long long rows = (long long)a.bh * a.nq;
        auto kern = bf ? exm_prep_kernel<bf16_tag> : exm_prep_kernel<f16_tag>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, (const uint16_t*)a.o, (const uint16_t*)a.dout,
                           (const float*)a.lse, nlse, ndelta, rows, (int)d_row, 1.f / a.scale, a.dlse);
    }
    return hipGetLastError();
}

// one call of a family: its FEAT (exm_feat, fa_ex_mfma_feat.h), then the instantiation of the family's list that has it
template <typename Feats>
static hipError_t exm_launch(ExmFamily fam, const ExArgs& a, bool backward, hipStream_t st) {
    return exm_dispatch<Feats>(a, exm_feat_of(fam, a, backward), [&](auto tag, auto d, auto feat) -> hipError_t {
        using Tag = decltype(tag);
        constexpr int D = decltype(d)::value, FEAT = decltype(feat)::value;
        if (!backward) return exm_fwd_t<Tag, D, FEAT>(a, st);
        if constexpr ((FEAT & (kFeatSink | kFeatPaged)) != 0) return hipErrorInvalidValue;   // forward-only instantiations
        else return exm_bwd_t<Tag, D, FEAT>(a, st);
    });
}
hipError_t launch_ex_mfma(const ExArgs& a, bool backward, hipStream_t st) { return exm_launch<ExmDenseFeats>(kExmDense, a, backward, st); }

// ---- packed sequences: the varlen kernels on the padded grid (a.bh = batch * heads_q units, a.nq / a.nk = the maxima)
bool ex_mfma_varlen_supported(const ExArgs& a) {
    if (!ex_mfma_supported(a)) return false;
    if (a.stride_q % 8 != 0 || a.stride_k % 8 != 0 || a.stride_v % 8 != 0) return false;   // 16-byte rows
    const void* ptrs[] = {a.q, a.k, a.v, a.o, a.dout, a.dq, a.dk, a.dv};
    for (const void* ptr : ptrs)
        if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) return false;
    int64_t smax = a.heads_q * a.d;   // o, dout, dq rows
    if (a.stride_q > smax) smax = a.stride_q;
    if (a.stride_k > smax) smax = a.stride_k;
    if (a.stride_v > smax) smax = a.stride_v;
    const int64_t nmax = a.nq > a.nk ? a.nq : a.nk;
    return nmax * smax * 2 < ((int64_t)1 << 31);   // the 32-bit buffer offsets inside one sequence
}

// (the caller has checked ex_mfma_varlen_supported, and that max_seqlen_q, max_seqlen_k, total_q, total_k are > 0)
hipError_t launch_ex_mfma_varlen(const ExArgs& a, bool backward, hipStream_t st) { return exm_launch<ExmVarlenFeats>(kExmVarlen, a, backward, st); }

// ---- paged K/V (a.block_table != null): the varlen forward with kFeatPaged, {window} x {plain, score, score + sink}
bool ex_mfma_paged_supported(const ExArgs& a) {
    if (!ex_mfma_supported(a) || a.dropout_p > 0.0) return false;
    if (a.stride_q % 8 != 0 || a.stride_k % 8 != 0 || a.stride_v % 8 != 0 || a.page_stride_k % 8 != 0 || a.page_stride_v % 8 != 0) return false;
    const void* ptrs[] = {a.q, a.k, a.v, a.o};
    for (const void* ptr : ptrs)
        if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) return false;
    const int64_t sq = a.stride_q > a.heads_q * a.d ? a.stride_q : a.heads_q * a.d;
    const int64_t skv = a.stride_k > a.stride_v ? a.stride_k : a.stride_v;
    // the 32-bit buffer offsets: inside one sequence of q and o, inside one piece (at most 8 rows) of a page
    return a.nq * sq * 2 < ((int64_t)1 << 31) && 8 * skv * 2 < ((int64_t)1 << 31);
}

// (the caller has checked ex_mfma_paged_supported, and that max_seqlen_q and the key cap are > 0)
hipError_t launch_ex_mfma_varlen_paged(const ExArgs& a, hipStream_t st) { return exm_launch<ExmPagedFeats>(kExmPaged, a, false, st); }

}  // namespace fa
