// The paged varlen forward of fa_ex_mfma.hip on an e4m3 pool (fa_ex_forward_varlen_paged_fp8): FEAT bit 7, kFeatKv8, always with
// bits 3 (varlen) and 6 (paged), never with bits 0 and 1 (mask, dropout).  k and v address OCP e4m3 bytes, strides are bytes, and
// the parameter block grows by the two scale pointers (ExKv8, ExParamsPg8).  The kernels are the kFeatKv8 instantiations of
// exm_fwd_kernel (fa_ex_mfma_kernels.h says what the bit changes in it); this file holds only their launch.
// A translation unit of its own: hipcc allocates the registers of a kernel differently when other kernels join its module
// (instantiated inside fa_ex_mfma.hip these 24 changed that file's 72 varlen forward kernels, although no line of those changed),
// and the kernels of fa_ex_mfma.hip are to stay the instructions they were.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_ex_mfma_feat.h"
#include "fa_ex_mfma_kernels.h"
#include "fa_kernels.h"

namespace fa {

// ------------------------------------------------------------------------------------------------ launch
// Dword DMA and 8-byte staging reads: what the C layer checked of the pools (8-byte alignment, strides % 8) will do; q and o as in
// ex_mfma_paged_supported
bool ex_mfma_paged_kv8_supported(const ExArgs& a) {
    if (!ex_mfma_supported(a) || a.dropout_p > 0.0) return false;
    if (a.stride_q % 8 != 0 || ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.o)) & 15) != 0) return false;
    if (a.stride_k % 4 != 0 || a.stride_v % 4 != 0 || a.page_stride_k % 4 != 0 || a.page_stride_v % 4 != 0) return false;
    if (((reinterpret_cast<uintptr_t>(a.k) | reinterpret_cast<uintptr_t>(a.v)) & 3) != 0) return false;
    const int64_t sq = a.stride_q > a.heads_q * a.d ? a.stride_q : a.heads_q * a.d;
    const int64_t skv = a.stride_k > a.stride_v ? a.stride_k : a.stride_v;
    // the 32-bit buffer offsets: inside one sequence of q and o, inside one block of 16 rows of a page (bytes)
    return a.nq * sq * 2 < ((int64_t)1 << 31) && 16 * skv < ((int64_t)1 << 31);
}

// (the caller has checked ex_mfma_paged_kv8_supported, and that max_seqlen_q and the key cap are > 0)
hipError_t launch_ex_mfma_varlen_paged_kv8(const ExArgs& a, hipStream_t st) {
    return exm_dispatch<ExmPagedKv8Feats>(a, exm_feat_of(kExmPagedKv8, a, false), [&](auto tag, auto d, auto feat) {
        return exm_fwd_t<decltype(tag), decltype(d)::value, decltype(feat)::value>(a, st);
    });
}

}  // namespace fa
