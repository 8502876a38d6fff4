// Shared by the translation units of the 16-bit MFMA extended kernels (fa_ex_mfma.hip; fa_ex_mfma_kv8.hip: the e4m3 pool): the
// FEAT bits of an instantiation (fa_ex_mfma.hip's header has what each stands for), the parameter block that goes with them, and
// the accumulator register map.  Internal linkage, as when each file had its own.
#pragma once
#include <type_traits>

#include "fa_ex_common.h"
#include "fa_kernels.h"

namespace fa {

namespace {

constexpr int kFeatMask = 1, kFeatDrop = 2, kFeatWindow = 4, kFeatVarlen = 8, kFeatScore = 16, kFeatSink = 32, kFeatPaged = 64, kFeatKv8 = 128;
// the parameter block of an instantiation: ExParamsK (+ the sinks) with kFeatSink, ExParamsS (+ the score modifiers) with
// kFeatScore, else ExParams as before
template <int FEAT> using ExP = typename std::conditional<(FEAT & kFeatSink) != 0, ExParamsK,
                                typename std::conditional<(FEAT & kFeatScore) != 0, ExParamsS, ExParams>::type>::type;
template <int FEAT> inline ExP<FEAT> make_exm_params(const ExArgs& a) {
    if constexpr ((FEAT & kFeatSink) != 0) return make_ex_params_k(a);
    else if constexpr ((FEAT & kFeatScore) != 0) return make_ex_params_s(a);
    else return make_ex_params(a);
}

// rc(i): row (or key) offset inside a 32-wide block of accumulator register i, before the 4 * (lane >> 5) term
__device__ __forceinline__ constexpr int rc_of(int i) { return (i & 3) + 8 * (i >> 2); }

}  // namespace

}  // namespace fa
