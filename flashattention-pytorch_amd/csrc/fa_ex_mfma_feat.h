// Shared by the translation units of the 16-bit MFMA extended kernels (fa_ex_mfma.hip; fa_ex_mfma_kv8.hip: the e4m3 pool;
// fa_ex_mfma_bias.hip: the additive bias; and fa_ex_mfma_vdim.hip, which takes the bits, ExP and the register map): the FEAT bits of an instantiation (fa_ex_mfma.hip's header
// has what each stands for), the parameter block that goes with them, the one function from a call to its FEAT with the table
// that pins it, the FEAT values each call family may instantiate, and the accumulator register map.  Internal linkage, as when
// each file had its own.
#pragma once
#include <type_traits>
#include <utility>

#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_kernels.h"

namespace fa {

namespace {

constexpr int kFeatMask = 1, kFeatDrop = 2, kFeatWindow = 4, kFeatVarlen = 8, kFeatScore = 16, kFeatSink = 32, kFeatPaged = 64, kFeatKv8 = 128;
constexpr int kFeatBias = 256;   // an additive bias (fa_ex_mfma_bias.hip): always with kFeatScore, never with another bit
// the parameter block of an instantiation: ExParamsK (+ the sinks) with kFeatSink, ExParamsS (+ the score modifiers) with
// kFeatScore, else ExParams as before
template <int FEAT> using ExP = typename std::conditional<(FEAT & kFeatSink) != 0, ExParamsK,
                                typename std::conditional<(FEAT & kFeatScore) != 0, ExParamsS, ExParams>::type>::type;
template <int FEAT> inline ExP<FEAT> make_exm_params(const ExArgs& a) {
    if constexpr ((FEAT & kFeatSink) != 0) return make_ex_params_k(a);
    else if constexpr ((FEAT & kFeatScore) != 0) return make_ex_params_s(a);
    else return make_ex_params(a);
}
// ... grown by the pages with kFeatPaged (ExParamsPg), and by the scales of an e4m3 pool with kFeatKv8 (ExParamsPg8): what a
// kernel takes.  K and V are addressed as 16-bit words, or as bytes with kFeatKv8.
// ... or by the bias group with kFeatBias (ExParamsB)
template <int FEAT> using ExB = typename std::conditional<(FEAT & kFeatBias) != 0, ExParamsB,
                                typename std::conditional<(FEAT & kFeatKv8) != 0, ExParamsPg8<ExP<FEAT>>,
                                typename std::conditional<(FEAT & kFeatPaged) != 0, ExParamsPg<ExP<FEAT>>, ExP<FEAT>>::type>::type>::type;
template <int FEAT> using ExKV = typename std::conditional<(FEAT & kFeatKv8) != 0, uint8_t, uint16_t>::type;
template <int FEAT> inline ExB<FEAT> make_exm_block(const ExArgs& a) {
    ExB<FEAT> p;
    static_cast<ExP<FEAT>&>(p) = make_exm_params<FEAT>(a);
    if constexpr ((FEAT & kFeatPaged) != 0) p.pg = make_ex_page(a);
    if constexpr ((FEAT & kFeatKv8) != 0) p.q8 = make_ex_kv8(a);
    if constexpr ((FEAT & kFeatBias) != 0) p.bs = make_ex_bias(a);
    return p;
}

// rc(i): row (or key) offset inside a 32-wide block of accumulator register i, before the 4 * (lane >> 5) term
__device__ __forceinline__ constexpr int rc_of(int i) { return (i & 3) + 8 * (i >> 2); }

// ---- from a call to its FEAT.  The four call families (the five launch_ex_mfma* entry points):
enum ExmFamily { kExmDense, kExmVarlen, kExmPaged, kExmPagedKv8, kExmBias };
// masks: a dense or a block-sparse mask; sink_fwd: the forward of a call with sinks (its backward is the call's without them).
//   dense          dropout takes the mask bit with it (the dropout kernels are the masked ones); a mask alone is bit 0
//   varlen         never bit 0 (the C layer hands a packed call no mask); dropout is bit 1 alone
//   paged, e4m3    forward only, neither mask nor dropout (ex_mfma_paged_supported turns dropout away)
//   a sink forward always carries kFeatScore: it runs on the score-modifier body, with or without a modifier
//   bias           kFeatBias | kFeatScore and nothing else: the C layer has refused every other feature by name
constexpr int exm_feat(ExmFamily fam, bool masks, bool drop, bool window, bool score, bool sink_fwd) {
    if (fam == kExmBias) return kFeatBias | kFeatScore;
    int f = fam == kExmDense ? 0 : fam == kExmVarlen ? kFeatVarlen : fam == kExmPaged ? kFeatVarlen | kFeatPaged : kFeatVarlen | kFeatPaged | kFeatKv8;
    if (fam == kExmDense) f |= drop ? kFeatMask | kFeatDrop : masks ? kFeatMask : 0;
    if (fam == kExmVarlen && drop) f |= kFeatDrop;
    if (window) f |= kFeatWindow;
    if (sink_fwd) f |= kFeatScore | kFeatSink;
    else if (score) f |= kFeatScore;
    return f;
}
inline int exm_feat_of(ExmFamily fam, const ExArgs& a, bool backward) {
    return exm_feat(fam, a.mask || a.block_mask, a.dropout_p > 0.0, ex_windowed(a), ex_scoremod(a), a.sinks && !backward);
}

// Every reachable combination, as the six if-ladders of the kernels' host side spelled them before this function
// (comments: line of fa_ex_mfma.hip, or of fa_ex_mfma_kv8.hip where it says kv8, at commit 11dac10).  x0 / x1: an input the ladder did not look at, given both ways.
namespace exm_feat_table {
constexpr bool x0 = false, x1 = true;
constexpr int S = kFeatScore, K = kFeatScore | kFeatSink, V = kFeatVarlen, P = kFeatVarlen | kFeatPaged, Q = kFeatVarlen | kFeatPaged | kFeatKv8;
// exm_by_feat_s<S = 0>, <S = kFeatScore> (a backward, or a forward without sinks)                masks drop   win  score sink
static_assert(exm_feat(kExmDense, x0, x1, true, false, false) == 7 && exm_feat(kExmDense, x1, x1, true, false, false) == 7);          // 493
static_assert(exm_feat(kExmDense, true, false, true, false, false) == 5);                                                              // 494
static_assert(exm_feat(kExmDense, false, false, true, false, false) == 4);                                                             // 495
static_assert(exm_feat(kExmDense, x0, x1, false, false, false) == 3 && exm_feat(kExmDense, x1, x1, false, false, false) == 3);        // 497
static_assert(exm_feat(kExmDense, true, false, false, false, false) == 1);                                                             // 498
static_assert(exm_feat(kExmDense, false, false, false, false, false) == 0);                                                            // 499
static_assert(exm_feat(kExmDense, x0, x1, true, true, false) == (S | 7) && exm_feat(kExmDense, x1, x1, true, true, false) == (S | 7));   // 493, 518
static_assert(exm_feat(kExmDense, true, false, true, true, false) == (S | 5));                                                         // 494
static_assert(exm_feat(kExmDense, false, false, true, true, false) == (S | 4));                                                        // 495
static_assert(exm_feat(kExmDense, x0, x1, false, true, false) == (S | 3) && exm_feat(kExmDense, x1, x1, false, true, false) == (S | 3)); // 497
static_assert(exm_feat(kExmDense, true, false, false, true, false) == (S | 1));                                                        // 498
static_assert(exm_feat(kExmDense, false, false, false, true, false) == S);                                                             // 499
// exm_fwd_sink (the forward of a sink call, with a modifier or without)
static_assert(exm_feat(kExmDense, x0, x1, true, x0, true) == (K | 7) && exm_feat(kExmDense, x1, x1, true, x1, true) == (K | 7));      // 507
static_assert(exm_feat(kExmDense, true, false, true, x0, true) == (K | 5) && exm_feat(kExmDense, true, false, true, x1, true) == (K | 5));     // 508
static_assert(exm_feat(kExmDense, false, false, true, x0, true) == (K | 4) && exm_feat(kExmDense, false, false, true, x1, true) == (K | 4));   // 509
static_assert(exm_feat(kExmDense, x0, x1, false, x0, true) == (K | 3) && exm_feat(kExmDense, x1, x1, false, x1, true) == (K | 3));    // 511
static_assert(exm_feat(kExmDense, true, false, false, x0, true) == (K | 1) && exm_feat(kExmDense, true, false, false, x1, true) == (K | 1));   // 512
static_assert(exm_feat(kExmDense, false, false, false, x0, true) == K && exm_feat(kExmDense, false, false, false, x1, true) == K);    // 513
// exm_varlen_by_feat_s<0>, <kFeatScore> (+ kFeatVarlen in exm_varlen_t, 541 / 573 / 583); masks never looked at
static_assert(exm_feat(kExmVarlen, x0, true, true, false, false) == (V | 6) && exm_feat(kExmVarlen, x1, true, true, false, false) == (V | 6));     // 595
static_assert(exm_feat(kExmVarlen, x0, false, true, false, false) == (V | 4) && exm_feat(kExmVarlen, x1, false, true, false, false) == (V | 4));   // 595
static_assert(exm_feat(kExmVarlen, x0, true, false, false, false) == (V | 2) && exm_feat(kExmVarlen, x0, false, false, false, false) == V);        // 596
static_assert(exm_feat(kExmVarlen, x0, true, true, true, false) == (V | S | 6) && exm_feat(kExmVarlen, x0, false, true, true, false) == (V | S | 4));   // 595, 606
static_assert(exm_feat(kExmVarlen, x0, true, false, true, false) == (V | S | 2) && exm_feat(kExmVarlen, x0, false, false, true, false) == (V | S));     // 596, 606
// exm_varlen_by_feat, the forward of a sink call
static_assert(exm_feat(kExmVarlen, x0, true, true, x0, true) == (V | K | 6) && exm_feat(kExmVarlen, x0, false, true, x1, true) == (V | K | 4));    // 603
static_assert(exm_feat(kExmVarlen, x0, true, false, x0, true) == (V | K | 2) && exm_feat(kExmVarlen, x0, false, false, x1, true) == (V | K));      // 604
// exm_paged_by_feat (+ kFeatVarlen | kFeatPaged, 628); forward only, dropout turned away by ex_mfma_paged_supported
static_assert(exm_feat(kExmPaged, x0, false, true, x0, true) == (P | K | 4) && exm_feat(kExmPaged, x0, false, false, x1, true) == (P | K));        // 639
static_assert(exm_feat(kExmPaged, x0, false, true, true, false) == (P | S | 4) && exm_feat(kExmPaged, x0, false, false, true, false) == (P | S));  // 640
static_assert(exm_feat(kExmPaged, x0, false, true, false, false) == (P | 4) && exm_feat(kExmPaged, x1, false, false, false, false) == P);          // 641
// exm_paged_kv8_by_feat (+ kFeatVarlen | kFeatPaged | kFeatKv8, kv8 286)
static_assert(exm_feat(kExmPagedKv8, x0, false, true, x0, true) == (Q | K | 4) && exm_feat(kExmPagedKv8, x0, false, false, x1, true) == (Q | K));  // kv8 297
static_assert(exm_feat(kExmPagedKv8, x0, false, true, true, false) == (Q | S | 4) && exm_feat(kExmPagedKv8, x0, false, false, true, false) == (Q | S));   // kv8 298
static_assert(exm_feat(kExmPagedKv8, x0, false, true, false, false) == (Q | 4) && exm_feat(kExmPagedKv8, x1, false, false, false, false) == Q);    // kv8 299
// the bias family (fa_ex_mfma_bias.hip): one FEAT, whatever the other inputs say
static_assert(exm_feat(kExmBias, x0, x0, x0, x0, x0) == (256 | S) && exm_feat(kExmBias, x1, x1, x1, x1, x1) == (256 | S));
static_assert(exm_feat(kExmBias, x0, x0, x0, x1, x0) == (kFeatBias | kFeatScore));
}  // namespace exm_feat_table

// ---- the FEAT values a family may instantiate: {feature bits} x {plain, score, score + sink}.  An instantiation with kFeatSink
// or kFeatPaged is a forward kernel alone; every other one is a forward, a dK/dV (two with the mask bit: M16) and a dQ kernel.
template <int... F> struct ExmFeats {};
template <int BASE, int... F> using ExmFeatsX3 = ExmFeats<(BASE | F)..., (BASE | kFeatScore | F)..., (BASE | kFeatScore | kFeatSink | F)...>;
using ExmDenseFeats = ExmFeatsX3<0, 0, 1, 3, 4, 5, 7>;
using ExmVarlenFeats = ExmFeatsX3<kFeatVarlen, 0, 2, 4, 6>;
using ExmPagedFeats = ExmFeatsX3<kFeatVarlen | kFeatPaged, 0, 4>;
using ExmPagedKv8Feats = ExmFeatsX3<kFeatVarlen | kFeatPaged | kFeatKv8, 0, 4>;
using ExmBiasFeats = ExmFeats<kFeatBias | kFeatScore>;   // a forward, a dK/dV and a dQ kernel (fa_ex_mfma_bias.hip)

// run(tag, D, FEAT as integral constants) for the call's dtype and head_dim and for `feat`, if the list holds it; a FEAT outside
// the list is hipErrorInvalidValue, never another kernel
template <typename Tag, int D, typename Run, int... F>
inline hipError_t exm_walk(ExmFeats<F...>, int feat, Run&& run) {
    hipError_t e = hipErrorInvalidValue;
    (void)((feat == F && ((e = run(Tag{}, std::integral_constant<int, D>{}, std::integral_constant<int, F>{})), true)) || ...);
    return e;
}
template <typename Feats, typename Run>
inline hipError_t exm_dispatch(const ExArgs& a, int feat, Run&& run) {
    if (a.dtype == 2) return a.d > 64 ? exm_walk<bf16_tag, 128>(Feats{}, feat, run) : exm_walk<bf16_tag, 64>(Feats{}, feat, run);
    return a.d > 64 ? exm_walk<f16_tag, 128>(Feats{}, feat, run) : exm_walk<f16_tag, 64>(Feats{}, feat, run);
}

}  // namespace

}  // namespace fa
