// What the readers of a quantised KV cache share (fa_fp8_decode.hip, fa_fp4_decode.hip, fa_fp4_prefill.hip): the operand vector
// types, the 4 x 4 byte transpose, the MXFP4 V^T image, the featured kernel arguments with the one function that fills them, and
// the dtype x paged launch ladder.  One definition each.
#pragma once
#include <algorithm>
#include <type_traits>

#include "fa_decode_common.h"   // kv_cu_range, kPlseFill: the packed calls

namespace fa {

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef long long i64x4_t __attribute__((ext_vector_type(4)));   // four group bases, held as values (an array becomes an indexed scratch slot)

constexpr int kFp4 = 4;                                  // v_mfma_scale_f32_32x32x64_f8f6f4's format selector of e2m1 (0: e4m3)

// 4 x 4 byte transpose: x[c] holds bytes (d0, d1, d2, d3) of key c; t[dd] gets byte dd of keys 0 .. 3 (key 0 in the low byte).
// v_perm_b32 selects bytes 0 .. 3 from its second source and 4 .. 7 from its first.
__device__ __forceinline__ void transpose4x4(const uint32_t (&x)[4], uint32_t (&t)[4]) {
    const uint32_t lo01 = __builtin_amdgcn_perm(x[1], x[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(x[1], x[0], 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(x[3], x[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(x[3], x[2], 0x07030602u);
    t[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    t[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    t[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// the MXFP4 V^T image: 32 key bytes a channel row, 16 bytes of padding after every eight rows (the bank argument: the header of
// fa_fp4_decode.hip)
constexpr int kVt4Bytes = 32 * 128 + 16 * 16;
__device__ __forceinline__ int vt4_off(int row) { return 32 * row + 16 * (row >> 3); }

// What a featured instantiation takes beside its kernel's parameter block (the _mod calls; DESIGN.md sections 9zc, 9zi).  It is
// the kernel's argument pack Mod...: the plain instantiation has no such argument, and with its argument list keeps its instructions.
struct KvqMod {
    int wl, wr;                           // token i sees keys [i + coff - wl, i + coff + wr]; kWinNone: unbounded, wr = 0 if causal
    float cap_k, cap2;                    // 2 / softcap, softcap * log2(e); cap2 == 0: no softcap
};
// fp4kv_prefill_kernel's: it has no combine for the sinks to join in
struct KvqModSinks : KvqMod {
    const float* sinks;                   // one logit a query head (natural-log units), sinks[h % sink_heads]; null: none
    int sink_heads;
};

// the first argument of a kernel's pack Mod..., or for the plain instantiation (an empty pack) a value that nothing reads
template <typename M> __device__ __forceinline__ M kvq_mod_of() { return M{}; }
template <typename M, typename... Rest> __device__ __forceinline__ M kvq_mod_of(const M& m, const Rest&...) { return m; }

// the featured kernel arguments of an Fp8Mod (one that is not any(): no window, no cap)
inline KvqMod kvq_mod_args(const Fp8Mod& m, bool causal) {
    KvqMod md;
    md.wl = m.window_left >= 0 ? (int)std::min<int64_t>(m.window_left, kWinNone) : kWinNone;
    md.wr = causal ? 0 : (m.window_right >= 0 ? (int)std::min<int64_t>(m.window_right, kWinNone) : kWinNone);
    md.cap_k = m.softcap > 0.0 ? (float)(2.0 / m.softcap) : 0.f;
    md.cap2 = m.softcap > 0.0 ? (float)(m.softcap * 1.4426950408889634) : 0.f;
    return md;
}

// the launch ladder: f(tag, paged) with o's dtype as bf16_tag{} / f16_tag{} and paged as std::true_type{} / std::false_type{}
template <typename F> inline void kvq_dispatch(int dtype, bool paged, F&& f) {
    if (dtype == 2) {
        if (paged) f(bf16_tag{}, std::true_type{});
        else f(bf16_tag{}, std::false_type{});
    } else {
        if (paged) f(f16_tag{}, std::true_type{});
        else f(f16_tag{}, std::false_type{});
    }
}

}  // namespace

}  // namespace fa
