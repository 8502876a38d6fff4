// C-ABI entry points declared in include/fa_mi355x.h: argument validation, kernel dispatch,
// error reporting.  No torch types, no allocation, no device synchronisation: everything is
// enqueued on the caller's stream.
#include "../../include/fa_mi355x.h"
#include "fa_kernels.h"
#include <unordered_map>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <cstdint>

namespace {

thread_local char g_err[512] = "";
std::atomic<int> g_mode{FA_MODE_AUTO};

// ---- per-kernel event timing -------------------------------------------------------------------
struct ProfRec { int id; hipEvent_t a, b; };
std::atomic<int> g_prof_on{0};
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_free;
hipEvent_t g_prof_open[fa::K_COUNT];
const char* const kKernelNames[fa::K_COUNT] = {"fwd_f32", "bwd_delta", "bwd_dkdv_f32", "bwd_dq_f32", "fwd_mfma",
                                               "bwd_mfma", "bwd_dq_cvt", "bwd_dq_mfma", "fp8_quant", "fwd_fp8", "ex_fwd", "ex_bwd", "kv_group_sum",
                                               "fp8in_vt", "fp8in_fwd", "fp8in_vt_varlen", "fp8in_fwd_varlen", "idx_pack", "idx_logits",
                                               "idx_topk", "fp8kv_split", "fp8q_amax", "fp8q_quant", "fp8q_fused", "fp8in_fwd_mod",
                                               "fp8in_fwd_varlen_mod", "fp8kv_split_mod", "fp8kv_step_prep", "fp8in_fwd_hdim",
    "fp8in_fwd_varlen_hdim", "fp8kv_split_hdim", "fp8kv_split_varlen", "fp8kv_step_prep_varlen"};

hipEvent_t prof_get_event() {
    if (!g_prof_free.empty()) { hipEvent_t e = g_prof_free.back(); g_prof_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// ---- tuning knobs ---------------------------------------------------------------------------------
constexpr const char* kOptNames[fa::OPT_COUNT] = {"fwd_kb", "fwd_stag", "dkdv", "dq_kt", "fwd_rs", "dkdv_kreg", "fwd_eager", "fwd_hs", "fwd_tpw", "dq_tpw", "dkdv_tpw", "dq_nlf", "dq_w4", "fwd_abl", "small_grid", "fp8_rot", "dkdv_stg", "dkdv_abl", "dq", "dq_abl", "ex_path", "ds_chunk_mb", "fp8_pv", "fwd_rd", "fwd_w2", "dkdv_lean"};
constexpr const char* kOptEnv[fa::OPT_COUNT] = {"FA_FWD_KB", "FA_FWD_STAG", "FA_DKDV", "FA_DQ_KT", "FA_FWD_RS", "FA_DKDV_KREG", "FA_FWD_EAGER", "FA_FWD_HS", "FA_FWD_TPW", "FA_DQ_TPW", "FA_DKDV_TPW", "FA_DQ_NLF", "FA_DQ_W4", "FA_FWD_ABL", "FA_SMALL_GRID", "FA_FP8_ROT", "FA_DKDV_STG", "FA_DKDV_ABL", "FA_DQ", "FA_DQ_ABL", "FA_EX_PATH", "FA_DS_CHUNK_MB", "FA_FP8_PV", "FA_FWD_RD", "FA_FWD_W2", "FA_DKDV_LEAN"};
// a name added to OptionId without its two strings here would leave a null at the end of a table
template <size_t N> constexpr bool all_set(const char* const (&t)[N]) {
    for (size_t i = 0; i < N; ++i)
        if (!t[i]) return false;
    return true;
}
static_assert(all_set(kOptNames) && all_set(kOptEnv), "kOptNames / kOptEnv: one string per OptionId");
std::atomic<int> g_opts[fa::OPT_COUNT];
std::once_flag g_opts_once;
void init_opts() {
    for (int i = 0; i < fa::OPT_COUNT; ++i) {
        const char* e = getenv(kOptEnv[i]);
        int v = 0;
        if (e) v = (e[0] == 'w') ? atoi(e + 1) : atoi(e);   // FA_DKDV=w4 / w8 are accepted as 4 / 8
        g_opts[i].store(v);
    }
}

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// the end of a call that enqueued something: e is what HIP said
int launched(const char* who, hipError_t e) {
    if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "%s: HIP error %d (%s)", who, (int)e, hipGetErrorString(e));
    return FA_OK;
}

int check_common(const char* who, int64_t bh, int64_t n, int64_t d, int dtype, double scale) {
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: unknown dtype code %d", who, dtype);
    if (bh < 0 || n < 0 || d <= 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: bad shape (BH=%lld, N=%lld, d=%lld)", who, (long long)bh, (long long)n,
                    (long long)d);
    if (d > 256) return fail(FA_ERR_UNSUPPORTED, "%s: head_dim %lld > 256 is not supported", who, (long long)d);
    if (n > (int64_t)1 << 24) return fail(FA_ERR_UNSUPPORTED, "%s: N=%lld too large", who, (long long)n);
    if (bh * ((n + 63) / 64) >= ((int64_t)1 << 31))
        return fail(FA_ERR_UNSUPPORTED, "%s: BH*N too large for one launch", who);
    if (!(scale == scale)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale is NaN", who);
    return FA_OK;
}

// FA_MODE_BWD_ATOMIC (or the environment variable FA_BWD_VARIANT=atomic) selects the single-kernel backward whose
// dQ tiles are summed with global float atomics (5 GEMMs, not bitwise reproducible); the default is the split
// backward: dK/dV kernel + dQ kernel (7 GEMMs, no atomics, deterministic).
bool bwd_atomic_variant() {
    static const int env = [] { const char* e = getenv("FA_BWD_VARIANT"); return (e && !strcmp(e, "atomic")) ? 1 : 0; }();
    return env != 0 || g_mode.load() == FA_MODE_BWD_ATOMIC;
}
// the 16-bit MFMA kernels fold softmax_scale into the exp2 argument and need it finite and > 0
bool scale_ok(double s) { return s > 1e-20 && s < 1e20; }
// The 16-bit MFMA kernels read 16 bytes per lane and address each (b,h) slab with 32-bit byte offsets:
// every tensor must be 16-byte aligned and N*d*2 must stay below 2^31.  Anything else takes the exact-f32 kernels.
bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}
bool slab_ok(int64_t n, int64_t d) { return n * d * 2 < ((int64_t)1 << 31) - 65536; }
bool use_mfma_fwd(int dtype, int64_t n, int64_t d, double s, std::initializer_list<const void*> ps) {
    return g_mode.load() != FA_MODE_F32_GENERIC && scale_ok(s) && slab_ok(n, d) && aligned16(ps) &&
           fa::fwd_mfma_supported(dtype, d);
}
bool use_mfma_bwd(int dtype, int64_t n, int64_t d, double s, std::initializer_list<const void*> ps) {
    return g_mode.load() != FA_MODE_F32_GENERIC && scale_ok(s) && slab_ok(n, d) && aligned16(ps) &&
           fa::bwd_mfma_supported(dtype, d);
}

// Does an fa3 call with fp8 = 1 take the e4m3 path?  ONE predicate for fa3_forward and fa3_backward, over arguments that are the
// same in both calls (the workspace is not: a misaligned one is an error there), so that the backward always differentiates the
// function the forward evaluated.  It holds wherever the 16-bit MFMA kernels serve the call (f16 / bf16 tensors, head dims that
// are multiples of 8 up to 256): Q, K and V then go through OCP e4m3 with one scale per 64-row block, as the reference's wiring
// has it (csrc/fa3/fa3_fwd.cu:196-208) — at d = 128 on the e4m3 MFMA kernel, elsewhere as a round trip ahead of the 16-bit kernels.
// V~ is the same in both: where the all-e4m3 kernel runs (fa::fp8_v_pow2) every row of the forward and the backward's round trip
// use power-of-two V scales, elsewhere absmax / 448 ones.  What the backward does NOT reproduce is the e4m3 rounding of P in that
// kernel: it recomputes P exactly from lse (straight-through over the 8-bit P, as over the rounding of Q, K and V).
bool fp8_path(int dtype, int64_t n, int64_t d, double s, const void* q, const void* k, const void* v, const void* o) {
    return fa::fwd_mfma_supported(dtype, d) && fa::bwd_mfma_supported(dtype, d) && scale_ok(s) && g_mode.load() != FA_MODE_F32_GENERIC &&
           slab_ok(n, d) && aligned16({q, k, v, o});
}
size_t slab_bytes(int64_t bh, int64_t n, int64_t d) { return ((size_t)bh * n * d * 2 + 255) & ~(size_t)255; }   // one round-tripped 16-bit tensor

int forward_impl(const char* who, const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh,
                 int64_t n, int64_t d, int dtype, int causal, double scale, void* stream) {
    int rc = check_common(who, bh, n, d, dtype, scale);
    if (rc != FA_OK) return rc;
    if (bh == 0 || n == 0) return FA_OK;  // empty problem: nothing to write
    if (!q || !k || !v || !o || !lse) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    fa::FwdArgs a{q, k, v, o, lse, bh, n, d, dtype, causal ? 1 : 0, (float)scale};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = use_mfma_fwd(dtype, n, d, scale, {q, k, v, o}) ? fa::launch_fwd_mfma(a, st) : fa::launch_fwd_generic(a, st);
    if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "%s: HIP error %d (%s)", who, (int)e, hipGetErrorString(e));
    return FA_OK;
}

int backward_impl(const char* who, const void* q, const void* k, const void* v, const void* o, const void* dout,
                  const float* lse, void* dq, void* dk, void* dv, int64_t bh, int64_t n, int64_t d, int dtype,
                  int causal, double scale, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(who, bh, n, d, dtype, scale);
    if (rc != FA_OK) return rc;
    if (bh == 0 || n == 0) return FA_OK;
    if (!q || !k || !v || !o || !dout || !lse || !dq || !dk || !dv)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    const size_t need = fa_backward_workspace_bytes(bh, n, d, dtype);
    if (!ws || ws_bytes < need)
        return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, ws_bytes);
    fa::BwdArgs a{q, k, v, o, dout, lse, dq, dk, dv, bh, n, d, dtype, causal ? 1 : 0, (float)scale, ws, ws_bytes,
                   bwd_atomic_variant() ? 1 : 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = use_mfma_bwd(dtype, n, d, scale, {q, k, v, o, dout, dq, dk, dv, ws}) ? fa::launch_bwd_mfma(a, st) : fa::launch_bwd_generic(a, st);
    if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "%s: HIP error %d (%s)", who, (int)e, hipGetErrorString(e));
    return FA_OK;
}

}  // namespace

namespace fa {
int option(int id) {
    std::call_once(g_opts_once, init_opts);
    return g_opts[id].load(std::memory_order_relaxed);
}
int set_option(const char* name, int value) {
    std::call_once(g_opts_once, init_opts);
    for (int i = 0; i < OPT_COUNT; ++i)
        if (!strcmp(name, kOptNames[i])) { g_opts[i].store(value); return 0; }
    return -1;
}
std::atomic<long long> g_route_hits[ROUTE_COUNT];
constexpr const char* kRouteNames[ROUTE_COUNT] = {"dkdv_stream", "dkdv_lean", "fp8_quant_fused", "fp8_quant_two_pass", "fp8_quant_static",
                                                   "fp8in_fwd_mod", "fp8in_fwd_varlen_mod", "fp8kv_split_mod", "fp8kv_step_prep", "fp8in_fwd_hdim",
                                                   "fp8in_fwd_varlen_hdim", "fp8kv_split_hdim", "fp8kv_split_varlen",
                                                   "fp8kv_step_prep_varlen"};
void route_hit(int id) { g_route_hits[id].fetch_add(1, std::memory_order_relaxed); }
long long route_count(const char* name) {
    for (int i = 0; i < ROUTE_COUNT; ++i)
        if (!strcmp(name, kRouteNames[i])) return g_route_hits[i].load(std::memory_order_relaxed);
    return -1;
}
void prof_begin(int id, hipStream_t st) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t e = prof_get_event();
    (void)hipEventRecord(e, st);
    g_prof_open[id] = e;
}
void prof_end(int id, hipStream_t st) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t e = prof_get_event();
    (void)hipEventRecord(e, st);
    g_prof_recs.push_back(ProfRec{id, g_prof_open[id], e});
}
}  // namespace fa

namespace fa {
hipError_t ensure_dynamic_smem(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::unordered_map<uint64_t, int> granted;   // (device, kernel) -> bytes: the attribute is per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t key = reinterpret_cast<uint64_t>(kernel) ^ (static_cast<uint64_t>(dev + 1) << 56);
    std::lock_guard<std::mutex> lock(mu);
    auto it = granted.find(key);
    if (it != granted.end() && it->second >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) granted[key] = bytes;
    return e;
}
}  // namespace fa


extern "C" {

int fa_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof_recs) { g_prof_free.push_back(r.a); g_prof_free.push_back(r.b); }
    g_prof_recs.clear();
    return g_prof_on.exchange(on ? 1 : 0);
}

// Waits for the recorded events and writes "name count total_ms\n" lines for every kernel launched since
// fa_profile_enable(1). Returns the number of bytes written (excluding the NUL), or a negative error code.
int fa_profile_report(char* buf, size_t cap) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    double total[fa::K_COUNT] = {0};
    long count[fa::K_COUNT] = {0};
    for (auto& r : g_prof_recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) return fail(FA_ERR_LAUNCH, "fa_profile_report: event sync failed");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return fail(FA_ERR_LAUNCH, "fa_profile_report: elapsed failed");
        total[r.id] += ms;
        count[r.id] += 1;
    }
    std::string out;
    char line[128];
    for (int i = 0; i < fa::K_COUNT; ++i) {
        if (!count[i]) continue;
        snprintf(line, sizeof(line), "%s %ld %.6f\n", kKernelNames[i], count[i], total[i]);
        out += line;
    }
    if (!buf || cap == 0) return (int)out.size();
    const size_t nw = out.size() < cap - 1 ? out.size() : cap - 1;
    memcpy(buf, out.data(), nw);
    buf[nw] = 0;
    return (int)nw;
}

int fa1_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t n, int64_t d,
                int dtype, int causal, double softmax_scale, int64_t br, int64_t bc, void* stream) {
    (void)br; (void)bc;  // tile hints: results are tile independent (SURVEY §8b "Tile params")
    return forward_impl("fa1_forward", q, k, v, o, lse, bh, n, d, dtype, causal, softmax_scale, stream);
}

int fa1_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                 void* dq, void* dk, void* dv, int64_t bh, int64_t n, int64_t d, int dtype, int causal,
                 double softmax_scale, int64_t br, int64_t bc, void* workspace, size_t workspace_bytes, void* stream) {
    (void)br; (void)bc;
    return backward_impl("fa1_backward", q, k, v, o, do_, lse, dq, dk, dv, bh, n, d, dtype, causal, softmax_scale,
                         workspace, workspace_bytes, stream);
}

int fa2_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t n, int64_t d,
                int dtype, int causal, double softmax_scale, int64_t br, int64_t bc, void* stream) {
    (void)br; (void)bc;
    return forward_impl("fa2_forward", q, k, v, o, lse, bh, n, d, dtype, causal, softmax_scale, stream);
}

int fa2_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                 void* dq, void* dk, void* dv, int64_t bh, int64_t n, int64_t d, int dtype, int causal,
                 double softmax_scale, int64_t br, int64_t bc, void* workspace, size_t workspace_bytes, void* stream) {
    (void)br; (void)bc;
    return backward_impl("fa2_backward", q, k, v, o, do_, lse, dq, dk, dv, bh, n, d, dtype, causal, softmax_scale,
                         workspace, workspace_bytes, stream);
}

int fa3_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t n, int64_t d,
                int dtype, int causal, double softmax_scale, int64_t br, int64_t bc, int64_t stages, int fp8,
                void* workspace, size_t workspace_bytes, void* stream) {
    (void)br; (void)bc; (void)stages;
    // fp8: Q, K and V through e4m3 (see fp8_path).  fp32 tensors and head dims the 16-bit kernels do not take run the regular,
    // more accurate path (as the reference quietly skips its rotation for non-power-of-two d, src/fa3/torch/impl.py:60-61).
    if (fp8 && fp8_path(dtype, n, d, softmax_scale, q, k, v, o)) {
        int rc = check_common("fa3_forward", bh, n, d, dtype, softmax_scale);
        if (rc != FA_OK) return rc;
        if (bh == 0 || n == 0) return FA_OK;
        if (!q || !k || !v || !o || !lse) return fail(FA_ERR_INVALID_ARGUMENT, "fa3_forward: null tensor pointer");
        const size_t need = fa3_forward_workspace_bytes(bh, n, d, dtype, 1);
        if (!workspace || workspace_bytes < need || !aligned16({workspace}))
            return fail(FA_ERR_WORKSPACE, "fa3_forward: a 16-byte aligned workspace of %zu bytes is needed, %zu given", need, workspace_bytes);
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        const size_t slab = slab_bytes(bh, n, d);
        char* ws = reinterpret_cast<char*>(workspace);
        hipError_t e;
        if (fa::fwd_fp8_supported(dtype, d)) {
            // d = 128: [V~][the e4m3 kernels' own workspace: Q, K, V^T bytes and scales].  Default: S and P.V on the e4m3 MFMA;
            // option fp8_pv = 1: S on the e4m3 MFMA, P.V 16-bit on the round-tripped V.
            fa::FwdArgs a{q, k, v, o, lse, bh, n, d, dtype, causal ? 1 : 0, (float)softmax_scale};
            e = fa::launch_fwd_fp8(a, ws + slab, ws, st);
        } else {
            // [Q~][K~][V~] (original basis), then the 16-bit kernels as they are
            e = fa::launch_fp8_roundtrip(q, k, v, ws, ws + slab, ws + 2 * slab, bh, n, d, dtype, st);
            if (e == hipSuccess)
                return forward_impl("fa3_forward", ws, ws + slab, ws + 2 * slab, o, lse, bh, n, d, dtype, causal, softmax_scale, stream);
        }
        if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "fa3_forward: HIP error %d (%s)", (int)e, hipGetErrorString(e));
        return FA_OK;
    }
    return forward_impl("fa3_forward", q, k, v, o, lse, bh, n, d, dtype, causal, softmax_scale, stream);
}

int fa3_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                 void* dq, void* dk, void* dv, int64_t bh, int64_t n, int64_t d, int dtype, int causal,
                 double softmax_scale, int64_t br, int64_t bc, int64_t stages, int fp8, void* workspace,
                 size_t workspace_bytes, void* stream) {
    (void)br; (void)bc; (void)stages;
    // fp8: differentiate the function the forward evaluated, i.e. attention of the e4m3-round-tripped Q, K and V
    // (the reference's fa3_backward does the same, csrc/fa3/fa3_bwd.cu:134-146); the gradients are returned for
    // q, k, v themselves (straight-through over the rounding).  o and lse then match the recomputed probabilities.
    if (fp8 && fp8_path(dtype, n, d, softmax_scale, q, k, v, o) && bh > 0 && n > 0) {
        int rc = check_common("fa3_backward", bh, n, d, dtype, softmax_scale);
        if (rc != FA_OK) return rc;
        if (!q || !k || !v) return fail(FA_ERR_INVALID_ARGUMENT, "fa3_backward: null tensor pointer");
        const size_t need = fa3_backward_workspace_bytes(bh, n, d, dtype, 1);
        if (!workspace || workspace_bytes < need || !aligned16({workspace}))
            return fail(FA_ERR_WORKSPACE, "fa3_backward: a 16-byte aligned workspace of %zu bytes is needed, %zu given", need, workspace_bytes);
        // layout: [Q~][K~][V~][the plain backward's workspace: everything that is left, so a caller who sized it with
        // fa_backward_workspace_bytes_fast's surplus gets the dS hand-over here too]
        const size_t slab = slab_bytes(bh, n, d);
        char* qt = reinterpret_cast<char*>(workspace);
        char *kt = qt + slab, *vt = qt + 2 * slab;
        hipError_t e = fa::launch_fp8_roundtrip(q, k, v, qt, kt, vt, bh, n, d, dtype, reinterpret_cast<hipStream_t>(stream));
        if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "fa3_backward: HIP error %d (%s)", (int)e, hipGetErrorString(e));
        return backward_impl("fa3_backward", qt, kt, vt, o, do_, lse, dq, dk, dv, bh, n, d, dtype, causal, softmax_scale,
                             qt + 3 * slab, workspace_bytes - 3 * slab, stream);
    }
    return backward_impl("fa3_backward", q, k, v, o, do_, lse, dq, dk, dv, bh, n, d, dtype, causal, softmax_scale,
                         workspace, workspace_bytes, stream);
}

// ---- extended attention: see include/fa_mi355x.h
static int ex_check(const char* who, int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype, double scale, const uint8_t* block_mask,
                    int64_t br, int64_t bc, double p) {
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: unknown dtype code %d", who, dtype);
    if (bh < 0 || nq < 0 || nk < 0 || d <= 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: bad shape (BH=%lld, Nq=%lld, Nk=%lld, d=%lld)", who, (long long)bh, (long long)nq,
                    (long long)nk, (long long)d);
    if (d > 256) return fail(FA_ERR_UNSUPPORTED, "%s: head_dim %lld > 256 is not supported", who, (long long)d);
    if (nq > (int64_t)1 << 24 || nk > (int64_t)1 << 24 || nq * d >= ((int64_t)1 << 31) || nk * d >= ((int64_t)1 << 31) ||
        bh * ((nq + 15) / 16) >= ((int64_t)1 << 31) || bh * ((nk + 15) / 16) >= ((int64_t)1 << 31))
        return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    if (!(scale == scale)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale is NaN", who);
    if (block_mask && (br <= 0 || bc <= 0)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: block-sparse mask needs br, bc > 0", who);
    if (!(p >= 0.0 && p < 1.0)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: dropout_p must lie in [0, 1)", who);
    return FA_OK;
}

// grouped-query attention: kv_group query heads per K/V head (k and v hold bh / kv_group units)
static int group_check(const char* who, int64_t bh, int64_t kv_group) {
    if (kv_group < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: kv_group must be >= 1 (got %lld)", who, (long long)kv_group);
    if (bh % kv_group != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: BH=%lld is not a multiple of kv_group=%lld", who, (long long)bh, (long long)kv_group);
    if (kv_group > 1 && bh * kv_group >= ((int64_t)1 << 32))   // (the kernels divide by kv_group with a 32-bit multiplier)
        return fail(FA_ERR_UNSUPPORTED, "%s: BH * kv_group too large", who);
    return FA_OK;
}

// sliding window (local attention): key j is visible to query i only if j >= i + (Nk - Nq) - wl and j <= i + (Nk - Nq) + wr,
// -1 = unbounded on that side.  Canonical form (a window that bounds nothing is then exactly the call without one): bounds that
// cut nothing are dropped, and wr = 0 without the causal mask IS the causal mask.
static int window_canon(const char* who, int64_t nq, int64_t nk, int& causal, int64_t& wl, int64_t& wr) {
    if (wl < -1 || wr < -1)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: window (%lld, %lld): each bound must be >= 0, or -1 for unbounded", who,
                    (long long)wl, (long long)wr);
    if (wl >= nk - 1) wl = -1;            // the first key is in every row's band
    if (wr >= nq - 1) wr = -1;            // the last key is in every row's band
    if (causal && wr >= 0) wr = -1;       // the diagonal bounds more
    if (!causal && wr == 0) { causal = 1; wr = -1; }
    return FA_OK;
}

// score modifiers (fa_ex_*_scoremod): softcap and ALiBi slopes; the default is none
struct ScoreMod {
    double softcap = 0.0;
    const float* alibi = nullptr;
    int64_t heads = 1, bstride = 0;
};
static int score_check(const char* who, const ScoreMod& m, int64_t bh) {
    if (!(m.softcap >= 0.0) || m.softcap > 1.7976931348623157e308)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softcap must be a finite number >= 0 (got %g)", who, m.softcap);
    if (m.bstride < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: alibi_batch_stride must be >= 0 (got %lld)", who, (long long)m.bstride);
    if (m.alibi && m.heads < 1)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: alibi_heads must be >= 1 (got %lld)", who, (long long)m.heads);
    if (m.alibi && bh % m.heads != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: alibi_heads=%lld does not divide BH=%lld", who, (long long)m.heads, (long long)bh);
    if (m.alibi && (m.heads >= ((int64_t)1 << 31) || m.bstride >= ((int64_t)1 << 31) || (bh / m.heads) * m.bstride >= ((int64_t)1 << 31)))
        return fail(FA_ERR_UNSUPPORTED, "%s: alibi slope indices too large", who);
    return FA_OK;
}
static void score_args(fa::ExArgs& a, const ScoreMod& m) {
    a.softcap = m.softcap;
    a.alibi = m.alibi;
    a.alibi_heads = m.heads;
    a.alibi_bstride = m.bstride;
}

// attention sinks (fa_ex_*_sink): one learnable logit per head as an extra softmax column; the default is none.  sinks == null is
// the call without them and nothing else of the struct is read.
struct SinkArg {
    const float* sinks = nullptr;
    int64_t heads = 1;
    float* dsinks = nullptr;   // backward: (heads,) float32
};
// units: the query units u (unit u takes sinks[u % heads]); backward: the call writes dsinks
static int sink_check(const char* who, const SinkArg& sk, int64_t units, bool backward) {
    if (!sk.sinks) return FA_OK;
    if ((uintptr_t)sk.sinks % 4 != 0 || (uintptr_t)sk.dsinks % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: sinks and dsinks must be 4-byte aligned", who);
    if (sk.heads < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: sink_heads must be >= 1 (got %lld)", who, (long long)sk.heads);
    if (units % sk.heads != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: sink_heads=%lld does not divide the %lld query units", who, (long long)sk.heads,
                    (long long)units);
    if (sk.heads >= ((int64_t)1 << 31)) return fail(FA_ERR_UNSUPPORTED, "%s: sink_heads too large", who);
    if (backward && !sk.dsinks) return fail(FA_ERR_INVALID_ARGUMENT, "%s: sinks without dsinks", who);
    return FA_OK;
}
static void sink_args(fa::ExArgs& a, const SinkArg& sk) {
    a.sinks = sk.sinks;
    a.sink_heads = sk.sinks ? sk.heads : 1;
    a.dsinks = sk.dsinks;
}

// A forward without a key: every row is a row without a visible key, o = 0 and lse = -inf, with sinks the head's sink.
// o: units * rows * d elements, lse: units * rows.
static int no_key_fill(const char* who, void* o, float* lse, int64_t units, int64_t rows, int64_t d, int dtype, const SinkArg& sk, hipStream_t st) {
    hipError_t e = hipMemsetAsync(o, 0, (size_t)units * rows * d * (dtype == FA_DTYPE_F32 ? 4 : 2), st);
    if (e == hipSuccess && sk.sinks) e = fa::launch_ex_sink_fill(lse, sk.sinks, sk.heads, units, rows, st);
    else if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lse), (int)0xFF800000u, (size_t)units * rows, st);
    return launched(who, e);
}

// A backward without a query row or without a key.  With sinks their gradient is 0 (no row, or rows with o = 0: delta = 0); nothing
// else where both sides are empty; else the gradients of the side that has rows are sums over nothing: dk and dv where there is no
// query row, dq where there is no key.
// (dv_bytes: dv's own size where v is narrower than k, fa_ex_*_vdim; default: dk's)
static int empty_backward(const char* who, bool both, bool no_q, void* dq, size_t dq_bytes, void* dk, void* dv, size_t dkv_bytes,
                          const SinkArg& sk, hipStream_t st, size_t dv_bytes = ~(size_t)0) {
    hipError_t e = sk.sinks ? hipMemsetAsync(sk.dsinks, 0, (size_t)sk.heads * 4, st) : hipSuccess;
    if (e != hipSuccess || both) return launched(who, e);
    if (no_q ? (!dk || !dv) : !dq) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (no_q) {
        e = hipMemsetAsync(dk, 0, dkv_bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(dv, 0, dv_bytes == ~(size_t)0 ? dkv_bytes : dv_bytes, st);
    } else {
        e = hipMemsetAsync(dq, 0, dq_bytes, st);
    }
    return launched(who, e);
}

// V narrower than Q / K (fa_ex_*_vdim: d_v after the sink / dlse group).  d_v = 0 and d_v = d are the call without the argument and
// never come here.  The first broken rule, in this order: the widths (d_v > d; multiples of 8; d <= 192; d_v <= 128), the dtype,
// then each feature the two-width kernels do not have, by name, then the scale.  Before any other check and any HIP call.
struct VdimExtras {
    bool mask = false, block_mask = false, dropout = false, window = false, softcap = false, alibi = false, sinks = false;
};
static int vdim_check(const char* who, int64_t d, int64_t d_v, int dtype, double scale, const VdimExtras& x) {
    if (d_v < 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: d_v must be >= 0 (got %lld)", who, (long long)d_v);
    if (d_v > d)
        return fail(FA_ERR_UNSUPPORTED, "%s: d_v=%lld > d=%lld: a v wider than q and k is not supported", who, (long long)d_v, (long long)d);
    if (d % 8 != 0 || d_v % 8 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs d and d_v to be multiples of 8 (got d=%lld, d_v=%lld)", who, (long long)d,
                    (long long)d_v);
    if (d > 192) return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs d <= 192 (got d=%lld)", who, (long long)d);
    if (d_v > 128) return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs d_v <= 128 (got d_v=%lld)", who, (long long)d_v);
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs f16 or bf16 tensors (dtype code %d): there are no exact-f32 kernels with two widths",
                    who, dtype);
    const char* name = x.mask ? "mask" : x.block_mask ? "block_sparse_mask" : x.dropout ? "dropout_p > 0" : x.window ? "window_size"
                       : x.softcap ? "softcap" : x.alibi ? "alibi_slopes" : x.sinks ? "sinks" : nullptr;
    if (name) return fail(FA_ERR_UNSUPPORTED, "%s: %s is not supported with d_v != d", who, name);
    if (!(scale > 0.0)) return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs softmax_scale > 0", who);
    return FA_OK;
}
// ... and what only the pointers and strides tell, once they are known to be there: 16-byte aligned tensors, 16-byte rows
static int vdim_layout_check(const char* who, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides) {
    for (const void* ptr : ptrs)
        if ((uintptr_t)ptr % 16 != 0) return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs 16-byte aligned tensors", who);
    for (const int64_t st : strides)
        if (st % 8 != 0) return fail(FA_ERR_UNSUPPORTED, "%s: d_v != d needs token strides that are multiples of 8 elements", who);
    return FA_OK;
}

// An additive attention bias (fa_ex_*_bias: the group after d_v).  bias == null with everything else of the group 0 / null is the
// call without the argument and goes no further than the first rule.  The first broken rule, in this order, before any other check
// and any HIP call: (1) a null bias with a stride or a dbias; (2) bias or dbias not 16-byte aligned; (3) a stride that is negative
// or no multiple of 8; (4) bias_heads < 1 or not dividing BH; (5) a dbias for a row-broadcast bias; then each feature the bias kernels
// do not have, by name: (6) mask, block_sparse_mask, dropout_p > 0, window_size, softcap, alibi_slopes, sinks, d_v != d;
// (7) f32 tensors; (8) d > 128 or d % 8 != 0; (9) softmax_scale <= 0; (10) a unit's rows beyond the 32-bit offsets.
struct BiasArg {
    const void* bias = nullptr;
    int64_t heads = 0, bs = 0, hs = 0, rs = 0;
    void* dbias = nullptr;         // backward: null = no gradient asked for
    int64_t dbs = 0, dhs = 0, drs = 0;
};
struct BiasExtras {
    bool mask = false, block_mask = false, dropout = false, window = false, softcap = false, alibi = false, sinks = false, vdim = false;
};
static int bias_check(const char* who, const BiasArg& b, int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype, double scale,
                      const BiasExtras& x) {
    if (!b.bias) {
        if (b.bs != 0 || b.hs != 0 || b.rs != 0 || b.dbias || b.dbs != 0 || b.dhs != 0 || b.drs != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: bias is null, but a bias stride or dbias is given", who);
        return FA_OK;
    }
    if ((uintptr_t)b.bias % 16 != 0 || (uintptr_t)b.dbias % 16 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: bias and dbias must be 16-byte aligned", who);
    for (const int64_t s : {b.bs, b.hs, b.rs, b.dbs, b.dhs, b.drs})
        if (s < 0 || s % 8 != 0)
            return fail(FA_ERR_UNSUPPORTED,
                        "%s: every bias and dbias stride must be 0 (broadcast) or a positive multiple of 8 elements (got %lld): allocate the "
                        "last dim padded to a multiple of 8 and pass the slice", who, (long long)s);
    if (b.heads < 1 || bh % b.heads != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: bias_heads=%lld does not divide BH=%lld", who, (long long)b.heads, (long long)bh);
    if (b.dbias && nq > 1 && (b.rs == 0 || b.drs == 0))
        return fail(FA_ERR_UNSUPPORTED, "%s: dbias for a row-broadcast bias (bias_row_stride = 0) is not supported", who);
    if (x.mask) return fail(FA_ERR_UNSUPPORTED, "%s: mask is not supported with a bias: fold it into the bias as -inf", who);
    const char* name = x.block_mask ? "block_sparse_mask" : x.dropout ? "dropout_p > 0" : x.window ? "window_size" : x.softcap ? "softcap"
                       : x.alibi ? "alibi_slopes" : x.sinks ? "sinks" : x.vdim ? "d_v != d" : nullptr;
    if (name) return fail(FA_ERR_UNSUPPORTED, "%s: %s is not supported with a bias", who, name);
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_UNSUPPORTED, "%s: a bias needs f16 or bf16 tensors (dtype code %d): there are no exact-f32 kernels with a bias", who, dtype);
    if (d > 128 || d % 8 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: a bias needs d <= 128 and d %% 8 == 0 (got d=%lld): there are no exact-f32 kernels with a bias", who,
                    (long long)d);
    if (!(scale > 0.0)) return fail(FA_ERR_UNSUPPORTED, "%s: a bias needs softmax_scale > 0", who);
    const int64_t rmax = b.rs > b.drs ? b.rs : b.drs;
    if (nq > 0 && nk > 0 && (nq + 256) > (((int64_t)1 << 30) - nk - 512) / (rmax > 0 ? rmax : 1))
        return fail(FA_ERR_UNSUPPORTED, "%s: a unit's bias rows span more than 2^31 bytes", who);
    return FA_OK;
}

// One call of the fa_ex_forward* / fa_ex_backward* family.  The defaults are the narrower entry points' "argument absent": an entry
// point assigns the arguments it has (ex_call / ex_bwd_call: the ones all of them have) and leaves the rest.
struct ExCall {
    const void *q = nullptr, *k = nullptr, *v = nullptr, *do_ = nullptr;
    void* o = nullptr;      // (the backward only reads o and lse)
    float* lse = nullptr;
    void *dq = nullptr, *dk = nullptr, *dv = nullptr;
    int64_t bh = 0, kv_group = 1, nq = 0, nk = 0, d = 0, window_left = -1, window_right = -1;
    int dtype = 0, causal = 0;
    double softmax_scale = 0.0, dropout_p = 0.0;
    ScoreMod sm;
    SinkArg sk;
    const float* dlse = nullptr;   // fa_ex_backward_dlse: the gradient of lse, (bh, nq) float32
    int64_t d_v = 0;               // fa_ex_*_vdim: the width of v, o, do_ and dv (0: d)
    BiasArg bi;                    // fa_ex_*_bias
    const uint8_t *mask = nullptr, *block_mask = nullptr;
    int64_t mask_bh_stride = 0, br = 0, bc = 0;
    uint64_t dropout_seed = 0;
    void *workspace = nullptr, *stream = nullptr;
    size_t workspace_bytes = 0;
};

// does the call carry a v of its own width?  (d_v = 0 and d_v = d: the call without the argument)
static bool ex_vdim(const ExCall& c) { return c.d_v != 0 && c.d_v != c.d; }
static int ex_vdim_check(const char* who, const ExCall& c) {
    if (!ex_vdim(c) || c.d <= 0) return FA_OK;
    VdimExtras x;
    x.mask = c.mask != nullptr; x.block_mask = c.block_mask != nullptr; x.dropout = c.dropout_p > 0.0;
    x.window = c.window_left != -1 || c.window_right != -1; x.softcap = c.sm.softcap > 0.0; x.alibi = c.sm.alibi != nullptr;
    x.sinks = c.sk.sinks != nullptr;
    return vdim_check(who, c.d, c.d_v, c.dtype, c.softmax_scale, x);
}

static int ex_bias_check(const char* who, const ExCall& c) {
    BiasExtras x;
    x.mask = c.mask != nullptr; x.block_mask = c.block_mask != nullptr; x.dropout = c.dropout_p > 0.0;
    x.window = c.window_left != -1 || c.window_right != -1; x.softcap = c.sm.softcap > 0.0; x.alibi = c.sm.alibi != nullptr;
    x.sinks = c.sk.sinks != nullptr; x.vdim = ex_vdim(c);
    return bias_check(who, c.bi, c.bh, c.nq, c.nk, c.d, c.dtype, c.softmax_scale, x);
}
// is dbias the sum over a broadcast batch or head dimension (through the workspace)?
static bool ex_dbias_reduced(const ExCall& c) {
    return c.bi.bias && c.bi.dbias && fa::ex_bias_reduced(c.bh, c.bi.heads, c.bi.dbs, c.bi.dhs);
}

// the argument checks of a forward and a backward, in their order; the mask comes back canonical
static int ex_checks(const char* who, const ExCall& c, bool backward, int& causal, int64_t& wl, int64_t& wr) {
    int rc = ex_check(who, c.bh, c.nq, c.nk, c.d, c.dtype, c.softmax_scale, c.block_mask, c.br, c.bc, c.dropout_p);
    if (rc != FA_OK) return rc;
    if ((rc = group_check(who, c.bh, c.kv_group)) != FA_OK) return rc;
    if ((rc = score_check(who, c.sm, c.bh)) != FA_OK) return rc;
    if ((rc = sink_check(who, c.sk, c.bh, backward)) != FA_OK) return rc;
    return window_canon(who, c.nq, c.nk, causal, wl, wr);
}

// what the launcher takes (the canonical mask: the caller's; a forward leaves the backward's pointers and the workspace absent)
static fa::ExArgs ex_args(const ExCall& c, int causal, int64_t wl, int64_t wr) {
    fa::ExArgs a{c.q, c.k, c.v, c.o, c.lse, c.do_, c.dq, c.dk, c.dv, c.bh, c.nq, c.nk, c.d, c.dtype, causal ? 1 : 0,
                 (float)c.softmax_scale, c.mask, c.mask_bh_stride, c.block_mask, c.br, c.bc, c.dropout_p, c.dropout_seed, c.workspace,
                 c.workspace_bytes};
    a.kv_group = c.kv_group;
    a.window_left = wl;
    a.window_right = wr;
    score_args(a, c.sm);
    sink_args(a, c.sk);
    a.dlse = c.dlse;
    a.d_v = ex_vdim(c) ? c.d_v : 0;
    if (c.bi.bias) {
        a.bias = c.bi.bias; a.bias_heads = c.bi.heads;
        a.bias_bstride = c.bi.bs; a.bias_hstride = c.bi.hs; a.bias_rstride = c.bi.rs;
        a.dbias = c.bi.dbias;
        a.dbias_bstride = c.bi.dbs; a.dbias_hstride = c.bi.dhs; a.dbias_rstride = c.bi.drs;
    }
    return a;
}

// the gradient of lse (fa_ex_backward_dlse / fa_ex_backward_varlen_dlse): null = none
static int dlse_check(const char* who, const float* dlse) {
    if ((uintptr_t)dlse % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: dlse must be 4-byte aligned", who);
    return FA_OK;
}
// A backward with query rows but without a key, with sinks and a gradient of lse: every row's lse is its head's sink, so
// dsinks[h] = the sum of dlse over the rows of head h (empty_backward has zeroed it; the sum kernel overwrites it)
static int no_key_dsinks(const char* who, const fa::ExArgs& a, hipStream_t st) {
    if (!a.lse) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    return launched(who, fa::launch_ex_dsink(a, a.dlse, a.cu_q ? a.total_q : 0, 1, -1.f, st));
}

static int ex_forward_impl(const char* who, const ExCall& c) {
    int causal = c.causal;
    int64_t wl = c.window_left, wr = c.window_right;   // (window_canon rewrites the three)
    if (const int rc = ex_bias_check(who, c); rc != FA_OK) return rc;
    if (const int rc = ex_vdim_check(who, c); rc != FA_OK) return rc;
    if (const int rc = ex_checks(who, c, false, causal, wl, wr); rc != FA_OK) return rc;
    if (c.bh == 0 || c.nq == 0) return FA_OK;
    if (!c.q || !c.o || !c.lse || (c.nk > 0 && (!c.k || !c.v))) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (ex_vdim(c))
        if (const int rc = vdim_layout_check(who, {c.q, c.k, c.v, c.o}, {}); rc != FA_OK) return rc;
    if (c.nk == 0) return no_key_fill(who, c.o, c.lse, c.bh, c.nq, ex_vdim(c) ? c.d_v : c.d, c.dtype, c.sk, reinterpret_cast<hipStream_t>(c.stream));
    return launched(who, fa::launch_ex(ex_args(c, causal, wl, wr), false, reinterpret_cast<hipStream_t>(c.stream)));
}

// the grouped minimum: the ungrouped one for bh query units, plus (kv_group > 1) the dK / dV partial slabs in front of it
static size_t ex_bwd_ws_grouped(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype) {
    size_t need = fa_ex_backward_workspace_bytes(bh, nq, nk, d, dtype);
    if (kv_group > 1 && bh > 0 && nq > 0 && nk > 0 && d > 0) need += 2 * fa::kv_partial_bytes(bh, nk, d, dtype);
    return need;
}

static int ex_backward_impl(const char* who, const ExCall& c) {
    int causal = c.causal;
    int64_t wl = c.window_left, wr = c.window_right;
    if (const int rc = ex_bias_check(who, c); rc != FA_OK) return rc;
    if (const int rc = ex_vdim_check(who, c); rc != FA_OK) return rc;
    if (const int rc = ex_checks(who, c, true, causal, wl, wr); rc != FA_OK) return rc;
    if (const int rc = dlse_check(who, c.dlse); rc != FA_OK) return rc;
    const bool no_q = c.bh == 0 || c.nq == 0, no_k = c.bh == 0 || c.nk == 0;
    const size_t es = c.dtype == FA_DTYPE_F32 ? 4 : 2;
    if (no_q || no_k) {   // (grouped: dk and dv hold bh / kv_group units)
        const int rc = empty_backward(who, no_q && no_k, no_q, c.dq, (size_t)c.bh * c.nq * c.d * es, c.dk, c.dv,
                                      (size_t)(c.bh / c.kv_group) * c.nk * c.d * es, c.sk, reinterpret_cast<hipStream_t>(c.stream),
                                      (size_t)(c.bh / c.kv_group) * c.nk * (ex_vdim(c) ? c.d_v : c.d) * es);
        if (rc != FA_OK || no_q || !c.sk.sinks || !c.dlse) return rc;
        return no_key_dsinks(who, ex_args(c, causal, wl, wr), reinterpret_cast<hipStream_t>(c.stream));
    }
    if (!c.q || !c.k || !c.v || !c.o || !c.do_ || !c.lse || !c.dq || !c.dk || !c.dv)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (ex_vdim(c))
        if (const int rc = vdim_layout_check(who, {c.q, c.k, c.v, c.o, c.do_, c.dq, c.dk, c.dv}, {}); rc != FA_OK) return rc;
    size_t need = ex_bwd_ws_grouped(c.bh, c.kv_group, c.nq, c.nk, c.d, c.dtype);   // (d_v < d: the same rows, slabs of d's size)
    if (ex_dbias_reduced(c)) need += fa::ex_bias_ds_bytes(c.bh, c.nq, c.nk);          // (the per-unit dS of a broadcast dbias)
    if (!c.workspace || c.workspace_bytes < need)
        return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, c.workspace_bytes);
    return launched(who, fa::launch_ex(ex_args(c, causal, wl, wr), true, reinterpret_cast<hipStream_t>(c.stream)));
}

// the dS room of the hand-over where it serves the call (the plain backward's rule; grouped: sized for chunks of whole groups)
static size_t ex_bwd_ds_room(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal, int extras) {
    if (extras || bh <= 0 || nq <= 0 || nk <= 0 || g_mode.load() == FA_MODE_F32_GENERIC || fa::option(fa::OPT_EX_PATH) == 1 || fa::option(fa::OPT_EX_PATH) == 3) return 0;
    if (!fa::bwd_mfma_supported(dtype, d)) return 0;
    if (nq == nk) return fa::bwd_ds_extra_bytes(bh, nq, d, dtype, causal != 0, bwd_atomic_variant(), 0, kv_group);   // the plain backward's own rule
    if (!fa::nqnk_mfma_supported(dtype, d, bh, nq, nk, causal)) return 0;   // (under the mask: Nk >= Nq)
    return fa::bwd_ds_extra_bytes(bh, nq, d, dtype, causal != 0, false, nk, kv_group);
}

// the arguments every fa_ex_forward* has
static ExCall ex_call(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t nq, int64_t nk, int64_t d,
                      int dtype, int causal, double softmax_scale, const uint8_t* mask, int64_t mask_bh_stride,
                      const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream) {
    ExCall c;
    c.q = q; c.k = k; c.v = v; c.o = o; c.lse = lse;
    c.bh = bh; c.nq = nq; c.nk = nk; c.d = d; c.dtype = dtype; c.causal = causal; c.softmax_scale = softmax_scale;
    c.mask = mask; c.mask_bh_stride = mask_bh_stride; c.block_mask = block_mask; c.br = br; c.bc = bc;
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    return c;
}
// ... and every fa_ex_backward*
static ExCall ex_bwd_call(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                          void* dv, int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype, int causal, double softmax_scale,
                          const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p,
                          uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    ExCall c = ex_call(q, k, v, const_cast<void*>(o), const_cast<float*>(lse), bh, nq, nk, d, dtype, causal, softmax_scale, mask,
                       mask_bh_stride, block_mask, br, bc, dropout_p, dropout_seed, stream);
    c.do_ = do_; c.dq = dq; c.dk = dk; c.dv = dv; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return c;
}

int fa_ex_forward(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t nq, int64_t nk, int64_t d,
                  int dtype, int causal, double softmax_scale, const uint8_t* mask, int64_t mask_bh_stride,
                  const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream) {
    return ex_forward_impl("fa_ex_forward", ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride,
                                                    block_mask, br, bc, dropout_p, dropout_seed, stream));
}

int fa_ex_forward_grouped(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                          int64_t nk, int64_t d, int dtype, int causal, double softmax_scale, const uint8_t* mask, int64_t mask_bh_stride,
                          const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream) {
    ExCall c = ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask, br, bc, dropout_p,
                       dropout_seed, stream);
    c.kv_group = kv_group;
    return ex_forward_impl("fa_ex_forward_grouped", c);
}

int fa_ex_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                   void* dv, int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype, int causal, double softmax_scale,
                   const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p,
                   uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    return ex_backward_impl("fa_ex_backward", ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask,
                                                          mask_bh_stride, block_mask, br, bc, dropout_p, dropout_seed, workspace,
                                                          workspace_bytes, stream));
}

int fa_ex_backward_grouped(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq,
                           void* dk, void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                           double softmax_scale, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br,
                           int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group;
    return ex_backward_impl("fa_ex_backward_grouped", c);
}

int fa_ex_forward_window(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                         int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                         const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p,
                         uint64_t dropout_seed, void* stream) {
    ExCall c = ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask, br, bc, dropout_p,
                       dropout_seed, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    return ex_forward_impl("fa_ex_forward_window", c);
}

int fa_ex_backward_window(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq,
                          void* dk, void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                          int64_t window_left, int64_t window_right, double softmax_scale, const uint8_t* mask, int64_t mask_bh_stride,
                          const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace,
                          size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    return ex_backward_impl("fa_ex_backward_window", c);
}

int fa_ex_forward_scoremod(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                           int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                           double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const uint8_t* mask,
                           int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p,
                           uint64_t dropout_seed, void* stream) {
    ExCall c = ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask, br, bc, dropout_p,
                       dropout_seed, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    return ex_forward_impl("fa_ex_forward_scoremod", c);
}

int fa_ex_backward_scoremod(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq,
                            void* dk, void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                            int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                            int64_t alibi_heads, int64_t alibi_batch_stride, const uint8_t* mask, int64_t mask_bh_stride,
                            const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace,
                            size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    return ex_backward_impl("fa_ex_backward_scoremod", c);
}

int fa_ex_forward_sink(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                       int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                       double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks,
                       int64_t sink_heads, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc,
                       double dropout_p, uint64_t dropout_seed, void* stream) {
    ExCall c = ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask, br, bc, dropout_p,
                       dropout_seed, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    return ex_forward_impl("fa_ex_forward_sink", c);
}

int fa_ex_backward_sink(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p,
                        uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    return ex_backward_impl("fa_ex_backward_sink", c);
}

int fa_ex_backward_dlse(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const float* dlse, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc,
                        double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    c.dlse = dlse;
    return ex_backward_impl("fa_ex_backward_dlse", c);
}

int fa_ex_forward_vdim(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                       int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                       double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks,
                       int64_t sink_heads, int64_t d_v, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br,
                       int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream) {
    ExCall c = ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask, br, bc, dropout_p,
                       dropout_seed, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    c.d_v = d_v;
    return ex_forward_impl("fa_ex_forward_vdim", c);
}

int fa_ex_backward_vdim(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const float* dlse, int64_t d_v, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br,
                        int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    c.dlse = dlse;
    c.d_v = d_v;
    return ex_backward_impl("fa_ex_backward_vdim", c);
}

int fa_ex_forward_bias(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                       int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                       double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks,
                       int64_t sink_heads, int64_t d_v, const void* bias, int64_t bias_heads, int64_t bias_batch_stride,
                       int64_t bias_head_stride, int64_t bias_row_stride, const uint8_t* mask, int64_t mask_bh_stride,
                       const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream) {
    ExCall c = ex_call(q, k, v, o, lse, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask, br, bc, dropout_p,
                       dropout_seed, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    c.d_v = d_v;
    c.bi = {bias, bias_heads, bias_batch_stride, bias_head_stride, bias_row_stride, nullptr, 0, 0, 0};
    return ex_forward_impl("fa_ex_forward_bias", c);
}

int fa_ex_backward_bias(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const float* dlse, int64_t d_v, const void* bias, int64_t bias_heads, int64_t bias_batch_stride,
                        int64_t bias_head_stride, int64_t bias_row_stride, void* dbias, int64_t dbias_batch_stride,
                        int64_t dbias_head_stride, int64_t dbias_row_stride, const uint8_t* mask, int64_t mask_bh_stride,
                        const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace,
                        size_t workspace_bytes, void* stream) {
    ExCall c = ex_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, bh, nq, nk, d, dtype, causal, softmax_scale, mask, mask_bh_stride, block_mask,
                           br, bc, dropout_p, dropout_seed, workspace, workspace_bytes, stream);
    c.kv_group = kv_group; c.window_left = window_left; c.window_right = window_right;
    c.sm = {softcap, alibi_slopes, alibi_heads, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    c.dlse = dlse;
    c.d_v = d_v;
    c.bi = {bias, bias_heads, bias_batch_stride, bias_head_stride, bias_row_stride, dbias, dbias_batch_stride, dbias_head_stride,
            dbias_row_stride};
    return ex_backward_impl("fa_ex_backward_bias", c);
}

size_t fa_ex_backward_workspace_bytes_bias(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int dbias_reduced) {
    size_t need = fa_ex_backward_workspace_bytes_grouped(bh, kv_group, nq, nk, d, dtype);
    if (dbias_reduced && bh > 0 && nq > 0 && nk > 0) need += fa::ex_bias_ds_bytes(bh, nq, nk);
    return need;
}

// ---- variable-length (packed) sequences: see include/fa_mi355x.h
// Everything that can be checked without reading cu_seqlens (which would take a synchronise), before any HIP call.
// One call of the fa_ex_*_varlen* family, fa_ex_forward_varlen_paged / _paged_fp8 included.  Defaults: "argument absent"; cache_dtype is the
// exception, an entry point without one sets it to dtype.
struct VarlenCall {
    const void *q = nullptr, *k = nullptr, *v = nullptr, *do_ = nullptr;
    void* o = nullptr;      // (the backward only reads o and lse)
    float* lse = nullptr;
    void *dq = nullptr, *dk = nullptr, *dv = nullptr;
    const int32_t *cu_seqlens_q = nullptr, *cu_seqlens_k = nullptr;
    int64_t batch = 0, heads_q = 0, heads_kv = 0, total_q = 0, total_k = 0, max_seqlen_q = 0, max_seqlen_k = 0, d = 0;
    int64_t q_stride = 0, k_stride = 0, v_stride = 0, window_left = -1, window_right = -1;
    int dtype = 0, causal = 0;
    double softmax_scale = 0.0, dropout_p = 0.0;
    uint64_t dropout_seed = 0;
    ScoreMod sm;            // (heads: heads_q)
    SinkArg sk;
    const float* dlse = nullptr;   // fa_ex_backward_varlen_dlse: the gradient of lse, (heads_q, total_q) float32
    int64_t d_v = 0;               // fa_ex_*_varlen_vdim: the width of v, o, do_ and dv (0: d)
    const int32_t* block_table = nullptr;   // the paged forward, and (cache_dtype, the scales) its e4m3 pool
    int64_t max_blocks_per_seq = 0, num_blocks = 0, page_block_size = 0, k_page_stride = 0, v_page_stride = 0, descale_batch_stride = 0;
    int cache_dtype = 0;
    const float *k_descale = nullptr, *v_descale = nullptr;
    void *workspace = nullptr, *stream = nullptr;
    size_t workspace_bytes = 0;
};

static bool varlen_vdim(const VarlenCall& c) { return c.d_v != 0 && c.d_v != c.d; }
static int varlen_vdim_check(const char* who, const VarlenCall& c) {
    if (!varlen_vdim(c) || c.d <= 0) return FA_OK;
    VdimExtras x;
    x.dropout = c.dropout_p > 0.0; x.window = c.window_left != -1 || c.window_right != -1; x.softcap = c.sm.softcap > 0.0;
    x.alibi = c.sm.alibi != nullptr; x.sinks = c.sk.sinks != nullptr;
    return vdim_check(who, c.d, c.d_v, c.dtype, c.softmax_scale, x);
}

// (total_k: the paged call has no token count and passes 1)
static int varlen_check(const char* who, const VarlenCall& c, int64_t total_k) {
    const int32_t *cu_q = c.cu_seqlens_q, *cu_k = c.cu_seqlens_k;
    const int64_t batch = c.batch, hq = c.heads_q, hkv = c.heads_kv, total_q = c.total_q, max_q = c.max_seqlen_q, max_k = c.max_seqlen_k, d = c.d;
    const int64_t sq = c.q_stride, sk = c.k_stride, sv = c.v_stride, wl = c.window_left, wr = c.window_right;
    const int dtype = c.dtype;
    const double scale = c.softmax_scale, p = c.dropout_p;
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: unknown dtype code %d", who, dtype);
    if (batch < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch must be >= 1 (got %lld)", who, (long long)batch);
    if (hq < 1 || hkv < 1 || hq % hkv != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_q=%lld must be a positive multiple of heads_kv=%lld", who, (long long)hq, (long long)hkv);
    if (d <= 0 || total_q < 0 || total_k < 0 || max_q < 0 || max_k < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: bad shape (d=%lld, total_q=%lld, total_k=%lld, max_seqlen_q=%lld, max_seqlen_k=%lld)", who,
                    (long long)d, (long long)total_q, (long long)total_k, (long long)max_q, (long long)max_k);
    if (sq < hq * d || sk < hkv * d || sv < hkv * (varlen_vdim(c) ? c.d_v : d))   // (a v of its own width: rows of heads_kv * d_v)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: token strides (%lld, %lld, %lld) must be >= heads * d (%lld, %lld)", who, (long long)sq,
                    (long long)sk, (long long)sv, (long long)(hq * d), (long long)(hkv * d));
    if ((total_q > 0 && !cu_q) || (total_k > 0 && !cu_k)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null cu_seqlens", who);
    if (wl < -1 || wr < -1)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: window (%lld, %lld): each bound must be >= 0, or -1 for unbounded", who,
                    (long long)wl, (long long)wr);
    if (!(scale == scale)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale is NaN", who);
    if (!(p >= 0.0 && p < 1.0)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: dropout_p must lie in [0, 1)", who);
    if (batch > ((int64_t)1 << 31) || hq > ((int64_t)1 << 31) || batch * hq * ((max_q + 1) / 2) >= ((int64_t)1 << 32))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch * heads_q * ceil(max_seqlen_q / 2) must stay below 2^32 (dropout counters)", who);
    if (d > 256) return fail(FA_ERR_UNSUPPORTED, "%s: head_dim %lld > 256 is not supported", who, (long long)d);
    const int64_t lim = (int64_t)1 << 31;
    if (max_q > (int64_t)1 << 24 || max_k > (int64_t)1 << 24 || total_q >= lim || total_k >= lim || sq >= lim || sk >= lim || sv >= lim ||
        hq * d >= lim || batch * hq * ((max_q + 15) / 16) >= lim || batch * hq * ((max_k + 15) / 16) >= lim ||
        (total_q + 15) / 16 * hq >= ((int64_t)1 << 32))
        return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    return FA_OK;
}

// (total_k, max_k and the canonical mask: the caller's)
static fa::ExArgs varlen_args(const VarlenCall& c, int64_t total_k, int64_t max_k, int causal, int64_t wl, int64_t wr) {
    fa::ExArgs a{c.q, c.k, c.v, c.o, c.lse, c.do_, c.dq, c.dk, c.dv, c.batch * c.heads_q, c.max_seqlen_q, max_k, c.d, c.dtype,
                 causal ? 1 : 0, (float)c.softmax_scale, nullptr, 0, nullptr, 0, 0, c.dropout_p, c.dropout_seed, c.workspace, c.workspace_bytes};
    a.kv_group = c.heads_q / c.heads_kv;
    a.window_left = wl;
    a.window_right = wr;
    a.cu_q = c.cu_seqlens_q;
    a.cu_k = c.cu_seqlens_k;
    a.heads_q = c.heads_q;
    a.total_q = c.total_q;
    a.total_k = total_k;
    a.stride_q = c.q_stride;
    a.stride_k = c.k_stride;
    a.stride_v = c.v_stride;
    score_args(a, c.sm);
    sink_args(a, c.sk);
    a.dlse = c.dlse;
    a.d_v = varlen_vdim(c) ? c.d_v : 0;
    return a;
}

static int varlen_forward_impl(const char* who, const VarlenCall& c) {
    int causal = c.causal;
    int64_t wl = c.window_left, wr = c.window_right;   // (window_canon rewrites the three)
    int rc = varlen_vdim_check(who, c);
    if (rc != FA_OK) return rc;
    rc = varlen_check(who, c, c.total_k);
    if (rc != FA_OK) return rc;
    if (c.heads_q >= 1 && (rc = score_check(who, c.sm, c.batch * c.heads_q)) != FA_OK) return rc;
    if ((rc = sink_check(who, c.sk, c.heads_q, false)) != FA_OK) return rc;   // (indexed by query head)
    if ((rc = window_canon(who, c.max_seqlen_q, c.max_seqlen_k, causal, wl, wr)) != FA_OK) return rc;
    if (c.total_q == 0 || c.max_seqlen_q == 0) return FA_OK;   // no query row in any sequence
    if (!c.q || !c.o || !c.lse || (c.total_k > 0 && (!c.k || !c.v))) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    if (varlen_vdim(c) && (rc = vdim_layout_check(who, {c.q, c.k, c.v, c.o}, {c.q_stride, c.k_stride, c.v_stride})) != FA_OK) return rc;
    if (c.total_k == 0 || c.max_seqlen_k == 0)   // in any sequence
        return no_key_fill(who, c.o, c.lse, c.heads_q, c.total_q, varlen_vdim(c) ? c.d_v : c.d, c.dtype, c.sk, st);
    fa::ExArgs a = varlen_args(c, c.total_k, c.max_seqlen_k, causal, wl, wr);
    return launched(who, fa::launch_ex(a, false, st));
}

// the leading arguments every forward of the family has
static VarlenCall varlen_call(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                              const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                              int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                              int causal, int64_t window_left, int64_t window_right, double softmax_scale) {
    VarlenCall c;
    c.q = q; c.k = k; c.v = v; c.o = o; c.lse = lse; c.cu_seqlens_q = cu_seqlens_q; c.cu_seqlens_k = cu_seqlens_k;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.total_q = total_q; c.total_k = total_k;
    c.max_seqlen_q = max_seqlen_q; c.max_seqlen_k = max_seqlen_k; c.d = d; c.dtype = dtype; c.cache_dtype = dtype;
    c.q_stride = q_stride; c.k_stride = k_stride; c.v_stride = v_stride;
    c.causal = causal; c.window_left = window_left; c.window_right = window_right; c.softmax_scale = softmax_scale;
    return c;
}
// ... and every backward, with its workspace
static VarlenCall varlen_bwd_call(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                                  void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q,
                                  int64_t heads_kv,
                                  int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype,
                                  int64_t q_stride,
                                  int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                                  double softmax_scale, void* workspace,
                                  size_t workspace_bytes) {
    VarlenCall c = varlen_call(q, k, v, const_cast<void*>(o), const_cast<float*>(lse), cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv,
                               total_q, total_k, max_seqlen_q, max_seqlen_k, d, dtype, q_stride, k_stride, v_stride, causal, window_left,
                               window_right, softmax_scale);
    c.do_ = do_; c.dq = dq; c.dk = dk; c.dv = dv; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return c;
}

int fa_ex_forward_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                         const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                         int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                         int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                         double dropout_p, uint64_t dropout_seed, void* stream) {
    VarlenCall c = varlen_call(q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k,
                               d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right, softmax_scale);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    return varlen_forward_impl("fa_ex_forward_varlen", c);
}

int fa_ex_forward_varlen_scoremod(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                                  const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                                  int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride,
                                  int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                  double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, double dropout_p,
                                  uint64_t dropout_seed, void* stream) {
    VarlenCall c = varlen_call(q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k,
                               d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right, softmax_scale);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    return varlen_forward_impl("fa_ex_forward_varlen_scoremod", c);
}

int fa_ex_forward_varlen_sink(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                              const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                              int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                              int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                              double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks,
                              int64_t sink_heads, double dropout_p, uint64_t dropout_seed, void* stream) {
    VarlenCall c = varlen_call(q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k,
                               d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right, softmax_scale);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    return varlen_forward_impl("fa_ex_forward_varlen_sink", c);
}

size_t fa_ex_backward_workspace_bytes_varlen(int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t d, int dtype) {
    size_t need = fa_ex_backward_workspace_bytes(heads_q, total_q, total_k, d, dtype);   // the row constants, (heads_q, total_q)
    if (heads_kv > 0 && heads_q > heads_kv && total_q > 0 && total_k > 0 && d > 0)
        need += 2 * fa::kv_partial_bytes(total_k * heads_q, 1, d, dtype);              // + the per-query-head dK / dV partials
    return need;
}

static int varlen_backward_impl(const char* who, const VarlenCall& c) {
    int causal = c.causal;
    int64_t wl = c.window_left, wr = c.window_right;   // (window_canon rewrites the three)
    int rc = varlen_vdim_check(who, c);
    if (rc != FA_OK) return rc;
    rc = varlen_check(who, c, c.total_k);
    if (rc != FA_OK) return rc;
    if (c.heads_q >= 1 && (rc = score_check(who, c.sm, c.batch * c.heads_q)) != FA_OK) return rc;
    if ((rc = sink_check(who, c.sk, c.heads_q, true)) != FA_OK) return rc;
    if ((rc = dlse_check(who, c.dlse)) != FA_OK) return rc;
    if ((rc = window_canon(who, c.max_seqlen_q, c.max_seqlen_k, causal, wl, wr)) != FA_OK) return rc;
    const bool no_q = c.total_q == 0 || c.max_seqlen_q == 0, no_k = c.total_k == 0 || c.max_seqlen_k == 0;
    const size_t es = c.dtype == FA_DTYPE_F32 ? 4 : 2;
    if (no_q || no_k) {   // ... in every sequence
        rc = empty_backward(who, no_q && no_k, no_q, c.dq, (size_t)c.total_q * c.heads_q * c.d * es, c.dk, c.dv,
                            (size_t)c.total_k * c.heads_kv * c.d * es, c.sk, reinterpret_cast<hipStream_t>(c.stream),
                            (size_t)c.total_k * c.heads_kv * (varlen_vdim(c) ? c.d_v : c.d) * es);
        if (rc != FA_OK || no_q || !c.sk.sinks || !c.dlse) return rc;
        return no_key_dsinks(who, varlen_args(c, c.total_k, c.max_seqlen_k, causal, wl, wr), reinterpret_cast<hipStream_t>(c.stream));
    }
    if (!c.q || !c.k || !c.v || !c.o || !c.do_ || !c.lse || !c.dq || !c.dk || !c.dv)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (varlen_vdim(c) && (rc = vdim_layout_check(who, {c.q, c.k, c.v, c.o, c.do_, c.dq, c.dk, c.dv}, {c.q_stride, c.k_stride, c.v_stride})) != FA_OK)
        return rc;
    const size_t need = fa_ex_backward_workspace_bytes_varlen(c.heads_q, c.heads_kv, c.total_q, c.total_k, c.d, c.dtype);
    if (!c.workspace || c.workspace_bytes < need)
        return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, c.workspace_bytes);
    fa::ExArgs a = varlen_args(c, c.total_k, c.max_seqlen_k, causal, wl, wr);
    return launched(who, fa::launch_ex(a, true, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_ex_backward_varlen(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                          void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv,
                          int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                          int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                          double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    VarlenCall c = varlen_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k,
                                   max_seqlen_q, max_seqlen_k, d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right,
                                   softmax_scale, workspace, workspace_bytes);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    return varlen_backward_impl("fa_ex_backward_varlen", c);
}

int fa_ex_backward_varlen_scoremod(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                                   void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q,
                                   int64_t heads_kv,
                                   int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype,
                                   int64_t q_stride,
                                   int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                   double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, double dropout_p,
                                   uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream) {
    VarlenCall c = varlen_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k,
                                   max_seqlen_q, max_seqlen_k, d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right,
                                   softmax_scale, workspace, workspace_bytes);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    return varlen_backward_impl("fa_ex_backward_varlen_scoremod", c);
}

int fa_ex_backward_varlen_sink(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                               void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv,
                               int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                               int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                               double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks,
                               int64_t sink_heads, float* dsinks, double dropout_p, uint64_t dropout_seed, void* workspace,
                               size_t workspace_bytes, void* stream) {
    VarlenCall c = varlen_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k,
                                   max_seqlen_q, max_seqlen_k, d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right,
                                   softmax_scale, workspace, workspace_bytes);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    return varlen_backward_impl("fa_ex_backward_varlen_sink", c);
}

int fa_ex_backward_varlen_dlse(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                               void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv,
                               int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                               int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                               double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks,
                               int64_t sink_heads, float* dsinks, const float* dlse, double dropout_p, uint64_t dropout_seed, void* workspace,
                               size_t workspace_bytes, void* stream) {
    VarlenCall c = varlen_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k,
                                   max_seqlen_q, max_seqlen_k, d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right,
                                   softmax_scale, workspace, workspace_bytes);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    c.dlse = dlse;
    return varlen_backward_impl("fa_ex_backward_varlen_dlse", c);
}

int fa_ex_forward_varlen_vdim(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                              const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                              int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                              int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                              double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks,
                              int64_t sink_heads, int64_t d_v, double dropout_p, uint64_t dropout_seed, void* stream) {
    VarlenCall c = varlen_call(q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k,
                               d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right, softmax_scale);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    c.d_v = d_v;
    return varlen_forward_impl("fa_ex_forward_varlen_vdim", c);
}

int fa_ex_backward_varlen_vdim(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                               void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv,
                               int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                               int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                               double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks,
                               int64_t sink_heads, float* dsinks, const float* dlse, int64_t d_v, double dropout_p, uint64_t dropout_seed,
                               void* workspace, size_t workspace_bytes, void* stream) {
    VarlenCall c = varlen_bwd_call(q, k, v, o, do_, lse, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k,
                                   max_seqlen_q, max_seqlen_k, d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right,
                                   softmax_scale, workspace, workspace_bytes);
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed; c.stream = stream;
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, dsinks};
    c.dlse = dlse;
    c.d_v = d_v;
    return varlen_backward_impl("fa_ex_backward_varlen_vdim", c);
}

// ---- the varlen forward over a paged K/V cache: see include/fa_mi355x.h
// One body under both entry points: fa_ex_forward_varlen_paged leaves cache_dtype = dtype and the scales absent, so none of the e4m3
// checks below can fire and the launch is the one it was.
static int varlen_paged_impl(const char* who, const VarlenCall& c) {
    int causal = c.causal;
    int64_t wl = c.window_left, wr = c.window_right;   // (window_canon rewrites the three)
    // (a pool has no token count: total_k is not read, the keys of a sequence are found through the table)
    // the pool's element type: q's, or e4m3 with a dequantisation scale per (sequence, K/V head): the checks of fa_ex_forward_kvcache_fp8
    const bool e4m3 = c.cache_dtype == FA_DTYPE_E4M3;
    if (c.cache_dtype != c.dtype && !e4m3)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_dtype must be dtype (code %d) or FA_DTYPE_E4M3 (got code %d)", who, c.dtype,
                    c.cache_dtype);
    if (e4m3 && c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype must be f16 or bf16 with an e4m3 pool (got code %d)", who, c.dtype);
    if (!e4m3 && (c.k_descale || c.v_descale))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_descale / v_descale need an e4m3 pool (cache_dtype is code %d)", who, c.cache_dtype);
    if (!e4m3 && c.descale_batch_stride != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale_batch_stride must be 0 with a 16-bit pool (got %lld)", who,
                    (long long)c.descale_batch_stride);
    if (c.descale_batch_stride < 0 || (c.descale_batch_stride != 0 && (c.descale_batch_stride < c.heads_kv ||
        c.descale_batch_stride > ((int64_t)1 << 40))))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale_batch_stride=%lld must be 0 or >= heads_kv=%lld (and <= 2^40)", who,
                    (long long)c.descale_batch_stride, (long long)c.heads_kv);
    if ((uintptr_t)c.k_descale % 4 != 0 || (uintptr_t)c.v_descale % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_descale and v_descale must be 4-byte aligned", who);
    if (e4m3) {   // an 8-element chunk of an e4m3 pool is 8 bytes: loads of 4 and 8 bytes
        if (c.d < 8 || c.d % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: head_dim must be a multiple of 8 with an e4m3 pool (got %lld)", who, (long long)c.d);
        if ((uintptr_t)c.k % 8 != 0 || (uintptr_t)c.v % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: an e4m3 k / v pool must be 8-byte aligned", who);
        if (c.k_stride % 8 != 0 || c.v_stride % 8 != 0 || c.k_page_stride % 8 != 0 || c.v_page_stride % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of an e4m3 pool must be multiples of 8 elements", who);
    }
    if (!c.block_table) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null block_table", who);
    if ((uintptr_t)c.block_table % 4 != 0 || (uintptr_t)c.cu_seqlens_k % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table and cu_seqlens_k must be 4-byte aligned", who);
    if (c.page_block_size < 16 || c.page_block_size % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: page_block_size must be a positive multiple of 16 (got %lld)", who, (long long)c.page_block_size);
    if (c.num_blocks < 0 || c.max_blocks_per_seq < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_blocks=%lld and max_blocks_per_seq=%lld must be >= 0", who, (long long)c.num_blocks,
                    (long long)c.max_blocks_per_seq);
    // (the token strides against heads_kv * d, cu_seqlens_k against null with a key to read: total_k stands in as 1)
    int rc = varlen_check(who, c, 1);
    if (rc != FA_OK) return rc;
    const int64_t page_span = (c.page_block_size - 1) * (c.k_stride > c.v_stride ? c.k_stride : c.v_stride) + c.heads_kv * c.d;
    if (c.num_blocks > 1 && (c.k_page_stride < (c.page_block_size - 1) * c.k_stride + c.heads_kv * c.d ||
                           c.v_page_stride < (c.page_block_size - 1) * c.v_stride + c.heads_kv * c.d))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: page strides (%lld, %lld) must span a page of %lld tokens at token strides (%lld, %lld)",
                    who, (long long)c.k_page_stride, (long long)c.v_page_stride, (long long)c.page_block_size, (long long)c.k_stride,
                    (long long)c.v_stride);
    if (c.k_page_stride < 0 || c.v_page_stride < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: page strides must be >= 0", who);
    if ((rc = score_check(who, c.sm, c.batch * c.heads_q)) != FA_OK) return rc;
    if ((rc = sink_check(who, c.sk, c.heads_q, false)) != FA_OK) return rc;
    if (c.page_block_size > 65536 || page_span * (e4m3 ? 1 : c.dtype == FA_DTYPE_F32 ? 4 : 2) >= ((int64_t)1 << 31) ||
        c.num_blocks >= ((int64_t)1 << 31) ||
        c.max_blocks_per_seq >= ((int64_t)1 << 31) || c.batch * c.max_blocks_per_seq >= ((int64_t)1 << 40))
        return fail(FA_ERR_UNSUPPORTED, "%s: a page above 65536 tokens or 2^31 bytes, or a table too large", who);
    // the window against the same (max_seqlen_q, max_seqlen_k) as the packed call on the gathered tokens
    if ((rc = window_canon(who, c.max_seqlen_q, c.max_seqlen_k, causal, wl, wr)) != FA_OK) return rc;
    if (c.total_q == 0 || c.max_seqlen_q == 0) return FA_OK;
    const int64_t capacity = c.max_blocks_per_seq * c.page_block_size;
    const int64_t cap = c.max_seqlen_k < capacity ? c.max_seqlen_k : capacity;   // a sequence's keys: [0, cap]
    if (!c.q || !c.o || !c.lse || (cap > 0 && c.num_blocks > 0 && (!c.k || !c.v)))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    if (cap == 0) return no_key_fill(who, c.o, c.lse, c.heads_q, c.total_q, c.d, c.dtype, c.sk, st);   // in any sequence, as the packed call
    fa::ExArgs a = varlen_args(c, 0, cap, causal, wl, wr);
    a.block_table = c.block_table;
    a.max_blocks = c.max_blocks_per_seq;
    a.num_blocks = c.num_blocks;
    a.page_size = c.page_block_size;
    a.page_stride_k = c.k_page_stride;
    a.page_stride_v = c.v_page_stride;
    a.kv_e4m3 = e4m3 ? 1 : 0; a.k_descale = c.k_descale; a.v_descale = c.v_descale; a.descale_bstride = c.descale_batch_stride;
    return launched(who, fa::launch_ex(a, false, st));
}

int fa_ex_forward_varlen_paged(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                               const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                               int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                               double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads,
                               const int32_t* block_table, int64_t max_blocks_per_seq,
                               int64_t num_blocks, int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride, void* stream) {
    VarlenCall c = varlen_call(q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k,
                               d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right, softmax_scale);
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    c.block_table = block_table; c.max_blocks_per_seq = max_blocks_per_seq; c.num_blocks = num_blocks; c.page_block_size = page_block_size;
    c.k_page_stride = k_page_stride; c.v_page_stride = v_page_stride; c.stream = stream;
    return varlen_paged_impl("fa_ex_forward_varlen_paged", c);
}

int fa_ex_forward_varlen_paged_fp8(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                                   const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k,
                                   int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride,
                                   int64_t v_stride,
                                   int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                   double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads,
                                   const int32_t* block_table, int64_t max_blocks_per_seq,
                                   int64_t num_blocks, int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride, int cache_dtype,
                                   const float* k_descale, const float* v_descale, int64_t descale_batch_stride, void* stream) {
    VarlenCall c = varlen_call(q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k,
                               d, dtype, q_stride, k_stride, v_stride, causal, window_left, window_right, softmax_scale);
    c.sm = {softcap, alibi_slopes, heads_q, alibi_batch_stride};
    c.sk = {sinks, sink_heads, nullptr};
    c.block_table = block_table; c.max_blocks_per_seq = max_blocks_per_seq; c.num_blocks = num_blocks; c.page_block_size = page_block_size;
    c.k_page_stride = k_page_stride; c.v_page_stride = v_page_stride; c.stream = stream;
    c.cache_dtype = cache_dtype; c.k_descale = k_descale; c.v_descale = v_descale; c.descale_batch_stride = descale_batch_stride;
    return varlen_paged_impl("fa_ex_forward_varlen_paged_fp8", c);
}

// ---- KV-cache decoding with split-KV: see include/fa_mi355x.h
static int64_t kv_splits(int64_t batch, int64_t hq, int64_t hkv, int64_t nq, int64_t cache_len, int64_t num_splits) {
    if (num_splits > 0) return num_splits;
    return fa::kv_num_splits(batch, hkv, ((hq / hkv) * nq + 15) / 16, cache_len);
}

// the same for a call with qv (fa_mla.hip: workgroups of up to four row tiles)
static int64_t kv_splits_qv(int64_t batch, int64_t hq, int64_t hkv, int64_t nq, int64_t cache_len, int64_t num_splits) {
    if (num_splits > 0) return num_splits;
    return fa::mla_num_splits(batch, hkv, (hq / hkv) * nq, cache_len);
}

// the arguments of the three workspace queries (seqlen_q: max_seqlen_q of the packed one); a bad one makes the answer 0
static bool kv_ws_args_ok(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t d, int64_t num_splits) {
    return batch > 0 && heads_q > 0 && heads_kv > 0 && heads_q % heads_kv == 0 && seqlen_q > 0 && d > 0 && cache_len >= 0 && num_splits >= 0 &&
           num_splits <= 256;
}

size_t fa_ex_kvcache_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t d,
                                     int64_t num_splits) {
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits)) return 0;
    return fa::kv_workspace_bytes(batch, heads_q, seqlen_q, d, (int)kv_splits(batch, heads_q, heads_kv, seqlen_q, cache_len, num_splits));
}

// a sink call always runs the combine: at least two splits
size_t fa_ex_kvcache_workspace_bytes_sink(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t d,
                                          int64_t num_splits) {
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits)) return 0;
    const int64_t S = kv_splits(batch, heads_q, heads_kv, seqlen_q, cache_len, num_splits);
    return fa::kv_workspace_bytes(batch, heads_q, seqlen_q, d, (int)(S < 2 ? 2 : S));
}

// packed queries: S from max_seqlen_q's row tiles (shapes only), partials for total_q tokens; with_sinks: at least two splits
size_t fa_ex_kvcache_workspace_bytes_varlen(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q,
                                            int64_t cache_len, int64_t d, int64_t num_splits, int with_sinks) {
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, max_seqlen_q, cache_len, d, num_splits) || max_seqlen_q > total_q) return 0;
    const int64_t S = kv_splits(batch, heads_q, heads_kv, max_seqlen_q, cache_len, num_splits);
    return fa::kv_workspace_bytes(1, heads_q, total_q, d, (int)(with_sinks && S < 2 ? 2 : S));
}

// d_v = 0: fa_ex_kvcache_workspace_bytes_varlen.  d_v > 0 (a call with qv): o and the partials are d_v wide and S follows the
// launch rule of that kernel
size_t fa_ex_kvcache_workspace_bytes_qv(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q,
                                        int64_t cache_len, int64_t d, int64_t num_splits, int with_sinks, int64_t d_v) {
    if (d_v == 0) return fa_ex_kvcache_workspace_bytes_varlen(batch, heads_q, heads_kv, total_q, max_seqlen_q, cache_len, d, num_splits, with_sinks);
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, max_seqlen_q, cache_len, d, num_splits) || max_seqlen_q > total_q || d_v < 0) return 0;
    const int64_t S = kv_splits_qv(batch, heads_q, heads_kv, max_seqlen_q, cache_len, num_splits);
    return fa::kv_workspace_bytes(1, heads_q, total_q, d_v, (int)(with_sinks && S < 2 ? 2 : S));
}

// One call of the fa_ex_forward_kvcache* family, a field per argument of the widest entry point under its name in the header.
// Defaults: "argument absent", which is 0 / null but for sink_heads (1) and cache_dtype (kv_call sets it to dtype).
struct KvCall {
    const void *q = nullptr, *k_new = nullptr, *v_new = nullptr;
    void *k_cache = nullptr, *v_cache = nullptr, *o = nullptr;
    const int32_t* cache_seqlens = nullptr;
    float* lse = nullptr;
    int64_t batch = 0, heads_q = 0, heads_kv = 0, seqlen_q = 0, seqlen_new = 0, cache_len = 0, d = 0;
    int64_t q_batch_stride = 0, q_token_stride = 0, k_cache_batch_stride = 0, k_cache_token_stride = 0, v_cache_batch_stride = 0,
            v_cache_token_stride = 0, k_new_batch_stride = 0, k_new_token_stride = 0, v_new_batch_stride = 0, v_new_token_stride = 0;
    int dtype = 0, causal = 0;
    int64_t window_left = -1, window_right = -1, alibi_batch_stride = 0, num_splits = 0;
    double softmax_scale = 0.0, softcap = 0.0;
    const float* alibi_slopes = nullptr;
    void *workspace = nullptr, *stream = nullptr;
    size_t workspace_bytes = 0;
    // fa_ex_forward_kvcache_paged adds
    const int32_t *block_table = nullptr, *cache_batch_idx = nullptr, *cache_leftpad = nullptr;
    int64_t block_table_row_stride = 0, num_blocks = 0, page_block_size = 0, max_blocks_per_seq = 0, cache_batch = 0;
    // _rotary
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;
    int64_t rotary_cos_row_stride = 0, rotary_sin_row_stride = 0, seqlen_ro = 0, rotary_dim = 0;
    int rotary_interleaved = 0;
    // _fp8
    int cache_dtype = 0;
    const float *k_descale = nullptr, *v_descale = nullptr;
    int64_t descale_batch_stride = 0;
    // _sink
    const float* sinks = nullptr;
    int64_t sink_heads = 1;
    // _varlen
    const int32_t *cu_seqlens_q = nullptr, *cu_seqlens_k_new = nullptr;
    int64_t total_q = 0, max_seqlen_q = 0, total_k_new = 0;
    // _qv
    const void* qv = nullptr;
    int64_t qv_batch_stride = 0, qv_token_stride = 0, d_v = 0;
};

static int kvcache_impl(const char* who, const KvCall& c) {
    // what the packed and the paged forms, and the canonical window, overwrite below
    int64_t seqlen_q = c.seqlen_q, seqlen_new = c.seqlen_new, cache_len = c.cache_len, window_left = c.window_left, window_right = c.window_right;
    int64_t q_batch_stride = c.q_batch_stride, k_new_batch_stride = c.k_new_batch_stride, v_new_batch_stride = c.v_new_batch_stride;
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype must be f16 or bf16 (got code %d)", who, c.dtype);
    // the cache's element type: q's, or e4m3 with a dequantisation scale per (sequence, K/V head)
    if (c.cache_dtype != c.dtype && c.cache_dtype != FA_DTYPE_E4M3)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_dtype must be dtype (code %d) or FA_DTYPE_E4M3 (got code %d)", who, c.dtype,
                    c.cache_dtype);
    const bool e4m3 = c.cache_dtype == FA_DTYPE_E4M3;
    if (!e4m3 && (c.k_descale || c.v_descale))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_descale / v_descale need an e4m3 cache (cache_dtype is code %d)", who, c.cache_dtype);
    if (!e4m3 && c.descale_batch_stride != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale_batch_stride must be 0 with a 16-bit cache (got %lld)", who,
                    (long long)c.descale_batch_stride);
    if (c.descale_batch_stride < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale_batch_stride must be >= 0 (got %lld)", who, (long long)c.descale_batch_stride);
    if ((uintptr_t)c.k_descale % 4 != 0 || (uintptr_t)c.v_descale % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_descale and v_descale must be 4-byte aligned", who);
    if (c.d < 8 || c.d > 256 || c.d % 8 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: head_dim must be a multiple of 8 in [8, 256] (got %lld)", who, (long long)c.d);
    if (c.batch < 1 || c.batch > 65535) return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch must lie in [1, 65535] (got %lld)", who, (long long)c.batch);
    if (c.heads_kv < 1 || c.heads_q < 1 || c.heads_q % c.heads_kv != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_q=%lld must be a positive multiple of heads_kv=%lld", who, (long long)c.heads_q,
                    (long long)c.heads_kv);
    // packed queries / new keys: from here on seqlen_q stands for max_seqlen_q, the bound on every sequence's tokens (the grid,
    // the split rule and the window take it), and q is one unit of tokens at q_token_stride
    const bool vq = c.cu_seqlens_q != nullptr, vk = c.cu_seqlens_k_new != nullptr;
    if (!vq && (c.total_q != 0 || c.max_seqlen_q != 0))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_q and max_seqlen_q must be 0 without cu_seqlens_q (got %lld, %lld)", who,
                    (long long)c.total_q, (long long)c.max_seqlen_q);
    if (!vk && c.total_k_new != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_k_new must be 0 without cu_seqlens_k_new (got %lld)", who, (long long)c.total_k_new);
    if (vk && !vq) return fail(FA_ERR_INVALID_ARGUMENT, "%s: cu_seqlens_k_new needs cu_seqlens_q", who);
    if (vk && (!c.k_new || !c.v_new)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: cu_seqlens_k_new needs k_new and v_new", who);
    if ((uintptr_t)c.cu_seqlens_q % 4 != 0 || (uintptr_t)c.cu_seqlens_k_new % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cu_seqlens_q and cu_seqlens_k_new must be 4-byte aligned", who);
    if (vq) {
        if (c.total_q < 0 || c.total_q > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_q must lie in [0, 2^31) (got %lld)", who, (long long)c.total_q);
        if (c.max_seqlen_q < 0 || c.max_seqlen_q > c.total_q)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_seqlen_q=%lld must lie in [0, total_q=%lld]", who, (long long)c.max_seqlen_q,
                        (long long)c.total_q);
        seqlen_q = c.max_seqlen_q;
        q_batch_stride = 0;
    } else if (seqlen_q < 1) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_q must be >= 1 (got %lld)", who, (long long)seqlen_q);
    }
    if (vk && (c.total_k_new < 0 || c.total_k_new > 0x7fffffff))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_k_new must lie in [0, 2^31) (got %lld)", who, (long long)c.total_k_new);
    // attention sinks: head h of every sequence takes sinks[h % sink_heads]
    if (const int rc = sink_check(who, SinkArg{c.sinks, c.sink_heads, nullptr}, c.heads_q, false); rc != FA_OK) return rc;
    if (c.descale_batch_stride != 0 && (c.descale_batch_stride < c.heads_kv || c.descale_batch_stride > ((int64_t)1 << 40)))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale_batch_stride=%lld must be 0 or >= heads_kv=%lld (and <= 2^40)", who,
                    (long long)c.descale_batch_stride, (long long)c.heads_kv);
    // the paged cache and the two per-sequence cache selectors
    if (c.block_table) {
        if (c.cache_batch_idx || c.cache_leftpad)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table cannot be combined with cache_batch_idx or cache_leftpad", who);
        if (c.page_block_size < 16 || c.page_block_size % 16 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: page_block_size must be a positive multiple of 16 (got %lld)", who,
                        (long long)c.page_block_size);
        if (c.num_blocks < 1 || c.num_blocks > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_blocks must lie in [1, 2^31) (got %lld)", who, (long long)c.num_blocks);
        if (c.max_blocks_per_seq < 1)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_blocks_per_seq must be >= 1 (got %lld)", who, (long long)c.max_blocks_per_seq);
        if (c.max_blocks_per_seq > ((int64_t)1 << 28) / c.page_block_size)
            return fail(FA_ERR_UNSUPPORTED, "%s: capacity max_blocks_per_seq * page_block_size = %lld * %lld is beyond 2^28 tokens", who,
                        (long long)c.max_blocks_per_seq, (long long)c.page_block_size);
        if ((uintptr_t)c.block_table % 4 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table must be 4-byte aligned", who);
        if (c.block_table_row_stride < c.max_blocks_per_seq || c.block_table_row_stride > ((int64_t)1 << 40))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table_row_stride=%lld must be >= max_blocks_per_seq=%lld (and <= 2^40)", who,
                        (long long)c.block_table_row_stride, (long long)c.max_blocks_per_seq);
        cache_len = c.max_blocks_per_seq * c.page_block_size;   // the capacity: it stands for cache_len from here on
    } else if (c.block_table_row_stride != 0 || c.num_blocks != 0 || c.page_block_size != 0 || c.max_blocks_per_seq != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT,
                    "%s: block_table_row_stride, num_blocks, page_block_size and max_blocks_per_seq must be 0 without block_table", who);
    }
    if (c.cache_batch_idx) {
        if (c.cache_batch < 1 || c.cache_batch > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch must lie in [1, 2^31) with cache_batch_idx (got %lld)", who,
                        (long long)c.cache_batch);
    } else if (c.cache_batch != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch must be 0 without cache_batch_idx (got %lld)", who, (long long)c.cache_batch);
    }
    if ((uintptr_t)c.cache_batch_idx % 4 != 0 || (uintptr_t)c.cache_leftpad % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch_idx and cache_leftpad must be 4-byte aligned", who);
    if (cache_len < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_len must be >= 1 (got %lld)", who, (long long)cache_len);
    if (vk) {   // seqlen_new stands for the most tokens one sequence can append (the device clamps nnew_b to it)
        seqlen_new = c.total_k_new < cache_len ? c.total_k_new : cache_len;
        k_new_batch_stride = v_new_batch_stride = 0;
    }
    if (seqlen_new < 0 || seqlen_new > cache_len)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_new=%lld must lie in [0, cache_len=%lld]", who, (long long)seqlen_new,
                    (long long)cache_len);
    // strides: the heads of a token adjacent at stride d, tokens at >= heads * d, batch elements past the last token's heads
    // (a cache's units: its num_blocks pages of page_block_size tokens, its cache_batch rows, or its batch rows)
    const int64_t c_n = c.block_table ? c.page_block_size : cache_len;
    const int64_t c_units = c.block_table ? c.num_blocks : c.cache_batch_idx ? c.cache_batch : c.batch;
    // (esz: bytes an element.  The kernels keep 32-bit byte offsets inside one batch element or page, so the limit is on bytes:
    // an e4m3 cache may hold twice the tokens of a 16-bit one)
    const int64_t c_esz = e4m3 ? 1 : 2;
    // (w: a head's width.  With qv, v_cache and o are d_v wide; the checks of qv's own group follow the existing ones below)
    const int64_t d_o = (c.qv && c.d_v > 0) ? c.d_v : c.d;
    struct { const char* name; int64_t bs, ts, n, heads, units, esz, w; } st[5] = {
        {"q", q_batch_stride, c.q_token_stride, seqlen_q, c.heads_q, vq ? 1 : c.batch, 2, c.d},
        {"k_cache", c.k_cache_batch_stride, c.k_cache_token_stride, c_n, c.heads_kv, c_units, c_esz, c.d},
        {"v_cache", c.v_cache_batch_stride, c.v_cache_token_stride, c_n, c.heads_kv, c_units, c_esz, d_o},
        {"k_new", k_new_batch_stride, c.k_new_token_stride, seqlen_new, c.heads_kv, vk ? 1 : c.batch, 2, c.d},
        {"v_new", v_new_batch_stride, c.v_new_token_stride, seqlen_new, c.heads_kv, vk ? 1 : c.batch, 2, c.d}};
    for (int i = 0; i < (seqlen_new > 0 ? 5 : 3); ++i) {
        const int64_t span = (st[i].n - 1) * st[i].ts + st[i].heads * st[i].w;   // elements of one batch element (or page)
        if (st[i].ts < st[i].heads * st[i].w || (st[i].units > 1 && st[i].bs < span) || st[i].bs < 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)",
                        who, st[i].name, (long long)st[i].bs, (long long)st[i].ts, (long long)(st[i].heads * st[i].w), (long long)span);
        if (st[i].ts % 8 != 0 || st[i].bs % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s must be multiples of 8 elements", who, st[i].name);
        if (span * st[i].esz >= ((int64_t)1 << 31))
            return fail(FA_ERR_UNSUPPORTED, "%s: one batch element of %s spans %lld bytes, beyond 32-bit offsets", who, st[i].name,
                        (long long)(span * st[i].esz));
    }
    if (seqlen_new > 0 && (!c.cache_seqlens || !c.k_new || !c.v_new))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_new > 0 needs cache_seqlens, k_new and v_new", who);
    if (window_left < -1 || window_right < -1)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: window (%lld, %lld): each bound must be >= 0, or -1 for unbounded", who,
                    (long long)window_left, (long long)window_right);
    // rotary embedding: the tables are read on the device without a check, so every position a clamped length can give
    // (new key n at L_b - P_b + n, q token i at L_b - P_b + i, L_b <= cache_len - seqlen_new) must be a table row
    if ((c.rotary_cos != nullptr) != (c.rotary_sin != nullptr))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must be given together", who);
    if (c.rotary_cos) {
        if (c.rotary_dim < 16 || c.rotary_dim > c.d || c.rotary_dim % 16 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_dim must be a multiple of 16 in [16, head_dim=%lld] (got %lld)", who,
                        (long long)c.d, (long long)c.rotary_dim);
        if (seqlen_new < 1 || !c.cache_seqlens)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary needs seqlen_new > 0 (k_new, v_new) and cache_seqlens", who);
        // (packed queries: nq_b - nnew_b is not known here; nq_b <= max_seqlen_q)
        const int64_t ro_need = cache_len + (vq ? c.max_seqlen_q : seqlen_q > seqlen_new ? seqlen_q - seqlen_new : 0);
        if (c.seqlen_ro < ro_need)
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: seqlen_ro=%lld must be >= capacity + %s = %lld (the tables are not bounds-checked on the device)", who,
                        (long long)c.seqlen_ro, vq ? "max_seqlen_q" : "max(0, seqlen_q - seqlen_new)", (long long)ro_need);
        if (c.rotary_cos_row_stride < c.rotary_dim / 2 || c.rotary_sin_row_stride < c.rotary_dim / 2 ||
            c.rotary_cos_row_stride > ((int64_t)1 << 40) || c.rotary_sin_row_stride > ((int64_t)1 << 40))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be >= rotary_dim / 2 = %lld (and <= 2^40)", who,
                        (long long)c.rotary_cos_row_stride, (long long)c.rotary_sin_row_stride, (long long)(c.rotary_dim / 2));
        if (c.rotary_cos_row_stride % 2 != 0 || c.rotary_sin_row_stride % 2 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be even", who,
                        (long long)c.rotary_cos_row_stride, (long long)c.rotary_sin_row_stride);
        if ((uintptr_t)c.rotary_cos % 4 != 0 || (uintptr_t)c.rotary_sin % 4 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must be 4-byte aligned", who);
    } else if (c.rotary_cos_row_stride != 0 || c.rotary_sin_row_stride != 0 || c.seqlen_ro != 0 || c.rotary_dim != 0 || c.rotary_interleaved != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT,
                    "%s: the rotary row strides, seqlen_ro, rotary_dim and rotary_interleaved must be 0 without rotary_cos / rotary_sin", who);
    }
    // q token i is rotated at its own position when causal or a window bound was given: decided here, on the arguments as
    // passed, before the window is canonicalised
    const int rotary_q_per_token = (c.causal || window_left >= 0 || window_right >= 0) ? 1 : 0;
    if (!(c.softmax_scale == c.softmax_scale) || c.softmax_scale - c.softmax_scale != 0.0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be finite (got %g)", who, c.softmax_scale);
    if (!scale_ok(c.softmax_scale))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be > 0 (got %g)", who, c.softmax_scale);
    if (!(c.softcap >= 0.0) || c.softcap > 1.7976931348623157e308)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softcap must be a finite number >= 0 (got %g)", who, c.softcap);
    if (c.alibi_batch_stride < 0 || c.alibi_batch_stride >= ((int64_t)1 << 31) / c.batch)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: alibi_batch_stride must be >= 0 and batch * stride < 2^31 (got %lld)", who,
                    (long long)c.alibi_batch_stride);
    if (c.num_splits < 0 || c.num_splits > 256)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_splits must lie in [0, 256] (got %lld)", who, (long long)c.num_splits);
    if (cache_len > ((int64_t)1 << 28) || seqlen_q > ((int64_t)1 << 24) || c.heads_q > 65535 ||
        ((c.heads_q / c.heads_kv) * seqlen_q + 15) / 16 * c.heads_kv > 65535)
        return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    int64_t S = c.qv ? kv_splits_qv(c.batch, c.heads_q, c.heads_kv, seqlen_q, cache_len, c.num_splits)
                     : kv_splits(c.batch, c.heads_q, c.heads_kv, seqlen_q, cache_len, c.num_splits);
    if (c.sinks && S < 2) S = 2;   // the sink joins in the combine: where the rule or the caller gives one split, two are launched
    const int64_t q_rows = vq ? c.heads_q * c.total_q : c.batch * c.heads_q * seqlen_q;
    if (S > 1 && q_rows >= ((int64_t)1 << 26))   // the combine: one wave per row, 2^32 lanes per launch
        return fail(FA_ERR_UNSUPPORTED, "%s: %s = %lld rows are too many to combine %lld splits in one launch", who,
                    vq ? "heads_q * total_q" : "batch * heads_q * seqlen_q", (long long)q_rows, (long long)S);
    // Canonical window: a bound that cuts no key in any row is -1 (len_k <= cache_len: key 0 is in every row's band once
    // window_left >= cache_len - 1, key len_k - 1 once window_right >= seqlen_q - 1), so the bounds the kernels take in int
    // stay below 2^28 and the band arithmetic cannot overflow.
    if (window_left >= cache_len - 1) window_left = -1;
    if (window_right >= seqlen_q - 1) window_right = -1;
    const size_t need = vq ? (seqlen_q > 0 ? fa::kv_workspace_bytes(1, c.heads_q, c.total_q, d_o, (int)S) : 0)
                           : fa::kv_workspace_bytes(c.batch, c.heads_q, seqlen_q, d_o, (int)S);
    if (c.workspace_bytes < need || (need > 0 && !c.workspace))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace of %zu bytes needed, %zu given", who, need, c.workspace_bytes);
    // (packed queries without a token: q, o and lse are empty and may be null)
    if (!c.k_cache || !c.v_cache || ((!c.q || !c.o || !c.lse) && !(vq && c.total_q == 0)))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (e4m3) {   // an 8-element chunk of an e4m3 cache is 8 bytes: one load or store of 8 bytes, 8-byte aligned
        if ((uintptr_t)c.k_cache % 8 != 0 || (uintptr_t)c.v_cache % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: an e4m3 k_cache / v_cache must be 8-byte aligned", who);
        if (!aligned16({c.q, c.o, c.workspace}) || (seqlen_new > 0 && !aligned16({c.k_new, c.v_new})))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: tensors must be 16-byte aligned", who);
    } else if (!aligned16({c.q, c.k_cache, c.v_cache, c.o, c.workspace}) || (seqlen_new > 0 && !aligned16({c.k_new, c.v_new})))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: tensors must be 16-byte aligned", who);
    // qv (fa_ex_forward_kvcache_qv): a second query operand against v_cache, K and V of different widths
    if (!c.qv && (c.qv_batch_stride != 0 || c.qv_token_stride != 0 || c.d_v != 0))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: qv_batch_stride, qv_token_stride and d_v must be 0 without qv (got %lld, %lld, %lld)", who,
                    (long long)c.qv_batch_stride, (long long)c.qv_token_stride, (long long)c.d_v);
    if (c.qv) {
        if (c.d != 64 || c.d_v != 512)
            return fail(FA_ERR_UNSUPPORTED, "%s: qv is supported for head_dim = 64 with d_v = 512 only (got head_dim = %lld, d_v = %lld)", who,
                        (long long)c.d, (long long)c.d_v);
        const char* with = seqlen_new > 0 || c.k_new || c.v_new ? "k_new / v_new (new tokens to append)"
                           : vk ? "cu_seqlens_k_new"
                           : c.rotary_cos ? "rotary_cos / rotary_sin"
                           : e4m3 ? "an e4m3 cache (cache_dtype, k_descale, v_descale)"
                           : c.softcap > 0.0 ? "softcap"
                           : c.alibi_slopes ? "alibi_slopes"
                           : c.sinks ? "sinks"
                           : vq ? "cu_seqlens_q"
                           : c.cache_leftpad ? "cache_leftpad" : nullptr;
        if (with) return fail(FA_ERR_UNSUPPORTED, "%s: qv cannot be combined with %s", who, with);
        const int64_t span = (seqlen_q - 1) * c.qv_token_stride + c.heads_q * c.d_v;
        if (c.qv_token_stride < c.heads_q * c.d_v || (c.batch > 1 && c.qv_batch_stride < span) || c.qv_batch_stride < 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of qv too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)",
                        who, (long long)c.qv_batch_stride, (long long)c.qv_token_stride, (long long)(c.heads_q * c.d_v), (long long)span);
        if (c.qv_token_stride % 8 != 0 || c.qv_batch_stride % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of qv must be multiples of 8 elements", who);
        if (span * 2 >= ((int64_t)1 << 31))
            return fail(FA_ERR_UNSUPPORTED, "%s: one batch element of qv spans %lld bytes, beyond 32-bit offsets", who, (long long)(span * 2));
        if (!aligned16({c.qv})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: tensors must be 16-byte aligned", who);
    }
    fa::KvArgs a{};
    a.q = c.q; a.k_cache = c.k_cache; a.v_cache = c.v_cache; a.k_new = c.k_new; a.v_new = c.v_new; a.o = c.o; a.lse = c.lse;
    a.cache_seqlens = c.cache_seqlens;
    a.block_table = c.block_table; a.cache_batch_idx = c.cache_batch_idx; a.cache_leftpad = c.cache_leftpad;
    a.table_row_stride = c.block_table_row_stride; a.num_blocks = c.num_blocks; a.page_size = c.page_block_size; a.cache_batch = c.cache_batch;
    a.batch = c.batch; a.heads_q = c.heads_q; a.heads_kv = c.heads_kv; a.seqlen_q = seqlen_q; a.seqlen_new = seqlen_new;
    a.cache_len = cache_len; a.d = c.d; a.dtype = c.dtype; a.causal = c.causal ? 1 : 0;
    a.q_bs = q_batch_stride; a.q_ts = c.q_token_stride; a.kc_bs = c.k_cache_batch_stride; a.kc_ts = c.k_cache_token_stride;
    a.vc_bs = c.v_cache_batch_stride; a.vc_ts = c.v_cache_token_stride; a.kn_bs = k_new_batch_stride; a.kn_ts = c.k_new_token_stride;
    a.vn_bs = v_new_batch_stride; a.vn_ts = c.v_new_token_stride;
    a.window_left = window_left; a.window_right = window_right;
    a.scale = (float)c.softmax_scale; a.softcap = c.softcap; a.alibi = c.alibi_slopes; a.alibi_bstride = c.alibi_batch_stride;
    a.num_splits = S; a.workspace = c.workspace;
    a.rotary_cos = c.rotary_cos; a.rotary_sin = c.rotary_sin; a.rotary_cos_rs = c.rotary_cos_row_stride; a.rotary_sin_rs = c.rotary_sin_row_stride;
    a.rotary_dim = c.rotary_dim; a.rotary_interleaved = c.rotary_interleaved ? 1 : 0; a.rotary_q_per_token = c.rotary_cos ? rotary_q_per_token : 0;
    a.cache_e4m3 = e4m3 ? 1 : 0; a.k_descale = c.k_descale; a.v_descale = c.v_descale; a.descale_bstride = c.descale_batch_stride;
    a.sinks = c.sinks; a.sink_heads = c.sinks ? c.sink_heads : 1;
    a.cu_seqlens_q = c.cu_seqlens_q; a.cu_seqlens_k_new = c.cu_seqlens_k_new;
    a.total_q = c.total_q; a.max_seqlen_q = c.max_seqlen_q; a.total_k_new = c.total_k_new;
    a.qv = c.qv; a.qv_bs = c.qv_batch_stride; a.qv_ts = c.qv_token_stride; a.d_v = c.d_v;
    if (vq && seqlen_q == 0 && seqlen_new == 0) return FA_OK;   // no query token and nothing to append: no launch
    return launched(who, fa::launch_kvcache(a, reinterpret_cast<hipStream_t>(c.stream)));
}

// the 37 arguments of fa_ex_forward_kvcache, which every entry point of the family has
static KvCall kv_call(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                      void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                      int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                      int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                      int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                      int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                      double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, void* workspace,
                      size_t workspace_bytes, void* stream) {
    KvCall c;
    c.q = q; c.k_cache = k_cache; c.v_cache = v_cache; c.k_new = k_new; c.v_new = v_new; c.cache_seqlens = cache_seqlens; c.o = o; c.lse = lse;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.seqlen_new = seqlen_new; c.cache_len = cache_len;
    c.d = d; c.dtype = dtype; c.cache_dtype = dtype; c.q_batch_stride = q_batch_stride; c.q_token_stride = q_token_stride;
    c.k_cache_batch_stride = k_cache_batch_stride; c.k_cache_token_stride = k_cache_token_stride; c.k_new_batch_stride = k_new_batch_stride;
    c.v_cache_batch_stride = v_cache_batch_stride; c.v_cache_token_stride = v_cache_token_stride; c.v_new_batch_stride = v_new_batch_stride;
    c.k_new_token_stride = k_new_token_stride; c.v_new_token_stride = v_new_token_stride;
    c.causal = causal; c.window_left = window_left; c.window_right = window_right; c.softmax_scale = softmax_scale; c.softcap = softcap;
    c.alibi_slopes = alibi_slopes; c.alibi_batch_stride = alibi_batch_stride; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    return c;
}

int fa_ex_forward_kvcache(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                          void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                          int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                          int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                          int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                          int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                          double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                          void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    return kvcache_impl("fa_ex_forward_kvcache", c);
}

int fa_ex_forward_kvcache_paged(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                                void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                                int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                                int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                                int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                                int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                                const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                                int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                                void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch; c.cache_leftpad = cache_leftpad;
    return kvcache_impl("fa_ex_forward_kvcache_paged", c);
}

int fa_ex_forward_kvcache_rotary(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                                 void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                                 int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                                 int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                                 int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                                 int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                 double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                                 const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                                 int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                                 const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                                 int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch; c.cache_leftpad = cache_leftpad;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    return kvcache_impl("fa_ex_forward_kvcache_rotary", c);
}

int fa_ex_forward_kvcache_fp8(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                              void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                              int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                              int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                              int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                              int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                              double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                              const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                              int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                              const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                              int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                              int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                              void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch; c.cache_leftpad = cache_leftpad;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    c.cache_dtype = cache_dtype; c.k_descale = k_descale; c.v_descale = v_descale; c.descale_batch_stride = descale_batch_stride;
    return kvcache_impl("fa_ex_forward_kvcache_fp8", c);
}

int fa_ex_forward_kvcache_sink(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                               void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                               int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                               int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                               int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                               int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                               double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                               const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                               int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                               const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                               int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                               int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                               const float* sinks, int64_t sink_heads,
                               void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch; c.cache_leftpad = cache_leftpad;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    c.cache_dtype = cache_dtype; c.k_descale = k_descale; c.v_descale = v_descale; c.descale_batch_stride = descale_batch_stride;
    c.sinks = sinks; c.sink_heads = sink_heads;
    return kvcache_impl("fa_ex_forward_kvcache_sink", c);
}

int fa_ex_forward_kvcache_varlen(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                                 void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                                 int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                                 int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                                 int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                                 int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                 double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                                 const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                                 int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                                 const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                                 int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                                 int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                                 const float* sinks, int64_t sink_heads,
                                 const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k_new, int64_t total_q,
                                 int64_t max_seqlen_q, int64_t total_k_new,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch; c.cache_leftpad = cache_leftpad;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    c.cache_dtype = cache_dtype; c.k_descale = k_descale; c.v_descale = v_descale; c.descale_batch_stride = descale_batch_stride;
    c.sinks = sinks; c.sink_heads = sink_heads;
    c.cu_seqlens_q = cu_seqlens_q; c.cu_seqlens_k_new = cu_seqlens_k_new; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    c.total_k_new = total_k_new;
    return kvcache_impl("fa_ex_forward_kvcache_varlen", c);
}

int fa_ex_forward_kvcache_qv(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                                 void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                                 int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                                 int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                                 int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                                 int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                                 double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits,
                                 const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                                 int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                                 const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                                 int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                                 int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                                 const float* sinks, int64_t sink_heads,
                                 const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k_new, int64_t total_q,
                                 int64_t max_seqlen_q, int64_t total_k_new,
                                 const void* qv, int64_t qv_batch_stride, int64_t qv_token_stride, int64_t d_v,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    KvCall c = kv_call(q, k_cache, v_cache, k_new, v_new, cache_seqlens, o, lse, batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d, dtype,
                       q_batch_stride, q_token_stride, k_cache_batch_stride, k_cache_token_stride, v_cache_batch_stride, v_cache_token_stride,
                       k_new_batch_stride, k_new_token_stride, v_new_batch_stride, v_new_token_stride, causal, window_left, window_right,
                       softmax_scale, softcap, alibi_slopes, alibi_batch_stride, num_splits, workspace, workspace_bytes, stream);
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch; c.cache_leftpad = cache_leftpad;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    c.cache_dtype = cache_dtype; c.k_descale = k_descale; c.v_descale = v_descale; c.descale_batch_stride = descale_batch_stride;
    c.sinks = sinks; c.sink_heads = sink_heads;
    c.cu_seqlens_q = cu_seqlens_q; c.cu_seqlens_k_new = cu_seqlens_k_new; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    c.total_k_new = total_k_new;
    c.qv = qv; c.qv_batch_stride = qv_batch_stride; c.qv_token_stride = qv_token_stride; c.d_v = d_v;
    return kvcache_impl("fa_ex_forward_kvcache_qv", c);
}

// ---- sparse MLA decoding: see include/fa_mi355x.h
static int64_t mla_sparse_splits(int64_t batch, int64_t hq, int64_t hkv, int64_t nq, int64_t topk, int64_t num_splits) {
    if (num_splits > 0) return num_splits;
    return fa::mla_sparse_num_splits(batch * nq, hkv, hq / hkv, topk);
}

size_t fa_mla_sparse_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t topk, int64_t num_splits) {
    if (batch <= 0 || heads_q <= 0 || heads_kv <= 0 || heads_q % heads_kv != 0 || seqlen_q <= 0 || topk < 0 || num_splits < 0 || num_splits > 256)
        return 0;
    return fa::kv_workspace_bytes(1, heads_q, batch * seqlen_q, 512, (int)mla_sparse_splits(batch, heads_q, heads_kv, seqlen_q, topk, num_splits));
}

// One call of the fa_mla_sparse_forward family, a field per argument under its name in the header.  Defaults: "argument absent".
struct MlaSparseCall {
    const void *q = nullptr, *qv = nullptr, *k_cache = nullptr, *v_cache = nullptr;
    const int32_t *indices = nullptr, *cache_seqlens = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    int64_t batch = 0, heads_q = 0, heads_kv = 0, seqlen_q = 0, cache_len = 0, topk = 0, d = 0, d_v = 0;
    int dtype = 0;
    int64_t q_batch_stride = 0, q_token_stride = 0, qv_batch_stride = 0, qv_token_stride = 0, k_cache_batch_stride = 0,
            k_cache_token_stride = 0, v_cache_batch_stride = 0, v_cache_token_stride = 0, indices_batch_stride = 0,
            indices_token_stride = 0, indices_head_stride = 0;
    int causal = 0;
    double softmax_scale = 0.0;
    int64_t num_splits = 0;
    const int32_t *block_table = nullptr, *cache_batch_idx = nullptr;
    int64_t block_table_row_stride = 0, num_blocks = 0, page_block_size = 0, max_blocks_per_seq = 0, cache_batch = 0;
    void *workspace = nullptr, *stream = nullptr;
    size_t workspace_bytes = 0;
};

// The checks, in the order the header documents: (0) the shape's signs and the empty call; (1) null pointers; (2) widths; (3) dtype,
// then the ranges of the shape; (4) strides and alignment of every tensor; (5) indices; (6) the page geometry; (7) the workspace.
static int mla_sparse_impl(const char* who, const MlaSparseCall& c) {
    if (c.batch < 0 || c.seqlen_q < 0 || c.heads_q < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch, seqlen_q and heads_q must be >= 0 (got %lld, %lld, %lld)", who, (long long)c.batch,
                    (long long)c.seqlen_q, (long long)c.heads_q);
    if (c.batch == 0 || c.seqlen_q == 0 || c.heads_q == 0) return FA_OK;   // no row: no launch
    // (1)
    if (!c.q || !c.qv || !c.k_cache || !c.v_cache || !c.o || !c.lse || (!c.indices && c.topk != 0))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    // (2)
    if (c.d != 64 || c.d_v != 512)
        return fail(FA_ERR_UNSUPPORTED, "%s: supported for head_dim = 64 with d_v = 512 only (got head_dim = %lld, d_v = %lld)", who,
                    (long long)c.d, (long long)c.d_v);
    // (3)
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype must be f16 or bf16 (got code %d)", who, c.dtype);
    if (c.heads_kv < 1 || c.heads_q % c.heads_kv != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_q=%lld must be a positive multiple of heads_kv=%lld", who, (long long)c.heads_q,
                    (long long)c.heads_kv);
    if (!(c.softmax_scale == c.softmax_scale) || c.softmax_scale - c.softmax_scale != 0.0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be finite (got %g)", who, c.softmax_scale);
    if (!scale_ok(c.softmax_scale)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be > 0 (got %g)", who, c.softmax_scale);
    if (c.num_splits < 0 || c.num_splits > 256)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_splits must lie in [0, 256] (got %lld)", who, (long long)c.num_splits);
    const bool paged = c.block_table != nullptr;
    if (!paged && c.cache_len < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_len must be >= 1 (got %lld)", who, (long long)c.cache_len);
    if (c.cache_batch_idx) {
        if (paged) return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table cannot be combined with cache_batch_idx", who);
        if (c.cache_batch < 1 || c.cache_batch > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch must lie in [1, 2^31) with cache_batch_idx (got %lld)", who,
                        (long long)c.cache_batch);
    } else if (c.cache_batch != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch must be 0 without cache_batch_idx (got %lld)", who, (long long)c.cache_batch);
    }
    // (one list per grid column, the K/V heads' row tiles along z, the combine one wave per row)
    if (c.batch > 0x7fffffff / c.seqlen_q || c.heads_q > 65535 || c.cache_len > ((int64_t)1 << 28) || c.seqlen_q > ((int64_t)1 << 24) ||
        c.batch * c.seqlen_q * c.heads_q >= ((int64_t)1 << 31))
        return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    // (4) the heads of a token adjacent at its width, tokens at >= heads * width, units past the last token's heads
    const int64_t c_n = paged ? c.page_block_size : c.cache_len;
    const int64_t c_units = paged ? c.num_blocks : c.cache_batch_idx ? c.cache_batch : c.batch;
    struct { const char* name; int64_t bs, ts, n, heads, units, w; } st[4] = {
        {"q", c.q_batch_stride, c.q_token_stride, c.seqlen_q, c.heads_q, c.batch, c.d},
        {"qv", c.qv_batch_stride, c.qv_token_stride, c.seqlen_q, c.heads_q, c.batch, c.d_v},
        {"k_cache", c.k_cache_batch_stride, c.k_cache_token_stride, c_n, c.heads_kv, c_units, c.d},
        {"v_cache", c.v_cache_batch_stride, c.v_cache_token_stride, c_n, c.heads_kv, c_units, c.d_v}};
    for (auto& t : st) {
        const int64_t span = (t.n > 0 ? (t.n - 1) * t.ts : 0) + t.heads * t.w;   // elements of one batch element (or page)
        if (t.ts < t.heads * t.w || (t.units > 1 && t.bs < span) || t.bs < 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)",
                        who, t.name, (long long)t.bs, (long long)t.ts, (long long)(t.heads * t.w), (long long)span);
        if (t.ts % 8 != 0 || t.bs % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s must be multiples of 8 elements", who, t.name);
        if (span * 2 >= ((int64_t)1 << 31) || t.bs > ((int64_t)1 << 44))
            return fail(FA_ERR_UNSUPPORTED, "%s: one batch element of %s spans %lld bytes, beyond 32-bit offsets", who, t.name,
                        (long long)(span * 2));
    }
    if (!aligned16({c.q, c.qv, c.k_cache, c.v_cache, c.o}))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: tensors must be 16-byte aligned", who);
    if ((uintptr_t)c.lse % 4 != 0 || (uintptr_t)c.indices % 4 != 0 || (uintptr_t)c.cache_seqlens % 4 != 0 || (uintptr_t)c.block_table % 4 != 0 ||
        (uintptr_t)c.cache_batch_idx % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: lse, indices, cache_seqlens, block_table and cache_batch_idx must be 4-byte aligned", who);
    // (5) a list is topk adjacent entries; head stride 0: one list for the K/V heads of a token
    if (c.topk < 0 || c.topk > ((int64_t)1 << 30))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: topk must lie in [0, 2^30] (got %lld)", who, (long long)c.topk);
    const int64_t kIxMax = (int64_t)1 << 40;
    const int64_t ix_tok = c.indices_head_stride > 0 ? (c.heads_kv - 1) * c.indices_head_stride + c.topk : c.topk;
    const int64_t ix_seq = (c.seqlen_q - 1) * c.indices_token_stride + ix_tok;
    if ((c.indices_head_stride != 0 && c.indices_head_stride < c.topk) || c.indices_head_stride > kIxMax ||
        (c.seqlen_q > 1 && c.indices_token_stride < ix_tok) || c.indices_token_stride < 0 || c.indices_token_stride > kIxMax ||
        (c.batch > 1 && c.indices_batch_stride < ix_seq) || c.indices_batch_stride < 0 || c.indices_batch_stride > kIxMax)
        return fail(FA_ERR_INVALID_ARGUMENT,
                    "%s: strides of indices (batch %lld, token %lld, head %lld): head must be 0 or >= topk = %lld, token >= %lld, batch >= %lld "
                    "(each <= 2^40)", who, (long long)c.indices_batch_stride, (long long)c.indices_token_stride,
                    (long long)c.indices_head_stride, (long long)c.topk, (long long)ix_tok, (long long)ix_seq);
    // (6)
    int64_t capacity = c.cache_len;
    if (paged) {
        if (c.page_block_size < 16 || c.page_block_size % 16 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: page_block_size must be a positive multiple of 16 (got %lld)", who,
                        (long long)c.page_block_size);
        if (c.num_blocks < 1 || c.num_blocks > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_blocks must lie in [1, 2^31) (got %lld)", who, (long long)c.num_blocks);
        if (c.max_blocks_per_seq < 1)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_blocks_per_seq must be >= 1 (got %lld)", who, (long long)c.max_blocks_per_seq);
        if (c.max_blocks_per_seq > ((int64_t)1 << 28) / c.page_block_size)
            return fail(FA_ERR_UNSUPPORTED, "%s: capacity max_blocks_per_seq * page_block_size = %lld * %lld is beyond 2^28 tokens", who,
                        (long long)c.max_blocks_per_seq, (long long)c.page_block_size);
        if (c.block_table_row_stride < c.max_blocks_per_seq || c.block_table_row_stride > ((int64_t)1 << 40))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table_row_stride=%lld must be >= max_blocks_per_seq=%lld (and <= 2^40)", who,
                        (long long)c.block_table_row_stride, (long long)c.max_blocks_per_seq);
        capacity = c.max_blocks_per_seq * c.page_block_size;
    } else if (c.block_table_row_stride != 0 || c.num_blocks != 0 || c.page_block_size != 0 || c.max_blocks_per_seq != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT,
                    "%s: block_table_row_stride, num_blocks, page_block_size and max_blocks_per_seq must be 0 without block_table", who);
    }
    // (7)
    const int64_t S = mla_sparse_splits(c.batch, c.heads_q, c.heads_kv, c.seqlen_q, c.topk, c.num_splits);
    if (S > 1 && c.batch * c.seqlen_q * c.heads_q >= ((int64_t)1 << 26))   // the combine: one wave per row, 2^32 lanes per launch
        return fail(FA_ERR_UNSUPPORTED, "%s: batch * seqlen_q * heads_q = %lld rows are too many to combine %lld splits in one launch", who,
                    (long long)(c.batch * c.seqlen_q * c.heads_q), (long long)S);
    const size_t need = fa::kv_workspace_bytes(1, c.heads_q, c.batch * c.seqlen_q, c.d_v, (int)S);
    if (c.workspace_bytes < need || (need > 0 && !c.workspace))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace of %zu bytes needed, %zu given", who, need, c.workspace_bytes);
    if (need > 0 && !aligned16({c.workspace})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
    fa::MlaSparseArgs a{};
    fa::KvArgs& kv = a.kv;
    kv.q = c.q; kv.qv = c.qv; kv.k_cache = const_cast<void*>(c.k_cache); kv.v_cache = const_cast<void*>(c.v_cache); kv.o = c.o; kv.lse = c.lse;
    kv.cache_seqlens = c.cache_seqlens; kv.block_table = c.block_table; kv.cache_batch_idx = c.cache_batch_idx;
    kv.table_row_stride = c.block_table_row_stride; kv.num_blocks = c.num_blocks; kv.page_size = c.page_block_size; kv.cache_batch = c.cache_batch;
    kv.batch = c.batch; kv.heads_q = c.heads_q; kv.heads_kv = c.heads_kv; kv.seqlen_q = c.seqlen_q; kv.cache_len = capacity;
    kv.d = c.d; kv.d_v = c.d_v; kv.dtype = c.dtype; kv.causal = c.causal ? 1 : 0;
    kv.q_bs = c.q_batch_stride; kv.q_ts = c.q_token_stride; kv.qv_bs = c.qv_batch_stride; kv.qv_ts = c.qv_token_stride;
    kv.kc_bs = c.k_cache_batch_stride; kv.kc_ts = c.k_cache_token_stride; kv.vc_bs = c.v_cache_batch_stride; kv.vc_ts = c.v_cache_token_stride;
    kv.window_left = kv.window_right = -1;
    kv.scale = (float)c.softmax_scale; kv.num_splits = S; kv.workspace = c.workspace;
    a.indices = c.indices; a.ix_bs = c.indices_batch_stride; a.ix_ts = c.indices_token_stride; a.ix_hs = c.indices_head_stride; a.topk = c.topk;
    return launched(who, fa::launch_mla_sparse(a, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_mla_sparse_forward(const void* q, const void* qv, const void* k_cache, const void* v_cache, const int32_t* indices,
                          const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                          int64_t cache_len, int64_t topk, int64_t d, int64_t d_v, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                          int64_t qv_batch_stride, int64_t qv_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                          int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t indices_batch_stride,
                          int64_t indices_token_stride, int64_t indices_head_stride, int causal, double softmax_scale, int64_t num_splits,
                          const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                          int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, void* workspace,
                          size_t workspace_bytes, void* stream) {
    MlaSparseCall c;
    c.q = q; c.qv = qv; c.k_cache = k_cache; c.v_cache = v_cache; c.indices = indices; c.cache_seqlens = cache_seqlens; c.o = o; c.lse = lse;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.cache_len = cache_len; c.topk = topk;
    c.d = d; c.d_v = d_v; c.dtype = dtype;
    c.q_batch_stride = q_batch_stride; c.q_token_stride = q_token_stride; c.qv_batch_stride = qv_batch_stride; c.qv_token_stride = qv_token_stride;
    c.k_cache_batch_stride = k_cache_batch_stride; c.k_cache_token_stride = k_cache_token_stride;
    c.v_cache_batch_stride = v_cache_batch_stride; c.v_cache_token_stride = v_cache_token_stride;
    c.indices_batch_stride = indices_batch_stride; c.indices_token_stride = indices_token_stride; c.indices_head_stride = indices_head_stride;
    c.causal = causal; c.softmax_scale = softmax_scale; c.num_splits = num_splits;
    c.block_table = block_table; c.block_table_row_stride = block_table_row_stride; c.num_blocks = num_blocks;
    c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.cache_batch_idx = cache_batch_idx; c.cache_batch = cache_batch;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    return mla_sparse_impl("fa_mla_sparse_forward", c);
}

// ---- MLA decoding from the packed 8-bit latent cache, and the append into it: see include/fa_mi355x.h
static int64_t mla_fp8_splits(int64_t batch, int64_t hq, int64_t hkv, int64_t nq, int64_t capacity, int64_t topk, bool sparse, int64_t num_splits) {
    return sparse ? mla_sparse_splits(batch, hq, hkv, nq, topk, num_splits) : kv_splits_qv(batch, hq, hkv, nq, capacity, num_splits);
}

size_t fa_mla_fp8_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t topk,
                                  int with_indices, int64_t num_splits) {
    if (batch <= 0 || heads_q <= 0 || heads_kv != 1 || seqlen_q <= 0 || cache_len < 0 || topk < 0 || (!with_indices && topk != 0) ||
        num_splits < 0 || num_splits > 256)
        return 0;
    return fa::kv_workspace_bytes(1, heads_q, batch * seqlen_q, 512,
                                  (int)mla_fp8_splits(batch, heads_q, heads_kv, seqlen_q, cache_len, topk, with_indices != 0, num_splits));
}

static const int64_t kF8TokenBytes = 656;

// the rules of a packed pool's geometry that fa_mla_fp8_forward and fa_mla_fp8_pack share: the two byte strides, then the pages
static int mla_fp8_pool_ok(const char* who, const void* pool, int64_t page_stride_bytes, int64_t token_stride_bytes, int64_t page_block_size) {
    if (token_stride_bytes < kF8TokenBytes || token_stride_bytes % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: token_stride_bytes must be >= 656 and a multiple of 16 (got %lld)", who,
                    (long long)token_stride_bytes);
    if (token_stride_bytes >= ((int64_t)1 << 31))
        return fail(FA_ERR_UNSUPPORTED, "%s: token_stride_bytes = %lld is beyond 32-bit offsets", who, (long long)token_stride_bytes);
    const int64_t span = (page_block_size > 0 ? page_block_size - 1 : 0) * token_stride_bytes + kF8TokenBytes;
    if (page_stride_bytes < span || page_stride_bytes % 16 != 0 || page_stride_bytes > ((int64_t)1 << 44))
        return fail(FA_ERR_INVALID_ARGUMENT,
                    "%s: page_stride_bytes must be >= (page_block_size - 1) * token_stride_bytes + 656 = %lld and a multiple of 16 (got %lld)", who,
                    (long long)span, (long long)page_stride_bytes);
    if (!aligned16({pool})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: kv_cache must be 16-byte aligned", who);
    return FA_OK;
}

static int mla_fp8_pages_ok(const char* who, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq) {
    if (page_block_size < 16 || page_block_size % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: page_block_size must be a positive multiple of 16 (got %lld)", who, (long long)page_block_size);
    if (num_blocks < 1 || num_blocks > 0x7fffffff)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_blocks must lie in [1, 2^31) (got %lld)", who, (long long)num_blocks);
    if (max_blocks_per_seq < 1)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_blocks_per_seq must be >= 1 (got %lld)", who, (long long)max_blocks_per_seq);
    if (max_blocks_per_seq > ((int64_t)1 << 28) / page_block_size)
        return fail(FA_ERR_UNSUPPORTED, "%s: capacity max_blocks_per_seq * page_block_size = %lld * %lld is beyond 2^28 tokens", who,
                    (long long)max_blocks_per_seq, (long long)page_block_size);
    if (block_table_row_stride < max_blocks_per_seq || block_table_row_stride > ((int64_t)1 << 40))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table_row_stride=%lld must be >= max_blocks_per_seq=%lld (and <= 2^40)", who,
                    (long long)block_table_row_stride, (long long)max_blocks_per_seq);
    return FA_OK;
}

// The checks, in the order the header documents: (0) the shape's signs and the empty call; (1) null pointers; (2) widths; (3) dtype,
// heads_kv, block_table, then the ranges of the shape; (4) strides and alignment of q and qv, then the pool's; (5) indices; (6) the
// page geometry; (7) the workspace.
int fa_mla_fp8_forward(const void* q, const void* qv, const void* kv_cache, const int32_t* indices, const int32_t* cache_seqlens,
                       const int32_t* block_table, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                       int64_t topk, int64_t d, int64_t d_v, int dtype, int64_t q_batch_stride, int64_t q_token_stride, int64_t q_head_stride,
                       int64_t qv_batch_stride, int64_t qv_token_stride, int64_t qv_head_stride, int64_t page_stride_bytes, int64_t token_stride_bytes,
                       int64_t indices_batch_stride, int64_t indices_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                       int64_t page_block_size, int64_t max_blocks_per_seq, int causal, double softmax_scale, int64_t num_splits,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "fa_mla_fp8_forward";
    if (batch < 0 || seqlen_q < 0 || heads_q < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch, seqlen_q and heads_q must be >= 0 (got %lld, %lld, %lld)", who, (long long)batch,
                    (long long)seqlen_q, (long long)heads_q);
    if (batch == 0 || seqlen_q == 0 || heads_q == 0) return FA_OK;   // no row: no launch
    // (1)
    if (!q || !qv || !kv_cache || !o || !lse) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    // (2)
    if (d != 64 || d_v != 512)
        return fail(FA_ERR_UNSUPPORTED, "%s: supported for head_dim = 64 with d_v = 512 only (got head_dim = %lld, d_v = %lld)", who,
                    (long long)d, (long long)d_v);
    // (3)
    if (dtype == FA_DTYPE_F16)
        return fail(FA_ERR_UNSUPPORTED, "%s: f16 is not supported: the rotary part of a packed token is bf16, and so are q, qv and o", who);
    if (dtype != FA_DTYPE_BF16) return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype must be bf16 (got code %d)", who, dtype);
    if (heads_kv != 1)
        return fail(FA_ERR_UNSUPPORTED, "%s: heads_kv must be 1: a packed token holds one latent row (got %lld)", who, (long long)heads_kv);
    if (!block_table) return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table is required: the packed cache is a paged pool", who);
    if (!(softmax_scale == softmax_scale) || softmax_scale - softmax_scale != 0.0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be finite (got %g)", who, softmax_scale);
    if (!scale_ok(softmax_scale)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be > 0 (got %g)", who, softmax_scale);
    if (num_splits < 0 || num_splits > 256)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_splits must lie in [0, 256] (got %lld)", who, (long long)num_splits);
    // (dense: the row tiles along grid y, the sequences along z; lists: one per grid column)
    if (batch > 0x7fffffff / seqlen_q || heads_q > 65535 || seqlen_q > ((int64_t)1 << 24) || batch * seqlen_q * heads_q >= ((int64_t)1 << 31) ||
        (!indices && (batch > 65535 || (heads_q * seqlen_q + 15) / 16 > 65535)))
        return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    // (4)
    struct { const char* name; int64_t bs, ts, hs, w; } st[2] = {{"q", q_batch_stride, q_token_stride, q_head_stride, d},
                                                                {"qv", qv_batch_stride, qv_token_stride, qv_head_stride, d_v}};
    for (auto& t : st) {
        if (t.hs < t.w || t.hs > ((int64_t)1 << 20))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: head stride of %s must lie in [%lld, 2^20] (got %lld)", who, t.name, (long long)t.w,
                        (long long)t.hs);
        const int64_t tok = (heads_q - 1) * t.hs + t.w, span = (seqlen_q - 1) * t.ts + tok;
        if (t.ts < tok || (batch > 1 && t.bs < span) || t.bs < 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)",
                        who, t.name, (long long)t.bs, (long long)t.ts, (long long)tok, (long long)span);
        if (t.ts % 8 != 0 || t.bs % 8 != 0 || t.hs % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s must be multiples of 8 elements", who, t.name);
        if (span * 2 >= ((int64_t)1 << 31) || t.bs > ((int64_t)1 << 44))
            return fail(FA_ERR_UNSUPPORTED, "%s: one batch element of %s spans %lld bytes, beyond 32-bit offsets", who, t.name,
                        (long long)(span * 2));
    }
    if (int rc = mla_fp8_pool_ok(who, kv_cache, page_stride_bytes, token_stride_bytes, page_block_size)) return rc;
    if (!aligned16({q, qv, o})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: tensors must be 16-byte aligned", who);
    if ((uintptr_t)lse % 4 != 0 || (uintptr_t)indices % 4 != 0 || (uintptr_t)cache_seqlens % 4 != 0 || (uintptr_t)block_table % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: lse, indices, cache_seqlens and block_table must be 4-byte aligned", who);
    // (5) a list is topk adjacent entries, one list a query token
    if (indices) {
        if (topk < 0 || topk > ((int64_t)1 << 30))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: topk must lie in [0, 2^30] (got %lld)", who, (long long)topk);
        const int64_t kIxMax = (int64_t)1 << 40;
        const int64_t ix_seq = (seqlen_q - 1) * indices_token_stride + topk;
        if ((seqlen_q > 1 && indices_token_stride < topk) || indices_token_stride < 0 || indices_token_stride > kIxMax ||
            (batch > 1 && indices_batch_stride < ix_seq) || indices_batch_stride < 0 || indices_batch_stride > kIxMax)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of indices (batch %lld, token %lld): token >= topk = %lld, batch >= %lld (each <= 2^40)",
                        who, (long long)indices_batch_stride, (long long)indices_token_stride, (long long)topk, (long long)ix_seq);
    } else if (topk != 0 || indices_batch_stride != 0 || indices_token_stride != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: topk, indices_batch_stride and indices_token_stride must be 0 without indices", who);
    }
    // (6)
    if (int rc = mla_fp8_pages_ok(who, block_table_row_stride, num_blocks, page_block_size, max_blocks_per_seq)) return rc;
    const int64_t capacity = max_blocks_per_seq * page_block_size;
    // (7)
    const int64_t S = mla_fp8_splits(batch, heads_q, heads_kv, seqlen_q, capacity, topk, indices != nullptr, num_splits);
    if (S > 1 && batch * seqlen_q * heads_q >= ((int64_t)1 << 26))   // the combine: one wave per row, 2^32 lanes per launch
        return fail(FA_ERR_UNSUPPORTED, "%s: batch * seqlen_q * heads_q = %lld rows are too many to combine %lld splits in one launch", who,
                    (long long)(batch * seqlen_q * heads_q), (long long)S);
    const size_t need = fa::kv_workspace_bytes(1, heads_q, batch * seqlen_q, d_v, (int)S);
    if (workspace_bytes < need || (need > 0 && !workspace))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    if (need > 0 && !aligned16({workspace})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
    fa::MlaF8Args a{};
    fa::KvArgs& kv = a.sa.kv;
    kv.q = q; kv.qv = qv; kv.o = o; kv.lse = lse;
    kv.cache_seqlens = cache_seqlens; kv.block_table = block_table;
    kv.table_row_stride = block_table_row_stride; kv.num_blocks = num_blocks; kv.page_size = page_block_size;
    kv.batch = batch; kv.heads_q = heads_q; kv.heads_kv = heads_kv; kv.seqlen_q = seqlen_q; kv.cache_len = capacity;
    kv.d = d; kv.d_v = d_v; kv.dtype = dtype; kv.causal = causal ? 1 : 0;
    kv.q_bs = q_batch_stride; kv.q_ts = q_token_stride; kv.qv_bs = qv_batch_stride; kv.qv_ts = qv_token_stride;
    kv.window_left = kv.window_right = -1;
    kv.scale = (float)softmax_scale; kv.num_splits = S; kv.workspace = workspace;
    a.sa.indices = indices; a.sa.ix_bs = indices_batch_stride; a.sa.ix_ts = indices_token_stride; a.sa.ix_hs = 0; a.sa.topk = topk;
    a.pool = kv_cache; a.page_sb = page_stride_bytes; a.tok_sb = token_stride_bytes;
    a.q_hs = q_head_stride; a.qv_hs = qv_head_stride;
    return launched(who, fa::launch_mla_f8(a, reinterpret_cast<hipStream_t>(stream)));
}

int fa_mla_fp8_pack(const void* latent_new, const void* rope_new, void* kv_cache, const int32_t* cache_seqlens, const int32_t* block_table,
                    int64_t batch, int64_t seqlen_new, int64_t latent_batch_stride, int64_t latent_token_stride, int64_t rope_batch_stride,
                    int64_t rope_token_stride, int64_t page_stride_bytes, int64_t token_stride_bytes, int64_t block_table_row_stride,
                    int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq, int scale_pow2, void* stream) {
    const char* who = "fa_mla_fp8_pack";
    if (batch < 0 || seqlen_new < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch and seqlen_new must be >= 0 (got %lld, %lld)", who, (long long)batch, (long long)seqlen_new);
    if (batch == 0 || seqlen_new == 0) return FA_OK;   // no token: no launch
    if (!latent_new || !rope_new || !kv_cache || !cache_seqlens || !block_table) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (batch > 0x7fffffff / seqlen_new) return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    struct { const char* name; int64_t bs, ts, w; } st[2] = {{"latent_new", latent_batch_stride, latent_token_stride, 512},
                                                            {"rope_new", rope_batch_stride, rope_token_stride, 64}};
    for (auto& t : st) {
        const int64_t span = (seqlen_new - 1) * t.ts + t.w;
        if (t.ts < t.w || (batch > 1 && t.bs < span) || t.bs < 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)",
                        who, t.name, (long long)t.bs, (long long)t.ts, (long long)t.w, (long long)span);
        if (t.ts % 8 != 0 || t.bs % 8 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of %s must be multiples of 8 elements", who, t.name);
        if (t.ts > ((int64_t)1 << 31) || t.bs > ((int64_t)1 << 44))
            return fail(FA_ERR_UNSUPPORTED, "%s: strides of %s beyond 2^31 (token) or 2^44 (batch) elements", who, t.name);
    }
    if (int rc = mla_fp8_pool_ok(who, kv_cache, page_stride_bytes, token_stride_bytes, page_block_size)) return rc;
    if (!aligned16({latent_new, rope_new})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: tensors must be 16-byte aligned", who);
    if ((uintptr_t)cache_seqlens % 4 != 0 || (uintptr_t)block_table % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_seqlens and block_table must be 4-byte aligned", who);
    if (int rc = mla_fp8_pages_ok(who, block_table_row_stride, num_blocks, page_block_size, max_blocks_per_seq)) return rc;
    fa::MlaF8PackArgs a{};
    a.latent = latent_new; a.rope = rope_new; a.pool = kv_cache; a.cache_seqlens = cache_seqlens; a.block_table = block_table;
    a.batch = batch; a.seqlen_new = seqlen_new; a.lat_bs = latent_batch_stride; a.lat_ts = latent_token_stride;
    a.rope_bs = rope_batch_stride; a.rope_ts = rope_token_stride; a.page_sb = page_stride_bytes; a.tok_sb = token_stride_bytes;
    a.table_row_stride = block_table_row_stride; a.num_blocks = num_blocks; a.page_size = page_block_size; a.max_blocks = max_blocks_per_seq;
    a.scale_pow2 = scale_pow2;
    return launched(who, fa::launch_mla_f8_pack(a, reinterpret_cast<hipStream_t>(stream)));
}

// ---- the lightning indexer (fa_indexer_pack, fa_indexer_logits, fa_indexer_topk): see include/fa_mi355x.h.  One record a call, a
// field per argument under its name in the header.
static const int64_t kIdxTokenBytes = 132;

// the rules of an index-key pool's geometry that the append and the logits share: the two byte strides, then the address
static int indexer_pool_ok(const char* who, const void* pool, int64_t page_stride_bytes, int64_t token_stride_bytes, int64_t page_block_size) {
    if (token_stride_bytes < kIdxTokenBytes || token_stride_bytes % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: token_stride_bytes must be >= 132 and a multiple of 16 (got %lld)", who,
                    (long long)token_stride_bytes);
    if (token_stride_bytes >= ((int64_t)1 << 31))
        return fail(FA_ERR_UNSUPPORTED, "%s: token_stride_bytes = %lld is beyond 32-bit offsets", who, (long long)token_stride_bytes);
    const int64_t span = (page_block_size > 0 ? page_block_size - 1 : 0) * token_stride_bytes + kIdxTokenBytes;
    if (page_stride_bytes < span || page_stride_bytes % 16 != 0 || page_stride_bytes > ((int64_t)1 << 44))
        return fail(FA_ERR_INVALID_ARGUMENT,
                    "%s: page_stride_bytes must be >= (page_block_size - 1) * token_stride_bytes + 132 = %lld and a multiple of 16 (got %lld)", who,
                    (long long)span, (long long)page_stride_bytes);
    if (!aligned16({pool})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_cache must be 16-byte aligned", who);
    return FA_OK;
}

struct IndexerPackCall {
    const void* k_new = nullptr;
    void* k_cache = nullptr;
    const int32_t *cache_seqlens = nullptr, *block_table = nullptr;
    int64_t batch = 0, seqlen_new = 0, d = 0, k_new_batch_stride = 0, k_new_token_stride = 0, page_stride_bytes = 0, token_stride_bytes = 0,
            block_table_row_stride = 0, num_blocks = 0, page_block_size = 0, max_blocks_per_seq = 0;
    int scale_pow2 = 0;
    void* stream = nullptr;
};

static int indexer_pack_impl(const char* who, const IndexerPackCall& c) {
    if (c.batch < 0 || c.seqlen_new < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch and seqlen_new must be >= 0 (got %lld, %lld)", who, (long long)c.batch,
                    (long long)c.seqlen_new);
    if (c.batch == 0 || c.seqlen_new == 0) return FA_OK;   // no token: no launch
    // (1)
    if (!c.k_new || !c.k_cache || !c.cache_seqlens || !c.block_table) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    // (2)
    if (c.d != 128) return fail(FA_ERR_UNSUPPORTED, "%s: supported for head_dim = 128 only (got %lld)", who, (long long)c.d);
    if (c.batch > 0x7fffffff / c.seqlen_new) return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    // (3)
    const int64_t span = (c.seqlen_new - 1) * c.k_new_token_stride + c.d;
    if (c.k_new_token_stride < c.d || (c.batch > 1 && c.k_new_batch_stride < span) || c.k_new_batch_stride < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of k_new too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)", who,
                    (long long)c.k_new_batch_stride, (long long)c.k_new_token_stride, (long long)c.d, (long long)span);
    if (c.k_new_token_stride % 8 != 0 || c.k_new_batch_stride % 8 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of k_new must be multiples of 8 elements", who);
    if (c.k_new_token_stride > ((int64_t)1 << 31) || c.k_new_batch_stride > ((int64_t)1 << 44))
        return fail(FA_ERR_UNSUPPORTED, "%s: strides of k_new beyond 2^31 (token) or 2^44 (batch) elements", who);
    if (int rc = indexer_pool_ok(who, c.k_cache, c.page_stride_bytes, c.token_stride_bytes, c.page_block_size)) return rc;
    if (!aligned16({c.k_new})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_new must be 16-byte aligned", who);
    if ((uintptr_t)c.cache_seqlens % 4 != 0 || (uintptr_t)c.block_table % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_seqlens and block_table must be 4-byte aligned", who);
    // (4)
    if (int rc = mla_fp8_pages_ok(who, c.block_table_row_stride, c.num_blocks, c.page_block_size, c.max_blocks_per_seq)) return rc;
    fa::IndexerPackArgs a{};
    a.k_new = c.k_new; a.pool = c.k_cache; a.cache_seqlens = c.cache_seqlens; a.block_table = c.block_table;
    a.batch = c.batch; a.seqlen_new = c.seqlen_new; a.k_bs = c.k_new_batch_stride; a.k_ts = c.k_new_token_stride;
    a.page_sb = c.page_stride_bytes; a.tok_sb = c.token_stride_bytes; a.table_row_stride = c.block_table_row_stride;
    a.num_blocks = c.num_blocks; a.page_size = c.page_block_size; a.max_blocks = c.max_blocks_per_seq; a.scale_pow2 = c.scale_pow2;
    return launched(who, fa::launch_indexer_pack(a, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_indexer_pack(const void* k_new, void* k_cache, const int32_t* cache_seqlens, const int32_t* block_table, int64_t batch,
                    int64_t seqlen_new, int64_t d, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t page_stride_bytes,
                    int64_t token_stride_bytes, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                    int64_t max_blocks_per_seq, int scale_pow2, void* stream) {
    IndexerPackCall c;
    c.k_new = k_new; c.k_cache = k_cache; c.cache_seqlens = cache_seqlens; c.block_table = block_table;
    c.batch = batch; c.seqlen_new = seqlen_new; c.d = d; c.k_new_batch_stride = k_new_batch_stride; c.k_new_token_stride = k_new_token_stride;
    c.page_stride_bytes = page_stride_bytes; c.token_stride_bytes = token_stride_bytes; c.block_table_row_stride = block_table_row_stride;
    c.num_blocks = num_blocks; c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.scale_pow2 = scale_pow2; c.stream = stream;
    return indexer_pack_impl("fa_indexer_pack", c);
}

static const int64_t kIdxWidthMax = (int64_t)1 << 28, kIdxTopkMax = (int64_t)1 << 20;

// the rules of a (batch, seqlen_q, width) float32 logits tensor that the logits and the selection share
static int indexer_logits_ok(const char* who, const void* logits, int64_t batch, int64_t seqlen_q, int64_t width, int64_t bs, int64_t rs) {
    const int64_t kMax = (int64_t)1 << 44, seq = (seqlen_q - 1) * rs + width;
    if ((seqlen_q > 1 && rs < width) || rs < 0 || rs > kMax || (batch > 1 && bs < seq) || bs < 0 || bs > kMax)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of logits (batch %lld, row %lld): row >= width = %lld, batch >= %lld (each <= 2^44)", who,
                    (long long)bs, (long long)rs, (long long)width, (long long)seq);
    if ((uintptr_t)logits % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: logits must be 4-byte aligned", who);
    return FA_OK;
}

struct IndexerLogitsCall {
    const void *q = nullptr, *k_cache = nullptr;
    const float* weights = nullptr;
    const int32_t *cache_seqlens = nullptr, *block_table = nullptr;
    float* logits = nullptr;
    int64_t batch = 0, seqlen_q = 0, heads = 0, d = 0, width = 0, q_batch_stride = 0, q_token_stride = 0, q_head_stride = 0,
            weights_batch_stride = 0, weights_token_stride = 0, logits_batch_stride = 0, logits_row_stride = 0, page_stride_bytes = 0,
            token_stride_bytes = 0, block_table_row_stride = 0, num_blocks = 0, page_block_size = 0, max_blocks_per_seq = 0;
    int causal = 0;
    void* stream = nullptr;
};

static int indexer_logits_impl(const char* who, const IndexerLogitsCall& c) {
    if (c.batch < 0 || c.seqlen_q < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch and seqlen_q must be >= 0 (got %lld, %lld)", who, (long long)c.batch, (long long)c.seqlen_q);
    if (c.batch == 0 || c.seqlen_q == 0) return FA_OK;   // no row: no launch
    // (1)
    if (!c.q || !c.weights || !c.k_cache || !c.cache_seqlens || !c.block_table || !c.logits)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    // (2)
    if (c.d != 128) return fail(FA_ERR_UNSUPPORTED, "%s: supported for head_dim = 128 only (got %lld)", who, (long long)c.d);
    if (c.heads != 32 && c.heads != 64)
        return fail(FA_ERR_UNSUPPORTED, "%s: supported for 32 or 64 index heads only (got %lld)", who, (long long)c.heads);
    // (3)
    if (c.width < 1 || c.width > kIdxWidthMax)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: width must lie in [1, 2^28] (got %lld)", who, (long long)c.width);
    if (c.batch > 65535 || c.seqlen_q > ((int64_t)1 << 22)) return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    // (4) q in bytes, weights and logits in elements
    if (c.q_head_stride < c.d || c.q_head_stride > ((int64_t)1 << 20))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: head stride of q must lie in [128, 2^20] (got %lld)", who, (long long)c.q_head_stride);
    const int64_t qtok = (c.heads - 1) * c.q_head_stride + c.d, qspan = (c.seqlen_q - 1) * c.q_token_stride + qtok;
    if (c.q_token_stride < qtok || (c.batch > 1 && c.q_batch_stride < qspan) || c.q_batch_stride < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of q too small (batch %lld, token %lld; need token >= %lld, batch >= %lld)", who,
                    (long long)c.q_batch_stride, (long long)c.q_token_stride, (long long)qtok, (long long)qspan);
    if (c.q_head_stride % 16 != 0 || c.q_token_stride % 16 != 0 || c.q_batch_stride % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of q must be multiples of 16 bytes", who);
    if (c.q_token_stride > ((int64_t)1 << 31) || c.q_batch_stride > ((int64_t)1 << 44))
        return fail(FA_ERR_UNSUPPORTED, "%s: strides of q beyond 2^31 (token) or 2^44 (batch) bytes", who);
    const int64_t wspan = (c.seqlen_q - 1) * c.weights_token_stride + c.heads;
    if (c.weights_token_stride < c.heads || (c.batch > 1 && c.weights_batch_stride < wspan) || c.weights_batch_stride < 0 ||
        c.weights_token_stride > ((int64_t)1 << 31) || c.weights_batch_stride > ((int64_t)1 << 44))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of weights (batch %lld, token %lld): token >= heads = %lld, batch >= %lld", who,
                    (long long)c.weights_batch_stride, (long long)c.weights_token_stride, (long long)c.heads, (long long)wspan);
    if (int rc = indexer_logits_ok(who, c.logits, c.batch, c.seqlen_q, c.width, c.logits_batch_stride, c.logits_row_stride)) return rc;
    if (int rc = indexer_pool_ok(who, c.k_cache, c.page_stride_bytes, c.token_stride_bytes, c.page_block_size)) return rc;
    if (!aligned16({c.q})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q must be 16-byte aligned", who);
    if ((uintptr_t)c.weights % 4 != 0 || (uintptr_t)c.cache_seqlens % 4 != 0 || (uintptr_t)c.block_table % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: weights, cache_seqlens and block_table must be 4-byte aligned", who);
    // (5)
    if (int rc = mla_fp8_pages_ok(who, c.block_table_row_stride, c.num_blocks, c.page_block_size, c.max_blocks_per_seq)) return rc;
    fa::IndexerLogitsArgs a{};
    a.q = c.q; a.pool = c.k_cache; a.weights = c.weights; a.cache_seqlens = c.cache_seqlens; a.block_table = c.block_table; a.logits = c.logits;
    a.batch = c.batch; a.seqlen_q = c.seqlen_q; a.heads = c.heads; a.width = c.width;
    a.q_bs = c.q_batch_stride; a.q_ts = c.q_token_stride; a.q_hs = c.q_head_stride; a.w_bs = c.weights_batch_stride; a.w_ts = c.weights_token_stride;
    a.lg_bs = c.logits_batch_stride; a.lg_rs = c.logits_row_stride; a.page_sb = c.page_stride_bytes; a.tok_sb = c.token_stride_bytes;
    a.table_row_stride = c.block_table_row_stride; a.num_blocks = c.num_blocks; a.page_size = c.page_block_size;
    a.max_blocks = c.max_blocks_per_seq; a.causal = c.causal ? 1 : 0;
    return launched(who, fa::launch_indexer_logits(a, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_indexer_logits(const void* q, const float* weights, const void* k_cache, const int32_t* cache_seqlens, const int32_t* block_table,
                      float* logits, int64_t batch, int64_t seqlen_q, int64_t heads, int64_t d, int64_t width, int64_t q_batch_stride,
                      int64_t q_token_stride, int64_t q_head_stride, int64_t weights_batch_stride, int64_t weights_token_stride,
                      int64_t logits_batch_stride, int64_t logits_row_stride, int64_t page_stride_bytes, int64_t token_stride_bytes,
                      int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq, int causal,
                      void* stream) {
    IndexerLogitsCall c;
    c.q = q; c.weights = weights; c.k_cache = k_cache; c.cache_seqlens = cache_seqlens; c.block_table = block_table; c.logits = logits;
    c.batch = batch; c.seqlen_q = seqlen_q; c.heads = heads; c.d = d; c.width = width;
    c.q_batch_stride = q_batch_stride; c.q_token_stride = q_token_stride; c.q_head_stride = q_head_stride;
    c.weights_batch_stride = weights_batch_stride; c.weights_token_stride = weights_token_stride;
    c.logits_batch_stride = logits_batch_stride; c.logits_row_stride = logits_row_stride;
    c.page_stride_bytes = page_stride_bytes; c.token_stride_bytes = token_stride_bytes; c.block_table_row_stride = block_table_row_stride;
    c.num_blocks = num_blocks; c.page_block_size = page_block_size; c.max_blocks_per_seq = max_blocks_per_seq;
    c.causal = causal; c.stream = stream;
    return indexer_logits_impl("fa_indexer_logits", c);
}

struct IndexerTopkCall {
    const float* logits = nullptr;
    const int32_t* cache_seqlens = nullptr;
    int32_t* indices = nullptr;
    int64_t batch = 0, seqlen_q = 0, width = 0, topk = 0, logits_batch_stride = 0, logits_row_stride = 0, indices_batch_stride = 0,
            indices_token_stride = 0;
    int causal = 0;
    void* stream = nullptr;
};

static int indexer_topk_impl(const char* who, const IndexerTopkCall& c) {
    if (c.batch < 0 || c.seqlen_q < 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch and seqlen_q must be >= 0 (got %lld, %lld)", who, (long long)c.batch, (long long)c.seqlen_q);
    if (c.batch == 0 || c.seqlen_q == 0) return FA_OK;   // no row: no launch
    // (1)
    if (!c.logits || !c.cache_seqlens || !c.indices) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    // (2)
    if (c.topk < 1 || c.topk > kIdxTopkMax) return fail(FA_ERR_INVALID_ARGUMENT, "%s: topk must lie in [1, 2^20] (got %lld)", who, (long long)c.topk);
    if (c.width < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: width must be >= 1 (got %lld)", who, (long long)c.width);
    if (c.width > kIdxWidthMax) return fail(FA_ERR_UNSUPPORTED, "%s: width = %lld is beyond 2^28 keys a row", who, (long long)c.width);
    if (c.batch > 65535 || c.seqlen_q > 0x7fffffff) return fail(FA_ERR_UNSUPPORTED, "%s: problem too large for one launch", who);
    // (3)
    if (int rc = indexer_logits_ok(who, c.logits, c.batch, c.seqlen_q, c.width, c.logits_batch_stride, c.logits_row_stride)) return rc;
    const int64_t kIxMax = (int64_t)1 << 40, ix_seq = (c.seqlen_q - 1) * c.indices_token_stride + c.topk;
    if ((c.seqlen_q > 1 && c.indices_token_stride < c.topk) || c.indices_token_stride < 0 || c.indices_token_stride > kIxMax ||
        (c.batch > 1 && c.indices_batch_stride < ix_seq) || c.indices_batch_stride < 0 || c.indices_batch_stride > kIxMax)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: strides of indices (batch %lld, token %lld): token >= topk = %lld, batch >= %lld (each <= 2^40)",
                    who, (long long)c.indices_batch_stride, (long long)c.indices_token_stride, (long long)c.topk, (long long)ix_seq);
    if ((uintptr_t)c.indices % 4 != 0 || (uintptr_t)c.cache_seqlens % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: indices and cache_seqlens must be 4-byte aligned", who);
    fa::IndexerTopkArgs a{};
    a.logits = c.logits; a.cache_seqlens = c.cache_seqlens; a.indices = c.indices;
    a.batch = c.batch; a.seqlen_q = c.seqlen_q; a.width = c.width; a.topk = c.topk;
    a.lg_bs = c.logits_batch_stride; a.lg_rs = c.logits_row_stride; a.ix_bs = c.indices_batch_stride; a.ix_ts = c.indices_token_stride;
    a.causal = c.causal ? 1 : 0;
    return launched(who, fa::launch_indexer_topk(a, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_indexer_topk(const float* logits, const int32_t* cache_seqlens, int32_t* indices, int64_t batch, int64_t seqlen_q, int64_t width,
                    int64_t topk, int64_t logits_batch_stride, int64_t logits_row_stride, int64_t indices_batch_stride,
                    int64_t indices_token_stride, int causal, void* stream) {
    IndexerTopkCall c;
    c.logits = logits; c.cache_seqlens = cache_seqlens; c.indices = indices;
    c.batch = batch; c.seqlen_q = seqlen_q; c.width = width; c.topk = topk;
    c.logits_batch_stride = logits_batch_stride; c.logits_row_stride = logits_row_stride;
    c.indices_batch_stride = indices_batch_stride; c.indices_token_stride = indices_token_stride;
    c.causal = causal; c.stream = stream;
    return indexer_topk_impl("fa_indexer_topk", c);
}

// One call of the fa_rotary_apply family, a field per argument under its name in the header.  Defaults: "argument absent".
struct RotaryCall {
    const void* x = nullptr;
    void* y = nullptr;
    int64_t batch = 0, seqlen = 0, heads = 0, d = 0;
    int dtype = 0;
    int64_t x_batch_stride = 0, x_token_stride = 0, y_batch_stride = 0, y_token_stride = 0;
    // _rotary
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;
    int64_t rotary_cos_row_stride = 0, rotary_sin_row_stride = 0, seqlen_ro = 0, rotary_dim = 0;
    int rotary_interleaved = 0;
    int conjugate = 0;
    int64_t seqlen_offset = 0;
    const int32_t *seqlen_offsets = nullptr, *cu_seqlens = nullptr;
    int64_t total = 0, max_seqlen = 0;
    void* stream = nullptr;
};

static int rotary_impl(const char* who, const RotaryCall& c) {
    const int64_t kStrideMax = (int64_t)1 << 31, kBatchStrideMax = (int64_t)1 << 44;   // no 64-bit offset can overflow
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype must be f16 or bf16 (got code %d)", who, c.dtype);
    if (c.d < 8 || c.d > 256 || c.d % 8 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: head_dim must be a multiple of 8 in [8, 256] (got %lld)", who, (long long)c.d);
    if (c.batch < 1 || c.batch > 65535) return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch must lie in [1, 65535] (got %lld)", who, (long long)c.batch);
    if (c.heads < 1 || c.heads > 0x7fffffff / c.d)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads must be >= 1 with heads * head_dim < 2^31 (got %lld)", who, (long long)c.heads);
    if (c.seqlen < 0 || c.seqlen > 0x7fffffff)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen must lie in [0, 2^31) (got %lld)", who, (long long)c.seqlen);
    if (!c.x || !c.y) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if ((uintptr_t)c.x % 16 != 0 || (uintptr_t)c.y % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: x and y must be 16-byte aligned", who);
    if ((uintptr_t)c.seqlen_offsets % 4 != 0 || (uintptr_t)c.cu_seqlens % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_offsets and cu_seqlens must be 4-byte aligned", who);
    const bool packed = c.cu_seqlens != nullptr;
    if (packed) {
        if (c.total < 0 || c.total > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: total must lie in [0, 2^31) (got %lld)", who, (long long)c.total);
        if (c.max_seqlen < 0 || c.max_seqlen > c.total)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_seqlen=%lld must lie in [0, total=%lld]", who, (long long)c.max_seqlen,
                        (long long)c.total);
        if (c.seqlen != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen must be 0 with cu_seqlens (got %lld)", who, (long long)c.seqlen);
    } else if (c.total != 0 || c.max_seqlen != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total and max_seqlen must be 0 without cu_seqlens (got %lld, %lld)", who,
                    (long long)c.total, (long long)c.max_seqlen);
    }
    const int64_t row = c.heads * c.d;
    if (c.x_token_stride < row || c.y_token_stride < row || c.x_token_stride > kStrideMax || c.y_token_stride > kStrideMax)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: token strides (%lld, %lld) must be >= heads * head_dim = %lld (and <= 2^31)", who,
                    (long long)c.x_token_stride, (long long)c.y_token_stride, (long long)row);
    if (!packed && c.batch > 1) {
        const int64_t xs = (c.seqlen > 0 ? (c.seqlen - 1) * c.x_token_stride : 0) + row;
        const int64_t ys = (c.seqlen > 0 ? (c.seqlen - 1) * c.y_token_stride : 0) + row;
        if (c.x_batch_stride < xs || c.y_batch_stride < ys || c.x_batch_stride > kBatchStrideMax || c.y_batch_stride > kBatchStrideMax)
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: batch strides (%lld, %lld) must be >= (seqlen - 1) * token stride + heads * head_dim = (%lld, %lld) (and <= 2^44)", who,
                        (long long)c.x_batch_stride, (long long)c.y_batch_stride, (long long)xs, (long long)ys);
    }
    const bool batch_strides = !packed && c.batch > 1;   // the only form that addresses with them
    if (c.x_token_stride % 8 != 0 || c.y_token_stride % 8 != 0 ||
        (batch_strides && (c.x_batch_stride % 8 != 0 || c.y_batch_stride % 8 != 0)))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: every stride must be a multiple of 8 elements", who);
    if (c.y == c.x && (c.x_token_stride != c.y_token_stride || (batch_strides && c.x_batch_stride != c.y_batch_stride)))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: y == x (in place) needs equal strides", who);
    if (!c.rotary_cos || !c.rotary_sin) return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must both be given", who);
    if ((uintptr_t)c.rotary_cos % 4 != 0 || (uintptr_t)c.rotary_sin % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must be 4-byte aligned", who);
    if (c.rotary_dim < 16 || c.rotary_dim > c.d || c.rotary_dim % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_dim must be a multiple of 16 in [16, head_dim=%lld] (got %lld)", who,
                    (long long)c.d, (long long)c.rotary_dim);
    if (c.rotary_cos_row_stride < c.rotary_dim / 2 || c.rotary_sin_row_stride < c.rotary_dim / 2 ||
        c.rotary_cos_row_stride > kStrideMax || c.rotary_sin_row_stride > kStrideMax)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be >= rotary_dim / 2 = %lld (and <= 2^31)", who,
                    (long long)c.rotary_cos_row_stride, (long long)c.rotary_sin_row_stride, (long long)(c.rotary_dim / 2));
    if (c.rotary_cos_row_stride % 2 != 0 || c.rotary_sin_row_stride % 2 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be even", who,
                    (long long)c.rotary_cos_row_stride, (long long)c.rotary_sin_row_stride);
    if (c.seqlen_ro < 1 || c.seqlen_ro > 0x7fffffff)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_ro must lie in [1, 2^31) (got %lld)", who, (long long)c.seqlen_ro);
    if (c.seqlen_offset <= -((int64_t)1 << 31) || c.seqlen_offset >= ((int64_t)1 << 31))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: |seqlen_offset| must be < 2^31 (got %lld)", who, (long long)c.seqlen_offset);
    if ((packed ? c.max_seqlen : c.seqlen) == 0) return FA_OK;   // no token: no launch
    fa::RotaryArgs a;
    a.x = c.x; a.y = c.y; a.batch = c.batch; a.seqlen = c.seqlen; a.heads = c.heads; a.d = c.d; a.dtype = c.dtype;
    a.x_bs = batch_strides ? c.x_batch_stride : 0; a.x_ts = c.x_token_stride;
    a.y_bs = batch_strides ? c.y_batch_stride : 0; a.y_ts = c.y_token_stride;
    a.rotary_cos = c.rotary_cos; a.rotary_sin = c.rotary_sin; a.rotary_cos_rs = c.rotary_cos_row_stride; a.rotary_sin_rs = c.rotary_sin_row_stride;
    a.seqlen_ro = c.seqlen_ro; a.rotary_dim = c.rotary_dim; a.rotary_interleaved = c.rotary_interleaved ? 1 : 0;
    a.conjugate = c.conjugate ? 1 : 0; a.seqlen_offset = c.seqlen_offset; a.seqlen_offsets = c.seqlen_offsets;
    a.cu_seqlens = c.cu_seqlens; a.total = c.total; a.max_seqlen = c.max_seqlen;
    return launched(who, fa::launch_rotary(a, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_rotary_apply(const void* x, void* y, int64_t batch, int64_t seqlen, int64_t heads, int64_t d, int dtype, int64_t x_batch_stride,
                    int64_t x_token_stride, int64_t y_batch_stride, int64_t y_token_stride, const void* rotary_cos, const void* rotary_sin,
                    int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim,
                    int rotary_interleaved, int conjugate, int64_t seqlen_offset, const int32_t* seqlen_offsets,
                    const int32_t* cu_seqlens, int64_t total, int64_t max_seqlen, void* stream) {
    RotaryCall c;
    c.x = x; c.y = y; c.batch = batch; c.seqlen = seqlen; c.heads = heads; c.d = d; c.dtype = dtype;
    c.x_batch_stride = x_batch_stride; c.x_token_stride = x_token_stride; c.y_batch_stride = y_batch_stride; c.y_token_stride = y_token_stride;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    c.conjugate = conjugate; c.seqlen_offset = seqlen_offset; c.seqlen_offsets = seqlen_offsets;
    c.cu_seqlens = cu_seqlens; c.total = total; c.max_seqlen = max_seqlen; c.stream = stream;
    return rotary_impl("fa_rotary_apply", c);
}

// ---- the fp8 quantiser: see include/fa_mi355x.h
// One call of the fa_fp8_quantize family, a field per argument under its name in the header.  Defaults: "argument absent".
struct Fp8QuantCall {
    const void* x = nullptr;
    void* out = nullptr;
    const float* descale = nullptr;
    float* descale_out = nullptr;
    const int32_t* cu_seqlens = nullptr;
    // _rotary
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;
    int64_t rotary_cos_row_stride = 0, rotary_sin_row_stride = 0, seqlen_ro = 0, rotary_dim = 0;
    int rotary_interleaved = 0;
    int64_t seqlen_offset = 0;
    const int32_t* seqlen_offsets = nullptr;
    int64_t batch = 0, heads = 0, seqlen = 0, d = 0, heads_per_scale = 0, total = 0, max_seqlen = 0;
    int dtype = 0;
    int64_t x_batch_stride = 0, x_head_stride = 0, x_token_stride = 0, out_batch_stride = 0, out_head_stride = 0, out_token_stride = 0,
            descale_batch_stride = 0;
    int scale_pow2 = 0;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    void* stream = nullptr;
};

static int fp8_quantize_impl(const char* who, const Fp8QuantCall& c) {
    const int64_t kSpan = (int64_t)1 << 58, kStrideMax = (int64_t)1 << 31;
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype must be f16 or bf16 (got code %d)", who, c.dtype);
    if (c.d < 16 || c.d > 256 || c.d % 16 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: head_dim must be a multiple of 16 in [16, 256] (got %lld)", who, (long long)c.d);
    if (c.batch < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch must be >= 1 (got %lld)", who, (long long)c.batch);
    if (c.heads < 1 || c.heads > 0x7fffffff / c.d)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads must be >= 1 with heads * head_dim < 2^31 (got %lld)", who, (long long)c.heads);
    if (c.heads_per_scale < 1 || c.heads % c.heads_per_scale != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_per_scale must be >= 1 and divide heads = %lld (got %lld)", who, (long long)c.heads,
                    (long long)c.heads_per_scale);
    const int64_t nj = c.heads / c.heads_per_scale;
    if (c.batch > 0x7fffffff / nj)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch * heads / heads_per_scale must be < 2^31 (got %lld * %lld)", who, (long long)c.batch,
                    (long long)nj);
    if (c.seqlen < 0 || c.seqlen > 0x7fffffff)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen must lie in [0, 2^31) (got %lld)", who, (long long)c.seqlen);
    if (!c.x || !c.out) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if ((uintptr_t)c.x % 16 != 0 || (uintptr_t)c.out % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: x and out must be 16-byte aligned", who);
    if ((uintptr_t)c.descale % 4 != 0 || (uintptr_t)c.descale_out % 4 != 0 || (uintptr_t)c.cu_seqlens % 4 != 0 ||
        (uintptr_t)c.seqlen_offsets % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale, descale_out, cu_seqlens and seqlen_offsets must be 4-byte aligned", who);
    if (!c.descale && !c.descale_out)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dynamic mode (descale == NULL) needs descale_out", who);
    const bool packed = c.cu_seqlens != nullptr;
    if (packed) {
        if (c.total < 0 || c.total > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: total must lie in [0, 2^31) (got %lld)", who, (long long)c.total);
        if (c.max_seqlen < 0 || c.max_seqlen > c.total)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_seqlen=%lld must lie in [0, total=%lld]", who, (long long)c.max_seqlen,
                        (long long)c.total);
        if (c.seqlen != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen must be 0 with cu_seqlens (got %lld)", who, (long long)c.seqlen);
    } else if (c.total != 0 || c.max_seqlen != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total and max_seqlen must be 0 without cu_seqlens (got %lld, %lld)", who,
                    (long long)c.total, (long long)c.max_seqlen);
    }
    const bool batch_strides = !packed && c.batch > 1;   // the only form that addresses with them
    const int64_t tokens = packed ? c.total : c.seqlen;
    const int64_t ext[3] = {batch_strides ? c.batch : 1, c.heads, tokens};
    const int64_t xs[3] = {c.x_batch_stride, c.x_head_stride, c.x_token_stride};
    const int64_t os[3] = {c.out_batch_stride, c.out_head_stride, c.out_token_stride};
    for (int j = 0; j < 3; ++j)
        if (ext[j] > 1 && (xs[j] < 0 || xs[j] % 8 != 0 || xs[j] > kSpan / (ext[j] - 1)))
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: the strides of x (batch %lld, head %lld, token %lld) must be >= 0 and multiples of 8 elements with (extent - 1) * "
                        "stride <= 2^58", who, (long long)xs[0], (long long)xs[1], (long long)xs[2]);
    for (int j = 0; j < 3; ++j)
        if (ext[j] > 1 && (os[j] < 0 || os[j] % 16 != 0 || os[j] > kSpan / (ext[j] - 1)))
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: the strides of out (batch %lld, head %lld, token %lld) must be >= 0 and multiples of 16 bytes with (extent - 1) * "
                        "stride <= 2^58", who, (long long)os[0], (long long)os[1], (long long)os[2]);
    {   // two addressed rows of out never overlap
        const int64_t hspan = c.heads > 1 ? (c.heads - 1) * c.out_head_stride : 0, tspan = tokens > 1 ? (tokens - 1) * c.out_token_stride : 0;
        const bool heads_inner = (c.heads == 1 || c.out_head_stride >= c.d) && (tokens <= 1 || c.out_token_stride >= hspan + c.d);
        const bool tokens_inner = (tokens <= 1 || c.out_token_stride >= c.d) && (c.heads == 1 || c.out_head_stride >= tspan + c.d);
        if (!heads_inner && !tokens_inner)
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: rows of out overlap: head stride %lld >= head_dim and token stride %lld >= (heads - 1) * head stride + head_dim, or "
                        "the two the other way round", who, (long long)c.out_head_stride, (long long)c.out_token_stride);
        if (batch_strides && c.out_batch_stride < hspan + tspan + c.d)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: out's batch stride %lld must cover one batch element (%lld bytes)", who,
                        (long long)c.out_batch_stride, (long long)(hspan + tspan + c.d));
    }
    if (c.descale && c.descale_batch_stride != 0 && (c.descale_batch_stride < nj || c.descale_batch_stride > ((int64_t)1 << 40)))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: descale_batch_stride must be 0 or lie in [heads / heads_per_scale = %lld, 2^40] (got %lld)",
                    who, (long long)nj, (long long)c.descale_batch_stride);
    const bool rot = c.rotary_cos || c.rotary_sin;
    if (rot) {
        if (!c.rotary_cos || !c.rotary_sin) return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must both be given", who);
        if ((uintptr_t)c.rotary_cos % 4 != 0 || (uintptr_t)c.rotary_sin % 4 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must be 4-byte aligned", who);
        if (c.rotary_dim < 16 || c.rotary_dim > c.d || c.rotary_dim % 16 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_dim must be a multiple of 16 in [16, head_dim=%lld] (got %lld)", who,
                        (long long)c.d, (long long)c.rotary_dim);
        if (c.rotary_cos_row_stride < c.rotary_dim / 2 || c.rotary_sin_row_stride < c.rotary_dim / 2 ||
            c.rotary_cos_row_stride > kStrideMax || c.rotary_sin_row_stride > kStrideMax)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be >= rotary_dim / 2 = %lld (and <= 2^31)", who,
                        (long long)c.rotary_cos_row_stride, (long long)c.rotary_sin_row_stride, (long long)(c.rotary_dim / 2));
        if (c.rotary_cos_row_stride % 2 != 0 || c.rotary_sin_row_stride % 2 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be even", who,
                        (long long)c.rotary_cos_row_stride, (long long)c.rotary_sin_row_stride);
        if (c.seqlen_ro < 1 || c.seqlen_ro > 0x7fffffff)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_ro must lie in [1, 2^31) (got %lld)", who, (long long)c.seqlen_ro);
        if (c.seqlen_offset <= -((int64_t)1 << 31) || c.seqlen_offset >= ((int64_t)1 << 31))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: |seqlen_offset| must be < 2^31 (got %lld)", who, (long long)c.seqlen_offset);
    }
    fa::Fp8QuantArgs a;
    a.x = c.x; a.out = c.out; a.descale = c.descale; a.descale_out = c.descale_out; a.cu_seqlens = c.cu_seqlens;
    if (rot) {
        a.rotary_cos = c.rotary_cos; a.rotary_sin = c.rotary_sin; a.rotary_cos_rs = c.rotary_cos_row_stride;
        a.rotary_sin_rs = c.rotary_sin_row_stride; a.seqlen_ro = c.seqlen_ro; a.rotary_dim = c.rotary_dim;
        a.rotary_interleaved = c.rotary_interleaved ? 1 : 0; a.seqlen_offset = c.seqlen_offset; a.seqlen_offsets = c.seqlen_offsets;
    }
    a.batch = c.batch; a.heads = c.heads; a.seqlen = c.seqlen; a.d = c.d; a.heads_per_scale = c.heads_per_scale; a.total = c.total;
    a.max_seqlen = c.max_seqlen; a.dtype = c.dtype;
    a.x_bs = batch_strides ? c.x_batch_stride : 0; a.x_hs = c.heads > 1 ? c.x_head_stride : 0; a.x_ts = tokens > 1 ? c.x_token_stride : 0;
    a.o_bs = batch_strides ? c.out_batch_stride : 0; a.o_hs = c.heads > 1 ? c.out_head_stride : 0; a.o_ts = tokens > 1 ? c.out_token_stride : 0;
    a.descale_bs = c.descale_batch_stride; a.scale_pow2 = c.scale_pow2 ? 1 : 0;
    if (fa::fp8_quant_unit_items(a) > 0x7fffffff)
        return fail(FA_ERR_UNSUPPORTED, "%s: a scale unit of %lld 16-byte chunks is beyond 2^31", who, (long long)fa::fp8_quant_unit_items(a));
    if (fa::fp8_quant_two_pass(a)) {
        const size_t need = fa::fp8_quant_workspace_bytes(c.batch, c.heads, c.heads_per_scale);
        if (!c.workspace || c.workspace_bytes < need)
            return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, c.workspace ? c.workspace_bytes : (size_t)0);
        if ((uintptr_t)c.workspace % 16 != 0) return fail(FA_ERR_WORKSPACE, "%s: the workspace must be 16-byte aligned", who);
        if ((void*)c.descale_out == c.workspace) return fail(FA_ERR_WORKSPACE, "%s: the workspace must not be descale_out", who);
        a.workspace = c.workspace;
    }
    if ((packed ? c.max_seqlen : c.seqlen) == 0 && c.descale && !c.descale_out) return FA_OK;   // nothing to write: no launch
    return launched(who, fa::launch_fp8_quantize(a, reinterpret_cast<hipStream_t>(c.stream)));
}

int fa_fp8_quantize(const void* x, void* out, const float* descale, float* descale_out, const int32_t* cu_seqlens, const void* rotary_cos,
                    const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride, int64_t seqlen_ro,
                    int64_t rotary_dim, int rotary_interleaved, int64_t seqlen_offset, const int32_t* seqlen_offsets, int64_t batch,
                    int64_t heads, int64_t seqlen, int64_t d, int64_t heads_per_scale, int64_t total, int64_t max_seqlen, int dtype,
                    int64_t x_batch_stride, int64_t x_head_stride, int64_t x_token_stride, int64_t out_batch_stride,
                    int64_t out_head_stride, int64_t out_token_stride, int64_t descale_batch_stride, int scale_pow2, void* workspace,
                    size_t workspace_bytes, void* stream) {
    Fp8QuantCall c;
    c.x = x; c.out = out; c.descale = descale; c.descale_out = descale_out; c.cu_seqlens = cu_seqlens;
    c.rotary_cos = rotary_cos; c.rotary_sin = rotary_sin; c.rotary_cos_row_stride = rotary_cos_row_stride;
    c.rotary_sin_row_stride = rotary_sin_row_stride; c.seqlen_ro = seqlen_ro; c.rotary_dim = rotary_dim; c.rotary_interleaved = rotary_interleaved;
    c.seqlen_offset = seqlen_offset; c.seqlen_offsets = seqlen_offsets;
    c.batch = batch; c.heads = heads; c.seqlen = seqlen; c.d = d; c.heads_per_scale = heads_per_scale; c.total = total;
    c.max_seqlen = max_seqlen; c.dtype = dtype;
    c.x_batch_stride = x_batch_stride; c.x_head_stride = x_head_stride; c.x_token_stride = x_token_stride;
    c.out_batch_stride = out_batch_stride; c.out_head_stride = out_head_stride; c.out_token_stride = out_token_stride;
    c.descale_batch_stride = descale_batch_stride; c.scale_pow2 = scale_pow2;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    return fp8_quantize_impl("fa_fp8_quantize", c);
}

size_t fa_fp8_quantize_workspace_bytes(int64_t batch, int64_t heads, int64_t heads_per_scale) {
    if (batch < 1 || heads < 1 || heads_per_scale < 1 || heads % heads_per_scale != 0 || batch > 0x7fffffff / (heads / heads_per_scale))
        return 0;
    return fa::fp8_quant_workspace_bytes(batch, heads, heads_per_scale);
}

// ---- merge of two partial attention results: see include/fa_mi355x.h
// One call of the fa_merge_states family (forward and backward): a tensor is a pointer and its (batch, head, row) strides.
struct MergeCall {
    fa::MergeTensor o_a, lse_a, o_b, lse_b, o, lse, do_, dlse, do_a, do_b, dlse_a, dlse_b;
    int64_t batch = 0, heads = 0, rows = 0, d = 0;
    int dtype = 0;
    void* stream = nullptr;
};

static int merge_impl(const char* who, const MergeCall& c, bool backward) {
    struct Named { const char* name; const fa::MergeTensor* t; bool wide, optional; };   // wide: d elements of the dtype per row
    const Named fwd[] = {{"o_a", &c.o_a, true, false}, {"lse_a", &c.lse_a, false, false}, {"o_b", &c.o_b, true, false},
                         {"lse_b", &c.lse_b, false, false}, {"o", &c.o, true, false}, {"lse", &c.lse, false, false}};
    const Named bwd[] = {{"o_a", &c.o_a, true, false}, {"lse_a", &c.lse_a, false, false}, {"o_b", &c.o_b, true, false},
                         {"lse_b", &c.lse_b, false, false}, {"do_", &c.do_, true, false}, {"dlse", &c.dlse, false, true},
                         {"do_a", &c.do_a, true, false}, {"do_b", &c.do_b, true, false}, {"dlse_a", &c.dlse_a, false, false},
                         {"dlse_b", &c.dlse_b, false, false}};
    const Named* ts = backward ? bwd : fwd;
    const int nt = backward ? 10 : 6;
    if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: unknown dtype code %d", who, c.dtype);
    const int64_t lim = (int64_t)1 << 31;
    if (c.batch < 0 || c.heads < 0 || c.rows < 0 || c.d < 1 || c.batch >= lim || c.heads >= lim || c.rows >= lim)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: bad shape (batch=%lld, heads=%lld, rows=%lld, d=%lld)", who, (long long)c.batch,
                    (long long)c.heads, (long long)c.rows, (long long)c.d);
    if (c.d > 256) return fail(FA_ERR_UNSUPPORTED, "%s: head_dim %lld > 256 is not supported", who, (long long)c.d);
    const bool f32 = c.dtype == FA_DTYPE_F32;
    if (!f32 && c.d % 8 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: head_dim must be a multiple of 8 for 16-bit tensors (got %lld)", who, (long long)c.d);
    if (c.batch == 0 || c.heads == 0 || c.rows == 0) return FA_OK;   // no row: no launch
    if (c.batch * c.heads >= lim) return fail(FA_ERR_UNSUPPORTED, "%s: batch * heads too large for one launch", who);
    for (int i = 0; i < nt; ++i)
        if (!ts[i].t->p && !ts[i].optional) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer (%s)", who, ts[i].name);
    bool vec = f32 && c.d % 4 == 0;   // fp32: 16-byte accesses where everything allows them, 4-byte ones otherwise
    for (int i = 0; i < nt; ++i) {
        const Named& n = ts[i];
        if (!n.t->p) continue;
        const uintptr_t ptr = (uintptr_t)n.t->p;
        if (!n.wide || f32) {
            if (ptr % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", who, n.name);
            if (n.wide && (ptr % 16 != 0 || n.t->bs % 4 != 0 || n.t->hs % 4 != 0 || n.t->rs % 4 != 0)) vec = false;
        } else {
            if (ptr % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s must be 16-byte aligned", who, n.name);
            if (n.t->bs % 8 != 0 || n.t->hs % 8 != 0 || n.t->rs % 8 != 0)
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (%lld, %lld, %lld) must be multiples of 8 elements", who, n.name,
                            (long long)n.t->bs, (long long)n.t->hs, (long long)n.t->rs);
        }
    }
    // no 64-bit byte offset can overflow: every (extent - 1) * stride stays below 2^58 elements
    const int64_t kSpan = (int64_t)1 << 58;
    for (int i = 0; i < nt; ++i) {
        const fa::MergeTensor& t = *ts[i].t;
        if (!t.p) continue;
        const int64_t ext[3] = {c.batch, c.heads, c.rows}, str[3] = {t.bs, t.hs, t.rs};
        for (int j = 0; j < 3; ++j)
            if (str[j] < 0 || (ext[j] > 1 && str[j] > kSpan / (ext[j] - 1)))
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (%lld, %lld, %lld) must be >= 0 with (extent - 1) * stride <= 2^58",
                            who, ts[i].name, (long long)t.bs, (long long)t.hs, (long long)t.rs);
    }
    if (!backward) {   // the in-place forms: the output pair on one of the input pairs, with that one's strides
        const fa::MergeTensor* pairs[2][2] = {{&c.o_a, &c.lse_a}, {&c.o_b, &c.lse_b}};
        for (auto& pr : pairs) {
            const bool same_o = c.o.p == pr[0]->p, same_l = c.lse.p == pr[1]->p;
            if ((same_o && (c.o.bs != pr[0]->bs || c.o.hs != pr[0]->hs || c.o.rs != pr[0]->rs)) ||
                (same_l && (c.lse.bs != pr[1]->bs || c.lse.hs != pr[1]->hs || c.lse.rs != pr[1]->rs)))
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: an output that is an input (in place) needs that input's strides", who);
        }
    }
    fa::MergeArgs a;
    a.o_a = c.o_a; a.lse_a = c.lse_a; a.o_b = c.o_b; a.lse_b = c.lse_b; a.o = c.o; a.lse = c.lse;
    a.dout = c.do_; a.dlse = c.dlse; a.do_a = c.do_a; a.do_b = c.do_b; a.dlse_a = c.dlse_a; a.dlse_b = c.dlse_b;
    a.batch = c.batch; a.heads = c.heads; a.rows = c.rows; a.d = c.d; a.dtype = c.dtype; a.vec = vec;
    return launched(who, fa::launch_merge(a, backward, reinterpret_cast<hipStream_t>(c.stream)));
}

static fa::MergeTensor merge_t(const void* p, int64_t bs, int64_t hs, int64_t rs) {
    fa::MergeTensor t;
    t.p = p; t.bs = bs; t.hs = hs; t.rs = rs;
    return t;
}

int fa_merge_states(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, void* o, float* lse, int64_t batch,
                    int64_t heads, int64_t rows, int64_t d, int dtype, int64_t o_a_batch_stride, int64_t o_a_head_stride,
                    int64_t o_a_row_stride, int64_t lse_a_batch_stride, int64_t lse_a_head_stride, int64_t lse_a_row_stride,
                    int64_t o_b_batch_stride, int64_t o_b_head_stride, int64_t o_b_row_stride, int64_t lse_b_batch_stride,
                    int64_t lse_b_head_stride, int64_t lse_b_row_stride, int64_t o_batch_stride, int64_t o_head_stride,
                    int64_t o_row_stride, int64_t lse_batch_stride, int64_t lse_head_stride, int64_t lse_row_stride, void* stream) {
    MergeCall c;
    c.o_a = merge_t(o_a, o_a_batch_stride, o_a_head_stride, o_a_row_stride);
    c.lse_a = merge_t(lse_a, lse_a_batch_stride, lse_a_head_stride, lse_a_row_stride);
    c.o_b = merge_t(o_b, o_b_batch_stride, o_b_head_stride, o_b_row_stride);
    c.lse_b = merge_t(lse_b, lse_b_batch_stride, lse_b_head_stride, lse_b_row_stride);
    c.o = merge_t(o, o_batch_stride, o_head_stride, o_row_stride);
    c.lse = merge_t(lse, lse_batch_stride, lse_head_stride, lse_row_stride);
    c.batch = batch; c.heads = heads; c.rows = rows; c.d = d; c.dtype = dtype; c.stream = stream;
    return merge_impl("fa_merge_states", c, false);
}

int fa_merge_states_backward(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, const void* do_, const float* dlse,
                             void* do_a, void* do_b, float* dlse_a, float* dlse_b, int64_t batch, int64_t heads, int64_t rows, int64_t d,
                             int dtype, int64_t o_a_batch_stride, int64_t o_a_head_stride, int64_t o_a_row_stride,
                             int64_t lse_a_batch_stride, int64_t lse_a_head_stride, int64_t lse_a_row_stride, int64_t o_b_batch_stride,
                             int64_t o_b_head_stride, int64_t o_b_row_stride, int64_t lse_b_batch_stride, int64_t lse_b_head_stride,
                             int64_t lse_b_row_stride, int64_t do_batch_stride, int64_t do_head_stride, int64_t do_row_stride,
                             int64_t dlse_batch_stride, int64_t dlse_head_stride, int64_t dlse_row_stride, int64_t do_a_batch_stride,
                             int64_t do_a_head_stride, int64_t do_a_row_stride, int64_t do_b_batch_stride, int64_t do_b_head_stride,
                             int64_t do_b_row_stride, int64_t dlse_a_batch_stride, int64_t dlse_a_head_stride, int64_t dlse_a_row_stride,
                             int64_t dlse_b_batch_stride, int64_t dlse_b_head_stride, int64_t dlse_b_row_stride, void* stream) {
    MergeCall c;
    c.o_a = merge_t(o_a, o_a_batch_stride, o_a_head_stride, o_a_row_stride);
    c.lse_a = merge_t(lse_a, lse_a_batch_stride, lse_a_head_stride, lse_a_row_stride);
    c.o_b = merge_t(o_b, o_b_batch_stride, o_b_head_stride, o_b_row_stride);
    c.lse_b = merge_t(lse_b, lse_b_batch_stride, lse_b_head_stride, lse_b_row_stride);
    c.do_ = merge_t(do_, do_batch_stride, do_head_stride, do_row_stride);
    c.dlse = merge_t(dlse, dlse_batch_stride, dlse_head_stride, dlse_row_stride);
    c.do_a = merge_t(do_a, do_a_batch_stride, do_a_head_stride, do_a_row_stride);
    c.do_b = merge_t(do_b, do_b_batch_stride, do_b_head_stride, do_b_row_stride);
    c.dlse_a = merge_t(dlse_a, dlse_a_batch_stride, dlse_a_head_stride, dlse_a_row_stride);
    c.dlse_b = merge_t(dlse_b, dlse_b_batch_stride, dlse_b_head_stride, dlse_b_row_stride);
    c.batch = batch; c.heads = heads; c.rows = rows; c.d = d; c.dtype = dtype; c.stream = stream;
    return merge_impl("fa_merge_states_backward", c, true);
}

// ---- e4m3 q, k, v with per-head descales (FlashAttention-3's fp8 call): see include/fa_mi355x.h
// One call of fa_fp8_forward: a tensor is a pointer and its (batch, head, token) strides.
struct Fp8Tensor {
    const void* p = nullptr;
    int64_t bs = 0, hs = 0, ts = 0;
};
// What the _mod entry points of the three fp8 calls add, checked by name: window bounds >= -1, a finite softcap >= 0, one sink
// per query head.  The parents' entry points leave Fp8Mod at its defaults, which is no feature.
static int fp8_mod_check(const char* who, const fa::Fp8Mod& m, int64_t heads_q) {
    if (m.window_left < -1 || m.window_right < -1)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: window (%lld, %lld): each bound must be >= 0, or -1 for unbounded", who,
                    (long long)m.window_left, (long long)m.window_right);
    if (!(m.softcap == m.softcap) || m.softcap < 0.0 || m.softcap > 3.0e38)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softcap must be a finite number >= 0 (got %g)", who, m.softcap);
    if (m.sinks) {
        if (m.sink_heads != heads_q)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: sink_heads=%lld must be heads_q=%lld (one sink per query head)", who,
                        (long long)m.sink_heads, (long long)heads_q);
        if ((uintptr_t)m.sinks % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: sinks must be 4-byte aligned", who);
    } else if (m.sink_heads != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: sink_heads must be 0 without sinks (got %lld)", who, (long long)m.sink_heads);
    }
    return FA_OK;
}

// The head dim of an fp8 call: 128 through the entry points up to _mod, 64 / 128 / 256 through the _hdim ones (`hdim`).
static int fp8_head_dim_check(const char* who, int64_t d, bool hdim) {
    if (hdim ? (d != 64 && d != 128 && d != 256) : d != 128)
        return fail(FA_ERR_UNSUPPORTED, hdim ? "%s: head_dim %lld is not supported (64, 128 or 256)" : "%s: head_dim %lld is not supported (128 only)",
                    who, (long long)d);
    return FA_OK;
}

struct Fp8Call {
    bool hdim = false;                     // the _hdim entry point: d in {64, 128, 256}, and d bounds what 128 bounds elsewhere
    fa::Fp8Mod mod;
    Fp8Tensor q, k, v, o;
    float* lse = nullptr;
    const float *q_descale = nullptr, *k_descale = nullptr, *v_descale = nullptr;
    int64_t qds_bs = 0, kds_bs = 0, vds_bs = 0;
    int64_t batch = 0, heads_q = 0, heads_kv = 0, nq = 0, nk = 0, d = 0;
    int dtype = 0, causal = 0;
    double scale = 0.0;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    void* stream = nullptr;
};

static int fp8_forward_impl(const char* who, const Fp8Call& c) {
    // (1) null pointers
    if (!c.q.p || !c.k.p || !c.v.p || !c.o.p || !c.lse) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    // (2) dims
    if (c.batch <= 0 || c.heads_q <= 0 || c.heads_kv <= 0 || c.nq <= 0 || c.nk <= 0 || c.d <= 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch, heads_q, heads_kv, seqlen_q, seqlen_k and d must be > 0 (got %lld, %lld, %lld, %lld, %lld, %lld)",
                    who, (long long)c.batch, (long long)c.heads_q, (long long)c.heads_kv, (long long)c.nq, (long long)c.nk, (long long)c.d);
    // (3) the head dim
    if (const int rc = fp8_head_dim_check(who, c.d, c.hdim)) return rc;
    const int64_t d = c.d;
    // (4) the heads ratio
    if (c.heads_q % c.heads_kv != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_q=%lld must be a multiple of heads_kv=%lld", who, (long long)c.heads_q, (long long)c.heads_kv);
    // (5) the output dtype, the scale, the descale strides
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype (of o) must be f16 or bf16 (got code %d)", who, c.dtype);
    if (!(c.scale == c.scale) || !scale_ok(c.scale))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be finite and > 0", who);
    const struct { const char* name; const float* p; int64_t bs; } ds[3] = {
        {"q_descale", c.q_descale, c.qds_bs}, {"k_descale", c.k_descale, c.kds_bs}, {"v_descale", c.v_descale, c.vds_bs}};
    for (const auto& s : ds) {
        if (!s.p && s.bs != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s_batch_stride must be 0 without %s", who, s.name, s.name);
        if (s.bs < 0 || (s.bs != 0 && s.bs < c.heads_kv) || s.bs >= ((int64_t)1 << 31) / c.batch)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s_batch_stride=%lld must be 0 or >= heads_kv=%lld", who, s.name, (long long)s.bs,
                        (long long)c.heads_kv);
        if ((uintptr_t)s.p % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", who, s.name);
    }
    if (const int rc = fp8_mod_check(who, c.mod, c.heads_q)) return rc;
    // (6) alignment and strides: 16-byte units (q, k, v in bytes, o in 16-bit elements), rows that do not overlap
    if (!aligned16({c.q.p, c.k.p, c.v.p, c.o.p})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q, k, v and o must be 16-byte aligned", who);
    if ((uintptr_t)c.lse % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: lse must be 4-byte aligned", who);
    const struct { const char* name; const Fp8Tensor* t; int64_t unit, heads, rows; } ts[4] = {
        {"q", &c.q, 16, c.heads_q, c.nq}, {"k", &c.k, 16, c.heads_kv, c.nk}, {"v", &c.v, 16, c.heads_kv, c.nk}, {"o", &c.o, 8, c.heads_q, c.nq}};
    const int64_t kMaxStride = (int64_t)1 << 44;
    for (const auto& t : ts) {
        const int64_t bs = c.batch > 1 ? t.t->bs : 0, hs = t.heads > 1 ? t.t->hs : 0, tk = t.rows > 1 ? t.t->ts : d;
        if (bs % t.unit != 0 || hs % t.unit != 0 || tk % t.unit != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (%lld, %lld, %lld) must be multiples of %lld elements (16 bytes)", who,
                        t.name, (long long)t.t->bs, (long long)t.t->hs, (long long)t.t->ts, (long long)t.unit);
        if (bs < 0 || hs < 0 || tk < d || bs > kMaxStride || hs > kMaxStride || tk > kMaxStride)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (%lld, %lld, %lld) must be >= 0, the token stride >= %lld", who, t.name,
                        (long long)t.t->bs, (long long)t.t->hs, (long long)t.t->ts, (long long)d);
    }
    // (7) the span limit: q and k are read through 32-bit buffer descriptors and offsets per (batch, head) unit
    const int64_t kSpan = ((int64_t)1 << 31) - 1;
    const int64_t q_span = (c.nq + 255) / 256 * 256 * (c.nq > 1 ? c.q.ts : d), k_span = (c.nk + 255) / 256 * 256 * (c.nk > 1 ? c.k.ts : d);
    if (q_span > kSpan || k_span > kSpan)
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: round_up(rows, 256) * token stride of %s is %lld bytes, at or above 2^31", who,
                    q_span > kSpan ? "q" : "k", (long long)(q_span > kSpan ? q_span : k_span));
    if (c.batch * c.heads_q >= ((int64_t)1 << 31) / ((c.nq + 255) / 256) || c.batch * c.heads_kv >= ((int64_t)1 << 31) / ((c.nk + 63) / 64))
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: batch * heads * tiles too large for one launch", who);
    // (8) the workspace
    const size_t need = fa::fp8in_workspace_bytes(c.batch * c.heads_kv, c.nk, d);
    if (!c.workspace || c.workspace_bytes < need)
        return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes is too small (need %zu: fa_fp8_forward%s_workspace_bytes)", who,
                    c.workspace ? c.workspace_bytes : (size_t)0, need, c.hdim ? "_hdim" : "");
    if ((uintptr_t)c.workspace % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);

    fa::Fp8InArgs a;
    a.q = c.q.p; a.k = c.k.p; a.v = c.v.p; a.o = const_cast<void*>(c.o.p); a.lse = c.lse;
    a.q_descale = c.q_descale; a.k_descale = c.k_descale; a.v_descale = c.v_descale;
    a.qds_bs = c.qds_bs; a.kds_bs = c.kds_bs; a.vds_bs = c.vds_bs;
    a.batch = c.batch; a.heads_q = c.heads_q; a.heads_kv = c.heads_kv; a.nq = c.nq; a.nk = c.nk; a.dtype = c.dtype;
    a.q_bs = c.batch > 1 ? c.q.bs : 0; a.q_hs = c.heads_q > 1 ? c.q.hs : 0; a.q_ts = c.nq > 1 ? c.q.ts : d;
    a.k_bs = c.batch > 1 ? c.k.bs : 0; a.k_hs = c.heads_kv > 1 ? c.k.hs : 0; a.k_ts = c.nk > 1 ? c.k.ts : d;
    a.v_bs = c.batch > 1 ? c.v.bs : 0; a.v_hs = c.heads_kv > 1 ? c.v.hs : 0; a.v_ts = c.nk > 1 ? c.v.ts : d;
    a.o_bs = c.batch > 1 ? c.o.bs : 0; a.o_hs = c.heads_q > 1 ? c.o.hs : 0; a.o_ts = c.nq > 1 ? c.o.ts : d;
    a.causal = c.causal != 0; a.scale = (float)c.scale; a.workspace = c.workspace; a.d = d;
    return launched(who, fa::launch_fp8_inputs_hdim(a, c.mod, reinterpret_cast<hipStream_t>(c.stream)));   // (d == 128: launch_fp8_inputs_mod)
}

size_t fa_fp8_forward_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t seqlen_k, int64_t d) {
    if (batch <= 0 || heads_kv <= 0 || seqlen_k <= 0 || d != 128) return 0;
    return fa::fp8in_workspace_bytes(batch * heads_kv, seqlen_k);
}

// the parent's size at d = 128; the V^T image is units_kv * tiles * d * 128 + 256 bytes
size_t fa_fp8_forward_hdim_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t seqlen_k, int64_t head_dim) {
    if (batch <= 0 || heads_kv <= 0 || seqlen_k <= 0 || (head_dim != 64 && head_dim != 128 && head_dim != 256)) return 0;
    return fa::fp8in_workspace_bytes(batch * heads_kv, seqlen_k, head_dim);
}

int fa_fp8_forward(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
                   const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k, int64_t d,
                   int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride,
                   int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
                   int64_t o_batch_stride, int64_t o_head_stride, int64_t o_token_stride, int64_t q_descale_batch_stride,
                   int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace,
                   size_t workspace_bytes, void* stream) {
    Fp8Call c;
    c.q.p = q; c.q.bs = q_batch_stride; c.q.hs = q_head_stride; c.q.ts = q_token_stride;
    c.k.p = k; c.k.bs = k_batch_stride; c.k.hs = k_head_stride; c.k.ts = k_token_stride;
    c.v.p = v; c.v.bs = v_batch_stride; c.v.hs = v_head_stride; c.v.ts = v_token_stride;
    c.o.p = o; c.o.bs = o_batch_stride; c.o.hs = o_head_stride; c.o.ts = o_token_stride;
    c.lse = lse; c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.nq = seqlen_q; c.nk = seqlen_k; c.d = d;
    c.dtype = dtype; c.causal = causal; c.scale = softmax_scale;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    return fp8_forward_impl("fa_fp8_forward", c);
}

// the arguments of fa_fp8_forward_mod and fa_fp8_forward_hdim alike (hdim: the head dims 64, 128 and 256)
static int fp8_forward_mod_entry(const char* who, bool hdim, const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k, int64_t d,
        int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
        int64_t o_batch_stride, int64_t o_head_stride, int64_t o_token_stride, int64_t q_descale_batch_stride,
        int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace,
        size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap, const float* sinks,
        int64_t sink_heads) {
    Fp8Call c;
    c.hdim = hdim;
    c.q.p = q; c.q.bs = q_batch_stride; c.q.hs = q_head_stride; c.q.ts = q_token_stride;
    c.k.p = k; c.k.bs = k_batch_stride; c.k.hs = k_head_stride; c.k.ts = k_token_stride;
    c.v.p = v; c.v.bs = v_batch_stride; c.v.hs = v_head_stride; c.v.ts = v_token_stride;
    c.o.p = o; c.o.bs = o_batch_stride; c.o.hs = o_head_stride; c.o.ts = o_token_stride;
    c.lse = lse; c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.nq = seqlen_q; c.nk = seqlen_k; c.d = d;
    c.dtype = dtype; c.causal = causal; c.scale = softmax_scale;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.mod.window_left = window_left; c.mod.window_right = window_right; c.mod.softcap = softcap; c.mod.sinks = sinks;
    c.mod.sink_heads = sink_heads;
    return fp8_forward_impl(who, c);
}

int fa_fp8_forward_mod(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k, int64_t d,
        int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
        int64_t o_batch_stride, int64_t o_head_stride, int64_t o_token_stride, int64_t q_descale_batch_stride,
        int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace,
        size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap, const float* sinks,
        int64_t sink_heads) {
    return fp8_forward_mod_entry("fa_fp8_forward_mod", false, q, k, v, o, lse, q_descale, k_descale, v_descale, batch, heads_q,
           heads_kv, seqlen_q, seqlen_k, d, dtype, q_batch_stride, q_head_stride, q_token_stride, k_batch_stride, k_head_stride,
           k_token_stride, v_batch_stride, v_head_stride, v_token_stride, o_batch_stride, o_head_stride, o_token_stride,
           q_descale_batch_stride, k_descale_batch_stride, v_descale_batch_stride, causal, softmax_scale, workspace, workspace_bytes,
           stream, window_left, window_right, softcap, sinks, sink_heads);
}

int fa_fp8_forward_hdim(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k, int64_t head_dim,
        int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
        int64_t o_batch_stride, int64_t o_head_stride, int64_t o_token_stride, int64_t q_descale_batch_stride,
        int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace,
        size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap, const float* sinks,
        int64_t sink_heads) {
    return fp8_forward_mod_entry("fa_fp8_forward_hdim", true, q, k, v, o, lse, q_descale, k_descale, v_descale, batch, heads_q,
           heads_kv, seqlen_q, seqlen_k, head_dim, dtype, q_batch_stride, q_head_stride, q_token_stride, k_batch_stride, k_head_stride,
           k_token_stride, v_batch_stride, v_head_stride, v_token_stride, o_batch_stride, o_head_stride, o_token_stride,
           q_descale_batch_stride, k_descale_batch_stride, v_descale_batch_stride, causal, softmax_scale, workspace, workspace_bytes,
           stream, window_left, window_right, softcap, sinks, sink_heads);
}

// ---- the packed and the paged form of the fp8 call: see include/fa_mi355x.h
// One call of fa_fp8_forward_varlen, a family of its own.
struct Fp8VarCall {
    bool hdim = false;                     // as Fp8Call's
    fa::Fp8Mod mod;
    const void *q = nullptr, *k = nullptr, *v = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const float *q_descale = nullptr, *k_descale = nullptr, *v_descale = nullptr;
    const int32_t *cu_q = nullptr, *cu_k = nullptr, *block_table = nullptr;
    int64_t batch = 0, heads_q = 0, heads_kv = 0, total_q = 0, total_k = 0, max_q = 0, max_k = 0, d = 0;
    int dtype = 0;
    int64_t q_ts = 0, q_hs = 0, k_ts = 0, k_hs = 0, v_ts = 0, v_hs = 0;
    int64_t max_blocks = 0, num_blocks = 0, ps = 0, k_ps = 0, v_ps = 0;
    int64_t qds_bs = 0, kds_bs = 0, vds_bs = 0;
    int causal = 0;
    double scale = 0.0;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    void* stream = nullptr;
};

static int fp8_forward_varlen_impl(const char* who, const Fp8VarCall& c) {
    const bool paged = c.block_table != nullptr;
    const int64_t kInt = ((int64_t)1 << 31) - 1;
    // (1) null pointers
    if (!c.q || !c.k || !c.v || !c.o || !c.lse) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (!c.cu_q || !c.cu_k) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null cu_seqlens pointer", who);
    // (2) dims
    if (c.batch <= 0 || c.heads_q <= 0 || c.heads_kv <= 0 || c.d <= 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch, heads_q, heads_kv and d must be > 0 (got %lld, %lld, %lld, %lld)", who,
                    (long long)c.batch, (long long)c.heads_q, (long long)c.heads_kv, (long long)c.d);
    if (c.total_q < 0 || c.total_k < 0 || c.max_q < 0 || c.max_k < 0 || c.total_q > kInt || c.total_k > kInt || c.max_q > kInt || c.max_k > kInt ||
        c.batch >= kInt)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_q, total_k, max_seqlen_q and max_seqlen_k must lie in [0, 2^31) (got %lld, %lld, %lld, %lld)",
                    who, (long long)c.total_q, (long long)c.total_k, (long long)c.max_q, (long long)c.max_k);
    // (3) the head dim
    if (const int rc = fp8_head_dim_check(who, c.d, c.hdim)) return rc;
    const int64_t d = c.d;
    // (4) the heads ratio
    if (c.heads_q % c.heads_kv != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_q=%lld must be a multiple of heads_kv=%lld", who, (long long)c.heads_q, (long long)c.heads_kv);
    // (5) the output dtype, the scale
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: dtype (of o) must be f16 or bf16 (got code %d)", who, c.dtype);
    if (!(c.scale == c.scale) || !scale_ok(c.scale))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be finite and > 0", who);
    if (const int rc = fp8_mod_check(who, c.mod, c.heads_q)) return rc;
    // (6) the pages
    if (paged) {
        if (c.ps < 16 || c.ps % 16 != 0 || c.ps > 65536)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: page_block_size must be a multiple of 16 in [16, 65536] (got %lld)", who, (long long)c.ps);
        if (c.num_blocks < 1 || c.num_blocks > kInt)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_blocks must lie in [1, 2^31) (got %lld)", who, (long long)c.num_blocks);
        if (c.max_blocks < 0 || c.max_blocks > kInt / c.batch)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch * max_blocks_per_seq must lie in [0, 2^31) (got max_blocks_per_seq=%lld)", who,
                        (long long)c.max_blocks);
    } else if (c.max_blocks != 0 || c.num_blocks != 0 || c.ps != 0 || c.k_ps != 0 || c.v_ps != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_blocks_per_seq, num_blocks, page_block_size and the page strides must be 0 without block_table", who);
    }
    // (7) the descale strides
    const struct { const char* name; const float* p; int64_t bs; } ds[3] = {
        {"q_descale", c.q_descale, c.qds_bs}, {"k_descale", c.k_descale, c.kds_bs}, {"v_descale", c.v_descale, c.vds_bs}};
    for (const auto& s : ds) {
        if (!s.p && s.bs != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s_batch_stride must be 0 without %s", who, s.name, s.name);
        if (s.bs < 0 || (s.bs != 0 && s.bs < c.heads_kv) || s.bs >= ((int64_t)1 << 31) / c.batch)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s_batch_stride=%lld must be 0 or >= heads_kv=%lld", who, s.name, (long long)s.bs,
                        (long long)c.heads_kv);
        if ((uintptr_t)s.p % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", who, s.name);
    }
    // (8) alignment and strides: 16-byte units, rows that do not overlap
    if (!aligned16({c.q, c.k, c.v, c.o})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q, k, v and o must be 16-byte aligned", who);
    if ((uintptr_t)c.lse % 4 != 0 || (uintptr_t)c.cu_q % 4 != 0 || (uintptr_t)c.cu_k % 4 != 0 || (uintptr_t)c.block_table % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: lse, cu_seqlens_q, cu_seqlens_k and block_table must be 4-byte aligned", who);
    const int64_t kMaxStride = (int64_t)1 << 44;
    const struct { const char* name; int64_t ts, hs, heads, ps; } ts[3] = {
        {"q", c.q_ts, c.q_hs, c.heads_q, 0}, {"k", c.k_ts, c.k_hs, c.heads_kv, c.k_ps}, {"v", c.v_ts, c.v_hs, c.heads_kv, c.v_ps}};
    for (const auto& t : ts) {
        const int64_t hs = t.heads > 1 ? t.hs : 0;
        if (t.ts % 16 != 0 || hs % 16 != 0 || t.ps % 16 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (token %lld, head %lld, page %lld) must be multiples of 16 bytes", who, t.name,
                        (long long)t.ts, (long long)t.hs, (long long)t.ps);
        if (t.ts < d || hs < 0 || t.ps < 0 || t.ts > kMaxStride || hs > kMaxStride || t.ps > kMaxStride)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (token %lld, head %lld, page %lld) must be >= 0, the token stride >= %lld", who,
                        t.name, (long long)t.ts, (long long)t.hs, (long long)t.ps, (long long)d);
    }
    // (9) the span limits: q, packed k and one page are read through 32-bit buffer descriptors and offsets
    const int64_t kSpan = ((int64_t)1 << 31) - 1;
    const int64_t q_span = (c.max_q + 255) / 256 * 256 * c.q_ts;
    if (q_span > kSpan)
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: round_up(max_seqlen_q, 256) * token stride of q is %lld bytes, at or above 2^31", who,
                    (long long)q_span);
    const int64_t cap = paged ? std::min(c.max_k, c.max_blocks * c.ps) : c.max_k;
    if (paged) {
        const int64_t kp = c.ps * c.k_ts, vp = c.ps * c.v_ts;
        if (kp > kSpan || vp > kSpan)
            return fail(FA_ERR_UNSUPPORTED, "%s: span limit: page_block_size * token stride of %s is %lld bytes, at or above 2^31", who,
                        kp > kSpan ? "k" : "v", (long long)(kp > kSpan ? kp : vp));
        if (cap >= ((int64_t)1 << 24))
            return fail(FA_ERR_UNSUPPORTED, "%s: span limit: min(max_seqlen_k, max_blocks_per_seq * page_block_size) = %lld is at or above 2^24", who,
                        (long long)cap);
    } else {
        const int64_t k_span = (c.max_k + 255) / 256 * 256 * c.k_ts;
        if (k_span > kSpan)
            return fail(FA_ERR_UNSUPPORTED, "%s: span limit: round_up(max_seqlen_k, 256) * token stride of k is %lld bytes, at or above 2^31", who,
                        (long long)k_span);
    }
    fa::Fp8InVarArgs a;
    a.batch = c.batch; a.heads_q = c.heads_q; a.heads_kv = c.heads_kv; a.total_q = c.total_q; a.total_k = paged ? 0 : c.total_k;
    a.max_q = c.max_q; a.max_k = c.max_k; a.max_blocks = c.max_blocks; a.num_blocks = c.num_blocks; a.page_size = c.ps; a.d = d;
    const int64_t nqt = (c.max_q + 255) / 256, nbmax = (cap + 63) / 64, tiles = fa::fp8in_varlen_workspace_bytes(a) / (128 * d);
    if ((nqt > 0 && c.batch * c.heads_q >= ((int64_t)1 << 31) / nqt) || (nbmax > 0 && c.batch * c.heads_kv >= ((int64_t)1 << 31) / nbmax) ||
        tiles >= ((int64_t)1 << 31))
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: batch * heads * tiles too large for one launch", who);
    // (10) the workspace
    const size_t need = fa::fp8in_varlen_workspace_bytes(a);
    if (!c.workspace || c.workspace_bytes < need)
        return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes is too small (need %zu: fa_fp8_forward_varlen%s_workspace_bytes)", who,
                    c.workspace ? c.workspace_bytes : (size_t)0, need, c.hdim ? "_hdim" : "");
    if ((uintptr_t)c.workspace % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);

    a.q = c.q; a.k = c.k; a.v = c.v; a.o = c.o; a.lse = c.lse;
    a.q_descale = c.q_descale; a.k_descale = c.k_descale; a.v_descale = c.v_descale;
    a.qds_bs = c.qds_bs; a.kds_bs = c.kds_bs; a.vds_bs = c.vds_bs;
    a.cu_q = c.cu_q; a.cu_k = c.cu_k; a.block_table = c.block_table;
    a.dtype = c.dtype;
    a.q_ts = c.q_ts; a.q_hs = c.heads_q > 1 ? c.q_hs : 0; a.k_ts = c.k_ts; a.k_hs = c.heads_kv > 1 ? c.k_hs : 0;
    a.v_ts = c.v_ts; a.v_hs = c.heads_kv > 1 ? c.v_hs : 0; a.k_ps = c.k_ps; a.v_ps = c.v_ps;
    a.causal = c.causal != 0; a.scale = (float)c.scale; a.workspace = c.workspace;
    return launched(who, fa::launch_fp8_inputs_varlen_hdim(a, c.mod, reinterpret_cast<hipStream_t>(c.stream)));   // (d == 128: .._varlen_mod)
}

static size_t fp8_varlen_ws(int64_t batch, int64_t heads_kv, int64_t total_k, int64_t max_seqlen_k, int64_t max_blocks_per_seq,
                            int64_t page_block_size, int64_t d, bool hdim) {
    const int64_t kInt = ((int64_t)1 << 31) - 1;
    if (batch <= 0 || heads_kv <= 0 || total_k < 0 || max_seqlen_k < 0 || max_blocks_per_seq < 0 || page_block_size < 0) return 0;
    if (hdim ? (d != 64 && d != 128 && d != 256) : d != 128) return 0;
    if (batch > kInt || total_k > kInt || max_seqlen_k > kInt || max_blocks_per_seq > kInt || page_block_size > 65536) return 0;
    if (page_block_size % 16 != 0) return 0;
    fa::Fp8InVarArgs a;
    a.batch = batch; a.heads_kv = heads_kv; a.total_k = page_block_size ? 0 : total_k; a.max_k = max_seqlen_k;
    a.max_blocks = page_block_size ? max_blocks_per_seq : 0; a.page_size = page_block_size; a.d = d;
    return fa::fp8in_varlen_workspace_bytes(a);
}

size_t fa_fp8_forward_varlen_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t total_k, int64_t max_seqlen_k, int64_t max_blocks_per_seq,
                                             int64_t page_block_size, int64_t d) {
    return fp8_varlen_ws(batch, heads_kv, total_k, max_seqlen_k, max_blocks_per_seq, page_block_size, d, false);
}

size_t fa_fp8_forward_varlen_hdim_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t total_k, int64_t max_seqlen_k,
                                                  int64_t max_blocks_per_seq, int64_t page_block_size, int64_t head_dim) {
    return fp8_varlen_ws(batch, heads_kv, total_k, max_seqlen_k, max_blocks_per_seq, page_block_size, head_dim, true);
}

int fa_fp8_forward_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
                          const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, const int32_t* block_table,
                          int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q,
                          int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_token_stride, int64_t q_head_stride, int64_t k_token_stride,
                          int64_t k_head_stride, int64_t v_token_stride, int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks,
                          int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride,
                          int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace,
                          size_t workspace_bytes, void* stream) {
    Fp8VarCall c;
    c.q = q; c.k = k; c.v = v; c.o = o; c.lse = lse; c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.block_table = block_table;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.total_q = total_q; c.total_k = total_k; c.max_q = max_seqlen_q;
    c.max_k = max_seqlen_k; c.d = d; c.dtype = dtype;
    c.q_ts = q_token_stride; c.q_hs = q_head_stride; c.k_ts = k_token_stride; c.k_hs = k_head_stride; c.v_ts = v_token_stride;
    c.v_hs = v_head_stride;
    c.max_blocks = max_blocks_per_seq; c.num_blocks = num_blocks; c.ps = page_block_size; c.k_ps = k_page_stride; c.v_ps = v_page_stride;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    return fp8_forward_varlen_impl("fa_fp8_forward_varlen", c);
}

// the arguments of fa_fp8_forward_varlen_mod and fa_fp8_forward_varlen_hdim alike (hdim: the head dims 64, 128 and 256)
static int fp8_forward_varlen_mod_entry(const char* who, bool hdim, const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, const int32_t* block_table, int64_t batch,
        int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d,
        int dtype, int64_t q_token_stride, int64_t q_head_stride, int64_t k_token_stride, int64_t k_head_stride,
        int64_t v_token_stride, int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks, int64_t page_block_size,
        int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
        int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads) {
    Fp8VarCall c;
    c.hdim = hdim;
    c.q = q; c.k = k; c.v = v; c.o = o; c.lse = lse; c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.block_table = block_table;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.total_q = total_q; c.total_k = total_k; c.max_q = max_seqlen_q;
    c.max_k = max_seqlen_k; c.d = d; c.dtype = dtype;
    c.q_ts = q_token_stride; c.q_hs = q_head_stride; c.k_ts = k_token_stride; c.k_hs = k_head_stride; c.v_ts = v_token_stride;
    c.v_hs = v_head_stride;
    c.max_blocks = max_blocks_per_seq; c.num_blocks = num_blocks; c.ps = page_block_size; c.k_ps = k_page_stride; c.v_ps = v_page_stride;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.mod.window_left = window_left; c.mod.window_right = window_right; c.mod.softcap = softcap; c.mod.sinks = sinks;
    c.mod.sink_heads = sink_heads;
    return fp8_forward_varlen_impl(who, c);
}

int fa_fp8_forward_varlen_mod(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, const int32_t* block_table, int64_t batch,
        int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d,
        int dtype, int64_t q_token_stride, int64_t q_head_stride, int64_t k_token_stride, int64_t k_head_stride,
        int64_t v_token_stride, int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks, int64_t page_block_size,
        int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
        int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads) {
    return fp8_forward_varlen_mod_entry("fa_fp8_forward_varlen_mod", false, q, k, v, o, lse, q_descale, k_descale, v_descale,
           cu_seqlens_q, cu_seqlens_k, block_table, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k, d, dtype,
           q_token_stride, q_head_stride, k_token_stride, k_head_stride, v_token_stride, v_head_stride, max_blocks_per_seq, num_blocks,
           page_block_size, k_page_stride, v_page_stride, q_descale_batch_stride, k_descale_batch_stride, v_descale_batch_stride,
           causal, softmax_scale, workspace, workspace_bytes, stream, window_left, window_right, softcap, sinks, sink_heads);
}

int fa_fp8_forward_varlen_hdim(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, const int32_t* block_table, int64_t batch,
        int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k,
        int64_t head_dim, int dtype, int64_t q_token_stride, int64_t q_head_stride, int64_t k_token_stride, int64_t k_head_stride,
        int64_t v_token_stride, int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks, int64_t page_block_size,
        int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
        int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads) {
    return fp8_forward_varlen_mod_entry("fa_fp8_forward_varlen_hdim", true, q, k, v, o, lse, q_descale, k_descale, v_descale,
           cu_seqlens_q, cu_seqlens_k, block_table, batch, heads_q, heads_kv, total_q, total_k, max_seqlen_q, max_seqlen_k, head_dim,
           dtype, q_token_stride, q_head_stride, k_token_stride, k_head_stride, v_token_stride, v_head_stride, max_blocks_per_seq,
           num_blocks, page_block_size, k_page_stride, v_page_stride, q_descale_batch_stride, k_descale_batch_stride,
           v_descale_batch_stride, causal, softmax_scale, workspace, workspace_bytes, stream, window_left, window_right, softcap, sinks,
           sink_heads);
}

// ---- fp8 KV-cache decoding with split-KV (e4m3 q over an e4m3 cache): see include/fa_mi355x.h
// One call of fa_fp8_forward_kvcache, a family of its own.
struct Fp8KvCall {
    bool hdim = false;                     // as Fp8Call's
    fa::Fp8Mod mod;
    const void *q = nullptr, *k_cache = nullptr, *v_cache = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const float *q_descale = nullptr, *k_descale = nullptr, *v_descale = nullptr;
    const int32_t *cache_seqlens = nullptr, *block_table = nullptr, *cache_batch_idx = nullptr;
    int64_t batch = 0, heads_q = 0, heads_kv = 0, seqlen_q = 0, cache_len = 0, cache_batch = 0, d = 0;
    int dtype = 0, q_dtype = 0, cache_dtype = 0;
    int64_t q_bs = 0, q_ts = 0, k_bs = 0, k_ts = 0, v_bs = 0, v_ts = 0;
    int64_t table_rs = 0, num_blocks = 0, ps = 0;
    int64_t qds_bs = 0, kds_bs = 0, vds_bs = 0;
    int causal = 0;
    double scale = 0.0;
    int64_t num_splits = 0;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    void* stream = nullptr;
    // the _varlen entry points (varlen: one of them was called; its packed group, all null / 0: the padded call)
    bool varlen = false;
    const int32_t* cu_seqlens_q = nullptr;
    int64_t total_q = 0, max_seqlen_q = 0;
};

static int64_t fp8_kv_splits(int64_t batch, int64_t hq, int64_t hkv, int64_t nq, int64_t cache_len, int64_t num_splits) {
    if (num_splits > 0) return num_splits;
    return fa::fp8kv_num_splits(batch, hq, hkv, nq, cache_len);
}

// the featured call: the rule sees the keys a window can show instead of the capacity, and sinks raise 1 split to 2 (the sink
// joins in the combine, which such a call always runs)
static int64_t fp8_kv_splits_mod(int64_t batch, int64_t hq, int64_t hkv, int64_t nq, int64_t cache_len, int64_t num_splits, int causal,
                                 const fa::Fp8Mod& m) {
    const int64_t S = fp8_kv_splits(batch, hq, hkv, nq, fa::fp8kv_split_len(cache_len, nq, causal, m), num_splits);
    return m.sinks && S < 2 ? 2 : S;
}

// What fa_fp8_kvcache_step adds to fa_fp8_forward_kvcache_mod's arguments: the new tokens, the q8 buffer and the rotary tables
struct Fp8StepCall {
    const void *k_new = nullptr, *v_new = nullptr;
    int64_t seqlen_new = 0, kn_bs = 0, kn_ts = 0, vn_bs = 0, vn_ts = 0;
    int in_dtype = 0;
    void* q8_out = nullptr;
    int64_t q8_bs = 0, q8_ts = 0;
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;
    int64_t cos_rs = 0, sin_rs = 0, seqlen_ro = 0, rotary_dim = 0;
    int rotary_interleaved = 0;
    const int32_t* cu_seqlens_k_new = nullptr;   // fa_fp8_kvcache_step_varlen
    int64_t total_k_new = 0;
};

// The rules of fa_fp8_forward_kvcache[_mod] (st == null) and of fa_fp8_kvcache_step (st: what it adds), in the header's order.
// With packed queries (c.cu_seqlens_q; the _varlen entry points) seqlen_q and q's batch stride are not looked at, nor seqlen_new
// and the batch strides of k_new / v_new with cu_seqlens_k_new; the rules of the packed group follow the parents' (9).
// FA_OK: `empty` says that there is nothing to launch; otherwise S is the number of splits and need the workspace's bytes.
static int fp8_kvcache_check(const char* who, const Fp8KvCall& c, const Fp8StepCall* st, bool& empty, int64_t& S, size_t& need) {
    const bool paged = c.block_table != nullptr;
    const int64_t kInt = ((int64_t)1 << 31) - 1;
    const int64_t kMaxStride = (int64_t)1 << 44;
    const int64_t qe = st && c.q_dtype != FA_DTYPE_E4M3 ? 2 : 1;   // bytes an element of q (and of k_new, v_new)
    const bool packed = c.cu_seqlens_q != nullptr, packed_kn = st && st->cu_seqlens_k_new != nullptr;
    const int64_t q_bs = packed ? 0 : c.q_bs;                      // (packed: not used)
    const int64_t nq = packed ? c.max_seqlen_q : c.seqlen_q;       // the most query tokens a sequence has
    empty = false;
    // (0) the empty call
    if (c.batch == 0 || (!st && !packed && c.seqlen_q == 0) || (!st && packed && (c.total_q == 0 || c.max_seqlen_q == 0))) {
        empty = true;
        return FA_OK;
    }
    // (1) null pointers
    if (!c.q || !c.k_cache || !c.v_cache || !c.o || !c.lse) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer", who);
    if (st && (!st->k_new || !st->v_new)) return fail(FA_ERR_INVALID_ARGUMENT, "%s: null tensor pointer (k_new, v_new)", who);
    if (st && !c.cache_seqlens)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_seqlens is required (the lengths before the append)", who);
    // (2) the head dim and the dtypes
    if (const int rc = fp8_head_dim_check(who, c.d, c.hdim)) return rc;
    const int64_t d = c.d;
    if (st) {
        if (c.q_dtype != FA_DTYPE_F16 && c.q_dtype != FA_DTYPE_BF16 && c.q_dtype != FA_DTYPE_E4M3)
            return fail(FA_ERR_UNSUPPORTED, "%s: q_dtype must be f16, bf16 or FA_DTYPE_E4M3 (got code %d)", who, c.q_dtype);
        if (st->in_dtype != c.q_dtype)
            return fail(FA_ERR_UNSUPPORTED, "%s: mixed dtypes: q, k_new and v_new must be all f16, all bf16 or all e4m3 (q_dtype code %d, "
                        "in_dtype code %d)", who, c.q_dtype, st->in_dtype);
    } else if (c.q_dtype != FA_DTYPE_E4M3)
        return fail(FA_ERR_UNSUPPORTED, "%s: q_dtype must be FA_DTYPE_E4M3 (got code %d; a 16-bit q is fa_ex_forward_kvcache_fp8's)", who,
                    c.q_dtype);
    if (c.cache_dtype != FA_DTYPE_E4M3)
        return fail(FA_ERR_UNSUPPORTED, "%s: cache_dtype must be FA_DTYPE_E4M3 (got code %d)", who, c.cache_dtype);
    if (c.dtype != FA_DTYPE_F16 && c.dtype != FA_DTYPE_BF16)
        return fail(FA_ERR_UNSUPPORTED, "%s: dtype (of o) must be f16 or bf16 (got code %d)", who, c.dtype);
    // (3) the heads ratio
    if (c.heads_kv < 1 || c.heads_q < 1 || c.heads_q % c.heads_kv != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: heads_q=%lld must be a positive multiple of heads_kv=%lld", who, (long long)c.heads_q,
                    (long long)c.heads_kv);
    // (4) ranges
    if (c.batch < 1 || c.batch > 65535) return fail(FA_ERR_INVALID_ARGUMENT, "%s: batch must lie in [1, 65535] (got %lld)", who, (long long)c.batch);
    if (!packed && c.seqlen_q < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_q must be >= 1 (got %lld)", who, (long long)c.seqlen_q);
    if (c.cache_len < 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_len must be >= 1 (got %lld)", who, (long long)c.cache_len);
    if (st && !packed_kn && (st->seqlen_new < 1 || st->seqlen_new > c.cache_len))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: seqlen_new=%lld must lie in [1, cache_len=%lld]", who, (long long)st->seqlen_new,
                    (long long)c.cache_len);
    if (c.heads_q > ((int64_t)1 << 20) || (!packed && (c.seqlen_q > ((int64_t)1 << 20) || (c.heads_q / c.heads_kv) * c.seqlen_q > ((int64_t)1 << 20))))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: (heads_q / heads_kv) * seqlen_q = %lld * %lld must be <= 2^20", who,
                    (long long)(c.heads_q / c.heads_kv), (long long)c.seqlen_q);
    if (!(c.scale == c.scale) || !scale_ok(c.scale))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: softmax_scale must be finite and > 0", who);
    if (c.cache_batch_idx) {
        if (c.cache_batch < 1 || c.cache_batch > kInt)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch must lie in [1, 2^31) with cache_batch_idx (got %lld)", who,
                        (long long)c.cache_batch);
    } else if (c.cache_batch != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_batch must be 0 without cache_batch_idx (got %lld)", who, (long long)c.cache_batch);
    }
    // (5) alignment and strides
    if (!aligned16({c.q, c.k_cache, c.v_cache, c.o})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q, k_cache, v_cache and o must be 16-byte aligned", who);
    if ((uintptr_t)c.lse % 4 != 0 || (uintptr_t)c.cache_seqlens % 4 != 0 || (uintptr_t)c.block_table % 4 != 0 || (uintptr_t)c.cache_batch_idx % 4 != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: lse, cache_seqlens, block_table and cache_batch_idx must be 4-byte aligned", who);
    if (st && !aligned16({st->k_new, st->v_new})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: k_new and v_new must be 16-byte aligned", who);
    // (heads: the elements of a token's heads over d, in bytes for a 16-bit q, k_new, v_new)
    const struct { const char* name; int64_t bs, ts, heads; } ts[5] = {
        {"q", q_bs, c.q_ts, c.heads_q * qe}, {"k_cache", c.k_bs, c.k_ts, c.heads_kv}, {"v_cache", c.v_bs, c.v_ts, c.heads_kv},
        {"k_new", st && !packed_kn ? st->kn_bs : 0, st ? st->kn_ts : 0, c.heads_kv * qe},
        {"v_new", st && !packed_kn ? st->vn_bs : 0, st ? st->vn_ts : 0, c.heads_kv * qe}};
    for (int i = 0; i < (st ? 5 : 3); ++i) {
        const auto& t = ts[i];
        if (t.ts % 16 != 0 || t.bs % 16 != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (batch %lld, token %lld) must be multiples of 16 bytes", who, t.name,
                        (long long)t.bs, (long long)t.ts);
        if (t.ts < t.heads * d || t.ts > kMaxStride || t.bs < 0 || t.bs > kMaxStride)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of %s (batch %lld, token %lld) must be >= 0, the token stride >= heads * %lld = %lld",
                        who, t.name, (long long)t.bs, (long long)t.ts, (long long)d, (long long)(t.heads * d));
    }
    if (st && st->q8_out) {
        if (qe == 1) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q8_out goes with a 16-bit q only (an e4m3 q is used in place)", who);
        if (!aligned16({st->q8_out})) return fail(FA_ERR_INVALID_ARGUMENT, "%s: q8_out must be 16-byte aligned", who);
        const int64_t q8_bs = packed ? 0 : st->q8_bs;              // (packed: not used)
        if (st->q8_ts % 16 != 0 || q8_bs % 16 != 0 || st->q8_ts < c.heads_q * d || st->q8_ts > kMaxStride || q8_bs < 0 || q8_bs > kMaxStride)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: the strides of q8_out (batch %lld, token %lld) must be multiples of 16 bytes and >= 0, "
                        "the token stride >= heads_q * %lld = %lld", who, (long long)q8_bs, (long long)st->q8_ts, (long long)d,
                        (long long)(c.heads_q * d));
    } else if (st && (st->q8_bs != 0 || st->q8_ts != 0)) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: q8_batch_stride and q8_token_stride must be 0 without q8_out", who);
    }
    // (6) the descale strides
    const struct { const char* name; const float* p; int64_t bs; } ds[3] = {
        {"q_descale", c.q_descale, c.qds_bs}, {"k_descale", c.k_descale, c.kds_bs}, {"v_descale", c.v_descale, c.vds_bs}};
    for (const auto& s : ds) {
        if (!s.p && s.bs != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s_batch_stride must be 0 without %s", who, s.name, s.name);
        if (s.bs < 0 || (s.bs != 0 && s.bs < c.heads_kv) || s.bs >= ((int64_t)1 << 31) / c.batch)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s_batch_stride=%lld must be 0 or >= heads_kv=%lld", who, s.name, (long long)s.bs,
                        (long long)c.heads_kv);
        if ((uintptr_t)s.p % 4 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", who, s.name);
    }
    // (7) the pages
    if (paged) {
        if (c.cache_batch_idx) return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table cannot be combined with cache_batch_idx", who);
        if (c.ps < 16 || c.ps % 16 != 0 || c.ps > 65536)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: page_block_size must be a multiple of 16 in [16, 65536] (got %lld)", who, (long long)c.ps);
        if (c.cache_len % c.ps != 0)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: cache_len=%lld (the capacity) must be a multiple of page_block_size=%lld", who,
                        (long long)c.cache_len, (long long)c.ps);
        if (c.num_blocks < 1 || c.num_blocks > kInt)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_blocks must lie in [1, 2^31) (got %lld)", who, (long long)c.num_blocks);
        if (c.table_rs < c.cache_len / c.ps || c.table_rs > ((int64_t)1 << 40))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table_row_stride=%lld must be >= max_blocks_per_seq=%lld (and <= 2^40)", who,
                        (long long)c.table_rs, (long long)(c.cache_len / c.ps));
    } else if (c.table_rs != 0 || c.num_blocks != 0 || c.ps != 0) {
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: block_table_row_stride, num_blocks and page_block_size must be 0 without block_table", who);
    }
    // (8) the span limits: 32-bit byte offsets inside one batch element or page
    const int64_t kSpan = ((int64_t)1 << 31) - 1;
    const int64_t c_n = paged ? c.ps : c.cache_len;
    const int64_t q_span = packed ? 0 : c.seqlen_q * c.q_ts, k_span = c_n * c.k_ts, v_span = c_n * c.v_ts;   // (packed: rule (P5))
    if (q_span > kSpan || k_span > kSpan || v_span > kSpan)
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: tokens * token stride of %s is %lld bytes, at or above 2^31", who,
                    q_span > kSpan ? "q" : k_span > kSpan ? "k_cache" : "v_cache", (long long)(q_span > kSpan ? q_span : k_span > kSpan ? k_span : v_span));
    if (c.cache_len >= ((int64_t)1 << 28))
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: cache_len = %lld (the capacity) is at or above 2^28", who, (long long)c.cache_len);
    const int64_t row_tiles = packed ? 0 : ((c.heads_q / c.heads_kv) * c.seqlen_q + 31) / 32;   // (packed: rule (P6))
    if (row_tiles * c.heads_kv > 65535)
        return fail(FA_ERR_UNSUPPORTED, "%s: span limit: row tiles * heads_kv = %lld is beyond 65535 for one launch", who,
                    (long long)(row_tiles * c.heads_kv));
    if (st) {
        // (packed new keys: the kernel addresses their rows in 64 bits; packed queries: rule (P5))
        const int64_t kn_span = packed_kn ? 0 : st->seqlen_new * st->kn_ts, vn_span = packed_kn ? 0 : st->seqlen_new * st->vn_ts;
        const int64_t q8_span = packed ? 0 : c.seqlen_q * st->q8_ts;
        if (kn_span > kSpan || vn_span > kSpan || q8_span > kSpan)
            return fail(FA_ERR_UNSUPPORTED, "%s: span limit: tokens * token stride of %s is %lld bytes, at or above 2^31", who,
                        kn_span > kSpan ? "k_new" : vn_span > kSpan ? "v_new" : "q8_out",
                        (long long)(kn_span > kSpan ? kn_span : vn_span > kSpan ? vn_span : q8_span));
        // the rotary tables (the step's rule (9)): read on the device without a check, so every position a clamped length can give
        // (new key n at L_b + n, q token i at L_b + i, L_b <= cache_len - seqlen_new) must be a table row
        if ((st->rotary_cos != nullptr) != (st->rotary_sin != nullptr))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must be given together", who);
        if (st->rotary_cos) {
            if (qe == 1)
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos / rotary_sin go with 16-bit q, k_new, v_new only (e4m3 codes cannot be rotated)", who);
            if (st->rotary_dim < 16 || st->rotary_dim > d || st->rotary_dim % 16 != 0)
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_dim must be a multiple of 16 in [16, %lld] (got %lld)", who, (long long)d,
                            (long long)st->rotary_dim);
            const int64_t ro_need = c.cache_len + (c.seqlen_q > st->seqlen_new ? c.seqlen_q - st->seqlen_new : 0);
            if (!packed && st->seqlen_ro < ro_need)
                return fail(FA_ERR_INVALID_ARGUMENT,
                            "%s: seqlen_ro=%lld must be >= capacity + max(0, seqlen_q - seqlen_new) = %lld (the tables are not bounds-checked on the device)",
                            who, (long long)st->seqlen_ro, (long long)ro_need);
            if (st->cos_rs < st->rotary_dim / 2 || st->sin_rs < st->rotary_dim / 2 || st->cos_rs > ((int64_t)1 << 40) || st->sin_rs > ((int64_t)1 << 40))
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be >= rotary_dim / 2 = %lld (and <= 2^40)", who,
                            (long long)st->cos_rs, (long long)st->sin_rs, (long long)(st->rotary_dim / 2));
            if (st->cos_rs % 2 != 0 || st->sin_rs % 2 != 0)
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary row strides (%lld, %lld) must be even", who, (long long)st->cos_rs,
                            (long long)st->sin_rs);
            if ((uintptr_t)st->rotary_cos % 4 != 0 || (uintptr_t)st->rotary_sin % 4 != 0)
                return fail(FA_ERR_INVALID_ARGUMENT, "%s: rotary_cos and rotary_sin must be 4-byte aligned", who);
        } else if (st->cos_rs != 0 || st->sin_rs != 0 || st->seqlen_ro != 0 || st->rotary_dim != 0 || st->rotary_interleaved != 0) {
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: the rotary row strides, seqlen_ro, rotary_dim and rotary_interleaved must be 0 without rotary_cos / rotary_sin", who);
        }
    }
    // (9) the splits
    if (c.num_splits < 0 || c.num_splits > 256)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: num_splits must lie in [0, 256] (got %lld)", who, (long long)c.num_splits);
    if (const int rc = fp8_mod_check(who, c.mod, c.heads_q)) return rc;
    // (P) the packed group of the _varlen entry points (every other entry point hands nulls and zeros on)
    // (P1) no extent without its array
    if (!packed && (c.total_q != 0 || c.max_seqlen_q != 0))
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_q and max_seqlen_q must be 0 without cu_seqlens_q (got %lld, %lld)", who,
                    (long long)c.total_q, (long long)c.max_seqlen_q);
    if (st && !packed_kn && st->total_k_new != 0)
        return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_k_new must be 0 without cu_seqlens_k_new (got %lld)", who, (long long)st->total_k_new);
    // (P2) packed new keys go with packed queries
    if (packed_kn && !packed) return fail(FA_ERR_INVALID_ARGUMENT, "%s: cu_seqlens_k_new needs cu_seqlens_q (packed new keys go with packed queries)", who);
    if (packed) {
        // (P3), (P4) the extents
        if (c.max_seqlen_q < 0 || c.max_seqlen_q > c.total_q)
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: max_seqlen_q=%lld must lie in [0, total_q=%lld]", who, (long long)c.max_seqlen_q,
                        (long long)c.total_q);
        if (c.total_q > kInt || (st && (st->total_k_new < 0 || st->total_k_new > kInt)))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: total_q=%lld and total_k_new=%lld must lie in [0, 2^31)", who, (long long)c.total_q,
                        (long long)(st ? st->total_k_new : 0));
        // (P5) the span limit of one sequence's tokens
        const int64_t pq_span = c.max_seqlen_q * c.q_ts, pq8_span = st ? c.max_seqlen_q * st->q8_ts : 0;
        if (pq_span > kSpan || pq8_span > kSpan)
            return fail(FA_ERR_UNSUPPORTED, "%s: span limit: max_seqlen_q * token stride of %s is %lld bytes, at or above 2^31", who,
                        pq_span > kSpan ? "q" : "q8_out", (long long)(pq_span > kSpan ? pq_span : pq8_span));
        // (P6) the rows of one sequence
        if (c.max_seqlen_q > ((int64_t)1 << 20) || (c.heads_q / c.heads_kv) * c.max_seqlen_q > ((int64_t)1 << 20))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: (heads_q / heads_kv) * max_seqlen_q = %lld * %lld must be <= 2^20", who,
                        (long long)(c.heads_q / c.heads_kv), (long long)c.max_seqlen_q);
        const int64_t prow_tiles = ((c.heads_q / c.heads_kv) * c.max_seqlen_q + 31) / 32;
        if (prow_tiles * c.heads_kv > 65535)
            return fail(FA_ERR_UNSUPPORTED, "%s: span limit: row tiles * heads_kv = %lld is beyond 65535 for one launch", who,
                        (long long)(prow_tiles * c.heads_kv));
        // (P7) the rotary tables: q token i of a sequence sits at L_b + i, L_b <= cache_len
        if (st && st->rotary_cos && st->seqlen_ro < c.cache_len + c.max_seqlen_q)
            return fail(FA_ERR_INVALID_ARGUMENT,
                        "%s: seqlen_ro=%lld must be >= capacity + max_seqlen_q = %lld (the tables are not bounds-checked on the device)", who,
                        (long long)st->seqlen_ro, (long long)(c.cache_len + c.max_seqlen_q));
        // (P8) alignment
        if ((uintptr_t)c.cu_seqlens_q % 4 != 0 || (st && (uintptr_t)st->cu_seqlens_k_new % 4 != 0))
            return fail(FA_ERR_INVALID_ARGUMENT, "%s: cu_seqlens_q and cu_seqlens_k_new must be 4-byte aligned", who);
    }
    S = fp8_kv_splits_mod(c.batch, c.heads_q, c.heads_kv, nq, c.cache_len, c.num_splits, c.causal, c.mod);
    // (10) the workspace
    need = packed ? fa::kv_workspace_bytes(1, c.heads_q, c.total_q, d, (int)S) : fa::kv_workspace_bytes(c.batch, c.heads_q, c.seqlen_q, d, (int)S);
    if (st && c.varlen) need += fa::fp8kv_step_prep_bytes_varlen(c.batch, packed ? c.total_q : c.batch * c.seqlen_q, c.heads_q, d, qe == 2 && !st->q8_out);
    else if (st) need += fa::fp8kv_step_prep_bytes(c.batch, c.heads_q, c.seqlen_q, qe == 2 && !st->q8_out);
    if (need > 0) {
        if (!c.workspace || c.workspace_bytes < need)
            return fail(FA_ERR_WORKSPACE, "%s: workspace of %zu bytes is too small (need %zu: %s%s)", who,
                        c.workspace ? c.workspace_bytes : (size_t)0, need,
                        c.varlen ? (st ? "fa_fp8_kvcache_step_varlen_workspace_bytes" : "fa_fp8_forward_kvcache_varlen_workspace_bytes") :
                        st ? "fa_fp8_kvcache_step_workspace_bytes" : c.hdim ? "fa_fp8_forward_kvcache_hdim_workspace_bytes" : "fa_fp8_forward_kvcache_workspace_bytes",
                        !st && !c.hdim && c.mod.any() ? "_mod" : "");
        if ((uintptr_t)c.workspace % 16 != 0) return fail(FA_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
    }
    return FA_OK;
}

static fa::Fp8KvArgs fp8_kvcache_args(const Fp8KvCall& c, int64_t S) {
    fa::Fp8KvArgs a;
    a.q = c.q; a.k_cache = c.k_cache; a.v_cache = c.v_cache; a.o = c.o; a.lse = c.lse;
    a.q_descale = c.q_descale; a.k_descale = c.k_descale; a.v_descale = c.v_descale;
    a.qds_bs = c.qds_bs; a.kds_bs = c.kds_bs; a.vds_bs = c.vds_bs;
    a.cache_seqlens = c.cache_seqlens; a.block_table = c.block_table; a.cache_batch_idx = c.cache_batch_idx;
    a.batch = c.batch; a.heads_q = c.heads_q; a.heads_kv = c.heads_kv; a.seqlen_q = c.seqlen_q; a.cache_len = c.cache_len;
    a.cache_batch = c.cache_batch; a.dtype = c.dtype;
    a.q_bs = c.q_bs; a.q_ts = c.q_ts; a.kc_bs = c.k_bs; a.kc_ts = c.k_ts; a.vc_bs = c.v_bs; a.vc_ts = c.v_ts;
    a.table_row_stride = c.table_rs; a.num_blocks = c.num_blocks; a.page_size = c.ps;
    a.causal = c.causal != 0; a.scale = (float)c.scale; a.num_splits = S; a.workspace = c.workspace; a.d = c.d;
    a.cu_seqlens_q = c.cu_seqlens_q; a.total_q = c.total_q; a.max_seqlen_q = c.max_seqlen_q;
    return a;
}

static int fp8_kvcache_impl(const char* who, const Fp8KvCall& c) {
    bool empty;
    int64_t S = 1;
    size_t need = 0;
    if (const int rc = fp8_kvcache_check(who, c, nullptr, empty, S, need)) return rc;
    if (empty) return FA_OK;
    // (d == 128: .._mod; packed queries: launch_fp8_kvcache_varlen)
    if (c.cu_seqlens_q) return launched(who, fa::launch_fp8_kvcache_varlen(fp8_kvcache_args(c, S), c.mod, reinterpret_cast<hipStream_t>(c.stream)));
    return launched(who, fa::launch_fp8_kvcache_hdim(fp8_kvcache_args(c, S), c.mod, reinterpret_cast<hipStream_t>(c.stream)));
}

size_t fa_fp8_forward_kvcache_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t d,
                                              int64_t num_splits) {
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits) || d != 128) return 0;
    return fa::kv_workspace_bytes(batch, heads_q, seqlen_q, 128, (int)fp8_kv_splits(batch, heads_q, heads_kv, seqlen_q, cache_len, num_splits));
}

int fa_fp8_forward_kvcache(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale,
                           const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                           const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                           int64_t cache_batch, int64_t d, int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride,
                           int64_t k_batch_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride,
                           int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t q_descale_batch_stride,
                           int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits,
                           void* workspace, size_t workspace_bytes, void* stream) {
    Fp8KvCall c;
    c.q = q; c.k_cache = k_cache; c.v_cache = v_cache; c.o = o; c.lse = lse;
    c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cache_seqlens = cache_seqlens; c.block_table = block_table; c.cache_batch_idx = cache_batch_idx;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.cache_len = cache_len; c.cache_batch = cache_batch;
    c.d = d; c.dtype = dtype; c.q_dtype = q_dtype; c.cache_dtype = cache_dtype;
    c.q_bs = q_batch_stride; c.q_ts = q_token_stride; c.k_bs = k_batch_stride; c.k_ts = k_token_stride; c.v_bs = v_batch_stride;
    c.v_ts = v_token_stride;
    c.table_rs = block_table_row_stride; c.num_blocks = num_blocks; c.ps = page_block_size;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    return fp8_kvcache_impl("fa_fp8_forward_kvcache", c);
}

size_t fa_fp8_forward_kvcache_workspace_bytes_mod(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                                  int64_t d, int64_t num_splits, int causal, int64_t window_left, int64_t window_right,
                                                  int with_sinks) {
    if (d != 128) return 0;
    return fa_fp8_forward_kvcache_hdim_workspace_bytes(batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits, causal, window_left,
                                                       window_right, with_sinks);
}

// the decode partials follow kv_workspace_bytes at the head dim; the split rule counts keys and is the same at every head dim
size_t fa_fp8_forward_kvcache_hdim_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                                   int64_t head_dim, int64_t num_splits, int causal, int64_t window_left,
                                                   int64_t window_right, int with_sinks) {
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, seqlen_q, cache_len, head_dim, num_splits) || window_left < -1 || window_right < -1) return 0;
    if (head_dim != 64 && head_dim != 128 && head_dim != 256) return 0;
    fa::Fp8Mod m;
    m.window_left = window_left; m.window_right = window_right;
    int64_t S = fp8_kv_splits(batch, heads_q, heads_kv, seqlen_q, fa::fp8kv_split_len(cache_len, seqlen_q, causal, m), num_splits);
    if (with_sinks && S < 2) S = 2;
    return fa::kv_workspace_bytes(batch, heads_q, seqlen_q, head_dim, (int)S);
}

// the arguments of fa_fp8_forward_kvcache_mod and fa_fp8_forward_kvcache_hdim alike (hdim: the head dims 64, 128 and 256)
static int fp8_forward_kvcache_mod_entry(const char* who, bool hdim, const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table, const int32_t* cache_batch_idx,
        int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t cache_batch, int64_t d,
        int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
        int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride, int64_t v_descale_batch_stride,
        int causal, double softmax_scale, int64_t num_splits, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads) {
    Fp8KvCall c;
    c.hdim = hdim;
    c.q = q; c.k_cache = k_cache; c.v_cache = v_cache; c.o = o; c.lse = lse;
    c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cache_seqlens = cache_seqlens; c.block_table = block_table; c.cache_batch_idx = cache_batch_idx;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.cache_len = cache_len; c.cache_batch = cache_batch;
    c.d = d; c.dtype = dtype; c.q_dtype = q_dtype; c.cache_dtype = cache_dtype;
    c.q_bs = q_batch_stride; c.q_ts = q_token_stride; c.k_bs = k_batch_stride; c.k_ts = k_token_stride; c.v_bs = v_batch_stride;
    c.v_ts = v_token_stride;
    c.table_rs = block_table_row_stride; c.num_blocks = num_blocks; c.ps = page_block_size;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.mod.window_left = window_left; c.mod.window_right = window_right; c.mod.softcap = softcap; c.mod.sinks = sinks;
    c.mod.sink_heads = sink_heads;
    return fp8_kvcache_impl(who, c);
}

int fa_fp8_forward_kvcache_mod(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table, const int32_t* cache_batch_idx,
        int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t cache_batch, int64_t d,
        int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
        int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride, int64_t v_descale_batch_stride,
        int causal, double softmax_scale, int64_t num_splits, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads) {
    return fp8_forward_kvcache_mod_entry("fa_fp8_forward_kvcache_mod", false, q, k_cache, v_cache, o, lse, q_descale, k_descale,
           v_descale, cache_seqlens, block_table, cache_batch_idx, batch, heads_q, heads_kv, seqlen_q, cache_len, cache_batch, d, dtype,
           q_dtype, cache_dtype, q_batch_stride, q_token_stride, k_batch_stride, k_token_stride, v_batch_stride, v_token_stride,
           block_table_row_stride, num_blocks, page_block_size, q_descale_batch_stride, k_descale_batch_stride, v_descale_batch_stride,
           causal, softmax_scale, num_splits, workspace, workspace_bytes, stream, window_left, window_right, softcap, sinks,
           sink_heads);
}

int fa_fp8_forward_kvcache_hdim(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table, const int32_t* cache_batch_idx,
        int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t cache_batch, int64_t head_dim,
        int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
        int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride, int64_t v_descale_batch_stride,
        int causal, double softmax_scale, int64_t num_splits, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads) {
    return fp8_forward_kvcache_mod_entry("fa_fp8_forward_kvcache_hdim", true, q, k_cache, v_cache, o, lse, q_descale, k_descale,
           v_descale, cache_seqlens, block_table, cache_batch_idx, batch, heads_q, heads_kv, seqlen_q, cache_len, cache_batch, head_dim,
           dtype, q_dtype, cache_dtype, q_batch_stride, q_token_stride, k_batch_stride, k_token_stride, v_batch_stride, v_token_stride,
           block_table_row_stride, num_blocks, page_block_size, q_descale_batch_stride, k_descale_batch_stride, v_descale_batch_stride,
           causal, softmax_scale, num_splits, workspace, workspace_bytes, stream, window_left, window_right, softcap, sinks,
           sink_heads);
}

// ---- the fp8 decode step (append, rotary and q quantise in front of fa_fp8_forward_kvcache_mod): see include/fa_mi355x.h
size_t fa_fp8_kvcache_step_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t d,
                                           int64_t num_splits, int causal, int64_t window_left, int64_t window_right, int with_sinks,
                                           int in_dtype, int with_q8_out) {
    if (!kv_ws_args_ok(batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits) || d != 128 || window_left < -1 || window_right < -1)
        return 0;
    const bool e4m3 = in_dtype == FA_DTYPE_E4M3;
    if ((!e4m3 && in_dtype != FA_DTYPE_F16 && in_dtype != FA_DTYPE_BF16) || (e4m3 && with_q8_out)) return 0;
    return fa::fp8kv_step_prep_bytes(batch, heads_q, seqlen_q, !e4m3 && !with_q8_out) +
           fa_fp8_forward_kvcache_workspace_bytes_mod(batch, heads_q, heads_kv, seqlen_q, cache_len, d, num_splits, causal, window_left,
                                                      window_right, with_sinks);
}

int fa_fp8_kvcache_step(const void* q, void* k_cache, void* v_cache, void* o, float* lse, const float* q_descale, const float* k_descale,
                        const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table, const int32_t* cache_batch_idx,
                        int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t cache_batch, int64_t d,
                        int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride,
                        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride,
                        int64_t num_blocks, int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                        int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                        size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap, const float* sinks,
                        int64_t sink_heads, const void* k_new, const void* v_new, int64_t seqlen_new, int64_t k_new_batch_stride,
                        int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int in_dtype, void* q8_out,
                        int64_t q8_batch_stride, int64_t q8_token_stride, const void* rotary_cos, const void* rotary_sin,
                        int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim,
                        int rotary_interleaved) {
    const char* who = "fa_fp8_kvcache_step";
    Fp8KvCall c;
    c.q = q; c.k_cache = k_cache; c.v_cache = v_cache; c.o = o; c.lse = lse;
    c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cache_seqlens = cache_seqlens; c.block_table = block_table; c.cache_batch_idx = cache_batch_idx;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.cache_len = cache_len; c.cache_batch = cache_batch;
    c.d = d; c.dtype = dtype; c.q_dtype = q_dtype; c.cache_dtype = cache_dtype;
    c.q_bs = q_batch_stride; c.q_ts = q_token_stride; c.k_bs = k_batch_stride; c.k_ts = k_token_stride; c.v_bs = v_batch_stride;
    c.v_ts = v_token_stride;
    c.table_rs = block_table_row_stride; c.num_blocks = num_blocks; c.ps = page_block_size;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.mod.window_left = window_left; c.mod.window_right = window_right; c.mod.softcap = softcap; c.mod.sinks = sinks;
    c.mod.sink_heads = sink_heads;
    Fp8StepCall t;
    t.k_new = k_new; t.v_new = v_new; t.seqlen_new = seqlen_new; t.kn_bs = k_new_batch_stride; t.kn_ts = k_new_token_stride;
    t.vn_bs = v_new_batch_stride; t.vn_ts = v_new_token_stride; t.in_dtype = in_dtype;
    t.q8_out = q8_out; t.q8_bs = q8_batch_stride; t.q8_ts = q8_token_stride;
    t.rotary_cos = rotary_cos; t.rotary_sin = rotary_sin; t.cos_rs = rotary_cos_row_stride; t.sin_rs = rotary_sin_row_stride;
    t.seqlen_ro = seqlen_ro; t.rotary_dim = rotary_dim; t.rotary_interleaved = rotary_interleaved;
    bool empty;
    int64_t S = 1;
    size_t need = 0;
    if (const int rc = fp8_kvcache_check(who, c, &t, empty, S, need)) return rc;
    if (empty) return FA_OK;
    fa::Fp8StepArgs s;
    s.kv = fp8_kvcache_args(c, S);
    s.in_dtype = in_dtype; s.k_new = k_new; s.v_new = v_new; s.seqlen_new = seqlen_new;
    s.kn_bs = t.kn_bs; s.kn_ts = t.kn_ts; s.vn_bs = t.vn_bs; s.vn_ts = t.vn_ts;
    s.q8_out = q8_out; s.q8_bs = t.q8_bs; s.q8_ts = t.q8_ts;
    s.rotary_cos = rotary_cos; s.rotary_sin = rotary_sin; s.rotary_cos_rs = t.cos_rs; s.rotary_sin_rs = t.sin_rs; s.rotary_dim = rotary_dim;
    s.rotary_interleaved = rotary_interleaved ? 1 : 0;
    // q token i is rotated at its own position when causal or a window bound was given (fa_ex_forward_kvcache_rotary's rule)
    s.rotary_q_per_token = (causal || window_left >= 0 || window_right >= 0) ? 1 : 0;
    return launched(who, fa::launch_fp8_kvcache_step(s, c.mod, reinterpret_cast<hipStream_t>(stream)));
}

// ---- packed queries and new keys on the fp8 decode call and the step, and the step at head dims 64 / 256: see include/fa_mi355x.h
// the splits of a packed call: the rule over max_seqlen_q (the most rows a sequence has), as the call's rule (9) takes them
static int64_t fp8_kv_splits_varlen(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t max_seqlen_q, int64_t cache_len,
                                    int64_t num_splits, int causal, int64_t window_left, int64_t window_right, int with_sinks) {
    fa::Fp8Mod m;
    m.window_left = window_left; m.window_right = window_right;
    int64_t S = fp8_kv_splits(batch, heads_q, heads_kv, max_seqlen_q, fa::fp8kv_split_len(cache_len, max_seqlen_q, causal, m), num_splits);
    if (with_sinks && S < 2) S = 2;
    return S;
}

static bool fp8_varlen_ws_args_ok(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q, int64_t cache_len,
                                  int64_t head_dim, int64_t num_splits, int64_t window_left, int64_t window_right) {
    const int64_t kInt = ((int64_t)1 << 31) - 1;
    return batch > 0 && batch <= 65535 && heads_q > 0 && heads_kv > 0 && heads_q % heads_kv == 0 && total_q >= 0 && total_q <= kInt &&
           max_seqlen_q >= 0 && max_seqlen_q <= total_q && (heads_q / heads_kv) * max_seqlen_q <= ((int64_t)1 << 20) && cache_len >= 1 &&
           num_splits >= 0 && num_splits <= 256 && window_left >= -1 && window_right >= -1 &&
           (head_dim == 64 || head_dim == 128 || head_dim == 256);
}

size_t fa_fp8_forward_kvcache_varlen_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q,
                                                     int64_t cache_len, int64_t head_dim, int64_t num_splits, int causal,
                                                     int64_t window_left, int64_t window_right, int with_sinks) {
    if (!fp8_varlen_ws_args_ok(batch, heads_q, heads_kv, total_q, max_seqlen_q, cache_len, head_dim, num_splits, window_left, window_right))
        return 0;
    if (total_q == 0 || max_seqlen_q == 0) return 0;
    const int64_t S = fp8_kv_splits_varlen(batch, heads_q, heads_kv, max_seqlen_q, cache_len, num_splits, causal, window_left, window_right, with_sinks);
    return fa::kv_workspace_bytes(1, heads_q, total_q, head_dim, (int)S);
}

int fa_fp8_forward_kvcache_varlen(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale, const float* k_descale,
        const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table, const int32_t* cache_batch_idx,
        int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t cache_batch, int64_t head_dim,
        int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride,
        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
        int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride, int64_t v_descale_batch_stride,
        int causal, double softmax_scale, int64_t num_splits, void* workspace, size_t workspace_bytes, void* stream,
        int64_t window_left, int64_t window_right, double softcap, const float* sinks, int64_t sink_heads,
        const int32_t* cu_seqlens_q, int64_t total_q, int64_t max_seqlen_q) {
    Fp8KvCall c;
    c.hdim = true; c.varlen = true;
    c.q = q; c.k_cache = k_cache; c.v_cache = v_cache; c.o = o; c.lse = lse;
    c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cache_seqlens = cache_seqlens; c.block_table = block_table; c.cache_batch_idx = cache_batch_idx;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.cache_len = cache_len; c.cache_batch = cache_batch;
    c.d = head_dim; c.dtype = dtype; c.q_dtype = q_dtype; c.cache_dtype = cache_dtype;
    c.q_bs = q_batch_stride; c.q_ts = q_token_stride; c.k_bs = k_batch_stride; c.k_ts = k_token_stride; c.v_bs = v_batch_stride;
    c.v_ts = v_token_stride;
    c.table_rs = block_table_row_stride; c.num_blocks = num_blocks; c.ps = page_block_size;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.mod.window_left = window_left; c.mod.window_right = window_right; c.mod.softcap = softcap; c.mod.sinks = sinks;
    c.mod.sink_heads = sink_heads;
    c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    return fp8_kvcache_impl("fa_fp8_forward_kvcache_varlen", c);
}

size_t fa_fp8_kvcache_step_varlen_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                                  int64_t head_dim, int64_t num_splits, int causal, int64_t window_left, int64_t window_right,
                                                  int with_sinks, int in_dtype, int with_q8_out, int64_t total_q, int64_t max_seqlen_q) {
    const bool e4m3 = in_dtype == FA_DTYPE_E4M3;
    if ((!e4m3 && in_dtype != FA_DTYPE_F16 && in_dtype != FA_DTYPE_BF16) || (e4m3 && with_q8_out)) return 0;
    if (seqlen_q != 0) {   // the padded step at head_dim (a packed call is asked about with seqlen_q == 0)
        if (total_q != 0 || max_seqlen_q != 0) return 0;
        if (head_dim == 128)
            return fa_fp8_kvcache_step_workspace_bytes(batch, heads_q, heads_kv, seqlen_q, cache_len, 128, num_splits, causal, window_left,
                                                       window_right, with_sinks, in_dtype, with_q8_out);
        const size_t att = fa_fp8_forward_kvcache_hdim_workspace_bytes(batch, heads_q, heads_kv, seqlen_q, cache_len, head_dim, num_splits, causal,
                                                                       window_left, window_right, with_sinks);
        if (!kv_ws_args_ok(batch, heads_q, heads_kv, seqlen_q, cache_len, head_dim, num_splits) || window_left < -1 || window_right < -1 ||
            (head_dim != 64 && head_dim != 256))
            return 0;
        return fa::fp8kv_step_prep_bytes_varlen(batch, batch * seqlen_q, heads_q, head_dim, !e4m3 && !with_q8_out) + att;
    }
    if (!fp8_varlen_ws_args_ok(batch, heads_q, heads_kv, total_q, max_seqlen_q, cache_len, head_dim, num_splits, window_left, window_right))
        return 0;
    const int64_t S = fp8_kv_splits_varlen(batch, heads_q, heads_kv, max_seqlen_q, cache_len, num_splits, causal, window_left, window_right, with_sinks);
    return fa::fp8kv_step_prep_bytes_varlen(batch, total_q, heads_q, head_dim, !e4m3 && !with_q8_out) +
           fa::kv_workspace_bytes(1, heads_q, total_q, head_dim, (int)S);
}

int fa_fp8_kvcache_step_varlen(const void* q, void* k_cache, void* v_cache, void* o, float* lse, const float* q_descale, const float* k_descale,
                               const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table, const int32_t* cache_batch_idx,
                               int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t cache_batch,
                               int64_t head_dim, int dtype, int q_dtype, int cache_dtype, int64_t q_batch_stride, int64_t q_token_stride,
                               int64_t k_batch_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_token_stride,
                               int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t q_descale_batch_stride,
                               int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale,
                               int64_t num_splits, void* workspace, size_t workspace_bytes, void* stream, int64_t window_left,
                               int64_t window_right, double softcap, const float* sinks, int64_t sink_heads, const void* k_new,
                               const void* v_new, int64_t seqlen_new, int64_t k_new_batch_stride, int64_t k_new_token_stride,
                               int64_t v_new_batch_stride, int64_t v_new_token_stride, int in_dtype, void* q8_out, int64_t q8_batch_stride,
                               int64_t q8_token_stride, const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                               int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                               const int32_t* cu_seqlens_q, int64_t total_q, int64_t max_seqlen_q, const int32_t* cu_seqlens_k_new,
                               int64_t total_k_new) {
    const char* who = "fa_fp8_kvcache_step_varlen";
    Fp8KvCall c;
    c.hdim = true; c.varlen = true;
    c.q = q; c.k_cache = k_cache; c.v_cache = v_cache; c.o = o; c.lse = lse;
    c.q_descale = q_descale; c.k_descale = k_descale; c.v_descale = v_descale;
    c.cache_seqlens = cache_seqlens; c.block_table = block_table; c.cache_batch_idx = cache_batch_idx;
    c.batch = batch; c.heads_q = heads_q; c.heads_kv = heads_kv; c.seqlen_q = seqlen_q; c.cache_len = cache_len; c.cache_batch = cache_batch;
    c.d = head_dim; c.dtype = dtype; c.q_dtype = q_dtype; c.cache_dtype = cache_dtype;
    c.q_bs = q_batch_stride; c.q_ts = q_token_stride; c.k_bs = k_batch_stride; c.k_ts = k_token_stride; c.v_bs = v_batch_stride;
    c.v_ts = v_token_stride;
    c.table_rs = block_table_row_stride; c.num_blocks = num_blocks; c.ps = page_block_size;
    c.qds_bs = q_descale_batch_stride; c.kds_bs = k_descale_batch_stride; c.vds_bs = v_descale_batch_stride;
    c.causal = causal; c.scale = softmax_scale; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
    c.mod.window_left = window_left; c.mod.window_right = window_right; c.mod.softcap = softcap; c.mod.sinks = sinks;
    c.mod.sink_heads = sink_heads;
    c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    Fp8StepCall t;
    t.k_new = k_new; t.v_new = v_new; t.seqlen_new = seqlen_new; t.kn_bs = k_new_batch_stride; t.kn_ts = k_new_token_stride;
    t.vn_bs = v_new_batch_stride; t.vn_ts = v_new_token_stride; t.in_dtype = in_dtype;
    t.q8_out = q8_out; t.q8_bs = q8_batch_stride; t.q8_ts = q8_token_stride;
    t.rotary_cos = rotary_cos; t.rotary_sin = rotary_sin; t.cos_rs = rotary_cos_row_stride; t.sin_rs = rotary_sin_row_stride;
    t.seqlen_ro = seqlen_ro; t.rotary_dim = rotary_dim; t.rotary_interleaved = rotary_interleaved;
    t.cu_seqlens_k_new = cu_seqlens_k_new; t.total_k_new = total_k_new;
    bool empty;
    int64_t S = 1;
    size_t need = 0;
    if (const int rc = fp8_kvcache_check(who, c, &t, empty, S, need)) return rc;
    if (empty) return FA_OK;
    fa::Fp8StepArgs s;
    s.kv = fp8_kvcache_args(c, S);
    s.in_dtype = in_dtype; s.k_new = k_new; s.v_new = v_new; s.seqlen_new = seqlen_new;
    s.kn_bs = t.kn_bs; s.kn_ts = t.kn_ts; s.vn_bs = t.vn_bs; s.vn_ts = t.vn_ts;
    s.q8_out = q8_out; s.q8_bs = t.q8_bs; s.q8_ts = t.q8_ts;
    s.rotary_cos = rotary_cos; s.rotary_sin = rotary_sin; s.rotary_cos_rs = t.cos_rs; s.rotary_sin_rs = t.sin_rs; s.rotary_dim = rotary_dim;
    s.rotary_interleaved = rotary_interleaved ? 1 : 0;
    s.rotary_q_per_token = (causal || window_left >= 0 || window_right >= 0) ? 1 : 0;   // the step's rule
    s.cu_seqlens_k_new = cu_seqlens_k_new; s.total_k_new = total_k_new;
    return launched(who, fa::launch_fp8_kvcache_step_varlen(s, c.mod, reinterpret_cast<hipStream_t>(stream)));
}

size_t fa_ex_backward_workspace_bytes_grouped(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype) {
    return ex_bwd_ws_grouped(bh, kv_group, nq, nk, d, dtype);
}

size_t fa_ex_backward_workspace_bytes_fast_grouped(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                                                   int extras) {
    return ex_bwd_ws_grouped(bh, kv_group, nq, nk, d, dtype) + ex_bwd_ds_room(bh, kv_group, nq, nk, d, dtype, causal, extras);
}

size_t fa_ex_backward_workspace_bytes(int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype) {
    (void)nk; (void)d; (void)dtype;
    if (bh <= 0 || nq <= 0) return 256;
    return (fa::ex_backward_workspace_bytes(bh, nq) + 255) & ~(size_t)255;
}

size_t fa_ex_backward_workspace_bytes_fast(int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype, int causal, int extras) {
    return fa_ex_backward_workspace_bytes(bh, nq, nk, d, dtype) + ex_bwd_ds_room(bh, 1, nq, nk, d, dtype, causal, extras);
}

size_t fa3_backward_workspace_bytes(int64_t bh, int64_t n, int64_t d, int dtype, int fp8) {
    size_t need = fa_backward_workspace_bytes(bh, n, d, dtype);
    if (fp8 && bh > 0 && n > 0 && d > 0 && fa::fwd_mfma_supported(dtype, d) && fa::bwd_mfma_supported(dtype, d)) need += 3 * slab_bytes(bh, n, d);
    return need;
}

size_t fa_backward_workspace_bytes(int64_t bh, int64_t n, int64_t d, int dtype) {
    if (bh <= 0 || n <= 0 || d <= 0) return 256;
    size_t g = fa::bwd_generic_workspace_bytes(bh, n);
    size_t m = fa::bwd_mfma_supported(dtype, d) ? fa::bwd_mfma_workspace_bytes(bh, n, d, bwd_atomic_variant()) : 0;
    size_t need = g > m ? g : m;
    return (need + 255) & ~(size_t)255;
}

size_t fa_backward_workspace_bytes_fast(int64_t bh, int64_t n, int64_t d, int dtype, int causal) {
    size_t need = fa_backward_workspace_bytes(bh, n, d, dtype);
    if (bh > 0 && n > 0 && d > 0 && fa::bwd_mfma_supported(dtype, d) && g_mode.load() != FA_MODE_F32_GENERIC)
        need += fa::bwd_ds_extra_bytes(bh, n, d, dtype, causal != 0, bwd_atomic_variant());
    return need;
}

size_t fa3_forward_workspace_bytes(int64_t bh, int64_t n, int64_t d, int dtype, int fp8) {
    if (!fp8 || bh <= 0 || n <= 0 || d <= 0 || !fa::fwd_mfma_supported(dtype, d) || !fa::bwd_mfma_supported(dtype, d)) return 0;
    if (fa::fwd_fp8_supported(dtype, d)) return slab_bytes(bh, n, d) + fa::fwd_fp8_workspace_bytes(bh, n, d);
    return 3 * slab_bytes(bh, n, d);
}

int fa_debug_trace_buffer(void* device_ptr) {
    return fa::set_trace_buffer(device_ptr) == hipSuccess ? FA_OK : fail(FA_ERR_LAUNCH, "fa_debug_trace_buffer: hipMemcpyToSymbol failed");
}

int fa_set_option(const char* name, int value) {
    if (!name || fa::set_option(name, value) != 0) return fail(FA_ERR_INVALID_ARGUMENT, "fa_set_option: unknown option '%s'", name ? name : "(null)");
    return FA_OK;
}

int64_t fa_route_count(const char* name) {
    const long long c = name ? fa::route_count(name) : -1;
    if (c < 0) return fail(FA_ERR_INVALID_ARGUMENT, "fa_route_count: unknown route '%s'", name ? name : "(null)");
    return c;
}

const char* fa_last_error(void) { return g_err; }
const char* fa_version(void) { return "fa_mi355x 0.1.0 (gfx950)"; }

int fa_set_kernel_mode(int mode) {
    if (mode != FA_MODE_AUTO && mode != FA_MODE_F32_GENERIC && mode != FA_MODE_BWD_ATOMIC) return fail(FA_ERR_INVALID_ARGUMENT, "fa_set_kernel_mode: bad mode %d", mode);
    return g_mode.exchange(mode);
}

int fa_device_is_gfx950(int device) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "hipGetDeviceProperties(%d): %s", device, hipGetErrorString(e));
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

}  // extern "C"
