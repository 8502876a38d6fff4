// Internal launcher interface between the C-ABI layer (fa_capi.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fa {

// Grouped-query attention: the multiplier for bh / g as umulhi(bh, m), m = ceil(2^32 / g); 0 for g = 1 (no grouping).  Exact for
// bh * g < 2^32 (m g = 2^32 + e with e < g: the error bh e / (g 2^32) stays below 1 / g), which the C-ABI layer checks.
inline unsigned kv_magic(int64_t g) { return g <= 1 ? 0u : (unsigned)((((uint64_t)1 << 32) + (uint64_t)g - 1) / (uint64_t)g); }

struct FwdArgs {
    const void *q, *k, *v;
    void* o;
    float* lse;
    int64_t bh, n, d;
    int dtype;  // FA_DTYPE_*
    int causal;
    float scale;
    int64_t nk = 0;   // keys (0: = n, the query rows).  Only the kernels fwd_nqnk_supported() names take nk != n.
    int64_t kv_group = 1;   // query heads per K/V head: k, v hold bh / kv_group units, query unit bh reads unit bh / kv_group
};

struct BwdArgs {
    const void *q, *k, *v, *o, *dout;
    const float* lse;
    void *dq, *dk, *dv;
    int64_t bh, n, d;
    int dtype;
    int causal;
    float scale;
    void* workspace;
    size_t workspace_bytes;
    int fused_dq;  // 1: single kernel, dQ by global float atomics; 0: dK/dV kernel + dQ kernel (deterministic)
    int64_t nk = 0;   // keys (0: = n, the query rows).  Only the stream kernels take nk != n (causal: nk >= n).
    // query heads per K/V head: k and v hold bh / kv_group units, read through unit bh / kv_group; dk and dv then receive the
    // per-query-head partials (bh units, as ungrouped) that kv_group_sum adds up.  > 1 only with fused_dq = 0.
    int64_t kv_group = 1;
};

// Optional per-kernel timing with HIP events recorded on the launch stream (used by bench.py for the
// roofline figure; off by default, costs nothing when off).
enum KernelId { K_FWD_F32 = 0, K_BWD_DELTA, K_BWD_DKDV_F32, K_BWD_DQ_F32, K_FWD_MFMA, K_BWD_MFMA, K_BWD_DQ_CVT, K_BWD_DQ_MFMA,
                K_FP8_QUANT, K_FWD_FP8, K_EX_FWD, K_EX_BWD, K_KV_GROUP_SUM, K_FP8IN_VT, K_FP8IN_FWD, K_FP8IN_VT_VARLEN,
                K_FP8IN_FWD_VARLEN, K_IDX_PACK, K_IDX_LOGITS, K_IDX_TOPK, K_FP8KV_SPLIT, K_FP8Q_AMAX, K_FP8Q_QUANT, K_FP8Q_FUSED,
                K_FP8IN_FWD_MOD, K_FP8IN_FWD_VARLEN_MOD, K_FP8KV_SPLIT_MOD, K_FP8KV_STEP_PREP, K_FP8IN_FWD_HDIM,
                K_FP8IN_FWD_VARLEN_HDIM, K_FP8KV_SPLIT_HDIM, K_FP8KV_SPLIT_VARLEN, K_FP8KV_STEP_PREP_VARLEN, K_COUNT };
void prof_begin(int id, hipStream_t st);
void prof_end(int id, hipStream_t st);
struct ProfScope {
    int id; hipStream_t st;
    ProfScope(int i, hipStream_t s) : id(i), st(s) { prof_begin(id, st); }
    ~ProfScope() { prof_end(id, st); }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and size instead of before every launch (a host
// call of a few microseconds: visible on the small launches).  Device-wide attribute; thread safe.
hipError_t ensure_dynamic_smem(const void* kernel, int bytes);

// Tuning knobs (tile sweep / A-B runs).  Each starts from an environment variable of the same upper-case name with
// an FA_ prefix (FA_FWD_KB, FA_FWD_STAG, FA_DKDV (4|8), FA_DQ_KT, FA_FWD_RS, FA_DKDV_KREG, FA_FWD_EAGER, FA_FWD_HS, FA_FWD_TPW, FA_DQ_TPW, FA_DKDV_TPW, FA_DQ_NLF, FA_DQ_W4, FA_FWD_ABL, FA_SMALL_GRID, FA_FP8_ROT, FA_DKDV_STG, FA_DKDV_LEAN) and can be changed at run time through
// fa_set_option() so that variants can be interleaved in one process.
enum OptionId { OPT_FWD_KB = 0, OPT_FWD_STAG, OPT_DKDV, OPT_DQ_KT, OPT_FWD_RS, OPT_DKDV_KREG, OPT_FWD_EAGER, OPT_FWD_HS, OPT_FWD_TPW, OPT_DQ_TPW, OPT_DKDV_TPW, OPT_DQ_NLF, OPT_DQ_W4, OPT_FWD_ABL, OPT_SMALL_GRID, OPT_FP8_ROT, OPT_DKDV_STG, OPT_DKDV_ABL, OPT_DQ, OPT_DQ_ABL, OPT_EX_PATH, OPT_DS_CHUNK_MB, OPT_FP8_PV, OPT_FWD_RD, OPT_FWD_W2, OPT_DKDV_LEAN, OPT_COUNT };
int option(int id);
int set_option(const char* name, int value);   // returns 0, or -1 for an unknown name

// Which form a launcher took, counted since the library was loaded and read back through fa_route_count(): a test asks the
// library, it does not guess from timing.  "dkdv_stream": the dS-storing dK/dV stream kernel, "dkdv_lean": its lean form;
// "fp8_quant_fused", "fp8_quant_two_pass", "fp8_quant_static": the routes of the fp8 quantiser (fa_fp8_quantize.hip);
// "fp8in_fwd_mod", "fp8in_fwd_varlen_mod", "fp8kv_split_mod": the featured kernels of the fp8 calls (window, softcap, sinks);
// "fp8kv_step_prep": the append / rotary / q quantise launch of the fp8 decode step (fa_fp8_step.hip);
// "fp8in_fwd_hdim", "fp8in_fwd_varlen_hdim", "fp8kv_split_hdim": the fp8 calls at head dim 64 or 256 (the _hdim entry points);
// "fp8kv_split_varlen": the packed-query split kernel of fa_fp8_forward_kvcache_varlen / fa_fp8_kvcache_step_varlen;
// "fp8kv_step_prep_varlen": the prep launch of fa_fp8_kvcache_step_varlen with packed tokens or at head dim 64 / 256.
enum RouteId { ROUTE_DKDV_STREAM = 0, ROUTE_DKDV_LEAN, ROUTE_FP8Q_FUSED, ROUTE_FP8Q_TWO_PASS, ROUTE_FP8Q_STATIC, ROUTE_FP8IN_FWD_MOD,
               ROUTE_FP8IN_FWD_VARLEN_MOD, ROUTE_FP8KV_SPLIT_MOD, ROUTE_FP8KV_STEP_PREP, ROUTE_FP8IN_FWD_HDIM,
               ROUTE_FP8IN_FWD_VARLEN_HDIM, ROUTE_FP8KV_SPLIT_HDIM, ROUTE_FP8KV_SPLIT_VARLEN, ROUTE_FP8KV_STEP_PREP_VARLEN, ROUTE_COUNT };
void route_hit(int id);

// exact-f32 kernels (fa_generic.hip): any dtype, d <= 256
hipError_t launch_fwd_generic(const FwdArgs& a, hipStream_t st);
hipError_t launch_bwd_generic(const BwdArgs& a, hipStream_t st);
size_t bwd_generic_workspace_bytes(int64_t bh, int64_t n);

// 16-bit MFMA kernels (fa_fwd_mfma.hip / fa_bwd_mfma.hip): f16/bf16, d in {64, 128}
bool fwd_mfma_supported(int dtype, int64_t d);
bool small_grid(int64_t bh, int64_t n, bool backward, int64_t d = 128);   // the 4-wave / 128-row kernels serve the launch better than 256-row tiles
hipError_t set_trace_buffer(void* device_ptr);   // debug: phase timestamps of the staggered forward (fa_fwd_mfma.hip)
hipError_t launch_fwd_mfma(const FwdArgs& a, hipStream_t st);
// Nq != Nk on the plain path's d = 128 kernels (staggered forward, stream backward): 16-bit tensors, Nk % 64 == 0 not needed,
// causal only with Nk >= Nq, launches big enough for the 256-row tiles
bool nqnk_mfma_supported(int dtype, int64_t d, int64_t bh, int64_t nq, int64_t nk, int causal);
hipError_t launch_fwd_nqnk(const FwdArgs& a, hipStream_t st);
bool bwd_mfma_supported(int dtype, int64_t d);
hipError_t launch_bwd_mfma(const BwdArgs& a, hipStream_t st);
size_t bwd_mfma_workspace_bytes(int64_t bh, int64_t n, int64_t d, bool atomic_variant);   // fp32 dQ scratch only for the single-kernel variant
// bytes the dS hand-over (fa_bwd_dq_ds.hip) wants on top of that; 0 where it does not serve the call
// (kv_group > 1: the chunks of query units are whole groups, so the room is sized for the rounded step)
size_t bwd_ds_extra_bytes(int64_t bh, int64_t n, int64_t d, int dtype, bool causal, bool atomic_variant, int64_t nk = 0, int64_t kv_group = 1);
// row constants + the chunk loop [dK/dV with dS stores, dQ product]; a.nk keys (0: = a.n), ds: bwd_ds_extra_bytes of room
hipError_t launch_bwd_handover(const BwdArgs& a, float* nlse, float* ndelta, void* ds, hipStream_t st);
hipError_t launch_bwd_dkdv_mfma(const BwdArgs& a, const float* nlse, const float* ndelta, hipStream_t st);  // 8-wave dK/dV
hipError_t launch_bwd_dq_mfma(const BwdArgs& a, float* nlse, float* ndelta, hipStream_t st);   // d > 64: also WRITES nlse / ndelta
inline bool dq_makes_row_constants(int64_t d) { return d > 64; }
// one wave per SIMD, 64 keys per wave, hand-ordered MFMA stream (fa_bwd_dkdv_w4.hip): d = 128
bool bwd_dkdv_w4_supported(int dtype, int64_t d);
// ds != null: the kernel also stores the packed dS tiles there (ds_workspace_bytes) for launch_bwd_dq_ds
hipError_t launch_bwd_dkdv_w4(const BwdArgs& a, const float* nlse, const float* ndelta, hipStream_t st, void* ds = nullptr);
// dS hand-over between the dK/dV stream kernel and the dQ product kernel (fa_bwd_dq_ds.hip): 2-KiB tiles of 32 queries x
// 32 keys, (b,h)-major, then 32-query block, then 32-key block; the key blocks are padded to the dK/dV kernel's 256-key tiles
inline int ds_tile_rows(int64_t nq) { return (int)((nq + 31) / 32); }
inline int ds_tile_cols(int64_t nk) { return (int)(8 * ((nk + 255) / 256)); }
inline size_t ds_workspace_bytes(int64_t bh, int64_t nq, int64_t nk) { return (size_t)bh * ds_tile_rows(nq) * ds_tile_cols(nk) * 2048; }
// dQ = scale * dS K from the stored dS tiles: d = 128, one pass over dS at HBM rate (no recomputation of S and dP)
hipError_t launch_bwd_dq_ds(const BwdArgs& a, const void* ds, hipStream_t st);

// the dQ pass in the same shape (fa_bwd_dq_w4.hip): d = 128; writes nlse / ndelta like launch_bwd_dq_mfma at d > 64
bool bwd_dq_w4_supported(int dtype, int64_t d);
hipError_t launch_bwd_dq_w4(const BwdArgs& a, float* nlse, float* ndelta, hipStream_t st);

// FA3-style fp8 forward (fa_fwd_fp8.hip): Q/K quantised to e4m3 per 64-row block, S on the fp8 MFMA
bool fwd_fp8_supported(int dtype, int64_t d);
bool fp8_v_pow2(int dtype, int64_t n, int64_t d);   // V~ with power-of-two block scales (forward and backward alike)
// workspace: fwd_fp8_workspace_bytes; vslab: room for one 16-bit (bh, n, d) tensor (the round-tripped V of the 16-bit P.V kernel)
hipError_t launch_fwd_fp8(const FwdArgs& a, void* workspace, void* vslab, hipStream_t st);
size_t fwd_fp8_workspace_bytes(int64_t bh, int64_t n, int64_t d);
// e4m3 round trip (one scale per 64-row block) of q, k (rotated around the quantisation for power-of-two d) and v into 16-bit
// tensors, any d % 8 == 0 up to 256; null sources are skipped
hipError_t launch_fp8_roundtrip(const void* q, const void* k, const void* v, void* qt, void* kt, void* vt, int64_t bh, int64_t n,
                                int64_t d, int dtype, hipStream_t st);

// Extended attention: Nq != Nk with a bottom-right aligned causal mask, dense mask, block-sparse mask, dropout.
// fa_ex.hip: exact-f32 kernels, any dtype, d <= 256.  fa_ex_mfma.hip: bf16 / f16, d % 8 == 0 up to 128, block-sparse
// blocks that are multiples of 32 — the default where it applies (option ex_path: 1 = always exact f32,
// 2 = MFMA or fail, 3 = the extended MFMA kernels or fail, also where the plain kernels would do: square, no extras).
struct ExArgs {
    const void *q, *k, *v;        // q: (bh, nq, d); k, v: (bh, nk, d)
    void* o;                      // (bh, nq, d)
    float* lse;                   // (bh, nq)
    const void* dout;             // backward: (bh, nq, d)
    void *dq, *dk, *dv;           // backward outputs
    int64_t bh, nq, nk, d;
    int dtype, causal;
    float scale;
    const uint8_t* mask;          // (nq, nk) bytes, 0 = masked; null = none
    int64_t mask_bh_stride;       // 0 = one mask shared by all (b,h), nq * nk = one per (b,h)
    const uint8_t* block_mask;    // (ceil(nq/br), ceil(nk/bc)) bytes, 0 = tile skipped; null = none
    int64_t br, bc;
    double dropout_p;
    uint64_t seed;
    void* workspace;              // backward: ex_backward_workspace_bytes
    size_t workspace_bytes = 0;   // what the caller really gave (more than the minimum lets plain calls hand dS over)
    int64_t kv_group = 1;         // query heads per K/V head: k, v, dk, dv hold bh / kv_group units (grouped-query attention)
    // sliding window, canonicalised by the C layer (fa_capi.hip: window_canon): key j is visible to row i only if
    // j >= i + (nk - nq) - window_left and j <= i + (nk - nq) + window_right; -1 = unbounded on that side.  After
    // canonicalisation a bound that is not -1 bounds something, and causal != 0 comes with window_right = -1.
    int64_t window_left = -1, window_right = -1;
    // variable-length (packed) sequences (fa_ex_*_varlen; cu_q != null): bh = batch * heads_q units, nq / nk = max_seqlen_q / _k
    // (the padded call's grid and dropout counters), the window canonicalised against them.  q: (total_q, heads_q, d) at token
    // stride stride_q, k / v: (total_k, heads_q / kv_group, d) at stride_k / stride_v; o, dout, dq dense (total_q, heads_q, d),
    // lse (heads_q, total_q); dk, dv dense (total_k, heads_q / kv_group, d).  cu_q / cu_k: batch + 1 untrusted device offsets.
    const int* cu_q = nullptr;
    const int* cu_k = nullptr;
    int64_t heads_q = 0, total_q = 0, total_k = 0, stride_q = 0, stride_k = 0, stride_v = 0;
    // score modifiers (fa_ex_*_scoremod), between Q K^T and the softmax: s' = softcap tanh(s / softcap) if softcap > 0, then
    // s'' = s' - slope(u) |i + coff - j| if alibi != null, s = scale q.k.  Query unit u takes slope
    // alibi[(u / alibi_heads) * alibi_bstride + u % alibi_heads] (device memory, read by the kernels only).
    double softcap = 0.0;
    const float* alibi = nullptr;
    int64_t alibi_heads = 1, alibi_bstride = 0;
    // attention sinks (fa_ex_*_sink; sinks != null): one extra softmax column per row with logit sinks[u % sink_heads] of query
    // unit u (natural-log units, after softcap and ALiBi; never masked or dropped) and a zero value vector.  Device memory, read
    // by the kernels only; -inf = no sink for that head.  Backward: dsinks (sink_heads,) float32 receives the gradient.
    const float* sinks = nullptr;
    int64_t sink_heads = 1;
    float* dsinks = nullptr;
    // the gradient of lse (fa_ex_backward_dlse / fa_ex_backward_varlen_dlse; null: none): float32 in lse's layout, added to the row
    // constant the backward kernels read, -delta + dlse; rows whose lse is -inf ignore it.  Such a call runs the recomputing extended
    // kernels (fa_ex_mfma.hip, fa_ex.hip), whose pre-pass is a launch of its own.
    const float* dlse = nullptr;
    // paged K/V of the varlen forward (fa_ex_forward_varlen_paged; block_table != null, forward only, no dropout): k and v are pools
    // (num_blocks, page_size, heads_q / kv_group, d) with token strides stride_k / stride_v and page strides page_stride_k / _v;
    // key t of sequence b is row t % page_size of page block_table[b * max_blocks + t / page_size] (untrusted device numbers);
    // len_k[b] = cu_k[b + 1] - cu_k[b] clamped to [0, nk], nk = min(max_seqlen_k, max_blocks * page_size); total_k is not used.
    const int* block_table = nullptr;
    int64_t max_blocks = 0, num_blocks = 0, page_size = 0, page_stride_k = 0, page_stride_v = 0;
    // an e4m3 pool under the paged varlen forward (fa_ex_forward_varlen_paged_fp8; 0 / null: a pool of q's dtype).  kv_e4m3: k and v
    // hold OCP e4m3 bytes and stride_k / stride_v / page_stride_k / _v (still in elements) are bytes; a stored byte c of K head h of
    // sequence b stands for e4m3(c) * k_descale[b * descale_bstride + h] (V likewise), a null scale for 1.0 (KvArgs has the same).
    int kv_e4m3 = 0;
    const float *k_descale = nullptr, *v_descale = nullptr;
    int64_t descale_bstride = 0;
    // V narrower than Q / K (fa_ex_*_vdim; 0: v, o, dout, dv are d wide like q and k).  d_v != 0: v, o, dout and dv are d_v wide
    // (varlen: o, dout rows of heads_q * d_v), the call goes to launch_ex_vdim (fa_ex_mfma_vdim.hip) and carries no other feature
    // than causal, kv_group, packing and dlse.  The C layer passes d_v = d as 0.
    int64_t d_v = 0;
    // additive attention bias (fa_ex_*_bias; bias != null): s = scale q.k + bias[b, h, i, j] for query unit u = b * bias_heads + h,
    // in q's dtype (f16 / bf16), read at bias + b * bias_bstride + h * bias_hstride + i * bias_rstride + j (elements; a stride of 0
    // broadcasts); -inf = the key is not visible.  The call goes to launch_ex_mfma_bias (fa_ex_mfma_bias.hip) and carries no other
    // feature than causal, kv_group and dlse.  Backward: dbias != null receives dS = P (dP - delta + dlse) at its own strides, every
    // element [.., :nq, :nk] written; a dbias stride of 0 over a dimension of more than one unit is the fp32 sum over it, in unit
    // order, rounded once (through a workspace of ex_bias_ds_bytes behind the row constants).
    const void* bias = nullptr;
    int64_t bias_heads = 1, bias_bstride = 0, bias_hstride = 0, bias_rstride = 0;
    void* dbias = nullptr;
    int64_t dbias_bstride = 0, dbias_hstride = 0, dbias_rstride = 0;
};
// does the call carry a score modifier (softcap or ALiBi)?  Such a call runs on the extended kernels only.
inline bool ex_scoremod(const ExArgs& a) { return a.softcap > 0.0 || a.alibi != nullptr; }
// does the call carry a window that bounds something (canonicalised: any bound that is not -1)?
inline bool ex_windowed(const ExArgs& a) { return a.window_left >= 0 || a.window_right >= 0; }
hipError_t launch_ex(const ExArgs& a, bool backward, hipStream_t st);
// dsinks[h] = -dsign * sum over the rows of head h of exp(sinks[h] - lse) * delta (fa_ex.hip: ex_dsink_kernel), launched by the
// backward of a sink call after its delta pre-pass.  delta: the pre-pass's rowsum(dO * O) (dsign = 1) or its negation (-1); row i
// of unit u at delta[u * nq + i], varlen token t of head h at delta[h * d_hstride + t * d_tstride].
hipError_t launch_ex_dsink(const ExArgs& a, const float* delta, long long d_hstride, long long d_tstride, float dsign, hipStream_t st);
// lse[u * nq + i] = sinks[u % sink_heads]: the rows of a sink call without any key
hipError_t launch_ex_sink_fill(float* lse, const float* sinks, int64_t sink_heads, int64_t units, int64_t nq, hipStream_t st);
bool ex_mfma_supported(const ExArgs& a);
hipError_t launch_ex_mfma(const ExArgs& a, bool backward, hipStream_t st);
bool ex_mfma_varlen_supported(const ExArgs& a);
hipError_t launch_ex_mfma_varlen(const ExArgs& a, bool backward, hipStream_t st);
bool ex_mfma_paged_supported(const ExArgs& a);                        // the paged varlen forward (a.block_table != null)
hipError_t launch_ex_mfma_varlen_paged(const ExArgs& a, hipStream_t st);
bool ex_mfma_paged_kv8_supported(const ExArgs& a);                    // the same from an e4m3 pool (a.kv_e4m3; fa_ex_mfma_kv8.hip)
hipError_t launch_ex_mfma_varlen_paged_kv8(const ExArgs& a, hipStream_t st);
size_t ex_backward_workspace_bytes(int64_t bh, int64_t nq);
// a call with an additive bias (a.bias != null; fa_ex_mfma_bias.hip): the kFeatBias instantiations of the 16-bit MFMA kernels
bool ex_mfma_bias_supported(const ExArgs& a);
hipError_t launch_ex_mfma_bias(const ExArgs& a, bool backward, hipStream_t st);
// is a.dbias the sum of the per-unit dS over a broadcast batch or head dimension?  Then the kernels write (bh, nq, nk padded to 8)
// 16-bit dS into the workspace behind the row constants, ex_bias_ds_bytes of it, and one more launch sums them.
inline bool ex_bias_reduced(int64_t bh, int64_t bias_heads, int64_t dbias_bstride, int64_t dbias_hstride) {
    return bias_heads > 0 && ((dbias_bstride == 0 && bh / bias_heads > 1) || (dbias_hstride == 0 && bias_heads > 1));
}
inline size_t ex_bias_ds_bytes(int64_t bh, int64_t nq, int64_t nk) { return (size_t)bh * nq * ((nk + 7) & ~(int64_t)7) * 2; }
// the row constants [-lse / scale | -delta (+ dlse)] of a backward whose o and dout rows are d_row wide (fa_ex_mfma.hip's pre-pass)
hipError_t launch_exm_prep(const ExArgs& a, int64_t d_row, float* nlse, float* ndelta, hipStream_t st);
// a.d_v != 0 (fa_ex_mfma_vdim.hip): 16-bit MFMA kernels with two widths, d <= 192 and d_v <= 128; padded and packed
bool ex_vdim_supported(const ExArgs& a);
hipError_t launch_ex_vdim(const ExArgs& a, bool backward, hipStream_t st);
// the two per-query-head dK / dV partial slabs of a grouped backward (kv_group > 1), each rounded to 256 bytes
inline size_t kv_partial_bytes(int64_t bh, int64_t nk, int64_t d, int dtype) {
    return (((size_t)bh * nk * d * (dtype == 0 ? 4 : 2) + 255) & ~(size_t)255);
}

// KV-cache decoding with split-KV (fa_decode.hip; fa_ex_forward_kvcache).  16-bit tensors, d % 8 == 0 up to 256, strides
// multiples of 8 elements, 16-byte aligned tensors, a batch element's cache span below 2^31 bytes (fa_capi.hip checks all of it).
struct KvArgs {
    const void* q;                 // (batch, seqlen_q, heads_q, d): batch stride q_bs, token stride q_ts, heads at stride d
    void *k_cache, *v_cache;       // (batch, cache_len, heads_kv, d): kc_bs / kc_ts, vc_bs / vc_ts
    const void *k_new, *v_new;     // (batch, seqlen_new, heads_kv, d): kn_bs / kn_ts, vn_bs / vn_ts; appended at L_b
    void* o;                       // (batch, seqlen_q, heads_q, d) dense
    float* lse;                    // (batch, heads_q, seqlen_q)
    const int* cache_seqlens;      // (batch,) untrusted device lengths, null: L_b = cache_len
    // fa_ex_forward_kvcache_paged (all null / 0: the contiguous call).  With block_table k_cache / v_cache are pools
    // (num_blocks, page_size, heads_kv, d), kc_bs / vc_bs their page strides and cache_len = max_blocks_per_seq * page_size.
    const int* block_table;        // (batch, max_blocks_per_seq) untrusted device page numbers, rows at table_row_stride
    const int* cache_batch_idx;    // (batch,) untrusted device cache rows in [0, cache_batch); contiguous cache only
    const int* cache_leftpad;      // (batch,) untrusted device first cache positions; contiguous cache only
    int64_t table_row_stride, num_blocks, page_size, cache_batch;
    int64_t batch, heads_q, heads_kv, seqlen_q, seqlen_new, cache_len, d;
    int dtype, causal;
    int64_t q_bs, q_ts, kc_bs, kc_ts, vc_bs, vc_ts, kn_bs, kn_ts, vn_bs, vn_ts;
    int64_t window_left, window_right;   // -1 = unbounded
    float scale;
    double softcap;
    const float* alibi;            // slope of (b, h): alibi[b * alibi_bstride + h]; null = none
    int64_t alibi_bstride;
    int64_t num_splits;            // >= 1 (the C layer resolves 0 through kv_num_splits)
    void* workspace;               // kv_workspace_bytes
    // fa_ex_forward_kvcache_rotary (null / 0: no rotation).  Tables (seqlen_ro, rotary_dim / 2) in q's dtype, rows at even
    // strides; seqlen_ro >= cache_len + max(0, seqlen_q - seqlen_new), so the kernels read them unchecked; seqlen_new > 0.
    const void *rotary_cos, *rotary_sin;
    int64_t rotary_cos_rs, rotary_sin_rs, rotary_dim;
    int rotary_interleaved;        // pairs (2j, 2j + 1), else (j, j + rotary_dim / 2)
    int rotary_q_per_token;        // q token i at position L_b - P_b + i (causal or a window bound given), else all at L_b - P_b
    // fa_ex_forward_kvcache_fp8 (0 / null: a 16-bit cache).  cache_e4m3: k_cache / v_cache hold OCP e4m3 bytes, their strides
    // (still in elements) are bytes, 8-byte aligned; a stored byte c of K head h of sequence b stands for
    // e4m3(c) * k_descale[b * descale_bstride + h] (V likewise), a null scale for 1.0.
    int cache_e4m3 = 0;
    const float *k_descale = nullptr, *v_descale = nullptr;
    int64_t descale_bstride = 0;
    // fa_ex_forward_kvcache_sink (null: no sinks): head h of every sequence takes the extra column sinks[h % sink_heads].  The call
    // then always runs the combine (num_splits >= 2): the sink joins there (kv_combine_kernel<Tag, SINK = true>).
    const float* sinks = nullptr;
    int64_t sink_heads = 1;
    // fa_ex_forward_kvcache_varlen (null / 0: the padded call).  cu_seqlens_q: q and o are packed (total_q, heads_q, d) at token
    // stride q_ts (o dense), lse is (heads_q, total_q), sequence b owns at most max_seqlen_q of the tokens; seqlen_q and q_bs
    // are not used.  cu_seqlens_k_new: k_new, v_new are packed (total_k_new, heads_kv, d); seqlen_new, kn_bs and vn_bs are
    // not used.  Both untrusted device offsets (batch + 1,), clamped in the kernels (fa_decode_common.h: kv_cu_range).
    const int *cu_seqlens_q = nullptr, *cu_seqlens_k_new = nullptr;
    int64_t total_q = 0, max_seqlen_q = 0, total_k_new = 0;
    // fa_ex_forward_kvcache_qv (null / 0: K and V of one width).  qv: a second query operand (batch, seqlen_q, heads_q, d_v) at
    // qv_bs / qv_ts, heads at stride d_v; v_cache and o are then d_v wide, the score is scale * (q . k + qv . v), and the call goes
    // to launch_kvcache_mla (fa_mla.hip: d = 64, d_v = 512; no new tokens, rotary, e4m3, softcap, ALiBi, sinks, packing, leftpad).
    const void* qv = nullptr;
    int64_t qv_bs = 0, qv_ts = 0, d_v = 0;
};
int kv_num_splits(int64_t batch, int64_t heads_kv, int64_t row_tiles, int64_t cache_len);
// the qv call's launch rule (fa_mla.hip): waves a workgroup for rows = (heads_q / heads_kv) * seqlen_q packed rows, and its splits
int mla_waves(int64_t rows);
int mla_num_splits(int64_t batch, int64_t heads_kv, int64_t rows, int64_t cache_len);
size_t kv_workspace_bytes(int64_t batch, int64_t heads_q, int64_t seqlen_q, int64_t d, int splits);
hipError_t launch_kvcache(const KvArgs& a, hipStream_t st);
hipError_t launch_kvcache_mla(const KvArgs& a, hipStream_t st);

// Sparse MLA decoding (fa_mla.hip; fa_mla_sparse_forward): the qv call over a list of cached tokens per (sequence, query token,
// K/V head).  kv: that call's arguments (d = 64, d_v = 512, no window); indices: untrusted device int32 token positions, entry j
// of (b, i, hk) at indices[b * ix_bs + i * ix_ts + hk * ix_hs + j], j < topk.  An entry outside [0, L_b) (causal: above
// L_b - seqlen_q + i) is no key and is never turned into an address.
struct MlaSparseArgs {
    KvArgs kv;
    const int* indices;
    int64_t ix_bs, ix_ts, ix_hs, topk;
};
// its launch rule: units = batch * seqlen_q lists a K/V head, each a workgroup row of mla_waves(group) waves over the group's heads
int mla_sparse_num_splits(int64_t units, int64_t heads_kv, int64_t group, int64_t topk);
hipError_t launch_mla_sparse(const MlaSparseArgs& a, hipStream_t st);

// MLA decoding from the packed 8-bit latent cache (fa_mla.hip; fa_mla_fp8_forward): 656-byte tokens [512 e4m3 | 4 float32 scales,
// one per 128-wide tile | 64 bf16] in a paged pool, token slot of page pg at pool + pg * page_sb + slot * tok_sb bytes.  sa: the
// sparse call's arguments with k_cache / v_cache null, bf16, heads_kv = 1 and a block_table; sa.indices null: the dense call
// (sa.kv as launch_kvcache_mla takes it), else the list call with ix_hs = 0.  Waves, splits and workspace are those calls'.
struct MlaF8Args {
    MlaSparseArgs sa;
    const void* pool;
    int64_t page_sb, tok_sb;
    int64_t q_hs, qv_hs;   // head strides of q and qv in elements (>= 64, >= 512)
};
hipError_t launch_mla_f8(const MlaF8Args& a, hipStream_t st);
// the append into that pool (fa_mla_fp8_pack): new token i of sequence b, latent (512) and rope (64) bf16 rows at their batch /
// token strides in elements, quantised and written at position cache_seqlens[b] + i; both device arrays untrusted
struct MlaF8PackArgs {
    const void *latent, *rope;
    void* pool;
    const int *cache_seqlens, *block_table;
    int64_t batch, seqlen_new, lat_bs, lat_ts, rope_bs, rope_ts, page_sb, tok_sb, table_row_stride, num_blocks, page_size, max_blocks;
    int scale_pow2;
};
hipError_t launch_mla_f8_pack(const MlaF8PackArgs& a, hipStream_t st);

// The lightning indexer (fa_indexer.hip; fa_indexer_pack, fa_indexer_logits, fa_indexer_topk): the index-key cache is a paged pool of
// 132-byte tokens [128 e4m3 | 1 float32 scale], token slot of page pg at pool + pg * page_sb + slot * tok_sb bytes; lengths and
// table are untrusted as for MlaF8PackArgs.  The append: k_new (batch, seqlen_new, 128) bf16 at its strides in elements.
struct IndexerPackArgs {
    const void* k_new;
    void* pool;
    const int *cache_seqlens, *block_table;
    int64_t batch, seqlen_new, k_bs, k_ts, page_sb, tok_sb, table_row_stride, num_blocks, page_size, max_blocks;
    int scale_pow2;
};
hipError_t launch_indexer_pack(const IndexerPackArgs& a, hipStream_t st);
// the logits: q (batch, seqlen_q, heads, 128) e4m3 at byte strides, weights (batch, seqlen_q, heads) and logits (batch, seqlen_q,
// width) float32 at element strides; heads 32 | 64.  Only the entries a token sees are written.
struct IndexerLogitsArgs {
    const void *q, *pool;
    const float* weights;
    const int *cache_seqlens, *block_table;
    float* logits;
    int64_t batch, seqlen_q, heads, width, q_bs, q_ts, q_hs, w_bs, w_ts, lg_bs, lg_rs, page_sb, tok_sb, table_row_stride, num_blocks,
        page_size, max_blocks;
    int causal;
};
hipError_t launch_indexer_logits(const IndexerLogitsArgs& a, hipStream_t st);
// the selection: per row the topk largest visible logits' positions, ascending, then -1
struct IndexerTopkArgs {
    const float* logits;
    const int* cache_seqlens;
    int* indices;
    int64_t batch, seqlen_q, width, topk, lg_bs, lg_rs, ix_bs, ix_ts;
    int causal;
};
hipError_t launch_indexer_topk(const IndexerTopkArgs& a, hipStream_t st);

// Rotary embedding for training and prefill (fa_rotary.hip; fa_rotary_apply).  16-bit x, y (batch, seqlen, heads, d), heads at
// stride d, strides multiples of 8 elements, 16-byte aligned; y == x (with x's strides) is the in-place form.  Tables as KvArgs'.
struct RotaryArgs {
    const void* x;
    void* y;
    int64_t batch, seqlen, heads, d;
    int dtype;
    int64_t x_bs, x_ts, y_bs, y_ts;
    const void *rotary_cos, *rotary_sin;
    int64_t rotary_cos_rs, rotary_sin_rs, seqlen_ro, rotary_dim;
    int rotary_interleaved, conjugate;   // conjugate: rotate by -sin (the backward)
    int64_t seqlen_offset;               // token i of sequence b at seqlen_offset + seqlen_offsets[b] + i; rotated iff in [0, seqlen_ro)
    const int* seqlen_offsets;           // (batch,) untrusted device memory, or null
    const int* cu_seqlens;               // (batch + 1,) untrusted device offsets of packed (total, heads, d) tensors, or null
    int64_t total, max_seqlen;
};
hipError_t launch_rotary(const RotaryArgs& a, hipStream_t st);

// The fp8 quantiser (fa_fp8_quantize.hip; fa_fp8_quantize): 16-bit x -> e4m3 out with one float32 descale per (batch, group of
// heads_per_scale heads).  x strides in elements, out strides in bytes; tables and positions as RotaryArgs' (rotary_cos null: none).
struct Fp8QuantArgs {
    const void* x = nullptr;
    void* out = nullptr;
    const float* descale = nullptr;      // static mode: (batch, heads / heads_per_scale) at descale_bs (0: one row); null: dynamic
    float* descale_out = nullptr;        // (batch, heads / heads_per_scale) contiguous; may be null in static mode
    const int* cu_seqlens = nullptr;     // (batch + 1,) untrusted device offsets of a packed (total, heads, d) x, or null
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;
    int64_t rotary_cos_rs = 0, rotary_sin_rs = 0, seqlen_ro = 0, rotary_dim = 0;
    int rotary_interleaved = 0;
    int64_t seqlen_offset = 0;
    const int* seqlen_offsets = nullptr;
    int64_t batch = 0, heads = 0, seqlen = 0, d = 0, heads_per_scale = 1, total = 0, max_seqlen = 0;
    int dtype = 0;
    int64_t x_bs = 0, x_hs = 0, x_ts = 0, o_bs = 0, o_hs = 0, o_ts = 0, descale_bs = 0;
    int scale_pow2 = 0;
    void* workspace = nullptr;           // fp8_quant_workspace_bytes, the two-pass route only
};
// work items (one 16-byte chunk, or a non-interleaved rotary pair of them) of the largest unit; at most kFp8QuantFused of them:
// the dynamic call is one launch that holds the unit in registers
constexpr int64_t kFp8QuantFused = 1024;
int64_t fp8_quant_unit_items(const Fp8QuantArgs& a);
inline bool fp8_quant_two_pass(const Fp8QuantArgs& a) { return !a.descale && fp8_quant_unit_items(a) > kFp8QuantFused; }
size_t fp8_quant_workspace_bytes(int64_t batch, int64_t heads, int64_t heads_per_scale);
hipError_t launch_fp8_quantize(const Fp8QuantArgs& a, hipStream_t st);

// Merge of two partial attention results over disjoint key sets (fa_merge.hip; fa_merge_states / fa_merge_states_backward).  Every
// tensor is addressed by (batch, head, row) through a stride triple in elements; the d elements of an o-like row are contiguous.
struct MergeTensor {
    const void* p = nullptr;
    int64_t bs = 0, hs = 0, rs = 0;
};
struct MergeArgs {
    MergeTensor o_a, lse_a, o_b, lse_b;   // inputs of both directions
    MergeTensor o, lse;                   // forward outputs (o == o_a and lse == lse_a with equal strides: in place)
    MergeTensor dout, dlse;               // backward inputs (dlse.p null: zero)
    MergeTensor do_a, do_b, dlse_a, dlse_b;   // backward outputs
    int64_t batch = 0, heads = 0, rows = 0, d = 0;
    int dtype = 0;
    bool vec = true;                      // fp32 only: 16-byte accesses (d % 4 == 0 and everything aligned); else 4-byte ones
};
hipError_t launch_merge(const MergeArgs& a, bool backward, hipStream_t st);

// Grouped-query attention (fa_kv_group.hip): dk[u] = sum over m = 0 .. g-1 of pk[u g + m] (and dv from pv), accumulated in fp32 in
// that order and rounded once to the tensor dtype; units of nk * d elements, bh / g of them in dk and dv.
hipError_t launch_kv_group_sum(const void* pk, const void* pv, void* dk, void* dv, int64_t bh_kv, int64_t g, int64_t nk, int64_t d,
                               int dtype, hipStream_t st);

// the same for one tensor (dK and dV of different widths)
hipError_t launch_kv_group_sum_one(const void* src, void* dst, int64_t bh_kv, int64_t g, int64_t nk, int64_t d, int dtype, hipStream_t st);

// e4m3 q, k, v with per-(batch, K/V head) descales (fa_fp8_inputs.hip; fa_fp8_forward): a V^T byte permutation into the workspace,
// then the attention kernel.  q, k, v strides in bytes (= e4m3 elements), o strides in elements of its 16-bit dtype; head_dim 128.
struct Fp8InArgs {
    const void *q = nullptr, *k = nullptr, *v = nullptr;
    void* o = nullptr;
    float* lse = nullptr;                                   // (batch, heads_q, nq) contiguous
    const float *q_descale = nullptr, *k_descale = nullptr, *v_descale = nullptr;   // (batch, heads_kv) device floats; null: 1
    int64_t qds_bs = 0, kds_bs = 0, vds_bs = 0;             // their batch strides (0: one row for every batch)
    int64_t batch = 0, heads_q = 0, heads_kv = 0, nq = 0, nk = 0;
    int dtype = 0;                                          // of o: FA_DTYPE_F16 / FA_DTYPE_BF16
    int64_t q_bs = 0, q_hs = 0, q_ts = 0, k_bs = 0, k_hs = 0, k_ts = 0, v_bs = 0, v_hs = 0, v_ts = 0, o_bs = 0, o_hs = 0, o_ts = 0;
    int causal = 0;
    float scale = 0.f;
    void* workspace = nullptr;                              // fp8in_workspace_bytes(batch * heads_kv, nk, d)
    int64_t d = 128;                                        // the head dim: 128, or 64 / 256 through launch_fp8_inputs_hdim alone
};
size_t fp8in_workspace_bytes(int64_t units_kv, int64_t nk, int64_t d = 128);
hipError_t launch_fp8_inputs(const Fp8InArgs& a, hipStream_t st);

// What the _mod entry points of the three fp8 calls add (fa_fp8_forward_mod, fa_fp8_forward_varlen_mod,
// fa_fp8_forward_kvcache_mod): a sliding window (-1: unbounded; causal sets the right bound to 0), a softcap (0: off) and one
// sink logit per query head (device float32, natural-log units; null: none).  A call whose Fp8Mod is not any() is its parent
// call, launch for launch; any other takes the featured kernels (fwd_fp8in_mod_kernel, fp8kv_split_mod_kernel).
struct Fp8Mod {
    int64_t window_left = -1, window_right = -1;
    double softcap = 0.0;
    const float* sinks = nullptr;
    int64_t sink_heads = 0;
    bool any() const { return window_left >= 0 || window_right >= 0 || softcap > 0.0 || sinks != nullptr; }
};
hipError_t launch_fp8_inputs_mod(const Fp8InArgs& a, const Fp8Mod& m, hipStream_t st);
// The _hdim entry points of the three fp8 calls (fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim, fa_fp8_forward_kvcache_hdim):
// a.d in {64, 128, 256}.  a.d == 128 is the _mod launcher above, launch for launch; 64 and 256 run the head-dim instantiations of
// the featured kernels (fwd_fp8in_hdim_kernel<.., D>, fp8kv_split_mod_kernel<.., D>) whether or not the Fp8Mod is any().
hipError_t launch_fp8_inputs_hdim(const Fp8InArgs& a, const Fp8Mod& m, hipStream_t st);

// The packed and the paged form (fa_fp8_forward_varlen): q (total_q, heads_q, 128) and o, lse as the varlen calls lay them out;
// k, v (total_k, heads_kv, 128), or with block_table the pools (num_blocks, page_size, heads_kv, 128).  Strides in bytes.
struct Fp8InVarArgs {
    const void *q = nullptr, *k = nullptr, *v = nullptr;
    void* o = nullptr;                                      // (total_q, heads_q, 128) contiguous
    float* lse = nullptr;                                   // (heads_q, total_q) contiguous
    const float *q_descale = nullptr, *k_descale = nullptr, *v_descale = nullptr;   // (batch, heads_kv) device floats; null: 1
    int64_t qds_bs = 0, kds_bs = 0, vds_bs = 0;
    const int *cu_q = nullptr, *cu_k = nullptr;             // [batch + 1] untrusted device offsets
    const int* block_table = nullptr;                       // (batch, max_blocks) untrusted page numbers; null: the packed form
    int64_t batch = 0, heads_q = 0, heads_kv = 0, total_q = 0, total_k = 0, max_q = 0, max_k = 0;
    int dtype = 0;                                          // of o: FA_DTYPE_F16 / FA_DTYPE_BF16
    int64_t q_ts = 0, q_hs = 0, k_ts = 0, k_hs = 0, v_ts = 0, v_hs = 0;
    int64_t max_blocks = 0, num_blocks = 0, page_size = 0, k_ps = 0, v_ps = 0;   // the pools: page strides
    int causal = 0;
    float scale = 0.f;
    void* workspace = nullptr;                              // fp8in_varlen_workspace_bytes
    int64_t d = 128;                                        // the head dim: 128, or 64 / 256 through launch_fp8_inputs_varlen_hdim alone
};
// from batch, heads_kv, total_k (packed: page_size == 0) or max_k, max_blocks, page_size (paged) alone
size_t fp8in_varlen_workspace_bytes(const Fp8InVarArgs& a);
hipError_t launch_fp8_inputs_varlen(const Fp8InVarArgs& a, hipStream_t st);
hipError_t launch_fp8_inputs_varlen_mod(const Fp8InVarArgs& a, const Fp8Mod& m, hipStream_t st);
hipError_t launch_fp8_inputs_varlen_hdim(const Fp8InVarArgs& a, const Fp8Mod& m, hipStream_t st);

// fp8 KV-cache decoding (fa_fp8_decode.hip; fa_fp8_forward_kvcache): e4m3 q (batch, seqlen_q, heads_q, 128) over an e4m3 cache
// (cache_batch, cache_len, heads_kv, 128), or with block_table the pools (num_blocks, page_size, heads_kv, 128).  Strides in bytes;
// o (batch, seqlen_q, heads_q, 128) and lse (batch, heads_q, seqlen_q) contiguous.
struct Fp8KvArgs {
    const void *q = nullptr, *k_cache = nullptr, *v_cache = nullptr;
    void* o = nullptr;
    float* lse = nullptr;
    const float *q_descale = nullptr, *k_descale = nullptr, *v_descale = nullptr;   // (batch, heads_kv) device floats; null: 1
    int64_t qds_bs = 0, kds_bs = 0, vds_bs = 0;
    const int *cache_seqlens = nullptr, *block_table = nullptr, *cache_batch_idx = nullptr;   // untrusted device memory, or null
    int64_t batch = 0, heads_q = 0, heads_kv = 0, seqlen_q = 0, cache_len = 0, cache_batch = 0;   // cache_len: the capacity
    int dtype = 0;                                          // of o: FA_DTYPE_F16 / FA_DTYPE_BF16
    int64_t q_bs = 0, q_ts = 0, kc_bs = 0, kc_ts = 0, vc_bs = 0, vc_ts = 0;   // kc_bs / vc_bs: the batch or the page stride
    int64_t table_row_stride = 0, num_blocks = 0, page_size = 0;
    int causal = 0;
    float scale = 0.f;
    int64_t num_splits = 1;                                 // >= 1 (the C layer resolves 0 through fp8kv_num_splits)
    void* workspace = nullptr;                              // kv_workspace_bytes(batch, heads_q, seqlen_q, d, num_splits)
    int64_t d = 128;                                        // the head dim: 128, or 64 / 256 through launch_fp8_kvcache_hdim alone
    // launch_fp8_kvcache_varlen (null: the padded call): q and o (total_q, heads_q, d), lse (heads_q, total_q); sequence b owns the
    // tokens kv_cu_range (fa_decode_common.h) gives it from the untrusted device offsets, at most max_seqlen_q; seqlen_q, q_bs unused
    const int* cu_seqlens_q = nullptr;
    int64_t total_q = 0, max_seqlen_q = 0;
};
int fp8kv_num_splits(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len);
hipError_t launch_fp8_kvcache(const Fp8KvArgs& a, hipStream_t st);
// The featured call.  The keys a window of `window_left` lets the rows of one tile see are at most window_left + max(window_right,
// 0) + seqlen_q, whatever the lengths: fp8kv_split_len is what the split rule takes for cache_len then (the host cannot see the
// lengths, and a short window over a long capacity would be cut into splits of under one tile).  With sinks num_splits >= 2:
// the sink joins in the combine, which such a call always runs.
int64_t fp8kv_split_len(int64_t cache_len, int64_t seqlen_q, int causal, const Fp8Mod& m);
hipError_t launch_fp8_kvcache_mod(const Fp8KvArgs& a, const Fp8Mod& m, hipStream_t st);
hipError_t launch_fp8_kvcache_hdim(const Fp8KvArgs& a, const Fp8Mod& m, hipStream_t st);
// a.cu_seqlens_q == null: launch_fp8_kvcache_hdim.  Else the packed split kernel at a.d in {64, 128, 256}, a memset of the lse
// partials and the packed combine for num_splits > 1; workspace: kv_workspace_bytes(1, heads_q, total_q, d, num_splits)
hipError_t launch_fp8_kvcache_varlen(const Fp8KvArgs& a, const Fp8Mod& m, hipStream_t st);
// The fp8 decode step (fa_fp8_step.hip; fa_fp8_kvcache_step): one launch of fp8kv_step_prep_kernel appends the new tokens to the
// e4m3 cache, rotates and quantises q into a q8 buffer and writes len_eff[b] = L_b + seqlen_new; then launch_fp8_kvcache_mod runs
// on kv with q = the q8 buffer and cache_seqlens = len_eff.  kv.q / kv.q_bs / kv.q_ts describe the caller's q (bytes), in in_dtype;
// kv.cache_seqlens holds the lengths BEFORE the append (non-null); kv.workspace is the whole workspace, laid out
// [len_eff | q8 (16-bit mode without q8_out) | the attention call's partials], each part rounded up to 256 bytes.
struct Fp8StepArgs {
    Fp8KvArgs kv;
    int in_dtype = 0;                                       // of q, k_new, v_new: 1 = f16, 2 = bf16 (quantised here), 3 = e4m3 (copied)
    const void *k_new = nullptr, *v_new = nullptr;          // (batch, seqlen_new, heads_kv, 128)
    int64_t seqlen_new = 0, kn_bs = 0, kn_ts = 0, vn_bs = 0, vn_ts = 0;   // strides in bytes
    void* q8_out = nullptr;                                 // 16-bit mode: the caller's (batch, seqlen_q, heads_q, 128) e4m3 buffer, or null
    int64_t q8_bs = 0, q8_ts = 0;                           // its strides in bytes
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;   // 16-bit mode only; rows in in_dtype at strides in elements
    int64_t rotary_cos_rs = 0, rotary_sin_rs = 0, rotary_dim = 0;
    int rotary_interleaved = 0, rotary_q_per_token = 0;
    // launch_fp8_kvcache_step_varlen: k_new / v_new (total_k_new, heads_kv, d) by untrusted device offsets (null: padded, seqlen_new)
    const int* cu_seqlens_k_new = nullptr;
    int64_t total_k_new = 0;
};
size_t fp8kv_step_prep_bytes(int64_t batch, int64_t heads_q, int64_t seqlen_q, bool q8_in_workspace);   // the first two parts
hipError_t launch_fp8_kvcache_step(const Fp8StepArgs& s, const Fp8Mod& m, hipStream_t st);
// The step with packed q (kv.cu_seqlens_q), packed or padded new keys, at kv.d in {64, 128, 256} (fa_fp8_kvcache_step_varlen):
// fp8kv_step_prep_varlen_kernel, then launch_fp8_kvcache_varlen on the q8 buffer and len_eff.  The workspace's first two parts:
// len_eff (batch int32) and, with q8_in_workspace, q_tokens * heads_q * d code bytes (q_tokens: total_q, or batch * seqlen_q)
size_t fp8kv_step_prep_bytes_varlen(int64_t batch, int64_t q_tokens, int64_t heads_q, int64_t d, bool q8_in_workspace);
hipError_t launch_fp8_kvcache_step_varlen(const Fp8StepArgs& s, const Fp8Mod& m, hipStream_t st);
// kv_combine_kernel<Tag, false> (fa_decode.hip) over partials in kv_workspace_bytes' layout, for a caller outside that file
hipError_t launch_kv_combine(void* o, float* lse, float* po, float* plse, int64_t batch, int64_t heads_q, int64_t seqlen_q, int64_t d,
                             int dtype, int splits, hipStream_t st);
// kv_combine_kernel<Tag, true>: the same with the sink column of head h, sinks[h % sink_heads]
hipError_t launch_kv_combine_sink(void* o, float* lse, float* po, float* plse, int64_t batch, int64_t heads_q, int64_t seqlen_q, int64_t d,
                                  int dtype, int splits, const float* sinks, int sink_heads, hipStream_t st);
// kv_combine_kernel in its packed mode (kv_combine_row: row = h * total_q + packed token; a row whose first lse partial still holds
// the kPlseFill bytes belongs to no sequence and is left unwritten); sinks null: kv_combine_kernel<Tag, false>
hipError_t launch_kv_combine_packed(void* o, float* lse, float* po, float* plse, const int* cu_seqlens_q, int64_t heads_q, int64_t total_q,
                                    int64_t d, int dtype, int splits, const float* sinks, int sink_heads, hipStream_t st);

}  // namespace fa
