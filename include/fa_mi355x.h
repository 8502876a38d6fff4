/*
 * fa_mi355x.h — C ABI of the MI355X (gfx950) FlashAttention forward/backward library.
 *
 * This is the drop-in boundary for the hot path of PeTeRr0/FlashAttention-pytorch.
 * The six `fa*_forward/backward` entry points below are what the reference's Python
 * wrappers call on its native extension module (reference file:line, relative to the
 * reference tree):
 *
 *   csrc/common/torch.extension.cpp:74  m.def("fa1_forward",  &fa1_forward)   -> fa1_forward
 *   csrc/common/torch.extension.cpp:75  m.def("fa1_backward", &fa1_backward)  -> fa1_backward
 *   csrc/common/torch.extension.cpp:78  m.def("forward",      &fa2_forward)   -> fa2_forward
 *   csrc/common/torch.extension.cpp:79  m.def("backward",     &fa2_backward)  -> fa2_backward
 *   csrc/common/torch.extension.cpp:81  m.def("fa3_forward",  &fa3_forward)   -> fa3_forward
 *   csrc/common/torch.extension.cpp:82  m.def("fa3_backward", &fa3_backward)  -> fa3_backward
 *
 * The reference's functions take and return `torch::Tensor`; here every tensor is a
 * plain device pointer plus sizes, the caller owns all memory (inputs, outputs and the
 * backward workspace), and work is enqueued on the caller's `hipStream_t` (passed as
 * `void*`) without synchronising the device.  The Python shim
 * `flashattention-pytorch_amd/flashattention_lab_cuda/__init__.py` re-creates the
 * reference's tensor-level signatures on top of these via ctypes.
 *
 * Tensor layout (same as the reference, csrc/fa2/fa2_fwd.cu:40-54):
 *   q, k, v, o, do, dq, dk, dv : contiguous row-major (BH, N, d), element type `dtype`
 *   lse                        : contiguous (BH, N) float32, natural-log logsumexp
 * Results do not depend on the tile hints `br`, `bc`, `stages`.
 *
 * Every function returns FA_OK (0) or a negative error code; `fa_last_error()` returns a
 * thread-local message for the last failure.
 */
#ifndef FA_MI355X_H
#define FA_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_OK 0
#define FA_ERR_INVALID_ARGUMENT (-1) /* bad shape / dtype / null pointer (reference: TORCH_CHECK -> RuntimeError) */
#define FA_ERR_UNSUPPORTED (-2)      /* head_dim > 256, or no gfx950 device */
#define FA_ERR_WORKSPACE (-3)        /* workspace too small */
#define FA_ERR_LAUNCH (-4)           /* HIP launch error */

/* element type of q/k/v/o/do/dq/dk/dv */
#define FA_DTYPE_F32 0
#define FA_DTYPE_F16 1
#define FA_DTYPE_BF16 2
#define FA_DTYPE_E4M3 3 /* OCP e4m3 (float8_e4m3fn): as cache_dtype of fa_ex_forward_kvcache_fp8 / fa_ex_forward_varlen_paged_fp8; q, k, v of fa_fp8_forward are e4m3 by definition (its dtype argument names o's) */

/* Which implementation the dispatcher picks (fa_set_kernel_mode): AUTO = MFMA bf16/f16 kernels
 * when dtype is 16-bit and d is a multiple of 8 up to 256 (64 / 128 / 256 wide tiles, narrower rows zero-padded in the
 * kernel), exact-f32 MFMA kernels otherwise.
 * The mode and the fa_set_option knobs are PROCESS-GLOBAL tuning state (sweeps, A/B runs): set them before the
 * streams start working, not concurrently with calls from other threads. */
#define FA_MODE_AUTO 0
#define FA_MODE_F32_GENERIC 1
#define FA_MODE_BWD_ATOMIC 2 /* as AUTO, but the 16-bit backward is the single-kernel variant with float-atomic dQ */

/* --- FlashAttention-1 names (replaces csrc/fa1/fa1_fwd.cu:30, csrc/fa1/fa1_bwd.cu:30) --- */
int fa1_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                int64_t bh, int64_t n, int64_t d, int dtype,
                int causal, double softmax_scale, int64_t br, int64_t bc, void* stream);

int fa1_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                 void* dq, void* dk, void* dv,
                 int64_t bh, int64_t n, int64_t d, int dtype,
                 int causal, double softmax_scale, int64_t br, int64_t bc,
                 void* workspace, size_t workspace_bytes, void* stream);

/* --- FlashAttention-2 (Python names `forward` / `backward`; replaces csrc/fa2/fa2_fwd.cu:30, fa2_bwd.cu:30) --- */
int fa2_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                int64_t bh, int64_t n, int64_t d, int dtype,
                int causal, double softmax_scale, int64_t br, int64_t bc, void* stream);

int fa2_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                 void* dq, void* dk, void* dv,
                 int64_t bh, int64_t n, int64_t d, int dtype,
                 int causal, double softmax_scale, int64_t br, int64_t bc,
                 void* workspace, size_t workspace_bytes, void* stream);

/* --- FlashAttention-3 (replaces csrc/fa3/fa3_fwd.cu:172, csrc/fa3/fa3_bwd.cu:104).
 * fp8 != 0 (f16/bf16 tensors, head dims that are multiples of 8 up to 256): Q, K and V go through OCP e4m3 with one
 * scale per (bh, 64-row block); Q and K are rotated (sign + Hadamard) around the quantisation at power-of-two head dims.
 * d = 128: QK^T runs on the e4m3 MFMA; for N > 256 (unless option fp8_pv = 1) P.V does too, with P rounded to e4m3 and
 * V scaled by powers of two; otherwise P stays 16-bit and V has absmax / 448 scales.  Under the causal mask the first
 * 256 query rows always take the 16-bit P, on the same V~ as the other rows.  Other head dims: the round-tripped Q~, K~,
 * V~ feed the 16-bit kernels.  Accumulation is fp32 throughout.  The forward needs fa3_forward_workspace_bytes.
 * fp32 tensors take the regular path.  The fp8 backward differentiates attention of the same Q~, K~, V~ (cf.
 * csrc/fa3/fa3_bwd.cu:134-146) with P recomputed exactly (straight-through over the e4m3 P) and needs
 * fa3_backward_workspace_bytes. */
int fa3_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                int64_t bh, int64_t n, int64_t d, int dtype,
                int causal, double softmax_scale, int64_t br, int64_t bc, int64_t stages, int fp8,
                void* workspace, size_t workspace_bytes, void* stream);

int fa3_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                 void* dq, void* dk, void* dv,
                 int64_t bh, int64_t n, int64_t d, int dtype,
                 int causal, double softmax_scale, int64_t br, int64_t bc, int64_t stages, int fp8,
                 void* workspace, size_t workspace_bytes, void* stream);

/* --- Extended attention: the extras the reference's notebook model wires around its tiled attention,
 * src/fa3/torch/flashattention_pytorch.py (MultiHeadAttention._block_sparse_flash_attention :94-174, look_ahead_mask_ :176-190,
 * dense branch :80-87; src/common/dropout.py:3-15), as kernel features behind one entry point.
 *   q, o, do, dq : (BH, Nq, d)      k, v, dk, dv : (BH, Nk, d)      lse : (BH, Nq) float32
 *   causal != 0      : key j is visible to query i iff j <= i + (Nk - Nq)          (look_ahead_mask_, bottom-right aligned)
 *   mask             : Nq x Nk bytes, 0 = masked (masked_fill(mask == 0, -inf)); mask_bh_stride = 0 shares one mask over all
 *                      (b,h), Nq*Nk gives every (b,h) its own; NULL = none
 *   block_mask       : ceil(Nq/br) x ceil(Nk/bc) bytes, 0 = the tile is skipped (Algorithm 5 line 8); NULL = none
 *   dropout_p, seed  : standard dropout of the attention probabilities, scale 1/(1-p); an element is kept where its 16
 *                      uniform bits — a counter-based generator of (seed, b*h, i, j): one splitmix64 value per 2 x 2 quad of
 *                      (row, key) elements — are >= floor(65536 p) + 1, so the backward regenerates the same mask; 0 = none
 *   softmax_scale    : includes the model's temperature tau
 * A query row with no visible key returns o = 0, lse = -inf, dq = 0 (the reference's softmax of an all -inf row is NaN).
 * Kernels: f16 / bf16 tensors with d % 8 == 0, d <= 128, softmax_scale > 0 and block-mask blocks that are multiples of 32 run
 * on 16-bit MFMA kernels (a call without mask and dropout takes the plain fa2 kernels: square as it is; Nq != Nk at d = 128,
 * causal only with Nk >= Nq); everything else — f32, d <= 256 — on exact-f32
 * kernels.  Same results contract either way. */
int fa_ex_forward(const void* q, const void* k, const void* v, void* o, float* lse,
                  int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype,
                  int causal, double softmax_scale,
                  const uint8_t* mask, int64_t mask_bh_stride,
                  const uint8_t* block_mask, int64_t br, int64_t bc,
                  double dropout_p, uint64_t dropout_seed, void* stream);

int fa_ex_backward(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                   void* dq, void* dk, void* dv,
                   int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype,
                   int causal, double softmax_scale,
                   const uint8_t* mask, int64_t mask_bh_stride,
                   const uint8_t* block_mask, int64_t br, int64_t bc,
                   double dropout_p, uint64_t dropout_seed,
                   void* workspace, size_t workspace_bytes, void* stream);

size_t fa_ex_backward_workspace_bytes(int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype);
/* The size with which a call WITHOUT mask, block-sparse mask and dropout (extras = 0) hands dS from its dK/dV kernel to its dQ
 * kernel, as fa_backward_workspace_bytes_fast does for the square backward and by the same rule (d = 128, 16-bit tensors; Nq != Nk
 * included, under the causal mask with Nk >= Nq; at most 4 GiB more).  Equals fa_ex_backward_workspace_bytes where that does not apply. */
size_t fa_ex_backward_workspace_bytes_fast(int64_t bh, int64_t nq, int64_t nk, int64_t d, int dtype, int causal, int extras);

/* --- Grouped-query attention (GQA; MQA at kv_group = BH / B): K and V with fewer heads than Q.  The fa_ex_* calls above with
 * kv_group = H_q / H_kv right after bh; kv_group = 1 is exactly the fa_ex_* call.
 *   q, o, do, dq : (BH, Nq, d) with BH = B * H_q      k, v, dk, dv : (BH / kv_group, Nk, d)      lse : (BH, Nq) float32
 *   query unit u reads K/V unit u / kv_group (= b * H_kv + h / kv_group: heads are b-major); mask_bh_stride, the dropout counter
 *   and lse stay indexed by the query unit.  kv_group >= 1 and BH % kv_group == 0, else FA_ERR_INVALID_ARGUMENT.
 * The backward runs the dK/dV kernels with one output per query head into two partial slabs of the workspace and sums each group
 * into dk and dv (fp32, member 0 first, one rounding): deterministic, the same bits on every run.
 * Workspace: fa_ex_backward_workspace_bytes_grouped = fa_ex_backward_workspace_bytes for BH query units, plus for kv_group > 1 the
 * two slabs, 2 * round_up(BH * Nk * d * sizeof(dtype), 256) bytes.  _fast_grouped adds the dS hand-over's room by the rule of
 * fa_ex_backward_workspace_bytes_fast (chunks of whole groups).  Same kernels as the fa_ex_* calls, with the exception of the
 * plain path's exact-f32 kernels: square calls of f32 tensors without extras take the extended exact-f32 kernels instead. */
int fa_ex_forward_grouped(const void* q, const void* k, const void* v, void* o, float* lse,
                          int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                          int causal, double softmax_scale,
                          const uint8_t* mask, int64_t mask_bh_stride,
                          const uint8_t* block_mask, int64_t br, int64_t bc,
                          double dropout_p, uint64_t dropout_seed, void* stream);

int fa_ex_backward_grouped(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                           void* dq, void* dk, void* dv,
                           int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                           int causal, double softmax_scale,
                           const uint8_t* mask, int64_t mask_bh_stride,
                           const uint8_t* block_mask, int64_t br, int64_t bc,
                           double dropout_p, uint64_t dropout_seed,
                           void* workspace, size_t workspace_bytes, void* stream);

size_t fa_ex_backward_workspace_bytes_grouped(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype);
size_t fa_ex_backward_workspace_bytes_fast_grouped(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                                                   int causal, int extras);

/* --- Sliding-window (local) attention: the fa_ex_*_grouped calls with window_left, window_right right after causal
 * (FlashAttention-2's window_size).  In the causal flag's coordinates (bottom-right aligned, coff = Nk - Nq) key j is visible to
 * query row i iff
 *     (window_left  < 0  or  j >= i + coff - window_left)   and   (window_right < 0  or  j <= i + coff + window_right)
 *     and (causal == 0 or j <= i + coff), the dense mask, the block-sparse mask and the row / key ranges, as fa_ex_*.
 * -1 = unbounded on that side; any other negative bound is FA_ERR_INVALID_ARGUMENT (checked before any HIP call).  Dropout
 * counters, lse and the GQA indexing are those of the call without a window.  A row without a visible key gives o = 0,
 * lse = -inf, dq = 0, a key that no row sees dk = dv = 0.  The bounds are canonicalised first: a left bound >= Nk - 1 or a right
 * bound >= Nq - 1 bounds nothing and is dropped, so is a right bound >= 0 under the causal mask, and window_right = 0 without it
 * is the causal mask.  What is left of a window that bounds nothing is exactly the fa_ex_*_grouped call (kv_group = 1: the
 * fa_ex_* call): the same kernels, the same bits.  A window that bounds something runs on the extended kernels only — 16-bit
 * MFMA where fa_ex_* would take them, exact f32 otherwise — which visit the key (query) tiles of each row's (key's) band and
 * no others: O(N w) work instead of O(N^2).  The backward's workspace is fa_ex_backward_workspace_bytes_grouped: a window adds
 * no storage, and the dS hand-over does not serve it — pass extras = 1 to fa_ex_backward_workspace_bytes_fast_grouped when the
 * window bounds something. */
int fa_ex_forward_window(const void* q, const void* k, const void* v, void* o, float* lse,
                         int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                         int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                         const uint8_t* mask, int64_t mask_bh_stride,
                         const uint8_t* block_mask, int64_t br, int64_t bc,
                         double dropout_p, uint64_t dropout_seed, void* stream);

int fa_ex_backward_window(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                          void* dq, void* dk, void* dv,
                          int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                          int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                          const uint8_t* mask, int64_t mask_bh_stride,
                          const uint8_t* block_mask, int64_t br, int64_t bc,
                          double dropout_p, uint64_t dropout_seed,
                          void* workspace, size_t workspace_bytes, void* stream);

/* --- Variable-length (packed) sequences: FlashAttention-2's varlen layout.  Sequence b (0 <= b < batch) is tokens
 * [cu_seqlens_q[b], cu_seqlens_q[b+1]) of q, o, do, dq and [cu_seqlens_k[b], cu_seqlens_k[b+1]) of k, v, dk, dv; cu_seqlens_* are
 * int32 device arrays of batch + 1 entries.
 *     q (total_q, heads_q, d), token stride q_stride elements (>= heads_q * d; the heads of a token adjacent at stride d);
 *     k, v (total_k, heads_kv, d), token strides k_stride, v_stride (>= heads_kv * d): views such as qkv.unbind(1) of a
 *     (total, 3, H, d) projection go in without a copy;  o, do, dq (total_q, heads_q, d) and dk, dv (total_k, heads_kv, d)
 *     dense;  lse (heads_q, total_q) float32.
 * Attention never crosses a sequence.  In each sequence, with len_q, len_k its lengths and coff = len_k - len_q, the fa_ex_*_window
 * rules hold in the sequence's own coordinates: causal is bottom-right aligned per sequence, the window (window_left,
 * window_right) bounds keys to [i + coff - window_left, i + coff + window_right], query head h reads K/V head
 * h / (heads_q / heads_kv).  A row without a visible key gives o = 0, lse = -inf, dq = 0; a key no row sees dk = dv = 0 (every
 * key of a sequence with len_q = 0).  Empty sequences are allowed.
 * Dropout: unit u = b * heads_q + h, row and key inside the sequence, ceil(max_seqlen_q / 2) row pairs per unit — the counters of
 * the padded (batch * heads_q, max_seqlen_q, max_seqlen_k) fa_ex call, so its keep mask restricted to [u, :len_q, :len_k] is this
 * call's.  The mask therefore depends on the max_seqlen_q passed.
 * cu_seqlens are not read on the host (that would take a synchronise) and are not trusted: the kernels use
 * start = clamp(cu[b], 0, total), end = clamp(cu[b+1], start, total), len = min(end - start, max_seqlen), so that malformed
 * offsets never make them read or write outside the packed tensors.  Outputs at tokens that no sequence covers are unspecified.
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT): dtype, batch >= 1, heads_q a positive multiple of heads_kv, d > 0,
 * totals and max_seqlen >= 0, strides >= heads * d, non-null cu_seqlens where the total is > 0, window bounds >= -1, the NaN
 * scale, dropout_p in [0, 1), batch * heads_q * ceil(max_seqlen_q / 2) < 2^32.  The window is canonicalised against max_seqlen_q
 * and max_seqlen_k (a bound that cuts nothing there cuts nothing in any sequence).  No dense or block-sparse mask.
 * Kernels: the extended ones only — 16-bit MFMA for f16 / bf16, d % 8 == 0, d <= 128, strides multiples of 8 elements, 16-byte
 * aligned tensors and max_seqlen * stride * 2 < 2^31; exact f32 otherwise (d <= 256).  The grid is that of the padded call:
 * ceil(max_seqlen / tile) * batch * heads_q workgroups, those past their sequence's end leave at once.
 * Backward workspace: fa_ex_backward_workspace_bytes_varlen (row constants; with heads_kv < heads_q also the per-query-head dK / dV
 * partials, (total_k, heads_q, d) each, which are added in fp32 over each group in a fixed order). */
int fa_ex_forward_varlen(const void* q, const void* k, const void* v, void* o, float* lse,
                         const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv,
                         int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype,
                         int64_t q_stride, int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                         double softmax_scale, double dropout_p, uint64_t dropout_seed, void* stream);

int fa_ex_backward_varlen(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                          void* dq, void* dk, void* dv,
                          const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv,
                          int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype,
                          int64_t q_stride, int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                          double softmax_scale, double dropout_p, uint64_t dropout_seed,
                          void* workspace, size_t workspace_bytes, void* stream);

size_t fa_ex_backward_workspace_bytes_varlen(int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t d, int dtype);

/* --- Score modifiers: FlashAttention-2's softcap and alibi_slopes.  With s = softmax_scale * q_i . k_j and coff = Nk - Nq (per
 * sequence in the varlen calls), the score that enters the softmax is
 *     s'  = softcap * tanh(s / softcap)               if softcap > 0, else s
 *     s'' = s' - slope(u) * |i + coff - j|            if alibi_slopes != NULL
 * and lse is the logsumexp of s'' over the visible keys (causal, window, masks and row / key ranges as in fa_ex_*_window and
 * fa_ex_*_varlen).  Query unit u takes slope alibi_slopes[(u / alibi_heads) * alibi_batch_stride + u % alibi_heads]: stride 0 is
 * FlashAttention-2's (H,) form, stride alibi_heads its (B, H) form; alibi_heads = bh with stride 0 gives one slope per unit.  The
 * varlen calls use alibi_heads = heads_q (u = b * heads_q + h, slope alibi_slopes[b * alibi_batch_stride + h]).  The slopes are
 * float32 device memory, read by the kernels only (no synchronise), and receive no gradient; the softcap is differentiated
 * (ds'/ds = 1 - tanh^2(s / softcap)).  Dropout, the dead-row and dead-key conventions and the GQA indexing are unchanged.
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT): softcap finite and >= 0, alibi_batch_stride >= 0, and with slopes
 * alibi_heads >= 1 dividing bh.  softcap = 0 without slopes is exactly the fa_ex_*_window / fa_ex_*_varlen call.  A call with a
 * modifier runs on the extended kernels only (16-bit MFMA where fa_ex_* would take them, exact f32 otherwise).  Workspaces are
 * those of the calls without modifiers; the dS hand-over does not serve them — pass extras = 1 to
 * fa_ex_backward_workspace_bytes_fast_grouped. */
int fa_ex_forward_scoremod(const void* q, const void* k, const void* v, void* o, float* lse,
                           int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                           int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                           double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride,
                           const uint8_t* mask, int64_t mask_bh_stride,
                           const uint8_t* block_mask, int64_t br, int64_t bc,
                           double dropout_p, uint64_t dropout_seed, void* stream);

int fa_ex_backward_scoremod(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                            void* dq, void* dk, void* dv,
                            int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype,
                            int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                            double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride,
                            const uint8_t* mask, int64_t mask_bh_stride,
                            const uint8_t* block_mask, int64_t br, int64_t bc,
                            double dropout_p, uint64_t dropout_seed,
                            void* workspace, size_t workspace_bytes, void* stream);

int fa_ex_forward_varlen_scoremod(const void* q, const void* k, const void* v, void* o, float* lse,
                                  const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q,
                                  int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k,
                                  int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride, int causal,
                                  int64_t window_left, int64_t window_right, double softmax_scale,
                                  double softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                                  double dropout_p, uint64_t dropout_seed, void* stream);

int fa_ex_backward_varlen_scoremod(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                                   void* dq, void* dk, void* dv,
                                   const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q,
                                   int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k,
                                   int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride, int causal,
                                   int64_t window_left, int64_t window_right, double softmax_scale,
                                   double softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                                   double dropout_p, uint64_t dropout_seed,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* --- KV-cache decoding with split-KV: FlashAttention-2's flash_attn_with_kvcache, forward only (the paged cache, cache_batch_idx
 * and cache_leftpad: fa_ex_forward_kvcache_paged below; rotary embedding: fa_ex_forward_kvcache_rotary below).
 * Layouts are batch first, tokens second; within a token the heads are adjacent at stride d; each tensor has its own batch and
 * token stride (elements), so views such as kv.unbind(2) of a (B, cache_len, 2, H_kv, d) buffer go in without a copy:
 *     q (batch, seqlen_q, heads_q, d);  k_cache, v_cache (batch, cache_len, heads_kv, d);  k_new, v_new (batch, seqlen_new, heads_kv, d);
 *     o (batch, seqlen_q, heads_q, d) dense, q's dtype;  lse (batch, heads_q, seqlen_q) float32 dense.
 * For batch element b, L_b = clamp(cache_seqlens[b], 0, cache_len - seqlen_new) (cache_seqlens: int32 (batch,) device memory, not read
 * on the host and not trusted; NULL: L_b = cache_len, and seqlen_new must be 0).  k_new / v_new are first written in place into
 * k_cache[b, L_b : L_b + seqlen_new] and v_cache[...]; nothing else in the caches changes.  Then queries attend over keys
 * [0, len_k), len_k = L_b + seqlen_new, under the fa_ex_*_window / fa_ex_*_scoremod rules with coff = len_k - seqlen_q: causal is
 * bottom-right aligned, the window bounds key j to [i + coff - window_left, i + coff + window_right] (-1 = unbounded), softcap and
 * ALiBi (slope of (b, h): alibi_slopes[b * alibi_batch_stride + h], float32; stride 0 = the (H_q,) form) with distance
 * |i + coff - j|, query head h reads K/V head h / (heads_q / heads_kv).  A row without a visible key gives o = 0, lse = -inf.
 * Kernels (csrc/fa_decode.hip): an append launch when seqlen_new > 0; one wave per (split, 16-row tile of the heads_q / heads_kv *
 * seqlen_q query rows that share a K/V head, K/V head, b) reads its share of the cache once; with num_splits S > 1 a combine launch
 * merges the fp32 partials in split order (deterministic).  Split s takes 32-key tiles [floor(s nt / S), floor((s + 1) nt / S)) of
 * the tile's visible band, cut from its first key; the band and nt follow len_k on the device.  num_splits = 0 takes the library's
 * rule, which reads shapes only (batch, heads_kv, row tiles, cache_len and the MI355X's 256 CUs), so the call never synchronises or
 * allocates and can be captured in a graph.  The workspace (fa_ex_kvcache_workspace_bytes with the same num_splits; 0 bytes for
 * S = 1) holds batch * heads_q * seqlen_q * S rows of d floats, then as many floats of lse, each part rounded up to 256 bytes.
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT): dtype f16 or bf16; d a multiple of 8 in [8, 256]; batch in [1, 65535];
 * heads_q a positive multiple of heads_kv; seqlen_q >= 1; cache_len >= 1; seqlen_new in [0, cache_len]; token strides >= heads * d,
 * batch strides (batch > 1) >= (tokens - 1) * token stride + heads * d, all strides multiples of 8 (k_new / v_new only when
 * seqlen_new > 0); seqlen_new > 0 with cache_seqlens, k_new and v_new; window bounds >= -1; a finite softmax_scale > 0; softcap
 * finite and >= 0; alibi_batch_stride >= 0; num_splits in [0, 256]; the workspace; non-null q, caches, o, lse; 16-byte aligned
 * tensors.  FA_ERR_UNSUPPORTED: a batch element of any tensor spanning 2^31 bytes or more (batch offsets are 64-bit, so the
 * caches as a whole may be larger), cache_len > 2^28, seqlen_q > 2^24, and with S > 1 batch * heads_q * seqlen_q >= 2^26 (the
 * combine launch).  The window is canonicalised first: window_left >= cache_len - 1 and window_right >= seqlen_q - 1 cut no key
 * in any row and are taken as -1, so any bound up to INT64_MAX means unbounded. */
int fa_ex_forward_kvcache(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new, const int32_t* cache_seqlens,
                          void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_new,
                          int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride, int64_t q_token_stride,
                          int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                          int64_t v_cache_token_stride, int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                          int64_t v_new_token_stride, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                          double softcap, const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, void* workspace,
                          size_t workspace_bytes, void* stream);

/* fa_ex_forward_kvcache with a paged cache (block_table), continuous batching (cache_batch_idx) and left-padded prompts
 * (cache_leftpad), as in FlashAttention-2.  All three null with the five integers 0 is fa_ex_forward_kvcache, bit for bit.
 * Everything not named here keeps its meaning; all three arrays are int32 device memory, never read on the host and not trusted.
 *
 * block_table (batch, max_blocks_per_seq), rows at block_table_row_stride entries.  k_cache / v_cache are pools
 * (num_blocks, page_block_size, heads_kv, d): the two "batch" strides are the page strides, the token strides as before (each pool
 * its own, so pool.unbind(1) of a (num_blocks, 2, ps, heads_kv, d) buffer goes in without a copy).  With ps = page_block_size, token
 * t of sequence b lives at pool[block_table[b, t / ps], t % ps], element offset
 *     block_table[b, t / ps] * page_stride + (t % ps) * token_stride + head * d + i.
 * cache_len is ignored: the capacity max_blocks_per_seq * ps takes its place everywhere (the cache_seqlens clamp, seqlen_new's
 * bound, the num_splits = 0 rule, the window canonicalisation; ask fa_ex_kvcache_workspace_bytes with the capacity as cache_len).
 * k_new / v_new go through the table to tokens L_b .. L_b + seqlen_new - 1.  ps is any positive multiple of 16; page offsets are
 * 64-bit (a pool may be larger than 4 GiB), offsets inside a page 32-bit.  Only entries j < ceil(len_k / ps) of row b are read.
 * An entry outside [0, num_blocks) never leads to an access outside the pools: the tokens of that page read as zero K and zero V
 * (they still take part in the softmax, with score 0), and an append to it is dropped.  Several sequences may name the same page
 * (prefix sharing) for reading; appending to one page from two sequences in one call is undefined.
 *
 * cache_batch_idx (batch,), contiguous cache only: sequence b uses k_cache[idx[b]] / v_cache[idx[b]] of a cache with cache_batch
 * rows (which may differ from batch); the append lands in that row and no other row changes.  An index outside [0, cache_batch)
 * reads as zeros and drops the append.  Two sequences with the same index and seqlen_new > 0 are undefined.
 *
 * cache_leftpad (batch,), contiguous cache only: with L_b as before (cache_seqlens counts from cache position 0) and
 * P_b = clamp(cache_leftpad[b], 0, L_b), the keys of sequence b are cache positions [P_b, L_b + seqlen_new): len_k = L_b +
 * seqlen_new - P_b, and causal alignment, window, ALiBi distance and the split rule use these local coordinates (coff = len_k -
 * seqlen_q).  k_new / v_new are still written at L_b.  cache_batch_idx and cache_leftpad may be combined.
 *
 * Checked before any HIP call, besides fa_ex_forward_kvcache's list (FA_ERR_INVALID_ARGUMENT): block_table together with
 * cache_batch_idx or cache_leftpad; page_block_size a positive multiple of 16; num_blocks and max_blocks_per_seq >= 1; block_table
 * 4-byte aligned with block_table_row_stride >= max_blocks_per_seq; the four table integers 0 without block_table; cache_batch >= 1
 * with cache_batch_idx and 0 without; the cache strides, for a page of ps tokens (num_blocks > 1: page stride >= (ps - 1) * token
 * stride + heads_kv * d) or for cache_batch rows.  FA_ERR_UNSUPPORTED: a capacity above 2^28 tokens; a page spanning 2^31 bytes
 * or more. */
int fa_ex_forward_kvcache_paged(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                                const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                                int64_t seqlen_q, int64_t seqlen_new, int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride,
                                int64_t q_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                                int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t k_new_batch_stride,
                                int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int causal,
                                int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                                const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, const int32_t* block_table,
                                int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                                const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad, void* workspace,
                                size_t workspace_bytes, void* stream);

/* fa_ex_forward_kvcache_paged with rotary position embedding fused into the call, as in FlashAttention-2 (rotary_cos, rotary_sin,
 * rotary_interleaved).  Null tables with the five integers 0 is fa_ex_forward_kvcache_paged, bit for bit.  Everything not named here
 * keeps its meaning.
 *
 * rotary_cos, rotary_sin (seqlen_ro, rotary_dim / 2): device memory in q's dtype, last dim contiguous, rows at
 * rotary_cos_row_stride / rotary_sin_row_stride elements.  rotary_dim is a multiple of 16 in [16, d]; head-dim elements at and past
 * it pass through unchanged.  rotary_interleaved != 0: the pairs are elements (2j, 2j + 1) (GPT-J); 0: (j, j + rotary_dim / 2)
 * (GPT-NeoX).  A pair (x, y) with table entry j at table row `position` becomes
 *     x' = x cos[position, j] - y sin[position, j],   y' = x sin[position, j] + y cos[position, j],
 * evaluated in fp32 from the 16-bit inputs and rounded once to the 16-bit dtype.
 * Positions are the sequence's own key coordinates, the ones causal, window and ALiBi use: with L_b and P_b as above (the clamps
 * included; P_b = 0 without cache_leftpad), new key token n of sequence b has position L_b - P_b + n.  k_new[b, n] is rotated there
 * and the rotated value is what the cache receives (contiguous, indexed, left-padded or paged); v_new is appended as it is.  q token
 * i is rotated at position L_b - P_b + i when causal is set or a window bound is given, and otherwise every q token at L_b - P_b.
 * "Given" is decided on window_left / window_right as the caller passed them (>= 0), before the canonicalisation described above: a
 * bound so large that it cuts no key, and is therefore taken as -1 for masking, still selects the per-token positions.  q itself is
 * not modified; only the kernel's operand is.
 * The tables are read on the device without a bounds check.  Instead the call requires
 *     seqlen_ro >= capacity + max(0, seqlen_q - seqlen_new),   capacity = cache_len, or max_blocks_per_seq * page_block_size,
 * and since L_b <= capacity - seqlen_new after the clamp, every position used is below seqlen_ro whatever cache_seqlens and
 * cache_leftpad hold.  (FlashAttention-2 does not check its tables against a paged cache's capacity; this call does, so a table
 * that FlashAttention-2 accepts for a paged call can be refused here.)
 * Checked before any HIP call, besides fa_ex_forward_kvcache_paged's list (FA_ERR_INVALID_ARGUMENT): one table without the other;
 * rotary_dim not a multiple of 16 in [16, d]; rotary with seqlen_new = 0 or without cache_seqlens; seqlen_ro below the bound; a
 * row stride below rotary_dim / 2, or odd; a table that is not 4-byte aligned; any of the five integers non-zero without tables.
 * The workspace is fa_ex_forward_kvcache_paged's. */
int fa_ex_forward_kvcache_rotary(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                                 const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                                 int64_t seqlen_q, int64_t seqlen_new, int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride,
                                 int64_t q_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                                 int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t k_new_batch_stride,
                                 int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int causal,
                                 int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                                 const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, const int32_t* block_table,
                                 int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                                 const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                                 const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                                 int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* fa_ex_forward_kvcache_rotary with a cache stored in 8 bits: k_cache and v_cache hold OCP e4m3 (float8_e4m3fn: 1 byte, finite
 * max 448, no infinities) with a float32 dequantisation scale per (sequence, K/V head), as FlashAttention-3's k_descale / v_descale.
 * cache_dtype = dtype with null scales and descale_batch_stride = 0 is fa_ex_forward_kvcache_rotary, bit for bit.  Everything not
 * named here keeps its meaning; q, k_new, v_new, o and the rotary tables stay in dtype (f16 or bf16), lse and the workspace fp32.
 *
 * cache_dtype: dtype (a 16-bit cache, no scales) or FA_DTYPE_E4M3, for both caches.  The MI300X fnuz variant and e5m2 have no code.
 * k_descale, v_descale: float32 device memory, read by the kernels only (no host read, no synchronisation: the call can still be
 * captured in a graph).  The scale of K head h of sequence b is k_descale[b * descale_batch_stride + h]; stride 0 is the (heads_kv,)
 * form, one row for every sequence.  b is the sequence of the call: cache_batch_idx and block_table do not move it.  A stored byte
 * c stands for e4m3(c) * k_descale[b, h] (V: v_descale).  A null scale means 1.0.  Scales must be finite and > 0; not checked.
 *
 * Reading.  e4m3 -> f16 / bf16 is exact, so the split kernel widens K and V to dtype in registers and runs the 16-bit loop; q and
 * the probabilities are not quantised.  The scales enter in fp32: the score is softmax_scale * k_descale[b, hk] * (q . k_stored),
 * scaled before softcap and ALiBi, and v_descale[b, hk] multiplies the normalised output once, before its single rounding to dtype
 * (one split) or before the fp32 partial is stored (more).  The result is that of fa_ex_forward_kvcache_rotary on the dequantised
 * cache up to these two fp32 multiplies; lse is the logsumexp of the scaled, modified scores.
 *
 * Appending.  k_new is first rotated and rounded to dtype exactly as fa_ex_forward_kvcache_rotary does (when tables are given);
 * v_new is taken as it is.  Each 16-bit value x then becomes a byte by
 *     inv = 1.0f / descale (correctly rounded fp32);   y = clamp(float(x) * inv, -448, 448) in fp32;   byte = e4m3(y), nearest even.
 * The clamp precedes the conversion, so values beyond the range store +-448 (0x7e / 0xfe) and a finite x never stores the NaN
 * code; NaN input is unspecified.  The position clamp, the paged translation, dropped appends and cache_leftpad are unchanged.
 *
 * Strides of the e4m3 caches are in elements, which are bytes, and keep the multiple-of-8 rule; k_cache and v_cache must be 8-byte
 * aligned (a chunk of 8 head dims is one 8-byte load or store), all other tensors 16-byte aligned as before.  The 2^31 limits are on
 * bytes: a batch element or page of an e4m3 cache may span up to 2^31 - 1 elements, twice the tokens of a 16-bit one.
 * Checked before any HIP call, besides fa_ex_forward_kvcache_rotary's list (FA_ERR_INVALID_ARGUMENT): cache_dtype neither dtype nor
 * FA_DTYPE_E4M3; a scale or a non-zero descale_batch_stride with a 16-bit cache; descale_batch_stride negative, or non-zero and
 * below heads_kv; a scale that is not 4-byte aligned; an e4m3 cache that is not 8-byte aligned.  The workspace is
 * fa_ex_forward_kvcache's (fa_ex_kvcache_workspace_bytes does not depend on the cache's type). */
int fa_ex_forward_kvcache_fp8(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                              const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                              int64_t seqlen_q, int64_t seqlen_new, int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride,
                              int64_t q_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                              int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t k_new_batch_stride,
                              int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int causal,
                              int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                              const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, const int32_t* block_table,
                              int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                              const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                              const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                              int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                              int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                              void* workspace, size_t workspace_bytes, void* stream);

/* bytes of workspace a fa_ex_forward_kvcache call with these shapes and num_splits needs (0 for S = 1 and for invalid shapes) */
size_t fa_ex_kvcache_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len, int64_t d,
                                     int64_t num_splits);

/* --- Attention sinks (gpt-oss; `sinks` / `s_aux` of FlashAttention-3 and the serving stacks): every head carries one learnable
 * logit that joins each row's softmax as an extra column with a zero value vector, so a row can give weight to nothing.  For query
 * row i of head h with visible-key logits s_ij (after softcap and ALiBi, as the *_scoremod calls define them):
 *     lse_i = log(exp(sink_h) + sum_j exp(s_ij))        o_i = sum_j exp(s_ij - lse_i) * keep_ij / (1 - p) * v_j
 * The sink is in the units of the final logit (natural log); it is not softcapped, biased, masked, windowed or dropped.  The returned
 * lse contains it (the backward needs that).  A row without a visible key gives o = 0 and lse = sink_h (-inf without sinks).  The
 * normaliser is formed around max(row max, sink), so sinks of +-1e4 are safe.  sinks[h] = -inf means "no sink for this head": o and
 * lse of that head are the bits of the call without sinks, and its gradient is 0.  NaN / +inf are undefined.
 * sinks: float32 (sink_heads,) in device memory, read by the kernels only (no host read, no synchronisation).  Query unit u takes
 * sinks[u % sink_heads] (the varlen and KV-cache calls: query head h takes sinks[h % sink_heads]).  The remaining arguments are those
 * of fa_ex_*_scoremod / fa_ex_*_varlen_scoremod / fa_ex_forward_kvcache_fp8; sinks == NULL is exactly that call (sink_heads and dsinks
 * are then not read).
 * Backward: dq, dk, dv as before from the sink-including lse, and dsinks[h] = - sum over the rows i of the units of head h of
 * exp(sink_h - lse_i) * rowsum(dO_i * O_i), float32 (sink_heads,), summed in a fixed order without atomics (the same bits on every
 * run).  The workspace is that of the call without sinks.
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT): sinks (and dsinks) 4-byte aligned; sink_heads >= 1 dividing the number of
 * query units (BH; heads_q for the varlen and KV-cache calls); a backward with sinks needs dsinks. */
int fa_ex_forward_sink(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                       int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                       double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks,
                       int64_t sink_heads, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc,
                       double dropout_p, uint64_t dropout_seed, void* stream);
int fa_ex_backward_sink(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p,
                        uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream);
int fa_ex_forward_varlen_sink(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                              const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                              int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                              int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                              double softmax_scale, double softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                              const float* sinks, int64_t sink_heads, double dropout_p, uint64_t dropout_seed, void* stream);
int fa_ex_backward_varlen_sink(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq,
                               void* dk, void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch,
                               int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q,
                               int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int causal, int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                               const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads,
                               float* dsinks, double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes,
                               void* stream);
/* --- A gradient of lse in the extended backward: what a merge of partial results (fa_merge_states) sends back to the attention
 * call of each key chunk, in ring / context-parallel training.  With P = exp(S - lse), dP = dO V^T and delta = rowsum(dO * O), a
 * gradient dlse on a row's lse gives
 *     dS = P * (dP - delta + dlse)
 * and leaves dV as it is; with sinks, dsinks[h] = sum over the rows of head h of exp(sink_h - lse) * (-delta + dlse).  So dlse
 * enters the whole backward through the one row constant its kernels read, -delta + dlse, and through nothing else.
 * dlse: float32 in lse's own layout, (BH, Nq), for the varlen call (heads_q, total_q); device memory on the tensors' device, 4-byte
 * aligned (checked, FA_ERR_INVALID_ARGUMENT, after the sink checks), read by the kernels only.  It sits after the sink group and
 * before the masks / dropout group; the remaining arguments, their checks and the order of those are fa_ex_backward_sink's /
 * fa_ex_backward_varlen_sink's, and so is the workspace.  dlse == NULL is exactly that call: the same launches, the same bits.
 * Rows whose lse is -inf (no visible key and no sink) ignore their dlse, whatever it holds, and keep dq = 0.
 * A call with dlse != NULL runs the recomputing extended kernels (the 16-bit MFMA ones where they take the call, the exact-f32
 * ones otherwise), whose row-constant pre-pass is a launch of its own: the plain kernels and the dS hand-over form -delta inside
 * their matrix kernels and are not used.  fa_ex_backward_workspace_bytes_fast answers for such a call with extras = 1.  A call with
 * query rows, no key, sinks and dlse gives dsinks[h] = the sum of dlse over the head's rows (every lse there is the sink). */
int fa_ex_backward_dlse(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const float* dlse, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br,
                        int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes, void* stream);
int fa_ex_backward_varlen_dlse(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq,
                               void* dk, void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch,
                               int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q,
                               int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int causal, int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                               const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads,
                               float* dsinks, const float* dlse, double dropout_p, uint64_t dropout_seed, void* workspace,
                               size_t workspace_bytes, void* stream);
/* --- V narrower than Q and K: attention whose q, k (dq, dk) are d wide while v, o, do_ (dv) are d_v wide, as FlashAttention-2
 * (>= 2.7, head dim 192 / 128) and FlashAttention-3 take it.  DeepSeek-style multi-head latent attention before weight absorption,
 * in training and prefill: d = 192 (128 nope + 64 rope), d_v = 128.  One argument, d_v, after the sink group (forward) and after
 * dlse (backward), in front of the masks / dropout group; the remaining arguments are those of fa_ex_forward_sink /
 * fa_ex_backward_dlse / fa_ex_forward_varlen_sink / fa_ex_backward_varlen_dlse.  d_v = 0 and d_v = d are exactly that call: the same
 * checks, the same launches, the same bits.
 *   Layout with d_v != d: q, dq (BH, Nq, d); k, dk (BH / kv_group, Nk, d); v, dv (BH / kv_group, Nk, d_v); o, do_ (BH, Nq, d_v);
 *   lse, dlse (BH, Nq).  Packed: q (total_q, heads_q, d) at q_stride, k (total_k, heads_kv, d) at k_stride, v (total_k, heads_kv, d_v)
 *   at v_stride >= heads_kv * d_v; o, do_ dense (total_q, heads_q, d_v); dq dense (total_q, heads_q, d); dk dense (total_k, heads_kv, d),
 *   dv dense (total_k, heads_kv, d_v); lse, dlse (heads_q, total_q).  The heads of a tensor stay adjacent at its own width.
 *   softmax_scale is the caller's (FlashAttention's default is d^-1/2 with q's width: 192^-1/2 for MLA).
 * Supported: f16 / bf16, d % 8 == 0, d_v % 8 == 0, 8 <= d_v < d <= 192, d_v <= 128, softmax_scale > 0, 16-byte aligned tensors, token
 * strides that are multiples of 8; causal (bottom-right aligned), kv_group, cu_seqlens (clamped in the kernels as in
 * fa_ex_forward_varlen: no host read, no synchronisation), lse and dlse.  Kernels of their own on the 16-bit MFMA
 * (fa_ex_mfma_vdim.hip), one instantiation at 192 + 128 into which narrower widths are zero-padded; deterministic, no atomics.
 * Refused before any other check and before any HIP call, the first broken rule in this order, each with a text of its own:
 * d_v < 0 (FA_ERR_INVALID_ARGUMENT); then FA_ERR_UNSUPPORTED for d_v > d; d or d_v not a multiple of 8; d > 192; d_v > 128; f32
 * tensors; then by name mask, block_sparse_mask, dropout_p > 0, window_size (window_left / window_right other than -1), softcap,
 * alibi_slopes, sinks; then softmax_scale <= 0.  (The paged forward, fa_ex_forward_varlen_paged*, has no d_v.)
 * Workspace of the backward: two float rows per query row as without d_v, plus for kv_group > 1 (heads_q > heads_kv) the per-query-head
 * dK / dV partials, summed per group at each tensor's own width.  fa_ex_backward_workspace_bytes_grouped(bh, kv_group, nq, nk, d, dtype)
 * and fa_ex_backward_workspace_bytes_varlen(heads_q, heads_kv, total_q, total_k, d, dtype) with q's width d answer for a d_v call as
 * they stand (the dV slab is sized like dK's): there is no query of its own. */
int fa_ex_forward_vdim(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                       int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                       double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks,
                       int64_t sink_heads, int64_t d_v, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask, int64_t br,
                       int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream);
int fa_ex_backward_vdim(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const float* dlse, int64_t d_v, const uint8_t* mask, int64_t mask_bh_stride, const uint8_t* block_mask,
                        int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace, size_t workspace_bytes,
                        void* stream);
int fa_ex_forward_varlen_vdim(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                              const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                              int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                              int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                              double softmax_scale, double softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                              const float* sinks, int64_t sink_heads, int64_t d_v, double dropout_p, uint64_t dropout_seed,
                              void* stream);
int fa_ex_backward_varlen_vdim(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq,
                               void* dk, void* dv, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch,
                               int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t total_k, int64_t max_seqlen_q,
                               int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int causal, int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                               const float* alibi_slopes, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads,
                               float* dsinks, const float* dlse, int64_t d_v, double dropout_p, uint64_t dropout_seed,
                               void* workspace, size_t workspace_bytes, void* stream);
/* --- An additive attention bias with its gradient: the float attn_mask of scaled_dot_product_attention, CK FlashAttention's bias,
 * xFormers' attn_bias, a relative-position table, a pair bias.  For query unit u = b * bias_heads + h, row i, key j
 *     s[i, j] = softmax_scale * (q_i . k_j) + bias[b, h, i, j]
 * and the softmax, o and lse are those of s; the causal flag (bottom-right aligned, Nq != Nk) applies as without a bias.  The bias
 * has q's dtype (f16 / bf16), is read as stored, widened exactly and added in fp32; it is not multiplied by the scale.  An element
 * may be -inf: that key is not visible, and a row whose visible keys are all -inf gives o = 0, lse = -inf, dq = 0.  +inf and NaN are
 * the caller's error and are not checked.  fa_ex_forward_bias / fa_ex_backward_bias take the arguments of fa_ex_forward_vdim /
 * fa_ex_backward_vdim and after d_v the group (bias, bias_heads, bias_batch_stride, bias_head_stride, bias_row_stride), the backward
 * then (dbias, dbias_batch_stride, dbias_head_stride, dbias_row_stride).  bias == NULL with the rest of the group 0 / NULL is
 * exactly the _vdim call: the same checks, the same launches, the same bits.
 *   Layout: element [b, h, i, j] at bias + b * bias_batch_stride + h * bias_head_stride + i * bias_row_stride + j (elements); a
 *   stride of 0 broadcasts that dimension and nothing is expanded in memory.  With kv_group > 1 the bias is per query head.  The
 *   last dim is contiguous, the pointer 16-byte aligned, every non-zero stride a multiple of 8, and the storage of a row extends
 *   to Nk rounded up to 8 elements (allocate the last dim padded and pass the slice); the padding may hold anything, NaN included,
 *   and reaches no result.  The library never copies a bias.
 *   dbias (NULL: none) receives dS[i, j] = P (dP - delta + dlse_i), the value the kernels round to 16 bits for their dQ / dK products
 *   (without the scale), in the bias dtype at its own strides: exactly 0 wherever the key is not visible (causal flag, dead row,
 *   -inf bias); every element [.., :Nq, :Nk] is written by the call and nothing past column Nk of a row is.  A dbias stride of 0
 *   over the batch (BH / bias_heads > 1) or the heads (bias_heads > 1) makes dbias the sum of the per-unit dS over that dimension,
 *   in fp32 in unit order, rounded once: deterministic, no atomics, through the workspace.  A dbias for a row-broadcast bias
 *   (bias_row_stride = 0 with Nq > 1) is refused.
 * Combines with causal, Nq != Nk, kv_group, softmax_scale, lse and dlse.  Kernels: the kFeatBias instantiations of the 16-bit MFMA
 * extended kernels (fa_ex_mfma_bias.hip); never the plain kernels, the dS hand-over or the exact-f32 kernels.
 * Refused before any other check and before any HIP call, the first broken rule in this order, each with a text of its own:
 * (1) bias NULL with a stride or a dbias (FA_ERR_INVALID_ARGUMENT); (2) bias or dbias not 16-byte aligned (FA_ERR_UNSUPPORTED);
 * (3) a stride that is negative or no multiple of 8 (FA_ERR_UNSUPPORTED); (4) bias_heads < 1 or not dividing BH
 * (FA_ERR_INVALID_ARGUMENT); (5) dbias for a row-broadcast bias; then FA_ERR_UNSUPPORTED by name for (6) mask (fold it into the bias
 * as -inf), block_sparse_mask, dropout_p > 0, window_size (window_left / window_right other than -1), softcap, alibi_slopes, sinks,
 * d_v != d; (7) f32 tensors; (8) d > 128 or d % 8 != 0; (9) softmax_scale <= 0; (10) a unit's rows beyond 2^31 bytes.
 * Workspace of the backward: fa_ex_backward_workspace_bytes_bias = fa_ex_backward_workspace_bytes_grouped, plus with dbias_reduced != 0
 * (a dbias that is a sum over the batch or the heads) BH * Nq * (Nk rounded up to 8) * 2 bytes of per-unit dS. */
int fa_ex_forward_bias(const void* q, const void* k, const void* v, void* o, float* lse, int64_t bh, int64_t kv_group, int64_t nq,
                       int64_t nk, int64_t d, int dtype, int causal, int64_t window_left, int64_t window_right, double softmax_scale,
                       double softcap, const float* alibi_slopes, int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks,
                       int64_t sink_heads, int64_t d_v, const void* bias, int64_t bias_heads, int64_t bias_batch_stride,
                       int64_t bias_head_stride, int64_t bias_row_stride, const uint8_t* mask, int64_t mask_bh_stride,
                       const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* stream);
int fa_ex_backward_bias(const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse, void* dq, void* dk,
                        void* dv, int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int causal,
                        int64_t window_left, int64_t window_right, double softmax_scale, double softcap, const float* alibi_slopes,
                        int64_t alibi_heads, int64_t alibi_batch_stride, const float* sinks, int64_t sink_heads, float* dsinks,
                        const float* dlse, int64_t d_v, const void* bias, int64_t bias_heads, int64_t bias_batch_stride,
                        int64_t bias_head_stride, int64_t bias_row_stride, void* dbias, int64_t dbias_batch_stride,
                        int64_t dbias_head_stride, int64_t dbias_row_stride, const uint8_t* mask, int64_t mask_bh_stride,
                        const uint8_t* block_mask, int64_t br, int64_t bc, double dropout_p, uint64_t dropout_seed, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t fa_ex_backward_workspace_bytes_bias(int64_t bh, int64_t kv_group, int64_t nq, int64_t nk, int64_t d, int dtype, int dbias_reduced);
/* --- The varlen forward over a paged K/V cache: FlashAttention-2's flash_attn_varlen_func(..., block_table=).  Chunked prefill, or
 * prefill behind a shared prefix, reads its keys straight from the pools of the KV-cache calls, without a gathered copy and on the
 * kernel that reads a sequence's keys once per 256 query rows.  Forward only, no dropout.  The arguments are those of
 * fa_ex_forward_varlen_sink without dropout_p / dropout_seed, plus the table; q, o, lse, cu_seqlens_q, the masks (causal per
 * sequence, bottom-right aligned; window), GQA, softcap, alibi_slopes and sinks (all three may be 0 / NULL) keep their meaning.
 *   k, v: pools (num_blocks, page_block_size, heads_kv, d) in q's dtype.  k_stride / v_stride are the token strides inside a page,
 *     k_page_stride / v_page_stride the page strides (elements): a view of a larger allocation is fine, K and V may differ.
 *   block_table: int32 (batch, max_blocks_per_seq), contiguous, device memory.  Key t of sequence b is at element offset
 *     block_table[b, t / ps] * page_stride + (t % ps) * token_stride + head * d + i.
 *   len_k[b] = cu_seqlens_k[b + 1] - cu_seqlens_k[b], clamped in the kernels to [0, min(max_seqlen_k, max_blocks_per_seq * ps)]:
 *     only the differences of cu_seqlens_k mean anything for a pool, and total_k is not used (pass anything).  cu_seqlens_q is
 *     clamped as in fa_ex_forward_varlen.  Nothing is read on the host: no synchronisation, and a captured call may be replayed
 *     with a changed table and changed offsets.
 *   The table is untrusted: an entry outside [0, num_blocks) never leads to an access outside the pools — the keys of that page
 *     read as zero K and zero V (they still take part in the softmax, with score 0).  Only entries j < ceil(len_k[b] / ps) of row b
 *     are read.  Page offsets are 64-bit (a pool may be larger than 4 GiB), offsets inside a page 32-bit.  Sequences may name the
 *     same pages (prefix sharing).  The pools are only read.
 * Each sequence gets the bits of fa_ex_forward_varlen* on the same tokens gathered into packed k and v (same max_seqlen_q,
 * max_seqlen_k), o and lse alike: the kernels differ only in where a K/V tile's rows come from.
 * Kernels: 16-bit MFMA for f16 / bf16, d % 8 == 0, d <= 128, every stride a multiple of 8 elements and q, k, v, o 16-byte
 * aligned; exact f32 otherwise (d <= 256).
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT), besides fa_ex_forward_varlen_sink's list: block_table null or not 4-byte
 * aligned; page_block_size not a positive multiple of 16; num_blocks or max_blocks_per_seq negative; token strides below
 * heads_kv * d; with num_blocks > 1 a page stride below (ps - 1) * token stride + heads_kv * d.  FA_ERR_UNSUPPORTED: a page above
 * 65536 tokens or spanning 2^31 bytes or more. */
int fa_ex_forward_varlen_paged(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                               const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                               int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                               int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                               double softmax_scale, double softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                               const float* sinks, int64_t sink_heads, const int32_t* block_table, int64_t max_blocks_per_seq,
                               int64_t num_blocks, int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride,
                               void* stream);
/* --- The same over an e4m3 pool: the cache that fa_ex_forward_kvcache_fp8 appends to and decodes from, read by the prefill kernel.
 * The arguments are those of fa_ex_forward_varlen_paged plus cache_dtype, k_descale, v_descale, descale_batch_stride in front of
 * stream; cache_dtype == dtype with null scales and stride 0 IS fa_ex_forward_varlen_paged, bit for bit.  With FA_DTYPE_E4M3:
 *   k, v: pools (num_blocks, page_block_size, heads_kv, d) of OCP e4m3 (float8_e4m3fn) bytes; their token and page strides are in
 *     elements, which are bytes.  q and o stay f16 / bf16 (dtype), lse fp32.
 *   A stored byte c of K head h of sequence b (the sequence of the call, not the page) stands for
 *     e4m3(c) * k_descale[b * descale_batch_stride + h], for V with v_descale: float32, device memory, read by the kernels only,
 *     (batch, heads_kv) or, at stride 0, (heads_kv,); NULL = 1.0.  The sentences of fa_ex_forward_kvcache_fp8: both calls agree on
 *     one cache.
 *   Widening e4m3 to f16 / bf16 is exact, so K and V are widened and the 16-bit kernel is kept; Q and P are not quantised.  The
 *     score is softmax_scale * k_descale[b,h] * (q . k_stored), scaled before softcap and ALiBi; v_descale[b,h] multiplies the
 *     normalised output once in fp32 before its single rounding; lse is the logsumexp of the scaled, modified scores (the sink
 *     included, untouched by the scales).
 *   Everything else is fa_ex_forward_varlen_paged's: the untrusted table (a page outside the pool reads as zero K and V, byte 0x00),
 *     no entry past ceil(len_k / ps) read, 64-bit page offsets, strided pool views, device-side clamped lengths, no host read, graph
 *     capture and replay (with changed scale values in the same scale tensors too).
 * With null scales o and lse have the bits of fa_ex_forward_varlen_paged on the pools widened to dtype; with power-of-two scales
 * those of that call at softmax_scale * k_descale, o times v_descale.
 * Kernels: 16-bit MFMA for d <= 128 (q, o 16-byte aligned, q_stride % 8 == 0; every pool this call accepts), exact f32 for
 * d <= 256.
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT), besides fa_ex_forward_varlen_paged's list: cache_dtype neither dtype nor
 * FA_DTYPE_E4M3; a scale or a non-zero descale_batch_stride with a 16-bit pool; descale_batch_stride negative, or non-zero and
 * below heads_kv; a scale not 4-byte aligned; with FA_DTYPE_E4M3: dtype not f16 / bf16, d not a multiple of 8, a pool not 8-byte
 * aligned, a pool stride not a multiple of 8.  FA_ERR_UNSUPPORTED: a page spanning 2^31 bytes or more (bytes: an e4m3 page may
 * hold twice the tokens). */
int fa_ex_forward_varlen_paged_fp8(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* cu_seqlens_q,
                                   const int32_t* cu_seqlens_k, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                                   int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_stride,
                                   int64_t k_stride, int64_t v_stride, int causal, int64_t window_left, int64_t window_right,
                                   double softmax_scale, double softcap, const float* alibi_slopes, int64_t alibi_batch_stride,
                                   const float* sinks, int64_t sink_heads, const int32_t* block_table, int64_t max_blocks_per_seq,
                                   int64_t num_blocks, int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride,
                                   int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                                   void* stream);
/* Decoding: the sink joins when the per-split partials are combined,
 *     m = max(max_s lse_s, sink)   denom = sum_s exp(lse_s - m) + exp(sink - m)   o = sum_s exp(lse_s - m) O_s / denom
 *     lse = m + log(denom)
 * so a sink call always runs the combine: where the split rule or num_splits gives one split, two are launched (the second is
 * empty on a short cache).  The workspace is fa_ex_kvcache_workspace_bytes_sink (that of max(S, 2) splits).  o is rounded to 16 bits
 * once, from fp32.  Like the other KV-cache calls it never synchronises or allocates and can be captured in a graph. */
int fa_ex_forward_kvcache_sink(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                               const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                               int64_t seqlen_q, int64_t seqlen_new, int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride,
                               int64_t q_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                               int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t k_new_batch_stride,
                               int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int causal,
                               int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                               const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, const int32_t* block_table,
                               int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                               const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                               const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                               int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                               int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                               const float* sinks, int64_t sink_heads, void* workspace, size_t workspace_bytes, void* stream);
size_t fa_ex_kvcache_workspace_bytes_sink(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                          int64_t d, int64_t num_splits);

/* --- variable-length queries and new keys in KV-cache decoding (FlashAttention-3's cu_seqlens_q / cu_seqlens_k_new) ---
 * fa_ex_forward_kvcache_sink plus five arguments between sink_heads and workspace.  All null / 0: exactly that call.
 * cu_seqlens_q (int32 (batch + 1,), device): q is packed (total_q, heads_q, d) at q_token_stride, sequence b owns tokens
 * [cu_seqlens_q[b], cu_seqlens_q[b + 1]) (none allowed), at most max_seqlen_q of them; o is (total_q, heads_q, d) dense and lse
 * (heads_q, total_q), the packed convention of the varlen calls.  seqlen_q and q_batch_stride are not used.
 * cu_seqlens_k_new (int32 (batch + 1,), device; only with k_new, v_new and cu_seqlens_q): k_new, v_new are packed
 * (total_k_new, heads_kv, d) and sequence b appends its nnew_b tokens (none allowed); seqlen_new and the k_new / v_new batch
 * strides are not used.  cu_seqlens_q may also go with padded (batch, seqlen_new, ..) k_new, v_new, or with none.
 * Every sequence gets what the padded call returns for it alone (batch = 1, its own q tokens, new keys, cache row, table row,
 * leftpad, descale row, ALiBi row): L_b = clamp(cache_seqlens[b], 0, capacity - nnew_b), len_k = L_b + nnew_b - P_b, causal
 * diagonal len_k - nq_b, rotary positions L_b - P_b + n (new key n) and L_b - P_b + i or L_b - P_b (q token i).  A sequence
 * without q tokens writes nothing to o / lse and still appends; rows of o / lse that no sequence owns are not written.
 * Both arrays are untrusted, as cache_seqlens is: start_b = clamp(cu[b], 0, total) and n_b = clamp(cu[b + 1] - cu[b], 0,
 * min(bound, total - start_b)) with bound = max_seqlen_q (q) or the capacity (k_new), so no content reads outside q / k_new /
 * v_new or writes outside o, lse, the workspace or the cache; overlapping ranges give unspecified values in the rows they share.
 * num_splits = 0 takes ceil(max_seqlen_q * (heads_q / heads_kv) / 16) for the row tiles of the split rule; rotary needs
 * seqlen_ro >= capacity + max_seqlen_q; a window bound is canonicalised against max_seqlen_q.  The workspace is
 * fa_ex_kvcache_workspace_bytes_varlen: S * total_q * heads_q * (d + 1) floats for S > 1 splits (with_sinks: at least two), each
 * of the two parts rounded up to 256 bytes.  Refused before any HIP call: total_q, max_seqlen_q or total_k_new non-zero without
 * their array; cu_seqlens_k_new without k_new / v_new or without cu_seqlens_q; max_seqlen_q < 0 or > total_q; total_q or
 * total_k_new at or past 2^31; max_seqlen_q tokens of q spanning 2^31 bytes or more (FA_ERR_UNSUPPORTED: the kernels keep 32-bit
 * offsets inside one sequence and 64-bit ones between sequences).  Never synchronises or allocates; can be captured in a graph and
 * replayed after the contents of the arrays changed (total_q, max_seqlen_q and total_k_new are fixed by the capture). */
int fa_ex_forward_kvcache_varlen(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                                 const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                                 int64_t seqlen_q, int64_t seqlen_new, int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride,
                                 int64_t q_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                                 int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t k_new_batch_stride,
                                 int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int causal,
                                 int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                                 const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, const int32_t* block_table,
                                 int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                                 const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                                 const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                                 int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                                 int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                                 const float* sinks, int64_t sink_heads, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k_new,
                                 int64_t total_q, int64_t max_seqlen_q, int64_t total_k_new, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t fa_ex_kvcache_workspace_bytes_varlen(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q,
                                            int64_t cache_len, int64_t d, int64_t num_splits, int with_sinks);

/* --- a second query operand and K, V of different widths in KV-cache decoding (FlashAttention-3's qv): multi-head latent
 * attention (MLA) at decode time.  fa_ex_forward_kvcache_varlen plus four arguments between total_k_new and workspace.  All null /
 * 0: exactly that call.  With qv (device, q's dtype, (batch, seqlen_q, heads_q, d_v) at qv_batch_stride / qv_token_stride elements,
 * heads adjacent at stride d_v, 16-byte aligned, strides multiples of 8) v_cache is (.., heads_kv, d_v) — a contiguous cache or a
 * pool, addressed with its own batch / page and token strides, so k_cache and v_cache may be the two column ranges of one
 * (.., d + d_v) allocation — o is (batch, seqlen_q, heads_q, d_v) dense, and for query head h reading K/V head h / G
 *     s[i, j] = softmax_scale * (q[i, h, :] . k[j, :] + qv[i, h, :] . v[j, :]),   o[i, h, :] = sum_j softmax_j(s)[i, j] * v[j, :]
 * (callers following FlashAttention-3 pass softmax_scale = (d + d_v)^-1/2).  Each row of v_cache is read from memory once and
 * serves as the score operand and as the value operand.  cache_seqlens, block_table (untrusted; a page outside the pool reads as
 * a zero key with a zero value), cache_batch_idx, causal, the window, num_splits, graph capture and the o = 0 / lse = -inf of a row
 * without a visible key are as without qv.  Supported: d = 64 with d_v = 512; any other pair is FA_ERR_UNSUPPORTED, with both
 * numbers in the text.  Not supported with qv, each FA_ERR_UNSUPPORTED with the argument's name before any HIP call: k_new / v_new
 * (seqlen_new > 0), cu_seqlens_k_new, rotary_cos / rotary_sin, an e4m3 cache (cache_dtype, k_descale, v_descale), softcap,
 * alibi_slopes, sinks, cu_seqlens_q, cache_leftpad.  (The checks every entry point of the family shares come first, in their
 * order and with their texts: rotary tables without new tokens, for one, are refused there as FA_ERR_INVALID_ARGUMENT.)
 * qv_batch_stride, qv_token_stride and d_v must be 0 without qv.
 * The workspace is fa_ex_kvcache_workspace_bytes_qv: fa_ex_kvcache_workspace_bytes_varlen plus d_v (0: that query; pass total_q =
 * batch * seqlen_q and max_seqlen_q = seqlen_q for the padded call): S * total_q * heads_q * (d_v + 1) floats for S > 1 splits, each
 * part rounded up to 256 bytes, with S from this kernel's own launch rule when num_splits = 0. */
int fa_ex_forward_kvcache_qv(const void* q, void* k_cache, void* v_cache, const void* k_new, const void* v_new,
                             const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                             int64_t seqlen_q, int64_t seqlen_new, int64_t cache_len, int64_t d, int dtype, int64_t q_batch_stride,
                             int64_t q_token_stride, int64_t k_cache_batch_stride, int64_t k_cache_token_stride,
                             int64_t v_cache_batch_stride, int64_t v_cache_token_stride, int64_t k_new_batch_stride,
                             int64_t k_new_token_stride, int64_t v_new_batch_stride, int64_t v_new_token_stride, int causal,
                             int64_t window_left, int64_t window_right, double softmax_scale, double softcap,
                             const float* alibi_slopes, int64_t alibi_batch_stride, int64_t num_splits, const int32_t* block_table,
                             int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                             const int32_t* cache_batch_idx, int64_t cache_batch, const int32_t* cache_leftpad,
                             const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                             int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                             int cache_dtype, const float* k_descale, const float* v_descale, int64_t descale_batch_stride,
                             const float* sinks, int64_t sink_heads, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k_new,
                             int64_t total_q, int64_t max_seqlen_q, int64_t total_k_new, const void* qv, int64_t qv_batch_stride,
                             int64_t qv_token_stride, int64_t d_v, void* workspace, size_t workspace_bytes,
                             void* stream);
size_t fa_ex_kvcache_workspace_bytes_qv(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q,
                                        int64_t cache_len, int64_t d, int64_t num_splits, int with_sinks, int64_t d_v);

/* --- Sparse MLA decoding: fa_ex_forward_kvcache_qv over a per-query list of cached tokens (DeepSeek sparse attention: an indexer
 * picks, for every query token, the topk cached tokens it may attend to).  A call family of its own; the caches, cache_seqlens,
 * block_table and cache_batch_idx are those of the dense qv call and mean the same.  q (batch, seqlen_q, heads_q, 64) and qv
 * (batch, seqlen_q, heads_q, 512) at their batch / token strides, heads adjacent; k_cache (.., heads_kv, 64) and v_cache
 * (.., heads_kv, 512) contiguous caches (batch or cache_batch rows of cache_len tokens) or pools (num_blocks pages of
 * page_block_size tokens; cache_len is then not used, the capacity is max_blocks_per_seq * page_block_size), each with its own
 * batch / page and token strides; o (batch, seqlen_q, heads_q, 512) dense, lse (batch, heads_q, seqlen_q) float32.
 * indices: int32 device memory, entry j < topk of (sequence b, query token i, K/V head hk) at
 *     indices[b * indices_batch_stride + i * indices_token_stride + hk * indices_head_stride + j]
 * (indices_head_stride = 0: one list for all K/V heads of a token).  For query head h reading K/V head hk = h / G, list I and
 * len_b = clamp(cache_seqlens[b], 0, capacity) (null: the capacity):
 *     visible(j)  <=>  0 <= I[j] < len_b  and, if causal,  I[j] <= len_b - seqlen_q + i
 *     s[j] = softmax_scale * (q[b, i, h, :] . k[I[j], hk, :] + qv[b, i, h, :] . v[I[j], hk, :])   over the visible j
 *     o[b, i, h, :] = sum_j softmax_j(s)[j] * v[I[j], hk, :],     lse[b, h, i] = logsumexp_j s[j]
 * An index is a logical token position of sequence b, resolved as the dense call resolves a position: token I of cache row
 * (cache_batch_idx ? cache_batch_idx[b] : b), or slot I % page_block_size of page block_table[b, I / page_block_size].  Every list
 * position is a key: a token named twice counts twice; the order of a list changes the result by rounding only.  An entry that is
 * not visible (-1 padding, anything negative or >= len_b, above the causal bound) is no key and never becomes an address: the
 * indices are untrusted and are not read on the host.  A visible entry whose page lies outside [0, num_blocks), or whose cache
 * row lies outside [0, cache_batch), is a zero key with a zero value and score 0 that takes part in the softmax (the dense call's
 * rule).  A row without a visible entry (topk = 0 included) gives o = 0, lse = -inf.  No window, softcap, ALiBi, sinks, rotary, new
 * tokens, e4m3 cache, packed queries or left padding.
 * Split-KV over the list positions: num_splits in [1, 256], or 0 for the launch rule; the partials are combined in a fixed order
 * (the same bits on every run).  workspace: fa_mla_sparse_workspace_bytes (0 for one split; 0 too for arguments the call would
 * reject): S * batch * seqlen_q * heads_q * (512 + 1) floats, each part rounded up to 256 bytes.  Nothing allocates, synchronises
 * or reads device memory on the host: the call can be captured and replayed with changed indices, lengths and tables.
 * Checked before any HIP call, the first broken rule named in fa_last_error(), in this order: batch, seqlen_q, heads_q >= 0, and a
 * call with one of them 0 returns FA_OK without a launch and without looking at anything else; (1) q, qv, k_cache, v_cache, o, lse
 * (and indices unless topk = 0) non-null; (2) d = 64 and d_v = 512, else FA_ERR_UNSUPPORTED with both numbers in the text; (3) dtype
 * f16 or bf16, then heads_q a multiple of heads_kv >= 1, softmax_scale finite and > 0, num_splits in [0, 256], cache_len >= 1
 * without block_table, cache_batch in [1, 2^31) with cache_batch_idx (which does not go with block_table) and 0 without, and
 * (FA_ERR_UNSUPPORTED) heads_q <= 65535, cache_len <= 2^28, seqlen_q <= 2^24, batch * seqlen_q * heads_q < 2^31; (4) for q, qv,
 * k_cache, v_cache token strides >= heads * width, with more than one batch element (page, cache row) batch strides >= (tokens - 1)
 * * token stride + heads * width, strides multiples of 8, one batch element below 2^31 bytes (FA_ERR_UNSUPPORTED), q, qv, k_cache,
 * v_cache, o 16-byte and lse, indices, cache_seqlens, block_table, cache_batch_idx 4-byte aligned; (5) topk in [0, 2^30],
 * indices_head_stride 0 or >= topk, with seqlen_q > 1 indices_token_stride >= a token's lists, with batch > 1
 * indices_batch_stride >= a sequence's lists, none negative; (6) with block_table page_block_size a positive multiple of 16,
 * num_blocks in [1, 2^31), max_blocks_per_seq >= 1 with a capacity <= 2^28 tokens (FA_ERR_UNSUPPORTED),
 * block_table_row_stride >= max_blocks_per_seq, and without it all four 0; (7) with S > 1 fewer than 2^26 rows
 * (FA_ERR_UNSUPPORTED), workspace_bytes >= the need, workspace non-null and 16-byte aligned. */
int fa_mla_sparse_forward(const void* q, const void* qv, const void* k_cache, const void* v_cache, const int32_t* indices,
                          const int32_t* cache_seqlens, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                          int64_t seqlen_q, int64_t cache_len, int64_t topk, int64_t d, int64_t d_v, int dtype,
                          int64_t q_batch_stride, int64_t q_token_stride, int64_t qv_batch_stride, int64_t qv_token_stride,
                          int64_t k_cache_batch_stride, int64_t k_cache_token_stride, int64_t v_cache_batch_stride,
                          int64_t v_cache_token_stride, int64_t indices_batch_stride, int64_t indices_token_stride,
                          int64_t indices_head_stride, int causal, double softmax_scale, int64_t num_splits,
                          const int32_t* block_table, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                          int64_t max_blocks_per_seq, const int32_t* cache_batch_idx, int64_t cache_batch, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t fa_mla_sparse_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t topk,
                                     int64_t num_splits);

/* --- MLA decoding from a packed 8-bit latent cache (FlashMLA's fp8 KV cache), and the append into it.  A call family of its own:
 * fa_ex_forward_kvcache_qv and fa_mla_sparse_forward keep refusing an e4m3 cache and new tokens.  A cached token is 656 bytes:
 *     byte   0 .. 511   512 e4m3 (OCP, torch.float8_e4m3fn)   the latent, quantised per 128-wide tile
 *     byte 512 .. 527   4 float32                             one scale per tile
 *     byte 528 .. 655   64 bf16                               the rotary part, not quantised
 * kv_cache is a paged pool of such tokens, one K/V head: slot s of page p starts at kv_cache + p * page_stride_bytes + s *
 * token_stride_bytes (64-bit arithmetic); token t of sequence b is slot t % page_block_size of page block_table[b, t /
 * page_block_size].  A contiguous (B, cap, 656) cache with cap a multiple of 16 is a pool of B pages of cap tokens.
 * Read contract: latent element i of a token is  bf16_rne(float(e4m3[i]) * scale[i / 128])  — one exact widening, one fp32
 * multiply, one rounding to nearest even — and the 64 rotary values are taken as they are.  fa_mla_fp8_forward on a pool is, to
 * the bit, the 16-bit call on these values with the same table, lengths and num_splits: fa_ex_forward_kvcache_qv (q against the
 * rotary part as k_cache, qv against the latent as v_cache, paged) when indices is null, fa_mla_sparse_forward with one list a
 * query token (indices_head_stride 0) when it is not; indices, topk, visibility, causal, cache_seqlens (untrusted, clamped to the
 * capacity max_blocks_per_seq * page_block_size; null: the capacity), a page outside [0, num_blocks) (a zero key with a zero
 * value), the o = 0 / lse = -inf of a row without a key, num_splits, the launch rule and the combine are those calls'.  q
 * (batch, seqlen_q, heads_q, 64) and qv (batch, seqlen_q, heads_q, 512) bf16 at their batch / token / head strides (elements) —
 * the two column ranges of one (.., 576) tensor, say, heads 576 apart; o (batch, seqlen_q, heads_q, 512) bf16 dense, lse (batch, heads_q,
 * seqlen_q) float32.  bf16 only, heads_kv = 1, paged only; no window.  Scales that are not finite are outside the contract
 * (nothing is read or written out of bounds).  workspace: fa_mla_fp8_workspace_bytes (cache_len: the capacity; with_indices != 0
 * for a call with indices, else topk must be 0), which equals fa_ex_kvcache_workspace_bytes_qv / fa_mla_sparse_workspace_bytes of
 * the same shape.  Nothing allocates, synchronises or reads device memory on the host: the calls can be captured in a graph.
 * fa_mla_fp8_forward checks before any HIP call, the first broken rule named in fa_last_error(), in this order: batch, seqlen_q,
 * heads_q >= 0, and a call with one of them 0 returns FA_OK without a launch and without looking at anything else; (1) q, qv,
 * kv_cache, o, lse non-null; (2) d = 64 and d_v = 512, else FA_ERR_UNSUPPORTED with both numbers in the text; (3) dtype bf16
 * (f16: FA_ERR_UNSUPPORTED by name; any other code FA_ERR_INVALID_ARGUMENT), heads_kv = 1 (FA_ERR_UNSUPPORTED), block_table
 * non-null, softmax_scale finite and > 0, num_splits in [0, 256], and (FA_ERR_UNSUPPORTED) heads_q <= 65535, seqlen_q <= 2^24,
 * batch * seqlen_q * heads_q < 2^31, without indices batch <= 65535 and at most 65535 tiles of 16 rows; (4) for q and qv head
 * strides in [width, 2^20], token strides >= (heads_q - 1) * head stride + width, with batch > 1 batch strides >= (seqlen_q - 1)
 * * token stride + a token's heads, strides multiples of 8, one batch element below 2^31 bytes (FA_ERR_UNSUPPORTED);
 * token_stride_bytes >= 656 and a multiple of 16 (below 2^31: FA_ERR_UNSUPPORTED); page_stride_bytes >= (page_block_size - 1) *
 * token_stride_bytes + 656 and a multiple of 16; kv_cache 16-byte aligned; q, qv, o 16-byte and lse, indices, cache_seqlens,
 * block_table 4-byte aligned; (5) with indices topk in [0, 2^30], with seqlen_q > 1 indices_token_stride >= topk, with batch > 1
 * indices_batch_stride >= a sequence's lists, none negative; without indices all three 0; (6) page_block_size a positive multiple
 * of 16, num_blocks in [1, 2^31), max_blocks_per_seq >= 1 with a capacity <= 2^28 tokens (FA_ERR_UNSUPPORTED),
 * block_table_row_stride >= max_blocks_per_seq; (7) with S > 1 fewer than 2^26 rows (FA_ERR_UNSUPPORTED), workspace_bytes >= the
 * need, workspace non-null and 16-byte aligned.
 * fa_mla_fp8_pack quantises and appends: latent_new (batch, seqlen_new, 512) and rope_new (batch, seqlen_new, 64) bf16 at their
 * batch / token strides (elements; the two column ranges of one (.., 576) tensor, say; rotate the rope part first, with
 * fa_rotary_apply); token i of sequence b goes to position cache_seqlens[b] + i (cache_seqlens: the lengths before the append,
 * required, not modified) through block_table.  Per 128-wide tile, in fp32 from the exact bf16 values:
 *     amax = max |x|;   scale = amax > 0 ? amax / 448 : 1   (scale_pow2 != 0: rounded up to the next power of two);
 *     byte = e4m3_rne(clamp(x / scale, -448, 448))
 * with both divisions IEEE-rounded; the rotary 128 bytes are copied.  (The power of two is exact for every normal scale; a
 * subnormal scale, or one in the top binade — amax below 448 * 2^-126 or above 448 * 2^127 — is outside the contract.)  Both device arrays are untrusted: a negative length, a
 * position at or beyond max_blocks_per_seq * page_block_size, or a page outside [0, num_blocks) drops that token, and nothing of
 * it is written; bytes of a token's stride past its 656 are never written.  Two tokens mapped to one slot: undefined.  A tile
 * with a NaN or an infinity is outside the contract (nothing is written out of bounds).  Checked before any HIP call, in this
 * order: batch, seqlen_new >= 0 (one of them 0: FA_OK, no launch); the five pointers non-null; batch * seqlen_new < 2^31; token
 * strides >= 512 / 64, with batch > 1 batch strides >= (seqlen_new - 1) * token stride + width, multiples of 8; the rules of
 * token_stride_bytes, page_stride_bytes and kv_cache above; latent_new, rope_new 16-byte, cache_seqlens, block_table 4-byte
 * aligned; the page geometry (6). */
int fa_mla_fp8_forward(const void* q, const void* qv, const void* kv_cache, const int32_t* indices, const int32_t* cache_seqlens,
                       const int32_t* block_table, void* o, float* lse, int64_t batch, int64_t heads_q, int64_t heads_kv,
                       int64_t seqlen_q, int64_t topk, int64_t d, int64_t d_v, int dtype, int64_t q_batch_stride,
                       int64_t q_token_stride, int64_t q_head_stride, int64_t qv_batch_stride, int64_t qv_token_stride,
                       int64_t qv_head_stride, int64_t page_stride_bytes, int64_t token_stride_bytes,
                       int64_t indices_batch_stride, int64_t indices_token_stride,
                       int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                       int causal, double softmax_scale, int64_t num_splits, void* workspace, size_t workspace_bytes, void* stream);
size_t fa_mla_fp8_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                  int64_t topk, int with_indices, int64_t num_splits);
int fa_mla_fp8_pack(const void* latent_new, const void* rope_new, void* kv_cache, const int32_t* cache_seqlens,
                    const int32_t* block_table, int64_t batch, int64_t seqlen_new, int64_t latent_batch_stride,
                    int64_t latent_token_stride, int64_t rope_batch_stride, int64_t rope_token_stride, int64_t page_stride_bytes,
                    int64_t token_stride_bytes, int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size,
                    int64_t max_blocks_per_seq, int scale_pow2, void* stream);

/* --- The lightning indexer (DeepSeek-V3.2): the step that makes the token lists fa_mla_sparse_forward and fa_mla_fp8_forward take as
 * `indices`.  A call family of its own; three launches, each usable alone.  For query token i and cached token j of sequence b
 *     I[b, i, j] = sum_h  w[b, i, h] * max(0, q[b, i, h] . k8[j]) * k_scale[j]
 * over `heads` = 32 or 64 index heads, 128 wide, and per token the topk largest I among the tokens it sees.
 * The index-key cache is a paged pool, one key a token.  A cached token is 132 bytes:
 *     byte   0 .. 127   128 e4m3 (OCP, torch.float8_e4m3fn)   the index key, quantised as one 128-wide tile
 *     byte 128 .. 131   1 float32                             its scale
 * slot s of page p starts at k_cache + p * page_stride_bytes + s * token_stride_bytes (64-bit arithmetic); token_stride_bytes >= 132
 * and a multiple of 16 (144: the dense form); bytes of a token's stride past its 132 are never written and never read.
 * block_table, cache_seqlens, num_blocks, page_block_size, max_blocks_per_seq and block_table_row_stride mean what they mean for
 * fa_mla_fp8_forward (the same table serves both pools); cache_seqlens is required.  Paged only: a contiguous cache is an identity
 * table.  Both device arrays are untrusted: a length is clamped on the device to [0, min(max_blocks_per_seq * page_block_size,
 * width)] (fa_indexer_topk, which takes no table: [0, width]); no table entry past ceil(len / page_block_size) is read; a page
 * outside [0, num_blocks) is not fetched.  Nothing allocates, synchronises or reads device memory on the host: every call can be
 * captured in a graph and replayed after lengths, table, cache bytes and weights changed in place.  No workspace.
 * Visibility (fa_mla_sparse_forward's rule): key j is visible to token i of sequence b iff 0 <= j < len_b and, with causal != 0,
 * j <= len_b - seqlen_q + i; len_b counts the seqlen_q new tokens.
 *
 * fa_indexer_pack quantises and appends: k_new (batch, seqlen_new, 128) bf16 at its batch / token strides (elements); token i of
 * sequence b goes to position cache_seqlens[b] + i (the lengths before the append; not modified) through block_table.
 * fa_mla_fp8_pack's rule on the one tile, in fp32 from the exact bf16 values:
 *     amax = max |x|;   scale = amax > 0 ? amax / 448 : 1   (scale_pow2 != 0: rounded up to the next power of two);
 *     byte = e4m3_rne(clamp(x / scale, -448, 448))
 * with both divisions IEEE-rounded, and the same things outside the contract (a NaN or an infinity in the tile, a subnormal scale,
 * one in the top binade).  A negative length, a position at or beyond max_blocks_per_seq * page_block_size, or a page outside
 * [0, num_blocks) drops that token and nothing of it is written.  Two tokens mapped to one slot: undefined.  Checked before any HIP
 * call, the first broken rule named in fa_last_error(), in this order: batch, seqlen_new >= 0 (one of them 0: FA_OK, no launch);
 * (1) the four pointers non-null; (2) d = 128 (FA_ERR_UNSUPPORTED, with the number), batch * seqlen_new < 2^31 (FA_ERR_UNSUPPORTED);
 * (3) token stride >= 128, with batch > 1 batch stride >= (seqlen_new - 1) * token stride + 128, multiples of 8, at most 2^31 / 2^44
 * (FA_ERR_UNSUPPORTED); token_stride_bytes >= 132 and a multiple of 16 (below 2^31: FA_ERR_UNSUPPORTED); page_stride_bytes >=
 * (page_block_size - 1) * token_stride_bytes + 132 and a multiple of 16; k_cache 16-byte aligned; k_new 16-byte, cache_seqlens and
 * block_table 4-byte aligned; (4) the page geometry: page_block_size a positive multiple of 16, num_blocks in [1, 2^31),
 * max_blocks_per_seq >= 1 with a capacity <= 2^28 tokens (FA_ERR_UNSUPPORTED), block_table_row_stride >= max_blocks_per_seq.
 *
 * fa_indexer_logits: q (batch, seqlen_q, heads, 128) e4m3 bytes at its batch / token / head strides (bytes = elements); weights
 * (batch, seqlen_q, heads) float32 at its batch / token strides (elements) -- the caller folds the query's own quantisation scale and
 * the heads^-1/2 * d^-1/2 factors into it; there is no scale argument.  logits (batch, seqlen_q, width) float32 at 64-bit batch / row
 * strides (elements); batch * seqlen_q * width may exceed 2^31.  For a visible key the value above is written: the dot products on
 * v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales (two instructions a product), ReLU, weight and head sum in fp32 in the order
 * csrc/fa_indexer.hip and tests/indexer_ref.py document, k_scale applied once after the head sum.  A visible key on a page outside
 * the pool reads as a zero row with scale 0: its logit is 0, and it takes part in the selection.  ENTRIES THAT ARE NOT VISIBLE ARE
 * NOT WRITTEN: the row keeps its bytes there, and fa_indexer_topk never reads them.  e4m3 NaN codes in a visible q or key propagate.
 * Checked in this order: batch, seqlen_q >= 0 (one of them 0: FA_OK, no launch); (1) the six pointers non-null; (2) d = 128, then
 * heads 32 or 64 (each FA_ERR_UNSUPPORTED, with the number); (3) width in [1, 2^28]; batch <= 65535 and seqlen_q <= 2^22
 * (FA_ERR_UNSUPPORTED); (4) q: head stride in [128, 2^20], token stride >= (heads - 1) * head stride + 128, with batch > 1 batch
 * stride >= (seqlen_q - 1) * token stride + a token's heads, multiples of 16, at most 2^31 / 2^44 (FA_ERR_UNSUPPORTED); weights: token
 * stride >= heads, with batch > 1 batch stride >= a sequence's rows; logits: with seqlen_q > 1 row stride >= width, with batch > 1
 * batch stride >= (seqlen_q - 1) * row stride + width, none negative, each <= 2^44, 4-byte aligned; the rules of token_stride_bytes,
 * page_stride_bytes and k_cache above; q 16-byte, weights, cache_seqlens and block_table 4-byte aligned; (5) the page geometry.
 *
 * fa_indexer_topk: logits as above, from any source.  Per row (b, i) with n visible keys (the positions 0 .. n - 1):
 *     key(x) = bits(x) ^ (sign(x) ? 0xFFFFFFFF : 0x80000000), compared as unsigned: a total order on bit patterns (-0 < +0, a positive
 *     NaN above +inf, -inf an ordinary small value);
 *     selected: the min(topk, n) visible positions largest by (key descending, position ascending): among equal keys the lowest
 *     positions win;
 *     indices[b, i, :]: the selected positions in ASCENDING position order, then -1 in the remaining topk - min(topk, n) entries.
 * A pure function of the logits' bits.  With n <= topk the row is 0 .. n - 1 and padding and the logits are not read.  indices
 * (batch, seqlen_q, topk) int32 at its batch / token strides (elements), the list fa_mla_sparse_forward (indices_head_stride 0) and
 * fa_mla_fp8_forward take.  Checked in this order: batch, seqlen_q >= 0 (one of them 0: FA_OK, no launch); (1) the three pointers
 * non-null; (2) topk in [1, 2^20]; width >= 1, and <= 2^28 (FA_ERR_UNSUPPORTED); batch <= 65535, seqlen_q < 2^31 (FA_ERR_UNSUPPORTED);
 * (3) the rules of logits above; with seqlen_q > 1 indices_token_stride >= topk, with batch > 1 indices_batch_stride >= a sequence's
 * lists, none negative, each <= 2^40; indices and cache_seqlens 4-byte aligned. */
int fa_indexer_pack(const void* k_new, void* k_cache, const int32_t* cache_seqlens, const int32_t* block_table, int64_t batch,
                    int64_t seqlen_new, int64_t d, int64_t k_new_batch_stride, int64_t k_new_token_stride,
                    int64_t page_stride_bytes, int64_t token_stride_bytes, int64_t block_table_row_stride, int64_t num_blocks,
                    int64_t page_block_size, int64_t max_blocks_per_seq, int scale_pow2, void* stream);
int fa_indexer_logits(const void* q, const float* weights, const void* k_cache, const int32_t* cache_seqlens,
                      const int32_t* block_table, float* logits, int64_t batch, int64_t seqlen_q, int64_t heads, int64_t d,
                      int64_t width, int64_t q_batch_stride, int64_t q_token_stride, int64_t q_head_stride,
                      int64_t weights_batch_stride, int64_t weights_token_stride, int64_t logits_batch_stride,
                      int64_t logits_row_stride, int64_t page_stride_bytes, int64_t token_stride_bytes,
                      int64_t block_table_row_stride, int64_t num_blocks, int64_t page_block_size, int64_t max_blocks_per_seq,
                      int causal, void* stream);
int fa_indexer_topk(const float* logits, const int32_t* cache_seqlens, int32_t* indices, int64_t batch, int64_t seqlen_q,
                    int64_t width, int64_t topk, int64_t logits_batch_stride, int64_t logits_row_stride,
                    int64_t indices_batch_stride, int64_t indices_token_stride, int causal, void* stream);

/* --- Rotary position embedding for training and prefill (FlashAttention's flash_attn.layers.rotary: apply_rotary_emb,
 * apply_rotary_emb_qkv_), forward and backward.  One memory-bound launch on `stream` rotates the first rotary_dim head dims of
 * every head of one 16-bit tensor: x -> y, both (batch, seqlen, heads, d) with the heads adjacent at stride d, the last dim
 * contiguous, and a batch stride and a token stride each (elements).  So qkv[:, :, :2] of a (B, S, 3, H, d) projection is one call
 * with heads = 2 H at token stride 3 H d, and the first H_q + H_kv heads of a GQA-packed (B, S, H_q + 2 H_kv, d) tensor likewise.
 * y == x (the same pointer, with the same strides) is the in-place form; any other overlap of x and y is undefined.  Head dims at
 * and past rotary_dim are copied out of place and neither read nor written in place.
 * Tables and arithmetic are fa_ex_forward_kvcache_rotary's, to the bit: rotary_cos, rotary_sin (seqlen_ro, rotary_dim / 2) in x's
 * dtype, last dim contiguous, rows at the even strides rotary_cos_row_stride / rotary_sin_row_stride, 4-byte aligned; rotary_dim
 * a multiple of 16 in [16, d]; rotary_interleaved != 0 pairs elements (2j, 2j + 1) (GPT-J), 0 pairs (j, j + rotary_dim / 2)
 * (GPT-NeoX); a pair (x, y) with table entry j at table row pos becomes
 *     x' = x cos[pos, j] - y sin[pos, j],   y' = x sin[pos, j] + y cos[pos, j],
 * in fp32 from the 16-bit inputs (the products are exact), rounded once to nearest even.  A key rotated here at position p has
 * the bits the decode call stores for the same k_new at position p.
 * conjugate != 0 rotates by -sin: x' = x cos + y sin, y' = -x sin + y cos.  That is the transpose of the forward map, so applied
 * to the gradient of y it is the whole backward; the sign flip is exact.
 * Positions: token i of sequence b is at pos = seqlen_offset + (seqlen_offsets ? seqlen_offsets[b] : 0) + i.  seqlen_offset is a
 * host integer; seqlen_offsets is int32 (batch,) device memory, never read on the host and not trusted: pos is formed in 64 bits,
 * and a token is rotated iff 0 <= pos < seqlen_ro.  Every other token passes through unrotated (copied out of place, untouched
 * in place), FlashAttention's rule, where rows past the table read cos = 1, sin = 0; no table row outside the table is addressed
 * whatever the offsets hold.  (fa_ex_forward_kvcache_rotary bounds seqlen_ro on the host instead.)
 * Packed form: cu_seqlens int32 (batch + 1,) device memory; x and y are (total, heads, d) at their token strides, seqlen is 0
 * and the batch strides are not used.  Sequence b owns the tokens of fa_ex_forward_varlen's clamp: start = clamp(cu[b], 0, total),
 * end = clamp(cu[b + 1], start, total), len = min(end - start, max_seqlen); positions count from the sequence's own first token.
 * Tokens that no sequence owns are not written out of place and unchanged in place; nothing outside x / y is touched whatever
 * cu_seqlens holds.
 * Nothing allocates, synchronises or reads device memory on the host: the call can be captured in a graph and replayed with
 * changed offsets and changed cu_seqlens (batch, total, max_seqlen and seqlen_offset are fixed by the capture).  fp32 tensors
 * and separate tables for K are not supported.
 * Checked before any HIP call (FA_ERR_INVALID_ARGUMENT, the first broken rule named in fa_last_error()), in this order: dtype f16
 * or bf16; d a multiple of 8 in [8, 256]; batch in [1, 65535]; heads >= 1 (heads * d < 2^31); seqlen in [0, 2^31); x, y non-null
 * and 16-byte aligned; seqlen_offsets, cu_seqlens 4-byte aligned; with cu_seqlens 0 <= max_seqlen <= total < 2^31 and
 * seqlen == 0, without it total == max_seqlen == 0; token strides >= heads * d (and <= 2^31); with batch > 1 in the padded form
 * batch strides >= (seqlen - 1) * token stride + heads * d (and <= 2^44); every stride used a multiple of 8; y == x only with
 * equal strides; both tables given and 4-byte aligned; rotary_dim a multiple of 16 in [16, d]; row strides >= rotary_dim / 2 (and
 * <= 2^31) and even; seqlen_ro in [1, 2^31); |seqlen_offset| < 2^31.  A call with no tokens (seqlen == 0, or max_seqlen == 0)
 * that passes them returns FA_OK without a launch. */
int fa_rotary_apply(const void* x, void* y, int64_t batch, int64_t seqlen, int64_t heads, int64_t d, int dtype,
                    int64_t x_batch_stride, int64_t x_token_stride, int64_t y_batch_stride, int64_t y_token_stride,
                    const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                    int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved, int conjugate, int64_t seqlen_offset,
                    const int32_t* seqlen_offsets, const int32_t* cu_seqlens, int64_t total, int64_t max_seqlen, void* stream);

/* --- Merge of two partial attention results (merge_attn_states of the serving stacks; the update step of ring attention).
 * (o_a, lse_a) and (o_b, lse_b) are attention of the same queries over two DISJOINT key sets, each with its natural-log lse as the
 * calls above return it.  Then attention over the union is
 *     lse = logaddexp(lse_a, lse_b),    w_x = exp(lse_x - lse),    o = w_a * o_a + w_b * o_b.
 * The weights are formed around the larger lse, once per row, in fp64; each element's w_a o_a + w_b o_b is formed in fp64 (the
 * products are exact there) and rounded to fp32 and then to the tensor dtype, to nearest even.  A side with w_x = 0 (lse_x = -inf, or
 * lse_x so far below the other that exp underflows) is not used: its o_x may hold NaN or garbage, and the result is the other side's
 * o with its own bits.  Both -inf (a row without a visible key on either side): o = 0 and lse = -inf, the convention of the calls
 * above.  NaN or +inf in an lse is undefined.
 * Every tensor is addressed by (batch, head, row) through its own stride triple in elements: element e of row (b, h, i) of o_a is
 * o_a[b * o_a_batch_stride + h * o_a_head_stride + i * o_a_row_stride + e], the d elements of a row contiguous; lse_a[b *
 * lse_a_batch_stride + h * lse_a_head_stride + i * lse_a_row_stride] is that row's lse.  So (B, H, N, d) with lse (B, H, N), the
 * decode call's (B, N, H, d) with lse (B, H, N), and packed (T, H, d) with lse (H, T) (batch = 1, rows = T) are all one call
 * without a copy, and so is a slice of a wider tensor.  o_a, o_b and o share dtype (f16, bf16 or f32); every lse is float32.
 * d <= 256; for 16-bit tensors d is a multiple of 8, for fp32 any d >= 1 (fp32 rows are moved by 16-byte accesses when d % 4 == 0
 * and every o-like pointer is 16-byte aligned with strides that are multiples of 4, by 4-byte accesses otherwise).
 * In place: o == o_a with o_a's strides and lse == lse_a with lse_a's strides is allowed (likewise on the b pair): every element
 * is read before the thread that owns it writes it.  Any other overlap of an output with anything is undefined.
 * fa_merge_states_backward: from dO (do_) and dlse, the gradients of o and lse (dlse == NULL: zero), with t = <dO, o_a - o_b> per
 * row (an fp32 sum in a fixed order: the same bits on every run)
 *     dO_a = w_a dO,   dO_b = w_b dO,   dlse_a = w_a (dlse + w_b t),   dlse_b = w_b (dlse - w_a t),
 * all four written by the one launch.  A side with w_x = 0 gets zeros (and t, which may hold its NaN, is not used); a row with
 * both lse -inf gets zeros everywhere and its dlse is not read.  The stored o is not needed.  No in-place form.
 * Both calls are one launch on `stream`; nothing allocates, synchronises or reads device memory on the host: they can be captured.
 * Checked before any HIP call, the first broken rule named in fa_last_error(), in this order: dtype f32, f16 or bf16; 0 <= batch,
 * heads, rows < 2^31 and d >= 1 (FA_ERR_INVALID_ARGUMENT); d <= 256 (FA_ERR_UNSUPPORTED); d % 8 == 0 for 16-bit tensors; then a call
 * without a row (batch, heads or rows == 0) returns FA_OK without a launch and without looking at the pointers; batch * heads < 2^31
 * (FA_ERR_UNSUPPORTED); every pointer non-null (dlse alone may be); 16-bit o-like tensors 16-byte aligned with strides that are
 * multiples of 8 elements, every float32 tensor 4-byte aligned; every stride >= 0 with (extent - 1) * stride <= 2^58, so that no
 * 64-bit offset can overflow; an output that is an input has that input's strides. */
int fa_merge_states(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, void* o, float* lse, int64_t batch,
                    int64_t heads, int64_t rows, int64_t d, int dtype, int64_t o_a_batch_stride, int64_t o_a_head_stride,
                    int64_t o_a_row_stride, int64_t lse_a_batch_stride, int64_t lse_a_head_stride, int64_t lse_a_row_stride,
                    int64_t o_b_batch_stride, int64_t o_b_head_stride, int64_t o_b_row_stride, int64_t lse_b_batch_stride,
                    int64_t lse_b_head_stride, int64_t lse_b_row_stride, int64_t o_batch_stride, int64_t o_head_stride,
                    int64_t o_row_stride, int64_t lse_batch_stride, int64_t lse_head_stride, int64_t lse_row_stride, void* stream);
int fa_merge_states_backward(const void* o_a, const float* lse_a, const void* o_b, const float* lse_b, const void* do_,
                             const float* dlse, void* do_a, void* do_b, float* dlse_a, float* dlse_b, int64_t batch, int64_t heads,
                             int64_t rows, int64_t d, int dtype, int64_t o_a_batch_stride, int64_t o_a_head_stride,
                             int64_t o_a_row_stride, int64_t lse_a_batch_stride, int64_t lse_a_head_stride, int64_t lse_a_row_stride,
                             int64_t o_b_batch_stride, int64_t o_b_head_stride, int64_t o_b_row_stride, int64_t lse_b_batch_stride,
                             int64_t lse_b_head_stride, int64_t lse_b_row_stride, int64_t do_batch_stride, int64_t do_head_stride,
                             int64_t do_row_stride, int64_t dlse_batch_stride, int64_t dlse_head_stride, int64_t dlse_row_stride,
                             int64_t do_a_batch_stride, int64_t do_a_head_stride, int64_t do_a_row_stride, int64_t do_b_batch_stride,
                             int64_t do_b_head_stride, int64_t do_b_row_stride, int64_t dlse_a_batch_stride, int64_t dlse_a_head_stride,
                             int64_t dlse_a_row_stride, int64_t dlse_b_batch_stride, int64_t dlse_b_head_stride,
                             int64_t dlse_b_row_stride, void* stream);

/* --- FlashAttention-3's fp8 call: q, k, v ALREADY in OCP e4m3 (float8_e4m3fn), one float32 descale per (batch, K/V head) each.
 * Forward only.  q is (batch, heads_q, seqlen_q, 128), k and v are (batch, heads_kv, seqlen_k, 128) as raw e4m3 bytes; heads_q is a
 * multiple of heads_kv and query head h reads K/V head h / (heads_q / heads_kv).  q_descale, k_descale, v_descale: float32
 * (batch, heads_kv) device memory at their batch strides (0: one (heads_kv,) row for every batch), q's included (FlashAttention-3's
 * shape); NULL means 1.0 (and needs a stride of 0).  They are read on the device only and must be positive and finite.
 *     o = softmax(softmax_scale * q_descale * k_descale * q8 k8^T [causal]) (v8 * v_descale)
 * The causal diagonal is bottom-right aligned: row i sees key j <= i + seqlen_k - seqlen_q (fa_ex_forward's rule).  o is f16 or bf16
 * (`dtype`), lse float32 (batch, heads_q, seqlen_q) contiguous, natural log.  A row without a visible key gives o = 0, lse = -inf.
 * Arithmetic: both products run on the e4m3 matrix instruction with unit hardware scales and fp32 accumulation;
 * f = softmax_scale * log2(e) * q_descale * k_descale is one float per workgroup; p = exp2(fma(s, f, -m)); P is rounded to e4m3 on
 * EVERY row (l and lse come from the unrounded p); v_descale is applied once, with 1 / l.  There is no 16-bit-P route for short rows
 * (fa3_forward(fp8 = 1) has one for its backward's sake; FlashAttention-3 rounds P everywhere): 2^-4 relative per probability stands in
 * full on a row that sees a couple of keys.  NaN codes in the inputs propagate.
 * Layouts: each of q, k, v, o has batch, head and token strides in ELEMENTS of its own type (bytes for q, k, v; 16-bit elements for
 * o), the 128 elements of a row contiguous; bases and strides are multiples of 16 bytes.  So (B, N, H, 128) tensors need no copy,
 * nor does the [:, :seqlen_k] prefix of a contiguous (B, capacity, heads_kv, 128) e4m3 cache: bytes outside rows [0, seqlen_k) of a
 * view never reach a result, whatever they hold.  A stride of a dimension of extent 1 is not used.
 * Span limit: q and k are addressed through 32-bit buffer descriptors per (batch, head) unit, so round_up(rows, 256) * token stride
 * (bytes) must stay below 2^31 for both; above it the call is refused (FA_ERR_UNSUPPORTED, "span limit").
 * Workspace: the caller's, fa_fp8_forward_workspace_bytes(batch, heads_kv, seqlen_k, d) bytes (V^T: batch * heads_kv *
 * ceil(seqlen_k / 128) * 16384, plus 256 of padding; 0 for arguments the call would refuse), 16-byte aligned.  Two launches on
 * `stream` (a byte permutation of V into the workspace, the attention kernel); nothing allocates, synchronises or reads device
 * memory on the host: the call can be captured in a graph and replayed with changed descale values.
 * Checked before any HIP call, the first broken rule named in fa_last_error(), in this order: (1) q, k, v, o, lse non-null; (2) batch,
 * heads_q, heads_kv, seqlen_q, seqlen_k, d > 0; (3) d == 128, else FA_ERR_UNSUPPORTED; (4) heads_q % heads_kv == 0; (5) dtype f16 or
 * bf16, softmax_scale finite and > 0, a descale stride 0 or >= heads_kv (0 with a NULL descale), descales 4-byte aligned; (6) q, k,
 * v, o 16-byte aligned, lse 4-byte aligned, every stride used >= 0 and a multiple of 16 bytes, token strides >= 128; (7) the span
 * limit, and batch * heads * tiles below 2^31 (FA_ERR_UNSUPPORTED); (8) workspace non-null with workspace_bytes >= the need
 * (FA_ERR_WORKSPACE), 16-byte aligned.  Everything else is FA_ERR_INVALID_ARGUMENT. */
int fa_fp8_forward(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
                   const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k,
                   int64_t d, int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride,
                   int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride,
                   int64_t v_token_stride, int64_t o_batch_stride, int64_t o_head_stride, int64_t o_token_stride,
                   int64_t q_descale_batch_stride, int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal,
                   double softmax_scale, void* workspace, size_t workspace_bytes, void* stream);
size_t fa_fp8_forward_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t seqlen_k, int64_t d);

/* --- The packed and the paged form of the fp8 call (FlashAttention-3's flash_attn_varlen_func with q_descale / k_descale /
 * v_descale).  Forward only; a call family of its own.  Every sequence gets the bits of fa_fp8_forward on that sequence alone.
 * q is (total_q, heads_q, 128) raw e4m3 bytes packed by cu_seqlens_q (batch + 1 int32 device offsets), at its token and head
 * strides (a slice of a fused projection needs no copy).  Without block_table (NULL: the packed form) k and v are
 * (total_k, heads_kv, 128) packed by cu_seqlens_k, and max_blocks_per_seq, num_blocks, page_block_size and both page strides are 0.
 * With block_table, an int32 (batch, max_blocks_per_seq) device tensor, k and v are pools (num_blocks, page_block_size, heads_kv,
 * 128) with their own page and token strides; key t of sequence b is row t % page_block_size of page
 * block_table[b][t / page_block_size], and len_k[b] = cu_seqlens_k[b + 1] - cu_seqlens_k[b] clamped on the device to
 * [0, min(max_seqlen_k, max_blocks_per_seq * page_block_size)] (total_k is not used).  All strides are in bytes.
 * Descales as in fa_fp8_forward, (batch, heads_kv) with batch the number of sequences.  Query head h reads K/V head
 * h / (heads_q / heads_kv).  The causal diagonal is bottom-right aligned per sequence: j <= i + len_k[b] - len_q[b].
 * o is (total_q, heads_q, 128) contiguous in `dtype` (f16 / bf16), lse float32 (heads_q, total_q) contiguous, natural log.  A row
 * without a visible key (an empty key sequence, a causal row above the diagonal) gives o = 0, lse = -inf; rows of o and lse that
 * belong to no sequence are not written.
 * Nothing is read on the host: no synchronisation, and a captured call replays after the offsets, the table and the descale values
 * changed in place.  Offsets and table are untrusted: starts are clamped to [0, total], lengths to [0, max_seqlen_*]; a page
 * outside [0, num_blocks) reads as zero bytes for K and V; no table entry past ceil(len_k / page_block_size) is read; page offsets
 * are 64-bit and pages may be shared.
 * Span limits (FA_ERR_UNSUPPORTED, "span limit"): round_up(max_seqlen_q, 256) * q_token_stride below 2^31; packed,
 * round_up(max_seqlen_k, 256) * k_token_stride below 2^31; paged, page_block_size * token stride below 2^31 for both pools and
 * min(max_seqlen_k, max_blocks_per_seq * page_block_size) below 2^24.  Sequence, head and page offsets are 64-bit.
 * Workspace: the caller's, fa_fp8_forward_varlen_workspace_bytes(...) bytes, a function of host-known sizes only: V^T tiles of
 * 16384 bytes, heads_kv * (total_k / 128 + batch) of them packed (sequence b's start at tile cu_seqlens_k[b] / 128 + b of its
 * head), heads_kv * batch * ceil(min(max_seqlen_k, max_blocks_per_seq * page_block_size) / 128) paged (page_block_size > 0 selects
 * that form; sequence b's start at b * ceil(.. / 128)), plus 256; 0 for arguments the call would refuse.  Two launches on `stream`.
 * Checked before any HIP call, the first broken rule named in fa_last_error(), in this order: (1) q, k, v, o, lse, cu_seqlens_q,
 * cu_seqlens_k non-null; (2) batch, heads_q, heads_kv, d > 0, total_q, total_k, max_seqlen_q, max_seqlen_k in [0, 2^31); (3) d ==
 * 128, else FA_ERR_UNSUPPORTED; (4) heads_q % heads_kv == 0; (5) dtype f16 or bf16, softmax_scale finite and > 0; (6) with
 * block_table page_block_size a multiple of 16 in [16, 65536], num_blocks in [1, 2^31), batch * max_blocks_per_seq in [0, 2^31),
 * without it the five page arguments 0; (7) a descale stride 0 or >= heads_kv (0 with a NULL descale), descales 4-byte aligned; (8) q,
 * k, v, o 16-byte aligned, lse, offsets and table 4-byte aligned, every stride >= 0 and a multiple of 16 bytes, token strides >= 128;
 * (9) the span limits, and batch * heads * tiles below 2^31 (FA_ERR_UNSUPPORTED); (10) workspace non-null with workspace_bytes >=
 * the need (FA_ERR_WORKSPACE), 16-byte aligned.  Everything else is FA_ERR_INVALID_ARGUMENT. */
int fa_fp8_forward_varlen(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale,
                          const float* k_descale, const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                          const int32_t* block_table, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                          int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype, int64_t q_token_stride,
                          int64_t q_head_stride, int64_t k_token_stride, int64_t k_head_stride, int64_t v_token_stride,
                          int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks, int64_t page_block_size,
                          int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                          int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace, size_t workspace_bytes,
                          void* stream);
size_t fa_fp8_forward_varlen_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t total_k, int64_t max_seqlen_k,
                                             int64_t max_blocks_per_seq, int64_t page_block_size, int64_t d);

/* --- fp8 KV-cache decoding with split-KV: an e4m3 q over the e4m3 cache that fa_ex_forward_kvcache_fp8 writes.
 * Forward only; a call family of its own.  Both products run on the e4m3 matrix instruction:
 *     s[i, j] = softmax_scale * q_descale * k_descale * (q8[i] . k8[j]),   o[i] = sum_j softmax(s)[i, j] * v8[j] * v_descale
 * P is rounded to e4m3 on every row; l and lse come from the unrounded p.
 * q is (batch, seqlen_q, heads_q, 128) raw e4m3 bytes at its batch and token strides (heads adjacent, 128 bytes each).  Without
 * block_table the caches are (cache_batch or batch, cache_len, heads_kv, 128) e4m3 at their batch and token strides; with
 * block_table, an int32 (batch, cache_len / page_block_size) device tensor at block_table_row_stride, they are pools (num_blocks,
 * page_block_size, heads_kv, 128), k_batch_stride / v_batch_stride are the page strides and cache_len is the capacity
 * max_blocks_per_seq * page_block_size, as fa_ex_kvcache_workspace_bytes documents.  All strides are in bytes.  q_dtype and
 * cache_dtype must be FA_DTYPE_E4M3 (a 16-bit q is fa_ex_forward_kvcache_fp8's call); dtype names o's type, f16 or bf16.
 * len[b] = clamp(cache_seqlens[b], 0, cache_len) on the device (NULL: cache_len).  cache_batch_idx (contiguous form only; then
 * cache_batch > 0 is the caches' row count, else 0): sequence b lives in row cache_batch_idx[b]; an index outside [0, cache_batch)
 * gives an empty sequence.  Query head h reads K/V head h / (heads_q / heads_kv).  causal is bottom-right aligned: key j is visible
 * to token i iff j <= len[b] - seqlen_q + i.  Descales: float32 (batch, heads_kv) device tensors at their batch strides (0: one row
 * for every batch element), NULL = 1; finite and > 0 is the caller's contract.
 * o is (batch, seqlen_q, heads_q, 128) contiguous in dtype, lse float32 (batch, heads_q, seqlen_q) contiguous, natural log.  A row
 * without a visible key gives o = 0, lse = -inf.
 * Nothing is read on the host: lengths, table, indices and descales are untrusted device memory, and a captured call replays after
 * they changed in place.  A page outside [0, num_blocks) reads as zero K and zero V and takes part with score 0; no table entry
 * past ceil(len[b] / page_block_size) is read; bytes of the caches that no live token owns never reach a result.
 * num_splits: 0 = the library's rule (kv_num_splits' constants over 32-row tiles), else 1 .. 256.  Workspace: the caller's,
 * fa_fp8_forward_kvcache_workspace_bytes(...) bytes (0 for one split): fp32 partials in fa_ex_kvcache_workspace_bytes' layout.  One
 * launch, or two with more than one split.
 * Span limits (FA_ERR_UNSUPPORTED, "span limit"): seqlen_q * q_token_stride, and cache_len * token stride (contiguous) or
 * page_block_size * token stride (paged) of both caches, below 2^31; cache_len below 2^28.  Batch and page offsets are 64-bit.
 * Checked before any HIP call, the first broken rule named in fa_last_error(), in this order: (0) batch == 0 or seqlen_q == 0 is the
 * empty call, FA_OK; (1) q, k_cache, v_cache, o, lse non-null; (2) d == 128, q_dtype and cache_dtype FA_DTYPE_E4M3, dtype f16 or
 * bf16, else FA_ERR_UNSUPPORTED; (3) heads_q, heads_kv > 0 and heads_q % heads_kv == 0; (4) batch in [1, 65535], seqlen_q >= 1,
 * cache_len >= 1, (heads_q / heads_kv) * seqlen_q <= 2^20, softmax_scale finite and > 0, cache_batch in [1, 2^31) with
 * cache_batch_idx and 0 without; (5) q, k_cache, v_cache, o 16-byte aligned, lse, cache_seqlens, block_table and cache_batch_idx
 * 4-byte aligned, token strides multiples of 16 and >= heads * 128, batch / page strides multiples of 16, >= 0 and <= 2^44; (6) a
 * descale stride 0 or >= heads_kv (0 with a NULL descale), descales 4-byte aligned; (7) with block_table no cache_batch_idx,
 * page_block_size a multiple of 16 in [16, 65536] that divides cache_len, num_blocks in [1, 2^31), block_table_row_stride >=
 * cache_len / page_block_size, without it the three page arguments 0; (8) the span limits (FA_ERR_UNSUPPORTED); (9) num_splits in
 * [0, 256]; (10) with more than one split workspace non-null with workspace_bytes >= the need (FA_ERR_WORKSPACE), 16-byte aligned.
 * Everything else is FA_ERR_INVALID_ARGUMENT. */
int fa_fp8_forward_kvcache(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale,
                           const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                           const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                           int64_t cache_len, int64_t cache_batch, int64_t d, int dtype, int q_dtype, int cache_dtype,
                           int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_token_stride,
                           int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                           int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                           int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                           size_t workspace_bytes, void* stream);
/* cache_len: the capacity (paged: max_blocks_per_seq * page_block_size); 0 for arguments the call would refuse */
size_t fa_fp8_forward_kvcache_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                              int64_t d, int64_t num_splits);

/* --- A sliding window, a softcap and attention sinks on the three fp8 calls above.  Each _mod entry point takes its parent's
 * arguments followed by (window_left, window_right, softcap, sinks, sink_heads) and, given (-1, -1, 0.0, NULL, 0), IS its parent:
 * the same checks, the same launches of the same kernels.  Any other call launches kernels of its own (fwd_fp8in_mod_kernel,
 * fp8kv_split_mod_kernel; routes "fp8in_fwd_mod", "fp8in_fwd_varlen_mod", "fp8kv_split_mod" of fa_route_count) after the same
 * transposer.  The semantics are those of the 16-bit calls (fa_ex_forward_window / _scoremod / _sink, fa_ex_forward_kvcache*):
 *   window   (window_left, window_right), each >= 0 or -1 for unbounded; causal != 0 sets the right bound to 0.  Bottom-right
 *            aligned: row i of a sequence with len_q queries and len_k keys sits at pos = i + len_k - len_q and sees key j iff
 *            pos - window_left <= j <= pos + window_right and 0 <= j < len_k (the decode call: len_k = the clamped cache length,
 *            len_q = seqlen_q).  The prefill kernels walk only the 128-key tiles some row of a 256-row workgroup sees, the decode
 *            kernel cuts [lo, hi) into its splits, lo the first 64-key tile some row of the 32-row tile sees, and reads no table
 *            entry, K byte or V byte below lo.  The transposers of the prefill calls still transpose every key.
 *   softcap  >= 0, 0 = off: s~ = softcap * tanh(s / softcap) with s = softmax_scale * q_descale * k_descale * (q8 . k8), applied
 *            before the mask.
 *   sinks    NULL, or sink_heads == heads_q float32 on the device in natural-log units, one per QUERY head, read on the device
 *            only: an extra softmax column with a zero value (l += exp(sink - m), lse contains it), never capped, masked or
 *            windowed.  A row without a visible key gives o = 0 and lse = sink (without sinks: -inf); a head at -inf gives the
 *            bits of the call without sinks (prefill calls); +-1e4 stay finite.  The decode call joins the sink in the combine,
 *            once per row, so with sinks it runs at least two splits (num_splits 1 is raised to 2).
 * The decode call's split rule (num_splits = 0) takes min(cache_len, window_left + max(window_right, 0) + seqlen_q) for
 * cache_len when window_left >= 0 (causal: window_right counts as 0): the host cannot see the lengths, and the capacity would cut
 * a short window into splits of under one tile.  The result's bits depend on num_splits, the window and nothing else of the
 * launch.  fa_fp8_forward_kvcache_workspace_bytes_mod is that call's need (with_sinks: sinks != NULL); the parents' workspace
 * functions serve the other two.
 * Checked beside the parent's rules, by name (FA_ERR_INVALID_ARGUMENT): the window bounds >= -1; softcap finite and >= 0;
 * sink_heads == heads_q with sinks and 0 without, sinks 4-byte aligned. */
int fa_fp8_forward_mod(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
                       const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k,
                       int64_t d, int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride,
                       int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride,
                       int64_t v_head_stride, int64_t v_token_stride, int64_t o_batch_stride, int64_t o_head_stride,
                       int64_t o_token_stride, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                       int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace, size_t workspace_bytes,
                       void* stream, int64_t window_left, int64_t window_right, double softcap, const float* sinks,
                       int64_t sink_heads);
int fa_fp8_forward_varlen_mod(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale,
                              const float* k_descale, const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                              const int32_t* block_table, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                              int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t d, int dtype,
                              int64_t q_token_stride, int64_t q_head_stride, int64_t k_token_stride, int64_t k_head_stride,
                              int64_t v_token_stride, int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks,
                              int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride,
                              int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale,
                              void* workspace, size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right,
                              double softcap, const float* sinks, int64_t sink_heads);
int fa_fp8_forward_kvcache_mod(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale,
                               const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                               const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                               int64_t cache_len, int64_t cache_batch, int64_t d, int dtype, int q_dtype, int cache_dtype,
                               int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_token_stride,
                               int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                               int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                               int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap,
                               const float* sinks, int64_t sink_heads);
/* 0 for arguments the call would refuse */
size_t fa_fp8_forward_kvcache_workspace_bytes_mod(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                                  int64_t d, int64_t num_splits, int causal, int64_t window_left, int64_t window_right,
                                                  int with_sinks);

/* --- Head dims 64 and 256 beside 128 on the three fp8 calls.  Each _hdim entry point takes its _mod parent's argument list (the
 * head dim is named head_dim here) and the same rules in the same order, with two changes: head_dim may be 64, 128 or 256 (any other
 * value: FA_ERR_UNSUPPORTED, "head_dim N is not supported (64, 128 or 256)", where the parent checks d == 128), and head_dim
 * stands where the parent's rules say 128: the least token stride (heads * head_dim for the decode call), the stride handed on for
 * a single row, the spans.  The entry points above keep refusing everything but 128.
 * head_dim == 128 IS the _mod call: the same launches of the same kernels, the same routes counted, the same workspace size.
 * head_dim 64 and 256 run instantiations of the featured kernels at that width (routes "fp8in_fwd_hdim", "fp8in_fwd_varlen_hdim",
 * "fp8kv_split_hdim" of fa_route_count, one count a call that launched), with or without a window, a softcap or sinks, and
 * everything documented for 128 holds: GQA, seqlen_q != seqlen_k with the bottom-right diagonal, strided views, untrusted
 * lengths, tables and indices, graph replay, f16 / bf16 o.  The arithmetic is that of 128 with head_dim / 64 score instructions
 * a 32-key block accumulated in ascending head-dim order; at 256 the prefill kernels take the softmax step (maximum, lazy
 * rescale, e4m3 P) over 64 keys instead of 128.
 * Workspace: the V^T image of the prefill calls is units_kv * tiles * head_dim * 128 + 256 bytes (tiles as the parents count
 * them); the decode partials follow fa_fp8_forward_kvcache_workspace_bytes_mod at head_dim (the split rule counts keys, not bytes).
 * Not here: fa_fp8_kvcache_step (128 only; a 64 / 256 cache is filled by fa_ex_forward_kvcache_fp8's append and q comes from
 * fa_fp8_quantize), head dims 96 and 192, fa3_forward(fp8 = 1), the MLA and indexer families. */
int fa_fp8_forward_hdim(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale, const float* k_descale,
                       const float* v_descale, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t seqlen_k,
                       int64_t head_dim, int dtype, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride,
                       int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride,
                       int64_t v_head_stride, int64_t v_token_stride, int64_t o_batch_stride, int64_t o_head_stride,
                       int64_t o_token_stride, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                       int64_t v_descale_batch_stride, int causal, double softmax_scale, void* workspace, size_t workspace_bytes,
                       void* stream, int64_t window_left, int64_t window_right, double softcap, const float* sinks,
                       int64_t sink_heads);
int fa_fp8_forward_varlen_hdim(const void* q, const void* k, const void* v, void* o, float* lse, const float* q_descale,
                              const float* k_descale, const float* v_descale, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                              const int32_t* block_table, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q,
                              int64_t total_k, int64_t max_seqlen_q, int64_t max_seqlen_k, int64_t head_dim, int dtype,
                              int64_t q_token_stride, int64_t q_head_stride, int64_t k_token_stride, int64_t k_head_stride,
                              int64_t v_token_stride, int64_t v_head_stride, int64_t max_blocks_per_seq, int64_t num_blocks,
                              int64_t page_block_size, int64_t k_page_stride, int64_t v_page_stride, int64_t q_descale_batch_stride,
                              int64_t k_descale_batch_stride, int64_t v_descale_batch_stride, int causal, double softmax_scale,
                              void* workspace, size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right,
                              double softcap, const float* sinks, int64_t sink_heads);
int fa_fp8_forward_kvcache_hdim(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale,
                               const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                               const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                               int64_t cache_len, int64_t cache_batch, int64_t head_dim, int dtype, int q_dtype, int cache_dtype,
                               int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_token_stride,
                               int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                               int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                               int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap,
                               const float* sinks, int64_t sink_heads);
/* the three needs; 0 for arguments the call would refuse (head_dim outside {64, 128, 256} among them) */
size_t fa_fp8_forward_hdim_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t seqlen_k, int64_t head_dim);
size_t fa_fp8_forward_varlen_hdim_workspace_bytes(int64_t batch, int64_t heads_kv, int64_t total_k, int64_t max_seqlen_k,
                                                  int64_t max_blocks_per_seq, int64_t page_block_size, int64_t head_dim);
size_t fa_fp8_forward_kvcache_hdim_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                                  int64_t head_dim, int64_t num_splits, int causal, int64_t window_left, int64_t window_right,
                                                  int with_sinks);

/* --- The fp8 quantiser: one 16-bit tensor x -> e4m3 codes plus float32 descales of the shape the fp8 calls above read (the
 * producer of fa_fp8_forward / _varlen / _kvcache and of the e4m3 cache).  One call covers one tensor, addressed through its own
 * strides like fa_rotary_apply's, so a slice of a fused qkv projection goes in without a copy.
 * x: f16 or bf16, element (b, h, i, e) at x[b * x_batch_stride + h * x_head_stride + i * x_token_stride + e], the d elements of a
 * head row contiguous; d a multiple of 16 in [16, 256]; strides in elements, multiples of 8, the base 16-byte aligned; offsets are
 * 64-bit.  (B, H, N, d) and (B, N, H, d) differ in their strides only.  Packed form: cu_seqlens int32 (batch + 1,) device memory, x
 * (total, heads, d) at its token and head strides, seqlen == 0 and the batch strides unused; sequence b owns the tokens of
 * fa_ex_forward_varlen's clamp (start = clamp(cu[b], 0, total), end = clamp(cu[b + 1], start, total), len = min(end - start,
 * max_seqlen)), so decreasing or oversized offsets address nothing outside x and out.
 * Scale units: heads_per_scale = g divides heads; unit (b, j) is heads [j g, (j + 1) g) x all tokens of sequence b x all of d.  For
 * q under grouped-query attention g = H_q / H_kv gives the (batch, H_kv) descales of the fp8 calls; for k and v g = 1.
 * Dynamic mode (descale == NULL): amax[b, j] = max |float(x)| over the unit (exact: a maximum does not depend on the order);
 *     descale[b, j] = amax > 0 ? amax / 448 : 1        (the division IEEE-rounded, __fdiv_rn)
 * and with scale_pow2 != 0 rounded up to a power of two by fa_mla_fp8_pack's rule: taken in the bit pattern, a mantissa that is
 * not zero goes to the next exponent (exact for every normal descale below 2^127).  It is written to descale_out, float32 (batch,
 * heads / g) contiguous, which must be given.  A sequence of length 0 writes descale 1.
 * Static mode (descale given): float32, unit (b, j) reads descale[b * descale_batch_stride + j]; descale_batch_stride == 0 shares
 * one (heads / g,) row among the batch.  Read on the device only; positive and finite by contract.  descale_out may be NULL; given,
 * it receives a copy.  One launch, no workspace.
 * Codes, both modes: inv = 1 / descale (IEEE-rounded), y = min(max(float(x) * inv, -448), 448), then rounded to nearest even to
 * OCP e4m3 (v_cvt_pk_fp8_f32).  That is the arithmetic of the e4m3 cache append (fa_ex_forward_kvcache_fp8), so with the same
 * descale the bytes are the ones the append stores.  NaN and infinity in x are outside the contract.
 * out: e4m3 bytes, element (b, h, i, e) at out[b * out_batch_stride + h * out_head_stride + i * out_token_stride + e] with its own
 * strides in bytes, each a multiple of 16, the base 16-byte aligned: (B, H, N, d) -> (B, N, H, d) costs nothing, and out may be
 * the [:, :N] prefix of a larger (B, capacity, H, d) e4m3 cache.  The strides must not let two addressed rows overlap.  Bytes of
 * out outside the addressed rows are never written, nor are the rows of packed tokens that no sequence owns.
 * Optional fused rotary (for q and k): rotary_cos / rotary_sin non-NULL are fa_rotary_apply's tables, to the letter: (seqlen_ro,
 * rotary_dim / 2) in x's dtype, rows at even strides, 4-byte aligned, rotary_dim a multiple of 16 in [16, d], rotary_interleaved
 * selecting the pairing, token i of sequence b at pos = seqlen_offset + (seqlen_offsets ? seqlen_offsets[b] : 0) + i, formed in 64
 * bits, rotated iff 0 <= pos < seqlen_ro and passed through otherwise.  The rotated value is formed in fp32 and rounded ONCE to
 * x's dtype (fp32 sum, then nearest even), the rule fa_rotary_apply states; amax and codes are taken from that 16-bit value.  So
 * this call with tables equals this call without them on fa_rotary_apply's result, in every byte and every descale, wherever
 * fa_rotary_apply rounds through fp32 too: always for bf16; for f16 its compiled code rounds one slot of the interleaved pairing
 * from the exact sum instead, which moves a 16-bit value by one step where the fp32 sum is an f16 tie (about 1 value in 3 * 10^4;
 * DESIGN 9zb).  Both tables NULL: no rotation, and the other rotary arguments are not looked at.
 * Kernels: static mode is one launch (route "fp8_quant_static").  Dynamic mode on a unit of at most 1024 chunks of 16 bytes of
 * work per workgroup (seqlen * g * d / 8 <= 1024, max_seqlen for seqlen in the packed form; with non-interleaved rotary a chunk
 * pair counts once) is one launch of one workgroup per unit that holds the unit in registers (route "fp8_quant_fused", no
 * workspace: the decode step's q is such a unit); larger units take an amax launch, whose workgroups meet in an atomic maximum on
 * an amax scratch in the workspace (zeroed by a small kernel on the stream first), and a quantise launch (route "fp8_quant_two_pass").  Every
 * route gives the same bits, and two runs give the same bits.  fa_fp8_quantize_workspace_bytes sizes the scratch: 4 bytes a unit,
 * rounded up to 256; 0 for arguments the call would refuse.  The workspace is 16-byte aligned and is not descale_out.
 * Nothing allocates, synchronises or reads device memory on the host: a captured call replays after x, descale, cu_seqlens, the
 * offsets and the tables' contents change in place (shapes, strides and seqlen_offset are fixed by the capture).
 * Checked before any HIP call (the first broken rule named in fa_last_error(), FA_ERR_INVALID_ARGUMENT unless said otherwise),
 * in this order: dtype f16 or bf16; d a multiple of 16 in [16, 256]; batch >= 1, heads >= 1 with heads * d < 2^31; heads_per_scale
 * >= 1 dividing heads; batch * heads / heads_per_scale < 2^31; seqlen in [0, 2^31); x and out non-null and 16-byte aligned;
 * descale, descale_out, cu_seqlens, seqlen_offsets 4-byte aligned; dynamic mode needs descale_out; with cu_seqlens 0 <= max_seqlen
 * <= total < 2^31 and seqlen == 0, without it total == max_seqlen == 0; x's strides >= 0, multiples of 8, every (extent - 1) *
 * stride <= 2^58; out's strides >= 0, multiples of 16, every (extent - 1) * stride <= 2^58; out's rows do not overlap: head stride
 * >= d and token stride >= (heads - 1) * head stride + d, or token stride >= d and head stride >= (tokens - 1) * token stride + d,
 * and with batch > 1 in the padded form the batch stride covers one batch element; static mode: descale_batch_stride == 0 or in
 * [heads / g, 2^40]; with tables: both given and 4-byte aligned, rotary_dim a multiple of 16 in [16, d], row strides >=
 * rotary_dim / 2 (and <= 2^31) and even, seqlen_ro in [1, 2^31), |seqlen_offset| < 2^31; a unit of seqlen * g * d / 8 >= 2^31
 * chunks is FA_ERR_UNSUPPORTED; the two-pass route needs the workspace (FA_ERR_WORKSPACE).  A static call without tokens and
 * without descale_out returns FA_OK without a launch. */
int fa_fp8_quantize(const void* x, void* out, const float* descale, float* descale_out, const int32_t* cu_seqlens,
                    const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride, int64_t rotary_sin_row_stride,
                    int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved, int64_t seqlen_offset,
                    const int32_t* seqlen_offsets, int64_t batch, int64_t heads, int64_t seqlen, int64_t d, int64_t heads_per_scale,
                    int64_t total, int64_t max_seqlen, int dtype, int64_t x_batch_stride, int64_t x_head_stride,
                    int64_t x_token_stride, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_token_stride,
                    int64_t descale_batch_stride, int scale_pow2, void* workspace, size_t workspace_bytes, void* stream);
size_t fa_fp8_quantize_workspace_bytes(int64_t batch, int64_t heads, int64_t heads_per_scale);

/* --- The fp8 decode step: append the new tokens to the e4m3 cache, rotate and quantise q, and attend, in one
 * call; a family of its own.  It takes fa_fp8_forward_kvcache_mod's arguments, which keep their meaning except where said here,
 * followed by the new-token group (k_new .. v_new_token_stride), in_dtype, the q8 group and the rotary group as
 * fa_ex_forward_kvcache_rotary spells it.  All strides are in bytes, but the rotary row strides, which count elements.
 * cache_seqlens (required) holds the lengths BEFORE the append: L_b = clamp(cache_seqlens[b], 0, cache_len - seqlen_new),
 * hk = h / (heads_q / heads_kv), len_b = L_b + seqlen_new.  q_dtype names the type of q and in_dtype that of k_new and v_new
 * (batch, seqlen_new, heads_kv, 128); they must be equal.
 * 16-bit mode (FA_DTYPE_F16 or FA_DTYPE_BF16):
 *   1. Append.  Token n of sequence b goes to position L_b + n of cache row cache_batch_idx[b] (or b), or through the table to
 *      pool[block_table[b, pos / page_block_size], pos % page_block_size].  k_new is rotated at table row L_b + n when tables are
 *      given, in fp32 from the 16-bit inputs, and rounded once to in_dtype; v_new is taken as it is.  The stored bytes are
 *      clamp(float(x) * (1.0f / descale[b, hk]), -448, 448) rounded to nearest even: the bytes fa_ex_forward_kvcache_fp8 stores,
 *      by the same device functions.  A row index outside [0, cache_batch) or a page outside [0, num_blocks) drops the token.  No
 *      other byte of the caches is written.
 *   2. q.  Token i is rotated by fa_ex_forward_kvcache_rotary's rule: at table row L_b + i when causal is set or a window bound
 *      is given (>= 0 as passed), otherwise every token at L_b; rounded once to in_dtype; then quantised with
 *      1.0f / q_descale[b, hk] by the append's arithmetic.  The codes go to q8_out, e4m3 (batch, seqlen_q, heads_q, 128) at
 *      q8_batch_stride / q8_token_stride, or with q8_out NULL (both strides 0) into the workspace.  q is not modified.
 *   3. Attention.  o and lse are, bit for bit, fa_fp8_forward_kvcache_mod on those codes and the caches as step 1 left them with
 *      cache_seqlens = len_b and the same descales, causal, window, softcap, sinks and num_splits.
 * e4m3 mode (FA_DTYPE_E4M3, FlashAttention-3's form): the new bytes are scattered as they are, q is used in place, q8_out and
 * the rotary tables must be NULL.
 * Kernels: one launch of fp8kv_step_prep_kernel (route and profile scope "fp8kv_step_prep") does steps 1 and 2 and writes len_b
 * for every sequence; then the launches of fa_fp8_forward_kvcache_mod, unchanged.  Nothing is read on the host: lengths, table,
 * indices, descales and tables are device memory, the first three untrusted and clamped as above, so a captured call replays
 * after any of them changed in place.  Two sequences that append to one page, and a duplicate cache_batch_idx, are undefined.
 * Workspace: fa_fp8_kvcache_step_workspace_bytes(...) bytes, always > 0: [len_b, int32 | the q codes, 16-bit mode without q8_out |
 * fa_fp8_forward_kvcache_workspace_bytes_mod's partials], each part rounded up to 256 bytes; 0 for arguments the call would refuse.
 * Checked before any HIP call, the first broken rule named in fa_last_error(), in this order: (0) batch == 0 is the empty call,
 * FA_OK; (1) q, k_cache, v_cache, o, lse, k_new, v_new, cache_seqlens non-null; (2) d == 128, q_dtype f16, bf16 or e4m3, in_dtype
 * == q_dtype ("mixed"), cache_dtype FA_DTYPE_E4M3, dtype f16 or bf16, else FA_ERR_UNSUPPORTED; (3), (4) the parent's, and 1 <=
 * seqlen_new <= cache_len; (5) the parent's with q's token stride >= heads_q * 128 elements of q_dtype, and k_new, v_new 16-byte
 * aligned with strides that are multiples of 16, the token stride >= heads_kv * 128 elements and <= 2^44; q8_out only in 16-bit
 * mode, 16-byte aligned, its strides multiples of 16, the token stride >= heads_q * 128, and both 0 without it; (6), (7) the
 * parent's; (8) the parent's span limits, and seqlen_new * token stride of k_new and v_new and seqlen_q * q8_token_stride below
 * 2^31 (FA_ERR_UNSUPPORTED); (9) rotary: only in 16-bit mode; both tables or none; rotary_dim a multiple of 16 in [16, 128];
 * seqlen_ro >= cache_len + max(0, seqlen_q - seqlen_new) (the tables are not bounds-checked on the device); row strides >=
 * rotary_dim / 2, even and <= 2^40; tables 4-byte aligned; the five integers 0 without tables; (10) num_splits in [0, 256] and the
 * window, softcap and sinks rules of the _mod calls; (11) workspace non-null with workspace_bytes >= the need (FA_ERR_WORKSPACE),
 * 16-byte aligned.  Everything else is FA_ERR_INVALID_ARGUMENT. */
int fa_fp8_kvcache_step(const void* q, void* k_cache, void* v_cache, void* o, float* lse, const float* q_descale,
                        const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                        const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                        int64_t cache_len, int64_t cache_batch, int64_t d, int dtype, int q_dtype, int cache_dtype,
                        int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_token_stride,
                        int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                        int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                        int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                        size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap,
                        const float* sinks, int64_t sink_heads, const void* k_new, const void* v_new, int64_t seqlen_new,
                        int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                        int64_t v_new_token_stride, int in_dtype, void* q8_out, int64_t q8_batch_stride, int64_t q8_token_stride,
                        const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                        int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved);
/* with_q8_out: q8_out != NULL; 0 for arguments the call would refuse */
size_t fa_fp8_kvcache_step_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                           int64_t d, int64_t num_splits, int causal, int64_t window_left, int64_t window_right,
                                           int with_sinks, int in_dtype, int with_q8_out);

/* --- Packed queries and new keys on the fp8 decode call and the fp8 decode step, and the step at head dims 64 / 256 (DESIGN.md
 * 9zf): FlashAttention-3's cu_seqlens_q / cu_seqlens_k_new / max_seqlen_q as fa_ex_forward_kvcache_varlen states them.  Two
 * families of one, each with its size function.
 * fa_fp8_forward_kvcache_varlen takes fa_fp8_forward_kvcache_hdim's list followed by cu_seqlens_q, total_q, max_seqlen_q.  With
 * NULL, 0, 0 it IS the _hdim call: the same checks, launches and routes.  With cu_seqlens_q (int32 (batch + 1,) device memory) q is
 * packed (total_q, heads_q, head_dim) at q_token_stride, o is dense (total_q, heads_q, head_dim), lse (heads_q, total_q); seqlen_q
 * and q_batch_stride are not used.  Sequence b owns the tokens [start, start + nq_b) with start = clamp(cu[b], 0, total_q) and nq_b
 * = clamp(cu[b + 1] - cu[b], 0, min(max_seqlen_q, total_q - start)) (kv_cu_range, csrc/fa_decode_common.h): whatever the array
 * holds, nothing outside q is read and nothing outside o, lse and the workspace written.  Every sequence gets, bit for bit, what the
 * padded call returns for it alone (batch 1, its own tokens, its cache row / table row / cache_batch_idx entry / descale row, the
 * same num_splits, window, softcap and sinks): len_b = clamp(cache_seqlens[b], 0, cache_len), the causal diagonal is len_b - nq_b.
 * nq_b == 0 writes nothing; rows of o / lse that no sequence owns keep their contents.  total_q == 0 or max_seqlen_q == 0 is the
 * empty call (FA_OK).
 * Kernels: fp8kv_split_mod_kernel's packed instantiation on the grid (S, ceil(max_seqlen_q * G / 32) * heads_kv, batch), route and
 * profile scope "fp8kv_split_varlen", one count a call, at every head dim and with or without a window, a softcap or sinks; for S >
 * 1 a memset of the lse partials (a graph node) and kv_combine_kernel in its packed mode.  num_splits == 0 takes the parents' rule
 * over ceil(max_seqlen_q * G / 32) row tiles, and a window is measured against max_seqlen_q.  Nothing is read on the host; a
 * captured call replays after offsets, lengths, table and descales changed in place (total_q, max_seqlen_q fixed by the capture).
 * fa_fp8_forward_kvcache_varlen_workspace_bytes: S * total_q * heads_q * (head_dim + 1) floats for S > 1, each of the two parts
 * rounded up to 256 bytes; sinks raise S to at least 2; 0 for one split and for arguments the call would refuse.
 *
 * fa_fp8_kvcache_step_varlen takes fa_fp8_kvcache_step's list with head_dim in {64, 128, 256}, followed by cu_seqlens_q, total_q,
 * max_seqlen_q, cu_seqlens_k_new, total_k_new.  With the five NULL / 0 and head_dim == 128 it IS fa_fp8_kvcache_step, launch for
 * launch; with the five NULL / 0 at 64 / 256 it is the padded step at that width.  With cu_seqlens_q, q is packed as above and
 * q8_out is (total_q, heads_q, head_dim) at q8_token_stride (q8_batch_stride unused).  The new keys are packed (total_k_new,
 * heads_kv, head_dim) by cu_seqlens_k_new (clamped likewise, the bound being cache_len; seqlen_new and the batch strides of k_new,
 * v_new unused), or padded (batch, seqlen_new, heads_kv, head_dim) when that array is NULL.  Per sequence: L_b =
 * clamp(cache_seqlens[b], 0, cache_len - nnew_b), len_b = L_b + nnew_b, new key n is rotated at L_b + n, q token i at L_b + i when
 * causal or a window bound >= 0 is given, else at L_b; nq_b == 0 still appends, nnew_b == 0 appends nothing.  The cache bytes, the
 * q codes and o / lse are those of the padded step on the sequence alone.  Kernels: fp8kv_step_prep_varlen_kernel (route
 * "fp8kv_step_prep_varlen", one count a call; every packed call and every call at 64 / 256), then the launches above on the q codes
 * and len_b; total_q == 0 or max_seqlen_q == 0 launches the prep only.  Workspace: [len_b, batch int32 | the q codes, total_q *
 * heads_q * head_dim bytes (batch * seqlen_q * .. padded), 16-bit mode without q8_out | the decode call's partials], each part
 * rounded up to 256 bytes.  fa_fp8_kvcache_step_varlen_workspace_bytes: the step's list with head_dim, plus total_q, max_seqlen_q;
 * seqlen_q == 0 asks about a packed call, seqlen_q != 0 (with total_q == max_seqlen_q == 0) about the padded one.
 *
 * Rules, both entry points: the parents' rules in the parents' order up to and including the window / softcap / sinks rules, with
 * head_dim wherever a rule says 128 (token strides >= heads * head_dim elements, rotary_dim <= head_dim, head_dim outside {64, 128,
 * 256}: FA_ERR_UNSUPPORTED "(64, 128 or 256)"), and with cu_seqlens_q without the rules on seqlen_q and q_batch_stride (with
 * cu_seqlens_k_new: on seqlen_new and the batch strides of k_new / v_new).  Then the packed group, in this order: (P1) total_q and
 * max_seqlen_q are 0 without cu_seqlens_q, total_k_new is 0 without cu_seqlens_k_new; (P2) cu_seqlens_k_new needs cu_seqlens_q;
 * (P3) 0 <= max_seqlen_q <= total_q; (P4) total_q and total_k_new in [0, 2^31); (P5) max_seqlen_q * token stride of q and of
 * q8_out below 2^31 bytes (FA_ERR_UNSUPPORTED, "span limit"); (P6) (heads_q / heads_kv) * max_seqlen_q <= 2^20, and the row tiles
 * * heads_kv fit one launch (FA_ERR_UNSUPPORTED); (P7) with rotary tables seqlen_ro >= cache_len + max_seqlen_q; (P8) both arrays
 * 4-byte aligned.  Last the parents' workspace rule.  Still refused: head dims 96 / 192 and block_table with cache_batch_idx. */
int fa_fp8_forward_kvcache_varlen(const void* q, const void* k_cache, const void* v_cache, void* o, float* lse, const float* q_descale,
                                 const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                                 const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                                 int64_t cache_len, int64_t cache_batch, int64_t head_dim, int dtype, int q_dtype, int cache_dtype,
                                 int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_token_stride,
                                 int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                                 int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                                 int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                                 size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap,
                                 const float* sinks, int64_t sink_heads, const int32_t* cu_seqlens_q, int64_t total_q,
                                 int64_t max_seqlen_q);
size_t fa_fp8_forward_kvcache_varlen_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t total_q, int64_t max_seqlen_q,
                                                     int64_t cache_len, int64_t head_dim, int64_t num_splits, int causal,
                                                     int64_t window_left, int64_t window_right, int with_sinks);
int fa_fp8_kvcache_step_varlen(const void* q, void* k_cache, void* v_cache, void* o, float* lse, const float* q_descale,
                               const float* k_descale, const float* v_descale, const int32_t* cache_seqlens, const int32_t* block_table,
                               const int32_t* cache_batch_idx, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q,
                               int64_t cache_len, int64_t cache_batch, int64_t head_dim, int dtype, int q_dtype, int cache_dtype,
                               int64_t q_batch_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_token_stride,
                               int64_t v_batch_stride, int64_t v_token_stride, int64_t block_table_row_stride, int64_t num_blocks,
                               int64_t page_block_size, int64_t q_descale_batch_stride, int64_t k_descale_batch_stride,
                               int64_t v_descale_batch_stride, int causal, double softmax_scale, int64_t num_splits, void* workspace,
                               size_t workspace_bytes, void* stream, int64_t window_left, int64_t window_right, double softcap,
                               const float* sinks, int64_t sink_heads, const void* k_new, const void* v_new, int64_t seqlen_new,
                               int64_t k_new_batch_stride, int64_t k_new_token_stride, int64_t v_new_batch_stride,
                               int64_t v_new_token_stride, int in_dtype, void* q8_out, int64_t q8_batch_stride, int64_t q8_token_stride,
                               const void* rotary_cos, const void* rotary_sin, int64_t rotary_cos_row_stride,
                               int64_t rotary_sin_row_stride, int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved,
                               const int32_t* cu_seqlens_q, int64_t total_q, int64_t max_seqlen_q, const int32_t* cu_seqlens_k_new,
                               int64_t total_k_new);
size_t fa_fp8_kvcache_step_varlen_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t seqlen_q, int64_t cache_len,
                                                  int64_t head_dim, int64_t num_splits, int causal, int64_t window_left, int64_t window_right,
                                                  int with_sinks, int in_dtype, int with_q8_out, int64_t total_q, int64_t max_seqlen_q);

/* --- support entry points (no reference counterpart: the reference allocates inside the callee) --- */
/* bytes for the CURRENT kernel mode: two float row constants per query row (+ an fp32 dQ scratch of bh*n*d floats in
 * FA_MODE_BWD_ATOMIC only); ask again after changing the mode */
size_t fa_backward_workspace_bytes(int64_t bh, int64_t n, int64_t d, int dtype);
/* The size that lets the backward hand dS from its dK/dV kernel to its dQ kernel instead of recomputing S and dP there
 * (d = 128, 16-bit tensors: N * N * 2 bytes per (b,h), at most 4 GiB whatever BH and N are — the (b,h) units are worked through
 * in equal chunks of that size; option ds_chunk_mb moves the bound).  Without the causal mask that serves every launch; under it
 * rows of 4096 and more, or launches of 160 and more 256-row tiles, while a chunk holds 16 units or the whole launch (option
 * dq = 6 forces it elsewhere).  Equals fa_backward_workspace_bytes where it does not apply.  A backward call given less than this
 * (but at least fa_backward_workspace_bytes) runs the recomputing dQ pass: same results up to summation order, 4 - 17 % more
 * backward time depending on the launch (profiles/r03_bwd_variants.md, r03_ds_chunk_sweep.md). */
size_t fa_backward_workspace_bytes_fast(int64_t bh, int64_t n, int64_t d, int dtype, int causal);
size_t fa3_forward_workspace_bytes(int64_t bh, int64_t n, int64_t d, int dtype, int fp8);
size_t fa3_backward_workspace_bytes(int64_t bh, int64_t n, int64_t d, int dtype, int fp8);
const char* fa_last_error(void);
const char* fa_version(void);
int fa_set_kernel_mode(int mode);      /* FA_MODE_*; returns the previous mode */
/* debug only: device buffer of 4096 int64 for the phase timestamps of the staggered forward kernel (NULL = off) */
int fa_debug_trace_buffer(void* device_ptr);
int fa_set_option(const char* name, int value); /* tuning knobs for sweeps: fwd_kb, fwd_stag, fwd_tpw, dq_tpw, dkdv_tpw, ... (csrc/fa_kernels.h) */
int fa_device_is_gfx950(int device);   /* 1 if `device` reports gcnArchName gfx950, 0 otherwise, <0 on HIP error */
/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline figure).
 * fa_profile_enable(1) starts collecting (and clears old records), fa_profile_report waits for the events and
 * writes one "kernel_name launches total_ms" line per kernel; returns bytes written or a negative code. */
int fa_profile_enable(int on);
int fa_profile_report(char* buf, size_t cap);
/* Which form a launcher took: the number of launches of the named route since the library was loaded, negative for an unknown
 * name.  "dkdv_stream": the dS-storing dK/dV stream kernel in its general form; "dkdv_lean": its lean form (non-causal launches
 * whose key count is a multiple of 256; option dkdv_lean = 2 forces the general form).  "fp8_quant_fused", "fp8_quant_two_pass",
 * "fp8_quant_static": the three routes of fa_fp8_quantize, one count a call that launched.  "fp8in_fwd_mod",
 * "fp8in_fwd_varlen_mod", "fp8kv_split_mod": the featured kernels of fa_fp8_forward_mod, fa_fp8_forward_varlen_mod and
 * fa_fp8_forward_kvcache_mod, one count a call that launched one (a _mod call with default trailing arguments counts none).
 * "fp8kv_step_prep": the append / rotary / quantise launch of fa_fp8_kvcache_step, one count a call.  "fp8in_fwd_hdim",
 * "fp8in_fwd_varlen_hdim", "fp8kv_split_hdim": the head dim 64 / 256 kernels of fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim and
 * fa_fp8_forward_kvcache_hdim, one count a call that launched one (head_dim 128 counts what the _mod call counts).
 * "fp8kv_split_varlen": the packed split kernel of fa_fp8_forward_kvcache_varlen and fa_fp8_kvcache_step_varlen;
 * "fp8kv_step_prep_varlen": the prep launch of fa_fp8_kvcache_step_varlen with packed tokens or at head dim 64 / 256; one count a
 * call that launched one (null packed groups count what the parent calls count). */
int64_t fa_route_count(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* FA_MI355X_H */
