// Shared by the extended-attention kernels (fa_ex.hip: exact f32; fa_ex_mfma.hip: 16-bit MFMA): the parameter block, the
// visibility rule and the counter-based dropout generator.
#pragma once
#include "fa_common.h"
#include "fa_kernels.h"

namespace fa {

struct ExParams {
    // the band of row i: keys [i + coff - wl, i + coff + wr].  wr = 0 under the causal mask, kWinNone (wider than any
    // problem: nq, nk <= 2^24) on an unbounded side, so the bounds enter the arithmetic without a branch.  (First: the
    // fields after them keep their relative offsets and alignment, so kernels without a window load them as before.)
    int wl, wr;
    int nq, nk, d;
    int causal;            // 0 | 1 (bottom-right aligned)
    int coff;              // nk - nq
    // Variable-length (packed) sequences (the varlen instantiations; fa_ex_mfma.hip FEAT bit 3): their fields take the padding
    // before `mask` and the places of the masks, which a varlen call does not have, so no other field moves and the kernels
    // without them are the ones they were.  nq, nk are then max_seqlen_q / _k (grid, dropout counters) and each workgroup
    // narrows them and coff to its sequence (seq_span).  Unit u = b * hq + h; token t of sequence b, head h of q is at
    // q + (cu_q[b] + t) * sq + h * d (k, v: sk, sv and head h / kv_group); of o, do, dq, and of dk, dv per query head, at
    // ((cu_q[b] + t) * hq + h) * d; lse (hq, total_q).
    int hq;                // query heads
    union { const uint8_t* mask;  const int* cu_q; };   // [nq][nk] bytes or null | varlen: [B + 1] untrusted token offsets
    union { long long mask_bh;    struct { int total_q, total_k; }; };   // elements between the masks of consecutive (b,h): 0 = shared
    union { const uint8_t* bmask; const int* cu_k; };   // [nbr][nbc] bytes or null
    union { struct { int br, bc, nbc; }; struct { int sq, sk, sv; }; };   // varlen: token strides of q, k, v (elements)
    float p_drop, keep_scale;   // keep_scale = 1 / (1 - p)
    unsigned drop_thr;          // keep iff the element's 16 uniform bits are >= drop_thr = floor(65536 p) + 1
    unsigned nqh;               // ceil(nq / 2): row pairs per (b,h)
    unsigned long long seedmix; // seed * G + G
    float scale;
    unsigned kvg;          // kv_magic(query heads per K/V head g): K / V rows of unit bh / g (dK / dV: of bh, the per-head partials)
};
// (the varlen fields moved nothing: the offsets every kernel without them loads from)
static_assert(offsetof(ExParams, mask) == 32 && offsetof(ExParams, mask_bh) == 40 && offsetof(ExParams, bmask) == 48 &&
              offsetof(ExParams, br) == 56 && offsetof(ExParams, p_drop) == 68 && sizeof(ExParams) == 104, "ExParams layout");
constexpr int kWinNone = 1 << 30;

// Score modifiers (softcap, ALiBi: ExArgs; the kFeatScore instantiations of fa_ex_mfma.hip and the *_score_kernel entries of
// fa_ex.hip).  A kernel parameter block of their own, ExParamsS = ExParams + ExScore: the kernels without a modifier keep
// ExParams, and with it their kernel-argument layout and their code.
struct ExScore {
    const float* alibi;    // null: no ALiBi; unit u: alibi[(u / al_heads) * al_bstride + u % al_heads]
    int al_heads, al_bstride;
    float softcap;         // > 0: on (the exact-f32 kernels: softcap tanh(x / softcap) of x = scale q.k)
    // the 16-bit kernels work on raw scores S = q.k with scale log2(e) folded into exp2, so the modifier is applied in that
    // domain: S~ = cap_a tanh(S / (scale softcap)) ... = cap_a (1 - 2 / (2^(cap_k S) + 1)) - al_k slope |i + coff - j|
    float cap_k;           // 2 log2(e) scale / softcap
    float cap_a;           // softcap / scale
    float al_k;            // 1 / scale
};
struct ExParamsS : ExParams {
    ExScore sc;
};
static_assert(sizeof(ExScore) == 32 && sizeof(ExParamsS) == sizeof(ExParams) + sizeof(ExScore), "ExParamsS layout: ExScore after every ExParams field");

// Attention sinks (ExArgs; the *_sink_kernel forward entries of fa_ex.hip and fa_ex_mfma.hip, FEAT bit 5): a parameter block of
// their own again, ExParamsK = ExParamsS + ExSink, so that every other kernel keeps its block and its code.  A sink call always
// takes the score-modifier body (cap_a = 0 and alibi = null are run-time no-ops there).
struct ExSink {
    const float* sinks;    // unit u: sinks[u % heads] (natural-log units; -inf = none)
    int heads, pad_;
};
struct ExParamsK : ExParamsS {
    ExSink snk;
};
static_assert(sizeof(ExSink) == 16 && sizeof(ExParamsK) == sizeof(ExParamsS) + sizeof(ExSink), "ExParamsK layout: ExSink after every ExParamsS field");
// this unit's sink logit: uniform over the workgroup (a scalar load)
__device__ __forceinline__ float ex_sink(const ExSink& sk, int bh) { return sk.sinks[bh % sk.heads]; }
// The row normaliser with the sink column.  In: m = the row's running max in natural-log units (-inf: no visible key), l = the sum
// of exp(s - m) over the visible keys (0 then), snk = the sink logit (not -inf: the caller keeps the sink-free formulas for that,
// bit for bit).  With m' = max(m, snk): l' = l exp(m - m') + exp(snk - m') >= 1, never exp(snk - m) itself, so a sink of +-1e4 is
// safe.  Out: the factor for the unnormalised accumulator, exp(m - m') / l' (0 for a row without a visible key: o = 0), and
// lse = m' + log(l') (= snk exactly for such a row: l' = 1).
__device__ __forceinline__ void ex_sink_norm(float m, float l, float snk, float& inv, float& lse) {
    const float mp = fmaxf(m, snk);
    const float a = l > 0.f ? expf(m - mp) : 0.f;
    const float lp = fmaf(l, a, expf(snk - mp));
    inv = a / lp;
    lse = mp + logf(lp);
}

// An additive bias on the scores (fa_ex_*_bias; the kFeatBias instantiations of fa_ex_mfma_bias.hip): one more parameter block of
// its own, ExParamsB = ExParamsS + ExBias (the bias joins on the score-modifier body, where ALiBi joins), so every other kernel
// keeps its block and its code.  Unit u = b * heads + h reads bias + b * b_bs + h * b_hs + i * b_rs + j (elements, 0 = broadcast)
// and the dQ kernel stores its 16-bit dS at ds + b * s_bs + h * s_hs + i * s_rs + j where ds is not null.
struct ExBias {
    const uint16_t* bias;
    uint16_t* ds;
    long long b_bs, b_hs, s_bs, s_hs;
    int b_rs, s_rs;
    int heads;
    float inv_scale;       // 1 / scale: the kernels work on raw scores q.k, so the bias enters as fma(bias, 1 / scale, q.k)
};
struct ExParamsB : ExParamsS {
    ExBias bs;
};
static_assert(sizeof(ExBias) == 64 && sizeof(ExParamsB) == sizeof(ExParamsS) + sizeof(ExBias), "ExParamsB layout: ExBias after every ExParamsS field");

// Paged K/V for the varlen forward (fa_ex_forward_varlen_paged; the kFeatPaged instantiations of fa_ex_mfma.hip and the
// ex_fwd_varlen_paged_kernel entries of fa_ex.hip): k and v are pools (num_blocks, ps, heads_kv, d) and key t of sequence b is row
// t % ps of page table[b * max_blocks + t / ps].  Once more a parameter block of its own, ExParamsPg<B> = B + ExPage for B any of
// the three blocks above, so every other kernel keeps its block and its code.  nk is then the host's cap on a sequence's keys,
// min(max_seqlen_k, max_blocks * ps); sk, sv stay the token strides inside a page; total_k is not used.
struct ExPage {
    const int* table;      // (batch, max_blocks) untrusted page numbers: one outside [0, num_blocks) reads as zero K and V
    long long kps, vps;    // page strides of the K and the V pool (elements): page offsets are 64-bit
    int max_blocks, num_blocks;
    int ps;                // tokens per page, a multiple of 16 up to 2^16
    unsigned ps16m;        // ceil(2^32 / (ps / 16)), 0 for ps = 16: t / ps = umulhi(t / 16, ps16m), exact for t < 2^24
};
template <typename B> struct ExParamsPg : B {
    ExPage pg;
};
static_assert(sizeof(ExPage) == 40 && sizeof(ExParamsPg<ExParamsK>) == sizeof(ExParamsK) + sizeof(ExPage), "ExParamsPg layout: ExPage after every other field");
// An e4m3 pool under the paged varlen forward (fa_ex_forward_varlen_paged_fp8; the kernels of fa_ex_mfma_kv8.hip and the
// ex_fwd_varlen_paged_kernel instantiations of fa_ex.hip with this block): k and v address bytes, sk / sv / kps / vps are in
// bytes, and a stored byte c of K head hk of sequence b stands for e4m3(c) * kd[b * bs + hk] (V: vd), null = 1.0.  One more
// block of its own, ExParamsPg8<B> = ExParamsPg<B> + ExKv8, so every other kernel keeps its block and its code.
struct ExKv8 {
    const float *kd, *vd;  // (batch, heads_kv) at batch stride bs (0: one row for every sequence), or null
    long long bs;
};
template <typename B> struct ExParamsPg8 : ExParamsPg<B> {
    ExKv8 q8;
};
static_assert(sizeof(ExKv8) == 24 && sizeof(ExParamsPg8<ExParamsK>) == sizeof(ExParamsPg<ExParamsK>) + sizeof(ExKv8), "ExParamsPg8 layout: ExKv8 after every other field");
// the two scales of (sequence b, K/V head hk): uniform over the workgroup (scalar loads)
__device__ __forceinline__ float kv8_scale(const float* sc, long long bs, int b, int hk) { return sc ? sc[(long long)b * bs + hk] : 1.0f; }
// 8 e4m3 bytes -> 8 values of q's 16-bit dtype, exact (every finite e4m3 value is a normal f16 and bf16 number): one
// v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1.0 per pair, element order kept (fa_decode.hip widens its cache with it as well)
template <typename Tag> __device__ __forceinline__ u32x4 kv_q8_widen(u32x2 c);
template <> __device__ __forceinline__ u32x4 kv_q8_widen<f16_tag>(u32x2 c) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    u32x4 out;
    out[0] = __builtin_bit_cast(uint32_t, (h2)__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], 1.0f, false));
    out[1] = __builtin_bit_cast(uint32_t, (h2)__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], 1.0f, true));
    out[2] = __builtin_bit_cast(uint32_t, (h2)__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], 1.0f, false));
    out[3] = __builtin_bit_cast(uint32_t, (h2)__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], 1.0f, true));
    return out;
}
template <> __device__ __forceinline__ u32x4 kv_q8_widen<bf16_tag>(u32x2 c) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    u32x4 out;
    out[0] = __builtin_bit_cast(uint32_t, (b2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], 1.0f, false));
    out[1] = __builtin_bit_cast(uint32_t, (b2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], 1.0f, true));
    out[2] = __builtin_bit_cast(uint32_t, (b2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], 1.0f, false));
    out[3] = __builtin_bit_cast(uint32_t, (b2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], 1.0f, true));
    return out;
}

// page slot t / ps of key t (uniform where t is)
__device__ __forceinline__ int pg_slot(const ExPage& pg, int t) {
    return pg.ps16m ? (int)__umulhi((unsigned)t >> 4, pg.ps16m) : (t >> 4);
}
// keys of sequence b of a paged call: only the difference of its two offsets means anything; clamped to [0, cap]
__device__ __forceinline__ int paged_len(const int* cu, int b, int cap) {
    const long long n = (long long)cu[b + 1] - (long long)cu[b];
    return (int)min(max(n, 0ll), (long long)cap);
}

// this unit's slope (0 without ALiBi): uniform over the workgroup
__device__ __forceinline__ float ex_slope(const ExScore& sc, int bh) {
    return sc.alibi ? sc.alibi[(bh / sc.al_heads) * sc.al_bstride + bh % sc.al_heads] : 0.f;
}

// Score modifiers on a raw score S of the 16-bit kernels (fa_ex_mfma.hip FEAT bit 4, fa_decode.hip) (ExScore): the softcap as
//   S~ = cap_a t,  t = tanh(S / (scale softcap)) = 1 - 2 r,  r = 1 / (2^(cap_k S) + 1)
// (two transcendentals; safe at both ends: 2^x = inf gives r = 0, t = 1; 2^x = 0 gives r = 1, t = -1), and its derivative
// dt = 1 - t^2 = 4 r (1 - r) for the backward.  The forward and both backward kernels evaluate S~ with these same fp32 operations,
// so P in the backward is the P of the forward's lse.
__device__ __forceinline__ float mod_softcap(float s, const ExScore& sc, float& dt) {
    const float r = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(s * sc.cap_k) + 1.f);
    dt = r * fmaf(r, -4.f, 4.f);
    return fmaf(r, -2.f * sc.cap_a, sc.cap_a);
}
// ALiBi: S~ - al |dist|, al = slope / scale, dist = i + coff - j an exact small integer held as a float
__device__ __forceinline__ float mod_alibi(float s, float al, float dist) { return fmaf(-al, fabsf(dist), s); }
// first token and length of sequence b: start = clamp(cu[b], 0, total), end = clamp(cu[b + 1], start, total),
// len = min(end - start, max_len).  b is uniform over the workgroup: scalar loads.
__device__ __forceinline__ void seq_span(const int* cu, int b, int total, int max_len, int& start, int& len) {
    const int a = min(max(cu[b], 0), total);
    const int e = min(max(cu[b + 1], a), total);
    start = a;
    len = min(e - a, max_len);
}
// bytes of a buffer range that covers rows [0, n) of d 16-bit elements, `stride` elements apart (0 rows: nothing)
__device__ __forceinline__ unsigned span_bytes(int n, int d, int stride) { return n > 0 ? (unsigned)((n - 1) * stride + d) * 2u : 0u; }

// Dropout generator: ONE splitmix64 value per 2 x 2 quad of (query row, key) elements, 16 uniform bits per element — the
// 64-bit mixing (two 64 x 64 multiplies) is the expensive part on a GPU, and in every kernel a lane owns either two
// neighbouring keys of one row or two neighbouring rows of one key, so a lane uses two fields of each value it makes.
//   counter = (bh * ceil(nq / 2) + row / 2) << 32 | key / 2 ;   z = splitmix64(counter + seed * G + G)
//   field   = 2 * (row & 1) + (key & 1) ;   u = (z >> 16 field) & 0xffff ;   keep iff u >= floor(65536 p) + 1
// The oracle (oracle/attention_oracle.py: dropout_keep) runs the same arithmetic on uint64, so the masks agree bit for bit.
__device__ __forceinline__ unsigned long long ex_hash(unsigned hi, unsigned lo, unsigned long long seedmix) {
    unsigned long long z = (((unsigned long long)hi << 32) | lo) + seedmix;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ bool ex_keep(const ExParams& p, int bh, int row, int key) {
    if (p.p_drop <= 0.f) return true;
    const unsigned long long z = ex_hash((unsigned)bh * p.nqh + ((unsigned)row >> 1), (unsigned)key >> 1, p.seedmix);
    const unsigned u = (unsigned)(z >> (16 * (2 * (row & 1) + (key & 1)))) & 0xffffu;
    return u >= p.drop_thr;
}
// WIN: the call has a window (a separate instantiation: calls without one run the code they ran before it existed)
// VAR: a varlen call (no masks: their fields hold the sequence offsets)
template <bool WIN, bool VAR = false>
__device__ __forceinline__ bool ex_visible(const ExParams& p, int bh, int row, int key) {
    if (row >= p.nq || key >= p.nk) return false;
    if (p.causal && key > row + p.coff) return false;
    if (WIN && (key > row + p.coff + p.wr || key < row + p.coff - p.wl)) return false;   // (wr = 0 under the causal flag)
    if (!VAR && p.mask && p.mask[(size_t)bh * p.mask_bh + (size_t)row * p.nk + key] == 0) return false;
    if (!VAR && p.bmask && p.bmask[(row / p.br) * p.nbc + key / p.bc] == 0) return false;
    return true;
}
// does the block-sparse mask leave anything of rows [r0, r1) x keys [k0, k1)?  (uniform over the workgroup)
__device__ __forceinline__ bool ex_tile_live(const ExParams& p, int r0, int r1, int k0, int k1) {
    if (!p.bmask) return true;
    for (int rb = r0 / p.br; rb <= (r1 - 1) / p.br; ++rb)
        for (int cb = k0 / p.bc; cb <= (k1 - 1) / p.bc; ++cb)
            if (p.bmask[rb * p.nbc + cb]) return true;
    return false;
}

// Paged staging of one K tile and one V tile (the varlen forward of fa_ex_mfma.hip with kFeatPaged), in place of two
// dma_stage_tile calls.  The LDS image, the pieces (1 KiB = RPP = 512 / D rows, wave w issues pieces w, w + NW, ..) and the lane
// offsets inside a piece (dma_lane_voff with the pool's token stride) are dma_stage_tile's.  A piece starts at key row0 + RPP * pc,
// row0 a multiple of ROWS = 128 and RPP * pc a multiple of RPP <= 8, and a page holds a multiple of 16 keys: no piece straddles a
// page, so one wave-uniform table entry (a scalar load) serves a piece, K and V alike.  Instead of a 32-bit soffset from the
// tensor's start each piece gets a descriptor of its own: the 64-bit address of its first row, and as num_records the bytes of
// its rows below nk — 0 for a piece past the sequence or on a page outside the pool, whose lanes all fail the range check and
// land as zeros, as the rows past a packed tensor's end do.  Never a branch around the DMA: the image is always fully written.
// The descriptor words are SGPRs written right before dma16_issue, whose s_mov m0 + s_nop 3 are the five wait states a buffer
// instruction needs after a v_readfirstlane wrote one of its SGPR operands.
// trow: the sequence's table row; last = pg_slot(nk - 1) bounds the slot, so no entry past ceil(nk / ps) is read.
template <int D, int ROWS, int NW>
__device__ __forceinline__ void dma_stage_kv_paged(const ExPage& pg, const int* __restrict__ trow, int last, const uint16_t* kh,
                                                   const uint16_t* vh, char* ktile, char* vtile, int row0, int nk, int voff_k,
                                                   int voff_v, int w, int dr, int sk, int sv) {
    constexpr int RPP = 512 / D, PIECES = ROWS / RPP, PER_WAVE = PIECES / NW;
    static_assert(PIECES % NW == 0 && (RPP * NW) % 16 == 0 && 16 % RPP == 0, "pieces: whole per wave, one swizzle class, inside a page");
    const unsigned tk = lds_addr_of(ktile), tv = lds_addr_of(vtile);
#pragma unroll
    for (int j = 0; j < PER_WAVE; ++j) {
        const int pc = w + NW * j;
        const int key = __builtin_amdgcn_readfirstlane(row0 + RPP * pc);
        const int rows = min(RPP, nk - key);                 // <= 0: the piece lies past the sequence
        const int slot = min(pg_slot(pg, key), last);
        const int page = trow[slot];
        const bool ok = rows > 0 && (unsigned)page < (unsigned)pg.num_blocks;
        const long long inpage = key - slot * pg.ps;
        const long long ko = ok ? (long long)page * pg.kps + inpage * sk : 0ll;
        const long long vo = ok ? (long long)page * pg.vps + inpage * sv : 0ll;
        dma16_issue(make_rsrc_s(kh + ko, ok ? span_bytes(rows, dr, sk) : 0u), tk + pc * 1024, voff_k, 0);
        dma16_issue(make_rsrc_s(vh + vo, ok ? span_bytes(rows, dr, sv) : 0u), tv + pc * 1024, voff_v, 0);
    }
}

// The same for an e4m3 pool (kFeatKv8): the DMA moves the pool's bytes into a staging area and the waves widen them into the 16-bit
// tile image afterwards (kv8_widen_block).  Wave w owns the 16 keys row0 + 16 w .. + 15 of the tile, K and V alike: 16 keys never
// straddle a page (a page holds a multiple of 16), so ONE table entry and one descriptor per tensor serve the wave's block, whose
// num_records are the bytes of its rows below nk (0: past the sequence or a page outside the pool, everything lands as zeros).  The
// block moves as 16 D / 256 buffer_load_dword .. lds of 256 bytes each: dword granularity, because an e4m3 head row of d bytes
// (d % 8 == 0, the pool 8-byte aligned) starts on an 8-byte boundary only and the range check cuts a row at d, which a 16-byte
// piece does neither.  Lane l of instruction j fetches bytes 4 (l % (D / 4)) .. + 3 of row (256 / D) j + l / (D / 4), so the staged
// block is row-major [16][D] bytes; the columns past dr are requested at kOobOff and land as zeros.
template <int D>
__device__ __forceinline__ int dma_lane_voff8(int lane, int dr, int stride) {
    constexpr int LPR = D / 4;   // lanes per row
    const int rl = lane / LPR, c = lane - rl * LPR;
    return 4 * c < dr ? rl * stride + 4 * c : kOobOff;
}
// one tensor's share of a block: its descriptor, then the 16 D / 256 loads.  The LDS address and the row offset (soffset) walk
// from values made opaque per call: left to hipcc they are hoisted out of the key loop as 2 * 16 D / 256 scalar registers per
// tensor, which the scalar file does not have (they came back as SGPRs spilled to VGPR lanes)
template <int D>
__device__ __forceinline__ void dma_stage_block8(const char* base, long long off, unsigned bytes, unsigned lds, int voff, int stride) {
    constexpr int RPI = 256 / D, NI = 16 / RPI;   // rows per instruction, instructions per block
    const rsrc_s_t rs = make_rsrc_s(base + off, bytes);
    int soff = 0;
    asm volatile("" : "+s"(lds), "+s"(soff));
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        dma4_issue(rs, lds, voff, soff);
        lds += 256;
        soff += RPI * stride;
    }
}
// (K's loads are all issued before V's descriptor is made: one descriptor's four scalar registers live at a time)
template <int D, int ROWS, int NW>
__device__ __forceinline__ void dma_stage_kv_paged8(const ExPage& pg, const int* __restrict__ trow, int last, const char* kh, const char* vh,
                                                    char* kstage, char* vstage, int row0, int nk, int voff_k, int voff_v, int w, int dr,
                                                    int sk, int sv) {
    static_assert(ROWS == 16 * NW, "one block of 16 keys per wave");
    const int key = __builtin_amdgcn_readfirstlane(row0 + 16 * w);
    const int rows = min(16, nk - key);                  // <= 0: the block lies past the sequence
    const int slot = min(pg_slot(pg, key), last);
    const int page = trow[slot];
    const bool ok = rows > 0 && (unsigned)page < (unsigned)pg.num_blocks;
    const long long inpage = key - slot * pg.ps;
    dma_stage_block8<D>(kh, ok ? (long long)page * pg.kps + inpage * sk : 0ll, ok ? (unsigned)((rows - 1) * sk + dr) : 0u,
                        lds_addr_of(kstage) + w * 16 * D, voff_k, sk);
    dma_stage_block8<D>(vh, ok ? (long long)page * pg.vps + inpage * sv : 0ll, ok ? (unsigned)((rows - 1) * sv + dr) : 0u,
                        lds_addr_of(vstage) + w * 16 * D, voff_v, sv);
}
// Wave w widens the block it staged (after the caller's vmcnt(0) and barrier; no other wave touches these bytes) into rows
// 16 w .. 16 w + 15 of the TileSwz<D> image: 8 bytes in, one 16-byte chunk out, chunk i * 64 + lane of the block's 2 D.
template <typename Tag, int D>
__device__ __forceinline__ void kv8_widen_block(const char* stage, char* tile, int w, int lane) {
    constexpr int CPR = D / 8, PER_LANE = 16 * CPR / 64;
    const char* src = stage + w * 16 * D + 8 * lane;
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int idx = i * 64 + lane, row = idx / CPR, ch = idx - row * CPR;
        const u32x2 c = *reinterpret_cast<const u32x2*>(src + i * 512);
        *reinterpret_cast<u32x4*>(tile + TileSwz<D>::off(16 * w + row, ch)) = kv_q8_widen<Tag>(c);
    }
}

inline ExParams make_ex_params(const ExArgs& a) {
    ExParams p;
    p.nq = (int)a.nq; p.nk = (int)a.nk; p.d = (int)a.d;
    p.causal = a.causal ? 1 : 0;
    p.coff = (int)(a.nk - a.nq);
    p.mask = a.mask; p.mask_bh = a.mask_bh_stride;
    p.bmask = a.block_mask; p.br = (int)(a.br > 0 ? a.br : 1); p.bc = (int)(a.bc > 0 ? a.bc : 1);
    p.nbc = (int)((a.nk + p.bc - 1) / p.bc);
    p.p_drop = (float)a.dropout_p;
    p.keep_scale = a.dropout_p > 0.0 ? (float)(1.0 / (1.0 - a.dropout_p)) : 1.f;
    const double t = a.dropout_p * 65536.0;
    p.drop_thr = a.dropout_p > 0.0 ? (unsigned)((long long)t + 1) : 0u;   // floor(65536 p) + 1 <= 65536
    p.nqh = (unsigned)((a.nq + 1) / 2);
    p.seedmix = a.seed * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    p.scale = a.scale;
    p.kvg = kv_magic(a.kv_group);
    p.wl = a.window_left >= 0 ? (int)a.window_left : kWinNone;
    p.wr = a.causal ? 0 : (a.window_right >= 0 ? (int)a.window_right : kWinNone);
    p.hq = 0;
    if (a.cu_q) {   // varlen (no masks): the mask fields hold the sequences
        p.hq = (int)a.heads_q;
        p.cu_q = a.cu_q; p.cu_k = a.cu_k;
        p.total_q = (int)a.total_q; p.total_k = (int)a.total_k;
        p.sq = (int)a.stride_q; p.sk = (int)a.stride_k; p.sv = (int)a.stride_v;
    }
    return p;
}
inline ExParamsS make_ex_params_s(const ExArgs& a) {
    ExParamsS p;
    static_cast<ExParams&>(p) = make_ex_params(a);
    p.sc.alibi = a.alibi;
    p.sc.al_heads = (int)(a.alibi_heads > 0 ? a.alibi_heads : 1);
    p.sc.al_bstride = (int)a.alibi_bstride;
    const double cap = a.softcap > 0.0 ? a.softcap : 0.0, sc = a.scale;
    p.sc.softcap = (float)cap;
    p.sc.cap_k = cap > 0.0 ? (float)(2.0 * 1.4426950408889634 * sc / cap) : 0.f;
    p.sc.cap_a = cap > 0.0 ? (float)(cap / sc) : 0.f;
    p.sc.al_k = (float)(1.0 / sc);
    return p;
}
inline ExParamsK make_ex_params_k(const ExArgs& a) {
    ExParamsK p;
    static_cast<ExParamsS&>(p) = make_ex_params_s(a);
    p.snk.sinks = a.sinks;
    p.snk.heads = (int)(a.sink_heads > 0 ? a.sink_heads : 1);
    p.snk.pad_ = 0;
    return p;
}

inline ExBias make_ex_bias(const ExArgs& a) {
    ExBias b;
    b.bias = reinterpret_cast<const uint16_t*>(a.bias);
    b.ds = reinterpret_cast<uint16_t*>(a.dbias);
    b.b_bs = a.bias_bstride; b.b_hs = a.bias_hstride; b.s_bs = a.dbias_bstride; b.s_hs = a.dbias_hstride;
    b.b_rs = (int)a.bias_rstride; b.s_rs = (int)a.dbias_rstride;
    b.heads = (int)(a.bias_heads > 0 ? a.bias_heads : 1);
    b.inv_scale = (float)(1.0 / (double)a.scale);
    return b;
}

inline ExPage make_ex_page(const ExArgs& a) {
    ExPage g;
    g.table = a.block_table;
    g.kps = a.page_stride_k; g.vps = a.page_stride_v;
    g.max_blocks = (int)a.max_blocks; g.num_blocks = (int)a.num_blocks;
    g.ps = (int)a.page_size;
    g.ps16m = kv_magic(a.page_size / 16);
    return g;
}
inline ExKv8 make_ex_kv8(const ExArgs& a) { return ExKv8{a.k_descale, a.v_descale, (long long)a.descale_bstride}; }

}  // namespace fa
