// Multi-head latent attention at decode time: KV-cache decoding with a second query operand and K and V of different widths
// (fa_ex_forward_kvcache_qv; FlashAttention-3's qv), over a per-query list of cached tokens (fa_mla_sparse_forward), and over
// FlashMLA's packed 8-bit latent cache (fa_mla_fp8_forward, fa_mla_fp8_pack).  Every cached token is a 64-wide rotary row k and a
// 512-wide latent row v; for query head h reading K/V head hk = h / G
//   s[i, j] = scale * (q[i, h, :] . k[j, hk, :] + qv[i, h, :] . v[j, hk, :]),   o[i, h, :] = sum_j softmax_j(s)[i, j] v[j, hk, :]
// so the latent row is the score operand and the value operand.  It is fetched from memory once per workgroup.
//
// One kernel text, mla_decode, in three shells.  A workgroup has NW waves (1 | 2 | 4), each with a tile of 16 query rows.  Per
// tile of 32 keys the workgroup copies the 32 x 512 latent rows and the 32 x 64 rotary rows into LDS (36 KiB, 16 bytes a lane and
// step, through registers; with four waves the loads of tile t + 1 are issued before tile t is computed on), the latent in the
// swizzled image MlaSwz.  mla_tile_step: S^T = K Q^T reads that image row-wise (ds_read_b128: 8 consecutive head dims a lane,
// 2 + 16 k-steps of v_mfma_f32_16x16x32 per 16 keys against the q and qv fragments the wave keeps in registers); O^T = V^T P^T
// reads the same bytes transposed (ds_read_b64_tr_b16), 32 MFMAs into a 16 x 512 fp32 accumulator.  Online softmax in fp32 on the
// lane of its query row, as in kv_split_kernel.  mla_epilogue: o and lse (S == 1) or the fp32 partials of a split, which meet in
// mla_combine_kernel (kv_combine_kernel with a loop over the two 256-column halves of a 512-wide row) in the fixed split order.
//
// What differs between the forms is who names a tile's keys and how a key's bytes reach LDS; each piece is written once:
//   keys    MlaDenseKeys  the keys [kbeg, kend) of a split (kv_split_range: the union of the workgroup's rows' bands; every row
//                         masks its own band), contiguous or through the page table.  Row = token * G + head, the mapping of
//                         kv_split_kernel; lengths, pages and cache rows follow fa_decode.hip (fa_decode_common.h).
//           MlaListKeys   the topk entries of the list of a (sequence, query token, K/V head); a workgroup serves one list and
//                         its rows are the G heads.  The mask is the tile's ballot of the per-entry visibility flag.
//           Both hand out, per lane, the key's page (or cache row) and its slot there, or "not fetched".
//   copy    MlaCopy16Contig  16-bit caches, contiguous: buffer loads with the bound in the descriptor
//           MlaCopy16At      16-bit caches by per-key offset (paged dense, every list): v_readlane for the latent row's base
//           MlaCopyF8        the packed token: scales and e4m3 chunks, widened to the same bf16 image (mla_f8_widen)
//   shell   mla_split_kernel<Tag, NW, PAGED>   MlaDenseKeys + (PAGED ? MlaCopy16At : MlaCopy16Contig)
//           mla_sparse_kernel<Tag, NW, PAGED>  MlaListKeys  + MlaCopy16At
//           mla_f8_kernel<NW, SPARSE>          (SPARSE ? MlaListKeys : MlaDenseKeys), paged, + MlaCopyF8; bf16 only
// From the barrier after the copy on every form runs the same instructions on the same LDS image, so a call on a packed pool gives
// the bits of the 16-bit call on the pool's dequantised rows, and a paged call those of the contiguous call on the gathered tokens.
//
// Small launches: the wave count follows the packed rows (mla_waves: 16 rows -> one wave a workgroup), so no wave of a
// workgroup is without rows unless the last row tile of a larger call is; the launch rule (mla_num_splits) then cuts the keys
// into more splits.  That is the merge a workgroup-internal key split would need a second, LDS-resident copy of; here it is the
// one the split path already has.
#include "fa_decode_common.h"
#include <algorithm>
#include <type_traits>

namespace fa {

namespace {

constexpr int kMlaDk = 64, kMlaDv = 512, kMlaKT = 32;
constexpr int kMlaLatBytes = kMlaKT * kMlaDv * 2, kMlaLdsBytes = kMlaLatBytes + kMlaKT * kMlaDk * 2;

// the latent tile [32][512]: 1024-byte rows, the 16-chunk pattern of TileSwz<256> repeating (a chunk's bank is its index mod 16)
struct MlaSwz {
    static __device__ __forceinline__ int off(int row, int ch) { return 1024 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
};

struct MlaParams {
    KvParams p;            // p.d = 64: q, k_cache; v_cache, o and the partials are 512 wide
    const uint16_t* qv;    // (batch, nq, hq, 512): batch stride qv_bs, token stride qv_ts
    long long qv_bs;
    int qv_ts;
};

// Sparse form: the keys of a (sequence b, query token i, K/V head hk) are the topk entries of a list of token positions.  An
// entry is visible if 0 <= entry < len_b (and <= len_b - nq + i if causal).  An entry that is not visible is never turned into
// an address: its row is zeros in LDS and its score is -inf.  A visible entry on a page outside the pool or in a cache row outside
// the cache is a zero row too, with score 0 (the page rule of fa_decode.hip).  Splits cut the list positions [0, topk) into
// ranges of whole tiles.
struct MlaSparseParams {
    MlaParams mp;          // mp.p.nq: the query tokens of a sequence (the window fields are not used)
    const int* idx;        // entry j of (b, i, hk): idx[b * ix_bs + i * ix_ts + hk * ix_hs + j]; untrusted device memory
    long long ix_bs, ix_ts, ix_hs;
    int topk, causal;
};

// The packed 8-bit latent cache: FlashMLA's 656-byte token
//   byte 0 .. 511: 512 e4m3 (the latent, quantised per 128-wide tile) | 512 .. 527: 4 float32 scales | 528 .. 655: 64 bf16 (rotary)
// in a paged pool, token t of sequence b at pool + page * page_sb + (t % ps) * tok_sb bytes (64-bit), one K/V head, bf16 only.
constexpr int kF8Scales = 512, kF8Rope = 528;   // byte offsets in a token (656 bytes)

struct MlaF8Params {
    MlaSparseParams sp;    // sp.mp.p.kc / vc are not used; sp.idx, topk: SPARSE only
    const unsigned char* pool;
    long long page_sb;     // bytes from page to page
    int tok_sb;            // bytes from token to token of a page
    int q_hs, qv_hs;       // head strides of q and qv (elements): the two column ranges of one (.., 576) tensor are 576 apart
};

// ---- keys.  What mla_decode reads of either producer: the workgroup's sequence b, split s of S and positions [kbeg, kend) (keys,
// or list positions); this wave's row tile (active; none: the wave only copies) and this lane's query row (valid), its query token
// qi and head h.  start() does the first lookups, next(kt, unit, slot) gives this lane's key kt + (lane & 31) of the tile at kt as
// the page (or cache row) it is in and its slot there, unit = -1: not fetched, and moves on; it returns the tile's flags for mask().
struct MlaRows {
    int b, s, S, kbeg, kend, qi, h;
    bool active, valid;
};

// register i of score block kb holds position k0 + 16 kb + 4 g + i: inside the row's band
struct MlaBandMask {
    int k0, g, rlo, rhi;
    __device__ __forceinline__ bool operator()(int kb, int i) const {
        const int key = k0 + 16 * kb + 4 * g + i;
        return key >= rlo && key <= rhi;
    }
};

// ... or flagged visible in the list: bit k of the tile's flags is list position k0 + k
struct MlaFlagMask {
    unsigned vg;
    __device__ __forceinline__ bool operator()(int kb, int i) const { return (vg >> (16 * kb + i)) & 1u; }
};

// Dense: grid (split, row tiles of 16 NW rows x K/V heads, sequence).  PAGED: kv_split_kernel's lookup, done by every wave for
// itself, the next tile's a tile ahead of its use.  Contiguous: the copy takes the key from kt itself, there is nothing to hand out.
template <int NW, bool PAGED>
struct MlaDenseKeys : MlaRows {
    const KvParams& p;
    const int* tbl;
    int lane, rlo, rhi, j0 = 0, s0 = 0, pg = -1;

    __device__ __forceinline__ MlaDenseKeys(const KvParams& p_, int hk, int wt) : p(p_) {
        lane = threadIdx.x & 63;
        const int w = threadIdx.x >> 6, r = lane & 15;
        s = blockIdx.x, S = gridDim.x, b = blockIdx.z;
        const int nq = p.nq, rows = p.rows;
        int L_b, P_b;
        const int lk = kv_len_k(p, b, 0, L_b, P_b), coff = lk - nq;
        // the workgroup's rows [wr0, wr1) and the key range of their bands' union; wr0 < rows by the grid
        const int wr0 = 16 * NW * wt, wr1 = min(wr0 + 16 * NW, rows);
        kv_split_range(p, lk, nq, wr0 / p.G, (wr1 - 1) / p.G, s, S, kbeg, kend);
        // this wave's row tile, this lane's query row and its visible keys [rlo, rhi]
        const int pr0 = wr0 + 16 * w, pr = pr0 + r;
        active = pr0 < rows, valid = pr < rows;
        const int qlo = min(pr0, rows - 1) / p.G;
        qi = valid ? pr / p.G : qlo;
        h = hk * p.G + (valid ? pr - qi * p.G : 0);
        rlo = max(qi + coff - p.wl, kbeg);
        rhi = valid ? min(min(qi + coff + p.wr, lk - 1), kend - 1) : -1;
        tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    }
    __device__ __forceinline__ int page_of(int jt, int st, int kt) const {
        int j = jt, sl = st + (lane & 31);
        if (sl >= p.ps) { sl -= p.ps; ++j; }
        if (sl >= p.ps) ++j;
        return kt + (lane & 31) < kend ? tbl[j] : -1;
    }
    __device__ __forceinline__ void start() {
        if (PAGED && kbeg < kend) {
            j0 = kbeg / p.ps;
            s0 = kbeg - j0 * p.ps;
            pg = page_of(j0, s0, kbeg);
        }
    }
    // a key past the split's end or on a page outside the pool is not fetched
    __device__ __forceinline__ unsigned next(int kt, int& unit, int& slot) {
        unit = -1, slot = 0;
        if constexpr (PAGED) {
            int sl = s0 + (lane & 31);
            if (sl >= p.ps) sl -= p.ps;
            if (sl >= p.ps) sl -= p.ps;
            slot = sl;
            if ((unsigned)pg < (unsigned)p.nblk) unit = pg;
            s0 += kMlaKT;
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (kt + kMlaKT < kend) pg = page_of(j0, s0, kt + kMlaKT);   // the next tile's lookup, a tile ahead of its use
        }
        return 0u;
    }
    __device__ __forceinline__ MlaBandMask mask(int k0, unsigned, int g) const { return MlaBandMask{k0, g, rlo, rhi}; }
};

// Lists: grid (list = b * nq + i, split, row tiles of 16 NW heads x K/V heads).  The pipeline of lane l (list position + (l & 31)
// of a tile): e2 the raw entry of the tile after next, one coalesced 128-byte read two tiles ahead of its use; s1 the next tile's
// visible entry as its token position (contiguous) or its slot in its page pg1 (paged), -1 = not visible, decided a tile ahead.
template <int NW, bool PAGED>
struct MlaListKeys : MlaRows {
    const KvParams& p;
    const int *tbl, *il;
    unsigned tlim;
    int lane, crow, e2 = -1, s1 = -1, pg1 = -1;

    __device__ __forceinline__ MlaListKeys(const MlaSparseParams& sp, int hk, int wt) : p(sp.mp.p) {
        constexpr int KT = kMlaKT;
        lane = threadIdx.x & 63;
        const int w = threadIdx.x >> 6, r = lane & 15;
        s = blockIdx.y, S = gridDim.y;
        const int nq = p.nq;
        b = blockIdx.x / nq, qi = blockIdx.x - b * nq;
        int L_b, P_b;
        const int lk = kv_len_k(p, b, 0, L_b, P_b);
        // visible token positions: [0, tlim)
        const int thi = sp.causal ? lk - nq + qi : lk - 1;
        tlim = thi >= 0 ? (unsigned)thi + 1u : 0u;
        // list positions [kbeg, kend) of split s: whole tiles
        const int nt = (sp.topk + KT - 1) / KT;
        kbeg = (int)((long long)s * nt / S) * KT, kend = min(sp.topk, (int)((long long)(s + 1) * nt / S) * KT);
        // this wave's row tile of the G heads and this lane's head
        const int pr0 = 16 * NW * wt + 16 * w, pr = pr0 + r;
        active = pr0 < p.G, valid = pr < p.G;
        h = hk * p.G + (valid ? pr : 0);
        // contiguous: cache row (bidx ? bidx[b] : b); a row outside the cache holds zero rows
        crow = b;
        if (!PAGED && p.bidx) {
            const int ix = p.bidx[b];
            crow = (unsigned)ix < (unsigned)p.bcache ? ix : -1;
        }
        tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
        il = sp.idx + b * sp.ix_bs + qi * sp.ix_ts + hk * sp.ix_hs;
    }
    __device__ __forceinline__ int entry(int jt) const {
        const int pos = jt + (lane & 31);
        return pos < kend ? il[pos] : -1;
    }
    __device__ __forceinline__ void advance(int jt) {   // e2 -> s1 (pg1); e2 = the entries of the tile at jt
        const bool vis = (unsigned)e2 < tlim;
        if constexpr (PAGED) {
            const unsigned j = (unsigned)e2 / (unsigned)p.ps;   // (< max_blocks_per_seq: e2 < len_b <= the capacity)
            s1 = vis ? (int)((unsigned)e2 - j * (unsigned)p.ps) : -1;
            pg1 = vis ? tbl[j] : -1;
        } else {
            s1 = vis ? e2 : -1;
        }
        e2 = entry(jt);
    }
    __device__ __forceinline__ void start() {
        if (kbeg < kend) {
            e2 = entry(kbeg);
            advance(kbeg + kMlaKT);
        }
    }
    __device__ __forceinline__ unsigned next(int kt, int& unit, int& slot) {
        unit = -1, slot = s1;
        if constexpr (PAGED) {
            if (s1 >= 0 && (unsigned)pg1 < (unsigned)p.nblk) unit = pg1;
        } else if (s1 >= 0 && crow >= 0) {
            unit = crow;
        }
        const unsigned vm = (unsigned)__ballot(s1 >= 0);
        advance(kt + 2 * kMlaKT);
        return vm;
    }
    __device__ __forceinline__ MlaFlagMask mask(int, unsigned vm, int g) const { return MlaFlagMask{valid ? vm >> (4 * g) : 0u}; }
};

// ---- copies.  One tile's copy, loads and LDS writes apart: place(unit, slot) takes this lane's key from the producer,
// load_lat / load_rot fetch a thread's share into registers, store_lat / mla_store_rot write it to LDS.  A key that is not fetched
// is zeros in LDS: its loads are redirected to the first bytes of q and their results selected away, no address is formed from
// the key.  Four waves: a thread holds a whole tile's share (CH == B latent chunks) and the loads of tile k0 + 32 are in flight
// while tile k0 is computed on.  Fewer waves move their CH chunks B at a time between the barriers; there the other workgroups of
// the CU cover the latency.

// 16-bit caches: chunk idx = T i + tid of the latent rows (row idx / 64 = (T / 64) i + w, the same for the whole wave; chunk
// idx % 64 = lane), 9, 18 or 36 chunks a thread with the rotary ones
template <int NW>
struct MlaCopy16 {
    static constexpr int T = 64 * NW, CH = kMlaKT * (kMlaDv / 8) / T, B = CH <= 8 ? CH : 8, RCH = kMlaKT * (kMlaDk / 8) / T;
    static_assert(CH * T == kMlaKT * kMlaDv / 8 && CH % B == 0 && RCH >= 1, "tile copy");
    const KvParams& p;
    const int hk, tid, lane, wu;
    u32x4 xl[B], xr[RCH];

    __device__ __forceinline__ MlaCopy16(const KvParams& p_, int hk_)
        : p(p_), hk(hk_), tid(threadIdx.x), lane(threadIdx.x & 63), wu(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {}
    __device__ __forceinline__ void store_lat(char* lat, int i0) const {
#pragma unroll
        for (int i = 0; i < B; ++i) *reinterpret_cast<u32x4*>(lat + MlaSwz::off((T / 64) * (i0 + i) + wu, lane)) = xl[i];
    }
};

// contiguous: cache row (bidx ? bidx[b] : b); a row outside the cache is an empty range (kv_split_kernel's rule), keys past the
// split's end are requested at kOobOff
template <int NW>
struct MlaCopy16Contig : MlaCopy16<NW> {
    using Base = MlaCopy16<NW>;
    using Base::p, Base::hk, Base::tid, Base::lane, Base::wu, Base::xl, Base::xr;
    buf_rsrc_t k_rs, v_rs;

    __device__ __forceinline__ MlaCopy16Contig(const KvParams& p_, int hk_, int b) : Base(p_, hk_) {
        long long crow = b;
        int ctok = p.cap;
        if (p.bidx) {
            const int ix = p.bidx[b];
            crow = ix;
            if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; ctok = 0; }
        }
        k_rs = make_rsrc(p.kc + crow * p.kc_bs, ctok > 0 ? (unsigned)(((ctok - 1) * p.kc_ts + p.hkv * kMlaDk) * 2) : 0u);
        v_rs = make_rsrc(p.vc + crow * p.vc_bs, ctok > 0 ? (unsigned)(((ctok - 1) * p.vc_ts + p.hkv * kMlaDv) * 2) : 0u);
    }
    __device__ __forceinline__ void place(int, int) {}
    __device__ __forceinline__ void load_lat(int kt, int kend, int i0) {
#pragma unroll
        for (int i = 0; i < Base::B; ++i) {
            const int key = kt + (Base::T / 64) * (i0 + i) + wu;
            xl[i] = __builtin_amdgcn_raw_buffer_load_b128(v_rs, key < kend ? (key * p.vc_ts + hk * kMlaDv + 8 * lane) * 2 : kOobOff, 0, 0);
        }
    }
    __device__ __forceinline__ void load_rot(int kt, int kend) {
#pragma unroll
        for (int i = 0; i < Base::RCH; ++i) {
            const int idx = Base::T * i + tid, key = kt + (idx >> 3), ch = idx & 7;
            xr[i] = __builtin_amdgcn_raw_buffer_load_b128(k_rs, key < kend ? (key * p.kc_ts + hk * kMlaDk + 8 * ch) * 2 : kOobOff, 0, 0);
        }
    }
};

// by offset: this lane's key has element offsets ko / vo in the two caches (pools), -1 = not fetched
template <int NW>
struct MlaCopy16At : MlaCopy16<NW> {
    using Base = MlaCopy16<NW>;
    using Base::p, Base::hk, Base::tid, Base::lane, Base::wu, Base::xl, Base::xr;
    static constexpr bool kPre = Base::B == Base::CH;   // the prefetch: a thread holds a whole tile's share
    long long ko = -1, vo = -1;

    __device__ __forceinline__ MlaCopy16At(const KvParams& p_, int hk_, int) : Base(p_, hk_) {}
    __device__ __forceinline__ void place(int unit, int slot) {
        ko = vo = -1;
        if (unit >= 0) {
            ko = unit * p.kc_bs + (long long)slot * p.kc_ts;
            vo = unit * p.vc_bs + (long long)slot * p.vc_ts;
        }
    }
    __device__ __forceinline__ void load_lat(int, int, int i0) {
        bool ok[Base::B];
#pragma unroll
        for (int i = 0; i < Base::B; ++i) {
            const int row = (Base::T / 64) * (i0 + i) + wu;
            const long long ro = ((long long)__builtin_amdgcn_readlane((int)(vo >> 32), row) << 32) |
                                 (unsigned)__builtin_amdgcn_readlane((int)vo, row);   // (wave-uniform: a scalar base)
            ok[i] = ro >= 0;
            xl[i] = *reinterpret_cast<const u32x4*>(ok[i] ? p.vc + ro + hk * kMlaDv + 8 * lane : p.q);
        }
        // (without the prefetch the LDS writes follow at once: every load of the batch is issued before the first select waits
        // for one; hipcc otherwise holds the last load back behind the first wait, and in load_rot waits after each)
        if constexpr (!kPre) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < Base::B; ++i) xl[i] = ok[i] ? xl[i] : u32x4{0u, 0u, 0u, 0u};
    }
    __device__ __forceinline__ void load_rot(int, int) {
        bool ok[Base::RCH];
#pragma unroll
        for (int i = 0; i < Base::RCH; ++i) {
            const int idx = Base::T * i + tid, row = idx >> 3, ch = idx & 7;
            const long long ro = __shfl(ko, row, 64);
            ok[i] = ro >= 0;
            xr[i] = *reinterpret_cast<const u32x4*>(ok[i] ? p.kc + ro + hk * kMlaDk + 8 * ch : p.q);
        }
        if constexpr (!kPre) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < Base::RCH; ++i) xr[i] = ok[i] ? xr[i] : u32x4{0u, 0u, 0u, 0u};
    }
};

// 16 e4m3 bytes times one scale -> the two 16-byte chunks of bf16 they fill
__device__ __forceinline__ void mla_f8_widen(u32x4 x, float sc, u32x4& lo, u32x4& hi) {
    uint32_t out[8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[d], false);
        const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[d], true);
        out[2 * d] = pack2<bf16_tag>(a[0] * sc, a[1] * sc);
        out[2 * d + 1] = pack2<bf16_tag>(b[0] * sc, b[1] * sc);
    }
    lo = u32x4{out[0], out[1], out[2], out[3]};
    hi = u32x4{out[4], out[5], out[6], out[7]};
}

// the packed token: row tid / TPR of the tile belongs to TPR = T / 32 threads; a thread loads the row's four scales (one 16-byte
// load) and its 16-byte chunks c = tid % TPR + TPR i of e4m3 (16 head dims of the 128-wide tile c / 8), and writes for each the
// two MlaSwz chunks 2c, 2c + 1 of
//   bf16_rne(fp32(e4m3) * scale)    (one exact widening, one fp32 multiply, one rounding to nearest even).
// The rotary 128 bytes are 8 chunks, copied as in the 16-bit forms.  to: the byte offset of this lane's token in the pool, -1 =
// not fetched: zero bytes and zero scales, zeros.  Four waves: a thread holds 4 + 1 + 1 chunks of tile t + 1 while tile t is
// computed on.
template <int NW>
struct MlaCopyF8 {
    static constexpr int T = 64 * NW, TPR = T / kMlaKT, CH = (kMlaDv / 16) / TPR, B = CH < 8 ? CH : 8, RCH = kMlaKT * (kMlaDk / 8) / T;
    static_assert(TPR * CH * 16 == kMlaDv && 8 % TPR == 0 && CH % B == 0 && RCH >= 1, "tile copy");
    const MlaF8Params& fp;
    const unsigned char* const none;   // where the loads of a token that is not fetched go
    const int tid, lrow, lc0;
    u32x4 xl[B], xs, xr[RCH];
    long long to = -1, lro = -1;

    __device__ __forceinline__ MlaCopyF8(const MlaF8Params& fp_)
        : fp(fp_), none((const unsigned char*)fp_.sp.mp.p.q), tid(threadIdx.x), lrow(threadIdx.x / TPR), lc0(threadIdx.x % TPR) {}
    __device__ __forceinline__ void place(int unit, int slot) { to = unit >= 0 ? unit * fp.page_sb + (long long)slot * fp.tok_sb : -1; }
    __device__ __forceinline__ void load_lat(int, int, int i0) {
        if (i0 == 0) {
            lro = __shfl(to, lrow, 64);
            const u32x4 y = *reinterpret_cast<const u32x4*>(lro >= 0 ? fp.pool + lro + kF8Scales : none);
            xs = lro >= 0 ? y : u32x4{0u, 0u, 0u, 0u};
        }
        const bool ok = lro >= 0;
#pragma unroll
        for (int i = 0; i < B; ++i) {
            const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? fp.pool + lro + 16 * (lc0 + TPR * (i0 + i)) : none);
            xl[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
        }
    }
    __device__ __forceinline__ void store_lat(char* lat, int i0) const {
#pragma unroll
        for (int i = 0; i < B; ++i) {
            const int c = lc0 + TPR * (i0 + i), tile = (TPR * (i0 + i)) >> 3;
            const uint32_t sb = tile == 0 ? xs[0] : tile == 1 ? xs[1] : tile == 2 ? xs[2] : xs[3];
            u32x4 lo, hi;
            mla_f8_widen(xl[i], __uint_as_float(sb), lo, hi);
            *reinterpret_cast<u32x4*>(lat + MlaSwz::off(lrow, 2 * c)) = lo;
            *reinterpret_cast<u32x4*>(lat + MlaSwz::off(lrow, 2 * c + 1)) = hi;
        }
    }
    __device__ __forceinline__ void load_rot(int, int) {
#pragma unroll
        for (int i = 0; i < RCH; ++i) {
            const int idx = T * i + tid, row = idx >> 3, ch = idx & 7;
            const long long ro = __shfl(to, row, 64);
            const bool ok = ro >= 0;
            const u32x4 y = *reinterpret_cast<const u32x4*>(ok ? fp.pool + ro + kF8Rope + 16 * ch : none);
            xr[i] = ok ? y : u32x4{0u, 0u, 0u, 0u};
        }
    }
};

// the rotary rows of a tile, chunk idx = T i + tid (row idx / 8, chunk idx % 8), from a thread's registers to LDS
template <int T, int RCH>
__device__ __forceinline__ void mla_store_rot(char* rop, const u32x4 (&xr)[RCH]) {
#pragma unroll
    for (int i = 0; i < RCH; ++i) {
        const int idx = T * i + (int)threadIdx.x;
        *reinterpret_cast<u32x4*>(rop + TileSwz<64>::off(idx >> 3, idx & 7)) = xr[i];
    }
}

// ---- the wave's share of the work

// q and qv as the B operand of S^T = K Q^T: head dims 32 ks + 8 g .. of row (qi, h), heads q_hs / qv_hs elements apart
__device__ __forceinline__ void mla_load_q(const MlaParams& mp, int q_hs, int qv_hs, const MlaRows& row, int g,
                                           s16x8 (&qf)[kMlaDk / 32], s16x8 (&qvf)[kMlaDv / 32]) {
    constexpr int DK = kMlaDk, DV = kMlaDv;
    const KvParams& p = mp.p;
    const buf_rsrc_t q_rs = make_rsrc(p.q + row.b * p.q_bs, (unsigned)(((p.nq - 1) * p.q_ts + (p.hq - 1) * q_hs + DK) * 2));
    const buf_rsrc_t qv_rs = make_rsrc(mp.qv + row.b * mp.qv_bs, (unsigned)(((p.nq - 1) * mp.qv_ts + (p.hq - 1) * qv_hs + DV) * 2));
#pragma unroll
    for (int ks = 0; ks < DK / 32; ++ks)
        qf[ks] = buf_load_frag(q_rs, row.valid ? (row.qi * p.q_ts + row.h * q_hs + 32 * ks + 8 * g) * 2 : kOobOff);
#pragma unroll
    for (int ks = 0; ks < DV / 32; ++ks)
        qvf[ks] = buf_load_frag(qv_rs, row.valid ? (row.qi * mp.qv_ts + row.h * qv_hs + 32 * ks + 8 * g) * 2 : kOobOff);
}

// One tile of 32 keys in LDS against the wave's 16 rows: scores, mask (vis(kb, i): register i of score block kb is visible),
// online softmax, P^T and the update of the accumulator
template <typename Tag, typename Mask>
__device__ __forceinline__ void mla_tile_step(const char* lat, const char* rop, const s16x8 (&qf)[kMlaDk / 32], const s16x8 (&qvf)[kMlaDv / 32],
                                              f32x4_t (&oacc)[kMlaDv / 16], float& m_run, float& l_run, float c_log2, int r, int g, Mask vis) {
    constexpr int DK = kMlaDk, DV = kMlaDv, NDB = DV / 16;
    const int q4 = r >> 2, p4 = r & 3;
    // S^T = K Q^T: A = key 16 kb + r, head dims 32 ks + 8 g .. of the rotary row, then of the latent row
    f32x4_t sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < DK / 32; ++ks)
            sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(rop + TileSwz<64>::off(16 * kb + r, 4 * ks + g)), qf[ks], sacc[kb]);
#pragma unroll
        for (int ks = 0; ks < DV / 32; ++ks) {
            // (four operand reads in flight: hipcc would otherwise hoist all of a tile's reads and spill)
            if (ks % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            sacc[kb] = mfma16<Tag>(*reinterpret_cast<const s16x8*>(lat + MlaSwz::off(16 * kb + r, 4 * ks + g)), qvf[ks], sacc[kb]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // both score tiles live in VGPRs at one point (kv_split_kernel: the second chain must not end in the first one's registers)
    asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = vis(kb, i) ? sacc[kb][i] : -INFINITY;
            sacc[kb][i] = x;
            mx = fmaxf(mx, x);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * c_log2);
    const float mc = m_use * c_log2;
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < NDB; ++t) oacc[t] *= alpha;
    // P^T as the B operand of O^T = V^T P^T: k-slot 8 g + j is key 4 g + j (j < 4) and 16 + 4 g + j - 4 (j >= 4).
    // l_run = l_run * alpha + the tile's four pair sums in order; the product and the first sum are one fma.  That is what hipcc's
    // contraction made of `l_run *= alpha; l_run += e0 + e1` in every instantiation while each form had its own text; it is
    // written out because the contraction depends on how the adds around it get vectorised.
    u32x4 pk;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float e0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][2 * j], c_log2, -mc));
            const float e1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][2 * j + 1], c_log2, -mc));
            l_run = kb + j == 0 ? fmaf(l_run, alpha, e0 + e1) : l_run + (e0 + e1);
            pk[2 * kb + j] = pack2<Tag>(e0, e1);
        }
    const s16x8 pb = *reinterpret_cast<s16x8*>(&pk);
    // V^T operand from the same latent image: rows (keys) 4 g + q and 16 + 4 g + q, head dims 16 t + 4 p ..
#pragma unroll
    for (int t = 0; t < NDB; ++t) {
        if (t % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        const int ch = 2 * t + (p4 >> 1), bo = 8 * (p4 & 1);
        const s16x4 lo = lds_tr16(lat + MlaSwz::off(4 * g + q4, ch) + bo);
        const s16x4 hi = lds_tr16(lat + MlaSwz::off(16 + 4 * g + q4, ch) + bo);
        oacc[t] = mfma16<Tag>(cat8(lo, hi), pb, oacc[t]);
    }
}

// kv_split_kernel's epilogue: O^T register i of block t is head dim 16 t + 4 g + i of row (b, qi, h); o and lse, or with S > 1
// the partials of split s
template <typename Tag>
__device__ __forceinline__ void mla_epilogue(const KvParams& p, const MlaRows& row, int g, const f32x4_t (&oacc)[kMlaDv / 16], float m_run, float l_run) {
    constexpr int DV = kMlaDv, NDB = DV / 16;
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const float lse_v = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if (!row.valid) return;
    const size_t row_id = ((size_t)row.b * p.hq + row.h) * p.nq + row.qi;
    if (row.S == 1) {
        uint16_t* orow = p.o + (((size_t)row.b * p.nq + row.qi) * p.hq + row.h) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            u32x2 v;
            v[0] = pack2_rn<Tag>(oacc[t][0] * inv, oacc[t][1] * inv);
            v[1] = pack2_rn<Tag>(oacc[t][2] * inv, oacc[t][3] * inv);
            *reinterpret_cast<u32x2*>(orow + 16 * t + 4 * g) = v;
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * row.S + row.s) * DV;
#pragma unroll
        for (int t = 0; t < NDB; ++t) *reinterpret_cast<f32x4_t*>(prow + 16 * t + 4 * g) = oacc[t] * inv;
        if (g == 0) p.plse[row_id * row.S + row.s] = lse_v;
    }
}

// The kernel: the tile pipeline over the keys that `keys` names, brought to LDS by `copy`
template <typename Tag, int NW, typename Keys, typename Copy>
__device__ __forceinline__ void mla_decode(char* lds, const MlaParams& mp, int q_hs, int qv_hs, Keys& keys, Copy& copy) {
    constexpr int KT = kMlaKT, NDB = kMlaDv / 16;
    constexpr bool PRE = NW == 4;
    char* const lat = lds;
    char* const rop = lds + kMlaLatBytes;
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int kbeg = keys.kbeg, kend = keys.kend;

    s16x8 qf[kMlaDk / 32], qvf[kMlaDv / 32];
    mla_load_q(mp, q_hs, qv_hs, keys, g, qf, qvf);
    keys.start();

    f32x4_t oacc[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t) oacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // this lane's key of the tile at kt, from the producer to the copy; the tile's flags
    auto produce = [&](int kt) {
        int unit, slot;
        const unsigned vm = keys.next(kt, unit, slot);
        copy.place(unit, slot);
        return vm;
    };
    unsigned vm_next = 0u;
    if (PRE && kbeg < kend) {
        vm_next = produce(kbeg);
        copy.load_lat(kbeg, kend, 0);
        copy.load_rot(kbeg, kend);
    }

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        unsigned vm = vm_next;
        if constexpr (!PRE) vm = produce(k0);
        __syncthreads();   // every wave has read the previous tile
        if constexpr (PRE) {
            copy.store_lat(lat, 0);
        } else {
#pragma unroll 1
            for (int i0 = 0; i0 < Copy::CH; i0 += Copy::B) {
                copy.load_lat(k0, kend, i0);
                copy.store_lat(lat, i0);
            }
            copy.load_rot(k0, kend);
        }
        mla_store_rot<64 * NW>(rop, copy.xr);
        __syncthreads();
        if (PRE && k0 + KT < kend) {
            vm_next = produce(k0 + KT);
            copy.load_lat(k0 + KT, kend, 0);
            copy.load_rot(k0 + KT, kend);
        }
        if (!keys.active) continue;   // (wave-uniform; the wave still takes part in the copies and the barriers)
        mla_tile_step<Tag>(lat, rop, qf, qvf, oacc, m_run, l_run, mp.p.c_log2, r, g, keys.mask(k0, vm, g));
    }
    mla_epilogue<Tag>(mp.p, keys, g, oacc, m_run, l_run);
}

template <typename Tag, int NW, bool PAGED>
__global__ __launch_bounds__(64 * NW) void mla_split_kernel(MlaParams mp) {
    __shared__ __attribute__((aligned(16))) char lds[kMlaLdsBytes];
    const int hk = blockIdx.y % mp.p.hkv, wt = blockIdx.y / mp.p.hkv;
    MlaDenseKeys<NW, PAGED> keys(mp.p, hk, wt);
    std::conditional_t<PAGED, MlaCopy16At<NW>, MlaCopy16Contig<NW>> copy(mp.p, hk, keys.b);
    mla_decode<Tag, NW>(lds, mp, kMlaDk, kMlaDv, keys, copy);
}

template <typename Tag, int NW, bool PAGED>
__global__ __launch_bounds__(64 * NW) void mla_sparse_kernel(MlaSparseParams sp) {
    __shared__ __attribute__((aligned(16))) char lds[kMlaLdsBytes];
    const int hk = blockIdx.z % sp.mp.p.hkv, wt = blockIdx.z / sp.mp.p.hkv;
    MlaListKeys<NW, PAGED> keys(sp, hk, wt);
    MlaCopy16At<NW> copy(sp.mp.p, hk, keys.b);
    mla_decode<Tag, NW>(lds, sp.mp, kMlaDk, kMlaDv, keys, copy);
}

// (one K/V head: hk = 0 throughout)
template <int NW, bool SPARSE>
__global__ __launch_bounds__(64 * NW) void mla_f8_kernel(MlaF8Params fp) {
    __shared__ __attribute__((aligned(16))) char lds[kMlaLdsBytes];
    MlaCopyF8<NW> copy(fp);
    if constexpr (SPARSE) {
        MlaListKeys<NW, true> keys(fp.sp, 0, blockIdx.z);
        mla_decode<bf16_tag, NW>(lds, fp.sp.mp, fp.q_hs, fp.qv_hs, keys, copy);
    } else {
        MlaDenseKeys<NW, true> keys(fp.sp.mp.p, 0, blockIdx.y);
        mla_decode<bf16_tag, NW>(lds, fp.sp.mp, fp.q_hs, fp.qv_hs, keys, copy);
    }
}

// kv_combine_kernel for 512-wide rows: one wave per (b, h_q, token) row, four rows a workgroup; the weights as there, then lane c
// adds head dims 256 j + 4 c .. + 3 (j = 0, 1) of the O partials in split order.  A split with lse_s = -inf has weight 0 and its
// O partial, which it never wrote, is selected away; a row without any visible key gives o = 0, lse = -inf.  Same bits on every run.
template <typename Tag>
__global__ __launch_bounds__(256) void mla_combine_kernel(KvParams p, int S, long long nrows) {
    constexpr int DV = kMlaDv;
    __shared__ float wsh[4][256];
    const int wv = threadIdx.x >> 6, c = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + wv;
    if (row >= nrows) return;   // (wave-uniform; the LDS rows are wave-private, no barrier)
    const float* pl = p.plse + row * S;
    int h;
    long long orow;
    if (!kv_combine_row(p, row, pl, h, orow)) return;
    float m = -INFINITY;
    for (int s = c; s < S; s += 64) m = fmaxf(m, pl[s]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int s = c; s < S; s += 64) {
        const float ls = pl[s];
        const float wgt = (ls == -INFINITY) ? 0.f : __expf(ls - m);
        wsh[wv][s] = wgt;
        sum += wgt;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
    for (int j = 0; j < DV / 256; ++j) {
        const int col = 256 * j + 4 * c;
        const float* po = p.po + row * S * DV + col;
        f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int s = 0; s < S; ++s) {
            const float wgt = wsh[wv][s];
            const f32x4_t x = *reinterpret_cast<const f32x4_t*>(po + (size_t)s * DV);
            acc += (wgt != 0.f) ? wgt * x : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        u32x2 v;
        v[0] = pack2_rn<Tag>(acc[0] * inv, acc[1] * inv);
        v[1] = pack2_rn<Tag>(acc[2] * inv, acc[3] * inv);
        *reinterpret_cast<u32x2*>(p.o + orow * DV + col) = v;
    }
    if (c == 0) p.lse[row] = sum > 0.f ? m + logf(sum) : -INFINITY;
}

// fa_mla_fp8_pack: one wave a new token.  Lane l holds 8 latent elements of tile l / 16: amax over the tile's 16 lanes,
// scale = amax > 0 ? amax / 448 : 1 (pow2: rounded up to a power of two), byte = e4m3_rne(clamp(x / scale, +-448)) with both
// divisions IEEE-rounded; 8 bytes a lane, the four scales one 16-byte store of lane 0, the rotary 128 bytes by lanes 0 .. 7.
// The token goes to position cache_seqlens[b] + i through the table; a negative length, a position at or past the table's
// capacity or a page outside the pool drops it: nothing is written.  The power of two is taken in the bit pattern (a mantissa
// that is not zero: the next exponent), exact for every normal scale below 2^127; a subnormal scale would go to 2^-126 and one
// in the top binade to +inf, where tests/mla_fp8_ref.py (frexp / ldexp) differs: amax below 448 * 2^-126 or above 448 * 2^127,
// outside the contract as NaN and infinity are (values in [2^-6, 8] give scales in [2^-15, 2^-5]).
struct MlaF8PackParams {
    const uint16_t *lat, *rope;
    unsigned char* pool;
    const int *seqlens, *table;
    long long lat_bs, lat_ts, rope_bs, rope_ts, page_sb, tok_sb, tbl_rs, tokens;
    int nnew, nblk, ps, mb, pow2;
};

__global__ __launch_bounds__(256) void mla_f8_pack_kernel(MlaF8PackParams a) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.tokens) return;   // (wave-uniform, as everything up to the loads)
    const long long b = t / a.nnew;
    const int i = (int)(t - b * a.nnew);
    const int len = a.seqlens[b];
    const long long pos = (long long)len + i;
    if (len < 0 || pos >= (long long)a.mb * a.ps) return;
    const int j = (int)(pos / a.ps), slot = (int)(pos - (long long)j * a.ps);
    const int pg = a.table[b * a.tbl_rs + j];
    if ((unsigned)pg >= (unsigned)a.nblk) return;
    unsigned char* dst = a.pool + pg * a.page_sb + slot * a.tok_sb;

    const u32x4 x = *reinterpret_cast<const u32x4*>(a.lat + b * a.lat_bs + i * a.lat_ts + 8 * lane);
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = unpack_lo<bf16_tag>(x[k]);
        v[2 * k + 1] = unpack_hi<bf16_tag>(x[k]);
    }
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(v[k]));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    float scale = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
    if (a.pow2) {
        uint32_t bits = __float_as_uint(scale);
        if (bits & 0x007fffffu) bits = (bits & 0x7f800000u) + 0x00800000u;
        scale = __uint_as_float(bits);
    }
    float y[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = fminf(fmaxf(__fdiv_rn(v[k], scale), -448.f), 448.f);
    u32x2 q8;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * k], y[4 * k + 1], 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * k + 2], y[4 * k + 3], c, true);
        q8[k] = (uint32_t)c;
    }
    *reinterpret_cast<u32x2*>(dst + 8 * lane) = q8;
    u32x4 sc;
#pragma unroll
    for (int k = 0; k < 4; ++k) sc[k] = __float_as_uint(__shfl(scale, 16 * k, 64));
    if (lane == 0) *reinterpret_cast<u32x4*>(dst + kF8Scales) = sc;
    if (lane < 8)
        *reinterpret_cast<u32x4*>(dst + kF8Rope + 16 * lane) = *reinterpret_cast<const u32x4*>(a.rope + b * a.rope_bs + i * a.rope_ts + 8 * lane);
}

// ---- host

// The split rule of every form.  A unit is a workgroup of mla_waves(rows) waves over 16 * waves of the rows that share a key
// stream; there are lists * heads_kv such streams.  The 16 x 512 fp32 accumulator beside the q and qv fragments takes a wave past
// 256 registers, so one wave runs per SIMD and a CU holds 4 / waves workgroups (36 KiB of LDS each).  Enough splits to fill the
// 256 CUs once, none shorter than 128 keys, at most 256 (the combine's weight row).
int mla_split_rule(int64_t lists, int64_t heads_kv, int64_t rows, int64_t keys) {
    constexpr int64_t kCUs = 256, kMinKeys = 128;
    if (rows <= 0) return 1;
    const int64_t nw = mla_waves(rows), per_cu = 4 / nw;
    const int64_t units = lists * heads_kv * ((rows + 16 * nw - 1) / (16 * nw));
    if (units <= 0 || keys <= 0) return 1;
    int64_t s = (kCUs * per_cu + units - 1) / units;
    s = std::min<int64_t>(s, (keys + kMinKeys - 1) / kMinKeys);
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, 256));
}

// What the three launchers share: the kernel parameters of the call in mp, with the workspace (S > 1: kv_workspace_bytes at d_v,
// the O partials and then the lse partials); the split kernel with the wave count of the rows of a workgroup's key stream (lists:
// the G heads, else the G * Nq packed rows) through split(tag, waves), which returns the launch's error; then the combine.
template <typename Tag, typename Split>
hipError_t mla_launch(MlaParams& mp, const KvArgs& kv, bool lists, hipStream_t st, Split&& split) {
    mp.p = kv_make_params(kv);
    mp.qv = (const uint16_t*)kv.qv; mp.qv_bs = kv.qv_bs; mp.qv_ts = (int)kv.qv_ts;
    const int S = (int)kv.num_splits;
    const size_t q_rows = (size_t)kv.batch * kv.heads_q * kv.seqlen_q;
    mp.p.po = (float*)kv.workspace;
    mp.p.plse = S > 1 ? (float*)((char*)kv.workspace + ((q_rows * S * kMlaDv * 4 + 255) & ~(size_t)255)) : nullptr;
    const int nw = mla_waves(lists ? mp.p.G : mp.p.rows);
    const hipError_t e = nw == 1 ? split(Tag{}, std::integral_constant<int, 1>{})
                       : nw == 2 ? split(Tag{}, std::integral_constant<int, 2>{}) : split(Tag{}, std::integral_constant<int, 4>{});
    if (e != hipSuccess || S == 1) return e;
    const long long nrows = (long long)q_rows;
    hipLaunchKernelGGL((mla_combine_kernel<Tag>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, mp.p, S, nrows);
    return hipGetLastError();
}

// the grids: dense (split, row tiles x K/V heads, sequence); lists (list, split, row tiles x K/V heads)
inline dim3 mla_grid(const KvParams& p, const KvArgs& kv, bool lists, int nw) {
    const unsigned S = (unsigned)kv.num_splits, tiles = (unsigned)(((lists ? p.G : p.rows) + 16 * nw - 1) / (16 * nw) * p.hkv);
    return lists ? dim3((unsigned)(kv.batch * kv.seqlen_q), S, tiles) : dim3(S, tiles, (unsigned)kv.batch);
}

}  // namespace

// Waves a workgroup: one per 16-row tile of the rows = G * Nq packed rows of a (sequence, K/V head), at most four (one per SIMD)
int mla_waves(int64_t rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : 4; }

// kv_num_splits for the dense forms: rows = G * Nq packed rows of each of the batch sequences, over cache_len keys
int mla_num_splits(int64_t batch, int64_t heads_kv, int64_t rows, int64_t cache_len) { return mla_split_rule(batch, heads_kv, rows, cache_len); }

// ... and for the lists: units = batch * seqlen_q lists a K/V head, the group heads of each over topk list positions
int mla_sparse_num_splits(int64_t units, int64_t heads_kv, int64_t group, int64_t topk) { return mla_split_rule(units, heads_kv, group, topk); }

hipError_t launch_kvcache_mla(const KvArgs& a, hipStream_t st) {
    if (a.d != kMlaDk || a.d_v != kMlaDv) return hipErrorInvalidValue;   // (the C layer's check)
    MlaParams mp;
    auto split = [&](auto tag, auto nw) {
        using Tag = decltype(tag);
        constexpr int NW = decltype(nw)::value;
        const dim3 grid = mla_grid(mp.p, a, false, NW);
        if (mp.p.table) hipLaunchKernelGGL((mla_split_kernel<Tag, NW, true>), grid, dim3(64 * NW), 0, st, mp);
        else hipLaunchKernelGGL((mla_split_kernel<Tag, NW, false>), grid, dim3(64 * NW), 0, st, mp);
        return hipGetLastError();
    };
    return a.dtype == 1 ? mla_launch<f16_tag>(mp, a, false, st, split) : mla_launch<bf16_tag>(mp, a, false, st, split);
}

hipError_t launch_mla_sparse(const MlaSparseArgs& a, hipStream_t st) {
    const KvArgs& kv = a.kv;
    if (kv.d != kMlaDk || kv.d_v != kMlaDv) return hipErrorInvalidValue;   // (the C layer's check)
    MlaSparseParams sp;
    sp.idx = a.indices; sp.ix_bs = a.ix_bs; sp.ix_ts = a.ix_ts; sp.ix_hs = a.ix_hs;
    sp.topk = (int)a.topk; sp.causal = kv.causal;
    auto split = [&](auto tag, auto nw) {
        using Tag = decltype(tag);
        constexpr int NW = decltype(nw)::value;
        const dim3 grid = mla_grid(sp.mp.p, kv, true, NW);
        if (sp.mp.p.table) hipLaunchKernelGGL((mla_sparse_kernel<Tag, NW, true>), grid, dim3(64 * NW), 0, st, sp);
        else hipLaunchKernelGGL((mla_sparse_kernel<Tag, NW, false>), grid, dim3(64 * NW), 0, st, sp);
        return hipGetLastError();
    };
    return kv.dtype == 1 ? mla_launch<f16_tag>(sp.mp, kv, true, st, split) : mla_launch<bf16_tag>(sp.mp, kv, true, st, split);
}

hipError_t launch_mla_f8(const MlaF8Args& a, hipStream_t st) {
    const KvArgs& kv = a.sa.kv;
    if (kv.d != kMlaDk || kv.d_v != kMlaDv || kv.dtype != 2 || kv.heads_kv != 1 || !kv.block_table) return hipErrorInvalidValue;   // (the C layer's checks)
    const bool sparse = a.sa.indices != nullptr;
    MlaF8Params fp;
    fp.sp.idx = a.sa.indices; fp.sp.ix_bs = a.sa.ix_bs; fp.sp.ix_ts = a.sa.ix_ts; fp.sp.ix_hs = 0;
    fp.sp.topk = (int)a.sa.topk; fp.sp.causal = kv.causal;
    fp.pool = (const unsigned char*)a.pool; fp.page_sb = a.page_sb; fp.tok_sb = (int)a.tok_sb;
    fp.q_hs = (int)a.q_hs; fp.qv_hs = (int)a.qv_hs;
    auto split = [&](auto, auto nw) {
        constexpr int NW = decltype(nw)::value;
        const dim3 grid = mla_grid(fp.sp.mp.p, kv, sparse, NW);
        if (sparse) hipLaunchKernelGGL((mla_f8_kernel<NW, true>), grid, dim3(64 * NW), 0, st, fp);
        else hipLaunchKernelGGL((mla_f8_kernel<NW, false>), grid, dim3(64 * NW), 0, st, fp);
        return hipGetLastError();
    };
    return mla_launch<bf16_tag>(fp.sp.mp, kv, sparse, st, split);
}

hipError_t launch_mla_f8_pack(const MlaF8PackArgs& a, hipStream_t st) {
    MlaF8PackParams k;
    k.lat = (const uint16_t*)a.latent; k.rope = (const uint16_t*)a.rope; k.pool = (unsigned char*)a.pool;
    k.seqlens = a.cache_seqlens; k.table = a.block_table;
    k.lat_bs = a.lat_bs; k.lat_ts = a.lat_ts; k.rope_bs = a.rope_bs; k.rope_ts = a.rope_ts;
    k.page_sb = a.page_sb; k.tok_sb = a.tok_sb; k.tbl_rs = a.table_row_stride; k.tokens = a.batch * a.seqlen_new;
    k.nnew = (int)a.seqlen_new; k.nblk = (int)a.num_blocks; k.ps = (int)a.page_size; k.mb = (int)a.max_blocks; k.pow2 = a.scale_pow2 ? 1 : 0;
    hipLaunchKernelGGL(mla_f8_pack_kernel, dim3((unsigned)((k.tokens + 3) / 4)), dim3(256), 0, st, k);
    return hipGetLastError();
}

}  // namespace fa
