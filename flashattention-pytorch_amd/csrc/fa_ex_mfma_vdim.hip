// Extended attention on the 16-bit MFMA with V narrower than Q and K (bf16 / f16): q, k, dq, dk are d wide, v, o, dO, dv are d_v
// wide, 8 <= d_v < d <= 192, d_v <= 128, both multiples of 8 — DeepSeek-style MLA before weight absorption (192 = 128 nope + 64
// rope, 128) and every narrower pair, zero-padded into ONE instantiation D = 192, DV = 128 the way fa_ex_mfma.hip pads p.d into D.
// Bodies of their own: the .inc bodies of fa_ex_mfma.hip carry a single width and are shared textually by the existing entries.
//
// A 192-wide tile is no power of two, and TileSwz / dma_stage_tile / dma_lane_voff know 64, 128 and 256.  So a [rows][192] tile
// is kept as TWO images, columns 0 .. 127 as a TileSwz<128> image and columns 128 .. 191 as a TileSwz<64> image behind it
// (Tile192), each staged by its own LDS-DMA from a buffer descriptor of its own: the second one starts 128 elements into the
// row and covers d - 128 columns (nothing for d <= 128).  Every read is then one of the two conflict-free patterns the 64- and
// 128-wide kernels already use; chunk >= 16 is a compile-time fact at every use (ks >= 8 of 12, block >= 4 of 6).
//
//   forward : 8 waves x 32 query rows, K/V tiles of 64 keys double-buffered: 2 x (24 + 16) KiB = 80 KiB (a 128-key tile would be
//             the whole 160 KiB).  Q in registers (12 fragments), S^T = K Q^T with the query on the lane, online softmax in
//             registers, O^T += V^T P^T into 4 accumulator blocks.
//   dK/dV   : 8 waves x 32 keys = 256 keys of K in LDS (96 KiB), V in registers (8 fragments), Q / dO tiles of 32 rows
//             double-buffered: 2 x (12 + 8) KiB.  137 KiB.  The key on the lane; 6 + 4 accumulator blocks = 160 registers.
//   dQ      : 8 waves x 32 query rows, the forward's K/V tiles; Q in registers, the lane's dO fragments in LDS (64 KiB: 144 KiB),
//             one 32-key block of S, dP, dS at a time, 6 accumulator blocks.
// No kernel touches scratch (tools/kernel_resources.sh fa_ex_mfma_vdim: 243 / 256 / 256 VGPRs); DESIGN.md 9s has the accounting.
// Features: the causal mask with the shifted diagonal (coff = nk - nq), softmax_scale, GQA (kv unit = bh / g; dK / dV per query
// head, summed by kv_group_sum at each one's width), packed sequences (cu_seqlens clamped by seq_span, token strides), lse out,
// dlse in (through the row constant the pre-pass of fa_ex_mfma.hip writes).  Everything else is refused by the C layer.
// A row without a visible key: o = 0, lse = -inf, dQ = 0.
#include "fa_common.h"
#include "fa_ex_common.h"
#include "fa_ex_mfma_feat.h"
#include "fa_kernels.h"

namespace fa {

namespace {

constexpr int VD = 192, VDV = 128;   // the instantiation's widths

struct VdParams {
    int nq, nk, d, dv;     // rows, keys (varlen: the maxima), run-time widths
    int causal, coff;      // coff = nk - nq (varlen: per sequence)
    int hq;                // varlen: query heads
    int total_q, total_k;
    int sq, sk, sv;        // varlen: token strides of q, k, v (elements)
    const int* cu_q;       // varlen: [B + 1] untrusted token offsets
    const int* cu_k;
    float scale;
    unsigned kvg;          // kv_magic(query heads per K/V head)
};

// A [ROWS][192] tile as [ROWS][128] (TileSwz<128>) followed by [ROWS][64] (TileSwz<64>)
template <int ROWS> struct Tile192 {
    static constexpr int LO_BYTES = ROWS * 256, BYTES = ROWS * 384;
    // byte offset of 16-byte chunk `ch` (0 .. 23) of row `row`; hi = (ch >= 16), a constant once the caller's loop is unrolled
    static __device__ __forceinline__ int off(int row, int ch, bool hi) {
        return hi ? LO_BYTES + TileSwz<64>::off(row, ch - 16) : TileSwz<128>::off(row, ch);
    }
};

// the two descriptors and lane offsets that stage rows of a (n, d) tensor, rows `stride` elements apart, into a Tile192
struct Src192 {
    rsrc_s_t lo, hi;
    int voff_lo, voff_hi, stride;
};
__device__ __forceinline__ Src192 make_src192(const uint16_t* base, int n, int d, int stride, int lane, int w) {
    Src192 s;
    const int dlo = min(d, 128), dhi = max(d - 128, 0);
    s.lo = make_rsrc_s(base, span_bytes(n, dlo, stride));
    s.hi = make_rsrc_s(base + 128, dhi > 0 ? span_bytes(n, dhi, stride) : 0u);
    s.voff_lo = dma_lane_voff<128, true>(lane, w, dlo, stride);
    s.voff_hi = dma_lane_voff<64, true>(lane, w, dhi, stride);
    s.stride = stride;
    return s;
}
template <int ROWS, int NW>
__device__ __forceinline__ void stage192(const Src192& s, char* tile, int row0, int w) {
    dma_stage_tile<128, ROWS, NW, true>(s.lo, tile, row0, s.voff_lo, w, 128, 0, s.stride);
    if constexpr (ROWS % (8 * NW) == 0) {
        dma_stage_tile<64, ROWS, NW, true>(s.hi, tile + Tile192<ROWS>::LO_BYTES, row0, s.voff_hi, w, 64, 0, s.stride);
    } else {
        // fewer 1-KiB pieces (8 rows each) than waves: wave w < ROWS / 8 takes piece w, whose row class is voff_hi's
        static_assert(ROWS % 8 == 0 && ROWS / 8 < NW, "pieces of the 64-wide image");
        if (w < ROWS / 8)
            dma16_issue(s.hi, lds_addr_of(tile + Tile192<ROWS>::LO_BYTES) + w * 1024, s.voff_hi,
                        __builtin_amdgcn_readfirstlane((row0 + 8 * w) * 2 * s.stride));
    }
}

// Lane-constant operand addresses.  Inside a row the swizzle is an XOR on the chunk index, so the offsets a loop walks differ from
// ONE base by an XOR with a constant: TileSwz<128>::off(r, 2 ks + h) = off(r, h) ^ 32 ks (TileSwz<64> alike), and the transposed
// read of block db at rows 16 s + 4 h + tq (+ 8) is (base ^ 64 db) + 16 s rows.  A kernel keeps the few bases (made opaque once
// per tile, so that hipcc does not hoist every derived address into a register of its own: they spilled) and pays one v_xor a read.
struct OpBase {
    int row_lo, row_hi;        // row-wise 16-byte reads: TileSwz<128>::off(r, h), TileSwz<64>::off(r, h)
    int tr_lo[2], tr_hi[2];    // transposed reads, rows 4 h + tq and + 8: the 128-wide and the 64-wide image
};
__device__ __forceinline__ OpBase make_op_base(int lane) {
    const int r = lane & 31, h = lane >> 5, li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;
    OpBase b;
    b.row_lo = TileSwz<128>::off(r, h);
    b.row_hi = TileSwz<64>::off(r, h);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        b.tr_lo[e] = TileSwz<128>::off(4 * h + tq + 8 * e, 2 * g16 + (tp >> 1)) + 8 * (tp & 1);
        b.tr_hi[e] = TileSwz<64>::off(4 * h + tq + 8 * e, 2 * g16 + (tp >> 1)) + 8 * (tp & 1);
    }
    return b;
}
__device__ __forceinline__ void opaque(OpBase& b) {
    asm volatile("" : "+v"(b.row_lo), "+v"(b.row_hi), "+v"(b.tr_lo[0]), "+v"(b.tr_lo[1]), "+v"(b.tr_hi[0]), "+v"(b.tr_hi[1]));
}
// transposed 8 x 16-bit operand of block db (4 of 128 columns each in the wide image, then 2 in the narrow one) at rows row0 + ..
template <int ROWS>
__device__ __forceinline__ s16x8 tr_frag192(const char* tile, const OpBase& b, int row0, int db) {
    if (db < 4) return cat8(lds_tr16(tile + row0 * 256 + (b.tr_lo[0] ^ (64 * db))), lds_tr16(tile + row0 * 256 + (b.tr_lo[1] ^ (64 * db))));
    return cat8(lds_tr16(tile + Tile192<ROWS>::LO_BYTES + row0 * 128 + (b.tr_hi[0] ^ (64 * (db - 4)))),
                lds_tr16(tile + Tile192<ROWS>::LO_BYTES + row0 * 128 + (b.tr_hi[1] ^ (64 * (db - 4)))));
}
__device__ __forceinline__ s16x8 tr_frag128(const char* tile, const OpBase& b, int row0, int db) {
    return cat8(lds_tr16(tile + row0 * 256 + (b.tr_lo[0] ^ (64 * db))), lds_tr16(tile + row0 * 256 + (b.tr_lo[1] ^ (64 * db))));
}
// row-wise operand of k-step ks of row row0 + r
template <int ROWS>
__device__ __forceinline__ s16x8 row_frag192(const char* tile, const OpBase& b, int row0, int ks) {
    if (ks < 8) return *reinterpret_cast<const s16x8*>(tile + row0 * 256 + (b.row_lo ^ (32 * ks)));
    return *reinterpret_cast<const s16x8*>(tile + Tile192<ROWS>::LO_BYTES + row0 * 128 + (b.row_hi ^ (32 * (ks - 8))));
}
__device__ __forceinline__ s16x8 row_frag128(const char* tile, const OpBase& b, int row0, int ks) {
    return *reinterpret_cast<const s16x8*>(tile + row0 * 256 + (b.row_lo ^ (32 * ks)));
}

// the workgroup's unit: bases, strides and the sequence's row counts
struct VdUnit {
    int nq, nk, coff;
    size_t qbase, kbase, vbase, obase, lbase;
    int sq, sk, sv, so;    // row strides of q, k, v and of o / dout (elements)
    size_t dqbase;         // dq: q's rows, dense
    int sdq;
    int sk0, hh;           // varlen: first key token, query head
};
// VAR: narrows the padded grid's unit bh = b * hq + h to sequence b (the caller leaves at once when its tile starts past it)
template <bool VAR>
__device__ __forceinline__ void vd_unit(const VdParams& p, int bh, VdUnit& u) {
    u.nq = p.nq; u.nk = p.nk; u.coff = p.coff; u.sk0 = 0; u.hh = 0;
    if constexpr (VAR) {
        const int b = bh / p.hq;
        const int hh = bh - b * p.hq, hk = kv_unit(hh, p.kvg);
        int sq0, sk0, lq, lk;
        seq_span(p.cu_q, b, p.total_q, p.nq, sq0, lq);
        seq_span(p.cu_k, b, p.total_k, p.nk, sk0, lk);
        u.nq = lq; u.nk = lk; u.coff = lk - lq; u.sk0 = sk0; u.hh = hh;
        u.qbase = (size_t)sq0 * p.sq + hh * p.d;
        u.kbase = (size_t)sk0 * p.sk + hk * p.d;
        u.vbase = (size_t)sk0 * p.sv + hk * p.dv;
        u.obase = ((size_t)sq0 * p.hq + hh) * p.dv;
        u.lbase = (size_t)hh * p.total_q + sq0;
        u.dqbase = ((size_t)sq0 * p.hq + hh) * p.d;
        u.sq = p.sq; u.sk = p.sk; u.sv = p.sv; u.so = p.hq * p.dv; u.sdq = p.hq * p.d;
    } else {
        const size_t kvu = (size_t)kv_unit(bh, p.kvg);
        u.qbase = (size_t)bh * p.nq * p.d;
        u.kbase = kvu * p.nk * p.d;
        u.vbase = kvu * p.nk * p.dv;
        u.obase = (size_t)bh * p.nq * p.dv;
        u.lbase = (size_t)bh * p.nq;
        u.dqbase = u.qbase;
        u.sq = p.d; u.sk = p.d; u.sv = p.dv; u.so = p.dv; u.sdq = p.d;
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <typename Tag, bool VAR>
__global__ __launch_bounds__(512, 2) void exv_fwd_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                         const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
                                                         float* __restrict__ lse, VdParams p, float c_log2) {
    constexpr int NW = 8, BM = 32 * NW, KB = 2, BN = 32 * KB, NKS = VD / 16, NDV = VDV / 32;
    constexpr int K_BYTES = Tile192<BN>::BYTES, V_BYTES = BN * VDV * 2, BUF_BYTES = K_BYTES + V_BYTES;
    using KT = Tile192<BN>;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K tile | V tile]
    const int nqt = (p.nq + BM - 1) / BM;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;
    const int q0 = (L - bh * nqt) * BM;
    VdUnit u;
    vd_unit<VAR>(p, bh, u);
    const int nq = u.nq, nk = u.nk, coff = u.coff;
    if (VAR && q0 >= nq) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int DR = p.d, DVR = p.dv;
    const int qrow = q0 + 32 * w + r;

    const buf_rsrc_t q_rs = make_rsrc(q + u.qbase, span_bytes(nq, DR, u.sq));
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = buf_load_frag(q_rs, frag_off<true>(qrow, 16 * ks + 8 * h, DR, true, u.sq));

    const Src192 ksrc = make_src192(k + u.kbase, nk, DR, u.sk, lane, w);
    const rsrc_s_t v_rs = make_rsrc_s(v + u.vbase, span_bytes(nk, DVR, u.sv));
    const int voff_v = dma_lane_voff<VDV, true>(lane, w, DVR, u.sv);
    auto stage = [&](int buf, int k0) {
        char* kb_ = smem + buf * BUF_BYTES;
        stage192<BN, NW>(ksrc, kb_, k0, w);
        dma_stage_tile<VDV, BN, NW, true>(v_rs, kb_ + K_BYTES, k0, voff_v, w, VDV, 0, u.sv);
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // keys past the last row's diagonal are masked for every row of the tile (of the wave)
    const int kend = p.causal ? max(0, min(nk, q0 + BM + coff)) : nk;
    const int kend_w = p.causal ? max(0, min(nk, q0 + 32 * w + 32 + coff)) : nk;
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int t = 0, cur = 0;
    if (t < ntiles) stage(0, 0);
    dma_wait_all();
    __syncthreads();
    // tiles this wave computes, then the ones it only helps to load
    while (t < ntiles_w) {
        const int tn = t + 1;
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * BUF_BYTES;
        const char* Vt = Kt + K_BYTES;
        f32x16 sacc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const s16x8 a = *reinterpret_cast<const s16x8*>(Kt + KT::off(32 * kb + r, 2 * ks + h, ks >= 8));
                sacc[kb] = mfma32<Tag>(a, qf[ks], sacc[kb]);
            }
        }
        // ---- causal diagonal / ragged last tile: key index of register i is k0 + 32 kb + 4 h + rc(i)
        const bool need_mask = (p.causal && (k0 + BN - 1 > q0 + 32 * w + coff)) || (k0 + BN > nk);
        if (need_mask) {
            const int lim = p.causal ? min(qrow + coff, nk - 1) : nk - 1;   // last visible key of this lane's row
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const int thr = lim - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (rc_of(i) > thr) sacc[kb][i] = -INFINITY;
            }
        }
        // ---- online softmax, with rows that have not met a visible key yet (m = -inf)
        float mx = sacc[0][0];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
        mx = fmaxf(mx, wave_half_swap(mx));
        const float m_new = fmaxf(m_run, mx);
        float mc;
        // lazy rescale: keep the stale max while no row has grown past it by more than 2^8; -inf - -inf = NaN counts as "rescale"
        const bool rescale = __any(!((m_new - m_run) * c_log2 <= 8.0f)) != 0;
        if (rescale) {
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * c_log2);
            mc = m_use * c_log2;
            m_run = m_new;
#pragma unroll
            for (int t2 = 0; t2 < NDV; ++t2)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
            l_run *= alpha;
        } else {
            mc = m_run * c_log2;
        }
        float rs = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float pe = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], c_log2, -mc));
                rs += pe;
                sacc[kb][i] = pe;
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                u32x4 pk;
#pragma unroll
                for (int j = 0; j < 4; ++j) pk[j] = pack2<Tag>(sacc[kb][8 * s + 2 * j], sacc[kb][8 * s + 2 * j + 1]);
                const s16x8 pb = *reinterpret_cast<s16x8*>(&pk);
                const int key_a = 32 * kb + 16 * s + 4 * h + tq;
#pragma unroll
                for (int dvb = 0; dvb < NDV; ++dvb) {
                    const int ch = 4 * dvb + 2 * g16 + (tp >> 1);
                    const s16x4 lo = lds_tr16(Vt + TileSwz<VDV>::off(key_a, ch) + 8 * (tp & 1));
                    const s16x4 hi4 = lds_tr16(Vt + TileSwz<VDV>::off(key_a + 8, ch) + 8 * (tp & 1));
                    oacc[dvb] = mfma32<Tag>(cat8(lo, hi4), pb, oacc[dvb]);
                }
            }
        }
        l_run += rs;
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    while (t < ntiles) {
        const int tn = t + 1;
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }

    // ---- epilogue: normalise, store O and lse.  Every wave is past the last barrier and nothing is in flight: each wave
    // stages its rows in 32 x DV x 2 bytes of the tile memory
    const float l_tot = l_run + wave_half_swap(l_run);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vals[4 * dvb + g][0] = pack2_rn<Tag>(oacc[dvb][4 * g + 0] * inv, oacc[dvb][4 * g + 1] * inv);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(oacc[dvb][4 * g + 2] * inv, oacc[dvb][4 * g + 3] * inv);
        }
    store_rows_via_lds<VDV, true>(smem + w * 32 * VDV * 2, vals, o + u.obase, q0 + 32 * w, nq, lane, DVR, -1, u.so);
    if (qrow < nq && h == 0) lse[u.lbase + qrow] = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
}

// ------------------------------------------------------------------------------------------------ dK / dV
template <typename Tag, bool VAR>
__global__ __launch_bounds__(512, 2) void exv_dkdv_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                          const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                          const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                          uint16_t* __restrict__ dk, uint16_t* __restrict__ dv, VdParams p,
                                                          float c_log2) {
    constexpr int NW = 8, BK = 32 * NW, BQ = 32, NKS = VD / 16, NVS = VDV / 16, NDB = VD / 32, NVB = VDV / 32;
    using KT = Tile192<BK>;
    using QT = Tile192<BQ>;
    constexpr int K_BYTES = KT::BYTES, Q_BYTES = QT::BYTES, O_BYTES = BQ * VDV * 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                      // [256][192]
    char* Qs = Ks + K_BYTES;              // [2][32][192]
    char* Os = Qs + 2 * Q_BYTES;          // [2][32][128]   (dO)
    float* Ls = reinterpret_cast<float*>(Os + 2 * O_BYTES);  // [2][ 64 x -lse/scale | 64 x -delta ] (the first 32 of each are the tile's)
    const int nkt = (p.nk + BK - 1) / BK;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nkt;
    const int key0 = (L - bh * nkt) * BK;
    VdUnit u;
    vd_unit<VAR>(p, bh, u);
    const int nq = u.nq, nk = u.nk, coff = u.coff;
    if (VAR && key0 >= nk) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int DR = p.d, DVR = p.dv;
    const int kw0 = key0 + 32 * w, key = kw0 + r;

    const Src192 ksrc = make_src192(k + u.kbase, nk, DR, u.sk, lane, w);
    const Src192 qsrc = make_src192(q + u.qbase, nq, DR, u.sq, lane, w);
    const rsrc_s_t o_rs = make_rsrc_s(dout + u.obase, span_bytes(nq, DVR, u.so));
    const rsrc_s_t l_rs = make_rsrc_s(nlse + u.lbase, (unsigned)nq * 4);
    const rsrc_s_t d_rs = make_rsrc_s(ndelta + u.lbase, (unsigned)nq * 4);
    const buf_rsrc_t v_rs = make_rsrc(v + u.vbase, span_bytes(nk, DVR, u.sv));
    const int voff_o = dma_lane_voff<VDV, true>(lane, w, DVR, u.so);
    auto stage = [&](int buf, int qs) {
        stage192<BQ, NW>(qsrc, Qs + buf * Q_BYTES, qs, w);
        dma_stage_tile<VDV, BQ, NW, true>(o_rs, Os + buf * O_BYTES, qs, voff_o, w, VDV, 0, u.so);
        // row constants: one 4-byte LDS-DMA per lane (rows >= nq read as 0: harmless, their dO is 0)
        if (w == 6) dma4_issue(l_rs, lds_addr_of(Ls + buf * 128), lane * 4, __builtin_amdgcn_readfirstlane(qs * 4));
        if (w == 7) dma4_issue(d_rs, lds_addr_of(Ls + buf * 128 + 64), lane * 4, __builtin_amdgcn_readfirstlane(qs * 4));
    };

    stage192<BK, NW>(ksrc, Ks, key0, w);
    s16x8 vf[NVS];
#pragma unroll
    for (int ks = 0; ks < NVS; ++ks) vf[ks] = buf_load_frag(v_rs, frag_off<true>(key, 16 * ks + 8 * h, DVR, true, u.sv));

    f32x16 dka[NDB], dva[NVB];
#pragma unroll
    for (int t = 0; t < NDB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dka[t][i] = 0.f;
#pragma unroll
    for (int t = 0; t < NVB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dva[t][i] = 0.f;

    // key j is visible from row j - coff on: earlier query tiles see none of this workgroup's (this wave's) keys
    const int qs_first = p.causal ? (max(0, key0 - coff) / BQ) * BQ : 0;
    const int ntile = qs_first < nq ? (nq - qs_first + BQ - 1) / BQ : 0;
    const int it_first = p.causal ? max(0, kw0 - coff) / BQ - qs_first / BQ : 0;
    const OpBase ob0 = make_op_base(lane);

    int it = 0, cur = 0;
    if (it < ntile) stage(0, qs_first);
    dma_wait_all();
    __syncthreads();
    // feed-only iterations first (tiles before this wave's first visible row), then the computing ones
    while (it < min(it_first, ntile)) {
        const int itn = it + 1;
        if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        it = itn;
    }
    while (it < ntile) {
        const int itn = it + 1;
        if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
        const int rb0 = qs_first + it * BQ;        // first row of the block; register i holds row rb0 + 4 h + rc(i)
        const char* Qt = Qs + cur * Q_BYTES;
        const char* Ot = Os + cur * O_BYTES;
        const float* Lt = Ls + cur * 128;
        // masked: the row precedes the key's first visible row (causal), or the key lies past nk: rc(i) < thr
        const bool need_mask = (p.causal && (kw0 + 31 - coff > rb0)) || (kw0 + 32 > nk);
        const int thr = !need_mask ? -1 : (key >= nk ? 64 : (p.causal ? key - coff - rb0 - 4 * h : -1));
        OpBase ob = ob0;
        opaque(ob);
        int kw = 32 * w;
        asm volatile("" : "+v"(kw));
        u32x4 pp[2], sp[2];
        {
            f32x16 sacc;
            // seeded with -lse / scale
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(Lt + 8 * g + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) sacc[4 * g + j] = a[j];
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const s16x8 qa = row_frag192<BQ>(Qt, ob, 0, ks);
                const s16x8 kf = row_frag192<BK>(Ks, ob, kw, ks);
                sacc = mfma32<Tag>(qa, kf, sacc);
            }
            if (!need_mask) {   // wave-uniform
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[i] = __builtin_amdgcn_exp2f(sacc[i] * c_log2);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[i] = rc_of(i) < thr ? 0.f : __builtin_amdgcn_exp2f(sacc[i] * c_log2);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) pp[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
        }
        {
            f32x16 pacc;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(Lt + 64 + 8 * g + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) pacc[4 * g + j] = a[j];
            }
#pragma unroll
            for (int ks = 0; ks < NVS; ++ks) {
                const s16x8 oa = row_frag128(Ot, ob, 0, ks);
                pacc = mfma32<Tag>(oa, vf[ks], pacc);
            }
            if constexpr (std::is_same<Tag, f16_tag>::value) mfma_result_fence(pacc);   // mul_pack<f16> reads pacc from asm
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) sp[s][j] = mul_pack<Tag>(pp[s][j], pacc[8 * s + 2 * j], pacc[8 * s + 2 * j + 1]);
            if constexpr (std::is_same<Tag, f16_tag>::value) asm volatile("s_nop 1" : "+v"(sp[0]), "+v"(sp[1]));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const s16x8 pb = *reinterpret_cast<s16x8*>(&pp[s]);
            const s16x8 sb = *reinterpret_cast<s16x8*>(&sp[s]);
#pragma unroll
            for (int db = 0; db < NVB; ++db) dva[db] = mfma32<Tag>(tr_frag128(Ot, ob, 16 * s, db), pb, dva[db]);
#pragma unroll
            for (int db = 0; db < NDB; ++db) dka[db] = mfma32<Tag>(tr_frag192<BQ>(Qt, ob, 16 * s, db), sb, dka[db]);
            __builtin_amdgcn_sched_barrier(0);
        }
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        it = itn;
    }

    if (key < nk) {
        // dK / dV rows: per query head (grouped: the partials kv_group_sum adds up), each at its own width
        // (varlen: rows of (total_k, hq, d) and (total_k, hq, d_v) — the partials, or dk / dv themselves when hq = hkv)
        const size_t krow = VAR ? (size_t)(u.sk0 + key) * p.hq + u.hh : (size_t)bh * nk + key;
        uint16_t* dkrow = dk + krow * DR;
        uint16_t* dvrow = dv + krow * DVR;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 a;
                a[0] = pack2_rn<Tag>(dka[db][4 * g + 0] * p.scale, dka[db][4 * g + 1] * p.scale);
                a[1] = pack2_rn<Tag>(dka[db][4 * g + 2] * p.scale, dka[db][4 * g + 3] * p.scale);
                if (32 * db + 8 * g + 4 * h >= DR) continue;   // padded columns (DR is a multiple of 8)
                *reinterpret_cast<u32x2*>(dkrow + 32 * db + 8 * g + 4 * h) = a;
            }
#pragma unroll
        for (int db = 0; db < NVB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 b;
                b[0] = pack2_rn<Tag>(dva[db][4 * g + 0], dva[db][4 * g + 1]);
                b[1] = pack2_rn<Tag>(dva[db][4 * g + 2], dva[db][4 * g + 3]);
                if (32 * db + 8 * g + 4 * h >= DVR) continue;
                *reinterpret_cast<u32x2*>(dvrow + 32 * db + 8 * g + 4 * h) = b;
            }
    }
}

// ------------------------------------------------------------------------------------------------ dQ
template <typename Tag, bool VAR>
__global__ __launch_bounds__(512, 2) void exv_dq_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                        const uint16_t* __restrict__ v, const uint16_t* __restrict__ dout,
                                                        const float* __restrict__ nlse, const float* __restrict__ ndelta,
                                                        uint16_t* __restrict__ dq, VdParams p, float c_log2) {
    constexpr int NW = 8, BM = 32 * NW, BN = 64, NKS = VD / 16, NVS = VDV / 16, NDB = VD / 32;
    using KT = Tile192<BN>;
    constexpr int K_BYTES = KT::BYTES, V_BYTES = BN * VDV * 2, BUF_BYTES = K_BYTES + V_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][K tile | V tile][8 waves x 8 dO fragments x 1 KiB]
    const int nqt = (p.nq + BM - 1) / BM;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;
    const int q0 = (L - bh * nqt) * BM;
    VdUnit u;
    vd_unit<VAR>(p, bh, u);
    const int nq = u.nq, nk = u.nk, coff = u.coff;
    if (VAR && q0 >= nq) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int DR = p.d, DVR = p.dv;
    const int qrow = q0 + 32 * w + r;
    const bool live_row = qrow < nq;

    const buf_rsrc_t q_rs = make_rsrc(q + u.qbase, span_bytes(nq, DR, u.sq));
    const buf_rsrc_t o_rs = make_rsrc(dout + u.obase, span_bytes(nq, DVR, u.so));
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = buf_load_frag(q_rs, frag_off<true>(qrow, 16 * ks + 8 * h, DR, true, u.sq));
    // the lane's dO fragments live in LDS, not in registers (Q's 48 and the 96 of dQ leave no room for their 32): fragment ks of
    // wave w at Of + (w NVS + ks) 1 KiB + 16 lane — written and read by the same lane, lane-linear, no barrier
    char* Of = smem + 2 * BUF_BYTES + w * NVS * 1024 + lane * 16;
#pragma unroll
    for (int ks = 0; ks < NVS; ++ks)
        *reinterpret_cast<s16x8*>(Of + ks * 1024) = buf_load_frag(o_rs, frag_off<true>(qrow, 16 * ks + 8 * h, DVR, true, u.so));
    const float nl = live_row ? nlse[u.lbase + qrow] : 0.f;
    const float nd = live_row ? ndelta[u.lbase + qrow] : 0.f;

    const Src192 ksrc = make_src192(k + u.kbase, nk, DR, u.sk, lane, w);
    const rsrc_s_t v_rs = make_rsrc_s(v + u.vbase, span_bytes(nk, DVR, u.sv));
    const int voff_v = dma_lane_voff<VDV, true>(lane, w, DVR, u.sv);
    auto stage = [&](int buf, int k0) {
        char* kb_ = smem + buf * BUF_BYTES;
        stage192<BN, NW>(ksrc, kb_, k0, w);
        dma_stage_tile<VDV, BN, NW, true>(v_rs, kb_ + K_BYTES, k0, voff_v, w, VDV, 0, u.sv);
    };

    f32x16 dqa[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dqa[t][i] = 0.f;

    const int kend = p.causal ? max(0, min(nk, q0 + BM + coff)) : nk;
    const int kend_w = p.causal ? max(0, min(nk, q0 + 32 * w + 32 + coff)) : nk;
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const OpBase ob0 = make_op_base(lane);

    int t = 0, cur = 0;
    if (t < ntiles) stage(0, 0);
    dma_wait_all();
    __syncthreads();
    while (t < ntiles_w) {
        const int tn = t + 1;
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * BUF_BYTES;
        const char* Vt = Kt + K_BYTES;
        OpBase ob = ob0;
        opaque(ob);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            u32x4 dsb[2];
            {
                f32x16 sacc, pacc;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sacc[i] = nl;
                    pacc[i] = nd;
                }
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) sacc = mfma32<Tag>(row_frag192<BN>(Kt, ob, 32 * kb, ks), qf[ks], sacc);
#pragma unroll
                for (int ks = 0; ks < NVS; ++ks) {
                    const s16x8 of = *reinterpret_cast<const s16x8*>(Of + ks * 1024);
                    pacc = mfma32<Tag>(row_frag128(Vt, ob, 32 * kb, ks), of, pacc);
                }
                const bool need_mask = (p.causal && (k0 + 32 * kb + 31 > q0 + 32 * w + coff)) || (k0 + 32 * kb + 32 > nk);
                if (!need_mask) {   // wave-uniform
#pragma unroll
                    for (int i = 0; i < 16; ++i) pacc[i] = __builtin_amdgcn_exp2f(sacc[i] * c_log2) * pacc[i];
                } else {
                    const int lim = p.causal ? min(qrow + coff, nk - 1) : nk - 1;
                    const int thr = lim - (k0 + 32 * kb + 4 * h);
#pragma unroll
                    for (int i = 0; i < 16; ++i) pacc[i] = rc_of(i) > thr ? 0.f : __builtin_amdgcn_exp2f(sacc[i] * c_log2) * pacc[i];
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) dsb[s][j] = pack2<Tag>(pacc[8 * s + 2 * j], pacc[8 * s + 2 * j + 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const s16x8 sb = *reinterpret_cast<s16x8*>(&dsb[s]);
#pragma unroll
                for (int db = 0; db < NDB; ++db) dqa[db] = mfma32<Tag>(tr_frag192<BN>(Kt, ob, 32 * kb + 16 * s, db), sb, dqa[db]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    while (t < ntiles) {
        const int tn = t + 1;
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    // the epilogue's row and half come from the lane id afresh (mbcnt), so that nothing but the loop's own state lives across the
    // loop: carried over, the row's address was what spilled
    const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int qrow_e = q0 + 32 * w + (lane_e & 31), h_e = lane_e >> 5;
    if (qrow_e < nq) {
        uint16_t* drow = dq + u.dqbase + (size_t)qrow_e * u.sdq;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int h = h_e;
                if (32 * db + 8 * g + 4 * h >= DR) continue;
                u32x2 val;
                val[0] = pack2_rn<Tag>(dqa[db][4 * g + 0] * p.scale, dqa[db][4 * g + 1] * p.scale);
                val[1] = pack2_rn<Tag>(dqa[db][4 * g + 2] * p.scale, dqa[db][4 * g + 3] * p.scale);
                *reinterpret_cast<u32x2*>(drow + 32 * db + 8 * g + 4 * h) = val;
            }
    }
}

VdParams make_vd_params(const ExArgs& a) {
    VdParams p;
    p.nq = (int)a.nq; p.nk = (int)a.nk; p.d = (int)a.d; p.dv = (int)a.d_v;
    p.causal = a.causal ? 1 : 0;
    p.coff = (int)(a.nk - a.nq);
    p.hq = (int)a.heads_q;
    p.total_q = (int)a.total_q; p.total_k = (int)a.total_k;
    p.sq = (int)a.stride_q; p.sk = (int)a.stride_k; p.sv = (int)a.stride_v;
    p.cu_q = a.cu_q; p.cu_k = a.cu_k;
    p.scale = a.scale;
    p.kvg = kv_magic(a.kv_group);
    return p;
}

constexpr size_t kFwdSmem = 2 * (Tile192<64>::BYTES + 64 * VDV * 2);                                       // 80 KiB
constexpr size_t kDkdvSmem = Tile192<256>::BYTES + 2 * Tile192<32>::BYTES + 2 * 32 * VDV * 2 + 2 * 128 * sizeof(float);   // 137 KiB
constexpr size_t kDqSmem = kFwdSmem + 8 * (VDV / 16) * 1024;                                                // + the dO fragments: 144 KiB
static_assert(kFwdSmem >= 8 * 32 * VDV * 2, "the forward's epilogue stages 32 x DV per wave in the tile memory");
static_assert(kDkdvSmem <= 160 * 1024, "LDS of a CU");

template <typename Tag, bool VAR>
hipError_t exv_fwd_t(const ExArgs& a, hipStream_t st) {
    auto kern = exv_fwd_kernel<Tag, VAR>;
    hipError_t e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)kFwdSmem);
    if (e != hipSuccess) return e;
    ProfScope ps(K_EX_FWD, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nq + 255) / 256) * a.bh)), dim3(512), kFwdSmem, st, (const uint16_t*)a.q,
                       (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.o, a.lse, make_vd_params(a), a.scale * 1.4426950408889634f);
    return hipGetLastError();
}

// a.dk / a.dv: one unit per query head (the caller's tensors when kv_group = 1, else the partial slabs)
template <typename Tag, bool VAR>
hipError_t exv_bwd_t(const ExArgs& a, hipStream_t st) {
    const long long rows = VAR ? (long long)a.heads_q * a.total_q : (long long)a.bh * a.nq;
    float* nlse = reinterpret_cast<float*>(a.workspace);
    float* ndelta = nlse + ((rows + 63) & ~63ll);
    const VdParams p = make_vd_params(a);
    const float c = a.scale * 1.4426950408889634f;
    ProfScope ps(K_EX_BWD, st);
    hipError_t e = launch_exm_prep(a, a.d_v, nlse, ndelta, st);
    if (e != hipSuccess) return e;
    {
        auto kern = exv_dkdv_kernel<Tag, VAR>;
        e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)kDkdvSmem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nk + 255) / 256) * a.bh)), dim3(512), kDkdvSmem, st, (const uint16_t*)a.q,
                           (const uint16_t*)a.k, (const uint16_t*)a.v, (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta,
                           (uint16_t*)a.dk, (uint16_t*)a.dv, p, c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    auto kern = exv_dq_kernel<Tag, VAR>;
    e = ensure_dynamic_smem(reinterpret_cast<const void*>(kern), (int)kDqSmem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(((a.nq + 255) / 256) * a.bh)), dim3(512), kDqSmem, st, (const uint16_t*)a.q,
                       (const uint16_t*)a.k, (const uint16_t*)a.v, (const uint16_t*)a.dout, (const float*)nlse, (const float*)ndelta,
                       (uint16_t*)a.dq, p, c);
    return hipGetLastError();
}

template <typename Tag>
hipError_t exv_one(const ExArgs& a, bool backward, hipStream_t st) {
    if (a.cu_q) return backward ? exv_bwd_t<Tag, true>(a, st) : exv_fwd_t<Tag, true>(a, st);
    return backward ? exv_bwd_t<Tag, false>(a, st) : exv_fwd_t<Tag, false>(a, st);
}

}  // namespace

// What the kernels take, beyond the widths and features the C layer has checked by name: a positive scale (the running max is
// taken on the raw scores), 16-byte rows and tensors, and the 32-bit buffer offsets inside one unit / one sequence.
bool ex_vdim_supported(const ExArgs& a) {
    if (a.dtype != 1 && a.dtype != 2) return false;
    if (a.d_v < 8 || a.d_v >= a.d || a.d > VD || a.d_v > VDV || a.d % 8 != 0 || a.d_v % 8 != 0) return false;
    if (!(a.scale > 0.f)) return false;
    if (a.mask || a.block_mask || a.dropout_p > 0.0 || ex_windowed(a) || ex_scoremod(a) || a.sinks || a.block_table || a.kv_e4m3) return false;
    const void* ptrs[] = {a.q, a.k, a.v, a.o, a.dout, a.dq, a.dk, a.dv};
    for (const void* ptr : ptrs)
        if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) return false;
    int64_t smax = a.d;
    if (a.cu_q) {
        if (a.stride_q % 8 != 0 || a.stride_k % 8 != 0 || a.stride_v % 8 != 0) return false;
        smax = a.heads_q * a.d;
        if (a.stride_q > smax) smax = a.stride_q;
        if (a.stride_k > smax) smax = a.stride_k;
        if (a.stride_v > smax) smax = a.stride_v;
    }
    const int64_t nmax = a.nq > a.nk ? a.nq : a.nk;
    return (nmax + 256) * smax * 2 < ((int64_t)1 << 31);
}

// (the caller has checked ex_vdim_supported, and that no side is empty)
hipError_t launch_ex_vdim(const ExArgs& a, bool backward, hipStream_t st) {
    auto one = [&](const ExArgs& x) { return a.dtype == 2 ? exv_one<bf16_tag>(x, backward, st) : exv_one<f16_tag>(x, backward, st); };
    if (!backward || a.kv_group <= 1) return one(a);
    // Grouped backward.  Workspace: [dK partials][dV partials][the row constants], the slabs sized as the call with d_v = d sizes
    // them (fa_ex_backward_workspace_bytes_grouped / _varlen with q's width); the kernels write one dK / dV unit per query head,
    // then one group sum per tensor, each at its own width.
    const bool var = a.cu_q != nullptr;
    const size_t slab = var ? kv_partial_bytes(a.total_k * a.heads_q, 1, a.d, a.dtype) : kv_partial_bytes(a.bh, a.nk, a.d, a.dtype);
    if (a.workspace_bytes < 2 * slab) return hipErrorInvalidValue;
    ExArgs g = a;
    g.dk = a.workspace;
    g.dv = reinterpret_cast<char*>(a.workspace) + slab;
    g.workspace = reinterpret_cast<char*>(a.workspace) + 2 * slab;
    g.workspace_bytes = a.workspace_bytes - 2 * slab;
    hipError_t e = one(g);
    if (e != hipSuccess) return e;
    const int64_t units = var ? a.total_k * (a.heads_q / a.kv_group) : a.bh / a.kv_group;
    const int64_t rows = var ? 1 : a.nk;
    e = launch_kv_group_sum_one(g.dk, a.dk, units, a.kv_group, rows, a.d, a.dtype, st);
    if (e != hipSuccess) return e;
    return launch_kv_group_sum_one(g.dv, a.dv, units, a.kv_group, rows, a.d_v, a.dtype, st);
}

}  // namespace fa
