// The MXFP4 KV cache at head dims 64 and 256 (fa_fp4_kvcache_append_hdim, fa_fp4_forward_kvcache_hdim, fa_fp4_forward_varlen_hdim;
// include/fa_mi355x.h).  The cache is fa_fp4_decode.hip's at width d: k_cache / v_cache (.., H_kv, d / 2) codes,
// k_scale (.., H_kv, d / 32), v_scale (.., H_kv) with ONE byte a (token, head) over all d channels: 67 bytes a token and head at
// d = 64, 265 at d = 256.  The exponent, tie, descale and trust rules, the joint-maximum softmax, the split cut, the combine and the
// graph-replay property are those of fa_fp4_decode.hip's and fa_fp4_prefill.hip's headers; what follows is what differs from the 128
// kernels, which stay in their files with their instructions.  A call at d = 128 through these launchers IS the 128 call.
//
//   fp4kv_append_hdim_kernel<Tag, D>   one thread per 32-channel block, 2 D / 32 = 4 / 16 live lanes a (token, head): NB = D / 32
//                                      lanes of K, then NB of V.  V's amax is a butterfly over the NB lanes (xor 1 .. NB / 2, inside
//                                      an aligned group of NB); the early return cuts whole groups of 2 NB lanes (2 NB divides 64).
//   fp4kv_split_hdim_kernel<Tag, PAGED, D, Mod...>   fp4kv_split_kernel's wave: 32 rows x 64-key tiles, lane l = (r = l & 31, h = l >> 5).
//   fp4kv_prefill_hdim_kernel<Tag, D, Mod...>        fp4kv_prefill_kernel's workgroup: 4 waves x 32 rows, the three-deep ring, one barrier a tile.
//
// S^T = K Q^T, NM = D / 64 instructions a 32-key block.  Instruction M takes channels 64 M .. 64 M + 63: the fp4 A operand of lane
// half h is the 16 code bytes at 32 M + 16 h of the key's D / 2, which is MX block 2 M + h, so its E8M0 operand is byte 2 M + h of the
// key's k_scale row: at D = 64 ONE instruction, block h, byte h of a 2-byte row (a ushort load); at D = 256 four, the row is two dwords
// and instruction M reads dword M >> 1.  The e4m3 B operand of instruction M is q at channels 64 M + 16 h and 64 M + 32 + 16 h.
//
// O^T = V^T P'^T, D / 32 instructions out of the V^T image: D rows (channels) x 32 key bytes at vt4_off(row) = 32 row + 16 (row >> 3),
// row byte 16 h + 8 hv + 2 j + cc = keys 32 h + 4 hv + 8 j + 2 cc (low nibble) and + 1 (high nibble), as at 128.
//   D = 256 (decode)  two passes of the 128 kernel's transpose, channels 128 pass + 8 rd ..: the second pass lies 128 rows = 17 x 256
//                     bytes on, so each pass has the 128 image's banks: 8-byte writes of 32 lanes and 16-byte reads of 16 lanes
//                     cover the 64 banks once.  One pass is live at a time (16 dwords a lane).
//   D = 64 (decode)   64 rows: the 128 map (8 channels x 16 keys a lane) would leave 32 lanes idle.  Lane (rd = l & 7, hv = (l >> 3) & 1,
//                     g4 = l >> 4) loads the dword at channels 8 rd .. of the EIGHT keys 4 hv + 8 jj + c (jj < 2, c < 4) of 16-key group
//                     g4 = 2 h + jp; one 4 x 4 byte transpose each for the even and the odd channels gives a dword a channel, written
//                     at row byte 16 h + 8 hv + 4 jp.  Banks: the 16-byte reads of lanes r = 0 .. 15 land at 32 r + 16 (r >> 3) mod
//                     256, every bank once, as at 128.  The dword writes of the 64 lanes land at dword 4 rd + q + 16 m mod 64 with
//                     q = 4 h + 2 hv + jp in 0 .. 7: banks 0 .. 35, at most two lanes a bank, so a write takes two passes where the
//                     128 kernel's takes one.  No padding of 32-byte rows clears both: the reads need rows r and r + 8 an odd
//                     multiple of 16 bytes apart mod 32, the writes need the row groups 8 rd a multiple of 32 apart.  Eight dword
//                     writes a lane and tile against 64 operand bytes read: the reads keep the clean pattern.
//   prefill           wave w stages 16-key group w.  K: 16 keys x D / 32 chunks of 16 bytes, chunk id = lane + 64 i -> (key id / (D /
//                     32), chunk id % (D / 32)): lanes 0 .. 31 at 64, two chunks a lane at 256.  A K stage row is D / 2 code bytes +
//                     D / 32 scale bytes padded to an ODD multiple of 16: 48 at 64, 144 at 256, so the 16-byte operand reads of 16
//                     lanes land at sixteen different multiples of 16 mod 256.  V at 256: the 128 loader's map twice (channels 128
//                     pass + 8 rd ..), eight dwords a lane.  V at 64: lane (rd = l & 7, hv = (l >> 3) & 1, jl = (l >> 4) & 1, cc = l >> 5)
//                     loads channels 8 rd .. of the TWO keys 4 hv + 8 jl + 2 cc (+ 1); mask / shift / or give a byte a channel, written
//                     at row byte 16 h + 8 hv + 2 j + cc with h = w >> 1, j = 2 (w & 1) + jl.  LDS: 2 x (64 x 48 + 2176 + 256) = 11008
//                     bytes at 64, 2 x (64 x 144 + 8704 + 256) = 36352 at 256.
//
// Registers at D = 256: O^T is 8 x 16 = 128 fp32 accumulators, q four operands (32), a tile's scores and exponents 64 more: beyond the
// 256 of two waves a SIMD.  Both readers run ONE wave a SIMD there (__launch_bounds__(.., 1): 512 registers, the accumulators in
// AGPRs), as the e4m3 kernel does at 256.  The other way, the value channels split over two waves, reads K and runs S twice or hands
// P' through LDS behind a barrier a tile; the decode wave has no barrier today and is bound by the cache bytes it pulls, which the
// split count, not the occupancy, spreads over the chip.  D = 64 keeps two waves a SIMD.  No kernel here uses scratch.
#include <climits>

#include "fa_kvq_common.h"

namespace fa {

namespace {

template <int D> struct Fp4Hd {
    static_assert(D == 64 || D == 256, "the 128 kernels live in fa_fp4_decode.hip / fa_fp4_prefill.hip");
    static constexpr int KT = 64, NM = D / 64, NDV = D / 32, HB = D / 2, SB = D / 32;   // HB / SB: code / k_scale bytes a key and head
    static constexpr int VT = 34 * D;                      // the V^T image: vt4_off(D)
    static constexpr int KROW = D == 64 ? 48 : 144;        // a key's row in the prefill K stage
    static constexpr int WAVES = D == 256 ? 1 : 2;         // a SIMD
};

// a key's k_scale row (D / 32 bytes, global or LDS) as two words
template <int D> __device__ __forceinline__ void fp4h_scale_row(const void* sp, uint32_t (&w)[2]) {
    if constexpr (D == 64) {
        w[0] = *reinterpret_cast<const uint16_t*>(sp);
        w[1] = 0u;
    } else {
        const u32x2 x = *reinterpret_cast<const u32x2*>(sp);
        w[0] = x[0];
        w[1] = x[1];
    }
}

// the lane's e4m3 q operands: qp = the row's D bytes + 16 h
template <int NM> __device__ __forceinline__ void fp4h_load_q(const uint8_t* qp, bool valid, i32x8_t (&qb)[NM]) {
#pragma unroll
    for (int M = 0; M < NM; ++M) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(qp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(qp + 64 * M + 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qb[M][i] = valid ? (int)a0[i] : 0;
            qb[M][4 + i] = valid ? (int)a1[i] : 0;
        }
    }
}

// S^T of one 32-key block: a[M] the lane's 16 code bytes at 32 M + 16 h, w its key's scale row; instruction M's block is 2 M + h
template <int NM> __device__ __forceinline__ f32x16 fp4h_scores(const u32x4 (&a)[NM], const uint32_t (&w)[2], int h, const i32x8_t (&qb)[NM]) {
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int M = 0; M < NM; ++M) {
        const i32x8_t ka = {(int)a[M][0], (int)a[M][1], (int)a[M][2], (int)a[M][3], 0, 0, 0, 0};
        const int sc = (int)((w[M >> 1] >> (16 * (M & 1) + 8 * h)) & 0xffu);
        s = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb[M], s, kFp4, 0, 0, sc, 0, 127);
    }
    return s;
}

// what the softmax of a lane's row needs beside the scores
struct Fp4hRow {
    bool valid, capped;
    int rhi, rlo;                         // the row sees keys [rlo, rhi] (rlo: a window alone)
    float fe, ck, cap2;
};

// One 64-key tile from its scores on: softcap, mask, t = s f + ev under the joint running maximum with the lazy rescale, P' rounded
// to e4m3, l from the unrounded ldexp, O^T += V^T P'^T out of the image.  fp4kv_split_kernel's arithmetic, statement for statement.
template <int D>
__device__ __forceinline__ void fp4h_softmax_pv(f32x16 (&sacc)[2], const int* evb, const char* vtb, f32x16 (&oacc)[D / 32], float& m_run,
                                                float& l_run, const Fp4hRow& rw, int k0, int r, int h, bool need_mask, bool need_lo) {
    if (rw.capped) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * rw.ck) + 1.f);
                sacc[kb][i] = fmaf(rr, -2.f * rw.cap2, rw.cap2);
            }
    }
    int ev[2][16];
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i32x4_t e4 = *reinterpret_cast<const i32x4_t*>(evb + 32 * kb + 4 * h + 8 * j);
#pragma unroll
            for (int c = 0; c < 4; ++c) ev[kb][4 * j + c] = e4[c];
        }
        if (need_mask) {
            const int thr = rw.rhi - (k0 + 32 * kb + 4 * h);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
        }
        if (need_lo) {
            const int thr = rw.rlo - (k0 + 32 * kb + 4 * h);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((i & 3) + 8 * (i >> 2) < thr) sacc[kb][i] = -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sacc[kb][i] = fmaf(sacc[kb][i], rw.fe, (float)ev[kb][i]);   // (a masked key stays -inf whatever its ev: fe > 0)
            mx = fmaxf(mx, sacc[kb][i]);
        }
    }
    mx = fmaxf(mx, wave_half_swap(mx));
    const float m_new = fmaxf(m_run, mx);
    float m_use;
    if (__any(rw.valid && m_new - m_run > 8.0f) != 0) {   // lazy rescale on the real rows; a row's first visible key: inf > 8
        m_use = m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int t2 = 0; t2 < D / 32; ++t2)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[t2][i] *= alpha;
    } else {
        m_use = m_run;
    }
    if (m_use == -INFINITY) m_use = 0.f;      // a row without a visible key so far: p = exp2(-inf) = 0, not exp2(-inf + inf)
    float rs = 0.f;
    i32x8_t pb;                               // P'^T as the accumulators hold it, rounded to e4m3 (RNE)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float pe = __builtin_amdgcn_exp2f(sacc[kb][i] - m_use);
            sacc[kb][i] = pe;
            rs += __builtin_ldexpf(pe, -ev[kb][i]);          // the key's share of l: exp2(s f - M), V's scale taken out again
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int wd = 0;
            wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 0], sacc[kb][4 * j + 1], wd, false);
            wd = __builtin_amdgcn_cvt_pk_fp8_f32(sacc[kb][4 * j + 2], sacc[kb][4 * j + 3], wd, true);
            pb[4 * kb + j] = wd;
        }
    }
    l_run += rs;
#pragma unroll
    for (int dvb = 0; dvb < D / 32; ++dvb) {
        const u32x4 a0 = *reinterpret_cast<const u32x4*>(vtb + vt4_off(32 * dvb + r) + 16 * h);
        const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], 0, 0, 0, 0};
        oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], kFp4, 0, 0, 127, 0, 127);
    }
}

// a lane's row of O^T out: register i of block dvb is channel 32 dvb + 4 h + (i & 3) + 8 (i >> 2); scaled by inv, zeros if dead
template <typename Tag, int NDV> __device__ __forceinline__ void fp4h_store_o(uint16_t* orow, const f32x16 (&oacc)[NDV], float inv, bool dead, int h) {
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
            u32x2 v;
            v[0] = pack2_rn<Tag>(y[0], y[1]);
            v[1] = pack2_rn<Tag>(y[2], y[3]);
            *reinterpret_cast<u32x2*>(orow + 32 * dvb + 8 * g + 4 * h) = v;
        }
}

// four keys' dwords (eight channels each) to the even-channel and odd-channel dwords of key pairs (0, 1) and (2, 3), two keys a byte
__device__ __forceinline__ void fp4h_pair_nibbles(const uint32_t (&x)[4], uint32_t& e01, uint32_t& o01, uint32_t& e23, uint32_t& o23) {
    constexpr uint32_t LO = 0x0f0f0f0fu;
    e01 = (x[0] & LO) | ((x[1] & LO) << 4);
    o01 = ((x[0] >> 4) & LO) | (x[1] & ~LO);
    e23 = (x[2] & LO) | ((x[3] & LO) << 4);
    o23 = ((x[2] >> 4) & LO) | (x[3] & ~LO);
}

// ---- split-KV decode ------------------------------------------------------------------------------------------------------------
template <typename Tag, bool PAGED, int D, typename... Mod>
__global__ __launch_bounds__(64, Fp4Hd<D>::WAVES) void fp4kv_split_hdim_kernel(const Fp4KvParams p, const Mod... mod) {
    constexpr bool MOD = sizeof...(Mod) != 0;                     // the featured instantiation: (KvqMod) follows p
    static_assert(sizeof...(Mod) <= 1, "Mod...: nothing, or (KvqMod)");
    const KvqMod md = kvq_mod_of<KvqMod>(mod...);
    using C = Fp4Hd<D>;
    constexpr int KT = C::KT, NM = C::NM, NDV = C::NDV, HB = C::HB, SB = C::SB;
    __shared__ __attribute__((aligned(16))) char vt[C::VT];       // V^T tile, [channel][32 key bytes in P's key order]
    __shared__ __attribute__((aligned(16))) int evs[KT];          // the tile's V exponents, by key
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int nq = p.nq, rows = p.rows, G = p.G;
    const int pr0 = 32 * rt, pr = pr0 + r;                        // (the grid has ceil(rows / 32) row tiles: pr0 < rows)

    int lk = p.seqlens ? min(max(p.seqlens[b], 0), p.cap) : p.cap;
    long long crow = b;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; lk = 0; }   // an index outside the cache: an empty sequence
    }
    const int coff = lk - nq;                                     // causal: token i sees key j <= i + coff; MOD: [i + coff - wl, i + coff + wr]
    const int qlo = pr0 / G, qhi = (min(pr0 + 32, rows) - 1) / G;
    // the split's keys [kbeg, kend): the tile's visible keys [lo, hi) cut into 64-key tiles, as in fp4kv_split_kernel
    const int hi = MOD ? max(0, min(lk, qhi + coff + md.wr + 1)) : p.causal ? max(0, min(lk, qhi + coff + 1)) : lk;
    const int lo = MOD ? max(0, qlo + coff - md.wl) & ~(KT - 1) : 0;
    const int nt = MOD ? (hi > lo ? (hi - lo + KT - 1) / KT : 0) : (hi + KT - 1) / KT;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    const int kbeg = lo + t0 * KT, kend = min(hi, lo + t1 * KT);

    const bool valid = pr < rows;
    // (a padding row takes the tile's first token: its scores are masked like a real row's, and nothing of it is stored)
    const int qi = valid ? pr / G : qlo, hd = hk * G + (valid ? pr - qi * G : 0);
    i32x8_t qb[NM];
    fp4h_load_q<NM>(p.q + (long long)b * p.q_bs + (long long)qi * p.q_ts + hd * D + 16 * h, valid, qb);
    const float qd = p.qds ? p.qds[b * p.qds_bs + hk] : 1.f;
    const float kd = p.kds ? p.kds[b * p.kds_bs + hk] : 1.f;
    const float vd = p.vds ? p.vds[b * p.vds_bs + hk] : 1.f;
    const float f = (p.c_log2 * qd) * kd;                         // the one score factor of this wave, > 0
    Fp4hRow rw;
    rw.valid = valid;
    rw.capped = MOD && md.cap2 != 0.f;
    rw.rhi = MOD ? min(min(qi + coff + md.wr, lk - 1), kend - 1) : min(p.causal ? qi + coff : lk - 1, kend - 1);
    rw.rlo = qi + coff - md.wl;
    rw.ck = f * md.cap_k;
    rw.cap2 = md.cap2;
    rw.fe = rw.capped ? 1.f : f;                                  // the factor of what the accumulators hold after the cap

    // byte offsets of the first token of the tile's four 16-key groups in the four arrays (wave-uniform); kB < 0: the group
    // reads as zero codes with unit scales (past the split's end, or a page outside the pool)
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    auto group_bases = [&](int k0, i64x4_t& kB, i64x4_t& sB, i64x4_t& vB, i64x4_t& eB) {
        int j0 = 0, s0 = 0;
        if (PAGED) { j0 = k0 / p.ps; s0 = k0 - j0 * p.ps; }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int key0 = k0 + 16 * g4;
            kB[g4] = -1; sB[g4] = 0; vB[g4] = 0; eB[g4] = 0;
            if (key0 < kend) {
                long long pg = crow, sl = key0;
                if (PAGED) {
                    int j = j0, sj = s0 + 16 * g4;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (sj >= p.ps) { sj -= p.ps; ++j; }
                    pg = tbl[j]; sl = sj;
                    if ((unsigned long long)pg >= (unsigned long long)p.nblk) continue;
                }
                kB[g4] = pg * p.kc_bs + sl * p.kc_ts; sB[g4] = pg * p.ks_bs + sl * p.ks_ts;
                vB[g4] = pg * p.vc_bs + sl * p.vc_ts; eB[g4] = pg * p.vs_bs + sl * p.vs_ts;
            }
        }
    };
    auto pick = [](const i64x4_t& x, int g4) { return g4 == 0 ? x[0] : g4 == 1 ? x[1] : g4 == 2 ? x[2] : x[3]; };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                         // running max of t, in log2 units
    const uint8_t* nowhere = p.q;                                 // readable and 16-byte aligned, for a load whose value is selected away
    const int kr = r & 15;                                        // K: the lane's key in its 16-key group
    const bool up = (r >> 4) != 0;                                // K: that group is the block's second

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        i64x4_t kB, sB, vB, eB;
        group_bases(k0, kB, sB, vB, eB);
        // a whole tile below the split's end on pages inside the pool: no lane needs a select on its addresses or its bytes
        const bool full = k0 + KT <= kend && kB[0] >= 0 && kB[1] >= 0 && kB[2] >= 0 && kB[3] >= 0;
        f32x16 sacc[2];
        auto front = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        // ---- S^T = K Q^T: K codes as they lie in memory, the lane's MX block scales on the instructions
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const long long bk = up ? kB[2 * kb + 1] : kB[2 * kb], bs = up ? sB[2 * kb + 1] : sB[2 * kb];
            const bool ok = FULL || (bk >= 0 && k0 + 32 * kb + r < kend);
            const uint8_t* kp = ok ? p.kc + bk + kr * p.kc_ts + hk * HB + 16 * h : nowhere;
            const uint8_t* sp = ok ? p.ksc + bs + kr * p.ks_ts + hk * SB : nowhere;
            u32x4 a[NM];
#pragma unroll
            for (int M = 0; M < NM; ++M) {
                a[M] = *reinterpret_cast<const u32x4*>(kp + 32 * M);
                if (!ok) a[M] = u32x4{0u, 0u, 0u, 0u};
            }
            uint32_t w[2];
            fp4h_scale_row<D>(sp, w);
            if (!ok) w[0] = w[1] = 0x7f7f7f7fu;
            sacc[kb] = fp4h_scores<NM>(a, w, h, qb);
        }

        // ---- the tile's V exponents: key k0 + lane on this lane, through LDS to the lanes that hold its scores
        {
            const int g4 = lane >> 4;
            const bool ok = FULL || (pick(kB, g4) >= 0 && k0 + lane < kend);
            const uint8_t* ep = ok ? p.vsc + pick(eB, g4) + (lane & 15) * p.vs_ts + hk : nowhere;
            const int byte = *ep;
            evs[lane] = ok ? byte - 127 : 0;
        }

        // ---- V -> V^T (the previous tile's operand reads were issued before these writes: one wave, LDS in order)
        if constexpr (D == 64) {
            // eight keys x eight channels a lane: keys 4 hv + 8 jj + c of group g4, one dword a channel at row byte 16 h + 8 hv + 4 jp
            const int rd = lane & 7, hv = (lane >> 3) & 1, g4 = lane >> 4;
            const long long bv = pick(vB, g4), bkk = pick(kB, g4);
            uint32_t ein[4], oin[4], te[4], to[4];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                uint32_t x[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int pos = 4 * hv + 8 * jj + c;          // the key's place in its 16-key group
                    const bool ok = FULL || (bkk >= 0 && k0 + 16 * g4 + pos < kend);
                    const uint8_t* vp = ok ? p.vc + bv + pos * p.vc_ts + hk * HB + 4 * rd : nowhere;
                    const uint32_t y = *reinterpret_cast<const uint32_t*>(vp);
                    x[c] = ok ? y : 0u;
                }
                fp4h_pair_nibbles(x, ein[2 * jj], oin[2 * jj], ein[2 * jj + 1], oin[2 * jj + 1]);
            }
            transpose4x4(ein, te);
            transpose4x4(oin, to);
            char* base = vt + 4 * g4 + 8 * (g4 >> 1) + 8 * hv;    // 16 h + 4 jp + 8 hv with g4 = 2 h + jp
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                *reinterpret_cast<uint32_t*>(base + vt4_off(8 * rd + 2 * m)) = te[m];
                *reinterpret_cast<uint32_t*>(base + vt4_off(8 * rd + 2 * m + 1)) = to[m];
            }
        } else {
            // the 128 kernel's transpose, once per 128 channels: 16 keys x 8 channels a lane and pass
            // (a rolled loop: one pass's 16 dwords and their addresses live at a time, beside 128 accumulators)
            const int rd = r & 15, hv = r >> 4;
#pragma unroll 1
            for (int pass = 0; pass < D / 128; ++pass) {
                uint32_t te[2][4], to[2][4];                      // [jp][m]: channels 8 rd + 2 m and + 2 m + 1 of keys j = 2 jp, 2 jp + 1
#pragma unroll
                for (int jp = 0; jp < 2; ++jp) {
                    const long long bv = h ? vB[2 + jp] : vB[jp], bkk = h ? kB[2 + jp] : kB[jp];   // (wave halves: group 2 h + jp)
                    uint32_t ein[4], oin[4];
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        uint32_t x[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int pos = 4 * hv + 8 * jj + c;
                            const bool ok = FULL || (bkk >= 0 && k0 + 32 * h + 16 * jp + pos < kend);
                            const uint8_t* vp = ok ? p.vc + bv + pos * p.vc_ts + hk * HB + 64 * pass + 4 * rd : nowhere;
                            const uint32_t y = *reinterpret_cast<const uint32_t*>(vp);
                            x[c] = ok ? y : 0u;
                        }
                        fp4h_pair_nibbles(x, ein[2 * jj], oin[2 * jj], ein[2 * jj + 1], oin[2 * jj + 1]);
                    }
                    transpose4x4(ein, te[jp]);
                    transpose4x4(oin, to[jp]);
                }
                char* base = vt + 16 * h + 8 * hv;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    *reinterpret_cast<u32x2*>(base + vt4_off(128 * pass + 8 * rd + 2 * m)) = u32x2{te[0][m], te[1][m]};
                    *reinterpret_cast<u32x2*>(base + vt4_off(128 * pass + 8 * rd + 2 * m + 1)) = u32x2{to[0][m], to[1][m]};
                }
            }
        }
        };
        if (full) front(std::true_type{});
        else front(std::false_type{});

        // (the selects only where a row's upper bound, the end, or with a window a row's lower bound lies inside this key tile)
        const bool need_mask = !full || (MOD ? k0 + KT - 1 > qlo + coff + md.wr : p.causal && k0 + KT - 1 > qlo + coff);
        const bool need_lo = MOD && k0 < qhi + coff - md.wl;
        fp4h_softmax_pv<D>(sacc, evs, vt, oacc, m_run, l_run, rw, k0, r, h, need_mask, need_lo);
    }

    // ---- epilogue
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    const bool dead = l_tot == 0.f;                      // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
    const float inv = vd * (1.f / l_tot);                // v_descale once, with 1 / l
    const float lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    const size_t row_id = ((size_t)b * p.hq + hd) * nq + qi;
    if (S == 1) {
        fp4h_store_o<Tag, NDV>(p.o + (((size_t)b * nq + qi) * p.hq + hd) * D, oacc, inv, dead, h);
        if (h == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * D;
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = dead ? 0.f : oacc[dvb][4 * g + j] * inv;
                *reinterpret_cast<f32x4*>(prow + 32 * dvb + 8 * g + 4 * h) = y;
            }
        if (h == 0) p.plse[row_id * S + s] = lse_v;
    }
}

// ---- the append -----------------------------------------------------------------------------------------------------------------
template <typename Tag, int D>
__global__ __launch_bounds__(256) void fp4kv_append_hdim_kernel(const Fp4AppendParams p) {
    constexpr int NB = D / 32;                           // lanes (MX blocks) a head
    const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (idx >= p.nnew * p.hkv * 2 * NB) return;          // (whole groups of 2 NB lanes: the shuffles below stay among live lanes)
    const int blk = idx % NB, isv = (idx / NB) & 1, th = idx / (2 * NB), hk = th % p.hkv, i = th / p.hkv;

    const uint8_t* src = (isv ? p.vn + b * p.vn_bs + i * p.vn_ts : p.kn + b * p.kn_bs + i * p.kn_ts) + (hk * D + 32 * blk) * 2;
    const float* dsp = isv ? p.vds : p.kds;
    const float ds = dsp ? dsp[b * (isv ? p.vds_bs : p.kds_bs) + hk] : 1.f;
    const float inv = 1.0f / ds;
    float x[32];
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(src + 16 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[8 * c + 2 * j] = unpack_lo<Tag>(w[j]) * inv;
            x[8 * c + 2 * j + 1] = unpack_hi<Tag>(w[j]) * inv;
            amax = fmaxf(amax, fmaxf(fabsf(x[8 * c + 2 * j]), fabsf(x[8 * c + 2 * j + 1])));
        }
    }
    // V: one scale a head, the maximum over the head's NB lanes (an aligned group: lane bits below NB)
    float ah = amax;
#pragma unroll
    for (int sh = 1; sh < NB; sh *= 2) ah = fmaxf(ah, __shfl_xor(ah, sh));
    const int e = fp4_block_exponent(isv ? ah : amax);
    const float sc = __uint_as_float((uint32_t)(127 - e) << 23);   // 2^-e, exact
    u32x4 codes;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) w |= fp4_code(x[8 * c + j] * sc) << (4 * j);
        codes[c] = w;
    }

    // where the token goes: nowhere if its position, its cache row or its page lies outside the cache
    const int len = min(max(p.seqlens[b], 0), p.cap), pos = len + i;
    if (pos >= p.cap) return;
    long long pg = b, sl = pos;
    if (p.table) {
        const int j = pos / p.ps;
        pg = p.table[b * p.tbl_rs + j];
        sl = pos - j * p.ps;
        if ((unsigned long long)pg >= (unsigned long long)p.nblk) return;
    } else if (p.bidx) {
        pg = p.bidx[b];
        if ((unsigned long long)pg >= (unsigned long long)p.bcache) return;
    }
    uint8_t* cp = (isv ? p.vc + pg * p.vc_bs + sl * p.vc_ts : p.kc + pg * p.kc_bs + sl * p.kc_ts) + hk * (D / 2) + 16 * blk;
    *reinterpret_cast<u32x4*>(cp) = codes;
    const uint8_t byte = (uint8_t)(e + 127);
    if (!isv) p.ksc[pg * p.ks_bs + sl * p.ks_ts + hk * NB + blk] = byte;
    else if (blk == 0) p.vsc[pg * p.vs_bs + sl * p.vs_ts + hk] = byte;
}

// ---- chunked prefill ------------------------------------------------------------------------------------------------------------
// what a lane holds of a tile in flight
template <int D> struct Fp4hStaged {
    u32x4 k[D == 256 ? 2 : 1];
    uint32_t v[D / 32];
    uint32_t s[2];
};

template <typename Tag, int D, typename... Mod>
__global__ __launch_bounds__(256, Fp4Hd<D>::WAVES) void fp4kv_prefill_hdim_kernel(const Fp4PrefillParams p, const Mod... mod) {
    constexpr bool MOD = sizeof...(Mod) != 0;                     // the featured instantiation: (KvqModSinks) follows p
    static_assert(sizeof...(Mod) <= 1, "Mod...: nothing, or (KvqModSinks)");
    const KvqModSinks md = kvq_mod_of<KvqModSinks>(mod...);
    using C = Fp4Hd<D>;
    constexpr int KT = C::KT, NM = C::NM, NDV = C::NDV, HB = C::HB, SB = C::SB, KROW = C::KROW;
    constexpr int CPK = D / 32, NKC = D == 256 ? 2 : 1;           // 16-byte chunks a key; chunks a lane
    __shared__ __attribute__((aligned(16))) char kt[2][KT * KROW];   // K stages: [key][D / 2 code bytes, D / 32 scale bytes, pad]
    __shared__ __attribute__((aligned(16))) char vt[2][C::VT];    // V^T stages, [channel][32 key bytes in P's key order]
    __shared__ __attribute__((aligned(16))) int evs[2][KT];       // the tiles' V exponents, by key
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rt = gridDim.x - 1 - blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int G = p.G;

    int qstart, kdummy;
    const int nq = kv_cu_range(p.cu_q, b, p.total_q, p.max_q, qstart);
    const int nk = kv_cu_range(p.cu_k, b, INT_MAX, p.cap, kdummy);
    const int rows = nq * G, pr0 = 128 * rt;
    if (pr0 >= rows) return;                                      // (the whole workgroup)
    const int coff = nk - nq;
    // the workgroup's keys [klo, kend) in tiles [t_lo, t_hi), the wave's [wlo, whi): fp4kv_prefill_kernel's bounds
    const int wr0 = pr0 + 32 * w;
    const bool wave_on = wr0 < rows;
    const int qlo = (wave_on ? wr0 : pr0) / G, qhi = (min(wr0 + 32, rows) - 1) / G;
    const int qlo_wg = pr0 / G, qhi_wg = (min(pr0 + 128, rows) - 1) / G;
    const int kend = MOD ? max(0, min(nk, qhi_wg + coff + md.wr + 1)) : p.causal ? max(0, min(nk, qhi_wg + coff + 1)) : nk;
    const int klo = MOD ? max(0, qlo_wg + coff - md.wl) : 0;
    const int whi = !wave_on ? 0 : MOD ? max(0, min(nk, qhi + coff + md.wr + 1)) : p.causal ? max(0, min(nk, qhi + coff + 1)) : nk;
    const int wlo = MOD ? max(0, qlo + coff - md.wl) : 0;
    const int t_lo = klo / KT, t_hi = (kend + KT - 1) / KT;       // (t_hi <= t_lo: no visible key, the ring below runs no tile)

    const int pr = wr0 + r;
    const bool valid = pr < rows;
    // (a padding row takes the wave's first token: its scores are masked like a real row's, and nothing of it is stored)
    const int qi = valid ? pr / G : qlo, hd = hk * G + (valid ? pr - qi * G : 0);
    i32x8_t qb[NM];
    fp4h_load_q<NM>(p.q + (long long)(qstart + qi) * p.q_ts + hd * D + 16 * h, valid, qb);
    const float qd = p.qds ? p.qds[b * p.qds_bs + hk] : 1.f;
    const float kd = p.kds ? p.kds[b * p.kds_bs + hk] : 1.f;
    const float vd = p.vds ? p.vds[b * p.vds_bs + hk] : 1.f;
    const float f = (p.c_log2 * qd) * kd;                         // the one score factor of this workgroup, > 0
    Fp4hRow rw;
    rw.valid = valid;
    rw.capped = MOD && md.cap2 != 0.f;
    rw.rhi = MOD ? min(min(qi + coff + md.wr, nk - 1), kend - 1) : min(p.causal ? qi + coff : nk - 1, kend - 1);
    rw.rlo = qi + coff - md.wl;
    rw.ck = f * md.cap_k;
    rw.cap2 = md.cap2;
    rw.fe = rw.capped ? 1.f : f;

    // ---- the loader: this wave's 16-key group of a tile (the lane maps: the header)
    const int* tbl = p.table + b * p.tbl_rs;
    const int rd = D == 64 ? lane & 7 : lane & 15;                // V: channels 8 rd ..
    const int hv = (lane >> (D == 64 ? 3 : 4)) & 1;
    const int jl = D == 64 ? (lane >> 4) & 1 : lane >> 5, cc = lane >> 5;   // (cc: D = 64 alone)
    constexpr int NVK = D == 64 ? 2 : 4;                          // V: keys a lane (and pass)
    auto vpos = [&](int c) { return D == 64 ? 4 * hv + 8 * jl + 2 * cc + c : 4 * hv + 8 * jl + c; };
    // the group's table entry, -1 where the group lies outside [klo, kend) (no entry is read there)
    auto fetch_page = [&](int t) -> int {
        const int key0 = t * KT + 16 * w;
        return key0 < kend && (!MOD || key0 + 16 > klo) ? tbl[key0 / p.ps] : -1;
    };
    auto load_tile = [&](int t, int pg) -> Fp4hStaged<D> {
        Fp4hStaged<D> st;
#pragma unroll
        for (int i = 0; i < NKC; ++i) st.k[i] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < D / 32; ++i) st.v[i] = 0u;
        st.s[0] = st.s[1] = lane < 16 ? 0x7f7f7f7fu : 127u;
        const int key0 = t * KT + 16 * w;
        if (key0 >= kend || (MOD && key0 + 16 <= klo) || (unsigned)pg >= (unsigned)p.nblk) return st;      // (wave-uniform)
        const long long sl = key0 % p.ps;
        const uint8_t* kp = p.kc + pg * p.kc_bs + sl * p.kc_ts + hk * HB;
        const uint8_t* vp = p.vc + pg * p.vc_bs + sl * p.vc_ts + hk * HB + 4 * rd;
        const uint8_t* sp = p.ksc + pg * p.ks_bs + sl * p.ks_ts + hk * SB;
        const uint8_t* ep = p.vsc + pg * p.vs_bs + sl * p.vs_ts + hk;
        const bool full = key0 + 16 <= kend;                     // no lane needs a compare
#pragma unroll
        for (int i = 0; i < NKC; ++i) {
            const int id = lane + 64 * i, kk = id / CPK, kch = id % CPK;
            if (id < 16 * CPK && (full || key0 + kk < kend)) st.k[i] = *reinterpret_cast<const u32x4*>(kp + kk * p.kc_ts + 16 * kch);
        }
#pragma unroll
        for (int pass = 0; pass < (D == 64 ? 1 : D / 128); ++pass)
#pragma unroll
            for (int c = 0; c < NVK; ++c) {
                const int pos = vpos(c);
                if (full || key0 + pos < kend) st.v[NVK * pass + c] = *reinterpret_cast<const uint32_t*>(vp + 64 * pass + pos * p.vc_ts);
            }
        if (lane < 16) {
            if (full || key0 + lane < kend) fp4h_scale_row<D>(sp + lane * p.ks_ts, st.s);
        } else if (lane < 32) {
            if (full || key0 + lane - 16 < kend) st.s[0] = ep[(lane - 16) * p.vs_ts];
        }
        return st;
    };
    auto store_tile = [&](const Fp4hStaged<D>& st, int buf) {
#pragma unroll
        for (int i = 0; i < NKC; ++i) {
            const int id = lane + 64 * i, kk = id / CPK, kch = id % CPK;
            if (id < 16 * CPK) *reinterpret_cast<u32x4*>(kt[buf] + KROW * (16 * w + kk) + 16 * kch) = st.k[i];
        }
        if (lane < 16) {
            char* srow = kt[buf] + KROW * (16 * w + lane) + HB;
            if constexpr (D == 64) *reinterpret_cast<uint16_t*>(srow) = (uint16_t)st.s[0];
            else *reinterpret_cast<u32x2*>(srow) = u32x2{st.s[0], st.s[1]};
        } else if (lane < 32) {
            evs[buf][16 * w + lane - 16] = (int)st.s[0] - 127;
        }
        constexpr uint32_t LO = 0x0f0f0f0fu;
        if constexpr (D == 64) {
            // two keys x eight channels a lane: the even (odd) channels of the key pair in a byte each
            const uint32_t e = (st.v[0] & LO) | ((st.v[1] & LO) << 4), o = ((st.v[0] >> 4) & LO) | (st.v[1] & ~LO);
            char* base = vt[buf] + 16 * (w >> 1) + 8 * hv + 2 * (2 * (w & 1) + jl) + cc;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                base[vt4_off(8 * rd + 2 * m)] = (char)(e >> (8 * m));
                base[vt4_off(8 * rd + 2 * m + 1)] = (char)(o >> (8 * m));
            }
        } else {
            // fp4kv_prefill_kernel's transpose of four keys x eight channels, once per 128 channels
            char* base = vt[buf] + 16 * (w >> 1) + 8 * hv + 2 * (2 * (w & 1) + jl);
#pragma unroll
            for (int pass = 0; pass < D / 128; ++pass) {
                const uint32_t x[4] = {st.v[4 * pass], st.v[4 * pass + 1], st.v[4 * pass + 2], st.v[4 * pass + 3]};
                uint32_t ea, oa, eb, ob;
                fp4h_pair_nibbles(x, ea, oa, eb, ob);
                // bytes {a.m, b.m} side by side: channel pair m = 0, 1 in the first word's halves, m = 2, 3 in the second's
                const uint32_t e01 = __builtin_amdgcn_perm(eb, ea, 0x05010400u), e23 = __builtin_amdgcn_perm(eb, ea, 0x07030602u);
                const uint32_t o01 = __builtin_amdgcn_perm(ob, oa, 0x05010400u), o23 = __builtin_amdgcn_perm(ob, oa, 0x07030602u);
                const int row0 = 128 * pass + 8 * rd;
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 0)) = (uint16_t)e01;
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 1)) = (uint16_t)o01;
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 2)) = (uint16_t)(e01 >> 16);
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 3)) = (uint16_t)(o01 >> 16);
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 4)) = (uint16_t)e23;
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 5)) = (uint16_t)o23;
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 6)) = (uint16_t)(e23 >> 16);
                *reinterpret_cast<uint16_t*>(base + vt4_off(row0 + 7)) = (uint16_t)(o23 >> 16);
            }
        }
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                         // running max of t, in log2 units

    // ---- one 64-key tile of this wave out of stage buf
    auto compute = [&](int k0, int buf) {
        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const char* row = kt[buf] + KROW * (32 * kb + r);
            u32x4 a[NM];
#pragma unroll
            for (int M = 0; M < NM; ++M) a[M] = *reinterpret_cast<const u32x4*>(row + 32 * M + 16 * h);
            uint32_t ws[2];
            fp4h_scale_row<D>(row + HB, ws);
            sacc[kb] = fp4h_scores<NM>(a, ws, h, qb);
        }
        const bool need_mask = k0 + KT > kend || (MOD ? k0 + KT - 1 > qlo + coff + md.wr : p.causal && k0 + KT - 1 > qlo + coff);
        const bool need_lo = MOD && k0 < qhi + coff - md.wl;
        fp4h_softmax_pv<D>(sacc, evs[buf], vt[buf], oacc, m_run, l_run, rw, k0, r, h, need_mask, need_lo);
    };

    // ---- the ring over tiles [t_lo, t_hi): tile t in stage t & 1, tile t + 1 in the other, tile t + 2 in st, the table entry of
    // tile t + 3 in pg.  Every wave meets the prologue's barrier and one a tile, whatever its own band.
    Fp4hStaged<D> st = load_tile(t_lo, fetch_page(t_lo));
    int pg = fetch_page(t_lo + 1);
    store_tile(st, t_lo & 1);
    st = load_tile(t_lo + 1, pg);
    pg = fetch_page(t_lo + 2);
    __syncthreads();
    for (int t = t_lo; t < t_hi; ++t) {
        store_tile(st, (t + 1) & 1);              // (its last readers, of tile t - 1, are behind the barrier)
        st = load_tile(t + 2, pg);
        pg = fetch_page(t + 3);
        // (a tile wholly right or, with a window, left of the wave's band: skipped)
        if (t * KT < whi && (!MOD || (t + 1) * KT > wlo)) compute(t * KT, t & 1);
        __syncthreads();
    }

    // ---- epilogue: the sink joins here, once per row, after the last tile (fp4kv_prefill_kernel's)
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    const float snk = MOD && md.sinks ? md.sinks[hd % md.sink_heads] : -INFINITY;
    bool dead;
    float inv, lse_v;
    if (snk != -INFINITY) {
        float iv;
        ex_sink_norm(m_run * 0.6931471805599453f, l_tot, snk, iv, lse_v);
        dead = false;                                    // (no visible key: iv = 0, lse = sink)
        inv = vd * iv;
    } else {
        dead = l_tot == 0.f;
        inv = vd * (1.f / l_tot);
        lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    }
    fp4h_store_o<Tag, NDV>(p.o + ((size_t)(qstart + qi) * p.hq + hd) * D, oacc, inv, dead, h);
    if (h == 0) p.lse[(size_t)hd * p.total_q + qstart + qi] = lse_v;
}

// f(std::integral_constant<int, d>) for d in {64, 256}
template <typename F> inline void fp4h_width(int64_t d, F&& f) {
    if (d == 64) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 256>{});
}

}  // namespace

hipError_t launch_fp4_kvcache_append_hdim(const Fp4AppendArgs& a, hipStream_t st) {
    if (a.d == 128) return launch_fp4_kvcache_append(a, st);     // the parent call, launch for launch
    if (a.d != 64 && a.d != 256) return hipErrorInvalidValue;
    const Fp4AppendParams p = fp4_append_params(a);
    const dim3 grid((unsigned)((a.seqlen_new * a.c.heads_kv * (a.d / 16) + 255) / 256), (unsigned)a.batch);
    route_hit(ROUTE_FP4KV_APPEND_HDIM);
    ProfScope ps(K_FP4KV_APPEND_HDIM, st);
    fp4h_width(a.d, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        if (a.dtype == 2) hipLaunchKernelGGL((fp4kv_append_hdim_kernel<bf16_tag, D>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((fp4kv_append_hdim_kernel<f16_tag, D>), grid, dim3(256), 0, st, p);
    });
    return hipGetLastError();
}

hipError_t launch_fp4_kvcache_hdim(const Fp4KvArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (a.d == 128) return launch_fp4_kvcache_mod(a, m, st);     // the parent call, launch for launch
    if (a.d != 64 && a.d != 256) return hipErrorInvalidValue;
    if (m.sinks && a.num_splits < 2) return hipErrorInvalidValue;   // (the C layer raises a sink call's S to 2: the sink joins in the combine)
    const Fp4KvParams p = fp4_kv_params(a, (int)a.d);
    const int S = (int)a.num_splits;
    const dim3 grid((unsigned)S, (unsigned)((p.rows + 31) / 32 * p.hkv), (unsigned)a.batch);
    const KvqMod md = kvq_mod_args(m, a.causal != 0);
    route_hit(ROUTE_FP4KV_SPLIT_HDIM);
    {
        ProfScope ps(K_FP4KV_SPLIT_HDIM, st);
        fp4h_width(a.d, [&](auto dc) {
            constexpr int D = decltype(dc)::value;
            kvq_dispatch(a.dtype, a.c.block_table != nullptr, [&](auto tag, auto paged) {
                using T = decltype(tag);
                constexpr bool P = decltype(paged)::value;
                if (m.any()) hipLaunchKernelGGL((fp4kv_split_hdim_kernel<T, P, D, KvqMod>), grid, dim3(64), 0, st, p, md);
                else hipLaunchKernelGGL((fp4kv_split_hdim_kernel<T, P, D>), grid, dim3(64), 0, st, p);
            });
        });
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || S == 1) return e;
    if (m.sinks)
        return launch_kv_combine_sink(a.o, a.lse, p.po, p.plse, a.batch, a.heads_q, a.seqlen_q, a.d, a.dtype, S, m.sinks,
                                      (int)(m.sink_heads > 0 ? m.sink_heads : 1), st);
    return launch_kv_combine(a.o, a.lse, p.po, p.plse, a.batch, a.heads_q, a.seqlen_q, a.d, a.dtype, S, st);
}

hipError_t launch_fp4_prefill_hdim(const Fp4VarlenArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (a.d == 128) return launch_fp4_prefill_mod(a, m, st);     // the parent call, launch for launch
    if (a.d != 64 && a.d != 256) return hipErrorInvalidValue;
    const Fp4PrefillParams p = fp4_prefill_params(a);
    const dim3 grid((unsigned)((a.max_seqlen_q * p.G + 127) / 128), (unsigned)a.c.heads_kv, (unsigned)a.batch);
    const KvqModSinks md{kvq_mod_args(m, a.causal != 0), m.sinks, (int)(m.sink_heads > 0 ? m.sink_heads : 1)};
    route_hit(ROUTE_FP4KV_PREFILL_HDIM);
    ProfScope ps(K_FP4KV_PREFILL_HDIM, st);
    fp4h_width(a.d, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        kvq_dispatch(a.dtype, false, [&](auto tag, auto) {
            using T = decltype(tag);
            if (m.any()) hipLaunchKernelGGL((fp4kv_prefill_hdim_kernel<T, D, KvqModSinks>), grid, dim3(256), 0, st, p, md);
            else hipLaunchKernelGGL((fp4kv_prefill_hdim_kernel<T, D>), grid, dim3(256), 0, st, p);
        });
    });
    return hipGetLastError();
}

}  // namespace fa
