// Chunked prefill over the paged MXFP4 KV cache for gfx950 at head dim d in {64, 128, 256} (fa_fp4_forward_varlen and its _mod /
// _hdim entry points; include/fa_mi355x.h; DESIGN.md sections 9zh - 9zj): packed e4m3 queries (total_q, H_q, d) over the four pool
// arrays fa_fp4_kvcache_append fills, per sequence, with the bottom-right causal diagonal of that sequence alone, in one launch and
// without a workspace.  Two bodies behind one launcher: fp4kv_prefill_kernel<Tag, Mod...> at 128, fp4kv_prefill_hdim_kernel<Tag, D,
// Mod...> at 64 / 256 on Fp4Hd<D> and the shared tile pieces of fa_fp4_common.h.
//
//     o[i] = sum_j softmax_j(softmax_scale q_descale k_descale q8[i] . (k4[j] 2^ek[j])) v4[j] 2^ev[j] v_descale
//
// The decode kernel (fa_fp4_decode.hip) reads every visible key once per WAVE of 32 rows.  Here a workgroup of four waves owns 128
// rows and reads a cache byte from memory once: the 64-key tile goes through LDS.
//
//   rows and waves   row = token * G + head in the group (the decode kernel's packing), a workgroup takes 128 consecutive rows of
//                    one (sequence, K/V head), wave w rows 32 w .. 32 w + 31.  Any G works the same way, the whole group shares the
//                    staged tile, and the four waves end within 96 / G tokens of each other under the causal mask: no wave
//                    idles through a quarter of the diagonal as it would with one head a wave.  The grid is (row tiles of
//                    max_seqlen_q, H_kv, B), the heaviest (last) row tile first; a workgroup past its sequence's rows returns.
//   the tile ring    tile t is computed from LDS stage t & 1 while tile t + 1 lies in the other stage and tile t + 2 is in flight
//                    in 9 registers a lane at 128 (three tiles deep); the table entry of tile t + 3 is fetched at the same time.  One
//                    barrier a tile: a stage is rewritten at the top of iteration t + 1, after the barrier that ended its last reader.
//   the loader       wave w moves the tile's 16-key group w (ps % 16 == 0: one page, one wave-uniform table entry):
//                      K      16 keys x D / 32 chunks of 16 code bytes, chunk id = lane + 64 i -> (key id / (D / 32), chunk id %
//                             (D / 32)) -> row KROW (16 w + key) + 16 chunk of the K stage
//                      scales lanes 0 .. 15 the k_scale row of key l -> byte D / 2 of the key's row; lanes 16 .. 31 the v_scale
//                             byte of key l - 16 -> evs[key] = byte - 127
//                      V      lane (rd = l & 15, hv = (l >> 4) & 1, jl = l >> 5): the dwords at channels 8 rd .. + 7 of the four
//                             keys pos = 4 hv + 8 jl + c of the group (a row of 16 lanes reads 64 bytes of a key), the decode kernel's
//                             nibble transpose cut to four keys (mask / shift / or, then 4 v_perm_b32), and eight 2-byte writes into
//                             the V^T image: channel 8 rd + 2 m (+ 1), byte 16 h + 8 hv + 2 j with h = w >> 1, j = 2 (w & 1) + jl.
//                    by width:          D = 64                        D = 128                  D = 256
//                      K chunks a lane  1, lanes 0 .. 31 alone         1                        2
//                      k_scale row      a ushort                      a dword                  two dwords
//                      K stage row      48 bytes                      80                       144
//                      V                two keys a lane, byte writes  four keys, as above      the 128 map twice (channels 128 pass
//                                       (below)                                                + 8 rd ..), eight dwords a lane
//                      LDS, two stages  11008 bytes                   19456                    36352
//                      V at 64: lane (rd = l & 7, hv = (l >> 3) & 1, jl = (l >> 4) & 1, cc = l >> 5) loads channels 8 rd .. of the TWO
//                      keys 4 hv + 8 jl + 2 cc (+ 1); mask / shift / or give a byte a channel, written at row byte 16 h + 8 hv + 2 j +
//                      cc with h = w >> 1, j = 2 (w & 1) + jl.
//                    So V is transposed ONCE a workgroup and tile, out of the registers the load landed in; the raw codes never
//                    lie in LDS.  A key at or past the workgroup's last visible key or on a page outside [0, num_blocks) is not
//                    loaded: zero codes, scale bytes 127, ev = 0.  A group whole below that bound on a valid page skips the
//                    per-lane compares (wave-uniform).
//   LDS              K stage: 64 rows of KROW bytes, D / 2 code bytes + D / 32 scale bytes padded to an ODD multiple of 16 (48 /
//                    80 / 144), so the 16-byte operand reads of 16 lanes land at sixteen different multiples of 16 mod 256, every
//                    bank once.  V^T stage: vt4_off's padded image of the decode kernel, 34 D bytes.  evs: 64 ints.  Two stages:
//                    2 x (64 KROW + 34 D + 256) bytes.
//   a wave's tile    the decode kernel's arithmetic with its operand orders (the header of fa_fp4_decode.hip): S^T = K Q^T with K
//                    in fp4 as operand A and the lane's k_scale byte on the instruction, q at channels 64 M + 16 h and 64 M + 32 +
//                    16 h; t = fma(s, f, ev) under the joint running maximum with the lazy rescale; P' rounded to e4m3; l from the
//                    unrounded ldexp(P', -ev); O^T = V^T P'^T with V^T in fp4 from the image.  The mask (a select on the scores) only
//                    where the tile holds the sequence's end or a row's diagonal: wave-uniform.  A wave skips the tiles past its own
//                    rows' last key but keeps loading and meeting the barrier.
//
// What is untrusted: cu_seqlens_q, cu_seqlens_k, block_table, the descales and every cache byte, read on the device only.  (start,
// nq_b) = kv_cu_range(cu_seqlens_q, b, total_q, max_seqlen_q); nk_b = kv_cu_range(cu_seqlens_k, b, 2^31 - 1, capacity).  A scale
// byte is only ever an operand of arithmetic.  Rows of no sequence are not written.
//
// fa_fp4_forward_varlen_mod (a sliding window, a softcap, attention sinks) launches the featured
// instantiation, fp4kv_prefill_kernel<Tag, KvqModSinks> at 128 and fp4kv_prefill_hdim_kernel<Tag, D, KvqModSinks> at 64 / 256:
// the same text with one more kernel argument (fa_kvq_common.h) and the features as run-time switches, noted at the sites
// they change.
#include <climits>

#include "fa_fp4_common.h"

namespace fa {

namespace {

// ---- chunked prefill ------------------------------------------------------------------------------------------------------------
// Two bodies: the 128 kernel below with its tile softmax inline, and fp4kv_prefill_hdim_kernel<.., D> for D = 64 / 256 on the shared
// pieces of fa_fp4_common.h.  No one text over the three widths kept the instructions of both (profiles/fp4_merge.md has the
// forms and their figures).
constexpr int kKRow = 80;                                // bytes of a key's row in the K stage
constexpr int kKBytes = 64 * kKRow;

// what a lane holds of a tile in flight
struct Fp4Staged {
    u32x4 k;
    uint32_t v[4];
    uint32_t s;
};

template <typename Tag, typename... Mod>
__global__ __launch_bounds__(256, 2) void fp4kv_prefill_kernel(const Fp4PrefillParams p, const Mod... mod) {
    constexpr bool MOD = sizeof...(Mod) != 0;                     // the featured instantiation: (KvqModSinks) follows p
    static_assert(sizeof...(Mod) <= 1, "Mod...: nothing, or (KvqModSinks)");
    const KvqModSinks md = kvq_mod_of<KvqModSinks>(mod...);
    constexpr int D = 128, KT = 64, NDV = D / 32, HB = D / 2;     // HB: code bytes a head
    __shared__ __attribute__((aligned(16))) char kt[2][kKBytes];  // K stages: [key][64 code bytes, 4 scale bytes, pad]
    __shared__ __attribute__((aligned(16))) char vt[2][kVt4Bytes];   // V^T stages, [channel][32 key bytes in P's key order]
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
    const int coff = nk - nq;                                     // causal: token i sees key j <= i + coff; MOD: [i + coff - wl, i + coff + wr]
    // the workgroup's keys [klo, kend) in tiles [t_lo, t_hi), the wave's [wlo, whi); without a window klo = wlo = t_lo = 0
    // window: klo is the smallest lower bound of the workgroup's 128 rows, kend its largest upper bound + 1 (the sequence's end at
    // most).  The ring walks tiles [klo / 64, ceil(kend / 64)) alone, O(N w) tiles a sequence; prologue, stage parity, the tile in
    // flight and the table entry of t + 3 all count from t_lo.  The loader reads no table entry, code or scale byte of a 16-key
    // group outside [klo, kend).  A wave computes the tiles that meet its own rows' band [wlo, whi) and only loads and meets the
    // barrier on the others.
    // (wl, wr <= 2^30, coff < 2^28, a token < 2^28: the sums stay inside an int)
    const int wr0 = pr0 + 32 * w;
    const bool wave_on = wr0 < rows;
    const int qlo = (wave_on ? wr0 : pr0) / G, qhi = (min(wr0 + 32, rows) - 1) / G;
    const int qlo_wg = pr0 / G, qhi_wg = (min(pr0 + 128, rows) - 1) / G;
    const int kend = MOD ? max(0, min(nk, qhi_wg + coff + md.wr + 1)) : p.causal ? max(0, min(nk, qhi_wg + coff + 1)) : nk;
    const int klo = MOD ? max(0, qlo_wg + coff - md.wl) : 0;
    const int whi = !wave_on ? 0 : MOD ? max(0, min(nk, qhi + coff + md.wr + 1)) : p.causal ? max(0, min(nk, qhi + coff + 1)) : nk;
    const int wlo = MOD ? max(0, qlo + coff - md.wl) : 0;
    const int t_lo = klo / KT, t_hi = (kend + KT - 1) / KT;      // (t_hi <= t_lo: no visible key, the ring below runs no tile)

    // this lane's query row: token qi, query head hd; it sees keys [rlo, rhi] (rlo: MOD alone)
    const int pr = wr0 + r;
    const bool valid = pr < rows;
    // (a padding row takes the wave's first token: its scores are masked like a real row's, and nothing of it is stored)
    const int qi = valid ? pr / G : qlo, hd = hk * G + (valid ? pr - qi * G : 0);
    const int rhi = MOD ? min(min(qi + coff + md.wr, nk - 1), kend - 1) : min(p.causal ? qi + coff : nk - 1, kend - 1);
    const int rlo = qi + coff - md.wl;

    i32x8_t qb[2];
    {
        // (an 8-bit operand's byte 16 g + x of lane half h is k = 32 g + 16 h + x: the two 16-byte halves lie 32 channels apart)
        const uint8_t* qp = p.q + (long long)(qstart + qi) * p.q_ts + hd * D + 16 * h;
#pragma unroll
        for (int M = 0; M < 2; ++M) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(qp + 64 * M), a1 = *reinterpret_cast<const u32x4*>(qp + 64 * M + 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qb[M][i] = valid ? (int)a0[i] : 0;
                qb[M][4 + i] = valid ? (int)a1[i] : 0;
            }
        }
    }
    const float qd = p.qds ? p.qds[b * p.qds_bs + hk] : 1.f;
    const float kd = p.kds ? p.kds[b * p.kds_bs + hk] : 1.f;
    const float vd = p.vds ? p.vds[b * p.vds_bs + hk] : 1.f;
    const float f = (p.c_log2 * qd) * kd;                         // the one score factor of this workgroup, > 0
    const bool capped = MOD && md.cap2 != 0.f;
    const float ck = f * md.cap_k;
    const float fe = capped ? 1.f : f;                            // the factor of what the accumulators hold after the cap

    // ---- the loader: this wave's 16-key group of a tile
    const int* tbl = p.table + b * p.tbl_rs;
    const int kk = lane >> 2, kch = lane & 3;                     // K: key of the group, 16-byte chunk
    const int rd = lane & 15, hv = (lane >> 4) & 1, jl = lane >> 5;   // V: channels 8 rd .., keys 4 hv + 8 jl + c of the group
    // the group's table entry, -1 where the group lies outside [klo, kend) (no entry is read there)
    auto fetch_page = [&](int t) -> int {
        const int key0 = t * KT + 16 * w;
        return key0 < kend && (!MOD || key0 + 16 > klo) ? tbl[key0 / p.ps] : -1;
    };
    auto load_tile = [&](int t, int pg) -> Fp4Staged {
        Fp4Staged st;
        st.k = u32x4{0u, 0u, 0u, 0u};
        st.v[0] = st.v[1] = st.v[2] = st.v[3] = 0u;
        st.s = lane < 16 ? 0x7f7f7f7fu : 127u;
        const int key0 = t * KT + 16 * w;
        if (key0 >= kend || (MOD && key0 + 16 <= klo) || (unsigned)pg >= (unsigned)p.nblk) return st;      // (wave-uniform)
        const long long sl = key0 % p.ps;
        const uint8_t* kp = p.kc + pg * p.kc_bs + sl * p.kc_ts + hk * HB;
        const uint8_t* vp = p.vc + pg * p.vc_bs + sl * p.vc_ts + hk * HB + 4 * rd;
        const uint8_t* sp = p.ksc + pg * p.ks_bs + sl * p.ks_ts + hk * 4;
        const uint8_t* ep = p.vsc + pg * p.vs_bs + sl * p.vs_ts + hk;
        const bool full = key0 + 16 <= kend;                     // no lane needs a compare
        if (full || key0 + kk < kend) st.k = *reinterpret_cast<const u32x4*>(kp + kk * p.kc_ts + 16 * kch);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int pos = 4 * hv + 8 * jl + c;
            if (full || key0 + pos < kend) st.v[c] = *reinterpret_cast<const uint32_t*>(vp + pos * p.vc_ts);
        }
        if (lane < 16) {
            if (full || key0 + lane < kend) st.s = *reinterpret_cast<const uint32_t*>(sp + lane * p.ks_ts);
        } else if (lane < 32) {
            if (full || key0 + lane - 16 < kend) st.s = ep[(lane - 16) * p.vs_ts];
        }
        return st;
    };
    auto store_tile = [&](const Fp4Staged& st, int buf) {
        *reinterpret_cast<u32x4*>(kt[buf] + kKRow * (16 * w + kk) + 16 * kch) = st.k;
        if (lane < 16) *reinterpret_cast<uint32_t*>(kt[buf] + kKRow * (16 * w + lane) + 64) = st.s;
        else if (lane < 32) evs[buf][16 * w + lane - 16] = (int)st.s - 127;
        // V -> V^T: four keys x eight channels a lane; the even (odd) channels of key pairs (0, 1) and (2, 3) in a byte each
        constexpr uint32_t LO = 0x0f0f0f0fu;
        const uint32_t ea = (st.v[0] & LO) | ((st.v[1] & LO) << 4), eb = (st.v[2] & LO) | ((st.v[3] & LO) << 4);
        const uint32_t oa = ((st.v[0] >> 4) & LO) | (st.v[1] & ~LO), ob = ((st.v[2] >> 4) & LO) | (st.v[3] & ~LO);
        // bytes {a.m, b.m} side by side: channel pair m = 0, 1 in the first word's halves, m = 2, 3 in the second's
        const uint32_t e01 = __builtin_amdgcn_perm(eb, ea, 0x05010400u), e23 = __builtin_amdgcn_perm(eb, ea, 0x07030602u);
        const uint32_t o01 = __builtin_amdgcn_perm(ob, oa, 0x05010400u), o23 = __builtin_amdgcn_perm(ob, oa, 0x07030602u);
        char* base = vt[buf] + 16 * (w >> 1) + 8 * hv + 2 * (2 * (w & 1) + jl);
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 0)) = (uint16_t)e01;
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 1)) = (uint16_t)o01;
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 2)) = (uint16_t)(e01 >> 16);
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 3)) = (uint16_t)(o01 >> 16);
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 4)) = (uint16_t)e23;
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 5)) = (uint16_t)o23;
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 6)) = (uint16_t)(e23 >> 16);
        *reinterpret_cast<uint16_t*>(base + vt4_off(8 * rd + 7)) = (uint16_t)(o23 >> 16);
    };

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                         // running max of t, in log2 units

    // ---- one 64-key tile of this wave out of stage buf
    auto compute = [&](int k0, int buf) {
        const char* ktb = kt[buf];
        const char* vtb = vt[buf];
        const int* evb = evs[buf];
        f32x16 sacc[2];
        // S^T = K Q^T: K codes as they lie in memory, the lane's MX block scale on the instruction
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const char* row = ktb + kKRow * (32 * kb + r);
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(row + 16 * h), a1 = *reinterpret_cast<const u32x4*>(row + 32 + 16 * h);
            const uint32_t ws = *reinterpret_cast<const uint32_t*>(row + 64);
            const int sc0 = (int)((ws >> (8 * h)) & 0xffu), sc1 = (int)((ws >> (16 + 8 * h)) & 0xffu);
            const i32x8_t k0a = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], 0, 0, 0, 0};
            const i32x8_t k1a = {(int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3], 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
            sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k0a, qb[0], sacc[kb], kFp4, 0, 0, sc0, 0, 127);
            sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k1a, qb[1], sacc[kb], kFp4, 0, 0, sc1, 0, 127);
        }

        // softcap (before the mask), as in fp4kv_split_kernel: the capped score in log2 units replaces s f, one exp2 and one rcp an element
        if (capped) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * ck) + 1.f);
                    sacc[kb][i] = fmaf(rr, -2.f * md.cap2, md.cap2);
                }
        }
        // the mask, t = (s f or the capped score) + ev, the row maximum over t
        // (the selects only where the sequence's end, a row's upper bound or with a window a row's lower bound lies inside this key
        // tile: wave-uniform.  A masked key's score is -inf before ev is added: its ev never reaches the joint maximum.)
        const bool need_mask = k0 + KT > kend || (MOD ? k0 + KT - 1 > qlo + coff + md.wr : p.causal && k0 + KT - 1 > qlo + coff);
        const bool need_lo = MOD && k0 < qhi + coff - md.wl;
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
                const int thr = rhi - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) > thr) sacc[kb][i] = -INFINITY;
            }
            if (need_lo) {
                const int thr = rlo - (k0 + 32 * kb + 4 * h);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((i & 3) + 8 * (i >> 2) < thr) sacc[kb][i] = -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                sacc[kb][i] = fmaf(sacc[kb][i], fe, (float)ev[kb][i]);   // (a masked key stays -inf whatever its ev: fe > 0)
                mx = fmaxf(mx, sacc[kb][i]);
            }
        }
        mx = fmaxf(mx, wave_half_swap(mx));
        const float m_new = fmaxf(m_run, mx);
        float m_use;
        if (__any(valid && m_new - m_run > 8.0f) != 0) {   // lazy rescale on the real rows; a row's first visible key: inf > 8
            m_use = m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int t2 = 0; t2 < NDV; ++t2)
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

        // O^T = V^T P'^T: the lane's 16 key bytes (32 keys) of channel 32 dvb + r
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(vtb + vt4_off(32 * dvb + r) + 16 * h);
            const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], 0, 0, 0, 0};
            oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], kFp4, 0, 0, 127, 0, 127);
        }
    };

    // ---- the ring over tiles [t_lo, t_hi): tile t in stage t & 1, tile t + 1 in the other, tile t + 2 in st, the table entry of
    // tile t + 3 in pg.  Every wave meets the prologue's barrier and one a tile, whatever its own band (an empty range: the one).
    Fp4Staged st = load_tile(t_lo, fetch_page(t_lo));
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

    // ---- epilogue: O^T register i of block dvb is channel 32 dvb + 4 h + (i & 3) + 8 (i >> 2) of the lane's query row
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    // sinks: the sink joins here, once per row, after the last tile: a softmax column with a zero value (it multiplies no V)
    const float snk = MOD && md.sinks ? md.sinks[hd % md.sink_heads] : -INFINITY;
    bool dead;
    float inv, lse_v;
    if (snk != -INFINITY) {                              // ex_sink_norm is finite at +-1e4
        float iv;
        ex_sink_norm(m_run * 0.6931471805599453f, l_tot, snk, iv, lse_v);
        dead = false;                                    // (no visible key: iv = 0, lse = sink)
        inv = vd * iv;
    } else {                                             // a head at -inf: the epilogue of the call without sinks, bit for bit
        dead = l_tot == 0.f;                             // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
        inv = vd * (1.f / l_tot);                        // v_descale once, with 1 / l
        lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    }
    uint16_t* orow = p.o + ((size_t)(qstart + qi) * p.hq + hd) * D;
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
    if (h == 0) p.lse[(size_t)hd * p.total_q + qstart + qi] = lse_v;
}

// D = 64 / 256: the same workgroup on Fp4Hd<D> and the shared tile pieces
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
    static_assert(D != 128, "128: fp4kv_prefill_kernel");
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
    // the workgroup's keys [klo, kend) in tiles [t_lo, t_hi), the wave's [wlo, whi); without a window klo = wlo = t_lo = 0
    // window: klo is the smallest lower bound of the workgroup's 128 rows, kend its largest upper bound + 1 (the sequence's end at
    // most).  The ring walks tiles [klo / 64, ceil(kend / 64)) alone, O(N w) tiles a sequence; prologue, stage parity, the tile in
    // flight and the table entry of t + 3 all count from t_lo.  The loader reads no table entry, code or scale byte of a 16-key
    // group outside [klo, kend).  A wave computes the tiles that meet its own rows' band [wlo, whi) and only loads and meets the
    // barrier on the others.
    // (wl, wr <= 2^30, coff < 2^28, a token < 2^28: the sums stay inside an int)
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
            // four keys x eight channels a lane and pass of 128 channels: the even (odd) channels of key pairs (0, 1) and (2, 3) in a byte each
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
    // tile t + 3 in pg.  Every wave meets the prologue's barrier and one a tile, whatever its own band (an empty range: the one).
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

    // ---- epilogue.  sinks: the sink joins here, once per row, after the last tile: a softmax column with a zero value (it multiplies no V)
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    const float snk = MOD && md.sinks ? md.sinks[hd % md.sink_heads] : -INFINITY;
    bool dead;
    float inv, lse_v;
    if (snk != -INFINITY) {                              // ex_sink_norm is finite at +-1e4
        float iv;
        ex_sink_norm(m_run * 0.6931471805599453f, l_tot, snk, iv, lse_v);
        dead = false;                                    // (no visible key: iv = 0, lse = sink)
        inv = vd * iv;
    } else {                                             // a head at -inf: the epilogue of the call without sinks, bit for bit
        dead = l_tot == 0.f;                             // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
        inv = vd * (1.f / l_tot);                        // v_descale once, with 1 / l
        lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    }
    fp4h_store_o<Tag, NDV>(p.o + ((size_t)(qstart + qi) * p.hq + hd) * D, oacc, inv, dead, h);
    if (h == 0) p.lse[(size_t)hd * p.total_q + qstart + qi] = lse_v;
}

}  // namespace

// (the route and the profiler id: as in launch_fp4_kvcache, fa_fp4_decode.hip)
hipError_t launch_fp4_prefill(const Fp4VarlenArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (a.d != 64 && a.d != 128 && a.d != 256) return hipErrorInvalidValue;
    const Fp4PrefillParams p = fp4_prefill_params(a);
    const dim3 grid((unsigned)((a.max_seqlen_q * p.G + 127) / 128), (unsigned)a.c.heads_kv, (unsigned)a.batch);
    const KvqModSinks md{kvq_mod_args(m, a.causal != 0), m.sinks, (int)(m.sink_heads > 0 ? m.sink_heads : 1)};
    route_hit(a.d != 128 ? ROUTE_FP4KV_PREFILL_HDIM : m.any() ? ROUTE_FP4KV_PREFILL_MOD : ROUTE_FP4KV_PREFILL);
    ProfScope ps(a.d != 128 ? K_FP4KV_PREFILL_HDIM : m.any() ? K_FP4KV_PREFILL_MOD : K_FP4KV_PREFILL, st);
    fp4h_width(a.d, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        kvq_dispatch(a.dtype, false, [&](auto tag, auto) {
            using T = decltype(tag);
            if constexpr (D == 128) {
                if (m.any()) hipLaunchKernelGGL((fp4kv_prefill_kernel<T, KvqModSinks>), grid, dim3(256), 0, st, p, md);
                else hipLaunchKernelGGL((fp4kv_prefill_kernel<T>), grid, dim3(256), 0, st, p);
            } else {
                if (m.any()) hipLaunchKernelGGL((fp4kv_prefill_hdim_kernel<T, D, KvqModSinks>), grid, dim3(256), 0, st, p, md);
                else hipLaunchKernelGGL((fp4kv_prefill_hdim_kernel<T, D>), grid, dim3(256), 0, st, p);
            }
        });
    });
    return hipGetLastError();
}

}  // namespace fa
