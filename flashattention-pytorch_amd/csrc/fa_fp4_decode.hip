// An MXFP4 KV cache for gfx950 at head dim d in {64, 128, 256}: the append and split-KV decoding (fa_fp4_kvcache_append,
// fa_fp4_forward_kvcache and their _mod / _hdim entry points; include/fa_mi355x.h; DESIGN.md sections 9zg, 9zi, 9zj).  The cache
// holds OCP e2m1 codes, two a byte (low nibble = the even channel), with E8M0 scale bytes (value 2^(byte - 127)):
//     k_cache (.., H_kv, d / 2) codes, k_scale (.., H_kv, d / 32)   one scale per 32 channels (an MX block)
//     v_cache (.., H_kv, d / 2) codes, v_scale (.., H_kv)           ONE scale per (token, head) over all d channels
// 67 / 133 / 265 bytes a token and head at d = 64 / 128 / 256 against 128 / 256 / 512 in e4m3.  q stays e4m3, and both products
// run on v_mfma_scale_f32_32x32x64_f8f6f4 with an fp4 A operand and an e4m3 B operand; nothing dequantises on the VALU.
//
//     o = softmax(softmax_scale q_descale k_descale q8 (k4 2^ek)^T [causal, bottom-right]) (v4 2^ev v_descale)
//
// The append is one kernel template over D.  The decode wave has two bodies, fp4kv_split_kernel at 128 and fp4kv_split_hdim_kernel<..,
// D> at 64 / 256 (the per-width facts: Fp4Hd<D>, fa_fp4_common.h, which also holds what the 64 / 256 reader shares with
// fa_fp4_prefill.hip's: the q load, the score block, the tile softmax with the PV product, the row store), behind one launcher:
//   fp4kv_append_kernel<Tag, D>     one thread per (token, head, K or V, 32-channel block): 64 bytes of 16-bit input in, 16 code
//                                   bytes and a scale byte out; NB = D / 32 lanes of K, then NB of V, a (token, head).
//                                   x' = x * (1 / descale) in fp32; e = the smallest integer with 6 * 2^e >= amax over the block
//                                   (32 channels for K, all D for V: a butterfly maximum over the head's NB lanes, xor 1 .. NB / 2
//                                   inside an aligned group of NB), clamped to [-64, 64], 0 for amax = 0, read off amax's exponent
//                                   and mantissa; the code is x' * 2^-e (exact) rounded to e2m1, nearest, ties to the even code,
//                                   by seven compares.  The early return cuts whole groups of 2 NB lanes (2 NB divides 64).
//   fp4kv_split_kernel<Tag, PAGED, Mod...>, fp4kv_split_hdim_kernel<Tag, PAGED, D, Mod...>
//                                   fp8kv_split_kernel's mapping (fa_fp8_decode.hip): one wave per (split, 32-row tile x K/V head,
//                                   sequence), row = token * G + head in the group, 64-key tiles, every cache byte read once.
//                                   Mod...: nothing, or (KvqMod) for the featured call below.
//   kv_combine_kernel<Tag, false>   fa_decode.hip's combine, unchanged, for S > 1 (kv_workspace_bytes' layout).
//
// What differs by width in the decode wave (everything else is the same arithmetic, statement for statement):
//                          D = 64                         D = 128                       D = 256
//   S^T instructions a     1, MX block h,                 2, blocks 2 M + h,            4, blocks 2 M + h,
//   32-key block           byte h of a ushort row         a dword row                   two dwords, instruction M reads dword M >> 1
//   V -> V^T               8 keys x 8 channels a lane,    16 keys x 8 channels a        the 128 map twice, channels 128 pass + 8 rd ..,
//                          dword writes (below)           lane, 8-byte writes           one pass live at a time (a rolled loop)
//   O^T instructions       2                              4                             8 (128 accumulators, in AGPRs)
//   waves a SIMD           2                              2                             1 (why: Fp4Hd's comment)
//
// One 64-key tile of a wave, lane l = (r = l & 31, h = l >> 5):
//   S^T = K Q^T     A = K in fp4 as it lies in memory: key k0 + 32 kb + r, channels 64 M + 32 h .. + 31 are the 16 bytes at
//                   32 M + 16 h of the head's D / 2 (the low four operand dwords; the high four are not read by the fp4 format):
//                   a 4-bit operand's nibble x of lane half h is k = 32 h + x.  The lane's block of instruction M is channel
//                   block 2 M + h, exactly one MX block: its k_scale byte (one load a key, a bit-field extract a block) is
//                   A's E8M0 scale operand.  B = the e4m3 q row with scale 127; an 8-bit operand's byte 16 g + x of lane half h
//                   is k = 32 g + 16 h + x, so the lane's two 16-byte loads are channels 64 M + 16 h .. and 64 M + 32 + 16 h ..
//                   (between two 8-bit operands the order cancels; against a 4-bit one it has to be the instruction's own).
//                   Accumulator register i of block kb is key k0 + 32 kb + 4 h + (i & 3) + 8 (i >> 2), as in the e4m3 kernel.
//   softmax         V's per-token scale rides in the exponent: t_j = fma(s_j, f, ev_j) with f = softmax_scale log2(e) q_descale
//                   k_descale and ev_j = v_scale byte - 127.  The running maximum M and the lazy rescale (threshold 8) run over t;
//                   P'_j = exp2(t_j - M) is rounded to e4m3 (RNE) and meets the RAW v4 codes; l adds ldexp(P'_j, -ev_j), the
//                   unscaled exp2(s_j f - M) from the unrounded value.  o = acc v_descale / l, lse = (M + log2 l) ln 2.  With
//                   every ev small P' still peaks at 1 (the maximum is joint), with ev spread wide the small keys lose what
//                   their share of o is worth.  The 64 ev of a tile are loaded one a lane and handed round through 256 bytes of LDS.
//   O^T = V^T P^T   B = P'^T as the accumulators hold it: byte 16 kb + 4 j + c of lane half h is key 32 kb + 4 h + 8 j + c (the
//                   e4m3 kernel's registers), which the instruction takes as k = 32 kb + 16 h + 4 j + c.  A = V^T in fp4, unit
//                   scale, in that order: the 16 bytes of lane (r, half kb) are channel 32 dvb + r, byte 8 h + 2 j + cc = keys
//                   32 kb + 4 h + 8 j + 2 cc (low nibble) and + 2 cc + 1 (high nibble).  The cache has two CHANNELS of a key in a
//                   byte, so the transpose is one of nibbles: lane (rd = r & 15, hv = r >> 4, h) loads the dword at channels
//                   8 rd .. + 7 of the 16 keys 32 h + 4 hv + 8 j + c; mask / shift / or turn the dwords of keys c = 0, 1 (and
//                   2, 3) into a dword of the even channels and one of the odd channels with the two keys in a byte; the 4 x 4
//                   byte transpose (8 v_perm_b32) of {01, 23 of j, 01, 23 of j + 1} then gives one dword a channel, and j = 0, 1
//                   with j = 2, 3 make the 8 bytes written at row = channel, byte 16 h + 8 hv.  (That is the map at D = 128 and,
//                   once per 128 channels, at 256; D = 64 below.)
//   LDS image       D rows (channels) x 32 key bytes, 16 bytes of padding after every eight rows: vt4_off(row) = 32 row +
//                   16 (row >> 3), row byte 16 h + 8 hv + 2 j + cc = keys 32 h + 4 hv + 8 j + 2 cc (low nibble) and + 1 (high).
//                   Banks (64 x 4 bytes): the 8-byte writes of lanes 0 .. 31 (h = 0) land at 16 rd + 8 hv + 32 m
//                   mod 256, all 256 bytes once; the 16-byte reads of lanes r = 0 .. 15 land at 32 r + 16 (r >> 3) mod 256, all
//                   256 bytes once.  One wave: LDS runs in order, no barrier.
//     D = 256       two passes of the transpose above, channels 128 pass + 8 rd ..: the second pass lies 128 rows = 17 x 256
//                   bytes on, so each pass has the 128 image's banks.  One pass is live at a time (16 dwords a lane).
//     D = 64        64 rows: the 128 map (8 channels x 16 keys a lane) would leave 32 lanes idle.  Lane (rd = l & 7, hv = (l >> 3) & 1,
//                   g4 = l >> 4) loads the dword at channels 8 rd .. of the EIGHT keys 4 hv + 8 jj + c (jj < 2, c < 4) of 16-key group
//                   g4 = 2 h + jp; one 4 x 4 byte transpose each for the even and the odd channels gives a dword a channel, written
//                   at row byte 16 h + 8 hv + 4 jp.  Banks: the 16-byte reads of lanes r = 0 .. 15 land at 32 r + 16 (r >> 3) mod
//                   256, every bank once, as at 128.  The dword writes of the 64 lanes land at dword 4 rd + q + 16 m mod 64 with
//                   q = 4 h + 2 hv + jp in 0 .. 7: banks 0 .. 35, at most two lanes a bank, so a write takes two passes where the
//                   128 map's takes one.  No padding of 32-byte rows clears both: the reads need rows r and r + 8 an odd
//                   multiple of 16 bytes apart mod 32, the writes need the row groups 8 rd a multiple of 32 apart.  Eight dword
//                   writes a lane and tile against 64 operand bytes read: the reads keep the clean pattern.
//
// What is untrusted: cache_seqlens, block_table, cache_batch_idx, the descales and every cache byte are device memory read on the
// device only.  len_b = clamp(cache_seqlens[b], 0, capacity); a cache_batch_idx outside [0, B_cache) is an empty sequence (decode)
// or drops the tokens (append); a page outside [0, num_blocks) reads as zero codes with scale bytes 127 (score 0, value 0) and
// drops an appended token; a position at or past the capacity drops the token.  Keys at or past the split's end are never loaded:
// codes read as zero, scale bytes as 127, the score is masked by a select.  A scale byte is only ever an operand of arithmetic
// (0xFF is a NaN to the instruction and ev = 128 to the softmax): it can make a key's share any number, never an address.
// A tile whole below the split's end on pages inside the pool takes the wave-uniform path without the selects, as in the e4m3 kernel.
//
// fa_fp4_forward_kvcache_mod (a sliding window, a softcap, attention sinks) launches the featured
// instantiation, fp4kv_split_kernel<Tag, PAGED, KvqMod> at 128 and fp4kv_split_hdim_kernel<Tag, PAGED, D, KvqMod> at 64 / 256:
// the same text with one more kernel argument (fa_kvq_common.h) and the three features as wave-uniform run-time switches,
// noted at the sites they change.  The bounds live in SGPRs (md is a kernel argument); a lane's lower bound is recomputed from
// its token where it is needed.  Sinks are not this kernel's: they join in kv_combine_kernel<Tag, true>, once per row.
#include "fa_fp4_common.h"

namespace fa {

namespace {

// ---- split-KV decode ------------------------------------------------------------------------------------------------------------
// Two bodies: the 128 kernel below with its tile softmax inline, and fp4kv_split_hdim_kernel<.., D> for D = 64 / 256 on the shared
// pieces of fa_fp4_common.h.  No one text over the three widths kept the instructions of both, and the forms that moved the 128
// kernel ran slower (profiles/fp4_merge.md has the forms and their figures).
template <typename Tag, bool PAGED, typename... Mod>
__global__ __launch_bounds__(64, 2) void fp4kv_split_kernel(const Fp4KvParams p, const Mod... mod) {
    constexpr bool MOD = sizeof...(Mod) != 0;                     // the featured instantiation: (KvqMod) follows p
    static_assert(sizeof...(Mod) <= 1, "Mod...: nothing, or (KvqMod)");
    const KvqMod md = kvq_mod_of<KvqMod>(mod...);
    constexpr int D = 128, KT = 64, NDV = D / 32, HB = D / 2;     // HB: code bytes a head
    __shared__ __attribute__((aligned(16))) char vt[kVt4Bytes];   // V^T tile, [channel][32 key bytes in P's key order]
    __shared__ __attribute__((aligned(16))) int evs[KT];          // the tile's V exponents, by key
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int nq = p.nq, rows = p.rows, G = p.G;
    const int pr0 = 32 * rt, pr = pr0 + r;                        // (the grid has ceil(rows / 32) row tiles: pr0 < rows)

    // the sequence: its length, and the cache row its keys lie in (contiguous)
    int lk = p.seqlens ? min(max(p.seqlens[b], 0), p.cap) : p.cap;
    long long crow = b;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; lk = 0; }   // an index outside the cache: an empty sequence
    }
    const int coff = lk - nq;                                     // causal: token i sees key j <= i + coff; MOD: [i + coff - wl, i + coff + wr]
    const int qlo = pr0 / G, qhi = (min(pr0 + 32, rows) - 1) / G;
    // the split's keys [kbeg, kend): the tile's visible keys [lo, hi) cut into 64-key tiles, tiles [s nt / S, (s + 1) nt / S)
    // window: lo is the first 64-key tile some row of the 32 sees (whole 16-key groups), hi the last visible key + 1.  The splits
    // cut [lo, hi): no table entry, code byte or scale byte below lo or at / past hi is read.
    // (wl, wr <= 2^30, coff < 2^28, a token < 2^20: the sums stay inside an int)
    const int hi = MOD ? max(0, min(lk, qhi + coff + md.wr + 1)) : p.causal ? max(0, min(lk, qhi + coff + 1)) : lk;
    const int lo = MOD ? max(0, qlo + coff - md.wl) & ~(KT - 1) : 0;
    const int nt = MOD ? (hi > lo ? (hi - lo + KT - 1) / KT : 0) : (hi + KT - 1) / KT;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    const int kbeg = lo + t0 * KT, kend = min(hi, lo + t1 * KT);

    // this lane's query row: token qi, query head hd; its last visible key rhi (MOD: it sees keys [qi + coff - wl, rhi])
    const bool valid = pr < rows;
    // (a padding row takes the tile's first token: its scores are masked like a real row's, and nothing of it is stored)
    const int qi = valid ? pr / G : qlo, hd = hk * G + (valid ? pr - qi * G : 0);
    const int rhi = MOD ? min(min(qi + coff + md.wr, lk - 1), kend - 1) : min(p.causal ? qi + coff : lk - 1, kend - 1);

    i32x8_t qb[2];
    {
        // (an 8-bit operand's byte 16 g + x of lane half h is k = 32 g + 16 h + x: the two 16-byte halves lie 32 channels apart)
        const uint8_t* qp = p.q + (long long)b * p.q_bs + (long long)qi * p.q_ts + hd * D + 16 * h;
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
    const float f = (p.c_log2 * qd) * kd;                         // the one score factor of this wave, > 0
    const bool capped = MOD && md.cap2 != 0.f;
    const float ck = f * md.cap_k;
    const float fe = capped ? 1.f : f;                            // the factor of what the accumulators hold after the cap

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

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;                         // running max of t, in log2 units
    const uint8_t* nowhere = p.q;                                 // readable and 16-byte aligned, for a load whose value is selected away
    const int rd = r & 15, hv = r >> 4;                           // the lane's place in the V transpose: channels 8 rd .., keys 32 h + 4 hv + ..
    const bool up = hv != 0;                                      // K: the lane's key lies in the block's second 16-key group

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        i64x4_t kB, sB, vB, eB;
        group_bases(k0, kB, sB, vB, eB);

        // a whole tile below the split's end on pages inside the pool: no lane needs a select on its addresses or its bytes
        const bool full = k0 + KT <= kend && kB[0] >= 0 && kB[1] >= 0 && kB[2] >= 0 && kB[3] >= 0;
        f32x16 sacc[2];
        auto front = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        // ---- S^T = K Q^T: K codes as they lie in memory, the lane's MX block scale on the instruction
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const long long bk = up ? kB[2 * kb + 1] : kB[2 * kb], bs = up ? sB[2 * kb + 1] : sB[2 * kb];
            const bool ok = FULL || (bk >= 0 && k0 + 32 * kb + r < kend);
            const uint8_t* kp = ok ? p.kc + bk + rd * p.kc_ts + hk * HB + 16 * h : nowhere;
            const uint8_t* sp = ok ? p.ksc + bs + rd * p.ks_ts + hk * 4 : nowhere;
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(kp), a1 = *reinterpret_cast<const u32x4*>(kp + 32);
            uint32_t w = *reinterpret_cast<const uint32_t*>(sp);
            if (!ok) w = 0x7f7f7f7fu;
            const int sc0 = (int)((w >> (8 * h)) & 0xffu), sc1 = (int)((w >> (16 + 8 * h)) & 0xffu);
            i32x8_t k0a = {0, 0, 0, 0, 0, 0, 0, 0}, k1a = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                k0a[i] = ok ? (int)a0[i] : 0;
                k1a[i] = ok ? (int)a1[i] : 0;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
            sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k0a, qb[0], sacc[kb], kFp4, 0, 0, sc0, 0, 127);
            sacc[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k1a, qb[1], sacc[kb], kFp4, 0, 0, sc1, 0, 127);
        }

        // ---- the tile's V exponents: key k0 + lane on this lane, through LDS to the lanes that hold its scores
        {
            const int g4 = lane >> 4;
            const long long bkk = g4 == 0 ? kB[0] : g4 == 1 ? kB[1] : g4 == 2 ? kB[2] : kB[3];
            const long long be = g4 == 0 ? eB[0] : g4 == 1 ? eB[1] : g4 == 2 ? eB[2] : eB[3];
            const bool ok = FULL || (bkk >= 0 && k0 + lane < kend);
            const uint8_t* ep = ok ? p.vsc + be + (lane & 15) * p.vs_ts + hk : nowhere;
            const int byte = *ep;
            evs[lane] = ok ? byte - 127 : 0;
        }

        // ---- V -> V^T: 16 keys x 8 channels a lane, the nibble transpose, 8 bytes a channel into the image
        // (the previous tile's operand reads were issued before these writes: one wave, LDS in order)
        {
            uint32_t te[2][4], to[2][4];                          // [jp][m]: channels 8 rd + 2 m and + 2 m + 1 of keys j = 2 jp, 2 jp + 1
#pragma unroll
            for (int jp = 0; jp < 2; ++jp) {
                const long long bv = h ? vB[2 + jp] : vB[jp], bkk = h ? kB[2 + jp] : kB[jp];   // (wave halves: group 2 h + jp)
                uint32_t ein[4], oin[4];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    uint32_t x[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int pos = 4 * hv + 8 * jj + c;      // the key's place in its 16-key group
                        const bool ok = FULL || (bkk >= 0 && k0 + 32 * h + 16 * jp + pos < kend);
                        const uint8_t* vp = ok ? p.vc + bv + pos * p.vc_ts + hk * HB + 4 * rd : nowhere;
                        const uint32_t y = *reinterpret_cast<const uint32_t*>(vp);
                        x[c] = ok ? y : 0u;
                    }
                    constexpr uint32_t LO = 0x0f0f0f0fu;
                    ein[2 * jj] = (x[0] & LO) | ((x[1] & LO) << 4);
                    oin[2 * jj] = ((x[0] >> 4) & LO) | (x[1] & ~LO);
                    ein[2 * jj + 1] = (x[2] & LO) | ((x[3] & LO) << 4);
                    oin[2 * jj + 1] = ((x[2] >> 4) & LO) | (x[3] & ~LO);
                }
                transpose4x4(ein, te[jp]);
                transpose4x4(oin, to[jp]);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                *reinterpret_cast<u32x2*>(vt + vt4_off(8 * rd + 2 * m) + 16 * h + 8 * hv) = u32x2{te[0][m], te[1][m]};
                *reinterpret_cast<u32x2*>(vt + vt4_off(8 * rd + 2 * m + 1) + 16 * h + 8 * hv) = u32x2{to[0][m], to[1][m]};
            }
        }
        };
        if (full) front(std::true_type{});
        else front(std::false_type{});

        // ---- softcap (before the mask): the capped score in log2 units, cap2 (1 - 2 r) with r = 1 / (2^(ck s) + 1), ck = f cap_k,
        // replaces s f: one exp2 and one rcp an element
        if (capped) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rr = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(sacc[kb][i] * ck) + 1.f);
                    sacc[kb][i] = fmaf(rr, -2.f * md.cap2, md.cap2);
                }
        }
        // ---- the mask, t = (s f or the capped score) + ev, the row maximum over t
        // (the selects only where a row's upper bound, the end, or with a window a row's lower bound lies inside this key tile:
        // wave-uniform.  A masked key's score is -inf BEFORE ev is added: its ev never reaches the joint maximum.)
        const bool need_mask = !full || (MOD ? k0 + KT - 1 > qlo + coff + md.wr : p.causal && k0 + KT - 1 > qlo + coff);
        const bool need_lo = MOD && k0 < qhi + coff - md.wl;      // some row's lower bound lies inside or past this tile
        int ev[2][16];
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const i32x4_t e4 = *reinterpret_cast<const i32x4_t*>(evs + 32 * kb + 4 * h + 8 * j);
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
                const int thr = qi + coff - md.wl - (k0 + 32 * kb + 4 * h);
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

        // ---- O^T = V^T P'^T: the lane's 16 key bytes (32 keys) of channel 32 dvb + r
#pragma unroll
        for (int dvb = 0; dvb < NDV; ++dvb) {
            const u32x4 a0 = *reinterpret_cast<const u32x4*>(vt + vt4_off(32 * dvb + r) + 16 * h);
            const i32x8_t va = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], 0, 0, 0, 0};
            oacc[dvb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, pb, oacc[dvb], kFp4, 0, 0, 127, 0, 127);
        }
    }

    // ---- epilogue: O^T register i of block dvb is channel 32 dvb + 4 h + (i & 3) + 8 (i >> 2) of the lane's query row
    const float l_tot = l_run + wave_half_swap(l_run);
    if (!valid) return;
    const bool dead = l_tot == 0.f;                      // no visible key: o = 0, lse = -inf (a NaN l is not dead: it propagates)
    const float inv = vd * (1.f / l_tot);                // v_descale once, with 1 / l
    const float lse_v = dead ? -INFINITY : (m_run + log2f(l_tot)) * 0.6931471805599453f;
    const size_t row_id = ((size_t)b * p.hq + hd) * nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + (((size_t)b * nq + qi) * p.hq + hd) * D;
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

// D = 64 / 256: the same wave on Fp4Hd<D> and the shared tile pieces
template <typename Tag, bool PAGED, int D, typename... Mod>
__global__ __launch_bounds__(64, Fp4Hd<D>::WAVES) void fp4kv_split_hdim_kernel(const Fp4KvParams p, const Mod... mod) {
    constexpr bool MOD = sizeof...(Mod) != 0;                     // the featured instantiation: (KvqMod) follows p
    static_assert(sizeof...(Mod) <= 1, "Mod...: nothing, or (KvqMod)");
    static_assert(D != 128, "128: fp4kv_split_kernel");
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

    // the sequence: its length, and the cache row its keys lie in (contiguous)
    int lk = p.seqlens ? min(max(p.seqlens[b], 0), p.cap) : p.cap;
    long long crow = b;
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; lk = 0; }   // an index outside the cache: an empty sequence
    }
    const int coff = lk - nq;                                     // causal: token i sees key j <= i + coff; MOD: [i + coff - wl, i + coff + wr]
    const int qlo = pr0 / G, qhi = (min(pr0 + 32, rows) - 1) / G;
    // the split's keys [kbeg, kend): the tile's visible keys [lo, hi) cut into 64-key tiles, tiles [s nt / S, (s + 1) nt / S)
    // window: lo is the first 64-key tile some row of the 32 sees (whole 16-key groups), hi the last visible key + 1.  The splits
    // cut [lo, hi): no table entry, code byte or scale byte below lo or at / past hi is read.
    // (wl, wr <= 2^30, coff < 2^28, a token < 2^20: the sums stay inside an int)
    const int hi = MOD ? max(0, min(lk, qhi + coff + md.wr + 1)) : p.causal ? max(0, min(lk, qhi + coff + 1)) : lk;
    const int lo = MOD ? max(0, qlo + coff - md.wl) & ~(KT - 1) : 0;
    const int nt = MOD ? (hi > lo ? (hi - lo + KT - 1) / KT : 0) : (hi + KT - 1) / KT;
    const int t0 = (int)((long long)s * nt / S), t1 = (int)((long long)(s + 1) * nt / S);
    const int kbeg = lo + t0 * KT, kend = min(hi, lo + t1 * KT);

    // this lane's query row: token qi, query head hd; its last visible key rw.rhi (MOD: it sees keys [rw.rlo, rw.rhi])
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
            // 16 keys x 8 channels a lane and pass of 128 channels, the nibble transpose, 8 bytes a channel into the image
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

    // ---- epilogue: O^T register i of block dvb is channel 32 dvb + 4 h + (i & 3) + 8 (i >> 2) of the lane's query row
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
__global__ __launch_bounds__(256) void fp4kv_append_kernel(const Fp4AppendParams p) {
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

}  // namespace

// The route and the profiler id of a call: the 128 kernels keep the names they had before the other widths came (plain and
// featured), every call at 64 / 256 counts under _hdim.
hipError_t launch_fp4_kvcache_append(const Fp4AppendArgs& a, hipStream_t st) {
    if (a.d != 64 && a.d != 128 && a.d != 256) return hipErrorInvalidValue;
    const Fp4AppendParams p = fp4_append_params(a);
    const dim3 grid((unsigned)((a.seqlen_new * a.c.heads_kv * (a.d / 16) + 255) / 256), (unsigned)a.batch);
    route_hit(a.d == 128 ? ROUTE_FP4KV_APPEND : ROUTE_FP4KV_APPEND_HDIM);
    ProfScope ps(a.d == 128 ? K_FP4KV_APPEND : K_FP4KV_APPEND_HDIM, st);
    fp4h_width(a.d, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        if (a.dtype == 2) hipLaunchKernelGGL((fp4kv_append_kernel<bf16_tag, D>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((fp4kv_append_kernel<f16_tag, D>), grid, dim3(256), 0, st, p);
    });
    return hipGetLastError();
}

hipError_t launch_fp4_kvcache(const Fp4KvArgs& a, const Fp8Mod& m, hipStream_t st) {
    if (a.d != 64 && a.d != 128 && a.d != 256) return hipErrorInvalidValue;
    if (m.sinks && a.num_splits < 2) return hipErrorInvalidValue;   // (the C layer raises a sink call's S to 2: the sink joins in the combine)
    const Fp4KvParams p = fp4_kv_params(a, (int)a.d);
    const int S = (int)a.num_splits;
    const dim3 grid((unsigned)S, (unsigned)((p.rows + 31) / 32 * p.hkv), (unsigned)a.batch);
    const KvqMod md = kvq_mod_args(m, a.causal != 0);
    route_hit(a.d != 128 ? ROUTE_FP4KV_SPLIT_HDIM : m.any() ? ROUTE_FP4KV_SPLIT_MOD : ROUTE_FP4KV_SPLIT);
    {
        ProfScope ps(a.d != 128 ? K_FP4KV_SPLIT_HDIM : m.any() ? K_FP4KV_SPLIT_MOD : K_FP4KV_SPLIT, st);
        fp4h_width(a.d, [&](auto dc) {
            constexpr int D = decltype(dc)::value;
            kvq_dispatch(a.dtype, a.c.block_table != nullptr, [&](auto tag, auto paged) {
                using T = decltype(tag);
                constexpr bool P = decltype(paged)::value;
                if constexpr (D == 128) {
                    if (m.any()) hipLaunchKernelGGL((fp4kv_split_kernel<T, P, KvqMod>), grid, dim3(64), 0, st, p, md);
                    else hipLaunchKernelGGL((fp4kv_split_kernel<T, P>), grid, dim3(64), 0, st, p);
                } else {
                    if (m.any()) hipLaunchKernelGGL((fp4kv_split_hdim_kernel<T, P, D, KvqMod>), grid, dim3(64), 0, st, p, md);
                    else hipLaunchKernelGGL((fp4kv_split_hdim_kernel<T, P, D>), grid, dim3(64), 0, st, p);
                }
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

}  // namespace fa
