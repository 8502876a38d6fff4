// The append and split kernels of fa_decode.hip, included twice: KV_ROT 0 gives kv_append_kernel and kv_split_kernel, KV_ROT 1
// kv_append_rot_kernel and kv_split_rot_kernel (rotary embedding, KvRot).  One source, so the two cannot drift apart, and the
// kernels without rotation are compiled from exactly the text they had before the rotation existed.
// Two more inclusions with KV_Q8 1 give the same four kernels for an e4m3 cache (kv_*_q8_kernel, a KvQ8 as last argument):
// the cache is addressed in bytes, a chunk of 8 head dims is 8 bytes, K and V chunks are widened to q's 16-bit dtype in
// registers (kv_q8_widen) on their way into the unchanged 16-bit loop, and the append quantises (kv_q8_quant).  With KV_Q8 0
// every line below but one (the register constraint after the score MFMAs) preprocesses to what it was before KV_Q8 existed.
// Packed queries and new keys (fa_ex_forward_kvcache_varlen) are run-time null tests on p.cu_q / p.cu_kn in every inclusion.

// Token L_b + n of batch element b (k_new[b, n], or row cu_k_new[b] + n of a packed k_new) goes to cache row
// (bidx ? bidx[b] : b) at position L_b + n, or through the table to
// pool[table[b, (L_b + n) / ps], (L_b + n) % ps]; a row or page outside the cache / pool drops the token.
// KV_ROT: k_new[b, n] is rotated at position L_b - P_b + n on the way (Tag: its dtype).
#if KV_Q8 && KV_ROT
template <typename Tag>
__global__ __launch_bounds__(256) void kv_append_rot_q8_kernel(KvParams p, KvRot ro, KvQ8 q8) {
#elif KV_Q8
template <typename Tag>
__global__ __launch_bounds__(256) void kv_append_q8_kernel(KvParams p, KvQ8 q8) {
#elif KV_ROT
template <typename Tag>
__global__ __launch_bounds__(256) void kv_append_rot_kernel(KvParams p, KvRot ro) {
#else
__global__ __launch_bounds__(256) void kv_append_kernel(KvParams p) {
#endif
    const int cpr = p.d / 8;                                      // 16-byte chunks per head row
    const int b = blockIdx.y;
    int kn0, L, P;
    const int nnew = kv_seq_new(p, b, kn0);                       // packed k_new: nnew_b tokens from row kn0 (else N_new, 0)
    const long long per_b = (long long)nnew * p.hkv * cpr;
    kv_len_k(p, b, nnew, L, P);
    const long long kn_b = p.cu_kn ? (long long)kn0 * p.kn_ts : b * p.kn_bs, vn_b = p.cu_kn ? (long long)kn0 * p.vn_ts : b * p.vn_bs;
    long long row = b;
    if (p.bidx) {
        const int ix = p.bidx[b];
        if ((unsigned)ix >= (unsigned)p.bcache) return;
        row = ix;
    }
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < per_b; t += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(t % cpr);
        const long long r = t / cpr;
        const int h = (int)(r % p.hkv), n = (int)(r / p.hkv);
        const size_t col = (size_t)h * p.d + 8 * c;
        int pos = L + n;
        long long unit = row;
        if (p.table) {
            const int j = pos / p.ps;
            const int pg = p.table[b * p.tbl_rs + j];
            if ((unsigned)pg >= (unsigned)p.nblk) continue;
            pos -= j * p.ps;
            unit = pg;
        }
#if KV_ROT
        u32x4 kx = *reinterpret_cast<const u32x4*>(p.kn + kn_b + (size_t)n * p.kn_ts + col);
        if (8 * c < ro.rdim) {
            u32x4 par = kx;
            if (!ro.inter)
                par = *reinterpret_cast<const u32x4*>(p.kn + kn_b + (size_t)n * p.kn_ts + (size_t)h * p.d + kv_rot_partner(ro, 8 * c));
            kx = kv_rotate_chunk<Tag>(ro, L - P + n, 8 * c, kx, par);
        }
#else
        const u32x4 kx = *reinterpret_cast<const u32x4*>(p.kn + kn_b + (size_t)n * p.kn_ts + col);
#endif
        const u32x4 vx = *reinterpret_cast<const u32x4*>(p.vn + vn_b + (size_t)n * p.vn_ts + col);
#if KV_Q8
        // the (rotated, rounded) 16-bit values, quantised: one 8-byte store a chunk, the cache addressed in bytes
        const float kinv = 1.0f / (q8.kd ? q8.kd[b * q8.bs + h] : 1.0f), vinv = 1.0f / (q8.vd ? q8.vd[b * q8.bs + h] : 1.0f);
        uint8_t* kc8 = reinterpret_cast<uint8_t*>(p.kc);
        uint8_t* vc8 = reinterpret_cast<uint8_t*>(p.vc);
        *reinterpret_cast<u32x2*>(kc8 + unit * p.kc_bs + (size_t)pos * p.kc_ts + col) = kv_q8_quant<Tag>(kx, kinv);
        *reinterpret_cast<u32x2*>(vc8 + unit * p.vc_bs + (size_t)pos * p.vc_ts + col) = kv_q8_quant<Tag>(vx, vinv);
#else
        *reinterpret_cast<u32x4*>(p.kc + unit * p.kc_bs + (size_t)pos * p.kc_ts + col) = kx;
        *reinterpret_cast<u32x4*>(p.vc + unit * p.vc_bs + (size_t)pos * p.vc_ts + col) = vx;
#endif
    }
}

// One wave: split blockIdx.x of gridDim.x, row tile blockIdx.y / hkv and K/V head blockIdx.y % hkv, batch element blockIdx.z.
// Lane l: query row r = l & 15 of the tile (S^T's column, O^T's column), lane group g = l >> 4 (4 keys of each 16-key block
// of S^T, 4 head-dim elements of each 16-wide block of O^T).  D: the padded tile width (64 | 128 | 256), p.d <= D.
// PAGED: keys are reached through p.table (see the head of this file); otherwise through one buffer range per wave.
// KV_ROT: the q fragments are rotated (ro) before the key loop.
// KV_Q8: the cache holds e4m3 (q8: the scales of (b, hk)); each lane loads 8 bytes where it loaded 16 and widens them.
template <typename Tag, int D, bool PAGED>
#if KV_Q8 && KV_ROT
__global__ __launch_bounds__(64) void kv_split_rot_q8_kernel(KvParams p, KvRot ro, KvQ8 q8) {
#elif KV_Q8
__global__ __launch_bounds__(64) void kv_split_q8_kernel(KvParams p, KvQ8 q8) {
#elif KV_ROT
__global__ __launch_bounds__(64) void kv_split_rot_kernel(KvParams p, KvRot ro) {
#else
__global__ __launch_bounds__(64) void kv_split_kernel(KvParams p) {
#endif
    constexpr int KT = 32, NKS = D / 32, NDB = D / 16, CPR = D / 8, VLD = KT * CPR / 64;
    __shared__ __attribute__((aligned(16))) char vs[KT * D * 2];   // V tile, [key][D] in the TileSwz<D> image
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int s = blockIdx.x, S = gridDim.x;
    const int hk = blockIdx.y % p.hkv, rt = blockIdx.y / p.hkv, b = blockIdx.z;
    const int DR = p.d;
    // packed queries (p.cu_q): the sequence's nq_b tokens start at packed token tok0 and the grid is sized for max_seqlen_q, so
    // a wave whose row tile lies past the sequence's rows leaves before its first load.  Wave-uniform, scalar.
    long long tok0;
    const int nq = kv_seq_q(p, b, tok0), rows = p.G * nq;
    const int pr0 = 16 * rt, pr = pr0 + r;
    if (pr0 >= rows) return;
    int kn0, L_b, P_b;
    const int lk = kv_len_k(p, b, kv_seq_new(p, b, kn0), L_b, P_b), coff = lk - nq;
    const int qlo = pr0 / p.G, qhi = (min(pr0 + 16, rows) - 1) / p.G;
    int kbeg, kend;
    kv_split_range(p, lk, nq, qlo, qhi, s, S, kbeg, kend);

    // this lane's query row: token qi, query head h; its visible keys [rlo, rhi] (padding rows of the tile: none)
    const bool valid = pr < rows;
    const int qi = valid ? pr / p.G : qlo, h = hk * p.G + (valid ? pr - qi * p.G : 0);
    const int rlo = max(qi + coff - p.wl, kbeg);
    const int rhi = valid ? min(min(qi + coff + p.wr, lk - 1), kend - 1) : -1;
    float al = 0.f;
    if (p.alibi && valid) al = p.alibi[(size_t)b * p.al_bs + h] * p.sc.al_k;

    const buf_rsrc_t q_rs = make_rsrc(p.q + (p.cu_q ? tok0 * p.q_ts : b * p.q_bs), (unsigned)(((nq - 1) * p.q_ts + p.hq * DR) * 2));
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int col = 32 * ks + 8 * g;
        qf[ks] = buf_load_frag(q_rs, (valid && col < DR) ? (qi * p.q_ts + h * DR + col) * 2 : kOobOff);
    }
#if KV_ROT
    // fragment ks of this lane is the chunk at head dims 32 ks + 8 g of row (qi, h); rdim <= DR
    const long long qpos = L_b - P_b + (ro.qseq ? qi : 0);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int col = 32 * ks + 8 * g;
        if (valid && col < ro.rdim) {
            const u32x4 own = __builtin_bit_cast(u32x4, qf[ks]);
            u32x4 par = own;
            if (!ro.inter) par = __builtin_bit_cast(u32x4, buf_load_frag(q_rs, (qi * p.q_ts + h * DR + kv_rot_partner(ro, col)) * 2));
            qf[ks] = __builtin_bit_cast(s16x8, kv_rotate_chunk<Tag>(ro, qpos, col, own, par));
        }
    }
#endif
    // contiguous: the sequence's keys start P_b tokens into cache row (bidx ? bidx[b] : b); a row outside the cache is an empty range
    long long crow = b;
    int ctok = PAGED ? 0 : p.cap - P_b;   // tokens the buffer range holds
    if (!PAGED && p.bidx) {
        const int ix = p.bidx[b];
        crow = ix;
        if ((unsigned)ix >= (unsigned)p.bcache) { crow = 0; ctok = 0; }
    }
#if KV_Q8
    const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(p.kc);
    const uint8_t* vc8 = reinterpret_cast<const uint8_t*>(p.vc);
    const float kdsc = q8.kd ? q8.kd[b * q8.bs + hk] : 1.0f, vdsc = q8.vd ? q8.vd[b * q8.bs + hk] : 1.0f;
    const buf_rsrc_t k_rs = make_rsrc(kc8 + crow * p.kc_bs + (long long)P_b * p.kc_ts,
                                      ctok > 0 ? (unsigned)((ctok - 1) * p.kc_ts + p.hkv * DR) : 0u);
    const buf_rsrc_t v_rs = make_rsrc(vc8 + crow * p.vc_bs + (long long)P_b * p.vc_ts,
                                      ctok > 0 ? (unsigned)((ctok - 1) * p.vc_ts + p.hkv * DR) : 0u);
#else
    const buf_rsrc_t k_rs = make_rsrc(p.kc + crow * p.kc_bs + (long long)P_b * p.kc_ts,
                                      ctok > 0 ? (unsigned)(((ctok - 1) * p.kc_ts + p.hkv * DR) * 2) : 0u);
    const buf_rsrc_t v_rs = make_rsrc(p.vc + crow * p.vc_bs + (long long)P_b * p.vc_ts,
                                      ctok > 0 ? (unsigned)(((ctok - 1) * p.vc_ts + p.hkv * DR) * 2) : 0u);
#endif
    // paged: the table row, and the page j0 and slot s0 of the tile's first key (a 32-key tile spans at most three pages)
    const int* tbl = PAGED ? p.table + b * p.tbl_rs : nullptr;
    int j0 = 0, s0 = 0, pg = -1;
    auto page_of = [&](int jt, int st, int kt) {   // the table entry of key kt + (lane & 31), or -1 past the split's end
        int j = jt, sl = st + (lane & 31);
        if (sl >= p.ps) { sl -= p.ps; ++j; }
        if (sl >= p.ps) ++j;
        return kt + (lane & 31) < kend ? tbl[j] : -1;
    };
    if (PAGED && kbeg < kend) {
        j0 = kbeg / p.ps;
        s0 = kbeg - j0 * p.ps;
        pg = page_of(j0, s0, kbeg);
    }

    f32x4_t oacc[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t) oacc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const int q4 = r >> 2, p4 = r & 3;   // ds_read_b64_tr_b16: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p + 3

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        // K fragments (A of S^T = K Q^T: key k0 + 16 kb + r, head dims 32 ks + 8 g ..) and this lane's share of the V tile;
        // keys past the split's end read as zeros (the cache behind them may hold anything)
        s16x8 kf[2][NKS];
        u32x4 vr[VLD];
        if constexpr (PAGED) {
            // this lane's key k0 + (lane & 31): element offsets of its token in the two pools, -1 = reads as zeros
            long long ko = -1, vo = -1;
            {
                int sl = s0 + (lane & 31);
                if (sl >= p.ps) sl -= p.ps;
                if (sl >= p.ps) sl -= p.ps;
                if ((unsigned)pg < (unsigned)p.nblk) {
                    ko = pg * p.kc_bs + (long long)sl * p.kc_ts;
                    vo = pg * p.vc_bs + (long long)sl * p.vc_ts;
                }
            }
            s0 += KT;
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (s0 >= p.ps) { s0 -= p.ps; ++j0; }
            if (k0 + KT < kend) pg = page_of(j0, s0, k0 + KT);   // the next tile's lookup, a tile ahead of its use
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const long long ro = __shfl(ko, 16 * kb + r, 64);
#if KV_Q8
                const uint8_t* kp = kc8 + ro + hk * DR + 8 * g;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bool ok = ro >= 0 && 32 * ks + 8 * g < DR;
                    const u32x2 x = *reinterpret_cast<const u32x2*>(ok ? kp + 32 * ks : reinterpret_cast<const uint8_t*>(p.q));
                    kf[kb][ks] = __builtin_bit_cast(s16x8, kv_q8_widen<Tag>(ok ? x : u32x2{0u, 0u}));
                }
#else
                const uint16_t* kp = p.kc + ro + hk * DR + 8 * g;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bool ok = ro >= 0 && 32 * ks + 8 * g < DR;
                    const s16x8 x = *reinterpret_cast<const s16x8*>(ok ? kp + 32 * ks : p.q);
                    kf[kb][ks] = ok ? x : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
#endif
            }
#pragma unroll
            for (int i = 0; i < VLD; ++i) {
                const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR;
                const long long ro = __shfl(vo, row, 64);
                const bool ok = ro >= 0 && 8 * ch < DR;
#if KV_Q8
                const u32x2 x = *reinterpret_cast<const u32x2*>(ok ? vc8 + ro + hk * DR + 8 * ch : reinterpret_cast<const uint8_t*>(p.q));
                vr[i] = kv_q8_widen<Tag>(ok ? x : u32x2{0u, 0u});
#else
                const u32x4 x = *reinterpret_cast<const u32x4*>(ok ? p.vc + ro + hk * DR + 8 * ch : p.q);
                vr[i] = ok ? x : u32x4{0u, 0u, 0u, 0u};
#endif
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int key = k0 + 16 * kb + r;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const int col = 32 * ks + 8 * g;
#if KV_Q8
                    kf[kb][ks] = __builtin_bit_cast(s16x8, kv_q8_widen<Tag>(__builtin_amdgcn_raw_buffer_load_b64(
                        k_rs, (key < kend && col < DR) ? key * p.kc_ts + hk * DR + col : kOobOff, 0, 0)));
#else
                    kf[kb][ks] = buf_load_frag(k_rs, (key < kend && col < DR) ? (key * p.kc_ts + hk * DR + col) * 2 : kOobOff);
#endif
                }
            }
#pragma unroll
            for (int i = 0; i < VLD; ++i) {
                const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR, key = k0 + row;
#if KV_Q8
                vr[i] = kv_q8_widen<Tag>(__builtin_amdgcn_raw_buffer_load_b64(
                    v_rs, (key < kend && 8 * ch < DR) ? key * p.vc_ts + hk * DR + 8 * ch : kOobOff, 0, 0));
#else
                vr[i] = __builtin_amdgcn_raw_buffer_load_b128(v_rs, (key < kend && 8 * ch < DR) ? (key * p.vc_ts + hk * DR + 8 * ch) * 2 : kOobOff,
                                                              0, 0);
#endif
            }
        }
        f32x4_t sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) sacc[kb] = mfma16<Tag>(kf[kb][ks], qf[ks], sacc[kb]);
        }
        // both score tiles live in VGPRs at one point: without this hipcc ends the second chain in the first one's registers
        // (a[0:3] = .. + a[4:7]), a C operand that is not the destination, which tools/mfma_hazard_audit.py R1 does not pass
        // (the e4m3 kernels always did that; with the packed-query prologue the contiguous 16-bit D = 128 ones do as well)
        asm volatile("" : "+v"(sacc[0]), "+v"(sacc[1]));
        // (the previous tile's transposed reads were issued before these writes: one wave, LDS in order)
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const int idx = 64 * i + lane, row = idx / CPR, ch = idx - row * CPR;
            *reinterpret_cast<u32x4*>(vs + TileSwz<D>::off(row, ch)) = vr[i];
        }
        // score modifiers (before any mask, as in the extended kernels), then the row's band: register i of block kb holds key
        // k0 + 16 kb + 4 g + i
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 16 * kb + 4 * g + i;
#if KV_Q8
                float x = sacc[kb][i] * kdsc;   // s = softmax_scale * k_descale * (q . k_stored): before softcap and ALiBi
#else
                float x = sacc[kb][i];
#endif
                if (p.sc.cap_a > 0.f) { float dt; x = mod_softcap(x, p.sc, dt); }
                if (p.alibi) x = mod_alibi(x, al, (float)(qi + coff - key));
                x = (key >= rlo && key <= rhi) ? x : -INFINITY;
                sacc[kb][i] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * p.c_log2);
        const float mc = m_use * p.c_log2;
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int t = 0; t < NDB; ++t) oacc[t] *= alpha;
        // P^T as the B operand of O^T = V^T P^T: k-slot 8 g + j is key 4 g + j (j < 4) and 16 + 4 g + j - 4 (j >= 4)
        u32x4 pk;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float e0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][2 * j], p.c_log2, -mc));
                const float e1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][2 * j + 1], p.c_log2, -mc));
                l_run += e0 + e1;
                pk[2 * kb + j] = pack2<Tag>(e0, e1);
            }
        const s16x8 pb = *reinterpret_cast<s16x8*>(&pk);
        // V^T operand, the same k-slots: rows (keys) 4 g + q and 16 + 4 g + q, head dims 16 t + 4 p ..
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int ch = 2 * t + (p4 >> 1), bo = 8 * (p4 & 1);
            const s16x4 lo = lds_tr16(vs + TileSwz<D>::off(4 * g + q4, ch) + bo);
            const s16x4 hi = lds_tr16(vs + TileSwz<D>::off(16 + 4 * g + q4, ch) + bo);
            oacc[t] = mfma16<Tag>(cat8(lo, hi), pb, oacc[t]);
        }
    }

    // ---- epilogue: the row's sum over the four lane groups; O^T register i of block t is head dim 16 t + 4 g + i
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    const float lse_v = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    if (!valid) return;
    // o row (token, h) of the (packed or padded) token tok0 + qi; lse / partials row (b, h, qi), packed (h, token)
    const size_t row_id = p.cu_q ? (size_t)h * p.total_q + tok0 + qi : ((size_t)b * p.hq + h) * p.nq + qi;
    if (S == 1) {
        uint16_t* orow = p.o + ((size_t)(tok0 + qi) * p.hq + h) * DR;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int col = 16 * t + 4 * g;
            if (col < DR) {
                u32x2 v;
#if KV_Q8
                v[0] = pack2_rn<Tag>(oacc[t][0] * inv * vdsc, oacc[t][1] * inv * vdsc);
                v[1] = pack2_rn<Tag>(oacc[t][2] * inv * vdsc, oacc[t][3] * inv * vdsc);
#else
                v[0] = pack2_rn<Tag>(oacc[t][0] * inv, oacc[t][1] * inv);
                v[1] = pack2_rn<Tag>(oacc[t][2] * inv, oacc[t][3] * inv);
#endif
                *reinterpret_cast<u32x2*>(orow + col) = v;
            }
        }
        if (g == 0) p.lse[row_id] = lse_v;
    } else {
        float* prow = p.po + (row_id * S + s) * DR;
#pragma unroll
        for (int t = 0; t < NDB; ++t) {
            const int col = 16 * t + 4 * g;
#if KV_Q8
            if (col < DR) *reinterpret_cast<f32x4_t*>(prow + col) = oacc[t] * inv * vdsc;
#else
            if (col < DR) *reinterpret_cast<f32x4_t*>(prow + col) = oacc[t] * inv;
#endif
        }
        if (g == 0) p.plse[row_id * S + s] = lse_v;
    }
}
