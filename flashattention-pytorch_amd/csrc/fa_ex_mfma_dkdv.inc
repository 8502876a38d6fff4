// Kernel body, included by the kernel entries of fa_ex_mfma.hip (the plain and the score-modifier entry of one kernel share
// it textually, so that each entry is compiled as the one function it was before the score modifiers; a device function
// called from both changes the code of the existing entries).  In scope: the kernel's parameters, p an ExParams or an
// ExParamsS (kFeatScore), and the template parameters Tag, D, FEAT.

    constexpr int NW = 8, BK = 32 * NW, BQ = 64, NKS = D / 16, NDB = D / 32;
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0, SC = (FEAT & kFeatScore) != 0;
    constexpr int K_BYTES = BK * D * 2, Q_BYTES = BQ * D * 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                      // [256][D]
    char* Qs = Ks + K_BYTES;              // [2][64][D]
    char* Os = Qs + 2 * Q_BYTES;          // [2][64][D]   (dO)
    float* Ls = reinterpret_cast<float*>(Os + 2 * Q_BYTES);  // [2][ 64 x -lse/scale | 64 x -delta ]
    const int DR = p.d;
    int nq = p.nq, nk = p.nk;
    const int nkt = (nk + BK - 1) / BK;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nkt;
    const int key0 = (L - bh * nkt) * BK;
    EXM_VARLEN_UNIT(key0, nk)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const size_t qbase = VAR ? (size_t)sq0 * p.sq + hh * DR : (size_t)bh * nq * DR;
    const size_t kbase = VAR ? (size_t)sk0 * p.sk + hk * DR : (size_t)kv_unit(bh, p.kvg) * nk * DR;
    const size_t vbase = VAR ? (size_t)sk0 * p.sv + hk * DR : kbase;
    const size_t obase = VAR ? ((size_t)sq0 * p.hq + hh) * DR : qbase;
    const size_t rbase = VAR ? (size_t)hh * p.total_q + sq0 : (size_t)bh * nq;
    const int kw0 = key0 + 32 * w, key = kw0 + r;

    const rsrc_s_t k_rs = make_rsrc_s(k + kbase, VAR ? span_bytes(nk, DR, p.sk) : (unsigned)nk * DR * 2);
    const rsrc_s_t q_rs = make_rsrc_s(q + qbase, VAR ? span_bytes(nq, DR, p.sq) : (unsigned)nq * DR * 2);
    const rsrc_s_t o_rs = make_rsrc_s(dout + obase, VAR ? span_bytes(nq, DR, p.hq * DR) : (unsigned)nq * DR * 2);
    const rsrc_s_t l_rs = make_rsrc_s(nlse + rbase, (unsigned)nq * 4);
    const rsrc_s_t d_rs = make_rsrc_s(ndelta + rbase, (unsigned)nq * 4);
    const buf_rsrc_t v_rs = make_rsrc(v + vbase, VAR ? span_bytes(nk, DR, p.sv) : (unsigned)nk * DR * 2);
    const int dma_voff = dma_lane_voff<D, VAR>(lane, w, DR, VAR ? p.sq : DR);
    const int dma_voff_o = VAR ? dma_lane_voff<D, VAR>(lane, w, DR, p.hq * DR) : dma_voff;
    auto stage = [&](int buf, int qs) {
        dma_stage_tile<D, BQ, NW, VAR>(q_rs, Qs + buf * Q_BYTES, qs, dma_voff, w, DR, 0, VAR ? p.sq : DR);
        dma_stage_tile<D, BQ, NW, VAR>(o_rs, Os + buf * Q_BYTES, qs, dma_voff_o, w, DR, 0, VAR ? p.hq * DR : DR);
        // row constants: 64 floats each, one 4-byte LDS-DMA per lane (rows >= nq read as 0: harmless, their dO is 0)
        if (w == 0) dma4_issue(l_rs, lds_addr_of(Ls + buf * 128), lane * 4, __builtin_amdgcn_readfirstlane(qs * 4));
        if (w == 1) dma4_issue(d_rs, lds_addr_of(Ls + buf * 128 + 64), lane * 4, __builtin_amdgcn_readfirstlane(qs * 4));
    };
    const MaskSrc msk = make_mask_src(p, bh);
    const bool use_bm = (FEAT & kFeatMask) && p.bmask != nullptr;
    const bool drop = (FEAT & kFeatDrop) && p.p_drop > 0.f;
    const int cbw = min(kw0, nk - 1) / p.bc;   // block column of this wave's 32 keys (bc is a multiple of 32)
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = alibi_k(sc_of<FEAT>(p), bh);

    if constexpr (VAR) dma_stage_tile<D, BK, NW, VAR>(k_rs, Ks, key0, dma_lane_voff<D, VAR>(lane, w, DR, p.sk), w, DR, 0, p.sk);
    else dma_stage_tile<D, BK, NW>(k_rs, Ks, key0, dma_voff, w, DR);
    s16x8 vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) vf[ks] = buf_load_frag(v_rs, frag_off<VAR>(key, 16 * ks + 8 * h, DR, true, VAR ? p.sv : DR));

    f32x16 dka[NDB], dva[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { dka[t][i] = 0.f; dva[t][i] = 0.f; }

    // key j is visible from row j - coff on: earlier query tiles see none of this workgroup's (this wave's) keys
    constexpr bool WIN = (FEAT & kFeatWindow) != 0;
    // window: key j is visible from row j - coff - wr to row j - coff + wl; rows past the last key's band see none of
    // the workgroup's (query tiles [0, ntile)) or of this wave's keys (iterations [it_first, it_last) compute)
    const int qs_first = WIN ? (max(0, key0 - p.coff - p.wr) / BQ) * BQ : (p.causal ? (max(0, key0 - p.coff) / BQ) * BQ : 0);
    const int qend = WIN ? min(nq, min(key0 + BK, nk) - p.coff + p.wl) : nq;
    const int ntile = qs_first < qend ? (qend - qs_first + BQ - 1) / BQ : 0;
    const int it_first = WIN ? max(0, kw0 - p.coff - p.wr) / BQ - qs_first / BQ
                             : (p.causal ? max(0, kw0 - p.coff) / BQ - qs_first / BQ : 0);
    const int it_last = WIN ? (kw0 < nk ? min(ntile, (max(0, min(nq, min(kw0 + 32, nk) - p.coff + p.wl)) + BQ - 1) / BQ - qs_first / BQ) : 0)
                            : ntile;
    LiveScan<false, BQ> scan;
    if (use_bm) scan.init(p, key0, min(key0 + BK, nk), qs_first, nq, ntile, lane);   // (window: over the band's tiles)
    auto next_live = [&](int it) { return use_bm ? scan.next(it) : it; };
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int it = next_live(0), cur = 0;
    if (it < ntile) stage(0, qs_first + it * BQ);
    dma_wait_all();
    __syncthreads();
    // feed-only iterations first (tiles before this wave's first visible row), then the computing ones
    while (it < min(it_first, ntile)) {
        const int itn = next_live(it + 1);
        if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        it = itn;
    }
    while (it < it_last) {
        const int itn = next_live(it + 1);
        if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
        const int qs = qs_first + it * BQ;
        const char* Qt = Qs + cur * Q_BYTES;
        const char* Ot = Os + cur * Q_BYTES;
        const float* Lt = Ls + cur * 128;
#pragma unroll
        for (int qb = 0; qb < BQ / 32; ++qb) {
            const int rb0 = qs + 32 * qb;              // first row of the block; register i holds row rb0 + 4 h + rc(i)
            unsigned vis = 0xffffu, kp = 0xffffu;
            if constexpr (FEAT & kFeatMask) {
                if constexpr (M16) { if (msk.on) vis = dense_bits_k_lds(msk, rb0, nk, kw0, lane, reinterpret_cast<char*>(Ls + 2 * 128) + 1024 * w); }
                else if (msk.on) vis = dense_bits_k(msk, rb0 + 4 * h, nk, key);
                if (use_bm && p.bmask[(min(rb0, nq - 1) / p.br) * p.nbc + cbw] == 0) vis = 0;
            }
            if constexpr (FEAT & kFeatDrop) {
                if (drop) kp = keep_bits_k(p, (unsigned)bh * p.nqh, rb0 + 4 * h, key);
            }
            // a block of which this wave sees nothing is not computed (wave-uniform; see the forward kernel)
            if ((FEAT & kFeatMask) && !__any(vis != 0)) continue;
            // masked: the row precedes the key's first visible row (causal), or the key lies past nk: rc(i) < thr;
            // window: also the row follows the key's last visible row, rc(i) > thh
            const bool need_mask = WIN ? ((kw0 + 31 - p.coff - p.wr > rb0) || (kw0 + 32 > nk) || (rb0 + 31 > kw0 - p.coff + p.wl))
                                       : ((p.causal && (kw0 + 31 - p.coff > rb0)) || (kw0 + 32 > nk));
            const int thr = WIN ? (!need_mask ? -1 : (key >= nk ? 64 : key - p.coff - p.wr - rb0 - 4 * h))
                                : (!need_mask ? -1 : (key >= nk ? 64 : (p.causal ? key - p.coff - rb0 - 4 * h : -1)));
            [[maybe_unused]] const int thh = WIN && need_mask ? key - p.coff + p.wl - rb0 - 4 * h : 64;
            int kofs = 32 * w * 2 * D;
            asm volatile("" : "+v"(kofs));
            u32x4 pp[2], sp[2];
            [[maybe_unused]] u32x4 pu[2];   // dropout: the un-dropped 16-bit P (dS = P (dP_drop - delta)); score modifiers: P (1 - t^2)
            [[maybe_unused]] float dt[16];  // score modifiers: the softcap's derivative 1 - t^2
            {
                f32x16 sacc;
                // seeded with -lse / scale; with a score modifier S starts at 0, is modified, and then -lse / scale is added
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(Lt + 32 * qb + 8 * g + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (SC) sacc[4 * g + j] = 0.f;
                        else sacc[4 * g + j] = a[j];
                    }
                }
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const int ro = TileSwz<D>::off(r, 2 * ks + h);
                    const s16x8 qa = *reinterpret_cast<const s16x8*>(Qt + 32 * qb * 2 * D + ro);
                    const s16x8 kf = *reinterpret_cast<const s16x8*>(Ks + ro + kofs);
                    sacc = mfma32<Tag>(qa, kf, sacc);
                }
                if constexpr (SC) {
                    if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[i] = mod_softcap(sacc[i], sc_of<FEAT>(p), dt[i]);
                    }
                    if (sc_of<FEAT>(p).alibi) {
                        const float fb = (float)(rb0 + 4 * h + p.coff - key);   // dist of register i: fb + rc(i)
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[i] = mod_alibi(sacc[i], al, fb + (float)rc_of(i));
                    }
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(Lt + 32 * qb + 8 * g + 4 * h);
#pragma unroll
                        for (int j = 0; j < 4; ++j) sacc[4 * g + j] += a[j];
                    }
                }
                // wave-uniform: blocks that every lane sees whole (most of a structured mask) skip the selects
                // (score modifiers: the rows past nq of the last tile are masked as well — a zero dO no longer makes them
                // harmless, since a negative slope can make their modified score, taken against lse = 0, overflow exp2)
                const bool plain = !need_mask && (!(FEAT & kFeatMask) || !__any(vis != 0xffffu)) && (!SC || rb0 + 32 <= nq);
                if (plain) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) sacc[i] = __builtin_amdgcn_exp2f(sacc[i] * c_log2);
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        bool dead = rc_of(i) < thr;
                        if constexpr (WIN) dead = dead || rc_of(i) > thh;
                        if constexpr (SC) dead = dead || rc_of(i) >= nq - rb0 - 4 * h;
                        if constexpr (FEAT & kFeatMask) dead = dead || !((vis >> i) & 1u);
                        sacc[i] = dead ? 0.f : __builtin_amdgcn_exp2f(sacc[i] * c_log2);
                    }
                }
                if constexpr (SC) {
                    // the dS side of P: P (1 - t^2), multiplied in fp32 and packed once (dS = [P (1 - t^2)] (dP - delta), the
                    // product rounded to 16 bits where P alone is otherwise) — so dt does not live on across the dP product
                    if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                        for (int s = 0; s < 2; ++s)
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                pu[s][j] = pack2<Tag>(sacc[8 * s + 2 * j] * dt[8 * s + 2 * j], sacc[8 * s + 2 * j + 1] * dt[8 * s + 2 * j + 1]);
                    } else {
#pragma unroll
                        for (int s = 0; s < 2; ++s)
#pragma unroll
                            for (int j = 0; j < 4; ++j) pu[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
                    }
                    if constexpr (FEAT & kFeatDrop) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[i] = ((kp >> i) & 1u) ? sacc[i] * p.keep_scale : 0.f;
                    }
                } else if constexpr (FEAT & kFeatDrop) {
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int j = 0; j < 4; ++j) pu[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
#pragma unroll
                    for (int i = 0; i < 16; ++i) sacc[i] = ((kp >> i) & 1u) ? sacc[i] * p.keep_scale : 0.f;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) pp[s][j] = pack2<Tag>(sacc[8 * s + 2 * j], sacc[8 * s + 2 * j + 1]);
            }
            {
                f32x16 pacc;
                f32x4 ndv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) ndv[g] = *reinterpret_cast<const f32x4*>(Lt + 64 + 32 * qb + 8 * g + 4 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) pacc[4 * g + j] = (FEAT & kFeatDrop) ? 0.f : ndv[g][j];
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const s16x8 oa = *reinterpret_cast<const s16x8*>(Ot + 32 * qb * 2 * D + TileSwz<D>::off(r, 2 * ks + h));
                    pacc = mfma32<Tag>(oa, vf[ks], pacc);
                }
                if constexpr (FEAT & kFeatDrop) {   // dP' = keep / (1 - p) * (dO V^T) - delta
#pragma unroll
                    for (int i = 0; i < 16; ++i) pacc[i] = (((kp >> i) & 1u) ? pacc[i] * p.keep_scale : 0.f) + ndv[i >> 2][i & 3];
                }
                if constexpr (std::is_same<Tag, f16_tag>::value) mfma_result_fence(pacc);   // mul_pack<f16> reads pacc from asm
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        sp[s][j] = mul_pack<Tag>(((FEAT & kFeatDrop) || SC) ? pu[s][j] : pp[s][j], pacc[8 * s + 2 * j], pacc[8 * s + 2 * j + 1]);
                if constexpr (std::is_same<Tag, f16_tag>::value) asm volatile("s_nop 1" : "+v"(sp[0]), "+v"(sp[1]));
            }
            if (D > 64) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const s16x8 pb = *reinterpret_cast<s16x8*>(&pp[s]);
                const s16x8 sb = *reinterpret_cast<s16x8*>(&sp[s]);
                const int qa_ = 32 * qb + 16 * s + 4 * h + tq;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const int ch = 4 * db + 2 * g16 + (tp >> 1);
                    const int o1 = TileSwz<D>::off(qa_, ch) + 8 * (tp & 1);
                    const int o2 = TileSwz<D>::off(qa_ + 8, ch) + 8 * (tp & 1);
                    const s16x8 doT = cat8(lds_tr16(Ot + o1), lds_tr16(Ot + o2));
                    dva[db] = mfma32<Tag>(doT, pb, dva[db]);
                    const s16x8 qT = cat8(lds_tr16(Qt + o1), lds_tr16(Qt + o2));
                    dka[db] = mfma32<Tag>(qT, sb, dka[db]);
                }
                if (D > 64) __builtin_amdgcn_sched_barrier(0);
            }
        }
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        it = itn;
    }
    if constexpr (WIN) {
        // trailing feed-only iterations: rows past this wave's keys' band, inside the workgroup's
        while (it < ntile) {
            const int itn = next_live(it + 1);
            if (itn < ntile) stage(cur ^ 1, qs_first + itn * BQ);
            dma_wait_all();
            __syncthreads();
            cur ^= 1;
            it = itn;
        }
    }

    if (key < nk) {
        // dK / dV rows: per query head (grouped: the partials kv_group_sum adds up)
        // (varlen: rows of (total_k, hq, d) — the partials, or dk / dv themselves when hq = hkv)
        const size_t krow = VAR ? ((size_t)(sk0 + key) * p.hq + hh) * DR : ((size_t)bh * nk + key) * DR;
        uint16_t* dkrow = dk + krow;
        uint16_t* dvrow = dv + krow;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 a, b;
                a[0] = pack2_rn<Tag>(dka[db][4 * g + 0] * p.scale, dka[db][4 * g + 1] * p.scale);
                a[1] = pack2_rn<Tag>(dka[db][4 * g + 2] * p.scale, dka[db][4 * g + 3] * p.scale);
                b[0] = pack2_rn<Tag>(dva[db][4 * g + 0], dva[db][4 * g + 1]);
                b[1] = pack2_rn<Tag>(dva[db][4 * g + 2], dva[db][4 * g + 3]);
                if (32 * db + 8 * g + 4 * h >= DR) continue;   // padded columns (DR is a multiple of 8)
                *reinterpret_cast<u32x2*>(dkrow + 32 * db + 8 * g + 4 * h) = a;
                *reinterpret_cast<u32x2*>(dvrow + 32 * db + 8 * g + 4 * h) = b;
            }
    }
