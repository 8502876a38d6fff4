// Kernel body, included by the kernel entries of fa_ex_mfma.hip (the plain and the score-modifier entry of one kernel share
// it textually, so that each entry is compiled as the one function it was before the score modifiers; a device function
// called from both changes the code of the existing entries).  In scope: the kernel's parameters, p an ExParams or an
// ExParamsS (kFeatScore), and the template parameters Tag, D, FEAT.

    constexpr int NW = 8, BM = 32 * NW, BN = 64, NKS = D / 16, NDB = D / 32, TILE_BYTES = BN * D * 2;
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0, SC = (FEAT & kFeatScore) != 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][K tile | V tile]
    const int DR = p.d;
    int nq = p.nq, nk = p.nk;
    const int nqt = (nq + BM - 1) / BM;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = L / nqt;
    const int q0 = (L - bh * nqt) * BM;
    EXM_VARLEN_UNIT(q0, nq)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const size_t qbase = VAR ? (size_t)sq0 * p.sq + hh * DR : (size_t)bh * nq * DR;
    const size_t kbase = VAR ? (size_t)sk0 * p.sk + hk * DR : (size_t)kv_unit(bh, p.kvg) * nk * DR;
    const size_t vbase = VAR ? (size_t)sk0 * p.sv + hk * DR : kbase;
    const size_t obase = VAR ? ((size_t)sq0 * p.hq + hh) * DR : qbase;
    const size_t rbase = VAR ? (size_t)hh * p.total_q + sq0 : (size_t)bh * nq;
    const int ostr = VAR ? p.hq * DR : DR;   // rows of dout and dq
    const int qrow = q0 + 32 * w + r;
    const bool live_row = qrow < nq;

    const buf_rsrc_t q_rs = make_rsrc(q + qbase, VAR ? span_bytes(nq, DR, p.sq) : (unsigned)nq * DR * 2);
    const buf_rsrc_t o_rs = make_rsrc(dout + obase, VAR ? span_bytes(nq, DR, ostr) : (unsigned)nq * DR * 2);
    s16x8 qf[NKS], of[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        qf[ks] = buf_load_frag(q_rs, frag_off<VAR>(qrow, 16 * ks + 8 * h, DR, true, VAR ? p.sq : DR));
        of[ks] = buf_load_frag(o_rs, frag_off<VAR>(qrow, 16 * ks + 8 * h, DR, true, ostr));
    }
    const float nl = live_row ? nlse[rbase + qrow] : 0.f;
    const float nd = live_row ? ndelta[rbase + qrow] : 0.f;

    const rsrc_s_t k_rs = make_rsrc_s(k + kbase, VAR ? span_bytes(nk, DR, p.sk) : (unsigned)nk * DR * 2);
    const rsrc_s_t v_rs = make_rsrc_s(v + vbase, VAR ? span_bytes(nk, DR, p.sv) : (unsigned)nk * DR * 2);
    const int dma_voff = dma_lane_voff<D, VAR>(lane, w, DR, VAR ? p.sk : DR);
    const int dma_voff_v = VAR ? dma_lane_voff<D, VAR>(lane, w, DR, p.sv) : dma_voff;
    auto stage = [&](int buf, int k0) {
        char* kb_ = smem + buf * 2 * TILE_BYTES;
        dma_stage_tile<D, BN, NW, VAR>(k_rs, kb_, k0, dma_voff, w, DR, 0, VAR ? p.sk : DR);
        dma_stage_tile<D, BN, NW, VAR>(v_rs, kb_ + TILE_BYTES, k0, dma_voff_v, w, DR, 0, VAR ? p.sv : DR);
    };
    const MaskSrc msk = make_mask_src(p, bh);
    const bool use_bm = (FEAT & kFeatMask) && p.bmask != nullptr;
    const bool drop = (FEAT & kFeatDrop) && p.p_drop > 0.f;
    const unsigned hi = (unsigned)bh * p.nqh + ((unsigned)qrow >> 1);
    const int rbw = min(q0 + 32 * w, nq - 1) / p.br;
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = alibi_k(sc_of<FEAT>(p), bh);

    f32x16 dqa[NDB];
#pragma unroll
    for (int t = 0; t < NDB; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dqa[t][i] = 0.f;

    constexpr bool WIN = (FEAT & kFeatWindow) != 0;   // (the tile ranges of the forward kernel)
    const int kend = WIN ? max(0, min(nk, min(q0 + BM, nq) + p.coff + p.wr)) : (p.causal ? max(0, min(nk, q0 + BM + p.coff)) : nk);
    const int kend_w = WIN ? (q0 + 32 * w < nq ? max(0, min(nk, min(q0 + 32 * w + 32, nq) + p.coff + p.wr)) : 0)
                           : (p.causal ? max(0, min(nk, q0 + 32 * w + 32 + p.coff)) : nk);
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const int t_lo = WIN ? max(0, q0 + p.coff - p.wl) / BN : 0;
    const int t_lo_w = WIN ? max(0, q0 + 32 * w + p.coff - p.wl) / BN : 0;
    LiveScan<true, BN> scan;
    if (use_bm) scan.init(p, q0, min(q0 + BM, nq), 0, nk, ntiles, lane);
    auto next_live = [&](int t) { return use_bm ? scan.next(t) : t; };
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int t = next_live(t_lo), cur = 0;
    if (t < ntiles) stage(0, t * BN);
    dma_wait_all();
    __syncthreads();
    if constexpr (WIN) {
        while (t < min(t_lo_w, ntiles)) {   // leading feed-only tiles
            const int tn = next_live(t + 1);
            if (tn < ntiles) stage(cur ^ 1, tn * BN);
            dma_wait_all();
            __syncthreads();
            cur ^= 1;
            t = tn;
        }
    }
    const bool late_stage = (FEAT & kFeatMask) && msk.on;   // see the forward kernel
    while (t < ntiles_w) {
        const int tn = next_live(t + 1);
        if (!late_stage && tn < ntiles) stage(cur ^ 1, tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * 2 * TILE_BYTES;
        const char* Vt = Kt + TILE_BYTES;
        u32x4 dsb[2][2];
        unsigned visw[2] = {0xffffu, 0xffffu};
        if constexpr (FEAT & kFeatMask) {
            if (msk.on) {
                visw[0] = dense_bits_q(msk, qrow, nk, k0 + 4 * h, h);
                visw[1] = dense_bits_q(msk, qrow, nk, k0 + 32 + 4 * h, h);
                if (tn < ntiles) stage(cur ^ 1, tn * BN);
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
                if (use_bm && p.bmask[rbw * p.nbc + min(k0 + 32 * kb, nk - 1) / p.bc] == 0) visw[kb] = 0;
        }
        // a tile of which this wave sees nothing is not computed (wave-uniform; see the forward kernel)
        const bool any_vis = !(FEAT & kFeatMask) || __any((visw[0] | visw[1]) != 0) != 0;
        if (any_vis) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            unsigned vis = visw[kb], kp = 0xffffu;
            if constexpr (FEAT & kFeatDrop) {
                if (drop) kp = keep_bits_q(p, hi, qrow, k0 + 32 * kb + 4 * h);
            }
            f32x16 sacc, pacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if constexpr (SC) sacc[i] = 0.f;
                else sacc[i] = nl;
                pacc[i] = (FEAT & kFeatDrop) ? 0.f : nd;
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int off = TileSwz<D>::off(32 * kb + r, 2 * ks + h);
                const s16x8 ka = *reinterpret_cast<const s16x8*>(Kt + off);
                sacc = mfma32<Tag>(ka, qf[ks], sacc);
                const s16x8 va = *reinterpret_cast<const s16x8*>(Vt + off);
                pacc = mfma32<Tag>(va, of[ks], pacc);
            }
            [[maybe_unused]] float dt[16];
            if constexpr (SC) {   // modify S from 0, then add -lse / scale (the dK/dV kernel's order)
                if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        // dS = P (dP - delta) (1 - t^2) in fp32: without dropout dP - delta is final here, so dt goes in at once
                        float d;
                        sacc[i] = mod_softcap(sacc[i], sc_of<FEAT>(p), d);
                        if constexpr (FEAT & kFeatDrop) dt[i] = d;
                        else pacc[i] *= d;
                    }
                }
                if (sc_of<FEAT>(p).alibi) {
                    const float fb = (float)(qrow + p.coff - (k0 + 32 * kb + 4 * h));
#pragma unroll
                    for (int i = 0; i < 16; ++i) sacc[i] = mod_alibi(sacc[i], al, fb - (float)rc_of(i));
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[i] += nl;
            }
            const bool need_mask = WIN ? ((k0 + 32 * kb + 31 > q0 + 32 * w + p.coff + p.wr) || (k0 + 32 * kb + 32 > nk) ||
                                          (k0 + 32 * kb < q0 + 32 * w + 31 + p.coff - p.wl))
                                       : ((p.causal && (k0 + 32 * kb + 31 > q0 + 32 * w + p.coff)) || (k0 + 32 * kb + 32 > nk));
            const int lim = WIN ? min(qrow + p.coff + p.wr, nk - 1) : (p.causal ? min(qrow + p.coff, nk - 1) : nk - 1);
            const int thr = need_mask ? lim - (k0 + 32 * kb + 4 * h) : 64;
            [[maybe_unused]] const int thl = WIN && need_mask ? qrow + p.coff - p.wl - (k0 + 32 * kb + 4 * h) : -64;
            // wave-uniform (not in the dropout build: two copies of its selects cost registers it does not have)
            const bool plain = !(FEAT & kFeatDrop) && !need_mask && (!(FEAT & kFeatMask) || !__any(vis != 0xffffu));
            if (plain) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float dpv = pacc[i];
                    if constexpr (FEAT & kFeatDrop) dpv = (((kp >> i) & 1u) ? dpv * p.keep_scale : 0.f) + nd;
                    pacc[i] = __builtin_amdgcn_exp2f(sacc[i] * c_log2) * dpv;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    bool dead = rc_of(i) > thr;
                    if constexpr (WIN) dead = dead || rc_of(i) < thl;
                    if constexpr (FEAT & kFeatMask) dead = dead || !((vis >> i) & 1u);
                    float dpv = pacc[i];
                    if constexpr (FEAT & kFeatDrop) dpv = (((kp >> i) & 1u) ? dpv * p.keep_scale : 0.f) + nd;
                    pacc[i] = dead ? 0.f : __builtin_amdgcn_exp2f(sacc[i] * c_log2) * dpv;
                }
            }
            if constexpr (SC && (FEAT & kFeatDrop)) {   // dS *= 1 - t^2 in fp32, before the pack
                if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) pacc[i] *= dt[i];
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) dsb[kb][s][j] = pack2<Tag>(pacc[8 * s + 2 * j], pacc[8 * s + 2 * j + 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const s16x8 sb = *reinterpret_cast<s16x8*>(&dsb[kb][s]);
                const int key_a = 32 * kb + 16 * s + 4 * h + tq;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const int ch = 4 * db + 2 * g16 + (tp >> 1);
                    const s16x8 a = cat8(lds_tr16(Kt + TileSwz<D>::off(key_a, ch) + 8 * (tp & 1)),
                                         lds_tr16(Kt + TileSwz<D>::off(key_a + 8, ch) + 8 * (tp & 1)));
                    dqa[db] = mfma32<Tag>(a, sb, dqa[db]);
                }
            }
        }   // any_vis
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    while (t < ntiles) {
        const int tn = next_live(t + 1);
        if (tn < ntiles) stage(cur ^ 1, tn * BN);
        dma_wait_all();
        __syncthreads();
        cur ^= 1;
        t = tn;
    }
    if (live_row) {
        uint16_t* drow = dq + obase + (size_t)qrow * ostr;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (32 * db + 8 * g + 4 * h >= DR) continue;
                u32x2 val;
                val[0] = pack2_rn<Tag>(dqa[db][4 * g + 0] * p.scale, dqa[db][4 * g + 1] * p.scale);
                val[1] = pack2_rn<Tag>(dqa[db][4 * g + 2] * p.scale, dqa[db][4 * g + 3] * p.scale);
                *reinterpret_cast<u32x2*>(drow + 32 * db + 8 * g + 4 * h) = val;
            }
    }
