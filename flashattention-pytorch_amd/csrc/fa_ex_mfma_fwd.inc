// Kernel body, included by the kernel entries of fa_ex_mfma.hip (the plain and the score-modifier entry of one kernel share
// it textually, so that each entry is compiled as the one function it was before the score modifiers; a device function
// called from both changes the code of the existing entries).  In scope: the kernel's parameters, p an ExParams or an
// ExParamsS (kFeatScore) or an ExParamsK (kFeatSink), or one of them grown by the pages (kFeatPaged: ExParamsPg), and the
// template parameters Tag, D, FEAT.

    constexpr int NW = 8, BM = 32 * NW, KB = 4, BN = 32 * KB, NKS = D / 16, NDV = D / 32, TILE_BYTES = BN * D * 2;
    constexpr bool VAR = (FEAT & kFeatVarlen) != 0, SC = (FEAT & kFeatScore) != 0, SNK = (FEAT & kFeatSink) != 0;
    constexpr bool PG = (FEAT & kFeatPaged) != 0;   // k, v are pools read through a block table: only `stage` differs
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][K tile | V tile]
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
    const size_t lbase = VAR ? (size_t)hh * p.total_q + sq0 : (size_t)bh * nq;
    const int qrow = q0 + 32 * w + r;

    const buf_rsrc_t q_rs = make_rsrc(q + qbase, VAR ? span_bytes(nq, DR, p.sq) : (unsigned)nq * DR * 2);
    s16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = buf_load_frag(q_rs, frag_off<VAR>(qrow, 16 * ks + 8 * h, DR, true, VAR ? p.sq : DR));

    const rsrc_s_t k_rs = make_rsrc_s(k + kbase, VAR ? span_bytes(nk, DR, p.sk) : (unsigned)nk * DR * 2);
    const rsrc_s_t v_rs = make_rsrc_s(v + vbase, VAR ? span_bytes(nk, DR, p.sv) : (unsigned)nk * DR * 2);
    const int dma_voff = dma_lane_voff<D, VAR>(lane, w, DR, VAR ? p.sk : DR);
    const int dma_voff_v = VAR ? dma_lane_voff<D, VAR>(lane, w, DR, p.sv) : dma_voff;
    [[maybe_unused]] const int* pg_row = nullptr;   // kFeatPaged: this sequence's table row and its last slot in use
    [[maybe_unused]] int pg_last = 0;
    if constexpr (PG) {
        pg_row = pg_of<FEAT>(p).table + (size_t)ub * pg_of<FEAT>(p).max_blocks;
        pg_last = pg_slot(pg_of<FEAT>(p), max(nk, 1) - 1);
    }
    auto stage = [&](int buf, int k0) {
        char* kb_ = smem + buf * 2 * TILE_BYTES;
        if constexpr (PG) {
            dma_stage_kv_paged<D, BN, NW>(pg_of<FEAT>(p), pg_row, pg_last, k + kbase, v + vbase, kb_, kb_ + TILE_BYTES, k0, nk, dma_voff,
                                          dma_voff_v, w, DR, p.sk, p.sv);
        } else {
            dma_stage_tile<D, BN, NW, VAR>(k_rs, kb_, k0, dma_voff, w, DR, 0, VAR ? p.sk : DR);
            dma_stage_tile<D, BN, NW, VAR>(v_rs, kb_ + TILE_BYTES, k0, dma_voff_v, w, DR, 0, VAR ? p.sv : DR);
        }
    };
    const MaskSrc msk = make_mask_src(p, bh);
    const bool use_bm = (FEAT & kFeatMask) && p.bmask != nullptr;
    const bool drop = (FEAT & kFeatDrop) && p.p_drop > 0.f;
    const unsigned hi = (unsigned)bh * p.nqh + ((unsigned)qrow >> 1);
    const int rbw = min(q0 + 32 * w, nq - 1) / p.br;   // block row of this wave's 32 rows (br is a multiple of 32)
    [[maybe_unused]] float al = 0.f;
    if constexpr (SC) al = alibi_k(sc_of<FEAT>(p), bh);
    [[maybe_unused]] float snk = -INFINITY;   // this unit's sink logit (kFeatSink): workgroup-uniform, one scalar load
    if constexpr (SNK) snk = ex_sink(sink_of<FEAT>(p), bh);

    f32x16 oacc[NDV];
#pragma unroll
    for (int t = 0; t < NDV; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[t][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // keys past the last row's diagonal are masked for every row of the tile (of the wave)
    constexpr bool WIN = (FEAT & kFeatWindow) != 0;
    // window: the band's right edge takes the diagonal's place (wr = 0 under the causal mask), and keys left of the first
    // row's left edge are masked for every row as well: tiles [t_lo, ntiles) for the workgroup, [t_lo_w, ntiles_w) per wave,
    // both bounded by the last row < nq (a wave without one computes nothing)
    const int kend = WIN ? max(0, min(nk, min(q0 + BM, nq) + p.coff + p.wr)) : (p.causal ? max(0, min(nk, q0 + BM + p.coff)) : nk);
    const int kend_w = WIN ? (q0 + 32 * w < nq ? max(0, min(nk, min(q0 + 32 * w + 32, nq) + p.coff + p.wr)) : 0)
                           : (p.causal ? max(0, min(nk, q0 + 32 * w + 32 + p.coff)) : nk);
    const int ntiles = (kend + BN - 1) / BN, ntiles_w = (kend_w + BN - 1) / BN;
    const int t_lo = WIN ? max(0, q0 + p.coff - p.wl) / BN : 0;
    const int t_lo_w = WIN ? max(0, q0 + 32 * w + p.coff - p.wl) / BN : 0;
    LiveScan<true, BN> scan;   // (tiles keep their absolute index: the scan's first probe is at t_lo)
    if (use_bm) scan.init(p, q0, min(q0 + BM, nq), 0, nk, ntiles, lane);
    auto next_live = [&](int t) { return use_bm ? scan.next(t) : t; };
    const int li = lane & 15, g16 = (lane >> 4) & 1, tq = li >> 2, tp = li & 3;

    int t = next_live(t_lo), cur = 0;
    if (t < ntiles) stage(0, t * BN);
    dma_wait_all();
    __syncthreads();
    if constexpr (WIN) {
        // leading feed-only tiles: left of this wave's band, inside the workgroup's
        while (t < min(t_lo_w, ntiles)) {
            const int tn = next_live(t + 1);
            if (tn < ntiles) stage(cur ^ 1, tn * BN);
            dma_wait_all();
            __syncthreads();
            cur ^= 1;
            t = tn;
        }
    }
    // two loops instead of an `if` inside one (a conditional accumulate makes hipcc carry the accumulators through
    // copies): tiles this wave computes, then the ones it only helps to load
    // Dense mask: its loads are ordinary VMEM loads, and VMEM returns in order — were the next tile's LDS-DMA issued
    // first, the wait for the mask words would also be a wait for that whole tile.  So the DMA goes out when the mask has
    // been read (it still has the tile's products to land).  Fetching the words a tile ahead instead (16 more live
    // registers) was measured slower: 1.15 vs 1.08 ms forward at BH 64, N 4096, half the pairs masked.
    const bool late_stage = (FEAT & kFeatMask) && msk.on;
    while (t < ntiles_w) {
        const int tn = next_live(t + 1);
        if (!late_stage && tn < ntiles) stage(cur ^ 1, tn * BN);
        const int k0 = t * BN;
        const char* Kt = smem + cur * 2 * TILE_BYTES;
        const char* Vt = Kt + TILE_BYTES;
        {
            // visibility / keep bits of this lane's 4 x 16 elements, requested ahead of the S MFMAs
            unsigned vis[KB], kp[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                vis[kb] = 0xffffu;
                kp[kb] = 0xffffu;
                if constexpr (FEAT & kFeatMask) {
                    if (msk.on) vis[kb] = dense_bits_q(msk, qrow, nk, k0 + 32 * kb + 4 * h, h);
                    if (use_bm && p.bmask[rbw * p.nbc + min(k0 + 32 * kb, nk - 1) / p.bc] == 0) vis[kb] = 0;
                }
                if constexpr (FEAT & kFeatDrop) {
                    if (drop) kp[kb] = keep_bits_q(p, hi, qrow, k0 + 32 * kb + 4 * h);
                }
            }
            // a tile of which this wave sees nothing (the upper triangle of a causal mask handed over as a dense one, the
            // dead blocks of a block-sparse tile) is not computed: wave-uniform
            bool any_vis = true;
            if constexpr (FEAT & kFeatMask) {
                unsigned all = 0;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) all |= vis[kb];
                any_vis = __any(all != 0) != 0;
                if (late_stage && tn < ntiles) stage(cur ^ 1, tn * BN);   // the mask words have arrived
            }
            if (any_vis) {
            f32x16 sacc[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const s16x8 a = *reinterpret_cast<const s16x8*>(Kt + TileSwz<D>::off(32 * kb + r, 2 * ks + h));
                    sacc[kb] = mfma32<Tag>(a, qf[ks], sacc[kb]);
                }
            }
            if constexpr (SC) {   // ---- score modifiers (wave-uniform switches), before every mask
                if (sc_of<FEAT>(p).cap_a > 0.f) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                        for (int i = 0; i < 16; ++i) { float dt; sacc[kb][i] = mod_softcap(sacc[kb][i], sc_of<FEAT>(p), dt); }
                }
                if (sc_of<FEAT>(p).alibi) {
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) {
                        const float fb = (float)(qrow + p.coff - (k0 + 32 * kb + 4 * h));   // dist of register i: fb - rc(i)
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[kb][i] = mod_alibi(sacc[kb][i], al, fb - (float)rc_of(i));
                    }
                }
            }
            // ---- causal diagonal / ragged last tile: key index of register i is k0 + 32 kb + 4 h + rc(i)
            const bool need_mask = WIN ? ((k0 + BN - 1 > q0 + 32 * w + p.coff + p.wr) || (k0 + BN > nk) ||
                                          (k0 < q0 + 32 * w + 31 + p.coff - p.wl))   // + the band's left edge
                                       : ((p.causal && (k0 + BN - 1 > q0 + 32 * w + p.coff)) || (k0 + BN > nk));
            if (need_mask) {
                // last visible key of this lane's row
                const int lim = WIN ? min(qrow + p.coff + p.wr, nk - 1) : (p.causal ? min(qrow + p.coff, nk - 1) : nk - 1);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const int thr = lim - (k0 + 32 * kb + 4 * h);
                    if constexpr (WIN) {
                        const int thl = qrow + p.coff - p.wl - (k0 + 32 * kb + 4 * h);   // the row's first visible key
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            if (rc_of(i) > thr || rc_of(i) < thl) sacc[kb][i] = -INFINITY;
                    } else {
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            if (rc_of(i) > thr) sacc[kb][i] = -INFINITY;
                    }
                }
            }
            if constexpr (FEAT & kFeatMask) {
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
                    if (__any(vis[kb] != 0xffffu)) {   // wave-uniform
#pragma unroll
                        for (int i = 0; i < 16; ++i) sacc[kb][i] = keep_or_minus_inf(sacc[kb][i], vis[kb], i);
                    }
            }
            // ---- online softmax (fa_fwd_mfma.hip), with rows that have not met a visible key yet (m = -inf)
            float mx = sacc[0][0];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
            mx = fmaxf(mx, wave_half_swap(mx));
            const float m_new = fmaxf(m_run, mx);
            float mc;
            // lazy rescale: keep the stale max while no row has grown past it by more than 2^8; -inf - -inf = NaN counts
            // as "rescale", so a wave with a dead row takes the exact path
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
                    float pe = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], c_log2, -mc));
                    rs += pe;   // the denominator counts every visible key, dropped or not
                    if constexpr (FEAT & kFeatDrop) pe = ((kp[kb] >> i) & 1u) ? pe * p.keep_scale : 0.f;
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
                        const s16x4 lo = lds_tr16(Vt + TileSwz<D>::off(key_a, ch) + 8 * (tp & 1));
                        const s16x4 hi4 = lds_tr16(Vt + TileSwz<D>::off(key_a + 8, ch) + 8 * (tp & 1));
                        oacc[dvb] = mfma32<Tag>(cat8(lo, hi4), pb, oacc[dvb]);
                    }
                }
            }
            l_run += rs;
            }   // any_vis
        }
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

    // ---- epilogue: normalise, store O and lse.  Every wave is past the last barrier and nothing is in flight: each wave
    // stages its rows in 32 x D x 2 bytes of buffer 0
    const float l_tot = l_run + wave_half_swap(l_run);
    float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    [[maybe_unused]] float lse_k = 0.f;
    if constexpr (SNK) {   // the sink column (a head at -inf keeps the formulas of the call without sinks: the same bits)
        lse_k = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
        if (snk != -INFINITY) ex_sink_norm(l_tot > 0.f ? m_run * p.scale : -INFINITY, l_tot, snk, inv, lse_k);
    }
    u32x2 vals[NDV * 4];
#pragma unroll
    for (int dvb = 0; dvb < NDV; ++dvb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vals[4 * dvb + g][0] = pack2_rn<Tag>(oacc[dvb][4 * g + 0] * inv, oacc[dvb][4 * g + 1] * inv);
            vals[4 * dvb + g][1] = pack2_rn<Tag>(oacc[dvb][4 * g + 2] * inv, oacc[dvb][4 * g + 3] * inv);
        }
    store_rows_via_lds<D, VAR>(smem + w * 32 * D * 2, vals, o + obase, q0 + 32 * w, nq, lane, DR, -1, p.hq * DR);
    if constexpr (SNK) {
        if (qrow < nq && h == 0) lse[lbase + qrow] = lse_k;
    } else {
        if (qrow < nq && h == 0) lse[lbase + qrow] = l_tot > 0.f ? m_run * p.scale + logf(l_tot) : -INFINITY;
    }
