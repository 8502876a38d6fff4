"""The fp8 calls at head dims 64, 128 and 256 (fwd_fp8in_hdim_kernel<Tag, MODE, D> in csrc/fa_fp8_inputs.hip,
fp8kv_split_mod_kernel<Tag, PAGED, D> in csrc/fa_fp8_decode.hip; fa_fp8_forward_hdim, fa_fp8_forward_varlen_hdim,
fa_fp8_forward_kvcache_hdim in csrc/fa_capi.hip) on the CPU (torch), one model with the head dim d as a parameter and two levels:

    reference(call), decode_reference(call)   the fp64 definition on the dequantised codes: the band of the window, the softcap
                                              before the mask, the sink column, dead rows (o = 0, lse = the sink or -inf)
    baseline(call), decode_baseline(call)     the kernels' arithmetic order: tests/fp8_mod_ref.baseline and
                                              tests/fp8_kvcache_mod_ref.baseline with d in the shapes and the key tile of d

What changes with d, each read from the kernels:
  * the raw score is d / 64 instructions of 64 terms, accumulated in float32 in ascending head-dim order (`for M < NM / 2`, `for M <
    NMQ`): fp8_ref._mfma_f8 over a contraction of d;
  * the prefill kernel's softmax step (raw maximum times f once, lazy rescale at 8 per 32-row wave, p = exp2(fma), P to e4m3, l from
    the unrounded p) covers 128 keys at d = 64 and 128 and 64 keys at d = 256 (`KBS`): key_tile(d).  The decode kernel's is 64 keys at
    every d;
  * o is d wide, and the V^T image has d rows a 128-key tile: v8t_bytes / workspace sizes below.
At d = 128 both baselines reproduce the pinned ones bit for bit (tests/test_fp8_hdim_cpu.py).

Prefill `call`: fp8_mod_ref's dict plus d.  Decode `call`: fp8_kvcache_mod_ref's dict plus d."""
import torch

from tests import fp8_inputs_cases as fc
from tests import fp8_inputs_ref as fr
from tests import fp8_kvcache_mod_ref as km
from tests import fp8_kvcache_ref as fk
from tests import fp8_mod_ref as fm
from tests.ex_full_ref import NEG_INF, _fma, _mm, round_to
from tests.fp8_ref import LN2_F, LOG2E_F, SENTINEL, _PV_KEY_OF_K, _mfma_f8, e4m3_code, e4m3_value

HEAD_DIMS = (64, 128, 256)
GAIN = 3.5                # fp8_mod_ref.INPUT_GAIN: with softmax_scale = d ** -0.5 the scaled scores have a deviation of 12 at every d


def key_tile(d):
    """keys of one softmax step of the prefill kernel (fwd_fp8in_hdim_kernel: BNS)"""
    return 64 if d == 256 else 128


# ---- the workspace sizes (include/fa_mi355x.h)

def forward_workspace_bytes(batch, heads_kv, seqlen_k, d):
    return batch * heads_kv * ((seqlen_k + 127) // 128) * d * 128 + 256


def varlen_workspace_bytes(batch, heads_kv, total_k, max_seqlen_k, max_blocks, page_size, d):
    tiles = batch * ((min(max_seqlen_k, max_blocks * page_size) + 127) // 128) if page_size else total_k // 128 + batch
    return heads_kv * tiles * d * 128 + 256


def kvcache_workspace_bytes(batch, heads_q, seqlen_q, d, splits):
    """fa_decode.hip, kv_workspace_bytes"""
    if splits <= 1:
        return 0
    rows = batch * heads_q * seqlen_q * splits
    return ((rows * d * 4 + 255) & ~255) + ((rows * 4 + 255) & ~255)


# ---- prefill

def make_call(d, n, causal=False, window=(-1, -1), softcap=0.0, sinks=None, dtype=torch.bfloat16, batch=2, hq=4, hkv=2, seed=0):
    """fp8_mod_ref.make_call at head dim d (other random numbers: the tensors have other shapes)"""
    nq, nk = n
    g = torch.Generator().manual_seed(777 + seed)
    gain = GAIN
    q = gain * torch.randn((batch, hq, nq, d), generator=g, dtype=torch.float32)
    k = gain * torch.randn((batch, hkv, nk, d), generator=g, dtype=torch.float32)
    v = torch.randn((batch, hkv, nk, d), generator=g, dtype=torch.float32)
    ds = {name: fc.odd_mantissa(0.05 * 4.0 ** torch.rand((batch, hkv), generator=g, dtype=torch.float32))
          for name in ("q_descale", "k_descale", "v_descale")}
    return dict(B=batch, hq=hq, hkv=hkv, nq=nq, nk=nk, d=d, causal=causal, dtype=dtype, scale=d ** -0.5, layout="bhnd", input="normal",
                q8=fc.quantise(q, ds["q_descale"].repeat_interleave(hq // hkv, dim=1)), k8=fc.quantise(k, ds["k_descale"]),
                v8=fc.quantise(v, ds["v_descale"]), window=tuple(window), softcap=float(softcap), sinks=sinks, **ds)


def the_sinks(hq):
    """N(0, 2) with one head at -inf and one at +1e4"""
    s = 2.0 * torch.randn((hq,), generator=torch.Generator().manual_seed(11), dtype=torch.float32)
    s[1], s[2] = float("-inf"), 1.0e4
    return s


def dequantised(call):
    """fp64 q (B * H_q, Nq, d), k, v (B * H_kv, Nk, d): code * descale"""
    qd, kd, vd = fr.descales(call)
    g, d = call["hq"] // call["hkv"], call["d"]
    q = e4m3_value(call["q8"]).double() * qd.double().repeat_interleave(g, dim=1)[:, :, None, None]
    k = e4m3_value(call["k8"]).double() * kd.double()[:, :, None, None]
    v = e4m3_value(call["v8"]).double() * vd.double()[:, :, None, None]
    return q.reshape(-1, call["nq"], d), k.reshape(-1, call["nk"], d), v.reshape(-1, call["nk"], d)


def reference(call):
    """the fp64 definition (fp8_mod_ref.evaluate's closed form at head dim d)"""
    q, k, v = dequantised(call)
    kvi = fr.kv_unit(call)
    s = _mm(q, k[kvi].transpose(1, 2)) * call["scale"]
    cap = call["softcap"]
    if cap > 0.0:
        s = cap * torch.tanh(s / cap)
    s = torch.where(fm.band(call), s, torch.tensor(NEG_INF, dtype=torch.float64))
    o, lse = fm.attend(s, v[kvi], fm.sink_column(call))
    return fr._result(o, lse)


def baseline(call, compute=torch.float32, rounding=True):
    """fp8_mod_ref.baseline with d in the shapes and key_tile(d) keys a softmax step"""
    ct = compute
    f32 = ct == torch.float32
    nb, hq, nq, nk, d = call["B"], call["hq"], call["nq"], call["nk"], call["d"]
    kt = key_tile(d)
    U = nb * hq
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    kvi = fr.kv_unit(call)
    q8 = e4m3_value(call["q8"]).to(ct).reshape(U, nq, d)
    k8 = e4m3_value(call["k8"]).to(ct).reshape(-1, nk, d)[kvi]
    v8 = e4m3_value(call["v8"]).to(ct).reshape(-1, nk, d)[kvi]
    qd, kd, vd = (t.reshape(-1)[kvi].to(ct) for t in fr.descales(call))
    if f32:
        c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)
        ln2 = torch.tensor(LN2_F, dtype=torch.float32)
    else:
        c_log2, ln2 = torch.tensor(call["scale"] * LOG2E_F, dtype=ct), torch.tensor(LN2_F, dtype=ct)
    f = ((c_log2 * qd) * kd)[:, None, None]                                        # (U, 1, 1): one factor per workgroup
    capped = call["softcap"] > 0.0
    if capped:
        cap_k, cap2 = fm.cap_constants(call, ct)
        ck = f * cap_k
        fe = torch.ones_like(f)
    else:
        fe = f
    zero, one, ninf = torch.zeros((), dtype=ct), torch.ones((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    vis_all = fm.band(call)
    snk = None if call["sinks"] is None else call["sinks"].to(ct).repeat(nb)       # (U,)
    o = torch.zeros((U, nq, d), dtype=ct)
    lse = torch.zeros((U, nq), dtype=ct)
    for r0 in range(0, nq, fr.ROW_TILE):
        r1 = min(r0 + fr.ROW_TILE, nq)
        nr = r1 - r0
        sacc = _mfma_f8(q8[:, r0:r1], k8.transpose(1, 2), ct, torch.zeros((U, nr, nk), dtype=ct), rounding)
        if capped:
            rr = 1.0 / (torch.exp2(sacc * ck) + 1.0)
            sacc = _fma(rr, (-2.0 * cap2).expand_as(rr), cap2.expand_as(rr), ct)
        sacc = torch.where(vis_all[r0:r1], sacc, ninf)
        m = torch.full((U, nr), NEG_INF, dtype=ct)
        l_ = torch.zeros((U, nr), dtype=ct)
        acc = torch.zeros((U, nr, d), dtype=ct)
        for t0 in range(0, nk, kt):
            sl = slice(t0, min(t0 + kt, nk))
            if not bool(vis_all[r0:r1, sl].any()):
                continue                                                            # (nothing visible: no change)
            mx = sacc[..., sl].max(-1).values * fe[:, :, 0]
            m_new = torch.maximum(m, mx)
            grow = m_new - m > 8.0                                                  # (first visible key: inf > 8; none yet: nan > 8 is False)
            pad = (-nr) % 32
            gw = torch.nn.functional.pad(grow, (0, pad)).reshape(U, -1, 32).any(-1, keepdim=True).expand(U, -1, 32).reshape(U, -1)[:, :nr]
            m_use = torch.where(gw, m_new, m)
            m_use = torch.where(m_use > NEG_INF, m_use, zero)
            alpha = torch.where(gw, torch.exp2(m - torch.where(m_new > NEG_INF, m_new, zero)), one)
            m = torch.where(gw, m_new, m)
            l_ = l_ * alpha
            acc = acc * alpha.unsqueeze(-1)
            w = sl.stop - sl.start
            p = torch.exp2(_fma(sacc[..., sl], fe.expand(U, nr, w), -m_use.unsqueeze(-1).expand(U, nr, w), ct))
            acc = _mfma_f8(p8(p), v8[:, sl], ct, acc, rounding, order=_PV_KEY_OF_K)
            l_ = l_ + p.sum(-1)
        dead = l_ == 0
        inv = vd[:, None] * (1.0 / l_)
        o_t = torch.where(dead.unsqueeze(-1), zero, rnd(acc * inv.unsqueeze(-1)))
        lse_t = torch.where(dead, ninf, (m + torch.log2(l_)) * ln2)
        if snk is not None:
            has = (snk > NEG_INF)[:, None].expand(U, nr)
            sk = torch.where(snk > NEG_INF, snk, zero)[:, None].expand(U, nr)
            iv, ls = fm.sink_norm(m * ln2, l_, sk, ct)
            o_t = torch.where(has.unsqueeze(-1), rnd(acc * (vd[:, None] * iv).unsqueeze(-1)), o_t)
            lse_t = torch.where(has, ls, lse_t)
        o[:, r0:r1], lse[:, r0:r1] = o_t, lse_t
    return fr._result(o, lse)


def sequence_call(call, b, nq, nk, zero_keys=None):
    """the padded call of one batch element's first nq queries and nk keys (what a packed or paged sequence is), optionally with keys
    [a, z) of K and V as zero bytes (a page outside the pool)"""
    k8, v8 = call["k8"][b:b + 1, :, :nk].clone(), call["v8"][b:b + 1, :, :nk].clone()
    if zero_keys is not None:
        k8[:, :, zero_keys[0]:zero_keys[1]], v8[:, :, zero_keys[0]:zero_keys[1]] = 0, 0
    return dict(call, B=1, nq=nq, nk=nk, q8=call["q8"][b:b + 1, :, :nq].contiguous(), k8=k8, v8=v8,
                **{n: call[n][b:b + 1] for n in ("q_descale", "k_descale", "v_descale")})


# ---- decode

def decode_call(d, heads, nq, lens, layout, splits, window=(-1, -1), sinks=False, causal=True, capacity=192, dtype=torch.bfloat16, seed=0):
    """fp8_kvcache_mod_ref.build_call's dict at head dim d: layout "ps16" (a shuffled table with garbage past a sequence's pages) or
    "bidx" (cache_batch_idx; the LAST sequence's index lies outside the cache: an empty sequence).  Bytes no live token owns are
    e4m3 NaN codes."""
    from tests import fp8_kvcache_cases as kc

    hq, hkv = heads
    nb = len(lens)
    g = torch.Generator().manual_seed(4100 + seed)
    gain = GAIN
    q = gain * torch.randn((nb, nq, hq, d), generator=g)
    k = gain * torch.randn((nb, capacity, hkv, d), generator=g)
    v = torch.randn((nb, capacity, hkv, d), generator=g)

    def quantise(x):          # kc.quantise's "bhkv" form, without its fixed head dim
        xg = x.reshape(x.shape[0], x.shape[1], hkv, x.shape[2] // hkv, d)
        ds = (xg.abs().amax(dim=(1, 3, 4)).clamp_min(1e-3) / 448.0).float()
        ds = (ds.contiguous().view(torch.int32) | 1).view(torch.float32)
        return kc.e4m3((xg / ds[:, None, :, None, None]).reshape(x.shape)), ds.contiguous()

    (q8, qd), (k8, kd), (v8, vd) = quantise(q), quantise(k), quantise(v)
    table, bidx = None, None
    if layout == "ps16":
        ps = 16
        need = [(n + ps - 1) // ps for n in lens]
        max_blocks, num_blocks = capacity // ps, sum(need) + 3
        perm = torch.randperm(num_blocks, generator=g).tolist()
        table = torch.randint(-5, num_blocks + 5, (nb, max_blocks), generator=g, dtype=torch.int32)
        kcache = torch.full((num_blocks, ps, hkv, d), SENTINEL, dtype=torch.uint8)
        vcache = torch.full((num_blocks, ps, hkv, d), SENTINEL, dtype=torch.uint8)
        for b, n in enumerate(lens):
            for j in range(need[b]):
                pg = perm.pop()
                table[b, j] = pg
                m = min(ps, n - j * ps)
                kcache[pg, :m], vcache[pg, :m] = k8[b, j * ps:j * ps + m], v8[b, j * ps:j * ps + m]
    else:
        rows = nb + 2
        kcache = torch.full((rows, capacity, hkv, d), SENTINEL, dtype=torch.uint8)
        vcache = torch.full((rows, capacity, hkv, d), SENTINEL, dtype=torch.uint8)
        where = [(2 * b + 3) % rows for b in range(nb)]
        assert len(set(where)) == nb
        for b, n in enumerate(lens):
            kcache[where[b], :n], vcache[where[b], :n] = k8[b, :n], v8[b, :n]
        where[-1] = rows + 2
        bidx = torch.tensor(where, dtype=torch.int32)
    return dict(B=nb, hq=hq, hkv=hkv, nq=nq, d=d, causal=causal, dtype=dtype, scale=d ** -0.5, num_splits=splits, q8=q8, k_cache=kcache,
                v_cache=vcache, cache_seqlens=torch.tensor(lens, dtype=torch.int32), block_table=table, cache_batch_idx=bidx,
                q_descale=qd, k_descale=kd, v_descale=vd, values="normal", window=tuple(window), softcap=0.0,
                sinks=the_sinks(hq) if sinks else None)


def pack(o, lse, call):
    """fp8_kvcache_ref.pack at head dim d: the Result in the kernel's row order of o (B, Nq, H_q, d), lse (B, H_q, Nq)"""
    nb, hkv, nq, d = call["B"], call["hkv"], call["nq"], call["d"]
    g = call["hq"] // hkv
    op = o.reshape(nb, nq, hkv, g, d).permute(0, 2, 1, 3, 4).reshape(nb * hkv, nq * g, d)
    lp = lse.reshape(nb, hkv, g, nq).permute(0, 1, 3, 2).reshape(nb * hkv, nq * g)
    return fk._result(op, lp)


def decode_reference(call):
    """the fp64 definition in the kernel's row order (fp8_kvcache_mod_ref.evaluate's closed form at head dim d)"""
    nb, hq, hkv, d = call["B"], call["hq"], call["hkv"], call["d"]
    g = hq // hkv
    R = g * call["nq"]
    qd, kd, vd = (t.double() for t in km.descales(call))
    cap = call["softcap"]
    sinks = None if call["sinks"] is None else call["sinks"].double()
    _qi, hg = fk.row_map(call)
    o = torch.zeros((nb * hkv, R, d), dtype=torch.float64)
    lse = torch.full((nb * hkv, R), NEG_INF, dtype=torch.float64)
    for b, (k8, v8) in enumerate(fk.sequences(call)):
        lk = k8.shape[0]
        vis = km.visible(call, lk)
        for hk in range(hkv):
            u = b * hkv + hk
            snk = None if sinks is None else sinks[hk * g + hg]                                   # (R,)
            if lk == 0:
                if snk is not None:
                    lse[u] = snk
                continue
            q = e4m3_value(fk._q_rows(call, b, hk)).double() * qd[b, hk]
            k = e4m3_value(k8[:, hk]).double() * kd[b, hk]
            v = e4m3_value(v8[:, hk]).double() * vd[b, hk]
            s = (q @ k.T) * call["scale"]
            if cap > 0.0:
                s = cap * torch.tanh(s / cap)
            s = torch.where(vis, s, torch.tensor(NEG_INF, dtype=torch.float64))
            cols = s if snk is None else torch.cat([s, snk[:, None]], dim=-1)
            live = (cols > NEG_INF).any(-1, keepdim=True)
            z = torch.zeros((), dtype=torch.float64)
            p = torch.softmax(torch.where(live, cols, z), -1) * live
            o[u] = p[:, :lk] @ v
            lse[u] = torch.where(live.squeeze(-1), torch.logsumexp(torch.where(live, cols, z), -1), torch.tensor(NEG_INF, dtype=torch.float64))
    return fk._result(o, lse)


def decode_baseline(call, compute=torch.float32, rounding=True):
    """fp8_kvcache_mod_ref.baseline with d in the shapes (the 64-key tile, the splits and the combine do not depend on d)"""
    ct = compute
    f32 = ct == torch.float32
    nb, hkv, d = call["B"], call["hkv"], call["d"]
    g = call["hq"] // hkv
    R = g * call["nq"]
    S = km.num_splits(call)
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    qd, kd, vd = (t.to(ct) for t in km.descales(call))
    if f32:
        c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)
        ln2 = torch.tensor(LN2_F, dtype=torch.float32)
    else:
        c_log2, ln2 = torch.tensor(call["scale"] * LOG2E_F, dtype=ct), torch.tensor(LN2_F, dtype=ct)
    capped = call["softcap"] > 0.0
    if capped:
        cap_k, cap2 = km.cap_constants(call, ct)
    zero, one, ninf = torch.zeros((), dtype=ct), torch.ones((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    _qi, hg = fk.row_map(call)
    o = torch.zeros((nb * hkv, R, d), dtype=ct)
    lse = torch.full((nb * hkv, R), NEG_INF, dtype=ct)
    for b, (k8s, v8s) in enumerate(fk.sequences(call)):
        lk = k8s.shape[0]
        vis_all = km.visible(call, lk)
        for hk in range(hkv):
            u = b * hkv + hk
            f = (c_log2 * qd[b, hk]) * kd[b, hk]
            fe = one if capped else f
            q8 = e4m3_value(fk._q_rows(call, b, hk)).to(ct)
            k8, v8 = e4m3_value(k8s[:, hk]).to(ct), e4m3_value(v8s[:, hk]).to(ct)
            snk_u = None if call["sinks"] is None else call["sinks"].to(ct)[hk * g + hg]
            for rt in range((R + km.ROW_TILE - 1) // km.ROW_TILE):
                r0, r1 = km.ROW_TILE * rt, min(km.ROW_TILE * rt + km.ROW_TILE, R)
                nr = r1 - r0
                po, pl = [], []
                for kbeg, kend in km.split_ranges(call, lk, rt, S):
                    m = torch.full((nr,), NEG_INF, dtype=ct)
                    l_ = torch.zeros((nr,), dtype=ct)
                    acc = torch.zeros((nr, d), dtype=ct)
                    for t0 in range(kbeg, kend, km.KEY_TILE):
                        sl = slice(t0, min(t0 + km.KEY_TILE, kend))
                        n = sl.stop - sl.start
                        sacc = _mfma_f8(q8[r0:r1], k8[sl].T, ct, torch.zeros((nr, n), dtype=ct), rounding)
                        if capped:
                            rr = 1.0 / (torch.exp2(sacc * (f * cap_k)) + 1.0)
                            sacc = _fma(rr, (-2.0 * cap2).expand_as(rr), cap2.expand_as(rr), ct)
                        sacc = torch.where(vis_all[r0:r1, sl], sacc, ninf)
                        mx = sacc.max(-1).values * fe
                        m_new = torch.maximum(m, mx)
                        gw = bool((m_new - m > 8.0).any())          # (first visible key: inf > 8; none yet: nan > 8 is False)
                        m_use = m_new if gw else m
                        m_use = torch.where(m_use > NEG_INF, m_use, zero)
                        alpha = torch.exp2(m - torch.where(m_new > NEG_INF, m_new, zero)) if gw else one.expand(nr)
                        if gw:
                            m = m_new
                        l_ = l_ * alpha
                        acc = acc * alpha.unsqueeze(-1)
                        p = torch.exp2(_fma(sacc, fe.expand(nr, n), -m_use.unsqueeze(-1).expand(nr, n), ct))
                        acc = _mfma_f8(p8(p), v8[sl], ct, acc, rounding, order=_PV_KEY_OF_K)
                        l_ = l_ + p.sum(-1)
                    dead = l_ == 0
                    inv = vd[b, hk] * (1.0 / l_)
                    po.append(torch.where(dead.unsqueeze(-1), zero, acc * inv.unsqueeze(-1)))
                    pl.append(torch.where(dead, ninf, (m + torch.log2(l_)) * ln2))
                if S == 1:
                    o[u, r0:r1], lse[u, r0:r1] = rnd(po[0]), pl[0]
                    continue
                # kv_combine_kernel: weights exp(lse_s - max), partials added in split order, the sink after the sum, one division
                pls = torch.stack(pl, -1)                                                       # (nr, S)
                mm = pls.max(-1).values
                snk = None if snk_u is None else snk_u[r0:r1]
                if snk is not None:
                    mm = torch.maximum(mm, snk)
                mz = torch.where(mm > NEG_INF, mm, zero)
                w = torch.where(pls == NEG_INF, zero, torch.exp(pls - mz.unsqueeze(-1)))
                tot = w.sum(-1)
                if snk is not None:
                    tot = tot + torch.where(snk == NEG_INF, zero, torch.exp(snk - mz))
                acc = torch.zeros((nr, d), dtype=ct)
                for s_i in range(S):
                    acc = acc + w[:, s_i:s_i + 1] * po[s_i]
                live = tot > 0
                inv = torch.where(live, 1.0 / torch.where(live, tot, one), zero)
                o[u, r0:r1] = rnd(acc * inv.unsqueeze(-1))
                lse[u, r0:r1] = torch.where(live, mm + torch.log(torch.where(live, tot, one)), ninf)
    return fk._result(o, lse)
