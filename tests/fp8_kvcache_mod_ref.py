"""A sliding window, a softcap and attention sinks on fp8 KV-cache decoding (fp8kv_split_mod_kernel in
csrc/fa_fp8_decode.hip, fa_fp8_forward_kvcache_mod in csrc/fa_capi.hip) on the CPU (torch), on top of tests/fp8_kvcache_ref.py:

    TABLE, build_call(i)     B = 4, H_q = 8, H_kv = 2, capacity 1024, lengths (0, 1, 65, 1000); Nq, the window, num_splits, the layout
                             (contiguous with cache_batch_idx, one index out of range; paged with ps = 16), sinks and softcap vary
    reference(call)          the project's fp64 reference, ex_full_ref.full_reference, on every sequence's dequantised live tokens
    evaluate(call, mutant)   the same closed form written out in fp64 with a bug built in (fp8_mod_ref.MUTANTS)
    baseline(call)           the closed form with the kernel's rounding points and nothing else of it
    num_splits, split_len    the host's split rule with a window (fa_fp8_decode.hip: fp8kv_split_len; fa_capi.hip: fp8_kv_splits_mod)

`call` is fp8_kvcache_ref's dict plus window (left, right), softcap and sinks (float32 (H_q,) or None).  Results are in the kernel's
row order (fp8_kvcache_ref: row = token * G + head in the group).

What the baseline adds to fp8_kvcache_ref.baseline, each read from fp8kv_split_mod_kernel:
  * the tile's keys [lo, hi): `hi = max(0, min(lk, qhi + coff + wr + 1))`, `lo = max(0, qlo + coff - wl) & ~63`, nt tiles from lo,
    `kbeg = lo + t0 * KT`, `kend = min(hi, lo + t1 * KT)`; wr = 0 under causal (launch_fp8_kvcache_mod);
  * the row's band `rlo = qi + coff - wl`, `rhi = min(qi + coff + wr, lk - 1, kend - 1)`;
  * the softcap before the mask, as fwd_fp8in_mod_kernel has it (fp8_mod_ref.baseline), and `fe = 1` after it;
  * S: the rule over split_len, raised to 2 with sinks; the sink joins in kv_combine_kernel<Tag, true> (fa_decode.hip): m =
    max(max_s lse_s, snk), sum = sum_s exp(lse_s - m) + exp(snk - m), once per row."""
import math

import torch

from tests import fp8_kvcache_cases as kc
from tests import fp8_kvcache_ref as fk
from tests.ex_full_ref import NEG_INF, _fma, full_reference, round_to
from tests.fp8_inputs_ref import descales
from tests.fp8_mod_ref import CAP, MUTANTS, cap_constants, the_sinks
from tests.fp8_ref import LN2_F, LOG2E_F, SENTINEL, _PV_KEY_OF_K, _mfma_f8, e4m3_code, e4m3_value

B, HQ, HKV, D = 4, 8, 2, 128
CAPACITY = 1024
LENS = (0, 1, 65, 1000)
ROW_TILE, KEY_TILE = fk.ROW_TILE, fk.KEY_TILE
GAIN = 2.5
# nq, window, causal, num_splits, layout, softcap, sinks: every Nq, L, num_splits and layout of the issue at least twice
TABLE = (
    dict(nq=1, window=(0, -1), causal=True, splits=1, layout="bidx", cap=False, sinks=False),
    dict(nq=3, window=(17, -1), causal=True, splits=3, layout="ps16", cap=False, sinks=False),
    dict(nq=1, window=(128, -1), causal=False, splits=0, layout="bidx", cap=False, sinks=False),
    dict(nq=3, window=(2000, -1), causal=True, splits=1, layout="ps16", cap=False, sinks=False),
    dict(nq=3, window=(17, 1), causal=False, splits=0, layout="ps16", cap=False, sinks=False),
    dict(nq=1, window=(17, -1), causal=True, splits=1, layout="bidx", cap=False, sinks=True),
    dict(nq=3, window=(128, -1), causal=True, splits=3, layout="ps16", cap=False, sinks=True),
    dict(nq=3, window=(128, -1), causal=True, splits=1, layout="bidx", cap=True, sinks=False),
    dict(nq=1, window=(0, -1), causal=True, splits=3, layout="ps16", cap=True, sinks=True),
    dict(nq=3, window=(2000, -1), causal=True, splits=0, layout="bidx", cap=False, sinks=True),
    dict(nq=1, window=(128, -1), causal=True, splits=3, layout="bidx", cap=False, sinks=False),
    dict(nq=3, window=(0, -1), causal=True, splits=0, layout="ps16", cap=True, sinks=True),
)


def case_id(i):
    c = TABLE[i]
    return (f"{i:02d}-nq{c['nq']}-L{c['window'][0]}R{c['window'][1]}-{'causal' if c['causal'] else 'full'}-S{c['splits']}-{c['layout']}"
            f"{'-cap' if c['cap'] else ''}{'-sinks' if c['sinks'] else ''}")


def build_call(i, dtype=torch.bfloat16):
    """the call of TABLE[i] as CPU tensors.  Cache bytes no live token owns are 0x7F (e4m3 NaN); table entries past a sequence's last
    page are garbage; with cache_batch_idx the index of the sequence of 65 keys lies outside the cache (an empty sequence)."""
    c = TABLE[i]
    g = torch.Generator().manual_seed(9001 + 31 * i)
    nq = c["nq"]
    q = GAIN * torch.randn((B, nq, HQ, D), generator=g)
    k = GAIN * torch.randn((B, max(LENS), HKV, D), generator=g)
    v = torch.randn((B, max(LENS), HKV, D), generator=g)
    q8, qd = kc.quantise(q, HKV, "bhkv")
    k8, kd = kc.quantise(k, HKV, "bhkv")
    v8, vd = kc.quantise(v, HKV, "bhkv")
    table, bidx = None, None
    if c["layout"] == "ps16":
        ps = 16
        need = [(n + ps - 1) // ps for n in LENS]
        max_blocks, num_blocks = CAPACITY // ps, sum(need) + 3
        perm = torch.randperm(num_blocks, generator=g).tolist()
        table = torch.randint(-5, num_blocks + 5, (B, max_blocks), generator=g, dtype=torch.int32)
        kcache = torch.full((num_blocks, ps, HKV, D), SENTINEL, dtype=torch.uint8)
        vcache = torch.full((num_blocks, ps, HKV, D), SENTINEL, dtype=torch.uint8)
        for b, n in enumerate(LENS):
            for j in range(need[b]):
                pg = perm.pop()
                table[b, j] = pg
                m = min(ps, n - j * ps)
                kcache[pg, :m], vcache[pg, :m] = k8[b, j * ps:j * ps + m], v8[b, j * ps:j * ps + m]
    else:
        rows = B + 2
        kcache = torch.full((rows, CAPACITY, HKV, D), SENTINEL, dtype=torch.uint8)
        vcache = torch.full((rows, CAPACITY, HKV, D), SENTINEL, dtype=torch.uint8)
        where = [3, 0, 5, 4]
        for b, n in enumerate(LENS):
            kcache[where[b], :n], vcache[where[b], :n] = k8[b, :n], v8[b, :n]
        where[2] = rows + 2                                 # the sequence of 65 keys loses its row: an index out of range
        bidx = torch.tensor(where, dtype=torch.int32)
    return dict(B=B, hq=HQ, hkv=HKV, nq=nq, causal=c["causal"], dtype=dtype, scale=D ** -0.5, num_splits=c["splits"], q8=q8,
                k_cache=kcache, v_cache=vcache, cache_seqlens=torch.tensor(LENS, dtype=torch.int32), block_table=table,
                cache_batch_idx=bidx, q_descale=qd, k_descale=kd, v_descale=vd, values="normal", window=tuple(c["window"]),
                softcap=CAP if c["cap"] else 0.0, sinks=the_sinks(HQ) if c["sinks"] else None)


def bounds(call):
    """(wl, wr) as the kernel takes them: None = unbounded; causal sets the right bound to 0"""
    wl, wr = call["window"]
    return (wl if wl >= 0 else None), (0 if call["causal"] else (wr if wr >= 0 else None))


def split_len(cache_len, nq, causal, window):
    """fp8kv_split_len: what the split rule takes for cache_len"""
    wl, wr = window
    if wl < 0:
        return cache_len
    return min(cache_len, wl + (0 if causal or wr < 0 else wr) + nq)


def num_splits(call):
    """S as fa_capi.hip's fp8_kv_splits_mod sets it"""
    if call["num_splits"] > 0:
        s = call["num_splits"]
    else:
        g = call["hq"] // call["hkv"]
        units = call["B"] * call["hkv"] * ((g * call["nq"] + 31) // 32)
        n = split_len(fk.capacity(call), call["nq"], call["causal"], call["window"])
        s = max(1, min(min((256 * 16 + units - 1) // units, (n + 127) // 128), 256))
    return max(s, 2) if call["sinks"] is not None else s


def split_ranges(call, lk, rt, S=None):
    """[(kbeg, kend)] of the S splits of row tile rt over a sequence of lk keys (fp8kv_split_mod_kernel: `hi`, `lo`, `nt`)"""
    g, nq = call["hq"] // call["hkv"], call["nq"]
    S = num_splits(call) if S is None else S
    wl, wr = bounds(call)
    qlo, qhi = ROW_TILE * rt // g, (min(ROW_TILE * rt + ROW_TILE, g * nq) - 1) // g
    coff = lk - nq
    hi = lk if wr is None else max(0, min(lk, qhi + coff + wr + 1))
    lo = 0 if wl is None else max(0, qlo + coff - wl) // KEY_TILE * KEY_TILE
    nt = (hi - lo + KEY_TILE - 1) // KEY_TILE if hi > lo else 0
    return [(lo + s * nt // S * KEY_TILE, min(hi, lo + (s + 1) * nt // S * KEY_TILE)) for s in range(S)]


def visible(call, lk, mutant=None):
    """(rows, lk) bool: packed row (token i, .) at pos = lk - Nq + i sees key j iff pos - L <= j <= pos + R"""
    qi, _ = fk.row_map(call)
    wl, wr = bounds(call)
    if call["causal"] and mutant == "right_bound_ignored_under_causal" and wl is not None:
        wr = None
    if mutant == "left_bound_off_by_one" and wl is not None:
        wl += 1
    pos = qi[:, None] + (0 if mutant == "window_top_left" else lk - call["nq"])
    j = torch.arange(lk)[None, :]
    vis = torch.ones((qi.numel(), lk), dtype=torch.bool)
    if wl is not None:
        vis = vis & (j >= pos - wl)
    if wr is not None:
        vis = vis & (j <= pos + wr)
    return vis


def reference(call):
    """Result (fp64, the kernel's row order) of ex_full_ref.full_reference on every sequence's dequantised live tokens"""
    nb, hq, hkv, nq = call["B"], call["hq"], call["hkv"], call["nq"]
    g = hq // hkv
    qd, kd, vd = (t.double() for t in descales(call))
    o = torch.zeros((nb, nq, hq, 128), dtype=torch.float64)
    lse = torch.full((nb, hq, nq), NEG_INF, dtype=torch.float64)
    for b, (k8, v8) in enumerate(fk.sequences(call)):
        if k8.shape[0] == 0:
            if call["sinks"] is not None:
                lse[b] = call["sinks"].double()[:, None]
            continue
        q = e4m3_value(call["q8"][b]).double().transpose(0, 1) * qd[b].repeat_interleave(g)[:, None, None]      # (H_q, Nq, 128)
        k = e4m3_value(k8).double().transpose(0, 1) * kd[b][:, None, None]
        v = e4m3_value(v8).double().transpose(0, 1) * vd[b][:, None, None]
        r = full_reference(dict(q=q, k=k, v=v, do=torch.zeros_like(q), dlse=None, sinks=call["sinks"], alibi_slopes=None, layout="padded",
                                heads=(hq, hkv), dropout_p=0.0, seed=0, causal=call["causal"], window=call["window"], mask=None,
                                block_mask=None, br=0, bc=0, softcap=call["softcap"], scale=call["scale"]))
        o[b], lse[b] = r.o.transpose(0, 1), r.lse
    return fk.pack(o, lse, call)


def applies(call, mutant):
    wl, _wr = call["window"]
    cap, snk = call["softcap"] > 0.0, call["sinks"] is not None
    return {"window_top_left": True, "left_bound_off_by_one": wl >= 0, "right_bound_ignored_under_causal": call["causal"] and wl >= 0 and call["nq"] > 1,
            "sink_per_kv_head": snk, "sink_in_log2_units": snk, "sink_once_per_split": snk and num_splits(call) > 1,
            "softcap_after_mask_max_only": cap, "sink_capped": cap and snk}[mutant]


def evaluate(call, mutant=None):
    """The fp64 Result (the kernel's row order) written out; with a mutant of fp8_mod_ref.MUTANTS built in (None: does not apply)"""
    assert mutant is None or mutant in MUTANTS
    if mutant is not None and not applies(call, mutant):
        return None
    nb, hq, hkv = call["B"], call["hq"], call["hkv"]
    g = hq // hkv
    R = g * call["nq"]
    qd, kd, vd = (t.double() for t in descales(call))
    cap = call["softcap"]
    sinks = None
    if call["sinks"] is not None:
        sinks = call["sinks"].double()
        if mutant == "sink_per_kv_head":
            sinks = sinks[torch.arange(hq) // g]
        if mutant == "sink_in_log2_units":
            sinks = sinks * math.log(2.0)
        if mutant == "sink_once_per_split":
            sinks = sinks + math.log(num_splits(call))
        if mutant == "sink_capped":
            sinks = cap * torch.tanh(sinks / cap)
    _qi, hg = fk.row_map(call)
    o = torch.zeros((nb * hkv, R, 128), dtype=torch.float64)
    lse = torch.full((nb * hkv, R), NEG_INF, dtype=torch.float64)
    for b, (k8, v8) in enumerate(fk.sequences(call)):
        lk = k8.shape[0]
        vis = visible(call, lk, mutant)
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
            if cap > 0.0 and mutant != "softcap_after_mask_max_only":
                s = cap * torch.tanh(s / cap)
            s = torch.where(vis, s, torch.tensor(NEG_INF, dtype=torch.float64))
            cols = s if snk is None else torch.cat([s, snk[:, None]], dim=-1)
            live = (cols > NEG_INF).any(-1, keepdim=True)
            z = torch.zeros((), dtype=torch.float64)
            p = torch.softmax(torch.where(live, cols, z), -1) * live
            o[u] = p[:, :lk] @ v
            lse[u] = torch.where(live.squeeze(-1), torch.logsumexp(torch.where(live, cols, z), -1), torch.tensor(NEG_INF, dtype=torch.float64))
    return fk._result(o, lse)


def baseline(call, compute=torch.float32, rounding=True):
    """Result (o, lse in `compute`, the kernel's row order) of the closed form with the kernel's rounding points (module docstring; the
    loop is fp8_kvcache_ref.baseline's).  rounding=False with compute = float64: the reference again."""
    ct = compute
    f32 = ct == torch.float32
    nb, hkv = call["B"], call["hkv"]
    g = call["hq"] // hkv
    R = g * call["nq"]
    S = num_splits(call)
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    qd, kd, vd = (t.to(ct) for t in descales(call))
    if f32:
        c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)
        ln2 = torch.tensor(LN2_F, dtype=torch.float32)
    else:
        c_log2, ln2 = torch.tensor(call["scale"] * LOG2E_F, dtype=ct), torch.tensor(LN2_F, dtype=ct)
    capped = call["softcap"] > 0.0
    if capped:
        cap_k, cap2 = cap_constants(call, ct)
    zero, one, ninf = torch.zeros((), dtype=ct), torch.ones((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    _qi, hg = fk.row_map(call)
    o = torch.zeros((nb * hkv, R, 128), dtype=ct)
    lse = torch.full((nb * hkv, R), NEG_INF, dtype=ct)
    for b, (k8s, v8s) in enumerate(fk.sequences(call)):
        lk = k8s.shape[0]
        vis_all = visible(call, lk)
        for hk in range(hkv):
            u = b * hkv + hk
            f = (c_log2 * qd[b, hk]) * kd[b, hk]
            fe = one if capped else f
            q8 = e4m3_value(fk._q_rows(call, b, hk)).to(ct)
            k8, v8 = e4m3_value(k8s[:, hk]).to(ct), e4m3_value(v8s[:, hk]).to(ct)
            snk_u = None if call["sinks"] is None else call["sinks"].to(ct)[hk * g + hg]
            for rt in range((R + ROW_TILE - 1) // ROW_TILE):
                r0, r1 = ROW_TILE * rt, min(ROW_TILE * rt + ROW_TILE, R)
                nr = r1 - r0
                po, pl = [], []
                for kbeg, kend in split_ranges(call, lk, rt, S):
                    m = torch.full((nr,), NEG_INF, dtype=ct)
                    l_ = torch.zeros((nr,), dtype=ct)
                    acc = torch.zeros((nr, 128), dtype=ct)
                    for t0 in range(kbeg, kend, KEY_TILE):
                        sl = slice(t0, min(t0 + KEY_TILE, kend))
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
                acc = torch.zeros((nr, 128), dtype=ct)
                for s_i in range(S):
                    acc = acc + w[:, s_i:s_i + 1] * po[s_i]
                live = tot > 0
                inv = torch.where(live, 1.0 / torch.where(live, tot, one), zero)
                o[u, r0:r1] = rnd(acc * inv.unsqueeze(-1))
                lse[u, r0:r1] = torch.where(live, mm + torch.log(torch.where(live, tot, one)), ninf)
    return fk._result(o, lse)
