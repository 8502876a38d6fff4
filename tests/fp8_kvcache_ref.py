"""fp8 KV-cache decoding (csrc/fa_fp8_decode.hip, fa_fp8_forward_kvcache in csrc/fa_capi.hip) on the CPU (torch), for
the table of tests/fp8_kvcache_cases.py:

    sequences(call)          per sequence the live tokens (k8, v8 (len_b, H_kv, 128) codes) behind lengths, table and row index
    reference(call)          fp64 attention per sequence on code * descale, with the GQA rule, the bottom-right diagonal, dead rows
    baseline(call)           the same closed form with the kernel's rounding points and nothing else of it
    mutant(call, name)       the fp64 evaluation with one plausible kernel bug built in (MUTANTS)

`call` is the dict of tests.fp8_kvcache_cases.build_call: B, hq, hkv, nq, causal, dtype (of o), scale, num_splits, q8 (B, Nq, H_q, 128)
uint8 e4m3 codes, k_cache / v_cache uint8 (B_cache, cache_len, H_kv, 128) or pools (num_blocks, ps, H_kv, 128), cache_seqlens (B,)
int32 or None, block_table (B, max_blocks) int32 or None, cache_batch_idx (B,) int32 or None, q_descale / k_descale / v_descale as the
caller passes them.  Results are tests/ex_full_ref.py's Result in the KERNEL'S ROW ORDER: o (B * H_kv, G * Nq, 128) and lse
(B * H_kv, G * Nq) with row = token * G + head in the group, so that a wave's 32-row tile is a slice; unpack() gives the call's layout.
It builds on mla_ref.lengths, kvcache_paged_ref.paged_tokens and fp8_inputs_ref.descales; _mfma_f8, _PV_KEY_OF_K and the e4m3 codecs
are tests/fp8_ref.py's, unchanged (the 32x32x64 instruction's measured sum, §9l-5).

The baseline's rounding points, each read from csrc/fa_fp8_decode.hip (fp8kv_split_kernel unless named otherwise):
  * raw scores: `__builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ka, qb[M], ...)`, two instructions over the 128 head-dim bytes in
    memory order, float32 accumulation — fp8_ref._mfma_f8 with its truncation;
  * P.V on the same instruction with the kernel's key order (`pb[4 * kb + j]`, `vt_off`): fp8_ref._PV_KEY_OF_K;
  * f as float products: `const float f = (p.c_log2 * qd) * kd`, c_log2 = float(softmax_scale) * 1.4426950408889634f
    (launch_fp8_kvcache: `p.c_log2`);
  * the raw-max softmax: the maximum of the RAW scores of a tile times f once (`mx = mx * f`), p = exp2(fma(s, f, -m_use))
    (`__builtin_amdgcn_exp2f(fmaf(sacc[kb][i], f, -m_use))`);
  * the kernel's key tile (`KT = 64`) and lazy rescale per 32-row wave over its real rows
    (`__any(valid && m_new - m_run > 8.0f)`);
  * P to e4m3 by RNE on every row (`__builtin_amdgcn_cvt_pk_fp8_f32`);
  * l from the unrounded p (`rs += pe`);
  * the split ranges (`t0`, `t1`, `kbeg`, `kend`) and fp32 partials normalised by `inv = vd * (1.f / l_tot)` with
    lse = (m + log2 l) * ln 2 (`lse_v`);
  * the combine's order (fa_decode.hip, kv_combine_kernel: weights exp(lse_s - max), partials added in split order, one division);
  * one rounding of o (`pack2_rn`), in the split kernel with one split and in the combine otherwise.
With float64 and no rounding the baseline is the reference again (tests/test_fp8_kvcache_cpu.py, 1e-10)."""
import torch

from tests.ex_full_ref import NEG_INF, Result, _fma, round_to
from tests.fp8_inputs_ref import descales
from tests.fp8_ref import LN2_F, LOG2E_F, _PV_KEY_OF_K, _mfma_f8, e4m3_code, e4m3_value
from tests.kvcache_paged_ref import paged_tokens
from tests.mla_ref import lengths

ROW_TILE = 32
KEY_TILE = 64
MUTANTS = ("causal_top_left", "kv_head_modulo", "tail_keys_dropped", "q_descale_of_batch_0", "v_descale_dropped", "p_truncated",
           "rowsum_from_rounded_p", "page_slot_off_by_one", "split_tile_twice")


def _result(o, lse):
    return Result(o, lse, None, None, None, None, None, None, None, None, None)


def capacity(call):
    if call["block_table"] is not None:
        return call["block_table"].shape[1] * call["k_cache"].shape[1]
    return call["k_cache"].shape[1]


def num_splits(call):
    """S as the C layer sets it: num_splits, or for 0 kv_num_splits (fa_decode.hip) over this kernel's 32-row tiles"""
    if call["num_splits"] > 0:
        return call["num_splits"]
    g = call["hq"] // call["hkv"]
    units = call["B"] * call["hkv"] * ((g * call["nq"] + 31) // 32)
    cap = capacity(call)
    if units <= 0 or cap <= 0:
        return 1
    s = min((256 * 16 + units - 1) // units, (cap + 127) // 128)
    return max(1, min(s, 256))


def workspace_bytes(call):
    """fa_decode.hip, kv_workspace_bytes at d = 128"""
    s = num_splits(call)
    if s <= 1:
        return 0
    rows = call["B"] * call["hq"] * call["nq"] * s
    return ((rows * 128 * 4 + 255) & ~255) + ((rows * 4 + 255) & ~255)


def sequences(call, mutant=None):
    """[(k8, v8)] per sequence: uint8 (len_b, H_kv, 128), len_b = clamp(cache_seqlens[b], 0, capacity); a cache_batch_idx outside the
    cache gives an empty sequence, a page outside the pool zero bytes"""
    B = call["B"]
    lens = lengths(None if call["cache_seqlens"] is None else call["cache_seqlens"].tolist(), B, capacity(call))
    out = []
    for b in range(B):
        n = lens[b]
        if call["block_table"] is not None:
            ps = call["k_cache"].shape[1]
            k, v = (paged_tokens(call[c], call["block_table"][b], n, ps) for c in ("k_cache", "v_cache"))
            if mutant == "page_slot_off_by_one":          # the first slot of every page but the first read from the page before
                for t in range(ps, n, ps):
                    pg = int(call["block_table"][b, t // ps - 1])
                    ok = 0 <= pg < call["k_cache"].shape[0]
                    k[t] = call["k_cache"][pg, 0] if ok else 0
                    v[t] = call["v_cache"][pg, 0] if ok else 0
        else:
            row = b if call["cache_batch_idx"] is None else int(call["cache_batch_idx"][b])
            if not 0 <= row < call["k_cache"].shape[0]:
                n, row = 0, 0
            k, v = call["k_cache"][row, :n], call["v_cache"][row, :n]
        out.append((k, v))
    return out


def row_map(call):
    """(token, head in group) of every packed row: row = token * G + head in the group"""
    g = call["hq"] // call["hkv"]
    rows = torch.arange(g * call["nq"])
    return rows // g, rows % g


def _visible(call, lk, mutant=None):
    """(rows, lk) bool: packed row r = (token i, .) sees key j <= lk - Nq + i under the mask"""
    qi, _ = row_map(call)
    vis = torch.ones((qi.numel(), lk), dtype=torch.bool)
    if call["causal"]:
        c = 0 if mutant == "causal_top_left" else lk - call["nq"]
        vis = torch.arange(lk)[None, :] <= qi[:, None] + c
    if mutant == "tail_keys_dropped" and lk % KEY_TILE:
        vis = vis.clone()
        vis[:, lk - lk % KEY_TILE:] = False
    return vis


def _q_rows(call, b, hk, mutant=None):
    """(rows, 128) uint8: the packed rows of K/V head hk (mutant kv_head_modulo: the query heads h with h % H_kv == hk)"""
    g = call["hq"] // call["hkv"]
    qi, hg = row_map(call)
    heads = hg * call["hkv"] + hk if mutant == "kv_head_modulo" else hk * g + hg
    return call["q8"][b, qi, heads]


def split_ranges(call, lk, rt):
    """[(kbeg, kend)] of the S splits of row tile rt over a sequence of lk keys (fp8kv_split_kernel: `hi`, `nt`, `t0`, `t1`)"""
    g, nq, S = call["hq"] // call["hkv"], call["nq"], num_splits(call)
    qhi = (min(ROW_TILE * rt + ROW_TILE, g * nq) - 1) // g
    hi = max(0, min(lk, qhi + lk - nq + 1)) if call["causal"] else lk
    nt = (hi + KEY_TILE - 1) // KEY_TILE
    return [(s * nt // S * KEY_TILE, min(hi, (s + 1) * nt // S * KEY_TILE)) for s in range(S)]


def _softmax_pv(s, v, mult=None):
    live = (s > NEG_INF).any(-1, keepdim=True)
    mrow = torch.where(live, s.max(-1, keepdim=True).values, torch.zeros((), dtype=torch.float64))
    p = torch.exp(s - mrow)
    if mult is not None:
        p = p * mult
    l_ = p.sum(-1)
    dead = ~live.squeeze(-1)
    o = torch.where(dead.unsqueeze(-1), torch.zeros((), dtype=torch.float64), (p @ v) / l_.clamp_min(1e-300).unsqueeze(-1))
    lse = torch.where(dead, torch.tensor(NEG_INF, dtype=torch.float64), mrow.squeeze(-1) + torch.log(l_.clamp_min(1e-300)))
    return o, lse


def reference(call, mutant=None):
    """Result (o, lse fp64, the kernel's row order) of softmax(scale * (q8 q_descale)(k8 k_descale)^T [causal]) (v8 v_descale) per sequence"""
    B, hkv = call["B"], call["hkv"]
    R = (call["hq"] // hkv) * call["nq"]
    qd, kd, vd = (t.double() for t in descales(call))
    if mutant == "q_descale_of_batch_0":
        qd = qd[:1].expand_as(qd)
    if mutant == "v_descale_dropped":
        vd = torch.ones_like(vd)
    o = torch.zeros((B * hkv, R, 128), dtype=torch.float64)
    lse = torch.full((B * hkv, R), NEG_INF, dtype=torch.float64)
    for b, (k8, v8) in enumerate(sequences(call, mutant)):
        lk = k8.shape[0]
        if lk == 0:
            continue
        vis = _visible(call, lk, mutant)
        for hk in range(hkv):
            q = e4m3_value(_q_rows(call, b, hk, mutant)).double() * qd[b, hk]
            k = e4m3_value(k8[:, hk]).double() * kd[b, hk]
            v = e4m3_value(v8[:, hk]).double() * vd[b, hk]
            s = torch.where(vis, (q @ k.T) * call["scale"], torch.tensor(NEG_INF, dtype=torch.float64))
            u = b * hkv + hk
            if mutant in ("p_truncated", "rowsum_from_rounded_p"):
                live = (s > NEG_INF).any(-1, keepdim=True)
                mrow = torch.where(live, s.max(-1, keepdim=True).values, torch.zeros((), dtype=torch.float64))
                p = torch.exp(s - mrow)
                codes = e4m3_code(p.float())
                pr = e4m3_value(codes).double()
                if mutant == "p_truncated":
                    pr = e4m3_value((codes.to(torch.int16) - (pr > p).to(torch.int16)).clamp_min(0).to(torch.uint8)).double()
                    l_ = p.sum(-1)
                else:
                    l_ = pr.sum(-1)
                dead = ~live.squeeze(-1)
                o[u] = torch.where(dead.unsqueeze(-1), torch.zeros((), dtype=torch.float64), (pr @ v) / l_.clamp_min(1e-300).unsqueeze(-1))
                lse[u] = torch.where(dead, torch.tensor(NEG_INF, dtype=torch.float64), mrow.squeeze(-1) + torch.log(l_.clamp_min(1e-300)))
                continue
            mult = None
            if mutant == "split_tile_twice":               # the first tile of every split but the first also counted by the split before
                mult = torch.ones((s.shape[0], lk), dtype=torch.float64)
                for rt in range((R + ROW_TILE - 1) // ROW_TILE):
                    for kbeg, kend in split_ranges(call, lk, rt)[1:]:
                        if kbeg < kend:
                            mult[ROW_TILE * rt:ROW_TILE * rt + ROW_TILE, kbeg:min(kbeg + KEY_TILE, kend)] = 2.0
            o[u], lse[u] = _softmax_pv(s, v, mult)
    return _result(o, lse)


def unpack(res, call):
    """(o (B, Nq, H_q, 128), lse (B, H_q, Nq)) of a Result in the kernel's row order"""
    B, hkv, nq = call["B"], call["hkv"], call["nq"]
    g = call["hq"] // hkv
    o = res.o.reshape(B, hkv, nq, g, 128).permute(0, 2, 1, 3, 4).reshape(B, nq, call["hq"], 128)
    lse = res.lse.reshape(B, hkv, nq, g).permute(0, 1, 3, 2).reshape(B, call["hq"], nq)
    return o, lse


def pack(o, lse, call):
    """the Result in the kernel's row order of o (B, Nq, H_q, 128), lse (B, H_q, Nq)"""
    B, hkv, nq = call["B"], call["hkv"], call["nq"]
    g = call["hq"] // hkv
    op = o.reshape(B, nq, hkv, g, 128).permute(0, 2, 1, 3, 4).reshape(B * hkv, nq * g, 128)
    lp = lse.reshape(B, hkv, g, nq).permute(0, 1, 3, 2).reshape(B * hkv, nq * g)
    return _result(op, lp)


def baseline(call, compute=torch.float32, rounding=True, trace=None):
    """Result (o, lse in `compute`, the kernel's row order) of the closed form with the kernel's rounding points (module docstring).
    rounding=False: no rounding of P and o and no truncation in the matrix instruction (with compute = float64: the reference
    again).  trace: a list that receives (sequence, K/V head, row tile, split, key tile, moved (rows,) bool: the wave rescaled)."""
    ct = compute
    f32 = ct == torch.float32
    B, hkv = call["B"], call["hkv"]
    R = (call["hq"] // hkv) * call["nq"]
    S = num_splits(call)
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    qd, kd, vd = (t.to(ct) for t in descales(call))
    if f32:
        c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)
        ln2 = torch.tensor(LN2_F, dtype=torch.float32)
    else:
        c_log2, ln2 = torch.tensor(call["scale"] * LOG2E_F, dtype=ct), torch.tensor(LN2_F, dtype=ct)
    zero, one, ninf = torch.zeros((), dtype=ct), torch.ones((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    o = torch.zeros((B * hkv, R, 128), dtype=ct)
    lse = torch.full((B * hkv, R), NEG_INF, dtype=ct)
    for b, (k8s, v8s) in enumerate(sequences(call)):
        lk = k8s.shape[0]
        vis_all = _visible(call, lk)
        for hk in range(hkv):
            u = b * hkv + hk
            f = (c_log2 * qd[b, hk]) * kd[b, hk]
            q8 = e4m3_value(_q_rows(call, b, hk)).to(ct)
            k8, v8 = e4m3_value(k8s[:, hk]).to(ct), e4m3_value(v8s[:, hk]).to(ct)
            for rt in range((R + ROW_TILE - 1) // ROW_TILE):
                r0, r1 = ROW_TILE * rt, min(ROW_TILE * rt + ROW_TILE, R)
                nr = r1 - r0
                po, pl = [], []
                for s_i, (kbeg, kend) in enumerate(split_ranges(call, lk, rt)):
                    m = torch.full((nr,), NEG_INF, dtype=ct)
                    l_ = torch.zeros((nr,), dtype=ct)
                    acc = torch.zeros((nr, 128), dtype=ct)
                    for t0 in range(kbeg, kend, KEY_TILE):
                        sl = slice(t0, min(t0 + KEY_TILE, kend))
                        n = sl.stop - sl.start
                        sacc = _mfma_f8(q8[r0:r1], k8[sl].T, ct, torch.zeros((nr, n), dtype=ct), rounding)
                        sacc = torch.where(vis_all[r0:r1, sl], sacc, ninf)
                        mx = sacc.max(-1).values * f
                        m_new = torch.maximum(m, mx)
                        gw = bool((m_new - m > 8.0).any())          # (first visible key: inf > 8; none yet: nan > 8 is False)
                        if trace is not None:
                            trace.append((b, hk, rt, s_i, t0 // KEY_TILE, gw))
                        m_use = m_new if gw else m
                        m_use = torch.where(m_use > NEG_INF, m_use, zero)
                        alpha = torch.exp2(m - torch.where(m_new > NEG_INF, m_new, zero)) if gw else one.expand(nr)
                        if gw:
                            m = m_new
                        l_ = l_ * alpha
                        acc = acc * alpha.unsqueeze(-1)
                        p = torch.exp2(_fma(sacc, f.expand(nr, n), -m_use.unsqueeze(-1).expand(nr, n), ct))
                        acc = _mfma_f8(p8(p), v8[sl], ct, acc, rounding, order=_PV_KEY_OF_K)
                        l_ = l_ + p.sum(-1)
                    dead = l_ == 0
                    inv = vd[b, hk] * (1.0 / l_)
                    po.append(torch.where(dead.unsqueeze(-1), zero, acc * inv.unsqueeze(-1)))
                    pl.append(torch.where(dead, ninf, (m + torch.log2(l_)) * ln2))
                if S == 1:
                    o[u, r0:r1], lse[u, r0:r1] = rnd(po[0]), pl[0]
                    continue
                # kv_combine_kernel: weights exp(lse_s - max), partials added in split order, one division
                pls = torch.stack(pl, -1)                                                       # (nr, S)
                mm = pls.max(-1).values
                w = torch.where(pls == NEG_INF, zero, torch.exp(pls - torch.where(mm > NEG_INF, mm, zero).unsqueeze(-1)))
                tot = w.sum(-1)
                acc = torch.zeros((nr, 128), dtype=ct)
                for s_i in range(S):
                    acc = acc + w[:, s_i:s_i + 1] * po[s_i]
                live = tot > 0
                inv = torch.where(live, 1.0 / torch.where(live, tot, one), zero)
                o[u, r0:r1] = rnd(acc * inv.unsqueeze(-1))
                lse[u, r0:r1] = torch.where(live, mm + torch.log(torch.where(live, tot, one)), ninf)
    return _result(o, lse)


def rounded(res, dtype):
    """a Result as the kernel returns it: o in dtype, lse float32"""
    return res._replace(o=res.o.to(dtype), lse=res.lse.float())


def tile_bar(got, ref, base, dtype):
    """ex_full_ref.sharp_bar — the same function, the same factor 2 — per 32-row tile of the kernel: (failures, {tensor[tile]: ratio})"""
    from tests.ex_full_ref import sharp_bar
    bad, ratio = [], {}
    cut = lambda r, a, b: _result(r.o[:, a:b], r.lse[:, a:b])   # noqa: E731
    for a in range(0, ref.o.shape[1], ROW_TILE):
        fails, r = sharp_bar(cut(got, a, a + ROW_TILE), cut(ref, a, a + ROW_TILE), cut(base, a, a + ROW_TILE), dtype)
        bad += [f"rows [{a}:{a + ROW_TILE}] {x}" for x in fails]
        ratio.update({f"{k}[{a}]": v for k, v in r.items()})
    return bad, ratio


def mutant(call, name):
    """the fp64 Result with one bug built in, or None where the bug does not apply to the call (it changes nothing):
      causal_top_left          the diagonal aligned top-left: token i sees j <= i
      kv_head_modulo           query head h reads K/V head h % H_kv
      tail_keys_dropped        the last len % 64 keys never visited
      q_descale_of_batch_0     every sequence scored with batch 0's q_descale
      v_descale_dropped        o without v_descale
      p_truncated              p = exp2(s - rowmax) truncated toward zero to e4m3 before P.V
      rowsum_from_rounded_p    l (o's divisor and lse) from the e4m3-rounded p
      page_slot_off_by_one     the first slot of a page (but the sequence's first) read from the page before
      split_tile_twice         the first key tile of a split also counted by the split before it"""
    assert name in MUTANTS
    hq, hkv = call["hq"], call["hkv"]
    lens = [k.shape[0] for k, _v in sequences(call)]
    if name == "causal_top_left" and (not call["causal"] or all(n == call["nq"] or n == 0 for n in lens)):
        return None
    if name == "kv_head_modulo" and (hq == hkv or hkv == 1):
        return None
    if name == "tail_keys_dropped" and all(n % KEY_TILE == 0 for n in lens):
        return None
    if name == "q_descale_of_batch_0" and (call["q_descale"] is None or call["q_descale"].dim() == 1):
        return None
    if name == "v_descale_dropped" and call["v_descale"] is None:
        return None
    if name == "page_slot_off_by_one" and (call["block_table"] is None or all(n <= call["k_cache"].shape[1] for n in lens)):
        return None
    if name == "split_tile_twice":
        R = (hq // hkv) * call["nq"]
        if not any(kb < ke for n in lens for rt in range((R + ROW_TILE - 1) // ROW_TILE) for kb, ke in split_ranges(call, n, rt)[1:]):
            return None
    return reference(call, name)
