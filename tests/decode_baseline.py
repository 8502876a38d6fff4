"""A rounding model of the decode kernels (csrc/fa_decode.hip, fa_decode_kernels.h, fa_mla.hip), for the sharp bar on the decode
sweeps (tests/test_kvcache_sweep_gpu.py, tests/test_mla_routes_gpu.py; proved on the CPU by tests/test_decode_sharp_cpu.py):

    kv_baseline(call, S)                the whole ex_kvcache_forward call at S splits, as a careful kernel of the tensors' dtype
    mla_dense_baseline / mla_list_baseline   the same for the MLA forms (qv; lists of cached tokens)
    ...(compute=float64, tensor_dtype=None)  no rounding anywhere: the fp64 references again (kvcache_full_ref.full_reference,
                                        mla_ref.mla_reference, mla_sparse_ref.mla_sparse_reference)
    ...(mutant=m)                       one plausible decode bug built in (MUTANTS, MLA_MUTANTS)
    sharp_rows                          ex_full_ref.sharp_bar on the rows of a call and of each of its sequences

It holds no kernel code: it is the closed form with the kernels' rounding points, reusing ex_full_ref._mm, _fma and round_to.  The
addressing and the append are kvcache_full_ref.front_half's, shared with the reference.  The points, each with where it was read:

  * inputs as stored; an e4m3 element widens exactly (fa_ex_common.h, kv_q8_widen).  With rotary, q is rotated in fp32 from the
    16-bit values — the products are exact, the sum is rounded to fp32 — and rounded once to 16 bits (fa_decode_kernels.h,
    kv_rotate_chunk and the kKvRot branch of kv_split_kernel's prologue)
  * scores: unscaled products, 32 terms an instruction into an fp32 accumulator (fa_decode_common.h, mfma16:
    v_mfma_f32_16x16x32; kv_split_kernel `sacc[kb] = mfma16(kf[kb][ks], qf[ks], sacc[kb])`).  MLA: the 64 rotary dims, then the
    512 latent dims (fa_mla.hip, mla_tile_step)
  * the modifiers on the unscaled score, in this order (kv_split_kernel, "score modifiers"): times k_descale (e4m3); the softcap
    in reciprocal form, r = 1 / (2^(cap_k s) + 1), s~ = fma(r, -2 cap_a, cap_a) with the float constants cap_k = 2 log2(e) scale /
    softcap and cap_a = softcap / scale (fa_ex_common.h, mod_softcap; fa_decode_common.h, kv_make_params); ALiBi as
    fma(-al, |dist|, s~) with al = slope * (1 / scale) (mod_alibi); then the row's band
  * split ranges from kv_split_range (fa_decode_common.h) per tile of 16 packed rows (row = token * G + head of the group) — MLA
    dense: per workgroup of 16 * mla_waves(rows) rows (fa_mla.hip, MlaDenseKeys); lists: whole tiles of list positions
    (MlaListKeys) — and tiles of 32 keys counted from the split's first key
  * the online softmax per tile in the exp2 domain with the float c_log2 = scale * log2(e) (kv_make_params): m_new = max(m_run,
    tile max), alpha = exp2((m_run - m_use) c_log2), p = exp2(fma(s, c_log2, -(m_use c_log2))), the accumulator and l rescaled by
    alpha at every tile (kv_split_kernel; mla_tile_step)
  * l from the unrounded p: per lane group g the four pair sums of keys 16 kb + 4 g + 2 j + {0, 1} added in turn, then
    (l_0 + l_1) + (l_2 + l_3) (kv_split_kernel's epilogue, mla_epilogue).  MLA takes l * alpha + the first pair sum as one fma
    (mla_tile_step)
  * P rounded to the tensor dtype (fa_common.h, pack2) before P V; P V 32 keys an instruction onto the rescaled accumulator
  * S = 1: o = round(acc * (1 / l) [* v_descale]), lse = m * scale + log(l) in fp32
  * S > 1: fp32 partials acc * (1 / l) [* v_descale] and lse_s; the combine (fa_decode.hip, kv_combine_kernel; fa_mla.hip,
    mla_combine_kernel): m = max_s lse_s, w_s = exp(lse_s - m), their sum by a butterfly over the 64 lanes (xor 32, 16, .. 1),
    acc += w_s O_s in split order, o = round(acc * (1 / sum)), lse = m + log(sum)
  * the sink column joins in the combine only (kv_combine_kernel<Tag, SINK = true>): m = max(m, sink), sum += exp(sink - m) after the
    butterfly.  The C layer raises a sink call's S from 1 to 2 (fa_capi.hip)
  * the number of splits of num_splits = 0: kv_num_splits (fa_decode.hip), mla_split_rule (fa_mla.hip), transcribed below and held
    to the library's workspace-size entry points by tests/test_decode_sharp_cpu.py
Not modelled: the hardware's exp2, log and reciprocal are taken as correctly rounded, and hipcc's choice between a * b + c and
fma where the source leaves it open; both are a few ulp of fp32."""
import math
from types import SimpleNamespace

import torch

from tests import ex_full_ref as fr
from tests.ex_full_ref import LOG2E, _fma, _mm, round_to
from tests.kvcache_full_ref import front_half, place
from tests.kvcache_paged_ref import paged_tokens
from tests.mla_ref import lengths
from tests.test_kvcache_cpu import split_range

NEG_INF = -math.inf
KT = 32

MUTANTS = ("v_from_next_slot", "v_descale_of_next_head", "k_descale_after_softcap", "seam_key_dropped", "tile_counted_from_zero",
           "sink_in_every_split", "combine_weight_from_split0", "o_times_1.02", "lse_plus_2e-4", "tail_head_dims_zero",
           "softmax_scale_as_bf16", "k_descale_as_bf16", "v_descale_as_bf16", "alibi_slope_as_bf16", "lse_partials_as_f16")
MLA_MUTANTS = ("rotary_part_unscaled", "list_tail_dropped", "seam_key_dropped", "combine_weight_from_split0", "o_times_1.02", "lse_plus_2e-4")
TAIL_DIMS = (8, 24, 40, 72, 136, 200)


# ---- the number of splits

def kv_num_splits(batch, heads_kv, row_tiles, cache_len):
    """fa_decode.hip, kv_num_splits: enough one-wave workgroups to fill 256 CUs 16 deep, none shorter than 128 keys, at most 256"""
    units = batch * heads_kv * row_tiles
    if units <= 0 or cache_len <= 0:
        return 1
    s = min((256 * 16 + units - 1) // units, (cache_len + 127) // 128)
    return max(1, min(s, 256))


def mla_waves(rows):
    return 1 if rows <= 16 else 2 if rows <= 32 else 4


def mla_split_rule(lists, heads_kv, rows, keys):
    """fa_mla.hip, mla_split_rule: a unit is a workgroup of mla_waves(rows) waves, 4 / waves of them a CU"""
    if rows <= 0:
        return 1
    nw = mla_waves(rows)
    units = lists * heads_kv * ((rows + 16 * nw - 1) // (16 * nw))
    if units <= 0 or keys <= 0:
        return 1
    s = min((256 * (4 // nw) + units - 1) // units, (keys + 127) // 128)
    return max(1, min(s, 256))


def workspace_bytes(rows, d, splits):
    """fa_decode.hip, kv_workspace_bytes, for rows = batch * heads_q * seqlen_q"""
    if splits <= 1:
        return 0
    r256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    return r256(rows * splits * d * 4) + r256(rows * splits * 4)


def kv_shape(kw):
    """(batch, H_q, H_kv, seqlen_q or max_seqlen_q, capacity, d, total_q or None) of an ex_kvcache_forward call"""
    q, kc = kw["q"], kw["k_cache"]
    packed = kw.get("cu_seqlens_q") is not None
    cap = kw["block_table"].shape[1] * kc.shape[1] if kw.get("block_table") is not None else kc.shape[1]
    bsz = len(kw["cu_seqlens_q"]) - 1 if packed else q.shape[0]
    return bsz, q.shape[-2], kc.shape[2], (kw["max_seqlen_q"] if packed else q.shape[1]), cap, q.shape[-1], (q.shape[0] if packed else None)


def kv_splits(kw):
    """the S an ex_kvcache_forward call runs at (fa_capi.hip, kv_splits, and the sink's 1 -> 2)"""
    bsz, hq, hkv, nq, cap, _d, _tq = kv_shape(kw)
    s = kw.get("num_splits", 0) or kv_num_splits(bsz, hkv, ((hq // hkv) * nq + 15) // 16, cap)
    return max(s, 2) if kw.get("sinks") is not None else s


# ---- the arithmetic the kernels share

def _consts(scale, ct):
    """(scale, c_log2, 1 / scale) as the kernels hold them: floats made from the float scale (kv_make_params) — or exact"""
    if ct != torch.float32:
        return scale, scale * LOG2E, 1.0 / scale
    sc = torch.tensor(scale, dtype=torch.float32)
    return float(sc), float(sc * torch.tensor(1.4426950408889634, dtype=torch.float32)), float(torch.tensor(1.0 / float(sc), dtype=torch.float32))


def _tiles(x, v, kbeg, kend, c2, ct, rnd, l_fma):
    """One split: the online softmax over the 32-key tiles of keys [kbeg, kend), counted from kbeg.  x (U, R, K): the modified,
    masked, unscaled scores; v (U, K, dv).  Returns (acc (U, R, dv), l (U, R), m (U, R))."""
    u, r = x.shape[:2]
    m = torch.full((u, r), NEG_INF, dtype=ct)
    lg = torch.zeros((u, r, 4), dtype=ct)
    acc = torch.zeros((u, r, v.shape[2]), dtype=ct)
    zero = torch.zeros((), dtype=ct)
    for k0 in range(kbeg, kend, KT):
        k1 = min(k0 + KT, kend)
        xt, vt = x[..., k0:k1], v[:, k0:k1]
        if k1 - k0 < KT:      # keys past the split's end: masked, their V rows zeros
            xt = torch.nn.functional.pad(xt, (0, KT - (k1 - k0)), value=NEG_INF)
            vt = torch.nn.functional.pad(vt, (0, 0, 0, KT - (k1 - k0)))
        m_new = torch.maximum(m, xt.max(-1).values)
        m_use = torch.where(m_new > NEG_INF, m_new, zero)
        alpha = torch.exp2((m - m_use) * c2)
        mc = m_use * c2
        p = torch.exp2(_fma(xt, c2, -mc.unsqueeze(-1), ct))
        pairs = p.reshape(u, r, 2, 4, 2, 2).sum(-1)                      # [kb, g, j]: keys 16 kb + 4 g + 2 j + {0, 1}
        al = alpha.unsqueeze(-1)
        lg = _fma(lg, al, pairs[:, :, 0, :, 0], ct) if l_fma else lg * al + pairs[:, :, 0, :, 0]
        lg = ((lg + pairs[:, :, 0, :, 1]) + pairs[:, :, 1, :, 0]) + pairs[:, :, 1, :, 1]
        acc = acc * al + rnd(p) @ vt
        m = m_new
    return acc, (lg[..., 0] + lg[..., 1]) + (lg[..., 2] + lg[..., 3]), m


def _butterfly(w):
    """the sum over dimension 0 (the splits, one a lane) as the combine's wave takes it: xor 32, 16, .. 1"""
    x = torch.cat([w, torch.zeros((64 - w.shape[0],) + tuple(w.shape[1:]), dtype=w.dtype)])
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[lane ^ o]
    return x[0]


def _finish(parts, scale, vds, sink, ct, rnd, mutant):
    """(o, lse) of rows from their splits' (acc, l, m): the direct store of one split, or the partials and the combine.  vds:
    broadcastable to acc[..., 0], or None; sink: broadcastable to l, or None."""
    zero, one = torch.zeros((), dtype=ct), torch.ones((), dtype=ct)
    ninf = torch.tensor(NEG_INF, dtype=ct)
    po, pl = [], []
    for acc, l_, m in parts:
        inv = torch.where(l_ > 0, 1.0 / torch.where(l_ > 0, l_, one), zero)
        ob = acc * inv.unsqueeze(-1)
        if vds is not None:
            ob = ob * vds.unsqueeze(-1)
        po.append(ob)
        pl.append(torch.where(l_ > 0, torch.where(l_ > 0, m, zero) * scale + torch.log(torch.where(l_ > 0, l_, one)), ninf))
    if len(parts) == 1:
        assert sink is None
        return rnd(po[0]), pl[0]
    po, pl = torch.stack(po), torch.stack(pl)
    if mutant == "lse_partials_as_f16":
        pl = pl.half().to(ct)
    if mutant == "sink_in_every_split" and sink is not None:
        new = torch.logaddexp(pl, sink.expand(pl.shape))
        po = po * torch.where(pl > NEG_INF, torch.exp(pl - torch.where(new > NEG_INF, new, zero)), zero).unsqueeze(-1)
        pl = new
    m = pl.max(0).values
    if mutant == "combine_weight_from_split0":
        m = torch.where(pl[0] > NEG_INF, pl[0], m)
    if sink is not None:
        m = torch.maximum(m, sink.expand(m.shape))
    msafe = torch.where(m > NEG_INF, m, zero)
    w = torch.where(pl > NEG_INF, torch.exp(pl - msafe), zero)
    if mutant == "combine_weight_from_split0":
        w = w.clamp(max=1.0)
    tot = _butterfly(w)
    if sink is not None:
        tot = tot + torch.where(sink > NEG_INF, torch.exp(sink - msafe), zero)
    acc = torch.zeros(po.shape[1:], dtype=ct)
    for s in range(po.shape[0]):
        acc = acc + torch.where((w[s] != 0).unsqueeze(-1), w[s].unsqueeze(-1) * po[s], zero)
    inv = torch.where(tot > 0, 1.0 / torch.where(tot > 0, tot, one), zero)
    return rnd(acc * inv.unsqueeze(-1)), torch.where(tot > 0, m + torch.log(torch.where(tot > 0, tot, one)), ninf)


def _split_rows(x, v, ranges, c2, scale, vds, sink, ct, rnd, mutant, l_fma):
    """rows that share their splits' key ranges: x (U, R, K), v (U, K, dv), ranges [(kbeg, kend)] per split"""
    parts = []
    for s, (kbeg, kend) in enumerate(ranges):
        xs = x
        if mutant == "seam_key_dropped" and s >= 1 and kbeg < kend:
            xs = x.clone()
            xs[..., kbeg] = NEG_INF
        if mutant == "tile_counted_from_zero" and kbeg % KT and kbeg < kend:
            kend -= (kend - kbeg) % KT
        parts.append(_tiles(xs, v, kbeg, kend, c2, ct, rnd, l_fma))
    return _finish(parts, scale, vds, sink, ct, rnd, mutant)


def _setup(compute, tensor_dtype, dtype):
    dt = dtype if tensor_dtype == "call" else tensor_dtype
    return compute, round_to(None if dt is None or dt == compute else dt)


def _results(o, lse, dtype, mutant):
    if mutant == "o_times_1.02":
        o = o * 1.02
    if mutant == "lse_plus_2e-4":
        lse = lse + 2e-4
    return o, lse


# ---- ex_kvcache_forward

def kv_baseline(kw, splits=None, compute=torch.float32, tensor_dtype="call", mutant=None, caches_after=None):
    """The call kw (the keywords of ex_kvcache_forward, CPU tensors) at `splits` splits (default: kv_splits(kw)) in dtype
    `compute`, rounded at the points of the module docstring to `tensor_dtype` (default: q's; None: nowhere).  Returns a namespace
    with o, lse in `compute`, in the call's shapes (rows no sequence owns: o = 0, lse = nan)."""
    assert mutant is None or mutant in MUTANTS
    S = kv_splits(kw) if splits is None else max(splits, 2 if kw.get("sinks") is not None else 1)
    call, seqs = front_half(**kw, caches_after=caches_after)
    ct, rnd = _setup(compute, tensor_dtype, call.dtype)
    f32 = ct == torch.float32
    as_bf16 = lambda t: t.bfloat16().to(t.dtype)   # noqa: E731
    scale, c2, inv_scale = _consts(float(as_bf16(torch.tensor(call.scale))) if mutant == "softmax_scale_as_bf16" else call.scale, ct)
    hq, hkv, d = call.hq, call.hkv, call.d
    g = hq // hkv
    cap = call.softcap
    if cap > 0.0:
        cap_k, cap_a = 2.0 * LOG2E * scale / cap, cap / scale
        if f32:
            cap_k, cap_a = float(torch.tensor(cap_k, dtype=torch.float32)), float(torch.tensor(cap_a, dtype=torch.float32))
    wl, wr = call.window
    o = torch.zeros(call.o_shape, dtype=ct)
    lse = torch.full(call.lse_shape, math.nan, dtype=ct)
    sinks = None if call.sinks is None else call.sinks.to(ct)
    for sq in seqs:
        nq, lk = sq.n, sq.k.shape[0]
        rows = g * nq
        qb = sq.q_exact.float().to(call.dtype) if (sq.q_exact is not None and f32) else sq.q
        # (hkv, rows, d): packed row pr = token * G + head of the group
        qr = qb.to(ct).reshape(nq, hkv, g, d).permute(1, 0, 2, 3).reshape(hkv, rows, d)
        kk, vv = sq.k.to(ct).permute(1, 0, 2), sq.v.to(ct).permute(1, 0, 2)           # (hkv, lk, d)
        kds, vds = sq.k_scale.to(ct).view(hkv, 1, 1), sq.v_scale.to(ct).view(hkv, 1)
        if mutant == "v_from_next_slot" and call.paged and lk:
            pos = torch.arange(lk)
            last = pos % call.ps == call.ps - 1
            vv = vv.clone()
            vv[:, pos[last]] = vv[:, pos[last] - (call.ps - 1)]
        if mutant == "v_descale_of_next_head":
            vds = vds.roll(-1, 0)
        if mutant == "k_descale_as_bf16":
            kds = as_bf16(kds)
        if mutant == "v_descale_as_bf16":
            vds = as_bf16(vds)
        x = _mm(qr, kk.transpose(1, 2), KT)
        if call.e4m3 and mutant != "k_descale_after_softcap":
            x = x * kds
        if cap > 0.0:
            r = 1.0 / (torch.exp2(x * cap_k) + 1.0)
            x = _fma(r, -2.0 * cap_a, torch.full((), cap_a, dtype=ct), ct)
        if call.e4m3 and mutant == "k_descale_after_softcap":
            x = x * kds
        qi = (torch.arange(rows) // g).view(rows, 1)
        dist = qi + (lk - nq) - torch.arange(lk).view(1, lk)                          # (rows, lk)
        if sq.slopes is not None:
            sl = (as_bf16(sq.slopes) if mutant == "alibi_slope_as_bf16" else sq.slopes).to(ct).reshape(hkv, 1, g).expand(hkv, nq, g).reshape(hkv, rows, 1)
            x = _fma(-(sl * inv_scale), dist.abs().to(ct).unsqueeze(0), x, ct)
        vis = torch.ones((rows, lk), dtype=torch.bool)
        if call.causal or wr >= 0:
            vis &= dist >= -(0 if call.causal else wr)
        if wl >= 0:
            vis &= dist <= wl
        x = torch.where(vis.unsqueeze(0), x, torch.tensor(NEG_INF, dtype=ct))
        snk = None if sinks is None else sinks.reshape(hkv, 1, g).expand(hkv, nq, g).reshape(hkv, rows)
        ob = torch.zeros((hkv, rows, d), dtype=ct)
        lb = torch.zeros((hkv, rows), dtype=ct)
        # row tiles that share their splits' ranges go together
        groups = {}
        for pr0 in range(0, rows, 16):
            pr1 = min(pr0 + 16, rows)
            rng = tuple(split_range(lk, nq, pr0 // g, (pr1 - 1) // g, call.causal, wl, wr, s, S) for s in range(S))
            groups.setdefault(rng, []).extend(range(pr0, pr1))
        for rng, idx in groups.items():
            ob[:, idx], lb[:, idx] = _split_rows(x[:, idx], vv, rng, c2, scale, vds if call.e4m3 else None,
                                                 None if snk is None else snk[:, idx], ct, rnd, mutant, False)
        ob = ob.reshape(hkv, nq, g, d).permute(1, 0, 2, 3).reshape(nq, hq, d)
        lb = lb.reshape(hkv, nq, g).permute(0, 2, 1).reshape(hq, nq)
        if mutant == "tail_head_dims_zero" and d in TAIL_DIMS:
            ob = ob.clone()
            ob[..., d - d % 16:] = 0
        place(call, sq, o, lse, ob, lb)
    o, lse = _results(o, lse, call.dtype, mutant)
    return SimpleNamespace(o=o, lse=lse, own=call.own, splits=S)


# ---- MLA (fa_mla.hip): q (B, Nq, H_q, 64), qv (B, Nq, H_q, 512), caches (B, cap, H_kv, .) or pools under block_table

def _mla_tokens(k_cache, v_cache, block_table, b, lk):
    ps = k_cache.shape[1]
    if block_table is not None:
        return paged_tokens(k_cache, block_table[b], lk, ps), paged_tokens(v_cache, block_table[b], lk, ps)
    return k_cache[b, :lk], v_cache[b, :lk]


def _mla_scores(q, qv, kt, vt, hkv, scale, ct, mutant):
    """x (hkv, rows, keys) unscaled, rows = token * G + head of the group: the rotary dims, then the latent dims, 32 a run"""
    nq, hq = q.shape[:2]
    g = hq // hkv
    rows = g * nq
    a = torch.cat([q, qv], -1).to(ct)
    if mutant == "rotary_part_unscaled":      # s = q . k + scale * qv . v
        a = torch.cat([q.to(ct) / scale, qv.to(ct)], -1)
    a = a.reshape(nq, hkv, g, -1).permute(1, 0, 2, 3).reshape(hkv, rows, -1)
    kv = torch.cat([kt, vt], -1).to(ct).permute(1, 0, 2)
    return _mm(a, kv.transpose(1, 2), KT)


def mla_dense_baseline(q, qv, k_cache, v_cache, cache_seqlens=None, causal=False, window=(-1, -1), softmax_scale=None, block_table=None,
                       splits=1, compute=torch.float32, tensor_dtype="call", mutant=None):
    """flash_attn_with_kvcache(q, k_cache, v_cache, qv=qv, ..) at `splits` splits: (o (B, Nq, H_q, 512), lse (B, H_q, Nq))"""
    assert mutant is None or mutant in MLA_MUTANTS
    bsz, nq, hq, d = q.shape
    dv, hkv = qv.shape[3], k_cache.shape[2]
    g = hq // hkv
    rows = g * nq
    cap = block_table.shape[1] * k_cache.shape[1] if block_table is not None else k_cache.shape[1]
    ct, rnd = _setup(compute, tensor_dtype, q.dtype)
    scale, c2, _inv = _consts((d + dv) ** -0.5 if softmax_scale is None else float(softmax_scale), ct)
    wl, wr = window
    o = torch.zeros((bsz, nq, hq, dv), dtype=ct)
    lse = torch.full((bsz, hq, nq), NEG_INF, dtype=ct)
    per_wg = 16 * mla_waves(rows)
    for b, lk in enumerate(lengths(cache_seqlens, bsz, cap)):
        kt, vt = _mla_tokens(k_cache, v_cache, block_table, b, lk)
        x = _mla_scores(q[b], qv[b], kt, vt, hkv, scale, ct, mutant)
        dist = (torch.arange(rows) // g).view(rows, 1) + (lk - nq) - torch.arange(lk).view(1, lk)
        vis = torch.ones((rows, lk), dtype=torch.bool)
        if causal or wr >= 0:
            vis &= dist >= -(0 if causal else wr)
        if wl >= 0:
            vis &= dist <= wl
        x = torch.where(vis.unsqueeze(0), x, torch.tensor(NEG_INF, dtype=ct))
        vv = vt.to(ct).permute(1, 0, 2)
        ob, lb = torch.zeros((hkv, rows, dv), dtype=ct), torch.zeros((hkv, rows), dtype=ct)
        for pr0 in range(0, rows, per_wg):
            pr1 = min(pr0 + per_wg, rows)
            rng = [split_range(lk, nq, pr0 // g, (pr1 - 1) // g, causal, wl, wr, s, splits) for s in range(splits)]
            ob[:, pr0:pr1], lb[:, pr0:pr1] = _split_rows(x[:, pr0:pr1], vv, rng, c2, scale, None, None, ct, rnd, mutant, True)
        o[b] = ob.reshape(hkv, nq, g, dv).permute(1, 0, 2, 3).reshape(nq, hq, dv)
        lse[b] = lb.reshape(hkv, nq, g).permute(0, 2, 1).reshape(hq, nq)
    return _results(o, lse, q.dtype, mutant)


def mla_list_baseline(q, qv, k_cache, v_cache, indices, cache_seqlens=None, causal=False, softmax_scale=None, block_table=None,
                      splits=1, compute=torch.float32, tensor_dtype="call", mutant=None):
    """flash_mla_sparse_attn(q, qv, k_cache, v_cache, indices, ..) at `splits` splits.  The keys of a tile are 32 list entries in
    list order; an entry that is -1, at or past the length or (causal) past the row's bound is masked, its row zeros."""
    assert mutant is None or mutant in MLA_MUTANTS
    bsz, nq, hq, d = q.shape
    dv, hkv = qv.shape[3], k_cache.shape[2]
    g = hq // hkv
    cap = block_table.shape[1] * k_cache.shape[1] if block_table is not None else k_cache.shape[1]
    ct, rnd = _setup(compute, tensor_dtype, q.dtype)
    scale, c2, _inv = _consts((d + dv) ** -0.5 if softmax_scale is None else float(softmax_scale), ct)
    if indices.dim() == 3:
        indices = indices.unsqueeze(2).expand(-1, -1, hkv, -1)
    topk = indices.shape[-1]
    nt = (topk + KT - 1) // KT
    rng = [(s * nt // splits * KT, min(topk, (s + 1) * nt // splits * KT)) for s in range(splits)]
    o = torch.zeros((bsz, nq, hq, dv), dtype=ct)
    lse = torch.full((bsz, hq, nq), NEG_INF, dtype=ct)
    for b, lk in enumerate(lengths(cache_seqlens, bsz, cap)):
        if lk == 0:      # no entry is visible: o = 0, lse = -inf
            continue
        kt, vt = _mla_tokens(k_cache, v_cache, block_table, b, lk)
        for i in range(nq):
            bound = lk - nq + i if causal else lk - 1
            for hk in range(hkv):
                ent = indices[b, i, hk].long()
                vis = (ent >= 0) & (ent < lk) & (ent <= bound)
                if mutant == "list_tail_dropped" and topk % KT:
                    vis[topk - topk % KT:] = False
                at = torch.where(vis, ent, torch.zeros_like(ent))
                kl = torch.where(vis.view(-1, 1), kt[at, hk], torch.zeros((), dtype=kt.dtype)).unsqueeze(1)      # (topk, 1, 64)
                vl = torch.where(vis.view(-1, 1), vt[at, hk], torch.zeros((), dtype=vt.dtype)).unsqueeze(1)
                hs = slice(hk * g, (hk + 1) * g)
                x = _mla_scores(q[b, i:i + 1, hs], qv[b, i:i + 1, hs], kl, vl, 1, scale, ct, mutant)               # (1, G, topk)
                x = torch.where(vis.view(1, 1, -1), x, torch.tensor(NEG_INF, dtype=ct))
                ob, lb = _split_rows(x, vl.to(ct).permute(1, 0, 2), rng, c2, scale, None, None, ct, rnd, mutant, True)
                o[b, i, hs], lse[b, hs, i] = ob[0], lb[0]
    return _results(o, lse, q.dtype, mutant)


# ---- the sharp bar on a decode call's rows

def _rows(o, lse, sel):
    """o (.., H_q, d) and lse as a Result of the rows `sel` picks: (o[sel], lse[sel])"""
    return fr.Result(sel(o, False), sel(lse, True), None, None, None, None, None, None, None, None, None)


def sharp_rows(o, lse, ref_o, ref_lse, base_o, base_lse, dtype, groups):
    """ex_full_ref.sharp_bar — its inequality, its factor 2, eps of the tensor dtype for o and of float32 for lse — on every
    group of rows: groups = [(name, sel)] with sel(tensor, is_lse) cutting o or lse to the group's rows.  Returns (failures,
    {name: {tensor: kernel error / baseline error}}, the largest share of a bound that was used)."""
    bad, ratios, used = [], {}, 0.0
    for name, sel in groups:
        got, ref, base = _rows(o, lse, sel), _rows(ref_o, ref_lse, sel), _rows(base_o, base_lse, sel)
        fails, ratio = fr.sharp_bar(got, ref, base, dtype)
        bad += [f"[{name}] {f}" for f in fails]
        ratios[name] = ratio
        eg, eb = fr.errors(got, ref), fr.errors(base, ref)
        for t, (err, big) in eg.items():
            bound = 2.0 * eb[t][0] + torch.finfo(torch.float32 if t == "lse" else dtype).eps * big
            used = max(used, err / bound if bound > 0.0 else (0.0 if err == 0.0 else math.inf))
    return bad, ratios, used


def mla_groups(lens):
    """the row groups of an MLA call on sequences of these lengths ((B, Nq, H_q, 512) and (B, H_q, Nq) results): the call, and each
    sequence with keys alone"""
    return [("call", lambda t, is_lse: t)] + [(f"seq{b}", lambda t, is_lse, b=b: t[b]) for b, n in enumerate(lens) if n > 0]


def kv_groups(r):
    """the row groups of an ex_kvcache_forward call for sharp_rows, from its full_reference r: the call's owned rows, and each
    sequence's rows alone — a case holds lengths 0, 1, 33, 100 and full side by side, and the short rows, where |o| ~ |v|, would
    otherwise set the maximum for the long ones.  A sequence without a visible key in any row is left to the exact rules."""
    packed = r.lse.dim() == 2
    groups = [("call", (lambda t, is_lse: t[:, r.own] if is_lse else t[r.own]) if packed else (lambda t, is_lse: t))]
    for b, n in enumerate(r.nq):
        if n == 0:
            continue
        rows = slice(r.q_first[b], r.q_first[b] + n) if packed else b
        if bool(r.novis[rows].all()):
            continue
        groups.append((f"seq{b}", (lambda t, is_lse, rows=rows: t[:, rows] if is_lse else t[rows]) if packed else
                       (lambda t, is_lse, rows=rows: t[rows])))
    return groups
