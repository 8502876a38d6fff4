"""The whole of one ex_kvcache_forward call, once, in fp64 on the CPU: full_reference takes the call's arguments as CPU tensors
(an e4m3 cache as torch.float8_e4m3fn) and models, in this order, the packed-tensor clamp, the length clamps, the choice of the
cache row or page, the append (rotated, rounded to the 16-bit dtype, quantised), the keys as the reference itself appended
them (dequantised), the rotated queries, the scores (GQA, scale, softcap, ALiBi, the causal / window band aligned bottom-right)
and the softmax with the sink column.  ALiBi goes with sinks.  It never imports the extension.

Everything up to the rotated queries is addressing, not arithmetic, and lives in front_half, which tests/decode_baseline.py (the
rounding model of the decode kernels) shares: per sequence it hands out the rotated q, the keys and values as they lie in the
cache, the scales, slopes and mask parameters.  Both take caches_after: the caches some call left behind, to attend over instead
of the ones appended here.  full_reference is dense_attention on front_half's sequences.

The parts are the ones the feature tests use: kvcache_varlen_ref.cu_range, kvcache_rotary_ref.rotate64 / round_once / slot_of,
kvcache_fp8_ref.quantize / dequantize, kvcache_paged_ref.paged_tokens.  tests/test_kvcache_sweep_cpu.py holds this module to
each of the single-feature references on every case they can express."""
import math
from types import SimpleNamespace

import torch

from tests.kvcache_fp8_ref import E4M3, quantize
from tests.kvcache_paged_ref import paged_tokens
from tests.kvcache_rotary_ref import rotate64, round_once, slot_of
from tests.kvcache_varlen_ref import cu_range

NEG_INF = -math.inf


def dense_attention(qd, kd, vd, causal, window, scale, softcap=0.0, slopes=None, sinks=None):
    """(o (nq, H_q, d), lse (H_q, nq), novis (nq,)) of one sequence, fp64 and bool (the rows without a visible key): qd
    (nq, H_q, d), kd, vd (lk, H_kv, d) fp64, slopes (H_q,) or None, sinks (H_q,) or None.  Row i sees key j inside
    [i + lk - nq - wl, i + lk - nq + wr] (causal: wr = 0); a row without a visible key gives o = 0 and lse = its sink (-inf
    without one)."""
    nq, hq, d = qd.shape
    lk = kd.shape[0]
    o = torch.zeros((nq, hq, d), dtype=torch.float64)
    snk = None if sinks is None else sinks.double().view(hq, 1)
    if lk == 0:
        return o, (snk.expand(hq, nq).clone() if snk is not None else torch.full((hq, nq), NEG_INF, dtype=torch.float64)), \
            torch.ones((nq,), dtype=torch.bool)
    g = hq // kd.shape[1]
    qq = qd.permute(1, 0, 2)                                       # (H_q, nq, d)
    kk = kd.permute(1, 0, 2).repeat_interleave(g, 0)               # (H_q, lk, d): query head h reads K/V head h // G
    vv = vd.permute(1, 0, 2).repeat_interleave(g, 0)
    s = scale * (qq @ kk.transpose(1, 2))
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    diag = torch.arange(nq).view(-1, 1) + (lk - nq)
    j = torch.arange(lk).view(1, -1)
    if slopes is not None:
        s = s - slopes.double().view(hq, 1, 1) * (diag - j).abs().double()
    wl, wr = window
    vis = torch.ones((nq, lk), dtype=torch.bool)
    if causal:
        vis &= j <= diag
    if wl >= 0:
        vis &= j >= diag - wl
    if wr >= 0:
        vis &= j <= diag + wr
    s = s.masked_fill(~vis, NEG_INF)
    if snk is not None:
        s = torch.cat([s, snk.view(hq, 1, 1).expand(hq, nq, 1)], dim=-1)     # the sink column: never capped, biased or masked
    m = s.max(-1, keepdim=True).values
    live = m > NEG_INF
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m))) * live
    tot = e.sum(-1, keepdim=True)
    lse = torch.where(live, m + torch.log(torch.where(live, tot, torch.ones_like(tot))), torch.full_like(m, NEG_INF)).squeeze(-1)
    p = (e / torch.where(live, tot, torch.ones_like(tot)))[..., :lk]         # the sink's value vector is zero
    return (p @ vv).permute(1, 0, 2), lse, ~vis.any(-1)


def front_half(q, k_cache, v_cache, k_new=None, v_new=None, cache_seqlens=None, causal=False, softmax_scale=None,
               window=(-1, -1), softcap=0.0, alibi_slopes=None, num_splits=0, block_table=None, cache_batch_idx=None,
               cache_leftpad=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, *, cu_seqlens_q=None,
               cu_seqlens_k_new=None, max_seqlen_q=None, sinks=None, k_descale=None, v_descale=None, caches_after=None):
    """Everything of a call that is addressing and not arithmetic, shared by full_reference and tests/decode_baseline.py: the
    packed-tensor clamp, the length clamps, the cache row or pages, the append and, per sequence with query tokens, what its
    attention reads.  caches_after = (k_cache, v_cache) as some call left them (the caches' shape and dtype): the sequences'
    keys and values are then read from those instead of from the caches this function appended to itself.
    Returns (call, seqs).  call: a namespace of the per-call fields full_reference returns (all but o, lse, novis) and of packed,
    bsz, hq, hkv, d, ps (tokens a page or cache row), paged, e4m3, dtype, scale, causal, window, softcap, sinks, o_shape,
    lse_shape.  seqs: one namespace per sequence with query tokens:
      b, start, n   the sequence, its first query token (packed) and its query tokens
      q             (n, H_q, d) in the tensor dtype, rotated and rounded once when rotary is on
      q_exact       the fp64 rotation before its rounding (None without rotary)
      k, v          (lk, H_kv, d) as they lie in the cache: the 16-bit dtype, or e4m3 codes as torch.float8_e4m3fn
      k_scale, v_scale   (H_kv,) float32 (ones for a 16-bit cache)
      slopes        (H_q,) or None"""
    packed = cu_seqlens_q is not None
    dtype = q.dtype
    hq, d = q.shape[-2], q.shape[-1]
    hkv, ps = k_cache.shape[2], k_cache.shape[1]
    cap = block_table.shape[1] * ps if block_table is not None else ps
    e4m3 = k_cache.dtype == E4M3
    scale = d ** -0.5 if softmax_scale is None else float(softmax_scale)
    rotary = rotary_cos is not None
    per_token = bool(causal) or window[0] >= 0 or window[1] >= 0
    # ---- packed tensors: every sequence's tokens, clamped as the device clamps them
    if packed:
        bsz, total_q = len(cu_seqlens_q) - 1, q.shape[0]
        q_rng = [cu_range(cu_seqlens_q, b, total_q, max_seqlen_q) for b in range(bsz)]
        o_shape, lse_shape = (total_q, hq, d), (hq, total_q)
        own = torch.zeros((total_q,), dtype=torch.bool)
    else:
        bsz, nq_all = q.shape[0], q.shape[1]
        q_rng = [(0, nq_all)] * bsz
        o_shape, lse_shape = (bsz, nq_all, hq, d), (bsz, hq, nq_all)
        own = torch.ones((bsz, nq_all), dtype=torch.bool)
    if cu_seqlens_k_new is not None:
        kn_rng = [cu_range(cu_seqlens_k_new, b, k_new.shape[0], cap) for b in range(bsz)]
        new_of = lambda t, b: t[kn_rng[b][0]:kn_rng[b][0] + kn_rng[b][1]]   # noqa: E731
    elif k_new is not None:
        kn_rng = [(0, k_new.shape[1])] * bsz
        new_of = lambda t, b: t[b]   # noqa: E731
    else:
        kn_rng = [(0, 0)] * bsz
        new_of = lambda t, b: torch.zeros((0, hkv, d), dtype=dtype)   # noqa: E731
    nq, nnew = [n for _, n in q_rng], [n for _, n in kn_rng]
    # ---- lengths
    if cache_seqlens is None:
        raw = [cap] * bsz
    elif isinstance(cache_seqlens, int):
        raw = [cache_seqlens] * bsz
    else:
        raw = [int(x) for x in cache_seqlens]
    L = [min(max(raw[b], 0), cap - nnew[b]) for b in range(bsz)]
    P = [min(max(int(cache_leftpad[b]), 0), L[b]) if cache_leftpad is not None else 0 for b in range(bsz)]

    def scale_row(ds, b):   # (H_kv,) float32: the scales of sequence b; None = 1.0
        if ds is None:
            return torch.ones((hkv,), dtype=torch.float32)
        return ds if ds.dim() == 1 else ds[b]

    # ---- the append
    as_bits = (lambda t: t.view(torch.uint8)) if e4m3 else (lambda t: t)   # noqa: E731
    ek, ev = as_bits(k_cache.clone()), as_bits(v_cache.clone())
    k_mask, v_mask = torch.zeros(ek.shape, dtype=torch.bool), torch.zeros(ev.shape, dtype=torch.bool)
    slots, k_exact, k_new16, v_new16 = [], [], [], []
    for b in range(bsz):
        kb, vb = new_of(k_new, b), new_of(v_new, b)
        first = L[b] - P[b]
        ex = rotate64(kb, rotary_cos, rotary_sin, [first + n for n in range(nnew[b])], rotary_interleaved) if rotary and nnew[b] else kb.double()
        k16 = round_once(ex, dtype) if rotary else kb
        k_exact.append(ex)
        k_new16.append(k16)
        v_new16.append(vb)
        if nnew[b] == 0:
            continue
        ks, vs = k16, vb
        if e4m3:
            ks = quantize(k16.unsqueeze(0), scale_row(k_descale, b))[0]
            vs = quantize(vb.unsqueeze(0), scale_row(v_descale, b))[0]
        for n in range(nnew[b]):
            unit, pos = slot_of(b, L[b] + n, block_table, cache_batch_idx, ps)
            if 0 <= unit < ek.shape[0]:
                ek[unit, pos], ev[unit, pos] = ks[n], vs[n]
                k_mask[unit, pos] = v_mask[unit, pos] = True
                slots.append((b, n, unit, pos))
    out_bits = (lambda t: t.view(E4M3)) if e4m3 else (lambda t: t)   # noqa: E731
    # ---- per sequence: the keys as they now lie in the caches (or in the caches some call left behind)
    rk, rv = (ek, ev) if caches_after is None else (as_bits(caches_after[0]), as_bits(caches_after[1]))
    assert rk.shape == ek.shape and rv.shape == ev.shape and rk.dtype == ek.dtype
    seqs = []
    for b in range(bsz):
        start, n = q_rng[b]
        if n == 0:
            continue
        lk = L[b] + nnew[b]
        if block_table is not None:
            kt, vt = paged_tokens(rk, block_table[b], lk, ps), paged_tokens(rv, block_table[b], lk, ps)
        else:
            row = int(cache_batch_idx[b]) if cache_batch_idx is not None else b
            if 0 <= row < rk.shape[0]:
                kt, vt = rk[row, P[b]:lk], rv[row, P[b]:lk]
            else:   # a row outside the cache reads as zeros
                kt, vt = torch.zeros((lk - P[b], hkv, d), dtype=rk.dtype), torch.zeros((lk - P[b], hkv, d), dtype=rv.dtype)
        qb = q[start:start + n] if packed else q[b]
        q_exact = None
        if rotary:
            first = L[b] - P[b]
            q_exact = rotate64(qb, rotary_cos, rotary_sin, [first + (i if per_token else 0) for i in range(n)], rotary_interleaved)
            qb = round_once(q_exact, dtype)
        sl = None if alibi_slopes is None else (alibi_slopes[b] if alibi_slopes.dim() == 2 else alibi_slopes)
        own_b = slice(start, start + n) if packed else b
        if packed:
            own[start:start + n] = True
        seqs.append(SimpleNamespace(b=b, start=start, n=n, rows=own_b, q=qb, q_exact=q_exact, k=out_bits(kt), v=out_bits(vt),
                                    k_scale=scale_row(k_descale, b) if e4m3 else torch.ones((hkv,), dtype=torch.float32),
                                    v_scale=scale_row(v_descale, b) if e4m3 else torch.ones((hkv,), dtype=torch.float32), slopes=sl))
    call = SimpleNamespace(own=own, k_cache=out_bits(ek), v_cache=out_bits(ev), k_mask=k_mask, v_mask=v_mask, slots=slots, k_exact=k_exact,
                           k_new16=k_new16, v_new16=v_new16, L=L, P=P, nq=nq, nnew=nnew, q_first=[a for a, _ in q_rng], packed=packed, bsz=bsz, hq=hq, hkv=hkv, d=d, ps=ps,
                           paged=block_table is not None, e4m3=e4m3, dtype=dtype, scale=scale, causal=bool(causal), window=tuple(window),
                           softcap=float(softcap), sinks=sinks, o_shape=o_shape, lse_shape=lse_shape)
    return call, seqs


def place(call, sq, o, lse, ob, lb):
    """sequence sq's (n, H_q, d) rows ob and (H_q, n) rows lb into the call's o and lse"""
    if call.packed:
        o[sq.start:sq.start + sq.n], lse[:, sq.start:sq.start + sq.n] = ob, lb
    else:
        o[sq.b], lse[sq.b] = ob, lb


def full_reference(*args, **kwargs):
    """The arguments of ex_kvcache_forward (num_splits changes nothing that is defined) and caches_after (front_half).  Returns a
    namespace of
      o, lse        fp64, in the call's shapes; rows that no sequence owns: o = 0, lse = nan
      own           bool (total_q,) (packed) or (B, Nq): the tokens some sequence owns
      novis         bool, own's shape: the owned tokens whose rows see no key (o = 0 exactly, lse = the sink or -inf)
      k_cache, v_cache   the caches after the call, in the caches' dtype
      k_mask, v_mask     bool, the caches' shape: the elements the call may write
      slots         [(b, n, unit, pos)]: new key n of sequence b landed at cache[unit, pos]
      k_exact       per sequence the fp64 (nnew_b, H_kv, d) value of its new keys before any rounding (rotated when rotary is on)
      k_new16, v_new16   per sequence the 16-bit values that are stored or quantised (K: rotated and rounded once)
      L, P, nq, nnew     per sequence: the clamped length and left pad, its query tokens, its new keys
    and of front_half's other per-call fields."""
    call, seqs = front_half(*args, **kwargs)
    o = torch.zeros(call.o_shape, dtype=torch.float64)
    lse = torch.full(call.lse_shape, math.nan, dtype=torch.float64)
    novis = torch.zeros(call.own.shape, dtype=torch.bool)
    for sq in seqs:
        kd = sq.k.double() * sq.k_scale.double().view(1, call.hkv, 1) if call.e4m3 else sq.k.double()
        vd = sq.v.double() * sq.v_scale.double().view(1, call.hkv, 1) if call.e4m3 else sq.v.double()
        ob, lb, nv = dense_attention(sq.q.double(), kd, vd, call.causal, call.window, call.scale, call.softcap, sq.slopes, call.sinks)
        place(call, sq, o, lse, ob, lb)
        novis[sq.rows] = nv
    call.o, call.lse, call.novis = o, lse, novis
    return call
