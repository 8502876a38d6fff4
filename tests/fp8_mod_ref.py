"""A sliding window, a softcap and attention sinks on the fp8 calls (fwd_fp8in_mod_kernel in csrc/fa_fp8_inputs.hip,
fa_fp8_forward_mod / fa_fp8_forward_varlen_mod in csrc/fa_capi.hip) on the CPU (torch):

    TABLE, build_call(i)     the padded cases the issue of §9zc names, each with and without the softcap and the sinks
    reference(call)          the project's fp64 reference: ex_full_ref.full_reference on the dequantised tensors (fp8_inputs_ref.ex_call
                             with window, softcap and sinks filled in)
    evaluate(call, mutant)   the same closed form written out here in fp64, so that a bug can be built into it (MUTANTS); without a
                             mutant it is the reference (tests/test_fp8_mod_cpu.py, 1e-10)
    baseline(call)           the closed form with the kernel's rounding points and nothing else of it
    sequence_calls(v)        the packed / paged case as one padded call per sequence (every sequence has the bits of the padded call)

`call` is fp8_inputs_ref's dict (B, hq, hkv, nq, nk, causal, dtype, scale, q8, k8, v8, the three descales) plus window (left, right),
softcap and sinks (float32 (H_q,) or None).

What the baseline adds to fp8_inputs_ref.baseline, each read from fwd_fp8in_mod_kernel:
  * the band: `lim_lo = qrow + shift - wl`, `lim_hi = min(qrow + shift + wr, nk - 1)`, wr = 0 under causal (fp8in_mod_fill).  The
    kernel's tile range [t_lo, t_hi) and the waves' [tw_lo, tw_hi) leave out only tiles in which every element of the rows
    concerned is masked; such a tile changes nothing (mx = -inf moves no maximum, p = 0), so the baseline walks every tile;
  * the softcap, before the mask: `rr = rcp(exp2(sacc * ck) + 1)`, `sacc = fma(rr, -2 cap2, cap2)` with ck = f * cap_k, cap_k =
    float(2 / softcap), cap2 = float(softcap * log2(e)) (fp8in_mod_fill), and the factor of what follows `fe = 1`;
  * the sink in the epilogue, ex_sink_norm (fa_ex_common.h) on m ln 2 and the half-wave sum l: mp = max(m, snk), a = l > 0 ?
    exp(m - mp) : 0, lp = fma(l, a, exp(snk - mp)), inv = v_descale * (a / lp), lse = mp + log(lp); a head at -inf takes the
    epilogue without sinks."""
import math

import torch

from tests import fp8_inputs_cases as fc
from tests import fp8_inputs_ref as fr
from tests.ex_full_ref import NEG_INF, _fma, _mm, full_reference, round_to
from tests.fp8_ref import LN2_F, LOG2E_F, _PV_KEY_OF_K, _mfma_f8, e4m3_code, e4m3_value

B, HQ, HKV, D = 2, 4, 2, 128
CAP = 15.0
INPUT_GAIN = 3.5          # q and k are 3.5 x unit normal: the scaled scores have a deviation of 12, so the cap of 15 saturates some
# (Nq, Nk), causal, window: the issue's five
TABLE = (
    dict(n=(300, 300), causal=True, window=(70, -1)),      # crosses a 256-row tile and 128-key tiles on both band edges
    dict(n=(130, 400), causal=False, window=(50, 30)),     # Nq != Nk: the band sits bottom-right; tiles skipped on the left
    dict(n=(300, 300), causal=False, window=(-1, 16)),     # a right bound alone
    dict(n=(260, 200), causal=True, window=(40, -1)),      # rows above the diagonal are dead
    dict(n=(130, 257), causal=True, window=(0, -1)),       # one key a row: P's rounding stands in full
)
MUTANTS = ("window_top_left", "left_bound_off_by_one", "right_bound_ignored_under_causal", "sink_per_kv_head", "sink_in_log2_units",
           "sink_once_per_split", "softcap_after_mask_max_only", "sink_capped")


def the_sinks(hq=HQ, seed=11):
    """N(0, 2) with one head at -inf, one at +1e4 and one at -1e4"""
    g = torch.Generator().manual_seed(seed)
    s = 2.0 * torch.randn((hq,), generator=g, dtype=torch.float32)
    s[1], s[2], s[hq - 1] = float("-inf"), 1.0e4, -1.0e4
    return s


def make_call(n, causal, window, softcap, sinks, dtype=torch.bfloat16, batch=B, seed=0):
    nq, nk = n
    g = torch.Generator().manual_seed(4242 + seed)
    q = INPUT_GAIN * torch.randn((batch, HQ, nq, D), generator=g, dtype=torch.float32)
    k = INPUT_GAIN * torch.randn((batch, HKV, nk, D), generator=g, dtype=torch.float32)
    v = torch.randn((batch, HKV, nk, D), generator=g, dtype=torch.float32)
    ds = {name: fc.odd_mantissa(0.05 * 4.0 ** torch.rand((batch, HKV), generator=g, dtype=torch.float32))
          for name in ("q_descale", "k_descale", "v_descale")}
    return dict(B=batch, hq=HQ, hkv=HKV, nq=nq, nk=nk, causal=causal, dtype=dtype, scale=D ** -0.5, layout="bhnd", input="normal",
                q8=fc.quantise(q, ds["q_descale"].repeat_interleave(HQ // HKV, dim=1)), k8=fc.quantise(k, ds["k_descale"]),
                v8=fc.quantise(v, ds["v_descale"]), window=tuple(window), softcap=float(softcap), sinks=sinks, **ds)


def build_call(i, softcap=False, sinks=False, dtype=torch.bfloat16):
    c = TABLE[i]
    return make_call(c["n"], c["causal"], c["window"], CAP if softcap else 0.0, the_sinks() if sinks else None, dtype, seed=i)


def reference(call):
    """Result (o, lse fp64, units (B * H_q, Nq, .)) of ex_full_ref.full_reference on the dequantised tensors"""
    ec = fr.ex_call(call)
    ec.update(window=call["window"], softcap=call["softcap"], sinks=call["sinks"])
    r = full_reference(ec)
    return fr._result(r.o, r.lse)


def band(call, mutant=None):
    """(Nq, Nk) bool: row i at pos = i + Nk - Nq sees key j iff pos - L <= j <= pos + R; causal sets R = 0"""
    nq, nk = call["nq"], call["nk"]
    wl, wr = call["window"]
    if call["causal"]:
        wr = -1 if (mutant == "right_bound_ignored_under_causal" and wl >= 0) else 0
    if mutant == "left_bound_off_by_one" and wl >= 0:
        wl += 1
    pos = torch.arange(nq)[:, None] + (0 if mutant == "window_top_left" else nk - nq)
    j = torch.arange(nk)[None, :]
    vis = torch.ones((nq, nk), dtype=torch.bool)
    if wl >= 0:
        vis = vis & (j >= pos - wl)
    if wr >= 0:
        vis = vis & (j <= pos + wr)
    return vis


def sink_column(call, mutant=None, splits=1):
    """(B * H_q,) fp64 sink logits of the query units, or None"""
    if call["sinks"] is None:
        return None
    s = call["sinks"].double()
    hq, g = call["hq"], call["hq"] // call["hkv"]
    if mutant == "sink_per_kv_head":
        s = s[torch.arange(hq) // g]
    if mutant == "sink_in_log2_units":
        s = s * math.log(2.0)
    if mutant == "sink_once_per_split":
        s = s + math.log(splits)
    if mutant == "sink_capped" and call["softcap"] > 0.0:
        s = call["softcap"] * torch.tanh(s / call["softcap"])
    return s.repeat(call["B"])


def attend(s, v, sink):
    """(o, lse) fp64 of masked logits s (U, Nq, Nk), v (U, Nk, d) and the sink column (U,) or None: rows without a visible key
    give o = 0 and lse = the sink (-inf without one)"""
    cols = s if sink is None else torch.cat([s, sink[:, None, None].expand(s.shape[0], s.shape[1], 1)], dim=-1)
    live = (cols > NEG_INF).any(-1, keepdim=True)
    z = torch.zeros((), dtype=torch.float64)
    p = torch.softmax(torch.where(live, cols, z), -1) * live
    lse = torch.where(live.squeeze(-1), torch.logsumexp(torch.where(live, cols, z), -1), torch.tensor(NEG_INF, dtype=torch.float64))
    return p[..., :s.shape[-1]] @ v, lse


def applies(call, mutant):
    """False where the bug changes nothing of the call"""
    wl, wr = call["window"]
    cap, snk = call["softcap"] > 0.0, call["sinks"] is not None
    return {"window_top_left": call["nq"] != call["nk"] and (wl >= 0 or wr >= 0 or call["causal"]),
            "left_bound_off_by_one": wl >= 0,
            "right_bound_ignored_under_causal": call["causal"] and wl >= 0,
            "sink_per_kv_head": snk and call["hq"] != call["hkv"],
            "sink_in_log2_units": snk,
            "sink_once_per_split": False,                  # (the decode call's: tests/fp8_kvcache_mod_ref.py)
            "softcap_after_mask_max_only": cap,
            "sink_capped": cap and snk}[mutant]


def evaluate(call, mutant=None):
    """The fp64 Result written out; with a mutant, one plausible kernel bug built in (None where it does not apply):
      window_top_left                   the band around pos = i, not i + Nk - Nq
      left_bound_off_by_one             a row also sees key pos - L - 1
      right_bound_ignored_under_causal  with a left bound, the causal flag's right bound of 0 is not applied
      sink_per_kv_head                  query head h takes sinks[h // (H_q / H_kv)]
      sink_in_log2_units                l += exp2(sink - m log2 e): the sink read as if it were in log2 units
      sink_once_per_split               (decode) every split adds the sink
      softcap_after_mask_max_only       the cap applied to the row maximum but not to the elements: exp(s - cap(max)) normalises to
                                        the uncapped softmax, so this is the call without its softcap
      sink_capped                       the sink capped like a score"""
    assert mutant is None or mutant in MUTANTS
    if mutant is not None and not applies(call, mutant):
        return None
    q, k, v = fr.dequantised(call)
    kvi = fr.kv_unit(call)
    s = _mm(q, k[kvi].transpose(1, 2)) * call["scale"]
    cap = call["softcap"]
    if cap > 0.0 and mutant != "softcap_after_mask_max_only":
        s = cap * torch.tanh(s / cap)
    s = torch.where(band(call, mutant), s, torch.tensor(NEG_INF, dtype=torch.float64))
    o, lse = attend(s, v[kvi], sink_column(call, mutant))
    return fr._result(o, lse)


def cap_constants(call, ct):
    """(cap_k, cap2) as fp8in_mod_fill makes them: doubles on the host, rounded once to float"""
    cap = call["softcap"]
    return torch.tensor(2.0 / cap, dtype=ct), torch.tensor(cap * 1.4426950408889634, dtype=ct)


def sink_norm(m_ln, l_, snk, ct):
    """ex_sink_norm (fa_ex_common.h), elementwise: (inv, lse)"""
    mp = torch.maximum(m_ln, snk)
    a = torch.where(l_ > 0, torch.exp(m_ln - mp), torch.zeros((), dtype=ct))
    lp = _fma(l_, a, torch.exp(snk - mp), ct)
    return a / lp, mp + torch.log(lp)


def baseline(call, compute=torch.float32, rounding=True):
    """Result (o, lse in `compute`) of the closed form with the kernel's rounding points (module docstring; the loop is
    fp8_inputs_ref.baseline's).  rounding=False: no rounding of P and o and no truncation in the matrix instruction (with compute =
    float64: the reference again)."""
    ct = compute
    f32 = ct == torch.float32
    nb, hq, nq, nk = call["B"], call["hq"], call["nq"], call["nk"]
    U = nb * hq
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    kvi = fr.kv_unit(call)
    q8 = e4m3_value(call["q8"]).to(ct).reshape(U, nq, 128)
    k8 = e4m3_value(call["k8"]).to(ct).reshape(-1, nk, 128)[kvi]
    v8 = e4m3_value(call["v8"]).to(ct).reshape(-1, nk, 128)[kvi]
    qd, kd, vd = (t.reshape(-1)[kvi].to(ct) for t in fr.descales(call))
    if f32:
        c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)
        ln2 = torch.tensor(LN2_F, dtype=torch.float32)
    else:
        c_log2, ln2 = torch.tensor(call["scale"] * LOG2E_F, dtype=ct), torch.tensor(LN2_F, dtype=ct)
    f = ((c_log2 * qd) * kd)[:, None, None]                                        # (U, 1, 1): one factor per workgroup
    capped = call["softcap"] > 0.0
    if capped:
        cap_k, cap2 = cap_constants(call, ct)
        ck = f * cap_k
        fe = torch.ones_like(f)
    else:
        fe = f
    zero, one, ninf = torch.zeros((), dtype=ct), torch.ones((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    vis_all = band(call)
    snk = None if call["sinks"] is None else call["sinks"].to(ct).repeat(nb)       # (U,)
    o = torch.zeros((U, nq, 128), dtype=ct)
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
        acc = torch.zeros((U, nr, 128), dtype=ct)
        for t0 in range(0, nk, fr.KEY_TILE):
            sl = slice(t0, min(t0 + fr.KEY_TILE, nk))
            if not bool(vis_all[r0:r1, sl].any()):
                continue                                                            # (outside [t_lo, t_hi), or nothing visible: no change)
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
            iv, ls = sink_norm(m * ln2, l_, sk, ct)
            o_t = torch.where(has.unsqueeze(-1), rnd(acc * (vd[:, None] * iv).unsqueeze(-1)), o_t)
            lse_t = torch.where(has, ls, lse_t)
        o[:, r0:r1], lse[:, r0:r1] = o_t, lse_t
    return fr._result(o, lse)


# ---- the packed and the paged form: the issue's lengths.  Every sequence is the padded call on it alone.
SEQ_K = (0, 1, 37, 300, 129)
SEQ_Q = (5, 1, 37, 40, 0)


def varlen_case(causal, window, softcap, sinks, dtype=torch.bfloat16):
    """dict: per sequence the padded call of one batch (None for a sequence without a query or without a key), and the packed
    tensors q8 (total_q, H_q, 128), k8, v8 (total_k, H_kv, 128) uint8, cu_q, cu_k, descales (B, H_kv)"""
    nb = len(SEQ_K)
    calls = []
    for b, (nq, nk) in enumerate(zip(SEQ_Q, SEQ_K)):
        calls.append(make_call((max(nq, 1), max(nk, 1)), causal, window, CAP if softcap else 0.0, the_sinks() if sinks else None, dtype,
                               batch=1, seed=100 + b))
    cut = lambda t, n: t[0, :, :n].transpose(0, 1)   # noqa: E731  (1, H, N, 128) -> (n, H, 128)
    q8 = torch.cat([cut(c["q8"], nq) for c, nq in zip(calls, SEQ_Q)])
    k8 = torch.cat([cut(c["k8"], nk) for c, nk in zip(calls, SEQ_K)])
    v8 = torch.cat([cut(c["v8"], nk) for c, nk in zip(calls, SEQ_K)])
    cu = lambda lens: torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32)   # noqa: E731
    ds = {n: torch.cat([c[n] for c in calls]) for n in ("q_descale", "k_descale", "v_descale")}
    return dict(calls=[c if nq > 0 and nk > 0 else None for c, nq, nk in zip(calls, SEQ_Q, SEQ_K)], B=nb, q8=q8.contiguous(),
                k8=k8.contiguous(), v8=v8.contiguous(), cu_q=cu(SEQ_Q), cu_k=cu(SEQ_K), causal=causal, window=tuple(window),
                softcap=CAP if softcap else 0.0, sinks=the_sinks() if sinks else None, dtype=dtype, scale=D ** -0.5, **ds)


def varlen_expected(v, fn):
    """(o (total_q, H_q, 128), lse (H_q, total_q)) of fn (reference / baseline) on every sequence alone; a sequence without a key
    gives o = 0 and lse = the sink (-inf without one)"""
    tq = int(v["cu_q"][-1])
    o = torch.zeros((tq, HQ, 128), dtype=torch.float64)
    lse = torch.zeros((HQ, tq), dtype=torch.float64)
    for b, c in enumerate(v["calls"]):
        a, z = int(v["cu_q"][b]), int(v["cu_q"][b + 1])
        if z == a:
            continue
        if c is None:
            snk = torch.full((HQ,), NEG_INF, dtype=torch.float64) if v["sinks"] is None else v["sinks"].double()
            lse[:, a:z] = snk[:, None]
            continue
        r = fn(c)
        o[a:z] = r.o.double().transpose(0, 1)
        lse[:, a:z] = r.lse.double()
    return o, lse
