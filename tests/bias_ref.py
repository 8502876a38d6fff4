"""An additive attention bias with its gradient (ex_forward / ex_backward with attn_bias; flash_attention_ex(attn_bias=)) modelled on
the CPU, on top of tests/ex_full_ref.py (imported, not edited):

    bias_reference(call)            fp64, gradients by autograd (dbias too): the reference
    bias_reference(call, mutant=m)  the same with one plausible kernel bug built in (BIAS_MUTANTS)
    bias_baseline(call)             the closed-form flash evaluation with the extended kernels' rounding points (ex_full_ref.baseline's),
                                    plus: the bias added in fp32, dbias = the rounded dS, the broadcast sum in fp32 in unit order with
                                    one more rounding
    project_bar / sharp_bar         ex_full_ref's two bars, extended by the tensor dbias (eps that of the call's dtype)

Semantics, for query unit u = b * H_q + h, row i, key j:  s[i, j] = scale * q_i . k_j + bias[b, h, i, j], the causal flag bottom-right
aligned, a key whose bias is -inf not visible, a row without a visible key o = 0, lse = -inf, dq = 0; dbias = dS = P (dP - delta +
dlse), exactly 0 where the key is not visible, summed over a broadcast batch / head dimension.  With GQA the bias is per query head.

`call`: dict(q (BH, Nq, d), k, v (BH_kv, Nk, d), do, dlse or None, bias (Bb, Hb, Rb, Nk) in the call's dtype, heads=(H_q, H_kv),
causal, scale, dtype); pad: what the padding columns of the bias rows hold (the mutant that reads them needs a value)."""
from collections import namedtuple

import torch

from tests import ex_full_ref as xr
from tests.helpers import dtype_tolerances

NEG_INF = float("-inf")
BIAS_MUTANTS = ("bias_times_scale", "head_is_u_div_hq", "bias_by_kv_head", "block_transposed", "dbias_under_causal", "dbias_from_batch0",
                "padding_read_as_keys")
BiasResult = namedtuple("BiasResult", "o lse dq dk dv dbias dsinks dead_rows dead_keys sink_rows unowned_q unowned_k")


def _units(call):
    hq, hkv = call["heads"]
    bh = call["q"].shape[0]
    u = torch.arange(bh)
    return hq, hkv, bh, (u // hq) * hkv + (u % hq) // (hq // hkv)


def _expand(bias, call, mutant=None):
    """the bias of every query unit, (BH, Nq, Nk): unit u = b * H_q + h reads bias[b or 0, h or 0, i or 0, j]"""
    hq, hkv, bh, _kvi = _units(call)
    nq, nk = call["q"].shape[1], call["k"].shape[1]
    u = torch.arange(bh)
    b, h = u // hq, u % hq
    if mutant == "head_is_u_div_hq":
        h = (u // hq) % hq
    if mutant == "bias_by_kv_head":
        h = h // (hq // hkv)
    bi = b if bias.shape[0] > 1 else torch.zeros_like(b)
    hi = h if bias.shape[1] > 1 else torch.zeros_like(h)
    out = bias[bi, hi].expand(bh, nq, nk)
    if mutant == "block_transposed":       # every whole 32 x 32 block read transposed
        out = out.clone()
        for i0 in range(0, nq - 31, 32):
            for j0 in range(0, nk - 31, 32):
                out[:, i0:i0 + 32, j0:j0 + 32] = out[:, i0:i0 + 32, j0:j0 + 32].transpose(1, 2).clone()
    return out


def _reduce(ds, bias_shape, call, sequential_dtype=None, rnd=None, mutant=None):
    """per-unit dS (BH, Nq, Nk) -> dbias in the bias's shape: the sum over the units that broadcast onto an element, in unit order"""
    hq = call["heads"][0]
    bh, nq, nk = ds.shape
    x = ds.reshape(bh // hq, hq, nq, nk)
    red_b, red_h = bias_shape[0] == 1 and bh // hq > 1, bias_shape[1] == 1 and hq > 1
    assert bias_shape[2] == nq or nq == 1, "no gradient for a row-broadcast bias"
    if not red_b and not red_h:
        return x.reshape(bias_shape)
    if mutant == "dbias_from_batch0" and red_b:
        x = x[:1] * 1.0
        red_b = False
    acc = torch.zeros((1 if red_b else x.shape[0], 1 if red_h else hq, nq, nk), dtype=x.dtype)
    for b in range(x.shape[0]):
        for h in range(hq):
            acc[0 if red_b else b, 0 if red_h else h] += x[b, h]          # unit order, one term at a time in the accumulator's dtype
    return acc if rnd is None else rnd(acc)


def _visible(call, bu):
    nq, nk = call["q"].shape[1], call["k"].shape[1]
    vis = xr._visible(bu.shape[0], nq, nk, call["causal"], (-1, -1), None, None, 0, 0, None)
    return vis & (bu > NEG_INF)


def _sets(call, vis):
    hq, hkv, bh, _kvi = _units(call)
    g = hq // hkv
    dead_rows = ~vis.any(-1)
    seen = vis.any(1).reshape(bh // hq, hkv, g, -1).any(2).reshape(bh // g, -1)
    return dead_rows, ~seen


def bias_reference(call, mutant=None):
    assert mutant is None or mutant in BIAS_MUTANTS
    hq, hkv, bh, kvi = _units(call)
    nq, nk = call["q"].shape[1], call["k"].shape[1]
    qd, kd, vd = (call[n].detach().double().clone().requires_grad_(True) for n in ("q", "k", "v"))
    bias = call["bias"].detach().double()
    bu = _expand(bias, call, mutant).clone().requires_grad_(True)          # the leaf: its gradient is the per-unit dS
    vis = _visible(call, bu.detach())
    b0 = torch.where(torch.isinf(bu), torch.zeros((), dtype=torch.float64), bu)
    qk = qd @ kd[kvi].transpose(1, 2)
    s = (qk + b0) * call["scale"] if mutant == "bias_times_scale" else qk * call["scale"] + b0
    s = torch.where(vis, s, torch.tensor(NEG_INF, dtype=torch.float64))
    vv = vd[kvi]
    if mutant == "padding_read_as_keys" and nk % 8:      # the row's padding joins as keys with k = v = 0 and the padding's value as bias
        extra = torch.full((bh, nq, 8 - nk % 8), float(call.get("pad", 0.0)), dtype=torch.float64)
        s = torch.cat([s, extra], -1)
        vv = torch.cat([vv, torch.zeros((bh, 8 - nk % 8, vv.shape[2]), dtype=torch.float64)], 1)
    live = (s > NEG_INF).any(-1, keepdim=True)
    zero = torch.zeros((), dtype=torch.float64)
    p = torch.softmax(torch.where(live, s, zero), -1) * live
    lse = torch.where(live.squeeze(-1), torch.logsumexp(torch.where(live, s, zero), -1), torch.tensor(NEG_INF, dtype=torch.float64))
    o = p @ vv
    loss = (o * call["do"].double()).sum()
    if call["dlse"] is not None:
        loss = loss + xr.lse_loss(lse, call["dlse"].double())
    loss.backward()
    ds = torch.where(vis, bu.grad, zero)
    if mutant == "dbias_under_causal" and call["causal"]:      # dS stored in front of the mask's select: the call's without the flag
        assert tuple(bias.shape[:2]) == (bh // hq, hq)
        ds = torch.where(vis, ds, bias_reference(dict(call, causal=False)).dbias.reshape(bh, nq, nk))
    dbias = _reduce(ds, tuple(bias.shape), call, mutant=mutant) if bias.shape[2] == nq or nq == 1 else None
    return BiasResult(o.detach(), lse.detach(), qd.grad, kd.grad, vd.grad, dbias, None, *_sets(call, vis), None, None, None)


def bias_baseline(call, compute=torch.float32, tensor_dtype="call"):
    """ex_full_ref.baseline's default model (the extended kernels' rounding points) with the bias: added to the scaled scores in
    `compute`, dbias the dS that was rounded for dS K and dS^T Q, a broadcast dbias their sum in `compute` in unit order, rounded once"""
    ct = compute
    dt = call["dtype"] if tensor_dtype == "call" else tensor_dtype
    rnd = xr.round_to(None if dt is None or dt == ct else dt)
    chunk = 16
    hq, hkv, bh, kvi = _units(call)
    g = hq // hkv
    q, k, v, do = (call[n].to(ct) for n in ("q", "k", "v", "do"))
    nq, nk, scale = q.shape[1], k.shape[1], call["scale"]
    bu = _expand(call["bias"].to(ct), call)                                  # widened exactly
    vis = _visible(call, bu)
    zero = torch.zeros((), dtype=ct)
    kr, vr = k[kvi], v[kvi]
    s = xr._mm(q, kr.transpose(1, 2), chunk) * scale + torch.where(vis, bu, zero)
    s = torch.where(vis, s, torch.tensor(NEG_INF, dtype=ct))
    m = torch.full((bh, nq), NEG_INF, dtype=ct)
    l_ = torch.zeros((bh, nq), dtype=ct)
    acc = torch.zeros((bh, nq, vr.shape[2]), dtype=ct)
    for t0 in range(0, nk, xr.KEY_TILE):
        st = s[..., t0:t0 + xr.KEY_TILE]
        m_new = torch.maximum(m, st.max(-1).values)
        msafe = torch.where(m_new > NEG_INF, m_new, zero)
        alpha = torch.exp(m - msafe)
        pt = torch.exp(st - msafe.unsqueeze(-1))
        l_ = l_ * alpha + pt.sum(-1)
        acc = acc * alpha.unsqueeze(-1) + xr._mm(rnd(pt), vr[:, t0:t0 + xr.KEY_TILE], chunk)
        m = m_new
    live = m > NEG_INF
    l_ = torch.where(live, l_, torch.ones((), dtype=ct))
    lse = torch.where(live, m + torch.log(l_), torch.tensor(NEG_INF, dtype=ct))
    o = rnd(acc * (1.0 / l_).unsqueeze(-1))
    prob = torch.where(live.unsqueeze(-1), torch.exp(s - torch.where(live, lse, zero).unsqueeze(-1)), zero)
    dp = xr._mm(do, vr.transpose(1, 2), chunk)
    c = -xr._delta(do, o)
    if call["dlse"] is not None:
        c = c + torch.where(live, call["dlse"].to(ct), zero)
    c = torch.where(live, c, zero)
    ds = rnd(torch.where(vis, prob * (dp + c.unsqueeze(-1)), zero))
    dq = rnd(scale * xr._mm(ds, kr, chunk))
    dk_u, dv_u = scale * xr._mm(ds.transpose(1, 2), q, chunk), xr._mm(rnd(prob).transpose(1, 2), do, chunk)
    if g > 1:
        dk_u, dv_u = rnd(dk_u), rnd(dv_u)
    dk = rnd(torch.zeros_like(k).index_add_(0, kvi, dk_u))
    dv = rnd(torch.zeros_like(v).index_add_(0, kvi, dv_u))
    shape = tuple(call["bias"].shape)
    dbias = _reduce(ds, shape, call, rnd=rnd) if shape[2] == nq or nq == 1 else None
    return BiasResult(o, lse, dq, dk, dv, dbias, None, None, None, None, None, None)


def rounded(res, dtype):
    r16 = lambda t: None if t is None else t.to(dtype)   # noqa: E731
    return res._replace(o=r16(res.o), dq=r16(res.dq), dk=r16(res.dk), dv=r16(res.dv), dbias=r16(res.dbias), lse=res.lse.float())


# ---- the two bars of ex_full_ref, extended by dbias

def project_bar(got, ref, dtype):
    """ex_full_ref.project_bar, and for dbias: no NaN, within dtype_tolerances of fp64, exactly 0 wherever the reference is (a key
    that is not visible: the causal flag, a dead row, a -inf bias — where a broadcast sum has no visible term at all)"""
    bad = xr.project_bar(got, ref, dtype)
    if ref.dbias is not None:
        tol = dtype_tolerances(dtype)
        a, b = got.dbias.double(), ref.dbias
        if torch.isnan(a).any():
            bad.append("dbias: NaN")
        elif not bool(((a - b).abs() <= tol["atol"] + tol["rtol"] * b.abs()).all()):
            bad.append(f"dbias: max |got - fp64| = {(a - b).abs().max().item():.3e} outside rtol = atol = {tol['atol']:g}")
    return bad


def dbias_zeros(got, call):
    """failures of the exact zeros of dbias: every element none of whose units sees the key"""
    bu = _expand(call["bias"].double(), call)
    vis = _visible(call, bu).double()
    seen = _reduce(vis, tuple(call["bias"].shape), call) > 0
    return [] if not bool((got.dbias[~seen] != 0).any()) else ["dbias != 0 where no unit sees the key"]


def sharp_bar(got, ref, base, dtype):
    """ex_full_ref.sharp_bar over o, lse, dq, dk, dv, and the same inequality for dbias with the call's eps"""
    bad, ratio = xr.sharp_bar(got, ref, base, dtype)
    if ref.dbias is not None:
        err = (got.dbias.double() - ref.dbias).abs().max().item()
        eb = (base.dbias.double() - ref.dbias).abs().max().item()
        big = ref.dbias.abs().max().item()
        eps = torch.finfo(dtype).eps
        bound = 2.0 * eb + eps * big
        ratio["dbias"] = err / eb if eb > 0.0 else (0.0 if err == 0.0 else float("inf"))
        if not err <= bound:
            bad.append(f"dbias: max |got - fp64| = {err:.3e} > 2 * {eb:.3e} (baseline) + {eps:.1e} * {big:.3e} = {bound:.3e}")
    return bad, ratio


def make_call(b, hq, hkv, nq, nk, d, dtype, causal, bias_shape="full", seed=0, with_dlse=False, inf_frac=0.0, dead_rows=0, scale=None):
    """a seeded call: q, k, v, do ~ N(0, 1) in dtype, bias randn * 2 in dtype; bias_shape: "full" or a (Bb, Hb, Rb) triple of 0 / 1
    flags (1 = that dimension is broadcast); inf_frac of the entries -inf, and the first dead_rows rows all -inf"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g).to(dtype)   # noqa: E731
    flags = (0, 0, 0) if bias_shape == "full" else bias_shape
    shape = (1 if flags[0] else b, 1 if flags[1] else hq, 1 if flags[2] else nq, nk)
    bias = (torch.randn(shape, generator=g) * 2).to(dtype)
    if inf_frac > 0.0:
        bias[torch.rand(shape, generator=g) < inf_frac] = NEG_INF
    if dead_rows:
        bias[:, :, :dead_rows] = NEG_INF
    return dict(q=r(b * hq, nq, d), k=r(b * hkv, nk, d), v=r(b * hkv, nk, d), do=r(b * hq, nq, d),
                dlse=torch.randn((b * hq, nq), generator=g) if with_dlse else None, bias=bias, heads=(hq, hkv), causal=bool(causal),
                scale=float(d ** -0.5 if scale is None else scale), dtype=dtype, pad=0.0)
