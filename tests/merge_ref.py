"""fp64 torch references for the differentiable lse and the merge of partial attention results (fa_ex_backward_dlse,
fa_merge_states, include/fa_mi355x.h), CPU only.  tests/test_merge_states_cpu.py checks them against torch.autograd and against
each other; tests/test_merge_states_gpu.py and tests/test_dlse_gpu.py hold the kernels to them.

    attention(...)            dense attention with mask, window, sinks and GQA returning (o, lse), differentiable (tests/sink_ref.py)
    attention_grads(...)      o, lse and the gradients of a loss sum(o * do) + sum(lse * dlse) by autograd
    closed_form_backward(...) the same gradients from dS = P * (dP - delta + dlse), no autograd
    merge(...)                the merge, differentiable
    merge_backward(...)       its closed-form backward
    varlen_attention(...)     packed sequences, sequence by sequence
"""
import torch

from tests.sink_ref import sink_attention, unit_sinks, window_visible

NEG_INF = float("-inf")

attention = sink_attention


def _f64(t):
    return None if t is None else t.detach().cpu().double()


def lse_loss(lse, dlse):
    """sum(lse * dlse) over the rows with a finite lse: rows at -inf take no part, whatever their dlse holds (NaN included)"""
    fin = torch.isfinite(lse)
    return (torch.where(fin, lse, torch.zeros_like(lse)) * torch.where(fin, dlse, torch.zeros_like(dlse))).sum()


def attention_grads(q, k, v, do, dlse, sinks, causal, scale, **kw):
    """(o, lse, dq, dk, dv, dsinks) in fp64 of the loss sum(o * do) + sum(lse * dlse); do or dlse may be None (zero); dsinks None
    without sinks, 0 for a head whose sink is -inf"""
    qd, kd, vd = (_f64(t).requires_grad_(True) for t in (q, k, v))
    sd = None if sinks is None else _f64(sinks).requires_grad_(True)
    o, lse = sink_attention(qd, kd, vd, sd, causal, scale, **kw)
    loss = torch.zeros((), dtype=torch.float64)
    if do is not None:
        loss = loss + (o * _f64(do)).sum()
    if dlse is not None:
        loss = loss + lse_loss(lse, _f64(dlse))
    loss.backward()
    ds = None
    if sd is not None:
        ds = torch.zeros_like(sd) if sd.grad is None else torch.nan_to_num(sd.grad, nan=0.0)
        ds = torch.where(torch.isinf(sd.detach()), torch.zeros_like(ds), ds)
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return o.detach(), lse.detach(), zero(qd), zero(kd), zero(vd), ds


def closed_form_backward(q, k, v, do, dlse, sinks, causal, scale, window=(-1, -1)):
    """(dq, dk, dv, dsinks) in fp64 without autograd, the formulas the kernels implement (no dropout, no score modifier):
        P = exp(S - lse), dP = dO V^T, delta = rowsum(dO * O), c = -delta + dlse (rows at lse = -inf: 0),
        dS = P * (dP + c), dV = P^T dO, dQ = scale dS K, dK = scale dS^T Q, dsinks[h] = sum_rows exp(sink_h - lse) * c"""
    qd, kd, vd, dod = (_f64(t) for t in (q, k, v, do))
    sd = _f64(sinks)
    bh, nq, _ = qd.shape
    nk = kd.shape[1]
    g = bh // kd.shape[0]
    with torch.no_grad():
        o, lse = sink_attention(qd, kd, vd, sd, causal, scale, window=window)
    kr, vr = kd.repeat_interleave(g, 0), vd.repeat_interleave(g, 0)
    vis = window_visible(nq, nk, causal, window).unsqueeze(0)
    fin = torch.isfinite(lse)
    lse0 = torch.where(fin, lse, torch.zeros_like(lse))
    p = torch.where(vis & fin.unsqueeze(-1), torch.exp(qd @ kr.transpose(1, 2) * scale - lse0.unsqueeze(-1)), torch.zeros((), dtype=torch.float64))
    c = -(dod * o).sum(-1)
    if dlse is not None:
        c = c + torch.where(fin, _f64(dlse), torch.zeros_like(lse))
    c = torch.where(fin, c, torch.zeros_like(c))
    ds = p * (dod @ vr.transpose(1, 2) + c.unsqueeze(-1))
    dq = scale * ds @ kr
    dk = (scale * ds.transpose(1, 2) @ qd).reshape(bh // g, g, nk, -1).sum(1)
    dv = (p.transpose(1, 2) @ dod).reshape(bh // g, g, nk, -1).sum(1)
    dsinks = None
    if sd is not None:
        su = unit_sinks(sd, bh).reshape(bh, 1)
        w = torch.where(torch.isinf(su) | ~fin, torch.zeros_like(lse), torch.exp(su - lse0))
        dsinks = (w * c).reshape(bh // sd.shape[0], sd.shape[0], nq).sum((0, 2))
    return dq, dk, dv, dsinks


def merge_weights(lse_a, lse_b):
    """(w_a, w_b, lse) in the tensors' dtype, formed around the larger lse; both -inf: weights 0 and lse = -inf"""
    m = torch.maximum(lse_a, lse_b)
    dead = m == NEG_INF
    m0 = torch.where(dead, torch.zeros_like(m), m)
    ea, eb = torch.exp(lse_a - m0), torch.exp(lse_b - m0)
    s = torch.where(dead, torch.ones_like(m), ea + eb)
    lse = torch.where(dead, torch.full_like(m, NEG_INF), m0 + torch.log(s))
    return ea / s, eb / s, lse


def merge(o_a, lse_a, o_b, lse_b):
    """(o, lse) of the merge for o_x (..., rows, d) and lse_x (..., rows) of one floating dtype (fp64 in the tests), differentiable.
    A side with weight 0 is not used (its o may hold NaN); both -inf: o = 0, lse = -inf."""
    wa, wb, lse = merge_weights(lse_a, lse_b)
    wa, wb = wa.unsqueeze(-1), wb.unsqueeze(-1)
    oa = torch.where(wa > 0, o_a, torch.zeros_like(o_a))
    ob = torch.where(wb > 0, o_b, torch.zeros_like(o_b))
    return wa * oa + wb * ob, lse


def merge_backward(o_a, lse_a, o_b, lse_b, do, dlse=None):
    """(do_a, do_b, dlse_a, dlse_b), closed form: t = <do, o_a - o_b>, do_x = w_x do, dlse_a = w_a (dlse + w_b t),
    dlse_b = w_b (dlse - w_a t); a side with weight 0 gets zeros, a row with both -inf zeros everywhere"""
    wa, wb, lse = merge_weights(lse_a, lse_b)
    g = torch.zeros_like(lse) if dlse is None else torch.where(lse == NEG_INF, torch.zeros_like(lse), dlse)
    both = (wa > 0) & (wb > 0)
    diff = torch.where(both.unsqueeze(-1), o_a - o_b, torch.zeros_like(o_a))
    t = (do * diff).sum(-1)
    return wa.unsqueeze(-1) * do, wb.unsqueeze(-1) * do, wa * (g + wb * t), wb * (g - wa * t)


def varlen_attention(qd, kd, vd, sd, cu_q, cu_k, causal, scale, window=(-1, -1)):
    """(o, lse) of packed sequences in fp64, differentiable: qd (total_q, H_q, d), kd, vd (total_k, H_kv, d), sd (H_q,) or None; o
    (total_q, H_q, d), lse (H_q, total_q).  Each sequence is one dense call over its own tokens."""
    hq = qd.shape[1]
    os_, ls = [], []
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if q1 == q0:
            continue
        if k1 == k0:   # rows without any key: o = 0, lse = the sink (-inf without)
            os_.append(torch.zeros_like(qd[q0:q1]))
            ls.append(torch.full((hq, q1 - q0), NEG_INF, dtype=torch.float64) if sd is None else sd.reshape(hq, 1).expand(hq, q1 - q0))
            continue
        o, lse = sink_attention(qd[q0:q1].transpose(0, 1), kd[k0:k1].transpose(0, 1), vd[k0:k1].transpose(0, 1), sd, causal, scale,
                                window=window)
        os_.append(o.transpose(0, 1))
        ls.append(lse)
    return torch.cat(os_, 0), torch.cat(ls, 1).reshape(hq, -1)
