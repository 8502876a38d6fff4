"""fp64 torch reference for attention sinks (fa_ex_*_sink, include/fa_mi355x.h), CPU only; tests/test_sinks_cpu.py checks its
identities and tests/test_sinks_gpu.py holds the kernels to it.

The logits are built with the project's rules in its order — scale, softcap, ALiBi, then causal / window / dense mask / block mask —
the sink column is appended (never capped, biased, masked, windowed or dropped), the softmax is taken and the column dropped
again; dropout then follows oracle.attention_oracle.dropout_keep.  dq, dk, dv and dsinks come from autograd."""
import torch

from oracle import attention_oracle as orc

NEG_INF = float("-inf")


def window_visible(nq, nk, causal, window):
    """(nq, nk) boolean of the causal flag and the window, bottom-right aligned."""
    wl, wr = window
    i = torch.arange(nq).unsqueeze(1)
    j = torch.arange(nk).unsqueeze(0)
    c = nk - nq
    m = torch.ones((nq, nk), dtype=torch.bool)
    if wl >= 0:
        m &= j >= i + c - wl
    if wr >= 0:
        m &= j <= i + c + wr
    if causal:
        m &= j <= i + c
    return m


def unit_sinks(sinks, bh):
    """(bh,) the sink of each query unit: unit u takes sinks[u % sink_heads]; None without sinks."""
    if sinks is None:
        return None
    return sinks[torch.arange(bh) % sinks.shape[0]]


def sink_attention(qd, kd, vd, sd, causal, scale, softcap=0.0, slopes=None, window=(-1, -1), mask=None, block_mask=None, br=128,
                   bc=128, dropout_p=0.0, seed=0):
    """(o, lse) of fp64 tensors qd (BH, Nq, d), kd, vd (BH / g, Nk, d) and sd (sink_heads,) or None, differentiable.
    A row without a visible key: o = 0 and lse = its sink (-inf without sinks, or with a sink of -inf)."""
    bh, nq, _ = qd.shape
    nk = kd.shape[1]
    g = bh // kd.shape[0]
    kr, vr = kd.repeat_interleave(g, 0), vd.repeat_interleave(g, 0)
    s = qd @ kr.transpose(1, 2) * scale
    if softcap > 0.0:
        s = softcap * torch.tanh(s / softcap)
    if slopes is not None:
        dist = (torch.arange(nq).unsqueeze(1) + (nk - nq) - torch.arange(nk).unsqueeze(0)).abs().double()
        s = s - slopes.detach().cpu().double().reshape(bh, 1, 1) * dist
    vis = orc.extended_visible(bh, nq, nk, False, None if mask is None else mask.cpu(), None if block_mask is None else block_mask.cpu(),
                               br, bc)
    vis = vis & window_visible(nq, nk, causal, window).unsqueeze(0)
    s = torch.where(vis, s, torch.tensor(NEG_INF, dtype=torch.float64))
    if sd is not None:
        s = torch.cat([s, unit_sinks(sd, bh).reshape(bh, 1, 1).expand(bh, nq, 1)], dim=-1)   # the sink column
    live = (s > NEG_INF).any(-1, keepdim=True)
    sm = torch.where(live, s, torch.zeros((), dtype=torch.float64))     # (a row of -inf only: no softmax of it)
    p = torch.softmax(sm, -1) * live
    lse = torch.where(live.squeeze(-1), torch.logsumexp(sm, -1), torch.tensor(NEG_INF, dtype=torch.float64))
    p = p[..., :nk]                                                      # the sink's value vector is zero
    if dropout_p > 0.0:
        keep = orc.dropout_keep(bh, nq, nk, dropout_p, seed)
        p = p * keep / (1.0 - dropout_p)
    return p @ vr, lse


def sink_reference(q, k, v, do, sinks, causal, scale, **kw):
    """(o, lse, dq, dk, dv, dsinks): o, dq, dk, dv, dsinks fp64, lse float32; the gradients are None without `do`, dsinks None
    without `sinks`.  A head whose sink is -inf gets dsinks = 0."""
    qd, kd, vd = (t.detach().cpu().double().requires_grad_(True) for t in (q, k, v))
    sd = None if sinks is None else sinks.detach().cpu().double().requires_grad_(True)
    o, lse = sink_attention(qd, kd, vd, sd, causal, scale, **kw)
    if do is None:
        return o.detach(), lse.detach().float(), None, None, None, None
    (o * do.detach().cpu().double()).sum().backward()
    ds = None
    if sd is not None:
        ds = torch.zeros_like(sd) if sd.grad is None else torch.nan_to_num(sd.grad, nan=0.0)
        ds = torch.where(torch.isinf(sd.detach()), torch.zeros_like(ds), ds)
    return o.detach(), lse.detach().float(), qd.grad, kd.grad, vd.grad, ds


def dsink_terms(o, do, lse, sinks):
    """The analytic gradient's summands in fp64: term[u, i] = -exp(sink_u - lse[u, i]) * rowsum(do * o)[u, i] for o, do (BH, Nq, d),
    lse (BH, Nq); dsinks[h] is their sum over the units u with u % sink_heads == h and all rows.  Heads at -inf give 0."""
    bh = o.shape[0]
    su = unit_sinks(sinks.detach().cpu().double(), bh).reshape(bh, 1)
    delta = (o.detach().cpu().double() * do.detach().cpu().double()).sum(-1)
    w = torch.where(torch.isinf(su) & (su < 0), torch.zeros_like(delta), torch.exp(su - lse.detach().cpu().double()))
    return -w * delta


def dsink_sum(term, sink_heads):
    """(sink_heads,) sums of term (BH, Nq) over units u = h, h + sink_heads, .. and rows."""
    bh = term.shape[0]
    return term.reshape(bh // sink_heads, sink_heads, -1).sum((0, 2))


def combine_model(po, plse, sink):
    """The decode combine (kv_combine_kernel<Tag, SINK = true>) as a torch model in fp64: po (S, d) per-split normalised partial
    outputs, plse (S,) their lse (-inf: an empty split, whose po is never written — any value), sink a float (-inf: none).
        m = max(max_s lse_s, sink), denom = sum_s exp(lse_s - m) + exp(sink - m), o = sum_s exp(lse_s - m) O_s / denom,
        lse = m + log(denom);  nothing visible at all (and no sink): o = 0, lse = -inf."""
    plse = plse.double()
    m = max(plse.max().item(), sink)
    if m == NEG_INF:
        return torch.zeros(po.shape[1], dtype=torch.float64), NEG_INF
    w = torch.where(plse == NEG_INF, torch.zeros_like(plse), torch.exp(plse - m))
    ws = 0.0 if sink == NEG_INF else float(torch.exp(torch.tensor(sink - m, dtype=torch.float64)))
    denom = w.sum().item() + ws
    o = (torch.where(w.unsqueeze(1) != 0, w.unsqueeze(1) * po.double(), torch.zeros((), dtype=torch.float64))).sum(0) / denom
    return o, m + float(torch.log(torch.tensor(denom, dtype=torch.float64)))
