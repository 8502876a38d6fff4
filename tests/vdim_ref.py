"""fp64 CPU reference of attention whose v is narrower than q and k (include/fa_mi355x.h: fa_ex_forward_vdim and its family), with
fp64 autograd for the gradients:

    s[i, j] = scale * q[i, h, :d] . k[j, hk, :d]          o[i, h, :d_v] = sum_j softmax_j(s)[i, j] v[j, hk, :d_v]

for query head h reading K/V head hk = h // (H / H_kv), `causal` aligned bottom-right (row i sees keys j <= i + Nk - Nq).  A row
without a visible key gives o = 0 and lse = -inf and sends no gradient anywhere.  The inputs are the 16-bit tensors of the call,
taken to fp64 as they are: the reference sees the rounded values the kernels see.  CPU tensors only; it never imports the
extension."""
import math

import torch

NEG_INF = -math.inf


def vdim_attention(q, k, v, causal, scale):
    """(o (H, Nq, d_v), lse (H, Nq)) in fp64, differentiable in q (H, Nq, d), k (H_kv, Nk, d), v (H_kv, Nk, d_v): fp64 tensors."""
    h, nq, _d = q.shape
    hkv, nk, dv = v.shape
    g = h // hkv
    o = torch.zeros((h, nq, dv), dtype=torch.float64)
    lse = torch.full((h, nq), NEG_INF, dtype=torch.float64)
    if nk == 0 or nq == 0:
        return o, lse
    vis = torch.ones((nq, nk), dtype=torch.bool)
    if causal:
        vis &= torch.arange(nk).view(1, -1) <= torch.arange(nq).view(-1, 1) + (nk - nq)
    live = vis.any(dim=1)                       # rows with a visible key (the same for every head)
    if not bool(live.any()):
        return o, lse
    kk, vv = k.repeat_interleave(g, dim=0), v.repeat_interleave(g, dim=0)
    s = scale * (q[:, live] @ kk.transpose(1, 2))
    s = s.masked_fill(~vis[live], NEG_INF)
    lse_l = torch.logsumexp(s, dim=-1)
    o_l = torch.exp(s - lse_l.unsqueeze(-1)) @ vv
    o[:, live] = o_l
    lse[:, live] = lse_l
    return o, lse


def vdim_reference(q, k, v, causal, scale, do=None, dlse=None):
    """The fp64 results of one (H, Nq, d) / (H_kv, Nk, d) / (H_kv, Nk, d_v) problem from its 16-bit tensors: (o, lse), and with do
    (H, Nq, d_v) also (dq, dk, dv) of the loss sum(o * do) + sum(lse * dlse) over the rows whose lse is finite (dlse: (H, Nq) or
    None)."""
    qd, kd, vd = (t.detach().double().cpu().requires_grad_(do is not None) for t in (q, k, v))
    o, lse = vdim_attention(qd, kd, vd, bool(causal), float(scale))
    if do is None:
        return o.detach(), lse.detach()
    loss = (o * do.detach().double().cpu()).sum()
    if dlse is not None:
        finite = torch.isfinite(lse)
        loss = loss + (torch.where(finite, lse, torch.zeros_like(lse)) * dlse.detach().double().cpu() * finite).sum()
    if loss.requires_grad:
        dq, dk, dv = torch.autograd.grad(loss, (qd, kd, vd), allow_unused=True)
    else:   # no row sees a key: the loss does not depend on anything
        dq = dk = dv = None
    grads = tuple(torch.zeros_like(t) if g is None else g for g, t in zip((dq, dk, dv), (qd, kd, vd)))
    return o.detach(), lse.detach(), grads
