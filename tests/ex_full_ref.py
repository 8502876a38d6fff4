"""The whole extended forward + backward call (ex_forward / ex_backward, ex_varlen_forward / ex_varlen_backward) modelled once on the
CPU, for the sweep of tests/ex_sweep_cases.py:

    full_reference(call)            fp64, gradients by autograd: the reference
    full_reference(call, mutant=m)  the same with one plausible kernel bug built in (MUTANTS)
    baseline(call)                  the same function evaluated as a careful flash kernel of the tensors' dtype would evaluate it
    project_bar / sharp_bar         the two comparisons the sweep applies to a kernel's (or a mutant's) results

`call` is the dict of tests.ex_sweep_cases.build_inputs: the arguments of the raw entry points as CPU tensors, padded
((BH, N, .) tensors) or packed ((total, H, .) tensors with cu_seqlens).  The rules are tests/sink_ref.sink_attention's — scale, softcap,
ALiBi, then causal / window / dense / block visibility, the sink column, the softmax, oracle.attention_oracle.dropout_keep — with a v
of its own width, packed sequences one at a time (the keep mask of a packed call is the padded (batch * H_q, max_seqlen_q,
max_seqlen_k) call's, cut to [u, :len_q, :len_k]: include/fa_mi355x.h) and the loss sum(o * do) + sum(lse * dlse over rows with a
finite lse).

The baseline has no kernel code; it is the closed-form forward and backward with a model of the rounding points, each read from
the kernels and named where it is applied below:
  * inputs as stored, scores and softmax in fp32; the softcap's tanh in the 16-bit kernels' reciprocal form (mod_softcap);
  * the forward's softmax online over tiles of 64 keys (running max, sum and accumulator rescaled per tile), o = acc * (1 / l);
  * P (after dropout) rounded to the tensor dtype before P V and P^T dO; the backward's P taken again from the stored fp32 lse;
  * delta = rowsum(dO * O) from the stored o, in the pre-pass kernel's own summation order (ex_delta_kernel);
  * dS rounded before dS K and dS^T Q;
  * every product accumulated a matrix instruction's run of terms at a time (_mm);
  * with GQA the per-query-head dK / dV partials rounded before the group sum (fa_ex.hip, launch_ex: the kernels write them into the
    workspace in the tensor dtype, kv_partial_bytes / launch_kv_group_sum);
  * every result rounded once.
Those are the extended kernels' points and the defaults of `Model`; the plain path's kernels differ in some of them, and
tests/hot_cases.py passes baseline a Model per route (below: key tile, lazy rescale, exp2 domain, row sum, dS of dK, fa_generic.hip).
For float32 tensors it is the whole computation in fp32.  With fp64 and no rounding it is the reference again
(tests/test_ex_sweep_cpu.py holds the two to each other at 1e-10; the references of single features at 1e-12)."""
from collections import namedtuple

import torch

from oracle import attention_oracle as orc
from tests.helpers import dtype_tolerances

NEG_INF = float("-inf")
MUTANTS = ("window_left_off_by_one", "alibi_without_shift", "sink_not_in_lse", "kv_head_modulo", "tail_keys_dropped", "causal_top_left",
           "dlse_ignored", "softcap_after_alibi", "dropout_unscaled")
TENSORS = ("o", "lse", "dq", "dk", "dv", "dsinks")

# o, dq (as q), dk, dv (as k, v), lse float32-shaped (BH, Nq) / (H_q, total_q), dsinks (H_q,) or None;
# dead_rows: lse-shaped, query rows (of a sequence) without a visible key; dead_keys: (BH_kv, Nk) / (total_k, H_kv), keys no row sees;
# sink_rows: dead rows whose lse is a finite sink; unowned_q, unowned_k: (total,) tokens no sequence owns (None when padded)
Result = namedtuple("Result", "o lse dq dk dv dsinks dead_rows dead_keys sink_rows unowned_q unowned_k")


def _visible(units, nq, nk, causal, window, mask, block_mask, br, bc, mutant):
    """(units or 1, nq, nk) boolean: bottom-right aligned causal flag and window, dense mask, block mask"""
    wl, wr = window
    i = torch.arange(nq).unsqueeze(1)
    j = torch.arange(nk).unsqueeze(0)
    c = nk - nq
    vis = torch.ones((nq, nk), dtype=torch.bool)
    if wl >= 0:
        vis &= j >= i + c - (wl + 1 if mutant == "window_left_off_by_one" else wl)
    if wr >= 0:
        vis &= j <= i + c + wr
    if causal:
        edge = j <= i + (0 if mutant == "causal_top_left" else c)
        if mutant == "diagonal_mask_shifted":      # (hot_mutant) one key more, inside the row's 64 x 64 diagonal block
            edge = edge | ((j == i + c + 1) & (j // 64 == (i + c) // 64))
        vis &= edge
        if mutant == "causal_tail_keys_dropped" and nk % 128 and nk > 128:      # (hot_mutant) the ragged last 128-key tile, under the mask only
            vis[:, nk - nk % 128:] = False
    vis = vis.unsqueeze(0)
    if mask is not None or block_mask is not None:
        vis = vis & orc.extended_visible(units, nq, nk, False, mask, block_mask, br, bc)
    if mutant == "tail_keys_dropped" and nk % 32:
        vis = vis.clone()
        vis[..., nk - nk % 32:] = False
    return vis


def _problems(call, mutant=None):
    """The dense problems a call is made of: the one (BH, Nq, Nk) problem of a padded call, or one (H_q, len_q, len_k) problem per
    sequence with query rows.  Each is a dict: tq / tk / tl cut a query-token, key-token or lse-shaped tensor of the call to the
    problem's (units, rows, .) view; kvi the K/V unit of each query unit; sink / slope per unit; vis; keep."""
    hq, hkv = call["heads"]
    g = hq // hkv
    p, seed = call["dropout_p"], call["seed"]
    sinks, slopes = call["sinks"], call["alibi_slopes"]
    head_kv = (lambda h: h % hkv) if mutant == "kv_head_modulo" else (lambda h: h // g)
    if call["layout"] == "padded":
        bh, nq = call["q"].shape[:2]
        nk = call["k"].shape[1]
        u = torch.arange(bh)
        ident = lambda t: t   # noqa: E731
        yield dict(tq=ident, tk=ident, tl=ident, nq=nq, nk=nk, kvi=(u // hq) * hkv + head_kv(u % hq),
                   sink=None if sinks is None else (lambda s: s[u % hq]), slope=None if slopes is None else slopes.double().reshape(bh),
                   vis=_visible(bh, nq, nk, call["causal"], call["window"], call["mask"], call["block_mask"], call["br"], call["bc"], mutant),
                   keep=orc.dropout_keep(bh, nq, nk, p, seed) if p > 0.0 else None)
        return
    cu_q, cu_k = call["cu_seqlens_q"].tolist(), call["cu_seqlens_k"].tolist()
    nb = len(cu_q) - 1
    keep_all = orc.dropout_keep(nb * hq, call["max_seqlen_q"], call["max_seqlen_k"], p, seed) if p > 0.0 else None
    h = torch.arange(hq)
    for b in range(nb):
        q0, q1, k0, k1 = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        nq, nk = q1 - q0, k1 - k0
        if nq == 0:
            continue
        yield dict(tq=lambda t, a=q0, z=q1: t[a:z].transpose(0, 1), tk=lambda t, a=k0, z=k1: t[a:z].transpose(0, 1),
                   tl=lambda t, a=q0, z=q1: t[:, a:z], nq=nq, nk=nk, kvi=head_kv(h),
                   sink=None if sinks is None else (lambda s: s),
                   slope=None if slopes is None else (slopes[b] if slopes.dim() == 2 else slopes).double(),
                   vis=_visible(hq, nq, nk, call["causal"], call["window"], None, None, 0, 0, mutant),
                   keep=None if keep_all is None else keep_all[b * hq:(b + 1) * hq, :nq, :nk])


LOG2E = 1.4426950408889634
KEY_TILE = 64      # keys per step of the forward's online softmax

# The rounding points that differ between kernel families, as one record (the argument `model` of baseline).  The defaults are the
# extended kernels' (the module docstring); tests/hot_cases.py names a model per route of the plain path.  Each non-default value
# models the file and function written beside it:
#   key_tile           keys per step of the online softmax: 128 on the plain forward (fa_fwd_mfma.hip, launch_fwd_kb: launch_fwd_t<Tag, D,
#                      4>, KB = 4 blocks of 32 keys), 64 at d = 64 without the mask and at 256-wide (launch_fwd_kb / launch_fwd_mfma:
#                      launch_fwd_t<Tag, D, 2>), 32 / 64 under fwd_kb = 1 / 2
#   lazy_rescale       the running max moves, and o and l are rescaled, only on a tile where some row of the wave's 32 grew by more than
#                      2^8 (fa_fwd_mfma.hip, fwd_mfma_kernel: `if (LAZY) rescale = __any((m_new - m_run) * c_log2 > 8.0f)`; every row of
#                      the 32 then moves to its own new max); False: every tile (fwd_eager, and the extended kernels)
#   exp2               P = exp2(fma(q.k, scale * log2 e, -m * scale * log2 e)) on the unscaled scores with the max of the unscaled scores,
#                      lse = m * scale + log(l) (fa_fwd_mfma.hip, fwd_mfma_kernel: `exp2f(fmaf(sacc, c_log2, -mc))`, `m_run * scale +
#                      logf(l_tot)`)
#   rowsum_rounded_p   the row sum l from the P that was rounded for P V, on the matrix pipe (fa_fwd_mfma.hip, fwd_mfma_kernel, RS_MFMA:
#                      `lacc = mfma32(ones, pb, lacc)`; option fwd_rs)
#   dk_ds_from_rounded_p  the dS of dK = dS^T Q is round(round(P) * (dP - delta)): the 8-wave dK/dV kernel multiplies the 16-bit P it made
#                      for P^T dO (fa_bwd_dkdv_mfma.hip, bwd_dkdv_mfma_kernel: "dS = P dP' with the 16-bit P that also feeds dV", mul_pack;
#                      DESIGN.md section 6, "stream: dS"); False: from the f32 P, one rounding (fa_bwd_dkdv_w4.hip, bwd_dkdv_w4_kernel;
#                      fa_bwd_mfma.hip, bwd_mfma_kernel: `pacc[i] = p * pacc[i]`).  The dS of dQ is from the f32 P in every kernel
#                      (fa_bwd_dq_mfma.hip, bwd_dq_mfma_kernel: `pacc[i] = exp2f(..) * pacc[i]`)
#   f32_inside         16-bit tensors through the exact kernels: P and dS stay float32, every product is the float32 matrix instruction's
#                      (fa_generic.hip, header: "any dtype in, f32 math", v_mfma_f32_16x16x4_f32; fwd_f32_kernel walks key tiles of 32);
#                      only the results are rounded
#   fma_chain          every product an fma chain, one term at a time on the accumulator (_mm, chunk = 1), the forward's P V chain starting
#                      from the rescaled running o (fa_generic.hip, fwd_f32_kernel: `acc[t] = MFMA_F32(a[j], Vs[..], acc[t])`).  Four
#                      roundings at the accumulator's magnitude where a product summed a run at a time has one: twice the noise
Model = namedtuple("Model", "key_tile lazy_rescale exp2 rowsum_rounded_p dk_ds_from_rounded_p f32_inside fma_chain",
                   defaults=(KEY_TILE, False, False, False, False, False, False))
DEFAULT_MODEL = Model()


def _fma(a, b, c, ct):
    """a * b + c rounded once, as v_fma_f32 rounds it (float32: through float64, where the product is exact)"""
    if ct != torch.float32:
        return a * b + c
    return (a.double() * b + c.double()).float()


def _mm(a, b, chunk=0, init=None):
    """a @ b with the contraction cut into runs of `chunk` terms that are added to the accumulator one after another, as a matrix
    instruction adds its short dot product to an fp32 accumulator register (0: one product, the library's own order).  chunk = 4
    is the exact-f32 kernels' order (fa_ex.hip, the MFMA_F32 loops of ex_fwd_body / ex_dkdv_body / ex_dq_body): per block of 16
    columns, instruction j = 0 .. 3 takes the columns j, 4 + j, 8 + j, 12 + j, one from each of the four lane groups.  chunk = 1 is
    that order with every term added to the accumulator on its own, rounded once — the plain path's exact kernels (fa_generic.hip,
    header: v_mfma_f32_16x16x4_f32, "whose result is bit-for-bit an f32 fma chain"); `init` is then the accumulator the chain
    starts from (the rescaled running o of the forward)."""
    k = a.shape[-1]
    if chunk == 1:
        pad = (-k) % 16
        if pad:
            a = torch.nn.functional.pad(a, (0, pad))
            b = torch.nn.functional.pad(b, (0, 0, 0, pad))
        order = torch.arange(k + pad).reshape(-1, 4, 4).transpose(1, 2).reshape(-1)
        a, b = a[..., order], b[..., order, :]
        # float32: term by term in float64, where the product is exact, rounded to float32 after every addition (in place: the
        # (Nq, Nk) products take d steps each)
        acc = (torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=a.dtype) if init is None else init).double()
        a64, b64 = a.double(), b.double()
        if a.dtype != torch.float32:
            for k0 in range(k + pad):
                acc.addcmul_(a64[..., k0:k0 + 1], b64[..., k0:k0 + 1, :])
            return acc.to(a.dtype)
        out = torch.empty(acc.shape, dtype=torch.float32)
        for k0 in range(k + pad):
            acc.addcmul_(a64[..., k0:k0 + 1], b64[..., k0:k0 + 1, :])
            out.copy_(acc)
            acc.copy_(out)
        return out
    assert init is None
    if chunk <= 0 or k <= chunk:
        return a @ b
    if chunk == 4:
        pad = (-k) % 16
        if pad:
            a = torch.nn.functional.pad(a, (0, pad))
            b = torch.nn.functional.pad(b, (0, 0, 0, pad))
            k += pad
        order = torch.arange(k).reshape(-1, 4, 4).transpose(1, 2).reshape(-1)      # (block, lane group, j) -> (block, j, lane group)
        a, b = a[..., order], b[..., order, :]
    acc = a[..., :chunk] @ b[..., :chunk, :]
    for k0 in range(chunk, k, chunk):
        acc = acc + a[..., k0:k0 + chunk] @ b[..., k0:k0 + chunk, :]
    return acc


def _scores(q, kr, pr, call, ct, mutant=None, rcp_form=False, chunk=0):
    """(s, dt): the masked logits of a problem in dtype ct and, under a softcap, dt = 1 - tanh(s_raw / softcap)^2.  rcp_form: the
    tanh as the 16-bit kernels take it (fa_ex_common.h, mod_softcap): t = 1 - 2 r, r = 1 / (2^(2 log2(e) s / softcap) + 1),
    dt = 4 r (1 - r), every operation in ct"""
    nq, nk, cap = pr["nq"], pr["nk"], call["softcap"]
    s = _mm(q, kr.transpose(1, 2), chunk) * call["scale"]
    bias = dt = None
    if pr["slope"] is not None:
        coff = 0 if mutant == "alibi_without_shift" else nk - nq
        dist = (torch.arange(nq).unsqueeze(1) + coff - torch.arange(nk).unsqueeze(0)).abs().to(ct)
        bias = pr["slope"].to(ct).reshape(-1, 1, 1) * dist
    if mutant == "softcap_after_alibi" and cap > 0.0 and bias is not None:
        s = cap * torch.tanh((s - bias) / cap)
    else:
        if cap > 0.0 and rcp_form:
            r = 1.0 / (torch.exp2(s * (2.0 * LOG2E / cap)) + 1.0)
            dt = r * (4.0 - 4.0 * r)
            s = cap - (2.0 * cap) * r
        elif cap > 0.0:
            t = torch.tanh(s / cap)
            dt = 1.0 - t * t
            s = cap * t
        if bias is not None:
            s = s - bias
    return torch.where(pr["vis"], s, torch.tensor(NEG_INF, dtype=ct)), dt


def _delta(dop, op):
    """rowsum(dO * O) in the order of the backward's pre-pass (fa_ex.hip, ex_delta_kernel): sixteen lanes a row, lane c adds the
    products c, c + 16, .. in turn, then a butterfly over the lanes — a sum of its own, not the dP product's accumulation"""
    prod = dop * op
    pad = (-prod.shape[-1]) % 16
    if pad:
        prod = torch.nn.functional.pad(prod, (0, pad))
    x = prod.reshape(prod.shape[:-1] + (-1, 16))
    acc = x[..., 0, :]
    for i in range(1, x.shape[-2]):
        acc = acc + x[..., i, :]
    for _ in range(4):
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def _attend(q, k, v, sinks, pr, call, mutant):
    """(o, lse) of one problem in fp64, differentiable in q (U, nq, d), k, v (U_kv, nk, .) and sinks"""
    u, nq, nk = q.shape[0], pr["nq"], pr["nk"]
    su = None if sinks is None else pr["sink"](sinks).reshape(u, 1, 1).expand(u, nq, 1)
    if nk == 0:        # no key at all: o = 0 and lse = the sink (-inf without one)
        o = torch.zeros((u, nq, v.shape[2]), dtype=torch.float64)
        return o, (torch.full((u, nq), NEG_INF, dtype=torch.float64) if su is None or mutant == "sink_not_in_lse" else su.squeeze(-1) + 0.0)
    s, _t = _scores(q, k[pr["kvi"]], pr, call, torch.float64, mutant)
    cols = s if su is None else torch.cat([s, su], dim=-1)
    live = (cols > NEG_INF).any(-1, keepdim=True)
    p = torch.softmax(torch.where(live, cols, torch.zeros((), dtype=torch.float64)), -1) * live
    lcols = s if mutant == "sink_not_in_lse" else cols
    llive = (lcols > NEG_INF).any(-1)
    lse = torch.where(llive, torch.logsumexp(torch.where(llive.unsqueeze(-1), lcols, torch.zeros((), dtype=torch.float64)), -1),
                      torch.tensor(NEG_INF, dtype=torch.float64))
    p = p[..., :nk]
    if pr["keep"] is not None:
        p = p * pr["keep"] / (1.0 if mutant == "dropout_unscaled" else 1.0 - call["dropout_p"])
    return p @ v[pr["kvi"]], lse


def _sets(call, lse):
    """dead_rows, dead_keys, sink_rows, unowned_q, unowned_k of a call (by visibility alone; dropout removes nothing)"""
    hq, hkv = call["heads"]
    g = hq // hkv
    dead_rows = torch.zeros(lse.shape, dtype=torch.bool)
    seen = torch.zeros(tuple(call["k"].shape[:2]), dtype=torch.bool)
    packed = call["layout"] != "padded"
    own_q = torch.zeros(call["q"].shape[0], dtype=torch.bool) if packed else None
    own_k = torch.zeros(call["k"].shape[0], dtype=torch.bool) if packed else None
    for pr in _problems(call):
        vis = pr["vis"].expand(pr["kvi"].shape[0], pr["nq"], pr["nk"])
        pr["tl"](dead_rows).copy_(~vis.any(-1))
        by_unit = vis.any(1)                                                      # (units, nk)
        seen_kv = by_unit.reshape(by_unit.shape[0] // g, g, pr["nk"]).any(1)                         # (units / g, nk): unit u reads K/V unit u // g
        tgt = seen if not packed else pr["tk"](seen.unsqueeze(-1)).squeeze(-1)     # (U_kv, nk) view
        tgt.copy_(seen_kv)
    if packed:
        cu_q, cu_k = call["cu_seqlens_q"].tolist(), call["cu_seqlens_k"].tolist()
        for b in range(len(cu_q) - 1):
            own_q[cu_q[b]:cu_q[b + 1]] = True
            own_k[cu_k[b]:cu_k[b + 1]] = True
    dead_keys = ~seen
    if packed:
        dead_keys &= own_k.unsqueeze(1)
        dead_rows &= own_q.unsqueeze(0)
    sink_rows = dead_rows & torch.isfinite(lse)
    return dead_rows, dead_keys, sink_rows, None if not packed else ~own_q, None if not packed else ~own_k


def lse_loss(lse, dlse):
    """sum(lse * dlse) over the rows with a finite lse, whatever dlse holds elsewhere"""
    fin = torch.isfinite(lse)
    return (torch.where(fin, lse, torch.zeros_like(lse)) * torch.where(fin, dlse, torch.zeros_like(dlse))).sum()


def full_reference(call, mutant=None):
    """Result of the call in fp64 (lse too); tokens no sequence owns hold zeros (lse: NaN)"""
    assert mutant is None or mutant in MUTANTS or mutant in ("causal_tail_keys_dropped", "diagonal_mask_shifted")
    qd, kd, vd = (call[n].detach().double().clone().requires_grad_(True) for n in ("q", "k", "v"))
    sd = None if call["sinks"] is None else call["sinks"].detach().double().clone().requires_grad_(True)
    packed = call["layout"] != "padded"
    lse_shape = (call["heads"][0], qd.shape[0]) if packed else tuple(qd.shape[:2])
    o = torch.zeros(tuple(qd.shape[:2]) + (vd.shape[2],), dtype=torch.float64)
    lse = torch.full(lse_shape, float("nan") if packed else 0.0, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    do = call["do"].double()
    dlse = None if call["dlse"] is None or mutant == "dlse_ignored" else call["dlse"].double()
    for pr in _problems(call, mutant):
        op, lp = _attend(pr["tq"](qd), pr["tk"](kd), pr["tk"](vd), sd, pr, call, mutant)
        pr["tq"](o).copy_(op.detach())
        pr["tl"](lse).copy_(lp.detach())
        loss = loss + (op * pr["tq"](do)).sum()
        if dlse is not None:
            loss = loss + lse_loss(lp, pr["tl"](dlse))
    if loss.requires_grad:
        loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
    ds = None
    if sd is not None:
        ds = torch.nan_to_num(zero(sd), nan=0.0)
        ds = torch.where(torch.isinf(sd.detach()), torch.zeros_like(ds), ds)
    return Result(o, lse, zero(qd), zero(kd), zero(vd), ds, *_sets(call, lse))


def round_to(dtype):
    """x -> x rounded to dtype and back (identity for None)"""
    if dtype is None:
        return lambda x: x
    return lambda x: x.to(dtype).to(x.dtype)


def baseline(call, compute=torch.float32, tensor_dtype="call", model=DEFAULT_MODEL):
    """The call through the closed-form forward and backward in dtype `compute`, rounded at the points of the module docstring to
    `tensor_dtype` (default: the call's; None: nowhere), with the rounding points of `model` (a Model; the default is the extended
    kernels').  Results in `compute`; the sets are not filled in."""
    ct = compute
    md = model
    assert not md.exp2 or (call["softcap"] == 0.0 and call["alibi_slopes"] is None and call["sinks"] is None), "exp2: plain calls only"
    dt = call["dtype"] if tensor_dtype == "call" else tensor_dtype
    rnd = round_to(None if dt is None or dt == ct else dt)
    # the products' accumulation: 16 terms an instruction on the 16-bit kernels (v_mfma_f32_32x32x16_{bf16,f16}: DESIGN.md §4), 4 on
    # the exact-f32 kernels (fa_ex.hip, MFMA_F32 over f32x4 operands, four per 16 columns)
    chunk = 1 if md.fma_chain else 4 if call["dtype"] == torch.float32 or md.f32_inside else 16
    rin = round_to(None) if md.f32_inside else rnd      # the roundings between the loads and the stores
    hq, hkv = call["heads"]
    g = hq // hkv
    q, k, v, do = (call[n].to(ct) for n in ("q", "k", "v", "do"))
    packed = call["layout"] != "padded"
    lse = torch.full((hq, q.shape[0]) if packed else tuple(q.shape[:2]), float("nan") if packed else 0.0, dtype=ct)
    o = torch.zeros(tuple(q.shape[:2]) + (v.shape[2],), dtype=ct)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    sinks = None if call["sinks"] is None else call["sinks"].to(ct)
    ds = None if sinks is None else torch.zeros_like(sinks)
    dlse = None if call["dlse"] is None else call["dlse"].to(ct)
    p_drop, scale, cap = call["dropout_p"], call["scale"], call["softcap"]
    zero = torch.zeros((), dtype=ct)
    for pr in _problems(call):
        qp, kp, vp, dop = pr["tq"](q), pr["tk"](k), pr["tk"](v), pr["tq"](do)
        u, nq, nk, kvi = qp.shape[0], pr["nq"], pr["nk"], pr["kvi"]
        su = None if sinks is None else pr["sink"](sinks).reshape(u, 1)
        kr, vr = kp[kvi], vp[kvi]
        s, dt = _scores(qp, kr, pr, call, ct, rcp_form=True, chunk=chunk)
        dmul = pr["keep"].to(ct) / (1.0 - p_drop) if pr["keep"] is not None else None
        # forward: the online softmax over key tiles (fa_ex.hip, ex_fwd_body: alpha = expf(m - msafe), p = expf(x - msafe); the
        # MFMA kernels alike) — running max m, sum l and accumulator, each rescaled at every tile; the sink joins at the end
        m = torch.full((u, nq), NEG_INF, dtype=ct)
        l_ = torch.zeros((u, nq), dtype=ct)
        acc = torch.zeros((u, nq, vr.shape[2]), dtype=ct)
        c2 = scale * LOG2E                                                   # (exp2: the kernels' c_log2, a float)
        if md.exp2:
            c2 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)) if ct == torch.float32 else c2
            s_fwd = torch.where(pr["vis"], _mm(qp, kr.transpose(1, 2), chunk), torch.tensor(NEG_INF, dtype=ct))    # unscaled scores
        else:
            s_fwd = s
        for t0 in list(range(0, nk, md.key_tile)) + ([None] if su is not None else []):
            if t0 is None:
                m_new = torch.maximum(m, su.expand(u, nq))
            else:
                st = s_fwd[..., t0:t0 + md.key_tile]
                m_new = torch.maximum(m, st.max(-1).values)
            if md.lazy_rescale:
                # a wave's 32 query rows decide together; a row that stays keeps its stale max (and alpha = 1)
                grow = (m_new - m) * (c2 if md.exp2 else LOG2E) > 8.0            # (first visible key: inf > 8; none yet: nan > 8 is False)
                pad = (-nq) % 32
                gw = torch.nn.functional.pad(grow, (0, pad)).reshape(u, -1, 32).any(-1, keepdim=True).expand(u, -1, 32).reshape(u, -1)[:, :nq]
                m_new = torch.where(gw, m_new, m)
            msafe = torch.where(m_new > NEG_INF, m_new, zero)
            alpha = torch.exp2((m - msafe) * c2) if md.exp2 else torch.exp(m - msafe)
            if t0 is None:
                l_ = l_ * alpha + torch.exp(su - msafe)
                acc = acc * alpha.unsqueeze(-1)
            else:
                pt = torch.exp2(_fma(st, c2, -(msafe * c2).unsqueeze(-1), ct)) if md.exp2 else torch.exp(st - msafe.unsqueeze(-1))
                ptd = rin(pt if dmul is None else pt * dmul[..., t0:t0 + md.key_tile])
                l_ = l_ * alpha + (rin(pt) if md.rowsum_rounded_p else pt).sum(-1)
                if md.fma_chain:
                    acc = _mm(ptd, vr[:, t0:t0 + md.key_tile], chunk, init=acc * alpha.unsqueeze(-1))
                else:
                    acc = acc * alpha.unsqueeze(-1) + _mm(ptd, vr[:, t0:t0 + md.key_tile], chunk)
            m = m_new
        live = m > NEG_INF
        l_ = torch.where(live, l_, torch.ones((), dtype=ct))
        lp = torch.where(live, (m * scale if md.exp2 else m) + torch.log(l_), torch.tensor(NEG_INF, dtype=ct))
        op = rnd(acc * (1.0 / l_).unsqueeze(-1))                  # (fa_ex.hip, ex_fwd_body: inv = 1.f / l, o = acc * inv)
        # backward, from the stored o and lse: P = exp(s - lse) again (ex_dq_body / ex_dkdv_body and the MFMA kernels read lse back)
        prob = torch.where(live.unsqueeze(-1), torch.exp(s - torch.where(live, lp, zero).unsqueeze(-1)), zero)
        pd = rin(prob if dmul is None else prob * dmul)
        dp = _mm(dop, vr.transpose(1, 2), chunk)
        if dmul is not None:
            dp = dp * dmul
        c = -_delta(dop, op)
        if dlse is not None:
            c = c + torch.where(live, pr["tl"](dlse), zero)
        c = torch.where(live, c, zero)
        dsc = prob * (dp + c.unsqueeze(-1))
        if dt is not None:
            dsc = dsc * dt
        dsc = rin(torch.where(pr["vis"], dsc, zero))
        dsk = dsc
        if md.dk_ds_from_rounded_p:
            assert dt is None, "dk_ds_from_rounded_p: plain calls only"
            dsk = rin(torch.where(pr["vis"], rin(prob) * (dp + c.unsqueeze(-1)), zero))
        dqp = rnd(scale * _mm(dsc, kr, chunk))
        dk_u, dv_u = scale * _mm(dsk.transpose(1, 2), qp, chunk), _mm(pd.transpose(1, 2), dop, chunk)
        if g > 1:
            dk_u, dv_u = rnd(dk_u), rnd(dv_u)
        dkp = rnd(torch.zeros_like(kp).index_add_(0, kvi, dk_u))
        dvp = rnd(torch.zeros_like(vp).index_add_(0, kvi, dv_u))
        pr["tq"](o).copy_(op)
        pr["tl"](lse).copy_(lp)
        pr["tq"](dq).copy_(dqp)
        pr["tk"](dk).copy_(dkp)
        pr["tk"](dv).copy_(dvp)
        if su is not None:
            w = torch.where(live & torch.isfinite(su), torch.exp(su - torch.where(live, lp, zero)), zero)
            term = (w * c).sum(-1)                                                                    # per unit
            ds += term.reshape(-1, hq).sum(0)
    return Result(o, lse, dq, dk, dv, ds, None, None, None, None, None)


def rounded(res, dtype):
    """a Result as a kernel would return it: o, dq, dk, dv in dtype, lse and dsinks float32 (the sets kept)"""
    r16 = lambda t: t.to(dtype)   # noqa: E731
    return res._replace(o=r16(res.o), dq=r16(res.dq), dk=r16(res.dk), dv=r16(res.dv), lse=res.lse.float(),
                        dsinks=None if res.dsinks is None else res.dsinks.float())


# ---- the two bars.  `got`: anything with o, lse, dq, dk, dv, dsinks in the call's layout (a Result, or the kernel's tensors)

def _owned(name, t, ref):
    """tensor `name` without the tokens no sequence owns"""
    if ref.unowned_q is None or name == "dsinks":
        return t
    if name == "lse":
        return t[:, ~ref.unowned_q]
    return t[~(ref.unowned_k if name in ("dk", "dv") else ref.unowned_q)]


def project_bar(got, ref, dtype, only_tolerances=False):
    """The project's bar as a list of failures (empty: passed): nothing NaN, o, dq, dk, dv, dsinks within dtype_tolerances of fp64,
    the -inf pattern of lse exact and finite lse at rtol = atol = 1e-3; the exact zeros — o and dq on rows without a visible key,
    dk and dv on keys no row sees — and lse = the sink on sink-only rows.  only_tolerances: the dtype_tolerances part alone."""
    tol = dtype_tolerances(dtype)
    bad = []
    for name in ("o", "dq", "dk", "dv", "dsinks"):
        r = getattr(ref, name)
        if r is None:
            continue
        a, b = _owned(name, getattr(got, name).double(), ref), _owned(name, r, ref)
        if torch.isnan(a).any():
            bad.append(f"{name}: NaN")
        elif not bool(((a - b).abs() <= tol["atol"] + tol["rtol"] * b.abs()).all()):
            bad.append(f"{name}: max |got - fp64| = {(a - b).abs().max().item():.3e} outside rtol = atol = {tol['atol']:g}")
    if only_tolerances:
        return bad
    a, b = _owned("lse", got.lse.double(), ref), _owned("lse", ref.lse, ref)
    fin = torch.isfinite(b)
    if torch.isnan(a).any():
        bad.append("lse: NaN")
    elif not torch.equal(torch.isfinite(a), fin) or not bool((a[~fin] == NEG_INF).all()):
        bad.append("lse: the -inf pattern differs")
    elif not bool(((a[fin] - b[fin]).abs() <= 1e-3 + 1e-3 * b[fin].abs()).all()):
        bad.append(f"lse: max |got - fp64| = {(a[fin] - b[fin]).abs().max().item():.3e} outside rtol = atol = 1e-3")
    dead_q = ref.dead_rows.transpose(0, 1) if ref.unowned_q is not None else ref.dead_rows            # (tokens, H_q) when packed
    if bool((got.o[dead_q] != 0).any()) or bool((got.dq[dead_q] != 0).any()):
        bad.append("o or dq != 0 on a row without a visible key")
    if bool((got.dk[ref.dead_keys] != 0).any()) or bool((got.dv[ref.dead_keys] != 0).any()):
        bad.append("dk or dv != 0 on a key no row sees")
    return bad


def errors(got, ref):
    """{tensor: (max |got - fp64| over the owned tokens and finite lse, max |fp64|)}"""
    out = {}
    for name in TENSORS:
        r = getattr(ref, name)
        if r is None:
            continue
        a, b = _owned(name, getattr(got, name).double(), ref), _owned(name, r, ref)
        if name == "lse":
            fin = torch.isfinite(b) & torch.isfinite(a)
            a, b = a[fin], b[fin]
        out[name] = ((a - b).abs().max().item(), b.abs().max().item()) if b.numel() else (0.0, 0.0)
    return out


def sharp_bar(got, ref, base, dtype):
    """(failures, {tensor: kernel error / baseline error}) of the sharp bar, per tensor in the max norm:
        max |got - fp64| <= 2 * max |baseline - fp64| + eps * max |fp64|
    with eps that of the call's dtype — for dsinks too, a float32 sum over every row of terms made from the stored o — and of float32
    for lse, which the kernels make in fp32 from exact products (the one final rounding)."""
    eg, eb = errors(got, ref), errors(base, ref)
    bad, ratio = [], {}
    for name, (err, big) in eg.items():
        eps = torch.finfo(torch.float32 if name == "lse" else dtype).eps
        bound = 2.0 * eb[name][0] + eps * big
        ratio[name] = err / eb[name][0] if eb[name][0] > 0.0 else (0.0 if err == 0.0 else float("inf"))
        if not err <= bound:
            bad.append(f"{name}: max |got - fp64| = {err:.3e} > 2 * {eb[name][0]:.3e} (baseline) + {eps:.1e} * {big:.3e} = {bound:.3e}")
    return bad, ratio


def _cut(res, names, a, b):
    """a Result with the tensors `names` cut to [a, b) of dimension 1 and nothing else (padded calls)"""
    return Result(*[(getattr(res, n)[:, a:b] if n in names and getattr(res, n) is not None else None) for n in TENSORS], None, None, None, None, None)


def band_edges(nq, nk):
    """The bands of a padded call under the causal mask: query rows [0, 64), [64, 256), [256, Nq) for o, lse and dq — the first rows,
    where |o| ~ |v|, would otherwise set the maximum for the long rows — and keys [0, Nk - 256), [Nk - 256, Nk - 64), [Nk - 64, Nk)
    for dk and dv, whose last keys few rows see.  Empty bands are left out."""
    rows = [(a, min(b, nq)) for a, b in ((0, 64), (64, 256), (256, nq)) if a < min(b, nq)]
    e1, e2 = max(nk - 256, 0), max(nk - 64, 0)
    keys = [(a, b) for a, b in ((0, e1), (e1, e2), (e2, nk)) if a < b]
    return rows, keys


def banded_sharp_bar(got, ref, base, dtype):
    """sharp_bar — the same function, the same factor — on each band of band_edges alone: (failures, {tensor[a:b]: ratio})"""
    rows, keys = band_edges(ref.o.shape[1], ref.dk.shape[1])
    bad, ratio = [], {}
    for names, bands in ((("o", "lse", "dq"), rows), (("dk", "dv"), keys)):
        for a, b in bands:
            fails, r = sharp_bar(_cut(got, names, a, b), _cut(ref, names, a, b), _cut(base, names, a, b), dtype)
            bad += [f"[{a}:{b}] {f}" for f in fails]
            ratio.update({f"{n}[{a}:{b}]": v for n, v in r.items()})
    return bad, ratio


# ---- bugs of the kind a schedule rewrite of the plain kernels makes (tests/test_hot_sweep_cpu.py; plain padded calls only)

HOT_MUTANTS = ("delta_over_half_d", "o_times_1.02", "dq_times_1.1", "lse_plus_2e-4", "causal_tail_keys_dropped", "pv_block_rescaled_twice",
               "dq_stale_k_block", "diagonal_mask_shifted", "dk_last_query_tile_missing")


def hot_mutant(call, ref, name):
    """the fp64 Result of a plain padded call with one bug built in:
      delta_over_half_d           delta = rowsum(dO * O) over the first d / 2 columns (a row constant made from half a row)
      o_times_1.02, dq_times_1.1  a scale slip; lse_plus_2e-4: lse off by 200 times its rounding error
      causal_tail_keys_dropped    under the mask, the last Nk % 128 keys are never visited (the ragged last key tile)
      diagonal_mask_shifted       under the mask, row i also sees key i + 1 inside its 64 x 64 diagonal block
      pv_block_rescaled_twice     unit 0, the last 32-row block of queries: the P V sum over keys [0, 64) multiplied once more by the
                                  factor exp(m(keys < 64) - m(keys < 128)) of the second tile
      dq_stale_k_block            unit 0: dS[:, 64:96] meets K[0:32], the rows the operand slot held one 64-key tile earlier
      dk_last_query_tile_missing  dK without the contribution of the last 64-row query tile"""
    assert name in HOT_MUTANTS and call["layout"] == "padded" and call["heads"] == (1, 1)
    if name in ("causal_tail_keys_dropped", "diagonal_mask_shifted"):
        return full_reference(call, mutant=name)
    if name == "o_times_1.02":
        return ref._replace(o=ref.o * 1.02)
    if name == "dq_times_1.1":
        return ref._replace(dq=ref.dq * 1.1)
    if name == "lse_plus_2e-4":
        return ref._replace(lse=ref.lse + 2e-4)
    q, k, v, do = (call[n].double() for n in ("q", "k", "v", "do"))
    (pr,) = _problems(call)
    nq, nk, scale = pr["nq"], pr["nk"], call["scale"]
    s, _dt = _scores(q, k, pr, call, torch.float64)
    p = torch.exp(s - ref.lse.unsqueeze(-1))                      # (no dead rows in a plain call: Nk >= Nq under the mask)
    if name == "pv_block_rescaled_twice":
        if nk <= 64:
            return ref
        r0 = 32 * ((nq - 1) // 32)
        alpha = torch.exp(s[0, r0:, :64].max(-1).values - s[0, r0:, :128].max(-1).values)
        o = ref.o.clone()
        o[0, r0:] += (alpha - 1.0).unsqueeze(-1) * (p[0, r0:, :64] @ v[0, :64])
        return ref._replace(o=o)
    d = q.shape[2]
    half = name == "delta_over_half_d"
    delta = (do * ref.o)[..., :d // 2 if half else d].sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(1, 2) - delta)
    if half:
        return ref._replace(dq=scale * ds @ k, dk=scale * ds.transpose(1, 2) @ q)
    if name == "dq_stale_k_block":
        if nk < 96:
            return ref
        dq = ref.dq.clone()
        dq[0] += scale * ds[0, :, 64:96] @ (k[0, 0:32] - k[0, 64:96])
        return ref._replace(dq=dq)
    r0 = 64 * ((nq - 1) // 64)                                       # dk_last_query_tile_missing
    return ref._replace(dk=ref.dk - scale * ds[:, r0:].transpose(1, 2) @ q[:, r0:])
