"""Host-side counterpart of the attention core of the reference's notebook model
(`MultiHeadAttention._block_sparse_flash_attention(q, k, v, tau, mask, block_sparse_mask)`,
/root/reference/src/fa3/torch/flashattention_pytorch.py:94-174, and its dense branch :80-87) over the HIP library's
extended entry points (`fa_ex_forward` / `fa_ex_backward`, include/fa_mi355x.h):

    flash_attention_ex(q, k, v, tau=1.0, mask=None, block_sparse_mask=None, block_size=128,
                       causal=False, dropout_p=0.0, seed=0, softmax_scale=None, window_size=(-1, -1),
                       softcap=0.0, alibi_slopes=None, *, return_lse=False, sinks=None) -> o  |  (o, lse)

q: (B, H, Nq, d) or (BH, Nq, d); k, v: (B, H_kv, Nk, d) or (B*H_kv, Nk, d); v may be narrower, (B, H_kv, Nk, d_v) or (B*H_kv, Nk, d_v)
(see "A v of its own width" below).  H_kv < H is grouped-query attention (GQA; H_kv = 1:
multi-query attention) with H % H_kv == 0: query head h reads K/V head h // (H / H_kv), with no copy of K and V, and the
gradients of k and v come back in k's and v's shape, summed over each group by the library.  `mask` follows the model's convention — a boolean / 0-1 tensor
broadcastable to (B, H, Nq, Nk), True / 1 = allowed (`look_ahead_mask_` builds the causal one for Nq != Nk, :176-190;
`causal=True` is the same mask without materialising it) — and `block_sparse_mask[i, j] == 0` skips tile (i, j) of
`block_size` x `block_size` (Algorithm 5).  `window_size=(left, right)` is a sliding window (local attention, FlashAttention-2's
argument) in the causal flag's coordinates: key j is visible to query i only if i + Nk - Nq - left <= j <= i + Nk - Nq + right,
-1 = unbounded on that side; `causal=True, window_size=(left, -1)` is the usual causal local attention.  It composes with every
other argument (GQA K/V included), and the kernels visit only the tiles of each row's band (fa_ex_forward_window); a window
that bounds nothing is the call without one, bit for bit.  `softcap` > 0 (Gemma-2 style) replaces each score s = scale q.k by
softcap * tanh(s / softcap), and `alibi_slopes` (float32 (H,) or (B, H) for 4-D q, (BH,) for 3-D q; BLOOM / MPT style) then
subtracts slope * |i + Nk - Nq - j|, FlashAttention-2's arguments of the same names; the slopes get no gradient
(fa_ex_forward_scoremod).  softcap = 0 without slopes is the call without them, bit for bit.  `sinks` (float32 (H,) for 4-D q,
(sink_heads,) with sink_heads dividing BH for 3-D q: unit u takes sinks[u % sink_heads]) are attention sinks (gpt-oss): one learnable
logit per head that joins each row's softmax as an extra column with a zero value vector, in the units of the final logit, never
capped, biased, masked or dropped; -inf switches a head's sink off.  `sinks` receives a float32 gradient (a bf16 parameter is passed
as `p.float()` and gets its gradient through the cast).  Differentiable (autograd Function; the backward recomputes P and
regenerates the dropout mask from the seed).  No CPU path: the tensors must live on the GPU.

`return_lse=True` (keyword-only, and `sinks` with it now: sinks stays the last parameter, so both are passed by name) returns (o, lse): lse is the natural-log normaliser of each row, float32 (B, H, Nq) for 4-D q and
(BH, Nq) for 3-D q, -inf for a row without a visible key (and without a sink), and it is differentiable: a gradient of lse enters
the backward as one more row constant (fa_ex_backward_dlse).  o has the bits of the call without the keyword, and while lse
receives no gradient so have dq, dk, dv and dsinks.  (o, lse) pairs over disjoint key sets are combined by
common.merge_states.merge_attention_states; chained through autograd that gives the gradients of the one call over all the keys.

Chunking the keys of one call.  `causal` is aligned bottom-right (row i sees keys j <= i + Nk - Nq), so a chunk keys[j0:j1] of a
causal call over Nk keys is NOT a causal call on the chunk.  It is `causal=False, window_size=(left, Nk - j1)` on the chunk, where
`left` is the full call's left bound moved with the chunk (-1 if it had none: left' = left - (Nk - j1) where that is >= 0, and a
chunk wholly left of the band is not called at all): the chunk's last key j1 - 1 then sits Nk - j1 to the right of where the
full call's diagonal ends.  The last chunk (j1 = Nk) is plain `causal=True`.  Rows that see no key of a chunk come back with o = 0
and lse = -inf, which the merge treats as weight 0.  With `sinks`, pass them to exactly one chunk (the sink is one more column of
the union).  `mask` and `block_sparse_mask` are sliced with the keys.  ALiBi across chunks is not expressible (the bias of a chunk
would need the chunk's offset, which the call does not take) and is out of scope; dropout draws a different mask per chunk.

A v of its own width (fa_ex_forward_vdim / fa_ex_backward_vdim; flash_attention_varlen takes v (total_k, H_kv, d_v) alike).  Before
weight absorption, in training and prefill, DeepSeek-style multi-head latent attention is ordinary attention whose q and k are 192
wide (128 nope + 64 rope) and whose v and o are 128 wide.  v (..., d_v) with 8 <= d_v < d <= 192, d_v <= 128, both multiples of 8,
float16 / bfloat16: o (and dO) are d_v wide, dv comes back in v's shape, and the default scale stays d ** -0.5 with q's width d
(FlashAttention's rule: 192 ** -0.5 for MLA).  It goes with causal (bottom-right aligned for Nq != Nk), softmax_scale / tau, GQA,
return_lse with a differentiable lse, and packed sequences; mask, block_sparse_mask, dropout_p > 0, window_size, softcap,
alibi_slopes, sinks (and block_table, k_descale / v_descale of flash_attention_varlen) raise NotImplementedError naming the
argument, as do d_v > d, wider tensors and float32.  d_v == d is the call it always was.  Strides: flash_attention_ex copies a
non-contiguous k or v (.contiguous()), so a v sliced out of a (.., 128 + 128) kv projection costs one copy of v; the packed call
takes token-strided views without a copy but wants the heads of v adjacent at stride d_v, as it wants k's at d, and raises
RuntimeError otherwise.  Chunked MLA prefill composes with merge_attention_states exactly as above: o, lse pairs of key chunks
merge at any width.
"""
from __future__ import annotations

import math
import operator

import torch


def look_ahead_mask(q_len, k_len=None, device=None):
    """True = allowed: key j visible to query i iff j <= i + (k_len - q_len) (flashattention_pytorch.py:176-190)."""
    k_len = q_len if k_len is None else k_len
    qi = torch.arange(q_len, device=device).unsqueeze(1)
    kj = torch.arange(k_len, device=device).unsqueeze(0)
    return (kj <= qi + (k_len - q_len)).unsqueeze(0).unsqueeze(0)


def normalize_mask(mask, lead, nq, nk):
    """The model's `mask` (True / non-zero = allowed), "broadcastable to (B, H, Nq, Nk)" as the reference uses it
    (`scores.masked_fill(mask[:, :, i0:i1, j0:j1] == 0, -inf)`, flashattention_pytorch.py:139-141: ordinary broadcasting against
    the (B, H, Br, Bc) scores), in one of the two forms the library takes: (Nq, Nk) when every leading dim is 1 — one mask
    shared by all (b,h) — else (BH, Nq, Nk).  `lead` = q's leading dims, (B, H) or (BH,).  A key-padding mask (B, 1, 1, Nk)
    or (1, 1, 1, Nk) is expanded over the query rows like any other broadcast dim."""
    m = mask != 0
    if m.dim() > len(lead) + 2:
        if all(s == 1 for s in m.shape[: m.dim() - 2]):
            m = m.reshape(m.shape[-2:])
        elif len(lead) == 1 and math.prod(m.shape[:-2]) == lead[0]:
            m = m.reshape(lead[0], *m.shape[-2:])      # a (B, H, ., .) mask with already merged (BH, N, d) tensors
        else:
            raise RuntimeError(f"mask of shape {tuple(mask.shape)} does not broadcast to {(*lead, nq, nk)}")
    while m.dim() < len(lead) + 2:
        m = m.unsqueeze(0)
    shared = all(s == 1 for s in m.shape[:-2])
    try:
        m = torch.broadcast_to(m, ((1,) * len(lead) if shared else lead) + (nq, nk))
    except RuntimeError as exc:
        raise RuntimeError(f"mask of shape {tuple(mask.shape)} does not broadcast to {(*lead, nq, nk)}") from exc
    return m.reshape(nq, nk) if shared else m.reshape(-1, nq, nk)


class _FlashAttnExFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, mask, block_mask, br, bc, dropout_p, seed, window, softcap=0.0, alibi_slopes=None,
                sinks=None):
        import flashattention_lab_cuda as ext

        ctx.args = (causal, scale, mask, block_mask, br, bc, dropout_p, seed, window, softcap, alibi_slopes)
        ctx.with_sinks = sinks is not None
        if sinks is not None:
            o, lse = ext.ex_forward(q, k, v, causal, scale, mask, block_mask, br, bc, dropout_p, seed, window=window, softcap=softcap,
                                    alibi_slopes=alibi_slopes, sinks=sinks)
            ctx.save_for_backward(q, k, v, o, lse, sinks)
            return o
        o, lse = ext.ex_forward(q, k, v, causal, scale, mask, block_mask, br, bc, dropout_p, seed, window=window, softcap=softcap,
                                alibi_slopes=alibi_slopes)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        import flashattention_lab_cuda as ext

        causal, scale, mask, block_mask, br, bc, dropout_p, seed, window, softcap, alibi_slopes = ctx.args
        if ctx.with_sinks:
            q, k, v, o, lse, sinks = ctx.saved_tensors
            dq, dk, dv, dsinks = ext.ex_backward(q, k, v, o, do.contiguous(), lse, causal, scale, mask, block_mask, br, bc, dropout_p,
                                                 seed, window=window, softcap=softcap, alibi_slopes=alibi_slopes, sinks=sinks)
            return (dq, dk, dv) + (None,) * 11 + (dsinks,)
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = ext.ex_backward(q, k, v, o, do.contiguous(), lse, causal, scale, mask, block_mask, br, bc, dropout_p, seed,
                                     window=window, softcap=softcap, alibi_slopes=alibi_slopes)
        return (dq, dk, dv) + (None,) * 11   # (no gradient for the slopes, as in FlashAttention-2)


class _FlashAttnExLseFn(torch.autograd.Function):
    """_FlashAttnExFn that also returns lse (flash_attention_ex(..., return_lse=True)).  A gradient of lse goes to the library as
    dlse; without one the backward is _FlashAttnExFn's call, launch for launch."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, mask, block_mask, br, bc, dropout_p, seed, window, softcap, alibi_slopes, sinks):
        import flashattention_lab_cuda as ext

        ctx.set_materialize_grads(False)
        ctx.args = (causal, scale, mask, block_mask, br, bc, dropout_p, seed, window, softcap, alibi_slopes)
        ctx.with_sinks = sinks is not None
        kw = {"sinks": sinks} if sinks is not None else {}
        o, lse = ext.ex_forward(q, k, v, causal, scale, mask, block_mask, br, bc, dropout_p, seed, window=window, softcap=softcap,
                                alibi_slopes=alibi_slopes, **kw)
        ctx.save_for_backward(q, k, v, o, lse, *kw.values())
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        import flashattention_lab_cuda as ext

        if do is None and dlse is None:
            return (None,) * 15
        causal, scale, mask, block_mask, br, bc, dropout_p, seed, window, softcap, alibi_slopes = ctx.args
        q, k, v, o, lse = ctx.saved_tensors[:5]
        do = torch.zeros_like(o) if do is None else do.contiguous()
        kw = {"sinks": ctx.saved_tensors[5]} if ctx.with_sinks else {}
        if dlse is not None:
            kw["dlse"] = dlse.contiguous()
        grads = ext.ex_backward(q, k, v, o, do, lse, causal, scale, mask, block_mask, br, bc, dropout_p, seed, window=window,
                                softcap=softcap, alibi_slopes=alibi_slopes, **kw)
        return tuple(grads[:3]) + (None,) * 11 + ((grads[3],) if ctx.with_sinks else (None,))


class _FlashAttnExBiasFn(torch.autograd.Function):
    """flash_attention_ex(..., attn_bias=) (fa_ex_forward_bias / fa_ex_backward_bias): a Function of its own, so the calls without a
    bias stay launch for launch what they were.  With_lse: (o, lse) and a gradient of lse; dbias only where the bias requires grad."""

    @staticmethod
    def forward(ctx, q, k, v, bias, causal, scale, with_lse):
        import flashattention_lab_cuda as ext

        ctx.set_materialize_grads(False)
        ctx.args = (causal, scale)
        o, lse = ext.ex_forward(q, k, v, causal, scale, attn_bias=bias)
        ctx.save_for_backward(q, k, v, o, lse, bias)
        if with_lse:
            return o, lse
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        import flashattention_lab_cuda as ext

        if do is None and dlse is None:
            return (None,) * 7
        causal, scale = ctx.args
        q, k, v, o, lse, bias = ctx.saved_tensors
        do = torch.zeros_like(o) if do is None else do.contiguous()
        kw = {"dlse": dlse.contiguous()} if dlse is not None else {}
        need = bool(ctx.needs_input_grad[3])
        grads = ext.ex_backward(q, k, v, o, do, lse, causal, scale, attn_bias=bias, need_dbias=need, **kw)
        return tuple(grads[:3]) + (grads[3] if need else None,) + (None,) * 3


def _bias_units(who, bias, lead, nq, nk):
    """attn_bias for a 4-D q ((B, H) = lead): (Bb, Hb, Rb, Nk) with Bb in {1, B}, Hb in {1, H}, Rb in {1, Nq}; for a 3-D q
    (BH or 1, Rb, Nk).  The library checks the rest (dtype, device, layout: flashattention_lab_cuda.bias_arg)."""
    if not isinstance(bias, torch.Tensor):
        raise RuntimeError(f"{who}: attn_bias must be a tensor of q's dtype")
    shape = tuple(bias.shape)
    if len(lead) == 2:
        want = f"(1 or {lead[0]}, 1 or {lead[1]}, 1 or {nq}, {nk})"
        ok = bias.dim() == 4 and shape[0] in (1, lead[0]) and shape[1] in (1, lead[1]) and shape[2] in (1, nq) and shape[3] == nk
    else:
        want = f"(1 or {lead[0]}, 1 or {nq}, {nk})"
        ok = bias.dim() == 3 and shape[0] in (1, lead[0]) and shape[1] in (1, nq) and shape[2] == nk
    if not ok:
        raise RuntimeError(f"{who}: attn_bias must be {want}, got {shape}")
    return bias


def _window_size(window_size):
    """(left, right) ints >= -1, with the library's error text (flashattention_lab_cuda.window_arg, fa_capi.hip)."""
    try:
        left, right = window_size
        if isinstance(left, bool) or isinstance(right, bool):
            raise TypeError
        left, right = operator.index(left), operator.index(right)
    except (TypeError, ValueError):
        raise RuntimeError(f"flash_attention_ex: window_size must be a pair (left, right) of ints, got {window_size!r}") from None
    if left < -1 or right < -1:
        raise RuntimeError(f"flash_attention_ex: window ({left}, {right}): each bound must be >= 0, or -1 for unbounded")
    return left, right


def _alibi_units(slopes, lead):
    """4-D q (lead = (B, H)): FlashAttention-2's (H,) slopes as a (B, H) view with row stride 0 (no copy); the library checks
    the rest (dtype, device, shape, layout: flashattention_lab_cuda.alibi_arg)."""
    if slopes is None or len(lead) != 2 or not isinstance(slopes, torch.Tensor):
        return slopes
    if slopes.dim() == 1 and slopes.shape[0] == lead[1] and slopes.is_contiguous():
        return slopes.detach().unsqueeze(0).expand(lead[0], lead[1])
    if slopes.dim() == 2 and tuple(slopes.shape) == tuple(lead):
        return slopes.detach()
    raise RuntimeError(f"flash_attention_ex: alibi_slopes must be ({lead[1]},) or {tuple(lead)}, got {tuple(slopes.shape)}")


def _sinks_units(who, sinks, heads):
    """`sinks` for a call whose query heads are known (4-D q, varlen): float32 (heads,); the library checks the rest."""
    if not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32:
        raise RuntimeError(f"{who}: sinks must be a float32 tensor (pass a 16-bit parameter as p.float())")
    if tuple(sinks.shape) != (heads,):
        raise RuntimeError(f"{who}: sinks must be ({heads},), got {tuple(sinks.shape)}")
    return sinks.contiguous()


def flash_attention_ex(q, k, v, tau=1.0, mask=None, block_sparse_mask=None, block_size=128, causal=False, dropout_p=0.0,
                       seed=0, softmax_scale=None, window_size=(-1, -1), softcap=0.0, alibi_slopes=None, *, return_lse=False,
                       attn_bias=None, sinks=None):
    window = _window_size(window_size)
    if attn_bias is not None:
        # an additive bias: what the bias kernels do not take is refused by name, before anything runs
        import flashattention_lab_cuda as ext

        ext.bias_refuse("flash_attention_ex", mask=mask is not None, block_sparse_mask=block_sparse_mask is not None,
                        dropout_p=float(dropout_p) > 0.0, window_size=window != (-1, -1), softcap=softcap != 0.0,
                        alibi_slopes=alibi_slopes is not None, sinks=sinks is not None,
                        **{"d_v != d": isinstance(v, torch.Tensor) and isinstance(k, torch.Tensor) and v.shape[-1] != k.shape[-1]})
    if all(isinstance(t, torch.Tensor) for t in (q, k, v)) and k.dim() == v.dim() and v.shape[:-1] == k.shape[:-1] and v.shape[-1] != k.shape[-1]:
        # a v of its own width: what the two-width kernels do not take is refused by name, before anything runs
        _vdim_refuse("flash_attention_ex", k.shape[-1], v.shape[-1], q.dtype, mask=mask is not None,
                     block_sparse_mask=block_sparse_mask is not None, dropout_p=float(dropout_p) > 0.0, window_size=window != (-1, -1),
                     softcap=softcap != 0.0, alibi_slopes=alibi_slopes is not None, sinks=sinks is not None)
    if not q.is_cuda:
        raise RuntimeError("Inputs must be CUDA tensors")   # as the reference's wrappers (src/fa2/cuda/impl.py:44)
    four_d = q.dim() == 4
    if four_d:
        b, h, nq, d = q.shape
        if k.dim() != 4 or k.shape[0] != b or v.dim() != 4 or v.shape[:3] != k.shape[:3]:
            raise RuntimeError(f"k must be (B, H_kv, Nk, d) with q's B and v (B, H_kv, Nk, d_v); got {tuple(k.shape)}, {tuple(v.shape)}")
        hkv, nk = k.shape[1], k.shape[2]
        if hkv == 0 or h % hkv != 0:
            raise RuntimeError(f"the query heads ({h}) must be a multiple of the K/V heads ({hkv})")
        q3, k3, v3 = q.reshape(b * h, nq, d), k.reshape(b * hkv, nk, d), v.reshape(b * hkv, nk, v.shape[3])
    else:
        q3, k3, v3 = q, k, v
        (_, nq, d), nk = q.shape, k.shape[1]
    d_v = v.shape[-1]
    scale = (tau / math.sqrt(d)) if softmax_scale is None else float(softmax_scale) * tau   # :134
    if attn_bias is not None:
        bias = _bias_units("flash_attention_ex", attn_bias, tuple(q.shape[:-2]), nq, nk)
        o, lse = _FlashAttnExBiasFn.apply(q3, k3, v3, bias, bool(causal), scale, bool(return_lse))
        if four_d:
            o, lse = o.reshape(b, h, nq, d_v), lse.reshape(b, h, nq)
        return (o, lse) if return_lse else o
    m = None
    if mask is not None:
        m = normalize_mask(mask, tuple(q.shape[:-2]), nq, nk)
    br = bc = int(block_size)
    if block_sparse_mask is not None:
        br, bc = min(br, nq), min(bc, nk)         # Br = min(block_size, q_len), Bc = min(block_size, kv_len)  (:100-101)
    slopes = _alibi_units(alibi_slopes, tuple(q.shape[:-2]))
    if return_lse:
        if sinks is not None:
            if four_d:
                sinks = _sinks_units("flash_attention_ex", sinks, h)
            elif not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32:
                raise RuntimeError("flash_attention_ex: sinks must be a float32 tensor (pass a 16-bit parameter as p.float())")
        o, lse = _FlashAttnExLseFn.apply(q3, k3, v3, bool(causal), scale, m, block_sparse_mask, br, bc, float(dropout_p), int(seed),
                                         window, softcap, slopes, sinks)
        return (o.reshape(b, h, nq, d_v), lse.reshape(b, h, nq)) if four_d else (o, lse)
    if sinks is not None:
        if four_d:
            sinks = _sinks_units("flash_attention_ex", sinks, h)
        elif not isinstance(sinks, torch.Tensor) or sinks.dtype != torch.float32:
            raise RuntimeError("flash_attention_ex: sinks must be a float32 tensor (pass a 16-bit parameter as p.float())")
        o = _FlashAttnExFn.apply(q3, k3, v3, bool(causal), scale, m, block_sparse_mask, br, bc, float(dropout_p), int(seed), window,
                                 softcap, slopes, sinks)
    elif softcap == 0.0 and slopes is None:   # (the call without modifiers, as before they existed)
        o = _FlashAttnExFn.apply(q3, k3, v3, bool(causal), scale, m, block_sparse_mask, br, bc, float(dropout_p), int(seed), window)
    else:
        o = _FlashAttnExFn.apply(q3, k3, v3, bool(causal), scale, m, block_sparse_mask, br, bc, float(dropout_p), int(seed), window,
                                 softcap, slopes)
    return o.reshape(b, h, nq, d_v) if four_d else o


def _vdim_refuse(who, d, d_v, dtype, **carried):
    """the rules of a v of its own width (flashattention_lab_cuda.vdim_arg), under this module's argument names"""
    import flashattention_lab_cuda as ext

    ext.vdim_arg(who, d, d_v, dtype, **carried)


class _FlashAttnVarlenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q, max_k, dropout_p, scale, causal, window, seed, softcap=0.0, alibi_slopes=None,
                sinks=None):
        import flashattention_lab_cuda as ext

        ctx.with_sinks = sinks is not None
        if sinks is not None:
            o, lse = ext.ex_varlen_forward(q, k, v, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed, window=window,
                                           softcap=softcap, alibi_slopes=alibi_slopes, sinks=sinks)
            ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k, sinks)
            ctx.args = (max_q, max_k, dropout_p, scale, causal, window, seed, softcap, alibi_slopes)
            return o
        o, lse = ext.ex_varlen_forward(q, k, v, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed, window=window, softcap=softcap,
                                       alibi_slopes=alibi_slopes)
        ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
        ctx.args = (max_q, max_k, dropout_p, scale, causal, window, seed, softcap, alibi_slopes)
        return o

    @staticmethod
    def backward(ctx, do):
        import flashattention_lab_cuda as ext

        max_q, max_k, dropout_p, scale, causal, window, seed, softcap, alibi_slopes = ctx.args
        if ctx.with_sinks:
            q, k, v, o, lse, cu_q, cu_k, sinks = ctx.saved_tensors
            dq, dk, dv, dsinks = ext.ex_varlen_backward(q, k, v, o, do.contiguous(), lse, cu_q, cu_k, max_q, max_k, causal, scale,
                                                        dropout_p, seed, window=window, softcap=softcap, alibi_slopes=alibi_slopes,
                                                        sinks=sinks)
            return (dq, dk, dv) + (None,) * 11 + (dsinks,)
        q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
        dq, dk, dv = ext.ex_varlen_backward(q, k, v, o, do.contiguous(), lse, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed,
                                            window=window, softcap=softcap, alibi_slopes=alibi_slopes)
        return (dq, dk, dv) + (None,) * 11


class _FlashAttnVarlenLseFn(torch.autograd.Function):
    """_FlashAttnVarlenFn that also returns lse (flash_attention_varlen(..., return_softmax_lse=True)), as _FlashAttnExLseFn"""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q, max_k, dropout_p, scale, causal, window, seed, softcap, alibi_slopes, sinks):
        import flashattention_lab_cuda as ext

        ctx.set_materialize_grads(False)
        ctx.with_sinks = sinks is not None
        kw = {"sinks": sinks} if sinks is not None else {}
        o, lse = ext.ex_varlen_forward(q, k, v, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed, window=window, softcap=softcap,
                                       alibi_slopes=alibi_slopes, **kw)
        ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k, *kw.values())
        ctx.args = (max_q, max_k, dropout_p, scale, causal, window, seed, softcap, alibi_slopes)
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        import flashattention_lab_cuda as ext

        if do is None and dlse is None:
            return (None,) * 15
        max_q, max_k, dropout_p, scale, causal, window, seed, softcap, alibi_slopes = ctx.args
        q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors[:7]
        do = torch.zeros_like(o) if do is None else do.contiguous()
        kw = {"sinks": ctx.saved_tensors[7]} if ctx.with_sinks else {}
        if dlse is not None:
            kw["dlse"] = dlse.contiguous()
        grads = ext.ex_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, causal, scale, dropout_p, seed, window=window,
                                       softcap=softcap, alibi_slopes=alibi_slopes, **kw)
        return tuple(grads[:3]) + (None,) * 11 + ((grads[3],) if ctx.with_sinks else (None,))


def flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0, softmax_scale=None,
                           causal=False, window_size=(-1, -1), seed=0, softcap=0.0, alibi_slopes=None, *,
                           return_softmax_lse=False, block_table=None, k_descale=None, v_descale=None, sinks=None):
    """FlashAttention-2's flash_attn_varlen_func over packed sequences, differentiable: q (total_q, H_q, d), k and v
    (total_k, H_kv, d) — v may be narrower, (total_k, H_kv, d_v): "A v of its own width" in this module's docstring; o is then
    (total_q, H_q, d_v) — with H_q % H_kv == 0 (GQA), token-strided views (qkv.unbind(1) of a (total, 3, H, d) projection) taken
    without a copy; cu_seqlens_* int32 (batch + 1,) device offsets.  Attention stays inside each sequence; `causal` is
    bottom-right aligned per sequence and `window_size` has flash_attention_ex's meaning in each sequence's coordinates.
    Returns o (total_q, H_q, d); the gradients of k and v come back in their shapes.  The dropout mask is that of the padded
    (batch * H_q, max_seqlen_q, max_seqlen_k) call (include/fa_mi355x.h), so it depends on the max_seqlen_q passed.  softcap and
    alibi_slopes (float32 (H_q,) or (batch, H_q)) as in flash_attention_ex, in each sequence's coordinates.  sinks: float32 (H_q,)
    attention sinks as in flash_attention_ex, differentiable.
    block_table (keyword-only, and `sinks` with it: sinks stays the last parameter, so both are passed by name;
    FlashAttention-2's argument of flash_attn_varlen_func): int32 (batch, max_blocks_per_seq) on the
    device — k and v are then the pools of a paged KV cache, (num_blocks, page_block_size, H_kv, d) in q's dtype, page_block_size
    a positive multiple of 16, and key t of sequence b lives at pool[block_table[b, t // ps], t % ps]: chunked prefill, or prefill
    behind a shared prefix, straight from the cache flash_attn_with_kvcache appends to.  The lengths still come from
    cu_seqlens_k — len_k[b] = cu_seqlens_k[b + 1] - cu_seqlens_k[b], its absolute offsets mean nothing for a pool — clamped on
    the device to [0, min(max_seqlen_k, max_blocks_per_seq * ps)]; nothing is read on the host, so the call never synchronises
    and can be captured and replayed with a changed table and changed offsets.  The table is untrusted: a page number outside
    [0, num_blocks) reads as zero K and zero V, entries past ceil(len_k[b] / ps) are never read, page offsets are 64-bit (pools
    above 4 GiB), sequences may share pages, and the pools are only read.  A pool may be a view with its own page and token
    strides (the two halves of a K|V-interleaved allocation, a slice of the heads); the elements of a head must be contiguous,
    and a view the library cannot take without a copy raises ValueError.  causal, window_size, GQA, softcap, alibi_slopes,
    sinks, a token-strided q and empty sequences work as without the table, and each sequence gets the bits of this function on
    the same tokens gathered into packed k, v.  Forward only: dropout_p > 0 raises ValueError, and q, k or v requiring grad
    under grad mode raises RuntimeError (no paged backward, as in FlashAttention-2).  A block_table that is not an int32
    tensor raises NotImplementedError.
    k_descale, v_descale (keyword-only, with block_table): the pools may both be torch.float8_e4m3fn (OCP e4m3), the cache that
    flash_attn_with_kvcache appends to and decodes from, while q and o stay float16 / bfloat16.  A stored byte c of K head h of
    sequence b (of this call, not of the page) stands for e4m3(c) * k_descale[b, h], for V with v_descale: float32 (batch, H_kv) or
    (H_kv,) on the device, read by the kernels only, None = 1.0 — the same sentences as the decode call's, so one cache serves
    append, decode and prefill.  Widening e4m3 to q's dtype is exact and the 16-bit kernel is kept: the score is softmax_scale *
    k_descale * (q . k_stored), scaled before softcap and ALiBi, v_descale multiplies the normalised output once in fp32, and
    everything above about the table, the views, the lengths and graph replay (changed scale values included) holds unchanged.
    Give both scales in the same form: with one (H_kv,) and one (batch, H_kv) the former is first copied into (batch, H_kv) rows,
    one more small kernel per call.  Other float8 dtypes raise NotImplementedError; scales without e4m3 pools, and e4m3 pools without block_table, RuntimeError.
    return_softmax_lse (keyword-only; FlashAttention-2's name): return (o, lse), lse float32 (H_q, total_q), the natural-log
    normaliser of each token and head, -inf for a row without a visible key; tokens no sequence owns hold unspecified values.  lse
    is differentiable (fa_ex_backward_varlen_dlse); with block_table it is returned without a gradient, that path being forward only.
    o has the bits of the call without the keyword, and so have the gradients while lse receives none.  (o, lse) pairs over
    disjoint key sets merge with common.merge_states.merge_attention_states(..., layout="thd").  Chunking keys under `causal`:
    per sequence the rule of flash_attention_ex's docstring — the chunk keys[j0:j1] of a sequence's Nk keys is causal=False,
    window_size=(left', Nk - j1), the last chunk plain causal=True — which one call can express only where Nk - j1 is the same
    for every sequence; sinks go to exactly one chunk; ALiBi across chunks is not expressible and out of scope."""
    window = _window_size(window_size)
    if all(isinstance(t, torch.Tensor) for t in (q, k, v)) and k.dim() == v.dim() and v.shape[:-1] == k.shape[:-1] and v.shape[-1] != k.shape[-1]:
        _vdim_refuse("flash_attention_varlen", k.shape[-1], v.shape[-1], q.dtype, dropout_p=float(dropout_p) > 0.0,
                     window_size=window != (-1, -1), softcap=softcap != 0.0, alibi_slopes=alibi_slopes is not None,
                     sinks=sinks is not None, block_table=block_table is not None, k_descale=k_descale is not None,
                     v_descale=v_descale is not None)
    if block_table is not None:
        return _flash_attention_varlen_paged(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale,
                                             causal, window, softcap, alibi_slopes, sinks, block_table, k_descale, v_descale,
                                             return_softmax_lse)
    _no_fp8_without_table("flash_attention_varlen", k, v, k_descale, v_descale)
    if not q.is_cuda:
        raise RuntimeError("Inputs must be CUDA tensors")
    scale = (1.0 / math.sqrt(q.shape[-1])) if softmax_scale is None else float(softmax_scale)
    args = (q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), float(dropout_p), scale, bool(causal), window,
            int(seed))
    if return_softmax_lse:
        if isinstance(alibi_slopes, torch.Tensor):
            alibi_slopes = alibi_slopes.detach()
        if sinks is not None:
            sinks = _sinks_units("flash_attention_varlen", sinks, q.shape[1])
        return _FlashAttnVarlenLseFn.apply(*args, softcap, alibi_slopes, sinks)
    if softcap == 0.0 and alibi_slopes is None and sinks is None:
        return _FlashAttnVarlenFn.apply(*args)
    if isinstance(alibi_slopes, torch.Tensor):
        alibi_slopes = alibi_slopes.detach()
    if sinks is None:
        return _FlashAttnVarlenFn.apply(*args, softcap, alibi_slopes)
    return _FlashAttnVarlenFn.apply(*args, softcap, alibi_slopes, _sinks_units("flash_attention_varlen", sinks, q.shape[1]))


def _flash_attention_varlen_paged(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, causal,
                                  window, softcap, alibi_slopes, sinks, block_table, k_descale=None, v_descale=None,
                                  return_softmax_lse=False):
    """flash_attention_varlen with a block_table: forward only, nothing differentiable"""
    who = "flash_attention_varlen"
    if not (isinstance(block_table, torch.Tensor) and block_table.dtype == torch.int32):
        dt = block_table.dtype if isinstance(block_table, torch.Tensor) else type(block_table).__name__
        raise NotImplementedError(f"{who}: block_table of dtype {dt} is not supported (int32 tensor expected)")
    if float(dropout_p) > 0.0:
        raise ValueError(f"{who}: dropout_p > 0 is not supported with block_table (an inference path)")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (q, k, v)):
        raise RuntimeError(f"{who}: block_table is forward only — q, k or v requires grad and there is no backward through a paged "
                           f"cache (call it under torch.no_grad(), or detach the tensors)")
    if not q.is_cuda:
        raise RuntimeError("Inputs must be CUDA tensors")
    import flashattention_lab_cuda as ext

    scale = (1.0 / math.sqrt(q.shape[-1])) if softmax_scale is None else float(softmax_scale)
    if isinstance(alibi_slopes, torch.Tensor):
        alibi_slopes = alibi_slopes.detach()
    if sinks is not None:
        sinks = _sinks_units(who, sinks, q.shape[1]).detach()
    with torch.no_grad():
        o, lse = ext.ex_varlen_forward(q.detach(), k.detach(), v.detach(), cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q),
                                       int(max_seqlen_k), bool(causal), scale, 0.0, 0, window=window, softcap=softcap,
                                       alibi_slopes=alibi_slopes, sinks=sinks, block_table=block_table, k_descale=k_descale,
                                       v_descale=v_descale)
    return (o, lse) if return_softmax_lse else o


def _no_fp8_without_table(who, k, v, k_descale, v_descale):
    """the packed (non-paged) call has no 8-bit K/V: float8 tensors and scales are refused before anything runs"""
    f8 = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz") if hasattr(torch, n))
    for name, t in (("k", k), ("v", v)):
        if isinstance(t, torch.Tensor) and t.dtype in f8:
            if t.dtype != torch.float8_e4m3fn:
                raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (an 8-bit cache is torch.float8_e4m3fn)")
            raise RuntimeError(f"{who}: torch.float8_e4m3fn k, v are pools of a paged cache and need block_table")
    if k_descale is not None or v_descale is not None:
        raise RuntimeError(f"{who}: k_descale / v_descale need torch.float8_e4m3fn pools and block_table")


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, rotary_cos=None, rotary_sin=None, cache_seqlens=None,
                            cache_batch_idx=None, cache_leftpad=None, block_table=None, softmax_scale=None, causal=False,
                            window_size=(-1, -1), softcap=0.0, rotary_interleaved=True, alibi_slopes=None, num_splits=0,
                            return_softmax_lse=False, *, cu_seqlens_q=None, cu_seqlens_k_new=None, max_seqlen_q=None, qv=None,
                            sinks=None, k_descale=None, v_descale=None):
    """FlashAttention-2's flash_attn_with_kvcache (forward; its argument order): q (B, Nq, H_q, d); k_cache, v_cache
    (B, cache_len, H_kv, d) with H_q % H_kv == 0, updated in place — k, v (B, N_new, H_kv, d) are written at
    cache_seqlens[b] .. + N_new before attention, and a cache view the library cannot take without a copy raises ValueError.
    cache_seqlens: int32 (B,) device lengths, or an int; None means every sequence fills the cache (no k, v then).  Queries
    attend over keys [0, cache_seqlens[b] + N_new) with causal bottom-right aligned, window_size, softcap and alibi_slopes
    (float32 (H_q,) or (B, H_q)) as in flash_attention_ex.  num_splits = 0 lets the library split the keys over workgroups.
    block_table: int32 (B, max_blocks_per_seq) on the device — k_cache, v_cache are then pools (num_blocks, page_block_size,
    H_kv, d), page_block_size a multiple of 16, and token t of sequence b lives at pool[block_table[b, t // ps], t % ps]; a page
    number outside the pool reads as zeros and drops the append.  cache_batch_idx: int32 (B,), sequence b uses cache row
    idx[b] (the cache's batch dim may differ from B).  cache_leftpad: int32 (B,), the keys of sequence b start at cache position
    leftpad[b] while cache_seqlens keeps counting from 0.  The last two combine; neither goes with block_table.
    rotary_cos, rotary_sin: (seqlen_ro, rotary_dim / 2) in q's dtype on the device, rotary_dim a multiple of 16 up to d; needs k, v
    and cache_seqlens.  k is rotated at its position in the sequence (cache_seqlens[b] - leftpad[b] + n) before it is written to
    the cache; q at the position of its token when causal or a window bound is given, else every q token at the position of
    the first new token; q itself is not modified.  rotary_interleaved: pairs (2j, 2j + 1), else (j, j + rotary_dim / 2).
    seqlen_ro must be at least the capacity (cache_len, or max_blocks_per_seq * page_block_size) + max(0, Nq - N_new).
    k_descale, v_descale (FlashAttention-3's): k_cache and v_cache may both be torch.float8_e4m3fn, half the bytes of a 16-bit
    cache, with float32 dequantisation scales of shape (B, H_kv) or (H_kv,) on the device (None: 1.0; finite and > 0): a stored
    value c of K head h of sequence b stands for c * k_descale[b, h].  q, k, v and the result stay 16-bit; k and v are quantised
    as they are appended (after the rotation), with saturation at +-448.  Other 8-bit dtypes raise NotImplementedError.
    sinks (keyword-only, as k_descale and v_descale now are: FlashAttention-2's positional order ends before them): float32 (H_q,) attention sinks on q's device, one extra softmax column per query head with a zero value
    (flash_attention_ex); the returned lse contains it, and a sequence without any key gives o = 0, lse = sink.
    cu_seqlens_q, cu_seqlens_k_new, max_seqlen_q (keyword-only; FlashAttention-3's): one call for sequences that bring different
    numbers of tokens, a continuous-batching step.  With cu_seqlens_q (int32 (B + 1,) on the device) and max_seqlen_q (an int)
    q is packed (total_q, H_q, d) — a token-strided view such as qkv[:, 0] is used without a copy — and sequence b owns tokens
    [cu_seqlens_q[b], cu_seqlens_q[b + 1]), at most max_seqlen_q, none allowed.  With cu_seqlens_k_new (int32 (B + 1,); needs k,
    v and cu_seqlens_q) k and v are packed (total_k_new, H_kv, d) and sequence b appends its own number of tokens; without it k,
    v stay (B, N_new, H_kv, d) or None.  Each sequence gets exactly what the padded call returns for it alone, with its own
    causal diagonal len_k_b - nq_b; one without q tokens still appends.  The arrays are never read on the host and may hold
    anything: the kernels clamp them to the tensors.  Rotary then needs seqlen_ro >= capacity + max_seqlen_q.  A 4-D q with
    cu_seqlens_q, a missing max_seqlen_q, or a packed q that would need a copy raises ValueError.  o is then (total_q, H_q, d) and
    lse (H_q, total_q).
    qv (keyword-only; FlashAttention-3's): a second query operand (B, Nq, H_q, 512) in q's dtype, for K and V of different widths —
    DeepSeek-style multi-head latent attention at decode time after weight absorption.  q and k_cache are then 64 wide (the
    rotary part), v_cache (.., H_kv, 512) holds the latent rows and o is (B, Nq, H_q, 512):
        s[i, j] = softmax_scale * (q[i, h] . k[j] + qv[i, h] . v[j]),   o[i, h] = sum_j softmax_j(s)[i, j] v[j]
    with softmax_scale defaulting to (64 + 512) ** -0.5.  Each latent row is read from memory once and serves the score and the
    value.  k_cache and v_cache may be views of one allocation (pool[..., 512:] and pool[..., :512] of a (.., 576) pool,
    contiguous or paged); their own strides are used, never a copy.  Goes with cache_seqlens, cache_batch_idx, block_table,
    causal, window_size, softmax_scale, num_splits and return_softmax_lse.  Other widths, k / v, cu_seqlens_k_new, rotary_cos /
    rotary_sin, an e4m3 cache (k_descale / v_descale), softcap, alibi_slopes, sinks, cu_seqlens_q and cache_leftpad raise
    NotImplementedError with the argument's name.
    Returns o (B, Nq, H_q, d), and with return_softmax_lse also lse (B, H_q, Nq) float32.  No gradient."""
    for name, val in (("block_table", block_table), ("cache_batch_idx", cache_batch_idx), ("cache_leftpad", cache_leftpad),
                      ("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k_new", cu_seqlens_k_new)):
        if val is not None and not (isinstance(val, torch.Tensor) and val.dtype == torch.int32):
            dt = val.dtype if isinstance(val, torch.Tensor) else type(val).__name__
            raise NotImplementedError(f"flash_attn_with_kvcache: {name} of dtype {dt} is not supported (int32 tensor expected)")
    for name, val in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if val is not None and not (isinstance(val, torch.Tensor) and val.dtype == q.dtype):
            dt = val.dtype if isinstance(val, torch.Tensor) else type(val).__name__
            raise NotImplementedError(f"flash_attn_with_kvcache: {name} of dtype {dt} is not supported (q's dtype expected)")
    for name, val in (("k_descale", k_descale), ("v_descale", v_descale)):
        if val is not None and not (isinstance(val, torch.Tensor) and val.dtype == torch.float32):
            dt = val.dtype if isinstance(val, torch.Tensor) else type(val).__name__
            raise NotImplementedError(f"flash_attn_with_kvcache: {name} of dtype {dt} is not supported (float32 tensor expected)")
    import flashattention_lab_cuda as ext

    if isinstance(alibi_slopes, torch.Tensor):
        alibi_slopes = alibi_slopes.detach()
    extra = {} if sinks is None else {"sinks": sinks.detach() if isinstance(sinks, torch.Tensor) else sinks}
    if cu_seqlens_q is not None or cu_seqlens_k_new is not None or max_seqlen_q is not None:
        extra.update(cu_seqlens_q=cu_seqlens_q, cu_seqlens_k_new=cu_seqlens_k_new, max_seqlen_q=max_seqlen_q)
    if qv is not None:
        if not isinstance(qv, torch.Tensor):
            raise NotImplementedError(f"flash_attn_with_kvcache: qv of type {type(qv).__name__} is not supported (a tensor of q's dtype expected)")
        extra.update(qv=qv.detach())
    with torch.no_grad():
        o, lse = ext.ex_kvcache_forward(q.detach(), k_cache, v_cache, None if k is None else k.detach(),
                                        None if v is None else v.detach(), cache_seqlens, bool(causal), softmax_scale,
                                        _window_size(window_size), softcap, alibi_slopes, num_splits, block_table, cache_batch_idx,
                                        cache_leftpad, None if rotary_cos is None else rotary_cos.detach(),
                                        None if rotary_sin is None else rotary_sin.detach(), bool(rotary_interleaved),
                                        k_descale=None if k_descale is None else k_descale.detach(),
                                        v_descale=None if v_descale is None else v_descale.detach(), **extra)
    return (o, lse) if return_softmax_lse else o


def flash_mla_sparse_attn(q, qv, k_cache, v_cache, indices, *, cache_seqlens=None, block_table=None, cache_batch_idx=None,
                          softmax_scale=None, causal=False, num_splits=0, return_softmax_lse=False):
    """Sparse multi-head latent attention at decode time (DeepSeek sparse attention): flash_attn_with_kvcache(..., qv=qv) over a
    per-query list of cached tokens instead of every token of the sequence.  q (B, Nq, H_q, 64), qv (B, Nq, H_q, 512), k_cache
    (.., H_kv, 64) and v_cache (.., H_kv, 512) exactly as that call takes them: contiguous (B, cache_len, H_kv, .) caches, rows
    picked by cache_batch_idx, or pools under block_table; views of one (.., 576) allocation are used with their own strides,
    never copied.  indices: int32 (B, Nq, topk), one list per query token for all K/V heads, or (B, Nq, H_kv, topk), on q's device,
    last dim contiguous.  An entry is a token position of sequence b; for query token i and head h reading K/V head h // G
        visible(j)  <=>  0 <= I[j] < len_b  and, if causal,  I[j] <= len_b - Nq + i           (len_b = cache_seqlens[b], clamped)
        s[j] = softmax_scale * (q[b, i, h] . k[I[j]] + qv[b, i, h] . v[I[j]]),    o[b, i, h] = sum_j softmax_j(s)[j] v[I[j]]
    over the visible j.  Every list position is a key (a token named twice counts twice); -1 padding and any entry outside the
    sequence are skipped and never read; a row without a visible entry gives o = 0, lse = -inf.  A visible entry on a page outside
    the pool reads as a zero key with a zero value (flash_attn_with_kvcache's rule).  cache_seqlens: int32 (B,) on the device, an int
    or None (the capacity).  softmax_scale defaults to (64 + 512) ** -0.5.  Nothing is read on the host: the call can be captured
    in a graph and replayed with changed indices, lengths and tables.  indices (block_table, cache_batch_idx) of another dtype
    raise NotImplementedError with the name; wrong shapes and devices RuntimeError.  No window, softcap, ALiBi, sinks, rotary, new
    tokens, e4m3 cache, packed queries or left padding.
    Returns o (B, Nq, H_q, 512), and with return_softmax_lse also lse (B, H_q, Nq) float32.  No gradient."""
    for name, val in (("indices", indices), ("block_table", block_table), ("cache_batch_idx", cache_batch_idx)):
        if (val is not None or name == "indices") and not (isinstance(val, torch.Tensor) and val.dtype == torch.int32):
            dt = val.dtype if isinstance(val, torch.Tensor) else type(val).__name__
            raise NotImplementedError(f"flash_mla_sparse_attn: {name} of dtype {dt} is not supported (int32 tensor expected)")
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.ex_mla_sparse_forward(q.detach(), qv.detach(), k_cache, v_cache, indices, cache_seqlens, bool(causal), softmax_scale,
                                           block_table, cache_batch_idx, num_splits)
    return (o, lse) if return_softmax_lse else o


def mla_fp8_pack_cache(latent_new, rope_new, kv_cache, cache_seqlens, block_table, *, scale_pow2=False):
    """Quantise new MLA tokens and append them to a packed 8-bit latent cache, in place: the write side of
    flash_mla_with_kvcache(..., is_fp8_kvcache=True).  latent_new (B, N_new, 512) and rope_new (B, N_new, 64) bfloat16 on the GPU
    (the two column ranges of one (B, N_new, 576) tensor are used as they are; rotate the rope part first, with rotary_apply);
    kv_cache (num_blocks, page_block_size, 1, 656) torch.uint8 or torch.float8_e4m3fn, FlashMLA's token:
        byte 0 .. 511: 512 e4m3, quantised per 128-wide tile | 512 .. 527: 4 float32 scales | 528 .. 655: 64 bfloat16, as they are
    Token i of sequence b goes to position cache_seqlens[b] + i (cache_seqlens: int32 (B,) lengths before the append, or an int;
    not modified) through block_table (int32 (B, max_blocks_per_seq)).  Per tile, in fp32: scale = amax / 448 (1 for an all-zero
    tile; scale_pow2: rounded up to a power of two, FlashMLA's ue8m0 option), byte = e4m3(clamp(x / scale, +-448)), round to
    nearest even.  Neither array is read on the host: a negative length, a position past the table's capacity or a page outside
    the pool drops that token, and the call can be captured in a graph.  Two tokens on one slot, or a NaN / infinity in a tile,
    are undefined (nothing is written out of bounds).  Wrong dtypes raise NotImplementedError with the name, wrong shapes and
    devices RuntimeError, a cache view that would need a copy ValueError.  Returns None.  No gradient."""
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        ext.ex_mla_fp8_pack(latent_new.detach() if isinstance(latent_new, torch.Tensor) else latent_new,
                            rope_new.detach() if isinstance(rope_new, torch.Tensor) else rope_new, kv_cache, cache_seqlens, block_table,
                            bool(scale_pow2))


def flash_mla_with_kvcache(q, k_cache, block_table, cache_seqlens, head_dim_v=512, *, softmax_scale=None, causal=False,
                           is_fp8_kvcache=False, indices=None, num_splits=0):
    """FlashMLA's flash_mla_with_kvcache (its argument order): multi-head latent attention at decode time over a paged cache of
    576-wide tokens [latent 512 | rotary 64].  q (B, Nq, H_q, 576) in the same layout: q[..., :512] meets the latent (which is
    also the value), q[..., 512:] the rotary part; block_table int32 (B, max_blocks_per_seq), cache_seqlens int32 (B,) on the
    device (or an int, or None: the capacity); indices None, or int32 (B, Nq, topk) token positions per query token (sparse
    attention: flash_mla_sparse_attn's rules).  softmax_scale defaults to 576 ** -0.5.
    is_fp8_kvcache=False: k_cache (num_blocks, page_block_size, 1, 576) in q's dtype (bfloat16 / float16); the call is
    flash_attn_with_kvcache(q[..., 512:], k_cache[..., 512:], k_cache[..., :512], qv=q[..., :512], ...) — with indices
    flash_mla_sparse_attn on the same views — and gives those calls' bits.
    is_fp8_kvcache=True: k_cache (num_blocks, page_block_size, 1, 656) torch.uint8 or torch.float8_e4m3fn, read as bytes: 512 e4m3
    | 4 float32 scales, one per 128-wide tile | 64 bfloat16 (mla_fp8_pack_cache writes it); q bfloat16, used without a copy.  A
    latent element is bfloat16(float(e4m3) * scale), rounded once, and the result is, to the bit, the 16-bit call's on these
    values.  0.57 of the 16-bit cache's bytes a token.
    head_dim_v other than 512 and wrong dtypes raise NotImplementedError with the name, wrong shapes and devices RuntimeError.
    Returns (o (B, Nq, H_q, 512), lse (B, H_q, Nq) float32).  No gradient."""
    who = "flash_mla_with_kvcache"
    if head_dim_v != 512:
        raise NotImplementedError(f"{who}: head_dim_v = {head_dim_v} is not supported (512 expected)")
    if not isinstance(q, torch.Tensor) or q.dtype not in (torch.bfloat16, torch.float16):
        dt = q.dtype if isinstance(q, torch.Tensor) else type(q).__name__
        raise NotImplementedError(f"{who}: q of dtype {dt} is not supported (bfloat16 or float16 expected)")
    if is_fp8_kvcache and q.dtype != torch.bfloat16:
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported with is_fp8_kvcache (bfloat16 expected: the rotary part "
                                  f"of a packed token is bfloat16)")
    want = (torch.uint8, torch.float8_e4m3fn) if is_fp8_kvcache else (q.dtype,)
    if not isinstance(k_cache, torch.Tensor) or k_cache.dtype not in want:
        dt = k_cache.dtype if isinstance(k_cache, torch.Tensor) else type(k_cache).__name__
        raise NotImplementedError(f"{who}: k_cache of dtype {dt} is not supported ({' or '.join(str(w) for w in want)} expected with "
                                  f"is_fp8_kvcache={bool(is_fp8_kvcache)})")
    for name, val in (("block_table", block_table), ("indices", indices)):
        if (val is not None or name == "block_table") and not (isinstance(val, torch.Tensor) and val.dtype == torch.int32):
            dt = val.dtype if isinstance(val, torch.Tensor) else type(val).__name__
            raise NotImplementedError(f"{who}: {name} of dtype {dt} is not supported (int32 tensor expected)")
    if isinstance(cache_seqlens, torch.Tensor) and cache_seqlens.dtype != torch.int32:
        raise NotImplementedError(f"{who}: cache_seqlens of dtype {cache_seqlens.dtype} is not supported (int32 tensor expected)")
    if not q.is_cuda or not k_cache.is_cuda:
        raise RuntimeError(f"{who}: q and k_cache must be GPU (HIP device) tensors; there is no CPU path")
    if q.dim() != 4 or q.shape[3] != 576:
        raise RuntimeError(f"{who}: q must be (B, Nq, H_q, 576), got {tuple(q.shape)}")
    width = 656 if is_fp8_kvcache else 576
    if k_cache.dim() != 4 or k_cache.shape[2:] != (1, width):
        raise RuntimeError(f"{who}: k_cache must be (num_blocks, page_block_size, 1, {width}) with is_fp8_kvcache={bool(is_fp8_kvcache)}, "
                           f"got {tuple(k_cache.shape)}")
    if indices is not None and (indices.dim() != 3 or indices.shape[:2] != q.shape[:2]):
        raise RuntimeError(f"{who}: indices must be an int32 (B, Nq, topk) tensor, got {tuple(indices.shape)}")
    import flashattention_lab_cuda as ext

    scale = 576 ** -0.5 if softmax_scale is None else softmax_scale
    q = q.detach()
    with torch.no_grad():
        if is_fp8_kvcache:
            return ext.ex_mla_fp8_forward(q[..., 512:], q[..., :512], k_cache, block_table, cache_seqlens, indices, bool(causal), scale,
                                          num_splits)
        if indices is not None:
            return flash_mla_sparse_attn(q[..., 512:], q[..., :512], k_cache[..., 512:], k_cache[..., :512], indices,
                                         cache_seqlens=cache_seqlens, block_table=block_table, softmax_scale=scale, causal=causal,
                                         num_splits=num_splits, return_softmax_lse=True)
        return flash_attn_with_kvcache(q[..., 512:], k_cache[..., 512:], k_cache[..., :512], cache_seqlens=cache_seqlens,
                                       block_table=block_table, softmax_scale=scale, causal=causal, num_splits=num_splits,
                                       return_softmax_lse=True, qv=q[..., :512])


_FP8_REFUSED = ("window_size", "softcap", "alibi_slopes", "sinks", "attn_bias", "mask", "block_sparse_mask", "dropout_p", "cu_seqlens_q",
                "cu_seqlens_k", "block_table", "rotary_cos", "rotary_sin")


_FP8_MOD_ARGS = ("window_size", "softcap", "sinks")   # what the flash_attn_fp8_* functions take and the older wrappers refuse


def _fp8_mod_args(who, window_size, softcap, sinks):
    """window_size, softcap and sinks of the flash_attn_fp8_* functions as the shim takes them (the shim and the library check
    the rest: the sinks' shape and device against q)"""
    try:
        left, right = window_size
        if isinstance(left, bool) or isinstance(right, bool):
            raise TypeError
        left, right = operator.index(left), operator.index(right)
    except (TypeError, ValueError):
        raise RuntimeError(f"{who}: window_size must be a pair (left, right) of ints, got {window_size!r}") from None
    if left < -1 or right < -1:
        raise RuntimeError(f"{who}: window ({left}, {right}): each bound must be >= 0, or -1 for unbounded")
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)) or not math.isfinite(softcap) or softcap < 0:
        raise RuntimeError(f"{who}: softcap must be a finite number >= 0 (got {softcap!r})")
    if sinks is not None and not (isinstance(sinks, torch.Tensor) and sinks.dtype == torch.float32):
        raise RuntimeError(f"{who}: sinks must be a float32 tensor (pass a 16-bit parameter as p.float())")
    return dict(window=(left, right), softcap=float(softcap), sinks=None if sinks is None else sinks.detach())


def _fp8_refuse(who, refused, unsupported, what, hint_to=None):
    """The refusals by name of the fp8 wrappers: an argument of `refused` at its neutral value passes, at any other it is a
    NotImplementedError (hint_to: the function that takes window_size / softcap / sinks), an unknown name a TypeError."""
    for name, val in unsupported.items():
        if name in refused:
            if val is None or val is False or (name == "window_size" and tuple(val) == (-1, -1)) or \
                    (name in ("softcap", "dropout_p") and val == 0.0) or (name == "max_seqlen_q" and val == 0 and "max_seqlen_q" in refused):
                continue
            hint = " (the cache is filled by flash_attn_with_kvcache's append, or by the caller)" if name in ("k", "v") and "k" in refused else ""
            if hint_to and name in _FP8_MOD_ARGS:
                hint = f" ({hint_to} takes it)"
            raise NotImplementedError(f"{who}: {name} is not supported by the fp8 {what}{hint}")
        raise TypeError(f"{who}() got an unexpected keyword argument {name!r}")


def flash_attention_fp8(q, k, v, *, q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False,
                        out_dtype=torch.bfloat16, layout="bhnd", return_lse=False, **unsupported):
    """FlashAttention-3's fp8 call: attention over q, k, v that are ALREADY torch.float8_e4m3fn, with one float32 descale per
    (batch, K/V head) for each of them (flash_attn_func(..., q_descale=, k_descale=, v_descale=)).  Forward only.
        o = softmax(softmax_scale * q_descale * k_descale * q8 k8^T [causal]) (v8 * v_descale)
    q (B, H_q, Nq, 128), k and v (B, H_kv, Nk, 128) with layout="bhnd"; (B, N, H, 128), FlashAttention-3's own layout, with
    layout="bnhd".  Views are used at their own strides and never copied (a contiguous last dim, a 16-byte aligned start and strides
    that are multiples of 16 bytes): the [:, :Nk] prefix of a (B, capacity, H_kv, 128) e4m3 cache of flash_attn_with_kvcache is such a
    view, and nothing of the cache past Nk reaches the result.  H_q is a multiple of H_kv; query head h reads K/V head
    h // (H_q // H_kv).  Descales: float32 (B, H_kv) or (H_kv,) on q's device, q_descale included; None = 1.  They are read on the
    device only (positive, finite), so a captured call replays with changed values.  softmax_scale defaults to 128 ** -0.5; the
    causal diagonal is bottom-right aligned (row i sees j <= i + Nk - Nq), and a row without a visible key gives o = 0, lse = -inf.
    Both products run on the e4m3 matrix instruction; P is rounded to e4m3 on every row, as in FlashAttention-3 (2^-4 relative
    per probability: it averages out over a row's keys and stands in full on a row that sees a couple).
    Refused by name before anything runs (NotImplementedError): window_size, softcap, alibi_slopes, sinks, attn_bias, masks,
    dropout, packed or paged forms, head dims other than 128, 16-bit q / k / v (fa3_attention(fp8=True) and flash_attention_ex take
    those), out_dtype other than bfloat16 / float16.  Wrong shapes and devices raise RuntimeError, a view that would need a copy
    ValueError.  Returns o in `layout` and out_dtype, and with return_lse also lse (B, H_q, Nq) float32.  No gradient."""
    _fp8_refuse("flash_attention_fp8", _FP8_REFUSED, unsupported, "call", "flash_attn_fp8_func")
    return _fp8_func("flash_attention_fp8", q, k, v, q_descale, k_descale, v_descale, softmax_scale, causal, out_dtype, layout,
                     return_lse, {})


def flash_attn_fp8_func(q, k, v, *, q_descale=None, k_descale=None, v_descale=None, softmax_scale=None, causal=False,
                        window_size=(-1, -1), softcap=0.0, sinks=None, out_dtype=torch.bfloat16, layout="bhnd", return_lse=False,
                        **unsupported):
    """flash_attention_fp8 with a sliding window, a softcap and attention sinks (FlashAttention-3's flash_attn_func arguments of
    those names), composing with each other and with everything flash_attention_fp8 takes; its docstring holds for the rest.
      window_size  (left, right) ints >= -1, -1 = unbounded; causal=True sets right = 0.  Bottom-right aligned: row i sits at
                   pos = i + Nk - Nq and sees key j iff pos - left <= j <= pos + right and 0 <= j < Nk.  The kernel walks only the
                   key tiles a workgroup's rows see: O(N w) work.
      softcap      C > 0: s~ = C tanh(s / C) of s = softmax_scale q_descale k_descale (q8 . k8), before the mask; 0 = off.
      sinks        float32 (H_q,) on q's device in natural-log units, one per QUERY head, read on the device only: an extra softmax
                   column with a zero value (lse contains it), never capped, masked or windowed.  A head at -inf gives the bits
                   of the call without sinks.
    A row that sees no key gives o = 0 and lse = -inf, with sinks lse = sink.  With all three at their defaults the call IS
    flash_attention_fp8 (the same kernels).  Everything else flash_attention_fp8 refuses is refused here by name."""
    who = "flash_attn_fp8_func"
    _fp8_refuse(who, tuple(n for n in _FP8_REFUSED if n not in _FP8_MOD_ARGS), unsupported, "call")
    return _fp8_func(who, q, k, v, q_descale, k_descale, v_descale, softmax_scale, causal, out_dtype, layout, return_lse,
                     _fp8_mod_args(who, window_size, softcap, sinks))


def _fp8_func(who, q, k, v, q_descale, k_descale, v_descale, softmax_scale, causal, out_dtype, layout, return_lse, mod):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype in (torch.float16, torch.bfloat16, torch.float32):
            raise NotImplementedError(f"{who}: 16-bit inputs are not supported: {name} is {t.dtype}, torch.float8_e4m3fn expected "
                                      f"(quantise first, or use fa3_attention(fp8=True) / flash_attention_ex)")
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
        if t.dim() == 4 and t.shape[3] != 128:
            raise NotImplementedError(f"{who}: head_dim {t.shape[3]} is not supported (128 only)")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        o, lse = ext.fp8_forward(q.detach(), k.detach(), v.detach(), bool(causal), softmax_scale,
                                 None if q_descale is None else q_descale.detach() if isinstance(q_descale, torch.Tensor) else q_descale,
                                 None if k_descale is None else k_descale.detach() if isinstance(k_descale, torch.Tensor) else k_descale,
                                 None if v_descale is None else v_descale.detach() if isinstance(v_descale, torch.Tensor) else v_descale,
                                 out_dtype, layout, **mod)
    return (o, lse) if return_lse else o


_FP8_VARLEN_REFUSED = ("window_size", "softcap", "alibi_slopes", "sinks", "attn_bias", "mask", "block_sparse_mask", "dropout_p",
                       "seqused_q", "seqused_k", "cache_leftpad", "cache_batch_idx", "rotary_cos", "rotary_sin")


def flash_attention_fp8_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, block_table=None, q_descale=None,
                               k_descale=None, v_descale=None, softmax_scale=None, causal=False, out_dtype=torch.bfloat16,
                               return_softmax_lse=False, **unsupported):
    """The packed and the paged form of flash_attention_fp8 (FlashAttention-3's flash_attn_varlen_func with q_descale / k_descale /
    v_descale): q (total_q, H_q, 128) in torch.float8_e4m3fn packed by cu_seqlens_q, a token- or head-strided view (a slice of a
    fused projection) taken without a copy.  Without block_table k and v are (total_k, H_kv, 128) e4m3 packed by cu_seqlens_k.  With
    block_table, int32 (B, max_blocks_per_seq) on the device, k and v are the e4m3 pools (num_blocks, ps, H_kv, 128) of the paged
    cache flash_attn_with_kvcache appends to, ps a multiple of 16, each pool at its own page and token strides; key t of sequence
    b is pool[block_table[b, t // ps], t % ps] and len_k[b] = cu_seqlens_k[b + 1] - cu_seqlens_k[b], clamped on the device to
    [0, min(max_seqlen_k, max_blocks_per_seq * ps)].  Descales: float32 (B, H_kv), B the number of sequences, or (H_kv,); None = 1;
    read on the device only.  H_q % H_kv == 0 and query head h reads K/V head h // (H_q // H_kv).  softmax_scale defaults to
    128 ** -0.5; the causal diagonal is bottom-right aligned per sequence (j <= i + len_k[b] - len_q[b]).  Every sequence has the
    bits of flash_attention_fp8 on that sequence alone.  A row without a visible key (an empty key sequence, a causal row above the
    diagonal) gives o = 0 and lse = -inf; rows of o that belong to no sequence are not written.
    Nothing is read on the host: the call never synchronises and a captured call replays after the offsets, the table and the
    descale values changed in place.  Offsets and table are untrusted: offsets and lengths are clamped, a page outside
    [0, num_blocks) reads as zero bytes for K and V, no entry past ceil(len_k / ps) is read, page offsets are 64-bit and pages may be
    shared.  Forward only: q, k or v requiring grad under grad mode raises RuntimeError.
    Refused by name before anything runs (NotImplementedError): window_size, softcap, alibi_slopes, sinks, attn_bias, masks,
    dropout, seqused_q / seqused_k, cache_leftpad, cache_batch_idx, head dims other than 128, 16-bit q / k / v
    (flash_attention_varlen takes those), out_dtype other than bfloat16 / float16.
    Returns o (total_q, H_q, 128) in out_dtype, and with return_softmax_lse also lse float32 (H_q, total_q), the layout of
    flash_attention_varlen(return_softmax_lse=True)."""
    _fp8_refuse("flash_attention_fp8_varlen", _FP8_VARLEN_REFUSED, unsupported, "call", "flash_attn_fp8_varlen_func")
    return _fp8_varlen_func("flash_attention_fp8_varlen", q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, block_table,
                            q_descale, k_descale, v_descale, softmax_scale, causal, out_dtype, return_softmax_lse, {})


def flash_attn_fp8_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, block_table=None, q_descale=None,
                               k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                               sinks=None, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """flash_attention_fp8_varlen with a sliding window, a softcap and attention sinks, packed or paged; its docstring holds for the
    rest, and window_size, softcap and sinks are flash_attn_fp8_func's, per sequence (pos = i + len_k[b] - len_q[b]; sinks float32
    (H_q,)).  Every sequence has the bits of flash_attn_fp8_func on that sequence alone with the same window, cap and sinks.  With
    all three at their defaults the call IS flash_attention_fp8_varlen.  Everything else that one refuses is refused here."""
    who = "flash_attn_fp8_varlen_func"
    _fp8_refuse(who, tuple(n for n in _FP8_VARLEN_REFUSED if n not in _FP8_MOD_ARGS), unsupported, "call")
    return _fp8_varlen_func(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, block_table, q_descale, k_descale,
                            v_descale, softmax_scale, causal, out_dtype, return_softmax_lse,
                            _fp8_mod_args(who, window_size, softcap, sinks))


def _fp8_varlen_func(who, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, block_table, q_descale, k_descale, v_descale,
                     softmax_scale, causal, out_dtype, return_softmax_lse, mod):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype in (torch.float16, torch.bfloat16, torch.float32):
            raise NotImplementedError(f"{who}: 16-bit inputs are not supported: {name} is {t.dtype}, torch.float8_e4m3fn expected "
                                      f"(quantise first, or use flash_attention_varlen)")
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
        if t.dim() >= 1 and t.shape[-1] != 128:
            raise NotImplementedError(f"{who}: head_dim {t.shape[-1]} is not supported (128 only)")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        raise RuntimeError(f"{who}: forward only — q, k or v requires grad and the fp8 call has no backward (call it under "
                           f"torch.no_grad(), or detach the tensors)")
    import flashattention_lab_cuda as ext

    det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t   # noqa: E731
    with torch.no_grad():
        o, lse = ext.fp8_varlen_forward(q.detach(), k.detach(), v.detach(), cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                        bool(causal), softmax_scale, det(q_descale), det(k_descale), det(v_descale), out_dtype,
                                        block_table, **mod)
    return (o, lse) if return_softmax_lse else o


_FP8_KVCACHE_REFUSED = ("k", "v", "rotary_cos", "rotary_sin", "rotary_interleaved", "window_size", "softcap", "alibi_slopes", "sinks",
                        "cache_leftpad", "cu_seqlens_q", "max_seqlen_q", "cu_seqlens_k_new", "qv", "attn_bias", "mask", "dropout_p")


def flash_attention_fp8_kvcache(q, k_cache, v_cache, *, cache_seqlens=None, block_table=None, cache_batch_idx=None, q_descale=None,
                                k_descale=None, v_descale=None, softmax_scale=None, causal=False, num_splits=0,
                                out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """fp8 KV-cache decoding with split-KV: an e4m3 q over the e4m3 cache that flash_attn_with_kvcache(..., k_descale=, v_descale=)
    writes, both products on the e4m3 matrix instruction (FlashAttention-3's fp8 contract in the decode loop).
        s[i, j] = softmax_scale * q_descale * k_descale * (q8[i] . k8[j]),   o[i] = sum_j softmax(s)[i, j] * v8[j] * v_descale
    q (B, Nq, H_q, 128) in torch.float8_e4m3fn; a token- or batch-strided view is used without a copy (contiguous last dim, 16-byte
    aligned).  k_cache, v_cache: contiguous form (B_cache, cache_len, H_kv, 128) e4m3, or with block_table (int32 (B,
    max_blocks_per_seq) on the device) the pools (num_blocks, ps, H_kv, 128), ps a positive multiple of 16.  Both forms keep their own
    batch / page and token strides (64-bit page offsets; views such as pool.unbind(1) are never copied).  H_q % H_kv == 0; query head
    h reads K/V head h // (H_q // H_kv).  cache_seqlens: int32 (B,) on the device, an int, or None (full); len_b =
    clamp(cache_seqlens[b], 0, capacity), capacity = cache_len or max_blocks_per_seq * ps.  cache_batch_idx: int32 (B,), contiguous
    form only; an index outside [0, B_cache) gives an empty sequence.  Descales: float32 (B, H_kv) or (H_kv,), q_descale included;
    None = 1; read on the device only (finite, > 0).  softmax_scale defaults to 128 ** -0.5.  causal is bottom-right aligned: key j
    is visible to token i iff j <= len_b - Nq + i.  A row without a visible key gives o = 0 and lse = -inf.  P is rounded to e4m3 on
    every row; l and lse come from the unrounded p.
    Lengths, table, indices and descales are untrusted device memory, never read on the host: a captured call replays after they
    change in place.  A page outside [0, num_blocks) reads as zero K and V and takes part with score 0; no table entry past
    ceil(len_b / ps) is read; cache bytes that no live token owns never reach a result.
    num_splits: 0 = the library's rule, else 1 .. 256; the result's bits depend on it and on nothing else of the launch.
    Refused by name before anything runs (NotImplementedError): a 16-bit q (flash_attn_with_kvcache takes it), a 16-bit or other
    8-bit cache, head dims other than 128, new tokens k / v (fill the cache with flash_attn_with_kvcache's append), rotary,
    window_size, softcap, alibi_slopes, sinks, cache_leftpad, cu_seqlens_q, qv, block_table together with cache_batch_idx, out_dtype
    other than bfloat16 / float16.
    Returns o (B, Nq, H_q, 128) in out_dtype, and with return_softmax_lse also lse float32 (B, H_q, Nq).  No gradient."""
    _fp8_refuse("flash_attention_fp8_kvcache", _FP8_KVCACHE_REFUSED, unsupported, "decode call", "flash_attn_fp8_with_kvcache")
    return _fp8_kvcache_func("flash_attention_fp8_kvcache", q, k_cache, v_cache, cache_seqlens, block_table, cache_batch_idx, q_descale,
                             k_descale, v_descale, softmax_scale, causal, num_splits, out_dtype, return_softmax_lse, {})


def flash_attn_fp8_with_kvcache(q, k_cache, v_cache, *, cache_seqlens=None, block_table=None, cache_batch_idx=None, q_descale=None,
                                k_descale=None, v_descale=None, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                                sinks=None, num_splits=0, out_dtype=torch.bfloat16, return_softmax_lse=False, **unsupported):
    """flash_attention_fp8_kvcache with a sliding window, a softcap and attention sinks; its docstring holds for the rest.
      window_size  (left, right) ints >= -1, -1 = unbounded; causal=True sets right = 0.  Token i of a sequence of len_b cached
                   keys sits at pos = len_b - Nq + i and sees key j iff pos - left <= j <= pos + right and 0 <= j < len_b: the
                   visible set of flash_attn_with_kvcache given the same arguments.  The splits cut only the keys from the
                   first 64-key tile some row of a 32-row tile sees; no table entry and no cache byte below it is read.  The
                   split rule (num_splits=0) takes min(capacity, left + max(right, 0) + Nq) for the capacity when left >= 0.
      softcap      C > 0: s~ = C tanh(s / C), before the mask; 0 = off.
      sinks        float32 (H_q,) on q's device in natural-log units, one per QUERY head, read on the device only (a captured call
                   replays with changed values).  The sink joins in the combine, once per row, so such a call runs at least two
                   splits (num_splits=1 is raised to 2).  A row without a visible key gives o = 0, lse = sink.
    The result's bits depend on num_splits, the window and nothing else of the launch.  With all three at their defaults the call
    IS flash_attention_fp8_kvcache.  Everything else that one refuses is refused here by name."""
    who = "flash_attn_fp8_with_kvcache"
    _fp8_refuse(who, tuple(n for n in _FP8_KVCACHE_REFUSED if n not in _FP8_MOD_ARGS), unsupported, "decode call")
    return _fp8_kvcache_func(who, q, k_cache, v_cache, cache_seqlens, block_table, cache_batch_idx, q_descale, k_descale, v_descale,
                             softmax_scale, causal, num_splits, out_dtype, return_softmax_lse,
                             _fp8_mod_args(who, window_size, softcap, sinks))


def _fp8_kvcache_func(who, q, k_cache, v_cache, cache_seqlens, block_table, cache_batch_idx, q_descale, k_descale, v_descale,
                      softmax_scale, causal, num_splits, out_dtype, return_softmax_lse, mod):
    if not isinstance(q, torch.Tensor):
        raise RuntimeError(f"{who}: q must be a tensor, got {type(q).__name__}")
    if q.dtype in (torch.float16, torch.bfloat16, torch.float32):
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported: torch.float8_e4m3fn expected (a 16-bit q over an e4m3 "
                                  f"cache is flash_attn_with_kvcache(..., k_descale=, v_descale=))")
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
        if t.dim() >= 1 and t.shape[-1] != 128:
            raise NotImplementedError(f"{who}: head_dim {t.shape[-1]} is not supported (128 only); got {name} of shape {tuple(t.shape)}")
    if block_table is not None and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    import flashattention_lab_cuda as ext

    det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t   # noqa: E731
    with torch.no_grad():
        o, lse = ext.fp8_kvcache_forward(q.detach(), k_cache.detach(), v_cache.detach(), cache_seqlens, block_table, cache_batch_idx,
                                         det(q_descale), det(k_descale), det(v_descale), softmax_scale, bool(causal), num_splits,
                                         out_dtype, **mod)
    return (o, lse) if return_softmax_lse else o


_FP8_STEP_REFUSED = ("cache_leftpad", "cu_seqlens_q", "max_seqlen_q", "cu_seqlens_k_new", "qv", "alibi_slopes", "attn_bias", "mask",
                     "dropout_p")


def flash_attn_fp8_kvcache_step(q, k_cache, v_cache, k, v, *, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, cache_seqlens,
                                block_table=None, cache_batch_idx=None, q_descale=None, k_descale=None, v_descale=None,
                                softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0, sinks=None, num_splits=0,
                                out_dtype=None, q8_out=None, return_softmax_lse=False, **unsupported):
    """One decode step on the e4m3 matrix instruction in one call: append the new tokens k, v (B, N_new, H_kv, 128) to the e4m3
    cache, rotate and quantise q (B, Nq, H_q, 128), and attend with flash_attn_fp8_with_kvcache's kernels; FlashAttention-3's
    flash_attn_with_kvcache(q, k_cache, v_cache, k=, v=, rotary_cos=, rotary_sin=, q_descale=, k_descale=, v_descale=).
    cache_seqlens (required; int32 (B,) on the device, or an int) holds the lengths BEFORE the append.  With
    L_b = clamp(cache_seqlens[b], 0, capacity - N_new), hk = h // (H_q // H_kv) and len_b = L_b + N_new:
      16-bit mode  q, k, v all float16 or all bfloat16.
        1. Token n of sequence b goes to position L_b + n of cache row cache_batch_idx[b] (or b), or through block_table to
           pool[table[b, pos // ps], pos % ps].  k is rotated at table row L_b + n when rotary_cos / rotary_sin ((seqlen_ro,
           rotary_dim / 2) in q's dtype, rotary_dim a multiple of 16 up to 128; rotary_interleaved as flash_attn_with_kvcache) are
           given, and rounded once to its dtype.  The stored bytes are clamp(x * (1 / descale[b, hk]), +-448) rounded to nearest
           even: the bytes flash_attn_with_kvcache(..., k=, v=, k_descale=, v_descale=) stores.  A cache row outside [0, B_cache)
           or a page outside the pool drops the token; no other byte of the caches is written.
        2. q token i is rotated at L_b + i when causal or a window bound is given, otherwise every token at L_b
           (flash_attn_with_kvcache's rule), rounded once to its dtype and quantised with 1 / q_descale[b, hk].  The codes go into
           q8_out, a torch.float8_e4m3fn tensor of q's shape, when one is passed, else into the call's workspace.
        3. o, lse are, bit for bit, flash_attn_fp8_with_kvcache(q8, k_cache, v_cache, cache_seqlens=len_b, ...) with the same
           descales, causal, window_size, softcap, sinks and num_splits on the caches as step 1 left them.
      e4m3 mode    q, k, v all torch.float8_e4m3fn: the new bytes are scattered as they are and q is used in place; rotary and
                   q8_out are refused.  Mixed dtypes are refused.
    Descales: float32 (B, H_kv) or (H_kv,), static, None = 1.  out_dtype defaults to q's dtype, bfloat16 in e4m3 mode.  Lengths,
    table, row indices, descales and rotary tables are read on the device only, the first three clamped as above, so the call
    captures into a graph and replays after any of them change in place; seqlen_ro >= capacity + max(0, Nq - N_new) is checked on
    the host.  Two sequences appending to one page and duplicate cache_batch_idx rows are undefined.
    Refused by name before anything runs (NotImplementedError): cache_leftpad, cu_seqlens_q, cu_seqlens_k_new, qv, alibi_slopes,
    attn_bias, dropout_p, head dims other than 128, block_table together with cache_batch_idx, and k / v missing (attention alone
    is flash_attn_fp8_with_kvcache).  Dynamic q scales are quantize_fp8's, in front of flash_attn_fp8_with_kvcache.
    Returns o (B, Nq, H_q, 128) in out_dtype, and with return_softmax_lse also lse float32 (B, H_q, Nq).  No gradient."""
    who = "flash_attn_fp8_kvcache_step"
    _fp8_refuse(who, _FP8_STEP_REFUSED, unsupported, "decode step")
    if k is None or v is None:
        raise NotImplementedError(f"{who}: k / v missing: the step appends new tokens (attention over the cache as it is: "
                                  f"flash_attn_fp8_with_kvcache)")
    for name, t in (("q", q), ("k", k), ("v", v), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() >= 1 and t.shape[-1] != 128:
            raise NotImplementedError(f"{who}: head_dim {t.shape[-1]} is not supported (128 only); got {name} of shape {tuple(t.shape)}")
    if q.dtype not in (torch.float16, torch.bfloat16, torch.float8_e4m3fn):
        raise NotImplementedError(f"{who}: q of dtype {q.dtype} is not supported (float16, bfloat16 or torch.float8_e4m3fn)")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise NotImplementedError(f"{who}: mixed dtypes are not supported: q, k, v must be all float16, all bfloat16 or all "
                                  f"torch.float8_e4m3fn (got {q.dtype}, {k.dtype}, {v.dtype})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dtype != torch.float8_e4m3fn:
            raise NotImplementedError(f"{who}: {name} of dtype {t.dtype} is not supported (torch.float8_e4m3fn expected)")
    if q.dtype == torch.float8_e4m3fn:
        for name, val in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin), ("q8_out", q8_out)):
            if val is not None:
                raise NotImplementedError(f"{who}: {name} is not supported with torch.float8_e4m3fn q, k, v (the codes are used as they are)")
    if block_table is not None and cache_batch_idx is not None:
        raise NotImplementedError(f"{who}: block_table together with cache_batch_idx is not supported (a table row is the indirection)")
    if out_dtype is not None and out_dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{who}: out_dtype {out_dtype} is not supported (torch.bfloat16 or torch.float16)")
    mod = _fp8_mod_args(who, window_size, softcap, sinks)
    import flashattention_lab_cuda as ext

    det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t   # noqa: E731
    with torch.no_grad():
        o, lse = ext.fp8_kvcache_step(q.detach(), k_cache.detach(), v_cache.detach(), k.detach(), v.detach(), cache_seqlens, block_table,
                                      cache_batch_idx, det(q_descale), det(k_descale), det(v_descale), softmax_scale, bool(causal),
                                      num_splits, out_dtype, rotary_cos=det(rotary_cos), rotary_sin=det(rotary_sin),
                                      rotary_interleaved=bool(rotary_interleaved), q8_out=det(q8_out), **mod)
    return (o, lse) if return_softmax_lse else o


def quantize_fp8(x, heads_per_scale=1, descale=None, layout="bnhd", out=None, out_layout=None, descale_out=None, scale_pow2=False,
                 cu_seqlens=None, max_seqlen=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, seqlen_offsets=0):
    """The producer of the fp8 calls' inputs: a float16 / bfloat16 tensor as torch.float8_e4m3fn codes plus the float32 descales
    (B, H / heads_per_scale) that flash_attention_fp8 / _varlen / _kvcache and the e4m3 cache of flash_attn_with_kvcache read
    (fa_fp8_quantize, include/fa_mi355x.h).  Returns (x8, descale).
    x: (B, N, H, d) with layout="bnhd", (B, H, N, d) with "bhnd", packed (total, H, d) with "thd" plus cu_seqlens (int32 (B + 1,))
    and max_seqlen; d a multiple of 16 in [16, 256].  A view with a contiguous last dim, a 16-byte aligned start and strides that are
    multiples of 8 elements, such as qkv[:, :, :H_q] of a fused projection, is read in place.  One descale covers heads_per_scale
    adjacent heads x all tokens of a sequence x d: H_q // H_kv for q under grouped-query attention, 1 for k and v.
    descale=None (dynamic): descale = amax / 448 over the unit, 1 for an all-zero or empty unit; scale_pow2 rounds it up to a power
    of two.  descale given (float32 (B, H / g) or (H / g,), positive and finite, read on the device only): the static mode, one
    launch, and the tensor itself is returned.  Codes: e4m3 round-to-nearest-even of clamp(x * (1 / descale), +-448), the arithmetic
    of the e4m3 cache append, so quantize_fp8(k_new, descale=k_descale) has the bytes flash_attn_with_kvcache(k=k_new,
    k_descale=k_descale) stores.  NaN and infinity in x are outside the contract.
    out: an e4m3 tensor in out_layout (default: layout) at its own strides (multiples of 16 bytes), e.g. cache[:, :N] of a
    (B, capacity, H, d) cache; bytes outside the addressed rows are never written, nor are packed tokens no sequence owns.
    rotary_cos / rotary_sin: (seqlen_ro, rotary_dim / 2) tables in x's dtype rotate the first rotary_dim head dims on the way, by
    common.rotary.apply_rotary_emb's rules and with its bits (rotary_interleaved; seqlen_offsets an int or int32 (B,); a token
    outside the table passes through): the call equals itself on the rotated tensor, in every byte and descale.
    Nothing is read on the host, so projection -> quantise -> fp8 attention captures into one graph and replays after x, descale,
    cu_seqlens and the offsets change in place; two runs give the same bits.  NotImplementedError for other dtypes and head dims,
    ValueError for views that would need a copy.  Nothing is recorded by autograd."""
    import flashattention_lab_cuda as ext

    det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t   # noqa: E731
    with torch.no_grad():
        return ext.fp8_quantize(det(x), heads_per_scale, det(descale), layout, det(out), out_layout, det(descale_out), scale_pow2,
                                cu_seqlens, max_seqlen, det(rotary_cos), det(rotary_sin), rotary_interleaved, seqlen_offsets)


def quantize_fp8_qkv(q, k, v, *, layout="bnhd", q_descale=None, k_descale=None, v_descale=None, scale_pow2=False, rotary_cos=None,
                     rotary_sin=None, rotary_interleaved=False, seqlen_offsets=0, cu_seqlens_q=None, cu_seqlens_k=None,
                     max_seqlen_q=None, max_seqlen_k=None):
    """quantize_fp8 on q, k and v with the scale units of the fp8 calls: (q8, k8, v8, q_descale, k_descale, v_descale), every
    descale float32 (B, H_kv).  q takes heads_per_scale = H_q // H_kv, k and v take 1; the tables rotate q and k and never v.
    A descale that is given makes that tensor's call static.  layout as quantize_fp8's; "thd" takes cu_seqlens_q / max_seqlen_q for
    q and cu_seqlens_k / max_seqlen_k for k and v.  The results go straight into flash_attention_fp8(layout=layout),
    flash_attention_fp8_varlen and flash_attention_fp8_kvcache."""
    who = "quantize_fp8_qkv"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    hdim = 1 if layout == "bhnd" else -2
    if q.dim() < 3 or k.dim() != q.dim() or v.dim() != q.dim():
        raise RuntimeError(f"{who}: q, k, v must share the layout {layout!r}; got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    hq, hkv = q.shape[hdim], k.shape[hdim]
    if v.shape[hdim] != hkv or hkv < 1 or hq % hkv != 0:
        raise RuntimeError(f"{who}: H_q = {hq} must be a multiple of H_kv = {hkv}, shared by k and v (v has {v.shape[hdim]})")
    rot = dict(rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved, seqlen_offsets=seqlen_offsets)
    q8, qd = quantize_fp8(q, hq // hkv, q_descale, layout, scale_pow2=scale_pow2, cu_seqlens=cu_seqlens_q, max_seqlen=max_seqlen_q, **rot)
    k8, kd = quantize_fp8(k, 1, k_descale, layout, scale_pow2=scale_pow2, cu_seqlens=cu_seqlens_k, max_seqlen=max_seqlen_k, **rot)
    v8, vd = quantize_fp8(v, 1, v_descale, layout, scale_pow2=scale_pow2, cu_seqlens=cu_seqlens_k, max_seqlen=max_seqlen_k)
    return q8, k8, v8, qd, kd, vd


# The fp8 calls at head dims 64, 128 and 256 live in a module of their own (common/fp8_attention.py, which imports this one); they are
# reachable from here too, where their namesakes are.
_FP8_HDIM_FUNCS = ("fp8_attn_func", "fp8_attn_varlen_func", "fp8_attn_with_kvcache", "fp8_attn_with_kvcache_varlen",
                   "fp8_attn_kvcache_step")


def __getattr__(name):
    if name in _FP8_HDIM_FUNCS:
        from common import fp8_attention

        return getattr(fp8_attention, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
