"""The packed fp8 decode step (include/fa_mi355x.h: fa_fp8_kvcache_step_varlen, fa_fp8_forward_kvcache_varlen;
common.fp8_attention.fp8_attn_kvcache_step / fp8_attn_with_kvcache_varlen) on the CPU (torch): a d- and
offset-parameterised model of the prep kernel, built from what the padded step's model (tests/fp8_step_ref.py) is built from.

    cu_range(cu, b, total, bound)   the device clamp (csrc/fa_decode_common.h: kv_cu_range), tests/kvcache_varlen_ref.cu_range's
    BAD_OFFSETS                     out-of-range offset arrays: negative, past total, decreasing, a range longer than the bound
    PROBLEM, problem(...)           the one problem of the GPU tests: B = 5, nq = [1, 0, 5, 20, 3], lengths [300, 17, 0, 64, 129],
                                    nnew = [1, 0, 5, 2, 3], capacity 384, H_kv = 2
    model(call)                     (k_after, v_after, q8 (total_q, H_q, d) uint8, len_eff [B]) of the step's prep: per sequence
                                    nnew_b / nq_b from the clamp, L_b = clamp(cache_seqlens[b], 0, capacity - nnew_b), new key n
                                    rotated at L_b + n and stored at L_b + n, q token i rotated at L_b + i (causal or a window
                                    bound) or at L_b, both quantised with 1 / descale[b, hk]; q8 rows no sequence owns are None-marked
                                    by `owned`
    from_padded(call)               a call of tests/fp8_step_ref.build_call as a packed one (uniform lengths)

Caches and codes are uint8 throughout."""
import torch

from tests.fp8_quantize_ref import codes_of, rotate32, tables
from tests.fp8_step_ref import scales_bh
from tests.kvcache_fp8_ref import quantize
from tests.kvcache_rotary_ref import slot_of

FILL = 0xA5
HEAD_DIMS = (64, 128, 256)
PROBLEM = dict(B=5, nq=(1, 0, 5, 20, 3), lens=(300, 17, 0, 64, 129), nnew=(1, 0, 5, 2, 3), capacity=384, hkv=2)


def cu_range(cu, b, total, bound):
    """(start, n): start = clamp(cu[b], 0, total), n = clamp(cu[b + 1] - cu[b], 0, min(bound, total - start))"""
    c0, c1 = int(cu[b]), int(cu[b + 1])
    start = min(max(c0, 0), total)
    return start, min(max(c1 - c0, 0), min(bound, total - start))


def lengths_to_cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


# offsets for (total 29, bound 20, B = 5): each breaks the well-formed shape in one way; the clamp makes every one of them safe
BAD_OFFSETS = {
    "negative": [-7, 1, 1, 6, 26, 29],
    "past_total": [0, 1, 1, 6, 40, 2 ** 31 - 1],
    "decreasing": [0, 9, 4, 6, 2, 29],
    "longer_than_bound": [0, 1, 1, 1, 29, 29],
    "int_min": [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, 3, 3],
}


def capacity(call):
    return call["block_table"].shape[1] * call["k_cache"].shape[1] if call["block_table"] is not None else call["k_cache"].shape[1]


def ranges(call):
    """per sequence (tok0, nq_b, start_b, nnew_b, L_b) as the device computes them"""
    nb, cap = call["B"], capacity(call)
    out = []
    for b in range(nb):
        tok0, nq = cu_range(call["cu_q"], b, call["q"].shape[0], call["max_seqlen_q"])
        if call["cu_kn"] is not None:
            st, nnew = cu_range(call["cu_kn"], b, call["k_new"].shape[0], cap)
        else:
            st, nnew = 0, call["k_new"].shape[1]
        L = min(max(int(call["cache_seqlens"][b]), 0), cap - nnew)
        out.append((tok0, nq, st, nnew, L))
    return out


def model(call):
    """(k_after, v_after, q8, len_eff, owned): q8 uint8 (total_q, H_q, d) with zeros in rows no sequence owns, owned bool (total_q,)"""
    nb, hq, hkv = call["B"], call["hq"], call["hkv"]
    g = hq // hkv
    cos, sin, inter = call["rotary_cos"], call["rotary_sin"], call["rotary_interleaved"]
    per_token = call["causal"] or call["window"][0] >= 0 or call["window"][1] >= 0
    kd, vd, qd = (scales_bh(call[n], nb, hkv) for n in ("k_descale", "v_descale", "q_descale"))
    ka, va = call["k_cache"].clone(), call["v_cache"].clone()
    ps = ka.shape[1]
    total_q = call["q"].shape[0]
    q8 = torch.zeros(tuple(call["q"].shape), dtype=torch.uint8)
    owned = torch.zeros((total_q,), dtype=torch.bool)
    len_eff = []
    e4 = call["q"].dtype == torch.uint8
    for b, (tok0, nq, st, nnew, L) in enumerate(ranges(call)):
        len_eff.append(L + nnew)
        if nnew:
            src_k = call["k_new"][st:st + nnew] if call["cu_kn"] is not None else call["k_new"][b]
            src_v = call["v_new"][st:st + nnew] if call["cu_kn"] is not None else call["v_new"][b]
            k16, v16 = src_k[None], src_v[None]
            if e4:
                k8, v8 = k16, v16
            else:
                if cos is not None:
                    k16 = rotate32(k16, cos, sin, [L], inter)
                k8, v8 = quantize(k16, kd[b:b + 1]), quantize(v16, vd[b:b + 1])
            for n in range(nnew):
                unit, pos = slot_of(b, L + n, call["block_table"], call["cache_batch_idx"], ps)
                if 0 <= unit < ka.shape[0]:
                    ka[unit, pos], va[unit, pos] = k8[0, n], v8[0, n]
        if nq:
            q16 = call["q"][tok0:tok0 + nq][None]
            if e4:
                codes = q16[0]
            else:
                if cos is not None:
                    if per_token:
                        q16 = rotate32(q16, cos, sin, [L], inter)
                    else:
                        q16 = torch.cat([rotate32(q16[:, i:i + 1], cos, sin, [L], inter) for i in range(nq)], dim=1)
                codes = codes_of(q16, qd[b:b + 1], g)[0]
            q8[tok0:tok0 + nq] = codes.view(torch.uint8) if codes.dtype != torch.uint8 else codes
            owned[tok0:tok0 + nq] = True
    return ka, va, q8, len_eff, owned


def from_padded(call):
    """a call of tests/fp8_step_ref.build_call in this model's packed form: uniform lengths, the same tensors"""
    nb, nq, nnew = call["B"], call["nq"], call["nnew"]
    out = dict(call)
    out.update(q=call["q"].reshape(nb * nq, call["hq"], -1), k_new=call["k_new"].reshape(nb * nnew, call["hkv"], -1),
               v_new=call["v_new"].reshape(nb * nnew, call["hkv"], -1), cu_q=lengths_to_cu([nq] * nb), cu_kn=lengths_to_cu([nnew] * nb),
               max_seqlen_q=nq)
    return out


def problem(d, g, layout, dtype=torch.bfloat16, rot=None, seed=0, e4=False, packed_kn=True):
    """The GPU tests' problem at head dim d, G query heads a K/V head, as CPU tensors.  layout: "contig", "bidx" (a permutation of seven
    rows with the second sequence's index outside them), "ps16", "ps48".  rot: None or (interleaved, rotary_dim).  e4: q, k_new,
    v_new are codes.  packed_kn False: the new keys padded (B, max nnew, H_kv, d) (every sequence then appends max nnew)."""
    P = PROBLEM
    nb, hkv, cap = P["B"], P["hkv"], P["capacity"]
    hq = g * hkv
    gen = torch.Generator().manual_seed(9100 + seed + d)
    total_q, total_kn = sum(P["nq"]), sum(P["nnew"])
    nnew_pad = max(P["nnew"])
    mk = lambda *shape, s=1.0: (s * torch.randn(shape, generator=gen)).to(dtype)   # noqa: E731
    q = mk(total_q, hq, d, s=2.0)
    k_new = mk(total_kn, hkv, d, s=2.0) if packed_kn else mk(nb, nnew_pad, hkv, d, s=2.0)
    v_new = mk(total_kn, hkv, d) if packed_kn else mk(nb, nnew_pad, hkv, d)
    qd, kd, vd = (2.0 ** -6 * (1.0 + torch.rand((nb, hkv), generator=gen)) for _ in range(3))
    if e4:
        q = quantize(q.view(1, total_q, hq, d), torch.ones((1, hq)))[0]
        k_new = quantize(k_new.reshape(1, -1, hkv, d), torch.ones((1, hkv)))[0].reshape(k_new.shape)
        v_new = quantize(v_new.reshape(1, -1, hkv, d), torch.ones((1, hkv)))[0].reshape(v_new.shape)
    old_k = quantize(mk(nb, cap, hkv, d, s=2.0), kd)
    old_v = quantize(mk(nb, cap, hkv, d), vd)
    L = [min(max(x, 0), cap - (n if packed_kn else nnew_pad)) for x, n in zip(P["lens"], P["nnew"])]
    table = bidx = None
    if layout in ("ps16", "ps48"):
        ps = int(layout[2:])
        per = cap // ps
        nblk = nb * per + 2
        perm = torch.randperm(nblk, generator=gen).tolist()
        table = torch.tensor([[perm[b * per + j] for j in range(per)] for b in range(nb)], dtype=torch.int32)
        kc = torch.full((nblk, ps, hkv, d), FILL, dtype=torch.uint8)
        vc = torch.full((nblk, ps, hkv, d), FILL, dtype=torch.uint8)
        for b in range(nb):
            for t in range(L[b]):
                kc[table[b, t // ps], t % ps], vc[table[b, t // ps], t % ps] = old_k[b, t], old_v[b, t]
    else:
        rows = nb + 2 if layout == "bidx" else nb
        where = [3, 0, 6, 1, 4] if layout == "bidx" else list(range(nb))
        kc = torch.full((rows, cap, hkv, d), FILL, dtype=torch.uint8)
        vc = torch.full((rows, cap, hkv, d), FILL, dtype=torch.uint8)
        for b in range(nb):
            kc[where[b], :L[b]], vc[where[b], :L[b]] = old_k[b, :L[b]], old_v[b, :L[b]]
        if layout == "bidx":
            where[1] = rows + 1
            bidx = torch.tensor(where, dtype=torch.int32)
    cos = sin = None
    inter = False
    if rot is not None:
        inter, rdim = rot
        cos, sin = tables(cap + max(P["nq"]), rdim, dtype)
    return dict(B=nb, hq=hq, hkv=hkv, d=d, dtype=dtype, q=q, k_new=k_new, v_new=v_new, k_cache=kc, v_cache=vc,
                cache_seqlens=torch.tensor(P["lens"], dtype=torch.int32), block_table=table, cache_batch_idx=bidx, q_descale=qd,
                k_descale=kd, v_descale=vd, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, causal=True, scale=d ** -0.5,
                window=(-1, -1), softcap=0.0, sinks=None, cu_q=lengths_to_cu(P["nq"]),
                cu_kn=lengths_to_cu(P["nnew"]) if packed_kn else None, max_seqlen_q=max(P["nq"]), layout=layout)
