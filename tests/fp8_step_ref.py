"""The fp8 decode step (include/fa_mi355x.h: fa_fp8_kvcache_step; common.attention_ex.flash_attn_fp8_kvcache_step)
on the CPU (torch), composed of what the tests already have:

    TABLE, build_call(i)       B = 3, capacity 192 (contiguous, cache_batch_idx with one index out of range, pages of 16 with one table
                               entry outside the pool, strided pool views), the lengths of the issue (0, 17, 63, 64, capacity - N_new,
                               capacity + 5 and -3, both clamped), H 4 / 2 and 8 / 1, Nq and N_new in {1, 3}, bf16 and f16, rotary none /
                               NeoX / GPT-J with rotary_dim 32 / 128, num_splits 1 / 3 / 0, bare or window (20, -1) + softcap 30 + sinks
    model(call, wrong=None)    (k_after, v_after, q8, len_eff): the append (the clamp and the slot are kvcache_full_ref.front_half's,
                               which a test holds this model to; the codes kvcache_fp8_ref.quantize's), the rotation in fp32 rounded
                               once (fp8_quantize_ref.rotate32: the decode append's rounding is the contract), q's codes by
                               fp8_quantize_ref.codes_of, and the lengths after the append.  wrong: one of WRONG built in.
    attention_call(...)        the dict tests/fp8_kvcache_mod_ref.py takes: the attention over the caches as the append left them
    reference / baseline       fp8_kvcache_mod_ref.reference / baseline on that dict: the fp64 reference of the whole step and the
                               closed form with the kernel's rounding points

Caches are uint8 throughout; cache bytes no token owns are 0xA5 (a finite e4m3 code, so a rule that reads one moves the result
and does not hide in a NaN)."""
import torch

from tests import fp8_kvcache_mod_ref as fm
from tests.fp8_quantize_ref import codes_of, odd_mantissa, rotate32, tables
from tests.kvcache_fp8_ref import quantize
from tests.kvcache_rotary_ref import slot_of

B, D, CAPACITY, PS = 3, 128, 192, 16
FILL = 0xA5
WINDOW, SOFTCAP = (20, -1), 30.0
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
WRONG = ("append_unclamped", "len_eff_without_new", "q_rotated_past_new", "q_scale_per_query_head", "noncausal_q_per_token")

# heads (H_q, H_kv), nq, nnew, layout, the three lengths before the append ("full" = capacity - N_new), dtype, rotary
# (None or (interleaved, rotary_dim)), num_splits, causal, mod (window + softcap + sinks), and the forms of the q, k, v descales
# ("b": (B, H_kv), "h": (H_kv,), "-": None = 1)
_T = lambda heads, nq, nnew, layout, lens, dtype, rot, splits, causal, mod, scales="bbb": dict(   # noqa: E731
    heads=heads, nq=nq, nnew=nnew, layout=layout, lens=lens, dtype=dtype, rot=rot, splits=splits, causal=causal, mod=mod, scales=scales)
TABLE = (
    _T((4, 2), 1, 1, "contig", (0, 17, 63), "bf16", None, 1, False, False),
    _T((4, 2), 3, 3, "bidx", (64, "full", 197), "bf16", (False, 32), 3, True, False),
    _T((8, 1), 1, 3, "paged", (-3, 63, 64), "f16", (True, 128), 0, False, False),
    _T((8, 1), 3, 1, "paged_hole", (17, 197, 0), "bf16", (True, 32), 1, True, True),
    _T((4, 2), 3, 1, "strided", ("full", -3, 63), "f16", (False, 128), 3, False, True),
    _T((4, 2), 1, 3, "contig", (197, 64, 17), "f16", (True, 32), 0, True, True),
    _T((8, 1), 3, 3, "bidx", (63, 0, "full"), "f16", None, 1, False, True, "-hb"),
    _T((8, 1), 1, 1, "strided", (64, 17, -3), "bf16", (False, 128), 3, True, False),
    _T((4, 2), 3, 3, "paged", (0, 197, 63), "bf16", (True, 128), 0, False, False),
    _T((4, 2), 3, 1, "paged_hole", (63, 64, "full"), "f16", (False, 32), 3, True, False),
    _T((8, 1), 3, 3, "contig", (17, -3, 64), "bf16", (False, 32), 0, False, False, "hhh"),
    _T((4, 2), 1, 3, "strided", ("full", 0, 197), "bf16", None, 0, True, True),
)


def case_id(i):
    c = TABLE[i]
    rot = "norot" if c["rot"] is None else f"{'gptj' if c['rot'][0] else 'neox'}{c['rot'][1]}"
    return (f"{i:02d}-h{c['heads'][0]}_{c['heads'][1]}-nq{c['nq']}-new{c['nnew']}-{c['layout']}-{c['dtype']}-{rot}-S{c['splits']}-"
            f"{'causal' if c['causal'] else 'full'}{'-mod' if c['mod'] else ''}")


def build_call(i):
    """the step of TABLE[i] as CPU tensors.  The caches hold 0xA5 except for the live tokens of every sequence (quantised randn).
    bidx: five rows, the second sequence's index outside them.  paged: 12 table entries a sequence over a shuffled pool;
    paged_hole: the page the first sequence appends to lies outside the pool.  strided: K and V pools are the two halves of one
    (num_blocks, PS, 2, H_kv, 128) allocation (the GPU test makes the views; here they are two tensors)."""
    c = TABLE[i]
    g = torch.Generator().manual_seed(4200 + 17 * i)
    hq, hkv = c["heads"]
    nq, nnew, dtype = c["nq"], c["nnew"], DTYPES[c["dtype"]]
    lens = [CAPACITY - nnew if x == "full" else x for x in c["lens"]]
    L = [min(max(x, 0), CAPACITY - nnew) for x in lens]
    q = (2.0 * torch.randn((B, nq, hq, D), generator=g)).to(dtype)
    k_new = (2.0 * torch.randn((B, nnew, hkv, D), generator=g)).to(dtype)
    v_new = torch.randn((B, nnew, hkv, D), generator=g).to(dtype)
    # static descales with odd mantissas (inexact reciprocals), distinct per (sequence, K/V head)
    qd, kd, vd = (odd_mantissa(2.0 ** -6 * (1.0 + torch.rand((B, hkv), generator=g))) for _ in range(3))
    qd, kd, vd = (None if f == "-" else t[0].clone() if f == "h" else t for f, t in zip(c["scales"], (qd, kd, vd)))
    old_k = quantize((2.0 * torch.randn((B, CAPACITY, hkv, D), generator=g)).to(dtype), scales_bh(kd, B, hkv))
    old_v = quantize(torch.randn((B, CAPACITY, hkv, D), generator=g).to(dtype), scales_bh(vd, B, hkv))
    table = bidx = None
    paged = c["layout"] in ("paged", "paged_hole", "strided")
    if paged:
        per = CAPACITY // PS
        nblk = B * per + 2
        perm = torch.randperm(nblk, generator=g).tolist()
        table = torch.tensor([[perm[b * per + j] for j in range(per)] for b in range(B)], dtype=torch.int32)
        kc = torch.full((nblk, PS, hkv, D), FILL, dtype=torch.uint8)
        vc = torch.full((nblk, PS, hkv, D), FILL, dtype=torch.uint8)
        for b in range(B):
            for t in range(L[b]):
                kc[table[b, t // PS], t % PS], vc[table[b, t // PS], t % PS] = old_k[b, t], old_v[b, t]
        if c["layout"] == "paged_hole":
            table[0, L[0] // PS] = nblk + 3
    else:
        rows = B + 2 if c["layout"] == "bidx" else B
        where = [3, 0, 4] if c["layout"] == "bidx" else list(range(B))
        kc = torch.full((rows, CAPACITY, hkv, D), FILL, dtype=torch.uint8)
        vc = torch.full((rows, CAPACITY, hkv, D), FILL, dtype=torch.uint8)
        for b in range(B):
            kc[where[b], :L[b]], vc[where[b], :L[b]] = old_k[b, :L[b]], old_v[b, :L[b]]
        if c["layout"] == "bidx":
            where[1] = rows + 1
            bidx = torch.tensor(where, dtype=torch.int32)
    cos = sin = None
    inter = False
    if c["rot"] is not None:
        inter, rdim = c["rot"]
        cos, sin = tables(CAPACITY + max(0, nq - nnew), rdim, dtype)
    sinks = None
    if c["mod"]:
        sinks = 2.0 * torch.randn((hq,), generator=g, dtype=torch.float32)
        sinks[1] = float("-inf")
    return dict(B=B, hq=hq, hkv=hkv, nq=nq, nnew=nnew, dtype=dtype, q=q, k_new=k_new, v_new=v_new, k_cache=kc, v_cache=vc,
                cache_seqlens=torch.tensor(lens, dtype=torch.int32), block_table=table, cache_batch_idx=bidx, q_descale=qd, k_descale=kd,
                v_descale=vd, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, causal=c["causal"], scale=D ** -0.5,
                window=WINDOW if c["mod"] else (-1, -1), softcap=SOFTCAP if c["mod"] else 0.0, sinks=sinks, num_splits=c["splits"],
                layout=c["layout"])


def scales_bh(t, nb, hkv):
    """a descale as float32 (B, H_kv): None is 1, (H_kv,) every sequence's row"""
    if t is None:
        return torch.ones((nb, hkv), dtype=torch.float32)
    return (t[None, :].expand(nb, hkv) if t.dim() == 1 else t).float().contiguous()


def capacity(call):
    return call["block_table"].shape[1] * call["k_cache"].shape[1] if call["block_table"] is not None else call["k_cache"].shape[1]


def clamped(call):
    """L_b = clamp(cache_seqlens[b], 0, capacity - N_new)"""
    return [min(max(int(x), 0), capacity(call) - call["nnew"]) for x in call["cache_seqlens"]]


def applies(call, wrong):
    rot, nq = call["rotary_cos"] is not None, call["nq"]
    per_token = call["causal"] or call["window"][0] >= 0 or call["window"][1] >= 0
    raw = [int(x) for x in call["cache_seqlens"]]
    return {"append_unclamped": raw != clamped(call), "len_eff_without_new": True, "q_rotated_past_new": rot,
            "q_scale_per_query_head": call["hkv"] > 1, "noncausal_q_per_token": rot and nq > 1 and not per_token}[wrong]


def model(call, wrong=None):
    """(k_after, v_after uint8 in the caches' shape, q8 uint8 (B, Nq, H_q, 128), len_eff [B]) of the step; with one of WRONG built in
    (None where it changes nothing of this call)"""
    assert wrong is None or wrong in WRONG
    if wrong is not None and not applies(call, wrong):
        return None
    nb, hq, hkv, nq, nnew = call["B"], call["hq"], call["hkv"], call["nq"], call["nnew"]
    g = hq // hkv
    L = clamped(call)
    cos, sin, inter = call["rotary_cos"], call["rotary_sin"], call["rotary_interleaved"]
    per_token = call["causal"] or call["window"][0] >= 0 or call["window"][1] >= 0
    if wrong == "noncausal_q_per_token":
        per_token = True
    k16, q16 = call["k_new"], call["q"]
    if cos is not None:
        k16 = rotate32(k16, cos, sin, L, inter)
        shift = nnew if wrong == "q_rotated_past_new" else 0
        if per_token:
            q16 = rotate32(q16, cos, sin, [x + shift for x in L], inter)
        else:   # every token at L_b: one token a call of rotate32
            q16 = torch.cat([rotate32(q16[:, i:i + 1], cos, sin, [x + shift for x in L], inter) for i in range(nq)], dim=1)
    k8 = quantize(k16, scales_bh(call["k_descale"], nb, hkv))
    v8 = quantize(call["v_new"], scales_bh(call["v_descale"], nb, hkv))
    ka, va = call["k_cache"].clone(), call["v_cache"].clone()
    ps = ka.shape[1]
    first = [int(x) for x in call["cache_seqlens"]] if wrong == "append_unclamped" else L
    for b in range(nb):
        for n in range(nnew):
            t = first[b] + n
            if not 0 <= t < capacity(call):
                continue
            unit, pos = slot_of(b, t, call["block_table"], call["cache_batch_idx"], ps)
            if 0 <= unit < ka.shape[0]:
                ka[unit, pos], va[unit, pos] = k8[b, n], v8[b, n]
    qd = scales_bh(call["q_descale"], nb, hkv)
    if wrong == "q_scale_per_query_head":   # query head h takes the scale of K/V head h % H_kv
        q8 = codes_of(q16, qd[:, torch.arange(hq) % hkv], 1)
    else:
        q8 = codes_of(q16, qd, g)
    len_eff = [x + (0 if wrong == "len_eff_without_new" else nnew) for x in L]
    return ka, va, q8, len_eff


def attention_call(call, k_after, v_after, q8, len_eff):
    """the fp8 decode call over the caches as the append left them, as tests/fp8_kvcache_mod_ref.py takes it"""
    return dict(B=call["B"], hq=call["hq"], hkv=call["hkv"], nq=call["nq"], causal=call["causal"], dtype=call["dtype"], scale=call["scale"],
                num_splits=call["num_splits"], q8=q8, k_cache=k_after, v_cache=v_after,
                cache_seqlens=torch.tensor(len_eff, dtype=torch.int32), block_table=call["block_table"],
                cache_batch_idx=call["cache_batch_idx"], q_descale=call["q_descale"], k_descale=call["k_descale"],
                v_descale=call["v_descale"], values="normal", window=tuple(call["window"]), softcap=call["softcap"], sinks=call["sinks"])


def reference(call, wrong=None):
    """the fp64 reference of the whole step (a Result in the kernel's row order); None where `wrong` does not apply"""
    m = model(call, wrong)
    return None if m is None else fm.reference(attention_call(call, *m))


def baseline(call):
    """the closed form with the attention kernel's rounding points, on the right model"""
    return fm.baseline(attention_call(call, *model(call)))
