"""FlashAttention-3's fp8 call (csrc/fa_fp8_inputs.hip, fa_fp8_forward in csrc/fa_capi.hip) on the CPU (torch), for the
table of tests/fp8_inputs_cases.py:

    reference(call)          fp64 attention of code * descale, with the GQA rule, the shifted diagonal and dead rows
    baseline(call)           the same closed form with the kernel's rounding points and nothing else of it
    expected_v8t(call)       the bytes fp8in_vt_kernel writes into the workspace
    mutant(call, name)       the fp64 evaluation with one plausible kernel bug built in (MUTANTS)

`call` is the dict of tests.fp8_inputs_cases.build_call: B, hq, hkv, nq, nk, causal, dtype (of o), scale, q8 (B, H_q, Nq, 128), k8, v8
(B, H_kv, Nk, 128) uint8 e4m3 codes, q_descale / k_descale / v_descale as the caller passes them (None, (B, H_kv) or (H_kv,) float32).
Results are tests/ex_full_ref.py's Result with units (B * H_q, Nq, .); _mfma_f8, e4m3_code / e4m3_value, the V^T key-of-byte map,
_PV_KEY_OF_K and tiled_sharp_bar are tests/fp8_ref.py's, unchanged.

The baseline's rounding points, each read from the code (all in csrc/fa_fp8_inputs.hip, fwd_fp8in_kernel unless named otherwise):
  * raw scores: __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4 on the e4m3 codes with unit scales, two instructions per score,
    float32 accumulation — fp8_ref._mfma_f8 with its truncation;
  * f = (c_log2 * q_descale) * k_descale, float products in that order (`f`), with c_log2 = float(softmax_scale) * 1.4426950408889634f
    (launch_fp8_inputs: `a.c_log2`);
  * the maximum of the RAW scores of a 128-key tile, times f once (`mx = mx * f`);
  * the lazy rescale per 32-row wave (`__any(m_new - m_run > 8.0f)`), a row without a visible key so far keeping m_use = 0;
  * p = exp2(fma(s, f, -m_use)) (`__builtin_amdgcn_exp2f(fmaf(sacc, f, -m_use))`); 128-key tiles;
  * P rounded to e4m3, RNE, on every row (`__builtin_amdgcn_cvt_pk_fp8_f32`), and P.V on the same instruction, 64 keys at a time
    in the key order of fp8_ref._PV_KEY_OF_K (fp8in_vt_kernel gives V^T that permutation);
  * l from the unrounded float p (`rs += p`);
  * the epilogue: inv = v_descale * (1 / l), o = RNE(acc * inv) to the output dtype (`pack2_rn`), lse = (m + log2 l) * ln 2 in float;
    a row with l = 0 gives o = 0 and lse = -inf (`dead`).
With float64 and no rounding the baseline is the reference again (tests/test_fp8_inputs_cpu.py, 1e-10)."""
import torch

from tests.ex_full_ref import NEG_INF, Result, _fma, _mm, round_to
from tests.fp8_ref import LN2_F, LOG2E_F, _PV_KEY_OF_K, _mfma_f8, _v8t_key_of_byte, e4m3_code, e4m3_value

ROW_TILE = 256
KEY_TILE = 128
MUTANTS = ("kv_head_modulo", "causal_top_left", "v_descale_dropped", "descales_of_batch_0", "tail_keys_dropped", "v8t_without_permutation",
           "p_truncated", "rowsum_from_rounded_p", "diagonal_off_by_4")


def _result(o, lse):
    return Result(o, lse, None, None, None, None, None, None, None, None, None)


def descales(call):
    """q, k, v descales as (B, H_kv) float32 (None: ones; (H_kv,): every batch the same row)"""
    out = []
    for name in ("q_descale", "k_descale", "v_descale"):
        t = call[name]
        if t is None:
            t = torch.ones((call["B"], call["hkv"]), dtype=torch.float32)
        elif t.dim() == 1:
            t = t[None, :].expand(call["B"], call["hkv"])
        out.append(t.float().contiguous())
    return out


def kv_unit(call, mutant=None):
    """(B * H_q,) the K/V unit b * H_kv + h / (H_q / H_kv) of every query unit"""
    u = torch.arange(call["B"] * call["hq"])
    b, h = u // call["hq"], u % call["hq"]
    hk = h % call["hkv"] if mutant == "kv_head_modulo" else h // (call["hq"] // call["hkv"])
    return b * call["hkv"] + hk


def visible(call, mutant=None):
    """(Nq, Nk) bool: row i sees key j <= i + Nk - Nq under the mask (bottom-right aligned)"""
    nq, nk = call["nq"], call["nk"]
    vis = torch.ones((nq, nk), dtype=torch.bool)
    if call["causal"]:
        i, j = torch.arange(nq)[:, None], torch.arange(nk)[None, :]
        c = 0 if mutant == "causal_top_left" else nk - nq
        vis = j <= i + c
        if mutant == "diagonal_off_by_4":          # the mask threshold off by 4 inside the row's 64-key block of the diagonal
            vis = vis | ((j <= i + c + 4) & (j // 64 == (i + c) // 64))
    if mutant == "tail_keys_dropped" and nk % 64:
        vis = vis.clone()
        vis[:, nk - nk % 64:] = False
    return vis


def dequantised(call, mutant=None):
    """fp64 q (B * H_q, Nq, 128), k, v (B * H_kv, Nk, 128): code * descale, and the scale"""
    qd, kd, vd = descales(call)
    if mutant == "descales_of_batch_0":
        qd, kd, vd = (t[:1].expand_as(t) for t in (qd, kd, vd))
    if mutant == "v_descale_dropped":
        vd = torch.ones_like(vd)
    g = call["hq"] // call["hkv"]
    q = e4m3_value(call["q8"]).double() * qd.double().repeat_interleave(g, dim=1)[:, :, None, None]
    k = e4m3_value(call["k8"]).double() * kd.double()[:, :, None, None]
    v = e4m3_value(call["v8"]).double() * vd.double()[:, :, None, None]
    return q.reshape(-1, call["nq"], 128), k.reshape(-1, call["nk"], 128), v.reshape(-1, call["nk"], 128)


def _softmax_pv(s, v):
    """(o, lse) of masked logits s (U, Nq, Nk) fp64 and v (U, Nk, d): rows without a visible key give o = 0, lse = -inf (the arithmetic
    of ex_full_ref._attend)"""
    live = (s > NEG_INF).any(-1, keepdim=True)
    p = torch.softmax(torch.where(live, s, torch.zeros((), dtype=torch.float64)), -1) * live
    llive = live.squeeze(-1)
    lse = torch.where(llive, torch.logsumexp(torch.where(live, s, torch.zeros((), dtype=torch.float64)), -1),
                      torch.tensor(NEG_INF, dtype=torch.float64))
    return p @ v, lse


def reference(call, mutant=None):
    """Result (o, lse fp64) of softmax(scale * (q8 q_descale)(k8 k_descale)^T [causal]) (v8 v_descale)"""
    q, k, v = dequantised(call, mutant)
    kvi = kv_unit(call, mutant)
    s = _mm(q, k[kvi].transpose(1, 2)) * call["scale"]
    s = torch.where(visible(call, mutant), s, torch.tensor(NEG_INF, dtype=torch.float64))
    o, lse = _softmax_pv(s, v[kvi])
    return _result(o, lse)


def ex_call(call):
    """the call on the dequantised tensors as a dict tests/ex_full_ref.full_reference takes"""
    q, k, v = dequantised(call)
    return dict(q=q, k=k, v=v, do=torch.zeros_like(q), dlse=None, sinks=None, alibi_slopes=None, layout="padded",
                heads=(call["hq"], call["hkv"]), dropout_p=0.0, seed=0, causal=call["causal"], window=(-1, -1), mask=None, block_mask=None,
                br=0, bc=0, softcap=0.0, scale=call["scale"])


def expected_v8t(call):
    """uint8 (B * H_kv, ntile, 128 d rows, 128 key bytes): byte b of d row r of tile t is v8[128 t + key_of_byte(b), r], zero for keys
    >= Nk (fp8in_vt_kernel: `pos`, and the zeroed second half of an odd last tile)"""
    nk = call["nk"]
    ntile = (nk + 127) // 128
    v = call["v8"].reshape(-1, nk, 128)
    pad = torch.zeros((v.shape[0], ntile * 128, 128), dtype=torch.uint8)
    pad[:, :nk] = v
    t = pad.reshape(-1, ntile, 128, 128)[:, :, _v8t_key_of_byte(), :]          # [unit][tile][byte][d]
    return t.transpose(2, 3).contiguous()


def workspace_bytes(call):
    """include/fa_mi355x.h, fa_fp8_forward_workspace_bytes"""
    return call["B"] * call["hkv"] * ((call["nk"] + 127) // 128) * 128 * 128 + 256


def baseline(call, compute=torch.float32, rounding=True, trace=None):
    """Result (o, lse in `compute`) of the closed form with the kernel's rounding points (module docstring).  rounding=False: no
    rounding of P and o and no truncation in the matrix instruction (with compute = float64: the reference again).  trace: a list
    that receives, per query tile and key tile, (key tile, first row, moved (U, rows) bool: the row's wave rescaled, stale (U, rows)
    bool: the row's own max grew but its wave did not move)."""
    ct = compute
    f32 = ct == torch.float32
    B, hq, nq, nk = call["B"], call["hq"], call["nq"], call["nk"]
    U = B * hq
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    kvi = kv_unit(call)
    q8 = e4m3_value(call["q8"]).to(ct).reshape(U, nq, 128)
    k8 = e4m3_value(call["k8"]).to(ct).reshape(-1, nk, 128)[kvi]
    v8 = e4m3_value(call["v8"]).to(ct).reshape(-1, nk, 128)[kvi]
    qd, kd, vd = (t.reshape(-1)[kvi].to(ct) for t in descales(call))
    if f32:
        c_log2 = torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)
        ln2 = torch.tensor(LN2_F, dtype=torch.float32)
    else:
        c_log2, ln2 = torch.tensor(call["scale"] * LOG2E_F, dtype=ct), torch.tensor(LN2_F, dtype=ct)
    f = ((c_log2 * qd) * kd)[:, None, None]                                        # (U, 1, 1): one factor per workgroup
    zero, one, ninf = torch.zeros((), dtype=ct), torch.ones((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    vis_all = visible(call)
    shift = nk - nq
    o = torch.zeros((U, nq, 128), dtype=ct)
    lse = torch.zeros((U, nq), dtype=ct)
    for r0 in range(0, nq, ROW_TILE):
        r1 = min(r0 + ROW_TILE, nq)
        nr = r1 - r0
        vis = vis_all[r0:r1]
        sacc = _mfma_f8(q8[:, r0:r1], k8.transpose(1, 2), ct, torch.zeros((U, nr, nk), dtype=ct), rounding)
        sacc = torch.where(vis, sacc, ninf)
        kend = max(0, min(nk, r0 + ROW_TILE + shift)) if call["causal"] else nk
        m = torch.full((U, nr), NEG_INF, dtype=ct)
        l_ = torch.zeros((U, nr), dtype=ct)
        acc = torch.zeros((U, nr, 128), dtype=ct)
        for t0 in range(0, kend, KEY_TILE):
            sl = slice(t0, min(t0 + KEY_TILE, nk))
            mx = sacc[..., sl].max(-1).values * f[:, :, 0]
            m_new = torch.maximum(m, mx)
            grow = m_new - m > 8.0                                                  # (first visible key: inf > 8; none yet: nan > 8 is False)
            pad = (-nr) % 32
            gw = torch.nn.functional.pad(grow, (0, pad)).reshape(U, -1, 32).any(-1, keepdim=True).expand(U, -1, 32).reshape(U, -1)[:, :nr]
            if trace is not None:
                trace.append((t0 // KEY_TILE, r0, gw.clone(), (m_new > m) & ~gw))
            m_use = torch.where(gw, m_new, m)
            m_use = torch.where(m_use > NEG_INF, m_use, zero)
            alpha = torch.where(gw, torch.exp2(m - torch.where(m_new > NEG_INF, m_new, zero)), one)
            m = torch.where(gw, m_new, m)
            l_ = l_ * alpha
            acc = acc * alpha.unsqueeze(-1)
            p = torch.exp2(_fma(sacc[..., sl], f.expand(U, nr, sl.stop - sl.start), -m_use.unsqueeze(-1).expand(U, nr, sl.stop - sl.start), ct))
            acc = _mfma_f8(p8(p), v8[:, sl], ct, acc, rounding, order=_PV_KEY_OF_K)
            l_ = l_ + p.sum(-1)
        dead = l_ == 0
        inv = vd[:, None] * (1.0 / l_)
        o[:, r0:r1] = torch.where(dead.unsqueeze(-1), zero, rnd(acc * inv.unsqueeze(-1)))
        lse[:, r0:r1] = torch.where(dead, ninf, (m + torch.log2(l_)) * ln2)
    return _result(o, lse)


def rounded(res, dtype):
    """a Result as the kernel returns it: o in dtype, lse float32"""
    return res._replace(o=res.o.to(dtype), lse=res.lse.float())


def mutant(call, name):
    """the fp64 Result with one bug built in, or None where the bug does not apply to the call (it changes nothing):
      kv_head_modulo           query head h reads K/V head h % H_kv
      causal_top_left          the diagonal aligned top-left: row i sees j <= i
      v_descale_dropped        o without v_descale
      descales_of_batch_0      every batch scaled with batch 0's three descales
      tail_keys_dropped        the last Nk % 64 keys never visited
      v8t_without_permutation  V^T written in key order: inside every 64-key group the probability of key _PV_KEY_OF_K[k] meets the
                               value of key k
      p_truncated              p = exp2(s - rowmax) truncated toward zero to e4m3 before P.V
      rowsum_from_rounded_p    l (o's divisor and lse) from the e4m3-rounded p
      diagonal_off_by_4        under the mask a row also sees up to 4 keys above its diagonal inside the diagonal's 64-key block"""
    assert name in MUTANTS
    hq, hkv, nq, nk, causal = call["hq"], call["hkv"], call["nq"], call["nk"], call["causal"]
    if name == "kv_head_modulo" and (hq == hkv or hkv == 1):
        return None
    if name in ("causal_top_left", "diagonal_off_by_4") and not causal:
        return None
    if name == "causal_top_left" and nq == nk:
        return None
    if name == "v_descale_dropped" and call["v_descale"] is None:
        return None
    if name == "descales_of_batch_0" and all(call[n] is None or call[n].dim() == 1 for n in ("q_descale", "k_descale", "v_descale")):
        return None
    if name == "tail_keys_dropped" and (nk % 64 == 0 or nk < 64):
        return None
    if name in ("kv_head_modulo", "causal_top_left", "v_descale_dropped", "descales_of_batch_0", "tail_keys_dropped", "diagonal_off_by_4"):
        return reference(call, name)
    q, k, v = dequantised(call)
    kvi = kv_unit(call)
    s = _mm(q, k[kvi].transpose(1, 2)) * call["scale"]
    s = torch.where(visible(call), s, torch.tensor(NEG_INF, dtype=torch.float64))
    vu = v[kvi]
    if name == "v8t_without_permutation":
        pad = (-nk) % 64
        sp = torch.nn.functional.pad(s, (0, pad), value=NEG_INF)
        vp = torch.nn.functional.pad(vu, (0, 0, 0, pad))
        key_of_k = (torch.arange(0, nk + pad, 64)[:, None] + _PV_KEY_OF_K[None, :]).reshape(-1)
        o, _ = _softmax_pv(sp[..., key_of_k], vp)
        return _result(o, reference(call).lse)
    live = (s > NEG_INF).any(-1, keepdim=True)
    mrow = torch.where(live, s.max(-1, keepdim=True).values, torch.zeros((), dtype=torch.float64))
    p = torch.exp(s - mrow)
    codes = e4m3_code(p.float())
    pr = e4m3_value(codes).double()
    if name == "p_truncated":
        down = pr > p
        pr = e4m3_value((codes.to(torch.int16) - down.to(torch.int16)).clamp_min(0).to(torch.uint8)).double()
        l_ = p.sum(-1)
    else:
        l_ = pr.sum(-1)
    dead = ~live.squeeze(-1)
    o = torch.where(dead.unsqueeze(-1), torch.zeros((), dtype=torch.float64), (pr @ vu) / l_.clamp_min(1e-300).unsqueeze(-1))
    lse = torch.where(dead, torch.tensor(NEG_INF, dtype=torch.float64), mrow.squeeze(-1) + torch.log(l_.clamp_min(1e-300)))
    return _result(o, lse)
