"""The FA3 fp8 path (csrc/fa_fwd_fp8.hip and the fp8 branches of fa3_forward / fa3_backward in csrc/fa_capi.hip) cut at
the caller's workspace, on the CPU (torch + numpy), for the table of tests/fp8_cases.py:

    ws_layout(bh, n, d, dtype, direction)   offsets and sizes of every region of the forward / backward workspace
    parse_forward_ws(bytes, call)           the regions of a d = 128 forward workspace as tensors (`ws_contents`)
    quantise / quantise_v / roundtrip       float32 transcriptions of the three quantisers: what they write, bit for bit
    expected_ws(call)                       ws_contents by the transcriptions alone (no GPU)
    reference(ws_contents, call)            fp64 attention of the dequantised tensors as the workspace holds them
    baseline(ws_contents, call)             the same closed form with the two kernels' rounding points and nothing else of them
    mutant(ws_contents, call, name)         the fp64 evaluation with one plausible kernel bug built in (MUTANTS)

The quantisers are judged on their bytes, the attention kernels on the bytes they actually read; neither is excused by the other.
`call` is the dict of tests.fp8_cases.build_call.  _mm, _fma, round_to, sharp_bar and Result are tests/ex_full_ref.py's.

The baseline's rounding points, each read from the code (all in csrc/fa_fwd_fp8.hip):
  * raw scores accumulated in float32, 64 terms per instruction (fwd_fp8_kernel / fwd_fp8v_kernel:
    __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4 on e4m3 codes with unit scales, two instructions per score).  The instruction
    was first modelled as ONE float32 rounding (the exact sum of its 64 products added to the accumulator and rounded once); the
    MI355X showed that its sum is not exact, and _mfma_f8 now has what was measured: groups of 8 products aligned to the group's
    largest exponent and truncated toward zero 13 bits below it, then one float32 rounding per instruction.  The P.V product of
    fwd_fp8v_kernel is the same instruction and takes the same model;
  * score scales: fq = sq[block of the wave's 32 rows] * c_log2 with c_log2 = float(scale) * 1.4426950408889634f, then
    f = fq * sk[block], float products in that order (both kernels: `fq`, `f` / `f0`, `f1`);
  * fwd_fp8_kernel: s = sacc * f rounded once, the max of s, p = exp2(s - m_use); 64-key tiles; P rounded to the tensor dtype
    (pack2: RNE) before P.V, 16 terms per instruction (mfma32), V~ the 16-bit slab;
  * fwd_fp8v_kernel: the max is max(mx0 * f0, mx1 * f1) over the raw maxima of the tile's two 64-key blocks,
    p = exp2(fma(sacc, f, -m_use)); 128-key tiles; P rounded to e4m3 (cvt_pk_fp8_f32: RNE) relative to m_use; P.V on e4m3 codes,
    64 keys per instruction, the V block's power of two applied exactly (the instruction's E8M0 scale operand);
  * both: the lazy rescale (the running max moves only on a tile where some row of the wave's 32 grew by more than 8 in log2
    units; the other rows keep a stale max: ex_full_ref.Model.lazy_rescale), l from the unrounded float p, o = RNE(acc * (1 / l)),
    lse = (m_run + log2(l)) * 0.6931471805599453f.
With float64 and no rounding the baseline is the reference again (tests/test_fp8_sharp_cpu.py, 1e-10)."""
import numpy as np
import torch

from tests.ex_full_ref import NEG_INF, Result, _fma, _mm, round_to, sharp_bar

E4M3_MAX = 448.0
LOG2E_F = 1.4426950408889634
LN2_F = 0.6931471805599453
SENTINEL = 0x7F                       # e4m3 NaN; as a float or 16-bit pattern ~3.4e38
ROW_TILE = 256                        # query rows per workgroup of both attention kernels
MUTANTS = ("o_times_1.2", "o_plus_0.05", "lse_plus_1.5e-2", "k_scale_of_previous_block", "q_scale_per_workgroup",
           "both_halves_scored_with_f0", "both_v_halves_with_e0", "v_exponent_off_by_one", "p_truncated", "rowsum_from_rounded_p",
           "tail_keys_dropped", "diagonal_block_visible", "e4m3_rows_read_the_slab")


def _align(x, a=256):
    return (x + a - 1) // a * a


def slab_bytes(bh, n, d):
    """one round-tripped 16-bit tensor (fa_capi.hip, slab_bytes)"""
    return _align(bh * n * d * 2)


def rows16(call):
    """[0, r): the query rows fwd_fp8_kernel (16-bit P.V) serves; the rest are fwd_fp8v_kernel's (fa_fwd_fp8.hip, launch_fp8_t: pv16,
    nqt16; fp8_v_pow2)"""
    n = call["n"]
    if n <= 256 or call["fp8_pv"] == 1:
        return n
    return min(n, ROW_TILE) if call["causal"] else 0


def v_pow2(call):
    """fa_fwd_fp8.hip, fp8_v_pow2: d = 128, option fp8_pv != 1, N > 256"""
    return call["d"] == 128 and call["fp8_pv"] != 1 and call["n"] > 256


def vrows(call):
    """rows of the V~ slab the d = 128 forward fills (launch_fp8_t: vrows)"""
    n = call["n"]
    if not v_pow2(call):
        return n
    return min(n, 256) if call["causal"] else 0


def ws_layout(bh, n, d, dtype, direction, plain_bytes=0):
    """{region: (offset, bytes)} and "total" of the workspace of fa3_forward(fp8 = 1) (`direction` "forward") or fa3_backward
    ("backward"; plain_bytes = fa_backward_workspace_bytes(bh, n, d, dtype), the plain backward's own part).  Transcribes
    fa_fwd_fp8.hip fp8_ws_layout, fa_capi.hip slab_bytes and the layouts in fa3_forward / fa3_backward /
    fa3_forward_workspace_bytes / fa3_backward_workspace_bytes.  d = 128 forward: [V~ slab][q8][k8][pad][sq][sk][svexp][pad][v8t]
    [256 tail]; other head dims: [Q~][K~][V~]; backward: [Q~][K~][V~][plain]."""
    assert dtype in (torch.float16, torch.bfloat16) and d % 8 == 0 and 8 <= d <= 256
    slab = slab_bytes(bh, n, d)
    if direction == "backward":
        return {"qt": (0, bh * n * d * 2), "kt": (slab, bh * n * d * 2), "vt": (2 * slab, bh * n * d * 2), "plain": (3 * slab, plain_bytes),
                "total": 3 * slab + plain_bytes}
    assert direction == "forward"
    if d != 128:
        return {"qt": (0, bh * n * d * 2), "kt": (slab, bh * n * d * 2), "vt": (2 * slab, bh * n * d * 2), "total": 3 * slab}
    nb, ntile, nbytes = (n + 63) // 64, (n + 127) // 128, bh * n * d
    off = _align(2 * nbytes)
    off2 = _align(off + 12 * bh * nb)
    return {"vt": (0, bh * n * d * 2), "q8": (slab, nbytes), "k8": (slab + nbytes, nbytes), "sq": (slab + off, 4 * bh * nb),
            "sk": (slab + off + 4 * bh * nb, 4 * bh * nb), "svexp": (slab + off + 8 * bh * nb, 4 * bh * nb),
            "v8t": (slab + off2, bh * ntile * 128 * 128), "total": slab + off2 + bh * ntile * 128 * 128 + 256}


def untouched(buf, layout):
    """the bytes of a workspace buffer (uint8, 1-D) that belong to no region — pads and the tail — as one tensor"""
    keep = torch.ones(layout["total"], dtype=torch.bool)
    for name, region in layout.items():
        if name != "total":
            keep[region[0]:region[0] + region[1]] = False
    return buf[:layout["total"]][keep]


# ---- decoders

def e4m3_value(codes):
    """uint8 e4m3 codes -> float32 values (exact)"""
    return codes.contiguous().view(torch.float8_e4m3fn).float()


def e4m3_code(x):
    """float32 -> uint8 e4m3 codes, round to nearest even (v_cvt_pk_fp8_f32)"""
    return x.float().to(torch.float8_e4m3fn).view(torch.uint8)


def _v8t_key_of_byte():
    """key within a 128-key tile of byte b of a d row: within each 64-key group byte 32 hi + 16 h + jj is key
    32 hi + 4 h + (jj & 3) + 8 (jj >> 2) (fa_fwd_fp8.hip, the comment above fp8_quant_v_kernel)"""
    b = torch.arange(128)
    grp, w = b // 64, b % 64
    hi, h, jj = w // 32, (w % 32) // 16, w % 16
    return 64 * grp + 32 * hi + 4 * h + (jj & 3) + 8 * (jj >> 2)


def decode_v8t(v8t, bh, n):
    """the v8t region (uint8, bh * ntile * 128 * 128) -> codes (bh, ntile * 128, 128) [key][d]: undo the transposed tile layout
    [tile][d row][128 key bytes] and the key permutation"""
    ntile = (n + 127) // 128
    t = v8t.reshape(bh, ntile, 128, 128)                      # [bh][tile][d row][byte]
    out = torch.empty((bh, ntile, 128, 128), dtype=torch.uint8)      # [bh][tile][key][d]
    out[:, :, _v8t_key_of_byte(), :] = t.transpose(2, 3)
    return out.reshape(bh, ntile * 128, 128)


def svexp_scale(svexp):
    """E8M0 exponents (int32) -> 2^(e - 127) as float64"""
    return torch.exp2(svexp.double() - 127.0)


def per_row(scales, n):
    """(bh, nb) block values -> (bh, n, 1) per row"""
    return torch.repeat_interleave(scales, 64, dim=1)[:, :n, None]


def dequant(codes, scales):
    """codes (bh, n, d) uint8 x per-64-row-block scales (bh, nb) -> float64"""
    return e4m3_value(codes).double() * per_row(scales.double(), codes.shape[1])


def parse_forward_ws(buf, call):
    """ws_contents of a d = 128 forward workspace (uint8 CPU tensor): q8, k8 (bh, n, 128) uint8; sq, sk (bh, nb) float32; svexp
    (bh, nb) int32; v8 (bh, ntile * 128, 128) uint8 codes [key][d] and v8t_raw; vt (bh, n, 128) 16-bit, rows >= vrows(call) as found"""
    bh, n, d, dt = call["bh"], call["n"], call["d"], call["dtype"]
    lay = ws_layout(bh, n, d, dt, "forward")
    cut = lambda name: buf[lay[name][0]:lay[name][0] + lay[name][1]].clone()   # noqa: E731
    nb = (n + 63) // 64
    return dict(q8=cut("q8").reshape(bh, n, d), k8=cut("k8").reshape(bh, n, d), sq=cut("sq").view(torch.float32).reshape(bh, nb),
                sk=cut("sk").view(torch.float32).reshape(bh, nb), svexp=cut("svexp").view(torch.int32).reshape(bh, nb),
                v8t_raw=cut("v8t"), v8=decode_v8t(cut("v8t"), bh, n), vt=cut("vt").view(dt).reshape(bh, n, d))


# ---- the quantisers in float32, in the kernels' order

def rot_sign(d):
    """fa_fwd_fp8.hip, rot_sign: the fixed +-1 vector (oracle.attention_oracle.incoherent_signs)"""
    e = np.arange(d, dtype=np.uint64)
    h = ((e * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(27)
    return torch.from_numpy(1.0 - 2.0 * ((np.uint64(0x5A3C96E1) >> h) & np.uint64(1)).astype(np.float32)).float()


def butterfly(x):
    """fa_fwd_fp8.hip, hadamard_row / the two loops of fp8_roundtrip_kernel: element e = 8 ch + j; three in-register stages over j
    (st = 1, 2, 4: x[j] = a + b, x[j | st] = a - b), then log2(d / 8) cross-lane stages over the chunk index
    ((ch & bit) ? other - x : x + other).  Both are `low + high` and `low - high` of the pair that differs in one bit of e,
    stage by stage from bit 0 up, each a single rounded operation in x's dtype."""
    d = x.shape[-1]
    st = 1
    while st < d:
        y = x.reshape(x.shape[:-1] + (d // (2 * st), 2, st))
        lo, hi = y[..., 0, :], y[..., 1, :]
        x = torch.stack((lo + hi, lo - hi), dim=-2).reshape(x.shape)
        st *= 2
    return x


def rs_of(d, kernel):
    """the factor after the butterfly: the literal 0.08838834764831845f in fp8_quant_kernel (d = 128), rsqrtf((float)d) in
    fp8_roundtrip_kernel — taken here as the correctly rounded float of d^-0.5 (not known for the device's rsqrtf unless d is a
    power of four, where it is exact)"""
    return torch.tensor(0.08838834764831845 if kernel == "quant" else float(d) ** -0.5, dtype=torch.float32)


def pow2_scale_exp(amax):
    """fa_fwd_fp8.hip, pow2_scale_exp: e = exponent field of float(amax / 448) - 127, + 1 if 2^e * 448 < amax, clamped to [-126, 126]"""
    quo = (amax.float() / torch.tensor(E4M3_MAX, dtype=torch.float32)).contiguous()
    e = ((quo.view(torch.int32) >> 23) & 0xFF) - 127
    e = e + (torch.exp2(e.float()) * E4M3_MAX < amax).to(torch.int32)
    return e.clamp(-126, 126)


def _blocks(x):
    """(bh, n, d) -> (bh, nb, 64, d) with rows >= n as zeros (the kernels load them as zeros)"""
    bh, n, d = x.shape
    nb = (n + 63) // 64
    return torch.nn.functional.pad(x, (0, 0, 0, nb * 64 - n)).reshape(bh, nb, 64, d)


def quantise(x, rot, pow2=False, kernel="quant"):
    """dict(codes (bh, n, d) uint8, scale (bh, nb) float32, quo (bh, n, d) float32 the float quotient that was rounded, exact
    (bh, n, d) bool: the quotient is the exact one) of a 16-bit tensor, as fp8_quant_kernel (kernel = "quant": Q and K of the
    d = 128 forward) and the first half of fp8_roundtrip_kernel ("roundtrip") compute them: [signs, butterfly, * rs], block amax
    over 64 rows (rows >= N zeros), max(amax, 1e-6f), scl = amax / 448 as one correctly rounded division (__fdiv_rn) or 2^e of
    pow2_scale_exp, codes = RNE e4m3 of the float quotient x / scl (cvt_pk_e4m3_div)."""
    bh, n, d = x.shape
    xf = x.float()
    if rot:
        xf = butterfly(xf * rot_sign(d)) * rs_of(d, kernel)
    xb = _blocks(xf)
    amax = torch.clamp_min(xb.abs().amax(dim=(2, 3)), torch.tensor(1e-6, dtype=torch.float32))
    scl = amax / torch.tensor(E4M3_MAX, dtype=torch.float32)
    if pow2:
        scl = torch.exp2(pow2_scale_exp(amax).float())
    quo = (xb / scl[:, :, None, None]).reshape(bh, -1, d)[:, :n]
    exact = quo.double() * per_row(scl.double(), n) == xf.double()
    return dict(codes=e4m3_code(quo), scale=scl, quo=quo, exact=exact, rotated=xf)


def quantise_v(v):
    """dict(codes, svexp (bh, nb) int32 = e + 127, scale = 2^e) as fp8_quant_v_kernel computes them: e = pow2_scale_exp(max(amax,
    1e-6f)), codes = RNE e4m3 of the product x * 2^-e, which is exact"""
    xb = _blocks(v.float())
    amax = torch.clamp_min(xb.abs().amax(dim=(2, 3)), torch.tensor(1e-6, dtype=torch.float32))
    e = pow2_scale_exp(amax)
    inv = torch.exp2(-e.float())
    codes = e4m3_code((xb * inv[:, :, None, None]).reshape(v.shape[0], -1, v.shape[2])[:, :v.shape[1]])
    return dict(codes=codes, svexp=e + 127, scale=torch.exp2(e.float()))


def inverse_rotation64(y):
    """fp64: y . H . diag(s) / sqrt(d), the transpose of the rotation (exact arithmetic up to fp64 rounding)"""
    d = y.shape[-1]
    return butterfly(y.double()) * (float(d) ** -0.5) * rot_sign(d).double()


def rotation64(x):
    d = x.shape[-1]
    return butterfly(x.double() * rot_sign(d).double()) * (float(d) ** -0.5)


def roundtrip(x, rot, pow2=False):
    """dict(out (bh, n, d) in x's dtype, out64 the fp64 inverse rotation of codes x scale, q = quantise(...)) as
    fp8_roundtrip_kernel (and fp8_quant_kernel<OUT16>) write it: y = code * scl as one float multiply; rotated tensors: the
    butterfly back, then * (rs * sign); then RNE to the tensor dtype"""
    q = quantise(x, rot, pow2, kernel="roundtrip")
    n, d = x.shape[1], x.shape[2]
    y = e4m3_value(q["codes"]) * per_row(q["scale"], n)
    y64 = e4m3_value(q["codes"]).double() * per_row(q["scale"].double(), n)
    if rot:
        y = butterfly(y) * (rs_of(d, "roundtrip") * rot_sign(d))
        y64 = inverse_rotation64(y64)
    return dict(out=y.to(x.dtype), out64=y64, q=q)


def near_ties(q):
    """(bh, n, d) bool: elements whose float quotient is inexact and lies within 4 float ulps of the midpoint of two neighbouring
    e4m3 values — the only ones a division that is an ulp off may round the other way (by one e4m3 step)"""
    quo = q["quo"]
    a = quo.abs().double().clamp_max(E4M3_MAX)
    val = e4m3_value(q["codes"]).abs().double()
    code = (q["codes"] & 0x7F).to(torch.int16)
    up = e4m3_value((code + 1).clamp_max(0x7E).to(torch.uint8)).double()
    dn = e4m3_value((code - 1).clamp_min(0).to(torch.uint8)).double()
    ulp = torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -126))) - 23.0)
    near = (((a - (val + up) / 2).abs() <= 4 * ulp) & (code < 0x7E)) | (((a - (val + dn) / 2).abs() <= 4 * ulp) & (code > 0))
    return near & ~q["exact"]


def code_steps(a, b):
    """|a - b| in e4m3 steps for two uint8 code tensors (sign-magnitude order)"""
    key = lambda c: torch.where(c >= 0x80, -(c.to(torch.int16) - 0x80), c.to(torch.int16))   # noqa: E731
    return (key(a) - key(b)).abs()


def compare_codes(got, q, what):
    """the bitwise rule with its permitted near-tie differences: list of failures (empty: passed) and the number of differing
    elements.  An element may differ only where near_ties holds, then by one e4m3 step, at most 8 per tensor."""
    diff = got != q["codes"]
    nd = int(diff.sum())
    bad = []
    if nd:
        if nd > 8:
            bad.append(f"{what}: {nd} codes differ from the transcription (at most 8 near-tie elements may)")
        if bool((diff & ~near_ties(q)).any()):
            bad.append(f"{what}: {int((diff & ~near_ties(q)).sum())} codes differ where the quotient is no near tie")
        if int(code_steps(got, q["codes"])[diff].max()) > 1:
            bad.append(f"{what}: a code differs by more than one e4m3 step")
    return bad, nd


def expected_ws(call):
    """ws_contents of the d = 128 forward by the transcriptions alone (what parse_forward_ws must find); regions the call leaves
    unwritten hold the sentinel.  Also "quant": the quantise() records of q and k."""
    bh, n, d, dt = call["bh"], call["n"], call["d"], call["dtype"]
    assert d == 128
    rot = call["fp8_rot"] != 2
    qq, qk = quantise(call["q"], rot), quantise(call["k"], rot)
    nb, ntile = (n + 63) // 64, (n + 127) // 128
    sent16 = torch.full((bh, n, d), SENTINEL, dtype=torch.uint8).repeat(1, 1, 2).view(dt).reshape(bh, n, d)
    vt = sent16.clone()
    r = vrows(call)
    if r:
        # fp8_roundtrip_kernel over the leading rows only (launch_fp8_t: nbl blocks; rows >= N are zeros, rows in [vrows, N) are
        # never loaded because vrows is N or a multiple of 64)
        vt[:, :r] = roundtrip(call["v"][:, :r], False, pow2=v_pow2(call))["out"]
    if v_pow2(call):
        qv = quantise_v(call["v"])
        v8 = torch.zeros((bh, ntile * 128, d), dtype=torch.uint8)
        v8[:, :n] = qv["codes"]
        svexp = qv["svexp"]
    else:
        v8 = torch.full((bh, ntile * 128, d), SENTINEL, dtype=torch.uint8)
        svexp = torch.full((bh, nb), 0x7F7F7F7F, dtype=torch.int32)
    return dict(q8=qq["codes"], k8=qk["codes"], sq=qq["scale"], sk=qk["scale"], svexp=svexp, v8=v8, vt=vt, quant=(qq, qk))


# ---- attention over the workspace

def _operands(ws, call):
    """fp64 Q^, K^ (rotated basis, dequantised), V~ of the slab and of v8t (None where the call does not fill them)"""
    n = call["n"]
    qd, kd = dequant(ws["q8"], ws["sq"]), dequant(ws["k8"], ws["sk"])
    r16 = rows16(call)
    v16 = ws["vt"][:, :vrows(call)].double() if r16 else None
    v8 = e4m3_value(ws["v8"][:, :n]).double() * per_row(svexp_scale(ws["svexp"]), n) if r16 < n else None
    return qd, kd, v16, v8


def _masked(s, causal):
    if causal:
        nq, nk = s.shape[-2:]
        s = s.masked_fill(torch.arange(nk)[None, :] > torch.arange(nq)[:, None], NEG_INF)
    return s


def _fp64_attention(qd, kd, v16, v8, call, s=None, lse_keys=None):
    """o, lse in fp64; rows [0, rows16) over v16, the rest over v8"""
    n, r16 = call["n"], rows16(call)
    if s is None:
        s = _masked(qd @ kd.transpose(1, 2) * call["scale"], call["causal"])
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.empty((qd.shape[0], n, call["d"]), dtype=torch.float64)
    if r16:
        o[:, :r16] = p[:, :r16, :v16.shape[1]] @ v16       # (under the mask the first 256 rows see the first 256 keys only)
    if r16 < n:
        o[:, r16:] = p[:, r16:] @ v8
    return o, lse


def reference(ws, call):
    """Result (o, lse fp64) of attention of the dequantised tensors as the workspace holds them: (q8 sq)(k8 sk)^T scale, the
    softmax, V~ — the decoded v8t 2^e for the rows the all-e4m3 kernel serves, the 16-bit slab for the rows fwd_fp8_kernel
    serves (rows16).  No rotation appears: both operands are in the rotated basis and S is what it is."""
    o, lse = _fp64_attention(*_operands(ws, call), call)
    return _result(o, lse)


def _result(o, lse):
    return Result(o, lse, None, None, None, None, None, None, None, None, None)


def _mfma(a, b, terms, ct, init):
    """init + a @ b, the contraction cut into the matrix instructions' runs of `terms`; an instruction adds the exact sum of its
    products to the accumulator and rounds once to ct (mfma32's 16 terms; the e4m3 instruction without its truncation)"""
    acc = init
    for k0 in range(0, a.shape[-1], terms):
        acc = (acc.double() + _mm(a[..., k0:k0 + terms].double(), b[..., k0:k0 + terms, :].double())).to(ct)
    return acc


def _e4m3_exponent(v):
    """floor(log2 |v|) of e4m3 values with the subnormals at -6; -1000 for zero"""
    a = v.abs().double()
    return torch.where(a > 0, torch.floor(torch.log2(a.clamp_min(2.0 ** -9))).clamp_min(-6.0), torch.full_like(a, -1000.0))


MFMA_F8_GROUP, MFMA_F8_BITS = 8, 13
# the k indices of a 64-key P.V instruction in key order: fwd_fp8v_kernel hands the e4m3 P over as it holds the S^T accumulators, so
# k = 32 h + 16 kk + 4 j + byte is key 32 kk + 4 h + byte + 8 j of the 64-key block (the permutation fp8_quant_v_kernel gives V^T)
_PV_KEY_OF_K = torch.tensor([32 * kk + 4 * h + b + 8 * j for h in range(2) for kk in range(2) for j in range(4) for b in range(4)])


def _mfma_f8(a, b, ct, init, truncate, scale=None, order=None):
    """init + a @ b for e4m3 values a (.., K), b (.., K, n) as v_mfma_scale_f32_32x32x64_f8f6f4 adds them, 64 terms an instruction
    (fa_fwd_fp8.hip, fwd_fp8_kernel / fwd_fp8v_kernel: __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4).  The instruction's sum is
    NOT exact (measured on the MI355X, profiles/fp8_sweep.md: under the mask row 0 sees one key, so lse / (ln 2 f) is its raw
    score): the 64 products are taken in groups of 8 consecutive k; within a group every product is aligned to the largest
    exponent sum E of its two operands and truncated toward zero at 2^(E - 13); the eight group sums and the accumulator are then
    added and rounded once to float32.  That model reproduces every recovered score to the 0.01 the recovery resolves (values near
    1e5; the exact sums lie up to 2.8 away).  scale: (.., K / 64) a power of two per instruction applied to its sum (exact: the
    E8M0 operand); order: the k index -> contraction index map of one instruction (P.V).  truncate=False: the exact sum."""
    acc = init
    pad = (-a.shape[-1]) % 64                                                         # (the kernels read zeros there)
    if pad:
        a, b = torch.nn.functional.pad(a, (0, pad)), torch.nn.functional.pad(b, (0, 0, 0, pad))
    K = a.shape[-1]
    for k0 in range(0, K, 64):
        idx = k0 + (torch.arange(64) if order is None else order)
        tot = torch.zeros(init.shape, dtype=torch.float64)
        for g0 in range(0, idx.numel(), MFMA_F8_GROUP):
            gi = idx[g0:g0 + MFMA_F8_GROUP]
            pa, pb = a[..., gi].double(), b[..., gi, :].double()                       # (.., r, 8), (.., 8, n)
            prod = pa.unsqueeze(-1) * pb.unsqueeze(-3)                                # (.., r, 8, n)
            if truncate:
                es = _e4m3_exponent(pa).unsqueeze(-1) + _e4m3_exponent(pb).unsqueeze(-3)
                gran = torch.exp2(es.max(dim=-2, keepdim=True).values.clamp_min(-100.0) - MFMA_F8_BITS)
                prod = torch.trunc(prod / gran) * gran
            tot += prod.sum(-2)
        if scale is not None:
            tot = tot * scale[..., k0 // 64].double().reshape(scale.shape[:-1] + (1, 1))
        acc = (acc.double() + tot).to(ct)
    return acc


def baseline(ws, call, compute=torch.float32, rounding=True, trace=None):
    """Result (o, lse in `compute`) of the closed form with the two kernels' rounding points (module docstring).  rounding=False:
    no rounding of P and o (with compute = float64: the reference again).  trace: a list that receives, per kernel and tile,
    (kernel, tile, first row, moved (bh, rows) bool: the row's wave rescaled, stale (bh, rows) bool: the row's own max grew but its
    wave did not move)."""
    ct, n, d, bh = compute, call["n"], call["d"], call["bh"]
    f32 = ct == torch.float32
    rnd = round_to(call["dtype"] if rounding else None)
    p8 = (lambda p: e4m3_value(e4m3_code(p)).to(ct)) if rounding else (lambda p: p)
    r16 = rows16(call)
    q8, k8 = e4m3_value(ws["q8"]).to(ct), e4m3_value(ws["k8"]).to(ct)
    sq, sk = ws["sq"].to(ct), ws["sk"].to(ct)
    c_log2 = (torch.tensor(call["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32)).to(ct) if f32 \
        else torch.tensor(call["scale"] * LOG2E_F, dtype=ct)
    ln2 = torch.tensor(LN2_F, dtype=torch.float32).to(ct) if f32 else torch.tensor(LN2_F, dtype=ct)
    zero, ninf = torch.zeros((), dtype=ct), torch.tensor(NEG_INF, dtype=ct)
    o = torch.zeros((bh, n, d), dtype=ct)
    lse = torch.zeros((bh, n), dtype=ct)
    key_i = torch.arange(n)

    def run(kernel, r0, r1, vmat, vexp):
        tile = 64 if kernel == "fwd_fp8_kernel" else 128
        rows = torch.arange(r0, r1)
        nr = r1 - r0
        # raw scores: two 64-term instructions over the 128 head-dim bytes
        sacc = _mfma_f8(q8[:, r0:r1], k8.transpose(1, 2), ct, torch.zeros((bh, nr, n), dtype=ct), rounding)
        vis = (key_i[None, :] <= rows[:, None]) if call["causal"] else torch.ones((nr, n), dtype=torch.bool)
        sacc = torch.where(vis, sacc, ninf)
        fq = per_row(sq, n)[:, r0:r1] * c_log2                                     # (bh, nr, 1): the row's 64-row block = its wave's
        fk = fq * per_row(sk, n).transpose(1, 2)                                   # (bh, nr, n): f per key block
        kend = min(n, (r1 + ROW_TILE - 1) // ROW_TILE * ROW_TILE) if call["causal"] else n
        m = torch.full((bh, nr), NEG_INF, dtype=ct)
        l_ = torch.zeros((bh, nr), dtype=ct)
        acc = torch.zeros((bh, nr, d), dtype=ct)
        for t0 in range(0, kend, tile):
            sl = slice(t0, min(t0 + tile, n))
            if kernel == "fwd_fp8_kernel":
                s = sacc[..., sl] * fk[..., sl]                                     # s = sacc * f rounded once
                mx = s.max(-1).values
            else:
                mx = torch.full((bh, nr), NEG_INF, dtype=ct)
                for h0 in range(t0, min(t0 + tile, n), 64):                         # mx0 * f0, mx1 * f1 over the raw maxima
                    hs = slice(h0, min(h0 + 64, n))
                    mx = torch.maximum(mx, sacc[..., hs].max(-1).values * fk[..., h0])
            m_new = torch.maximum(m, mx)
            grow = m_new - m > 8.0                                                  # (first visible key: inf > 8; none yet: nan > 8 is False)
            pad = (-nr) % 32                                                        # (r0 is a multiple of 256: waves are aligned)
            gw = torch.nn.functional.pad(grow, (0, pad)).reshape(bh, -1, 32).any(-1, keepdim=True).expand(bh, -1, 32).reshape(bh, -1)[:, :nr]
            if trace is not None:
                trace.append((kernel, t0 // tile, r0, gw.clone(), (m_new > m) & ~gw))
            m_use = torch.where(gw, torch.where(m_new > NEG_INF, m_new, zero), m)
            alpha = torch.where(gw, torch.exp2(m - m_use), torch.ones((), dtype=ct))
            m = torch.where(gw, m_new, m)
            l_ = l_ * alpha
            acc = acc * alpha.unsqueeze(-1)
            if kernel == "fwd_fp8_kernel":
                p = torch.exp2(s - m_use.unsqueeze(-1))
                acc = _mfma(rnd(p), vmat[:, sl], 16, ct, acc)
            else:
                p = torch.exp2(_fma(sacc[..., sl], fk[..., sl], -m_use.unsqueeze(-1), ct))
                p = torch.where(vis[..., sl], p, zero)                              # (-inf * f + .. = -inf: exp2 gives 0)
                acc = _mfma_f8(p8(p), vmat[:, sl], ct, acc, rounding, scale=vexp[:, t0 // 64:(sl.stop + 63) // 64], order=_PV_KEY_OF_K)
            l_ = l_ + p.sum(-1)
        o[:, r0:r1] = rnd(acc * (1.0 / l_).unsqueeze(-1))
        lse[:, r0:r1] = (m + torch.log2(l_)) * ln2

    if r16:
        v16 = ws["vt"][:, :vrows(call)].to(ct)
        for r0 in range(0, r16, ROW_TILE):
            run("fwd_fp8_kernel", r0, min(r0 + ROW_TILE, r16), v16, None)
    if r16 < n:
        v8 = e4m3_value(ws["v8"][:, :n]).to(ct)                                    # the codes; 2^e goes to the instruction
        for r0 in range(r16, n, ROW_TILE):
            run("fwd_fp8v_kernel", r0, min(r0 + ROW_TILE, n), v8, svexp_scale(ws["svexp"]))
    return _result(o, lse)


def rounded(res, dtype):
    """a Result as the kernel returns it: o in dtype, lse float32"""
    return res._replace(o=res.o.to(dtype), lse=res.lse.float())


def tiles(n):
    """the query tiles [0, 256), [256, 512), .. the sharp bar is applied on"""
    return [(a, min(a + ROW_TILE, n)) for a in range(0, n, ROW_TILE)]


def tiled_sharp_bar(got, ref, base, dtype):
    """ex_full_ref.sharp_bar — the same function, the same factor 2 — per tensor and per query tile, so that the rows of one kernel
    do not set the maximum for the other's: (failures, {tensor[a:b]: kernel error / baseline error})"""
    bad, ratio = [], {}
    cut = lambda r, a, b: _result(r.o[:, a:b], r.lse[:, a:b])   # noqa: E731
    for a, b in tiles(ref.o.shape[1]):
        fails, r = sharp_bar(cut(got, a, b), cut(ref, a, b), cut(base, a, b), dtype)
        bad += [f"[{a}:{b}] {f}" for f in fails]
        ratio.update({f"{k}[{a}:{b}]": v for k, v in r.items()})
    return bad, ratio


def old_bars(got, model_o, model_lse, call):
    """today's bars of tests/test_fp8_gpu.py against a model (o, lse): rtol = atol = 3e-2 on o where P.V is 16-bit, 8e-2 where the
    all-e4m3 kernel runs (its _fp8_model: one tolerance per call), 2e-2 on lse.  True: passes."""
    tol = 8e-2 if v_pow2(call) else 3e-2
    a, b = got.o.double(), model_o.double()
    return bool(((a - b).abs() <= tol + tol * b.abs()).all()) and bool(((got.lse.double() - model_lse.double()).abs() < 2e-2).all())


# ---- mutants: bugs built into the fp64 evaluation

def mutant(ws, call, name):
    """the fp64 Result with one bug built in, or None where the bug does not apply to the call (it changes nothing):
      o_times_1.2                  o x 1.2 on the rows of the all-e4m3 kernel
      o_plus_0.05, lse_plus_1.5e-2
      k_scale_of_previous_block    sk of block t read from block t - 1 (block 0 its own)
      q_scale_per_workgroup        sq of the workgroup's first 64-row block for all eight waves (256 rows)
      both_halves_scored_with_f0   fwd_fp8v_kernel: the second 64 keys of a 128-key tile scored with the first block's sk
      both_v_halves_with_e0        fwd_fp8v_kernel: the second 64 keys of a V tile given the first block's exponent
      v_exponent_off_by_one        the exponent of V block 1 one too large
      p_truncated                  fwd_fp8v_kernel: p = exp2(s - rowmax) truncated toward zero to e4m3 before P.V
      rowsum_from_rounded_p        fwd_fp8v_kernel: l (o's divisor and lse) from the e4m3-rounded p
      tail_keys_dropped            the last N % 64 keys never visited
      diagonal_block_visible       under the mask a row also sees the keys above it inside its 64 x 64 diagonal block, up to
                                   4 h = 4 further (the mask threshold off by 4 h)
      e4m3_rows_read_the_slab      rows 256.. attend over the 16-bit V~ slab, which holds the sentinel there"""
    assert name in MUTANTS
    n, r16, causal = call["n"], rows16(call), call["causal"]
    qd, kd, v16, v8 = _operands(ws, call)
    ref = reference(ws, call)
    e4 = r16 < n
    if name == "o_times_1.2":
        if not e4:
            return None
        o = ref.o.clone()
        o[:, r16:] *= 1.2
        return ref._replace(o=o)
    if name == "o_plus_0.05":
        return ref._replace(o=ref.o + 0.05)
    if name == "lse_plus_1.5e-2":
        return ref._replace(lse=ref.lse + 1.5e-2)
    nb = (n + 63) // 64
    blk = torch.arange(nb)
    if name == "k_scale_of_previous_block":
        if nb < 2:
            return None
        kd = dequant(ws["k8"], ws["sk"][:, (blk - 1).clamp_min(0)])
    elif name == "q_scale_per_workgroup":
        if nb < 2:
            return None
        qd = dequant(ws["q8"], ws["sq"][:, blk // 4 * 4])
    elif name == "both_halves_scored_with_f0":
        if not e4:
            return None
        sk = ws["sk"].clone()
        sk[:, 1::2] = ws["sk"][:, 0:2 * (nb // 2):2]
        k_alt = dequant(ws["k8"], sk)
        s = _masked(qd @ kd.transpose(1, 2) * call["scale"], causal)
        s[:, r16:] = _masked(qd @ k_alt.transpose(1, 2) * call["scale"], causal)[:, r16:]
        return _result(*_fp64_attention(qd, kd, v16, v8, call, s=s))
    elif name in ("both_v_halves_with_e0", "v_exponent_off_by_one"):
        if not e4:
            return None
        ex = ws["svexp"].clone()
        if name == "both_v_halves_with_e0":
            ex[:, 1::2] = ws["svexp"][:, 0:2 * (nb // 2):2]
        else:
            ex[:, 1] += 1
        v8 = e4m3_value(ws["v8"][:, :n]).double() * per_row(svexp_scale(ex), n)
    elif name in ("p_truncated", "rowsum_from_rounded_p"):
        if not e4:
            return None
        s = _masked(qd @ kd.transpose(1, 2) * call["scale"], causal)
        m = s.max(-1, keepdim=True).values
        p = torch.exp(s - m)
        pr = e4m3_value(e4m3_code(p.float())).double()
        if name == "p_truncated":
            codes = e4m3_code(p.float())
            down = e4m3_value(codes).double() > p
            pr = e4m3_value((codes.to(torch.int16) - down.to(torch.int16)).clamp_min(0).to(torch.uint8)).double()
            l_ = p.sum(-1)
        else:
            l_ = pr.sum(-1)
        o, lse = ref.o.clone(), ref.lse.clone()
        o[:, r16:] = (pr @ v8)[:, r16:] / l_[:, r16:, None]
        lse[:, r16:] = (m.squeeze(-1) + torch.log(l_))[:, r16:]
        return _result(o, lse)
    elif name == "tail_keys_dropped":
        if n % 64 == 0 or n < 64:
            return None
        s = _masked(qd @ kd.transpose(1, 2) * call["scale"], causal)
        s[..., n - n % 64:] = NEG_INF
        return _result(*_fp64_attention(qd, kd, v16, v8, call, s=s))
    elif name == "diagonal_block_visible":
        if not causal:
            return None
        i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
        vis = (j <= i) | ((j <= i + 4) & (j // 64 == i // 64))
        s = (qd @ kd.transpose(1, 2) * call["scale"]).masked_fill(~vis, NEG_INF)
        if r16 and vrows(call) < n:
            s[:, :r16, vrows(call):] = NEG_INF
        return _result(*_fp64_attention(qd, kd, v16, v8, call, s=s))
    elif name == "e4m3_rows_read_the_slab":
        if not (e4 and r16):
            return None
        o = ref.o.clone()
        o[:, r16:] = float("nan")                    # P x the sentinel (3.4e38 next to finite values of both signs)
        return ref._replace(o=o)
    return _result(*_fp64_attention(qd, kd, v16, v8, call))
