"""The table of the fp8-inputs sweep: tests/test_fp8_inputs_cpu.py proves the reference, baseline and mutants of
tests/fp8_inputs_ref.py on it, tests/test_fp8_inputs_gpu.py runs it on the kernels of csrc/fa_fp8_inputs.hip.  d = 128 and B = 2
everywhere (so that batch strides and the per-batch descales count).

heads (H_q, H_kv): (2, 2) ungrouped, (4, 2) groups of two, (3, 1) an odd group over one K/V head.
(Nq, Nk), each naming the edge it crosses:
    (1, 300)      one query row; a ragged third key tile
    (64, 64)      half a key tile
    (256, 256)    one whole query tile, whole key tiles
    (257, 257)    the query-tile edge: one row in the second tile, one key in the third key tile
    (130, 257)    a tail key; three 64-key groups of queries; the diagonal shifted by 127
    (300, 130)    170 dead rows under the mask (a whole wave of them, and waves that mix dead and live rows); nb = 3 is odd, so the
                  second half of the last V^T tile is the zeroed one
    (48, 16)      fewer keys than a 64-key group, fewer rows than two waves; 32 dead rows under the mask
    (384, 640)    five key tiles; the second query tile under a diagonal shifted by 256
    (520, 520)    three query tiles, the second and third under the diagonal; a ragged fifth key tile
mask: none, causal (bottom-right aligned).  out dtype: bf16, f16.
layout: "bhnd" contiguous (B, H, N, 128); "bnhd" views of (B, N, H, 128) tensors; "prefix": q as bnhd and K/V the [:, :Nk] prefix
of (B, Nk + 37, H_kv, 128) buffers whose other bytes are 0x7F (e4m3 NaN).
descales: None; "bh" (B, H_kv) random in [0.25, 4] with odd 24-bit mantissas; "h" (H_kv,).
values: "normal" unit normal x, codes = e4m3(clamp(x / descale, +-448)); "growing": the keys' norm rises 13-fold along the sequence so
that the running max climbs by more than 2^8 several times.

From §9l's greedy pairwise generator (tests/fp8_cases.generate) with a fixed seed, under a cap of 40 cases."""
import torch

from tests.fp8_cases import generate

B, D = 2, 128
SEED = 2718            # of the table
DATA_SEED = 7          # of the tensors (build_call)
PREFIX_EXTRA = 37      # tokens of a "prefix" cache past Nk
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
AXES = {
    "heads": ((2, 2), (4, 2), (3, 1)),
    "n": ((1, 300), (64, 64), (256, 256), (257, 257), (130, 257), (300, 130), (48, 16), (384, 640), (520, 520)),
    "mask": ("none", "causal"),
    "dtype": ("bf16", "f16"),
    "layout": ("bhnd", "bnhd", "prefix"),
    "descale": ("none", "bh", "h"),
    "input": ("normal", "growing"),
}
MAX_CASES = 40
CASES = generate(AXES, SEED)
assert len(CASES) <= MAX_CASES, len(CASES)


def case_id(c, i):
    return f"{i:02d}-" + "-".join("x".join(str(x) for x in v) if isinstance(v, tuple) else str(v) for v in c.values())


def odd_mantissa(x):
    """float32 x with the last mantissa bit set"""
    return (x.float().contiguous().view(torch.int32) | 1).view(torch.float32)


def quantise(x, descale_bh):
    """uint8 e4m3 codes of x (B, H, N, 128) under descales (B, H): clamp(x / descale, +-448), then torch's RNE conversion (which gives
    NaN, not saturation, above 448: hence the clamp)"""
    y = (x / descale_bh[:, :, None, None]).clamp(-448.0, 448.0)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def build_call(c, i):
    """the call of case c (index i of CASES) as CPU tensors; see tests/fp8_inputs_ref.py for the keys"""
    hq, hkv = c["heads"]
    nq, nk = c["n"]
    g = torch.Generator(device="cpu")
    g.manual_seed(DATA_SEED + 1000 * i)
    q = torch.randn((B, hq, nq, D), generator=g, dtype=torch.float32)
    k = torch.randn((B, hkv, nk, D), generator=g, dtype=torch.float32)
    v = torch.randn((B, hkv, nk, D), generator=g, dtype=torch.float32)
    if c["input"] == "growing":
        k = k * (1.0 + 12.0 * torch.arange(nk, dtype=torch.float32) / nk)[None, None, :, None]
    ds = {}
    for name in ("q_descale", "k_descale", "v_descale"):
        if c["descale"] == "none":
            ds[name] = None
        else:
            shape = (B, hkv) if c["descale"] == "bh" else (hkv,)
            ds[name] = odd_mantissa(0.25 * 16.0 ** torch.rand(shape, generator=g, dtype=torch.float32)).clamp(0.25, 4.0)
    full = lambda t: torch.ones((B, hkv)) if t is None else (t if t.dim() == 2 else t[None, :].expand(B, hkv))   # noqa: E731
    q8 = quantise(q, full(ds["q_descale"]).repeat_interleave(hq // hkv, dim=1))
    k8 = quantise(k, full(ds["k_descale"]))
    v8 = quantise(v, full(ds["v_descale"]))
    return dict(B=B, hq=hq, hkv=hkv, nq=nq, nk=nk, causal=c["mask"] == "causal", dtype=DTYPES[c["dtype"]], scale=D ** -0.5,
                layout=c["layout"], input=c["input"], q8=q8, k8=k8, v8=v8, **ds)
