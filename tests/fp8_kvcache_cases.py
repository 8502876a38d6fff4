"""The case table of fp8 KV-cache decoding (tests/test_fp8_kvcache_cpu.py, tests/test_fp8_kvcache_gpu.py) and its
builder.  Axes:
    dtype     of o: bf16, f16
    heads     (H_q, H_kv): (4, 4), (8, 2), (6, 1) partial 32-row tiles (G Nq = 1 .. 30 rows); (40, 1) more than one tile: 40, 80 and
              200 rows, whose first tiles are exactly full and whose last one is partial
    nq        1, 2, 5 query tokens
    lens      three sequences, lengths from {0, 1, 63, 64, 65, 127, 128, 129, 300}, always one dead sequence (length 0)
    mask      none, causal (bottom-right; with Nq > len rows have no key: lens holding 1 with Nq 2 or 5)
    layout    contiguous; contiguous + cache_batch_idx with one out-of-range index; paged with ps 16 / 48 / 256
    splits    1, 2, 5, 0 (the library's rule), 64 (more than there are 64-key tiles)
    descales  None, (H_kv,), (B, H_kv) — not powers of two
    values    normal: unit normals quantised by absmax; growing: keys growing along the sequence so that a wave rescales several times
              (asserted on the baseline's trace in the CPU test)
From §9l's greedy pairwise generator (tests/fp8_cases.generate) with a fixed seed, under a cap of 40 cases; no axis value dropped."""
import torch

from tests.fp8_cases import DTYPES, generate

SEED = 6174
DATA_SEED = 11
SENTINEL = 0x7F
D = 128
LENS = {"a": (0, 1, 300), "b": (63, 0, 129), "c": (64, 128, 0), "d": (65, 0, 127), "e": (300, 64, 0)}
AXES = {
    "dtype": ("bf16", "f16"),
    "heads": ((4, 4), (8, 2), (6, 1), (40, 1)),
    "nq": (1, 2, 5),
    "lens": tuple(LENS),
    "mask": ("none", "causal"),
    "layout": ("contig", "bidx", "ps16", "ps48", "ps256"),
    "splits": (1, 2, 5, 0, 64),
    "descales": ("none", "hkv", "bhkv"),
    "values": ("normal", "growing"),
}
MAX_CASES = 40
CASES = generate(AXES, SEED)
assert len(CASES) <= MAX_CASES, len(CASES)
assert all({c[a] for c in CASES} == set(v) for a, v in AXES.items()), "an axis value was dropped"


def case_id(c, i):
    return f"{i:02d}-" + "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c.values())


def e4m3(x):
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def quantise(x, hkv, form):
    """x (B, n, H, 128) float -> (uint8 codes, descale): form "none": the codes of x itself, no descale; "hkv": absmax / 448 per K/V
    head over the batch, a (H_kv,) descale; "bhkv": per (batch, K/V head), (B, H_kv).  The heads of x are H_kv groups of H / H_kv."""
    B, n, H, _ = x.shape
    if form == "none":
        return e4m3(x), None
    xg = x.reshape(B, n, hkv, H // hkv, D)
    amax = xg.abs().amax(dim=(1, 3, 4)) if form == "bhkv" else xg.abs().amax(dim=(0, 1, 3, 4))[None].expand(B, hkv)
    d = (amax.clamp_min(1e-3) / 448.0).float()
    d = (d.contiguous().view(torch.int32) | 1).view(torch.float32)          # an odd mantissa: never a power of two
    codes = e4m3((xg / d[:, None, :, None, None]).reshape(B, n, H, D))
    return codes, (d.contiguous() if form == "bhkv" else d[0].contiguous())


def build_call(c, i):
    """the call of case c (index i of the table) as CPU tensors: the dict tests/fp8_kvcache_ref.py takes.  Cache bytes no live token
    owns are 0x7F (e4m3 NaN); table entries past a sequence's last page are garbage; with cache_batch_idx one live sequence's index
    lies outside the cache."""
    g = torch.Generator().manual_seed(DATA_SEED + 977 * i)
    hq, hkv = c["heads"]
    nq, lens = c["nq"], LENS[c["lens"]]
    B, maxlen = len(lens), max(LENS[c["lens"]])
    q = torch.randn((B, nq, hq, D), generator=g)
    k = torch.randn((B, maxlen, hkv, D), generator=g)
    v = torch.randn((B, maxlen, hkv, D), generator=g)
    if c["values"] == "growing":
        k = k * (1.0 + 12.0 * torch.arange(maxlen, dtype=torch.float32) / maxlen)[None, :, None, None]
        q = q * 3.0
    for b, n in enumerate(lens):
        k[b, n:], v[b, n:] = 0.0, 0.0
    q8, qd = quantise(q, hkv, c["descales"])
    k8, kd = quantise(k, hkv, c["descales"])
    v8, vd = quantise(v, hkv, c["descales"])
    layout = c["layout"]
    table, bidx = None, None
    if layout.startswith("ps"):
        ps = int(layout[2:])
        need = [(n + ps - 1) // ps for n in lens]
        max_blocks, num_blocks = max(need) + 2, sum(need) + 3
        perm = torch.randperm(num_blocks, generator=g).tolist()
        table = torch.randint(-5, num_blocks + 5, (B, max_blocks), generator=g, dtype=torch.int32)
        kc = torch.full((num_blocks, ps, hkv, D), SENTINEL, dtype=torch.uint8)
        vc = torch.full((num_blocks, ps, hkv, D), SENTINEL, dtype=torch.uint8)
        for b, n in enumerate(lens):
            for j in range(need[b]):
                pg = perm.pop()
                table[b, j] = pg
                m = min(ps, n - j * ps)
                kc[pg, :m], vc[pg, :m] = k8[b, j * ps:j * ps + m], v8[b, j * ps:j * ps + m]
    else:
        cap = maxlen + 9
        rows = B + 2 if layout == "bidx" else B
        kc = torch.full((rows, cap, hkv, D), SENTINEL, dtype=torch.uint8)
        vc = torch.full((rows, cap, hkv, D), SENTINEL, dtype=torch.uint8)
        where = list(range(B))
        if layout == "bidx":
            where = [3, 0, 4]
        for b, n in enumerate(lens):
            kc[where[b], :n], vc[where[b], :n] = k8[b, :n], v8[b, :n]
        if layout == "bidx":
            lens = list(lens)
            dead = max(range(B), key=lambda b: lens[b] if lens[b] < maxlen else -1)    # one live sequence loses its row: out of range
            where[dead] = rows + 2
            bidx = torch.tensor(where, dtype=torch.int32)
    return dict(B=B, hq=hq, hkv=hkv, nq=nq, causal=c["mask"] == "causal", dtype=DTYPES[c["dtype"]], scale=D ** -0.5,
                num_splits=c["splits"], q8=q8, k_cache=kc, v_cache=vc, cache_seqlens=torch.tensor(lens, dtype=torch.int32),
                block_table=table, cache_batch_idx=bidx, q_descale=qd, k_descale=kd, v_descale=vd, values=c["values"])
