"""The all-pairs case table of the extended forward / backward sweep (tests/test_ex_sweep_gpu.py runs it, tests/test_ex_sweep_cpu.py
checks it) and the inputs of a case, as CPU tensors in the arguments of ex_forward / ex_backward (padded) or ex_varlen_forward /
ex_varlen_backward (packed).

AXES lists the options a call of the extended path combines.  CASES comes from the greedy covering-array generator of
tests/kvcache_sweep_cases.py (the same thirty lines, over this module's axes) with a fixed seed: every pair of values of two
different axes that the C layer accepts together (pair_legal) is in at least one case, every case is legal, and there are at most
MAX_CASES of them.  A new feature of the extended path adds its axis here.

Sizes: B = 2 for the padded calls, four sequences for the packed ones (an empty one and a one-token one in every tuple, one length
above 128 that is no multiple of 32; with separate q / k lengths also a sequence with len_q > len_k and one without keys).  A packed
tensor has one token in front of the first sequence and one behind the last that no sequence owns."""
import itertools
import random

import torch

from oracle import attention_oracle as orc
from tests.sink_ref import window_visible

B = 2                # padded calls
SEQS = 4             # packed calls
MAX_CASES = 120
SEED = 31337
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PATHS = {"auto": 0, "exact": 1, "mfma_only": 3}
NEG_INF = float("-inf")

# (Nq, Nk) of the padded calls; the packed layouts read the same axis value as an index into PACKED / PACKED_QK
LENGTHS = ((160, 160), (256, 256), (300, 300), (1, 200), (48, 16), (130, 257))
PACKED = ((160, 0, 1, 137), (256, 1, 0, 130), (300, 0, 1, 64), (1, 200, 0, 33), (48, 0, 1, 145), (130, 257, 1, 0))
PACKED_QK = (((160, 0, 1, 137), (100, 40, 0, 200)), ((256, 1, 0, 130), (256, 0, 33, 70)), ((300, 0, 1, 64), (257, 5, 0, 300)),
             ((1, 200, 0, 33), (200, 130, 16, 0)), ((48, 0, 1, 145), (16, 7, 0, 145)), ((130, 257, 1, 0), (257, 130, 0, 9)))

AXES = {
    "dtype": ("bf16", "f16", "f32"),
    "path": ("auto", "exact", "mfma_only"),
    "layout": ("padded", "packed", "packed_qk", "packed_strided"),
    "widths": ((8, 8), (24, 24), (40, 40), (64, 64), (72, 72), (96, 96), (128, 128), (136, 136), (200, 200), (256, 256), (20, 20),
               (192, 128), (72, 40), (64, 32)),                                                        # (d, d_v)
    "heads": ((4, 4), (4, 2), (4, 1), (6, 2), (3, 1)),                                                 # (H_q, H_kv)
    "lengths": LENGTHS,
    "mask": ("none", "causal", "causal+window20", "window30_10", "causal+window0"),
    "dense": ("none", "mask", "mask_bh", "block32", "block64"),
    "dropout": (0.0, 0.1),
    "mods": ("none", "softcap", "alibi", "alibi_b+softcap"),
    "sinks": (False, True),
    "dlse": (False, True),
    "scale": ("default", 0.37),
}
NAMES = tuple(AXES)


def window_of(mask):
    return {"causal+window20": (20, -1), "window30_10": (30, 10), "causal+window0": (0, -1)}.get(mask, (-1, -1))


def pair_legal(a, va, b, vb):
    """may axis a = va go with axis b = vb in one call?  Each rule names the line of the C layer (flashattention-pytorch_amd/csrc)
    or of the Python layer (flashattention_lab_cuda/__init__.py) that it transcribes."""
    p = {a: va, b: vb}
    two = "widths" in p and p["widths"][0] != p["widths"][1]
    if p.get("path") == "mfma_only":
        # launch_ex_one / launch_ex_varlen_one (fa_ex.hip: `if (path >= 2) return hipErrorInvalidConfiguration`) after
        # ex_mfma_supported (fa_ex_mfma.hip): dtype 1 or 2, 8 <= d <= 128, d % 8 == 0, br and bc multiples of 32 (32 and 64 are).
        # A two-width call never gets there: launch_ex sends it to launch_ex_vdim first, whatever the option says.
        if p.get("dtype") == "f32":
            return False
        if "widths" in p and not two and (p["widths"][0] > 128 or p["widths"][0] % 8):
            return False
    if two:
        # vdim_check (fa_capi.hip) and vdim_arg (__init__.py): f16 / bf16 only, and by name none of mask, block_sparse_mask,
        # dropout_p > 0, window_size (either bound other than -1), softcap, alibi_slopes, sinks
        if p.get("dtype") == "f32" or p.get("dense", "none") != "none" or p.get("dropout", 0.0) > 0.0 or p.get("mods", "none") != "none":
            return False
        if p.get("sinks", False) or window_of(p.get("mask", "none")) != (-1, -1):
            return False
    if p.get("layout", "padded") != "padded" and p.get("dense", "none") != "none":
        return False    # ex_varlen_forward / fa_ex_forward_varlen have no mask arguments (include/fa_mi355x.h: "No dense or block-sparse mask")
    return True


def case_legal(c):
    return all(pair_legal(a, c[a], b, c[b]) for a, b in itertools.combinations(NAMES, 2))


def all_pairs():
    """every legal ((axis, value), (axis, value)) with the axes in NAMES order"""
    out = set()
    for a, b in itertools.combinations(NAMES, 2):
        for va, vb in itertools.product(AXES[a], AXES[b]):
            if pair_legal(a, va, b, vb):
                out.add(((a, va), (b, vb)))
    return out


def pairs_of(c):
    return {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(NAMES, 2)}


def generate(seed=SEED, tries=40):
    """Greedy (tests/kvcache_sweep_cases.generate): each new case is the best of `tries` candidates; a candidate starts from an
    uncovered pair and takes, axis by axis in a shuffled order, the legal value that covers the most uncovered pairs with the
    values already chosen."""
    rng = random.Random(seed)
    uncovered = all_pairs()
    cases = []
    while uncovered:
        best, best_gain = None, -1
        for _ in range(tries):
            (a, va), (b, vb) = rng.choice(sorted(uncovered, key=repr))
            c = {a: va, b: vb}
            rest = [n for n in NAMES if n not in c]
            rng.shuffle(rest)
            for n in rest:
                scored = []
                for v in AXES[n]:
                    if not all(pair_legal(n, v, m, c[m]) for m in c):
                        continue
                    gain = sum(1 for m in c if (((n, v), (m, c[m])) if NAMES.index(n) < NAMES.index(m) else ((m, c[m]), (n, v))) in uncovered)
                    scored.append((gain, rng.random(), v))
                c[n] = max(scored, key=lambda t: t[:2])[2]
            gain = len(pairs_of(c) & uncovered)
            if gain > best_gain:
                best, best_gain = c, gain
        cases.append({n: best[n] for n in NAMES})
        uncovered -= pairs_of(best)
    return cases


CASES = generate()


def case_id(i):
    c = CASES[i]
    return f"{i:03d}-" + "-".join(str(c[n]).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") for n in NAMES)


def lengths_of(c):
    """(lens_q, lens_k) of a packed case, ((Nq,), (Nk,)) of a padded one"""
    n = LENGTHS.index(c["lengths"])
    if c["layout"] == "padded":
        return (c["lengths"][0],), (c["lengths"][1],)
    if c["layout"] == "packed_qk":
        return PACKED_QK[n]
    return PACKED[n], PACKED[n]


def cu_of(lens):
    """offsets of a packed tensor whose token 0 and last token belong to no sequence"""
    out = [1]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _visible_rows(nq, nk, causal, window, mask, block_mask, br, bc):
    vis = orc.extended_visible(1 if mask is None or mask.dim() == 2 else mask.shape[0], nq, nk, False, mask, block_mask, br, bc)
    return (vis & window_visible(nq, nk, causal, window).unsqueeze(0)).any(-1)


def build_inputs(i, case=None):
    """The call of case i, seeded by i, as a dict of CPU tensors and values:
        layout, dtype, path (the ex_path option), heads (H_q, H_kv), q, k, v, do, causal, scale, window, softcap, alibi_slopes, sinks,
        dlse (finite everywhere; the tests write NaN where the reference's lse is -inf), dropout_p, seed,
        padded:  q, do (B H_q, Nq, .), k, v (B H_kv, Nk, .); mask, block_mask, br, bc
        packed:  q, do (total_q, H_q, .), k, v (total_k, H_kv, .), cu_seqlens_q, cu_seqlens_k (int32), max_seqlen_q, max_seqlen_k;
                 packed_strided: q, k (and v when it is as wide) are views of "qkv", one (total, 3, H_q, d) buffer."""
    c = CASES[i] if case is None else case
    g = torch.Generator().manual_seed(SEED + i)
    dtype, (d, dv), (hq, hkv) = DTYPES[c["dtype"]], c["widths"], c["heads"]
    rn = lambda *shape: torch.randn(shape, generator=g).to(dtype)   # noqa: E731
    # k, v, do are unit normal; q too under the default scale.  Under scale = 0.37 q has the deviation d^-0.5 / 0.37, so that the
    # logits keep unit variance: that is the regime the project's 5e-2 bar is set for.  With unit-normal q the logits would have a
    # deviation of 0.37 sqrt(d), up to 5.9; the softmax is then near one-hot and the 16-bit rounding of the stored o alone moves dq
    # and dk by more than 5e-2 through delta (the baseline of tests/ex_full_ref.py, which has no kernel in it, misses the bar by
    # 0.07 to 0.17 at d >= 192).  A kernel that took d^-0.5 for the scale passed is off by the same factor either way.
    qstd = 1.0 if c["scale"] == "default" else d ** -0.5 / float(c["scale"])
    rq = lambda *shape: (torch.randn(shape, generator=g) * qstd).to(dtype)   # noqa: E731
    lens_q, lens_k = lengths_of(c)
    causal = c["mask"] in ("causal", "causal+window20", "causal+window0")
    kw = dict(layout=c["layout"], dtype=dtype, path=PATHS[c["path"]], heads=(hq, hkv), causal=causal, window=window_of(c["mask"]),
              scale=d ** -0.5 if c["scale"] == "default" else float(c["scale"]), softcap=0.0, alibi_slopes=None, sinks=None, dlse=None,
              dropout_p=float(c["dropout"]), seed=1000 + i, mask=None, block_mask=None, br=128, bc=128, cu_seqlens_q=None,
              cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None)
    if c["layout"] == "padded":
        nq, nk = lens_q[0], lens_k[0]
        kw.update(q=rq(B * hq, nq, d), k=rn(B * hkv, nk, d), v=rn(B * hkv, nk, dv), do=rn(B * hq, nq, dv))
        nb, lse_shape = B, (B * hq, nq)
        for attempt in range(50):      # a mask under which no row sees a key checks nothing: draw again (never needed more than twice)
            gm = torch.Generator().manual_seed(SEED + 7919 * (i + 1) + attempt)
            mask = bmask = None
            br = bc = 128
            if c["dense"] == "mask":
                mask = (torch.rand((nq, nk), generator=gm) > 0.3).to(torch.uint8)
            elif c["dense"] == "mask_bh":
                mask = (torch.rand((B * hq, nq, nk), generator=gm) > 0.3).to(torch.uint8)
                mask[0, :5] = 0                                    # rows of unit 0 without a visible key
            elif c["dense"] in ("block32", "block64"):
                br = bc = int(c["dense"][5:])
                bmask = (torch.rand(((nq + br - 1) // br, (nk + bc - 1) // bc), generator=gm) > 0.35).to(torch.uint8)
                if br == 64:
                    bmask[0, 0] = 1
            if bool(_visible_rows(nq, nk, causal, kw["window"], mask, bmask, br, bc).any()):
                break
        kw.update(mask=mask, block_mask=bmask, br=br, bc=bc)
    else:
        cu_q, cu_k = cu_of(lens_q), cu_of(lens_k)
        tq, tk = cu_q[-1] + 1, cu_k[-1] + 1
        if c["layout"] == "packed_strided":
            qkv = rn(tq, 3, hq, d)
            qkv[:, 0] = (qkv[:, 0].float() * qstd).to(dtype)
            kw.update(qkv=qkv, q=qkv[:, 0], k=qkv[:, 1, :hkv], v=qkv[:, 2, :hkv] if dv == d else rn(tk, hkv, dv))
        else:
            kw.update(q=rq(tq, hq, d), k=rn(tk, hkv, d), v=rn(tk, hkv, dv))
        kw.update(do=rn(tq, hq, dv), cu_seqlens_q=torch.tensor(cu_q, dtype=torch.int32), cu_seqlens_k=torch.tensor(cu_k, dtype=torch.int32),
                  max_seqlen_q=max(lens_q), max_seqlen_k=max(lens_k))
        nb, lse_shape = SEQS, (hq, tq)
    if "softcap" in c["mods"]:
        kw["softcap"] = 30.0
    if "alibi" in c["mods"]:
        sl = torch.tensor([2.0 ** (-8.0 * (h + 1) / hq) for h in range(hq)], dtype=torch.float32)
        if c["mods"] == "alibi":      # (H_q,): the 3-D padded call takes it as the (B, H_q) view of the vector, row stride 0
            kw["alibi_slopes"] = sl.view(1, hq).expand(nb, hq) if c["layout"] == "padded" else sl
        else:
            kw["alibi_slopes"] = (sl.view(1, hq) * torch.arange(1, nb + 1).view(nb, 1).float()).contiguous()
    if c["sinks"]:
        sk = torch.randn((hq,), generator=g)
        sk[1 % hq], sk[3 % hq] = NEG_INF, 9.0                # one sink that adds nothing, one that outweighs the keys
        kw["sinks"] = sk
    if c["dlse"]:
        kw["dlse"] = torch.randn(lse_shape, generator=g)
    return kw
