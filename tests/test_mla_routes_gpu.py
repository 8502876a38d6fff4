"""GPU: every instantiation of the MLA decode kernels (csrc/fa_mla.hip) named as a route and run once on one small problem.

  form                    entry point                                        kernel
  dense, 16-bit caches    flash_attn_with_kvcache(qv=)                       mla_split_kernel<dtype, waves, paged>
  lists, 16-bit caches    flash_mla_sparse_attn                              mla_sparse_kernel<dtype, waves, paged>
  dense, packed pool      flash_mla_with_kvcache(is_fp8_kvcache=True)        mla_f8_kernel<waves, false>
  lists, packed pool      flash_mla_with_kvcache(.., indices=)               mla_f8_kernel<waves, true>

H_q = 16, 17, 33 with one K/V head and one query token are the smallest row counts that take one, two and four waves a workgroup
(mla_waves); at 33 the four-wave workgroup has a wave with a single row and a wave that only copies.  Two sequences of lengths 100
(four 32-key tiles, the last partial) and 0 (dead); lists of 40 entries (two tiles, the second partial) with one entry that is
the length itself.  num_splits 1 and 3 (dense), 1 and 2 (lists): the direct store, and the partials with the combine.  A case runs
its form on the contiguous and on the paged cache (page size 16; the packed forms are paged only), so bf16 with both split counts
and float16 with one per wave count reach all 30 instantiations.

One pool serves every case: a packed pool, the bf16 pool its read contract gives (tests/mla_fp8_ref.unpack_pool), that pool
rounded to float16, and per sequence the same tokens gathered into a contiguous cache.  Per case: within
tests/test_kvcache_gpu.py::check of the fp64 reference (tests/mla_ref.py, tests/mla_sparse_ref.py) on those values; the paged call
has the bits of the contiguous call; the packed call has the bits of the 16-bit paged call; a repeated call has the same bits;
the dead sequence gives o = 0, lse = -inf.  A reference is computed once per (form, dtype, H_q) and shared.

Every case is also held to the sharp bar (sharp_out): tests/ex_full_ref.sharp_bar's inequality against the rounding model of
mla_decode (tests/decode_baseline.mla_dense_baseline / mla_list_baseline at the case's split count), per call and per sequence.
tests/test_decode_sharp_cpu.py proves that this bar rejects the bugs `check` lets through; profiles/decode_sweep.md has the ratios."""
import functools

import pytest
import torch

from tests import decode_baseline as db
from tests import mla_fp8_ref as ref
from tests.kvcache_paged_ref import paged_tokens
from tests.mla_ref import mla_reference
from tests.mla_sparse_ref import mla_sparse_reference
from tests.test_kvcache_gpu import check
from tests.test_mla_fp8_gpu import SCALE, fm, qv_call, sparse_call, values

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
LENS = (100, 0)
PS, NBLK, MB = 16, 9, 7          # capacity 112
TOPK = 40
WAVES = {16: 1, 17: 2, 33: 4}    # H_q -> waves a workgroup (csrc/fa_mla.hip: mla_waves)

# (form, dtype, H_q, num_splits)
CASES = [(form, BF16, hq, s) for form, splits in (("dense", (1, 3)), ("lists", (1, 2))) for hq in WAVES for s in splits]
CASES += [(form, F16, hq, s) for form, splits in (("dense", (3, 1, 3)), ("lists", (2, 1, 2))) for hq, s in zip(WAVES, splits)]
PACKED = [(form, hq, s) for form, splits in (("dense", (1, 3)), ("lists", (1, 2))) for hq in WAVES for s in splits]


def routes(form, dtype, hq, packed=False):
    """the kernel instantiations a case launches"""
    if packed:
        return [f"mla_f8_kernel<{WAVES[hq]}, {'true' if form == 'lists' else 'false'}>"]
    name, tag = ("mla_split_kernel" if form == "dense" else "mla_sparse_kernel"), ("bf16_tag" if dtype == BF16 else "f16_tag")
    return [f"{name}<{tag}, {WAVES[hq]}, {paged}>" for paged in ("false", "true")]


def test_the_cases_name_every_instantiation():
    named = {r for c in CASES for r in routes(*c[:3])} | {r for form, hq, _s in PACKED for r in routes(form, BF16, hq, True)}
    assert len(named) == 2 * 2 * 3 * 2 + 3 * 2


@functools.lru_cache(maxsize=None)
def pools():
    """CPU: the packed pool (9 pages of 16 tokens), its bf16 pool (.., 576) = [latent | rotary], and a (2, 7) table whose rows share
    pages"""
    rows = ref.pack_rows(values((NBLK, PS, 1, 512), 1), values((NBLK, PS, 1, 64), 2))
    g = torch.Generator().manual_seed(3)
    table = torch.stack([torch.randperm(NBLK, generator=g)[:MB] for _ in LENS]).to(torch.int32)
    return rows, ref.unpack_pool(rows), table


@functools.lru_cache(maxsize=None)
def caches(dtype):
    """CPU: the 16-bit pool in dtype and the contiguous cache (2, 112, 1, 576) of the same tokens"""
    _rows, pool16, table = pools()
    pool = pool16.to(dtype)
    return pool, torch.stack([paged_tokens(pool, table[b], MB * PS, PS) for b in range(len(LENS))])


@functools.lru_cache(maxsize=None)
def queries(dtype, hq):
    g = torch.Generator().manual_seed(hq)
    return torch.randn((len(LENS), 1, hq, 576), generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def lists():
    """(2, 1, 40) int32: tokens of the sequence at random list positions (some twice), -1 padding, and one entry that is the length
    itself; the dead sequence's list holds positions of the cache, none visible"""
    g = torch.Generator().manual_seed(4)
    ix = torch.full((len(LENS), 1, TOPK), -1, dtype=torch.int64)
    for b, ln in enumerate(LENS):
        if ln == 0:
            ix[b, 0] = torch.randint(0, MB * PS, (TOPK,), generator=g)
            continue
        pos = torch.randperm(TOPK, generator=g)
        ix[b, 0, pos[:30]] = torch.randint(0, ln, (30,), generator=g)
        ix[b, 0, 33], ix[b, 0, 35] = ln, ln - 1          # in the partial tile: no key, and the last token
    return ix.to(torch.int32)


@functools.lru_cache(maxsize=None)
def expected(form, dtype, hq):
    """the fp64 reference on the 16-bit values (for the packed forms: the dequantised ones)"""
    pool, _cont = caches(dtype)
    q, table, sl = queries(dtype, hq), pools()[2], torch.tensor(LENS, dtype=torch.int32)
    if form == "dense":
        return mla_reference(q[..., 512:], q[..., :512], pool[..., 512:], pool[..., :512], sl, False, (-1, -1), SCALE, table)
    return mla_sparse_reference(q[..., 512:], q[..., :512], pool[..., 512:], pool[..., :512], lists(), sl, False, SCALE, table)


@functools.lru_cache(maxsize=None)
def baseline(form, dtype, hq, splits):
    """the rounding model of the case's kernel on the values expected() reads, at the case's split count"""
    pool, _cont = caches(dtype)
    q, table, sl = queries(dtype, hq), pools()[2], torch.tensor(LENS, dtype=torch.int32)
    if form == "dense":
        return db.mla_dense_baseline(q[..., 512:], q[..., :512], pool[..., 512:], pool[..., :512], sl, False, (-1, -1), SCALE, table, splits=splits)
    return db.mla_list_baseline(q[..., 512:], q[..., :512], pool[..., 512:], pool[..., :512], lists(), sl, False, SCALE, table, splits=splits)


def sharp_out(o, lse, form, dtype, hq, splits, what):
    """tests/ex_full_ref.sharp_bar on o and lse — max |kernel - fp64| <= 2 * max |baseline - fp64| + eps * max |fp64|, eps of the
    tensor dtype for o and of float32 for lse — over the call and over the sequence with keys alone; the dead sequence stays under
    hold's exact rules"""
    ro, rlse = expected(form, dtype, hq)
    bo, bl = baseline(form, dtype, hq, splits)
    bad, ratios, used = db.sharp_rows(o.cpu(), lse.cpu(), ro, rlse, bo, bl, dtype, db.mla_groups(LENS))
    top = lambda t: max([g[t] for n, g in ratios.items() if n != "call" and t in g], default=0.0)   # noqa: E731
    kernel = what.split(": ")[1].split("<")[0]
    print(f"decode_sweep_ratio {ident(form, dtype, hq, splits)} o={ratios['call'].get('o', 0.0):.3f} lse={ratios['call'].get('lse', 0.0):.3f} "
          f"per sequence o={top('o'):.3f} lse={top('lse'):.3f} used={used:.3f} "
          f"family={kernel}<{'lists' if form == 'lists' else 'dense'}>+{'mla_combine_kernel' if splits > 1 else 'direct'}")
    assert not bad, f"sharp bar {what}: " + "; ".join(bad)


def run_16bit(form, dtype, hq, splits):
    """(contiguous, paged, paged again), each (o, lse) on the device"""
    pool, cont = caches(dtype)
    q, dpool, dcont, dtab = queries(dtype, hq).to(DEV), pool.to(DEV), cont.to(DEV), pools()[2].to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    if form == "dense":
        return [qv_call(q, cache, tab, lens, num_splits=splits) for cache, tab in ((dcont, None), (dpool, dtab), (dpool, dtab))]
    ix = lists().to(DEV)
    return [sparse_call(q, cache, ix, tab, lens, num_splits=splits) for cache, tab in ((dcont, None), (dpool, dtab), (dpool, dtab))]


def run_packed(form, hq, splits):
    """(packed, 16-bit paged on the dequantised pool, packed again)"""
    rows, pool16, table = pools()
    q, d8, d16, dtab = queries(BF16, hq).to(DEV), rows.to(DEV), pool16.to(DEV), table.to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    ix = lists().to(DEV) if form == "lists" else None
    packed = [fm(q, d8, dtab, lens, is_fp8_kvcache=True, indices=ix, num_splits=splits) for _ in range(2)]
    wide = qv_call(q, d16, dtab, lens, num_splits=splits) if form == "dense" else sparse_call(q, d16, ix, dtab, lens, num_splits=splits)
    return [packed[0], wide, packed[1]]


def hold(outs, form, dtype, hq, what, splits):
    """outs = (a call, the call it must equal bit for bit, the first call repeated)"""
    ro, rlse = expected(form, dtype, hq)
    (o, lse), (o2, lse2), (o3, lse3) = outs
    assert o.shape == (len(LENS), 1, hq, 512) and o.dtype == dtype and lse.shape == (len(LENS), hq, 1) and lse.dtype == torch.float32
    check(o, lse, ro, rlse, dtype)
    check(o2, lse2, ro, rlse, dtype)
    assert torch.equal(o, o2) and torch.equal(lse, lse2), what
    assert torch.equal(o, o3) and torch.equal(lse, lse3), "a repeated call"
    sharp_out(o, lse, form, dtype, hq, splits, what)
    dead = LENS.index(0)
    assert (o[dead] == 0).all() and (lse[dead] == -float("inf")).all() and torch.isfinite(lse[1 - dead]).all()


def ident(form, dtype, hq, splits):
    return f"{form}_{'bf16' if dtype == BF16 else 'f16'}_hq{hq}_w{WAVES[hq]}_s{splits}"


@pytest.mark.parametrize("form,dtype,hq,splits", CASES, ids=[ident(*c) for c in CASES])
def test_16_bit_routes(form, dtype, hq, splits):
    cont, paged, again = run_16bit(form, dtype, hq, splits)
    hold((paged, cont, again), form, dtype, hq, "paged against contiguous: " + ", ".join(routes(form, dtype, hq)), splits)


@pytest.mark.parametrize("form,hq,splits", PACKED, ids=[ident(f, BF16, h, s) for f, h, s in PACKED])
def test_packed_routes(form, hq, splits):
    hold(run_packed(form, hq, splits), form, BF16, hq, "packed against 16-bit paged: " + routes(form, BF16, hq, True)[0], splits)
