"""GPU: the lightning indexer (common/indexer.py; fa_indexer_pack, fa_indexer_logits, fa_indexer_topk).  The logits at the sharp
fp64 bar per (sequence, 256-key band) over the pairwise table of tests/indexer_ref.py, and exactly the visible entries written; the
untrusted lengths and table; the selection bit for bit against indexer_ref.select; the chain; the lists into flash_mla_sparse_attn;
the append byte for byte; graph capture and replay; one raw ctypes call of each entry point.  At most 1000 keys a sequence in the
logits (the largest length of the table) and 70 001 in the selection (more than a 64 K row, an odd tail)."""
import ctypes
import functools

import pytest
import torch

from tests import indexer_ref as ir

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC12345   # a NaN pattern no kernel result has
IDS = ["-".join(f"{k}{v}" for k, v in c.items()).replace(" ", "") for c in ir.CASES]


def api():
    from common import indexer

    return indexer


def sentinel_like(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(i):
    call = ir.build_call(ir.CASES[i], 100 + i)
    pool, table = ir.paged(call, 200 + i)
    return call, pool, table, ir.reference(call), ir.baseline(call)


def gpu_logits(call, pool, table, lens=None, out=None, width=None):
    q = call["q8"].to(DEV).view(torch.float8_e4m3fn)
    lens = torch.tensor(call["lens"] if lens is None else lens, dtype=torch.int32, device=DEV)
    return api().indexer_logits(q, call["w"].to(DEV), pool.to(DEV), lens, table.to(DEV), causal=call["causal"], out=out, width=width)


def written(out):
    """float32 CPU copy with NaN where the sentinel survived"""
    o = out.cpu()
    return torch.where(bits(o) == SENTINEL, torch.full_like(o, float("nan")), o)


# ---- 1. the logits at the sharp bar, and exactly the visible entries written
@pytest.mark.parametrize("i", range(len(ir.CASES)), ids=IDS)
def test_logits_at_the_sharp_bar_and_only_visible_entries_are_written(i):
    call, pool, table, ref, base = case(i)
    b, nq = call["q8"].shape[:2]
    out = sentinel_like((b, nq, call["cap"]))
    got = gpu_logits(call, pool, table, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = written(got)
    assert torch.equal(torch.isnan(got), ~ir.visible(call)), "the written entries are not exactly the visible ones"
    for (sq, band, err, big), (_s, _b, eb, _g) in zip(ir.band_errors(got, ref, call["lens"]), ir.band_errors(base, ref, call["lens"])):
        print(f"case {i} sequence {sq} band {band}: kernel {err:.3e} baseline {eb:.3e} max |fp64| {big:.3e}")
    bad = ir.sharp_bar(got, ref, base, call["lens"])
    assert not bad, bad


# ---- 2. untrusted lengths and table
def _untrusted_call():
    c = dict(heads=32, nq=2, lens=(144, 0, 50), page=16, causal=True, stride=144)
    call = ir.build_call(c, 7)
    assert call["cap"] == 144
    pool, table = ir.paged(call, 8)
    # sequence 2 reads sequence 0's first three pages (shared) and a fourth of its own
    k8, ks = call["k8"].clone(), call["ks"].clone()
    k8[2, :48], ks[2, :48] = k8[0, :48], ks[0, :48]
    table[2, :3] = table[0, :3]
    call = dict(call, k8=k8, ks=ks)
    return call, pool, table


def test_untrusted_lengths_table_and_poisoned_tokens_give_the_clean_bits():
    call, pool, table = _untrusted_call()
    clean = gpu_logits(call, pool, table, out=sentinel_like((3, 2, 144))).cpu()
    dirty_pool, dirty_table = pool.clone(), table.clone()
    nblk = pool.shape[0]
    nan_scale = torch.tensor([float("nan")]).view(torch.uint8)
    seen = set(int(p) for p in table[0]) | set(int(p) for p in table[2, :4])
    for pg in range(nblk):                       # every token no row can see: NaN codes and a NaN scale
        for slot in range(16):
            if pg not in seen or (pg == int(table[2, 3]) and slot >= 50 - 48):
                dirty_pool[pg, slot, 0, :128] = 0x7F
                dirty_pool[pg, slot, 0, 128:132] = nan_scale
    dirty_table[1] = torch.tensor([-1, nblk, 2 ** 31 - 1, -2 ** 31, 5, 6, 7, nblk + 9, -7], dtype=torch.int32)   # length 0: never read
    dirty_table[2, 4:] = torch.tensor([-1, nblk, 2 ** 31 - 1, -2 ** 31, 12345], dtype=torch.int32)             # past ceil(50 / 16)
    dirty = gpu_logits(call, dirty_pool, dirty_table, lens=(10 ** 6, -5, 50), out=sentinel_like((3, 2, 144))).cpu()
    assert torch.equal(bits(dirty), bits(clean))
    ref, base = ir.reference(call), ir.baseline(call)
    assert not ir.sharp_bar(written(clean), ref, base, call["lens"])
    # a narrower result clamps the lengths to its width
    narrow = gpu_logits(call, pool, table, out=sentinel_like((3, 2, 100)), width=100).cpu()
    call100 = dict(call, lens=(100, 0, 50), k8=call["k8"][:, :100], ks=call["ks"][:, :100])
    assert torch.equal(torch.isnan(written(narrow)), ~ir.visible(call100))
    assert not ir.sharp_bar(written(narrow), ir.reference(call100), ir.baseline(call100), call100["lens"])


def test_a_visible_page_outside_the_pool_gives_logit_zero():
    call, pool, table = _untrusted_call()
    table = table.clone()
    table[0, 2], table[2, 1] = pool.shape[0] + 3, -1
    got = written(gpu_logits(call, pool, table, out=sentinel_like((3, 2, 144))))
    assert torch.equal(torch.isnan(got), ~ir.visible(call))
    assert bool((got[0, 1, 32:48] == 0).all()) and bool((got[2, 1, 16:32] == 0).all())
    k8, ks = call["k8"].clone(), call["ks"].clone()
    k8[0, 32:48], ks[0, 32:48], k8[2, 16:32], ks[2, 16:32] = 0, 0, 0, 0
    zeroed = dict(call, k8=k8, ks=ks)
    assert not ir.sharp_bar(got, ir.reference(zeroed), ir.baseline(zeroed), call["lens"])


# ---- 3. the selection, exact
SPECIALS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
            0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000]
ROW_KINDS = ("random", "equal", "two_values", "specials", "ascending", "descending", "few_distinct")


def rows_of(length, seed):
    """float32 (len(ROW_KINDS), 1, length + 3): one row a kind, NaN patterns in the three entries past the length"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    rows.append(torch.randn(length, generator=g))
    rows.append(torch.full((length,), 0.75))
    rows.append(torch.where(torch.rand(length, generator=g) < 0.3, torch.tensor(1.0), torch.tensor(0.5)))   # the tie spans every chunk
    sp = torch.tensor([s - (1 << 32) if s >= 1 << 31 else s for s in SPECIALS], dtype=torch.int32)
    pick = torch.randint(0, len(SPECIALS) * 2, (length,), generator=g)
    rows.append(torch.where(pick < len(SPECIALS), sp[pick % len(SPECIALS)].view(torch.float32), torch.randn(length, generator=g)))
    rows.append(torch.arange(length).float() - length / 2)
    rows.append(length / 2 - torch.arange(length).float())
    rows.append(torch.randint(-2, 3, (length,), generator=g).float())
    x = torch.stack(rows).view(len(rows), 1, length)
    return torch.cat([x, torch.full((len(rows), 1, 3), float("nan"))], dim=2)


@pytest.mark.parametrize("length", (1, 255, 256, 257, 4097, 70001))
def test_selection_is_the_model_bit_for_bit(length):
    logits = rows_of(length, length)
    dl = logits.to(DEV)
    lens = [length] * logits.shape[0]
    dlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for topk in (1, 16, 64, 2048, 2049):
        got = api().indexer_topk(dl, dlens, topk, causal=False)
        again = api().indexer_topk(dl, dlens, topk, seqlen_q=1, causal=False)
        assert got.dtype == torch.int32 and got.shape == (logits.shape[0], 1, topk)
        assert torch.equal(got, again)
        want = ir.select_all(logits, lens, topk, False)
        for r, kind in enumerate(ROW_KINDS):
            assert torch.equal(got[r].cpu(), want[r]), (length, topk, kind)


def test_selection_around_n_equal_topk_and_rows_without_a_key():
    g = torch.Generator().manual_seed(5)
    topk, nq = 64, 5
    logits = torch.randn((4, nq, 80), generator=g)
    lens = [topk + 1, 2, 0, 80]        # sequence 0, causal: n = 61 .. 65 (topk - 1, topk, topk + 1 among them); sequence 1: n = 0, 0, 0, 1, 2
    for causal in (True, False):
        got = api().indexer_topk(logits.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), topk, causal=causal).cpu()
        assert torch.equal(got, ir.select_all(logits, lens, topk, causal)), causal
    got = api().indexer_topk(logits.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), topk, causal=True).cpu()
    assert bool((got[1, :3] == -1).all()) and bool((got[2] == -1).all())
    assert got[0, 2].tolist() == list(range(63)) + [-1] and got[0, 3].tolist() == list(range(64)) and -1 not in got[0, 4].tolist()
    # untrusted lengths: clamped to [0, width]; an int is a length for every sequence; strided outputs
    big = api().indexer_topk(logits.to(DEV), torch.tensor([10 ** 6, -3, 80, 80], dtype=torch.int32, device=DEV), 16, causal=False).cpu()
    assert torch.equal(big, ir.select_all(logits, [80, 0, 80, 80], 16, False))
    wide = torch.full((4, nq, 40), 7, dtype=torch.int32, device=DEV)
    api().indexer_topk(logits.to(DEV), 80, 16, causal=True, out=wide[:, :, 8:24])
    assert torch.equal(wide[:, :, 8:24].cpu(), ir.select_all(logits, [80] * 4, 16, True))
    assert bool((wide[:, :, :8] == 7).all()) and bool((wide[:, :, 24:] == 7).all())


def test_the_fast_path_reads_no_logit():
    nan = torch.full((3, 2, 300), float("nan"), device=DEV)
    lens = [300, 17, 1]
    got = api().indexer_topk(nan, torch.tensor(lens, dtype=torch.int32, device=DEV), 512, causal=True).cpu()
    for b, n in enumerate(lens):
        for i in range(2):
            m = max(n - 2 + i + 1, 0)
            assert got[b, i].tolist() == list(range(m)) + [-1] * (512 - m)


# ---- 4. the chain
def test_the_chain_is_the_two_calls_and_the_model_on_its_own_logits():
    c = dict(heads=64, nq=5, lens=(1000, 130, 3), page=48, causal=True, stride=208)
    call = ir.build_call(c, 11)
    pool, table = ir.paged(call, 12)
    q, w, dpool, dtab = call["q8"].to(DEV).view(torch.float8_e4m3fn), call["w"].to(DEV), pool.to(DEV), table.to(DEV)
    lens = torch.tensor(call["lens"], dtype=torch.int32, device=DEV)
    for topk in (64, 200):
        chain = api().lightning_indexer(q, w, dpool, lens, dtab, topk, causal=True)
        logits = api().indexer_logits(q, w, dpool, lens, dtab, causal=True)
        two = api().indexer_topk(logits, lens, topk, causal=True)
        assert torch.equal(chain, two)
        assert torch.equal(chain.cpu(), ir.select_all(logits.cpu(), call["lens"], topk, True))
        assert torch.equal(chain, api().lightning_indexer(q, w, dpool, lens, dtab, topk, causal=True))


# ---- 5. into the consumer
def test_the_lists_feed_sparse_mla_attention():
    from common.attention_ex import flash_mla_sparse_attn

    c = dict(heads=32, nq=1, lens=(33, 20, 0), page=16, causal=True, stride=144)
    call = ir.build_call(c, 21)
    pool, table = ir.paged(call, 22)
    lens = torch.tensor(call["lens"], dtype=torch.int32, device=DEV)
    topk = 64
    ix = api().lightning_indexer(call["q8"].to(DEV).view(torch.float8_e4m3fn), call["w"].to(DEV), pool.to(DEV), lens, table.to(DEV), topk)
    hand = torch.full((3, 1, topk), -1, dtype=torch.int32)
    for b, n in enumerate(call["lens"]):
        hand[b, 0, :n] = torch.arange(n, dtype=torch.int32)
    assert torch.equal(ix.cpu(), hand)
    g = torch.Generator().manual_seed(23)
    q = torch.randn((3, 1, 16, 576), generator=g).to(torch.bfloat16).to(DEV)
    kv = torch.randn((pool.shape[0], 16, 1, 576), generator=g).to(torch.bfloat16).to(DEV)
    args = (q[..., 512:], q[..., :512], kv[..., 512:], kv[..., :512])
    kw = dict(cache_seqlens=lens, block_table=table.to(DEV), causal=True, return_softmax_lse=True)
    o1, l1 = flash_mla_sparse_attn(*args, ix, **kw)
    o2, l2 = flash_mla_sparse_attn(*args, hand.to(DEV), **kw)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)


# ---- 6. the append
def _new_keys(b, nnew, seed):
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn((b, nnew, 128), generator=g) * torch.exp2(torch.randint(-4, 4, (b, nnew, 1), generator=g).float())).to(torch.bfloat16)
    k[0, 0] = 0                                             # a zero row: scale 1
    k[1, 0] = k[1, 0].clamp(-3, 3)
    k[1, 0, 5] = 448.0 * 2 ** -6                            # amax exactly 448 * 2^k
    k[2, 1] = k[2, 1].clamp(-100, 100)
    k[2, 1, 77] = -448.0
    return k


@pytest.mark.parametrize("pow2", (False, True))
def test_append_is_the_model_byte_for_byte(pow2):
    page, mb, nblk, nnew = 16, 3, 8, 5
    k = _new_keys(4, nnew, 31)
    table = torch.tensor([[0, 1, 2], [3, nblk + 2, 4], [5, 6, 1], [7, 7, 7]], dtype=torch.int32)
    before = [0, 14, 44, -1]           # sequence 1 crosses onto a page outside the pool, 2 past the capacity 48, 3 is negative
    want = ir.scatter(torch.full((nblk, page, 1, 144), 0x7F, dtype=torch.uint8), ir.token_bytes(*ir.pack(k, pow2)), before, table, page)
    wide = torch.full((nblk, page, 1, 160), 0x7F, dtype=torch.uint8, device=DEV)
    dpool = wide[..., :144]            # a view of a wider allocation keeps its strides
    wide_k = torch.zeros((4, nnew, 256), dtype=torch.bfloat16, device=DEV)
    wide_k[..., 64:192] = k.to(DEV)
    assert api().indexer_pack_cache(wide_k[..., 64:192], dpool, torch.tensor(before, dtype=torch.int32, device=DEV), table.to(DEV),
                                    scale_pow2=pow2) is None
    assert torch.equal(dpool.cpu(), want)
    assert bool((wide[..., 144:] == 0x7F).all())
    assert bool((want[1, 12:, 0, :132] != 0x7F).any()) and all(bool((want[pg] == 0x7F).all()) for pg in (2, 4, 5, 6, 7))


def test_logits_on_a_pool_the_append_wrote():
    call, pool, table, ref, base = case(0)
    b, cap = 3, call["cap"]
    dpool = torch.full(pool.shape, 0x7F, dtype=torch.uint8, device=DEV)
    api().indexer_pack_cache(call["k_bf16"].to(DEV), dpool, 0, table.to(DEV))
    used = torch.zeros(pool.shape[0], dtype=torch.bool)
    used[table.reshape(-1).long()] = True
    assert torch.equal(dpool.cpu()[used], pool[used])
    out = sentinel_like((b, call["q8"].shape[1], cap))
    gpu_logits(call, dpool.cpu(), table, out=out)
    assert not ir.sharp_bar(written(out), ref, base, call["lens"])


# ---- 7. graph capture
def test_append_and_chain_replay_in_a_graph_after_everything_changed_in_place():
    page, mb, nblk, nnew, topk, h, nq = 16, 6, 20, 2, 16, 32, 2
    g = torch.Generator().manual_seed(41)
    dpool = torch.full((nblk, page, 1, 144), 0x7F, dtype=torch.uint8, device=DEV)
    dtab = torch.arange(3 * mb, dtype=torch.int32, device=DEV).view(3, mb)
    dbefore = torch.zeros((3,), dtype=torch.int32, device=DEV)
    dafter = torch.zeros((3,), dtype=torch.int32, device=DEV)
    dnew = torch.zeros((3, nnew, 128), dtype=torch.bfloat16, device=DEV)
    dq = torch.zeros((3, nq, h, 128), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    dw = torch.zeros((3, nq, h), dtype=torch.float32, device=DEV)

    def step():
        api().indexer_pack_cache(dnew, dpool, dbefore, dtab)
        return api().lightning_indexer(dq, dw, dpool, dafter, dtab, topk, causal=True)

    step()   # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = step()
    torch.cuda.current_stream().wait_stream(s)
    for seed, lens in ((50, (60, 0, 94)), (60, (95, 33, 17))):          # 95 + 2: the last token past the capacity 96
        table = torch.randperm(nblk, generator=g)[:3 * mb].view(3, mb).to(torch.int32)   # no page twice: no two tokens on one slot
        table[seed // 10 - 5, 1] = nblk                                 # a page outside the pool, read as zeros
        new = _new_keys(3, nnew, seed)
        start = torch.full((nblk, page, 1, 144), 0x7F, dtype=torch.uint8)
        start[..., :132] = ir.token_bytes(*ir.pack((torch.randn((nblk, page, 1, 128), generator=g) * 2).to(torch.bfloat16)))
        before = torch.tensor(lens, dtype=torch.int32)
        dtab.copy_(table)
        dnew.copy_(new)
        dpool.copy_(start)
        dbefore.copy_(before)
        dafter.copy_(before + nnew)
        dq.view(torch.uint8).copy_(ir.fp8_ref.e4m3_code(torch.randn((3, nq, h, 128), generator=g)))
        dw.copy_(torch.randn((3, nq, h), generator=g))
        graph.replay()
        torch.cuda.synchronize()
        want = ir.scatter(start.clone(), ir.token_bytes(*ir.pack(new)), lens, table, page)
        assert torch.equal(dpool.cpu(), want)
        logits = api().indexer_logits(dq, dw, want.to(DEV), dafter, dtab, causal=True)
        assert torch.equal(out, api().indexer_topk(logits, dafter, topk, causal=True))
        assert torch.equal(out.cpu(), ir.select_all(logits.cpu(), (before + nnew).tolist(), topk, True))


# ---- 8. the C ABI, one raw call of each entry point
def test_raw_ctypes_calls():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    page, mb, nblk, h = 16, 2, 3, 32
    g = torch.Generator().manual_seed(51)
    k = torch.randn((1, 20, 128), generator=g).to(torch.bfloat16)
    dk = k.to(DEV)
    dpool = torch.full((nblk, page, 1, 144), 0x7F, dtype=torch.uint8, device=DEV)
    dtab = torch.tensor([[2, 0]], dtype=torch.int32, device=DEV)
    zero = torch.zeros((1,), dtype=torch.int32, device=DEV)
    lens = torch.tensor([20], dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = lib.fa_indexer_pack(p(dk), p(dpool), p(zero), p(dtab), 1, 20, 128, 20 * 128, 128, page * 144, 144, mb, nblk, page, mb, 0, st)
    assert rc == 0, lib.fa_last_error().decode()
    table = dtab.cpu()
    want = ir.scatter(torch.full((nblk, page, 1, 144), 0x7F, dtype=torch.uint8), ir.token_bytes(*ir.pack(k)), [0], table, page)
    assert torch.equal(dpool.cpu(), want)
    q8 = ir.fp8_ref.e4m3_code(torch.randn((1, 1, h, 128), generator=g))
    w = torch.randn((1, 1, h), generator=g) * 0.02
    dq, dw = q8.to(DEV), w.to(DEV)
    out = sentinel_like((1, 1, 32))
    rc = lib.fa_indexer_logits(p(dq), p(dw), p(dpool), p(lens), p(dtab), p(out), 1, 1, h, 128, 32, h * 128, h * 128, 128, h, h, 32, 32,
                               page * 144, 144, mb, nblk, page, mb, 1, st)
    assert rc == 0, lib.fa_last_error().decode()
    k8, ks = ir.pack(k)
    call = dict(q8=q8, w=w, k8=torch.cat([k8, torch.zeros((1, 12, 128), dtype=torch.uint8)], 1), ks=torch.cat([ks, torch.zeros((1, 12))], 1),
                lens=[20], causal=True)
    got = written(out)
    assert torch.equal(torch.isnan(got), ~ir.visible(call))
    assert not ir.sharp_bar(got, ir.reference(call), ir.baseline(call), [20])
    ix = torch.full((1, 1, 8), 99, dtype=torch.int32, device=DEV)
    rc = lib.fa_indexer_topk(p(out), p(lens), p(ix), 1, 1, 32, 8, 32, 32, 8, 8, 1, st)
    assert rc == 0, lib.fa_last_error().decode()
    assert torch.equal(ix.cpu(), ir.select_all(out.cpu(), [20], 8, True))
