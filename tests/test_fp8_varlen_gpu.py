"""GPU: the packed and the paged form of the fp8 call (csrc/fa_fp8_inputs.hip: fp8in_vt_varlen_kernel, fwd_fp8in_varlen_kernel;
flash_attention_fp8_varlen) on the sequence sets of tests/fp8_varlen_cases.py.  The contract: every sequence has the
bits of flash_attention_fp8 on that sequence alone.  Also: packed = paged, untrusted tables and offsets, the V^T bytes of the
gathering transposer, the sharp bar of tests/test_fp8_inputs_gpu.py per sequence, the GQA / descale / view identities and a graph
replay with changed offsets, table and descales.  The models behind the builders are proved on the CPU
(tests/test_fp8_varlen_cpu.py)."""
import functools

import pytest
import torch

from common.attention_ex import flash_attention_fp8, flash_attention_fp8_varlen
from tests import fp8_inputs_ref as fr
from tests import fp8_varlen_cases as vc
from tests.fp8_ref import SENTINEL, tiled_sharp_bar

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4M3 = torch.float8_e4m3fn
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
HEADS = {"shuffled": (4, 2), "shared": (4, 1), "strided": (2, 2)}      # H_kv in {1, 2, H_q}
NINF = float("-inf")


@functools.lru_cache(maxsize=None)
def _call(setname, ps, table):
    hq, hkv = HEADS[table]
    return vc.build_paged(vc.SETS[setname], hq, hkv, ps, table, seed=100 * ps + len(table) + ord(setname))


def strided_pool(pool, extra_token, extra_page):
    """the pool as a view with padded token and page strides into a 0x7F-filled buffer"""
    nb, ps, hkv, d = pool.shape
    ts = hkv * d + extra_token
    pst = ps * ts + extra_page
    flat = torch.full((nb * pst + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(flat, (nb, ps, hkv, d), (pst, ts, d, 1), 16)
    view.copy_(pool.to(DEV))
    return view


def device_args(call, form, **over):
    """(q, k, v, cu_q, cu_k, max_q, max_k, keywords) of the call on the device; form "paged" or "packed"""
    c = dict(call, **over)
    q = c["q8"].to(DEV).view(E4M3)
    kw = {n: c[n].to(DEV) for n in ("q_descale", "k_descale", "v_descale") if c[n] is not None}
    if form == "paged":
        if c["strided"]:
            k, v = strided_pool(c["pool_k"], 128, 256).view(E4M3), strided_pool(c["pool_v"], c["hkv"] * 128, 1024).view(E4M3)
        else:
            k, v = c["pool_k"].to(DEV).view(E4M3), c["pool_v"].to(DEV).view(E4M3)
        kw["block_table"] = c["block_table"].to(DEV)
        cu_k = c["cu_k"]
    else:
        k8, v8, cu_k = vc.packed_kv(c)
        k, v = k8.to(DEV).view(E4M3), v8.to(DEV).view(E4M3)
    return q, k, v, c["cu_q"].to(DEV), cu_k.to(DEV), c["max_q"], c["max_k"], kw


def run(call, form, causal, dtype, **over):
    q, k, v, cu_q, cu_k, mq, mk, kw = device_args(call, form, **over)
    o, lse = flash_attention_fp8_varlen(q, k, v, cu_q, cu_k, mq, mk, causal=causal, out_dtype=dtype, return_softmax_lse=True, **kw)
    torch.cuda.synchronize()
    assert o.shape == (q.shape[0], call["hq"], 128) and o.dtype == dtype and lse.shape == (call["hq"], q.shape[0]) and lse.dtype == torch.float32
    return o.cpu(), lse.cpu()


def padded(call, b, causal, dtype, lq=None, lk=None):
    """(o (lq, H_q, 128), lse (H_q, lq)) of flash_attention_fp8 with B = 1 on sequence b's tokens (bnhd), the first lq rows and lk
    keys of them; an empty side: what the contract says (nothing, or o = 0 and lse = -inf)"""
    nq, nk = call["seqs"][b]
    lq, lk = nq if lq is None else min(lq, nq), nk if lk is None else min(lk, nk)
    hq = call["hq"]
    if lq == 0 or lk == 0:
        return torch.zeros((lq, hq, 128), dtype=dtype), torch.full((hq, lq), NINF)
    qs = int(call["cu_q"][b])
    q = call["q8"][qs:qs + lq][None].to(DEV).view(E4M3)
    k, v = (call[n][b][:lk][None].to(DEV).view(E4M3) for n in ("k8", "v8"))
    ds = {n: call[n][b:b + 1].to(DEV) for n in ("q_descale", "k_descale", "v_descale") if call[n] is not None}
    o, lse = flash_attention_fp8(q, k, v, causal=causal, out_dtype=dtype, layout="bnhd", return_lse=True, **ds)
    return o[0].cpu(), lse[0].cpu()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_sequences_equal_padded(call, got, causal, dtype, max_q=None, max_k=None):
    o, lse = got
    for b in range(len(call["seqs"])):
        want_o, want_lse = padded(call, b, causal, dtype, max_q, max_k)
        qs, n = int(call["cu_q"][b]), want_o.shape[0]
        assert torch.equal(bits(o[qs:qs + n]), bits(want_o)), (b, call["seqs"][b])
        assert torch.equal(bits(lse[:, qs:qs + n]), bits(want_lse)), (b, call["seqs"][b])


FORMS = [("packed", 16, "shuffled")] + [("paged", ps, table) for ps in vc.PAGE_SIZES for table in vc.TABLES]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("form,ps,table", FORMS, ids=[f"{f}-{p}-{t}" if f == "paged" else f for f, p, t in FORMS])
@pytest.mark.parametrize("setname", list(vc.SETS))
def test_every_sequence_has_the_bits_of_the_padded_call(setname, form, ps, table, causal, dtype):
    call = _call(setname, ps, table)
    got = run(call, form, causal, DTYPES[dtype])
    assert_sequences_equal_padded(call, got, causal, DTYPES[dtype])


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("ps,table", [(16, "shared"), (48, "strided"), (256, "shuffled")])
@pytest.mark.parametrize("setname", list(vc.SETS))
def test_packed_and_paged_give_equal_bits(setname, ps, table, causal):
    call = _call(setname, ps, table)
    a, b = run(call, "packed", causal, torch.bfloat16), run(call, "paged", causal, torch.bfloat16)
    live = torch.zeros(a[0].shape[0], dtype=torch.bool)                 # (every row of these sets belongs to a sequence)
    live[:int(call["cu_q"][-1])] = True
    assert bool(live.all()) and torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("ps", [16, 48])
def test_a_page_outside_the_pool_reads_as_zero_bytes(ps):
    call = dict(_call("B", ps, "shuffled"))
    bt = call["block_table"].clone()
    nb = call["pool_k"].shape[0]
    bt[1, 2] = -1                     # sequence (64, 300): its third page
    bt[3, 1] = nb                     # sequence (17, 191): its second page
    bt[0, 0] = 2 ** 31 - 1            # sequence (257, 129): its first page
    call["block_table"] = bt
    call["k8"] = [vc.gather(call["pool_k"], bt[b], lk, ps) for b, (_lq, lk) in enumerate(call["seqs"])]
    call["v8"] = [vc.gather(call["pool_v"], bt[b], lk, ps) for b, (_lq, lk) in enumerate(call["seqs"])]
    assert bool((call["k8"][1][2 * ps:3 * ps] == 0).all()) and bool((call["v8"][0][:ps] == 0).all())
    for causal in (False, True):
        got = run(call, "paged", causal, torch.bfloat16)
        assert bool(torch.isfinite(got[0].float()).all())
        assert_sequences_equal_padded(call, got, causal, torch.bfloat16)


def test_garbage_past_the_live_entries_and_nan_bytes_outside_live_tokens_change_nothing():
    call = _call("B", 48, "shuffled")
    plain = run(call, "paged", True, torch.float16)
    bt = call["block_table"].clone()
    for b, (_lq, lk) in enumerate(call["seqs"]):
        bt[b, (lk + 47) // 48:] = torch.tensor([-7, 2 ** 30, 0, 1, -1, 5, 3])[:bt.shape[1] - (lk + 47) // 48]
    assert not torch.equal(bt, call["block_table"])
    got = run(call, "paged", True, torch.float16, block_table=bt)
    assert torch.equal(bits(got[0]), bits(plain[0])) and torch.equal(bits(got[1]), bits(plain[1]))
    # the builder leaves 0x7F (e4m3 NaN) in every pool byte no live token owns; zeros there give the same bits
    pk, pv = call["pool_k"].clone(), call["pool_v"].clone()
    dead = (pk == SENTINEL).all(-1).all(-1)
    assert bool(dead.any())
    pk[dead], pv[dead] = 0, 0
    got = run(call, "paged", True, torch.float16, pool_k=pk, pool_v=pv)
    assert torch.equal(bits(got[0]), bits(plain[0])) and torch.equal(bits(got[1]), bits(plain[1]))
    assert bool(torch.isfinite(plain[0].float()).all()) and not bool(torch.isnan(plain[1]).any())


@pytest.mark.parametrize("form", ["packed", "paged"])
def test_lengths_above_the_maxima_are_clamped_and_nothing_else_is_written(form):
    """through the C entry point on caller buffers cut out of sentinel-filled ones: max_seqlen_q = 200 and max_seqlen_k = 100 clamp
    the sequences of set B, each result is the padded call on the clamped lengths, and the rows past a clamped length, like
    everything outside o and lse, keep the sentinel"""
    import flashattention_lab_cuda as ext

    call = _call("B", 16, "shuffled")
    mq, mk = 200, 100
    q, k, v, cu_q, cu_k, _mq, _mk, kw = device_args(call, form)
    total_q, hq, hkv, B = q.shape[0], call["hq"], call["hkv"], len(call["seqs"])
    obuf = torch.full((total_q * hq * 128 + 2048,), -1, dtype=torch.int16, device=DEV)
    lbuf = torch.full((hq * total_q + 2048,), -1, dtype=torch.int32, device=DEV)
    o, lse = obuf[1024:-1024], lbuf[1024:-1024]
    bt = kw.get("block_table")
    pages = (bt.shape[1], k.shape[0], k.shape[1], k.stride(0), v.stride(0)) if form == "paged" else (0, 0, 0, 0, 0)
    total_k = 0 if form == "paged" else k.shape[0]
    need = int(ext._lib.fa_fp8_forward_varlen_workspace_bytes(B, hkv, total_k, mk, pages[0], pages[2], 128))
    assert need == vc.workspace_bytes(B, hkv, total_k, mk, pages[0], pages[2])
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    ext._call("fa_fp8_forward_varlen", (
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), kw["q_descale"].data_ptr(), kw["k_descale"].data_ptr(),
        kw["v_descale"].data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), bt.data_ptr() if form == "paged" else 0, B, hq, hkv, total_q, total_k,
        mq, mk, 128, 2, q.stride(0), q.stride(1), k.stride(-3), k.stride(-2), v.stride(-3), v.stride(-2), *pages, hkv, hkv, hkv, 1,
        128 ** -0.5, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ob, lb = obuf.cpu(), lbuf.cpu()
    assert bool((ob[:1024] == -1).all()) and bool((ob[-1024:] == -1).all()) and bool((lb[:1024] == -1).all()) and bool((lb[-1024:] == -1).all())
    got_o, got_lse = ob[1024:-1024].reshape(total_q, hq, 128), lb[1024:-1024].reshape(hq, total_q)
    written = torch.zeros(total_q, dtype=torch.bool)
    for b, (lq, _lk) in enumerate(call["seqs"]):
        qs = int(call["cu_q"][b])
        written[qs:qs + min(lq, mq)] = True
    assert bool((~written).any())
    assert bool((got_o[~written] == -1).all()) and bool((got_lse[:, ~written] == -1).all())
    assert_sequences_equal_padded(call, (got_o.view(torch.bfloat16), got_lse.view(torch.float32)), True, torch.bfloat16, mq, mk)


@pytest.mark.parametrize("form,ps", [("packed", 16), ("paged", 16), ("paged", 48), ("paged", 256)])
@pytest.mark.parametrize("setname", list(vc.SETS))
def test_the_transposer_writes_every_sequence_its_image_and_nothing_else(setname, form, ps, monkeypatch):
    """V^T in a workspace cut out of a 0x7F buffer: every sequence's region holds tests/fp8_inputs_ref.py's expected image of that
    sequence alone, and every other byte keeps the sentinel"""
    import flashattention_lab_cuda as ext

    call = _call(setname, ps, "shuffled")
    B, hkv = len(call["seqs"]), call["hkv"]
    if form == "paged":
        max_blocks = call["block_table"].shape[1]
        need = vc.workspace_bytes(B, hkv, 0, call["max_k"], max_blocks, ps)
        regions = vc.paged_regions(call["cu_k"].tolist(), call["max_k"], max_blocks, ps)
    else:
        cu_k = vc.packed_kv(call)[2].tolist()
        need = vc.workspace_bytes(B, hkv, cu_k[-1], call["max_k"])
        regions = vc.packed_regions(cu_k, cu_k[-1], call["max_k"])
    buf = torch.full((need + 8192,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = buf[4096:4096 + need]
    monkeypatch.setattr(ext, "_workspace", lambda device, nbytes: ws if nbytes == need else None)
    run(call, form, False, torch.bfloat16)
    got = buf.cpu()
    assert bool((got[:4096] == SENTINEL).all()) and bool((got[4096 + need - 256:] == SENTINEL).all())
    tiles = got[4096:4096 + need - 256].reshape(hkv, -1, 128, 128)
    untouched = torch.ones(tiles.shape[1], dtype=torch.bool)
    for b, (first, n) in enumerate(regions):
        if n == 0:
            continue
        want = fr.expected_v8t(vc.padded_call(call, b, False, torch.bfloat16))          # (hkv, n, 128, 128)
        assert want.shape[1] == n and torch.equal(tiles[:, first:first + n], want), (b, first, n)
        assert bool(untouched[first:first + n].all())
        untouched[first:first + n] = False
    assert bool(untouched.any()) and bool((tiles[:, untouched] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _references(setname, causal, dtype):
    call = _call(setname, 16, "shuffled")
    out = {}
    for b, (lq, lk) in enumerate(call["seqs"]):
        if lq and lk:
            one = vc.padded_call(call, b, causal, DTYPES[dtype])
            out[b] = (fr.reference(one), fr.baseline(one))
    return out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("form", ["packed", "paged"])
@pytest.mark.parametrize("setname", list(vc.SETS))
def test_every_sequence_meets_the_sharp_bar(setname, form, causal, dtype):
    """the bar tests/test_fp8_inputs_gpu.py holds the padded call to (tiled_sharp_bar: §9l-2's bar per 256-row tile, factor 2, on o
    and lse), per sequence against the fp64 reference and the rounding-point baseline of tests/fp8_inputs_ref.py"""
    call = _call(setname, 16, "shuffled")
    o, lse = run(call, form, causal, DTYPES[dtype])
    for b, (lq, lk) in enumerate(call["seqs"]):
        qs = int(call["cu_q"][b])
        if lq == 0:
            continue
        got = fr._result(o[qs:qs + lq].transpose(0, 1).contiguous(), lse[:, qs:qs + lq].contiguous())
        if lk == 0:
            assert bool((got.o == 0).all()) and bool((got.lse == NINF).all())
            continue
        ref, base = _references(setname, causal, dtype)[b]
        dead = ~torch.isfinite(ref.lse)
        assert not bool(torch.isnan(got.lse).any()) and torch.equal(got.lse == NINF, dead)
        assert bool(torch.isfinite(got.o.float()).all()) and bool((got.o[dead] == 0).all())
        bad, ratio = tiled_sharp_bar(got, ref, base, DTYPES[dtype])
        print(setname, form, call["seqs"][b], " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
        assert not bad, (b, bad)
    if setname == "A" and causal:
        ref = _references(setname, causal, dtype)[3][0]
        assert bool((~torch.isfinite(ref.lse))[:, :256].all())          # (300, 40): the whole first query tile is dead


@pytest.mark.parametrize("form", ["packed", "paged"])
def test_gqa_is_the_ungrouped_call_on_repeated_heads(form):
    for table, g in (("shuffled", 2), ("shared", 4)):
        call = _call("B", 48, table)
        rep = lambda t: t.repeat_interleave(g, dim=-2)   # noqa: E731
        wide = dict(call, hkv=call["hq"], pool_k=rep(call["pool_k"]), pool_v=rep(call["pool_v"]), k8=[rep(t) for t in call["k8"]],
                    v8=[rep(t) for t in call["v8"]], **{n: call[n].repeat_interleave(g, dim=1) for n in ("q_descale", "k_descale", "v_descale")})
        a, b = run(call, form, True, torch.bfloat16), run(wide, form, True, torch.bfloat16)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("form", ["packed", "paged"])
def test_power_of_two_descales_and_a_second_run(form):
    call = _call("B", 256, "shuffled")
    B, hkv = len(call["seqs"]), call["hkv"]
    none = dict(q_descale=None, k_descale=None, v_descale=None)
    q, k, v, cu_q, cu_k, mq, mk, kw = device_args(call, form, **none)
    f = lambda **over: flash_attention_fp8_varlen(q, k, v, cu_q, cu_k, mq, mk, causal=True, return_softmax_lse=True, **dict(kw, **over))   # noqa: E731
    # q and k descales that are powers of two are the softmax scale
    plain = f(softmax_scale=128 ** -0.5 * 2.0 ** (3 - 5))
    got = f(q_descale=torch.full((B, hkv), 8.0, device=DEV), k_descale=torch.full((hkv,), 2.0 ** -5, device=DEV))
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # a power-of-two v descale scales o exactly and leaves lse alone
    plain = f()
    again = f()
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])       # two runs, the same bits
    vd = torch.exp2(torch.arange(B * hkv, dtype=torch.float32) - 2.0).reshape(B, hkv)
    got = f(v_descale=vd.to(DEV))
    per_token = torch.ones((q.shape[0], call["hq"], 1))
    for b in range(B):
        per_token[int(call["cu_q"][b]):int(call["cu_q"][b + 1])] = vd[b].repeat_interleave(call["hq"] // hkv)[None, :, None]
    assert torch.equal(got[0].float().cpu(), plain[0].float().cpu() * per_token) and torch.equal(got[1], plain[1])


@pytest.mark.parametrize("form", ["packed", "paged"])
def test_a_strided_q_view_equals_its_contiguous_copy(form):
    call = _call("B", 16, "shuffled")
    q, k, v, cu_q, cu_k, mq, mk, kw = device_args(call, form)
    total_q, hq = q.shape[0], q.shape[1]
    fused = torch.full((total_q, 3, hq + 1, 128), SENTINEL, dtype=torch.uint8, device=DEV)     # a token- and head-padded projection
    fused[:, 1, :hq] = q.view(torch.uint8)
    view = fused.view(E4M3)[:, 1, :hq]
    assert not view.is_contiguous() and view.stride(0) == 3 * (hq + 1) * 128
    f = lambda x: flash_attention_fp8_varlen(x, k, v, cu_q, cu_k, mq, mk, causal=True, out_dtype=torch.float16, return_softmax_lse=True, **kw)   # noqa: E731
    a, b = f(view), f(q)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and a head-strided one: every second head of a wider tensor
    wide = torch.full((total_q, 2 * hq, 128), SENTINEL, dtype=torch.uint8, device=DEV)
    wide[:, ::2] = q.view(torch.uint8)
    c = f(wide.view(E4M3)[:, ::2])
    assert torch.equal(c[0], b[0]) and torch.equal(c[1], b[1])


def test_graph_replay_with_changed_offsets_table_and_descales():
    first = _call("B", 48, "shuffled")
    second = vc.build_paged(tuple(reversed(vc.SET_B)), first["hq"], first["hkv"], 48, "shuffled", seed=4242)
    assert second["block_table"].shape == first["block_table"].shape and second["pool_k"].shape == first["pool_k"].shape
    assert (second["max_q"], second["max_k"]) == (first["max_q"], first["max_k"])
    # (the second table makes other tokens live: no NaN byte anywhere in these pools)
    finite = {n: torch.where(first[n] == SENTINEL, torch.tensor(0x30, dtype=torch.uint8), first[n]) for n in ("pool_k", "pool_v")}
    q, k, v, cu_q, cu_k, mq, mk, kw = device_args(first, "paged", **finite)
    f = lambda: flash_attention_fp8_varlen(q, k, v, cu_q, cu_k, mq, mk, causal=True, return_softmax_lse=True, **kw)   # noqa: E731
    f()                                         # warm-up (workspace, modules)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = f()
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    eager = f()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    before = out[0].clone()
    cu_q.copy_(second["cu_q"])
    cu_k.copy_(second["cu_k"])
    kw["block_table"].copy_(second["block_table"])
    for n in ("q_descale", "k_descale", "v_descale"):
        kw[n].copy_(second[n])
    graph.replay()
    torch.cuda.synchronize()
    eager = f()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    assert not torch.equal(out[0], before)
