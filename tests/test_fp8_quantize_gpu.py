"""GPU: the fp8 quantiser (fa_fp8_quantize; common.attention_ex.quantize_fp8 / quantize_fp8_qkv) against the CPU model of
tests/fp8_quantize_ref.py.  The call is a pure function of IEEE operations, so the bar is BIT EQUALITY on codes and descales:
there is no tolerance anywhere in this file.  Shapes are the smallest that cross every boundary: one and several workgroups a
unit, both sides of the fused / two-pass threshold (asked of the library through route_count), odd lengths, every head dim class,
both dtypes, grouped and ungrouped scale units, empty sequences."""
import itertools

import pytest
import torch

from tests.fp8_quantize_ref import VALUES, make_x, quantize_model, rotate32, span, static_descales, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8, F8 = torch.uint8, torch.float8_e4m3fn
BF16, F16 = torch.bfloat16, torch.float16
ROUTES = ("fp8_quant_fused", "fp8_quant_two_pass", "fp8_quant_static")
FUSED_ITEMS = 1024          # include/fa_mi355x.h: a unit of at most this many 16-byte chunks is one fused launch


def routes():
    import flashattention_lab_cuda as ext

    return tuple(ext.route_count(r) for r in ROUTES)


def took(before):
    return tuple(a - b for a, b in zip(routes(), before))


def quantise(x, g=1, **kw):
    """quantize_fp8 on the device; (codes uint8, descale) back on the CPU, and the route the call took"""
    from common.attention_ex import quantize_fp8

    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and not v.is_cuda else v) for k, v in kw.items()}
    before = routes()
    x8, ds = quantize_fp8(x.to(DEV) if not x.is_cuda else x, g, **kw)
    route = took(before)
    assert x8.dtype == F8 and ds.dtype == torch.float32
    return x8.view(U8).cpu(), ds.cpu(), route


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else a.dtype),
                                               b.contiguous().view(torch.int32 if b.dtype == torch.float32 else b.dtype))


def expected_route(n, g, d, static=False):
    return (0, 0, 1) if static else (1, 0, 0) if n * g * (d // 8) <= FUSED_ITEMS else (0, 1, 0)


# ---- 1. dynamic, static and scale_pow2 equal the model; 2. static with the dynamic descale gives the dynamic codes

SHAPES = list(itertools.product(((4, 2), (3, 1), (8, 8)), (1, 63, 257, 1030), (16, 64, 128, 256)))


@pytest.mark.parametrize("hg,n,d", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_every_mode_equals_the_model(hg, n, d):
    (h, g), b = hg, 2
    idx = SHAPES.index((hg, n, d))
    for dtype in (BF16, F16):
        kind = VALUES[(idx + (dtype == F16)) % len(VALUES)]
        x = make_x(kind, (b, n, h, d), g, dtype, seed=idx)
        xd = x.to(DEV)
        want, wds = quantize_model(x, g)
        got, ds, route = quantise(xd, g)
        assert route == expected_route(n, g, d), (route, kind)
        assert same(ds, wds) and same(got, want), (kind, dtype)
        want2, wds2 = quantize_model(x, g, scale_pow2=True)
        got2, ds2, _ = quantise(xd, g, scale_pow2=True)
        assert same(ds2, wds2) and same(got2, want2), (kind, dtype)
        sd = static_descales((b, h // g) if idx % 2 else (h // g,), seed=idx + 1)
        want3, _ = quantize_model(x, g, descale=sd)
        got3, ds3, route3 = quantise(xd, g, descale=sd)
        assert route3 == (0, 0, 1) and same(ds3, sd) and same(got3, want3), (kind, dtype)
        # identity 2: the dynamic call's own descale, handed back, gives the dynamic codes
        again, _, _ = quantise(xd, g, descale=ds)
        assert same(again, got)
        # two runs, the same bits
        rerun, rds, _ = quantise(xd, g)
        assert same(rerun, got) and same(rds, ds)


@pytest.mark.parametrize("kind", VALUES)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_value_patterns_on_both_sides_of_the_threshold(kind, dtype):
    """g = 1, d = 128: 16 chunks a token, so 64 tokens are the last fused unit and 65 the first two-pass one"""
    for n, route in ((64, (1, 0, 0)), (65, (0, 1, 0))):
        x = make_x(kind, (2, n, 3, 128), 1, dtype, seed=40 + n)
        want, wds = quantize_model(x, 1)
        got, ds, took_ = quantise(x, 1)
        assert took_ == route
        assert same(ds, wds) and same(got, want)
        if kind == "ties":
            assert bool((ds == 1).all())
        if kind == "zero_units":
            assert bool((ds[0, 0] == 1)) and int(got[0, :, 0].max()) == 0


# ---- 3. cache consistency: the e4m3 cache append stores quantize_fp8's bytes

@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("rotary", [None, "neox", "gptj"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_the_cache_append_stores_these_bytes(d, rotary, paged):
    from common.attention_ex import flash_attn_with_kvcache, quantize_fp8

    b, hq, hkv, nnew, cap, ps, dtype = 2, 4, 2, 19, 48, 16, BF16
    g = torch.Generator().manual_seed(300 + d)
    q = torch.randn((b, 1, hq, d), generator=g).to(dtype).to(DEV)
    kn, vn = (torch.randn((b, nnew, hkv, d), generator=g).to(dtype).to(DEV) for _ in range(2))
    kd, vd = (static_descales((b, hkv), seed=310 + i).to(DEV) for i in range(2))
    rot = {}
    if rotary:
        cos, sin = tables(cap + 1, d // 2, dtype)
        rot = dict(rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=rotary == "gptj")
    lens = torch.zeros(b, dtype=torch.int32, device=DEV)
    if paged:
        nblk = b * cap // ps
        kc, vc = (torch.zeros((nblk, ps, hkv, d), dtype=U8, device=DEV).view(F8) for _ in range(2))
        table = torch.randperm(nblk, generator=g).to(torch.int32).view(b, cap // ps).to(DEV)
        flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, block_table=table, k_descale=kd, v_descale=vd, **rot)
        rows = lambda c: torch.stack([c.view(U8)[table[bb].long()].reshape(cap, hkv, d)[:nnew] for bb in range(b)])   # noqa: E731
    else:
        kc, vc = (torch.zeros((b, cap, hkv, d), dtype=U8, device=DEV).view(F8) for _ in range(2))
        flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=lens, k_descale=kd, v_descale=vd, **rot)
        rows = lambda c: c.view(U8)[:, :nnew]   # noqa: E731
    k8, kds = quantize_fp8(kn, 1, kd, **rot)
    v8, vds = quantize_fp8(vn, 1, vd)
    assert kds.data_ptr() == kd.data_ptr() and vds.data_ptr() == vd.data_ptr()      # static: the caller's own descales
    assert torch.equal(rows(kc), k8.view(U8)) and torch.equal(rows(vc), v8.view(U8))
    # and the quantiser writing straight into an empty cache's prefix leaves the cache the append leaves
    if not paged:
        kc2 = torch.zeros((b, cap, hkv, d), dtype=U8, device=DEV).view(F8)
        quantize_fp8(kn, 1, kd, out=kc2[:, :nnew], **rot)
        assert torch.equal(kc2.view(U8), kc.view(U8))


# ---- 4. fused rotary equals rotary_apply, then quantise

ROTARY = [(BF16, 128, 64, False, "int", 37), (F16, 64, 64, True, "vector", 37), (BF16, 256, 16, True, "int", 5),
          (F16, 128, 128, False, "vector", 130), (BF16, 64, 32, False, "vector", 1), (BF16, 128, 96, True, "zero", 70)]


@pytest.mark.parametrize("dtype,d,rdim,inter,offsets,n", ROTARY, ids=lambda v: str(v).replace("torch.", ""))
def test_fused_rotary_is_rotary_apply_then_quantise(dtype, d, rdim, inter, offsets, n):
    import flashattention_lab_cuda as ext

    b, h, g, ro = 3, 4, 2, 50
    gen = torch.Generator().manual_seed(400 + d + rdim)
    x = torch.randn((b, n, h, d), generator=gen).to(dtype)
    cos, sin = tables(ro, rdim, dtype)
    pos0 = {"zero": [0, 0, 0], "int": [11, 11, 11], "vector": [-3, 40, 7]}[offsets]      # tokens before and past the tables
    offs = torch.tensor(pos0, dtype=torch.int32, device=DEV) if offsets == "vector" else pos0[0]
    xd, cd, sd = x.to(DEV), cos.to(DEV), sin.to(DEV)
    kw = dict(rotary_cos=cd, rotary_sin=sd, rotary_interleaved=inter, seqlen_offsets=offs)
    rotated = ext.rotary_apply(xd, cd, sd, interleaved=inter, seqlen_offsets=offs)
    model_rot = rotate32(x, cos, sin, pos0, inter)
    print("16-bit values where rotary_apply and the fp32 model differ:", int((rotated.cpu().view(torch.int16) != model_rot.view(torch.int16)).sum()))
    for mode in (dict(), dict(scale_pow2=True), dict(descale=static_descales((b, h // g), seed=7).to(DEV))):
        fused, fds, route = quantise(xd, g, **mode, **kw)
        two, tds, _ = quantise(rotated, g, **mode)       # (a rotary pair counts once, so the two calls may take different routes)
        assert same(fused, two) and same(fds, tds), mode
        want, wds = quantize_model(model_rot, g, **mode) if "descale" not in mode else quantize_model(model_rot, g, descale=mode["descale"].cpu())
        assert same(fused, want) and same(fds, wds), mode


# ---- 5. layouts

def guarded(shape, dtype):
    """a tensor of `shape` cut out of a larger 0x7F-filled buffer: (the buffer as bytes, the view)"""
    n = 1
    for s in shape:
        n *= s
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n * size + 512,), 0x7F, dtype=U8, device=DEV)
    return buf, buf[256:256 + n * size].view(dtype).view(shape)


def untouched_around(buf, nbytes):
    return bool((buf[:256] == 0x7F).all()) and bool((buf[256 + nbytes:] == 0x7F).all())


@pytest.mark.parametrize("n", [5, 300])
def test_layouts_give_the_contiguous_bytes(n):
    from common.attention_ex import quantize_fp8

    b, hq, hkv, d, g = 2, 4, 2, 64, 2
    gen = torch.Generator().manual_seed(500 + n)
    qkv = torch.randn((b, n, hq + 2 * hkv, d), generator=gen).to(BF16).to(DEV)           # a fused projection
    x = qkv[:, :, :hq]                                                                    # its q slice: token stride 8 d
    ref8, refds, _ = quantise(x.contiguous(), g)
    want, wds = quantize_model(x.cpu(), g)
    assert same(ref8, want) and same(refds, wds)
    # the strided slice, read in place
    got, ds, _ = quantise(x, g)
    assert same(got, ref8) and same(ds, refds)
    # (B, H, N, d) in, (B, H, N, d) out and (B, N, H, d) out
    xh = x.permute(0, 2, 1, 3).contiguous()
    got, ds, _ = quantise(xh, g, layout="bhnd")
    assert same(got.permute(0, 2, 1, 3), ref8) and same(ds, refds)
    got, ds, _ = quantise(xh, g, layout="bhnd", out_layout="bnhd")
    assert same(got, ref8) and same(ds, refds)
    got, ds, _ = quantise(x, g, out_layout="bhnd")
    assert same(got.permute(0, 2, 1, 3), ref8)
    # out = the [:, :n] prefix of a larger cache and descale_out, both cut out of 0x7F-filled buffers
    cap = n + 11
    cbuf, cache = guarded((b, cap, hq, d), F8)
    dbuf, dso = guarded((b, hq // g), torch.float32)
    x8, dsr = quantize_fp8(x, g, out=cache[:, :n], descale_out=dso)
    assert x8.data_ptr() == cache.data_ptr() and dsr.data_ptr() == dso.data_ptr()
    assert same(cache.view(U8)[:, :n].cpu(), ref8) and same(dso.cpu(), refds)
    assert bool((cache.view(U8)[:, n:] == 0x7F).all())                                   # the rest of the cache
    assert untouched_around(cbuf, cache.numel()) and untouched_around(dbuf, dso.numel() * 4)
    # static mode writes descale_out when given one
    dbuf2, dso2 = guarded((b, hq // g), torch.float32)
    sd = static_descales((hq // g,), seed=9).to(DEV)
    quantize_fp8(x, g, sd, descale_out=dso2)
    assert same(dso2.cpu(), sd.cpu().expand(b, hq // g)) and untouched_around(dbuf2, dso2.numel() * 4)


@pytest.mark.parametrize("lens", [(0, 1, 300), (129, 0, 64)], ids=str)
def test_packed_sequences_equal_the_padded_call_on_each(lens):
    from common.attention_ex import quantize_fp8

    h, g, d, dtype = 4, 2, 64, F16
    slack = 7                                                                              # tokens behind the last sequence: no one's
    total = sum(lens) + slack
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)
    x = make_x("normal", (1, total, h, d), g, dtype, seed=600 + lens[0])[0]               # (total, H, d)
    xd = x.to(DEV)
    cos, sin = tables(200, 32, dtype)
    offs = torch.tensor([3, -2, 150], dtype=torch.int32)
    for rot in (dict(), dict(rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), seqlen_offsets=offs.to(DEV))):
        buf, out = guarded((total, h, d), F8)
        x8, ds = quantize_fp8(xd, g, layout="thd", out=out, cu_seqlens=cu.to(DEV), max_seqlen=max(lens), **rot)
        got, ds = out.view(U8).cpu(), ds.cpu()
        assert ds.shape == (3, h // g)
        for bb, n in enumerate(lens):
            lo = int(cu[bb])
            one = dict(rot, seqlen_offsets=rot["seqlen_offsets"][bb:bb + 1]) if rot else {}
            alone, ads, _ = quantise(xd[lo:lo + n].unsqueeze(0), g, **one)
            assert same(got[lo:lo + n], alone[0]) and same(ds[bb:bb + 1], ads)
            xs = x[lo:lo + n].unsqueeze(0)
            if rot:
                xs = rotate32(xs, cos, sin, [int(offs[bb])], False)
            want, wds = quantize_model(xs, g)
            assert same(alone, want) and same(ads, wds)
            if n == 0:
                assert bool((ads == 1).all())                                              # an empty sequence writes descale 1
        assert bool((got[sum(lens):] == 0x7F).all()) and untouched_around(buf, out.numel())


def test_untrusted_offsets_write_nothing_they_do_not_own():
    from common.attention_ex import quantize_fp8

    h, g, d, total, mx = 2, 1, 32, 40, 12
    x = make_x("normal", (1, total, h, d), g, BF16, seed=77)[0]
    xd = x.to(DEV)
    # decreasing, oversized and negative offsets; the spans the clamp gives them do not overlap (overlapping owners would race)
    for cu_list, spans in (([0, 30, 12, 25], [(0, 12), (30, 0), (12, 12)]), ([-5, 100, 2 ** 31 - 1, 7], [(0, 12), (40, 0), (40, 0)]),
                           ([39, 40, 41, 0], [(39, 1), (40, 0), (40, 0)])):
        assert [span(cu_list, bb, total, mx) for bb in range(3)] == spans
        cu = torch.tensor(cu_list, dtype=torch.int32)
        buf, out = guarded((total, h, d), F8)
        _, ds = quantize_fp8(xd, g, layout="thd", out=out, cu_seqlens=cu.to(DEV), max_seqlen=mx)
        got, ds = out.view(U8).cpu(), ds.cpu()
        owned = torch.zeros(total, dtype=torch.bool)
        for bb, (lo, n) in enumerate(spans):
            owned[lo:lo + n] = True
            codes, wds = quantize_model(x[lo:lo + n].unsqueeze(0), g)
            assert same(ds[bb:bb + 1], wds) and same(got[lo:lo + n], codes[0])
        assert bool((got[~owned] == 0x7F).all()) and untouched_around(buf, out.numel())


# ---- 6. graph capture

def test_graph_replay_follows_changed_inputs():
    """One captured dynamic two-pass call (memset, amax, quantise) and one static call with rotary, packed; x, the static descale,
    cu_seqlens and the offsets change in place between replays."""
    from common.attention_ex import quantize_fp8

    h, g, d, total, mx, dtype = 4, 2, 128, 400, 300, BF16
    cos, sin = tables(64, 64, dtype)
    cd, sd_ = cos.to(DEV), sin.to(DEV)
    x = torch.zeros((total, h, d), dtype=dtype, device=DEV)
    cu = torch.zeros(3, dtype=torch.int32, device=DEV)
    offs = torch.zeros(2, dtype=torch.int32, device=DEV)
    sdesc = torch.ones((2, h // g), dtype=torch.float32, device=DEV)
    out_d, out_s = (torch.zeros((total, h, d), dtype=U8, device=DEV).view(F8) for _ in range(2))
    ds_d = torch.zeros((2, h // g), dtype=torch.float32, device=DEV)

    def both():
        quantize_fp8(x, g, layout="thd", out=out_d, descale_out=ds_d, cu_seqlens=cu, max_seqlen=mx)
        quantize_fp8(x, g, sdesc, layout="thd", out=out_s, cu_seqlens=cu, max_seqlen=mx, rotary_cos=cd, rotary_sin=sd_,
                     seqlen_offsets=offs)

    before = routes()
    both()                                           # warm-up (module load)
    assert took(before) == (0, 1, 1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            both()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for step, (new_cu, new_offs) in enumerate((([0, 300, 400], [0, 0]), ([0, 1, 260], [60, -4]), ([10, 10, 5], [7, 7]))):
        xs = make_x(("normal", "outlier", "ties")[step], (1, total, h, d), g, dtype, seed=800 + step)[0]
        nsd = static_descales((2, h // g), seed=810 + step)
        x.copy_(xs)
        sdesc.copy_(nsd)
        cu.copy_(torch.tensor(new_cu, dtype=torch.int32))
        offs.copy_(torch.tensor(new_offs, dtype=torch.int32))
        out_d.view(U8).fill_(0x7F)
        out_s.view(U8).fill_(0x7F)
        graph.replay()
        torch.cuda.synchronize()
        gd, gs, gds = out_d.view(U8).cpu(), out_s.view(U8).cpu(), ds_d.cpu()
        owned = torch.zeros(total, dtype=torch.bool)
        for bb in range(2):
            lo, n = span(new_cu, bb, total, mx)
            owned[lo:lo + n] = True
            seq = xs[lo:lo + n].unsqueeze(0)
            want, wds = quantize_model(seq, g)
            print(f"step {step} sequence {bb}: descale {gds[bb].tolist()} model {wds[0].tolist()}, "
                  f"{int((gd[lo:lo + n] != want[0]).sum())} of {want[0].numel()} codes differ")
            assert same(gd[lo:lo + n], want[0]) and same(gds[bb:bb + 1], wds), step
            wants, _ = quantize_model(rotate32(seq, cos, sin, [new_offs[bb]], False), g, descale=nsd[bb:bb + 1])
            assert same(gs[lo:lo + n], wants[0]), step
        assert bool((gd[~owned] == 0x7F).all()) and bool((gs[~owned] == 0x7F).all())


# ---- 7. end to end

@pytest.mark.parametrize("layout", ["bhnd", "bnhd"])
def test_qkv_into_flash_attention_fp8(layout):
    from common.attention_ex import flash_attention_fp8, quantize_fp8_qkv

    b, hq, hkv, nq, nk, d, dtype = 2, 4, 2, 70, 131, 128, BF16
    gen = torch.Generator().manual_seed(900)
    q = torch.randn((b, nq, hq, d), generator=gen).to(dtype)
    k, v = (torch.randn((b, nk, hkv, d), generator=gen).to(dtype) for _ in range(2))
    cos, sin = tables(nk, 64, dtype)
    # quantize_fp8_qkv rotates q and k with ONE offset; here both start at 0 and the model does the same
    mq, mqd = quantize_model(rotate32(q, cos, sin, [0] * b, False), hq // hkv)
    mk, mkd = quantize_model(rotate32(k, cos, sin, [0] * b, False), 1)
    mv, mvd = quantize_model(v, 1)
    lay = (lambda t: t.permute(0, 2, 1, 3).contiguous()) if layout == "bhnd" else (lambda t: t)
    q8, k8, v8, qd, kd, vd = quantize_fp8_qkv(lay(q).to(DEV), lay(k).to(DEV), lay(v).to(DEV), layout=layout, rotary_cos=cos.to(DEV),
                                              rotary_sin=sin.to(DEV))
    for got, want in ((q8, mq), (k8, mk), (v8, mv)):
        assert same(got.view(U8).cpu(), lay(want))
    for got, want in ((qd, mqd), (kd, mkd), (vd, mvd)):
        assert got.shape == (b, hkv) and same(got.cpu(), want)
    o, lse = flash_attention_fp8(q8, k8, v8, q_descale=qd, k_descale=kd, v_descale=vd, causal=True, layout=layout, return_lse=True)
    dev8 = lambda t: lay(t).to(DEV).view(F8)   # noqa: E731
    ro, rlse = flash_attention_fp8(dev8(mq), dev8(mk), dev8(mv), q_descale=mqd.to(DEV), k_descale=mkd.to(DEV), v_descale=mvd.to(DEV),
                                   causal=True, layout=layout, return_lse=True)
    assert torch.equal(o.view(torch.int16), ro.view(torch.int16)) and torch.equal(lse.view(torch.int32), rlse.view(torch.int32))
    assert bool(torch.isfinite(o.float()).all())


def test_one_decode_step():
    """quantise the step's q (a fused unit: g Nq d / 8 = 32 chunks), then flash_attention_fp8_kvcache over a cache the quantiser
    filled; the bits of the same call on the CPU model's tensors"""
    from common.attention_ex import flash_attention_fp8_kvcache, quantize_fp8

    b, hq, hkv, d, cap, dtype = 2, 4, 2, 128, 96, F16
    gen = torch.Generator().manual_seed(950)
    q = torch.randn((b, 1, hq, d), generator=gen).to(dtype)
    k, v = (torch.randn((b, cap, hkv, d), generator=gen).to(dtype) for _ in range(2))
    lens = torch.tensor([cap, 37], dtype=torch.int32, device=DEV)
    kc, vc = (torch.zeros((b, cap, hkv, d), dtype=U8, device=DEV).view(F8) for _ in range(2))
    _, kd = quantize_fp8(k.to(DEV), 1, out=kc)
    _, vd = quantize_fp8(v.to(DEV), 1, out=vc)
    before = routes()
    q8, qd = quantize_fp8(q.to(DEV), hq // hkv)
    assert took(before) == (1, 0, 0)
    mq, mqd = quantize_model(q, hq // hkv)
    mk, mkd = quantize_model(k, 1)
    mv, mvd = quantize_model(v, 1)
    assert same(q8.view(U8).cpu(), mq) and same(qd.cpu(), mqd)
    assert same(kc.view(U8).cpu(), mk) and same(vc.view(U8).cpu(), mv) and same(kd.cpu(), mkd) and same(vd.cpu(), mvd)
    kw = dict(cache_seqlens=lens, causal=True, return_softmax_lse=True)
    o, lse = flash_attention_fp8_kvcache(q8, kc, vc, q_descale=qd, k_descale=kd, v_descale=vd, **kw)
    ro, rlse = flash_attention_fp8_kvcache(mq.to(DEV).view(F8), mk.to(DEV).view(F8), mv.to(DEV).view(F8), q_descale=mqd.to(DEV),
                                           k_descale=mkd.to(DEV), v_descale=mvd.to(DEV), **kw)
    assert torch.equal(o.view(torch.int16), ro.view(torch.int16)) and torch.equal(lse.view(torch.int32), rlse.view(torch.int32))
    assert bool(torch.isfinite(o.float()).all())
