"""GPU: rotary embedding for training and prefill (fa_rotary_apply, common/rotary.py) against the fp64 reference of
tests/rotary_ref.py.  Every element must be one of the two dtype neighbours of the exact value, at most 1 in 10^4 of the rotated
elements may differ from the reference's rounding (tests/test_rotary_cpu.py shows an fp32 evaluation gives 0 on these inputs),
pass-through head dims and tokens outside the tables are compared bitwise, and so is everything around the addressed views.
The decode-agreement test is bitwise: a key rotated here has the bits flash_attn_with_kvcache stores."""
import pytest
import torch

from tests.helpers import dtype_tolerances
from tests.kvcache_paged_ref import reference
from tests.rotary_ref import (BATCH, CASES, DTYPES, EXTRA_HEADS, SEQLEN_RO, case_id, case_inputs, check_rotated, reference64, round_once,
                              span, tables)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def dev(t):
    return t.to(DEV) if isinstance(t, torch.Tensor) else t


def bits(t):
    return t.contiguous().view(torch.int16)


def pattern(shape, dtype):
    """a recognisable fill for memory no call may touch"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.int32) * 37 + 11) % 251 - 125).to(dtype).view(shape)


def device_tables(r):
    """the case's tables on the device; wide ones stay slices of their wide buffer (rows at a stride above rotary_dim / 2)"""
    if r["wide_tables"]:
        wide = r["wide"].to(DEV)
        half = r["rdim"] // 2
        cos, sin = wide[0, :, :half], wide[1, :, :half]
        assert cos.stride(0) == half + 8 and not cos.is_contiguous()
        return cos, sin
    return r["cos"].to(DEV), r["sin"].to(DEV)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_parity(idx):
    import flashattention_lab_cuda as ext

    r = case_inputs(idx)
    heads, rdim = r["heads"], r["rdim"]
    cos, sin = device_tables(r)
    kw = dict(interleaved=r["inter"], conjugate=r["conj"], seqlen_offsets=dev(r["offsets"]))
    if r["strided"]:
        buf = r["buf"].to(DEV)
        x = buf[:, :, :heads]
        assert not x.is_contiguous()
    else:
        buf = x = r["x"].to(DEV)
    before = buf.clone()
    exact, rotated = reference64(r["x"], r["cos"], r["sin"], r["pos0"], r["inter"], r["conj"])
    if r["offsets"] == "vector" and r["seqlen"] == 37:
        assert not rotated[0, :3].any() and rotated[0, 3:].all() and rotated[1, :10].all() and not rotated[1, 10:].any()
    # out of place into a fresh tensor: x is only read
    out = ext.rotary_apply(x, cos, sin, **kw)
    assert out.is_contiguous() and torch.equal(bits(buf), bits(before))
    mism = check_rotated(out.cpu(), r["x"].contiguous(), exact, rotated, rdim)
    print(f"case {idx}: {mism} rotated elements differ from the fp64 rounding")
    # out of place into a strided view: the same bits, and nothing around the view changes
    obuf = pattern((BATCH, r["seqlen"], heads + EXTRA_HEADS, r["d"]), r["dtype"]).to(DEV)
    oview = obuf[:, :, :heads]
    assert ext.rotary_apply(x, cos, sin, out=oview, **kw) is oview
    assert torch.equal(bits(oview), bits(out))
    assert torch.equal(bits(obuf[:, :, heads:]), bits(pattern(obuf.shape, r["dtype"]).to(DEV)[:, :, heads:]))
    # in place: the bits of out of place; the rest of the buffer keeps its bits
    assert ext.rotary_apply(x, cos, sin, out=x, **kw) is x
    assert torch.equal(bits(x), bits(out))
    if r["strided"]:
        assert torch.equal(bits(buf[:, :, heads:]), bits(before[:, :, heads:]))


def test_positions_do_not_wrap():
    """host offset 2^31 - 1 plus device offsets near 2^31: a 32-bit sum would land inside the tables; the 64-bit one passes the
    tokens through.  Through the C entry point, which takes both offsets."""
    import flashattention_lab_cuda as ext

    b, s, h, d, rdim = 3, 4, 2, 64, 32
    g = torch.Generator().manual_seed(11)
    x = torch.randn((b, s, h, d), generator=g).to(BF16).to(DEV)
    cos, sin = (t.to(DEV) for t in tables(SEQLEN_RO, rdim, BF16))
    offs = torch.tensor([2 ** 31 - 1, -(2 ** 31) + 9, 2 ** 31 - 3], dtype=torch.int32, device=DEV)
    out = torch.full_like(x, 7.0)
    for off0 in (2 ** 31 - 1, -(2 ** 31) + 1):
        ext._call("fa_rotary_apply", (x.data_ptr(), out.data_ptr(), b, s, h, d, 2, s * h * d, h * d, s * h * d, h * d, cos.data_ptr(),
                                      sin.data_ptr(), rdim // 2, rdim // 2, SEQLEN_RO, rdim, 0, 0, off0, offs.data_ptr(), 0, 0, 0,
                                      torch.cuda.current_stream().cuda_stream))
        pos0 = [off0 + int(v) for v in offs.tolist()]            # exact integers: 2^32 - 2, 8, 2^32 - 4, then 0, -2^32 + 10, -2
        exact, rotated = reference64(x.cpu(), cos.cpu(), sin.cpu(), pos0, False, False)
        want = [[False] * 4, [True] * 4, [False] * 4] if off0 > 0 else [[True] * 4, [False] * 4, [False, False, True, True]]
        assert rotated.tolist() == want
        check_rotated(out.cpu(), x.cpu(), exact, rotated, rdim)


@pytest.mark.parametrize("nnew", [1, 3])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_decode_agreement_is_bitwise(dt, interleaved, d, nnew):
    """The contract: the rows flash_attn_with_kvcache appends with fused rotary are, bit for bit, apply_rotary_emb of k_new at
    seqlen_offsets = cache_seqlens."""
    from common.attention_ex import flash_attn_with_kvcache
    from common.rotary import apply_rotary_emb

    dtype = DTYPES[dt]
    b, cap, hq, hkv = 3, 64, 4, 2
    rdim = d if nnew == 1 else d // 2
    g = torch.Generator().manual_seed(900 + d + nnew)
    rn = lambda *shape: torch.randn(shape, generator=g).to(dtype).to(DEV)   # noqa: E731
    q, kn, vn = rn(b, nnew, hq, d), rn(b, nnew, hkv, d), rn(b, nnew, hkv, d)
    kc, vc = torch.zeros((b, cap, hkv, d), dtype=dtype, device=DEV), torch.zeros((b, cap, hkv, d), dtype=dtype, device=DEV)
    lens = [0, 17, cap - nnew]
    L = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cos, sin = (t.to(DEV) for t in tables(cap, rdim, dtype))
    flash_attn_with_kvcache(q, kc, vc, kn, vn, rotary_cos=cos, rotary_sin=sin, cache_seqlens=L, causal=True,
                            rotary_interleaved=interleaved)
    mine = apply_rotary_emb(kn, cos, sin, interleaved=interleaved, seqlen_offsets=L)
    assert not torch.equal(mine, kn)
    for bb in range(b):
        assert torch.equal(bits(kc[bb, lens[bb]:lens[bb] + nnew]), bits(mine[bb])), f"sequence {bb}"
    # and an int offset is the same position rule
    for bb in range(b):
        one = apply_rotary_emb(kn[bb:bb + 1], cos, sin, interleaved=interleaved, seqlen_offsets=lens[bb])
        assert torch.equal(bits(one[0]), bits(mine[bb]))


PACKED_LENS = (5, 0, 37, 1)


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("dt,d,rdim,heads", [("bf16", 128, 64, 3), ("f16", 96, 96, 1), ("bf16", 256, 16, 8)])
def test_packed_sequences_equal_the_padded_call_on_each(dt, d, rdim, heads, interleaved):
    import flashattention_lab_cuda as ext

    dtype = DTYPES[dt]
    spare = 4                                            # tokens behind the last sequence that no sequence owns
    total = sum(PACKED_LENS) + spare
    cu = torch.tensor([0, 5, 5, 42, 43], dtype=torch.int32, device=DEV)
    offs = torch.tensor([0, 3, 20, -1], dtype=torch.int32, device=DEV)       # sequence 2 runs past SEQLEN_RO = 50, sequence 3 is at -1
    g = torch.Generator().manual_seed(31 + d)
    buf = torch.randn((total, heads + EXTRA_HEADS, d), generator=g).to(dtype).to(DEV)
    x = buf[:, :heads]
    before = buf.clone()
    cos, sin = (t.to(DEV) for t in tables(SEQLEN_RO, rdim, dtype))
    for conj in (False, True):
        kw = dict(interleaved=interleaved, conjugate=conj)
        out = torch.full((total, heads, d), 3.0, dtype=dtype, device=DEV)
        ext.rotary_apply(x, cos, sin, out=out, seqlen_offsets=offs, cu_seqlens=cu, max_seqlen=max(PACKED_LENS), **kw)
        start = 0
        for bb, n in enumerate(PACKED_LENS):
            if n:
                alone = ext.rotary_apply(x[start:start + n].unsqueeze(0), cos, sin, seqlen_offsets=offs[bb:bb + 1], **kw)
                assert torch.equal(bits(out[start:start + n]), bits(alone[0])), (conj, bb)
            start += n
        assert (out[start:] == 3.0).all()                # unowned tokens are not written out of place
        assert torch.equal(bits(buf), bits(before))
        # sequence 2 against the reference: tokens at 20 .. 49 rotated, 50 .. 56 passed through
        xs = x[5:42].unsqueeze(0).cpu()
        exact, rotated = reference64(xs, cos.cpu(), sin.cpu(), [20], interleaved, conj)
        assert rotated[0, :30].all() and not rotated[0, 30:].any()
        check_rotated(out[5:42].unsqueeze(0).cpu(), xs.contiguous(), exact, rotated, rdim)
        # in place on the strided view: the same bits; unowned tokens and the other heads keep theirs
        work = before.clone()
        ext.rotary_apply(work[:, :heads], cos, sin, out=work[:, :heads], seqlen_offsets=offs, cu_seqlens=cu, max_seqlen=max(PACKED_LENS), **kw)
        assert torch.equal(bits(work[:start, :heads]), bits(out[:start]))
        assert torch.equal(bits(work[start:]), bits(before[start:])) and torch.equal(bits(work[:, heads:]), bits(before[:, heads:]))
    # max_seqlen below a sequence's length cuts it: the tokens past it are not owned
    out = torch.full((total, heads, d), 3.0, dtype=dtype, device=DEV)
    ext.rotary_apply(x, cos, sin, out=out, cu_seqlens=cu, max_seqlen=10)
    assert not (out[5:15] == 3.0).all() and (out[15:42] == 3.0).all()


@pytest.mark.parametrize("cu_list", [[0, 9, 4, 30, 12], [-7, 3, 1000, 2, 2 ** 31 - 1], [50, 40, 30, 20, 10], [-(2 ** 31), 2 ** 31 - 1, 0, 5, 6]],
                         ids=["decreasing", "beyond-total", "all-decreasing", "extremes"])
def test_untrusted_cu_seqlens_write_nothing_outside_y(cu_list):
    """canary rows in front of and behind x and y: whatever cu_seqlens holds, they keep their bits, tokens that the clamped spans
    do not own are not written, and owned ones are (out of place)"""
    import flashattention_lab_cuda as ext

    total, heads, d, rdim, guard, mx = 20, 3, 64, 32, 6, 8
    g = torch.Generator().manual_seed(77)
    xbuf = torch.randn((total + 2 * guard, heads, d), generator=g).to(BF16).to(DEV)
    ybuf = pattern((total + 2 * guard, heads, d), BF16).to(DEV)
    x, y = xbuf[guard:guard + total], ybuf[guard:guard + total]
    xb0, yb0 = xbuf.clone(), ybuf.clone()
    cos, sin = (t.to(DEV) for t in tables(SEQLEN_RO, rdim, BF16))
    cu = torch.tensor(cu_list, dtype=torch.int32, device=DEV)
    ext.rotary_apply(x, cos, sin, out=y, cu_seqlens=cu, max_seqlen=mx)
    torch.cuda.synchronize()
    owned = torch.zeros(total, dtype=torch.bool)
    for bb in range(len(cu_list) - 1):
        st, n = span(cu_list, bb, total, mx)
        assert 0 <= st and st + n <= total
        owned[st:st + n] = True
    assert torch.equal(bits(xbuf), bits(xb0))
    assert torch.equal(bits(ybuf[:guard]), bits(yb0[:guard])) and torch.equal(bits(ybuf[guard + total:]), bits(yb0[guard + total:]))
    yc, y0 = y.cpu(), yb0[guard:guard + total].cpu()
    assert torch.equal(bits(yc[~owned]), bits(y0[~owned]))
    if owned.any():
        assert torch.equal(bits(yc[owned][..., rdim:]), bits(x.cpu()[owned][..., rdim:]))      # written: x's pass-through dims arrived
    # in place: the canaries and the unowned tokens keep their bits
    ext.rotary_apply(x, cos, sin, out=x, cu_seqlens=cu, max_seqlen=mx)
    torch.cuda.synchronize()
    assert torch.equal(bits(xbuf[:guard]), bits(xb0[:guard])) and torch.equal(bits(xbuf[guard + total:]), bits(xb0[guard + total:]))
    assert torch.equal(bits(x.cpu()[~owned]), bits(xb0[guard:guard + total].cpu()[~owned]))


def _grad_check(got, w, cos, sin, pos0, interleaved, rdim):
    """got: the gradient (B, S, H, d) of sum(out * w) in x: the fp64 transpose of the rotation, applied to w"""
    exact, rotated = reference64(w, cos, sin, pos0, interleaved, True)
    return check_rotated(got, w, exact, rotated, rdim)


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_apply_rotary_emb_autograd(dt, interleaved):
    from common.rotary import apply_rotary_emb

    dtype = DTYPES[dt]
    b, s, h, d, rdim = 3, 37, 3, 128, 64
    g = torch.Generator().manual_seed(55)
    x0, w = (torch.randn((b, s, h, d), generator=g).to(dtype) for _ in range(2))
    cos, sin = tables(SEQLEN_RO, rdim, dtype)
    offs = torch.tensor([0, 30, -2], dtype=torch.int32)
    cd, sd, wd = cos.to(DEV), sin.to(DEV), w.to(DEV)
    # padded, a device offset vector
    x = x0.to(DEV).requires_grad_(True)
    out = apply_rotary_emb(x, cd, sd, interleaved=interleaved, seqlen_offsets=offs.to(DEV))
    exact, rotated = reference64(x0, cos, sin, offs.tolist(), interleaved, False)
    check_rotated(out.detach().cpu(), x0, exact, rotated, rdim)
    w_before = wd.clone()
    (dx,) = torch.autograd.grad(out, x, wd)
    assert torch.equal(bits(wd), bits(w_before))                              # the incoming gradient is only read
    _grad_check(dx.cpu(), w, cos, sin, offs.tolist(), interleaved, rdim)
    # through a sum: the incoming gradient is an expanded tensor the kernel cannot address as it is
    x = x0.to(DEV).requires_grad_(True)
    apply_rotary_emb(x, cd, sd, interleaved=interleaved, seqlen_offsets=5).float().sum().backward()
    ones = torch.ones_like(x0)
    _grad_check(x.grad.cpu(), ones, cos, sin, [5] * b, interleaved, rdim)
    # inplace=True on a non-leaf: the same bits, the version counter moves, and the gradient flows through
    x = x0.to(DEV).requires_grad_(True)
    y = x * 1
    version = y._version
    z = apply_rotary_emb(y, cd, sd, interleaved=interleaved, inplace=True, seqlen_offsets=offs.to(DEV))
    assert z is y and y._version > version
    assert torch.equal(bits(z.detach()), bits(out.detach()))
    (dx2,) = torch.autograd.grad(z, x, wd)
    assert torch.equal(bits(dx2), bits(dx))
    # packed
    cu = torch.tensor([0, 37, 37, 111], dtype=torch.int32, device=DEV)       # 37, 0 and 74 tokens; max_seqlen cuts the last to 60
    xp = x0.reshape(b * s, h, d).to(DEV).requires_grad_(True)
    outp = apply_rotary_emb(xp, cd, sd, interleaved=interleaved, seqlen_offsets=offs.to(DEV), cu_seqlens=cu, max_seqlen=60)
    wp = w.reshape(b * s, h, d)
    (dxp,) = torch.autograd.grad(outp, xp, wp.to(DEV))
    dxp = dxp.cpu()
    _grad_check(dxp[:37].unsqueeze(0), wp[:37].unsqueeze(0), cos, sin, [0], interleaved, rdim)
    _grad_check(dxp[37:97].unsqueeze(0), wp[37:97].unsqueeze(0), cos, sin, [-2], interleaved, rdim)
    # tokens no sequence owns: the forward leaves the fresh output unwritten there, and so does the backward; nothing to compare


@pytest.mark.parametrize("layout", ["qkv5", "gqa4", "qkv4-packed", "gqa3-packed"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
def test_apply_rotary_emb_qkv_autograd(layout, interleaved):
    from common.rotary import apply_rotary_emb_qkv_

    dtype, b, s, d, rdim = BF16, 3, 5, 64, 32
    hq, hkv = (3, 3) if layout.startswith("qkv") else (8, 1)
    packed = layout.endswith("packed")
    g = torch.Generator().manual_seed(66)
    lead = (b * s,) if packed else (b, s)
    shape = lead + ((3, hq, d) if layout.startswith("qkv") else (hq + 2 * hkv, d))
    q0, w = (torch.randn(shape, generator=g).to(dtype) for _ in range(2))
    cos, sin = tables(SEQLEN_RO, rdim, dtype)
    offs = torch.tensor([0, 47, -2], dtype=torch.int32)
    kw = dict(interleaved=interleaved, seqlen_offsets=offs.to(DEV))
    if packed:
        kw.update(cu_seqlens=torch.arange(0, b * s + 1, s, dtype=torch.int32, device=DEV), max_seqlen=s)
    if not layout.startswith("qkv"):
        kw.update(num_heads_q=hq)
    leaf = q0.to(DEV).requires_grad_(True)
    qkv = leaf * 1
    version = qkv._version
    ret = apply_rotary_emb_qkv_(qkv, cos.to(DEV), sin.to(DEV), **kw)
    assert ret is qkv and qkv._version > version
    wd = w.to(DEV)
    w_before = wd.clone()
    (dleaf,) = torch.autograd.grad(ret, leaf, wd)
    assert torch.equal(bits(wd), bits(w_before))                              # never modified in place
    nqk = hq + hkv
    as_heads = lambda t: t.cpu().reshape(b, s, -1, d)     # noqa: E731  ((B, S, all heads, d): q heads, k heads, v heads)
    got, x0, gw, gr = as_heads(ret.detach()), as_heads(q0), as_heads(w), as_heads(dleaf)
    exact, rotated = reference64(x0[:, :, :nqk], cos, sin, offs.tolist(), interleaved, False)
    assert rotated[0].all() and rotated[1, :3].all() and not rotated[1, 3:].any() and not rotated[2, :2].any()
    check_rotated(got[:, :, :nqk].contiguous(), x0[:, :, :nqk].contiguous(), exact, rotated, rdim)
    assert torch.equal(bits(got[:, :, nqk:]), bits(x0[:, :, nqk:]))           # v: untouched
    _grad_check(gr[:, :, :nqk].contiguous(), gw[:, :, :nqk].contiguous(), cos, sin, offs.tolist(), interleaved, rdim)
    assert torch.equal(bits(gr[:, :, nqk:]), bits(gw[:, :, nqk:]))            # v's gradient: the incoming bits


def test_graph_replay_follows_changed_offsets():
    """One captured call with device offsets, one stream, a linear graph; the offsets (and cu_seqlens) change between replays."""
    import flashattention_lab_cuda as ext

    b, s, h, d, rdim = 3, 5, 3, 128, 64
    g = torch.Generator().manual_seed(88)
    x0 = torch.randn((b * s, h, d), generator=g).to(BF16)
    cos, sin = tables(SEQLEN_RO, rdim, BF16)
    x, cd, sd = x0.to(DEV), cos.to(DEV), sin.to(DEV)
    offs = torch.zeros(b, dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 5, 10, 15], dtype=torch.int32, device=DEV)
    out = torch.zeros_like(x)
    kw = dict(out=out, interleaved=False, seqlen_offsets=offs, cu_seqlens=cu, max_seqlen=s)
    ext.rotary_apply(x, cd, sd, **kw)                    # warm-up (module load)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            ext.rotary_apply(x, cd, sd, **kw)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for new_offs, new_cu in (([0, 0, 0], [0, 5, 10, 15]), ([7, 45, -1], [0, 5, 10, 15]), ([2, 9, 30], [0, 3, 8, 12])):
        offs.copy_(torch.tensor(new_offs, dtype=torch.int32))
        cu.copy_(torch.tensor(new_cu, dtype=torch.int32))
        out.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu()
        owned = torch.zeros(b * s, dtype=torch.bool)
        for bb in range(b):
            lo, n = span(new_cu, bb, b * s, s)
            owned[lo:lo + n] = True
            xs = x0[lo:lo + n].unsqueeze(0)
            exact, rotated = reference64(xs, cos, sin, [new_offs[bb]], False, False)
            check_rotated(got[lo:lo + n].unsqueeze(0), xs, exact, rotated, rdim)
        assert (got[~owned] == 3.0).all()
        eager = ext.rotary_apply(x, cd, sd, out=torch.full_like(x, 3.0), interleaved=False, seqlen_offsets=offs, cu_seqlens=cu, max_seqlen=s)
        assert torch.equal(bits(eager), bits(out))


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
def test_prefill_then_decode_end_to_end(interleaved):
    """Prefill two sequences through apply_rotary_emb_qkv_ and flash_attention_varlen(causal=True), copy the rotated K and V into a
    cache, run one decode step through flash_attn_with_kvcache with fused rotary; o against the fp64 attention over
    fp64-rotated, once-rounded q and k."""
    from common.attention_ex import flash_attention_varlen, flash_attn_with_kvcache
    from common.rotary import apply_rotary_emb_qkv_

    dtype, h, d, rdim, cap = BF16, 4, 64, 32, 64
    lens = [19, 33]
    b, total = len(lens), sum(lens)
    g = torch.Generator().manual_seed(99)
    qkv0 = torch.randn((total, 3, h, d), generator=g).to(dtype)
    q1, k1, v1 = (torch.randn((b, 1, h, d), generator=g).to(dtype) for _ in range(3))
    cos, sin = tables(cap, rdim, dtype)
    cd, sd = cos.to(DEV), sin.to(DEV)
    cu = torch.tensor([0, lens[0], total], dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    qkv = apply_rotary_emb_qkv_(qkv0.to(DEV), cd, sd, interleaved=interleaved, cu_seqlens=cu, max_seqlen=max(lens))
    q, k, v = qkv.unbind(1)
    o = flash_attention_varlen(q, k, v, cu, cu, max(lens), max(lens), causal=True)
    kc, vc = torch.zeros((b, cap, h, d), dtype=dtype, device=DEV), torch.zeros((b, cap, h, d), dtype=dtype, device=DEV)
    start = 0
    for bb, n in enumerate(lens):
        kc[bb, :n], vc[bb, :n] = k[start:start + n], v[start:start + n]
        start += n
    L = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o1, lse1 = flash_attn_with_kvcache(q1.to(DEV), kc, vc, k1.to(DEV), v1.to(DEV), rotary_cos=cd, rotary_sin=sd, cache_seqlens=L,
                                       causal=True, rotary_interleaved=interleaved, return_softmax_lse=True)
    # the reference
    rot = lambda x, pos: round_once(reference64(x.unsqueeze(0), cos, sin, [pos], interleaved, False)[0][0], dtype)   # noqa: E731
    start = 0
    ks, vs, qn = [], [], []
    for bb, n in enumerate(lens):
        qr, kr, vv = rot(qkv0[start:start + n, 0], 0), rot(qkv0[start:start + n, 1], 0), qkv0[start:start + n, 2]
        ro, _ = reference(qr.unsqueeze(0), [kr], [vv], True, (-1, -1), scale)
        torch.testing.assert_close(o[start:start + n].double().cpu(), ro[0], **dtype_tolerances(dtype))
        ks.append(torch.cat([kr, rot(k1[bb], n)]))
        vs.append(torch.cat([vv, v1[bb]]))
        qn.append(rot(q1[bb], n))
        start += n
    ro1, rlse1 = reference(torch.stack(qn), ks, vs, True, (-1, -1), scale)
    assert not torch.isnan(o1).any()
    torch.testing.assert_close(o1.double().cpu(), ro1, **dtype_tolerances(dtype))
    torch.testing.assert_close(lse1.double().cpu(), rlse1, rtol=1e-3, atol=1e-3)
    # one cache, one rounding: the prefilled rows and the appended row are what a decode-only fill would have stored
    for bb, n in enumerate(lens):
        assert torch.equal(bits(kc[bb, :n + 1].cpu()), bits(ks[bb])) or \
            int((kc[bb, :n + 1].cpu().double() != ks[bb].double()).sum()) * 10 ** 4 <= (n + 1) * h * rdim
