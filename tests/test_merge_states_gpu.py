"""GPU: the merge of two partial attention results (fa_merge_states / fa_merge_states_backward; common/merge_states.py) against
the fp64 references of tests/merge_ref.py.

Bars.  o and dO_x: every element is one of the two neighbours, in the tensor dtype, of the exact (fp64) value computed from the same
stored inputs.  lse: rtol = atol = 1e-5 (a few tens of fp32 ulps at |lse| <~ 20).  dlse_x: rtol = atol = 1e-4 for 16-bit inputs (t
is an fp32 sum of d products of 16-bit values) and 1e-5 for fp32.  Rows with a side at -inf, whose o is NaN, come back finite and
equal to the live side bit for bit."""
import pytest
import torch

from tests import merge_ref as ref

pytestmark = pytest.mark.gpu

B, H, N = 2, 3, 37
GAPS = (0.0, 30.0, -30.0, 200.0, -200.0)
INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def _step(t, up):
    """the next representable value of t's dtype above (up) or below each element"""
    bits = t.contiguous().view(INT[t.dtype]).to(torch.int64)
    nb = 16 if t.element_size() == 2 else 32
    mag = bits & ((1 << (nb - 1)) - 1)
    key = torch.where(bits >= 0, bits, -mag) + (1 if up else -1)          # sign-magnitude -> ordered integers
    back = torch.where(key >= 0, key, -key - (1 << (nb - 1)))
    return back.to(INT[t.dtype]).view(t.dtype)


def neighbour_misses(got, exact):
    """how many elements of `got` are neither of the two values of its dtype that enclose the fp64 `exact`"""
    got = got.detach().cpu()
    near = exact.to(got.dtype)                                            # one of the two (whatever its rounding)
    other = torch.where(near.double() > exact, _step(near, False), torch.where(near.double() < exact, _step(near, True), near))
    ok = (got == near) | (got == other)
    return int((~ok).sum())


def _inputs(dtype, d, seed, special=True, b=B, h=H, n=N):
    """canonical (b, h, n, d) partial results: lse gaps of 0, +-30, +-200 by row, and (special) rows with one and with both sides
    at -inf whose dead o is NaN"""
    g = torch.Generator().manual_seed(seed)
    o_a, o_b = (torch.randn((b, h, n, d), generator=g).to(dtype) for _ in range(2))
    lse_a = 4.0 * torch.randn((b, h, n), generator=g)
    gap = torch.tensor(GAPS)[torch.arange(n) % len(GAPS)] + torch.randn((b, h, n), generator=g)
    gap[..., 0] = 0.0                                                     # equal lse, exactly
    lse_b = lse_a + gap
    if special:
        lse_a[..., 5] = ref.NEG_INF
        lse_b[..., 6] = ref.NEG_INF
        lse_a[..., 7] = lse_b[..., 7] = ref.NEG_INF
        o_a[..., 5, :] = o_b[..., 6, :] = o_a[..., 7, :] = o_b[..., 7, :] = float("nan")
    return o_a, lse_a, o_b, lse_b


def _to_layout(o, lse, layout):
    """a canonical (b, h, n, d) / (b, h, n) pair in `layout` (contiguous in that layout)"""
    if layout == "bhnd":
        return o, lse
    if layout == "bnhd":
        return o.transpose(1, 2).contiguous(), lse
    b, h, n, d = o.shape                                                  # "thd": the batch's tokens packed one after another
    return o.permute(0, 2, 1, 3).reshape(b * n, h, d).contiguous(), lse.permute(1, 0, 2).reshape(h, b * n).contiguous()


def _from_layout(o, lse, layout, b=B, h=H, n=N):
    if layout == "bhnd":
        return o, lse
    if layout == "bnhd":
        return o.transpose(1, 2), lse
    return o.reshape(b, n, h, -1).permute(0, 2, 1, 3), lse.reshape(h, b, n).permute(1, 0, 2)


def _check_forward(o, lse, o_a, lse_a, o_b, lse_b):
    """canonical GPU results against the fp64 merge of the same stored inputs"""
    o64, lse64 = ref.merge(o_a.double(), lse_a.double(), o_b.double(), lse_b.double())
    o, lse = o.detach().cpu(), lse.detach().cpu()
    assert torch.isfinite(o).all()
    misses = neighbour_misses(o, o64)
    fin = torch.isfinite(lse64)
    err = (lse[fin].double() - lse64[fin]).abs().max().item()
    print(f"o elements off the two neighbours: {misses} of {o.numel()}; max |lse - ref| = {err:.3e}")
    assert misses == 0
    assert torch.equal(torch.isfinite(lse), fin) and (lse[~fin] == ref.NEG_INF).all()
    torch.testing.assert_close(lse[fin].double(), lse64[fin], rtol=1e-5, atol=1e-5)
    return o64, lse64


CASES = [(dt, d, "bhnd") for dt in (torch.bfloat16, torch.float16, torch.float32) for d in (8, 64, 128, 256)] + \
        [(torch.float32, 40, "bhnd"), (torch.float32, 7, "bhnd")] + \
        [(dt, 128, lay) for dt in (torch.bfloat16, torch.float32) for lay in ("bnhd", "thd")] + [(torch.float16, 64, "thd"), (torch.float32, 40, "bnhd")]


@pytest.mark.parametrize("dtype,d,layout", CASES, ids=[f"{str(dt)[6:]}-d{d}-{lay}" for dt, d, lay in CASES])
def test_forward_rounding_and_backward(device, dtype, d, layout):
    from flashattention_lab_cuda import merge_states, merge_states_backward

    o_a, lse_a, o_b, lse_b = _inputs(dtype, d, seed=d)
    dev = [t.to(device) for pair in ((o_a, lse_a), (o_b, lse_b)) for t in _to_layout(*pair, layout)]
    o, lse = merge_states(*dev, layout)
    assert o.dtype == dtype and lse.dtype == torch.float32 and o.shape == dev[0].shape and lse.shape == dev[1].shape
    o_c, lse_c = _from_layout(o, lse, layout)
    _check_forward(o_c, lse_c, o_a, lse_a, o_b, lse_b)
    # a dead side (-inf) leaves the live side's bits; both dead: o = 0 (and lse = -inf, checked above)
    o_c = o_c.cpu()
    assert torch.equal(o_c[..., 5, :], o_b[..., 5, :]) and torch.equal(o_c[..., 6, :], o_a[..., 6, :])
    assert torch.equal(lse_c.cpu()[..., 5], lse_b[..., 5]) and torch.equal(lse_c.cpu()[..., 6], lse_a[..., 6])
    assert (o_c[..., 7, :] == 0).all()

    # backward, with and without dlse; NaN dlse where both sides are dead
    g = torch.Generator().manual_seed(1000 + d)
    do = torch.randn(o_a.shape, generator=g).to(dtype)
    dlse = torch.randn(lse_a.shape, generator=g)
    dlse[..., 7] = float("nan")
    do_l, dlse_l = (t.to(device) for t in _to_layout(do, dlse, layout))
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-4, atol=1e-4)
    for with_dlse in (True, False):
        got = merge_states_backward(*dev, do_l, dlse_l if with_dlse else None, layout)
        again = merge_states_backward(*dev, do_l, dlse_l if with_dlse else None, layout)
        for x, y in zip(got, again):
            assert torch.equal(x, y)                                       # deterministic
        da, la = _from_layout(got[0], got[2], layout)
        db, lb = _from_layout(got[1], got[3], layout)
        want = ref.merge_backward(o_a.double(), lse_a.double(), o_b.double(), lse_b.double(), do.double(), dlse.double() if with_dlse else None)
        for name, x in (("dO_a", da), ("dO_b", db), ("dlse_a", la), ("dlse_b", lb)):
            assert torch.isfinite(x).all(), name
        miss = neighbour_misses(da, want[0]) + neighbour_misses(db, want[1])
        err = max((la.cpu().double() - want[2]).abs().max().item(), (lb.cpu().double() - want[3]).abs().max().item())
        print(f"dlse={with_dlse}: dO elements off the two neighbours: {miss}; max |dlse_x - ref| = {err:.3e}")
        assert miss == 0
        torch.testing.assert_close(la.cpu().double(), want[2], **tol)
        torch.testing.assert_close(lb.cpu().double(), want[3], **tol)
        for t in (da[..., 5, :], la[..., 5], db[..., 6, :], lb[..., 6], da[..., 7, :], db[..., 7, :], la[..., 7], lb[..., 7]):
            assert (t == 0).all()                                          # a side with weight 0, a row with both dead


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_strided_views_and_canaries(device, dtype):
    """o_a a slice of a wider tensor, o a slice of a canary-filled one: the kernel follows the views' strides and writes nothing else"""
    from common.merge_states import merge_attention_states

    d = 64
    o_a, lse_a, o_b, lse_b = _inputs(dtype, d, seed=3)
    wide = torch.full((B, H, N, 3 * d), 7.0, dtype=dtype)
    wide[..., d: 2 * d] = o_a
    wide = wide.to(device)
    lse_wide = torch.full((B, H, 2 * N), 9.0)
    lse_wide[..., ::2] = lse_b
    lse_wide = lse_wide.to(device)
    canary = torch.full((B, H, N + 2, 2 * d), -3.0, dtype=dtype, device=device)
    lse_canary = torch.full((B, H + 1, N), -5.0, device=device)
    out = (canary[:, :, 1:-1, :d], lse_canary[:, :H])
    with torch.no_grad():
        o, lse = merge_attention_states(wide[..., d: 2 * d], lse_a.to(device), o_b.to(device), lse_wide[..., ::2], out=out)
    assert o.data_ptr() == out[0].data_ptr() and lse.data_ptr() == out[1].data_ptr()
    _check_forward(o, lse, o_a, lse_a, o_b, lse_b)
    keep = torch.full_like(canary, -3.0)
    keep[:, :, 1:-1, :d] = o
    assert torch.equal(canary.view(INT[dtype]), keep.view(INT[dtype]))     # bitwise: every canary element is untouched
    assert (lse_canary[:, H] == -5.0).all()
    assert (wide[..., :d] == 7.0).all() and (wide[..., 2 * d:] == 7.0).all() and (lse_wide[..., 1::2] == 9.0).all()


@pytest.mark.parametrize("layout", ["bhnd", "thd"])
def test_in_place_gives_the_out_of_place_bits(device, layout):
    from common.merge_states import merge_attention_states

    o_a, lse_a, o_b, lse_b = _inputs(torch.bfloat16, 128, seed=5)
    dev = [t.to(device) for pair in ((o_a, lse_a), (o_b, lse_b)) for t in _to_layout(*pair, layout)]
    o, lse = merge_attention_states(*dev, layout=layout)
    acc_o, acc_lse = dev[0].clone(), dev[1].clone()
    with torch.no_grad():
        r = merge_attention_states(acc_o, acc_lse, dev[2], dev[3], layout=layout, out=(acc_o, acc_lse))
    assert r[0] is acc_o and r[1] is acc_lse
    assert torch.equal(acc_o.view(torch.int16), o.view(torch.int16)) and torch.equal(acc_lse.view(torch.int32), lse.view(torch.int32))


def test_autograd_through_the_wrapper(device):
    """the Function hands back the kernel's gradients for all four inputs; a loss on lse alone works (no dO materialised by autograd)"""
    from common.merge_states import merge_attention_states
    from flashattention_lab_cuda import merge_states_backward

    o_a, lse_a, o_b, lse_b = (t.to(device) for t in _inputs(torch.float16, 64, seed=7, special=False))
    leaves = [t.clone().requires_grad_(True) for t in (o_a, lse_a, o_b, lse_b)]
    o, lse = merge_attention_states(*leaves)
    g, h = torch.randn_like(o), torch.randn_like(lse)
    ((o.float() * g.float()).sum() + (lse * h).sum()).backward()
    want = merge_states_backward(o_a, lse_a, o_b, lse_b, g, h)
    for leaf, w in zip(leaves, (want[0], want[2], want[1], want[3])):
        assert torch.equal(leaf.grad, w)
    leaves = [t.clone().requires_grad_(True) for t in (o_a, lse_a, o_b, lse_b)]
    (merge_attention_states(*leaves)[1] * h).sum().backward()
    want = merge_states_backward(o_a, lse_a, o_b, lse_b, torch.zeros_like(o_a), h)
    assert torch.equal(leaves[1].grad, want[2]) and torch.equal(leaves[3].grad, want[3]) and (leaves[0].grad == 0).all()


def test_graph_capture_and_replay(device):
    """forward + backward captured once; after the inputs' contents change a replay follows them"""
    from flashattention_lab_cuda import merge_states, merge_states_backward

    first = [t.to(device) for t in _inputs(torch.bfloat16, 128, seed=11)]
    do, dlse = torch.randn_like(first[0]), torch.randn_like(first[1])
    merge_states(*first)                                                   # (warm up outside the capture)
    merge_states_backward(*first, do, dlse)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            o, lse = merge_states(*first)
            grads = merge_states_backward(*first, do, dlse)
    torch.cuda.current_stream().wait_stream(side)
    second = [t.to(device) for t in _inputs(torch.bfloat16, 128, seed=12)]
    for dst, src in zip(first, second):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    o2, lse2 = merge_states(*second)
    grads2 = merge_states_backward(*second, do, dlse)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32))
    for x, y in zip(grads, grads2):
        assert torch.equal(x.view(INT[x.dtype]), y.view(INT[y.dtype]))
    _check_forward(o, lse, *[t.cpu() for t in second])
