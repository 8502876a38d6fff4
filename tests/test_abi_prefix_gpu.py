"""GPU: every entry point of a C-ABI family is the wider one with its added arguments absent.  Raw ctypes calls on one tiny problem
per family: each entry point gets the same inputs and its added arguments at their defaults (null, 0, -1 for a window bound, 1 for
kv_group / alibi_heads / sink_heads, cache_dtype = dtype), and must return the bits of the narrowest one.  The forward kernels
and the split combine use no atomics; the backward of these shapes was run twice through the narrowest entry point and gave the same
bits both times, so torch.equal is the bar there too.  The argument lists below are written out group by group, independent of
the shim's table."""
import functools

import pytest
import torch

import flashattention_lab_cuda as ext

pytestmark = pytest.mark.gpu

D, HQ, HKV, CODE = 64, 4, 2, 2   # bf16
SCALE = D ** -0.5
NOMASK = [None, 0, None, 0, 0, 0.0, 0]   # mask, mask_bh_stride, block_mask, br, bc, dropout_p, dropout_seed


def _ok(rc):
    assert rc == 0, ext._lib.fa_last_error().decode()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(gen, *shape):
    return torch.randn(shape, generator=gen).to(torch.bfloat16).cuda()


# ---- fa_ex_forward / _grouped / _window / _scoremod / _sink and the five backward ones: BH 4, Nq 40, Nk 130, causal
EX = ("", "_grouped", "_window", "_scoremod", "_sink")
BH, NQ, NK = 4, 40, 130


@functools.lru_cache(maxsize=None)
def _ex_problem():
    gen = torch.Generator().manual_seed(17)
    return _randn(gen, BH, NQ, D), _randn(gen, BH, NK, D), _randn(gen, BH, NK, D), _randn(gen, BH, NQ, D)


def _ex_args(level, ptrs, tail, backward):
    a = [t.data_ptr() for t in ptrs] + [BH]
    a += [1] if level >= 1 else []                       # kv_group
    a += [NQ, NK, D, CODE, 1]
    a += [-1, -1] if level >= 2 else []                  # window_left, window_right
    a += [SCALE]
    a += [0.0, None, 1, 0] if level >= 3 else []         # softcap, alibi_slopes, alibi_heads, alibi_batch_stride
    a += [None, 1] + ([None] if backward else []) if level >= 4 else []   # sinks, sink_heads (, dsinks)
    return a + NOMASK + tail


def _ex_forward(level):
    q, k, v, _do = _ex_problem()
    o, lse = torch.empty_like(q), torch.empty((BH, NQ), dtype=torch.float32, device=q.device)
    _ok(getattr(ext._lib, "fa_ex_forward" + EX[level])(*_ex_args(level, (q, k, v, o, lse), [_stream()], False)))
    return o, lse


def _ex_backward(level):
    q, k, v, do = _ex_problem()
    o, lse = _ex_forward(0)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    nbytes = int(ext._lib.fa_ex_backward_workspace_bytes(BH, NQ, NK, D, CODE))   # (kv_group = 1: the grouped minimum is the same)
    assert nbytes == int(ext._lib.fa_ex_backward_workspace_bytes_grouped(BH, 1, NQ, NK, D, CODE))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
    _ok(getattr(ext._lib, "fa_ex_backward" + EX[level])(
        *_ex_args(level, (q, k, v, o, do, lse, dq, dk, dv), [ws.data_ptr(), nbytes, _stream()], True)))
    return dq, dk, dv


@pytest.mark.parametrize("level", range(1, 5), ids=EX[1:])
def test_ex_forward_entry_points_agree(device, level):
    for got, want in zip(_ex_forward(level), _ex_forward(0)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("level", range(1, 5), ids=EX[1:])
def test_ex_backward_entry_points_agree(device, level):
    for got, want in zip(_ex_backward(level), _ex_backward(0)):
        assert torch.equal(got, want)


# ---- fa_ex_forward_varlen / _scoremod / _sink, the three backward ones, and _paged / _paged_fp8: two sequences of (5, 40) queries and
# (33, 130) keys, causal
VARLEN = ("", "_scoremod", "_sink")
LENS_Q, LENS_K, PAGE = (5, 40), (33, 130), 16


def _cu(lens):
    return torch.tensor([0, lens[0], lens[0] + lens[1]], dtype=torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def _varlen_problem():
    gen = torch.Generator().manual_seed(18)
    tq, tk = sum(LENS_Q), sum(LENS_K)
    return _randn(gen, tq, HQ, D), _randn(gen, tk, HKV, D), _randn(gen, tk, HKV, D), _randn(gen, tq, HQ, D), _cu(LENS_Q), _cu(LENS_K)


def _varlen_args(level, ptrs, cu_q, cu_k, total_k, k_stride, tail, backward):
    a = [t.data_ptr() for t in ptrs] + [cu_q.data_ptr(), cu_k.data_ptr(), len(LENS_Q), HQ, HKV, sum(LENS_Q), total_k, max(LENS_Q), max(LENS_K),
                                        D, CODE, HQ * D, k_stride, k_stride, 1, -1, -1, SCALE]
    a += [0.0, None, 0] if level >= 1 else []                             # softcap, alibi_slopes, alibi_batch_stride
    a += [None, 1] + ([None] if backward else []) if level >= 2 else []   # sinks, sink_heads (, dsinks)
    return a + tail


def _varlen_forward(level):
    q, k, v, _do, cu_q, cu_k = _varlen_problem()
    o, lse = torch.empty_like(q), torch.empty((HQ, q.shape[0]), dtype=torch.float32, device=q.device)
    _ok(getattr(ext._lib, "fa_ex_forward_varlen" + VARLEN[level])(
        *_varlen_args(level, (q, k, v, o, lse), cu_q, cu_k, k.shape[0], HKV * D, [0.0, 0, _stream()], False)))
    return o, lse


def _varlen_backward(level):
    q, k, v, do, cu_q, cu_k = _varlen_problem()
    o, lse = _varlen_forward(0)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    nbytes = int(ext._lib.fa_ex_backward_workspace_bytes_varlen(HQ, HKV, q.shape[0], k.shape[0], D, CODE))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
    _ok(getattr(ext._lib, "fa_ex_backward_varlen" + VARLEN[level])(
        *_varlen_args(level, (q, k, v, o, do, lse, dq, dk, dv), cu_q, cu_k, k.shape[0], HKV * D,
                      [0.0, 0, ws.data_ptr(), nbytes, _stream()], True)))
    return dq, dk, dv


@pytest.mark.parametrize("level", (1, 2), ids=VARLEN[1:])
def test_varlen_forward_entry_points_agree(device, level):
    for got, want in zip(_varlen_forward(level), _varlen_forward(0)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("level", (1, 2), ids=VARLEN[1:])
def test_varlen_backward_entry_points_agree(device, level):
    for got, want in zip(_varlen_backward(level), _varlen_backward(0)):
        assert torch.equal(got, want)


def _paged_forward(fp8_entry):
    """the same lengths over 16-token pages handed out in a shuffled order (page 0 is left unused)"""
    q, k, v, _do, cu_q, cu_k = _varlen_problem()
    pages = [(n + PAGE - 1) // PAGE for n in LENS_K]
    order = torch.randperm(sum(pages), generator=torch.Generator().manual_seed(19)) + 1
    table = torch.zeros((len(LENS_K), max(pages)), dtype=torch.int32)
    kp, vp = (torch.zeros((sum(pages) + 1, PAGE, HKV, D), dtype=torch.bfloat16, device=q.device) for _ in range(2))
    start = page = 0
    for b, n in enumerate(LENS_K):
        for j in range(pages[b]):
            rows = min(PAGE, n - j * PAGE)
            table[b, j] = order[page]
            kp[order[page], :rows] = k[start + j * PAGE:start + j * PAGE + rows]
            vp[order[page], :rows] = v[start + j * PAGE:start + j * PAGE + rows]
            page += 1
        start += n
    table = table.cuda()
    o, lse = torch.empty_like(q), torch.empty((HQ, q.shape[0]), dtype=torch.float32, device=q.device)
    tail = [table.data_ptr(), table.shape[1], kp.shape[0], PAGE, PAGE * HKV * D, PAGE * HKV * D]
    tail += [CODE, None, None, 0] if fp8_entry else []   # cache_dtype = dtype, k_descale, v_descale, descale_batch_stride
    fn = ext._lib.fa_ex_forward_varlen_paged_fp8 if fp8_entry else ext._lib.fa_ex_forward_varlen_paged
    _ok(fn(*_varlen_args(2, (q, kp, vp, o, lse), cu_q, cu_k, 0, HKV * D, tail + [_stream()], False)))
    return o, lse


def test_varlen_paged_entry_points_agree(device):
    for got, want in zip(_paged_forward(True), _paged_forward(False)):
        assert torch.equal(got, want)
        assert bool(torch.isfinite(got.float()).all())


# ---- fa_ex_forward_kvcache / _paged / _rotary / _fp8 / _sink / _varlen: B 2, Nq 3, one new token, cache_len 160, causal
KV = ("", "_paged", "_rotary", "_fp8", "_sink", "_varlen")
B, NQ_KV, NNEW, CACHE = 2, 3, 1, 160


@functools.lru_cache(maxsize=None)
def _kv_problem():
    gen = torch.Generator().manual_seed(20)
    return (_randn(gen, B, NQ_KV, HQ, D), _randn(gen, B, CACHE, HKV, D), _randn(gen, B, CACHE, HKV, D), _randn(gen, B, NNEW, HKV, D),
            _randn(gen, B, NNEW, HKV, D), torch.tensor([100, CACHE - NNEW], dtype=torch.int32).cuda())


def _kv_forward(level, num_splits):
    q, kc, vc, kn, vn, seqlens = _kv_problem()
    kc, vc = kc.clone(), vc.clone()   # the append writes to them
    o, lse = torch.empty_like(q), torch.empty((B, HQ, NQ_KV), dtype=torch.float32, device=q.device)
    if level == 5:   # each entry point with its own workspace query
        nbytes = int(ext._lib.fa_ex_kvcache_workspace_bytes_varlen(B, HQ, HKV, B * NQ_KV, NQ_KV, CACHE, D, num_splits, 0))
    else:
        query = ext._lib.fa_ex_kvcache_workspace_bytes_sink if level == 4 else ext._lib.fa_ex_kvcache_workspace_bytes
        nbytes = int(query(B, HQ, HKV, NQ_KV, CACHE, D, num_splits))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=q.device)
    a = [t.data_ptr() for t in (q, kc, vc, kn, vn, seqlens, o, lse)] + [B, HQ, HKV, NQ_KV, NNEW, CACHE, D, CODE]
    for t in (q, kc, vc, kn, vn):
        a += [t.stride(0), t.stride(1)]
    a += [1, -1, -1, SCALE, 0.0, None, 0, num_splits]
    a += [None, 0, 0, 0, 0, None, 0, None] if level >= 1 else []   # block_table ... cache_leftpad
    a += [None, None, 0, 0, 0, 0, 0] if level >= 2 else []         # rotary_cos ... rotary_interleaved
    a += [CODE, None, None, 0] if level >= 3 else []               # cache_dtype = dtype, k_descale, v_descale, descale_batch_stride
    a += [None, 1] if level >= 4 else []                           # sinks, sink_heads
    a += [None, None, 0, 0, 0] if level >= 5 else []               # cu_seqlens_q, cu_seqlens_k_new, total_q, max_seqlen_q, total_k_new
    _ok(getattr(ext._lib, "fa_ex_forward_kvcache" + KV[level])(*a, ws.data_ptr(), nbytes, _stream()))
    return o, lse, kc, vc


@pytest.mark.parametrize("num_splits", (0, 2))
@pytest.mark.parametrize("level", range(1, 6), ids=KV[1:])
def test_kvcache_entry_points_agree(device, level, num_splits):
    want = _kv_forward(0, num_splits)
    assert not torch.equal(want[2], _kv_problem()[1])   # (the new token went into the cache)
    for got, ref in zip(_kv_forward(level, num_splits), want):
        assert torch.equal(got, ref)
