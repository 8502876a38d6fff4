"""GPU: packed queries and new keys on the fp8 decode call and the fp8 decode step, and the step at head dims 64 / 256
(csrc/fa_fp8_decode.hip: fp8kv_split_mod_kernel's packed instantiation; csrc/fa_fp8_step.hip: fp8kv_step_prep_varlen_kernel;
common/fp8_attention.py: fp8_attn_with_kvcache_varlen, fp8_attn_kvcache_step).  The padded fp8 decode call, already
held to the sharp fp64 bar, is the definition of every per-sequence result, so the bar here is torch.equal.  One problem serves
most tests (tests/fp8_step_varlen_ref.PROBLEM): B = 5, nq = [1, 0, 5, 20, 3], lengths [300, 17, 0, 64, 129], nnew = [1, 0, 5, 2, 3],
capacity 384, H_kv = 2 with G = 4 (nq = 20 spans three 32-row tiles, every other sequence's later tiles leave empty) or G = 1."""
import functools

import pytest
import torch

from tests import fp8_step_varlen_ref as vr
from tests.kvcache_fp8_ref import quantize
from tests.test_abi_signatures_cpu import PROTOTYPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
WIDTHS = vr.HEAD_DIMS
LAYOUTS = ("contig", "bidx", "ps16", "ps48")
CANARY = 0x5A
DECODE_FN, STEP_FN = "fa_fp8_forward_kvcache_varlen", "fa_fp8_kvcache_step_varlen"
# the bare call, causal, and the composite: window (20, -1) + softcap 30 + sinks (one at -inf, one at 1e4)
MODS = {"bare": dict(causal=False, window_size=(-1, -1), softcap=0.0, sinks=False),
        "causal": dict(causal=True, window_size=(-1, -1), softcap=0.0, sinks=False),
        "composite": dict(causal=False, window_size=(20, -1), softcap=30.0, sinks=True)}


def _dev(t):
    return None if t is None else t.to(DEV)


def the_sinks(hq):
    s = 2.0 * torch.randn((hq,), generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    s[1], s[2 if hq > 2 else 0] = float("-inf"), 1e4
    return s


def mod_kw(name, hq):
    m = dict(MODS[name])
    m["sinks"] = the_sinks(hq).to(DEV) if m["sinks"] else None
    return m


@functools.lru_cache(maxsize=None)
def problem(d, g, layout, rot=None, e4=False, packed_kn=True, dtype=torch.bfloat16):
    return vr.problem(d, g, layout, dtype=dtype, rot=rot, e4=e4, packed_kn=packed_kn)


def cu_t(cu):
    return None if cu is None else torch.tensor(cu, dtype=torch.int32, device=DEV)


def codes(call):
    """e4m3 codes of the problem's packed q under its q descales (any codes do for the decode tests)"""
    total_q, hq, d = call["q"].shape
    if call["q"].dtype == torch.uint8:
        return call["q"]
    return quantize(call["q"].view(1, total_q, hq, d), torch.full((1, hq), 2.0 ** -5))[0]


def cache_kw(call, b=None):
    """the cache-side keywords of the wrappers, of the whole batch or of sequence b alone (its length before the append, its table
    row, its cache_batch_idx entry, its descale rows; a contiguous cache without indices: its row)"""
    sl = slice(None) if b is None else slice(b, b + 1)
    kw = dict(cache_seqlens=_dev(call["cache_seqlens"][sl]), q_descale=_dev(call["q_descale"][sl]), k_descale=_dev(call["k_descale"][sl]),
              v_descale=_dev(call["v_descale"][sl]), softmax_scale=call["scale"], return_softmax_lse=True)
    if call["block_table"] is not None:
        kw["block_table"] = _dev(call["block_table"][sl])
    if call["cache_batch_idx"] is not None:
        kw["cache_batch_idx"] = _dev(call["cache_batch_idx"][sl])
    return kw


def cache_rows(call, kc, vc, b):
    """the caches the padded call on sequence b alone takes"""
    if call["block_table"] is None and call["cache_batch_idx"] is None:
        return kc[b:b + 1], vc[b:b + 1]
    return kc, vc


def per_sequence(call, q8, kc, vc, ranges, lens, num_splits, mod, out_dtype=torch.bfloat16):
    """[(tok0, nq, o (nq, H_q, d), lse (H_q, nq))] of the padded call on every sequence with nq > 0 alone"""
    from common.fp8_attention import fp8_attn_with_kvcache

    out = []
    for b, (tok0, nq) in enumerate(ranges):
        if nq == 0:
            continue
        kw = cache_kw(call, b)
        kw["cache_seqlens"] = lens[b:b + 1]
        kb, vb = cache_rows(call, kc, vc, b)
        o, lse = fp8_attn_with_kvcache(q8[tok0:tok0 + nq][None].view(E4), kb.view(E4), vb.view(E4), num_splits=num_splits, out_dtype=out_dtype,
                                       **kw, **mod)
        out.append((tok0, nq, o[0], lse[0]))
    return out


def check_rows(o, lse, want):
    for tok0, nq, ob, lb in want:
        assert torch.equal(o[tok0:tok0 + nq], ob), (tok0, nq)
        assert torch.equal(lse[:, tok0:tok0 + nq], lb), (tok0, nq)


def run_decode(call, q8, kc, vc, lens, num_splits, mod, cu=None, max_q=None, out_dtype=torch.bfloat16):
    from common.fp8_attention import fp8_attn_with_kvcache_varlen

    kw = cache_kw(call)
    kw["cache_seqlens"] = lens
    return fp8_attn_with_kvcache_varlen(q8.view(E4), kc.view(E4), vc.view(E4), cu_seqlens_q=cu_t(call["cu_q"] if cu is None else cu),
                                        max_seqlen_q=call["max_seqlen_q"] if max_q is None else max_q, num_splits=num_splits,
                                        out_dtype=out_dtype, **kw, **mod)


def q_ranges(call, cu=None):
    cu = call["cu_q"] if cu is None else cu
    return [vr.cu_range(cu, b, call["q"].shape[0], call["max_seqlen_q"]) for b in range(call["B"])]


# ---- 1. packed decode equals the padded call bit for bit

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", WIDTHS)
def test_packed_decode_is_the_padded_call_on_every_sequence(d, layout):
    call = problem(d, 4, layout)
    q8, kc, vc, lens = _dev(codes(call)), _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
    for name in MODS:
        mod = mod_kw(name, call["hq"])
        for ns in (1, 4):
            o, lse = run_decode(call, q8, kc, vc, lens, ns, mod)
            assert o.shape == (29, call["hq"], d) and lse.shape == (call["hq"], 29) and o.dtype == torch.bfloat16
            check_rows(o, lse, per_sequence(call, q8, kc, vc, q_ranges(call), lens, ns, mod))
            if name == "composite":         # the sequence without a key: o = 0, lse = the sink of the row's head
                assert bool((o[1:6] == 0).all()) and torch.equal(lse[:, 1:6], mod["sinks"][:, None].expand(-1, 5))


@pytest.mark.parametrize("layout", ("contig", "ps48"))
@pytest.mark.parametrize("d", WIDTHS)
def test_packed_decode_with_one_head_a_group_f16_out_and_the_split_rule(d, layout):
    call = problem(d, 1, layout)
    q8, kc, vc, lens = _dev(codes(call)), _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
    for name, ns, dt in (("causal", 1, torch.bfloat16), ("composite", 4, torch.float16)):
        mod = mod_kw(name, call["hq"])
        o, lse = run_decode(call, q8, kc, vc, lens, ns, mod, out_dtype=dt)
        assert o.dtype == dt
        check_rows(o, lse, per_sequence(call, q8, kc, vc, q_ranges(call), lens, ns, mod, out_dtype=dt))
    # num_splits = 0: the rule over ceil(max_seqlen_q * G / 32) = 1 row tile, 5 * 2 units: min(ceil(4096 / 10), ceil(384 / 128)) = 3
    # splits, whatever the head dim; the padded call with that many gives the same bits
    import flashattention_lab_cuda as ext

    mod = mod_kw("causal", call["hq"])
    assert ext._lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(5, call["hq"], 2, 29, 20, 384, d, 0, 1, -1, -1, 0) == \
        ext._lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(5, call["hq"], 2, 29, 20, 384, d, 3, 1, -1, -1, 0) > 0
    o, lse = run_decode(call, q8, kc, vc, lens, 0, mod)
    check_rows(o, lse, per_sequence(call, q8, kc, vc, q_ranges(call), lens, 3, mod))


# ---- raw calls by the header's parameter names

def raw(name, **a):
    import flashattention_lab_cuda as ext

    names = PROTOTYPES[name][2]
    assert set(names) == set(a), set(names) ^ set(a)
    rc = getattr(ext._lib, name)(*[a[n] for n in names])
    assert rc == 0, ext._lib.fa_last_error().decode()


def ptr(t):
    return None if t is None else t.data_ptr()


def decode_args(call, q8, kc, vc, o, lse, lens, ws, ws_bytes, num_splits, mod, keep):
    """fa_fp8_forward_kvcache_hdim's arguments of the problem on the device tensors given (keep: what must outlive the call)"""
    hq, hkv, d = call["hq"], call["hkv"], kc.shape[-1]
    table, bidx = _dev(call["block_table"]), _dev(call["cache_batch_idx"])
    qd, kd, vd = (_dev(call[n]) for n in ("q_descale", "k_descale", "v_descale"))
    keep += [table, bidx, qd, kd, vd]
    wl, wr = mod["window_size"]
    return dict(q=ptr(q8), k_cache=ptr(kc), v_cache=ptr(vc), o=ptr(o), lse=ptr(lse), q_descale=ptr(qd), k_descale=ptr(kd), v_descale=ptr(vd),
                cache_seqlens=ptr(lens), block_table=ptr(table), cache_batch_idx=ptr(bidx), batch=call["B"], heads_q=hq, heads_kv=hkv,
                seqlen_q=0, cache_len=vr.capacity(call), cache_batch=kc.shape[0] if bidx is not None else 0, head_dim=d, dtype=2, q_dtype=3,
                cache_dtype=3, q_batch_stride=0, q_token_stride=hq * d, k_batch_stride=kc.stride(0), k_token_stride=kc.stride(1),
                v_batch_stride=vc.stride(0), v_token_stride=vc.stride(1), block_table_row_stride=table.stride(0) if table is not None else 0,
                num_blocks=kc.shape[0] if table is not None else 0, page_block_size=kc.shape[1] if table is not None else 0,
                q_descale_batch_stride=hkv, k_descale_batch_stride=hkv, v_descale_batch_stride=hkv, causal=int(mod["causal"]),
                softmax_scale=call["scale"], num_splits=num_splits, workspace=ptr(ws), workspace_bytes=ws_bytes,
                stream=torch.cuda.current_stream().cuda_stream, window_left=wl, window_right=wr, softcap=mod["softcap"],
                sinks=ptr(mod["sinks"]), sink_heads=hq if mod["sinks"] is not None else 0)


def guarded(shape, dtype, margin=4096):
    """(the tensor cut out of a canary-filled buffer, the buffer): `margin` bytes of guard on both sides"""
    n = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * margin,), CANARY, dtype=torch.uint8, device=DEV)
    return buf[margin:margin + n].view(dtype).view(shape), buf


def guards_intact(buf, margin=4096):
    return bool((buf[:margin] == CANARY).all()) and bool((buf[-margin:] == CANARY).all())


# ---- 2. a null packed group is the parent call

@pytest.mark.parametrize("d,name", [(64, "bare"), (128, "bare"), (128, "composite"), (256, "causal")])
def test_a_null_packed_group_is_the_hdim_call(d, name):
    import flashattention_lab_cuda as ext

    call = problem(d, 4, "ps16")
    nq, hq = 3, call["hq"]
    mod = mod_kw(name, hq)
    q8 = _dev(codes(call))[:5 * nq].reshape(5, nq, hq, d).contiguous()
    kc, vc, lens = _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
    need = int(ext._lib.fa_fp8_forward_kvcache_hdim_workspace_bytes(5, hq, 2, nq, 384, d, 4, int(mod["causal"]), *mod["window_size"],
                                                                    int(mod["sinks"] is not None)))
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    routes = ("fp8kv_split_mod", "fp8kv_split_hdim", "fp8kv_split_varlen", "fp8kv_step_prep", "fp8kv_step_prep_varlen")
    got, counts = [], []
    for fn, extra in (("fa_fp8_forward_kvcache_hdim", {}), (DECODE_FN, dict(cu_seqlens_q=None, total_q=0, max_seqlen_q=0))):
        o = torch.zeros((5, nq, hq, d), dtype=torch.bfloat16, device=DEV)
        lse = torch.zeros((5, hq, nq), dtype=torch.float32, device=DEV)
        keep = []
        a = decode_args(call, q8, kc, vc, o, lse, lens, ws, need, 4, mod, keep)
        a.update(seqlen_q=nq, q_batch_stride=nq * hq * d, **extra)
        before = [ext.route_count(r) for r in routes]
        raw(fn, **a)
        torch.cuda.synchronize()
        counts.append([ext.route_count(r) - x for r, x in zip(routes, before)])
        got.append((o.cpu(), lse.cpu()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and bool(got[0][0].any())
    assert counts[0] == counts[1] and sum(counts[0]) == (0 if (d, name) == (128, "bare") else 1) and counts[0][2:] == [0, 0, 0]


def step_args(call, q, kc, vc, o, lse, lens, ws, num_splits, mod, k_new, v_new, q8_out, cos, sin, keep):
    a = decode_args(call, q, kc, vc, o, lse, lens, ws, ws.numel(), num_splits, mod, keep)
    esz = q.element_size()
    code = 3 if q.dtype == torch.uint8 else {torch.float16: 1, torch.bfloat16: 2}[q.dtype]
    a.update(q_dtype=code, q_token_stride=a["q_token_stride"] * esz, k_new=ptr(k_new), v_new=ptr(v_new), seqlen_new=0, k_new_batch_stride=0,
             k_new_token_stride=k_new.stride(-3) * esz, v_new_batch_stride=0, v_new_token_stride=v_new.stride(-3) * esz, in_dtype=code,
             q8_out=ptr(q8_out), q8_batch_stride=0, q8_token_stride=q8_out.stride(-3) if q8_out is not None else 0, rotary_cos=ptr(cos),
             rotary_sin=ptr(sin), rotary_cos_row_stride=cos.stride(0) if cos is not None else 0,
             rotary_sin_row_stride=sin.stride(0) if sin is not None else 0, seqlen_ro=cos.shape[0] if cos is not None else 0,
             rotary_dim=2 * cos.shape[1] if cos is not None else 0, rotary_interleaved=int(call["rotary_interleaved"]))
    return a


def test_a_null_packed_group_at_128_is_the_padded_step():
    import flashattention_lab_cuda as ext

    call = problem(128, 4, "ps16", rot=(True, 32))
    nq, nnew, hq, d = 2, 2, call["hq"], 128
    mod = mod_kw("composite", hq)
    q = _dev(call["q"])[:5 * nq].reshape(5, nq, hq, d).contiguous()
    kn, vn = _dev(call["k_new"])[:5 * nnew].reshape(5, nnew, 2, d).contiguous(), _dev(call["v_new"])[:5 * nnew].reshape(5, nnew, 2, d).contiguous()
    cos, sin, lens = _dev(call["rotary_cos"]), _dev(call["rotary_sin"]), _dev(call["cache_seqlens"])
    need = int(ext._lib.fa_fp8_kvcache_step_workspace_bytes(5, hq, 2, nq, 384, 128, 4, 0, 20, -1, 1, 2, 1))
    assert need == int(ext._lib.fa_fp8_kvcache_step_varlen_workspace_bytes(5, hq, 2, nq, 384, 128, 4, 0, 20, -1, 1, 2, 1, 0, 0))
    routes = ("fp8kv_step_prep", "fp8kv_split_mod", "fp8kv_step_prep_varlen", "fp8kv_split_varlen")
    got, counts = [], []
    for fn, extra in (("fa_fp8_kvcache_step", {}), (STEP_FN, dict(cu_seqlens_q=None, total_q=0, max_seqlen_q=0, cu_seqlens_k_new=None,
                                                                  total_k_new=0))):
        kc, vc = _dev(call["k_cache"]), _dev(call["v_cache"])
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
        o = torch.zeros((5, nq, hq, d), dtype=torch.bfloat16, device=DEV)
        lse = torch.zeros((5, hq, nq), dtype=torch.float32, device=DEV)
        q8 = torch.zeros((5, nq, hq, d), dtype=torch.uint8, device=DEV)
        keep = []
        a = step_args(call, q, kc, vc, o, lse, lens, ws, 4, mod, kn, vn, q8, cos, sin, keep)
        a.update(seqlen_q=nq, q_batch_stride=q.stride(0) * 2, seqlen_new=nnew, k_new_batch_stride=kn.stride(0) * 2,
                 v_new_batch_stride=vn.stride(0) * 2, q8_batch_stride=q8.stride(0), **extra)
        if fn == "fa_fp8_kvcache_step":
            a["d"] = a.pop("head_dim")
        before = [ext.route_count(r) for r in routes]
        raw(fn, **a)
        torch.cuda.synchronize()
        counts.append([ext.route_count(r) - x for r, x in zip(routes, before)])
        got.append([t.cpu() for t in (kc, vc, q8, o, lse)])
    for x, y in zip(*got):
        assert torch.equal(x, y)
    assert bool(got[0][2].any()) and not torch.equal(got[0][0], call["k_cache"])
    assert counts[0] == counts[1] == [1, 1, 0, 0]


# ---- 3 - 5. the step: cache bytes, q codes, attention

_RUNS = {}


def ran(d, layout, rot, g=4):
    """the packed step of the problem on the GPU, once: with q8_out on caches A; the 16-bit call's e4m3 append on caches B; the packed
    decode call on the step's codes, caches A and len_b"""
    key = (d, layout, rot, g)
    if key in _RUNS:
        return _RUNS[key]
    from common.attention_ex import flash_attn_with_kvcache
    from common.fp8_attention import fp8_attn_kvcache_step, fp8_attn_with_kvcache_varlen

    call = problem(d, g, layout, rot=rot)
    mod = mod_kw("causal", call["hq"])
    ka, va, kb, vb = (_dev(call[n]) for n in ("k_cache", "v_cache", "k_cache", "v_cache"))
    q8 = torch.full(tuple(call["q"].shape), 0x7F, dtype=torch.uint8, device=DEV)
    kw = cache_kw(call)
    rkw = dict(rotary_cos=_dev(call["rotary_cos"]), rotary_sin=_dev(call["rotary_sin"]), rotary_interleaved=call["rotary_interleaved"])
    pk = dict(cu_seqlens_q=cu_t(call["cu_q"]), max_seqlen_q=call["max_seqlen_q"], cu_seqlens_k_new=cu_t(call["cu_kn"]))
    o, lse = fp8_attn_kvcache_step(_dev(call["q"]), ka.view(E4), va.view(E4), _dev(call["k_new"]), _dev(call["v_new"]), num_splits=4,
                                   q8_out=q8.view(E4), **kw, **rkw, **pk, **mod)
    ka2, va2 = _dev(call["k_cache"]), _dev(call["v_cache"])
    o_ws, _lse = fp8_attn_kvcache_step(_dev(call["q"]), ka2.view(E4), va2.view(E4), _dev(call["k_new"]), _dev(call["v_new"]), num_splits=4,
                                       **kw, **rkw, **pk, **mod)                      # the codes in the workspace
    kw16 = {n: v for n, v in kw.items() if n not in ("q_descale", "return_softmax_lse")}
    flash_attn_with_kvcache(_dev(call["q"]), kb.view(E4), vb.view(E4), k=_dev(call["k_new"]), v=_dev(call["v_new"]), causal=True, **kw16,
                            **rkw, **pk)
    _ka, _va, _q8, len_eff, _owned = vr.model(call)
    kw2 = dict(kw, cache_seqlens=torch.tensor(len_eff, dtype=torch.int32, device=DEV))
    o2, lse2 = fp8_attn_with_kvcache_varlen(q8.view(E4), ka.view(E4), va.view(E4), cu_seqlens_q=pk["cu_seqlens_q"],
                                            max_seqlen_q=pk["max_seqlen_q"], num_splits=4, **kw2, **mod)
    torch.cuda.synchronize()
    _RUNS[key] = dict(o=o.cpu(), lse=lse.cpu(), o_ws=o_ws.cpu(), o2=o2.cpu(), lse2=lse2.cpu(), q8=q8.cpu(), ka=ka.cpu(), va=va.cpu(),
                      kb=kb.cpu(), vb=vb.cpu(), ka2=ka2.cpu())
    return _RUNS[key]


STEP_CASES = [(d, layout, rot) for d in WIDTHS for layout in ("contig", "ps16") for rot in ((False, 32), (True, d))] + \
    [(d, "ps48", (True, 32)) for d in WIDTHS] + [(d, "bidx", (False, d)) for d in WIDTHS]
STEP_IDS = [f"d{d}-{layout}-{'gptj' if rot[0] else 'neox'}{rot[1]}" for d, layout, rot in STEP_CASES]


@pytest.mark.parametrize("d,layout,rot", STEP_CASES, ids=STEP_IDS)
def test_step_cache_bytes_are_the_16_bit_calls_append(d, layout, rot):
    r = ran(d, layout, rot)
    call = problem(d, 4, layout, rot=rot)
    assert torch.equal(r["ka"], r["kb"]) and torch.equal(r["va"], r["vb"])
    ka, va, _q8, _len, _owned = vr.model(call)
    assert torch.equal(r["ka"], ka) and torch.equal(r["va"], va)                       # and no byte outside the appended slots changed
    changed = int((r["ka"] != call["k_cache"]).any(-1).any(-1).sum())
    assert 0 < changed <= 11


@pytest.mark.parametrize("d,layout,rot", STEP_CASES, ids=STEP_IDS)
def test_step_q_codes_are_the_models_and_the_workspace_form_gives_the_same_o(d, layout, rot):
    r = ran(d, layout, rot)
    _ka, _va, q8, _len, owned = vr.model(problem(d, 4, layout, rot=rot))
    assert bool(owned.all()) and torch.equal(r["q8"], q8)
    assert torch.equal(r["o_ws"], r["o"]) and torch.equal(r["ka2"], r["ka"])


@pytest.mark.parametrize("d,layout,rot", STEP_CASES, ids=STEP_IDS)
def test_step_attention_is_the_packed_decode_call(d, layout, rot):
    r = ran(d, layout, rot)
    assert torch.equal(r["o"], r["o2"]) and torch.equal(r["lse"], r["lse2"])
    assert bool(torch.isfinite(r["o"].float()).all()) and bool(r["o"].any())


@pytest.mark.parametrize("d", WIDTHS)
def test_the_padded_step_at_every_width_is_the_three_call_chain(d):
    """five null / 0 packed arguments: append + rotary + quantise + attend at d, against the 16-bit call's append, the model's codes and
    the padded decode call"""
    from common.attention_ex import flash_attn_with_kvcache
    from common.fp8_attention import fp8_attn_kvcache_step, fp8_attn_with_kvcache

    call = problem(d, 4, "ps16", rot=(False, 32))
    nq, nnew, hq = 3, 2, call["hq"]
    q = _dev(call["q"])[:5 * nq].reshape(5, nq, hq, d)
    kn, vn = _dev(call["k_new"])[:5 * nnew].reshape(5, nnew, 2, d), _dev(call["v_new"])[:5 * nnew].reshape(5, nnew, 2, d)
    ka, va, kb, vb = (_dev(call[n]) for n in ("k_cache", "v_cache", "k_cache", "v_cache"))
    mod = mod_kw("composite", hq)
    kw = cache_kw(call)
    rkw = dict(rotary_cos=_dev(call["rotary_cos"]), rotary_sin=_dev(call["rotary_sin"]), rotary_interleaved=False)
    q8 = torch.zeros((5, nq, hq, d), dtype=torch.uint8, device=DEV)
    o, lse = fp8_attn_kvcache_step(q, ka.view(E4), va.view(E4), kn, vn, num_splits=4, q8_out=q8.view(E4), **kw, **rkw, **mod)
    kw16 = {n: v for n, v in kw.items() if n not in ("q_descale", "return_softmax_lse")}
    flash_attn_with_kvcache(q, kb.view(E4), vb.view(E4), k=kn, v=vn, window_size=(20, -1), **kw16, **rkw)
    assert torch.equal(ka, kb) and torch.equal(va, vb) and not torch.equal(ka.cpu(), call["k_cache"])
    len_eff = (call["cache_seqlens"].clamp(0, 384 - nnew) + nnew).to(DEV)
    o2, lse2 = fp8_attn_with_kvcache(q8.view(E4), ka.view(E4), va.view(E4), num_splits=4, **dict(kw, cache_seqlens=len_eff), **mod)
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and o.shape == (5, nq, hq, d)


# ---- 6. e4m3 mode

@pytest.mark.parametrize("d,layout", [(64, "ps48"), (128, "bidx"), (256, "contig")])
def test_e4m3_mode_scatters_the_codes_and_uses_q_in_place(d, layout):
    from common.fp8_attention import fp8_attn_kvcache_step, fp8_attn_with_kvcache_varlen

    call = problem(d, 4, layout, e4=True)
    ka, va, q8_m, len_eff, _owned = vr.model(call)
    assert torch.equal(q8_m, call["q"])
    kc, vc, q8 = _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["q"])
    mod = mod_kw("causal", call["hq"])
    kw = cache_kw(call)
    pk = dict(cu_seqlens_q=cu_t(call["cu_q"]), max_seqlen_q=20)
    o, lse = fp8_attn_kvcache_step(q8.view(E4), kc.view(E4), vc.view(E4), _dev(call["k_new"]).view(E4), _dev(call["v_new"]).view(E4),
                                   cu_seqlens_k_new=cu_t(call["cu_kn"]), num_splits=1, **kw, **pk, **mod)
    assert o.dtype == torch.bfloat16 and torch.equal(kc.cpu(), ka) and torch.equal(vc.cpu(), va) and torch.equal(q8.cpu(), call["q"])
    o2, lse2 = fp8_attn_with_kvcache_varlen(q8.view(E4), kc.view(E4), vc.view(E4), num_splits=1,
                                            **dict(kw, cache_seqlens=torch.tensor(len_eff, dtype=torch.int32, device=DEV)), **pk, **mod)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


# ---- 7. padded new keys with packed queries; a strided packed q

@pytest.mark.parametrize("d", WIDTHS)
def test_padded_new_keys_with_packed_queries_and_a_strided_q(d):
    from common.fp8_attention import fp8_attn_kvcache_step, fp8_attn_with_kvcache_varlen

    call = problem(d, 4, "ps16", rot=(True, 32), packed_kn=False)
    ka, va, q8_m, len_eff, _owned = vr.model(call)
    mod = mod_kw("causal", call["hq"])
    kw = cache_kw(call)
    rkw = dict(rotary_cos=_dev(call["rotary_cos"]), rotary_sin=_dev(call["rotary_sin"]), rotary_interleaved=True)
    pk = dict(cu_seqlens_q=cu_t(call["cu_q"]), max_seqlen_q=20)
    qkv = torch.randn((29, 3, call["hq"], d), device=DEV).to(torch.bfloat16)
    qkv[:, 0] = _dev(call["q"])
    outs = []
    for q in (_dev(call["q"]), qkv[:, 0]):
        kc, vc = _dev(call["k_cache"]), _dev(call["v_cache"])
        q8 = torch.zeros((29, call["hq"], d), dtype=torch.uint8, device=DEV)
        o, lse = fp8_attn_kvcache_step(q, kc.view(E4), vc.view(E4), _dev(call["k_new"]), _dev(call["v_new"]), num_splits=4, q8_out=q8.view(E4),
                                       **kw, **rkw, **pk, **mod)
        outs.append((o.cpu(), lse.cpu(), q8.cpu(), kc.cpu(), vc.cpu()))
    assert not qkv[:, 0].is_contiguous()
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert torch.equal(outs[0][2], q8_m) and torch.equal(outs[0][3], ka) and torch.equal(outs[0][4], va)
    # the strided view on the decode call as well
    q8s = torch.zeros((29, 2, call["hq"], d), dtype=torch.uint8, device=DEV)
    q8s[:, 1] = outs[0][2].to(DEV)
    kw2 = dict(kw, cache_seqlens=torch.tensor(len_eff, dtype=torch.int32, device=DEV))
    for q8 in (q8s[:, 1], q8s[:, 1].contiguous()):
        o2, lse2 = fp8_attn_with_kvcache_varlen(q8.view(E4), _dev(ka).view(E4), _dev(va).view(E4), num_splits=4, **kw2, **pk, **mod)
        assert torch.equal(o2.cpu(), outs[0][0]) and torch.equal(lse2.cpu(), outs[0][1])


# ---- 8, 9. rows nobody owns; untrusted offsets

def raw_packed_decode(call, q8, kc, vc, lens, cu, num_splits, mod, total_q=29, max_q=20):
    """the packed decode call on o, lse and a workspace cut out of canary-filled buffers: (o, lse, workspace, the three buffers)"""
    import flashattention_lab_cuda as ext

    hq, d = call["hq"], kc.shape[-1]
    need = int(ext._lib.fa_fp8_forward_kvcache_varlen_workspace_bytes(call["B"], hq, 2, total_q, max_q, vr.capacity(call), d, num_splits,
                                                                      int(mod["causal"]), *mod["window_size"], int(mod["sinks"] is not None)))
    (o, ob), (lse, lb), (ws, wb) = guarded((total_q, hq, d), torch.bfloat16), guarded((hq, total_q), torch.float32), \
        guarded((max(need, 16),), torch.uint8)
    keep = []
    a = decode_args(call, q8, kc, vc, o, lse, lens, ws if need else None, need, num_splits, mod, keep)
    cu_dev = cu_t(cu)
    raw(DECODE_FN, **a, cu_seqlens_q=ptr(cu_dev), total_q=total_q, max_seqlen_q=max_q)
    torch.cuda.synchronize()
    return o, lse, ws, (ob, lb, wb)


def canary_rows(o, lse, rows):
    return bool((o[rows].view(torch.uint8) == CANARY).all()) and bool((lse[:, rows].contiguous().view(torch.uint8) == CANARY).all())


@pytest.mark.parametrize("ns", (1, 4))
@pytest.mark.parametrize("d,layout", [(64, "ps16"), (128, "contig"), (256, "bidx")])
def test_rows_nobody_owns_keep_their_contents(d, layout, ns):
    call = problem(d, 4, layout)
    q8, kc, vc, lens = _dev(codes(call)), _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
    mod = mod_kw("composite" if ns > 1 else "causal", call["hq"])
    cu = [2, 3, 3, 8, 8, 25]                       # rows 0, 1 and 25 .. 28 belong to nobody, and the offsets do not reach total_q
    o, lse, _ws, bufs = raw_packed_decode(call, q8, kc, vc, lens, cu, ns, mod)
    ranges = q_ranges(call, cu)
    assert ranges == [(2, 1), (3, 0), (3, 5), (8, 0), (8, 17)]
    check_rows(o, lse, per_sequence(call, q8, kc, vc, ranges, lens, max(ns, 2) if mod["sinks"] is not None else ns, mod))
    assert canary_rows(o, lse, [0, 1, 25, 26, 27, 28]) and all(guards_intact(b) for b in bufs)
    # nq_b = 0 everywhere: nothing is touched
    o, lse, _ws, bufs = raw_packed_decode(call, q8, kc, vc, lens, [4, 4, 4, 4, 4, 4], ns, mod)
    assert canary_rows(o, lse, list(range(29))) and all(guards_intact(b) for b in bufs)


@pytest.mark.parametrize("d", WIDTHS)
def test_an_all_empty_step_touches_nothing_but_the_append(d):
    import flashattention_lab_cuda as ext

    call = problem(d, 4, "ps16")
    mod = mod_kw("causal", call["hq"])
    hq = call["hq"]
    kc, vc, lens = _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
    q, kn, vn = _dev(call["q"]), _dev(call["k_new"]), _dev(call["v_new"])
    need = int(ext._lib.fa_fp8_kvcache_step_varlen_workspace_bytes(5, hq, 2, 0, 384, d, 4, 1, -1, -1, 0, 2, 1, 29, 20))
    (o, ob), (lse, lb), (ws, wb), (q8, qb) = guarded((29, hq, d), torch.bfloat16), guarded((hq, 29), torch.float32), \
        guarded((need,), torch.uint8), guarded((29, hq, d), torch.uint8)
    keep = []
    a = step_args(call, q, kc, vc, o, lse, lens, ws, 4, mod, kn, vn, q8, None, None, keep)
    cu_q, cu_kn = cu_t([7] * 6), cu_t(call["cu_kn"])
    raw(STEP_FN, **a, cu_seqlens_q=ptr(cu_q), total_q=29, max_seqlen_q=20, cu_seqlens_k_new=ptr(cu_kn), total_k_new=11)
    torch.cuda.synchronize()
    ka, va, _q8, len_eff, _owned = vr.model(dict(call, cu_q=[7] * 6))
    assert torch.equal(kc.cpu(), ka) and torch.equal(vc.cpu(), va) and not torch.equal(ka, call["k_cache"])
    assert canary_rows(o, lse, list(range(29))) and bool((q8 == CANARY).all()) and all(guards_intact(b) for b in (ob, lb, wb, qb))
    assert ws[:20].view(torch.int32).tolist() == len_eff                              # len_b leads the workspace


@pytest.mark.parametrize("name", sorted(vr.BAD_OFFSETS))
def test_untrusted_offsets_are_clamped(name):
    """out-of-range cu_seqlens_q: every sequence gets the rows the documented clamp gives it (checked where one sequence alone owns
    them), rows nobody owns keep the canary, and nothing around o, lse and the workspace is touched"""
    d = {"negative": 64, "past_total": 128, "decreasing": 256, "longer_than_bound": 64, "int_min": 128}[name]
    call = problem(d, 4, "ps48")
    cu = vr.BAD_OFFSETS[name]
    q8, kc, vc, lens = _dev(codes(call)), _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
    mod = mod_kw("causal", call["hq"])
    ranges = q_ranges(call, cu)
    owners = torch.zeros(29, dtype=torch.int32)
    for st, n in ranges:
        assert 0 <= st and n <= 20 and st + n <= 29
        owners[st:st + n] += 1
    for ns in (1, 4):
        o, lse, _ws, bufs = raw_packed_decode(call, q8, kc, vc, lens, cu, ns, mod)
        for tok0, nq, ob, lb in per_sequence(call, q8, kc, vc, ranges, lens, ns, mod):
            alone = owners[tok0:tok0 + nq] == 1
            assert torch.equal(o[tok0:tok0 + nq][alone.to(DEV)], ob[alone.to(DEV)])
            assert torch.equal(lse[:, tok0:tok0 + nq][:, alone.to(DEV)], lb[:, alone.to(DEV)])
        free = [i for i in range(29) if owners[i] == 0]
        assert (not free or canary_rows(o, lse, free)) and all(guards_intact(b) for b in bufs)
    # the same offsets on the new keys of the step: the caches are the model's
    from common.fp8_attention import fp8_attn_kvcache_step

    cu_kn = [min(max(x, -2 ** 31), 2 ** 31 - 1) for x in cu]
    kn, vn = torch.randn((29, 2, d)).to(torch.bfloat16), torch.randn((29, 2, d)).to(torch.bfloat16)
    scall = dict(call, k_new=kn, v_new=vn, cu_kn=cu_kn, cu_q=cu)
    ranges_kn = [vr.cu_range(cu_kn, b, 29, 384) for b in range(5)]
    assert all(0 <= st and st + n <= 29 for st, n in ranges_kn)
    ka, va, q8_m, _len, owned = vr.model(scall)
    kc2, vc2 = _dev(call["k_cache"]), _dev(call["v_cache"])
    q8o, qb = guarded((29, call["hq"], d), torch.uint8)
    fp8_attn_kvcache_step(_dev(call["q"]), kc2.view(E4), vc2.view(E4), _dev(kn), _dev(vn), cu_seqlens_q=cu_t(cu), max_seqlen_q=20,
                          cu_seqlens_k_new=cu_t(cu_kn), num_splits=1, q8_out=q8o.view(E4), **cache_kw(call), **mod)
    torch.cuda.synchronize()
    assert torch.equal(kc2.cpu(), ka) and torch.equal(vc2.cpu(), va) and guards_intact(qb)
    one = (owners == 1)
    assert torch.equal(q8o.cpu()[one], q8_m[one]) and bool((q8o.cpu()[owners == 0] == CANARY).all())


# ---- 10. graph replay

@pytest.mark.parametrize("d,layout", [(64, "ps16"), (256, "contig")])
def test_a_captured_packed_step_replays_after_its_inputs_changed_in_place(d, layout):
    """prep + memset + split + combine in one graph; then offsets (same totals), lengths, table, tokens, descales and sinks change in
    place: the replay equals the eager call on the new values in o, lse, the codes and every cache byte"""
    from common.fp8_attention import fp8_attn_kvcache_step

    call = problem(d, 4, layout, rot=(False, 32))
    gen = torch.Generator().manual_seed(123)
    st = {n: _dev(call[n]) for n in ("q", "k_new", "v_new", "cache_seqlens", "block_table", "q_descale", "k_descale", "v_descale")}
    st["cu_q"], st["cu_kn"] = cu_t(call["cu_q"]), cu_t(call["cu_kn"])
    mod = mod_kw("composite", call["hq"])
    kc, vc = _dev(call["k_cache"]), _dev(call["v_cache"])
    start_k, start_v = kc.clone(), vc.clone()
    q8 = torch.zeros(tuple(call["q"].shape), dtype=torch.uint8, device=DEV)
    kw = dict(cache_seqlens=st["cache_seqlens"], q_descale=st["q_descale"], k_descale=st["k_descale"], v_descale=st["v_descale"],
              softmax_scale=call["scale"], return_softmax_lse=True, rotary_cos=_dev(call["rotary_cos"]), rotary_sin=_dev(call["rotary_sin"]),
              rotary_interleaved=False, cu_seqlens_q=st["cu_q"], max_seqlen_q=20, cu_seqlens_k_new=st["cu_kn"], num_splits=4,
              q8_out=q8.view(E4), **mod)
    if st["block_table"] is not None:
        kw["block_table"] = st["block_table"]

    def step():
        return fp8_attn_kvcache_step(st["q"], kc.view(E4), vc.view(E4), st["k_new"], st["v_new"], **kw)

    def reset():
        kc.copy_(start_k)
        vc.copy_(start_v)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # the warm-up sizes the shim's workspace before the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step()
    st["cu_q"].copy_(torch.tensor([0, 20, 21, 21, 24, 29], dtype=torch.int32))       # the same totals, other owners
    st["cu_kn"].copy_(torch.tensor([0, 2, 5, 5, 10, 11], dtype=torch.int32))
    st["cache_seqlens"].copy_(torch.tensor([40, 393, 5, 0, 200], dtype=torch.int32))
    for n in ("q", "k_new", "v_new"):
        st[n].copy_((1.5 * torch.randn(call[n].shape, generator=gen)).to(torch.bfloat16))
    for n in ("q_descale", "k_descale", "v_descale"):
        st[n].mul_(1.75)
    mod["sinks"].copy_(torch.tensor([0.5, 1e4, float("-inf"), 2.0, -1.0, 0.0, 3.0, 1.0]))
    if st["block_table"] is not None:
        st["block_table"][0].copy_(st["block_table"][0].flip(0))
    reset()
    o.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    got = (o.cpu(), lse.cpu(), q8.cpu(), kc.cpu(), vc.cpu())
    reset()
    q8.zero_()
    o_e, lse_e = step()
    torch.cuda.synchronize()
    for x, y in zip(got, (o_e.cpu(), lse_e.cpu(), q8.cpu(), kc.cpu(), vc.cpu())):
        assert torch.equal(x, y)
    assert not torch.equal(got[3], start_k.cpu()) and bool(got[2].any())


# ---- 11. route counters

def test_route_counters():
    import flashattention_lab_cuda as ext
    from common.attention_ex import flash_attn_fp8_kvcache_step, flash_attn_fp8_with_kvcache
    from common.fp8_attention import fp8_attn_kvcache_step, fp8_attn_with_kvcache

    new, old = ("fp8kv_split_varlen", "fp8kv_step_prep_varlen"), ("fp8kv_split_mod", "fp8kv_split_hdim", "fp8kv_step_prep")
    count = lambda names: [ext.route_count(n) for n in names]   # noqa: E731
    for d in (64, 128):
        call = problem(d, 4, "contig")
        q8, kc, vc, lens = _dev(codes(call)), _dev(call["k_cache"]), _dev(call["v_cache"]), _dev(call["cache_seqlens"])
        for name in ("bare", "composite"):
            mod = mod_kw(name, call["hq"])
            b_new, b_old = count(new), count(old)
            run_decode(call, q8, kc, vc, lens, 4, mod)
            assert count(new) == [b_new[0] + 1, b_new[1]] and count(old) == b_old
            fp8_attn_kvcache_step(_dev(call["q"]), kc.view(E4), vc.view(E4), _dev(call["k_new"]), _dev(call["v_new"]),
                                  cu_seqlens_q=cu_t(call["cu_q"]), max_seqlen_q=20, cu_seqlens_k_new=cu_t(call["cu_kn"]), num_splits=4,
                                  **cache_kw(call), **mod)
            assert count(new) == [b_new[0] + 2, b_new[1] + 1] and count(old) == b_old
        # the old calls count what they counted, and none of the new routes
        mod = mod_kw("composite", call["hq"])
        b_new, b_old = count(new), count(old)
        q4 = q8[:10].reshape(5, 2, call["hq"], d)
        fp8_attn_with_kvcache(q4.view(E4), kc.view(E4), vc.view(E4), num_splits=4, **cache_kw(call), **mod)
        assert count(new) == b_new and count(old) == [b_old[0] + (d == 128), b_old[1] + (d == 64), b_old[2]]
        if d == 128:
            flash_attn_fp8_with_kvcache(q4.view(E4), kc.view(E4), vc.view(E4), num_splits=4, **cache_kw(call), **mod)
            q16 = _dev(call["q"])[:10].reshape(5, 2, call["hq"], d)
            kn, vn = _dev(call["k_new"])[:10].reshape(5, 2, 2, d), _dev(call["v_new"])[:10].reshape(5, 2, 2, d)
            flash_attn_fp8_kvcache_step(q16, kc.view(E4), vc.view(E4), kn, vn, num_splits=4, **cache_kw(call), **mod)
            fp8_attn_kvcache_step(q16, kc.view(E4), vc.view(E4), kn, vn, num_splits=4, **cache_kw(call), **mod)   # IS the step above
            assert count(new) == b_new and count(old) == [b_old[0] + 4, b_old[1], b_old[2] + 2]
        else:
            q16 = _dev(call["q"])[:10].reshape(5, 2, call["hq"], d)
            kn, vn = _dev(call["k_new"])[:10].reshape(5, 2, 2, d), _dev(call["v_new"])[:10].reshape(5, 2, 2, d)
            fp8_attn_kvcache_step(q16, kc.view(E4), vc.view(E4), kn, vn, num_splits=4, **cache_kw(call), **mod)   # the padded step at 64
            assert count(new) == [b_new[0], b_new[1] + 1] and count(old) == [b_old[0], b_old[1] + 2, b_old[2]]
    torch.cuda.synchronize()
