"""CPU: the KV-cache decoding sweep without a GPU — the case table (tests/kvcache_sweep_cases.py) is deterministic, legal under a
transcription of the kvcache_impl argument rules (csrc/fa_capi.hip), covers every allowed pair and stays within its cap; the
whole-call reference (tests/kvcache_full_ref.py) agrees to fp64 round-off with each single-feature reference on every case that
reference can express; and the split kernel's row packing and split rule, modelled in tests/test_kvcache_cpu.py for any group
size, give every row of every table case its band exactly once."""
import functools
import math

import pytest
import torch

from tests import kvcache_sweep_cases as sc
from tests import sink_ref as sr
from tests.kvcache_full_ref import full_reference
from tests.kvcache_paged_ref import paged_tokens, reference
from tests.kvcache_rotary_ref import rotary_reference, rotate64, round_once, slot_of
from tests.kvcache_varlen_ref import cu_range, packed_reference
from tests.test_kvcache_cpu import check_group_arithmetic

TIGHT = dict(rtol=1e-12, atol=1e-12)
IDS = [sc.case_id(i) for i in range(len(sc.CASES))]


# ---- the table

def test_table_is_deterministic_and_within_its_cap():
    assert sc.generate() == sc.CASES
    assert 0 < len(sc.CASES) <= sc.MAX_CASES <= 120
    assert len(set(IDS)) == len(IDS)


def test_every_allowed_pair_is_covered():
    covered = set()
    for c in sc.CASES:
        covered |= sc.pairs_of(c)
    assert sc.all_pairs() <= covered
    # the only pairs left out are the ones the C layer refuses
    for (a, va), (b, vb) in covered:
        assert sc.pair_legal(a, va, b, vb)
    every = {((a, va), (b, vb)) for i, a in enumerate(sc.NAMES) for b in sc.NAMES[i + 1:] for va in sc.AXES[a] for vb in sc.AXES[b]}
    for (a, va), (b, vb) in every - sc.all_pairs():
        assert "rotary" in (a, b) and va != "off" and vb != "off", ((a, va), (b, vb))


def test_every_bold_value_is_in_at_least_three_cases():
    for axis, vals in sc.BOLD.items():
        for v in vals:
            assert v in sc.AXES[axis]
            assert sum(1 for c in sc.CASES if c[axis] == v) >= 3, (axis, v)
    assert 8 <= len(sc.fixed_split_cases()) <= 12


def impl_error(kw):
    """the first argument rule of kvcache_impl (csrc/fa_capi.hip) that the call kw breaks, or None"""
    q, kc = kw["q"], kw["k_cache"]
    hq, d = q.shape[-2:]
    ps, hkv = kc.shape[1], kc.shape[2]
    vq, vk = kw["cu_seqlens_q"] is not None, kw["cu_seqlens_k_new"] is not None
    if q.dtype not in (torch.float16, torch.bfloat16):
        return "dtype"
    if kc.dtype not in (q.dtype, torch.float8_e4m3fn) or kw["v_cache"].dtype != kc.dtype:
        return "cache_dtype"
    if kc.dtype == q.dtype and (kw["k_descale"] is not None or kw["v_descale"] is not None):
        return "descale without an e4m3 cache"
    if d < 8 or d > 256 or d % 8:
        return "head_dim"
    if hkv < 1 or hq % hkv:
        return "heads"
    if vk and not vq:
        return "cu_seqlens_k_new needs cu_seqlens_q"
    if vk and kw["k_new"] is None:
        return "cu_seqlens_k_new needs k_new"
    if vq:
        seqlen_q = kw["max_seqlen_q"]
        if not 0 <= seqlen_q <= q.shape[0]:
            return "max_seqlen_q"
    else:
        seqlen_q = q.shape[1]
        if seqlen_q < 1:
            return "seqlen_q"
    if kw["sinks"] is not None and kw["sinks"].shape != (hq,):
        return "sinks"
    cache_len = ps
    if kw["block_table"] is not None:
        if kw["cache_batch_idx"] is not None or kw["cache_leftpad"] is not None:
            return "block_table with cache_batch_idx / cache_leftpad"
        if ps < 16 or ps % 16:
            return "page_block_size"
        cache_len = kw["block_table"].shape[1] * ps
    if vk:
        seqlen_new = min(kw["k_new"].shape[0], cache_len)
    else:
        seqlen_new = kw["k_new"].shape[1] if kw["k_new"] is not None else 0
    if seqlen_new > cache_len:
        return "seqlen_new"
    if seqlen_new > 0 and (kw["cache_seqlens"] is None or kw["v_new"] is None):
        return "seqlen_new needs cache_seqlens"
    if min(kw["window"]) < -1:
        return "window"
    if (kw["rotary_cos"] is None) != (kw["rotary_sin"] is None):
        return "rotary tables"
    if kw["rotary_cos"] is not None:
        rdim = 2 * kw["rotary_cos"].shape[1]
        if rdim < 16 or rdim > d or rdim % 16:
            return "rotary_dim"
        if seqlen_new < 1 or kw["cache_seqlens"] is None:
            return "rotary needs new keys"
        if kw["rotary_cos"].shape[0] < cache_len + (seqlen_q if vq else max(0, seqlen_q - seqlen_new)):
            return "seqlen_ro"
    if kw["softcap"] < 0 or not 0 <= kw["num_splits"] <= 256:
        return "softcap / num_splits"
    return None


@functools.lru_cache(maxsize=None)
def case_ref(i):
    kw = sc.build_inputs(i)
    return kw, full_reference(**sc.call_keywords(kw))


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_case_is_legal_and_has_the_promised_sequences(i):
    c = sc.CASES[i]
    assert sc.case_legal(c)
    kw, r = case_ref(i)
    assert impl_error(kw) is None
    assert kw["q"].shape[-1] == c["d"] and kw["q"].shape[-2] == c["heads"][0] and kw["k_cache"].shape[2] == c["heads"][1]
    assert (kw["k_cache"].dtype == torch.float8_e4m3fn) == (c["cache"] == "e4m3")
    assert 0 in r.L and any(r.L[b] + r.nnew[b] == sc.CAP for b in range(sc.B))             # an empty and a full sequence
    assert all(x in (0, 1, 33, 100) or x + n == sc.CAP for x, n in zip(r.L, r.nnew))
    if c["queries"].startswith("packed"):
        assert 0 in r.nq and max(r.nq) == kw["max_seqlen_q"] and not r.own.all() and torch.isnan(r.lse[:, ~r.own]).all()
    assert not torch.isnan(r.o).any() and not torch.isnan(r.lse[..., r.own] if r.lse.dim() == 2 else r.lse).any()
    if c["sinks"]:
        assert torch.isfinite(r.lse[0, r.own] if r.lse.dim() == 2 else r.lse[:, 0]).all()   # head 0 has a finite sink


def test_rule_transcription_refuses_what_the_table_leaves_out():
    kw = dict(sc.build_inputs(0))
    assert impl_error(kw) is None
    paged = next(i for i, c in enumerate(sc.CASES) if c["addr"] == "paged16")
    assert "block_table" in impl_error(dict(sc.build_inputs(paged), cache_leftpad=torch.zeros(4, dtype=torch.int32)))
    rot = next(i for i, c in enumerate(sc.CASES) if c["rotary"] != "off" and not c["queries"].startswith("packed"))
    assert impl_error(dict(sc.build_inputs(rot), k_new=None, v_new=None)) == "rotary needs new keys"
    assert impl_error(dict(sc.build_inputs(rot), rotary_cos=torch.zeros(400, 4), rotary_sin=torch.zeros(400, 4))) == "rotary_dim"
    pk = next(i for i, c in enumerate(sc.CASES) if c["queries"].startswith("packed") and c["nnew"])
    assert "cu_seqlens_q" in impl_error(dict(sc.build_inputs(pk), cu_seqlens_q=None))


# ---- the reference against the single-feature references

def stitched(kw):
    """The call kw (16-bit cache) through the existing helpers, the way the feature tests stitch them: append by hand (rotate64 +
    round_once when rotary), gather each sequence's tokens, then kvcache_paged_ref.reference (padded, no sinks),
    sink_ref.sink_attention per sequence (sinks) or kvcache_varlen_ref.packed_reference (packed).  Returns (o, lse, k, v)."""
    q, table, bidx, pad = kw["q"], kw["block_table"], kw["cache_batch_idx"], kw["cache_leftpad"]
    ek, ev = kw["k_cache"].clone(), kw["v_cache"].clone()
    ps, hkv, d = ek.shape[1], ek.shape[2], ek.shape[3]
    cap = ps * (table.shape[1] if table is not None else 1)
    packed = kw["cu_seqlens_q"] is not None
    rotary, causal, window = kw["rotary_cos"] is not None, kw["causal"], kw["window"]
    per_token = causal or max(window) >= 0
    ks, vs, pos_q = [], [], []
    for b in range(sc.B):
        if kw["cu_seqlens_k_new"] is not None:
            s0, nn = cu_range(kw["cu_seqlens_k_new"], b, kw["k_new"].shape[0], cap)
            kn, vn = kw["k_new"][s0:s0 + nn], kw["v_new"][s0:s0 + nn]
        elif kw["k_new"] is not None:
            kn, vn = kw["k_new"][b], kw["v_new"][b]
            nn = kn.shape[0]
        else:
            nn = 0
        L = min(max(int(kw["cache_seqlens"][b]), 0), cap - nn)
        P = min(max(int(pad[b]), 0), L) if pad is not None else 0
        if nn and rotary:
            kn = round_once(rotate64(kn, kw["rotary_cos"], kw["rotary_sin"], [L - P + n for n in range(nn)], kw["rotary_interleaved"]), q.dtype)
        for n in range(nn):
            unit, slot = slot_of(b, L + n, table, bidx, ps)
            if 0 <= unit < ek.shape[0]:
                ek[unit, slot], ev[unit, slot] = kn[n], vn[n]
        pos_q.append(L - P)
    for b in range(sc.B):
        nn = cu_range(kw["cu_seqlens_k_new"], b, kw["k_new"].shape[0], cap)[1] if kw["cu_seqlens_k_new"] is not None else \
            (kw["k_new"].shape[1] if kw["k_new"] is not None else 0)
        L = min(max(int(kw["cache_seqlens"][b]), 0), cap - nn)
        P = min(max(int(pad[b]), 0), L) if pad is not None else 0
        if table is not None:
            ks.append(paged_tokens(ek, table[b], L + nn, ps))
            vs.append(paged_tokens(ev, table[b], L + nn, ps))
        else:
            row = int(bidx[b]) if bidx is not None else b
            inside = 0 <= row < ek.shape[0]
            ks.append(ek[row, P:L + nn] if inside else torch.zeros((L + nn - P, hkv, d), dtype=ek.dtype))
            vs.append(ev[row, P:L + nn] if inside else torch.zeros((L + nn - P, hkv, d), dtype=ev.dtype))
    scale, softcap, slopes, sinks = d ** -0.5, kw["softcap"], kw["alibi_slopes"], kw["sinks"]
    if packed:
        cu = [int(x) for x in kw["cu_seqlens_q"]]
        qr = q
        if rotary:
            pos = [0] * q.shape[0]
            for b in range(sc.B):
                for t in range(cu[b], cu[b + 1]):
                    pos[t] = pos_q[b] + (t - cu[b] if per_token else 0)
            qr = round_once(rotate64(q, kw["rotary_cos"], kw["rotary_sin"], pos, kw["rotary_interleaved"]), q.dtype)
        o, lse = packed_reference(qr, cu, ks, vs, causal, window, scale, softcap, slopes, None)
        if sinks is None:
            return o, lse, ek, ev
        q_of = lambda b: qr[cu[b]:cu[b + 1]]   # noqa: E731
        put = lambda b: (slice(cu[b], cu[b + 1]), (slice(None), slice(cu[b], cu[b + 1])))   # noqa: E731
    else:
        nq = q.shape[1]
        qr = q
        if rotary:
            qr = torch.stack([round_once(rotate64(q[b], kw["rotary_cos"], kw["rotary_sin"], [pos_q[b] + (i if per_token else 0) for i in range(nq)],
                                                  kw["rotary_interleaved"]), q.dtype) for b in range(sc.B)])
        if sinks is None:
            o, lse = reference(qr, ks, vs, causal, window, scale, softcap, slopes)
            return o, lse, ek, ev
        o = torch.zeros(q.shape, dtype=torch.float64)
        lse = torch.zeros((sc.B, q.shape[2], nq), dtype=torch.float64)
        q_of = lambda b: qr[b]   # noqa: E731
        put = lambda b: (b, b)   # noqa: E731
    assert slopes is None, "no existing reference takes ALiBi with sinks"
    for b in range(sc.B):   # sinks: sink_ref's fp64 core on each sequence alone
        qb = q_of(b)
        if qb.shape[0] == 0:
            continue
        io, il = put(b)
        if ks[b].shape[0] == 0:
            o[io], lse[il] = 0.0, sinks.double().view(-1, 1).expand(-1, qb.shape[0])
            continue
        ob, lb = sr.sink_attention(qb.double().transpose(0, 1), ks[b].double().transpose(0, 1), vs[b].double().transpose(0, 1), sinks.double(),
                                   causal, scale, softcap=softcap, window=window)
        o[io], lse[il] = ob.transpose(0, 1), lb
    return o, lse, ek, ev


def compare(r, o, lse, ek, ev):
    own = r.own
    if r.lse.dim() == 2:
        assert torch.equal(torch.isnan(lse[0]), ~own)
        torch.testing.assert_close(r.o[own], o[own], **TIGHT)
        a, b = r.lse[:, own], lse[:, own]
    else:
        torch.testing.assert_close(r.o, o, **TIGHT)
        a, b = r.lse, lse
    assert torch.equal(torch.isfinite(a), torch.isfinite(b))
    torch.testing.assert_close(a[torch.isfinite(a)], b[torch.isfinite(a)], **TIGHT)
    assert torch.equal(r.k_cache.view(torch.int16), ek.view(torch.int16)) and torch.equal(r.v_cache.view(torch.int16), ev.view(torch.int16))


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_reference_agrees_with_the_single_feature_references(i):
    """case i with a 16-bit cache, once without sinks (kvcache_paged_ref.reference, packed_reference, rotate64 + either) and once
    with sinks and without ALiBi (sink_ref); the case itself when it already is one of these"""
    c = sc.CASES[i]
    no_alibi = {"alibi": "none", "alibi_b+softcap": "softcap"}.get(c["mods"], c["mods"])
    for variant in (dict(c, cache="16bit", sinks=False), dict(c, cache="16bit", sinks=True, mods=no_alibi)):
        kw = sc.build_inputs(i, variant)
        r = full_reference(**sc.call_keywords(kw))
        compare(r, *stitched(kw))


def test_reference_agrees_with_rotary_reference():
    """the padded rotary cases through kvcache_rotary_ref.rotary_reference as a whole (caches included)"""
    n = 0
    for i, c in enumerate(sc.CASES):
        if c["rotary"] == "off" or c["queries"].startswith("packed"):
            continue
        kw = sc.build_inputs(i, dict(c, cache="16bit", sinks=False))
        if kw["cache_batch_idx"] is not None and int(kw["cache_batch_idx"].max()) >= kw["k_cache"].shape[0]:
            continue   # (rotary_reference cannot read a row outside the cache)
        r = full_reference(**sc.call_keywords(kw))
        ro, rlse, ek, ev, exact, L, P = rotary_reference(kw["q"], kw["k_cache"], kw["v_cache"], kw["k_new"], kw["v_new"], kw["cache_seqlens"],
                                                         kw["rotary_cos"], kw["rotary_sin"], kw["rotary_interleaved"], kw["causal"], kw["window"],
                                                         kw["q"].shape[-1] ** -0.5, kw["softcap"], kw["alibi_slopes"], kw["block_table"],
                                                         kw["cache_batch_idx"], kw["cache_leftpad"])
        compare(r, ro, rlse, ek, ev)
        assert r.L == L and r.P == P
        for b in range(sc.B):
            assert torch.equal(r.k_exact[b], exact[b])
        n += 1
    assert n >= 5


def test_reference_dequantises_and_quantises_as_kvcache_fp8_ref():
    """the e4m3 cases without rotary and sinks: kvcache_fp8_ref.dequantize of the reference's own caches + kvcache_paged_ref.reference,
    and the appended codes are kvcache_fp8_ref.quantize of the new keys under the sequence's scale"""
    from tests.kvcache_fp8_ref import dequantize, quantize

    n = 0
    for i, c in enumerate(sc.CASES):
        if c["cache"] != "e4m3" or c["queries"].startswith("packed") or c["addr"] != "contig":
            continue
        kw = sc.build_inputs(i, dict(c, rotary="off", sinks=False))
        r = full_reference(**sc.call_keywords(kw))
        kd, vd = dequantize(r.k_cache.view(torch.uint8), kw["k_descale"]), dequantize(r.v_cache.view(torch.uint8), kw["v_descale"])
        ks = [kd[b, :r.L[b] + r.nnew[b]] for b in range(sc.B)]
        vs = [vd[b, :r.L[b] + r.nnew[b]] for b in range(sc.B)]
        o, lse = reference(kw["q"], ks, vs, kw["causal"], kw["window"], kw["q"].shape[-1] ** -0.5, kw["softcap"], kw["alibi_slopes"])
        torch.testing.assert_close(r.o, o, **TIGHT)
        fin = torch.isfinite(lse)
        assert torch.equal(torch.isfinite(r.lse), fin)
        torch.testing.assert_close(r.lse[fin], lse[fin], **TIGHT)
        if c["nnew"]:
            want = quantize(kw["k_new"], kw["k_descale"])
            for b, n_, unit, pos in r.slots:
                assert torch.equal(r.k_cache.view(torch.uint8)[unit, pos], want[b, n_])
        n += 1
    assert n >= 3


def test_alibi_with_sinks_against_a_dense_softmax():
    """no existing reference takes ALiBi and sinks together: element by element, softmax over [scores, sink] in fp64"""
    done = 0
    for i, c in enumerate(sc.CASES):
        if not (c["sinks"] and "alibi" in c["mods"]) or done >= 4:
            continue
        kw = sc.build_inputs(i, dict(c, cache="16bit", rotary="off"))
        r = full_reference(**sc.call_keywords(kw))
        _o, _lse, ek, ev = stitched(dict(kw, sinks=None))                      # (the gathered caches only)
        assert torch.equal(ek, r.k_cache) and torch.equal(ev, r.v_cache)
        hq, d = kw["q"].shape[-2:]
        g = hq // ek.shape[2]
        packed = kw["cu_seqlens_q"] is not None
        wl, wr = kw["window"]
        for b in range(sc.B):
            start = int(kw["cu_seqlens_q"][b]) if packed else 0
            lk = r.L[b] + r.nnew[b] - r.P[b]
            if kw["block_table"] is not None:
                kt, vt = paged_tokens(ek, kw["block_table"][b], lk, ek.shape[1]), paged_tokens(ev, kw["block_table"][b], lk, ek.shape[1])
            else:
                row = int(kw["cache_batch_idx"][b]) if kw["cache_batch_idx"] is not None else b
                if not 0 <= row < ek.shape[0]:
                    continue
                kt, vt = ek[row, r.P[b]:r.P[b] + lk], ev[row, r.P[b]:r.P[b] + lk]
            sl = kw["alibi_slopes"][b] if kw["alibi_slopes"].dim() == 2 else kw["alibi_slopes"]
            for t in range(r.nq[b]):
                for h in (0, 1 % hq, 3 % hq, hq - 1):
                    qv = (kw["q"][start + t, h] if packed else kw["q"][b, t, h]).double()
                    logits, vals = [], []
                    for j in range(lk):
                        dist = t + lk - r.nq[b] - j
                        if (kw["causal"] and dist < 0) or (wl >= 0 and dist > wl) or (wr >= 0 and -dist > wr):
                            continue
                        s = float(qv @ kt[j, h // g].double()) * d ** -0.5
                        if kw["softcap"] > 0:
                            s = kw["softcap"] * math.tanh(s / kw["softcap"])
                        logits.append(s - float(sl[h]) * abs(dist))
                        vals.append(vt[j, h // g].double())
                    logits.append(float(kw["sinks"][h]))
                    x = torch.tensor(logits, dtype=torch.float64)
                    want_lse = torch.logsumexp(x, 0)
                    got_o = r.o[start + t, h] if packed else r.o[b, t, h]
                    got_lse = r.lse[h, start + t] if packed else r.lse[b, h, t]
                    if want_lse == -math.inf:
                        assert got_lse == -math.inf and (got_o == 0).all()
                        continue
                    w = torch.exp(x - want_lse)[:-1]
                    want_o = (w.view(-1, 1) * torch.stack(vals)).sum(0) if vals else torch.zeros(d, dtype=torch.float64)
                    torch.testing.assert_close(got_o, want_o, **TIGHT)
                    torch.testing.assert_close(got_lse, want_lse, **TIGHT)
        done += 1
    assert done >= 2


# ---- group arithmetic on the table's own shapes

def launched_splits(c):
    """S as the C layer sets it (kv_splits, kv_num_splits in csrc/fa_decode.hip; a sink call runs at least two)"""
    hq, hkv = c["heads"]
    mq = int(c["queries"][6:] if c["queries"].startswith("packed") else c["queries"][2:])
    s = c["splits"]
    if s == 0:
        units = sc.B * hkv * ((hq // hkv * mq + 15) // 16)
        s = max(1, min((256 * 16 + units - 1) // units, (sc.CAP + 127) // 128, 256))
    return max(s, 2) if c["sinks"] else s


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_group_arithmetic_on_the_case(i):
    c = sc.CASES[i]
    _kw, r = case_ref(i)
    g = c["heads"][0] // c["heads"][1]
    causal = c["mask"] in ("causal", "causal+window33")
    wl, wr = sc.window_of(c["mask"])
    for b in range(sc.B):
        if r.nq[b]:
            check_group_arithmetic(g, r.nq[b], r.L[b] + r.nnew[b] - r.P[b], causal, wl, wr, launched_splits(c))
