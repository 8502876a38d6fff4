"""GPU: which C entry point, and which workspace-size function, every form of the fp8 / MXFP4 shim calls reaches
(flashattention_lab_cuda: fp8_forward, fp8_varlen_forward, fp8_kvcache_forward, fp8_kvcache_step, fp4_kvcache_forward,
fp4_varlen_forward; DESIGN.md, the host boundary).  "Launch for launch the parent's call" is a promise of these families: a call with
no feature goes through its parent's entry point, a featured one through _mod, hdim=True through _hdim, packed queries through
_varlen, the padded step at 128 through fa_fp8_kvcache_step.  ext._call and the library's *_workspace_bytes functions are wrapped by
recorders that note the name and delegate, so every call below launches; the shapes are the smallest that do: B 2, H_q 4 / H_kv 2,
Nq 1, 64 cached keys, contiguous caches, bf16 out.  The outputs' values are other files' business; here they must be finite.
Below the entry points, the three MXFP4 launchers pick a kernel route by head dim and features; test_fp4_kernel_route_* read it back
from the library's route counters (fa_route_count)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, E4 = "cuda", torch.float8_e4m3fn
B, HQ, HKV, CAP = 2, 4, 2, 64
WINDOW = dict(window=(16, -1))


@pytest.fixture
def routes(monkeypatch):
    """the names ext._call and the workspace-size functions were called with, in order"""
    import flashattention_lab_cuda as ext

    seen = []
    real = ext._call

    def call(name, values):
        seen.append(name)
        return real(name, values)

    monkeypatch.setattr(ext, "_call", call)
    for name in ext.EXPORTED_C_SYMBOLS:
        if name.startswith(("fa_fp8_", "fa_fp4_")) and "_workspace_bytes" in name:
            fn = getattr(ext._lib, name)
            monkeypatch.setattr(ext._lib, name, lambda *a, _fn=fn, _name=name: (seen.append(_name), _fn(*a))[1])
    return seen


def f8(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(E4).to(DEV)


def bf(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(torch.bfloat16).to(DEV)


def i32(*values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def finite(o, lse):
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())


KV = "fa_fp8_forward_kvcache"


@pytest.mark.parametrize("form,d,kw,want", [
    ("plain", 128, {}, [KV + "_workspace_bytes", KV]),
    ("windowed", 128, WINDOW, [KV + "_workspace_bytes_mod", KV + "_mod"]),
    ("hdim", 64, dict(hdim=True), [KV + "_hdim_workspace_bytes", KV + "_hdim"]),
    ("packed", 128, dict(packed=True), [KV + "_varlen_workspace_bytes", KV + "_varlen"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp8_kvcache_forward(routes, form, d, kw, want):
    import flashattention_lab_cuda as ext

    kw = dict(kw)
    q = f8(B, HQ, d) if kw.pop("packed", False) else f8(B, 1, HQ, d)
    if q.dim() == 3:
        kw.update(cu_seqlens_q=i32(0, 1, 2), max_seqlen_q=1)
    finite(*ext.fp8_kvcache_forward(q, f8(B, CAP, HKV, d, seed=1), f8(B, CAP, HKV, d, seed=2), cache_seqlens=i32(64, 33), **kw))
    assert routes == want


STEP = "fa_fp8_kvcache_step"


@pytest.mark.parametrize("form,d,kw,want", [
    ("padded", 128, {}, [STEP + "_workspace_bytes", STEP]),
    ("hdim", 64, dict(hdim=True), [STEP + "_varlen_workspace_bytes", STEP + "_varlen"]),
    ("packed", 128, dict(packed=True), [STEP + "_varlen_workspace_bytes", STEP + "_varlen"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp8_kvcache_step(routes, form, d, kw, want):
    import flashattention_lab_cuda as ext

    kw = dict(kw)
    q = bf(B, HQ, d) if kw.pop("packed", False) else bf(B, 1, HQ, d)
    if q.dim() == 3:
        kw.update(cu_seqlens_q=i32(0, 1, 2), max_seqlen_q=1)
    finite(*ext.fp8_kvcache_step(q, f8(B, CAP, HKV, d, seed=1), f8(B, CAP, HKV, d, seed=2), bf(B, 1, HKV, d, seed=3), bf(B, 1, HKV, d, seed=4),
                                 i32(63, 33), **kw))
    assert routes == want


def fp4_cache(lead):
    """random code bytes and unit scale bytes (127) of an MXFP4 cache with the leading extents `lead`"""
    g = torch.Generator().manual_seed(5)
    kc, vc = (torch.randint(0, 256, (*lead, HKV, 64), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    return kc, torch.full((*lead, HKV, 4), 127, dtype=torch.uint8, device=DEV), vc, torch.full((*lead, HKV), 127, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("form,kw,want", [
    ("plain", {}, ["fa_fp4_forward_kvcache_workspace_bytes", "fa_fp4_forward_kvcache"]),
    ("windowed", WINDOW, ["fa_fp4_forward_kvcache_workspace_bytes_mod", "fa_fp4_forward_kvcache_mod"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp4_kvcache_forward(routes, form, kw, want):
    import flashattention_lab_cuda as ext

    finite(*ext.fp4_kvcache_forward(f8(B, 1, HQ, 128), *fp4_cache((B, CAP)), cache_seqlens=i32(64, 33), **kw))
    assert routes == want


@pytest.mark.parametrize("form,kw,want", [
    ("plain", {}, ["fa_fp4_forward_varlen"]),
    ("windowed", WINDOW, ["fa_fp4_forward_varlen_mod"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp4_varlen_forward(routes, form, kw, want):
    import flashattention_lab_cuda as ext

    table = torch.arange(8, dtype=torch.int32, device=DEV).reshape(B, 4)          # 8 pages of 16 tokens, 4 a sequence
    finite(*ext.fp4_varlen_forward(f8(B, HQ, 128), *fp4_cache((8, 16)), i32(0, 1, 2), i32(0, 64, 97), 1, CAP, table, **kw))
    assert routes == want


FP4_ROUTES = ("fp4kv_append", "fp4kv_split", "fp4kv_prefill", "fp4kv_split_mod", "fp4kv_prefill_mod",
              "fp4kv_append_hdim", "fp4kv_split_hdim", "fp4kv_prefill_hdim")
FP4_FORMS = [("plain", 128, {}, ""), ("windowed", 128, WINDOW, "_mod"), ("hdim64", 64, dict(hdim=True), "_hdim"),
             ("hdim256", 256, dict(hdim=True), "_hdim"), ("hdim64_windowed", 64, dict(hdim=True, **WINDOW), "_hdim"),
             # 128 through the _hdim entry points counts under the 128 names
             ("hdim128", 128, dict(hdim=True), ""), ("hdim128_windowed", 128, dict(hdim=True, **WINDOW), "_mod")]


def fp4_cache_d(lead, d):
    """fp4_cache at head dim d: codes (.., d / 2), k_scale (.., d / 32)"""
    g = torch.Generator().manual_seed(5)
    kc, vc = (torch.randint(0, 256, (*lead, HKV, d // 2), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    return kc, torch.full((*lead, HKV, d // 32), 127, dtype=torch.uint8, device=DEV), vc, torch.full((*lead, HKV), 127, dtype=torch.uint8, device=DEV)


def fp4_route_hits(fn):
    """the fp4 routes the library counted during fn(), each with its count"""
    import flashattention_lab_cuda as ext

    before = [ext.route_count(r) for r in FP4_ROUTES]
    fn()
    torch.cuda.synchronize()
    return {r: ext.route_count(r) - x for r, x in zip(FP4_ROUTES, before) if ext.route_count(r) != x}


@pytest.mark.parametrize("form,d,kw,suffix", FP4_FORMS, ids=[f[0] for f in FP4_FORMS])
def test_fp4_kernel_route_decode(form, d, kw, suffix):
    """the kernel route of the decode call (the library's own counters): 128 plain, 128 featured, 64 / 256 whatever the features;
    B 2, H 4:2, Nq 1 over 80 cached keys"""
    import flashattention_lab_cuda as ext

    hits = fp4_route_hits(lambda: finite(*ext.fp4_kvcache_forward(f8(B, 1, HQ, d), *fp4_cache_d((B, 80), d), cache_seqlens=i32(80, 33), **kw)))
    assert hits == {"fp4kv_split" + suffix: 1}


@pytest.mark.parametrize("form,d,kw,suffix", FP4_FORMS, ids=[f[0] for f in FP4_FORMS])
def test_fp4_kernel_route_prefill(form, d, kw, suffix):
    """the same of the prefill call: a 40-token chunk a sequence over 80 keys, pages of 16"""
    import flashattention_lab_cuda as ext

    table = torch.arange(10, dtype=torch.int32, device=DEV).reshape(B, 5)
    hits = fp4_route_hits(lambda: finite(*ext.fp4_varlen_forward(f8(B * 40, HQ, d), *fp4_cache_d((10, 16), d), i32(0, 40, 80), i32(0, 80, 160),
                                                                 40, 80, table, **kw)))
    assert hits == {"fp4kv_prefill" + suffix: 1}


@pytest.mark.parametrize("d,kw,suffix", [(128, {}, ""), (64, dict(hdim=True), "_hdim"), (256, dict(hdim=True), "_hdim"),
                                           (128, dict(hdim=True), "")])
def test_fp4_kernel_route_append(d, kw, suffix):
    """the same of the append: one new token a sequence into a cache of 80"""
    import flashattention_lab_cuda as ext

    hits = fp4_route_hits(lambda: ext.fp4_kvcache_append(bf(B, 1, HKV, d, seed=3), bf(B, 1, HKV, d, seed=4), *fp4_cache_d((B, 80), d), i32(40, 33), **kw))
    assert hits == {"fp4kv_append" + suffix: 1}


FWD = "fa_fp8_forward"


@pytest.mark.parametrize("form,d,kw,want", [
    ("plain", 128, {}, [FWD + "_workspace_bytes", FWD]),
    ("windowed", 128, WINDOW, [FWD + "_workspace_bytes", FWD + "_mod"]),
    ("hdim", 64, dict(hdim=True), [FWD + "_hdim_workspace_bytes", FWD + "_hdim"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp8_forward(routes, form, d, kw, want):
    import flashattention_lab_cuda as ext

    finite(*ext.fp8_forward(f8(B, HQ, 1, d), f8(B, HKV, CAP, d, seed=1), f8(B, HKV, CAP, d, seed=2), False, None, **kw))
    assert routes == want


@pytest.mark.parametrize("form,d,kw,want", [
    ("plain", 128, {}, [FWD + "_varlen_workspace_bytes", FWD + "_varlen"]),
    ("windowed", 128, WINDOW, [FWD + "_varlen_workspace_bytes", FWD + "_varlen_mod"]),
    ("hdim", 64, dict(hdim=True), [FWD + "_varlen_hdim_workspace_bytes", FWD + "_varlen_hdim"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp8_varlen_forward(routes, form, d, kw, want):
    import flashattention_lab_cuda as ext

    finite(*ext.fp8_varlen_forward(f8(B, HQ, d), f8(97, HKV, d, seed=1), f8(97, HKV, d, seed=2), i32(0, 1, 2), i32(0, 64, 97), 1, CAP, False, None,
                                   **kw))
    assert routes == want
