"""GPU: which C entry point, and which workspace-size function, every form of the fp8 / MXFP4 shim calls reaches
(flashattention_lab_cuda: fp8_forward, fp8_varlen_forward, fp8_kvcache_forward, fp8_kvcache_step, fp4_kvcache_forward,
fp4_varlen_forward; DESIGN.md, the host boundary).  "Launch for launch the parent's call" is a promise of these families: a call with
no feature goes through its parent's entry point, a featured one through _mod, hdim=True through _hdim, packed queries through
_varlen, the padded step at 128 through fa_fp8_kvcache_step.  ext._call and the library's *_workspace_bytes functions are wrapped by
recorders that note the name and delegate, so every call below launches; the shapes are the smallest that do: B 2, H_q 4 / H_kv 2,
Nq 1, 64 cached keys, contiguous caches, bf16 out.  The outputs' values are other files' business; here they must be finite."""
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
