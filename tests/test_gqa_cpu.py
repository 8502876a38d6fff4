"""CPU: the grouped-query attention entry points (include/fa_mi355x.h, fa_ex_*_grouped) — declared, exported, argument
validation and workspace sizes, all before any HIP call."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")
GROUPED = ("fa_ex_forward_grouped", "fa_ex_backward_grouped", "fa_ex_backward_workspace_bytes_grouped",
           "fa_ex_backward_workspace_bytes_fast_grouped")
INVALID_ARGUMENT = -1


def test_header_declares_and_library_exports_the_grouped_symbols():
    import flashattention_lab_cuda as ext

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(ext.LIBRARY_PATH)
    for name in GROUPED:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in ext.EXPORTED_C_SYMBOLS


def _fwd(lib, bh, g):
    return lib.fa_ex_forward_grouped(None, None, None, None, None, bh, g, 64, 64, 128, 2, 0, 0.125, None, 0, None, 128, 128, 0.0, 0,
                                     None)


def _bwd(lib, bh, g):
    return lib.fa_ex_backward_grouped(None, None, None, None, None, None, None, None, None, bh, g, 64, 64, 128, 2, 0, 0.125, None, 0,
                                      None, 128, 128, 0.0, 0, None, 0, None)


def test_kv_group_must_divide_bh_and_be_positive():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for bh, g in ((6, 4), (8, 3), (4, 0), (4, -1), (4, -4)):
        for call in (_fwd, _bwd):
            assert call(lib, bh, g) == INVALID_ARGUMENT, (call.__name__, bh, g)
            assert b"kv_group" in lib.fa_last_error()
    # a valid group gets past the group check to the null-pointer check
    for call in (_fwd, _bwd):
        assert call(lib, 8, 4) == INVALID_ARGUMENT and b"null" in lib.fa_last_error()
        assert call(lib, 8, 8) == INVALID_ARGUMENT and b"null" in lib.fa_last_error()   # MQA
    # the ungrouped calls are the grouped ones with kv_group = 1
    assert lib.fa_ex_forward(None, None, None, None, None, 8, 64, 64, 128, 2, 0, 0.125, None, 0, None, 128, 128, 0.0, 0, None) == INVALID_ARGUMENT
    assert b"fa_ex_forward: null" in lib.fa_last_error()


def _slabs(bh, nk, d, es):
    return 2 * ((bh * nk * d * es + 255) // 256 * 256)


def test_grouped_workspace_is_the_ungrouped_one_plus_the_partial_slabs():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    for bh, nq, nk, d, dtype in ((32, 4096, 4096, 128, 2), (24, 256, 256, 128, 1), (8, 100, 37, 40, 2), (6, 33, 65, 36, 0),
                                 (256, 4096, 4096, 128, 2), (64, 1024, 1536, 128, 2)):
        es = 4 if dtype == 0 else 2
        small = lib.fa_ex_backward_workspace_bytes(bh, nq, nk, d, dtype)
        assert lib.fa_ex_backward_workspace_bytes_grouped(bh, 1, nq, nk, d, dtype) == small
        for causal in (0, 1):
            for extras in (0, 1):
                assert (lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, 1, nq, nk, d, dtype, causal, extras) ==
                        lib.fa_ex_backward_workspace_bytes_fast(bh, nq, nk, d, dtype, causal, extras))
        for g in (2, 4, 8):
            if bh % g:
                continue
            assert lib.fa_ex_backward_workspace_bytes_grouped(bh, g, nq, nk, d, dtype) == small + _slabs(bh, nk, d, es)
            # _fast: the dS room of the ungrouped rule on top, where the chunk of whole groups holds the same units
            fast = lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, g, nq, nk, d, dtype, 1, 1)
            assert fast == small + _slabs(bh, nk, d, es)                       # extras: no hand-over
    # ragged sizes: 256-byte rounding of each slab
    assert lib.fa_ex_backward_workspace_bytes_grouped(4, 2, 3, 5, 8, 2) == lib.fa_ex_backward_workspace_bytes(4, 3, 5, 8, 2) + 2 * 512   # 320 -> 512
    # an empty side needs no partials
    assert lib.fa_ex_backward_workspace_bytes_grouped(8, 4, 0, 64, 128, 2) == lib.fa_ex_backward_workspace_bytes(8, 0, 64, 128, 2)
    assert lib.fa_ex_backward_workspace_bytes_grouped(8, 4, 64, 0, 128, 2) == lib.fa_ex_backward_workspace_bytes(8, 64, 0, 128, 2)


def test_grouped_ds_room_is_sized_for_chunks_of_whole_groups():
    import flashattention_lab_cuda as ext

    lib = ext._lib
    bh, n, d = 24, 256, 128
    per_unit = (n // 32) * 8 * 2048                                     # 128 KiB of dS tiles per (b,h) unit
    small = lib.fa_ex_backward_workspace_bytes(bh, n, n, d, 2)
    slabs = _slabs(bh, n, d, 2)
    ext.set_option("ds_chunk_mb", 1)                                    # 8 units fit: chunks of 8 ungrouped
    try:
        assert lib.fa_ex_backward_workspace_bytes_fast(bh, n, n, d, 2, 0, 0) == small + 8 * per_unit
        assert lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, 3, n, n, d, 2, 0, 0) == small + slabs + 6 * per_unit   # 8 -> 6
        assert lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, 2, n, n, d, 2, 0, 0) == small + slabs + 8 * per_unit
        assert lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, 12, n, n, d, 2, 0, 0) == small + slabs + 12 * per_unit  # >= g
    finally:
        ext.set_option("ds_chunk_mb", 0)
    assert lib.fa_ex_backward_workspace_bytes_fast_grouped(bh, 3, n, n, d, 2, 0, 0) == small + slabs + bh * per_unit
