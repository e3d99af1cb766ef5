"""The large-k entry points of the C ABI (120 < k <= ISC_TOPK_LARGE_MAX_K): declared in include/imagescry_hip.h, exported by
the built library, bound in the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_cosine_topk_large_workspace_bytes", "isc_cosine_topk_large",
         "isc_cosine_topk_exhaustive_large_workspace_bytes", "isc_cosine_topk_exhaustive_large")
FAKE = 0x10000  # a 256-byte aligned address that is never dereferenced: the checks below fail before any launch


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_large_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    fast, slow = _prototype("isc_cosine_topk_large"), _prototype("isc_cosine_topk_exhaustive_large")
    grouped = _prototype("isc_cosine_topk_grouped")
    assert fast == grouped and len(fast) == 20  # the arguments of the grouped call, the filters optional
    assert slow == [p for p in fast if p not in ("const float* norm_bound", "int32_t* status")] and len(slow) == 18
    assert slow == _prototype("isc_cosine_topk_exhaustive_grouped")
    text = HEADER.read_text()
    assert re.search(r"#define ISC_TOPK_LARGE_MAX_K 4096\b", text) and _lib.ISC_TOPK_LARGE_MAX_K == 4096
    assert re.search(r"#define ISC_TOPK_MAX_K 120\b", text) and _lib.ISC_TOPK_MAX_K == 120


def test_large_workspace_sizes_and_limits() -> None:
    lib = _lib.load()
    need = ctypes.c_size_t()
    for ws in (lib.isc_cosine_topk_large_workspace_bytes, lib.isc_cosine_topk_exhaustive_large_workspace_bytes):
        assert ws(_lib.ISC_F16, 100_000, 64, 4, 4097, need) == _lib.ISC_ERR_UNSUPPORTED
        assert ws(_lib.ISC_F16, 100_000, 64, 4, 4096, need) == _lib.ISC_OK
        assert ws(_lib.ISC_F16, 100_000, 64, 4, 121, need) == _lib.ISC_OK
        assert ws(_lib.ISC_F16, 100_000, 64, 4, 1, need) == _lib.ISC_OK  # (small k is served too; the binding does not use it)
        assert ws(_lib.ISC_F16, 100_000, 64, 4, 0, need) == _lib.ISC_ERR_INVALID_ARG
        assert ws(_lib.ISC_F16, 100_000, 64, 4, -3, need) == _lib.ISC_ERR_INVALID_ARG
        assert ws(_lib.ISC_F16, 500, 64, 4, 501, need) == _lib.ISC_ERR_INVALID_ARG  # k > N
        assert ws(_lib.ISC_F16, 500, 64, 4, 500, need) == _lib.ISC_OK
        assert ws(_lib.ISC_U8, 1000, 64, 4, 200, need) == _lib.ISC_ERR_INVALID_ARG
        assert ws(_lib.ISC_F16, 0, 64, 4, 200, need) == _lib.ISC_ERR_INVALID_ARG
        assert ws(_lib.ISC_F16, 1000, 64, 0, 200, need) == _lib.ISC_ERR_INVALID_ARG
        assert ws(_lib.ISC_F16, 1000, _lib.ISC_SEARCH_MAX_D + 1, 4, 200, need) == _lib.ISC_ERR_UNSUPPORTED
        assert ws(_lib.ISC_F16, 1000, _lib.ISC_SEARCH_MAX_D, 4, 200, need) == _lib.ISC_OK
        assert ws(_lib.ISC_F16, 1000, 64, 4, 200, None) == _lib.ISC_ERR_INVALID_ARG
        # the size does not grow with N, nor with Q beyond one pass; it is O(queries per pass x k)
        small, big, many = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert ws(_lib.ISC_F16, 10_000, 768, 1024, 4096, small) == 0 and ws(_lib.ISC_F16, 100_000_000, 768, 1024, 4096, big) == 0
        assert ws(_lib.ISC_F16, 10_000, 768, 1 << 20, 4096, many) == 0
        assert small.value == big.value == many.value < 160e6
        assert ws(_lib.ISC_F16, 10_000, 768, 1024, 121, need) == 0 and need.value < 64e6
    # the existing entry points keep their limit
    assert lib.isc_cosine_topk_workspace_bytes(_lib.ISC_F32, 500, 32, 4, 121, need) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_cosine_topk_exhaustive_workspace_bytes(_lib.ISC_F32, 500, 32, 4, 121, need) == _lib.ISC_ERR_UNSUPPORTED


def _fast(lib, *, bank=FAKE, n=1000, d=64, q=FAKE, q_dtype=_lib.ISC_F16, nq=4, ldq=64, k=200, out_s=FAKE, out_i=FAKE,
          status=FAKE, ws=FAKE, ws_bytes=1 << 40, mask=None, row_group=None, query_group=None) -> int:
    return lib.isc_cosine_topk_large(bank, _lib.ISC_F16, n, d, q, q_dtype, nq, ldq, k, 0, None, out_s, out_i, status, ws,
                                     ws_bytes, mask, row_group, query_group, None)


def _slow(lib, *, bank=FAKE, n=1000, d=64, q=FAKE, q_dtype=_lib.ISC_F16, nq=4, ldq=64, k=200, out_s=FAKE, out_i=FAKE,
          ws=FAKE, ws_bytes=1 << 40, mask=None, row_group=None, query_group=None, status=None) -> int:
    del status
    return lib.isc_cosine_topk_exhaustive_large(bank, _lib.ISC_F16, n, d, q, q_dtype, nq, ldq, k, 0, out_s, out_i, ws,
                                                ws_bytes, mask, row_group, query_group, None)


def test_large_argument_checks_match_the_sibling_calls() -> None:
    """NULL pointers, limits, alignment and the workspace size are refused, in that order, before anything is launched -- the
    statuses isc_cosine_topk_grouped / isc_cosine_range give for the same mistakes."""
    lib = _lib.load()
    need = ctypes.c_size_t()
    for call, sizer in ((_fast, lib.isc_cosine_topk_large_workspace_bytes),
                        (_slow, lib.isc_cosine_topk_exhaustive_large_workspace_bytes)):
        for null in ("bank", "q", "out_s", "out_i"):
            assert call(lib, **{null: None}) == _lib.ISC_ERR_INVALID_ARG, null
        assert call(lib, q_dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
        assert call(lib, k=4097, n=100_000) == _lib.ISC_ERR_UNSUPPORTED
        assert call(lib, k=0) == _lib.ISC_ERR_INVALID_ARG
        assert call(lib, k=1001) == _lib.ISC_ERR_INVALID_ARG
        assert call(lib, ldq=63) == _lib.ISC_ERR_INVALID_ARG
        assert call(lib, row_group=FAKE) == _lib.ISC_ERR_INVALID_ARG  # the row codes and the query codes come together
        assert call(lib, query_group=FAKE) == _lib.ISC_ERR_INVALID_ARG
        assert call(lib, bank=FAKE + 8) == _lib.ISC_ERR_ALIGNMENT
        assert call(lib, ws=FAKE + 128) == _lib.ISC_ERR_ALIGNMENT
        assert call(lib, mask=FAKE + 2) == _lib.ISC_ERR_ALIGNMENT
        assert call(lib, row_group=FAKE + 4, query_group=FAKE) == _lib.ISC_ERR_ALIGNMENT
        assert call(lib, row_group=FAKE, query_group=FAKE + 2) == _lib.ISC_ERR_ALIGNMENT
        assert sizer(_lib.ISC_F16, 1000, 64, 4, 200, need) == 0
        assert call(lib, ws_bytes=need.value - 1) == _lib.ISC_ERR_WORKSPACE
        assert call(lib, ws=None) == _lib.ISC_ERR_WORKSPACE
    assert _fast(lib, status=None) == _lib.ISC_ERR_INVALID_ARG
