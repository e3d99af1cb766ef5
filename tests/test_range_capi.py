"""The range-search entry points of the C ABI: declared in include/imagescry_hip.h, exported by the built library, bound in
the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_cosine_range_workspace_bytes", "isc_cosine_range")


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_range_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    params = _prototype("isc_cosine_range")
    assert params[:8] == ["const void* bank", "int dtype", "int64_t N", "int D", "const void* queries", "int q_dtype",
                          "int Q", "int64_t ldq"]
    assert "const float* min_score" in params and "int64_t capacity" in params and "int64_t* needed" in params


def test_range_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    assert lib.isc_abi_version() == 4
    need = ctypes.c_size_t()
    ws = lib.isc_cosine_range_workspace_bytes
    assert ws(_lib.ISC_U8, 1000, 64, 4, 100, need) == _lib.ISC_ERR_INVALID_ARG
    assert ws(_lib.ISC_F16, 0, 64, 4, 100, need) == _lib.ISC_ERR_INVALID_ARG
    assert ws(_lib.ISC_F16, 1000, 64, 4, 0, need) == _lib.ISC_ERR_INVALID_ARG
    assert ws(_lib.ISC_F16, 1000, _lib.ISC_SEARCH_MAX_D + 1, 4, 100, need) == _lib.ISC_ERR_UNSUPPORTED
    assert ws(_lib.ISC_F16, 1000, 64, 4, 1 << 31, need) == _lib.ISC_ERR_UNSUPPORTED
    assert ws(_lib.ISC_F16, 1000, 64, 4, 100, None) == _lib.ISC_ERR_INVALID_ARG
    # NULL outputs are refused before anything is launched
    st = lib.isc_cosine_range(None, _lib.ISC_F16, 1000, 64, None, _lib.ISC_F16, 4, 64, None, 0, None, 100, None, None,
                              None, None, None, None, 0, None)
    assert st == _lib.ISC_ERR_INVALID_ARG
