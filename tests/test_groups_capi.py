"""The group-exclusion entry points of the C ABI: declared in include/imagescry_hip.h, exported by the built library, bound
in the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_row_groups_pack", "isc_cosine_topk_grouped", "isc_cosine_topk_exhaustive_grouped", "isc_cosine_range_grouped")
GROUP_ARGS = ["const uint32_t* row_mask", "const int32_t* row_group", "const int32_t* query_group", "void* stream"]


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_group_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    # each grouped search is its unmasked twin's argument list plus the three pointers, in front of the stream
    for name in ("isc_cosine_topk", "isc_cosine_topk_exhaustive", "isc_cosine_range"):
        twin, grouped = _prototype(name), _prototype(name + "_grouped")
        assert grouped == twin[:-1] + GROUP_ARGS
        assert _lib.SIGNATURES[name + "_grouped"][1][:-4] == _lib.SIGNATURES[name][1][:-1]
    assert _prototype("isc_row_groups_pack") == ["const int32_t* codes", "int64_t N", "int32_t* packed_codes",
                                                 "void* stream"]


def test_group_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    assert lib.isc_abi_version() == 4
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks before a launch
    odd = ctypes.c_void_p(0x1002)
    assert lib.isc_row_groups_pack(None, 100, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_groups_pack(fake, 100, None, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_groups_pack(fake, 0, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_groups_pack(fake, 1 << 31, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_groups_pack(fake, 100, ctypes.c_void_p(0x1004), None) == _lib.ISC_ERR_ALIGNMENT
    ws = 1 << 20

    def topk(rm, rg, qg, n=1000, k=10):
        return lib.isc_cosine_topk_grouped(fake, _lib.ISC_F16, n, 64, fake, _lib.ISC_F16, 4, 64, k, 0, None, fake, fake,
                                           fake, fake, ws, rm, rg, qg, None)

    def exhaustive(rm, rg, qg):
        return lib.isc_cosine_topk_exhaustive_grouped(fake, _lib.ISC_F16, 1000, 64, fake, _lib.ISC_F16, 4, 64, 10, 0,
                                                      fake, fake, fake, ws, rm, rg, qg, None)

    def rng(rm, rg, qg, dtype=_lib.ISC_F16):
        return lib.isc_cosine_range_grouped(fake, dtype, 1000, 64, fake, _lib.ISC_F16, 4, 64, fake, 0, None, 100, fake,
                                            fake, fake, fake, fake, fake, ws, rm, rg, qg, None)

    for call in (topk, exhaustive, rng):
        assert call(None, None, fake) == _lib.ISC_ERR_INVALID_ARG  # row codes are required
        assert call(None, fake, None) == _lib.ISC_ERR_INVALID_ARG  # ... and query codes
        assert call(None, odd, fake) == _lib.ISC_ERR_ALIGNMENT  # row codes: 16-byte vector loads
        assert call(None, fake, odd) == _lib.ISC_ERR_ALIGNMENT
        assert call(odd, fake, fake) == _lib.ISC_ERR_ALIGNMENT
    # the grouped calls keep their twins' other checks (k > N, bad dtype)
    assert topk(None, fake, fake, n=5, k=10) == _lib.ISC_ERR_INVALID_ARG
    assert rng(None, fake, fake, dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
