"""The row-filter entry points of the C ABI: declared in include/imagescry_hip.h, exported by the built library, bound in
the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_row_mask_words", "isc_row_mask_pack", "isc_cosine_topk_masked", "isc_cosine_topk_exhaustive_masked",
         "isc_cosine_range_masked")


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_filter_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    # each masked search is its twin's argument list plus the bitmap, in front of the stream
    for name in ("isc_cosine_topk", "isc_cosine_topk_exhaustive", "isc_cosine_range"):
        twin, masked = _prototype(name), _prototype(name + "_masked")
        assert masked == twin[:-1] + ["const uint32_t* row_mask", "void* stream"]
    assert _prototype("isc_row_mask_pack") == ["const uint8_t* allow", "int64_t N", "uint32_t* packed_mask",
                                               "int64_t* allowed_count", "void* stream"]


def test_filter_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    assert lib.isc_abi_version() == 4
    words = ctypes.c_size_t()
    for n, want in ((1, 8), (256, 8), (257, 16), (10_000_000, 39_063 * 8)):
        assert lib.isc_row_mask_words(n, words) == _lib.ISC_OK and words.value == want
    assert lib.isc_row_mask_words(0, words) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_mask_words(-5, words) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_mask_words(1 << 31, words) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_mask_words(100, None) == _lib.ISC_ERR_INVALID_ARG
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks before a launch
    assert lib.isc_row_mask_pack(None, 100, fake, None, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_mask_pack(fake, 100, None, None, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_mask_pack(fake, 0, fake, None, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_row_mask_pack(fake, 100, ctypes.c_void_p(0x1002), None, None) == _lib.ISC_ERR_ALIGNMENT
    # a NULL bitmap is an error, not "no filter"
    ws = ctypes.c_size_t(1 << 20)
    st = lib.isc_cosine_topk_masked(fake, _lib.ISC_F16, 1000, 64, fake, _lib.ISC_F16, 4, 64, 10, 0, None, fake, fake,
                                    fake, fake, ws.value, None, None)
    assert st == _lib.ISC_ERR_INVALID_ARG
    st = lib.isc_cosine_topk_exhaustive_masked(fake, _lib.ISC_F16, 1000, 64, fake, _lib.ISC_F16, 4, 64, 10, 0, fake, fake,
                                               fake, ws.value, None, None)
    assert st == _lib.ISC_ERR_INVALID_ARG
    st = lib.isc_cosine_range_masked(fake, _lib.ISC_F16, 1000, 64, fake, _lib.ISC_F16, 4, 64, fake, 0, None, 100, fake,
                                     fake, fake, fake, fake, fake, ws.value, None, None)
    assert st == _lib.ISC_ERR_INVALID_ARG
    # the masked calls keep their twins' other checks (k > N, bad dtype)
    st = lib.isc_cosine_topk_masked(fake, _lib.ISC_F16, 5, 64, fake, _lib.ISC_F16, 4, 64, 10, 0, None, fake, fake, fake,
                                    fake, ws.value, fake, None)
    assert st == _lib.ISC_ERR_INVALID_ARG
    st = lib.isc_cosine_range_masked(fake, _lib.ISC_U8, 1000, 64, fake, _lib.ISC_F16, 4, 64, fake, 0, None, 100, fake,
                                     fake, fake, fake, fake, fake, ws.value, fake, None)
    assert st == _lib.ISC_ERR_INVALID_ARG
