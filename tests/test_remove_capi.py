"""The remove / replace / compact entry points of the C ABI (isc_bank_remove, isc_bank_replace, isc_bank_repack_map,
isc_row_mask_unpack): declared in include/imagescry_hip.h, exported by the built library, bound in the ctypes table, and
their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_bank_remove", "isc_bank_replace", "isc_bank_repack_map", "isc_row_mask_unpack")


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_remove_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    assert _prototype("isc_bank_remove") == [
        "const int64_t* rows", "int64_t n_rows", "int64_t n_filled", "int64_t capacity", "uint32_t* fill_mask",
        "int32_t* packed_codes", "int64_t* group_counts", "int64_t* removed_count", "void* stream"]
    assert _prototype("isc_bank_replace") == [
        "const void* rows", "int in_dtype", "int64_t n_rows", "int D", "int64_t ldx", "const int64_t* row_index",
        "int64_t capacity", "int normalize", "float eps", "void* packed", "int dtype", "float* norm_bound",
        "const uint32_t* fill_mask", "void* stream"]
    # isc_bank_repack's argument list plus the index map
    repack = _prototype("isc_bank_repack")
    assert _prototype("isc_bank_repack_map") == repack[:-1] + ["const int64_t* new_index", "void* stream"]
    assert _prototype("isc_row_mask_unpack") == [
        "const uint32_t* packed_mask", "int64_t N", "int64_t n_rows", "uint8_t* allow", "void* stream"]


def test_the_abi_version_stays_4() -> None:
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4


def test_remove_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks before a launch
    odd4, odd8, odd16 = ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)

    def remove(rows=fake, n=10, filled=50, cap=100, fill=fake, codes=None, counts=None, removed=None):
        return lib.isc_bank_remove(rows, n, filled, cap, fill, codes, counts, removed, None)

    assert remove(rows=None) == _lib.ISC_ERR_INVALID_ARG
    assert remove(fill=None) == _lib.ISC_ERR_INVALID_ARG
    assert remove(n=0) == _lib.ISC_ERR_INVALID_ARG
    assert remove(n=-1) == _lib.ISC_ERR_INVALID_ARG
    assert remove(filled=-1) == _lib.ISC_ERR_INVALID_ARG
    assert remove(filled=101) == _lib.ISC_ERR_INVALID_ARG  # n_filled > capacity
    assert remove(cap=0, filled=0) == _lib.ISC_ERR_INVALID_ARG
    assert remove(cap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert remove(counts=fake) == _lib.ISC_ERR_INVALID_ARG  # group counts without the codes they are indexed by
    assert remove(rows=odd8) == _lib.ISC_ERR_ALIGNMENT
    assert remove(fill=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert remove(codes=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert remove(codes=fake, counts=odd8) == _lib.ISC_ERR_ALIGNMENT
    assert remove(removed=odd8) == _lib.ISC_ERR_ALIGNMENT


def test_replace_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    F16, F32 = _lib.ISC_F16, _lib.ISC_F32
    fake = ctypes.c_void_p(0x1000)
    odd4, odd8, odd16 = ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)

    def replace(rows=fake, in_dtype=F32, n=10, d=64, ldx=64, index=fake, cap=100, packed=fake, dtype=F16, nb=fake,
                fill=fake):
        return lib.isc_bank_replace(rows, in_dtype, n, d, ldx, index, cap, 1, 1e-12, packed, dtype, nb, fill, None)

    assert replace(rows=None) == _lib.ISC_ERR_INVALID_ARG
    assert replace(index=None) == _lib.ISC_ERR_INVALID_ARG
    assert replace(packed=None) == _lib.ISC_ERR_INVALID_ARG
    assert replace(n=0) == _lib.ISC_ERR_INVALID_ARG
    assert replace(d=0) == _lib.ISC_ERR_INVALID_ARG
    assert replace(ldx=63) == _lib.ISC_ERR_INVALID_ARG
    assert replace(cap=0) == _lib.ISC_ERR_INVALID_ARG
    assert replace(cap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert replace(dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert replace(in_dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert replace(packed=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert replace(index=odd8) == _lib.ISC_ERR_ALIGNMENT
    assert replace(fill=odd4) == _lib.ISC_ERR_ALIGNMENT


def test_repack_map_and_mask_unpack_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    F16 = _lib.ISC_F16
    fake = ctypes.c_void_p(0x1000)
    odd4, odd8, odd16 = ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1008)

    def repack(src=fake, scap=100, dst=ctypes.c_void_p(0x2000), dcap=100, dtype=F16, d=64, first=0, n=100, scodes=None,
               dcodes=None, fill=fake, index=fake):
        return lib.isc_bank_repack_map(src, scap, dst, dcap, dtype, d, first, n, scodes, dcodes, fill, index, None)

    assert repack(src=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dst=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(fill=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(index=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dst=fake) == _lib.ISC_ERR_INVALID_ARG  # src == dst: in place
    assert repack(n=101) == _lib.ISC_ERR_INVALID_ARG  # rows past the source
    assert repack(n=0) == _lib.ISC_ERR_INVALID_ARG
    assert repack(first=-1) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dcap=0) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dcap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert repack(scap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert repack(scodes=fake) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dcodes=fake) == _lib.ISC_ERR_INVALID_ARG
    assert repack(src=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert repack(dst=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert repack(fill=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert repack(index=odd8) == _lib.ISC_ERR_ALIGNMENT
    assert repack(scodes=fake, dcodes=odd16) == _lib.ISC_ERR_ALIGNMENT

    def unpack(mask=fake, n_total=100, n=50, allow=fake):
        return lib.isc_row_mask_unpack(mask, n_total, n, allow, None)

    assert unpack(mask=None) == _lib.ISC_ERR_INVALID_ARG
    assert unpack(allow=None) == _lib.ISC_ERR_INVALID_ARG
    assert unpack(n=0) == _lib.ISC_ERR_INVALID_ARG
    assert unpack(n=101) == _lib.ISC_ERR_INVALID_ARG  # rows past the bank
    assert unpack(n_total=0) == _lib.ISC_ERR_INVALID_ARG
    assert unpack(n_total=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert unpack(mask=odd4) == _lib.ISC_ERR_ALIGNMENT
