"""The append entry points of the C ABI (isc_bank_append, isc_bank_repack): declared in include/imagescry_hip.h, exported by
the built library, bound in the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_bank_append", "isc_bank_repack")


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_append_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    # isc_bank_append is isc_bank_pack's argument list (n_total named capacity) plus the fill bitmap and the group codes
    pack, append = _prototype("isc_bank_pack"), _prototype("isc_bank_append")
    assert append == pack[:6] + ["int64_t capacity"] + pack[7:-1] + [
        "uint32_t* fill_mask", "const int32_t* codes", "int32_t* packed_codes", "void* stream"]
    assert _prototype("isc_bank_repack") == [
        "const void* src_packed", "int64_t src_capacity", "void* dst_packed", "int64_t dst_capacity", "int dtype", "int D",
        "int64_t first_row", "int64_t n_rows", "const int32_t* src_codes", "int32_t* dst_codes", "uint32_t* dst_fill_mask",
        "void* stream"]


def test_append_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    assert lib.isc_abi_version() == 4
    F16, F32 = _lib.ISC_F16, _lib.ISC_F32
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks before a launch
    odd4, odd16 = ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004)

    def append(rows=fake, in_dtype=F32, n=10, d=64, ldx=64, first=0, cap=100, packed=fake, dtype=F16, nb=fake, fill=fake,
               codes=None, pcodes=None):
        return lib.isc_bank_append(rows, in_dtype, n, d, ldx, first, cap, 1, 1e-12, packed, dtype, nb, fill, codes, pcodes,
                                   None)

    assert append(rows=None) == _lib.ISC_ERR_INVALID_ARG
    assert append(packed=None) == _lib.ISC_ERR_INVALID_ARG
    assert append(fill=None) == _lib.ISC_ERR_INVALID_ARG
    assert append(first=91) == _lib.ISC_ERR_INVALID_ARG  # first_row + n_rows > capacity
    assert append(first=-1) == _lib.ISC_ERR_INVALID_ARG
    assert append(n=0) == _lib.ISC_ERR_INVALID_ARG
    assert append(ldx=63) == _lib.ISC_ERR_INVALID_ARG
    assert append(cap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert append(dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert append(in_dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    # exactly one of codes / packed_codes NULL
    assert append(codes=fake) == _lib.ISC_ERR_INVALID_ARG
    assert append(pcodes=fake) == _lib.ISC_ERR_INVALID_ARG
    assert append(packed=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert append(fill=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert append(codes=fake, pcodes=odd16) == _lib.ISC_ERR_ALIGNMENT

    def repack(src=fake, scap=100, dst=ctypes.c_void_p(0x2000), dcap=200, dtype=F16, d=64, first=0, n=100, scodes=None,
               dcodes=None, fill=fake):
        return lib.isc_bank_repack(src, scap, dst, dcap, dtype, d, first, n, scodes, dcodes, fill, None)

    assert repack(src=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dst=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(fill=None) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dst=fake) == _lib.ISC_ERR_INVALID_ARG  # in place
    assert repack(n=101) == _lib.ISC_ERR_INVALID_ARG  # rows past the source
    assert repack(dcap=99) == _lib.ISC_ERR_INVALID_ARG  # rows past the destination
    assert repack(n=0) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dcap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert repack(scodes=fake) == _lib.ISC_ERR_INVALID_ARG
    assert repack(dcodes=fake) == _lib.ISC_ERR_INVALID_ARG
    assert repack(src=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert repack(dst=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert repack(fill=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert repack(scodes=fake, dcodes=odd16) == _lib.ISC_ERR_ALIGNMENT
