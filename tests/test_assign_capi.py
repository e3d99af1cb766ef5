"""The assign / group-sums entry points of the C ABI (isc_bank_assign, isc_bank_assign_exhaustive, isc_bank_group_sums and
their workspace sizing): declared in include/imagescry_hip.h, exported by the built library, bound in the ctypes table; the
workspace sizes and the host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_bank_assign_workspace_bytes", "isc_bank_assign", "isc_bank_assign_exhaustive",
         "isc_bank_group_sums_workspace_bytes", "isc_bank_group_sums")
F16, F32, U8 = _lib.ISC_F16, _lib.ISC_F32, _lib.ISC_U8
INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = (_lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_WORKSPACE,
                                              _lib.ISC_ERR_ALIGNMENT)


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_assign_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    fast = _prototype("isc_bank_assign")
    assert fast == [
        "const void* bank", "int dtype", "int64_t N", "int D", "const void* centroids", "int c_dtype", "int C",
        "int64_t ldc", "const float* norm_bound", "const uint32_t* row_mask", "int32_t* out_labels", "float* out_scores",
        "int32_t* status", "void* workspace", "size_t workspace_bytes", "void* stream"]
    # the exhaustive call: the same arguments without norm_bound
    assert _prototype("isc_bank_assign_exhaustive") == [p for p in fast if p != "const float* norm_bound"]
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4


def test_workspace_sizing() -> None:
    lib = _lib.load()
    need = ctypes.c_size_t()

    def size(dtype=F16, n=100_000, d=768, c=256):
        assert lib.isc_bank_assign_workspace_bytes(dtype, n, d, c, need) == 0
        return need.value

    # monotone in N
    sizes = [size(n=n) for n in (0, 1, 255, 256, 257, 10_000, 1_000_000, 10_000_000)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # per row: a count, four candidates with their filter scores, the redo byte and a score between passes
    assert size(n=10_000_000) < 10_000_000 * 48 + (1 << 21)
    # depends on min(C, 1024): every call with more centroids runs as passes over the workspace of 1024
    assert size(c=1024) == size(c=1025) == size(c=70_000) == size(c=1 << 24)
    assert size(c=17) <= size(c=64) <= size(c=65) <= size(c=1024)
    assert size(c=64) < size(c=1024)
    assert size(c=0) <= size(c=1)
    # limits and invalid arguments
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, _lib.ISC_SEARCH_MAX_D, 4, need) == 0
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, _lib.ISC_SEARCH_MAX_D + 1, 4, need) == UNSUPPORTED
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, 64, (1 << 24) + 1, need) == UNSUPPORTED
    assert lib.isc_bank_assign_workspace_bytes(U8, 1000, 64, 4, need) == INVALID
    assert lib.isc_bank_assign_workspace_bytes(F16, -1, 64, 4, need) == INVALID
    assert lib.isc_bank_assign_workspace_bytes(F16, 2**31 - 1, 64, 4, need) == INVALID
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, 0, 4, need) == INVALID
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, 64, -1, need) == INVALID
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, 64, 4, None) == INVALID
    # group sums: two partial rows per chunk of 1024 list entries, columns padded to 256
    assert lib.isc_bank_group_sums_workspace_bytes(F16, 1024, 768, need) == 0
    one = need.value
    assert lib.isc_bank_group_sums_workspace_bytes(F16, 1025, 768, need) == 0
    assert need.value > one >= 2 * 768 * 8
    assert lib.isc_bank_group_sums_workspace_bytes(F16, 1 << 20, 768, need) == 0
    assert need.value == 1024 * 2 * 768 * 8 + 1024 * 2 * 8
    assert lib.isc_bank_group_sums_workspace_bytes(F16, 10, _lib.ISC_SEARCH_MAX_D + 1, need) == UNSUPPORTED
    assert lib.isc_bank_group_sums_workspace_bytes(F16, -1, 64, need) == INVALID
    assert lib.isc_bank_group_sums_workspace_bytes(U8, 10, 64, need) == INVALID
    assert lib.isc_bank_group_sums_workspace_bytes(F16, 10, 64, None) == INVALID


def test_assign_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)  # never dereferenced: every call below ends before a launch
    odd2, odd4 = ctypes.c_void_p(0x10001), ctypes.c_void_p(0x10002)
    need = ctypes.c_size_t()
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, 64, 8, need) == 0

    def assign(bank=fake, dtype=F16, n=1000, d=64, cent=fake, c_dtype=F32, c=8, ldc=64, nb=fake, mask=None, labels=fake,
               scores=fake, status=fake, ws=fake, ws_bytes=None, exhaustive=False):
        ws_bytes = need.value if ws_bytes is None else ws_bytes
        if exhaustive:
            return lib.isc_bank_assign_exhaustive(bank, dtype, n, d, cent, c_dtype, c, ldc, mask, labels, scores, status,
                                                  ws, ws_bytes, None)
        return lib.isc_bank_assign(bank, dtype, n, d, cent, c_dtype, c, ldc, nb, mask, labels, scores, status, ws, ws_bytes,
                                   None)

    for ex in (False, True):
        assert assign(bank=None, exhaustive=ex) == INVALID
        assert assign(cent=None, exhaustive=ex) == INVALID
        assert assign(labels=None, exhaustive=ex) == INVALID
        assert assign(status=None, exhaustive=ex) == INVALID
        assert assign(dtype=U8, exhaustive=ex) == INVALID
        assert assign(c_dtype=U8, exhaustive=ex) == INVALID
        assert assign(n=-1, exhaustive=ex) == INVALID
        assert assign(n=2**31 - 1, exhaustive=ex) == INVALID
        assert assign(d=0, exhaustive=ex) == INVALID
        assert assign(c=-1, exhaustive=ex) == INVALID
        assert assign(ldc=63, exhaustive=ex) == INVALID
        assert assign(d=_lib.ISC_SEARCH_MAX_D + 1, ldc=10_000, exhaustive=ex) == UNSUPPORTED
        assert assign(c=(1 << 24) + 1, exhaustive=ex) == UNSUPPORTED
        assert assign(bank=odd4, exhaustive=ex) == ALIGNMENT
        assert assign(cent=odd2, exhaustive=ex) == ALIGNMENT
        assert assign(cent=odd2, c_dtype=F16, exhaustive=ex) == ALIGNMENT
        assert assign(mask=odd4, exhaustive=ex) == ALIGNMENT
        assert assign(labels=odd4, exhaustive=ex) == ALIGNMENT
        assert assign(scores=odd4, exhaustive=ex) == ALIGNMENT
        assert assign(status=odd4, exhaustive=ex) == ALIGNMENT
        # nothing to do: ISC_OK without a launch, whatever the pointers
        assert assign(c=0, bank=None, cent=None, labels=None, status=None, ws=None, exhaustive=ex) == 0
        assert assign(n=0, bank=None, cent=None, labels=None, status=None, ws=None, exhaustive=ex) == 0
    assert assign(ws=None) == INVALID
    assert assign(ws=ctypes.c_void_p(0x10010)) == ALIGNMENT
    assert assign(nb=odd4) == ALIGNMENT
    assert assign(ws_bytes=need.value - 1) == WORKSPACE
    assert assign(ws_bytes=0) == WORKSPACE
    # a workspace sized for fewer centroids of the pass is too small
    small = ctypes.c_size_t()
    assert lib.isc_bank_assign_workspace_bytes(F16, 1000, 64, 8, small) == 0
    assert assign(c=1024, ws_bytes=small.value) == WORKSPACE


def test_group_sums_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)
    odd = ctypes.c_void_p(0x10004)
    need = ctypes.c_size_t()
    assert lib.isc_bank_group_sums_workspace_bytes(F16, 500, 64, need) == 0

    def sums(bank=fake, dtype=F16, n=1000, d=64, rows=fake, m=500, offsets=fake, g=4, fill=None, out=fake, ld=64,
             counts=fake, ws=fake, ws_bytes=None):
        return lib.isc_bank_group_sums(bank, dtype, n, d, rows, m, offsets, g, fill, out, ld, counts, ws,
                                       need.value if ws_bytes is None else ws_bytes, None)

    assert sums(bank=None) == INVALID
    assert sums(rows=None) == INVALID
    assert sums(offsets=None) == INVALID
    assert sums(out=None) == INVALID
    assert sums(counts=None) == INVALID
    assert sums(ws=None) == INVALID
    assert sums(dtype=U8) == INVALID
    assert sums(n=0) == INVALID
    assert sums(n=2**31 - 1) == INVALID
    assert sums(d=0) == INVALID
    assert sums(m=-1) == INVALID
    assert sums(g=-1) == INVALID
    assert sums(ld=63) == INVALID
    assert sums(d=_lib.ISC_SEARCH_MAX_D + 1, ld=10_000) == UNSUPPORTED
    assert sums(g=2**31) == UNSUPPORTED
    assert sums(rows=odd) == ALIGNMENT
    assert sums(offsets=odd) == ALIGNMENT
    assert sums(out=odd) == ALIGNMENT
    assert sums(counts=odd) == ALIGNMENT
    assert sums(fill=ctypes.c_void_p(0x10002)) == ALIGNMENT
    assert sums(ws=ctypes.c_void_p(0x10010)) == ALIGNMENT
    assert sums(ws_bytes=need.value - 1) == WORKSPACE
    assert sums(g=0, bank=None, rows=None, offsets=None, out=None, counts=None, ws=None) == 0
