"""The farthest-point entry points of the C ABI (isc_bank_farthest and its workspace sizing): declared in
include/imagescry_hip.h, exported by the built library, bound in the ctypes table; the workspace size and the host-side
argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
F16, F32, U8 = _lib.ISC_F16, _lib.ISC_F32, _lib.ISC_U8
INVALID, UNSUPPORTED, WORKSPACE, ALIGNMENT = (_lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_WORKSPACE,
                                              _lib.ISC_ERR_ALIGNMENT)


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_farthest_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("isc_bank_farthest_workspace_bytes", "isc_bank_farthest"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(_prototype(name))
    assert _prototype("isc_bank_farthest") == [
        "const void* bank", "int dtype", "int64_t N", "int D", "const int64_t* start", "int64_t S", "int64_t M",
        "const uint32_t* fill_mask", "const uint32_t* row_mask", "int64_t* out_rows", "float* out_cover", "float* out_near",
        "void* workspace", "size_t workspace_bytes", "void* stream"]
    assert _prototype("isc_bank_farthest_workspace_bytes") == ["int dtype", "int64_t N", "int D", "size_t* bytes"]
    assert re.search(r"#define ISC_FARTHEST_MAX_PICKS \(1 << 20\)", HEADER.read_text())
    assert _lib.ISC_FARTHEST_MAX_PICKS == 1 << 20
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4


def test_workspace_sizing() -> None:
    lib = _lib.load()
    need = ctypes.c_size_t()

    def size(dtype=F16, n=100_000, d=768):
        assert lib.isc_bank_farthest_workspace_bytes(dtype, n, d, need) == 0
        return need.value

    sizes = [size(n=n) for n in (0, 1, 255, 256, 257, 10_000, 1_000_000, 10_000_000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # per row a float32 `near` and a candidate byte; two buffers of per-workgroup keys
    assert size(n=10_000_000) < 10_000_000 * 5 + (1 << 16)
    assert size(dtype=F32) == size(dtype=F16) and size(d=8) == size(d=_lib.ISC_SEARCH_MAX_D)
    assert lib.isc_bank_farthest_workspace_bytes(F16, 1000, _lib.ISC_SEARCH_MAX_D + 1, need) == UNSUPPORTED
    assert lib.isc_bank_farthest_workspace_bytes(U8, 1000, 64, need) == INVALID
    assert lib.isc_bank_farthest_workspace_bytes(F16, -1, 64, need) == INVALID
    assert lib.isc_bank_farthest_workspace_bytes(F16, 2**31 - 1, 64, need) == INVALID
    assert lib.isc_bank_farthest_workspace_bytes(F16, 1000, 0, need) == INVALID
    assert lib.isc_bank_farthest_workspace_bytes(F16, 1000, 64, None) == INVALID


def test_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)  # never dereferenced: every call below ends before a launch
    odd4 = ctypes.c_void_p(0x10002)
    need = ctypes.c_size_t()
    assert lib.isc_bank_farthest_workspace_bytes(F16, 1000, 64, need) == 0

    def far(bank=fake, dtype=F16, n=1000, d=64, start=fake, s=2, m=8, fill=None, mask=None, rows=fake, cover=fake,
            near=None, ws=fake, ws_bytes=None):
        return lib.isc_bank_farthest(bank, dtype, n, d, start, s, m, fill, mask, rows, cover, near, ws,
                                     need.value if ws_bytes is None else ws_bytes, None)

    assert far(dtype=U8) == INVALID
    assert far(n=-1) == INVALID
    assert far(n=0) == INVALID  # picks were asked of an image laid out for no row
    assert far(n=2**31 - 1) == INVALID
    assert far(d=0) == INVALID
    assert far(s=-1) == INVALID
    assert far(m=-1) == INVALID
    assert far(bank=None) == INVALID
    assert far(rows=None) == INVALID
    assert far(cover=None) == INVALID
    assert far(ws=None) == INVALID
    assert far(start=None) == INVALID  # S > 0 rows were announced
    assert far(d=_lib.ISC_SEARCH_MAX_D + 1) == UNSUPPORTED
    assert far(m=_lib.ISC_FARTHEST_MAX_PICKS + 1) == UNSUPPORTED
    assert far(bank=odd4) == ALIGNMENT
    assert far(start=ctypes.c_void_p(0x10004)) == ALIGNMENT
    assert far(fill=odd4) == ALIGNMENT
    assert far(mask=odd4) == ALIGNMENT
    assert far(rows=ctypes.c_void_p(0x10004)) == ALIGNMENT
    assert far(cover=odd4) == ALIGNMENT
    assert far(near=odd4) == ALIGNMENT
    assert far(ws=ctypes.c_void_p(0x10010)) == ALIGNMENT
    assert far(ws_bytes=need.value - 1) == WORKSPACE
    assert far(ws_bytes=0) == WORKSPACE
    big = ctypes.c_size_t()
    assert lib.isc_bank_farthest_workspace_bytes(F16, 100_000, 64, big) == 0
    assert far(n=100_000, ws_bytes=need.value) == WORKSPACE and big.value > need.value
    # nothing to pick: ISC_OK without a launch, whatever the pointers
    assert far(m=0, bank=None, start=None, s=0, rows=None, cover=None, ws=None, ws_bytes=0) == 0
    assert far(m=0, n=0, bank=None, start=None, s=0, rows=None, cover=None, ws=None, ws_bytes=0) == 0
