"""The host side of isc_trace_regions, which needs no GPU: the entry points are declared, exported and bound, the geometry
and workspace calls answer, and every argument error and limit is returned before anything is launched -- so the pointers
here are made-up addresses that nothing may touch."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest

from imagescry_amd import _lib, build, segmentation

P = 0x10000  # a made-up, well aligned device address
HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_trace_regions", "isc_trace_regions_workspace_bytes", "isc_trace_regions_geometry")
ARGS = ("ids", "B", "H", "W", "R", "connectivity", "N", "V", "vertices", "ring_start", "ring_region", "image_start",
        "ring_area2", "num_rings", "num_vertices", "workspace", "workspace_bytes", "stream")
OUTPUTS = ("vertices", "ring_start", "ring_region", "image_start", "num_rings", "num_vertices")


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


def workspace_bytes(lib: ctypes.CDLL, b: int, h: int, w: int) -> int:
    need = ctypes.c_size_t()
    assert lib.isc_trace_regions_workspace_bytes(b, h, w, need) == _lib.ISC_OK
    return need.value


def trace(lib: ctypes.CDLL, **kw: object) -> int:
    a = dict(ids=P, B=2, H=40, W=100, R=3, connectivity=8, N=6, V=64, vertices=2 * P, ring_start=3 * P, ring_region=4 * P,
             image_start=5 * P, ring_area2=6 * P, num_rings=7 * P, num_vertices=8 * P, workspace=16 * P,
             workspace_bytes=None, stream=None)
    a.update(kw)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = 1 << 62  # room for any shape: the shape checks come first
    return lib.isc_trace_regions(*(a[name] for name in ARGS))


def test_entry_points_are_declared_exported_and_bound(lib: ctypes.CDLL) -> None:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S)
        assert proto is not None, f"{name} is not declared"
        assert hasattr(raw, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(proto.group(1).split(","))
        assert getattr(lib, name).argtypes == argtypes
    assert len(_lib.SIGNATURES["isc_trace_regions"][1]) == len(ARGS)
    assert lib.isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive


def test_geometry(lib: ctypes.CDLL) -> None:
    pc, nc, rt, passed = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.isc_trace_regions_geometry(pc, nc, rt, passed) == _lib.ISC_OK
    assert all(1 <= v.value <= 4096 for v in (pc, nc, rt))
    assert 4096 <= passed.value <= 1 << 20  # small enough for a test image to exceed it
    for hole in range(4):
        args = [pc, nc, rt, passed]
        args[hole] = None
        assert lib.isc_trace_regions_geometry(*args) == _lib.ISC_ERR_INVALID_ARG
    assert segmentation.trace_geometry() == (pc.value, nc.value, rt.value, passed.value)


def test_workspace_is_sized_by_the_shape_alone(lib: ctypes.CDLL) -> None:
    one = workspace_bytes(lib, 1, 40, 100)
    assert workspace_bytes(lib, 0, 40, 100) == one  # B == 0 asks for what one image takes
    assert one >= 4 * 40 * 100 * 4  # a word for each of the 4 H W vertices an image can have, at the least
    assert one <= 256 * 40 * 100 + 4096  # ... and a bounded number of bytes a pixel
    assert workspace_bytes(lib, 1, 100, 40) == one
    assert 3 * one - 4096 <= workspace_bytes(lib, 3, 40, 100) <= 3 * one + 4096
    assert workspace_bytes(lib, 1, 1, 1) >= 16
    need = ctypes.c_size_t()
    assert lib.isc_trace_regions_workspace_bytes(1, 40, 100, None) == _lib.ISC_ERR_INVALID_ARG
    for b, h, w in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -2, 4)):
        assert lib.isc_trace_regions_workspace_bytes(b, h, w, need) == _lib.ISC_ERR_INVALID_ARG
    for b, h, w in ((65536, 4, 4), (1, 32769, 1), (1, 1, 32769), (1, 32768, 32768), (1, 16384, 32768)):
        assert lib.isc_trace_regions_workspace_bytes(b, h, w, need) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_trace_regions_workspace_bytes(65535, 1, 1, need) == _lib.ISC_OK
    assert lib.isc_trace_regions_workspace_bytes(1, 16383, 32768, need) == _lib.ISC_OK


def test_argument_errors_come_before_any_launch(lib: ctypes.CDLL) -> None:
    for name in ("H", "W", "R", "N", "V"):
        assert trace(lib, **{name: 0}) == _lib.ISC_ERR_INVALID_ARG, name
        assert trace(lib, **{name: -3}) == _lib.ISC_ERR_INVALID_ARG, name
    assert trace(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    for connectivity in (0, 1, 6, -8, 16):
        assert trace(lib, connectivity=connectivity) == _lib.ISC_ERR_INVALID_ARG
    for name in ("ids", *OUTPUTS):
        assert trace(lib, **{name: None}) == _lib.ISC_ERR_INVALID_ARG, name
    assert trace(lib, connectivity=4, ids=None) == _lib.ISC_ERR_INVALID_ARG  # the connectivity passed
    assert trace(lib, ring_area2=None, ids=None) == _lib.ISC_ERR_INVALID_ARG  # a NULL ring_area2 is no error: ids is


def test_limits_at_their_edges(lib: ctypes.CDLL) -> None:
    # a call that passes every limit goes on to the NULL ids, which is the next check
    assert trace(lib, H=32768, W=1, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, H=32769, W=1) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, H=1, W=32768, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, H=1, W=32769) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, H=16383, W=32768, ids=None) == _lib.ISC_ERR_INVALID_ARG  # below 2^29 pixels
    assert trace(lib, H=16384, W=32768) == _lib.ISC_ERR_UNSUPPORTED  # 2^29 pixels: 2^31 vertices are no int32 count
    assert trace(lib, H=(1 << 31) - 1, W=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED  # no overflow in the product
    assert trace(lib, B=65535, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, R=(1 << 31) - 1, ids=None) == _lib.ISC_ERR_INVALID_ARG  # any R
    # B * (N + 1) < 2^31 and B * V < 2^31
    assert trace(lib, B=1, N=(1 << 31) - 2, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=1, N=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, B=2, N=(1 << 30) - 2, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=2, N=(1 << 30) - 1) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, B=1, V=(1 << 31) - 1, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=2, V=(1 << 30) - 1, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=2, V=1 << 30) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, B=65535, V=32768, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=65535, V=32769) == _lib.ISC_ERR_UNSUPPORTED


def test_workspace_and_alignment(lib: ctypes.CDLL) -> None:
    need = workspace_bytes(lib, 2, 40, 100)
    assert trace(lib, workspace=None) == _lib.ISC_ERR_WORKSPACE
    assert trace(lib, workspace_bytes=0) == _lib.ISC_ERR_WORKSPACE
    assert trace(lib, workspace_bytes=need - 1) == _lib.ISC_ERR_WORKSPACE
    assert trace(lib, workspace_bytes=workspace_bytes(lib, 1, 40, 100)) == _lib.ISC_ERR_WORKSPACE  # B counts
    # the exact size passes the workspace check and goes on to the alignment checks
    assert trace(lib, workspace_bytes=need, workspace=16 * P + 8) == _lib.ISC_ERR_ALIGNMENT
    assert trace(lib, workspace_bytes=need, vertices=2 * P + 4) == _lib.ISC_ERR_ALIGNMENT  # an (x, y) pair is stored at once
    assert trace(lib, ring_area2=6 * P + 4) == _lib.ISC_ERR_ALIGNMENT  # 64-bit atomics
    for name in ("ids", "ring_start", "ring_region", "image_start", "num_rings", "num_vertices"):
        assert trace(lib, **{name: 9 * P + 2}) == _lib.ISC_ERR_ALIGNMENT, name


def test_empty_batch_launches_nothing(lib: ctypes.CDLL) -> None:
    assert trace(lib, B=0) == _lib.ISC_OK
    nothing = dict.fromkeys(("ids", *OUTPUTS, "ring_area2", "workspace"))
    assert trace(lib, B=0, workspace_bytes=0, **nothing) == _lib.ISC_OK
    assert trace(lib, B=0, H=0) == _lib.ISC_ERR_INVALID_ARG  # ... but is checked all the same
    assert trace(lib, B=0, W=32769) == _lib.ISC_ERR_UNSUPPORTED
    assert trace(lib, B=0, connectivity=5) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=0, N=0) == _lib.ISC_ERR_INVALID_ARG
    assert trace(lib, B=0, V=1 << 30) == _lib.ISC_OK
