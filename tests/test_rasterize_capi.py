"""The host side of isc_rasterize_polygons, which needs no GPU: the entry points are declared, exported and bound, the
geometry and workspace calls answer, and every argument error and limit is returned before anything is launched -- so the
pointers here are made-up addresses that nothing may touch."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest

from imagescry_amd import _lib, build, segmentation

P = 0x10000  # a made-up, well aligned device address
HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_rasterize_polygons", "isc_rasterize_polygons_workspace_bytes", "isc_rasterize_polygons_geometry")
ARGS = ("vertices", "ring_start", "ring_region", "image_start", "B", "H", "W", "R", "fill_rule", "all_touched", "ids",
        "counts", "workspace", "workspace_bytes", "stream")


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


def raster(lib: ctypes.CDLL, **kw: object) -> int:
    a = dict(vertices=P, ring_start=2 * P, ring_region=3 * P, image_start=4 * P, B=2, H=40, W=100, R=3,
             fill_rule=_lib.ISC_FILL_EVENODD, all_touched=0, ids=5 * P, counts=6 * P, workspace=7 * P, workspace_bytes=64,
             stream=None)
    a.update(kw)
    return lib.isc_rasterize_polygons(*(a[name] for name in ARGS))


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
    assert len(_lib.SIGNATURES["isc_rasterize_polygons"][1]) == len(ARGS)
    assert lib.isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive
    header = HEADER.read_text()
    assert re.search(r"#define ISC_FILL_EVENODD 0\b", header) and _lib.ISC_FILL_EVENODD == 0
    assert re.search(r"#define ISC_FILL_NONZERO 1\b", header) and _lib.ISC_FILL_NONZERO == 1
    assert re.search(r"#define ISC_RASTER_MAX_COORD \(1 << 23\)", header) and _lib.ISC_RASTER_MAX_COORD == 1 << 23


def test_geometry(lib: ctypes.CDLL) -> None:
    tw, th, chunk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.isc_rasterize_polygons_geometry(tw, th, chunk) == _lib.ISC_OK
    assert tw.value >= 1 and th.value >= 1 and tw.value * th.value <= 4096 and 1 <= chunk.value <= 4096
    for hole in range(3):
        args = [tw, th, chunk]
        args[hole] = None
        assert lib.isc_rasterize_polygons_geometry(*args) == _lib.ISC_ERR_INVALID_ARG
    assert segmentation.rasterize_geometry() == (tw.value, th.value, chunk.value)


def test_workspace_bytes(lib: ctypes.CDLL) -> None:
    need = ctypes.c_size_t()
    sizes = {}
    for n in (0, 1, 2, 1000, (1 << 31) - 1):
        assert lib.isc_rasterize_polygons_workspace_bytes(n, need) == _lib.ISC_OK
        sizes[n] = need.value
    assert sizes[0] >= 16 and sizes[1] >= 16 and sizes[1000] >= sizes[2] >= sizes[1]
    assert sizes[1000] <= 64 * 1000  # a few words a ring
    assert lib.isc_rasterize_polygons_workspace_bytes(-1, need) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_rasterize_polygons_workspace_bytes(5, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_rasterize_polygons_workspace_bytes(1 << 31, need) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_rasterize_polygons_workspace_bytes(1 << 40, need) == _lib.ISC_ERR_UNSUPPORTED


def test_argument_errors_come_before_any_launch(lib: ctypes.CDLL) -> None:
    for name in ("H", "W", "R"):
        assert raster(lib, **{name: 0}) == _lib.ISC_ERR_INVALID_ARG, name
        assert raster(lib, **{name: -3}) == _lib.ISC_ERR_INVALID_ARG, name
    assert raster(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    for name in ("vertices", "ring_start", "ring_region", "image_start", "ids"):
        assert raster(lib, **{name: None}) == _lib.ISC_ERR_INVALID_ARG, name
    for rule in (-1, 2, 7):
        assert raster(lib, fill_rule=rule) == _lib.ISC_ERR_INVALID_ARG
    assert raster(lib, fill_rule=_lib.ISC_FILL_NONZERO, ids=None) == _lib.ISC_ERR_INVALID_ARG  # the rule passed
    assert raster(lib, counts=None, ids=None) == _lib.ISC_ERR_INVALID_ARG  # a NULL counts is no error: ids is


def test_limits_at_their_edges(lib: ctypes.CDLL) -> None:
    # a call that passes every limit goes on to the NULL ids, which is the next check
    assert raster(lib, H=32768, W=1, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert raster(lib, H=32769, W=1) == _lib.ISC_ERR_UNSUPPORTED
    assert raster(lib, H=1, W=32768, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert raster(lib, H=1, W=32769) == _lib.ISC_ERR_UNSUPPORTED
    assert raster(lib, H=32768, W=32768, ids=None) == _lib.ISC_ERR_INVALID_ARG  # 2^30 pixels: the most two sides give
    assert raster(lib, H=65536, W=32767) == _lib.ISC_ERR_UNSUPPORTED
    assert raster(lib, H=(1 << 31) - 1, W=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED  # no overflow in the product
    assert raster(lib, B=65535, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert raster(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED
    assert raster(lib, R=(1 << 31) - 1, ids=None) == _lib.ISC_ERR_INVALID_ARG  # any R


def test_workspace_and_alignment(lib: ctypes.CDLL) -> None:
    assert raster(lib, workspace=None) == _lib.ISC_ERR_WORKSPACE
    assert raster(lib, workspace_bytes=0) == _lib.ISC_ERR_WORKSPACE
    assert raster(lib, workspace_bytes=15) == _lib.ISC_ERR_WORKSPACE
    assert raster(lib, workspace_bytes=16, workspace=7 * P + 8) == _lib.ISC_ERR_ALIGNMENT  # 16 bytes are a workspace
    assert raster(lib, vertices=P + 4) == _lib.ISC_ERR_ALIGNMENT  # an (x, y) pair is loaded at once
    for name in ("ring_start", "ring_region", "image_start", "ids", "counts"):
        assert raster(lib, **{name: 9 * P + 2}) == _lib.ISC_ERR_ALIGNMENT, name


def test_empty_batch_launches_nothing(lib: ctypes.CDLL) -> None:
    assert raster(lib, B=0) == _lib.ISC_OK
    assert raster(lib, B=0, vertices=None, ring_start=None, ring_region=None, image_start=None, ids=None, counts=None,
                  workspace=None, workspace_bytes=0) == _lib.ISC_OK
    assert raster(lib, B=0, H=0) == _lib.ISC_ERR_INVALID_ARG  # ... but is checked all the same
    assert raster(lib, B=0, W=32769) == _lib.ISC_ERR_UNSUPPORTED
    assert raster(lib, B=0, fill_rule=2) == _lib.ISC_ERR_INVALID_ARG
