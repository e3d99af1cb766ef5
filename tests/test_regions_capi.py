"""isc_label_regions' host side, which needs no GPU: the geometry, the workspace size, and every argument error -- each
returned before anything is launched, so the pointers here are made-up addresses that nothing may touch."""

from __future__ import annotations

import ctypes

import pytest

from imagescry_amd import _lib, build

P = 0x10000  # a made-up, well aligned device address


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


def workspace_bytes(lib: ctypes.CDLL, b: int, h: int, w: int) -> int:
    need = ctypes.c_size_t()
    assert lib.isc_label_regions_workspace_bytes(b, h, w, need) == _lib.ISC_OK
    return need.value


ARGS = ("labels", "best", "B", "H", "W", "connectivity", "min_area", "max_regions", "region_ids", "num_regions",
        "labels_out", "region_label", "region_area", "region_anchor", "region_box", "region_sum", "region_peak",
        "region_peak_score", "workspace", "workspace_bytes", "stream")


def call(lib: ctypes.CDLL, **kw: object) -> int:
    """isc_label_regions on 2 images of 40 x 100 with every pointer set, 8-byte aligned and far apart; `kw` replaces
    arguments."""
    a = {name: P * (i + 1) for i, name in enumerate(ARGS)}
    a.update(B=2, H=40, W=100, connectivity=8, min_area=1, max_regions=16, stream=None)
    a["workspace_bytes"] = workspace_bytes(lib, 2, 40, 100)
    a.update(kw)
    return lib.isc_label_regions(*(a[name] for name in ARGS))


def test_geometry(lib: ctypes.CDLL) -> None:
    tw, th = ctypes.c_int(), ctypes.c_int()
    assert lib.isc_label_regions_geometry(tw, th) == _lib.ISC_OK
    assert tw.value >= 1 and th.value >= 1 and tw.value * th.value <= 4096
    assert lib.isc_label_regions_geometry(None, th) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_label_regions_geometry(tw, None) == _lib.ISC_ERR_INVALID_ARG
    from imagescry_amd import segmentation

    assert segmentation.label_regions_geometry() == (tw.value, th.value)


def test_workspace_bytes(lib: ctypes.CDLL) -> None:
    assert workspace_bytes(lib, 1, 1, 1) > 0
    sizes = [workspace_bytes(lib, b, h, w) for b, h, w in ((1, 30, 40), (2, 30, 40), (2, 31, 40), (2, 31, 41), (2, 448, 448))]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)  # monotone in B, H and W
    assert sizes[-1] >= 2 * 448 * 448 * 4  # at least an int32 per pixel
    assert workspace_bytes(lib, 64, 448, 448) < 64 * 448 * 448 * 6  # ... and little more: no table per pixel
    need = ctypes.c_size_t()
    assert lib.isc_label_regions_workspace_bytes(1, 4, 4, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_label_regions_workspace_bytes(1, 0, 4, need) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_label_regions_workspace_bytes(-1, 4, 4, need) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_label_regions_workspace_bytes(1, 1 << 16, 1 << 15, need) == _lib.ISC_ERR_UNSUPPORTED  # 2^31 pixels
    assert lib.isc_label_regions_workspace_bytes(65536, 4, 4, need) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_label_regions_workspace_bytes(1, 65536, 32767, need) == _lib.ISC_OK  # just below 2^31


@pytest.mark.parametrize("name", ["labels", "region_ids", "num_regions"])
def test_required_pointers(lib: ctypes.CDLL, name: str) -> None:
    assert call(lib, **{name: None}) == _lib.ISC_ERR_INVALID_ARG


def test_argument_errors_come_before_any_launch(lib: ctypes.CDLL) -> None:
    for connectivity in (0, 1, 6, 9, -8):
        assert call(lib, connectivity=connectivity) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, min_area=0) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, min_area=-3) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, max_regions=0) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, H=0) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, W=-1) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    # peak outputs without best
    assert call(lib, best=None) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, best=None, region_peak=None) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, best=None, region_peak_score=None) == _lib.ISC_ERR_INVALID_ARG
    # the despeckled map may not be the input
    assert call(lib, labels_out=P) == _lib.ISC_ERR_INVALID_ARG
    assert call(lib, labels_out=P + 2 * 40 * 100 - 1) == _lib.ISC_ERR_INVALID_ARG


def test_limits(lib: ctypes.CDLL) -> None:
    assert call(lib, H=1 << 16, W=1 << 15) == _lib.ISC_ERR_UNSUPPORTED  # H * W = 2^31
    assert call(lib, H=1 << 15, W=1 << 16) == _lib.ISC_ERR_UNSUPPORTED
    assert call(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED
    # the peak keys: min(max_regions, H * W) <= max(1024, H * W / 8); no such limit without peak outputs
    assert call(lib, max_regions=1025) == _lib.ISC_ERR_UNSUPPORTED
    assert call(lib, max_regions=1025, region_peak=None, region_peak_score=None, workspace=None) == _lib.ISC_ERR_WORKSPACE
    assert call(lib, max_regions=1024, workspace=None) == _lib.ISC_ERR_WORKSPACE  # 1024 passes the limit


def test_workspace_and_alignment(lib: ctypes.CDLL) -> None:
    need = workspace_bytes(lib, 2, 40, 100)
    assert call(lib, workspace=None) == _lib.ISC_ERR_WORKSPACE
    assert call(lib, workspace_bytes=need - 1) == _lib.ISC_ERR_WORKSPACE
    assert call(lib, workspace_bytes=0) == _lib.ISC_ERR_WORKSPACE
    assert call(lib, workspace=P * 19 + 8) == _lib.ISC_ERR_ALIGNMENT
    for name in ("best", "region_ids", "num_regions", "region_label", "region_area", "region_anchor", "region_box",
                 "region_peak", "region_peak_score"):
        assert call(lib, **{name: P * 30 + 2}) == _lib.ISC_ERR_ALIGNMENT, name
    assert call(lib, region_sum=P * 30 + 4) == _lib.ISC_ERR_ALIGNMENT


def test_empty_batch_launches_nothing(lib: ctypes.CDLL) -> None:
    assert call(lib, B=0) == _lib.ISC_OK
    assert call(lib, B=0, labels=None, region_ids=None, num_regions=None, workspace=None, workspace_bytes=0) == _lib.ISC_OK
    assert call(lib, B=0, connectivity=5) == _lib.ISC_ERR_INVALID_ARG  # ... but is checked all the same
