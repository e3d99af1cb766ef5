"""The host side of isc_region_cell_weights and isc_region_pool, which needs no GPU: the geometry and every argument
error -- each returned before anything is launched, so the pointers here are made-up addresses that nothing may touch."""

from __future__ import annotations

import ctypes

import pytest

from imagescry_amd import _lib, build

P = 0x10000  # a made-up, well aligned device address

WEIGHT_ARGS = ("ids", "B", "H", "W", "h", "w", "R", "weights", "stream")
POOL_ARGS = ("maps", "B", "E", "S", "weights", "R", "mode", "out", "mass", "stream")


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


def weights(lib: ctypes.CDLL, **kw: object) -> int:
    a = dict(ids=P, B=2, H=40, W=100, h=3, w=7, R=16, weights=2 * P, stream=None)
    a.update(kw)
    return lib.isc_region_cell_weights(*(a[name] for name in WEIGHT_ARGS))


def pool(lib: ctypes.CDLL, **kw: object) -> int:
    a = dict(maps=P, B=2, E=48, S=21, weights=2 * P, R=16, mode=_lib.ISC_POOL_UNIT, out=3 * P, mass=4 * P, stream=None)
    a.update(kw)
    return lib.isc_region_pool(*(a[name] for name in POOL_ARGS))


def test_geometry(lib: ctypes.CDLL) -> None:
    tw, th = ctypes.c_int(), ctypes.c_int()
    assert lib.isc_region_pool_geometry(tw, th) == _lib.ISC_OK
    assert tw.value >= 1 and th.value >= 1 and tw.value * th.value <= 4096
    assert lib.isc_region_pool_geometry(None, th) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_region_pool_geometry(tw, None) == _lib.ISC_ERR_INVALID_ARG
    from imagescry_amd import segmentation

    assert segmentation.region_pool_geometry() == (tw.value, th.value)


def test_weights_argument_errors_come_before_any_launch(lib: ctypes.CDLL) -> None:
    for name in ("H", "W", "h", "w", "R"):
        assert weights(lib, **{name: 0}) == _lib.ISC_ERR_INVALID_ARG, name
        assert weights(lib, **{name: -3}) == _lib.ISC_ERR_INVALID_ARG, name
    assert weights(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    assert weights(lib, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert weights(lib, weights=None) == _lib.ISC_ERR_INVALID_ARG


def test_weights_limits(lib: ctypes.CDLL) -> None:
    assert weights(lib, H=4096, W=4096, ids=None) == _lib.ISC_ERR_INVALID_ARG  # 2^24 pixels pass the limit
    assert weights(lib, H=4097, W=4096) == _lib.ISC_ERR_UNSUPPORTED
    assert weights(lib, H=1, W=(1 << 24) + 1) == _lib.ISC_ERR_UNSUPPORTED
    assert weights(lib, H=1 << 16, W=1 << 16) == _lib.ISC_ERR_UNSUPPORTED  # no overflow in the product
    assert weights(lib, h=1 << 16, w=1 << 15, R=1) == _lib.ISC_ERR_UNSUPPORTED  # h * w = 2^31
    assert weights(lib, h=1 << 16, w=1 << 16, R=1) == _lib.ISC_ERR_UNSUPPORTED
    assert weights(lib, h=1 << 12, w=1 << 13, R=1, ids=None) == _lib.ISC_ERR_INVALID_ARG  # R * h * w = 2^25 passes
    assert weights(lib, h=1 << 12, w=1 << 13, R=2) == _lib.ISC_ERR_UNSUPPORTED
    assert weights(lib, h=1, w=3, R=(1 << 25) // 3 + 1) == _lib.ISC_ERR_UNSUPPORTED
    assert weights(lib, h=3, w=7, R=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED
    assert weights(lib, B=65535, ids=None) == _lib.ISC_ERR_INVALID_ARG
    assert weights(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED


def test_weights_alignment(lib: ctypes.CDLL) -> None:
    assert weights(lib, ids=P + 2) == _lib.ISC_ERR_ALIGNMENT
    assert weights(lib, ids=P + 4, weights=None) == _lib.ISC_ERR_INVALID_ARG  # 4 bytes are enough for ids
    assert weights(lib, weights=2 * P + 4) == _lib.ISC_ERR_ALIGNMENT


def test_pool_argument_errors_come_before_any_launch(lib: ctypes.CDLL) -> None:
    for name in ("E", "S", "R"):
        assert pool(lib, **{name: 0}) == _lib.ISC_ERR_INVALID_ARG, name
        assert pool(lib, **{name: -1}) == _lib.ISC_ERR_INVALID_ARG, name
    assert pool(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    for mode in (-1, 2, 7):
        assert pool(lib, mode=mode) == _lib.ISC_ERR_INVALID_ARG
    for name in ("maps", "weights", "out"):
        assert pool(lib, **{name: None}) == _lib.ISC_ERR_INVALID_ARG, name


def test_pool_limits_and_alignment(lib: ctypes.CDLL) -> None:
    assert pool(lib, S=1 << 25, R=1, maps=None) == _lib.ISC_ERR_INVALID_ARG  # R * S = 2^25 passes the limit
    assert pool(lib, S=(1 << 25) + 1, R=1) == _lib.ISC_ERR_UNSUPPORTED
    assert pool(lib, S=1 << 13, R=(1 << 12) + 1) == _lib.ISC_ERR_UNSUPPORTED
    assert pool(lib, S=(1 << 31) - 1, R=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED
    assert pool(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED
    for name in ("maps", "out"):
        assert pool(lib, **{name: 5 * P + 2}) == _lib.ISC_ERR_ALIGNMENT, name
    for name in ("weights", "mass"):
        assert pool(lib, **{name: 5 * P + 4}) == _lib.ISC_ERR_ALIGNMENT, name
    assert pool(lib, mass=None, out=None) == _lib.ISC_ERR_INVALID_ARG  # a NULL mass is no error: out is


def test_empty_batch_launches_nothing(lib: ctypes.CDLL) -> None:
    assert weights(lib, B=0) == _lib.ISC_OK
    assert weights(lib, B=0, ids=None, weights=None) == _lib.ISC_OK
    assert weights(lib, B=0, H=0) == _lib.ISC_ERR_INVALID_ARG  # ... but is checked all the same
    assert pool(lib, B=0) == _lib.ISC_OK
    assert pool(lib, B=0, maps=None, weights=None, out=None, mass=None) == _lib.ISC_OK
    assert pool(lib, B=0, mode=3) == _lib.ISC_ERR_INVALID_ARG
