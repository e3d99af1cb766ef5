"""The host side of isc_overlap_table and isc_overlap_best, which needs no GPU: the entry points are declared, exported
and bound, the geometry calls answer, and every argument error and limit is returned before anything is launched -- so the
pointers here are made-up addresses that nothing may touch."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest

from imagescry_amd import _lib, build, segmentation

P = 0x10000  # a made-up, well aligned device address
HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_overlap_table", "isc_overlap_geometry", "isc_overlap_best", "isc_overlap_best_geometry")
TABLE_ARGS = ("a", "a_dtype", "b", "b_dtype", "B", "H", "W", "Ra", "Rb", "per_image", "accumulate", "table", "stream")
BEST_ARGS = ("table", "B", "Ra", "Rb", "axis", "exclude_none", "best", "inter", "uni", "stream")
U8, I32 = _lib.ISC_U8, _lib.ISC_I32


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


def table(lib: ctypes.CDLL, **kw: object) -> int:
    a = dict(a=P, a_dtype=I32, b=2 * P, b_dtype=I32, B=2, H=40, W=100, Ra=5, Rb=7, per_image=1, accumulate=0, table=3 * P,
             stream=None)
    a.update(kw)
    return lib.isc_overlap_table(*(a[name] for name in TABLE_ARGS))


def best(lib: ctypes.CDLL, **kw: object) -> int:
    a = dict(table=P, B=2, Ra=5, Rb=7, axis=0, exclude_none=0, best=2 * P, inter=3 * P, uni=4 * P, stream=None)
    a.update(kw)
    return lib.isc_overlap_best(*(a[name] for name in BEST_ARGS))


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
    assert len(_lib.SIGNATURES["isc_overlap_table"][1]) == len(TABLE_ARGS)
    assert len(_lib.SIGNATURES["isc_overlap_best"][1]) == len(BEST_ARGS)
    assert re.search(r"#define ISC_I32 3\b", text) and _lib.ISC_I32 == 3
    assert (_lib.ISC_U8, _lib.ISC_F16, _lib.ISC_F32) == (0, 1, 2)
    assert lib.isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive


def test_geometry(lib: ctypes.CDLL) -> None:
    tw, th, slots = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.isc_overlap_geometry(tw, th, slots) == _lib.ISC_OK
    assert tw.value == 64 and 1 <= th.value <= 256  # a wave owns a row of the tile
    assert 64 <= slots.value <= 4096 and slots.value < tw.value * th.value * 4  # 2 x 2 tiles can hold more pairs
    for hole in range(3):
        args = [tw, th, slots]
        args[hole] = None
        assert lib.isc_overlap_geometry(*args) == _lib.ISC_ERR_INVALID_ARG
    assert segmentation.overlap_geometry() == (tw.value, th.value, slots.value)
    columns = ctypes.c_int()
    assert lib.isc_overlap_best_geometry(columns) == _lib.ISC_OK
    assert 64 <= columns.value <= 4096  # small enough for a test table to exceed it
    assert lib.isc_overlap_best_geometry(None) == _lib.ISC_ERR_INVALID_ARG
    assert segmentation.overlap_best_geometry() == columns.value


def test_table_argument_errors_come_before_any_launch(lib: ctypes.CDLL) -> None:
    assert table(lib, a=None, b=None, table=None, B=0) == _lib.ISC_OK  # the shape of the calls below is a valid one
    for name in ("H", "W", "Ra", "Rb"):
        assert table(lib, **{name: 0}) == _lib.ISC_ERR_INVALID_ARG, name
        assert table(lib, **{name: -3}) == _lib.ISC_ERR_INVALID_ARG, name
        assert table(lib, **{name: 1}, a=None) == _lib.ISC_ERR_INVALID_ARG, name  # 1 passes: the NULL is next
        assert table(lib, **{name: 1}, table=3 * P + 4) == _lib.ISC_ERR_ALIGNMENT, name
    assert table(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    for name in ("a_dtype", "b_dtype"):
        for dtype in (_lib.ISC_F16, _lib.ISC_F32, -1, 4):
            assert table(lib, **{name: dtype}) == _lib.ISC_ERR_INVALID_ARG, (name, dtype)
            assert table(lib, **{name: dtype}, B=0) == _lib.ISC_ERR_INVALID_ARG, (name, dtype)
    for name in ("a", "b", "table"):
        assert table(lib, **{name: None}) == _lib.ISC_ERR_INVALID_ARG, name
    # all four combinations of dtypes pass the dtype check and reach the misaligned table
    for da in (U8, I32):
        for db in (U8, I32):
            assert table(lib, a_dtype=da, b_dtype=db, table=3 * P + 4) == _lib.ISC_ERR_ALIGNMENT


def test_table_alignment_goes_by_dtype(lib: ctypes.CDLL) -> None:
    for off in (1, 2, 3):
        assert table(lib, a=P + off) == _lib.ISC_ERR_ALIGNMENT
        assert table(lib, b=2 * P + off) == _lib.ISC_ERR_ALIGNMENT
        # a uint8 raster may start anywhere: the call goes on to the table, which is off 8 bytes
        assert table(lib, a=P + off, a_dtype=U8, table=None) == _lib.ISC_ERR_INVALID_ARG
        assert table(lib, b=2 * P + off, b_dtype=U8, table=None) == _lib.ISC_ERR_INVALID_ARG
        assert table(lib, a=P + off, a_dtype=U8, b=2 * P + off) == _lib.ISC_ERR_ALIGNMENT  # b is still int32
    for off in (1, 2, 4, 7):
        assert table(lib, table=3 * P + off) == _lib.ISC_ERR_ALIGNMENT
        assert table(lib, table=3 * P + off, accumulate=1, per_image=0) == _lib.ISC_ERR_ALIGNMENT


def test_table_limits_at_their_edges(lib: ctypes.CDLL) -> None:
    # a call that passes every limit goes on to the NULL a, which is the next check
    assert table(lib, B=65535, a=None) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED
    assert table(lib, H=1, W=(1 << 31) - 1, a=None) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, H=(1 << 31) - 1, W=1, a=None) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, H=1 << 15, W=1 << 16) == _lib.ISC_ERR_UNSUPPORTED  # 2^31 pixels
    assert table(lib, H=(1 << 15) + 1, W=(1 << 16) - 2, a=None) == _lib.ISC_ERR_INVALID_ARG  # 2^31 - 2 pixels
    assert table(lib, H=(1 << 31) - 1, W=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED  # no overflow in the product
    assert table(lib, Ra=(1 << 13) - 1, Rb=(1 << 12) - 1, a=None) == _lib.ISC_ERR_INVALID_ARG  # 2^25 entries
    assert table(lib, Ra=(1 << 24) - 1, Rb=1, a=None) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, Ra=1, Rb=(1 << 24) - 1, a=None) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, Ra=1 << 24, Rb=1) == _lib.ISC_ERR_UNSUPPORTED  # 2^25 + 2
    assert table(lib, Ra=5792, Rb=5791, a=None) == _lib.ISC_ERR_INVALID_ARG  # 5793 * 5792 = 2^25 - 1376
    assert table(lib, Ra=5792, Rb=5792) == _lib.ISC_ERR_UNSUPPORTED  # 5793^2 = 2^25 + 4417
    assert table(lib, Ra=(1 << 31) - 1, Rb=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED  # no overflow either
    assert table(lib, Ra=(1 << 31) - 1, Rb=(1 << 31) - 1, per_image=0) == _lib.ISC_ERR_UNSUPPORTED


def test_table_of_2_25_plus_1_entries_is_refused(lib: ctypes.CDLL) -> None:
    # (Ra + 1) * (Rb + 1) = 2^25 + 1 = 3 * 11184811
    assert 3 * 11184811 == (1 << 25) + 1
    assert table(lib, Ra=2, Rb=11184810) == _lib.ISC_ERR_UNSUPPORTED
    assert table(lib, Ra=11184810, Rb=2) == _lib.ISC_ERR_UNSUPPORTED
    assert best(lib, Ra=2, Rb=11184810) == _lib.ISC_ERR_UNSUPPORTED
    assert table(lib, Ra=1, Rb=(1 << 24) - 1, a=None) == _lib.ISC_ERR_INVALID_ARG  # 2^25 itself passes


def test_best_argument_errors_and_limits(lib: ctypes.CDLL) -> None:
    assert best(lib, B=0) == _lib.ISC_OK
    for axis in (0, 1):
        assert best(lib, axis=axis, table=None) == _lib.ISC_ERR_INVALID_ARG  # the axis passed: the NULL is next
        assert best(lib, axis=axis, best=2 * P + 2) == _lib.ISC_ERR_ALIGNMENT
    for axis in (-1, 2, 3):
        assert best(lib, axis=axis) == _lib.ISC_ERR_INVALID_ARG
        assert best(lib, axis=axis, B=0) == _lib.ISC_ERR_INVALID_ARG
    for name in ("Ra", "Rb"):
        assert best(lib, **{name: 0}) == _lib.ISC_ERR_INVALID_ARG, name
        assert best(lib, **{name: -1}) == _lib.ISC_ERR_INVALID_ARG, name
        assert best(lib, **{name: 1}, table=None) == _lib.ISC_ERR_INVALID_ARG, name
    assert best(lib, B=-1) == _lib.ISC_ERR_INVALID_ARG
    for name in ("table", "best", "inter", "uni"):
        assert best(lib, **{name: None}) == _lib.ISC_ERR_INVALID_ARG, name
    assert best(lib, B=65535, table=None) == _lib.ISC_ERR_INVALID_ARG
    assert best(lib, B=65536) == _lib.ISC_ERR_UNSUPPORTED
    assert best(lib, Ra=(1 << 13) - 1, Rb=(1 << 12) - 1, table=None) == _lib.ISC_ERR_INVALID_ARG
    assert best(lib, Ra=5792, Rb=5792) == _lib.ISC_ERR_UNSUPPORTED
    assert best(lib, Ra=(1 << 31) - 1, Rb=(1 << 31) - 1) == _lib.ISC_ERR_UNSUPPORTED
    for name in ("table", "inter", "uni"):
        assert best(lib, **{name: 5 * P + 4}) == _lib.ISC_ERR_ALIGNMENT, name
    for off in (1, 2, 3):
        assert best(lib, best=2 * P + off) == _lib.ISC_ERR_ALIGNMENT
    assert best(lib, best=2 * P + 4, table=None) == _lib.ISC_ERR_INVALID_ARG  # 4 bytes are enough for best


def test_empty_batch_launches_nothing(lib: ctypes.CDLL) -> None:
    for accumulate in (0, 1):
        for per_image in (0, 1):
            assert table(lib, B=0, accumulate=accumulate, per_image=per_image) == _lib.ISC_OK
    assert table(lib, B=0, H=0) == _lib.ISC_ERR_INVALID_ARG  # ... but is checked all the same
    assert table(lib, B=0, Rb=0) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, B=0, a_dtype=_lib.ISC_F32) == _lib.ISC_ERR_INVALID_ARG
    assert table(lib, B=0, H=1 << 15, W=1 << 16) == _lib.ISC_ERR_UNSUPPORTED
    assert table(lib, B=0, Ra=5792, Rb=5792) == _lib.ISC_ERR_UNSUPPORTED
    assert best(lib, B=0, table=None, best=None, inter=None, uni=None) == _lib.ISC_OK
    assert best(lib, B=0, Ra=0) == _lib.ISC_ERR_INVALID_ARG
    assert best(lib, B=0, Ra=5792, Rb=5792) == _lib.ISC_ERR_UNSUPPORTED
