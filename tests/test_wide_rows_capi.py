"""The int8 shadow's cut-off in D, read from the host-only entry isc_cosine_topk_uses_shadow: the shadow is admitted while
Dpad * 127^2 < 2^24 (i8_dims_ok), i.e. up to D = 1024, where k_rescore's 64 lanes each cover two of the 128 sixteen-byte
chunks of a row.  No GPU is needed."""

from __future__ import annotations

import ctypes

import pytest

from imagescry_amd import _lib, build

SHAPE = (6_000_123, 512, 10)  # (N, Q, k): a plan with an int8 level at every admitted D (tests/test_gpu_shadow.py)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def _uses(lib, dtype: int, d: int) -> int:
    n, q, k = SHAPE
    uses = ctypes.c_int(-1)
    assert lib.isc_cosine_topk_uses_shadow(dtype, n, d, q, k, uses) == _lib.ISC_OK
    return uses.value


def test_the_last_admitted_dimension_is_1024(lib) -> None:
    assert _uses(lib, _lib.ISC_F16, 1024) == 1
    assert _uses(lib, _lib.ISC_F16, 1025) == 0
    assert _uses(lib, _lib.ISC_F16, 1152) == 0
    assert 1024 * 127 * 127 < 2 ** 24 <= 1152 * 127 * 127  # 1025 pads to 1152 int8 columns


@pytest.mark.parametrize("d", [64, 768, 1024, 1025, 8192])
def test_an_fp32_bank_never_uses_it(lib, d: int) -> None:
    assert _uses(lib, _lib.ISC_F32, d) == 0


@pytest.mark.parametrize("d", [64, 100, 768, 1023])
def test_every_dimension_below_the_cut_off_is_admitted(lib, d: int) -> None:
    assert _uses(lib, _lib.ISC_F16, d) == 1
