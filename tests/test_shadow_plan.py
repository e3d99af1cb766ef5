"""The level plan of a search, read from the host-only entry isc_cosine_topk_plan (cosine_topk.hip, make_plan; DESIGN.md
section 2, "The int8 level").  Without a shadow the plan is the float one, level for level; with one, every level after the
sample of a call with more than 256 queries per pass is an int8 level that satisfies the survivor inequality with the
segments of its real number of chunks -- but for the short piece next to the sample, which runs in fp16 when longer
levels follow it (the faster form of the two at the headline shape, LABLOG.md)."""

from __future__ import annotations

import ctypes
import math

import pytest

from imagescry_amd import _lib, build

TM = 256
CAP = 32
QCAP = 8192
I8_INFLATION = 16
SEGS_PER_CHUNK = 8  # the 256-query tile: 2 row-block waves x 4 lane groups
MAX = 16


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def _plan(lib, n: int, d: int, q: int, k: int, shadow: int, dtype: int = _lib.ISC_F16):
    nl = ctypes.c_int()
    ends = (ctypes.c_int64 * MAX)()
    kinds = (ctypes.c_int * MAX)()
    assert lib.isc_cosine_topk_plan(dtype, n, d, q, k, shadow, MAX, nl, ends, kinds) == 0
    return list(ends[: nl.value]), list(kinds[: nl.value])


def _kp(k: int) -> int:
    return (k + 6 + 15) // 16 * 16


def _wgs(q: int) -> int:
    return 256 // math.ceil(min(q, 1024) / 256)


def _list_budget(kp: int) -> int:
    return int(QCAP * kp / (kp + 8.0 * math.sqrt(kp)))


def _nchunks(rows: int, wgs: int) -> int:
    ntiles = math.ceil(rows / TM)
    per = math.ceil(ntiles / min(wgs, ntiles))
    return math.ceil(ntiles / per)


# the level ends of the float plan, from the build before the int8 plan existed
FLOAT_PLANS = {
    (10_000_000, 768, 1024, 10): [16_384, 2_113_536, 10_000_000],
    (6_000_123, 64, 512, 10): [32_768, 5_603_328, 6_000_123],
    (1_250_000, 768, 64, 10): [65_536, 1_250_000],
}


@pytest.mark.parametrize("shape", sorted(FLOAT_PLANS))
def test_without_a_shadow_the_plan_is_the_float_plan(lib, shape) -> None:
    ends, kinds = _plan(lib, *shape, 0)
    assert ends == FLOAT_PLANS[shape]
    assert kinds == [0] + [1] * (len(ends) - 1)


@pytest.mark.parametrize("k", [10, 58])
@pytest.mark.parametrize("q", [257, 512, 1024])
@pytest.mark.parametrize("n", [100_000, 300_123, 1_400_123, 2_200_003, 6_000_123, 10_000_000, 100_000_000])
def test_int8_plan(lib, n: int, q: int, k: int) -> None:
    d = 768
    kp, wgs = _kp(k), _wgs(q)
    ends, kinds = _plan(lib, n, d, q, k, 1)
    flt_ends, _ = _plan(lib, n, d, q, k, 0)
    # contiguous, tile-aligned, the sample unchanged
    assert ends[-1] == n and ends[0] == flt_ends[0] and kinds[0] == 0
    assert all(a < b for a, b in zip(ends, ends[1:]))
    assert all(e % TM == 0 for e in ends[:-1])
    assert all(kd in (1, 2) for kd in kinds[1:])
    # every swept shape runs on the shadow; only the piece next to the sample may be a float level, and only in front of
    # longer int8 levels
    assert 2 in kinds
    assert all(kd == 2 for kd in kinds[2:]) and (kinds[1] == 2 or len(kinds) > 2)
    # every int8 level holds I8_INFLATION x the float filter's expected survivors in the segments of its real chunks
    # (a float piece in front of int8 levels is held to the int8 inequality too)
    for r0, r1 in zip(ends, ends[1:]):
        budget = min(_list_budget(kp), SEGS_PER_CHUNK * _nchunks(r1 - r0, wgs) * CAP // 8)
        assert kp * (r1 - r0) / r0 * I8_INFLATION <= budget, (r0, r1)
    # a shape whose last float level qualified before the int8 plan still runs on the shadow
    full = min(_list_budget(kp), SEGS_PER_CHUNK * wgs * CAP // 8)
    qualified = len(flt_ends) >= 3 and kp * (n - flt_ends[-2]) / flt_ends[-2] * I8_INFLATION <= full
    uses = ctypes.c_int()
    assert lib.isc_cosine_topk_uses_shadow(_lib.ISC_F16, n, d, q, k, uses) == 0
    assert bool(uses.value) == (2 in kinds)
    if qualified:
        assert 2 in kinds
    # the backward layout: when every level is an int8 level, the last one starts at n / R8, or -- when its tiles do not
    # divide into `wgs` chunks, so that its segments hold less than the full budget -- at most one unit of ratio later
    # The float plan with its last level on the shadow -- what make_plan falls back to when the layout does not fit --
    # would have the float plan's ends: no swept shape with more than one level after the sample may come out that way.
    r8 = 1 + full // (kp * I8_INFLATION)
    if n > r8 * ends[0]:
        assert len(ends) > 2 and ends != flt_ends
    if len(ends) > 2:
        assert math.ceil(math.ceil(n / r8) / TM) * TM <= ends[-2] <= math.ceil(math.ceil(n / max(r8 - 1, 2)) / TM) * TM


def test_headline_plan(lib) -> None:
    ends, kinds = _plan(lib, 10_000_000, 768, 1024, 10, 1)
    assert kinds == [0, 1, 2, 2]
    assert ends == [16_384, 123_648, 1_111_296, 10_000_000]


@pytest.mark.parametrize("n,d,q,k,kinds", [
    (300_123, 64, 1024, 10, [0, 1, 2]),
    (400_123, 100, 300, 10, [0, 1, 2]),
    (1_400_123, 64, 1024, 10, [0, 1, 2, 2]),
    (12_100_123, 64, 1024, 10, [0, 1, 2, 2, 2]),
    (300_123, 768, 1000, 10, [0, 1, 2]),
    (16_684, 64, 1024, 10, [0, 2]),
    (300_123, 64, 1024, 58, [0, 1, 2, 2, 2]),
])
def test_smallest_banks_with_chained_levels(lib, n, d, q, k, kinds) -> None:
    """The banks of tests/test_gpu_shadow_levels.py have the structure they are there for."""
    assert _plan(lib, n, d, q, k, 1)[1] == kinds


@pytest.mark.parametrize("shape", [(10_000_000, 768, 256, 10), (10_000_000, 1152, 1024, 10), (10_000_000, 768, 64, 10)])
def test_shapes_that_never_use_the_shadow(lib, shape) -> None:
    assert _plan(lib, *shape, 1) == _plan(lib, *shape, 0)
    uses = ctypes.c_int(1)
    assert lib.isc_cosine_topk_uses_shadow(_lib.ISC_F16, *shape, uses) == 0 and uses.value == 0


def test_fp32_banks_and_short_buffers(lib) -> None:
    shape = (10_000_000, 768, 1024, 10)
    assert _plan(lib, *shape, 1, dtype=_lib.ISC_F32) == _plan(lib, *shape, 0, dtype=_lib.ISC_F32)
    nl = ctypes.c_int()
    ends = (ctypes.c_int64 * 2)()
    kinds = (ctypes.c_int * 2)()
    assert lib.isc_cosine_topk_plan(_lib.ISC_F16, *shape, 1, 2, nl, ends, kinds) == _lib.ISC_ERR_INVALID_ARG
    assert nl.value == 4
    # Q > 1024 runs as passes of 1024: the same plan
    assert _plan(lib, 10_000_000, 768, 16_384, 10, 1) == _plan(lib, *shape, 1)
