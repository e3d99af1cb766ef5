"""Host model of the int8 level's filter test (cosine_topk.hip, k_dots_filter's int8 epilogue):
quantise a tile and a query as k_bank_quantize / k_prep_i8 do, take the integer dot, evaluate the threshold in float32
as the kernel does, and check the SUPERSET property -- no row whose exact dot with the query exceeds tau is rejected --
on random and adversarial vectors."""

from __future__ import annotations

import numpy as np
import pytest

F = np.float32
UP = F(1.0) + F(1e-6)


def _quantise(x: np.ndarray) -> tuple[np.ndarray, np.float32, np.float32, np.float32]:
    """x: fp16 values as float32 [rows, d] sharing one scale -> (X int, c, e bound, n bound) as the kernels compute them."""
    mx = F(np.abs(x).max())
    c = F(127.0) / mx if mx > 0 else F(1.0)
    xi = np.clip(np.rint((x * c).astype(F)), -127, 127)
    r = x.astype(np.float64) * np.float64(c) - xi
    e = F(np.sqrt((r * r).sum(axis=1).max())) * UP
    n = F(np.sqrt((xi * xi).sum(axis=1).max())) * UP
    return xi.astype(np.int64), c, e, n


def _threshold(tau: np.float32, cq: np.float32, qn: np.float32, eq: np.float32, ct: np.float32, et: np.float32,
               nt: np.float32) -> int:
    with np.errstate(all="ignore"):
        t = F(F(tau * cq) * ct)
        mg = F(F(qn * et) + F(eq * F(nt + et)))
        lo = F(F(t - mg) - F(F(abs(t) + mg) * F(2.0**-20)) - F(1e-30))
    if not lo <= F(2.0e9):
        return 2**31 - 1
    if lo < F(-2.0e9):
        return -(2**31)
    return int(np.floor(lo))


def _check(tile: np.ndarray, query: np.ndarray, taus) -> None:
    tile = tile.astype(np.float16).astype(F)
    query = query.astype(np.float16).astype(F)
    xi, ct, et, nt = _quantise(tile)
    qi, cq, eq, qn = _quantise(query[None, :])
    acc = xi @ qi[0]
    assert np.abs(acc).max() < 2**24
    exact = tile.astype(np.float64) @ query.astype(np.float64)
    for tau in taus:
        thr = _threshold(F(tau), cq, qn, eq, ct, et, nt)
        rejected = acc <= thr
        assert not np.any(rejected & (exact > np.float64(F(tau)))), (tau, thr)


@pytest.mark.parametrize("d", [64, 100, 768, 1024])
def test_random_vectors(d: int) -> None:
    rng = np.random.default_rng(d)
    for _ in range(4):
        tile = rng.standard_normal((256, d)) / np.sqrt(d)
        query = rng.standard_normal(d)
        exact = tile.astype(np.float16).astype(np.float64) @ query.astype(np.float16).astype(np.float64)
        # thresholds AT scores (ties), between them, and far outside
        taus = list(np.sort(exact)[[-1, -2, -16, 0]]) + [0.0, -1e3, 1e3, float(np.median(exact))]
        _check(tile, query, taus)


def test_adversarial_vectors() -> None:
    rng = np.random.default_rng(0)
    d = 768
    # entries at +-max: every element quantises to +-127
    tile = np.where(rng.random((256, d)) < 0.5, -1.0, 1.0) * 0.25
    query = np.where(rng.random(d) < 0.5, -1.0, 1.0) * 3.0
    exact = tile @ query
    _check(tile, query, list(np.sort(exact)[-3:]) + [0.0])
    # every residual at +-0.5: values at half-integer multiples of the scale, one element pinning the scale
    steps = rng.integers(-100, 100, size=(256, d)) + 0.5
    tile = steps / 127.0
    tile[:, 0] = 1.0
    qsteps = rng.integers(-100, 100, size=d) + 0.5
    query = qsteps / 127.0
    query[0] = 1.0
    exact = tile.astype(np.float16).astype(np.float64) @ query.astype(np.float16).astype(np.float64)
    _check(tile, query, list(np.sort(exact)[[-1, -2, -10]]) + [float(exact.mean())])
    # residuals aligned with the query: dx = +0.5 sign(q) raises every dot as far as the bound allows
    tile = (np.rint(rng.standard_normal((256, d)) * 30) + 0.5 * np.sign(qsteps)) / 127.0
    tile[:, 0] = 1.0
    exact = tile.astype(np.float16).astype(np.float64) @ query.astype(np.float16).astype(np.float64)
    _check(tile, query, list(np.sort(exact)[[-1, -5]]))
    # tiny rows beside huge ones: the tile's scale is the huge rows', the tiny rows quantise to zero
    tile = rng.standard_normal((256, d))
    tile[::2] *= 1e-3
    tile[1::2] *= 30.0
    query = rng.standard_normal(d) * 1e-2
    exact = tile.astype(np.float16).astype(np.float64) @ query.astype(np.float16).astype(np.float64)
    small = exact[::2]
    _check(tile, query, [float(np.sort(small)[-1]), float(np.sort(small)[-2]), float(np.sort(small)[0]), 0.0,
                         float(np.sort(exact)[-2])])


def test_degenerate_thresholds() -> None:
    one = F(1.0)
    assert _threshold(F(np.inf), one, one, one, one, one, one) == 2**31 - 1  # padding query: nothing passes
    assert _threshold(F(-np.inf), one, one, one, one, one, one) == -(2**31)  # no threshold yet: everything passes
    assert _threshold(F(1.0), F(np.nan), one, one, one, one, one) == 2**31 - 1  # a query that takes no part
    # a bound that underflows to zero still lets acc = 0 through
    assert _threshold(F(-1e-30), F(1e-20), F(0), F(0), one, F(0), F(0)) == -1
