"""The definitions of isc_region_cell_weights and isc_region_pool (include/imagescry_hip.h) in numpy and pure Python:
what tests/test_gpu_region_pool.py holds the kernels to, weights exactly and vectors bit for bit, and what
tests/test_region_pool_host.py checks against torch on the CPU.

The chains need an EXACT fma: a weight of up to 50 bits times a float32 of 24 does not fit a double, so numpy's
`a * b + c` rounds twice where the kernel's `fma` rounds once.  `fma` below is `float(Fraction(a) * Fraction(b) +
Fraction(c))` -- Python rounds a Fraction to a float correctly -- computed on the integer ratios directly (`int / int` is
correctly rounded too, and needs no gcd); `fma_fraction` is the slow form, and the host test holds one to the other."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

UNIT, MEAN = 0, 1


# ---------------------------------------------------------------------------------------------------------------- weights
def axis_taps(L: int, l: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(i0, i1, weight of i0, weight of i1) of every pixel of an axis of L pixels over l cells, int64."""
    d = np.arange(L, dtype=np.int64)
    n = np.maximum((2 * d + 1) * l - L, 0)
    i0 = n // (2 * L)
    f = n - i0 * 2 * L
    i1 = np.minimum(i0 + 1, l - 1)
    return i0, i1, 2 * L - f, f


def cell_weights_ref(ids: np.ndarray, grid: tuple[int, int], num_regions: int) -> np.ndarray:
    """ids int32 [B, H, W] -> int64 [B, R, h * w], a pixel at a time."""
    b, H, W = ids.shape
    h, w = grid
    y0, y1, wy0, wy1 = axis_taps(H, h)
    x0, x1, wx0, wx1 = axis_taps(W, w)
    out = np.zeros((b, num_regions, h * w), np.int64)
    for img in range(b):
        ys, xs = np.nonzero((ids[img] >= 0) & (ids[img] < num_regions))
        r = ids[img, ys, xs].astype(np.int64)
        for iy, wy in ((y0, wy0), (y1, wy1)):
            for ix, wx in ((x0, wx0), (x1, wx1)):
                np.add.at(out[img], (r, iy[ys] * w + ix[xs]), wy[ys] * wx[xs])
    return out


# -------------------------------------------------------------------------------------------------------------- the chains
def fma_fraction(a: float, b: float, c: float) -> float:
    """The definition, for finite operands."""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:
        return a * b + c  # exact: the sign of the zero by the IEEE rule
    try:
        return float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf


def fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding; non-finite operands by the IEEE rules."""
    if not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))  # inf * 0 = NaN, inf + -inf = NaN
    if not math.isfinite(c):
        return c  # a finite product, however large, does not move an infinity
    an, ad = a.as_integer_ratio()
    bn, bd = b.as_integer_ratio()
    cn, cd = c.as_integer_ratio()
    num = an * bn * cd + cn * ad * bd
    if num == 0:
        return a * b + c
    try:
        return num / (ad * bd * cd)
    except OverflowError:
        return math.inf if num > 0 else -math.inf


def pool_ref(maps: np.ndarray, weights: np.ndarray, mode: int) -> tuple[np.ndarray, np.ndarray]:
    """maps float32 [B, E, S], weights int64 [B, R, S] -> (out float32 [B, R, E], mass int64 [B, R])."""
    b, e, s = maps.shape
    r = weights.shape[1]
    assert weights.shape == (b, r, s) and weights.dtype == np.int64 and maps.dtype == np.float32
    out = np.zeros((b, r, e), np.float32)
    mass = weights.sum(axis=2)
    m64 = maps.astype(np.float64)
    for img in range(b):
        for row in range(r):
            if mass[img, row] == 0:
                continue
            cells = np.nonzero(weights[img, row])[0]  # ascending; the zero cells are skipped, not multiplied
            wts = [float(int(v)) for v in weights[img, row, cells]]
            sums = []
            for dim in range(e):
                acc = 0.0
                for wt, v in zip(wts, m64[img, dim, cells].tolist()):
                    acc = fma(wt, v, acc)
                sums.append(acc)
            with np.errstate(all="ignore"):
                if mode == MEAN:
                    out[img, row] = (np.array(sums, np.float64) / np.float64(float(int(mass[img, row])))).astype(np.float32)
                    continue
                n = 0.0
                for v in sums:
                    n = fma(v, v, n)
                if n != 0.0:  # a NaN n is not zero: the row is what the division gives
                    out[img, row] = (np.array(sums, np.float64) / np.sqrt(np.float64(n))).astype(np.float32)
    return out, mass


def same_floats(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------------------------- maps
def random_ids(rng: np.random.Generator, shape: tuple[int, int, int], num_regions: int, blocks: int = 6) -> np.ndarray:
    """Blocky region maps with ids from -1 to num_regions + 1: both kinds of skipped pixel occur."""
    b, H, W = shape
    coarse = rng.integers(-1, num_regions + 2, size=(b, blocks, blocks))
    ys = np.minimum(np.arange(H) * blocks // H, blocks - 1)
    xs = np.minimum(np.arange(W) * blocks // W, blocks - 1)
    ids = coarse[:, ys][:, :, xs]
    noise = rng.random(shape) < 0.05
    ids[noise] = rng.integers(-1, num_regions + 2, size=int(noise.sum()))
    return np.ascontiguousarray(ids, dtype=np.int32)  # the fancy index leaves another memory order
