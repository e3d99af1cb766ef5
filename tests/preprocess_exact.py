"""References for the statistics, normalise, bilinear and L2-norm kernels of csrc/preprocess.hip that need no measured
tolerance (a helper, not a conftest).  Everything here is numpy and Python integers; torch only carries the tensors.
tests/test_preprocess_exact_host.py makes these references prove themselves on the CPU, tests/test_gpu_preprocess_exact.py
holds the kernels to them.  u = 2^-24 is the float32 unit roundoff, U64 = 2^-53 the float64 one.

NORMALISE (`normalize_ref`), bit for bit.  `norm_clip` is `r = __fdiv_rn(v - mu, sd + eps); r != r ? r : fminf(fmaxf(r,
lo), hi)`: one float32 add for the denominator, one float32 subtract, one correctly rounded float32 division, and a
clamp that lets NaN through.  There is no product next to a sum, so nothing can be contracted, and numpy's float32
`+ - /` are the same correctly rounded IEEE operations: given the float32 mean, std and eps the output is reproducible
exactly, a u8 pixel converting to float32 without rounding.  `np.maximum` / `np.minimum` pass NaN on, as the kernel does.

STATISTICS OF u8 (`u8_stats_exact`), bit for bit.  a = sum x and q = sum x^2 are Python integers, the mean is the
fraction a / n and the unbiased variance the fraction (n q - a^2) / (n (n - 1)).  `round_fraction_f32` rounds a fraction
to the nearest float32 (ties to even) with integer arithmetic only, `sqrt_fraction_f32` the square root of one: it takes
m = floor(sqrt(V / 4^e)) with `math.isqrt` and decides the rounding by comparing V / 4^e with (m + 1/2)^2 as fractions.
n = 1 gives a NaN std, as torch's unbiased std.
`final_f64_plain` and `final_f64_shifted` restate the two finalisations of `k_stats_final` in float64 from the exact
integer sums (which is what the u8 partial kernel delivers): the plain `(q - a a / n) / (n - 1)`, which cancels once
a a passes 2^53, and the one shifted by m0 = rint(a / n).  The GPU test may demand equality with the exact value
because the host test shows that the shifted restatement hits it on every input the GPU test uses (`u8_stat_inputs`).

STATISTICS OF float32 (`f32_stats_ref`, `f32_stats_bound`), by a bound.  The reference is the two-pass float64 mean and
unbiased std.  The kernels sum x and x^2 in float64 (the square of a float32 is exact in float64) and an element
passes through this chain of float64 additions, counted from the code:

    k_stats_partial_f32, 4-wide path:  3 (x + y + z + w) + 16 (`s +=`, 16 384 / (256 * 4) trips) + 6 (wave) + 4 (LDS)
    k_stats_partial_f32, scalar path:  64 (`s +=`, 16 384 / 256 trips) + 6 (wave) + 4 (LDS)
    k_stats_final:                     ceil(B * chunks / 256) (`s +=`) + 6 (wave) + 4 (LDS)

so K = 39 + ceil(B chunks / 256) for the 4-wide path and 84 + ceil(B chunks / 256) for the scalar one (`stats_chain`).
The bounds are  |mean' - mean| <= K U64 sum|x| / n  and  |var' - var| <= K U64 sum x^2 / (n - 1)  before the final
cast; the std bound is the larger of sqrt(var + dv) - std and std - sqrt(max(var - dv, 0)), plus U64 std for the
float64 sqrt; both get half a float32 ulp (of the largest value the bound allows) for the cast.  The variance bound
charges the K additions to sum x^2 only.  A worst-case analysis would also charge a a / n (<= sum x^2) twice and add
five roundings of the closing operations, 3 K + 5 in place of K; the test asserts the tighter K, which a sum whose
errors do not all point the same way stays far inside (the host test runs the kernel's summation order against it).

BILINEAR (`bilinear_taps`, `bilinear_ref`).  torch's source index is scale * (dst + 0.5) - 0.5 with scale = in / out in
float32.  `fused=True` evaluates it with one rounding (the product of two float32 numbers and the subtraction of 0.5
are exact in float64, then one cast: `fmaf`), `fused=False` with two.  The rest follows the kernel: clamp at 0, i0 =
min(int(src), in - 1), i1 = min(i0 + 1, in - 1), l1 = clamp(src - i0, 0, 1) and l0 = 1 - l1 in float32.  The blend
ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) is taken in float64 from those float32 taps, so the comparison under
the suite's RESIZE_RTOL / RESIZE_ATOL only has to absorb the kernel's six float32 roundings of the blend.
`tap_disagreements` lists the outputs at which the two evaluations pick another pixel or weight: a size pair where it
is empty cannot tell them apart.

L2 NORM (`l2norm_ref`, `l2norm_rel_bound`), by a bound relative to the float64 value x / max(sqrt(sum x^2), eps).  A
thread squares and adds A0 = ceil(E / 256) (rows) or ceil(E / 4) (spatial) elements in sequence, then the partial sums
meet in 6 wave additions + 3 LDS additions (rows) or 3 LDS additions (spatial): A = A0 + 9 or A0 + 3 additions on an
element's path, and one more rounding for its square unless it is fused.  All terms are positive, so the sum of
squares is off by at most (A + 1) u relatively, its root by half of that; `sqrtf` adds at most one ulp (2 u) and the
division u:

    |y' - y| <= ((A + 1) / 2 + 3) u / (1 - (A + 4) u) |y|

A zero row is 0 / eps = 0 exactly, and a row whose norm is below eps is divided by eps, which the reference does too.
"""

from __future__ import annotations

import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import cases  # noqa: E402

F32 = np.float32
U32 = 2.0**-24
U64 = 2.0**-53
STATS_CHUNK = 16384  # kStatsChunk
STATS_THREADS = 256  # kStatsThreads
WAVE = 64


# ------------------------------------------------------------------------------------------------------- normalise
def normalize_ref(x: np.ndarray, mean: np.ndarray, std: np.ndarray, eps: float, lo: float | None, hi: float | None,
                  *, nhwc4: bool = False) -> np.ndarray:
    """`clip((x - mean) / (std + eps), lo, hi)` in numpy float32.  `x` [B, C, H, W] uint8 or float32; `mean`, `std`
    float32 with C (per channel) or B * C (per image) elements.  `nhwc4`: as [B, H, W, 4], channels past C zero."""
    b, c, h, w = x.shape
    assert x.dtype in (np.uint8, np.float32) and mean.dtype == np.float32 and std.dtype == np.float32
    mu = mean.reshape(-1, c, 1, 1)
    denom = (std + F32(eps)).astype(F32).reshape(-1, c, 1, 1)
    assert mu.shape[0] in (1, b) and denom.shape[0] in (1, b)
    with np.errstate(all="ignore"):
        r = (x.astype(F32) - mu) / denom
        r = np.minimum(np.maximum(r, F32(-np.inf if lo is None else lo)), F32(np.inf if hi is None else hi))
    assert r.dtype == np.float32
    if not nhwc4:
        return r
    out = np.zeros((b, h, w, 4), dtype=F32)
    out[..., :c] = r.transpose(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------- exact rounding to float32
def round_fraction_f32(v: Fraction) -> np.float32:
    """The float32 nearest to the fraction `v` (ties to even, subnormals included), by integer arithmetic."""
    if v == 0:
        return F32(0.0)
    sign, v = (-1.0, -v) if v < 0 else (1.0, v)
    e = v.numerator.bit_length() - v.denominator.bit_length() - 24
    while v >= Fraction(2) ** (e + 24):
        e += 1
    while v < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)
    scaled = v / Fraction(2) ** e
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    out = math.ldexp(m, e)
    assert out < 2.0**128
    return F32(sign * out)


def sqrt_fraction_f32(v: Fraction) -> np.float32:
    """The float32 nearest to sqrt(v) for a fraction v >= 0 of normal size, by `math.isqrt` and a fraction compare."""
    assert v >= 0
    if v == 0:
        return F32(0.0)
    e = (v.numerator.bit_length() - v.denominator.bit_length()) // 2 - 24
    while True:
        w = v / Fraction(4) ** e
        m = math.isqrt(w.numerator // w.denominator)  # floor(sqrt(w))
        if m >= 1 << 24:
            e += 1
        elif m < 1 << 23:
            e -= 1
        else:
            break
    assert e > -149
    half = Fraction(2 * m + 1, 2) ** 2  # (m + 1/2)^2
    if w > half or (w == half and m % 2 == 1):
        m += 1
    return F32(math.ldexp(m, e))


# ------------------------------------------------------------------------------------------------------ u8 statistics
def u8_sums(x: np.ndarray) -> list[tuple[int, int, int]]:
    """Per channel (a, q, n) = (sum x, sum x^2, count) of a uint8 [B, C, H, W] array as Python integers."""
    assert x.dtype == np.uint8 and x.ndim == 4
    out = []
    for c in range(x.shape[1]):
        v = x[:, c].astype(np.int64).ravel()  # 255^2 n < 2^63 for any array that fits in memory
        out.append((int(v.sum()), int((v * v).sum()), int(v.size)))
    return out


def exact_from_sums(a: int, q: int, n: int) -> tuple[np.float32, np.float32]:
    """Correctly rounded float32 mean and unbiased std from the integer sums."""
    mean = round_fraction_f32(Fraction(a, n))
    if n == 1:
        return mean, F32(np.nan)
    return mean, sqrt_fraction_f32(Fraction(n * q - a * a, n * (n - 1)))


def u8_stats_exact(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Correctly rounded float32 per-channel mean and unbiased std of a uint8 [B, C, H, W] array."""
    stats = [exact_from_sums(*s) for s in u8_sums(x)]
    return np.array([m for m, _ in stats], dtype=F32), np.array([s for _, s in stats], dtype=F32)


def final_f64_plain(a: int, q: int, n: int) -> tuple[np.float32, np.float32]:
    """`k_stats_final` without the shift (the float32 path's formula, and the u8 path's before the shift), float64."""
    a, q, n = np.float64(a), np.float64(q), np.float64(n)
    with np.errstate(all="ignore"):
        var = (q - a * a / n) / (n - np.float64(1.0))
        var = np.float64(0.0) if var < 0 else var
        return F32(a / n), F32(np.sqrt(var))


def final_f64_shifted(a: int, q: int, n: int) -> tuple[np.float32, np.float32]:
    """`k_stats_final` with `integer_data`: the sums shifted by m0 = rint(a / n) before the subtraction, float64."""
    assert 65025 * n < 2**53  # every intermediate below is then an exact integer
    a, q, n = np.float64(a), np.float64(q), np.float64(n)
    with np.errstate(all="ignore"):
        m = a / n
        m0 = np.rint(m)
        s1 = a - n * m0
        s2 = q - m0 * (a + s1)
        var = (s2 - s1 * s1 / n) / (n - np.float64(1.0))
        var = np.float64(0.0) if var < 0 else var
        return F32(m), F32(np.sqrt(var))


def ulp_distance(got: np.float32, want: np.float32) -> int:
    """got - want in float32 ulps (both finite and of one sign)."""
    g = int(np.array(got, dtype=F32).view(np.int32))
    w = int(np.array(want, dtype=F32).view(np.int32))
    return g - w


def near_constant(n: int, off: int) -> np.ndarray:
    """n uint8 pixels of 255 with `off` of them, spread over the array, at 254."""
    v = np.full(n, 255, dtype=np.uint8)
    for k in range(off):
        v[(k * 104729 + 12345) % n] = 254
    assert int((v != 255).sum()) == off
    return v


def u8_stat_inputs() -> dict[str, np.ndarray]:
    """Every uint8 [B, C, H, W] input of the GPU statistics test, by name (seeded; the host test proves on the same
    arrays that the shifted float64 finalisation rounds to the exact value)."""
    out = {}
    for name, shape in (("hw5", (3, 2, 1, 5)), ("hw16", (3, 2, 4, 4)), ("hw16383", (3, 2, 129, 127)),
                        ("hw16384", (3, 2, 128, 128)), ("hw16400", (3, 2, 100, 164)), ("hw224", (2, 2, 224, 224)),
                        ("items300", (300, 2, 4, 4)), ("items600", (600, 2, 4, 4)), ("one_plane", (8, 1, 224, 224))):
        out[name] = cases.images_u8(shape, seed=sum(shape)).numpy()
    for name, b, side in (("flat8", 8, 224), ("flat16", 16, 224), ("flat1032", 2, 1032)):
        n = b * side * side
        planes = [near_constant(n, off).reshape(b, side, side) for off in (0, 1, 10)]
        out[name] = np.ascontiguousarray(np.stack(planes, axis=1))
    return out


# ---------------------------------------------------------------------------------------------------- f32 statistics
def f32_stat_inputs() -> dict[str, np.ndarray]:
    """Every float32 [B, C, H, W] input of the GPU statistics test: the u8 shapes as floats, and mean 1e4 with std 1."""
    out = {}
    for name, x in u8_stat_inputs().items():
        if name not in ("flat16", "flat1032"):
            out[name] = x.astype(F32) * F32(0.37) - F32(11.0)
    out["offset"] = (torch.randn(4, 2, 100, 164, generator=cases.gen(41)) + 1.0e4).numpy()
    return out


def stats_chain(b: int, hw: int, vec: bool) -> int:
    """K: the longest chain of float64 additions an element passes through (module docstring)."""
    chunks = -(-hw // STATS_CHUNK)
    return (39 if vec else 84) + -(-(b * chunks) // STATS_THREADS)


def f32_stats_ref(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Two-pass float64 per-channel mean and unbiased std of a float32 [B, C, H, W] array."""
    v = x.astype(np.float64).transpose(1, 0, 2, 3).reshape(x.shape[1], -1)
    n = v.shape[1]
    mean = v.mean(axis=1)
    with np.errstate(all="ignore"):
        var = ((v - mean[:, None]) ** 2).sum(axis=1) / np.float64(n - 1)
    return mean, np.sqrt(var)


def f32_stats_bound(x: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """Per-channel bounds on |mean' - mean| and |std' - std| for float32 results of a chain of `k` additions."""
    v = x.astype(np.float64).transpose(1, 0, 2, 3).reshape(x.shape[1], -1)
    n = v.shape[1]
    mean, std = f32_stats_ref(x)
    dm = k * U64 * np.abs(v).sum(axis=1) / n
    dv = k * U64 * (v * v).sum(axis=1) / (n - 1)
    var = std * std
    ds = np.maximum(np.sqrt(var + dv) - std, std - np.sqrt(np.maximum(var - dv, 0.0))) + U64 * std
    half_ulp = lambda t: 0.5 * np.spacing(np.abs(t).astype(F32)).astype(np.float64)  # noqa: E731
    return dm + half_ulp(np.abs(mean) + dm), ds + half_ulp(std + ds)


def wave_sum(v: np.ndarray) -> np.ndarray:
    """`isc_wave_sum` over the last axis (64 lanes, xor butterfly 32, 16, ... 1) in the array's own precision: lane 0."""
    assert v.shape[-1] == WAVE
    lanes = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0]


def _block_sum(t: np.ndarray) -> np.ndarray:
    """256 per-thread values (last axis) -> the workgroup's sum: wave butterflies, then the four waves in order."""
    w = wave_sum(t.reshape(*t.shape[:-1], STATS_THREADS // WAVE, WAVE))
    acc = np.zeros(w.shape[:-1], dtype=t.dtype)
    for i in range(STATS_THREADS // WAVE):
        acc = acc + w[..., i]
    return acc


def emulate_stats_f32(x: np.ndarray, vec: bool) -> tuple[np.ndarray, np.ndarray]:
    """`k_stats_partial_f32` + `k_stats_final` in float64 in the kernels' own summation order (padding a sum with
    zeros changes no rounding).  Returns the float32 mean and std per channel."""
    b, c, h, w = x.shape
    hw = h * w
    chunks = -(-hw // STATS_CHUNK)
    v = np.zeros((c, b, chunks * STATS_CHUNK), dtype=np.float64)
    v[:, :, :hw] = x.astype(np.float64).transpose(1, 0, 2, 3).reshape(c, b, hw)
    v = v.reshape(c, b * chunks, STATS_CHUNK)
    parts = []
    for t in (v, v * v):
        if vec:
            g = t.reshape(c, -1, 16, STATS_THREADS, 4)
            g = ((g[..., 0] + g[..., 1]) + g[..., 2]) + g[..., 3]
        else:
            g = t.reshape(c, -1, 64, STATS_THREADS)
        acc = np.zeros(g.shape[:2] + (STATS_THREADS,), dtype=np.float64)
        for i in range(g.shape[2]):
            acc = acc + g[:, :, i]
        parts.append(_block_sum(acc))  # [c, items]
    sums = []
    for p in parts:
        items = p.shape[1]
        trips = -(-items // STATS_THREADS)
        padded = np.zeros((c, trips * STATS_THREADS), dtype=np.float64)
        padded[:, :items] = p
        padded = padded.reshape(c, trips, STATS_THREADS)
        acc = np.zeros((c, STATS_THREADS), dtype=np.float64)
        for i in range(trips):
            acc = acc + padded[:, i]
        sums.append(_block_sum(acc))
    a, q = sums
    n = np.float64(b * hw)
    with np.errstate(all="ignore"):
        var = (q - a * a / n) / (n - 1.0)
        var = np.where(var < 0, 0.0, var)
        return (a / n).astype(F32), np.sqrt(var).astype(F32)


# ----------------------------------------------------------------------------------------------------------- bilinear
def bilinear_taps(in_size: int, out_size: int, *, fused: bool) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(i0, i1, l0, l1) of every output index along one axis, as `bilinear_tap` computes them in float32."""
    scale = F32(in_size) / F32(out_size)
    centre = np.arange(out_size, dtype=F32) + F32(0.5)  # exact
    if fused:
        src = (np.float64(scale) * centre.astype(np.float64) - 0.5).astype(F32)  # exact in float64, one rounding
    else:
        src = (scale * centre).astype(F32) - F32(0.5)
    assert src.dtype == np.float32
    src = np.maximum(src, F32(0.0))
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = np.clip(src - i0.astype(F32), F32(0.0), F32(1.0)).astype(F32)
    l0 = (F32(1.0) - l1).astype(F32)
    return i0, i1, l0, l1


def tap_disagreements(in_size: int, out_size: int) -> np.ndarray:
    """The output indices at which the fused and the unfused source index give another pixel or another weight."""
    f = bilinear_taps(in_size, out_size, fused=True)
    u = bilinear_taps(in_size, out_size, fused=False)
    return np.flatnonzero((f[0] != u[0]) | (f[1] != u[1]) | (f[3] != u[3]))


def bilinear_ref(x: np.ndarray, h2: int, w2: int, *, fused: bool = True) -> np.ndarray:
    """[P, H1, W1] uint8 or float32 -> [P, H2, W2] float64: the float64 blend of the float32 taps."""
    _, h1, w1 = x.shape
    y0, y1, ly0, ly1 = bilinear_taps(h1, h2, fused=fused)
    x0, x1, lx0, lx1 = bilinear_taps(w1, w2, fused=fused)
    v = x.astype(np.float64)
    lx0, lx1 = lx0.astype(np.float64), lx1.astype(np.float64)
    ly0, ly1 = ly0.astype(np.float64)[:, None], ly1.astype(np.float64)[:, None]
    top = lx0 * v[:, y0][:, :, x0] + lx1 * v[:, y0][:, :, x1]
    bot = lx0 * v[:, y1][:, :, x0] + lx1 * v[:, y1][:, :, x1]
    return ly0 * top + ly1 * bot


# ------------------------------------------------------------------------------------------------------------ L2 norm
def l2norm_ref(x: np.ndarray, eps: float) -> np.ndarray:
    """[B, E, S] float32 -> x / max(sqrt(sum_E x^2), eps) in float64 (eps as the float32 the kernel receives)."""
    v = x.astype(np.float64)
    norm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    return v / np.maximum(norm, np.float64(F32(eps)))


def l2norm_rel_bound(e: int, s: int) -> float:
    """The relative bound of the module docstring for `k_l2norm_rows` (s == 1) or `k_l2norm_spatial`."""
    adds = -(-e // 256) + 9 if s == 1 else -(-e // 4) + 3
    return ((adds + 1) / 2 + 3) * U32 / (1 - (adds + 4) * U32)


def l2_rows_input(e: int) -> np.ndarray:
    """[4, E, 1] float32 rows: random, zero, norm 1e-13 (below eps = 1e-12) and random of size 300."""
    x = torch.randn(4, e, 1, generator=cases.gen(100 + e)).numpy()
    x[1] = 0.0
    x[2] *= F32(1e-13) / F32(np.sqrt((x[2].astype(np.float64) ** 2).sum()))
    x[3] *= F32(300.0)
    return x


def l2_spatial_input(e: int, s: int) -> np.ndarray:
    """[2, E, S] float32 with a zero column at [0, :, 1]."""
    x = torch.randn(2, e, s, generator=cases.gen(e + s)).numpy()
    x[0, :, 1] = 0.0
    return x


def emulate_l2norm(x: np.ndarray, eps: float, *, fused: bool) -> np.ndarray:
    """`k_l2norm_rows` (S == 1) / `k_l2norm_spatial` in float32 in the kernels' summation order.  `fused`: each square
    enters its sum with one rounding (fmaf) or with two."""
    b, e, s = x.shape
    stride, lanes = (256, 256) if s == 1 else (4, 4)
    trips = -(-e // stride)
    v = np.zeros((b, trips * stride, s), dtype=F32)
    v[:, :e] = x
    v = v.reshape(b, trips, lanes, s)
    acc = np.zeros((b, lanes, s), dtype=F32)
    for i in range(trips):
        t = v[:, i]
        if fused:
            acc = (acc.astype(np.float64) + t.astype(np.float64) * t.astype(np.float64)).astype(F32)
        else:
            acc = acc + t * t
    if s == 1:
        red = wave_sum(acc[:, :, 0].reshape(b, 4, WAVE))  # [b, 4]
    else:
        red = acc  # [b, 4, s]
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    assert tot.dtype == np.float32
    denom = np.maximum(np.sqrt(tot), F32(eps)).astype(F32).reshape(b, 1, s)
    return (x / denom).astype(F32)


def worst_ratio(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    """max |got - want| / bound; 0 / 0 counts as 0, a NaN or infinite `got` as infinitely wrong."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isfinite(got) & ~np.isnan(ratio), ratio, np.inf)
    return float(ratio.max())
