"""References and derived bounds for the patch-token head in its LayerNorm form (isc_vit_tokens_out,
isc_vit_tokens_out_skip) and for the plain bicubic position resampling (isc_vit_pos_resample), both in
csrc/vit_tokens.hip: a helper like vit_bounds.py, not a conftest.  Nothing here is fitted to a GPU result.  The GPU
tests are tests/test_gpu_vit_tokens_exact.py, the CPU checks of these references tests/test_vit_token_bounds_host.py.
u = 2^-24 is the float32 unit roundoff and SLACK = 1.01 covers second-order products of first-order terms, as in
vit_bounds.py.

THE HEAD.  out[b][e][cell] = normalize?(LayerNorm(tokens[b][skip + cell]))[e].

Rows (`head_case`).  The families of `vit_bounds.layernorm_case` -- among them `small`, 1e-3 * randn, whose variance is
about eps, so that eps = 1e-6, 1e-5 and 0 give outputs that differ by far more than the bound -- and `constant-exact`:
constant rows whose value is a multiple of 2^-10 below 2.  Such a value has at most 11 significant bits, every partial
sum k c (k <= 1024) at most 21, so a float32 sum of the row is exact in ANY order, the mean is c, every deviation 0, the
variance 0, the reciprocal root 1 / sqrt(eps) finite, and 0 * r * gamma + beta = beta whether or not the last two
operations are fused: the un-normalised cell must EQUAL beta.  The `constant` family of vit_bounds draws c with 24
random bits.  For it the same claim is false in float32 arithmetic: in the kernel's own summation order (four per lane,
xor butterfly) 41 to 72 of 195 such rows have a float32 mean that is not c at D = 252, 260, 516, 768, 772, 1020 (none at
D = 4, 256, 512, 1024, where every step doubles), and the deviation of one ulp of c is multiplied by 1 / sqrt(eps) = 1000.
Those rows are held to the derived bound and to isc_layernorm's bits like every other family.

Un-normalised map: `vit_bounds.layernorm_reference(..., out_f16=False)`, unchanged.

Normalised map (`l2_compose`).  y = LN(x) in float64 with the element-wise LayerNorm bound b (|y^ - y| <= b for the
float32 row y^ that phase 1 leaves in LDS), N = max(||y||, l2_eps), N^ = max(||y^||, l2_eps), z = y / N the reference.
  * max(., l2_eps) and the norm are 1-Lipschitz: |N^ - N| <= ||y^ - y|| <= ||b||, so N^ >= N - ||b|| (the function raises
    unless ||b|| < N / 2).
  * y^_i / N^ - y_i / N = (y^_i - y_i) / N^ + y_i (N - N^) / (N N^):  at most (b_i + |y_i| ||b|| / N) / (N - ||b||).
  * phase 2 and 3 in float32 (k_l2norm_spatial's arithmetic: D / 4 squares added in sequence, three more additions, a
    root, a division) return y^_i / N^ to within rho |y^_i| / N^, rho = preprocess_exact.l2norm_rel_bound(D, 2).
  bound_i = (b_i + |y_i| ||b|| / N + rho (|y_i| + b_i)) / (N - ||b||)
No step is first-order only, so there is no SLACK here beyond the one inside b.

THE POSITION TABLE.  out[1 + oy w + ox] = sum_a sum_b wy_a wx_b pos[1 + iy_a g + ix_b], A = -0.75, source coordinate
src = (g / n) (dst + 1/2) - 1/2 per axis, t = src - floor(src), taps floor(src) - 1 .. + 2 clamped to the table.

Reference (`resample_reference`).  src is formed as a `fractions.Fraction`, its floor and its taps from that fraction
(never from a float32 coordinate), t and the four weights in float64 (2^-53 relative: nothing next to u), the 16-tap
sum in float64.

The interpolant as a function of the coordinate is f(s) = sum_k W(s - k) pos[clamp(k)] over ALL integers k, W the cubic
convolution kernel: continuous, piecewise polynomial, zero outside (-2, 2).  f is therefore Lipschitz in s with constant
L max|pos|, L = sup_t sum_k |dw_k / dt|, across integers too: where the float32 coordinate falls on the other side of an
integer than the rational one (14 -> 46, output 11) the tap SETS differ by one, the weight of the tap that changes is
within L |ds| of zero, and the bound below needs no case for it.  `weight_constants` evaluates SW = sup sum_k |w_k| and
L on a grid of phases from the polynomials and their derivatives and adds half a grid step times the next derivative's
supremum (the second derivatives are linear in t: their suprema are taken at the interval ends); nothing is hard-coded.

Coordinate term.  The kernel receives scale = fl(g / n) (|scale - g / n| <= u g / n) and evaluates scale * (dst + 0.5) -
0.5 with dst + 0.5 exact: the product p = (g / n)(dst + 0.5) carries the scale's u p, its own rounding u p unless the
compiler contracts it into the subtraction, and the subtraction rounds by u |src|; t = src - floor(src) is exact except
for src in [-0.5, 0), where it rounds by at most u:
    ds(dst) = u (2 p + |src| + 1)
Both contraction variants are inside it (the host test checks the two float32 values against it on every grid).
    coordinate = SLACK L SW max_rows|pos[:, c]| (ds_y(oy) + ds_x(ox))
(L on the axis whose coordinate moved, SW = the weights' absolute sum on the other.)

Float32 arithmetic term, at a given float32 phase t.  With A = -0.75 the constants 5A, 8A, 4A, A + 2, A + 3 are float32
numbers.  Outer weights, x = fl(t + 1) or fl(2 - t) in [1, 2] (rounding <= u, |dw / dx| <= 0.75 there):
    A x                 |.| <= 1.5    rounds by 1.5 u                                  1.5 u
    . + 3.75            in [2.25, 3]  3 u                                              4.5 u
    . x                 <= 4.5        2 * 4.5 u + 4.5 u                               13.5 u
    . - 6               in [-3, -1.5] 3 u                                             16.5 u
    . x                 <= 3.12       2 * 16.5 u + 3.12 u                             36.12 u
    . + 3               <= 0.112      0.12 u, and 0.75 u for x                         -> EW_OUTER = 37 u
Inner weights, x = t (exact) or fl(1 - t) (rounding <= u / 2, |dw / dx| <= 1.35):
    1.25 x  1.25 u;  . - 2.25 (<= 2.25)  3.5 u;  . x (<= 1.02)  4.52 u;  . x (<= 1)  5.52 u;  . + 1 (<= 1)  6.52 u;
    0.68 u for x                                                                       -> EW_INNER = 8 u
A fused multiply-add drops one of these roundings and never adds one.  The 16-tap sum: a term wy_a wx_b pos passes
through the product with wx, at most four additions of its line, the product with wy and at most four additions of the
accumulator: ten roundings.
    arithmetic = SLACK (10 u S + sum_ab (EW_a |wx_b| + |wy_a| EW_b) |pos_ab|),  S = sum_ab |wy_a| |wx_b| |pos_ab|
S and the weights are taken at the rational coordinate; at the float32 one they differ by at most L ds max|pos| times
10 u or 37 u, which is below the 1 % that SLACK adds to the coordinate term.
    bound = arithmetic + coordinate

Exact cases (`exact_resample_case`).  Integer tables in [-16, 16] and ratios with dyadic phases: g -> 2 g (scale 1/2,
src = dst / 2 - 1/4, t = 1/4 or 3/4, weights n / 256), 2 g -> g (scale 2, src = 2 dst + 1/2, t = 1/2, weights n / 32)
and the identity on the other axis (weights 0, 1, 0, 0).  `exact_axis_weights` walks the kernel's own evaluation order in
float32, one operation at a time, and asserts that EVERY intermediate equals its float64 value (so a fused operation is
exact too) and that the weights are multiples of the quantum; `exact_resample_case` then asserts, in the manner of
matmul_bound.assert_exact_range, that sum_ab |wy_a| |wx_b| |pos_ab| < 2^24 qy qx -- every partial sum is a multiple of
qy qx below that, a float32 number in any order -- and that the float64 result is a float32 number.  The kernel must
EQUAL it.  The border clamp is exercised on all four sides without a tolerance.
"""

from __future__ import annotations

import functools
import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import torch
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

import preprocess_exact as pe  # noqa: E402
import vit_bounds as vb  # noqa: E402

U = vb.U
SLACK = vb.SLACK
F32 = np.float32

# ------------------------------------------------------------------------------------------------------ the head
L2_EPS = 1e-12
HEAD_EPS = (1e-6, 1e-5)
# NV = ceil(D / 256) 16-byte vectors per lane: 4, 252, 256 -> 1; 260, 512 -> 2; 516, 768 -> 3; 772, 1020, 1024 -> 4; the
# last lane row is partly empty at 4, 252, 260, 516, 772, 1020
HEAD_D = (4, 252, 256, 260, 512, 516, 768, 772, 1020, 1024)
# eight waves, tokens wave + 8 k, 32-cell tiles: one wave, seven, eight, nine (k = 1 starts), 31, a whole tile, 33, two
# whole tiles, 65
HEAD_CELLS = (1, 7, 8, 9, 31, 32, 33, 64, 65)
HEAD_SKIPS = (1, 5)
HEAD_BATCHES = (1, 3)
HEAD_FAMILIES = (*vb.LN_FAMILIES, "constant-exact")
MAX_SKIP, MAX_CELLS, MAX_B = max(HEAD_SKIPS), max(HEAD_CELLS), max(HEAD_BATCHES)


def head_case(d: int, family: str, seed: int) -> dict:
    """`x` [3, 65, D], the patch rows every sub-case of (D, family) takes its cells from, `gamma`, `beta`."""
    rows = MAX_B * MAX_CELLS
    if family == "constant-exact":
        g = vb.gen(seed)
        c = torch.randint(-2 * 1024 + 1, 2 * 1024, (rows, 1), generator=g).float() / 1024.0
        case = {"x": c.expand(rows, d).contiguous(), "gamma": torch.rand(d, generator=g) + 0.5,
                "beta": torch.randn(d, generator=g)}
        assert torch.equal(case["x"] * 1024, (case["x"] * 1024).round()) and float(case["x"].abs().max()) < 2
    else:
        case = vb.layernorm_case(rows, d, family, seed)
    case["x"] = case["x"].reshape(MAX_B, MAX_CELLS, d)
    return case


def head_tokens(x: Tensor, b: int, skip: int, cells: int) -> Tensor:
    """[b, skip + cells, D]: the first `cells` rows of the first `b` images of `x` behind `skip` rows of NaN (rows in
    front of the patches are never read into a cell)."""
    d = x.shape[2]
    tokens = torch.full((b, skip + cells, d), float("nan"))
    tokens[:, skip:] = x[:b, :cells]
    return tokens


def l2_compose(y: Tensor, bound: Tensor, l2_eps: float = L2_EPS) -> tuple[Tensor, Tensor]:
    """(want, bound) of y / max(||y||, l2_eps) over the LAST axis, `bound` the element-wise bound on y (module docstring)."""
    d = y.shape[-1]
    eps = float(torch.tensor(l2_eps, dtype=torch.float32))
    n = torch.clamp(torch.linalg.vector_norm(y, dim=-1, keepdim=True), min=eps)
    nb = torch.linalg.vector_norm(bound, dim=-1, keepdim=True)
    if not bool((nb < n / 2).all()):
        raise ValueError("the LayerNorm bound is not small against the norm of the row: no bound for its direction")
    rho = pe.l2norm_rel_bound(d, 2)
    return y / n, (bound + y.abs() * nb / n + rho * (y.abs() + bound)) / (n - nb)


def head_reference(x: Tensor, gamma: Tensor, beta: Tensor, eps: float) -> dict:
    """float64 references of both forms of the head for rows `x` [..., D]: `ln`, `ln_bound`, `map`, `map_bound`, all
    shaped like `x` (the caller transposes)."""
    shape = x.shape
    want, bound = vb.layernorm_reference(x.reshape(-1, shape[-1]), gamma, beta, eps, out_f16=False)
    z, zb = l2_compose(want, bound)
    return {"ln": want.reshape(shape), "ln_bound": bound.reshape(shape), "map": z.reshape(shape),
            "map_bound": zb.reshape(shape)}


def head_restated(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, *, skip_vector: tuple[int, int] | None = None,
                  neighbour_norm: bool = False) -> Tensor:
    """The normalised head in float32 torch in another order than the kernel's (`vit_bounds.layernorm_restated`, torch's
    own norm over all channels at once, a multiplication by the reciprocal) for rows `x` [rows, D].  Planted faults:
    `skip_vector` = (row, c) leaves the 16-byte vector y[row, 4 c : 4 c + 4] out of that row's norm; `neighbour_norm`
    divides row i by the norm of row i + 1 (cyclically)."""
    y = vb.layernorm_restated(x, gamma, beta, eps)
    ys = y
    if skip_vector is not None:
        row, c = skip_vector
        ys = y.clone()
        ys[row, 4 * c : 4 * c + 4] = 0.0
    n = torch.clamp(torch.linalg.vector_norm(ys, dim=1, keepdim=True), min=L2_EPS)
    if neighbour_norm:
        n = n.roll(-1, dims=0)
    return y * (1.0 / n)


# --------------------------------------------------------------------------------------------- the position table
CUBIC_A = -0.75
EW = np.array([37.0, 8.0, 8.0, 37.0]) * U  # absolute error of a float32 weight (module docstring)
SUM_ROUNDINGS = 10
# (g, h, w): both aspect grids of a 14 x 14 table, one row of 196, 46 x 46 (output 11: another tap set), the DINOv2 sizes
# both ways, a long axis next to a short one from a 64 x 64 table, a one-sample table, a one-cell grid
RESAMPLE_GRIDS = [(14, 11, 17), (14, 17, 11), (14, 1, 196), (14, 46, 46), (16, 37, 37), (37, 16, 16), (64, 100, 3),
                  (1, 3, 2), (5, 1, 1)]
RESAMPLE_D = (4, 64)
# g -> 2 g, 2 g -> g, and each of them on one axis with the identity on the other
EXACT_GRIDS = [(7, 14, 14), (8, 16, 16), (14, 7, 7), (7, 14, 7), (7, 7, 14), (8, 8, 16), (14, 7, 14), (14, 14, 7)]


def cubic_weights(t, a: float = CUBIC_A):
    """The four weights at phase t (numpy float64, last axis 4), in the kernel's polynomial form."""
    t = np.asarray(t, dtype=np.float64)
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    outer = lambda x: ((a * x - 5 * a) * x + 8 * a) * x - 4 * a  # noqa: E731
    inner = lambda x: ((a + 2) * x - (a + 3)) * x * x + 1  # noqa: E731
    return np.stack([outer(x0), inner(x1), inner(x2), outer(x3)], axis=-1)


def cubic_slopes(t, a: float = CUBIC_A):
    """d w_k / d t of `cubic_weights` (last axis 4)."""
    t = np.asarray(t, dtype=np.float64)
    d_outer = lambda x: 3 * a * x * x - 10 * a * x + 8 * a  # noqa: E731
    d_inner = lambda x: 3 * (a + 2) * x * x - 2 * (a + 3) * x  # noqa: E731
    return np.stack([d_outer(t + 1.0), d_inner(t), -d_inner(1.0 - t), -d_outer(2.0 - t)], axis=-1)


@functools.lru_cache(maxsize=None)
def weight_constants(phases: int = 100001, a: float = CUBIC_A) -> tuple[float, float]:
    """(SW, L): upper bounds of sup_t sum_k |w_k(t)| and sup_t sum_k |dw_k / dt| on [0, 1], from a grid of `phases`
    points plus half a step times a bound of the next derivative."""
    t = np.linspace(0.0, 1.0, phases)
    step = 1.0 / (phases - 1)
    lip_grid = float(np.abs(cubic_slopes(t, a)).sum(axis=-1).max())
    # second derivatives are linear in x: |outer''| = |6 a x - 10 a| on [1, 2], |inner''| = |6 (a + 2) x - 2 (a + 3)| on [0, 1]
    outer2 = max(abs(6 * a * x - 10 * a) for x in (1.0, 2.0))
    inner2 = max(abs(6 * (a + 2) * x - 2 * (a + 3)) for x in (0.0, 1.0))
    lip = lip_grid + 0.5 * step * 2 * (outer2 + inner2)
    sw = float(np.abs(cubic_weights(t, a)).sum(axis=-1).max()) + 0.5 * step * lip
    return sw, lip


def rational_axis(g: int, n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per output index of an axis resampled from `g` to `n` samples, from the exact rational coordinate: clamped taps
    [n, 4] (int), float64 weights [n, 4] and the coordinate bound ds [n] of the module docstring."""
    idx = np.empty((n, 4), dtype=np.int64)
    t = np.empty(n)
    ds = np.empty(n)
    for dst in range(n):
        p = Fraction(g, n) * (Fraction(dst) + Fraction(1, 2))
        src = p - Fraction(1, 2)
        fl = math.floor(src)
        t[dst] = float(src - fl)
        idx[dst] = np.clip(np.arange(fl - 1, fl + 3), 0, g - 1)
        ds[dst] = U * (2 * float(p) + abs(float(src)) + 1)
    return idx, cubic_weights(t), ds


def resample_reference(pos: Tensor, g: int, h: int, w: int) -> tuple[Tensor, Tensor]:
    """(want, bound), float64 [1 + h w, D]: row 0 is the class row with bound 0 (a copy)."""
    table = pos.double().numpy()
    d = table.shape[1]
    grid = table[1:].reshape(g, g, d)
    iy, wy, dsy = rational_axis(g, h)
    ix, wx, dsx = rational_axis(g, w)
    taps = grid[iy[:, None, :, None], ix[None, :, None, :]]  # [h, w, 4, 4, D]
    want = np.einsum("ya,xb,yxabd->yxd", wy, wx, taps)
    mag = np.abs(taps)
    s = np.einsum("ya,xb,yxabd->yxd", np.abs(wy), np.abs(wx), mag)
    ew_y = np.broadcast_to(EW, wy.shape)
    ew_x = np.broadcast_to(EW, wx.shape)
    werr = np.einsum("ya,xb,yxabd->yxd", ew_y, np.abs(wx), mag) + np.einsum("ya,xb,yxabd->yxd", np.abs(wy), ew_x, mag)
    sw, lip = weight_constants()
    top = np.abs(grid).max(axis=(0, 1))  # per channel
    coordinate = lip * sw * top[None, None, :] * (dsy[:, None, None] + dsx[None, :, None])
    bound = SLACK * (SUM_ROUNDINGS * U * s + werr + coordinate)
    want = np.concatenate([table[:1], want.reshape(h * w, d)])
    bound = np.concatenate([np.zeros((1, d)), bound.reshape(h * w, d)])
    return torch.from_numpy(want), torch.from_numpy(bound)


def float32_coordinate(g: int, n: int, *, fused: bool, half_pixel: bool = True, outputs: int | None = None) -> np.ndarray:
    """scale * (dst + 0.5) - 0.5 as the kernel evaluates it with scale = fl(g / n), float32 [outputs or n]: `fused` with
    one rounding (the product of two float32 numbers is exact in float64), otherwise with two.  `half_pixel=False`
    drops the - 0.5 (a planted fault); `outputs` != n is an axis under the OTHER axis' scale (another one)."""
    scale = F32(g) / F32(n)
    dst = np.arange(n if outputs is None else outputs, dtype=F32) + F32(0.5)
    off = 0.5 if half_pixel else 0.0
    if fused:
        return (scale.astype(np.float64) * dst.astype(np.float64) - off).astype(F32)
    return (scale * dst).astype(F32) - F32(off)


def _taps_f32(src: np.ndarray, g: int, a: float, mirror: bool) -> tuple[np.ndarray, np.ndarray]:
    """`cubic_taps` in numpy float32, one operation at a time: (idx [n, 4], weights [n, 4])."""
    a = F32(a)
    one, two = F32(1), F32(2)
    fl = np.floor(src)
    t = (src - fl).astype(F32)
    x0, x1, x2, x3 = t + one, t, one - t, two - t

    def outer(x):
        return ((a * x - F32(5) * a) * x + F32(8) * a) * x - F32(4) * a

    def inner(x):
        return ((a + two) * x - (a + F32(3))) * x * x + one

    wgt = np.stack([outer(x0), inner(x1), inner(x2), outer(x3)], axis=-1)
    assert wgt.dtype == np.float32
    idx = fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    if mirror and g >= 4:  # reflect without repeating the border sample: -1 -> 1, g -> g - 2
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx > g - 1, 2 * (g - 1) - idx, idx)
    return np.clip(idx, 0, g - 1), wgt


def resample_restated(pos: Tensor, g: int, h: int, w: int, *, fused: bool, a: float = CUBIC_A, half_pixel: bool = True,
                      swap_scales: bool = False, mirror: bool = False) -> Tensor:
    """The kernel in numpy float32 in its own order (weights, lines of four taps, four lines); `fused` contracts the
    coordinate and every multiply-add, the other variant rounds each operation.  Planted faults: another `a`, the - 0.5
    dropped from the coordinate, the two axis scales exchanged, border taps mirrored instead of clamped."""
    table = pos.numpy()
    d = table.shape[1]
    grid = table[1:].reshape(g, g, d)
    sy = float32_coordinate(g, w if swap_scales else h, fused=fused, half_pixel=half_pixel, outputs=h)
    sx = float32_coordinate(g, h if swap_scales else w, fused=fused, half_pixel=half_pixel, outputs=w)
    iy, wy = _taps_f32(sy, g, a, mirror)
    ix, wx = _taps_f32(sx, g, a, mirror)

    def madd(acc, wgt, val):
        if fused:
            return (acc.astype(np.float64) + wgt.astype(np.float64) * val.astype(np.float64)).astype(F32)
        return acc + wgt * val

    acc = np.zeros((h, w, d), dtype=F32)
    for ta in range(4):
        line = np.zeros((h, w, d), dtype=F32)
        for tb in range(4):
            line = madd(line, wx[None, :, tb, None], grid[iy[:, ta][:, None], ix[:, tb][None, :]])
        acc = madd(acc, wy[:, None, ta, None], line)
    assert acc.dtype == np.float32
    return torch.from_numpy(np.concatenate([table[:1], acc.reshape(h * w, d)]))


def resample_table(g: int, d: int, seed: int) -> Tensor:
    """[1 + g g, D] float32: a table of the size of a checkpoint's (0.02 * randn)."""
    return torch.randn(1 + g * g, d, generator=vb.gen(seed)) * 0.02


def exact_axis_weights(g: int, n: int) -> tuple[np.ndarray, np.ndarray, float, np.ndarray]:
    """(idx [n, 4], weights [n, 4] float64, quantum, clamped [n, 2]) of an axis whose phases are dyadic.  Walks the
    kernel's evaluation order in float32 and in float64 side by side and asserts that no operation rounds.  `clamped`:
    does the output use, with a weight that is not zero, a tap clamped at the low / at the high end of the table?"""
    scale32 = F32(g) / F32(n)
    assert float(scale32) == g / n and Fraction(g, n) == Fraction(float(scale32)), f"{g} / {n} is no float32 number"
    a = CUBIC_A
    quantum = 1.0 if g == n else 2.0**-8
    idx = np.empty((n, 4), dtype=np.int64)
    wgt = np.empty((n, 4))
    clamped = np.zeros((n, 2), dtype=bool)
    for dst in range(n):
        src_q = Fraction(g, n) * (Fraction(dst) + Fraction(1, 2)) - Fraction(1, 2)
        steps32, steps64 = [], []
        for kind, store in ((F32, steps32), (np.float64, steps64)):
            c = lambda v: kind(v)  # noqa: E731
            prod = c(scale32) * (c(dst) + c(0.5))
            src = prod - c(0.5)
            fl = np.floor(src)
            t = src - fl
            x = [t + c(1), t, c(1) - t, c(2) - t]
            store += [prod, src, t, *x]
            for k in (0, 3):
                v = c(a) * x[k]; store.append(v)  # noqa: E702
                v = v - c(5) * c(a); store.append(v)  # noqa: E702
                v = v * x[k]; store.append(v)  # noqa: E702
                v = v + c(8) * c(a); store.append(v)  # noqa: E702
                v = v * x[k]; store.append(v)  # noqa: E702
                v = v - c(4) * c(a); store.append(v)  # noqa: E702
            for k in (1, 2):
                v = (c(a) + c(2)) * x[k]; store.append(v)  # noqa: E702
                v = v - (c(a) + c(3)); store.append(v)  # noqa: E702
                v = v * x[k]; store.append(v)  # noqa: E702
                v = v * x[k]; store.append(v)  # noqa: E702
                v = v + c(1); store.append(v)  # noqa: E702
        assert all(type(v) is np.float32 for v in steps32)
        assert [float(v) for v in steps32] == [float(v) for v in steps64], f"{g} -> {n}, output {dst}: an operation rounds"
        assert Fraction(float(steps64[1])) == src_q
        fl = math.floor(src_q)
        raw = np.arange(fl - 1, fl + 3)
        idx[dst] = np.clip(raw, 0, g - 1)
        wgt[dst] = cubic_weights(float(src_q - fl))
        clamped[dst] = [bool(((raw < 0) & (wgt[dst] != 0)).any()), bool(((raw > g - 1) & (wgt[dst] != 0)).any())]
        assert [float(steps64[k]) for k in (12, 18, 23, 28)] == [wgt[dst][0], wgt[dst][3], wgt[dst][1], wgt[dst][2]]
    assert np.array_equal(wgt / quantum, np.round(wgt / quantum)), "weights are no multiples of the quantum"
    return idx, wgt, quantum, clamped


def exact_resample_case(g: int, h: int, w: int, d: int, seed: int) -> dict:
    """`pos` [1 + g g, D] of integers in [-16, 16] and `want` [1 + h w, D] float32, which the kernel must EQUAL; the
    exact range of every partial sum is asserted (module docstring).  `border`: which sides of the table some output clamps a weighted tap at."""
    pos = torch.randint(-16, 17, (1 + g * g, d), generator=vb.gen(seed)).float()
    grid = pos[1:].double().numpy().reshape(g, g, d)
    iy, wy, qy, cy = exact_axis_weights(g, h)
    ix, wx, qx, cx = exact_axis_weights(g, w)
    taps = grid[iy[:, None, :, None], ix[None, :, None, :]]
    want = np.einsum("ya,xb,yxabd->yxd", wy, wx, taps)
    top = float(np.einsum("ya,xb,yxabd->yxd", np.abs(wy), np.abs(wx), np.abs(taps)).max())
    if not top < 2.0**24 * qy * qx:
        raise AssertionError(f"partial sums may reach {top}, outside the exact range of float32 (2^24 * {qy * qx})")
    assert np.array_equal(want / (qy * qx), np.round(want / (qy * qx)))
    want32 = want.astype(F32)
    assert np.array_equal(want32.astype(np.float64), want), "the reference is not a float32 number"
    want32 = torch.from_numpy(np.concatenate([pos[:1].numpy(), want32.reshape(h * w, d)]))
    return {"pos": pos, "want": want32, "top": top,
            "border": {"top": bool(cy[:, 0].any()), "bottom": bool(cy[:, 1].any()), "left": bool(cx[:, 0].any()),
                       "right": bool(cx[:, 1].any())}}
