"""CPU restatement of the antialiased bicubic image resize (test infrastructure, next to tests/dinov2_oracle.py, whose
per-axis weights it is built from) and the bound a float32 evaluation of it has to meet.

The bound is the derivation in tests/test_dinov2_host.py's module docstring with each axis' own input size in place of
`g`: an output is sum_a wy_a sum_b wx_b v_ab over ny x nx taps, Ay = max sum_a |wy_a| and Ax likewise;
bound = u top ((ny + nx) Ay Ax + Ay Ex + Ax Ey), E the summed error of one axis' normalised float32 weights,
E = ((1 + A) q rho + n A^2 + A) u with rho = 2.8 min(in, out) + 33 and q = max taps / raw weight sum.  It is a worst
case, so a correct float32 kernel (torch's included) lies far inside it, while a kernel without antialiasing, with the
crop one row off or with A = -0.75 misses it by orders of magnitude on random images (figures: test_preprocess_aa_host)."""

from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path

import torch
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

from dinov2_oracle import aa_axis_weights, cubic_aa  # noqa: E402

# (H1, W1) -> resize / crop of `resize_center_crop`: the shapes of the GPU tests
SHAPES = [
    ((45, 70), 32, 28),    # columns cropped
    ((70, 45), 32, 32),    # rows cropped, top = 8
    ((20, 13), 28, 28),    # upscale
    ((33, 33), 28, 28),
    ((97, 301), 14, 14),   # s ~ 6.9, about 29 taps
    ((448, 470), 14, 14),  # scale 32 and a little more: 130+ taps
    ((31, 40), 31, 28),    # odd margin, offset 2
]


@lru_cache(maxsize=None)
def axis_matrix(n_in: int, n_out: int) -> Tensor:
    """float64 `[n_out, n_in]`: row i holds the normalised weights of output i."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i, (lo, wt) in enumerate(aa_axis_weights(n_in, n_out)):
        m[i, lo : lo + len(wt)] = wt
    return m


def resize_aa_f64(x: Tensor, h2: int, w2: int) -> Tensor:
    """`[..., H1, W1]` -> float64 `[..., H2, W2]`: two matrix products, the horizontal one first."""
    h1, w1 = x.shape[-2:]
    return axis_matrix(h1, h2) @ (x.double() @ axis_matrix(w1, w2).T)


@lru_cache(maxsize=None)
def _axis_terms(n_in: int, n_out: int) -> tuple[int, float, float]:
    """(most taps n, A = max sum |w_i|, E = sum |error of w_i| in units of u) of one axis."""
    s = n_in / n_out
    inv = 1.0 / max(s, 1.0)
    taps = aa_axis_weights(n_in, n_out)
    n = max(len(wt) for _, wt in taps)
    a = max(float(wt.abs().sum()) for _, wt in taps)
    q = max(len(wt) / float(cubic_aa((torch.arange(lo, lo + len(wt), dtype=torch.float64) - s * (i + 0.5) + 0.5)
                                     * inv).sum()) for i, (lo, wt) in enumerate(taps))
    rho = 2.8 * min(n_in, n_out) + 33.0
    return n, a, (1.0 + a) * q * rho + n * a * a + a


def aa_image_bound(h1: int, w1: int, h2: int, w2: int, top: float = 255.0) -> float:
    """The largest difference allowed between a float32 evaluation and `resize_aa_f64`, inputs of magnitude <= top."""
    u = 2.0**-24
    ny, ay, ey = _axis_terms(h1, h2)
    nx, ax, ex = _axis_terms(w1, w2)
    return u * top * ((ny + nx) * ay * ax + ay * ex + ax * ey)


def random_u8(shape: tuple[int, ...], seed: int) -> Tensor:
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
