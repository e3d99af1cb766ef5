"""numpy restatement of isc_label_map_windows (a helper, not a conftest), built on tests/segment_oracle.py: the window
grid by its formula, every window's blend with `so.upsampled` (steps 1 - 3 of isc_label_map, `fmaf` with one rounding),
the sum over a pixel's covering windows as float32 additions in the order the header fixes (window rows ascending, inside
a row the columns ascending), one correctly rounded float32 division by their number, and `so.choose` for the rest.  Every
operation is correctly rounded, so the GPU tests ask for equality (`so.same`); tests/test_segment_windows_host.py makes it
prove itself against per-window `F.interpolate`, a sum, a division by the count map and `max` on the CPU.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import segment_oracle as so  # noqa: E402

F32 = np.float32

# (B, C, E, h, w, H, W, win_h, win_w, stride_y, stride_x); case i is seeded with 4321 + i.  Case 0 has pixels in 12
# windows (4 window rows x 3 window columns: the shifted last window on both axes).
CASES = [(2, 7, 32, 3, 4, 37, 53, 24, 20, 10, 8), (1, 9, 64, 3, 3, 48, 48, 24, 24, 12, 12),
         (1, 3, 16, 2, 2, 33, 17, 16, 17, 5, 4), (2, 5, 16, 4, 4, 64, 129, 32, 32, 32, 32),
         (1, 150, 64, 7, 7, 130, 200, 112, 112, 56, 56)]


def starts(length: int, win: int, stride: int) -> list[int]:
    """The window starts along one axis, by the formula of include/imagescry_hip.h."""
    assert 1 <= stride <= win <= length
    n = max(length - win + stride - 1, 0) // stride + 1
    return [min(i * stride, length - win) for i in range(n)]


def cover(length: int, win: int, stride: int) -> np.ndarray:
    """Windows per pixel along one axis, counted window by window."""
    count = np.zeros(length, dtype=np.int64)
    for s in starts(length, win, stride):
        count[s:s + win] += 1
    return count


def averaged(scores: np.ndarray, size: tuple[int, int], window: tuple[int, int], stride: tuple[int, int]) -> np.ndarray:
    """Steps 1 - 4: float32 [B, ny, nx, h, w, C] -> v float32 [B, H, W, C]."""
    assert scores.dtype == np.float32 and scores.ndim == 6
    ys, xs = starts(size[0], window[0], stride[0]), starts(size[1], window[1], stride[1])
    b, ny, nx, _, _, c = scores.shape
    assert (ny, nx) == (len(ys), len(xs))
    acc = np.zeros((b, *size, c), dtype=F32)
    seen = np.zeros(size, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i, y in enumerate(ys):  # i ascending, inside it j ascending: every pixel meets its windows in that order
            for j, x in enumerate(xs):
                u = so.upsampled(scores[:, i, j], window)
                block = acc[:, y:y + window[0], x:x + window[1]]
                first = (seen[y:y + window[0], x:x + window[1]] == 0)[None, :, :, None]
                block[...] = np.where(first, u, block + u)  # acc = u the first time, one float32 addition afterwards
                seen[y:y + window[0], x:x + window[1]] += 1
        assert seen.min() >= 1 and acc.dtype == np.float32
        v = acc / seen.astype(F32)[None, :, :, None]
    assert v.dtype == np.float32
    return v


def label_map_windows_ref(scores: np.ndarray, size, window, stride, class_of=None, min_score: float = -np.inf):
    """Steps 1 - 5 -> labels uint8 [B, H, W], best and margin float32 [B, H, W], counts int32 [B, 256]."""
    return so.choose(averaged(scores, size, window, stride), class_of, min_score)


def case_inputs(i: int):
    """(maps [B * ny * nx, E, h, w], vectors [C, E], scores [B, ny, nx, h, w, C], size, window, stride) of case i as numpy
    float32: unit-norm cells and vectors, the scores the float64 dot products rounded to float32."""
    import torch
    import torch.nn.functional as F

    b, c, e, h, w, big_h, big_w, win_h, win_w, sy, sx = CASES[i]
    ny, nx = len(starts(big_h, win_h, sy)), len(starts(big_w, win_w, sx))
    g = torch.Generator().manual_seed(4321 + i)
    m = F.normalize(torch.randn(b * ny * nx, e, h, w, generator=g), dim=1)
    t = F.normalize(torch.randn(c, e, generator=g), dim=1)
    scores = torch.einsum("behw,ce->bhwc", m.double(), t.double()).float().reshape(b, ny, nx, h, w, c)
    return m.numpy(), t.numpy(), scores.contiguous().numpy(), (big_h, big_w), (win_h, win_w), (sy, sx)
