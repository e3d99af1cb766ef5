"""The definition of isc_label_regions (include/imagescry_hip.h) in plain numpy and Python: a flood fill in raster order,
so that regions are met in the order of their anchors, then `min_area`, the numbering, the tables and the peak.  Slow
and obviously right; tests/test_regions_host.py checks it against scipy.ndimage.label.  Reads nothing outside the
repository."""

from __future__ import annotations

import numpy as np

UNLABELED = 255
TABLES = ("label", "area", "anchor", "box", "sum", "peak", "peak_score")
OUTPUTS = ("ids", "num", "labels_out") + TABLES

NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def image_regions(labels: np.ndarray, connectivity: int) -> list[np.ndarray]:
    """The regions of one uint8 [H, W] map, by ascending anchor; each as its ascending linear indices."""
    h, w = labels.shape
    seen = labels == UNLABELED
    steps = NEIGHBOURS[connectivity]
    regions = []
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0]:
                continue
            v = labels[y0, x0]
            seen[y0, x0] = True
            stack, members = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                members.append(y * w + x)
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx] and labels[yy, xx] == v:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
            regions.append(np.sort(np.asarray(members, dtype=np.int64)))
    return regions


def peak_of(values: np.ndarray) -> int:
    """The position of the first element in the order of the searches: value descending (-0.0 == +0.0), NaN last, ties to
    the lower position."""
    numbers = ~np.isnan(values)
    if not numbers.any():
        return 0
    return int(np.flatnonzero(numbers & (values == values[numbers].max()))[0])


def label_regions_ref(labels: np.ndarray, best: np.ndarray | None = None, connectivity: int = 8, min_area: int = 1,
                      max_regions: int = 1024) -> dict[str, np.ndarray]:
    """Every output of isc_label_regions for uint8 [B, H, W] `labels` (peak and peak_score only with `best`)."""
    assert labels.dtype == np.uint8 and labels.ndim == 3 and connectivity in (4, 8) and min_area >= 1 and max_regions >= 1
    b, h, w = labels.shape
    r = max_regions
    out = {"ids": np.full((b, h, w), -1, np.int32), "num": np.zeros(b, np.int32),
           "labels_out": np.full((b, h, w), UNLABELED, np.uint8), "label": np.full((b, r), -1, np.int32),
           "area": np.zeros((b, r), np.int32), "anchor": np.full((b, r), -1, np.int32),
           "box": np.zeros((b, r, 4), np.int32), "sum": np.zeros((b, r, 2), np.int64)}
    if best is not None:
        assert best.dtype == np.float32 and best.shape == labels.shape
        out["peak"] = np.full((b, r), -1, np.int32)
        out["peak_score"] = np.full((b, r), -np.inf, np.float32)
    for i in range(b):
        kept = [m for m in image_regions(labels[i], connectivity) if len(m) >= min_area]
        out["num"][i] = len(kept)
        flat_ids, flat_out, flat_in = out["ids"][i].reshape(-1), out["labels_out"][i].reshape(-1), labels[i].reshape(-1)
        for k, m in enumerate(kept):
            flat_ids[m] = k
            flat_out[m] = flat_in[m]
            if k >= r:
                continue
            ys, xs = m // w, m % w
            out["label"][i, k] = flat_in[m[0]]
            out["area"][i, k] = len(m)
            out["anchor"][i, k] = m[0]
            out["box"][i, k] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
            out["sum"][i, k] = (ys.sum(), xs.sum())
            if best is not None:
                at = m[peak_of(best[i].reshape(-1)[m])]
                out["peak"][i, k] = at
                out["peak_score"][i, k] = best[i].reshape(-1)[at]
    return out


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal shapes, types and values; for floats equal signs of zero too, and a NaN equals a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


# ------------------------------------------------------------------------------------------------------ the test maps
def checkerboard(h: int, w: int) -> np.ndarray:
    y, x = np.mgrid[:h, :w]
    return ((y + x) % 2).astype(np.uint8)[None]


def serpentine(h: int, w: int, label: int = 3) -> np.ndarray:
    """A one-pixel path through the whole image: every other row full, joined alternately at the right and left end."""
    m = np.full((h, w), UNLABELED, np.uint8)
    m[0::2] = label
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = label
    return m[None]


def spiral(h: int, w: int, label: int = 5) -> np.ndarray:
    """A one-pixel spiral from the corner inwards, a one-pixel gap between its turns."""
    m = np.full((h, w), UNLABELED, np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = label
    for _ in range(4 * (h + w)):
        moved = False
        while True:
            yy, xx = y + dy, x + dx
            ahead = (yy + dy, xx + dx)
            if not (0 <= yy < h and 0 <= xx < w) or m[yy, xx] != UNLABELED:
                break
            if 0 <= ahead[0] < h and 0 <= ahead[1] < w and m[ahead] != UNLABELED:
                break
            y, x = yy, xx
            m[y, x] = label
            moved = True
        if not moved:
            break
        dy, dx = dx, -dy
    return m[None]


def random_map(shape: tuple[int, int, int], probabilities: list[float], seed: int, smooth: int = 0) -> np.ndarray:
    """uint8 `shape`, class c with probabilities[c], the rest unlabeled.  `smooth` > 0: classes are drawn on a grid
    `smooth` times coarser and repeated, then a tenth of the pixels is redrawn: large regions with speckle."""
    rng = np.random.default_rng(seed)
    p = np.asarray(probabilities + [1.0 - sum(probabilities)])
    values = np.asarray(list(range(len(probabilities))) + [UNLABELED], np.uint8)
    b, h, w = shape
    if not smooth:
        return values[rng.choice(len(p), size=shape, p=p)]
    coarse = values[rng.choice(len(p), size=(b, -(-h // smooth), -(-w // smooth)), p=p)]
    m = np.repeat(np.repeat(coarse, smooth, axis=1), smooth, axis=2)[:, :h, :w].copy()
    redraw = rng.random(shape) < 0.1
    m[redraw] = values[rng.choice(len(p), size=int(redraw.sum()), p=p)]
    return m
