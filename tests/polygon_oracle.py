"""isc_rasterize_polygons by its definition (include/imagescry_hip.h): the only yardstick for the kernel.

`pixel_region` is the definition itself in plain Python integers, one pixel and one edge at a time; `rasterize` is the
same arithmetic in numpy int64 (every difference fits 2^25 and every product 2^50), one edge at a time over all pixels
of an image, so that whole test images stay affordable.  tests/test_rasterize_host.py holds the two to each other.
Neither skips a ring, drops an edge or knows about tiles: what the kernel saves must not show."""

from __future__ import annotations

import numpy as np

MAX_COORD = 1 << 23
EVENODD, NONZERO = 0, 1


def clamp(q: int) -> int:
    """The load-time clamp of a coordinate."""
    return min(max(int(q), -MAX_COORD), MAX_COORD)


def shapes_of(ring_region: list[int], first: int, last: int, num_regions: int) -> list[tuple[int, list[int]]]:
    """The shapes of rings [first, last): maximal runs of equal ring_region values as (region, rings); a run whose value
    is outside [0, R) is dropped after it has separated its neighbours."""
    runs: list[tuple[int, list[int]]] = []
    for r in range(first, last):
        value = int(ring_region[r])
        if runs and runs[-1][0] == value and runs[-1][1][-1] == r - 1:
            runs[-1][1].append(r)
        else:
            runs.append((value, [r]))
    return [(value, rings) for value, rings in runs if 0 <= value < num_regions]


def ring_edges(vertices, ring_start, r: int) -> list[tuple[int, int, int, int]]:
    """The edges (Ax, Ay, Bx, By) of ring r, clamped, without those of zero length."""
    s, e = int(ring_start[r]), int(ring_start[r + 1])
    pts = [(clamp(vertices[i][0]), clamp(vertices[i][1])) for i in range(s, e)]
    out = []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        if a != b:
            out.append((a[0], a[1], b[0], b[1]))
    return out


def edge_covers(edge: tuple[int, int, int, int], x: int, y: int) -> tuple[int, int, bool]:
    """(crossings, winding, touches) of one edge for pixel (y, x), in Python integers."""
    ax, ay, bx, by = edge
    cx, cy = 256 * x + 128, 256 * y + 128
    d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    cross = wind = 0
    if ay <= cy < by and d > 0:
        cross, wind = 1, 1
    elif by <= cy < ay and d < 0:
        cross, wind = 1, -1
    x0, x1, y0, y1 = 256 * x, 256 * x + 256, 256 * y, 256 * y + 256
    corners = [(bx - ax) * (py - ay) - (by - ay) * (qx - ax) for qx in (x0, x1) for py in (y0, y1)]
    touch = (min(ax, bx) < x1 and max(ax, bx) > x0 and min(ay, by) < y1 and max(ay, by) > y0
             and min(corners) < 0 and max(corners) > 0)
    return cross, wind, touch


def pixel_region(vertices, ring_start, ring_region, first: int, last: int, x: int, y: int, num_regions: int,
                 fill_rule: int, all_touched: bool) -> int:
    """The id of pixel (y, x) of an image that owns rings [first, last)."""
    winner = -1
    for region, rings in shapes_of(ring_region, first, last, num_regions):
        cross = wind = 0
        touched = False
        for r in rings:
            for edge in ring_edges(vertices, ring_start, r):
                c, w, t = edge_covers(edge, x, y)
                cross += c
                wind += w
                touched = touched or t
        inside = wind != 0 if fill_rule == NONZERO else cross % 2 == 1
        if inside or (all_touched and touched):
            winner = region
    return winner


def rasterize_image(vertices, ring_start, ring_region, first: int, last: int, height: int, width: int, num_regions: int,
                    fill_rule: int, all_touched: bool) -> np.ndarray:
    """int32 [H, W]: `pixel_region` of every pixel, an edge at a time in int64."""
    x0 = (256 * np.arange(width, dtype=np.int64))[None, :]
    y0 = (256 * np.arange(height, dtype=np.int64))[:, None]
    cx, cy = x0 + 128, y0 + 128
    out = np.full((height, width), -1, dtype=np.int32)
    for region, rings in shapes_of(ring_region, first, last, num_regions):
        cross = np.zeros((height, width), dtype=np.int64)
        wind = np.zeros((height, width), dtype=np.int64)
        touched = np.zeros((height, width), dtype=bool)
        for r in rings:
            for ax, ay, bx, by in ring_edges(vertices, ring_start, r):
                dx, dy = np.int64(bx - ax), np.int64(by - ay)
                d = dx * (cy - ay) - dy * (cx - ax)
                up = (ay <= cy) & (cy < by) & (d > 0)
                down = (by <= cy) & (cy < ay) & (d < 0)
                cross += up.astype(np.int64) + down.astype(np.int64)
                wind += up.astype(np.int64) - down.astype(np.int64)
                if all_touched:
                    corners = [dx * (py - ay) - dy * (qx - ax) for qx in (x0, x0 + 256) for py in (y0, y0 + 256)]
                    low = np.minimum(np.minimum(corners[0], corners[1]), np.minimum(corners[2], corners[3]))
                    high = np.maximum(np.maximum(corners[0], corners[1]), np.maximum(corners[2], corners[3]))
                    touched |= ((min(ax, bx) < x0 + 256) & (max(ax, bx) > x0) & (min(ay, by) < y0 + 256)
                                & (max(ay, by) > y0) & (low < 0) & (high > 0))
        inside = wind != 0 if fill_rule == NONZERO else cross % 2 == 1
        out[inside | touched] = region
    return out


def rasterize(vertices, ring_start, ring_region, image_start, height: int, width: int, num_regions: int,
              fill_rule: int = EVENODD, all_touched: bool = False) -> np.ndarray:
    """int32 [B, H, W] from the four arrays of the C ABI (numpy arrays or nested lists)."""
    vertices = np.asarray(vertices, dtype=np.int64).reshape(-1, 2).tolist()
    ring_start = [int(v) for v in np.asarray(ring_start).reshape(-1)]
    ring_region = [int(v) for v in np.asarray(ring_region).reshape(-1)]
    image_start = [int(v) for v in np.asarray(image_start).reshape(-1)]
    images = [rasterize_image(vertices, ring_start, ring_region, image_start[b], image_start[b + 1], height, width,
                              num_regions, fill_rule, all_touched) for b in range(len(image_start) - 1)]
    return np.stack(images) if images else np.zeros((0, height, width), dtype=np.int32)


def rasterize_packed(pack, size: tuple[int, int], num_regions: int | None = None, fill_rule: int = EVENODD,
                     all_touched: bool = False) -> np.ndarray:
    """`rasterize` of a `PackedPolygons`."""
    return rasterize(pack.vertices.cpu().numpy(), pack.ring_start.cpu().numpy(), pack.ring_region.cpu().numpy(),
                     pack.image_start.cpu().numpy(), size[0], size[1], pack.num_regions if num_regions is None else num_regions,
                     fill_rule, all_touched)
