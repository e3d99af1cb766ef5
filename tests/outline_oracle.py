"""The definition of isc_trace_regions (include/imagescry_hip.h) in plain numpy and Python: a dict of directed boundary
edges, the successor of each, the cycles, their corners.  Slow and obviously right; tests/test_outline_host.py holds it
to tests/polygon_oracle.py (the round trip), tests/regions_oracle.py (anchors, boxes, areas) and scipy (holes).  It knows
nothing of nodes, leaders, chunks or pointer jumping: what the kernels save must not show.  Reads nothing outside the
repository."""

from __future__ import annotations

import numpy as np

# side -> (from, to) as offsets (dx, dy) from the pixel's top-left vertex, and the direction (dx, dy) of travel
SIDES = (((0, 0), (1, 0), (1, 0)), ((1, 0), (1, 1), (0, 1)), ((1, 1), (0, 1), (-1, 0)), ((0, 1), (0, 0), (0, -1)))
ACROSS = ((-1, 0), (0, 1), (1, 0), (0, -1))  # (dy, dx) of the neighbour across side s
OUTPUTS = ("vertices", "ring_start", "ring_region", "image_start", "ring_area2", "num_rings", "num_vertices")


def image_edges(ids: np.ndarray, num_regions: int) -> dict[int, tuple[int, tuple[int, int], tuple[int, int], int]]:
    """key -> (region, from, to, side) of every boundary edge of one int32 [H, W] image."""
    h, w = ids.shape
    edges = {}
    for y in range(h):
        for x in range(w):
            r = int(ids[y, x])
            if not 0 <= r < num_regions:
                continue
            for s, ((ax, ay), (bx, by), _) in enumerate(SIDES):
                yy, xx = y + ACROSS[s][0], x + ACROSS[s][1]
                if 0 <= yy < h and 0 <= xx < w and ids[yy, xx] == r:
                    continue
                edges[4 * (y * w + x) + s] = (r, (x + ax, y + ay), (x + bx, y + by), s)
    return edges


def successors(edges: dict, connectivity: int) -> dict[int, int]:
    """The successor of every edge: the edge of the same region that starts where it ends; at a saddle the edge of the
    same pixel (4) or of the other pixel (8)."""
    starts: dict[tuple[int, tuple[int, int]], list[int]] = {}
    for key, (r, a, _, _) in edges.items():
        starts.setdefault((r, a), []).append(key)
    succ = {}
    for key, (r, _, b, _) in edges.items():
        options = starts[(r, b)]
        if len(options) == 1:
            succ[key] = options[0]
            continue
        assert len(options) == 2, "a vertex starts at most two edges of one region"
        same = [k for k in options if k // 4 == key // 4]
        other = [k for k in options if k // 4 != key // 4]
        assert len(same) == 1 and len(other) == 1
        succ[key] = same[0] if connectivity == 4 else other[0]
    return succ


def image_rings(ids: np.ndarray, num_regions: int, connectivity: int) -> list[dict]:
    """The rings of one image in the order of the definition, each {"region", "vertices" [(x, y)], "area2", "keys"}."""
    edges = image_edges(ids, num_regions)
    succ = successors(edges, connectivity)
    assert sorted(succ.values()) == sorted(edges), "the successor map is a permutation"
    pred = {v: k for k, v in succ.items()}
    seen: set[int] = set()
    rings = []
    for first in sorted(edges):
        if first in seen:
            continue
        cycle, k = [], first
        while k not in seen:
            seen.add(k)
            cycle.append(k)
            k = succ[k]
        corners = [edges[k][1] for k in cycle if SIDES[edges[pred[k]][3]][2] != SIDES[edges[k][3]][2]]
        at = min(range(len(corners)), key=lambda i: (corners[i][1], corners[i][0]))
        corners = corners[at:] + corners[:at]
        n = len(corners)
        area2 = sum(corners[i][0] * corners[(i + 1) % n][1] - corners[(i + 1) % n][0] * corners[i][1] for i in range(n))
        rings.append({"region": edges[first][0], "vertices": corners, "area2": area2, "keys": cycle})
    rings.sort(key=lambda ring: (ring["region"], ring["vertices"][0][1], ring["vertices"][0][0]))
    return rings


def trace_regions_ref(ids: np.ndarray, num_regions: int, connectivity: int, max_rings: int,
                      max_vertices: int) -> dict[str, np.ndarray]:
    """Every output of isc_trace_regions for int32 [B, H, W] `ids`.  `vertices` is zeros where the call leaves it
    untouched; `written` marks the rows it writes."""
    assert ids.dtype == np.int32 and ids.ndim == 3 and connectivity in (4, 8)
    b = ids.shape[0]
    n, v = max_rings, max_vertices
    out = {"vertices": np.zeros((b, v, 2), np.int32), "written": np.zeros((b, v), bool),
           "ring_start": np.zeros(b * (n + 1) + 1, np.int32), "ring_region": np.full((b, n + 1), -1, np.int32),
           "image_start": np.arange(b + 1, dtype=np.int32) * (n + 1), "ring_area2": np.zeros((b, n), np.int64),
           "num_rings": np.zeros(b, np.int32), "num_vertices": np.zeros(b, np.int32)}
    out["ring_start"][-1] = b * v
    for i in range(b):
        rings = image_rings(ids[i], num_regions, connectivity)
        out["num_rings"][i] = len(rings)
        out["num_vertices"][i] = sum(len(ring["vertices"]) for ring in rings)
        if len(rings) > n or out["num_vertices"][i] > v:
            rings = []
        at = i * v
        for j in range(n + 1):
            out["ring_start"][i * (n + 1) + j] = at
            if j < len(rings):
                pts = np.asarray(rings[j]["vertices"], np.int32) * 256
                out["vertices"][i, at - i * v:at - i * v + len(pts)] = pts
                out["written"][i, at - i * v:at - i * v + len(pts)] = True
                out["ring_region"][i, j] = rings[j]["region"]
                out["ring_area2"][i, j] = rings[j]["area2"]
                at += len(pts)
    return out


def shapes_ref(ids: np.ndarray, num_regions: int, connectivity: int) -> list[list[list[np.ndarray]]]:
    """What RegionOutlines.shapes() returns: per image and region the rings as float64 [n, 2] of (x, y)."""
    out = []
    for image in ids:
        per_region: list[list[np.ndarray]] = [[] for _ in range(num_regions)]
        for ring in image_rings(image, num_regions, connectivity):
            per_region[ring["region"]].append(np.asarray(ring["vertices"], np.float64))
        out.append(per_region)
    return out


# ------------------------------------------------------------------------------------------------------ the test maps
def random_ids(shape: tuple[int, ...], num_regions: int, seed: int, fill: float = 0.6) -> np.ndarray:
    """int32 `shape`: ids in [-2, R + 1], so that values on both sides of [0, R) occur; `fill` of them inside."""
    rng = np.random.default_rng(seed)
    inside = rng.integers(0, num_regions, size=shape)
    outside = rng.choice(np.asarray([-2, -1, num_regions, num_regions + 1]), size=shape)
    return np.where(rng.random(shape) < fill, inside, outside).astype(np.int32)


def checkerboard_ids(h: int, w: int, regions: int) -> np.ndarray:
    """One region on the even squares (the odd ones -1), or two regions."""
    y, x = np.mgrid[:h, :w]
    odd = (y + x) % 2
    return np.where(odd == 0, 0, 1 if regions == 2 else -1).astype(np.int32)


def nested_ids(h: int = 13, w: int = 15) -> np.ndarray:
    """Region 0 as a ring with a hole, region 1 as an island in the hole, and a pixel of region 0 inside a hole of that
    island: an island of the SAME id in the hole."""
    m = np.full((h, w), -1, np.int32)
    m[1:h - 1, 1:w - 1] = 0
    m[3:h - 3, 3:w - 3] = -1
    m[4:h - 4, 4:w - 4] = 1
    m[5:h - 5, 5:w - 5] = -1
    m[6, 7] = 0
    return m
