"""isc_rasterize_polygons on the GPU against its definition (tests/polygon_oracle.py), value for value: every case below
must give the oracle's ids exactly, and counts must be the histogram of the ids.  The shapes sit on the seams that
isc_rasterize_polygons_geometry reports; every call gets a workspace of 0xFF bytes."""

from __future__ import annotations

import ctypes
import json
import math
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import polygon_oracle as po
from imagescry_amd import PackedPolygons, _lib, create_roi_mask, pack_polygons, pool_polygons, pool_regions
from imagescry_amd import rasterize_polygons, segmentation

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "roi_mask_cases.json").read_text())["cases"]
Q = 256
Ring = list  # of (qx, qy)
Image = list  # of (region value, Ring)


def px(ring: list) -> Ring:
    """Pixel coordinates (multiples of 1/256) -> fixed point."""
    out = [(x * Q, y * Q) for x, y in ring]
    assert all(float(v).is_integer() for p in out for v in p)
    return [(int(x), int(y)) for x, y in out]


def arrays(images: list[Image]) -> tuple[list, list, list, list]:
    verts, ring_start, ring_region, image_start = [], [0], [], [0]
    for image in images:
        for value, ring in image:
            verts.extend(ring)
            ring_start.append(len(verts))
            ring_region.append(value)
        image_start.append(len(ring_region))
    return verts, ring_start, ring_region, image_start


def device_arrays(device: torch.device, images: list[Image]) -> list[torch.Tensor]:
    verts, ring_start, ring_region, image_start = arrays(images)
    verts = torch.tensor(verts, dtype=torch.int32).reshape(-1, 2)
    rest = [torch.tensor(v, dtype=torch.int32) for v in (ring_start, ring_region, image_start)]
    return [torch.cat([t.reshape(-1), torch.zeros(2, dtype=torch.int32)]).to(device) for t in (verts, *rest)]  # never empty


def run(device: torch.device, images: list[Image], size: tuple[int, int], rows: int, fill: int = po.EVENODD,
        touch: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """The C ABI itself -> (ids, counts)."""
    lib = _lib.load()
    verts, ring_start, ring_region, image_start = device_arrays(device, images)
    b = len(images)
    need = ctypes.c_size_t()
    assert lib.isc_rasterize_polygons_workspace_bytes(sum(len(i) for i in images), need) == _lib.ISC_OK
    workspace = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=device)
    ids = torch.full((b, *size), -7, dtype=torch.int32, device=device)
    counts = torch.full((b, rows), -7, dtype=torch.int32, device=device)
    st = lib.isc_rasterize_polygons(verts.data_ptr(), ring_start.data_ptr(), ring_region.data_ptr(), image_start.data_ptr(),
                                    b, size[0], size[1], rows, fill, int(touch), ids.data_ptr(), counts.data_ptr(),
                                    workspace.data_ptr(), need.value, _lib.stream_handle(device))
    assert st == _lib.ISC_OK
    return ids.cpu().numpy(), counts.cpu().numpy()


def histogram(ids: np.ndarray, rows: int) -> np.ndarray:
    return np.stack([np.bincount(image[image >= 0].ravel(), minlength=rows)[:rows] for image in ids]).astype(np.int32)


def check(device: torch.device, images: list[Image], size: tuple[int, int], rows: int,
          modes: tuple = ((po.EVENODD, False), (po.NONZERO, False), (po.EVENODD, True), (po.NONZERO, True))) -> dict:
    """Every mode against the oracle -> the ids by mode."""
    out = {}
    for fill, touch in modes:
        want = po.rasterize(*arrays(images), size[0], size[1], rows, fill, touch)
        got, counts = run(device, images, size, rows, fill, touch)
        wrong = np.argwhere(got != want)
        assert wrong.size == 0, (f"fill {fill} touch {touch}: {len(wrong)} pixels differ, the first at (b, y, x) = "
                                 f"{wrong[0].tolist()}: got {got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}")
        assert np.array_equal(counts, histogram(want, rows)), f"fill {fill} touch {touch}: counts"
        out[fill, touch] = got
    return out


@pytest.fixture(scope="module")
def geometry() -> tuple[int, int, int]:
    return segmentation.rasterize_geometry()


def circle(n: int, cx: float, cy: float, radius: float, seed: int) -> Ring:
    """A star-shaped ring of n distinct vertices (n edges), radii jittered, on the 1/256 lattice."""
    rng = random.Random(seed)
    return [(round((cx + radius * rng.uniform(0.6, 1.0) * math.cos(2 * math.pi * i / n)) * Q),
             round((cy + radius * rng.uniform(0.6, 1.0) * math.sin(2 * math.pi * i / n)) * Q)) for i in range(n)]


def test_rectangle_across_both_tile_seams(device, geometry) -> None:
    tw, th, _ = geometry
    rect = px([(tw - 2.5, th - 3), (tw + 0.75, th - 3), (tw + 0.75, th + 0.5), (tw - 2.5, th + 0.5)])
    got = check(device, [[(0, rect)]], (th + 1, tw + 1), 1)
    assert (got[po.EVENODD, False][0, th, tw - 2:] == 0).sum() == 0  # the last row's centres lie at th + 0.5: out
    assert (got[po.EVENODD, True][0, th, tw - 3:] == 0).all()  # ... but the row is touched
    big = px([(-5, -5), (2 * tw + 3, -5), (2 * tw + 3, 3 * th), (-5, 3 * th)])
    check(device, [[(1, big), (0, rect)]], (2 * th + 3, 2 * tw + 5), 2)


def test_degenerate_image_sizes(device, geometry) -> None:
    tw, th, _ = geometry
    tri = px([(-1, -1), (3 * tw, -1), (-1, 5 * th)])
    sliver = px([(0.25, 0.25), (2 * tw + 0.5, 0.75), (0.25, 0.75)])
    for size in ((1, 1), (1, 2 * tw + 7), (4 * th + 3, 1)):
        check(device, [[(0, tri)], [(0, sliver)]], size, 1)


def test_images_without_rings(device) -> None:
    square = px([(1, 1), (9, 1), (9, 6), (1, 6)])
    assert (check(device, [[]], (7, 11), 2)[po.EVENODD, True] == -1).all()
    got = check(device, [[(0, square)], [], [(1, square)]], (7, 11), 2)[po.EVENODD, False]
    assert (got[1] == -1).all() and got[0].max() == 0 and got[2].max() == 1


def test_centres_on_edges_and_vertices(device) -> None:
    square = px([(2.5, 1.5), (7.5, 1.5), (7.5, 5.5), (2.5, 5.5)])
    got = check(device, [[(0, square)]], (8, 10), 1)[po.EVENODD, False][0]
    assert got[1, 2] == 0 and got[1, 7] == -1 and got[5, 2] == -1 and got[4, 6] == 0 and (got >= 0).sum() == 20
    upper = px([(0.5, 0.5), (8.5, 0.5), (8.5, 8.5)])
    lower = px([(0.5, 0.5), (8.5, 8.5), (0.5, 8.5)])
    a = check(device, [[(0, upper), (1, lower)]], (10, 10), 2)[po.EVENODD, False][0]
    b = check(device, [[(1, lower), (0, upper)]], (10, 10), 2)[po.EVENODD, False][0]
    assert np.array_equal(a, b) and (a[0:8, 0:8] >= 0).all()  # the diagonal's centres belong to one triangle each
    assert [a[k, k] for k in range(8)] == [a[0, 0]] * 8


def test_triangle_mesh_partitions_the_image(device) -> None:
    height, width, step = 40, 70, 7
    rng = random.Random(3)
    nx, ny = width // step + 3, height // step + 3
    grid = {}
    for j in range(ny):
        for i in range(nx):
            x, y = (i - 1) * step * Q + rng.randint(-2 * Q, 2 * Q), (j - 1) * step * Q + rng.randint(-2 * Q, 2 * Q)
            if rng.random() < 0.4:  # onto a pixel centre
                x, y = x // Q * Q + Q // 2, y // Q * Q + Q // 2
            if i == 0 or j == 0 or i == nx - 1 or j == ny - 1:  # the rim stays outside the image
                x = -3 * Q if i == 0 else (width + 3) * Q if i == nx - 1 else x
                y = -3 * Q if j == 0 else (height + 3) * Q if j == ny - 1 else y
            grid[i, j] = (x, y)
    triangles = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = grid[i, j], grid[i + 1, j], grid[i + 1, j + 1], grid[i, j + 1]
            triangles += [[a, b, c], [a, c, d]] if rng.random() < 0.5 else [[a, b, d], [b, c, d]]
    image = [(r, tri) for r, tri in enumerate(triangles)]
    rows = len(triangles)
    for modes in (((po.EVENODD, False),), ((po.NONZERO, False),)):
        forward = check(device, [image], (height, width), rows, modes)[modes[0]]
        backward = check(device, [image[::-1]], (height, width), rows, modes)[modes[0]]
        assert (forward >= 0).all(), "a pixel lies in no triangle"
        assert np.array_equal(forward, backward), "a pixel lies in two triangles"


def test_pentagram_under_both_fill_rules(device) -> None:
    points = [(20 + 18 * math.sin(2 * math.pi * k * 2 / 5), 20 - 18 * math.cos(2 * math.pi * k * 2 / 5)) for k in range(5)]
    star = [(round(x * Q), round(y * Q)) for x, y in points]
    got = check(device, [[(0, star)]], (40, 41), 1)
    assert got[po.EVENODD, False][0, 20, 20] == -1 and got[po.NONZERO, False][0, 20, 20] == 0  # the core winds twice


def test_holes_of_either_orientation(device) -> None:
    outer = px([(1, 1), (30, 1), (30, 20), (1, 20)])
    same = px([(5, 5), (25.5, 5), (25.5, 15.5), (5, 15.5)])
    for hole in (same, same[::-1]):
        got = check(device, [[(0, outer), (0, hole)]], (22, 33), 1)
        assert got[po.EVENODD, False][0, 10, 10] == -1
        assert (got[po.NONZERO, False][0, 10, 10] == 0) == (hole is same)


def test_shape_of_two_disjoint_rings(device) -> None:
    left, right = px([(1, 1), (6, 2), (3, 9)]), px([(60, 3), (75, 3), (75, 14.5), (60, 14.5)])
    got = check(device, [[(0, left), (0, right), (1, px([(4, 4), (70, 5), (70, 6)]))]], (17, 80), 2)
    assert got[po.EVENODD, False][0, 10, 65] == 0


def test_rings_around_the_edge_chunk(device, geometry) -> None:
    chunk = geometry[2]
    for n in (chunk - 1, chunk, chunk + 1, 3 * chunk + 5):
        ring = circle(n, 45.3, 19.2, 18, seed=n)
        assert len(set(ring)) == n
        check(device, [[(0, ring)]], (40, 90), 1)


def test_state_survives_chunk_and_ring_boundaries_inside_a_shape(device, geometry) -> None:
    chunk = geometry[2]
    outer, hole = circle(chunk + 3, 40, 20, 19, seed=1), circle(2 * chunk - 1, 40, 20, 9, seed=2)
    dot = px([(39, 19), (41, 19), (41, 21), (39, 21)])
    check(device, [[(0, outer), (0, hole), (0, dot)], [(1, hole), (1, dot), (1, outer)]], (41, 83), 2)


def test_painters_order_runs_and_skipped_regions(device) -> None:
    a, b = px([(2, 2), (20, 2), (20, 12), (2, 12)]), px([(10, 5), (30, 5), (30, 16), (10, 16)])
    got = check(device, [[(0, a), (1, b)], [(1, b), (0, a)]], (18, 33), 2)[po.EVENODD, False]
    assert got[0, 8, 15] == 1 and got[1, 8, 15] == 0  # the last shape wins
    # one id in two separate runs: two shapes, so the overlap is covered, not cancelled
    got = check(device, [[(0, a), (1, b), (0, a)], [(0, a), (0, a)]], (18, 33), 2)[po.EVENODD, False]
    assert got[0, 8, 15] == 0 and got[0, 14, 25] == 1 and (got[1] == -1).all()
    # -1 and R are skipped, and still part two runs of one id
    got = check(device, [[(0, a), (-1, b), (0, a), (2, b), (5, a)]], (18, 33), 2)[po.EVENODD, False]
    assert got[0, 8, 15] == 0 and got[0, 14, 25] == -1
    check(device, [[(-1, a)], [(2, b)], [(1, b)]], (18, 33), 2)


def test_coordinates_at_and_beyond_the_bound(device) -> None:
    m = 1 << 23
    tri = [(-m, -m), (m, -m), (0, m)]
    assert (check(device, [[(0, tri)]], (9, 13), 1)[po.EVENODD, False] == 0).all()
    check(device, [[(0, [(m, m), (-m, 300), (700, -m)])]], (9, 13), 1)
    # through the C ABI, beyond the bound: the oracle clamps as the kernel must
    far = [(-(1 << 31), -(1 << 31)), ((1 << 31) - 1, -(1 << 31)), (m + 1, (1 << 31) - 1), (-m - 1, 5 * Q + 7)]
    check(device, [[(0, far)], [(0, [(m + 77, 3 * Q), (-3 * Q, -m - 5), (6 * Q, 8 * Q + 1)])]], (9, 13), 1)


def test_zero_length_collinear_and_horizontal_edges(device) -> None:
    square = px([(1, 1), (9, 1), (9, 1), (9, 6), (1, 6), (1, 6), (1, 6), (1, 1)])  # repeats, and the closing vertex
    check(device, [[(0, square)]], (8, 12), 1)
    line = px([(1.25, 1.25), (5.25, 3.25), (9.25, 5.25)])  # collinear: no area
    got = check(device, [[(0, line)]], (8, 12), 1)
    assert (got[po.EVENODD, False] == -1).all() and (got[po.NONZERO, False] == -1).all()
    assert (got[po.EVENODD, True] == 0).sum() >= 9
    flat = px([(1, 2.5), (10, 2.5), (10, 5.5), (6, 5.5), (6, 4.5), (3, 4.5), (3, 5.5), (1, 5.5)])  # edges on centre lines
    got = check(device, [[(0, flat)]], (8, 12), 1)[po.EVENODD, False][0]
    assert got[2, 5] == 0 and got[5, 5] == -1 and got[4, 4] == -1 and got[4, 7] == 0


def test_all_touched_boundaries(device) -> None:
    diagonal = px([(1, 1), (7, 7), (1, 1)])  # a segment through pixel corners
    got = check(device, [[(0, diagonal)]], (9, 9), 1)[po.EVENODD, True][0]
    assert [got[k, k] for k in range(9)] == [-1, 0, 0, 0, 0, 0, 0, -1, -1] and (got >= 0).sum() == 6
    border = px([(2, 2), (6, 2), (6, 5), (2, 5)])  # edges on pixel borders touch no neighbour
    got = check(device, [[(0, border)]], (8, 9), 1)
    assert np.array_equal(got[po.EVENODD, True], got[po.EVENODD, False]) and (got[po.EVENODD, True] >= 0).sum() == 12
    speck = px([(3.125, 4.125), (3.375, 4.125), (3.125, 4.375)])  # misses its pixel's centre
    got = check(device, [[(0, speck)]], (8, 9), 1)
    assert (got[po.EVENODD, False] == -1).all() and np.argwhere(got[po.EVENODD, True] == 0).tolist() == [[0, 4, 3]]
    segment = px([(1.5, 2.5), (4.25, 2.75), (1.5, 2.5)])  # ends inside a pixel
    got = check(device, [[(0, segment)]], (8, 9), 1)[po.EVENODD, True]
    assert np.argwhere(got == 0).tolist() == [[0, 2, 1], [0, 2, 2], [0, 2, 3], [0, 2, 4]]


def random_case(seed: int) -> tuple[list[Image], tuple[int, int], int]:
    rng = random.Random(seed)
    height, width, rows = rng.randint(1, 80), rng.randint(1, 80), rng.randint(1, 5)
    images = []
    for _ in range(rng.randint(1, 3)):
        image = []
        for _ in range(rng.randint(0, 6)):
            value = rng.randint(-1, rows)
            for _ in range(rng.choice([1, 1, 1, 2, 3])):  # rings of one shape
                ring = [(rng.randint(-20, 2 * width + 20) * (Q // 2), rng.randint(-20, 2 * height + 20) * (Q // 2))
                        for _ in range(rng.choice([3, 3, 4, 5, 8, 13]))]  # the half-pixel lattice, some outside
                image.append((value, ring))
        images.append(image)
    return images, (height, width), rows


@pytest.mark.parametrize("seed", range(20))
def test_random_polygons(device, seed: int) -> None:
    images, size, rows = random_case(seed)
    check(device, images, size, rows)


def test_batch_place_and_repeat_do_not_matter(device) -> None:
    images, size, rows = random_case(101)
    extra, _, _ = random_case(102)
    for mode in ((po.EVENODD, False), (po.NONZERO, True)):
        whole, whole_counts = run(device, images + extra + images[::-1], size, rows, *mode)
        again, again_counts = run(device, images + extra + images[::-1], size, rows, *mode)
        assert np.array_equal(whole, again) and np.array_equal(whole_counts, again_counts)
        n = len(images)
        for k, image in enumerate(images):
            alone, alone_counts = run(device, [image], size, rows, *mode)
            for place in (k, len(whole) - 1 - k):
                assert np.array_equal(alone[0], whole[place]) and np.array_equal(alone_counts[0], whole_counts[place])
        assert n >= 1


def test_graph_replay_after_refilling_the_polygons_in_place(device) -> None:
    size = (37, 70)
    sets = [[[circle(9, 20 + 7 * k, 15 + k, 12, seed=10 * k + 1), circle(5, 50 - 5 * k, 20, 14, seed=10 * k + 2)],
             [circle(9, 35, 18, 16 - k, seed=10 * k + 3), circle(5, 10 + 20 * k, 9, 8, seed=10 * k + 4)]] for k in range(3)]
    packs = [pack_polygons([[[(x / Q, y / Q) for x, y in ring] for ring in image] for image in polys]) for polys in sets]
    assert all(p.vertices.shape == packs[0].vertices.shape and torch.equal(p.ring_start, packs[0].ring_start) for p in packs)
    want = [po.rasterize_packed(p, size, all_touched=True) for p in packs]
    assert not np.array_equal(want[0], want[1])
    live = packs[0].to(device)
    live = PackedPolygons(live.vertices.clone(), live.ring_start.clone(), live.ring_region.clone(), live.image_start.clone(),
                          live.num_regions)
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        rasterize_polygons(live, size, all_touched=True, return_counts=True)  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ids, counts = rasterize_polygons(live, size, all_touched=True, return_counts=True)
    for i in (1, 2, 0, 1):
        live.vertices.copy_(packs[i].vertices)  # refilled in place
        ids.fill_(-9)
        counts.fill_(-9)  # garbage where the graph has to start from zero
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), want[i]), f"replay on polygons {i}"
        assert np.array_equal(counts.cpu().numpy(), histogram(want[i], live.num_regions))


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_create_roi_mask_on_the_recorded_cases(device, case: dict) -> None:
    roi = case["polygons"][0] if case["single"] else case["polygons"]
    mask = create_roi_mask(roi, tuple(case["original_image_shape"]), tuple(case["feature_map_shape"]), device=device)
    assert mask.dtype == torch.int64 and mask.device.type == "cuda" and mask.cpu().tolist() == case["expected"]
    mask = create_roi_mask(roi, case["original_image_shape"], case["feature_map_shape"], class_index=7, device=device)
    assert mask.cpu().tolist() == [[7 * v for v in row] for row in case["expected"]]


def test_rasterize_polygons_with_extent(device) -> None:
    shapes = [[[(3.0, 2.0), (90.5, 7.25), (60.0, 55.0)], [[(10, 30), (40, 30), (40, 58), (10, 58)], [(20, 35), (30, 35), (25, 50)]]],
              [torch.tensor([(0.0, 0.0), (100.0, 0.0), (50.0, 60.0)])]]
    size, extent = (23, 41), (60, 100)
    pack = pack_polygons(shapes, size=size, extent=extent)
    for fill, rule in ((po.EVENODD, "evenodd"), (po.NONZERO, "nonzero")):
        for touch in (False, True):
            want = po.rasterize_packed(pack, size, fill_rule=fill, all_touched=touch)
            ids, counts = rasterize_polygons(shapes, size, extent=extent, fill_rule=rule, all_touched=touch,
                                             return_counts=True, device=device)
            assert ids.dtype == torch.int32 and counts.shape == (2, 2) and np.array_equal(ids.cpu().numpy(), want)
            assert np.array_equal(counts.cpu().numpy(), histogram(want, 2))
            assert torch.equal(rasterize_polygons(pack, size, fill_rule=rule, all_touched=touch, device=device), ids)
            assert torch.equal(rasterize_polygons(pack.to(device), size, fill_rule=rule, all_touched=touch), ids)
    one = rasterize_polygons(pack, size, num_regions=1, device=device)  # shapes at or beyond R are skipped
    assert int(one.max()) == 0 and torch.equal(one == 0, rasterize_polygons(
        [[shapes[0][0]], shapes[1]], size, extent=extent, device=device) == 0)


def test_pool_polygons_is_pool_regions_of_the_oracle_ids(device) -> None:
    shapes = [[[(3.0, 2.0), (90.5, 7.25), (60.0, 55.0)], [(10, 30), (40, 30), (40, 58), (10, 58)]],
              [[(0.0, 0.0), (100.0, 0.0), (50.0, 60.0)]]]
    size, extent = (45, 75), (60, 100)
    maps = torch.randn((2, 24, 4, 6), generator=torch.Generator().manual_seed(5)).to(device)
    pack = pack_polygons(shapes, size=size, extent=extent)
    for touch in (False, True):
        want_ids = torch.from_numpy(po.rasterize_packed(pack, size, all_touched=touch)).to(device)
        for normalize in (True, False):
            want = pool_regions(maps, want_ids, 2, normalize=normalize)
            got = pool_polygons(maps, shapes, size, extent=extent, all_touched=touch, normalize=normalize)
            assert torch.equal(got.vectors.view(torch.int32), want.vectors.view(torch.int32))
            assert torch.equal(got.mass, want.mass) and int(got.mass[1, 1]) == 0 and int(got.mass[0, 1]) > 0
    packed = pool_polygons(maps, pack, size)
    assert torch.equal(packed.vectors, pool_polygons(maps, shapes, size, extent=extent).vectors)
