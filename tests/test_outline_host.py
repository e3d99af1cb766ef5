"""tests/outline_oracle.py proves itself, without a GPU: the round trip through tests/polygon_oracle.py under both fill
rules, the rings of connected regions against tests/regions_oracle.py (anchor, box, area), hole counts against scipy, the
facts about a ring's smallest edge key that the kernels lean on, the worst-case counts and the layout of the arrays; and
the parts of imagescry_amd.segmentation's outline layer that need no device."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import outline_oracle as oo  # noqa: E402
import polygon_oracle as po  # noqa: E402
import regions_oracle as ro  # noqa: E402

from imagescry_amd import PackedPolygons, RegionOutlines, Regions, pack_polygons, trace_regions  # noqa: E402

SIZES = ((1, 1), (1, 7), (6, 1), (2, 2), (5, 8), (11, 11), (9, 4))


def round_trip(ids: np.ndarray, rows: int, connectivity: int) -> None:
    ref = oo.trace_regions_ref(ids, rows, connectivity, ids[0].size, 4 * ids[0].size)
    want = np.where((ids >= 0) & (ids < rows), ids, -1)
    for fill in (po.EVENODD, po.NONZERO):
        got = po.rasterize(ref["vertices"].reshape(-1, 2), ref["ring_start"], ref["ring_region"].reshape(-1),
                           ref["image_start"], ids.shape[1], ids.shape[2], rows, fill)
        assert np.array_equal(got, want), (connectivity, fill)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_rasterising_the_rings_gives_back_the_ids(connectivity: int) -> None:
    for seed in range(40):
        h, w = SIZES[seed % len(SIZES)]
        rows = 1 + seed % 3
        round_trip(oo.random_ids((2, h, w), rows, seed), rows, connectivity)
    round_trip(oo.nested_ids()[None], 2, connectivity)
    for regions in (1, 2):
        round_trip(oo.checkerboard_ids(6, 7, regions)[None], 2, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_rings_of_connected_regions_match_their_tables(connectivity: int) -> None:
    labels = ro.random_map((2, 17, 23), [0.35, 0.3, 0.2], seed=5 + connectivity, smooth=3)
    regions = ro.label_regions_ref(labels, connectivity=connectivity, max_regions=512)
    for b in range(labels.shape[0]):
        num = int(regions["num"][b])
        assert 5 < num <= 512
        rings = oo.image_rings(regions["ids"][b], num, connectivity)
        for r in range(num):
            mine = [ring for ring in rings if ring["region"] == r]
            outer = [ring for ring in mine if ring["area2"] > 0]
            assert len(outer) == 1 and mine[0] is outer[0], "one positive ring a region, and it comes first"
            anchor = int(regions["anchor"][b, r])
            assert outer[0]["vertices"][0] == (anchor % 23, anchor // 23)
            xs, ys = zip(*outer[0]["vertices"])
            assert (min(ys), min(xs), max(ys), max(xs)) == tuple(regions["box"][b, r])
            assert sum(ring["area2"] for ring in mine) == 2 * int(regions["area"][b, r])
            assert all(len(ring["vertices"]) >= 4 for ring in mine)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_holes_are_the_enclosed_components_of_the_complement(connectivity: int) -> None:
    ndimage = pytest.importorskip("scipy.ndimage")
    dual = ndimage.generate_binary_structure(2, 1) if connectivity == 8 else np.ones((3, 3), int)
    for seed in range(12):
        mask = np.random.default_rng(seed).random((12, 14)) < 0.62
        ids = np.where(mask, 0, -1).astype(np.int32)
        rings = oo.image_rings(ids, 1, connectivity)
        comp, n = ndimage.label(~mask, structure=dual)
        border = set(comp[0]) | set(comp[-1]) | set(comp[:, 0]) | set(comp[:, -1])
        enclosed = [k for k in range(1, n + 1) if k not in border]
        assert sum(ring["area2"] < 0 for ring in rings) == len(enclosed)
        own = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
        assert sum(ring["area2"] > 0 for ring in rings) == ndimage.label(mask, structure=own)[1]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_smallest_edge_key_tells_the_start_vertex_and_the_sign(connectivity: int) -> None:
    seen = {True: 0, False: 0}
    for seed in range(60):
        h, w = SIZES[seed % len(SIZES)]
        rows = 1 + seed % 2  # one dense region: holes also where connectivity 4 makes them rare
        ids = oo.random_ids((h, w), rows, 100 + seed, fill=0.6 if rows == 2 else 0.85)
        edges = oo.image_edges(ids, rows)
        rings = oo.image_rings(ids, rows, connectivity)
        assert sorted(k for ring in rings for k in ring["keys"]) == sorted(edges)  # the cycles partition the edges
        starts = [(ring["region"], ring["vertices"][0]) for ring in rings]
        assert len(set(starts)) == len(starts), "two rings of one region never share a start vertex"
        for ring in rings:
            _, a, b, side = edges[min(ring["keys"])]
            positive = ring["area2"] > 0
            assert ring["area2"] != 0 and side == (0 if positive else 2)
            assert (a if positive else b) == ring["vertices"][0]
            seen[positive] += 1
    assert min(seen.values()) > 20


def test_checkerboards_reach_the_bounds() -> None:
    h, w = 6, 8
    two = oo.trace_regions_ref(oo.checkerboard_ids(h, w, 2)[None], 2, 4, h * w, 4 * h * w)
    assert two["num_rings"][0] == h * w and two["num_vertices"][0] == 4 * h * w
    assert (two["ring_area2"] == 2).all()
    joined = oo.trace_regions_ref(oo.checkerboard_ids(h, w, 1)[None], 1, 8, h * w, 4 * h * w)
    assert joined["num_vertices"][0] == 2 * h * w and joined["num_rings"][0] < h * w // 2


def test_layout_and_the_image_that_does_not_fit() -> None:
    ids = np.stack([oo.nested_ids(), np.full((13, 15), 1, np.int32), oo.nested_ids()])
    full = oo.trace_regions_ref(ids, 2, 8, 9, 40)
    n, v = 9, 40
    assert full["num_rings"].tolist() == [5, 1, 5] and full["num_vertices"].tolist() == [20, 4, 20]
    assert full["ring_region"][0].tolist() == [0, 0, 0, 1, 1, -1, -1, -1, -1, -1]
    assert full["ring_area2"][0].tolist() == [2 * 11 * 13, -2 * 7 * 9, 2, 2 * 5 * 7, -2 * 3 * 5, 0, 0, 0, 0]
    assert full["ring_start"][:n + 1].tolist() == [0, 4, 8, 12, 16, 20, 20, 20, 20, 20]
    assert full["ring_start"][n + 1:2 * n + 2].tolist() == [v, v + 4] + [v + 4] * 8 and full["ring_start"][-1] == 3 * v
    assert full["image_start"].tolist() == [0, 10, 20, 30]
    assert full["vertices"][1, :4].tolist() == [[0, 0], [15 * 256, 0], [15 * 256, 13 * 256], [0, 13 * 256]]
    assert full["vertices"][0, 4:8].tolist() == [[3 * 256, 3 * 256], [3 * 256, 10 * 256], [12 * 256, 10 * 256],
                                                 [12 * 256, 3 * 256]]  # a hole runs the other way round
    for n2, v2 in ((4, 40), (9, 19)):
        short = oo.trace_regions_ref(ids, 2, 8, n2, v2)
        assert short["num_rings"].tolist() == [5, 1, 5] and short["num_vertices"].tolist() == [20, 4, 20]
        assert (short["ring_region"][0] == -1).all() and (short["ring_area2"][0] == 0).all()
        assert (short["ring_start"][:n2 + 1] == 0).all() and not short["written"][0].any()
        assert short["ring_region"][1].tolist() == [1] + [-1] * n2 and short["written"][1].sum() == 4
    saddle = np.asarray([[[0, -1], [-1, 0]]], np.int32)
    assert oo.trace_regions_ref(saddle, 1, 4, 4, 16)["num_rings"][0] == 2
    one = oo.trace_regions_ref(saddle, 1, 8, 4, 16)
    assert one["num_rings"][0] == 1 and one["num_vertices"][0] == 8 and one["ring_area2"][0, 0] == 4
    assert (one["vertices"][0, :8] // 256).tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]


# ------------------------------------------------------------------------------------------------- the Python surface
def outlines_of(ids: np.ndarray, rows: int, connectivity: int, n: int, v: int) -> RegionOutlines:
    ref = oo.trace_regions_ref(ids, rows, connectivity, n, v)
    t = {k: torch.from_numpy(a) for k, a in ref.items()}
    pack = PackedPolygons(t["vertices"].reshape(-1, 2), t["ring_start"], t["ring_region"].reshape(-1), t["image_start"], rows)
    return RegionOutlines(pack, t["ring_area2"], t["num_rings"], t["num_vertices"], tuple(ids.shape[1:]), n, v)


def test_shapes_complete_and_holes_on_the_host() -> None:
    ids = np.stack([oo.nested_ids(), np.full((13, 15), 1, np.int32)])
    out = outlines_of(ids, 2, 8, 6, 64)
    assert len(out) == 2 and out.device.type == "cpu" and out.cpu().size == (13, 15)
    assert out.complete().tolist() == [True, True]
    assert out.holes()[0].tolist() == [False, True, False, False, True, False]
    shapes = out.shapes()
    want = oo.shapes_ref(ids, 2, 8)
    assert [[len(r) for r in image] for image in shapes] == [[3, 2], [0, 1]]
    for got_image, want_image in zip(shapes, want):
        for got_rings, want_rings in zip(got_image, want_image):
            assert all(g.dtype == np.float64 and np.array_equal(g, w) for g, w in zip(got_rings, want_rings))
    pack = pack_polygons([[s for s in image if s] for image in shapes])  # a non-empty entry is a shape
    assert pack.ring_region.tolist() == [0, 0, 0, 1, 1, 0]
    short = outlines_of(ids, 2, 8, 4, 64)
    assert short.complete().tolist() == [False, True]
    with pytest.raises(ValueError, match="image 0 has 5 rings"):
        short.shapes()
    assert [[len(r) for r in image] for image in short.shapes(strict=False)] == [[0, 0], [0, 1]]
    with pytest.raises(TypeError):
        short.shapes(strict=1)


def test_argument_checks_come_before_the_device() -> None:
    ids = torch.zeros((2, 5, 6), dtype=torch.int32)
    with pytest.raises(TypeError, match="torch.Tensor"):
        trace_regions(ids.numpy(), 3)
    with pytest.raises(TypeError, match="int32"):
        trace_regions(ids.to(torch.int64), 3)
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        trace_regions(ids[0], 3)
    with pytest.raises(ValueError, match="num_regions"):
        trace_regions(ids, 0)
    with pytest.raises(TypeError, match="num_regions"):
        trace_regions(ids, 2.0)
    with pytest.raises(ValueError, match="connectivity"):
        trace_regions(ids, 3, connectivity=6)
    with pytest.raises(TypeError, match="connectivity"):
        trace_regions(ids, 3, connectivity=True)
    with pytest.raises(ValueError, match="max_rings"):
        trace_regions(ids, 3, max_rings=0)
    with pytest.raises(TypeError, match="max_vertices"):
        trace_regions(ids, 3, max_vertices="many")
    with pytest.raises(ValueError, match="2\\^31"):
        trace_regions(ids, 3, max_vertices=2**30)
    with pytest.raises(Exception, match="no CPU fallback"):
        trace_regions(ids, 3)
    assert hasattr(Regions, "outlines")
