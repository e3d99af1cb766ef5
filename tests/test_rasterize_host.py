"""The host side of polygon rasterisation, which needs no GPU: packing of every input form, snapping, scaling, every
error, and the oracle (tests/polygon_oracle.py) on the two mask cases recorded from the reference's geometry tests."""

from __future__ import annotations

import json
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import polygon_oracle as po
from imagescry_amd import PackedPolygons, _lib, pack_polygons, segmentation

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "roi_mask_cases.json").read_text())["cases"]

SQUARE = [(1, 1), (5, 1), (5, 4), (1, 4)]
HOLE = [(2, 2), (2, 3), (4, 3), (4, 2)]


class Ring:
    def __init__(self, coords: list) -> None:
        self.coords = coords


class Poly:
    """What pack_polygons needs of a shapely Polygon."""

    def __init__(self, exterior: list, interiors: list = ()) -> None:
        self.exterior = Ring(exterior)
        self.interiors = [Ring(r) for r in interiors]


class Multi:
    def __init__(self, *parts: Poly) -> None:
        self.geoms = list(parts)


def q(ring: list) -> list:
    return [[256 * x, 256 * y] for x, y in ring]


def test_every_shape_form_packs_to_the_same_arrays() -> None:
    closed = SQUARE + [SQUARE[0]]  # a repeated closing vertex, as shapely stores it
    forms = [
        [SQUARE, HOLE],
        [np.array(SQUARE, dtype=np.float32), torch.tensor(HOLE, dtype=torch.float64)],
        torch.tensor([SQUARE, HOLE]),
        Poly(SQUARE, [HOLE]),
        Multi(Poly(SQUARE), Poly(HOLE)),
    ]
    for form in forms:
        pack = pack_polygons([[form]])
        assert isinstance(pack, PackedPolygons) and len(pack) == 1 and pack.num_regions == 1
        assert pack.vertices.dtype == pack.ring_start.dtype == pack.ring_region.dtype == pack.image_start.dtype == torch.int32
        assert pack.vertices.tolist() == q(SQUARE) + q(HOLE)
        assert pack.ring_start.tolist() == [0, 4, 8] and pack.ring_region.tolist() == [0, 0]
        assert pack.image_start.tolist() == [0, 2]
    for one in (SQUARE, np.array(SQUARE), torch.tensor(SQUARE), Poly(SQUARE), [torch.tensor(SQUARE)],
                [torch.tensor(v) for v in SQUARE]):
        pack = pack_polygons([[one]])
        assert pack.vertices.tolist() == q(SQUARE) and pack.ring_start.tolist() == [0, 4]
    assert pack_polygons([[Poly(closed)]]).vertices.tolist() == q(closed)


def test_regions_are_places_in_the_image_list() -> None:
    pack = pack_polygons([[SQUARE, Poly(SQUARE, [HOLE]), HOLE], [], [HOLE]])
    assert len(pack) == 3 and pack.num_regions == 3
    assert pack.ring_region.tolist() == [0, 1, 1, 2, 0]
    assert pack.image_start.tolist() == [0, 4, 4, 5]
    assert pack.ring_start.tolist() == [0, 4, 8, 12, 16, 20]
    empty = pack_polygons([[], []])
    assert len(empty) == 2 and empty.num_regions == 1 and empty.vertices.shape == (0, 2)
    assert empty.ring_start.tolist() == [0] and empty.image_start.tolist() == [0, 0, 0]
    assert len(pack_polygons([])) == 0
    moved = pack.to("cpu")
    assert isinstance(moved, PackedPolygons) and moved.num_regions == 3 and moved.device.type == "cpu"


def test_snapping_rounds_halves_to_even() -> None:
    xs = [k / 512 for k in (1, 3, 5, 7, -1, -3, 255, 257)]  # q = k / 2: exactly between two integers
    ring = [(x, 0.0) for x in xs]
    got = pack_polygons([[ring]]).vertices[:, 0].tolist()
    assert got == [0, 2, 2, 4, 0, -2, 128, 128]
    assert pack_polygons([[[(0.001953125, 1), (0.3, 2.7), (3, 0.00390625)]]]).vertices.tolist() == [
        [0, 256], [77, 691], [768, 1]]  # 0.5 -> 0, 76.8 -> 77, 691.2 -> 691


def test_extent_scales_left_to_right_in_float64() -> None:
    pack = pack_polygons([[[(0, 0), (4, 0), (4, 3), (0, 3)]]], size=(3, 4), extent=(6, 8))
    assert pack.vertices.tolist() == [[0, 0], [512, 0], [512, 384], [0, 384]]
    ring = [(10.0, 7.0), (1.0, 2.0), (5.0, 9.5)]
    pack = pack_polygons([[ring]], size=(7, 5), extent=(9, 3))
    sx, sy = 5 / 3, 7 / 9
    want = [[int(np.rint(x * sx * 256.0)), int(np.rint(y * sy * 256.0))] for x, y in ring]
    assert pack.vertices.tolist() == want
    assert pack_polygons([[ring]], size=(7, 5)).vertices.tolist() == [[2560, 1792], [256, 512], [1280, 2432]]


def test_pack_errors() -> None:
    with pytest.raises(ValueError, match="at least 3"):
        pack_polygons([[[(0, 0), (1, 1)]]])
    with pytest.raises(ValueError, match="at least 3"):
        pack_polygons([[Poly(SQUARE, [[(0, 0), (1, 1)]])]])
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            pack_polygons([[[(0, 0), (1, bad), (2, 2)]]])
    assert pack_polygons([[[(32768, 0), (0, -32768), (1, 1)]]]).vertices[0].tolist() == [1 << 23, 0]  # the bound itself
    with pytest.raises(ValueError, match="beyond"):
        pack_polygons([[[(32768.01, 0), (0, 0), (1, 1)]]])
    with pytest.raises(ValueError, match="beyond"):
        pack_polygons([[[(100, 0), (0, 0), (1, 1)]]], size=(4, 4000), extent=(4, 10))  # 100 * 400 pixels
    with pytest.raises(ValueError, match=r"\[V, 2\]"):
        pack_polygons([[np.zeros((4, 3))]])
    with pytest.raises(ValueError, match="at least one ring"):
        pack_polygons([[[]]])
    with pytest.raises(ValueError, match="extent needs size"):
        pack_polygons([[SQUARE]], extent=(4, 4))
    with pytest.raises(ValueError):
        pack_polygons([[SQUARE]], size=(0, 4))
    with pytest.raises(TypeError):
        pack_polygons([[SQUARE]], size=(4.0, 4))
    with pytest.raises(TypeError):
        pack_polygons([[SQUARE]], size=(4, 4), extent="big")
    with pytest.raises(TypeError):
        pack_polygons(SQUARE[0])
    with pytest.raises(TypeError):
        pack_polygons([Poly(SQUARE)])  # an image's entry is a list of shapes
    with pytest.raises(TypeError):
        pack_polygons([[7]])
    with pytest.raises(TypeError):
        pack_polygons([[["ab", "cd", "ef"]]])


def test_rasterize_argument_errors_need_no_device() -> None:
    pack = pack_polygons([[SQUARE]])
    with pytest.raises(ValueError, match="fill_rule"):
        segmentation.rasterize_polygons(pack, (8, 8), fill_rule="odd")
    with pytest.raises(TypeError):
        segmentation.rasterize_polygons(pack, (8, 8), all_touched=1)
    with pytest.raises(TypeError):
        segmentation.rasterize_polygons(pack, (8, 8), return_counts=None)
    with pytest.raises(TypeError):
        segmentation.rasterize_polygons(pack, (8.0, 8))
    with pytest.raises(ValueError):
        segmentation.rasterize_polygons(pack, (0, 8))
    with pytest.raises(ValueError, match="32768"):
        segmentation.rasterize_polygons(pack, (1, 32769))
    with pytest.raises(ValueError, match="scaled already"):
        segmentation.rasterize_polygons(pack, (8, 8), extent=(16, 16))
    with pytest.raises(ValueError, match="num_regions"):
        segmentation.rasterize_polygons(pack, (8, 8), num_regions=0)
    with pytest.raises(TypeError):
        segmentation.rasterize_polygons(pack, (8, 8), num_regions=1.5)
    wrong = PackedPolygons(pack.vertices.to(torch.int64), pack.ring_start, pack.ring_region, pack.image_start, 1)
    with pytest.raises(TypeError, match="int32"):
        segmentation.rasterize_polygons(wrong, (8, 8))
    wrong = PackedPolygons(pack.vertices, pack.ring_start[:-1], pack.ring_region, pack.image_start, 1)
    with pytest.raises(ValueError, match="ring_start"):
        segmentation.rasterize_polygons(wrong, (8, 8))
    with pytest.raises(_lib.HipLibraryError):
        segmentation.rasterize_polygons(pack, (8, 8), device="cpu")  # there is no CPU path
    with pytest.raises(TypeError, match="class_index"):
        segmentation.create_roi_mask(SQUARE, (8, 8), (4, 4), class_index=1.0)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_oracle_reproduces_the_recorded_masks(case: dict) -> None:
    pack = pack_polygons([case["polygons"]], size=tuple(case["feature_map_shape"]),
                         extent=tuple(case["original_image_shape"]))
    ids = po.rasterize_packed(pack, tuple(case["feature_map_shape"]), all_touched=True)
    assert (ids[0] >= 0).astype(int).tolist() == case["expected"]


def test_oracle_edge_cases_by_hand() -> None:
    def ids(shapes: list, size: tuple, **kw: object) -> list:
        return po.rasterize_packed(pack_polygons([shapes]), size, **kw)[0].tolist()

    # a square with corners on pixel centres: the top-left rule keeps the left and top centres only
    assert ids([[(0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (0.5, 2.5)]], (3, 3)) == [[0, 0, -1], [0, 0, -1], [-1, -1, -1]]
    # a diagonal touches the pixels it runs through, not those it meets at a corner only; nor do edges on pixel borders
    assert ids([[(0, 0), (3, 3), (0, 0.0)]], (3, 3), all_touched=True) == [[0, -1, -1], [-1, 0, -1], [-1, -1, 0]]
    assert ids([[(1, 1), (2, 1), (2, 2), (1, 2)]], (3, 3), all_touched=True) == [[-1] * 3, [-1, 0, -1], [-1] * 3]
    # a sub-pixel triangle that misses its pixel's centre
    tri = [(1.1, 1.1), (1.4, 1.1), (1.1, 1.4)]
    assert ids([tri], (3, 3)) == [[-1] * 3] * 3
    assert ids([tri], (3, 3), all_touched=True) == [[-1] * 3, [-1, 0, -1], [-1] * 3]
    # the last shape wins
    assert ids([[(0, 0), (2, 0), (2, 2), (0, 2)], [(1, 0), (3, 0), (3, 2), (1, 2)]], (2, 3)) == [[0, 1, 1], [0, 1, 1]]
    # a hole is a hole under even-odd whatever its orientation; under non-zero only if it runs the other way
    outer, same, other = [(0, 0), (5, 0), (5, 5), (0, 5)], [(1, 1), (4, 1), (4, 4), (1, 4)], [(1, 1), (1, 4), (4, 4), (4, 1)]
    assert ids([[outer, same]], (5, 5))[2] == [0, -1, -1, -1, 0] == ids([[outer, other]], (5, 5))[2]
    assert ids([[outer, same]], (5, 5), fill_rule=po.NONZERO)[2] == [0] * 5
    assert ids([[outer, other]], (5, 5), fill_rule=po.NONZERO)[2] == [0, -1, -1, -1, 0]


def test_vectorised_oracle_equals_the_scalar_definition() -> None:
    rng = random.Random(11)
    for _ in range(12):
        height, width, rows = rng.randint(1, 9), rng.randint(1, 9), rng.randint(1, 3)
        verts, ring_start, ring_region = [], [0], []
        for _ in range(rng.randint(0, 5)):
            for _ in range(rng.choice([1, 2, 3, 4, 6])):
                far = rng.random() < 0.1
                verts.append((rng.choice([-2**31, 2**31 - 1, 2**23 + 9]) if far else 128 * rng.randint(-3, 2 * width + 3),
                              128 * rng.randint(-3, 2 * height + 3)))
            ring_start.append(len(verts))
            ring_region.append(rng.randint(-1, rows))
        image_start = [0, len(ring_region)]
        for fill in (po.EVENODD, po.NONZERO):
            for touch in (False, True):
                got = po.rasterize(verts, ring_start, ring_region, image_start, height, width, rows, fill, touch)
                for y in range(height):
                    for x in range(width):
                        want = po.pixel_region(verts, ring_start, ring_region, 0, len(ring_region), x, y, rows, fill, touch)
                        assert got[0, y, x] == want
