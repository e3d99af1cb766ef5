"""tests/regions_oracle.py against scipy.ndimage.label and against cases worked out by hand, and the parts of
imagescry_amd.segmentation's region layer that need no device: `Regions.centroids`, `Regions.peak_cells` and the argument
checks of `label_regions`."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import regions_oracle as ro  # noqa: E402

from imagescry_amd import LabelMaps, Regions, label_regions, segmentation  # noqa: E402


# ---------------------------------------------------------------------------------------------------- oracle vs scipy
@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_equals_scipy_per_class(connectivity: int) -> None:
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    labels = ro.random_map((2, 41, 53), [0.3, 0.25, 0.2, 0.15], seed=connectivity)
    ref = ro.label_regions_ref(labels, connectivity=connectivity, max_regions=4096)
    for b in range(labels.shape[0]):
        h, w = labels.shape[1:]
        found = []  # (anchor, class, mask, box) of every component scipy finds, class by class
        for c in range(4):
            comp, n = ndimage.label(labels[b] == c, structure=structure)
            for k, box in enumerate(ndimage.find_objects(comp)):
                mask = comp == k + 1
                found.append((int(np.flatnonzero(mask.reshape(-1))[0]), c, mask, box))
        found.sort(key=lambda f: f[0])
        assert ref["num"][b] == len(found) and 100 < len(found) <= 4096
        ids = np.full((h, w), -1, np.int32)
        for r, (anchor, c, mask, box) in enumerate(found):
            ids[mask] = r
            assert ref["anchor"][b, r] == anchor and ref["label"][b, r] == c and ref["area"][b, r] == mask.sum()
            assert tuple(ref["box"][b, r]) == (box[0].start, box[1].start, box[0].stop, box[1].stop)
        assert np.array_equal(ref["ids"][b], ids)
        assert (ref["label"][b, len(found):] == -1).all() and (ref["area"][b, len(found):] == 0).all()
    # for one class alone the numbering is scipy's minus one
    one = np.where(labels[:1] == 0, 0, 255).astype(np.uint8)
    comp, _ = ndimage.label(one[0] == 0, structure=structure)
    assert np.array_equal(ro.label_regions_ref(one, connectivity=connectivity)["ids"][0], comp.astype(np.int32) - 1)


# -------------------------------------------------------------------------------------------------- hand-written cases
def test_checkerboard() -> None:
    board = ro.checkerboard(5, 7)
    four = ro.label_regions_ref(board, connectivity=4, max_regions=8)
    assert four["num"][0] == 35  # every pixel its own region, the tables truncated at 8 rows, the ids not
    assert np.array_equal(four["ids"][0].reshape(-1), np.arange(35))
    assert four["anchor"][0].tolist() == list(range(8)) and four["label"][0].tolist() == [0, 1] * 4
    assert (four["area"][0] == 1).all() and four["box"][0, 3].tolist() == [0, 3, 1, 4]
    eight = ro.label_regions_ref(board, connectivity=8)
    assert eight["num"][0] == 2 and np.array_equal(eight["ids"][0], board[0].astype(np.int32))
    assert eight["area"][0, :3].tolist() == [18, 17, 0] and eight["box"][0, :2].tolist() == [[0, 0, 5, 7]] * 2
    assert eight["sum"][0, 0].tolist() == [sum(y for y in range(5) for x in range(7) if (y + x) % 2 == 0),
                                           sum(x for y in range(5) for x in range(7) if (y + x) % 2 == 0)]


def test_diagonal_pair() -> None:
    m = np.full((1, 3, 4), 255, np.uint8)
    m[0, 0, 1] = m[0, 1, 2] = 9
    eight = ro.label_regions_ref(m, connectivity=8)
    assert eight["num"][0] == 1 and eight["area"][0, 0] == 2 and eight["box"][0, 0].tolist() == [0, 1, 2, 3]
    assert eight["anchor"][0, 0] == 1 and eight["label"][0, 0] == 9 and eight["sum"][0, 0].tolist() == [1, 3]
    four = ro.label_regions_ref(m, connectivity=4)
    assert four["num"][0] == 2 and four["anchor"][0, :2].tolist() == [1, 6]
    assert four["ids"][0].tolist() == [[-1, 0, -1, -1], [-1, -1, 1, -1], [-1, -1, -1, -1]]
    dropped = ro.label_regions_ref(m, connectivity=4, min_area=2)
    assert dropped["num"][0] == 0 and (dropped["ids"] == -1).all() and (dropped["labels_out"] == 255).all()


def test_ring_around_a_hole_of_another_class() -> None:
    m = np.full((1, 5, 5), 1, np.uint8)
    m[0, 1:4, 1:4] = 2
    m[0, 2, 2] = 255
    best = np.zeros((1, 5, 5), np.float32)
    best[0, 4, 4] = best[0, 0, 3] = 2.0  # a tie inside the ring: the lower index wins
    best[0, 1, 1] = np.nan
    best[0, 3, 3] = -0.0  # against the +0.0 of (1, 2), which comes first
    for connectivity in (4, 8):
        ref = ro.label_regions_ref(m, best, connectivity=connectivity)
        assert ref["num"][0] == 2 and ref["label"][0, :2].tolist() == [1, 2] and ref["area"][0, :2].tolist() == [16, 8]
        assert ref["anchor"][0, :2].tolist() == [0, 6] and ref["box"][0, :2].tolist() == [[0, 0, 5, 5], [1, 1, 4, 4]]
        assert ref["ids"][0, 2, 2] == -1 and ref["labels_out"][0, 2, 2] == 255
        assert ref["peak"][0, :3].tolist() == [3, 7, -1] and ref["peak_score"][0, 0] == 2.0
        assert ref["peak_score"][0, 2] == -np.inf and not np.signbit(ref["peak_score"][0, 1])
        kept = ro.label_regions_ref(m, best, connectivity=connectivity, min_area=9)
        assert kept["num"][0] == 1 and kept["label"][0, 0] == 1 and (kept["labels_out"][0, 1:4, 1:4] == 255).all()
        assert (kept["ids"][0][m[0] == 1] == 0).all()


def test_peak_order() -> None:
    nan = np.nan
    assert ro.peak_of(np.array([nan, nan], np.float32)) == 0
    assert ro.peak_of(np.array([nan, -np.inf, nan], np.float32)) == 1
    assert ro.peak_of(np.array([-0.0, 0.0, nan], np.float32)) == 0 and ro.peak_of(np.array([0.0, -0.0], np.float32)) == 0
    assert ro.peak_of(np.array([1.0, 3.0, 3.0, np.inf, np.inf], np.float32)) == 3
    assert ro.same(np.array([nan, 0.0], np.float32), np.array([nan, 0.0], np.float32))
    assert not ro.same(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not ro.same(np.array([1], np.int32), np.array([1], np.int64))


def test_shapes_of_the_test_maps() -> None:
    s = ro.label_regions_ref(ro.serpentine(9, 6), connectivity=4)
    assert s["num"][0] == 1 and s["area"][0, 0] == 5 * 6 + 4
    p = ro.spiral(9, 11)
    assert ro.label_regions_ref(p, connectivity=4)["num"][0] == 1 and (p != 255).sum() > 40
    assert ro.label_regions_ref(p, connectivity=8)["area"][0, 0] == (p != 255).sum()


# ------------------------------------------------------------------------------------------- Regions' own arithmetic
def make_regions(**kw: torch.Tensor) -> Regions:
    base = dict(ids=torch.full((1, 6, 8), -1, dtype=torch.int32), num=torch.tensor([2], dtype=torch.int32),
                label=torch.tensor([[1, 2, -1]], dtype=torch.int32), area=torch.tensor([[4, 3, 0]], dtype=torch.int32),
                anchor=torch.tensor([[0, 9, -1]], dtype=torch.int32), boxes=torch.zeros((1, 3, 4), dtype=torch.int32),
                sums=torch.tensor([[[6, 10], [7, 2], [0, 0]]], dtype=torch.int64))
    base.update(kw)
    return Regions(**base)


def test_centroids() -> None:
    c = make_regions().centroids()
    assert c.dtype == torch.float64 and c.shape == (1, 3, 2)
    assert c[0, 0].tolist() == [1.5, 2.5] and c[0, 1].tolist() == [7 / 3, 2 / 3] and torch.isnan(c[0, 2]).all()


def test_peak_cells() -> None:
    # a 6 x 8 image: pixel (5, 7) = 47, pixel (2, 3) = 19, an empty row
    r = make_regions(peak=torch.tensor([[47, 19, -1]], dtype=torch.int32),
                     peak_scores=torch.tensor([[1.0, 0.5, -math.inf]]))
    cells = r.peak_cells((3, 4))
    assert cells.dtype == torch.int64 and cells.tolist() == [[2 * 4 + 3, 1 * 4 + 1, -1]]
    assert r.peak_cells((6, 8)).tolist() == [[47, 19, -1]]  # the identity grid
    assert r.peak_cells((1, 1)).tolist() == [[0, 0, -1]]
    # a grid finer than the image: the cell that holds the pixel's centre, ((2y + 1) h // (2H)) w + (2x + 1) w // (2W)
    assert r.peak_cells((12, 16)).tolist() == [[11 * 16 + 15, 5 * 16 + 7, -1]]
    with pytest.raises(ValueError, match="peaks"):
        make_regions().peak_cells((3, 4))
    with pytest.raises(TypeError):
        r.peak_cells(3)
    assert len(r) == 1 and r.device.type == "cpu" and r.cpu().labels is None and r.to("cpu").peak.tolist() == [[47, 19, -1]]


# ----------------------------------------------------------------------------------------------------- argument checks
def test_label_regions_argument_checks() -> None:
    labels = torch.zeros((2, 5, 6), dtype=torch.uint8)
    with pytest.raises(TypeError, match="Tensor or LabelMaps"):
        label_regions(labels.numpy())
    with pytest.raises(TypeError, match="uint8"):
        label_regions(labels.to(torch.int32))
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        label_regions(labels[0])
    with pytest.raises(TypeError, match="float32"):
        label_regions(labels, scores=torch.zeros((2, 5, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="shape of labels"):
        label_regions(labels, scores=torch.zeros((2, 5, 7)))
    with pytest.raises(ValueError, match="connectivity"):
        label_regions(labels, connectivity=6)
    with pytest.raises(TypeError, match="connectivity"):
        label_regions(labels, connectivity=8.0)
    for name in ("min_area", "max_regions"):
        with pytest.raises(ValueError, match=name):
            label_regions(labels, **{name: 0})
        with pytest.raises(TypeError, match=name):
            label_regions(labels, **{name: 2.5})
        with pytest.raises(TypeError, match=name):
            label_regions(labels, **{name: True})
    big = torch.zeros((1, 100, 100), dtype=torch.uint8)
    with pytest.raises(ValueError, match="max_regions may be at most"):
        label_regions(big, scores=torch.zeros((1, 100, 100)), max_regions=2000)
    # everything else in order: the device is asked for last
    with pytest.raises(segmentation._lib.HipLibraryError, match="no CPU fallback"):
        label_regions(labels)
    with pytest.raises(segmentation._lib.HipLibraryError, match="no CPU fallback"):
        LabelMaps(labels, scores=torch.zeros((2, 5, 6))).regions(min_area=3)
    with pytest.raises(ValueError, match="min_area"):
        LabelMaps(labels).regions(min_area=0)
