"""tests/overlap_oracle.py proves itself, without a GPU: its formulations agree with each other and with brute force on
random maps with unlabeled and ignored pixels; and the parts of imagescry_amd.segmentation's overlap layer that need no
device -- SegmentationScores on CPU tables, the NaN handling of its means, and the argument errors."""

from __future__ import annotations

import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import overlap_oracle as ov  # noqa: E402

from imagescry_amd import (LabelMaps, RegionMatches, SegmentationScores, _lib, confusion_matrix, match_regions,  # noqa: E402
                           overlap_table, segmentation)


def random_pair(seed: int, shape: tuple[int, int, int], classes: int) -> tuple[np.ndarray, np.ndarray]:
    """A prediction with unlabeled (255) pixels and a target with ignored (255 and -100) ones."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, classes, shape).astype(np.int64)
    target = np.where(rng.random(shape) < 0.6, pred, rng.integers(0, classes, shape)).astype(np.int64)
    pred[rng.random(shape) < 0.1] = 255
    target[rng.random(shape) < 0.1] = 255
    target[rng.random(shape) < 0.05] = -100
    return pred, target


@pytest.mark.parametrize("seed", range(6))
def test_table_counts_every_pixel_once_and_agrees_with_brute_force(seed: int) -> None:
    rng = np.random.default_rng(seed)
    b, h, w = 3, int(rng.integers(1, 12)), int(rng.integers(1, 12))
    ra, rb = int(rng.integers(1, 6)), int(rng.integers(1, 6))
    a = rng.integers(-2, ra + 3, (b, h, w)).astype(np.int32)
    bb = rng.integers(-2, rb + 3, (b, h, w)).astype(np.int32)
    table = ov.table_ref(a, bb, ra, rb)
    assert table.shape == (b, ra + 1, rb + 1) and table.dtype == np.int64
    assert (table.sum(axis=(1, 2)) == h * w).all()
    assert np.array_equal(ov.table_ref(a, bb, ra, rb, per_image=False), table.sum(axis=0))
    for k in range(b):
        for i in range(ra + 1):
            in_a = (a[k] == i) if i < ra else ((a[k] < 0) | (a[k] >= ra))
            for j in range(rb + 1):
                in_b = (bb[k] == j) if j < rb else ((bb[k] < 0) | (bb[k] >= rb))
                assert table[k, i, j] == np.count_nonzero(in_a & in_b)
    # uint8: 255 is "none" with R <= 255
    u = rng.integers(0, 256, (1, h, w)).astype(np.uint8)
    assert ov.table_ref(u, u, 255, 255)[0, 255, 255] == np.count_nonzero(u == 255)


@pytest.mark.parametrize("exclude_none", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_best_match_agrees_with_masks(seed: int, exclude_none: bool) -> None:
    rng = np.random.default_rng(100 + seed)
    ra, rb = 5, 4
    a = rng.integers(-1, ra + 1, (2, 9, 11)).astype(np.int32)
    b = rng.integers(-1, rb + 1, (2, 9, 11)).astype(np.int32)
    a[a == 2] = 0  # a region without pixels
    table = ov.table_ref(a, b, ra, rb)
    for axis in (0, 1):
        best, inter, uni = ov.best_ref(table, axis, exclude_none)
        x, y, rx, ry = (a, b, ra, rb) if axis == 0 else (b, a, rb, ra)
        assert best.shape == (2, rx) and best.dtype == np.int32
        for k in range(2):
            some_x, some_y = (x[k] >= 0) & (x[k] < rx), (y[k] >= 0) & (y[k] < ry)
            for i in range(rx):
                mine = (x[k] == i) & (some_y if exclude_none else True)
                top = None
                for j in range(ry):
                    theirs = (y[k] == j) & (some_x if exclude_none else True)
                    shared, either = np.count_nonzero(mine & theirs), np.count_nonzero(mine | theirs)
                    if shared and (top is None or Fraction(shared, either) > top[0]):
                        top = (Fraction(shared, either), j, shared, either)
                want = (-1, 0, np.count_nonzero(mine)) if top is None else top[1:]
                assert (best[k, i], inter[k, i], uni[k, i]) == want
    assert (ov.best_ref(table, 0, False)[0][:, 2] == -1).all()


@pytest.mark.parametrize("seed", range(5))
def test_confusion_counts_agree_with_mask_then_histogram(seed: int) -> None:
    classes = 6
    pred, target = random_pair(seed, (3, 13, 17), classes)
    pred[pred == 4] = 255  # a class nobody predicts ...
    target[target == 4] = 255  # ... and nobody drew
    table = ov.table_ref(pred, target, classes, classes, per_image=False)
    direct, derived = ov.mmseg_counts(pred, target, classes), ov.counts_from_table(table)
    for name in ("intersect", "pred_area", "target_area", "union"):
        assert np.array_equal(direct[name], derived[name]), name
    scores = SegmentationScores.from_confusion(torch.from_numpy(table))
    for name in ("intersect", "pred_area", "target_area", "union"):
        got = getattr(scores, name)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), direct[name]), name
    ref = ov.scores_ref(direct)
    for name, got in (("iou", scores.iou()), ("accuracy", scores.accuracy()), ("dice", scores.dice())):
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), ref[name], equal_nan=True), name
    assert math.isnan(ref["iou"][4]) and math.isnan(ref["accuracy"][4]) and math.isnan(ref["dice"][4])
    for name, got in (("miou", scores.miou()), ("macc", scores.macc()), ("aacc", scores.aacc())):
        assert got.dtype == torch.float64 and got.ndim == 0 and float(got) == ref[name], name
    assert len(scores) == classes and scores.cpu().device.type == "cpu" and scores.to("cpu").union.equal(scores.union)


def test_absent_classes_are_left_out_of_the_means() -> None:
    # class 1 is in neither map: its IoU is NaN and the mean runs over the other two
    table = torch.tensor([[6, 0, 2, 1], [0, 0, 0, 0], [1, 0, 3, 0], [1, 0, 0, 5]], dtype=torch.int64)
    s = SegmentationScores.from_confusion(table)
    assert s.intersect.tolist() == [6, 0, 3] and s.pred_area.tolist() == [8, 0, 4] and s.target_area.tolist() == [8, 0, 5]
    assert s.union.tolist() == [10, 0, 6]
    iou = s.iou()
    assert math.isnan(float(iou[1])) and iou[0] == 0.6 and iou[2] == 0.5
    assert float(s.miou()) == (0.6 + 0.5) / 2
    assert float(s.macc()) == (6 / 8 + 3 / 5) / 2
    assert float(s.aacc()) == 9 / 13
    nothing = SegmentationScores.from_confusion(torch.zeros((3, 3), dtype=torch.int64))
    assert math.isnan(float(nothing.miou())) and math.isnan(float(nothing.macc())) and math.isnan(float(nothing.aacc()))
    assert ov.nan_mean(np.array([np.nan, 0.25, np.nan])) == 0.25 and math.isnan(ov.nan_mean(np.array([np.nan])))


def test_from_confusion_refuses_other_tables() -> None:
    with pytest.raises(TypeError):
        SegmentationScores.from_confusion(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(TypeError):
        SegmentationScores.from_confusion(torch.zeros((3, 3), dtype=torch.int32))
    for shape in ((3, 4), (2, 3, 3), (1, 1), (9,)):
        with pytest.raises(ValueError):
            SegmentationScores.from_confusion(torch.zeros(shape, dtype=torch.int64))


def test_region_matches_iou() -> None:
    m = RegionMatches(torch.tensor([[1, -1, -1]], dtype=torch.int32), torch.tensor([[3, 0, 0]]), torch.tensor([[4, 7, 0]]))
    iou = m.iou()
    assert iou.dtype == torch.float64 and iou[0, 0] == 0.75 and iou[0, 1] == 0.0 and math.isnan(float(iou[0, 2]))
    assert len(m) == 1 and m.cpu().best_b is None
    with pytest.raises(ValueError):
        m.iou_b()


def test_argument_errors_that_need_no_device() -> None:
    u8 = torch.zeros((2, 4, 5), dtype=torch.uint8)
    i32 = torch.zeros((2, 4, 5), dtype=torch.int32)
    with pytest.raises(TypeError):
        overlap_table(u8.numpy(), u8, 3, 3)
    for bad in (torch.int64, torch.int16, torch.float32, torch.bool):
        with pytest.raises(TypeError):
            overlap_table(u8.to(bad), u8, 3, 3)
        with pytest.raises(TypeError):
            overlap_table(u8, i32.to(bad), 3, 3)
    with pytest.raises(ValueError):
        overlap_table(u8[0], u8[0], 3, 3)
    with pytest.raises(ValueError):
        overlap_table(u8, i32[:, :, :4], 3, 3)
    with pytest.raises(ValueError):
        overlap_table(u8[:, :0], i32[:, :0], 3, 3)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            overlap_table(u8, i32, bad, 3)
        with pytest.raises(ValueError):
            match_regions(u8, i32, 3, bad)
    for bad in (2.0, True, None):
        with pytest.raises(TypeError):
            overlap_table(u8, i32, 3, bad)
        with pytest.raises(TypeError):
            confusion_matrix(u8, i32, bad)
    # (Ra + 1) * (Rb + 1) <= 2^25: the passing side goes on to the device check
    with pytest.raises(ValueError):
        overlap_table(u8, i32, 2**13, 2**12 - 1)
    with pytest.raises(_lib.HipLibraryError):
        overlap_table(u8, i32, 2**13 - 1, 2**12 - 1)
    assert segmentation.MAX_OVERLAP_TABLE == 2**25 and segmentation.MAX_OVERLAP_PIXELS == 2**31 - 1
    assert segmentation.OVERLAP_PASS_BYTES == segmentation.POOL_PASS_BYTES == 256 << 20
    # CPU tensors: the error class of the neighbours
    for call in (lambda: overlap_table(u8, i32, 3, 3), lambda: confusion_matrix(LabelMaps(u8), i32.to(torch.int64), 3),
                 lambda: match_regions(i32, u8, 3, 3), lambda: LabelMaps(u8).confusion(i32, 3)):
        with pytest.raises(_lib.HipLibraryError):
            call()
