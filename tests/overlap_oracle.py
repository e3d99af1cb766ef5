"""The definitions of isc_overlap_table and isc_overlap_best (include/imagescry_hip.h) and of SegmentationScores in plain
numpy and Python integers, independent of the code under test: the table by np.bincount over the clamped indices, the
best partner by fractions.Fraction, and mmseg's IoUMetric counts by its own mask-then-histogram formulation."""

from __future__ import annotations

from fractions import Fraction

import numpy as np


def clamp(values: np.ndarray, num: int) -> np.ndarray:
    """The index of every pixel on an axis of `num` regions: the value in [0, num), else the "none" slot `num`."""
    v = np.asarray(values).astype(np.int64)
    return np.where((v >= 0) & (v < num), v, num)


def table_ref(a: np.ndarray, b: np.ndarray, num_a: int, num_b: int, per_image: bool = True) -> np.ndarray:
    """int64 [B, num_a + 1, num_b + 1] (or the sum over B) for [B, H, W] rasters of any integer dtype."""
    assert a.shape == b.shape and a.ndim == 3
    size = (num_a + 1) * (num_b + 1)
    out = np.zeros((a.shape[0], num_a + 1, num_b + 1), dtype=np.int64)
    for k in range(a.shape[0]):
        fused = clamp(a[k], num_a).ravel() * (num_b + 1) + clamp(b[k], num_b).ravel()
        out[k] = np.bincount(fused, minlength=size).reshape(num_a + 1, num_b + 1)
    return out if per_image else out.sum(axis=0)


def best_ref(tables: np.ndarray, axis: int, exclude_none: bool) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(best int32, inter int64, uni int64), each [B, R], of int64 [B, Ra + 1, Rb + 1] tables: exact rationals."""
    assert tables.ndim == 3 and axis in (0, 1)
    if axis == 1:
        tables = tables.transpose(0, 2, 1)
    n, rows, cols = tables.shape[0], tables.shape[1] - 1, tables.shape[2] - 1
    best = np.full((n, rows), -1, dtype=np.int32)
    inter = np.zeros((n, rows), dtype=np.int64)
    uni = np.zeros((n, rows), dtype=np.int64)
    for k in range(n):
        t = tables[k]
        area_r = [int(v) for v in (t[:, :cols] if exclude_none else t).sum(axis=1)]
        area_c = [int(v) for v in (t[:rows, :] if exclude_none else t).sum(axis=0)]
        top = [None] * rows
        for i, j in zip(*np.nonzero(t[:rows, :cols])):  # row major: ascending j within a row
            shared = int(t[i, j])
            union = area_r[i] + area_c[j] - shared
            iou = Fraction(shared, union)
            if top[i] is None or iou > top[i][0]:
                top[i] = (iou, int(j), shared, union)
        for i in range(rows):
            if top[i] is None:
                uni[k, i] = area_r[i]
            else:
                _, best[k, i], inter[k, i], uni[k, i] = top[i]
    return best, inter, uni


def mmseg_counts(pred: np.ndarray, target: np.ndarray, num_classes: int) -> dict[str, np.ndarray]:
    """intersect, pred_area, target_area, union as mmseg's IoUMetric.intersect_and_union finds them: mask the ignored
    target pixels away, then histogram what is left over the bins 0 .. C - 1 (values outside fall in no bin)."""
    pred, target = np.asarray(pred).astype(np.int64).ravel(), np.asarray(target).astype(np.int64).ravel()
    keep = (target >= 0) & (target < num_classes)  # the "none" of the target: ignore_index and anything out of range
    pred, target = pred[keep], target[keep]

    def hist(v: np.ndarray) -> np.ndarray:
        v = v[(v >= 0) & (v < num_classes)]
        return np.bincount(v, minlength=num_classes).astype(np.int64)

    intersect, pred_area, target_area = hist(pred[pred == target]), hist(pred), hist(target)
    return {"intersect": intersect, "pred_area": pred_area, "target_area": target_area,
            "union": pred_area + target_area - intersect}


def counts_from_table(table: np.ndarray) -> dict[str, np.ndarray]:
    """The same four from a confusion matrix [C + 1, C + 1] (rows the prediction, columns the target)."""
    c = table.shape[0] - 1
    intersect = np.array([table[k, k] for k in range(c)], dtype=np.int64)
    pred_area = np.array([sum(int(table[k, j]) for j in range(c)) for k in range(c)], dtype=np.int64)
    target_area = np.array([sum(int(table[i, k]) for i in range(c + 1)) for k in range(c)], dtype=np.int64)
    return {"intersect": intersect, "pred_area": pred_area, "target_area": target_area,
            "union": pred_area + target_area - intersect}


def nan_mean(values: np.ndarray) -> float:
    """The mean of the non-NaN entries as SegmentationScores defines it: NaN reads as 0, zeros pad the vector to a power
    of two, neighbours are added until one value is left, which is divided by the count of non-NaN entries."""
    v = [0.0 if np.isnan(x) else float(x) for x in values]
    count = sum(1 for x in values if not np.isnan(x))
    while len(v) & (len(v) - 1) or not v:
        v.append(0.0)
    while len(v) > 1:
        v = [v[k] + v[k + 1] for k in range(0, len(v), 2)]
    return v[0] / count if count else float("nan")


def scores_ref(counts: dict[str, np.ndarray]) -> dict[str, object]:
    """iou, accuracy, dice float64 [C] (NaN where the denominator is 0) and the scalars miou, macc, aacc."""
    f = {k: v.astype(np.float64) for k, v in counts.items()}
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = f["intersect"] / f["union"]
        acc = f["intersect"] / f["target_area"]
        dice = (2 * counts["intersect"]).astype(np.float64) / (counts["pred_area"] + counts["target_area"]).astype(np.float64)
        aacc = np.float64(counts["intersect"].sum()) / np.float64(counts["target_area"].sum())
    return {"iou": iou, "accuracy": acc, "dice": dice, "miou": nan_mean(iou), "macc": nan_mean(acc), "aacc": float(aacc)}
