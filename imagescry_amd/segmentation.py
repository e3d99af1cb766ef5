"""Pixel label maps from dense patch scores (new; the counterpart of the reference's `geometry.py`, which turns a
polygon into a mask on the feature-map grid: this turns feature-map scores into a mask on the image grid).

`class_scores` scores every cell of an embedding map against C vectors (`isc_map_class_scores`), `label_map` upsamples
the scores bilinearly to the image and takes the arg max per pixel in one kernel (`isc_label_map`) without ever writing
the `[B, C, H, W]` tensor of `F.interpolate(scores, size).max(1)`, and `segment` runs the two back to back.  The
arithmetic is fixed (include/imagescry_hip.h): the answers are deterministic, bit for bit reproducible and capturable
into a graph.  The producers are a dense CLIP map with text embeddings (`CLIPEmbedder.segment`), a DINOv2 map with
`KMeans` centroids, and `EmbeddingBank.similarity_map` (`EmbeddingBank.label_map`).

Sliding-window inference (what MaskCLIP, SCLIP, ClearCLIP and NACLIP evaluate with): `window_grid` places windows of the
checkpoint's own resolution over a larger image, `crop_windows` cuts them out, and `label_map_windows` upsamples every
window's scores to its pixels, averages the windows that overlap on a pixel and takes the arg max, again in one kernel
(`isc_label_map_windows`); `segment_windows` is `class_scores` + `label_map_windows`, `CLIPEmbedder.segment(window=)` the
whole path.

Pixels back to regions: `label_regions` (or `LabelMaps.regions`) finds the connected regions of a label map on the device
(`isc_label_regions`: a union-find across tiles) -- ids per pixel, and per region its class, area, box, coordinate sums
and best-scoring pixel -- and drops regions below `min_area`: what `scipy.ndimage.label` per class and image does on the
host, without the round trip.

Regions back to vectors: `pool_regions` (or `Regions.embed`) pools a patch map over every region's pixels -- the mean of
the bilinearly upsampled map over the mask, as a weighted sum over cells whose weights are exact integers
(`isc_region_cell_weights`, `isc_region_pool`) -- so that an object is described by all of its patches and is a row of a
bank like any other.

Drawn regions: `rasterize_polygons` burns ROI polygons -- what an annotator drew -- onto a pixel grid as region ids on the
device (`isc_rasterize_polygons`: an exact integer definition of rasterio's `rasterize`, with or without `all_touched`),
`pack_polygons` snaps and flattens them on the host, `create_roi_mask` is the reference's `geometry.create_roi_mask`, and
`pool_polygons` turns every drawn shape into a query vector.

Outlines: `trace_regions` (or `Regions.outlines`) turns region ids back into polygon rings on the device
(`isc_trace_regions`: rasterio's `shapes`, defined exactly) -- corners only, holes as rings of negative area, laid out as
a `PackedPolygons` that `rasterize_polygons` takes as it is -- and `RegionOutlines.shapes()` brings them to the host.

Two rasters compared: `overlap_table` counts the pixels of every pair of values in two aligned rasters on the device
(`isc_overlap_table`: integer atomics, the same bytes on every run) -- `confusion_matrix` (or `LabelMaps.confusion`) is
the batch-summed class table and `SegmentationScores` the mIoU, mAcc and aAcc of mmseg's `IoUMetric` from it;
`match_regions` (or `Regions.match`) finds for every region of one id raster the region of the other it fits best by
IoU, compared exactly (`isc_overlap_best`).
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from imagescry_amd import _lib
from imagescry_amd.data import EmbeddingBatch

__all__ = ["LabelMaps", "UNLABELED", "MAX_PROMPTS", "MAX_CLASSES", "class_scores", "label_map", "label_map_geometry",
           "segment", "window_grid", "crop_windows", "label_map_windows", "segment_windows", "Regions", "label_regions",
           "label_regions_geometry", "RegionVectors", "region_cell_weights", "pool_regions",
           "region_pool_geometry", "PackedPolygons", "pack_polygons", "rasterize_polygons", "rasterize_geometry",
           "create_roi_mask", "pool_polygons", "RegionOutlines", "trace_regions", "trace_geometry", "overlap_table",
           "overlap_geometry", "overlap_best_geometry", "confusion_matrix", "SegmentationScores", "RegionMatches",
           "match_regions"]

UNLABELED = 255  # the label of a pixel whose best score is NaN or below `min_score`
MAX_PROMPTS = 1024  # isc_label_map: 1 <= C <= 1024
MAX_CLASSES = 255  # class ids 0 .. 254


@dataclass(frozen=True)
class LabelMaps:
    """What `label_map` returns; a field that was not asked for is None.

    labels:  uint8 `[B, H, W]`, the class of the best prompt per pixel, `UNLABELED` (255) where it is unlabeled
    scores:  float32 `[B, H, W]`, the best prompt's upsampled score
    margins: float32 `[B, H, W]`, that score minus the best score of any OTHER class (+inf with a single class): the
             confidence to threshold on
    counts:  int32 `[B, 256]`, pixels per label, the unlabeled ones at index 255
    indices: int64 `[B]` dataset indices, where the producer had them (`CLIPEmbedder.segment`)"""

    labels: Tensor
    scores: Tensor | None = None
    margins: Tensor | None = None
    counts: Tensor | None = None
    indices: Tensor | None = None

    def to(self, device: str | torch.device) -> "LabelMaps":
        return LabelMaps(*(None if t is None else t.to(device)
                           for t in (self.labels, self.scores, self.margins, self.counts, self.indices)))

    def cpu(self) -> "LabelMaps":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.labels.device

    def __len__(self) -> int:
        return self.labels.shape[0]

    def regions(self, **kw: object) -> "Regions":
        """`label_regions(self, **kw)`: the connected regions of these maps, `scores` scoring the peaks."""
        return label_regions(self, **kw)

    def confusion(self, target: Tensor, num_classes: int, out: Tensor | None = None) -> Tensor:
        """`confusion_matrix(self, target, num_classes, out=out)`: these maps as the prediction against `target`."""
        return confusion_matrix(self, target, num_classes, out=out)


def label_map_geometry() -> tuple[int, int, int]:
    """(tile_w, tile_h, prompt_chunk) of the `isc_label_map` kernel."""
    tw, th, pc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().isc_label_map_geometry(tw, th, pc), "isc_label_map_geometry")
    return tw.value, th.value, pc.value


def _check_size(size: object) -> tuple[int, int]:
    if (not isinstance(size, (tuple, list)) or len(size) != 2
            or not all(isinstance(v, int) and not isinstance(v, bool) for v in size)):
        raise TypeError(f"size must be a pair of ints (H, W), got {size!r}")
    h, w = size
    if h < 1 or w < 1:
        raise ValueError(f"size must be at least 1 x 1, got {h} x {w}")
    if h * w >= 2**31:
        raise ValueError(f"size {h} x {w} has 2^31 pixels or more")
    return h, w


def _check_float_tensor(name: str, t: object, ndim: int, what: str) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.ndim != ndim:
        raise ValueError(f"{name} must have shape {what}, got {tuple(t.shape)}")
    return t


def _check_class_of(class_of: object, prompts: int) -> Tensor | None:
    """-> a checked integer tensor `[C]`.  A tensor on the device costs one host read for its range."""
    if class_of is None:
        if prompts > MAX_CLASSES:
            raise ValueError(f"{prompts} prompts without class_of would be {prompts} classes; labels hold at most "
                             f"{MAX_CLASSES} (ids 0 .. {MAX_CLASSES - 1})")
        return None
    if not isinstance(class_of, Tensor):
        if not isinstance(class_of, (list, tuple)) or not all(isinstance(v, int) and not isinstance(v, bool)
                                                              for v in class_of):
            raise TypeError("class_of must be an integer tensor or a sequence of ints")
        class_of = torch.tensor(list(class_of), dtype=torch.int64)
    if class_of.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16):
        raise TypeError(f"class_of must be an integer tensor, got {class_of.dtype}")
    if class_of.shape != (prompts,):
        raise ValueError(f"class_of must have one entry per prompt, [{prompts}], got {tuple(class_of.shape)}")
    lo, hi = int(class_of.min()), int(class_of.max())
    if lo < 0 or hi >= MAX_CLASSES:
        raise ValueError(f"class_of values must be in [0, {MAX_CLASSES - 1}], got [{lo}, {hi}]")
    return class_of


def class_scores(maps: "EmbeddingBatch | Tensor", vectors: Tensor) -> Tensor:
    """Cosine-style scores of every cell of `maps` (an `EmbeddingBatch` or float32 `[B, E, h, w]`) against `vectors`
    (float32 `[C, E]`): float32 `[B, h, w, C]`, the layout `label_map` reads.  `out[b, i, j, c] = float32(m . t / max(|t|,
    1e-12))`, the dot product and the norm as float64 chains over the embedding axis ascending (`isc_map_class_scores`):
    the vector is normalised, the cell is taken as stored (`predict_step` maps are unit norm already), as `search` takes
    the bank's rows.  Not the bits of `bank.scores`, whose chain runs in another order."""
    if isinstance(maps, EmbeddingBatch):
        maps = maps.embeddings
    maps = _check_float_tensor("maps", maps, 4, "[B, E, h, w]")
    vectors = _check_float_tensor("vectors", vectors, 2, "[C, E]")
    b, e, h, w = maps.shape
    c = vectors.shape[0]
    if vectors.shape[1] != e:
        raise ValueError(f"vectors have {vectors.shape[1]} dimensions but the map has {e}")
    if c < 1 or e < 1 or h < 1 or w < 1:
        raise ValueError(f"maps {tuple(maps.shape)} and vectors {tuple(vectors.shape)} must not be empty")
    if h * w >= 2**31:
        raise ValueError(f"a {h} x {w} map has 2^31 cells or more")
    _lib.require_device(maps, "maps")
    if vectors.device != maps.device:
        raise ValueError(f"maps are on {maps.device} but vectors on {vectors.device}")
    maps, vectors = maps.contiguous(), vectors.contiguous()
    out = torch.empty((b, h, w, c), dtype=torch.float32, device=maps.device)
    with torch.cuda.device(maps.device):
        st = _lib.load().isc_map_class_scores(maps.data_ptr(), b, e, h * w, vectors.data_ptr(), c, e, out.data_ptr(), c,
                                              _lib.stream_handle(maps.device))
    _lib.check(st, "isc_map_class_scores")
    return out


def label_map(scores: Tensor, size: "tuple[int, int]", *, layout: str = "bhwc", class_of: "Tensor | list[int] | None" = None,
              min_score: float | None = None, return_scores: bool = True, return_margin: bool = False,
              return_counts: bool = False) -> LabelMaps:
    """Upsample class scores bilinearly (`align_corners=False`) to `size = (H, W)` and label every pixel with the class
    of its best prompt, in one kernel.

    `scores`: float32 `[B, h, w, C]` (`layout="bhwc"`, what `class_scores` returns) or `[B, C, h, w]` (`"bchw"`, what
    `F.interpolate` would take; permuted on the device -- it is the small tensor).  `class_of` (int `[C]`, values in
    `[0, 254]`) maps prompts to classes, so that "a car" and "a photo of a car" can stand for one class; without it the
    class is the prompt, and `C <= 255`.  `min_score`: pixels whose best score is below it (or NaN) get `UNLABELED`
    (255); None switches the threshold off.  `LabelMaps.scores` / `.margins` / `.counts` are filled as `return_scores` /
    `return_margin` / `return_counts` say.  `1 <= C <= 1024`.  Nothing synchronises with the host (a `class_of` tensor on
    the device costs one read for its range; pass a list, or check it once and keep it on the CPU)."""
    if layout not in ("bhwc", "bchw"):
        raise ValueError(f'layout must be "bhwc" or "bchw", got {layout!r}')
    scores = _check_float_tensor("scores", scores, 4, "[B, h, w, C]" if layout == "bhwc" else "[B, C, h, w]")
    big_h, big_w = _check_size(size)
    if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float))):
        raise TypeError(f"min_score must be a number or None, got {type(min_score).__name__}")
    if min_score is not None and math.isnan(min_score):
        raise ValueError("min_score must not be NaN")
    if layout == "bchw":
        scores = scores.permute(0, 2, 3, 1)
    b, h, w, c = scores.shape
    if not 1 <= c <= MAX_PROMPTS:
        raise ValueError(f"scores hold {c} prompts; label_map takes 1 .. {MAX_PROMPTS}")
    if h < 1 or w < 1:
        raise ValueError(f"scores must hold at least one cell, got a {h} x {w} grid")
    if h * w >= 2**31:
        raise ValueError(f"a {h} x {w} grid has 2^31 cells or more")
    classes = _check_class_of(class_of, c)
    _lib.require_device(scores, "scores")
    device = scores.device
    if classes is not None:
        classes = classes.to(device=device, dtype=torch.int32).contiguous()
    scores = scores.contiguous()
    labels = torch.empty((b, big_h, big_w), dtype=torch.uint8, device=device)
    best = torch.empty((b, big_h, big_w), dtype=torch.float32, device=device) if return_scores else None
    margins = torch.empty((b, big_h, big_w), dtype=torch.float32, device=device) if return_margin else None
    counts = torch.empty((b, 256), dtype=torch.int32, device=device) if return_counts else None
    with torch.cuda.device(device):
        st = _lib.load().isc_label_map(scores.data_ptr(), b, h, w, c, c, _lib.ptr(classes), big_h, big_w,
                                       -math.inf if min_score is None else float(min_score), labels.data_ptr(),
                                       _lib.ptr(best), _lib.ptr(margins), _lib.ptr(counts), _lib.stream_handle(device))
    _lib.check(st, "isc_label_map")
    return LabelMaps(labels=labels, scores=best, margins=margins, counts=counts)


def segment(maps: "EmbeddingBatch | Tensor", vectors: Tensor, size: "tuple[int, int]", **kw: object) -> LabelMaps:
    """`label_map(class_scores(maps, vectors), size, **kw)`: two launches (three with `return_counts`, whose table is
    zeroed first), capturable as one chain.  An `EmbeddingBatch`'s indices are carried into `LabelMaps.indices`."""
    if "layout" in kw:
        raise TypeError("segment takes no layout: class_scores already writes the one label_map reads")
    _check_size(size)
    out = label_map(class_scores(maps, vectors), size, **kw)
    if isinstance(maps, EmbeddingBatch):
        return LabelMaps(out.labels, out.scores, out.margins, out.counts, maps.indices)
    return out


# ------------------------------------------------------------------------------------------------------ sliding windows
def _check_pair(name: str, value: object) -> tuple[int, int]:
    """An int or a pair of ints, all at least 1 -> (vertical, horizontal)."""
    if isinstance(value, int) and not isinstance(value, bool):
        value = (value, value)
    if (not isinstance(value, (tuple, list)) or len(value) != 2
            or not all(isinstance(v, int) and not isinstance(v, bool) for v in value)):
        raise TypeError(f"{name} must be an int or a pair of ints, got {value!r}")
    if value[0] < 1 or value[1] < 1:
        raise ValueError(f"{name} must be at least 1, got {tuple(value)}")
    return value[0], value[1]


def _window_geometry(size: object, window: object, stride: object) -> tuple[tuple[int, int], tuple[int, int], tuple[int, int]]:
    """The checked (size, window, stride): a window larger than the image on an axis is clamped to the image there, and
    `stride=None` is half the (clamped) window, rounded up."""
    big_h, big_w = _check_size(size)
    win = _check_pair("window", window)
    win = (min(win[0], big_h), min(win[1], big_w))
    step = ((win[0] + 1) // 2, (win[1] + 1) // 2) if stride is None else _check_pair("stride", stride)
    if step[0] > win[0] or step[1] > win[1]:
        raise ValueError(f"stride {step} must not exceed the window {win} (clamped to the image): pixels between two "
                         "windows would be covered by none")
    return (big_h, big_w), win, step


def _axis_starts(length: int, win: int, stride: int) -> list[int]:
    return [min(i * stride, length - win) for i in range(max(length - win + stride - 1, 0) // stride + 1)]


def window_grid(size: "tuple[int, int]", window: "int | tuple[int, int]",
                stride: "int | tuple[int, int] | None" = None) -> tuple[list[int], list[int]]:
    """The first row of every window row and the first column of every window column, `(ys, xs)`, of the sliding-window
    grid over an image of `size = (H, W)` (mmseg's `slide_inference`; `isc_label_map_window_grid` counts the same):
    along an axis of length L there are `max(L - win + stride - 1, 0) // stride + 1` windows, window i starting at
    `min(i * stride, L - win)` -- the last one is shifted back to end at the border.  The starts are distinct, every
    pixel is covered, by at most `ceil(win / stride) + 1` windows an axis.  Window `(i, j)` covers rows `ys[i] : ys[i] +
    win_h` and columns `xs[j] : xs[j] + win_w`; an image's windows are ordered i major."""
    (big_h, big_w), win, step = _window_geometry(size, window, stride)
    return _axis_starts(big_h, win[0], step[0]), _axis_starts(big_w, win[1], step[1])


def crop_windows(images: Tensor, window: "int | tuple[int, int]", stride: "int | tuple[int, int] | None" = None) -> Tensor:
    """`[B, 3, H, W]` (any channel count, any dtype: uint8 stays uint8) -> the window crops `[B * ny * nx, 3, win_h,
    win_w]` of `window_grid`, image-major and i major inside an image: the order `label_map_windows` reads."""
    if not isinstance(images, Tensor):
        raise TypeError(f"images must be a torch.Tensor, got {type(images).__name__}")
    if images.ndim != 4:
        raise ValueError(f"images must have shape [B, C, H, W], got {tuple(images.shape)}")
    size, win, step = _window_geometry((int(images.shape[2]), int(images.shape[3])), window, stride)
    ys, xs = window_grid(size, win, step)
    crops = torch.stack([images[:, :, y:y + win[0], x:x + win[1]] for y in ys for x in xs], dim=1)
    return crops.reshape(images.shape[0] * len(ys) * len(xs), images.shape[1], win[0], win[1])


def label_map_windows(scores: Tensor, size: "tuple[int, int]", window: "int | tuple[int, int]",
                      stride: "int | tuple[int, int] | None" = None, *, class_of: "Tensor | list[int] | None" = None,
                      min_score: float | None = None, return_scores: bool = True, return_margin: bool = False,
                      return_counts: bool = False) -> LabelMaps:
    """Sliding-window inference in one kernel (`isc_label_map_windows`): every window's class scores are upsampled
    bilinearly to the window's pixels, the windows that cover a pixel are averaged there and the pixel is labelled with
    the class of the best prompt -- without writing a window's `[C, win_h, win_w]` upsampling or the `[B, C, H, W]` sum.

    `scores`: float32 `[B * ny * nx, h, w, C]` (what `class_scores` returns for `crop_windows`' crops) or `[B, ny, nx, h,
    w, C]`, the grid being `window_grid(size, window, stride)`'s.  Everything else as in `label_map`; the arithmetic is
    fixed (include/imagescry_hip.h): with one window equal to the image the answer is `label_map`'s bit for bit."""
    size, win, step = _window_geometry(size, window, stride)
    scores = _check_float_tensor("scores", scores, 6 if isinstance(scores, Tensor) and scores.ndim == 6 else 4,
                                 "[B * ny * nx, h, w, C] or [B, ny, nx, h, w, C]")
    if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float))):
        raise TypeError(f"min_score must be a number or None, got {type(min_score).__name__}")
    if min_score is not None and math.isnan(min_score):
        raise ValueError("min_score must not be NaN")
    ys, xs = window_grid(size, win, step)
    ny, nx = len(ys), len(xs)
    if scores.ndim == 6:
        if tuple(scores.shape[1:3]) != (ny, nx):
            raise ValueError(f"scores hold {scores.shape[1]} x {scores.shape[2]} windows an image but the grid of window "
                             f"{win}, stride {step} over {size} has {ny} x {nx}")
        b = scores.shape[0]
    else:
        if scores.shape[0] % (ny * nx):
            raise ValueError(f"scores hold {scores.shape[0]} windows, not a multiple of the {ny} x {nx} windows of window "
                             f"{win}, stride {step} over {size}")
        b = scores.shape[0] // (ny * nx)
    h, w, c = (int(v) for v in scores.shape[-3:])
    if not 1 <= c <= MAX_PROMPTS:
        raise ValueError(f"scores hold {c} prompts; label_map_windows takes 1 .. {MAX_PROMPTS}")
    if h < 1 or w < 1:
        raise ValueError(f"scores must hold at least one cell a window, got a {h} x {w} grid")
    if h * w >= 2**31:
        raise ValueError(f"a {h} x {w} grid has 2^31 cells or more")
    classes = _check_class_of(class_of, c)
    _lib.require_device(scores, "scores")
    device = scores.device
    if classes is not None:
        classes = classes.to(device=device, dtype=torch.int32).contiguous()
    scores = scores.contiguous()
    labels = torch.empty((b, *size), dtype=torch.uint8, device=device)
    best = torch.empty((b, *size), dtype=torch.float32, device=device) if return_scores else None
    margins = torch.empty((b, *size), dtype=torch.float32, device=device) if return_margin else None
    counts = torch.empty((b, 256), dtype=torch.int32, device=device) if return_counts else None
    with torch.cuda.device(device):
        st = _lib.load().isc_label_map_windows(scores.data_ptr(), b, h, w, c, c, _lib.ptr(classes), *size, *win, *step,
                                               -math.inf if min_score is None else float(min_score), labels.data_ptr(),
                                               _lib.ptr(best), _lib.ptr(margins), _lib.ptr(counts),
                                               _lib.stream_handle(device))
    _lib.check(st, "isc_label_map_windows")
    return LabelMaps(labels=labels, scores=best, margins=margins, counts=counts)


MAX_SCORED_MAPS = 65535  # isc_map_class_scores: B <= 65535 a launch


def segment_windows(maps: "EmbeddingBatch | Tensor", vectors: Tensor, size: "tuple[int, int]",
                    window: "int | tuple[int, int]", stride: "int | tuple[int, int] | None" = None,
                    **kw: object) -> LabelMaps:
    """`label_map_windows(class_scores(maps, vectors), size, window, stride, **kw)`: `maps` is the `[B * ny * nx, E, h,
    w]` map of `crop_windows`' crops or its `EmbeddingBatch` (whose indices, one per crop, are not carried: the caller
    knows the images').  `class_scores` runs in slices of 65 535 crops, its limit a launch."""
    size, win, step = _window_geometry(size, window, stride)
    m = maps.embeddings if isinstance(maps, EmbeddingBatch) else maps
    if isinstance(m, Tensor) and m.ndim == 4 and m.shape[0] > MAX_SCORED_MAPS:
        scores = torch.cat([class_scores(m[i:i + MAX_SCORED_MAPS], vectors) for i in range(0, m.shape[0], MAX_SCORED_MAPS)])
    else:
        scores = class_scores(m, vectors)
    return label_map_windows(scores, size, win, step, **kw)


# -------------------------------------------------------------------------------------------------- connected regions
@dataclass(frozen=True)
class Regions:
    """What `label_regions` returns, R = `max_regions` rows an image; a field that was not asked for is None.

    ids:         int32 `[B, H, W]`, the id of the pixel's kept region, -1 for unlabeled pixels and dropped regions
                 (never truncated to R)
    num:         int32 `[B]`, the true number of kept regions, also above R
    label, area, anchor: int32 `[B, R]`, the region's class, pixels and smallest linear index `y * W + x`
    boxes:       int32 `[B, R, 4]`, `(y0, x0, y1, x1)` with exclusive ends
    sums:        int64 `[B, R, 2]`, `(sum of y, sum of x)` over the region's pixels
    peak, peak_scores: int32 / float32 `[B, R]`, the region's best-scoring pixel (linear index) and its score; None
                 without scores
    labels:      uint8 `[B, H, W]`, the map without the dropped regions (`return_labels=True`)
    indices:     int64 `[B]` dataset indices, carried over from a `LabelMaps`
    Rows at and above `min(num[b], R)` read (-1, 0, -1, zeros, zeros, -1, -inf)."""

    ids: Tensor
    num: Tensor
    label: Tensor
    area: Tensor
    anchor: Tensor
    boxes: Tensor
    sums: Tensor
    peak: Tensor | None = None
    peak_scores: Tensor | None = None
    labels: Tensor | None = None
    indices: Tensor | None = None

    def to(self, device: str | torch.device) -> "Regions":
        return Regions(*(None if t is None else t.to(device)
                         for t in (self.ids, self.num, self.label, self.area, self.anchor, self.boxes, self.sums,
                                   self.peak, self.peak_scores, self.labels, self.indices)))

    def cpu(self) -> "Regions":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.ids.device

    def __len__(self) -> int:
        return self.ids.shape[0]

    def centroids(self) -> Tensor:
        """float64 `[B, R, 2]`, `(y, x) = sums / area`; NaN for empty rows."""
        area = self.area.to(torch.float64).unsqueeze(-1)
        return torch.where(area > 0, self.sums.to(torch.float64) / area, torch.full_like(area, math.nan))

    def peak_cells(self, grid: "tuple[int, int]") -> Tensor:
        """int64 `[B, R]`: the cell of an `h x w` grid over the image that contains the peak pixel's centre,
        `((2y + 1) * h // (2H)) * w + (2x + 1) * w // (2W)`, -1 for empty rows.  With an image's row offset in a patch
        bank this is the row to hand to `bank.search_rows`."""
        if self.peak is None:
            raise ValueError("these regions were found without scores: there are no peaks")
        h, w = _check_size(grid)
        big_h, big_w = self.ids.shape[1:]
        peak = self.peak.to(torch.int64)
        y, x = peak // big_w, peak % big_w
        cell = ((2 * y + 1) * h // (2 * big_h)) * w + (2 * x + 1) * w // (2 * big_w)
        return torch.where(peak >= 0, cell, torch.full_like(cell, -1))

    def embed(self, maps: "EmbeddingBatch | Tensor", **kw: object) -> "RegionVectors":
        """`pool_regions(maps, self.ids, R, **kw)`, R the rows of these tables: a vector per region, pooled from the
        patch map over the region's pixels, with `label`, `num` and `indices` carried over."""
        out = pool_regions(maps, self.ids, int(self.label.shape[1]), **kw)
        return RegionVectors(out.vectors, out.mass, out.weights, self.label, self.num, self.indices)

    def outlines(self, **kw: object) -> "RegionOutlines":
        """`trace_regions(self.ids, R, **kw)`, R the rows of these tables: the outline of every region as polygon rings,
        with `label`, `num` and `indices` carried over.  Pass the `connectivity` the regions were found with."""
        out = trace_regions(self.ids, int(self.label.shape[1]), **kw)
        return RegionOutlines(out.packed, out.ring_area2, out.num_rings, out.num_vertices, out.size, out.max_rings,
                              out.max_vertices, self.label, self.num, self.indices)

    def match(self, other: "Regions", **kw: object) -> "RegionMatches":
        """`match_regions(self, other, R, R', **kw)`, R and R' the rows of the two tables: the region of `other` every
        region here fits best."""
        if not isinstance(other, Regions):
            raise TypeError(f"other must be a Regions (match_regions takes rasters), got {type(other).__name__}")
        return match_regions(self, other, int(self.label.shape[1]), int(other.label.shape[1]), **kw)


def label_regions_geometry() -> tuple[int, int]:
    """(tile_w, tile_h) of `isc_label_regions`' first pass."""
    tw, th = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().isc_label_regions_geometry(tw, th), "isc_label_regions_geometry")
    return tw.value, th.value


def _check_count(name: str, value: object) -> int:
    if isinstance(value, bool) or not isinstance(value, int):
        raise TypeError(f"{name} must be an int, got {type(value).__name__}")
    if value < 1:
        raise ValueError(f"{name} must be at least 1, got {value}")
    return value


def label_regions(labels: "Tensor | LabelMaps", *, scores: Tensor | None = None, connectivity: int = 8, min_area: int = 1,
                  max_regions: int = 1024, return_labels: bool = False) -> Regions:
    """The connected regions of label maps (`isc_label_regions`, include/imagescry_hip.h has the definition): two pixels
    of one image belong to one region if they carry the same label (not `UNLABELED`) and are linked through neighbours
    that do -- across edges (`connectivity=4`) or edges and corners (`8`).  Regions of fewer than `min_area` pixels are
    dropped; the others are numbered from 0 in raster order of their first pixel, per image.

    `labels`: uint8 `[B, H, W]` or a `LabelMaps` (whose `scores` then score the peaks unless `scores` is given, and whose
    `indices` are carried over).  `scores`: float32 `[B, H, W]`; without them `Regions.peak` / `.peak_scores` are None.
    `max_regions`: rows an image in the tables; `Regions.num` holds the true count, so `num > max_regions` tells of a
    truncated table without a host read here.  `return_labels`: also the map with the dropped regions unlabeled.
    Integers throughout: deterministic, the same for an image wherever it stands in a batch, capturable.  Nothing
    synchronises with the host."""
    indices = None
    if isinstance(labels, LabelMaps):
        indices = labels.indices
        if scores is None:
            scores = labels.scores
        labels = labels.labels
    if not isinstance(labels, Tensor):
        raise TypeError(f"labels must be a torch.Tensor or LabelMaps, got {type(labels).__name__}")
    if labels.dtype != torch.uint8:
        raise TypeError(f"labels must be uint8, got {labels.dtype}")
    if labels.ndim != 3:
        raise ValueError(f"labels must have shape [B, H, W], got {tuple(labels.shape)}")
    if scores is not None:
        scores = _check_float_tensor("scores", scores, 3, "[B, H, W]")
        if scores.shape != labels.shape:
            raise ValueError(f"scores {tuple(scores.shape)} must have the shape of labels {tuple(labels.shape)}")
    if isinstance(connectivity, bool) or not isinstance(connectivity, int):
        raise TypeError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    min_area = _check_count("min_area", min_area)
    rows = _check_count("max_regions", max_regions)
    b, big_h, big_w = (int(v) for v in labels.shape)
    _check_size((big_h, big_w))
    if scores is not None and min(rows, big_h * big_w) > max(1024, big_h * big_w // 8):
        raise ValueError(f"with scores, max_regions may be at most max(1024, H * W / 8) = "
                         f"{max(1024, big_h * big_w // 8)} for {big_h} x {big_w} images, got {rows}")
    _lib.require_device(labels, "labels")
    device = labels.device
    if scores is not None and scores.device != device:
        raise ValueError(f"labels are on {device} but scores on {scores.device}")
    labels = labels.contiguous()
    scores = None if scores is None else scores.contiguous()
    lib = _lib.load()
    need = ctypes.c_size_t()
    _lib.check(lib.isc_label_regions_workspace_bytes(b, big_h, big_w, need), "isc_label_regions_workspace_bytes")

    def table(*shape: int, dtype: torch.dtype = torch.int32) -> Tensor:
        return torch.empty((b, rows, *shape), dtype=dtype, device=device)

    ids = torch.empty((b, big_h, big_w), dtype=torch.int32, device=device)
    num = torch.empty((b,), dtype=torch.int32, device=device)
    kept = torch.empty_like(labels) if return_labels else None
    label, area, anchor, boxes, sums = table(), table(), table(), table(4), table(2, dtype=torch.int64)
    peak = None if scores is None else table()
    peak_scores = None if scores is None else table(dtype=torch.float32)
    workspace = torch.empty((need.value,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        st = lib.isc_label_regions(labels.data_ptr(), _lib.ptr(scores), b, big_h, big_w, connectivity, min_area, rows,
                                   ids.data_ptr(), num.data_ptr(), _lib.ptr(kept), label.data_ptr(), area.data_ptr(),
                                   anchor.data_ptr(), boxes.data_ptr(), sums.data_ptr(), _lib.ptr(peak),
                                   _lib.ptr(peak_scores), workspace.data_ptr(), need.value, _lib.stream_handle(device))
    _lib.check(st, "isc_label_regions")
    return Regions(ids, num, label, area, anchor, boxes, sums, peak, peak_scores, kept, indices)


# ------------------------------------------------------------------------------------------------------ region vectors
MAX_POOL_PIXELS = 2**24  # isc_region_cell_weights: H * W <= 2^24, every weight below 2^50
MAX_POOL_TABLE = 2**25  # ... and R * h * w <= 2^25
MAX_POOLED_MAPS = 65535  # images a launch
POOL_PASS_BYTES = 256 << 20  # the weights of one pass of pool_regions


@dataclass(frozen=True)
class RegionVectors:
    """What `pool_regions` returns, R rows an image; a field that was not asked for or not known is None.

    vectors: float32 `[B, R, E]`, the pooled map of every region: unit length (`normalize=True`) or the mean of the
             upsampled map over the region's pixels; zeros for a region without pixels
    mass:    int64 `[B, R]`, `4 * H * W *` the region's pixels
    weights: int64 `[B, R, h, w]`, what `region_cell_weights` returns (`return_weights=True`)
    label, num, indices: the regions' classes int32 `[B, R]`, their true number int32 `[B]` and the images' dataset
             indices int64 `[B]`, carried over from a `Regions` (`Regions.embed`)"""

    vectors: Tensor
    mass: Tensor
    weights: Tensor | None = None
    label: Tensor | None = None
    num: Tensor | None = None
    indices: Tensor | None = None

    def to(self, device: str | torch.device) -> "RegionVectors":
        return RegionVectors(*(None if t is None else t.to(device)
                               for t in (self.vectors, self.mass, self.weights, self.label, self.num, self.indices)))

    def cpu(self) -> "RegionVectors":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.vectors.device

    def __len__(self) -> int:
        return self.vectors.shape[0]

    def valid(self) -> Tensor:
        """bool `[B, R]`: the rows of regions that have pixels (`mass > 0`)."""
        return self.mass > 0

    def flat(self) -> tuple[Tensor, Tensor, Tensor]:
        """The valid rows as `(vectors [M, E], image int64 [M], region int64 [M])`, image major: what an
        `EmbeddingBank(vectors, row_groups=image)` takes.  `image` is the dataset index where `indices` are known, the
        place in the batch otherwise.  This synchronises with the host, which has to learn M."""
        image, region = torch.nonzero(self.valid(), as_tuple=True)
        vectors = self.vectors[image, region]
        if self.indices is not None:
            image = self.indices.to(device=image.device, dtype=torch.int64)[image]
        return vectors, image, region


def region_pool_geometry() -> tuple[int, int]:
    """(tile_w, tile_h): the pixels a workgroup of `isc_region_cell_weights` owns."""
    tw, th = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().isc_region_pool_geometry(tw, th), "isc_region_pool_geometry")
    return tw.value, th.value


def _check_region_ids(ids: object, num_regions: object, grid: tuple[int, int]) -> tuple[Tensor, int]:
    if not isinstance(ids, Tensor):
        raise TypeError(f"ids must be a torch.Tensor, got {type(ids).__name__}")
    if ids.dtype != torch.int32:
        raise TypeError(f"ids must be int32, got {ids.dtype}")
    if ids.ndim != 3:
        raise ValueError(f"ids must have shape [B, H, W], got {tuple(ids.shape)}")
    rows = _check_count("num_regions", num_regions)
    big_h, big_w = (int(v) for v in ids.shape[1:])
    h, w = grid
    if big_h < 1 or big_w < 1:
        raise ValueError(f"ids must hold at least one pixel an image, got {big_h} x {big_w}")
    if big_h * big_w > MAX_POOL_PIXELS:
        raise ValueError(f"ids of {big_h} x {big_w} pixels exceed the 2^24 pixels the integer weights are exact for")
    if rows * h * w > MAX_POOL_TABLE:
        raise ValueError(f"{rows} regions x {h} x {w} cells exceed the 2^25 entries an image of the weights table")
    return ids, rows


def _cell_weights(ids: Tensor, rows: int, grid: tuple[int, int], out: Tensor) -> None:
    """isc_region_cell_weights of contiguous `ids` (at most 65 535 images) into contiguous `out`."""
    big_h, big_w = (int(v) for v in ids.shape[1:])
    with torch.cuda.device(ids.device):
        st = _lib.load().isc_region_cell_weights(ids.data_ptr(), ids.shape[0], big_h, big_w, *grid, rows, out.data_ptr(),
                                                 _lib.stream_handle(ids.device))
    _lib.check(st, "isc_region_cell_weights")


def region_cell_weights(ids: Tensor, num_regions: int, grid: "tuple[int, int]") -> Tensor:
    """How much every cell of an `h x w` grid counts for every region of `ids` (int32 `[B, H, W]` on the device,
    `Regions.ids` or any raster mask; negative ids and ids at or above `num_regions` are skipped) when the grid is
    upsampled bilinearly (`align_corners=False`) to `H x W` and summed over the region's pixels: int64 `[B, R, h, w]`,
    exact integers (`isc_region_cell_weights`, include/imagescry_hip.h has the definition).  `weights / (4 * H * W)` is
    the antialiased coverage of each cell by each region and sums to the region's area; `weights > 0` marks the cells a
    region touches under the bilinear support, the device-side analogue of the reference's
    `create_roi_mask(all_touched=True)` for masks that are rasters already.  Deterministic, capturable, nothing
    synchronises."""
    h, w = _check_size(grid)
    ids, rows = _check_region_ids(ids, num_regions, (h, w))
    _lib.require_device(ids, "ids")
    out = torch.empty((ids.shape[0], rows, h, w), dtype=torch.int64, device=ids.device)
    ids = ids.contiguous()
    for i in range(0, ids.shape[0], MAX_POOLED_MAPS):  # images a launch
        _cell_weights(ids[i:i + MAX_POOLED_MAPS], rows, (h, w), out[i:i + MAX_POOLED_MAPS])
    return out


def pool_regions(maps: "EmbeddingBatch | Tensor", ids: Tensor, num_regions: int, *, normalize: bool = True,
                 return_weights: bool = False) -> RegionVectors:
    """A vector per region: `maps` (an `EmbeddingBatch` or float32 `[B, E, h, w]`) upsampled bilinearly to the pixels of
    `ids` (int32 `[B, H, W]`) and averaged over each region's pixels -- computed as a weighted sum over cells with the
    exact integer weights of `region_cell_weights`, in float64 chains of a fixed order (`isc_region_pool`), so neither the
    `[B, E, H, W]` upsampling is written nor a float summed by atomics: deterministic bit for bit and capturable.

    `ids` may have any `H, W`: an upsampled `Regions.ids`, or a mask drawn on the feature grid itself (`H == h, W == w`:
    plain masked mean pooling); downsampling is defined as well.  `normalize=True` gives rows of unit length (a bank's
    rows, in the text tower's space for a CLIP map), `False` the mean.  Rows of regions without pixels are zeros with
    mass 0.  `return_weights` also returns the `[B, R, h, w]` weights.  Runs in passes of images whose weights stay within
    256 MiB; the number of launches depends on the shapes alone, and nothing synchronises with the host."""
    if isinstance(maps, EmbeddingBatch):
        maps = maps.embeddings
    maps = _check_float_tensor("maps", maps, 4, "[B, E, h, w]")
    b, e, h, w = (int(v) for v in maps.shape)
    if e < 1 or h < 1 or w < 1:
        raise ValueError(f"maps {tuple(maps.shape)} must not be empty")
    if h * w >= 2**31:
        raise ValueError(f"a {h} x {w} map has 2^31 cells or more")
    ids, rows = _check_region_ids(ids, num_regions, (h, w))
    if ids.shape[0] != b:
        raise ValueError(f"maps hold {b} images but ids {ids.shape[0]}")
    if not isinstance(normalize, bool) or not isinstance(return_weights, bool):
        raise TypeError("normalize and return_weights must be bools")
    _lib.require_device(maps, "maps")
    device = maps.device
    if ids.device != device:
        raise ValueError(f"maps are on {device} but ids on {ids.device}")
    maps, ids = maps.contiguous(), ids.contiguous()
    cells = h * w
    step = max(1, min(POOL_PASS_BYTES // (rows * cells * 8), MAX_POOLED_MAPS))  # images a pass
    vectors = torch.empty((b, rows, e), dtype=torch.float32, device=device)
    mass = torch.empty((b, rows), dtype=torch.int64, device=device)
    weights = torch.empty((b if return_weights else min(b, step), rows, h, w), dtype=torch.int64, device=device)
    mode = _lib.ISC_POOL_UNIT if normalize else _lib.ISC_POOL_MEAN
    lib = _lib.load()
    for i in range(0, b, step):
        n = min(step, b - i)
        part = weights[i:i + n] if return_weights else weights[:n]
        _cell_weights(ids[i:i + n], rows, (h, w), part)
        with torch.cuda.device(device):
            st = lib.isc_region_pool(maps[i:i + n].data_ptr(), n, e, cells, part.data_ptr(), rows, mode,
                                     vectors[i:i + n].data_ptr(), mass[i:i + n].data_ptr(), _lib.stream_handle(device))
        _lib.check(st, "isc_region_pool")
    return RegionVectors(vectors, mass, weights if return_weights else None)


# ------------------------------------------------------------------------------------------------------ drawn regions
RASTER_FRACTION = 256  # vertices are fixed point: q = 256 * coordinate
MAX_RASTER_SIDE = 32768  # isc_rasterize_polygons: H, W <= 32768
MAX_RASTER_IMAGES = 65535  # images a launch
FILL_RULES = {"evenodd": _lib.ISC_FILL_EVENODD, "nonzero": _lib.ISC_FILL_NONZERO}


@dataclass(frozen=True)
class PackedPolygons:
    """Polygons of B images, snapped to 1/256 pixel and flattened: what `isc_rasterize_polygons` reads.

    vertices:    int32 `[V, 2]`, `(256 x, 256 y)`
    ring_start:  int32 `[N + 1]`, ring n is `vertices[ring_start[n]:ring_start[n + 1]]`, closed
    ring_region: int32 `[N]`, the region of the ring's shape; consecutive rings of one image with one value are one shape
    image_start: int32 `[B + 1]`, image b owns rings `image_start[b]:image_start[b + 1]`
    num_regions: the most shapes any image has, at least 1: the R of the tables downstream

    The tensors may be refilled in place (same sizes) between the replays of a captured graph."""

    vertices: Tensor
    ring_start: Tensor
    ring_region: Tensor
    image_start: Tensor
    num_regions: int

    def to(self, device: str | torch.device) -> "PackedPolygons":
        return PackedPolygons(self.vertices.to(device), self.ring_start.to(device), self.ring_region.to(device),
                              self.image_start.to(device), self.num_regions)

    def cpu(self) -> "PackedPolygons":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.vertices.device

    def __len__(self) -> int:
        return self.image_start.shape[0] - 1


def rasterize_geometry() -> tuple[int, int, int]:
    """(tile_w, tile_h, edge_chunk) of `isc_rasterize_polygons`."""
    tw, th, ec = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().isc_rasterize_polygons_geometry(tw, th, ec), "isc_rasterize_polygons_geometry")
    return tw.value, th.value, ec.value


def _check_raster_size(name: str, size: object) -> tuple[int, int]:
    try:
        h, w = _check_size(size)
    except (TypeError, ValueError) as exc:
        raise type(exc)(str(exc).replace("size", name, 1)) from None
    return h, w


def _is_number(v: object) -> bool:
    if isinstance(v, Tensor):
        return v.ndim == 0
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _ring_array(ring: object) -> np.ndarray:
    """One ring as float64 `[V, 2]`."""
    if isinstance(ring, Tensor):
        a = ring.detach().cpu().to(torch.float64).numpy()
    else:
        try:
            a = np.asarray(ring if isinstance(ring, np.ndarray) else [tuple(float(c) for c in v) for v in ring],
                           dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise TypeError(f"a ring must be a [V, 2] array-like of (x, y), got {type(ring).__name__}") from exc
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"a ring must have shape [V, 2], got {tuple(a.shape)}")
    if a.shape[0] < 3:
        raise ValueError(f"a ring needs at least 3 vertices, got {a.shape[0]}")
    if not np.isfinite(a).all():
        raise ValueError("a ring holds a coordinate that is not finite")
    return a


def _shape_rings(shape: object) -> list[np.ndarray]:
    """The rings of one shape: a ring, a list of rings, a polygon-like (`.exterior.coords`, `.interiors`) or a
    multipolygon-like (`.geoms`)."""
    if hasattr(shape, "geoms"):
        return [ring for part in shape.geoms for ring in _shape_rings(part)]
    if hasattr(shape, "exterior"):
        return [_ring_array(shape.exterior.coords), *(_ring_array(hole.coords) for hole in shape.interiors)]
    if isinstance(shape, (Tensor, np.ndarray)):
        return [_ring_array(ring) for ring in shape] if shape.ndim == 3 else [_ring_array(shape)]
    if isinstance(shape, (list, tuple)):
        if len(shape) == 0:
            raise ValueError("a shape must hold at least one ring")
        first = shape[0]
        if isinstance(first, (list, tuple)) and len(first) == 2 and all(_is_number(v) for v in first):
            return [_ring_array(shape)]
        if isinstance(first, (Tensor, np.ndarray)) and first.ndim == 1:
            return [_ring_array(np.stack([np.asarray(v, dtype=np.float64) for v in shape]))]
        return [_ring_array(ring) for ring in shape]
    raise TypeError(f"a shape must be a [V, 2] ring, a list of rings, or an object with .exterior / .geoms, "
                    f"got {type(shape).__name__}")


def pack_polygons(polygons: object, *, size: "tuple[int, int] | None" = None,
                  extent: "tuple[int, int] | None" = None) -> PackedPolygons:
    """Snap and flatten polygons on the host.  `polygons`: a list with one entry per image, each a list of shapes; the
    region id of a shape is its place in that list.  A shape is a `[V, 2]` array-like or tensor of `(x, y)` (one ring), a
    list of rings (an exterior and its holes, or the parts of a multipolygon), any object with `.exterior.coords` and
    `.interiors`, or any object with `.geoms` holding such objects -- shapely's `Polygon` and `MultiPolygon` fit without
    shapely being imported.  x runs right, y down, pixel `(y, x)` covers `[x, x + 1) x [y, y + 1)`.

    With `size=(H, W)` and `extent=(H0, W0)` the polygons are given on an `H0 x W0` image and scaled onto `H x W`:
    `sx = W / W0`, `sy = H / H0`; otherwise both are 1.  Snapping is `q = rint(x * sx * 256.0)`, left to right in
    float64, halves to even.  `ValueError`: a ring of fewer than 3 vertices, a coordinate that is not finite, or
    `|q| > 2^23` (32768 pixels)."""
    sx = sy = 1.0
    if size is not None:
        out_h, out_w = _check_raster_size("size", size)
    if extent is not None:
        ext_h, ext_w = _check_raster_size("extent", extent)
        if size is None:
            raise ValueError("extent needs size: the grid the polygons are scaled onto")
        sx, sy = out_w / ext_w, out_h / ext_h
    if not isinstance(polygons, (list, tuple)):
        raise TypeError(f"polygons must be a list with one list of shapes per image, got {type(polygons).__name__}")
    verts: list[np.ndarray] = []
    ring_start, ring_region, image_start = [0], [], [0]
    most = 1
    for shapes in polygons:
        if not isinstance(shapes, (list, tuple)):
            raise TypeError(f"every image's entry must be a list of shapes, got {type(shapes).__name__}")
        most = max(most, len(shapes))
        for region, shape in enumerate(shapes):
            for ring in _shape_rings(shape):
                q = np.stack([np.rint(ring[:, 0] * sx * 256.0), np.rint(ring[:, 1] * sy * 256.0)], axis=1)
                if np.abs(q).max() > _lib.ISC_RASTER_MAX_COORD:
                    raise ValueError(f"a vertex lies beyond {MAX_RASTER_SIDE} pixels from the origin after scaling")
                verts.append(q.astype(np.int32))
                ring_start.append(ring_start[-1] + q.shape[0])
                ring_region.append(region)
        image_start.append(len(ring_region))
    if ring_start[-1] >= 2**31:
        raise ValueError("2^31 vertices or more")
    vertices = np.concatenate(verts, axis=0) if verts else np.zeros((0, 2), dtype=np.int32)
    return PackedPolygons(torch.from_numpy(vertices), torch.tensor(ring_start, dtype=torch.int32),
                          torch.tensor(ring_region, dtype=torch.int32), torch.tensor(image_start, dtype=torch.int32), most)


def _check_packed(pack: PackedPolygons) -> None:
    fields = (("vertices", pack.vertices), ("ring_start", pack.ring_start), ("ring_region", pack.ring_region),
              ("image_start", pack.image_start))
    for name, t in fields:
        if not isinstance(t, Tensor) or t.dtype != torch.int32:
            raise TypeError(f"PackedPolygons.{name} must be an int32 tensor")
        if t.device != pack.vertices.device:
            raise ValueError(f"PackedPolygons.{name} is on {t.device} but vertices on {pack.vertices.device}")
    if pack.vertices.ndim != 2 or pack.vertices.shape[1] != 2:
        raise ValueError(f"PackedPolygons.vertices must have shape [V, 2], got {tuple(pack.vertices.shape)}")
    if pack.ring_region.ndim != 1 or pack.ring_start.shape != (pack.ring_region.shape[0] + 1,):
        raise ValueError("PackedPolygons.ring_start must have one entry more than ring_region")
    if pack.image_start.ndim != 1 or pack.image_start.shape[0] < 1:
        raise ValueError("PackedPolygons.image_start must have shape [B + 1]")


def _some(t: Tensor) -> Tensor:
    """`t`, or one element where it is empty: the kernels take no NULL."""
    return t.contiguous() if t.numel() else torch.zeros((2,), dtype=t.dtype, device=t.device)


def rasterize_polygons(polygons: object, size: "tuple[int, int]", *, extent: "tuple[int, int] | None" = None,
                       fill_rule: str = "evenodd", all_touched: bool = False, num_regions: int | None = None,
                       return_counts: bool = False,
                       device: "str | torch.device | None" = None) -> "Tensor | tuple[Tensor, Tensor]":
    """Polygons to region ids on the device (`isc_rasterize_polygons`, include/imagescry_hip.h has the definition): int32
    `[B, H, W]`, every pixel the region of the LAST shape of its image that covers it (rasterio's order for a list of
    shapes), -1 where none does; with `return_counts` also int32 `[B, R]`, the pixels of every region.

    `polygons`: what `pack_polygons` takes (packed here with `size` and `extent`) or a `PackedPolygons`, which is moved to
    `device` if it lives on the CPU; `device=None` is where the pack lives, else the current GPU.  A shape covers a pixel
    whose centre lies inside it -- by the parity of crossings (`fill_rule="evenodd"`: holes are holes whatever their
    orientation) or by the winding number (`"nonzero"`) -- under the top-left rule, so shapes that share an edge partition
    the pixels; with `all_touched=True` also every pixel whose interior an edge of the shape passes through (rasterio's
    `all_touched`, GDAL's ALL_TOUCHED).  `extent=(H0, W0)`: the polygons are given on an `H0 x W0` image.  `num_regions`:
    R, by default the pack's; shapes at or beyond it are skipped.  Integers throughout: deterministic, the same for an
    image wherever it stands in a batch, capturable; nothing synchronises with the host."""
    big_h, big_w = _check_raster_size("size", size)
    if big_h > MAX_RASTER_SIDE or big_w > MAX_RASTER_SIDE:
        raise ValueError(f"size {big_h} x {big_w} exceeds {MAX_RASTER_SIDE} pixels a side")
    if not isinstance(fill_rule, str) or fill_rule not in FILL_RULES:
        raise ValueError(f"fill_rule must be one of {sorted(FILL_RULES)}, got {fill_rule!r}")
    if not isinstance(all_touched, bool) or not isinstance(return_counts, bool):
        raise TypeError("all_touched and return_counts must be bools")
    if isinstance(polygons, PackedPolygons):
        if extent is not None:
            raise ValueError("a PackedPolygons is scaled already: give extent to pack_polygons")
        pack = polygons
    else:
        pack = pack_polygons(polygons, size=(big_h, big_w), extent=extent)
    _check_packed(pack)
    rows = pack.num_regions if num_regions is None else num_regions
    rows = _check_count("num_regions", rows)
    if device is not None:
        device = torch.device(device)
    if pack.device.type == "cpu":
        pack = pack.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    elif device is not None and device != pack.device and (device.index is not None or device.type != pack.device.type):
        raise ValueError(f"the polygons are on {pack.device} but device is {device}")
    _lib.require_device(pack.vertices, "polygons")
    device = pack.device
    b, rings = len(pack), int(pack.ring_region.shape[0])
    ids = torch.empty((b, big_h, big_w), dtype=torch.int32, device=device)
    counts = torch.empty((b, rows), dtype=torch.int32, device=device) if return_counts else None
    lib = _lib.load()
    need = ctypes.c_size_t()
    _lib.check(lib.isc_rasterize_polygons_workspace_bytes(rings, need), "isc_rasterize_polygons_workspace_bytes")
    workspace = torch.empty((need.value,), dtype=torch.uint8, device=device)
    vertices, ring_start, ring_region = _some(pack.vertices), pack.ring_start.contiguous(), _some(pack.ring_region)
    image_start = pack.image_start.contiguous()
    for i in range(0, b, MAX_RASTER_IMAGES):  # images a launch; image_start holds offsets into all the rings
        n = min(MAX_RASTER_IMAGES, b - i)
        with torch.cuda.device(device):
            st = lib.isc_rasterize_polygons(vertices.data_ptr(), ring_start.data_ptr(), ring_region.data_ptr(),
                                            image_start[i:].data_ptr(), n, big_h, big_w, rows, FILL_RULES[fill_rule],
                                            int(all_touched), ids[i:i + n].data_ptr(),
                                            None if counts is None else counts[i:i + n].data_ptr(), workspace.data_ptr(),
                                            need.value, _lib.stream_handle(device))
        _lib.check(st, "isc_rasterize_polygons")
    return (ids, counts) if return_counts else ids


def create_roi_mask(roi: object, original_image_shape: "tuple[int, int]", feature_map_shape: "tuple[int, int]",
                    class_index: int = 1, *, device: "str | torch.device | None" = None) -> Tensor:
    """The reference's `geometry.create_roi_mask`, on the device: `roi` -- one shape or a list of shapes (what
    `pack_polygons` takes for one image), drawn on an image of `original_image_shape = (h, w)` -- burnt onto the
    `feature_map_shape = (hf, wf)` grid with `all_touched=True`: int64 `[hf, wf]` holding `class_index` where any shape
    covers or touches the cell and 0 elsewhere."""
    if isinstance(class_index, bool) or not isinstance(class_index, int):
        raise TypeError(f"class_index must be an int, got {type(class_index).__name__}")
    extent = tuple(int(v) for v in original_image_shape)
    grid = tuple(int(v) for v in feature_map_shape)
    single = not isinstance(roi, (list, tuple)) or (
        len(roi) > 0 and isinstance(roi[0], (list, tuple)) and len(roi[0]) == 2 and all(_is_number(v) for v in roi[0]))
    shapes = [roi] if single else list(roi)
    ids = rasterize_polygons([shapes], grid, extent=extent, all_touched=True, device=device)
    return (ids[0] >= 0).to(torch.int64) * class_index


def pool_polygons(maps: "EmbeddingBatch | Tensor", polygons: object, size: "tuple[int, int]", *,
                  extent: "tuple[int, int] | None" = None, fill_rule: str = "evenodd", all_touched: bool = False,
                  **pool_kw: object) -> RegionVectors:
    """A vector per drawn shape: `pool_regions(maps, rasterize_polygons(polygons, size, ...), R, **pool_kw)` with R the
    most shapes an image has -- `maps` upsampled to `size` and averaged over every shape's pixels, rows of unit length by
    default: what `bank.search` takes for "more like what I outlined"."""
    tensor = maps.embeddings if isinstance(maps, EmbeddingBatch) else maps
    if not isinstance(tensor, Tensor):
        raise TypeError(f"maps must be an EmbeddingBatch or a torch.Tensor, got {type(maps).__name__}")
    _lib.require_device(tensor, "maps")
    pack = polygons if isinstance(polygons, PackedPolygons) else pack_polygons(polygons, size=_check_raster_size("size", size),
                                                                              extent=extent)
    if isinstance(polygons, PackedPolygons) and extent is not None:
        raise ValueError("a PackedPolygons is scaled already: give extent to pack_polygons")
    if len(pack) != tensor.shape[0]:
        raise ValueError(f"maps hold {tensor.shape[0]} images but the polygons {len(pack)}")
    ids = rasterize_polygons(pack, size, fill_rule=fill_rule, all_touched=all_touched,
                             device=tensor.device if pack.device.type == "cpu" else None)
    return pool_regions(tensor, ids, pack.num_regions, **pool_kw)


# ----------------------------------------------------------------------------------------------------- region outlines
MAX_TRACE_PIXELS = 2**29  # isc_trace_regions: H * W < 2^29, the 4 H W possible vertices are counted in an int32


@dataclass(frozen=True)
class RegionOutlines:
    """What `trace_regions` returns: the outlines of the regions of B id maps as closed rings on the pixel lattice, N =
    `max_rings` rows and V = `max_vertices` vertices an image.

    packed:       a `PackedPolygons` over the call's four arrays (a view, nothing copied): vertices `[B * V, 2]`,
                  ring_start `[B * (N + 1) + 1]`, ring_region `[B * (N + 1)]`, image_start `[B + 1]`.  Image b owns rings
                  `b * (N + 1) + j`; unused rows have region -1 and no vertices.  `rasterize_polygons(packed, size,
                  num_regions=R)` gives back the ids under either fill rule.
    ring_area2:   int64 `[B, N]`, twice the signed area: positive for a ring with its region inside, negative for a hole,
                  0 for unused rows
    num_rings, num_vertices: int32 `[B]`, the TRUE counts, also above N and V.  An image that does not fit is written as
                  empty; `complete()` tells, and the counts are the capacities to retry with.
    size:         `(H, W)`;  max_rings, max_vertices: N and V
    label, num, indices: carried over by `Regions.outlines`, else None."""

    packed: PackedPolygons
    ring_area2: Tensor
    num_rings: Tensor
    num_vertices: Tensor
    size: tuple[int, int]
    max_rings: int
    max_vertices: int
    label: Tensor | None = None
    num: Tensor | None = None
    indices: Tensor | None = None

    def to(self, device: str | torch.device) -> "RegionOutlines":
        return RegionOutlines(self.packed.to(device), self.ring_area2.to(device), self.num_rings.to(device),
                              self.num_vertices.to(device), self.size, self.max_rings, self.max_vertices,
                              *(None if t is None else t.to(device) for t in (self.label, self.num, self.indices)))

    def cpu(self) -> "RegionOutlines":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.ring_area2.device

    def __len__(self) -> int:
        return self.ring_area2.shape[0]

    def complete(self) -> Tensor:
        """bool `[B]`: the image's rings and vertices fit `max_rings` and `max_vertices`."""
        return (self.num_rings <= self.max_rings) & (self.num_vertices <= self.max_vertices)

    def holes(self) -> Tensor:
        """bool `[B, N]`: the ring is a hole (`ring_area2 < 0`)."""
        return self.ring_area2 < 0

    def shapes(self, *, strict: bool = True) -> "list[list[list[np.ndarray]]]":
        """The outlines on the host -- the one call here that synchronises.  Per image a list of length R (the
        `num_regions` of the call); entry r is the list of that region's rings as float64 `[n, 2]` arrays of `(x, y)` in
        pixels, ordered by start vertex.  A non-empty entry is what `pack_polygons` takes for a shape.  For a connected
        region it is the exterior followed by its holes: the arguments of `shapely.Polygon(shell, holes)`.  A region of
        several components is a list of rings for even-odd fill, not a list of polygons: holes are not assigned to
        exteriors.  An incomplete image (`complete()`) raises `ValueError` unless `strict=False`, with which it is
        empty."""
        if not isinstance(strict, bool):
            raise TypeError("strict must be a bool")
        n = self.max_rings
        host = self.cpu()
        fits = host.complete().tolist()
        if strict and not all(fits):
            b = fits.index(False)
            raise ValueError(f"image {b} has {int(host.num_rings[b])} rings and {int(host.num_vertices[b])} vertices: "
                             f"beyond max_rings = {n} or max_vertices = {self.max_vertices}; trace it again with those")
        vertices = host.packed.vertices.to(torch.float64).numpy() / RASTER_FRACTION
        start = host.packed.ring_start.numpy()
        region = host.packed.ring_region.numpy()
        out = []
        for b in range(len(host)):
            per_region: list[list[np.ndarray]] = [[] for _ in range(host.packed.num_regions)]
            for j in range(min(int(host.num_rings[b]), n) if fits[b] else 0):
                k = b * (n + 1) + j
                per_region[int(region[k])].append(vertices[start[k]:start[k + 1]].copy())
            out.append(per_region)
        return out


def trace_geometry() -> tuple[int, int, int, int]:
    """(pixel_chunk, node_chunk, ring_tile, node_pass) of `isc_trace_regions`."""
    pc, nc, rt, np_ = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().isc_trace_regions_geometry(pc, nc, rt, np_), "isc_trace_regions_geometry")
    return pc.value, nc.value, rt.value, np_.value


def trace_regions(ids: Tensor, num_regions: int, *, connectivity: int = 8, max_rings: int | None = None,
                  max_vertices: int | None = None) -> RegionOutlines:
    """Region ids back to outlines on the device (`isc_trace_regions`, include/imagescry_hip.h has the definition): the
    boundary of every region r in `[0, num_regions)` of int32 `[B, H, W]` `ids` as closed rings of lattice vertices --
    corners only, the region on the right of the direction of travel, holes as rings of negative area -- ordered by
    (region, start vertex).  The inverse of `rasterize_polygons`, rasterio's `shapes`.

    `connectivity`: where two pixels of a region meet at a corner only, 8 runs one ring through the corner and 4 keeps
    the rings apart; use what `label_regions` used.  `max_rings` (N) and `max_vertices` (V): the rows an image has; the
    defaults `2 * num_regions` and `max(4096, H * W // 4)` are heuristics, not bounds -- the worst case is `H * W` rings
    and `4 * H * W` vertices -- and `RegionOutlines.num_rings` / `.num_vertices` hold the true counts: an image beyond
    either comes out empty, `complete()` says so without a host read here, and the counts are what to call again with.
    Integers throughout: deterministic, the same for an image wherever it stands in a batch, capturable.  Nothing
    synchronises with the host."""
    if not isinstance(ids, Tensor):
        raise TypeError(f"ids must be a torch.Tensor, got {type(ids).__name__}")
    if ids.dtype != torch.int32:
        raise TypeError(f"ids must be int32, got {ids.dtype}")
    if ids.ndim != 3:
        raise ValueError(f"ids must have shape [B, H, W], got {tuple(ids.shape)}")
    rows = _check_count("num_regions", num_regions)
    if isinstance(connectivity, bool) or not isinstance(connectivity, int):
        raise TypeError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    b, big_h, big_w = (int(v) for v in ids.shape)
    _check_size((big_h, big_w))
    if big_h > MAX_RASTER_SIDE or big_w > MAX_RASTER_SIDE or big_h * big_w >= MAX_TRACE_PIXELS:
        raise ValueError(f"ids of {big_h} x {big_w} exceed {MAX_RASTER_SIDE} pixels a side or 2^29 pixels")
    if b > MAX_RASTER_IMAGES:
        raise ValueError(f"at most {MAX_RASTER_IMAGES} images a call, got {b}")
    n = _check_count("max_rings", 2 * rows if max_rings is None else max_rings)
    v = _check_count("max_vertices", max(4096, big_h * big_w // 4) if max_vertices is None else max_vertices)
    if max(b, 1) * (n + 1) >= 2**31 or max(b, 1) * v >= 2**31:
        raise ValueError(f"B * (max_rings + 1) and B * max_vertices must stay below 2^31, got B = {b}, {n} and {v}")
    _lib.require_device(ids, "ids")
    device = ids.device
    ids = ids.contiguous()
    lib = _lib.load()
    need = ctypes.c_size_t()
    _lib.check(lib.isc_trace_regions_workspace_bytes(b, big_h, big_w, need), "isc_trace_regions_workspace_bytes")

    def empty(*shape: int, dtype: torch.dtype = torch.int32) -> Tensor:
        return torch.empty(shape, dtype=dtype, device=device)

    vertices, ring_start, ring_region = empty(b * v, 2), empty(b * (n + 1) + 1), empty(b * (n + 1))
    image_start, area2 = empty(b + 1), empty(b, n, dtype=torch.int64)
    num_rings, num_vertices = empty(b), empty(b)
    if b == 0:
        ring_start.zero_()
        image_start.zero_()
    workspace = torch.empty((need.value,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        st = lib.isc_trace_regions(ids.data_ptr(), b, big_h, big_w, rows, connectivity, n, v, vertices.data_ptr(),
                                   ring_start.data_ptr(), ring_region.data_ptr(), image_start.data_ptr(),
                                   area2.data_ptr(), num_rings.data_ptr(), num_vertices.data_ptr(), workspace.data_ptr(),
                                   need.value, _lib.stream_handle(device))
    _lib.check(st, "isc_trace_regions")
    return RegionOutlines(PackedPolygons(vertices, ring_start, ring_region, image_start, rows), area2, num_rings,
                          num_vertices, (big_h, big_w), n, v)


# ------------------------------------------------------------------------------------------------------ overlap tables
MAX_OVERLAP_PIXELS = 2**31 - 1  # isc_overlap_table: H * W < 2^31
MAX_OVERLAP_TABLE = 2**25  # ... and (Ra + 1) * (Rb + 1) <= 2^25: a pair's key is a non-negative int32
MAX_OVERLAP_MAPS = 65535  # images a launch
OVERLAP_PASS_BYTES = POOL_PASS_BYTES  # the tables of one pass of match_regions: the rule of pool_regions


def overlap_geometry() -> tuple[int, int, int]:
    """(tile_w, tile_h, slots): the pixels a workgroup of `isc_overlap_table` owns and the pairs its LDS table holds."""
    tw, th, slots = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().isc_overlap_geometry(tw, th, slots), "isc_overlap_geometry")
    return tw.value, th.value, slots.value


def overlap_best_geometry() -> int:
    """The columns `isc_overlap_best` reduces at a time."""
    columns = ctypes.c_int()
    _lib.check(_lib.load().isc_overlap_best_geometry(columns), "isc_overlap_best_geometry")
    return columns.value


def _overlap_raster(name: str, t: object) -> Tensor:
    if isinstance(t, LabelMaps):
        t = t.labels
    elif isinstance(t, Regions):
        t = t.ids
    if not isinstance(t, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, LabelMaps or Regions, got {type(t).__name__}")
    if t.dtype not in (torch.uint8, torch.int32):
        raise TypeError(f"{name} must be uint8 or int32, got {t.dtype}")
    if t.ndim != 3:
        raise ValueError(f"{name} must have shape [B, H, W], got {tuple(t.shape)}")
    return t


def _check_overlap_pair(a: object, b: object, num_a: object, num_b: object) -> tuple[Tensor, Tensor, int, int]:
    a, b = _overlap_raster("a", a), _overlap_raster("b", b)
    ra, rb = _check_count("num_a", num_a), _check_count("num_b", num_b)
    if a.shape != b.shape:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must have one shape")
    big_h, big_w = (int(v) for v in a.shape[1:])
    if big_h < 1 or big_w < 1:
        raise ValueError(f"the rasters must hold at least one pixel an image, got {big_h} x {big_w}")
    if big_h * big_w > MAX_OVERLAP_PIXELS:
        raise ValueError(f"rasters of {big_h} x {big_w} pixels have 2^31 pixels or more")
    if (ra + 1) * (rb + 1) > MAX_OVERLAP_TABLE:
        raise ValueError(f"a table of {ra + 1} x {rb + 1} entries exceeds the 2^25 entries of an overlap table")
    _lib.require_device(a, "a")
    if b.device != a.device:
        raise ValueError(f"a is on {a.device} but b on {b.device}")
    return a.contiguous(), b.contiguous(), ra, rb


def _overlap_dtype(t: Tensor) -> int:
    return _lib.ISC_U8 if t.dtype == torch.uint8 else _lib.ISC_I32


def _overlap_into(a: Tensor, b: Tensor, ra: int, rb: int, per_image: bool, accumulate: bool, table: Tensor) -> None:
    """isc_overlap_table of contiguous `a` and `b` into contiguous `table`, in launches of at most 65 535 images."""
    lib = _lib.load()
    big_h, big_w = (int(v) for v in a.shape[1:])
    for i in range(0, a.shape[0], MAX_OVERLAP_MAPS):
        n = min(MAX_OVERLAP_MAPS, a.shape[0] - i)
        part = table[i:i + n] if per_image else table
        with torch.cuda.device(a.device):
            st = lib.isc_overlap_table(a[i:i + n].data_ptr(), _overlap_dtype(a), b[i:i + n].data_ptr(), _overlap_dtype(b), n,
                                       big_h, big_w, ra, rb, int(per_image), int(accumulate or (i > 0 and not per_image)),
                                       part.data_ptr(), _lib.stream_handle(a.device))
        _lib.check(st, "isc_overlap_table")


def overlap_table(a: "Tensor | LabelMaps | Regions", b: "Tensor | LabelMaps | Regions", num_a: int, num_b: int, *,
                  per_image: bool = True, out: Tensor | None = None) -> Tensor:
    """How many pixels carry every pair of values in two aligned rasters (`isc_overlap_table`, include/imagescry_hip.h
    has the definition): int64 `[B, num_a + 1, num_b + 1]`, or `[num_a + 1, num_b + 1]` summed over the batch with
    `per_image=False`.  `a` and `b` are uint8 or int32 `[B, H, W]` of one shape on one device, each with its own dtype; a
    `LabelMaps` stands for its `labels`, a `Regions` for its `ids`.  Entry `[.., i, j]` counts the pixels whose value is
    `i` in `a` and `j` in `b`; a value outside `[0, num_a)` -- a negative id, an id beyond a truncated table,
    `UNLABELED`, an ignore index -- counts at the "none" index `num_a`, and likewise `num_b` for `b`.  Every pixel is
    counted once: a per-image table sums to `H * W`.

    `out=`: an int64 table of that shape on the device, to which the counts are ADDED -- the running total over a
    dataset (and a captured call with `out=` adds again on every replay).  Integer atomics throughout: the same bytes
    on every run, for an image wherever it stands in a batch; capturable; nothing synchronises with the host."""
    a, b, ra, rb = _check_overlap_pair(a, b, num_a, num_b)
    if not isinstance(per_image, bool):
        raise TypeError("per_image must be a bool")
    shape = (a.shape[0], ra + 1, rb + 1) if per_image else (ra + 1, rb + 1)
    if out is None:
        # an empty batch launches nothing, so nothing zeroes its table
        table = (torch.empty if a.shape[0] else torch.zeros)(shape, dtype=torch.int64, device=a.device)
    else:
        if not isinstance(out, Tensor):
            raise TypeError(f"out must be a torch.Tensor, got {type(out).__name__}")
        if out.dtype != torch.int64:
            raise TypeError(f"out must be int64, got {out.dtype}")
        if tuple(out.shape) != shape:
            raise ValueError(f"out must have shape {shape}, got {tuple(out.shape)}")
        if out.device != a.device:
            raise ValueError(f"a is on {a.device} but out on {out.device}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous: the counts are added to it in place")
        table = out
    _overlap_into(a, b, ra, rb, per_image, out is not None, table)
    return table


def confusion_matrix(pred: "Tensor | LabelMaps", target: Tensor, num_classes: int, *, out: Tensor | None = None) -> Tensor:
    """The class confusion matrix of a batch, int64 `[C + 1, C + 1]` with C = `num_classes`: entry `[i, j]` counts the
    pixels predicted as class `i` whose target is class `j` -- rows are the prediction, columns the target -- and row and
    column C hold the pixels without a class: `UNLABELED` predictions, an `ignore_index` (255, -100, ...) in the target.
    `overlap_table(pred, target, C, C, per_image=False, out=out)`; an int64 target (torch's usual dtype for label
    maps) is narrowed to int32 first, which keeps every value a label map holds.  `out=` adds to a running matrix: one
    per dataset, `SegmentationScores.from_confusion` at the end."""
    if isinstance(target, Tensor) and target.dtype == torch.int64:
        target = target.to(torch.int32)
    rows = _check_count("num_classes", num_classes)
    return overlap_table(pred, target, rows, rows, per_image=False, out=out)


def _ratio(num: Tensor, den: Tensor) -> Tensor:
    return num.to(torch.float64) / den.to(torch.float64)  # 0 / 0 is NaN


def _nan_mean(values: Tensor) -> Tensor:
    """The mean of the non-NaN entries of a float64 vector, NaN without any, in a FIXED order of additions: NaN reads
    as 0, the vector is padded with zeros to a power of two, and neighbours `v[2k] + v[2k + 1]` are added until one value
    is left, which is divided by the count.  A library reduction picks its order by device and size; this one gives the
    same bits everywhere."""
    valid = ~torch.isnan(values)
    v = torch.where(valid, values, torch.zeros_like(values))
    size = 1 << max(0, v.numel() - 1).bit_length()
    v = torch.cat([v, v.new_zeros(size - v.numel())])
    while v.numel() > 1:
        v = v[0::2] + v[1::2]
    return v[0] / valid.sum().to(torch.float64)


@dataclass(frozen=True)
class SegmentationScores:
    """The per-class counts of mmseg's `IoUMetric` from a confusion matrix T (rows the prediction, columns the target,
    index C "none"), int64 `[C]` each.  Pixels whose target is "none" are ignored entirely; an unlabeled prediction on a
    labeled pixel counts against the target's class.

    intersect:   `T[c, c]`
    pred_area:   the sum of `T[c, j]` over `j < C`
    target_area: the sum of `T[i, c]` over `i <= C`
    union:       `pred_area + target_area - intersect`"""

    intersect: Tensor
    pred_area: Tensor
    target_area: Tensor
    union: Tensor

    @classmethod
    def from_confusion(cls, table: Tensor) -> "SegmentationScores":
        """From an int64 `[C + 1, C + 1]` table of `confusion_matrix`, on the table's device, without a host read."""
        if not isinstance(table, Tensor):
            raise TypeError(f"table must be a torch.Tensor, got {type(table).__name__}")
        if table.dtype != torch.int64:
            raise TypeError(f"table must be int64, got {table.dtype}")
        if table.ndim != 2 or table.shape[0] != table.shape[1] or table.shape[0] < 2:
            raise ValueError(f"table must have shape [C + 1, C + 1] with C >= 1, got {tuple(table.shape)}")
        c = table.shape[0] - 1
        intersect = torch.diagonal(table)[:c].contiguous()
        pred_area = table[:c, :c].sum(dim=1)
        target_area = table[:, :c].sum(dim=0)
        return cls(intersect, pred_area, target_area, pred_area + target_area - intersect)

    def to(self, device: str | torch.device) -> "SegmentationScores":
        return SegmentationScores(*(t.to(device) for t in (self.intersect, self.pred_area, self.target_area, self.union)))

    def cpu(self) -> "SegmentationScores":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.intersect.device

    def __len__(self) -> int:
        return self.intersect.shape[0]

    def iou(self) -> Tensor:
        """float64 `[C]`, `intersect / union`; NaN for a class in neither prediction nor target."""
        return _ratio(self.intersect, self.union)

    def accuracy(self) -> Tensor:
        """float64 `[C]`, `intersect / target_area`; NaN for a class absent from the target."""
        return _ratio(self.intersect, self.target_area)

    def dice(self) -> Tensor:
        """float64 `[C]`, `2 * intersect / (pred_area + target_area)`; NaN where both are empty."""
        return _ratio(2 * self.intersect, self.pred_area + self.target_area)

    def miou(self) -> Tensor:
        """0-dim float64: the mean of `iou()` over the classes where it is not NaN (a fixed order of additions: the same
        bits on every device)."""
        return _nan_mean(self.iou())

    def macc(self) -> Tensor:
        """0-dim float64: the mean of `accuracy()` over the classes where it is not NaN."""
        return _nan_mean(self.accuracy())

    def aacc(self) -> Tensor:
        """0-dim float64: `intersect.sum() / target_area.sum()`, the share of labeled pixels predicted right."""
        return _ratio(self.intersect.sum(), self.target_area.sum())


@dataclass(frozen=True)
class RegionMatches:
    """What `match_regions` returns: for every region of `a` its best partner in `b` by IoU.

    best:  int32 `[B, num_a]`, the region of `b`, -1 for a region that overlaps none (or has no pixels)
    inter: int64 `[B, num_a]`, the pixels the two share
    union: int64 `[B, num_a]`, the pixels of either; the region's own area where `best` is -1
    best_b, inter_b, union_b: the same for every region of `b` against `a`, `[B, num_b]` (`both=True`), else None"""

    best: Tensor
    inter: Tensor
    union: Tensor
    best_b: Tensor | None = None
    inter_b: Tensor | None = None
    union_b: Tensor | None = None

    def to(self, device: str | torch.device) -> "RegionMatches":
        return RegionMatches(*(None if t is None else t.to(device)
                               for t in (self.best, self.inter, self.union, self.best_b, self.inter_b, self.union_b)))

    def cpu(self) -> "RegionMatches":
        return self.to("cpu")

    @property
    def device(self) -> torch.device:
        return self.best.device

    def __len__(self) -> int:
        return self.best.shape[0]

    def iou(self) -> Tensor:
        """float64 `[B, num_a]`, `inter / union`; NaN for a region without pixels.  Above 1/2 the match is mutual."""
        return _ratio(self.inter, self.union)

    def iou_b(self) -> Tensor:
        """float64 `[B, num_b]`, `inter_b / union_b` (`both=True`)."""
        if self.inter_b is None:
            raise ValueError("these matches were computed without both=True")
        return _ratio(self.inter_b, self.union_b)


def match_regions(a: "Tensor | LabelMaps | Regions", b: "Tensor | LabelMaps | Regions", num_a: int, num_b: int, *,
                  exclude_none: bool = False, both: bool = False) -> RegionMatches:
    """For every region of `a` the region of `b` it fits best: the largest IoU among the regions it shares a pixel with,
    compared exactly in integers, ties to the lower id (`isc_overlap_table` + `isc_overlap_best`, include/imagescry_hip.h
    has the definition).  `a`, `b`, `num_a`, `num_b` as in `overlap_table`, per image.  A region's area counts all of
    its pixels; with `exclude_none=True` only those that lie on some region of the other raster (pixels that are "none"
    on the other side are left out of both areas).  `both=True` also answers for every region of `b`.  Two regions with
    IoU above 1/2 are each other's unique best.  Runs in passes of images whose tables stay within 256 MiB; the number of
    launches depends on the shapes alone, and nothing synchronises with the host."""
    a, b, ra, rb = _check_overlap_pair(a, b, num_a, num_b)
    if not isinstance(exclude_none, bool) or not isinstance(both, bool):
        raise TypeError("exclude_none and both must be bools")
    device = a.device
    n_img = a.shape[0]
    step = max(1, min(OVERLAP_PASS_BYTES // ((ra + 1) * (rb + 1) * 8), MAX_OVERLAP_MAPS))  # images a pass
    tables = torch.empty((min(n_img, step), ra + 1, rb + 1), dtype=torch.int64, device=device)

    def outputs(rows: int) -> tuple[Tensor, Tensor, Tensor]:
        return (torch.empty((n_img, rows), dtype=torch.int32, device=device),
                torch.empty((n_img, rows), dtype=torch.int64, device=device),
                torch.empty((n_img, rows), dtype=torch.int64, device=device))

    found = [outputs(ra)] + ([outputs(rb)] if both else [])
    lib = _lib.load()
    for i in range(0, n_img, step):
        n = min(step, n_img - i)
        _overlap_into(a[i:i + n], b[i:i + n], ra, rb, True, False, tables[:n])
        for axis, (best, inter, union) in enumerate(found):
            with torch.cuda.device(device):
                st = lib.isc_overlap_best(tables.data_ptr(), n, ra, rb, axis, int(exclude_none), best[i:i + n].data_ptr(),
                                          inter[i:i + n].data_ptr(), union[i:i + n].data_ptr(), _lib.stream_handle(device))
            _lib.check(st, "isc_overlap_best")
    return RegionMatches(*found[0], *(found[1] if both else (None, None, None)))
