"""Pixel label maps from dense patch scores (new; the counterpart of the reference's `geometry.py`, which turns a
polygon into a mask on the feature-map grid: this turns feature-map scores into a mask on the image grid).

`class_scores` scores every cell of an embedding map against C vectors (`isc_map_class_scores`), `label_map` upsamples
the scores bilinearly to the image and takes the arg max per pixel in one kernel (`isc_label_map`) without ever writing
the `[B, C, H, W]` tensor of `F.interpolate(scores, size).max(1)`, and `segment` runs the two back to back.  The
arithmetic is fixed (include/imagescry_hip.h): the answers are deterministic, bit for bit reproducible and capturable
into a graph.  The producers are a dense CLIP map with text embeddings (`CLIPEmbedder.segment`), a DINOv2 map with
`KMeans` centroids, and `EmbeddingBank.similarity_map` (`EmbeddingBank.label_map`).
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch
from torch import Tensor

from imagescry_amd import _lib
from imagescry_amd.data import EmbeddingBatch

__all__ = ["LabelMaps", "UNLABELED", "MAX_PROMPTS", "MAX_CLASSES", "class_scores", "label_map", "label_map_geometry",
           "segment"]

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
