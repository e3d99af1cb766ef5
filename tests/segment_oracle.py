"""numpy restatement of isc_label_map and isc_map_class_scores (a helper, not a conftest).  include/imagescry_hip.h
states the arithmetic as a fixed sequence of operations; this file follows it step by step with correctly rounded
operations only, so the GPU tests ask for equality.  tests/test_segment_host.py makes it prove itself against
`F.interpolate(mode="bilinear", align_corners=False)` + `argmax` on the CPU.

FMAF.  numpy has no fused multiply-add.  The product of two float32 numbers is exact in float64 (48 significant bits);
adding the float32 addend in float64 rounds once, to 53 bits, and the cast to float32 rounds again.  The two roundings
give the one rounding of `fmaf` unless the float64 sum sits exactly half-way between two neighbouring float32 numbers:
the half-way points are float64 numbers and rounding is monotone, so the exact value and its float64 rounding lie on the
same side of every half-way point the float64 rounding does not hit.  A float64 number s, |s| >= 2^-126, is such a point
iff the 29 mantissa bits float32 drops are 1 0 ... 0.  Those elements (and the ones in float32's subnormal range, where
the dropped bits sit elsewhere) are redone as fractions and rounded with `round_fraction_f32` of
tests/preprocess_exact.py; `FALLBACKS` counts them.  Infinities and NaN need no care: float64 gives 0 * inf = NaN,
inf - inf = NaN and inf + x = inf as the fused operation does.

ORDER.  The best prompt is the first in (v descending, NaN last, lower c first): among the prompts that are numbers,
those equal to the largest, the lowest of them; prompt 0 when every prompt is NaN.  This is stated by masks and
`argmax` (which returns the first maximum), not by the kernel's running comparison.

A NaN is a NaN: the tests compare values with NaN == NaN (`same`), not NaN payloads or signs, which the operations that
produce one (0 * inf on the host, on the device) need not agree on.
"""

from __future__ import annotations

import sys
from fractions import Fraction
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import preprocess_exact as pe  # noqa: E402

F32 = np.float32
F64 = np.float64
UNLABELED = 255
FALLBACKS = {"fmaf": 0}

# (B, C, E, h, w, H, W); case i is seeded with 1234 + i
CASES = [(2, 7, 32, 5, 4, 37, 29), (1, 9, 64, 3, 3, 48, 48), (2, 21, 64, 14, 14, 224, 224), (1, 3, 16, 2, 2, 33, 17),
         (1, 150, 64, 7, 9, 112, 144)]


def fmaf(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """round_to_float32(a * b + c) with one rounding, elementwise on float32 arrays (module docstring)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), np.asarray(c, dtype=F32))
    with np.errstate(all="ignore"):
        s = np.ascontiguousarray(a.astype(F64) * b.astype(F64) + c.astype(F64))
        out = s.astype(F32)
    dropped = s.view(np.uint64) & np.uint64(0x1FFFFFFF)
    redo = np.isfinite(s) & (s != 0) & ((dropped == np.uint64(0x10000000)) | (np.abs(s) < 2.0**-126))
    for idx in zip(*np.nonzero(redo)):
        exact = Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx]))
        out[idx] = pe.round_fraction_f32(exact)
        FALLBACKS["fmaf"] += 1
    return out


def upsampled(scores: np.ndarray, size: tuple[int, int]) -> np.ndarray:
    """Steps 1 - 3: float32 [B, h, w, C] -> v float32 [B, H, W, C]."""
    assert scores.dtype == np.float32 and scores.ndim == 4
    _, h, w, _ = scores.shape
    big_h, big_w = size
    y0, y1, ly0, ly1 = pe.bilinear_taps(h, big_h, fused=True)
    x0, x1, lx0, lx1 = pe.bilinear_taps(w, big_w, fused=True)
    w00 = (ly0[:, None] * lx0[None, :])[None, :, :, None]
    w01 = (ly0[:, None] * lx1[None, :])[None, :, :, None]
    w10 = (ly1[:, None] * lx0[None, :])[None, :, :, None]
    w11 = (ly1[:, None] * lx1[None, :])[None, :, :, None]
    assert w00.dtype == np.float32
    s00 = scores[:, y0][:, :, x0]
    s01 = scores[:, y0][:, :, x1]
    s10 = scores[:, y1][:, :, x0]
    s11 = scores[:, y1][:, :, x1]
    with np.errstate(all="ignore"):
        v = w00 * s00
    assert v.dtype == np.float32
    return fmaf(w11, s11, fmaf(w10, s10, fmaf(w01, s01, v)))


def choose(v: np.ndarray, class_of: np.ndarray | None = None, min_score: float = -np.inf) -> dict[str, np.ndarray]:
    """Steps 4 - 7 on the upsampled values v float32 [B, H, W, C]."""
    assert v.dtype == np.float32 and v.ndim == 4
    b, _, _, c = v.shape
    classes = np.arange(c) if class_of is None else np.asarray(class_of, dtype=np.int64)
    assert classes.shape == (c,) and classes.min() >= 0 and classes.max() < UNLABELED
    number = ~np.isnan(v)
    top = np.where(number, v, -np.inf).max(axis=-1, keepdims=True)
    winners = number & (v == top)
    cstar = np.where(winners.any(axis=-1), winners.argmax(axis=-1), 0)
    best = np.take_along_axis(v, cstar[..., None], axis=-1)[..., 0]
    label = classes[cstar]
    rivals = number & (classes[None, None, None, :] != label[..., None])
    rival = np.where(rivals, v, -np.inf).max(axis=-1).astype(F32)
    with np.errstate(all="ignore"):
        margin = np.where(rivals.any(axis=-1), best - rival, F32(np.inf)).astype(F32)
        unlabeled = np.isnan(best) | (best < F32(min_score))
    labels = np.where(unlabeled, UNLABELED, label).astype(np.uint8)
    counts = np.stack([np.bincount(labels[i].ravel(), minlength=256) for i in range(b)]).astype(np.int32)
    assert best.dtype == np.float32 and margin.dtype == np.float32
    return {"labels": labels, "best": best, "margin": margin, "counts": counts}


def label_map_ref(scores: np.ndarray, size: tuple[int, int], class_of: np.ndarray | None = None,
                  min_score: float = -np.inf) -> dict[str, np.ndarray]:
    """Steps 1 - 7 -> labels uint8 [B, H, W], best and margin float32 [B, H, W], counts int32 [B, 256]."""
    return choose(upsampled(scores, size), class_of, min_score)


def class_scores_ref(maps: np.ndarray, vectors: np.ndarray) -> np.ndarray:
    """isc_map_class_scores: float32 [B, E, S] and [C, E] -> float32 [B, S, C].  A float32 product is exact in float64,
    so `acc + a * b` in float64 is the fused step of the kernel's chain."""
    assert maps.dtype == np.float32 and vectors.dtype == np.float32
    b, e, s = maps.shape
    c = vectors.shape[0]
    m, t = maps.astype(F64), vectors.astype(F64)
    acc = np.zeros((b, s, c), dtype=F64)
    norm = np.zeros((c,), dtype=F64)
    with np.errstate(all="ignore"):
        for i in range(e):
            acc = acc + m[:, i, :, None] * t[None, None, :, i]
            norm = norm + t[:, i] * t[:, i]
        return (acc / np.maximum(np.sqrt(norm), 1e-12)).astype(F32)


def same(got: np.ndarray, want: np.ndarray) -> bool:
    """Equal dtype, shape and values, a NaN equal to a NaN (module docstring)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    return bool(np.array_equal(got, want, equal_nan=True)) and bool(np.array_equal(np.signbit(got) & ~np.isnan(got),
                                                                                  np.signbit(want) & ~np.isnan(want)))


def case_inputs(i: int):
    """(maps [B, E, h, w], vectors [C, E], scores [B, h, w, C], size) of case i as numpy float32: unit-norm cells and
    vectors, the scores the float64 dot products rounded to float32."""
    import torch
    import torch.nn.functional as F

    b, c, e, h, w, big_h, big_w = CASES[i]
    g = torch.Generator().manual_seed(1234 + i)
    m = F.normalize(torch.randn(b, e, h, w, generator=g), dim=1)
    t = F.normalize(torch.randn(c, e, generator=g), dim=1)
    scores = torch.einsum("behw,ce->bhwc", m.double(), t.double()).float()
    return m.numpy(), t.numpy(), scores.contiguous().numpy(), (big_h, big_w)
