"""The label-map oracle (tests/segment_oracle.py) proves itself on the CPU against torch's bilinear interpolation and
arg max, its `fmaf` against exact fractions, and the Python layer of `imagescry_amd.segmentation` refuses what it must
before the library is called.  No GPU.

Labels: the oracle and `F.interpolate` blend in different orders, each within about 6 * 2^-24 = 3.6e-7 of the real value
for |score| <= 1, so they must agree at every pixel whose top-2 gap in torch's values is at least 1e-5 (more than
four such errors, 1.5e-6), and at most 0.1 % of a case's pixels may fall under that gap."""

from __future__ import annotations

import dataclasses
import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import preprocess_exact as pe  # noqa: E402
import segment_oracle as so  # noqa: E402

from imagescry_amd import EmbeddingBatch, LabelMaps, _lib, segmentation  # noqa: E402

F32 = np.float32
GAP = 1e-5
MAX_LEFT_OUT = 1e-3


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("i", range(len(so.CASES)))
def test_oracle_labels_agree_with_torch(i: int) -> None:
    _, _, scores, size = so.case_inputs(i)
    ref = so.label_map_ref(scores, size)
    up = F.interpolate(torch.from_numpy(scores).permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False)
    top2 = up.topk(min(2, up.shape[1]), dim=1)
    gap = (top2.values[:, 0] - top2.values[:, 1]).numpy()
    clear = gap >= GAP
    left_out = 1.0 - clear.mean()
    diff = np.abs(so.upsampled(scores, size) - up.permute(0, 2, 3, 1).numpy()).max()
    print(f"case {i}: {100 * left_out:.3f} % of the pixels under the gap, max |oracle - torch| = {diff:.2e}")
    assert left_out <= MAX_LEFT_OUT
    assert np.array_equal(ref["labels"][clear], top2.indices[:, 0].numpy()[clear])
    assert diff <= 4 * 3.6e-7
    # best is the upsampled value of the chosen prompt; counts are the labels' histogram
    assert ref["labels"].max() < scores.shape[-1] and ref["counts"].sum() == scores.shape[0] * size[0] * size[1]
    assert np.abs(ref["best"] - up.max(dim=1).values.numpy()).max() <= 4 * 3.6e-7
    # the margin is the top-2 gap (every prompt its own class), to the same accuracy
    assert np.abs(ref["margin"] - gap).max() <= 8 * 3.6e-7 and (ref["margin"] >= 0).all()


def test_fmaf_is_one_rounding() -> None:
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 2, 4000)).astype(F32)
    got = so.fmaf(a, b, c)
    for k in range(0, 4000, 7):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        assert got[k] == pe.round_fraction_f32(exact)
    # a float64 sum that lands on a half-way point only by its own rounding: the two-rounding answer is wrong there
    a1 = F32(1 + 2.0**-12)
    c1 = F32(2.0**-60)
    before = so.FALLBACKS["fmaf"]
    got = so.fmaf(np.array([a1]), np.array([a1]), np.array([c1]))
    assert so.FALLBACKS["fmaf"] == before + 1
    naive = F32(np.float64(a1) * np.float64(a1) + np.float64(c1))
    assert naive == F32(1 + 2.0**-11) and got[0] == F32(1 + 2.0**-11 + 2.0**-23)
    # an exact tie goes to even; non-finite operands behave as the fused operation does
    assert so.fmaf(np.array([F32(1)]), np.array([F32(1)]), np.array([F32(2.0**-24)]))[0] == F32(1)
    inf = F32(np.inf)
    out = so.fmaf(np.array([F32(0), F32(1), F32(1)]), np.array([inf, inf, inf]), np.array([F32(1), -inf, F32(1)]))
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == inf
    # float32's subnormal range
    tiny = so.fmaf(np.array([F32(2.0**-75)]), np.array([F32(2.0**-75)]), np.array([F32(0)]))
    assert tiny[0] == F32(0) and so.fmaf(np.array([F32(2.0**-75)]), np.array([F32(2.0**-74)]), np.array([F32(0)]))[0] == F32(2.0**-149)


def test_the_fallback_is_taken_inside_a_label_map() -> None:
    """A 1 x 2 grid upsampled to 1 x 4: pixel 1 blends 0.75 * 4 + 0.25 * 2^-21 = 3 + 2^-23, half-way between 3 and its
    float32 successor; the tie goes to the even 3."""
    scores = np.array([F32(4), F32(2.0**-21)], dtype=F32).reshape(1, 1, 2, 1)
    before = so.FALLBACKS["fmaf"]
    ref = so.label_map_ref(scores, (1, 4))
    assert so.FALLBACKS["fmaf"] > before
    assert ref["best"][0, 0, 1] == F32(3) and ref["labels"].tolist() == [[[0, 0, 0, 0]]]
    assert np.isinf(ref["margin"]).all() and ref["counts"][0, 0] == 4


def test_oracle_order_classes_threshold() -> None:
    nan, inf = F32(np.nan), F32(np.inf)
    # steps 4 - 7 on given values (in a blend a zero weight would turn the infinities into NaN)
    s = np.array([[3, 3, 1, 2], [nan, 5, 5, nan], [nan, nan, nan, nan], [-inf, nan, -inf, 1], [nan, -inf, -inf, nan]],
                 dtype=F32).reshape(1, 1, 5, 4)
    ref = so.choose(s)
    assert ref["labels"][0, 0].tolist() == [0, 1, 255, 3, 1]  # ties to the lower prompt, NaN last, all NaN unlabeled
    assert so.same(ref["best"][0, 0], np.array([3, 5, nan, 1, -inf], dtype=F32))
    assert so.same(ref["margin"][0, 0], np.array([0, 0, inf, inf, nan], dtype=F32))
    assert ref["counts"][0, [0, 1, 3, 255]].tolist() == [1, 2, 1, 1]
    # prompts 0 and 1 are one class: the margin looks past the twin
    ref = so.choose(s, class_of=np.array([7, 7, 2, 2]))
    assert ref["labels"][0, 0].tolist() == [7, 7, 255, 2, 7]
    assert so.same(ref["margin"][0, 0], np.array([1, 0, inf, inf, nan], dtype=F32))
    # the threshold is `<`: a pixel whose best equals min_score stays labeled
    ref = so.choose(s, min_score=3.0)
    assert ref["labels"][0, 0].tolist() == [0, 1, 255, 255, 255]


def test_class_scores_oracle_against_float64_einsum() -> None:
    m, t, scores, _ = so.case_inputs(0)
    b, e, h, w = m.shape
    got = so.class_scores_ref(m.reshape(b, e, h * w), t).reshape(b, h, w, -1)
    assert np.abs(got - scores).max() <= 2.0**-22  # unit vectors: the norm division moves the last bits only
    zero = so.class_scores_ref(m.reshape(b, e, h * w), np.zeros_like(t))
    assert (zero == 0).all()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_label_maps_container() -> None:
    lm = LabelMaps(labels=torch.zeros(2, 3, 4, dtype=torch.uint8), scores=torch.zeros(2, 3, 4))
    assert len(lm) == 2 and lm.device.type == "cpu" and lm.margins is None and lm.counts is None and lm.indices is None
    moved = lm.cpu()
    assert isinstance(moved, LabelMaps) and moved.margins is None and torch.equal(moved.labels, lm.labels)
    assert lm.to("cpu").scores.shape == (2, 3, 4)
    with pytest.raises(dataclasses.FrozenInstanceError):
        lm.labels = lm.labels  # type: ignore[misc]
    assert segmentation.UNLABELED == 255


def test_label_map_validation() -> None:
    s = torch.zeros(1, 2, 2, 3)
    for bad, exc in ((s.double(), TypeError), (s.numpy(), TypeError), (s[0], ValueError),
                     (torch.zeros(1, 2, 2, 0), ValueError), (torch.zeros(1, 2, 2, 1025), ValueError),
                     (torch.zeros(1, 0, 2, 3), ValueError)):
        with pytest.raises(exc):
            segmentation.label_map(bad, (4, 4))
    for size, exc in (((4,), TypeError), ((4.0, 4), TypeError), ("44", TypeError), ((0, 4), ValueError),
                      ((4, -1), ValueError), ((65536, 32768), ValueError), (4, TypeError)):
        with pytest.raises(exc):
            segmentation.label_map(s, size)
    with pytest.raises(ValueError, match="layout"):
        segmentation.label_map(s, (4, 4), layout="hwc")
    for class_of, exc in (([0, 1], ValueError), ([0, 1, 255], ValueError), ([0, -1, 2], ValueError),
                          (torch.zeros(3), TypeError), ([0.0, 1.0, 2.0], TypeError), ("abc", TypeError),
                          (torch.zeros(3, 1, dtype=torch.int64), ValueError)):
        with pytest.raises(exc):
            segmentation.label_map(s, (4, 4), class_of=class_of)
    with pytest.raises(ValueError, match="without class_of"):
        segmentation.label_map(torch.zeros(1, 2, 2, 256), (4, 4))
    with pytest.raises(ValueError, match="NaN"):
        segmentation.label_map(s, (4, 4), min_score=math.nan)
    with pytest.raises(TypeError):
        segmentation.label_map(s, (4, 4), min_score="0")
    # everything valid but the device: there is no CPU path
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        segmentation.label_map(s, (4, 4), class_of=[0, 0, 254], min_score=0.5)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        segmentation.label_map(torch.zeros(1, 3, 2, 2), (4, 4), layout="bchw")


def test_class_scores_and_segment_validation() -> None:
    m, t = torch.zeros(2, 8, 3, 3), torch.zeros(5, 8)
    for maps, vectors, exc in ((m.half(), t, TypeError), (m, t.double(), TypeError), (m[0], t, ValueError),
                               (m, t[0], ValueError), (m, torch.zeros(5, 7), ValueError), (m, t[:0], ValueError),
                               (m.numpy(), t, TypeError)):
        with pytest.raises(exc):
            segmentation.class_scores(maps, vectors)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        segmentation.class_scores(EmbeddingBatch(indices=torch.arange(2), embeddings=m), t)
    with pytest.raises(TypeError, match="layout"):
        segmentation.segment(m, t, (4, 4), layout="bchw")
    with pytest.raises(ValueError):
        segmentation.segment(m, t, (0, 4))


def test_clip_embedder_refuses_segment_without_a_dense_map() -> None:
    from imagescry_amd import CLIPEmbedder, ImageBatch

    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
    import clip_oracle as co

    cfg, sd = co.shallow("ViT-B/32")
    batch = ImageBatch(indices=torch.arange(1), images=torch.zeros(1, 3, 32, 32, dtype=torch.uint8))
    q = torch.zeros(2, cfg.embed_dim)
    with pytest.raises(ValueError, match="dense"):
        CLIPEmbedder(cfg, state_dict=sd).segment(batch, q)
    with pytest.raises(ValueError, match="checkpoint"):
        CLIPEmbedder(cfg, state_dict=sd, output="patches", dense="kk", preprocess="checkpoint").segment(batch, q)
