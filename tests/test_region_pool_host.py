"""tests/region_pool_oracle.py on the CPU: the integer weights against their own invariants and against torch's bilinear
upsampling in float64, the exact fma against its definition, and the argument errors of the Python layer, which are
raised before the library is asked."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import region_pool_oracle as po  # noqa: E402

from imagescry_amd import RegionVectors, _lib, pool_regions, region_cell_weights, segmentation  # noqa: E402

SHAPES = [(37, 53, 5, 7), (16, 16, 16, 16), (3, 5, 7, 4), (64, 48, 4, 3), (1, 9, 1, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_weights_sum_to_the_area_and_match_interpolate(shape) -> None:
    H, W, h, w = shape
    rng = np.random.default_rng(H * 1000 + W)
    R = 5
    ids = po.random_ids(rng, (2, H, W), R, blocks=3)
    wts = po.cell_weights_ref(ids, (h, w), R)
    area = np.stack([(ids == r).sum(axis=(1, 2)) for r in range(R)], axis=1)
    assert np.array_equal(wts.sum(axis=2), 4 * H * W * area)
    assert (wts >= 0).all()
    maps = torch.from_numpy(rng.standard_normal((2, 6, h, w)))
    up = F.interpolate(maps, size=(H, W), mode="bilinear", align_corners=False).numpy()  # float64
    for r in range(R):
        inside = (ids == r)[:, None]
        want = (up * inside).sum(axis=(2, 3))  # [B, E]
        got = np.einsum("bc,bec->be", wts[:, r] / (4.0 * H * W), maps.numpy().reshape(2, 6, h * w))
        scale = (np.abs(up) * inside).sum(axis=(2, 3))  # per image and dimension: the magnitudes this very sum adds up
        assert (np.abs(got - want) <= 1e-12 * scale).all(), (r, (np.abs(got - want) / (scale + 1e-300)).max())


def test_identity_grid_puts_each_pixel_on_its_own_cell() -> None:
    ids = np.arange(35, dtype=np.int32).reshape(1, 7, 5)
    wts = po.cell_weights_ref(ids, (7, 5), 35)
    assert np.array_equal(wts[0], 4 * 35 * np.eye(35, dtype=np.int64))


def test_skipped_pixels() -> None:
    ids = np.array([[[-1, 0, 1, 2, -7]]], np.int32)
    wts = po.cell_weights_ref(ids, (1, 5), 2)  # region 2 lies beyond the table
    assert np.array_equal(wts[0], [[0, 20, 0, 0, 0], [0, 0, 20, 0, 0]])


def test_fma_is_the_definition() -> None:
    rng = np.random.default_rng(3)
    for _ in range(300):
        a = float(rng.integers(1, 2**50))
        b = float(np.float32(rng.standard_normal() * 10.0 ** rng.integers(-30, 30)))
        c = float(rng.standard_normal() * 10.0 ** rng.integers(-10, 20))
        assert po.fma(a, b, c) == po.fma_fraction(a, b, c)
    # one rounding, where a * b + c makes two
    a, b, c = float(2**50 - 1), float(np.float32(1 + 2**-23)), -float(2**50)
    assert po.fma(a, b, c) == po.fma_fraction(a, b, c) != a * b + c
    assert po.fma(3.0, -2.0, 6.0) == 0.0 and not math.copysign(1, po.fma(3.0, -2.0, 6.0)) < 0
    assert math.isnan(po.fma(2.0, math.nan, 1.0)) and math.isnan(po.fma(math.inf, 1.0, -math.inf))
    assert po.fma(2.0, math.inf, 1.0) == math.inf and po.fma(1e308, 1e308, -math.inf) == -math.inf
    assert po.fma(1e308, 10.0, 0.0) == math.inf


def test_pool_ref_semantics() -> None:
    maps = np.array([[[1.0, np.nan, 2.0, -2.0], [0.5, 1.0, np.inf, 3.0]]], np.float32)  # [1, 2, 4]
    wts = np.array([[[3, 0, 0, 1], [0, 1, 0, 0], [0, 0, 5, 0], [0, 0, 0, 0], [0, 0, 0, 0]]], np.int64)
    wts[0, 4] = [0, 0, 7, 7]
    mean, mass = po.pool_ref(maps, wts, po.MEAN)
    assert mass.tolist() == [[4, 1, 5, 0, 14]]
    assert mean[0, 0].tolist() == [0.25, 1.125]  # the NaN and the inf lie outside its support
    assert math.isnan(mean[0, 1, 0]) and mean[0, 1, 1] == 1.0
    assert mean[0, 2].tolist() == [2.0, math.inf] and mean[0, 3].tolist() == [0.0, 0.0]
    unit, _ = po.pool_ref(maps, wts, po.UNIT)
    assert np.allclose(np.linalg.norm(unit[0, 0].astype(np.float64)), 1.0, atol=1e-7)
    assert unit[0, 2, 0] == 0.0 and math.isnan(unit[0, 2, 1])  # 10 / inf, inf / inf
    zero = np.array([[[1.0, -1.0]]], np.float32)
    out, m = po.pool_ref(zero, np.array([[[6, 6]]], np.int64), po.UNIT)
    assert m[0, 0] == 12 and out.tolist() == [[[0.0]]]  # n == 0: zeros, not NaN


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_argument_errors_come_before_the_library() -> None:
    maps = torch.zeros((2, 8, 3, 4))
    ids = torch.zeros((2, 30, 40), dtype=torch.int32)
    with pytest.raises(TypeError, match="torch.Tensor"):
        pool_regions(maps, [[0]], 4)
    with pytest.raises(TypeError, match="int32"):
        pool_regions(maps, ids.long(), 4)
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        pool_regions(maps, ids[0], 4)
    with pytest.raises(TypeError, match="float32"):
        pool_regions(maps.double(), ids, 4)
    with pytest.raises(ValueError, match=r"\[B, E, h, w\]"):
        pool_regions(maps[0], ids, 4)
    with pytest.raises(ValueError, match="2 images but ids 1"):
        pool_regions(maps, ids[:1], 4)
    with pytest.raises(TypeError, match="num_regions"):
        pool_regions(maps, ids, 4.0)
    with pytest.raises(ValueError, match="num_regions"):
        pool_regions(maps, ids, 0)
    with pytest.raises(TypeError, match="bools"):
        pool_regions(maps, ids, 4, normalize=1)
    with pytest.raises(ValueError, match="2\\^25"):
        pool_regions(maps, ids, 2**25 // 12 + 1)
    with pytest.raises(ValueError, match="2\\^24"):
        pool_regions(maps[:1], torch.empty((1, 4097, 4096), dtype=torch.int32), 4)  # never touched
    with pytest.raises(ValueError, match="must not be empty"):
        pool_regions(maps[:, :0], ids, 4)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        pool_regions(maps, ids, 4)
    with pytest.raises(TypeError, match="pair of ints"):
        region_cell_weights(ids, 4, 3)
    with pytest.raises(ValueError, match="at least 1 x 1"):
        region_cell_weights(ids, 4, (0, 3))
    with pytest.raises(TypeError, match="int32"):
        region_cell_weights(ids.to(torch.int16), 4, (3, 4))
    with pytest.raises(ValueError, match="2\\^25"):
        region_cell_weights(ids, 1024, (256, 256))
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        region_cell_weights(ids, 4, (3, 4))


def test_region_vectors_container() -> None:
    vectors = torch.arange(2 * 3 * 2, dtype=torch.float32).reshape(2, 3, 2)
    mass = torch.tensor([[4, 0, 8], [0, 0, 12]])
    rv = RegionVectors(vectors, mass)
    assert len(rv) == 2 and rv.device.type == "cpu" and rv.weights is None and rv.label is None
    assert rv.valid().tolist() == [[True, False, True], [False, False, True]]
    vec, image, region = rv.flat()
    assert image.tolist() == [0, 0, 1] and region.tolist() == [0, 2, 2] and image.dtype == region.dtype == torch.int64
    assert torch.equal(vec, torch.stack([vectors[0, 0], vectors[0, 2], vectors[1, 2]]))
    with_indices = RegionVectors(vectors, mass, indices=torch.tensor([70, 30]))
    assert with_indices.flat()[1].tolist() == [70, 70, 30]
    assert with_indices.cpu().indices.tolist() == [70, 30] and with_indices.to("cpu").mass is not None
    with pytest.raises(Exception):
        rv.mass = mass  # frozen
    assert segmentation.POOL_PASS_BYTES == 256 << 20
