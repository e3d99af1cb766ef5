"""isc_region_cell_weights and isc_region_pool on the GPU against tests/region_pool_oracle.py (which
tests/test_region_pool_host.py checks on the CPU): the weights exactly, vectors and mass bit for bit in both modes.  The
kernels are called through the C ABI into the interior of buffers filled with a pattern, whose guard bytes must survive;
the Python layer follows.  The shapes aim at the borders of the weights kernel's tile (`isc_region_pool_geometry`) and at
the sizes where the pooling kernel's loops turn over: 16 staged cells, 256 cells a scan, 256 dimensions a block, 1024
sums kept for the norm."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import region_pool_oracle as po  # noqa: E402

from imagescry_amd import (  # noqa: E402
    EmbeddingBatch,
    RegionVectors,
    _lib,
    label_regions,
    pool_regions,
    region_cell_weights,
    segmentation,
)

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes on either side of an output
FILL = 0xA5  # int64 0xA5A5.. is negative, float32 0xA5A5A5A5 is -2.87e-16: wrong wherever it survives
TILE = (64, 16)  # isc_region_pool_geometry, needed before a library can be asked (test ids); test_geometry checks it
TW, TH = TILE


class Guarded:
    """`nbytes` inside a uint8 buffer of FILL."""

    def __init__(self, nbytes: int, dtype: type, device: torch.device) -> None:
        self.lo, self.hi = GUARD, GUARD + nbytes
        self.buf = torch.full((self.hi + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.dtype = dtype
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.lo

    def numpy(self, shape: tuple[int, ...]) -> np.ndarray:
        raw = self.buf.cpu().numpy()
        assert (raw[:self.lo] == FILL).all(), "bytes before the output were written"
        assert (raw[self.hi:] == FILL).all(), "bytes after the output were written"
        return raw[self.lo:self.hi].copy().view(self.dtype).reshape(shape)


def run_weights(device: torch.device, ids: np.ndarray, grid: tuple[int, int], R: int) -> np.ndarray:
    b, H, W = ids.shape
    h, w = grid
    assert ids.flags["C_CONTIGUOUS"] and ids.dtype == np.int32
    idd = torch.from_numpy(ids).to(device)
    out = Guarded(b * R * h * w * 8, np.int64, device)
    st = _lib.load().isc_region_cell_weights(idd.data_ptr(), b, H, W, h, w, R, out.ptr, _lib.stream_handle(device))
    assert st == 0, _lib.strerror(st)
    torch.cuda.synchronize()
    assert np.array_equal(idd.cpu().numpy(), ids), "the input was written"
    return out.numpy((b, R, h * w))


def run_pool(device: torch.device, maps: np.ndarray, weights: np.ndarray, mode: int,
             with_mass: bool = True) -> tuple[np.ndarray, np.ndarray | None]:
    b, e, s = maps.shape
    r = weights.shape[1]
    assert maps.flags["C_CONTIGUOUS"] and weights.flags["C_CONTIGUOUS"]
    md, wd = torch.from_numpy(maps).to(device), torch.from_numpy(weights).to(device)
    out = Guarded(b * r * e * 4, np.float32, device)
    mass = Guarded(b * r * 8, np.int64, device) if with_mass else None
    st = _lib.load().isc_region_pool(md.data_ptr(), b, e, s, wd.data_ptr(), r, mode, out.ptr,
                                     mass.ptr if with_mass else None, _lib.stream_handle(device))
    assert st == 0, _lib.strerror(st)
    torch.cuda.synchronize()
    assert md.cpu().numpy().tobytes() == maps.tobytes() and np.array_equal(wd.cpu().numpy(), weights), "an input was written"
    return out.numpy((b, r, e)), mass.numpy((b, r)) if with_mass else None


def random_maps(seed: int, b: int, e: int, cells: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((b, e, cells)).astype(np.float32)


def check_case(device: torch.device, ids: np.ndarray, grid: tuple[int, int], R: int, maps: np.ndarray,
               modes: tuple[int, ...] = (po.UNIT, po.MEAN)) -> np.ndarray:
    """Weights against the oracle exactly, then the vectors pooled from the DEVICE's weights against the oracle's
    chains over the oracle's weights.  -> the weights."""
    want = po.cell_weights_ref(ids, grid, R)
    got = run_weights(device, ids, grid, R)
    assert np.array_equal(got, want), f"weights differ from the oracle at {int((got != want).sum())} places"
    for mode in modes:
        ref, ref_mass = po.pool_ref(maps, want, mode)
        out, mass = run_pool(device, maps, got, mode)
        assert np.array_equal(mass, ref_mass)
        assert po.same_floats(out, ref), f"mode {mode}: {int((out.view(np.uint32) != ref.view(np.uint32)).sum())} values differ"
    return want


def test_geometry() -> None:
    assert segmentation.region_pool_geometry() == TILE, "the maps below are aimed at TILE: change it with the kernel's tile"


# ----------------------------------------------------------------------------------------------------------------- shapes
def test_one_pixel_past_a_tile_and_both_kinds_of_skipped_pixel(device) -> None:
    rng = np.random.default_rng(1)
    R = 4
    ids = po.random_ids(rng, (2, TH + 1, TW + 1), R, blocks=4)
    assert ids.min() == -1 and ids.max() == R + 1
    wts = check_case(device, ids, (3, 5), R, random_maps(1, 2, 6, 15))
    area = np.stack([(ids == r).sum(axis=(1, 2)) for r in range(R)], axis=1)
    assert np.array_equal(wts.sum(axis=2), 4 * (TH + 1) * (TW + 1) * area)


def test_one_region_over_every_tile(device) -> None:
    H, W = 2 * TH, 3 * TW
    ids = np.zeros((2, H, W), np.int32)
    wts = check_case(device, ids, (2, 2), 1, random_maps(2, 2, 5, 4))
    assert (wts.sum(axis=2) == 4 * (H * W) ** 2).all() and (wts == (H * W) ** 2).all()  # every tile on the same four cells


def test_checkerboard_of_two_regions(device) -> None:
    H, W = 33, 70
    ids = ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2).astype(np.int32)[None]
    check_case(device, ids, (4, 9), 2, random_maps(3, 1, 3, 36))


def test_every_pixel_its_own_region(device) -> None:
    """4 keys a pixel, 1024 pixels a tile: more keys than the tile's table holds, so some go to memory directly."""
    H, W = TH, TW + 3
    ids = np.arange(H * W, dtype=np.int32).reshape(1, H, W)
    check_case(device, ids, (7, 5), H * W, random_maps(4, 1, 2, 35))


def test_identity_grid(device) -> None:
    rng = np.random.default_rng(5)
    ids = rng.integers(-1, 4, size=(2, 7, 5)).astype(np.int32)
    wts = check_case(device, ids, (7, 5), 3, random_maps(5, 2, 9, 35))
    onehot = np.stack([(ids == r).reshape(2, 35) for r in range(3)], axis=1)
    assert np.array_equal(wts, 4 * 35 * onehot)  # each pixel puts 4HW on its own cell only


def test_downsampling_leaves_cells_without_weight(device) -> None:
    ids = np.zeros((1, 3, 5), np.int32)
    ids[0, 1] = 1
    wts = check_case(device, ids, (7, 4), 2, random_maps(6, 1, 4, 28))
    assert ((wts[0, 0] == 0) & (wts[0, 1] == 0)).any()


SMALL = {"one cell": ((9, 11), (1, 1), 3), "one pixel row": ((1, TW + 9), (3, 4), 3), "one pixel column": ((TH + 9, 1), (4, 3), 3),
         "one region": ((19, 23), (3, 4), 1)}


@pytest.mark.parametrize("name", list(SMALL))
def test_degenerate_axes(device, name: str) -> None:
    size, grid, R = SMALL[name]
    ids = po.random_ids(np.random.default_rng(len(name)), (2, *size), R, blocks=3)
    check_case(device, ids, grid, R, random_maps(7, 2, 5, grid[0] * grid[1]))


def test_a_long_table_with_three_regions_present(device) -> None:
    R = 1024
    ids = np.full((1, 20, 30), -1, np.int32)
    ids[0, :10, :10], ids[0, 5:, 15:], ids[0, 15:, :8] = 0, 517, 1023
    wts = check_case(device, ids, (3, 4), R, random_maps(8, 1, 7, 12))
    assert sorted(np.nonzero(wts.sum(axis=2)[0])[0].tolist()) == [0, 517, 1023]


@functools.lru_cache(maxsize=None)
def dims_case() -> tuple[np.ndarray, np.ndarray]:
    ids = po.random_ids(np.random.default_rng(11), (1, 20, 30), 3, blocks=3)
    return ids, po.cell_weights_ref(ids, (2, 3), 3)


# 1 .. 130: the issue's; 256 / 257: a block of dimensions and one more; 1024 / 1025: the sums kept for the norm and one
# more, where the rows are summed a second time
@pytest.mark.parametrize("E", [1, 3, 64, 65, 130, 256, 257, 1024, 1025])
def test_embedding_dimensions(device, E: int) -> None:
    ids, wts = dims_case()
    maps = random_maps(E, 1, E, 6)
    for mode in (po.UNIT, po.MEAN):
        ref, ref_mass = po.pool_ref(maps, wts, mode)
        out, mass = run_pool(device, maps, wts, mode, with_mass=mode == po.UNIT)  # a NULL mass is accepted
        assert po.same_floats(out, ref) and (mass is None or np.array_equal(mass, ref_mass))


def test_more_cells_than_a_scan_and_than_a_stage(device) -> None:
    """18 x 16 = 288 cells: two scans of the weight row; region 0 has weight on far more than 16 cells."""
    ids = np.zeros((1, 20, 20), np.int32)
    ids[0, 12:, 9:] = 1
    wts = check_case(device, ids, (18, 16), 2, random_maps(12, 1, 5, 288))
    assert (wts[0, 0] != 0).sum() > 200 and (wts[0, 0, 256:] != 0).any()


@pytest.mark.parametrize("axis", ["rows", "columns"])
def test_taps_beyond_32_bits(device, axis: str) -> None:
    """(2L - 1) * l > 2^31: the taps are computed in 64 bits."""
    L, l = 1 << 15, 1 << 16
    ids = (np.arange(L) % 5 != 0).astype(np.int32).reshape((1, L, 1) if axis == "rows" else (1, 1, L)) - 1  # -1 or 0
    grid = (l, 1) if axis == "rows" else (1, l)
    want = po.cell_weights_ref(ids, grid, 1)
    got = run_weights(device, ids, grid, 1)
    assert np.array_equal(got, want)
    if axis == "rows":
        maps = random_maps(13, 1, 1, l)
        ref, ref_mass = po.pool_ref(maps, want, po.MEAN)
        out, mass = run_pool(device, maps, got, po.MEAN)
        assert po.same_floats(out, ref) and np.array_equal(mass, ref_mass)


# ----------------------------------------------------------------------------------------------------------------- values
def test_non_finite_cells_stay_inside_their_support(device) -> None:
    ids = np.array([[[0, 0, 1], [2, 2, 1]]], np.int32)  # on the grid itself: region r sees exactly its own cells
    for bad in (np.nan, np.inf, -np.inf):
        maps = random_maps(14, 1, 4, 6)
        maps[0, 2, 2] = bad  # a cell of region 1
        wts = po.cell_weights_ref(ids, (2, 3), 4)
        for mode in (po.UNIT, po.MEAN):
            ref, _ = po.pool_ref(maps, wts, mode)
            out, mass = run_pool(device, maps, run_weights(device, ids, (2, 3), 4), mode)
            assert po.same_floats(out, ref)
            assert np.isfinite(out[0, 0]).all() and np.isfinite(out[0, 2]).all() and not np.isfinite(out[0, 1]).all()
            assert mass[0].tolist() == [48, 48, 48, 0] and (out[0, 3] == 0).all()  # the empty row: zeros, mass 0
    assert not np.isfinite(ref[0, 1, 2])


def test_opposite_cells_give_a_zero_row_without_nan(device) -> None:
    ids = np.array([[[0, 0, 1]]], np.int32)
    maps = np.array([[[1.5, -1.5, 2.0], [-0.25, 0.25, 1.0]]], np.float32)
    wts = run_weights(device, ids, (1, 3), 2)
    out, mass = run_pool(device, maps, wts, po.UNIT)
    assert po.same_floats(out, po.pool_ref(maps, wts, po.UNIT)[0])
    assert mass[0, 0] == 24 and out[0, 0].tolist() == [0.0, 0.0] and np.isfinite(out).all()
    assert np.allclose(np.linalg.norm(out[0, 1].astype(np.float64)), 1.0, atol=1e-7)


# ------------------------------------------------------------------------------------------------- invariance and random
def test_an_image_gets_its_bits_wherever_it_stands(device) -> None:
    rng = np.random.default_rng(15)
    R, grid = 5, (4, 6)
    ids = po.random_ids(rng, (3, TH + 7, TW + 20), R, blocks=4)
    maps = random_maps(15, 3, 33, 24)
    assert not np.array_equal(ids[0], ids[1]) and not np.array_equal(ids[1], ids[2])
    wts = check_case(device, ids, grid, R, maps)
    full = {mode: run_pool(device, maps, wts, mode) for mode in (po.UNIT, po.MEAN)}
    for order in ([2], [1, 0], [2, 0, 1]):
        got = run_weights(device, ids[order], grid, R)
        assert np.array_equal(got, wts[order])
        for mode, (out, mass) in full.items():
            o, m = run_pool(device, maps[order], got, mode)
            assert o.tobytes() == out[order].tobytes() and np.array_equal(m, mass[order])
    # ... and whatever the length of the table: R = 3 gives the first three rows of R = 5
    short = run_weights(device, ids, grid, 3)
    assert np.array_equal(short, wts[:, :3])
    assert run_pool(device, maps, short, po.UNIT)[0].tobytes() == np.ascontiguousarray(full[po.UNIT][0][:, :3]).tobytes()


@pytest.mark.parametrize("seed", range(20))
def test_random_cases(device, seed: int) -> None:
    rng = np.random.default_rng(100 + seed)
    H, W = int(rng.integers(1, 81)), int(rng.integers(1, 151))
    h, w = int(rng.integers(1, 10)), int(rng.integers(1, 12))
    R, E, b = int(rng.integers(1, 13)), int(rng.integers(1, 71)), int(rng.integers(1, 3))
    ids = po.random_ids(rng, (b, H, W), R, blocks=int(rng.integers(1, 7)))
    check_case(device, ids, (h, w), R, random_maps(seed, b, E, h * w))


# ------------------------------------------------------------------------------------------------------ the Python layer
@functools.lru_cache(maxsize=None)
def pipeline_case() -> tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(21)
    return torch.randn((3, 5, 6, 3), generator=g), torch.randn((3, 40, 5, 6), generator=g)


def test_python_layer(device, monkeypatch) -> None:
    scores, maps = (t.to(device) for t in pipeline_case())
    labels = segmentation.label_map(scores, (45, 70), min_score=-0.3)
    labels = segmentation.LabelMaps(labels.labels, labels.scores, indices=torch.tensor([9, 4, 6]))
    regions = label_regions(labels, min_area=6, max_regions=24)
    ids = regions.ids.cpu().numpy()
    assert (ids == -1).any() and 3 < int(regions.num.min()) and int(regions.num.max()) <= 24
    wts = po.cell_weights_ref(ids, (5, 6), 24)
    m = maps.cpu().numpy().reshape(3, 40, 30)

    got = regions.embed(maps, return_weights=True)
    assert isinstance(got, RegionVectors) and got.device == device and len(got) == 3
    assert got.label is regions.label and got.num is regions.num and got.indices.tolist() == [9, 4, 6]
    assert got.weights.shape == (3, 24, 5, 6) and np.array_equal(got.weights.cpu().numpy().reshape(3, 24, 30), wts)
    ref, ref_mass = po.pool_ref(m, wts, po.UNIT)
    assert po.same_floats(got.vectors.cpu().numpy(), ref) and np.array_equal(got.mass.cpu().numpy(), ref_mass)
    assert np.array_equal(got.mass.cpu().numpy(), 4 * 45 * 70 * regions.area.cpu().numpy())
    assert torch.equal(got.valid().cpu(), torch.arange(24)[None, :] < regions.num.cpu()[:, None])
    assert torch.equal(region_cell_weights(regions.ids, 24, (5, 6)), got.weights)

    vec, image, region = got.flat()  # exactly the valid rows, image major
    valid = got.valid().cpu().numpy()
    where = np.argwhere(valid)
    assert region.cpu().tolist() == where[:, 1].tolist() and image.cpu().tolist() == [[9, 4, 6][i] for i in where[:, 0]]
    assert torch.equal(vec, got.vectors[torch.from_numpy(valid).to(device)]) and vec.shape == (int(valid.sum()), 40)

    mean = pool_regions(EmbeddingBatch(indices=torch.arange(3, device=device), embeddings=maps), regions.ids, 24, normalize=False)
    assert mean.weights is None and mean.label is None and mean.indices is None
    assert po.same_floats(mean.vectors.cpu().numpy(), po.pool_ref(m, wts, po.MEAN)[0])
    assert pool_regions(maps, regions.ids, 24, normalize=False).flat()[1].tolist() == where[:, 0].tolist()

    # against the composition a torch user would write, in float64
    up = F.interpolate(maps.double(), size=(45, 70), mode="bilinear", align_corners=False)
    onehot = (regions.ids[:, None].long() == torch.arange(24, device=device)[None, :, None, None]).double()  # [B, R, H, W]
    sums = torch.einsum("brhw,behw->bre", onehot, up)
    area = onehot.sum(dim=(2, 3)).clamp(min=1)[..., None]
    for ours, theirs in ((mean.vectors, sums / area), (got.vectors, sums / sums.norm(dim=2, keepdim=True).clamp(min=1e-300))):
        scale = theirs.abs().amax(dim=2, keepdim=True)
        assert bool(((ours.double() - theirs).abs() <= 1e-6 * scale).all())

    again = regions.embed(maps, return_weights=True)  # two calls, the same bits
    assert torch.equal(again.vectors.view(torch.int32), got.vectors.view(torch.int32)) and torch.equal(again.mass, got.mass)

    # two passes (a budget that holds one image's weights, and the last pass a single image) equal one
    monkeypatch.setattr(segmentation, "POOL_PASS_BYTES", 2 * 24 * 30 * 8)
    split = regions.embed(maps, return_weights=True)
    for a, c in ((split.vectors.view(torch.int32), got.vectors.view(torch.int32)), (split.mass, got.mass), (split.weights, got.weights)):
        assert torch.equal(a, c)
    monkeypatch.setattr(segmentation, "POOL_PASS_BYTES", 1)  # an image a pass at the least
    assert torch.equal(regions.embed(maps).vectors.view(torch.int32), got.vectors.view(torch.int32))
    monkeypatch.undo()

    empty = pool_regions(maps[:0], regions.ids[:0], 24)
    assert empty.vectors.shape == (0, 24, 40) and empty.mass.shape == (0, 24) and empty.flat()[0].shape == (0, 40)
    with pytest.raises(ValueError, match="ids on"):
        pool_regions(maps, regions.ids.cpu(), 24)


def test_masked_mean_pooling_on_the_grid_itself(device) -> None:
    """H == h, W == w: plain masked mean pooling of the cells."""
    g = torch.Generator().manual_seed(22)
    maps = torch.randn((2, 17, 6, 7), generator=g)
    ids = torch.randint(-1, 3, (2, 6, 7), generator=g, dtype=torch.int32)
    out = pool_regions(maps.to(device), ids.to(device), 3, normalize=False)
    for b in range(2):
        for r in range(3):
            cells = maps[b][:, ids[b] == r].double()  # [E, n] in ascending cell order
            assert cells.shape[1] > 0
            want = cells.mean(dim=1)
            assert torch.allclose(out.vectors[b, r].cpu().double(), want, rtol=0, atol=1e-6 * float(want.abs().max()))
            assert int(out.mass[b, r]) == 4 * 42 * cells.shape[1]
