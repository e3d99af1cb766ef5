"""isc_overlap_table and isc_overlap_best on the GPU against their definitions (tests/overlap_oracle.py), value for value.
The shapes sit on the seams that isc_overlap_geometry and isc_overlap_best_geometry report; tables and outputs start as
garbage wherever the call has to initialise them itself."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import overlap_oracle as ov
from imagescry_amd import (LabelMaps, SegmentationScores, _lib, confusion_matrix, label_regions, match_regions,
                           overlap_table, rasterize_polygons, segmentation)

pytestmark = pytest.mark.gpu

CODES = {np.dtype(np.uint8): _lib.ISC_U8, np.dtype(np.int32): _lib.ISC_I32}
DTYPES = [(np.uint8, np.uint8), (np.uint8, np.int32), (np.int32, np.uint8), (np.int32, np.int32)]


def garbage(device: torch.device, shape: tuple[int, ...], dtype: torch.dtype, byte: int = 0x5A) -> torch.Tensor:
    count = int(np.prod(shape)) * dtype.itemsize
    return torch.full((count,), byte, dtype=torch.uint8, device=device).view(dtype).reshape(shape)


def run_table(device: torch.device, a: np.ndarray, b: np.ndarray, ra: int, rb: int, per_image: bool = True,
              into: torch.Tensor | None = None) -> torch.Tensor:
    """The C ABI itself on [B, H, W] rasters -> the table on the device; `into` turns accumulate on."""
    assert a.shape == b.shape and a.ndim == 3 and a.shape[0] >= 1
    n, h, w = a.shape
    shape = (n, ra + 1, rb + 1) if per_image else (ra + 1, rb + 1)
    table = garbage(device, shape, torch.int64) if into is None else into
    assert tuple(table.shape) == shape and table.dtype == torch.int64 and table.is_contiguous()
    dev_a = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    dev_b = torch.from_numpy(np.ascontiguousarray(b)).to(device)
    st = _lib.load().isc_overlap_table(dev_a.data_ptr(), CODES[a.dtype], dev_b.data_ptr(), CODES[b.dtype], n, h, w, ra, rb,
                                       int(per_image), int(into is not None), table.data_ptr(), _lib.stream_handle(device))
    assert st == _lib.ISC_OK
    torch.cuda.synchronize(device)
    return table


def run_best(device: torch.device, tables: np.ndarray, axis: int, exclude_none: bool) -> tuple[np.ndarray, ...]:
    """The C ABI itself on int64 [B, Ra + 1, Rb + 1] -> (best, inter, uni), whose buffers start as garbage."""
    n, ra, rb = tables.shape[0], tables.shape[1] - 1, tables.shape[2] - 1
    rows = ra if axis == 0 else rb
    dev = torch.from_numpy(np.ascontiguousarray(tables, dtype=np.int64)).to(device)
    best = garbage(device, (n, rows), torch.int32, 0xA5)
    inter, uni = garbage(device, (n, rows), torch.int64, 0xA5), garbage(device, (n, rows), torch.int64, 0xA5)
    st = _lib.load().isc_overlap_best(dev.data_ptr(), n, ra, rb, axis, int(exclude_none), best.data_ptr(), inter.data_ptr(),
                                      uni.data_ptr(), _lib.stream_handle(device))
    assert st == _lib.ISC_OK
    torch.cuda.synchronize(device)
    return best.cpu().numpy(), inter.cpu().numpy(), uni.cpu().numpy()


def same(got: np.ndarray, want: np.ndarray, what: str) -> None:
    assert got.dtype == want.dtype and got.shape == want.shape, what
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, (f"{what}: {len(wrong)} entries differ, the first at {wrong[0].tolist()}: got "
                             f"{got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}")


def check(device: torch.device, a: np.ndarray, b: np.ndarray, ra: int, rb: int, summed: bool = True) -> np.ndarray:
    """Both forms of the table against the oracle -> the per-image tables."""
    want = ov.table_ref(a, b, ra, rb)
    got = run_table(device, a, b, ra, rb).cpu().numpy()
    same(got, want, "per-image table")
    if summed:
        same(run_table(device, a, b, ra, rb, per_image=False).cpu().numpy(), want.sum(axis=0), "summed table")
    return got


def check_best(device: torch.device, tables: np.ndarray) -> None:
    for axis in (0, 1):
        for exclude_none in (False, True):
            got, want = run_best(device, tables, axis, exclude_none), ov.best_ref(tables, axis, exclude_none)
            for name, g, w in zip(("best", "inter", "uni"), got, want):
                same(g, w, f"{name} (axis {axis}, exclude_none {exclude_none})")


def with_none(rng: np.random.Generator, shape: tuple[int, ...], num: int, dtype: type) -> np.ndarray:
    """Values in [0, num) with both kinds of "none": below zero and at or above num (255 for uint8)."""
    v = rng.integers(0, num, shape).astype(np.int64)
    kind = rng.random(shape)
    if dtype is np.uint8:
        assert num <= 255
        v[kind < 0.1] = 255
        v[kind > 0.9] = min(num + 1, 255)
    else:
        v[kind < 0.1] = rng.integers(-5, 0, shape)[kind < 0.1]
        v[kind > 0.9] = num + rng.integers(0, 5, shape)[kind > 0.9]
        v[kind > 0.98] = np.iinfo(np.int32).max
        v[kind < 0.02] = np.iinfo(np.int32).min
    return v.astype(dtype)


def blocky(rng: np.random.Generator, shape: tuple[int, int, int], num: int, block: tuple[int, int], dtype: type,
           none: float) -> np.ndarray:
    """A raster of constant blocks -- runs along the rows -- with a share `none` of "none" pixels."""
    n, h, w = shape
    small = rng.integers(0, num, (n, -(-h // block[0]), -(-w // block[1])))
    v = np.kron(small, np.ones(block, dtype=np.int64))[:, :h, :w]
    out = rng.random(shape) < none
    v[out] = 255 if dtype is np.uint8 else -1
    if dtype is not np.uint8:
        v[out & (rng.random(shape) < 0.5)] = num + 3
    return (v % 256 if dtype is np.uint8 else v).astype(dtype)


@pytest.fixture(scope="module")
def geometry() -> tuple[int, int, int]:
    return segmentation.overlap_geometry()


@pytest.mark.parametrize("ta,tb", DTYPES)
def test_one_pixel_past_a_tile_with_both_kinds_of_none(device, geometry, ta: type, tb: type) -> None:
    tw, th, _ = geometry
    rng = np.random.default_rng(7)
    shape = (2, th + 1, tw + 1)
    a, b = with_none(rng, shape, 5, ta), with_none(rng, shape, 6, tb)
    got = check(device, a, b, 5, 6)
    assert got[:, 5, :].sum() > 0 and got[:, :, 6].sum() > 0 and (got.sum(axis=(1, 2)) == (th + 1) * (tw + 1)).all()


def test_one_pair_over_an_image_of_3_by_3_tiles(device, geometry) -> None:
    tw, th, _ = geometry
    shape = (1, 3 * th, 3 * tw)
    got = check(device, np.full(shape, 2, dtype=np.uint8), np.full(shape, 1, dtype=np.int32), 4, 3)
    assert got[0, 2, 1] == 9 * th * tw and np.count_nonzero(got) == 1


def test_stripes_end_runs_inside_a_wave_at_its_last_lane_and_at_tile_borders(device, geometry) -> None:
    tw, th, _ = geometry
    h, w = th + 3, 2 * tw + 2
    x = np.broadcast_to(np.arange(w), (2, h, w))
    a, b = (x % 7).astype(np.int32), ((x // 3) % 5).astype(np.uint8)
    check(device, a, b, 7, 5)
    check(device, np.ascontiguousarray(a.transpose(0, 2, 1)), np.ascontiguousarray(b.transpose(0, 2, 1)), 7, 5)
    # a run that ends at lane 63 exactly, and one that crosses the tile border
    b2 = (x // tw).astype(np.int32)
    check(device, (x // (tw + 1)).astype(np.int32), b2, 3, 3)


def test_every_pixel_its_own_pair_overflows_the_lds_table(device, geometry) -> None:
    tw, th, slots = geometry
    assert tw * th > slots  # more pairs in a tile than slots: some go to memory directly
    h, w = 2 * th, 2 * tw
    n = h * w
    assert (n + 1) ** 2 <= segmentation.MAX_OVERLAP_TABLE
    a = np.arange(n, dtype=np.int32).reshape(1, h, w)
    step = 1571
    assert np.gcd(step, n) == 1
    b = ((np.arange(n, dtype=np.int64) * step + 17) % n).astype(np.int32).reshape(1, h, w)
    got = check(device, a, b, n, n, summed=False)
    assert np.count_nonzero(got) == n and got.max() == 1


def test_noise_with_few_pairs_and_no_runs(device, geometry) -> None:
    tw, th, _ = geometry
    rng = np.random.default_rng(11)
    shape = (2, 2 * th + 5, tw + 9)
    check(device, rng.integers(0, 8, shape).astype(np.uint8), rng.integers(-1, 8, shape).astype(np.int32), 7, 7)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 150), (150, 1), (1, 64), (1, 65)])
def test_degenerate_axes(device, h: int, w: int) -> None:
    rng = np.random.default_rng(h * 1000 + w)
    a, b = with_none(rng, (2, h, w), 3, np.int32), with_none(rng, (2, h, w), 3, np.uint8)
    check(device, a, b, 3, 3)
    check(device, a, b, 1, 1)  # one region and "none" on both axes


def test_more_tiles_than_workgroups_an_image(device, geometry) -> None:
    """An image has at most 1024 workgroups; the rest of the tiles is strided over."""
    tw, th, _ = geometry
    rng = np.random.default_rng(3)
    for h, w in ((th * 1024 + 1, 1), (th * 700, tw + 1)):
        check(device, blocky(rng, (2, h, w), 6, (5, 2), np.uint8, 0.1), blocky(rng, (2, h, w), 9, (3, 1), np.int32, 0.1), 6, 9)


def test_summed_table_is_the_sum_of_the_per_image_tables(device, geometry) -> None:
    tw, th, _ = geometry
    rng = np.random.default_rng(5)
    shape = (3, th + 7, tw + 30)
    a, b = blocky(rng, shape, 9, (4, 6), np.uint8, 0.2), blocky(rng, shape, 12, (3, 9), np.int32, 0.2)
    per_image = run_table(device, a, b, 9, 12)
    summed = run_table(device, a, b, 9, 12, per_image=False)
    assert torch.equal(per_image.sum(dim=0), summed)
    same(summed.cpu().numpy(), ov.table_ref(a, b, 9, 12, per_image=False), "summed table")


def test_accumulate_adds_and_a_plain_call_starts_from_garbage(device, geometry) -> None:
    tw, th, _ = geometry
    rng = np.random.default_rng(6)
    shape = (2, th + 2, tw + 2)
    a, b = blocky(rng, shape, 5, (3, 5), np.int32, 0.1), blocky(rng, shape, 5, (2, 7), np.int32, 0.1)
    for per_image in (True, False):
        want = ov.table_ref(a, b, 5, 5, per_image=per_image)
        first = run_table(device, a, b, 5, 5, per_image=per_image)  # over 0x5A bytes
        same(first.cpu().numpy(), want, "from garbage")
        second = run_table(device, a, b, 5, 5, per_image=per_image, into=first)
        assert second.data_ptr() == first.data_ptr()
        same(second.cpu().numpy(), 2 * want, "accumulated")
        seeded = torch.full_like(first, 1000)
        same(run_table(device, a, b, 5, 5, per_image=per_image, into=seeded).cpu().numpy(), want + 1000, "onto 1000s")
    # the Python layer: out= accumulates, no out= does not
    da, db = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
    total = torch.zeros((6, 6), dtype=torch.int64, device=device)
    for _ in range(3):
        assert overlap_table(da, db, 5, 5, per_image=False, out=total) is total
    same(total.cpu().numpy(), 3 * ov.table_ref(a, b, 5, 5, per_image=False), "out=")
    same(overlap_table(da, db, 5, 5).cpu().numpy(), ov.table_ref(a, b, 5, 5), "no out=")


def test_an_image_gets_its_bits_wherever_it_stands(device, geometry) -> None:
    tw, th, _ = geometry
    rng = np.random.default_rng(8)
    shape = (5, 2 * th + 3, 2 * tw + 5)
    a, b = blocky(rng, shape, 30, (5, 9), np.int32, 0.1), blocky(rng, shape, 200, (2, 3), np.uint8, 0.1)
    a[4], b[4] = a[0], b[0]
    one = run_table(device, a, b, 30, 200).cpu().numpy()
    two = run_table(device, a, b, 30, 200).cpu().numpy()
    assert one.tobytes() == two.tobytes()
    assert one[0].tobytes() == one[4].tobytes()
    alone = run_table(device, a[:1], b[:1], 30, 200).cpu().numpy()
    assert alone[0].tobytes() == one[0].tobytes()
    same(one, ov.table_ref(a, b, 30, 200), "per-image table")


# ------------------------------------------------------------------------------------------------------------- best
def test_best_ties_go_to_the_lower_id_and_rows_without_overlap_say_so(device) -> None:
    t = np.zeros((2, 6, 6), dtype=np.int64)
    # image 0, row 0: columns 1 and 3 tie at 4 / (8 + 6 - 4); row 1 overlaps nothing but "none"; row 4 is empty
    t[0, 0, 1] = t[0, 0, 3] = 4
    t[0, 3, 1] = t[0, 2, 3] = 2
    t[0, 1, 5] = 9
    # image 1: ties between DIFFERENT pairs -- row 0: 2 / 6 in column 0 and 1 / 3 in column 2; row 2: 1 / 3 in column 1
    # and 2 / 6 in column 3 -- go to the lower column whichever pair is larger
    t[1, 0, 0], t[1, 0, 2], t[1, 1, 0] = 2, 1, 3
    t[1, 2, 1], t[1, 2, 3], t[1, 3, 3] = 1, 2, 3
    t[1, 5, 5] = 7
    check_best(device, t)
    best, inter, uni = run_best(device, t, 0, False)
    assert best[0].tolist() == [1, -1, 3, 1, -1] and inter[0].tolist() == [4, 0, 2, 2, 0]
    assert uni[0].tolist() == [10, 9, 6, 6, 0]
    assert run_best(device, t, 0, True)[2][0].tolist() == [10, 0, 6, 6, 0]  # the "none" pixels of row 1 leave its area
    assert (best[1, 0], inter[1, 0], uni[1, 0]) == (0, 2, 6) and (best[1, 2], inter[1, 2], uni[1, 2]) == (1, 1, 3)


def last_unit_table(p: int, winner: int) -> np.ndarray:
    """[3, 3]: row 0 meets columns 0 and 1 with IoUs p / (3p - 1) and (p + 1) / (3p + 2), whose cross products differ by
    exactly 1 -- p (3p + 2) - (p + 1)(3p - 1) = 1 -- so the first is larger; `winner` is the column it stands in."""
    t = np.zeros((3, 3), dtype=np.int64)
    t[0, 0], t[0, 1] = p, p + 1
    t[1, 0], t[1, 1] = p - 2, p + 1
    assert p * (3 * p + 2) - (p + 1) * (3 * p - 1) == 1
    return t if winner == 0 else np.ascontiguousarray(t[:, [1, 0, 2]])


@pytest.mark.parametrize("p", [(1 << 30) - 5, (1 << 30) - 2, 7, 94906267])
def test_best_compares_in_exact_integers(device, p: int) -> None:
    """Every sum stays below 2^31 and every product below 2^63; a float64 sees the two IoUs as equal from p = 2^27 on
    and picks the lower column, a float32 long before."""
    tables = np.stack([last_unit_table(p, 0), last_unit_table(p, 1)])
    assert tables.sum(axis=1).max() < 1 << 31 and tables.sum(axis=2).max() < 1 << 31
    check_best(device, tables)
    best, inter, uni = run_best(device, tables, 0, False)
    assert best[:, 0].tolist() == [0, 1] and inter[:, 0].tolist() == [p, p] and uni[:, 0].tolist() == [3 * p - 1] * 2
    if p > 1 << 27:
        assert np.float64(p) / np.float64(3 * p - 1) == np.float64(p + 1) / np.float64(3 * p + 2)  # what a float sees
    # the transposed question on the transposed tables
    best_t = run_best(device, np.ascontiguousarray(tables.transpose(0, 2, 1)), 1, False)[0]
    assert best_t[:, 0].tolist() == [0, 1]


@pytest.mark.parametrize("extra", [0, 1, 1027])
def test_best_one_past_the_column_chunk(device, extra: int) -> None:
    """Ra + 1 = Rb + 1 = columns + 1 is one past the chunk with the "none" column counted; the tables above it put real
    columns into a second and third chunk, where the running best has to carry over."""
    columns = segmentation.overlap_best_geometry()
    r = columns + extra
    rng = np.random.default_rng(40 + extra)
    tables = np.zeros((2, r + 1, r + 1), dtype=np.int64)
    for k in range(2):
        at = rng.integers(0, r + 1, (5000, 2))
        tables[k, at[:, 0], at[:, 1]] = rng.integers(1, 50, 5000)
        tables[k, 3, :] = 0
        tables[k, 3, r - 1] = 5  # a row whose only partner is the last real column
        tables[k, 4, :] = 0
        tables[k, 4, [2, r - 2]] = 6, 6  # equal overlaps at both ends: the column sums decide
    check_best(device, tables)


# ----------------------------------------------------------------------------------------------------------- random
@pytest.mark.parametrize("seed", range(20))
def test_random_cases(device, seed: int) -> None:
    rng = np.random.default_rng(1000 + seed)
    ta, tb = DTYPES[seed % 4]
    n, h, w = int(rng.integers(1, 4)), int(rng.integers(1, 90)), int(rng.integers(1, 260))
    ra = int(rng.choice([1, 2, 5, 40, 255])) if ta is np.uint8 else int(rng.choice([1, 3, 17, 300, 2000]))
    rb = int(rng.choice([1, 2, 5, 40, 255])) if tb is np.uint8 else int(rng.choice([1, 3, 17, 300, 2000]))
    none = float(rng.choice([0.0, 0.05, 0.5, 1.0]))
    block = (int(rng.integers(1, 9)), int(rng.integers(1, 40)))
    a = blocky(rng, (n, h, w), ra, block, ta, none)
    b = blocky(rng, (n, h, w), rb, (int(rng.integers(1, 9)), int(rng.integers(1, 40))), tb, none / 2)
    per_image = bool(seed % 3)
    want = ov.table_ref(a, b, ra, rb, per_image=per_image)
    got = run_table(device, a, b, ra, rb, per_image=per_image).cpu().numpy()
    same(got, want, "table")
    if per_image:
        exclude_none = bool(seed & 1)
        for axis in (0, 1):
            for name, g, v in zip(("best", "inter", "uni"), run_best(device, got, axis, exclude_none),
                                  ov.best_ref(want, axis, exclude_none)):
                same(g, v, f"{name} (axis {axis})")


# ------------------------------------------------------------------------------------------------------ Python layer
@pytest.fixture(scope="module")
def label_pair(device) -> dict[str, object]:
    """A prediction with unlabeled pixels and a target with ignored ones, 6 classes, and their regions."""
    rng = np.random.default_rng(77)
    shape = (3, 50, 70)
    pred = blocky(rng, shape, 6, (7, 9), np.uint8, 0.1)
    target = np.where(rng.random(shape) < 0.7, pred, blocky(rng, shape, 6, (5, 11), np.uint8, 0.0)).astype(np.int64)
    target[rng.random(shape) < 0.05] = 255
    target[rng.random(shape) < 0.05] = -100
    return {"pred": pred, "target": target, "dev_pred": torch.from_numpy(pred).to(device),
            "dev_target": torch.from_numpy(target).to(device)}


def test_confusion_matrix_and_scores(device, label_pair) -> None:
    pred, target = label_pair["pred"], label_pair["target"]
    maps = LabelMaps(label_pair["dev_pred"])
    want = ov.table_ref(pred, target, 6, 6, per_image=False)
    for got in (confusion_matrix(maps, label_pair["dev_target"], 6), maps.confusion(label_pair["dev_target"], 6),
                confusion_matrix(label_pair["dev_pred"], label_pair["dev_target"].to(torch.int32), 6)):
        assert got.dtype == torch.int64 and got.device.type == "cuda"
        same(got.cpu().numpy(), want, "confusion matrix")
    running = torch.zeros((7, 7), dtype=torch.int64, device=device)
    for k in range(3):  # image by image into one table: a loader
        maps_k = LabelMaps(label_pair["dev_pred"][k:k + 1])
        assert maps_k.confusion(label_pair["dev_target"][k:k + 1], 6, out=running) is running
    same(running.cpu().numpy(), want, "running confusion matrix")
    scores = SegmentationScores.from_confusion(running)
    assert scores.device.type == "cuda"
    ref = ov.scores_ref(ov.mmseg_counts(pred, target, 6))
    for name in ("intersect", "pred_area", "target_area", "union"):
        same(getattr(scores, name).cpu().numpy(), ov.mmseg_counts(pred, target, 6)[name], name)
    for name, got in (("iou", scores.iou()), ("accuracy", scores.accuracy()), ("dice", scores.dice())):
        assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), ref[name], equal_nan=True), name
    for name, got in (("miou", scores.miou()), ("macc", scores.macc()), ("aacc", scores.aacc())):
        print(name, float(got), ref[name])
        assert got.dtype == torch.float64 and got.ndim == 0 and float(got) == ref[name], name  # float64 equality


def test_regions_and_label_maps_as_inputs(device, label_pair) -> None:
    maps = LabelMaps(label_pair["dev_pred"])
    regions = label_regions(maps, max_regions=64)
    ids = regions.ids.cpu().numpy()
    same(overlap_table(regions, maps, 64, 6).cpu().numpy(), ov.table_ref(ids, label_pair["pred"], 64, 6), "Regions x LabelMaps")
    # every region lies in one class: its row has one entry, in its label's column
    table = overlap_table(regions, maps, 64, 6).cpu().numpy()
    label, area = regions.label.cpu().numpy(), regions.area.cpu().numpy()
    for k in range(3):
        for r in range(min(int(regions.num[k]), 64)):
            assert table[k, r, label[k, r]] == area[k, r] == table[k, r].sum()


def test_match_regions(device, label_pair, monkeypatch) -> None:
    found = label_regions(LabelMaps(label_pair["dev_pred"]), max_regions=64)
    shifted = torch.from_numpy(np.roll(label_pair["pred"], 1, axis=1)).to(device)  # the same blocks a row lower
    other = label_regions(shifted, max_regions=40, connectivity=4)
    tables = ov.table_ref(found.ids.cpu().numpy(), other.ids.cpu().numpy(), 64, 40)

    def agrees(m: object, exclude_none: bool, both: bool) -> None:
        want = ov.best_ref(tables, 0, exclude_none)
        for name, g, v in zip(("best", "inter", "union"), (m.best, m.inter, m.union), want):
            same(g.cpu().numpy(), v, name)
        with np.errstate(invalid="ignore"):
            ref_iou = want[1].astype(np.float64) / want[2].astype(np.float64)
        assert m.iou().dtype == torch.float64 and np.array_equal(m.iou().cpu().numpy(), ref_iou, equal_nan=True)
        if not both:
            assert m.best_b is None and m.inter_b is None and m.union_b is None
            return
        for name, g, v in zip(("best_b", "inter_b", "union_b"), (m.best_b, m.inter_b, m.union_b),
                              ov.best_ref(tables, 1, exclude_none)):
            same(g.cpu().numpy(), v, name)
        assert m.iou_b().shape == (3, 40)

    agrees(match_regions(found, other, 64, 40), False, False)
    agrees(match_regions(found.ids, other.ids, 64, 40, exclude_none=True, both=True), True, True)
    agrees(found.match(other, both=True), False, True)
    agrees(found.match(other, exclude_none=True), True, False)
    # mutual best above IoU 1/2
    m = found.match(other, both=True)
    best, best_b = m.best.cpu().numpy(), m.best_b.cpu().numpy()
    strong = np.argwhere(2 * m.inter.cpu().numpy() > m.union.cpu().numpy())
    assert len(strong) > 0 and all(best_b[k, best[k, i]] == i for k, i in strong)
    # several passes equal one
    single = match_regions(found, other, 64, 40, both=True)
    monkeypatch.setattr(segmentation, "OVERLAP_PASS_BYTES", 65 * 41 * 8 * 2)  # two images a pass: 2 + 1
    split = match_regions(found, other, 64, 40, both=True)
    for name in ("best", "inter", "union", "best_b", "inter_b", "union_b"):
        assert torch.equal(getattr(single, name), getattr(split, name)), name
    monkeypatch.setattr(segmentation, "OVERLAP_PASS_BYTES", 1)  # an image a pass at the least
    assert torch.equal(match_regions(found, other, 64, 40).best, single.best)


def test_python_layer_on_empty_and_odd_inputs(device) -> None:
    none = torch.zeros((0, 4, 5), dtype=torch.uint8, device=device)
    assert overlap_table(none, none, 3, 2).shape == (0, 4, 3)
    assert torch.equal(overlap_table(none, none, 3, 2, per_image=False), torch.zeros((4, 3), dtype=torch.int64, device=device))
    m = match_regions(none, none, 3, 2, both=True)
    assert m.best.shape == (0, 3) and m.best_b.shape == (0, 2)
    # views that are not contiguous are made so
    rng = np.random.default_rng(9)
    a, b = with_none(rng, (2, 20, 33), 4, np.int32), with_none(rng, (2, 20, 33), 4, np.uint8)
    da, db = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
    same(overlap_table(da[:, ::2, 1:], db[:, ::2, 1:], 4, 4).cpu().numpy(), ov.table_ref(a[:, ::2, 1:], b[:, ::2, 1:], 4, 4),
         "strided views")


def test_refusals(device) -> None:
    u8 = torch.zeros((2, 4, 5), dtype=torch.uint8, device=device)
    i32 = torch.zeros((2, 4, 5), dtype=torch.int32, device=device)
    with pytest.raises(_lib.HipLibraryError):
        overlap_table(u8.cpu(), i32.cpu(), 3, 3)
    with pytest.raises(ValueError):
        overlap_table(u8, i32.cpu(), 3, 3)  # mixed devices
    with pytest.raises(ValueError):
        match_regions(u8, i32.cpu(), 3, 3)
    with pytest.raises(ValueError):
        overlap_table(u8, i32[:1], 3, 3)
    with pytest.raises(TypeError):
        overlap_table(u8, i32.to(torch.int64), 3, 3)
    with pytest.raises(TypeError):
        overlap_table(u8.to(torch.float32), i32, 3, 3)
    with pytest.raises(ValueError):
        overlap_table(u8, i32, 2**13, 2**12 - 1)
    with pytest.raises(TypeError):
        overlap_table(u8, i32, 3, 3, per_image=1)
    with pytest.raises(TypeError):
        match_regions(u8, i32, 3, 3, both=1)
    good = torch.zeros((2, 4, 4), dtype=torch.int64, device=device)
    with pytest.raises(TypeError):
        overlap_table(u8, i32, 3, 3, out=good.to(torch.int32))
    with pytest.raises(TypeError):
        overlap_table(u8, i32, 3, 3, out=good.cpu().numpy())
    with pytest.raises(ValueError):
        overlap_table(u8, i32, 3, 3, out=good[0])  # the shape of per_image=False
    with pytest.raises(ValueError):
        overlap_table(u8, i32, 3, 3, per_image=False, out=good)
    with pytest.raises(ValueError):
        overlap_table(u8, i32, 3, 3, out=good.cpu())
    with pytest.raises(ValueError):
        overlap_table(u8, i32, 3, 3, out=torch.zeros((2, 4, 8), dtype=torch.int64, device=device)[:, :, ::2])
    assert overlap_table(u8, i32, 3, 3, out=good) is good and int(good.sum()) == 40
    with pytest.raises(TypeError):
        label_regions(u8).match(i32)  # a raster has no row count: match_regions takes it


# ----------------------------------------------------------------------------------------------------------- capture
def test_graph_replay_after_the_rasters_are_refilled_in_place(device, geometry) -> None:
    tw, th, _ = geometry
    rng = np.random.default_rng(21)
    shape, ra, rb = (3, th + 9, tw + 21), 12, 9
    pairs = [(blocky(rng, shape, ra, (4, 7), np.int32, 0.1), blocky(rng, shape, rb, (6, 5), np.uint8, 0.1)) for _ in range(3)]
    want = [ov.table_ref(a, b, ra, rb) for a, b in pairs]
    want_best = [ov.best_ref(t, 0, False) for t in want]
    live_a, live_b = torch.from_numpy(pairs[0][0]).to(device), torch.from_numpy(pairs[0][1]).to(device)
    running = torch.zeros((ra + 1, rb + 1), dtype=torch.int64, device=device)
    best = torch.empty((3, ra), dtype=torch.int32, device=device)
    inter, uni = (torch.empty((3, ra), dtype=torch.int64, device=device) for _ in range(2))
    lib = _lib.load()

    def work() -> torch.Tensor:
        tables = overlap_table(live_a, live_b, ra, rb)
        st = lib.isc_overlap_best(tables.data_ptr(), 3, ra, rb, 0, 0, best.data_ptr(), inter.data_ptr(), uni.data_ptr(),
                                  _lib.stream_handle(device))
        assert st == _lib.ISC_OK
        overlap_table(live_a, live_b, ra, rb, per_image=False, out=running)
        return tables

    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        work()  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    torch.cuda.synchronize()
    running.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        tables = work()
    total = np.zeros((ra + 1, rb + 1), dtype=np.int64)
    for i in (1, 2, 0, 1):
        live_a.copy_(torch.from_numpy(pairs[i][0]))  # refilled in place
        live_b.copy_(torch.from_numpy(pairs[i][1]))
        for t in (tables, best, inter, uni):
            t.fill_(-9)  # garbage where the graph has to start over
        graph.replay()
        torch.cuda.synchronize()
        total += want[i].sum(axis=0)
        same(tables.cpu().numpy(), want[i], f"replay on pair {i}: tables")
        for name, g, v in zip(("best", "inter", "uni"), (best, inter, uni), want_best[i]):
            same(g.cpu().numpy(), v, f"replay on pair {i}: {name}")
        same(running.cpu().numpy(), total, f"replay on pair {i}: the running table adds")


# -------------------------------------------------------------------------------------------------------- round trip
def test_drawn_shapes_match_the_regions_found_in_their_own_label_map(device) -> None:
    square = [(3.0, 2.0), (20.0, 2.0), (20.0, 17.0), (3.0, 17.0)]
    octagon = [(40.0, 5.5), (52.0, 5.5), (60.5, 14.0), (60.5, 26.0), (52.0, 34.5), (40.0, 34.5), (31.5, 26.0), (31.5, 14.0)]
    frame = [[(5.0, 24.0), (26.0, 24.0), (26.0, 44.0), (5.0, 44.0)], [(10.0, 29.0), (21.0, 29.0), (21.0, 39.0), (10.0, 39.0)]]
    inside = [(12.0, 31.0), (19.0, 31.0), (19.0, 37.0), (12.0, 37.0)]  # in the frame's hole, touching nothing
    slab = [(0.0, 46.0), (70.0, 46.0), (70.0, 50.0), (0.0, 50.0)]
    polygons = [[square, octagon, frame, inside, slab], [octagon, slab], []]
    drawn = rasterize_polygons(polygons, (50, 70), device=device)
    assert drawn.dtype == torch.int32 and int(drawn.max()) == 4
    labels = torch.where(drawn >= 0, drawn + 10, torch.full_like(drawn, 255)).to(torch.uint8)  # a class per shape
    found = label_regions(labels, max_regions=16)
    assert found.num.tolist() == [5, 2, 0]
    m = match_regions(drawn, found, 5, 16, both=True)
    pixels = torch.stack([(drawn == r).sum(dim=(1, 2)) for r in range(5)], dim=1)
    has = pixels > 0
    assert has.tolist() == [[True] * 5, [True, True, False, False, False], [False] * 5]
    assert torch.equal(m.inter, m.union) and torch.equal(m.inter, pixels)  # IoU exactly 1 for every drawn shape
    assert bool((m.best[has] >= 0).all()) and bool((m.best[~has] == -1).all())
    assert bool((m.iou()[has] == 1.0).all()) and bool(torch.isnan(m.iou()[~has]).all())
    # ... and each found region is matched back by the shape it came from
    back = m.best_b.cpu().numpy()
    for k, i in torch.nonzero(has).tolist():
        assert back[k, int(m.best[k, i])] == i
    # the classes found are the shapes' own
    label = found.label.cpu().numpy()
    for k, i in torch.nonzero(has).tolist():
        assert label[k, int(m.best[k, i])] == i + 10
