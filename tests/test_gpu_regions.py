"""isc_label_regions on the GPU against tests/regions_oracle.py (which tests/test_regions_host.py checks on the CPU),
value for value on every output.  The kernels are called through the C ABI into the interior of buffers filled with a
pattern, whose guard bytes must survive, with a workspace full of the same pattern; the Python layer follows.  The maps
aim at the borders of the kernel's tiles (`isc_label_regions_geometry`)."""

from __future__ import annotations

import ctypes
import functools
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import regions_oracle as ro  # noqa: E402

from imagescry_amd import LabelMaps, _lib, label_regions, segmentation  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes on either side of an output
FILL = 0xA5  # int32 0xA5A5A5A5 is negative and no id, label 165 no class of these maps: wrong wherever it survives
TILE = (64, 16)  # isc_label_regions_geometry, needed before a library can be asked (test ids); test_geometry checks it
TW, TH = TILE
U = ro.UNLABELED

DTYPES = {"ids": np.int32, "num": np.int32, "labels_out": np.uint8, "label": np.int32, "area": np.int32,
          "anchor": np.int32, "box": np.int32, "sum": np.int64, "peak": np.int32, "peak_score": np.float32}
ORDER = ("ids", "num", "labels_out", "label", "area", "anchor", "box", "sum", "peak", "peak_score")  # the C ABI's


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


def shapes(b: int, h: int, w: int, r: int) -> dict[str, tuple[int, ...]]:
    return {"ids": (b, h, w), "num": (b,), "labels_out": (b, h, w), "label": (b, r), "area": (b, r), "anchor": (b, r),
            "box": (b, r, 4), "sum": (b, r, 2), "peak": (b, r), "peak_score": (b, r)}


def workspace(device: torch.device, b: int, h: int, w: int) -> torch.Tensor:
    need = ctypes.c_size_t()
    assert _lib.load().isc_label_regions_workspace_bytes(b, h, w, need) == 0
    return torch.full((need.value,), FILL, dtype=torch.uint8, device=device)


def run(device: torch.device, labels: np.ndarray, best: np.ndarray | None = None, connectivity: int = 8, min_area: int = 1,
        max_regions: int = 1024, outputs: tuple[str, ...] | None = None, expect: int = 0,
        shift: int = 0) -> dict[str, np.ndarray]:
    """isc_label_regions into guarded buffers; `outputs` defaults to all (the peaks only with `best`).  `shift` moves the
    input labels off their buffer's alignment by that many bytes."""
    b, h, w = labels.shape
    if outputs is None:
        outputs = ORDER if best is not None else ORDER[:-2]
    ld = torch.cat([torch.zeros(shift, dtype=torch.uint8), torch.from_numpy(labels).reshape(-1)]).to(device)[shift:]
    ld = ld.reshape(labels.shape)
    assert ld.data_ptr() % 256 == shift
    bd = None if best is None else torch.from_numpy(best).to(device)
    shp = shapes(b, h, w, max_regions)
    bufs = {k: Guarded(int(np.prod(shp[k])) * np.dtype(DTYPES[k]).itemsize, DTYPES[k], device) for k in outputs}
    ws = workspace(device, b, h, w)
    st = _lib.load().isc_label_regions(ld.data_ptr(), _lib.ptr(bd), b, h, w, connectivity, min_area, max_regions,
                                       *(bufs[k].ptr if k in bufs else None for k in ORDER), ws.data_ptr(), ws.numel(),
                                       _lib.stream_handle(device))
    assert st == expect, _lib.strerror(st)
    torch.cuda.synchronize()
    assert np.array_equal(ld.cpu().numpy(), labels), "the input was written"
    return {k: bufs[k].numpy(shp[k]) for k in outputs}


def check(got: dict[str, np.ndarray], want: dict[str, np.ndarray]) -> None:
    for k, v in got.items():
        assert ro.same(v, want[k]), f"{k} differs from the oracle at {int((v != want[k]).sum())} places"


def scores_for(labels: np.ndarray, seed: int) -> np.ndarray:
    """Scores on a grid of halves, so that they tie, with a few NaNs."""
    rng = np.random.default_rng(seed)
    best = (np.round(rng.standard_normal(labels.shape) * 2) / 2).astype(np.float32)
    best[rng.random(labels.shape) < 0.03] = np.nan
    return best


def both(device: torch.device, labels: np.ndarray, seed: int = 0, **kw: int) -> dict[int, dict[str, np.ndarray]]:
    """Run and check both connectivities with scores; -> the oracle's outputs per connectivity."""
    best = scores_for(labels, seed)
    refs = {}
    for connectivity in (4, 8):
        refs[connectivity] = ro.label_regions_ref(labels, best, connectivity=connectivity, **kw)
        check(run(device, labels, best, connectivity=connectivity, **kw), refs[connectivity])
    return refs


def canvas(h: int, w: int) -> np.ndarray:
    return np.full((1, h, w), U, np.uint8)


def tiles_touched(ids: np.ndarray, region: int) -> int:
    ys, xs = np.nonzero(ids == region)
    return len(set(zip((ys // TH).tolist(), (xs // TW).tolist())))


# ---------------------------------------------------------------------------------------------------------------- sizes
def test_geometry() -> None:
    assert segmentation.label_regions_geometry() == TILE, "the maps below are aimed at TILE: change it with the kernel's tile"


DEGENERATE = [(1, 1), (1, TW + 1), (TH + 1, 1), (TH, TW), (TH - 1, TW - 1), (TH - 1, TW + 1), (TH + 1, TW - 1), (TH + 1, TW + 1)]


@pytest.mark.parametrize("size", DEGENERATE, ids=[f"{h}x{w}" for h, w in DEGENERATE])
def test_degenerate_sizes(device, size) -> None:
    labels = ro.random_map((2, *size), [0.5, 0.3], seed=sum(size))
    both(device, labels, seed=size[0])
    both(device, np.full((1, *size), 4, np.uint8), max_regions=1)


def test_one_class_and_no_class(device) -> None:
    h, w = 3 * TH + 5, 3 * TW + 7
    refs = both(device, np.full((2, h, w), 7, np.uint8))
    for ref in refs.values():
        assert ref["num"].tolist() == [1, 1] and ref["area"][:, 0].tolist() == [h * w] * 2 and (ref["ids"] == 0).all()
        assert ref["box"][0, 0].tolist() == [0, 0, h, w] and ref["sum"][0, 0].tolist() == [w * h * (h - 1) // 2, h * w * (w - 1) // 2]
    refs = both(device, np.full((2, h, w), U, np.uint8))
    for ref in refs.values():
        assert ref["num"].tolist() == [0, 0] and (ref["ids"] == -1).all() and (ref["label"] == -1).all()


def test_checkerboard(device) -> None:
    h, w = 2 * TH + 1, 2 * TW + 3
    refs = both(device, ro.checkerboard(h, w), max_regions=100)
    assert refs[4]["num"][0] == h * w > 100  # the true count; the tables stop at 100 rows, the ids do not
    assert np.array_equal(refs[4]["ids"][0].reshape(-1), np.arange(h * w)) and refs[4]["anchor"][0, 99] == 99
    assert refs[8]["num"][0] == 2 and refs[8]["area"][0, :3].tolist() == [(h * w + 1) // 2, h * w // 2, 0]


@pytest.mark.parametrize("anti", [False, True], ids=["diagonal", "anti-diagonal"])
def test_contact_across_a_tile_corner(device, anti: bool) -> None:
    m = canvas(2 * TH, 2 * TW)
    m[0, TH - 1, TW if anti else TW - 1] = m[0, TH, TW - 1 if anti else TW] = 2
    refs = both(device, m)
    assert refs[8]["num"][0] == 1 and refs[8]["area"][0, 0] == 2 and refs[4]["num"][0] == 2
    # the same with a second class on the other diagonal of the corner: the two cross without joining
    m[0, TH - 1, TW - 1 if anti else TW] = m[0, TH, TW if anti else TW - 1] = 3
    refs = both(device, m)
    assert refs[8]["num"][0] == 2 and refs[4]["num"][0] == 4


def reentry_maps() -> dict[str, np.ndarray]:
    h, w = 3 * TH + 5, 3 * TW + 7
    arms = canvas(h, w)  # two arms apart inside the first tile column, joined only inside the second
    arms[0, 2, 10:TW + 7] = arms[0, 5, 10:TW + 7] = 1
    arms[0, 2:6, TW + 6] = 1
    arms_v = canvas(h, w)  # two arms apart inside the first tile row, joined only inside the second
    arms_v[0, 3:TH + 5, 20] = arms_v[0, 3:TH + 5, 23] = 1
    arms_v[0, TH + 4, 20:24] = 1
    comb = canvas(h, w)  # teeth that cross a horizontal tile border at every other column, the spine below it
    comb[0, TH - 6:TH + 4, 0::2] = 6
    comb[0, TH + 4, :] = 6
    comb_v = canvas(h, w)  # teeth that cross a vertical tile border at every other row, the spine right of it
    comb_v[0, 0::2, TW - 6:TW + 4] = 6
    comb_v[0, :, TW + 4] = 6
    return {"arms": arms, "arms vertical": arms_v, "comb": comb, "comb vertical": comb_v}


@pytest.mark.parametrize("name", list(reentry_maps()))
def test_reentry(device, name: str) -> None:
    m = reentry_maps()[name]
    refs = both(device, m)
    assert refs[4]["num"][0] == refs[8]["num"][0] == 1 and refs[4]["area"][0, 0] == (m != U).sum()
    # without the joining piece the parts are apart: the map tests what its name says
    cut = m.copy()
    if name.startswith("arms"):
        cut[0, 3:5, TW + 6] = U
        cut[0, TH + 4, 21:23] = U
        assert ro.label_regions_ref(cut)["num"][0] == 2
    else:
        cut[0, TH + 4, :] = U
        cut[0, :, TW + 4] = U
        assert ro.label_regions_ref(cut)["num"][0] > 20
    both(device, cut)


@pytest.mark.parametrize("name", ["serpentine", "spiral"])
def test_longest_chains(device, name: str) -> None:
    m = getattr(ro, name)(3 * TH, 3 * TW)
    refs = both(device, m)
    assert refs[4]["num"][0] == 1 and refs[4]["area"][0, 0] == (m != U).sum() > 3 * TH * TW and tiles_touched(refs[4]["ids"][0], 0) == 9
    # the width is a multiple of four: rows are read four labels a load -- unless the map starts off a dword
    best = scores_for(m, 0)
    for shift in (1, 2):
        check(run(device, m, best, connectivity=8, shift=shift), refs[8])


# ---------------------------------------------------------------------------------------------------------- random maps
RANDOM = {3: [0.7, 0.12, 0.08], 7: [0.66] + [0.04] * 6}  # + a tenth unlabeled; the first class percolates


@functools.lru_cache(maxsize=None)
def random_case(classes: int, seed: int) -> np.ndarray:
    return ro.random_map((3, 2 * TH + 13, 2 * TW + 22), RANDOM[classes], seed=seed)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("classes", [3, 7])
def test_random_maps(device, classes: int, seed: int) -> None:
    labels = random_case(classes, seed)
    assert not np.array_equal(labels[0], labels[1]) and not np.array_equal(labels[1], labels[2])
    refs = both(device, labels, seed=seed, max_regions=512)
    for ref in refs.values():  # the case cannot go soft: single pixels, and a region over more than four tiles
        for b in range(3):
            n = min(int(ref["num"][b]), 512)
            assert n > 50 and (ref["area"][b, :n] == 1).any()
            big = int(ref["area"][b, :n].argmax())
            assert tiles_touched(ref["ids"][b], big) > 4
    # an image's answer does not depend on its place in the batch
    best = scores_for(labels, seed)
    alone = run(device, labels[2:3], best[2:3], connectivity=4, max_regions=512)
    check(alone, {k: v[2:3] for k, v in refs[4].items()})


@pytest.mark.parametrize("min_area", [2, 5, "all"])
def test_min_area(device, min_area) -> None:
    labels = random_case(3, 1)
    largest = int(ro.label_regions_ref(labels, max_regions=4096)["area"].max())
    area = largest + 1 if min_area == "all" else min_area
    refs = both(device, labels, seed=5, min_area=area, max_regions=512)
    plain = ro.label_regions_ref(labels, max_regions=4096)
    for b in range(3):
        if min_area == "all":
            assert refs[8]["num"][b] == 0 and (refs[8]["labels_out"][b] == U).all() and (refs[8]["ids"][b] == -1).all()
        else:  # numbering is over the kept regions only, in the same order
            keep = plain["area"][b, :plain["num"][b]] >= area
            assert 0 < refs[8]["num"][b] == keep.sum() < plain["num"][b]
            assert np.array_equal(refs[8]["anchor"][b, :keep.sum()], plain["anchor"][b, :plain["num"][b]][keep][:512])
            assert ((refs[8]["labels_out"][b] == U) == (refs[8]["ids"][b] == -1)).all()
    # a NULL labels_out is accepted and changes nothing else
    best = scores_for(labels, 5)
    names = tuple(k for k in ORDER if k != "labels_out")
    check(run(device, labels, best, min_area=area, max_regions=512, outputs=names), refs[8])


def test_peak_order(device) -> None:
    h, w = 2 * TH + 8, 2 * TW + 22
    m = canvas(h, w)
    m[0, :, :TW + 6] = 1  # region 0 lies in four tiles and more
    m[0, :20, TW + 6:] = 2
    m[0, 20:, TW + 6:] = 3
    best = np.full((1, h, w), -1.0, np.float32)
    best[0, 30, TW + 1] = best[0, 3, 10] = best[0, TH + 2, 5] = 5.0  # a tie across three tiles: the lowest index
    best[0, 0, :8] = np.nan  # NaNs in front of it
    best[0, 3, 11] = np.nan
    best[0, :20, TW + 6:] = 0.0
    best[0, 0, TW + 6] = -0.0  # -0.0 ties with the +0.0 behind it and comes first
    best[0, 1, TW + 6:] = np.nan
    best[0, 20:, TW + 6:] = np.nan  # a region that is all NaN: its anchor
    for connectivity in (4, 8):
        ref = ro.label_regions_ref(m, best, connectivity=connectivity)
        check(run(device, m, best, connectivity=connectivity), ref)
        assert ref["peak"][0, :3].tolist() == [3 * w + 10, TW + 6, 20 * w + TW + 6]
        assert ref["peak_score"][0, 0] == 5.0 and np.signbit(ref["peak_score"][0, 1]) and np.isnan(ref["peak_score"][0, 2])
    best[0, 0, TW + 6] = 0.0
    best[0, 0, TW + 9] = -0.0  # the other way round: still the first of the tie
    got = run(device, m, best)
    check(got, ro.label_regions_ref(m, best))
    assert got["peak"][0, 1] == TW + 6 and not np.signbit(got["peak_score"][0, 1])
    inf = np.full((1, h, w), -np.inf, np.float32)  # -inf everywhere still beats a NaN
    inf[0, 0, 0] = np.nan
    got = run(device, m, inf)
    check(got, ro.label_regions_ref(m, inf))
    assert got["peak"][0, 0] == 1


def test_every_subset_of_tables(device) -> None:
    labels = np.concatenate([ro.random_map((1, TH + 3, TW + 5), [0.5, 0.3], seed=9),
                             ro.random_map((1, TH + 3, TW + 5), [0.85, 0.05], seed=109)])
    best = scores_for(labels, 8)
    ref = ro.label_regions_ref(labels, best, min_area=2, max_regions=40)
    assert 5 < ref["num"].min() and ref["num"].max() > 40 > ref["num"].min()  # one image truncated, one not
    for n in range(len(ro.TABLES) + 1):
        for tables in itertools.combinations(ORDER[3:], n):
            check(run(device, labels, best, min_area=2, max_regions=40, outputs=ORDER[:3] + tables), ref)
    # without scores: the peak outputs are an error, everything else is the same
    run(device, labels, None, outputs=("ids", "num", "peak"), expect=_lib.ISC_ERR_INVALID_ARG)
    check(run(device, labels, None, min_area=2, max_regions=40), ref)
    check(run(device, labels, None, min_area=2, max_regions=40, outputs=("ids", "num")), ref)


# ------------------------------------------------------------------------------------------------ determinism and replay
def test_determinism_and_graph_replay(device) -> None:
    maps = [random_case(3, 1), random_case(7, 2), ro.serpentine(2 * TH + 13, 2 * TW + 22).repeat(3, axis=0)]
    bests = [scores_for(m, 20 + i) for i, m in enumerate(maps)]
    refs = [ro.label_regions_ref(m, s, min_area=2, max_regions=300) for m, s in zip(maps, bests)]
    first, second = (run(device, maps[0], bests[0], min_area=2, max_regions=300) for _ in range(2))
    for k in ORDER:
        assert first[k].tobytes() == second[k].tobytes() or k == "peak_score" and ro.same(first[k], second[k])
    b, h, w = maps[0].shape
    shp = shapes(b, h, w, 300)
    torch_dtype = {np.int32: torch.int32, np.uint8: torch.uint8, np.int64: torch.int64, np.float32: torch.float32}
    labels, best = torch.from_numpy(maps[0]).to(device), torch.from_numpy(bests[0]).to(device)
    out = {k: torch.empty(shp[k], dtype=torch_dtype[DTYPES[k]], device=device) for k in ORDER}
    ws = workspace(device, b, h, w)

    def call() -> None:
        st = _lib.load().isc_label_regions(labels.data_ptr(), best.data_ptr(), b, h, w, 8, 2, 300,
                                           *(out[k].data_ptr() for k in ORDER), ws.data_ptr(), ws.numel(),
                                           _lib.stream_handle(device))
        assert st == 0

    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        call()  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        call()
    for i in (1, 2, 0):
        labels.copy_(torch.from_numpy(maps[i]))  # the input overwritten in place
        best.copy_(torch.from_numpy(bests[i]))
        for k in ORDER:
            out[k].fill_(-7 if k != "labels_out" else 99)
        graph.replay()
        torch.cuda.synchronize()
        check({k: out[k].cpu().numpy() for k in ORDER}, refs[i])
    assert not np.array_equal(refs[0]["ids"], refs[1]["ids"])


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer(device) -> None:
    labels = random_case(3, 2)
    best = scores_for(labels, 9)
    ld, bd = torch.from_numpy(labels).to(device), torch.from_numpy(best).to(device)
    ref = ro.label_regions_ref(labels, best, connectivity=4, min_area=3, max_regions=200)

    def fields(r) -> dict[str, np.ndarray]:
        pairs = {"ids": r.ids, "num": r.num, "labels_out": r.labels, "label": r.label, "area": r.area, "anchor": r.anchor,
                 "box": r.boxes, "sum": r.sums, "peak": r.peak, "peak_score": r.peak_scores}
        return {k: v.cpu().numpy() for k, v in pairs.items() if v is not None}

    got = label_regions(ld, scores=bd, connectivity=4, min_area=3, max_regions=200, return_labels=True)
    assert set(fields(got)) == set(ORDER) and got.indices is None and got.device == device and len(got) == 3
    check(fields(got), ref)
    plain = label_regions(ld, connectivity=4, min_area=3, max_regions=200)  # a tensor alone: no peaks, no map
    assert plain.peak is None and plain.peak_scores is None and plain.labels is None
    check(fields(plain), ref)
    maps = LabelMaps(labels=ld, scores=bd, indices=torch.tensor([7, 3, 5]))
    via = maps.regions(connectivity=4, min_area=3, max_regions=200, return_labels=True)
    check(fields(via), ref)
    assert via.indices.tolist() == [7, 3, 5]
    check(fields(label_regions(maps, connectivity=4, min_area=3, max_regions=200)), ref)
    defaults = label_regions(ld)
    check(fields(defaults), ro.label_regions_ref(labels, connectivity=8, min_area=1, max_regions=1024))
    n = int(ref["num"].min())
    centroids = got.centroids().cpu().numpy()
    assert np.array_equal(centroids[:, :n], ref["sum"][:, :n] / ref["area"][:, :n, None]) and np.isnan(centroids[:, 199]).all()
    cells = got.peak_cells((5, 9)).cpu().numpy()
    h, w = labels.shape[1:]
    y, x = ref["peak"] // w, ref["peak"] % w
    assert np.array_equal(cells, np.where(ref["peak"] >= 0, ((2 * y + 1) * 5 // (2 * h)) * 9 + (2 * x + 1) * 9 // (2 * w), -1))
    host = got.cpu()
    assert host.device.type == "cpu" and torch.equal(host.ids, got.ids.cpu())
    assert label_regions(ld[:0]).ids.shape == (0, h, w)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        label_regions(ld.cpu())
    with pytest.raises(TypeError, match="uint8"):
        label_regions(ld.to(torch.int64))
    with pytest.raises(TypeError, match="float32"):
        label_regions(ld, scores=bd.double())
    with pytest.raises(ValueError, match="scores on"):
        label_regions(ld, scores=bd.cpu())


def test_regions_behind_a_label_map(device) -> None:
    g = torch.Generator().manual_seed(4)
    scores = torch.randn((2, 5, 5, 3), generator=g).to(device)
    maps = segmentation.label_map(scores, (37, 41), min_score=-0.2)
    regions = maps.regions(min_area=4, return_labels=True)
    labels, best = maps.labels.cpu().numpy(), maps.scores.cpu().numpy()
    assert (labels == U).any() and len(np.unique(labels)) == 4
    ref = ro.label_regions_ref(labels, best, min_area=4, max_regions=1024)
    check({"ids": regions.ids.cpu().numpy(), "num": regions.num.cpu().numpy(), "labels_out": regions.labels.cpu().numpy(),
           "label": regions.label.cpu().numpy(), "area": regions.area.cpu().numpy(), "box": regions.boxes.cpu().numpy(),
           "sum": regions.sums.cpu().numpy(), "peak": regions.peak.cpu().numpy(),
           "peak_score": regions.peak_scores.cpu().numpy(), "anchor": regions.anchor.cpu().numpy()}, ref)
    assert 0 < ref["num"].min()
