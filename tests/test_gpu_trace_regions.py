"""isc_trace_regions on the GPU against its definition (tests/outline_oracle.py), value for value: every output array of
every case below must equal the oracle's.  The shapes sit on the seams that isc_trace_regions_geometry reports; every call
gets a workspace and outputs full of 0xA5 bytes, and the vertex rows the definition leaves untouched must stay so."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import outline_oracle as oo
import regions_oracle as ro
from imagescry_amd import _lib, label_regions, pack_polygons, rasterize_polygons, segmentation, trace_regions

pytestmark = pytest.mark.gpu

FILL = np.int32(np.uint32(0xA5A5A5A5).view(np.int32))
NAMES = ("vertices", "ring_start", "ring_region", "image_start", "ring_area2", "num_rings", "num_vertices")


def run(device: torch.device, ids: np.ndarray, rows: int, connectivity: int, n: int, v: int,
        area: bool = True) -> dict[str, np.ndarray]:
    """The C ABI itself on int32 [B, H, W] -> every output."""
    lib = _lib.load()
    b, h, w = ids.shape
    need = ctypes.c_size_t()
    assert lib.isc_trace_regions_workspace_bytes(b, h, w, need) == _lib.ISC_OK
    workspace = torch.full((need.value,), 0xA5, dtype=torch.uint8, device=device)

    def filled(*shape: int, dtype: torch.dtype = torch.int32) -> torch.Tensor:
        count = int(np.prod(shape)) * dtype.itemsize
        return torch.full((count,), 0xA5, dtype=torch.uint8, device=device).view(dtype).reshape(shape)

    out = {"vertices": filled(b, v, 2), "ring_start": filled(b * (n + 1) + 1), "ring_region": filled(b, n + 1),
           "image_start": filled(b + 1), "ring_area2": filled(b, n, dtype=torch.int64), "num_rings": filled(b),
           "num_vertices": filled(b)}
    dev_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(device)
    st = lib.isc_trace_regions(dev_ids.data_ptr(), b, h, w, rows, connectivity, n, v, out["vertices"].data_ptr(),
                               out["ring_start"].data_ptr(), out["ring_region"].data_ptr(), out["image_start"].data_ptr(),
                               out["ring_area2"].data_ptr() if area else None, out["num_rings"].data_ptr(),
                               out["num_vertices"].data_ptr(), workspace.data_ptr(), need.value,
                               _lib.stream_handle(device))
    assert st == _lib.ISC_OK
    torch.cuda.synchronize(device)
    return {k: t.cpu().numpy() for k, t in out.items()}


def expected(ids: np.ndarray, rows: int, connectivity: int, n: int, v: int) -> dict[str, np.ndarray]:
    ref = oo.trace_regions_ref(ids, rows, connectivity, n, v)
    ref["vertices"] = np.where(ref.pop("written")[..., None], ref["vertices"], FILL)  # untouched rows keep the fill
    return ref


def check(device: torch.device, ids: np.ndarray, rows: int, connectivity: int, n: int | None = None,
          v: int | None = None) -> dict[str, np.ndarray]:
    """The call against the oracle, with capacities that hold the worst case unless given -> the outputs."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n = ids[0].size if n is None else n
    v = 4 * ids[0].size if v is None else v
    want = expected(ids, rows, connectivity, n, v)
    got = run(device, ids, rows, connectivity, n, v)
    for name in ("num_vertices", "num_rings", "image_start", "ring_region", "ring_start", "ring_area2", "vertices"):
        wrong = np.argwhere(got[name] != want[name])
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert wrong.size == 0, (f"{name} (connectivity {connectivity}): {len(wrong)} entries differ, the first at "
                                 f"{wrong[0].tolist()}: got {got[name][tuple(wrong[0])]}, want {want[name][tuple(wrong[0])]}")
    return got


@pytest.fixture(scope="module")
def geometry() -> tuple[int, int, int, int]:
    return segmentation.trace_geometry()


def side_for(pixels: int) -> tuple[int, int]:
    """An odd-sized image of a little more than `pixels` pixels."""
    h = int(np.sqrt(pixels)) | 1
    return h, pixels // h + 2


@pytest.mark.parametrize("connectivity", [4, 8])
def test_degenerate_images_single_pixels_and_full_images(device, geometry, connectivity: int) -> None:
    chunk = geometry[0]
    for size in ((1, 1), (1, 2 * chunk + 7), (chunk + 3, 1)):
        full = np.zeros((1, *size), np.int32)
        got = check(device, full, 1, connectivity)
        assert got["num_rings"][0] == 1 and got["num_vertices"][0] == 4  # a full image: one ring of 4 vertices
        check(device, np.stack([oo.random_ids(size, 2, seed) for seed in range(3)]), 2, connectivity)
    h, w = side_for(2 * chunk)
    one = np.full((2, h, w), -1, np.int32)
    one[0, h - 1, w - 1] = 0  # a single pixel, in the last chunk's last place
    one[1, 0, 0] = 0
    got = check(device, one, 1, connectivity)
    assert got["ring_area2"][:, 0].tolist() == [2, 2]
    got = check(device, np.zeros((1, h, w), np.int32), 1, connectivity)
    assert got["ring_area2"][0, 0] == 2 * h * w
    check(device, np.full((2, h, w), -1, np.int32), 3, connectivity)  # nothing at all


@pytest.mark.parametrize("connectivity", [4, 8])
def test_rectangle_across_every_chunk_seam(device, geometry, connectivity: int) -> None:
    h, w = side_for(3 * geometry[0])
    ids = np.full((1, h, w), -1, np.int32)
    ids[0, 1:h - 1, 2:w - 1] = 0
    got = check(device, ids, 1, connectivity)
    assert got["num_vertices"][0] == 4 and got["ring_area2"][0, 0] == 2 * (h - 2) * (w - 3)


def test_diagonal_pair_under_both_connectivities(device) -> None:
    pair = np.asarray([[[0, -1], [-1, 0]]], np.int32)
    apart = check(device, pair, 1, 4)
    assert apart["num_rings"][0] == 2 and apart["num_vertices"][0] == 8
    joined = check(device, pair, 1, 8)
    assert joined["num_rings"][0] == 1 and joined["num_vertices"][0] == 8 and joined["ring_area2"][0, 0] == 4
    other = np.asarray([[[-1, 0], [0, -1]]], np.int32)
    assert check(device, other, 1, 4)["num_rings"][0] == 2
    assert check(device, other, 1, 8)["num_rings"][0] == 1


@pytest.mark.parametrize("connectivity", [4, 8])
def test_holes_islands_and_an_island_of_the_same_id(device, connectivity: int) -> None:
    for ids in (np.stack([oo.nested_ids(), np.flipud(oo.nested_ids())]), oo.nested_ids(31, 45)[None]):
        got = check(device, ids, 2, connectivity)
        assert (got["num_rings"] == 5).all()
        assert (np.sign(got["ring_area2"][:, :5]) == [1, -1, 1, 1, -1]).all()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("regions", [1, 2])
def test_checkerboards(device, geometry, connectivity: int, regions: int) -> None:
    # more rings than a ring tile, more nodes than a node chunk, more pixels than a pixel chunk
    h, w = side_for(max(geometry[0], geometry[1], 2 * geometry[2]) + 100)
    got = check(device, oo.checkerboard_ids(h, w, regions)[None], 2, connectivity)
    if connectivity == 4:
        assert got["num_rings"][0] == (h * w if regions == 2 else (h * w + 1) // 2) > geometry[2]
    assert got["num_vertices"][0] == (4 * h * w if regions == 2 else 4 * ((h * w + 1) // 2)) > geometry[1]


def test_more_nodes_than_one_pass_of_the_node_launches(device, geometry) -> None:
    h, w = side_for(geometry[3] // 4 + 1)
    got = check(device, oo.checkerboard_ids(h, w, 2)[None], 2, 4)
    assert got["num_vertices"][0] > geometry[3]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_longest_rings(device, connectivity: int) -> None:
    for labels in (ro.serpentine(61, 83), ro.spiral(57, 64), ro.serpentine(2, 300), ro.spiral(90, 3)):
        ids = np.where(labels != ro.UNLABELED, 0, -1).astype(np.int32)
        got = check(device, ids, 1, connectivity)
        assert got["num_rings"][0] == 1 and got["num_vertices"][0] >= 4


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ids_outside_the_regions_are_no_region(device, connectivity: int) -> None:
    ids = oo.random_ids((2, 23, 37), 3, 77)
    ids[0, :5] = np.iinfo(np.int32).min
    ids[1, :, :4] = np.iinfo(np.int32).max
    ids[1, 10:14, 10:20] = 3  # == R
    check(device, ids, 3, connectivity)
    check(device, ids, 1, connectivity)  # regions 1 and 2 are outside now


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("group", range(4))
def test_random_maps(device, connectivity: int, group: int) -> None:
    size = ((37, 61), (64, 64), (5, 431), (130, 9))[group]
    rows = 1 + group
    ids = np.stack([oo.random_ids(size, rows, 5 * group + k, fill=0.35 + 0.15 * k) for k in range(5)])  # 20 seeds
    check(device, ids, rows, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_capacities_at_and_below_the_counts(device, connectivity: int) -> None:
    ids = np.stack([oo.random_ids((19, 26), 2, 3 + k, fill=fill) for k, fill in enumerate((0.1, 0.4, 0.05))])
    full = check(device, ids, 2, connectivity)
    rings, vertices = full["num_rings"].tolist(), full["num_vertices"].tolist()
    assert rings[1] > max(rings[0], rings[2]) and vertices[1] > max(vertices[0], vertices[2])
    exact = check(device, ids, 2, connectivity, n=rings[1], v=vertices[1])
    assert (exact["ring_region"][1, :rings[1]] >= 0).all()
    for n, v in ((rings[1] - 1, vertices[1]), (rings[1], vertices[1] - 1), (rings[1] - 1, vertices[1] - 1)):
        short = check(device, ids, 2, connectivity, n=n, v=v)
        assert short["num_rings"].tolist() == rings and short["num_vertices"].tolist() == vertices  # the true counts
        assert (short["ring_region"][1] == -1).all() and (short["vertices"][1] == FILL).all()
        assert (short["ring_start"][(n + 1):2 * (n + 1)] == v).all()
        for b in (0, 2):  # the images that fit come out as they did
            assert np.array_equal(short["ring_region"][b, :rings[b]], full["ring_region"][b, :rings[b]])
            assert np.array_equal(short["vertices"][b, :vertices[b]], full["vertices"][b, :vertices[b]])
            assert np.array_equal(short["ring_area2"][b, :rings[b]], full["ring_area2"][b, :rings[b]])


def test_no_area_output(device) -> None:
    ids = oo.random_ids((2, 21, 30), 2, 11)
    with_area = run(device, ids, 2, 8, 200, 900)
    without = run(device, ids, 2, 8, 200, 900, area=False)
    assert (without["ring_area2"] == np.int64(np.uint64(0xA5A5A5A5A5A5A5A5).view(np.int64))).all()  # never touched
    assert all(np.array_equal(without[k], with_area[k]) for k in NAMES if k != "ring_area2")


@pytest.mark.parametrize("connectivity", [4, 8])
def test_an_image_alone_and_in_a_batch_and_two_runs(device, connectivity: int) -> None:
    ids = np.stack([oo.random_ids((33, 47), 3, seed, fill=0.3 + 0.1 * seed) for seed in range(4)])
    n, v = 33 * 47, 4 * 33 * 47
    batch = run(device, ids, 3, connectivity, n, v)
    again = run(device, ids, 3, connectivity, n, v)
    assert all(batch[k].tobytes() == again[k].tobytes() for k in NAMES)
    for b in range(4):
        alone = run(device, ids[b:b + 1], 3, connectivity, n, v)
        assert alone["num_rings"][0] == batch["num_rings"][b] and alone["num_vertices"][0] == batch["num_vertices"][b]
        assert alone["vertices"][0].tobytes() == batch["vertices"][b].tobytes()
        assert alone["ring_region"][0].tobytes() == batch["ring_region"][b].tobytes()
        assert alone["ring_area2"][0].tobytes() == batch["ring_area2"][b].tobytes()
        assert np.array_equal(alone["ring_start"][:n + 1], batch["ring_start"][b * (n + 1):(b + 1) * (n + 1)] - b * v)


def test_graph_replay_after_ids_are_overwritten_in_place(device) -> None:
    maps = [oo.random_ids((3, 40, 52), 3, seed, fill=0.5) for seed in (21, 22, 23)]
    n, v = 600, 4000
    want = [expected(m, 3, 8, n, v) for m in maps]
    assert all((w["num_rings"] <= n).all() and (w["num_vertices"] <= v).all() for w in want)
    live = torch.from_numpy(maps[0]).to(device)
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        trace_regions(live, 3, max_rings=n, max_vertices=v)  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = trace_regions(live, 3, max_rings=n, max_vertices=v)
    for i in (1, 2, 0, 1):
        live.copy_(torch.from_numpy(maps[i]))  # refilled in place
        for t in (out.packed.ring_start, out.packed.ring_region, out.packed.image_start, out.ring_area2, out.num_rings,
                  out.num_vertices):
            t.fill_(-9)  # garbage where the graph has to start over
        out.packed.vertices.copy_(torch.from_numpy(np.full((3 * v, 2), FILL)))
        graph.replay()
        torch.cuda.synchronize()
        got = {"vertices": out.packed.vertices.reshape(3, v, 2), "ring_start": out.packed.ring_start,
               "ring_region": out.packed.ring_region.reshape(3, n + 1), "image_start": out.packed.image_start,
               "ring_area2": out.ring_area2, "num_rings": out.num_rings, "num_vertices": out.num_vertices}
        for name in NAMES:
            assert np.array_equal(got[name].cpu().numpy(), want[i][name]), f"replay on map {i}: {name}"


@pytest.mark.parametrize("connectivity", [4, 8])
def test_device_round_trip_through_rasterize_polygons(device, connectivity: int) -> None:
    ids = np.concatenate([oo.random_ids((3, 70, 90), 4, 31, fill=0.8), oo.nested_ids(70, 90)[None],
                          oo.checkerboard_ids(70, 90, 2)[None]])
    dev = torch.from_numpy(ids).to(device)
    out = trace_regions(dev, 4, connectivity=connectivity, max_rings=70 * 90, max_vertices=4 * 70 * 90)
    want = torch.where((dev >= 0) & (dev < 4), dev, torch.full_like(dev, -1))
    back = [rasterize_polygons(out.packed, out.size, num_regions=4, fill_rule=rule) for rule in ("evenodd", "nonzero")]
    assert bool(out.complete().all())  # the first host read
    assert torch.equal(back[0], want) and torch.equal(back[1], want)
    assert out.packed.vertices.shape == (5 * out.max_vertices, 2) and len(out.packed) == 5 == len(out)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_outlines_of_label_regions_match_its_tables(device, connectivity: int) -> None:
    labels = ro.random_map((3, 75, 101), [0.35, 0.3, 0.2], seed=40 + connectivity, smooth=5)
    regions = label_regions(torch.from_numpy(labels).to(device), connectivity=connectivity, max_regions=1024)
    out = regions.outlines(connectivity=connectivity, max_rings=4096, max_vertices=30000)
    assert out.label is regions.label and out.num is regions.num
    assert bool(out.complete().all())
    host, tables = out.cpu(), regions.cpu()
    n = out.max_rings
    region = host.packed.ring_region.reshape(3, n + 1).numpy()
    start = host.packed.ring_start.numpy()
    vertices = host.packed.vertices.numpy() // 256
    for b in range(3):
        num = int(tables.num[b])
        assert 20 < num <= 1024
        for r in range(num):
            mine = np.flatnonzero(region[b] == r)
            assert len(mine) >= 1 and (np.diff(mine) == 1).all()
            area2 = host.ring_area2[b, mine].numpy()
            assert area2[0] > 0 and (area2[1:] < 0).all(), "one positive ring a region, and it comes first"
            assert area2.sum() == 2 * int(tables.area[b, r])
            k = b * (n + 1) + mine[0]
            ring = vertices[start[k]:start[k + 1]]
            anchor = int(tables.anchor[b, r])
            assert ring[0].tolist() == [anchor % 101, anchor // 101]
            assert [ring[:, 1].min(), ring[:, 0].min(), ring[:, 1].max(), ring[:, 0].max()] == tables.boxes[b, r].tolist()
        assert int(host.num_rings[b]) == int((region[b] >= 0).sum())
        assert np.array_equal(host.holes()[b].numpy(), host.ring_area2[b].numpy() < 0)


def test_shapes_back_through_pack_polygons(device) -> None:
    labels = ro.random_map((2, 48, 67), [0.4, 0.3], seed=9, smooth=4)
    regions = label_regions(torch.from_numpy(labels).to(device), connectivity=8, max_regions=512)
    out = regions.outlines(max_rings=2048, max_vertices=20000)
    shapes = out.shapes()
    want = oo.shapes_ref(regions.ids.cpu().numpy(), 512, 8)
    assert all(len(image) == 512 for image in shapes)
    for got_image, want_image in zip(shapes, want):
        for got_rings, want_rings in zip(got_image, want_image):
            assert len(got_rings) == len(want_rings)
            assert all(np.array_equal(g, w) for g, w in zip(got_rings, want_rings))
    kept = [[s for s in image if s] for image in shapes]  # regions 0 .. num - 1 are the non-empty ones, in order
    assert [len(k) for k in kept] == regions.num.tolist()
    back = rasterize_polygons(pack_polygons(kept), out.size, device=device)
    assert torch.equal(back, regions.ids)
    short = regions.outlines(max_rings=3, max_vertices=20000)
    assert not bool(short.complete().any())
    with pytest.raises(ValueError, match="beyond max_rings"):
        short.shapes()
    assert all(not rings for image in short.shapes(strict=False) for rings in image)
