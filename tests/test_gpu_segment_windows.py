"""isc_label_map_windows on the GPU against tests/segment_windows_oracle.py (which tests/test_segment_windows_host.py
checks on the CPU), value for value: labels, best, margin and counts must equal the oracle's (`so.same`).  The kernel is
called through the C ABI into guarded buffers (the helpers of tests/test_gpu_segment.py); the Python layer, graph capture
and the dense CLIP path follow.  The shapes aim at the tile (64 x 4 pixels), the prompt chunk (32), the four windows a
pixel the staged path holds, and the direct path behind it."""

from __future__ import annotations

import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_oracle as co  # noqa: E402
import segment_oracle as so  # noqa: E402
import segment_windows_oracle as swo  # noqa: E402
import test_gpu_segment as tgs  # noqa: E402  (Guarded, check, randn, the shallow CLIP: helpers, no test is taken over)

from imagescry_amd import _lib, segmentation  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
OUTPUTS = tgs.OUTPUTS
check = tgs.check
randn = tgs.randn


def grid_of(size, window, stride) -> tuple[int, int]:
    return len(swo.starts(size[0], window[0], stride[0])), len(swo.starts(size[1], window[1], stride[1]))


def run(device, scores: np.ndarray, size, window, stride, class_of=None, min_score: float = -math.inf,
        outputs: tuple[str, ...] = OUTPUTS, pad: int = 0, label_shift: int = 0, expect: int = 0) -> dict[str, np.ndarray]:
    """isc_label_map_windows on float32 [B, ny, nx, h, w, C] `scores`; `pad` extra floats of 1e30 behind every cell's
    prompts (ldc = C + pad).  Returns the outputs asked for, read back from guarded buffers."""
    b, ny, nx, h, w, c = scores.shape
    assert (ny, nx) == grid_of(size, window, stride)
    src = np.full((b, ny, nx, h, w, c + pad), F32(1e30), dtype=F32)
    src[..., :c] = scores
    sd = torch.from_numpy(src).to(device)
    cd = None if class_of is None else torch.tensor(np.asarray(class_of), dtype=torch.int32, device=device)
    shapes = {"labels": (b, *size), "best": (b, *size), "margin": (b, *size), "counts": (b, 256)}
    bufs = {k: tgs.Guarded(int(np.prod(shapes[k])) * np.dtype(tgs.NP_DTYPE[k]).itemsize, tgs.NP_DTYPE[k], device,
                           label_shift if k == "labels" else 0) for k in outputs}
    st = _lib.load().isc_label_map_windows(sd.data_ptr(), b, h, w, c, c + pad, _lib.ptr(cd), *size, *window, *stride,
                                           min_score, *(bufs[k].ptr if k in bufs else None for k in OUTPUTS),
                                           _lib.stream_handle(device))
    assert st == expect, _lib.strerror(st)
    return {k: bufs[k].numpy(shapes[k]) for k in outputs}


def random_scores(b: int, c: int, h: int, w: int, size, window, stride, seed: int) -> np.ndarray:
    return randn((b, *grid_of(size, window, stride), h, w, c), seed=seed)


@functools.lru_cache(maxsize=None)
def case(i: int):
    m, t, scores, size, window, stride = swo.case_inputs(i)
    return m, t, scores, size, window, stride, swo.label_map_windows_ref(scores, size, window, stride)


# ------------------------------------------------------------------------------------------------ isc_label_map_windows
@pytest.mark.parametrize("i", range(len(swo.CASES)))
def test_cases_equal_the_oracle(device, i: int) -> None:
    _, _, scores, size, window, stride, ref = case(i)
    check(run(device, scores, size, window, stride), ref)


def test_one_window_is_the_gpu_label_map(device) -> None:
    for i in (0, 4):
        _, _, scores, size, ref = tgs.case(i)
        got = run(device, scores[:, None, None], size, size, size)
        check(got, tgs.run(device, scores, size))
        check(got, ref)
    classes = [0, 0, 1, 2, 2, 3, 3]
    _, _, scores, size, _ = tgs.case(0)
    check(run(device, scores[:, None, None], size, size, (1, size[1]), class_of=classes, min_score=0.05),
          tgs.run(device, scores, size, class_of=classes, min_score=0.05))  # the stride of a single window says nothing


def test_stride_equal_to_the_window(device) -> None:
    _, _, scores, size, window, stride, ref = case(3)  # 129 columns: the last window column overlaps its neighbour
    got = run(device, scores, size, window, stride)
    check(got, ref)
    scores = np.ascontiguousarray(scores[:, :, :4])  # 128 columns: every pixel has one window
    got = run(device, scores, (64, 128), window, stride)
    for i in range(2):
        for j in range(4):
            block = tgs.run(device, np.ascontiguousarray(scores[:, i, j]), window, outputs=("labels", "best", "margin"))
            for k, v in block.items():
                assert so.same(got[k][:, 32 * i:32 * i + 32, 32 * j:32 * j + 32], v), (k, i, j)


def edge_cases():
    # name, (B, C, h, w), size, window, stride
    return [("W 63", (1, 5, 3, 3), (9, 63), (6, 20), (3, 20)), ("W 64", (1, 5, 3, 3), (9, 64), (6, 20), (3, 20)),
            ("W 65", (2, 5, 3, 3), (9, 65), (6, 20), (3, 20)), ("odd W, two images", (2, 4, 2, 3), (7, 131), (5, 50), (2, 27)),
            ("H 4k + 1", (1, 6, 3, 2), (13, 40), (8, 16), (4, 8)), ("H 4k + 3", (2, 6, 3, 2), (11, 40), (8, 16), (4, 8)),
            # window borders at rows 5, 10, 11, ... and columns 70, 77, 140, ...: inside tiles of 4 rows x 64 columns
            ("borders inside tiles", (1, 7, 4, 5), (23, 200), (11, 77), (5, 70)),
            # a grid cell a pixel: footprints of 9 x 75 cells in four windows, staged eight prompts at a time (21 = 8 + 8 + 5)
            ("large footprints", (1, 21, 6, 40), (9, 70), (6, 40), (3, 30)),
            ("one pixel windows", (1, 3, 1, 1), (3, 5), (1, 1), (1, 1)),
            ("one row", (1, 4, 2, 3), (1, 90), (1, 40), (1, 25)), ("one column", (1, 4, 3, 2), (30, 1), (12, 1), (5, 1)),
            # one window a pixel, 16 windows a tile row (the most the staged path holds an axis) and 22 (the direct path)
            ("16 windows a tile", (1, 5, 2, 2), (8, 80), (4, 4), (4, 4)), ("22 windows a tile", (1, 5, 2, 2), (8, 80), (4, 3), (4, 3)),
            # 5 x 5 = 25 windows on a pixel (four regular ones and the shifted last an axis): the direct path, no upper limit
            ("25 a pixel", (1, 5, 2, 2), (17, 71), (8, 8), (2, 2))]


@pytest.mark.parametrize("name,shape,size,window,stride", edge_cases(), ids=[c[0] for c in edge_cases()])
def test_tile_and_window_edges(device, name: str, shape, size, window, stride) -> None:
    b, c, h, w = shape
    scores = random_scores(b, c, h, w, size, window, stride, seed=sum(shape) + size[1])
    ref = swo.label_map_windows_ref(scores, size, window, stride)
    check(run(device, scores, size, window, stride), ref)
    if name == "odd W, two images":  # a label pointer off the dword grid: no packed store may straddle the guard
        check(run(device, scores, size, window, stride, label_shift=1), ref)
        check(run(device, scores, size, window, stride, label_shift=3, outputs=("labels",)), ref)
    if name == "25 a pixel":
        most = np.multiply.outer(swo.cover(size[0], window[0], stride[0]), swo.cover(size[1], window[1], stride[1])).max()
        assert most == 25


@pytest.mark.parametrize("which", ["1", "chunk", "chunk + 1", "150", "1024"])
def test_prompt_counts(device, which: str) -> None:
    _, _, chunk = segmentation.label_map_geometry()
    c = {"1": 1, "chunk": chunk, "chunk + 1": chunk + 1, "150": 150, "1024": 1024}[which]
    size, window, stride = (9, 70), (6, 40), (3, 30)  # 2 x 2 windows, all four on the pixels of rows 3 - 5, columns 30 - 39
    scores = random_scores(1, c, 3, 3, size, window, stride, seed=c)
    classes = np.arange(c) % 250 if c > 255 else None
    check(run(device, scores, size, window, stride, class_of=classes),
          swo.label_map_windows_ref(scores, size, window, stride, class_of=classes))


def test_leading_dimension(device) -> None:
    _, _, scores, size, window, stride, ref = case(1)
    check(run(device, scores, size, window, stride, pad=3), ref)  # ldc = 12: 16-byte rows
    check(run(device, scores, size, window, stride, pad=1), ref)  # ldc = 10: rows off the 16-byte grid
    _, _, scores, size, window, stride, ref = case(0)  # the direct path
    check(run(device, scores, size, window, stride, pad=2), ref)


def test_null_outputs_and_batch_independence(device) -> None:
    size, window, stride = (21, 75), (12, 40), (6, 20)
    scores = random_scores(3, 7, 3, 4, size, window, stride, seed=33)
    classes = [0, 0, 1, 2, 2, 3, 4]
    ref = swo.label_map_windows_ref(scores, size, window, stride, class_of=classes, min_score=0.0)
    for outputs in (("labels",), ("best",), ("labels", "margin"), ("best", "counts"), OUTPUTS):
        check(run(device, scores, size, window, stride, class_of=classes, min_score=0.0, outputs=outputs), ref)
    run(device, scores, size, window, stride, outputs=("margin", "counts"), expect=_lib.ISC_ERR_INVALID_ARG)
    for i in range(3):
        one = run(device, scores[i:i + 1], size, window, stride, class_of=classes, min_score=0.0)
        check(one, {k: v[i:i + 1] for k, v in ref.items()})


def test_a_grid_finer_than_the_window(device) -> None:
    """12 x 12 cells on 6 x 5 pixels: a downscale, and a tile row meets 13 windows of 144 cells each -- too many to stage."""
    size, window, stride = (14, 66), (6, 5), (4, 5)
    scores = random_scores(1, 6, 12, 12, size, window, stride, seed=12)
    check(run(device, scores, size, window, stride), swo.label_map_windows_ref(scores, size, window, stride))


def test_nan_and_infinite_cells(device) -> None:
    size, window, stride = (16, 80), (8, 40), (4, 20)  # 3 x 3 windows, up to 2 x 2 on a pixel
    scores = random_scores(1, 4, 4, 5, size, window, stride, seed=21)
    scores[0, 1, 1, 2, 2, :] = np.nan  # a cell of the centre window, NaN for every prompt
    got = run(device, scores, size, window, stride)
    ref = swo.label_map_windows_ref(scores, size, window, stride)
    check(got, ref)
    # exactly the pixels whose taps in the centre window touch the cell are NaN, overlap or not: it poisons the sum
    alone = so.upsampled(scores[:, 1, 1], window)[0, :, :, 0]
    touched = np.zeros(size, dtype=bool)
    touched[4:12, 20:60] = np.isnan(alone)
    assert touched.any() and not touched[4:12, 20:60].all()
    assert np.array_equal(np.isnan(got["best"][0]), touched) and np.array_equal(got["labels"][0] == 255, touched)
    assert (swo.cover(16, 8, 4)[4:12] == 2).all()  # every such pixel lies in other windows too
    # +inf in one window and -inf in another over the same pixels: NaN; where only one of them reaches, the infinity
    # (or NaN again where a tap of weight zero meets it, at the window's clamped borders)
    scores = random_scores(1, 4, 4, 5, size, window, stride, seed=22)
    scores[0, 0, 0, :, :, 1] = np.inf
    scores[0, 0, 1, :, :, 1] = -np.inf
    got = run(device, scores, size, window, stride)
    ref = swo.label_map_windows_ref(scores, size, window, stride)
    check(got, ref)
    v = swo.averaged(scores, size, window, stride)[0, :, :, 1]
    assert np.isnan(v[:4, 20:40]).all() and np.isposinf(v[1:4, 4:20]).all() and np.isneginf(v[1:4, 40:60]).all()
    assert (got["labels"][0][np.isposinf(v)] == 1).all() and (got["labels"][0, :4, 20:60] != 1).all()
    assert np.isposinf(got["best"][0][np.isposinf(v)]).all()


def test_classes_threshold_and_counts(device) -> None:
    _, _, scores, size, window, stride, ref = case(1)
    scores = scores.copy()
    scores[..., 4] = scores[..., 1]  # prompts 1 and 4 are twins
    got = run(device, scores, size, window, stride)
    check(got, swo.label_map_windows_ref(scores, size, window, stride))
    assert not (got["labels"] == 4).any() and (got["labels"] == 1).any()
    assert (got["margin"][got["labels"] == 1] == 0).all()
    classes = [0, 1, 2, 3, 1, 4, 5, 6, 7]  # one class: the margin looks past the twin
    got = run(device, scores, size, window, stride, class_of=classes)
    plain = swo.label_map_windows_ref(scores, size, window, stride, class_of=classes)
    check(got, plain)
    assert (got["margin"][got["labels"] == 1] > 0).all()
    # the threshold is strict: a pixel whose best equals min_score stays labeled; best and margin are written either way
    pivot = float(np.sort(plain["best"].ravel())[plain["best"].size // 2])
    got = run(device, scores, size, window, stride, class_of=classes, min_score=pivot)
    check(got, swo.label_map_windows_ref(scores, size, window, stride, class_of=classes, min_score=pivot))
    at = plain["best"] == F32(pivot)
    assert at.any() and (got["labels"][at] != 255).all() and (got["labels"][plain["best"] < F32(pivot)] == 255).all()
    assert so.same(got["best"], plain["best"]) and so.same(got["margin"], plain["margin"])
    # counts: a histogram of the labels that sums to H * W an image, from zero on a second call into the same buffer
    _, _, scores, size, window, stride, _ = case(0)
    b = scores.shape[0]
    sd = torch.from_numpy(scores).to(device)
    labels = torch.empty((b, *size), dtype=torch.uint8, device=device)
    counts = torch.full((b, 256), 12345, dtype=torch.int32, device=device)
    for _ in range(2):
        st = _lib.load().isc_label_map_windows(sd.data_ptr(), b, *scores.shape[3:], scores.shape[5], None, *size, *window,
                                               *stride, 0.1, labels.data_ptr(), None, None, counts.data_ptr(),
                                               _lib.stream_handle(device))
        assert st == 0
        for i in range(b):
            assert torch.equal(counts[i].long().cpu(), torch.bincount(labels[i].flatten().long().cpu(), minlength=256))
        assert counts.sum(dim=1).tolist() == [size[0] * size[1]] * b and int(counts[:, 255].sum()) > 0


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_matches_the_oracle(device) -> None:
    m, t, _, size, window, stride, _ = case(0)
    md, td = torch.from_numpy(m).to(device), torch.from_numpy(t).to(device)
    n, e, h, w = m.shape
    ny, nx = grid_of(size, window, stride)
    want_scores = so.class_scores_ref(m.reshape(n, e, h * w), t).reshape(n // (ny * nx), ny, nx, h, w, -1)
    classes = [0, 0, 1, 2, 2, 3, 3]
    ref = swo.label_map_windows_ref(want_scores, size, window, stride, class_of=classes, min_score=0.05)
    scores = segmentation.class_scores(md, td)
    out = segmentation.label_map_windows(scores, size, window, stride, class_of=classes, min_score=0.05,
                                         return_margin=True, return_counts=True)
    check({"labels": out.labels.cpu().numpy(), "best": out.scores.cpu().numpy(), "margin": out.margins.cpu().numpy(),
           "counts": out.counts.cpu().numpy()}, ref)
    assert out.indices is None and len(out) == n // (ny * nx)
    six = segmentation.label_map_windows(scores.reshape(-1, ny, nx, h, w, len(classes)), size, window, stride,
                                         class_of=torch.tensor(classes), min_score=0.05)
    assert torch.equal(six.labels, out.labels) and torch.equal(six.scores, out.scores) and six.margins is None
    seg = segmentation.segment_windows(md, td, size, window, stride, class_of=classes, min_score=0.05)
    assert torch.equal(seg.labels, out.labels) and torch.equal(seg.scores, out.scores)
    # an oversized window is clamped to the image: one window, label_map's own answer
    one = segmentation.label_map_windows(scores[:2], size, 1000, class_of=classes)
    plain = segmentation.label_map(scores[:2], size, class_of=classes)
    assert torch.equal(one.labels, plain.labels) and torch.equal(one.scores, plain.scores)
    empty = segmentation.label_map_windows(scores[:0], size, window, stride)
    assert empty.labels.shape == (0, *size)


def test_segment_windows_is_capturable(device) -> None:
    """One chain (score kernel, zeroing of the counts, label kernel) captured once and replayed on new inputs written in
    place, as tests/test_gpu_segment.py does for `segment`."""
    m, t, _, size, window, stride, _ = case(1)
    td = torch.from_numpy(t).to(device)
    inputs = [torch.from_numpy(m).to(device)] + [torch.nn.functional.normalize(
        torch.from_numpy(randn(m.shape, seed=50 + k)), dim=1).to(device) for k in range(2)]
    kw = dict(min_score=0.05, return_margin=True, return_counts=True)
    eager = [segmentation.segment_windows(x, td, size, window, stride, **kw) for x in inputs]
    static = inputs[0].clone()
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        segmentation.segment_windows(static, td, size, window, stride, **kw)  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = segmentation.segment_windows(static, td, size, window, stride, **kw)
    for k in (1, 2, 0):
        static.copy_(inputs[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((out.labels, eager[k].labels), (out.scores, eager[k].scores),
                          (out.margins, eager[k].margins), (out.counts, eager[k].counts)):
            assert so.same(got.cpu().numpy(), want.cpu().numpy())
    assert not torch.equal(eager[0].labels, eager[1].labels)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_dense_clip_sliding_windows(device, monkeypatch) -> None:
    from imagescry_amd import ImageBatch

    model, cfg = tgs._clip_model(monkeypatch, device, output="patches", dense="kk")
    batch = ImageBatch(indices=torch.tensor([11, 4]), images=co.model_images(2, 96, 128, seed=5)).to(device)
    ids, _ = co.text_ids(5, 12, cfg.text.vocab, seed=6)
    q = model.encode_text(ids)
    classes = [0, 0, 1, 2, 2]
    size, window, stride = (96, 128), (64, 64), (32, 32)
    out = model.segment(batch, q, class_of=classes, window=64, stride=32, return_margin=True, return_counts=True)
    assert out.labels.shape == (2, 96, 128) and out.indices.tolist() == [11, 4]
    crops = segmentation.crop_windows(batch.images, 64, 32)
    ny, nx = grid_of(size, window, stride)
    assert crops.shape == (2 * ny * nx, 3, 64, 64) and (ny, nx) == (2, 3)
    maps = model.predict_step(ImageBatch(indices=torch.arange(len(crops), device=device), images=crops)).embeddings
    maps = maps.cpu().numpy()  # the GPU's own map of the crops
    n, e, h, w = maps.shape
    scores = so.class_scores_ref(maps.reshape(n, e, h * w), q.cpu().numpy()).reshape(2, ny, nx, h, w, 5)
    check({"labels": out.labels.cpu().numpy(), "best": out.scores.cpu().numpy(), "margin": out.margins.cpu().numpy(),
           "counts": out.counts.cpu().numpy()}, swo.label_map_windows_ref(scores, size, window, stride, class_of=classes))
    same = model.segment(batch, q, class_of=classes, window=64, size=(96, 128))  # the default stride; the batch's own size
    assert torch.equal(same.labels, out.labels) and torch.equal(same.scores, out.scores)
    with pytest.raises(ValueError, match="size"):
        model.segment(batch, q, window=64, size=(48, 64))
    # without a window nothing has changed
    whole = model.segment(batch, q, class_of=classes, window=None)
    plain = segmentation.segment(model.predict_step(batch), q, (96, 128), class_of=classes)
    assert torch.equal(whole.labels, plain.labels) and torch.equal(whole.scores, plain.scores)
    assert whole.indices.tolist() == [11, 4] and not torch.equal(whole.labels, out.labels)
