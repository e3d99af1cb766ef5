"""isc_label_map and isc_map_class_scores on the GPU against tests/segment_oracle.py (which tests/test_segment_host.py
checks on the CPU), value for value: labels, best, margin and counts must equal the oracle's (`so.same`: equal values
and signs of zero, a NaN equal to a NaN).  The kernels are called through the C ABI into the interior of buffers filled
with a pattern, whose guard bytes must survive; the Python layer, graph capture, the dense CLIP map and the bank path
follow.  The shapes aim at the kernel's own constants (`isc_label_map_geometry`)."""

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

from imagescry_amd import _lib, segmentation  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 256  # bytes on either side of an output
FILL = 0xA5  # float32 0xA5A5A5A5 = -2.9e-16, int32 negative, label 165: wrong wherever it survives
OUTPUTS = ("labels", "best", "margin", "counts")
TILE = (64, 4)  # isc_label_map_geometry, needed before a library can be asked (test ids); test_shapes checks it


class Guarded:
    """`nbytes` inside a uint8 buffer of FILL; `shift` moves the interior off the buffer's alignment by that many bytes."""

    def __init__(self, nbytes: int, dtype: type, device: torch.device, shift: int = 0) -> None:
        self.lo, self.hi = GUARD + shift, GUARD + shift + nbytes
        self.buf = torch.full((self.hi + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.dtype = dtype
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.lo

    def numpy(self, shape: tuple[int, ...]) -> np.ndarray:
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[:self.lo] == FILL).all(), "bytes before the output were written"
        assert (raw[self.hi:] == FILL).all(), "bytes after the output were written"
        return raw[self.lo:self.hi].copy().view(self.dtype).reshape(shape)


NP_DTYPE = {"labels": np.uint8, "best": np.float32, "margin": np.float32, "counts": np.int32}


def run(device: torch.device, scores: np.ndarray, size: tuple[int, int], class_of=None, min_score: float = -math.inf,
        outputs: tuple[str, ...] = OUTPUTS, pad: int = 0, label_shift: int = 0, expect: int = 0) -> dict[str, np.ndarray]:
    """isc_label_map on float32 [B, h, w, C] `scores`; `pad` extra floats of 1e30 behind every cell's prompts (ldc = C +
    pad).  Returns the outputs asked for, read back from guarded buffers."""
    b, h, w, c = scores.shape
    big_h, big_w = size
    src = np.full((b, h, w, c + pad), F32(1e30), dtype=F32)
    src[..., :c] = scores
    sd = torch.from_numpy(src).to(device)
    cd = None if class_of is None else torch.tensor(np.asarray(class_of), dtype=torch.int32, device=device)
    shapes = {"labels": (b, big_h, big_w), "best": (b, big_h, big_w), "margin": (b, big_h, big_w), "counts": (b, 256)}
    bufs = {k: Guarded(int(np.prod(shapes[k])) * np.dtype(NP_DTYPE[k]).itemsize, NP_DTYPE[k], device,
                       label_shift if k == "labels" else 0) for k in outputs}
    st = _lib.load().isc_label_map(sd.data_ptr(), b, h, w, c, c + pad, _lib.ptr(cd), big_h, big_w, min_score,
                                   *(bufs[k].ptr if k in bufs else None for k in OUTPUTS), _lib.stream_handle(device))
    assert st == expect, _lib.strerror(st)
    return {k: bufs[k].numpy(shapes[k]) for k in outputs}


def check(got: dict[str, np.ndarray], want: dict[str, np.ndarray]) -> None:
    for k, v in got.items():
        assert so.same(v, want[k]), f"{k} differs from the oracle at {int((v != want[k]).sum())} places"


def randn(shape: tuple[int, ...], seed: int) -> np.ndarray:
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).numpy()


@functools.lru_cache(maxsize=None)
def case(i: int):
    m, t, scores, size = so.case_inputs(i)
    return m, t, scores, size, so.label_map_ref(scores, size)


def geometry() -> tuple[int, int, int]:
    return segmentation.label_map_geometry()


# -------------------------------------------------------------------------------------------------------- isc_label_map
@pytest.mark.parametrize("i", range(len(so.CASES)))
def test_cases_equal_the_oracle(device, i: int) -> None:
    _, _, scores, size, ref = case(i)
    check(run(device, scores, size), ref)


def shape_cases() -> list[tuple[str, tuple[int, int, int, int], tuple[int, int]]]:
    tw, th = TILE
    return [("downscale", (1, 9, 11, 5), (4, 6)), ("identity", (1, 6, 6, 4), (6, 6)), ("one cell", (2, 1, 1, 3), (5, 7)),
            ("one row", (1, 3, 3, 4), (1, 20)), ("one column", (1, 3, 3, 4), (20, 1)), ("one pixel", (1, 3, 2, 4), (1, 1)),
            ("ragged quads", (2, 4, 4, 3), (9, 13)), ("one tile", (1, 5, 7, 3), (th, tw)),
            ("tile + 1", (1, 5, 7, 3), (th + 1, tw + 1)),
            # a footprint of 65 x 5 cells: the prompt chunk shrinks to 20 to fit the staging buffer (37 prompts: 20 + 17)
            ("wide footprint", (1, 9, 70, 37), (9, 70)),
            # a steep downscale: the footprint does not fit at any chunk and the cells are read from memory
            ("steep downscale", (1, 40, 300, 5), (3, 5)), ("mild downscale", (1, 20, 150, 6), (9, 70))]


@pytest.mark.parametrize("name,shape,size", shape_cases(), ids=[c[0] for c in shape_cases()])
def test_shapes(device, name: str, shape, size) -> None:
    assert geometry()[:2] == TILE, "shape_cases() is aimed at TILE: change it with the kernel's tile"
    scores = randn(shape, seed=sum(shape) + size[0])
    classes = None if shape[3] < 30 else np.arange(shape[3]) % 11
    ref = so.label_map_ref(scores, size, class_of=classes)
    check(run(device, scores, size, class_of=classes), ref)
    if name == "identity":
        assert np.array_equal(ref["labels"], scores.argmax(axis=-1))
    if name == "ragged quads":  # a label pointer off the dword grid: no packed store may straddle the guard
        check(run(device, scores, size, label_shift=1), ref)
        check(run(device, scores, size, label_shift=3, outputs=("labels",)), ref)


@pytest.mark.parametrize("which", ["1", "chunk", "chunk + 1", "1024"])
def test_prompt_counts(device, which: str) -> None:
    _, _, chunk = geometry()
    c = {"1": 1, "chunk": chunk, "chunk + 1": chunk + 1, "1024": 1024}[which]
    scores = randn((1, 3, 3, c), seed=c)
    classes = np.arange(c) % 250 if c > 255 else None
    check(run(device, scores, (20, 20), class_of=classes), so.label_map_ref(scores, (20, 20), class_of=classes))


def test_leading_dimension(device) -> None:
    _, _, scores, size, ref = case(0)
    check(run(device, scores, size, pad=5), ref)  # ldc = 12: 16-byte rows
    check(run(device, scores, size, pad=2), ref)  # ldc = 9: rows off the 16-byte grid


def test_ties_and_classes(device) -> None:
    scores = randn((1, 4, 5, 6), seed=9)
    scores[..., 4] = scores[..., 1]  # prompts 1 and 4 are the same column
    size = (19, 23)
    got = run(device, scores, size)
    check(got, so.label_map_ref(scores, size))
    assert not (got["labels"] == 4).any() and (got["labels"] == 1).any()  # the lower prompt wins the tie
    assert (got["margin"][got["labels"] == 1] == 0).all()  # ... and its twin is the runner-up
    classes = [0, 1, 2, 3, 1, 4]  # now the twins are one class: the margin looks past it
    got = run(device, scores, size, class_of=classes)
    check(got, so.label_map_ref(scores, size, class_of=classes))
    assert (got["margin"][got["labels"] == 1] > 0).all()
    got = run(device, scores, size, class_of=[7] * 6)  # a single class
    check(got, so.label_map_ref(scores, size, class_of=[7] * 6))
    assert (got["labels"] == 7).all() and np.isposinf(got["margin"]).all() and got["counts"][0, 7] == 19 * 23
    flat = np.full((1, 4, 5, 6), F32(0.25), dtype=F32)  # an all-equal map
    got = run(device, flat, size)
    check(got, so.label_map_ref(flat, size))
    assert (got["labels"] == 0).all() and (got["margin"] == 0).all()


def test_nan_and_infinite_cells(device) -> None:
    scores = randn((1, 5, 5, 4), seed=21)
    scores[0, 1, 1, :] = np.nan  # a cell that is NaN for every prompt
    scores[0, 3, 3, 2] = np.nan  # a cell that is NaN for one prompt
    scores[0, 0, 4, :] = -np.inf  # a cell no prompt scores
    scores[0, 4, 0, 1] = np.inf
    size = (40, 40)
    got = run(device, scores, size)
    ref = so.label_map_ref(scores, size)
    check(got, ref)
    v = so.upsampled(scores, size)
    all_nan = np.isnan(v).all(axis=-1)
    assert all_nan.any() and not all_nan.all()
    assert ((got["labels"] == 255) == all_nan).all()  # unlabeled only where every prompt is NaN
    one_nan = np.isnan(v[..., 2]) & ~all_nan
    assert one_nan.any() and (got["labels"][one_nan] != 2).all()  # a NaN prompt loses to any number
    assert np.isneginf(got["best"]).any() and np.isposinf(got["best"]).any()
    # with a finite threshold the pixels around the unscored cell are unlabeled too
    got = run(device, scores, size, min_score=-1e30)
    check(got, so.label_map_ref(scores, size, min_score=-1e30))
    assert (got["labels"][np.isneginf(got["best"])] == 255).all()


def test_threshold_is_strict(device) -> None:
    _, _, scores, size, ref = case(3)
    pivot = float(np.sort(ref["best"].ravel())[ref["best"].size // 2])
    got = run(device, scores, size, min_score=pivot)
    check(got, so.label_map_ref(scores, size, min_score=pivot))
    at = ref["best"] == F32(pivot)
    assert at.any() and (got["labels"][at] != 255).all() and (got["labels"][ref["best"] < F32(pivot)] == 255).all()
    assert so.same(got["best"], ref["best"]) and so.same(got["margin"], ref["margin"])  # written as computed either way


def test_counts_are_a_histogram_and_start_from_zero(device) -> None:
    _, _, scores, size, ref = case(0)
    b, big = scores.shape[0], size[0] * size[1]
    sd = torch.from_numpy(scores).to(device)
    labels = torch.empty((b, *size), dtype=torch.uint8, device=device)
    counts = torch.full((b, 256), 12345, dtype=torch.int32, device=device)
    for _ in range(2):  # the second call into the same buffer does not double it
        st = _lib.load().isc_label_map(sd.data_ptr(), b, *scores.shape[1:], scores.shape[3], None, *size, 0.1,
                                       labels.data_ptr(), None, None, counts.data_ptr(), _lib.stream_handle(device))
        assert st == 0
        for i in range(b):
            assert torch.equal(counts[i].long().cpu(), torch.bincount(labels[i].flatten().long().cpu(), minlength=256))
        assert counts.sum(dim=1).tolist() == [big] * b and int(counts[:, 255].sum()) > 0


def test_null_outputs_and_batch_independence(device) -> None:
    scores = randn((3, 5, 4, 7), seed=33)
    size = (37, 29)
    ref = so.label_map_ref(scores, size, class_of=[0, 0, 1, 2, 2, 3, 4], min_score=0.0)
    for outputs in (("labels",), ("best",), ("labels", "best"), ("labels", "margin"), ("best", "counts"),
                    ("labels", "best", "margin", "counts")):
        check(run(device, scores, size, class_of=[0, 0, 1, 2, 2, 3, 4], min_score=0.0, outputs=outputs), ref)
    run(device, scores, size, outputs=("margin", "counts"), expect=_lib.ISC_ERR_INVALID_ARG)  # neither labels nor best
    for i in range(3):
        one = run(device, scores[i:i + 1], size, class_of=[0, 0, 1, 2, 2, 3, 4], min_score=0.0)
        check(one, {k: v[i:i + 1] for k, v in ref.items()})


# ------------------------------------------------------------------------------------------------- isc_map_class_scores
def test_class_scores_equal_the_float64_chain(device) -> None:
    lib = _lib.load()
    for e in (1, 5, 64, 513):
        for s in (1, 49, 50):
            for c in (1, 7, 65):
                m = randn((2, e, s), seed=e + s + c)
                t = randn((c, e), seed=e * s + c)
                if c > 1:
                    t[1] = 0.0  # a zero vector scores 0, not NaN
                md, td = torch.from_numpy(m).to(device), torch.from_numpy(t).to(device)
                for pad in (0, 3):
                    out = Guarded(2 * s * (c + pad) * 4, np.float32, device)
                    st = lib.isc_map_class_scores(md.data_ptr(), 2, e, s, td.data_ptr(), c, e, out.ptr, c + pad,
                                                  _lib.stream_handle(device))
                    assert st == 0
                    got = out.numpy((2, s, c + pad))
                    assert so.same(got[..., :c], so.class_scores_ref(m, t)), (e, s, c, pad)
                    assert (got[..., c:].view(np.uint32) == 0xA5A5A5A5).all()  # the padding of a row is not written
                    if c > 1:
                        assert (got[..., 1] == 0).all()


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_matches_the_oracle(device) -> None:
    m, t, _, size, _ = case(0)
    md, td = torch.from_numpy(m).to(device), torch.from_numpy(t).to(device)
    b, e, h, w = m.shape
    scores = segmentation.class_scores(md, td)
    want_scores = so.class_scores_ref(m.reshape(b, e, h * w), t).reshape(b, h, w, -1)
    assert so.same(scores.cpu().numpy(), want_scores)
    classes = [0, 0, 1, 2, 2, 3, 3]
    ref = so.label_map_ref(want_scores, size, class_of=classes, min_score=0.05)
    out = segmentation.label_map(scores, size, class_of=classes, min_score=0.05, return_margin=True, return_counts=True)
    check({"labels": out.labels.cpu().numpy(), "best": out.scores.cpu().numpy(), "margin": out.margins.cpu().numpy(),
           "counts": out.counts.cpu().numpy()}, ref)
    assert out.indices is None and out.device == device and len(out) == b
    # "bchw" is the same map permuted; the defaults return labels and scores only
    chw = segmentation.label_map(scores.permute(0, 3, 1, 2).contiguous(), size, layout="bchw", class_of=torch.tensor(classes),
                                 min_score=0.05)
    assert torch.equal(chw.labels, out.labels) and torch.equal(chw.scores, out.scores)
    assert chw.margins is None and chw.counts is None
    assert segmentation.label_map(scores, size, return_scores=False).scores is None
    seg = segmentation.segment(md, td, size, class_of=classes, min_score=0.05)
    assert torch.equal(seg.labels, out.labels) and torch.equal(seg.scores, out.scores)
    host = out.cpu()
    assert host.device.type == "cpu" and torch.equal(host.labels, out.labels.cpu())
    empty = segmentation.label_map(scores[:0], size)
    assert empty.labels.shape == (0, *size)
    with pytest.raises(ValueError, match="vectors on"):
        segmentation.class_scores(md, td.cpu())


def test_segment_is_capturable(device) -> None:
    """One chain (score kernel, zeroing of the counts, label kernel) captured once and replayed on new inputs written in place."""
    m, t, _, size, _ = case(0)
    td = torch.from_numpy(t).to(device)
    inputs = [torch.from_numpy(m).to(device)] + [torch.nn.functional.normalize(
        torch.from_numpy(randn(m.shape, seed=50 + k)), dim=1).to(device) for k in range(2)]
    eager = [segmentation.segment(x, td, size, min_score=0.05, return_margin=True, return_counts=True) for x in inputs]
    static = inputs[0].clone()
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        segmentation.segment(static, td, size, min_score=0.05, return_margin=True, return_counts=True)  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = segmentation.segment(static, td, size, min_score=0.05, return_margin=True, return_counts=True)
    for k in (1, 2, 0):
        static.copy_(inputs[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((out.labels, eager[k].labels), (out.scores, eager[k].scores),
                          (out.margins, eager[k].margins), (out.counts, eager[k].counts)):
            assert so.same(got.cpu().numpy(), want.cpu().numpy())
    assert not torch.equal(eager[0].labels, eager[1].labels)


# ------------------------------------------------------------------------------------------------------------ end to end
def _clip_model(monkeypatch, device, **kw):
    from imagescry_amd import CLIPEmbedder, clip

    cfg, sd = co.shallow("ViT-B/32")
    monkeypatch.setitem(clip.PRESETS, "ViT-B/32", cfg)
    return CLIPEmbedder("ViT-B/32", state_dict=sd, **kw).to(device), cfg


def test_dense_clip_map_to_pixel_labels(device, monkeypatch) -> None:
    from imagescry_amd import ImageBatch

    model, cfg = _clip_model(monkeypatch, device, output="patches", dense="kk")
    batch = ImageBatch(indices=torch.tensor([11, 4]), images=co.model_images(2, 96, 128, seed=5)).to(device)
    ids, _ = co.text_ids(5, 12, cfg.text.vocab, seed=6)
    q = model.encode_text(ids)
    classes = [0, 0, 1, 2, 2]
    out = model.segment(batch, q, class_of=classes, return_margin=True, return_counts=True)
    assert out.labels.shape == (2, 96, 128) and out.indices.tolist() == [11, 4]
    maps = model.predict_step(batch).embeddings.cpu().numpy()  # the GPU's own map
    b, e, h, w = maps.shape
    scores = so.class_scores_ref(maps.reshape(b, e, h * w), q.cpu().numpy()).reshape(b, h, w, 5)
    check({"labels": out.labels.cpu().numpy(), "best": out.scores.cpu().numpy(), "margin": out.margins.cpu().numpy(),
           "counts": out.counts.cpu().numpy()}, so.label_map_ref(scores, (96, 128), class_of=classes))
    assert set(np.unique(out.labels.cpu().numpy())) <= {0, 1, 2}
    half = model.segment(batch, q, class_of=classes, size=(48, 64))
    assert so.same(half.labels.cpu().numpy(), so.label_map_ref(scores, (48, 64), class_of=classes)["labels"])


def test_clip_embedder_refusals(device, monkeypatch) -> None:
    from imagescry_amd import ImageBatch

    batch = ImageBatch(indices=torch.arange(1), images=co.model_images(1, 64, 64, seed=1)).to(device)
    model, cfg = _clip_model(monkeypatch, device)
    q = torch.zeros(2, cfg.embed_dim, device=device)
    with pytest.raises(ValueError, match="dense"):
        model.segment(batch, q)
    model, _ = _clip_model(monkeypatch, device, output="patches", dense="kk", preprocess="checkpoint")
    with pytest.raises(ValueError, match="checkpoint"):
        model.segment(batch, q)


def test_bank_label_map(device) -> None:
    from imagescry_amd import EmbeddingBank

    # image 5: a 3 x 4 grid without its cell (1, 2); image 8: one cell
    cells = [(5, i, j) for i in range(3) for j in range(4) if (i, j) != (1, 2)] + [(8, 0, 0)]
    origin = torch.tensor(cells)
    rows = torch.nn.functional.normalize(torch.from_numpy(randn((len(cells), 32), seed=77)), dim=1)
    bank = EmbeddingBank(rows.to(device), dtype=torch.float32, normalize=False, row_groups=origin[:, 0].to(device))
    bank.row_origin = origin
    q = torch.nn.functional.normalize(torch.from_numpy(randn((4, 32), seed=78)), dim=1).to(device)
    size = (30, 40)
    kw = dict(min_score=-1.0, return_margin=True, return_counts=True)
    got = bank.label_map(q, 5, size, **kw)
    want = segmentation.label_map(bank.similarity_map(q, 5)[None], size, layout="bchw", **kw)
    for a, b in ((got.labels, want.labels), (got.scores, want.scores), (got.margins, want.margins),
                 (got.counts, want.counts)):
        assert so.same(a.cpu().numpy(), b.cpu().numpy())
    assert got.labels.shape == (1, *size)
    sim = bank.similarity_map(q, 5).permute(1, 2, 0).contiguous().cpu().numpy()[None]
    ref = so.label_map_ref(sim, size, min_score=-1.0)
    assert so.same(got.labels.cpu().numpy(), ref["labels"]) and so.same(got.scores.cpu().numpy(), ref["best"])
    hole = np.isnan(ref["best"]) | np.isneginf(ref["best"])
    assert hole.any() and (ref["labels"][hole] == 255).all() and (ref["labels"][~hole] != 255).all()
    plain = bank.label_map(q, 5, size)  # the defaults
    assert torch.equal(plain.labels, segmentation.label_map(bank.similarity_map(q, 5)[None], size, layout="bchw").labels)
