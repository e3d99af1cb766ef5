"""Sliding-window label maps without a GPU: the window grid of `segmentation.window_grid` and of the host-only C entry
`isc_label_map_window_grid` against a brute-force statement of its formula, the oracle of tests/segment_windows_oracle.py
against the torch composition it stands for, its two degenerate cases against tests/segment_oracle.py, and the refusals
of the Python layer and of the C ABI, which come before any launch.

Labels: the oracle and the composition (per window `F.interpolate`, a sum, a division by the count map) round in
different places; averaging up to 12 blends keeps both within about 1e-6 of the real value for |score| <= 1, so they must
agree at every pixel whose top-2 gap in torch's values is at least 1e-5, and at most 0.1 % of a case's pixels may fall
under that gap -- the rule of tests/test_segment_host.py."""

from __future__ import annotations

import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import segment_oracle as so  # noqa: E402
import segment_windows_oracle as swo  # noqa: E402

from imagescry_amd import EmbeddingBatch, _lib, segmentation  # noqa: E402

F32 = np.float32
GAP = 1e-5
MAX_LEFT_OUT = 1e-3
MAX_DIFF = 2e-6
OK, INVALID, UNSUPPORTED, ALIGNMENT = _lib.ISC_OK, _lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_ALIGNMENT
P = 4096  # a 16-byte aligned non-NULL address no call reaches


def c_grid(size, window, stride) -> tuple[int, int, int, int]:
    ny, nx, most = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    st = _lib.load().isc_label_map_window_grid(*size, *window, *stride, ny, nx, most)
    return st, ny.value, nx.value, most.value


# ------------------------------------------------------------------------------------------------------- the window grid
def test_window_grid_against_the_formula() -> None:
    for length in range(1, 41):
        for win in range(1, length + 1):
            for stride in range(1, win + 1):
                n = max(length - win + stride - 1, 0) // stride + 1
                want = [min(i * stride, length - win) for i in range(n)]
                ys, xs = segmentation.window_grid((length, 3), (win, 2), (stride, 1))
                assert ys == want and xs == [0, 1], (length, win, stride)
                assert len(set(want)) == n and want == sorted(want) and want[-1] + win == length
                count = [sum(s <= p < s + win for s in want) for p in range(length)]
                assert min(count) >= 1, (length, win, stride)  # every pixel is covered
                assert max(count) <= -(-win // stride) + 1, (length, win, stride)
                assert np.array_equal(swo.cover(length, win, stride), count)
                # the C entry agrees on the count and on the most windows over one pixel, on either axis
                assert c_grid((length, 1), (win, 1), (stride, 1)) == (OK, n, 1, max(count))
                assert c_grid((1, length), (1, win), (1, stride)) == (OK, 1, n, max(count))


def test_window_grid_in_two_dimensions_and_defaults() -> None:
    ys, xs = segmentation.window_grid((37, 53), (24, 20), (10, 8))
    assert ys == [0, 10, 13] and xs == [0, 8, 16, 24, 32, 33]
    cover = np.multiply.outer(swo.cover(37, 24, 10), swo.cover(53, 20, 8))
    assert cover.max() == 12 and c_grid((37, 53), (24, 20), (10, 8)) == (OK, 3, 6, 12)
    assert segmentation.window_grid((448, 448), 224) == ([0, 112, 224], [0, 112, 224])  # stride: half the window
    assert segmentation.window_grid((10, 10), (5, 3)) == ([0, 3, 5], [0, 2, 4, 6, 7])  # ... rounded up
    assert c_grid((448, 448), (224, 224), (112, 112)) == (OK, 3, 3, 4)
    assert segmentation.window_grid((30, 50), 64, 16) == ([0], [0])  # an oversized window is clamped to the image
    assert segmentation.window_grid((30, 50), (64, 20), (16, 16)) == ([0], [0, 16, 30])
    assert segmentation.window_grid((7, 7), 7, 7) == ([0], [0])


def test_crop_windows() -> None:
    images = torch.arange(2 * 3 * 9 * 11, dtype=torch.int64).reshape(2, 3, 9, 11).to(torch.uint8)
    crops = segmentation.crop_windows(images, (4, 5), (3, 4))
    ys, xs = segmentation.window_grid((9, 11), (4, 5), (3, 4))
    assert (ys, xs) == ([0, 3, 5], [0, 4, 6])
    assert crops.dtype == torch.uint8 and crops.shape == (2 * 9, 3, 4, 5)
    for b in range(2):
        for i, y in enumerate(ys):
            for j, x in enumerate(xs):
                assert torch.equal(crops[(b * 3 + i) * 3 + j], images[b, :, y:y + 4, x:x + 5])
    assert segmentation.crop_windows(images.float(), 100).shape == (2, 3, 9, 11)  # clamped: the image itself
    assert segmentation.crop_windows(images[:0], 4).shape == (0, 3, 4, 4)
    with pytest.raises(ValueError):
        segmentation.crop_windows(images[0], 4)
    with pytest.raises(TypeError):
        segmentation.crop_windows(images.numpy(), 4)


# ------------------------------------------------------------------------------------------------------------ the oracle
def torch_composition(scores: np.ndarray, size, window, stride) -> torch.Tensor:
    """[B, ny, nx, h, w, C] -> the averaged upsampled scores [B, C, H, W]."""
    ys, xs = swo.starts(size[0], window[0], stride[0]), swo.starts(size[1], window[1], stride[1])
    s = torch.from_numpy(scores)
    acc = torch.zeros(s.shape[0], s.shape[-1], *size)
    count = torch.zeros(size)
    for i, y in enumerate(ys):
        for j, x in enumerate(xs):
            acc[:, :, y:y + window[0], x:x + window[1]] += F.interpolate(
                s[:, i, j].permute(0, 3, 1, 2), size=window, mode="bilinear", align_corners=False)
            count[y:y + window[0], x:x + window[1]] += 1
    return acc / count


@pytest.mark.parametrize("i", range(len(swo.CASES)))
def test_oracle_labels_agree_with_torch(i: int) -> None:
    _, _, scores, size, window, stride = swo.case_inputs(i)
    ref = swo.label_map_windows_ref(scores, size, window, stride)
    up = torch_composition(scores, size, window, stride)
    top2 = up.topk(min(2, up.shape[1]), dim=1)
    gap = (top2.values[:, 0] - top2.values[:, 1]).numpy()
    clear = gap >= GAP
    left_out = 1.0 - clear.mean()
    diff = np.abs(swo.averaged(scores, size, window, stride) - up.permute(0, 2, 3, 1).numpy()).max()
    most = int(np.multiply.outer(swo.cover(size[0], window[0], stride[0]), swo.cover(size[1], window[1], stride[1])).max())
    print(f"case {i}: up to {most} windows a pixel, {100 * left_out:.3f} % of the pixels under the gap, "
          f"max |oracle - torch| = {diff:.2e}")
    if i == 0:
        assert most == 12
    assert left_out <= MAX_LEFT_OUT
    assert np.array_equal(ref["labels"][clear], top2.indices[:, 0].numpy()[clear])
    assert diff <= MAX_DIFF
    assert ref["labels"].max() < scores.shape[-1] and ref["counts"].sum() == scores.shape[0] * size[0] * size[1]
    assert np.abs(ref["best"] - up.max(dim=1).values.numpy()).max() <= MAX_DIFF


def test_a_single_window_is_the_label_map() -> None:
    _, _, scores, size = so.case_inputs(0)
    ref = so.label_map_ref(scores, size, class_of=[0, 0, 1, 2, 2, 3, 3], min_score=0.05)
    got = swo.label_map_windows_ref(scores[:, None, None], size, size, size, class_of=[0, 0, 1, 2, 2, 3, 3], min_score=0.05)
    for k in ref:
        assert so.same(got[k], ref[k]), k


def test_stride_equal_to_the_window_gives_label_map_blocks() -> None:
    _, _, scores, size, window, stride = swo.case_inputs(3)
    assert window == stride
    got = swo.label_map_windows_ref(scores, size, window, stride)
    ys, xs = swo.starts(size[0], window[0], stride[0]), swo.starts(size[1], window[1], stride[1])
    # W = 129: the last column of windows is shifted back onto the one before it; everywhere else a pixel has one window
    alone = np.multiply.outer(swo.cover(size[0], window[0], stride[0]), swo.cover(size[1], window[1], stride[1])) == 1
    assert xs[-2:] == [96, 97] and alone[:, :97].all() and alone[:, 128].all() and not alone[:, 97:128].any()
    for i, y in enumerate(ys):
        for j, x in enumerate(xs):
            block = so.label_map_ref(scores[:, i, j], window)
            own = alone[y:y + window[0], x:x + window[1]]
            for k in ("labels", "best", "margin"):
                assert so.same(got[k][:, y:y + window[0], x:x + window[1]][:, own], block[k][:, own]), (k, i, j)
    # and where the windows tile the image exactly, every pixel has one window
    scores = np.ascontiguousarray(scores[:, :, :4])
    got = swo.label_map_windows_ref(scores, (64, 128), window, stride)
    for i in range(2):
        for j in range(4):
            block = so.label_map_ref(scores[:, i, j], window)
            for k in ("labels", "best", "margin"):
                assert so.same(got[k][:, 32 * i:32 * i + 32, 32 * j:32 * j + 32], block[k]), (k, i, j)


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_label_map_windows_validation() -> None:
    s = torch.zeros(9, 2, 2, 3)  # 3 x 3 windows of one image: window 4, stride 2 over 8 x 8
    kw = dict(size=(8, 8), window=4, stride=2)
    for bad, exc in ((s.double(), TypeError), (s.numpy(), TypeError), (s[0], ValueError), (s[:8], ValueError),
                     (s.reshape(1, 3, 3, 2, 2, 3)[:, :2], ValueError), (torch.zeros(9, 2, 2, 0), ValueError),
                     (torch.zeros(9, 2, 2, 1025), ValueError), (torch.zeros(9, 0, 2, 3), ValueError)):
        with pytest.raises(exc):
            segmentation.label_map_windows(bad, **kw)
    for size, exc in (((8,), TypeError), ((8.0, 8), TypeError), ((0, 8), ValueError), (8, TypeError)):
        with pytest.raises(exc):
            segmentation.label_map_windows(s, size, 4, 2)
    for window, exc in ((4.0, TypeError), ((4, 4, 4), TypeError), ("4", TypeError), (True, TypeError), (0, ValueError),
                        ((4, -1), ValueError), (None, TypeError)):
        with pytest.raises(exc):
            segmentation.label_map_windows(s, (8, 8), window, 2)
    for stride, exc in ((2.0, TypeError), ((2,), TypeError), (0, ValueError), (5, ValueError), ((2, 5), ValueError)):
        with pytest.raises(exc):
            segmentation.label_map_windows(s, (8, 8), 4, stride)
    with pytest.raises(ValueError, match="stride"):
        segmentation.window_grid((8, 3), 4, 4)  # the window is clamped to 3 columns: a stride of 4 would leave a gap
    with pytest.raises(ValueError, match="NaN"):
        segmentation.label_map_windows(s, **kw, min_score=math.nan)
    with pytest.raises(TypeError):
        segmentation.label_map_windows(s, **kw, min_score="0")
    with pytest.raises(ValueError):
        segmentation.label_map_windows(s, **kw, class_of=[0, 1])
    with pytest.raises(TypeError):
        segmentation.label_map_windows(s, **kw, layout="bchw")
    # everything valid but the device: there is no CPU path.  Both layouts; the default stride; an oversized window
    for scores, args in ((s, ((8, 8), 4, 2)), (s.reshape(1, 3, 3, 2, 2, 3), ((8, 8), 4)), (s[:2], ((8, 8), (4, 100), (4, 8))),
                         (s[:1], ((8, 8), 100))):
        with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
            segmentation.label_map_windows(scores, *args, class_of=[0, 0, 254], min_score=0.5)


def test_segment_windows_validation() -> None:
    m, t = torch.zeros(9, 8, 2, 2), torch.zeros(5, 8)
    with pytest.raises(ValueError, match="stride"):
        segmentation.segment_windows(m, t, (8, 8), 4, 5)
    with pytest.raises(TypeError):
        segmentation.segment_windows(m.half(), t, (8, 8), 4, 2)
    with pytest.raises(ValueError):
        segmentation.segment_windows(m, torch.zeros(5, 7), (8, 8), 4, 2)
    with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
        segmentation.segment_windows(EmbeddingBatch(indices=torch.arange(9), embeddings=m), t, (8, 8), 4, 2)


def test_clip_embedder_window_refusals() -> None:
    from imagescry_amd import CLIPEmbedder, ImageBatch

    sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
    import clip_oracle as co

    cfg, sd = co.shallow("ViT-B/32")
    batch = ImageBatch(indices=torch.arange(1), images=torch.zeros(1, 3, 48, 64, dtype=torch.uint8))
    q = torch.zeros(2, cfg.embed_dim)
    with pytest.raises(ValueError, match="dense"):
        CLIPEmbedder(cfg, state_dict=sd).segment(batch, q, window=32)
    with pytest.raises(ValueError, match="checkpoint"):
        CLIPEmbedder(cfg, state_dict=sd, output="patches", dense="kk", preprocess="checkpoint").segment(batch, q, window=32)
    model = CLIPEmbedder(cfg, state_dict=sd, output="patches", dense="kk")
    with pytest.raises(ValueError, match="size"):
        model.segment(batch, q, window=32, size=(24, 32))
    with pytest.raises(ValueError, match="stride"):
        model.segment(batch, q, window=32, stride=33)
    with pytest.raises(ValueError, match="window"):
        model.segment(batch, q, stride=16)
    with pytest.raises(TypeError):
        model.segment(batch, q, window=32.0)


# --------------------------------------------------------------------------------------------------------------- the C ABI
def _windows(scores=P, b=1, h=2, w=2, c=3, ldc=3, class_of=None, big_h=8, big_w=8, win_h=4, win_w=4, stride_y=2,
             stride_x=2, min_score=-math.inf, labels=P, best=P, margin=None, counts=None) -> int:
    return _lib.load().isc_label_map_windows(scores, b, h, w, c, ldc, class_of, big_h, big_w, win_h, win_w, stride_y,
                                             stride_x, min_score, labels, best, margin, counts, None)


def test_c_abi_argument_checks_come_before_any_launch() -> None:
    """The pointers are never dereferenced: every check precedes the launch, and B = 0 launches nothing."""
    assert _windows(b=0) == OK
    assert _windows(b=0, scores=None, labels=None, best=None) == OK
    assert _windows(b=-1) == INVALID
    for kw in (dict(h=0), dict(w=0), dict(big_h=0), dict(big_w=0), dict(c=0), dict(ldc=2), dict(scores=None),
               dict(labels=None, best=None), dict(min_score=math.nan), dict(stride_y=0), dict(stride_x=0),
               dict(stride_x=-1), dict(stride_y=5), dict(stride_x=5), dict(win_h=9), dict(win_w=9), dict(win_h=0, stride_y=0),
               dict(win_w=0), dict(win_h=-4)):
        assert _windows(**kw) == INVALID, kw
    for kw in (dict(c=1025, ldc=1025), dict(h=65536, w=32768), dict(big_h=65536, big_w=32768), dict(b=65536),
               dict(big_h=4 * 65535 + 1)):
        assert _windows(**kw) == UNSUPPORTED, kw
    for kw in (dict(scores=P + 4), dict(best=P + 2), dict(margin=P + 1), dict(counts=P + 2), dict(class_of=P + 2)):
        assert _windows(**kw) == ALIGNMENT, kw
    assert _windows(b=0, c=1024, ldc=1024, big_h=4 * 65535, big_w=8192, win_h=4 * 65535, win_w=1, stride_x=1) == OK
    # the grid entry: the same geometry errors, and NULL results
    lib = _lib.load()
    n = ctypes.c_int()
    assert lib.isc_label_map_window_grid(8, 8, 4, 4, 2, 2, None, n, n) == INVALID
    assert lib.isc_label_map_window_grid(8, 8, 4, 4, 2, 2, n, None, n) == INVALID
    assert lib.isc_label_map_window_grid(8, 8, 4, 4, 2, 2, n, n, None) == INVALID
    for size, window, stride in (((8, 8), (9, 4), (2, 2)), ((8, 8), (4, 4), (5, 2)), ((8, 8), (4, 4), (2, 0)),
                                 ((0, 8), (4, 4), (2, 2)), ((8, 8), (4, 0), (2, 2))):
        assert c_grid(size, window, stride)[0] == INVALID, (size, window, stride)


def test_declared_bound_and_abi_unchanged() -> None:
    import re

    header = (Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in ("isc_label_map_windows", "isc_label_map_window_grid"):
        proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S)
        assert proto is not None, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name)
    assert lib.isc_abi_version() == _lib.ISC_ABI_VERSION == 4
