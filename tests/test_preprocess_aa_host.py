"""Host side of the checkpoint-faithful preprocessing: the float64 oracle of the antialiased resize
(tests/preprocess_oracle.py) against torch, the proven float32 bound, the output-size and crop-offset rule of
`resize_center_crop`, and the `preprocess=` / `crop_size=` / `resize_size=` arguments of the two embedders.  CPU only.

What the bound separates, random uint8 images, (H1, W1) -> resize / crop (`test_bound_holds_for_torch_float32` and
`test_wrong_kernels_miss_the_bound` print the figures):

    shape                    torch f32 max error   bound     no antialiasing   crop one row off
    (45, 70)   -> 32 / 28    4e-4                  5.0e-2    108               >= 150
    (70, 45)   -> 32 / 32    4e-4                  5.0e-2    108               >= 150
    (20, 13)   -> 28 / 28    3e-4                  2.8e-2    21                >= 150
    (33, 33)   -> 28 / 28    5e-4                  4.1e-2    64                >= 150
"""

from __future__ import annotations

import dataclasses
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_oracle as co  # noqa: E402
from preprocess_oracle import SHAPES, aa_image_bound, random_u8, resize_aa_f64  # noqa: E402
from imagescry_amd import CLIPEmbedder, DINOv2Embedder, ViTB16Embedder, clip, embedding, vit  # noqa: E402
from imagescry_amd.transforms import center_crop_geometry  # noqa: E402


def _case(shape, size, crop_size, seed=0):
    (h2, w2), crop = center_crop_geometry(*shape, size, crop_size)
    x = random_u8((2, 3, *shape), seed + shape[0] * 1000 + shape[1])
    return x, h2, w2, crop


@pytest.mark.parametrize("shape,size,crop_size", SHAPES)
def test_oracle_equals_torch_float64(shape, size, crop_size):
    x, h2, w2, _ = _case(shape, size, crop_size)
    want = F.interpolate(x.double(), size=(h2, w2), mode="bicubic", antialias=True, align_corners=False)
    err = (resize_aa_f64(x, h2, w2) - want).abs().max().item()
    print(f"{shape} -> ({h2}, {w2}): restated vs torch float64 {err:.1e}")
    assert err < 1e-10


@pytest.mark.parametrize("shape,size,crop_size", SHAPES)
def test_bound_holds_for_torch_float32(shape, size, crop_size):
    x, h2, w2, _ = _case(shape, size, crop_size)
    got = F.interpolate(x.float(), size=(h2, w2), mode="bicubic", antialias=True, align_corners=False)
    err = (got.double() - resize_aa_f64(x, h2, w2)).abs().max().item()
    bound = aa_image_bound(*shape, h2, w2)
    print(f"{shape} -> ({h2}, {w2}): torch float32 max error {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    assert bound < 0.5  # far below one uint8 level: the bound can tell a wrong kernel from a right one


@pytest.mark.parametrize("shape,size,crop_size", SHAPES)
def test_wrong_kernels_miss_the_bound(shape, size, crop_size):
    x, h2, w2, (top, left, hc, wc) = _case(shape, size, crop_size)
    ref = resize_aa_f64(x, h2, w2)
    bound = aa_image_bound(*shape, h2, w2)
    plain = F.interpolate(x.double(), size=(h2, w2), mode="bicubic", antialias=False, align_corners=False)
    shifted = ref.roll(1, dims=-2)
    e_plain, e_shift = (plain - ref).abs().max().item(), (shifted - ref).abs().max().item()
    print(f"{shape} -> ({h2}, {w2}): bound {bound:.2e}, without antialiasing {e_plain:.3g}, one row off {e_shift:.3g}")
    assert e_shift > 100 * bound
    if max(shape[0] / h2, shape[1] / w2) > 1.0:  # at an exact upscale the two filters differ only in A
        assert e_plain > 100 * bound


def test_geometry_rule():
    # shorter side -> size, longer -> int(size * long / short); offsets int(round(margin / 2.0)), round half to even
    assert center_crop_geometry(500, 375, 256, 224) == ((341, 256), (58, 16, 224, 224))  # 341.33 -> 341, 117 / 2 -> 58
    assert center_crop_geometry(375, 500, 256, 224) == ((256, 341), (16, 58, 224, 224))
    assert center_crop_geometry(45, 70, 32, 28) == ((32, 49), (2, 10, 28, 28))  # 49.78 -> 49, margin 21 -> 10
    assert center_crop_geometry(70, 45, 32, 32) == ((49, 32), (8, 0, 32, 32))   # margin 17 -> 8
    assert center_crop_geometry(448, 470, 14, 14) == ((14, 14), (0, 0, 14, 14))  # 14.69 -> 14
    assert center_crop_geometry(40, 40, 40) == ((40, 40), (0, 0, 40, 40))  # crop_size defaults to size
    # margins of 1, 3 and 5 pixels: offsets 0, 2 and 2 (CenterCrop's rule), where margin // 2 gives 0, 1 and 2
    for margin, offset in ((1, 0), (3, 2), (5, 2), (2, 1), (7, 4)):
        assert center_crop_geometry(31, 40, 28 + margin, 28)[1][0] == offset
        assert center_crop_geometry(40, 31, 28 + margin, 28)[1][1] == offset
    assert center_crop_geometry(31, 40, 31, 28) == ((31, 40), (2, 6, 28, 28))
    assert center_crop_geometry(31, 40, 31, (31, 10)) == ((31, 40), (0, 15, 31, 10))  # a rectangular crop
    for bad in ((31, 40, 31, 32), (31, 40, 31, (28, 41)), (0, 40, 31, 28), (31, 40, 0, None), (31, 40, 31, 0)):
        with pytest.raises(ValueError):
            center_crop_geometry(*bad)


# ------------------------------------------------------------------------------------------------- the embedders
@pytest.fixture()
def shallow(monkeypatch):
    """Depth 1 presets: the constructors draw every weight."""
    for key, cfg in list(embedding.DINOV2_PRESETS.items()):
        monkeypatch.setitem(embedding.DINOV2_PRESETS, key, dataclasses.replace(cfg, depth=1))
    cfg, sd = co.shallow("ViT-B/32")
    monkeypatch.setitem(clip.PRESETS, "ViT-B/32", cfg)
    return sd


def test_dinov2_preprocess_arguments(shallow):
    plain = DINOv2Embedder("vits14")
    assert plain.preprocess_mode == "squash" and plain.crop_size is None and plain.resize_size is None
    assert plain.hparams == {"image_size": 518, "patch_size": 14, "depth": 1, "variant": "vits14", "registers": False}
    assert DINOv2Embedder("vits14", preprocess="squash").hparams == plain.hparams
    m = DINOv2Embedder("vits14", preprocess="checkpoint")  # fixed grid: the native 518, resized from round(518 * 8 / 7)
    assert (m.crop_size, m.resize_size) == (518, 592)
    assert m.hparams == {**plain.hparams, "preprocess": "checkpoint", "crop_size": 518, "resize_size": 592}
    m = DINOv2Embedder("vits14", True, preprocess="checkpoint", grid="aspect", output="patches")
    assert (m.crop_size, m.resize_size) == (224, 256)  # the published evaluation transform
    m = DINOv2Embedder("vits14", preprocess="checkpoint", grid="aspect", crop_size=70)
    assert (m.crop_size, m.resize_size) == (70, 80)
    m = DINOv2Embedder("vits14", preprocess="checkpoint", grid="aspect", crop_size=70, resize_size=70)
    assert (m.crop_size, m.resize_size) == (70, 70)
    for kw in (dict(crop_size=224), dict(resize_size=256), dict(preprocess="squash", crop_size=518),
               dict(preprocess="pil"),
               dict(preprocess="checkpoint", crop_size=224),  # a fixed grid takes 518 only
               dict(preprocess="checkpoint", grid="aspect", crop_size=225),  # no multiple of the patch size
               dict(preprocess="checkpoint", grid="aspect", max_patches=16, crop_size=70),  # 25 patches > 16
               dict(preprocess="checkpoint", grid="aspect", crop_size=70, resize_size=64),  # would need padding
               dict(preprocess="checkpoint", grid="aspect", crop_size=0),
               dict(preprocess="checkpoint", grid="aspect", crop_size=70.0)):
        with pytest.raises(ValueError):
            DINOv2Embedder("vits14", **kw)


def test_clip_preprocess_arguments(shallow):
    plain = CLIPEmbedder("ViT-B/32", state_dict=shallow)
    assert plain.preprocess_mode == "squash" and plain.crop_size is None and plain.resize_size is None
    assert set(plain.hparams) == {"image_size", "patch_size", "depth", "act", "embed_dim", "preset"}
    m = CLIPEmbedder("ViT-B/32", state_dict=shallow, preprocess="checkpoint")
    assert (m.crop_size, m.resize_size) == (224, 224)  # shorter side to image_size, centre square
    assert m.hparams == {**plain.hparams, "preprocess": "checkpoint", "crop_size": 224, "resize_size": 224}
    m = CLIPEmbedder("ViT-B/32", state_dict=shallow, preprocess="checkpoint", grid="aspect", crop_size=96)
    assert (m.crop_size, m.resize_size) == (96, 96)
    m = CLIPEmbedder("ViT-B/32", state_dict=shallow, preprocess="checkpoint", resize_size=256)
    assert (m.crop_size, m.resize_size) == (224, 256)
    for kw in (dict(crop_size=224), dict(resize_size=224), dict(preprocess="center"),
               dict(preprocess="checkpoint", crop_size=96),  # a fixed grid takes image_size only
               dict(preprocess="checkpoint", grid="aspect", crop_size=100),
               dict(preprocess="checkpoint", resize_size=200)):
        with pytest.raises(ValueError):
            CLIPEmbedder("ViT-B/32", state_dict=shallow, **kw)


def test_vit_b16_embedder_has_no_preprocess_argument():
    with pytest.raises(TypeError):
        ViTB16Embedder(config=dataclasses.replace(vit.VIT_B16, depth=1), preprocess="checkpoint")
    assert vit.IMAGENET_MEAN == (0.485, 0.456, 0.406) and vit.IMAGENET_STD == (0.229, 0.224, 0.225)
