"""The antialiased bicubic resize + centre crop on the GPU (isc_resize_aa, `resize_antialias`, `resize_center_crop`) and
the `preprocess="checkpoint"` mode of `CLIPEmbedder` / `DINOv2Embedder`.

Tolerances.  Against the float64 oracle (tests/preprocess_oracle.py) the kernel has to lie inside `aa_image_bound`, the
proven worst case of a float32 evaluation (a few 1e-2 of 255 levels; torch's own float32 kernel is two orders of
magnitude inside it, a kernel without antialiasing or with the crop one row off two or more orders outside:
tests/test_preprocess_aa_host.py).  Everything else is bit for bit: the crop against the slice of the full result, an
image against itself in a larger batch, the fused normalisation against `normalize_per_channel`, a graph replay against
an eager call.  With `quantize` every element has to be one of the levels rint(clamp(v)) of the values v within the
bound of the float64 result -- one level, or two where that result is within the bound of a half."""

from __future__ import annotations

import dataclasses
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_oracle as co  # noqa: E402
from dinov2_oracle import aa_axis_weights  # noqa: E402
from preprocess_oracle import SHAPES, aa_image_bound, random_u8, resize_aa_f64  # noqa: E402

pytestmark = pytest.mark.gpu


def _geometry(shape, size, crop_size):
    from imagescry_amd.transforms import center_crop_geometry

    return center_crop_geometry(*shape, size, crop_size)


def _reference(x: torch.Tensor, out, crop) -> torch.Tensor:
    top, left, hc, wc = crop
    return resize_aa_f64(x, *out)[..., top : top + hc, left : left + wc]


# ------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("as_float", [False, True], ids=["uint8", "float32"])
@pytest.mark.parametrize("shape,size,crop_size", SHAPES)
def test_kernel_matches_oracle_within_the_bound(device, shape, size, crop_size, as_float):
    from imagescry_amd import resize_center_crop

    out, crop = _geometry(shape, size, crop_size)
    x = random_u8((2, 3, *shape), 11 + shape[0] * 1000 + shape[1])
    xin = x.float() if as_float else x
    got = resize_center_crop(xin.to(device), size, crop_size).cpu()
    assert got.shape == (2, 3, crop[2], crop[3]) and got.dtype == torch.float32
    err = (got.double() - _reference(x, out, crop)).abs().max().item()
    bound = aa_image_bound(*shape, *out)
    print(f"{shape} -> {out} crop {crop}: max error {err:.2e}, bound {bound:.2e}")
    assert err <= bound


# even whole scales take the kernel's bank-padded staging: with the 64-column tile (scale 2) and with a narrower one
# (scale 32 on a 2048-pixel row); (50, 700) -> 23 columns is a narrower tile without the padding
@pytest.mark.parametrize("shape,out", [((64, 96), (32, 48)), ((8, 2048), (4, 64)), ((50, 700), (25, 23))])
def test_kernel_variants_match_oracle_within_the_bound(device, shape, out):
    from imagescry_amd import resize_antialias

    x = random_u8((1, 2, *shape), 12 + shape[1])
    for xin in (x, x.float()):
        got = resize_antialias(xin.to(device), out).cpu()
        err = (got.double() - resize_aa_f64(x, *out)).abs().max().item()
        bound = aa_image_bound(*shape, *out)
        print(f"{shape} -> {out}: max error {err:.2e}, bound {bound:.2e}")
        assert err <= bound


def test_identity_size_returns_the_input(device):
    from imagescry_amd import resize_antialias

    x = random_u8((2, 3, 37, 53), 5)
    assert torch.equal(resize_antialias(x.to(device), (37, 53)).cpu(), x.float())  # at s = 1 the weights are 0 and 1
    xf = torch.randn(1, 2, 19, 70, generator=torch.Generator().manual_seed(6))
    assert torch.equal(resize_antialias(xf.to(device), (19, 70)).cpu(), xf)
    assert resize_antialias(x[0, 0].to(device), (37, 53)).shape == (37, 53)  # 2-D in, 2-D out
    assert resize_antialias(x[:0].to(device), (20, 20)).shape == (0, 3, 20, 20)  # an empty batch: no launch


# ------------------------------------------------------------------------------------------------- independence
# (input, resized, crop): the issue's case, and one whose rectangle starts and ends off every band (up to 32 rows) and
# tile (up to 64 columns) boundary of the full call, with several bands and tiles of its own
CROPS = [((70, 45), (49, 32), (8, 0, 32, 32)), ((150, 230), (100, 170), (5, 7, 77, 141))]


@pytest.mark.parametrize("shape,out,crop", CROPS)
def test_crop_equals_the_slice_of_the_full_result(device, shape, out, crop):
    from imagescry_amd import resize_antialias

    top, left, hc, wc = crop
    x = random_u8((2, 3, *shape), 21).to(device)
    full = resize_antialias(x, out)
    part = resize_antialias(x, out, crop=crop)
    assert torch.equal(part, full[:, :, top : top + hc, left : left + wc])
    assert (full.cpu().double() - resize_aa_f64(x.cpu(), *out)).abs().max().item() <= aa_image_bound(*shape, *out)
    # nothing outside the support of the crop rectangle matters: overwrite it
    rows, cols = aa_axis_weights(shape[0], out[0]), aa_axis_weights(shape[1], out[1])
    r0, r1 = rows[top][0], rows[top + hc - 1][0] + len(rows[top + hc - 1][1])
    c0, c1 = cols[left][0], cols[left + wc - 1][0] + len(cols[left + wc - 1][1])
    assert (r0, c0) != (0, 0) or (r1, c1) != shape
    noise = random_u8((2, 3, *shape), 22).to(device)
    noise[:, :, r0:r1, c0:c1] = x[:, :, r0:r1, c0:c1]
    assert torch.equal(resize_antialias(noise, out, crop=crop), part)


def test_image_in_a_batch_equals_the_image_alone(device):
    from imagescry_amd import resize_center_crop

    x = random_u8((5, 3, 70, 45), 31).to(device)
    batch = resize_center_crop(x, 32, 28)
    assert torch.equal(batch[3], resize_center_crop(x[3:4], 32, 28)[0])
    assert torch.equal(batch[3, 1], resize_center_crop(x[3, 1], 32, 28))  # one plane, 2-D


def test_unaligned_uint8_rows(device):
    """Rows of an odd width start at every byte offset; so does an image inside a larger buffer."""
    from imagescry_amd import resize_antialias

    x = random_u8((2, 3, 41, 67), 41)
    want = resize_antialias(x.to(device), (17, 29), crop=(2, 3, 13, 22))
    flat = torch.zeros(x.numel() + 3, dtype=torch.uint8, device=device)
    for off in (1, 2, 3):
        view = flat[off : off + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 4 == (flat.data_ptr() + off) % 4
        assert torch.equal(resize_antialias(view, (17, 29), crop=(2, 3, 13, 22)), want)


def test_more_planes_than_one_launch_holds(device):
    from imagescry_amd import resize_antialias

    b = 23334  # x 3 channels = 70 002 planes
    x = random_u8((b, 3, 9, 8), 51)
    got = resize_antialias(x.to(device), (4, 4)).cpu()
    assert got.shape == (b, 3, 4, 4)
    picks = torch.cat([torch.tensor([0, 3 * b - 1]),
                       torch.randint(0, 3 * b, (100,), generator=torch.Generator().manual_seed(52))])
    want = resize_aa_f64(x.reshape(3 * b, 9, 8)[picks], 4, 4)
    err = (got.reshape(3 * b, 4, 4)[picks].double() - want).abs().max().item()
    bound = aa_image_bound(9, 8, 4, 4)
    print(f"70 002 planes, 102 checked: max error {err:.2e}, bound {bound:.2e}")
    assert err <= bound


# ----------------------------------------------------------------------------------------------------- epilogue
def _stats(device):
    from imagescry_amd import clip

    mean = torch.tensor(clip.IMAGE_MEAN, device=device) * 255.0
    std = torch.tensor(clip.IMAGE_STD, device=device) * 255.0
    return mean, std


@pytest.mark.parametrize("quantize", [False, True])
def test_fused_normalisation_equals_normalize_per_channel(device, quantize):
    from imagescry_amd import normalize_per_channel, resize_antialias

    mean, std = _stats(device)
    x = random_u8((2, 3, 70, 45), 61).to(device)
    plain = resize_antialias(x, (49, 32), crop=(8, 0, 32, 32), quantize=quantize)
    want = normalize_per_channel(plain, channel_means=mean.reshape(1, 3, 1, 1), channel_stds=std.reshape(1, 3, 1, 1),
                                 eps=0.0)
    for m, s in ((mean, std), (mean.reshape(1, 3, 1, 1), std.reshape(1, 3, 1, 1))):
        got = resize_antialias(x, (49, 32), crop=(8, 0, 32, 32), channel_means=m, channel_stds=s, quantize=quantize)
        assert torch.equal(got, want)
    with pytest.raises(ValueError):
        resize_antialias(x, (49, 32), channel_means=mean)  # both or neither
    with pytest.raises(ValueError):
        resize_antialias(x, (49, 32), crop=(18, 0, 32, 32))  # outside the resized image


@pytest.mark.parametrize("shape,size,crop_size", [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_quantize_gives_the_allowed_uint8_levels(device, shape, size, crop_size):
    from imagescry_amd import resize_center_crop

    out, crop = _geometry(shape, size, crop_size)
    x = random_u8((2, 3, *shape), 71)
    x[0, 0, : shape[0] // 2] = 255 * (torch.arange(shape[1]) % 2).to(torch.uint8)  # overshoot below 0 and above 255
    got = resize_center_crop(x.to(device), size, crop_size, quantize=True).cpu().double()
    ref = _reference(x, out, crop)
    bound = aa_image_bound(*shape, *out)
    assert torch.equal(got, got.round()) and got.min().item() >= 0 and got.max().item() <= 255
    lo = torch.round((ref - bound).clamp(0, 255))  # torch.round and rint both round half to even
    hi = torch.round((ref + bound).clamp(0, 255))
    two = (lo != hi).double().mean().item()
    print(f"{shape} -> {out}: {100 * two:.2f} % of the elements may take either of two levels; "
          f"float64 range [{ref.min().item():.1f}, {ref.max().item():.1f}]")
    assert bool(((got >= lo) & (got <= hi)).all())
    assert bool((hi - lo <= 1).all())


# -------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_equals_an_eager_call(device):
    from imagescry_amd import resize_center_crop

    mean, std = _stats(device)
    x = random_u8((3, 3, 70, 45), 81).to(device)
    new = random_u8((3, 3, 70, 45), 82).to(device)

    def run():
        return resize_center_crop(x, 32, 28, channel_means=mean, channel_stds=std, quantize=True)

    run()  # warm-up: the library is loaded outside the capture
    torch.cuda.synchronize(device)
    stream = torch.cuda.Stream(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = run()
    x.copy_(new)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(out, resize_center_crop(new, 32, 28, channel_means=mean, channel_stds=std, quantize=True))


# ---------------------------------------------------------------------------------------------------- embedders
def _clip_model(monkeypatch, device, **kw):
    from imagescry_amd import CLIPEmbedder, clip

    cfg, sd = co.shallow("ViT-B/32")
    monkeypatch.setitem(clip.PRESETS, "ViT-B/32", cfg)
    return CLIPEmbedder("ViT-B/32", state_dict=sd, **kw).to(device)


def _dino_model(monkeypatch, device, **kw):
    from imagescry_amd import DINOv2Embedder, embedding, vit

    cfg = dataclasses.replace(embedding.DINOV2_PRESETS["vits14", True], depth=2)
    monkeypatch.setitem(embedding.DINOV2_PRESETS, ("vits14", True), cfg)
    sd = vit.make_state_dict(cfg, seed=9, randomize_affine=True)
    return DINOv2Embedder("vits14", True, state_dict=sd, grid="aspect", **kw).to(device)


@pytest.mark.parametrize("family", ["clip", "dinov2"])
def test_checkpoint_preprocess_of_the_embedders(device, monkeypatch, family):
    from imagescry_amd import ImageBatch, clip, l2_normalize_channels, resize_center_crop, vit

    if family == "clip":
        model = _clip_model(monkeypatch, device, preprocess="checkpoint")
        size, crop, mean, std = 224, 224, clip.IMAGE_MEAN, clip.IMAGE_STD
    else:
        model = _dino_model(monkeypatch, device, preprocess="checkpoint", crop_size=70)
        size, crop, mean, std = 80, 70, vit.IMAGENET_MEAN, vit.IMAGENET_STD
    assert (model.resize_size, model.crop_size) == (size, crop)
    images = co.model_images(2, 70, 45, 91).to(device)
    x = model.preprocess(images)
    want = resize_center_crop(images, size, crop, quantize=True,
                              channel_means=torch.tensor([255.0 * v for v in mean], device=device),
                              channel_stds=torch.tensor([255.0 * v for v in std], device=device))
    assert x.shape == (2, 3, crop, crop) and torch.equal(x, want)
    got = model.predict_step(ImageBatch(images=images, indices=torch.arange(2, device=device))).embeddings
    assert torch.equal(got, l2_normalize_channels(model.forward(x)))
    with pytest.raises(TypeError):
        model.preprocess(images.float())


@pytest.mark.parametrize("family", ["clip", "dinov2"])
def test_squash_preprocess_is_the_earlier_path(device, monkeypatch, family):
    from imagescry_amd import clip, normalize_per_channel, resize, vit

    images = co.model_images(2, 70, 45, 92).to(device)
    if family == "clip":
        model = _clip_model(monkeypatch, device)
        mean, std = ((torch.tensor(v, device=device) * 255.0).reshape(1, 3, 1, 1) for v in (clip.IMAGE_MEAN, clip.IMAGE_STD))
        want = normalize_per_channel(resize(images, output_size=(224, 224)), channel_means=mean, channel_stds=std, eps=0.0)
    else:
        model = _dino_model(monkeypatch, device, max_patches=24)
        h, w = vit.token_grid(70, 45, 24)
        want = normalize_per_channel(resize(images, output_size=(14 * h, 14 * w)), min_value=-3, max_value=3)
    assert model.preprocess_mode == "squash" and "preprocess" not in model.hparams
    assert torch.equal(model.preprocess(images), want)
