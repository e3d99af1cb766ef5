"""Host side of the long ViT token grids (more than 196 patches): `vit.token_grid` at large caps, the `max_patches`
argument of `ViTB16Embedder`, `vit.images_per_pass`, and the two C-ABI entries of the streaming attention kernel.  No
device is touched."""

from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

from imagescry_amd import ViTB16Embedder, _lib, vit
from imagescry_amd.vit import MAX_PATCHES, images_per_pass  # noqa: F401  (the module is about these)

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
SMALL = vit.ViTConfig(dim=128, depth=1, heads=2, mlp_dim=256)


@pytest.mark.parametrize("m", [400, 784, 1024, 4096])
def test_token_grid_at_large_caps(m: int) -> None:
    side = int(round(m**0.5))
    assert side * side == m <= MAX_PATCHES
    assert vit.token_grid(640, 640, m) == (side, side)  # a square image gets the square grid
    for hh, ww in ((300, 500), (500, 300), (480, 640), (1, 5000), (5000, 1), (1080, 1920), (33, 35)):
        h, w = vit.token_grid(hh, ww, m)
        assert h >= 1 and w >= 1 and h * w <= m, (hh, ww, h, w)
        assert (h >= w) == (hh >= ww) or h == w


def test_max_patches_is_validated_in_the_constructor() -> None:
    assert vit.MAX_PATCHES == 4096
    for bad in (0, -1, vit.MAX_PATCHES + 1):
        with pytest.raises(ValueError, match="max_patches"):
            ViTB16Embedder(config=SMALL, grid="aspect", max_patches=bad)
    with pytest.raises(ValueError, match="max_patches"):
        ViTB16Embedder(config=SMALL, grid="fixed", max_patches=400)
    with pytest.raises(ValueError, match="max_patches"):
        ViTB16Embedder(config=SMALL, max_patches=196)  # the default grid is the fixed one
    m = ViTB16Embedder(config=SMALL, output="patches", grid="aspect", max_patches=vit.MAX_PATCHES)
    assert m.hparams["max_patches"] == vit.MAX_PATCHES and m.max_patches == vit.MAX_PATCHES


def test_hparams_record_max_patches_only_when_set() -> None:
    assert "max_patches" not in ViTB16Embedder(config=SMALL).hparams
    assert "max_patches" not in ViTB16Embedder(config=SMALL, output="patches", grid="aspect").hparams
    m = ViTB16Embedder(config=SMALL, output="patches", grid="aspect", max_patches=400)
    assert m.hparams == {"image_size": 224, "patch_size": 16, "depth": 1, "output": "patches", "grid": "aspect",
                         "max_patches": 400}


def test_the_default_still_refuses_more_than_196_patches_before_any_device() -> None:
    m = ViTB16Embedder(config=SMALL, output="patches", grid="aspect")
    with pytest.raises(ValueError, match="h w <= 196"):
        m.forward(torch.zeros(1, 3, 240, 224))  # 15 x 14 = 210 patches, a CPU tensor: the shape is refused first
    net = vit.prepare(vit.make_state_dict(SMALL, seed=0), SMALL)
    for fn in (vit.forward_cls, vit.forward_tokens):
        with pytest.raises(ValueError, match=r"1 \.\. 196 patches"):
            fn(net, torch.zeros(1, 3, 240, 224), (15, 14))
        with pytest.raises(ValueError, match=r"1 \.\. 200 patches"):
            fn(net, torch.zeros(1, 3, 240, 224), (15, 14), max_patches=200)
    long = ViTB16Embedder(config=SMALL, output="patches", grid="aspect", max_patches=400)
    with pytest.raises(ValueError, match="h w <= 400"):
        long.forward(torch.zeros(1, 3, 16 * 21, 16 * 20))
    with pytest.raises(_lib.HipLibraryError):  # 210 patches pass the shape check now; a CPU tensor does not
        long.forward(torch.zeros(1, 3, 240, 224))


def test_preprocess_follows_max_patches() -> None:
    m = ViTB16Embedder(config=SMALL, output="patches", grid="aspect", max_patches=784)
    assert vit.token_grid(300, 500, 784) == (22, 35)
    assert vit.token_grid(320, 320, 400) == (20, 20)
    assert m._patch_cap == 784 and ViTB16Embedder(config=SMALL, grid="aspect")._patch_cap == 196


def test_images_per_pass() -> None:
    for tokens in (2, 50, 197, 224):
        for n in (1, 7, 1024, 5000):
            assert vit.images_per_pass(tokens, n) == n  # the native grids keep their pass size
    for tokens in (225, 401, 577, 785, 1025, 4097, 1024 * 197, 1024 * 197 + 1, 10**7):
        for n in (1, 2, 7, 1024, 5000):
            got = vit.images_per_pass(tokens, n)
            assert 1 <= got <= n
            assert got == max(1, min(n, (1024 * 197) // tokens))
            assert got * tokens <= 1024 * 197 or got == 1
    assert vit.images_per_pass(401, 1024) == 503 and vit.images_per_pass(1025, 1024) == 196


def test_the_new_entries_are_declared_and_bound() -> None:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, nargs in (("isc_attention_f16_stream", 8), ("isc_attention_stream_geometry", 2)):
        proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S)
        assert proto is not None, name
        assert len(proto.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    assert _lib.SIGNATURES["isc_attention_f16_stream"] == _lib.SIGNATURES["isc_attention_f16"]
    assert _lib.ISC_ABI_VERSION == 4  # entries were added, none changed
