"""Host side of the ViT patch-token maps: the token-grid rule, the constructor surface, and the token oracle
(tests/vit_tokens_oracle.py) against an independent implementation -- `transformers.ViTModel` run with
`interpolate_pos_encoding=True` on the same weights.  CPU only."""

from __future__ import annotations

import random
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from imagescry_amd import ViTB16Embedder, vit  # noqa: E402
from oracle.vit_oracle import to_transformers_state_dict, vit_forward  # noqa: E402
from vit_tokens_oracle import interpolate_pos_embed, vit_tokens  # noqa: E402


@pytest.mark.parametrize("shape,want", [((224, 224), (14, 14)), ((37, 37), (14, 14)), ((100, 160), (11, 17)),
                                        ((300, 200), (17, 11)), ((1, 1000), (1, 196)), ((1000, 1), (196, 1))])
def test_token_grid_cases(shape, want):
    assert vit.token_grid(*shape, 196) == want
    assert vit.token_grid(*shape) == want  # ViT-B/16's 196 patches are the default


def test_token_grid_never_exceeds_the_patch_budget():
    rng = random.Random(20)
    for _ in range(5000):
        hh, ww = rng.randint(1, 4000), rng.randint(1, 4000)
        mp = rng.choice([1, 2, 16, 49, 196, 196, 196, 223])
        h, w = vit.token_grid(hh, ww, mp)
        assert h >= 1 and w >= 1 and h * w <= mp, (hh, ww, mp, h, w)
        assert vit.token_grid(hh, ww, mp) == (h, w)  # one shape, one grid
    assert "token_grid" in vit.__all__
    with pytest.raises(ValueError):
        vit.token_grid(0, 5)


def test_constructor_arguments():
    cfg = vit.ViTConfig(depth=1)
    default = ViTB16Embedder(config=cfg)
    assert (default.output, default.grid) == ("cls", "fixed")
    assert default.hparams == {"image_size": 224, "patch_size": 16, "depth": 1}  # unchanged for the default mode
    m = ViTB16Embedder(config=cfg, output="patches", grid="aspect")
    assert (m.output, m.grid, m.embedding_dim) == ("patches", "aspect", 768)
    with pytest.raises(ValueError):
        ViTB16Embedder(config=cfg, output="tokens")
    with pytest.raises(ValueError):
        ViTB16Embedder(config=cfg, grid="free")
    # shapes are refused before anything touches a device
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 16 * 15, 16 * 14))  # 210 patches
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 100, 160))  # not a multiple of the patch size
    with pytest.raises(ValueError):
        ViTB16Embedder(config=cfg, output="patches").forward(torch.zeros(1, 3, 176, 272))  # fixed grid: 224 x 224 only


def test_position_cache_belongs_to_the_prepared_net():
    cfg = vit.ViTConfig(depth=1)
    a = vit.prepare(vit.make_state_dict(cfg), cfg)
    b = vit.prepare(vit.make_state_dict(cfg), cfg)
    assert a.pos_cache is not b.pos_cache and a.to(torch.device("cpu")).pos_cache is not a.pos_cache
    assert vit.position_table(a, (14, 14)) is a.pos_embed and not a.pos_cache  # the native grid: no launch, no entry


def test_interpolated_table_is_the_identity_on_the_native_grid():
    pos = torch.randn(1, 197, 8, generator=torch.Generator().manual_seed(0))
    assert interpolate_pos_embed(pos, (14, 14)) is pos
    out = interpolate_pos_embed(pos, (11, 17))
    assert out.shape == (1, 188, 8) and torch.equal(out[:, 0], pos[:, 0])


@pytest.mark.parametrize("grid", [(11, 17), (14, 14)])
def test_token_oracle_matches_transformers(grid):
    transformers = pytest.importorskip("transformers")
    cfg = vit.ViTConfig(depth=2)
    sd = vit.make_state_dict(cfg, seed=5, randomize_affine=True)
    hf_cfg = transformers.ViTConfig(num_hidden_layers=cfg.depth, layer_norm_eps=cfg.ln_eps)
    model = transformers.ViTModel(hf_cfg, add_pooling_layer=False).eval()
    hf_sd = to_transformers_state_dict(sd, list(model.state_dict().keys()))
    assert set(hf_sd) == set(model.state_dict().keys())
    model.load_state_dict(hf_sd)
    x = torch.randn(2, 3, 16 * grid[0], 16 * grid[1], generator=torch.Generator().manual_seed(1)).clamp(-3, 3)
    with torch.no_grad():
        want = model(pixel_values=x, interpolate_pos_encoding=True).last_hidden_state
        got = vit_tokens(sd, x, eps=cfg.ln_eps)
    assert got.shape == (2, grid[0] * grid[1] + 1, 768)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)  # the tolerance of tests/test_oracle_vit.py
    if grid == (14, 14):
        with torch.no_grad():
            assert torch.equal(got[:, 0], vit_forward(sd, x, eps=cfg.ln_eps))  # the class-token oracle, bit for bit
