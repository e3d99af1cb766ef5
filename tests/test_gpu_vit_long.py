"""`ViTB16Embedder` on token grids of more than 196 patches (sequences beyond 224 tokens run on
isc_attention_f16_stream): aspect grids through `max_patches`, a fixed-grid config larger than 14 x 14, pass slicing and
the way into `EmbeddingBank` -- against the float32 torch restatement of tests/vit_tokens_oracle.py at the tolerances
tests/test_gpu_vit_tokens.py uses for this path (1e-2 to the float32 oracle, 2e-3 to the oracle with fp16-rounded
operands, unit norm to 1e-5).  A small net (dim 128, two blocks, two heads) keeps every case at seconds."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

from oracle import transforms_oracle  # noqa: E402
from vit_tokens_oracle import patch_map, vit_tokens  # noqa: E402

pytestmark = pytest.mark.gpu

NET = dict(dim=128, depth=2, heads=2, mlp_dim=256)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _images(batch: int, h: int, w: int, seed: int) -> torch.Tensor:
    return torch.randint(0, 256, (batch, 3, h, w), dtype=torch.uint8, generator=_gen(seed))


def _oracle(sd: dict, cfg, images: torch.Tensor, grid: tuple[int, int]) -> tuple[torch.Tensor, torch.Tensor]:
    h, w = grid
    resized = images if tuple(images.shape[-2:]) == (16 * h, 16 * w) else transforms_oracle.resize(images, (16 * h, 16 * w))
    x = transforms_oracle.normalize_per_channel(resized, min_value=-3, max_value=3)
    with torch.no_grad():
        tok = vit_tokens(sd, x, heads=cfg.heads, eps=cfg.ln_eps)
        tok16 = vit_tokens(sd, x, heads=cfg.heads, eps=cfg.ln_eps, round_operands_fp16=True)
    return tok, tok16


def _check_map(e: torch.Tensor, tok: torch.Tensor, tok16: torch.Tensor, grid: tuple[int, int], what: str) -> None:
    want, want16 = patch_map(tok, grid), patch_map(tok16, grid)
    err, err16 = (e - want).abs().max().item(), (e - want16).abs().max().item()
    cos = (e * want).sum(dim=1).min().item()
    print(f"{what}: max|err| f32 {err:.3e}, fp16-operand oracle {err16:.3e}, 1 - min cell cosine {1 - cos:.2e}")
    assert err < 1e-2
    assert err16 < 2e-3
    assert torch.allclose(e.norm(dim=1), torch.ones(e.shape[0], *grid), atol=1e-5)


@pytest.mark.parametrize("shape,max_patches,grid", [((320, 320), 400, (20, 20)), ((300, 500), 784, (22, 35))],
                         ids=["square-400", "wide-784"])
def test_aspect_grid_matches_oracle(device, shape, max_patches, grid):
    from imagescry_amd import ImageBatch, ViTB16Embedder, vit

    cfg = vit.ViTConfig(**NET)
    sd = vit.make_state_dict(cfg, seed=11, randomize_affine=True)
    assert vit.token_grid(*shape, max_patches) == grid and grid[0] * grid[1] + 1 > 224
    images = _images(2, *shape, seed=shape[1])
    ib = ImageBatch(indices=torch.arange(2), images=images).to(device)
    model = ViTB16Embedder(config=cfg, state_dict=sd, output="patches", grid="aspect", max_patches=max_patches).to(device)
    got = model.predict_step(ib).embeddings
    assert got.shape == (2, 128, *grid) and got.dtype == torch.float32
    tok, tok16 = _oracle(sd, cfg, images, grid)
    _check_map(got.cpu(), tok, tok16, grid, f"aspect {shape} -> {grid[0]}x{grid[1]}")
    cls_model = ViTB16Embedder(config=cfg, state_dict=sd, output="cls", grid="aspect", max_patches=max_patches).to(device)
    e_cls = cls_model.predict_step(ib).embeddings.cpu().reshape(2, 128)
    err_cls = (e_cls - F.normalize(tok[:, 0], dim=1)).abs().max().item()
    print(f"  class token: max|err| {err_cls:.3e}")
    assert err_cls < 1e-2


def test_fixed_grid_of_577_tokens_matches_oracle(device):
    from imagescry_amd import ImageBatch, ViTB16Embedder, vit

    cfg = vit.ViTConfig(image_size=384, **NET)
    assert cfg.tokens == 577
    sd = vit.make_state_dict(cfg, seed=12, randomize_affine=True)
    images = _images(2, 384, 384, seed=7)
    ib = ImageBatch(indices=torch.arange(2), images=images).to(device)
    tok, tok16 = _oracle(sd, cfg, images, (24, 24))
    patches = ViTB16Embedder(config=cfg, state_dict=sd, output="patches").to(device)
    got = patches.predict_step(ib).embeddings
    assert got.shape == (2, 128, 24, 24)
    _check_map(got.cpu(), tok, tok16, (24, 24), "fixed 24x24")
    cls_model = ViTB16Embedder(config=cfg, state_dict=sd).to(device)
    e_cls = cls_model.predict_step(ib).embeddings.cpu()
    assert e_cls.shape == (2, 128, 1, 1)
    e_cls = e_cls.reshape(2, 128)
    err_cls = (e_cls - F.normalize(tok[:, 0], dim=1)).abs().max().item()
    err_cls16 = (e_cls - F.normalize(tok16[:, 0], dim=1)).abs().max().item()
    print(f"fixed 24x24 class token: max|err| f32 {err_cls:.3e}, fp16-operand oracle {err_cls16:.3e}")
    assert err_cls < 1e-2
    assert err_cls16 < 2e-3


def test_a_batch_equals_its_single_images(device):
    from imagescry_amd import ViTB16Embedder, vit

    cfg = vit.ViTConfig(**NET)
    sd = vit.make_state_dict(cfg, seed=13, randomize_affine=True)
    kw = dict(config=cfg, state_dict=sd, output="patches", grid="aspect", max_patches=400)
    model = ViTB16Embedder(max_images_per_pass=2, **kw).to(device)
    x = model.preprocess(_images(5, 320, 320, seed=5).to(device))
    full = model(x)  # three passes: 2 + 2 + 1 images
    assert full.shape == (5, 128, 20, 20)
    singles = torch.cat([model(x[i : i + 1]) for i in range(5)])
    assert torch.equal(full, singles)
    assert torch.equal(ViTB16Embedder(**kw).to(device)(x), full)  # one pass


def test_a_20_x_20_patch_map_reaches_the_search(device):
    from imagescry_amd import EmbeddingBank, ImageBatch, ViTB16Embedder, vit

    cfg = vit.ViTConfig(**NET)
    model = ViTB16Embedder(config=cfg, seed=3, output="patches", grid="aspect", max_patches=400).to(device)
    ib = ImageBatch(indices=torch.tensor([0, 1, 2]), images=_images(3, 320, 320, seed=1)).to(device)
    emb = model.predict_step(ib)
    assert emb.embeddings.shape == (3, 128, 20, 20)
    cells = 400
    row_groups = emb.indices.cpu().repeat_interleave(cells)
    bank = EmbeddingBank.from_batches([emb], dtype=torch.float16, row_groups=row_groups)
    assert bank.num_local_rows == 3 * cells and bank.dim == 128
    q = emb.get_flat_vectors()[cells : 2 * cells]  # the second image's cells
    scores, idx = bank.search(q, k=1)
    assert torch.equal(idx[:, 0].cpu(), torch.arange(cells, 2 * cells))  # every cell finds itself
    assert (scores[:, 0].cpu() - 1).abs().max().item() <= 1e-3  # fp16 bank
    labels = torch.full((cells,), 1, dtype=torch.int64)
    _s, gi, gl = bank.search_groups(q, k=2, exclude_group=labels)
    assert not (gl.cpu() == 1).any() and (gi.cpu() >= 0).all()
