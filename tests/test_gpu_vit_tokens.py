"""ViT patch-token embedding maps on the GPU: the position-table resampling (isc_vit_pos_resample), the patch-token head
(isc_vit_tokens_out), and `ViTB16Embedder(output="patches", grid="fixed" | "aspect")` end to end -- against float32
torch restatements (tests/vit_tokens_oracle.py, pinned to transformers.ViTModel in tests/test_vit_tokens_host.py) and
through `EmbeddingBank` / `EmbedSearchPipeline`.

Tolerances.  isc_vit_pos_resample: every output is a 16-tap dot product whose weights have an absolute sum below
1.375^2 < 2 (A = -0.75, worst at the half-way phase), so two float32 evaluations differ by a few dozen ulps of the largest
input at most: 64 * 2^-24 * max|pos_embed|.  isc_vit_tokens_out: rtol = atol = 1e-5, what `test_layernorm` uses for a
float32 LayerNorm.  The model: the bounds of `test_vit_embedder_matches_oracle` (1e-2 to the float32 oracle, 2e-3 to the
oracle with fp16-rounded operands, unit norm to 1e-5) on every cell."""

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


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- isc_vit_pos_resample
def _resample(device, pos: torch.Tensor, g: int, h: int, w: int) -> torch.Tensor:
    from imagescry_amd import _lib

    d = pos.shape[1]
    pd = pos.to(device)
    out = torch.full((1 + h * w, d), float("nan"), dtype=torch.float32, device=device)
    st = _lib.load().isc_vit_pos_resample(pd.data_ptr(), g, h, w, d, out.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_vit_pos_resample")
    assert torch.equal(pd.cpu(), pos)
    return out.cpu()


@pytest.mark.parametrize("grid", [(11, 17), (17, 11), (1, 196), (7, 7), (14, 13)])
def test_pos_resample_matches_interpolate(device, grid):
    h, w = grid
    g, d = 14, 768
    pos = torch.randn(1 + g * g, d, generator=_gen(h * 100 + w)) * 0.02
    got = _resample(device, pos, g, h, w)
    want = F.interpolate(pos[1:].reshape(1, g, g, d).permute(0, 3, 1, 2), size=(h, w), mode="bicubic", align_corners=False)
    want = want.permute(0, 2, 3, 1).reshape(h * w, d)
    assert torch.equal(got[0], pos[0])  # the class row is kept
    err = (got[1:] - want).abs().max().item()
    bound = 64 * 2.0**-24 * pos.abs().max().item()
    print(f"pos_resample {h}x{w}: max|err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_pos_resample_native_grid_and_cache(device):
    from imagescry_amd import vit

    pos = torch.randn(197, 768, generator=_gen(3)) * 0.02
    assert torch.equal(_resample(device, pos, 14, 14, 14), pos)  # weights (0, 1, 0, 0): the table, bit for bit
    cfg = vit.ViTConfig(depth=1)
    net = vit.prepare(vit.make_state_dict(cfg, seed=1), cfg).to(device)
    assert vit.position_table(net, (14, 14)) is net.pos_embed and not net.pos_cache
    t1 = vit.position_table(net, (11, 17))
    assert vit.position_table(net, (11, 17)) is t1 and t1.shape == (188, 768)
    assert torch.equal(t1.cpu(), _resample(device, net.pos_embed.cpu(), 14, 11, 17))
    for h in range(1, vit.POS_CACHE_MAX + 4):  # the cache is bounded
        vit.position_table(net, (h, 3))
    assert len(net.pos_cache) == vit.POS_CACHE_MAX and (11, 17) not in net.pos_cache


def test_pos_resample_rejects_bad_arguments(device):
    from imagescry_amd import _lib

    lib = _lib.load()
    s = _lib.stream_handle(device)
    pos = torch.zeros(197 * 768 + 8, dtype=torch.float32, device=device)
    out = torch.zeros(188 * 768 + 8, dtype=torch.float32, device=device)
    assert lib.isc_vit_pos_resample(pos.data_ptr() + 4, 14, 11, 17, 768, out.data_ptr(), s) == _lib.ISC_ERR_ALIGNMENT
    assert lib.isc_vit_pos_resample(pos.data_ptr(), 14, 11, 17, 768, out.data_ptr() + 8, s) == _lib.ISC_ERR_ALIGNMENT
    assert lib.isc_vit_pos_resample(pos.data_ptr(), 14, 11, 17, 6, out.data_ptr(), s) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_vit_pos_resample(None, 14, 11, 17, 768, out.data_ptr(), s) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_vit_pos_resample(pos.data_ptr(), 14, 0, 17, 768, out.data_ptr(), s) == _lib.ISC_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ isc_vit_tokens_out
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("t", [2, 50, 188, 197])
@pytest.mark.parametrize("b", [1, 3, 40])
def test_tokens_out(device, b, t, normalize):
    from imagescry_amd import _lib

    d = 768
    g = _gen(b * 1000 + t)
    tokens = torch.randn(b, t, d, generator=g) * 3 + 1.5
    tokens[b - 1, t - 1] = 0.0  # an all-zero patch token: LayerNorm leaves the bias, which normalises without NaN
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    want = F.layer_norm(tokens[:, 1:], (d,), gamma, beta, 1e-6).transpose(1, 2)
    if normalize:
        want = F.normalize(want, dim=1, eps=1e-12)
    td, gd, bd = tokens.to(device), gamma.to(device), beta.to(device)
    out = torch.full((b, d, t - 1), float("nan"), dtype=torch.float32, device=device)
    st = _lib.load().isc_vit_tokens_out(td.data_ptr(), b, t, d, gd.data_ptr(), bd.data_ptr(), 1e-6, int(normalize),
                                        1e-12, out.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_vit_tokens_out")
    got = out.cpu()
    assert not torch.isnan(got).any()  # every cell written
    assert torch.equal(td.cpu(), tokens)  # the source, class rows included, is untouched
    torch.testing.assert_close(got, want.contiguous(), rtol=1e-5, atol=1e-5)
    zero = got[b - 1, :, t - 2]
    ref = F.normalize(beta, dim=0) if normalize else beta
    torch.testing.assert_close(zero, ref, rtol=1e-5, atol=1e-5)


def test_tokens_out_rejects_bad_arguments(device):
    from imagescry_amd import _lib

    lib = _lib.load()
    s = _lib.stream_handle(device)
    x = torch.zeros(2 * 5 * 768 + 8, dtype=torch.float32, device=device)
    gam = torch.ones(2048, dtype=torch.float32, device=device)
    out = torch.zeros(2 * 4 * 2048 + 8, dtype=torch.float32, device=device)

    def call(xp, t, d, gp, op):
        return lib.isc_vit_tokens_out(xp, 2, t, d, gp, gam.data_ptr(), 1e-6, 1, 1e-12, op, s)

    assert call(x.data_ptr() + 4, 5, 768, gam.data_ptr(), out.data_ptr()) == _lib.ISC_ERR_ALIGNMENT
    assert call(x.data_ptr(), 5, 768, gam.data_ptr() + 8, out.data_ptr()) == _lib.ISC_ERR_ALIGNMENT
    assert call(x.data_ptr(), 5, 768, gam.data_ptr(), out.data_ptr() + 4) == _lib.ISC_ERR_ALIGNMENT
    assert call(x.data_ptr(), 5, 6, gam.data_ptr(), out.data_ptr()) == _lib.ISC_ERR_UNSUPPORTED  # D % 4
    assert call(x.data_ptr(), 5, 2048, gam.data_ptr(), out.data_ptr()) == _lib.ISC_ERR_UNSUPPORTED  # D > 1024
    assert call(x.data_ptr(), 1, 768, gam.data_ptr(), out.data_ptr()) == _lib.ISC_ERR_INVALID_ARG  # no patch token
    assert call(None, 5, 768, gam.data_ptr(), out.data_ptr()) == _lib.ISC_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------ the embedder
def _images(batch: int, h: int, w: int, seed: int) -> torch.Tensor:
    return torch.randint(0, 256, (batch, 3, h, w), dtype=torch.uint8, generator=_gen(seed))


def test_fused_head_equals_separate_normalisation(device):
    from imagescry_amd import ImageBatch, ViTB16Embedder, vit
    from imagescry_amd.embedding import l2_normalize_channels

    cfg = vit.ViTConfig(depth=2)
    sd = vit.make_state_dict(cfg, seed=4, randomize_affine=True)
    for grid, shape in (("fixed", (224, 224)), ("aspect", (100, 160)), ("aspect", (40, 2000))):
        model = ViTB16Embedder(config=cfg, state_dict=sd, output="patches", grid=grid).to(device)
        assert model._head_normalizes
        ib = ImageBatch(indices=torch.arange(3), images=_images(3, *shape, seed=9)).to(device)
        got = model.predict_step(ib).embeddings
        want = l2_normalize_channels(model.forward(model.preprocess(ib.images)))
        assert got.shape == want.shape and got.shape[:2] == (3, 768)
        assert torch.equal(got, want)


@pytest.mark.parametrize("depth", [2, 12])
@pytest.mark.parametrize("grid,shape", [("fixed", (224, 224)), ("aspect", (100, 160)), ("aspect", (300, 200))])
def test_patch_map_matches_oracle(device, depth, grid, shape):
    from imagescry_amd import ImageBatch, ViTB16Embedder, vit

    batch = 2
    cfg = vit.ViTConfig(depth=depth)
    sd = vit.make_state_dict(cfg, seed=depth, randomize_affine=True)
    images = _images(batch, *shape, seed=depth + shape[0])
    h, w = vit.token_grid(*shape, cfg.grid**2) if grid == "aspect" else (cfg.grid, cfg.grid)
    ib = ImageBatch(indices=torch.arange(batch), images=images).to(device)
    model = ViTB16Embedder(config=cfg, state_dict=sd, output="patches", grid=grid).to(device)
    got = model.predict_step(ib).embeddings
    assert got.shape == (batch, 768, h, w) and got.dtype == torch.float32
    e = got.cpu()
    cls_model = ViTB16Embedder(config=cfg, state_dict=sd, output="cls", grid=grid).to(device)
    e_cls = cls_model.predict_step(ib).embeddings.cpu()
    assert e_cls.shape == (batch, 768, 1, 1)

    resized = images if tuple(shape) == (16 * h, 16 * w) else transforms_oracle.resize(images, (16 * h, 16 * w))
    x = transforms_oracle.normalize_per_channel(resized, min_value=-3, max_value=3)
    with torch.no_grad():
        tok = vit_tokens(sd, x, eps=cfg.ln_eps)
        tok16 = vit_tokens(sd, x, eps=cfg.ln_eps, round_operands_fp16=True)
    want, want16 = patch_map(tok, (h, w)), patch_map(tok16, (h, w))
    want_cls = F.normalize(tok[:, 0], dim=1)

    err, err16 = (e - want).abs().max().item(), (e - want16).abs().max().item()
    cos = (e * want).sum(dim=1).min().item()
    err_cls = (e_cls.reshape(batch, 768) - want_cls).abs().max().item()
    cos_cls = (e_cls.reshape(batch, 768) * want_cls).sum(dim=1).min().item()
    print(f"patch map depth {depth} {grid} {shape} -> {h}x{w}: max|err| f32 {err:.3e}, fp16-operand oracle {err16:.3e}, "
          f"1 - min cell cosine {1 - cos:.2e}; class token: max|err| {err_cls:.3e}, 1 - min cosine {1 - cos_cls:.2e}")
    assert err < 1e-2  # the fp16 tolerance of the brief
    assert err16 < 2e-3  # against the same operand rounding: implementation error only
    assert torch.allclose(e.norm(dim=1), torch.ones(batch, h, w), atol=1e-5)
    assert err_cls < 1e-2


def test_default_mode_is_unchanged_and_modes_share_no_state(device):
    from imagescry_amd import ImageBatch, ViTB16Embedder, vit

    cfg = vit.ViTConfig(depth=2)
    sd = vit.make_state_dict(cfg, seed=6, randomize_affine=True)
    ib = ImageBatch(indices=torch.arange(4), images=_images(4, 120, 90, seed=2)).to(device)
    default = ViTB16Embedder(config=cfg, state_dict=sd).to(device)
    before = default.predict_step(ib).embeddings.clone()
    explicit = ViTB16Embedder(config=cfg, state_dict=sd, output="cls", grid="fixed").to(device)
    assert torch.equal(explicit.predict_step(ib).embeddings, before)
    patches = ViTB16Embedder(config=cfg, state_dict=sd, output="patches", grid="aspect").to(device)
    m = patches.predict_step(ib).embeddings
    assert m.shape == (4, 768, *vit.token_grid(120, 90))
    assert patches._net.pos_cache and not default._net.pos_cache and not explicit._net.pos_cache
    assert torch.equal(default.predict_step(ib).embeddings, before)
    # a 224 x 224 input in aspect mode IS the fixed path
    sq = ImageBatch(indices=torch.arange(2), images=_images(2, 224, 224, seed=3)).to(device)
    fixed = ViTB16Embedder(config=cfg, state_dict=sd, output="patches", grid="fixed").to(device)
    assert torch.equal(patches.predict_step(sq).embeddings, fixed.predict_step(sq).embeddings)
    aspect_cls = ViTB16Embedder(config=cfg, state_dict=sd, output="cls", grid="aspect").to(device)
    assert torch.equal(aspect_cls.predict_step(sq).embeddings, default.predict_step(sq).embeddings)
    assert aspect_cls.predict_step(ib).embeddings.shape == (4, 768, 1, 1)
    with pytest.raises(ValueError):
        fixed(torch.zeros(1, 3, 176, 272, device=device))
    with pytest.raises(ValueError):
        patches(torch.zeros(1, 3, 16 * 15, 16 * 14, device=device))


def test_batch_512_equals_its_slices(device):
    from imagescry_amd import ViTB16Embedder, vit

    cfg = vit.ViTConfig(depth=2)
    sd = vit.make_state_dict(cfg, seed=8, randomize_affine=True)
    model = ViTB16Embedder(config=cfg, state_dict=sd, output="patches", max_images_per_pass=100).to(device)
    x = model.preprocess(_images(512, 224, 224, seed=5).to(device))
    full = model(x)  # six passes: 5 x 100 + 12 images
    assert full.shape == (512, 768, 14, 14)
    parts = torch.cat([model(x[i : i + 64]) for i in range(0, 512, 64)])
    assert torch.equal(full, parts)
    one_pass = ViTB16Embedder(config=cfg, state_dict=sd, output="patches").to(device)
    assert torch.equal(one_pass(x), full)


def test_patch_maps_reach_the_search(device):
    from imagescry_amd import EmbeddingBank, EmbedSearchPipeline, ImageBatch, ViTB16Embedder, vit

    cfg = vit.ViTConfig(depth=2)
    model = ViTB16Embedder(config=cfg, seed=3, output="patches", grid="aspect").to(device)
    batches = [ImageBatch(indices=torch.tensor([0, 1, 2]), images=_images(3, 100, 160, seed=1)).to(device),
               ImageBatch(indices=torch.tensor([3, 4, 5]), images=_images(3, 200, 120, seed=2)).to(device)]
    embs = [model.predict_step(b) for b in batches]
    cells = [e.embeddings.shape[2] * e.embeddings.shape[3] for e in embs]
    assert cells == [11 * 17, 18 * 10]
    row_groups = torch.cat([e.indices.cpu().repeat_interleave(c) for e, c in zip(embs, cells)])
    bank = EmbeddingBank.from_batches(embs, dtype=torch.float16, row_groups=row_groups)
    assert bank.num_local_rows == 3 * (cells[0] + cells[1]) and bank.dim == 768

    own = 4  # the second image of the second batch
    first = 3 * cells[0] + cells[1]
    q = embs[1].get_flat_vectors()[cells[1] : 2 * cells[1]]
    scores, idx = bank.search(q, k=1)
    assert torch.equal(idx[:, 0].cpu(), torch.arange(first, first + cells[1]))  # every cell finds itself
    assert (scores[:, 0].cpu() - 1).abs().max().item() <= 1e-3  # fp16 bank
    labels = torch.full((cells[1],), own, dtype=torch.int64)
    _s, gi, gl = bank.search_groups(q, k=2, exclude_group=labels)
    assert not (gl.cpu() == own).any() and (gi.cpu() >= 0).all()
    assert not (row_groups[gi.cpu()] == own).any()
    _s, _gi, gl1 = bank.search_groups(q, k=1)
    assert (gl1.cpu() == own).all()

    pipe = EmbedSearchPipeline(embedding_model=model, bank=bank, k=3, image_groups=torch.arange(6))
    res = pipe.run([batches[0]])
    torch.cuda.synchronize(device)
    assert len(res) == 1 and res[0].neighbours.shape == (3 * cells[0], 3)
    nb = res[0].neighbours.cpu()
    own_of_row = torch.arange(3).repeat_interleave(cells[0])[:, None]
    assert (nb >= 0).all() and not (row_groups[nb] == own_of_row).any()  # "similar cells in OTHER images"
