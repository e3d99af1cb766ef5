"""Host side of the DINOv2 backbones: the token oracle (tests/dinov2_oracle.py) against `transformers.Dinov2Model` and
`Dinov2WithRegistersModel`, what `vit.prepare` / `vit.make_state_dict` / `vit.from_transformers_state_dict` do with the
new parameters, the `DINOv2Embedder` constructor, and the bound of the antialiased position resampling.  CPU only.

The bound of isc_vit_pos_resample_aa (`dinov2_oracle.aa_bound`), against the float64 result, u = 2^-24, `top` the largest
|input|.  An output is sum_a wy_a sum_b wx_b v_ab over ny x nx taps with normalised weights, Ay = max sum_a |wy_a| and Ax
likewise (recomputed in float64 for the grid under test).

* Accumulation.  A float32 dot product of n terms is off by at most n u sum |w_i v_i|.  The inner sums are each within
  nx u Ax top, the outer sum adds ny u Ay (Ax top) and carries the inner errors with weight Ay:
  (ny + nx) u Ay Ax top.
* Weights.  A raw weight is cubic(t), t = (j - centre + 0.5) / max(s, 1), centre = s (i + 0.5), s = g / n_out.  In
  float32 s and the product carry a rounding each, so centre is off by 2 u g at most; the subtraction and the 0.5 add
  2 u (support + 1), the reciprocal and the last product 3 u |t| with |t| <= 2: with g / max(s, 1) = min(g, n_out),
  |dt| <= (2 min(g, n_out) + 12) u.  |cubic'| <= 1.4 (A = -0.5: 4.5 x^2 - 5 x at x = 5/9), and the six operations of the
  Horner form on intermediates below 8 add 16 u: a raw weight is within rho u, rho = 2.8 min(g, n_out) + 33.
  The normaliser, a sum of n raw weights r_i, is within n rho u + n u sum |r_i|.  With w_i = r_i / total,
  |dw_i| <= |dr_i| / total + |w_i| |dtotal| / total + u |w_i|, and summed over the taps, with q = max n / total:
  E = sum |dw_i| <= ((1 + A) q rho + n A^2 + A) u.
  The weight errors of one axis act on sums bounded by the other axis' A: Ay Ex top + Ax Ey top.

bound = u top ((ny + nx) Ay Ax + Ay Ex + Ax Ey); second-order terms are below 1e-4 of it.  It is a worst case (every
rounding in the same direction, the coordinate error at the steepest point of the kernel), so a float32 evaluation is
expected far inside it -- `test_antialias_bound_holds_for_torch_float32` prints how far torch's own is -- while a
wrong kernel constant (A = -0.75), a wrong support or missing normalisation is off by 1e-2 top or more."""

from __future__ import annotations

import dataclasses
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

from dinov2_oracle import AA_GRIDS, aa_bound, aa_restated_f64, dinov2_tokens, interpolate_pos_embed  # noqa: E402
from imagescry_amd import DINOv2Embedder, ViTB16Embedder, vit  # noqa: E402


# ------------------------------------------------------------------------------------------ oracle vs transformers
@pytest.mark.parametrize("grid", [(5, 5), (4, 6), (7, 3)])
@pytest.mark.parametrize("registers", [0, 4])
def test_token_oracle_matches_transformers(registers, grid):
    transformers = pytest.importorskip("transformers")
    kw = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, image_size=70, patch_size=14, mlp_ratio=4)
    if registers:
        model = transformers.Dinov2WithRegistersModel(
            transformers.Dinov2WithRegistersConfig(num_register_tokens=registers, **kw)).eval()
    else:
        model = transformers.Dinov2Model(transformers.Dinov2Config(**kw)).eval()
    g = torch.Generator().manual_seed(7 + registers)
    with torch.no_grad():  # random init leaves LayerScale at 1, biases at 0 and norms at the identity
        for name, p in model.named_parameters():
            if "lambda1" in name:
                p.copy_(10.0 ** (-3.0 * torch.rand(p.shape, generator=g)))
            elif name.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif "norm" in name:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.75)
            elif "tokens" in name or "position" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    sd = vit.from_transformers_state_dict(model.state_dict())
    assert ("register_tokens" in sd) == bool(registers) and "mask_token" not in sd
    assert sd["blocks.1.attn.qkv.weight"].shape == (384, 128) and sd["blocks.0.ls2.gamma"].shape == (128,)
    assert torch.equal(sd["blocks.0.attn.qkv.bias"][128:256], model.state_dict()["encoder.layer.0.attention.attention.key.bias"])
    x = torch.randn(2, 3, 14 * grid[0], 14 * grid[1], generator=g).clamp(-3, 3)
    with torch.no_grad():
        want = model(pixel_values=x).last_hidden_state
        got = dinov2_tokens(sd, x, patch=14, heads=2, eps=model.config.layer_norm_eps, antialias=bool(registers))
    assert got.shape == (2, 1 + registers + grid[0] * grid[1], 128)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)  # the tolerance of tests/test_oracle_vit.py
    # the converted dict is one `prepare` takes (head size 64: two heads of 128 channels)
    cfg = vit.ViTConfig(image_size=70, patch_size=14, dim=128, depth=2, heads=2, mlp_dim=512, registers=registers,
                        layerscale=True, pos_antialias=bool(registers))
    net = vit.prepare(sd, cfg)
    assert (net.reg_tokens is not None) == bool(registers) and net.blocks[1].ls2.dtype == torch.float32


def test_resample_modes_differ():
    pos = torch.randn(1, 26, 8, generator=torch.Generator().manual_seed(0))
    assert interpolate_pos_embed(pos, (5, 5), antialias=True) is pos
    plain, aa = interpolate_pos_embed(pos, (7, 3)), interpolate_pos_embed(pos, (7, 3), antialias=True)
    assert torch.equal(plain[:, 0], pos[:, 0]) and torch.equal(aa[:, 0], pos[:, 0])
    assert (plain - aa).abs().max().item() > 0.05  # downsampling: the antialiased filter is another function


# -------------------------------------------------------------------------------------- prepare and make_state_dict
SMALL = vit.ViTConfig(image_size=70, patch_size=14, dim=128, depth=2, heads=2, mlp_dim=256, registers=4, layerscale=True,
                      pos_antialias=True)


def test_patch_weight_is_padded_to_whole_k_steps():
    assert (SMALL.patch_kdim, vit.VIT_B16.patch_kdim, SMALL.num_prefix, SMALL.tokens) == (640, 768, 5, 30)
    sd = vit.make_state_dict(SMALL, seed=1)
    net = vit.prepare(sd, SMALL)
    assert (net.patch.out_features, net.patch.in_features) == (128, 640)
    w = vit.unpack_rows(net.patch.weight, 128, 640)
    assert torch.equal(w[:, :588], sd["patch_embed.proj.weight"].reshape(128, 588).half())
    assert torch.equal(w[:, 588:], torch.zeros(128, 52, dtype=torch.float16))
    assert net.pos_embed.shape == (26, 128) and net.reg_tokens.shape == (4, 128)
    # LayerScale is kept apart in float32, not folded into the fp16 weights
    assert torch.equal(net.blocks[0].ls1, sd["blocks.0.ls1.gamma"]) and net.blocks[0].ls1.dtype == torch.float32
    assert torch.equal(vit.unpack_rows(net.blocks[0].proj.weight, 128, 128), sd["blocks.0.attn.proj.weight"].half())
    moved = net.to(torch.device("cpu"))
    assert torch.equal(moved.reg_tokens, net.reg_tokens) and torch.equal(moved.blocks[1].ls2, net.blocks[1].ls2)


def test_prepare_refuses_what_the_state_dict_lacks():
    sd = vit.make_state_dict(SMALL, seed=2)
    no_reg = {k: v for k, v in sd.items() if k != "register_tokens"}
    with pytest.raises(ValueError, match="register"):
        vit.prepare(no_reg, SMALL)
    timm = dict(no_reg, reg_token=sd["register_tokens"], mask_token=torch.zeros(1, 128))  # timm's spelling; ignored key
    assert torch.equal(vit.prepare(timm, SMALL).reg_tokens, vit.prepare(sd, SMALL).reg_tokens)
    with pytest.raises(ValueError, match="ls2.gamma"):
        vit.prepare({k: v for k, v in sd.items() if k != "blocks.1.ls2.gamma"}, SMALL)
    with pytest.raises(ValueError, match="register_tokens has shape"):
        vit.prepare(dict(sd, register_tokens=torch.zeros(1, 3, 128)), SMALL)
    with pytest.raises(ValueError, match="head size 64"):  # ViT-g's head size of 96, say
        bad = dataclasses.replace(SMALL, dim=192)
        vit.prepare(vit.make_state_dict(bad), bad)
    plain = dataclasses.replace(SMALL, registers=0, layerscale=False)
    net = vit.prepare(sd, plain)  # a config that asks for less ignores the rest
    assert net.reg_tokens is None and net.blocks[0].ls1 is None


def _parent_state_dict(cfg: vit.ViTConfig, seed: int, randomize_affine: bool) -> dict[str, torch.Tensor]:
    """`make_state_dict` as it drew before registers and LayerScale existed."""
    g = torch.Generator().manual_seed(seed)
    tn = lambda *shape: torch.nn.init.trunc_normal_(torch.empty(*shape), std=0.02, a=-0.04, b=0.04, generator=g)  # noqa: E731
    bias = lambda n: torch.randn(n, generator=g) * 0.05 if randomize_affine else torch.zeros(n)  # noqa: E731
    gamma = lambda n: torch.rand(n, generator=g) * 0.5 + 0.75 if randomize_affine else torch.ones(n)  # noqa: E731
    d = cfg.dim
    sd = {"cls_token": tn(1, 1, d), "pos_embed": tn(1, cfg.grid**2 + 1, d),
          "patch_embed.proj.weight": tn(d, 3, cfg.patch_size, cfg.patch_size), "patch_embed.proj.bias": bias(d)}
    for i in range(cfg.depth):
        p = f"blocks.{i}"
        sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"] = gamma(d), bias(d)
        sd[f"{p}.attn.qkv.weight"], sd[f"{p}.attn.qkv.bias"] = tn(3 * d, d), bias(3 * d)
        sd[f"{p}.attn.proj.weight"], sd[f"{p}.attn.proj.bias"] = tn(d, d), bias(d)
        sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"] = gamma(d), bias(d)
        sd[f"{p}.mlp.fc1.weight"], sd[f"{p}.mlp.fc1.bias"] = tn(cfg.mlp_dim, d), bias(cfg.mlp_dim)
        sd[f"{p}.mlp.fc2.weight"], sd[f"{p}.mlp.fc2.bias"] = tn(d, cfg.mlp_dim), bias(d)
    sd["norm.weight"], sd["norm.bias"] = gamma(d), bias(d)
    return sd


@pytest.mark.parametrize("randomize_affine", [False, True])
def test_make_state_dict_keeps_the_existing_draws(randomize_affine):
    cfg = vit.ViTConfig(depth=2)
    for seed in (0, 5):
        want = _parent_state_dict(cfg, seed, randomize_affine)
        got = vit.make_state_dict(cfg, seed=seed, randomize_affine=randomize_affine)
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    # the new parameters come after every existing draw
    want = _parent_state_dict(SMALL, 3, randomize_affine)
    got = vit.make_state_dict(SMALL, seed=3, randomize_affine=randomize_affine)
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert sorted(set(got) - set(want)) == sorted(["register_tokens"] + [f"blocks.{i}.ls{n}.gamma" for i in (0, 1) for n in (1, 2)])
    ls = torch.stack([got[f"blocks.{i}.ls{n}.gamma"] for i in (0, 1) for n in (1, 2)])
    if randomize_affine:  # log-uniform over the range trained checkpoints cover
        assert 1e-5 <= ls.min() < 1e-4 and 0.1 < ls.max() <= 1.0
    else:
        assert torch.equal(ls, torch.ones(4, 128))


def test_presets():
    table = {"S": (384, 12, 6, 1536), "B": (768, 12, 12, 3072), "L": (1024, 24, 16, 4096)}
    for letter, (dim, depth, heads, mlp) in table.items():
        plain, reg = getattr(vit, f"DINOV2_{letter}14"), getattr(vit, f"DINOV2_{letter}14_REG")
        assert (plain.image_size, plain.patch_size, plain.dim, plain.depth, plain.heads, plain.mlp_dim) == (518, 14, dim, depth, heads, mlp)
        assert plain.layerscale and not plain.registers and not plain.pos_antialias and plain.grid == 37
        assert reg == dataclasses.replace(plain, registers=4, pos_antialias=True)
        assert (plain.tokens, reg.tokens, reg.num_prefix, plain.patch_kdim) == (1370, 1374, 5, 640)
    assert vit.VIT_B16 == vit.ViTConfig() and vit.VIT_B16.num_prefix == 1 and vit.VIT_B16.tokens == 197
    assert vit.gemm_flops(vit.DINOV2_B14_REG) > vit.gemm_flops(vit.DINOV2_B14) > vit.gemm_flops(vit.VIT_B16)
    # long sequences run in passes of fewer images, counted with the registers
    assert vit.images_per_pass(261, 1024) == 1024 * 197 // 261


# -------------------------------------------------------------------------------------------------- DINOv2Embedder
def test_embedder_constructor(monkeypatch):
    from imagescry_amd import embedding

    for (variant, reg), cfg in list(embedding.DINOV2_PRESETS.items()):  # depth 1: the constructor draws every weight
        monkeypatch.setitem(embedding.DINOV2_PRESETS, (variant, reg), dataclasses.replace(cfg, depth=1))
    for variant, dim in (("vits14", 384), ("vitb14", 768), ("vitl14", 1024)):
        m = DINOv2Embedder(variant)
        assert isinstance(m, ViTB16Embedder) and m.embedding_dim == dim and m.config.registers == 0
        assert m.hparams == {"image_size": 518, "patch_size": 14, "depth": 1, "variant": variant, "registers": False}
    m = DINOv2Embedder("vitb14", registers=True, output="patches", grid="aspect", max_patches=256)
    assert m.config.registers == 4 and m.config.pos_antialias and m._net.reg_tokens.shape == (4, 768)
    assert m.hparams == {"image_size": 518, "patch_size": 14, "depth": 1, "output": "patches", "grid": "aspect",
                         "max_patches": 256, "variant": "vitb14", "registers": True}
    assert DINOv2Embedder().hparams["variant"] == "vitb14"
    with pytest.raises(ValueError, match="variant"):
        DINOv2Embedder("vitg14")
    with pytest.raises(TypeError):
        DINOv2Embedder("vitb14", 4)
    with pytest.raises(ValueError):
        DINOv2Embedder("vits14", output="tokens")
    with pytest.raises(ValueError):
        DINOv2Embedder("vits14", max_patches=256)  # needs grid="aspect"
    with pytest.raises(ValueError, match="register"):  # a checkpoint without registers for a register model
        DINOv2Embedder("vits14", True, state_dict=vit.make_state_dict(dataclasses.replace(vit.DINOV2_S14, depth=1)))
    # shapes are refused before anything touches a device: 17 x 16 patches against max_patches = 256
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 14 * 17, 14 * 16))
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 224, 225))
    # ViTB16Embedder's own hparams are as they were
    assert ViTB16Embedder(config=vit.ViTConfig(depth=1)).hparams == {"image_size": 224, "patch_size": 16, "depth": 1}


# ------------------------------------------------------------------------------------------------ antialias bound
@pytest.mark.parametrize("g,h,w", AA_GRIDS)
def test_antialias_bound_holds_for_torch_float32(g, h, w):
    """torch's own float32 `F.interpolate(antialias=True)` is inside the bound the GPU kernel is held to
    (tests/test_gpu_dinov2.py), measured against the float64 call; the float64 call equals the restatement the bound is
    computed from (A = -0.5, support 2 max(s, 1), clipped and normalised taps)."""
    d = 64
    pos = torch.randn(1 + g * g, d, generator=torch.Generator().manual_seed(g * 100 + h * 10 + w)) * 0.02
    src = pos[1:].reshape(1, g, g, d).permute(0, 3, 1, 2)
    kw = dict(size=(h, w), mode="bicubic", align_corners=False, antialias=True)
    want = F.interpolate(src.double(), **kw).permute(0, 2, 3, 1).reshape(h * w, d)
    got = F.interpolate(src, **kw).permute(0, 2, 3, 1).reshape(h * w, d)
    restated = aa_restated_f64(pos, g, h, w)
    assert torch.equal(restated[0], pos[0].double())
    torch.testing.assert_close(restated[1:], want, rtol=0, atol=1e-12)
    bound = aa_bound(g, h, w, pos.abs().max().item())
    err = (got.double() - want).abs().max().item()
    print(f"antialiased resample {g} -> {h}x{w}: torch float32 max|err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert bound < 1e-3 * pos.abs().max().item()  # ... and the bound still tells a wrong filter from a right one
    wrong = F.interpolate(src.double(), size=(h, w), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(h * w, d)
    if (h, w) != (1, 1) or g > 1:
        assert (wrong - want).abs().max().item() > 100 * bound
