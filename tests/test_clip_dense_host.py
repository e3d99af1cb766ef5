"""The dense CLIP patch map on the CPU: the constructor rules of `CLIPEmbedder(dense=...)`, the value Linear, and what
the GPU tests (tests/test_gpu_clip_dense.py) rest on -- the fp16-operand oracle's distance to the float32 one, the
distance between the modes, and the self-selector operands of tests/clip_dense_oracle.py."""

from __future__ import annotations

import functools
import itertools
import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_dense_oracle as do  # noqa: E402
import clip_oracle as co  # noqa: E402
import vit_bounds as vb  # noqa: E402

from imagescry_amd import CLIPEmbedder, clip, vit  # noqa: E402

VOCAB, CONTEXT = 64, 16
SMALL = clip.CLIPConfig(
    vit.ViTConfig(image_size=32, patch_size=8, dim=128, depth=2, heads=2, mlp_dim=256, ln_eps=1e-5, pre_norm=True,
                  act="quick_gelu", embed_dim=64),
    clip.CLIPTextConfig(dim=64, depth=2, heads=1, mlp_dim=128, embed_dim=64, context=CONTEXT, vocab=VOCAB))


def test_constructor_rules():
    sd = clip.make_state_dict(SMALL, seed=1)
    with pytest.raises(ValueError, match="patches"):  # as before the keyword existed
        CLIPEmbedder(SMALL, state_dict=sd, output="patches")
    for mode in do.MODES:
        with pytest.raises(ValueError, match="dense"):
            CLIPEmbedder(SMALL, state_dict=sd, dense=mode)  # output="cls"
        with pytest.raises(ValueError, match="dense"):
            CLIPEmbedder(SMALL, state_dict=sd, output="cls", dense=mode)
    for bad in ("vv", "qk", "", "KK", 1):
        with pytest.raises(ValueError, match="dense"):
            CLIPEmbedder(SMALL, state_dict=sd, output="patches", dense=bad)
    with pytest.raises(ValueError, match="output"):
        CLIPEmbedder(SMALL, state_dict=sd, output="tokens", dense="kk")
    with pytest.raises(ValueError, match="max_patches"):
        CLIPEmbedder(SMALL, state_dict=sd, output="patches", dense="kk", max_patches=64)  # needs grid="aspect"
    plain = CLIPEmbedder(SMALL, state_dict=sd)
    assert plain.dense is None and "dense" not in plain.hparams and plain._dense_value is None
    for mode in do.MODES:
        m = CLIPEmbedder(SMALL, state_dict=sd, output="patches", dense=mode, grid="aspect", max_patches=64)
        assert m.embedding_dim == 64 and m.dense == mode and m.output == "patches"
        assert m.hparams["dense"] == mode and m.hparams["output"] == "patches" and m.hparams["max_patches"] == 64
        assert (m._dense_value is not None) == (mode == "value")
        assert m._head_normalizes  # predict_step normalises in the head kernel
    m = CLIPEmbedder(SMALL, state_dict=sd, output="patches", dense="qq", preprocess="checkpoint")
    assert m.hparams["preprocess"] == "checkpoint" and m.crop_size == 32
    with pytest.raises(TypeError):  # the text side is what it was
        m.encode_text(torch.zeros(2, CONTEXT))


def test_the_value_linear_is_the_last_third_of_the_qkv_weight():
    sd = clip.make_state_dict(SMALL, seed=2, randomize_affine=True)
    d = SMALL.vision.dim
    m = CLIPEmbedder(SMALL, state_dict=sd, output="patches", dense="value")
    lin = m._dense_value
    last = f"visual.blocks.{SMALL.vision.depth - 1}.attn.qkv"
    assert (lin.out_features, lin.in_features) == (d, d)
    assert torch.equal(vit.unpack_rows(lin.weight, d, d), sd[f"{last}.weight"][2 * d : 3 * d].half())
    assert torch.equal(lin.bias, sd[f"{last}.bias"][2 * d : 3 * d])
    first = "visual.blocks.0.attn.qkv"  # and of the LAST block
    assert not torch.equal(vit.unpack_rows(lin.weight, d, d), sd[f"{first}.weight"][2 * d : 3 * d].half())
    # the fused weight of that block is still whole
    assert torch.equal(vit.unpack_rows(m._net.blocks[-1].qkv.weight, 3 * d, d), sd[f"{last}.weight"].half())
    with pytest.raises(ValueError, match="value"):
        vit.forward_dense(m._net, torch.zeros(1, 3, 32, 32), "value")
    with pytest.raises(ValueError, match="mode"):
        vit.forward_dense(m._net, torch.zeros(1, 3, 32, 32), "vv")
    with pytest.raises(ValueError, match="projection head"):
        vit.forward_dense(vit.prepare(vit.make_state_dict(vit.ViTConfig(depth=1)), vit.ViTConfig(depth=1)),
                          torch.zeros(1, 3, 224, 224), "kk")


# ------------------------------------------------------- the model-level tolerances of tests/test_gpu_clip_dense.py
@functools.lru_cache(maxsize=None)
def _oracles(preset: str, shape: tuple[int, int], tokens: int) -> tuple[int, dict, dict]:
    """(E, float32 oracle per mode, fp16-operand oracle per mode), unit-norm cells [B h w, E]."""
    cfg, sd = co.shallow(preset)
    x = co.preprocess_reference(co.model_images(co.MODEL_BATCH, *shape, seed=tokens))
    kw = dict(patch=cfg.vision.patch_size, heads=cfg.vision.heads, act=cfg.vision.act)
    with torch.no_grad():
        want = {m: do.unit_cells(do.clip_dense_features(sd, x, mode=m, **kw)) for m in do.MODES}
        want16 = {m: do.unit_cells(do.clip_dense_features(sd, x, mode=m, round_operands_fp16=True, **kw)) for m in do.MODES}
    assert want["kk"].shape == (co.MODEL_BATCH * (tokens - 1), cfg.embed_dim)
    return cfg.embed_dim, want, want16


@pytest.mark.parametrize("preset,shape,grid,max_patches,tokens", do.DENSE_CASES)
def test_fp16_operand_dense_oracle_is_well_inside_its_bound(preset, shape, grid, max_patches, tokens):
    e, want, want16 = _oracles(preset, shape, tokens)
    bound = 2e-3 * math.sqrt(768 / e)
    for mode in do.MODES:
        err = (want[mode] - want16[mode]).abs().max().item()
        print(f"dense CLIP {preset} {mode} {shape} (T = {tokens}): fp16-operand oracle to float32 oracle {err:.3e}, "
              f"bound {bound:.2e}, ratio {err / bound:.3f}")
        assert err < bound / 5


@pytest.mark.parametrize("preset,shape,grid,max_patches,tokens", do.DENSE_CASES)
def test_the_modes_are_further_apart_than_twice_the_loose_bound(preset, shape, grid, max_patches, tokens):
    """What lets the GPU test tell the modes apart: a kernel that ran another mode is outside the 1e-2 bound by a factor."""
    e, want, _ = _oracles(preset, shape, tokens)
    loose = 1e-2 * math.sqrt(768 / e)
    for a, b in itertools.combinations(do.MODES, 2):
        gap = (want[a] - want[b]).abs().max().item()
        print(f"dense CLIP {preset} (T = {tokens}) {a} vs {b}: {gap:.3e} = {gap / loose:.2f} x the loose bound")
        assert gap >= 2 * loose


def test_the_dense_oracle_differs_from_a_transposed_map_and_from_the_class_token():
    """The 4 x 6 case: reading the cells column-major is another map; and the dense cells are not the class feature."""
    preset, shape, _grid, _mp, tokens = do.DENSE_CASES[1]
    cfg, sd = co.shallow(preset)
    x = co.preprocess_reference(co.model_images(co.MODEL_BATCH, *shape, seed=tokens))
    kw = dict(patch=cfg.vision.patch_size, heads=cfg.vision.heads)
    with torch.no_grad():
        m = do.clip_dense_features(sd, x, mode="kk", **kw)
    assert m.shape == (co.MODEL_BATCH, cfg.embed_dim, 4, 6)
    swapped = m.reshape(co.MODEL_BATCH, cfg.embed_dim, 6, 4).transpose(2, 3)
    loose = 1e-2 * math.sqrt(768 / cfg.embed_dim)
    assert (do.unit_cells(m) - do.unit_cells(swapped.contiguous())).abs().max().item() > 2 * loose


# ---------------------------------------------------------------------------------------------- the self operands
def test_rewritten_makes_query_key_attention_the_self_attention():
    qkv = vb.random_case(2, 19, 3, 0.5, seed=5)
    d = 3 * 64
    for part in (do.PART_QUERY, do.PART_KEY):
        rw = do.rewritten(do.poisoned(qkv, part), part)
        assert not torch.isnan(rw).any()
        z = qkv[..., part * d : (part + 1) * d]
        assert torch.equal(rw[..., :d], z) and torch.equal(rw[..., d : 2 * d], z) and torch.equal(rw[..., 2 * d :], qkv[..., 2 * d :])
        # ... and a float64 self attention written out directly is `attention_reference` of it
        zz, v = (t.double().reshape(2, 19, 3, 64).transpose(1, 2) for t in (z, qkv[..., 2 * d :]))
        direct = (torch.softmax(zz @ zz.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(2, 19, d)
        want, _bound = vb.attention_reference(rw, 3)
        torch.testing.assert_close(want, direct, rtol=1e-12, atol=1e-12)
    assert torch.isnan(do.poisoned(qkv, do.PART_KEY)[..., :d]).all() and torch.isnan(do.poisoned(qkv, do.PART_QUERY)[..., d : 2 * d]).all()


@pytest.mark.parametrize("part", [do.PART_QUERY, do.PART_KEY], ids=["qq", "kk"])
@pytest.mark.parametrize("t", [1, 17, 224, 257])
def test_self_selector_restated_equals_the_values(t, part):
    c = do.self_selector_case(2, t, 3, seed=7000 + t, part=part)
    d = 3 * 64
    assert c["gap"] >= vb.MIN_GAP and c["want"].shape == (2, t, d)
    other = 1 - part
    assert torch.isnan(c["qkv"][..., other * d : (other + 1) * d]).all()
    assert c["qkv"][..., part * d : (part + 1) * d].abs().eq(4).all()
    got = vb.attention_restated(do.rewritten(c["qkv"], part), 3)
    assert torch.equal(got, c["want"])
    if t > 1:  # a kernel that read the values of a neighbouring row is another tensor
        assert not torch.equal(vb.attention_restated(do.rewritten(c["qkv"], part), 3, swap_values=0), c["want"])
