"""Host side of the CLIP backbones: both tower oracles (tests/clip_oracle.py) against `transformers.CLIPModel`, the two
checkpoint conversions, `clip.make_state_dict` / `vit.prepare` / `clip.prepare_text` with the new parameters, the
`CLIPEmbedder` constructor and `encode_text` argument checks, the QuickGELU bound, and how far the fp16-operand oracle
lies from the float32 one on the cases of tests/test_gpu_clip.py.  CPU only."""

from __future__ import annotations

import dataclasses
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_oracle as co  # noqa: E402
import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402
from imagescry_amd import CLIPEmbedder, DINOv2Embedder, ViTB16Embedder, _lib, clip, vit  # noqa: E402

VOCAB, CONTEXT, EOS = 300, 16, 150


# ------------------------------------------------------------------------------------------ oracles vs transformers
def _hf_model(act: str, eos_token_id: int, image_size: int = 32):
    """A random-init two-layer CLIPModel of width 128 (two heads of 64) with every bias and affine randomised."""
    transformers = pytest.importorskip("transformers")
    common = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, projection_dim=64,
                  hidden_act=act)
    vc = transformers.CLIPVisionConfig(image_size=image_size, patch_size=16, **common)
    tc = transformers.CLIPTextConfig(vocab_size=VOCAB, max_position_embeddings=CONTEXT, eos_token_id=eos_token_id,
                                     bos_token_id=1, pad_token_id=0, **common)
    model = transformers.CLIPModel(transformers.CLIPConfig(text_config=tc, vision_config=vc, projection_dim=64)).eval()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # random init leaves biases at 0 and norms at the identity
        for name, p in model.named_parameters():
            if name.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif "norm" in name:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.75)
    return model


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("shape,interpolate", [((32, 48), True), ((32, 32), False)])
def test_image_oracle_matches_transformers(shape, interpolate, act):
    model = _hf_model(act, eos_token_id=2)
    sd = clip.from_transformers_state_dict(model.state_dict())
    assert sd["visual.blocks.1.attn.qkv.weight"].shape == (384, 128) and sd["visual.head.weight"].shape == (64, 128)
    assert not sd["visual.patch_embed.proj.bias"].any() and "logit_scale" not in sd
    x = torch.randn(2, 3, *shape, generator=torch.Generator().manual_seed(3)).clamp(-3, 3)
    with torch.no_grad():
        want = model.get_image_features(pixel_values=x, interpolate_pos_encoding=interpolate).pooler_output
        got = co.clip_image_features(sd, x, patch=16, heads=2, eps=model.config.vision_config.layer_norm_eps, act=act)
    assert got.shape == (2, 64)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


# EOT (id 150, NOT the largest id) at position 0, in the middle, last, and twice; ids above it in front of and behind it
def _text_cases() -> tuple[torch.Tensor, list[int]]:
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, VOCAB, (4, CONTEXT), generator=g)
    ids[ids == EOS] = EOS + 1
    first = [0, 7, CONTEXT - 1, 4]
    for row, at in enumerate(first):
        ids[row, at] = EOS
    ids[3, 11] = EOS  # a second one behind the first
    return ids, first


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("eos_set", [True, False], ids=["eos-id", "argmax"])
def test_text_oracle_matches_transformers(eos_set, act):
    # transformers pools at the first `eos_token_id`, except for the legacy value 2, where it pools at the largest id
    model = _hf_model(act, eos_token_id=EOS if eos_set else 2)
    sd = clip.from_transformers_state_dict(model.state_dict())
    ids, first = _text_cases()
    if not eos_set:  # the largest id stands where the EOT stood (and, in the last row, a second time behind it)
        ids = torch.where(ids == EOS, torch.tensor(VOCAB - 1), ids.clamp(max=VOCAB - 2))
    kw = dict(heads=2, eps=model.config.text_config.layer_norm_eps, act=act, eos_token_id=EOS if eos_set else None)
    assert co.pooled_positions(ids, kw["eos_token_id"]).tolist() == first
    with torch.no_grad():
        want = model.get_text_features(input_ids=ids).pooler_output
        got = co.clip_text_features(sd, ids, **kw)
        assert got.shape == (4, 64)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
        # a shorter sequence, and ids behind the (first) EOT: the output does not see them
        torch.testing.assert_close(co.clip_text_features(sd, ids[:, :9], **kw)[1:2],
                                   model.get_text_features(input_ids=ids[:, :9]).pooler_output[1:2], rtol=1e-5, atol=1e-5)
        other = ids.clone()
        for row, at in enumerate(first):
            other[row, at + 1 :] = torch.randint(3, EOS, (CONTEXT - at - 1,), generator=torch.Generator().manual_seed(row))
        assert not torch.equal(other, ids)
        assert torch.equal(co.clip_text_features(sd, other, **kw), got)


# ------------------------------------------------------------------------------------------------- the conversions
def _openai_names(sd: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
    """Our names -> the OpenAI / open_clip ones, by renaming and transposing the SAME tensors."""
    out = {"visual.conv1.weight": sd["visual.patch_embed.proj.weight"], "visual.class_embedding": sd["visual.cls_token"].reshape(-1),
           "visual.positional_embedding": sd["visual.pos_embed"][0], "visual.proj": sd["visual.head.weight"].t(),
           "token_embedding.weight": sd["text.token_embedding.weight"], "positional_embedding": sd["text.pos_embed"],
           "text_projection": sd["text.head.weight"].t(), "logit_scale": torch.tensor(4.6)}
    names = {"norm1": "ln_1", "attn.proj": "attn.out_proj", "norm2": "ln_2", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj"}
    for ours, theirs in (("visual.norm_pre", "visual.ln_pre"), ("visual.norm", "visual.ln_post"), ("text.norm", "ln_final")):
        for kind in ("weight", "bias"):
            out[f"{theirs}.{kind}"] = sd[f"{ours}.{kind}"]
    for tower, prefix in (("visual", "visual.transformer"), ("text", "transformer")):
        for i in range(2):
            for a, b in names.items():
                for kind in ("weight", "bias"):
                    out[f"{prefix}.resblocks.{i}.{b}.{kind}"] = sd[f"{tower}.blocks.{i}.{a}.{kind}"]
            for kind in ("weight", "bias"):
                out[f"{prefix}.resblocks.{i}.attn.in_proj_{kind}"] = sd[f"{tower}.blocks.{i}.attn.qkv.{kind}"]
    return out


def test_both_conversions_give_the_same_tensors():
    hf = _hf_model("quick_gelu", eos_token_id=2).state_dict()
    ours = clip.from_transformers_state_dict(hf)
    openai = _openai_names(ours)
    assert openai["visual.proj"].shape == (128, 64) and openai["text_projection"].shape == (128, 64)  # [D, E] there
    back = clip.from_openai_state_dict(openai)
    assert back.keys() == ours.keys()
    for k in ours:
        assert torch.equal(back[k], ours[k]), k
    q = hf["text_model.encoder.layers.1.self_attn.q_proj.weight"]
    assert torch.equal(ours["text.blocks.1.attn.qkv.weight"][:128], q)  # [q; k; v]
    assert torch.equal(ours["visual.norm_pre.bias"], hf["vision_model.pre_layrnorm.bias"])
    with pytest.raises(ValueError):
        clip.from_transformers_state_dict(openai)
    with pytest.raises(ValueError):
        clip.from_openai_state_dict(hf)
    # the converted dict is one the towers' `prepare` take
    cfg = clip.CLIPConfig(
        vit.ViTConfig(image_size=32, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=512, ln_eps=1e-5, pre_norm=True,
                      act="quick_gelu", embed_dim=64),
        clip.CLIPTextConfig(dim=128, depth=2, heads=2, mlp_dim=512, embed_dim=64, context=CONTEXT, vocab=VOCAB))
    net = vit.prepare(clip.tower(ours, "visual"), cfg.vision)
    assert net.head.bias is None and (net.head.out_features, net.head.in_features) == (64, 128)
    assert torch.equal(vit.unpack_rows(net.head.weight, 64, 128), hf["visual_projection.weight"].half())
    text = clip.prepare_text(clip.tower(ours, "text"), cfg.text)
    assert text.table.shape == (VOCAB, 128) and text.pos.shape == (CONTEXT, 128) and text.head.bias is None
    assert CLIPEmbedder(cfg, state_dict=ours).embedding_dim == 64


# --------------------------------------------------------------------------- make_state_dict, prepare, constructor
SMALL = clip.CLIPConfig(
    vit.ViTConfig(image_size=32, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=256, ln_eps=1e-5, pre_norm=True,
                  act="quick_gelu", embed_dim=64),
    clip.CLIPTextConfig(dim=128, depth=2, heads=2, mlp_dim=256, embed_dim=64, context=CONTEXT, vocab=VOCAB))


def test_make_state_dict_and_prepare():
    sd = clip.make_state_dict(SMALL, seed=3, randomize_affine=True)
    again = clip.make_state_dict(SMALL, seed=3, randomize_affine=True)
    assert sd.keys() == again.keys() and all(torch.equal(sd[k], again[k]) for k in sd)
    assert sd["visual.head.weight"].shape == (64, 128) and sd["text.head.weight"].shape == (64, 128)
    assert sd["text.token_embedding.weight"].shape == (VOCAB, 128) and sd["text.pos_embed"].shape == (CONTEXT, 128)
    assert not sd["visual.patch_embed.proj.bias"].any() and sd["visual.norm_pre.bias"].any()
    assert "visual.head.bias" not in sd and "text.head.bias" not in sd
    # the keys a plain ViT of the same shape has are the same tensors: the new parameters are drawn behind them
    plain = vit.make_state_dict(dataclasses.replace(SMALL.vision, pre_norm=False, embed_dim=0), seed=3, randomize_affine=True)
    assert all(torch.equal(sd[f"visual.{k}"], v) for k, v in plain.items() if k != "patch_embed.proj.bias")
    net = vit.prepare(clip.tower(sd, "visual"), SMALL.vision)
    assert torch.equal(net.norm_pre.weight, sd["visual.norm_pre.weight"]) and net.head.bias is None
    moved = net.to(torch.device("cpu"))
    assert torch.equal(moved.norm_pre.bias, net.norm_pre.bias) and torch.equal(moved.head.weight, net.head.weight)
    text = clip.prepare_text(clip.tower(sd, "text"), SMALL.text).to(torch.device("cpu"))
    assert len(text.blocks) == 2 and torch.equal(text.norm.weight, sd["text.norm.weight"])
    assert torch.equal(vit.unpack_rows(text.head.weight, 64, 128), sd["text.head.weight"].half())
    # what prepare refuses
    visual = clip.tower(sd, "visual")
    with pytest.raises(ValueError, match="norm_pre"):
        vit.prepare({k: v for k, v in visual.items() if not k.startswith("norm_pre")}, SMALL.vision)
    with pytest.raises(ValueError, match="head.weight"):
        vit.prepare({**visual, "head.weight": torch.zeros(32, 128)}, SMALL.vision)
    with pytest.raises(ValueError, match="act"):
        vit.prepare(visual, dataclasses.replace(SMALL.vision, act="relu"))
    with pytest.raises(ValueError, match="context"):
        clip.prepare_text(clip.tower(sd, "text"), dataclasses.replace(SMALL.text, context=129))
    with pytest.raises(ValueError, match="token_embedding"):
        clip.prepare_text(clip.tower(sd, "text"), dataclasses.replace(SMALL.text, vocab=VOCAB + 1))
    with pytest.raises(ValueError, match="visual"):
        clip.tower(clip.tower(sd, "text"), "visual")


def test_presets():
    want = {"ViT-B/32": (768, 12, 12, 50, 512, 8, 2048, 512), "ViT-B/16": (768, 12, 12, 197, 512, 8, 2048, 512),
            "ViT-L/14": (1024, 24, 16, 257, 768, 12, 3072, 768), "ViT-L/14@336": (1024, 24, 16, 577, 768, 12, 3072, 768)}
    assert clip.PRESETS.keys() == want.keys()
    for name, cfg in clip.PRESETS.items():
        v, t = cfg.vision, cfg.text
        assert (v.dim, v.depth, v.heads, v.tokens, t.dim, t.heads, t.mlp_dim, cfg.embed_dim) == want[name]
        assert v.dim // v.heads == 64 and t.dim // t.heads == 64 and t.depth == 12 and v.mlp_dim == 4 * v.dim
        assert (v.ln_eps, t.ln_eps, t.context, t.vocab, v.act, t.act) == (1e-5, 1e-5, 77, 49408, "quick_gelu", "quick_gelu")
        assert v.pre_norm and v.embed_dim == t.embed_dim and t.eos_token_id is None


def test_constructor_and_encode_text_argument_checks():
    sd = clip.make_state_dict(SMALL, seed=1)
    model = CLIPEmbedder(SMALL, state_dict=sd)
    assert model.embedding_dim == 64 and model.config == SMALL.vision and model.clip_config == SMALL
    assert CLIPEmbedder(SMALL, state_dict=sd, act="gelu").clip_config.text.act == "gelu"
    assert CLIPEmbedder(SMALL, state_dict=sd, act="gelu").config.act == "gelu"
    with pytest.raises(ValueError, match="preset"):
        CLIPEmbedder("ViT-H/14")
    with pytest.raises(ValueError, match="patches"):
        CLIPEmbedder(SMALL, state_dict=sd, output="patches")
    with pytest.raises(ValueError, match="act"):
        CLIPEmbedder(SMALL, state_dict=sd, act="tanh")
    with pytest.raises(ValueError, match="grid"):
        CLIPEmbedder(SMALL, state_dict=sd, grid="free")
    with pytest.raises(ValueError, match=r"\[Q, T\]"):
        model.encode_text(torch.zeros(CONTEXT, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[Q, T\]"):
        model.encode_text(torch.zeros(1, 2, CONTEXT, dtype=torch.int64))
    with pytest.raises(TypeError):
        model.encode_text(torch.zeros(2, CONTEXT))
    with pytest.raises(ValueError, match="T = 17"):
        model.encode_text(torch.zeros(2, CONTEXT + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="T = 0"):
        model.encode_text(torch.zeros(2, 0, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError):  # well-formed ids, but the module was never moved to a device
        model.encode_text(torch.zeros(2, CONTEXT, dtype=torch.int32))
    with pytest.raises(TypeError):
        model.preprocess(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        model.preprocess(torch.zeros(1, 1, 32, 32, dtype=torch.uint8))


def test_existing_configs_are_what_they_were():
    """The new fields have neutral defaults: every earlier preset compares equal to its definition without them."""
    assert vit.ViTConfig() == vit.ViTConfig(224, 16, 768, 12, 12, 3072, 1e-6, 0, False, False) == vit.VIT_B16
    assert vit.DINOV2_S14 == vit.ViTConfig(518, 14, 384, 12, 6, 1536, 1e-6, 0, True, False)
    assert vit.DINOV2_B14 == vit.ViTConfig(518, 14, 768, 12, 12, 3072, 1e-6, 0, True, False)
    assert vit.DINOV2_L14 == vit.ViTConfig(518, 14, 1024, 24, 16, 4096, 1e-6, 0, True, False)
    assert vit.DINOV2_S14_REG == vit.ViTConfig(518, 14, 384, 12, 6, 1536, 1e-6, 4, True, True)
    assert vit.DINOV2_B14_REG == vit.ViTConfig(518, 14, 768, 12, 12, 3072, 1e-6, 4, True, True)
    assert vit.DINOV2_L14_REG == vit.ViTConfig(518, 14, 1024, 24, 16, 4096, 1e-6, 4, True, True)
    for cfg in (vit.VIT_B16, vit.DINOV2_S14, vit.DINOV2_L14_REG):
        assert (cfg.pre_norm, cfg.act, cfg.embed_dim) == (False, "gelu", 0)
    net = ViTB16Embedder(config=dataclasses.replace(vit.VIT_B16, depth=1))._net
    assert net.norm_pre is None and net.head is None and net.patch.bias is not None
    assert ViTB16Embedder(config=dataclasses.replace(vit.VIT_B16, depth=1)).embedding_dim == 768
    assert DINOv2Embedder.embedding_dim.fget is ViTB16Embedder.embedding_dim.fget


# ---------------------------------------------------------------------------------------------- the QuickGELU bound
def _pre_activations() -> torch.Tensor:
    """The exact pre-activations of the GPU test's operands (quanta 2^-2 and 2^-3: multiples of 2^-5 in about [-8, 8])."""
    v = vb.gemm_case(77, 128, 384, seed=77 + 128 + 384, a_quantum=0.25, w_quantum=0.125, bias_top=32, res_top=64)["want"]
    assert float(v.min()) < -3 and float(v.max()) > 3
    return v


@pytest.mark.parametrize("out_f16", [False, True], ids=["f32", "f16"])
def test_quick_gelu_bound_holds_for_a_restatement_and_catches_other_activations(out_f16):
    v = _pre_activations()
    res = vb.gemm_case(77, 128, 384, seed=77 + 128 + 384, a_quantum=0.25, w_quantum=0.125, bias_top=32, res_top=64)["res"]
    cast = (lambda t: t.half()) if out_f16 else (lambda t: t)
    for residual in (None, res):
        want, bound = co.quick_gelu_bound(v, out_f16=out_f16, residual=residual)
        add = 0.0 if residual is None else residual
        got = cast(co.quick_gelu_restated_f32(v) + add)
        ratio = mb.assert_within_bound(got, want, bound, "QuickGELU restated in float32")
        print(f"QuickGELU restated, {'f16' if out_f16 else 'f32'}, residual {residual is not None}: error / bound = {ratio:.3f}")
        for name, fault in (("erf GELU", vb.gelu_restated_f32(v)), ("SiLU", v.float() * torch.sigmoid(v.float()))):
            worst, _ = mb.worst_ratio(cast(fault + add), want, bound)
            assert worst > 10, (name, worst)
    # saturation: -0 and v, never NaN, in the restatement and in the reference
    far = torch.tensor([-1e4, -200.0, 200.0, 1e4])
    assert torch.equal(co.quick_gelu_restated_f32(far), torch.tensor([-0.0, -0.0, 200.0, 1e4]))
    want, bound = co.quick_gelu_bound(far, out_f16=False)
    assert torch.isfinite(want).all() and torch.isfinite(bound).all()


# --------------------------------------------------------- the model-level tolerances of tests/test_gpu_clip.py
def _unit(x: torch.Tensor) -> torch.Tensor:
    return F.normalize(x, dim=1)


@pytest.mark.parametrize("preset,shape,grid,max_patches,tokens", co.IMAGE_CASES)
def test_fp16_operand_image_oracle_is_well_inside_its_bound(preset, shape, grid, max_patches, tokens):
    cfg, sd = co.shallow(preset)
    x = co.preprocess_reference(co.model_images(co.MODEL_BATCH, *shape, seed=tokens))
    kw = dict(patch=cfg.vision.patch_size, heads=cfg.vision.heads, act=cfg.vision.act)
    with torch.no_grad():
        want, want16 = _unit(co.clip_image_features(sd, x, **kw)), _unit(co.clip_image_features(sd, x, round_operands_fp16=True, **kw))
    bound = 2e-3 * math.sqrt(768 / cfg.embed_dim)
    err = (want - want16).abs().max().item()
    print(f"CLIP {preset} {shape} (T = {tokens}): fp16-operand oracle to float32 oracle {err:.3e}, bound {bound:.2e}, "
          f"ratio {err / bound:.3f}")
    assert err < bound / 5


@pytest.mark.parametrize("preset,t", co.TEXT_CASES)
def test_fp16_operand_text_oracle_is_well_inside_its_bound(preset, t):
    cfg, sd = co.shallow(preset)
    ids, _eot = co.text_ids(co.TEXT_QUERIES, t, cfg.text.vocab, seed=t)
    kw = dict(heads=cfg.text.heads, act=cfg.text.act)
    with torch.no_grad():
        want, want16 = _unit(co.clip_text_features(sd, ids, **kw)), _unit(co.clip_text_features(sd, ids, round_operands_fp16=True, **kw))
    bound = 2e-3 * math.sqrt(768 / cfg.embed_dim)
    err = (want - want16).abs().max().item()
    print(f"CLIP {preset} text T = {t}: fp16-operand oracle to float32 oracle {err:.3e}, bound {bound:.2e}, "
          f"ratio {err / bound:.3f}")
    assert err < bound / 5
