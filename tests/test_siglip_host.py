"""SigLIP on the host: the torch restatements of tests/siglip_oracle.py against `transformers.SiglipModel` (random weights,
nothing downloaded), the state-dict conversion, the preset table, seeded state dicts, the refusals, and the derived bounds
of the two new kernels checked on CPU restatements.  No GPU."""

from __future__ import annotations

import dataclasses
import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
import siglip_oracle as so  # noqa: E402
import vit_bounds as vb  # noqa: E402

from imagescry_amd import CLIPEmbedder, SigLIPEmbedder, ViTB16Embedder, _lib, siglip, vit  # noqa: E402

VOCAB, CONTEXT = 100, 16


# ------------------------------------------------------------------------------------------ oracles vs transformers
def _hf_model():
    """A random-init two-layer SiglipModel of width 128 (two heads of 64), 64 px / patch 16, with every bias and affine
    randomised."""
    transformers = pytest.importorskip("transformers")
    common = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2)
    cfg = transformers.SiglipConfig(text_config=dict(vocab_size=VOCAB, max_position_embeddings=CONTEXT, projection_size=128,
                                                     **common),
                                    vision_config=dict(image_size=64, patch_size=16, **common))
    model = transformers.SiglipModel(cfg).eval()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # random init leaves biases at 0 and norms at the identity
        for name, p in model.named_parameters():
            if name.endswith(("bias", "logit_scale")) and p.ndim == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05 + (2.0 if "logit" in name else 0.0))
            elif "norm" in name:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.75)
    assert cfg.vision_config.hidden_act == cfg.text_config.hidden_act == "gelu_pytorch_tanh"
    assert cfg.vision_config.layer_norm_eps == cfg.text_config.layer_norm_eps == so.LN_EPS
    return model


def _features(out) -> torch.Tensor:
    return getattr(out, "pooler_output", out)


@pytest.mark.parametrize("shape,interpolate", [((64, 64), False), ((48, 80), True)], ids=["native", "resampled"])
def test_image_oracle_matches_transformers(shape, interpolate):
    model = _hf_model()
    sd = siglip.from_transformers_state_dict(model.state_dict())
    x = torch.randn(2, 3, *shape, generator=torch.Generator().manual_seed(3)).clamp(-3, 3)
    with torch.no_grad():
        want = _features(model.get_image_features(pixel_values=x, interpolate_pos_encoding=interpolate))
        got = so.siglip_image_features(sd, x, patch=16, heads=2)
    assert got.shape == (2, 128)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_text_oracle_and_probability_match_transformers():
    model = _hf_model()
    sd = siglip.from_transformers_state_dict(model.state_dict())
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, VOCAB, (4, CONTEXT), generator=g)
    x = torch.randn(3, 3, 64, 64, generator=g).clamp(-3, 3)
    with torch.no_grad():
        want = _features(model.get_text_features(input_ids=ids))
        got = so.siglip_text_features(sd, ids, heads=2)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
        # a shorter sequence runs at its own length and pools ITS last position
        torch.testing.assert_close(so.siglip_text_features(sd, ids[:, :9], heads=2),
                                   _features(model.get_text_features(input_ids=ids[:, :9])), rtol=1e-5, atol=1e-5)
        out = model(input_ids=ids, pixel_values=x)
        q = torch.nn.functional.normalize(got, dim=1)
        r = torch.nn.functional.normalize(so.siglip_image_features(sd, x, patch=16, heads=2), dim=1)
    cos = q @ r.T
    want_p = torch.sigmoid(out.logits_per_text)
    scale, bias = float(sd["logit_scale"]), float(sd["logit_bias"])
    assert abs(scale - 2.0) < 0.5 and bias != 0.0  # the randomised values, not the initial ones
    torch.testing.assert_close(siglip.probability(cos, scale, bias), want_p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(so.probability(cos, sd).float(), want_p, rtol=1e-5, atol=1e-6)
    for p in (0.01, 0.5, 0.93):
        s = siglip.score_for_probability(p, scale, bias)
        assert abs(float(siglip.probability(torch.tensor(s, dtype=torch.float64), scale, bias)) - p) < 1e-12
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError, match="inside"):
            siglip.score_for_probability(bad, scale, bias)


def test_conversion_round_trip():
    model = _hf_model()
    hf = model.state_dict()
    sd = siglip.from_transformers_state_dict(hf)
    assert sd["visual.blocks.1.attn.qkv.weight"].shape == (384, 128) and sd["visual.pos_embed"].shape == (1, 16, 128)
    assert sd["visual.head.probe"].shape == (1, 1, 128) and sd["visual.head.attn.in_proj.weight"].shape == (384, 128)
    assert sd["text.head.weight"].shape == (128, 128) and sd["text.head.bias"].shape == (128,)
    assert sd["logit_scale"].shape == sd["logit_bias"].shape == (1,) and "visual.cls_token" not in sd
    for tw, theirs in (("visual", "vision_model"), ("text", "text_model")):
        for n, rows in (("q", slice(0, 128)), ("k", slice(128, 256)), ("v", slice(256, 384))):
            assert torch.equal(sd[f"{tw}.blocks.1.attn.qkv.weight"][rows], hf[f"{theirs}.encoder.layers.1.self_attn.{n}_proj.weight"])
            assert torch.equal(sd[f"{tw}.blocks.0.attn.qkv.bias"][rows], hf[f"{theirs}.encoder.layers.0.self_attn.{n}_proj.bias"])
    # every parameter of the model went somewhere: the converted dict holds as many numbers
    assert sum(v.numel() for v in sd.values()) == sum(p.numel() for p in model.parameters())
    cfg = siglip.SigLIPConfig(
        vit.ViTConfig(image_size=64, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=256, act="gelu_tanh", class_token=False),
        siglip.SigLIPTextConfig(dim=128, depth=2, heads=2, mlp_dim=256, context=CONTEXT, vocab=VOCAB))
    m = SigLIPEmbedder(cfg, state_dict=sd)
    assert m.embedding_dim == 128 and abs(m.logit_scale - float(hf["logit_scale"])) < 1e-7
    assert {k: tuple(v.shape) for k, v in siglip.make_state_dict(cfg).items()} == {k: tuple(v.shape) for k, v in sd.items()}
    with pytest.raises(ValueError, match="not a transformers SiglipModel"):
        siglip.from_transformers_state_dict({"visual.conv1.weight": torch.zeros(1)})


# ------------------------------------------------------------------------------------------------ configs and checks
def test_presets():
    assert len(siglip.PRESETS) == 12
    for name, cfg in siglip.PRESETS.items():
        v, t = cfg.vision, cfg.text
        large = name.startswith("ViT-L/16")
        assert (v.dim, v.depth, v.heads, v.mlp_dim) == ((1024, 24, 16, 4096) if large else (768, 12, 12, 3072)), name
        assert (t.dim, t.depth, t.heads, t.mlp_dim) == (v.dim, v.depth, v.heads, v.mlp_dim) and cfg.embed_dim == v.dim
        assert v.patch_size == 16 and not v.class_token and v.num_prefix == 0 and v.tokens == v.grid**2 and v.embed_dim == 0
        assert v.act == t.act == "gelu_tanh" and v.ln_eps == t.ln_eps == 1e-6 and not v.pre_norm and not v.layerscale
        assert (t.context, t.pad_token_id) == (64, 1) and t.vocab == (256000 if name.endswith("-siglip2") else 32000)
        size = int(name.split("@")[1].split("-")[0]) if "@" in name else 224
        assert v.image_size == size and v.dim // v.heads == 64
    assert sorted({c.vision.image_size for n, c in siglip.PRESETS.items() if n.startswith("ViT-B")}) == [224, 256, 384, 512]
    assert sorted({c.vision.image_size for n, c in siglip.PRESETS.items() if n.startswith("ViT-L")}) == [256, 384]
    assert siglip.IMAGE_MEAN == siglip.IMAGE_STD == (0.5, 0.5, 0.5)
    assert vit.ACTIVATIONS["gelu_tanh"] == _lib.ISC_ACT_GELU_TANH == 6


def _small() -> siglip.SigLIPConfig:
    return siglip.SigLIPConfig(
        vit.ViTConfig(image_size=64, patch_size=16, dim=128, depth=1, heads=2, mlp_dim=256, act="gelu_tanh", class_token=False),
        siglip.SigLIPTextConfig(dim=128, depth=1, heads=2, mlp_dim=256, context=CONTEXT, vocab=VOCAB))


def test_make_state_dict_and_prepare():
    cfg = _small()
    sd = siglip.make_state_dict(cfg, seed=3, randomize_affine=True)
    again = siglip.make_state_dict(cfg, seed=3, randomize_affine=True)
    assert sd.keys() == again.keys() and all(torch.equal(sd[k], again[k]) for k in sd)
    assert sd["visual.pos_embed"].shape == (1, 16, 128) and "visual.cls_token" not in sd
    assert sd["visual.head.mlp.fc1.weight"].shape == (256, 128) and sd["text.token_embedding.weight"].shape == (VOCAB, 128)
    assert float(sd["logit_scale"]) == pytest.approx(math.log(10.0)) and float(sd["logit_bias"]) == -10.0
    net = siglip.prepare_vision(siglip.tower(sd, "visual"), cfg.vision)
    enc = net.encoder
    assert enc.cls_token is None and enc.pos_embed.shape == (17, 128) and not enc.pos_embed[0].any()
    assert torch.equal(enc.pos_embed[1:], sd["visual.pos_embed"][0])
    # the probe's query: the float32 product, rounded once
    w, b = sd["visual.head.attn.in_proj.weight"], sd["visual.head.attn.in_proj.bias"]
    assert torch.equal(net.probe_q, (w[:128] @ sd["visual.head.probe"].reshape(128) + b[:128]).half())
    assert (net.kv.out_features, net.kv.in_features) == (256, 128)
    assert torch.equal(vit.unpack_rows(net.kv.weight, 256, 128), w[128:].half()) and torch.equal(net.kv.bias, b[128:])
    text = siglip.prepare_text(siglip.tower(sd, "text"), cfg.text)
    assert text.head.bias is not None and torch.equal(text.head.bias, sd["text.head.bias"]) and len(text.blocks) == 1
    moved = net.to(torch.device("cpu"))
    assert moved.encoder.cls_token is None and torch.equal(moved.probe_q, net.probe_q)
    broken = dict(siglip.tower(sd, "visual"))
    broken["head.probe"] = torch.zeros(1, 1, 64)
    with pytest.raises(ValueError, match="head.probe must have shape"):
        siglip.prepare_vision(broken, cfg.vision)
    # towers without a class token have no class-token outputs
    for fn in (vit.forward_cls, vit.forward_tokens):
        with pytest.raises(ValueError, match="needs a tower with a class token"):
            fn(enc, torch.zeros(1, 3, 64, 64))


def test_refusals():
    cfg = _small()
    # So400m: width 1152 with 16 heads is a head size of 72, and its MLP of 4304 is no multiple of 64
    so400m = siglip.SigLIPConfig(dataclasses.replace(cfg.vision, dim=1152, heads=16, mlp_dim=4304, depth=1),
                                 dataclasses.replace(cfg.text, dim=1152, heads=16, mlp_dim=4304, depth=1))
    with pytest.raises(ValueError, match="So400m.*NaFlex"):
        siglip.prepare_vision({}, so400m.vision)
    with pytest.raises(ValueError, match="So400m.*NaFlex"):
        siglip.prepare_text({}, so400m.text)
    with pytest.raises(ValueError, match="dense SigLIP map.*follow-up"):
        SigLIPEmbedder(cfg, output="patches")
    with pytest.raises(ValueError, match="preset must be one of"):
        SigLIPEmbedder("ViT-B/32")
    with pytest.raises(ValueError, match="preprocess must be"):
        SigLIPEmbedder(cfg, preprocess="crop")
    with pytest.raises(ValueError, match="max_patches needs"):
        SigLIPEmbedder(cfg, max_patches=64)
    with pytest.raises(ValueError, match="no class token"):
        siglip.prepare_vision({}, dataclasses.replace(cfg.vision, class_token=True))
    with pytest.raises(ValueError, match="pad_token_id"):
        siglip.prepare_text({}, dataclasses.replace(cfg.text, pad_token_id=VOCAB))
    model = SigLIPEmbedder(cfg, seed=1)
    assert model.hparams["preprocess"] == "squash" and model.embedding_dim == 128
    with pytest.raises(ValueError, match="1 .. 16 tokens"):
        model.encode_text(torch.zeros(2, CONTEXT + 1, dtype=torch.int64))
    with pytest.raises(TypeError, match="int64 or int32"):
        model.encode_text(torch.zeros(2, 4))
    with pytest.raises(ValueError, match=r"\[Q, T\]"):
        model.encode_text(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.HipLibraryError, match="call .to"):
        model.encode_text(torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(TypeError, match="uint8"):
        model.preprocess(torch.zeros(1, 3, 64, 64))


def test_pad_to_context_semantics():
    """Padding to the context IS running the padded row: the oracle on a short row padded by hand equals the oracle on
    `siglip.pad_ids`' row, differs from the unpadded run (another pooled position, no mask), and full rows are unchanged."""
    cfg = _small()
    sd = siglip.make_state_dict(cfg, seed=5, randomize_affine=True)
    ids = torch.randint(2, VOCAB, (3, 7), generator=vb.gen(1))
    padded = siglip.pad_ids(ids, cfg.text)
    assert padded.shape == (3, CONTEXT) and torch.equal(padded[:, :7], ids) and bool((padded[:, 7:] == cfg.text.pad_token_id).all())
    assert torch.equal(padded, so.pad_ids(ids, CONTEXT, 1)) and padded.dtype == ids.dtype
    assert siglip.pad_ids(padded, cfg.text) is padded
    assert siglip.pad_ids(ids.int(), cfg.text).dtype == torch.int32
    with torch.no_grad():
        long, short = so.siglip_text_features(sd, padded, heads=2), so.siglip_text_features(sd, ids, heads=2)
    assert (long - short).abs().max().item() > 1e-3
    other = dataclasses.replace(cfg.text, pad_token_id=0)
    assert bool((siglip.pad_ids(ids, other)[:, 7:] == 0).all())


def test_existing_configs_and_embedders_are_what_they_were():
    assert vit.VIT_B16.class_token and vit.VIT_B16.num_prefix == 1 and vit.DINOV2_B14_REG.num_prefix == 5
    assert vit.ACTIVATIONS["gelu"] == 2 and vit.ACTIVATIONS["quick_gelu"] == 5
    cfg = dataclasses.replace(vit.VIT_B16, depth=1)
    sd = vit.make_state_dict(cfg, seed=4)
    assert list(sd)[:4] == ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    g = torch.Generator().manual_seed(4)
    first = torch.nn.init.trunc_normal_(torch.empty(1, 1, 768), std=0.02, a=-0.04, b=0.04, generator=g)
    assert torch.equal(sd["cls_token"], first) and sd["pos_embed"].shape == (1, 197, 768)
    net = vit.prepare(sd, cfg)
    assert net.cls_token is not None and net.pos_embed.shape == (197, 768) and torch.equal(net.pos_embed, sd["pos_embed"][0])
    assert ViTB16Embedder(config=cfg, seed=4).embedding_dim == 768 and issubclass(SigLIPEmbedder, ViTB16Embedder)
    assert not issubclass(SigLIPEmbedder, CLIPEmbedder)


# ------------------------------------------------------------------------------------------ the bounds, on the CPU
@pytest.mark.parametrize("out_f16", [False, True])
def test_gelu_tanh_bound_holds_for_a_restatement_and_catches_the_erf_form(out_f16):
    """The kernel's operation sequence restated in float32 torch (exp2 as torch computes it) is inside the bound; the erf
    form and QuickGELU are outside it on the same pre-activations."""
    c = vb.gemm_case(77, 128, 384, seed=589, a_quantum=0.25, w_quantum=0.125, bias_top=32, res_top=64)
    v = c["want"]
    assert float(v.min()) < -3 and float(v.max()) > 3
    want, bound = so.gelu_tanh_bound(v, out_f16=out_f16)
    v32 = v.float()
    w = v32 * torch.addcmul(torch.ones_like(v32), v32 * v32, torch.tensor(0.044715))
    got = v32 * (1.0 / (1.0 + torch.exp2(w * -2.3022081851959229)))
    got = got.half() if out_f16 else got
    mb.assert_within_bound(got, want, bound, "restated")
    torch.testing.assert_close(want, torch.nn.functional.gelu(v, approximate="tanh"), rtol=1e-12, atol=1e-12)
    assert so.erf_is_outside(v, out_f16=out_f16) > 0.05 * v.numel()
    quick = v * torch.sigmoid(1.702 * v)
    assert int(((quick - want).abs() > bound).sum()) > 0.5 * v.numel()
    # saturation of the restated sequence: exactly 0 or v, never NaN
    big = torch.tensor([-3.0e4, -100.0, -12.0, 12.0, 100.0, 3.0e4, 6.0e4, -6.0e4, 0.0])
    wb = big * torch.addcmul(torch.ones_like(big), big * big, torch.tensor(0.044715))
    sat = big * (1.0 / (1.0 + torch.exp2(wb * -2.3022081851959229)))
    assert torch.equal(sat, torch.where(big > 0, big, torch.zeros_like(big)))


@pytest.mark.parametrize("t", [1, 17, 196])
def test_probe_bound_holds_for_a_restatement_and_catches_planted_faults(t):
    kv, q = so.probe_random_case(2, t, 2, 1.0, seed=t)
    want, bound = so.probe_reference(kv, q, 2)
    mb.assert_within_bound(so.probe_restated(kv, q, 2), want, bound, "restated")
    if t > 1:  # the key that image 0, head 0 weighs most goes missing
        top = int((kv[0, :, :64].double() @ q[:64].double()).argmax())
        ratio, _ = mb.worst_ratio(so.probe_restated(kv, q, 2, drop_key=top), want, bound)
        assert ratio > 1.0
    # a zero-filled padded key weighs something where the scores are flat (among peaked ones e^0 is nothing)
    kv, q = so.probe_random_case(2, t, 2, 0.25, seed=t)
    want, bound = so.probe_reference(kv, q, 2)
    mb.assert_within_bound(so.probe_restated(kv, q, 2), want, bound, "restated, flat")
    ratio, _ = mb.worst_ratio(so.probe_restated(kv, q, 2, extra_zero_keys=1), want, bound)
    assert ratio > 1.0
    u =so.probe_uniform_case(2, t, 2, seed=t)
    mb.assert_within_bound(so.probe_restated(u["kv"], u["q"], 2), u["want"], u["bound"], "uniform")
    ratio, _ = mb.worst_ratio(so.probe_restated(u["kv"], u["q"], 2, extra_zero_keys=1), u["want"], u["bound"])
    assert ratio > 1.0  # one padded key in the sum moves the divisor by 1 / T
    s = so.probe_selector_case(3, t, 2, seed=t)
    assert s["gap"] >= vb.MIN_GAP and torch.equal(so.probe_restated(s["kv"], s["q"], 2), s["want"])
    if t >= 3:
        assert sorted(s["pos"][:, 0].tolist()) == [0, t // 2, t - 1] and s["pos"][0, 0] != s["pos"][0, 1]


def test_interpolate_pos_is_the_identity_on_the_native_grid_and_resamples_otherwise():
    pos = torch.randn(16, 8, generator=vb.gen(2))
    assert so.interpolate_pos(pos, (4, 4)) is pos
    out = so.interpolate_pos(pos, (3, 5))
    assert out.shape == (15, 8)
    flat = so.interpolate_pos(torch.ones(16, 8), (3, 5))
    torch.testing.assert_close(flat, torch.ones(15, 8))
