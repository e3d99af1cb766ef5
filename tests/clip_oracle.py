"""CPU restatements for the CLIP towers and their kernels (test infrastructure, next to tests/dinov2_oracle.py and
tests/vit_bounds.py; a helper, not a conftest).

 * `clip_image_features`, `clip_text_features`: both towers in plain float32 torch under `imagescry_amd.clip`'s state-dict
   names (`visual.*`, `text.*`), pinned against `transformers.CLIPModel` in tests/test_clip_host.py.
 * `causal_attention_reference`: row i of (want, bound) is row i of `vit_bounds.attention_reference(qkv[:, : i + 1])`.
   Causal attention on a prefix IS plain attention on that prefix, and the derived bound's key counts (224 products per
   sum, 226 terms in SIGMA) are upper limits that a prefix of at most 128 keys respects.
 * `quick_gelu_bound`: the element-wise bound of the ISC_ACT_QUICK_GELU epilogue, derived here.

QuickGELU epilogue.  Notation of vit_bounds (u = 2^-24, a hardware transcendental documented to one ulp has 2 u).  The
pre-activation v (accumulator + bias) is exact with the quanta of `vit_bounds.gemm_case`; the kernel computes, in float32
(include/imagescry_hip.h),

    y = fl(v c)             c = fl(-1.702 log2 e): the constant's rounding u, the product's u       |dy| <= 2 u |y|
    t = exp2(y)             = exp(-1.702 v) (1 + theta):  the argument's error enters as ln 2 |dy| = 2 u * 1.702 |v|,
                            the instruction's own error is 2 u                  |theta| <= tau = 2 u (1 + 1.702 |v|)
    d = fl(1 + t)           relative error  t / (1 + t) tau + u  =  (1 - s) tau + u,   s = sigmoid(1.702 v) = 1 / (1 + t)
    r = rcp(d)              one ulp: 2 u
    out = fl(v r)           u

    |out - v s| <= SLACK |v s| u (4 + 2 (1 - s) (1 + 1.702 |v|))

(SLACK = 1.01 for the second-order products, as everywhere in vit_bounds).  For v -> -inf the factor grows like |v| while
v s vanishes like |v| e^{-1.702 |v|}; for v -> +inf, 1 - s vanishes and the bound is 4 u |v|.  Where exp2 saturates
(|y| > 126, |v| > 51) the result is exactly -0 or v, and v s is within 1e-37 of either.  A float32 residual added
afterwards is one more rounding, u (|want| + bound); an fp16 output one fp16 rounding, h (|want| + bound) + 2^-25.  The
erf GELU differs from QuickGELU by up to 0.02 and SiLU (x sigmoid(x)) by up to 0.1 on [-8, 8]: four orders of magnitude
outside this bound.
"""

from __future__ import annotations

import sys
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

import vit_bounds as vb  # noqa: E402
from dinov2_oracle import interpolate_pos_embed  # noqa: E402

QUICK_GELU_ALPHA = 1.702


# ------------------------------------------------------------------------------------------------------ QuickGELU
def quick_gelu_f64(v: Tensor) -> Tensor:
    v = v.double()
    return v * torch.sigmoid(QUICK_GELU_ALPHA * v)


def quick_gelu_bound(v: Tensor, *, out_f16: bool, residual: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """(want, bound) for quick_gelu(v) (+ residual) out of the epilogue, `v` the exact pre-activation (module docstring)."""
    v = v.double()
    s = torch.sigmoid(QUICK_GELU_ALPHA * v)
    one_minus_s = torch.sigmoid(-QUICK_GELU_ALPHA * v)  # keeps its digits where s is close to 1
    want = v * s
    bound = vb.SLACK * want.abs() * vb.U * (4 + 2 * one_minus_s * (1 + QUICK_GELU_ALPHA * v.abs()))
    if residual is not None:
        want = want + residual.double()
        bound = bound + vb.U * (want.abs() + bound)
    if out_f16:
        bound = bound + vb.H * (want.abs() + bound) + vb.TINY16
    return want, bound


def quick_gelu_restated_f32(v: Tensor) -> Tensor:
    """QuickGELU in float32 torch in another order than the kernel's: a division by 1 + exp(-1.702 v)."""
    v = v.float()
    return v / (1.0 + torch.exp(-QUICK_GELU_ALPHA * v))


def _act(name: str):
    if name == "quick_gelu":
        return lambda x: x * torch.sigmoid(QUICK_GELU_ALPHA * x)
    if name == "gelu":
        return F.gelu
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ causal attention
def causal_attention_reference(qkv: Tensor, heads: int) -> tuple[Tensor, Tensor]:
    """(want, bound), float64 [B, T, D], for causal attention on fp16 `qkv` [B, T, 3 D]: row i from the prefix 0 .. i."""
    b, t, _ = qkv.shape
    want = torch.empty(b, t, heads * 64, dtype=torch.float64)
    bound = torch.empty_like(want)
    for i in range(t):
        w, bd = vb.attention_reference(qkv[:, : i + 1], heads)
        want[:, i], bound[:, i] = w[:, i], bd[:, i]
    return want, bound


# ------------------------------------------------------------------------------------------------------ the towers
def _blocks(sd: dict[str, Tensor], prefix: str, tok: Tensor, heads: int, eps: float, act: str, causal: bool, r) -> Tensor:
    b, t, d = tok.shape
    fn = _act(act)
    depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(f"{prefix}.blocks."))
    mask = torch.full((t, t), float("-inf")).triu(1) if causal else None
    for i in range(depth):
        p = f"{prefix}.blocks.{i}"
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], eps)
        qkv = F.linear(r(h), r(sd[f"{p}.attn.qkv.weight"]), sd[f"{p}.attn.qkv.bias"])
        qkv = r(qkv).reshape(b, t, 3, heads, d // heads).permute(2, 0, 3, 1, 4)  # [3, B, H, T, 64]
        q, k, v = qkv[0], qkv[1], qkv[2]
        s = (q @ k.transpose(-1, -2)) * (d // heads) ** -0.5
        att = torch.softmax(s if mask is None else s + mask, dim=-1)
        a = (r(att) @ v).transpose(1, 2).reshape(b, t, d)
        tok = tok + F.linear(r(a), r(sd[f"{p}.attn.proj.weight"]), sd[f"{p}.attn.proj.bias"])
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"], eps)
        h = fn(F.linear(r(h), r(sd[f"{p}.mlp.fc1.weight"]), sd[f"{p}.mlp.fc1.bias"]))
        tok = tok + F.linear(r(h), r(sd[f"{p}.mlp.fc2.weight"]), sd[f"{p}.mlp.fc2.bias"])
    return tok


def _rounding(round_operands_fp16: bool):
    return (lambda t: t.half().float()) if round_operands_fp16 else (lambda t: t)


def clip_image_features(sd: dict[str, Tensor], x: Tensor, *, patch: int, heads: int, eps: float = 1e-5,
                        act: str = "quick_gelu", round_operands_fp16: bool = False) -> Tensor:
    """float32 `[B, 3, P h, P w]` -> float32 `[B, E]`, the projected class token (not normalised).  The position table
    is resampled by plain bicubic interpolation to the input's grid (`interpolate_pos_encoding` of transformers).
    `round_operands_fp16`: every matrix-product operand is rounded to fp16 first, as the kernels round theirs."""
    r = _rounding(round_operands_fp16)
    d = sd["visual.cls_token"].shape[-1]
    b = x.shape[0]
    grid = (x.shape[2] // patch, x.shape[3] // patch)
    tok = F.conv2d(r(x), r(sd["visual.patch_embed.proj.weight"]), sd["visual.patch_embed.proj.bias"], stride=patch)
    tok = tok.flatten(2).transpose(1, 2)
    tok = torch.cat([sd["visual.cls_token"].expand(b, -1, -1), tok], dim=1) + interpolate_pos_embed(sd["visual.pos_embed"], grid)
    tok = F.layer_norm(tok, (d,), sd["visual.norm_pre.weight"], sd["visual.norm_pre.bias"], eps)
    tok = _blocks(sd, "visual", tok, heads, eps, act, False, r)
    pooled = F.layer_norm(tok[:, 0], (d,), sd["visual.norm.weight"], sd["visual.norm.bias"], eps)
    return F.linear(r(pooled), r(sd["visual.head.weight"]))


def pooled_positions(ids: Tensor, eos_token_id: int | None) -> Tensor:
    """Per sequence: the first position holding `eos_token_id`; without one (None, or absent from the row) the first
    position of the largest id."""
    pos = ids.argmax(dim=1)  # the first maximum
    if eos_token_id is not None:
        hit = ids == eos_token_id
        pos = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), pos)
    return pos


def clip_text_features(sd: dict[str, Tensor], ids: Tensor, *, heads: int, eps: float = 1e-5, act: str = "quick_gelu",
                       eos_token_id: int | None = None, round_operands_fp16: bool = False) -> Tensor:
    """int64 `[Q, T]` -> float32 `[Q, E]`, the projected end-of-text token (not normalised)."""
    r = _rounding(round_operands_fp16)
    q, t = ids.shape
    d = sd["text.pos_embed"].shape[-1]
    tok = sd["text.token_embedding.weight"][ids] + sd["text.pos_embed"][:t]
    tok = _blocks(sd, "text", tok, heads, eps, act, True, r)
    tok = F.layer_norm(tok, (d,), sd["text.norm.weight"], sd["text.norm.bias"], eps)
    pooled = tok[torch.arange(q), pooled_positions(ids, eos_token_id)]
    return F.linear(r(pooled), r(sd["text.head.weight"]))


# ------------------------------------------------------------------------ the model-level cases of the GPU tests
# (preset, image shape, grid mode, max_patches, tokens): ViT-B/32 (T = 50), ViT-B/16 (197), ViT-L/14 (257: streaming
# attention) on their native grids, and a 4 x 6 aspect grid (25 tokens, resampled position table).  The images already
# have the grid's size, so preprocessing is the normalisation alone.
IMAGE_CASES = [("ViT-B/32", (224, 224), "fixed", None, 50), ("ViT-B/16", (224, 224), "fixed", None, 197),
               ("ViT-L/14", (224, 224), "fixed", None, 257), ("ViT-B/16", (64, 96), "aspect", 24, 25)]
TEXT_CASES = [("ViT-B/16", 77), ("ViT-B/16", 20), ("ViT-L/14", 77), ("ViT-L/14", 20)]  # both tower sizes
MODEL_DEPTH = 2
MODEL_BATCH = 2
TEXT_QUERIES = 16


def model_images(batch: int, h: int, w: int, seed: int) -> Tensor:
    return torch.randint(0, 256, (batch, 3, h, w), dtype=torch.uint8, generator=vb.gen(seed))


def preprocess_reference(images: Tensor) -> Tensor:
    """CLIP's fixed normalisation of uint8 images that already have the input size, float32."""
    from imagescry_amd import clip

    mean = torch.tensor(clip.IMAGE_MEAN).reshape(1, 3, 1, 1) * 255.0
    std = torch.tensor(clip.IMAGE_STD).reshape(1, 3, 1, 1) * 255.0
    return (images.float() - mean) / std


def text_ids(queries: int, t: int, vocab: int, seed: int) -> tuple[Tensor, Tensor]:
    """(ids [queries, t], EOT positions): random ids below the end-of-text id `vocab - 1`, one EOT a sequence at
    positions spread over 1 .. t - 1 (the first at 1, the last at t - 1), zeros behind it as the tokenizer pads."""
    g = vb.gen(seed)
    ids = torch.randint(1, vocab - 1, (queries, t), generator=g)
    eot = torch.linspace(1, t - 1, queries).round().long()
    for i, e in enumerate(eot.tolist()):
        ids[i, e] = vocab - 1
        ids[i, e + 1 :] = 0
    return ids, eot


def shallow(preset: str, act: str = "quick_gelu"):
    """(config at MODEL_DEPTH layers a tower, seeded state dict with random biases and LayerNorm affines)."""
    import dataclasses

    from imagescry_amd import clip

    cfg = clip.PRESETS[preset]
    cfg = clip.with_act(clip.CLIPConfig(dataclasses.replace(cfg.vision, depth=MODEL_DEPTH),
                                        dataclasses.replace(cfg.text, depth=MODEL_DEPTH)), act)
    return cfg, clip.make_state_dict(cfg, seed=len(preset) + cfg.embed_dim, randomize_affine=True)
