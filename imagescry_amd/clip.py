"""CLIP: an image tower and a text tower that embed into one space, so that a text query can search an image bank.

The image tower is the `vit` encoder on a `ViTConfig` with `pre_norm` (a LayerNorm between the token assembly and the
first block), `act` ("quick_gelu" for the OpenAI checkpoints, "gelu" for open_clip / LAION ones) and `embed_dim` (the
bias-free projection behind the class token's LayerNorm).  The text tower is the same pre-LN block over a residual stream
gathered from a token-embedding table (`isc_text_embed`), with CAUSAL attention (`isc_attention_f16_causal`), pooled at
the end-of-text token through the final LayerNorm (`isc_text_pool_layernorm`) and projected without bias.

State dicts are flat: `visual.*` holds the `vit` names plus `norm_pre.*` and `head.weight` `[E, D]`; `text.*` holds
`token_embedding.weight` `[vocab, D]`, `pos_embed` `[context, D]`, `blocks.i.*` as in `vit`, `norm.*` (the final
LayerNorm) and `head.weight` `[E, D]`.  `from_transformers_state_dict` and `from_openai_state_dict` convert a Hugging
Face `CLIPModel` and an OpenAI / open_clip checkpoint.  There is no tokenizer here: the text side takes token ids.
"""

from __future__ import annotations

from dataclasses import dataclass, field, replace

import torch
from torch import Tensor

from imagescry_amd import _lib, vit
from imagescry_amd.vit import Block, Linear, Norm, ViTConfig

# the fixed preprocessing statistics of every CLIP checkpoint, for pixels in 0 .. 1
IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_CONTEXT = 128  # isc_attention_f16_causal holds a head's keys whole up to here


@dataclass(frozen=True)
class CLIPTextConfig:
    dim: int = 512
    depth: int = 12
    heads: int = 8
    mlp_dim: int = 2048
    embed_dim: int = 512
    context: int = 77
    vocab: int = 49408
    ln_eps: float = 1e-5
    act: str = "quick_gelu"
    # pooling: the first position holding this id; None: the first position of the largest id (OpenAI's `argmax` -- the
    # end-of-text token is the tokenizer's largest id, so the two rules agree on its output)
    eos_token_id: int | None = None


@dataclass(frozen=True)
class CLIPConfig:
    vision: ViTConfig
    text: CLIPTextConfig

    @property
    def embed_dim(self) -> int:
        return self.text.embed_dim


def _preset(image: int, patch: int, width: int, depth: int, heads: int, text_width: int, text_heads: int,
            embed: int) -> CLIPConfig:
    return CLIPConfig(
        ViTConfig(image_size=image, patch_size=patch, dim=width, depth=depth, heads=heads, mlp_dim=4 * width, ln_eps=1e-5,
                  pre_norm=True, act="quick_gelu", embed_dim=embed),
        CLIPTextConfig(dim=text_width, depth=12, heads=text_heads, mlp_dim=4 * text_width, embed_dim=embed))


PRESETS: dict[str, CLIPConfig] = {
    "ViT-B/32": _preset(224, 32, 768, 12, 12, 512, 8, 512),
    "ViT-B/16": _preset(224, 16, 768, 12, 12, 512, 8, 512),
    "ViT-L/14": _preset(224, 14, 1024, 24, 16, 768, 12, 768),
    "ViT-L/14@336": _preset(336, 14, 1024, 24, 16, 768, 12, 768),
}


def with_act(cfg: CLIPConfig, act: str) -> CLIPConfig:
    """`cfg` with both towers' MLP activation set to `act` ("quick_gelu" or "gelu": a property of the checkpoint)."""
    if act not in vit.ACTIVATIONS:
        raise ValueError(f"act must be one of {sorted(vit.ACTIVATIONS)}, got {act!r}")
    return CLIPConfig(replace(cfg.vision, act=act), replace(cfg.text, act=act))


def make_state_dict(cfg: CLIPConfig, *, seed: int = 0, randomize_affine: bool = False) -> dict[str, Tensor]:
    """Seeded random parameters for both towers (CPU float32), drawn as `vit.make_state_dict` draws them; the patch
    embedding has no bias in CLIP, so `visual.patch_embed.proj.bias` is zero."""
    sd = {f"visual.{k}": v for k, v in vit.make_state_dict(cfg.vision, seed=seed, randomize_affine=randomize_affine).items()}
    sd["visual.patch_embed.proj.bias"] = torch.zeros(cfg.vision.dim)
    t = cfg.text
    # the text blocks and the final LayerNorm are those of an encoder of the text tower's shape
    shape = ViTConfig(image_size=16, patch_size=16, dim=t.dim, depth=t.depth, heads=t.heads, mlp_dim=t.mlp_dim)
    for k, v in vit.make_state_dict(shape, seed=seed + 1, randomize_affine=randomize_affine).items():
        if k.startswith(("blocks.", "norm.")):
            sd[f"text.{k}"] = v
    g = torch.Generator().manual_seed(seed + 2)
    sd["text.token_embedding.weight"] = torch.randn(t.vocab, t.dim, generator=g) * 0.02
    sd["text.pos_embed"] = torch.randn(t.context, t.dim, generator=g) * 0.01
    sd["text.head.weight"] = torch.randn(t.embed_dim, t.dim, generator=g) * t.dim**-0.5
    return sd


# ------------------------------------------------------------------------------------------------ checkpoint names
_HF_LAYER = (("norm1", "layer_norm1"), ("attn.proj", "self_attn.out_proj"), ("norm2", "layer_norm2"), ("mlp.fc1", "mlp.fc1"),
             ("mlp.fc2", "mlp.fc2"))
_OPENAI_LAYER = (("norm1", "ln_1"), ("attn.proj", "attn.out_proj"), ("norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                 ("mlp.fc2", "mlp.c_proj"))


def _affine(sd: dict[str, Tensor], ours: str, src: dict[str, Tensor], theirs: str) -> None:
    sd[f"{ours}.weight"], sd[f"{ours}.bias"] = src[f"{theirs}.weight"], src[f"{theirs}.bias"]


def from_transformers_state_dict(hf: dict[str, Tensor]) -> dict[str, Tensor]:
    """The state dict of a Hugging Face `CLIPModel` under this module's names: separate q / k / v projections fused into
    `attn.qkv` in `[q; k; v]` row order, `pre_layrnorm` (their spelling) -> `visual.norm_pre`, `post_layernorm` ->
    `visual.norm`, `final_layer_norm` -> `text.norm`, `visual_projection` / `text_projection` -> `head.weight`; a zero
    patch bias is supplied.  `logit_scale`, `position_ids` and anything else are dropped."""
    if "vision_model.embeddings.class_embedding" not in hf or "text_model.embeddings.token_embedding.weight" not in hf:
        raise ValueError("no `vision_model.*` / `text_model.*` keys: not a transformers CLIPModel state dict")
    sd: dict[str, Tensor] = {}
    d = hf["vision_model.embeddings.class_embedding"].shape[0]
    sd["visual.cls_token"] = hf["vision_model.embeddings.class_embedding"].reshape(1, 1, d)
    sd["visual.pos_embed"] = hf["vision_model.embeddings.position_embedding.weight"].unsqueeze(0)
    sd["visual.patch_embed.proj.weight"] = hf["vision_model.embeddings.patch_embedding.weight"]
    sd["visual.patch_embed.proj.bias"] = torch.zeros(d)
    _affine(sd, "visual.norm_pre", hf, "vision_model.pre_layrnorm")
    _affine(sd, "visual.norm", hf, "vision_model.post_layernorm")
    sd["visual.head.weight"] = hf["visual_projection.weight"]
    sd["text.token_embedding.weight"] = hf["text_model.embeddings.token_embedding.weight"]
    sd["text.pos_embed"] = hf["text_model.embeddings.position_embedding.weight"]
    _affine(sd, "text.norm", hf, "text_model.final_layer_norm")
    sd["text.head.weight"] = hf["text_projection.weight"]
    for ours, theirs in (("visual", "vision_model"), ("text", "text_model")):
        i = 0
        while f"{theirs}.encoder.layers.{i}.layer_norm1.weight" in hf:
            p, q = f"{ours}.blocks.{i}", f"{theirs}.encoder.layers.{i}"
            for a, b in _HF_LAYER:
                _affine(sd, f"{p}.{a}", hf, f"{q}.{b}")
            for kind in ("weight", "bias"):
                sd[f"{p}.attn.qkv.{kind}"] = torch.cat([hf[f"{q}.self_attn.{n}_proj.{kind}"] for n in "qkv"])
            i += 1
    return sd


def from_openai_state_dict(src: dict[str, Tensor]) -> dict[str, Tensor]:
    """An OpenAI / open_clip ViT checkpoint under this module's names.  `visual.proj` and `text_projection` are stored
    `[D, E]` there and transposed here; `attn.in_proj_weight` already is `[q; k; v]`; a zero patch bias is supplied.
    `logit_scale`, `attn_mask` and anything else are dropped."""
    if "visual.conv1.weight" not in src or "token_embedding.weight" not in src:
        raise ValueError("no `visual.conv1.weight` / `token_embedding.weight`: not an OpenAI CLIP ViT state dict")
    sd: dict[str, Tensor] = {}
    d = src["visual.class_embedding"].shape[0]
    sd["visual.cls_token"] = src["visual.class_embedding"].reshape(1, 1, d)
    sd["visual.pos_embed"] = src["visual.positional_embedding"].unsqueeze(0)
    sd["visual.patch_embed.proj.weight"] = src["visual.conv1.weight"]
    sd["visual.patch_embed.proj.bias"] = torch.zeros(d)
    _affine(sd, "visual.norm_pre", src, "visual.ln_pre")
    _affine(sd, "visual.norm", src, "visual.ln_post")
    sd["visual.head.weight"] = src["visual.proj"].t().contiguous()
    sd["text.token_embedding.weight"] = src["token_embedding.weight"]
    sd["text.pos_embed"] = src["positional_embedding"]
    _affine(sd, "text.norm", src, "ln_final")
    sd["text.head.weight"] = src["text_projection"].t().contiguous()
    for ours, theirs in (("visual", "visual.transformer"), ("text", "transformer")):
        i = 0
        while f"{theirs}.resblocks.{i}.ln_1.weight" in src:
            p, q = f"{ours}.blocks.{i}", f"{theirs}.resblocks.{i}"
            for a, b in _OPENAI_LAYER:
                _affine(sd, f"{p}.{a}", src, f"{q}.{b}")
            sd[f"{p}.attn.qkv.weight"], sd[f"{p}.attn.qkv.bias"] = src[f"{q}.attn.in_proj_weight"], src[f"{q}.attn.in_proj_bias"]
            i += 1
    return sd


def tower(sd: dict[str, Tensor], name: str) -> dict[str, Tensor]:
    """The keys of `sd` under `name.` ("visual" or "text") without that prefix."""
    out = {k[len(name) + 1 :]: v for k, v in sd.items() if k.startswith(name + ".")}
    if not out:
        raise ValueError(f"the state dict has no `{name}.*` keys")
    return out


# ---------------------------------------------------------------------------------------------------- the text tower
@dataclass
class PreparedText:
    cfg: CLIPTextConfig
    table: Tensor  # float32 [vocab, D]
    pos: Tensor  # float32 [context, D]
    blocks: list[Block] = field(default_factory=list)
    norm: Norm | None = None
    head: Linear | None = None  # [E, D], no bias

    def to(self, device: torch.device) -> "PreparedText":
        return PreparedText(self.cfg, self.table.to(device), self.pos.to(device), [b.to(device) for b in self.blocks],
                            self.norm.to(device), self.head.to(device))


def prepare_text(sd: dict[str, Tensor], cfg: CLIPTextConfig) -> PreparedText:
    """The text tower of `sd` (its `text.*` keys, prefix removed): GEMM weights fp16 and packed as `vit.prepare` stores
    them; the embedding table, positions, biases and LayerNorms float32."""
    if cfg.dim % 64 or cfg.mlp_dim % 64 or cfg.dim // cfg.heads != 64 or cfg.embed_dim % 4:
        raise ValueError("this build supports head size 64, GEMM inner dimensions that are multiples of 64 and an "
                         "embed_dim that is a multiple of 4")
    if not 1 <= cfg.context <= MAX_CONTEXT:
        raise ValueError(f"the causal attention kernel takes 1 .. {MAX_CONTEXT} tokens, got a context of {cfg.context}")
    if cfg.act not in vit.ACTIVATIONS:
        raise ValueError(f"act must be one of {sorted(vit.ACTIVATIONS)}, got {cfg.act!r}")
    for key, shape in (("token_embedding.weight", (cfg.vocab, cfg.dim)), ("pos_embed", (cfg.context, cfg.dim)),
                       ("head.weight", (cfg.embed_dim, cfg.dim))):
        if key not in sd or tuple(sd[key].shape) != shape:
            raise ValueError(f"text.{key} must have shape {shape}, got "
                             f"{tuple(sd[key].shape) if key in sd else 'no such key'}")
    return PreparedText(cfg, sd["token_embedding.weight"].float().contiguous(), sd["pos_embed"].float().contiguous(),
                        [vit.prepare_block(sd, f"blocks.{i}") for i in range(cfg.depth)], vit.prepare_norm(sd, "norm"),
                        vit.prepare_linear(sd, "head", bias=False))


def check_ids(ids: Tensor, cfg: CLIPTextConfig) -> None:
    """TypeError / ValueError unless `ids` is an int64 or int32 `[Q, T]` tensor with `1 <= T <= cfg.context`."""
    if not isinstance(ids, Tensor) or ids.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"ids must be an int64 or int32 tensor, got {getattr(ids, 'dtype', type(ids).__name__)}")
    if ids.ndim != 2:
        raise ValueError(f"ids must have shape [Q, T], got {tuple(ids.shape)}")
    if not 1 <= ids.shape[1] <= cfg.context:
        raise ValueError(f"sequences hold 1 .. {cfg.context} tokens, got T = {ids.shape[1]}")


def forward_text(net: PreparedText, ids: Tensor, *, validate: bool = True) -> Tensor:
    """int64 `[Q, T]` token ids on the net's HIP device, `T <= cfg.context` -> float32 `[Q, E]` text features (not
    normalised).  Sequences run in passes of `vit.PASS_ROWS // T`.  With `validate` a device word counts the ids outside
    `[0, vocab)` -- such a row is embedded as zeros, the table is never read out of range -- and is read ONCE, after the
    last pass: a non-zero count raises ValueError.  Without it there is no host read and the call can be captured."""
    cfg = net.cfg
    check_ids(ids, cfg)
    _lib.require_device(ids, "ids")
    if ids.device != net.table.device:
        raise ValueError(f"the text tower is on {net.table.device} but ids are on {ids.device}")
    ids = ids.to(torch.int64).contiguous()
    q, t = ids.shape
    d, dev = cfg.dim, ids.device
    out = torch.empty((q, cfg.embed_dim), dtype=torch.float32, device=dev)
    if q == 0:
        return out
    lib = _lib.load()
    step = max(1, vit.PASS_ROWS // t)
    eos = -1 if cfg.eos_token_id is None else cfg.eos_token_id
    with torch.cuda.device(dev):
        stream = _lib.stream_handle(dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev) if validate else None
        for q0 in range(0, q, step):
            part = ids[q0 : q0 + step]
            n = part.shape[0]
            xa = torch.empty((n * t, d), dtype=torch.float32, device=dev)
            xb = torch.empty_like(xa)
            _lib.check(lib.isc_text_embed(part.data_ptr(), n, t, cfg.vocab, d, net.table.data_ptr(), net.pos.data_ptr(),
                                          xa.data_ptr(), _lib.ptr(bad), stream), "isc_text_embed")
            xa = vit.run_blocks(net.blocks, xa, xb, n, t, heads=cfg.heads, mlp_dim=cfg.mlp_dim, ln_eps=cfg.ln_eps,
                                act=cfg.act, causal=True)
            pooled = torch.empty(vit.packed_elems(n, d), dtype=torch.float16, device=dev)
            _lib.check(lib.isc_text_pool_layernorm(xa.data_ptr(), part.data_ptr(), n, t, d, eos, net.norm.weight.data_ptr(),
                                                   net.norm.bias.data_ptr(), cfg.ln_eps, pooled.data_ptr(), _lib.ISC_F16, 1,
                                                   stream), "isc_text_pool_layernorm")
            vit._gemm(pooled, n, net.head, out[q0 : q0 + n], stream=stream)
        if validate:
            count = int(bad.item())
            if count:
                raise ValueError(f"{count} token id(s) outside [0, {cfg.vocab})")
    return out


__all__ = ["CLIPConfig", "CLIPTextConfig", "IMAGE_MEAN", "IMAGE_STD", "PRESETS", "PreparedText", "check_ids",
           "forward_text", "from_openai_state_dict", "from_transformers_state_dict", "make_state_dict", "prepare_text",
           "tower", "with_act"]
