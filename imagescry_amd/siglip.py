"""SigLIP / SigLIP 2 (ViT-B/16, ViT-L/16): an image tower and a text tower that embed into one space, with a per-pair
sigmoid score in place of CLIP's softmax.

The image tower is the `vit` encoder on a `ViTConfig` WITHOUT a class token (`class_token=False`: the tokens are the
patches plus their position rows, `isc_vit_assemble_plain`), tanh GELU (`act="gelu_tanh"`, `ISC_ACT_GELU_TANH`), LayerNorm
eps 1e-6, and behind the final LayerNorm the attention-pooling ("MAP") head:

    q    = in_proj[:D] probe + b[:D]               one vector for every image: computed ONCE in `prepare_vision`, in float32
                                                    from the float32 checkpoint, and rounded to fp16 there (the kernel
                                                    multiplies it by 1/8 exactly)
    k, v = in_proj[D:] LN_post(tokens) + b[D:]     one GEMM into a packed fp16 `[B T, 2 D]` operand
    a    = softmax(q k^T / 8) v   per head         `isc_attention_f16_probe`, fp16 `[B, D]`
    y    = out_proj a + b                          float32
    e    = y + fc2(gelu_tanh(fc1(LN(y))))          float32 `[B, D]`: the embedding, no projection matrix

The text tower is the same pre-LN block over `table[ids] + pos[:T]` (`isc_text_embed`) with BIDIRECTIONAL attention and no
padding mask (`isc_attention_f16`), pooled at the LAST position through the final LayerNorm (`isc_layernorm` on rows
`T - 1` of every sequence) and a Linear WITH bias.  The checkpoints were trained on rows padded to `context` with
`pad_token_id`, so position `context - 1` is the one they pool: `SigLIPEmbedder.encode_text` pads by default.

State dicts are flat: `visual.*` holds the `vit` names (no `cls_token`; `pos_embed` `[1, grid ** 2, D]`) plus `head.probe`
`[1, 1, D]`, `head.attn.in_proj.{weight, bias}` `[3 D, D]`, `head.attn.out_proj.*`, `head.norm.*`, `head.mlp.fc1.*`,
`head.mlp.fc2.*`; `text.*` holds `token_embedding.weight`, `pos_embed` `[context, D]`, `blocks.i.*`, `norm.*` and
`head.{weight, bias}`; `logit_scale` and `logit_bias` are one float each.  `from_transformers_state_dict` converts a
Hugging Face `SiglipModel`.  There is no tokenizer here: the text side takes token ids.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field, replace

import torch
from torch import Tensor

from imagescry_amd import _lib, vit
from imagescry_amd.vit import Block, Linear, Norm, PreparedViT, ViTConfig

# the fixed preprocessing statistics of every SigLIP checkpoint, for pixels in 0 .. 1
IMAGE_MEAN = (0.5, 0.5, 0.5)
IMAGE_STD = (0.5, 0.5, 0.5)
LN_EPS = 1e-6
UNSUPPORTED = ("this build supports head size 64 and widths that are multiples of 64: the So400m checkpoints (width 1152: "
               "head size 72, MLP 4304) and the NaFlex variants are not supported")


@dataclass(frozen=True)
class SigLIPTextConfig:
    dim: int = 768
    depth: int = 12
    heads: int = 12
    mlp_dim: int = 3072
    context: int = 64
    vocab: int = 32000
    ln_eps: float = LN_EPS
    act: str = "gelu_tanh"
    # what `encode_text(pad_to_context=True)` fills short rows with: 1 for the SigLIP sentencepiece vocabulary; a SigLIP 2
    # (Gemma tokenizer) user sets the id their tokenizer pads with
    pad_token_id: int = 1

    @property
    def embed_dim(self) -> int:
        return self.dim  # the head is a Linear(dim, dim)


@dataclass(frozen=True)
class SigLIPConfig:
    vision: ViTConfig
    text: SigLIPTextConfig

    @property
    def embed_dim(self) -> int:
        return self.text.embed_dim


def _preset(image: int, width: int, depth: int, heads: int, vocab: int = 32000) -> SigLIPConfig:
    return SigLIPConfig(
        ViTConfig(image_size=image, patch_size=16, dim=width, depth=depth, heads=heads, mlp_dim=4 * width, ln_eps=LN_EPS,
                  act="gelu_tanh", class_token=False),
        SigLIPTextConfig(dim=width, depth=depth, heads=heads, mlp_dim=4 * width, vocab=vocab))


_SHAPES = {"ViT-B/16": ((768, 12, 12), (224, 256, 384, 512)), "ViT-L/16": ((1024, 24, 16), (256, 384))}
# "ViT-B/16" (224), "ViT-B/16@256", ..., "ViT-L/16@256", "ViT-L/16@384"; "-siglip2": the 256000-entry vocabulary
PRESETS: dict[str, SigLIPConfig] = {}
for _name, (_shape, _sizes) in _SHAPES.items():
    for _size in _sizes:
        _key = _name if (_name, _size) == ("ViT-B/16", 224) else f"{_name}@{_size}"
        PRESETS[_key] = _preset(_size, *_shape)
        PRESETS[f"{_key}-siglip2"] = _preset(_size, *_shape, vocab=256000)


def _check_shape(dim: int, heads: int, mlp_dim: int) -> None:
    if dim % 64 or mlp_dim % 64 or heads <= 0 or dim % heads or dim // heads != 64:
        raise ValueError(f"{UNSUPPORTED} (got width {dim}, {heads} heads, MLP {mlp_dim})")


def make_state_dict(cfg: SigLIPConfig, *, seed: int = 0, randomize_affine: bool = False) -> dict[str, Tensor]:
    """Seeded random parameters for both towers (CPU float32), drawn as `vit.make_state_dict` draws them; the pooling head
    and the text head follow; `logit_scale` = log 10 and `logit_bias` = -10, the values training starts from."""
    sd = {f"visual.{k}": v for k, v in vit.make_state_dict(cfg.vision, seed=seed, randomize_affine=randomize_affine).items()}
    t = cfg.text
    shape = ViTConfig(image_size=16, patch_size=16, dim=t.dim, depth=t.depth, heads=t.heads, mlp_dim=t.mlp_dim)
    for k, v in vit.make_state_dict(shape, seed=seed + 1, randomize_affine=randomize_affine).items():
        if k.startswith(("blocks.", "norm.")):
            sd[f"text.{k}"] = v
    g = torch.Generator().manual_seed(seed + 2)

    def tn(*shape: int) -> Tensor:
        return torch.nn.init.trunc_normal_(torch.empty(*shape), std=0.02, a=-0.04, b=0.04, generator=g)

    def bias(n: int) -> Tensor:
        return torch.randn(n, generator=g) * 0.05 if randomize_affine else torch.zeros(n)

    sd["text.token_embedding.weight"] = torch.randn(t.vocab, t.dim, generator=g) * 0.02
    sd["text.pos_embed"] = torch.randn(t.context, t.dim, generator=g) * 0.01
    sd["text.head.weight"], sd["text.head.bias"] = torch.randn(t.dim, t.dim, generator=g) * t.dim**-0.5, bias(t.dim)
    d, m = cfg.vision.dim, cfg.vision.mlp_dim
    sd["visual.head.probe"] = torch.randn(1, 1, d, generator=g)  # a trained probe has entries of order one
    sd["visual.head.attn.in_proj.weight"], sd["visual.head.attn.in_proj.bias"] = tn(3 * d, d), bias(3 * d)
    sd["visual.head.attn.out_proj.weight"], sd["visual.head.attn.out_proj.bias"] = tn(d, d), bias(d)
    sd["visual.head.norm.weight"] = torch.rand(d, generator=g) * 0.5 + 0.75 if randomize_affine else torch.ones(d)
    sd["visual.head.norm.bias"] = bias(d)
    sd["visual.head.mlp.fc1.weight"], sd["visual.head.mlp.fc1.bias"] = tn(m, d), bias(m)
    sd["visual.head.mlp.fc2.weight"], sd["visual.head.mlp.fc2.bias"] = tn(d, m), bias(d)
    sd["logit_scale"], sd["logit_bias"] = torch.tensor([math.log(10.0)]), torch.tensor([-10.0])
    return sd


# ------------------------------------------------------------------------------------------------ checkpoint names
_HF_LAYER = (("norm1", "layer_norm1"), ("attn.proj", "self_attn.out_proj"), ("norm2", "layer_norm2"), ("mlp.fc1", "mlp.fc1"),
             ("mlp.fc2", "mlp.fc2"))


def _affine(sd: dict[str, Tensor], ours: str, src: dict[str, Tensor], theirs: str) -> None:
    sd[f"{ours}.weight"], sd[f"{ours}.bias"] = src[f"{theirs}.weight"], src[f"{theirs}.bias"]


def from_transformers_state_dict(hf: dict[str, Tensor]) -> dict[str, Tensor]:
    """The state dict of a Hugging Face `SiglipModel` under this module's names: separate q / k / v projections fused
    into `attn.qkv` in `[q; k; v]` row order, `post_layernorm` -> `visual.norm`, `head.attention.in_proj_*` ->
    `visual.head.attn.in_proj.*`, `head.layernorm` -> `visual.head.norm`, `final_layer_norm` -> `text.norm`; `logit_scale`
    and `logit_bias` are kept.  `position_ids` and anything else are dropped."""
    if "vision_model.head.probe" not in hf or "text_model.embeddings.token_embedding.weight" not in hf:
        raise ValueError("no `vision_model.head.probe` / `text_model.*` keys: not a transformers SiglipModel state dict")
    sd: dict[str, Tensor] = {}
    sd["visual.pos_embed"] = hf["vision_model.embeddings.position_embedding.weight"].unsqueeze(0)
    _affine(sd, "visual.patch_embed.proj", hf, "vision_model.embeddings.patch_embedding")
    _affine(sd, "visual.norm", hf, "vision_model.post_layernorm")
    sd["visual.head.probe"] = hf["vision_model.head.probe"]
    sd["visual.head.attn.in_proj.weight"] = hf["vision_model.head.attention.in_proj_weight"]
    sd["visual.head.attn.in_proj.bias"] = hf["vision_model.head.attention.in_proj_bias"]
    _affine(sd, "visual.head.attn.out_proj", hf, "vision_model.head.attention.out_proj")
    _affine(sd, "visual.head.norm", hf, "vision_model.head.layernorm")
    _affine(sd, "visual.head.mlp.fc1", hf, "vision_model.head.mlp.fc1")
    _affine(sd, "visual.head.mlp.fc2", hf, "vision_model.head.mlp.fc2")
    sd["text.token_embedding.weight"] = hf["text_model.embeddings.token_embedding.weight"]
    sd["text.pos_embed"] = hf["text_model.embeddings.position_embedding.weight"]
    _affine(sd, "text.norm", hf, "text_model.final_layer_norm")
    _affine(sd, "text.head", hf, "text_model.head")
    for ours, theirs in (("visual", "vision_model"), ("text", "text_model")):
        i = 0
        while f"{theirs}.encoder.layers.{i}.layer_norm1.weight" in hf:
            p, q = f"{ours}.blocks.{i}", f"{theirs}.encoder.layers.{i}"
            for a, b in _HF_LAYER:
                _affine(sd, f"{p}.{a}", hf, f"{q}.{b}")
            for kind in ("weight", "bias"):
                sd[f"{p}.attn.qkv.{kind}"] = torch.cat([hf[f"{q}.self_attn.{n}_proj.{kind}"] for n in "qkv"])
            i += 1
    sd["logit_scale"], sd["logit_bias"] = hf["logit_scale"].reshape(1), hf["logit_bias"].reshape(1)
    return sd


def tower(sd: dict[str, Tensor], name: str) -> dict[str, Tensor]:
    """The keys of `sd` under `name.` ("visual" or "text") without that prefix."""
    out = {k[len(name) + 1 :]: v for k, v in sd.items() if k.startswith(name + ".")}
    if not out:
        raise ValueError(f"the state dict has no `{name}.*` keys")
    return out


def _need(sd: dict[str, Tensor], prefix: str, key: str, shape: tuple[int, ...]) -> Tensor:
    if key not in sd or tuple(sd[key].shape) != shape:
        raise ValueError(f"{prefix}.{key} must have shape {shape}, got "
                         f"{tuple(sd[key].shape) if key in sd else 'no such key'}")
    return sd[key]


# --------------------------------------------------------------------------------------------------- the image tower
@dataclass
class PreparedVision:
    encoder: PreparedViT  # patches, position table, blocks, the final LayerNorm
    probe_q: Tensor  # fp16 [D]: in_proj[:D] probe + b[:D]
    kv: Linear  # [2 D, D]: rows [key; value] of in_proj
    out_proj: Linear
    norm: Norm
    fc1: Linear
    fc2: Linear

    @property
    def cfg(self) -> ViTConfig:
        return self.encoder.cfg

    def to(self, device: torch.device) -> "PreparedVision":
        return PreparedVision(self.encoder.to(device), self.probe_q.to(device), self.kv.to(device),
                              self.out_proj.to(device), self.norm.to(device), self.fc1.to(device), self.fc2.to(device))


def prepare_vision(sd: dict[str, Tensor], cfg: ViTConfig) -> PreparedVision:
    """The image tower of `sd` (its `visual.*` keys, prefix removed): the encoder as `vit.prepare` stores it, the head's
    GEMM weights fp16 and packed, and the probe's query (module docstring: float32 product, one rounding to fp16)."""
    _check_shape(cfg.dim, cfg.heads, cfg.mlp_dim)
    if cfg.class_token or cfg.registers or cfg.layerscale or cfg.pre_norm or cfg.embed_dim:
        raise ValueError("a SigLIP image tower has no class token, registers, LayerScale, pre-norm or projection")
    d = cfg.dim
    probe = _need(sd, "visual", "head.probe", (1, 1, d)).reshape(d).float()
    w = _need(sd, "visual", "head.attn.in_proj.weight", (3 * d, d)).float()
    b = _need(sd, "visual", "head.attn.in_proj.bias", (3 * d,)).float()
    q = (w[:d] @ probe + b[:d]).to(torch.float16).contiguous()
    return PreparedVision(vit.prepare(sd, cfg), q, vit.prepare_linear({"kv.weight": w[d:], "kv.bias": b[d:]}, "kv"),
                          vit.prepare_linear(sd, "head.attn.out_proj"), vit.prepare_norm(sd, "head.norm"),
                          vit.prepare_linear(sd, "head.mlp.fc1"), vit.prepare_linear(sd, "head.mlp.fc2"))


def forward_image(net: PreparedVision, x: Tensor, grid: tuple[int, int] | None = None,
                  max_patches: int | None = None) -> Tensor:
    """float32 `[B, 3, 16 h, 16 w]` (already preprocessed; `grid = (h, w)`, the native square grid by default) on a HIP
    device -> float32 `[B, D]` image features (not normalised): the encoder, then the pooling head of the module
    docstring.  No workspace, no host synchronisation."""
    cfg = net.cfg
    grid = (cfg.grid, cfg.grid) if grid is None else grid
    vit._check_grid(net.encoder, x, grid, max_patches)
    b, d, t = x.shape[0], cfg.dim, grid[0] * grid[1]
    dev = x.device
    xa = vit._encode(net.encoder, x, grid)
    lib = _lib.load()
    stream = _lib.stream_handle(dev)

    def packed(rows: int, cols: int) -> Tensor:
        return torch.empty(vit.packed_elems(rows, cols), dtype=torch.float16, device=dev)

    tokens = vit._layernorm_packed(xa, b * t, net.encoder.norm, cfg.ln_eps, packed(b * t, d), stream)
    kv = vit._gemm(tokens, b * t, net.kv, packed(b * t, 2 * d), stream=stream)
    del tokens
    att = packed(b, d)
    _lib.check(lib.isc_attention_f16_probe(kv.data_ptr(), net.probe_q.data_ptr(), b, t, cfg.heads, d // cfg.heads,
                                           att.data_ptr(), 1, stream), "isc_attention_f16_probe")
    y = vit._gemm(att, b, net.out_proj, torch.empty((b, d), dtype=torch.float32, device=dev), stream=stream)
    h = vit._layernorm_packed(y, b, net.norm, cfg.ln_eps, packed(b, d), stream)
    h = vit._gemm(h, b, net.fc1, packed(b, cfg.mlp_dim), act=vit.ACTIVATIONS[cfg.act], stream=stream)
    return vit._gemm(h, b, net.fc2, torch.empty((b, d), dtype=torch.float32, device=dev), residual=y, stream=stream)


# ---------------------------------------------------------------------------------------------------- the text tower
@dataclass
class PreparedText:
    cfg: SigLIPTextConfig
    table: Tensor  # float32 [vocab, D]
    pos: Tensor  # float32 [context, D]
    blocks: list[Block] = field(default_factory=list)
    norm: Norm | None = None
    head: Linear | None = None  # [D, D] with bias

    def to(self, device: torch.device) -> "PreparedText":
        return PreparedText(self.cfg, self.table.to(device), self.pos.to(device), [b.to(device) for b in self.blocks],
                            self.norm.to(device), self.head.to(device))


def prepare_text(sd: dict[str, Tensor], cfg: SigLIPTextConfig) -> PreparedText:
    """The text tower of `sd` (its `text.*` keys, prefix removed): GEMM weights fp16 and packed as `vit.prepare` stores
    them; the embedding table, positions, biases and LayerNorms float32."""
    _check_shape(cfg.dim, cfg.heads, cfg.mlp_dim)
    if cfg.context < 1:
        raise ValueError(f"context must be positive, got {cfg.context}")
    if not 0 <= cfg.pad_token_id < cfg.vocab:
        raise ValueError(f"pad_token_id {cfg.pad_token_id} is outside the vocabulary [0, {cfg.vocab})")
    if cfg.act not in vit.ACTIVATIONS:
        raise ValueError(f"act must be one of {sorted(vit.ACTIVATIONS)}, got {cfg.act!r}")
    table = _need(sd, "text", "token_embedding.weight", (cfg.vocab, cfg.dim))
    pos = _need(sd, "text", "pos_embed", (cfg.context, cfg.dim))
    _need(sd, "text", "head.weight", (cfg.dim, cfg.dim))
    _need(sd, "text", "head.bias", (cfg.dim,))
    return PreparedText(cfg, table.float().contiguous(), pos.float().contiguous(),
                        [vit.prepare_block(sd, f"blocks.{i}") for i in range(cfg.depth)], vit.prepare_norm(sd, "norm"),
                        vit.prepare_linear(sd, "head"))


def check_ids(ids: Tensor, cfg: SigLIPTextConfig) -> None:
    """TypeError / ValueError unless `ids` is an int64 or int32 `[Q, T]` tensor with `1 <= T <= cfg.context`."""
    if not isinstance(ids, Tensor) or ids.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"ids must be an int64 or int32 tensor, got {getattr(ids, 'dtype', type(ids).__name__)}")
    if ids.ndim != 2:
        raise ValueError(f"ids must have shape [Q, T], got {tuple(ids.shape)}")
    if not 1 <= ids.shape[1] <= cfg.context:
        raise ValueError(f"sequences hold 1 .. {cfg.context} tokens, got T = {ids.shape[1]}")


def pad_ids(ids: Tensor, cfg: SigLIPTextConfig) -> Tensor:
    """`ids` `[Q, T]` right-padded with `cfg.pad_token_id` to `[Q, cfg.context]`: the rows the checkpoints were trained on."""
    q, t = ids.shape
    if t == cfg.context:
        return ids
    out = torch.full((q, cfg.context), cfg.pad_token_id, dtype=ids.dtype, device=ids.device)
    out[:, :t] = ids
    return out


def forward_text(net: PreparedText, ids: Tensor, *, validate: bool = True) -> Tensor:
    """int64 / int32 `[Q, T]` token ids on the net's HIP device, `T <= cfg.context` -> float32 `[Q, D]` text features (not
    normalised), pooled at position `T - 1`.  Sequences run in passes of `vit.PASS_ROWS // T`.  `validate` as in
    `clip.forward_text`: ids outside `[0, vocab)` are embedded as zeros, counted on the device and reported by ONE host
    read after the last pass (ValueError); without it there is no host read and the call can be captured."""
    cfg = net.cfg
    check_ids(ids, cfg)
    _lib.require_device(ids, "ids")
    if ids.device != net.table.device:
        raise ValueError(f"the text tower is on {net.table.device} but ids are on {ids.device}")
    ids = ids.to(torch.int64).contiguous()
    q, t = ids.shape
    d, dev = cfg.dim, ids.device
    out = torch.empty((q, d), dtype=torch.float32, device=dev)
    if q == 0:
        return out
    lib = _lib.load()
    step = max(1, vit.PASS_ROWS // t)
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
                                act=cfg.act)
            pooled = torch.empty(vit.packed_elems(n, d), dtype=torch.float16, device=dev)
            # the last position of every sequence: rows T - 1, 2 T - 1, ... of the stream (row stride T * D)
            st = lib.isc_layernorm(xa.data_ptr() + 4 * (t - 1) * d, n, d, t * d, net.norm.weight.data_ptr(),
                                   net.norm.bias.data_ptr(), cfg.ln_eps, pooled.data_ptr(), _lib.ISC_F16, d, 1, stream)
            _lib.check(st, "isc_layernorm")
            vit._gemm(pooled, n, net.head, out[q0 : q0 + n], stream=stream)
        if validate:
            count = int(bad.item())
            if count:
                raise ValueError(f"{count} token id(s) outside [0, {cfg.vocab})")
    return out


# ------------------------------------------------------------------------------------------------------- the score
def probability(scores, logit_scale: float, logit_bias: float):
    """`sigmoid(exp(logit_scale) * scores + logit_bias)`: the probability SigLIP was trained to give a (text, image) pair
    whose unit-norm embeddings have the cosine `scores` (a tensor on any device, or anything `torch.as_tensor` takes)."""
    s = scores if isinstance(scores, Tensor) else torch.as_tensor(scores, dtype=torch.float32)
    return torch.sigmoid(math.exp(logit_scale) * s + logit_bias)


def score_for_probability(p: float, logit_scale: float, logit_bias: float) -> float:
    """The cosine at which `probability` is `p` (0 < p < 1), in float64 on the host."""
    if not 0.0 < p < 1.0:
        raise ValueError(f"p must be inside (0, 1), got {p}")
    return (math.log(p / (1.0 - p)) - logit_bias) / math.exp(logit_scale)


def shallow(cfg: SigLIPConfig, depth: int) -> SigLIPConfig:
    """`cfg` with `depth` layers in both towers."""
    return SigLIPConfig(replace(cfg.vision, depth=depth), replace(cfg.text, depth=depth))


__all__ = ["IMAGE_MEAN", "IMAGE_STD", "PRESETS", "PreparedText", "PreparedVision", "SigLIPConfig", "SigLIPTextConfig",
           "check_ids", "forward_image", "forward_text", "from_transformers_state_dict", "make_state_dict", "pad_ids",
           "prepare_text", "prepare_vision", "probability", "score_for_probability", "shallow", "tower"]
