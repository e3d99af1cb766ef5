"""ViT-B/16 encoder definition (BASELINE.json configs[4]: "ViT-B/16 (random weights) -> 768-d, fp16"): parameter
naming, seeded init, device-side weight preparation and the forward pass over the HIP transformer blocks.

The reference has no ViT (its encoder is torchvision EfficientNetV2, src/imagescry/models/embedding.py:133-147); this
is the build's own definition behind the same `EmbeddingModule` contract.  State dicts use timm's
`vit_base_patch16_224` parameter names (`cls_token`, `pos_embed`, `patch_embed.proj.weight`, `blocks.3.attn.qkv.weight`,
`blocks.3.mlp.fc1.bias`, `norm.weight`, ...) so such a checkpoint drops in.  The embedding of an image is the class
token after the final LayerNorm (pre-LN encoder, erf-form GELU, LayerNorm eps 1e-6 by default) -- `forward_cls` -- or
the map of its patch tokens -- `forward_tokens` --, on the checkpoint's square token grid or on any `h x w` grid of at
most as many patches (`token_grid`, `position_table`: bicubically resampled position embeddings).

The DINOv2 backbones (`DINOV2_S14` ... `DINOV2_L14_REG`; checkpoint names of facebookresearch/dinov2 and of timm, a
Hugging Face one through `from_transformers_state_dict`) are the same encoder with a patch size of 14, LayerScale behind
the attention and the MLP branch, and -- the `_REG` presets -- four register tokens between the class token and the
patches, whose position table is resampled with antialiasing.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field, replace

import torch
from torch import Tensor

from imagescry_amd import _lib


@dataclass(frozen=True)
class ViTConfig:
    image_size: int = 224
    patch_size: int = 16
    dim: int = 768
    depth: int = 12
    heads: int = 12
    mlp_dim: int = 3072
    ln_eps: float = 1e-6
    registers: int = 0  # register tokens between the class token and the patches (no position embedding)
    layerscale: bool = False  # per-channel scale (`ls1.gamma`, `ls2.gamma`) on the attention and the MLP branch
    pos_antialias: bool = False  # resample the position table with antialiasing (the register checkpoints)
    pre_norm: bool = False  # a LayerNorm (`norm_pre.*`) between the token assembly and the first block (CLIP)
    # the MLP activation: "gelu" (erf form), "quick_gelu" (x * sigmoid(1.702 x), OpenAI CLIP) or "gelu_tanh" (SigLIP)
    act: str = "gelu"
    embed_dim: int = 0  # > 0: a bias-free projection `head.weight` [embed_dim, dim] behind the class token's norm (CLIP)
    class_token: bool = True  # False: the sequence is the patches alone and `pos_embed` has `grid ** 2` rows (SigLIP)

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_prefix(self) -> int:
        """Token rows in front of the patches: the class token and the registers."""
        return int(self.class_token) + self.registers

    @property
    def tokens(self) -> int:
        """Sequence length on the native grid.  (`pos_embed` has `1 + grid ** 2` rows whatever `registers` is; without
        a class token, `grid ** 2`.)"""
        return self.grid * self.grid + self.num_prefix

    @property
    def patch_kdim(self) -> int:
        """Inner dimension of the patch-embedding GEMM: `3 P^2` padded with zeros to whole K steps of 64."""
        return -(-3 * self.patch_size**2 // 64) * 64


VIT_B16 = ViTConfig()
# DINOv2 (ViT-g/14 is not among them: SwiGLU MLP, head size 96)
DINOV2_S14 = ViTConfig(image_size=518, patch_size=14, dim=384, depth=12, heads=6, mlp_dim=1536, layerscale=True)
DINOV2_B14 = ViTConfig(image_size=518, patch_size=14, dim=768, depth=12, heads=12, mlp_dim=3072, layerscale=True)
DINOV2_L14 = ViTConfig(image_size=518, patch_size=14, dim=1024, depth=24, heads=16, mlp_dim=4096, layerscale=True)
DINOV2_S14_REG = replace(DINOV2_S14, registers=4, pos_antialias=True)
DINOV2_B14_REG = replace(DINOV2_B14, registers=4, pos_antialias=True)
DINOV2_L14_REG = replace(DINOV2_L14, registers=4, pos_antialias=True)
# the ImageNet statistics of the DINOv2 evaluation transform (fractions of 255), as `clip.IMAGE_MEAN` / `clip.IMAGE_STD`
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_PATCHES = 4096  # the largest token grid an embedder may ask for: 64 x 64 patches, 1024 x 1024 pixels
ONE_SHOT_TOKENS = 224  # isc_attention_f16 holds a head's keys whole up to here; longer sequences stream them
PASS_ROWS = 1024 * 197  # token rows of the default configuration's largest pass (1024 images x 197 tokens)


def images_per_pass(tokens: int, max_images: int) -> int:
    """Images one pass of the encoder takes at `tokens` tokens an image: `max_images` on the native grids (up to 224
    tokens), above that as many as keep a pass within the 1024 x 197 token rows the default configuration sends, at
    least one."""
    if tokens <= ONE_SHOT_TOKENS:
        return max_images
    return max(1, min(max_images, PASS_ROWS // tokens))


def token_grid(height: int, width: int, max_patches: int = VIT_B16.grid**2) -> tuple[int, int]:
    """The `(h, w)` token grid of an aspect-preserving ViT input: `h = clamp(round(sqrt(max_patches * H / W)), 1,
    max_patches)` (round half to even), `w = max(1, max_patches // h)`.  `h * w <= max_patches` always, a square image
    gets the square grid, and one input shape gets one grid."""
    if height <= 0 or width <= 0 or max_patches <= 0:
        raise ValueError(f"token_grid needs positive sizes, got {height} x {width}, max_patches {max_patches}")
    h = min(max(round(math.sqrt(max_patches * height / width)), 1), max_patches)
    return h, max(1, max_patches // h)


def make_state_dict(cfg: ViTConfig = VIT_B16, *, seed: int = 0, randomize_affine: bool = False) -> dict[str, Tensor]:
    """Seeded random parameters (CPU float32): truncated-normal(std 0.02) weights / tokens, zero biases and identity
    LayerNorms -- or, with `randomize_affine`, random biases and LayerNorm affines so that every term is exercised.
    Register tokens and LayerScale factors (ones; with `randomize_affine` log-uniform in [1e-5, 1], the range trained
    checkpoints cover) are drawn after everything else: a seed gives the other keys the same tensors with or without;
    `norm_pre.*` and the bias-free `head.weight` of a config with `pre_norm` / `embed_dim` follow them."""
    g = torch.Generator().manual_seed(seed)

    def tn(*shape: int) -> Tensor:
        return torch.nn.init.trunc_normal_(torch.empty(*shape), std=0.02, a=-0.04, b=0.04, generator=g)

    def bias(n: int) -> Tensor:
        return torch.randn(n, generator=g) * 0.05 if randomize_affine else torch.zeros(n)

    def gamma(n: int) -> Tensor:
        return torch.rand(n, generator=g) * 0.5 + 0.75 if randomize_affine else torch.ones(n)

    d = cfg.dim
    sd: dict[str, Tensor] = {"cls_token": tn(1, 1, d)} if cfg.class_token else {}
    sd["pos_embed"] = tn(1, int(cfg.class_token) + cfg.grid**2, d)
    sd["patch_embed.proj.weight"] = tn(d, 3, cfg.patch_size, cfg.patch_size)
    sd["patch_embed.proj.bias"] = bias(d)
    for i in range(cfg.depth):
        p = f"blocks.{i}"
        sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"] = gamma(d), bias(d)
        sd[f"{p}.attn.qkv.weight"], sd[f"{p}.attn.qkv.bias"] = tn(3 * d, d), bias(3 * d)
        sd[f"{p}.attn.proj.weight"], sd[f"{p}.attn.proj.bias"] = tn(d, d), bias(d)
        sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"] = gamma(d), bias(d)
        sd[f"{p}.mlp.fc1.weight"], sd[f"{p}.mlp.fc1.bias"] = tn(cfg.mlp_dim, d), bias(cfg.mlp_dim)
        sd[f"{p}.mlp.fc2.weight"], sd[f"{p}.mlp.fc2.bias"] = tn(d, cfg.mlp_dim), bias(d)
    sd["norm.weight"], sd["norm.bias"] = gamma(d), bias(d)
    if cfg.registers:
        sd["register_tokens"] = tn(1, cfg.registers, d)
    if cfg.layerscale:
        for i in range(cfg.depth):
            for name in ("ls1", "ls2"):
                sd[f"blocks.{i}.{name}.gamma"] = (10.0 ** (-5.0 * torch.rand(d, generator=g)) if randomize_affine
                                                  else torch.ones(d))
    if cfg.pre_norm:
        sd["norm_pre.weight"], sd["norm_pre.bias"] = gamma(d), bias(d)
    if cfg.embed_dim:
        sd["head.weight"] = tn(cfg.embed_dim, d)
    return sd


def gemm_flops(cfg: ViTConfig = VIT_B16) -> int:
    """Multiply-add FLOPs (2 per MAC) of the GEMMs and the attention products for ONE image."""
    t, d = cfg.tokens, cfg.dim
    per_layer = 2 * t * d * (3 * d) + 2 * t * d * d + 2 * 2 * t * d * cfg.mlp_dim + 2 * 2 * t * t * d
    return 2 * (t - cfg.num_prefix) * d * (3 * cfg.patch_size**2) + cfg.depth * per_layer


def pack_rows(x: Tensor) -> Tensor:
    """Row-major `[R, C]` (C % 64 == 0) -> the PACKED layout of include/imagescry_hip.h: rows in tiles of 256 (zero
    padded), columns in K steps of 64, stored `[tile][K step][row][64]`; returned flat."""
    r, c = x.shape
    if c % 64:
        raise ValueError(f"packed matrices need a multiple of 64 columns, got {c}")
    tiles = (r + 255) // 256
    padded = torch.zeros((tiles * 256, c), dtype=x.dtype, device=x.device)
    padded[:r] = x
    return padded.view(tiles, 256, c // 64, 64).permute(0, 2, 1, 3).contiguous().view(-1)


def unpack_rows(flat: Tensor, rows: int, cols: int) -> Tensor:
    """Inverse of `pack_rows`."""
    tiles = (rows + 255) // 256
    return flat.view(tiles, cols // 64, 256, 64).permute(0, 2, 1, 3).reshape(tiles * 256, cols)[:rows].contiguous()


def packed_elems(rows: int, cols: int) -> int:
    return (rows + 255) // 256 * 256 * cols


@dataclass
class Linear:
    weight: Tensor  # fp16, PACKED [out, in] (pack_rows of the torch.nn.Linear weight)
    bias: Tensor | None  # float32 [out]; None: no bias (the CLIP projections)
    out_features: int = 0
    in_features: int = 0

    def __post_init__(self) -> None:
        if not self.out_features:
            raise ValueError("Linear needs its logical shape")

    def to(self, device: torch.device) -> "Linear":
        return Linear(self.weight.to(device), None if self.bias is None else self.bias.to(device), self.out_features,
                      self.in_features)


@dataclass
class Norm:
    weight: Tensor
    bias: Tensor

    def to(self, device: torch.device) -> "Norm":
        return Norm(self.weight.to(device), self.bias.to(device))


@dataclass
class Block:
    norm1: Norm
    qkv: Linear
    proj: Linear
    norm2: Norm
    fc1: Linear
    fc2: Linear
    ls1: Tensor | None = None  # float32 [D] LayerScale of the attention branch (scales `proj`'s output), or None
    ls2: Tensor | None = None  # ... of the MLP branch (`fc2`)

    def to(self, device: torch.device) -> "Block":
        return Block(*(getattr(self, f).to(device) for f in ("norm1", "qkv", "proj", "norm2", "fc1", "fc2")),
                     *(None if s is None else s.to(device) for s in (self.ls1, self.ls2)))


@dataclass
class PreparedViT:
    cfg: ViTConfig
    cls_token: Tensor | None  # float32 [D]; None without a class token
    pos_embed: Tensor  # float32 [1 + grid ** 2, D]; without a class token row 0 is a zero row nothing adds to a token
    patch: Linear  # [D, cfg.patch_kdim]: columns past 3 * P * P are zero
    blocks: list[Block] = field(default_factory=list)
    norm: Norm | None = None
    reg_tokens: Tensor | None = None  # float32 [registers, D]
    norm_pre: Norm | None = None  # cfg.pre_norm
    head: Linear | None = None  # cfg.embed_dim: [embed_dim, D], no bias
    # resampled position tables, (h, w) -> float32 [1 + h * w, D] on pos_embed's device; belongs to THIS prepared net
    # (`to` starts an empty one), bounded by POS_CACHE_MAX
    pos_cache: dict[tuple[int, int], Tensor] = field(default_factory=dict, repr=False, compare=False)

    def to(self, device: torch.device) -> "PreparedViT":
        return PreparedViT(self.cfg, None if self.cls_token is None else self.cls_token.to(device),
                           self.pos_embed.to(device), self.patch.to(device),
                           [b.to(device) for b in self.blocks], self.norm.to(device),
                           None if self.reg_tokens is None else self.reg_tokens.to(device),
                           None if self.norm_pre is None else self.norm_pre.to(device),
                           None if self.head is None else self.head.to(device))


ACTIVATIONS = {"gelu": _lib.ISC_ACT_GELU, "quick_gelu": _lib.ISC_ACT_QUICK_GELU, "gelu_tanh": _lib.ISC_ACT_GELU_TANH}


def prepare_linear(sd: dict[str, Tensor], name: str, pad_to: int = 0, bias: bool = True) -> Linear:
    """`name.weight` (any trailing shape, flattened to `[out, in]`) cast to fp16, its inner dimension zero-padded to
    `pad_to`, packed; `name.bias` in float32, or no bias."""
    w = sd[f"{name}.weight"]
    w2 = w.reshape(w.shape[0], -1).to(torch.float16)
    if pad_to > w2.shape[1]:
        w2 = torch.nn.functional.pad(w2, (0, pad_to - w2.shape[1]))
    return Linear(pack_rows(w2), sd[f"{name}.bias"].float().contiguous() if bias else None, w2.shape[0], w2.shape[1])


def prepare_norm(sd: dict[str, Tensor], name: str) -> Norm:
    return Norm(sd[f"{name}.weight"].float().contiguous(), sd[f"{name}.bias"].float().contiguous())


def prepare_block(sd: dict[str, Tensor], p: str, ls1: Tensor | None = None, ls2: Tensor | None = None) -> Block:
    """The pre-LN block `p` = "blocks.i" of a state dict under this module's names."""
    return Block(prepare_norm(sd, f"{p}.norm1"), prepare_linear(sd, f"{p}.attn.qkv"), prepare_linear(sd, f"{p}.attn.proj"),
                 prepare_norm(sd, f"{p}.norm2"), prepare_linear(sd, f"{p}.mlp.fc1"), prepare_linear(sd, f"{p}.mlp.fc2"),
                 ls1, ls2)


def prepare(sd: dict[str, Tensor], cfg: ViTConfig = VIT_B16) -> PreparedViT:
    """Cast GEMM weights to fp16 (round-to-nearest-even) and store them in the packed layout the GEMM kernels stream; keep
    biases / LayerNorm / LayerScale / tokens in float32.  The patch weight's inner dimension is zero-padded to whole K
    steps of 64 (`cfg.patch_kdim`: 588 -> 640 for a patch size of 14).  LayerScale stays a float32 vector for the GEMM
    epilogue: trained values go down to 1e-5, and folded into the weights they would land in fp16 subnormals.
    `register_tokens` may be spelled `reg_token` (timm); `mask_token` is ignored.  `cfg.pre_norm` asks for `norm_pre.*`,
    `cfg.embed_dim` for a `head.weight` of shape `[embed_dim, dim]` (no bias).  Without `cfg.class_token` there is no
    `cls_token` key and `pos_embed` is `(1, grid ** 2, dim)`; it is stored behind one zero row, the shape
    `isc_vit_pos_resample` takes (that row is copied, never added to a token)."""
    d = cfg.dim
    if cfg.dim % 64 or cfg.mlp_dim % 64 or cfg.dim // cfg.heads != 64:
        raise ValueError("this build supports head size 64 and GEMM inner dimensions that are multiples of 64")
    if cfg.patch_size % 2:
        raise ValueError(f"this build supports even patch sizes, got {cfg.patch_size}")
    if cfg.act not in ACTIVATIONS:
        raise ValueError(f"act must be one of {sorted(ACTIVATIONS)}, got {cfg.act!r}")
    if cfg.embed_dim < 0 or cfg.embed_dim % 4:
        raise ValueError(f"embed_dim must be a non-negative multiple of 4, got {cfg.embed_dim}")
    if not cfg.class_token and (cfg.registers or cfg.embed_dim):
        raise ValueError("register tokens and a projection of the class token need a class token")
    rows = 1 + cfg.grid**2
    own = rows if cfg.class_token else rows - 1  # rows of the checkpoint's table
    if tuple(sd["pos_embed"].shape) != (1, own, d):
        raise ValueError(f"pos_embed has shape {tuple(sd['pos_embed'].shape)}, expected (1, {own}, {d})")

    def need(key: str, what: str) -> Tensor:
        if key not in sd:
            raise ValueError(f"the config asks for {what}, but the state dict has no `{key}`")
        return sd[key]

    def scale(key: str) -> Tensor | None:
        return need(key, "LayerScale").reshape(d).float().contiguous() if cfg.layerscale else None

    pos = sd["pos_embed"].reshape(own, d).float()
    if not cfg.class_token:
        pos = torch.cat([torch.zeros((1, d), dtype=torch.float32, device=pos.device), pos])
    net = PreparedViT(cfg, sd["cls_token"].reshape(d).float().contiguous() if cfg.class_token else None,
                      pos.contiguous(), prepare_linear(sd, "patch_embed.proj", cfg.patch_kdim))
    if cfg.registers:
        key = "register_tokens" if "register_tokens" in sd or "reg_token" not in sd else "reg_token"
        reg = need(key, f"{cfg.registers} register tokens")
        if tuple(reg.shape) != (1, cfg.registers, d):
            raise ValueError(f"{key} has shape {tuple(reg.shape)}, expected (1, {cfg.registers}, {d})")
        net.reg_tokens = reg.reshape(cfg.registers, d).float().contiguous()
    for i in range(cfg.depth):
        p = f"blocks.{i}"
        net.blocks.append(prepare_block(sd, p, scale(f"{p}.ls1.gamma"), scale(f"{p}.ls2.gamma")))
    net.norm = prepare_norm(sd, "norm")
    if cfg.pre_norm:
        need("norm_pre.weight", "a LayerNorm in front of the blocks")
        net.norm_pre = prepare_norm(sd, "norm_pre")
    if cfg.embed_dim:
        head = need("head.weight", f"a projection to {cfg.embed_dim} dimensions")
        if tuple(head.shape) != (cfg.embed_dim, d):
            raise ValueError(f"head.weight has shape {tuple(head.shape)}, expected ({cfg.embed_dim}, {d})")
        net.head = prepare_linear(sd, "head", bias=False)
    return net


def from_transformers_state_dict(hf: dict[str, Tensor]) -> dict[str, Tensor]:
    """The state dict of a Hugging Face `Dinov2Model` / `Dinov2WithRegistersModel` (with or without a leading
    `dinov2.` / `dinov2_with_registers.`) under this module's names: separate query / key / value are fused into
    `attn.qkv` in `[q; k; v]` row order, `layer_scale1.lambda1` becomes `ls1.gamma`, `layernorm` becomes `norm`.  Keys
    that belong to no encoder parameter (`mask_token`, a classifier head) are dropped."""
    wrappers = ("dinov2", "dinov2_with_registers")
    hf = {k.split(".", 1)[1] if k.split(".", 1)[0] in wrappers else k: v for k, v in hf.items()}
    sd: dict[str, Tensor] = {}
    for ours, theirs in (("cls_token", "embeddings.cls_token"), ("pos_embed", "embeddings.position_embeddings"),
                         ("register_tokens", "embeddings.register_tokens"),
                         ("patch_embed.proj.weight", "embeddings.patch_embeddings.projection.weight"),
                         ("patch_embed.proj.bias", "embeddings.patch_embeddings.projection.bias"),
                         ("norm.weight", "layernorm.weight"), ("norm.bias", "layernorm.bias")):
        if theirs in hf:
            sd[ours] = hf[theirs]
    per_layer = (("norm1", "norm1"), ("attn.proj", "attention.output.dense"), ("norm2", "norm2"), ("mlp.fc1", "mlp.fc1"),
                 ("mlp.fc2", "mlp.fc2"))
    i = 0
    while f"encoder.layer.{i}.norm1.weight" in hf:
        p, q = f"blocks.{i}", f"encoder.layer.{i}"
        for ours, theirs in per_layer:
            for kind in ("weight", "bias"):
                sd[f"{p}.{ours}.{kind}"] = hf[f"{q}.{theirs}.{kind}"]
        for kind in ("weight", "bias"):
            sd[f"{p}.attn.qkv.{kind}"] = torch.cat([hf[f"{q}.attention.attention.{n}.{kind}"]
                                                    for n in ("query", "key", "value")])
        for n in ("1", "2"):
            if f"{q}.layer_scale{n}.lambda1" in hf:
                sd[f"{p}.ls{n}.gamma"] = hf[f"{q}.layer_scale{n}.lambda1"]
        i += 1
    if i == 0:
        raise ValueError("no `encoder.layer.0.*` keys: not a transformers Dinov2 state dict")
    return sd


def _gemm(a: Tensor, m: int, lin: Linear, out: Tensor, *, act: int = _lib.ISC_ACT_NONE, residual: Tensor | None = None,
          scale: Tensor | None = None, stream: int = 0) -> Tensor:
    """`out = act(a . W^T + b) + residual`; `a` is a packed fp16 activation buffer of `m` rows, `out` either a packed
    fp16 buffer (next GEMM operand) or a row-major float32 `[m, N]` tensor (residual stream).  With `scale` (float32
    `[N]`, LayerScale; float32 output only): `out = scale * (a . W^T + b) + residual`, one launch
    (`isc_gemm_f16_scaled`)."""
    f16 = out.dtype == torch.float16
    flags = _lib.ISC_GEMM_A_PACKED | _lib.ISC_GEMM_W_PACKED | (_lib.ISC_GEMM_OUT_PACKED if f16 else 0)
    if scale is not None:
        st = _lib.load().isc_gemm_f16_scaled(a.data_ptr(), m, lin.in_features, lin.weight.data_ptr(), lin.out_features,
                                             _lib.ptr(lin.bias), scale.data_ptr(), _lib.ptr(residual), act,
                                             out.data_ptr(), _lib.ISC_F16 if f16 else _lib.ISC_F32, flags, stream)
        _lib.check(st, "isc_gemm_f16_scaled")
        return out
    # the tanh GELU goes through the entry that admits it; every other call is isc_gemm_f16, as before
    name = "isc_gemm_f16_act" if act == _lib.ISC_ACT_GELU_TANH else "isc_gemm_f16"
    st = getattr(_lib.load(), name)(a.data_ptr(), m, lin.in_features, lin.weight.data_ptr(), lin.out_features,
                                    _lib.ptr(lin.bias), _lib.ptr(residual), act, out.data_ptr(),
                                    _lib.ISC_F16 if f16 else _lib.ISC_F32, flags, stream)
    _lib.check(st, name)
    return out


def _layernorm_packed(x: Tensor, rows: int, nrm: Norm, eps: float, out: Tensor, stream: int) -> Tensor:
    d = nrm.weight.shape[0]
    st = _lib.load().isc_layernorm(x.data_ptr(), rows, d, d, nrm.weight.data_ptr(), nrm.bias.data_ptr(), eps,
                                   out.data_ptr(), _lib.ISC_F16, d, 1, stream)
    _lib.check(st, "isc_layernorm")
    return out


POS_CACHE_MAX = 16  # resampled position tables kept per prepared net (0.6 MB each for ViT-B/16)


def position_table(net: PreparedViT, grid: tuple[int, int]) -> Tensor:
    """float32 `[1 + h * w, D]` position table of an `h x w` token grid: the class row as it is, the `g x g` patch rows
    resampled bicubically (`isc_vit_pos_resample`, the arithmetic of `F.interpolate(mode="bicubic")`; with
    `cfg.pos_antialias` `isc_vit_pos_resample_aa`, that of `antialias=True`).  The native grid returns `net.pos_embed`
    itself, no launch; other grids are computed once per device and cached on `net`."""
    h, w = grid
    g = net.cfg.grid
    if (h, w) == (g, g):
        return net.pos_embed
    table = net.pos_cache.get((h, w))
    if table is None or table.device != net.pos_embed.device:
        _lib.require_device(net.pos_embed, "pos_embed")
        dev = net.pos_embed.device
        table = torch.empty((1 + h * w, net.cfg.dim), dtype=torch.float32, device=dev)
        name = "isc_vit_pos_resample_aa" if net.cfg.pos_antialias else "isc_vit_pos_resample"
        with torch.cuda.device(dev):
            st = getattr(_lib.load(), name)(net.pos_embed.data_ptr(), g, h, w, net.cfg.dim, table.data_ptr(),
                                            _lib.stream_handle(dev))
        _lib.check(st, name)
        net.pos_cache.pop((h, w), None)
        if len(net.pos_cache) >= POS_CACHE_MAX:  # bound what a net pins: drop the oldest grid
            net.pos_cache.pop(next(iter(net.pos_cache)))
        net.pos_cache[(h, w)] = table
    return table


def _encode(net: PreparedViT, x: Tensor, grid: tuple[int, int], blocks: list[Block] | None = None) -> Tensor:
    """float32 `[B, 3, P h, P w]` (already preprocessed) on a HIP device -> the float32 residual stream `[B * T, D]`
    after the last block, `T = h w + cfg.num_prefix` (the final LayerNorm is the caller's).  `blocks`: the blocks to
    run, all of `net.blocks` by default (`forward_dense` leaves the last one out).

    Every fp16 activation (patches, LayerNorm outputs, qkv, attention output, MLP hidden) lives in the packed layout;
    the float32 residual stream is row-major."""
    cfg = net.cfg
    b = x.shape[0]
    gh, gw = grid
    npatch, d = gh * gw, cfg.dim
    t = npatch + cfg.num_prefix
    m = b * t
    dev = x.device
    lib = _lib.load()
    stream = _lib.stream_handle(dev)
    f16, f32 = torch.float16, torch.float32
    kdim = cfg.patch_kdim

    def packed(rows: int, cols: int) -> Tensor:
        # rows past `rows` in the last tile are never read into a result that is kept; they only have to be finite
        # enough not to matter, and every consumer masks them, so the buffer is left uninitialised
        return torch.empty(packed_elems(rows, cols), dtype=f16, device=dev)

    pos = position_table(net, grid)
    patches = packed(b * npatch, kdim)
    if cfg.patch_size % 8 == 0 and kdim == 3 * cfg.patch_size**2:
        _lib.check(lib.isc_patchify_f16(x.data_ptr(), b, 3, gh * cfg.patch_size, gw * cfg.patch_size, cfg.patch_size,
                                        patches.data_ptr(), 1, stream), "isc_patchify_f16")
    else:  # any even patch size; the padding columns of the K steps are written as zeros
        _lib.check(lib.isc_patchify_f16_padded(x.data_ptr(), b, 3, gh * cfg.patch_size, gw * cfg.patch_size,
                                               cfg.patch_size, kdim, patches.data_ptr(), 1, stream),
                   "isc_patchify_f16_padded")
    pe = torch.empty((b * npatch, d), dtype=f32, device=dev)
    _gemm(patches, b * npatch, net.patch, pe, stream=stream)
    del patches
    xa = torch.empty((m, d), dtype=f32, device=dev)  # residual stream (ping)
    xb = torch.empty((m, d), dtype=f32, device=dev)  # residual stream (pong)
    if not cfg.class_token:  # the table's rows behind the leading one (D floats: the alignment holds)
        _lib.check(lib.isc_vit_assemble_plain(pe.data_ptr(), pos.data_ptr() + 4 * d, b, npatch, d, xa.data_ptr(), stream),
                   "isc_vit_assemble_plain")
    elif cfg.registers:
        _lib.check(lib.isc_vit_assemble_reg(pe.data_ptr(), net.cls_token.data_ptr(), net.reg_tokens.data_ptr(),
                                            pos.data_ptr(), b, t, cfg.registers, d, xa.data_ptr(), stream),
                   "isc_vit_assemble_reg")
    else:
        _lib.check(lib.isc_vit_assemble(pe.data_ptr(), net.cls_token.data_ptr(), pos.data_ptr(), b, t, d,
                                        xa.data_ptr(), stream), "isc_vit_assemble")
    del pe
    if cfg.pre_norm:  # float32 -> float32 into the other residual buffer
        _lib.check(lib.isc_layernorm(xa.data_ptr(), m, d, d, net.norm_pre.weight.data_ptr(), net.norm_pre.bias.data_ptr(),
                                     cfg.ln_eps, xb.data_ptr(), _lib.ISC_F32, d, 0, stream), "isc_layernorm")
        xa, xb = xb, xa
    return run_blocks(net.blocks if blocks is None else blocks, xa, xb, b, t, heads=cfg.heads, mlp_dim=cfg.mlp_dim,
                      ln_eps=cfg.ln_eps, act=cfg.act)


def run_blocks(blocks: list[Block], xa: Tensor, xb: Tensor, b: int, t: int, *, heads: int, mlp_dim: int, ln_eps: float,
               act: str = "gelu", causal: bool = False) -> Tensor:
    """The pre-LN transformer blocks over the float32 residual stream `xa` `[b * t, D]` (`xb`: a second buffer of that
    shape); returns `xa`, which holds the stream after the last block.  `causal`: `isc_attention_f16_causal` (a text
    tower, `t <= 128`) in place of the bidirectional kernels."""
    m, d = xa.shape
    dev = xa.device
    lib = _lib.load()
    stream = _lib.stream_handle(dev)

    def packed(rows: int, cols: int) -> Tensor:  # as in `_encode`: left uninitialised
        return torch.empty(packed_elems(rows, cols), dtype=torch.float16, device=dev)

    hbuf, qkv, att, mlp = packed(m, d), packed(m, 3 * d), packed(m, d), packed(m, mlp_dim)
    for blk in blocks:
        _layernorm_packed(xa, m, blk.norm1, ln_eps, hbuf, stream)
        _gemm(hbuf, m, blk.qkv, qkv, stream=stream)
        if causal:
            _lib.check(lib.isc_attention_f16_causal(qkv.data_ptr(), b, t, heads, d // heads, att.data_ptr(), 1, stream),
                       "isc_attention_f16_causal")
        elif t <= ONE_SHOT_TOKENS:
            _lib.check(lib.isc_attention_f16(qkv.data_ptr(), b, t, heads, d // heads, att.data_ptr(), 1, stream),
                       "isc_attention_f16")
        else:  # the keys of a head no longer fit in LDS: the streaming kernel
            _lib.check(lib.isc_attention_f16_stream(qkv.data_ptr(), b, t, heads, d // heads, att.data_ptr(), 1, stream),
                       "isc_attention_f16_stream")
        _gemm(att, m, blk.proj, xb, residual=xa, scale=blk.ls1, stream=stream)
        _layernorm_packed(xb, m, blk.norm2, ln_eps, hbuf, stream)
        _gemm(hbuf, m, blk.fc1, mlp, act=ACTIVATIONS[act], stream=stream)
        _gemm(mlp, m, blk.fc2, xa, residual=xb, scale=blk.ls2, stream=stream)
    return xa


def _check_grid(net: PreparedViT, x: Tensor, grid: tuple[int, int], max_patches: int | None = None) -> None:
    h, w = grid
    p = net.cfg.patch_size
    top = net.cfg.grid**2 if max_patches is None else max_patches
    if h < 1 or w < 1 or h * w > top:
        raise ValueError(f"a token grid holds 1 .. {top} patches, got {h} x {w}")
    if x.ndim != 4 or tuple(x.shape[1:]) != (3, h * p, w * p):
        raise ValueError(f"x must have shape [B, 3, {h * p}, {w * p}] for a {h} x {w} grid, got {tuple(x.shape)}")


def _need_class_token(cfg: ViTConfig, what: str) -> None:
    if not cfg.class_token:
        raise ValueError(f"{what} needs a tower with a class token; one without is pooled by its own head "
                         "(siglip.forward_image)")


def forward_cls(net: PreparedViT, x: Tensor, grid: tuple[int, int] | None = None,
                max_patches: int | None = None) -> Tensor:
    """float32 `[B, 3, P h, P w]` (already preprocessed; `grid = (h, w)`, the native square grid by default) on a HIP
    device -> float32 `[B, D]` class-token features.  `max_patches`: the most patches `grid` may hold, the native
    grid's count by default."""
    cfg = net.cfg
    _need_class_token(cfg, "forward_cls")
    grid = (cfg.grid, cfg.grid) if grid is None else grid
    _check_grid(net, x, grid, max_patches)
    b, d, t = x.shape[0], cfg.dim, grid[0] * grid[1] + cfg.num_prefix
    xa = _encode(net, x, grid)
    if net.head is not None:  # LayerNorm of the class rows into a packed fp16 operand, then the projection: [B, E]
        stream = _lib.stream_handle(x.device)
        cls = torch.empty(packed_elems(b, d), dtype=torch.float16, device=x.device)
        st = _lib.load().isc_layernorm(xa.data_ptr(), b, d, t * d, net.norm.weight.data_ptr(), net.norm.bias.data_ptr(),
                                       cfg.ln_eps, cls.data_ptr(), _lib.ISC_F16, d, 1, stream)
        _lib.check(st, "isc_layernorm")
        return _gemm(cls, b, net.head, torch.empty((b, net.head.out_features), dtype=torch.float32, device=x.device),
                     stream=stream)
    out = torch.empty((b, d), dtype=torch.float32, device=x.device)
    st = _lib.load().isc_layernorm(xa.data_ptr(), b, d, t * d, net.norm.weight.data_ptr(), net.norm.bias.data_ptr(),
                                   cfg.ln_eps, out.data_ptr(), _lib.ISC_F32, d, 0,
                                   _lib.stream_handle(x.device))  # class-token rows only (row stride T * D)
    _lib.check(st, "isc_layernorm")
    return out


def forward_tokens(net: PreparedViT, x: Tensor, grid: tuple[int, int] | None = None, normalize: bool = False,
                   out: Tensor | None = None, max_patches: int | None = None) -> Tensor:
    """float32 `[B, 3, P h, P w]` -> the float32 patch-token map `[B, D, h, w]`: cell `(i, j)` is token
    `cfg.num_prefix + i w + j` (the class token and any registers are left out) after the final LayerNorm, L2-normalised
    per cell (`F.normalize`, eps 1e-12) when `normalize` -- LayerNorm,
    normalisation and the transposition into the channels-first map are one kernel (`isc_vit_tokens_out`).  `out`: a
    contiguous `[B, D, h, w]` tensor to write into.  `max_patches`: the most patches `grid` may hold, the native grid's
    count by default."""
    cfg = net.cfg
    _need_class_token(cfg, "forward_tokens")
    grid = (cfg.grid, cfg.grid) if grid is None else grid
    _check_grid(net, x, grid, max_patches)
    h, w = grid
    b, d, t = x.shape[0], cfg.dim, h * w + cfg.num_prefix
    if out is None:
        out = torch.empty((b, d, h, w), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (b, d, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous float32 [{b}, {d}, {h}, {w}] tensor on {x.device}")
    xa = _encode(net, x, grid)
    args = (d, net.norm.weight.data_ptr(), net.norm.bias.data_ptr(), cfg.ln_eps, int(normalize), 1e-12, out.data_ptr(),
            _lib.stream_handle(x.device))
    if cfg.registers:
        _lib.check(_lib.load().isc_vit_tokens_out_skip(xa.data_ptr(), b, t, cfg.num_prefix, *args),
                   "isc_vit_tokens_out_skip")
    else:
        _lib.check(_lib.load().isc_vit_tokens_out(xa.data_ptr(), b, t, *args), "isc_vit_tokens_out")
    return out


DENSE_MODES = ("value", "kk", "qq")


def prepare_value_linear(sd: dict[str, Tensor], p: str) -> Linear:
    """The value projection of block `p` = "blocks.i" on its own: rows `2 D : 3 D` of the fused `attn.qkv` weight and
    bias, stored as `prepare_linear` stores a weight (`forward_dense(mode="value")` multiplies nothing else of it)."""
    w, b = sd[f"{p}.attn.qkv.weight"], sd[f"{p}.attn.qkv.bias"]
    d = w.shape[0] // 3
    return prepare_linear({"v.weight": w[2 * d :], "v.bias": b[2 * d :]}, "v")


def forward_dense(net: PreparedViT, x: Tensor, mode: str, grid: tuple[int, int] | None = None, normalize: bool = False,
                  out: Tensor | None = None, max_patches: int | None = None, value: Linear | None = None) -> Tensor:
    """float32 `[B, 3, P h, P w]` -> the float32 DENSE patch map `[B, E, h, w]` of a tower with a projection head
    (`cfg.embed_dim`, CLIP): per-token features in the space the class token is projected into, by the training-free
    change of the LAST block that MaskCLIP (`mode="value"`) and SCLIP / ClearCLIP ("kk", "qq") describe.  Blocks
    `0 .. depth - 2` run as they are; with `x` the residual stream behind them and `h = LN1(x)` of the last block,

        a = v_proj(h)                        "value": no attention, every token keeps its own value vector (`value`, the
                                             Linear of `prepare_value_linear`: a third of the qkv product)
        a = softmax(K K^T / 8) V per head    "kk", over all T tokens, the class token included (`isc_attention_f16_self`,
                                             above 224 tokens `isc_attention_f16_self_stream`); "qq": Q in place of K
        y = out_proj(a) + bias               NO residual and NO MLP
        e = LN_post(y) . head.weight^T       no bias; `isc_layernorm` into a packed fp16 operand, then the GEMM

    and the rows of the patch tokens go, transposed and (`normalize`) divided by `max(||cell||_2, 1e-12)`, into `out`
    (`isc_tokens_to_map`): cell `(i, j)` is token `1 + i w + j`.  No workspace, no host synchronisation."""
    cfg = net.cfg
    if mode not in DENSE_MODES:
        raise ValueError(f"mode must be one of {DENSE_MODES}, got {mode!r}")
    if net.head is None or cfg.registers or cfg.layerscale or not net.blocks or not cfg.class_token:
        raise ValueError("a dense map needs a tower with a projection head (embed_dim), at least one block, no register "
                         "tokens and no LayerScale")
    if mode == "value" and (value is None or (value.out_features, value.in_features) != (cfg.dim, cfg.dim)):
        raise ValueError('mode="value" needs the value Linear of the last block (prepare_value_linear)')
    grid = (cfg.grid, cfg.grid) if grid is None else grid
    _check_grid(net, x, grid, max_patches)
    h, w = grid
    b, d, e, t = x.shape[0], cfg.dim, net.head.out_features, h * w + 1
    m = b * t
    dev = x.device
    if out is None:
        out = torch.empty((b, e, h, w), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (b, e, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float32 [{b}, {e}, {h}, {w}] tensor on {dev}")
    xa = _encode(net, x, grid, net.blocks[:-1])
    lib = _lib.load()
    stream = _lib.stream_handle(dev)
    blk = net.blocks[-1]
    hbuf = torch.empty(packed_elems(m, d), dtype=torch.float16, device=dev)
    att = torch.empty_like(hbuf)
    _layernorm_packed(xa, m, blk.norm1, cfg.ln_eps, hbuf, stream)
    if mode == "value":
        _gemm(hbuf, m, value, att, stream=stream)
    else:
        qkv = torch.empty(packed_elems(m, 3 * d), dtype=torch.float16, device=dev)
        _gemm(hbuf, m, blk.qkv, qkv, stream=stream)
        part = _lib.ISC_ATT_PART_KEY if mode == "kk" else _lib.ISC_ATT_PART_QUERY
        name = "isc_attention_f16_self" if t <= ONE_SHOT_TOKENS else "isc_attention_f16_self_stream"
        _lib.check(getattr(lib, name)(qkv.data_ptr(), b, t, cfg.heads, d // cfg.heads, part, att.data_ptr(), 1, stream), name)
        del qkv
    y = _gemm(att, m, blk.proj, torch.empty((m, d), dtype=torch.float32, device=dev), stream=stream)
    _layernorm_packed(y, m, net.norm, cfg.ln_eps, hbuf, stream)
    tokens = _gemm(hbuf, m, net.head, torch.empty((m, e), dtype=torch.float32, device=dev), stream=stream)
    _lib.check(lib.isc_tokens_to_map(tokens.data_ptr(), b, t, 1, e, int(normalize), 1e-12, out.data_ptr(), stream),
               "isc_tokens_to_map")
    return out


__all__ = ["ACTIVATIONS", "DENSE_MODES", "DINOV2_B14", "DINOV2_B14_REG", "DINOV2_L14", "DINOV2_L14_REG", "DINOV2_S14", "DINOV2_S14_REG", "IMAGENET_MEAN", "IMAGENET_STD",
           "MAX_PATCHES",
           "VIT_B16", "ViTConfig", "forward_cls", "forward_tokens", "from_transformers_state_dict", "gemm_flops",
           "images_per_pass", "make_state_dict", "pack_rows", "position_table", "prepare", "prepare_block", "prepare_linear",
           "prepare_norm", "run_blocks", "token_grid", "unpack_rows"]
