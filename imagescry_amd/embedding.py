"""Embedder interface and the ResNet-50 embedder, on MI355X.

`EmbeddingModule` keeps the reference's extension point (src/imagescry/models/embedding.py:27-104): subclasses
implement `preprocess`, `forward` and `embedding_dim`; `predict_step` runs preprocess -> forward -> L2-normalise
over channels -> `EmbeddingBatch`; `embed_images` maps it over a dataloader.  The reference gets `.to()` /
`.device` / the predict loop from Lightning; here they are a few lines of plain Python so that nothing but the
HIP kernels touches the data.
"""

from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Iterable

import torch
from torch import Tensor

from imagescry_amd import _lib, clip, efficientnet, resnet50, segmentation, siglip, vit
from imagescry_amd.data import EmbeddingBatch, ImageBatch
from imagescry_amd.transforms import normalize_per_channel, resize, resize_antialias, resize_center_crop

__all__ = ["CLIPEmbedder", "DINOv2Embedder", "EfficientNetEmbedder", "EmbeddingModule", "ResNet50Embedder", "SigLIPEmbedder", "ViTB16Embedder",
           "l2_normalize_channels"]


def l2_normalize_channels(x: Tensor, eps: float = 1e-12) -> Tensor:
    """`F.normalize(x, p=2, dim=1)` for a float32 `[B, E, H, W]` map (reference: embedding.py:74)."""
    if x.ndim != 4 or x.dtype != torch.float32:
        raise ValueError(f"expected a float32 [B, E, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    _lib.require_device(x, "x")
    b, e, h, w = x.shape
    lib = _lib.load()
    nhwc = x.permute(0, 2, 3, 1)
    if not x.is_contiguous() and nhwc.is_contiguous():
        # a channels-last buffer seen through an NCHW view (what the NHWC encoders hand back): every location is a
        # contiguous row of E channels -- normalise the rows in place of a layout change
        y = torch.empty_like(nhwc)
        if x.numel():
            with torch.cuda.device(x.device):
                st = lib.isc_l2norm_channels(nhwc.data_ptr(), b * h * w, e, 1, eps, y.data_ptr(),
                                             _lib.stream_handle(x.device))
            _lib.check(st, "isc_l2norm_channels")
        return y.permute(0, 3, 1, 2)
    x = x.contiguous()
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    with torch.cuda.device(x.device):
        st = lib.isc_l2norm_channels(x.data_ptr(), b, e, h * w, eps, y.data_ptr(), _lib.stream_handle(x.device))
    _lib.check(st, "isc_l2norm_channels")
    return y


class EmbeddingModule(ABC):
    """Embedding module interface (reference: src/imagescry/models/embedding.py:27-104)."""

    def __init__(self) -> None:
        self._device = torch.device("cpu")
        self.hparams: dict[str, object] = {}

    # -- subclass contract ---------------------------------------------------------------------------
    @abstractmethod
    def preprocess(self, images: Tensor) -> Tensor:
        """uint8 `[B, C, H1, W1]` -> float `[B, C, H2, W2]` in the format the model expects."""

    @abstractmethod
    def forward(self, x: Tensor) -> Tensor:
        """float `[B, C, H1, W1]` -> embedding feature map float `[B, E, H2, W2]`."""

    @property
    @abstractmethod
    def embedding_dim(self) -> int:
        """Embedding dimension E."""

    def _move(self, device: torch.device) -> None:
        """Move parameters to `device` (subclasses with weights override this)."""

    # -- provided ------------------------------------------------------------------------------------
    def to(self, device: str | torch.device) -> "EmbeddingModule":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._move(device)
        self._device = device
        return self

    @property
    def device(self) -> torch.device:
        return self._device

    def __call__(self, x: Tensor) -> Tensor:
        return self.forward(x)

    def predict_step(self, batch: ImageBatch) -> EmbeddingBatch:
        """preprocess -> forward -> L2-normalise each embedding vector (reference: embedding.py:57-76)."""
        if not isinstance(batch, ImageBatch):
            raise TypeError(f"batch must be an ImageBatch, got {type(batch).__name__}")
        if self._fused_predict_ok():
            # preprocess and forward back to back: the normalisation writes the stem's channels-last layout directly
            # (same values as `forward(preprocess(images))`, one pass less over the batch)
            x4 = self.preprocess(batch.images, _nhwc4=True)
            if self._head_normalizes:  # the encoder's last kernel applies F.normalize itself (same bits)
                return EmbeddingBatch(indices=batch.indices, embeddings=self._forward_nhwc4(x4, normalized=True))
            x = self._forward_nhwc4(x4)
        else:
            x = self.forward(self.preprocess(batch.images))
        x = l2_normalize_channels(x)
        return EmbeddingBatch(indices=batch.indices, embeddings=x)

    # an encoder whose `_forward_nhwc4(x4, normalized=True)` returns the L2-normalised embedding (fused into its tail)
    _head_normalizes = False

    def _forward_nhwc4(self, x4: Tensor) -> Tensor:
        """`forward` from the stem's own input layout `[B, H, W, 4]` (RGB + a zero channel); optional."""
        raise NotImplementedError

    def _fused_predict_ok(self) -> bool:
        """The fused preprocess -> forward path is taken only when `forward`, `preprocess` and `_forward_nhwc4` are
        all the library class's own: a user subclass that overrides `forward` or `preprocess` (the two methods the
        reference's subclasses implement, embedding.py:42-55) gets exactly `forward(preprocess(images))`."""
        cls = type(self)
        owner = next((c for c in cls.__mro__ if "_forward_nhwc4" in c.__dict__), EmbeddingModule)
        if owner is EmbeddingModule:
            return False
        return (cls.forward is owner.forward and cls.preprocess is owner.preprocess
                and cls._forward_nhwc4 is owner._forward_nhwc4)

    def embed_images(
        self,
        dataloader: Iterable[ImageBatch],
        *,
        accelerator: str = "auto",
        devices: list[int] | str | int = "auto",
    ) -> list[EmbeddingBatch]:
        """One `EmbeddingBatch` per input batch, in loader order, `indices` passed through unchanged
        (reference: embedding.py:78-98, where Lightning's `Trainer.predict` runs the loop).

        `accelerator` must resolve to the GPU ("auto", "gpu", "cuda"); `devices` picks the HIP device of THIS
        process (an int index, a one-element list, or "auto" = the module's current device).  Whole batches are
        never split across GPUs -- the normalisation statistics are batch-wide (transforms.py:62-65)."""
        if accelerator not in ("auto", "gpu", "cuda"):
            raise ValueError(f"accelerator {accelerator!r} is not available: imagescry_amd runs on HIP devices only")
        if devices != "auto":
            ids = [devices] if isinstance(devices, int) else list(devices)
            if len(ids) != 1:
                raise ValueError("one process drives one GPU; launch one process per device for more")
            self.to(torch.device("cuda", int(ids[0])))
        elif self.device.type != "cuda":
            self.to(torch.device("cuda", torch.cuda.current_device()))
        results: list[EmbeddingBatch] = []
        for batch in dataloader:
            results.append(self.predict_step(batch.to(self.device)))
        return results


# The convolution kernels index activations with 32-bit ELEMENT offsets: a pass holds at most this many elements in
# its largest activation (tests lower it to take the multi-pass branch at small sizes).
MAX_ACTIVATION_ELEMENTS = 2**31 - 1


def images_per_pass(batch: int, per_image_elements: int) -> int:
    """Images one pass of an encoder may hold so that `per_image_elements` x images stays addressable."""
    return max(1, min(batch, MAX_ACTIVATION_ELEMENTS // max(per_image_elements, 1)))


def lib_nchw_to_nhwc(x: Tensor, x4: Tensor) -> int:
    """float32 `[B, C, H, W]` -> `[B, H, W, 4]` with the channels past C zero (status code of the C call)."""
    b, c, h, w = x.shape
    return _lib.load().isc_nchw_to_nhwc(x.data_ptr(), b, c, h, w, 4, x4.data_ptr(), _lib.stream_handle(x.device))


def _conv(x: Tensor, conv: resnet50.FoldedConv, act: int, residual: Tensor | None = None) -> Tensor:
    """NHWC float32 convolution + bias (+ residual) + activation through `isc_conv2d_nhwc`."""
    b, h, w, cin = x.shape
    cout = conv.weight.shape[0]
    ho = (h + 2 * conv.pad - conv.kernel) // conv.stride + 1
    wo = (w + 2 * conv.pad - conv.kernel) // conv.stride + 1
    out = torch.empty((b, ho, wo, cout), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    st = lib.isc_conv2d_nhwc(
        x.data_ptr(), b, h, w, cin, conv.weight.data_ptr(), cout, conv.kernel, conv.kernel, conv.stride, conv.pad,
        conv.bias.data_ptr(), _lib.ptr(residual), act, out.data_ptr(), _lib.stream_handle(x.device),
    )
    _lib.check(st, "isc_conv2d_nhwc")
    return out


def _conv_dual(x: Tensor, x2: Tensor, conv: resnet50.FoldedConv, act: int) -> Tensor:
    """`act(w[:, :Cin] . x + w[:, Cin:] . x2[:, ::s, ::s] + bias)`: a bottleneck's conv3 with its projection shortcut folded
    in (`isc_conv2d_nhwc_dual`; `conv.stride` is the shortcut's stride, `conv.weight` the two matrices side by side)."""
    b, h, w, cin = x.shape
    _, h2, w2, cin2 = x2.shape
    cout = conv.weight.shape[0]
    out = torch.empty((b, h, w, cout), dtype=torch.float32, device=x.device)
    st = _lib.load().isc_conv2d_nhwc_dual(
        x.data_ptr(), b, h, w, cin, x2.data_ptr(), h2, w2, cin2, conv.stride, conv.weight.data_ptr(), cout,
        conv.bias.data_ptr(), None, act, out.data_ptr(), _lib.stream_handle(x.device),
    )
    _lib.check(st, "isc_conv2d_nhwc_dual")
    return out


class ResNet50Embedder(EmbeddingModule):
    """ResNet-50 trunk -> global average pool -> linear projection to `embedding_dim` (BASELINE.json config 2).

    Mirrors the constructor style of the reference's `EfficientNetEmbedder` (embedding.py:111-147): keyword-only
    arguments, `max_side_length` resize policy, random weights unless a state dict is given.  The output map is
    `[B, embedding_dim, 1, 1]`, so `get_flat_vectors()` yields one bank row per image.
    """

    def __init__(
        self,
        *,
        embedding_dim: int = 768,
        max_side_length: int = 640,
        state_dict: dict[str, Tensor] | None = None,
        seed: int = 0,
    ) -> None:
        super().__init__()
        if embedding_dim <= 0 or embedding_dim % 4 != 0:
            raise ValueError(f"embedding_dim must be a positive multiple of 4, got {embedding_dim}")
        if max_side_length <= 0:
            raise ValueError(f"max_side_length must be positive, got {max_side_length}")
        self._embedding_dim = embedding_dim
        self.max_side_length = max_side_length
        self.hparams = {"embedding_dim": embedding_dim, "max_side_length": max_side_length}
        sd = state_dict if state_dict is not None else resnet50.make_state_dict(embedding_dim=embedding_dim, seed=seed)
        if sd["fc.weight"].shape[0] != embedding_dim:
            raise ValueError(f"state dict projects to {sd['fc.weight'].shape[0]} dims, expected {embedding_dim}")
        self._net = resnet50.fold_state_dict(sd)

    def _move(self, device: torch.device) -> None:
        self._net = self._net.to(device)

    @property
    def embedding_dim(self) -> int:
        return self._embedding_dim

    def preprocess(self, images: Tensor, *, _nhwc4: bool = False) -> Tensor:
        """Resize so the long side is at most `max_side_length`, then batch-statistics normalise and clip to
        [-3, 3] (reference: embedding.py:149-165).  `_nhwc4`: see `normalize_per_channel`."""
        if not isinstance(images, Tensor) or images.dtype != torch.uint8:
            raise TypeError("images must be a uint8 tensor")
        if images.ndim != 4:
            raise ValueError(f"images must have shape [B, C, H, W], got {tuple(images.shape)}")
        h, w = images.shape[-2:]
        if max(h, w) > self.max_side_length:
            images = resize(images, output_size=self.max_side_length, side_ref="long")
        return normalize_per_channel(images, min_value=-3, max_value=3, _nhwc4=_nhwc4)

    def forward(self, x: Tensor) -> Tensor:
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            raise TypeError("x must be a float32 tensor")
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError(f"x must have shape [B, 3, H, W], got {tuple(x.shape)}")
        _lib.require_device(x, "x")
        if self.device != x.device:
            raise ValueError(f"module is on {self.device} but the input is on {x.device}; call .to() first")
        x = x.contiguous()
        b, c, h, w = x.shape
        # NCHW -> NHWC with a zero fourth channel, the layout of the stem
        x4 = torch.empty((b, h, w, 4), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib_nchw_to_nhwc(x, x4), "isc_nchw_to_nhwc")
        return self._forward_nhwc4(x4)

    _head_normalizes = True

    def _forward_nhwc4(self, x4: Tensor, normalized: bool = False) -> Tensor:
        _lib.require_device(x4, "x")
        if self.device != x4.device:
            raise ValueError(f"module is on {self.device} but the input is on {x4.device}; call .to() first")
        b, h, w, _ = x4.shape
        ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
        # the kernels index with 32-bit element offsets: bound the images per pass (64 ho wo elements in the stem
        # output and in layer1's 256-channel output at half the resolution; 4x margin)
        chunk = images_per_pass(b, ho * wo * 256)
        out = torch.empty((b, self._embedding_dim), dtype=torch.float32, device=x4.device)
        with torch.cuda.device(x4.device):
            for b0 in range(0, b, chunk):
                self._forward_chunk(x4[b0 : b0 + chunk], out[b0 : b0 + chunk], normalized)
        return out[:, :, None, None]

    def _forward_chunk(self, x4: Tensor, out: Tensor, normalized: bool) -> None:
        lib = _lib.load()
        stream = _lib.stream_handle(x4.device)
        net = self._net
        b, h, w, _ = x4.shape
        dev = x4.device
        ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
        # stem: the 7x7 / 2 convolution in the kernel's packed-K mode (RGB + a zero channel)
        y = torch.empty((b, ho, wo, 64), dtype=torch.float32, device=dev)
        st = lib.isc_conv2d_nhwc(
            x4.data_ptr(), b, h, w, 4, net.stem.weight.data_ptr(), 64, 7, 7, 2, 3, net.stem.bias.data_ptr(), None,
            _lib.ISC_ACT_RELU, y.data_ptr(), stream,
        )
        _lib.check(st, "isc_conv2d_nhwc (stem)")
        hp, wp = (ho + 2 - 3) // 2 + 1, (wo + 2 - 3) // 2 + 1
        pooled = torch.empty((b, hp, wp, 64), dtype=torch.float32, device=dev)
        _lib.check(lib.isc_maxpool_nhwc(y.data_ptr(), b, ho, wo, 64, 3, 2, 1, pooled.data_ptr(), stream),
                   "isc_maxpool_nhwc")
        y = pooled
        for blk in net.blocks:
            t = _conv(y, blk.conv1, _lib.ISC_ACT_RELU)
            t = _conv(t, blk.conv2, _lib.ISC_ACT_RELU)
            if blk.fused is not None:  # the projection shortcut inside conv3 (resnet50.FUSED_SHORTCUT_STAGES)
                y = _conv_dual(t, y, blk.fused, _lib.ISC_ACT_RELU)
                continue
            identity = y if blk.downsample is None else _conv(y, blk.downsample, _lib.ISC_ACT_NONE)
            y = _conv(t, blk.conv3, _lib.ISC_ACT_RELU, residual=identity)
        # tail in one launch: global average pool -> projection (-> F.normalize when predict_step asks for it)
        bb, hh, ww, cc = y.shape
        st = lib.isc_pool_linear_l2norm(y.data_ptr(), bb, hh, ww, cc, net.fc.weight.data_ptr(), net.fc.bias.data_ptr(),
                                        self._embedding_dim, int(normalized), 1e-12, out.data_ptr(), stream)
        _lib.check(st, "isc_pool_linear_l2norm")


class EfficientNetEmbedder(EmbeddingModule):
    """Embedding model using EfficientNetV2 as the backbone feature extractor -- the reference's concrete embedder
    (src/imagescry/models/embedding.py:108-183), same constructor, same output geometry
    `[B, 1280, ceil(H/32), ceil(W/32)]` (one embedding vector per 32 x 32 pixel cell).

    `pretrained=True` needs the torchvision weight download (embedding.py:135-141), which this offline build cannot
    perform; pass a torchvision `features` state dict through `state_dict` instead.
    """

    def __init__(
        self,
        *,
        backbone_size: str = "s",
        max_side_length: int = 640,
        pretrained: bool = False,
        state_dict: dict[str, Tensor] | None = None,
        seed: int = 0,
    ) -> None:
        super().__init__()
        if backbone_size not in efficientnet.STAGES:
            raise ValueError(f"Invalid model size: {backbone_size}")
        if pretrained and state_dict is None:
            raise RuntimeError(
                "pretrained weights must be downloaded (EfficientNet_V2_*_Weights.DEFAULT) and there is no network here; "
                "pass the torchvision `features` state dict via `state_dict=`"
            )
        self._embedding_dim = efficientnet.LAST_CHANNELS
        self.backbone_size = backbone_size
        self.max_side_length = max_side_length
        self.hparams = {"backbone_size": backbone_size, "max_side_length": max_side_length}
        sd = state_dict if state_dict is not None else efficientnet.make_state_dict(backbone_size, seed=seed)
        self._net = efficientnet.fold_state_dict(sd, backbone_size)

    def _move(self, device: torch.device) -> None:
        self._net = self._net.to(device)

    @property
    def embedding_dim(self) -> int:
        return self._embedding_dim

    def preprocess(self, images: Tensor, *, _nhwc4: bool = False) -> Tensor:
        """reference: embedding.py:149-165.  `_nhwc4`: see `normalize_per_channel`."""
        if not isinstance(images, Tensor) or images.dtype != torch.uint8:
            raise TypeError("images must be a uint8 tensor")
        if images.ndim != 4:
            raise ValueError(f"images must have shape [B, C, H, W], got {tuple(images.shape)}")
        h, w = images.shape[-2:]
        if max(h, w) > self.max_side_length:
            images = resize(images, output_size=self.max_side_length, side_ref="long")
        return normalize_per_channel(images, min_value=-3, max_value=3, _nhwc4=_nhwc4)

    def forward(self, x: Tensor) -> Tensor:
        """float32 `[B, 3, H, W]` -> float32 `[B, 1280, ceil(H/32), ceil(W/32)]` (an NCHW view of the kernels'
        channels-last result; reference: embedding.py:167-177)."""
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            raise TypeError("x must be a float32 tensor")
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError(f"x must have shape [B, 3, H, W], got {tuple(x.shape)}")
        _lib.require_device(x, "x")
        if self.device != x.device:
            raise ValueError(f"module is on {self.device} but the input is on {x.device}; call .to() first")
        x = x.contiguous()
        b, _c, h, w = x.shape
        x4 = torch.empty((b, h, w, 4), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib_nchw_to_nhwc(x, x4), "isc_nchw_to_nhwc")
        return self._forward_nhwc4(x4)

    def _forward_nhwc4(self, x4: Tensor) -> Tensor:
        _lib.require_device(x4, "x")
        if self.device != x4.device:
            raise ValueError(f"module is on {self.device} but the input is on {x4.device}; call .to() first")
        b, h, w, _ = x4.shape
        ho, wo = (h + 1) // 2, (w + 1) // 2
        chunk = images_per_pass(b, ho * wo * 256)  # largest activation of one image (32-bit kernel offsets), 4x margin
        outs = []
        with torch.cuda.device(x4.device):
            for b0 in range(0, b, chunk):
                outs.append(efficientnet.forward_features_nhwc4(self._net, x4[b0 : b0 + chunk]))
        y = outs[0] if len(outs) == 1 else torch.cat(outs)
        return y.permute(0, 3, 1, 2)


class ViTB16Embedder(EmbeddingModule):
    """ViT-B/16 -> 768-d embeddings, fp16 matrix-core arithmetic (BASELINE.json configs[4]).

    Same constructor style as the other embedders.  By default (`output="cls"`, `grid="fixed"`) `preprocess` resizes
    every batch to `image_size` x `image_size` (the reference's `resize` with a tuple size, transforms.py:78-126)
    before the batch-statistics normalisation and the output map is the class token, `[B, 768, 1, 1]`: one bank row per
    image.

    `output="patches"` returns the spatial map the reference's contract describes (embedding.py:57-76): `[B, 768, h, w]`,
    cell `(i, j)` = patch token `1 + i w + j` after the final LayerNorm, one bank row per 16 x 16-pixel patch of the
    resized image.  `grid="aspect"` keeps the aspect ratio: a `[B, 3, H, W]` batch is resized to `(16 h, 16 w)` with
    `(h, w) = vit.token_grid(H, W, config.grid ** 2)` and the position embeddings are resampled bicubically to that
    grid (`vit.position_table`); `forward` then takes any `[B, 3, 16 h, 16 w]` with `h w <= config.grid ** 2`.

    `max_patches` (with `grid="aspect"`, 1 .. `vit.MAX_PATCHES`) replaces `config.grid ** 2` in both places: 400 gives
    a 20 x 20 map of a square image, 1024 a 32 x 32 one.  Sequences of more than 224 tokens run on the streaming
    attention kernel (`isc_attention_f16_stream`) and in passes of fewer images (`vit.images_per_pass`).  A config whose
    own grid is larger than 14 x 14 needs no `max_patches`.
    """

    def __init__(
        self,
        *,
        config: vit.ViTConfig = vit.VIT_B16,
        state_dict: dict[str, Tensor] | None = None,
        seed: int = 0,
        max_images_per_pass: int = 1024,
        output: str = "cls",
        grid: str = "fixed",
        max_patches: int | None = None,
    ) -> None:
        super().__init__()
        if max_images_per_pass <= 0:
            raise ValueError(f"max_images_per_pass must be positive, got {max_images_per_pass}")
        if output not in ("cls", "patches"):
            raise ValueError(f'output must be "cls" or "patches", got {output!r}')
        if grid not in ("fixed", "aspect"):
            raise ValueError(f'grid must be "fixed" or "aspect", got {grid!r}')
        if max_patches is not None:
            if grid == "fixed":
                raise ValueError('max_patches needs grid="aspect": a fixed grid is the config\'s')
            if not 1 <= max_patches <= vit.MAX_PATCHES:
                raise ValueError(f"max_patches must be in 1 .. {vit.MAX_PATCHES}, got {max_patches}")
        self.config = config
        self.max_patches = max_patches
        self.max_images_per_pass = max_images_per_pass
        self.output = output
        self.grid = grid
        self.hparams = {"image_size": config.image_size, "patch_size": config.patch_size, "depth": config.depth}
        if (output, grid) != ("cls", "fixed"):
            self.hparams.update(output=output, grid=grid)
        if max_patches is not None:
            self.hparams.update(max_patches=max_patches)
        # the patch-token head applies F.normalize itself when predict_step asks for it (isc_vit_tokens_out)
        self._head_normalizes = output == "patches"
        sd = state_dict if state_dict is not None else vit.make_state_dict(config, seed=seed)
        self._net = self._prepare_net(sd)

    # the prepared tower and its pooled `[B, embedding_dim]` features of one pass (`SigLIPEmbedder` puts its tower and
    # its attention-pooling head here)
    def _prepare_net(self, sd: dict[str, Tensor]):
        return vit.prepare(sd, self.config)

    def _pooled(self, x: Tensor, grid: tuple[int, int], cap: int | None) -> Tensor:
        return vit.forward_cls(self._net, x, grid, max_patches=cap)

    def _move(self, device: torch.device) -> None:
        self._net = self._net.to(device)

    @property
    def embedding_dim(self) -> int:
        return self.config.embed_dim or self.config.dim  # a projection head (CLIP) sets the width

    @property
    def _patch_cap(self) -> int:
        """The most patches an aspect grid may hold."""
        return self.config.grid**2 if self.max_patches is None else self.max_patches

    def _resized(self, images: Tensor) -> Tensor:
        """uint8 `[B, C, H, W]` at the size this mode's `forward` takes: `image_size` squared, or the aspect grid's."""
        if not isinstance(images, Tensor) or images.dtype != torch.uint8:
            raise TypeError("images must be a uint8 tensor")
        if images.ndim != 4:
            raise ValueError(f"images must have shape [B, C, H, W], got {tuple(images.shape)}")
        if self.grid == "aspect":
            h, w = vit.token_grid(images.shape[-2], images.shape[-1], self._patch_cap)
            size = (h * self.config.patch_size, w * self.config.patch_size)
        else:
            size = (self.config.image_size, self.config.image_size)
        if tuple(images.shape[-2:]) != size:
            images = resize(images, output_size=size)
        return images

    def preprocess(self, images: Tensor) -> Tensor:
        return normalize_per_channel(self._resized(images), min_value=-3, max_value=3)

    def _token_grid_of(self, x: Tensor) -> tuple[int, int]:
        """The token grid `forward` runs a float32 input on, or ValueError for a shape this mode does not take."""
        s, p = self.config.image_size, self.config.patch_size
        if self.grid == "fixed":
            if x.ndim != 4 or tuple(x.shape[1:]) != (3, s, s):
                raise ValueError(f"x must have shape [B, 3, {s}, {s}], got {tuple(x.shape)}")
            return self.config.grid, self.config.grid
        ok = x.ndim == 4 and x.shape[1] == 3 and x.shape[2] > 0 and x.shape[3] > 0 and x.shape[2] % p == 0 and x.shape[3] % p == 0
        if not ok or (x.shape[2] // p) * (x.shape[3] // p) > self._patch_cap:
            raise ValueError(f"x must have shape [B, 3, {p} h, {p} w] with h w <= {self._patch_cap}, "
                             f"got {tuple(x.shape)}")
        return x.shape[2] // p, x.shape[3] // p

    def forward(self, x: Tensor) -> Tensor:
        return self._forward(x, normalized=False)

    # the patch map of one pass, written into `out`: the tokens behind the final LayerNorm, `config.dim` channels
    # (`CLIPEmbedder` with `dense=` puts its projected map here)
    @property
    def _patch_map_dim(self) -> int:
        return self.config.dim

    def _patch_map(self, x: Tensor, grid: tuple[int, int], normalized: bool, out: Tensor, cap: int | None) -> None:
        vit.forward_tokens(self._net, x, grid, normalize=normalized, out=out, max_patches=cap)

    def _forward(self, x: Tensor, normalized: bool) -> Tensor:
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            raise TypeError("x must be a float32 tensor")
        grid = self._token_grid_of(x)
        _lib.require_device(x, "x")
        if self.device != x.device:
            raise ValueError(f"module is on {self.device} but the input is on {x.device}; call .to() first")
        x = x.contiguous()
        b = x.shape[0]
        step = vit.images_per_pass(grid[0] * grid[1] + self.config.num_prefix, self.max_images_per_pass)
        cap = self._patch_cap if self.grid == "aspect" else None
        if self.output == "patches":
            out = torch.empty((b, self._patch_map_dim, *grid), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                for b0 in range(0, b, step):
                    self._patch_map(x[b0 : b0 + step], grid, normalized, out[b0 : b0 + step], cap)
            return out
        out = torch.empty((b, self.embedding_dim), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            for b0 in range(0, b, step):
                out[b0 : b0 + step] = self._pooled(x[b0 : b0 + step], grid, cap)
        return out[:, :, None, None]

    def predict_step(self, batch: ImageBatch) -> EmbeddingBatch:
        """As `EmbeddingModule.predict_step`; in patches mode the head normalises (one pass less over the map, the same
        bits as `l2_normalize_channels(forward(preprocess(images)))`).  A subclass that overrides `forward` or
        `preprocess` gets exactly `forward(preprocess(images))` and the separate normalisation."""
        cls = type(self)
        own = cls.forward is ViTB16Embedder.forward and cls._forward is ViTB16Embedder._forward
        if not (self._head_normalizes and own):
            return super().predict_step(batch)
        if not isinstance(batch, ImageBatch):
            raise TypeError(f"batch must be an ImageBatch, got {type(batch).__name__}")
        x = self.preprocess(batch.images)
        if x.ndim == 4 and x.shape[2] * x.shape[3] == self.config.patch_size**2:
            # a one-cell map: isc_l2norm_channels sums a lone row in another order than the head does
            return EmbeddingBatch(indices=batch.indices, embeddings=l2_normalize_channels(self.forward(x)))
        return EmbeddingBatch(indices=batch.indices, embeddings=self._forward(x, normalized=True))


# (variant, registers) -> configuration
DINOV2_PRESETS: dict[tuple[str, bool], vit.ViTConfig] = {
    ("vits14", False): vit.DINOV2_S14, ("vits14", True): vit.DINOV2_S14_REG,
    ("vitb14", False): vit.DINOV2_B14, ("vitb14", True): vit.DINOV2_B14_REG,
    ("vitl14", False): vit.DINOV2_L14, ("vitl14", True): vit.DINOV2_L14_REG,
}


class _CheckpointPreprocess:
    """The `preprocess="checkpoint"` mode of the embedders that load published checkpoints: the pipeline those were
    evaluated behind -- shorter side to `resize_size` by antialiased bicubic interpolation, centre crop of `crop_size`,
    rounding to uint8 levels, fixed per-channel statistics -- as one `resize_center_crop` call.  "Faithful" means the
    float arithmetic of torch / torchvision's antialiased TENSOR resize with the result rounded to uint8 levels; PIL's
    own resize rounds to uint8 after each of its two passes with fixed-point weights and can differ from it by one level
    on some pixels, which is not emulated."""

    def _init_preprocess(self, mode: str, crop_size: int | None, resize_size: int | None, default_crop: int,
                         default_resize, mean: tuple[float, ...], std: tuple[float, ...]) -> None:
        if mode not in ("squash", "checkpoint"):
            raise ValueError(f'preprocess must be "squash" or "checkpoint", got {mode!r}')
        self.preprocess_mode = mode
        self.crop_size = self.resize_size = None
        if mode == "squash":
            if crop_size is not None or resize_size is not None:
                raise ValueError('crop_size and resize_size need preprocess="checkpoint"')
            return
        for name, v in (("crop_size", crop_size), ("resize_size", resize_size)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v <= 0):
                raise ValueError(f"{name} must be a positive int, got {v!r}")
        crop = default_crop if crop_size is None else crop_size
        size = default_resize(crop) if resize_size is None else resize_size
        if size < crop:
            raise ValueError(f"resize_size {size} is smaller than crop_size {crop}: the crop would need padding")
        # the crop has to be a shape `forward` takes
        self._token_grid_of(torch.empty((1, 3, crop, crop), dtype=torch.float32, device="meta"))
        self.crop_size, self.resize_size = crop, size
        self._checkpoint_stats = (tuple(255.0 * v for v in mean), tuple(255.0 * v for v in std))
        self._checkpoint_stats_on: dict[torch.device, tuple[Tensor, Tensor]] = {}
        self.hparams.update(preprocess=mode, crop_size=crop, resize_size=size)

    def _checkpoint_preprocess(self, images: Tensor) -> Tensor:
        if not isinstance(images, Tensor) or images.dtype != torch.uint8:
            raise TypeError("images must be a uint8 tensor")
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError(f"images must have shape [B, 3, H, W], got {tuple(images.shape)}")
        if images.device not in self._checkpoint_stats_on:
            self._checkpoint_stats_on[images.device] = tuple(
                torch.tensor(v, dtype=torch.float32, device=images.device) for v in self._checkpoint_stats)
        mean, std = self._checkpoint_stats_on[images.device]
        return resize_center_crop(images, self.resize_size, self.crop_size, channel_means=mean, channel_stds=std,
                                  quantize=True)


class DINOv2Embedder(_CheckpointPreprocess, ViTB16Embedder):
    """DINOv2 ViT-S/B/L with a patch size of 14 -> 384 / 768 / 1024-d embeddings: `ViTB16Embedder` on one of the
    `vit.DINOV2_*` configurations (LayerScale; with `registers` four register tokens, which the patch map leaves out
    like the class token, and the antialiased position resampling of those checkpoints).

    `state_dict` takes a `dinov2_vit{s,b,l}14[_reg]` checkpoint under its facebookresearch/dinov2 or timm names, or a
    Hugging Face one through `vit.from_transformers_state_dict`; without it the weights are seeded random ones.  The
    checkpoints' native grid is 37 x 37 (518 pixels); `output="patches", grid="aspect", max_patches=256` turns a square
    image into a 16 x 16 map.  A grid other than the native one resamples the position table by its size
    (`transformers.Dinov2Model`), not with the hub models' `+ 0.1` offset.

    `preprocess="squash"` (the default) is this package's preprocessing (`resize` to the mode's size without regard to
    the aspect ratio + batch-statistics `normalize_per_channel`).  `preprocess="checkpoint"` is the published evaluation
    transform: the shorter side to `resize_size` by antialiased bicubic interpolation, a centre crop of `crop_size`,
    rounding to uint8 levels and the ImageNet statistics (`vit.IMAGENET_MEAN`, `vit.IMAGENET_STD`, times 255), in one
    kernel (`resize_center_crop`; what "faithful" means: `_CheckpointPreprocess`).  `crop_size` defaults to
    `config.image_size` with `grid="fixed"` and to 224 otherwise, `resize_size` to `round(crop_size * 8 / 7)` (the
    256 / 224 of that transform); the crop must be a shape `forward` takes."""

    def __init__(
        self,
        variant: str = "vitb14",
        registers: bool = False,
        *,
        state_dict: dict[str, Tensor] | None = None,
        seed: int = 0,
        max_images_per_pass: int = 1024,
        output: str = "cls",
        grid: str = "fixed",
        max_patches: int | None = None,
        preprocess: str = "squash",
        crop_size: int | None = None,
        resize_size: int | None = None,
    ) -> None:
        if not isinstance(registers, bool):
            raise TypeError(f"registers must be a bool, got {registers!r}")
        if (variant, registers) not in DINOV2_PRESETS:
            raise ValueError(f"variant must be one of {sorted({v for v, _ in DINOV2_PRESETS})}, got {variant!r}")
        super().__init__(config=DINOV2_PRESETS[variant, registers], state_dict=state_dict, seed=seed,
                         max_images_per_pass=max_images_per_pass, output=output, grid=grid, max_patches=max_patches)
        self.hparams.update(variant=variant, registers=registers)
        self._init_preprocess(preprocess, crop_size, resize_size, self.config.image_size if grid == "fixed" else 224,
                              lambda crop: round(crop * 8 / 7), vit.IMAGENET_MEAN, vit.IMAGENET_STD)

    def preprocess(self, images: Tensor) -> Tensor:
        if self.preprocess_mode == "checkpoint":
            return self._checkpoint_preprocess(images)
        return super().preprocess(images)


class CLIPEmbedder(_CheckpointPreprocess, ViTB16Embedder):
    """CLIP: images and texts in one space.  The vision tower is `ViTB16Embedder` on a `clip.PRESETS` configuration
    ("ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336": a LayerNorm in front of the blocks and a bias-free projection
    to E = 512 / 768 dimensions behind the class token) and yields `[B, E, 1, 1]` rows for an `EmbeddingBank`;
    `encode_text` runs the text tower on token ids and returns unit-norm float32 `[Q, E]` queries for `bank.search`.

    `state_dict` holds both towers under `clip`'s names (`clip.from_openai_state_dict`, `clip.from_transformers_state_dict`,
    `clip.make_state_dict`); without it the weights are seeded random ones.  `act` is a property of the checkpoint:
    "quick_gelu" for OpenAI's, "gelu" for open_clip / LAION ones.  `preset` may also be a `clip.CLIPConfig`.

    `output="patches"` needs `dense=`: the raw patch tokens, projected, are not what the checkpoints were trained to align
    with text, and without `dense` the mode is refused.  `dense="value"` (MaskCLIP), `"kk"` or `"qq"` (SCLIP / ClearCLIP
    self-self attention) is the standard training-free remedy, a change of the LAST block only (`vit.forward_dense` has
    the arithmetic): no residual and no MLP there, and in place of query-key attention the value path alone, or
    `softmax(K K^T / 8) V` / `softmax(Q Q^T / 8) V`; every token then goes through the final LayerNorm and the
    projection.  The result is the `[B, E, h, w]` map of the other patch embedders -- cell `(i, j)` = patch token
    `1 + i w + j`, `forward` unnormalised, `predict_step` L2-normalised by the head kernel (`isc_tokens_to_map`) -- in
    the TEXT tower's space: a bank of its rows with `row_groups` = the image index answers `bank.search_groups(
    model.encode_text(ids), k)`, "which images contain this, and where".  `grid="aspect"`, `max_patches` (above 224
    tokens the streaming kernels) and `preprocess="checkpoint"` work as for `ViTB16Embedder` / `DINOv2Embedder`.

    `preprocess="squash"` (the default) is this package's squash-`resize` to `image_size` (or, with `grid="aspect"`, to
    the aspect grid) and `normalize_per_channel` with CLIP's FIXED statistics (`clip.IMAGE_MEAN`, `clip.IMAGE_STD`,
    times 255; no eps, no clipping) -- batch statistics would break the alignment with the text side.
    `preprocess="checkpoint"` is the checkpoints' own pipeline: the SHORTER side to `resize_size` by antialiased bicubic
    interpolation, the centre square of `crop_size`, rounding to uint8 levels and the same statistics, in one kernel
    (`resize_center_crop`; what "faithful" means: `_CheckpointPreprocess`), so the tower sees no squashed and no border
    content.  `crop_size` defaults to `image_size` and `resize_size` to `crop_size`; the crop must be a shape `forward`
    takes.  `forward` takes any float32 input a caller preprocessed themselves."""

    def __init__(
        self,
        preset: str | clip.CLIPConfig = "ViT-B/16",
        *,
        state_dict: dict[str, Tensor] | None = None,
        act: str = "quick_gelu",
        seed: int = 0,
        max_images_per_pass: int = 1024,
        output: str = "cls",
        grid: str = "fixed",
        max_patches: int | None = None,
        preprocess: str = "squash",
        crop_size: int | None = None,
        resize_size: int | None = None,
        dense: str | None = None,
    ) -> None:
        if isinstance(preset, clip.CLIPConfig):
            cfg = preset
        elif preset in clip.PRESETS:
            cfg = clip.PRESETS[preset]
        else:
            raise ValueError(f"preset must be one of {sorted(clip.PRESETS)} or a clip.CLIPConfig, got {preset!r}")
        if dense is not None and dense not in vit.DENSE_MODES:
            raise ValueError(f"dense must be None or one of {vit.DENSE_MODES}, got {dense!r}")
        if output == "patches" and dense is None:
            raise ValueError('CLIPEmbedder has no output="patches" without dense=: the projected raw patch tokens do not '
                             'live in the text tower\'s space; dense="value", "kk" or "qq" gives a patch map that does')
        if output not in ("cls", "patches"):
            raise ValueError(f'CLIPEmbedder has no output={output!r}: "cls" (the projected class token) or "patches" '
                             "(with dense=)")
        if dense is not None and output != "patches":
            raise ValueError(f'dense={dense!r} needs output="patches": the class token has no dense form')
        cfg = clip.with_act(cfg, act)
        sd = state_dict if state_dict is not None else clip.make_state_dict(cfg, seed=seed)
        super().__init__(config=cfg.vision, state_dict=clip.tower(sd, "visual"), seed=seed,
                         max_images_per_pass=max_images_per_pass, output=output, grid=grid, max_patches=max_patches)
        self.clip_config = cfg
        self.dense = dense
        # the value third of the last block's qkv projection, only where it is the whole of that block's attention
        self._dense_value = (vit.prepare_value_linear(clip.tower(sd, "visual"), f"blocks.{cfg.vision.depth - 1}")
                             if dense == "value" else None)
        self._text = clip.prepare_text(clip.tower(sd, "text"), cfg.text)
        self.hparams.update(act=act, embed_dim=cfg.embed_dim)
        if dense is not None:
            self.hparams.update(dense=dense)
        if isinstance(preset, str):
            self.hparams.update(preset=preset)
        self._stats: dict[torch.device, tuple[Tensor, Tensor]] = {}
        self._init_preprocess(preprocess, crop_size, resize_size, self.config.image_size, lambda crop: crop,
                              clip.IMAGE_MEAN, clip.IMAGE_STD)

    def _move(self, device: torch.device) -> None:
        super()._move(device)
        self._text = self._text.to(device)
        if self._dense_value is not None:
            self._dense_value = self._dense_value.to(device)

    @property
    def _patch_map_dim(self) -> int:
        return self.embedding_dim

    def _patch_map(self, x: Tensor, grid: tuple[int, int], normalized: bool, out: Tensor, cap: int | None) -> None:
        vit.forward_dense(self._net, x, self.dense, grid, normalize=normalized, out=out, max_patches=cap,
                          value=self._dense_value)

    def preprocess(self, images: Tensor) -> Tensor:
        if self.preprocess_mode == "checkpoint":
            return self._checkpoint_preprocess(images)
        images = self._resized(images)
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError(f"images must have shape [B, 3, H, W], got {tuple(images.shape)}")
        if images.device not in self._stats:
            self._stats[images.device] = tuple(
                (torch.tensor(v, device=images.device) * 255.0).reshape(1, 3, 1, 1) for v in (clip.IMAGE_MEAN, clip.IMAGE_STD))
        mean, std = self._stats[images.device]
        return normalize_per_channel(images, channel_means=mean, channel_stds=std, eps=0.0)

    def encode_text(self, ids: Tensor, *, normalize: bool = True, validate: bool = True) -> Tensor:
        """int64 / int32 `[Q, T <= context]` token ids (on the module's device, or on the CPU: copied over) -> float32
        `[Q, E]` on the device, unit norm unless `normalize=False`.  `validate` (`clip.forward_text`): ids outside the
        vocabulary raise ValueError after one host read; without it the call makes none."""
        clip.check_ids(ids, self.clip_config.text)
        if self.device.type != "cuda":
            raise _lib.HipLibraryError("the module is on the CPU; call .to() first: imagescry_amd runs on HIP devices only")
        if ids.device.type == "cpu":
            ids = ids.to(self.device)
        elif ids.device != self.device:
            raise ValueError(f"module is on {self.device} but ids are on {ids.device}")
        q = clip.forward_text(self._text, ids, validate=validate)
        return l2_normalize_channels(q[:, :, None, None]).reshape(q.shape) if normalize and q.shape[0] else q

    def segment(self, batch: ImageBatch, text_embeddings: Tensor, *, class_of: "Tensor | list[int] | None" = None,
                size: tuple[int, int] | None = None, window: "int | tuple[int, int] | None" = None,
                stride: "int | tuple[int, int] | None" = None, **kw: object) -> segmentation.LabelMaps:
        """Open-vocabulary segmentation: `predict_step(batch)`, then `segmentation.segment` of its patch map against
        `text_embeddings` (float32 `[C, E]`, `encode_text`) at `size`, by default the batch's own `(H, W)`; `class_of`,
        `min_score`, `return_*`: `segmentation.label_map`.  `LabelMaps.indices` carries `batch.indices`.  Needs
        `output="patches"` with a `dense` mode (only that map lives in the text tower's space), and refuses
        `preprocess="checkpoint"`, whose map covers the centre crop and not the image.

        `window=` (an int or `(win_h, win_w)`, clamped to the image) switches to sliding-window inference, the way the
        dense CLIP methods are evaluated: `segmentation.crop_windows` of the images at `stride` (default: half the window,
        rounded up), `predict_step` of the crops -- each squashed to what the tower takes, `max_images_per_pass` splitting
        the larger batch -- and `segmentation.segment_windows` at the batch's own `(H, W)`, the windows that overlap on
        a pixel averaged there.  Another `size` is refused with a window."""
        if self.output != "patches" or self.dense is None:
            raise ValueError('segment needs the dense patch map: build the CLIPEmbedder with output="patches" and dense=')
        if self.preprocess_mode == "checkpoint":
            raise ValueError('segment refuses preprocess="checkpoint": its patch map covers the centre crop only, so it '
                             "does not line up with the image's pixels; use preprocess=\"squash\"")
        own = (int(batch.images.shape[2]), int(batch.images.shape[3]))
        if window is None:
            if stride is not None:
                raise ValueError("stride needs window=")
            return segmentation.segment(self.predict_step(batch), text_embeddings, own if size is None else size,
                                        class_of=class_of, **kw)
        if size is not None and tuple(size) != own:
            raise ValueError(f"segment with window= labels the batch's own {own} pixels; resizing the averaged scores to "
                             f"size={tuple(size)} is not supported")
        crops = segmentation.crop_windows(batch.images, window, stride)
        crops = ImageBatch(indices=batch.indices.repeat_interleave(crops.shape[0] // max(len(batch), 1)), images=crops)
        out = segmentation.segment_windows(self.predict_step(crops), text_embeddings, own, window, stride,
                                           class_of=class_of, **kw)
        return segmentation.LabelMaps(out.labels, out.scores, out.margins, out.counts, batch.indices)


class SigLIPEmbedder(ViTB16Embedder):
    """SigLIP / SigLIP 2: images and texts in one space, scored per pair by a sigmoid.  The vision tower is the `vit`
    encoder on a `siglip.PRESETS` configuration ("ViT-B/16", "ViT-B/16@256" / "@384" / "@512", "ViT-L/16@256" / "@384",
    each also as "...-siglip2": no class token, tanh GELU) followed by the attention-pooling head (`siglip.forward_image`)
    and yields `[B, D, 1, 1]` rows for an `EmbeddingBank`; `encode_text` runs the text tower on token ids and returns
    unit-norm float32 `[Q, D]` queries for `bank.search`.  `probability` turns the cosines a search returns into the
    pair probabilities the checkpoint was trained to give and `score_for_probability` inverts it, so that
    `bank.search_range(q, min_score=model.score_for_probability(0.5))` is "every image that matches".

    `state_dict` holds both towers, `logit_scale` and `logit_bias` under `siglip`'s names
    (`siglip.from_transformers_state_dict`, `siglip.make_state_dict`); without it the weights are seeded random ones.
    `preset` may also be a `siglip.SigLIPConfig`.  The So400m checkpoints (head size 72) and the NaFlex variants are
    refused.

    `grid="fixed"` squashes to `image_size`; `grid="aspect"`, `max_patches=` resample the position table bicubically
    (without antialiasing, as `transformers` does); above 224 tokens the streaming attention kernel and
    `vit.images_per_pass` apply as for the other embedders.  `preprocess="squash"` (the default) is this package's
    squash-`resize` and `normalize_per_channel` with the FIXED statistics mean = std = 0.5 (times 255).
    `preprocess="checkpoint"` is the SigLIP processor's pipeline in one kernel (`resize_antialias`): antialiased bicubic
    squash to the input size -- no aspect preservation, no crop --, rounding to uint8 levels, then the same statistics;
    "faithful" as `_CheckpointPreprocess` defines it (PIL's own two-pass rounding is not emulated).

    `output="patches"` is refused: a dense SigLIP map (the head's value path per token) is a follow-up, not part of this
    embedder."""

    def __init__(
        self,
        preset: str | siglip.SigLIPConfig = "ViT-B/16",
        *,
        state_dict: dict[str, Tensor] | None = None,
        seed: int = 0,
        max_images_per_pass: int = 1024,
        output: str = "cls",
        grid: str = "fixed",
        max_patches: int | None = None,
        preprocess: str = "squash",
    ) -> None:
        if isinstance(preset, siglip.SigLIPConfig):
            cfg = preset
        elif preset in siglip.PRESETS:
            cfg = siglip.PRESETS[preset]
        else:
            raise ValueError(f"preset must be one of {sorted(siglip.PRESETS)} or a siglip.SigLIPConfig, got {preset!r}")
        if output == "patches":
            raise ValueError('SigLIPEmbedder has no output="patches": a dense SigLIP map (the pooling head\'s value path '
                             "per token) is a follow-up and not part of this embedder")
        if output != "cls":
            raise ValueError(f'SigLIPEmbedder has no output={output!r}: "cls" (the pooled embedding) only')
        if preprocess not in ("squash", "checkpoint"):
            raise ValueError(f'preprocess must be "squash" or "checkpoint", got {preprocess!r}')
        if cfg.vision.dim != cfg.text.embed_dim:
            raise ValueError(f"the towers embed into {cfg.vision.dim} and {cfg.text.embed_dim} dimensions")
        sd = state_dict if state_dict is not None else siglip.make_state_dict(cfg, seed=seed)
        for key in ("logit_scale", "logit_bias"):
            if key not in sd or sd[key].numel() != 1:
                raise ValueError(f"the state dict needs `{key}`, one float")
        super().__init__(config=cfg.vision, state_dict=siglip.tower(sd, "visual"), seed=seed,
                         max_images_per_pass=max_images_per_pass, output=output, grid=grid, max_patches=max_patches)
        self.siglip_config = cfg
        self.logit_scale, self.logit_bias = float(sd["logit_scale"]), float(sd["logit_bias"])
        self._text = siglip.prepare_text(siglip.tower(sd, "text"), cfg.text)
        self.preprocess_mode = preprocess
        self.hparams.update(embed_dim=cfg.embed_dim, preprocess=preprocess)
        if isinstance(preset, str):
            self.hparams.update(preset=preset)
        self._stats: dict[torch.device, tuple[Tensor, Tensor]] = {}

    def _prepare_net(self, sd: dict[str, Tensor]):
        return siglip.prepare_vision(sd, self.config)

    def _pooled(self, x: Tensor, grid: tuple[int, int], cap: int | None) -> Tensor:
        return siglip.forward_image(self._net, x, grid, max_patches=cap)

    def _move(self, device: torch.device) -> None:
        super()._move(device)
        self._text = self._text.to(device)

    def preprocess(self, images: Tensor) -> Tensor:
        if not isinstance(images, Tensor) or images.dtype != torch.uint8:
            raise TypeError("images must be a uint8 tensor")
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError(f"images must have shape [B, 3, H, W], got {tuple(images.shape)}")
        if images.device not in self._stats:
            self._stats[images.device] = tuple(
                (torch.tensor(v, device=images.device) * 255.0).reshape(1, 3, 1, 1) for v in (siglip.IMAGE_MEAN, siglip.IMAGE_STD))
        mean, std = self._stats[images.device]
        if self.preprocess_mode == "checkpoint":
            if self.grid == "aspect":
                h, w = vit.token_grid(images.shape[-2], images.shape[-1], self._patch_cap)
                size = (h * self.config.patch_size, w * self.config.patch_size)
            else:
                size = (self.config.image_size, self.config.image_size)
            return resize_antialias(images, size, channel_means=mean, channel_stds=std, quantize=True)
        return normalize_per_channel(self._resized(images), channel_means=mean, channel_stds=std, eps=0.0)

    def encode_text(self, ids: Tensor, *, normalize: bool = True, validate: bool = True,
                    pad_to_context: bool = True) -> Tensor:
        """int64 / int32 `[Q, T <= context]` token ids (on the module's device, or on the CPU: copied over) -> float32
        `[Q, D]` on the device, unit norm unless `normalize=False`.  With `pad_to_context` shorter rows are right-padded
        with `pad_token_id` to `context` before the tower runs -- the checkpoints saw only such rows and pool position
        `context - 1`; without it the tower runs at the given T and pools `T - 1`.  `validate`
        (`siglip.forward_text`): ids outside the vocabulary raise ValueError after one host read; without it the call
        makes none."""
        text = self.siglip_config.text
        siglip.check_ids(ids, text)
        if self.device.type != "cuda":
            raise _lib.HipLibraryError("the module is on the CPU; call .to() first: imagescry_amd runs on HIP devices only")
        if ids.device.type == "cpu":
            ids = ids.to(self.device)
        elif ids.device != self.device:
            raise ValueError(f"module is on {self.device} but ids are on {ids.device}")
        if pad_to_context:
            ids = siglip.pad_ids(ids, text)
        q = siglip.forward_text(self._text, ids, validate=validate)
        return l2_normalize_channels(q[:, :, None, None]).reshape(q.shape) if normalize and q.shape[0] else q

    def probability(self, scores):
        """`sigmoid(exp(logit_scale) * scores + logit_bias)` of the cosines `bank.search`, `bank.scores` or
        `similarity_map` return (`siglip.probability`)."""
        return siglip.probability(scores, self.logit_scale, self.logit_bias)

    def score_for_probability(self, p: float) -> float:
        """The cosine at which `probability` is `p`: a `min_score` for `bank.search_range`."""
        return siglip.score_for_probability(p, self.logit_scale, self.logit_bias)
