"""Image transforms on MI355X: bilinear resize, antialiased bicubic resize + crop, and per-channel normalisation.

Same names, arguments and error behaviour as the reference module
(src/imagescry/image/transforms.py:16-197); the arithmetic runs in the HIP kernels of
`csrc/preprocess.hip` through the C ABI (`isc_channel_stats`, `isc_normalize_clip`,
`isc_resize_bilinear`).  Inputs must live on a HIP device -- there is no CPU path.

`resize_antialias` and `resize_center_crop` are not the reference's: they are the preprocessing the published ViT
checkpoints were evaluated behind (torchvision's `Resize(size, BICUBIC, antialias=True)` + `CenterCrop` on a tensor,
rounded to uint8 levels, then `Normalize`), in one kernel (`isc_resize_aa`).
"""

from __future__ import annotations

import math
from typing import Literal

import torch
from torch import Tensor

from imagescry_amd import _lib

__all__ = ["center_crop_geometry", "normalize_per_channel", "resize", "resize_antialias", "resize_center_crop", "to_4d"]

SideRef = Literal["height", "width", "long", "short"]


def to_4d(image_tensor: Tensor) -> Tensor:
    """Add leading phantom dimensions until the tensor is `[B, C, H, W]` (reference: transforms.py:130-164)."""
    if image_tensor.ndim == 2:
        return image_tensor.unsqueeze(0).unsqueeze(0)
    if image_tensor.ndim == 3:
        return image_tensor.unsqueeze(0)
    if image_tensor.ndim == 4:
        return image_tensor
    raise ValueError(f"Invalid image tensor shape: {image_tensor.shape}")


def _calc_scale_factor(height: int, width: int, output_size: int, side_ref: str) -> float:
    """reference: transforms.py:168-197."""
    if side_ref == "height":
        return output_size / height
    if side_ref == "width":
        return output_size / width
    if side_ref == "long":
        return output_size / max(height, width)
    if side_ref == "short":
        return output_size / min(height, width)
    raise ValueError(f"Invalid side_ref: {side_ref}")


def _kernel_input(image_tensor: Tensor, name: str) -> Tensor:
    """uint8 and float32 are read directly by the kernels; any other numeric dtype is cast to float32 first,
    which is what the reference's `.float()` does (transforms.py:59,103)."""
    if not isinstance(image_tensor, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(image_tensor).__name__}")
    if image_tensor.dtype == torch.bool or image_tensor.is_complex():
        raise TypeError(f"{name} must be a real numeric tensor, got {image_tensor.dtype}")
    _lib.require_device(image_tensor, name)
    if image_tensor.dtype not in (torch.uint8, torch.float32):
        image_tensor = image_tensor.float()
    return image_tensor.contiguous()


def resize(image_tensor: Tensor, output_size: int | tuple[int, int], *, side_ref: SideRef = "long") -> Tensor:
    """Bilinear resize (`align_corners=False`, no antialias) to float32 (reference: transforms.py:78-126).

    `output_size` as an int fixes the side named by `side_ref` and scales the other proportionally, the output
    being `floor(side * scale)` as `F.interpolate(..., recompute_scale_factor=True)` computes it; a tuple is exact.
    """
    if image_tensor.ndim < 2 or image_tensor.ndim > 4:
        raise ValueError(f"Invalid image tensor shape: {image_tensor.shape}")
    squeeze = 4 - image_tensor.ndim
    x = _kernel_input(to_4d(image_tensor), "image_tensor")
    b, c, h1, w1 = x.shape
    if isinstance(output_size, int):
        scale = _calc_scale_factor(h1, w1, output_size, side_ref)
        h2, w2 = math.floor(h1 * scale), math.floor(w1 * scale)
    else:
        h2, w2 = (int(v) for v in output_size)
    if h2 <= 0 or w2 <= 0:
        raise ValueError(f"Input and output sizes should be greater than 0, got output ({h2}, {w2})")
    y = torch.empty((b, c, h2, w2), dtype=torch.float32, device=x.device)
    if b * c > 0:
        lib = _lib.load()
        with torch.cuda.device(x.device):
            st = lib.isc_resize_bilinear(
                x.data_ptr(), _lib.dtype_code(x.dtype), b * c, h1, w1, h2, w2, y.data_ptr(), _lib.stream_handle(x.device)
            )
        _lib.check(st, "isc_resize_bilinear")
    for _ in range(squeeze):
        y = y.squeeze(0)
    return y


def _channel_stats(x: Tensor) -> tuple[Tensor, Tensor]:
    """Batch-wide per-channel mean and unbiased std -> two float32 `[C]` tensors (reference: transforms.py:62-65)."""
    b, c, h, w = x.shape
    lib = _lib.load()
    code = _lib.dtype_code(x.dtype)
    need = _lib.c_size_t()
    _lib.check(lib.isc_channel_stats_workspace_bytes(code, b, c, h, w, need), "isc_channel_stats_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
    stats = torch.empty((2, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.isc_channel_stats(
            x.data_ptr(), code, b, c, h, w, stats[0].data_ptr(), stats[1].data_ptr(), ws.data_ptr(), need.value,
            _lib.stream_handle(x.device),
        )
    _lib.check(st, "isc_channel_stats")
    return stats[0], stats[1]


def _stat_arg(t: Tensor, name: str, b: int, c: int, device: torch.device) -> tuple[Tensor, int]:
    """Validate a caller-supplied `#B C 1 1` statistic and flatten it to `[stat_batch * C]`."""
    if not isinstance(t, Tensor) or not t.dtype.is_floating_point:
        raise TypeError(f"{name} must be a floating point tensor")
    if t.ndim != 4 or t.shape[1] != c or t.shape[2:] != (1, 1) or t.shape[0] not in (1, b):
        raise ValueError(f"{name} must have shape [1 or {b}, {c}, 1, 1], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).reshape(-1).contiguous(), t.shape[0]


def normalize_per_channel(
    image_tensor: Tensor,
    *,
    channel_means: Tensor | None = None,
    channel_stds: Tensor | None = None,
    min_value: float | None = None,
    max_value: float | None = None,
    eps: float = 1e-6,
    _nhwc4: bool = False,
) -> Tensor:
    """`clip((x - mean_c) / (std_c + eps), min_value, max_value)` as float32 (reference: transforms.py:16-74).

    Without caller-supplied statistics the mean and the UNBIASED standard deviation are taken per channel over
    the whole batch (dims 0, 2, 3), so the result depends on the batch composition, exactly as in the reference.

    `_nhwc4` (not part of the reference's signature; used by `predict_step`): write the same values channels-last as
    `[B, H, W, 4]` with the channels past C zero -- the layout the convolution stems read (C <= 4).
    """
    if not isinstance(image_tensor, Tensor):
        raise TypeError(f"image_tensor must be a torch.Tensor, got {type(image_tensor).__name__}")
    if image_tensor.ndim != 4:
        raise ValueError(f"image_tensor must have shape [B, C, H, W], got {tuple(image_tensor.shape)}")
    x = _kernel_input(image_tensor, "image_tensor")
    b, c, h, w = x.shape
    if _nhwc4 and c > 4:
        raise ValueError(f"the channels-last output holds at most 4 channels, got {c}")
    y = torch.empty((b, h, w, 4) if _nhwc4 else (b, c, h, w), dtype=torch.float32, device=x.device)
    if x.numel() == 0:
        return y
    mean = std = None
    mean_b = std_b = 1
    if channel_means is not None:
        mean, mean_b = _stat_arg(channel_means, "channel_means", b, c, x.device)
    if channel_stds is not None:
        std, std_b = _stat_arg(channel_stds, "channel_stds", b, c, x.device)
    if mean is None or std is None:
        auto_mean, auto_std = _channel_stats(x)
        mean = auto_mean if mean is None else mean
        std = auto_std if std is None else std
    stat_batch = max(mean_b, std_b)
    if stat_batch > 1:  # one of the two is per-image: broadcast the other one
        if mean_b == 1:
            mean = mean.repeat(stat_batch)
        if std_b == 1:
            std = std.repeat(stat_batch)
    lo = -math.inf if min_value is None else float(min_value)
    hi = math.inf if max_value is None else float(max_value)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        st = (lib.isc_normalize_clip_nhwc4 if _nhwc4 else lib.isc_normalize_clip)(
            x.data_ptr(), _lib.dtype_code(x.dtype), b, c, h, w, mean.data_ptr(), std.data_ptr(), stat_batch,
            float(eps), lo, hi, y.data_ptr(), _lib.stream_handle(x.device),
        )
    _lib.check(st, "isc_normalize_clip")
    return y


def _channel_stat(t: Tensor | None, name: str, c: int, device: torch.device) -> Tensor | None:
    """A fixed `[1, C, 1, 1]` or `[C]` statistic as a float32 `[C]` device tensor."""
    if t is None:
        return None
    if not isinstance(t, Tensor) or not t.dtype.is_floating_point:
        raise TypeError(f"{name} must be a floating point tensor")
    if tuple(t.shape) not in ((c,), (1, c, 1, 1)):
        raise ValueError(f"{name} must have shape [{c}] or [1, {c}, 1, 1], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).reshape(-1).contiguous()


def resize_antialias(
    image_tensor: Tensor,
    output_size: tuple[int, int],
    *,
    crop: tuple[int, int, int, int] | None = None,
    channel_means: Tensor | None = None,
    channel_stds: Tensor | None = None,
    quantize: bool = False,
) -> Tensor:
    """Antialiased bicubic resize to `output_size = (H2, W2)` as float32: the arithmetic of
    `F.interpolate(x.float(), output_size, mode="bicubic", antialias=True, align_corners=False)`.

    `crop = (top, left, height, width)` returns that rectangle of the resized image, and only it is computed (bit for
    bit the slice of the full result).  `quantize` rounds to uint8 levels, `rint(clamp(v, 0, 255))`, as a pipeline that
    resizes to a uint8 image does.  `channel_means` / `channel_stds` (`[C]` or `[1, C, 1, 1]` floats in the units of the
    input, both or neither) then give `(v - mean_c) / std_c`, bit for bit `normalize_per_channel(..., eps=0.0)` of the
    unnormalised result.  Input handling as `resize`."""
    if not isinstance(image_tensor, Tensor):
        raise TypeError(f"image_tensor must be a torch.Tensor, got {type(image_tensor).__name__}")
    if image_tensor.ndim < 2 or image_tensor.ndim > 4:
        raise ValueError(f"Invalid image tensor shape: {image_tensor.shape}")
    squeeze = 4 - image_tensor.ndim
    x = _kernel_input(to_4d(image_tensor), "image_tensor")
    b, c, h1, w1 = x.shape
    h2, w2 = (int(v) for v in output_size)
    if h2 <= 0 or w2 <= 0:
        raise ValueError(f"Input and output sizes should be greater than 0, got output ({h2}, {w2})")
    top, left, hc, wc = (0, 0, h2, w2) if crop is None else (int(v) for v in crop)
    if top < 0 or left < 0 or hc <= 0 or wc <= 0 or top + hc > h2 or left + wc > w2:
        raise ValueError(f"crop {(top, left, hc, wc)} does not lie inside the resized image ({h2}, {w2})")
    if (channel_means is None) != (channel_stds is None):
        raise ValueError("channel_means and channel_stds go together: give both or neither")
    mean = _channel_stat(channel_means, "channel_means", c, x.device)
    std = _channel_stat(channel_stds, "channel_stds", c, x.device)
    y = torch.empty((b, c, hc, wc), dtype=torch.float32, device=x.device)
    if b * c > 0:
        if h1 <= 0 or w1 <= 0:
            raise ValueError(f"Input and output sizes should be greater than 0, got input ({h1}, {w1})")
        lib = _lib.load()
        need = _lib.c_size_t()
        _lib.check(lib.isc_resize_aa_workspace_bytes(h1, w1, h2, w2, top, left, hc, wc, need),
                   "isc_resize_aa_workspace_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            st = lib.isc_resize_aa(
                x.data_ptr(), _lib.dtype_code(x.dtype), b, c, h1, w1, h2, w2, top, left, hc, wc, _lib.ptr(mean),
                _lib.ptr(std), int(bool(quantize)), y.data_ptr(), ws.data_ptr(), need.value, _lib.stream_handle(x.device),
            )
        _lib.check(st, "isc_resize_aa")
    for _ in range(squeeze):
        y = y.squeeze(0)
    return y


def center_crop_geometry(height: int, width: int, size: int,
                         crop_size: int | tuple[int, int] | None = None) -> tuple[tuple[int, int], tuple[int, int, int, int]]:
    """`((H2, W2), (top, left, Hc, Wc))` of torchvision's `Resize(size)` + `CenterCrop(crop_size)` on a `height` x
    `width` image: the shorter side becomes `size` and the longer `int(size * long / short)`; the crop offsets are
    `int(round((H2 - Hc) / 2.0))` (round half to even, so margins of 1, 3 and 5 pixels start at 0, 2 and 2).
    `crop_size` defaults to `size`; a crop larger than the resized image raises ValueError (no padding)."""
    if height <= 0 or width <= 0 or size <= 0:
        raise ValueError(f"sizes must be positive, got image ({height}, {width}) and size {size}")
    if height <= width:
        h2, w2 = size, int(size * width / height)
    else:
        h2, w2 = int(size * height / width), size
    if crop_size is None:
        crop_size = size
    hc, wc = (crop_size, crop_size) if isinstance(crop_size, int) else (int(v) for v in crop_size)
    if hc <= 0 or wc <= 0:
        raise ValueError(f"crop_size must be positive, got ({hc}, {wc})")
    if hc > h2 or wc > w2:
        raise ValueError(f"crop ({hc}, {wc}) is larger than the resized image ({h2}, {w2}); there is no padding")
    return (h2, w2), (int(round((h2 - hc) / 2.0)), int(round((w2 - wc) / 2.0)), hc, wc)


def resize_center_crop(
    image_tensor: Tensor,
    size: int,
    crop_size: int | tuple[int, int] | None = None,
    *,
    channel_means: Tensor | None = None,
    channel_stds: Tensor | None = None,
    quantize: bool = False,
) -> Tensor:
    """`resize_antialias` with the geometry of `center_crop_geometry`: shorter side to `size`, centre crop of
    `crop_size` (default `size`) -- what torchvision's `Resize(size, BICUBIC)` + `CenterCrop(crop_size)` (+
    `Normalize` with the statistics) compute on a tensor."""
    if not isinstance(image_tensor, Tensor):
        raise TypeError(f"image_tensor must be a torch.Tensor, got {type(image_tensor).__name__}")
    if image_tensor.ndim < 2 or image_tensor.ndim > 4:
        raise ValueError(f"Invalid image tensor shape: {image_tensor.shape}")
    output_size, crop = center_crop_geometry(image_tensor.shape[-2], image_tensor.shape[-1], int(size), crop_size)
    return resize_antialias(image_tensor, output_size, crop=crop, channel_means=channel_means,
                            channel_stds=channel_stds, quantize=quantize)
