"""CPU restatement of the DINOv2 encoder (test infrastructure, next to tests/vit_tokens_oracle.py): the pre-LN ViT of
`vit_tokens` with any patch size, register tokens between the class token and the patches (no position embedding),
LayerScale on the attention and the MLP branch, and the position table resampled to the input's token grid by plain or
antialiased bicubic interpolation.  Plain float32 torch; returns EVERY token after the final LayerNorm.  Pinned against
`transformers.Dinov2Model` and `Dinov2WithRegistersModel` in tests/test_dinov2_host.py."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor


def interpolate_pos_embed(pos_embed: Tensor, grid: tuple[int, int], antialias: bool = False) -> Tensor:
    """`[1, 1 + g * g, D]` -> `[1, 1 + h * w, D]`: class row kept, patch rows resampled with
    `F.interpolate(mode="bicubic", align_corners=False, antialias=antialias)` to the SIZE `grid`.  The native grid
    returns the table itself."""
    h, w = grid
    d = pos_embed.shape[-1]
    g = int(round((pos_embed.shape[1] - 1) ** 0.5))
    assert g * g + 1 == pos_embed.shape[1]
    if (h, w) == (g, g):
        return pos_embed
    patch = pos_embed[:, 1:].reshape(1, g, g, d).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(h, w), mode="bicubic", align_corners=False, antialias=antialias)
    return torch.cat([pos_embed[:, :1], patch.permute(0, 2, 3, 1).reshape(1, h * w, d)], dim=1)


def dinov2_tokens(sd: dict[str, Tensor], x: Tensor, *, patch: int = 14, heads: int = 12, eps: float = 1e-6,
                  antialias: bool = False, round_operands_fp16: bool = False) -> Tensor:
    """float32 `[B, 3, P h, P w]` -> float32 `[B, 1 + R + h * w, D]`, all tokens after the final LayerNorm (row 0 the
    class token, rows 1 .. R the registers when `sd` has `register_tokens`).  LayerScale where `sd` has
    `blocks.i.ls1.gamma`.  `round_operands_fp16`: every matrix-product operand is rounded to fp16 first, as the kernels
    round theirs; LayerScale, biases and the residual stream stay float32."""
    r = (lambda t: t.half().float()) if round_operands_fp16 else (lambda t: t)
    d = sd["cls_token"].shape[-1]
    b = x.shape[0]
    grid = (x.shape[2] // patch, x.shape[3] // patch)
    tok = F.conv2d(r(x), r(sd["patch_embed.proj.weight"]), sd["patch_embed.proj.bias"], stride=patch)
    tok = tok.flatten(2).transpose(1, 2)  # [B, h * w, D], patches row-major
    tok = torch.cat([sd["cls_token"].expand(b, -1, -1), tok], dim=1) + interpolate_pos_embed(sd["pos_embed"], grid, antialias)
    if "register_tokens" in sd:
        tok = torch.cat([tok[:, :1], sd["register_tokens"].expand(b, -1, -1), tok[:, 1:]], dim=1)
    t = tok.shape[1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    for i in range(depth):
        p = f"blocks.{i}"
        ls1, ls2 = sd.get(f"{p}.ls1.gamma", 1.0), sd.get(f"{p}.ls2.gamma", 1.0)
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], eps)
        qkv = F.linear(r(h), r(sd[f"{p}.attn.qkv.weight"]), sd[f"{p}.attn.qkv.bias"])
        qkv = r(qkv).reshape(b, t, 3, heads, d // heads).permute(2, 0, 3, 1, 4)  # [3, B, H, T, 64]
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = torch.softmax((q @ k.transpose(-1, -2)) * (d // heads) ** -0.5, dim=-1)
        a = (r(att) @ v).transpose(1, 2).reshape(b, t, d)
        tok = tok + ls1 * F.linear(r(a), r(sd[f"{p}.attn.proj.weight"]), sd[f"{p}.attn.proj.bias"])
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"], eps)
        h = F.gelu(F.linear(r(h), r(sd[f"{p}.mlp.fc1.weight"]), sd[f"{p}.mlp.fc1.bias"]))
        tok = tok + ls2 * F.linear(r(h), r(sd[f"{p}.mlp.fc2.weight"]), sd[f"{p}.mlp.fc2.bias"])
    return F.layer_norm(tok, (d,), sd["norm.weight"], sd["norm.bias"], eps)


def patch_map(tokens: Tensor, grid: tuple[int, int], prefix: int = 1, normalize: bool = True) -> Tensor:
    """`[B, prefix + h * w, D]` -> the channels-first map `[B, D, h, w]` of the patch tokens, L2-normalised per cell."""
    b, _t, d = tokens.shape
    m = tokens[:, prefix:].transpose(1, 2).reshape(b, d, *grid)
    return F.normalize(m, dim=1) if normalize else m


# ---------------------------------------------------------------------------------- the antialiased resampling bound
AA_GRIDS = [(5, 4, 6), (5, 7, 3), (5, 1, 1), (37, 16, 16)]  # (g, h, w): up- and downsampling, one cell, 518 -> 224 pixels


def cubic_aa(x: Tensor) -> Tensor:
    """The cubic convolution kernel with A = -0.5, float64."""
    a = -0.5
    x = x.abs()
    near = ((a + 2) * x - (a + 3)) * x * x + 1
    far = ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
    return torch.where(x < 1, near, torch.where(x < 2, far, torch.zeros_like(x)))


def aa_axis_weights(g: int, n: int) -> list[tuple[int, Tensor]]:
    """Per output index of an axis resampled from `g` to `n` samples: (first tap, normalised float64 weights) -- the
    taps within 2 max(s, 1) of the centre s (i + 0.5), s = g / n, weighted cubic((j - centre + 0.5) / max(s, 1))."""
    s = g / n
    support, inv = 2.0 * max(s, 1.0), 1.0 / max(s, 1.0)
    taps = []
    for i in range(n):
        centre = s * (i + 0.5)
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), g)
        w = cubic_aa((torch.arange(lo, hi, dtype=torch.float64) - centre + 0.5) * inv)
        taps.append((lo, w / w.sum()))
    return taps


def aa_restated_f64(pos: Tensor, g: int, h: int, w: int) -> Tensor:
    """`pos` [1 + g * g, D] -> float64 [1 + h * w, D] from the weights above: a second statement of what
    `F.interpolate(antialias=True)` computes, independent of torch's kernel."""
    d = pos.shape[1]
    src = pos[1:].double().reshape(g, g, d)
    wy = torch.zeros(h, g, dtype=torch.float64)
    wx = torch.zeros(w, g, dtype=torch.float64)
    for mat, n in ((wy, h), (wx, w)):
        for i, (lo, wt) in enumerate(aa_axis_weights(g, n)):
            mat[i, lo : lo + len(wt)] = wt
    out = torch.einsum("ya,xb,abd->yxd", wy, wx, src).reshape(h * w, d)
    return torch.cat([pos[:1].double(), out])


def aa_bound(g: int, h: int, w: int, top: float) -> float:
    """The largest difference allowed between a float32 evaluation of the antialiased table and the float64 one, for
    inputs of magnitude at most `top` (derivation: tests/test_dinov2_host.py)."""
    u = 2.0**-24

    def axis(n_out: int) -> tuple[int, float, float]:
        s = g / n_out
        inv = 1.0 / max(s, 1.0)
        taps = aa_axis_weights(g, n_out)
        n = max(len(wt) for _, wt in taps)
        a = max(float(wt.abs().sum()) for _, wt in taps)  # sum |w_i|, normalised weights
        # taps per unit of the raw (not yet normalised) weight sum
        q = max(len(wt) / float(cubic_aa((torch.arange(lo, lo + len(wt), dtype=torch.float64) - s * (i + 0.5) + 0.5)
                                         * inv).sum()) for i, (lo, wt) in enumerate(taps))
        rho = 2.8 * min(g, n_out) + 33.0  # error of one raw weight, in units of u
        return n, a, (1.0 + a) * q * rho + n * a * a + a  # ..., sum |error of w_i|, in units of u

    ny, ay, ey = axis(h)
    nx, ax, ex = axis(w)
    return u * top * ((ny + nx) * ay * ax + ay * ex + ax * ey)
