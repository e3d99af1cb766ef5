"""CPU restatement of the ViT patch-token path (test infrastructure, next to tests/collapse_oracle.py): the body of
`oracle.vit_oracle.vit_forward` with the position table resampled to the input's token grid, returning EVERY token
after the final LayerNorm.  Plain float32 torch; pinned against `transformers.ViTModel(interpolate_pos_encoding=True)`
in tests/test_vit_tokens_host.py."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor


def interpolate_pos_embed(pos_embed: Tensor, grid: tuple[int, int]) -> Tensor:
    """`[1, 1 + g * g, D]` -> `[1, 1 + h * w, D]`: class row kept, patch rows resampled with
    `F.interpolate(mode="bicubic", align_corners=False)`.  The native grid returns the table itself."""
    h, w = grid
    d = pos_embed.shape[-1]
    g = int(round((pos_embed.shape[1] - 1) ** 0.5))
    assert g * g + 1 == pos_embed.shape[1]
    if (h, w) == (g, g):
        return pos_embed
    patch = pos_embed[:, 1:].reshape(1, g, g, d).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(h, w), mode="bicubic", align_corners=False)
    return torch.cat([pos_embed[:, :1], patch.permute(0, 2, 3, 1).reshape(1, h * w, d)], dim=1)


def vit_tokens(sd: dict[str, Tensor], x: Tensor, *, patch: int = 16, heads: int = 12, eps: float = 1e-6,
               round_operands_fp16: bool = False) -> Tensor:
    """float32 `[B, 3, 16 h, 16 w]` -> float32 `[B, 1 + h * w, D]`, all tokens after the final LayerNorm (row 0 = class
    token).  `round_operands_fp16` as in `vit_forward`."""
    r = (lambda t: t.half().float()) if round_operands_fp16 else (lambda t: t)
    d = sd["cls_token"].shape[-1]
    b = x.shape[0]
    grid = (x.shape[2] // patch, x.shape[3] // patch)
    tok = F.conv2d(r(x), r(sd["patch_embed.proj.weight"]), sd["patch_embed.proj.bias"], stride=patch)
    tok = tok.flatten(2).transpose(1, 2)  # [B, h * w, D], patches row-major
    tok = torch.cat([sd["cls_token"].expand(b, -1, -1), tok], dim=1) + interpolate_pos_embed(sd["pos_embed"], grid)
    t = tok.shape[1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    for i in range(depth):
        p = f"blocks.{i}"
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], eps)
        qkv = F.linear(r(h), r(sd[f"{p}.attn.qkv.weight"]), sd[f"{p}.attn.qkv.bias"])
        qkv = r(qkv).reshape(b, t, 3, heads, d // heads).permute(2, 0, 3, 1, 4)  # [3, B, H, T, 64]
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = torch.softmax((q @ k.transpose(-1, -2)) * (d // heads) ** -0.5, dim=-1)
        a = (r(att) @ v).transpose(1, 2).reshape(b, t, d)
        tok = tok + F.linear(r(a), r(sd[f"{p}.attn.proj.weight"]), sd[f"{p}.attn.proj.bias"])
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"], eps)
        h = F.gelu(F.linear(r(h), r(sd[f"{p}.mlp.fc1.weight"]), sd[f"{p}.mlp.fc1.bias"]))
        tok = tok + F.linear(r(h), r(sd[f"{p}.mlp.fc2.weight"]), sd[f"{p}.mlp.fc2.bias"])
    return F.layer_norm(tok, (d,), sd["norm.weight"], sd["norm.bias"], eps)


def patch_map(tokens: Tensor, grid: tuple[int, int], normalize: bool = True) -> Tensor:
    """`[B, 1 + h * w, D]` -> the channels-first map `[B, D, h, w]` of the patch tokens, L2-normalised per cell."""
    b, _t, d = tokens.shape
    m = tokens[:, 1:].transpose(1, 2).reshape(b, d, *grid)
    return F.normalize(m, dim=1) if normalize else m
