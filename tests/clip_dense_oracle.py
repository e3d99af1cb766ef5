"""CPU restatements for the dense CLIP patch map (`CLIPEmbedder(output="patches", dense=...)`) and the self-attention
entries behind it (test infrastructure next to tests/clip_oracle.py and tests/vit_bounds.py; a helper, not a conftest).

 * `clip_dense_features`: `clip_oracle.clip_image_features` with the LAST block replaced -- `h = LN1(x)`; `a = v_proj(h)`
   ("value"), `softmax(K K^T / 8) V` ("kk") or `softmax(Q Q^T / 8) V` ("qq") per head over all T tokens; `y = out_proj(a)
   + bias`, no residual, no MLP; `e = LN_post(y) . head.weight^T` -- for every patch token, as a `[B, E, h, w]` map
   (cell `(i, j)` = token `1 + i w + j`), float32 torch with the same `round_operands_fp16` switch.
 * `rewritten(qkv, part)`: the operand on which ordinary query-key attention IS self attention on part `part`: the query
   AND the key columns both hold that part (part 1 overwrites the q columns with k, part 0 the k columns with q), so NaN
   planted in the part a self kernel must not read is gone from it.
 * `self_selector_case`: z = +-4 in 64 dimensions in the columns of `part`.  After the kernel's exact 1/8 a row scores
   16 * 64 / 8 = 128 against itself and 16 * dot / 8 = 2 dot <= 128 - 2 gap against any other, gap = 64 - (largest dot
   product of two distinct +-1 rows): the situation `vit_bounds` derives for its selector (own score 128, every other
   key >= 32 lower once `key_gap >= 16`), with the identity as the permutation -- the kernel must EQUAL the value rows.
"""

from __future__ import annotations

import sys
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_oracle as co  # noqa: E402
import vit_bounds as vb  # noqa: E402
from dinov2_oracle import interpolate_pos_embed  # noqa: E402

MODES = ("value", "kk", "qq")
PART_QUERY, PART_KEY = 0, 1  # ISC_ATT_PART_QUERY, ISC_ATT_PART_KEY
PART_OF = {"qq": PART_QUERY, "kk": PART_KEY}
NAN = float("nan")

# (preset, image shape, grid mode, max_patches, tokens): ViT-B/32 on its fixed grid (50 tokens), ViT-B/16 on a 4 x 6
# aspect grid (25 tokens, resampled positions, not square: a transposed map fails), ViT-L/14 fixed (257 tokens: the
# streaming self kernel)
DENSE_CASES = [("ViT-B/32", (224, 224), "fixed", None, 50), ("ViT-B/16", (64, 96), "aspect", 24, 25),
               ("ViT-L/14", (224, 224), "fixed", None, 257)]


def clip_dense_features(sd: dict[str, Tensor], x: Tensor, *, patch: int, heads: int, mode: str, eps: float = 1e-5,
                        act: str = "quick_gelu", round_operands_fp16: bool = False) -> Tensor:
    """float32 `[B, 3, P h, P w]` -> float32 `[B, E, h, w]`, the dense patch map (not normalised)."""
    if mode not in MODES:
        raise ValueError(mode)
    r = co._rounding(round_operands_fp16)
    d = sd["visual.cls_token"].shape[-1]
    b = x.shape[0]
    gh, gw = x.shape[2] // patch, x.shape[3] // patch
    tok = F.conv2d(r(x), r(sd["visual.patch_embed.proj.weight"]), sd["visual.patch_embed.proj.bias"], stride=patch)
    tok = tok.flatten(2).transpose(1, 2)
    tok = torch.cat([sd["visual.cls_token"].expand(b, -1, -1), tok], dim=1) + interpolate_pos_embed(sd["visual.pos_embed"], (gh, gw))
    tok = F.layer_norm(tok, (d,), sd["visual.norm_pre.weight"], sd["visual.norm_pre.bias"], eps)
    depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("visual.blocks."))
    p = f"visual.blocks.{depth - 1}"
    if depth > 1:  # blocks 0 .. depth - 2 as they are
        front = {k: v for k, v in sd.items() if not k.startswith(p + ".")}
        tok = co._blocks(front, "visual", tok, heads, eps, act, False, r)
    t = tok.shape[1]
    h = F.layer_norm(tok, (d,), sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], eps)
    w_qkv, b_qkv = sd[f"{p}.attn.qkv.weight"], sd[f"{p}.attn.qkv.bias"]
    if mode == "value":
        a = F.linear(r(h), r(w_qkv[2 * d :]), b_qkv[2 * d :])
    else:
        qkv = r(F.linear(r(h), r(w_qkv), b_qkv)).reshape(b, t, 3, heads, d // heads).permute(2, 0, 3, 1, 4)
        z, v = qkv[PART_OF[mode]], qkv[2]
        att = torch.softmax((z @ z.transpose(-1, -2)) * (d // heads) ** -0.5, dim=-1)
        a = (r(att) @ v).transpose(1, 2).reshape(b, t, d)
    y = F.linear(r(a), r(sd[f"{p}.attn.proj.weight"]), sd[f"{p}.attn.proj.bias"])
    z = F.layer_norm(y, (d,), sd["visual.norm.weight"], sd["visual.norm.bias"], eps)
    e = F.linear(r(z), r(sd["visual.head.weight"]))  # [B, T, E]
    return e[:, 1:].transpose(1, 2).reshape(b, -1, gh, gw).contiguous()


def unit_cells(m: Tensor) -> Tensor:
    """`[B, E, h, w]` -> `[B h w, E]`, every cell at unit norm."""
    return F.normalize(m.permute(0, 2, 3, 1).reshape(-1, m.shape[1]), dim=1)


def rewritten(qkv: Tensor, part: int) -> Tensor:
    """`qkv` [B, T, 3 D] with its query and key columns both holding part `part` (module docstring)."""
    d = qkv.shape[-1] // 3
    out = qkv.clone()
    z = qkv[..., part * d : (part + 1) * d]
    out[..., :d], out[..., d : 2 * d] = z, z
    return out


def poisoned(qkv: Tensor, part: int) -> Tensor:
    """`qkv` with NaN in the one of the query / key parts that a self kernel on `part` must never read."""
    d = qkv.shape[-1] // 3
    out = qkv.clone()
    other = 1 - part
    out[..., other * d : (other + 1) * d] = NAN
    return out


def self_selector_case(b: int, t: int, heads: int, seed: int, part: int) -> dict:
    """`qkv` [B, T, 3 D] fp16 with +-4 rows in the columns of `part`, NaN in the other of the two parts and integer
    values; `want` = the value rows [B, T, D] fp16 (module docstring).  Raises unless the gap is at least MIN_GAP."""
    g = vb.gen(seed)
    keys = torch.randint(0, 2, (b, t, heads, 64), generator=g) * 2 - 1
    values = torch.randint(-2048, 2049, (b, t, heads, 64), generator=g)
    gap = vb.key_gap(keys)
    if gap < vb.MIN_GAP:
        raise ValueError(f"weak selector: two rows of one head are within {gap} of each other (need {vb.MIN_GAP})")
    z = (4.0 * keys.float()).reshape(b, t, heads * 64)
    other = torch.full_like(z, NAN)
    vals = values.float().reshape(b, t, heads * 64)
    qkv = torch.cat([z, other, vals] if part == PART_QUERY else [other, z, vals], dim=-1).half()
    return {"qkv": qkv, "want": vals.half(), "gap": gap}
