"""CPU restatements for the SigLIP towers and their kernels (test infrastructure, next to tests/clip_oracle.py and
tests/vit_bounds.py; a helper, not a conftest).

 * `siglip_image_features`, `siglip_text_features`: both towers in plain float32 torch under `imagescry_amd.siglip`'s
   state-dict names, pinned against `transformers.SiglipModel` in tests/test_siglip_host.py.
 * `gelu_tanh_bound`: the element-wise bound of the ISC_ACT_GELU_TANH epilogue, derived here.
 * `probe_reference`: the float64 one-query attention of isc_attention_f16_probe on fp16 operands and its element-wise bound.
 * `probe_uniform_case`, `probe_selector_case`: operands on which the kernel's result is exactly computable.

Tanh GELU epilogue.  Notation of vit_bounds (u = 2^-24, a hardware transcendental documented to one ulp has 2 u).  The
pre-activation v (accumulator + bias) is exact with the quanta of `vit_bounds.gemm_case`; with U = sqrt(2 / pi) (v +
0.044715 v^3) and s = sigmoid(2 U) the wanted value is 0.5 v (1 + tanh U) = v s, and the kernel computes, in float32
(include/imagescry_hip.h),

    z = fl(v v)                                                                          u
    p = fma(z, a, 1)       a = fl(0.044715): u; the term a z carries 2 u and is < p; the fma's u        |dp| <= 3 u p
    w = fl(v p)            = (v + 0.044715 v^3)(1 + 4 u)
    y = fl(w k)            k = fl(-2 log2(e) sqrt(2 / pi)): u; the product's u                          |dy| <= 6 u |y|
    t = exp2(y)            = exp(-2 U)(1 + theta): the argument's error enters as ln 2 |dy| = 6 u * 2 |U|, the
                           instruction's own error is 2 u                         |theta| <= tau = 2 u (1 + 6 |U|)
    d = fl(1 + t)          relative error t / (1 + t) tau + u = (1 - s) tau + u
    r = rcp(d)             one ulp: 2 u
    out = fl(v r)          u

    |out - v s| <= SLACK |v s| u (4 + 2 (1 - s)(1 + 6 |U|)) + (|v| + 1) 2^-126

((|v| + 1) 2^-126: where t is so large that r, or the product v r, is a subnormal the hardware may flush to zero -- r
moves by at most 2^-126, the product by |v| times that and by 2^-126 of its own; beyond that t is +inf and the result 0
where v s is below |v| 2^-128.  It never matters next to the first term on |v| <= 8.)  For v -> -inf the factor grows like |v|^3 while v s vanishes like |v| e^{-2 |U|}; for v -> +inf 1 - s vanishes
and the bound is 4 u |v|.  A float32 residual added afterwards is one more rounding, u (|want| + bound); an fp16 output one
fp16 rounding, h (|want| + bound) + 2^-25.  The erf GELU differs from the tanh form by up to 4.7e-4 (near |v| = 2.2): more
than two orders of magnitude outside this bound there, which `erf_is_outside` asserts on the operands of a test.

One-query attention (`probe_reference`).  With s_j = q . k_j / 8, A_j = |q| . |k_j| / 8, pi = softmax(s), want = sum_j
pi_j v_j and N = sum_j pi_j |v_j| (float64, per output element), the kernel documents, all in float32:
     - q / 8: exact (a power of two, float32 range)
     - scores: 64 exact products (fma) and 64 additions in a fixed order:              |ds_j| <= 64 u A_j
     - the exponent fl(fl(s_j - m) fl(log2 e)): the subtraction's u, the constant's u and the product's u on |s_j - m|
       <= 2 max A; the maximum m itself is a common shift of all exponents and cancels in the softmax
                                                                                        eps_j = ds_j + 6 u max_j A_j
     - exp2 to one ulp: 2 u       => every exponential is c pi_j (1 + theta_j), |theta_j| <= E = expm1(max eps)(1 + 2 u) + 2 u
     - the float32 sum of the T exponentials in any order, and the division by it:      SIGMA = (T + 2) u
     - P V accumulated by fma over the T keys, any order:                               T u N
     - beyond 4096 keys, per further chunk one more exp2 of a rounded argument and one product on both sums:
                                                                                        R = (chunks - 1)(3 u + 6 u max A)
     - one fp16 rounding of the output.
   pre   = SLACK ((E + T u + R + 2 u) N + (E + SIGMA + R) |want|)
   bound = pre + h (|want| + pre) + 2^-25

 * Uniform.  q = 0: every score is 0, every exponential exactly 1, the float32 sum exactly T, P V the exact integer sum
   of the values (< 2^24): the output is fl16(fl(sum / T)), within (2^-11 + 2^-21) |mean| of the mean over exactly the
   image's T keys, `vit_bounds.uniform_case`'s bound.
 * Selector.  Keys are +-1 in 64 dimensions and q[h] = 32 x one of them, u_h: after the exact scaling by 1/8 the key
   equal to u_h scores 4 * 64 = 256 and any other 4 * dot <= 256 - 4 gap.  `probe_selector_case` raises unless gap >= 16:
   every other key is then >= 64 below the maximum (the issue asks for more than 60), its exponential <= e^-64 = 1.6e-28,
   the float32 sum of the exponentials 1 + T * 1.6e-28 = 1.0 and the accumulator the value row plus at most T * 2048 *
   1.6e-28 < 1e-21, which changes no float32 integer and rounds to zero in fp16 beside a zero: the kernel must EQUAL the
   value row at the planted position.
"""

from __future__ import annotations

import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

import vit_bounds as vb  # noqa: E402
from clip_oracle import _rounding  # noqa: E402

LN_EPS = 1e-6
GELU_TANH_C = math.sqrt(2.0 / math.pi)
GELU_TANH_A = 0.044715
PROBE_CHUNK = 4096


# ------------------------------------------------------------------------------------------------------ tanh GELU
def _gelu_tanh_arg(v: Tensor) -> Tensor:
    return GELU_TANH_C * (v + GELU_TANH_A * v * v * v)


def gelu_tanh_f64(v: Tensor) -> Tensor:
    v = v.double()
    return v * torch.sigmoid(2.0 * _gelu_tanh_arg(v))


def gelu_tanh_bound(v: Tensor, *, out_f16: bool, residual: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """(want, bound) for gelu_tanh(v) (+ residual) out of the epilogue, `v` the exact pre-activation (module docstring)."""
    v = v.double()
    arg = _gelu_tanh_arg(v)
    s = torch.sigmoid(2.0 * arg)
    one_minus_s = torch.sigmoid(-2.0 * arg)  # keeps its digits where s is close to 1
    want = v * s
    bound = vb.SLACK * want.abs() * vb.U * (4 + 2 * one_minus_s * (1 + 6 * arg.abs())) + (v.abs() + 1) * 2.0**-126
    if residual is not None:
        want = want + residual.double()
        bound = bound + vb.U * (want.abs() + bound)
    if out_f16:
        bound = bound + vb.H * (want.abs() + bound) + vb.TINY16
    return want, bound


def erf_is_outside(v: Tensor, *, out_f16: bool) -> int:
    """How many elements of the erf GELU of `v` lie outside the tanh form's bound (none: the test could not tell them apart)."""
    want, bound = gelu_tanh_bound(v, out_f16=out_f16)
    return int(((vb.gelu_f64(v) - want).abs() > bound).sum())


# ------------------------------------------------------------------------------------------- one-query attention
def _kv_heads(kv: Tensor, heads: int) -> tuple[Tensor, Tensor]:
    """kv [B, T, 2 D] -> k, v [B, heads, T, 64]."""
    b, t, _ = kv.shape
    k, v = (z.reshape(b, t, heads, 64).transpose(1, 2) for z in kv.split(heads * 64, dim=-1))
    return k, v


def probe_reference(kv: Tensor, q: Tensor, heads: int) -> tuple[Tensor, Tensor]:
    """(want, bound), float64 [B, D]: softmax(q k^T / 8) v per (image, head) on the fp16 operands `kv` [B, T, 2 D] and `q`
    [D], and the element-wise bound of the module docstring."""
    b, t, _ = kv.shape
    k, v = _kv_heads(kv.double(), heads)
    qh = q.double().reshape(1, heads, 1, 64)
    s = (qh * k).sum(-1) / 8.0  # [B, heads, T]
    mag = (qh.abs() * k.abs()).sum(-1) / 8.0
    top = mag.amax(-1, keepdim=True)
    eps = 64 * vb.U * mag + 6 * vb.U * top
    e = torch.expm1(eps.amax(-1)) * (1 + 2 * vb.U) + 2 * vb.U  # [B, heads]
    if float(e.max()) >= 2.0**-10 or (t + 2) * vb.U > 1e-3:
        raise ValueError(f"score errors up to {float(e.max()):.3g} over {t} keys: too large for the first-order bound")
    chunks = -(-t // PROBE_CHUNK)
    r = (chunks - 1) * (3 * vb.U + 6 * vb.U * top.squeeze(-1))
    e, r = e.unsqueeze(-1), r.unsqueeze(-1)
    pi = torch.softmax(s, dim=-1).unsqueeze(-2)  # [B, heads, 1, T]
    w = (pi @ v).squeeze(-2)  # [B, heads, 64]
    n = (pi @ v.abs()).squeeze(-2)
    pre = vb.SLACK * ((e + t * vb.U + r + 2 * vb.U) * n + (e + (t + 2) * vb.U + r) * w.abs())
    bound = pre + vb.H * (w.abs() + pre) + vb.TINY16
    return w.reshape(b, heads * 64), bound.reshape(b, heads * 64)


def probe_restated(kv: Tensor, q: Tensor, heads: int, *, drop_key: int | None = None, extra_zero_keys: int = 0) -> Tensor:
    """The kernel's arithmetic in float32 torch in another order (scores from the unscaled query divided by 8 afterwards,
    exp instead of exp2, torch's sums): fp16 [B, D].  Planted faults: `drop_key` leaves that key out, `extra_zero_keys`
    admits that many zero-filled keys (score 0, value 0) to the softmax."""
    b, t, _ = kv.shape
    k, v = (z.float() for z in _kv_heads(kv, heads))
    if drop_key is not None:
        keep = [j for j in range(t) if j != drop_key]
        k, v = k[:, :, keep], v[:, :, keep]
    if extra_zero_keys:
        pad = torch.zeros(b, heads, extra_zero_keys, 64)
        k, v = torch.cat([k, pad], dim=2), torch.cat([v, pad], dim=2)
    s = (q.float().reshape(1, heads, 1, 64) * k).sum(-1) / 8.0
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (p.unsqueeze(-2) @ v).squeeze(-2) / p.sum(-1, keepdim=True)
    return o.half().reshape(b, heads * 64)


def probe_uniform_case(b: int, t: int, heads: int, seed: int) -> dict:
    """q = 0, random keys, positive integer values: `want` [B, D] the float64 mean over exactly the image's T keys."""
    c = vb.uniform_case(b, t, heads, seed)
    d = heads * 64
    return {"kv": c["qkv"][:, :, d:].contiguous(), "q": torch.zeros(d, dtype=torch.float16), "want": c["want"][:, 0].contiguous(),
            "bound": c["bound"][:, 0].contiguous()}


def probe_positions(b: int, t: int, heads: int) -> Tensor:
    """[B, heads]: the first, the last and a middle key, a different one per image and head (while T allows)."""
    cand = [0, t - 1, t // 2]
    return torch.tensor([[cand[(i + h) % 3] for h in range(heads)] for i in range(b)])


def probe_selector_case(b: int, t: int, heads: int, seed: int) -> dict:
    """Operands on which the kernel must EQUAL a gather (module docstring): `kv` [B, T, 2 D] and `q` [D] fp16, `want` =
    the value rows at `pos` [B, heads], fp16 [B, D]."""
    g = vb.gen(seed)
    chosen = torch.randint(0, 2, (heads, 64), generator=g) * 2 - 1  # u_h
    keys = torch.randint(0, 2, (b, t, heads, 64), generator=g) * 2 - 1
    values = torch.randint(-2048, 2049, (b, t, heads, 64), generator=g)
    pos = probe_positions(b, t, heads)
    for i in range(b):
        for h in range(heads):
            keys[i, pos[i, h], h] = chosen[h]
    dots = (keys.float() * chosen.float().reshape(1, 1, heads, 64)).sum(-1)  # [B, T, heads], exact
    for i in range(b):
        for h in range(heads):
            dots[i, pos[i, h], h] = -64.0
    gap = 64 - int(dots.max()) if t > 1 else 64
    if gap < vb.MIN_GAP:
        raise ValueError(f"weak selector: a key is within {gap} of the probe's (need {vb.MIN_GAP})")
    d = heads * 64
    kv = torch.cat([keys.reshape(b, t, d), values.reshape(b, t, d)], dim=-1).half()
    want = torch.stack([torch.cat([values[i, pos[i, h], h] for h in range(heads)]) for i in range(b)]).half()
    return {"kv": kv, "q": (32 * chosen).reshape(d).half(), "want": want, "pos": pos, "gap": gap}


def probe_random_case(b: int, t: int, heads: int, scale: float, seed: int) -> tuple[Tensor, Tensor]:
    g = vb.gen(seed)
    return ((torch.randn(b, t, 2 * heads * 64, generator=g) * scale).half(),
            (torch.randn(heads * 64, generator=g) * scale * 8).half())


# ------------------------------------------------------------------------------------------------------ the towers
def interpolate_pos(pos: Tensor, grid: tuple[int, int]) -> Tensor:
    """`pos` [P, D], P = g^2 -> [h w, D]: `F.interpolate(mode="bicubic", align_corners=False)` on [D, g, g], as
    transformers resamples SigLIP's table; the native grid returns it unchanged."""
    p, d = pos.shape
    g = math.isqrt(p)
    assert g * g == p
    if grid == (g, g):
        return pos
    t = pos.reshape(1, g, g, d).permute(0, 3, 1, 2)
    t = F.interpolate(t, size=grid, mode="bicubic", align_corners=False)
    return t.permute(0, 2, 3, 1).reshape(grid[0] * grid[1], d)


def _gelu_tanh(x: Tensor) -> Tensor:
    return F.gelu(x, approximate="tanh")


def _blocks(sd: dict[str, Tensor], prefix: str, tok: Tensor, heads: int, r) -> Tensor:
    b, t, d = tok.shape
    depth = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(f"{prefix}.blocks."))
    for i in range(depth):
        p = f"{prefix}.blocks.{i}"
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"], LN_EPS)
        qkv = F.linear(r(h), r(sd[f"{p}.attn.qkv.weight"]), sd[f"{p}.attn.qkv.bias"])
        qkv = r(qkv).reshape(b, t, 3, heads, d // heads).permute(2, 0, 3, 1, 4)  # [3, B, H, T, 64]
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = torch.softmax((q @ k.transpose(-1, -2)) * (d // heads) ** -0.5, dim=-1)
        a = (r(att) @ v).transpose(1, 2).reshape(b, t, d)
        tok = tok + F.linear(r(a), r(sd[f"{p}.attn.proj.weight"]), sd[f"{p}.attn.proj.bias"])
        h = F.layer_norm(tok, (d,), sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"], LN_EPS)
        h = _gelu_tanh(F.linear(r(h), r(sd[f"{p}.mlp.fc1.weight"]), sd[f"{p}.mlp.fc1.bias"]))
        tok = tok + F.linear(r(h), r(sd[f"{p}.mlp.fc2.weight"]), sd[f"{p}.mlp.fc2.bias"])
    return tok


def siglip_image_features(sd: dict[str, Tensor], x: Tensor, *, patch: int, heads: int,
                          round_operands_fp16: bool = False) -> Tensor:
    """float32 `[B, 3, P h, P w]` -> float32 `[B, D]`, the attention-pooled embedding (not normalised).  The position table
    is resampled by plain bicubic interpolation to the input's grid.  `round_operands_fp16`: every matrix-product operand
    is rounded to fp16 first, as the kernels round theirs -- the probe's query after its float32 product, the key / value
    rows, the pooled row; the head's probabilities stay float32, as in `isc_attention_f16_probe`."""
    r = _rounding(round_operands_fp16)
    v = "visual"
    d = sd[f"{v}.pos_embed"].shape[-1]
    b = x.shape[0]
    grid = (x.shape[2] // patch, x.shape[3] // patch)
    tok = F.conv2d(r(x), r(sd[f"{v}.patch_embed.proj.weight"]), sd[f"{v}.patch_embed.proj.bias"], stride=patch)
    tok = tok.flatten(2).transpose(1, 2) + interpolate_pos(sd[f"{v}.pos_embed"][0], grid)
    tok = _blocks(sd, v, tok, heads, r)
    tok = F.layer_norm(tok, (d,), sd[f"{v}.norm.weight"], sd[f"{v}.norm.bias"], LN_EPS)
    w, bias = sd[f"{v}.head.attn.in_proj.weight"], sd[f"{v}.head.attn.in_proj.bias"]
    q = r(F.linear(sd[f"{v}.head.probe"].reshape(1, d), w[:d], bias[:d]))  # [1, D]
    kv = r(F.linear(r(tok), r(w[d:]), bias[d:]))  # [B, T, 2 D]
    t = kv.shape[1]
    k, val = (z.reshape(b, t, heads, 64).transpose(1, 2) for z in kv.split(d, dim=-1))
    s = (q.reshape(1, heads, 1, 64) * k).sum(-1) / 8.0  # [B, heads, T]
    a = (torch.softmax(s, dim=-1).unsqueeze(-2) @ val).reshape(b, d)
    y = F.linear(r(a), r(sd[f"{v}.head.attn.out_proj.weight"]), sd[f"{v}.head.attn.out_proj.bias"])
    h = F.layer_norm(y, (d,), sd[f"{v}.head.norm.weight"], sd[f"{v}.head.norm.bias"], LN_EPS)
    h = _gelu_tanh(F.linear(r(h), r(sd[f"{v}.head.mlp.fc1.weight"]), sd[f"{v}.head.mlp.fc1.bias"]))
    return y + F.linear(r(h), r(sd[f"{v}.head.mlp.fc2.weight"]), sd[f"{v}.head.mlp.fc2.bias"])


def pad_ids(ids: Tensor, context: int, pad_token_id: int) -> Tensor:
    """`ids` [Q, T] right-padded with `pad_token_id` to [Q, context]."""
    q, t = ids.shape
    return torch.cat([ids, torch.full((q, context - t), pad_token_id, dtype=ids.dtype)], dim=1)


def siglip_text_features(sd: dict[str, Tensor], ids: Tensor, *, heads: int, round_operands_fp16: bool = False) -> Tensor:
    """int64 `[Q, T]` -> float32 `[Q, D]`: bidirectional blocks without a mask, the final LayerNorm, the LAST position,
    the head with its bias (not normalised)."""
    r = _rounding(round_operands_fp16)
    t = ids.shape[1]
    d = sd["text.pos_embed"].shape[-1]
    tok = sd["text.token_embedding.weight"][ids] + sd["text.pos_embed"][:t]
    tok = _blocks(sd, "text", tok, heads, r)
    pooled = F.layer_norm(tok[:, -1], (d,), sd["text.norm.weight"], sd["text.norm.bias"], LN_EPS)
    return F.linear(r(pooled), r(sd["text.head.weight"]), sd["text.head.bias"])


def probability(cos: Tensor, sd: dict[str, Tensor]) -> Tensor:
    """sigmoid(exp(logit_scale) cos + logit_bias) in float64."""
    return torch.sigmoid(math.exp(float(sd["logit_scale"])) * cos.double() + float(sd["logit_bias"]))


# ------------------------------------------------------------------------ the model-level cases of the GPU tests
# (preset, image shape, grid mode, max_patches, tokens): every image size of both widths on its native grid -- 196 tokens
# (the one-shot attention), 256, 576 and 1024 (the streaming attention) --, and a 4 x 6 aspect grid (24 tokens, resampled
# position table) on a "-siglip2" name, whose tower is the same.  The images already have the grid's size, so
# preprocessing is the normalisation alone.
IMAGE_CASES = [("ViT-B/16", (224, 224), "fixed", None, 196), ("ViT-B/16@256", (256, 256), "fixed", None, 256),
               ("ViT-B/16@384", (384, 384), "fixed", None, 576), ("ViT-B/16@512", (512, 512), "fixed", None, 1024),
               ("ViT-L/16@256", (256, 256), "fixed", None, 256), ("ViT-L/16@384-siglip2", (384, 384), "fixed", None, 576),
               ("ViT-B/16-siglip2", (64, 96), "aspect", 24, 24)]
MODEL_DEPTH = 2
MODEL_BATCH = 2
TEXT_QUERIES = 8
TEST_VOCAB = 1000  # the presets' 32000 / 256000 rows are a table of up to 1 GB nothing here needs


def preprocess_reference(images: Tensor) -> Tensor:
    """SigLIP's fixed normalisation (mean = std = 0.5 of 255) of uint8 images that already have the input size, float32."""
    return (images.float() - 127.5) / 127.5


def shallow(preset: str):
    """(config at MODEL_DEPTH layers a tower and TEST_VOCAB ids, seeded state dict with random biases and LayerNorm
    affines); the logit scale and bias are set so that the probabilities of random pairs spread over (0, 1)."""
    import dataclasses

    from imagescry_amd import siglip

    cfg = siglip.shallow(siglip.PRESETS[preset], MODEL_DEPTH)
    cfg = siglip.SigLIPConfig(cfg.vision, dataclasses.replace(cfg.text, vocab=TEST_VOCAB))
    sd = siglip.make_state_dict(cfg, seed=len(preset) + cfg.embed_dim, randomize_affine=True)
    sd["logit_scale"], sd["logit_bias"] = torch.tensor([math.log(40.0)]), torch.tensor([-1.5])
    return cfg, sd
