"""References and derived bounds for the streaming attention kernel (isc_attention_f16_stream): a helper next to
vit_bounds.py, whose notation (u, h, SLACK, 2^-25), operand builders and packed-layout helpers it uses.  Nothing here is
fitted to a GPU result.

The kernel walks the keys of a head in C = ceil(T / key_chunk) chunks and keeps, per query and in float32, a running
maximum m and per-lane partial sums l, and the accumulator O:

    m' = max(m, chunk maximum)      alpha = exp2((m - m') L^)             L^ = fl(log2 e); chunk 0 has no rescale
    p_j = exp2(fma(s_j, L^, -fl(m' L^)))                                  as in isc_attention_f16, with the running m'
    l = l alpha + sum p_j           O = O alpha + sum fl16(p_j) v_j       the SAME alpha value in both

`stream_reference` is `vit_bounds.attention_reference` with the terms that depend on the sequence length redone:

 * The weights.  O / l is EXACTLY a weighted mean sum_j w_j v_j / sum_j w_j (before its roundings) with
   w_j = p_j prod(alpha of every later chunk): alpha is one value on both sides, so nothing of it is left but what it
   does to w_j.  In exact arithmetic the exponents telescope, w_j = exp(s_j - m_final).  In float32 a chunk's alpha has
   the argument fl(fl(m - m') L^): a subtraction, a product and the rounded constant, relative error 3 u on |m - m'|
   (natural units; log2 e ln 2 = 1).  m only grows, so over all chunks sum |m - m'| = m_final - m_0 <= 2 max_j A_j
   (A_j = |q| . |k_j| / 8 bounds every score): 6 u max A in the exponent of w_j, plus exp2 to one ulp per rescale,
   2 u (C - 1).  Both are added to eps_j, from which E = expm1(max eps)(1 + 2 u) + 2 u follows as before.  (The scores
   themselves and the fma exponent are unchanged: 64 * 2 u A_j + 2^-25 sum_d |k_jd| and 4 u max A.)
 * The sum: T exponentials in float32 in any order (the kernel adds per lane and joins the lanes at the end: two
   cross-lane steps) and C products with alpha, u each:                  SIGMA(T, C) = (T + 2 + C) * 2 u
   in the convention of vit_bounds.SIGMA = (224 + 2) * 2 u (2 u a term, which also covers the reciprocal).
 * P V: T exact products accumulated in float32 plus C multiplications of the accumulator by alpha:
                                                                          (T + C) * 2 u N
 * Probabilities rounded to fp16: h each, as before.  A subnormal one is off by <= 2^-25 relative to the running
   maximum of ITS chunk; every later alpha is <= 1 (exp2 of a number <= 0), so relative to the final maximum it is no
   larger, and the largest weight is 1 (1 - E): the absolute part stays 2^-25 sum_j |v_j|.
 * The product with 1 / sum and the fp16 rounding of the output: as before.

    pre   = SLACK ((E + h + (T + C) 2 u + 3 u) N + (E + SIGMA(T, C)) |want| + 2^-25 sum_j |v_j|)
    bound = pre + h (|want| + pre) + 2^-25

(T + C) 2 u stays below 1e-3 up to T = 8000, which `stream_reference` checks with the first-order check on E.

Selector (`stream_selector_case`).  vit_bounds' argument that the kernel must EQUAL the gather counts at most 224 keys
and one softmax.  Streamed, the chunks BEFORE the chosen key's see a smaller maximum: there a key's probability may be
1 and O collects up to T * 2048 before the chosen key arrives.  That chunk's alpha is <= exp(-2 gap) (every other key
scores >= 2 gap below the chosen one), so what is left of it is below T * 2048 * exp(-2 gap).  Required:

    T * 2048 * exp(-2 gap) < 2^-26

Then the residue rounds away when the chosen value row (integers, float32 spacing >= 2^-23 from 1 upwards) is added,
a chosen value of 0 gives an output below 2^-26, which is 0 in fp16 (half the smallest subnormal is 2^-25), and the
sum is 1 + T exp(-2 gap) = 1.0 in float32.  Keys behind the chosen one have probabilities <= exp(-2 gap) < 2^-25: zero
in fp16.  The chosen key's own exponent is as in vit_bounds (within 2^-16 of 0).  The case builder asserts the
condition for the case's own gap.

Rising and falling (`rising_case`).  q_i = a_i d and k_j = c_j d with d a +-1 direction, a_i in [0.5, 1] and c_j = j /
(T - 1) (rising) or 1 - j / (T - 1) (falling), all fp16: s_ij = 8 a_i c_j exactly monotone in j.  Rising: the maximum
of every chunk is above the one before, every chunk rescales, and the weights span e^4 .. e^8.  Falling: key 0 holds
the maximum, every alpha is exp2(0) = 1.  |s| <= 8, far inside the first-order check.

`stream_restated` is the online softmax in float32 / fp16 torch in another order (unscaled queries divided by 8
afterwards, exp instead of exp2, torch's sums, one alpha per chunk applied to whole tensors) with planted faults.
"""

from __future__ import annotations

import math
import sys
from pathlib import Path

import torch
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

import vit_bounds as vb  # noqa: E402

U, H, TINY16, SLACK = vb.U, vb.H, vb.TINY16, vb.SLACK
RESIDUE = 2.0**-26


def geometry() -> tuple[int, int]:
    """(query_block, key_chunk) of the built library; needs no device."""
    import ctypes

    from imagescry_amd import _lib, build

    if not _lib.LIB_PATH.exists():
        build.build(verbose=False)
    qb, kc = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().isc_attention_stream_geometry(ctypes.byref(qb), ctypes.byref(kc)), "isc_attention_stream_geometry")
    assert qb.value > 0 and kc.value > 0 and kc.value % 32 == 0, (qb.value, kc.value)
    return qb.value, kc.value


def stream_lengths(qb: int, kc: int) -> list[int]:
    """The sequence lengths of the GPU test: both sides of the old kernel's limit, of one and two key chunks and of one
    and two query blocks, and three long grids (24 x 24, 28 x 28, 32 x 32, each plus the class token)."""
    return sorted({1, 17, 224, 225, kc - 1, kc, kc + 1, 2 * kc - 1, 2 * kc, 2 * kc + 1, qb + 1, 2 * qb + 1, 577, 785, 1025})


def bound_lengths(kc: int) -> list[int]:
    return sorted({225, 2 * kc + 1, 785, 1025})


def seam_lengths(kc: int) -> list[int]:
    return sorted({2 * kc + 1, 785})


def chunks_of(t: int, key_chunk: int) -> int:
    return -(-t // key_chunk)


def stream_reference(qkv: Tensor, heads: int, key_chunk: int, *, chunk: int = 4) -> tuple[Tensor, Tensor]:
    """(want, bound), float64 [B, T, D]: the softmax product of the fp16 operands and the element-wise bound of the
    module docstring for a kernel that streams the keys in chunks of `key_chunk`."""
    b, t, _ = qkv.shape
    d = heads * 64
    c_n = chunks_of(t, key_chunk)
    if (t + c_n + 2) * 2 * U > 1e-3:
        raise ValueError(f"T = {t} is too long for the first-order bound")
    sigma = (t + 2 + c_n) * 2 * U
    want = torch.empty(b, t, d, dtype=torch.float64)
    bound = torch.empty(b, t, d, dtype=torch.float64)
    for i in range(0, b, chunk):
        q, k, v = vb._split_heads(qkv[i : i + chunk].double(), heads)
        s = q @ k.transpose(-1, -2) / 8.0
        mag = q.abs() @ k.abs().transpose(-1, -2) / 8.0
        top = mag.amax(-1, keepdim=True)
        ds = 64 * 2 * U * mag + TINY16 * k.abs().sum(-1).unsqueeze(-2)
        eps = ds + 4 * U * top + 6 * U * top + 2 * U * (c_n - 1)
        e = torch.expm1(eps.amax(-1)) * (1 + 2 * U) + 2 * U  # [c, heads, T]
        if float(e.max()) >= 2.0**-10:
            raise ValueError(f"score errors up to {float(e.max()):.3g}: too large for the first-order bound")
        e = e.unsqueeze(-1)
        pi = torch.softmax(s, dim=-1)
        w = pi @ v
        n = pi @ v.abs()
        vsum = v.abs().sum(-2, keepdim=True)
        pre = SLACK * ((e + H + (t + c_n) * 2 * U + 3 * U) * n + (e + sigma) * w.abs() + TINY16 * vsum)
        bd = pre + H * (w.abs() + pre) + TINY16
        c = w.shape[0]
        want[i : i + chunk] = w.transpose(1, 2).reshape(c, t, d)
        bound[i : i + chunk] = bd.transpose(1, 2).reshape(c, t, d)
    return want, bound


def selector_seed(t: int, masked: bool) -> int:
    return 1000 + t + (7 if masked else 0)


def stream_selector_case(b: int, t: int, heads: int, *, masked: bool = False) -> dict:
    """`vit_bounds.selector_case` with the seed of the tests, refused unless T * 2048 * exp(-2 gap) < 2^-26 (module
    docstring)."""
    c = vb.selector_case(b, t, heads, seed=selector_seed(t, masked), masked=masked)
    residue = t * 2048.0 * math.exp(-2.0 * c["gap"])
    if not residue < RESIDUE:
        raise ValueError(f"weak selector for a streamed softmax: T = {t}, gap {c['gap']} leaves {residue:.3g} >= 2^-26")
    return c


def rising_case(b: int, t: int, heads: int, seed: int, *, falling: bool = False) -> Tensor:
    """qkv [B, T, 3 D] fp16 whose scores are exactly monotone in the key index (module docstring)."""
    g = vb.gen(seed)
    direction = (torch.randint(0, 2, (b, 1, heads, 64), generator=g) * 2 - 1).float()
    a = (torch.rand(b, t, heads, 1, generator=g) * 0.5 + 0.5).half().float()
    ramp = torch.arange(t, dtype=torch.float32) / max(t - 1, 1)
    c = ((1.0 - ramp) if falling else ramp).half().float().reshape(1, t, 1, 1)
    q, k = a * direction, (c * direction).expand(b, t, heads, 64)
    v = torch.randn(b, t, heads, 64, generator=g)
    qkv = torch.cat([z.reshape(b, t, heads * 64) for z in (q, k, v)], dim=-1).half()
    s = (a * c.reshape(1, 1, 1, t)) * 8.0  # [B, Tq, heads, Tk]
    step = s[..., 1:] - s[..., :-1]
    assert bool((step <= 0).all() if falling else (step >= 0).all())
    return qkv


def stream_restated(qkv: Tensor, heads: int, key_chunk: int, *, skip_o_rescale: int | None = None,
                    skip_l_rescale: bool = False, drop_chunk: int | None = None, extra_zero_keys: int = 0) -> Tensor:
    """The online softmax in float32 / fp16 torch, fp16 [B, T, D].  Planted faults: `skip_o_rescale` = c leaves O
    unscaled when chunk c arrives; `skip_l_rescale` never rescales the sum; `drop_chunk` = c skips that chunk;
    `extra_zero_keys` admits that many zero-filled padded keys (score 0) at the end of the last chunk."""
    b, t, _ = qkv.shape
    q, k, v = (z.float() for z in vb._split_heads(qkv, heads))
    if extra_zero_keys:
        assert t % key_chunk and extra_zero_keys <= key_chunk - t % key_chunk
        pad = torch.zeros(b, heads, extra_zero_keys, 64)
        k, v = torch.cat([k, pad], dim=2), torch.cat([v, pad], dim=2)
    m = torch.full((b, heads, t, 1), -math.inf)
    lsum = torch.zeros(b, heads, t, 1)
    o = torch.zeros(b, heads, t, 64)
    for c, k0 in enumerate(range(0, k.shape[2], key_chunk)):
        if c == drop_chunk:
            continue
        kc, vc = k[:, :, k0 : k0 + key_chunk], v[:, :, k0 : k0 + key_chunk]
        s = (q @ kc.transpose(-1, -2)) / 8.0
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)  # chunk 0: exp(-inf) = 0 on zeros
        p = torch.exp(s - mn)
        lsum = (lsum if skip_l_rescale else lsum * alpha) + p.sum(-1, keepdim=True)
        o = (o if c == skip_o_rescale else o * alpha) + p.half().float() @ vc
        m = mn
    return (o / lsum).half().transpose(1, 2).reshape(b, t, heads * 64)
