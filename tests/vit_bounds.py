"""References and derived bounds for the fp16 transformer kernels (isc_gemm_f16, isc_attention_f16, isc_layernorm): a
helper like matmul_bound.py, not a conftest.  Nothing here is fitted to a GPU result: every bound is a sum of named
terms, and every operand builder is shared by the GPU tests (tests/test_gpu_vit_exact.py) and the CPU checks of these
references (tests/test_vit_bounds_host.py).

Notation: u = 2^-24 is the float32 unit roundoff, h = 2^-11 the fp16 one; a float32 operation has relative error <= u,
a hardware transcendental documented to one ulp has 2 u; rounding a real y to fp16 moves it by at most h |y| + 2^-25
(2^-25: half the smallest fp16 subnormal, the absolute term wherever y is below 2^-14).  A float32 sum of n terms in
ANY order has relative error <= gamma_n = n u / (1 - n u) on the sum of magnitudes; with n u <= 1e-3 that is within
1.001 n u, and every bound below carries a factor SLACK = 1.01 on its first-order terms for such second-order
products (the functions raise where a first-order quantity is too large for that).

GEMM, exact integers (`gemm_case`).  fp16 operands that are integers (times a power-of-two quantum) and float32 integer
bias / residual: matmul_bound.assert_exact_range proves that no partial sum can round, so float32 output must EQUAL
the float64 product and fp16 output that product rounded ONCE (`round_once_f16`, which also asserts |want| < 65504).

GELU epilogue (`gelu_f64`, `gelu_bound`).  With quanta 2^-2 / 2^-3 the pre-activation v (accumulator + bias) is exact,
so the only error is the epilogue's.  gelu_fast / gs_gelu compute, in float32,

    x = |v| c            c = fl(1 / sqrt 2)                rel. error of x: u (product) + u (constant)   = 2 u
    t = rcp(fma(p, x, 1))                                  u + u of its own; the constant p (u) and x (2 u) reach t
                                                           through p x t = p x / (1 + p x) < 1: rel. error <= 5 u
    poly = Horner, 4 fma                                   every intermediate is <= 1.5 in magnitude on t in [0, 1]
                                                           (the coefficients alternate): roundings <= 4 * 1.5 u = 6 u;
                                                           the five rounded coefficients, sum |a_i| u = 4.5 u;
                                                           |d poly / d t| <= 1.5 + (1.5 + (1.46 + 1.07)) = 5.53, times
                                                           the 5 u t of t: 27.7 u                         <= 38.2 u
    P = poly t                                             38.2 u t + |poly| 5 u t + u P                  <= 46.7 u
    X = __expf(-x x) = exp2(-x x log2 e)                   argument y = x^2 log2(e): 2 * 2 u + u (square) + u (product)
                                                           + u (constant) = 7 u relative; |dX| <= y e^-y 7 u <= 2.6 u,
                                                           plus exp2 to one ulp, 2 u X                    <= 4.6 u
    E = P X                                                46.7 u + 4.6 u + u (both factors <= 1)         <= 52.3 u
    e = 1 - E  ~ erf(|v| / sqrt 2)                         + u, + the polynomial's documented 1.5e-7
    out = 0.5 v + (0.5 |v|) e                              the halvings are exact; product u (0.5 |v|), sum u |v|

    |out - gelu(v)| <= |v| (0.5 (1.5e-7 + 53.3 u) + 1.5 u) = |v| (0.75e-7 + 28.15 u)  -> GELU_F32 = 0.75e-7 + 29 u

a float32 residual added afterwards is one more rounding, u (|want| + bound); an fp16 output one fp16 rounding,
h (|want| + bound) + 2^-25.

Attention.  Selector and uniform operands make the kernel's result exactly computable (`selector_case`,
`uniform_case`); `attention_reference` gives the float64 softmax product and an element-wise bound for real operands.

 * Selector.  Keys are +-1 in 64 dimensions, query i is 16 x key pi(i): after the kernel's exact scaling by 1/8 the
   chosen key scores 2 * 64 = 128 and any other 2 * dot <= 128 - 2 gap, gap = 64 - (largest dot product between
   distinct keys) -- all exact small integers in float32.  `key_gap` computes the gap and `selector_case` raises unless
   it is >= 16: every other key is then >= 32 below the maximum, its exponential is <= e^-32 = 1.3e-14 < 2^-25 and
   rounds to ZERO in fp16, and the float32 sum of the exponentials is 1 + 223 * 1.3e-14 = 1.0.  The chosen key's exponent
   is fma(s, L, -fl(m L)) with s = m: 0 where m L is exact (m = 128, a power of two), otherwise |m L| u <= 2^-16 in
   magnitude, so its exponential is within 2^-16 of 1 and rounds to 1.0 in fp16.  P V is then 1.0 x the value row,
   exact; times 1 / sum = 1 (1 +- 2^-15) it moves by <= 2048 * 2^-15 = 1/16, less than half the spacing (1) of fp16
   integers up to 2048: the output rounds back to the value row.  The kernel must EQUAL `values[pi]`.
   `masked=True` is the same with +-1 in dimensions 0..62 only, k[63] = 1 for every key and q[63] = -1328 (-166 after
   scaling, an fp16 integer): the chosen key scores 2 * 63 - 166 = -40 and every other real key >= 32 lower, but a
   zero-filled padded key that escapes the mask scores 0, takes all the weight and returns a row of zeros.
 * Uniform.  q = 0: every score is 0, every exponential exactly 1, the float32 sum exactly T, P V the exact integer
   sum of the values (< 2^24): the output is fl16(sum * fl(1 / T)), within (2^-11 + 2^-21) |mean| of the mean over
   exactly T keys -- one fp16 rounding plus the reciprocal and the product in float32 (2^-21 = 8 u covers a
   reciprocal to one ulp, the product and their cross terms).  One padded key in the sum changes the divisor by 1 / T.
 * Real operands (`attention_reference`).  With s_j = q . k_j / 8, A_j = |q| . |k_j| / 8, pi = softmax(s),
   want = sum_j pi_j v_j and N = sum_j pi_j |v_j| (all float64, per output element), the kernel documents:
     - q is scaled by 1/8 in fp16: exact unless the result is subnormal, then <= 2^-25 per element
                                                                            |ds_j| <= 2^-25 sum_d |k_jd|
     - scores are a float32 sum of 64 exact products (any order):           |ds_j| <= 64 * 2 u A_j
     - the exponent is one fma on (s, fl(log2 e), fl(m fl(log2 e))): the constant's rounding u |s_j|, the product's
       u |m| and the fma's u (|s_j| + |m|), together <= 4 u max_j A_j; a common shift of all exponents cancels in the
       softmax, so only these per-key differences count
     - exp2 to one float32 ulp: 2 u
       => every exponential is c pi_j (1 + theta_j), |theta_j| <= E = expm1(max_j eps_j) (1 + 2 u) + 2 u,
          eps_j = ds_j + 4 u max A
     - the float32 sum over the unrounded exponentials (<= 224 of them and two cross-lane steps), and 1 / sum:
                                                                            SIGMA = 226 * 2 u
     - probabilities rounded to fp16: h each, or 2^-25 absolute where they are subnormal; the largest exponential is
       1 (1 - E), so after normalisation the absolute part is <= 2^-25 sum_j |v_j|
     - P V accumulated in float32 over <= 224 exact products:               224 * 2 u N
     - the product with 1 / sum: u; then one fp16 rounding of the output.
   pre   = SLACK ((E + h + 224 * 2 u + 3 u) N + (E + SIGMA) |want| + 2^-25 sum_j |v_j|)
   bound = pre + h (|want| + pre) + 2^-25

LayerNorm (`layernorm_reference`).  y = (x - mu) r g + b, r = 1 / sqrt(var + eps), float64; the kernel (two passes,
float32, any summation order) gives
     mu^  = fl(sum x) / D:         |mu^ - mu| <= dmu = SLACK (D + 1) u mean|x|
     d^_i = fl(x_i - mu^):         |d^_i - d_i| <= dmu + u |d_i|             (d_i = x_i - mu)
     var^ = fl(sum d^_i^2) / D = (var + (mu^ - mu)^2) (1 + theta),  |theta| <= (D + 4) u     (the identity
            sum (x_i - mu^)^2 = sum (x_i - mu)^2 + D (mu^ - mu)^2 is exact; the roundings are two on d^, one on the
            square, D - 1 additions, one division)
     r^   = r (1 + rho),           |rho| <= SLACK (theta / 2 + (dmu r)^2 / 2) + 3 u   (adding eps, sqrt, reciprocal;
            1 - 1 / sqrt(1 + a) <= a / 2 for every a >= 0, so this holds for constant rows too, where dmu r is not small)
     y^   = fl(fl(fl(d^ r^) g) + b)
   bound = SLACK |g| r ((dmu + u |d|) (1 + rho) + |d| rho) + 4 u (|g| |d| r + |b|)
   and h (|y| + bound) + 2^-25 more for an fp16 output.  A one-pass variance (E[x^2] - mu^2) loses var / mu^2 of its
   digits instead and is what the rows with the mean at 32 standard deviations are for.  Every other family has a
   variance of about 1 or more, or exactly 0, where eps = 1e-6, 1e-5 or 0 move the result by a few u or not at all; the
   rows of `small` (1e-3 * randn, variance about 1e-6) are what shows that a kernel honours its eps argument
   (tests/test_vit_token_bounds_host.py: the restatement with another eps leaves the bound on every element).
"""

from __future__ import annotations

import math
import sys
from pathlib import Path

import torch
from torch import Tensor

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402

U = 2.0**-24
H = 2.0**-11
TINY16 = 2.0**-25
SLACK = 1.01
ERF_POLY = 1.5e-7
GELU_F32 = 0.5 * ERF_POLY + 29 * U
SIGMA = 226 * 2 * U
MIN_GAP = 16
F16_MAX = 65504.0


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the packed layout
def pack_padded(x: Tensor, fill: float) -> Tensor:
    """`x` [R, C] in the packed layout (tiles of 256 rows, K steps of 64 columns, [tile][K step][row][64], flat) with
    the padding rows of the last tile holding `fill` instead of zeros."""
    r, c = x.shape
    assert c % 64 == 0, c
    tiles = (r + 255) // 256
    padded = torch.full((tiles * 256, c), fill, dtype=x.dtype)
    padded[:r] = x
    return padded.view(tiles, 256, c // 64, 64).permute(0, 2, 1, 3).contiguous().view(-1)


def unpack_all(flat: Tensor, rows: int, cols: int) -> Tensor:
    """The inverse: EVERY row of the tiles that hold `rows` rows, padding rows included ([tiles * 256, cols])."""
    tiles = (rows + 255) // 256
    return flat.view(tiles, cols // 64, 256, 64).permute(0, 2, 1, 3).reshape(tiles * 256, cols).contiguous()


# ---------------------------------------------------------------------------------------------------------- GEMM
def gemm_case(m: int, k: int, n: int, seed: int, *, lo: int = -4, hi: int = 4, a_quantum: float = 1.0,
              w_quantum: float = 1.0, bias_top: int = 3000, res_top: int = 30000) -> dict:
    """Exact operands: `a` [M, K], `w` [N, K] fp16 integers in lo..hi times their quanta, float32 `bias` [N] and
    `res` [M, N], integers up to +-bias_top / +-res_top times q = a_quantum * w_quantum; the float64 products without
    (`want`) and with (`want_res`) the residual; the exact range is asserted for both."""
    g = gen(seed)
    q = a_quantum * w_quantum
    a = mb.int_tensor((m, k), lo, hi, g) * a_quantum
    w = mb.int_tensor((n, k), lo, hi, g) * w_quantum
    bias = mb.int_tensor((n,), -bias_top, bias_top, g) * q
    res = mb.int_tensor((m, n), -res_top, res_top, g) * q
    mb.assert_exact_range(a, w, bias, res, a_quantum=a_quantum, w_quantum=w_quantum)  # covers the case without residual
    want = mb.product_f64(a, w, bias)
    a16, w16 = a.half(), w.half()
    assert torch.equal(a16.float(), a) and torch.equal(w16.float(), w)
    return {"a": a16, "w": w16, "bias": bias, "res": res, "want": want, "want_res": want + res.double()}


def round_once_f16(want: Tensor) -> Tensor:
    """`want` (float64, exactly representable in float32) rounded once to fp16; |want| < 65504 is asserted."""
    top = float(want.abs().max())
    assert top < F16_MAX, f"|want| reaches {top}: outside fp16"
    w32 = want.float()
    assert torch.equal(w32.double(), want), "the reference is not a float32 number: it would be rounded twice"
    return w32.half()


def gelu_f64(v: Tensor) -> Tensor:
    """erf GELU in float64, through erfc so that the negative tail keeps its digits."""
    v = v.double()
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))


def gelu_bound(v: Tensor, *, out_f16: bool, residual: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """(want, bound) for gelu(v) (+ residual) out of the epilogue, `v` the exact pre-activation (module docstring)."""
    v = v.double()
    want = gelu_f64(v)
    bound = v.abs() * GELU_F32
    if residual is not None:
        want = want + residual.double()
        bound = bound + U * (want.abs() + bound)
    if out_f16:
        bound = bound + H * (want.abs() + bound) + TINY16
    return want, bound


def gelu_restated_f32(v: Tensor, *, tanh: bool = False) -> Tensor:
    """GELU in float32 torch in another order than the kernel's (library erf on v / sqrt 2, the 0.5 last); `tanh`: the
    tanh approximation, the planted fault."""
    v = v.float()
    if tanh:
        return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))
    return (v + v * torch.erf(v * 0.7071067811865476)) * 0.5


def gelu_polynomial_f32(v: Tensor) -> Tensor:
    """The Abramowitz & Stegun 7.1.26 form the kernels use, restated in float32 torch (separate multiplications and
    additions instead of fma, a division instead of the reciprocal, exp instead of exp2)."""
    v = v.float()
    x = v.abs() * 0.7071067811865476
    t = 1.0 / (1.0 + 0.3275911 * x)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    e = 1.0 - poly * torch.exp(-(x * x))
    return 0.5 * (v + v.abs() * e)


# ----------------------------------------------------------------------------------------------------- attention
def _split_heads(qkv: Tensor, heads: int) -> tuple[Tensor, Tensor, Tensor]:
    """qkv [B, T, 3 D] -> q, k, v [B, heads, T, 64]."""
    b, t, _ = qkv.shape
    d = heads * 64
    q, k, v = (z.reshape(b, t, heads, 64).transpose(1, 2) for z in qkv.split(d, dim=-1))
    return q, k, v


def key_gap(keys: Tensor) -> int:
    """`keys` [B, T, heads, dims] of +-1: dims - (the largest dot product between two distinct keys of one (image,
    head)).  Two equal keys give 0."""
    b, t, heads, dims = keys.shape
    if t == 1:
        return dims
    k = keys.float().transpose(1, 2)  # [B, heads, T, dims]
    dots = k @ k.transpose(-1, -2)  # exact: |dot| <= 64
    dots.diagonal(dim1=-2, dim2=-1).fill_(-float(dims))
    return dims - int(dots.max())


def selector_keys_to_case(keys: Tensor, values: Tensor, perm: Tensor, *, masked: bool) -> dict:
    """Assemble a selector case from +-1 `keys` [B, T, heads, 64], integer `values` and the permutation; raises unless
    the gap is at least MIN_GAP."""
    b, t, heads, _ = keys.shape
    dims = 63 if masked else 64
    k = keys.clone().float()
    if masked:
        k[..., 63] = 1.0
    gap = key_gap(k[..., :dims])
    if gap < MIN_GAP:
        raise ValueError(f"weak selector: two keys of one head are within {gap} of each other (need {MIN_GAP})")
    q = 16.0 * k[:, perm]
    if masked:
        q[..., 63] = -1328.0
    qkv = torch.cat([z.reshape(b, t, heads * 64) for z in (q, k, values.float())], dim=-1).half()
    want = values[:, perm].reshape(b, t, heads * 64).half()
    return {"qkv": qkv, "want": want, "perm": perm, "gap": gap}


def selector_case(b: int, t: int, heads: int, seed: int, *, masked: bool = False) -> dict:
    """Operands on which the attention kernel must EQUAL a gather (module docstring): `qkv` [B, T, 3 D] fp16 and
    `want` = values[:, perm] [B, T, D] fp16."""
    g = gen(seed)
    keys = torch.randint(0, 2, (b, t, heads, 64), generator=g) * 2 - 1
    values = torch.randint(-2048, 2049, (b, t, heads, 64), generator=g)
    perm = torch.randperm(t, generator=g)
    if t > 1:  # pi(0) = T - 1 and pi(T - 1) = 0, the rest stays a permutation
        rest = perm[(perm != 0) & (perm != t - 1)]
        perm = torch.cat([torch.tensor([t - 1]), rest, torch.tensor([0])])
    assert sorted(perm.tolist()) == list(range(t))
    return selector_keys_to_case(keys, values, perm, masked=masked)


def uniform_case(b: int, t: int, heads: int, seed: int) -> dict:
    """q = 0, random keys, positive integer values: `want` the float64 mean over exactly T keys, `bound` =
    (2^-11 + 2^-21) |mean|."""
    g = gen(seed)
    d = heads * 64
    k = torch.randn(b, t, d, generator=g)
    v = torch.randint(1, 2049, (b, t, d), generator=g).float()
    qkv = torch.cat([torch.zeros(b, t, d), k, v], dim=-1).half()
    mean = v.double().mean(dim=1, keepdim=True).expand(b, t, d).contiguous()
    return {"qkv": qkv, "want": mean, "bound": (H + 2.0**-21) * mean.abs()}


def random_case(b: int, t: int, heads: int, scale: float, seed: int) -> Tensor:
    return (torch.randn(b, t, 3 * heads * 64, generator=gen(seed)) * scale).half()


def attention_reference(qkv: Tensor, heads: int, *, chunk: int = 16) -> tuple[Tensor, Tensor]:
    """(want, bound), float64 [B, T, D]: the softmax product of the fp16 operands and the element-wise bound of the
    module docstring."""
    b, t, _ = qkv.shape
    d = heads * 64
    want = torch.empty(b, t, d, dtype=torch.float64)
    bound = torch.empty(b, t, d, dtype=torch.float64)
    for i in range(0, b, chunk):
        q, k, v = _split_heads(qkv[i : i + chunk].double(), heads)
        s = q @ k.transpose(-1, -2) / 8.0
        mag = q.abs() @ k.abs().transpose(-1, -2) / 8.0
        ds = 64 * 2 * U * mag + TINY16 * k.abs().sum(-1).unsqueeze(-2)
        eps = ds + 4 * U * mag.amax(-1, keepdim=True)
        e = torch.expm1(eps.amax(-1)) * (1 + 2 * U) + 2 * U  # [c, heads, T]
        if float(e.max()) >= 2.0**-10:
            raise ValueError(f"score errors up to {float(e.max()):.3g}: too large for the first-order bound")
        e = e.unsqueeze(-1)
        pi = torch.softmax(s, dim=-1)
        w = pi @ v
        n = pi @ v.abs()
        vsum = v.abs().sum(-2, keepdim=True)
        pre = SLACK * ((e + H + 224 * 2 * U + 3 * U) * n + (e + SIGMA) * w.abs() + TINY16 * vsum)
        bd = pre + H * (w.abs() + pre) + TINY16
        c = w.shape[0]
        want[i : i + chunk] = w.transpose(1, 2).reshape(c, t, d)
        bound[i : i + chunk] = bd.transpose(1, 2).reshape(c, t, d)
    return want, bound


def attention_restated(qkv: Tensor, heads: int, *, drop_largest: bool = False, extra_zero_keys: int = 0,
                       swap_values: int | None = None) -> Tensor:
    """The kernel's arithmetic in float32 / fp16 torch in another order: scores from the UNscaled queries divided by 8
    afterwards, exp(s - max) instead of exp2 of an fma, torch's sums, probabilities rounded to fp16, the product in
    float32, a division by the sum.  Returns fp16 [B, T, D].  Planted faults: `drop_largest` zeroes every query's
    largest probability; `extra_zero_keys` admits that many zero-filled padded keys (score 0) to the softmax;
    `swap_values` = j exchanges value rows j and j + 1."""
    b, t, _ = qkv.shape
    q, k, v = (z.float() for z in _split_heads(qkv, heads))
    if swap_values is not None:
        v = v.clone()
        v[:, :, [swap_values, swap_values + 1]] = v[:, :, [swap_values + 1, swap_values]]
    if extra_zero_keys:
        pad = torch.zeros(b, heads, extra_zero_keys, 64)
        k, v = torch.cat([k, pad], dim=2), torch.cat([v, pad], dim=2)
    s = (q @ k.transpose(-1, -2)) / 8.0
    e = torch.exp(s - s.amax(-1, keepdim=True))
    if drop_largest:
        e = e.masked_fill(e == e.amax(-1, keepdim=True), 0.0)
    total = e.sum(-1, keepdim=True)
    o = (e.half().float() @ v) / total
    return o.half().transpose(1, 2).reshape(b, t, heads * 64)


# ----------------------------------------------------------------------------------------------------- LayerNorm
LN_EPS = 1e-6
LN_FAMILIES = ("randn", "far-mean", "constant", "spike", "small")


def layernorm_case(rows: int, d: int, family: str, seed: int) -> dict:
    """`x` [rows, D], `gamma`, `beta` float32 of one of the row families of the issue."""
    g = gen(seed)
    if family == "randn":
        x = torch.randn(rows, d, generator=g) * 3 + 1.5
    elif family == "far-mean":  # the mean at 32 standard deviations
        x = 32 + torch.randn(rows, d, generator=g)
    elif family == "constant":
        x = (torch.randn(rows, 1, generator=g) * 2 + 0.7).expand(rows, d).contiguous()
    elif family == "spike":
        x = torch.randn(rows, d, generator=g)
        x[torch.arange(rows), torch.randint(0, d, (rows,), generator=g)] = 1e4
    elif family == "small":  # the variance about equal to eps: the rows on which a wrong or ignored eps shows
        x = torch.randn(rows, d, generator=g) * 1e-3
    else:
        raise ValueError(family)
    return {"x": x, "gamma": torch.rand(d, generator=g) + 0.5, "beta": torch.randn(d, generator=g)}


def layernorm_reference(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = LN_EPS, *,
                        out_f16: bool = False) -> tuple[Tensor, Tensor]:
    """(want, bound), float64 [rows, D] (module docstring)."""
    x, g, b = x.double(), gamma.double(), beta.double()
    d = x.shape[1]
    eps = float(torch.tensor(eps, dtype=torch.float32))  # the float32 the kernel receives
    mu = x.mean(dim=1, keepdim=True)
    dev = x - mu
    r = 1.0 / torch.sqrt((dev * dev).mean(dim=1, keepdim=True) + eps)
    want = dev * r * g + b
    if (d + 4) * U > 1e-3:
        raise ValueError(f"D = {d} is too long for the first-order bound")
    dmu = SLACK * (d + 1) * U * x.abs().mean(dim=1, keepdim=True)
    rho = SLACK * ((d + 4) * U / 2 + (dmu * r) ** 2 / 2) + 3 * U
    bound = SLACK * g.abs() * r * ((dmu + U * dev.abs()) * (1 + rho) + dev.abs() * rho) + 4 * U * (
        g.abs() * dev.abs() * r + b.abs())
    if out_f16:
        bound = bound + H * (want.abs() + bound) + TINY16
    return want, bound


def layernorm_restated(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = LN_EPS, *,
                       skip_vector: tuple[int, int] | None = None, neighbour_mean: bool = False) -> Tensor:
    """LayerNorm in float32 torch in another order than the kernel's (torch's own reductions, a division by the
    standard deviation).  Planted faults: `skip_vector` = (row, c) leaves the 16-byte vector x[row, 4 c : 4 c + 4] out of
    that row's statistics; `neighbour_mean` subtracts the mean of row i + 1 (cyclically) from row i."""
    x = x.float()
    d = x.shape[1]
    xs = x
    if skip_vector is not None:
        row, c = skip_vector
        xs = x.clone()
        xs[row, 4 * c : 4 * c + 4] = 0.0
    mean = xs.sum(dim=1, keepdim=True) / d
    if neighbour_mean:
        mean = mean.roll(-1, dims=0)
    dev = x - mean
    sq = dev * dev
    if skip_vector is not None:
        sq = sq.clone()
        sq[row, 4 * c : 4 * c + 4] = 0.0
    var = sq.sum(dim=1, keepdim=True) / d
    return dev / torch.sqrt(var + eps) * gamma.float() + beta.float()
