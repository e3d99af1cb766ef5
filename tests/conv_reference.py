"""What the convolution kernel tests share (a helper, not a conftest): the activation rule of the derived bound, the
GEMM operands of a convolution, and an output buffer that shows a write outside it.

Activations.  ReLU is 1-Lipschitz, so the activation is applied to `want` and the bound kept.  For SiLU, GELU and
sigmoid `want` is the float64 activation of the float64 pre-activation, and the bound is

    1.13 * (pre-activation bound) + 2^-21 * (1 + |value|)

The first term: max |silu'| = 1.0998, max |gelu'| = 1.1290, max |sigmoid'| = 0.25, all <= 1.13, so an error e of the
pre-activation moves the activation by at most 1.13 e.  The second: the float32 activation arithmetic itself, 2^-21 = 8
float32 roundoffs on a quantity of size 1 + |value| (exp and reciprocal at about 1 ulp each, two or three multiplications
and additions on top), `value` being the expected output.  With `ISC_ACT_RESIDUAL_AFTER` the residual is added to the
activation by one more float32 addition: `want` gets the residual, the pre-activation bound does not, and |value| is
|activation| + |residual|.

GEMM operands.  `gemm_operands` unfolds an NHWC input into the [M, K] matrix the implicit GEMM multiplies (pure data
movement: padding taps stay zero) and brings the weights to the same K order; tests/matmul_bound.py takes it from
there.

Guarded output.  Kernels store 16 bytes at a time and compute tiles that overhang the output; `GuardedOutput` is ONE
allocation of canary | payload | canary with the payload pre-filled with NaN.  After the call both canaries must be
untouched (compared as int32: the pattern is no number) and no payload element may still be NaN, so neither a store past
either end nor an element left unwritten -- nor a previous test's answer in recycled memory -- passes."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import Tensor

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_SIGMOID, RES_AFTER = 0, 1, 2, 3, 4, 0x100
ACT_SLACK = 2.0**-21
ACT_SLOPE = 1.13


def _activate(pre: Tensor, act: int) -> Tensor:
    if act == ACT_RELU:
        return pre.clamp_min(0.0)
    if act == ACT_GELU:
        return F.gelu(pre)  # exact erf form, float64
    if act == ACT_SILU:
        return F.silu(pre)
    if act == ACT_SIGMOID:
        return torch.sigmoid(pre)
    return pre


def expected(pre: Tensor, pre_bound: Tensor, act: int, residual_after: Tensor | None = None):
    """(want, bound) of act(pre) [+ residual_after] by the rule of the module docstring."""
    want = _activate(pre, act)
    if act in (ACT_NONE, ACT_RELU):
        assert residual_after is None
        return want, pre_bound
    size = want.abs()
    if residual_after is not None:
        size = size + residual_after.abs()
        want = want + residual_after
    return want, ACT_SLOPE * pre_bound + ACT_SLACK * (1 + size)


# ------------------------------------------------------------------------------------------------------- GEMM operands
def packed_k_rows(w_krsc: Tensor) -> Tensor:
    """[Cout, R, S, Cin] -> the packed-K rows of `isc_conv2d_nhwc` for Cin % 32 != 0: [Cout, ceil(R*S*Cin / 32) * 32],
    k = (r * S + s) * Cin + c, zero tail."""
    cout = w_krsc.shape[0]
    k = w_krsc[0].numel()
    rows = torch.zeros(cout, (k + 31) // 32 * 32, dtype=w_krsc.dtype)
    rows[:, :k] = w_krsc.reshape(cout, k)
    return rows


def gemm_operands(x_nhwc: Tensor, w_krsc: Tensor, r: int, s: int, stride: int, pad: int) -> tuple[Tensor, Tensor]:
    """`a` [B * Ho * Wo, K] and `w2` [Cout, K] (float32, K = Cin * R * S in unfold's (c, r, s) order) with
    conv(x, w) = a . w2^T.  `w_krsc` is [Cout, R, S, Cin], or the 2-D packed-K rows of it, whose zero tail is asserted."""
    b, h, w, cin = x_nhwc.shape
    cout = w_krsc.shape[0]
    k = r * s * cin
    if w_krsc.dim() == 2:
        assert w_krsc.shape[1] == (k + 31) // 32 * 32, (w_krsc.shape, k)
        assert not w_krsc[:, k:].any(), "the tail of a packed-K weight row is zero"
        w_krsc = w_krsc[:, :k].reshape(cout, r, s, cin)
    assert tuple(w_krsc.shape) == (cout, r, s, cin), (w_krsc.shape, (cout, r, s, cin))
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    if (r, s, stride, pad) == (1, 1, 1, 0):
        return x_nhwc.reshape(-1, cin), w_krsc.reshape(cout, cin)
    cols = F.unfold(x_nhwc.permute(0, 3, 1, 2), (r, s), padding=pad, stride=stride)  # [B, Cin * R * S, Ho * Wo]
    a = cols.transpose(1, 2).reshape(b * ho * wo, k).contiguous()
    return a, w_krsc.permute(0, 3, 1, 2).reshape(cout, k).contiguous()


# ------------------------------------------------------------------------------------------------------ guarded output
class GuardedOutput:
    MARGIN = 256  # floats on each side
    CANARY = 0x7FB1C4A3  # as float32 a NaN with a payload no arithmetic produces

    def __init__(self, shape: tuple[int, ...], device: torch.device) -> None:
        self.shape = tuple(shape)
        self.n = math.prod(self.shape)
        self.buf = torch.empty(self.n + 2 * self.MARGIN, dtype=torch.float32, device=device)
        bits = self.buf.view(torch.int32)
        bits[: self.MARGIN] = self.CANARY
        bits[self.MARGIN + self.n :] = self.CANARY
        self.buf[self.MARGIN : self.MARGIN + self.n] = float("nan")
        assert self.ptr % 16 == 0

    @property
    def ptr(self) -> int:
        """The 16-byte-aligned payload pointer for the C ABI."""
        return self.buf.data_ptr() + 4 * self.MARGIN

    def result(self, what: str = "") -> Tensor:
        """The payload on the CPU, after checking both margins and that every element was written."""
        host = self.buf.cpu()
        bits = host.view(torch.int32)
        for name, part in (("before", bits[: self.MARGIN]), ("after", bits[self.MARGIN + self.n :])):
            bad = (part != self.CANARY).nonzero().flatten()
            assert bad.numel() == 0, f"{what}: {bad.numel()} words written {name} the output, first at offset {int(bad[0])}"
        payload = host[self.MARGIN : self.MARGIN + self.n]
        unwritten = torch.isnan(payload).nonzero().flatten()
        assert unwritten.numel() == 0, (
            f"{what}: {unwritten.numel()} of {self.n} output elements are NaN (unwritten?), first at flat index {int(unwritten[0])}"
        )
        return payload.reshape(self.shape).clone()


# ------------------------------------------------------------------- depthwise convolution, squeeze-excitation, head
U2 = 2.0**-23  # twice the float32 unit roundoff, as in tests/matmul_bound.py


def dwconv_f64(x_nhwc: Tensor, w_rrc: Tensor, bias: Tensor | None, r: int, stride: int, pad: int) -> tuple[Tensor, Tensor]:
    """(pre, magnitude) of the depthwise convolution in float64, [B, Ho, Wo, C]: pre = sum over the R x R taps of
    x * w + bias, magnitude = the same sum of absolute values -- what every partial sum is bounded by.  A float32 sum
    of the K = R * R products and the bias, in any order, fused or not, is within (K + 2) 2^-23 magnitude of pre
    (tests/matmul_bound.py, form 2)."""
    b, h, w, c = x_nhwc.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    xp = F.pad(x_nhwc.double(), (0, 0, pad, pad, pad, pad))
    w64 = w_rrc.double()
    pre = torch.zeros(b, ho, wo, c, dtype=torch.float64)
    mag = torch.zeros_like(pre)
    for dr in range(r):
        for ds in range(r):
            window = xp[:, dr : dr + (ho - 1) * stride + 1 : stride, ds : ds + (wo - 1) * stride + 1 : stride, :]
            pre += window * w64[dr, ds]
            mag += window.abs() * w64[dr, ds].abs()
    if bias is not None:
        pre += bias.double()
        mag += bias.double().abs()
    return pre, mag


def dwconv_bound(mag: Tensor, r: int) -> Tensor:
    return (r * r + 2) * U2 * mag


def pooled_mean_bound(y_want: Tensor, y_bound: Tensor | None = None) -> Tensor:
    """Bound of the float32 mean over (H, W) of y [B, H, W, C] against the float64 mean of `y_want`.  The kernels add the
    HW values in some order, multiply by a rounded 1 / HW (or divide), and may add two strips' shares: at most HW + 2
    roundings on partial sums bounded by sum |y|, hence (HW + 2) 2^-23 mean |y|; an error `y_bound` of the values
    themselves passes through the mean as its own mean."""
    hw = y_want.shape[1] * y_want.shape[2]
    size = y_want.abs() if y_bound is None else y_want.abs() + y_bound
    bound = (hw + 2) * U2 * size.mean(dim=(1, 2))
    return bound if y_bound is None else bound + y_bound.mean(dim=(1, 2))


def se_gate_reference(pooled: Tensor, w1: Tensor, b1: Tensor | None, w2: Tensor, b2: Tensor | None, *,
                      fc1_exact: bool = False) -> tuple[Tensor, Tensor]:
    """(want, bound) of gate = sigmoid(w2 . silu(w1 . pooled + b1) + b2), all in float64 from the float32 operands
    (pooled [B, C], w1 [S, C], w2 [C, S]).

        e1 = (C + 2) 2^-23 (|p| |W1|^T + |b1|)                                fc1 as a float32 sum of C products + bias
        q, eq = expected(p W1^T + b1, e1, SiLU)
        e2 = (S + 2) 2^-23 ((|q| + eq) |W2|^T + |b2|) + eq |W2|^T             fc2 on the q the kernel holds, plus what
                                                                              q's own error moves the exact product by
        gate, bound = expected(q W2^T + b2, e2, sigmoid)

    e1 is a worst case that grows with C -- (C + 2) 2^-23 is 4.6e-4 at C = 3840, on a magnitude of some tens -- and e2
    multiplies it by the sum over a row of |W2|, so from C of several hundred on a dropped 16-byte chunk of a weight row
    stays inside the bound (tests/test_conv_bounds_host.py).  `fc1_exact` is the form for large C: the caller passes
    operands whose fc1 is exact in float32 in any order (`se_exact_fc1_operands`; asserted with `assert_exact_range`),
    e1 is then ZERO, and what is left is the SiLU arithmetic and fc2."""
    p, w1d, w2d = pooled.double(), w1.double(), w2.double()
    c, s = w1d.shape[1], w1d.shape[0]
    zero1, zero2 = torch.zeros(s, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    b1d = zero1 if b1 is None else b1.double()
    b2d = zero2 if b2 is None else b2.double()
    e1 = (c + 2) * U2 * (p.abs() @ w1d.abs().T + b1d.abs())
    if fc1_exact:
        e1 = torch.zeros_like(e1)
    q, eq = expected(p @ w1d.T + b1d, e1, ACT_SILU)
    e2 = (s + 2) * U2 * ((q.abs() + eq) @ w2d.abs().T + b2d.abs()) + eq @ w2d.abs().T
    return expected(q @ w2d.T + b2d, e2, ACT_SIGMOID)


def head_reference(x_nhwc: Tensor, w: Tensor, bias: Tensor | None) -> tuple[Tensor, Tensor]:
    """(want, bound) of feat = mean over (H, W) of x . w^T + bias in float64 (x [B, H, W, C], w [E, C]).

        ep = (HW + 1) 2^-23 mean |x|                                  HW - 1 additions and one division
        bound = (C + 2) 2^-23 ((|p| + ep) |W|^T + |b|) + ep |W|^T     the product on the p the kernel holds, plus what
                                                                      p's own error moves the exact product by"""
    b, h, wd, c = x_nhwc.shape
    hw = h * wd
    x64, w64 = x_nhwc.double().reshape(b, hw, c), w.double()
    b64 = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    p = x64.mean(dim=1)
    ep = (hw + 1) * U2 * x64.abs().mean(dim=1)
    want = p @ w64.T + b64
    bound = (c + 2) * U2 * ((p.abs() + ep) @ w64.abs().T + b64.abs()) + ep @ w64.abs().T
    return want, bound


def se_exact_fc1_operands(b: int, c: int, s: int, gen: torch.Generator) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(pooled, w1, b1, w2, b2) with an fc1 that is exact in float32: pooled integers in -3 .. 3, w1 in {-1, 0, 1} / 16
    (/ 64 from C = 1024 on, so that the squeezed values stay of order one), b1 multiples of the same quantum."""
    quantum = 1.0 / 16 if c < 1024 else 1.0 / 64
    pooled = torch.randint(-3, 4, (b, c), generator=gen).float()
    w1 = torch.randint(-1, 2, (s, c), generator=gen).float() * quantum
    b1 = torch.randint(-16, 17, (s,), generator=gen).float() * quantum
    top = float((pooled.double().abs() @ w1.double().abs().T + b1.double().abs()).max())
    assert top < 2.0**24 * quantum  # tests/matmul_bound.py, assert_exact_range: no partial sum of fc1 rounds
    w2 = torch.randn(c, s, generator=gen) / s**0.5
    return pooled, w1, b1, w2, torch.randn(c, generator=gen)
