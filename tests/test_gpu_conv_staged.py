"""The register-staged form of `k_conv_f32` (`DMA = false`): `isc_conv2d_nhwc_gated` and `isc_linear_centered` at the C
ABI, against the two references of tests/matmul_bound.py -- exact integers (`torch.equal` with the float64 product) and
the derived element-wise bound.  No tolerance here is measured.

The operand the kernel multiplies is `x * gate` (or `x - mean`) formed as ONE float32 operation; the tests form the same
float32 operand on the CPU and take its float64 product with the weights as `want`.  R x R filters go through
`torch.nn.functional.unfold` of that operand (pure data movement, padding taps stay zero).

Activations (`expected`, shared through tests/conv_reference.py).  ReLU is 1-Lipschitz, so the activation is applied to
`want` and the bound kept.  For SiLU, GELU and sigmoid `want` is the float64 activation of the float64 pre-activation, and the bound is

    1.13 * (pre-activation bound) + 2^-21 * (1 + |value|)

The first term: max |silu'| = 1.0998, max |gelu'| = 1.1290, max |sigmoid'| = 0.25, all <= 1.13, so an error e of the
pre-activation moves the activation by at most 1.13 e.  The second: the float32 activation arithmetic itself, 2^-21 = 8
float32 roundoffs on a quantity of size 1 + |value| (exp and reciprocal at about 1 ulp each, two or three multiplications
and additions on top), `value` being the expected output.  With `ISC_ACT_RESIDUAL_AFTER` the residual is added to the
activation by one more float32 addition: `want` gets the residual, the pre-activation bound does not, and |value| is
|activation| + |residual|.

Tiles.  `conv_launch` takes 64 x 256 tiles wherever 64-channel tiles pad Cout less than 128-channel ones do, so of the
shapes below Cout = 132, 160, 260, 36 and 64 run `k_conv_f32<64, 256, false, false>` and Cout = 128, 196 and 256 run
`k_conv_f32<128, 128, false, false>` (Cout = 196: a second channel tile of 68 = 64 + 4 channels)."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
from conv_reference import ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_SIGMOID, RES_AFTER, _activate, expected  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout, R, stride, pad)
GATED_CASES = (
    (3, 9, 9, 96, 132, 1, 1, 0),  # 243 pixels in one 256-pixel tile; channel tiles 64 + 64 + 4; three K steps
    (2, 13, 11, 32, 160, 1, 1, 0),  # 64 x 256 tiles; three channel tiles, the last half empty; one K step; ragged 2nd pixel tile of 30
    (2, 13, 11, 512, 160, 1, 1, 0),  # the same with 16 K steps
    (5, 1, 1, 64, 256, 1, 1, 0),  # one pixel per image: every row of a tile has its own gate
    (2, 9, 7, 32, 64, 3, 2, 1),  # padding taps stay zero after gating
    (2, 8, 8, 64, 128, 3, 1, 1),  # 128-channel tile, 18 K steps
    (3, 9, 9, 96, 196, 1, 1, 0),  # 128 x 128 tiles: two pixel tiles, the seam inside image 1; 2nd channel tile 68 wide
)
WAYS = ("bias", "bias_residual", "silu_residual_after")


@functools.lru_cache(maxsize=None)
def gated_case(case: tuple[int, ...]):
    """Operands of a gated case and its float32 GEMM operands on the CPU (computed once, never modified)."""
    b, h, w, cin, cout, r, stride, pad = case
    g = torch.Generator().manual_seed(sum(case) * 7 + cin)
    x = torch.randn(b, h, w, cin, generator=g)
    gate = torch.sigmoid(torch.randn(b, cin, generator=g) * 2).clamp_min(1e-3)  # (0, 1]
    wt = torch.randn(cout, r, r, cin, generator=g) / (r * r * cin) ** 0.5
    bias = torch.randn(cout, generator=g)
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    res = torch.randn(b * ho * wo, cout, generator=g)
    xg = x * gate[:, None, None, :]  # ONE float32 multiplication, as the kernel's staging does
    if r == 1 and stride == 1 and pad == 0:
        a, w2 = xg.reshape(-1, cin), wt.reshape(cout, cin)
    else:
        cols = F.unfold(xg.permute(0, 3, 1, 2), (r, r), padding=pad, stride=stride)  # [B, Cin * R * R, Ho * Wo], (c, r, s)
        a = cols.transpose(1, 2).reshape(b * ho * wo, cin * r * r).contiguous()
        w2 = wt.permute(0, 3, 1, 2).reshape(cout, cin * r * r).contiguous()
    return dict(x=x, gate=gate, w=wt, bias=bias, res=res, a=a, w2=w2, m=b * ho * wo)


def run_gated(device, case, x, gate, wt, bias, res, act) -> torch.Tensor:
    from imagescry_amd import _lib

    b, h, w, cin, cout, r, stride, pad = case
    lib = _lib.load()
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    dx, dg, dw = x.contiguous().to(device), gate.contiguous().to(device), wt.contiguous().to(device)
    db = None if bias is None else bias.to(device)
    dr = None if res is None else res.contiguous().to(device)
    out = torch.full((b * ho * wo, cout), float("nan"), device=device)  # an unwritten element fails
    st = lib.isc_conv2d_nhwc_gated(dx.data_ptr(), b, h, w, cin, dg.data_ptr(), dw.data_ptr(), cout, r, r, stride, pad,
                                   None if db is None else db.data_ptr(), None if dr is None else dr.data_ptr(), act,
                                   out.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_conv2d_nhwc_gated")
    return out.cpu()


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", GATED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gated_conv_within_bound(case, way, device: torch.device) -> None:
    c = gated_case(case)
    a, w2, bias, res = c["a"], c["w2"], c["bias"], c["res"]
    if way == "bias":
        want, bound = expected(mb.product_f64(a, w2, bias), mb.product_bound(a, w2, bias), ACT_NONE)
        got = run_gated(device, case, c["x"], c["gate"], c["w"], bias, None, ACT_NONE)
    elif way == "bias_residual":
        want, bound = expected(mb.product_f64(a, w2, bias, res), mb.product_bound(a, w2, bias, res), ACT_NONE)
        got = run_gated(device, case, c["x"], c["gate"], c["w"], bias, res, ACT_NONE)
    else:
        want, bound = expected(mb.product_f64(a, w2, bias), mb.product_bound(a, w2, bias), ACT_SILU, res.double())
        got = run_gated(device, case, c["x"], c["gate"], c["w"], bias, res, ACT_SILU | RES_AFTER)
    ratio = mb.assert_within_bound(got, want, bound, f"gated {case} {way}")
    print(f"gated {case} {way}: error / bound = {ratio:.4f}")


@pytest.mark.parametrize("act", (ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_SIGMOID))
@pytest.mark.parametrize("case", (GATED_CASES[0], GATED_CASES[6]), ids=lambda c: "x".join(map(str, c)))
def test_gated_conv_activations(case, act, device: torch.device) -> None:
    """Every activation, bias and residual inside it."""
    c = gated_case(case)
    a, w2, bias, res = c["a"], c["w2"], c["bias"], c["res"]
    want, bound = expected(mb.product_f64(a, w2, bias, res), mb.product_bound(a, w2, bias, res), act)
    got = run_gated(device, case, c["x"], c["gate"], c["w"], bias, res, act)
    ratio = mb.assert_within_bound(got, want, bound, f"gated {case} act {act}")
    print(f"gated {case} act {act}: error / bound = {ratio:.4f}")


@pytest.mark.parametrize("act", (ACT_NONE, ACT_RELU))
@pytest.mark.parametrize("cin,cout", ((2048, 260), (64, 36), (64, 200)))
def test_gated_conv_exact_integers(cin, cout, act, device: torch.device) -> None:
    """4 x 20 x 20 = 1600 pixels of integers: seven 256-pixel tiles (Cout = 260: five channel tiles, 64 K steps; Cout = 36:
    one ragged channel tile, two K steps) or thirteen 128-pixel tiles by two channel tiles (Cout = 200), image seams
    inside tiles; x in -2 .. 2, gate in {0.5, 1, 2}, w in {-1, 0, 1}: every partial sum is a multiple of 0.5 far below
    2^23, so the result must equal the float64 product bit for bit."""
    case = (4, 20, 20, cin, cout, 1, 1, 0)
    g = torch.Generator().manual_seed(cin + cout)
    x = mb.int_tensor((4, 20, 20, cin), -2, 2, g)
    gate = mb.choice_tensor((4, cin), (0.5, 1.0, 2.0), g)
    wt = mb.int_tensor((cout, 1, 1, cin), -1, 1, g)
    bias = mb.int_tensor((cout,), -8, 8, g)
    res = mb.int_tensor((1600, cout), -8, 8, g)
    a = (x * gate[:, None, None, :]).reshape(-1, cin)
    w2 = wt.reshape(cout, cin)
    mb.assert_exact_range(a, w2, bias, res, a_quantum=0.5)
    want = _activate(mb.product_f64(a, w2, bias, res), act)
    got = run_gated(device, case, x, gate, wt, bias, res, act)
    assert torch.equal(got.double(), want), mb.worst_ratio(got, want, torch.full_like(want, 2.0**-24))


# ------------------------------------------------------------------------------------------------ isc_linear_centered
def run_centered(device, x, mean, w, bias) -> torch.Tensor:
    from imagescry_amd import _lib

    lib = _lib.load()
    n, f = x.shape
    k = w.shape[0]
    dx, dm, dw = x.contiguous().to(device), mean.contiguous().to(device), w.contiguous().to(device)
    db = None if bias is None else bias.to(device)
    out = torch.full((n, k), float("nan"), device=device)
    st = lib.isc_linear_centered(dx.data_ptr(), n, f, dm.data_ptr(), dw.data_ptr(), k, None if db is None else db.data_ptr(),
                                 out.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_linear_centered")
    return out.cpu()


# (n, F, K).  K = 132 and 260 run 64 x 256 tiles (see the module docstring), K = 196 the 128 x 128 ones with three pixel
# tiles; F = 1280 is the one reduction above 1024 terms the bound is used for (the bound holds for any length; see
# tests/matmul_bound.py)
CENTERED_CASES = ((300, 64, 132), (1, 32, 4), (257, 1280, 64), (1000, 96, 260), (300, 64, 196))


@pytest.mark.parametrize("with_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("n,f,k", CENTERED_CASES)
def test_linear_centered_within_bound(n, f, k, with_bias, device: torch.device) -> None:
    """Rows randn + 50 with a mean near 50: the bound is taken on the centred operand, so the centring has to happen
    before the product -- x . w - mean . w carries the rounding of terms 50 times the size of the result."""
    g = torch.Generator().manual_seed(n + 3 * f + 5 * k)
    x = torch.randn(n, f, generator=g) + 50.0
    mean = 50.0 + 0.1 * torch.randn(f, generator=g)
    w = torch.randn(k, f, generator=g) / f**0.5
    bias = torch.randn(k, generator=g) if with_bias else None
    a = x - mean  # ONE float32 subtraction, as the kernel's staging does
    want = mb.product_f64(a, w, bias)
    bound = mb.product_bound(a, w, bias, long_k=f > mb.MAX_BOUND_K)
    got = run_centered(device, x, mean, w, bias)
    ratio = mb.assert_within_bound(got, want, bound, f"linear_centered {(n, f, k)} bias={with_bias}")
    print(f"linear_centered {(n, f, k)} bias={with_bias}: error / bound = {ratio:.4f}")


@pytest.mark.parametrize("with_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("k", (132, 196))
def test_linear_centered_exact_integers(k, with_bias, device: torch.device) -> None:
    n, f = 3000, 1024
    g = torch.Generator().manual_seed(k)
    x = mb.int_tensor((n, f), -3, 3, g)
    mean = mb.int_tensor((f,), -2, 2, g)
    w = mb.int_tensor((k, f), -1, 1, g)
    bias = mb.int_tensor((k,), -8, 8, g) if with_bias else None
    a = x - mean
    mb.assert_exact_range(a, w, bias)
    want = mb.product_f64(a, w, bias)
    got = run_centered(device, x, mean, w, bias)
    assert torch.equal(got.double(), want), mb.worst_ratio(got, want, torch.full_like(want, 2.0**-24))


def test_linear_centered_refusals(device: torch.device) -> None:
    from imagescry_amd import _lib

    lib = _lib.load()
    stream = _lib.stream_handle(device)
    x = torch.zeros(4, 64, device=device)
    mean = torch.zeros(68, device=device)
    w = torch.zeros(4, 64, device=device)
    out = torch.zeros(4, 4, device=device)
    call = lib.isc_linear_centered
    assert call(x.data_ptr(), 4, 48, mean.data_ptr(), w.data_ptr(), 4, None, out.data_ptr(), stream) == _lib.ISC_ERR_UNSUPPORTED
    assert call(x.data_ptr(), 4, 64, mean.data_ptr() + 4, w.data_ptr(), 4, None, out.data_ptr(), stream) == _lib.ISC_ERR_ALIGNMENT
    assert call(x.data_ptr(), 0, 64, mean.data_ptr(), w.data_ptr(), 4, None, out.data_ptr(), stream) == _lib.ISC_ERR_INVALID_ARG
    assert call(x.data_ptr(), 4, 64, mean.data_ptr(), w.data_ptr(), 4, None, out.data_ptr(), stream) == _lib.ISC_OK
    torch.cuda.synchronize(device)
    assert torch.equal(out.cpu(), torch.zeros(4, 4))
