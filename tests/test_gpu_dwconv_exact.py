"""The depthwise convolutions of the MBConv blocks at the C ABI (`isc_dwconv2d_nhwc`, `isc_dwconv2d_nhwc_pool`): the
3 x 3 row sweep `k_dwconv3x3_rows` in its five WRITE / POOL / GATE forms and both SILU flags, and the generic
`k_dwconv_nhwc`, against a float64 tap sum (tests/conv_reference.py).  No tolerance here is measured.

Exact integers.  x in -4 .. 4, w in -2 .. 2, integer bias: at most 9 * 8 + 8 (25 * 8 + 8) per output, so every fused
multiply-add is exact and y must EQUAL the float64 sum; a gate from {0.5, 1, 2} is one exact float32 multiplication.  The
pooled mean adds integers (exact) and multiplies by a float32 1 / HW: with H * W a power of two nothing rounds and the
mean equals the float64 mean bit for bit; otherwise 1 / HW, the product and the addition of two strips' shares round,
three roundings of 2^-24 on at most sum |y| / HW:  |pooled - want| <= 2^-22 sum |y| / HW.

Real operands.  y within `expected()` of the float64 sum with K = R * R; a real gate is one more float32 rounding; the
pooled mean by `pooled_mean_bound`.

Shapes.  H = 1, 2, 3, 4, 5, 9 covers every residue of the four-row register rotation; W = 1, 6, 7, 8, 13, 14, 15 is one
strip of seven columns (ragged, full), two strips, and the three strips that send the pooled forms to the fallback
(`isc_dwconv2d_nhwc` + `isc_global_avgpool_nhwc`; the pooling alone and the gated output are refused there).  C = 4 and
260 with B = 3: B * strips * C / 4 threads is never a multiple of the 256-thread workgroup."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
from conv_reference import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, GuardedOutput, _activate, dwconv_bound,  # noqa: E402
                            dwconv_f64, expected, pooled_mean_bound)

pytestmark = pytest.mark.gpu

B = 3
HS, WS, CS = (1, 2, 3, 4, 5, 9), (1, 6, 7, 8, 13, 14, 15), (4, 260)
POW2 = ((16, 4), (4, 8), (4, 16))  # H * W a power of two: one strip, two strips, the fallback
SHAPES = tuple((h, w) for h in HS for w in WS) + tuple(s for s in POW2 if s not in [(h, w) for h in HS for w in WS])
TW = 7  # columns of a strip


def is_pow2(n: int) -> bool:
    return n & (n - 1) == 0


class Depthwise:
    """Operands on the device and the two entries."""

    def __init__(self, device, x, w, bias, gate, r, stride, pad) -> None:
        self.device, self.r, self.stride, self.pad = device, r, stride, pad
        self.shape = tuple(x.shape)
        self.x, self.w = x.contiguous().to(device), w.contiguous().to(device)
        self.bias = None if bias is None else bias.to(device)
        self.gate = None if gate is None else gate.contiguous().to(device)
        b, h, wd, c = self.shape
        self.out_shape = (b, (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - r) // stride + 1, c)

    def pool(self, act: int, y: bool, pooled: bool, gate: bool):
        """`isc_dwconv2d_nhwc_pool` -> (status, y buffer or None, pooled buffer or None)."""
        from imagescry_amd import _lib

        b, h, wd, c = self.shape
        yb = GuardedOutput(self.out_shape, self.device) if y else None
        pb = GuardedOutput((b, c), self.device) if pooled else None
        st = _lib.load().isc_dwconv2d_nhwc_pool(self.x.data_ptr(), b, h, wd, c, self.w.data_ptr(), self.r, self.stride, self.pad,
                                                _lib.ptr(self.bias), act, self.gate.data_ptr() if gate else None,
                                                yb.ptr if y else None, pb.ptr if pooled else None, _lib.stream_handle(self.device))
        return st, yb, pb

    def plain(self, act: int, what: str) -> torch.Tensor:
        from imagescry_amd import _lib

        b, h, wd, c = self.shape
        yb = GuardedOutput(self.out_shape, self.device)
        st = _lib.load().isc_dwconv2d_nhwc(self.x.data_ptr(), b, h, wd, c, self.w.data_ptr(), self.r, self.stride, self.pad,
                                           _lib.ptr(self.bias), act, yb.ptr, _lib.stream_handle(self.device))
        _lib.check(st, what)
        return yb.result(what)


def integer_operands(shape, r: int, seed: int):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    x = mb.int_tensor((b, h, w, c), -4, 4, g)
    wt = mb.int_tensor((r, r, c), -2, 2, g)
    bias = mb.int_tensor((c,), -8, 8, g)
    gate = mb.choice_tensor((b, c), (0.5, 1.0, 2.0), g)
    return x, wt, bias, gate


def assert_pooled_integers(pooled: torch.Tensor, y_want: torch.Tensor, what: str) -> None:
    hw = y_want.shape[1] * y_want.shape[2]
    want = y_want.mean(dim=(1, 2))
    if is_pow2(hw):
        assert torch.equal(pooled.double(), want), (what, mb.worst_ratio(pooled, want, torch.full_like(want, 2.0**-24)))
    else:
        mb.assert_within_bound(pooled, want, 2.0**-22 * y_want.abs().sum(dim=(1, 2)) / hw, what)


def assert_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert torch.equal(got.double(), want), (what, mb.worst_ratio(got, want, torch.full_like(want, 2.0**-24)))


@pytest.mark.parametrize("h,w", SHAPES)
def test_rows_exact_integers(h: int, w: int, device: torch.device) -> None:
    from imagescry_amd import _lib

    strips = -(-w // TW)
    for c in CS:
        assert (B * strips * c // 4) % 256
        x, wt, bias, gate = integer_operands((B, h, w, c), 3, 100 * h + w + c)
        pre, mag = dwconv_f64(x, wt, bias, 3, 1, 1)
        assert float(mag.max()) * 2 < mb.EXACT_LIMIT  # ... and twice that: the gate
        dw = Depthwise(device, x, wt, bias, gate, 3, 1, 1)
        for act in (ACT_NONE, ACT_RELU):
            what = f"dwconv rows {(B, h, w, c)} act {act}"
            y_want = _activate(pre, act)
            gated = (y_want.float() * gate[:, None, None, :]).double()  # ONE float32 multiplication
            assert torch.equal(gated, y_want * gate[:, None, None, :].double())
            assert_equal(dw.plain(act, what), y_want, f"{what} write")
            st, yb, _ = dw.pool(act, True, False, True)
            _lib.check(st, what)
            assert_equal(yb.result(what), gated, f"{what} write + gate")
            if strips <= 2:
                st, _, pb = dw.pool(act, False, True, False)
                _lib.check(st, what)
                assert_pooled_integers(pb.result(what), y_want, f"{what} pool")
                st, yb, pb = dw.pool(act, True, True, True)
                _lib.check(st, what)
                assert_equal(yb.result(what), gated, f"{what} write + pool + gate: y")
                assert_pooled_integers(pb.result(what), y_want, f"{what} write + pool + gate: pooled (of the ungated y)")
            else:  # the pooling alone and the gated output exist in the row sweep only
                assert dw.pool(act, False, True, False)[0] == _lib.ISC_ERR_UNSUPPORTED
                assert dw.pool(act, True, True, True)[0] == _lib.ISC_ERR_UNSUPPORTED
            st, yb, pb = dw.pool(act, True, True, False)  # three strips: the row sweep, then the pooling kernel
            _lib.check(st, what)
            assert_equal(yb.result(what), y_want, f"{what} write + pool: y")
            assert_pooled_integers(pb.result(what), y_want, f"{what} write + pool: pooled")


# (B, H, W, C, R, stride, pad): k_dwconv_nhwc -- everything but 3 x 3 / 1 / 1
GENERIC = ((2, 9, 7, 260, 5, 2, 2), (3, 8, 10, 4, 3, 2, 1), (1, 5, 5, 8, 5, 1, 2), (2, 6, 6, 12, 3, 1, 0), (1, 8, 8, 4, 3, 2, 1),
           (1, 1030, 1030, 4, 5, 1, 2))  # the last: more than 4096 workgroups of threads, so the grid-stride loop goes round


@pytest.mark.parametrize("b,h,w,c,r,stride,pad", GENERIC)
def test_generic_exact_integers(b, h, w, c, r, stride, pad, device: torch.device) -> None:
    from imagescry_amd import _lib

    x, wt, bias, gate = integer_operands((b, h, w, c), r, h + w + c + r)
    pre, mag = dwconv_f64(x, wt, bias, r, stride, pad)
    assert float(mag.max()) < mb.EXACT_LIMIT
    dw = Depthwise(device, x, wt, bias, gate, r, stride, pad)
    for act in (ACT_NONE, ACT_RELU):
        what = f"dwconv {(b, h, w, c, r, stride, pad)} act {act}"
        y_want = _activate(pre, act)
        assert_equal(dw.plain(act, what), y_want, what)
        if h * w > 4096:
            continue  # a float32 sum of that many integers is no longer exact
        st, yb, pb = dw.pool(act, True, True, False)
        _lib.check(st, what)
        assert_equal(yb.result(what), y_want, f"{what} + pool: y")
        assert_pooled_integers(pb.result(what), y_want, f"{what} + pool: pooled")
        assert dw.pool(act, True, False, True)[0] == _lib.ISC_ERR_UNSUPPORTED
        assert dw.pool(act, False, True, False)[0] == _lib.ISC_ERR_UNSUPPORTED


@pytest.mark.parametrize("act", (ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_SIGMOID))
@pytest.mark.parametrize("h,w,r,stride,pad", ((5, 7, 3, 1, 1), (9, 13, 3, 1, 1), (4, 8, 3, 1, 1), (3, 15, 3, 1, 1), (1, 1, 3, 1, 1),
                                             (9, 7, 5, 2, 2), (8, 10, 3, 2, 1)))
def test_real_operands_within_bound(h, w, r, stride, pad, act, device: torch.device) -> None:
    """SiLU runs the SILU = true instantiations of the row sweep, every other activation the per-element switch."""
    from imagescry_amd import _lib

    rows = (r, stride, pad) == (3, 1, 1)
    strips = -(-w // TW)
    for c in CS:
        g = torch.Generator().manual_seed(h * 31 + w + c + act)
        x = torch.randn(B, h, w, c, generator=g)
        wt = torch.randn(r, r, c, generator=g) / r
        bias = torch.randn(c, generator=g)
        gate = torch.sigmoid(torch.randn(B, c, generator=g) * 2)
        pre, mag = dwconv_f64(x, wt, bias, r, stride, pad)
        want, bound = expected(pre, dwconv_bound(mag, r), act)
        g64 = gate[:, None, None, :].double()
        want_g, bound_g = want * g64, bound * g64 + 2.0**-24 * (want.abs() + bound) * g64  # one more float32 multiplication
        dw = Depthwise(device, x, wt, bias, gate, r, stride, pad)
        what = f"dwconv {(B, h, w, c, r, stride, pad)} act {act}"
        ratios = [mb.assert_within_bound(dw.plain(act, what), want, bound, f"{what} write")]
        st, yb, pb = dw.pool(act, True, True, False)
        _lib.check(st, what)
        ratios.append(mb.assert_within_bound(yb.result(what), want, bound, f"{what} write + pool: y"))
        pool_want, pool_bound = want.mean(dim=(1, 2)), pooled_mean_bound(want, bound)
        ratios.append(mb.assert_within_bound(pb.result(what), pool_want, pool_bound, f"{what} write + pool: pooled"))
        if rows:
            st, yb, _ = dw.pool(act, True, False, True)
            _lib.check(st, what)
            ratios.append(mb.assert_within_bound(yb.result(what), want_g, bound_g, f"{what} write + gate"))
        if rows and strips <= 2:
            st, _, pb = dw.pool(act, False, True, False)
            _lib.check(st, what)
            ratios.append(mb.assert_within_bound(pb.result(what), pool_want, pool_bound, f"{what} pool"))
            st, yb, pb = dw.pool(act, True, True, True)
            _lib.check(st, what)
            ratios.append(mb.assert_within_bound(yb.result(what), want_g, bound_g, f"{what} write + pool + gate: y"))
            ratios.append(mb.assert_within_bound(pb.result(what), pool_want, pool_bound, f"{what} write + pool + gate: pooled"))
        print(f"{what}: error / bound = {max(ratios):.4f}")
