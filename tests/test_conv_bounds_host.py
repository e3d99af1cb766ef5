"""CPU checks of the depthwise, squeeze-excitation and head bounds of tests/conv_reference.py, in the manner of
tests/test_matmul_bound_host.py: an honest float32 evaluation (torch's) stays inside each bound, and the faults a kernel
of this kind can have leave it -- one 16-byte chunk (four elements) of a weight row dropped, a neighbouring image's gate
or pooled vector used, a strip of the pooled sum added twice.  More than 90 % of the outputs the fault touches must fall
outside."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
from conv_reference import (ACT_GELU, ACT_NONE, ACT_SIGMOID, ACT_SILU, GuardedOutput, dwconv_bound, dwconv_f64, expected,  # noqa: E402
                            gemm_operands, head_reference, packed_k_rows, pooled_mean_bound, se_exact_fc1_operands, se_gate_reference)


def _outside(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    return (got.double() - want).abs() > bound


# ---------------------------------------------------------------------------------------------------------- depthwise
def _dw(act: int, r: int = 3, stride: int = 1, pad: int = 1):
    g = torch.Generator().manual_seed(40 + act + r)
    x = torch.randn(3, 9, 13, 8, generator=g)
    w = torch.randn(r, r, 8, generator=g) / r
    bias = torch.randn(8, generator=g)
    gate = torch.sigmoid(torch.randn(3, 8, generator=g) * 2)
    pre, mag = dwconv_f64(x, w, bias, r, stride, pad)
    want, bound = expected(pre, dwconv_bound(mag, r), act)
    return x, w, bias, gate, want, bound


def _dw_f32(x, w, bias, act: int, r: int = 3, stride: int = 1, pad: int = 1) -> torch.Tensor:
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(2, 0, 1)[:, None], bias, stride=stride, padding=pad, groups=x.shape[3])
    y = {ACT_NONE: lambda t: t, ACT_SILU: F.silu, ACT_GELU: F.gelu, ACT_SIGMOID: torch.sigmoid}[act](y)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("r,stride,pad", ((3, 1, 1), (5, 2, 2)))
@pytest.mark.parametrize("act", (ACT_NONE, ACT_SILU, ACT_GELU, ACT_SIGMOID))
def test_float32_depthwise_is_within_the_bound(act: int, r: int, stride: int, pad: int) -> None:
    x, w, bias, gate, want, bound = _dw(act, r, stride, pad)
    got = _dw_f32(x, w, bias, act, r, stride, pad)
    ratio = mb.assert_within_bound(got, want, bound, f"torch float32 depthwise, act {act}")
    print(f"depthwise {r} x {r} act {act}: torch float32 uses {ratio:.3f} of the bound")
    # the gated output: one more float32 multiplication
    g64 = gate[:, None, None, :].double()
    mb.assert_within_bound(got * gate[:, None, None, :], want * g64, bound * g64 + 2.0**-24 * (want.abs() + bound) * g64)
    # and the pooled mean
    mb.assert_within_bound(got.mean(dim=(1, 2)), want.mean(dim=(1, 2)), pooled_mean_bound(want, bound))


@pytest.mark.parametrize("act", (ACT_NONE, ACT_SILU))
def test_depthwise_faults_leave_the_bound(act: int) -> None:
    x, w, bias, gate, want, bound = _dw(act)
    # four channels of one filter tap dropped: those channels, every pixel the tap reaches
    for tap in ((1, 1), (0, 2)):
        bad = w.clone()
        bad[tap[0], tap[1], 4:8] = 0.0
        got = _dw_f32(x, bad, bias, act)
        out = _outside(got, want, bound)
        rows = [oy for oy in range(9) if 0 <= oy + tap[0] - 1 < 9]  # where the tap is no padding
        cols = [ox for ox in range(13) if 0 <= ox + tap[1] - 1 < 13]
        reached = out[:, rows][:, :, cols][..., 4:8]
        assert reached.double().mean() > 0.9, (act, tap, float(reached.double().mean()))
        assert not out[..., :4].any() and int(out.sum()) == int(reached.sum())
    # image 0 multiplied by the gate of image 1
    good = _dw_f32(x, w, bias, act)
    g64 = gate[:, None, None, :].double()
    bound_g = bound * g64 + 2.0**-24 * (want.abs() + bound) * g64
    wrong = good.clone() * gate[:, None, None, :]
    wrong[0] = good[0] * gate[1]
    out = _outside(wrong, want * g64, bound_g)
    assert out[0].double().mean() > 0.9 and not out[1:].any()
    # the second strip of seven columns added twice into the pooled sum
    hw = 9 * 13
    pooled = (good.sum(dim=(1, 2)) + good[:, :, 7:].sum(dim=(1, 2))) / hw
    out = _outside(pooled, want.mean(dim=(1, 2)), pooled_mean_bound(want, bound))
    assert out.double().mean() > 0.9
    # ... and the integer form of the pooled bound (tests/test_gpu_dwconv_exact.py): 2^-22 sum |y| / HW
    g = torch.Generator().manual_seed(5)
    y = mb.int_tensor((3, 9, 13, 8), -80, 80, g)
    want_i = y.double().mean(dim=(1, 2))
    bound_i = 2.0**-22 * y.double().abs().sum(dim=(1, 2)) / hw
    mb.assert_within_bound(y.sum(dim=(1, 2)) * torch.tensor(1.0 / hw), want_i, bound_i)
    mb.assert_within_bound(y[:, :, :7].sum(dim=(1, 2)) * torch.tensor(1.0 / hw) + y[:, :, 7:].sum(dim=(1, 2)) * torch.tensor(1.0 / hw),
                           want_i, bound_i)
    twice = (y.sum(dim=(1, 2)) + y[:, :, 7:8].sum(dim=(1, 2))) * torch.tensor(1.0 / hw)  # one COLUMN of the second strip twice
    assert _outside(twice, want_i, bound_i).double().mean() > 0.9


# ------------------------------------------------------------------------------------------------------------ SE gate
def _se(c: int, s: int, fc1_exact: bool = False):
    g = torch.Generator().manual_seed(c + s)
    if fc1_exact:  # fc1 is exact in float32, its term of the bound is zero
        ops = se_exact_fc1_operands(3, c, s, g)
        mb.assert_exact_range(ops[0], ops[1], ops[2], w_quantum=1.0 / 16 if c < 1024 else 1.0 / 64)
        return ops
    pooled = torch.randn(3, c, generator=g)
    w1 = torch.randn(s, c, generator=g) / c**0.5
    b1 = torch.randn(s, generator=g)
    w2 = torch.randn(c, s, generator=g) / s**0.5
    return pooled, w1, b1, w2, torch.randn(c, generator=g)


def _se_f32(pooled, w1, b1, w2, b2) -> torch.Tensor:
    return torch.sigmoid(F.linear(F.silu(F.linear(pooled, w1, b1)), w2, b2))


@pytest.mark.parametrize("c,s", ((4, 4), (772, 20), (3840, 256), (64, 8)))
def test_float32_se_gate_is_within_the_bound(c: int, s: int) -> None:
    ops = _se(c, s)
    want, bound = se_gate_reference(*ops)
    ratio = mb.assert_within_bound(_se_f32(*ops), want, bound, f"torch float32 SE gate C {c} S {s}")
    print(f"SE gate C {c} S {s}: torch float32 uses {ratio:.3f} of the bound")
    want0, bound0 = se_gate_reference(ops[0], ops[1], None, ops[3], None)
    mb.assert_within_bound(_se_f32(ops[0], ops[1], None, ops[3], None), want0, bound0)


def test_float32_se_gate_is_within_the_exact_fc1_bound() -> None:
    for c, s in ((772, 20), (3840, 256)):
        ops = _se(c, s, fc1_exact=True)
        want, bound = se_gate_reference(*ops, fc1_exact=True)
        ratio = mb.assert_within_bound(_se_f32(*ops), want, bound, f"torch float32 SE gate C {c} S {s}, exact fc1")
        print(f"SE gate C {c} S {s}, exact fc1: torch float32 uses {ratio:.3f} of the bound")


@pytest.mark.parametrize("c,s,fc1_exact", ((64, 8, False), (772, 20, True), (3840, 256, True)))
def test_se_gate_faults_leave_the_bound(c: int, s: int, fc1_exact: bool) -> None:
    """With real operands the fc1 term of the bound, (C + 2) 2^-23 (|p| |W1|^T + |b1|), is a worst case that grows with C
    and hides a dropped chunk from C of several hundred on; there the operands with an exact fc1 are the sensitive form."""
    pooled, w1, b1, w2, b2 = _se(c, s, fc1_exact)
    want, bound = se_gate_reference(pooled, w1, b1, w2, b2, fc1_exact=fc1_exact)
    # a 16-byte chunk of a row of w2 dropped: that channel's gate, every image
    for ch, chunk in ((0, 0), (c // 2, s // 4 - 1)):
        bad = w2.clone()
        bad[ch, chunk * 4 : chunk * 4 + 4] = 0.0
        out = _outside(_se_f32(pooled, w1, b1, bad, b2), want, bound)
        assert out[:, ch].double().mean() > 0.6, (c, s, ch, chunk)  # three images: two of them at least
        out[:, ch] = False
        assert not out.any()
    # a 16-byte chunk of a row of w1 dropped: one squeezed value, which every gate reads
    bad = w1.clone()
    bad[s // 2, 8:12] = 0.0
    out = _outside(_se_f32(pooled, bad, b1, w2, b2), want, bound)
    # ... each through ONE weight of its w2 row, and not at all for an image whose squeezed value sits where SiLU is
    # flat: the evaluation leaves the bound, in a good part of the gates of at least one image
    with pytest.raises(AssertionError, match="error / bound"):
        mb.assert_within_bound(_se_f32(pooled, bad, b1, w2, b2), want, bound)
    per_image = out.double().mean(dim=1)
    assert float(per_image.max()) > 0.25, per_image.tolist()
    # image 0 from the pooled vector of image 1
    wrong = _se_f32(pooled, w1, b1, w2, b2)
    wrong[0] = wrong[1]
    out = _outside(wrong, want, bound)
    assert out[0].double().mean() > 0.9 and not out[1:].any()


# --------------------------------------------------------------------------------------------------------------- head
def _head(hw: tuple[int, int], c: int, e: int):
    g = torch.Generator().manual_seed(hw[0] * hw[1] + c + e)
    x = torch.randn(3, hw[0], hw[1], c, generator=g)
    w = torch.randn(e, c, generator=g) / c**0.5
    return x, w, torch.randn(e, generator=g)


@pytest.mark.parametrize("hw,c,e", (((7, 1), 4, 5), ((7, 7), 2052, 33), ((7, 7), 64, 1000), ((3, 2), 64, 8)))
def test_float32_head_is_within_the_bound(hw, c: int, e: int) -> None:
    x, w, bias = _head(hw, c, e)
    want, bound = head_reference(x, w, bias)
    got = F.linear(x.mean(dim=(1, 2)), w, bias)
    ratio = mb.assert_within_bound(got, want, bound, f"torch float32 head HW {hw} C {c} E {e}")
    print(f"head HW {hw} C {c} E {e}: torch float32 uses {ratio:.3f} of the bound")
    # a sequential sum over the positions and one division, as the kernel does it
    acc = torch.zeros(3, c)
    for i in range(hw[0] * hw[1]):
        acc = acc + x.reshape(3, -1, c)[:, i]
    mb.assert_within_bound(F.linear(acc / float(hw[0] * hw[1]), w, bias), want, bound)


@pytest.mark.parametrize("hw,c,e", (((7, 7), 2052, 33), ((7, 7), 64, 1000)))
def test_head_faults_leave_the_bound(hw, c: int, e: int) -> None:
    x, w, bias = _head(hw, c, e)
    want, bound = head_reference(x, w, bias)
    p = x.mean(dim=(1, 2))
    for row, chunk in ((0, 0), (e - 1, c // 4 - 1)):
        bad = w.clone()
        bad[row, chunk * 4 : chunk * 4 + 4] = 0.0
        out = _outside(F.linear(p, bad, bias), want, bound)
        assert out[:, row].all(), (hw, c, e, row, chunk)
        out[:, row] = False
        assert not out.any()
    wrong = p.clone()
    wrong[0] = p[1]  # image 0 from the pooled vector of its neighbour
    out = _outside(F.linear(wrong, w, bias), want, bound)
    assert out[0].double().mean() > 0.9 and not out[1:].any()
    once_more = (x.sum(dim=(1, 2)) + x[:, 0, 0]) / float(hw[0] * hw[1])  # one position added twice
    assert _outside(F.linear(once_more, w, bias), want, bound).double().mean() > 0.9


# ----------------------------------------------------------------------------------- the shared helpers themselves
def test_gemm_operands_are_the_convolution() -> None:
    g = torch.Generator().manual_seed(3)
    for cin, cout, r, s, stride, pad in ((24, 8, 5, 3, 2, 2), (32, 12, 1, 7, 1, 1), (40, 4, 1, 1, 1, 0), (8, 4, 3, 1, 1, 1)):
        x = mb.int_tensor((2, 9, 11, cin), -2, 2, g)
        w = mb.int_tensor((cout, r, s, cin), -1, 1, g)
        ref = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)
        for rows in (w, packed_k_rows(w)):
            a, w2 = gemm_operands(x, rows, r, s, stride, pad)
            assert torch.equal(a @ w2.T, ref.reshape(-1, cout))  # integers: exact in any order
        assert packed_k_rows(w).shape[1] % 32 == 0
        bad = packed_k_rows(w)
        if bad.shape[1] > r * s * cin:
            bad[0, -1] = 1.0
            with pytest.raises(AssertionError, match="tail"):
                gemm_operands(x, bad, r, s, stride, pad)


def test_guarded_output_notices() -> None:
    dev = torch.device("cpu")
    out = GuardedOutput((3, 5), dev)
    assert out.ptr % 16 == 0 and out.ptr == out.buf.data_ptr() + 1024
    with pytest.raises(AssertionError, match="NaN"):
        out.result("untouched")
    out.buf[out.MARGIN : out.MARGIN + 15] = 1.0
    assert torch.equal(out.result(), torch.ones(3, 5))
    out.buf[out.MARGIN + 15] = 0.0
    with pytest.raises(AssertionError, match="after"):
        out.result()
    out = GuardedOutput((3, 5), dev)
    out.buf[out.MARGIN : out.MARGIN + 15] = 1.0
    out.buf[out.MARGIN - 1] = float("nan")  # another NaN than the canary's
    with pytest.raises(AssertionError, match="before"):
        out.result()
    out = GuardedOutput((3, 5), dev)
    out.buf[out.MARGIN : out.MARGIN + 14] = 1.0
    with pytest.raises(AssertionError, match="flat index 14"):
        out.result()
