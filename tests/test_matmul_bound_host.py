"""CPU checks of tests/matmul_bound.py: the two references the kernel-level GPU tests of the register-staged convolution
and of the PCA fit kernels rest on.

* The derived bound holds for an honest float32 product (torch's, at K = 32, 96, 512, 1024) and is left by two planted
  faults of the size a staging bug produces: one 16-byte chunk (four elements) of one operand row dropped, and one row
  multiplied by the gate of the neighbouring image.  More than 90 % of the mutated row's outputs must fall outside.
* Integer operands stay exact at K = 32 768: the float32 Gram matrix of randint(-3, 4) rows equals the float64 one, and
  operand sets that could leave the exact range raise."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402

KS = (32, 96, 512, 1024)
IMAGES, PIXELS, COUT = 3, 40, 256  # rows of `a` are pixels of three images, gated per image


def _gated(k: int):
    g = torch.Generator().manual_seed(1000 + k)
    x = torch.randn(IMAGES, PIXELS, k, generator=g)
    gate = torch.sigmoid(torch.randn(IMAGES, 1, k, generator=g))
    w = torch.randn(COUT, k, generator=g) / k**0.5
    bias = torch.randn(COUT, generator=g)
    res = torch.randn(IMAGES * PIXELS, COUT, generator=g)
    return x, gate, w, bias, res


@pytest.mark.parametrize("k", KS)
def test_float32_product_is_within_the_bound(k: int) -> None:
    x, gate, w, bias, res = _gated(k)
    a = (x * gate).reshape(-1, k)
    want = mb.product_f64(a, w, bias, res)
    bound = mb.product_bound(a, w, bias, res)
    got = a @ w.T + bias + res
    ratio = mb.assert_within_bound(got, want, bound, f"torch float32, K = {k}")
    print(f"K = {k}: torch float32 uses {ratio:.3f} of the bound")
    # and the same through the convolution torch would run for it
    got2 = torch.nn.functional.linear(a, w, bias) + res
    mb.assert_within_bound(got2, want, bound, f"torch linear, K = {k}")


@pytest.mark.parametrize("k", KS)
def test_a_dropped_chunk_leaves_the_bound(k: int) -> None:
    x, gate, w, bias, res = _gated(k)
    a = (x * gate).reshape(-1, k)
    want = mb.product_f64(a, w, bias, res)
    bound = mb.product_bound(a, w, bias, res)
    for row, chunk in ((0, 0), (PIXELS + 7, (k // 4) // 2), (IMAGES * PIXELS - 1, k // 4 - 1)):
        bad = a.clone()
        bad[row, chunk * 4 : chunk * 4 + 4] = 0.0
        got = bad @ w.T + bias + res
        outside = ((got.double() - want).abs() > bound)[row]
        assert outside.double().mean() > 0.9, (k, row, chunk, float(outside.double().mean()))
        with pytest.raises(AssertionError, match="error / bound"):
            mb.assert_within_bound(got, want, bound)
        # every other row is untouched
        others = torch.ones(a.shape[0], dtype=torch.bool)
        others[row] = False
        mb.assert_within_bound(got[others], want[others], bound[others])


@pytest.mark.parametrize("k", KS)
def test_a_neighbours_gate_leaves_the_bound(k: int) -> None:
    x, gate, w, bias, res = _gated(k)
    a = (x * gate).reshape(-1, k)
    want = mb.product_f64(a, w, bias, res)
    bound = mb.product_bound(a, w, bias, res)
    for img in (0, 1):  # the last row of image `img` with the gate of image img + 1
        row = (img + 1) * PIXELS - 1
        bad = a.clone()
        bad[row] = x[img, PIXELS - 1] * gate[img + 1, 0]
        got = bad @ w.T + bias + res
        outside = ((got.double() - want).abs() > bound)[row]
        assert outside.double().mean() > 0.9, (k, row, float(outside.double().mean()))


def test_nan_and_shape_are_failures() -> None:
    x, gate, w, bias, res = _gated(32)
    a = (x * gate).reshape(-1, 32)
    want, bound = mb.product_f64(a, w), mb.product_bound(a, w)
    got = (a @ w.T).clone()
    got[5, 9] = float("nan")
    with pytest.raises(AssertionError, match=r"\(5, 9\)"):
        mb.assert_within_bound(got, want, bound)
    with pytest.raises(AssertionError):
        mb.assert_within_bound(got[:4], want, bound)
    with pytest.raises(ValueError):
        mb.product_bound(torch.zeros(2, 1056), torch.zeros(2, 1056))


def test_integer_gram_is_exact_at_k_32768() -> None:
    g = torch.Generator().manual_seed(7)
    rows = mb.int_tensor((24, 32768), -3, 3, g)
    top = mb.assert_exact_range(rows, rows)
    assert top <= 9 * 32768
    want = mb.product_f64(rows, rows)
    assert float(want.abs().max()) <= 1.4e5 * 2.2  # diagonal: 4 * 32768 on average
    assert torch.equal((rows @ rows.T).double(), want)
    # any summation order: chunks of the reduction axis added in reverse
    parts = [rows[:, i : i + 4096] @ rows[:, i : i + 4096].T for i in range(0, 32768, 4096)]
    acc = torch.zeros(24, 24)
    for p in reversed(parts):
        acc = acc + p
    assert torch.equal(acc.double(), want)


def test_operands_outside_the_exact_range_raise() -> None:
    g = torch.Generator().manual_seed(8)
    big = mb.int_tensor((4, 32768), -30, 30, g)
    big[0] = 30.0  # 900 * 32768 > 2^24
    with pytest.raises(AssertionError, match="exact range"):
        mb.assert_exact_range(big, big)
    a = mb.int_tensor((4, 64), -2, 2, g)
    w = mb.int_tensor((8, 64), -1, 1, g)
    gate = mb.choice_tensor((4, 64), (0.5, 1.0, 2.0), g)
    with pytest.raises(AssertionError, match="no multiple"):
        mb.assert_exact_range(a * gate, w)  # halves declared as integers
    mb.assert_exact_range(a * gate, w, mb.int_tensor((8,), -8, 8, g), a_quantum=0.5)
    with pytest.raises(AssertionError, match="no multiple"):
        mb.assert_exact_range(a, w, torch.full((8,), 0.3))
    with pytest.raises(AssertionError, match="power of two"):
        mb.assert_exact_range(a, w, a_quantum=0.3)
    # 2^24 itself is outside: 2^24 + 1 is not a float32
    one = torch.ones(1, 1)
    with pytest.raises(AssertionError, match="exact range"):
        mb.assert_exact_range(one * 2.0**12, one * 2.0**12)
    mb.assert_exact_range(one * 2.0**12, one * (2.0**12 - 1))
