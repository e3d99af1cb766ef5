"""References for the float32 matrix-core products that need no measured tolerance (a helper, not a conftest).

Two forms, for `out = a . w^T + bias + residual` with `a` `[M, K]` and `w` `[N, K]` float32 AS THE KERNEL SEES THEM (a
transformed operand -- `x * gate`, `x - mean` -- is formed as one float32 operation by the caller first):

1. Exact integers (`int_tensor`, `choice_tensor`, `assert_exact_range`).  Every operand is a multiple of a power of two
   (its quantum), so every product and every partial sum is a multiple of `q = qa * qw`; while all of them stay below
   2^24 q in magnitude they are float32 numbers, no addition rounds, and the result has the same bits in any summation
   order: the kernel must EQUAL the float64 product.  `assert_exact_range` checks the condition from the operands
   (max over outputs of `|a| . |w|^T + |bias| + |residual|`, which bounds every partial sum) and raises when it does not
   hold, so that a test cannot pass on operands whose sums could have rounded.  The reference for long reductions.

2. A derived element-wise bound (`product_f64`, `product_bound`, `assert_within_bound`) for real-valued operands:

       |got - want| <= (K + 2) 2^-23 (|a| . |w|^T + |bias| + |residual|)

   `want` is the float64 product.  A float32 sum of the K products plus bias and residual, in ANY order and with the
   products fused into the additions or rounded on their own, passes each term through at most K + 2 roundings of
   relative size u = 2^-24: |error| <= gamma_{K+2} S with gamma_n = n u / (1 - n u) and S the sum of magnitudes above.
   gamma_n <= 2 n u while n u <= 1/2, and 2^-23 = 2 u, so (K + 2) 2^-23 S covers any summation order on the matrix
   cores, with about a factor two to spare, and nothing in it is measured.  The
   bound's SENSITIVITY (that a dropped 16-byte chunk or a neighbour's gate leaves it, tests/test_matmul_bound_host.py) is
   established for K <= 1024, so `product_bound` refuses longer reductions unless the caller says `long_k=True`; those
   belong to the integer form.
"""

from __future__ import annotations

import torch
from torch import Tensor

U2 = 2.0**-23  # twice the float32 unit roundoff
MAX_BOUND_K = 1024
EXACT_LIMIT = 2.0**24


def _f64(t: Tensor | None) -> Tensor | None:
    return None if t is None else t.detach().cpu().double()


def product_f64(a: Tensor, w: Tensor, bias: Tensor | None = None, residual: Tensor | None = None) -> Tensor:
    """`a . w^T + bias + residual` in float64: `a` [M, K], `w` [N, K], `bias` [N], `residual` [M, N]."""
    want = _f64(a) @ _f64(w).T
    if bias is not None:
        want = want + _f64(bias)
    if residual is not None:
        want = want + _f64(residual).reshape(want.shape)
    return want


def magnitude_f64(a: Tensor, w: Tensor, bias: Tensor | None = None, residual: Tensor | None = None) -> Tensor:
    """`|a| . |w|^T + |bias| + |residual|`: what every partial sum of an output is bounded by."""
    return product_f64(a.abs(), w.abs(), None if bias is None else bias.abs(), None if residual is None else residual.abs())


def product_bound(a: Tensor, w: Tensor, bias: Tensor | None = None, residual: Tensor | None = None, *,
                  long_k: bool = False) -> Tensor:
    """The element-wise bound of form 2 (float64 [M, N])."""
    k = a.shape[1]
    if k > MAX_BOUND_K and not long_k:
        raise ValueError(f"the product bound is for reductions of at most {MAX_BOUND_K} terms (got {k}): use exact integers")
    return (k + 2) * U2 * magnitude_f64(a, w, bias, residual)


def worst_ratio(got: Tensor, want: Tensor, bound: Tensor) -> tuple[float, tuple[int, ...]]:
    """(largest error / bound, its index); a NaN or infinite `got` counts as infinitely wrong, 0 / 0 as 0."""
    got64 = _f64(got).reshape(want.shape)
    err = (got64 - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(got64) & ~torch.isnan(ratio), ratio, torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    index = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    return float(ratio.reshape(-1)[flat]), index


def assert_within_bound(got: Tensor, want: Tensor, bound: Tensor, what: str = "") -> float:
    """Every element of `got` within `bound` of `want`; returns the largest error / bound ratio (information only)."""
    assert tuple(got.shape) == tuple(want.shape) == tuple(bound.shape), (got.shape, want.shape, bound.shape)
    ratio, index = worst_ratio(got, want, bound)
    if not ratio <= 1.0:
        got64 = _f64(got)
        outside = int((~((got64 - want).abs() <= bound)).sum())  # a NaN is outside
        raise AssertionError(
            f"{what}: element {index} is {float(got64[index])!r}, want {float(want[index])!r}: error / bound = "
            f"{ratio:.4g} (bound {float(bound[index]):.4g}); {outside} of {want.numel()} elements outside"
        )
    return ratio


# ---------------------------------------------------------------------------------------------- exact integer operands
def int_tensor(shape: tuple[int, ...], lo: int, hi: int, gen: torch.Generator) -> Tensor:
    """float32 integers drawn uniformly from lo .. hi (both included)."""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def choice_tensor(shape: tuple[int, ...], values: tuple[float, ...], gen: torch.Generator) -> Tensor:
    """float32 values drawn uniformly from `values`."""
    table = torch.tensor(values, dtype=torch.float32)
    return table[torch.randint(0, len(values), shape, generator=gen)]


def _is_multiple(t: Tensor, q: float) -> bool:
    s = _f64(t) / q
    return bool(torch.equal(s, s.round()))


def assert_exact_range(a: Tensor, w: Tensor, bias: Tensor | None = None, residual: Tensor | None = None, *,
                       a_quantum: float = 1.0, w_quantum: float = 1.0) -> float:
    """Raise unless the product is exact in float32 in any order: `a` multiples of `a_quantum`, `w` of `w_quantum`, bias
    and residual of q = a_quantum * w_quantum (powers of two), and |a| . |w|^T + |bias| + |residual| < 2^24 q everywhere.
    Returns the largest such magnitude."""
    q = a_quantum * w_quantum
    for name, quantum in (("a_quantum", a_quantum), ("w_quantum", w_quantum)):
        mant = torch.frexp(torch.tensor(quantum, dtype=torch.float64))[0]
        if quantum <= 0 or float(mant) != 0.5:
            raise AssertionError(f"{name} = {quantum} is not a power of two")
    if not _is_multiple(a, a_quantum):
        raise AssertionError(f"a holds values that are no multiple of {a_quantum}")
    if not _is_multiple(w, w_quantum):
        raise AssertionError(f"w holds values that are no multiple of {w_quantum}")
    for name, t in (("bias", bias), ("residual", residual)):
        if t is not None and not _is_multiple(t, q):
            raise AssertionError(f"{name} holds values that are no multiple of {q}")
    top = float(magnitude_f64(a, w, bias, residual).max())
    if not top < EXACT_LIMIT * q:
        raise AssertionError(f"partial sums may reach {top}, outside the exact range of float32 (2^24 * {q})")
    return top
