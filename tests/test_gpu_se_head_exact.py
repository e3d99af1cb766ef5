"""`isc_se_gate` (k_se_gate) and `isc_pool_linear_l2norm` (k_pool_linear_l2norm) at the C ABI against float64
references with derived bounds (`se_gate_reference`, `head_reference`, tests/conv_reference.py) and, for the head, exact
integers.  No tolerance here is measured.

SE gate.  S = 4, 8, 20, 256 puts 1, 2, 8, 64 lanes along a row of w2; C = 772 is one fc1 trip of 192 16-byte vectors
plus one; B = 1 and 3 leave the second image slot of a workgroup empty; row strides above C and S (the padding holds
NaN: a read of it shows); b1 / b2 absent.  The bound's fc1 term is a worst case that grows with C, so every shape also
runs with operands whose fc1 is exact in float32 (`se_exact_fc1_operands`), where that term is zero.

Head, exact integers.  x in -3 .. 3 over HW = 1, 4, 8, 64 positions: the pooled value is an integer sum divided by a power
of two, exact; w in -1 .. 1 and a bias of multiples of 1 / HW keep every partial sum a small multiple of 1 / HW, so with
`normalize = 0` the output EQUALS the float64 result.  With `normalize = 1` (weight rows of two non-zeros and a small bias, so that
the squares stay small) the sum of squares is exact as well -- asserted -- and what rounds is the square root, the
`max(., eps)` operand and the division: at most three roundings of 2^-24, so the relative error is at most 2^-22.

Head, real operands.  HW = 7 and 49 (no power of two): the bound of `head_reference`."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
from conv_reference import GuardedOutput, head_reference, se_exact_fc1_operands, se_gate_reference  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ SE gate
def _strided(t: torch.Tensor, ld: int) -> torch.Tensor:
    """`t` [rows, n] stored with row stride `ld`, NaN in the padding."""
    store = torch.full((t.shape[0], ld), float("nan"))
    store[:, : t.shape[1]] = t
    return store


@pytest.mark.parametrize("s", (4, 8, 20, 256))
@pytest.mark.parametrize("c", (4, 772, 3840))
def test_se_gate_within_bound(c: int, s: int, device: torch.device) -> None:
    from imagescry_amd import _lib

    lib = _lib.load()
    worst = 0.0
    for b in (1, 3):
        for variant in ("dense", "strided", "nobias", "exact_fc1"):
            g = torch.Generator().manual_seed(c + 7 * s + b)
            if variant == "exact_fc1":  # fc1 exact in float32: its term of the bound is zero (sensitive at large C too)
                pooled, w1, b1, w2, b2 = se_exact_fc1_operands(b, c, s, g)
                mb.assert_exact_range(pooled, w1, b1, w_quantum=1.0 / 16 if c < 1024 else 1.0 / 64)
            else:
                pooled = torch.randn(b, c, generator=g)
                w1 = torch.randn(s, c, generator=g) / c**0.5
                w2 = torch.randn(c, s, generator=g) / s**0.5
                b1 = None if variant == "nobias" else torch.randn(s, generator=g)
                b2 = None if variant == "nobias" else torch.randn(c, generator=g)
            ld1, ld2 = (c + 4, s + 8) if variant == "strided" else (c, s)
            want, bound = se_gate_reference(pooled, w1, b1, w2, b2, fc1_exact=variant == "exact_fc1")
            dp, dw1, dw2 = pooled.to(device), _strided(w1, ld1).to(device), _strided(w2, ld2).to(device)
            db1, db2 = (None, None) if b1 is None else (b1.to(device), b2.to(device))
            out = GuardedOutput((b, c), device)
            what = f"se_gate B {b} C {c} S {s} {variant}"
            _lib.check(lib.isc_se_gate(dp.data_ptr(), b, c, dw1.data_ptr(), ld1, _lib.ptr(db1), s, dw2.data_ptr(), ld2,
                                       _lib.ptr(db2), out.ptr, _lib.stream_handle(device)), what)
            worst = max(worst, mb.assert_within_bound(out.result(what), want, bound, what))
    print(f"se_gate C {c} S {s}: error / bound = {worst:.4f}")


# --------------------------------------------------------------------------------------------------------------- head
def run_head(device, x, w, bias, normalize: int, what: str, eps: float = 1e-12) -> torch.Tensor:
    from imagescry_amd import _lib

    b, h, wd, c = x.shape
    e = w.shape[0]
    dx, dw = x.contiguous().to(device), w.contiguous().to(device)
    db = None if bias is None else bias.to(device)
    out = GuardedOutput((b, e), device)
    _lib.check(_lib.load().isc_pool_linear_l2norm(dx.data_ptr(), b, h, wd, c, dw.data_ptr(), _lib.ptr(db), e, normalize, eps,
                                                  out.ptr, _lib.stream_handle(device)), what)
    return out.result(what)


@pytest.mark.parametrize("c", (4, 2052))
@pytest.mark.parametrize("h,w", ((1, 1), (2, 2), (2, 4), (8, 8)))
def test_head_exact_integers(h: int, w: int, c: int, device: torch.device) -> None:
    hw = h * w
    for e in (1, 5, 33, 1000):
        for b in (1, 3):
            g = torch.Generator().manual_seed(hw + c + e + b)
            x = mb.int_tensor((b, h, w, c), -3, 3, g)
            p = x.reshape(b, hw, c).sum(dim=1) / hw  # exact: an integer over a power of two
            assert torch.equal(p.double(), x.double().reshape(b, hw, c).mean(dim=1))
            bias = mb.int_tensor((e,), -8 * hw, 8 * hw, g) / hw
            what = f"head B {b} HW {hw} C {c} E {e}"
            # normalize = 0, dense weights
            wt = mb.int_tensor((e, c), -1, 1, g)
            mb.assert_exact_range(p, wt, bias, a_quantum=1.0 / hw)
            got = run_head(device, x, wt, bias, 0, what)
            want = mb.product_f64(p, wt, bias)
            assert torch.equal(got.double(), want), (what, mb.worst_ratio(got, want, torch.full_like(want, 2.0**-24)))
            # normalize = 1: two non-zeros per weight row and a bias of at most 2 / HW keep the squares small
            ws = torch.zeros(e, c)
            cols = torch.stack([torch.randperm(c, generator=g)[:2] for _ in range(e)])
            ws.scatter_(1, cols, mb.choice_tensor((e, 2), (-1.0, 1.0), g))
            small = mb.int_tensor((e,), -2, 2, g) / hw
            mb.assert_exact_range(p, ws, small, a_quantum=1.0 / hw)
            feat = mb.product_f64(p, ws, small)
            assert torch.equal(run_head(device, x, ws, small, 0, what).double(), feat), what
            units = feat * hw  # integers; the squares and every partial sum of them must be float32 numbers
            assert torch.equal(units, units.round()) and float((units**2).sum(dim=1).max()) < mb.EXACT_LIMIT, what
            ss = (feat**2).sum(dim=1, keepdim=True)
            assert torch.equal(ss.float().double(), ss)
            want_n = feat / ss.sqrt().clamp_min(1e-12)
            got_n = run_head(device, x, ws, small, 1, what)
            mb.assert_within_bound(got_n, want_n, 2.0**-22 * want_n.abs(), f"{what} normalised")


@pytest.mark.parametrize("c", (4, 2052))
@pytest.mark.parametrize("h,w", ((7, 1), (7, 7)))
def test_head_within_bound(h: int, w: int, c: int, device: torch.device) -> None:
    worst = 0.0
    for e in (1, 5, 33, 1000):
        for b in (1, 3):
            g = torch.Generator().manual_seed(h * w + c + e + b)
            x = torch.randn(b, h, w, c, generator=g)
            wt = torch.randn(e, c, generator=g) / c**0.5
            bias = torch.randn(e, generator=g) if e != 5 else None
            want, bound = head_reference(x, wt, bias)
            what = f"head B {b} HW {h * w} C {c} E {e}"
            worst = max(worst, mb.assert_within_bound(run_head(device, x, wt, bias, 0, what), want, bound, what))
    print(f"head HW {h * w} C {c}: error / bound = {worst:.4f}")


def test_head_refusals(device: torch.device) -> None:
    from imagescry_amd import _lib

    lib = _lib.load()
    stream = _lib.stream_handle(device)
    x = torch.zeros(2 * 4 * 4100 + 4, device=device)
    w = torch.zeros(4096 * 4100 + 4, device=device)
    out = GuardedOutput((2, 4096), device)
    call = lib.isc_pool_linear_l2norm
    # C + E = 8196: the pooled vectors and features of two images no longer fit the 64 KiB of LDS
    assert call(x.data_ptr(), 2, 2, 2, 4100, w.data_ptr(), None, 4096, 1, 1e-12, out.ptr, stream) == _lib.ISC_ERR_UNSUPPORTED
    # x and w are read 16 bytes at a time
    assert call(x.data_ptr() + 4, 2, 2, 2, 64, w.data_ptr(), None, 8, 1, 1e-12, out.ptr, stream) == _lib.ISC_ERR_ALIGNMENT
    assert call(x.data_ptr(), 2, 2, 2, 64, w.data_ptr() + 4, None, 8, 1, 1e-12, out.ptr, stream) == _lib.ISC_ERR_ALIGNMENT
    assert call(x.data_ptr(), 2, 2, 2, 62, w.data_ptr(), None, 8, 1, 1e-12, out.ptr, stream) == _lib.ISC_ERR_UNSUPPORTED
    # nothing was launched: the output still holds what it was filled with
    torch.cuda.synchronize(device)
    assert bool(torch.isnan(out.buf[out.MARGIN : out.MARGIN + out.n]).all())
    small = GuardedOutput((2, 8), device)
    assert call(x.data_ptr(), 2, 2, 2, 64, w.data_ptr(), None, 8, 0, 1e-12, small.ptr, stream) == _lib.ISC_OK
    assert torch.equal(small.result("head of zeros"), torch.zeros(2, 8))
