"""The references of tests/preprocess_exact.py prove themselves on the CPU: against the oracle, against exact integer
arithmetic, and (the bounds) against float32 / float64 emulations of the kernels' summation order.  No GPU."""

from __future__ import annotations

import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import cases  # noqa: E402
import preprocess_exact as pe  # noqa: E402

from oracle import transforms_oracle  # noqa: E402

RESIZE_RTOL, RESIZE_ATOL = 2e-6, 1e-5  # tests/test_gpu_preprocess.py


def _ulps(a: np.ndarray, b: np.ndarray) -> int:
    """Largest distance in float32 ulps between two finite float32 arrays (sign-magnitude order)."""
    def key(t):
        i = t.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b))).max())


# ----------------------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("clip", [(None, None), (-1.5, 2.0), (-0.5, None), (None, 0.25)])
def test_normalize_reference_is_the_oracle(dtype, clip) -> None:
    x = cases.images_u8((5, 3, 33, 17), seed=11)
    if dtype == torch.float32:
        x = x.float() * 0.37 - 11.0
    xf = x.float()
    lo, hi = clip
    for means, stds in ((xf.mean((0, 2, 3), keepdim=True), xf.std((0, 2, 3), keepdim=True)),
                        (torch.linspace(-1, 1, 15).reshape(5, 3, 1, 1), torch.linspace(0.5, 2, 3).reshape(1, 3, 1, 1))):
        want = transforms_oracle.normalize_per_channel(x, channel_means=means, channel_stds=stds, min_value=lo,
                                                       max_value=hi).numpy()
        mean = means.expand(-1, 3, 1, 1).reshape(-1).numpy()
        std = stds.expand(means.shape[0], 3, 1, 1).reshape(-1).numpy()
        got = pe.normalize_ref(x.numpy(), mean, std, 1e-6, lo, hi)
        assert got.shape == want.shape and _ulps(got, want) <= 1
        nhwc = pe.normalize_ref(x.numpy(), mean, std, 1e-6, lo, hi, nhwc4=True)
        np.testing.assert_array_equal(nhwc[..., :3], got.transpose(0, 2, 3, 1))
        assert not nhwc[..., 3:].any()


def test_normalize_reference_keeps_nan_and_clips_infinities() -> None:
    x = np.array([np.nan, np.inf, -np.inf, 0.0], dtype=np.float32).reshape(1, 1, 2, 2)
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    out = pe.normalize_ref(x, zero, one, 0.0, -2.0, 3.0).ravel()
    assert np.isnan(out[0]) and out[1] == 3.0 and out[2] == -2.0 and out[3] == 0.0
    out = pe.normalize_ref(x, zero, one, 0.0, None, None).ravel()
    assert np.isnan(out[0]) and out[1] == np.inf and out[2] == -np.inf


# ------------------------------------------------------------------------------------------------------- exact rounding
def test_fraction_rounding_is_correct_rounding() -> None:
    rng = np.random.default_rng(5)
    for v in rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200):
        assert pe.round_fraction_f32(Fraction(float(v))) == np.float32(v)  # a double -> float32 cast is one rounding
    tie = Fraction(2**24 + 1)  # halfway between 2^24 and 2^24 + 2: to even
    assert pe.round_fraction_f32(tie) == np.float32(2.0**24)
    assert pe.round_fraction_f32(Fraction(2**24 + 3)) == np.float32(2.0**24 + 4)
    assert pe.round_fraction_f32(Fraction(1, 2**149)) == np.float32(2.0**-149)
    assert pe.round_fraction_f32(-Fraction(1, 3)) == np.float32(-1.0 / 3.0)
    for m in (2**23, 2**23 + 1, 2**24 - 1, 12345677):  # squares of float32 numbers come back exactly
        for e in (-40, -3, 0, 7):
            f = Fraction(m) * Fraction(2) ** e
            assert pe.sqrt_fraction_f32(f * f) == np.float32(float(f))
    # just below / above the midpoint between two float32 neighbours
    m = 2**23 + 5
    mid = Fraction(2 * m + 1, 2)
    assert pe.sqrt_fraction_f32(mid * mid - Fraction(1, 2**40)) == np.float32(m)
    assert pe.sqrt_fraction_f32(mid * mid + Fraction(1, 2**40)) == np.float32(m + 1)
    assert pe.sqrt_fraction_f32(Fraction(2)) == np.float32(np.sqrt(np.float64(2.0)))


def test_exact_u8_statistics_equal_float64_on_a_high_contrast_image() -> None:
    x = cases.images_u8((16, 3, 224, 224), seed=2)
    m64, s64 = transforms_oracle.channel_stats_f64(x)
    mean, std = pe.u8_stats_exact(x.numpy())
    np.testing.assert_array_equal(mean, m64.float().numpy())
    np.testing.assert_array_equal(std, s64.float().numpy())


# ------------------------------------------------------------------------------------------- the variance finalisation
@pytest.mark.parametrize("name, channel, miss", [("flat8", 1, 17), ("flat16", 1, 6), ("flat1032", 2, -7)])
def test_plain_variance_formula_misses_near_constant_u8(name: str, channel: int, miss: int) -> None:
    """The defect, recorded without a GPU: `(q - a a / n) / (n - 1)` in float64 from exact integer sums is `miss`
    float32 ulp away from the correctly rounded std; the shifted form is not."""
    a, q, n = pe.u8_sums(pe.u8_stat_inputs()[name])[channel]
    assert a * a > 2**53
    want_mean, want_std = pe.exact_from_sums(a, q, n)
    _, plain = pe.final_f64_plain(a, q, n)
    assert pe.ulp_distance(plain, want_std) == miss and abs(miss) > 1
    mean, shifted = pe.final_f64_shifted(a, q, n)
    assert shifted == want_std and mean == want_mean


def test_shifted_variance_formula_is_exact_on_every_gpu_input() -> None:
    """What lets tests/test_gpu_preprocess_exact.py demand equality: on each of its uint8 inputs the float64
    finalisation of `k_stats_final` (shifted by rint(a / n)) rounds to the correctly rounded float32 mean and std."""
    for name, x in pe.u8_stat_inputs().items():
        for c, (a, q, n) in enumerate(pe.u8_sums(x)):
            want = pe.exact_from_sums(a, q, n)
            got = pe.final_f64_shifted(a, q, n)
            assert got[0] == want[0] and got[1] == want[1], (name, c, got, want)
    got = pe.final_f64_shifted(200, 40000, 1)  # one pixel: NaN std, as torch
    assert got[0] == 200.0 and np.isnan(got[1]) and np.isnan(pe.exact_from_sums(200, 40000, 1)[1])


# ---------------------------------------------------------------------------------------------------- f32 statistics
def test_f32_statistics_bound_holds_for_the_kernel_order() -> None:
    worst = 0.0
    for name, x in pe.f32_stat_inputs().items():
        b, _, h, w = x.shape
        want_mean, want_std = pe.f32_stats_ref(x)
        for vec in (False, True) if (h * w) % 4 == 0 else (False,):
            dm, ds = pe.f32_stats_bound(x, pe.stats_chain(b, h * w, vec))
            mean, std = pe.emulate_stats_f32(x, vec)
            rm, rs = pe.worst_ratio(mean, want_mean, dm), pe.worst_ratio(std, want_std, ds)
            assert rm <= 1.0 and rs <= 1.0, (name, vec, rm, rs)
            worst = max(worst, rm, rs)
    print(f"f32 statistics emulation: worst error / bound = {worst:.3f}")
    assert pe.stats_chain(600, 16, True) == 39 + 3 and pe.stats_chain(2, 16385, False) == 84 + 1


def test_f32_statistics_bound_notices_a_dropped_element() -> None:
    """Sensitivity: at mean 1e4, std 1 (the widest bound of the set) leaving one pixel of a channel's 65 600 out of
    the sums leaves the bound."""
    x = pe.f32_stat_inputs()["offset"]
    dm, ds = pe.f32_stats_bound(x, pe.stats_chain(x.shape[0], x.shape[2] * x.shape[3], True))
    want_mean, want_std = pe.f32_stats_ref(x)
    y = x.copy()
    y[1, :, 50, 60] = 0.0
    mean, std = pe.emulate_stats_f32(y, True)
    assert pe.worst_ratio(mean, want_mean, dm) > 1.0 and pe.worst_ratio(std, want_std, ds) > 1.0


# ----------------------------------------------------------------------------------------------------------- bilinear
@pytest.mark.parametrize("transpose", [False, True])
def test_fused_source_index_is_torch_and_unfused_is_not(transpose: bool) -> None:
    x = cases.images_u8((2, 2, 3001), seed=3001)
    h2, w2 = 2, 1000
    if transpose:
        x, h2, w2 = x.transpose(-2, -1).contiguous(), 1000, 2
    want = torch.nn.functional.interpolate(x.float().unsqueeze(0), size=(h2, w2), mode="bilinear",
                                           align_corners=False)[0].numpy()
    tol = RESIZE_ATOL + RESIZE_RTOL * np.abs(want)
    fused = pe.bilinear_ref(x.numpy(), h2, w2, fused=True)
    unfused = pe.bilinear_ref(x.numpy(), h2, w2, fused=False)
    assert (np.abs(fused - want) <= tol).all()
    bad = np.abs(unfused - want) > tol
    assert bad.any()
    where = pe.tap_disagreements(3001, 1000)
    assert len(where) >= 1 and set(np.argwhere(bad)[:, 1 if transpose else 2]) <= set(where)
    print(f"3001 -> 1000: taps differ at outputs {where.tolist()}, unfused is off by up to "
          f"{np.abs(unfused - want).max():.4g}, fused by {np.abs(fused - want).max():.3g}")


@pytest.mark.parametrize("sizes", [(1920, 500), (1000, 333), (4099, 1031), (100, 37)])
def test_ordinary_sizes_do_not_separate_the_two_forms(sizes: tuple[int, int]) -> None:
    assert len(pe.tap_disagreements(*sizes)) == 0


def test_bilinear_reference_matches_torch_on_small_edges() -> None:
    g = cases.gen(9)
    for (h1, w1), (h2, w2) in (((1, 7), (3, 5)), ((7, 1), (5, 3)), ((1, 1), (4, 6)), ((9, 11), (1, 1)), ((5, 300), (7, 257))):
        x = torch.randn(2, h1, w1, generator=g)
        want = torch.nn.functional.interpolate(x.unsqueeze(0), size=(h2, w2), mode="bilinear", align_corners=False)[0]
        got = pe.bilinear_ref(x.numpy(), h2, w2)
        np.testing.assert_allclose(got, want.numpy(), rtol=RESIZE_RTOL, atol=RESIZE_ATOL)


# ------------------------------------------------------------------------------------------------------------ L2 norm
@pytest.mark.parametrize("fused", [False, True])
def test_l2norm_bound_holds_for_the_kernel_order(fused: bool) -> None:
    worst = 0.0
    shapes = [(4, e, 1) for e in (1, 3, 100, 255, 257, 1000, 5000)] + [(2, e, s) for e in (1, 3, 5, 130) for s in (2, 65)]
    for b, e, s in shapes:
        x = pe.l2_rows_input(e) if s == 1 else pe.l2_spatial_input(e, s)
        want = pe.l2norm_ref(x, 1e-12)
        got = pe.emulate_l2norm(x, 1e-12, fused=fused)
        ratio = pe.worst_ratio(got, want, pe.l2norm_rel_bound(e, s) * np.abs(want))
        assert ratio <= 1.0, (b, e, s, ratio)
        worst = max(worst, ratio)
        zero = got[1] if s == 1 else got[0, :, 1]
        assert not zero.any()
    print(f"L2 norm emulation ({'fused' if fused else 'unfused'}): worst error / bound = {worst:.3f}")


def test_l2norm_bound_notices_a_dropped_element() -> None:
    """Sensitivity: a sum of squares that misses one of 1000 elements of ordinary size leaves the bound."""
    x = pe.l2_rows_input(1000)
    want = pe.l2norm_ref(x, 1e-12)
    y = x.copy()
    y[0, 999] = 0.0
    got = pe.emulate_l2norm(y, 1e-12, fused=True)
    got[0, 999] = want[0, 999]
    assert pe.worst_ratio(got[0], want[0], pe.l2norm_rel_bound(1000, 1) * np.abs(want[0])) > 1.0
