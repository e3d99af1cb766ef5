"""isc_channel_stats, isc_normalize_clip (planar and channels-last), isc_resize_bilinear and isc_l2norm_channels against
the references of tests/preprocess_exact.py (whose docstring holds every derivation; tests/test_preprocess_exact_host.py
checks the references on the CPU).  Normalise and the u8 statistics are pinned bit for bit, the float32 statistics and
the L2 norm by derived bounds, bilinear by the float64 blend of the fused float32 taps under the suite's resize
tolerance.  The error / bound ratios printed here are information, not thresholds.  Every output is written into the
interior of a larger buffer filled with a NaN bit pattern, and the elements before and after it must keep that pattern.

Shapes: the normalise launches are capped at 2048 blocks x 256 threads = 524 288 work items, so 527 076 four-pixel
groups (484 x 484 planes) or 527 067 pixels (243 x 241) send a few blocks round the grid-stride loops a second time,
the last of them partial; `k_stats_final` loops over the partials from B * chunks > 256 on."""

from __future__ import annotations

import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import cases  # noqa: E402
import preprocess_exact as pe  # noqa: E402

pytestmark = pytest.mark.gpu

RESIZE_RTOL, RESIZE_ATOL = 2e-6, 1e-5  # tests/test_gpu_preprocess.py
GUARD = 64  # float32 elements on either side of an output: 256 bytes, so the interior keeps the buffer's alignment
PATTERN = 0x7FC12345  # a NaN with a payload no arithmetic produces
EPS = 1e-6
CLIPS = [(None, None), (-1.5, 2.0), (-0.5, None), (None, 0.25)]
F32 = np.float32
WORST: dict[str, float] = {}


def _note(family: str, ratio: float) -> None:
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"{family}: error / bound = {ratio:.3f} (worst so far {WORST[family]:.3f})")


# ------------------------------------------------------------------------------------------------------------ plumbing
class Guarded:
    """`n` float32 elements inside a buffer of PATTERN; `shift` moves the interior by that many floats (4 bytes each)."""

    def __init__(self, n: int, device: torch.device, shift: int = 0) -> None:
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.buf = torch.full((self.hi + GUARD,), PATTERN, dtype=torch.int32, device=device)
        self.y = self.buf[self.lo:self.hi].view(torch.float32)
        assert self.buf.data_ptr() % 256 == 0 and self.y.data_ptr() % 16 == (4 * shift) % 16

    def numpy(self) -> np.ndarray:
        """The interior, after checking that the guard elements on both sides still hold the pattern."""
        torch.cuda.synchronize()
        bits = self.buf.cpu().numpy()
        assert (bits[:self.lo] == PATTERN).all(), "elements before the output were written"
        assert (bits[self.hi:] == PATTERN).all(), "elements after the output were written"
        return bits[self.lo:self.hi].view(F32)

    def untouched(self) -> bool:
        torch.cuda.synchronize()
        return bool((self.buf == PATTERN).all())


def _misaligned(x: np.ndarray, device: torch.device) -> torch.Tensor:
    """`x` on the device as the contiguous view `buf[1:]`: a uint8 pointer off every 4-byte boundary, a float32 pointer
    4-byte but not 16-byte aligned."""
    flat = torch.empty(x.size + 1, dtype=torch.from_numpy(x).dtype, device=device)
    view = flat[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == x.itemsize
    return view


def _image(shape: tuple[int, ...], dtype: str) -> np.ndarray:
    x = cases.images_u8(shape, seed=sum(shape)).numpy()
    return x if dtype == "u8" else x.astype(F32) * F32(0.37) - F32(11.0)


def _supplied(b: int, c: int) -> list[tuple[str, np.ndarray, np.ndarray, int]]:
    """Supplied statistics: per channel, and per image (what `channel_means` of shape [B, C, 1, 1] becomes)."""
    out = [("per channel", np.linspace(20, 140, c, dtype=F32), np.linspace(40, 90, c, dtype=F32), 1)]
    if b > 1:
        out.append(("per image", np.linspace(-30, 150, b * c, dtype=F32), np.linspace(90, 35, b * c, dtype=F32), b))
    return out


def _measured(xd: torch.Tensor) -> tuple[str, np.ndarray, np.ndarray, int]:
    from imagescry_amd.transforms import _channel_stats

    mean, std = _channel_stats(xd)
    return "measured", mean.cpu().numpy(), std.cpu().numpy(), 1


def _normalize(xd: torch.Tensor, mean: np.ndarray, std: np.ndarray, stat_batch: int, lo, hi, *, nhwc4: bool = False,
               y_shift: int = 0) -> tuple[int, Guarded]:
    from imagescry_amd import _lib

    lib = _lib.load()
    b, c, h, w = xd.shape
    out = Guarded(b * h * w * 4 if nhwc4 else b * c * h * w, xd.device, y_shift)
    md, sd = torch.from_numpy(mean).to(xd.device), torch.from_numpy(std).to(xd.device)
    fn = lib.isc_normalize_clip_nhwc4 if nhwc4 else lib.isc_normalize_clip
    st = fn(xd.data_ptr(), _lib.dtype_code(xd.dtype), b, c, h, w, md.data_ptr(), sd.data_ptr(), stat_batch, EPS,
            -math.inf if lo is None else lo, math.inf if hi is None else hi, out.y.data_ptr(),
            _lib.stream_handle(xd.device))
    return st, out


def _plant_specials(x: np.ndarray) -> None:
    flat = x.reshape(-1)
    flat[[0, 5, flat.size // 2, flat.size - 1]] = [np.nan, np.inf, -np.inf, np.nan]


def _check_normalize(x: np.ndarray, xd: torch.Tensor, clips, *, nhwc4: bool) -> None:
    """Every statistic source x every clip setting: status OK, output bits equal the reference, guards untouched.  The
    statistics are measured before NaN and infinities are planted into a float32 input."""
    b, c, h, w = x.shape
    stats = _supplied(b, c) + [_measured(xd)]
    if x.dtype == np.float32:
        x = x.copy()
        _plant_specials(x)
        xd = torch.from_numpy(x).to(xd.device) if xd.data_ptr() % 16 == 0 else _misaligned(x, xd.device)
    shape = (b, h, w, 4) if nhwc4 else x.shape
    for what, mean, std, stat_batch in stats:
        for lo, hi in clips:
            st, out = _normalize(xd, mean, std, stat_batch, lo, hi, nhwc4=nhwc4)
            assert st == 0, (what, lo, hi, st)
            got = out.numpy().reshape(shape)
            want = pe.normalize_ref(x, mean, std, EPS, lo, hi, nhwc4=nhwc4)
            np.testing.assert_array_equal(got, want, err_msg=f"{what}, clip {(lo, hi)}")
            if nhwc4:
                assert not got[..., c:].view(np.int32).any(), "channels past C are not +0.0"


# --------------------------------------------------------------------------------------------------- normalise, planar
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("shape", [(3, 3, 484, 484), (9, 3, 243, 241), (5, 3, 2, 2), (2, 3, 3, 5)])
def test_normalize_planar_is_bit_exact(shape: tuple[int, ...], dtype: str, device: torch.device) -> None:
    """4-wide kernels with a second, partial sweep (527 076 vectors); the scalar kernels with an odd plane; planes that
    change inside a wave (HW = 4, per-image statistics); all four clip settings; NaN and infinities for float32."""
    from imagescry_amd import normalize_per_channel

    x = _image(shape, dtype)
    xd = torch.from_numpy(x).to(device)
    _check_normalize(x, xd, CLIPS, nhwc4=False)
    # the public call, statistics taken by the kernels themselves
    _, mean, std, _ = _measured(xd)
    got = normalize_per_channel(xd, min_value=-1.5, max_value=2.0).cpu().numpy()
    np.testing.assert_array_equal(got, pe.normalize_ref(x, mean, std, EPS, -1.5, 2.0))


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_normalize_one_pixel_is_nan_as_torch(dtype: str, device: torch.device) -> None:
    from imagescry_amd import normalize_per_channel

    x = _image((1, 1, 1, 1), dtype)
    xd = torch.from_numpy(x).to(device)
    _, mean, std, _ = _measured(xd)
    assert mean[0] == F32(x.item()) and np.isnan(std[0])
    assert torch.isnan(normalize_per_channel(xd)).all() and torch.isnan(torch.from_numpy(x).float().std())
    st, out = _normalize(xd, mean, std, 1, -3.0, 3.0)
    assert st == 0 and np.isnan(out.numpy()).all()
    st, out = _normalize(xd, mean, np.ones(1, F32), 1, None, None)  # and the smallest legal call computes
    assert st == 0
    np.testing.assert_array_equal(out.numpy(), pe.normalize_ref(x, mean, np.ones(1, F32), EPS, None, None).ravel())


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_normalize_misaligned_input_takes_the_scalar_kernels(dtype: str, device: torch.device) -> None:
    """A `buf[1:]` view is contiguous and reaches the kernels through the public API: same bits as the reference, with
    the statistics the (scalar) statistics kernels return for it."""
    from imagescry_amd import normalize_per_channel

    x = _image((2, 3, 40, 40), dtype)
    xd = _misaligned(x, device)
    _, mean, std, _ = _measured(xd)
    if dtype == "u8":
        want_mean, want_std = pe.u8_stats_exact(x)
        np.testing.assert_array_equal(mean, want_mean)
        np.testing.assert_array_equal(std, want_std)
    got = normalize_per_channel(xd, min_value=-1.5, max_value=2.0).cpu().numpy()
    np.testing.assert_array_equal(got, pe.normalize_ref(x, mean, std, EPS, -1.5, 2.0))
    _check_normalize(x, xd, CLIPS[:2], nhwc4=False)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_normalize_misaligned_output_takes_the_scalar_kernels(dtype: str, device: torch.device) -> None:
    """`y` 4-byte but not 16-byte aligned: the planar form falls back to the scalar kernel and writes the same bits."""
    x = _image((2, 3, 40, 40), dtype)
    xd = torch.from_numpy(x).to(device)
    for what, mean, std, stat_batch in _supplied(2, 3):
        st, out = _normalize(xd, mean, std, stat_batch, -1.5, 2.0, y_shift=1)
        assert st == 0
        np.testing.assert_array_equal(out.numpy().reshape(x.shape), pe.normalize_ref(x, mean, std, EPS, -1.5, 2.0),
                                      err_msg=what)


# --------------------------------------------------------------------------------------------- normalise, channels-last
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("shape", [(9, 3, 484, 484), (9, 3, 243, 241), (1, 3, 2, 6), (2, 1, 6, 6), (2, 2, 6, 6),
                                   (2, 4, 6, 6), (2, 1, 3, 5), (2, 2, 3, 5), (2, 4, 3, 5)])
def test_normalize_channels_last_is_bit_exact(shape: tuple[int, ...], dtype: str, device: torch.device) -> None:
    """`k_normalize_nhwc4_t` with 527 076 groups (the LDS tile reused on the second sweep, whose last block is partial),
    the one-pixel form with 527 067, three groups, and C = 1, 2, 4 in both forms; channels past C exactly zero."""
    x = _image(shape, dtype)
    _check_normalize(x, torch.from_numpy(x).to(device), CLIPS[:2], nhwc4=True)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_normalize_channels_last_misaligned_input_and_output(dtype: str, device: torch.device) -> None:
    """A misaligned `x` falls back to the one-pixel form with the same values; a misaligned `y` is refused with
    ISC_ERR_ALIGNMENT before anything is written."""
    from imagescry_amd import _lib

    x = _image((2, 3, 40, 40), dtype)
    _check_normalize(x, _misaligned(x, device), CLIPS[:2], nhwc4=True)
    xd = torch.from_numpy(x).to(device)
    _, mean, std, stat_batch = _supplied(2, 3)[0]
    for shift in (1, 2, 3):
        st, out = _normalize(xd, mean, std, stat_batch, None, None, nhwc4=True, y_shift=shift)
        assert st == _lib.ISC_ERR_ALIGNMENT
        assert out.untouched()


# ---------------------------------------------------------------------------------------------------------- statistics
def _stats(xd: torch.Tensor) -> tuple[int, np.ndarray, np.ndarray]:
    """isc_channel_stats into a guarded [mean | std] buffer, from a workspace of exactly the size asked for, prefilled
    with garbage and followed by bytes that must survive."""
    from imagescry_amd import _lib

    lib = _lib.load()
    b, c, h, w = xd.shape
    code = _lib.dtype_code(xd.dtype)
    need = _lib.c_size_t()
    assert lib.isc_channel_stats_workspace_bytes(code, b, c, h, w, need) == 0
    ws = torch.full((need.value + 256,), 0xA5, dtype=torch.uint8, device=xd.device)
    out = Guarded(2 * c, xd.device)
    st = lib.isc_channel_stats(xd.data_ptr(), code, b, c, h, w, out.y[:c].data_ptr(), out.y[c:].data_ptr(),
                               ws.data_ptr(), need.value, _lib.stream_handle(xd.device))
    if st != 0:
        assert out.untouched()
        return st, np.empty(0, F32), np.empty(0, F32)
    got = out.numpy()
    assert bool((ws[need.value:] == 0xA5).all()), "bytes behind the workspace were written"
    return st, got[:c], got[c:]


@functools.lru_cache(maxsize=1)
def _u8_inputs() -> dict[str, np.ndarray]:
    return pe.u8_stat_inputs()


@functools.lru_cache(maxsize=1)
def _f32_inputs() -> dict[str, np.ndarray]:
    return pe.f32_stat_inputs()


U8_NAMES = ["hw5", "hw16", "hw16383", "hw16384", "hw16400", "hw224", "items300", "items600", "one_plane", "flat8",
            "flat16", "flat1032"]
F32_NAMES = ["hw5", "hw16", "hw16383", "hw16384", "hw16400", "hw224", "items300", "items600", "one_plane", "flat8",
             "offset"]


def test_statistics_cases_are_the_ones_the_host_test_proved() -> None:
    assert set(U8_NAMES) == set(_u8_inputs()) and set(F32_NAMES) == set(_f32_inputs())


@pytest.mark.parametrize("name, misalign", [(n, False) for n in U8_NAMES] +
                         [(n, True) for n in ("hw16", "hw16384", "hw16400", "flat8")])
def test_u8_statistics_are_correctly_rounded(name: str, misalign: bool, device: torch.device) -> None:
    """Mean and unbiased std equal the exact rational values rounded once to float32: planes of 5 to 224 x 224 pixels
    around the 16 384-pixel chunk, 300 and 600 partials per channel, near-constant batches (all 255; one or ten pixels
    at 254), and a base pointer that takes the scalar path."""
    x = _u8_inputs()[name]
    xd = _misaligned(x, device) if misalign else torch.from_numpy(x).to(device)
    st, mean, std = _stats(xd)
    assert st == 0
    want_mean, want_std = pe.u8_stats_exact(x)
    np.testing.assert_array_equal(mean, want_mean, err_msg=f"mean {mean.tolist()} want {want_mean.tolist()}")
    np.testing.assert_array_equal(std, want_std, err_msg=f"std {std.tolist()} want {want_std.tolist()}")


def test_u8_statistics_do_not_depend_on_the_layout(device: torch.device) -> None:
    """The same 401 408 pixels as 8 x 224 x 224, 2 x 448 x 448, 1 x 8 x 50 176 and 64 x 56 x 112."""
    x = _u8_inputs()["one_plane"]
    want = pe.u8_stats_exact(x)
    for b, h, w in ((8, 224, 224), (2, 448, 448), (1, 8, 50176), (64, 56, 112)):
        st, mean, std = _stats(torch.from_numpy(x.reshape(b, 1, h, w)).to(device))
        assert st == 0 and mean[0] == want[0][0] and std[0] == want[1][0], (b, h, w, mean, std, want)


@pytest.mark.parametrize("name, misalign", [(n, False) for n in F32_NAMES] +
                         [(n, True) for n in ("hw16", "hw16384", "offset")])
def test_f32_statistics_are_within_the_derived_bound(name: str, misalign: bool, device: torch.device) -> None:
    """Two-pass float64 reference, bound K 2^-53 sum x^2 / (n - 1) on the variance with K counted from the kernels
    (tests/preprocess_exact.py): 4-wide and scalar (HW % 4 != 0, or a misaligned pointer) paths, mean 1e4 with std 1."""
    x = _f32_inputs()[name]
    b, _, h, w = x.shape
    vec = (h * w) % 4 == 0 and not misalign
    xd = _misaligned(x, device) if misalign else torch.from_numpy(x).to(device)
    st, mean, std = _stats(xd)
    assert st == 0
    want_mean, want_std = pe.f32_stats_ref(x)
    dm, ds = pe.f32_stats_bound(x, pe.stats_chain(b, h * w, vec))
    rm, rs = pe.worst_ratio(mean, want_mean, dm), pe.worst_ratio(std, want_std, ds)
    _note("f32 mean", rm)
    _note("f32 std", rs)
    assert rm <= 1.0 and rs <= 1.0, (mean, want_mean, dm, std, want_std, ds)


# ------------------------------------------------------------------------------------------------------------ bilinear
def _resize(x: np.ndarray, h2: int, w2: int, device: torch.device) -> tuple[int, Guarded]:
    from imagescry_amd import _lib

    p, h1, w1 = x.shape
    xd = torch.from_numpy(x).to(device)
    out = Guarded(p * h2 * w2, device)
    st = _lib.load().isc_resize_bilinear(xd.data_ptr(), _lib.dtype_code(xd.dtype), p, h1, w1, h2, w2, out.y.data_ptr(),
                                         _lib.stream_handle(device))
    return st, out


def _plane(shape: tuple[int, ...], dtype: str) -> np.ndarray:
    x = cases.images_u8(shape, seed=shape[-1]).numpy()
    return x if dtype == "u8" else x.astype(F32) * F32(0.37) - F32(11.0)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("transpose", [False, True])
def test_bilinear_source_index_is_the_fused_one(transpose: bool, dtype: str, device: torch.device) -> None:
    """3001 -> 1000 along the columns, and transposed along the rows: the one size pair known to separate
    `fmaf(scale, dst + 0.5, -0.5)` (torch's values) from the two-rounding evaluation, which the test first checks."""
    x = _plane((2, 2, 3001), dtype)  # the planes of the host test
    h2, w2 = 2, 1000
    if transpose:
        x, h2, w2 = np.ascontiguousarray(x.transpose(0, 2, 1)), 1000, 2
    want = pe.bilinear_ref(x, h2, w2, fused=True)
    other = pe.bilinear_ref(x, h2, w2, fused=False)
    tol = RESIZE_ATOL + RESIZE_RTOL * np.abs(want)
    assert len(pe.tap_disagreements(3001, 1000)) >= 1
    assert (np.abs(other - want) > 10 * tol).any(), "this input does not separate the two forms"
    st, out = _resize(x, h2, w2, device)
    assert st == 0
    got = out.numpy().reshape(want.shape).astype(np.float64)
    print(f"3001 -> 1000 ({dtype}): max |got - fused| = {np.abs(got - want).max():.3g}, "
          f"max |got - unfused| = {np.abs(got - other).max():.3g}")
    _note("bilinear 3001 -> 1000", float((np.abs(got - want) / tol).max()))
    np.testing.assert_allclose(got, want, rtol=RESIZE_RTOL, atol=RESIZE_ATOL)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("sizes", [((1, 7), (3, 5)), ((7, 1), (5, 3)), ((1, 1), (4, 6)), ((9, 11), (1, 1)),
                                   ((5, 300), (7, 257)), ((1, 1), (1, 1))])
def test_bilinear_edges(sizes, dtype: str, device: torch.device) -> None:
    """H1 = 1, W1 = 1, 1 -> N, N -> 1, and W2 = 257 (a second, one-thread block along x)."""
    (h1, w1), (h2, w2) = sizes
    x = _plane((3, h1, w1), dtype)
    st, out = _resize(x, h2, w2, device)
    assert st == 0
    np.testing.assert_allclose(out.numpy().reshape(3, h2, w2).astype(np.float64), pe.bilinear_ref(x, h2, w2),
                               rtol=RESIZE_RTOL, atol=RESIZE_ATOL)


# ------------------------------------------------------------------------------------------------------------- L2 norm
def _l2norm(x: np.ndarray, device: torch.device, in_place: bool) -> tuple[int, Guarded]:
    from imagescry_amd import _lib

    b, e, s = x.shape
    out = Guarded(x.size, device)
    if in_place:
        out.y.copy_(torch.from_numpy(x).reshape(-1))
        src = out.y
    else:
        src = torch.from_numpy(x).to(device)
    st = _lib.load().isc_l2norm_channels(src.data_ptr(), b, e, s, 1e-12, out.y.data_ptr(), _lib.stream_handle(device))
    return st, out


def _check_l2norm(x: np.ndarray, device: torch.device, in_place: bool, family: str) -> None:
    b, e, s = x.shape
    st, out = _l2norm(x, device, in_place)
    assert st == 0
    got = out.numpy().reshape(x.shape)
    want = pe.l2norm_ref(x, 1e-12)
    ratio = pe.worst_ratio(got, want, pe.l2norm_rel_bound(e, s) * np.abs(want))
    _note(family, ratio)
    assert ratio <= 1.0, (e, s, in_place)
    assert not got[want == 0].view(np.int32).any(), "a zero vector does not stay +0.0"


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("e", [1, 3, 100, 255, 257, 1000])
def test_l2norm_rows_are_within_the_derived_bound(e: int, in_place: bool, device: torch.device) -> None:
    """E below, at and past the 256 threads of a row's workgroup; a zero row and a row of norm 1e-13 < eps."""
    _check_l2norm(pe.l2_rows_input(e), device, in_place, "l2norm rows")


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("e", [1, 3, 5, 130])
def test_l2norm_spatial_is_within_the_derived_bound(e: int, in_place: bool, device: torch.device) -> None:
    """E < 4 and E % 4 != 0 (channel groups without work), S around the 64 positions of a workgroup; a zero column."""
    for s in (2, 63, 64, 65, 129):
        _check_l2norm(pe.l2_spatial_input(e, s), device, in_place, "l2norm spatial")


# -------------------------------------------------------------------------------------------------------- status codes
def test_limits_return_unsupported_and_the_largest_legal_sizes_run(device: torch.device) -> None:
    from imagescry_amd import _lib

    # isc_channel_stats: C is the grid's y dimension
    x = (np.arange(65536) % 251).astype(np.uint8).reshape(1, 65536, 1, 1)
    st, _, _ = _stats(torch.from_numpy(x).to(device))
    assert st == _lib.ISC_ERR_UNSUPPORTED
    st, mean, std = _stats(torch.from_numpy(np.ascontiguousarray(x[:, :65535])).to(device))
    assert st == 0 and np.isnan(std).all()
    np.testing.assert_array_equal(mean, x[0, :65535, 0, 0].astype(F32))
    # isc_resize_bilinear: H2 and the plane count are grid dimensions
    one = np.full((1, 1, 1), 7, dtype=np.uint8)
    st, out = _resize(one, 65536, 1, device)
    assert st == _lib.ISC_ERR_UNSUPPORTED and out.untouched()
    st, out = _resize(one, 65535, 1, device)
    assert st == 0 and (out.numpy() == 7.0).all()
    planes = (np.arange(65536) % 256).astype(np.uint8).reshape(65536, 1, 1)
    st, out = _resize(planes, 1, 1, device)
    assert st == _lib.ISC_ERR_UNSUPPORTED and out.untouched()
    st, out = _resize(planes[:65535], 1, 1, device)
    assert st == 0
    np.testing.assert_array_equal(out.numpy(), planes[:65535, 0, 0].astype(F32))
    # isc_l2norm_channels with S > 1: B is the grid's y dimension
    v = np.tile(np.array([-2.0, 0.5, 4.0, -0.25], dtype=F32), 32768).reshape(65536, 1, 2)
    st, out = _l2norm(v, device, False)
    assert st == _lib.ISC_ERR_UNSUPPORTED and out.untouched()
    st, out = _l2norm(v[:65535], device, False)
    assert st == 0
    np.testing.assert_array_equal(out.numpy(), np.sign(v[:65535]).ravel())  # squares of powers of two: exact
    st, out = _l2norm(v.reshape(65536, 2, 1), device, False)  # S == 1 has no such limit
    rows = v.reshape(65536, 2, 1)
    want = pe.l2norm_ref(rows, 1e-12)
    assert st == 0 and pe.worst_ratio(out.numpy().reshape(rows.shape), want, pe.l2norm_rel_bound(2, 1) * np.abs(want)) <= 1.0
    # the smallest legal allocations
    st, out = _l2norm(np.full((1, 1, 1), -3.0, dtype=F32), device, False)
    assert st == 0 and out.numpy()[0] == -1.0
