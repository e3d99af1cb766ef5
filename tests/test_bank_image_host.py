"""The stored-state model of tests/bank_image.py, checked on the host: its layout against the header's formula and against
itself, its quantiser against the model tests/test_shadow_inequality.py proves the filter inequality on, and its derived
bounds against numpy emulations of the kernels' float32 arithmetic -- the references alone meet the bounds the GPU tests
(tests/test_gpu_bank_pack_exact.py, tests/test_gpu_bank_quantize_exact.py) hold the kernels to."""

from __future__ import annotations

import ctypes

import bank_image as bi
import numpy as np
import pytest
from test_shadow_inequality import _quantise

F = np.float32


def _perm(n: int) -> tuple[int, int]:
    from imagescry_amd import _lib

    mul, inv = ctypes.c_int64(), ctypes.c_int64()
    assert _lib.load().isc_bank_permutation(n, mul, inv) == 0
    return mul.value, inv.value


# ------------------------------------------------------------------------------------------------------------ layout
def test_offsets_follow_the_header() -> None:
    """include/imagescry_hip.h: [tile][K step][row in tile][128 B] -- counted segment by segment."""
    for ks in (1, 2, 3, 5, 128):
        seg = 0
        for tile in range(3):
            for s in range(ks):
                for r in range(0, 256, 51):
                    assert bi.packed_offset(tile * 256 + r, s, ks) == ((tile * ks + s) * 256 + r) * 128
                seg += 1
        assert bi.packed_offset(3 * 256, 0, ks) == seg * 256 * 128
    assert bi.ksteps(64, 2) == 1 and bi.ksteps(65, 2) == 2 and bi.ksteps(129, 2) == 3 and bi.ksteps(129, 4) == 5
    assert bi.ksteps(8192, 2) == 128 and bi.packed_bytes(257, 100, 2) == 2 * 2 * 32768
    assert bi.shadow_ksteps(160) == 2 and bi.shadow_data_bytes(700, 160) == 3 * 2 * 32768
    assert bi.shadow_bytes(700, 160) == 3 * 2 * 32768 + 256 and bi.shadow_bytes(256 * 17, 64) == 17 * 32768 + 512
    assert bi.mask_words(257) == 16


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("n,d", [(1, 1), (255, 7), (256, 64), (257, 100), (700, 129), (5, 8192)])
def test_encode_decode_round_trip(n: int, d: int, dtype) -> None:
    rng = np.random.default_rng(n * 10007 + d)
    mul, inv = _perm(n)
    rows = rng.standard_normal((n, d)).astype(dtype)
    esz = np.dtype(dtype).itemsize
    image = bi.encode(rows, n, inv, image=bi.prefill(n, d, esz))
    back = bi.decode(image, n, d, dtype, inv)
    assert np.array_equal(back[:, :d].view(np.uint8), rows.view(np.uint8))
    assert not back[:, d:].any()  # padding columns
    by_pos = bi.decode_positions(image, d, dtype)
    assert not by_pos[n:].view(np.uint8).any()  # padding rows: as prefill left them
    orig = (np.arange(n, dtype=np.int64) * mul) % n
    assert np.array_equal(by_pos[:n, :d].view(np.uint8), rows[orig].view(np.uint8))  # position p holds row mul * p mod n
    # a scalar walk through the offset formula reads the same element
    ks = bi.ksteps(d, esz)
    for r, e in ((0, 0), (n - 1, d - 1), (n // 2, d // 2)):
        byte = e * esz
        off = bi.packed_offset((inv * r) % n, byte >> 7, ks) + (byte & 127)
        assert image[off:off + esz].tobytes() == rows[r, e].tobytes()
    # two calls write what one call writes
    if n > 1:
        cut = n // 2 - 1 if n > 3 else 1
        two = bi.encode(rows[:cut], n, inv, image=bi.prefill(n, d, esz))
        two = bi.encode(rows[cut:], n, inv, first_row=cut, image=two)
        assert np.array_equal(two, image)


def test_shadow_mask_and_group_decoders() -> None:
    n, d = 700, 160
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, size=bi.shadow_bytes(n, d), dtype=np.uint8)
    codes, recs, tail = bi.decode_shadow(buf, n, d)
    assert codes.shape == (768, 256) and recs.shape == (3, 4) and tail.size == 256 - 48
    ks8 = 2
    for p, e in ((0, 0), (699, 159), (300, 128), (767, 255)):
        off = ((p // 256 * ks8 + e // 128) * 256 + p % 256) * 128 + e % 128
        assert codes[p, e] == buf[off].view(np.int8)
    assert recs[1, 2].tobytes() == buf[bi.shadow_data_bytes(n, d) + 16 + 8:][:4].tobytes()
    mul, _ = _perm(n)
    allow = (rng.random(n) < 0.4).astype(np.uint8) * 7
    bits = bi.mask_reference(allow, mul)
    assert bits.sum() == (allow != 0).sum() and not bits[n:].any()
    words = bi.encode_mask(bits)
    assert words.size == bi.mask_words(n) and np.array_equal(bi.decode_mask(words), bits)
    for p in (0, 31, 32, 699):
        assert bool(words[p // 32] >> np.uint32(p % 32) & np.uint32(1)) == bool(allow[(mul * p) % n])
    codes_in = rng.integers(-3, 50, size=n).astype(np.int32)
    packed = bi.groups_reference(codes_in, mul)
    assert (packed[n:] == -2).all() and packed[5] == (codes_in[(mul * 5) % n] if codes_in[(mul * 5) % n] >= 0 else -2)
    assert (packed[:n] >= 0).sum() == (codes_in >= 0).sum()


# ------------------------------------------------------------------------------------------------------- quantiser
def _inequality_tiles():
    """The random and adversarial tiles of tests/test_shadow_inequality.py (same constructions, same seeds)."""
    for d in (64, 100, 768, 1024):
        rng = np.random.default_rng(d)
        for _ in range(4):
            yield rng.standard_normal((256, d)) / np.sqrt(d)
            rng.standard_normal(d)
    rng = np.random.default_rng(0)
    d = 768
    yield np.where(rng.random((256, d)) < 0.5, -1.0, 1.0) * 0.25
    rng.random(d)
    tile = (rng.integers(-100, 100, size=(256, d)) + 0.5) / 127.0
    tile[:, 0] = 1.0
    yield tile
    qsteps = rng.integers(-100, 100, size=d) + 0.5
    tile = (np.rint(rng.standard_normal((256, d)) * 30) + 0.5 * np.sign(qsteps)) / 127.0
    tile[:, 0] = 1.0
    yield tile
    tile = rng.standard_normal((256, d))
    tile[::2] *= 1e-3
    tile[1::2] *= 30.0
    yield tile


def test_quantise_reference_is_the_inequality_model() -> None:
    count = 0
    for tile in _inequality_tiles():
        h = tile.astype(np.float16)
        xi, c, e, nq = _quantise(h.astype(F))
        got, s_rows, q_rows = bi.quantise_reference(h, c)
        assert np.array_equal(got, xi)
        # the model's bounds are the records the kernel would write: inside the derived window of the exact sums
        assert np.sqrt(s_rows.max()) * bi.RECORD_LO <= float(e) <= np.sqrt(s_rows.max()) * bi.RECORD_HI
        assert np.sqrt(float(q_rows.max())) * bi.RECORD_LO <= float(nq) <= np.sqrt(float(q_rows.max())) * bi.RECORD_HI
        count += 1
    assert count == 20


@pytest.mark.parametrize("d", [64, 100, 160, 192, 768, 8192])
def test_record_windows_hold_for_the_emulated_arithmetic(d: int) -> None:
    """k_bank_quantize's record arithmetic in numpy -- a float64 running sum in the kernel's order (16 dims per thread and
    K step, eight threads combined by xor shuffles), float32(sqrt) * float32(1 + 1e-6) -- against the exact sums."""
    rng = np.random.default_rng(d)
    rows = 64 if d == 8192 else 256
    tile = (rng.standard_normal((rows, d)) * 10.0 ** rng.uniform(-2, 2)).astype(np.float16)
    mx = F(np.abs(tile.astype(F)).max())
    c = F(127.0) / mx
    xi, s_rows, q_rows = bi.quantise_reference(tile, c)
    ks8 = bi.shadow_ksteps(d)
    x64 = np.zeros((rows, ks8 * 128))
    x64[:, :d] = tile.astype(np.float64)
    xq = np.zeros((rows, ks8 * 128))
    xq[:, :d] = xi
    r = (x64 * np.float64(c) - xq).reshape(rows, ks8, 8, 16)
    q = xq.reshape(rows, ks8, 8, 16)
    rs = np.zeros((rows, 8))
    qs = np.zeros((rows, 8))
    for s8 in range(ks8):
        for j in range(16):  # (fma in the kernel: one rounding less per step than this)
            rs = rs + r[:, s8, :, j] * r[:, s8, :, j]
            qs = qs + q[:, s8, :, j] * q[:, s8, :, j]
    for off in (1, 2, 4):
        rs = rs + rs[:, np.arange(8) ^ off]
        qs = qs + qs[:, np.arange(8) ^ off]
    up = F(1.0) + F(1e-6)
    resid = F(np.sqrt(rs[:, 0].max())) * up
    qnorm = F(np.sqrt(qs[:, 0].max())) * up
    assert resid.dtype == np.float32
    for got, exact in ((resid, np.sqrt(s_rows.max())), (qnorm, np.sqrt(float(q_rows.max())))):
        ratio = float(got) / exact
        print(f"d={d}: record / exact - 1 = {ratio - 1:.4e}")
        assert bi.RECORD_LO <= ratio <= bi.RECORD_HI


# ------------------------------------------------------------------------------------------------------ stored rows
def _wave_sum(v: np.ndarray) -> np.ndarray:
    """isc_wave_sum on [rows, 64] float32: xor shuffles 32, 16, .. 1."""
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, np.arange(64) ^ off]).astype(F)
    return v[:, 0]


def _emulate_pack(rows: np.ndarray, eps: float, out_dtype, fused: bool) -> tuple[np.ndarray, np.ndarray]:
    """isc_pack_row with normalize = 1 in numpy float32, in the kernel's summation order: lane l takes elements
    l, l + 64, ..; `fused`: the multiply-add contracted (emulated through float64: the square is exact there and the sum
    rounds once to float64, once to float32 -- within 2^-53 of the fused result).  -> (stored rows, norm_bound per row)."""
    n, d = rows.shape
    x = np.zeros((n, -(-d // 64) * 64), dtype=F)
    x[:, :d] = rows.astype(F)
    acc = np.zeros((n, 64), dtype=F)
    for i in range(0, x.shape[1], 64):
        v = x[:, i:i + 64]
        acc = (acc.astype(np.float64) + v.astype(np.float64) ** 2).astype(F) if fused else (acc + v * v).astype(F)
    denom = np.maximum(np.sqrt(_wave_sum(acc)), F(eps))
    stored = (x[:, :d] / denom[:, None]).astype(F).astype(out_dtype)
    # norm bound: lane l takes 16-byte chunks l, l + 64, ..; fmaf per element
    per = 16 // np.dtype(out_dtype).itemsize
    chunks = bi.ksteps(d, np.dtype(out_dtype).itemsize) * 8
    s = np.zeros((n, -(-chunks // 64) * 64 * per), dtype=np.float64)
    s[:, :d] = stored.astype(np.float64)
    s = s.reshape(n, -1, 64, per)
    sq = np.zeros((n, 64), dtype=F)
    for c in range(s.shape[1]):
        for j in range(per):
            sq = (sq.astype(np.float64) + s[:, c, :, j] ** 2).astype(F)
    nb = (np.sqrt(_wave_sum(sq)) * (F(1.0) + F(1e-3))).astype(F)
    return stored, nb


@pytest.mark.parametrize("in_dtype,out_dtype", bi.PACK_TYPES)
@pytest.mark.parametrize("d", bi.PACK_DIMS)
def test_emulated_kernel_meets_the_pack_bound(d: int, in_dtype, out_dtype) -> None:
    """The reference alone meets the bound: the float32 emulation of the kernel, fused and not, on the random rows of the
    GPU test, every element counted; its norm bound inside the derived window."""
    n = 5 if d == 8192 else 64
    rows = bi.random_rows(n, d, d, in_dtype)
    tiny = np.zeros((1, d), dtype=in_dtype)
    if in_dtype == np.float32:
        tiny[0, :] = 1e-14 / np.sqrt(d)  # norm 1e-14 < eps: stored as x / eps
    rows = np.concatenate([rows, tiny, np.zeros((1, d), dtype=in_dtype)])
    want, bound = bi.pack_reference(rows, True, 1e-12, out_dtype)
    assert not want[-1].any() and (bound > 0).all()
    dpad = bi.ksteps(d, np.dtype(out_dtype).itemsize) * 128 // np.dtype(out_dtype).itemsize
    for fused in (False, True):
        stored, nb = _emulate_pack(rows, 1e-12, out_dtype, fused)
        ratio = np.abs(stored.astype(np.float64) - want) / bound
        print(f"d={d} {np.dtype(in_dtype).name}->{np.dtype(out_dtype).name} fused={fused}: "
              f"worst error / bound {ratio.max():.3f}")
        assert (ratio <= 1.0).all()
        assert not stored[-1].any()
        for r in range(rows.shape[0]):
            lo, hi = bi.norm_bound_window(bi.stored_norm(stored[r:r + 1]), dpad)
            assert lo <= float(nb[r]) <= hi, (r, lo, float(nb[r]), hi)


def test_pack_bound_notices_a_wrong_denominator() -> None:
    """Sensitivity: a norm taken over all but one element, or a row divided by its neighbour's norm, leaves the bound."""
    rows = bi.random_rows(16, 100, 3, np.float32)
    want, bound = bi.pack_reference(rows, True, 1e-12, np.float16)
    x = rows.astype(np.float64)
    short = x / np.sqrt((x[:, :99] ** 2).sum(axis=1))[:, None]
    assert (np.abs(short.astype(np.float16).astype(np.float64) - want) > bound).any()
    shifted = x / np.roll(np.sqrt((x ** 2).sum(axis=1)), 1)[:, None]
    assert (np.abs(shifted.astype(np.float16).astype(np.float64) - want) > bound).any()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("d", bi.PACK_DIMS)
def test_exact_rows_cannot_round(d: int, dtype) -> None:
    """For `exact_rows` the emulation in the kernel's order, fused or not, EQUALS `exact_pack`, and the float64 quotient
    rounds to the same bytes: nothing but the division and the cast rounds."""
    rows = bi.exact_rows(5 if d == 8192 else 40, d, np.random.default_rng(d), dtype)
    for out_dtype in (np.float16, np.float32):
        expect = bi.exact_pack(rows, 1e-12, out_dtype)
        for fused in (False, True):
            stored, _ = _emulate_pack(rows, 1e-12, out_dtype, fused)
            assert np.array_equal(stored.view(np.uint8), expect.view(np.uint8))
        want, bound = bi.pack_reference(rows, True, 1e-12, out_dtype)
        assert (np.abs(expect.astype(np.float64) - want) <= bound).all()
    assert (np.abs(rows.astype(np.float64)).max(axis=1) > 0).all()
