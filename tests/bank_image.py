"""A numpy model of what a packed EmbeddingBank stores (a helper, not a conftest): the packed fp16 / fp32 image, the
int8 shadow with its per-tile records, the row-mask bitmap and the packed group codes -- and exact or derived references
for the numbers in them.  Nothing here calls the library or torch; the row permutation (`mul`, `mul_inv`) is an input, taken
from the host call `isc_bank_permutation` by the tests (tests/test_capi_symbols.py checks that call).

LAYOUT (include/imagescry_hip.h, "Packed bank layout").  Rows in tiles of 256, the embedding axis in K steps of 128 bytes,
storage order [tile][K step][row in tile][128 B]; ORIGINAL row r sits at packed position (mul_inv * r) mod N, position p
holds row (mul * p) mod N.  `encode` writes through the byte-offset formula `packed_offset`; `decode_positions` reads
through a reshape of the same image: the two share no arithmetic, and tests/test_bank_image_host.py holds them against
each other.  The shadow is the same scheme with 128 int8 per K step and one record of four float32 per tile
(scale, inv_scale, resid, qnorm) after the data, the records padded to a multiple of 256 bytes.

STORED ROWS (`pack_reference`).  With `normalize` the pack kernels store  out(x_i / max(||x||, eps))  computed in
float32.  `want` is that quotient in float64 and `bound` its derived distance from what any float32 evaluation of the
kernel's kind may store; u = 2^-24 is float32's unit roundoff:

  * the sum of squares: lane l adds the squares of elements l, l + 64, ... (t = ceil(D / 64) terms at most), then six
    shuffle levels add the 64 lane sums.  A square passes through one rounding of its own (none when the multiply-add is
    contracted, but then the addition into a zero accumulator rounds in its place), t - 1 additions in its lane and six
    across lanes: t + 6 roundings at most.  Every term is non-negative, so the computed sum is  ssq (1 + a)  with
    |a| <= g / (1 - g),  g = (t + 6) u;
  * sqrtf and the division are correctly rounded: one factor (1 + d), |d| <= u, each.  max(., eps) moves a relative error
    no further than it was: when the two sides of the comparison pick different branches, eps lies between them;
  * so the float32 quotient is  want (1 + a)^(-1/2) (1 + d1)^(-1) (1 + d2),  whose distance from `want` is at most
    (g / 2 + 2 u) (1 + g + 4 u)  to second order.  g <= 134 u for D <= 8192, so the second-order part is below
    69 u * 138 u < 6e-4 u, and the relative bound used is   g / 2 + 3 u   with the third u to spare;
  * a quotient below 2^-126 is a float32 subnormal and rounds with an absolute error of 2^-150 at most;
  * the cast to the bank type adds at most half a unit in the last place of the bank type at the stored value -- nothing
    for a float32 bank.  It is evaluated at  out(|want| (1 + g / 2 + 3 u)) , which no stored value exceeds (rounding is
    monotone), so that the bound does not depend on what the kernel returned.

  |got - want| <= |want| (g / 2 + 3 u) + 2^-150 + half_ulp_out.

EXACT ROWS (`exact_rows`, `exact_pack`).  Entries m 2^e with small integers m whose squares sum to a perfect square
s^2 < 2^24: every partial sum of squares, in any order and fused or not, is an integer multiple of 4^e below 2^24 such
quanta and does not round; sqrtf(s^2 4^e) = s 2^e exactly.  What remains is one correctly rounded division and one cast:
the stored bytes must EQUAL numpy's float32 division followed by `astype`.

NORM BOUND (`norm_bound_window`).  The kernel publishes  sqrtf(sum of the stored squares) * (1 + 1e-3f)  with the sum in
float32: at most 8 ceil(Dpad / 512) <= Dpad / 64 + 8 fused multiply-adds per lane and six shuffle levels; the square root
halves the sum's relative error and adds one rounding, the product another: (Dpad / 64 + 8) u covers them, and the window
is   true 1.001 (1 - g') <= norm_bound <= true float32(1 + 1e-3) (1 + g'),  g' = (Dpad / 64 + 8) u.

SHADOW RECORDS (`quantise_reference`, `RECORD_LO`, `RECORD_HI`).  X = clip(rint(float32(x) * float32(c)), +-127): one
correctly rounded float32 product and a round-to-nearest-even, reproducible bit for bit.  float64(x) * float64(c) has
11 x 24 significant bits and subtracting an integer below 2^7 keeps it a float64: the residuals are exact.  The kernel's
records are  float32(sqrt(S)) * float32(1 + 1e-6)  with S a float64 sum of at most 8192 squares (relative error
<= 8192 * 2^-53 < 1e-12, the same for the float64 sqrt), float32(1 + 1e-6) = 1 + 9.5367e-7, and two float32 roundings of
2^-24 = 5.96e-8 each: the ratio to the exact square root lies in 1 + [8.34e-7, 1.073e-6], inside
[1 + 8e-7, 1 + 1.2e-6].
"""

from __future__ import annotations

import math

import numpy as np

TILE_ROWS = 256
KSTEP_BYTES = 128
TILE_KSTEP_BYTES = TILE_ROWS * KSTEP_BYTES
SHADOW_KSTEP_DIMS = 128
SHADOW_RECORD_BYTES = 16
U = 2.0**-24
EXACT_LIMIT = 2**24
RECORD_LO = 1.0 + 8e-7
RECORD_HI = 1.0 + 1.2e-6


# ------------------------------------------------------------------------------------------------------------ layout
def ksteps(d: int, esz: int) -> int:
    return (d * esz + KSTEP_BYTES - 1) // KSTEP_BYTES


def tiles(n: int) -> int:
    return (n + TILE_ROWS - 1) // TILE_ROWS


def packed_offset(row, kstep, ks: int):
    """Byte offset of the 128-byte segment (packed position `row`, K step `kstep`); works on ints and int64 arrays."""
    return (((row >> 8) * ks + kstep) * TILE_ROWS + (row & 255)) * KSTEP_BYTES


def packed_bytes(n: int, d: int, esz: int) -> int:
    return tiles(n) * ksteps(d, esz) * TILE_KSTEP_BYTES


def positions(first_row: int, n_rows: int, n_total: int, mul_inv: int) -> np.ndarray:
    """Packed positions of ORIGINAL rows first_row .. first_row + n_rows - 1 of an n_total-row bank."""
    return (np.arange(first_row, first_row + n_rows, dtype=np.int64) * np.int64(mul_inv)) % np.int64(n_total)


def prefill(n: int, d: int, esz: int, byte: int = 0xA5) -> np.ndarray:
    """An image as a caller hands it to the pack call: `byte` everywhere, the padding rows of the last tile zero."""
    ks = ksteps(d, esz)
    img = np.full(packed_bytes(n, d, esz), byte, dtype=np.uint8)
    for p in range(n, tiles(n) * TILE_ROWS):
        for s in range(ks):
            off = packed_offset(p, s, ks)
            img[off:off + KSTEP_BYTES] = 0
    return img


def encode(rows: np.ndarray, n_total: int, mul_inv: int, *, first_row: int = 0,
           image: np.ndarray | None = None) -> np.ndarray:
    """Write `rows` (float16 or float32 [n, d]: ORIGINAL rows first_row ..) into the packed image of an n_total-row bank
    (a new zero image when none is given): each row's K-step segments at `packed_offset`, columns d .. Dpad - 1 zero."""
    rows = np.ascontiguousarray(rows)
    assert rows.dtype in (np.float16, np.float32) and rows.ndim == 2
    n, d = rows.shape
    esz = rows.dtype.itemsize
    ks = ksteps(d, esz)
    if image is None:
        image = np.zeros(packed_bytes(n_total, d, esz), dtype=np.uint8)
    assert image.dtype == np.uint8 and image.size == packed_bytes(n_total, d, esz)
    padded = np.zeros((n, ks * KSTEP_BYTES // esz), dtype=rows.dtype)
    padded[:, :d] = rows
    seg = padded.view(np.uint8).reshape(n, ks, KSTEP_BYTES)
    pos = positions(first_row, n, n_total, mul_inv)
    off = packed_offset(pos[:, None], np.arange(ks, dtype=np.int64)[None, :], ks)
    image[off[:, :, None] + np.arange(KSTEP_BYTES, dtype=np.int64)] = seg
    return image


def decode_positions(image: np.ndarray, d: int, dtype) -> np.ndarray:
    """Every packed position of the image, padding included: [tiles * 256, Dpad] of `dtype`, row p = position p."""
    esz = np.dtype(dtype).itemsize
    ks = ksteps(d, esz)
    assert image.dtype == np.uint8 and image.size % (ks * TILE_KSTEP_BYTES) == 0
    t = image.size // (ks * TILE_KSTEP_BYTES)
    by_pos = image.reshape(t, ks, TILE_ROWS, KSTEP_BYTES).transpose(0, 2, 1, 3).reshape(t * TILE_ROWS, ks * KSTEP_BYTES)
    return np.ascontiguousarray(by_pos).view(dtype)


def decode(image: np.ndarray, n: int, d: int, dtype, mul_inv: int) -> np.ndarray:
    """The ORIGINAL rows of an n-row image with their padding columns: [n, Dpad] of `dtype`."""
    return decode_positions(image, d, dtype)[positions(0, n, n, mul_inv)]


# ------------------------------------------------------------------------------------------------------------ shadow
def shadow_ksteps(d: int) -> int:
    return (d + SHADOW_KSTEP_DIMS - 1) // SHADOW_KSTEP_DIMS


def shadow_data_bytes(n: int, d: int) -> int:
    return tiles(n) * shadow_ksteps(d) * TILE_KSTEP_BYTES


def shadow_bytes(n: int, d: int) -> int:
    return shadow_data_bytes(n, d) + (tiles(n) * SHADOW_RECORD_BYTES + 255) // 256 * 256


def decode_shadow(buf: np.ndarray, n: int, d: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(int8 codes [tiles * 256, ks8 * 128] by packed position, float32 records [tiles, 4], the bytes after them)."""
    assert buf.dtype == np.uint8 and buf.size == shadow_bytes(n, d)
    t, ks8 = tiles(n), shadow_ksteps(d)
    data = buf[:shadow_data_bytes(n, d)].reshape(t, ks8, TILE_ROWS, KSTEP_BYTES)
    codes = np.ascontiguousarray(data.transpose(0, 2, 1, 3)).reshape(t * TILE_ROWS, ks8 * KSTEP_BYTES).view(np.int8)
    rec0 = shadow_data_bytes(n, d)
    recs = buf[rec0:rec0 + t * SHADOW_RECORD_BYTES].copy().view(np.float32).reshape(t, 4)
    return codes, recs, buf[rec0 + t * SHADOW_RECORD_BYTES:]


# ------------------------------------------------------------------------------------------- row mask and group codes
def mask_words(n: int) -> int:
    return tiles(n) * (TILE_ROWS // 32)


def mask_reference(allow: np.ndarray, mul: int) -> np.ndarray:
    """bool [tiles * 256]: packed position p is allowed iff p < n and allow[(mul * p) mod n] != 0."""
    n = allow.shape[0]
    bits = np.zeros(tiles(n) * TILE_ROWS, dtype=bool)
    orig = (np.arange(n, dtype=np.int64) * np.int64(mul)) % np.int64(n)
    bits[:n] = allow[orig] != 0
    return bits


def encode_mask(bits: np.ndarray) -> np.ndarray:
    """bool per packed position -> uint32 words, bit p % 32 of word p / 32."""
    return np.packbits(bits.astype(np.uint8), bitorder="little").view("<u4")


def decode_mask(words: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)


def groups_reference(codes: np.ndarray, mul: int) -> np.ndarray:
    """int32 [tiles * 256]: codes[(mul * p) mod n] at position p, -2 for a negative code and for the padding."""
    n = codes.shape[0]
    out = np.full(tiles(n) * TILE_ROWS, -2, dtype=np.int32)
    orig = (np.arange(n, dtype=np.int64) * np.int64(mul)) % np.int64(n)
    c = codes[orig].astype(np.int32)
    out[:n] = np.where(c < 0, np.int32(-2), c)
    return out


# ------------------------------------------------------------------------------------------------ int8 quantisation
def quantise_reference(tile_f16: np.ndarray, c) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """tile_f16 [rows, dims] float16 (finite), c the tile's float32 inverse scale -> (X int64 [rows, dims], the exact
    per-row sums of squared residuals as float64 [rows] (math.fsum), the per-row sums of X^2 as int64 [rows])."""
    assert tile_f16.dtype == np.float16
    x32 = tile_f16.astype(np.float32)
    c32 = np.float32(c)
    xq = np.clip(np.rint(x32 * c32), np.float32(-127), np.float32(127))
    assert xq.dtype == np.float32
    resid = x32.astype(np.float64) * np.float64(c32) - xq.astype(np.float64)
    sq = resid * resid
    s_rows = np.array([math.fsum(row) for row in sq], dtype=np.float64)
    xi = xq.astype(np.int64)
    return xi, s_rows, (xi * xi).sum(axis=1)


# --------------------------------------------------------------------------------------------------- stored rows
def _half_ulp(mag: np.ndarray, out_dtype) -> np.ndarray:
    if np.dtype(out_dtype) == np.float32:
        return np.zeros_like(mag)
    with np.errstate(over="ignore"):
        top = mag.astype(np.float16)
    top = np.where(top.astype(np.float64) < mag, np.nextafter(top, np.float16(np.inf)), top)  # rounded UP
    return np.spacing(top).astype(np.float64) / 2


def pack_reference(rows: np.ndarray, normalize: bool, eps: float, out_dtype) -> tuple[np.ndarray, np.ndarray]:
    """(want, bound), float64 [n, d]: the stored value of every element in exact arithmetic and how far a stored value
    may lie from it (module docstring).  Without `normalize` only the cast rounds (the tests compare that case bit for
    bit against a cast of their own instead)."""
    x = rows.astype(np.float64)
    d = x.shape[1]
    if normalize:
        norm = np.sqrt(np.array([math.fsum(r) for r in x * x]))
        want = x / np.maximum(norm, np.float64(np.float32(eps)))[:, None]
        rel = (-(-d // 64) + 6) * U / 2 + 3 * U
        mag = np.abs(want) * (1 + rel)
        return want, np.abs(want) * rel + 2.0**-150 + _half_ulp(mag, out_dtype)
    return x, _half_ulp(np.abs(x), out_dtype)


PACK_DIMS = (1, 7, 64, 100, 129, 160, 192, 768, 8192)  # 100, 129: a partial chunk; 129, 160, 192: odd ks; 8192: the limit
PACK_ROWS = (1, 255, 256, 257, 700)
PACK_TYPES = ((np.float32, np.float16), (np.float16, np.float16), (np.float32, np.float32), (np.float16, np.float32))


def random_rows(n: int, d: int, seed: int, dtype) -> np.ndarray:
    """Normal rows, each scaled by 10^uniform(-3, 3): what the GPU tests normalise and what the host emulation checks the
    bound on."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    return (rng.standard_normal((n, d)) * scale).astype(dtype)


def exact_rows(n: int, d: int, rng: np.random.Generator, dtype) -> np.ndarray:
    """[n, d] rows of `dtype` whose normalisation cannot round before the division (module docstring): integers of
    magnitude <= 3, up to four entries replaced by a four-square decomposition of what the sum of squares lacks to the
    next perfect square, the row scaled by a power of two.  The property is asserted, not assumed."""
    out = np.zeros((n, d), dtype=np.float64)
    for r in range(n):
        m = rng.integers(-3, 4, size=d).astype(np.int64)
        if d >= 5:
            slots = rng.choice(d, size=4, replace=False)
            m[slots] = 0
            total = int((m * m).sum())
            s = math.isqrt(total)
            if s * s < total or s == 0:
                s += 1
            m[slots] = _four_squares(s * s - total) * rng.choice([-1, 1], size=4)
        else:  # one non-zero entry: its own square
            m[:] = 0
            m[rng.integers(0, d)] = int(rng.integers(1, 200)) * int(rng.choice([-1, 1]))
        total = int((m * m).sum())
        assert math.isqrt(total) ** 2 == total and 0 < total < EXACT_LIMIT, total
        out[r] = m.astype(np.float64) * 2.0 ** int(rng.integers(-4, 5))
    rows = out.astype(dtype)
    assert np.array_equal(rows.astype(np.float64), out)  # every entry is a number of the input type
    return rows


def _four_squares(v: int) -> np.ndarray:
    top = math.isqrt(v)
    for a in range(top, -1, -1):
        for b in range(min(a, math.isqrt(v - a * a)), -1, -1):
            rest = v - a * a - b * b
            for c in range(min(b, math.isqrt(rest)), -1, -1):
                e = rest - c * c
                f = math.isqrt(e)
                if f * f == e and f <= c:
                    return np.array([a, b, c, f], dtype=np.int64)
    raise AssertionError(v)


def exact_pack(rows: np.ndarray, eps: float, out_dtype) -> np.ndarray:
    """What the pack kernels store for `exact_rows`: the exact sum of squares, np.sqrt and the division in float32, the
    cast."""
    x32 = rows.astype(np.float32)
    ssq = (rows.astype(np.float64) ** 2).sum(axis=1)
    ssq32 = ssq.astype(np.float32)
    assert np.array_equal(ssq32.astype(np.float64), ssq)
    denom = np.maximum(np.sqrt(ssq32), np.float32(eps))
    assert denom.dtype == np.float32 and np.array_equal(denom.astype(np.float64) ** 2, ssq)
    return (x32 / denom[:, None]).astype(out_dtype)


def stored_norm(decoded: np.ndarray) -> float:
    """The largest float64 Euclidean norm of the decoded rows (finite values)."""
    x = decoded.astype(np.float64)
    return float(np.sqrt((x * x).sum(axis=1)).max())


def norm_bound_window(true: float, dpad: int) -> tuple[float, float]:
    g = (dpad / 64 + 8) * U
    return true * 1.001 * (1 - g), true * float(np.float32(1) + np.float32(1e-3)) * (1 + g)
