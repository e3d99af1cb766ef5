"""`isc_bank_quantize` (k_bank_quantize, csrc/bank_pack.hip) against the model of tests/bank_image.py: the int8 filter is a
superset of the fp16 filter only if the kernel IS the model tests/test_shadow_inequality.py proves the inequality on --
X = rint(x * c_t) at every position of the shadow layout, resid >= max_row ||x * c_t - X||, qnorm >= max_row ||X|| --
so every code is compared with `quantise_reference` bit for bit and every record with the exact sums inside the derived
windows (module docstring of bank_image).  The fp16 image is built by the model's `encode`, not by the pack kernel, with
the identity permutation: packed position = row, so that a test chooses what a tile holds."""

from __future__ import annotations

import bank_image as bi
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _quantize(device: torch.device, rows: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(fp16 tiles [tiles, 256, Dpad] as stored, int8 codes [tiles, 256, ks8 * 128], records [tiles, 4], the bytes after
    the last record) of the bank `rows` (float16 [n, d])."""
    from imagescry_amd import _lib

    lib = _lib.load()
    n, d = rows.shape
    image = bi.encode(rows, n, 1)
    need = _lib.c_size_t()
    _lib.check(lib.isc_bank_shadow_bytes(n, d, need), "isc_bank_shadow_bytes")
    assert need.value == bi.shadow_bytes(n, d)
    bank = torch.from_numpy(image).to(device)
    shadow = torch.full((need.value,), 0xA5, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        st = lib.isc_bank_quantize(bank.data_ptr(), n, d, shadow.data_ptr(), need.value, _lib.stream_handle(device))
    _lib.check(st, "isc_bank_quantize")
    torch.cuda.synchronize(device)
    assert np.array_equal(bank.cpu().numpy(), image)  # the bank is read only
    codes, recs, tail = bi.decode_shadow(shadow.cpu().numpy(), n, d)
    t = bi.tiles(n)
    return bi.decode_positions(image, d, np.float16).reshape(t, 256, -1), codes.reshape(t, 256, -1), recs, tail


def _check_tile(x: np.ndarray, codes: np.ndarray, rec: np.ndarray, what: str) -> None:
    """One finite tile: x float16 [256, Dpad], codes int8 [256, ks8 * 128], rec = (scale, inv_scale, resid, qnorm)."""
    scale, inv, resid, qnorm = (float(v) for v in rec)
    mx = float(np.abs(x.astype(np.float32)).max())
    if mx == 0.0:
        assert scale == 1.0 and inv == 1.0, (what, scale, inv)
    else:
        assert abs(inv * mx - 127.0) <= 127.0 * 2.0**-22, (what, inv, mx)
        assert abs(scale * 127.0 - mx) <= mx * 2.0**-22, (what, scale, mx)
    xi, s_rows, q_rows = bi.quantise_reference(x, rec[1])
    expect = np.zeros(codes.shape, dtype=np.int64)  # the absent half K step of an odd ks reads as zeros
    expect[:, :x.shape[1]] = xi
    assert np.array_equal(codes.astype(np.int64), expect), \
        f"{what}: {int((codes != expect).sum())} codes differ from rint(x * c)"
    for name, got, total in (("resid", resid, float(s_rows.max())), ("qnorm", qnorm, float(q_rows.max()))):
        root = np.sqrt(total)
        if total == 0.0:
            assert got == 0.0, (what, name, got)
            continue
        print(f"{what}: {name} / exact - 1 = {got / root - 1:.4e}")
        assert root * bi.RECORD_LO <= got <= root * bi.RECORD_HI, \
            f"{what}: {name} {got!r} against sqrt {root!r}: ratio - 1 = {got / root - 1:.4e}"


def _check_bank(rows: np.ndarray, result, what: str) -> None:
    x, codes, recs, tail = result
    n, d = rows.shape
    assert np.array_equal(x.reshape(-1, x.shape[2])[:n, :d].view(np.uint8), rows.view(np.uint8))
    assert (tail == 0xA5).all(), "bytes after the last record were written"
    assert not codes.reshape(-1, codes.shape[2])[n:].any() and not codes[:, :, d:].any()  # padding rows and columns
    for t in range(x.shape[0]):
        _check_tile(x[t], codes[t], recs[t], f"{what} tile {t}")


SHAPES = [(n, d) for d in bi.PACK_DIMS for n in bi.PACK_ROWS if d < 8192 or n <= 257]


@pytest.mark.parametrize("n,d", SHAPES)
def test_random_banks(n: int, d: int, device: torch.device) -> None:
    """Rows of unit scale times a power of ten per row; D up to 64 and 129 .. 192 have an odd number of fp16 K steps (the
    second half of the last int8 K step is absent), 100 zero-padded columns, 700 rows three tiles with a ragged end."""
    rng = np.random.default_rng(n * 10007 + d)
    rows = rng.standard_normal((n, d)) / np.sqrt(d) * 10.0 ** rng.uniform(-2, 2, size=(n, 1)).round()
    rows = rows.astype(np.float16)
    _check_bank(rows, _quantize(device, rows), f"{n}x{d}")


def _adversarial(d: int, rng: np.random.Generator) -> tuple[np.ndarray, dict[str, int]]:
    """Seven tiles chosen to break things (packed position = row); -> (rows, tile index by name)."""
    blocks, index = [], {}

    def add(name: str, block: np.ndarray) -> None:
        index[name] = len(blocks)
        blocks.append(block.astype(np.float16))

    add("all_max", np.where(rng.random((256, d)) < 0.5, -0.75, 0.75))  # every code +-127
    # mx = 127 / 128 makes c exactly 128: (k + 0.5) / 128 quantises at a tie, k even and odd
    ties = (rng.integers(-126, 126, size=(256, d)) + 0.5) / 128.0
    ties[0, 0] = 127.0 / 128.0
    add("ties", ties)
    # one huge row among tiny ones: they quantise to zero, and at 0.49 of a step everywhere the largest residual is theirs
    mixed = np.full((256, d), 0.49 * 1000.0 / 127.0)
    mixed[:, ::2] *= -1
    mixed[77] = rng.standard_normal(d) * 250.0
    mixed[77, 3] = 1000.0
    add("huge_among_tiny", mixed)
    add("zero", np.zeros((256, d)))
    add("subnormal", rng.integers(-1, 2, size=(256, d)) * 2.0**-24)  # mx = 2^-24: c = 127 * 2^24 is finite
    top = rng.standard_normal((256, d)) * 9000.0
    top[5, 1] = -65504.0
    add("fp16_max", top)
    ragged = rng.standard_normal((188, d)) * 0.01
    ragged[187, d - 1] = 0.5  # the tile's maximum in its last real row and column
    add("ragged_last", ragged)
    return np.concatenate(blocks), index


@pytest.mark.parametrize("d", [160, 768])
def test_adversarial_tiles(d: int, device: torch.device) -> None:
    rows, index = _adversarial(d, np.random.default_rng(d))
    result = _quantize(device, rows)
    _check_bank(rows, result, f"adversarial d={d}")
    x, codes, recs, _ = result
    assert (np.abs(codes[index["all_max"], :, :d]) == 127).all()
    t = index["ties"]
    assert recs[t, 1] == 128.0
    steps = x[t, :, :d].astype(np.float64) * 128.0
    assert (np.abs(steps - np.floor(steps) - 0.5) < 1e-12).sum() >= 256 * d - 1  # every value but the maximum is a tie
    assert (codes[t, :, :d].astype(np.int64) % 2 == 0).sum() >= 256 * d - 1  # ties go to the even neighbour
    t = index["huge_among_tiny"]
    xi, s_rows, q_rows = bi.quantise_reference(x[t], recs[t, 1])
    assert int(q_rows.argmax()) == 77 and int(s_rows.argmax()) != 77 and not xi[:77].any()
    t = index["zero"]
    assert not codes[t].any() and tuple(recs[t]) == (1.0, 1.0, 0.0, 0.0)
    t = index["subnormal"]
    assert recs[t, 1] == 127.0 * 2.0**24 and set(np.unique(codes[t])) == {-127, 0, 127}
    t = index["fp16_max"]
    assert codes[t, 5, 1] == -127 and recs[t, 0] == np.float32(65504.0) / np.float32(127.0)
    t = index["ragged_last"]
    assert codes[t, 187, d - 1] == 127 and not codes[t, 188:].any()


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_non_finite_tile(poison: float, device: torch.device) -> None:
    """One non-finite value in the middle tile: qnorm = +inf (every row of the tile passes the filter), all its codes zero,
    resid finite; the neighbouring tiles as in the bank without it."""
    n, d = 700, 100
    rows = (np.random.default_rng(11).standard_normal((n, d)) / 10.0).astype(np.float16)
    clean = _quantize(device, rows)
    _check_bank(rows, clean, "clean")
    bad = rows.copy()
    bad[256 + 130, 41] = poison
    x, codes, recs, tail = _quantize(device, bad)
    assert recs[1, 3] == np.float32(np.inf) and np.isfinite(recs[1, 2]) and recs[1, 2] >= 0
    assert not codes[1].any()
    assert (tail == 0xA5).all()
    for t in (0, 2):
        assert np.array_equal(codes[t], clean[1][t])
        assert np.array_equal(recs[t].view(np.uint32), clean[2][t].view(np.uint32))
        _check_tile(x[t], codes[t], recs[t], f"beside {poison} tile {t}")
