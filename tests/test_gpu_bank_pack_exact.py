"""The pack kernels (`isc_bank_pack` and, through the one row body csrc/bank_pack_row.h, append / replace / project)
against the stored-state model of tests/bank_image.py: every byte of the packed image, the stored value of every element
(bit for bit where nothing but a cast or one division rounds, inside the derived bound otherwise) and `norm_bound`, the
number the search's rounding-error guard is built on, against the true norm of the bytes AS STORED.  Also the row-mask
bitmap and the packed group codes.  The C entry points are called directly (`_lib.load()`), not through EmbeddingBank --
but for the last test, which searches banks of denormal scale through it."""

from __future__ import annotations

import ctypes

import bank_image as bi
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-12
CODE = {np.dtype(np.float16): 1, np.dtype(np.float32): 2}
TYPE_IDS = [f"{np.dtype(a).name}-{np.dtype(b).name}" for a, b in bi.PACK_TYPES]


def _api():
    from imagescry_amd import _lib

    return _lib


def _perm(n: int) -> tuple[int, int]:
    mul, inv = ctypes.c_int64(), ctypes.c_int64()
    assert _api().load().isc_bank_permutation(n, mul, inv) == 0
    return mul.value, inv.value


def _rows_on_device(rows: np.ndarray, device: torch.device, offset: bool) -> tuple[torch.Tensor, int, int]:
    """(the allocation, the pointer of row 0, ldx).  `offset`: the rows start one element into the allocation and have
    three elements of another value between them -- no row is 16-byte aligned in a way the vector loads could use for
    all of them, and the padding must not be read."""
    n, d = rows.shape
    t = torch.from_numpy(np.ascontiguousarray(rows)).to(device)
    if not offset:
        return t, t.data_ptr(), d
    buf = torch.full((1 + n * (d + 3),), 77.0, dtype=t.dtype, device=device)
    view = buf[1:].view(n, d + 3)
    view[:, :d] = t
    assert view.data_ptr() % 16 != 0
    return buf, view.data_ptr(), d + 3


def _pack(device: torch.device, rows: np.ndarray, out_dtype, normalize: bool, *, n_total: int | None = None,
          first_row: int = 0, image: torch.Tensor | None = None, nb: torch.Tensor | None = None,
          offset: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """One isc_bank_pack call into `image` (a new one, prefilled with 0xA5 and zero padding rows, when none is given);
    `nb` a zeroed norm bound when none is given."""
    api = _api()
    n, d = rows.shape
    n_total = n if n_total is None else n_total
    need = api.c_size_t()
    api.check(api.load().isc_bank_packed_bytes(CODE[np.dtype(out_dtype)], n_total, d, need), "isc_bank_packed_bytes")
    assert need.value == bi.packed_bytes(n_total, d, np.dtype(out_dtype).itemsize)
    if image is None:
        image = torch.from_numpy(bi.prefill(n_total, d, np.dtype(out_dtype).itemsize)).to(device)
    assert image.numel() == need.value
    if nb is None:
        nb = torch.zeros(1, dtype=torch.float32, device=device)
    keep, ptr, ldx = _rows_on_device(rows, device, offset)
    with torch.cuda.device(device):
        st = api.load().isc_bank_pack(ptr, CODE[rows.dtype], n, d, ldx, first_row, n_total, int(normalize), EPS,
                                      image.data_ptr(), CODE[np.dtype(out_dtype)], nb.data_ptr(),
                                      api.stream_handle(device))
    api.check(st, "isc_bank_pack")
    torch.cuda.synchronize(device)
    del keep
    return image, nb


def _decode_checked(device: torch.device, image: torch.Tensor, n: int, d: int, out_dtype) -> np.ndarray:
    """The stored rows [n, d] -- after checking every byte the rows do not own: the image must equal the model's encoding
    of those rows on the prefilled image (padding columns zero, padding rows untouched, nothing else written), and
    isc_bank_unpack must return the same rows."""
    api = _api()
    _, inv = _perm(n)
    got = image.cpu().numpy()
    esz = np.dtype(out_dtype).itemsize
    stored = bi.decode(got, n, d, out_dtype, inv)[:, :d]
    expect = bi.encode(stored, n, inv, image=bi.prefill(n, d, esz))
    assert np.array_equal(got, expect), "bytes outside the rows' own elements changed, or padding columns are not zero"
    back = torch.full((n, d + 1), 3.0, dtype=torch.float16 if esz == 2 else torch.float32, device=device)
    with torch.cuda.device(device):
        st = api.load().isc_bank_unpack(image.data_ptr(), CODE[np.dtype(out_dtype)], d, n, 0, n, back.data_ptr(), d + 1,
                                        api.stream_handle(device))
    api.check(st, "isc_bank_unpack")
    back = back.cpu().numpy()
    assert np.array_equal(np.ascontiguousarray(back[:, :d]).view(np.uint8), np.ascontiguousarray(stored).view(np.uint8))
    assert (back[:, d] == 3.0).all()
    return stored


def _check_norm_bound(nb: torch.Tensor, stored: np.ndarray, out_dtype, what: str, may_overflow: bool = False) -> float:
    got = float(nb.cpu()[0])
    d = stored.shape[1]
    esz = np.dtype(out_dtype).itemsize
    if not np.isfinite(stored.astype(np.float64)).all():
        assert got == float("inf"), f"{what}: a stored NaN / inf must make the bound +inf, got {got!r}"
        return got
    true = bi.stored_norm(stored)
    if may_overflow and got == float("inf"):
        return got
    lo, hi = bi.norm_bound_window(true, bi.ksteps(d, esz) * 128 // esz)
    print(f"{what}: norm_bound {got!r}, largest stored norm {true!r}, ratio {got / true if true else float('nan'):.9f}")
    if may_overflow:
        assert got >= true, (what, got, true)
    else:
        assert lo <= got <= hi, f"{what}: norm_bound {got!r} outside [{lo!r}, {hi!r}] (largest stored norm {true!r})"
    return got


def _cases_n(d: int) -> int:
    return 5 if d == 8192 else 257


def _special_rows(n: int, d: int, in_dtype, seed: int) -> np.ndarray:
    """Random rows with a row of zeros and rows of the values a cast treats specially."""
    rows = bi.random_rows(n, d, seed, in_dtype)
    if np.dtype(in_dtype) == np.float32:
        special = [0.0, -0.0, 6e-8, -3e-6, 2.0**-25, 1e5, -1e5, np.nan, np.inf, -np.inf, 65519.0, 65520.0, -65520.0]
    else:
        special = [0.0, -0.0, 6e-8, -3e-6, 6.1e-5, np.inf, -np.inf, np.nan, 65504.0, -65504.0]
    special = np.array(special, dtype=in_dtype)
    rows[0] = 0
    if n > 1:
        rows[1] = np.resize(special, d)
    for i, v in enumerate(special):  # one special value in an otherwise ordinary row
        if 2 + i < n:
            rows[2 + i, (5 * i) % d] = v
    return rows


@pytest.mark.parametrize("types", bi.PACK_TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("d", bi.PACK_DIMS)
def test_cast_only_image_is_bit_exact(d: int, types, device: torch.device) -> None:
    """normalize = 0: the image EQUALS the model's encoding of a torch cast of the rows, +-0, fp16 subnormals, overflow to
    +-inf, NaN and a zero row included, from aligned rows (vector loads) and from offset rows with ldx = D + 3 (scalar
    loads) alike; norm_bound is +inf for the bank that stores a NaN / inf and inside its window for the finite one."""
    in_dtype, out_dtype = types
    n = _cases_n(d)
    _, inv = _perm(n)
    esz = np.dtype(out_dtype).itemsize
    rows = _special_rows(n, d, in_dtype, 100 + d)
    finite = np.clip(np.nan_to_num(rows, nan=0.25, posinf=3.0, neginf=-3.0), -60000, 60000).astype(in_dtype)
    for name, x in (("special", rows), ("finite", finite)):
        cast = torch.from_numpy(x).to(torch.float16 if esz == 2 else torch.float32).numpy()
        expect = bi.encode(cast, n, inv, image=bi.prefill(n, d, esz))
        image, nb = _pack(device, x, out_dtype, False)
        assert np.array_equal(image.cpu().numpy(), expect), name
        image2, nb2 = _pack(device, x, out_dtype, False, offset=True)
        assert torch.equal(image, image2), name
        assert torch.equal(nb.view(torch.int32), nb2.view(torch.int32))
        stored = _decode_checked(device, image, n, d, out_dtype)
        got = _check_norm_bound(nb, stored, out_dtype, f"{name} d={d} {TYPE_IDS[bi.PACK_TYPES.index(types)]}")
        if name == "special" and n > 1:
            assert got == float("inf")


@pytest.mark.parametrize("types", bi.PACK_TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("d", bi.PACK_DIMS)
def test_normalised_rows(d: int, types, device: torch.device) -> None:
    """normalize = 1: `exact_rows` are stored bit for bit as the float32 emulation says; random rows (scaled 1e-3 .. 1e3
    per row) within `pack_reference`'s derived bound, every element counted; a zero row stays zero; a float32 row of norm
    1e-14 is x / eps."""
    in_dtype, out_dtype = types
    n = _cases_n(d)
    n_exact = 2 if d == 8192 else 64
    exact = bi.exact_rows(n_exact, d, np.random.default_rng(d), in_dtype)
    tail = np.zeros((2, d), dtype=in_dtype)
    if np.dtype(in_dtype) == np.float32:
        tail[1] = 1e-14 / np.sqrt(d)
    rows = np.concatenate([exact, bi.random_rows(n - n_exact - 2, d, d, in_dtype), tail])
    assert rows.shape[0] == n
    image, nb = _pack(device, rows, out_dtype, True)
    image2, nb2 = _pack(device, rows, out_dtype, True, offset=True)
    assert torch.equal(image, image2) and torch.equal(nb.view(torch.int32), nb2.view(torch.int32))
    stored = _decode_checked(device, image, n, d, out_dtype)
    assert np.array_equal(stored[:n_exact].view(np.uint8), bi.exact_pack(exact, EPS, out_dtype).view(np.uint8))
    want, bound = bi.pack_reference(rows, True, EPS, out_dtype)
    ratio = np.abs(stored.astype(np.float64) - want) / bound
    print(f"d={d} {TYPE_IDS[bi.PACK_TYPES.index(types)]}: worst error / bound {ratio.max():.4f}")
    assert (ratio <= 1.0).all(), np.unravel_index(ratio.argmax(), ratio.shape)
    assert not stored[n - 2].view(np.uint8).any()
    if np.dtype(in_dtype) == np.float32:
        assert np.allclose(stored[n - 1].astype(np.float64), 1e-2 / np.sqrt(d), rtol=2e-3, atol=0)
    _check_norm_bound(nb, stored, out_dtype, f"normalised d={d}")


@pytest.mark.parametrize("types", bi.PACK_TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("n", bi.PACK_ROWS)
def test_row_counts_and_split_calls(n: int, types, device: torch.device) -> None:
    """One row, one row short of a tile, a full tile, one row more, three tiles with a ragged end: bound, image and norm
    bound as above; the bank packed in two calls (700 rows: split at row 333) equals the bank packed in one."""
    in_dtype, out_dtype = types
    d = 100
    rows = bi.random_rows(n, d, n, in_dtype)
    image, nb = _pack(device, rows, out_dtype, True)
    stored = _decode_checked(device, image, n, d, out_dtype)
    want, bound = bi.pack_reference(rows, True, EPS, out_dtype)
    assert (np.abs(stored.astype(np.float64) - want) <= bound).all()
    _check_norm_bound(nb, stored, out_dtype, f"n={n}")
    if n > 1:
        cut = 333 if n == 700 else n // 2
        two, nb2 = _pack(device, rows[:cut], out_dtype, True, n_total=n)
        two, nb2 = _pack(device, rows[cut:], out_dtype, True, n_total=n, first_row=cut, image=two, nb=nb2)
        assert torch.equal(two, image)
        assert torch.equal(nb2.view(torch.int32), nb.view(torch.int32))


def test_norm_bound_is_an_atomic_max(device: torch.device) -> None:
    """A second call that only adds smaller rows leaves the bound as it was; one that adds a larger row raises it."""
    d, n = 129, 700
    rows = np.random.default_rng(9).standard_normal((n, d)).astype(np.float32)
    rows[333:] *= np.float32(2.0**-12)  # the largest row is in the first call
    image, nb = _pack(device, rows[:333], np.float16, False, n_total=n)
    first = nb.clone()
    image, nb = _pack(device, rows[333:], np.float16, False, n_total=n, first_row=333, image=image, nb=nb)
    assert torch.equal(nb.view(torch.int32), first.view(torch.int32))
    stored = _decode_checked(device, image, n, d, np.float16)
    _check_norm_bound(nb, stored, np.float16, "two calls")
    big = (rows[:1] * np.float32(3.0)).astype(np.float32)
    image, nb = _pack(device, big, np.float16, False, n_total=n, first_row=0, image=image, nb=nb)
    assert float(nb.cpu()[0]) > float(first.cpu()[0])
    _check_norm_bound(nb, _decode_checked(device, image, n, d, np.float16), np.float16, "after a larger row")


def test_overflowing_sum_of_squares(device: torch.device) -> None:
    """A float32 bank with entries of 1e30: the float32 sum of squares overflows; the bound is +inf or a true upper bound."""
    rows = np.full((3, 64), 1e30, dtype=np.float32)
    image, nb = _pack(device, rows, np.float32, False)
    stored = _decode_checked(device, image, 3, 64, np.float32)
    assert np.array_equal(stored, rows)
    _check_norm_bound(nb, stored, np.float32, "entries 1e30", may_overflow=True)


def _tiny_bank(kind: str, n: int, d: int) -> tuple[np.ndarray, int]:
    """(rows, the row queries should point at: the centre of the near-tie rows, else any row)."""
    centre = 0
    rng = np.random.default_rng(len(kind))
    base = rng.standard_normal((n, d))
    if kind == "squares_underflow":  # entries ~1e-25: every square is below float32's smallest subnormal
        rows = (base * 1e-25).astype(np.float32)
    elif kind == "subnormal":  # entries ~1e-40: float32 subnormals
        rows = (base * 1e-40).astype(np.float32)
    elif kind == "mixed":  # one row of ordinary scale among rows of 1e-25
        rows = (base * 1e-25).astype(np.float32)
        rows[n // 3] = (base[n // 3] / np.sqrt(d)).astype(np.float32)
    else:  # near_ties: entries of a few thousand units of 2^-149 (~1e-41), a third of the rows within +-2 units of ONE row.
        # A float32 product with a query element is rounded to a whole unit, so a float32 dot product cannot order these
        # rows: whatever a filter keeps of them, the exact scores decide -- the case the error guard exists for.
        units = np.rint(base * 3000.0)
        near = rng.choice(n, size=max(n // 3, 1), replace=False)
        centre = int(near[0])
        units[near] = units[centre] + rng.integers(-2, 3, size=(near.size, d))
        rows = (units * 2.0**-149).astype(np.float32)
        assert np.array_equal(rows.astype(np.float64), units * 2.0**-149)
    assert np.abs(rows).max() > 0
    return rows, centre


def _tiny_queries(kind: str, centre: np.ndarray, nq: int) -> np.ndarray:
    """Queries of norm about 1; for the near-tie bank they point at the rows that tie."""
    d = centre.shape[0]
    q = np.random.default_rng(3).standard_normal((nq, d)) / np.sqrt(d)
    if kind == "near_ties":
        c = centre.astype(np.float64)
        q = 0.2 * q + c / np.linalg.norm(c)
    return q.astype(np.float32)


TINY = ("squares_underflow", "subnormal", "mixed", "near_ties")


@pytest.mark.parametrize("kind", TINY)
def test_tiny_float32_banks_keep_a_true_norm_bound(kind: str, device: torch.device) -> None:
    """Banks whose squares underflow in float32: the stored bytes are the rows, and norm_bound is still an upper bound of
    the stored norms (or +inf) -- a bound of 0 would switch the search's rounding-error guard off.  (The float32 sum of
    squares alone published 0 for the first, second and fourth bank: true norms 1.0e-24, 9.9e-40, 4.1e-41.)"""
    n, d = 257, 64
    rows, _ = _tiny_bank(kind, n, d)
    image, nb = _pack(device, rows, np.float32, False)
    stored = _decode_checked(device, image, n, d, np.float32)
    assert np.array_equal(stored.view(np.uint8), rows.view(np.uint8))
    got, true = float(nb.cpu()[0]), bi.stored_norm(stored)
    print(f"{kind}: norm_bound {got!r}, largest stored norm {true!r}")
    assert got >= true > 0.0, f"{kind}: norm_bound {got!r} is below the largest stored norm {true!r}"
    if kind == "mixed":  # the ordinary row decides, inside the usual window
        _check_norm_bound(nb, stored, np.float32, kind)


def _smallest_filtered_n(d: int, q: int, k: int) -> int:
    """The smallest N for which the plan of a float32 search holds a filter level after the sample."""
    lib = _api().load()
    ends, kinds, nl = (ctypes.c_int64 * 16)(), (ctypes.c_int * 16)(), ctypes.c_int()

    def levels(n: int) -> int:
        assert lib.isc_cosine_topk_plan(2, n, d, q, k, 0, 16, nl, ends, kinds) == 0
        return nl.value

    lo, hi = k, 1 << 24  # levels(lo) == 1 < levels(hi)
    assert levels(lo) == 1 and levels(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if levels(mid) > 1 else (mid, hi)
    return hi


@pytest.mark.parametrize("kind", TINY)
def test_search_guard_on_tiny_banks(kind: str, device: torch.device) -> None:
    """The filtered search of a tiny-scale bank (the smallest bank with a filter level, 8 queries of norm ~1, k = 10)
    returns what the exhaustive search returns, bit for bit.  The three random banks are answered right with any guard
    (the filter carries more candidates than k and random scores lie far apart); on the near-tie bank 42 of the 80
    indices were wrong while norm_bound was 0 (eps = 0), 11 with a true norm_bound alone -- eps is a relative bound and the
    products' error is absolute at this scale -- and none since k_final mistrusts the filter below ||q|| max||b|| = 1e-30."""
    from imagescry_amd import EmbeddingBank

    d, nq, k = 64, 8, 10
    n = _smallest_filtered_n(d, nq, k)
    assert n < 1 << 20, n
    rows, centre = _tiny_bank(kind, n, d)
    queries = torch.from_numpy(_tiny_queries(kind, rows[centre], nq)).to(device)
    bank = EmbeddingBank(torch.from_numpy(rows).to(device), dtype=torch.float32, normalize=False)
    scores, indices = bank.search(queries, k)
    exp_s, exp_i = bank.search_exhaustive(queries, k)
    torch.cuda.synchronize(device)
    print(f"{kind}: n = {n}, norm_bound {float(bank._norm_bound.cpu()[0])!r}, "
          f"{int((indices != exp_i).sum())} of {indices.numel()} indices differ")
    assert torch.equal(indices, exp_i)
    assert torch.equal(scores.view(torch.int32), exp_s.view(torch.int32))


# ------------------------------------------------------------------------------------------- row mask and group codes
@pytest.mark.parametrize("n", [1, 255, 257, 700])
def test_row_mask_bitmap(n: int, device: torch.device) -> None:
    """isc_row_mask_pack: the bitmap equals the model, zero bits for the tile padding included, and is written entirely;
    the allowed rows are ADDED to the counter; isc_row_mask_unpack inverts it."""
    api = _api()
    lib = api.load()
    mul, _ = _perm(n)
    rng = np.random.default_rng(n)
    allow = np.where(rng.random(n) < 0.45, rng.integers(1, 256, size=n), 0).astype(np.uint8)
    allow[0] = 200
    words = torch.full((bi.mask_words(n),), 0x5A5A5A5A, dtype=torch.int32, device=device)
    count = torch.full((1,), 5, dtype=torch.int64, device=device)
    allow_dev = torch.from_numpy(allow).to(device)
    with torch.cuda.device(device):
        api.check(lib.isc_row_mask_pack(allow_dev.data_ptr(), n, words.data_ptr(), count.data_ptr(),
                                        api.stream_handle(device)), "isc_row_mask_pack")
        back = torch.full((n,), 9, dtype=torch.uint8, device=device)
        api.check(lib.isc_row_mask_unpack(words.data_ptr(), n, n, back.data_ptr(), api.stream_handle(device)),
                  "isc_row_mask_unpack")
    expect = bi.encode_mask(bi.mask_reference(allow, mul))
    got = words.cpu().numpy().view(np.uint32)
    assert got.size == expect.size == -(-n // 256) * 8
    assert np.array_equal(got, expect)
    assert not bi.decode_mask(got)[n:].any()
    assert int(count.cpu()[0]) == 5 + int((allow != 0).sum())
    assert np.array_equal(back.cpu().numpy(), (allow != 0).astype(np.uint8))


@pytest.mark.parametrize("n", [1, 255, 257, 700])
def test_row_group_codes(n: int, device: torch.device) -> None:
    """isc_row_groups_pack: code[(mul * p) mod n] at packed position p; negative codes and the padding read -2."""
    api = _api()
    mul, _ = _perm(n)
    rng = np.random.default_rng(n)
    codes = rng.integers(-5, 1000, size=n).astype(np.int32)
    codes[0] = -1
    codes[n - 1] = 2**31 - 1 if n > 1 else -7
    packed = torch.full((-(-n // 256) * 256,), 77, dtype=torch.int32, device=device)
    codes_dev = torch.from_numpy(codes).to(device)
    with torch.cuda.device(device):
        api.check(api.load().isc_row_groups_pack(codes_dev.data_ptr(), n, packed.data_ptr(), api.stream_handle(device)),
                  "isc_row_groups_pack")
    got = packed.cpu().numpy()
    assert np.array_equal(got, bi.groups_reference(codes, mul))
    assert (got[n:] == -2).all() and (got >= -2).all() and -1 not in got
