"""The tile end of the half-major filter loop (cosine_topk.hip: k_dots_filter, launches with several query tiles, Q > 256).

A workgroup runs the consecutive 256-row tiles of its chunk through ONE set of accumulators: whatever a tile's end leaves
in them -- the -inf of a masked row, of a row past the level's end, the INT32_MIN of the int8 form -- must be gone when
the next tile's first K step has run, and the first K step of a tile may also be its last.  The shapes are the smallest
that reach that code: more than 256 queries, and levels of several tiles per chunk, of one tile per chunk and with empty
chunks, each at one to five K steps.

Yardstick: every case is BIT IDENTICAL (`torch.equal` on scores and indices) to `search_exhaustive` with the same
arguments -- the float64 kernel of search_exact.hip -- and `last_status` shows no overflowed buffer, no redone query
and none handed to the exhaustive pass: a filter that let garbage through would still be answered right by the redo, and
hide.  Every case reads the structure it is about from isc_cosine_topk_plan."""

from __future__ import annotations

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 10
N_LONG = 150_123  # last level of 459 tiles from row 32 768 (Q = 300): 115 chunks of 4 tiles, the last tile ragged
N_SHORT = 40_123  # ... of 29 tiles: one tile per chunk, the first tile of a chunk is also its last


def _rows(n: int, d: int, device: torch.device, seed: int) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, d, device=device, dtype=torch.float32, generator=g)
    return torch.nn.functional.normalize(x, dim=1).half()


def _queries(q: int, d: int, device: torch.device, seed: int) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(q, d, device=device, dtype=torch.float32, generator=g).half()


def _plan(dtype: torch.dtype, n: int, d: int, q: int, shadow: bool) -> tuple[list[int], list[int]]:
    from imagescry_amd import _lib

    nl = ctypes.c_int()
    ends = (ctypes.c_int64 * 16)()
    kinds = (ctypes.c_int * 16)()
    st = _lib.load().isc_cosine_topk_plan(_lib.dtype_code(dtype), n, d, q, K, int(shadow), 16, nl, ends, kinds)
    _lib.check(st, "isc_cosine_topk_plan")
    return list(ends[: nl.value]), list(kinds[: nl.value])


def _check(bank, queries: torch.Tensor, nref: int | None = None, **filters) -> tuple[torch.Tensor, torch.Tensor]:
    """search == search_exhaustive (on the first `nref` queries), and the search was clean."""
    got = bank.search(queries, K, **filters)
    status = bank.last_status.cpu().tolist()
    nref = queries.shape[0] if nref is None else nref
    ref_filters = {name: v[:nref] if name == "exclude_group" else v for name, v in filters.items()}
    ref = bank.search_exhaustive(queries[:nref], K, **ref_filters)
    print("status", status)
    assert torch.equal(got[1][:nref], ref[1])
    assert torch.equal(got[0][:nref], ref[0])
    assert (status[0], status[1], status[3]) == (0, 0, 0), status
    return got


# (n, Q, plan with the shadow, plan without): isc_cosine_topk_plan does not depend on D
SHAPES = {
    "long_q300": (N_LONG, 300, ([32_768, N_LONG], [0, 2]), ([32_768, N_LONG], [0, 1])),
    "long_q1024": (N_LONG, 1024, ([16_384, 18_944, N_LONG], [0, 1, 2]), ([16_384, N_LONG], [0, 1])),
    "short_q300": (N_SHORT, 300, ([32_768, N_SHORT], [0, 2]), ([32_768, N_SHORT], [0, 1])),
}


@pytest.mark.parametrize("shadow", [True, False], ids=["int8", "fp16"])
@pytest.mark.parametrize("d", [64, 129, 200, 300])  # K steps int8 / fp16: 1 / 1 (first = last), 2 / 3, 2 / 4, 3 / 5
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tiles_of_a_chunk(shape: str, d: int, shadow: bool, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    n, q, plan_i8, plan_f16 = SHAPES[shape]
    assert _plan(torch.float16, n, d, q, shadow) == (plan_i8 if shadow else plan_f16)
    bank = EmbeddingBank(_rows(n, d, device, n % 1000 + d), dtype=torch.float16, normalize=False, shadow=shadow)
    _check(bank, _queries(q, d, device, q + d), nref=64 if q == 1024 else None)  # every query of a 300-query case
    assert (bank._shadow is not None) == shadow


def test_fp32_bank(device: torch.device) -> None:
    """D = 70: three K steps of 32 floats; four matrix instructions per accumulator and 16-byte chunk."""
    from imagescry_amd import EmbeddingBank

    assert _plan(torch.float32, N_LONG, 70, 300, False) == ([32_768, N_LONG], [0, 1])
    bank = EmbeddingBank(_rows(N_LONG, 70, device, 70).float(), dtype=torch.float32, normalize=False)
    _check(bank, _queries(300, 70, device, 71).float())


@pytest.fixture(scope="module")
def rows129(device: torch.device) -> torch.Tensor:
    return _rows(N_LONG, 129, device, 129)


def test_dense_mask(rows129: torch.Tensor, device: torch.device) -> None:
    """Every second row disallowed: every tile of every chunk writes -inf into accumulators the next tile reuses."""
    from imagescry_amd import EmbeddingBank

    assert _plan(torch.float16, N_LONG, 129, 300, False) == ([32_768, N_LONG], [0, 1])
    bank = EmbeddingBank(rows129, dtype=torch.float16, normalize=False)
    allow = torch.arange(N_LONG, device=device) % 2 == 0
    got = _check(bank, _queries(300, 129, device, 5), mask=allow)
    assert bool((got[1] % 2 == 0).all())


def test_group_exclusion(rows129: torch.Tensor, device: torch.device) -> None:
    """Two groups of alternating rows, every query excludes one: about half the rows per query."""
    from imagescry_amd import EmbeddingBank

    assert _plan(torch.float16, N_LONG, 129, 300, False) == ([32_768, N_LONG], [0, 1])
    labels = torch.arange(N_LONG, device=device) % 2
    bank = EmbeddingBank(rows129, dtype=torch.float16, normalize=False, row_groups=labels)
    exclude = torch.arange(300, device=device) % 2
    got = _check(bank, _queries(300, 129, device, 6), exclude_group=exclude)
    assert bool((got[1] % 2 != exclude[:, None]).all())


def test_row_after_a_masked_one(rows129: torch.Tensor, device: torch.device) -> None:
    """The best row of each of 16 queries is the FIRST allowed row of its tile, at a position of the lane's accumulators that
    the tile before it in the same chunk left at -inf (that position disallowed there): a -inf that survived into the
    tile would cost the query its best result.  Positions are packed ones (isc_bank_permutation); the last level's chunks
    hold four consecutive tiles from tile 128, so tiles 128 + 4 c + 1 .. + 3 have a predecessor in their chunk."""
    from imagescry_amd import EmbeddingBank, _lib

    n, d = N_LONG, 129
    ends, kinds = _plan(torch.float16, n, d, 300, False)
    assert (ends, kinds) == ([32_768, n], [0, 1])
    ntiles = -(-(n - ends[0]) // 256)
    assert -(-ntiles // 128) == 4  # tiles per chunk: 128 workgroups per query tile
    mul, inv = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().isc_bank_permutation(n, mul, inv), "isc_bank_permutation")
    pos = torch.arange(n, device=device)
    orig = (pos * mul.value) % n  # packed position -> row

    queries = _queries(300, d, device, 7)
    rows = rows129.clone()
    allow_pos = pos % 2 == 0
    best = []
    for j in range(16):
        tile = ends[0] // 256 + 4 * (5 + 6 * j) + 1 + j % 3
        off = 3 + 13 * j
        allow_pos[tile * 256 : tile * 256 + off] = False
        allow_pos[tile * 256 + off] = True
        allow_pos[(tile - 1) * 256 + off] = False
        best.append(tile * 256 + off)
    best_rows = orig[torch.tensor(best, device=device)]
    rows[best_rows] = torch.nn.functional.normalize(queries[:16].float(), dim=1).half()
    allow = torch.empty(n, dtype=torch.bool, device=device)
    allow[orig] = allow_pos
    bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
    got = _check(bank, queries, mask=allow)
    assert torch.equal(got[1][:16, 0], best_rows)
