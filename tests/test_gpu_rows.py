"""Stored-row access of `EmbeddingBank` on the GPU: `rows` (isc_bank_gather), `scores` (isc_cosine_scores), `search_rows`.

Every comparison but one is exact, on bit patterns: `rows` against the unpacked bank, `scores` against the scores
`search_exhaustive` and `search` return for the same (query, row) pairs, `search_rows` against `search` of the gathered
vectors.  The one tolerance is the `atol=1e-6` of tests/test_gpu_search.py against the float64 oracle.

Shapes: banks of 255, 257 and 513 rows laid out for exactly that many (a tile boundary at 256, a short last tile), 300 rows
in an image laid out for 513, and a 513-row bank with holes at packed positions 0, 33 (bit 1 of mask word 1), 255, 256 (the
tile boundary) and 512; D = 100 fp16 and D = 40 fp32 (two K steps, the last ragged), D = 768 fp16 (two query stages of the
score kernel: 8 + 4 K steps) and D = 280 fp32 (8 + 1 K steps, the last ragged); Q around the kernel's query group of 8 and M
around a wave's 8 rows, plus 300 (five row blocks of 64).  Row lists are shuffled and name rows twice."""

from __future__ import annotations

import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import cases  # noqa: E402

from oracle import search_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
GQ = 8  # the query-group size of k_row_scores (csrc/exact_dots.h: ISC_ST_GQ)
QS = (1, GQ - 1, GQ, GQ + 1)
MS = (1, 7, 8, 9, 300)
K = 10
# name: (rows, capacity= (None: the rows), D, bank dtype, query dtype, queries with ldq > D, holes)
BANKS = {
    "255-f16": (255, None, 100, F16, F32, False, False),
    "257-f32": (257, None, 40, F32, F16, False, False),
    "513-f16": (513, None, 100, F16, F16, True, False),
    "300in513-f32": (300, 513, 40, F32, F32, False, False),
    "257-f16-d768": (257, None, 768, F16, F32, False, False),
    "255-f32-d280": (255, None, 280, F32, F32, True, False),
    "513-f16-holes": (513, None, 100, F16, F32, False, True),
}
HOLE_POSITIONS = (0, 33, 255, 256, 512)


def _vectors(n: int, d: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=cases.gen(seed)), dim=1).to(dtype)


def _labels(n: int) -> torch.Tensor:
    return torch.randint(2, 14, (n,), generator=cases.gen(77)) * 10


def _rows_at(capacity: int, positions) -> list[int]:
    """The ORIGINAL rows stored at these packed positions of an image laid out for `capacity` rows."""
    from imagescry_amd import _lib

    mul, inv = ctypes.c_int64(), ctypes.c_int64()
    assert _lib.load().isc_bank_permutation(capacity, mul, inv) == 0
    return [(mul.value * p) % capacity for p in positions]


def _queries(nq: int, d: int, dtype: torch.dtype, wide: bool, seed: int, device: torch.device) -> torch.Tensor:
    q = (torch.randn(nq, d, generator=cases.gen(seed)) * 1.5).to(dtype).to(device)
    if not wide:
        return q
    buf = torch.full((nq, d + 24), 9.0, dtype=dtype, device=device)  # ldq = D + 24: the padding must not be read
    buf[:, :d] = q
    return buf[:, :d]


_STATE: dict[str, dict] = {}


def _state(name: str, device: torch.device) -> dict:
    """Bank `name`, built once and never changed afterwards, with what every test compares against: the unpacked rows,
    the removed rows, GQ + 1 queries, their exhaustive top-K, and the float64 oracle's scores of every (query, row)."""
    if name in _STATE:
        return _STATE[name]
    from imagescry_amd import EmbeddingBank

    n, capacity, d, dtype, q_dtype, wide, holes = BANKS[name]
    vec = _vectors(n, d, dtype, 11)
    kw = {} if capacity is None else {"capacity": capacity}
    eb = EmbeddingBank(vec.to(device), dtype=dtype, normalize=False, row_groups=_labels(n), **kw)
    gone = torch.zeros(n, dtype=torch.bool)
    if holes:
        dead = _rows_at(n, HOLE_POSITIONS) + [5, 300, 301]
        assert eb.remove(rows=dead) == len(set(dead))
        gone[dead] = True
    stored = eb.bank
    assert torch.equal(stored.cpu(), vec)  # (removed rows keep their bytes in the image: `rows` must not show them)
    q = _queries(GQ + 1, d, q_dtype, wide, 12, device)
    top = eb.search_exhaustive(q, K)
    exact = search_oracle.exact_scores(vec, q.to(dtype).cpu())  # the queries rounded to the bank dtype first
    _STATE[name] = dict(bank=eb, stored=stored, gone=gone, q=q, top=top, exact=exact, n=n)
    torch.cuda.synchronize()
    return _STATE[name]


def _row_list(st: dict, nq: int, m: int, seed: int) -> torch.Tensor:
    """`m` global row indices, shuffled: the rows of the first `nq` queries' exhaustive top-K first in line, then random
    others (drawn with replacement), removed rows among them; a list of more than one row names one twice."""
    g = cases.gen(seed)
    own = st["top"][1][:nq].flatten().unique().cpu()
    own = own[torch.randperm(own.numel(), generator=g)]
    idx = torch.cat([own, torch.randint(0, st["n"], (max(m - own.numel(), 0),), generator=g)])[:m]
    if st["gone"].any() and m >= 7:
        idx[m // 2] = int(st["gone"].nonzero()[0])  # the row at packed position 0 ...
        idx[m // 3] = int(st["gone"].nonzero()[-1])
    if m > 1:
        idx[-1] = idx[0]
    return idx[torch.randperm(m, generator=g)]


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().cpu().view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


@pytest.mark.parametrize("name", list(BANKS))
def test_rows_are_the_unpacked_rows_bit_for_bit(name: str, device: torch.device) -> None:
    st = _state(name, device)
    eb = st["bank"]
    for m in MS:
        idx = _row_list(st, GQ + 1, m, 100 + m)
        got = eb.rows(idx.to(device) if m % 2 else idx.tolist())  # a device tensor or a list
        assert got.shape == (m, eb.dim) and got.dtype == eb.dtype and got.device == eb.device
        exp = st["stored"][idx.to(device)].clone()
        exp[st["gone"][idx].to(device)] = 0  # a removed row reads as zeros
        np.testing.assert_array_equal(_bits(got), _bits(exp), err_msg=f"{name} M={m}")
    assert eb.rows([]).shape == (0, eb.dim)


def test_rows_into_an_unaligned_output_take_the_element_stores(device: torch.device) -> None:
    """`_gather_rows` into a view whose rows start at odd element offsets (ldo = D + 1, first row one element in): no
    16-byte store is possible, the bytes are the same, and the elements around the rows are not touched."""
    for name in ("255-f16", "257-f32"):
        st = _state(name, device)
        eb = st["bank"]
        idx = _row_list(st, GQ + 1, 9, 140).to(device)
        buf = torch.full((9 * (eb.dim + 1) + 1,), 7.0, dtype=eb.dtype, device=device)
        out = buf[1:].view(9, eb.dim + 1)[:, : eb.dim]
        eb._gather_rows(idx, out)
        np.testing.assert_array_equal(_bits(out), _bits(st["stored"][idx]))
        pad = buf[1:].view(9, eb.dim + 1)[:, eb.dim]
        assert float(buf[0]) == 7.0 and bool((pad == 7.0).all())


@pytest.mark.parametrize("name", list(BANKS))
def test_scores_have_the_bits_of_the_exhaustive_search_and_of_search(name: str, device: torch.device) -> None:
    st = _state(name, device)
    eb, n = st["bank"], st["n"]
    live = (~st["gone"]).to(device)
    for nq in QS:
        q = st["q"][:nq]
        idx = _row_list(st, nq, 300, 200 + nq)
        got = eb.scores(q, idx.to(device))
        assert got.shape == (nq, 300) and got.dtype == F32
        # the score of every listed row in row order (a row listed twice has one score)
        table = torch.full((nq, n), float("nan"), device=device)
        table[:, idx.to(device)] = got
        np.testing.assert_array_equal(_bits(table[:, idx.to(device)]), _bits(got))
        for what, (s, i) in (("exhaustive", (st["top"][0][:nq], st["top"][1][:nq])), ("search", eb.search(q, K))):
            np.testing.assert_array_equal(_bits(table.gather(1, i)), _bits(s), err_msg=f"{name} Q={nq} {what}")
        # against the float64 oracle, every listed row; a removed row's column is -inf
        listed = torch.zeros(n, dtype=torch.bool, device=device)
        listed[idx.to(device)] = True
        ok = (listed & live).cpu().numpy()
        np.testing.assert_allclose(table.cpu().numpy()[:, ok], st["exact"][:nq][:, ok], rtol=0, atol=1e-6)
        dead = (listed & ~live).cpu().numpy()
        assert dead.any() == bool(st["gone"].any()) and np.all(table.cpu().numpy()[:, dead] == -np.inf)
        if nq == GQ + 1:
            for m in MS[:-1]:  # the short lists: the same bits as in the long one
                short = _row_list(st, nq, m, 300 + m)
                short[0] = idx[0]
                s = eb.scores(q, short.tolist())
                assert s.shape == (nq, m)
                exp = table[:, short.to(device)]
                known = ~torch.isnan(exp)  # (rows the long list does not name: checked against the oracle alone)
                np.testing.assert_array_equal(_bits(s)[known.cpu().numpy()], _bits(exp)[known.cpu().numpy()])
                alive = (~st["gone"][short]).numpy()
                np.testing.assert_allclose(s.cpu().numpy()[:, alive], st["exact"][:nq][:, short.numpy()[alive]], rtol=0,
                                           atol=1e-6)
                assert np.all(s.cpu().numpy()[:, ~alive] == -np.inf)
    assert eb.scores(st["q"][:0], [1, 2]).shape == (0, 2) and eb.scores(st["q"], []).shape == (GQ + 1, 0)


@pytest.mark.parametrize("dtype,d", [(F16, 520), (F32, 264)])
def test_every_exact_family_gives_the_same_score_bits(dtype: torch.dtype, d: int, device: torch.device) -> None:
    """One bank, every float64 pass (csrc/exact_dots.h): the score of a (query, row) pair has the same bits from `scores`,
    `search_exhaustive`, `search_groups_exhaustive` on singleton groups, `assign_exhaustive` and `assign`; and
    `search_range` at the k-th score of `search` returns `search`'s first k bit for bit.

    257 rows: two tiles, the second holding one row.  D = 520 fp16 / 264 fp32: 9 K steps, the last ragged, so the 8-step
    stage loop runs a second, short stage, the lanes of the wave-per-candidate re-scores wrap, and the zero padding is
    summed.  9 queries / centroids: a second, partial group of 8 in the staged kernels, a third group in the list search."""
    from imagescry_amd import EmbeddingBank

    n, nq, k = 257, GQ + 1, 5
    vec = _vectors(n, d, dtype, 61)
    eb = EmbeddingBank(vec.to(device), dtype=dtype, normalize=False, row_groups=torch.arange(n))
    q = _queries(nq, d, F32 if dtype == F16 else F16, False, 62, device)
    table = eb.scores(q, torch.arange(n))  # [9, 257]: every pair
    exact = search_oracle.exact_scores(vec, q.to(dtype).cpu())
    np.testing.assert_allclose(table.cpu().numpy(), exact, rtol=0, atol=1e-6)

    s, i = eb.search_exhaustive(q, k)
    np.testing.assert_array_equal(_bits(table.gather(1, i)), _bits(s), err_msg="search_exhaustive")
    gs, gi, gl = eb.search_groups_exhaustive(q, k)
    assert torch.equal(gi, i) and torch.equal(gl, i)  # every row its own group, labelled by its index
    np.testing.assert_array_equal(_bits(gs), _bits(s), err_msg="search_groups_exhaustive")

    # the queries as centroids: per row the best of its column (score desc, ties to the lower centroid) and that entry
    best = table.max(dim=0).values
    first = torch.where(table == best, torch.arange(nq, device=device)[:, None], nq).min(dim=0).values
    for what, fn in (("assign_exhaustive", eb.assign_exhaustive), ("assign", eb.assign)):
        labels, sc = fn(q)
        assert torch.equal(labels.long(), first), what
        np.testing.assert_array_equal(_bits(sc), _bits(best), err_msg=what)

    ss, si = eb.search(q, k)
    res = eb.search_range(q, ss[:, k - 1].contiguous())
    assert bool((res.counts >= k).all())
    for qi in range(nq):
        rs, ri = res[qi]
        assert torch.equal(ri[:k], si[qi]) and torch.equal(rs[:k].view(torch.int32), ss[qi].view(torch.int32)), qi


def _drop_self(s: torch.Tensor, i: torch.Tensor, own: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """Per query the k + 1 entries without the one that names the query's own row (or without the last)."""
    s, i = s.cpu().numpy(), i.cpu().numpy()
    keep = np.ones(i.shape, dtype=bool)
    for r, o in enumerate(own.tolist()):
        hit = np.nonzero(i[r] == o)[0]
        keep[r, hit[0] if hit.size else -1] = False
    return s[keep].reshape(i.shape[0], -1), i[keep].reshape(i.shape[0], -1)


@pytest.mark.parametrize("name", ["255-f16", "300in513-f32", "257-f16-d768", "513-f16-holes"])
def test_search_rows_is_search_of_the_gathered_vectors(name: str, device: torch.device) -> None:
    st = _state(name, device)
    eb = st["bank"]
    live = (~st["gone"]).nonzero().squeeze(1)
    idx = live[torch.randperm(live.numel(), generator=cases.gen(31))[:GQ + 1]]
    idx[-1] = idx[0]
    vec = eb.rows(idx)
    s, i = eb.search_rows(idx, K)
    es, ei = _drop_self(*eb.search(vec, K + 1), idx)
    np.testing.assert_array_equal(i.cpu().numpy(), ei)
    np.testing.assert_array_equal(_bits(s), es.view(np.int32))
    assert not bool((i.cpu() == idx[:, None]).any()) and s.shape == (GQ + 1, K)
    # the own row masked out for some queries: the last of the K + 1 entries goes instead
    allow = (~st["gone"]).clone()
    allow[idx[:4]] = False
    s, i = eb.search_rows(idx, K, mask=allow.to(device))
    es, ei = _drop_self(*eb.search(vec, K + 1, mask=allow.to(device)), idx)
    np.testing.assert_array_equal(i.cpu().numpy(), ei)
    np.testing.assert_array_equal(_bits(s), es.view(np.int32))
    # "own": the stored codes at the rows' packed positions are the codes of the rows' labels
    labels = _labels(st["n"])
    s, i = eb.search_rows(idx, K, exclude_group="own")
    es, ei = eb.search(vec, K, exclude_group=labels[idx])
    np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(es))
    assert not bool((labels[i.cpu().clamp(min=0)] == labels[idx][:, None]).any())
    if st["gone"].any():
        with pytest.raises(ValueError, match="removed row"):
            eb.search_rows([int(live[0]), int(st["gone"].nonzero()[0])], K)


def test_rows_and_scores_see_a_replace_and_a_remove(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    n, capacity, d = 300, 513, 100
    vec = _vectors(n, d, F16, 41)
    eb = EmbeddingBank(vec.to(device), dtype=F16, normalize=False, capacity=capacity)
    q = _queries(GQ + 1, d, F32, False, 42, device)
    idx = torch.randperm(n, generator=cases.gen(43))[:40]
    before = eb.scores(q, idx)
    np.testing.assert_array_equal(_bits(eb.rows(idx)), _bits(vec[idx]))
    new = (q[:3].float() * 0.5).to(F16).cpu()  # each becomes the best row of its query, by far
    eb.replace(idx[[0, 7, 39]], new.to(device))
    vec2 = vec.clone()
    vec2[idx[[0, 7, 39]]] = new
    np.testing.assert_array_equal(_bits(eb.rows(idx)), _bits(vec2[idx]))
    np.testing.assert_array_equal(_bits(eb.rows(idx)), _bits(eb.bank[idx.to(device)]))
    after = eb.scores(q, idx)
    same = np.ones(40, dtype=bool)
    same[[0, 7, 39]] = False
    np.testing.assert_array_equal(_bits(after)[:, same], _bits(before)[:, same])
    s, i = eb.search_exhaustive(q, K)  # the new state: where it names a listed row, the bits are the same
    table = torch.full((GQ + 1, n), float("nan"), device=device)
    table[:, idx.to(device)] = after
    found = table.gather(1, i)
    known = (~torch.isnan(found)).cpu().numpy()
    assert i[:3, 0].cpu().tolist() == idx[[0, 7, 39]].tolist() and known[:3, 0].all()
    np.testing.assert_array_equal(_bits(found)[known], _bits(s)[known])
    assert eb.remove(rows=idx[[7, 8]]) == 2
    exp = vec2[idx].clone()
    exp[[7, 8]] = 0
    np.testing.assert_array_equal(_bits(eb.rows(idx)), _bits(exp))
    last = eb.scores(q, idx)
    same[8] = False
    same[[0, 39]] = True
    np.testing.assert_array_equal(_bits(last)[:, same], _bits(after)[:, same])
    assert bool((last[:, [7, 8]] == -float("inf")).all())


def test_a_captured_score_call_replays_over_a_replace(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    n, capacity, d = 300, 513, 100
    vec = _vectors(n, d, F16, 51)
    eb = EmbeddingBank(vec.to(device), dtype=F16, normalize=False, capacity=capacity)
    q = _queries(GQ + 1, d, F32, False, 52, device)
    index = torch.randperm(n, generator=cases.gen(53))[:70].to(device)
    out = torch.zeros((GQ + 1, 70), dtype=F32, device=device)
    eb._score_rows(q, index, out)  # (loads the kernel before the capture)
    torch.cuda.synchronize()
    first = out.clone()
    np.testing.assert_array_equal(_bits(first), _bits(eb.scores(q, index)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eb._score_rows(q, index, out)
    torch.cuda.synchronize()
    eb.replace(index[[3]], (q[:1].float() * 0.5).to(F16))  # the listed row becomes query 0's direction
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = eb.scores(q, index)
    np.testing.assert_array_equal(_bits(out), _bits(eager))
    changed = (_bits(out) != _bits(first)).any(axis=0)
    assert changed[3] and changed.sum() == 1 and float(out[0, 3]) > 0.49
