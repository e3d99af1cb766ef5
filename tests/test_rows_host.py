"""Host-side logic of `EmbeddingBank.rows` / `scores` / `similarity_map` / `search_rows`: index validation, duplicates,
removed rows, the map's shape and holes, the self-drop of `search_rows`, the "own" group codes, the k bounds and the sharded
refusal.  No device is touched: the rows stay on the CPU and the bank's device hooks are replaced by row-order stand-ins
(packed position = row), as in tests/test_remove_host.py; the search hook is the float64 oracle (tests/groups_oracle.py)."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from groups_oracle import PAD, oracle  # noqa: E402

from imagescry_amd import EmbeddingBank, _lib  # noqa: E402
from imagescry_amd.search import RowFilter  # noqa: E402
from oracle import search_oracle  # noqa: E402


class HostBank(EmbeddingBank):
    calls: list  # (hook name, rows it was given), in call order

    def _store(self, embeddings, normalize):
        self._norm_bound = torch.zeros(1)
        self.calls = []
        return embeddings.clone()

    def _alloc_image(self, capacity, device, grouped):
        self.calls = []
        codes = torch.full((capacity,), -2, dtype=torch.int32) if grouped else None
        return torch.zeros(capacity, self.dim), torch.zeros(capacity, dtype=torch.bool), codes

    def _append_rows(self, embeddings, first_row, normalize, codes):
        hi = first_row + embeddings.shape[0]
        self._bank[first_row:hi] = embeddings
        self._fill[first_row:hi] = True
        if codes is not None:
            self._row_codes[first_row:hi] = codes

    def _remove_rows(self, index, removed):
        for r in index.tolist():
            if 0 <= r < self.num_local_rows and self._fill[r]:
                self._fill[r] = False
                removed += 1
                if self._row_codes is not None:
                    c = int(self._row_codes[r])
                    self._row_codes[r] = -2
                    if c >= 0:
                        self._group_counts[c] -= 1

    def _unpack_mask(self, packed, n_rows):
        return packed[:n_rows].clone()

    def _pack_groups(self, codes):
        return torch.nn.functional.pad(codes, (0, self.capacity - codes.shape[0]), value=-2)

    def _pack_filter(self, local):
        return RowFilter(self, torch.nn.functional.pad(local, (0, self.capacity - local.shape[0])), local.sum().reshape(1))

    def _live(self, index):
        return torch.ones(index.shape, dtype=torch.bool) if self._fill is None else self._fill[index]

    # ---- the two new hooks and the code hook, in row order
    def _gather_rows(self, index, out):
        assert index.dtype == torch.int64 and index.is_contiguous() and index.numel() > 0
        assert out.shape == (index.numel(), self.dim) and out.dtype == self.dtype
        self.calls.append(("gather", index.tolist()))
        out.copy_(torch.where(self._live(index)[:, None], self._bank[index], torch.zeros((), dtype=self.dtype)))

    def _score_rows(self, q, index, out):
        assert index.dtype == torch.int64 and index.numel() > 0 and q.shape[0] > 0
        assert out.shape == (q.shape[0], index.numel()) and out.dtype == torch.float32
        self.calls.append(("score", index.tolist()))
        s = torch.from_numpy(search_oracle.exact_scores(self._bank[index], q))
        out.copy_(s.masked_fill(~self._live(index)[None, :], -math.inf))

    def _stored_codes(self, index):
        self.calls.append(("codes", index.tolist()))
        return self._row_codes[index]

    def _local_topk(self, queries, kk, out=None, lane=-1, stream=None, mask=None, groups=None):
        n = self.num_local_rows
        allow = np.ones((queries.shape[0], n), dtype=bool)
        if groups is not None:
            assert groups.dtype == torch.int32 and groups.shape == (queries.shape[0],)
            allow &= self._row_codes[:n].numpy()[None, :] != groups.numpy()[:, None]
        if mask is not None:
            allow &= mask.packed[:n].numpy()[None, :]
        self.calls.append(("topk", kk))
        s, i = oracle(self._bank[:n], queries, kk, allow, self.index_base, pad=(np.nan, PAD))
        return torch.from_numpy(s), torch.from_numpy(i)


def _rows(n: int, d: int = 8, seed: int = 0) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


def _bank(n: int = 10, **kw) -> HostBank:
    return HostBank(_rows(n), dtype=torch.float32, normalize=False, **kw)


def test_index_validation_of_every_call() -> None:
    eb = _bank(10, capacity=12)
    q = _rows(2, seed=1)
    for call in (eb.rows, lambda ix: eb.scores(q, ix), lambda ix: eb.search_rows(ix, 2)):
        with pytest.raises(ValueError, match=r"must lie in \[0, 10\)"):
            call([3, 10])  # the reserved room is not a row
        with pytest.raises(ValueError, match=r"must lie in \[0, 10\)"):
            call(torch.tensor([-1]))
        with pytest.raises(ValueError, match="1-D sequence of integer"):
            call(torch.tensor([1.0]))
        with pytest.raises(ValueError, match="1-D sequence of integer"):
            call(torch.tensor([[1]]))
    assert eb.calls == []  # nothing was launched
    with pytest.raises(ValueError, match=r"shape \[Q, 8\]"):
        eb.scores(_rows(2, d=7), [1])
    with pytest.raises(TypeError, match="floating point"):
        eb.scores(torch.ones(2, 8, dtype=torch.int32), [1])
    pre = HostBank(_rows(10), dtype=torch.float32, normalize=False, presharded=True, index_base=100)
    with pytest.raises(ValueError, match=r"indices must lie in \[100, 110\)"):
        pre.rows([5])
    assert torch.equal(pre.rows([105, 100]), _rows(10)[[5, 0]]) and pre.calls == [("gather", [5, 0])]
    s, i = pre.search_rows([103], 2)  # global indices in, global indices out, self dropped by its global index
    assert 103 not in i.tolist()[0] and all(100 <= v < 110 for v in i.tolist()[0])


def test_rows_in_any_order_with_duplicates_and_removed_rows_as_zeros() -> None:
    eb = _bank(10, capacity=12)
    idx = [7, 2, 7, 9, 0, 2]
    got = eb.rows(idx)
    assert got.dtype == torch.float32 and torch.equal(got, _rows(10)[idx])
    assert torch.equal(eb.rows(torch.tensor(idx, dtype=torch.int32)), got)  # any integer dtype
    empty = eb.rows([])
    assert empty.shape == (0, 8) and empty.dtype == torch.float32 and eb.calls[-1] == ("gather", idx)  # no launch for []
    eb.remove(rows=[2])
    got = eb.rows(idx)
    exp = _rows(10)[idx]
    exp[[1, 5]] = 0
    assert torch.equal(got, exp)
    plain = _bank(10)  # a bank without a bitmap: every row is stored
    assert torch.equal(plain.rows(idx), _rows(10)[idx])


def test_scores_shape_duplicates_removed_columns_and_empty_sides() -> None:
    eb = _bank(10, capacity=12)
    q = _rows(3, seed=1)
    idx = [4, 4, 9, 0]
    s = eb.scores(q, idx)
    assert s.dtype == torch.float32 and s.shape == (3, 4)
    np.testing.assert_array_equal(s.numpy(), search_oracle.exact_scores(_rows(10)[idx], q))
    assert torch.equal(s[:, 0], s[:, 1])
    n = len(eb.calls)
    assert eb.scores(q[:0], idx).shape == (0, 4) and eb.scores(q, []).shape == (3, 0) and len(eb.calls) == n  # no launch
    eb.remove(rows=[9])
    s2 = eb.scores(q, idx)
    assert torch.isinf(s2[:, 2]).all() and (s2[:, 2] < 0).all()
    assert torch.equal(s2[:, [0, 1, 3]], s[:, [0, 1, 3]])
    # strided queries are made contiguous in the inner dimension, wide rows are passed as they are
    wide = torch.zeros(3, 16)
    wide[:, :8] = q
    assert torch.equal(eb.scores(wide[:, :8], idx), s2)


def _origin_bank(**kw) -> HostBank:
    # image 5: a 2 x 3 grid without its cell (1, 1); image 8: one cell at (0, 2)
    origin = torch.tensor([[5, 0, 0], [5, 0, 1], [5, 0, 2], [8, 0, 2], [5, 1, 0], [5, 1, 2]])
    eb = HostBank(_rows(6), dtype=torch.float32, normalize=False, row_groups=origin[:, 0], **kw)
    eb.row_origin = origin
    return eb


def test_similarity_map_shape_holes_and_unknown_images() -> None:
    eb = _origin_bank(capacity=8)
    q = _rows(2, seed=3)
    full = search_oracle.exact_scores(_rows(6), q)
    m = eb.similarity_map(q, 5)
    assert m.shape == (2, 2, 3) and m.dtype == torch.float32 and eb.calls[-1] == ("score", [0, 1, 2, 4, 5])
    np.testing.assert_array_equal(m[:, 0, :].numpy(), full[:, [0, 1, 2]])
    np.testing.assert_array_equal(m[:, 1, [0, 2]].numpy(), full[:, [4, 5]])
    assert (m[:, 1, 1] == -math.inf).all()  # a cell the bank does not hold
    m8 = eb.similarity_map(q, torch.tensor(8))
    assert m8.shape == (2, 1, 3) and (m8[:, 0, :2] == -math.inf).all()
    np.testing.assert_array_equal(m8[:, 0, 2].numpy(), full[:, 3])
    eb.remove(rows=[1])
    m = eb.similarity_map(q, 5)
    assert m.shape == (2, 2, 3) and (m[:, 0, 1] == -math.inf).all()  # a removed cell
    np.testing.assert_array_equal(m[:, 0, [0, 2]].numpy(), full[:, [0, 2]])
    assert eb.similarity_map(q[:0], 5).shape == (0, 2, 3)
    with pytest.raises(ValueError, match="image_id 6 is not in the bank"):
        eb.similarity_map(q, 6)
    with pytest.raises(ValueError, match="similarity_map needs row_origin"):
        _bank(10).similarity_map(_rows(1), 5)


def _without_self(rows: torch.Tensor, idx: list[int], k: int, allow: np.ndarray | None = None):
    """The float64 oracle's top-k of every row idx[i] over the rows other than idx[i] itself (and `allow`ed)."""
    ok = np.ones((len(idx), rows.shape[0]), dtype=bool) if allow is None else allow.copy()
    ok[np.arange(len(idx)), idx] = False
    return oracle(rows, rows[idx], k, ok)


def test_search_rows_drops_each_querys_own_row() -> None:
    eb = _bank(20)
    idx = [3, 17, 3, 0]
    s, i = eb.search_rows(idx, 4)
    assert eb.calls == [("gather", idx), ("topk", 5)]  # the stored vectors are the queries; k + 1 entries searched
    es, ei = _without_self(_rows(20), idx, 4)
    np.testing.assert_array_equal(i.numpy(), ei)
    np.testing.assert_array_equal(s.numpy(), es)
    assert s.shape == (4, 4) and i.dtype == torch.int64 and s.dtype == torch.float32
    # exclude_self=False: plain search of the stored vectors, self first
    s0, i0 = eb.search_rows(idx, 4, exclude_self=False)
    assert eb.calls[-1] == ("topk", 4) and i0[:, 0].tolist() == idx
    es0, ei0 = oracle(_rows(20), _rows(20)[idx], 4, np.ones((4, 20), dtype=bool))
    np.testing.assert_array_equal(i0.numpy(), ei0)
    np.testing.assert_array_equal(s0.numpy(), es0)
    s, i = eb.search_rows([], 4)
    assert s.shape == (0, 4) and i.shape == (0, 4)


def test_search_rows_when_the_mask_disallows_the_own_row() -> None:
    eb = _bank(20)
    idx = [3, 17, 5]
    allowed = torch.ones(20, dtype=torch.bool)
    allowed[[3, 4, 5]] = False  # the own rows of queries 0 and 2 are masked out; query 1's is not
    s, i = eb.search_rows(idx, 4, mask=allowed)
    allow = np.broadcast_to(allowed.numpy(), (3, 20))
    es, ei = _without_self(_rows(20), idx, 4, allow)
    np.testing.assert_array_equal(i.numpy(), ei)  # own row absent: the LAST of the k + 1 entries goes
    np.testing.assert_array_equal(s.numpy(), es)
    # fewer rows left than k: the masked search's padding survives the drop
    few = torch.zeros(20, dtype=torch.bool)
    few[[3, 8, 9]] = True
    s, i = eb.search_rows([3], 4, mask=few)
    assert sorted(i[0, :2].tolist()) == [8, 9] and i[0, 2:].tolist() == [-1, -1]
    assert (s[0, 2:] == -math.inf).all()


def test_search_rows_with_exact_copies_of_the_query_keeps_the_lower_index() -> None:
    rows = _rows(12)
    rows[2] = rows[7]
    rows[9] = rows[7]  # rows 2, 7, 9 are one vector: equal scores, ordered by index
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    s, i = eb.search_rows([7, 9, 2], 3)
    assert i[0, :2].tolist() == [2, 9] and i[1, :2].tolist() == [2, 7] and i[2, :2].tolist() == [7, 9]
    assert torch.equal(s[:, 0], s[:, 1])
    es, ei = _without_self(rows, [7, 9, 2], 3)
    np.testing.assert_array_equal(i.numpy(), ei)
    np.testing.assert_array_equal(s.numpy(), es)
    # k + 1 copies with lower indices precede the own row: it is not among the k + 1, the last entry goes
    rows = _rows(12)
    rows[1] = rows[2] = rows[3] = rows[0]
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    s, i = eb.search_rows([3], 2)
    assert i.tolist() == [[0, 1]]


def test_own_group_codes_come_from_the_stored_codes() -> None:
    labels = torch.tensor([50, 7, 50, 7, 7, 900, 7, 50, 900, 50])
    eb = HostBank(_rows(10), dtype=torch.float32, normalize=False, row_groups=labels, capacity=12)
    idx = [5, 0, 3]
    s, i = eb.search_rows(idx, 3, exclude_group="own")
    assert eb.calls == [("gather", idx), ("codes", idx), ("topk", 3)]  # k entries: the group exclusion drops self
    allow = labels.numpy()[None, :] != labels.numpy()[idx][:, None]
    es, ei = oracle(_rows(10), _rows(10)[idx], 3, allow)
    np.testing.assert_array_equal(i.numpy(), ei)
    np.testing.assert_array_equal(s.numpy(), es)
    # ... which is the search with the rows' labels
    s2, i2 = eb.search(_rows(10)[idx], 3, exclude_group=labels[idx])
    assert torch.equal(i, i2) and torch.equal(s, s2)
    # a label tensor is accepted as in `search`, and self is then dropped by index
    s3, i3 = eb.search_rows(idx, 3, exclude_group=torch.tensor([7, 7, 900]))
    allow = labels.numpy()[None, :] != np.array([7, 7, 900])[:, None]
    es, ei = _without_self(_rows(10), idx, 3, allow)
    np.testing.assert_array_equal(i3.numpy(), ei)
    np.testing.assert_array_equal(s3.numpy(), es)
    with pytest.raises(ValueError, match="exclude_group='own' needs row groups"):
        _bank(10).search_rows([1], 2, exclude_group="own")
    with pytest.raises(ValueError, match="label tensor or 'own'"):
        eb.search_rows([1], 2, exclude_group="mine")


def test_k_bounds() -> None:
    eb = _bank(10)
    for k in (0, -1):
        with pytest.raises(ValueError, match="k must be >= 1"):
            eb.search_rows([1], k)
    with pytest.raises(TypeError, match="k must be an int"):
        eb.search_rows([1], 2.0)
    with pytest.raises(ValueError, match=r"k=10 must be in \[1, 9\] with exclude_self=True"):
        eb.search_rows([1], 10)
    assert eb.search_rows([1], 9)[1].shape == (1, 9)
    assert eb.search_rows([1], 10, exclude_self=False)[1].shape == (1, 10)
    with pytest.raises(ValueError, match="k=11 exceeds the bank size 10"):
        eb.search_rows([1], 11, exclude_self=False)
    big = _bank(_lib.ISC_TOPK_MAX_K + 5)
    top = _lib.ISC_TOPK_MAX_K
    with pytest.raises(ValueError, match=rf"k={top} must be in \[1, {top - 1}\] with exclude_self=True"):
        big.search_rows([1], top)
    assert big.search_rows([1], top - 1)[1].shape == (1, top - 1)
    assert big.search_rows([1], top, exclude_self=False)[1].shape == (1, top)
    with pytest.raises(ValueError, match=f"k must be <= {top}"):
        big.search_rows([1], top + 1, exclude_self=False)
    grouped = HostBank(_rows(10), dtype=torch.float32, normalize=False, row_groups=torch.arange(10) // 2)
    assert grouped.search_rows([1], 10, exclude_group="own")[1][0, 8:].tolist() == [-1, -1]  # "own": the bounds of `search`


def test_a_removed_index_is_refused_by_search_rows() -> None:
    eb = _bank(10, capacity=12)
    eb.remove(rows=[4])
    with pytest.raises(ValueError, match="indices name a removed row"):
        eb.search_rows([1, 4], 2)
    s, i = eb.search_rows([1, 5], 2)
    assert 4 not in i.flatten().tolist()  # nor is a removed row ever found


def test_a_sharded_bank_refuses() -> None:
    eb = _origin_bank()
    eb.process_group = object()  # (only its presence is looked at before the refusal)
    q = _rows(1)
    for what, call in (("read rows back", lambda: eb.rows([1])), ("score rows", lambda: eb.scores(q, [1])),
                       ("map an image", lambda: eb.similarity_map(q, 5)),
                       ("search by row", lambda: eb.search_rows([1], 2))):
        with pytest.raises(ValueError, match=rf"a sharded bank \(process_group=\) cannot {what}: a row is stored on one"):
            call()
    assert eb.calls == []
