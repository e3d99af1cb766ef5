"""Host-side logic of `EmbeddingBank.remove` / `replace` / `compact` / `live` / `num_removed`: selectors, validation, counts,
stale filters, the index map, labels and origins after a compaction.  No device is touched: the rows stay on the CPU and the
bank's device hooks are replaced by row-order stand-ins (packed position = row), as in tests/test_append_host.py."""

from __future__ import annotations

import pytest
import torch

from imagescry_amd import EmbeddingBank
from imagescry_amd.search import RowFilter


class HostBank(EmbeddingBank):
    def _store(self, embeddings, normalize):
        self._norm_bound = torch.zeros(1)
        return embeddings.clone()

    def _alloc_image(self, capacity, device, grouped):
        codes = torch.full((capacity,), -2, dtype=torch.int32) if grouped else None
        return torch.zeros(capacity, self.dim), torch.zeros(capacity, dtype=torch.bool), codes

    def _append_rows(self, embeddings, first_row, normalize, codes):
        hi = first_row + embeddings.shape[0]
        assert hi <= self.capacity == self._bank.shape[0]
        self._bank[first_row:hi] = embeddings
        self._fill[first_row:hi] = True
        if codes is not None:
            self._row_codes[first_row:hi] = codes

    def _repack_rows(self, src, src_capacity, src_codes, dst, dst_capacity, dst_codes, dst_fill):
        assert not self._num_removed  # a bank with holes moves through the map
        n = self.num_local_rows
        dst[:n] = src[:n]
        dst_fill[:n] = True
        if dst_codes is not None:
            dst_codes[:n] = src_codes[:n]

    def _repack_map(self, src, src_capacity, src_codes, dst, dst_capacity, dst_codes, dst_fill, new_index):
        assert src_capacity == self.capacity and dst_capacity == dst.shape[0] and src.data_ptr() != dst.data_ptr()
        assert new_index.dtype == torch.int64 and new_index.shape == (self.num_local_rows,)
        for r, to in enumerate(new_index.tolist()):
            if to >= 0:
                assert not dst_fill[to]
                dst[to] = src[r]
                dst_fill[to] = True
                if dst_codes is not None:
                    dst_codes[to] = src_codes[r]

    def _remove_rows(self, index, removed):
        assert index.dtype == torch.int64 and index.numel() > 0 and self._fill.shape == (self.capacity,)
        for r in index.tolist():
            if 0 <= r < self.num_local_rows and self._fill[r]:
                self._fill[r] = False
                removed += 1
                if self._row_codes is not None:
                    c = int(self._row_codes[r])
                    self._row_codes[r] = -2
                    if c >= 0:
                        self._group_counts[c] -= 1

    def _replace_rows(self, embeddings, index, normalize):
        for i, r in enumerate(index.tolist()):
            if self._fill is None or self._fill[r]:
                self._bank[r] = embeddings[i]

    def _unpack_mask(self, packed, n_rows):
        return packed[:n_rows].clone()

    def _code_rows(self, codes):
        return torch.isin(self._row_codes, codes).nonzero().squeeze(1)

    def _pack_groups(self, codes):
        return torch.nn.functional.pad(codes, (0, self.capacity - codes.shape[0]), value=-2)

    def _pack_filter(self, local):
        return RowFilter(self, torch.nn.functional.pad(local, (0, self.capacity - local.shape[0])), local.sum().reshape(1))


def _rows(n: int, d: int = 8, seed: int = 0) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


def _bank(n: int = 10, **kw) -> HostBank:
    return HostBank(_rows(n), dtype=torch.float32, normalize=False, **kw)


def _labels_of_rows(eb: HostBank) -> list[int]:
    return eb.group_labels[eb._row_codes[: len(eb)].long()].tolist()


def test_a_bank_that_never_removes_carries_no_new_state() -> None:
    eb = _bank(10)
    assert eb.num_removed == 0 and "_num_removed" not in eb.__dict__ and eb._fill is None
    assert eb.live.tolist() == [True] * 10
    eb = _bank(10, capacity=12)
    assert eb.num_removed == 0 and "_num_removed" not in eb.__dict__ and eb.live.tolist() == [True] * 10


def test_exactly_one_selector_and_what_each_needs() -> None:
    eb = _bank(10, capacity=12)
    with pytest.raises(ValueError, match="exactly one of rows, image_ids or groups"):
        eb.remove()
    with pytest.raises(ValueError, match="exactly one of rows, image_ids or groups"):
        eb.remove(rows=[1], groups=[1])
    with pytest.raises(ValueError, match="image_ids needs row_origin"):
        eb.remove(image_ids=[1])
    with pytest.raises(ValueError, match="groups needs row groups"):
        eb.remove(groups=[1])
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 10\)"):
        eb.remove(rows=[3, 10])  # the reserved room is not a row
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 10\)"):
        eb.remove(rows=torch.tensor([-1]))
    with pytest.raises(ValueError, match="1-D sequence of integer"):
        eb.remove(rows=torch.tensor([1.0]))
    with pytest.raises(ValueError, match="1-D sequence of integer"):
        eb.remove(rows=torch.tensor([[1]]))
    assert eb.num_removed == 0 and eb._revision == 0 and eb._fill.sum() == 10
    pre = HostBank(_rows(10), dtype=torch.float32, normalize=False, presharded=True, index_base=100)
    with pytest.raises(ValueError, match=r"rows must lie in \[100, 110\)"):
        pre.remove(rows=[5])
    assert pre.remove(rows=[105]) == 1 and pre.live.tolist() == [True] * 5 + [False] + [True] * 4


def test_counts_with_duplicates_and_repeated_removals() -> None:
    eb = _bank(10, capacity=12)
    assert eb.remove(rows=[3, 3, 7, 3]) == 2 and len(eb) == 10 and eb.num_removed == 2
    assert eb.remove(rows=torch.tensor([3, 7], dtype=torch.int32)) == 0 and eb.num_removed == 2
    assert eb.remove(rows=[7, 8]) == 1 and eb.num_removed == 3 and len(eb) == 10 and eb.capacity == 12
    assert eb.live.tolist() == [True, True, True, False, True, True, True, False, False, True]
    assert eb.remove(rows=[]) == 0 and eb.num_removed == 3


def test_a_bank_that_never_reserved_gains_a_full_bitmap_and_keeps_its_image() -> None:
    eb = _bank(10)
    image = eb._bank.data_ptr()
    assert eb._as_filter(None) is None
    assert eb.remove(rows=[4]) == 1
    assert eb._bank.data_ptr() == image and eb.capacity == eb._capacity == 10 and len(eb) == 10
    assert eb._fill.tolist() == [True] * 4 + [False] + [True] * 5
    rf = eb._as_filter(None)
    assert rf is eb._fill_filter and rf.packed is eb._fill  # a full bank with a hole: the masked calls
    assert torch.equal(eb._bank, _rows(10))  # row bytes are not touched


def test_the_fill_filter_serves_while_there_is_a_hole_and_append_numbers_from_len() -> None:
    eb = _bank(10, capacity=12)
    eb.remove(rows=[0])
    assert eb.append(_rows(2, seed=1)) == range(10, 12) and len(eb) == 12 == eb.capacity
    assert eb._as_filter(None) is eb._fill_filter and eb._fill.tolist() == [False] + [True] * 11  # full, but holed
    assert eb.append(_rows(1, seed=2)) == range(12, 13) and eb.capacity == 24  # a growth keeps the hole
    assert eb.live.tolist() == [False] + [True] * 12 and eb.num_removed == 1 and eb._fill.sum() == 12
    assert torch.equal(eb._bank[1:10], _rows(10)[1:]) and torch.equal(eb._bank[12], _rows(1, seed=2)[0])
    eb.reserve(30)
    assert eb.capacity == 30 and eb.live.tolist() == [False] + [True] * 12


def test_stale_row_filters_are_refused_after_each_call() -> None:
    eb = _bank(10, capacity=12)
    for change in (lambda: eb.remove(rows=[1]), lambda: eb.replace([2], _rows(1, seed=5)), lambda: eb.compact()):
        rf = eb.row_filter(rows=[2, 3])
        assert eb._as_filter(rf) is rf
        before = eb._revision
        change()
        assert eb._revision == before + 1
        with pytest.raises(ValueError, match="made before the bank changed; make it again"):
            eb._as_filter(rf)
        assert eb._fill_filter._revision == eb._revision and eb._fill_filter.packed is eb._fill


def test_row_filter_never_allows_a_removed_row() -> None:
    eb = _bank(10, capacity=12)
    eb.remove(rows=[2, 5])
    rf = eb.row_filter(rows=[1, 2, 3])
    assert rf.packed.tolist() == [False, True, False, True] + [False] * 8 and int(rf.allowed_count) == 2
    rf = eb.row_filter(rows=[1], exclude=True)
    assert rf.packed[:10].tolist() == [True, False, False, True, True, False, True, True, True, True]
    assert int(rf.allowed_count) == 7 and not rf.packed[10:].any()
    rf = eb._as_filter(torch.ones(10, dtype=torch.bool))
    assert int(rf.allowed_count) == 8 and torch.equal(rf.packed, eb._fill)


def test_remove_by_image_and_by_group() -> None:
    labels = torch.tensor([10, 20, 20, 40, 10, 20, 30, 30])
    eb = HostBank(_rows(8), dtype=torch.float32, normalize=False, row_groups=labels, capacity=9)
    eb.row_origin = torch.stack([labels, torch.zeros(8, dtype=torch.int64), torch.arange(8)], dim=1)
    assert eb._max_group_rows == 3
    assert eb.remove(groups=[20, 999]) == 3  # a label no row carries selects nothing
    assert eb.live.tolist() == [True, False, False, True, True, False, True, True]
    assert eb._row_codes[:8].tolist() == [0, -2, -2, 3, 0, -2, 2, 2] and eb._group_counts.tolist() == [2, 0, 2, 1]
    assert eb.group_labels.tolist() == [10, 20, 30, 40] and eb._max_group_rows == 3  # an upper bound until compact
    assert eb.remove(groups=torch.tensor([20])) == 0
    assert eb.remove(image_ids=[40, 20]) == 1 and eb.num_removed == 4
    assert eb._group_counts.tolist() == [2, 0, 2, 0]
    with pytest.raises(TypeError, match="integer"):
        eb.remove(groups=torch.tensor([1.5]))
    # an append of a removed label counts from the lowered figure
    eb.append(_rows(1, seed=3), row_groups=torch.tensor([40]), row_origin=torch.tensor([[40, 0, 8]]))
    assert eb._group_counts.tolist() == [2, 0, 2, 1] and eb._max_group_rows == 2 and len(eb) == 9


def test_replace_validates_and_leaves_tombstones_alone() -> None:
    eb = _bank(10, capacity=12)
    new = _rows(3, seed=7)
    with pytest.raises(ValueError, match="indices must be distinct"):
        eb.replace([1, 4, 1], new)
    with pytest.raises(ValueError, match=r"shape \[m, 8\]"):
        eb.replace([1, 2, 3], _rows(3, d=7))
    with pytest.raises(ValueError, match=r"shape \[m, 8\]"):
        eb.replace([1], new[0])
    with pytest.raises(ValueError, match="one row per vector"):
        eb.replace([1, 2], new)
    with pytest.raises(TypeError, match="floating point"):
        eb.replace([1, 2, 3], torch.ones(3, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"indices must lie in \[0, 10\)"):
        eb.replace([1, 2, 10], new)
    assert eb._revision == 0 and torch.equal(eb._bank[:10], _rows(10))
    eb.remove(rows=[4])
    assert eb.replace(torch.tensor([9, 4, 0]), new) is None
    exp = _rows(10)
    exp[9], exp[0] = new[0], new[2]  # row 4 stays removed, with the bytes it had
    assert torch.equal(eb._bank[:10], exp) and eb.live.tolist() == [True] * 4 + [False] + [True] * 5
    before = eb._revision
    eb.replace([], torch.zeros(0, 8))  # nothing to do
    assert eb._revision == before
    plain = _bank(10)  # a bank without a bitmap stays without one
    plain.replace([3], new[:1])
    assert plain._fill is None and plain._fill_filter is None and plain._revision == 1
    assert torch.equal(plain._bank[3], new[0])


def test_compact_maps_indices_filters_origin_and_drops_labels() -> None:
    labels = torch.tensor([10, 20, 20, 40, 10, 20, 30, 30])
    eb = HostBank(_rows(8), dtype=torch.float32, normalize=False, row_groups=labels, capacity=9)
    eb.row_origin = torch.stack([labels, torch.zeros(8, dtype=torch.int64), torch.arange(8)], dim=1)
    eb.remove(rows=[1, 2, 3, 5])  # every row of 20 and of 40
    image = eb._bank.data_ptr()
    index_map = eb.compact()
    assert index_map.dtype == torch.int64 and index_map.tolist() == [0, -1, -1, -1, 1, -1, 2, 3]
    assert len(eb) == 4 and eb.capacity == 9 and eb.num_removed == 0 and eb._bank.data_ptr() != image
    assert torch.equal(eb._bank[:4], _rows(8)[[0, 4, 6, 7]]) and not eb._bank[4:].any()
    assert eb._fill.tolist() == [True] * 4 + [False] * 5 and eb.live.tolist() == [True] * 4
    assert eb.row_origin[:, 2].tolist() == [0, 4, 6, 7]
    assert eb.group_labels.tolist() == [10, 30] and _labels_of_rows(eb) == [10, 10, 30, 30]
    assert eb._row_codes[4:].tolist() == [-2] * 5 and eb._row_codes.dtype == torch.int32
    assert eb._group_counts.tolist() == [2, 2] and eb._max_group_rows == 2  # exact again (it was 3)
    fresh = HostBank(_rows(8)[[0, 4, 6, 7]], dtype=torch.float32, normalize=False, row_groups=labels[[0, 4, 6, 7]])
    assert torch.equal(fresh.group_labels, eb.group_labels) and torch.equal(fresh._row_codes, eb._row_codes[:4])
    # the next append numbers from the new length, and the bank filled exactly goes back to the unmasked calls
    got = eb.append(_rows(5, seed=2), row_groups=torch.tensor([20] * 5), row_origin=torch.zeros(5, 3, dtype=torch.int64))
    assert got == range(4, 9) and eb._as_filter(None) is None and eb.group_labels.tolist() == [10, 20, 30]


def test_compact_without_holes_is_the_identity() -> None:
    for eb in (_bank(10), _bank(10, capacity=12)):
        image = eb._bank.data_ptr()
        assert eb.compact().tolist() == list(range(10))
        assert eb._bank.data_ptr() == image and eb._revision == 0 and len(eb) == 10
    eb = _bank(10, capacity=12)
    eb.remove(rows=[9, 0])
    assert eb.compact().tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, 7, -1]
    assert eb.compact().tolist() == list(range(8))  # already compact
    eb.remove(rows=list(range(8)))
    assert eb.compact().tolist() == [-1] * 8 and len(eb) == 0 and eb.capacity == 12  # an emptied bank


def test_a_sharded_bank_refuses() -> None:
    eb = _bank(10)
    eb.process_group = object()  # (only its presence is looked at before the refusal)
    with pytest.raises(ValueError, match=r"a sharded bank \(process_group=\) cannot remove: its global indices"):
        eb.remove(rows=[1])
    with pytest.raises(ValueError, match=r"a sharded bank \(process_group=\) cannot replace: its global indices"):
        eb.replace([1], _rows(1))
    with pytest.raises(ValueError, match=r"a sharded bank \(process_group=\) cannot compact: its global indices"):
        eb.compact()
