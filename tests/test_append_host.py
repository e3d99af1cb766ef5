"""Host-side logic of `EmbeddingBank.append` / `reserve` / `capacity=`: validation, the returned indices, the label
re-map, stale filters.  No device is touched: the rows stay on the CPU and the bank's device hooks are replaced by
row-order stand-ins (packed position = row), the way tests/test_collapse_host.py rehearses the collapsed search."""

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
            assert codes.dtype == torch.int32
            self._row_codes[first_row:hi] = codes

    def _repack_rows(self, src, src_capacity, src_codes, dst, dst_capacity, dst_codes, dst_fill):
        n = self.num_local_rows
        assert src_capacity == self.capacity and dst_capacity == dst.shape[0]
        dst[:n] = src[:n]
        dst_fill[:n] = True
        if dst_codes is not None:
            dst_codes[:n] = src_codes[:n]

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


def test_a_bank_that_never_reserves_carries_no_fill_state() -> None:
    eb = _bank(10)
    assert eb.capacity == len(eb) == 10 and eb._fill is None and eb._capacity is None and eb._revision == 0
    assert eb._as_filter(None) is None


def test_capacity_is_validated() -> None:
    with pytest.raises(ValueError, match="at least"):
        _bank(10, capacity=9)
    with pytest.raises(ValueError, match="at least"):
        HostBank(torch.zeros(0, 8), dtype=torch.float32, capacity=0)
    with pytest.raises(TypeError, match="capacity must be an int"):
        _bank(10, capacity=12.0)
    eb = _bank(10, capacity=10)
    assert eb.capacity == 10 and eb._fill.all()
    with pytest.raises(ValueError, match="at least"):
        eb.reserve(9)
    with pytest.raises(TypeError, match="capacity must be an int"):
        eb.reserve(True)


def test_append_validates_rows() -> None:
    eb = _bank(10, capacity=20)
    with pytest.raises(ValueError, match=r"shape \[m, 8\]"):
        eb.append(_rows(3, d=7))
    with pytest.raises(ValueError, match=r"shape \[m, 8\]"):
        eb.append(_rows(3)[0])
    with pytest.raises(TypeError, match="floating point"):
        eb.append(torch.ones(3, 8, dtype=torch.int32))
    with pytest.raises(TypeError, match="floating point"):
        eb.append([[0.0] * 8])
    assert len(eb) == 10 and eb._revision == 0


def test_row_groups_and_row_origin_are_required_iff_the_bank_has_them() -> None:
    plain = _bank(10, capacity=20)
    with pytest.raises(ValueError, match="row_groups must be given iff"):
        plain.append(_rows(2), row_groups=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="row_origin must be given iff"):
        plain.append(_rows(2), row_origin=torch.zeros(2, 3, dtype=torch.int64))
    grouped = _bank(10, capacity=20, row_groups=torch.arange(10) // 3)
    with pytest.raises(ValueError, match="row_groups must be given iff"):
        grouped.append(_rows(2))
    with pytest.raises(ValueError, match=r"shape \[2\]"):
        grouped.append(_rows(2), row_groups=torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError, match="integer"):
        grouped.append(_rows(2), row_groups=torch.tensor([1.0, 2.0]))
    grouped.row_origin = torch.zeros(10, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="row_origin must be given iff"):
        grouped.append(_rows(2), row_groups=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match=r"shape \[2, 3\]"):
        grouped.append(_rows(2), row_groups=torch.tensor([1, 2]), row_origin=torch.zeros(2, 2, dtype=torch.int64))
    assert len(grouped) == 10
    got = grouped.append(_rows(2), row_groups=torch.tensor([1, 2]), row_origin=torch.tensor([[7, 0, 0], [7, 0, 1]]))
    assert got == range(10, 12) and grouped.row_origin.shape == (12, 3) and grouped.row_origin[-1].tolist() == [7, 0, 1]


def test_a_sharded_bank_refuses() -> None:
    eb = _bank(10)
    eb.process_group = object()  # (only its presence is looked at before the refusal)
    with pytest.raises(ValueError, match="sharded"):
        eb.append(_rows(2))
    with pytest.raises(ValueError, match="sharded"):
        eb.reserve(20)


def test_append_returns_the_new_indices_and_grows() -> None:
    eb = _bank(10, capacity=12)
    assert eb.append(_rows(2, seed=1)) == range(10, 12) and eb.capacity == 12 and len(eb) == 12
    assert eb._as_filter(None) is None  # full again: the unmasked calls
    assert eb.append(_rows(1, seed=2)) == range(12, 13) and eb.capacity == 24  # max(2 * capacity, len + m)
    assert eb._as_filter(None).packed is eb._fill and eb._fill.sum() == 13
    assert eb.append(_rows(40, seed=3)) == range(13, 53) and eb.capacity == 53
    assert torch.equal(eb._bank[:10], _rows(10)) and torch.equal(eb._bank[13:53], _rows(40, seed=3))
    # a bank that never reserved grows on its first append; a presharded bank's indices continue from its base
    eb = HostBank(_rows(10), dtype=torch.float32, normalize=False, presharded=True, index_base=100)
    assert eb.append(_rows(3, seed=1)) == range(110, 113) and eb.capacity == 20 and len(eb) == eb.num_local_rows == 13
    assert torch.equal(eb._bank[:10], _rows(10)) and eb._fill.tolist() == [True] * 13 + [False] * 7


def test_an_empty_append_is_a_no_op() -> None:
    eb = _bank(10, capacity=12)
    rf = eb.row_filter(rows=[1, 2])
    assert eb.append(torch.zeros(0, 8)) == range(10, 10)
    assert len(eb) == 10 and eb._revision == 0 and eb._as_filter(rf) is rf
    eb = _bank(10)
    assert eb.append(torch.zeros(0, 8)) == range(10, 10) and eb._fill is None and eb.capacity == 10


def test_a_bank_may_start_empty() -> None:
    eb = HostBank(torch.zeros(0, 8), dtype=torch.float32, capacity=16, row_groups=torch.zeros(0, dtype=torch.int64))
    assert len(eb) == 0 and eb.capacity == 16 and eb.group_labels.numel() == 0
    assert eb.append(_rows(3), row_groups=torch.tensor([5, -1, 5])) == range(0, 3)
    assert eb.group_labels.tolist() == [-1, 5] and _labels_of_rows(eb) == [5, -1, 5] and eb._max_group_rows == 2


def test_a_stale_row_filter_is_refused() -> None:
    eb = _bank(10, capacity=20)
    rf = eb.row_filter(rows=[1, 2])
    assert eb._as_filter(rf) is rf
    eb.append(_rows(1, seed=1))
    with pytest.raises(ValueError, match="made before the bank changed; make it again"):
        eb._as_filter(rf)
    rf = eb.row_filter(torch.ones(11, dtype=torch.bool))  # a bool mask has the bank's real row count
    assert eb._as_filter(rf) is rf and rf.packed.shape == (20,)
    with pytest.raises(ValueError, match="allow must be a bool tensor"):
        eb.row_filter(torch.ones(20, dtype=torch.bool))
    eb.reserve(40)
    with pytest.raises(ValueError, match="made before the bank changed"):
        eb._as_filter(rf)


def test_new_labels_keep_group_labels_sorted_and_codes_in_step() -> None:
    labels = [10, 20, 20, 40, 10, 20]
    eb = HostBank(_rows(6), dtype=torch.float32, normalize=False, row_groups=torch.tensor(labels), capacity=8)
    assert eb.group_labels.tolist() == [10, 20, 40] and eb._max_group_rows == 3
    eb.append(_rows(2, seed=1), row_groups=torch.tensor([20, 40]))  # existing labels: no re-map
    labels += [20, 40]
    assert eb.group_labels.tolist() == [10, 20, 40] and _labels_of_rows(eb) == labels and eb._max_group_rows == 4
    # before, between and after the old labels, a negative label, and across a growth
    new = [5, 30, 50, -7, 30, 30, 30]
    eb.append(_rows(7, seed=2), row_groups=torch.tensor(new, dtype=torch.int32))
    labels += new
    assert eb.capacity == 16 and eb.group_labels.tolist() == [-7, 5, 10, 20, 30, 40, 50]
    assert _labels_of_rows(eb) == labels and eb._max_group_rows == 4
    assert eb._row_codes[15:].tolist() == [-2] and eb._row_codes.dtype == torch.int32
    fresh = HostBank(_rows(15), dtype=torch.float32, normalize=False, row_groups=torch.tensor(labels))
    assert torch.equal(fresh.group_labels, eb.group_labels) and torch.equal(fresh._row_codes, eb._row_codes[:15])
    assert fresh._max_group_rows == eb._max_group_rows
