"""Host-side validation of `EmbeddingBank.search_groups` / `search_groups_exhaustive` (no device is touched: every call
fails before a launch), and the planning figure the bank takes at construction."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from collapse_oracle import collapse_bank_class  # noqa: E402


def _bank(labels=None, n=40, d=8):
    bank_cls = collapse_bank_class()
    rows = torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(0)), dim=1)
    return bank_cls(rows, dtype=torch.float32, normalize=False, row_groups=labels), rows


def test_max_group_rows_is_taken_at_construction() -> None:
    eb, _ = _bank(torch.arange(40) // 7)
    assert eb._max_group_rows == 7
    eb, _ = _bank(torch.arange(40))
    assert eb._max_group_rows == 1
    eb, _ = _bank(None)
    assert eb._max_group_rows == 0 and eb.group_labels is None


def test_search_groups_needs_row_groups() -> None:
    eb, rows = _bank(None)
    with pytest.raises(ValueError, match="row groups"):
        eb.search_groups(rows[:2], 3)
    with pytest.raises(ValueError, match="row groups"):
        eb.search_groups_exhaustive(rows[:2], 3)


@pytest.mark.parametrize("call", ["search_groups", "search_groups_exhaustive"])
def test_search_groups_validates_its_arguments(call: str) -> None:
    eb, rows = _bank(torch.arange(40) // 5)
    fn = getattr(eb, call)
    with pytest.raises(ValueError, match=">= 1"):
        fn(rows[:2], 0)
    with pytest.raises(ValueError, match="<= 120"):
        fn(rows[:2], 121)
    with pytest.raises(TypeError, match="k must be an int"):
        fn(rows[:2], 2.0)
    with pytest.raises(TypeError, match="k must be an int"):
        fn(rows[:2], True)
    with pytest.raises(ValueError, match="shape"):
        fn(rows[:2, :4], 2)
    with pytest.raises(TypeError, match="floating point"):
        fn(torch.ones(2, 8, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="exclude_group must have shape"):
        fn(rows[:2], 2, exclude_group=torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError, match="integer"):
        fn(rows[:2], 2, exclude_group=torch.tensor([1.0, 2.0]))
    with pytest.raises(TypeError, match="RowFilter"):
        fn(rows[:2], 2, mask=[1, 2])


def test_k_beyond_the_bank_is_refused() -> None:
    eb, rows = _bank(torch.arange(40) // 5)
    with pytest.raises(ValueError, match="bank size"):
        eb.search_groups(rows[:2], 41)
    with pytest.raises(ValueError, match=r"\[1, 40\]"):
        eb.search_groups_exhaustive(rows[:2], 41)
