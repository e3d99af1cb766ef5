"""Per-query group exclusion on the host: the label -> code mapping of `row_groups` / `exclude_group` and the argument
errors.  The device hooks of `EmbeddingBank` are the oracle (tests/groups_oracle.py); the mapping is the product code."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from groups_oracle import oracle, oracle_bank_class  # noqa: E402


def _bank(n: int = 40, labels=None, **kw):
    g = torch.Generator().manual_seed(5)
    rows = torch.nn.functional.normalize(torch.randn(n, 16, generator=g), dim=1).half()
    if labels is None:
        labels = torch.arange(n) // 7 * 10 + 3  # groups of 7 rows, labels 3, 13, 23, ...
    return oracle_bank_class()(rows, dtype=torch.float16, normalize=False, row_groups=labels, **kw), rows, labels


def test_labels_become_codes_of_the_sorted_distinct_labels() -> None:
    labels = torch.tensor([50, -4, 50, 7, 7, 1 << 40, -4, 50], dtype=torch.int64)
    bank, _, _ = _bank(8, labels)
    assert bank.group_labels.tolist() == [-4, 7, 50, 1 << 40]
    assert bank._row_codes.tolist() == [2, 0, 2, 1, 1, 3, 0, 2]
    q = torch.tensor([7, 8, -4, 1 << 40, 51, -5, 50], dtype=torch.int64)
    assert bank._query_codes(q, 7).tolist() == [1, -1, 0, 3, -1, -1, 2]
    assert bank._query_codes(q, 7).dtype == torch.int32
    for dt in (torch.int32, torch.int16, torch.uint8):  # any integer dtype
        assert bank._query_codes(torch.tensor([7, 50, 8], dtype=dt), 3).tolist() == [1, 2, -1]
    assert bank._query_codes(None, 7) is None


def test_grouped_search_skips_each_querys_own_group() -> None:
    bank, rows, labels = _bank()
    queries = (rows[[0, 9, 20, 39]].float() + 0.01).half()
    excl = labels[[0, 9, 20, 39]].clone()
    excl[2] = 999  # a label no row carries excludes nothing
    s, i = bank.search(queries, 5, exclude_group=excl)
    allow = labels.numpy()[None, :] != excl.numpy()[:, None]
    es, ei = oracle(rows, queries, 5, allow)
    np.testing.assert_array_equal(i.numpy(), ei)
    np.testing.assert_array_equal(s.numpy(), es)
    assert not np.isin(i[0].numpy(), np.nonzero(labels.numpy() == labels[0].item())[0]).any()


def test_short_answers_are_padded() -> None:
    labels = torch.zeros(10, dtype=torch.int64)
    labels[:2] = 1
    bank, rows, _ = _bank(10, labels)
    s, i = bank.search(rows[:1].float(), 5, exclude_group=torch.tensor([0]))
    assert i[0, :2].tolist() in ([0, 1], [1, 0]) and i[0, 2:].tolist() == [-1, -1, -1]
    assert torch.isinf(s[0, 2:]).all() and (s[0, 2:] < 0).all()


def test_argument_errors() -> None:
    bank, rows, _ = _bank()
    q = rows[:3].float()
    with pytest.raises(ValueError, match=r"\[Q\] = \[3\]"):
        bank.search(q, 3, exclude_group=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[Q\] = \[3\]"):
        bank.search(q, 3, exclude_group=torch.zeros((3, 1), dtype=torch.int64))
    for dt in (torch.float32, torch.float64, torch.bool):
        with pytest.raises(TypeError, match="integer"):
            bank.search(q, 3, exclude_group=torch.zeros(3, dtype=dt))
    with pytest.raises(TypeError, match="integer"):
        bank.search(q, 3, exclude_group=[1, 2, 3])
    for call in (lambda b: b.search(q, 3, exclude_group=torch.zeros(3, dtype=torch.int64)),
                 lambda b: b.search_async(q, 3, exclude_group=torch.zeros(3, dtype=torch.int64)),
                 lambda b: b.search_exhaustive(q, 3, exclude_group=torch.zeros(3, dtype=torch.int64)),
                 lambda b: b.search_range(q, 0.5, exclude_group=torch.zeros(3, dtype=torch.int64))):
        plain = oracle_bank_class()(rows, dtype=torch.float16, normalize=False)
        with pytest.raises(ValueError, match="row_groups"):
            call(plain)
    for call in (bank.search_exhaustive, bank.search_async):
        with pytest.raises(ValueError, match=r"\[Q\]"):
            call(q, 3, exclude_group=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[Q\]"):
        bank.search_range(q, 0.5, exclude_group=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError, match="integer"):
        _bank(40, torch.zeros(40))
    with pytest.raises(TypeError, match="integer"):
        _bank(40, torch.zeros(40, dtype=torch.bool))
    with pytest.raises(ValueError, match="row_groups"):
        _bank(40, torch.zeros(39, dtype=torch.int64))
