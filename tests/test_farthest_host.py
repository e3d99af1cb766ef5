"""Host-side logic of `EmbeddingBank.farthest_points` and `KMeans(init="farthest")`: validation of `m` and `start`, empty
inputs, the sharded refusal, the `RowFilter` handed to the device hook, output dtypes and shapes.  No device is touched: the
rows stay on the CPU and the `_farthest_rows` hook is the numpy float64 loop of tests/farthest_oracle.py in row order
(packed position = row), as in tests/test_assign_host.py."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import assign_oracle  # noqa: E402
import farthest_oracle  # noqa: E402
from test_assign_host import HostBank as AssignHostBank  # noqa: E402

from imagescry_amd import KMeans, _lib  # noqa: E402
from imagescry_amd.search import RowFilter  # noqa: E402


class HostBank(AssignHostBank):
    def _farthest_rows(self, start, m, mask, out_rows, out_cover, out_near):
        assert start.dtype == torch.int64 and start.ndim == 1
        assert isinstance(m, int) and m > 0
        assert mask is None or isinstance(mask, RowFilter)
        assert out_rows.shape == (m,) and out_rows.dtype == torch.int64
        assert out_cover.shape == (m,) and out_cover.dtype == torch.float32
        assert out_near is None or (out_near.shape == (self.capacity,) and out_near.dtype == torch.float32)
        self.calls.append(("farthest", start.tolist(), m, mask, out_near is not None))
        idx, cover, near, _ = farthest_oracle.greedy(self._bank, m, start.tolist(), self._live_np(), self._live_np(mask))
        out_rows.copy_(torch.from_numpy(idx))
        out_cover.copy_(torch.from_numpy(cover))
        if out_near is not None:
            out_near.copy_(torch.from_numpy(np.where(self._live_np(), near, -math.inf).astype(np.float32)))


def _rows(n: int, d: int = 8, seed: int = 0) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


def _bank(n: int = 10, d: int = 8, **kw) -> HostBank:
    return HostBank(_rows(n, d), dtype=torch.float32, normalize=False, **kw)


def test_shapes_dtypes_and_the_oracle() -> None:
    eb = _bank(12)
    idx, cover = eb.farthest_points(5)
    assert idx.shape == (5,) and idx.dtype == torch.int64 and cover.shape == (5,) and cover.dtype == torch.float32
    exp_i, exp_c, exp_n, _ = farthest_oracle.greedy(eb._bank, 5)
    assert idx.tolist() == exp_i.tolist() and np.array_equal(cover.numpy(), exp_c)
    assert idx[0] == 0 and cover[0] == -math.inf and len(set(idx.tolist())) == 5
    i2, c2, near = eb.farthest_points(5, return_near=True)
    assert torch.equal(i2, idx) and torch.equal(c2, cover)
    assert near.shape == (12,) and near.dtype == torch.float32 and np.array_equal(near.numpy(), exp_n)
    # a prefix, and a resumed call
    i3, c3 = eb.farthest_points(3)
    assert torch.equal(i3, idx[:3]) and torch.equal(c3, cover[:3])
    i4, c4 = eb.farthest_points(2, start=idx[:3])
    assert torch.equal(i4, idx[3:]) and torch.equal(c4, cover[3:])
    i5, _ = eb.farthest_points(2, start=idx[:3].tolist())
    assert torch.equal(i5, idx[3:])
    assert [c[1] for c in eb.calls[-2:]] == [idx[:3].tolist()] * 2
    # more picks than rows: the padding of `search`
    i6, c6 = eb.farthest_points(14)
    assert sorted(i6[:12].tolist()) == list(range(12)) and i6[12:].tolist() == [-1, -1]
    assert (c6[12:] == -math.inf).all()


def test_m_is_validated() -> None:
    eb = _bank(10)
    for bad in (True, False, -1, 2.0, "3", None, _lib.ISC_FARTHEST_MAX_PICKS + 1):
        with pytest.raises(ValueError):
            eb.farthest_points(bad)
    assert _lib.ISC_FARTHEST_MAX_PICKS == 1 << 20
    assert eb.calls == []


def test_start_is_range_checked_on_the_host() -> None:
    eb = _bank(10)
    for bad in ([10], [-1], torch.tensor([3, 11]), torch.tensor([0.5]), torch.tensor([[1]]), torch.tensor([True])):
        with pytest.raises(ValueError):
            eb.farthest_points(2, start=bad)
    with pytest.raises(TypeError):
        eb.farthest_points(2, mask="all")
    other = _bank(10)
    with pytest.raises(ValueError):
        eb.farthest_points(2, mask=other.row_filter(torch.ones(10, dtype=torch.bool)))
    assert eb.calls == []


def test_nothing_to_pick_never_calls_the_hook() -> None:
    eb = _bank(10)
    idx, cover = eb.farthest_points(0)
    assert idx.shape == (0,) and idx.dtype == torch.int64 and cover.shape == (0,) and cover.dtype == torch.float32
    idx, cover, near = eb.farthest_points(0, start=[1], return_near=True)
    assert idx.shape == (0,) and near.shape == (10,) and (near == -math.inf).all()
    empty = HostBank(torch.zeros(0, 8), dtype=torch.float32, normalize=False, capacity=4)
    idx, cover = empty.farthest_points(3)
    assert idx.tolist() == [-1, -1, -1] and idx.dtype == torch.int64
    assert cover.dtype == torch.float32 and (cover == -math.inf).all()
    idx, cover, near = empty.farthest_points(2, return_near=True)
    assert idx.tolist() == [-1, -1] and near.shape == (0,)
    assert eb.calls == [] and empty.calls == []


def test_sharded_banks_refuse() -> None:
    eb = _bank(10)
    eb.process_group = object()
    with pytest.raises(ValueError, match="sharded"):
        eb.farthest_points(3)
    with pytest.raises(ValueError, match="sharded"):
        KMeans(2, init="farthest").fit(eb)
    assert eb.calls == []


def test_the_row_filter_reaches_the_hook() -> None:
    eb = _bank(12)
    allow = torch.zeros(12, dtype=torch.bool)
    allow[[1, 4, 5, 11]] = True
    rf = eb.row_filter(allow)
    idx, cover = eb.farthest_points(5, mask=rf)
    assert eb.calls[-1][3] is rf
    assert sorted(idx[:4].tolist()) == [1, 4, 5, 11] and idx[4] == -1 and idx[0] == 1
    i2, c2 = eb.farthest_points(5, mask=allow)  # a bool tensor is packed into a filter of this bank
    assert isinstance(eb.calls[-1][3], RowFilter) and torch.equal(i2, idx) and torch.equal(c2, cover)
    # a start row outside the mask is a centre and is never picked
    i3, _ = eb.farthest_points(4, start=[0], mask=rf)
    assert 0 not in i3.tolist() and sorted(i3.tolist()) == [1, 4, 5, 11]
    full = _bank(12)
    full.farthest_points(2)
    assert full.calls[-1][3] is None  # no spare room, nothing removed, no mask: no filter
    # removed rows: the fill bitmap is the filter; a removed start row is skipped
    eb.remove(rows=[4])
    with pytest.raises(ValueError):
        eb.farthest_points(2, mask=rf)  # made before the bank changed
    i4, _, near = eb.farthest_points(12, start=[4], return_near=True)
    assert eb.calls[-1][3] is not None and eb.calls[-1][3].packed is eb._fill
    assert i4[0] == 0 and 4 not in i4.tolist() and i4[11] == -1 and near[4] == -math.inf
    live = np.ones(12, dtype=bool)
    live[4] = False
    assert i4.tolist() == farthest_oracle.greedy(eb._bank[:12], 12, [], live)[0].tolist()


def test_kmeans_farthest_init() -> None:
    rows, planted, _ = assign_oracle.planted(clusters=6, per=50, d=32, noise=0.05)
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    km = KMeans(6, init="farthest", seed=123).fit(eb)
    first = eb.calls[0]
    assert first[0] == "farthest" and first[1] == [] and first[2] == 6 and first[3] is None
    picks, _ = eb.farthest_points(6)
    assert sorted((picks // 50).tolist()) == list(range(6))  # one seed per planted cluster
    relabel = torch.empty(6, dtype=torch.int32)
    relabel[(picks // 50)] = torch.arange(6, dtype=torch.int32)
    assert torch.equal(km.labels, relabel[planted.long()])
    again = KMeans(6, init="farthest", seed=7).fit(eb)  # deterministic, the seed is ignored
    assert torch.equal(again.labels, km.labels) and again.objective == km.objective
    # the fit's mask is the selection's mask
    allow = torch.ones(300, dtype=torch.bool)
    allow[::7] = False
    eb.calls.clear()
    km2 = KMeans(6, init="farthest").fit(eb, mask=allow)
    call = eb.calls[0]
    assert call[0] == "farthest" and call[2] == 6 and isinstance(call[3], RowFilter)
    assert np.array_equal(call[3].packed.numpy()[:300], allow.numpy())
    assert (km2.labels[~allow] == -1).all() and int(km2.counts.sum()) == int(allow.sum())
    centres = KMeans(6, init="farthest")._initial_centers(eb, eb.live, 300)
    assert torch.equal(centres, eb._bank[picks])


def test_other_inits_still_raise() -> None:
    with pytest.raises(ValueError, match="farthest"):
        KMeans(2, init="k-means++")
    with pytest.raises(ValueError):
        KMeans(2, init="Farthest")
    assert KMeans(2).init == "sample" and KMeans(2, init="farthest").init == "farthest"
