"""Host-side logic of `EmbeddingBank.assign` / `assign_exhaustive` / `group_sums` and of `KMeans`: argument validation,
dtypes and shapes, dead rows, `mask=`, the sharded refusal, empty inputs; the k-means loop's seeded sampling, empty clusters,
stopping rules and a planted clustering.  No device is touched: the rows stay on the CPU and the two device hooks are the
float64 oracle of tests/assign_oracle.py in row order (packed position = row), as in tests/test_rows_host.py."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import assign_oracle  # noqa: E402

from imagescry_amd import EmbeddingBank, KMeans  # noqa: E402
from imagescry_amd.search import RowFilter  # noqa: E402


class HostBank(EmbeddingBank):
    calls: list

    def _store(self, embeddings, normalize):
        self._norm_bound = torch.zeros(1)
        self.calls = []
        return embeddings.clone()

    def _alloc_image(self, capacity, device, grouped):
        self.calls = []
        return torch.zeros(capacity, self.dim), torch.zeros(capacity, dtype=torch.bool), None

    def _append_rows(self, embeddings, first_row, normalize, codes):
        hi = first_row + embeddings.shape[0]
        self._bank[first_row:hi] = embeddings
        self._fill[first_row:hi] = True

    def _remove_rows(self, index, removed):
        for r in index.tolist():
            if 0 <= r < self.num_local_rows and self._fill[r]:
                self._fill[r] = False
                removed += 1

    def _unpack_mask(self, packed, n_rows):
        return packed[:n_rows].clone()

    def _pack_filter(self, local):
        return RowFilter(self, torch.nn.functional.pad(local, (0, self.capacity - local.shape[0])), local.sum().reshape(1))

    def _gather_rows(self, index, out):
        out.copy_(self._bank[index])

    def _live_np(self, mask=None):
        n = self.capacity
        live = np.ones(n, dtype=bool) if self._fill is None else self._fill.numpy().copy()
        if mask is not None:
            live = mask.packed.numpy().copy()
        return live

    # ---- the two new hooks, in row order
    def _assign_rows(self, q, mask, labels, scores, exhaustive):
        assert q.ndim == 2 and q.shape[0] > 0 and q.shape[1] == self.dim
        assert mask is None or isinstance(mask, RowFilter)
        assert labels.shape == (self.capacity,) and labels.dtype == torch.int32
        assert scores is None or (scores.shape == (self.capacity,) and scores.dtype == torch.float32)
        self.calls.append(("assign", q.shape[0], mask is not None, scores is not None, exhaustive))
        lab, sc = assign_oracle.assign(self._bank, q, self._live_np(mask))
        labels.copy_(torch.from_numpy(lab))
        if scores is not None:
            scores.copy_(torch.from_numpy(sc))

    def _group_sums(self, rows, offsets, sums, counts):
        assert rows.dtype == torch.int64 and offsets.dtype == torch.int64 and offsets.shape == (counts.numel() + 1,)
        assert sums.dtype == torch.float64 and sums.shape == (counts.numel(), self.dim) and counts.dtype == torch.int64
        assert int(offsets[0]) == 0 and bool((offsets[1:] >= offsets[:-1]).all()) and int(offsets[-1]) <= rows.numel()
        self.calls.append(("sums", counts.numel()))
        live = self._live_np()
        b = self._bank.numpy().astype(np.float64)
        for g in range(counts.numel()):
            members = [r for r in rows[int(offsets[g]) : int(offsets[g + 1])].tolist() if live[r]]
            assert members == sorted(members)  # a stable sort: the rows of a group in row order
            counts[g] = len(members)
            sums[g] = torch.from_numpy(np.array([math.fsum(col) for col in b[members].T]) if members
                                       else np.zeros(self.dim))


def _rows(n: int, d: int = 8, seed: int = 0) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


def _bank(n: int = 10, d: int = 8, **kw) -> HostBank:
    return HostBank(_rows(n, d), dtype=torch.float32, normalize=False, **kw)


def test_assign_shapes_dtypes_and_the_oracle() -> None:
    eb = _bank(10)
    cent = _rows(3, seed=1)
    labels, scores = eb.assign(cent)
    assert labels.shape == (10,) and labels.dtype == torch.int32
    assert scores.shape == (10,) and scores.dtype == torch.float32
    lab, sc = assign_oracle.assign(eb._bank, cent)
    assert np.array_equal(labels.numpy(), lab) and np.array_equal(scores.numpy(), sc)
    l2, s2 = eb.assign(cent, return_scores=False)
    assert s2 is None and torch.equal(l2, labels)
    l3, s3 = eb.assign_exhaustive(cent)
    assert torch.equal(l3, labels) and torch.equal(s3, scores)
    assert [c[4] for c in eb.calls] == [False, False, True]
    # float64 centroids are converted to the bank dtype, non-contiguous ones made contiguous
    l4, _ = eb.assign(cent.double())
    l5, _ = eb.assign(torch.cat([cent, cent], dim=1)[:, :8])
    assert torch.equal(l4, labels) and torch.equal(l5, labels)


def test_assign_argument_validation() -> None:
    eb = _bank(10)
    with pytest.raises(TypeError):
        eb.assign([[0.0] * 8])
    with pytest.raises(TypeError):
        eb.assign(torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        eb.assign(torch.zeros(2, 7))
    with pytest.raises(ValueError):
        eb.assign(torch.zeros(8))
    with pytest.raises(ValueError):
        eb.assign(torch.zeros(0, 8))  # no centroid: a row has no label
    with pytest.raises(TypeError):
        eb.assign(_rows(2), mask="all")
    other = _bank(10)
    with pytest.raises(ValueError):
        eb.assign(_rows(2), mask=other.row_filter(torch.ones(10, dtype=torch.bool)))
    assert eb.calls == []


def test_dead_rows_get_minus_one_and_minus_inf() -> None:
    eb = _bank(10, capacity=16)
    cent = _rows(4, seed=2)
    eb.remove(rows=[3, 7])
    labels, scores = eb.assign(cent)
    assert labels.shape == (10,)
    assert labels[[3, 7]].tolist() == [-1, -1] and torch.isinf(scores[[3, 7]]).all() and (scores[[3, 7]] < 0).all()
    live = np.ones(10, dtype=bool)
    live[[3, 7]] = False
    lab, sc = assign_oracle.assign(eb._bank[:10], cent, live)
    assert np.array_equal(labels.numpy(), lab) and np.array_equal(scores.numpy(), sc)
    assert eb.calls[-1][2] is True  # the fill bitmap is the row mask


def test_mask_limits_the_rows() -> None:
    eb = _bank(12)
    cent = _rows(3, seed=3)
    allow = torch.zeros(12, dtype=torch.bool)
    allow[[1, 4, 5, 11]] = True
    full, _ = eb.assign(cent)
    for mask in (allow, eb.row_filter(allow)):
        labels, scores = eb.assign(cent, mask=mask)
        assert torch.equal(labels[allow], full[allow]) and (labels[~allow] == -1).all()
        assert torch.isinf(scores[~allow]).all() and torch.isfinite(scores[allow]).all()
    stale = eb.row_filter(allow)
    eb.remove(rows=[0])
    with pytest.raises(ValueError):
        eb.assign(cent, mask=stale)


def test_sharded_banks_refuse() -> None:
    eb = _bank(10)
    eb.process_group = object()
    for call in (lambda: eb.assign(_rows(2)), lambda: eb.assign_exhaustive(_rows(2)),
                 lambda: eb.group_sums(torch.zeros(10, dtype=torch.int64), 2)):
        with pytest.raises(ValueError, match="sharded"):
            call()
    with pytest.raises(ValueError, match="sharded"):
        KMeans(2).fit(eb)
    assert eb.calls == []


def test_empty_inputs() -> None:
    eb = HostBank(torch.zeros(0, 8), dtype=torch.float32, normalize=False, capacity=4)
    labels, scores = eb.assign(_rows(2))
    assert labels.shape == (0,) and labels.dtype == torch.int32 and scores.shape == (0,)
    sums, counts = eb.group_sums(torch.zeros(0, dtype=torch.int64), 3)
    assert sums.shape == (3, 8) and not sums.any() and counts.tolist() == [0, 0, 0]
    eb2 = _bank(5)
    sums, counts = eb2.group_sums(torch.zeros(5, dtype=torch.int64), 0)
    assert sums.shape == (0, 8) and counts.shape == (0,)
    assert eb.calls == [] and eb2.calls == []


def test_group_sums_validation_and_semantics() -> None:
    eb = _bank(9, capacity=12)
    for bad in (torch.zeros(8, dtype=torch.int64), torch.zeros(9), torch.zeros(9, dtype=torch.bool),
                torch.zeros((9, 1), dtype=torch.int64), [0] * 9):
        with pytest.raises(ValueError):
            eb.group_sums(bad, 2)
    for g in (-1, 1.5, True):
        with pytest.raises(ValueError):
            eb.group_sums(torch.zeros(9, dtype=torch.int64), g)
    labels = torch.tensor([2, 0, 0, -1, 2, 5, 1, 2, 0], dtype=torch.int32)
    eb.remove(rows=[4])
    sums, counts = eb.group_sums(labels, 4)
    assert sums.dtype == torch.float64 and sums.shape == (4, 8) and counts.dtype == torch.int64
    assert counts.tolist() == [3, 1, 2, 0]  # -1 and 5 are outside [0, 4); row 4 is removed
    live = np.ones(9, dtype=bool)
    live[4] = False
    exp_s, exp_c = assign_oracle.group_sums(eb._bank[:9], labels.numpy(), 4, live)
    assert np.array_equal(counts.numpy(), exp_c) and np.array_equal(sums.numpy(), exp_s)


# ------------------------------------------------------------------ KMeans
def test_kmeans_argument_validation() -> None:
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            KMeans(bad)
    with pytest.raises(ValueError):
        KMeans(2, max_iter=0)
    with pytest.raises(ValueError):
        KMeans(2, tol=-1.0)
    with pytest.raises(ValueError):
        KMeans(2, init="k-means++")
    with pytest.raises(ValueError):
        KMeans(2, init=torch.zeros(3, 8))
    with pytest.raises(ValueError):
        KMeans(2, init=torch.zeros(2, 7)).fit(_bank(10))
    with pytest.raises(ValueError, match="live rows"):
        KMeans(11).fit(_bank(10))
    eb = _bank(10)
    eb.remove(rows=[0, 1])
    with pytest.raises(ValueError, match="live rows"):
        KMeans(9).fit(eb)
    with pytest.raises(RuntimeError):
        KMeans(2).predict(eb)


def test_init_sampling_is_seeded_distinct_and_live() -> None:
    eb = _bank(40)
    eb.remove(rows=list(range(0, 40, 3)))
    live = eb.live
    seen = []
    for seed in (0, 0, 1):
        km = KMeans(8, seed=seed, max_iter=1)
        centers = km._initial_centers(eb, live, int(live.sum()))
        assert centers.shape == (8, 8) and centers.dtype == torch.float32
        match = (centers[:, None, :] == eb._bank[None, :40, :]).all(dim=2)
        picked = match.float().argmax(dim=1)
        assert match.any(dim=1).all() and len(set(picked.tolist())) == 8 and live[picked].all()
        seen.append(picked.tolist())
    assert seen[0] == seen[1] and seen[0] != seen[2]


def test_empty_cluster_keeps_its_centroid() -> None:
    rows, _, first = assign_oracle.planted(clusters=3, per=20, d=16)
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    far = -first.sum(dim=0, keepdim=True)  # no row is nearest to it
    km = KMeans(4, init=torch.cat([first, far]), max_iter=5).fit(eb)
    assert km.counts.tolist() == [20, 20, 20, 0]
    assert torch.equal(km.cluster_centers[3], far[0].float())
    assert torch.allclose(km.cluster_centers[:3].norm(dim=1), torch.ones(3), atol=1e-6)


def test_stopping_rules() -> None:
    rows, _, first = assign_oracle.planted()
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    # no label changed: the second assignment repeats the first
    km = KMeans(6, init=first).fit(eb)
    assert km.num_iter == 2 and len(km.objective) == 2
    # max_iter
    g = torch.Generator().manual_seed(5)
    noisy = HostBank(torch.nn.functional.normalize(torch.randn(300, 16, generator=g), dim=1), dtype=torch.float32,
                     normalize=False)
    km1 = KMeans(5, max_iter=1).fit(noisy)
    assert km1.num_iter == 1 and len(km1.objective) == 1
    km3 = KMeans(5, max_iter=3, tol=0.0).fit(noisy)
    assert km3.num_iter <= 3 and len(km3.objective) == km3.num_iter
    assert torch.equal(km3.predict(noisy), km3.labels)  # the labels belong to the centroids that are kept
    # tol: a huge tolerance stops after the second objective
    kt = KMeans(5, max_iter=10, tol=10.0).fit(noisy)
    assert kt.num_iter == 2
    full = KMeans(5, max_iter=25, tol=0.0).fit(noisy)
    obj = np.array(full.objective)
    assert (np.diff(obj) >= -1e-12).all()
    assert [c[0] for c in noisy.calls[:4]] == ["assign", "sums", "assign", "sums"]
    assert all(c[3] is False for c in noisy.calls if c[0] == "assign")  # labels only: no per-row scores


def test_planted_clusters_are_recovered() -> None:
    rows, planted, first = assign_oracle.planted(clusters=6, per=50, d=32, noise=0.05)
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    km = KMeans(6, init=first).fit(eb)
    assert torch.equal(km.labels, planted)
    assert km.num_iter == 2  # converged after one update
    assert km.counts.tolist() == [50] * 6
    assert km.cluster_centers.shape == (6, 32) and km.cluster_centers.dtype == torch.float32
    assert (np.diff(np.array(km.objective)) >= -1e-12).all() and km.objective[-1] > 0.9
    assert torch.equal(km.predict(eb), planted)
    # a mask clusters the allowed rows only
    allow = torch.ones(300, dtype=torch.bool)
    allow[::7] = False
    km2 = KMeans(6, init=first).fit(eb, mask=allow)
    assert torch.equal(km2.labels[allow], planted[allow]) and (km2.labels[~allow] == -1).all()
    assert int(km2.counts.sum()) == int(allow.sum())
