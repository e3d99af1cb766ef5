"""Host-side logic of `PCA.fit_bank`, `EmbeddingBank.projected_rows` and `EmbeddingBank.project`: argument validation, the
sharded refusal, `mask=` and removed rows reaching the hooks, "fewer than 2 live rows", what `project` carries over to the new
bank, and a planted low-rank data set.  No device is touched: the rows stay on the CPU in row order (packed position = row,
as in tests/test_assign_host.py) and the two device hooks `_gram_rows` / `_project_rows` are answered in float64."""

from __future__ import annotations

import math

import pytest
import torch

from imagescry_amd import PCA, EmbeddingBank
from imagescry_amd.search import RowFilter


class HostBank(EmbeddingBank):
    calls: list

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

    def _code_rows(self, codes):
        return torch.isin(self._row_codes, codes).nonzero().squeeze(1)

    def _pack_filter(self, local):
        return RowFilter(self, torch.nn.functional.pad(local, (0, self.capacity - local.shape[0])), local.sum().reshape(1))

    def _gather_rows(self, index, out):
        live = torch.ones(index.shape, dtype=torch.bool) if self._fill is None else self._fill[index]
        out.copy_(torch.where(live[:, None], self._bank[index], torch.zeros((), dtype=self.dtype)))

    def _live_rows(self, mask):
        if mask is not None:
            return mask.packed.clone()
        return torch.ones(self.capacity, dtype=torch.bool) if self._fill is None else self._fill.clone()

    def _group_sums(self, rows, offsets, sums, counts):
        live = self._live_rows(None)
        for g in range(counts.numel()):
            members = [r for r in rows[int(offsets[g]) : int(offsets[g + 1])].tolist() if live[r]]
            counts[g] = len(members)
            cols = self._bank[members].double().T.tolist() if members else [[0.0]] * self.dim
            sums[g] = torch.tensor([math.fsum(col) for col in cols], dtype=torch.float64)

    # ---- the two new hooks, in row order and float64
    def _gram_rows(self, mean, mask, gram, count):
        assert mean.shape == (self.dim,) and mean.dtype == torch.float32
        assert mask is None or isinstance(mask, RowFilter)
        assert gram.shape == (self.dim, self.dim) and gram.dtype == torch.float64 and not gram.any()
        assert count.shape == (1,) and count.dtype == torch.int64 and int(count) == 0
        live = self._live_rows(mask)
        self.calls.append(("gram", live[: self.num_local_rows].nonzero().squeeze(1).tolist()))
        a = (self._bank[live].float() - mean).double()  # one float32 subtraction, then exact
        gram.copy_(a.T @ a)
        count[0] = int(live.sum())

    def _project_rows(self, mean, w, mask, out_rows, out_bank):
        k = w.shape[1]
        assert mean.shape == (self.dim,) and mean.dtype == torch.float32
        assert w.shape[0] == self.dim and w.dtype == torch.float32 and w.stride(1) == 1
        assert out_rows is not None or out_bank is not None
        live = self._live_rows(mask)
        self.calls.append(("project", live[: self.num_local_rows].nonzero().squeeze(1).tolist(), k))
        p = ((self._bank.float() - mean).double() @ w.double()).float()
        p[~live] = 0
        if out_rows is not None:
            assert out_rows.shape == (self.capacity, k) and out_rows.dtype == torch.float32
            out_rows.copy_(p)
        if out_bank is not None:
            assert out_bank.dim == k and out_bank.capacity == self.capacity and not out_bank._bank.any()
            if out_bank.normalize:
                p = torch.nn.functional.normalize(p, dim=1)
            out_bank._bank[live] = p[live]


def _data(n: int = 40, d: int = 8, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g) * torch.linspace(3.0, 0.5, d) + 2.0


def _bank(n: int = 40, d: int = 8, **kw) -> HostBank:
    return HostBank(_data(n, d), dtype=torch.float32, normalize=False, **kw)


def _ref_pca(rows: torch.Tensor, **kw) -> PCA:
    """The same host tail on the float64 Gram of the float32-centred rows."""
    rows = rows.float()
    n, f = rows.shape
    mean = (rows.double().sum(dim=0) / n).float()
    a = (rows - mean).double()
    return PCA(**kw)._finish_fit(a.T @ a, n, f, mean, torch.device("cpu"))


def _same(a: PCA, b: PCA) -> None:
    assert a.num_components == b.num_components and a.num_features == b.num_features
    assert torch.equal(a.feature_means, b.feature_means)
    assert torch.equal(a.explained_variance, b.explained_variance)
    assert torch.equal(a.component_vectors, b.component_vectors)


def test_fit_bank_is_fit_on_the_stored_rows() -> None:
    eb = _bank(40)
    pca = PCA(min_num_components=3).fit_bank(eb)
    assert pca.fitted and pca.num_features == 8 and pca.num_components == 3
    assert pca.feature_means.shape == (1, 8) and pca.feature_means.dtype == torch.float32
    assert pca.component_vectors.shape == (8, 3) and pca.explained_variance.shape == (8,)
    _same(pca, _ref_pca(eb._bank, min_num_components=3))
    assert eb.calls == [("gram", list(range(40)))]
    assert abs(float(pca.explained_variance.sum()) - 1.0) < 1e-5
    assert bool((pca.explained_variance[:-1] >= pca.explained_variance[1:]).all())


def test_removed_rows_spare_capacity_and_masks_reach_the_hooks() -> None:
    eb = _bank(40, capacity=64)
    eb.remove(rows=[3, 17, 17, 39])
    keep = [r for r in range(40) if r not in (3, 17, 39)]
    pca = PCA(min_num_components=2).fit_bank(eb)
    assert eb.calls[-1] == ("gram", keep)
    _same(pca, _ref_pca(eb._bank[keep], min_num_components=2))
    # a mask (bool tensor or RowFilter) on top of the removal
    allow = torch.zeros(40, dtype=torch.bool)
    allow[::2] = True
    allow[3] = True  # removed: a filter never allows it
    allowed = [r for r in keep if r % 2 == 0]
    for mask in (allow, eb.row_filter(allow)):
        masked = PCA(min_num_components=2).fit_bank(eb, mask=mask)
        assert eb.calls[-1] == ("gram", allowed)
        _same(masked, _ref_pca(eb._bank[allowed], min_num_components=2))
    # the projections see the fill bitmap: removed rows are zeros, the rest is transform's product
    out = eb.projected_rows(pca)
    assert eb.calls[-1] == ("project", keep, 2)
    assert out.shape == (40, 2) and out.dtype == torch.float32
    assert not out[[3, 17, 39]].any()
    want = ((eb._bank[:40] - pca.feature_means).double() @ pca.component_vectors.double()).float()
    assert torch.equal(out[keep], want[keep])
    stale = eb.row_filter(allow)
    eb.remove(rows=[0])
    with pytest.raises(ValueError):
        PCA().fit_bank(eb, mask=stale)
    with pytest.raises(ValueError):
        PCA().fit_bank(eb, mask=_bank(40).row_filter(torch.ones(40, dtype=torch.bool)))
    with pytest.raises(TypeError):
        PCA().fit_bank(eb, mask="all")


def test_fewer_than_two_live_rows() -> None:
    with pytest.raises(ValueError, match="at least 2"):
        PCA().fit_bank(HostBank(torch.zeros(0, 8), dtype=torch.float32, normalize=False, capacity=4))
    with pytest.raises(ValueError, match="at least 2"):
        PCA().fit_bank(_bank(1))
    eb = _bank(5)
    eb.remove(rows=[0, 1, 2, 4])
    with pytest.raises(ValueError, match="at least 2"):
        PCA().fit_bank(eb)
    eb2 = _bank(5)
    only = torch.zeros(5, dtype=torch.bool)
    only[2] = True
    with pytest.raises(ValueError, match="at least 2"):
        PCA().fit_bank(eb2, mask=only)
    assert eb.calls == [] and eb2.calls == []  # no Gram launch behind a refusal
    only[4] = True
    assert PCA().fit_bank(eb2, mask=only).fitted


def test_argument_validation() -> None:
    eb = _bank(20)
    pca = PCA(min_num_components=2).fit_bank(eb)
    eb.calls.clear()
    for call in (eb.projected_rows, eb.project):
        with pytest.raises(ValueError, match="not fitted"):
            call(PCA())
        with pytest.raises(ValueError, match="features"):
            call(PCA(min_num_components=2).fit_bank(_bank(20, d=6)))
        with pytest.raises(ValueError, match="device|pca.to"):
            call(PCA(min_num_components=2).fit_bank(_bank(20)).to("meta"))
        with pytest.raises(ValueError):
            call(None)
    with pytest.raises(ValueError, match="dtype"):
        eb.project(pca, dtype=torch.bfloat16)
    assert eb.calls == []


def test_sharded_banks_refuse() -> None:
    eb = _bank(20)
    pca = PCA(min_num_components=2).fit_bank(eb)
    eb.calls.clear()
    eb.process_group = object()
    for call in (lambda: eb.projected_rows(pca), lambda: eb.project(pca), lambda: PCA().fit_bank(eb)):
        with pytest.raises(ValueError, match="sharded"):
            call()
    assert eb.calls == []


def test_project_carries_the_bank_over() -> None:
    rows = _data(30)
    groups = torch.arange(30) // 4 + 100
    eb = HostBank(rows, dtype=torch.float32, normalize=False, row_groups=groups, capacity=48)
    eb.row_origin = torch.stack([groups, torch.arange(30) % 4, torch.zeros(30, dtype=torch.int64)], dim=1)
    eb.remove(rows=[5, 6])
    pca = PCA(min_num_components=3).fit_bank(eb)
    proj = eb.project(pca, normalize=False)
    assert type(proj) is HostBank and proj.dim == 3 and proj.dtype == eb.dtype and proj.normalize is False
    assert len(proj) == 30 and proj.capacity == 48 and proj.num_removed == 2 and proj.index_base == 0
    assert torch.equal(proj._fill, eb._fill) and proj._fill is not eb._fill
    assert torch.equal(proj.live, eb.live)
    assert torch.equal(proj.row_origin, eb.row_origin) and proj.row_origin is not eb.row_origin
    assert torch.equal(proj.group_labels, eb.group_labels) and torch.equal(proj._row_codes, eb._row_codes)
    assert proj._row_codes is not eb._row_codes and torch.equal(proj._group_counts, eb._group_counts)
    assert proj._max_group_rows == eb._max_group_rows
    assert torch.equal(proj.rows(torch.arange(30)), eb.projected_rows(pca))
    assert proj.project(PCA(min_num_components=2).fit_bank(proj), dtype=torch.float16).dtype == torch.float16
    # the new bank is a bank of its own: it appends and removes without touching the source
    new = proj.append(torch.ones(2, 3), row_groups=torch.tensor([100, 999]),
                      row_origin=torch.tensor([[100, 9, 9], [999, 0, 0]]))
    assert list(new) == [30, 31] and len(proj) == 32 and len(eb) == 30
    assert proj.remove(groups=[100]) == 5 and proj.num_removed == 7 and eb.num_removed == 2
    assert int(eb._fill.sum()) == 28 and eb.group_labels.numel() == 8 and proj.group_labels.numel() == 9
    filt = proj.row_filter(torch.ones(32, dtype=torch.bool))  # a filter of the new bank belongs to the new bank
    assert filt.belongs_to(proj) and not filt.belongs_to(eb)
    # normalised storage, and a bank that never reserved anything stays one
    plain = _bank(12)
    unit = plain.project(PCA(min_num_components=2).fit_bank(plain))
    assert unit.normalize is True and unit._fill is None and unit._capacity is None and unit.capacity == len(unit) == 12
    assert torch.allclose(unit._bank.norm(dim=1), torch.ones(12), atol=1e-6)
    empty = HostBank(torch.zeros(0, 8), dtype=torch.float32, normalize=False)
    assert len(empty.project(pca)) == 0 and empty.project(pca).dim == 3
    assert empty.projected_rows(pca).shape == (0, 3)


def test_planted_rank_is_found() -> None:
    g = torch.Generator().manual_seed(7)
    basis = torch.linalg.qr(torch.randn(24, 5, generator=g))[0]
    rows = (torch.randn(400, 5, generator=g) * torch.tensor([9.0, 7.0, 5.0, 4.0, 3.0])) @ basis.T
    rows = rows + 1e-3 * torch.randn(400, 24, generator=g) + 5.0
    eb = HostBank(rows, dtype=torch.float32, normalize=False)
    pca = PCA(min_explained_variance=0.999).fit_bank(eb)
    assert pca.num_components == 5
    # the planted subspace: its basis is reproduced by the components
    resid = basis - pca.component_vectors @ (pca.component_vectors.T @ basis)
    assert float(resid.abs().max()) < 1e-3
    out = eb.projected_rows(pca)
    assert out.shape == (400, 5)
    assert torch.allclose(out.var(dim=0), torch.tensor([81.0, 49.0, 25.0, 16.0, 9.0]), rtol=0.25)
