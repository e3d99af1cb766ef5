"""`isc_bank_gram` / `isc_bank_project` behind `PCA.fit_bank`, `EmbeddingBank.projected_rows` and `EmbeddingBank.project`.

Two references, neither of them measured (tests/matmul_bound.py):

- exact integers.  Rows `[c + R; c - R]` (c integers in [-8, 8], R integers in [-4, 4], shuffled, stored unnormalised): the
  mean is c exactly, every centred value is an integer and every partial sum stays below 2^24, which
  `assert_exact_range` confirms on the operands: the kernel must EQUAL the float64 product in any summation order;
- real values under `product_bound`, with a mean as large as the spread, which an un-centred `sum x x^T - n mu mu^T` would
  not meet.

Shapes cover one row pair, the 256-row tile and its remainder, partial K steps of both dtypes (72 fp16, 200 fp32 features),
several 128-feature Gram tiles (768, 1280), the seam between two partial Grams (chunk + 300 rows) and every LDS budget of
the projection (K = 1 ... 1280).  Each is run on a plain bank, on one with spare capacity (dead slots share tiles with live
rows) and after removing row pairs (stale vectors stay in the image).  The packed output is compared bit for bit with the
bank built from the projected rows."""

from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
DEV = "cuda:0"
STATES = ("plain", "capacity", "removed")


@lru_cache(maxsize=None)
def _chunk() -> int:
    from imagescry_amd import _lib

    return _lib.load().isc_bank_gram_chunk_rows()


def _shape_id(s) -> str:
    return f"{s[0]}x{s[1]}-{'f16' if s[2] is F16 else 'f32'}"


SEAM = "chunk+300"  # rows: one partial Gram and 300 rows of the next (the chunk is the library's to tell)
GRAM_SHAPES = ((2, 8, F16), (256, 64, F16), (258, 72, F16), (258, 200, F32), (700, 768, F16), (SEAM, 72, F16),
               (510, 1280, F32))
PROJ_SHAPES = ((2, 8, F16), (256, 64, F16), (258, 72, F16), (258, 200, F32), (700, 768, F16), (510, 1280, F32))


@lru_cache(maxsize=None)
def _int_rows(n: int, d: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rows [n, d] float32, c [d], partner [n]: the row that mirrors row i about c)."""
    g = torch.Generator().manual_seed(1000 * n + d)
    c = mb.int_tensor((d,), -8, 8, g)
    r = mb.int_tensor((n // 2, d), -4, 4, g)
    x0 = torch.cat([c + r, c - r])
    order = torch.randperm(n, generator=g)
    inv = torch.empty(n, dtype=torch.int64)
    inv[order] = torch.arange(n)
    partner0 = torch.cat([torch.arange(n // 2) + n // 2, torch.arange(n // 2)])
    return x0[order], c, inv[partner0[order]]


def _pair_rows(n: int, partner: torch.Tensor, modulus: int, residue: int) -> torch.Tensor:
    """Every `modulus`-th row pair (a row and its mirror), as row indices."""
    first = torch.arange(n)[torch.arange(n) < partner]  # one representative per pair
    pick = first[residue::modulus]
    return torch.cat([pick, partner[pick]])


@lru_cache(maxsize=None)
def _int_bank(n: int, d: int, dtype: torch.dtype, state: str):
    """(bank, live bool [n] on the host) of the exact-integer rows in one of the three states."""
    from imagescry_amd import EmbeddingBank

    x, _, partner = _int_rows(n, d)
    kw = {} if state == "plain" else {"capacity": n + 300}
    eb = EmbeddingBank(x.to(DEV), dtype=dtype, normalize=False, **kw)
    live = torch.ones(n, dtype=torch.bool)
    if state == "removed":
        gone = _pair_rows(n, partner, 7, 3)
        if gone.numel():
            assert eb.remove(rows=gone) == gone.numel()
            live[gone] = False
    return eb, live


def _gram(eb, mean: torch.Tensor, rf) -> tuple[torch.Tensor, int]:
    gram = torch.zeros((eb.dim, eb.dim), dtype=torch.float64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    eb._gram_rows(mean.to(DEV), rf, gram, count)
    return gram.cpu(), int(count)


# ------------------------------------------------------------------------------------------------ 1. Gram, exact integers
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("shape", GRAM_SHAPES, ids=_shape_id)
def test_gram_equals_the_float64_gram_on_exact_integers(shape, state, device) -> None:
    n, d, dtype = shape
    n = _chunk() + 300 if n == SEAM else n
    x, c, _ = _int_rows(n, d)
    eb, live = _int_bank(n, d, dtype, state)
    a = x[live] - c  # integers
    at = a.T.contiguous()
    top = mb.assert_exact_range(at, at)
    want = mb.product_f64(at, at)
    got, count = _gram(eb, c, eb._as_filter(None))
    print(f"{_shape_id(shape)} {state}: {int(live.sum())} live rows, largest partial sum {top:.0f}")
    assert count == int(live.sum())
    assert torch.equal(got, want)
    assert torch.equal(got, got.T)
    again, _ = _gram(eb, c, eb._as_filter(None))
    assert torch.equal(got, again)  # the same bits on the same inputs


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("shape", ((258, 72, F16), (700, 768, F16), (258, 200, F32)), ids=_shape_id)
def test_gram_of_a_masked_half_set(shape, state, device) -> None:
    n, d, dtype = shape
    x, c, partner = _int_rows(n, d)
    eb, live = _int_bank(n, d, dtype, state)
    allow = torch.zeros(n, dtype=torch.bool)
    allow[_pair_rows(n, partner, 2, 0)] = True  # whole mirrored pairs: the mean of the allowed rows is still c
    rf = eb.row_filter(allow.to(DEV))
    keep = allow & live
    at = (x[keep] - c).T.contiguous()
    mb.assert_exact_range(at, at)
    got, count = _gram(eb, c, rf)
    assert count == int(keep.sum()) and 0 < count < int(live.sum())
    assert torch.equal(got, mb.product_f64(at, at))


# ------------------------------------------------------------------------------------------------ 2. Gram, real values
@lru_cache(maxsize=None)
def _real_bank(n: int, d: int, dtype: torch.dtype, state: str):
    """(bank, stored rows [n, d] float32 on the host, live [n]): randn + 3, unnormalised, in one of the three states."""
    from imagescry_amd import EmbeddingBank

    g = torch.Generator().manual_seed(7 * n + d)
    x = torch.randn(n, d, generator=g) + 3.0
    kw = {} if state == "plain" else {"capacity": n + 300}
    eb = EmbeddingBank(x.to(DEV), dtype=dtype, normalize=False, **kw)
    live = torch.ones(n, dtype=torch.bool)
    if state == "removed":
        live[3::7] = False
        eb.remove(rows=(~live).nonzero().squeeze(1))
    return eb, x.to(dtype).float(), live


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("shape", ((1000, 72, F16), (1000, 200, F32), (1024, 768, F16)), ids=_shape_id)
def test_gram_of_real_rows_is_within_the_product_bound(shape, state, device) -> None:
    n, d, dtype = shape
    eb, stored, live = _real_bank(n, d, dtype, state)
    rows = stored[live]
    mean = (rows.double().sum(dim=0) / rows.shape[0]).float()
    at = (rows - mean).T.contiguous()  # the centred operand as the kernel forms it: one float32 subtraction
    want, bound = mb.product_f64(at, at), mb.product_bound(at, at)
    got, count = _gram(eb, mean, eb._as_filter(None))
    assert count == rows.shape[0]
    ratio = mb.assert_within_bound(got, want, bound, "centred Gram")
    print(f"{_shape_id(shape)} {state}: worst error / bound = {ratio:.3f}")
    assert torch.equal(got, got.T)


# ------------------------------------------------------------------------------------------------ 3. projection
SENTINEL = 12345.0


def _project_into_sentinel(eb, mean: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """`out_rows` as a view inside a sentinel-filled buffer: returns the [capacity, K] view after checking that nothing
    around it was written."""
    k = w.shape[1]
    buf = torch.full((eb.capacity + 2, k + 3), SENTINEL, dtype=F32, device=DEV)
    view = buf[1 : eb.capacity + 1, 1 : k + 1]
    eb._project_rows(mean.to(DEV), w.to(DEV).contiguous(), eb._as_filter(None), view, None)
    out = view.cpu().clone()
    host = buf.cpu()
    host[1 : eb.capacity + 1, 1 : k + 1] = SENTINEL
    assert bool((host == SENTINEL).all()), "written outside [N, K]"
    return out


def _ks(d: int) -> list[int]:
    return sorted({k for k in (1, 3, 64, d) if k <= d})


_PROJ_CASES = [(s, k) for s in PROJ_SHAPES for k in _ks(s[1])]


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("shape,k", _PROJ_CASES, ids=lambda v: _shape_id(v) if isinstance(v, tuple) else f"k{v}")
def test_projection_equals_the_float64_product_on_exact_integers(shape, k, state, device) -> None:
    n, d, dtype = shape
    x, c, _ = _int_rows(n, d)
    eb, live = _int_bank(n, d, dtype, state)
    w = mb.int_tensor((d, k), -3, 3, torch.Generator().manual_seed(d + k))
    a = x - c
    wt = w.T.contiguous()
    mb.assert_exact_range(a, wt)
    want = mb.product_f64(a, wt)
    want[~live] = 0.0
    out = _project_into_sentinel(eb, c, w)
    assert out.shape == (eb.capacity, k)
    assert torch.equal(out[:n].double(), want)
    assert not out[n:].any()  # the unused capacity: dead rows, written as zeros


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("shape", ((600, 72, F16), (600, 200, F32), (600, 768, F16), (600, 1024, F32)), ids=_shape_id)
def test_projection_of_real_rows_is_within_the_product_bound(shape, state, device) -> None:
    n, d, dtype = shape
    eb, stored, live = _real_bank(n, d, dtype, state)
    mean = (stored[live].double().sum(dim=0) / int(live.sum())).float()
    a = stored - mean
    for k in _ks(d):
        w = torch.randn(d, k, generator=torch.Generator().manual_seed(k))
        wt = w.T.contiguous()
        want, bound = mb.product_f64(a, wt), mb.product_bound(a, wt)
        out = _project_into_sentinel(eb, mean, w)[:n]
        ratio = mb.assert_within_bound(out[live], want[live], bound[live], f"projection K={k}")
        print(f"{_shape_id(shape)} {state} K={k}: worst error / bound = {ratio:.3f}")
        assert not out[~live].any()


# ------------------------------------------------------------------------------------------------ 4. packed output
def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.dtype.is_floating_point:
        return bool(torch.equal(a, b))
    view = torch.int16 if a.dtype == F16 else torch.int32
    return bool(torch.equal(a.view(view), b.view(view)))


def _same_answers(proj, twin, q: torch.Tensor, image_id: int) -> None:
    n = len(proj)
    assert len(twin) == n and proj.capacity == twin.capacity and proj.num_removed == twin.num_removed
    every = torch.arange(n, device=DEV)
    assert _bits_equal(proj.rows(every), twin.rows(every))
    assert _bits_equal(proj._norm_bound, twin._norm_bound)
    for a, b in zip(proj.search(q, 10), twin.search(q, 10)):
        assert _bits_equal(a, b)
    labels = proj.group_labels[torch.arange(q.shape[0], device=DEV) % proj.group_labels.numel()]
    for a, b in zip(proj.search(q, 10, exclude_group=labels), twin.search(q, 10, exclude_group=labels)):
        assert _bits_equal(a, b)
    for a, b in zip(proj.search_groups(q, 5), twin.search_groups(q, 5)):
        assert _bits_equal(a, b)
    assert _bits_equal(proj.similarity_map(q, image_id), twin.similarity_map(q, image_id))


@pytest.mark.parametrize("out_dtype", (F16, F32), ids=("to_f16", "to_f32"))
@pytest.mark.parametrize("normalize", (True, False), ids=("unit", "raw"))
@pytest.mark.parametrize("state", ("plain", "removed"))
def test_projected_bank_equals_the_bank_built_from_the_projected_rows(state, normalize, out_dtype, device) -> None:
    from imagescry_amd import PCA, EmbeddingBank

    n, d, k = 700, 72, 16
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(n, d, generator=g) * torch.linspace(2.0, 0.2, d) + 1.5).to(DEV)
    ids = torch.arange(n) // 10
    origin = torch.stack([ids, (torch.arange(n) % 10) // 5, torch.arange(n) % 5], dim=1)
    kw = {} if state == "plain" else {"capacity": n + 300}
    eb = EmbeddingBank(x, dtype=F16, normalize=True, row_groups=ids.to(DEV), **kw)
    eb.row_origin = origin.clone()
    gone = torch.arange(3, n, 7, device=DEV)
    if state == "removed":
        eb.remove(rows=gone)
    pca = PCA(min_num_components=k, max_num_components=k).fit_bank(eb)
    assert pca.num_components == k

    # ONE call with both outputs: `project` with the row-major output switched on as well
    out_rows = torch.full((eb.capacity, k), SENTINEL, dtype=F32, device=DEV)
    launch = eb._project_rows
    calls = []

    def both(mean, w, mask, rows, bank):
        calls.append(rows)
        launch(mean, w, mask, out_rows, bank)

    eb._project_rows = both
    proj = eb.project(pca, dtype=out_dtype, normalize=normalize)
    del eb._project_rows
    assert calls == [None]
    assert proj.dim == k and proj.dtype == out_dtype and proj.normalize is normalize
    assert _bits_equal(out_rows[:n], eb.projected_rows(pca))  # the same p_r from either call
    if state == "removed":
        assert not out_rows[gone].any() and not out_rows[n:].any()

    twin = EmbeddingBank(out_rows[:n].clone(), dtype=out_dtype, normalize=normalize, row_groups=ids.to(DEV), **kw)
    twin.row_origin = origin.clone()
    if state == "removed":
        twin.remove(rows=gone)
    q = torch.randn(7, k, generator=g).to(DEV)
    _same_answers(proj, twin, q, 3)

    # the new bank lives on: append (within the capacity, or by growing) and remove behave as on the twin
    more = torch.randn(9, k, generator=g).to(DEV)
    more_ids = torch.tensor([3, 3, 3, 70, 70, 71, 71, 71, 71], device=DEV)
    more_origin = torch.stack([more_ids.cpu(), torch.full((9,), 2), torch.arange(9) % 5], dim=1)
    for bank in (proj, twin):
        assert list(bank.append(more, row_groups=more_ids, row_origin=more_origin)) == list(range(n, n + 9))
        assert bank.remove(image_ids=[5]) == (10 if state == "plain" else 8)
    _same_answers(proj, twin, q, 3)
    assert len(eb) == n and eb.dim == d  # the source is untouched


# ------------------------------------------------------------------------------------------------ 5. fit_bank
@pytest.mark.parametrize("state", ("plain", "removed"))
@pytest.mark.parametrize("shape", ((258, 72, F16), (258, 200, F32)), ids=_shape_id)
def test_fit_bank_equals_fit_on_exact_integers(shape, state, device) -> None:
    from imagescry_amd import PCA

    n, d, dtype = shape
    eb, live = _int_bank(n, d, dtype, state)
    kw = {"min_num_components": 2, "min_explained_variance": 0.9}
    a = PCA(**kw).fit_bank(eb)
    b = PCA(**kw).fit(eb.bank[eb.live].float())
    assert a.num_components == b.num_components and a.num_features == b.num_features == d
    assert _bits_equal(a.feature_means, b.feature_means)
    assert _bits_equal(a.explained_variance, b.explained_variance)
    assert _bits_equal(a.component_vectors, b.component_vectors)
    assert a.device == b.device == eb.device


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("shape", ((1000, 72, F16), (1000, 200, F32)), ids=_shape_id)
def test_fit_bank_eigenvalues_obey_weyl(shape, state, device) -> None:
    """|lambda_i(G + E) - lambda_i(G)| <= ||E||_2 <= ||E||_F <= ||B||_F for the element-wise bound B of the Gram matrix."""
    from imagescry_amd import PCA

    n, d, dtype = shape
    eb, stored, live = _real_bank(n, d, dtype, state)
    pca = PCA()
    seen = []
    finish = pca._finish_fit
    pca._finish_fit = lambda g, *rest: (seen.append(g.clone()), finish(g, *rest))[1]
    pca.fit_bank(eb)
    rows = stored[live]
    assert torch.allclose(pca.feature_means.cpu().reshape(-1), rows.double().mean(dim=0).float(), rtol=0, atol=1e-6)
    at = (rows - pca.feature_means.cpu().reshape(-1)).T.contiguous()
    want = torch.linalg.eigvalsh(mb.product_f64(at, at))
    got = torch.linalg.eigvalsh((seen[0] + seen[0].T) * 0.5)  # the eigenvalues times (n - 1)
    slack = float(torch.linalg.matrix_norm(mb.product_bound(at, at)))
    assert float((got - want).abs().max()) <= slack
    assert abs(float(pca.explained_variance.sum()) - 1.0) < 1e-5


def test_fit_project_search_end_to_end(device) -> None:
    from imagescry_amd import PCA, EmbeddingBank

    g = torch.Generator().manual_seed(5)
    n, d = 600, 64
    basis = torch.linalg.qr(torch.randn(d, 5, generator=g))[0]
    rows = (torch.randn(n, 5, generator=g) * torch.tensor([6.0, 5.0, 4.0, 3.5, 3.0])) @ basis.T
    rows = rows + 0.01 * torch.randn(n, d, generator=g) + 2.0
    eb = EmbeddingBank(rows.to(DEV), dtype=F16, normalize=False, capacity=1000)
    eb.remove(rows=[1, 2, 3])
    pca = PCA(min_explained_variance=0.99).fit_bank(eb)
    assert pca.num_components == 5
    proj = eb.project(pca)
    assert proj.dim == 5 and proj.dtype == F16 and len(proj) == n and proj.num_removed == 3
    idx = torch.arange(10, 10 + 32 * 17, 17, device=DEV)
    q = pca.transform(eb.rows(idx).float())
    _, found = proj.search(q, 1)
    assert torch.equal(found[:, 0].cpu(), idx.cpu())


# ------------------------------------------------------------------------------------------------ 6. memory
def test_neither_call_unpacks_the_bank(device) -> None:
    from imagescry_amd import PCA, EmbeddingBank

    n, d, k = 200_000, 256, 32
    x = torch.randn(n, d, device=DEV, dtype=F16) + 1.0
    eb = EmbeddingBank(x, dtype=F16, normalize=False)
    del x
    packed = eb._bank.numel()
    assert packed >= n * d * 2
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pca = PCA(min_num_components=k, max_num_components=k).fit_bank(eb)
    torch.cuda.synchronize()
    fit_peak = torch.cuda.max_memory_allocated() - base
    print(f"fit_bank: peak {fit_peak / 2**20:.1f} MiB above the baseline, packed bank {packed / 2**20:.1f} MiB")
    assert fit_peak < packed / 4
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    proj = eb.project(pca)
    torch.cuda.synchronize()
    proj_peak = torch.cuda.max_memory_allocated() - base
    print(f"project: peak {proj_peak / 2**20:.1f} MiB above the baseline, new bank {proj._bank.numel() / 2**20:.1f} MiB")
    assert proj_peak < proj._bank.numel() + packed / 4
    assert proj.dim == k and len(proj) == n
