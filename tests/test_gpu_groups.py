"""Per-query group exclusion (`row_groups=`, `exclude_group=`; isc_cosine_topk_grouped, isc_cosine_topk_exhaustive_grouped,
isc_cosine_range_grouped) on the GPU.  Two checks: the float64 oracle applied per query to the rows it may return, bit for
bit; and GPU against GPU -- a grouped call equals, per query, the masked call that excludes that query's group."""

from __future__ import annotations

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


def _bank(rows: torch.Tensor, device: torch.device, **kw):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=kw.pop("dtype", rows.dtype), normalize=kw.pop("normalize", False), **kw)


def _allow(labels: torch.Tensor, excl: torch.Tensor, mask: np.ndarray | None = None) -> np.ndarray:
    a = labels.cpu().numpy()[None, :] != excl.cpu().numpy()[:, None]
    return a if mask is None else a & mask[None, :]


def _oracle(stored: torch.Tensor, queries: torch.Tensor, k: int, allow: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Top-k of each query over the rows allow[q] lets it return (queries rounded to the bank dtype), padded (-inf, -1)."""
    nq = queries.shape[0]
    s = search_oracle.exact_scores(stored, queries.cpu().to(stored.dtype))
    sc = np.full((nq, k), -np.inf, np.float32)
    ix = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        idx = np.nonzero(allow[q])[0]
        m = min(k, idx.size)
        o = np.lexsort((idx, -s[q, idx].astype(np.float64)))[:m]
        sc[q, :m], ix[q, :m] = s[q, idx[o]], idx[o]
    return sc, ix


def _range_oracle(stored: torch.Tensor, queries: torch.Tensor, thr, allow: np.ndarray):
    s = search_oracle.exact_scores(stored, queries.cpu().to(stored.dtype))
    t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (s.shape[0],))
    offs, sc, ix = [0], [], []
    for qi in range(s.shape[0]):
        sel = np.nonzero((s[qi] >= t[qi]) & allow[qi])[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))
        sc.append(s[qi, sel[order]])
        ix.append(sel[order].astype(np.int64))
        offs.append(offs[-1] + sel.size)
    return np.array(offs, np.int64), np.concatenate(sc).astype(np.float32), np.concatenate(ix)


def _same(got, exp) -> None:
    np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1])
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0])


def _same_range(res, exp) -> None:
    np.testing.assert_array_equal(res.offsets.cpu().numpy(), exp[0])
    np.testing.assert_array_equal(res.indices.cpu().numpy(), exp[2])
    np.testing.assert_array_equal(res.scores.cpu().numpy(), exp[1])


def _per_label(eb, labels: torch.Tensor, q: torch.Tensor, excl: torch.Tensor, k: int, mask: np.ndarray | None = None):
    """One masked call per distinct query label (that label's rows excluded), scattered back into query order."""
    s = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    i = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    for lab in torch.unique(excl).tolist():
        sel = (excl == lab).nonzero().flatten().to(q.device)
        allow = (labels != lab).numpy()
        if mask is not None:
            allow = allow & mask
        ms, mi = eb.search(q[sel], k, mask=torch.from_numpy(allow))
        s[sel], i[sel] = ms, mi
    return s, i


def _grouped_case(n: int, d: int, nq: int, dtype: torch.dtype, group: int, seed: int):
    """Bank of n rows in groups of `group` adjacent rows, labels 10 * g + 3; queries near banked rows, each excluding
    the group of its row."""
    bank, noise = cases.search_case(n, d, nq, torch.float32, seed=seed)
    labels = torch.arange(n, dtype=torch.int64) // group * 10 + 3
    src = torch.from_numpy(np.random.default_rng(seed).integers(0, n, nq))
    queries = bank[src] + 0.3 * torch.nn.functional.normalize(noise, dim=1)
    return bank.to(dtype), queries, labels, labels[src].clone()


# ---------------------------------------------------------------------------------------------------- every tiling
@pytest.mark.parametrize("nq", [1, 64, 65, 128, 129, 300, 2500])
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_grouped_topk_matches_oracle(nq: int, k: int, dtype: torch.dtype, device: torch.device) -> None:
    """Every query tiling (one tile of 64 / 128, tiles of 256, three passes of 1024 at Q = 2500), both bank dtypes,
    float32 queries at k = 10, float16 at k = 100."""
    bank, q, labels, excl = _grouped_case(3000, 64, nq, dtype, 49, seed=nq + k)
    excl[::7] = -99  # some queries carry a label no row has
    qd = q.to({1: dtype, 10: torch.float32, 100: torch.float16}[k])  # fp32 queries on both banks, fp16 on both
    eb = _bank(bank, device, row_groups=labels)
    stored = eb.bank.cpu()
    s, i = eb.search(qd.to(device), k, exclude_group=excl)
    _same((s, i), _oracle(stored, qd, k, _allow(labels, excl)))
    if k == 10 and nq <= 300:
        ps, pi = _per_label(eb, labels, qd.to(device), excl, k)
        assert torch.equal(i, pi) and torch.equal(s, ps)
    assert int(eb.last_status[1]) == 0


def test_database_ordered_near_duplicate_cells(device: torch.device) -> None:
    """Rows in the store's (record, h, w) order: the 49 cells of an image are adjacent and nearly identical, and a query
    -- a cell of a banked image -- would find its own image's 49 cells first.  None may be returned."""
    g = cases.gen(31)
    images, cells, d = 3000, 49, 96
    centres = torch.nn.functional.normalize(torch.randn(images, d, generator=g), dim=1)
    rows = (centres[:, None, :] + 0.05 * torch.randn(images, cells, d, generator=g)).reshape(images * cells, d)
    image_of = torch.arange(images * cells, dtype=torch.int64) // cells + 100
    eb = _bank(rows, device, dtype=torch.float16, normalize=True, row_groups=image_of)
    stored = eb.bank.cpu()
    src = torch.randint(0, images * cells, (96,), generator=g)
    queries = stored[src].float() + 0.01 * torch.randn((96, d), generator=g)
    excl = image_of[src]
    s, i = eb.search(queries.to(device), 10, exclude_group=excl.to(device))
    assert not (image_of[i.cpu()] == excl[:, None]).any()
    _same((s, i), _oracle(stored, queries, 10, _allow(image_of, excl)))
    st = eb.last_status.cpu().tolist()
    print(f"near-duplicate cells, grouped: last_status = {st}")
    assert st[0] == 0 and st[1] <= 2, st


def test_large_group_pads_and_absent_labels_change_nothing(device: torch.device) -> None:
    n, k = 2000, 20
    bank, q, _, _ = _grouped_case(n, 48, 70, torch.float16, 49, seed=4)
    labels = torch.zeros(n, dtype=torch.int64)
    labels[:12] = 1  # query 0..34 exclude group 0: 12 rows remain, fewer than k
    excl = torch.zeros(70, dtype=torch.int64)
    excl[35:] = 5  # no row carries label 5
    eb = _bank(bank, device, row_groups=labels)
    s, i = eb.search(q.to(device), k, exclude_group=excl.to(device))
    _same((s, i), _oracle(eb.bank.cpu(), q, k, _allow(labels, excl)))
    assert (i[:35, 12:] == -1).all() and torch.isneginf(s[:35, 12:]).all()
    us, ui = eb.search(q[35:].to(device), k)
    assert torch.equal(i[35:], ui) and torch.equal(s[35:], us)


def test_grouped_with_mask(device: torch.device) -> None:
    bank, q, labels, excl = _grouped_case(5000, 64, 100, torch.float16, 49, seed=8)
    allow = np.random.default_rng(3).random(5000) < 0.3
    eb = _bank(bank, device, row_groups=labels)
    rf = eb.row_filter(torch.from_numpy(allow))
    s, i = eb.search(q.to(device), 10, mask=rf, exclude_group=excl)
    _same((s, i), _oracle(eb.bank.cpu(), q, 10, _allow(labels, excl, allow)))
    ps, pi = _per_label(eb, labels, q.to(device), excl, 10, allow)
    assert torch.equal(i, pi) and torch.equal(s, ps)


@pytest.mark.parametrize("nq", [11, 300])
def test_ties_take_the_redo_and_the_exhaustive_pass(nq: int, device: torch.device) -> None:
    """24 distinct rows stored 40 times each, the copies spread over groups: the redo filter and k_exact apply the
    per-query exclusion."""
    bank, queries = cases.tie_case(torch.float16)
    queries = queries.repeat((nq + queries.shape[0] - 1) // queries.shape[0], 1)[:nq]
    labels = torch.arange(bank.shape[0], dtype=torch.int64) % 7
    excl = torch.arange(nq, dtype=torch.int64) % 9
    eb = _bank(bank, device, row_groups=labels)
    for k in (5, 30, 100):
        s, i = eb.search(queries.to(device), k, exclude_group=excl)
        _same((s, i), _oracle(eb.bank.cpu(), queries, k, _allow(labels, excl)))
        ps, pi = _per_label(eb, labels, queries.to(device), excl, k)
        assert torch.equal(i, pi) and torch.equal(s, ps)
    print(f"ties, grouped: last_status = {eb.last_status.cpu().tolist()}")


def test_nan_rows_zero_and_nonfinite_queries(device: torch.device) -> None:
    bank, q, labels, excl = _grouped_case(1500, 64, 70, torch.float32, 49, seed=12)
    bank[[3, 700, 701]] = float("nan")
    q[0] = 0
    q[1, 5] = float("inf")
    q[2, 9] = float("nan")
    q[3] = 0
    excl[0] = labels[0]
    eb = _bank(bank, device, row_groups=labels)
    for k in (1, 10, 60):
        s, i = eb.search(q.to(device), k, exclude_group=excl)
        _same((s, i), _oracle(eb.bank.cpu(), q, k, _allow(labels, excl)))
        _same(eb.search_exhaustive(q.to(device), k, exclude_group=excl), _oracle(eb.bank.cpu(), q, k, _allow(labels, excl)))


# ---------------------------------------------------------------------------------------------------- other searches
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_grouped_exhaustive_and_range(dtype: torch.dtype, device: torch.device) -> None:
    bank, q, labels, excl = _grouped_case(4000, 64, 150, dtype, 49, seed=21)
    q[4] = 0
    eb = _bank(bank, device, row_groups=labels)
    stored = eb.bank.cpu()
    allow = _allow(labels, excl)
    _same(eb.search_exhaustive(q.to(device), 10, exclude_group=excl), _oracle(stored, q, 10, allow))
    for thr in (0.6, 0.2):
        _same_range(eb.search_range(q.to(device), thr, exclude_group=excl), _range_oracle(stored, q, thr, allow))
    # a zero query with t <= 0 scans: every row it may return, in row order
    thr = torch.full((150,), 0.5, dtype=torch.float32)
    thr[4] = -0.5
    _same_range(eb.search_range(q.to(device), thr, exclude_group=excl), _range_oracle(stored, q, thr.numpy(), allow))
    # a capacity retry: the first guess holds a fraction of the answer
    eb._RANGE_GUESS_PER_QUERY = 1
    res = eb.search_range(q.to(device), 0.0, exclude_group=excl)
    _same_range(res, _range_oracle(stored, q, 0.0, allow))
    assert int(res.offsets[-1]) > (1 << 16)


def test_two_async_searches_in_flight(device: torch.device) -> None:
    bank, q, labels, excl = _grouped_case(6000, 64, 40, torch.float16, 49, seed=30)
    eb = _bank(bank, device, row_groups=labels)
    excl2 = excl.flip(0)
    h1 = eb.search_async(q.to(device), 10, exclude_group=excl.to(device))
    h2 = eb.search_async(q.to(device), 10, exclude_group=excl2.to(device))
    stored = eb.bank.cpu()
    _same(h2.result(), _oracle(stored, q, 10, _allow(labels, excl2)))
    _same(h1.result(), _oracle(stored, q, 10, _allow(labels, excl)))


def test_presharded_grouped_merge(device: torch.device) -> None:
    """Eight presharded banks with their own label dictionaries, searched with the same [Q] labels and merged with the
    product's merge: the unsharded grouped search.  Groups span shards; shard 3 holds one big group only."""
    from imagescry_amd.search import _unpad

    n, d, g = 4000, 64, 8
    bank, q, labels, excl = _grouped_case(n, d, 30, torch.float32, 170, seed=2)
    bounds = [(r * n // g, (r + 1) * n // g) for r in range(g)]
    labels[bounds[3][0] : bounds[3][1]] = 77
    excl[:5] = 77
    full = _bank(bank, device, row_groups=labels)
    want = _oracle(full.bank.cpu(), q, 10, _allow(labels, excl))
    for k in (1, 10, 64):
        want = _oracle(full.bank.cpu(), q, k, _allow(labels, excl))
        parts_s, parts_i = [], []
        for lo, hi in bounds:
            shard = _bank(bank[lo:hi], device, index_base=lo, presharded=True, row_groups=labels[lo:hi])
            s, i = shard._local_topk(q.to(device), k, groups=shard._query_codes(excl, q.shape[0]))
            parts_s.append(s)
            parts_i.append(i)
        _same(_unpad(*full._merge_topk(torch.stack(parts_s), torch.stack(parts_i), k)), want)
        _same(full.search(q.to(device), k, exclude_group=excl), want)


def test_database_bank_is_grouped_by_image(tmp_path: Path, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank, storage

    g = cases.gen(22)
    maps = [(100 + i, torch.randn(32, 7, 7, generator=g)) for i in range(40)]
    storage.write_embeddings(tmp_path, maps, checkpoint_id=1)
    eb = EmbeddingBank.from_database(tmp_path, device=device)
    origin = eb.row_origin
    stored = eb.bank.cpu()
    rows = torch.tensor([3, 7 * 49 + 24, 39 * 49 + 48, 100, 1500])
    q = stored[rows].float()
    excl = origin[rows, 0]
    s, i = eb.search(q.to(device), 20, exclude_group=excl)
    assert not (origin[i.cpu(), 0] == excl[:, None]).any()
    _same((s, i), _oracle(stored, q, 20, _allow(origin[:, 0], excl)))
    for r, img in zip(rows.tolist(), excl.tolist()):  # = one masked call per image
        ms, mi = eb.search(stored[r : r + 1].float().to(device), 20, mask=eb.row_filter(image_ids=[img], exclude=True))
        assert torch.equal(mi[0], i[rows.tolist().index(r)]) and torch.equal(ms[0], s[rows.tolist().index(r)])


# ---------------------------------------------------------------------------------------------------- scale
def test_ten_million_rows_grouped(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d, nq, k = 10_000_000, 768, 64, 10
    gen = torch.Generator(device=device).manual_seed(23)
    rows = torch.empty((n, d), dtype=torch.float16, device=device)
    for r0 in range(0, n, 1 << 20):
        blk = torch.randn((min(1 << 20, n - r0), d), generator=gen, device=device)
        rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
    src = torch.arange(nq, device=device) * (n // nq) + 7
    q = rows[src].float() + 0.05 * torch.randn((nq, d), generator=gen, device=device)
    labels = torch.arange(n, device=device) // 49
    eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False, row_groups=labels)
    del rows
    excl = labels[src]
    s, i = eb.search(q, k, exclude_group=excl)
    st = eb.last_status.cpu()
    assert int(st[1]) == 0, st  # an iid bank needs no redo
    assert not bool((i // 49 == excl[:, None]).any())
    sample = torch.tensor([0, 1, 17, 40, 63], device=device)
    es, ei = eb.search_exhaustive(q[sample], k, exclude_group=excl[sample])
    assert torch.equal(i[sample], ei) and torch.equal(s[sample], es)
    us, ui = eb.search(q, k)  # the unexcluded answer starts with the query's own cell
    assert bool((ui[:, 0] == src).all()) and not torch.equal(ui, i)


# ---------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_excludes_each_querys_own_image(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank, ImageBatch, ResNet50Embedder, resnet50
    from imagescry_amd.pipelines import EmbedSearchPipeline

    g = torch.Generator().manual_seed(9)
    model = ResNet50Embedder(state_dict=resnet50.make_state_dict(seed=0, randomize_bn=True)).to(device)
    images = torch.randint(0, 256, (12, 3, 96, 80), dtype=torch.uint8, generator=g)
    batches = [ImageBatch(indices=torch.arange(b, b + 4), images=images[b : b + 4]) for b in (0, 4, 8)]
    emb = [model.predict_step(b.to(device)) for b in batches]
    flat = torch.cat([e.get_flat_vectors() for e in emb])
    per_image = flat.shape[0] // 12
    image_ids = torch.arange(12, dtype=torch.int64) * 3 + 500
    labels = image_ids.repeat_interleave(per_image)
    filler = torch.nn.functional.normalize(torch.randn(3000, flat.shape[1], generator=g), dim=1)
    rows = torch.cat([filler.to(device), flat])
    row_groups = torch.cat([torch.full((3000,), -1, dtype=torch.int64), labels])
    bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False, row_groups=row_groups)
    for overlap in (True, False):
        pipe = EmbedSearchPipeline(embedding_model=model, bank=bank, k=10, overlap=overlap, image_groups=image_ids)
        results = pipe.run(batches)
        for b, res in zip(batches, results):
            qlab = image_ids[b.indices].repeat_interleave(per_image)
            q = model.predict_step(b.to(device)).get_flat_vectors()
            s, i = bank.search(q, 10, exclude_group=qlab)
            assert torch.equal(res.neighbours, i) and torch.equal(res.scores, s)
            assert not (row_groups[res.neighbours.cpu()] == qlab[:, None]).any()
