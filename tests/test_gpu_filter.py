"""Row-filtered search (`mask=`, `EmbeddingBank.row_filter`; isc_cosine_topk_masked, isc_cosine_topk_exhaustive_masked,
isc_cosine_range_masked) on the GPU.  The oracle of a masked search is the float64 oracle on the bank of the allowed rows,
indices mapped back; results must match bit for bit, the padding of short answers included."""

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


def _oracle(stored: torch.Tensor, queries: torch.Tensor, k: int, allow: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Top-k of the allowed rows alone (queries rounded to the bank dtype), padded with (-inf, -1)."""
    idx = np.nonzero(allow)[0]
    nq = queries.shape[0]
    sc = np.full((nq, k), -np.inf, np.float32)
    ix = np.full((nq, k), -1, np.int64)
    m = min(k, idx.size)
    if m:  # (score desc with NaN last, row asc) over the allowed rows
        s = search_oracle.exact_scores(stored[torch.from_numpy(idx)], queries.to(stored.dtype))
        for q in range(s.shape[0]):
            o = np.lexsort((idx, -s[q].astype(np.float64)))[:m]
            sc[q, :m], ix[q, :m] = s[q, o], idx[o]
    return sc, ix


def _range_oracle(stored: torch.Tensor, queries: torch.Tensor, thr, allow: np.ndarray):
    q = queries.to(stored.dtype)
    s = search_oracle.exact_scores(stored, q)
    t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (s.shape[0],))
    offs, sc, ix = [0], [], []
    for qi in range(s.shape[0]):
        sel = np.nonzero((s[qi] >= t[qi]) & allow)[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))
        sc.append(s[qi, sel[order]])
        ix.append(sel[order].astype(np.int64))
        offs.append(offs[-1] + sel.size)
    return np.array(offs, np.int64), np.concatenate(sc).astype(np.float32), np.concatenate(ix)


def _same(got, exp) -> None:
    np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1])
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0])  # NaN == NaN and -inf == -inf here; -0.0 == 0.0


def _same_range(res, exp) -> None:
    np.testing.assert_array_equal(res.offsets.cpu().numpy(), exp[0])
    np.testing.assert_array_equal(res.indices.cpu().numpy(), exp[2])
    np.testing.assert_array_equal(res.scores.cpu().numpy(), exp[1])


def _densities(n: int, seed: int) -> dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    out = {f"p{p}": rng.random(n) < p for p in (1.0, 0.5, 0.1, 0.01)}
    one = np.zeros(n, bool)
    one[n // 3] = True
    out["single"] = one
    out["empty"] = np.zeros(n, bool)
    return out


# ---------------------------------------------------------------------------------------------------- shapes x densities
@pytest.mark.parametrize("dtype,d", [(torch.float16, 64), (torch.float32, 96)])
@pytest.mark.parametrize("nq", [1, 7, 64, 100, 128, 300, 1024, 1500])
def test_masked_topk_matches_oracle(dtype: torch.dtype, d: int, nq: int, device: torch.device) -> None:
    """Every tile shape (64 / 128 / 256 queries), a two-pass call (1500), k up to the ABI's limit, six densities."""
    n = 5003
    rows, q = cases.search_case(n, d, nq, dtype, seed=nq)
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    qd = q.to(device)
    for name, allow in _densities(n, nq).items():
        rf = eb.row_filter(torch.from_numpy(allow))
        assert int(rf.allowed_count.item()) == int(allow.sum())
        for k in (1, 10, 64, 120):
            got = eb.search(qd, k, mask=rf)
            _same(got, _oracle(stored, q, k, allow))
            if name == "p1.0":  # an all-allowed filter is the unmasked search, bit for bit
                base = eb.search(qd, k)
                assert torch.equal(got[1], base[1]) and torch.equal(got[0].view(torch.int32), base[0].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- structured masks
def test_structured_masks(device: torch.device) -> None:
    n, d, nq = 20_000, 128, 64
    rows, q = cases.search_case(n, d, nq, torch.float16, seed=5)
    dup = torch.arange(0, n, n // nq)[:nq]  # the queries ARE rows: each query's best row is itself
    q = rows[dup].float()
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    block = np.zeros(n, bool)
    block[4_000:11_000] = True
    no_dup = np.ones(n, bool)
    no_dup[dup.numpy()] = False
    masks = {"block": block, "complement": ~block, "every_other": np.arange(n) % 2 == 0, "no_self": no_dup}
    for name, allow in masks.items():
        for k in (1, 10, 120):
            _same(eb.search(q.to(device), k, mask=torch.from_numpy(allow).to(device)), _oracle(stored, q, k, allow))
    # without its own row every query's best answer is someone else's
    s, i = eb.search(q.to(device), 5, mask=eb.row_filter(rows=dup, exclude=True))
    assert not np.isin(i.cpu().numpy(), dup.numpy()).any()


def test_ties_take_the_redo_and_the_exhaustive_pass(device: torch.device) -> None:
    """20 000 allowed copies of one row tie at the k-th score: the first pass cannot prove the answer (last_status[1]), the
    matrix-core redo cannot hold the copies and k_exact answers (last_status[3]); a zero query takes k_exact too (its
    first k ALLOWED rows)."""
    g = cases.gen(31)
    d = 128
    v = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1)
    rows = torch.cat([v.repeat(40_000, 1), torch.nn.functional.normalize(torch.randn(10_000, d, generator=g), dim=1)])
    rows = rows[torch.randperm(rows.shape[0], generator=g)].half()
    q = torch.cat([v * 2.0, torch.zeros(1, d), torch.randn(3, d, generator=g)])
    allow = np.arange(rows.shape[0]) % 2 == 1
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    rf = eb.row_filter(torch.from_numpy(allow))
    for k in (10, 120):
        got = eb.search(q.to(device), k, mask=rf)
        st = eb.last_status.cpu()
        _same(got, _oracle(stored, q, k, allow))
        assert int(st[1]) >= 1 and int(st[3]) >= 2, st
    zero = eb.search(q[1:2].to(device), 7, mask=rf)[1].cpu().numpy()[0]
    np.testing.assert_array_equal(zero, np.nonzero(allow)[0][:7])


def test_nan_rows_and_padding(device: torch.device) -> None:
    n, d = 3000, 64
    rows, q = cases.search_case(n, d, 9, torch.float32, seed=8)
    rows[17] = float("nan")
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    few = np.zeros(n, bool)
    few[[3, 17, 900, 2001, 2999]] = True  # the NaN row allowed: 4 real rows, the NaN row, then padding
    s, i = eb.search(q.to(device), 10, mask=eb.row_filter(torch.from_numpy(few)))
    _same((s, i), _oracle(stored, q, 10, few))
    assert (i[:, 4].cpu() == 17).all() and torch.isnan(s[:, 4]).all()
    assert (i[:, 5:] == -1).all() and (s[:, 5:] == -np.inf).all()
    for allow in (np.arange(n) != 17, np.arange(n) % 3 == 2):  # the NaN row masked out / left in
        for k in (1, 10, 64):
            _same(eb.search(q.to(device), k, mask=torch.from_numpy(allow)), _oracle(stored, q, k, allow))
    ex = eb.search_exhaustive(q.to(device), 10, mask=torch.from_numpy(few))
    _same(ex, _oracle(stored, q, 10, few))


# ---------------------------------------------------------------------------------------------------- equivalences
def test_filter_forms_reuse_and_async(device: torch.device) -> None:
    n, d = 40_000, 256
    rows, q = cases.search_case(n, d, 64, torch.float16, seed=12)
    eb = _bank(rows, device)
    allow = torch.from_numpy(np.random.default_rng(3).random(n) < 0.3)
    rf = eb.row_filter(allow)
    a = eb.search(q.to(device), 10, mask=rf)
    b = eb.search(q.to(device), 10, mask=allow.to(device))
    c = eb.search(q.to(device), 10, mask=rf)
    ids = eb.row_filter(rows=torch.nonzero(allow)[:, 0])
    e = eb.search(q.to(device), 10, mask=ids)
    for other in (b, c, e):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    rf2 = eb.row_filter(allow, exclude=True)
    h1 = eb.search_async(q[:32].to(device), 10, mask=rf)
    h2 = eb.search_async(q[32:].to(device), 10, mask=rf2)
    for got, qq, m in ((h1.result(), q[:32], rf), (h2.result(), q[32:], rf2)):
        ref = eb.search(qq.to(device), 10, mask=m)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    other = _bank(rows[:1000], device)
    with pytest.raises(ValueError):
        other.search(q[:2].to(device), 5, mask=rf)
    with pytest.raises(ValueError):
        eb.row_filter(allow[:-1])
    with pytest.raises(ValueError):
        eb.row_filter(allow, rows=[1])


# ---------------------------------------------------------------------------------------------------- range
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_masked_range(dtype: torch.dtype, device: torch.device) -> None:
    n, d = 30_011, 96
    rows, q = cases.search_case(n, d, 70, dtype, seed=41)
    q[2] = 0  # zero query: every score is 0
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    for name, allow in _densities(n, 7).items():
        rf = eb.row_filter(torch.from_numpy(allow))
        for t in (0.2, 0.0):
            res = eb.search_range(q.to(device), t, mask=rf)
            _same_range(res, _range_oracle(stored, q, t, allow))
        if name == "p1.0":
            a, b = eb.search_range(q.to(device), 0.2, mask=rf), eb.search_range(q.to(device), 0.2)
            assert torch.equal(a.offsets, b.offsets) and torch.equal(a.indices, b.indices)
    # more rows than the first call reserves: one retry of the exact size
    allow = np.random.default_rng(1).random(n) < 0.9
    big = eb.search_range(q[:4].to(device), -2.0, mask=torch.from_numpy(allow))
    assert int(big.offsets[-1]) == 4 * int(allow.sum()) > 1 << 16
    _same_range(big, _range_oracle(stored, q[:4], -2.0, allow))


# ---------------------------------------------------------------------------------------------------- shards
def test_presharded_masked_merge(device: torch.device) -> None:
    """Eight presharded banks, each searched with its slice of one global filter, merged with the product's merge: the
    unsharded masked search.  Shard 3 allows no row; shard 5 holds NaN rows next to the padding of the others."""
    from imagescry_amd.search import _unpad

    n, d, g = 4_000, 64, 8
    rows, q = cases.search_case(n, d, 12, torch.float32, seed=2)
    allow = np.random.default_rng(5).random(n) < 0.01
    bounds = [(r * n // g, (r + 1) * n // g) for r in range(g)]
    allow[bounds[3][0] : bounds[3][1]] = False
    lo5 = bounds[5][0]
    rows[lo5 + 1] = float("nan")
    rows[lo5 + 2] = float("nan")
    allow[[lo5 + 1, lo5 + 2]] = True
    full = _bank(rows, device)
    for k in (1, 10, 64):
        parts_s, parts_i = [], []
        for lo, hi in bounds:
            shard = _bank(rows[lo:hi], device, index_base=lo, presharded=True)
            s, i = shard._local_topk(q.to(device), k, mask=shard.row_filter(torch.from_numpy(allow)))
            parts_s.append(s)
            parts_i.append(i)
        ms, mi = _unpad(*full._merge_topk(torch.stack(parts_s), torch.stack(parts_i), k))
        want = _oracle(full.bank.cpu(), q, k, allow)
        _same((ms, mi), want)
        _same(full.search(q.to(device), k, mask=torch.from_numpy(allow)), want)


# ---------------------------------------------------------------------------------------------------- database bank
def test_database_bank_excluding_one_image(tmp_path: Path, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank, storage

    g = cases.gen(22)
    maps = [(100 + i, torch.randn(32, 7, 7, generator=g)) for i in range(40)]
    storage.write_embeddings(tmp_path, maps, checkpoint_id=1)
    eb = EmbeddingBank.from_database(tmp_path, device=device)
    origin = eb.row_origin
    stored = eb.bank.cpu()
    for r in (3, 7 * 49 + 24, 39 * 49 + 48):
        img = int(origin[r, 0])
        q = stored[r : r + 1].float()
        rf = eb.row_filter(image_ids=[img], exclude=True)
        s, i = eb.search(q.to(device), 20, mask=rf)
        assert not (origin[i.cpu()[0], 0] == img).any()
        _same((s, i), _oracle(stored, q, 20, (origin[:, 0] != img).numpy()))


# ---------------------------------------------------------------------------------------------------- scale
def test_ten_million_rows_masked(device: torch.device) -> None:
    n, d, nq, k = 10_000_000, 768, 64, 10
    gen = torch.Generator(device=device).manual_seed(23)
    rows = torch.empty((n, d), dtype=torch.float16, device=device)
    for r0 in range(0, n, 1 << 20):
        blk = torch.randn((min(1 << 20, n - r0), d), generator=gen, device=device)
        rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
    src = torch.arange(nq, device=device) * (n // nq) + 7
    q = rows[src].float() + 0.05 * torch.randn((nq, d), generator=gen, device=device)
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
    del rows
    half = torch.rand(n, generator=gen, device=device) < 0.5
    image = torch.ones(n, dtype=torch.bool, device=device)  # "images" of 64 adjacent cells: drop query 0's image
    image[(int(src[0]) // 64) * 64 : (int(src[0]) // 64 + 1) * 64] = False
    sample = torch.tensor([0, 1, 17, 40, 63], device=device)
    for allow in (half, image):
        rf = eb.row_filter(allow)
        s, i = eb.search(q, k, mask=rf)
        st = eb.last_status.cpu()
        assert int(st[1]) == 0, st  # an iid bank with half its rows allowed needs no redo
        es, ei = eb.search_exhaustive(q[sample], k, mask=rf)
        assert torch.equal(i[sample], ei) and torch.equal(s[sample], es)
        assert bool(allow[i.reshape(-1)].all())
