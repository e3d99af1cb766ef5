"""`EmbeddingBank.search_range` (isc_cosine_range) on the GPU against the float64 oracle: membership, scores and order bit
for bit, consistency with top-k, the rounding guard, edge cases, capacity, scale, sharding and a database bank."""

from __future__ import annotations

import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import cases  # noqa: E402

from oracle import search_oracle  # noqa: E402

pytestmark = pytest.mark.gpu


def _bank(rows: torch.Tensor, device: torch.device, **kw):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=kw.pop("dtype", rows.dtype), normalize=kw.pop("normalize", False), **kw)


def _oracle(stored: torch.Tensor, queries: torch.Tensor, thr) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Range answer of the oracle: queries rounded to the bank dtype, rows with score >= t, lexsorted."""
    q = queries.to(stored.dtype)
    s = search_oracle.exact_scores(stored, q)
    t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (s.shape[0],))
    offs, sc, ix = [0], [], []
    for qi in range(s.shape[0]):
        sel = np.nonzero(s[qi] >= t[qi])[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))
        sc.append(s[qi, sel[order]])
        ix.append(sel[order].astype(np.int64))
        offs.append(offs[-1] + sel.size)
    return np.array(offs, np.int64), np.concatenate(sc).astype(np.float32), np.concatenate(ix)


def _same(res, exp) -> None:
    offs, sc, ix = exp
    np.testing.assert_array_equal(res.offsets.cpu().numpy(), offs)
    np.testing.assert_array_equal(res.indices.cpu().numpy(), ix)
    got = res.scores.cpu().numpy()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, sc)  # bit for bit (up to the sign of zero, which the key order does not keep)


def _unit(n: int, d: int, seed: int) -> torch.Tensor:
    g = cases.gen(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)


def _quantile_thresholds(stored: torch.Tensor, q: torch.Tensor, per_query: int) -> np.ndarray:
    """Per-query thresholds that admit about `per_query` rows."""
    s = search_oracle.exact_scores(stored, q.to(stored.dtype))
    kk = min(per_query, s.shape[1])
    return np.sort(s, axis=1)[:, s.shape[1] - kk].astype(np.float32)


# ---------------------------------------------------------------------------------------------------- oracle parity
PARITY = [
    # (n, d, q)
    (1, 64, 7),
    (255, 768, 7),
    (256, 64, 64),
    (257, 1000, 1),
    (2000, 64, 1500),
    (3000, 768, 1024),
    (100_003, 768, 7),
    (100_003, 64, 64),
]


@pytest.mark.parametrize("bank_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("q_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("n,d,nq", PARITY)
def test_range_matches_oracle(n: int, d: int, nq: int, bank_dtype, q_dtype, device: torch.device) -> None:
    rows = _unit(n, d, 3).to(bank_dtype)
    q = _unit(nq, d, 4)
    q[0] = rows[n // 2].float() + 0.01 * q[0]  # a query next to a row
    q = q.to(q_dtype)
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    for thr in (0.999, 0.3, 0.05):  # ~0, a few, thousands (at the larger n) per query
        _same(eb.search_range(q.to(device), thr), _oracle(stored, q, thr))
    # per-query thresholds: a few rows each, one query admitting everything
    t = _quantile_thresholds(stored, q, 5)
    t[-1] = -2.0
    _same(eb.search_range(q.to(device), torch.from_numpy(t).to(device)), _oracle(stored, q, t))


# ---------------------------------------------------------------------------------------------------- top-k consistency
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_first_k_rows_equal_topk(k: int, dtype, device: torch.device) -> None:
    rows = _unit(20_000, 768, 5)
    q = _unit(16, 768, 6)
    rows[100:140] = rows[7]  # exact ties at the top for query 0 ...
    q[0] = rows[7] + 0.05 * q[0]
    rows[1000 : 1000 + 3 * k] = rows[11]  # ... and ties straddling the k-th score for query 1
    q[1] = rows[11] + 0.2 * q[1]
    rows = rows.to(dtype)
    eb = _bank(rows, device)
    qd = q.to(device)
    s, i = eb.search(qd, k)
    t = s[:, k - 1].contiguous()
    res = eb.search_range(qd, t)
    assert bool((res.counts >= k).all())
    for qi in range(q.shape[0]):
        rs, ri = res[qi]
        assert torch.equal(ri[:k], i[qi]) and torch.equal(rs[:k].view(torch.int32), s[qi].view(torch.int32))
    _same(res, _oracle(eb.bank.cpu(), q, t.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------- rounding guard
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_rows_one_ulp_either_side_of_the_threshold(dtype, device: torch.device) -> None:
    g = cases.gen(41)
    d, n = 768, 20000
    rows = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    q = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1)
    base = torch.nn.functional.normalize(q + 0.3 * torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1), dim=1)
    base = base.to(dtype)
    for j, r in enumerate(torch.randperm(n, generator=g)[:30].tolist()):
        row = base[0].clone()
        comp = torch.randint(0, d, (3,), generator=g)
        bits = row[comp].view(torch.int16 if dtype == torch.float16 else torch.int32)
        row[comp] = (bits + (1 if j % 2 else -1)).view(dtype)
        rows[r] = row.float()
    rows = rows.to(dtype)
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    s = search_oracle.exact_scores(stored, q.to(dtype))[0]
    near = np.unique(np.sort(s)[-30:])  # the cluster's distinct scores: thresholds exactly at each of them
    for t in list(near) + [np.nextafter(near[len(near) // 2], np.float32(2))]:
        _same(eb.search_range(q.to(device), float(t)), _oracle(stored, q, float(t)))
        ratio = eb.last_range_status.cpu()[2:3].view(torch.float32).item()
        assert ratio < 1.0


@pytest.mark.parametrize("d", [768, 4096])
def test_same_sign_vectors_keep_the_filter_error_small(d: int, device: torch.device) -> None:
    g = cases.gen(7)
    rows = torch.nn.functional.normalize(torch.rand(5000, d, generator=g), dim=1).half()
    q = torch.rand(8, d, generator=g)
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    t = _quantile_thresholds(stored, q, 50)
    res = eb.search_range(q.to(device), torch.from_numpy(t).to(device))
    _same(res, _oracle(stored, q, t))
    st = eb.last_range_status.cpu()
    ratio = st[2:3].view(torch.float32).item()
    assert 0.0 < ratio < 0.5, ratio
    assert int(st[1]) == 0 and int(st[0]) >= int(res.offsets[-1])


def test_long_segment_of_identical_rows(device: torch.device) -> None:
    rows = _unit(50_000, 256, 8)
    rows[10_000:30_000] = rows[3]  # 20 000 identical rows (plus the original): one long segment, all tied
    q = rows[3:4] + 0.01 * _unit(1, 256, 9)
    rows = rows.half()
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    t = float(search_oracle.exact_scores(stored, q.half())[0, 3]) - 1e-3
    res = eb.search_range(q.to(device), t)
    assert int(res.counts[0]) >= 20_001
    _same(res, _oracle(stored, q, t))


# ---------------------------------------------------------------------------------------------------- edge cases
def test_nan_inf_queries_and_nan_row(device: torch.device) -> None:
    rows = _unit(3000, 64, 10)
    q = _unit(6, 64, 11)
    q[1, 5] = float("nan")
    q[2, 7] = float("inf")
    eb = _bank(rows.half(), device)
    stored = eb.bank.cpu()
    for t in (0.1, -2.0):
        res = eb.search_range(q.to(device), t)
        _same(res, _oracle(stored, q, t))
        assert int(res.counts[1]) == 0 and int(res.counts[2]) == 0
    # a NaN row: the norm bound is not finite, every query takes the float64 scan and stays exact
    rows_nan = rows.clone()
    rows_nan[17, 3] = float("nan")
    eb = _bank(rows_nan.half(), device)
    stored = eb.bank.cpu()
    good = q[[0, 3, 4, 5]]
    for t in (0.1, -2.0):
        res = eb.search_range(good.to(device), t)
        _same(res, _oracle(stored, good, t))
        assert int(eb.last_range_status.cpu()[1]) == good.shape[0]
        assert 17 not in res.indices.cpu().tolist()


def test_zero_query(device: torch.device) -> None:
    rows = _unit(1234, 64, 12).half()
    q = torch.zeros(2, 64)
    q[1] = _unit(1, 64, 13)[0]
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    for t in (0.0, -0.5):
        res = eb.search_range(q.to(device), t)
        assert int(res.counts[0]) == 1234
        assert res[0][1].cpu().tolist() == list(range(1234))
        _same(res, _oracle(stored, q, t))
    res = eb.search_range(q.to(device), 1e-6)
    assert int(res.counts[0]) == 0
    _same(res, _oracle(stored, q, 1e-6))


@pytest.mark.parametrize("scale", [1e-36, 1e-25, 1e30, 1e36])
def test_extreme_query_scales(scale: float, device: torch.device) -> None:
    rows = _unit(4000, 128, 14)
    q = _unit(4, 128, 15) * scale
    eb = _bank(rows, device, dtype=torch.float32)
    stored = eb.bank.cpu()
    t = _quantile_thresholds(stored, q, 20)
    _same(eb.search_range(q.to(device), torch.from_numpy(t).to(device)), _oracle(stored, q, t))


def test_unnormalised_bank(device: torch.device) -> None:
    g = cases.gen(16)
    rows = torch.randn(5000, 96, generator=g) * torch.rand(5000, 1, generator=g) * 5
    q = torch.randn(9, 96, generator=g)
    for dtype in (torch.float16, torch.float32):
        eb = _bank(rows, device, dtype=dtype, normalize=False)
        stored = eb.bank.cpu()
        t = _quantile_thresholds(stored, q, 40)
        _same(eb.search_range(q.to(device), torch.from_numpy(t).to(device)), _oracle(stored, q, t))


# ---------------------------------------------------------------------------------------------------- capacity
def test_capacity_retry_and_max_results(device: torch.device) -> None:
    rows = _unit(40_000, 64, 17).half()
    q = _unit(2, 64, 18)
    eb = _bank(rows, device)
    stored = eb.bank.cpu()
    # ~35 000 rows per query: more than the first guess of 64 Ki entries for two queries
    res = eb.search_range(q.to(device), -0.5)
    exp = _oracle(stored, q, -0.5)
    assert exp[0][-1] > 1 << 16
    _same(res, exp)
    with pytest.raises(ValueError, match=str(int(exp[0][-1]))):
        eb.search_range(q.to(device), -0.5, max_results=int(exp[0][-1]) - 1)
    with pytest.raises(ValueError):
        eb.search_range(q.to(device), float("nan"))
    with pytest.raises(ValueError):
        eb.search_range(q.to(device), torch.tensor([0.1, float("nan")], device=device))


# ---------------------------------------------------------------------------------------------------- scale
def test_ten_million_rows(device: torch.device) -> None:
    n, d, nq = 10_000_000, 768, 16
    g = torch.Generator(device=device).manual_seed(19)
    rows = torch.empty((n, d), dtype=torch.float16, device=device)
    for r0 in range(0, n, 1 << 20):
        blk = torch.randn((min(1 << 20, n - r0), d), generator=g, device=device)
        rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
    q = torch.randn((nq, d), generator=g, device=device)
    q[:4] = rows[[5, 123_456, 5_000_000, n - 1]].float() + 0.02 * q[:4]
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
    t = 0.15
    res = eb.search_range(q, t)
    # float64 scores, blockwise on the device
    qh = q.half().double()
    denom = qh.norm(dim=1).clamp_min(1e-12)
    parts = []
    for r0 in range(0, n, 1 << 20):
        s = ((qh @ rows[r0 : r0 + (1 << 20)].double().T) / denom[:, None]).float()
        qi, ri = torch.nonzero(s >= t, as_tuple=True)
        parts.append((qi, ri + r0, s[qi, ri]))
    qi = torch.cat([p[0] for p in parts])
    ri = torch.cat([p[1] for p in parts])
    sc = torch.cat([p[2] for p in parts])
    order = np.lexsort((ri.cpu().numpy(), -sc.double().cpu().numpy(), qi.cpu().numpy()))
    offs = np.concatenate([[0], np.cumsum(np.bincount(qi.cpu().numpy(), minlength=nq))])
    assert 0 < offs[-1] < 1_000 * nq
    _same(res, (offs, sc.cpu().numpy()[order], ri.cpu().numpy()[order]))
    for j, r in enumerate([5, 123_456, 5_000_000, n - 1]):
        assert int(res[j][1][0]) == r


# ---------------------------------------------------------------------------------------------------- sharding
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from imagescry_amd import EmbeddingBank

        rows = _unit(30_011, 128, 20).half()
        q = _unit(9, 128, 21)
        q[0] = rows[77].float()
        out = {}
        for name, n in (("big", 30_011), ("one", 1)):  # "one": rank 0 holds no row
            eb = EmbeddingBank(rows[:n].to(device), dtype=torch.float16, normalize=False, process_group=dist.group.WORLD)
            for t in (0.2, -2.0):
                res = eb.search_range(q.to(device), t)
                out[f"{name}_{t}_o"] = res.offsets.cpu().numpy()
                out[f"{name}_{t}_s"] = res.scores.cpu().numpy()
                out[f"{name}_{t}_i"] = res.indices.cpu().numpy()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_sharded_bank_equals_unsharded(tmp_path: Path, device: torch.device) -> None:
    mp.spawn(_shard_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    rows = _unit(30_011, 128, 20).half()
    q = _unit(9, 128, 21)
    q[0] = rows[77].float()
    for name, n in (("big", 30_011), ("one", 1)):
        eb = _bank(rows[:n], device)
        for t in (0.2, -2.0):
            res = eb.search_range(q.to(device), t)
            for r in range(2):
                z = np.load(tmp_path / f"rank{r}.npz")
                np.testing.assert_array_equal(z[f"{name}_{t}_o"], res.offsets.cpu().numpy())
                np.testing.assert_array_equal(z[f"{name}_{t}_i"], res.indices.cpu().numpy())
                np.testing.assert_array_equal(z[f"{name}_{t}_s"].view(np.int32), res.scores.cpu().numpy().view(np.int32))


# ---------------------------------------------------------------------------------------------------- database bank
def test_database_bank_excluding_the_query_image(tmp_path: Path, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank, storage

    g = cases.gen(22)
    maps = [(100 + i, torch.randn(32, 7, 7, generator=g)) for i in range(40)]
    storage.write_embeddings(tmp_path, maps, checkpoint_id=1)
    eb = EmbeddingBank.from_database(tmp_path, device=device)
    origin = eb.row_origin
    stored = eb.bank.cpu()
    qrows = torch.tensor([3, 7 * 49 + 24, 39 * 49 + 48])
    q = stored[qrows].float()
    t = 0.3
    res = eb.search_range(q.to(device), t)
    for j, r in enumerate(qrows.tolist()):
        img = int(origin[r, 0])
        s, i = res[j]
        keep = origin[i.cpu(), 0] != img
        others = torch.nonzero(origin[:, 0] != img)[:, 0]
        offs, sc, ix = _oracle(stored[others], q[j : j + 1], t)
        np.testing.assert_array_equal(i.cpu()[keep].numpy(), others[ix].numpy())
        np.testing.assert_array_equal(s.cpu()[keep].numpy(), sc)
