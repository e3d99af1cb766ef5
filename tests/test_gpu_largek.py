"""`EmbeddingBank.search` / `search_exhaustive` for 120 < k <= 4096 (isc_cosine_topk_large, isc_cosine_topk_exhaustive_large)
on the GPU: scores and indices bit for bit against the float64 oracle and against each other, the fast path's status words,
consistency with k = 120 and with the range search, filters, ties and odd values."""

from __future__ import annotations

import struct
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

F16, F32 = torch.float16, torch.float32


def _bank(rows: torch.Tensor, device: torch.device, **kw):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=kw.pop("dtype", rows.dtype), normalize=kw.pop("normalize", False), **kw)


def _rows(n: int, d: int, seed: int, unit: bool = True) -> torch.Tensor:
    x = torch.randn(n, d, generator=cases.gen(seed))
    if unit:
        return torch.nn.functional.normalize(x, dim=1)
    return x * (0.25 + 4.0 * torch.rand(n, 1, generator=cases.gen(seed + 1)))  # norms spread over 1 : 16


def _oracle(stored: torch.Tensor, q: torch.Tensor, k: int, allow: np.ndarray | None = None):
    """The oracle's top-k of the stored rows for queries rounded to the bank dtype; `allow` (bool [Q, N] or [N]): the rows a
    query may return, short answers padded with (-inf, -1) as the public calls pad."""
    qb = q.to(stored.dtype)
    if allow is None:
        return search_oracle.cosine_topk(stored, qb, k)
    s = search_oracle.exact_scores(stored, qb)
    allow = np.broadcast_to(allow, s.shape)
    out_s = np.full((s.shape[0], k), -np.inf, np.float32)
    out_i = np.full((s.shape[0], k), -1, np.int64)
    for qi in range(s.shape[0]):
        sel = np.nonzero(allow[qi])[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))[:k]
        out_s[qi, : order.size] = s[qi, sel[order]]
        out_i[qi, : order.size] = sel[order]
    return out_s, out_i


def _same(got, exp, what: str = "") -> None:
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gs.dtype == np.float32 and gi.dtype == np.int64
    np.testing.assert_array_equal(gi, exp[1], err_msg=what)
    np.testing.assert_array_equal(gs, exp[0], err_msg=what)  # bit for bit (NaN == NaN here; the key order drops the sign of 0)


def _served_by_the_fast_path(eb) -> None:
    st = eb.last_status.cpu().tolist()
    ratio = struct.unpack("f", struct.pack("i", st[2]))[0]
    assert st[0] == 0 and st[1] == 0, st
    assert 0.0 <= ratio < 1.0, ratio


def _check(eb, q: torch.Tensor, k: int, device: torch.device, allow=None, fast: bool = True, **kw) -> None:
    exp = _oracle(eb.bank.cpu(), q, k, allow)
    _same(eb.search(q.to(device), k, **kw), exp, "search")
    if fast:
        _served_by_the_fast_path(eb)
    _same(eb.search_exhaustive(q.to(device), k, **kw), exp, "search_exhaustive")


# ------------------------------------------------------------------------------------------------------- shape sweep
NS = (121, 255, 256, 257, 1000, 5000)
DS = (32, 40, 768)
QS = (1, 63, 65, 1025)
DTYPES = ((F16, F16), (F16, F32), (F32, F16), (F32, F32))  # (bank, queries)
NK = [(n, k) for n in NS for k in sorted({kk for kk in (121, 128, 1000, min(n, 4096)) if kk <= n})]


@pytest.mark.parametrize("i,n,k", [(i, n, k) for i, (n, k) in enumerate(NK)])
def test_every_bank_size_and_k(i: int, n: int, k: int, device: torch.device) -> None:
    """Every N with every k it admits (k = N among them); D, Q, the dtypes and the row norms cycle through their values."""
    d, nq = DS[i % 3], QS[(i + i // 3) % 4]
    bdt, qdt = DTYPES[(i + i // 4) % 4]
    unit = i % 2 == 0
    eb = _bank(_rows(n, d, 10 + i, unit).to(bdt), device)
    _check(eb, _rows(nq, d, 50 + i).to(qdt), k, device)


@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("bdt,qdt", DTYPES)
@pytest.mark.parametrize("nq", QS)
@pytest.mark.parametrize("d", DS)
def test_every_d_q_dtype_and_norm(d: int, nq: int, bdt, qdt, unit: bool, device: torch.device) -> None:
    """The full cross of D, Q, bank dtype, query dtype and unit / raw rows on one bank that crosses a tile boundary."""
    eb = _bank(_rows(257, d, 3, unit).to(bdt), device)
    q = _rows(nq, d, 4)
    q[0] = eb.bank[128].float().cpu() + 0.01 * q[0]  # a query next to a row
    _check(eb, q.to(qdt), 128, device)


def test_passes_shrink_with_k(device: torch.device) -> None:
    """k = 2048 runs passes of 512 queries, k = 4096 of 256: 1025 queries are three passes, 300 two."""
    eb = _bank(_rows(5000, 40, 5).half(), device)
    _check(eb, _rows(1025, 40, 6), 2048, device)
    _check(eb, _rows(300, 40, 7), 4096, device)


def test_buckets_fold(device: torch.device) -> None:
    """200 000 rows are 12 500 blocks of 16 rows folded into 8192 buckets."""
    eb = _bank(_rows(200_000, 64, 8).half(), device)
    _check(eb, _rows(130, 64, 9), 4096, device)


# ------------------------------------------------------------------------------------------------------- consistency
@pytest.mark.parametrize("dtype", [F16, F32])
def test_consistent_with_k_120_and_with_the_range_search(dtype, device: torch.device) -> None:
    eb = _bank(_rows(20_000, 768, 11).to(dtype), device)
    q = _rows(16, 768, 12).to(device)
    k = 500
    s, i = eb.search(q, k)
    _served_by_the_fast_path(eb)
    s120, i120 = eb.search(q, 120)
    assert torch.equal(i[:, :120], i120) and torch.equal(s[:, :120].view(torch.int32), s120.view(torch.int32))
    res = eb.search_range(q, s[:, k - 1].contiguous())
    for qi in range(q.shape[0]):
        rs, ri = res[qi]
        assert rs.shape[0] >= k
        assert torch.equal(ri[:k], i[qi]) and torch.equal(rs[:k].view(torch.int32), s[qi].view(torch.int32))


# ------------------------------------------------------------------------------------------------------- filters
def test_mask_leaving_fewer_than_k_rows_pads(device: torch.device) -> None:
    n, k = 3000, 500
    eb = _bank(_rows(n, 64, 13).half(), device)
    allow = torch.zeros(n, dtype=torch.bool)
    allow[torch.randperm(n, generator=cases.gen(14))[:300]] = True
    q = _rows(5, 64, 15)
    exp = _oracle(eb.bank.cpu(), q, k, allow.numpy())
    assert (exp[1][:, 300:] == -1).all() and (exp[1][:, :300] >= 0).all()
    _check(eb, q, k, device, allow.numpy(), mask=allow.to(device))


def test_mask_leaving_about_2k_rows(device: torch.device) -> None:
    n, k = 50_000, 1000
    eb = _bank(_rows(n, 64, 16).half(), device)
    allow = torch.zeros(n, dtype=torch.bool)
    allow[torch.randperm(n, generator=cases.gen(17))[:2000]] = True
    rf = eb.row_filter(allow.to(device))
    _check(eb, _rows(70, 64, 18), k, device, allow.numpy(), mask=rf)


def test_exclude_group(device: torch.device) -> None:
    n, k = 4000, 300
    labels = torch.arange(n) // 500  # 8 groups of 500 rows
    eb = _bank(_rows(n, 40, 19).half(), device, row_groups=labels.to(device))
    q = _rows(9, 40, 20)
    own = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 99])  # (99: a label no row carries excludes nothing)
    allow = labels.numpy()[None, :] != own.numpy()[:, None]
    _check(eb, q, k, device, allow, exclude_group=own)
    mask = torch.rand(n, generator=cases.gen(21)) < 0.5
    _check(eb, q, k, device, allow & mask.numpy()[None, :], exclude_group=own, mask=mask.to(device))


def test_removed_rows_and_spare_capacity(device: torch.device) -> None:
    n, k = 3000, 400
    eb = _bank(_rows(n, 64, 22).half(), device, capacity=4000)
    gone = torch.randperm(n, generator=cases.gen(23))[:700]
    assert eb.remove(rows=gone.to(device)) == 700
    allow = np.ones(n, dtype=bool)
    allow[gone.numpy()] = False
    _check(eb, _rows(6, 64, 24), k, device, allow)


def test_an_appended_bank_equals_the_bank_built_at_once(device: torch.device) -> None:
    n, k = 6000, 1000
    rows = _rows(n, 64, 25).half()
    grown = _bank(rows[:2500], device, capacity=7000)
    grown.append(rows[2500:4000].to(device))
    grown.append(rows[4000:].to(device))
    whole = _bank(rows, device)
    q = _rows(20, 64, 26).to(device)
    a, b = grown.search(q, k), whole.search(q, k)
    _served_by_the_fast_path(grown)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    _same(a, _oracle(rows, q.cpu(), k))


# ------------------------------------------------------------------------------------------------------- ties and odd values
def test_ties_at_the_kth_resolve_by_lower_index_through_the_last_resort(device: torch.device) -> None:
    """6000 copies of one row among 10 000 rows, k = 4096.  For queries near the copied row the 4096 best are the copies
    with the lowest indices: 6000 candidates per query, which the fast path holds and its sort orders.  For queries opposite
    to it the 4000 other rows come first and the k-th falls among the copies again, so every row of the bank reaches the k-th
    score, the pass's candidate buffer (2 k + 512 per query) overflows and the last resort answers."""
    n, k = 10_000, 4096
    rows = _rows(n, 64, 27)
    copies = torch.randperm(n, generator=cases.gen(28))[:6000]
    rows[copies] = rows[int(copies[0])].clone()
    rows = rows.half()
    near = rows[int(copies[0])].float() + 0.05 * _rows(3, 64, 29)
    far = -rows[int(copies[0])].float() + 0.05 * _rows(3, 64, 30)
    lowest = np.sort(copies.numpy())
    eb = _bank(rows, device)
    _check(eb, near, k, device)
    np.testing.assert_array_equal(eb.search(near.to(device), k)[1].cpu().numpy()[0], lowest[:k])
    _check(eb, far, k, device, fast=False)
    np.testing.assert_array_equal(eb.search(far.to(device), k)[1].cpu().numpy()[2][-96:], lowest[:96])
    st = eb.last_status.cpu().tolist()
    assert st[0] == 1 and st[1] == 3, st  # the pass overflowed: its three queries took the last resort


def test_a_bank_of_one_repeated_row(device: torch.device) -> None:
    rows = _rows(1, 40, 30).repeat(700, 1).half()
    eb = _bank(rows, device)
    q = _rows(3, 40, 31)
    _check(eb, q, 300, device)
    assert eb.search(q.to(device), 300)[1].cpu().tolist() == [list(range(300))] * 3


def test_zero_nan_and_tiny_queries(device: torch.device) -> None:
    n, d, k = 900, 40, 200
    eb = _bank(_rows(n, d, 32).float(), device)
    q = _rows(5, d, 33)
    q[1] = 0.0
    q[2, 7] = float("nan")
    q[3] *= 1e-35 / float(q[3].norm())
    with np.errstate(invalid="ignore"):
        _check(eb, q, k, device, np.ones(n, dtype=bool), fast=False)  # (the lexsort form of the oracle ranks NaN last)
    assert int(eb.last_status[1]) == 3  # the zero, the NaN and the tiny query; the other two stay on the fast path
    s, i = eb.search(q.to(device), k)
    assert i[1].cpu().tolist() == list(range(k)) and i[2].cpu().tolist() == list(range(k))
    assert bool(torch.isnan(s[2]).all()) and bool((s[1] == 0).all())


def test_a_bank_with_a_nan_row_and_an_inf_row(device: torch.device) -> None:
    n, d, k = 1200, 32, 1200
    rows = _rows(n, d, 34).float()
    rows[17, 3] = float("nan")
    rows[400, 5] = float("inf")
    eb = _bank(rows, device)
    q = _rows(4, d, 35)
    with np.errstate(invalid="ignore"):
        _check(eb, q, k, device, np.ones(n, dtype=bool), fast=False)
    assert int(eb.last_status[1]) == 4  # the norm bound is not finite: every query takes the last resort
