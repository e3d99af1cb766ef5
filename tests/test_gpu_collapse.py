"""Collapsed (distinct-group) search on the GPU (`EmbeddingBank.search_groups`; isc_cosine_topk_collapse,
isc_cosine_topk_exhaustive_collapse, isc_topk_merge_groups).  Checked three ways, bit for bit: against the float64 oracle
(tests/collapse_oracle.py), against the float64 sweep on the device (`search_groups_exhaustive`), and against the row
search (singleton groups equal `search`; each returned group equals `search(q, 1)` masked to that group)."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import cases  # noqa: E402
from collapse_oracle import collapse_oracle  # noqa: E402

pytestmark = pytest.mark.gpu


def _bank(rows: torch.Tensor, device: torch.device, labels: torch.Tensor, dtype=None, normalize=False):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=dtype or rows.dtype, normalize=normalize, row_groups=labels)


def _same(got, exp, what: str = "") -> None:
    gs, gi, gl = (t.cpu().numpy() for t in got)
    es, ei, el = exp
    assert np.array_equal(gi, ei), (what, np.argwhere(gi != ei)[:5])
    assert np.array_equal(gl, el), what
    assert np.array_equal(gs.view(np.uint32), np.asarray(es, np.float32).view(np.uint32)) or \
        np.array_equal(gs, es, equal_nan=True), what


def _oracle(eb, q: torch.Tensor, k: int, labels: torch.Tensor, allow=None):
    """The oracle on the stored rows, the queries rounded to the bank dtype as the search does."""
    return collapse_oracle(eb.bank.cpu(), q.cpu().to(eb.dtype), k, labels.numpy(), allow)


def _case(n: int, d: int, nq: int, dtype: torch.dtype, group: int, seed: int):
    """Unit rows in groups of about `group` adjacent rows with random labels, queries near banked rows."""
    g = cases.gen(seed)
    bank = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    ids = torch.randperm(n // group + 1, generator=g)[torch.arange(n) // group] * 7 - 50  # negative labels too
    src = torch.randint(0, n, (nq,), generator=g)
    q = bank[src] + 0.3 * torch.nn.functional.normalize(torch.randn(nq, d, generator=g), dim=1)
    return bank.to(dtype), q.to(dtype), ids


# ------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize(
    "nq,k,dtype,qdtype",
    [(1, 10, torch.float16, torch.float16), (1, 1, torch.float32, torch.float32), (64, 10, torch.float16, torch.float32),
     (64, 120, torch.float32, torch.float16), (100, 10, torch.float16, torch.float16), (128, 1, torch.float32, torch.float32),
     (300, 10, torch.float16, torch.float16), (1024, 10, torch.float32, torch.float32), (1100, 10, torch.float16, torch.float32),
     (200, 120, torch.float16, torch.float16)],
)
def test_collapsed_topk_matches_oracle_and_exhaustive(nq, k, dtype, qdtype, device: torch.device) -> None:
    bank, q, labels = _case(6000, 64, nq, dtype, 7, seed=nq + k)
    eb = _bank(bank, device, labels)
    qd = q.to(qdtype).to(device)
    got = eb.search_groups(qd, k)
    exp = _oracle(eb, q.to(qdtype), k, labels)
    _same(got, exp, "fast")
    _same(eb.search_groups_exhaustive(qd, k), exp, "exhaustive")
    assert int(eb.last_status[0]) == 0


def test_singleton_groups_equal_search(device: torch.device) -> None:
    bank, q, _ = _case(20000, 96, 70, torch.float16, 1, seed=5)
    labels = torch.randperm(20000, generator=cases.gen(6)) + 10**12  # every row its own group, labels far from rows
    eb = _bank(bank, device, labels)
    for k in (1, 10, 120):
        s, i, lab = eb.search_groups(q.to(device), k)
        es, ei = eb.search(q.to(device), k)
        assert torch.equal(i, ei) and torch.equal(s, es), k
        assert torch.equal(lab.cpu(), labels[i.cpu()]), k
        assert int(eb.last_status[1]) == 0


def test_each_group_is_its_masked_best_row(device: torch.device) -> None:
    bank, q, labels = _case(8000, 64, 6, torch.float32, 49, seed=8)
    eb = _bank(bank, device, labels)
    qd = q.to(device)
    s, i, lab = eb.search_groups(qd, 10)
    s1, i1 = eb.search(qd, 1)
    assert torch.equal(s[:, 0], s1[:, 0]) and torch.equal(i[:, 0], i1[:, 0])
    for qi in range(qd.shape[0]):
        assert len(set(lab[qi].tolist())) == 10
        for j in range(10):
            ms, mi = eb.search(qd[qi : qi + 1], 1, mask=(labels == int(lab[qi, j])).to(device))
            assert int(mi[0, 0]) == int(i[qi, j]) and torch.equal(ms[0, 0], s[qi, j]), (qi, j)


def test_database_ordered_near_duplicate_cells(device: torch.device) -> None:
    """3 000 images x 49 nearly identical adjacent cells: the top rows of a cell query are one or two images."""
    g = cases.gen(31)
    images, cells, d = 3000, 49, 96
    centres = torch.nn.functional.normalize(torch.randn(images, d, generator=g), dim=1)
    rows = (centres[:, None, :] + 0.05 * torch.randn(images, cells, d, generator=g)).reshape(images * cells, d)
    labels = torch.arange(images * cells) // cells
    eb = _bank(rows, device, labels, dtype=torch.float16, normalize=True)
    stored = eb.bank.cpu()
    q = stored[torch.randint(0, images * cells, (96,), generator=g)].float() + 0.01 * torch.randn(96, d, generator=g)
    for k in (10, 30):
        got = eb.search_groups(q.to(device), k)
        st = eb.last_status.cpu().tolist()
        _same(got, collapse_oracle(stored, q.half(), k, labels.numpy()), str(k))
        assert st[0] == 0 and st[1] == 0, st
        assert len(set(got[2][0].tolist())) == k


def test_exact_copies_and_ties_across_groups(device: torch.device) -> None:
    bank, q = cases.tie_case(torch.float16)  # 24 distinct rows, each 40 times (row i = base[i % 24])
    n = bank.shape[0]
    for labels in (torch.arange(n) % 24, torch.arange(n) // 24, torch.arange(n) // 7):  # copies inside / ties across
        eb = _bank(bank, device, labels)
        for k in (1, 10, 30):
            kk = min(k, int(labels.unique().numel()))
            got = eb.search_groups(q.to(device), kk)
            exp = _oracle(eb, q, kk, labels)
            _same(got, exp, str(k))
            _same(eb.search_groups_exhaustive(q.to(device), kk), exp)


def test_one_group_of_identical_rows_reaches_the_exhaustive_pass(device: torch.device) -> None:
    g = cases.gen(9)
    d = 64
    other = torch.nn.functional.normalize(torch.randn(5000, d, generator=g), dim=1)
    dup = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1).repeat(20000, 1)
    rows = torch.cat([other[:2000], dup, other[2000:]]).half()
    labels = torch.cat([torch.arange(2000), torch.full((20000,), 99999), torch.arange(2000, 5000)])
    eb = _bank(rows, device, labels)
    q = torch.cat([dup[:1] + 0.01 * torch.randn(1, d, generator=g), other[:3]]).half()
    got = eb.search_groups(q.to(device), 10)
    _same(got, _oracle(eb, q, 10, labels))
    assert int(got[1][0, 0]) == 2000 and int(got[2][0, 0]) == 99999  # the copies' leader is the lowest row


def test_fewer_groups_than_k_pad(device: torch.device) -> None:
    bank, q, _ = _case(500, 32, 5, torch.float32, 1, seed=10)
    labels = torch.arange(500) % 4
    eb = _bank(bank, device, labels)
    s, i, lab = eb.search_groups(q.to(device), 10)
    assert bool((i[:, 4:] == -1).all()) and bool((lab[:, 4:] == -1).all()) and bool(torch.isinf(s[:, 4:]).all())
    _same((s, i, lab), _oracle(eb, q, 10, labels))
    ex = torch.tensor([0, 1, 2, 3, 7])
    got = eb.search_groups(q.to(device), 10, exclude_group=ex)
    _same(got, _oracle(eb, q, 10, labels, labels.numpy()[None, :] != ex.numpy()[:, None]))
    assert bool((got[1][:4, 3:] == -1).all()) and bool((got[1][4, :4] >= 0).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_mask_with_exclude_group(dtype: torch.dtype, device: torch.device) -> None:
    bank, q, labels = _case(9000, 64, 130, dtype, 49, seed=11)
    eb = _bank(bank, device, labels)
    allow = torch.rand(9000, generator=cases.gen(12)) < 0.4
    excl = labels[torch.randint(0, 9000, (130,), generator=cases.gen(13))]
    a = allow.numpy()[None, :] & (labels.numpy()[None, :] != excl.numpy()[:, None])
    for k in (1, 10, 100):
        exp = _oracle(eb, q, k, labels, a)
        _same(eb.search_groups(q.to(device), k, mask=allow.to(device), exclude_group=excl), exp, str(k))
        _same(eb.search_groups_exhaustive(q.to(device), k, mask=allow.to(device), exclude_group=excl), exp, str(k))


def test_nan_rows_zero_and_nonfinite_queries(device: torch.device) -> None:
    bank, q, labels = _case(1500, 64, 70, torch.float32, 49, seed=14)
    q[0] = 0
    q[1, 5] = float("inf")
    q[2, 9] = float("nan")
    eb = _bank(bank, device, labels)
    for k in (1, 10):
        exp = _oracle(eb, q, k, labels)
        _same(eb.search_groups(q.to(device), k), exp, "finite bank")
        _same(eb.search_groups_exhaustive(q.to(device), k), exp)
    bank[[3, 700, 701]] = float("nan")
    eb = _bank(bank, device, labels)
    for k in (1, 10, 60):
        exp = _oracle(eb, q, k, labels)
        _same(eb.search_groups(q.to(device), k), exp, "nan rows")
        _same(eb.search_groups_exhaustive(q.to(device), k), exp)


def test_eight_presharded_banks_merge_to_the_whole(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank, shard_bounds
    from imagescry_amd.search import _unpad_groups

    bank, q, labels = _case(20000, 64, 40, torch.float16, 49, seed=15)  # groups span shard boundaries
    whole = _bank(bank, device, labels)
    qd = q.to(device)
    for k in (1, 10, 120):
        parts = []
        for r in range(8):
            lo, hi = shard_bounds(20000, 8, r)
            sh = EmbeddingBank(bank[lo:hi].to(device), dtype=torch.float16, normalize=False, presharded=True, index_base=lo,
                               row_groups=labels[lo:hi])
            parts.append(sh._local_collapse(qd, k))
        s, i, lab = (torch.stack([p[j] for p in parts]) for j in range(3))
        merged = _unpad_groups(*whole._merge_groups(s, i, lab, k))
        got = whole.search_groups(qd, k)
        for a, b in zip(merged, got):
            assert torch.equal(a, b), k
        _same(got, _oracle(whole, q, k, labels), str(k))


def test_database_bank_groups_by_image(tmp_path: Path, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank, storage

    g = cases.gen(22)
    maps = [(100 + i, torch.randn(32, 7, 7, generator=g)) for i in range(40)]
    storage.write_embeddings(tmp_path, maps, checkpoint_id=1)
    eb = EmbeddingBank.from_database(tmp_path, device=device)
    stored = eb.bank.cpu()
    rows = torch.tensor([3, 7 * 49 + 24, 39 * 49 + 48, 100, 1500])
    q = stored[rows].float()
    s, i, img = eb.search_groups(q.to(device), 10)
    assert torch.equal(img[:, 0].cpu(), eb.row_origin[rows, 0])  # a banked cell's best image is its own
    assert torch.equal(eb.row_origin[i.cpu(), 0], img.cpu())
    _same((s, i, img), collapse_oracle(stored, q.half(), 10, eb.row_origin[:, 0].numpy()))
    s2, i2, img2 = eb.search_groups(q.to(device), 10, exclude_group=img[:, 0].cpu())
    assert torch.equal(img2[:, :9], img[:, 1:]) and torch.equal(i2[:, :9], i[:, 1:])


# ---------------------------------------------------------------------------------------------------- scale
def test_ten_million_rows_collapsed(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d, nq, k = 10_000_000, 768, 64, 10
    gen = torch.Generator(device=device).manual_seed(24)
    rows = torch.empty((n, d), dtype=torch.float16, device=device)
    for r0 in range(0, n, 1 << 20):
        blk = torch.randn((min(1 << 20, n - r0), d), generator=gen, device=device)
        rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
    src = torch.arange(nq, device=device) * (n // nq) + 7
    q = rows[src].float() + 0.05 * torch.randn((nq, d), generator=gen, device=device)
    labels = torch.arange(n, device=device) // 49
    eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False, row_groups=labels)
    del rows
    s, i, lab = eb.search_groups(q, k)
    st = eb.last_status.cpu()
    assert int(st[1]) == 0, st
    assert torch.equal(lab, i // 49) and torch.equal(lab[:, 0], src // 49)
    assert all(len(set(r)) == k for r in lab.tolist())
    s1, i1 = eb.search(q, 1)
    assert torch.equal(s[:, 0], s1[:, 0]) and torch.equal(i[:, 0], i1[:, 0])
    sample = torch.tensor([0, 17, 63], device=device)
    es, ei, el = eb.search_groups_exhaustive(q[sample], k)
    assert torch.equal(i[sample], ei) and torch.equal(s[sample], es) and torch.equal(lab[sample], el)
    # property: each returned group's leader is that group's masked best row
    for j in range(0, k, 3):
        ms, mi = eb.search(q[:1], 1, mask=(labels == lab[0, j]))
        assert int(mi[0, 0]) == int(i[0, j]) and torch.equal(ms[0, 0], s[0, j])
