"""In-place append (`EmbeddingBank.append`, `capacity=`, `reserve`; isc_bank_append, isc_bank_repack) on the GPU.  The
check is always the same: a bank that received its rows through appends -- within a reserved capacity and across growths --
equals the bank built from all the rows at once, bit for bit, in everything a caller can see: `search`, `search_range`,
`search_exhaustive`, `search_groups`, `.bank`, `group_labels` and the norm bound.  The fresh bank takes the path a bank
without reserved capacity always took.  Small banks are also checked against the float64 oracle."""

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

QK = ((1, 1), (65, 10), (130, 120), (1, 10), (65, 120), (130, 1), (1, 120), (65, 1), (130, 10))  # Q x k, one per step


def _bank(rows: torch.Tensor, device: torch.device, **kw):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=kw.pop("dtype", rows.dtype), normalize=kw.pop("normalize", False), **kw)


def _rows(n: int, d: int, dtype: torch.dtype, seed: int, unit: bool = True) -> torch.Tensor:
    x = torch.randn(n, d, generator=cases.gen(seed))
    return (torch.nn.functional.normalize(x, dim=1) if unit else x * 3.0).to(dtype)


def _queries(nq: int, d: int, dtype: torch.dtype, seed: int, device: torch.device) -> torch.Tensor:
    return torch.randn(nq, d, generator=cases.gen(1000 + seed)).to(dtype).to(device)


def _same(got, exp, what: str = "") -> None:
    np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1].cpu().numpy(), err_msg=what)
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0].cpu().numpy(), err_msg=what)  # NaN == NaN here
    for g, e in zip(got[2:], exp[2:]):
        np.testing.assert_array_equal(g.cpu().numpy(), e.cpu().numpy(), err_msg=what)


def _same_range(got, exp, what: str = "") -> None:
    for name in ("offsets", "indices", "scores"):
        np.testing.assert_array_equal(getattr(got, name).cpu().numpy(), getattr(exp, name).cpu().numpy(), err_msg=what)


def _same_state(eb, fresh, what: str = "") -> None:
    assert len(eb) == len(fresh) == eb.num_local_rows and eb.capacity >= len(eb)
    assert torch.equal(eb.bank.view(torch.uint8), fresh.bank.view(torch.uint8)), what  # the stored bytes
    assert torch.equal(eb._norm_bound.view(torch.int32), fresh._norm_bound.view(torch.int32)), what
    if fresh.group_labels is not None:
        assert torch.equal(eb.group_labels, fresh.group_labels), what
        assert eb._max_group_rows == fresh._max_group_rows, what


def _same_answers(eb, fresh, step: int, device: torch.device, **kw) -> None:
    """The appended bank against the fresh one: stored rows, norm bound, one (Q, k) of the grid per step through `search`,
    then `search_exhaustive` and `search_range` (thresholds = the 5th scores) with 65 queries.  `exclude_group` holds
    130 labels: each call takes the first Q."""
    what = f"step {step}: {len(eb)} rows in capacity {eb.capacity}"
    _same_state(eb, fresh, what)
    nq, k = QK[step % len(QK)]
    k = min(k, len(eb))
    q = _queries(nq, eb.dim, eb.dtype, step, device)
    kq = {name: v[:nq] if name == "exclude_group" else v for name, v in kw.items()}
    _same(eb.search(q, k, **kq), fresh.search(q, k, **kq), what + f" search Q={nq} k={k}")
    kw = {name: v[:65] if name == "exclude_group" else v for name, v in kw.items()}
    q = _queries(65, eb.dim, eb.dtype, step + 50, device)
    k = min(5, len(eb))
    top = fresh.search_exhaustive(q, k, **kw)
    _same(eb.search_exhaustive(q, k, **kw), top, what + " exhaustive")
    thr = top[0][:, -1].clamp(min=-2.0).contiguous()  # (-inf padding of a filtered query: every row it may return)
    _same_range(eb.search_range(q, thr, **kw), fresh.search_range(q, thr, **kw), what + " range")


def _oracle_topk(stored: torch.Tensor, q: torch.Tensor, k: int) -> tuple[np.ndarray, np.ndarray]:
    s = search_oracle.exact_scores(stored, q.cpu().to(stored.dtype))
    idx = np.arange(s.shape[1])
    order = np.stack([np.lexsort((idx, -s[i].astype(np.float64)))[:k] for i in range(s.shape[0])])
    return np.take_along_axis(s, order, axis=1), order.astype(np.int64)


# (D, bank dtype, input dtype, normalize, start rows, capacity= (None: nothing reserved), appends)
F16, F32 = torch.float16, torch.float32
SEQUENCES = {
    # an empty start; capacity 256 = one tile, filled exactly (the bank goes back to the unmasked calls), then two growths
    "empty-256": (40, F16, F32, True, 0, 256, (1, 1, 31, 33, 190, 1, 255, 257)),
    # no reservation, capacities 1 and 2 (the identity permutation), a growth at every step: 1 -> 2 -> 4 -> 34 -> 68
    "one-row": (72, F32, F16, False, 1, None, (1, 1, 31, 33)),
    # capacity len + 1, then growths past one tile and past two
    "len+1": (40, F32, F32, True, 2, 3, (1, 257, 33, 255)),
    # 255 rows in capacity 257: the tile boundary inside the reserved room, exact fill, growth to 514 and its exact fill
    "255-257": (72, F16, F16, False, 255, 257, (1, 1, 255, 1, 1)),
    # capacity 513 filled in four steps, mask-word boundaries on the way (331, 364, 365)
    "300-513": (72, F16, F32, True, 300, 513, (31, 33, 1, 148)),
    # capacity 512 = two full tiles filled exactly, then a growth to 1024
    "300-512": (40, F16, F16, True, 300, 512, (33, 179, 257)),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_appended_bank_equals_fresh_bank(name: str, device: torch.device) -> None:
    d, dtype, in_dtype, normalize, start, capacity, appends = SEQUENCES[name]
    parts = [_rows(start, d, in_dtype, 1, unit=not normalize)]
    kw = {} if capacity is None else {"capacity": capacity}
    eb = _bank(parts[0], device, dtype=dtype, normalize=normalize, **kw)
    assert eb.capacity == (start if capacity is None else capacity) and len(eb) == start
    growths = 0
    for step, m in enumerate(appends):
        new = _rows(m, d, in_dtype, 10 + step, unit=not normalize)
        before, cap = len(eb), eb.capacity
        image, reserved = eb._bank.data_ptr(), eb._fill is not None
        assert eb.append(new.to(device)) == range(before, before + m)
        if before + m <= cap and reserved:
            assert eb.capacity == cap and eb._bank.data_ptr() == image  # in place
        else:
            assert eb.capacity == max(2 * cap, before + m)
            growths += 1
        parts.append(new)
        fresh = _bank(torch.cat(parts), device, dtype=dtype, normalize=normalize)
        assert fresh._fill is None and fresh.capacity == len(fresh)
        _same_answers(eb, fresh, step, device)
    if name in ("empty-256", "len+1"):
        assert growths >= 2
    q = _queries(65, d, dtype, 99, device)
    k = min(10, len(eb))
    exp = _oracle_topk(eb.bank.cpu(), q, k)
    got = eb.search(q, k)
    np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1])
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0])


def test_reserve_then_append_in_place(device: torch.device) -> None:
    """`reserve` on a bank built without capacity moves it once; the appends after it are in place."""
    parts = [_rows(300, 72, F16, 3)]
    eb = _bank(parts[0], device)
    eb.reserve(513)
    assert eb.capacity == 513 and len(eb) == 300
    _same_answers(eb, _bank(parts[0], device), 1, device)
    image = eb._bank.data_ptr()
    for step, m in enumerate((33, 180)):
        parts.append(_rows(m, 72, F16, 20 + step))
        eb.append(parts[-1].to(device))
        assert eb._bank.data_ptr() == image and eb.capacity == 513
        _same_answers(eb, _bank(torch.cat(parts), device), 2 + step, device)


def test_appended_copies_tie_in_ascending_index(device: torch.device) -> None:
    rows = _rows(300, 72, F16, 5)
    copies = rows[[5] * 20 + [7] * 13]
    eb = _bank(rows, device, capacity=600)
    eb.append(copies.to(device))
    fresh = _bank(torch.cat([rows, copies]), device)
    q = (rows[[5, 7, 9]].float() * 3.0).half().to(device)
    got = eb.search(q, 40)
    _same(got, fresh.search(q, 40))
    _same(eb.search_exhaustive(q, 40), fresh.search_exhaustive(q, 40))
    idx = got[1].cpu()
    assert idx[0, :21].tolist() == [5] + list(range(300, 320))
    assert idx[1, :14].tolist() == [7] + list(range(320, 333))
    assert bool((got[0][0, :21] == got[0][0, 0]).all()) and bool((got[0][1, :14] == got[0][1, 0]).all())


@pytest.mark.parametrize("dtype", [F16, F32])
def test_appended_nan_row_raises_the_norm_bound_to_inf(dtype: torch.dtype, device: torch.device) -> None:
    rows = _rows(300, 40, dtype, 6)
    new = _rows(33, 40, dtype, 7)
    new[4, 11] = float("nan")
    eb = _bank(rows, device, capacity=512)
    assert float(eb._norm_bound) < 1.1
    eb.append(new.to(device))
    assert float(eb._norm_bound) == float("inf")
    fresh = _bank(torch.cat([rows, new]), device)
    _same_state(eb, fresh)
    for nq, k in ((1, 10), (65, 120), (130, 1)):
        q = _queries(nq, 40, dtype, nq, device)
        _same(eb.search(q, k), fresh.search(q, k))
    q = _queries(65, 40, dtype, 8, device)
    _same(eb.search_exhaustive(q, 10), fresh.search_exhaustive(q, 10))
    _same_range(eb.search_range(q, 0.3), fresh.search_range(q, 0.3))


def test_grouped_bank_appends_old_new_and_negative_labels(device: torch.device) -> None:
    """Rows of existing labels, of labels sorting before, between and after them, and of a negative label; within the
    capacity and across a growth.  `exclude_group=`, `search_groups` and the planning figure equal the fresh bank's."""
    g = cases.gen(21)
    parts = [_rows(300, 72, F16, 9)]
    labels = [torch.randint(2, 12, (300,), generator=g) * 10]  # 20, 30, ..., 110
    eb = _bank(parts[0], device, capacity=513, row_groups=labels[0])
    codes = eb._row_codes.data_ptr()
    plan = ((31, torch.randint(2, 12, (31,), generator=g) * 10),  # existing labels
            (33, torch.tensor([5, 25, 999, -3] * 8 + [5])),  # before, between, after, negative
            (149, torch.randint(-1, 14, (149,), generator=g) * 10 + 5),  # ... 513 rows: full
            (257, torch.randint(0, 40, (257,), generator=g) * 5))  # growth; one label now holds the most rows anew
    for step, (m, lab) in enumerate(plan):
        parts.append(_rows(m, 72, F16, 30 + step))
        labels.append(lab)
        eb.append(parts[-1].to(device), row_groups=lab.to(torch.int32 if step % 2 else torch.int64))
        assert (eb._row_codes.data_ptr() == codes) == (step < 3)  # re-mapped in place until the growth
        all_labels = torch.cat(labels)
        fresh = _bank(torch.cat(parts), device, row_groups=all_labels)
        assert torch.equal(eb.group_labels, torch.unique(all_labels).to(device))
        excl = all_labels[torch.randint(0, all_labels.numel(), (130,), generator=g)].clone()
        excl[3] = 12345  # a label no row carries
        _same_answers(eb, fresh, step, device, exclude_group=excl)
        for nq, k in ((1, 1), (65, 10), (130, min(120, eb.group_labels.numel()))):
            q = _queries(nq, 72, F16, 60 + step, device)
            ex = all_labels[torch.randint(0, all_labels.numel(), (nq,), generator=g)]
            _same(eb.search_groups(q, k), fresh.search_groups(q, k), f"step {step} groups Q={nq} k={k}")
            _same(eb.search_groups(q, k, exclude_group=ex), fresh.search_groups(q, k, exclude_group=ex))
        q = _queries(65, 72, F16, 70 + step, device)
        _same(eb.search_groups_exhaustive(q, 10), fresh.search_groups_exhaustive(q, 10))


def test_filters_made_after_an_append_work_and_older_ones_are_refused(device: torch.device) -> None:
    rows, new = _rows(300, 40, F16, 11), _rows(33, 40, F16, 12)
    eb = _bank(rows, device, capacity=512)
    old = eb.row_filter(rows=[1, 2, 3])
    q = _queries(65, 40, F16, 13, device)
    eb.search(q, 3, mask=old)
    eb.append(new.to(device))
    with pytest.raises(ValueError, match="made before the bank changed; make it again"):
        eb.search(q, 3, mask=old)
    fresh = _bank(torch.cat([rows, new]), device)
    pick = torch.randperm(333, generator=cases.gen(14))[:40]
    rf, frf = eb.row_filter(rows=pick), fresh.row_filter(rows=pick)
    assert int(rf.allowed_count) == int(frf.allowed_count) == 40
    allow = (torch.rand(333, generator=cases.gen(15)) < 0.5).to(device)
    with pytest.raises(ValueError, match="allow must be a bool tensor"):
        eb.search(q, 10, mask=torch.ones(512, dtype=torch.bool, device=device))  # the real row count, not the capacity
    for k in (1, 10, 120):  # 40 allowed rows: k = 120 ends in padding
        _same(eb.search(q, k, mask=rf), fresh.search(q, k, mask=frf))
        _same(eb.search(q, k, mask=allow), fresh.search(q, k, mask=allow))
    _same(eb.search_exhaustive(q, 10, mask=allow), fresh.search_exhaustive(q, 10, mask=allow))
    _same_range(eb.search_range(q, 0.2, mask=rf), fresh.search_range(q, 0.2, mask=frf))
    got = eb.search(q, 120, mask=eb.row_filter(rows=pick, exclude=True))  # the complement never reaches the empty room
    assert int(got[1].min()) >= 0 and int(got[1].max()) < 333
    _same(got, fresh.search(q, 120, mask=fresh.row_filter(rows=pick, exclude=True)))


def test_unresolved_async_searches_see_the_bank_before_the_append(device: torch.device) -> None:
    rows, new = _rows(300, 72, F16, 16), _rows(257, 72, F16, 17)
    eb = _bank(rows, device, capacity=600)
    before, after = _bank(rows, device), _bank(torch.cat([rows, new]), device)
    q = [_queries(65, 72, F16, 18 + i, device) for i in range(3)]
    torch.cuda.synchronize()
    h0 = eb.search_async(q[0], 10)
    h1 = eb.search_async(q[1], 120)
    eb.append(new.to(device))
    h2 = eb.search_async(q[2], 10)
    _same(h2.result(), after.search(q[2], 10))
    _same(h0.result(), before.search(q[0], 10))
    _same(h1.result(), before.search(q[1], 120))


def test_captured_search_replays_over_rows_appended_in_place(device: torch.device) -> None:
    """A `search` captured on a bank with spare capacity holds the image, the fill bitmap and the norm bound by pointer; an
    append within the capacity updates all three in place, so the next replay answers for the new rows too."""
    rows, new = _rows(300, 72, F16, 22), _rows(33, 72, F16, 23)
    new[7] *= 2.0  # raises the norm bound the graph reads
    eb = _bank(rows, device, capacity=512)
    q = _queries(65, 72, F16, 24, device)
    out = {}

    def run():
        out["r"] = eb.search(q, 10)

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    torch.cuda.synchronize()
    q.copy_(_queries(65, 72, F16, 25, device))
    graph.replay()
    torch.cuda.synchronize()
    _same(out["r"], _bank(rows, device).search(q, 10))
    eb.append(new.to(device))
    graph.replay()
    torch.cuda.synchronize()
    fresh = _bank(torch.cat([rows, new]), device)
    _same(out["r"], fresh.search(q, 10))
    _same(out["r"], eb.search(q, 10))
    assert float(eb._norm_bound) == float(fresh._norm_bound) > 1.9


def test_bank_started_empty_and_filled_by_three_appends(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(torch.empty(0, 40, device=device), capacity=600, normalize=True)
    assert len(eb) == 0 and eb.capacity == 600 and eb.bank.shape == (0, 40)
    with pytest.raises(ValueError, match="exceeds the bank size 0"):
        eb.search(_queries(1, 40, F16, 1, device), 1)
    assert len(eb.search_range(_queries(3, 40, F16, 1, device), 0.0).indices) == 0
    parts = []
    for step, m in enumerate((300, 257, 43)):
        parts.append(_rows(m, 40, F32, 40 + step, unit=False))
        assert eb.append(parts[-1].to(device)) == range(sum(p.shape[0] for p in parts[:-1]), sum(p.shape[0] for p in parts))
        _same_answers(eb, _bank(torch.cat(parts), device, dtype=F16, normalize=True), step, device)
    assert eb.capacity == len(eb) == 600 and eb._as_filter(None) is None


def test_row_origin_is_extended_and_image_filters_see_the_new_image(device: torch.device) -> None:
    """A bank shaped like `from_database`'s (`row_origin`, grouped by image id) takes one more image."""
    def origin(image: int, cells: int) -> torch.Tensor:
        return torch.tensor([[image, c // 4, c % 4] for c in range(cells)], dtype=torch.int64)

    o = torch.cat([origin(i, 30) for i in (3, 4, 8, 9)])
    rows, new = _rows(120, 72, F16, 26), _rows(31, 72, F16, 27)
    eb = _bank(rows, device, capacity=256, row_groups=o[:, 0])
    eb.row_origin = o
    got = eb.append(new.to(device), row_groups=origin(6, 31)[:, 0], row_origin=origin(6, 31))
    assert got == range(120, 151) and eb.row_origin.shape == (151, 3) and eb.group_labels.tolist() == [3, 4, 6, 8, 9]
    fresh = _bank(torch.cat([rows, new]), device, row_groups=eb.row_origin[:, 0])
    q = _queries(65, 72, F16, 28, device)
    res = eb.search(q, 40, mask=eb.row_filter(image_ids=[6]))
    _same(res, fresh.search(q, 40, mask=fresh.row_filter(rows=torch.arange(120, 151))))
    assert sorted(res[1][0].tolist()) == [-1] * 9 + list(range(120, 151))
    _same(eb.search(q, 10, mask=eb.row_filter(image_ids=[6, 3], exclude=True)),
          fresh.search(q, 10, mask=fresh.row_filter(rows=torch.arange(30, 120))))
    _same(eb.search_groups(q, 5), fresh.search_groups(q, 5))
