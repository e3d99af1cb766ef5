"""`EmbeddingBank.assign` / `assign_exhaustive` / `group_sums` and `KMeans` on the GPU.

`assign` (isc_bank_assign: a float32 matrix-core filter, an exact float64 finish, a proof per row) must equal
`assign_exhaustive` (the float64 kernel) and the argmax by key of `bank.scores(centroids, all rows)`, labels and score
bits; its labels must equal the numpy float64 oracle's (tests/assign_oracle.py) wherever that oracle's best two scores are
further apart than summation order can matter -- every row of every shape, which the test asserts first.

Shapes (n, d, c) cover the 256-row tile (255 / 256 / 257 / 513), the K-step padding (d = 8, 24, 40, 72, 100 against 32- and
64-element steps), the centroid tile (c = 2, 16 | 64 / 65, 255 / 256 / 257) and the pass of 1024 centroids (1025).  At
d = 768 the filter's bound (9e-5) exceeds many gaps between a row's best two centroids, so the multi-candidate re-score
runs on plain data.

`group_sums` is compared with `math.fsum` per component under the bound of any-order float64 summation,
|err| <= n_g 2^-53 sum |x| (first order in 2^-53, valid for n_g < 2^26)."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import assign_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
SHAPES = ((1, 8, 1), (1, 8, 3), (255, 64, 2), (256, 64, 64), (257, 72, 65), (513, 100, 255), (513, 64, 256), (600, 24, 257),
          (1000, 768, 16), (700, 40, 1025), (300, 8, 1025))


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _status(eb) -> tuple[int, int, float]:
    st = eb.last_assign_status.cpu().numpy()
    return int(st[0]), int(st[1]), float(st[2:3].view(np.float32)[0])


def _unit(n: int, d: int, seed: int, dtype: torch.dtype = F32) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1).to(dtype)


def _agree(eb, cent, *, mask=None) -> tuple[torch.Tensor, torch.Tensor]:
    """`assign` == `assign_exhaustive` (labels, score bits; NaN scores as NaN) and the proof held; returns assign's answer and
    leaves ITS status words (not those of the exhaustive call made here) in `eb.assign_status`."""
    labels, scores = eb.assign(cent, mask=mask)
    st = eb.assign_status = _status(eb)
    ex_l, ex_s = eb.assign_exhaustive(cent, mask=mask)
    np.testing.assert_array_equal(labels.cpu().numpy(), ex_l.cpu().numpy())
    a, b = scores.cpu().numpy(), ex_s.cpu().numpy()
    both_nan = np.isnan(a) & np.isnan(b)
    np.testing.assert_array_equal(_bits(scores)[~both_nan], _bits(ex_s)[~both_nan])
    assert st[2] < 1.0, st
    return labels, scores


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assign_equals_the_exhaustive_kernel_the_scores_and_the_oracle(shape, seed, dtype, device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d, c = shape
    rows, cent = assign_oracle.make_data(n, d, c, seed)
    eb = EmbeddingBank(rows.to(device), dtype=dtype)
    cent = cent.to(device)
    labels, scores = eb.assign(cent)
    status = _status(eb)
    print(f"{shape} seed {seed} {dtype}: status {status}")
    assert labels.shape == (n,) and labels.dtype == torch.int32 and scores.shape == (n,) and scores.dtype == F32
    # the float64 kernel, bit for bit
    ex_l, ex_s = eb.assign_exhaustive(cent)
    np.testing.assert_array_equal(labels.cpu().numpy(), ex_l.cpu().numpy())
    np.testing.assert_array_equal(_bits(scores), _bits(ex_s))
    # the argmax by key of the score table, bit for bit
    table = eb.scores(cent, torch.arange(n, device=device))
    key_l, key_s = assign_oracle.best_by_key(table.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), key_l)
    np.testing.assert_array_equal(_bits(scores), key_s.view(np.uint32))
    assert status[2] < 1.0
    assert status[1] == 0  # finite, well-scaled data: the filter proves every row
    if d == 768:
        assert status[0] > 0  # gaps below the bound: rows with several candidates
    # the numpy oracle on the stored rows: no row is left out, because no row is close to a tie
    stored = eb.bank.cpu()
    gap = assign_oracle.smallest_gap(stored, cent.cpu())
    print(f"  smallest float64 gap between a row's best two centroids: {gap:.3e}")
    assert gap > 1e-9
    np.testing.assert_array_equal(labels.cpu().numpy(), assign_oracle.assign(stored, cent.cpu())[0])
    # labels alone: the same labels
    only, none = eb.assign(cent, return_scores=False)
    assert none is None
    np.testing.assert_array_equal(only.cpu().numpy(), labels.cpu().numpy())


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_exact_ties_go_to_the_lower_centroid(dtype, device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(600, 72, 3).to(device), dtype=dtype)
    base = _unit(2, 72, 4).to(dtype).float()
    cent = torch.stack([base[0], base[1], base[0], 2 * base[0], base[1], 2 * base[1]]).to(device)
    labels, scores = _agree(eb, cent)
    assert set(labels.cpu().tolist()) == {0, 1}
    table = eb.scores(cent, torch.arange(600, device=device))
    np.testing.assert_array_equal(_bits(table[0]), _bits(table[2]))
    np.testing.assert_array_equal(_bits(table[0]), _bits(table[3]))  # 2 q / ||2 q||: the same bits
    key_l, key_s = assign_oracle.best_by_key(table.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), key_l)
    np.testing.assert_array_equal(_bits(scores), key_s.view(np.uint32))
    # the duplicates first: still the lower index
    swapped = cent[[2, 4, 0, 1]]
    l2, _ = _agree(eb, swapped)
    assert set(l2.cpu().tolist()) == {0, 1}


def test_a_zero_centroid(device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(300, 40, 5).to(device), dtype=F16)
    cent = torch.cat([torch.zeros(1, 40), _unit(2, 40, 6)]).to(device)
    labels, scores = _agree(eb, cent)
    table = eb.scores(cent, torch.arange(300, device=device))
    key_l, _ = assign_oracle.best_by_key(table.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), key_l)
    zero_wins = (table[1:] < 0).all(dim=0)
    assert bool(zero_wins.any()) and bool((labels[zero_wins] == 0).all()) and bool((scores[zero_wins] == 0).all())
    # all centroids zero: every score is zero, every row ties, label 0
    l0, s0 = _agree(eb, torch.zeros(3, 40, device=device))
    assert bool((l0 == 0).all()) and bool((s0 == 0).all())


def test_a_nan_centroid_ranks_last(device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(300, 40, 7).to(device), dtype=F32)
    good = _unit(2, 40, 8)
    cent = torch.stack([good[0], torch.full((40,), math.nan), good[1]]).to(device)
    labels, scores = _agree(eb, cent)
    assert set(labels.cpu().tolist()) <= {0, 2} and bool(torch.isfinite(scores).all())
    ref_l, ref_s = eb.assign(good.to(device))
    np.testing.assert_array_equal((labels // 2).cpu().numpy(), ref_l.cpu().numpy())
    np.testing.assert_array_equal(_bits(scores), _bits(ref_s))
    alone_l, alone_s = _agree(eb, cent[1:2])
    assert bool((alone_l == 0).all()) and bool(torch.isnan(alone_s).all())
    nan_first = cent[[1, 0]]
    l3, _ = _agree(eb, nan_first)
    assert bool((l3 == 1).all())


def test_a_bank_row_with_inf_takes_the_exhaustive_path(device) -> None:
    from imagescry_amd import EmbeddingBank

    rows = _unit(300, 40, 9, F16)
    rows[17, 3] = math.inf
    eb = EmbeddingBank(rows.to(device), dtype=F16, normalize=False)
    cent = _unit(5, 40, 10).to(device)
    labels, scores = eb.assign(cent)
    st = _status(eb)
    assert st[1] > 0
    ex_l, ex_s = eb.assign_exhaustive(cent)
    np.testing.assert_array_equal(labels.cpu().numpy(), ex_l.cpu().numpy())
    np.testing.assert_array_equal(np.nan_to_num(scores.cpu().numpy(), nan=7.0), np.nan_to_num(ex_s.cpu().numpy(), nan=7.0))
    table = eb.scores(cent, torch.arange(300, device=device))
    key_l, _ = assign_oracle.best_by_key(table.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), key_l)


def test_centroids_one_fp16_ulp_apart(device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(513, 64, 11).to(device), dtype=F16)
    a = _unit(1, 64, 12, F16)[0]
    b = a.clone()
    b[5] = torch.from_numpy(np.nextafter(a.numpy()[5:6], np.float16(np.inf)))[0]
    other = _unit(1, 64, 13, F16)[0]
    cent = torch.stack([b, a, other]).to(device)
    assert int((cent[0] != cent[1]).sum()) == 1
    labels, scores = _agree(eb, cent)
    print(f"one ulp apart: status {eb.assign_status}")
    assert eb.assign_status[0] > 0  # the filter cannot separate them: re-scored exactly
    table = eb.scores(cent, torch.arange(513, device=device))
    key_l, key_s = assign_oracle.best_by_key(table.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), key_l)
    np.testing.assert_array_equal(_bits(scores), key_s.view(np.uint32))
    assert {0, 1} <= set(labels.cpu().tolist())


def test_forty_near_equal_centroids_overflow_the_candidate_list(device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(300, 64, 14).to(device), dtype=F32)
    a = _unit(1, 64, 15)
    g = torch.Generator().manual_seed(16)
    cent = torch.cat([a + 1e-7 * torch.randn(40, 64, generator=g), _unit(3, 64, 17)]).to(device)
    labels, scores = _agree(eb, cent)
    st = eb.assign_status
    print(f"40 near-equal centroids: status {st}")
    assert st[1] > 0  # rows nearest to the cloud cannot keep 40 candidates: the float64 kernel answers them
    table = eb.scores(cent, torch.arange(300, device=device))
    key_l, key_s = assign_oracle.best_by_key(table.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), key_l)
    np.testing.assert_array_equal(_bits(scores), key_s.view(np.uint32))


def test_float32_centroids_equal_the_pre_rounded_ones(device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(513, 100, 18).to(device), dtype=F16)
    cent = (torch.randn(70, 100, generator=torch.Generator().manual_seed(19)) * 1.5).to(device)
    l32, s32 = _agree(eb, cent)
    l16, s16 = _agree(eb, cent.half())
    np.testing.assert_array_equal(l32.cpu().numpy(), l16.cpu().numpy())
    np.testing.assert_array_equal(_bits(s32), _bits(s16))
    wide = torch.full((70, 124), 9.0, device=device)  # ldc > D: the padding is never read
    wide[:, :100] = cent
    lw, sw = eb.assign(wide[:, :100])
    np.testing.assert_array_equal(lw.cpu().numpy(), l32.cpu().numpy())
    np.testing.assert_array_equal(_bits(sw), _bits(s32))


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_capacity_remove_replace_and_mask_equal_the_fresh_bank(dtype, device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d = 300, 100
    rows = _unit(n, d, 20, dtype)
    cent = _unit(70, d, 21).to(device)

    def fresh(vectors: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
        fb = EmbeddingBank(vectors.to(device), dtype=dtype, normalize=False)
        labels, scores = fb.assign(cent)
        return labels.cpu().numpy(), _bits(scores)

    def check(eb, live: torch.Tensor, vectors: torch.Tensor, mask=None) -> None:
        labels, scores = _agree(eb, cent, mask=mask)
        only, _ = eb.assign(cent, mask=mask, return_scores=False)
        np.testing.assert_array_equal(only.cpu().numpy(), labels.cpu().numpy())
        exp_l, exp_s = fresh(vectors[live])
        lv = live.numpy()
        np.testing.assert_array_equal(labels.cpu().numpy()[lv], exp_l)
        np.testing.assert_array_equal(_bits(scores)[lv], exp_s)
        assert bool((labels.cpu()[~live] == -1).all()) and bool((scores.cpu()[~live] == -math.inf).all())

    everything = torch.ones(n, dtype=torch.bool)
    eb = EmbeddingBank(rows.to(device), dtype=dtype, normalize=False, capacity=513)  # spare capacity
    assert len(eb) == n and eb.capacity == 513
    check(eb, everything, rows)
    gone = torch.tensor([0, 1, 77, 255, 256, 299])
    eb.remove(rows=gone)
    live = everything.clone()
    live[gone] = False
    check(eb, live, rows)
    new = _unit(3, d, 22, dtype)
    eb.replace(torch.tensor([5, 100, 298]), new.to(device), normalize=False)
    changed = rows.clone()
    changed[[5, 100, 298]] = new
    check(eb, live, changed)
    allow = torch.rand(n, generator=torch.Generator().manual_seed(23)) < 0.6
    check(eb, live & allow, changed, mask=allow.to(device))
    check(eb, live & allow, changed, mask=eb.row_filter(allow.to(device)))
    # a bank without spare room or holes, masked
    plain = EmbeddingBank(rows.to(device), dtype=dtype, normalize=False)
    check(plain, allow, rows, mask=allow.to(device))


def test_a_captured_assign_replays_bit_identically(device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d, c = 1000, 768, 80
    rows, cent = assign_oracle.make_data(n, d, c, 2)
    eb = EmbeddingBank(rows.to(device), dtype=F16)
    q = cent.to(device)
    labels = torch.empty(n, dtype=torch.int32, device=device)
    scores = torch.empty(n, dtype=F32, device=device)
    eb._assign_rows(q, None, labels, scores, False)  # (loads the kernels and sizes the workspace before the capture)
    torch.cuda.synchronize()
    first_l, first_s, first_st = labels.clone(), scores.clone(), eb.last_assign_status.clone()
    assert int(first_st[0]) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eb._assign_rows(q, None, labels, scores, False)
    status = eb.last_assign_status
    torch.cuda.synchronize()
    for _ in range(2):
        labels.fill_(-7)
        scores.fill_(-7.0)
        eb._assign_ws.fill_(0xA5)  # the workspace's contents on entry do not matter
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(labels.cpu().numpy(), first_l.cpu().numpy())
        np.testing.assert_array_equal(_bits(scores), _bits(first_s))
        np.testing.assert_array_equal(status.cpu().numpy(), first_st.cpu().numpy())
    # new centroids in the captured buffer: the replay answers them
    q.copy_(torch.randn(c, d, generator=torch.Generator().manual_seed(3)).to(device))
    graph.replay()
    torch.cuda.synchronize()
    eager_l, eager_s = eb.assign_exhaustive(q)
    np.testing.assert_array_equal(labels.cpu().numpy(), eager_l.cpu().numpy())
    np.testing.assert_array_equal(_bits(scores), _bits(eager_s))


# ------------------------------------------------------------------ group_sums
def _fsum_check(eb, labels: torch.Tensor, g: int, live: np.ndarray | None = None) -> None:
    sums, counts = eb.group_sums(labels, g)
    again, counts2 = eb.group_sums(labels, g)
    np.testing.assert_array_equal(sums.cpu().numpy().view(np.uint64), again.cpu().numpy().view(np.uint64))  # same bits
    np.testing.assert_array_equal(counts.cpu().numpy(), counts2.cpu().numpy())
    stored = eb.bank.cpu()
    exp_s, exp_c = assign_oracle.group_sums(stored, labels.cpu().numpy(), g, live)
    np.testing.assert_array_equal(counts.cpu().numpy(), exp_c)  # exact
    lab = labels.cpu().numpy().astype(np.int64)
    ok = np.ones(len(lab), dtype=bool) if live is None else live
    mag = np.zeros_like(exp_s)
    absrows = np.abs(stored.numpy().astype(np.float64))
    for k in range(g):
        mag[k] = absrows[ok & (lab == k)].sum(axis=0)
    bound = exp_c[:, None] * 2.0**-53 * mag
    err = np.abs(sums.cpu().numpy() - exp_s)
    print(f"group_sums G={g}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("dtype,d", ((F16, 100), (F32, 40), (F16, 768)), ids=("f16-100", "f32-40", "f16-768"))
def test_group_sums_against_fsum(dtype, d, device) -> None:
    from imagescry_amd import EmbeddingBank

    n = 3000 if d < 768 else 1300
    eb = EmbeddingBank(_unit(n, d, 24).to(device), dtype=dtype)
    g = torch.Generator().manual_seed(25)
    # five groups of ~n/6 rows (they span the 1024-entry chunks of the sorted list) and labels outside [0, 5)
    labels = torch.randint(-1, 7, (n,), generator=g).to(device)
    _fsum_check(eb, labels, 5)
    _fsum_check(eb, labels.to(torch.int32), 7)
    # one group: every row; first, interior and last chunk
    _fsum_check(eb, torch.zeros(n, dtype=torch.int64, device=device), 1)
    # many small groups, some of them empty: summed inside a chunk
    _fsum_check(eb, torch.randint(0, 700, (n,), generator=g).to(device), 700)
    # sorted labels with a boundary exactly on a chunk edge
    edge = torch.cat([torch.zeros(1024, dtype=torch.int64), torch.ones(n - 1024, dtype=torch.int64)]).to(device)
    _fsum_check(eb, edge, 3)


def test_group_sums_ignore_removed_rows(device) -> None:
    from imagescry_amd import EmbeddingBank

    n = 1500
    eb = EmbeddingBank(_unit(n, 72, 26).to(device), dtype=F16, capacity=2000)
    labels = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(27)).to(device)
    gone = torch.arange(0, n, 7)
    eb.remove(rows=gone)
    live = np.ones(n, dtype=bool)
    live[gone.numpy()] = False
    _fsum_check(eb, labels, 4, live)
    assign_l, _ = eb.assign(_unit(4, 72, 28).to(device))
    sums, counts = eb.group_sums(assign_l, 4)  # -1 labels of the removed rows are outside [0, 4)
    assert int(counts.sum()) == int(live.sum())


# ------------------------------------------------------------------ KMeans
@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_kmeans_recovers_the_planted_clusters(dtype, device) -> None:
    from imagescry_amd import EmbeddingBank, KMeans

    rows, planted, first = assign_oracle.planted(clusters=6, per=50, d=32, noise=0.05)
    eb = EmbeddingBank(rows.to(device), dtype=dtype)
    km = KMeans(6, init=first).fit(eb)
    np.testing.assert_array_equal(km.labels.cpu().numpy(), planted.numpy())
    assert km.counts.cpu().tolist() == [50] * 6
    assert km.cluster_centers.shape == (6, 32) and km.cluster_centers.dtype == F32 and km.cluster_centers.device == eb.device
    obj = np.array(km.objective)
    print(f"objective {obj}, {km.num_iter} iterations")
    assert (np.diff(obj) >= -1e-12).all() and obj[-1] > 0.9
    np.testing.assert_array_equal(km.predict(eb).cpu().numpy(), km.labels.cpu().numpy())
    # sampled initial centroids: seeded
    a = KMeans(6, seed=1, tol=0.0).fit(eb)
    b = KMeans(6, seed=1, tol=0.0).fit(eb)
    np.testing.assert_array_equal(a.labels.cpu().numpy(), b.labels.cpu().numpy())
    assert a.objective == b.objective and a.num_iter == b.num_iter
    np.testing.assert_array_equal(a.predict(eb).cpu().numpy(), a.labels.cpu().numpy())
