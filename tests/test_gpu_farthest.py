"""`EmbeddingBank.farthest_points` and `KMeans(init="farthest")` on the GPU.

The yardstick is `farthest_oracle.replay`: the greedy loop on top of the existing `bank.scores(bank.rows([c]), arange(len))`
with `near` and the pick done in numpy by the key order -- `idx` and `cover` must equal it bit for bit.  The picks must also
equal `farthest_oracle.greedy` (numpy float64 on the stored rows) after the test has asserted that greedy's closest decision
was further apart than 1e-6: a float32 score below 1 has an ulp of at most 6e-8 and float64 summation order moves a score by
about 1e-13, so a 1e-6 gap between rounded values cannot flip.

Shapes (n, d, m): (1, 8, 3) exhaustion; 255 / 256 / 257 rows the 256-row tile and, with d = 8, 70, 96, the K-step padding;
d = 520 crosses the 512-element stage of fp16 and d = 260 the 256-element stage of fp32 that `scores` runs in; 1030 rows
are four tiles and a partial one; d = 768 full-width rows."""

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
import farthest_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
SHAPES = ((1, 8, 3), (255, 8, 24), (256, 70, 24), (257, 96, 40), (513, 520, 40), (700, 260, 40), (1030, 64, 64),
          (300, 768, 32))


def _bits(t) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def _unit(n: int, d: int, seed: int, dtype: torch.dtype = F32) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1).to(dtype)


def _same(got: tuple, idx: np.ndarray, cover: np.ndarray) -> None:
    np.testing.assert_array_equal(got[0].cpu().numpy(), idx)
    np.testing.assert_array_equal(_bits(got[1]), _bits(cover))


def _equals_replay(eb, m: int, *, start=(), mask=None, allowed=None) -> tuple[np.ndarray, np.ndarray]:
    got = eb.farthest_points(m, start=list(start) if len(start) else None, mask=mask, return_near=True)
    idx, cover, near = farthest_oracle.replay(eb, m, start, allowed)
    _same(got, idx, cover)
    np.testing.assert_array_equal(_bits(got[2]), _bits(near))
    return idx, cover


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_picks_equal_the_replay_bit_for_bit_and_the_float64_greedy(shape, seed, dtype, device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d, m = shape
    eb = EmbeddingBank(_unit(n, d, seed).to(device), dtype=dtype)
    idx, cover = eb.farthest_points(m)
    assert idx.shape == (m,) and idx.dtype == torch.int64 and cover.shape == (m,) and cover.dtype == F32
    exp_i, exp_c, _ = farthest_oracle.replay(eb, m)
    _same((idx, cover), exp_i, exp_c)
    assert int(idx[0]) == 0 and float(cover[0]) == -math.inf
    if n < m:
        assert idx.cpu().tolist()[n:] == [-1] * (m - n) and bool((cover[n:] == -math.inf).all())
    g_i, g_c, _, gap = farthest_oracle.greedy(eb.bank, m)
    print(f"{shape} seed {seed} {dtype}: smallest gap between a pick and its runner-up {gap:.3e}")
    assert gap > 1e-6
    np.testing.assert_array_equal(idx.cpu().numpy(), g_i)


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_the_widest_rows_take_the_large_lds_path(dtype, device) -> None:
    """D = ISC_SEARCH_MAX_D: the centre's float64 image and its stored row need 80 KiB (fp16) / 96 KiB (fp32) of LDS, past
    the 64 KiB a kernel gets without asking."""
    from imagescry_amd import EmbeddingBank, _lib

    eb = EmbeddingBank(_unit(70, _lib.ISC_SEARCH_MAX_D, 5).to(device), dtype=dtype)
    _equals_replay(eb, 6)
    _equals_replay(eb, 3, start=(2, 40))


@pytest.fixture(scope="module")
def plain(device):
    """One bank and its answer, shared by the tests that compare `farthest_points` with itself."""
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(600, 100, 3).to(device), dtype=F16)
    idx, cover, near = eb.farthest_points(48, return_near=True)
    return eb, idx.clone(), cover.clone(), near.clone()


def test_a_smaller_m_is_a_prefix(plain) -> None:
    eb, idx, cover, _ = plain
    for j in (1, 2, 17, 47):
        got = eb.farthest_points(j)
        _same(got, idx[:j].cpu().numpy(), cover[:j].cpu().numpy())


def test_a_call_resumes_from_its_own_picks(plain) -> None:
    eb, idx, cover, near = plain
    for j in (1, 20, 47):
        got = eb.farthest_points(48 - j, start=idx[:j], return_near=True)
        _same(got, idx[j:].cpu().numpy(), cover[j:].cpu().numpy())
        np.testing.assert_array_equal(_bits(got[2]), _bits(near))
    dup = torch.cat([idx[:20], idx[:5]])  # duplicates in `start` are harmless
    _same(eb.farthest_points(28, start=dup), idx[20:].cpu().numpy(), cover[20:].cpu().numpy())


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_near_is_the_score_of_assign_against_the_centres(dtype, device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(700, 72, 4).to(device), dtype=dtype, capacity=1000)
    eb.remove(rows=[0, 13, 699])
    idx, cover, near = eb.farthest_points(30, start=[5, 13, 77], return_near=True)
    assert near.shape == (700,) and near.dtype == F32
    centres = torch.cat([torch.tensor([5, 77], device=device), idx])
    _, scores = eb.assign(eb.rows(centres))
    live = eb.live.cpu().numpy()
    np.testing.assert_array_equal(_bits(near)[live], _bits(scores)[live])
    assert bool((near.cpu()[~eb.live.cpu()] == -math.inf).all())
    # cover[t] is the near of pick t against the centres before it
    _, before = eb.assign(eb.rows(centres[:-1]))
    assert _bits(cover)[-1] == _bits(before)[int(idx[-1])]


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_changed_banks_equal_the_fresh_bank_of_their_rows(dtype, device) -> None:
    from imagescry_amd import EmbeddingBank

    n, d, m = 300, 100, 24
    rows = _unit(n, d, 20, dtype)

    def check(eb, keep: torch.Tensor, vectors: torch.Tensor, mask=None, start=()) -> None:
        """`keep`: the rows a pick may be; the fresh bank holds exactly those (and the start rows in front)."""
        index = keep.nonzero().squeeze(1)
        extra = torch.tensor([s for s in start if bool(eb.live[s])], dtype=torch.int64)
        fb = EmbeddingBank(torch.cat([vectors[extra], vectors[index]]).to(device), dtype=dtype, normalize=False)
        exp_i, exp_c = fb.farthest_points(m, start=list(range(len(extra))) or None)
        exp_i = exp_i.cpu()
        mapped = torch.where(exp_i >= 0, index[(exp_i - len(extra)).clamp_min(0)], exp_i)
        got = eb.farthest_points(m, mask=mask, start=list(start) or None)
        _same(got, mapped.numpy(), exp_c.cpu().numpy())

    everything = torch.ones(n, dtype=torch.bool)
    eb = EmbeddingBank(rows[:200].to(device), dtype=dtype, normalize=False, capacity=513)  # spare capacity
    check(eb, everything[:200], rows[:200])
    eb.append(rows[200:].to(device), normalize=False)
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
    # a removed start row is skipped; a start row outside the mask is a centre and is never picked
    outside = int((live & ~allow).nonzero()[0])
    keep = live & allow
    keep[[9, outside]] = False
    check(eb, keep, changed, mask=allow.to(device), start=(9, 77, outside))
    got, _ = eb.farthest_points(n, mask=allow.to(device), start=[outside])
    assert outside not in got.cpu().tolist() and int((got >= 0).sum()) == int((live & allow).sum())
    # a bank without spare room or holes, masked
    plain_bank = EmbeddingBank(rows.to(device), dtype=dtype, normalize=False)
    check(plain_bank, allow, rows, mask=allow.to(device))


def test_duplicates_a_zero_row_and_a_short_mask(device) -> None:
    from imagescry_amd import EmbeddingBank

    rows = _unit(300, 40, 30, F16)
    rows[[10, 150, 290]] = rows[3].clone()  # exact duplicates: ties go to the lower index
    rows[200] = 0
    eb = EmbeddingBank(rows.to(device), dtype=F16, normalize=False)
    idx, _ = _equals_replay(eb, 300)
    assert sorted(idx.tolist()) == list(range(300))
    where = {r: t for t, r in enumerate(idx.tolist())}
    assert where[3] < where[10] < where[150] < where[290]
    few = torch.zeros(300, dtype=torch.bool)
    few[[7, 150, 290]] = True
    idx, cover = _equals_replay(eb, 5, mask=few.to(device), allowed=few.numpy())
    assert idx.tolist() == [7, 150, 290, -1, -1] and cover[3:].tolist() == [-math.inf] * 2


def test_a_nan_row_and_an_inf_element(device) -> None:
    from imagescry_amd import EmbeddingBank

    rows = _unit(300, 40, 31)
    rows[17] = math.nan
    eb = EmbeddingBank(rows.to(device), dtype=F32, normalize=False)
    idx, cover = _equals_replay(eb, 20)
    assert idx[1] == 17 and cover[1] == -math.inf  # no centre gives it a number: picked at the first chance
    allow = torch.ones(300, dtype=torch.bool)
    allow[17] = False
    rest, rest_cover = eb.farthest_points(19, mask=allow.to(device))
    _same((rest, rest_cover), np.delete(idx, 1), np.delete(cover, 1))  # ... and changes nothing afterwards
    rows = _unit(300, 40, 32, F16)
    rows[21, 3] = math.inf
    eb = EmbeddingBank(rows.to(device), dtype=F16, normalize=False)
    _equals_replay(eb, 20)
    _equals_replay(eb, 5, start=(21, 4))


def test_a_captured_selection_replays_over_a_garbage_workspace(device) -> None:
    from imagescry_amd import EmbeddingBank

    eb = EmbeddingBank(_unit(700, 100, 33).to(device), dtype=F16, capacity=1000)
    first_i, first_c = eb.farthest_points(8)  # (loads the kernels and sizes the workspace before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no host read: a linear chain of launches
        idx, cover = eb.farthest_points(8)
    torch.cuda.synchronize()
    for _ in range(2):
        idx.fill_(-7)
        cover.fill_(-7.0)
        eb._farthest_ws.fill_(0xA5)  # the workspace's contents on entry do not matter
        graph.replay()
        torch.cuda.synchronize()
        _same((idx, cover), first_i.cpu().numpy(), first_c.cpu().numpy())


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_kmeans_from_farthest_points_recovers_the_planted_clusters(dtype, device) -> None:
    from imagescry_amd import EmbeddingBank, KMeans

    rows, planted, _ = assign_oracle.planted(clusters=6, per=50, d=32, noise=0.05)
    eb = EmbeddingBank(rows.to(device), dtype=dtype)
    picks, _ = eb.farthest_points(6)
    model = KMeans(6, init="farthest", seed=99)
    centres = model._initial_centers(eb, eb.live, 300)
    assert torch.equal(centres, eb.rows(picks).float())
    of_pick = (picks.cpu() // 50).tolist()
    assert sorted(of_pick) == list(range(6))  # one initial centre per planted cluster
    km = model.fit(eb)
    relabel = torch.empty(6, dtype=torch.int32)
    relabel[torch.tensor(of_pick)] = torch.arange(6, dtype=torch.int32)
    np.testing.assert_array_equal(km.labels.cpu().numpy(), relabel[planted.long()].numpy())
    assert km.counts.cpu().tolist() == [50] * 6
