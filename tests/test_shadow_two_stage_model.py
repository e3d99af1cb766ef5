"""Host model of the two-stage re-score after an int8 level (cosine_topk.hip, k_rescore).  This tests
the RULE, not the kernel: quantise tiles and a query as the kernels do (the model of tests/test_shadow_inequality.py), run
the int8 test with the level's threshold tau, score the P = 2 kp entries with the best approximate score, raise the threshold
to tau' and drop what the int8 test rejects against tau'.  Two properties make the level exact:

  * every row stage B drops has a float64 score <= tau';
  * tau' <= the kp-th best float32 score of the carried candidates and the kept entries, so the next selection's
    threshold is at least tau'.

Neither may depend on the approximate scores being any good: one case ranks the entries by noise."""

from __future__ import annotations

import numpy as np
import pytest
from test_shadow_inequality import F, _quantise, _threshold

TILE = 256


def _model(bank: np.ndarray, query: np.ndarray, kp: int, seen: int, approx_noise: bool = False, carried: bool = True):
    """bank [n, d], the first `seen` rows were searched before the level.  Returns the quantities of the two properties."""
    bank = bank.astype(np.float16).astype(F)
    query = query.astype(np.float16).astype(F)
    with np.errstate(all="ignore"):
        exact = bank.astype(np.float64) @ query.astype(np.float64)
        f32 = (bank @ query).astype(F)
    # carried candidates: the kp best float32 scores of the rows seen; tau = the kp-th (k_select)
    if carried:
        order = np.argsort(-np.nan_to_num(f32[:seen], nan=-np.inf), kind="stable")[:kp]
        carry = f32[:seen][order]
        tau = F(carry[kp - 1])
    else:  # a query that carries nothing yet: no threshold
        carry = np.zeros(0, F)
        tau = F(-np.inf)
    qi, cq, eq, qn = _quantise(query[None, :])
    rows, accs, recs = [], [], []
    for t0 in range(seen, bank.shape[0], TILE):
        tile = bank[t0 : t0 + TILE]
        if np.all(np.isfinite(tile)):
            xi, ct, et, nt = _quantise(tile)
        else:  # a tile with a non-finite value: n_t = +inf, every row passes
            xi, ct, et, nt = np.zeros(tile.shape, np.int64), F(1), F(0), F(np.inf)
        acc = xi @ qi[0]
        thr = _thr(tau, cq, qn, eq, ct, et, nt)
        for r in np.nonzero(acc > thr)[0]:
            rows.append(t0 + r)
            accs.append(int(acc[r]))
            recs.append((ct, et, nt))
    rows = np.array(rows, dtype=np.int64)
    accs = np.array(accs, dtype=np.int64)
    # stage A: the best P by approximate score
    with np.errstate(all="ignore"):
        approx = np.array([F(a) / F(cq * r[0]) if np.isfinite(r[2]) else -np.inf for a, r in zip(accs, recs)], dtype=F)
    if approx_noise:
        approx = np.random.default_rng(1).standard_normal(len(rows)).astype(F)
    p = min(2 * kp, len(rows))
    first = np.argsort(-approx, kind="stable")[:p]
    scores = np.concatenate([carry, f32[rows[first]]])
    scores = np.where(np.isnan(scores), -np.inf, scores).astype(F)
    tau2 = tau
    if len(scores) >= kp:
        tau2 = max(tau, F(np.sort(scores)[::-1][kp - 1]))
    # stage B
    in_first = np.zeros(len(rows), bool)
    in_first[first] = True
    passes = np.array([a > _thr(tau2, cq, qn, eq, *r) for a, r in zip(accs, recs)], dtype=bool)
    dropped = rows[~in_first & ~passes]
    fetched = rows[in_first | passes]
    kept = fetched[f32[fetched] > tau]
    return exact, f32, carry, tau, tau2, dropped, kept, len(rows), len(fetched)


def _thr(tau, cq, qn, eq, ct, et, nt) -> int:
    if not nt < np.inf:  # the kernel's special case
        return -(2**31) if F(tau * cq) < np.inf else 2**31 - 1
    return _threshold(F(tau), cq, qn, eq, ct, et, nt)


def _assert_exact(result, kp: int) -> None:
    exact, f32, carry, tau, tau2, dropped, kept, _, _ = result
    assert tau2 >= tau or np.isnan(tau)
    assert not np.any(exact[dropped] > np.float64(tau2))
    pool = np.concatenate([carry, f32[kept]])
    if tau2 > tau:  # a raised threshold is the kp-th best of scores that stay
        assert len(pool) >= kp
    if len(pool) >= kp:
        assert np.sort(pool)[::-1][kp - 1] >= tau2


@pytest.mark.parametrize("d,kp", [(64, 16), (100, 16), (768, 16), (768, 64)])
@pytest.mark.parametrize("noise", [False, True])
def test_random_unit_rows(d: int, kp: int, noise: bool) -> None:
    rng = np.random.default_rng(d + kp)
    seen, n = 4 * TILE, 36 * TILE  # a level of ratio 8
    bank = rng.standard_normal((n, d))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    for _ in range(3):
        result = _model(bank, rng.standard_normal(d), kp, seen, approx_noise=noise)
        _assert_exact(result, kp)
        if not noise and d == 768 and kp == 16:  # what the stage is for: most false positives are never fetched
            assert result[8] < result[7] // 2


def test_duplicates_tie_at_the_threshold() -> None:
    rng = np.random.default_rng(2)
    d, kp, seen, n = 64, 16, 4 * TILE, 20 * TILE
    bank = rng.standard_normal((n, d))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    bank[seen + 10 : seen + 50] = bank[seen + 5]  # forty copies: tau' is their score, and the other copies tie with it
    _assert_exact(_model(bank, bank[seen + 5].copy(), kp, seen), kp)
    bank[5 : 5 + kp] = bank[seen + 5]  # ... and the carried list is full of them too: tau itself is the tie
    _assert_exact(_model(bank, bank[seen + 5].copy(), kp, seen), kp)


def test_adversarial_tiles() -> None:
    rng = np.random.default_rng(3)
    d, kp, seen, n = 768, 16, 2 * TILE, 10 * TILE
    # every element at +-max
    bank = np.where(rng.random((n, d)) < 0.5, -1.0, 1.0) * 0.25
    query = np.where(rng.random(d) < 0.5, -1.0, 1.0) * 3.0
    _assert_exact(_model(bank, query, kp, seen), kp)
    # every residual at +-0.5, aligned with the query
    qsteps = rng.integers(-100, 100, size=d) + 0.5
    query = qsteps / 127.0
    query[0] = 1.0
    bank = (np.rint(rng.standard_normal((n, d)) * 30) + 0.5 * np.sign(qsteps)) / 127.0
    bank[:, 0] = 1.0
    _assert_exact(_model(bank, query, kp, seen), kp)
    # row norms from 1e-3 to 1e3 inside every tile: the tile's scale is the huge rows'
    bank = rng.standard_normal((n, d)) * np.power(10.0, rng.random((n, 1)) * 6 - 3) / np.sqrt(d)
    for scale in (1.0, 1e-2):
        _assert_exact(_model(bank, rng.standard_normal(d) * scale, kp, seen), kp)


def test_non_finite_tile_and_short_lists() -> None:
    rng = np.random.default_rng(4)
    d, kp, seen, n = 64, 16, 2 * TILE, 6 * TILE
    bank = rng.standard_normal((n, d))
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    query = rng.standard_normal(d)
    bad = bank.copy()
    bad[seen + TILE + 7, 3] = np.inf  # every row of that tile passes both tests; none may set a NaN threshold
    result = _model(bad, query, kp, seen)
    assert not np.isnan(result[4])
    _assert_exact(result, kp)
    # fewer than kp scores in all: tau' = tau (here no threshold at all), nothing is dropped
    result = _model(bank[: seen + 8], query, kp, seen, carried=False)
    assert result[4] == result[3] and len(result[5]) == 0
    _assert_exact(result, kp)
