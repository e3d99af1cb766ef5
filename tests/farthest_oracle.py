"""Two restatements of `EmbeddingBank.farthest_points` (a helper, not a conftest).

Both run the greedy loop of DESIGN.md ("Farthest-point selection") on the host in numpy: `near(r)` is the best score of row
r against the centres so far, -inf with none, "best" by the score half of `isc_make_key` (score descending, NaN below every
number, -0.0 equal to +0.0; a tie keeps the earlier value); every live row of `start` becomes a centre, then m times the
candidate whose `near` is LAST in that order is picked, ties to the lower row, and becomes a centre.

`replay` takes the scores of a centre from the EXISTING `bank.scores(bank.rows([c]), arange(len))`: the bit-level yardstick,
which runs no code of `farthest_points`.  `greedy` takes them from `oracle.search_oracle.exact_scores` (numpy float64, rounded
to float32 before every comparison) and also returns how close its closest decision was."""

from __future__ import annotations

import math

import numpy as np
import torch

from oracle import search_oracle


def score_bits(s: np.ndarray) -> np.ndarray:
    """The score half of `isc_make_key` for float32 `s`: uint32, larger = better."""
    s = np.asarray(s, dtype=np.float32)
    u = np.where(s == 0, np.float32(0.0), s).view(np.uint32)  # +0.0 for both zeros
    u = np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0), u).astype(np.uint32)


def _loop(scores_of, n: int, m: int, start, live: np.ndarray, allowed: np.ndarray):
    """`scores_of(c)`: float32 `[n]`, the scores of row c as a query against every row.  Returns (idx int64 [m], cover
    float32 [m], near float32 [n], smallest gap)."""
    near = np.full(n, -math.inf, dtype=np.float32)
    cand = live & allowed
    rows = np.arange(n, dtype=np.uint64)

    def add(c: int) -> None:
        s = np.asarray(scores_of(c), dtype=np.float32)
        better = live & (score_bits(s) > score_bits(near))
        near[better] = s[better]

    centres = 0
    for c in [int(r) for r in start]:
        cand[c] = False
        if live[c]:
            add(c)
            centres += 1
    idx = np.full(m, -1, dtype=np.int64)
    cover = np.full(m, -math.inf, dtype=np.float32)
    gap = math.inf
    for t in range(m):
        if not cand.any():
            break
        keys = (score_bits(near).astype(np.uint64) << np.uint64(32)) | rows
        keys[~cand] = np.uint64(2**64 - 1)
        r = int(np.argmin(keys))
        if centres and int(cand.sum()) > 1:  # with no centre every near is -inf and the index alone decides
            two = np.sort(near[cand].astype(np.float64))[:2]
            if not np.isnan(two).any():
                gap = min(gap, float(two[1] - two[0]))
        idx[t], cover[t] = r, near[r]
        cand[r] = False
        add(r)
        centres += 1
    return idx, cover, near, gap


def replay(bank, m: int, start=(), allowed: np.ndarray | None = None):
    """The loop on top of `bank.scores` / `bank.rows` (global row indices in and out).  `allowed`: bool `[len]` or None.
    Returns (idx, cover, near) as numpy arrays; a dead row's near is -inf."""
    n = len(bank)
    base = bank.index_base
    live = bank.live.cpu().numpy().astype(bool)
    every = torch.arange(base, base + n, device=bank.device)

    def scores_of(c: int) -> np.ndarray:
        return bank.scores(bank.rows([c + base]), every)[0].cpu().numpy()

    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool).copy()
    idx, cover, near, _ = _loop(scores_of, n, m, [int(r) - base for r in start], live, ok)
    return np.where(idx >= 0, idx + base, idx), cover, near


def greedy(stored: torch.Tensor, m: int, start=(), live: np.ndarray | None = None, allowed: np.ndarray | None = None):
    """The loop in numpy float64 on the rows as the bank holds them (`bank.bank`).  Returns (idx, cover, near, gap): `gap`
    is the smallest difference between the picked candidate's `near` and the runner-up's over all picks made with at least
    one centre (inf when there was no such pick)."""
    stored = stored.detach().cpu()
    n = stored.shape[0]
    lv = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool).copy()
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool).copy()

    def scores_of(c: int) -> np.ndarray:
        return search_oracle.exact_scores(stored, stored[c : c + 1])[0]

    return _loop(scores_of, n, m, start, lv, ok)
