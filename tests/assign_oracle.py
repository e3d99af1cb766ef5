"""numpy float64 restatement of `EmbeddingBank.assign` / `group_sums` (a helper, not a conftest), and the data generator of
the assign tests.

The score is `oracle.search_oracle.exact_scores` -- float32(dot_f64(q, b) / max(||q||, 1e-12)) with the centroid rounded to
the bank dtype first.  The label of a row is the centroid with the best key: score descending, NaN below every number,
-0.0 equal to +0.0, ties to the lower centroid; a row whose scores are all NaN gets label 0 and score NaN; a dead row gets
(-1, -inf)."""

from __future__ import annotations

import math

import numpy as np
import torch

from oracle import search_oracle


def make_data(n: int, d: int, c: int, seed: int) -> tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(n, d, generator=g)
    cent = torch.randn(c, d, generator=g)
    return rows, cent


def best_by_key(scores: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """float32 `[C, N]` scores -> (labels int32 `[N]`, scores float32 `[N]`) by the key above."""
    s = np.asarray(scores, dtype=np.float32)
    rank = np.where(np.isnan(s), -np.inf, s.astype(np.float64) + 0.0)  # NaN last; +0.0: both zeros compare equal anyway
    allnan = np.isnan(s).all(axis=0)
    labels = np.argmax(rank, axis=0).astype(np.int32)  # the first maximum: the lower centroid wins a tie
    cols = np.arange(s.shape[1])
    fix = np.isnan(s[labels, cols]) & ~allnan  # every number of the row is -inf: the first NUMBER wins, not a NaN before it
    labels[fix] = np.argmax(~np.isnan(s[:, fix]), axis=0).astype(np.int32)
    labels[allnan] = 0
    return labels, s[labels, np.arange(s.shape[1])]


def assign(stored: torch.Tensor, centroids: torch.Tensor, live: np.ndarray | None = None,
           dtype: torch.dtype | None = None) -> tuple[np.ndarray, np.ndarray]:
    """`stored`: the rows as the bank holds them (`bank.bank`); `centroids` are rounded to `dtype` (default: the rows')."""
    dtype = stored.dtype if dtype is None else dtype
    q = centroids.to(dtype)
    labels, scores = best_by_key(search_oracle.exact_scores(stored, q))
    if live is not None:
        labels = np.where(live, labels, -1).astype(np.int32)
        scores = np.where(live, scores, -math.inf).astype(np.float32)
    return labels, scores


def scores_f64(stored: torch.Tensor, centroids: torch.Tensor) -> np.ndarray:
    """The unrounded float64 scores `[C, N]` (for the gap check: how far apart a row's best two centroids are)."""
    b = stored.detach().cpu().numpy().astype(np.float64)
    q = centroids.to(stored.dtype).detach().cpu().numpy().astype(np.float64)
    denom = np.maximum(np.sqrt((q * q).sum(axis=1)), 1e-12)
    return (q @ b.T) / denom[:, None]


def smallest_gap(stored: torch.Tensor, centroids: torch.Tensor) -> float:
    """min over the rows of (best - second best float64 score); inf with one centroid."""
    s = scores_f64(stored, centroids)
    if s.shape[0] < 2:
        return math.inf
    top = np.sort(s, axis=0)[-2:]
    return float((top[1] - top[0]).min())


def group_sums(stored: torch.Tensor, labels: np.ndarray, num_groups: int,
               live: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    b = stored.detach().cpu().numpy().astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < num_groups)
    if live is not None:
        ok &= live
    sums = np.zeros((num_groups, b.shape[1]), dtype=np.float64)
    counts = np.zeros(num_groups, dtype=np.int64)
    for g in range(num_groups):
        sel = ok & (lab == g)
        counts[g] = int(sel.sum())
        if counts[g]:
            sums[g] = np.array([math.fsum(col) for col in b[sel].T])
    return sums, counts


def planted(clusters: int = 6, per: int = 50, d: int = 32, noise: float = 0.05,
            seed: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`clusters` x `per` unit rows around random unit directions, cluster by cluster: (rows, planted labels, the first row
    of each cluster)."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(clusters, d, generator=g), dim=1)
    rows = dirs.repeat_interleave(per, dim=0) + noise * torch.randn(clusters * per, d, generator=g)
    rows = torch.nn.functional.normalize(rows, dim=1)
    labels = torch.arange(clusters).repeat_interleave(per).to(torch.int32)
    return rows, labels, rows[::per].clone()
