"""Shared by the CPU tests of per-query group exclusion: a bank whose device hooks are the float64 oracle."""

from __future__ import annotations

import numpy as np
import torch

PAD = torch.iinfo(torch.int64).max


def oracle(bank: torch.Tensor, queries: torch.Tensor, k: int, allow: np.ndarray, index_base: int = 0,
           pad=(-np.inf, -1)) -> tuple[np.ndarray, np.ndarray]:
    """Top-k per query over the rows `allow[q]` ([Q, N] bool) lets it return: (score desc with NaN last, row asc)."""
    from oracle import search_oracle

    nq = queries.shape[0]
    s = search_oracle.exact_scores(bank, queries)
    sc = np.full((nq, k), pad[0], np.float32)
    ix = np.full((nq, k), pad[1], np.int64)
    for q in range(nq):
        idx = np.nonzero(allow[q])[0]
        m = min(k, idx.size)
        o = np.lexsort((idx, -s[q, idx].astype(np.float64)))[:m]
        sc[q, :m], ix[q, :m] = s[q, idx[o]], idx[o] + index_base
    return sc, ix


def oracle_bank_class():
    from imagescry_amd import EmbeddingBank

    class OracleBank(EmbeddingBank):
        """The device hooks replaced: rows stay on the CPU, the "packed" row codes are the codes in row order."""

        def _store(self, embeddings, normalize):
            return embeddings.contiguous()

        def _pack_groups(self, codes):
            return codes.clone()

        def _local_topk(self, queries, kk, out=None, lane=-1, stream=None, mask=None, groups=None):
            assert groups is not None and groups.dtype == torch.int32 and groups.shape == (queries.shape[0],)
            allow = self._row_codes.numpy()[None, :] != groups.numpy()[:, None]
            if mask is not None:
                allow &= mask.packed.numpy()[None, :]
            s, i = oracle(self._bank, queries, kk, allow, self.index_base, pad=(np.nan, PAD))
            s, i = torch.from_numpy(s), torch.from_numpy(i)
            if out is not None:
                out[0].copy_(s), out[1].copy_(i), out[2].zero_()
            return s, i

        def _merge_topk(self, scores, indices, kk):  # (score desc with NaN last, index asc): isc_topk_merge's order
            s = scores.permute(1, 0, 2).reshape(scores.shape[1], -1).numpy()
            i = indices.permute(1, 0, 2).reshape(indices.shape[1], -1).numpy()
            order = [np.lexsort((i[q], -s[q].astype(np.float64)))[:kk] for q in range(s.shape[0])]
            return (torch.from_numpy(np.stack([s[q, o] for q, o in enumerate(order)])),
                    torch.from_numpy(np.stack([i[q, o] for q, o in enumerate(order)])))

    return OracleBank
