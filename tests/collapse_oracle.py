"""The float64 oracle of the collapsed (distinct-group) search, built on `oracle.search_oracle.exact_scores`: per query,
every group's best key (score desc with NaN last, row asc) among the rows it may return, then the best k groups."""

from __future__ import annotations

import numpy as np
import torch

PAD = torch.iinfo(torch.int64).max


def collapse_oracle(bank, queries, k: int, labels, allow: np.ndarray | None = None, index_base: int = 0,
                    pad=(-np.inf, -1, -1)) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`(scores [Q, k], rows [Q, k], labels [Q, k])`: each query's k best groups by their leaders, padded with `pad`.
    `labels`: int `[N]`; `allow`: optional bool `[Q, N]` (the rows query q may return)."""
    from oracle import search_oracle

    s = search_oracle.exact_scores(bank, queries)
    lab = np.asarray(labels, dtype=np.int64)
    nq = s.shape[0]
    sc = np.full((nq, k), pad[0], np.float32)
    ix = np.full((nq, k), pad[1], np.int64)
    lb = np.full((nq, k), pad[2], np.int64)
    for q in range(nq):
        idx = np.nonzero(allow[q])[0] if allow is not None else np.arange(s.shape[1])
        order = idx[np.lexsort((idx, -s[q, idx].astype(np.float64)))]
        # the first row of each label in key order is the label's leader; leaders stay in key order
        _, first = np.unique(lab[order], return_index=True)
        lead = order[np.sort(first)][:k]
        m = lead.size
        sc[q, :m], ix[q, :m], lb[q, :m] = s[q, lead], lead + index_base, lab[lead]
    return sc, ix, lb


def collapse_bank_class():
    """`EmbeddingBank` whose device hooks are this oracle: rows stay on the CPU, the "packed" codes are the codes in row
    order (the CPU rehearsal of the sharded collapsed search)."""
    from imagescry_amd import EmbeddingBank

    class OracleBank(EmbeddingBank):
        def _store(self, embeddings, normalize):
            return embeddings.contiguous()

        def _pack_groups(self, codes):
            return codes.clone()

        def _local_collapse(self, queries, kk, out=None, mask=None, groups=None):
            codes = self._row_codes.numpy()
            allow = np.ones((queries.shape[0], codes.size), bool)
            if groups is not None:
                allow &= codes[None, :] != groups.numpy()[:, None]
            if mask is not None:
                allow &= mask.packed.numpy()[None, :]
            s, i, c = collapse_oracle(self._bank, queries, kk, codes, allow, self.index_base, pad=(np.nan, PAD, -1))
            s, i = torch.from_numpy(s), torch.from_numpy(i)
            if out is not None:
                out[0].copy_(s), out[1].copy_(i), out[2].zero_()
            return s, i, self._labels_of(torch.from_numpy(c).to(torch.int32))

        def _merge_groups(self, scores, indices, labels, kk):  # best entry per label, then isc_topk_merge's order
            g, nq, kin = scores.shape
            s = scores.permute(1, 0, 2).reshape(nq, -1).numpy()
            i = indices.permute(1, 0, 2).reshape(nq, -1).numpy()
            lab = labels.permute(1, 0, 2).reshape(nq, -1).numpy()
            out = (np.full((nq, kk), np.nan, np.float32), np.full((nq, kk), PAD, np.int64), np.full((nq, kk), -1, np.int64))
            for q in range(nq):
                o = np.lexsort((i[q], -s[q].astype(np.float64)))
                seen, keep = set(), []
                for e in o:
                    if i[q, e] != PAD:
                        if lab[q, e] in seen:
                            continue
                        seen.add(lab[q, e])
                    keep.append(e)
                keep = np.array(keep[:kk], np.int64)
                out[0][q, : keep.size], out[1][q, : keep.size] = s[q, keep], i[q, keep]
                out[2][q, : keep.size] = np.where(i[q, keep] == PAD, -1, lab[q, keep])
            return tuple(torch.from_numpy(a) for a in out)

    return OracleBank
