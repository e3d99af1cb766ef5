"""The multi-rank masked search on CPU: world sizes 2 and 3, gloo backend, 127.0.0.1 rendezvous.

The HIP kernels cannot run here, so the device hooks of `EmbeddingBank` (`_store`, `_pack_filter`, `_local_topk`,
`_merge_topk`) are replaced by the oracle in a test-only subclass; slicing the global filter per rank, the padding of
short shards, the single exchange, and the mapping of the padding to (-inf, -1) are the product code."""

from __future__ import annotations

import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

PAD = torch.iinfo(torch.int64).max


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _oracle(bank: torch.Tensor, queries: torch.Tensor, k: int, allow: np.ndarray, index_base: int = 0,
            pad=(-np.inf, -1)) -> tuple[np.ndarray, np.ndarray]:
    from oracle import search_oracle

    idx = np.nonzero(allow)[0]
    sc = np.full((queries.shape[0], k), pad[0], np.float32)
    ix = np.full((queries.shape[0], k), pad[1], np.int64)
    m = min(k, idx.size)
    if m:  # (score desc with NaN last, row asc) over the allowed rows
        s = search_oracle.exact_scores(bank[torch.from_numpy(idx)], queries)
        for q in range(s.shape[0]):
            o = np.lexsort((idx, -s[q].astype(np.float64)))[:m]
            sc[q, :m], ix[q, :m] = s[q, o], idx[o] + index_base
    return sc, ix


def _case(n: int, which: str):
    import cases

    bank, queries = cases.search_case(n, 48, 6, torch.float16, seed=3)
    queries[2] = 0
    rng = np.random.default_rng(n)
    if which == "random":
        allow = rng.random(n) < 0.3
    else:  # rows of the first rank's shard only (two ranks, or three, with the others allowing nothing)
        allow = np.zeros(n, bool)
        allow[: max(1, n // 4)] = True
    if n > 600:
        bank[600] = float("nan")  # a NaN row, allowed, on a later rank than most of the real answers
        allow[600] = True
    return bank, queries, allow


def _worker(rank: int, world: int, port: int, n: int, k: int, which: str, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from imagescry_amd import EmbeddingBank, RowFilter

        class OracleBank(EmbeddingBank):
            def _store(self, embeddings, normalize):  # keep the rows on the CPU
                return embeddings.contiguous()

            def _pack_filter(self, local):  # the "bitmap" is the local bool rows
                return RowFilter(self, local.clone(), local.sum().reshape(1))

            def _local_topk(self, queries, kk, out=None, lane=-1, stream=None, mask=None):
                assert mask is not None and mask.packed.shape == (len(self),)
                s, i = _oracle(self._bank, queries, kk, mask.packed.numpy(), self.index_base, pad=(np.nan, PAD))
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

        bank, queries, allow = _case(n, which)
        eb = OracleBank(bank, dtype=torch.float16, normalize=False, process_group=dist.group.WORLD)
        lo, hi = rank * n // world, (rank + 1) * n // world
        assert eb.index_base == lo and len(eb) == hi - lo
        rf = eb.row_filter(torch.from_numpy(allow))
        assert rf.packed.tolist() == allow[lo:hi].tolist()
        s1, i1 = eb.search(queries, k, mask=rf)
        s2, i2 = eb.search(queries, k, mask=torch.from_numpy(allow))
        rows = np.nonzero(allow)[0]
        s3, i3 = eb.search(queries, k, mask=eb.row_filter(rows=rows.tolist()))
        for s, i in ((s2, i2), (s3, i3)):
            assert torch.equal(i, i1) and np.array_equal(s.numpy(), s1.numpy(), equal_nan=True)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), scores=s1.numpy(), indices=i1.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,which", [(2, 1001, 10, "random"), (3, 1001, 10, "first_rank"),
                                             (2, 1001, 120, "first_rank"), (3, 7, 5, "random"), (3, 7, 5, "first_rank")])
def test_sharded_masked_search_equals_unsharded_oracle(world: int, n: int, k: int, which: str, tmp_path: Path) -> None:
    """"first_rank": every other rank has no allowed row and still takes part in the exchange.  (3, 7): every shard holds
    fewer rows than k."""
    mp.spawn(_worker, args=(world, _free_port(), n, k, which, str(tmp_path)), nprocs=world, join=True)
    bank, queries, allow = _case(n, which)
    exp_s, exp_i = _oracle(bank, queries, k, allow)
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        np.testing.assert_array_equal(z["indices"], exp_i)
        np.testing.assert_array_equal(z["scores"], exp_s)
