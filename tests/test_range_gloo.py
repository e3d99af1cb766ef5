"""The multi-rank range search on CPU: world sizes 2 and 3, gloo backend, 127.0.0.1 rendezvous.

The HIP kernels cannot run here, so the device hooks of `EmbeddingBank` (`_store`, `_local_range`) are replaced by the
oracle in a test-only subclass; the row sharding, the index_base arithmetic, the exchange of the per-rank totals and rows,
the merge and the `max_results` check are the product code."""

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


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _range_oracle(bank: torch.Tensor, queries: torch.Tensor, thr: np.ndarray, index_base: int = 0):
    from oracle import search_oracle

    offs, sc, ix = [0], [], []
    if bank.shape[0]:
        s = search_oracle.exact_scores(bank, queries.to(bank.dtype))
    for qi in range(queries.shape[0]):
        if bank.shape[0] == 0:
            offs.append(offs[-1])
            continue
        sel = np.nonzero(s[qi] >= thr[qi])[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))
        sc.append(s[qi, sel[order]])
        ix.append(sel[order].astype(np.int64) + index_base)
        offs.append(offs[-1] + sel.size)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.empty(0, dt)  # noqa: E731
    return np.array(offs, np.int64), cat(sc, np.float32), cat(ix, np.int64)


def _case(n: int):
    import cases

    bank, queries = cases.search_case(max(n, 1), 32, 6, torch.float16, seed=9)
    bank = bank[:n]
    queries[2] = 0  # a zero query: every row scores 0
    if n:
        queries[0] = bank[n // 2].float()
    return bank, queries


def _worker(rank: int, world: int, port: int, n: int, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from imagescry_amd import EmbeddingBank
        from imagescry_amd.search import RangeResult

        class OracleBank(EmbeddingBank):
            def _store(self, embeddings, normalize):  # keep the rows on the CPU
                return embeddings.contiguous()

            def _local_range(self, queries, min_score, max_results):
                o, s, i = _range_oracle(self._bank, queries, min_score.numpy(), self.index_base)
                total = int(o[-1])
                if total > max_results:
                    return total, None
                return total, RangeResult(torch.from_numpy(o), torch.from_numpy(s), torch.from_numpy(i))

        bank, queries = _case(n)
        eb = OracleBank(bank, dtype=torch.float16, normalize=False, process_group=dist.group.WORLD)
        lo, hi = rank * n // world, (rank + 1) * n // world
        assert eb.index_base == lo and len(eb) == hi - lo
        out = {}
        thr = torch.tensor([0.5, 0.1, 0.0, -2.0, 0.3, 2.0], dtype=torch.float32)
        for name, t in (("scalar", 0.1), ("per_query", thr)):
            res = eb.search_range(queries, t)
            out[f"{name}_o"], out[f"{name}_s"], out[f"{name}_i"] = (res.offsets.numpy(), res.scores.numpy(),
                                                                   res.indices.numpy())
            assert len(res) == queries.shape[0]
        total = int(out["per_query_o"][-1])
        if total:
            with pytest.raises(ValueError, match=str(total)):
                eb.search_range(queries, thr, max_results=total - 1)
        with pytest.raises(ValueError):
            eb.search_range(queries, float("nan"))
        with pytest.raises(ValueError):
            eb.search_range(queries, torch.zeros(3))
        with pytest.raises(TypeError):
            eb.search_range(queries, torch.zeros(6, dtype=torch.float64))
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 1001), (3, 7), (3, 2)])
def test_sharded_range_equals_unsharded_oracle(world: int, n: int, tmp_path: Path) -> None:
    """(3, 2): one of the three ranks holds no row."""
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    bank, queries = _case(n)
    thr = np.array([0.5, 0.1, 0.0, -2.0, 0.3, 2.0], np.float32)
    for name, t in (("scalar", np.full(6, 0.1, np.float32)), ("per_query", thr)):
        exp_o, exp_s, exp_i = _range_oracle(bank, queries, t)
        assert exp_o[-1] > 0
        for r in range(world):
            z = np.load(tmp_path / f"rank{r}.npz")
            np.testing.assert_array_equal(z[f"{name}_o"], exp_o)
            np.testing.assert_array_equal(z[f"{name}_i"], exp_i)
            np.testing.assert_array_equal(z[f"{name}_s"], exp_s)
