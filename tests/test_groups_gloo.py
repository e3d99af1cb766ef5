"""The multi-rank grouped search on CPU: world sizes 2 and 3, gloo backend, 127.0.0.1 rendezvous.

The HIP kernels cannot run here, so the device hooks of `EmbeddingBank` are the oracle (tests/groups_oracle.py); the
sharding of `row_groups`, each rank's own label dictionary and query codes, the padding of short shards, the single
exchange, and the mapping of the padding to (-inf, -1) are the product code."""

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
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

from groups_oracle import oracle, oracle_bank_class  # noqa: E402


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case(n: int, group: int):
    import cases

    bank, queries = cases.search_case(n, 48, 6, torch.float16, seed=3)
    labels = torch.arange(n, dtype=torch.int64) // group * 3 + 1000
    rows = torch.tensor([0, n - 1, n // 2, 1, n // 3, 5]) % n
    queries = (bank[rows].float() + 0.05 * queries.float()).half()
    excl = labels[rows].clone()
    excl[5] = 7  # no row carries it
    queries[3] = 0
    return bank, queries, labels, excl


def _worker(rank: int, world: int, port: int, n: int, k: int, group: int, presharded: bool, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bank, queries, labels, excl = _case(n, group)
        lo, hi = rank * n // world, (rank + 1) * n // world
        cls = oracle_bank_class()
        if presharded:
            eb = cls(bank[lo:hi], dtype=torch.float16, normalize=False, process_group=dist.group.WORLD, presharded=True,
                     index_base=lo, row_groups=labels[lo:hi])
        else:
            eb = cls(bank, dtype=torch.float16, normalize=False, process_group=dist.group.WORLD, row_groups=labels)
        assert eb.index_base == lo and len(eb) == hi - lo
        # this rank's dictionary holds its own labels only, and its codes index it
        assert eb.group_labels.tolist() == sorted(set(labels[lo:hi].tolist()))
        assert torch.equal(eb.group_labels[eb._row_codes.long()], labels[lo:hi]) if hi > lo else True
        s1, i1 = eb.search(queries, k, exclude_group=excl)
        s2, i2 = eb.search(queries, k, exclude_group=excl.to(torch.int32))
        assert torch.equal(i1, i2) and np.array_equal(s1.numpy(), s2.numpy(), equal_nan=True)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), scores=s1.numpy(), indices=i1.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,group,presharded", [(2, 1001, 10, 49, False), (3, 1001, 10, 400, False),
                                                        (3, 1001, 20, 49, True), (2, 1001, 120, 600, False),
                                                        (3, 7, 5, 2, False)])
def test_sharded_grouped_search_equals_unsharded_oracle(world: int, n: int, k: int, group: int, presharded: bool,
                                                        tmp_path: Path) -> None:
    """group 400 / 600: groups span ranks, and a rank may hold no row a query may return.  (3, 7): every shard holds fewer
    rows than k."""
    mp.spawn(_worker, args=(world, _free_port(), n, k, group, presharded, str(tmp_path)), nprocs=world, join=True)
    bank, queries, labels, excl = _case(n, group)
    allow = labels.numpy()[None, :] != excl.numpy()[:, None]
    exp_s, exp_i = oracle(bank, queries, k, allow)
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        np.testing.assert_array_equal(z["indices"], exp_i)
        np.testing.assert_array_equal(z["scores"], exp_s)
