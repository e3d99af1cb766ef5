"""The multi-rank collapsed search on CPU: world sizes 2 and 3, gloo backend, 127.0.0.1 rendezvous.

The HIP kernels cannot run here, so the device hooks of `EmbeddingBank` (`_local_collapse`, `_merge_groups`) are the
float64 oracle (tests/collapse_oracle.py); the sharding of `row_groups` (groups that span shard boundaries), each rank's
labels, the padding of short shards, the single exchange with its labels block and the mapping of the padding to
(-inf, -1, -1) are the product code."""

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

from collapse_oracle import collapse_bank_class, collapse_oracle  # noqa: E402


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case(n: int, group: int):
    import cases

    bank, queries = cases.search_case(n, 48, 6, torch.float16, seed=4)
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
        cls = collapse_bank_class()
        if presharded:
            eb = cls(bank[lo:hi], dtype=torch.float16, normalize=False, process_group=dist.group.WORLD, presharded=True,
                     index_base=lo, row_groups=labels[lo:hi])
        else:
            eb = cls(bank, dtype=torch.float16, normalize=False, process_group=dist.group.WORLD, row_groups=labels)
        out = {}
        for name, kw in (("plain", {}), ("excl", {"exclude_group": excl})):
            s, i, lab = eb.search_groups(queries, k, **kw)
            out[f"{name}_scores"], out[f"{name}_indices"], out[f"{name}_labels"] = s.numpy(), i.numpy(), lab.numpy()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,k,group,presharded", [(2, 1001, 10, 49, False), (3, 1001, 10, 400, False),
                                                        (3, 1001, 20, 49, True), (2, 1001, 120, 7, False),
                                                        (3, 7, 5, 2, False), (2, 1001, 10, 1001, False)])
def test_sharded_collapsed_search_equals_unsharded_oracle(world: int, n: int, k: int, group: int, presharded: bool,
                                                          tmp_path: Path) -> None:
    """group 400: groups span ranks (their leader may sit on either side).  (3, 7): every shard holds fewer rows than k.
    group 1001: one group, so every answer is one leader and padding."""
    mp.spawn(_worker, args=(world, _free_port(), n, k, group, presharded, str(tmp_path)), nprocs=world, join=True)
    bank, queries, labels, excl = _case(n, group)
    plain = collapse_oracle(bank, queries, k, labels.numpy())
    excluded = collapse_oracle(bank, queries, k, labels.numpy(), labels.numpy()[None, :] != excl.numpy()[:, None])
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        for name, exp in (("plain", plain), ("excl", excluded)):
            np.testing.assert_array_equal(z[f"{name}_indices"], exp[1])
            np.testing.assert_array_equal(z[f"{name}_labels"], exp[2])
            np.testing.assert_array_equal(z[f"{name}_scores"], exp[0])
