"""Host-side logic of `EmbeddingBank.search` / `search_async` / `search_exhaustive` beyond k = 120: the limits of every call,
the `_local_topk` hook above 120, the padding of a filtered answer and the sharded refusal.  No device is touched: the rows
stay on the CPU and the search hook is the float64 oracle (the HostBank of tests/test_rows_host.py)."""

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

sys.path.insert(0, str(Path(__file__).resolve().parent))

from test_rows_host import HostBank  # noqa: E402

from imagescry_amd import EmbeddingBank, _lib  # noqa: E402
from oracle import search_oracle  # noqa: E402


def _rows(n: int, d: int = 8, seed: int = 0) -> torch.Tensor:
    return torch.nn.functional.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


def _bank(n: int, **kw) -> HostBank:
    return HostBank(_rows(n), dtype=torch.float32, normalize=False, **kw)


@pytest.mark.parametrize("k", [121, 500])
def test_search_beyond_120_equals_the_oracle(k: int) -> None:
    eb, q = _bank(700), _rows(5, seed=1)
    exp_s, exp_i = search_oracle.cosine_topk(eb._bank, q, k)
    for s, i in (eb.search(q, k), eb.search_async(q, k).result()):
        np.testing.assert_array_equal(i.numpy(), exp_i)
        np.testing.assert_array_equal(s.numpy(), exp_s)
    assert eb.calls == [("topk", k), ("topk", k)]  # the one hook, whatever k
    s120, i120 = eb.search(q, 120)
    assert torch.equal(i[:, :120], i120) and torch.equal(s[:, :120], s120)


def test_limits_of_every_call() -> None:
    assert _lib.ISC_TOPK_MAX_K == 120 and _lib.ISC_TOPK_LARGE_MAX_K == 4096
    eb, q = _bank(5000, row_groups=torch.arange(5000) // 2), _rows(3, seed=2)
    for call in (eb.search, eb.search_async, eb.search_exhaustive):
        with pytest.raises(ValueError, match="k must be <= 4096, got 4097"):
            call(q, 4097)
    assert eb.search(q, 4096)[1].shape == (3, 4096)
    with pytest.raises(ValueError, match="exceeds the bank size"):
        _bank(300).search(q, 301)
    with pytest.raises(ValueError, match=r"must be in \[1, 300\]"):
        _bank(300).search_exhaustive(q, 301)
    # the calls without a large-k path keep their limit
    for call in (eb.search_groups, eb.search_groups_exhaustive):
        with pytest.raises(ValueError, match="k must be <= 120, got 121"):
            call(q, 121)
    with pytest.raises(ValueError, match="k must be <= 120, got 121"):
        eb.search_rows([1, 2], 121)
    with pytest.raises(ValueError, match=r"k=120 must be in \[1, 119\]"):
        eb.search_rows([1, 2], 120)  # (one of the 120 is the query's own row)
    with pytest.raises(TypeError):
        eb.search(q, 121.0)
    with pytest.raises(ValueError, match="k must be >= 1"):
        eb.search(q, 0)


def test_a_filtered_answer_shorter_than_k_is_padded() -> None:
    eb, q = _bank(400), _rows(4, seed=3)
    allow = torch.zeros(400, dtype=torch.bool)
    allow[::3] = True  # 134 rows
    s, i = eb.search(q, 200, mask=allow)
    exp_s, exp_i = search_oracle.cosine_topk(eb._bank[allow], q, 134)
    np.testing.assert_array_equal(i[:, :134].numpy(), np.nonzero(allow.numpy())[0][exp_i])
    np.testing.assert_array_equal(s[:, :134].numpy(), exp_s)
    assert (i[:, 134:] == -1).all() and torch.isneginf(s[:, 134:]).all()
    # removed rows and spare capacity go through the same filter
    eb = _bank(400, capacity=450)
    eb.remove(rows=torch.arange(0, 400, 2))
    s, i = eb.search(q, 300)
    assert (i[:, :200] % 2 == 1).all() and (i[:, 200:] == -1).all() and torch.isneginf(s[:, 200:]).all()


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank: int, world: int, port: int) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        class OracleBank(EmbeddingBank):
            def _store(self, embeddings, normalize):
                return embeddings.contiguous()

            def _local_topk(self, queries, kk, out=None, lane=-1, stream=None):
                s, i = search_oracle.cosine_topk(self._bank, queries, kk, index_base=self.index_base)
                out[0].copy_(torch.from_numpy(s)), out[1].copy_(torch.from_numpy(i)), out[2].zero_()
                return out[0], out[1]

            def _merge_topk(self, scores, indices, kk):
                s, i = search_oracle.topk_merge(scores.numpy(), indices.numpy(), kk)
                return torch.from_numpy(s), torch.from_numpy(i)

        rows, q = _rows(600), _rows(3, seed=4)
        eb = OracleBank(rows, dtype=torch.float32, normalize=False, process_group=dist.group.WORLD)
        for call in (eb.search, eb.search_async):
            with pytest.raises(ValueError, match="a sharded bank searches k <= 120, got 121"):
                call(q, 121)
        s, i = eb.search(q, 120)  # the limit itself is served, and the ranks are still in step
        exp_s, exp_i = search_oracle.cosine_topk(rows, q, 120)
        np.testing.assert_array_equal(i.numpy(), exp_i)
        np.testing.assert_array_equal(s.numpy(), exp_s)
    finally:
        dist.destroy_process_group()


def test_a_sharded_bank_refuses_k_beyond_120() -> None:
    mp.spawn(_worker, args=(2, _free_port()), nprocs=2, join=True)
