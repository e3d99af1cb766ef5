"""The int8 level of large-batch fp16 searches (isc_bank_quantize, isc_cosine_topk_shadow).

Yardstick: BIT IDENTITY with the fp16 path -- the same bank searched with `shadow=False` returns `torch.equal` scores
and indices.  The int8 level exists only in plans with a level between the sample and the last one at more than 256
queries: 32 768 x 171 = 5 603 328 rows at Q <= 512, 16 384 x 129 = 2 113 536 at Q > 512 (make_plan), so the banks here have
6 000 123 rows of 64 or 100 dimensions (a ragged last tile; D = 100 has a zero-padded K step), and 2 200 003 rows at D = 768.
Every bank is built once per module, on the device.  The bank variants are also compared with the exhaustive float64
search, on the first 16 queries (the exhaustive kernel evaluates every score of every query in float64)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 6_000_123
K = 10


def _rows(n: int, d: int, device: torch.device, seed: int) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, d, device=device, dtype=torch.float16, generator=g)
    return torch.nn.functional.normalize(x.float(), dim=1).half()


def _queries(q: int, d: int, device: torch.device, seed: int, dtype=torch.float16) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(q, d, device=device, dtype=torch.float32, generator=g).to(dtype)


def _same(a: tuple[torch.Tensor, torch.Tensor], b: tuple[torch.Tensor, torch.Tensor]) -> None:
    assert torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy(), equal_nan=True)


def _both(bank, queries: torch.Tensor, k: int = K):
    """(with the int8 level, without) on the same bank object; the first must really have used the shadow."""
    bank.shadow = True
    got = bank.search(queries, k)
    assert bank._shadow is not None, "the plan did not qualify for the int8 level"
    bank.shadow = False
    ref = bank.search(queries, k)
    bank.shadow = True
    return got, ref


@pytest.fixture(scope="module")
def rows64(device: torch.device) -> torch.Tensor:
    return _rows(N, 64, device, 1)


@pytest.fixture(scope="module")
def bank64(rows64: torch.Tensor):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows64, dtype=torch.float16, normalize=False)


@pytest.mark.parametrize("q", [257, 512, 1000, 1024, 1025])
def test_query_counts(q: int, bank64, device: torch.device) -> None:
    got, ref = _both(bank64, _queries(q, 64, device, q))
    _same(got, ref)
    assert int(bank64.last_status[3]) == 0


def test_fp32_queries_and_degenerate_queries(bank64, device: torch.device) -> None:
    queries = _queries(512, 64, device, 7, torch.float32)
    queries[3] = 0
    queries[5, 2] = float("nan")
    queries[9, 60] = float("inf")
    queries[11] = 1e6  # overflows fp16 when it is rounded to the bank type
    queries[13] *= 1e-3
    queries[15] *= 1e3
    got, ref = _both(bank64, queries)
    _same(got, ref)


def test_dim_100_has_a_zero_padded_k_step(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    bank = EmbeddingBank(_rows(N, 100, device, 2), dtype=torch.float16, normalize=False)
    _same(*_both(bank, _queries(512, 100, device, 3)))


def test_dim_768(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    bank = EmbeddingBank(_rows(2_200_003, 768, device, 4), dtype=torch.float16, normalize=False)
    _same(*_both(bank, _queries(1000, 768, device, 5)))


def test_index_base(rows64: torch.Tensor, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    bank = EmbeddingBank(rows64, dtype=torch.float16, normalize=False, presharded=True, index_base=1000)
    got, ref = _both(bank, _queries(300, 64, device, 11))
    _same(got, ref)
    assert int(got[1].min()) >= 1000


def _variant(rows: torch.Tensor, which: str) -> torch.Tensor:
    x = rows.clone()
    n = x.shape[0]
    g = torch.Generator(device=x.device).manual_seed(5)
    if which == "mixed_norms":  # row norms from 1e-3 to 1e3, mixed inside every tile
        e = torch.rand(n, 1, device=x.device, generator=g) * 6 - 3
        x = (x.float() * torch.pow(10.0, e)).half()
    elif which == "zero_rows":
        x[::997] = 0
    elif which == "duplicates":
        for r in range(0, n - 16, 50_021):
            x[r + 1 : r + 9] = x[r]
    elif which == "non_finite":
        x[12_345, 3] = float("inf")
        x[777_777] = float("nan")
        x[5_900_000, 63] = float("-inf")
    return x


@pytest.mark.parametrize("which", ["mixed_norms", "zero_rows", "duplicates", "non_finite"])
def test_bank_variants(which: str, rows64: torch.Tensor, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    bank = EmbeddingBank(_variant(rows64, which), dtype=torch.float16, normalize=False)
    queries = _queries(300, 64, device, 17)
    if which == "duplicates":
        queries[:8] = rows64[50_021 * torch.arange(8, device=device)].float().half()  # queries AT duplicated rows
    got, ref = _both(bank, queries)
    _same(got, ref)
    _same((got[0][:16], got[1][:16]), bank.search_exhaustive(queries[:16], K))


def test_append_drops_the_shadow(device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    rows = _rows(N, 64, device, 21)
    extra = _rows(1000, 64, device, 22)
    queries = _queries(300, 64, device, 23)
    bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
    bank.search(queries, K)
    assert bank._shadow is not None
    bank.append(extra, normalize=False)
    assert bank._shadow is None
    whole = EmbeddingBank(torch.cat([rows, extra]), dtype=torch.float16, normalize=False, shadow=False)
    _same(bank.search(queries, K), whole.search(queries, K))
    _same(_both(whole, queries)[0], bank.search(queries, K))


def test_capture_takes_the_fp16_path(bank64, device: torch.device) -> None:
    queries = _queries(512, 64, device, 31)
    eager = bank64.search(queries, K)  # warm-up: the shadow and the workspace exist
    assert bank64._shadow is not None
    seen = []
    real = bank64._row_search
    bank64._row_search = lambda base, *a, **kw: (seen.append(base), real(base, *a, **kw))[1]
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = bank64.search(queries, K, check=False)
    finally:
        del bank64._row_search
    assert seen == ["isc_cosine_topk"]
    out[0].zero_(), out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(out, eager)


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    device = torch.device("cuda", 0)  # both ranks share the device; the exchange goes through gloo
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from imagescry_amd import EmbeddingBank

        rows = _rows(2 * N, 64, device, 41)  # each shard has a level between the sample and the last one
        queries = _queries(300, 64, device, 42)
        sharded = EmbeddingBank(rows, dtype=torch.float16, normalize=False, process_group=dist.group.WORLD)
        s, i = sharded.search(queries, K)
        used = sharded._shadow is not None
        whole = EmbeddingBank(rows, dtype=torch.float16, normalize=False, shadow=False)
        ws, wi = whole.search(queries, K)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), used=np.array(used), same_i=np.array(torch.equal(i, wi)),
                 same_s=np.array(torch.equal(s, ws)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_the_unsharded_fp16_answer(tmp_path) -> None:
    import torch.multiprocessing as mp

    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        got = np.load(tmp_path / f"rank{rank}.npz")
        assert bool(got["used"]) and bool(got["same_i"]) and bool(got["same_s"])
