"""Chained int8 levels and the two-stage re-score (cosine_topk.hip: make_plan, k_rescore).

Yardstick, as in tests/test_gpu_shadow.py: BIT IDENTITY with the fp16 path -- the same bank object searched with
`shadow=False` returns `torch.equal` scores and indices.  The banks are small ones with a ragged last tile (D = 100: a
zero-padded K step; D = 768 once), and every test reads the structure it is about from isc_cosine_topk_plan.  The piece
next to the sample runs in fp16 when longer levels follow (the faster form at the headline shape, LABLOG.md), so the banks
of 300 123 and 400 123 rows have ONE int8 level after it, 1 400 123 rows two chained ones (D = 64 and D = 100) and
12 100 123 rows three.  The content cases are also compared with the exhaustive float64 search on the first 16 queries."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 10
N2 = 1_400_123  # the content cases' bank; Q = 1024: sample, an fp16 level to 19 456, int8 levels to 155 648 and to the end


def _rows(n: int, d: int, device: torch.device, seed: int) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, d, device=device, dtype=torch.float16, generator=g)
    return torch.nn.functional.normalize(x.float(), dim=1).half()


def _queries(q: int, d: int, device: torch.device, seed: int, dtype=torch.float16) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(q, d, device=device, dtype=torch.float32, generator=g).to(dtype)


def _kinds(n: int, d: int, q: int, k: int = K) -> list[int]:
    from imagescry_amd import _lib

    nl = ctypes.c_int()
    ends = (ctypes.c_int64 * 16)()
    kinds = (ctypes.c_int * 16)()
    _lib.check(_lib.load().isc_cosine_topk_plan(_lib.ISC_F16, n, d, q, k, 1, 16, nl, ends, kinds), "isc_cosine_topk_plan")
    return list(kinds[: nl.value])


def _same(a, b) -> None:
    assert torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy(), equal_nan=True)


def _both(bank, queries: torch.Tensor, k: int = K, clean: str = "yes"):
    """(with the int8 levels, without) on the same bank object.  clean = "yes": the int8 search overflowed no buffer, redid
    no query and handed none to the exhaustive pass -- a plan that overflows would still answer right and hide its cost;
    "as_fp16": it did so exactly as often as the fp16 search of the same queries (content that makes that one redo)."""
    bank.shadow = True
    got = bank.search(queries, k)
    assert bank._shadow is not None, "the plan holds no int8 level"
    status = bank.last_status.cpu().tolist()
    bank.shadow = False
    ref = bank.search(queries, k)
    ref_status = bank.last_status.cpu().tolist()
    bank.shadow = True
    print("status int8", status, "fp16", ref_status)
    if clean == "yes":
        assert (status[0], status[1], status[3]) == (0, 0, 0), status
    elif clean == "as_fp16":
        assert (status[0], status[1], status[3]) == (ref_status[0], ref_status[1], ref_status[3]), (status, ref_status)
    return got, ref


def _bank(rows: torch.Tensor):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows, dtype=torch.float16, normalize=False)


@pytest.fixture(scope="module")
def rows64(device: torch.device) -> torch.Tensor:
    return _rows(N2, 64, device, 1)


@pytest.fixture(scope="module")
def bank64(rows64: torch.Tensor):
    return _bank(rows64)


@pytest.mark.parametrize("n,d,q,kinds", [
    (300_123, 64, 1024, [0, 1, 2]),
    (400_123, 100, 300, [0, 1, 2]),  # a zero-padded K step; the piece next to the sample has 15 tiles
    (1_400_123, 64, 1024, [0, 1, 2, 2]),  # two chained int8 levels
    (1_400_123, 100, 1024, [0, 1, 2, 2]),  # ... with a zero-padded K step
    (12_100_123, 64, 1024, [0, 1, 2, 2, 2]),  # three
    (300_123, 768, 1000, [0, 1, 2]),
    # barely past the sample: lists of fewer than kp entries.  The carried list is full after the sample's selection, so
    # k_rescore still has kp scores and takes tau' from them; its tau' = tau branch needs a query that carries fewer than
    # kp candidates, which no finite bank of more than kp rows produces -- only the numpy model
    # (tests/test_shadow_two_stage_model.py, carried=False) runs that branch
    (16_684, 64, 1024, [0, 2]),
    (300_123, 160, 1024, [0, 1, 2]),  # three fp16 K steps, one and a half int8 steps: the absent half step reads as zeros
    (140_123, 1024, 1024, [0, 2]),  # the shadow's limit in D: eight int8 K steps
])
def test_chained_int8_levels(n: int, d: int, q: int, kinds: list[int], device: torch.device) -> None:
    assert _kinds(n, d, q) == kinds
    bank = _bank(_rows(n, d, device, n % 1000 + d))
    _same(*_both(bank, _queries(q, d, device, q + d)))


def _variant(rows: torch.Tensor, which: str) -> torch.Tensor:
    x = rows.clone()
    n = x.shape[0]
    g = torch.Generator(device=x.device).manual_seed(5)
    if which == "mixed_norms":  # row norms from 1e-3 to 1e3, mixed inside every tile
        e = torch.rand(n, 1, device=x.device, generator=g) * 6 - 3
        x = (x.float() * torch.pow(10.0, e)).half()
    elif which == "duplicates":  # rows stored nine times
        for r in range(0, n - 16, 5_021):
            x[r + 1 : r + 9] = x[r]
    elif which == "non_finite":
        x[12_345, 3] = float("inf")
        x[77_777] = float("nan")
        x[1_290_000, 63] = float("-inf")
    return x


@pytest.mark.parametrize("which", ["duplicates", "mixed_norms", "non_finite"])
def test_bank_contents(which: str, rows64: torch.Tensor, device: torch.device) -> None:
    assert _kinds(N2, 64, 1024) == [0, 1, 2, 2]
    bank = _bank(_variant(rows64, which))
    queries = _queries(1024, 64, device, 17)
    if which == "duplicates":  # queries AT rows stored nine times: stage A's threshold comes from the copies
        queries[:16] = rows64[5_021 * torch.arange(16, device=device)].float().half()
    got, ref = _both(bank, queries, clean="as_fp16" if which == "duplicates" else "no")
    _same(got, ref)
    _same((got[0][:16], got[1][:16]), bank.search_exhaustive(queries[:16], K))


def test_degenerate_queries(bank64, device: torch.device) -> None:
    queries = _queries(1024, 64, device, 7, torch.float32)
    queries[3] = 0
    queries[5, 2] = float("nan")
    queries[13] *= 1e-3
    queries[15] *= 1e3
    got, ref = _both(bank64, queries, clean="as_fp16")  # (the NaN query is answered by the exhaustive pass)
    _same(got, ref)
    _same((got[0][:16], got[1][:16]), bank64.search_exhaustive(queries[:16], K))


def test_k_58(bank64, device: torch.device) -> None:
    kinds = _kinds(N2, 64, 1024, 58)
    assert kinds == [0, 1, 2, 2, 2, 2]  # kp = 64: a level is once or twice as long as the rows before it
    queries = _queries(1024, 64, device, 58)
    got, ref = _both(bank64, queries, 58)
    _same(got, ref)
    _same((got[0][:16], got[1][:16]), bank64.search_exhaustive(queries[:16], 58))
