"""The large-k entry points (isc_cosine_topk_large, isc_cosine_topk_exhaustive_large) with garbage workspaces and outputs,
and isc_cosine_topk_large captured into a graph and replayed with new queries (the conventions of test_gpu_workspace.py /
test_gpu_graph.py)."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import capi_search as cs  # noqa: E402
import cases  # noqa: E402

from imagescry_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


def _case(device: torch.device, nq: int, dtype: torch.dtype):
    from imagescry_amd import EmbeddingBank

    bank, noise = cases.search_case(6000, 64, nq, torch.float32, seed=nq)
    src = torch.randint(0, 6000, (nq,), generator=cases.gen(nq))
    q = (bank[src] + 0.3 * torch.nn.functional.normalize(noise, dim=1)).to(device)
    return EmbeddingBank(bank.to(device), dtype=dtype, normalize=False), q


def _ws(eb, nq: int, k: int, exhaustive: bool = False) -> torch.Tensor:
    lib, need = _lib.load(), _lib.c_size_t()
    fn = lib.isc_cosine_topk_exhaustive_large_workspace_bytes if exhaustive else lib.isc_cosine_topk_large_workspace_bytes
    _lib.check(fn(_lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, nq, k, need), "workspace_bytes")
    return torch.empty(need.value, dtype=torch.uint8, device=eb.device)


def _large(eb, q, k, out_s, out_i, status, ws, mask=None) -> None:
    st = _lib.load().isc_cosine_topk_large(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), k, eb.index_base, eb._norm_bound.data_ptr(), out_s.data_ptr(), out_i.data_ptr(),
        status.data_ptr(), ws.data_ptr(), ws.numel(), None if mask is None else mask.packed.data_ptr(), None, None,
        _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_topk_large")


def _exhaustive(eb, q, k, out_s, out_i, ws, mask=None) -> None:
    st = _lib.load().isc_cosine_topk_exhaustive_large(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), k, eb.index_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
        None if mask is None else mask.packed.data_ptr(), None, None, _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_topk_exhaustive_large")


@pytest.mark.parametrize("nq,k", [(1, 121), (65, 500), (1100, 200), (70, 4096)])
def test_large_topk_with_garbage_workspace_and_outputs(nq: int, k: int, device: torch.device) -> None:
    eb, q = _case(device, nq, torch.float16)
    ws, ews = _ws(eb, nq, k), _ws(eb, nq, k, exhaustive=True)
    mask = eb.row_filter(torch.rand(6000, generator=cases.gen(3)) < 0.5)
    ref, mref = cs.zero_topk_out(nq, k, device), cs.zero_topk_out(nq, k, device)
    _large(eb, q, k, *ref, cs.fill_bytes(ws, "zero"))
    _large(eb, q, k, *mref, cs.fill_bytes(ws, "zero"), mask)
    assert ref[2].cpu().tolist()[:2] == [0, 0] and nq * k <= ref[2].cpu().tolist()[3] <= nq * (2 * k + 512)
    for how in ("ones", "random"):
        out = cs.garbage_topk_out(nq, k, device)
        _large(eb, q, k, *out, cs.fill_bytes(ws, how, seed=nq + k))
        cs.assert_bits_equal(out[0], ref[0], how)
        cs.assert_bits_equal(out[1], ref[1], how)
        assert out[2].cpu().tolist() == ref[2].cpu().tolist()
        out = cs.garbage_topk_out(nq, k, device)
        _large(eb, q, k, *out, cs.fill_bytes(ws, how, seed=nq + k + 1), mask)
        cs.assert_bits_equal(out[0], mref[0], how)
        cs.assert_bits_equal(out[1], mref[1], how)
        out = cs.garbage_topk_out(nq, k, device)[:2]
        _exhaustive(eb, q, k, *out, cs.fill_bytes(ews, how, seed=nq + k + 2))
        cs.assert_bits_equal(out[0], ref[0], how)
        cs.assert_bits_equal(out[1], ref[1], how)
        out = cs.garbage_topk_out(nq, k, device)[:2]
        _exhaustive(eb, q, k, *out, cs.fill_bytes(ews, how, seed=nq + k + 3), mask)
        cs.assert_bits_equal(out[0], mref[0], how)
        cs.assert_bits_equal(out[1], mref[1], how)
    s, i = eb.search(q, k)  # the public call gives the same answer
    assert torch.equal(i, ref[1]) and torch.equal(s, ref[0])


@pytest.mark.parametrize("nq,k", [(1, 121), (64, 1000), (300, 300)])
def test_captured_large_topk_replays_with_new_queries(nq: int, k: int, device: torch.device) -> None:
    eb, q = _case(device, nq, torch.float16)
    ws = _ws(eb, nq, k)
    static_q = q.clone()
    out = cs.garbage_topk_out(nq, k, device)
    _large(eb, static_q, k, *out, ws)  # warm-up: library state outside the capture
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _large(eb, static_q, k, *out, ws)
    gen = cases.gen(nq + 1)
    for rep in range(3):
        new_q = q + 0.05 * torch.randn(q.shape, generator=gen).to(device)
        if rep == 2:
            new_q[0] = 0.0  # a query for the last resort, whose launches were captured empty
        static_q.copy_(new_q)
        cs.fill_bytes(out[0], "ones"), cs.fill_bytes(out[1], "ones")
        graph.replay()
        es, ei = eb.search_exhaustive(new_q, k)
        torch.cuda.synchronize(device)
        assert torch.equal(out[1], ei) and torch.equal(out[0], es), rep
        assert out[2].cpu().tolist()[:2] == [0, 1 if rep == 2 else 0]
