"""The grouped entry points with garbage workspaces and outputs, and a grouped `EmbeddingBank.search` captured into a
graph and replayed with new labels (the conventions of test_gpu_workspace.py / test_gpu_graph.py)."""

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

    bank, noise = cases.search_case(4000, 64, nq, torch.float32, seed=nq)
    labels = torch.arange(4000, dtype=torch.int64) // 49
    src = torch.randint(0, 4000, (nq,), generator=cases.gen(nq))
    q = (bank[src] + 0.3 * torch.nn.functional.normalize(noise, dim=1)).to(device)
    eb = EmbeddingBank(bank.to(device), dtype=dtype, normalize=False, row_groups=labels)
    return eb, q, eb._query_codes(labels[src], nq)


def _topk(eb, q, k, out_s, out_i, status, ws, codes, mask=None) -> None:
    lib = _lib.load()
    st = lib.isc_cosine_topk_grouped(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), k, eb.index_base, eb._norm_bound.data_ptr(), out_s.data_ptr(), out_i.data_ptr(),
        status.data_ptr(), ws.data_ptr(), ws.numel(), None if mask is None else mask.packed.data_ptr(),
        eb._row_codes.data_ptr(), codes.data_ptr(), _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_topk_grouped")


def _exhaustive(eb, q, k, out_s, out_i, ws, codes) -> None:
    lib = _lib.load()
    st = lib.isc_cosine_topk_exhaustive_grouped(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), k, eb.index_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), None,
        eb._row_codes.data_ptr(), codes.data_ptr(), _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_topk_exhaustive_grouped")


def _range(eb, q, thr, capacity, outs, ws, codes) -> None:
    lib = _lib.load()
    offsets, scores, indices, needed, status = outs
    st = lib.isc_cosine_range_grouped(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), thr.data_ptr(), eb.index_base, eb._norm_bound.data_ptr(), capacity, offsets.data_ptr(),
        scores.data_ptr(), indices.data_ptr(), needed.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), None,
        eb._row_codes.data_ptr(), codes.data_ptr(), _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_range_grouped")


@pytest.mark.parametrize("nq", [1, 65, 129, 1100])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_grouped_topk_with_garbage_workspace_and_outputs(nq: int, k: int, device: torch.device) -> None:
    eb, q, codes = _case(device, nq, torch.float16)
    ws = torch.empty(cs.topk_ws_bytes(eb, nq, k), dtype=torch.uint8, device=device)
    ref = cs.zero_topk_out(nq, k, device)
    _topk(eb, q, k, *ref, cs.fill_bytes(ws, "zero"), codes)
    mask = eb.row_filter(torch.rand(4000, generator=cases.gen(3)) < 0.5)
    mref = cs.zero_topk_out(nq, k, device)
    _topk(eb, q, k, *mref, cs.fill_bytes(ws, "zero"), codes, mask)
    for how in ("zero", "ones", "random"):
        out = cs.garbage_topk_out(nq, k, device)
        _topk(eb, q, k, *out, cs.fill_bytes(ws, how, seed=nq + k), codes)
        cs.assert_bits_equal(out[0], ref[0], how)
        cs.assert_bits_equal(out[1], ref[1], how)
        cs.assert_topk_status_equal(out[2], ref[2], how)
        out = cs.garbage_topk_out(nq, k, device)
        _topk(eb, q, k, *out, cs.fill_bytes(ws, how, seed=nq + k + 1), codes, mask)
        cs.assert_bits_equal(out[0], mref[0], how)
        cs.assert_bits_equal(out[1], mref[1], how)
    # the public call gives the same answer (its padding mapped to (-inf, -1))
    s, i = eb.search(q, k, exclude_group=eb.group_labels[codes.long()])
    from imagescry_amd.search import _unpad

    us, ui = _unpad(ref[0], ref[1])
    assert torch.equal(i, ui) and torch.equal(s, us)


@pytest.mark.parametrize("how", ["zero", "ones", "random"])
def test_grouped_exhaustive_and_range_with_garbage(how: str, device: torch.device) -> None:
    nq, k, cap = 70, 10, 40000
    eb, q, codes = _case(device, nq, torch.float32)
    ews = torch.empty(cs.topk_ws_bytes(eb, nq, k, exhaustive=True), dtype=torch.uint8, device=device)
    ref = cs.zero_topk_out(nq, k, device)[:2]
    _exhaustive(eb, q, k, *ref, cs.fill_bytes(ews, "zero"), codes)
    out = cs.garbage_topk_out(nq, k, device)[:2]
    _exhaustive(eb, q, k, *out, cs.fill_bytes(ews, how, seed=4), codes)
    cs.assert_bits_equal(out[0], ref[0], how)
    cs.assert_bits_equal(out[1], ref[1], how)
    thr = torch.full((nq,), 0.3, dtype=torch.float32, device=device)
    rws = torch.empty(cs.range_ws_bytes(eb, nq, cap), dtype=torch.uint8, device=device)

    def outs(fill: str):
        o = (torch.empty(nq + 1, dtype=torch.int64, device=device), torch.empty(cap, dtype=torch.float32, device=device),
             torch.empty(cap, dtype=torch.int64, device=device), torch.empty(1, dtype=torch.int64, device=device),
             torch.empty(4, dtype=torch.int32, device=device))
        for t in o:
            cs.fill_bytes(t, fill, seed=9)
        return o

    r0 = outs("zero")
    _range(eb, q, thr, cap, r0, cs.fill_bytes(rws, "zero"), codes)
    r1 = outs(how)
    _range(eb, q, thr, cap, r1, cs.fill_bytes(rws, how, seed=5), codes)
    m = int(r0[0][-1].item())  # rows of the answer (`needed` may be the filter's larger candidate count)
    assert 0 < m <= int(r0[3].item()) <= cap and int(r1[3].item()) == int(r0[3].item())
    cs.assert_bits_equal(r1[0], r0[0], how)
    cs.assert_bits_equal(r1[1][:m], r0[1][:m], how)
    cs.assert_bits_equal(r1[2][:m], r0[2][:m], how)
    res = eb.search_range(q, 0.3, exclude_group=eb.group_labels[codes.long()])
    assert torch.equal(res.indices, r0[2][:m]) and torch.equal(res.offsets, r0[0])


@pytest.mark.parametrize("nq", [1, 64, 300])
def test_captured_grouped_search_replays_with_new_labels(nq: int, device: torch.device) -> None:
    eb, q, codes = _case(device, nq, torch.float16)
    labels = eb.group_labels[codes.long()].clone()
    static_q, static_lab = q.clone(), labels.clone()
    eb.search(static_q, 10, exclude_group=static_lab)  # warm-up: workspaces and library state outside the capture
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs, gi = eb.search(static_q, 10, exclude_group=static_lab)
    gen = cases.gen(nq + 1)
    for rep in range(4):
        new_lab = labels.roll(rep) if rep < 3 else torch.full_like(labels, -12345)  # last: a label no row carries
        new_q = q + 0.05 * torch.randn(q.shape, generator=gen).to(device)
        static_lab.copy_(new_lab)
        static_q.copy_(new_q)
        graph.replay()
        es, ei = eb.search(new_q, 10, exclude_group=new_lab)
        torch.cuda.synchronize(device)
        assert torch.equal(gi, ei) and torch.equal(gs, es), rep
    us, ui = eb.search(static_q, 10)
    assert torch.equal(gi, ui) and torch.equal(gs, us)
