"""The collapsed entry points with garbage workspaces and outputs, and `EmbeddingBank.search_groups` captured into a graph
and replayed with new queries (the conventions of test_gpu_workspace.py / test_gpu_graph.py)."""

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


def _ws_bytes(eb, nq, k, exhaustive=False) -> int:
    lib = _lib.load()
    need = _lib.c_size_t()
    code = _lib.dtype_code(eb.dtype)
    if exhaustive:
        st = lib.isc_cosine_topk_exhaustive_collapse_workspace_bytes(code, eb.num_local_rows, eb.dim, nq, k, need)
    else:
        st = lib.isc_cosine_topk_collapse_workspace_bytes(code, eb.num_local_rows, eb.dim, nq, k, eb._max_group_rows, need)
    _lib.check(st, "collapse workspace bytes")
    return need.value


def _collapse(eb, q, k, out_s, out_i, status, out_c, ws, codes=None, mask=None) -> None:
    lib = _lib.load()
    st = lib.isc_cosine_topk_collapse(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), k, eb.index_base, eb._norm_bound.data_ptr(), out_s.data_ptr(), out_i.data_ptr(),
        status.data_ptr(), ws.data_ptr(), ws.numel(), None if mask is None else mask.packed.data_ptr(),
        eb._row_codes.data_ptr(), None if codes is None else codes.data_ptr(), eb._max_group_rows, out_c.data_ptr(),
        _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_topk_collapse")


def _exhaustive(eb, q, k, out_s, out_i, out_c, ws, codes=None) -> None:
    lib = _lib.load()
    st = lib.isc_cosine_topk_exhaustive_collapse(
        eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(), _lib.dtype_code(q.dtype),
        q.shape[0], q.stride(0), k, eb.index_base, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), None,
        eb._row_codes.data_ptr(), None if codes is None else codes.data_ptr(), out_c.data_ptr(),
        _lib.stream_handle(q.device))
    _lib.check(st, "isc_cosine_topk_exhaustive_collapse")


@pytest.mark.parametrize("nq", [1, 65, 129, 1100])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_collapse_with_garbage_workspace_and_outputs(nq: int, k: int, device: torch.device) -> None:
    eb, q, codes = _case(device, nq, torch.float16)
    ws = torch.empty(_ws_bytes(eb, nq, k), dtype=torch.uint8, device=device)
    mask = eb.row_filter(torch.rand(4000, generator=cases.gen(3)) < 0.5)
    for qc, rm in ((None, None), (codes, mask)):
        ref = (*cs.zero_topk_out(nq, k, device), torch.zeros((nq, k), dtype=torch.int32, device=device))
        _collapse(eb, q, k, *ref, cs.fill_bytes(ws, "zero"), qc, rm)
        for how in ("zero", "ones", "random"):
            out = (*cs.garbage_topk_out(nq, k, device), cs.fill_bytes(torch.empty((nq, k), dtype=torch.int32,
                                                                                  device=device), how, seed=2))
            _collapse(eb, q, k, *out, cs.fill_bytes(ws, how, seed=nq + k), qc, rm)
            cs.assert_bits_equal(out[0], ref[0], how)
            cs.assert_bits_equal(out[1], ref[1], how)
            cs.assert_bits_equal(out[3], ref[3], how)
            cs.assert_topk_status_equal(out[2], ref[2], how)
    # the public call gives the same answer (its padding mapped to (-inf, -1, -1))
    from imagescry_amd.search import _unpad_groups

    s, i, lab = eb.search_groups(q, k, mask=mask, exclude_group=eb.group_labels[codes.long()])
    us, ui, ul = _unpad_groups(ref[0], ref[1], eb._labels_of(ref[3]))
    assert torch.equal(i, ui) and torch.equal(s, us) and torch.equal(lab, ul)


@pytest.mark.parametrize("how", ["zero", "ones", "random"])
def test_collapse_exhaustive_with_garbage(how: str, device: torch.device) -> None:
    nq, k = 70, 10
    eb, q, codes = _case(device, nq, torch.float32)
    ews = torch.empty(_ws_bytes(eb, nq, k, exhaustive=True), dtype=torch.uint8, device=device)
    ref = (*cs.zero_topk_out(nq, k, device)[:2], torch.zeros((nq, k), dtype=torch.int32, device=device))
    _exhaustive(eb, q, k, *ref, cs.fill_bytes(ews, "zero"), codes)
    out = (*cs.garbage_topk_out(nq, k, device)[:2], torch.full((nq, k), 77, dtype=torch.int32, device=device))
    _exhaustive(eb, q, k, *out, cs.fill_bytes(ews, how, seed=4), codes)
    for a, b in zip(out, ref):
        cs.assert_bits_equal(a, b, how)
    fast = eb.search_groups(q, k, exclude_group=eb.group_labels[codes.long()])
    assert torch.equal(fast[1], ref[1]) and torch.equal(fast[0], ref[0])


@pytest.mark.parametrize("nq", [1, 64, 300])
def test_captured_collapsed_search_replays_with_new_queries(nq: int, device: torch.device) -> None:
    eb, q, codes = _case(device, nq, torch.float16)
    labels = eb.group_labels[codes.long()].clone()
    static_q, static_lab = q.clone(), labels.clone()
    eb.search_groups(static_q, 10, exclude_group=static_lab)  # warm-up: workspaces and library state outside the capture
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs, gi, gl = eb.search_groups(static_q, 10, exclude_group=static_lab)
    gen = cases.gen(nq + 1)
    for rep in range(4):
        new_lab = labels.roll(rep) if rep < 3 else torch.full_like(labels, -12345)
        new_q = q + 0.05 * torch.randn(q.shape, generator=gen).to(device)
        static_lab.copy_(new_lab)
        static_q.copy_(new_q)
        graph.replay()
        es, ei, el = eb.search_groups(new_q, 10, exclude_group=new_lab)
        torch.cuda.synchronize(device)
        assert torch.equal(gi, ei) and torch.equal(gs, es) and torch.equal(gl, el), rep
