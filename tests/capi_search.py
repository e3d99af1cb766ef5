"""ctypes calls of the search and statistics entry points on caller-owned buffers, shared by test_gpu_workspace.py and
test_gpu_graph.py (test infrastructure).  Every call goes to the caller's current stream."""

from __future__ import annotations

import numpy as np
import torch

from imagescry_amd import _lib


def bank(rows: torch.Tensor, device: torch.device, dtype: torch.dtype | None = None, normalize: bool = False):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=dtype or rows.dtype, normalize=normalize)


def _stream(device: torch.device) -> int:
    return _lib.stream_handle(device)


def topk_ws_bytes(eb, nq: int, k: int, exhaustive: bool = False) -> int:
    lib, need = _lib.load(), _lib.c_size_t()
    fn = lib.isc_cosine_topk_exhaustive_workspace_bytes if exhaustive else lib.isc_cosine_topk_workspace_bytes
    _lib.check(fn(_lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, nq, k, need), "workspace_bytes")
    return need.value


def range_ws_bytes(eb, nq: int, capacity: int) -> int:
    lib, need = _lib.load(), _lib.c_size_t()
    _lib.check(lib.isc_cosine_range_workspace_bytes(_lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, nq, capacity,
                                                    need), "isc_cosine_range_workspace_bytes")
    return need.value


def topk(eb, q: torch.Tensor, k: int, out_s, out_i, status, ws: torch.Tensor, mask=None) -> None:
    """isc_cosine_topk (or _masked, `mask` a RowFilter) of `q` into the given tensors."""
    lib = _lib.load()
    args = (eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(),
            _lib.dtype_code(q.dtype), q.shape[0], q.stride(0), k, eb.index_base, eb._norm_bound.data_ptr(),
            out_s.data_ptr(), out_i.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())
    if mask is None:
        _lib.check(lib.isc_cosine_topk(*args, _stream(q.device)), "isc_cosine_topk")
    else:
        _lib.check(lib.isc_cosine_topk_masked(*args, mask.packed.data_ptr(), _stream(q.device)), "isc_cosine_topk_masked")


def exhaustive(eb, q: torch.Tensor, k: int, out_s, out_i, ws: torch.Tensor, mask=None) -> None:
    lib = _lib.load()
    args = (eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(),
            _lib.dtype_code(q.dtype), q.shape[0], q.stride(0), k, eb.index_base, out_s.data_ptr(), out_i.data_ptr(),
            ws.data_ptr(), ws.numel())
    if mask is None:
        _lib.check(lib.isc_cosine_topk_exhaustive(*args, _stream(q.device)), "isc_cosine_topk_exhaustive")
    else:
        _lib.check(lib.isc_cosine_topk_exhaustive_masked(*args, mask.packed.data_ptr(), _stream(q.device)),
                   "isc_cosine_topk_exhaustive_masked")


def cosine_range(eb, q: torch.Tensor, thr: torch.Tensor, capacity: int, offsets, scores, indices, needed, status,
                 ws: torch.Tensor, mask=None) -> None:
    lib = _lib.load()
    args = (eb._bank.data_ptr(), _lib.dtype_code(eb.dtype), eb.num_local_rows, eb.dim, q.data_ptr(),
            _lib.dtype_code(q.dtype), q.shape[0], q.stride(0), thr.data_ptr(), eb.index_base, eb._norm_bound.data_ptr(),
            capacity, offsets.data_ptr(), scores.data_ptr(), indices.data_ptr(), needed.data_ptr(), status.data_ptr(),
            ws.data_ptr(), ws.numel())
    if mask is None:
        _lib.check(lib.isc_cosine_range(*args, _stream(q.device)), "isc_cosine_range")
    else:
        _lib.check(lib.isc_cosine_range_masked(*args, mask.packed.data_ptr(), _stream(q.device)),
                   "isc_cosine_range_masked")


def topk_merge(scores, indices, kout: int, out_s, out_i) -> None:
    g, nq, kin = scores.shape
    _lib.check(_lib.load().isc_topk_merge(scores.data_ptr(), indices.data_ptr(), g, nq, kin, kout, 0, 0, out_s.data_ptr(),
                                          out_i.data_ptr(), _stream(scores.device)), "isc_topk_merge")


# ---- buffers -------------------------------------------------------------------------------------------------------
def fill_bytes(t: torch.Tensor, how: str, seed: int = 0) -> torch.Tensor:
    """Overwrite every byte of `t`: "zero", "ones" (0xFF) or "random" (seeded)."""
    raw = t.view(torch.uint8) if t.dtype != torch.uint8 else t
    if how == "zero":
        raw.zero_()
    elif how == "ones":
        raw.fill_(255)
    else:
        g = torch.Generator(device=t.device).manual_seed(seed)
        raw.copy_(torch.randint(0, 256, raw.shape, dtype=torch.uint8, device=t.device, generator=g))
    return t


def garbage_topk_out(nq: int, k: int, device: torch.device):
    """Outputs of a top-k pre-filled with what the call must overwrite: scores NaN, indices 0x7F.., status 0xFF."""
    s = torch.full((nq, k), float("nan"), dtype=torch.float32, device=device)
    i = torch.full((nq, k), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=device)
    st = torch.full((4,), -1, dtype=torch.int32, device=device)
    return s, i, st


def zero_topk_out(nq: int, k: int, device: torch.device):
    return (torch.zeros((nq, k), dtype=torch.float32, device=device),
            torch.zeros((nq, k), dtype=torch.int64, device=device), torch.zeros(4, dtype=torch.int32, device=device))


def bits(t: torch.Tensor) -> np.ndarray:
    """The raw bits of a tensor (NaN payloads and -0.0 included) as a numpy array."""
    t = t.detach()
    if t.dtype == torch.float32:
        t = t.view(torch.int32)
    elif t.dtype == torch.float64:
        t = t.view(torch.int64)
    return t.cpu().numpy()


def assert_bits_equal(a: torch.Tensor, b: torch.Tensor, what: str = "") -> None:
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def assert_topk_status_equal(got: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """Top-k status words of two runs of the same call.  Without an overflowed candidate list every word is decided by
    the data and must be equal.  Once a list overflows (status[0] > 0) the order of the atomic appends decides which
    workgroups find it full ([0]), which candidates it keeps ([2] is the largest filter error over them) and so the
    threshold of the redo, whose own lists may then overflow or not ([3]).  The answer is exact either way; both runs
    must then agree that an overflow happened and on the queries listed for the redo ([1], decided per query)."""
    g, r = got.cpu().tolist(), ref.cpu().tolist()
    if r[0] == 0:
        assert g == r, (what, g, r)
    else:
        assert g[0] > 0 and g[1] == r[1] and g[3] >= 0, (what, g, r)
