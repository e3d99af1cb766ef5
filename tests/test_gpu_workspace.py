"""Caller-owned memory holding garbage (include/imagescry_hip.h conventions): the contents of a workspace on entry do not
matter, and every output word a call documents is written.

Every entry point that takes a workspace runs with it filled three ways (0x00, 0xFF, seeded random bytes) and with its
outputs pre-filled with garbage (scores NaN, indices 0x7F.., status / needed / offsets 0xFF).  Results and status words
must be bit-identical to the same call on a freshly zeroed workspace with zeroed outputs -- an output word the call leaves
alone, or a counter it reads before resetting, shows up as a difference -- and the search results must match the
oracles.  A last test runs a sequence of calls on ONE oversized workspace, where each call finds the previous call's
counters at other offsets of its carve."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import capi_search as cs  # noqa: E402
import cases  # noqa: E402

from oracle import search_oracle, transforms_oracle  # noqa: E402
from props import assert_topk_properties  # noqa: E402

pytestmark = pytest.mark.gpu

FILLS = ("zero", "ones", "random")
QS = (1, 64, 100, 300, 1500)  # one 64 tile, the 128 tile, 256 tiles (two), two passes of 1024
KS = (1, 10, 100)
_BANKS: dict = {}


def _rows(kind: str) -> torch.Tensor:
    """float32 rows of a single-level bank below 4096 rows, or of the multi-level bank of test_large_k_on_a_multi_level_bank
    (300 000 x 64, a third of the rows duplicated)."""
    if kind == "single":
        return torch.nn.functional.normalize(torch.randn(3000, 96, generator=cases.gen(5)), dim=1)
    g = torch.Generator().manual_seed(100)
    n = 300_000
    rows = torch.randn(n, 64, generator=g)
    rows[torch.randint(0, n, (n // 3,), generator=g)] = rows[torch.randint(0, n, (n // 3,), generator=g)]
    return torch.nn.functional.normalize(rows, dim=1)


def _bank(kind: str, dtype: torch.dtype, device: torch.device):
    key = (kind, dtype)
    if key not in _BANKS:
        _BANKS.clear()  # one bank at a time on the device
        eb = cs.bank(_rows(kind).to(dtype), device)
        allow = torch.rand(eb.num_local_rows, generator=cases.gen(9)) < 0.5
        _BANKS[key] = (eb, eb.bank.float(), allow, eb.row_filter(allow.to(device)))
    return _BANKS[key]


def _queries(nq: int, d: int, dtype: torch.dtype, device: torch.device, seed: int) -> torch.Tensor:
    q = torch.randn(nq, d, generator=cases.gen(seed))
    if nq > 3:
        q[nq // 2] = 0  # a zero query: every score ties
    return q.to(dtype).to(device)


def _check_oracle(kind: str, stored: torch.Tensor, allow: torch.Tensor, q: torch.Tensor, k: int, s: torch.Tensor,
                  i: torch.Tensor, masked: bool) -> None:
    """Indices exact and scores to 1e-6 against the float64 C oracle (single-level bank), the size-independent proof of
    props.py (multi-level bank).  Masked: the same over the allowed rows, indices mapped back."""
    qb = q
    rows_idx = torch.nonzero(allow).flatten() if masked else None
    if kind == "single":
        from oracle import c_oracle

        rows = stored.cpu() if not masked else stored.cpu()[rows_idx]
        exp_s, exp_i = c_oracle.cosine_topk(rows.numpy(), qb.cpu().float().numpy(), k)
        if masked:
            exp_i = rows_idx.numpy()[exp_i]
        np.testing.assert_array_equal(i.cpu().numpy(), exp_i)
        np.testing.assert_allclose(s.cpu().numpy(), exp_s, rtol=0, atol=1e-6)
        return
    if not masked:
        assert_topk_properties(stored, qb.float(), s, i, k)
        return
    ridx = rows_idx.to(stored.device)
    local = torch.searchsorted(ridx, i)
    assert bool((ridx[local] == i).all())
    assert_topk_properties(stored[ridx], qb.float(), s, local, k)


def _stored(eb, stored: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The queries as the kernels see them: rounded to the bank dtype."""
    return q.to(eb.dtype).float()


@pytest.mark.parametrize("kind", ["single", "multi"])
@pytest.mark.parametrize("bank_dtype,q_dtype", [(torch.float16, torch.float16), (torch.float16, torch.float32),
                                                (torch.float32, torch.float32), (torch.float32, torch.float16)])
def test_topk_ignores_workspace_contents(kind: str, bank_dtype: torch.dtype, q_dtype: torch.dtype,
                                         device: torch.device) -> None:
    """isc_cosine_topk and isc_cosine_topk_masked at every query tiling and k in {1, 10, 100}."""
    eb, stored, allow, rf = _bank(kind, bank_dtype, device)
    for nq in QS:
        q = _queries(nq, eb.dim, q_dtype, device, seed=nq)
        for k in KS:
            for mask in (None, rf):
                # masked calls at one query dtype per bank dtype: the filter does not depend on it
                if mask is not None and q_dtype != bank_dtype:
                    continue
                ws_bytes = cs.topk_ws_bytes(eb, nq, k)
                ref = cs.zero_topk_out(nq, k, device)
                cs.topk(eb, q, k, *ref, torch.zeros(ws_bytes, dtype=torch.uint8, device=device), mask=mask)
                what = f"{kind} {bank_dtype} q {q_dtype} Q={nq} k={k} masked={mask is not None}"
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
                for fill in FILLS:
                    cs.fill_bytes(ws, fill, seed=nq * 1000 + k)
                    got = cs.garbage_topk_out(nq, k, device)
                    cs.topk(eb, q, k, *got, ws, mask=mask)
                    cs.assert_bits_equal(got[0], ref[0], what + f" scores {fill}")
                    cs.assert_bits_equal(got[1], ref[1], what + f" indices {fill}")
                    cs.assert_topk_status_equal(got[2], ref[2], what + f" {fill}")
                _check_oracle(kind, stored, allow, _stored(eb, stored, q), k, ref[0], ref[1], mask is not None)


@pytest.mark.parametrize("kind", ["single", "multi"])
@pytest.mark.parametrize("bank_dtype,q_dtype", [(torch.float16, torch.float32), (torch.float32, torch.float16)])
def test_exhaustive_ignores_workspace_contents(kind: str, bank_dtype: torch.dtype, q_dtype: torch.dtype,
                                               device: torch.device) -> None:
    """isc_cosine_topk_exhaustive and its _masked form: the partial lists and the arrival counter of k_exact live in
    the workspace."""
    eb, stored, allow, rf = _bank(kind, bank_dtype, device)
    for nq in (1, 100, 1500):
        q = _queries(nq, eb.dim, q_dtype, device, seed=nq + 7)
        for k in KS:
            for mask in (None, rf):
                ws_bytes = cs.topk_ws_bytes(eb, nq, k, exhaustive=True)
                rs, ri, _ = cs.zero_topk_out(nq, k, device)
                cs.exhaustive(eb, q, k, rs, ri, torch.zeros(ws_bytes, dtype=torch.uint8, device=device), mask=mask)
                what = f"{kind} {bank_dtype} Q={nq} k={k} masked={mask is not None}"
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
                for fill in FILLS:
                    cs.fill_bytes(ws, fill, seed=nq + k)
                    gs, gi, _ = cs.garbage_topk_out(nq, k, device)
                    cs.exhaustive(eb, q, k, gs, gi, ws, mask=mask)
                    cs.assert_bits_equal(gs, rs, what + f" scores {fill}")
                    cs.assert_bits_equal(gi, ri, what + f" indices {fill}")
                _check_oracle(kind, stored, allow, _stored(eb, stored, q), k, rs, ri, mask is not None)


def _range_out(nq: int, capacity: int, device: torch.device, garbage: bool):
    if garbage:
        return (torch.full((nq + 1,), -1, dtype=torch.int64, device=device),
                torch.full((capacity,), float("nan"), device=device),
                torch.full((capacity,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=device),
                torch.full((1,), -1, dtype=torch.int64, device=device), torch.full((4,), -1, dtype=torch.int32, device=device))
    return (torch.zeros(nq + 1, dtype=torch.int64, device=device), torch.zeros(capacity, device=device),
            torch.zeros(capacity, dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int64, device=device),
            torch.zeros(4, dtype=torch.int32, device=device))


def _assert_range_equal(got, ref, what: str) -> None:
    """offsets, needed and status bit for bit; the rows only when the call fitted (offsets[Q] of them: the rest of the
    buffers is not part of the result)."""
    offs, s, i, needed, status = got
    cs.assert_bits_equal(offs, ref[0], what + " offsets")
    cs.assert_bits_equal(needed, ref[3], what + " needed")
    cs.assert_bits_equal(status, ref[4], what + " status")
    total = int(ref[0][-1])
    cs.assert_bits_equal(s[:total], ref[1][:total], what + " scores")
    cs.assert_bits_equal(i[:total], ref[2][:total], what + " indices")


def _range_oracle(stored: torch.Tensor, q: torch.Tensor, thr: torch.Tensor, allow: np.ndarray):
    s = search_oracle.exact_scores(stored.cpu(), q.cpu())
    t = thr.cpu().numpy()
    offs, sc, ix = [0], [], []
    for qi in range(s.shape[0]):
        sel = np.nonzero((s[qi] >= t[qi]) & allow)[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))
        sc.append(s[qi, sel[order]])
        ix.append(sel[order].astype(np.int64))
        offs.append(offs[-1] + sel.size)
    return np.array(offs, np.int64), np.concatenate(sc).astype(np.float32), np.concatenate(ix)


@pytest.mark.parametrize("kind", ["single", "multi"])
@pytest.mark.parametrize("bank_dtype,q_dtype", [(torch.float16, torch.float32), (torch.float32, torch.float16)])
def test_range_ignores_workspace_contents(kind: str, bank_dtype: torch.dtype, q_dtype: torch.dtype,
                                          device: torch.device) -> None:
    """isc_cosine_range and its _masked form, thresholds at each query's 10th score (plus one query whose threshold admits
    every row): counters, candidate buffers, keys and the sort's temporary storage all live in the workspace.  Each call
    once with a capacity that fits and once with one that does not (needed > capacity: offsets all 0)."""
    eb, stored, allow, rf = _bank(kind, bank_dtype, device)
    for nq in QS:
        q = _queries(nq, eb.dim, q_dtype, device, seed=nq + 11)
        s10, _ = eb.search(q, 10)
        thr = s10[:, -1].contiguous()
        if kind == "single":
            thr[0] = -2.0  # every row of the bank
        for mask in (None, rf):
            probe = _range_out(nq, 1, device, garbage=False)
            cs.cosine_range(eb, q, thr, 1, *probe, torch.zeros(cs.range_ws_bytes(eb, nq, 1), dtype=torch.uint8,
                                                                device=device), mask=mask)
            fit = int(probe[3])
            assert fit > 1
            for capacity in (fit, fit // 2):
                ws_bytes = cs.range_ws_bytes(eb, nq, capacity)
                ref = _range_out(nq, capacity, device, garbage=False)
                cs.cosine_range(eb, q, thr, capacity, *ref, torch.zeros(ws_bytes, dtype=torch.uint8, device=device),
                                mask=mask)
                assert int(ref[3]) == fit
                what = f"{kind} {bank_dtype} Q={nq} cap={capacity} masked={mask is not None}"
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
                for fill in FILLS:
                    cs.fill_bytes(ws, fill, seed=nq + capacity)
                    got = _range_out(nq, capacity, device, garbage=True)
                    cs.cosine_range(eb, q, thr, capacity, *got, ws, mask=mask)
                    _assert_range_equal(got, ref, what + f" {fill}")
                if capacity < fit:
                    assert not bool(ref[0].any())  # overflowed: nothing usable
                    continue
                offs = ref[0].cpu().numpy()
                if kind == "single":
                    exp = _range_oracle(stored, _stored(eb, stored, q), thr, allow.numpy() if mask is not None
                                        else np.ones(eb.num_local_rows, bool))
                    np.testing.assert_array_equal(offs, exp[0])
                    np.testing.assert_array_equal(ref[2][: offs[-1]].cpu().numpy(), exp[2])
                    np.testing.assert_array_equal(ref[1][: offs[-1]].cpu().numpy(), exp[1])
                elif mask is None:  # the first 10 rows of every query are its top-10, bit for bit
                    i10 = eb.search(q, 10)[1]
                    for qi in range(0, nq, max(1, nq // 16)):
                        a = int(offs[qi])
                        assert int(offs[qi + 1]) - a >= 10
                        assert torch.equal(ref[2][a : a + 10], i10[qi]), (what, qi)


@pytest.mark.parametrize("dtype,shape", [(torch.uint8, (3, 3, 200, 300)), (torch.uint8, (2, 3, 17, 31)),
                                         (torch.float32, (2, 3, 150, 150)), (torch.float32, (1, 4, 5, 7))])
def test_channel_stats_ignore_workspace_contents(dtype: torch.dtype, shape: tuple, device: torch.device) -> None:
    """isc_channel_stats: its partial sums are overwrite-only."""
    from imagescry_amd import _lib

    if dtype == torch.uint8:
        x = cases.images_u8(shape, seed=3)
    else:
        x = torch.randn(shape, generator=cases.gen(3)) * 40 + 100
    xd = x.to(device)
    lib = _lib.load()
    code = _lib.dtype_code(dtype)
    need = _lib.c_size_t()
    _lib.check(lib.isc_channel_stats_workspace_bytes(code, *shape, need), "ws")
    c = shape[1]

    def run(ws: torch.Tensor, garbage: bool) -> torch.Tensor:
        out = torch.full((2, c), float("nan") if garbage else 0.0, device=device)
        _lib.check(lib.isc_channel_stats(xd.data_ptr(), code, *shape, out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(),
                                         ws.numel(), _lib.stream_handle(device)), "isc_channel_stats")
        return out

    ref = run(torch.zeros(need.value, dtype=torch.uint8, device=device), False)
    ws = torch.empty(need.value, dtype=torch.uint8, device=device)
    for fill in FILLS:
        cs.fill_bytes(ws, fill, seed=7)
        cs.assert_bits_equal(run(ws, True), ref, fill)
    m64, s64 = transforms_oracle.channel_stats_f64(x)
    np.testing.assert_allclose(ref[0].cpu().numpy(), m64.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(ref[1].cpu().numpy(), s64.numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("n,f,ldx", [(5000, 96, 96), (1024, 8, 8), (3001, 40, 64)])
def test_feature_sums_ignore_workspace_contents(n: int, f: int, ldx: int, device: torch.device) -> None:
    """isc_feature_sums: its per-block partials are overwrite-only."""
    from imagescry_amd import _lib

    x = torch.randn(n, ldx, generator=cases.gen(n)).to(device)
    lib = _lib.load()
    need = _lib.c_size_t()
    _lib.check(lib.isc_feature_sums_workspace_bytes(n, f, need), "ws")

    def run(ws: torch.Tensor, garbage: bool) -> torch.Tensor:
        out = torch.full((f,), float("nan") if garbage else 0.0, dtype=torch.float64, device=device)
        _lib.check(lib.isc_feature_sums(x.data_ptr(), n, f, ldx, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _lib.stream_handle(device)), "isc_feature_sums")
        return out

    ref = run(torch.zeros(need.value, dtype=torch.uint8, device=device), False)
    ws = torch.empty(need.value, dtype=torch.uint8, device=device)
    for fill in FILLS:
        cs.fill_bytes(ws, fill, seed=n)
        cs.assert_bits_equal(run(ws, True), ref, fill)
    exact = x[:, :f].double().sum(dim=0)
    np.testing.assert_allclose(ref.cpu().numpy(), exact.cpu().numpy(), rtol=1e-12, atol=1e-9)


def test_one_oversized_workspace_across_calls(device: torch.device) -> None:
    """One buffer, sized for the largest call, reused by a sequence of calls whose carves put their counters at different
    offsets -- each call must still equal the same call on a fresh zeroed workspace:
    1. a top-k (256-query tiles, k = 100) whose candidate buffers overflow (status[0] > 0);
    2. a top-k (one 64 tile) whose queries take the redo and the exhaustive sweep (status[1] > 0, status[3] > 0);
    3. a small ordinary top-k;
    4. a range call whose `needed` exceeds its capacity, then one that fits.
    The bank is test_more_ties_than_the_redo_lists_hold's: 20 000 copies of one row among 30 000."""
    _BANKS.clear()
    g = cases.gen(71)
    rows = torch.nn.functional.normalize(torch.randn(30_000, 64, generator=g), dim=1)
    patch = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
    where = torch.randperm(30_000, generator=g)[:20_000]
    rows[where] = patch
    eb = cs.bank(rows.half(), device)
    q1 = torch.randn(300, 64, generator=g)
    q1[::7] = patch * 2.0  # 43 queries whose top-100 lies among 20 000 tied rows
    q1[5] = 0
    q2 = torch.randn(6, 64, generator=g)
    q2[2] = patch * 3.0
    q2[4, 3] = float("nan")
    q3 = torch.randn(5, 64, generator=g)
    q1, q2, q3 = q1.half().to(device), q2.half().to(device), q3.to(device)
    thr = torch.full((6,), 0.3, device=device)

    steps = [("overflow", q1, 100), ("redo", q2, 10), ("small", q3, 10)]
    probe = _range_out(6, 1, device, garbage=False)
    cs.cosine_range(eb, q2, thr, 1, *probe, torch.zeros(cs.range_ws_bytes(eb, 6, 1), dtype=torch.uint8, device=device))
    fit = int(probe[3])
    assert fit > 20_000
    size = max(max(cs.topk_ws_bytes(eb, q.shape[0], k) for _, q, k in steps), cs.range_ws_bytes(eb, 6, fit))
    ws = cs.fill_bytes(torch.empty(size, dtype=torch.uint8, device=device), "random", seed=1)

    seen = {}
    for name, q, k in steps:
        got = cs.garbage_topk_out(q.shape[0], k, device)
        cs.topk(eb, q, k, *got, ws)
        ref = cs.zero_topk_out(q.shape[0], k, device)
        cs.topk(eb, q, k, *ref, torch.zeros(cs.topk_ws_bytes(eb, q.shape[0], k), dtype=torch.uint8, device=device))
        cs.assert_bits_equal(got[0], ref[0], name)
        cs.assert_bits_equal(got[1], ref[1], name)
        cs.assert_topk_status_equal(got[2], ref[2], name)
        seen[name] = ref[2].cpu().tolist()
        if name != "overflow":
            from oracle import c_oracle

            exp_s, exp_i = c_oracle.cosine_topk(rows.half().float().numpy(), q.half().float().cpu().numpy(), k)
            np.testing.assert_array_equal(ref[1].cpu().numpy(), exp_i)
            np.testing.assert_allclose(ref[0].cpu().numpy(), exp_s, rtol=0, atol=1e-6)
    assert seen["overflow"][0] > 0, seen
    assert seen["redo"][1] > 0 and seen["redo"][3] > 0, seen
    # the tied queries of step 1 answer with the 100 lowest indices of the copies
    low = sorted(where.tolist())[:100]
    assert all(r == low for r in ref_overflow_rows(eb, q1, ws, device)), "tied queries"

    for capacity in (fit // 3, fit):
        got = _range_out(6, capacity, device, garbage=True)
        cs.cosine_range(eb, q2, thr, capacity, *got, ws)
        ref = _range_out(6, capacity, device, garbage=False)
        cs.cosine_range(eb, q2, thr, capacity, *ref,
                        torch.zeros(cs.range_ws_bytes(eb, 6, capacity), dtype=torch.uint8, device=device))
        _assert_range_equal(got, ref, f"range cap={capacity}")
        assert int(ref[3]) == fit
    exp = _range_oracle(eb.bank.float(), q2.float(), thr, np.ones(30_000, bool))
    np.testing.assert_array_equal(ref[0].cpu().numpy(), exp[0])
    np.testing.assert_array_equal(ref[2][: exp[0][-1]].cpu().numpy(), exp[2])
    np.testing.assert_array_equal(ref[1][: exp[0][-1]].cpu().numpy(), exp[1])


def ref_overflow_rows(eb, q: torch.Tensor, ws: torch.Tensor, device: torch.device) -> list[list[int]]:
    """Top-100 rows of the tied queries (every 7th) of step 1, from a call on the reused workspace."""
    s, i, st = cs.garbage_topk_out(q.shape[0], 100, device)
    cs.topk(eb, q, 100, s, i, st, ws)
    return i[::7].cpu().tolist()
