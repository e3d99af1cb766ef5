"""Every bank operation on wide rows, 2048 <= D <= ISC_SEARCH_MAX_D = 8192 (tests/wide_rows.py has the dimension list and
why each entry is in it): the three instantiations of the float64 sweeps (k_exact, k_exact_collapse, k_lr_sweep), the
filtered search where the guard eps = Dpad 2^-23 ||q|| max||b|| is widest and the redo and the exact pass answer, the range
search, stored-row scores, assignment, group sums, the bank PCA at its own limit of 2048, the workspace formulas and the
int8 shadow at its last admitted D = 1024.

Indices must equal each family's existing float64 oracle.  Scores are held to the derived bound of wide_rows.Reference:
equal to float32 of the exact (math.fsum) quotient, one ulp32 allowed only where that quotient lies within the float64
chain's error of a float32 rounding boundary."""

from __future__ import annotations

import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import assign_oracle  # noqa: E402
import wide_rows as wr  # noqa: E402
from collapse_oracle import collapse_oracle  # noqa: E402
from wide_rows import F16, F32  # noqa: E402

from oracle import search_oracle  # noqa: E402

pytestmark = pytest.mark.gpu


def _bank(rows: torch.Tensor, device: torch.device, **kw):
    from imagescry_amd import EmbeddingBank

    return EmbeddingBank(rows.to(device), dtype=rows.dtype, normalize=False, **kw)


def _ratio(status: torch.Tensor) -> tuple[list[int], float]:
    st = status.cpu().tolist()
    return st, struct.unpack("f", struct.pack("i", st[2]))[0]


def _filter_held(eb, what: str) -> tuple[list[int], float]:
    """After a filtered top-k search: no candidate buffer overflowed, and the largest observed filter error stayed below the
    proven bound eps (status[2]: their ratio as float bits)."""
    st, ratio = _ratio(eb.last_status)
    assert st[0] == 0, (what, st)
    assert 0.0 <= ratio < 1.0, (what, ratio)
    return st, ratio


def _masked_topk(s32: np.ndarray, k: int, allow: np.ndarray):
    """The masked oracle of test_gpu_largek.py on the float32 scores of `search_oracle.exact_scores`: (score desc, row
    asc) over the rows a query may return, short answers padded with (-inf, -1)."""
    allow = np.broadcast_to(allow, s32.shape)
    out_s = np.full((s32.shape[0], k), -np.inf, np.float32)
    out_i = np.full((s32.shape[0], k), -1, np.int64)
    for qi in range(s32.shape[0]):
        sel = np.nonzero(allow[qi])[0]
        order = np.lexsort((sel, -s32[qi, sel].astype(np.float64)))[:k]
        out_s[qi, : order.size] = s32[qi, sel[order]]
        out_i[qi, : order.size] = sel[order]
    return out_s, out_i


def _same_rows(got_i: torch.Tensor, exp_i: np.ndarray, what: str) -> None:
    assert got_i.dtype == torch.int64
    assert torch.equal(got_i.cpu(), torch.from_numpy(np.ascontiguousarray(exp_i))), what


# ---------------------------------------------------------------------------------- search and search_exhaustive
UNIT = [("unit", d, b, q) for d in wr.WIDE_DIMS for (b, q) in wr.DTYPES]
HARD = [(kind, d, b, b) for kind in ("same_sign", "raw") for d in (4096, 8192) for b in (F16, F32)]


def _id(c) -> str:
    return f"{c[0]}-{c[1]}-{wr._name(c[2])}-{wr._name(c[3])}"


@pytest.mark.parametrize("kind,d,bdt,qdt", UNIT + HARD, ids=[_id(c) for c in UNIT + HARD])
def test_search_and_exhaustive(kind: str, d: int, bdt, qdt, device: torch.device) -> None:
    """Every D of the list with both bank and both query dtypes, and the same-sign and unnormalised banks at 4096 and 8192
    (every query of a same-sign bank has float32 ties among its best 121 scores; test_wide_rows_host.py shows that none of
    them is near a rounding boundary, so the oracle's (score desc, row asc) order is still every correct kernel's):
    Q = 1, 65, 130, 300 (every query tile; 1 and 130 from D = 6144 on), k = 1, 10, 120 (k = 120 with the one-query form is
    the largest LDS image of k_exact).  One oracle per case: the answers for fewer queries and smaller k are its prefixes."""
    c = wr.case(kind, d, bdt, qdt)
    eb = _bank(c.stored, device)
    assert torch.equal(eb.bank.cpu(), c.stored)
    ks = (1, 10, 120)
    exp_s, exp_i = search_oracle.cosine_topk(c.stored, c.queries.to(bdt), ks[-1])
    qd = wr.with_ldq(c.queries.to(device), c.ldq_pad)
    counts = tuple(n for n in wr.query_counts(d) if n <= qd.shape[0]) if kind == "unit" else (1, qd.shape[0])
    worst, unproven, tally = 0.0, 0, wr.Tally()
    for nq in counts:
        for k in ks:
            what = f"{c.id} Q={nq} k={k}"
            s, i = eb.search(qd[:nq], k)
            st, ratio = _filter_held(eb, what)
            worst, unproven = max(worst, ratio), max(unproven, st[1])
            _same_rows(i, exp_i[:nq, :k], what + " search")
            c.ref.check(s, i, tally, what=what + " search")
            es, ei = eb.search_exhaustive(qd[:nq], k)
            _same_rows(ei, exp_i[:nq, :k], what + " search_exhaustive")
            c.ref.check(es, ei, tally, what=what + " search_exhaustive")
            assert torch.equal(s.view(torch.int32), es.view(torch.int32)), what
    print(f"WIDE guard {c.id} N={c.n}: max filter error / eps = {worst:.4f}, most unproven queries = {unproven}, "
          f"near-boundary share {tally.share:.4f}")
    tally.assert_cap(c.id)
    if d == wr.MAX_D:  # the case is known to leave the filter: the redo or the exact pass answered some query
        assert unproven >= 1, unproven


# ---------------------------------------------------------------------- masked, group-excluded, collapsed, stored rows
class _Family:
    """One case (D, dtype) with row groups of seven adjacent rows, shared by the tests below."""

    def __init__(self, d: int, dt, n: int, device: torch.device) -> None:
        self.c = c = wr.family_case(d, dt, n)
        self.labels = (torch.randperm(c.n // 7 + 1, generator=wr.gen(d))[torch.arange(c.n) // 7] * 7 - 50).to(torch.int64)
        self.eb = _bank(c.stored, device, row_groups=self.labels.to(device))
        self.qd = wr.with_ldq(c.queries.to(device), c.ldq_pad)
        self.s32 = search_oracle.exact_scores(c.stored, c.queries)
        self.rank = np.argsort(np.argsort(-c.ref.s64, axis=1, kind="stable"), axis=1, kind="stable")  # [Q, N]
        self.allow = (torch.rand(c.n, generator=wr.gen(d + 1)) < 0.3).numpy()  # about 30 % of the rows
        self.own = self.labels[torch.randint(0, c.n, (130,), generator=wr.gen(d + 2))]
        self.own[5] = 10**9  # a label no row carries excludes nothing
        self.not_own = self.labels.numpy()[None, :] != self.own.numpy()[:, None]


@pytest.fixture(scope="module", params=wr.FAMILY, ids=[f"{d}-{wr._name(b)}-{n}" for d, b, n in wr.FAMILY])
def fam(request, device: torch.device):
    """Module scope: the tests that take it run case by case, on one bank and one reference per case."""
    return _Family(*request.param, device)


def _within_best(f: _Family, rows: np.ndarray, what: str) -> None:
    """The selection stays inside each query's best FAMILY_BEST rows, where the host test holds the order well defined."""
    q = np.broadcast_to(np.arange(rows.shape[0])[:, None], rows.shape)
    live = rows >= 0
    assert int(f.rank[q[live], rows[live]].max()) < wr.FAMILY_BEST, what


def _topk_family(f: _Family, allow: np.ndarray, tally: wr.Tally, **kw) -> None:
    for nq, k in ((1, 10), (130, 10), (130, 120)):
        exp_s, exp_i = _masked_topk(f.s32[:nq], k, allow if allow.ndim == 1 else allow[:nq])
        opts = {n: (v[:nq] if n == "exclude_group" else v) for n, v in kw.items()}
        what = f"{f.c.id} N={f.c.n} Q={nq} k={k} {sorted(kw)}"
        _within_best(f, exp_i, what)
        s, i = f.eb.search(f.qd[:nq], k, **opts)
        _filter_held(f.eb, what)
        _same_rows(i, exp_i, what + " search")
        f.c.ref.check(s, i, tally, what=what)
        es, ei = f.eb.search_exhaustive(f.qd[:nq], k, **opts)
        _same_rows(ei, exp_i, what + " search_exhaustive")
        f.c.ref.check(es, ei, tally, what=what)
        assert torch.equal(s.view(torch.int32), es.view(torch.int32)), what  # (-inf padding included)


def test_masked(fam: _Family, device: torch.device) -> None:
    rf = fam.eb.row_filter(torch.from_numpy(fam.allow).to(device))
    tally = wr.Tally()
    _topk_family(fam, fam.allow, tally, mask=rf)
    tally.assert_cap("masked")


def test_group_excluded(fam: _Family, device: torch.device) -> None:
    tally = wr.Tally()
    _topk_family(fam, fam.not_own, tally, exclude_group=fam.own)
    rf = fam.eb.row_filter(torch.from_numpy(fam.allow).to(device))
    _topk_family(fam, fam.not_own & fam.allow[None, :], tally, exclude_group=fam.own, mask=rf)
    tally.assert_cap("group-excluded")


def test_collapsed(fam: _Family, device: torch.device) -> None:
    """search_groups and search_groups_exhaustive against tests/collapse_oracle.py, plain and with both filters."""
    f = fam
    rf = f.eb.row_filter(torch.from_numpy(f.allow).to(device))
    tally = wr.Tally()
    for nq, k, filtered in ((1, 10, False), (130, 10, False), (130, 120 if f.c.n > 900 else 40, False), (130, 10, True)):
        allow = (f.not_own & f.allow[None, :])[:nq] if filtered else None
        kw = {"mask": rf, "exclude_group": f.own[:nq]} if filtered else {}
        es, ei, el = collapse_oracle(f.c.stored, f.c.queries[:nq], k, f.labels.numpy(), allow)
        _within_best(f, ei, f"{f.c.id} collapsed Q={nq} k={k} filtered={filtered}")
        for name in ("search_groups", "search_groups_exhaustive"):
            what = f"{f.c.id} {name} Q={nq} k={k} filtered={filtered}"
            s, i, lab = getattr(f.eb, name)(f.qd[:nq], k, **kw)
            _same_rows(i, ei, what)
            assert np.array_equal(lab.cpu().numpy(), el), what
            f.c.ref.check(s, i, tally, what=what)
            assert np.array_equal(np.isneginf(s.cpu().numpy()), ei < 0), what
            if name == "search_groups":
                assert int(f.eb.last_status[0]) == 0, what
    tally.assert_cap("collapsed")


def test_stored_rows_and_scores(fam: _Family, device: torch.device) -> None:
    """`rows`, `scores` and `search_rows`: `scores` has the bits of `search_exhaustive` and lies inside the reference's
    bound; `search_rows` is the search with the stored rows as queries."""
    f, n = fam, fam.c.n
    pick = wr.score_picks(n)
    tally = wr.Tally()
    assert torch.equal(f.eb.rows(pick.to(device)).cpu(), f.c.stored[pick])
    got = f.eb.scores(f.qd[:65], pick.to(device))
    assert got.shape == (65, 40) and got.dtype == torch.float32
    f.c.ref.check(got, np.broadcast_to(pick.numpy()[None, :], (65, 40)), tally, what=f"{f.c.id} scores")
    tally.assert_cap("scores of the picked rows")
    k = min(120, n)
    es, ei = f.eb.search_exhaustive(f.qd[:65], k)
    again = f.eb.scores(f.qd[:65], ei[0])  # the rows of query 0's answer, for every query
    assert torch.equal(again[0].view(torch.int32), es[0].view(torch.int32))
    full = f.eb.scores(f.qd[:3], torch.arange(n, device=device))
    for qi in range(3):  # every row's score: the exhaustive answer is its top k, bit for bit
        assert torch.equal(full[qi][ei[qi]].view(torch.int32), es[qi].view(torch.int32)), qi
    tally = wr.Tally()
    f.c.ref.check(full, np.broadcast_to(np.arange(n)[None, :], (3, n)), tally, what=f"{f.c.id} scores of every row")
    tally.assert_cap("scores of every row")
    # search_rows: the stored rows are the queries (rounding them to the bank dtype is the identity)
    src = pick[:9]
    ref = wr.Reference(f.c.stored, f.c.stored[src])
    s, i = f.eb.search_rows(src.to(device), 10)
    allow = np.arange(n)[None, :] != src.numpy()[:, None]
    _, exp_i = _masked_topk(search_oracle.exact_scores(f.c.stored, f.c.stored[src]), 10, allow)
    _same_rows(i, exp_i, f"{f.c.id} search_rows")
    tally = wr.Tally()
    ref.check(s, i, tally, what=f"{f.c.id} search_rows")
    tally.assert_cap("search_rows")
    s2, i2 = f.eb.search(f.eb.rows(src.to(device)), 11)
    assert torch.equal(i2[:, 0].cpu(), src)  # (a unit row's best match is itself: no other row is that close)
    assert torch.equal(i, i2[:, 1:]) and torch.equal(s.view(torch.int32), s2[:, 1:].view(torch.int32))


def test_assign_and_group_sums(fam: _Family, device: torch.device) -> None:
    """`assign` and `assign_exhaustive` with 3, 65 and 257 centroids against tests/assign_oracle.py (labels; the scores by
    the reference's bound), and `group_sums` against math.fsum under the bound of any-order float64 summation."""
    f, n = fam, fam.c.n
    cent_all = wr.centroids(f.c.d, f.c.q_dtype)
    ref = wr.Reference(f.c.stored, cent_all)
    tally = wr.Tally()
    for nc in (3, 65, 257):
        cent = cent_all[:nc]
        assert assign_oracle.smallest_gap(f.c.stored, cent) > 4 * float(ref.chain[:nc].max())  # the labels are well defined
        exp_l, _ = assign_oracle.assign(f.c.stored, cent)
        cd = wr.with_ldq(cent.to(device), f.c.ldq_pad)
        for name in ("assign", "assign_exhaustive"):
            labels, scores = getattr(f.eb, name)(cd)
            assert labels.dtype == torch.int32
            np.testing.assert_array_equal(labels.cpu().numpy(), exp_l, err_msg=f"{f.c.id} {name} C={nc}")
            ref.check_pairs(scores.cpu().numpy(), exp_l.astype(np.int64), np.arange(n), tally, f"{f.c.id} {name} C={nc}")
    tally.assert_cap("assign")
    labels = torch.randint(-1, 6, (n,), generator=wr.gen(5))  # five groups and labels outside [0, 5)
    sums, counts = f.eb.group_sums(labels.to(device), 5)
    exp_s, exp_c = assign_oracle.group_sums(f.c.stored, labels.numpy(), 5)
    np.testing.assert_array_equal(counts.cpu().numpy(), exp_c)
    absrows = np.abs(f.c.stored.numpy().astype(np.float64))
    mag = np.stack([absrows[labels.numpy() == g].sum(axis=0) for g in range(5)])
    assert (np.abs(sums.cpu().numpy() - exp_s) <= exp_c[:, None] * 2.0 ** -53 * mag).all()


# ---------------------------------------------------------------------------------------------------------- large k
@pytest.mark.parametrize("d,dt", wr.LARGE_K, ids=[f"{d}-{wr._name(b)}" for d, b in wr.LARGE_K])
def test_large_k(d: int, dt, device: torch.device) -> None:
    """k = 121 and 1000 of N = 1200 (k_lr_sweep's three forms) with the checks of test_gpu_largek.py: search and
    search_exhaustive equal the oracle, and the status words of the fast path."""
    c = wr.large_k_case(d, dt)
    tally = wr.Tally()
    eb = _bank(c.stored, device)
    qd = wr.with_ldq(c.queries.to(device), 8)
    exp_s, exp_i = search_oracle.cosine_topk(c.stored, c.queries, 1000)
    for k in (121, 1000):
        what = f"{c.id} k={k}"
        s, i = eb.search(qd, k)
        st, ratio = _ratio(eb.last_status)
        print(f"WIDE large-k {what}: status {st}, ratio {ratio:.4f}")
        assert st[0] == 0 and st[1] == 0 and 0.0 <= ratio < 1.0, (what, st, ratio)  # served by the fast path
        _same_rows(i, exp_i[:, :k], what + " search")
        c.ref.check(s, i, tally, what=what)
        es, ei = eb.search_exhaustive(qd, k)
        _same_rows(ei, exp_i[:, :k], what + " search_exhaustive")
        assert torch.equal(s.view(torch.int32), es.view(torch.int32)), what
    tally.assert_cap(c.id)


# ------------------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize("nq", [7, 300])
@pytest.mark.parametrize("d,dt,n", wr.RANGE, ids=[f"{d}-{wr._name(b)}-{n}" for d, b, n in wr.RANGE])
def test_range(d: int, dt, n: int, nq: int, device: torch.device) -> None:
    """search_range with the oracle's 5th score of each query as its threshold, against the oracle of test_gpu_range.py:
    rows with score >= t in (score desc, row asc) order -- offsets, indices, and the scores by the reference's bound."""
    c = wr.range_case(d, dt, n)
    tally = wr.Tally()
    eb = _bank(c.stored, device)
    s32 = search_oracle.exact_scores(c.stored, c.queries[:nq])
    thr = np.sort(s32, axis=1)[:, n - 5].astype(np.float32)
    offs, ix, qi = [0], [], []
    for q in range(nq):
        sel = np.nonzero(s32[q] >= thr[q])[0]
        ix.append(sel[np.lexsort((sel, -s32[q, sel].astype(np.float64)))].astype(np.int64))
        qi.append(np.full(sel.size, q))
        offs.append(offs[-1] + sel.size)
    ix, qi = np.concatenate(ix), np.concatenate(qi)
    assert offs[-1] == 5 * nq  # (no ties at the 5th score)
    res = eb.search_range(wr.with_ldq(c.queries[:nq].to(device), c.ldq_pad), torch.from_numpy(thr).to(device))
    np.testing.assert_array_equal(res.offsets.cpu().numpy(), np.array(offs, np.int64))
    np.testing.assert_array_equal(res.indices.cpu().numpy(), ix)
    c.ref.check_pairs(res.scores.cpu().numpy(), qi, ix, tally, f"{c.id} N={n} Q={nq} range")
    tally.assert_cap(f"{c.id} N={n} Q={nq} range")
    st, ratio = _ratio(eb.last_range_status)
    assert 0.0 <= ratio < 1.0, (st, ratio)


# --------------------------------------------------------------------------------------------------------- bank PCA
def _gram(eb, mean: torch.Tensor):
    """isc_bank_gram of every row through the bank's device hook: (float64 [D, D] on the host, the row count)."""
    gram = torch.zeros((eb.dim, eb.dim), dtype=torch.float64, device=eb.device)
    count = torch.zeros(1, dtype=torch.int64, device=eb.device)
    eb._gram_rows(mean.to(eb.device), None, gram, count)
    return gram.cpu(), int(count)


def _project(eb, mean: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """isc_bank_project into a [N, K] view inside a sentinel-filled buffer, after checking that nothing around it was
    written."""
    k, n = w.shape[1], eb.capacity
    buf = torch.full((n + 2, k + 3), 12345.0, dtype=F32, device=eb.device)
    view = buf[1 : n + 1, 1 : k + 1]
    eb._project_rows(mean.to(eb.device), w.to(eb.device).contiguous(), None, view, None)
    out = view.cpu().clone()
    host = buf.cpu()
    host[1 : n + 1, 1 : k + 1] = 12345.0
    assert bool((host == 12345.0).all()), "written outside [N, K]"
    return out


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("d", [2040, 2048])
def test_bank_pca_at_its_limit(d: int, dt, device: torch.device) -> None:
    """isc_bank_gram and isc_bank_project at D = 2048 (their limit) and 2040 (a ragged last K step in both dtypes), with the
    references and bounds of test_gpu_bank_pca.py (tests/matmul_bound.py).  Exact integers: rows [c + R; c - R], shuffled,
    so the mean is c and every centred value and partial sum is a small integer: the kernel must EQUAL the float64 product.
    Real rows (randn + 3: a mean as large as the spread) under the derived product bound."""
    import matmul_bound as mb

    n, g = 258, wr.gen(1000 * 258 + d)
    c = mb.int_tensor((d,), -8, 8, g)
    r = mb.int_tensor((n // 2, d), -4, 4, g)
    x = torch.cat([c + r, c - r])[torch.randperm(n, generator=g)]
    eb = _bank(x.to(dt), device)
    a = x - c
    at = a.T.contiguous()
    mb.assert_exact_range(at, at)
    got, count = _gram(eb, c)
    assert count == n
    assert torch.equal(got, mb.product_f64(at, at)) and torch.equal(got, got.T)
    for k in (1, 64, d):
        w = mb.int_tensor((d, k), -3, 3, wr.gen(d + k))
        wt = w.T.contiguous()
        mb.assert_exact_range(a, wt)
        assert torch.equal(_project(eb, c, w).double(), mb.product_f64(a, wt)), k
    x = torch.randn(600, d, generator=wr.gen(7 * 600 + d)) + 3.0
    eb = _bank(x.to(dt), device)
    stored = x.to(dt).float()
    mean = (stored.double().sum(dim=0) / stored.shape[0]).float()
    a = stored - mean  # the centred operand as the kernel forms it: one float32 subtraction
    at = a.T.contiguous()
    got, count = _gram(eb, mean)
    assert count == 600
    ratio = mb.assert_within_bound(got, mb.product_f64(at, at), mb.product_bound(at, at), "centred Gram")
    print(f"WIDE pca {d} {wr._name(dt)}: Gram worst error / bound = {ratio:.3f}")
    for k in (64, d):
        w = torch.randn(d, k, generator=wr.gen(k))
        wt = w.T.contiguous()
        # (long_k: the derivation of the bound holds for any reduction length while (D + 2) 2^-24 <= 1/2; what is only
        # established up to 1024 terms is its sensitivity, and the exact integers above are the sharp check at this D)
        bound = mb.product_bound(a, wt, long_k=True)
        ratio = mb.assert_within_bound(_project(eb, mean, w), mb.product_f64(a, wt), bound, f"projection K={k}")
        print(f"WIDE pca {d} {wr._name(dt)}: projection K={k} worst error / bound = {ratio:.3f}")


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_bank_pca_refuses_one_past_its_limit(dt, device: torch.device) -> None:
    d = 2049
    eb = _bank(wr.rows("unit", 4, d, 1).to(dt), device)
    with pytest.raises(ValueError, match="isc_bank_gram"):
        _gram(eb, torch.zeros(d))
    out = torch.zeros((4, 3), dtype=F32, device=device)
    with pytest.raises(ValueError, match="isc_bank_project"):
        eb._project_rows(torch.zeros(d, device=device), torch.zeros((d, 3), device=device), None, out, None)
    assert not out.any()


# ------------------------------------------------------------------------------------------------------ workspace sizes
CANARY = 0xA5
TAIL = 1 << 16


def _carve(nbytes: int, device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
    """(a buffer of `nbytes` + 64 KiB filled with the canary, its first `nbytes` bytes as the workspace)."""
    big = torch.full((nbytes + TAIL,), CANARY, dtype=torch.uint8, device=device)
    return big, big[:nbytes]


def _in_exact_workspace(name: str, nbytes: int, call, device: torch.device) -> None:
    """`call(ws)` in a workspace of exactly `nbytes`; one byte less is refused, and nothing behind it is written."""
    from imagescry_amd import _lib

    big, ws = _carve(nbytes, device)
    assert call(ws[: nbytes - 1]) == _lib.ISC_ERR_WORKSPACE, f"{name}: {nbytes} bytes are more than the call asks for"
    assert bool((big == CANARY).all()), f"{name}: a refused call wrote"
    assert call(ws) == _lib.ISC_OK, name
    assert bool((big[nbytes:] == CANARY).all()), f"{name}: written past the {nbytes} bytes its workspace_bytes reports"
    assert bool((ws != CANARY).any()), name


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == F32 else t


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_reported_workspace_sizes_suffice_at_the_limit(dt, device: torch.device) -> None:
    """Every family whose *_workspace_bytes takes D, at D = 8192: one C-ABI call with the size reported for ITS OWN
    arguments, the first bytes of a larger buffer whose tail holds a canary.  The call must accept that size and refuse one
    byte less (so the size is the one it carves), leave the tail intact and give the answer of the bank method, which runs
    in a workspace of its own."""
    import capi_search as cs
    from imagescry_amd import _lib

    lib = _lib.load()
    c = wr.case("unit", wr.MAX_D, dt, dt, n=4500)
    n, d, nq = c.n, c.d, c.queries.shape[0]
    eb = _bank(c.stored, device, row_groups=(torch.arange(n) // 7).to(device))
    qd = c.queries.to(device)
    code, stream = _lib.dtype_code(dt), _lib.stream_handle(device)
    need = _lib.c_size_t()

    def reported(fn: str, *args) -> int:
        _lib.check(getattr(lib, fn)(code, n, d, *args, need), fn)
        return need.value

    def head(q: torch.Tensor, k: int, s, i, st, ws) -> tuple:  # the arguments isc_cosine_topk and its kin share
        return (eb._bank.data_ptr(), code, n, d, q.data_ptr(), code, q.shape[0], q.stride(0), k, 0, eb._norm_bound.data_ptr(),
                s.data_ptr(), i.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel())

    # top-k
    for k in (10, 120):
        s, i, st = cs.garbage_topk_out(nq, k, device)
        _in_exact_workspace(f"topk k={k}", reported("isc_cosine_topk_workspace_bytes", nq, k),
                            lambda ws: lib.isc_cosine_topk(*head(qd, k, s, i, st, ws), stream), device)
        es, ei = eb.search(qd, k)
        assert torch.equal(i, ei) and torch.equal(_bits(s), _bits(es)), k
    # exhaustive
    for k in (10, 120):
        s, i, _ = cs.garbage_topk_out(nq, k, device)
        _in_exact_workspace(f"exhaustive k={k}", reported("isc_cosine_topk_exhaustive_workspace_bytes", nq, k),
                            lambda ws: lib.isc_cosine_topk_exhaustive(*head(qd, k, s, i, s, ws)[:10], s.data_ptr(),
                                                                      i.data_ptr(), ws.data_ptr(), ws.numel(), stream), device)
        es, ei = eb.search_exhaustive(qd, k)
        assert torch.equal(i, ei) and torch.equal(_bits(s), _bits(es)), k
    # large k
    for q9, k in ((qd[:9], 1000), (qd[:65], 121)):
        s, i, st = cs.garbage_topk_out(q9.shape[0], k, device)
        _in_exact_workspace(f"large k={k}", reported("isc_cosine_topk_large_workspace_bytes", q9.shape[0], k),
                            lambda ws: lib.isc_cosine_topk_large(*head(q9, k, s, i, st, ws), None, None, None, stream), device)
        es, ei = eb.search(q9, k)
        assert torch.equal(i, ei) and torch.equal(_bits(s), _bits(es)), k
    # collapse
    k, per = 10, max(eb._max_group_rows, 1)
    s, i, st = cs.garbage_topk_out(nq, k, device)
    codes = torch.full((nq, k), -7, dtype=torch.int32, device=device)
    _in_exact_workspace("collapse", reported("isc_cosine_topk_collapse_workspace_bytes", nq, k, per),
                        lambda ws: lib.isc_cosine_topk_collapse(*head(qd, k, s, i, st, ws), None, eb._row_codes.data_ptr(),
                                                                None, per, codes.data_ptr(), stream), device)
    es, ei, el = eb.search_groups(qd, k)
    assert torch.equal(i, ei) and torch.equal(_bits(s), _bits(es)) and torch.equal(codes.long(), el)  # (the labels 0, 1, ... are their own codes)
    # range
    thr = torch.full((nq,), 0.03, dtype=F32, device=device)
    cap = 1 << 16
    offsets = torch.full((nq + 1,), -1, dtype=torch.int64, device=device)
    rs = torch.full((cap,), float("nan"), dtype=F32, device=device)
    ri = torch.full((cap,), -1, dtype=torch.int64, device=device)
    needed = torch.full((1,), -1, dtype=torch.int64, device=device)
    st = torch.full((4,), -1, dtype=torch.int32, device=device)
    _in_exact_workspace("range", cs.range_ws_bytes(eb, nq, cap),
                        lambda ws: lib.isc_cosine_range(*head(qd, 0, s, i, st, ws)[:8], thr.data_ptr(), 0,
                                                        eb._norm_bound.data_ptr(), cap, offsets.data_ptr(), rs.data_ptr(),
                                                        ri.data_ptr(), needed.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), stream), device)
    res = eb.search_range(qd, thr)
    total = int(res.offsets[-1])
    assert 0 < total <= int(needed) <= cap and torch.equal(offsets, res.offsets)  # (needed: the capacity the call asks for)
    assert torch.equal(ri[:total], res.indices) and torch.equal(_bits(rs[:total]), _bits(res.scores))
    # assign
    cent = wr.centroids(d, dt)[:65].to(device)
    labels = torch.full((n,), -7, dtype=torch.int32, device=device)
    scores = torch.full((n,), float("nan"), dtype=F32, device=device)
    _in_exact_workspace("assign", reported("isc_bank_assign_workspace_bytes", 65),
                        lambda ws: lib.isc_bank_assign(eb._bank.data_ptr(), code, n, d, cent.data_ptr(), code, 65,
                                                       cent.stride(0), eb._norm_bound.data_ptr(), None, labels.data_ptr(),
                                                       scores.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                        device)
    el, es = eb.assign(cent)
    assert torch.equal(labels, el) and torch.equal(_bits(scores), _bits(es))
    # farthest points
    rows = torch.full((5,), -7, dtype=torch.int64, device=device)
    cover = torch.full((5,), float("nan"), dtype=F32, device=device)
    _in_exact_workspace("farthest", reported("isc_bank_farthest_workspace_bytes"),
                        lambda ws: lib.isc_bank_farthest(eb._bank.data_ptr(), code, n, d, None, 0, 5, None, None,
                                                         rows.data_ptr(), cover.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                                         stream), device)
    ei, ec = eb.farthest_points(5)
    assert torch.equal(rows, ei) and torch.equal(_bits(cover), _bits(ec))


# ------------------------------------------------------------------------------------------ the int8 shadow at D = 1024
def test_shadow_at_its_last_admitted_dimension(device: torch.device) -> None:
    """2 200 003 fp16 rows of D = 1024, built on the device, Q = 1025: every one of the 128 sixteen-byte chunks k_rescore's
    lanes cover (l and l + 64) is live.  The yardstick of test_gpu_shadow.py: `shadow=True` equals `shadow=False` bit for
    bit and the shadow was really used; the first 16 queries against the float64 sweep.  The one large case of the file."""
    from imagescry_amd import EmbeddingBank

    n, d, nq = 2_200_003, 1024, 1025
    g = torch.Generator(device=device).manual_seed(21)
    rows = torch.empty((n, d), dtype=F16, device=device)
    for r0 in range(0, n, 1 << 18):
        x = torch.randn(min(1 << 18, n - r0), d, device=device, dtype=F32, generator=g)
        rows[r0 : r0 + x.shape[0]] = torch.nn.functional.normalize(x, dim=1).half()
    bank = EmbeddingBank(rows, dtype=F16, normalize=False)
    del rows
    q = torch.randn(nq, d, device=device, dtype=F32, generator=g).half()
    bank.shadow = True
    got = bank.search(q, 10)
    assert bank._shadow is not None, "the plan did not qualify for the int8 level"
    st, ratio = _filter_held(bank, "shadow")
    bank.shadow = False
    ref = bank.search(q, 10)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
    es, ei = bank.search_exhaustive(q[:16], 10)
    assert torch.equal(got[1][:16], ei) and torch.equal(got[0][:16].view(torch.int32), es.view(torch.int32))
