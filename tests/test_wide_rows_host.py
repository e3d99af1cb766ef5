"""CPU checks of tests/wide_rows.py: the dimension list against the dispatch rule of the float64 sweeps, and the
conditions the score reference needs from the chosen seeds, for every bank test_gpu_wide_rows.py builds -- at most 1 % of
the scores a test compares lie near a float32 rounding boundary (numpy's float64 matmul stays inside the same chain
bound), and the (score, row) order the oracles sort by is well defined: no two of a query's best k + 1 scores tie on the
random banks, and where float32 ties cannot be avoided (same-sign rows, k = 1000 of 1200) no tied or adjacent score is near
a rounding boundary, so every correct kernel sees the same ties."""

from __future__ import annotations

import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import wide_rows as wr  # noqa: E402
from wide_rows import F16, F32  # noqa: E402

from oracle import search_oracle  # noqa: E402

CSRC = ROOT / "imagescry_amd" / "csrc"


def test_the_k_step_rule_is_the_librarys() -> None:
    text = (CSRC / "bank_layout.h").read_text()
    assert re.search(r"#define ISC_KSTEP_BYTES 128\b", text)
    assert "return (d * esz + ISC_KSTEP_BYTES - 1) / ISC_KSTEP_BYTES;" in text
    assert re.search(r"#define\s+ISC_SEARCH_MAX_D\s+8192\b", (ROOT / "include" / "imagescry_hip.h").read_text())
    assert wr.WIDE_DIMS[-1] == wr.MAX_D


@pytest.mark.parametrize("name", ["launch_exact_t", "launch_exact_collapse_t"])
def test_the_dispatch_thresholds_are_the_librarys(name: str) -> None:
    """launch_exact_t and launch_exact_collapse_t: four queries per sweep at dp <= 3072, two at dp <= 6144, else one."""
    text = (CSRC / "search_exact.hip").read_text()
    body = text[text.index(f"int {name}("):]
    body = body[: body.index("\n}\n")]
    found = re.findall(r"if \(dp <= (\d+)\)\s+return \w+<T, (\d)>", body)
    assert found == [("3072", "4"), ("6144", "2")], found
    assert re.search(r"return \w+<T, 1>\(", body)


def test_the_large_k_sweep_dispatches_alike() -> None:
    text = (CSRC / "search_large.hip").read_text()
    found = re.findall(r"if \(dp <= (\d+)\) return lr_sweeps<T, (\d)>", text)
    assert found == [("3072", "4"), ("6144", "2")], found
    assert re.search(r"return lr_sweeps<T, 1>\(", text)


EXPECT = {  # (D, dtype) -> (dp, queries per sweep)
    (2048, F16): (2048, 4), (2048, F32): (2048, 4),
    (3072, F16): (3072, 4), (3072, F32): (3072, 4),
    (3073, F16): (3136, 2), (3073, F32): (3104, 2),
    (6144, F16): (6144, 2), (6144, F32): (6144, 2),
    (6145, F16): (6208, 1), (6145, F32): (6176, 1),
    (8191, F16): (8192, 1), (8191, F32): (8192, 1),
    (8192, F16): (8192, 1), (8192, F32): (8192, 1),
}


def test_each_dimension_selects_the_form_it_is_listed_for() -> None:
    assert set(EXPECT) == {(d, t) for d in wr.WIDE_DIMS for t in (F16, F32)}
    for (d, t), (dp, gq) in EXPECT.items():
        assert (wr.dpad(d, t), wr.queries_per_sweep(d, t)) == (dp, gq), (d, t)
    for t in (F16, F32):  # every form has a first and a last D in the list
        assert [wr.queries_per_sweep(d, t) for d in wr.WIDE_DIMS] == [4, 4, 2, 2, 1, 1, 1]
    assert wr.ksteps(3073, F16) % 2 == 1 and wr.ksteps(6145, F16) % 2 == 1  # odd K steps for the half-major loop
    assert (8191 * 2) % 16 != 0 and (8191 * 4) % 16 != 0  # a ragged last 16-byte chunk


def test_both_bank_sizes_reach_every_form_with_every_dtype_pair() -> None:
    seen = {(wr.queries_per_sweep(d, b), b, q, 4500 if (i + j) % 2 == 0 else 300)
            for i, d in enumerate(wr.WIDE_DIMS) for j, (b, q) in enumerate(wr.DTYPES)}
    assert len(seen) == 3 * 4 * 2


def test_boundary_distance() -> None:
    one = np.float64(1.0)
    up = np.float64(np.nextafter(np.float32(1.0), np.float32(2.0)))
    mid = (one + up) / 2
    d = wr.boundary_distance(np.array([one, mid, mid - 1e-12, mid + 1e-12]))
    assert d[1] == 0.0 and abs(d[2] - 1e-12) < 1e-15 and abs(d[3] - 1e-12) < 1e-15
    assert d[0] == (one - np.float64(np.nextafter(np.float32(1.0), np.float32(0.0)))) / 2  # the narrower side below 1


SEARCH = [("unit", d, b, q) for d in wr.WIDE_DIMS for (b, q) in wr.DTYPES]
HARD = [(kind, d, b, b) for kind in ("same_sign", "raw") for d in (4096, 8192) for b in (F16, F32)]


def _ids(cases) -> list[str]:
    return ["-".join(wr._name(v) if v in (F16, F32) else str(v) for v in c) for c in cases]


def _rows_of(nq: int, rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    return np.broadcast_to(np.arange(nq)[:, None], (nq, rows.shape[-1])), np.broadcast_to(rows, (nq, rows.shape[-1]))


def _capped(ref: wr.Reference, qi, row, what: str) -> None:
    near, total = ref.near_count(qi, row)
    assert near <= wr.Reference.NEAR_CAP * total, (what, near, total)


def _matmul_within_chain(ref: wr.Reference, k: int, seed: int) -> None:
    """numpy's float64 matmul score is within the chain bound of the exact quotient (a sample: two queries' best k and as
    many pairs spread over the bank), which is what lets `Reference.expect` skip the fsum far from a boundary."""
    top = ref.best(k)
    rng = np.random.default_rng(seed)
    nq, n = ref.s64.shape
    pairs = [(qi, int(r)) for qi in (0, nq - 1) for r in top[qi]]
    pairs += [(int(rng.integers(nq)), int(rng.integers(n))) for _ in range(2 * k)]
    worst = max(abs(ref.s64[qi, r] - ref.want(qi, r)) / ref.chain[qi, r] for qi, r in pairs)
    assert worst <= 1.0, worst


def _tie_free(c, k: int) -> None:
    s, _ = search_oracle.cosine_topk(c.stored, c.queries.to(c.bank_dtype), k + 1)
    assert not (s[:, 1:] == s[:, :-1]).any(), np.nonzero(s[:, 1:] == s[:, :-1])


def search_conditions(c) -> None:
    """The top-k searches of a case: the cap over every query's best k_max, and a well-defined order of its best k_max + 1."""
    ref, k = c.ref, c.k_max
    assert ref.near_share(k) <= wr.Reference.NEAR_CAP
    _matmul_within_chain(ref, k, c.d)
    if c.kind == "same_sign":  # ~120 scores within 2e-3 of each other: float32 ties in every seed
        assert ref.fragile(k) == 0
    else:
        _tie_free(c, k)
    # the oracle's float32 scores are the reference's wherever the reference asserts equality
    s, i = search_oracle.cosine_topk(c.stored, c.queries.to(c.bank_dtype), k + 1)
    exp, near = ref.expect(np.repeat(np.arange(s.shape[0]), k + 1), i.reshape(-1))
    assert ((exp == s.reshape(-1)) | near).all()


@pytest.mark.parametrize("kind,d,bdt,qdt", SEARCH + HARD, ids=_ids(SEARCH + HARD))
def test_the_search_cases_meet_the_reference_conditions(kind: str, d: int, bdt, qdt) -> None:
    search_conditions(wr.case(kind, d, bdt, qdt))


def family_conditions(c) -> None:
    """The banks of the masked, group-excluded, collapsed, stored-row and assign tests.  Their answers are selections from
    a query's best FAMILY_BEST rows (the GPU tests assert that they are), so the order must be well defined there; the cap
    is held for each population those tests compare."""
    ref, n = c.ref, c.n
    search_conditions(c)
    assert ref.fragile(min(wr.FAMILY_BEST, n - 1)) == 0
    nq = ref.s64.shape[0]
    picks = wr.score_picks(n).numpy()
    _capped(ref, *_rows_of(65, picks[None, :]), "scores of the picked rows")
    _capped(ref, *_rows_of(3, np.arange(n)[None, :]), "scores of every row")
    _capped(ref, *_rows_of(nq, ref.best(min(400, n))), "best 400: what the filtered searches select from")
    # the rows as queries (search_rows) and the centroids (assign)
    src = torch.from_numpy(picks[:9])
    rows_ref = wr.Reference(c.stored, c.stored[src])
    assert rows_ref.fragile(12) == 0 and rows_ref.near_share(11) <= wr.Reference.NEAR_CAP
    cent = wr.Reference(c.stored, wr.centroids(c.d, c.q_dtype))
    win = np.argmax(cent.s64, axis=0)
    _capped(cent, win, np.arange(n), "the winning centroid of every row")
    two = np.sort(cent.s64, axis=0)[-2:]
    assert float((two[1] - two[0]).min()) > 4 * float(cent.chain.max())  # every row's label is well defined


@pytest.mark.parametrize("d,dt,n", wr.FAMILY, ids=_ids(wr.FAMILY))
def test_the_family_cases_meet_the_reference_conditions(d: int, dt, n: int) -> None:
    family_conditions(wr.family_case(d, dt, n))


def large_k_conditions(c) -> None:
    """k = 1000 of 1200 rows: float32 ties are likely, so the order is held well defined the other way."""
    assert c.ref.fragile(1000) == 0
    assert c.ref.near_share(1000) <= wr.Reference.NEAR_CAP
    _matmul_within_chain(c.ref, 120, c.d)


@pytest.mark.parametrize("d,dt", wr.LARGE_K, ids=_ids(wr.LARGE_K))
def test_the_large_k_cases_meet_the_reference_conditions(d: int, dt) -> None:
    large_k_conditions(wr.large_k_case(d, dt))


def range_conditions(c) -> None:
    """Thresholds at the 5th score: the best six must be tie-free, and the cap holds over the best five."""
    _tie_free(c, 5)
    assert c.ref.fragile(6) == 0
    for nq in (7, 300):
        top = c.ref.best(5)[:nq]
        _capped(c.ref, np.broadcast_to(np.arange(nq)[:, None], top.shape), top, f"best five of {nq} queries")


@pytest.mark.parametrize("d,dt,n", wr.RANGE, ids=_ids(wr.RANGE))
def test_the_range_cases_meet_the_reference_conditions(d: int, dt, n: int) -> None:
    range_conditions(wr.range_case(d, dt, n))
