"""Wide-row cases (2048 <= D <= ISC_SEARCH_MAX_D = 8192) shared by test_wide_rows_host.py and test_gpu_wide_rows.py (a
helper, not a conftest): the dimension list, the dispatch rule of the float64 sweeps restated, case builders with fixed
seeds, and a score reference with a derived bound.

The score reference.  `want` is the exact quotient: `math.fsum` of the products q_i * b_i (each exact in float64: the inputs
are fp16 or fp32) over the float64 norm of the query.  A kernel that accumulates the same products in float64, in any order,
ends within

    chain_err = (Dpad + 70) * 2^-53 * sum|q_i b_i| / ||q||

of `want`: Dpad fma steps (each at most one rounding of a partial sum bounded by sum|q_i b_i|), the six shuffle sums of a
wave and the sums across 16-byte chunks, the norm chain (its relative error carries over to the quotient, which
sum|q_i b_i| / ||q|| bounds), the square root and the division.  So the float32 it returns is float32(want) unless `want`
lies within chain_err of a float32 rounding boundary (the midpoint of two neighbouring float32 values); there it may be
the neighbour: one ulp32.  `Reference.check` asserts exactly that, and a `Tally` caps the share of a test's compared scores
that had the allowance at 1 %.

A float64 matmul is such a kernel too, which makes the check cheap: its score s64 is within chain_err of `want`, so a pair
whose s64 is farther than 2 * chain_err from every boundary has float32(want) == float32(s64) and `want` is farther than
chain_err from the boundary: equality is asserted without an fsum.  Only the pairs inside 2 * chain_err (a fraction of a
per cent) are summed with `math.fsum`; test_wide_rows_host.py checks |s64 - want| <= chain_err on a sample of each case.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

F16, F32 = torch.float16, torch.float32

KSTEP_BYTES = 128  # ISC_KSTEP_BYTES
MAX_D = 8192  # ISC_SEARCH_MAX_D

WIDE_DIMS = (
    2048,  # the bank PCA's limit; well inside the four-query form
    3072,  # the last D of the four-query form of k_exact / k_exact_collapse / k_lr_sweep (dp = 3072 in both dtypes)
    3073,  # pads to the next K step (fp16 dp = 3136, fp32 dp = 3104): the first D of the two-query form; 49 fp16 K steps, odd
    6144,  # the last D of the two-query form
    6145,  # fp16 dp = 6208, fp32 dp = 6176: the first D of the one-query form; 97 fp16 K steps, odd
    8191,  # a ragged last 16-byte chunk at the limit
    8192,  # ISC_SEARCH_MAX_D
)


def esz(dtype: torch.dtype) -> int:
    return 2 if dtype == F16 else 4


def ksteps(d: int, dtype: torch.dtype) -> int:
    """isc_ksteps: 128-byte K steps of a row of `d` elements."""
    return (d * esz(dtype) + KSTEP_BYTES - 1) // KSTEP_BYTES


def dpad(d: int, dtype: torch.dtype) -> int:
    """`dp`: the row length padded to whole K steps."""
    return ksteps(d, dtype) * (KSTEP_BYTES // esz(dtype))


def queries_per_sweep(d: int, dtype: torch.dtype) -> int:
    """The instantiation launch_exact_t, launch_exact_collapse_t and the large-k sweep select."""
    dp = dpad(d, dtype)
    return 4 if dp <= 3072 else 2 if dp <= 6144 else 1


# ---- builders -------------------------------------------------------------------------------------------------------
def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def rows(kind: str, n: int, d: int, seed: int) -> torch.Tensor:
    """float32 `[n, d]`: "unit" random unit rows; "same_sign" (rand + 0.05, normalised: every product of a dot has the same
    sign, the worst case of the guard's bound); "raw" (unit rows times 3: an unnormalised bank)."""
    g = gen(seed)
    if kind == "same_sign":
        return torch.nn.functional.normalize(torch.rand(n, d, generator=g) + 0.05, dim=1)
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    return x * 3.0 if kind == "raw" else x


def with_ldq(q: torch.Tensor, pad: int) -> torch.Tensor:
    """The same queries as a view of a wider buffer (row stride D + pad), the tail filled with a value that would show."""
    if pad == 0:
        return q
    big = torch.full((q.shape[0], q.shape[1] + pad), 7.0, dtype=q.dtype, device=q.device)
    big[:, : q.shape[1]] = q
    return big[:, : q.shape[1]]


@dataclass(frozen=True)
class Case:
    kind: str
    d: int
    bank_dtype: torch.dtype
    q_dtype: torch.dtype
    n: int
    stored: torch.Tensor  # [n, d] of the bank dtype: what the bank holds (built with normalize=False)
    queries: torch.Tensor  # [Q, d] of the query dtype
    ldq_pad: int
    k_max: int  # the largest k of the case's top-k searches: its best k_max + 1 scores per query are tie-free

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.d}-{_name(self.bank_dtype)}-{_name(self.q_dtype)}"

    @functools.cached_property
    def ref(self) -> "Reference":
        return Reference(self.stored, self.queries)


def _name(dt: torch.dtype) -> str:
    return "f16" if dt == F16 else "f32"


DTYPES = ((F16, F16), (F16, F32), (F32, F16), (F32, F32))  # (bank, queries)
SEED = 7100  # base of every seed below; a seed that fails a condition of test_wide_rows_host.py is changed here
SEED_OF: dict[str, int] = {  # "<case id>-<N>" -> replacement seed (the default one failed a condition of the host test)
    "unit-6145-f32-f16-4500": 9071,
    "unit-8191-f16-f32-4500": 9080,
    "unit-8191-f32-f32-4500": 9117,
    "unit-8192-f32-f16-4500": 9081,
    "raw-4096-f16-f16-4500": 9059,
    "raw-4096-f32-f32-300": 9059,
    "raw-8192-f32-f32-4500": 9081,
    "unit-6145-f32-f32-300": 9071,
}



def max_queries(d: int) -> int:
    return 300 if d < 6144 else 130


def query_counts(d: int) -> tuple[int, ...]:
    """Every query tile (one of 64, one of 128, 256 + a ragged one); the two widest forms run fewer queries."""
    return (1, 65, 130, 300) if d < 6144 else (1, 130)


HARD_N = {(4096, F16): 4500, (4096, F32): 300, (8192, F16): 300, (8192, F32): 4500}  # same-sign / unnormalised banks


@functools.lru_cache(maxsize=3)
def case(kind: str, d: int, bank_dtype: torch.dtype, q_dtype: torch.dtype, n: int | None = None,
         nq: int | None = None) -> Case:
    """The case of (kind, D, dtypes).  N alternates between 4500 (two levels: 4096 | rest) and 300 (one ragged level) so
    that each dispatch form sees both with each dtype pair (the same-sign and unnormalised banks: HARD_N; the callers that
    want both sizes pass `n`); every other case has its queries in a wider buffer."""
    i = WIDE_DIMS.index(d) if d in WIDE_DIMS else d
    j = DTYPES.index((bank_dtype, q_dtype))
    if n is None:
        n = HARD_N[(d, bank_dtype)] if kind != "unit" else 4500 if (i + j) % 2 == 0 else 300
    if nq is None:
        nq = max_queries(d)
    cid = f"{kind}-{d}-{_name(bank_dtype)}-{_name(q_dtype)}-{n}"
    seed = SEED_OF.get(cid, SEED + 16 * i + 2 * j)
    b = rows(kind, n, d, seed)
    q = rows("same_sign" if kind == "same_sign" else "unit", nq, d, seed + 1)
    q[0] = b[n // 2] + 0.01 * q[0]  # a query next to a row
    if nq > 2:
        q[2] *= 37.5  # the score does not depend on the query's length
    return Case(kind, d, bank_dtype, q_dtype, n, b.to(bank_dtype), q.to(q_dtype), 8 if (i + j) % 3 == 0 else 0,
                min(120, n - 1))


# The cases of the other families, built here so that test_wide_rows_host.py holds the same data to the reference's conditions.
FAMILY = [(d, b, n) for d in (3073, 6145, 8192) for b in (F16, F32) for n in (4500, 300)]  # masked ... assign
LARGE_K = [(d, b) for d in (3072, 3073, 6145, 8192) for b in (F16, F32)]
RANGE = [(d, b, n) for d in (3073, 8192) for b in (F16, F32) for n in (300, 4500)]


def family_case(d: int, dt: torch.dtype, n: int) -> Case:
    return case("unit", d, dt, dt, n=n, nq=130)


def large_k_case(d: int, dt: torch.dtype) -> Case:
    return case("unit", d, dt, dt, n=1200, nq=9)


def range_case(d: int, dt: torch.dtype, n: int) -> Case:
    return case("unit", d, dt, dt, n=n, nq=300)


def centroids(d: int, dt: torch.dtype) -> torch.Tensor:
    """The 257 centroids of the assign tests (their first 3 and 65 are the smaller sets)."""
    return rows("unit", 257, d, d + 11).to(dt)


FAMILY_BEST = 900  # the filtered searches of the family tests select from a query's best 900 rows (the tests assert it)


def score_picks(n: int) -> torch.Tensor:
    """The 40 rows of the `scores` test: random, with a duplicate, the first row and the last."""
    pick = torch.randint(0, n, (40,), generator=gen(3))
    pick[1] = pick[0]
    pick[2], pick[3] = 0, n - 1
    return pick


# ---- the reference ------------------------------------------------------------------------------------------------------
def ulp32(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


def boundary_distance(x: np.ndarray) -> np.ndarray:
    """Distance of float64 `x` from the nearer float32 rounding boundary (the midpoints around float32(x))."""
    f = x.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    return np.minimum(x - (f + dn) * 0.5, (f + up) * 0.5 - x)


class Reference:
    """Scores of `queries` (rounded to the bank dtype, as every search does) against the stored rows."""

    NEAR_CAP = 0.01  # the share of compared scores that may lie near a rounding boundary

    def __init__(self, stored: torch.Tensor, queries: torch.Tensor) -> None:
        self.stored = stored.detach().cpu()
        b = self.stored.numpy().astype(np.float64)
        self.q = queries.to(stored.dtype).detach().cpu().numpy().astype(np.float64)
        self.dpad = dpad(stored.shape[1], stored.dtype)
        self.norm = np.array([max(math.sqrt(math.fsum(r * r)), 1e-12) for r in self.q])
        self.s64 = (self.q @ b.T) / self.norm[:, None]  # [Q, N]
        mag = (np.abs(self.q) @ np.abs(b).T) / self.norm[:, None]  # sum|q_i b_i| / ||q||
        self.chain = (self.dpad + 70) * 2.0 ** -53 * mag

    def want(self, qi: int, row: int) -> float:
        """The exact quotient of one pair."""
        return math.fsum(self.q[qi] * self.stored[row].numpy().astype(np.float64)) / self.norm[qi]

    def expect(self, qi: np.ndarray, row: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """`(float32(want), near)` of the pairs (qi[j], row[j]); `near`: `want` within chain_err of a rounding boundary."""
        s = self.s64[qi, row]
        chain = self.chain[qi, row]
        maybe = boundary_distance(s) <= 2.0 * chain
        near = np.zeros(s.shape, bool)
        for j in np.nonzero(maybe)[0]:
            s[j] = self.want(int(qi[j]), int(row[j]))
            near[j] = boundary_distance(s[j : j + 1])[0] <= chain[j]
        return s.astype(np.float32), near

    def check_pairs(self, got: np.ndarray, qi: np.ndarray, row: np.ndarray, tally: "Tally", what: str = "") -> None:
        """float32 scores `got[j]` of the pairs (qi[j], row[j]); `tally` counts how many of them got the one-ulp allowance."""
        assert got.dtype == np.float32 and got.shape == qi.shape == row.shape, (got.dtype, got.shape, qi.shape, row.shape)
        exp, near = self.expect(qi, row)
        err = np.abs(got.astype(np.float64) - exp.astype(np.float64))
        bad = np.where(near, ~(err <= ulp32(exp)), got != exp)
        if bad.any():
            j = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} scores outside the bound; first: query {int(qi[j])} "
                                 f"row {int(row[j])} got {got[j]!r} want {exp[j]!r} near={bool(near[j])}")
        tally.add(int(near.sum()), int(near.size))

    def check(self, got_s, got_i, tally: "Tally", queries: np.ndarray | None = None, what: str = "") -> None:
        """Scores `got_s` (float32 `[Q', k]`) of rows `got_i` (`[Q', k]`, entries < 0 are padding and skipped) for the
        queries `queries` (default: the first Q')."""
        gs = np.asarray(got_s.cpu() if isinstance(got_s, torch.Tensor) else got_s)
        gi = np.asarray(got_i.cpu() if isinstance(got_i, torch.Tensor) else got_i)
        assert gs.shape == gi.shape, (gs.shape, gi.shape)
        qs = np.arange(gs.shape[0]) if queries is None else np.asarray(queries)
        qi = np.broadcast_to(qs[:, None], gi.shape)
        live = gi >= 0
        self.check_pairs(gs[live], qi[live], gi[live], tally, what)

    def near_count(self, qi: np.ndarray, row: np.ndarray) -> tuple[int, int]:
        """(near-boundary pairs, pairs) of a population: what a `Tally` would count for it."""
        near = self.expect(np.asarray(qi).reshape(-1), np.asarray(row).reshape(-1))[1]
        return int(near.sum()), int(near.size)

    def best(self, m: int) -> np.ndarray:
        """Each query's best `m` rows by the float64 score."""
        return np.argsort(-self.s64, axis=1, kind="stable")[:, :m]

    def fragile(self, m: int) -> int:
        """How many of each query's best `m` scores are near a rounding boundary AND within one ulp32 of the next better or
        next worse score among its best m + 1: there a kernel's other rounding could change the (score, row) order.  0 makes
        index equality with the oracle well defined for every selection from those rows, float32 ties included."""
        top = self.best(m + 1)
        qi = np.broadcast_to(np.arange(top.shape[0])[:, None], top.shape)
        exp, near = self.expect(qi.reshape(-1), top.reshape(-1))
        f = exp.reshape(top.shape).astype(np.float64)
        near = near.reshape(top.shape)
        close = np.abs(np.diff(f, axis=1)) <= ulp32(f[:, :-1])
        touch = np.zeros(top.shape, bool)
        touch[:, :-1] |= close
        touch[:, 1:] |= close
        return int((near & touch).sum())

    def near_share(self, k: int) -> float:
        """The share of near-boundary scores among each query's best k."""
        top = self.best(k)
        near, total = self.near_count(np.broadcast_to(np.arange(top.shape[0])[:, None], top.shape), top)
        return near / total


class Tally:
    """The compared scores of one test and how many of them lay near a rounding boundary (and so had the one-ulp allowance):
    the share is capped, so the allowance cannot carry a test."""

    def __init__(self) -> None:
        self.near = self.total = 0

    def add(self, near: int, total: int) -> None:
        self.near += near
        self.total += total

    @property
    def share(self) -> float:
        return self.near / self.total if self.total else 0.0

    def assert_cap(self, what: str = "") -> None:
        assert self.total > 0, what
        assert self.share <= Reference.NEAR_CAP, (what, self.near, self.total)
