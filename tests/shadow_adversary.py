"""Banks and queries built to sit ON the bound of the int8 filter levels, and the host model that says what each level
must do with them (a helper, not a conftest; DESIGN.md section 2, "The int8 level").

An int8 level keeps a row when  acc = Q.X > floor(tau c_q c_t - M - delta),  M = ||Q|| e_t + e_q (n_t + e_t)
(cosine_topk.hip: isc_i8_threshold).  On iid rows the true neighbours lie far above tau and M is several times what a row
really loses to quantisation, so a threshold that is too tight by a factor of two, or that reads the record of the wrong
tile or of the wrong query, drops no row that matters.  The builders here make it matter:

  * a VICTIM is a row of the exact top k of its query whose int8 image understates it by almost all of M: a query of
    constant magnitude and signs s has e_q = 0 and ||Q|| = 127 sqrt(|S|) on its support S; a row  (12 + 0.49) s / c_t  has
    the codes 12 s and the residual +0.49 s, so Q.dx = 127 * 0.49 |S| = ||Q|| e_t when no row of the tile has a larger
    residual.  The tile's scale c_t = 127 / ANCHOR is fixed by one ANCHOR element of the victim row, in column 0, where
    every adversarial query is zero;
  * PACE-SETTERS are NPACE rows per query in the sample level (the first packed positions), plain multiples of the
    victim's direction that score PACE_GAPS (0.5 % .. 1.7 %) below it: they are the kp-th best score k_select finds, so the
    level's tau lies that close under the victim.  e_t halved needs tau within 0.245 / 12.49 = 2 % to drop the victim,
    the plain fp16 threshold (M = 0) within 4 %;
  * the FILLER, every other row, is small against the adversarial queries (`Case.check_filler` asserts it in float64) and
    well quantised where no victim sits, so that the random queries of the call see an ordinary bank.

Everything is placed by PACKED position (isc_bank_permutation, isc_cosine_topk_plan): `Layout.named_tiles` lists, for every
int8 level of the plan, its first tile, a tile in the middle of a workgroup's chunk, the tile before its end and, in the
last level, the ragged last tile of the bank.

FAMILIES (`CASES`): A the tight bound; B tiles whose scales differ by powers of two, victims in the coarse ones, a fine
tile after each; C neighbouring queries of three kinds and of magnitudes 2^-6 .. 2^6 around the indices where a lane's four
queries, the 256-query tile and the 1024-query pass meet; D a bank in the far hemisphere: every score, tau and tau' negative;
E D = 1024 with rows and queries of codes +-127 only (|acc| = 16 516 096) beside family A's victims, and family A at D = 160
and D = 32; F a cluster of equal and nearly equal rows that stage A of k_rescore cannot hold.

THE MODEL.  `record` is tests/bank_image.py's `quantise_reference` with the kernels' scale and rounded-up norms,
`threshold` tests/test_shadow_inequality.py's float32 `_threshold`; `Case.tau` is the tau k_select leaves (see
tests/test_shadow_adversary_host.py), `Case.verdict` the epilogue's test of one victim under a named perturbation P1 .. P5
of the threshold, `stage_b` k_rescore's two stages on the special rows of family F.
"""

from __future__ import annotations

import ctypes
import dataclasses
import functools

import numpy as np
import torch
from bank_image import TILE_ROWS, quantise_reference
from test_shadow_inequality import UP, F, _threshold

K = 10
KP = 16  # plan_kp(10): k + 6 rounded up to 16
ANCHOR = 8.0  # c_t = 127 / 8 = 15.875, a float32
ANCHOR_COL = 0
CODE = 12
RESIDUAL = 0.49  # the victims' residual, in units of the code; -0.49 makes the int8 image OVERSTATE them (host test fails)
NPACE = 18
PACE_GAPS = np.linspace(0.005, 0.017, NPACE)
FILL = 0.4
PERTURBATIONS = ("P1", "P2", "P3", "P4", "P5")


# ------------------------------------------------------------------------------------------------------------ layout
def _plan(n: int, d: int, q: int, k: int) -> tuple[list[int], list[int]]:
    from imagescry_amd import _lib

    nl = ctypes.c_int()
    ends = (ctypes.c_int64 * 16)()
    kinds = (ctypes.c_int * 16)()
    _lib.check(_lib.load().isc_cosine_topk_plan(_lib.ISC_F16, n, d, q, k, 1, 16, nl, ends, kinds), "isc_cosine_topk_plan")
    return list(ends[: nl.value]), list(kinds[: nl.value])


def uses_shadow(n: int, d: int, q: int, k: int = K) -> int:
    from imagescry_amd import _lib

    uses = ctypes.c_int()
    _lib.check(_lib.load().isc_cosine_topk_uses_shadow(_lib.ISC_F16, n, d, q, k, uses), "isc_cosine_topk_uses_shadow")
    return uses.value


class Layout:
    """Where the rows of an n-row bank lie (packed position <-> ORIGINAL row) and how a search of q queries cuts it."""

    def __init__(self, n: int, d: int, q: int, k: int = K) -> None:
        from imagescry_amd import _lib

        self.n, self.d, self.q, self.k = n, d, q, k
        self.ends, self.kinds = _plan(n, d, q, k)
        mul, inv = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().isc_bank_permutation(n, mul, inv), "isc_bank_permutation")
        self.mul, self.inv = mul.value, inv.value
        self.ntiles = -(-n // TILE_ROWS)
        # workgroups per query tile of a filter level (make_plan: TARGET_WGS / query tiles of 256)
        self.wgs = max(1, 256 // -(-min(q, 1024) // 256))

    def orig(self, pos):
        return (np.asarray(pos, dtype=np.int64) * np.int64(self.mul)) % np.int64(self.n)

    def pos(self, row):
        return (np.asarray(row, dtype=np.int64) * np.int64(self.inv)) % np.int64(self.n)

    def level_start(self, level: int) -> int:
        return 0 if level == 0 else self.ends[level - 1]

    def level_of(self, pos: int) -> int:
        return next(i for i, e in enumerate(self.ends) if pos < e)

    def tile_rows(self, tile: int) -> int:
        return min(TILE_ROWS, self.n - tile * TILE_ROWS)

    def next_tile(self, tile: int) -> int:
        return (tile + 1) % self.ntiles

    def named_tiles(self) -> list[tuple[int, str, int]]:
        """(level, name, tile) for every int8 level: "first", "mid" (neither first nor last of its workgroup's chunk),
        "before_end" (the last FULL tile of the level) and "last" (the ragged last tile of the bank)."""
        out: list[tuple[int, str, int]] = []
        for level, kind in enumerate(self.kinds):
            if kind != 2:
                continue
            r0, r1 = self.level_start(level), self.ends[level]
            t0, t1 = r0 // TILE_ROWS, -(-r1 // TILE_ROWS)  # [t0, t1)
            ragged = r1 % TILE_ROWS != 0
            named = [("first", t0), ("before_end", t1 - 2 if ragged else t1 - 1)]
            if ragged:
                named.append(("last", t1 - 1))
            per = -(-(t1 - t0) // min(self.wgs, t1 - t0))  # tiles per chunk, as make_plan's add() cuts the level
            if per >= 3:
                chunk = ((t1 - t0) // per) // 2
                named.append(("mid", t0 + chunk * per + per // 2))
            seen: set[int] = set()
            for name, tile in named:
                if t0 <= tile < t1 and tile not in seen:
                    seen.add(tile)
                    out.append((level, name, tile))
        return out


# ------------------------------------------------------------------------------------------------------------- model
def record(tile_f16: np.ndarray):
    """(codes int64 [rows, d], c_t, e_t, n_t) of a tile as k_bank_quantize writes them -- of a query, as one row, k_prep_i8's
    (Q, c_q, e_q, ||Q||).  The quantisation is bank_image.quantise_reference."""
    mx = F(np.abs(tile_f16.astype(F)).max())
    c = F(127.0) / mx if mx > 0 else F(1.0)
    codes, s_rows, n_rows = quantise_reference(np.ascontiguousarray(tile_f16), c)
    e = F(np.sqrt(s_rows.max())) * UP
    nrm = F(np.sqrt(np.float64(n_rows.max()))) * UP
    return codes, c, F(e), F(nrm)


def threshold(tau, cq, qn, eq, ct, et, nt) -> int:
    return _threshold(F(tau), F(cq), F(qn), F(eq), F(ct), F(et), F(nt))


def perturbed_threshold(which: str | None, tau, qrec, trec, qrec_other, trec_next) -> int:
    """The epilogue's threshold, or what a kernel with one named fault would compute.  qrec = (c_q, ||Q||, e_q),
    trec = (c_t, e_t, n_t)."""
    (cq, qn, eq), (ct, et, nt) = qrec, trec
    if which == "P1":  # e_t halved
        et = F(et * F(0.5))
    elif which == "P2":  # M = 0: the plain fp16 threshold, scaled
        qn, eq = F(0), F(0)
    elif which == "P3":  # the record of the next tile in packed order
        ct, et, nt = trec_next
    elif which == "P4":  # the record of query n ^ 1
        cq, qn, eq = qrec_other
    elif which == "P5":  # the e_q (n_t + e_t) term left out
        eq = F(0)
    else:
        assert which is None
    return threshold(tau, cq, qn, eq, ct, et, nt)


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    family: str
    layout: Layout
    rows: torch.Tensor  # fp16 [n, d], CPU, ORIGINAL order, for normalize=False
    queries: torch.Tensor  # fp16 [q, d], CPU
    adv: list[int]  # the adversarial queries' indices
    victims: dict[int, list[int]]  # query -> ORIGINAL rows
    paces: dict[int, list[int]]
    others: dict[int, list[int]] = dataclasses.field(default_factory=dict)  # further planted rows a query scores high on
    kinds: list[int] = dataclasses.field(default_factory=list)  # the plan the case was built for

    # -- rows
    @property
    def n(self) -> int:
        return self.layout.n

    @property
    def d(self) -> int:
        return self.layout.d

    def tile(self, tile: int) -> np.ndarray:
        lay = self.layout
        pos = tile * TILE_ROWS + np.arange(lay.tile_rows(tile), dtype=np.int64)
        return self.rows[torch.from_numpy(lay.orig(pos))].numpy()

    @functools.cached_property
    def special(self) -> np.ndarray:
        rows = [r for group in (self.victims, self.paces, self.others) for v in group.values() for r in v]
        return np.unique(np.array(rows, dtype=np.int64))

    @functools.cached_property
    def exact(self) -> np.ndarray:
        """float64 dots of the adversarial queries with every row: [len(adv), n].  fp16 products are exact in float64 and
        the sums of at most 1024 of them are far inside 2^-53 relative."""
        q = self.queries[self.adv].double()
        out = torch.empty(len(self.adv), self.n, dtype=torch.float64)
        for r0 in range(0, self.n, 1 << 17):
            out[:, r0 : r0 + (1 << 17)] = q @ self.rows[r0 : r0 + (1 << 17)].double().T
        return out.numpy()

    @functools.cached_property
    def max_row_norm(self) -> float:
        best = 0.0
        for r0 in range(0, self.n, 1 << 17):
            best = max(best, float(self.rows[r0 : r0 + (1 << 17)].double().norm(dim=1).max()))
        return best

    def topk(self, qi: int) -> np.ndarray:
        """ORIGINAL rows of the exact top k of query qi: float64 score descending, row ascending."""
        s = self.exact[self.adv.index(qi)]
        cand = np.nonzero(s >= np.partition(s, -self.layout.k)[-self.layout.k])[0]
        return cand[np.lexsort((cand, -s[cand]))][: self.layout.k]

    def check_filler(self) -> None:
        """No row that is not planted FOR the query reaches the query's pace-setters, in float64."""
        for a, qi in enumerate(self.adv):
            own = np.array(self.victims[qi] + self.paces[qi] + self.others.get(qi, []), dtype=np.int64)
            s = self.exact[a].copy()
            floor = s[np.array(self.paces[qi])].min()
            s[own] = -np.inf
            assert s.max() < floor, (self.name, qi, float(s.max()), float(floor))

    # -- the model
    @functools.lru_cache(maxsize=None)
    def qrec(self, qi: int):
        codes, c, e, nrm = record(self.queries[qi : qi + 1].numpy())
        return codes[0], (c, nrm, e)

    @functools.lru_cache(maxsize=None)
    def trec(self, tile: int):
        codes, c, e, nrm = record(self.tile(tile))
        return codes, (c, e, nrm)

    def tau(self, qi: int, level: int) -> np.float32:
        """The threshold k_select leaves for `level`: the kp-th best float32 score of the rows packed before it.  Only the
        query's own planted rows can be among them (check_filler)."""
        lay = self.layout
        own = np.array(self.victims[qi] + self.paces[qi] + self.others.get(qi, []), dtype=np.int64)
        before = own[lay.pos(own) < lay.level_start(level)]
        s = np.sort(self.exact[self.adv.index(qi)][before].astype(F))[::-1]
        assert len(s) >= KP, (self.name, qi, level, len(s))
        return F(s[KP - 1])

    def verdict(self, qi: int, row: int, which: str | None = None, tau=None) -> tuple[bool, float]:
        """(kept, slack): the int8 test of ORIGINAL row `row` against query qi in the row's own level; slack = (acc - the
        threshold) / M."""
        lay = self.layout
        pos = int(lay.pos(row))
        level, tile = lay.level_of(pos), pos // TILE_ROWS
        assert lay.kinds[level] == 2, (self.name, row, level)
        qcodes, qrec = self.qrec(qi)
        tcodes, trec = self.trec(tile)
        acc = int(tcodes[pos % TILE_ROWS] @ qcodes)
        assert abs(acc) < 2**24
        tau = self.tau(qi, level) if tau is None else tau
        other = self.qrec(qi ^ 1)[1] if (qi ^ 1) < self.queries.shape[0] else qrec
        thr = perturbed_threshold(which, tau, qrec, trec, other, self.trec(lay.next_tile(tile))[1])
        m = float(qrec[1]) * float(trec[1]) + float(qrec[2]) * (float(trec[2]) + float(trec[1]))
        return acc > thr, (acc - thr) / m

    def eps(self, qi: int) -> float:
        """k_final's bound on |filter score - exact dot|: Dpad 2^-23 ||q|| max||b||, with the published norm bound (1.001
        times the largest row norm, rounded up)."""
        ks = -(-self.d * 2 // 128)
        return ks * 64 * 2.0**-23 * float(self.queries[qi].double().norm()) * self.max_row_norm * 1.0011

    def guard_margin(self, qi: int, room: float = 1.0) -> tuple[float, float]:
        """k_final's guard in float64: (float32((T + room eps) / ||q||), the k-th score).  The query
        is proven without the redo when the first is below the second."""
        qn = float(self.queries[qi].double().norm())
        eps = self.eps(qi) * room
        s = np.sort(self.exact[self.adv.index(qi)][np.array(self.victims[qi] + self.paces[qi] + self.others.get(qi, []))])[::-1]
        t, kth = s[KP - 1], F(s[self.layout.k - 1] / qn)
        return float(F((t + eps) / qn)), float(kth)


def stage_b(case: Case, qi: int, level: int, which: str | None = None):
    """k_rescore on the query's planted rows of `level` (the filler scores far below tau): the list = the rows the
    epilogue keeps; stage A = the P = 2 kp entries with the best (acc / (c_q c_t), lower packed row); tau' = max(tau, the
    kp-th best of the carried scores and the P scores); stage B tests the others against tau' -- under `which` with the
    faulty threshold.  Returns (tau, tau', ORIGINAL rows dropped by stage B)."""
    lay = case.layout
    exact = case.exact[case.adv.index(qi)]
    own = np.array(case.victims[qi] + case.paces[qi] + case.others.get(qi, []), dtype=np.int64)
    pos = lay.pos(own)
    tau = case.tau(qi, level)
    carried = np.sort(exact[own[pos < lay.level_start(level)]].astype(F))[::-1][:KP]
    qcodes, qrec = case.qrec(qi)
    entries = []
    for r, p in zip(own, pos):
        if not lay.level_start(level) <= p < lay.ends[level]:
            continue
        tcodes, trec = case.trec(int(p) // TILE_ROWS)
        acc = int(tcodes[int(p) % TILE_ROWS] @ qcodes)
        if acc > threshold(tau, *qrec, *trec):
            entries.append((-float(F(acc) / F(qrec[0] * trec[0])), int(p), int(r), acc))
    entries.sort()
    first, rest = entries[: 2 * KP], entries[2 * KP :]
    scores = np.sort(np.concatenate([carried, exact[[e[2] for e in first]].astype(F)]))[::-1]
    tau2 = max(tau, F(scores[KP - 1])) if len(scores) >= KP else tau
    dropped = []
    for _, p, r, acc in rest:
        tile = p // TILE_ROWS
        thr = perturbed_threshold(which, tau2, qrec, case.trec(tile)[1], qrec, case.trec(lay.next_tile(tile))[1])
        if not acc > thr:
            dropped.append(r)
    return tau, tau2, dropped


# ---------------------------------------------------------------------------------------------------------- builders
def _patterns(rng: np.random.Generator, count: int, width: int, limit: float = 0.5) -> np.ndarray:
    """`count` sign patterns of `width` entries, no two of which agree or disagree in more than (1 + limit) / 2 of them."""
    out: list[np.ndarray] = []
    while len(out) < count:
        s = rng.choice([-1.0, 1.0], size=width)
        if all(abs(float(s @ o)) <= limit * width for o in out):
            out.append(s)
    return np.array(out)


def _walsh(rng: np.random.Generator, d: int, indices) -> np.ndarray:
    """Rows `indices` of the d x d Sylvester matrix times one random sign pattern: exactly orthogonal sign vectors."""
    i = np.arange(d)
    base = rng.choice([-1.0, 1.0], size=d)
    return np.array([base * (1 - 2 * (np.array([bin(int(v)).count("1") for v in (i & j)]) & 1)) for j in indices])


def _filler(n: int, d: int, seed: int, amp: float = FILL) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, d, generator=g) * 2 - 1) * amp).half()


def _random_queries(q: int, d: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(q, d, generator=g).half()


def _victim(d: int, support: np.ndarray, s: np.ndarray, anchor: float, code: float = CODE, resid: float = RESIDUAL,
            with_anchor: bool = True) -> np.ndarray:
    """(code + resid) s / c_t on the support, the anchor in column 0: codes `code` s, residuals `resid` s."""
    ct = np.float64(F(127.0) / F(anchor))
    x = np.zeros(d, dtype=np.float64)
    x[support] = (code + resid) * s / ct
    if with_anchor:
        x[ANCHOR_COL] = anchor
    return x.astype(np.float16)


class _Planter:
    """Planted rows by packed position; one row per position, none in a position twice."""

    def __init__(self, layout: Layout, seed: int) -> None:
        self.lay = layout
        self.rng = np.random.default_rng(seed)
        self.at: dict[int, np.ndarray] = {}
        self._slots: dict[int, list[int]] = {}

    def put(self, pos: int, row: np.ndarray) -> int:
        assert pos not in self.at and 0 <= pos < self.lay.n
        self.at[pos] = row
        return int(self.lay.orig(pos))

    def slot(self, tile: int) -> int:
        """A position of `tile` nobody has yet (never the tile's first: family B keeps its scale there)."""
        if tile not in self._slots:
            self._slots[tile] = list(1 + self.rng.permutation(self.lay.tile_rows(tile) - 1))
        return tile * TILE_ROWS + int(self._slots[tile].pop())

    def sample_slot(self) -> int:
        while True:
            pos = int(self.rng.integers(0, self.lay.ends[0]))
            if pos not in self.at and pos % TILE_ROWS != 0:
                return pos

    def paces(self, direction: np.ndarray, away: float = -1.0) -> list[int]:
        """NPACE shortened copies of `direction` in the sample level, PACE_GAPS below it on average (away = +1: for
        negative scores, where "below" is the longer vector)."""
        out = []
        for g in PACE_GAPS:  # (per element 0 .. 2 g: one factor for the whole row would move in steps of an fp16 ulp, 0.05 %)
            factor = 1 + away * 2 * g * self.rng.random(direction.shape[0])
            out.append(self.put(self.sample_slot(), (direction.astype(np.float64) * factor).astype(np.float16)))
        return out

    def apply(self, rows: torch.Tensor) -> None:
        pos = np.array(sorted(self.at), dtype=np.int64)
        rows[torch.from_numpy(self.lay.orig(pos))] = torch.from_numpy(np.array([self.at[int(p)] for p in pos]))


def _adv_indices(q: int, count: int) -> list[int]:
    return sorted({int(v) for v in np.linspace(0, q - 1, count)})


def build_a(name: str, n: int, d: int, q: int, kinds: list[int], nadv: int = 16, family: str = "A") -> Case:
    """Sign queries of magnitudes 2^-2 .. 2^2 on columns 1 .. d - 1; per query one victim in every named tile."""
    lay = Layout(n, d, q)
    seed = n % 1000 + d
    pl = _Planter(lay, seed)
    support = np.arange(1, d)
    adv = _adv_indices(q, nadv)
    pats = _patterns(pl.rng, len(adv), d - 1)
    queries = _random_queries(q, d, seed + 1)
    victims, paces = {}, {}
    for j, qi in enumerate(adv):
        qv = np.zeros(d)
        qv[support] = pats[j] * 2.0 ** (j % 5 - 2)
        queries[qi] = torch.from_numpy(qv).half()
        row = _victim(d, support, pats[j], ANCHOR)
        victims[qi] = [pl.put(pl.slot(tile), row) for _, _, tile in lay.named_tiles()]
        paces[qi] = pl.paces(_victim(d, support, pats[j], ANCHOR, with_anchor=False))
    rows = _filler(n, d, seed + 2)
    pl.apply(rows)
    return Case(name, family, lay, rows, queries, adv, victims, paces, kinds=kinds)


def _tile_exponent(tile: int) -> int:
    return int((tile * 2654435761 >> 7) % 9) - 4  # -4 .. 4, a hash: periodic in nothing


def build_b(name: str, n: int, d: int, q: int, kinds: list[int], nadv: int = 16) -> Case:
    """Every tile has its own scale: columns d / 2 .. d - 1 of its filler are uniform in +-A_t, A_t = 8 * 2^(-4 .. 4), the
    tile's first row holding A_t itself.  The adversarial queries live on columns 1 .. d / 2 - 1, where the filler is small;
    victims sit in tiles of scale 2^4 (their own anchor is 128) and the tile after each has scale 2^-4."""
    lay = Layout(n, d, q)
    seed = n % 1000 + d + 7
    pl = _Planter(lay, seed)
    half = d // 2
    support = np.arange(1, half)
    adv = _adv_indices(q, nadv)
    pats = _patterns(pl.rng, len(adv), len(support))
    queries = _random_queries(q, d, seed + 1)
    expo = np.array([_tile_exponent(t) for t in range(lay.ntiles)])
    coarse = [tile for _, _, tile in lay.named_tiles()]
    for tile in coarse:
        expo[tile] = 4
    for tile in coarse:  # (two named tiles may be neighbours: the later one stays coarse)
        if lay.next_tile(tile) not in coarse:
            expo[lay.next_tile(tile)] = -4
    scale = ANCHOR * 2.0**expo
    big = float(scale.max())
    victims, paces = {}, {}
    for j, qi in enumerate(adv):
        qv = np.zeros(d)
        qv[support] = pats[j] * 2.0 ** (j % 5 - 2)
        queries[qi] = torch.from_numpy(qv).half()
        victims[qi] = [pl.put(pl.slot(tile), _victim(d, support, pats[j], big)) for tile in coarse]
        paces[qi] = pl.paces(_victim(d, support, pats[j], big, with_anchor=False))
    rows = _filler(n, d, seed + 2)
    amp = torch.from_numpy(scale[lay.pos(np.arange(n)) // TILE_ROWS])
    g = torch.Generator().manual_seed(seed + 3)
    rows[:, half:] = ((torch.rand(n, d - half, generator=g, dtype=torch.float64) * 2 - 1) * amp[:, None]).half()
    firsts = torch.from_numpy(lay.orig(np.arange(lay.ntiles, dtype=np.int64) * TILE_ROWS))
    rows[firsts, half] = torch.from_numpy(scale).half()
    pl.apply(rows)
    case = Case(name, "B", lay, rows, queries, adv, victims, paces, kinds=kinds)
    case.tile_scale = scale  # type: ignore[attr-defined]
    return case


C_INDICES = (0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025)
C_EXPONENTS = (-6, 6, -3, 3, 5, -5, 2, 0, -2, 6)
C_OFFGRID_CODE = 100


def build_c(name: str, n: int, d: int, q: int, kinds: list[int]) -> Case:
    """Three kinds of query on three disjoint sets of columns, alternating along C_INDICES, magnitudes 2^C_EXPONENTS:
    sign vectors (family A's victims); OFF-GRID queries with entries s (m + 0.49) / c_q, m in 1 .. 4, and one entry of
    127 / c_q fixing c_q -- e_q = 0.49 sqrt(width) -- whose victims are 100 s / c_t: codes 100 s, aligned with dq, so that
    dq.(X + dx) is nearly e_q n_t; one-hot queries, whose victims hold the code 120.49 in the query's column."""
    assert q > max(C_INDICES) and d >= 64
    lay = Layout(n, d, q)
    seed = n % 1000 + d + 13
    pl = _Planter(lay, seed)
    third = (d - 1) // 3
    supports = [np.arange(1 + i * third, 1 + (i + 1) * third) for i in range(3)]
    adv = list(C_INDICES)
    queries = _random_queries(q, d, seed + 1)
    pats = [_patterns(pl.rng, 4, third), _patterns(pl.rng, 4, third - 1), None]
    tiles = [tile for _, _, tile in lay.named_tiles()]
    victims, paces = {}, {}
    for j, qi in enumerate(adv):
        kind, mag = j % 3, 2.0 ** C_EXPONENTS[j]
        qv = np.zeros(d)
        if kind == 0:
            sup, s = supports[0], pats[0][j // 3]
            qv[sup] = s * mag
            row = _victim(d, sup, s, ANCHOR)
        elif kind == 1:
            sup, s = supports[1][1:], pats[1][j // 3]
            m = pl.rng.integers(1, 5, size=len(sup))
            qv[supports[1][0]] = mag  # code 127, no residual: c_q = 127 / mag
            qv[sup] = s * (m + RESIDUAL) * mag / 127.0
            row = _victim(d, sup, s, ANCHOR, code=C_OFFGRID_CODE, resid=0.0)
        else:
            sup, s = supports[2][j // 3 : j // 3 + 1], np.ones(1)
            qv[sup] = mag
            row = _victim(d, sup, s, ANCHOR, code=120)
        queries[qi] = torch.from_numpy(qv).half()
        victims[qi] = [pl.put(pl.slot(tile), row) for tile in tiles]
        bare = row.copy()
        bare[ANCHOR_COL] = 0
        paces[qi] = pl.paces(bare)
    rows = _filler(n, d, seed + 2)
    pl.apply(rows)
    return Case(name, "C", lay, rows, queries, adv, victims, paces, kinds=kinds)


def build_d(name: str, n: int, d: int, q: int, kinds: list[int], nadv: int = 8) -> Case:
    """One sign pattern s: the filler is -u s + noise with u = 2 +- 0.12, the adversarial queries are s at magnitudes
    2^-4 .. 2^3 and score negative on every row.  They share the victims (-12 + 0.49) s / c_t -- the least negative rows of
    the bank -- and the pace-setters, which are longer: tau c_q c_t < 0 takes isc_i8_threshold's |t| and floors below zero."""
    lay = Layout(n, d, q)
    seed = n % 1000 + d + 19
    pl = _Planter(lay, seed)
    support = np.arange(1, d)
    s = pl.rng.choice([-1.0, 1.0], size=d - 1)
    adv = _adv_indices(q, nadv)
    queries = _random_queries(q, d, seed + 1)
    row = _victim(d, support, s, ANCHOR, code=-CODE)
    shared_v = [pl.put(pl.slot(tile), row) for _, _, tile in lay.named_tiles()]
    shared_p = pl.paces(_victim(d, support, s, ANCHOR, code=-CODE, with_anchor=False), away=1.0)
    for j, qi in enumerate(adv):
        qv = np.zeros(d)
        qv[support] = s * 2.0 ** (j % 8 - 4)
        queries[qi] = torch.from_numpy(qv).half()
    g = torch.Generator().manual_seed(seed + 2)
    # (u normal and the noise wide: rows of one length and one direction put a tenth of the bank within M of every tau)
    u = 2.0 + 0.12 * torch.randn(n, 1, generator=g)
    rows = (-u * torch.from_numpy(np.concatenate([[0.0], s])).float()[None, :]
            + (torch.rand(n, d, generator=g) * 2 - 1) * 0.6).half()
    pl.apply(rows)
    return Case(name, "D", lay, rows, queries, adv, {qi: shared_v for qi in adv}, {qi: shared_p for qi in adv}, kinds=kinds)


def build_e(name: str, n: int, d: int, q: int, kinds: list[int]) -> Case:
    """D = 1024, exactly orthogonal sign patterns (Walsh).  Two SATURATED queries, sign vectors on every column, whose
    victims are +-8 everywhere: all codes +-127, acc = +16 516 096, the six victims one fp16 ulp apart in 0 .. 5 elements
    (equal codes, equal acc: their order is the float64 re-score's), and the row -8 s with acc = -16 516 096 in the same
    tiles.  Four queries of family A beside them."""
    assert d == 1024
    lay = Layout(n, d, q)
    seed = n % 1000 + d + 23
    pl = _Planter(lay, seed)
    pats = _walsh(pl.rng, d, range(1, 7))
    adv = _adv_indices(q, 6)
    queries = _random_queries(q, d, seed + 1)
    tiles = [tile for _, _, tile in lay.named_tiles()]
    victims, paces, others = {}, {}, {}
    for j, qi in enumerate(adv):
        qv = np.zeros(d)
        if j < 2:
            qv[:] = pats[j] * 2.0 ** (1 - 2 * j)
            full = (pats[j] * ANCHOR).astype(np.float16)
            victims[qi] = []
            for v in range(6):
                row = full.copy()
                idx = 17 + 31 * np.arange(v)
                row[idx] = np.nextafter(row[idx], np.float16(0))
                victims[qi].append(pl.put(pl.slot(tiles[v % len(tiles)]), row))
            pl.put(pl.slot(tiles[0]), -full)  # scores lowest of all: not among the query's high rows
            paces[qi] = pl.paces(full)
        else:
            support = np.arange(1, d)
            qv[support] = pats[j][1:] * 2.0 ** (j - 3)
            row = _victim(d, support, pats[j][1:], ANCHOR)
            victims[qi] = [pl.put(pl.slot(tile), row) for tile in tiles]
            paces[qi] = pl.paces(_victim(d, support, pats[j][1:], ANCHOR, with_anchor=False))
        queries[qi] = torch.from_numpy(qv).half()
    # (eight times the filler of D = 64: the victims' residual norm grows with sqrt(D) and a saturated row makes n_t = 127 * 32,
    # so M of a random query in the victims' tiles is 56 000; its tau c_q c_t must stay well above that)
    rows = _filler(n, d, seed + 2, amp=8 * FILL)
    pl.apply(rows)
    case = Case(name, "E", lay, rows, queries, adv, victims, paces, others, kinds=kinds)
    case.saturated = adv[:2]  # type: ignore[attr-defined]
    return case


F_COPIES = 42


def build_f(name: str, n: int, d: int, q: int, kinds: list[int]) -> Case:
    """One sign query.  In the last int8 level, F_COPIES rows one fp16 ulp (in every element) below the victim at the
    lowest packed positions -- three tiles from the level's first -- and F_COPIES exact copies of the victim in three later
    tiles.  All 84 have the same codes, hence the same acc and approximate score: stage A takes the 32 lowest packed rows,
    all of the lower kind, tau' is THEIR score, and stage B decides about every copy with a threshold one ulp under it.
    The answer is the k copies of lowest ORIGINAL index."""
    lay = Layout(n, d, q)
    seed = n % 1000 + d + 29
    pl = _Planter(lay, seed)
    support = np.arange(1, d)
    s = pl.rng.choice([-1.0, 1.0], size=d - 1)
    qi = 5
    queries = _random_queries(q, d, seed + 1)
    qv = np.zeros(d)
    qv[support] = s * 0.5
    queries[qi] = torch.from_numpy(qv).half()
    level = max(i for i, kind in enumerate(lay.kinds) if kind == 2)
    t0, t1 = lay.level_start(level) // TILE_ROWS, lay.ends[level] // TILE_ROWS
    copy = _victim(d, support, s, ANCHOR)
    near = copy.copy()
    near[support] = np.nextafter(copy[support], np.float16(0))
    low_tiles = [t0, t0 + 1, t0 + 2]
    high_tiles = [t0 + (t1 - t0) // 3, t0 + (t1 - t0) // 3 + 1, t1 - 1]
    nears = [pl.put(pl.slot(low_tiles[i % 3]), near) for i in range(F_COPIES)]
    copies = [pl.put(pl.slot(high_tiles[i % 3]), copy) for i in range(F_COPIES)]
    paces = pl.paces(_victim(d, support, s, ANCHOR, with_anchor=False))
    rows = _filler(n, d, seed + 2)
    pl.apply(rows)
    case = Case(name, "F", lay, rows, queries, [qi], {qi: sorted(copies)[:K]}, {qi: paces},
                {qi: sorted(copies)[K:] + nears}, kinds=kinds)
    case.level = level  # type: ignore[attr-defined]
    case.copies, case.nears = sorted(copies), sorted(nears)  # type: ignore[attr-defined]
    return case


# name -> (builder, n, d, q, the plan's kinds, keyword arguments)
CASES = {
    "A-16684x64": (build_a, 16_684, 64, 1024, [0, 2], {}),
    "A-300123x64": (build_a, 300_123, 64, 1024, [0, 1, 2], {}),
    "A-400123x100-q300": (build_a, 400_123, 100, 300, [0, 1, 2], {}),
    "A-1400123x64": (build_a, 1_400_123, 64, 1024, [0, 1, 2, 2], {}),
    "B-300123x64": (build_b, 300_123, 64, 1024, [0, 1, 2], {}),
    "B-1400123x64": (build_b, 1_400_123, 64, 1024, [0, 1, 2, 2], {}),
    "C-300123x64-q1030": (build_c, 300_123, 64, 1030, [0, 1, 2], {}),
    "D-300123x64": (build_d, 300_123, 64, 1024, [0, 1, 2], {}),
    # (132 tiles in the level: a tile with a saturated row has n_t = 127 * 32 and lets a third of its rows pass for a random
    # query; in a level of two tiles that overflows the lanes' segments, here it is four tiles in four chunks)
    "E-50123x1024": (build_e, 50_123, 1024, 1024, [0, 2], {}),
    "E-16684x160": (build_a, 16_684, 160, 1024, [0, 2], {"family": "E"}),
    "E-16684x32": (build_a, 16_684, 32, 1024, [0, 2], {"family": "E", "nadv": 6}),
    "F-300123x64": (build_f, 300_123, 64, 1024, [0, 1, 2], {}),
}


def build_case(name: str) -> Case:
    builder, n, d, q, kinds, kwargs = CASES[name]
    return builder(name, n, d, q, kinds, **kwargs)
