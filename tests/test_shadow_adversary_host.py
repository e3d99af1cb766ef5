"""The adversarial banks of tests/shadow_adversary.py do what they claim -- in the host model, without a GPU.  The GPU
test (tests/test_gpu_shadow_adversary.py) searches the very same banks; what it can show is only as strong as these inputs,
so every case is held here to:

  * the plan has an int8 level and every victim lies in one; no row that is not planted for a query reaches the query's
    pace-setters, and every victim is in the query's float64 top k;
  * THE THEOREM: every victim passes the unperturbed threshold of its level;
  * SENSITIVITY: each perturbation its family was built for drops at least one victim of at least one query --
        P1  e_t halved                          P2  M = 0, the plain fp16 threshold scaled
        P3  the record of the next tile in packed order (tile 0 after the last)
        P4  the record of query n ^ 1           P5  the e_q (n_t + e_t) term left out
    A, D, E: P1 and P2;  B: P3;  C: P4 and P5;  F: P2 in stage B's test against tau'.  The faults are detected in the model,
    not by running mutated kernels; the table is printed per case (pytest -s);
  * THE fp16 PATH DOES NOT NEED THE REDO: k_final's guard  float32((T + eps) / ||q||) < the k-th score  holds in float64
    with TWICE eps = Dpad 2^-23 ||q|| max||b||, T the kp-th best exact score.  A redo would run the fp16 filter over the
    whole bank and rescue a victim an int8 level had lost.  (F is exempt: its answer is a tie at T.)

WHICH TAU.  k_select (cosine_topk.hip) writes tau[q] = the score of entry kp - 1 of the carried list, and only when the list
holds kp entries; the list is the best kp, by (float32 filter score, lower packed row), of the previous list and the level's
survivors.  The sample level emits every row that reaches its workgroup's bound L, and at least kp rows of the workgroup
do, so the best kp rows of the sample are all emitted; a filter level keeps every row above tau, the int8 level (by the
theorem and k_rescore's proof) at least every row above tau' <= the next tau.  Hence tau of a level is EXACTLY the kp-th
best float32 filter score over all rows packed before the level -- nothing looser.  The model takes the float64 dot rounded
to float32 for the filter score; the kernel's differs by at most eps, so the theorem is checked with tau + eps and the
perturbations with tau - eps.

SLACK of the tightest victim, (acc - threshold) / M at the model's tau -- 1 - slack of M is really used up (CODE = 12,
RESIDUAL = 0.49, PACE_GAPS = 0.5 % .. 1.7 %, ANCHOR = 8, FILL = 0.4; tau rises from the 16th pace-setter as victims are found):

    A  16 684 x 64  0.365    300 123 x 64  0.366    400 123 x 100  0.371    1 400 123 x 64 (second chained level)  0.300
    B  300 123 x 64  0.361    1 400 123 x 64  0.292
    C  off-grid queries 0.34 .. 0.36, sign queries 0.46 .. 0.51 (on 21 columns the filler's residual is the tile's e_t),
       one-hot queries 1.6 .. 1.7 (a one-hot Q.dx cannot use up ||Q|| e_t; they are there as neighbours)
    D  0.371  (every term negative)
    E  50 123 x 1024: 0.391 (family A's queries; the saturated rows lose nothing: 5.0);  D = 160: 0.381;  D = 32: 0.370
    F  0.410 in the epilogue; in stage B the copies clear tau' by one fp16 ulp of every element, 0.06 % of the score

A slack below 0.5 is what lets P1 drop the row, below 1 P2.  Flipping RESIDUAL to -0.49 makes the int8 image overstate the
victims: the slack is 2.3, P1 and P2 keep them and this module fails -- the construction carries the sensitivity, not the shape.
"""

from __future__ import annotations

import numpy as np
import pytest
import shadow_adversary as sa
from bank_image import TILE_ROWS
from shadow_adversary import F

REQUIRED = {"A": ("P1", "P2"), "B": ("P3",), "C": ("P4", "P5"), "D": ("P1", "P2"), "E": ("P1", "P2"), "F": ()}


def _tau_window(case: sa.Case, qi: int, level: int) -> tuple[np.float32, np.float32]:
    """(tau - eps rounded down, tau + eps rounded up): the kernel's tau lies between them."""
    tau, eps = np.float64(case.tau(qi, level)), case.eps(qi)
    lo, hi = F(tau - eps), F(tau + eps)
    lo = np.nextafter(lo, F(-np.inf)) if np.float64(lo) > tau - eps else lo
    hi = np.nextafter(hi, F(np.inf)) if np.float64(hi) < tau + eps else hi
    return lo, hi


@pytest.mark.parametrize("name", list(sa.CASES))
def test_case(name: str) -> None:
    case = sa.build_case(name)
    lay = case.layout
    assert lay.kinds == case.kinds and 2 in lay.kinds
    assert sa.uses_shadow(lay.n, lay.d, min(lay.q, 1024)) == 1
    assert len(case.adv) <= 64 and lay.q > 256
    named = lay.named_tiles()
    assert {level for level, _, _ in named} == {i for i, kind in enumerate(lay.kinds) if kind == 2}  # every int8 level
    names = {nm for _, nm, _ in named}  # (a level of two tiles: its first tile is also the one before the ragged last)
    assert names == ({"first", "last"} if lay.n < 20_000 else {"first", "mid", "before_end", "last"})

    case.check_filler()
    slack, dropped, total = [], {p: 0 for p in sa.PERTURBATIONS}, 0
    for qi in case.adv:
        assert len(case.paces[qi]) >= sa.KP
        assert np.all(lay.pos(np.array(case.paces[qi])) < lay.ends[0])  # the pace-setters are in the sample level
        assert set(case.victims[qi]) <= set(case.topk(qi).tolist()), (name, qi)
        for row in case.victims[qi]:
            level = lay.level_of(int(lay.pos(row)))
            assert lay.kinds[level] == 2
            lo, hi = _tau_window(case, qi, level)
            kept, _ = case.verdict(qi, row, None, tau=hi)
            assert kept, (name, qi, row)  # the theorem
            slack.append(case.verdict(qi, row)[1])
            total += 1
            for p in sa.PERTURBATIONS:
                dropped[p] += 0 if case.verdict(qi, row, p, tau=lo)[0] else 1
        if case.family != "F":
            bound, kth = case.guard_margin(qi, room=2.0)
            assert bound < kth, (name, qi, bound, kth)
    cells = "  ".join(f"{p} {'dropped' if dropped[p] else 'kept   '} ({dropped[p]:3d}/{total})" for p in sa.PERTURBATIONS)
    print(f"\n{name:20s} {cells}  slack {min(slack):.3f} .. {max(slack):.3f} of M")
    for p in REQUIRED[case.family]:
        assert dropped[p] > 0, (name, p)
    globals()["_check_" + case.family.lower()](case)


def _check_a(case: sa.Case) -> None:
    for qi in case.adv:  # sign queries: no residual
        assert float(case.qrec(qi)[1][2]) == 0.0


def _check_b(case: sa.Case) -> None:
    lay = case.layout
    scale = case.tile_scale
    t0 = lay.ends[0] // TILE_ROWS  # (the pace-setters, in the sample level, are larger than the fine tiles' scales)
    recs = np.array([float(case.trec(t)[1][0]) for t in range(t0, lay.ntiles, 37)])
    assert np.allclose(recs * scale[t0::37], 127.0, rtol=1e-6)  # the records really follow the planned scales ...
    assert set(np.round(np.log2(scale / sa.ANCHOR)).astype(int)) == set(range(-4, 5))  # ... of 2^-4 .. 2^4
    expo = np.round(np.log2(scale / sa.ANCHOR)).astype(int)
    for level, kind in enumerate(lay.kinds):  # not periodic in the number of chunks of any int8 level (nor in tiles per chunk)
        if kind != 2:
            continue
        t0, t1 = lay.level_start(level) // TILE_ROWS, -(-lay.ends[level] // TILE_ROWS)
        per = -(-(t1 - t0) // min(lay.wgs, t1 - t0))
        for period in {per, -(-(t1 - t0) // per)}:
            assert np.any(expo[t0 : t1 - period] != expo[t0 + period : t1])
    for qi in case.adv:
        for row in case.victims[qi]:
            assert expo[int(lay.pos(row)) // TILE_ROWS] == 4


def _check_c(case: sa.Case) -> None:
    assert tuple(case.adv) == (0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025) and case.queries.shape[0] >= 1026
    eq = [float(case.qrec(qi)[1][2]) for qi in case.adv]
    for j in range(len(case.adv)):
        assert (eq[j] > 2.0) == (j % 3 == 1)  # only the off-grid queries have a residual, and a large one
    mags = [float(case.queries[qi].abs().max()) for qi in case.adv]
    assert min(mags) == 2.0**-6 and max(mags) == 2.0**6
    cq = [float(case.qrec(qi)[1][0]) for qi in case.adv]
    assert all(a != b for a, b in zip(cq, cq[1:]))
    # the neighbour's record drops a victim at each seam: among a lane's four queries, at the 256-query tile, at the pass
    for group in ((0, 1, 2, 3), (255, 256, 257), (1023, 1024, 1025)):
        lo = {qi: _tau_window(case, qi, max(i for i, kind in enumerate(case.layout.kinds) if kind == 2))[0] for qi in group}
        assert any(not case.verdict(qi, row, "P4", tau=lo[qi])[0] for qi in group for row in case.victims[qi]), group


def _check_d(case: sa.Case) -> None:
    assert case.exact.max() < 0  # every row scores negative on every adversarial query
    for qi in case.adv:
        for level, kind in enumerate(case.layout.kinds):
            if kind == 2:
                assert case.tau(qi, level) < 0


def _check_e(case: sa.Case) -> None:
    if case.d != 1024:
        return _check_a(case)
    assert sa.uses_shadow(case.n, 1024, 1024) == 1 and sa.uses_shadow(case.n, 1025, 1024) == 0
    lay = case.layout
    for qi in case.saturated:
        qcodes = case.qrec(qi)[0]
        assert np.all(np.abs(qcodes) == 127)
        accs = set()
        for _, _, tile in lay.named_tiles():
            codes = case.trec(tile)[0]
            accs |= {int(v) for v in codes[np.all(np.abs(codes) == 127, axis=1)] @ qcodes}
        assert {16_516_096, -16_516_096} <= accs
        s = case.exact[case.adv.index(qi)][np.array(case.victims[qi])]
        assert len(set(s.tolist())) == len(s)  # no two victims tie ...
        x = case.rows[np.array(case.victims[qi])].numpy()
        assert np.all(np.abs(x - x[0]) <= np.spacing(np.float16(4.0)))  # ... and they lie within one fp16 ulp of each other


def _check_f(case: sa.Case) -> None:
    qi = case.adv[0]
    assert len(case.copies) >= 40 and len(case.nears) >= 40 and len(case.copies) + len(case.nears) > 2 * sa.KP
    lay = case.layout
    assert len({int(p) // TILE_ROWS for p in lay.pos(np.array(case.copies + case.nears))}) >= 6
    tau, tau2, dropped = sa.stage_b(case, qi, case.level)
    assert tau < tau2 and not dropped  # stage A raised the threshold, stage B lost nothing
    exact = case.exact[0]
    assert float(tau2) == float(F(exact[case.nears[0]])) < float(F(exact[case.copies[0]]))
    _, _, lost = sa.stage_b(case, qi, case.level, "P2")
    assert set(lost) & set(case.victims[qi])  # M = 0 against tau' drops rows of the answer
    print(f"{case.name:20s} stage B: correct drops 0, P2 dropped ({len(set(lost) & set(case.copies))}/{len(case.copies)} copies)")
    assert case.victims[qi] == case.copies[: sa.K] == case.topk(qi).tolist()


def test_shadow_limit_in_d() -> None:
    for n, q in ((16_684, 1024), (300_123, 1024)):
        assert sa.uses_shadow(n, 1024, q) == 1 and sa.uses_shadow(n, 1025, q) == 0
