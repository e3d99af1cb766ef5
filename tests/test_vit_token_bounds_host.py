"""CPU checks of tests/vit_token_bounds.py, the references tests/test_gpu_vit_tokens_exact.py holds the patch-token head
(LayerNorm form) and isc_vit_pos_resample to, in the manner of test_vit_bounds_host.py.

* A correct float32 evaluation is inside every bound: torch / numpy restatements in another order than the kernel's
  (the head) or in the kernel's order with and without contraction (the position table), on the GPU test's own operands.
  The share of the bound they use is printed.
* Planted faults are outside.
    eps          on the `small` rows (variance about eps) a LayerNorm with 1e-5 for 1e-6, the reverse, or 0 leaves the
                 bound on at least 99 % of the elements (an element next to its row's mean is beta whatever eps
                 is); on the other families it cannot be seen, which is why `small` exists.
    the head     one 16-byte vector left out of a cell's norm; the norm of the neighbouring cell.
    the table    A = -0.5; the - 0.5 dropped from the source coordinate; the two axis scales exchanged (non-square
                 grids); border taps mirrored instead of clamped.
* The exact cases are exact: every float32 intermediate of the weights equals its float64 value, the partial sums stay
  in the exact range, both float32 restatements and float64 `F.interpolate` EQUAL the reference, and the four borders
  are clamped with a weight that is not zero.
* `constant-exact` rows return beta exactly in float32 whatever the order; rows of `constant` do not (their float32 mean
  in the kernel's summation order is off by an ulp on a good share of them), which is why the un-normalised cell is
  asserted to equal beta on the former only."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402
import vit_token_bounds as tb  # noqa: E402


def _outside(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    return ~((got.double() - want).abs() <= bound)


# ----------------------------------------------------------------------------------------------------------- eps
@pytest.mark.parametrize("d", [4, 252, 256, 768, 1024, 2048])
def test_small_rows_show_a_wrong_eps(d: int) -> None:
    c = vb.layernorm_case(5, d, "small", seed=d)
    x, g, b = c["x"], c["gamma"], c["beta"]
    var = float(x.double().var(dim=1, unbiased=False).mean())
    assert 0.2e-6 < var < 5e-6 or d == 4
    for eps in tb.HEAD_EPS:
        want, bound = vb.layernorm_reference(x, g, b, eps)
        ratio = mb.assert_within_bound(vb.layernorm_restated(x, g, b, eps), want, bound, f"small, D = {d}, eps {eps}")
        shares = []
        for wrong in (e for e in (1e-6, 1e-5, 0.0) if e != eps):
            out = _outside(vb.layernorm_restated(x, g, b, wrong), want, bound)
            shares.append(float(out.double().mean()))
            # an element next to the row's mean is beta whatever eps is: all but a hundredth, and in every row
            assert shares[-1] >= 0.99 and bool(out.any(dim=1).all()), f"D = {d}: eps {wrong} for {eps}: {shares[-1]}"
        print(f"small D = {d} eps {eps}: restatement uses {ratio:.3f} of the bound; wrong eps outside on {shares}")


@pytest.mark.parametrize("family", ["randn", "far-mean", "constant", "spike"])
def test_the_other_families_cannot_see_eps(family: str) -> None:
    c = vb.layernorm_case(5, 768, family, seed=768)
    want, bound = vb.layernorm_reference(c["x"], c["gamma"], c["beta"], 1e-6)
    out = _outside(vb.layernorm_restated(c["x"], c["gamma"], c["beta"], 1e-5), want, bound)
    print(f"{family}: eps 1e-5 for 1e-6 is outside on {float(out.double().mean()):.3f} of the elements")
    assert float(out.double().mean()) < 0.5


# ------------------------------------------------------------------------------------------------------- the head
@pytest.mark.parametrize("family", tb.HEAD_FAMILIES)
def test_head_restatement_is_within_both_bounds(family: str) -> None:
    worst_ln = worst_map = 0.0
    for d in tb.HEAD_D:
        c = tb.head_case(d, family, seed=d)  # the GPU test's operands
        x = c["x"].reshape(-1, d)
        for eps in tb.HEAD_EPS:
            ref = tb.head_reference(x, c["gamma"], c["beta"], eps)
            ln = vb.layernorm_restated(x, c["gamma"], c["beta"], eps)
            worst_ln = max(worst_ln, mb.assert_within_bound(ln, ref["ln"], ref["ln_bound"], f"{family}, D = {d}, LN"))
            z = tb.head_restated(x, c["gamma"], c["beta"], eps)
            worst_map = max(worst_map, mb.assert_within_bound(z, ref["map"], ref["map_bound"], f"{family}, D = {d}, map"))
            plain = F.normalize(F.layer_norm(x.double(), (d,), c["gamma"].double(), c["beta"].double(),
                                             float(torch.tensor(eps, dtype=torch.float32))), dim=1, eps=1e-12)
            assert float((plain - ref["map"]).abs().max()) <= 1e-9
    print(f"head {family}: restatement uses {worst_ln:.3f} (un-normalised) and {worst_map:.3f} (normalised) of the bound")


@pytest.mark.parametrize("d", [4, 252, 768, 1024])
def test_head_faults_leave_the_normalised_bound(d: int) -> None:
    c = vb.layernorm_case(40, d, "randn", seed=200 + d)
    x, g, b = c["x"], c["gamma"], c["beta"]
    ref = tb.head_reference(x, g, b, 1e-6)
    mb.assert_within_bound(tb.head_restated(x, g, b, 1e-6), ref["map"], ref["map_bound"], "fault operands")
    hit = []
    for row in range(40):  # one 16-byte vector left out of the norm of `row`
        out = _outside(tb.head_restated(x, g, b, 1e-6, skip_vector=(row, (row * 7) % (d // 4))), ref["map"], ref["map_bound"])
        hit.append(bool(out[row].any()))
        assert not bool(out[torch.arange(40) != row].any())
    assert sum(hit) >= 36, sum(hit)
    rows = _outside(tb.head_restated(x, g, b, 1e-6, neighbour_norm=True), ref["map"], ref["map_bound"]).any(dim=1)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())


def test_l2_compose_refuses_a_row_it_cannot_bound() -> None:
    y = torch.full((1, 8), 1e-3, dtype=torch.float64)
    with pytest.raises(ValueError, match="no bound for its direction"):
        tb.l2_compose(y, torch.full_like(y, 1e-3))


def _kernel_order_mean(x: np.ndarray) -> np.ndarray:
    """The float32 mean of each row in the head's documented order: four per lane and vector, vectors in sequence, the
    xor butterfly over 64 lanes, one division."""
    rows, d = x.shape
    nv = (d // 4 + 63) // 64
    v = np.zeros((rows, nv * 256), dtype=np.float32)
    v[:, :d] = x
    v = v.reshape(rows, nv, 64, 4)
    s = np.zeros((rows, 64), dtype=np.float32)
    for i in range(nv):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ off]
    return s[:, 0] / np.float32(d)


def test_constant_exact_rows_return_beta_and_constant_rows_need_not() -> None:
    inexact = {}
    for d in tb.HEAD_D:
        c = tb.head_case(d, "constant-exact", seed=d)
        x = c["x"].reshape(-1, d)
        for eps in tb.HEAD_EPS:
            got = vb.layernorm_restated(x, c["gamma"], c["beta"], eps)
            assert torch.equal(got, c["beta"].expand_as(got))
        for order in (torch.arange(d), torch.arange(d - 1, -1, -1), torch.randperm(d, generator=vb.gen(d))):
            assert torch.equal(x[:, order].cumsum(dim=1)[:, -1] / d, x[:, 0])  # a sequential sum in any order
        assert np.array_equal(_kernel_order_mean(x.numpy()), x[:, 0].numpy())
        loose = tb.head_case(d, "constant", seed=d)["x"].reshape(-1, d).numpy()
        inexact[d] = int((_kernel_order_mean(loose) != loose[:, 0]).sum())
    print(f"`constant` rows (of {tb.MAX_B * tb.MAX_CELLS}) whose float32 mean in the kernel's order is not the constant: {inexact}")
    assert all(inexact[d] == 0 for d in (4, 256, 512, 1024))  # every step doubles
    assert all(inexact[d] > 0 for d in (252, 260, 516, 768, 772, 1020))


# -------------------------------------------------------------------------------------------- the position table
def test_weight_constants_are_evaluated_not_assumed() -> None:
    sw, lip = tb.weight_constants()
    sw_fine, lip_fine = tb.weight_constants(phases=1000001)
    t = np.linspace(0.0, 1.0, 999)
    assert sw >= float(np.abs(tb.cubic_weights(t)).sum(axis=-1).max())
    assert lip >= float(np.abs(tb.cubic_slopes(t)).sum(axis=-1).max())
    assert 0 <= sw - sw_fine < 1e-4 and 0 <= lip - lip_fine < 1e-3  # the allowance shrinks with the step, from above
    num = (tb.cubic_weights(t + 1e-7) - tb.cubic_weights(t - 1e-7)) / 2e-7  # the slopes are the weights' derivatives
    assert float(np.abs(num - tb.cubic_slopes(t)).max()) < 1e-6
    assert float(np.abs(tb.cubic_weights(t).sum(axis=-1) - 1).max()) < 1e-12  # a partition of unity
    print(f"sum|w| <= {sw:.6f}, sum|dw/dt| <= {lip:.6f}")
    assert tb.weight_constants(a=-0.5) != (sw, lip)


def _interpolate64(pos: torch.Tensor, g: int, h: int, w: int) -> torch.Tensor:
    d = pos.shape[1]
    out = F.interpolate(pos[1:].double().reshape(1, g, g, d).permute(0, 3, 1, 2), size=(h, w), mode="bicubic",
                        align_corners=False)
    return torch.cat([pos[:1].double(), out.permute(0, 2, 3, 1).reshape(h * w, d)])


@pytest.mark.parametrize("g,h,w", tb.RESAMPLE_GRIDS)
def test_resample_restatements_are_within_the_bound(g: int, h: int, w: int) -> None:
    for n in (h, w):  # both float32 coordinates within ds of the rational one
        _idx, _wgt, ds = tb.rational_axis(g, n)
        exact = np.array([g / n * (i + 0.5) - 0.5 for i in range(n)])
        for fused in (True, False):
            off = np.abs(tb.float32_coordinate(g, n, fused=fused).astype(np.float64) - exact)
            assert bool((off <= ds).all()), (g, n, fused, float((off / ds).max()))
    for d in tb.RESAMPLE_D:
        pos = tb.resample_table(g, d, seed=g * 100 + h * 10 + w)  # the GPU test's table
        want, bound = tb.resample_reference(pos, g, h, w)
        ratios = [mb.assert_within_bound(tb.resample_restated(pos, g, h, w, fused=fused), want, bound,
                                         f"{g} -> {h} x {w}, D = {d}, fused = {fused}") for fused in (True, False)]
        top = float(pos[1:].abs().max())
        err = max(float((tb.resample_restated(pos, g, h, w, fused=f).double() - want).abs().max()) for f in (True, False))
        print(f"pos_resample {g} -> {h} x {w}, D = {d}: restatements use {ratios[0]:.3f} (fused) and {ratios[1]:.3f} of the "
              f"bound; max|err| = {err / (tb.U * top):.1f} u max|pos|")
        assert float((_interpolate64(pos, g, h, w) - want).abs().max()) <= 1e-9 * top  # the reference IS torch's bicubic


def test_the_tap_set_differs_at_14_to_46() -> None:
    idx, _w, _ds = tb.rational_axis(14, 46)
    crossed = []
    for fused in (True, False):
        src = tb.float32_coordinate(14, 46, fused=fused)
        got = np.clip(np.floor(src).astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, 13)
        crossed.append(np.nonzero((got != idx).any(axis=1))[0].tolist())
    print(f"14 -> 46: outputs whose float32 taps differ from the rational ones: fused {crossed[0]}, unfused {crossed[1]}")
    assert 11 in crossed[0] or 11 in crossed[1]


FAULTS = {
    "A = -0.5": (dict(a=-0.5), [(14, 11, 17), (14, 17, 11), (14, 1, 196), (14, 46, 46), (16, 37, 37), (37, 16, 16), (64, 100, 3)]),
    "no half-pixel offset": (dict(half_pixel=False), [(14, 11, 17), (14, 17, 11), (14, 1, 196), (14, 46, 46), (16, 37, 37),
                                                     (37, 16, 16), (64, 100, 3), (5, 1, 1)]),
    "scales exchanged": (dict(swap_scales=True), [(14, 11, 17), (14, 17, 11), (14, 1, 196), (64, 100, 3)]),
    "mirrored borders": (dict(mirror=True), [(14, 11, 17), (14, 17, 11), (14, 46, 46), (16, 37, 37), (64, 100, 3)]),
}


@pytest.mark.parametrize("fault", FAULTS)
def test_resample_faults_leave_the_bound(fault: str) -> None:
    kw, grids = FAULTS[fault]
    for g, h, w in grids:
        for d in tb.RESAMPLE_D:
            pos = tb.resample_table(g, d, seed=g * 100 + h * 10 + w)
            want, bound = tb.resample_reference(pos, g, h, w)
            for fused in (True, False):
                out = _outside(tb.resample_restated(pos, g, h, w, fused=fused, **kw), want, bound)
                assert not bool(out[0].any())  # the class row is a copy in every variant
                rows = out[1:].any(dim=1).reshape(h, w)
                share = float(rows.double().mean())
                if fault == "mirrored borders":  # only cells with a clamped tap can differ: the border cells all do
                    inner_y, inner_x = ((np.diff(tb.rational_axis(g, n)[0], axis=1) == 1).all(axis=1) for n in (h, w))
                    inner = torch.from_numpy(inner_y[:, None] & inner_x[None, :])
                    assert not bool(rows[inner].any()) and not bool(inner[0].any()) and not bool(inner[-1].any())
                    edge = torch.zeros(h, w, dtype=torch.bool)
                    edge[0], edge[-1] = ~torch.from_numpy(inner_y)[0], ~torch.from_numpy(inner_y)[-1]
                    edge[:, 0] |= ~torch.from_numpy(inner_x)[0]
                    edge[:, -1] |= ~torch.from_numpy(inner_x)[-1]
                    assert bool(edge.any()) and bool(rows[edge].all()), (fault, g, h, w)
                else:
                    assert share >= 0.9, (fault, g, h, w, d, share)
    print(f"{fault}: outside on {grids}")


@pytest.mark.parametrize("g,h,w", tb.EXACT_GRIDS)
def test_exact_resample_cases_are_exact(g: int, h: int, w: int) -> None:
    c = tb.exact_resample_case(g, h, w, 8, seed=g + h + w)  # asserts the weights and the range itself
    assert c["top"] < 2.0**24 * 2.0**-16
    for fused in (True, False):
        assert torch.equal(tb.resample_restated(c["pos"], g, h, w, fused=fused), c["want"])
    assert torch.equal(_interpolate64(c["pos"], g, h, w), c["want"].double())
    assert c["border"] == {"top": h != g, "bottom": h != g, "left": w != g, "right": w != g}
    assert not torch.equal(c["want"][1:], c["want"][1:].round())  # and the weights did something
    for kw in (dict(a=-0.5), dict(half_pixel=False), dict(mirror=True)):  # the exact cases see the faults too
        assert not torch.equal(tb.resample_restated(c["pos"], g, h, w, fused=True, **kw), c["want"])


def test_exact_case_helper_refuses_what_could_round() -> None:
    with pytest.raises(AssertionError, match="no float32 number"):
        tb.exact_axis_weights(14, 11)
    with pytest.raises(AssertionError, match="no multiples of the quantum"):
        tb.exact_axis_weights(8, 64)  # scale 1/8 is a float32 number; the weights at t = 1/16 are multiples of 2^-12 only


def test_native_grid_is_the_identity() -> None:
    pos = tb.resample_table(14, 4, seed=3)
    want, bound = tb.resample_reference(pos, 14, 14, 14)
    assert torch.equal(want, pos.double())
    for fused in (True, False):
        assert torch.equal(tb.resample_restated(pos, 14, 14, 14, fused=fused), pos)
