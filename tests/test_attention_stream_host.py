"""CPU checks of tests/attention_stream_bounds.py, the references tests/test_gpu_attention_stream.py rests on, in the
manner of test_vit_bounds_host.py: the restated online softmax stays inside the bound on the GPU test's own operands
and returns the selector gathers exactly; each planted fault (O not rescaled at a seam, the sum never rescaled, a chunk
dropped, a zero-filled padded key admitted) leaves the bound or breaks a selector; every selector case the GPU test
uses builds; the long random cases pass the first-order check."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import attention_stream_bounds as sb  # noqa: E402
import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402

HEADS = 3
B = 2
QB, KC = sb.geometry()


def _outside_rows(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    out = ~((got.double() - want).abs() <= bound)
    return out.reshape(-1, out.shape[-1]).any(dim=1)


def test_geometry_and_lengths() -> None:
    assert KC % 32 == 0 and QB % 16 == 0
    ts = sb.stream_lengths(QB, KC)
    assert ts == sorted(set(ts)) and {1, 224, 225, KC, 2 * KC + 1, QB + 1, 1025} <= set(ts)


@pytest.mark.parametrize("masked", [False, True])
def test_every_selector_case_builds_and_the_restatement_returns_the_gather(masked: bool) -> None:
    for t in sb.stream_lengths(QB, KC):
        if masked and t % 16 == 0:
            continue
        c = sb.stream_selector_case(B, t, HEADS, masked=masked)  # raises on a weak one
        assert torch.equal(sb.stream_restated(c["qkv"], HEADS, KC), c["want"]), t


def test_the_helper_refuses_a_selector_too_weak_for_a_streamed_softmax(monkeypatch) -> None:
    case = vb.selector_case(B, 600, HEADS, seed=5)
    assert 600 * 2048 * 2.718281828459045 ** (-2 * case["gap"]) < sb.RESIDUE
    # vit_bounds' own minimum gap of 16 is enough for 224 keys and not for 600: 600 * 2048 * e^-32 = 1.6e-8 > 2^-26
    monkeypatch.setattr(vb, "selector_case", lambda *a, **k: {**case, "gap": vb.MIN_GAP})
    with pytest.raises(ValueError, match="weak selector for a streamed softmax"):
        sb.stream_selector_case(B, 600, HEADS)


@pytest.mark.parametrize("scale", [1.5, 0.25])
@pytest.mark.parametrize("t", sb.bound_lengths(KC))
def test_restatement_is_within_the_bound_on_random_operands(t: int, scale: float) -> None:
    qkv = vb.random_case(B, t, HEADS, scale, seed=3000 + t)  # the GPU test's operands
    want, bound = sb.stream_reference(qkv, HEADS, KC)
    ratio = mb.assert_within_bound(sb.stream_restated(qkv, HEADS, KC), want, bound, f"T = {t}, scale {scale}")
    print(f"stream T = {t}, scale {scale}: restatement uses {ratio:.3f} of the bound")
    want0, bound0 = vb.attention_reference(qkv, HEADS)
    assert torch.equal(want, want0)  # the same float64 product
    print(f"  stream bound / the bound for 224 keys: at most {float((bound / bound0).max()):.4f}")


@pytest.mark.parametrize("falling", [False, True], ids=["rising", "falling"])
@pytest.mark.parametrize("t", sb.seam_lengths(KC))
def test_restatement_is_within_the_bound_on_monotone_scores(t: int, falling: bool) -> None:
    qkv = sb.rising_case(B, t, HEADS, seed=4000 + t, falling=falling)
    want, bound = sb.stream_reference(qkv, HEADS, KC)
    ratio = mb.assert_within_bound(sb.stream_restated(qkv, HEADS, KC), want, bound, f"T = {t}")
    print(f"{'falling' if falling else 'rising'} T = {t}: restatement uses {ratio:.3f} of the bound")


@pytest.mark.parametrize("t", [785, 1025])
def test_long_random_cases_pass_the_first_order_check(t: int) -> None:
    for scale in (1.5, 0.25):
        vb.attention_reference(vb.random_case(B, t, HEADS, scale, seed=3000 + t), HEADS)


@pytest.mark.parametrize("t", sb.seam_lengths(KC))
def test_missing_rescales_leave_the_bound(t: int) -> None:
    qkv = sb.rising_case(B, t, HEADS, seed=4000 + t)
    want, bound = sb.stream_reference(qkv, HEADS, KC)
    last = sb.chunks_of(t, KC) - 1
    # O not rescaled when chunk c arrives.  The weights rise by e^4 .. e^8 over the sequence, so what O holds before
    # the last two seams carries a visible share of the result; a seam far from the end does not at T = 785
    for c in sorted({max(1, last - 1), last}):
        rows = _outside_rows(sb.stream_restated(qkv, HEADS, KC, skip_o_rescale=c), want, bound)
        assert rows.double().mean() >= 0.9, (c, float(rows.double().mean()))
    rows = _outside_rows(sb.stream_restated(qkv, HEADS, KC, skip_l_rescale=True), want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())
    # the falling twin never rescales: the same faults are invisible there, which is why both are run
    twin = sb.rising_case(B, t, HEADS, seed=4000 + t, falling=True)
    assert torch.equal(sb.stream_restated(twin, HEADS, KC, skip_o_rescale=1, skip_l_rescale=True),
                       sb.stream_restated(twin, HEADS, KC))


def test_a_dropped_chunk_breaks_the_selector_and_leaves_the_bound() -> None:
    t = 2 * KC + 1
    c = sb.stream_selector_case(B, t, HEADS)
    for drop in range(sb.chunks_of(t, KC)):
        assert not torch.equal(sb.stream_restated(c["qkv"], HEADS, KC, drop_chunk=drop), c["want"]), drop
    qkv = vb.random_case(B, 785, HEADS, 0.25, seed=3000 + 785)
    want, bound = sb.stream_reference(qkv, HEADS, KC)
    rows = _outside_rows(sb.stream_restated(qkv, HEADS, KC, drop_chunk=3), want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())


def test_an_admitted_padded_key_breaks_the_masked_selector() -> None:
    t = 2 * KC + 1
    c = sb.stream_selector_case(B, t, HEADS, masked=True)
    got = sb.stream_restated(c["qkv"], HEADS, KC, extra_zero_keys=1)
    assert float(got.abs().max()) == 0.0  # the padded key scores 0 against -40 and takes all the weight
    u = vb.uniform_case(B, t, HEADS, seed=2000 + t)
    rows = _outside_rows(sb.stream_restated(u["qkv"], HEADS, KC, extra_zero_keys=1), u["want"], u["bound"])
    assert bool(rows.all())  # the divisor is T + 1
    mb.assert_within_bound(sb.stream_restated(u["qkv"], HEADS, KC), u["want"], u["bound"], "uniform")
