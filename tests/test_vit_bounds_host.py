"""CPU checks of tests/vit_bounds.py, the references the kernel-level GPU tests of the fp16 transformer kernels rest on
(tests/test_gpu_vit_exact.py), in the manner of test_matmul_bound_host.py.

* Restatements stay inside: a float32 / fp16 torch restatement of each operation, in another order than the kernel's,
  stays inside each bound on the GPU test's own operands (the share of the bound it uses is printed).
* The selector operands return the gather exactly through that restatement, and the helper refuses a key set with two
  equal keys.
* Planted faults leave the bound: for at least 90 % of the affected rows some element falls outside.
    attention   every query's largest-weight key dropped (peaked scale); one padded key admitted with score 0 at the flat
                scale, T = 207 -- with zero-mean values the output is a mean of about 0.25 / sqrt(207), far below the
                fp16 rounding of its own magnitude sum, so these operands give the values an offset of 1: the fault
                then moves every output by 1 / 208 of itself; two adjacent value rows swapped, the two rows +8 and -8.
    LayerNorm   one 16-byte vector of x left out of a row's statistics; the neighbouring row's mean.
    GELU        the tanh approximation in place of erf on the float32 path.  It differs from the erf form by up to
                about 4.7e-4 near |v| = 2 and LEAVES the fp16 bound too on the negative side, where the values are
                small; on the positive side, where fp16 spacing near 2 is 9.8e-4, it stays inside (printed below)."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402


def _outside_rows(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """Per row (all leading axes flattened): does some element leave the bound?"""
    out = ~((got.double() - want).abs() <= bound)
    return out.reshape(-1, out.shape[-1]).any(dim=1)


# ---------------------------------------------------------------------------------------------------------- GEMM
def test_gemm_case_is_exact_in_float32_in_any_order() -> None:
    c = vb.gemm_case(129, 128, 132, seed=3, lo=-8, hi=8)
    a, w = c["a"].float(), c["w"].float()
    got = a @ w.T + c["bias"]
    assert torch.equal(got.double(), c["want"])
    parts = [a[:, i : i + 32] @ w[:, i : i + 32].T for i in range(0, 128, 32)]
    acc = c["res"].clone()
    for p in reversed(parts):
        acc = acc + p
    assert torch.equal((acc + c["bias"]).double(), c["want_res"])
    want16 = vb.round_once_f16(c["want"])
    assert bool((c["want"].abs() > 2048).any()) and not torch.equal(want16.double(), c["want"])  # the rounding is exercised
    with pytest.raises(AssertionError, match="outside fp16"):
        vb.round_once_f16(c["want"] * 64)
    with pytest.raises(AssertionError, match="rounded twice"):
        vb.round_once_f16(c["want"] + 2.0**-30)


def test_pack_padded_matches_the_library_layout() -> None:
    from imagescry_amd.vit import pack_rows, unpack_rows

    x = torch.randn(300, 128, generator=vb.gen(1)).half()
    assert torch.equal(vb.pack_padded(x, 0.0), pack_rows(x))
    p = vb.pack_padded(x, float("nan"))
    assert torch.equal(unpack_rows(p, 300, 128), x)
    full = vb.unpack_all(p, 300, 128)
    assert full.shape == (512, 128) and torch.equal(full[:300], x) and bool(full[300:].isnan().all())


def _gelu_operands() -> torch.Tensor:
    c = vb.gemm_case(129, 128, 132, seed=21, a_quantum=0.25, w_quantum=0.125, bias_top=32, res_top=64)
    v = c["want"]
    assert float(v.min()) < -3 and float(v.max()) > 3 and float(v.abs().max()) < 12
    return v


def test_gelu_restatements_are_within_the_bound() -> None:
    v = _gelu_operands()
    want, bound = vb.gelu_bound(v, out_f16=False)
    r1 = mb.assert_within_bound(vb.gelu_restated_f32(v), want, bound, "erf restatement")
    r2 = mb.assert_within_bound(vb.gelu_polynomial_f32(v), want, bound, "polynomial restatement")
    want16, bound16 = vb.gelu_bound(v, out_f16=True)
    r3 = mb.assert_within_bound(vb.gelu_polynomial_f32(v).half(), want16, bound16, "polynomial restatement, fp16")
    print(f"GELU: erf restatement {r1:.3f}, polynomial restatement {r2:.3f}, fp16 {r3:.3f} of the bound")
    assert torch.equal(want, want16)


def test_tanh_gelu_leaves_the_float32_bound() -> None:
    v = _gelu_operands()
    want, bound = vb.gelu_bound(v, out_f16=False)
    got = vb.gelu_restated_f32(v, tanh=True)
    rows = _outside_rows(got, want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())
    share = float((~((got.double() - want).abs() <= bound)).double().mean())
    _, bound16 = vb.gelu_bound(v, out_f16=True)
    out16 = ~((got.half().double() - want).abs() <= bound16)
    print(f"tanh GELU: {share:.2f} of the float32 elements outside; fp16: {float(out16.double().mean()):.2f} outside, "
          f"{float(out16[v > 1].double().mean()):.2f} of those with v > 1")
    assert share > 0.5


# ----------------------------------------------------------------------------------------------------- attention
HEADS = 3
SELECTOR_T = (1, 15, 16, 17, 31, 33, 192, 193, 197, 207, 208, 209, 223, 224)


@pytest.mark.parametrize("masked", [False, True])
def test_selector_restatement_returns_the_gather(masked: bool) -> None:
    for t in SELECTOR_T:
        if masked and t % 16 == 0:
            continue
        c = vb.selector_case(2, t, HEADS, seed=1000 + t + (7 if masked else 0), masked=masked)  # the GPU test's operands
        assert c["gap"] >= vb.MIN_GAP
        assert c["perm"][0] == t - 1 and c["perm"][-1] == 0
        assert torch.equal(vb.attention_restated(c["qkv"], HEADS), c["want"]), t
        if t > 1:  # and it is a gather of DIFFERENT rows: the identity would not pass
            assert not torch.equal(c["want"], c["qkv"][..., 2 * HEADS * 64 :])


def test_masked_selector_fails_on_an_unmasked_padded_key() -> None:
    c = vb.selector_case(2, 207, HEADS, seed=9, masked=True)
    got = vb.attention_restated(c["qkv"], HEADS, extra_zero_keys=1)
    assert float(got.abs().max()) == 0.0  # the padded key took all the weight
    plain = vb.selector_case(2, 207, HEADS, seed=9)
    assert torch.equal(vb.attention_restated(plain["qkv"], HEADS, extra_zero_keys=1), plain["want"])  # (a) cannot see it


def test_the_helper_refuses_weak_selectors() -> None:
    g = vb.gen(4)
    keys = torch.randint(0, 2, (2, 40, HEADS, 64), generator=g) * 2 - 1
    values = torch.randint(-2048, 2049, (2, 40, HEADS, 64), generator=g)
    perm = torch.randperm(40, generator=g)
    vb.selector_keys_to_case(keys, values, perm, masked=False)
    keys[1, 17, 2] = keys[1, 3, 2]  # two equal keys in ONE (image, head)
    assert vb.key_gap(keys) == 0
    with pytest.raises(ValueError, match="weak selector"):
        vb.selector_keys_to_case(keys, values, perm, masked=False)
    keys[1, 17, 2, :6] *= -1  # six dimensions apart: dot product 64 - 12, just under the required gap of 16
    assert vb.key_gap(keys) == 12
    with pytest.raises(ValueError, match="weak selector"):
        vb.selector_keys_to_case(keys, values, perm, masked=False)


@pytest.mark.parametrize("t", [1, 17, 193, 207, 224])
def test_uniform_restatement_is_within_the_bound(t: int) -> None:
    c = vb.uniform_case(2, t, HEADS, seed=2000 + t)  # the GPU test's operands
    ratio = mb.assert_within_bound(vb.attention_restated(c["qkv"], HEADS), c["want"], c["bound"], f"uniform, T = {t}")
    print(f"uniform T = {t}: restatement uses {ratio:.3f} of the bound")
    if t > 1:
        got = vb.attention_restated(c["qkv"], HEADS, extra_zero_keys=1)  # the divisor is T + 1
        rows = _outside_rows(got, c["want"], c["bound"])
        assert bool(rows.all())


@pytest.mark.parametrize("scale", [1.5, 0.25])
@pytest.mark.parametrize("t", [193, 197, 208, 224])
def test_attention_restatement_is_within_the_bound(t: int, scale: float) -> None:
    qkv = vb.random_case(2, t, HEADS, scale, seed=3000 + t)  # the GPU test's operands
    want, bound = vb.attention_reference(qkv, HEADS)
    ratio = mb.assert_within_bound(vb.attention_restated(qkv, HEADS), want, bound, f"T = {t}, scale {scale}")
    print(f"attention T = {t}, scale {scale}: restatement uses {ratio:.3f} of the bound")
    # the reference is the plain float64 softmax product
    q, k, v = (z.reshape(2, t, HEADS, 64).transpose(1, 2).double() for z in qkv.split(HEADS * 64, dim=-1))
    plain = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(2, t, HEADS * 64)
    assert torch.equal(want, plain)


def test_attention_faults_leave_the_bound() -> None:
    # the largest-weight key dropped, peaked scale
    qkv = vb.random_case(2, 197, HEADS, 1.5, seed=31)
    want, bound = vb.attention_reference(qkv, HEADS)
    rows = _outside_rows(vb.attention_restated(qkv, HEADS, drop_largest=True), want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())
    # one padded key admitted with score 0, flat scale, T = 207, values offset by 1 (module docstring)
    d = HEADS * 64
    flat = vb.random_case(2, 207, HEADS, 0.25, seed=32).float()
    flat[..., 2 * d :] += 1.0
    flat = flat.half()
    want, bound = vb.attention_reference(flat, HEADS)
    mb.assert_within_bound(vb.attention_restated(flat, HEADS), want, bound, "flat, offset values")
    rows = _outside_rows(vb.attention_restated(flat, HEADS, extra_zero_keys=1), want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())
    # two adjacent value rows swapped, the rows +8 and -8
    swap = vb.random_case(2, 197, HEADS, 1.5, seed=33)
    swap[:, 100, 2 * d :] = 8.0
    swap[:, 101, 2 * d :] = -8.0
    want, bound = vb.attention_reference(swap, HEADS)
    mb.assert_within_bound(vb.attention_restated(swap, HEADS), want, bound, "swap operands")
    rows = _outside_rows(vb.attention_restated(swap, HEADS, swap_values=100), want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())


# ----------------------------------------------------------------------------------------------------- LayerNorm
LN_D = (4, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 2044, 2048)


@pytest.mark.parametrize("family", vb.LN_FAMILIES)
def test_layernorm_restatement_is_within_the_bound(family: str) -> None:
    worst = 0.0
    for d in LN_D:
        c = vb.layernorm_case(5, d, family, seed=d)
        got = vb.layernorm_restated(c["x"], c["gamma"], c["beta"])
        want, bound = vb.layernorm_reference(c["x"], c["gamma"], c["beta"])
        worst = max(worst, mb.assert_within_bound(got, want, bound, f"{family}, D = {d}"))
        want16, bound16 = vb.layernorm_reference(c["x"], c["gamma"], c["beta"], out_f16=True)
        mb.assert_within_bound(got.half(), want16, bound16, f"{family}, D = {d}, fp16")
        ref = torch.nn.functional.layer_norm(c["x"].double(), (d,), c["gamma"].double(), c["beta"].double(), vb.LN_EPS)
        assert float((ref - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))
    print(f"LayerNorm {family}: restatement uses {worst:.3f} of the bound")


@pytest.mark.parametrize("d", [252, 768, 1028, 2048])
def test_layernorm_faults_leave_the_bound(d: int) -> None:
    c = vb.layernorm_case(40, d, "randn", seed=100 + d)
    want, bound = vb.layernorm_reference(c["x"], c["gamma"], c["beta"])
    hit = []
    for row in range(40):  # one 16-byte vector left out of the statistics of `row`
        got = vb.layernorm_restated(c["x"], c["gamma"], c["beta"], skip_vector=(row, (row * 7) % (d // 4)))
        out = _outside_rows(got, want, bound)
        hit.append(bool(out[row]))
        assert not bool(out[torch.arange(40) != row].any())
    assert sum(hit) >= 36, sum(hit)
    rows = _outside_rows(vb.layernorm_restated(c["x"], c["gamma"], c["beta"], neighbour_mean=True), want, bound)
    assert rows.double().mean() >= 0.9, float(rows.double().mean())
