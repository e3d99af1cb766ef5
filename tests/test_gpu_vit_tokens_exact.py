"""The patch-token head in its LayerNorm form (isc_vit_tokens_out, isc_vit_tokens_out_skip: every instantiation, tails,
whole and partial tiles) and the plain bicubic position resampling (isc_vit_pos_resample) against references that need
no measured tolerance: the derived element-wise bounds and exact cases of tests/vit_token_bounds.py (whose docstring
holds every derivation; tests/test_vit_token_bounds_host.py checks the references on the CPU) and the bits of the
kernels whose arithmetic csrc/vit_tokens.hip says it repeats (isc_layernorm, isc_tokens_to_map).  The conventions are
those of tests/test_gpu_vit_exact.py: every call goes through the C ABI, outputs are prefilled with NaN with a sentinel
behind them, inputs are compared bit for bit after the call, every assertion is `torch.equal` (on the int32 view where
"bit for bit" is claimed) or `matmul_bound.assert_within_bound`, and the error / bound ratios printed here are
information, not thresholds.

Every LayerNorm family runs at eps = 1e-6 and 1e-5; the rows of `small` are the ones on which a kernel that ignores
its eps argument leaves the bound (isc_layernorm and isc_text_pool_layernorm receive them here too, at both values)."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402
import vit_token_bounds as tb  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0
WORST: dict[str, float] = {}


def _note(family: str, ratio: float) -> None:
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"{family}: error / bound = {ratio:.3f} (worst so far {WORST[family]:.3f})")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ======================================================================================================= the head
def _head(device, entry: str, tokens: torch.Tensor, skip: int, gd, bd, eps: float, normalize: bool,
          l2_eps: float = tb.L2_EPS) -> torch.Tensor:
    """One call of isc_vit_tokens_out_skip (`entry` = "skip") or isc_vit_tokens_out ("plain", skip = 1) on `tokens`
    [B, T, D] (CPU, NaN in the rows in front of the patches); returns the map [B, D, T - skip] (CPU)."""
    from imagescry_amd import _lib

    b, t, d = tokens.shape
    cells = t - skip
    td = tokens.to(device)
    flat = torch.full((b * d * cells + 4,), NAN, dtype=torch.float32, device=device)
    flat[b * d * cells :] = SENTINEL
    lib, s = _lib.load(), _lib.stream_handle(device)
    tail = (d, gd.data_ptr(), bd.data_ptr(), eps, int(normalize), l2_eps, flat.data_ptr(), s)
    if entry == "skip":
        st = lib.isc_vit_tokens_out_skip(td.data_ptr(), b, t, skip, *tail)
    else:
        assert skip == 1
        st = lib.isc_vit_tokens_out(td.data_ptr(), b, t, *tail)
    _lib.check(st, "isc_vit_tokens_out_skip")
    out = flat.cpu()
    assert torch.equal(out[b * d * cells :], torch.full((4,), SENTINEL)), "memory behind the map was written"
    assert _same_bits(td.cpu(), tokens), "the tokens were written"
    return out[: b * d * cells].view(b, d, cells)


def _layernorm_rows(device, tokens: torch.Tensor, gd, bd, eps: float) -> torch.Tensor:
    """isc_layernorm (float32 output) of every row of `tokens` [B, T, D]; returns the DEVICE tensor [B, T, D] (the rows
    in front of the patches hold NaN in, NaN out)."""
    from imagescry_amd import _lib

    b, t, d = tokens.shape
    rows = b * t
    xd = tokens.to(device)
    out = torch.full((rows + 1, d), NAN, dtype=torch.float32, device=device)
    out[rows] = SENTINEL
    st = _lib.load().isc_layernorm(xd.data_ptr(), rows, d, d, gd.data_ptr(), bd.data_ptr(), eps, out.data_ptr(), _lib.ISC_F32,
                                   d, 0, _lib.stream_handle(device))
    _lib.check(st, "isc_layernorm")
    assert torch.equal(out[rows].cpu(), torch.full((d,), SENTINEL)), "the row behind the output was written"
    assert _same_bits(xd.cpu(), tokens)
    return out[:rows].view(b, t, d)


def _rows_to_map(device, rows: torch.Tensor, skip: int, l2_eps: float = tb.L2_EPS) -> torch.Tensor:
    """isc_tokens_to_map(normalize = 1) of the DEVICE rows [B, T, D]; returns the map [B, D, T - skip] (CPU)."""
    from imagescry_amd import _lib

    b, t, d = rows.shape
    cells = t - skip
    before = rows.clone()
    flat = torch.full((b * d * cells + 4,), NAN, dtype=torch.float32, device=device)
    flat[b * d * cells :] = SENTINEL
    st = _lib.load().isc_tokens_to_map(rows.data_ptr(), b, t, skip, d, 1, l2_eps, flat.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_tokens_to_map")
    out = flat.cpu()
    assert torch.equal(out[b * d * cells :], torch.full((4,), SENTINEL)), "memory behind the map was written"
    assert _same_bits(rows.cpu(), before.cpu())
    return out[: b * d * cells].view(b, d, cells)


def _l2norm_channels(device, plain: torch.Tensor) -> torch.Tensor:
    """isc_l2norm_channels of the map [B, D, cells] (CPU in, CPU out): the kernel phase 2 says it repeats."""
    from imagescry_amd import _lib

    b, d, cells = plain.shape
    xd = plain.contiguous().to(device)
    flat = torch.full((b * d * cells + 4,), NAN, dtype=torch.float32, device=device)
    flat[b * d * cells :] = SENTINEL
    st = _lib.load().isc_l2norm_channels(xd.data_ptr(), b, d, cells, tb.L2_EPS, flat.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_l2norm_channels")
    out = flat.cpu()
    assert torch.equal(out[b * d * cells :], torch.full((4,), SENTINEL)) and _same_bits(xd.cpu(), plain)
    return out[: b * d * cells].view(b, d, cells)


@functools.lru_cache(maxsize=1)
def _head_case(d: int, family: str) -> dict:
    return tb.head_case(d, family, seed=d)  # the host test's operands


@functools.lru_cache(maxsize=1)
def _head_reference(d: int, family: str, eps: float) -> dict:
    c = _head_case(d, family)
    return tb.head_reference(c["x"], c["gamma"], c["beta"], eps)


@pytest.mark.parametrize("eps", tb.HEAD_EPS)
@pytest.mark.parametrize("family", tb.HEAD_FAMILIES)
@pytest.mark.parametrize("d", tb.HEAD_D)
def test_head_layernorm_form(device, d, family, eps):
    """Per (D, family, eps) every (B, skip, cells) of the issue's product: a. the un-normalised map within the LayerNorm
    bound; b. its bits those of isc_layernorm; c. the normalised map's bits those of isc_tokens_to_map(normalize = 1) on
    isc_layernorm's rows, and those of isc_l2norm_channels on the un-normalised map; d. the normalised map within the
    composed bound; e. `constant-exact` cells EQUAL beta; f. isc_vit_tokens_out is isc_vit_tokens_out_skip(skip = 1)."""
    c = _head_case(d, family)
    ref = _head_reference(d, family, eps)
    gd, bd = c["gamma"].to(device), c["beta"].to(device)
    worst_a = worst_d = 0.0
    for b in tb.HEAD_BATCHES:
        for skip in tb.HEAD_SKIPS:
            for cells in tb.HEAD_CELLS:
                what = f"{family}, D = {d}, eps = {eps}, B = {b}, skip = {skip}, {cells} cells"
                tokens = tb.head_tokens(c["x"], b, skip, cells)
                plain = _head(device, "skip", tokens, skip, gd, bd, eps, False)
                normed = _head(device, "skip", tokens, skip, gd, bd, eps, True)

                def cut(name: str) -> torch.Tensor:
                    return ref[name][:b, :cells].transpose(1, 2).contiguous()

                worst_a = max(worst_a, mb.assert_within_bound(plain, cut("ln"), cut("ln_bound"), "a. " + what))  # a
                rows = _layernorm_rows(device, tokens, gd, bd, eps)
                assert _same_bits(plain, rows[:, skip:].transpose(1, 2).cpu()), "b. " + what  # b
                assert _same_bits(normed, _rows_to_map(device, rows, skip)), "c. " + what  # c
                if cells > 1:  # and the spatial L2-norm kernel itself (one cell: it sums a lone row in another order)
                    assert _same_bits(normed, _l2norm_channels(device, plain)), "c. isc_l2norm_channels, " + what
                worst_d = max(worst_d, mb.assert_within_bound(normed, cut("map"), cut("map_bound"), "d. " + what))  # d
                if family == "constant-exact":  # e
                    assert torch.equal(plain, c["beta"][None, :, None].expand(b, d, cells)), "e. " + what
                if skip == 1:  # f
                    assert _same_bits(_head(device, "plain", tokens, 1, gd, bd, eps, False), plain), "f. " + what
                    assert _same_bits(_head(device, "plain", tokens, 1, gd, bd, eps, True), normed), "f. " + what
    _note(f"head {family} un-normalised", worst_a)
    _note(f"head {family} normalised", worst_d)


@pytest.mark.parametrize("d", [4, 260, 768, 1020])
def test_head_clamps_the_norm_at_l2_eps(device, d):
    """l2_eps at the median norm of the cells: half of them are divided by their norm, half by l2_eps (max, not a sum)."""
    c = _head_case(d, "randn")
    b, skip, cells = 3, 1, 33
    x = c["x"][:b, :cells]
    ln, ln_bound = vb.layernorm_reference(x.reshape(-1, d), c["gamma"], c["beta"], 1e-6)
    norms = torch.linalg.vector_norm(ln, dim=1)
    l2_eps = float(norms.median().float())
    assert 0.3 < float((norms > l2_eps).double().mean()) < 0.7
    want, bound = tb.l2_compose(ln, ln_bound, l2_eps)
    want, bound = (z.reshape(b, cells, d).transpose(1, 2).contiguous() for z in (want, bound))
    gd, bd = c["gamma"].to(device), c["beta"].to(device)
    tokens = tb.head_tokens(c["x"], b, skip, cells)
    got = _head(device, "skip", tokens, skip, gd, bd, 1e-6, True, l2_eps)
    _note("head l2_eps at the median norm", mb.assert_within_bound(got, want, bound, f"D = {d}, l2_eps = {l2_eps}"))
    rows = _layernorm_rows(device, tokens, gd, bd, 1e-6)
    assert _same_bits(got, _rows_to_map(device, rows, skip, l2_eps))
    assert _same_bits(got, _head(device, "plain", tokens, 1, gd, bd, 1e-6, True, l2_eps))


# ============================================================================ eps in the other LayerNorm kernels
@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "f16"])
@pytest.mark.parametrize("eps", tb.HEAD_EPS)
@pytest.mark.parametrize("d", [4, 252, 512, 768, 1024, 2048])  # NV = 1, 1, 2, 3, 4, 8
def test_layernorm_honours_eps_on_small_rows(device, d, eps, out_f32):
    from imagescry_amd import _lib

    c = vb.layernorm_case(5, d, "small", seed=d)
    xd, gd, bd = c["x"].to(device), c["gamma"].to(device), c["beta"].to(device)
    dtype = torch.float32 if out_f32 else torch.float16
    out = torch.full((6, d), NAN, dtype=dtype, device=device)
    out[5] = SENTINEL
    st = _lib.load().isc_layernorm(xd.data_ptr(), 5, d, d, gd.data_ptr(), bd.data_ptr(), eps, out.data_ptr(),
                                   _lib.ISC_F32 if out_f32 else _lib.ISC_F16, d, 0, _lib.stream_handle(device))
    _lib.check(st, "isc_layernorm")
    got = out.cpu()
    assert torch.equal(got[5], torch.full((d,), SENTINEL, dtype=dtype)) and torch.equal(xd.cpu(), c["x"])
    want, bound = vb.layernorm_reference(c["x"], c["gamma"], c["beta"], eps, out_f16=not out_f32)
    _note(f"LayerNorm small eps {eps} {'f32' if out_f32 else 'f16'}", mb.assert_within_bound(got[:5], want, bound, f"small, D = {d}, eps = {eps}"))


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "f16"])
@pytest.mark.parametrize("eps", tb.HEAD_EPS)
@pytest.mark.parametrize("d", [128, 512, 768, 1024, 2048])  # 1, 2, 3, 4 and 8 vectors per lane
def test_text_pool_layernorm_honours_eps_on_small_rows(device, d, eps, out_f32):
    from imagescry_amd import _lib

    b, t, eos = 5, 3, 900
    c = vb.layernorm_case(b * t, d, "small", seed=d + 1)
    tokens = c["x"].reshape(b, t, d)
    at = torch.tensor([0, 1, 2, 1, 0])
    ids = torch.zeros(b, t, dtype=torch.int64)
    ids[torch.arange(b), at] = eos
    td, idd, gd, bd = tokens.to(device), ids.to(device), c["gamma"].to(device), c["beta"].to(device)
    dtype = torch.float32 if out_f32 else torch.float16
    out = torch.full((b + 1, d), NAN, dtype=dtype, device=device)
    out[b] = SENTINEL
    st = _lib.load().isc_text_pool_layernorm(td.data_ptr(), idd.data_ptr(), b, t, d, eos, gd.data_ptr(), bd.data_ptr(), eps,
                                             out.data_ptr(), _lib.ISC_F32 if out_f32 else _lib.ISC_F16, 0,
                                             _lib.stream_handle(device))
    _lib.check(st, "isc_text_pool_layernorm")
    got = out.cpu()
    assert torch.equal(got[b], torch.full((d,), SENTINEL, dtype=dtype)) and torch.equal(td.cpu(), tokens)
    want, bound = vb.layernorm_reference(tokens[torch.arange(b), at], c["gamma"], c["beta"], eps, out_f16=not out_f32)
    _note(f"pool LayerNorm small eps {eps} {'f32' if out_f32 else 'f16'}", mb.assert_within_bound(got[:b], want, bound, f"small, D = {d}, eps = {eps}"))


# ============================================================================================ isc_vit_pos_resample
def _resample(device, pos: torch.Tensor, g: int, h: int, w: int) -> torch.Tensor:
    from imagescry_amd import _lib

    d = pos.shape[1]
    pd = pos.to(device)
    out = torch.full((2 + h * w, d), NAN, dtype=torch.float32, device=device)
    out[1 + h * w] = SENTINEL
    st = _lib.load().isc_vit_pos_resample(pd.data_ptr(), g, h, w, d, out.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_vit_pos_resample")
    got = out.cpu()
    assert torch.equal(got[1 + h * w], torch.full((d,), SENTINEL)), "the row behind the table was written"
    assert _same_bits(pd.cpu(), pos)
    assert _same_bits(got[0], pos[0])  # the class row is copied
    return got[: 1 + h * w]


@pytest.mark.parametrize("g,h,w", tb.EXACT_GRIDS)
def test_pos_resample_equals_the_exact_cases(device, g, h, w):
    c = tb.exact_resample_case(g, h, w, 8, seed=g + h + w)  # the host test's case; asserts its own exact range
    assert torch.equal(_resample(device, c["pos"], g, h, w), c["want"])


@pytest.mark.parametrize("g,d", [(14, 768), (5, 4), (1, 4)])
def test_pos_resample_native_grid_is_the_table(device, g, d):
    pos = tb.resample_table(g, d, seed=3)
    assert _same_bits(_resample(device, pos, g, g, g), pos)  # weights (0, 1, 0, 0)


@pytest.mark.parametrize("d", tb.RESAMPLE_D)
@pytest.mark.parametrize("g,h,w", tb.RESAMPLE_GRIDS)
def test_pos_resample_is_within_the_derived_bound(device, g, h, w, d):
    pos = tb.resample_table(g, d, seed=g * 100 + h * 10 + w)  # the host test's table
    want, bound = tb.resample_reference(pos, g, h, w)
    got = _resample(device, pos, g, h, w)
    ratio = mb.assert_within_bound(got, want, bound, f"{g} -> {h} x {w}, D = {d}")
    err = float((got.double() - want).abs().max()) / (tb.U * float(pos[1:].abs().max()))
    print(f"pos_resample {g} -> {h} x {w}, D = {d}: max|err| = {err:.1f} u max|pos|")
    _note("pos_resample", ratio)
