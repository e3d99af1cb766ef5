"""isc_attention_f16_stream through the C ABI against references that need no measured tolerance: exact gathers
(selector operands), the mean over exactly T keys (uniform operands) and the derived element-wise bound of
tests/attention_stream_bounds.py (random, rising and falling operands; its docstring holds every derivation and
tests/test_attention_stream_host.py checks the references on the CPU).  As in tests/test_gpu_vit_exact.py every
assertion is `torch.equal` or `matmul_bound.assert_within_bound`, the printed error / bound ratios are information, the
outputs are prefilled with NaN, the padding rows of packed operands hold NaN and memory the kernel must not write holds
a sentinel.  The sequence lengths follow the kernel's own constants (isc_attention_stream_geometry)."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import attention_stream_bounds as sb  # noqa: E402
import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0
HEADS = 3
B = 2
QB, KC = sb.geometry()
LENGTHS = sb.stream_lengths(QB, KC)
RAGGED = [t for t in LENGTHS if t % 16]
SHORT = [t for t in LENGTHS if t <= 224]
LAYOUTS = pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
WORST: dict[str, float] = {}


def _note(family: str, ratio: float) -> None:
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"{family}: error / bound = {ratio:.3f} (worst so far {WORST[family]:.3f})")


def _run(device, qkv: torch.Tensor, pk: bool, entry: str = "isc_attention_f16_stream") -> torch.Tensor:
    from imagescry_amd import _lib

    b, t, _ = qkv.shape
    d = HEADS * 64
    rows = b * t
    if pk:  # NaN in the padding rows of the qkv tile, a sentinel in those of the output
        qd = vb.pack_padded(qkv.reshape(rows, 3 * d), NAN).to(device)
        init = torch.full(((rows + 255) // 256 * 256, d), NAN, dtype=torch.float16)
        init[rows:] = SENTINEL
        out = vb.pack_padded(init, SENTINEL).to(device)
    else:
        qd = qkv.to(device)
        out = torch.full((rows + 1, d), NAN, dtype=torch.float16, device=device)
        out[rows] = SENTINEL
    st = getattr(_lib.load(), entry)(qd.data_ptr(), b, t, HEADS, 64, out.data_ptr(), int(pk), _lib.stream_handle(device))
    _lib.check(st, entry)
    full = vb.unpack_all(out.cpu(), rows, d) if pk else out.cpu()
    assert torch.equal(full[rows:], torch.full_like(full[rows:], SENTINEL)), "rows behind the output were written"
    return full[:rows].view(b, t, d)


@functools.lru_cache(maxsize=None)
def _selector(t: int, masked: bool) -> dict:
    return sb.stream_selector_case(B, t, HEADS, masked=masked)


@LAYOUTS
@pytest.mark.parametrize("t", LENGTHS)
def test_selector_equals_the_gather(device, t, pk):
    c = _selector(t, False)
    assert torch.equal(_run(device, c["qkv"], pk), c["want"])


@LAYOUTS
@pytest.mark.parametrize("t", RAGGED)
def test_masked_selector_equals_the_gather(device, t, pk):
    """The chosen key scores -40: a zero-filled padded key that escapes the mask scores 0 and turns the row to zeros."""
    c = _selector(t, True)
    assert torch.equal(_run(device, c["qkv"], pk), c["want"])


@LAYOUTS
@pytest.mark.parametrize("t", SHORT)
def test_both_kernels_equal_the_gather_up_to_224(device, t, pk):
    c = _selector(t, False)
    assert torch.equal(_run(device, c["qkv"], pk, "isc_attention_f16"), c["want"])
    assert torch.equal(_run(device, c["qkv"], pk), c["want"])


@functools.lru_cache(maxsize=None)
def _uniform(t: int) -> dict:
    assert t * 2048 < 2**24  # the sum of the values stays an exact float32 integer: vit_bounds' bound holds as it stands
    return vb.uniform_case(B, t, HEADS, seed=2000 + t)


@LAYOUTS
@pytest.mark.parametrize("t", LENGTHS)
def test_uniform_is_the_mean_over_exactly_t_keys(device, t, pk):
    c = _uniform(t)
    got = _run(device, c["qkv"], pk)
    _note("stream uniform", mb.assert_within_bound(got, c["want"], c["bound"], f"uniform T = {t}"))


@functools.lru_cache(maxsize=None)
def _random(t: int, scale: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    qkv = vb.random_case(B, t, HEADS, scale, seed=3000 + t)
    return (qkv, *sb.stream_reference(qkv, HEADS, KC))


@LAYOUTS
@pytest.mark.parametrize("scale", [1.5, 0.25], ids=["peaked", "flat"])
@pytest.mark.parametrize("t", sb.bound_lengths(KC))
def test_random_is_within_the_derived_bound(device, t, scale, pk):
    qkv, want, bound = _random(t, scale)
    got = _run(device, qkv, pk)
    name = f"stream randn * {scale}"
    _note(name, mb.assert_within_bound(got, want, bound, f"{name}, T = {t}"))


@functools.lru_cache(maxsize=None)
def _monotone(t: int, falling: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    qkv = sb.rising_case(B, t, HEADS, seed=4000 + t, falling=falling)
    return (qkv, *sb.stream_reference(qkv, HEADS, KC))


@LAYOUTS
@pytest.mark.parametrize("falling", [False, True], ids=["rising", "falling"])
@pytest.mark.parametrize("t", sb.seam_lengths(KC))
def test_monotone_scores_are_within_the_derived_bound(device, t, falling, pk):
    """Rising: every chunk raises the maximum and rescales.  Falling: the maximum is key 0 and no chunk does."""
    qkv, want, bound = _monotone(t, falling)
    got = _run(device, qkv, pk)
    name = "stream falling" if falling else "stream rising"
    _note(name, mb.assert_within_bound(got, want, bound, f"{name}, T = {t}"))


@LAYOUTS
def test_offsets_past_2_to_the_31_elements(device, pk):
    """3700 images of 1025 tokens: 2.18e9 qkv elements, 4.4 GB -- past a 32-bit element index and a 32-bit byte offset.
    The batch is four images repeated, so every group of four must give the bits of the four run alone."""
    from imagescry_amd import _lib, vit

    t, reps, d = 1025, 925, HEADS * 64
    b = 4 * reps
    assert b * t * 3 * d > 2**31 and b * t < 2**31
    small = (torch.randn(4, t, 3 * d, generator=vb.gen(77)) * 0.5).half()
    want = _run(device, small, pk)
    big = small.to(device).repeat(reps, 1, 1)
    rows = b * t
    if pk:
        qd = vit.pack_rows(big.view(rows, 3 * d))
        del big
        out = torch.zeros(vit.packed_elems(rows, d), dtype=torch.float16, device=device)
    else:
        qd = big
        out = torch.zeros((rows, d), dtype=torch.float16, device=device)
    st = _lib.load().isc_attention_f16_stream(qd.data_ptr(), b, t, HEADS, 64, out.data_ptr(), int(pk), _lib.stream_handle(device))
    _lib.check(st, "isc_attention_f16_stream")
    got = (vit.unpack_rows(out, rows, d) if pk else out).view(reps, 4, t, d)
    wd = want.to(device)
    assert torch.equal(got[0], wd) and torch.equal(got[reps // 2], wd) and torch.equal(got[-1], wd)
    assert bool((got == wd).all())


def test_other_head_sizes_are_unsupported(device):
    from imagescry_amd import _lib

    qkv = torch.zeros(2 * 17 * 3 * 96, dtype=torch.float16, device=device)
    out = torch.zeros(2 * 17 * 96, dtype=torch.float16, device=device)
    lib, s = _lib.load(), _lib.stream_handle(device)
    assert lib.isc_attention_f16_stream(qkv.data_ptr(), 2, 17, 3, 32, out.data_ptr(), 0, s) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_attention_f16_stream(qkv.data_ptr() + 2, 2, 17, 1, 64, out.data_ptr(), 0, s) == _lib.ISC_ERR_ALIGNMENT
    assert lib.isc_attention_f16_stream(None, 2, 17, 1, 64, out.data_ptr(), 0, s) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_attention_f16_stream(qkv.data_ptr(), 2, 0, 1, 64, out.data_ptr(), 0, s) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_attention_f16_stream(qkv.data_ptr(), 2**20, 2**11, 1, 64, out.data_ptr(), 0, s) == _lib.ISC_ERR_UNSUPPORTED
    assert not out.any()  # nothing was launched


def test_a_captured_call_replays_on_new_operands(device):
    """One launch, no workspace, no host synchronisation: a graph of the call gives an eager call's bits."""
    from imagescry_amd import _lib

    t, d = 2 * KC + 1, HEADS * 64
    lib = _lib.load()
    first, second = _selector(t, False), _random(t, 1.5)[0]
    qd = first["qkv"].to(device)
    out = torch.zeros((B * t, d), dtype=torch.float16, device=device)

    def call() -> None:
        _lib.check(lib.isc_attention_f16_stream(qd.data_ptr(), B, t, HEADS, 64, out.data_ptr(), 0,
                                                _lib.stream_handle(device)), "isc_attention_f16_stream")

    call()  # eager warm-up, as in tests/test_gpu_graph.py
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(B, t, d), first["want"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    torch.cuda.synchronize()
    qd.copy_(second.to(device))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(B, t, d), _run(device, second, False))
