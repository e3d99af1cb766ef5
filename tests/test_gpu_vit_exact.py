"""isc_gemm_f16 (all three kernels), isc_attention_f16 (both forms) and isc_layernorm (every instantiation) against
references that need no measured tolerance: exact integers, exact gathers and the derived element-wise bounds of
tests/vit_bounds.py (whose docstring holds every derivation; tests/test_vit_bounds_host.py checks the references on the
CPU).  Every assertion is `torch.equal` or `matmul_bound.assert_within_bound`; the error / bound ratios printed here
are information, not thresholds.  All calls go through the C ABI, outputs are prefilled with NaN, the padding rows of
packed operands hold NaN and memory the kernels must not write holds a sentinel."""

from __future__ import annotations

import ctypes
import functools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0
WORST: dict[str, float] = {}


def _note(family: str, ratio: float) -> None:
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"{family}: error / bound = {ratio:.3f} (worst so far {WORST[family]:.3f})")


# ================================================================================================ isc_gemm_f16
@functools.lru_cache(maxsize=1)
def _gemm_case(m: int, k: int, n: int, gelu: bool = False) -> dict:
    if gelu:  # quanta 2^-2 and 2^-3: the pre-activation is exact and lies in about [-8, 8]
        return vb.gemm_case(m, k, n, seed=m + k + n, a_quantum=0.25, w_quantum=0.125, bias_top=32, res_top=64)
    top = 8 if k <= 192 else 4
    return vb.gemm_case(m, k, n, seed=m + k + n, lo=-top, hi=top)


def _run_gemm(device, c: dict, kernel: str, *, packed: bool, out_f32: bool, res: bool, gelu: bool = False,
              out_packed: bool | None = None) -> torch.Tensor:
    """One isc_gemm_f16 call on the operands of `c`; returns the M real output rows (CPU) after checking the guard."""
    from imagescry_amd import _lib

    a, w = c["a"], c["w"]
    m, k = a.shape
    n = w.shape[0]
    if out_packed is None:
        out_packed = packed and not out_f32 and n % 64 == 0
    flags = {"tile128": _lib.ISC_GEMM_TILE_128 if packed else 0, "tile256": _lib.ISC_GEMM_TILE_256, "stream": 0}[kernel]
    if packed:  # padding rows of the last 256-row tile are NaN: no real output row may depend on them
        flags |= _lib.ISC_GEMM_A_PACKED | _lib.ISC_GEMM_W_PACKED
        ad, wd = vb.pack_padded(a, NAN).to(device), vb.pack_padded(w, NAN).to(device)
    else:
        ad, wd = a.to(device), w.to(device)
    bd = c["bias"].to(device)
    rd = c["res"].to(device) if res else None
    dtype = torch.float32 if out_f32 else torch.float16
    if out_packed:
        flags |= _lib.ISC_GEMM_OUT_PACKED
        out = torch.full(((m + 255) // 256 * 256 * n,), NAN, dtype=dtype, device=device)
    else:  # one row of sentinel behind the M rows
        out = torch.full((m + 1, n), NAN, dtype=dtype, device=device)
        out[m] = SENTINEL
    st = _lib.load().isc_gemm_f16(ad.data_ptr(), m, k, wd.data_ptr(), n, bd.data_ptr(), _lib.ptr(rd),
                                  _lib.ISC_ACT_GELU if gelu else _lib.ISC_ACT_NONE, out.data_ptr(),
                                  _lib.ISC_F32 if out_f32 else _lib.ISC_F16, flags, _lib.stream_handle(device))
    _lib.check(st, "isc_gemm_f16")
    out = out.cpu()
    if out_packed:
        return vb.unpack_all(out, m, n)[:m]
    assert torch.equal(out[m], torch.full((n,), SENTINEL, dtype=dtype)), "the row behind the output was written"
    return out[:m]


def _assert_exact(got: torch.Tensor, c: dict, *, out_f32: bool, res: bool, must_round: bool) -> None:
    want = c["want_res"] if res else c["want"]
    if out_f32:
        want32 = want.float()
        assert torch.equal(want32.double(), want)
        assert torch.equal(got, want32)
    else:
        want16 = vb.round_once_f16(want)
        if must_round:  # the single rounding is exercised: outputs above 2048 that are no fp16 numbers
            assert bool((want.abs() > 2048).any()) and not torch.equal(want16.double(), want)
        assert torch.equal(got, want16)


EPILOGUES = [("f16", False, False), ("f16-res", False, True), ("f32", True, False), ("f32-res", True, True)]

# 128 x 128 tiles (k_gemm_f16_dma), reached row-major without a flag and packed with ISC_GEMM_TILE_128.
#   (1, 64, 4)        the smallest legal problem: one K step, one row, one 16-byte store
#   (129, 128, 132)   two token tiles and two feature tiles, both ragged: the clamped staging rows and the N guards
#   (257, 3072, 260)  48 K steps, three ragged tiles each way; band = 2 MiB / (128 * 3072 * 2) = 2 over three token tiles
#   (640, 3072, 256)  five token tiles in bands of two: the last band holds one tile (`left < band`)
TILE128_SHAPES = [(1, 64, 4), (129, 128, 132), (257, 3072, 260), (640, 3072, 256)]


@pytest.mark.parametrize("epi,out_f32,res", EPILOGUES)
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("m,k,n", TILE128_SHAPES)
def test_gemm_tile128_equals_the_integer_product(device, m, k, n, packed, epi, out_f32, res):
    c = _gemm_case(m, k, n)
    got = _run_gemm(device, c, "tile128", packed=packed, out_f32=out_f32, res=res)
    _assert_exact(got, c, out_f32=out_f32, res=res, must_round=m > 1)


# 256 x 256 tiles (k_gemm_f16_big, ISC_GEMM_TILE_256; at least three K steps, no activation).
#   (257, 192, 260)    the minimum of three K steps: prologue and drain only; two ragged tiles each way
#   (513, 3072, 256)   band = 2 MiB / (256 * 3072 * 2) = 1: three bands of one tile
#   (1300, 1024, 516)  band = 4 over six token tiles: the last band holds two (`left < band`); three feature tiles
TILE256_SHAPES = [(257, 192, 260), (513, 3072, 256), (1300, 1024, 516)]


@pytest.mark.parametrize("epi,out_f32,res", EPILOGUES)
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("m,k,n", TILE256_SHAPES)
def test_gemm_tile256_equals_the_integer_product(device, m, k, n, packed, epi, out_f32, res):
    c = _gemm_case(m, k, n)
    got = _run_gemm(device, c, "tile256", packed=packed, out_f32=out_f32, res=res)
    _assert_exact(got, c, out_f32=out_f32, res=res, must_round=True)


# The streaming kernel (k_gemm_f16_stream: packed operands, N % 256 == 0, no tile flag).  fbs = N / 256 feature blocks.
#   M = 300, K = 128, N = 256 .. 1280: `group` = 4 | 3 | 2 | 1 by divisibility of fbs -> 1, 2, 3, 4, and 1 with FIVE groups
#   N = 3072: fbs = 12, group = 4, ngroups = 3, want = 8 * (32 / 4) / 3 = 21 chunks of token tiles;
#     M = 5376: 21 tiles, one per chunk; M = 5377: 22 tiles, two per chunk, the last tile one row; M = 10753: 43
#     tiles, three per chunk, the last chunk one tile of one row
#     K = 64, 128, 192: one, two and three K steps per tile against ring depths of three (tokens) and two (weights)
STREAM_SHAPES = [(300, 128, n) for n in (256, 512, 768, 1024, 1280)] + [
    (m, k, 3072) for m in (5376, 5377, 10753) for k in (64, 128, 192)]
STREAM_EPILOGUES = [("f16-packed", False, False, True), ("f16-rowmajor", False, False, False),
                    ("f32", True, False, False), ("f32-res", True, True, False)]


@pytest.mark.parametrize("epi,out_f32,res,out_packed", STREAM_EPILOGUES)
@pytest.mark.parametrize("m,k,n", STREAM_SHAPES)
def test_gemm_stream_equals_the_integer_product(device, m, k, n, epi, out_f32, res, out_packed):
    c = _gemm_case(m, k, n)
    got = _run_gemm(device, c, "stream", packed=True, out_f32=out_f32, res=res, out_packed=out_packed)
    _assert_exact(got, c, out_f32=out_f32, res=res, must_round=True)


# GELU epilogues: the 128-tile kernel (row-major: fp16, float32, float32 + residual; packed: fp16 into the packed layout)
# and the streaming kernel (fp16, one tile per chunk and two tiles per chunk with one K step)
@pytest.mark.parametrize("kernel,m,k,n,packed,out_f32,res", [
    ("tile128", 129, 128, 132, False, False, False),
    ("tile128", 129, 128, 132, False, True, False),
    ("tile128", 129, 128, 132, False, True, True),
    ("tile128", 300, 128, 256, True, False, False),
    ("stream", 300, 128, 512, True, False, False),
    ("stream", 5377, 64, 3072, True, False, False),
])
def test_gemm_gelu_epilogue_is_within_the_derived_bound(device, kernel, m, k, n, packed, out_f32, res):
    c = _gemm_case(m, k, n, True)
    v = c["want"]  # the exact pre-activation
    assert float(v.min()) < -3 and float(v.max()) > 3
    got = _run_gemm(device, c, kernel, packed=packed, out_f32=out_f32, res=res, gelu=True)
    want, bound = vb.gelu_bound(v, out_f16=not out_f32, residual=c["res"] if res else None)
    name = f"GELU {kernel} {'f32' if out_f32 else 'f16'}"
    _note(name, mb.assert_within_bound(got, want, bound, name))
    tail = v < -3  # and the negative tail on its own
    _note(name + " tail", mb.assert_within_bound(got[tail], want[tail], bound[tail], name + " tail"))


# =========================================================================================== isc_attention_f16
HEADS = 3
ONE_SHOT_T = (1, 15, 16, 17, 31, 33, 192, 193, 197, 207, 208, 209, 223, 224)
PERSISTENT_T = (1, 17, 193, 208, 209, 224)
FORMS = [("one-shot", t) for t in ONE_SHOT_T] + [("persistent", t) for t in PERSISTENT_T]
RAGGED_FORMS = [(f, t) for f, t in FORMS if t % 16]
RANDOM_FORMS = [(f, t) for f in ("one-shot", "persistent") for t in (193, 197, 208, 224)]


@functools.lru_cache(maxsize=1)
def _cus() -> int:
    from imagescry_amd import _lib

    cus, lds = ctypes.c_int(0), ctypes.c_int(0)
    name = ctypes.create_string_buffer(64)
    _lib.check(_lib.load().isc_device_info(ctypes.byref(cus), ctypes.byref(lds), name, 64), "isc_device_info")
    return cus.value


def _images(form: str) -> int:
    """One-shot form: 2 images x 3 heads.  Persistent form: the smallest B with B * 3 >= 2 * CUs + 5 (2 * CUs + 5 itself is
    no multiple of 3 on 256 CUs): some workgroup walks three pairs and returns to the first LDS image, and the pair
    count is no multiple of the grid."""
    cus = _cus()
    b = 2 if form == "one-shot" else -(-(2 * cus + 5) // HEADS)
    total = b * HEADS
    assert (total <= cus) if form == "one-shot" else (2 * cus < total < 3 * cus and total % cus), (form, total, cus)
    return b


def _run_attention(device, qkv: torch.Tensor, pk: bool) -> torch.Tensor:
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
    st = _lib.load().isc_attention_f16(qd.data_ptr(), b, t, HEADS, 64, out.data_ptr(), int(pk), _lib.stream_handle(device))
    _lib.check(st, "isc_attention_f16")
    full = vb.unpack_all(out.cpu(), rows, d) if pk else out.cpu()
    assert torch.equal(full[rows:], torch.full_like(full[rows:], SENTINEL)), "rows behind the output were written"
    return full[:rows].view(b, t, d)


@functools.lru_cache(maxsize=1)
def _selector(b: int, t: int, masked: bool) -> dict:
    return vb.selector_case(b, t, HEADS, seed=1000 + t + (7 if masked else 0), masked=masked)


@pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("form,t", FORMS)
def test_attention_selector_equals_the_gather(device, form, t, pk):
    c = _selector(_images(form), t, False)
    assert torch.equal(_run_attention(device, c["qkv"], pk), c["want"])


@pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("form,t", RAGGED_FORMS)
def test_attention_masked_selector_equals_the_gather(device, form, t, pk):
    """The chosen key scores -40: a zero-filled padded key that escapes the mask scores 0 and turns the row to zeros."""
    c = _selector(_images(form), t, True)
    assert torch.equal(_run_attention(device, c["qkv"], pk), c["want"])


@functools.lru_cache(maxsize=1)
def _uniform(b: int, t: int) -> dict:
    return vb.uniform_case(b, t, HEADS, seed=2000 + t)


@pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("form,t", FORMS)
def test_attention_uniform_is_the_mean_over_exactly_t_keys(device, form, t, pk):
    c = _uniform(_images(form), t)
    got = _run_attention(device, c["qkv"], pk)
    _note(f"attention uniform {form}", mb.assert_within_bound(got, c["want"], c["bound"], f"uniform T = {t}"))


@functools.lru_cache(maxsize=1)
def _random(b: int, t: int, scale: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    qkv = vb.random_case(b, t, HEADS, scale, seed=3000 + t)
    return (qkv, *vb.attention_reference(qkv, HEADS))


@pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("scale", [1.5, 0.25], ids=["peaked", "flat"])
@pytest.mark.parametrize("form,t", RANDOM_FORMS)
def test_attention_random_is_within_the_derived_bound(device, form, t, scale, pk):
    qkv, want, bound = _random(_images(form), t, scale)
    got = _run_attention(device, qkv, pk)
    name = f"attention randn * {scale} {form}"
    _note(name, mb.assert_within_bound(got, want, bound, f"{name}, T = {t}"))


@pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("t", [17, 197, 209])  # the generic, the thirteen-block and the fourteen-block instantiation
def test_attention_forms_agree_bit_for_bit(device, t, pk):
    """k_attention_f16_p's header: same staging, same query-block arithmetic, bit-identical results.  The persistent
    batch goes through the persistent form, its first two images alone (6 pairs <= CUs) through the one-shot form."""
    qkv = vb.random_case(_images("persistent"), t, HEADS, 0.5, seed=4000 + t)
    assert _images("one-shot") == 2
    persistent = _run_attention(device, qkv, pk)
    one_shot = _run_attention(device, qkv[:2].contiguous(), pk)
    assert torch.equal(one_shot, persistent[:2])


# =============================================================================================== isc_layernorm
# NV = 16-byte vectors per lane = ceil(D / 256): D = 4, 252, 256 -> 1; 260, 512 -> 2; 516, 768 -> 3; 772, 1024 -> 4; 1028,
# 2044, 2048 -> the NV = 8 instantiation.  D / 4 % 64 != 0 (4, 252, 260, 516, 772, 1028, 2044) leaves the last lane row
# partly empty.
LN_D = (4, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 2044, 2048)


def _run_layernorm(device, c: dict, *, out_f32: bool, pk: bool = False, ldx: int | None = None,
                   ldy: int | None = None) -> torch.Tensor:
    from imagescry_amd import _lib

    x = c["x"]
    rows, d = x.shape
    ldx, ldy = ldx or d, ldy or d
    xs = torch.full((rows, ldx), NAN)  # NaN in the gaps between rows
    xs[:, :d] = x
    dtype = torch.float32 if out_f32 else torch.float16
    if pk:
        init = torch.full(((rows + 255) // 256 * 256, d), NAN, dtype=dtype)
        init[rows:] = SENTINEL
        out = vb.pack_padded(init, SENTINEL).to(device)
    else:
        init = torch.full((rows + 1, ldy), SENTINEL, dtype=dtype)  # a sentinel in the gaps and behind the last row
        init[:rows, :d] = NAN
        out = init.to(device)
    xd, gd, bd = xs.to(device), c["gamma"].to(device), c["beta"].to(device)
    st = _lib.load().isc_layernorm(xd.data_ptr(), rows, d, ldx, gd.data_ptr(), bd.data_ptr(), vb.LN_EPS, out.data_ptr(),
                                   _lib.ISC_F32 if out_f32 else _lib.ISC_F16, ldy, int(pk), _lib.stream_handle(device))
    _lib.check(st, "isc_layernorm")
    full = vb.unpack_all(out.cpu(), rows, d) if pk else out.cpu()
    guard = torch.ones_like(full, dtype=torch.bool)
    guard[:rows, :d] = False
    assert torch.equal(full[guard], torch.full_like(full[guard], SENTINEL)), "memory outside the rows was written"
    return full[:rows, :d]


def _check_layernorm(got: torch.Tensor, c: dict, out_f32: bool, what: str, family: str) -> None:
    want, bound = vb.layernorm_reference(c["x"], c["gamma"], c["beta"], out_f16=not out_f32)
    _note(f"LayerNorm {family} {'f32' if out_f32 else 'f16'}", mb.assert_within_bound(got, want, bound, what))


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "f16"])
@pytest.mark.parametrize("family", vb.LN_FAMILIES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("d", LN_D)
def test_layernorm_is_within_the_derived_bound(device, d, rows, family, out_f32):
    c = vb.layernorm_case(rows, d, family, seed=d + rows)
    got = _run_layernorm(device, c, out_f32=out_f32)
    _check_layernorm(got, c, out_f32, f"{family}, D = {d}, {rows} rows", family)


@pytest.mark.parametrize("family", vb.LN_FAMILIES)
def test_layernorm_packed_output_crosses_the_tile_seam(device, family):
    c = vb.layernorm_case(257, 768, family, seed=77)
    got = _run_layernorm(device, c, out_f32=False, pk=True)
    _check_layernorm(got, c, False, f"{family}, packed", family)


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "f16"])
@pytest.mark.parametrize("d,ldx,ldy", [(516, 520, 516), (516, 516, 524), (2044, 2052, 2048)])
def test_layernorm_strided_rows_and_gaps(device, d, ldx, ldy, out_f32):
    """ldx > D with NaN in the gaps of x; ldy > D with a sentinel in the gaps of y that must survive."""
    c = vb.layernorm_case(5, d, "randn", seed=d + ldx + ldy)
    got = _run_layernorm(device, c, out_f32=out_f32, ldx=ldx, ldy=ldy)
    _check_layernorm(got, c, out_f32, f"D = {d}, ldx = {ldx}, ldy = {ldy}", "randn")
