"""The CLIP backbones on the GPU: the QuickGELU GEMM epilogue (ISC_ACT_QUICK_GELU, both kernels), the causal attention
kernel (isc_attention_f16_causal), the token-embedding gather (isc_text_embed), the end-of-text pooling head
(isc_text_pool_layernorm), and `CLIPEmbedder` end to end -- both towers against the float32 torch restatements of
tests/clip_oracle.py (pinned to transformers in tests/test_clip_host.py) and text queries through `EmbeddingBank`.

Every kernel call goes through the C ABI, outputs are prefilled with NaN, the padding rows of packed operands hold NaN
and a sentinel row sits behind row-major outputs, as in tests/test_gpu_vit_exact.py.  Assertions are `torch.equal` or
`matmul_bound.assert_within_bound` against bounds derived in tests/vit_bounds.py and tests/clip_oracle.py; the printed
error / bound ratios are information.  The model: the project's bounds on unit-norm outputs (tests/test_gpu_dinov2.py),
1e-2 to the float32 oracle and 2e-3 to the oracle with fp16-rounded operands, times sqrt(768 / E), norms within 1e-5."""

from __future__ import annotations

import functools
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import clip_oracle as co  # noqa: E402
import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0
HEADS = 3


def _note(what: str, ratio: float) -> None:
    print(f"{what}: error / bound = {ratio:.3f}")


# ============================================================================================ QuickGELU epilogue
# The first and last entries of TILE128_SHAPES and STREAM_SHAPES (tests/test_gpu_vit_exact.py), a text-tower shape with
# M no multiple of 16 and N = 384 no multiple of 256, and one with M just past a 256-row tile.
# (kernel, m, k, n, packed operands, float32 output, residual, packed output)
_EPI = [(False, False), (False, True), (True, False), (True, True)]  # (float32 output, residual)
QGELU_CASES = (
    [("tile128", m, k, n, pk, f32, res, pk and not f32 and n % 64 == 0)
     for m, k, n in ((1, 64, 4), (640, 3072, 256), (77, 128, 384)) for pk in (False, True) for f32, res in _EPI]
    # the streaming kernel takes fp16 output without residual; the other epilogues of such operands run on 128-tiles
    + [("stream", m, k, n, True, False, False, out_pk)
       for m, k, n in ((300, 128, 256), (257, 768, 768), (10753, 192, 3072)) for out_pk in (True, False)]
    + [("dispatch", 257, 768, 768, True, f32, res, False) for f32, res in _EPI[1:]])


@functools.lru_cache(maxsize=1)
def _gemm_case(m: int, k: int, n: int) -> dict:
    # quanta 2^-2 and 2^-3: the pre-activation is exact (about [-8, 8] at K = 128)
    return vb.gemm_case(m, k, n, seed=m + k + n, a_quantum=0.25, w_quantum=0.125, bias_top=32, res_top=64)


def _run_gemm(device, c: dict, kernel: str, *, packed: bool, out_f32: bool, res: bool, out_packed: bool, act: int) -> torch.Tensor:
    """One isc_gemm_f16 call on the operands of `c`; the M real output rows (CPU), after checking the guard."""
    from imagescry_amd import _lib

    a, w = c["a"], c["w"]
    m, k = a.shape
    n = w.shape[0]
    flags = _lib.ISC_GEMM_TILE_128 if kernel == "tile128" and packed else 0
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
    st = _lib.load().isc_gemm_f16(ad.data_ptr(), m, k, wd.data_ptr(), n, bd.data_ptr(), _lib.ptr(rd), act, out.data_ptr(),
                                  _lib.ISC_F32 if out_f32 else _lib.ISC_F16, flags, _lib.stream_handle(device))
    _lib.check(st, "isc_gemm_f16")
    out = out.cpu()
    if out_packed:
        return vb.unpack_all(out, m, n)[:m]
    assert torch.equal(out[m], torch.full((n,), SENTINEL, dtype=dtype)), "the row behind the output was written"
    return out[:m]


@pytest.mark.parametrize("kernel,m,k,n,packed,out_f32,res,out_packed", QGELU_CASES)
def test_quick_gelu_epilogue_is_within_the_derived_bound(device, kernel, m, k, n, packed, out_f32, res, out_packed):
    from imagescry_amd import _lib

    c = _gemm_case(m, k, n)
    v = c["want"]  # the exact pre-activation
    got = _run_gemm(device, c, kernel, packed=packed, out_f32=out_f32, res=res, out_packed=out_packed,
                    act=_lib.ISC_ACT_QUICK_GELU)
    want, bound = co.quick_gelu_bound(v, out_f16=not out_f32, residual=c["res"] if res else None)
    name = f"QuickGELU {kernel} {m}x{k}x{n} {'f32' if out_f32 else 'f16'}{' + res' if res else ''}"
    _note(name, mb.assert_within_bound(got, want, bound, name))
    if m > 1:
        assert float(v.min()) < -3 and float(v.max()) > 3
        tail = v < -3  # and the negative tail on its own
        _note(name + " tail", mb.assert_within_bound(got[tail], want[tail], bound[tail], name + " tail"))


def test_quick_gelu_saturates_to_zero_and_identity(device):
    """Large |v|: exp2 saturates to +inf / 0 and the result is 0 / v, never NaN (float32 output, K = 64, one product
    a row: a = 1, w = 0 and the bias carries v).  The activation's -0 meets the epilogue's `+ residual` (0 without one),
    so the sign of the zero is not part of the contract."""
    from imagescry_amd import _lib

    v = torch.tensor([-3.0e4, -100.0, -60.0, 60.0, 100.0, 3.0e4, 0.0, -0.0])
    c = {"a": torch.ones(3, 64, dtype=torch.float16), "w": torch.zeros(8, 64, dtype=torch.float16), "bias": v, "res": None}
    got = _run_gemm(device, c, "tile128", packed=False, out_f32=True, res=False, out_packed=False, act=_lib.ISC_ACT_QUICK_GELU)
    want = torch.tensor([0.0, 0.0, 0.0, 60.0, 100.0, 3.0e4, 0.0, 0.0]).expand(3, 8)
    assert not torch.isnan(got).any() and torch.equal(got, want)


# =========================================================================================== isc_attention_f16_causal
# One workgroup per (sequence, head) whatever their number: no form chosen by the pair count.  T = 1, 15, 16, 17: one and
# two waves, ragged and whole blocks; 33: three waves, two staged k-steps; 77: the text tower; 80: whole blocks, an odd
# number of them; 128: the limit, eight waves.
CAUSAL_T = (1, 15, 16, 17, 33, 77, 80, 128)
BATCH = 2
PK = pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])


def _run_causal(device, qkv: torch.Tensor, pk: bool) -> torch.Tensor:
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
    st = _lib.load().isc_attention_f16_causal(qd.data_ptr(), b, t, HEADS, 64, out.data_ptr(), int(pk),
                                              _lib.stream_handle(device))
    _lib.check(st, "isc_attention_f16_causal")
    full = vb.unpack_all(out.cpu(), rows, d) if pk else out.cpu()
    assert torch.equal(full[rows:], torch.full_like(full[rows:], SENTINEL)), "rows behind the output were written"
    return full[:rows].view(b, t, d)


@functools.lru_cache(maxsize=1)
def _uniform(t: int) -> dict:
    """q = 0, positive integer values: row i is the mean over exactly the keys 0 .. i (`vit_bounds.uniform_case`'s
    argument for every prefix: exponentials exactly 1, the float32 sum exactly i + 1, P V an exact integer sum)."""
    c = vb.uniform_case(BATCH, t, HEADS, seed=2000 + t)
    v = c["qkv"][:, :, 2 * HEADS * 64 :].double()
    mean = v.cumsum(dim=1) / torch.arange(1, t + 1, dtype=torch.float64).reshape(1, t, 1)
    return {"qkv": c["qkv"], "want": mean, "bound": (vb.H + 2.0**-21) * mean.abs()}


@PK
@pytest.mark.parametrize("t", CAUSAL_T)
def test_causal_uniform_is_the_mean_over_exactly_the_prefix(device, t, pk):
    """One leaked or lost key moves the divisor of row i by 1 / (i + 1)."""
    c = _uniform(t)
    got = _run_causal(device, c["qkv"], pk)
    _note(f"causal uniform T = {t}", mb.assert_within_bound(got, c["want"], c["bound"], f"causal uniform T = {t}"))


@functools.lru_cache(maxsize=1)
def _selector(t: int) -> dict:
    """Query i selects key pi(i) <= i: a random map with pi(i) = i and pi(i) = 0 both present beyond row 0."""
    g = vb.gen(1000 + t)
    keys = torch.randint(0, 2, (BATCH, t, HEADS, 64), generator=g) * 2 - 1
    values = torch.randint(-2048, 2049, (BATCH, t, HEADS, 64), generator=g)
    pi = (torch.rand(t, generator=g) * torch.arange(1, t + 1)).long().clamp(max=torch.arange(t))
    if t > 1:
        pi[t - 1], pi[t // 2] = 0, t // 2
    assert bool((pi <= torch.arange(t)).all()) and pi[0] == 0
    return vb.selector_keys_to_case(keys, values, pi, masked=False)


@PK
@pytest.mark.parametrize("t", CAUSAL_T)
def test_causal_selector_equals_the_gather(device, t, pk):
    c = _selector(t)
    assert torch.equal(_run_causal(device, c["qkv"], pk), c["want"])


@PK
@pytest.mark.parametrize("t", [t for t in CAUSAL_T if t > 1])
def test_causal_rows_do_not_see_a_poisoned_future(device, t, pk):
    """Key and value rows of tokens >= t0 hold the finite fp16 value 60000 (NaN would fail a correct kernel: 0 x NaN in
    the P V product): the rows in front of t0 equal, bit for bit, those of the unpoisoned run."""
    qkv = vb.random_case(BATCH, t, HEADS, 0.5, seed=5000 + t)
    clean = _run_causal(device, qkv, pk)
    assert torch.isfinite(clean).all()
    d = HEADS * 64
    for t0 in sorted({t0 for t0 in (1, 16, 17, t - 1) if 1 <= t0 < t}):
        poisoned = qkv.clone()
        poisoned[:, t0:, d:] = 60000.0
        got = _run_causal(device, poisoned, pk)
        assert torch.equal(got[:, :t0], clean[:, :t0]), f"T = {t}, poisoned from {t0}"


@functools.lru_cache(maxsize=1)
def _random(t: int, scale: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    qkv = vb.random_case(BATCH, t, HEADS, scale, seed=3000 + t)
    return (qkv, *co.causal_attention_reference(qkv, HEADS))


@PK
@pytest.mark.parametrize("scale", [1.5, 0.25], ids=["peaked", "flat"])
@pytest.mark.parametrize("t", CAUSAL_T)
def test_causal_random_is_within_the_prefix_bound(device, t, scale, pk):
    qkv, want, bound = _random(t, scale)
    got = _run_causal(device, qkv, pk)
    name = f"causal randn * {scale}, T = {t}"
    _note(name, mb.assert_within_bound(got, want, bound, name))


# ===================================================================================================== isc_text_embed
def _run_embed(device, ids: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, bad_start: int | None):
    from imagescry_amd import _lib

    b, t = ids.shape
    vocab, d = table.shape
    idd, td, pd = ids.to(device), table.to(device), pos.to(device)
    out = torch.full((b * t + 1, d), NAN, dtype=torch.float32, device=device)
    out[b * t] = SENTINEL
    bad = None if bad_start is None else torch.full((1,), bad_start, dtype=torch.int32, device=device)
    st = _lib.load().isc_text_embed(idd.data_ptr(), b, t, vocab, d, td.data_ptr(), pd.data_ptr(), out.data_ptr(),
                                    _lib.ptr(bad), _lib.stream_handle(device))
    _lib.check(st, "isc_text_embed")
    out = out.cpu()
    assert torch.equal(out[b * t], torch.full((d,), SENTINEL)), "the row behind the output was written"
    assert torch.equal(idd.cpu(), ids) and torch.equal(td.cpu(), table)
    return out[: b * t].reshape(b, t, d), None if bad is None else int(bad.item())


@pytest.mark.parametrize("b,t,vocab,d", [(1, 1, 5, 4), (3, 77, 1000, 512), (2, 16, 300, 768)])
def test_text_embed_equals_the_gather_plus_positions(device, b, t, vocab, d):
    g = vb.gen(b + t + vocab + d)
    table, pos = torch.randn(vocab, d, generator=g), torch.randn(t + 3, d, generator=g)  # more position rows than T
    ids = torch.randint(0, vocab, (b, t), generator=g)
    ids.view(-1)[0], ids.view(-1)[-1] = vocab - 1, 0  # both ends of the table
    want = table[ids] + pos[:t]
    got, bad = _run_embed(device, ids, table, pos, 0)
    assert torch.equal(got, want) and bad == 0
    got, bad = _run_embed(device, ids, table, pos, None)  # the counter is optional
    assert torch.equal(got, want) and bad is None
    if b * t >= 2:  # ids -1 and vocab: counted, embedded as zeros, the table never read out of range
        planted = ids.clone()
        planted.view(-1)[1], planted.view(-1)[-2] = -1, vocab
        want = want.clone()
        want.view(-1, d)[1], want.view(-1, d)[-2] = 0.0, 0.0
        got, bad = _run_embed(device, planted, table, pos, 0)
        assert torch.equal(got, want) and bad == 2
        got, bad = _run_embed(device, planted, table, pos, 10)  # the count is ADDED to the word
        assert torch.equal(got, want) and bad == 12
        got, bad = _run_embed(device, planted, table, pos, None)
        assert torch.equal(got, want)


# ============================================================================================ isc_text_pool_layernorm
POOL_T, POOL_EOS = 77, 900
POOL_FORMS = [("f32", True, False), ("f16", False, False), ("f16-packed", False, True)]


def _pool_ids() -> tuple[torch.Tensor, list[int], list[int]]:
    """Seven sequences of ids below 900 and (rows, want with eos_id = 900, want with eos_id = -1): the EOT 900 at 0, in
    the middle, last and twice (5 and 70); a row without it, whose maximum 800 stands at 66 and again at 70; the last two
    rows hold ids ABOVE the EOT in front of it, so the two rules differ."""
    g = vb.gen(9)
    ids = torch.randint(0, 700, (7, POOL_T), generator=g)
    for row, at in ((0, 0), (1, 38), (2, 76), (3, 5), (3, 70), (5, 64), (6, 20)):
        ids[row, at] = POOL_EOS
    ids[4, 66] = ids[4, 70] = 800
    ids[5, 3] = ids[5, 65] = 950
    ids[6, 76] = 1000
    return ids, [0, 38, 76, 5, 66, 64, 20], [0, 38, 76, 5, 66, 3, 76]


def _run_pool(device, tokens: torch.Tensor, ids: torch.Tensor, eos: int, gamma, beta, *, out_f32: bool, pk: bool) -> torch.Tensor:
    from imagescry_amd import _lib

    b, t, d = tokens.shape
    dtype = torch.float32 if out_f32 else torch.float16
    if pk:
        init = torch.full((256, d), NAN, dtype=dtype)
        init[b:] = SENTINEL
        out = vb.pack_padded(init, SENTINEL).to(device)
    else:
        out = torch.full((b + 1, d), NAN, dtype=dtype, device=device)
        out[b] = SENTINEL
    td, idd, gd, bd = tokens.to(device), ids.to(device), gamma.to(device), beta.to(device)
    st = _lib.load().isc_text_pool_layernorm(td.data_ptr(), idd.data_ptr(), b, t, d, eos, gd.data_ptr(), bd.data_ptr(), 1e-5,
                                             out.data_ptr(), _lib.ISC_F32 if out_f32 else _lib.ISC_F16, int(pk),
                                             _lib.stream_handle(device))
    _lib.check(st, "isc_text_pool_layernorm")
    full = vb.unpack_all(out.cpu(), b, d) if pk else out.cpu()
    assert torch.equal(full[b:], torch.full_like(full[b:], SENTINEL)), "rows behind the output were written"
    assert torch.equal(td.cpu(), tokens)
    return full[:b]


@pytest.mark.parametrize("form,out_f32,pk", POOL_FORMS)
@pytest.mark.parametrize("d", [128, 512, 768])
def test_text_pool_layernorm_takes_the_right_row(device, d, form, out_f32, pk):
    ids, want_eos, want_max = _pool_ids()
    b, t = ids.shape
    # exactly: token row t is the unit vector e_t, and with gamma = 1, beta = 0 its LayerNorm peaks in column t alone
    marks = torch.zeros(b, t, d)
    marks[:, torch.arange(t), torch.arange(t)] = 1.0
    ones, zeros = torch.ones(d), torch.zeros(d)
    for eos, rows in ((POOL_EOS, want_eos), (-1, want_max)):
        got = _run_pool(device, marks, ids, eos, ones, zeros, out_f32=out_f32, pk=pk)
        assert got.float().argmax(dim=1).tolist() == rows, f"eos_id = {eos}"
        assert co.pooled_positions(ids, None if eos < 0 else eos).tolist() == rows  # the oracle's rule is the same
    # values: random rows, each unlike every other, within the LayerNorm bound
    g = vb.gen(d)
    tokens = torch.randn(b, t, d, generator=g) * 3 + 1.5
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    for eos, rows in ((POOL_EOS, want_eos), (-1, want_max)):
        got = _run_pool(device, tokens, ids, eos, gamma, beta, out_f32=out_f32, pk=pk)
        want, bound = vb.layernorm_reference(tokens[torch.arange(b), rows], gamma, beta, 1e-5, out_f16=not out_f32)
        _note(f"pool LayerNorm D = {d} {form}", mb.assert_within_bound(got, want, bound, f"D = {d}, {form}, eos_id = {eos}"))


@pytest.mark.parametrize("form,out_f32,pk", POOL_FORMS)
@pytest.mark.parametrize("d", [128, 512, 768, 1024, 2048])  # 1, 2, 3, 4 and 8 vectors per lane: every instantiation
def test_text_pool_layernorm_has_the_bits_of_isc_layernorm(device, d, form, out_f32, pk):
    """The pooling kernel carries its own copy of k_layernorm's row arithmetic (vit.hip: `layernorm_row`); the two must
    not drift apart: on the pooled rows, gathered by the host, isc_layernorm gives the same bits."""
    from imagescry_amd import _lib

    ids, want_eos, _ = _pool_ids()
    b, t = ids.shape
    g = vb.gen(d + 1)
    tokens = torch.randn(b, t, d, generator=g) * 3 + 1.5
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    got = _run_pool(device, tokens, ids, POOL_EOS, gamma, beta, out_f32=out_f32, pk=pk)
    rows = tokens[torch.arange(b), want_eos].contiguous().to(device)
    gd, bd = gamma.to(device), beta.to(device)
    dtype = torch.float32 if out_f32 else torch.float16
    out = torch.full((256 * d,) if pk else (b, d), NAN, dtype=dtype, device=device)
    st = _lib.load().isc_layernorm(rows.data_ptr(), b, d, d, gd.data_ptr(), bd.data_ptr(), 1e-5, out.data_ptr(),
                                   _lib.ISC_F32 if out_f32 else _lib.ISC_F16, d, int(pk), _lib.stream_handle(device))
    _lib.check(st, "isc_layernorm")
    want = vb.unpack_all(out.cpu(), b, d)[:b] if pk else out.cpu()
    assert not torch.isnan(got.float()).any() and torch.equal(got, want)


# ====================================================================================================== the model
def _unit(x: torch.Tensor) -> torch.Tensor:
    return F.normalize(x, dim=1)


def _model(monkeypatch, device, preset: str, act: str = "quick_gelu", **kw):
    """`CLIPEmbedder(preset)` at two layers a tower (the preset table is patched, as `_shallow` of
    tests/test_gpu_dinov2.py patches DINOv2's) with seeded random weights, biases and LayerNorm affines."""
    from imagescry_amd import CLIPEmbedder, clip

    cfg, sd = co.shallow(preset, act)
    monkeypatch.setitem(clip.PRESETS, preset, cfg)
    model = CLIPEmbedder(preset, state_dict=sd, act=act, **kw).to(device)
    assert model.clip_config == cfg and len(model._net.blocks) == co.MODEL_DEPTH == len(model._text.blocks)
    return model, cfg, sd


def _check_model(what: str, got: torch.Tensor, want: torch.Tensor, want16: torch.Tensor, e: int) -> None:
    scale = math.sqrt(768 / e)
    err, err16 = (got - want).abs().max().item(), (got - want16).abs().max().item()
    print(f"{what}: max|err| f32 oracle {err:.3e} (bound {1e-2 * scale:.2e}), fp16-operand oracle {err16:.3e} "
          f"(bound {2e-3 * scale:.2e}), 1 - min cosine {1 - (got * want).sum(dim=1).min().item():.2e}")
    assert err < 1e-2 * scale
    assert err16 < 2e-3 * scale
    assert torch.allclose(got.norm(dim=1), torch.ones(got.shape[0]), atol=1e-5)


IMAGE_RUNS = [(*c, "quick_gelu") for c in co.IMAGE_CASES] + [(*co.IMAGE_CASES[0], "gelu")]
TEXT_RUNS = [(*c, "quick_gelu") for c in co.TEXT_CASES] + [(*co.TEXT_CASES[1], "gelu")]


@pytest.mark.parametrize("preset,shape,grid,max_patches,tokens,act", IMAGE_RUNS)
def test_image_tower_matches_oracle(device, monkeypatch, preset, shape, grid, max_patches, tokens, act):
    """Both `act` values run, but this bound cannot tell them apart: on these nets QuickGELU and the erf GELU differ by
    about 1.9e-3 at the output, inside the 2.4e-3 allowed to the fp16-operand oracle.  The activation is pinned by
    `test_quick_gelu_epilogue_is_within_the_derived_bound`, where the erf form is four orders of magnitude outside."""
    from imagescry_amd import ImageBatch, vit

    kw = dict(grid="aspect", max_patches=max_patches) if grid == "aspect" else {}
    model, cfg, sd = _model(monkeypatch, device, preset, act, **kw)
    p = cfg.vision.patch_size
    if grid == "aspect":
        assert vit.token_grid(*shape, max_patches) == (shape[0] // p, shape[1] // p)
    assert (shape[0] // p) * (shape[1] // p) + 1 == tokens
    images = co.model_images(co.MODEL_BATCH, *shape, seed=tokens)
    ib = ImageBatch(indices=torch.arange(co.MODEL_BATCH), images=images).to(device)
    e = model.predict_step(ib).embeddings
    assert e.shape == (co.MODEL_BATCH, cfg.embed_dim, 1, 1) and e.dtype == torch.float32 and model.embedding_dim == cfg.embed_dim
    x = co.preprocess_reference(images)
    torch.testing.assert_close(model.preprocess(ib.images).cpu(), x, rtol=1e-6, atol=1e-6)  # fixed statistics, no clipping
    okw = dict(patch=p, heads=cfg.vision.heads, act=act)
    with torch.no_grad():
        want, want16 = _unit(co.clip_image_features(sd, x, **okw)), _unit(co.clip_image_features(sd, x, round_operands_fp16=True, **okw))
    _check_model(f"CLIP {preset} {act} {shape} (T = {tokens})", e.reshape(co.MODEL_BATCH, -1).cpu(), want, want16, cfg.embed_dim)


@pytest.mark.parametrize("preset,t,act", TEXT_RUNS)
def test_text_tower_matches_oracle(device, monkeypatch, preset, t, act):
    """Sixteen sequences with the end-of-text token at positions 1 .. T - 1.  (The activation: see
    `test_image_tower_matches_oracle`.)"""
    model, cfg, sd = _model(monkeypatch, device, preset, act)
    ids, eot = co.text_ids(co.TEXT_QUERIES, t, cfg.text.vocab, seed=t)
    assert eot[0] == 1 and eot[-1] == t - 1 and co.pooled_positions(ids, None).tolist() == eot.tolist()
    got = model.encode_text(ids)  # CPU ids are copied over
    assert got.shape == (co.TEXT_QUERIES, cfg.embed_dim) and got.dtype == torch.float32 and got.device == model.device
    assert torch.equal(model.encode_text(ids.to(device).int(), validate=False), got)  # int32, on the device, no host read
    raw = model.encode_text(ids, normalize=False)
    assert torch.allclose(F.normalize(raw, dim=1), got, atol=1e-6) and not torch.equal(raw, got)
    okw = dict(heads=cfg.text.heads, act=act)
    with torch.no_grad():
        want, want16 = _unit(co.clip_text_features(sd, ids, **okw)), _unit(co.clip_text_features(sd, ids, round_operands_fp16=True, **okw))
    _check_model(f"CLIP {preset} {act} text T = {t}", got.cpu(), want, want16, cfg.embed_dim)
    # not seeing the future: other ids behind each EOT, the same bits
    other = ids.clone()
    for row, at in enumerate(eot.tolist()):
        other[row, at + 1 :] = torch.randint(1, cfg.text.vocab - 1, (t - at - 1,), generator=vb.gen(row))
    assert not torch.equal(other, ids)
    assert torch.equal(model.encode_text(other), got)


def test_eos_token_id_pools_at_the_first_one_and_bad_ids_raise(device, monkeypatch):
    import dataclasses

    from imagescry_amd import CLIPEmbedder

    model, cfg, sd = _model(monkeypatch, device, "ViT-B/16")
    ids, eot = co.text_ids(4, 20, cfg.text.vocab, seed=1)
    ids[:, 0] = cfg.text.vocab - 1  # a larger id than the EOT 1000 in front of it: the two rules differ
    for row, at in enumerate(eot.tolist()):
        ids[row, at] = 1000
    assert co.pooled_positions(ids, 1000).tolist() == eot.tolist() and co.pooled_positions(ids, None).tolist() == [0] * 4
    with_eos = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, eos_token_id=1000))
    got = CLIPEmbedder(with_eos, state_dict=sd).to(device).encode_text(ids).cpu()
    with torch.no_grad():
        want = _unit(co.clip_text_features(sd, ids, heads=cfg.text.heads, eos_token_id=1000))
        at_max = _unit(co.clip_text_features(sd, ids, heads=cfg.text.heads))
    assert (got - want).abs().max().item() < 1e-2 * math.sqrt(768 / cfg.embed_dim) < (got - at_max).abs().max().item()
    assert (model.encode_text(ids).cpu() - at_max).abs().max().item() < 1e-2 * math.sqrt(768 / cfg.embed_dim)
    bad = ids.clone()
    bad[1, 2], bad[3, 0] = cfg.text.vocab, -1
    with pytest.raises(ValueError, match="2 token id"):
        model.encode_text(bad)
    out = model.encode_text(bad, validate=False)  # no host read, no fault: the rows are embedded as zeros
    assert out.shape == (4, cfg.embed_dim) and torch.equal(out[0], model.encode_text(ids)[0])


def test_batch_of_five_in_passes_of_two_equals_its_slices(device, monkeypatch):
    from imagescry_amd import CLIPEmbedder, vit

    model, cfg, sd = _model(monkeypatch, device, "ViT-B/32", max_images_per_pass=2)
    x = model.preprocess(co.model_images(5, 224, 224, seed=5).to(device))
    full = model(x)  # three passes: 2 + 2 + 1 images
    assert full.shape == (5, cfg.embed_dim, 1, 1)
    one_pass = CLIPEmbedder("ViT-B/32", state_dict=sd).to(device)
    assert torch.equal(one_pass(x), full) and torch.equal(torch.cat([one_pass(x[:3]), one_pass(x[3:])]), full)
    ids, _ = co.text_ids(5, 20, cfg.text.vocab, seed=6)
    whole = model.encode_text(ids)
    monkeypatch.setattr(vit, "PASS_ROWS", 2 * 20)  # two sequences a pass
    assert torch.equal(model.encode_text(ids), whole)
    assert torch.equal(torch.cat([model.encode_text(ids[i : i + 1]) for i in range(5)]), whole)


# ====================================================================================================== end to end
def test_text_queries_search_an_image_bank(device, monkeypatch):
    """Every score is within ||q_gpu - q_oracle|| + ||r_gpu - r_oracle|| + 1e-6 of the oracle's cosine: for unit vectors
    |q.r - q'.r'| <= |q - q'| |r| + |q'| |r - r'| (Cauchy-Schwarz), computed from the measured vector errors; 1e-6 covers
    the float32 dot product of 512 terms and norms that are 1 to 1e-7."""
    from imagescry_amd import EmbeddingBank, ImageBatch

    model, cfg, sd = _model(monkeypatch, device, "ViT-B/32")
    images = co.model_images(6, 224, 224, seed=60)
    batches = [ImageBatch(indices=torch.arange(i, i + 3), images=images[i : i + 3]).to(device) for i in (0, 3)]
    bank = EmbeddingBank.from_batches([model.predict_step(b) for b in batches], dtype=torch.float32)
    assert bank.num_local_rows == 6 and bank.dim == cfg.embed_dim
    ids, _ = co.text_ids(4, 12, cfg.text.vocab, seed=61)
    q = model.encode_text(ids)
    scores, idx = bank.search(q, k=6)
    ex_scores, ex_idx = bank.search_exhaustive(q, k=6)
    assert torch.equal(idx, ex_idx) and torch.equal(scores, ex_scores)
    assert sorted(idx[0].tolist()) == list(range(6))
    with torch.no_grad():
        r_want = _unit(co.clip_image_features(sd, co.preprocess_reference(images), patch=32, heads=cfg.vision.heads))
        q_want = _unit(co.clip_text_features(sd, ids, heads=cfg.text.heads))
    rows = torch.cat([model.predict_step(b).embeddings for b in batches]).reshape(6, -1).cpu()
    dq, dr = (q.cpu() - q_want).norm(dim=1), (rows - r_want).norm(dim=1)
    cos = q_want @ r_want.T  # [4, 6]
    idx, scores = idx.cpu(), scores.cpu()
    for i in range(4):
        slack = dq[i] + dr[idx[i]] + 1e-6
        assert bool(((scores[i] - cos[i, idx[i]]).abs() <= slack).all()), (i, scores[i], cos[i, idx[i]], slack)
    print(f"text -> image search: |dq| <= {dq.max().item():.2e}, |dr| <= {dr.max().item():.2e}, "
          f"score error <= {(scores - cos.gather(1, idx)).abs().max().item():.2e}")


def test_earlier_embedders_are_untouched_by_clip_instances(device, monkeypatch):
    import dataclasses

    from imagescry_amd import DINOv2Embedder, ImageBatch, ViTB16Embedder, embedding, vit

    ib = ImageBatch(indices=torch.arange(3), images=co.model_images(3, 120, 90, seed=2)).to(device)
    default = ViTB16Embedder(seed=1).to(device)  # the default configuration
    aspect = ViTB16Embedder(seed=1, output="patches", grid="aspect").to(device)
    dcfg = dataclasses.replace(embedding.DINOV2_PRESETS["vits14", True], depth=2)
    monkeypatch.setitem(embedding.DINOV2_PRESETS, ("vits14", True), dcfg)
    dino = DINOv2Embedder("vits14", True, state_dict=vit.make_state_dict(dcfg, seed=3, randomize_affine=True),
                          output="patches", grid="aspect", max_patches=64).to(device)
    before = [m.predict_step(ib).embeddings.clone() for m in (default, aspect, dino)]
    for preset, act in (("ViT-B/32", "quick_gelu"), ("ViT-B/16", "gelu")):
        m, cfg, _sd = _model(monkeypatch, device, preset, act, grid="aspect")
        assert m.predict_step(ib).embeddings.shape == (3, cfg.embed_dim, 1, 1)
        ids, _ = co.text_ids(3, 9, cfg.text.vocab, seed=4)
        assert m.encode_text(ids).shape == (3, cfg.embed_dim)
    after = [m.predict_step(ib).embeddings for m in (default, aspect, dino)]
    assert all(torch.equal(a, b) for a, b in zip(after, before))
