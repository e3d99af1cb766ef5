"""The DINOv2 backbones on the GPU: the LayerScale GEMM epilogue (isc_gemm_f16_scaled, both kernels), the padded
patchify, the token assembly with registers, the patch head that skips them, the antialiased position resampling, and
`DINOv2Embedder` end to end -- against exact integer products, exact gathers, float32 torch restatements
(tests/dinov2_oracle.py, pinned to transformers in tests/test_dinov2_host.py) and through `EmbeddingBank`.

Exact cases assert `torch.equal`: the GEMM operands are the integers of `vit_bounds.gemm_case` and the scales come from
{-2, -1, -0.5, 0.25, 1, 3}, so scale * (product + bias) + residual is a multiple of 0.25 below 2^18 -- a float32 number
whether or not the multiplication and the addition are fused.  Every call goes through the C ABI, outputs are prefilled
with NaN, the padding rows of packed operands hold NaN and a sentinel row sits behind row-major outputs.

Tolerances.  isc_vit_tokens_out_skip: rtol = atol = 1e-5, as `test_tokens_out`.  isc_vit_pos_resample_aa:
`dinov2_oracle.aa_bound`, derived in tests/test_dinov2_host.py, where torch's own float32 is held to it.  The model:
the bounds of `test_patch_map_matches_oracle` on unit-norm outputs (1e-2 to the float32 oracle, 2e-3 to the oracle with
fp16-rounded operands, norms within 1e-5), the two absolute ones times sqrt(768 / D) -- the entries of a unit vector
scale as D^-1/2."""

from __future__ import annotations

import dataclasses
import functools
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import vit_bounds as vb  # noqa: E402
from dinov2_oracle import AA_GRIDS, aa_bound, dinov2_tokens, patch_map  # noqa: E402
from oracle import transforms_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0
SCALES = torch.tensor([-2.0, -1.0, -0.5, 0.25, 1.0, 3.0])


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ============================================================================================ isc_gemm_f16_scaled
# Copies of the first and last entries of TILE128_SHAPES and STREAM_SHAPES (tests/test_gpu_vit_exact.py), one with M no
# multiple of 16 and one with M just past a 256-row tile each; N = 384 is ViT-S's.
TILE128_SHAPES = [(1, 64, 4), (640, 3072, 256), (77, 128, 384), (257, 384, 384)]
STREAM_SHAPES = [(300, 128, 256), (10753, 192, 3072), (77, 128, 768), (257, 768, 768)]


@functools.lru_cache(maxsize=1)
def _gemm_case(m: int, k: int, n: int) -> dict:
    top = 8 if k <= 192 else 4
    c = vb.gemm_case(m, k, n, seed=m + k + n, lo=-top, hi=top)
    c["scale"] = SCALES[torch.randint(0, len(SCALES), (n,), generator=_gen(n + 1))]
    for res in (False, True):  # exact in float64, and a float32 number
        want = c["scale"].double() * c["want"] + (c["res"].double() if res else 0.0)
        assert torch.equal(want.float().double(), want)
        c["scaled_res" if res else "scaled"] = want.float()
    return c


def _run_gemm(device, c: dict, kernel: str, *, packed: bool, res: bool, scale: torch.Tensor | None) -> torch.Tensor:
    """One float32-output call on the operands of `c`: isc_gemm_f16_scaled with `scale`, isc_gemm_f16 without."""
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
    out = torch.full((m + 1, n), NAN, dtype=torch.float32, device=device)
    out[m] = SENTINEL
    args = (_lib.ptr(rd), _lib.ISC_ACT_NONE, out.data_ptr(), _lib.ISC_F32, flags, _lib.stream_handle(device))
    if scale is None:
        st = _lib.load().isc_gemm_f16(ad.data_ptr(), m, k, wd.data_ptr(), n, bd.data_ptr(), *args)
    else:
        sc = scale.to(device)
        st = _lib.load().isc_gemm_f16_scaled(ad.data_ptr(), m, k, wd.data_ptr(), n, bd.data_ptr(), sc.data_ptr(), *args)
    _lib.check(st, "isc_gemm_f16_scaled")
    out = out.cpu()
    assert torch.equal(out[m], torch.full((n,), SENTINEL)), "the row behind the output was written"
    if res:
        assert torch.equal(rd.cpu(), c["res"])
    return out[:m]


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("m,k,n", TILE128_SHAPES)
def test_scaled_gemm_tile128_is_exact(device, m, k, n, packed, res):
    c = _gemm_case(m, k, n)
    got = _run_gemm(device, c, "tile128", packed=packed, res=res, scale=c["scale"])
    assert torch.equal(got, c["scaled_res" if res else "scaled"])
    ones = _run_gemm(device, c, "tile128", packed=packed, res=res, scale=torch.ones(n))
    assert torch.equal(ones, _run_gemm(device, c, "tile128", packed=packed, res=res, scale=None))


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("m,k,n", STREAM_SHAPES)
def test_scaled_gemm_stream_is_exact(device, m, k, n, res):
    c = _gemm_case(m, k, n)
    got = _run_gemm(device, c, "stream", packed=True, res=res, scale=c["scale"])
    assert torch.equal(got, c["scaled_res" if res else "scaled"])
    ones = _run_gemm(device, c, "stream", packed=True, res=res, scale=torch.ones(n))
    assert torch.equal(ones, _run_gemm(device, c, "stream", packed=True, res=res, scale=None))


# ========================================================================================= isc_patchify_f16_padded
def _patch_rows(x: torch.Tensor, p: int, kpad: int) -> torch.Tensor:
    """[B, C, H, W] -> fp16 [B * gh * gw, kpad]: row (b, ph, pw), column c * P * P + r * P + s, zeros behind."""
    b, c, h, w = x.shape
    rows = x.unfold(2, p, p).unfold(3, p, p).permute(0, 2, 3, 1, 4, 5).reshape(b * (h // p) * (w // p), c * p * p).half()
    return F.pad(rows, (0, kpad - c * p * p))


def _run_patchify(device, x: torch.Tensor, p: int, kpad: int | None, packed: bool) -> torch.Tensor:
    """`kpad` None: isc_patchify_f16.  Returns every row of the buffer (packed: whole tiles; row-major: + one sentinel row)."""
    from imagescry_amd import _lib

    b, c, h, w = x.shape
    m = b * (h // p) * (w // p)
    cols = kpad or c * p * p
    xd = x.to(device)
    if packed:
        out = torch.full(((m + 255) // 256 * 256 * cols,), NAN, dtype=torch.float16, device=device)
    else:
        out = torch.full((m + 1, cols), NAN, dtype=torch.float16, device=device)
        out[m] = SENTINEL
    if kpad is None:
        st = _lib.load().isc_patchify_f16(xd.data_ptr(), b, c, h, w, p, out.data_ptr(), int(packed), _lib.stream_handle(device))
    else:
        st = _lib.load().isc_patchify_f16_padded(xd.data_ptr(), b, c, h, w, p, kpad, out.data_ptr(), int(packed),
                                                 _lib.stream_handle(device))
    _lib.check(st, "isc_patchify_f16_padded")
    assert torch.equal(xd.cpu(), x)
    out = out.cpu()
    return vb.unpack_all(out, m, cols) if packed else out


@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("b,gh,gw", [(1, 1, 1), (2, 3, 5), (2, 10, 13)])  # 260 rows: past one packed tile
def test_padded_patchify_equals_unfold(device, b, gh, gw, packed):
    p, kpad = 14, 640
    x = torch.randn(b, 3, gh * p, gw * p, generator=_gen(gh * 10 + gw)) * 3
    m = b * gh * gw
    got = _run_patchify(device, x, p, kpad, packed)
    want = _patch_rows(x, p, kpad)
    assert torch.equal(got[:m], want)
    assert torch.equal(got[:m, 588:], torch.zeros(m, 52, dtype=torch.float16))  # the padding columns: zero, not NaN
    if packed:
        assert torch.isnan(got[m:]).all()  # the padding ROWS of the last tile are nobody's to write
    else:
        assert torch.equal(got[m], torch.full((kpad,), SENTINEL, dtype=torch.float16))


@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
def test_padded_patchify_at_patch_16_is_the_existing_entry(device, packed):
    x = torch.randn(2, 3, 48, 80, generator=_gen(16)) * 3
    got = _run_patchify(device, x, 16, 768, packed)
    old = _run_patchify(device, x, 16, None, packed)
    assert torch.equal(got.view(torch.int16), old.view(torch.int16))  # the same bytes, NaN prefill included
    assert torch.equal(got[:30], _patch_rows(x, 16, 768))


# ============================================================================================ isc_vit_assemble_reg
@pytest.mark.parametrize("d", [4, 384])
@pytest.mark.parametrize("r", [0, 1, 4])
def test_assemble_with_registers(device, r, d):
    from imagescry_amd import _lib

    b, p = 2, 3
    t = 1 + r + p
    g = _gen(r * 1000 + d)
    pe, cls, pos = torch.randn(b * p, d, generator=g), torch.randn(d, generator=g), torch.randn(1 + p, d, generator=g)
    reg = torch.randn(max(r, 1), d, generator=g)
    want = torch.cat([(cls + pos[0]).expand(b, 1, d), reg[:r].expand(b, r, d), pe.reshape(b, p, d) + pos[1:]], dim=1)
    ped, clsd, posd, regd = pe.to(device), cls.to(device), pos.to(device), reg.to(device)
    lib, s = _lib.load(), _lib.stream_handle(device)

    def run(fn, *args):
        out = torch.full((b * t + 1, d), NAN, dtype=torch.float32, device=device)
        out[b * t] = SENTINEL
        _lib.check(fn(*args, out.data_ptr(), s), "isc_vit_assemble_reg")
        out = out.cpu()
        assert torch.equal(out[b * t], torch.full((d,), SENTINEL))
        return out[: b * t].reshape(b, t, d)

    got = run(lib.isc_vit_assemble_reg, ped.data_ptr(), clsd.data_ptr(), regd.data_ptr() if r else None, posd.data_ptr(),
              b, t, r, d)
    assert torch.equal(got, want)
    if r == 0:
        assert torch.equal(got, run(lib.isc_vit_assemble, ped.data_ptr(), clsd.data_ptr(), posd.data_ptr(), b, t, d))


# ========================================================================================= isc_vit_tokens_out_skip
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("d", [384, 1024])
@pytest.mark.parametrize("cells", [1, 15, 65])
@pytest.mark.parametrize("skip", [1, 5])
def test_tokens_out_skip(device, skip, cells, d, normalize):
    from imagescry_amd import _lib

    b, t = 2, skip + cells
    g = _gen(skip * 1000 + cells + d)
    tokens = torch.randn(b, t, d, generator=g) * 3 + 1.5
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    want = F.layer_norm(tokens[:, skip:], (d,), gamma, beta, 1e-6).transpose(1, 2)
    if normalize:
        want = F.normalize(want, dim=1, eps=1e-12)
    td, gd, bd = tokens.to(device), gamma.to(device), beta.to(device)
    lib, s = _lib.load(), _lib.stream_handle(device)

    def run(fn, *shape):
        out = torch.full((b * d * cells + 4,), NAN, dtype=torch.float32, device=device)
        out[b * d * cells :] = SENTINEL
        _lib.check(fn(td.data_ptr(), b, t, *shape, d, gd.data_ptr(), bd.data_ptr(), 1e-6, int(normalize), 1e-12,
                      out.data_ptr(), s), "isc_vit_tokens_out_skip")
        out = out.cpu()
        assert torch.equal(out[b * d * cells :], torch.full((4,), SENTINEL))
        return out[: b * d * cells].reshape(b, d, cells)

    got = run(lib.isc_vit_tokens_out_skip, skip)
    assert not torch.isnan(got).any() and torch.equal(td.cpu(), tokens)
    torch.testing.assert_close(got, want.contiguous(), rtol=1e-5, atol=1e-5)
    if skip == 1 and t > 1:
        assert torch.equal(got, run(lib.isc_vit_tokens_out))


# ========================================================================================= isc_vit_pos_resample_aa
@pytest.mark.parametrize("g,h,w", AA_GRIDS)
def test_pos_resample_aa_matches_interpolate(device, g, h, w):
    from imagescry_amd import _lib

    d = 64
    pos = torch.randn(1 + g * g, d, generator=_gen(g * 100 + h * 10 + w)) * 0.02  # the host test's table
    pd = pos.to(device)
    out = torch.full((2 + h * w, d), NAN, dtype=torch.float32, device=device)
    out[1 + h * w] = SENTINEL
    _lib.check(_lib.load().isc_vit_pos_resample_aa(pd.data_ptr(), g, h, w, d, out.data_ptr(), _lib.stream_handle(device)),
               "isc_vit_pos_resample_aa")
    got = out.cpu()
    assert torch.equal(got[1 + h * w], torch.full((d,), SENTINEL)) and torch.equal(pd.cpu(), pos)
    want = F.interpolate(pos[1:].double().reshape(1, g, g, d).permute(0, 3, 1, 2), size=(h, w), mode="bicubic",
                         align_corners=False, antialias=True).permute(0, 2, 3, 1).reshape(h * w, d)
    assert torch.equal(got[0], pos[0])  # the class row is kept
    err = (got[1 : 1 + h * w].double() - want).abs().max().item()
    bound = aa_bound(g, h, w, pos.abs().max().item())
    print(f"pos_resample_aa {g} -> {h}x{w}: max|err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ====================================================================================================== the model
def _images(batch: int, h: int, w: int, seed: int) -> torch.Tensor:
    return torch.randint(0, 256, (batch, 3, h, w), dtype=torch.uint8, generator=_gen(seed))


def _shallow(monkeypatch, variant: str, registers: bool):
    """The preset at depth 2, and seeded weights with random biases, norms and LayerScale for it."""
    from imagescry_amd import embedding, vit

    cfg = dataclasses.replace(embedding.DINOV2_PRESETS[variant, registers], depth=2)
    monkeypatch.setitem(embedding.DINOV2_PRESETS, (variant, registers), cfg)
    return cfg, vit.make_state_dict(cfg, seed=len(variant) + cfg.dim + registers, randomize_affine=True)


# (variant, registers, image shape, max_patches, token grid):
#   T = 20: one-shot attention, the 128-tile GEMMs (N = 384);  T = 226: streaming attention, stream GEMMs, plain resample;
#   T = 261: ViT-L at 224 x 224 pixels;  7 x 3: the antialiased table downsampled from 37 x 37
MODEL_CASES = [("vits14", True, (42, 70), 15, (3, 5)), ("vitb14", False, (210, 210), 225, (15, 15)),
               ("vitl14", True, (224, 224), 256, (16, 16)), ("vitb14", True, (98, 42), 21, (7, 3))]


@pytest.mark.parametrize("variant,registers,shape,max_patches,grid", MODEL_CASES)
def test_embedder_matches_oracle(device, monkeypatch, variant, registers, shape, max_patches, grid):
    from imagescry_amd import DINOv2Embedder, ImageBatch, vit

    batch = 2
    cfg, sd = _shallow(monkeypatch, variant, registers)
    d, (h, w) = cfg.dim, grid
    assert vit.token_grid(*shape, max_patches) == grid and shape == (14 * h, 14 * w)
    assert float(min(sd[f"blocks.{i}.ls{n}.gamma"].min() for i in (0, 1) for n in (1, 2))) < 1e-4
    images = _images(batch, *shape, seed=h * w)
    ib = ImageBatch(indices=torch.arange(batch), images=images).to(device)
    kw = dict(state_dict=sd, grid="aspect", max_patches=max_patches)
    model = DINOv2Embedder(variant, registers, output="patches", **kw).to(device)
    assert model.config == cfg
    e = model.predict_step(ib).embeddings
    assert e.shape == (batch, d, h, w) and e.dtype == torch.float32
    e = e.cpu()
    e_cls = DINOv2Embedder(variant, registers, output="cls", **kw).to(device).predict_step(ib).embeddings.cpu()
    assert e_cls.shape == (batch, d, 1, 1)
    e_cls = e_cls.reshape(batch, d)

    x = transforms_oracle.normalize_per_channel(images, min_value=-3, max_value=3)
    okw = dict(patch=14, heads=cfg.heads, eps=cfg.ln_eps, antialias=cfg.pos_antialias)
    with torch.no_grad():
        tok = dinov2_tokens(sd, x, **okw)
        tok16 = dinov2_tokens(sd, x, round_operands_fp16=True, **okw)
    assert tok.shape == (batch, cfg.num_prefix + h * w, d)
    want, want16 = patch_map(tok, grid, cfg.num_prefix), patch_map(tok16, grid, cfg.num_prefix)
    want_cls, want_cls16 = F.normalize(tok[:, 0], dim=1), F.normalize(tok16[:, 0], dim=1)

    scale = math.sqrt(768 / d)
    err, err16 = (e - want).abs().max().item(), (e - want16).abs().max().item()
    cos = (e * want).sum(dim=1).min().item()
    err_cls, err_cls16 = (e_cls - want_cls).abs().max().item(), (e_cls - want_cls16).abs().max().item()
    print(f"DINOv2 {variant} reg {registers} {shape} -> {h}x{w} (T = {cfg.num_prefix + h * w}): max|err| f32 {err:.3e} "
          f"(bound {1e-2 * scale:.2e}), fp16-operand oracle {err16:.3e} (bound {2e-3 * scale:.2e}), 1 - min cell cosine "
          f"{1 - cos:.2e}; class token: max|err| f32 {err_cls:.3e}, fp16-operand oracle {err_cls16:.3e}")
    assert err < 1e-2 * scale
    assert err16 < 2e-3 * scale
    assert torch.allclose(e.norm(dim=1), torch.ones(batch, h, w), atol=1e-5)
    assert err_cls < 1e-2 * scale
    assert err_cls16 < 2e-3 * scale
    assert torch.allclose(e_cls.norm(dim=1), torch.ones(batch), atol=1e-5)


def test_batch_of_five_in_passes_of_two_equals_its_slices(device, monkeypatch):
    from imagescry_amd import DINOv2Embedder

    _cfg, sd = _shallow(monkeypatch, "vits14", True)
    kw = dict(state_dict=sd, output="patches", grid="aspect", max_patches=15)
    model = DINOv2Embedder("vits14", True, max_images_per_pass=2, **kw).to(device)
    x = model.preprocess(_images(5, 42, 70, seed=5).to(device))
    full = model(x)  # three passes: 2 + 2 + 1 images
    assert full.shape == (5, 384, 3, 5)
    one_pass = DINOv2Embedder("vits14", True, **kw).to(device)
    assert torch.equal(torch.cat([one_pass(x[:3]), one_pass(x[3:])]), full)
    assert torch.equal(one_pass(x), full)
    assert torch.equal(torch.cat([model(x[i : i + 1]) for i in range(5)]), full)


def test_dinov2_patch_maps_reach_the_search(device, monkeypatch):
    from imagescry_amd import DINOv2Embedder, EmbeddingBank, ImageBatch

    _cfg, sd = _shallow(monkeypatch, "vitb14", True)
    model = DINOv2Embedder("vitb14", True, state_dict=sd, output="patches", grid="aspect", max_patches=64).to(device)
    batches = [ImageBatch(indices=torch.tensor([0, 1, 2]), images=_images(3, 100, 160, seed=1)).to(device),
               ImageBatch(indices=torch.tensor([3, 4]), images=_images(2, 112, 112, seed=2)).to(device)]
    embs = [model.predict_step(b) for b in batches]
    cells = [e.embeddings.shape[2] * e.embeddings.shape[3] for e in embs]
    assert cells == [6 * 10, 8 * 8] and embs[1].embeddings.shape == (2, 768, 8, 8)
    bank = EmbeddingBank.from_batches(embs, dtype=torch.float16)
    assert bank.num_local_rows == 3 * cells[0] + 2 * cells[1] and bank.dim == 768
    first = 3 * cells[0] + cells[1]  # the second image of the second batch
    q = embs[1].get_flat_vectors()[cells[1] : 2 * cells[1]]
    scores, idx = bank.search(q, k=1)
    assert torch.equal(idx[:, 0].cpu(), torch.arange(first, first + cells[1]))  # every cell finds itself
    assert (scores[:, 0].cpu() - 1).abs().max().item() <= 1e-3  # fp16 bank


def test_vit_b16_is_untouched_by_dinov2_instances(device, monkeypatch):
    from imagescry_amd import DINOv2Embedder, ImageBatch, ViTB16Embedder

    ib = ImageBatch(indices=torch.arange(3), images=_images(3, 120, 90, seed=2)).to(device)
    default = ViTB16Embedder(seed=1).to(device)  # the default configuration
    aspect = ViTB16Embedder(seed=1, output="patches", grid="aspect").to(device)
    before, before_map = default.predict_step(ib).embeddings.clone(), aspect.predict_step(ib).embeddings.clone()
    tables = {k: v.clone() for k, v in aspect._net.pos_cache.items()}
    assert tables and not default._net.pos_cache
    for variant, registers in (("vits14", True), ("vitb14", False)):
        _cfg, sd = _shallow(monkeypatch, variant, registers)
        m = DINOv2Embedder(variant, registers, state_dict=sd, output="patches", grid="aspect", max_patches=196).to(device)
        assert m.predict_step(ib).embeddings.shape[2:] == aspect.predict_step(ib).embeddings.shape[2:]  # the same grid key
        assert m._net.pos_cache is not aspect._net.pos_cache
    assert torch.equal(default.predict_step(ib).embeddings, before) and not default._net.pos_cache
    assert torch.equal(aspect.predict_step(ib).embeddings, before_map)
    assert all(torch.equal(aspect._net.pos_cache[k], v) for k, v in tables.items())
