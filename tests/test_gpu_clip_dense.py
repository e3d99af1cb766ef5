"""Dense CLIP patch maps on the GPU: the self-attention entries (isc_attention_f16_self, isc_attention_f16_self_stream),
the head without LayerNorm (isc_tokens_to_map), `CLIPEmbedder(output="patches", dense=...)` against the float32 torch
oracle of tests/clip_dense_oracle.py, and a text query finding image regions through `EmbeddingBank.search_groups`.

Every kernel call goes through the C ABI, outputs are prefilled with NaN, the padding rows of packed operands hold NaN
and a sentinel row sits behind row-major outputs, as in tests/test_gpu_clip.py.  The self entries are the existing
kernels with another template argument, so their reference is the existing entry on the rewritten operand
(`clip_dense_oracle.rewritten`), bit for bit, with the part they must not read full of NaN; that reference is itself
inside the derived bound of tests/vit_bounds.py / tests/attention_stream_bounds.py, which is asserted too.  The model:
the project's bounds on unit-norm cells (tests/test_gpu_clip.py: 1e-2 to the float32 oracle, 2e-3 to the oracle with
fp16-rounded operands, times sqrt(768 / E), norms within 1e-5); tests/test_clip_dense_host.py shows the three modes
at least twice the loose bound apart.  The printed error / bound ratios are information."""

from __future__ import annotations

import functools
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import attention_stream_bounds as sb  # noqa: E402
import clip_dense_oracle as do  # noqa: E402
import clip_oracle as co  # noqa: E402
import matmul_bound as mb  # noqa: E402
import vit_bounds as vb  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0
HEADS = 3
D = HEADS * 64
QB, KC = sb.geometry()
PARTS = pytest.mark.parametrize("part", [do.PART_QUERY, do.PART_KEY], ids=["qq", "kk"])
PK = pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
ONE_SHOT_T = (1, 16, 17, 33, 197, 224)  # with B * heads = 6
STREAM_T = sorted({*sb.stream_lengths(QB, KC), 257})


def _note(what: str, ratio: float) -> None:
    print(f"{what}: error / bound = {ratio:.3f}")


# ======================================================================================== the self-attention entries
def _run(device, qkv: torch.Tensor, pk: bool, entry: str, part: int | None, heads: int = HEADS) -> torch.Tensor:
    """One call of `entry` (`part` None: the query-key entries, which take no part) on `qkv` [B, T, 3 D]; the B * T real
    output rows (CPU) after the guard rows were checked."""
    from imagescry_amd import _lib

    b, t, _ = qkv.shape
    d = heads * 64
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
    args = (qd.data_ptr(), b, t, heads, 64) + (() if part is None else (part,)) + (out.data_ptr(), int(pk), _lib.stream_handle(device))
    _lib.check(getattr(_lib.load(), entry)(*args), entry)
    full = vb.unpack_all(out.cpu(), rows, d) if pk else out.cpu()
    assert torch.equal(full[rows:], torch.full_like(full[rows:], SENTINEL)), "rows behind the output were written"
    return full[:rows].view(b, t, d)


@functools.lru_cache(maxsize=None)
def _random(b: int, t: int, heads: int) -> torch.Tensor:
    return vb.random_case(b, t, heads, 0.75, seed=8000 + t + b)


def _check_self(device, qkv: torch.Tensor, part: int, pk: bool, stream: bool, heads: int = HEADS, bound: bool = True) -> None:
    """The self entry on `qkv` with NaN in the part it must not read == the query-key entry on the rewritten operand."""
    plain = "isc_attention_f16_stream" if stream else "isc_attention_f16"
    self_entry = "isc_attention_f16_self_stream" if stream else "isc_attention_f16_self"
    rw = do.rewritten(qkv, part)
    want = _run(device, rw, pk, plain, None, heads)
    got = _run(device, do.poisoned(qkv, part), pk, self_entry, part, heads)
    assert not torch.isnan(got).any(), "the part that must not be read reached the result"
    assert torch.equal(got, want)
    if bound:
        t = qkv.shape[1]
        ref, bd = sb.stream_reference(rw, heads, KC) if stream else vb.attention_reference(rw, heads)
        name = f"{self_entry} part {part} T = {t}"
        _note(name, mb.assert_within_bound(got, ref, bd, name))


@PK
@PARTS
@pytest.mark.parametrize("t", ONE_SHOT_T)
def test_self_attention_equals_the_query_key_kernel_on_the_rewritten_operand(device, t, part, pk):
    _check_self(device, _random(2, t, HEADS), part, pk, stream=False)


@PK
@PARTS
def test_self_attention_persistent_form(device, part, pk):
    """B * heads just above the CU count: one sixteen-wave workgroup per CU walks the pairs (k_attention_f16_p)."""
    import ctypes

    from imagescry_amd import _lib

    cus, lds = ctypes.c_int(0), ctypes.c_int(0)
    name = ctypes.create_string_buffer(64)
    _lib.check(_lib.load().isc_device_info(ctypes.byref(cus), ctypes.byref(lds), name, 64), "isc_device_info")
    b = cus.value // HEADS + 1
    assert cus.value < b * HEADS <= cus.value + HEADS
    # the float64 bound of these operands is that of the small batches above: the exact comparison carries this one
    _check_self(device, _random(b, 17, HEADS), part, pk, stream=False, bound=False)


@PK
@PARTS
@pytest.mark.parametrize("t", STREAM_T)
def test_streaming_self_attention_equals_the_streaming_kernel_on_the_rewritten_operand(device, t, part, pk):
    _check_self(device, _random(2, t, HEADS), part, pk, stream=True)


@functools.lru_cache(maxsize=None)
def _selector(t: int, part: int) -> dict:
    c = do.self_selector_case(2, t, HEADS, seed=7000 + t, part=part)
    # as `attention_stream_bounds.stream_selector_case`: what the other keys leave of a streamed softmax rounds away
    assert t * 2048.0 * math.exp(-2.0 * c["gap"]) < sb.RESIDUE
    return c


@PK
@PARTS
@pytest.mark.parametrize("t,entry", [(17, "isc_attention_f16_self"), (224, "isc_attention_f16_self"),
                                     (17, "isc_attention_f16_self_stream"), (224, "isc_attention_f16_self_stream"),
                                     (257, "isc_attention_f16_self_stream")])
def test_self_selector_equals_the_value_rows(device, t, entry, part, pk):
    """Every row scores 128 against itself and at least 32 less against any other: the result IS the value rows.  The
    other of the two parts holds NaN."""
    c = _selector(t, part)
    assert torch.equal(_run(device, c["qkv"], pk, entry, part), c["want"])


def test_other_parts_are_invalid_and_nothing_is_launched(device):
    from imagescry_amd import _lib

    qkv = torch.zeros((2 * 17, 3 * D), dtype=torch.float16, device=device)
    out = torch.zeros((2 * 17, D), dtype=torch.float16, device=device)
    lib, s = _lib.load(), _lib.stream_handle(device)
    for fn in (lib.isc_attention_f16_self, lib.isc_attention_f16_self_stream):
        for part in (2, -1):
            assert fn(qkv.data_ptr(), 2, 17, HEADS, 64, part, out.data_ptr(), 0, s) == _lib.ISC_ERR_INVALID_ARG
        assert fn(qkv.data_ptr(), 2, 17, 2, 96, 1, out.data_ptr(), 0, s) == _lib.ISC_ERR_UNSUPPORTED
        assert fn(qkv.data_ptr() + 2, 2, 17, HEADS, 64, 1, out.data_ptr(), 0, s) == _lib.ISC_ERR_ALIGNMENT
    assert lib.isc_attention_f16_self(qkv.data_ptr(), 2, 225, HEADS, 64, 1, out.data_ptr(), 0, s) == _lib.ISC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any()


# ================================================================================================ isc_tokens_to_map
# one cell; a partial tile of 33 cells; the 4 x 6 grid; over two tiles with a wider skip
MAP_SHAPES = [(1, 2, 1, 4), (2, 34, 1, 512), (3, 26, 1, 768), (2, 70, 5, 1024)]


def _to_map(device, tokens: torch.Tensor, skip: int, normalize: bool) -> torch.Tensor:
    """[B, T, D] float32 (CPU) -> [B, D, T - skip] (device); a NaN prefill, a sentinel behind the map, the input intact."""
    from imagescry_amd import _lib

    b, t, d = tokens.shape
    cells = t - skip
    td = tokens.to(device)
    flat = torch.full((b * d * cells + 4,), NAN, dtype=torch.float32, device=device)
    flat[b * d * cells :] = SENTINEL
    st = _lib.load().isc_tokens_to_map(td.data_ptr(), b, t, skip, d, int(normalize), 1e-12, flat.data_ptr(),
                                       _lib.stream_handle(device))
    _lib.check(st, "isc_tokens_to_map")
    assert torch.equal(flat[b * d * cells :].cpu(), torch.full((4,), SENTINEL)), "memory behind the map was written"
    assert torch.equal(td.cpu().view(torch.int32), tokens.view(torch.int32))  # bits: the prefix rows hold NaN
    return flat[: b * d * cells].view(b, d, cells)


@pytest.mark.parametrize("b,t,skip,d", MAP_SHAPES)
def test_tokens_to_map_is_the_transposition_and_the_channel_normalisation(device, b, t, skip, d):
    from imagescry_amd.embedding import l2_normalize_channels

    tokens = torch.randn(b, t, d, generator=vb.gen(b + t + d)) * 3 + 0.5
    tokens[:, :skip] = NAN  # the prefix rows are never read into a cell
    if t - skip > 1:
        tokens[b - 1, skip + 1] = 0.0  # a zero cell
    want = tokens[:, skip:].transpose(1, 2).contiguous()
    got = _to_map(device, tokens, skip, False)
    assert torch.equal(got.cpu(), want)
    normed = _to_map(device, tokens, skip, True)
    assert not torch.isnan(normed).any()
    assert torch.equal(normed, l2_normalize_channels(got.reshape(b, d, 1, t - skip)).reshape(b, d, t - skip))
    torch.testing.assert_close(normed.cpu(), F.normalize(want, dim=1), rtol=1e-6, atol=1e-7)
    if t - skip > 1:
        assert not normed[b - 1, :, 1].any()  # zeros, not NaN
        assert torch.allclose(normed[0].norm(dim=0).cpu(), torch.ones(t - skip), atol=1e-6)


# ====================================================================================================== the model
def _model(monkeypatch, device, preset: str, **kw):
    """`CLIPEmbedder(preset, **kw)` at two layers a tower with seeded random weights, biases and LayerNorm affines
    (`clip_oracle.shallow`; the preset table is patched as tests/test_gpu_clip.py patches it)."""
    from imagescry_amd import CLIPEmbedder, clip

    cfg, sd = co.shallow(preset)
    monkeypatch.setitem(clip.PRESETS, preset, cfg)
    model = CLIPEmbedder(preset, state_dict=sd, **kw).to(device)
    assert model.clip_config == cfg and len(model._net.blocks) == co.MODEL_DEPTH
    return model, cfg, sd


def _check_model(what: str, got: torch.Tensor, want: torch.Tensor, want16: torch.Tensor, e: int) -> None:
    """The two bounds of tests/test_gpu_clip.py's `_check_model`, per cell ([cells, E], unit norm)."""
    scale = math.sqrt(768 / e)
    err, err16 = (got - want).abs().max().item(), (got - want16).abs().max().item()
    print(f"{what}: max|err| f32 oracle {err:.3e} (bound {1e-2 * scale:.2e}, ratio {err / (1e-2 * scale):.3f}), "
          f"fp16-operand oracle {err16:.3e} (bound {2e-3 * scale:.2e}, ratio {err16 / (2e-3 * scale):.3f}), "
          f"1 - min cosine {1 - (got * want).sum(dim=1).min().item():.2e}")
    assert err < 1e-2 * scale
    assert err16 < 2e-3 * scale
    assert torch.allclose(got.norm(dim=1), torch.ones(got.shape[0]), atol=1e-5)


@functools.lru_cache(maxsize=None)
def _oracles(preset: str, shape: tuple[int, int], tokens: int, mode: str) -> tuple[torch.Tensor, torch.Tensor]:
    cfg, sd = co.shallow(preset)
    x = co.preprocess_reference(co.model_images(co.MODEL_BATCH, *shape, seed=tokens))
    kw = dict(patch=cfg.vision.patch_size, heads=cfg.vision.heads, mode=mode)
    with torch.no_grad():
        return (do.unit_cells(do.clip_dense_features(sd, x, **kw)),
                do.unit_cells(do.clip_dense_features(sd, x, round_operands_fp16=True, **kw)))


@pytest.mark.parametrize("mode", do.MODES)
@pytest.mark.parametrize("preset,shape,grid,max_patches,tokens", do.DENSE_CASES)
def test_dense_patch_map_matches_oracle(device, monkeypatch, preset, shape, grid, max_patches, tokens, mode):
    from imagescry_amd import ImageBatch, vit

    kw = dict(grid="aspect", max_patches=max_patches) if grid == "aspect" else {}
    model, cfg, _sd = _model(monkeypatch, device, preset, output="patches", dense=mode, **kw)
    p, e = cfg.vision.patch_size, cfg.embed_dim
    h, w = shape[0] // p, shape[1] // p
    if grid == "aspect":
        assert vit.token_grid(*shape, max_patches) == (h, w) and h != w
    assert h * w + 1 == tokens and model.embedding_dim == e
    images = co.model_images(co.MODEL_BATCH, *shape, seed=tokens)
    ib = ImageBatch(indices=torch.arange(co.MODEL_BATCH), images=images).to(device)
    got = model.predict_step(ib).embeddings
    assert got.shape == (co.MODEL_BATCH, e, h, w) and got.dtype == torch.float32 and got.is_contiguous()
    want, want16 = _oracles(preset, shape, tokens, mode)
    _check_model(f"dense CLIP {preset} {mode} {shape} (T = {tokens})", do.unit_cells(got.cpu()), want, want16, e)
    # forward: the same map before the normalisation
    raw = model(model.preprocess(ib.images))
    assert raw.shape == got.shape
    assert torch.allclose(F.normalize(raw, dim=1), got, atol=1e-6) and not torch.equal(raw, got)
    # passes of one image give the bits of one pass of two
    single, _, _ = _model(monkeypatch, device, preset, output="patches", dense=mode, max_images_per_pass=1, **kw)
    assert torch.equal(single.predict_step(ib).embeddings, got)


def test_one_cell_map_takes_the_separate_normalisation(device, monkeypatch):
    from imagescry_amd import ImageBatch
    from imagescry_amd.embedding import l2_normalize_channels

    model, cfg, _sd = _model(monkeypatch, device, "ViT-B/32", output="patches", dense="kk", grid="aspect", max_patches=1)
    ib = ImageBatch(indices=torch.arange(2), images=co.model_images(2, 50, 70, seed=3)).to(device)
    got = model.predict_step(ib).embeddings
    assert got.shape == (2, cfg.embed_dim, 1, 1)
    assert torch.equal(got, l2_normalize_channels(model(model.preprocess(ib.images))))


# ================================================================================================= text to region
def test_text_queries_find_regions_through_search_groups(device, monkeypatch):
    from imagescry_amd import EmbeddingBank, ImageBatch

    model, cfg, _sd = _model(monkeypatch, device, "ViT-B/32", output="patches", dense="kk")
    images = co.model_images(3, 224, 224, seed=70)
    batch = model.predict_step(ImageBatch(indices=torch.arange(3), images=images).to(device))
    cells = 49
    groups = torch.arange(3).repeat_interleave(cells)
    bank = EmbeddingBank.from_batches([batch], dtype=torch.float32, row_groups=groups)
    assert bank.num_local_rows == 3 * cells and bank.dim == cfg.embed_dim
    # row r of the bank is cell (r % 49) of image r // 49
    flat = batch.embeddings.permute(0, 2, 3, 1).reshape(3 * cells, cfg.embed_dim)
    assert torch.equal(bank.rows(torch.arange(3 * cells)), flat)
    ids, _ = co.text_ids(4, 12, cfg.text.vocab, seed=71)
    q = model.encode_text(ids)
    table = bank.scores(q, torch.arange(3 * cells)).cpu()  # [4, 147]
    exact = (q.cpu().double() @ flat.cpu().double().T)
    assert (table.double() - exact).abs().max().item() <= 1e-5
    scores, idx, labels = bank.search_groups(q, 2)
    best = table.view(4, 3, cells).amax(dim=2)  # the best cell of every image
    order = best.argsort(dim=1, descending=True)[:, :2]
    assert torch.equal(labels.cpu(), order)
    assert torch.equal(scores.cpu(), best.gather(1, order))
    assert torch.equal(idx.cpu() // cells, order)  # the leader is a row of that image: the region
    assert torch.equal(table.gather(1, idx.cpu()), scores.cpu())


# ================================================================================================== no regression
def test_earlier_embedders_are_untouched_by_dense_instances(device, monkeypatch):
    from imagescry_amd import ImageBatch, ViTB16Embedder

    ib = ImageBatch(indices=torch.arange(2), images=co.model_images(2, 120, 90, seed=2)).to(device)
    cls_model, _, _ = _model(monkeypatch, device, "ViT-B/32")  # output="cls"
    patches = ViTB16Embedder(config=vit_two_layers(), seed=1, output="patches", grid="aspect").to(device)
    before = [m.predict_step(ib).embeddings.clone() for m in (cls_model, patches)]
    for mode in do.MODES:
        m, cfg, _sd = _model(monkeypatch, device, "ViT-B/32", output="patches", dense=mode, grid="aspect")
        out = m.predict_step(ib).embeddings
        assert out.shape[:2] == (2, cfg.embed_dim) and out.shape[2] * out.shape[3] <= 49
    after = [m.predict_step(ib).embeddings for m in (cls_model, patches)]
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    # and the class-token model shares its weights' bits with a dense one built from the same state dict
    dense, _, _ = _model(monkeypatch, device, "ViT-B/32", output="patches", dense="value")
    assert torch.equal(dense._net.blocks[-1].qkv.weight, cls_model._net.blocks[-1].qkv.weight)


def vit_two_layers():
    import dataclasses

    from imagescry_amd import vit

    return dataclasses.replace(vit.VIT_B16, depth=2)
