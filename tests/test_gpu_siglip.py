"""The SigLIP backbones on the GPU: the tanh GELU GEMM epilogue (ISC_ACT_GELU_TANH through isc_gemm_f16_act, both
kernels), the one-query attention of the pooling head (isc_attention_f16_probe), the token assembly without a class row (isc_vit_assemble_plain), and
`SigLIPEmbedder` end to end -- both towers against the float32 torch restatements of tests/siglip_oracle.py (pinned to
transformers in tests/test_siglip_host.py), text queries through `EmbeddingBank` and the sigmoid pair probability.

Every kernel call goes through the C ABI, outputs are prefilled with NaN, the padding rows of packed operands hold NaN
and a sentinel row sits behind row-major outputs, as in tests/test_gpu_clip.py.  Assertions are `torch.equal` or
`matmul_bound.assert_within_bound` against bounds derived in tests/vit_bounds.py and tests/siglip_oracle.py; the printed
error / bound ratios are information.  The model: the project's bounds on unit-norm outputs (tests/test_gpu_clip.py),
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
import siglip_oracle as so  # noqa: E402
import vit_bounds as vb  # noqa: E402
from preprocess_oracle import aa_image_bound, resize_aa_f64  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.0


def _note(what: str, ratio: float) -> None:
    print(f"{what}: error / bound = {ratio:.3f}")


# ============================================================================================ tanh GELU epilogue
# The shape grid of test_quick_gelu_epilogue_is_within_the_derived_bound (tests/test_gpu_clip.py).
# (kernel, m, k, n, packed operands, float32 output, residual, packed output)
_EPI = [(False, False), (False, True), (True, False), (True, True)]  # (float32 output, residual)
TGELU_CASES = (
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
    """One isc_gemm_f16_act call on the operands of `c`; the M real output rows (CPU), after checking the guard."""
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
    st = _lib.load().isc_gemm_f16_act(ad.data_ptr(), m, k, wd.data_ptr(), n, bd.data_ptr(), _lib.ptr(rd), act, out.data_ptr(),
                                      _lib.ISC_F32 if out_f32 else _lib.ISC_F16, flags, _lib.stream_handle(device))
    _lib.check(st, "isc_gemm_f16_act")
    out = out.cpu()
    if out_packed:
        return vb.unpack_all(out, m, n)[:m]
    assert torch.equal(out[m], torch.full((n,), SENTINEL, dtype=dtype)), "the row behind the output was written"
    return out[:m]


@pytest.mark.parametrize("kernel,m,k,n,packed,out_f32,res,out_packed", TGELU_CASES)
def test_gelu_tanh_epilogue_is_within_the_derived_bound(device, kernel, m, k, n, packed, out_f32, res, out_packed):
    from imagescry_amd import _lib

    c = _gemm_case(m, k, n)
    v = c["want"]  # the exact pre-activation
    got = _run_gemm(device, c, kernel, packed=packed, out_f32=out_f32, res=res, out_packed=out_packed,
                    act=_lib.ISC_ACT_GELU_TANH)
    want, bound = so.gelu_tanh_bound(v, out_f16=not out_f32, residual=c["res"] if res else None)
    name = f"tanh GELU {kernel} {m}x{k}x{n} {'f32' if out_f32 else 'f16'}{' + res' if res else ''}"
    _note(name, mb.assert_within_bound(got, want, bound, name))
    if m > 1:
        assert float(v.min()) < -3 and float(v.max()) > 3
        tail = v < -3  # and the negative tail on its own
        _note(name + " tail", mb.assert_within_bound(got[tail], want[tail], bound[tail], name + " tail"))
        # the test can tell the two GELUs apart: on these pre-activations the erf form fails the same check.  (How many
        # elements show it depends on the case: the two forms differ by up to 4.7e-4 around |v| = 2 and agree where both
        # saturate, and an fp16 rounding of a sum with a residual of up to 2 allows up to 1e-3 on its own.)
        erf = vb.gelu_f64(v) + (c["res"].double() if res else 0.0)
        ratio, _ = mb.worst_ratio(erf, want, bound)
        outside = int(((erf - want).abs() > bound).sum())
        print(f"{name}: the erf form reaches error / bound = {ratio:.1f}, outside on {outside} of {v.numel()} elements")
        assert ratio > 2.0 and outside > 100


def test_gelu_tanh_saturates_to_zero_and_identity(device):
    """Large |v|: exp2 saturates to +inf / 0 (and v^2 overflows to +inf for the largest) and the result is 0 / v, never
    NaN (float32 output, K = 64, one product a row: a = 1, w = 0 and the bias carries v).  The activation's -0 meets the
    epilogue's `+ residual` (0 without one), so the sign of the zero is not part of the contract.  The second call sweeps
    every finite fp16 value a product of two fp16 numbers can start from: no NaN anywhere."""
    from imagescry_amd import _lib

    v = torch.tensor([-3.0e4, -100.0, -12.0, 12.0, 100.0, 3.0e4, 0.0, -0.0, 1.0e19, -1.0e19, 3.0e38, -3.0e38])
    c = {"a": torch.ones(3, 64, dtype=torch.float16), "w": torch.zeros(12, 64, dtype=torch.float16), "bias": v, "res": None}
    got = _run_gemm(device, c, "tile128", packed=False, out_f32=True, res=False, out_packed=False, act=_lib.ISC_ACT_GELU_TANH)
    want = torch.where(v > 0, v, torch.zeros_like(v)).expand(3, 12)
    assert not torch.isnan(got).any() and torch.equal(got, want)
    every = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(torch.float16).float()
    every = every[torch.isfinite(every)]  # 63488 values
    n = every.numel()
    c = {"a": torch.ones(2, 64, dtype=torch.float16), "w": torch.zeros(n, 64, dtype=torch.float16), "bias": every, "res": None}
    got = _run_gemm(device, c, "tile128", packed=False, out_f32=True, res=False, out_packed=False, act=_lib.ISC_ACT_GELU_TANH)
    assert not torch.isnan(got).any() and torch.isfinite(got).all()
    big = every.abs() > 12
    assert torch.equal(got[0][big], torch.where(every > 0, every, torch.zeros_like(every))[big])
    want, bound = so.gelu_tanh_bound(every, out_f16=False)
    _note("tanh GELU on every finite fp16 value", mb.assert_within_bound(got[0], want, bound, "every fp16"))


# ========================================================================================== isc_attention_f16_probe
PROBE_HEADS, PROBE_B = 2, 3
PROBE_T = (1, 15, 16, 17, 63, 64, 65, 196, 225, 577)
PROBE_SHAPES = [(PROBE_HEADS, t) for t in PROBE_T] + [(12, 196)]
PK = pytest.mark.parametrize("pk", [False, True], ids=["rowmajor", "packed"])
SHAPES = pytest.mark.parametrize("heads,t", PROBE_SHAPES)


def _run_probe(device, kv: torch.Tensor, q: torch.Tensor, heads: int, pk: bool, *, tail_rows: int = 0,
               tail_fill: float = NAN) -> torch.Tensor:
    """One isc_attention_f16_probe call on `kv` [B, T, 2 D] and `q` [D]: fp16 [B, D] (CPU), after checking the guards.
    Packed: the padding rows of the kv tile hold NaN.  `tail_rows`: that many rows of `tail_fill` behind the B * T rows of
    a row-major operand (an over-allocated buffer)."""
    from imagescry_amd import _lib

    b, t, _ = kv.shape
    d = heads * 64
    rows = b * t
    if pk:
        kd = vb.pack_padded(kv.reshape(rows, 2 * d), tail_fill).to(device)
        init = torch.full(((b + 255) // 256 * 256, d), NAN, dtype=torch.float16)
        init[b:] = SENTINEL
        out = vb.pack_padded(init, SENTINEL).to(device)
    else:
        kd = torch.cat([kv.reshape(rows, 2 * d), torch.full((tail_rows, 2 * d), tail_fill, dtype=torch.float16)]).to(device)
        out = torch.full((b + 1, d), NAN, dtype=torch.float16, device=device)
        out[b] = SENTINEL
    qd = q.to(device)
    st = _lib.load().isc_attention_f16_probe(kd.data_ptr(), qd.data_ptr(), b, t, heads, 64, out.data_ptr(), int(pk),
                                             _lib.stream_handle(device))
    _lib.check(st, "isc_attention_f16_probe")
    full = vb.unpack_all(out.cpu(), b, d) if pk else out.cpu()
    assert torch.equal(full[b:], torch.full_like(full[b:], SENTINEL)), "rows behind the output were written"
    assert torch.equal(qd.cpu(), q)
    return full[:b]


@PK
@SHAPES
def test_probe_uniform_is_the_mean_over_exactly_the_images_rows(device, heads, t, pk):
    """One leaked or lost key moves the divisor by 1 / T; a key of the neighbouring image moves the sum."""
    c = so.probe_uniform_case(PROBE_B, t, heads, seed=2000 + t + heads)
    got = _run_probe(device, c["kv"], c["q"], heads, pk)
    name = f"probe uniform T = {t}, {heads} heads"
    _note(name, mb.assert_within_bound(got, c["want"], c["bound"], name))


@PK
@SHAPES
def test_probe_selector_equals_the_gather(device, heads, t, pk):
    c = so.probe_selector_case(PROBE_B, t, heads, seed=1000 + t + heads)
    assert torch.equal(_run_probe(device, c["kv"], c["q"], heads, pk), c["want"])


@functools.lru_cache(maxsize=1)
def _probe_random(heads: int, t: int, scale: float):
    kv, q = so.probe_random_case(PROBE_B, t, heads, scale, seed=3000 + t + heads)
    return (kv, q, *so.probe_reference(kv, q, heads))


@PK
@pytest.mark.parametrize("scale", [1.0, 0.25], ids=["peaked", "flat"])
@SHAPES
def test_probe_random_is_within_the_derived_bound(device, heads, t, scale, pk):
    kv, q, want, bound = _probe_random(heads, t, scale)
    got = _run_probe(device, kv, q, heads, pk)
    name = f"probe randn * {scale}, T = {t}, {heads} heads"
    _note(name, mb.assert_within_bound(got, want, bound, name))


@PK
@SHAPES
def test_probe_images_are_isolated(device, heads, t, pk):
    """NaN in the kv rows of the OTHER images, or behind the B * T rows of an over-allocated operand, leaves an image's
    output bit-identical; B = 3 equals its three B = 1 calls bit for bit."""
    kv, q, _want, _bound = _probe_random(heads, t, 1.0)
    clean = _run_probe(device, kv, q, heads, pk)
    assert torch.isfinite(clean.float()).all()
    for i in range(PROBE_B):
        poisoned = torch.full_like(kv, NAN)
        poisoned[i] = kv[i]
        got = _run_probe(device, poisoned, q, heads, pk)
        assert torch.equal(got[i], clean[i]), f"image {i} saw its neighbours"
        assert torch.equal(_run_probe(device, kv[i : i + 1], q, heads, pk)[0], clean[i]), f"image {i} alone differs"
    # packed: the padding rows of the tile are NaN in every call above; row-major: 40 rows of NaN / of 60000 behind
    if not pk:
        for fill in (NAN, 60000.0):
            assert torch.equal(_run_probe(device, kv, q, heads, pk, tail_rows=40, tail_fill=fill), clean)


def test_probe_beyond_one_chunk_of_keys(device):
    """T = 4097 and 8200: the running maximum across chunks of 4096 keys.  Uniform, selector (the chosen key in the last
    chunk for one image, in the first for another) and random operands, packed."""
    for t in (4097, 8200):
        c = so.probe_uniform_case(2, t, PROBE_HEADS, seed=t)
        mb.assert_within_bound(_run_probe(device, c["kv"], c["q"], PROBE_HEADS, True), c["want"], c["bound"], f"uniform T = {t}")
        c = so.probe_selector_case(PROBE_B, t, PROBE_HEADS, seed=t + 1)
        assert torch.equal(_run_probe(device, c["kv"], c["q"], PROBE_HEADS, True), c["want"])
        kv, q = so.probe_random_case(2, t, PROBE_HEADS, 0.5, seed=t + 2)
        want, bound = so.probe_reference(kv, q, PROBE_HEADS)
        _note(f"probe T = {t}", mb.assert_within_bound(_run_probe(device, kv, q, PROBE_HEADS, True), want, bound, f"T = {t}"))


@PK
def test_probe_captured_graph_replays_to_the_same_bits(device, pk):
    from imagescry_amd import _lib

    heads, t, d = 12, 196, 768
    kv, q, _want, _bound = _probe_random(heads, t, 1.0)
    eager = _run_probe(device, kv, q, heads, pk)
    kd = (vb.pack_padded(kv.reshape(-1, 2 * d), NAN) if pk else kv.reshape(-1, 2 * d)).to(device)
    qd = q.to(device)
    out = torch.full((256 * d,) if pk else (PROBE_B, d), NAN, dtype=torch.float16, device=device)
    lib = _lib.load()

    def run():
        _lib.check(lib.isc_attention_f16_probe(kd.data_ptr(), qd.data_ptr(), PROBE_B, t, heads, 64, out.data_ptr(), int(pk),
                                               _lib.stream_handle(device)), "isc_attention_f16_probe")

    run()
    torch.cuda.synchronize(device)
    stream = torch.cuda.Stream(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        run()
    for _ in range(2):
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize(device)
        got = vb.unpack_all(out.cpu(), PROBE_B, d)[:PROBE_B] if pk else out.cpu()
        assert torch.equal(got, eager)


# ============================================================================================ isc_vit_assemble_plain
@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("p", [1, 196])
@pytest.mark.parametrize("b", [1, 3])
def test_plain_assemble_is_one_addition_per_element(device, b, p, d):
    from imagescry_amd import _lib

    g = vb.gen(b + p + d)
    pe, pos = torch.randn(b * p, d, generator=g), torch.randn(p + 2, d, generator=g)  # more position rows than P
    ped, posd = pe.to(device), pos.to(device)
    out = torch.full((b * p + 1, d), NAN, dtype=torch.float32, device=device)
    out[b * p] = SENTINEL
    st = _lib.load().isc_vit_assemble_plain(ped.data_ptr(), posd.data_ptr(), b, p, d, out.data_ptr(), _lib.stream_handle(device))
    _lib.check(st, "isc_vit_assemble_plain")
    out = out.cpu()
    assert torch.equal(out[b * p], torch.full((d,), SENTINEL)), "the row behind the output was written"
    assert torch.equal(out[: b * p].reshape(b, p, d), pe.reshape(b, p, d) + pos[:p])
    assert torch.equal(ped.cpu(), pe) and torch.equal(posd.cpu(), pos)


@pytest.mark.parametrize("grid", [(4, 6), (14, 14), (16, 16), (11, 17)])
def test_resampled_table_matches_interpolate(device, grid):
    """The table a prepared tower without a class token hands to isc_vit_assemble_plain: rows 1 .. of `vit.position_table`
    (isc_vit_pos_resample behind one zero row), against `F.interpolate` at the tolerance of
    tests/test_gpu_vit_tokens.py::test_pos_resample_matches_interpolate."""
    import dataclasses

    from imagescry_amd import siglip, vit

    cfg = dataclasses.replace(siglip.PRESETS["ViT-B/16"].vision, depth=0)
    sd = vit.make_state_dict(cfg, seed=grid[0])
    net = vit.prepare(sd, cfg).to(device)
    table = vit.position_table(net, grid).cpu()
    assert table.shape == (1 + grid[0] * grid[1], 768) and not table[0].any()
    pos = sd["pos_embed"][0]
    want = so.interpolate_pos(pos, grid)
    if grid == (14, 14):
        assert torch.equal(table[1:], pos)
        return
    err = (table[1:] - want).abs().max().item()
    bound = 64 * 2.0**-24 * pos.abs().max().item()
    print(f"SigLIP pos_resample {grid}: max|err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ====================================================================================================== the model
def _unit(x: torch.Tensor) -> torch.Tensor:
    return F.normalize(x, dim=1)


def _model(monkeypatch, device, preset: str, **kw):
    """`SigLIPEmbedder(preset)` at two layers a tower and a vocabulary of `so.TEST_VOCAB` (the preset table is patched, as
    tests/test_gpu_clip.py patches CLIP's) with seeded random weights, biases and LayerNorm affines."""
    from imagescry_amd import SigLIPEmbedder, siglip

    cfg, sd = so.shallow(preset)
    monkeypatch.setitem(siglip.PRESETS, preset, cfg)
    model = SigLIPEmbedder(preset, state_dict=sd, **kw).to(device)
    assert model.siglip_config == cfg and len(model._net.encoder.blocks) == so.MODEL_DEPTH == len(model._text.blocks)
    return model, cfg, sd


def _check_model(what: str, got: torch.Tensor, want: torch.Tensor, want16: torch.Tensor, e: int) -> None:
    scale = math.sqrt(768 / e)
    err, err16 = (got - want).abs().max().item(), (got - want16).abs().max().item()
    print(f"{what}: max|err| f32 oracle {err:.3e} (bound {1e-2 * scale:.2e}, ratio {err / (1e-2 * scale):.3f}), "
          f"fp16-operand oracle {err16:.3e} (bound {2e-3 * scale:.2e}, ratio {err16 / (2e-3 * scale):.3f}), "
          f"1 - min cosine {1 - (got * want).sum(dim=1).min().item():.2e}")
    assert err < 1e-2 * scale
    assert err16 < 2e-3 * scale
    assert torch.allclose(got.norm(dim=1), torch.ones(got.shape[0]), atol=1e-5)


@pytest.mark.parametrize("preset,shape,grid,max_patches,tokens", so.IMAGE_CASES)
def test_image_tower_matches_oracle(device, monkeypatch, preset, shape, grid, max_patches, tokens):
    from imagescry_amd import ImageBatch, vit

    kw = dict(grid="aspect", max_patches=max_patches) if grid == "aspect" else {}
    model, cfg, sd = _model(monkeypatch, device, preset, **kw)
    if grid == "aspect":
        assert vit.token_grid(*shape, max_patches) == (shape[0] // 16, shape[1] // 16)
    assert (shape[0] // 16) * (shape[1] // 16) == tokens
    images = co.model_images(so.MODEL_BATCH, *shape, seed=tokens)
    ib = ImageBatch(indices=torch.arange(so.MODEL_BATCH), images=images).to(device)
    e = model.predict_step(ib).embeddings
    assert e.shape == (so.MODEL_BATCH, cfg.embed_dim, 1, 1) and e.dtype == torch.float32 and model.embedding_dim == cfg.embed_dim
    x = so.preprocess_reference(images)
    torch.testing.assert_close(model.preprocess(ib.images).cpu(), x, rtol=1e-6, atol=1e-6)  # fixed statistics, no clipping
    okw = dict(patch=16, heads=cfg.vision.heads)
    with torch.no_grad():
        want = _unit(so.siglip_image_features(sd, x, **okw))
        want16 = _unit(so.siglip_image_features(sd, x, round_operands_fp16=True, **okw))
    _check_model(f"SigLIP {preset} {shape} (T = {tokens})", e.reshape(so.MODEL_BATCH, -1).cpu(), want, want16, cfg.embed_dim)


@pytest.mark.parametrize("preset", ["ViT-B/16", "ViT-L/16@256"])
def test_text_tower_matches_oracle(device, monkeypatch, preset):
    """T = context; a short T padded to the context (the default) and run at its own length; int32 ids on the device
    without validation give the same bits."""
    model, cfg, sd = _model(monkeypatch, device, preset)
    text = cfg.text
    okw = dict(heads=text.heads)
    for t, pad in ((text.context, True), (20, True), (20, False)):
        ids = torch.randint(2, text.vocab, (so.TEXT_QUERIES, t), generator=vb.gen(t + int(pad)))
        got = model.encode_text(ids, pad_to_context=pad)  # CPU ids are copied over
        assert got.shape == (so.TEXT_QUERIES, cfg.embed_dim) and got.dtype == torch.float32 and got.device == model.device
        assert torch.equal(model.encode_text(ids.to(device).int(), validate=False, pad_to_context=pad), got)
        raw = model.encode_text(ids, normalize=False, pad_to_context=pad)
        assert torch.allclose(F.normalize(raw, dim=1), got, atol=1e-6) and not torch.equal(raw, got)
        run = so.pad_ids(ids, text.context, text.pad_token_id) if pad else ids
        with torch.no_grad():
            want = _unit(so.siglip_text_features(sd, run, **okw))
            want16 = _unit(so.siglip_text_features(sd, run, round_operands_fp16=True, **okw))
        _check_model(f"SigLIP {preset} text T = {t}, pad_to_context = {pad}", got.cpu(), want, want16, cfg.embed_dim)
        if t < text.context:  # the two modes are different functions of a short row, and padding by hand is the default
            assert not torch.equal(model.encode_text(ids, pad_to_context=not pad), got)
            assert torch.equal(model.encode_text(so.pad_ids(ids, text.context, text.pad_token_id)),
                               model.encode_text(ids, pad_to_context=True))
    bad = torch.randint(2, text.vocab, (4, 9), generator=vb.gen(1))
    bad[1, 2], bad[3, 0] = text.vocab, -1
    with pytest.raises(ValueError, match="2 token id"):
        model.encode_text(bad)
    assert model.encode_text(bad, validate=False).shape == (4, cfg.embed_dim)  # no host read, no fault


def test_checkpoint_preprocess_is_the_antialiased_squash(device, monkeypatch):
    """`preprocess="checkpoint"`: every element is (level - 127.5) / 127.5 with `level` one of the uint8 levels
    rint(clamp(v)) of the values v within `aa_image_bound` of the float64 antialiased squash to (224, 224) -- the check of
    tests/test_gpu_preprocess_aa.py::test_quantize_gives_the_allowed_uint8_levels -- and the same bits as the transform."""
    from imagescry_amd import ImageBatch, l2_normalize_channels, resize_antialias

    model, cfg, _sd = _model(monkeypatch, device, "ViT-B/16", preprocess="checkpoint")
    assert model.hparams["preprocess"] == "checkpoint"
    images = co.model_images(2, 300, 190, 91)
    x = model.preprocess(images.to(device))
    assert x.shape == (2, 3, 224, 224) and x.dtype == torch.float32
    half = torch.full((3,), 127.5, device=device)
    assert torch.equal(x, resize_antialias(images.to(device), (224, 224), channel_means=half, channel_stds=half, quantize=True))
    raw = x.cpu().double() * 127.5 + 127.5
    levels = raw.round()
    assert (raw - levels).abs().max().item() < 1e-4  # x is a normalised uint8 level (float32: 2^-24 * 255 of it)
    ref = resize_aa_f64(images, 224, 224)
    bound = aa_image_bound(300, 190, 224, 224)
    lo, hi = torch.round((ref - bound).clamp(0, 255)), torch.round((ref + bound).clamp(0, 255))
    assert levels.min().item() >= 0 and levels.max().item() <= 255
    assert bool(((levels >= lo) & (levels <= hi)).all()) and bool((hi - lo <= 1).all())
    got = model.predict_step(ImageBatch(images=images.to(device), indices=torch.arange(2, device=device))).embeddings
    assert torch.equal(got, l2_normalize_channels(model.forward(x)))
    squash = _model(monkeypatch, device, "ViT-B/16")[0]
    assert not torch.equal(squash.preprocess(images.to(device)), x)


def test_batch_of_five_in_passes_of_two_equals_its_slices(device, monkeypatch):
    from imagescry_amd import SigLIPEmbedder, vit

    model, cfg, sd = _model(monkeypatch, device, "ViT-B/16", max_images_per_pass=2)
    x = model.preprocess(co.model_images(5, 224, 224, seed=5).to(device))
    full = model(x)  # three passes: 2 + 2 + 1 images
    assert full.shape == (5, cfg.embed_dim, 1, 1)
    one_pass = SigLIPEmbedder("ViT-B/16", state_dict=sd).to(device)
    assert torch.equal(one_pass(x), full) and torch.equal(torch.cat([one_pass(x[:3]), one_pass(x[3:])]), full)
    ids = torch.randint(2, cfg.text.vocab, (5, 20), generator=vb.gen(6))
    whole = model.encode_text(ids)
    monkeypatch.setattr(vit, "PASS_ROWS", 2 * cfg.text.context)  # two sequences a pass
    assert torch.equal(model.encode_text(ids), whole)
    assert torch.equal(torch.cat([model.encode_text(ids[i : i + 1]) for i in range(5)]), whole)


# ====================================================================================================== end to end
def test_text_queries_search_an_image_bank_and_probabilities(device, monkeypatch):
    """Every score is within ||q_gpu - q_oracle|| + ||r_gpu - r_oracle|| + 1e-6 of the oracle's cosine (Cauchy-Schwarz on
    unit vectors, tests/test_gpu_clip.py); the probability is sigmoid(a cos + b) with a = exp(logit_scale), and sigmoid has
    slope <= 1/4, so it moves by at most a / 4 times that.  `search_range` at the cosine of a probability p midway in the
    largest gap of the oracle's probabilities returns exactly the pairs whose oracle probability clears p."""
    from imagescry_amd import EmbeddingBank, ImageBatch

    model, cfg, sd = _model(monkeypatch, device, "ViT-B/16")
    images = co.model_images(6, 224, 224, seed=60)
    batches = [ImageBatch(indices=torch.arange(i, i + 3), images=images[i : i + 3]).to(device) for i in (0, 3)]
    bank = EmbeddingBank.from_batches([model.predict_step(b) for b in batches], dtype=torch.float32)
    assert bank.num_local_rows == 6 and bank.dim == cfg.embed_dim
    ids = torch.randint(2, cfg.text.vocab, (4, 12), generator=vb.gen(61))
    q = model.encode_text(ids)
    scores, idx = bank.search(q, k=6)
    assert sorted(idx[0].tolist()) == list(range(6))
    with torch.no_grad():
        r_want = _unit(so.siglip_image_features(sd, so.preprocess_reference(images), patch=16, heads=cfg.vision.heads))
        q_want = _unit(so.siglip_text_features(sd, so.pad_ids(ids, cfg.text.context, cfg.text.pad_token_id), heads=cfg.text.heads))
    rows = torch.cat([model.predict_step(b).embeddings for b in batches]).reshape(6, -1).cpu()
    dq, dr = (q.cpu() - q_want).norm(dim=1), (rows - r_want).norm(dim=1)
    cos = q_want @ r_want.T  # [4, 6]
    p_want = so.probability(cos, sd)
    idx, scores = idx.cpu(), scores.cpu()
    prob = model.probability(scores)
    assert prob.shape == scores.shape and torch.equal(model.probability(scores.to(device)).cpu(), prob)
    a = math.exp(model.logit_scale)
    assert a == pytest.approx(40.0) and model.logit_bias == -1.5
    for i in range(4):
        slack = dq[i] + dr[idx[i]] + 1e-6
        assert bool(((scores[i] - cos[i, idx[i]]).abs() <= slack).all()), (i, scores[i], cos[i, idx[i]], slack)
        assert bool(((prob[i].double() - p_want[i, idx[i]]).abs() <= a / 4 * slack.double() + 1e-6).all()), (i, prob[i], p_want[i])
    print(f"text -> image search: |dq| <= {dq.max().item():.2e}, |dr| <= {dr.max().item():.2e}, probabilities "
          f"{p_want.min().item():.3f} .. {p_want.max().item():.3f}, probability error <= "
          f"{(prob.double() - p_want.gather(1, idx)).abs().max().item():.2e}")
    # the threshold: midway in the largest gap of the sorted oracle probabilities, so that rounding moves no pair across
    flat = p_want.flatten().sort().values
    gaps = flat[1:] - flat[:-1]
    at = int(gaps.argmax())
    p = float((flat[at] + flat[at + 1]) / 2)
    need = a / 4 * float((dq.max() + dr.max() + 1e-6))
    assert float(gaps[at]) / 2 > need, f"the largest gap {float(gaps[at]):.3e} does not clear the model bound {need:.3e}"
    found = bank.search_range(q, min_score=model.score_for_probability(p))
    for i in range(4):
        got = sorted(found.indices[found.offsets[i] : found.offsets[i + 1]].tolist())
        assert got == sorted(torch.nonzero(p_want[i] > p).flatten().tolist()), (i, p)
    assert 0 < int(found.offsets[-1]) < 24  # the threshold cuts the table somewhere inside


def test_earlier_embedders_are_untouched_by_siglip_instances(device, monkeypatch):
    import dataclasses

    from imagescry_amd import CLIPEmbedder, DINOv2Embedder, ImageBatch, ViTB16Embedder, clip, embedding, vit

    ib = ImageBatch(indices=torch.arange(3), images=co.model_images(3, 120, 90, seed=2)).to(device)
    default = ViTB16Embedder(seed=1).to(device)  # the default configuration
    aspect = ViTB16Embedder(seed=1, output="patches", grid="aspect").to(device)
    dcfg = dataclasses.replace(embedding.DINOV2_PRESETS["vits14", True], depth=2)
    monkeypatch.setitem(embedding.DINOV2_PRESETS, ("vits14", True), dcfg)
    dino = DINOv2Embedder("vits14", True, state_dict=vit.make_state_dict(dcfg, seed=3, randomize_affine=True),
                          output="patches", grid="aspect", max_patches=64).to(device)
    ccfg, csd = co.shallow("ViT-B/32")
    monkeypatch.setitem(clip.PRESETS, "ViT-B/32", ccfg)
    cl = CLIPEmbedder("ViT-B/32", state_dict=csd).to(device)
    cids, _ = co.text_ids(3, 9, ccfg.text.vocab, seed=4)
    before = [m.predict_step(ib).embeddings.clone() for m in (default, aspect, dino, cl)] + [cl.encode_text(cids).clone()]
    for preset, kw in (("ViT-B/16", dict(grid="aspect")), ("ViT-L/16@256", {})):
        m, cfg, _sd = _model(monkeypatch, device, preset, **kw)
        assert m.predict_step(ib).embeddings.shape == (3, cfg.embed_dim, 1, 1)
        assert m.encode_text(torch.randint(2, cfg.text.vocab, (3, 9), generator=vb.gen(4))).shape == (3, cfg.embed_dim)
    after = [m.predict_step(ib).embeddings for m in (default, aspect, dino, cl)] + [cl.encode_text(cids)]
    for a, b in zip(before, after):
        assert torch.equal(a, b)
