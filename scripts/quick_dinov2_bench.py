"""Cost of the DINOv2 backbones (not the contract bench):

* the LayerScale epilogue -- isc_gemm_f16_scaled against isc_gemm_f16 on the same operands (ViT-B `proj` and `fc2`,
  M = 512 x 261 token rows, float32 output + residual), and against what it replaces: the GEMM without residual followed
  by a separate `out = residual + scale * y` pass over the residual stream (torch.addcmul here; ~3 M N 4 bytes);
* `predict_step` at batch 512, 224 x 224, output="patches" (a 16 x 16 map, 257 / 261 tokens) for vits14 / vitb14 / vitl14
  with and without registers, next to `ViTB16Embedder` (14 x 14, 197 tokens); all models interleaved in one process.

    python scripts/quick_dinov2_bench.py [--rounds 3] [--steps 3] [--gemm-only | --models-only]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import DINOv2Embedder, ImageBatch, ViTB16Embedder, _lib
from imagescry_amd.vit import packed_elems


def arg(name: str, default: int) -> int:
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


dev = torch.device("cuda:0")
lib = _lib.load()
s = _lib.stream_handle(dev)
rounds, steps = arg("--rounds", 3), arg("--steps", 3)
b = 512


def timed(fn, n: int) -> float:
    """milliseconds per call, device events around n calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def median(ts: list[float]) -> float:
    return sorted(ts)[len(ts) // 2]


if "--models-only" not in sys.argv:
    m = b * 261
    flags = _lib.ISC_GEMM_A_PACKED | _lib.ISC_GEMM_W_PACKED
    for name, k, n in (("proj", 768, 768), ("fc2", 3072, 768)):
        a = (torch.randn(packed_elems(m, k), device=dev) * 0.5).half()
        w = (torch.randn(packed_elems(n, k), device=dev) * 0.02).half()
        bias, scale = torch.randn(n, device=dev) * 0.05, torch.rand(n, device=dev)
        res, out, tmp = torch.randn(m, n, device=dev), torch.empty(m, n, device=dev), torch.empty(m, n, device=dev)

        def plain() -> None:
            _lib.check(lib.isc_gemm_f16(a.data_ptr(), m, k, w.data_ptr(), n, bias.data_ptr(), res.data_ptr(),
                                        _lib.ISC_ACT_NONE, out.data_ptr(), _lib.ISC_F32, flags, s), "isc_gemm_f16")

        def scaled() -> None:
            _lib.check(lib.isc_gemm_f16_scaled(a.data_ptr(), m, k, w.data_ptr(), n, bias.data_ptr(), scale.data_ptr(),
                                               res.data_ptr(), _lib.ISC_ACT_NONE, out.data_ptr(), _lib.ISC_F32, flags, s),
                       "isc_gemm_f16_scaled")

        def gemm_only() -> None:
            _lib.check(lib.isc_gemm_f16(a.data_ptr(), m, k, w.data_ptr(), n, bias.data_ptr(), None, _lib.ISC_ACT_NONE,
                                        tmp.data_ptr(), _lib.ISC_F32, flags, s), "isc_gemm_f16")

        def scale_pass() -> None:
            torch.addcmul(res, tmp, scale, out=out)

        def separate() -> None:
            gemm_only()
            scale_pass()

        fns = {"isc_gemm_f16 (+ residual)": plain, "isc_gemm_f16_scaled (+ residual)": scaled,
               "isc_gemm_f16 then a scale-and-add pass": separate, "the scale-and-add pass alone": scale_pass}
        for fn in fns.values():
            timed(fn, 3)
        times = {key: [] for key in fns}
        for _ in range(max(rounds, 5)):  # alternated
            for key, fn in fns.items():
                times[key].append(timed(fn, 10))
        for key, ts in times.items():
            note = f", {2.0 * m * n * k / median(ts) / 1e9:.0f} TFLOP/s" if "pass alone" not in key else \
                   f", {3.0 * m * n * 4 / median(ts) / 1e9:.2f} TB/s over 3 M N 4 bytes"
            print(f"{name} M={m} K={k} N={n} {key}: median {median(ts) * 1e3:.1f} us, min {min(ts) * 1e3:.1f}, "
                  f"max {max(ts) * 1e3:.1f}{note}", flush=True)
        del a, w, res, out, tmp
    if "--gemm-only" in sys.argv:
        sys.exit(0)

images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
batch = ImageBatch(indices=torch.arange(b), images=images).to(dev)
models = {"ViTB16Embedder (14 x 14)": ViTB16Embedder(output="patches").to(dev)}
for variant in ("vits14", "vitb14", "vitl14"):
    for registers in (False, True):
        models[f"DINOv2Embedder {variant}{' + registers' if registers else ''} (16 x 16)"] = DINOv2Embedder(
            variant, registers, output="patches", grid="aspect", max_patches=256).to(dev)
for model in models.values():
    timed(lambda: model.predict_step(batch), 2)
times = {key: [] for key in models}
for _ in range(rounds):
    for key, model in models.items():
        times[key].append(timed(lambda: model.predict_step(batch), steps))
for key, ts in times.items():
    print(f"predict_step B={b} 224x224 output=patches {key}: median {median(ts):.2f} ms, min {min(ts):.2f}, max {max(ts):.2f} "
          f"-> {b / median(ts) * 1e3:.0f} img/s ({rounds} rounds x {steps} steps)", flush=True)
