"""Encode time of the dense CLIP patch map (not the contract bench), the numbers of DESIGN.md's dense-CLIP section:
`CLIPEmbedder("ViT-B/16", output="patches", dense=m)` for m in value / kk / qq against `output="cls"` on the same batch
of --batch (256) images of 224 x 224 -- `forward` on the preprocessed batch, so the four routes differ in the tower's
last block and its head only.

Device events, warm-up of every route, the routes interleaved, median and spread of --samples (20) samples of --reps
(3) calls each.  The weights are seeded random ones: the time does not depend on them.

    python scripts/bench_clip_dense.py [--batch 256] [--samples 20] [--reps 3]
"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import CLIPEmbedder, clip


def arg(name: str, default: int) -> int:
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


if not torch.cuda.is_available():
    sys.exit("bench_clip_dense.py needs a HIP device: a time from anywhere else says nothing")
dev = torch.device("cuda:0")
nb, samples, reps = arg("--batch", 256), arg("--samples", 20), arg("--reps", 3)
preset = "ViT-B/16"
cfg = clip.PRESETS[preset]
sd = clip.make_state_dict(cfg, seed=0)
models = {"cls": CLIPEmbedder(preset, state_dict=sd).to(dev)}
for m in ("value", "kk", "qq"):
    models[m] = CLIPEmbedder(preset, state_dict=sd, output="patches", dense=m).to(dev)
images = torch.randint(0, 256, (nb, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
x = models["cls"].preprocess(images)


def timed(fn, n: int) -> float:
    """milliseconds per call, device events around n calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


routes = {name: (lambda mod=mod: mod(x)) for name, mod in models.items()}
for name, fn in routes.items():
    shape = tuple(fn().shape)
    timed(fn, 2)
    print(f"{name}: output {shape}", flush=True)
ts = {name: [] for name in routes}
for _ in range(samples):
    for name, fn in routes.items():
        ts[name].append(timed(fn, reps))
med = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
t, d, e = cfg.vision.tokens, cfg.vision.dim, cfg.embed_dim
print(f"CLIP {preset}, batch {nb} x 224 x 224 ({t} tokens, D = {d}, E = {e}), forward, median of {samples} x {reps} calls:")
for name, v in ts.items():
    v = sorted(v)
    print(f"  {name:5s} {med[name]:8.2f} ms  (min {v[0]:.2f}, max {v[-1]:.2f})  {nb / med[name] * 1e3:7.0f} images/s  "
          f"{med[name] / med['cls']:.3f} x cls", flush=True)
# what the operation counts say: GEMM multiply-adds of the last block and the head, per image
block = 2 * t * d * 3 * d + 2 * t * d * d + 2 * 2 * t * d * cfg.vision.mlp_dim + 2 * 2 * t * t * d
dense = {"value": 2 * t * d * d, "kk": 2 * t * d * 3 * d + 2 * 2 * t * t * d, "qq": 2 * t * d * 3 * d + 2 * 2 * t * t * d}
for name, fl in dense.items():
    fl += 2 * t * d * d + 2 * t * d * e  # out_proj, the projection of every token
    print(f"  {name}: last block + head {fl / 1e9:.2f} GFLOP an image against {(block + 2 * d * e) / 1e9:.2f} for cls; "
          f"map write {4 * e * (t - 1) / 1e6:.2f} MB an image")
