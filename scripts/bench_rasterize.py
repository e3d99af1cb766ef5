"""Times polygon rasterisation on the GPU, per case, with and without `all_touched`:

  (z)  segmentation.rasterize_polygons(packed polygons on the device, (H, W))   the box pass and the tile kernel
  (c)  ... with return_counts=True                                              plus the zeroing launch and the atomics
  (p)  segmentation.pool_regions(maps, ids, R)                                  the call that follows, on the same ids
  (i)  PIL.ImageDraw.polygon per shape into an int32 image, the images stacked and uploaded: a CPU baseline on this
       script's host, per image with the upload included, timed on the first `--cpu-images` images and scaled to the
       batch.  PIL fills by another boundary rule, so this is a TIMING baseline only, never a correctness one.

Cases: 64 x 448 x 448 with 16 shapes of 32 vertices an image, 512 x 224 x 224 with 4 shapes of 16 vertices, and the
worst case for the staging, one 4096-vertex ring that spans every image of the first shape.  All paths run in one
process, alternating, with device events after a warm-up (host clock around a synchronise for (i)), `--rounds` timed
windows a path (at least 20), each of `--window` seconds of back-to-back calls.  Prints per case the medians with the
spread and one JSON line.

    python scripts/bench_rasterize.py [--window 0.2] [--rounds 20] [--cpu-images 8]
"""

from __future__ import annotations

import argparse
import json
import math
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from PIL import Image, ImageDraw  # noqa: E402

from imagescry_amd import pack_polygons, pool_regions, rasterize_polygons  # noqa: E402

# (name, B, H, W, shapes an image, vertices a shape, E, h, w)
CASES = [("16 shapes x 32 vertices", 64, 448, 448, 16, 32, 512, 28, 28),
         ("4 shapes x 16 vertices", 512, 224, 224, 4, 16, 768, 14, 14),
         ("one 4096-vertex ring", 64, 448, 448, 1, 4096, 512, 28, 28)]


def blob(rng: random.Random, n: int, cx: float, cy: float, radius: float) -> list[tuple[float, float]]:
    """A star-shaped outline of n vertices with jittered radii."""
    return [(cx + radius * rng.uniform(0.6, 1.0) * math.cos(2 * math.pi * i / n),
             cy + radius * rng.uniform(0.6, 1.0) * math.sin(2 * math.pi * i / n)) for i in range(n)]


def polygons(b: int, height: int, width: int, shapes: int, vertices: int, seed: int) -> list[list[list[tuple[float, float]]]]:
    rng = random.Random(seed)
    if shapes == 1:  # one ring over the whole image
        return [[blob(rng, vertices, width / 2, height / 2, 0.55 * max(height, width))] for _ in range(b)]
    return [[blob(rng, vertices, rng.uniform(0, width), rng.uniform(0, height), rng.uniform(0.08, 0.25) * width)
             for _ in range(shapes)] for _ in range(b)]


def timed(fn, iters: int) -> float:
    """Seconds per call over `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def pil_raster(polys: list, height: int, width: int, dev: torch.device) -> torch.Tensor:
    images = []
    for shapes in polys:
        image = Image.new("I", (width, height), -1)
        draw = ImageDraw.Draw(image)
        for region, ring in enumerate(shapes):
            draw.polygon(ring, fill=region)
        images.append(np.asarray(image, dtype=np.int32))
    out = torch.from_numpy(np.stack(images)).to(dev)
    torch.cuda.synchronize()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--cpu-images", type=int, default=8)
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit("--rounds: a median of fewer than 20 windows is not reported")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rasterize.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    results = []
    for name, b, height, width, shapes, vertices, e, h, w in CASES:
        polys = polygons(b, height, width, shapes, vertices, seed=b + vertices)
        pack = pack_polygons(polys).to(dev)
        rows = pack.num_regions
        maps = F.normalize(torch.randn(b, e, h, w, generator=torch.Generator().manual_seed(b)), dim=1).to(dev)
        nc = min(args.cpu_images, b)
        for touch in (False, True):
            ids, counts = rasterize_polygons(pack, (height, width), all_touched=touch, return_counts=True)
            covered = float((ids >= 0).float().mean())
            assert torch.equal(counts.sum(1), (ids >= 0).sum(dim=(1, 2)).to(torch.int32))
            paths = {"z": lambda: rasterize_polygons(pack, (height, width), all_touched=touch),
                     "c": lambda: rasterize_polygons(pack, (height, width), all_touched=touch, return_counts=True),
                     "p": lambda: pool_regions(maps, ids, rows)}
            times: dict[str, list[float]] = {k: [] for k in (*paths, "i")}
            iters = {}
            for k, fn in paths.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                iters[k] = max(3, int(args.window / timed(fn, 3)) + 1)
            pil_raster(polys[:nc], height, width, dev)
            for _ in range(args.rounds):
                for k, fn in paths.items():
                    times[k].append(timed(fn, iters[k]))
                t0 = time.perf_counter()
                pil_raster(polys[:nc], height, width, dev)
                times["i"].append((time.perf_counter() - t0) * b / nc)
            med = {k: statistics.median(v) for k, v in times.items()}
            print(f"{b} x {height} x {width}, {name}, all_touched={touch}: {covered:.2f} of the pixels covered")
            for k, label in (("z", "(z)  rasterize_polygons          "), ("c", "(c)  ... with counts            "),
                             ("p", "(p)  pool_regions on the ids    "),
                             ("i", f"(i)  PIL on {nc} images, scaled    ")):
                print(f"  {label}: median {med[k] * 1e6:10.1f} us  (min {min(times[k]) * 1e6:.1f} .. max "
                      f"{max(times[k]) * 1e6:.1f}, {args.rounds} windows" + (f" of {iters[k]} calls)" if k in iters else ")"))
            print(f"  (z) / (p) = {med['z'] / med['p']:.2f}, (i) / (z) = {med['i'] / med['z']:.0f}, "
                  f"{b * height * width / med['z'] / 1e9:.2f} G pixels/s", flush=True)
            results.append({"case": name, "shape": [b, height, width, shapes, vertices], "all_touched": touch,
                            "covered": covered, "cpu_images_timed": nc,
                            **{f"{k}_us": [x * 1e6 for x in v] for k, v in times.items()}})
    print(json.dumps({"bench": "rasterize", "results": results}))


if __name__ == "__main__":
    main()
