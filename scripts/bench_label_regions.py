"""Times the connected regions of pixel label maps on the GPU, per shape and input:

  (r)  segmentation.label_regions(maps)              ids, counts, every table and the peaks: up to nine launches
  (r-) segmentation.label_regions(maps.labels)       the same without scores: no peaks
  (m)  segmentation.label_map(scores, (H, W))        the kernel that produced the map, at the same output size
  (s)  labels.cpu() + scipy.ndimage.label per class present and image (8-connectivity), what this replaces: timed on
       the first `--host-images` images including their copy to the host, and scaled to the batch

on two inputs: `blobby`, the labels `label_map` gives for smooth random score grids (3 x 3 box-filtered noise on the
cell grid: a few dozen regions an image), and `serpentine`, a one-pixel path through every image, the longest chains the
union-find can meet.  (r), (r-) and (m) run in one process, alternating, with device events after a warm-up, each window
of time `--window` seconds of back-to-back calls, `--rounds` of them a path.  Before timing, (r)'s regions are compared
with scipy's on the first image: the same count, and per class a one-to-one match of the components.
Prints per shape and input the medians with the spread and one JSON line.

    python scripts/bench_label_regions.py [--window 0.5] [--rounds 5] [--host-images 8]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from imagescry_amd import LabelMaps, label_map, label_regions  # noqa: E402

# (B, C, h, w, H, W): the shapes of the label-map sections -- ADE20K's 150 classes on 448 x 448, 21 classes on 224 x 224
SHAPES = [(64, 150, 14, 14, 448, 448), (512, 21, 7, 7, 224, 224)]


def timed(fn, iters: int) -> float:
    """Seconds per call over `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def serpentine(b: int, h: int, w: int, dev: torch.device) -> torch.Tensor:
    m = torch.full((h, w), 255, dtype=torch.uint8)
    m[0::2] = 3
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 3
    return m.expand(b, h, w).contiguous().to(dev)


def host_regions(labels: torch.Tensor, images: int):
    """scipy.ndimage.label per class present on the first `images` images -> (seconds, component arrays of image 0)."""
    from scipy import ndimage

    structure = np.ones((3, 3), int)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = labels[:images].cpu().numpy()
    first = {}
    for i in range(host.shape[0]):
        for c in np.unique(host[i]):
            if c == 255:
                continue
            comp, n = ndimage.label(host[i] == c, structure=structure)
            if i == 0:
                first[int(c)] = (comp, n)
    return time.perf_counter() - t0, first


def agrees_with_scipy(regions, first: dict) -> bool:
    ids = regions.ids[0].cpu().numpy()
    total = 0
    for comp, n in first.values():
        inside = comp > 0
        pairs = np.unique(np.stack([comp[inside], ids[inside]]), axis=1)
        if pairs.shape[1] != n or len(np.unique(pairs[1])) != n or (ids[inside] < 0).any():
            return False
        total += n
    return total == int(regions.num[0])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_regions.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    results = []
    for b, c, h, w, big_h, big_w in SHAPES:
        g = torch.Generator().manual_seed(b + c)
        noise = torch.randn(b * c, 1, h, w, generator=g)
        smooth = F.avg_pool2d(F.pad(noise, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
        scores = smooth.reshape(b, c, h, w).permute(0, 2, 3, 1).contiguous().to(dev)
        blobby = label_map(scores, (big_h, big_w))
        snake = LabelMaps(labels=serpentine(b, big_h, big_w, dev), scores=blobby.scores)
        for name, maps in (("blobby", blobby), ("serpentine", snake)):
            paths = {"r": lambda: label_regions(maps), "r-": lambda: label_regions(maps.labels),
                     "m": lambda: label_map(scores, (big_h, big_w))}
            found = paths["r"]()
            host_s, first = host_regions(maps.labels, min(args.host_images, b))
            ok = agrees_with_scipy(found, first)
            num = found.num.cpu()
            del found
            times = {k: [] for k in paths}
            iters = {}
            for k, fn in paths.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                iters[k] = max(5, int(args.window / timed(fn, 3)) + 1)
            for _ in range(args.rounds):
                for k, fn in paths.items():
                    times[k].append(timed(fn, iters[k]))
            med = {k: statistics.median(v) for k, v in times.items()}
            host_batch = host_s * b / min(args.host_images, b)
            print(f"{b} x {big_h} x {big_w}, {c} classes, {name}: {float(num.float().mean()):.1f} regions an image (max "
                  f"{int(num.max())}); regions {'agree' if ok else 'DISAGREE'} with scipy.ndimage.label on image 0")
            for k, label in (("r", "(r)  label_regions, all tables"), ("r-", "(r-) label_regions, no scores "),
                             ("m", "(m)  label_map                ")):
                print(f"  {label}: median {med[k] * 1e6:10.1f} us  (min {min(times[k]) * 1e6:.1f} .. max "
                      f"{max(times[k]) * 1e6:.1f}, {args.rounds} windows of {iters[k]} calls)")
            print(f"  (s)  copy + scipy per class    : {host_batch * 1e6:10.1f} us for the batch ({min(args.host_images, b)} images "
                  f"timed once: {host_s * 1e3:.1f} ms); (r) / (m) = {med['r'] / med['m']:.2f}, (s) / (r) = "
                  f"{host_batch / med['r']:.0f}, {b * big_h * big_w / med['r'] / 1e9:.2f} G pixels/s", flush=True)
            results.append({"shape": [b, c, h, w, big_h, big_w], "input": name, "r_us": [x * 1e6 for x in times["r"]],
                            "r_no_scores_us": [x * 1e6 for x in times["r-"]], "m_us": [x * 1e6 for x in times["m"]],
                            "scipy_batch_us": host_batch * 1e6, "scipy_images_timed": min(args.host_images, b),
                            "regions_mean": float(num.float().mean()), "regions_max": int(num.max()), "agrees": ok})
        del scores, blobby, snake
    print(json.dumps({"bench": "label_regions", "results": results}))


if __name__ == "__main__":
    main()
