"""Times the outlines of connected regions on the GPU, per shape and input:

  (t)  segmentation.trace_regions(ids, R)            rings, areas and counts: 11 + ceil(log2(4 H W)) launches
  (r)  segmentation.label_regions(maps.labels)       the call before it, which produced the ids
  (c)  ids.cpu()                                     the copy any host tracer pays before it starts

on the two inputs of scripts/bench_label_regions.py: `blobby`, the labels `label_map` gives for smooth random score grids
(a few dozen regions an image), and `serpentine`, a one-pixel path through every image: one ring of about 2 H vertices
that runs through every row.  (t) and (r) run in one process, alternating, with device events after a warm-up, each
window of time `--window` seconds of back-to-back calls, `--rounds` of them a path; (c) is timed on the host clock
around the synchronised copy.  Before timing, (t)'s rings are rasterised again on the device and compared with the ids,
and every image must fit its capacities.  Prints per shape and input the medians with the spread and one JSON line.

    python scripts/bench_trace_regions.py [--window 0.5] [--rounds 5]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from imagescry_amd import label_map, label_regions, rasterize_polygons, trace_regions  # noqa: E402

# (B, C, h, w, H, W): the shapes of scripts/bench_label_regions.py
SHAPES = [(64, 150, 14, 14, 448, 448), (512, 21, 7, 7, 224, 224)]
ROWS = 1024  # the default max_regions of label_regions


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


def copy_seconds(ids: torch.Tensor, rounds: int) -> list[float]:
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids.cpu()
        out.append(time.perf_counter() - t0)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trace_regions.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    results = []
    for b, c, h, w, big_h, big_w in SHAPES:
        g = torch.Generator().manual_seed(b + c)
        noise = torch.randn(b * c, 1, h, w, generator=g)
        smooth = F.avg_pool2d(F.pad(noise, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
        scores = smooth.reshape(b, c, h, w).permute(0, 2, 3, 1).contiguous().to(dev)
        inputs = (("blobby", label_map(scores, (big_h, big_w)).labels), ("serpentine", serpentine(b, big_h, big_w, dev)))
        del scores
        for name, labels in inputs:
            ids = label_regions(labels, max_regions=ROWS).ids
            paths = {"t": lambda: trace_regions(ids, ROWS), "r": lambda: label_regions(labels, max_regions=ROWS)}
            found = paths["t"]()
            fits = bool(found.complete().all())
            back = rasterize_polygons(found.packed, found.size, num_regions=ROWS)
            ok = fits and torch.equal(back, torch.where(ids < ROWS, ids, torch.full_like(ids, -1)))
            rings, vertices = found.num_rings.cpu(), found.num_vertices.cpu()
            del found, back
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
            times["c"] = copy_seconds(ids, args.rounds)
            med = {k: statistics.median(v) for k, v in times.items()}
            print(f"{b} x {big_h} x {big_w}, {name}: {float(rings.float().mean()):.1f} rings and "
                  f"{float(vertices.float().mean()):.1f} vertices an image (max {int(rings.max())}, {int(vertices.max())}); "
                  f"rasterising the rings {'gives back' if ok else 'DOES NOT GIVE BACK'} the ids")
            for k, label in (("t", "(t)  trace_regions           "), ("r", "(r)  label_regions, no scores"),
                             ("c", "(c)  ids.cpu()               ")):
                print(f"  {label}: median {med[k] * 1e6:10.1f} us  (min {min(times[k]) * 1e6:.1f} .. max "
                      f"{max(times[k]) * 1e6:.1f}, {args.rounds} windows" + (f" of {iters[k]} calls)" if k in iters else ")"))
            print(f"  (t) / (r) = {med['t'] / med['r']:.2f}, (c) / (t) = {med['c'] / med['t']:.2f}, "
                  f"{b * big_h * big_w / med['t'] / 1e9:.2f} G pixels/s", flush=True)
            results.append({"shape": [b, big_h, big_w], "input": name, "t_us": [x * 1e6 for x in times["t"]],
                            "r_us": [x * 1e6 for x in times["r"]], "copy_us": [x * 1e6 for x in times["c"]],
                            "rings_mean": float(rings.float().mean()), "vertices_mean": float(vertices.float().mean()),
                            "round_trip": ok})
            del ids
    print(json.dumps({"bench": "trace_regions", "results": results}))


if __name__ == "__main__":
    main()
