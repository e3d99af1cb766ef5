"""Times the overlap tables on the GPU, on the project's two standing batches (64 maps of 448 x 448 with 150 classes, 512
maps of 224 x 224 with 21 classes).  Per batch, three workloads:

  confusion   pred = the labels `label_map` gives for smooth random score grids, target = a shifted copy with an ignored
              band; C classes
    (n)  confusion_matrix(pred, target, C)               one table, batch-summed
    (N)  overlap_table(pred, target, C, C)               a table an image
    (t)  torch.bincount over the fused, clamped index    what (n) replaces: two int64 copies of every map
    (T)  ... with a per-image offset, reshaped           what (N) replaces
    (p)  label_map(scores, size)                         the call that produced the prediction
    (c)  pred.clone(); target.clone()                    a device copy of the same input bytes: the bandwidth floor
  noise       i.i.d. uniform classes in both inputs: every pixel its own run, the worst case -- (n), (N), (t), (T)
  match       a = label_regions(pred, max_regions=256).ids, b = 32 rasterised quadrilaterals an image
    (m)  match_regions(a, b, 256, 32)                    tables + the best partner of every region
    (M)  the torch composition                           bincount with a per-image offset, float64 IoU, argmax
    (r)  label_regions(pred, max_regions=256)            the call that produced a
    (c)  a.clone(); b.clone()
    and (m), (M) on i.i.d. noise ids

All paths of a workload run in one process, alternating, with device events after a warm-up, each window of time
`--window` seconds of back-to-back calls, `--rounds` of them a path.  Before timing, every new call is compared with the
torch composition it replaces, value for value.  Prints the medians with the spread and one JSON line.

    python scripts/bench_overlap.py [--window 0.3] [--rounds 5]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from imagescry_amd import (confusion_matrix, label_map, label_regions, match_regions, overlap_table,  # noqa: E402
                           rasterize_polygons)

# (B, C, h, w, H, W): the shapes of scripts/bench_label_regions.py
SHAPES = [(64, 150, 14, 14, 448, 448), (512, 21, 7, 7, 224, 224)]
ROWS = 256  # max_regions of label_regions
SHAPES_AN_IMAGE = 32  # drawn quadrilaterals


def timed(fn, iters: int) -> float:
    """Seconds per call over `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def clamped(v: torch.Tensor, num: int) -> torch.Tensor:
    v = v.long()
    return torch.where((v >= 0) & (v < num), v, torch.full_like(v, num))


def torch_table(a: torch.Tensor, b: torch.Tensor, ra: int, rb: int, per_image: bool) -> torch.Tensor:
    """The composition the new call replaces: bincount over the fused index."""
    fused = clamped(a, ra) * (rb + 1) + clamped(b, rb)
    size = (ra + 1) * (rb + 1)
    if not per_image:
        return torch.bincount(fused.reshape(-1), minlength=size).reshape(ra + 1, rb + 1)
    fused = fused + torch.arange(a.shape[0], device=a.device).reshape(-1, 1, 1) * size
    return torch.bincount(fused.reshape(-1), minlength=a.shape[0] * size).reshape(a.shape[0], ra + 1, rb + 1)


def torch_match(a: torch.Tensor, b: torch.Tensor, ra: int, rb: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    table = torch_table(a, b, ra, rb, True)
    inter = table[:, :ra, :rb]
    union = table.sum(dim=2)[:, :ra, None] + table.sum(dim=1)[:, None, :rb] - inter
    iou = torch.where(inter > 0, inter.double() / union.double(), torch.full_like(inter, -1, dtype=torch.float64))
    best = iou.argmax(dim=2, keepdim=True)
    hit = torch.gather(inter, 2, best) > 0
    return (torch.where(hit, best, torch.full_like(best, -1)).squeeze(2).int(), torch.gather(inter, 2, best).squeeze(2),
            torch.where(hit, torch.gather(union, 2, best), table.sum(dim=2)[:, :ra, None]).squeeze(2))


def quads(b: int, big_h: int, big_w: int, rng: np.random.Generator) -> list[list[np.ndarray]]:
    """32 convex quadrilaterals an image, a tenth of the image a side."""
    out = []
    for _ in range(b):
        shapes = []
        for _ in range(SHAPES_AN_IMAGE):
            cx, cy = rng.uniform(0, big_w), rng.uniform(0, big_h)
            rx, ry = rng.uniform(0.03, 0.1) * big_w, rng.uniform(0.03, 0.1) * big_h
            jitter = rng.uniform(0.7, 1.0, (4, 2))
            corners = np.array([[-rx, -ry], [rx, -ry], [rx, ry], [-rx, ry]]) * jitter + (cx, cy)
            shapes.append(corners)
        out.append(shapes)
    return out


def measure(paths: dict, window: float, rounds: int) -> tuple[dict, dict]:
    times, iters = {k: [] for k in paths}, {}
    for k, fn in paths.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(5, int(window / timed(fn, 3)) + 1)
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn, iters[k]))
    return times, iters


def report(title: str, labels: dict, times: dict, iters: dict, rounds: int) -> dict:
    print(title)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, label in labels.items():
        print(f"  ({k})  {label:<44}: median {med[k] * 1e6:10.1f} us  (min {min(times[k]) * 1e6:.1f} .. max "
              f"{max(times[k]) * 1e6:.1f}, {rounds} windows of {iters[k]} calls)")
    return med


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlap.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    results = []
    for b, c, h, w, big_h, big_w in SHAPES:
        g = torch.Generator().manual_seed(b + c)
        noise = torch.randn(b * c, 1, h, w, generator=g)
        smooth = F.avg_pool2d(F.pad(noise, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
        scores = smooth.reshape(b, c, h, w).permute(0, 2, 3, 1).contiguous().to(dev)
        pred = label_map(scores, (big_h, big_w)).labels
        target = torch.roll(pred, (3, 5), dims=(1, 2))
        target[:, :8] = 255  # an ignored band
        shape = f"{b} x {big_h} x {big_w}"
        pixels = b * big_h * big_w

        # ---- confusion
        assert torch.equal(confusion_matrix(pred, target, c), torch_table(pred, target, c, c, False))
        assert torch.equal(overlap_table(pred, target, c, c), torch_table(pred, target, c, c, True))
        paths = {"n": lambda: confusion_matrix(pred, target, c), "N": lambda: overlap_table(pred, target, c, c),
                 "t": lambda: torch_table(pred, target, c, c, False), "T": lambda: torch_table(pred, target, c, c, True),
                 "p": lambda: label_map(scores, (big_h, big_w)), "c": lambda: (pred.clone(), target.clone())}
        times, iters = measure(paths, args.window, args.rounds)
        med = report(f"{shape}, {c} classes, confusion",
                     {"n": "confusion_matrix", "N": "overlap_table, a table an image", "t": "torch.bincount, summed",
                      "T": "torch.bincount, per-image offset", "p": "label_map", "c": "pred.clone(); target.clone()"},
                     times, iters, args.rounds)
        print(f"  (t) / (n) = {med['t'] / med['n']:.2f}, (T) / (N) = {med['T'] / med['N']:.2f}, (n) / (p) = "
              f"{med['n'] / med['p']:.3f}, (n) / (c) = {med['n'] / med['c']:.2f}, {pixels / med['n'] / 1e9:.2f} G pixels/s",
              flush=True)
        results.append({"shape": [b, big_h, big_w], "classes": c, "workload": "confusion",
                        "us": {k: [x * 1e6 for x in v] for k, v in times.items()}})

        # ---- noise: every pixel its own run
        na = torch.randint(0, c, pred.shape, dtype=torch.uint8, device=dev)
        nb = torch.randint(0, c, pred.shape, dtype=torch.uint8, device=dev)
        assert torch.equal(overlap_table(na, nb, c, c), torch_table(na, nb, c, c, True))
        paths = {"n": lambda: confusion_matrix(na, nb, c), "N": lambda: overlap_table(na, nb, c, c),
                 "t": lambda: torch_table(na, nb, c, c, False), "T": lambda: torch_table(na, nb, c, c, True)}
        times, iters = measure(paths, args.window, args.rounds)
        med = report(f"{shape}, {c} classes, i.i.d. noise",
                     {"n": "confusion_matrix", "N": "overlap_table, a table an image", "t": "torch.bincount, summed",
                      "T": "torch.bincount, per-image offset"}, times, iters, args.rounds)
        print(f"  (t) / (n) = {med['t'] / med['n']:.2f}, (T) / (N) = {med['T'] / med['N']:.2f}", flush=True)
        results.append({"shape": [b, big_h, big_w], "classes": c, "workload": "confusion-noise",
                        "us": {k: [x * 1e6 for x in v] for k, v in times.items()}})
        del na, nb

        # ---- match
        ids = label_regions(pred, max_regions=ROWS).ids
        drawn = rasterize_polygons(quads(b, big_h, big_w, np.random.default_rng(b)), (big_h, big_w), device=dev)
        m, ref = match_regions(ids, drawn, ROWS, SHAPES_AN_IMAGE), torch_match(ids, drawn, ROWS, SHAPES_AN_IMAGE)
        # the float64 argmax may break an exact tie or a last-unit difference the other way: count, do not assert
        agree = float((m.best == ref[0]).double().mean())
        assert torch.equal(m.inter[m.best == ref[0]], ref[1][m.best == ref[0]])
        paths = {"m": lambda: match_regions(ids, drawn, ROWS, SHAPES_AN_IMAGE),
                 "M": lambda: torch_match(ids, drawn, ROWS, SHAPES_AN_IMAGE),
                 "r": lambda: label_regions(pred, max_regions=ROWS), "c": lambda: (ids.clone(), drawn.clone())}
        times, iters = measure(paths, args.window, args.rounds)
        med = report(f"{shape}, match: {ROWS} regions against {SHAPES_AN_IMAGE} drawn shapes ({agree:.4f} of the float64 "
                     f"argmax agrees)",
                     {"m": "match_regions", "M": "torch: bincount, float64 IoU, argmax", "r": "label_regions",
                      "c": "ids.clone(); drawn.clone()"}, times, iters, args.rounds)
        print(f"  (M) / (m) = {med['M'] / med['m']:.2f}, (m) / (r) = {med['m'] / med['r']:.3f}, (m) / (c) = "
              f"{med['m'] / med['c']:.2f}", flush=True)
        results.append({"shape": [b, big_h, big_w], "workload": "match", "agree": agree,
                        "us": {k: [x * 1e6 for x in v] for k, v in times.items()}})
        na = torch.randint(0, ROWS, pred.shape, dtype=torch.int32, device=dev)
        nb = torch.randint(0, SHAPES_AN_IMAGE, pred.shape, dtype=torch.int32, device=dev)
        paths = {"m": lambda: match_regions(na, nb, ROWS, SHAPES_AN_IMAGE),
                 "M": lambda: torch_match(na, nb, ROWS, SHAPES_AN_IMAGE)}
        times, iters = measure(paths, args.window, args.rounds)
        med = report(f"{shape}, match on i.i.d. noise ids", {"m": "match_regions", "M": "torch: bincount, float64 IoU, argmax"},
                     times, iters, args.rounds)
        print(f"  (M) / (m) = {med['M'] / med['m']:.2f}", flush=True)
        results.append({"shape": [b, big_h, big_w], "workload": "match-noise",
                        "us": {k: [x * 1e6 for x in v] for k, v in times.items()}})
        del scores, pred, target, ids, drawn, na, nb
    print(json.dumps({"bench": "overlap", "results": results}))


if __name__ == "__main__":
    main()
