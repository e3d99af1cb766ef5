"""Times the fused sliding-window labelling against the torch composition it replaces, on the GPU:

  (a) segmentation.label_map_windows(scores, (H, W), window, stride)     one launch: labels uint8 + best float32
  (b) per window F.interpolate(scores_bchw, window, mode="bilinear"), added into a [b, C, H, W] accumulator, divided by
      the count map, .max(dim=1); chunked over the images so that the accumulator stays under `--accumulator-gb`
  (c) segmentation.label_map(one window's scores per image, (H, W))      one blend a prompt and pixel: the per-blend
      reference at the same output size (not the same answer)

in one process, alternating, with device events after a warm-up, each window of time `--window` seconds of back-to-back
calls, `--rounds` of them a path.  Before timing, (a)'s labels are compared with (b)'s on the same input (the two round in
different places: the share of pixels that differ is printed; tests/test_segment_windows_host.py has the argument).
Prints per shape the medians with the spread (min .. max over the rounds), the prompt blends per second of (a) -- one
per prompt, pixel and covering window -- and one JSON line.

    python scripts/bench_label_map_windows.py [--window 0.5] [--rounds 5]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from imagescry_amd import label_map, label_map_windows, window_grid  # noqa: E402

# (B, C, h, w, H, W, window, stride): ADE20K's 150 classes, 448 x 448 images under 224 x 224 windows of 14 x 14 patches at
# half-window stride (9 windows); 21 classes, 224 x 224 under 112 x 112 windows of 7 x 7 patches
SHAPES = [(64, 150, 14, 14, 448, 448, 224, 112), (512, 21, 7, 7, 224, 224, 112, 56)]


def timed(fn, iters: int) -> float:
    """Seconds per call over `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accumulator-gb", type=float, default=4.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_map_windows.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    results = []
    for b, c, h, w, big_h, big_w, win, step in SHAPES:
        ys, xs = window_grid((big_h, big_w), win, step)
        ny, nx = len(ys), len(xs)
        g = torch.Generator().manual_seed(b + c)
        m = F.normalize(torch.randn(b * ny * nx, 64, h, w, generator=g), dim=1)
        t = F.normalize(torch.randn(c, 64, generator=g), dim=1)
        bhwc = torch.einsum("behw,ce->bhwc", m, t).reshape(b, ny, nx, h, w, c).contiguous().to(dev)
        bchw = bhwc.permute(0, 1, 2, 5, 3, 4).contiguous()  # [B, ny, nx, C, h, w]: what F.interpolate takes a window
        first = bhwc[:, 0, 0].contiguous()
        count = torch.zeros((big_h, big_w), device=dev)
        for y in ys:
            for x in xs:
                count[y:y + win, x:x + win] += 1
        blends = b * c * int(count.sum().item())
        images_a_pass = max(1, min(b, int(args.accumulator_gb * 1e9 / (c * big_h * big_w * 4))))

        def path_a():
            return label_map_windows(bhwc, (big_h, big_w), win, step)

        def path_b():
            values, indices = [], []
            for i in range(0, b, images_a_pass):
                part = bchw[i:i + images_a_pass]
                acc = torch.zeros((part.shape[0], c, big_h, big_w), device=dev)
                for iy, y in enumerate(ys):
                    for ix, x in enumerate(xs):
                        acc[:, :, y:y + win, x:x + win] += F.interpolate(part[:, iy, ix], size=(win, win), mode="bilinear",
                                                                         align_corners=False)
                best = (acc / count).max(dim=1)
                values.append(best.values)
                indices.append(best.indices)
            return torch.cat(values), torch.cat(indices)

        def path_c():
            return label_map(first, (big_h, big_w))

        ours, theirs = path_a(), path_b()
        differ = float((ours.labels.long() != theirs[1]).float().mean())
        far = float((ours.scores - theirs[0]).abs().max())
        del ours, theirs
        paths = (("a", path_a), ("b", path_b), ("c", path_c))
        times = {k: [] for k, _ in paths}
        iters = {}
        for name, fn in paths:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[name] = max(5, int(args.window / timed(fn, 3)) + 1)
        for _ in range(args.rounds):
            for name, fn in paths:
                times[name].append(timed(fn, iters[name]))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{b} x {c} prompts, {ny} x {nx} windows of {h} x {w} cells and {win} x {win} pixels at stride {step} -> "
              f"{big_h} x {big_w}: labels differ from the composition's at {100 * differ:.4f} % of the pixels, "
              f"max |best - max| = {far:.2e}")
        for k, label in (("a", "(a) label_map_windows      "), ("b", "(b) interpolate + add + max"),
                         ("c", "(c) label_map, one window  ")):
            print(f"  {label}: median {med[k] * 1e6:10.1f} us  (min {min(times[k]) * 1e6:.1f} .. max {max(times[k]) * 1e6:.1f}, "
                  f"{args.rounds} windows of {iters[k]} calls)")
        print(f"  (a) {blends / (b * c * big_h * big_w):.2f} blends a prompt and pixel, {blends / med['a'] / 1e9:.1f} G prompt "
              f"blends/s ((c): {b * c * big_h * big_w / med['c'] / 1e9:.1f} G); (b) / (a) = {med['b'] / med['a']:.2f}, "
              f"(a) / (c) = {med['a'] / med['c']:.2f}; (b) ran {images_a_pass} images a pass", flush=True)
        results.append({"shape": [b, c, h, w, big_h, big_w, win, step], "a_us": [x * 1e6 for x in times["a"]],
                        "b_us": [x * 1e6 for x in times["b"]], "c_us": [x * 1e6 for x in times["c"]],
                        "a_blends": blends, "labels_differ": differ, "max_abs_diff": far, "b_images_a_pass": images_a_pass})
        del bchw, bhwc, first
    print(json.dumps({"bench": "label_map_windows", "results": results}))


if __name__ == "__main__":
    main()
