"""Times the `preprocess="checkpoint"` path against the squash path it stands next to, on the GPU:

  (a) resize_center_crop(x, size, crop, fixed statistics, quantize=True)     one table launch + one fused kernel
  (b) normalize_per_channel(resize(x, (crop, crop)), fixed statistics)       the existing path: bilinear, no antialiasing

in one process, alternating, with device events after a warm-up, each window `--window` seconds of back-to-back calls,
`--rounds` windows a path.  Prints per shape the median call time of both with the spread (min .. max over the rounds),
the algorithmic bytes of (a) -- the uint8 bytes inside the support of the crop rectangle plus the float32 output -- and
the bytes/s they amount to as a share of the HBM peak (8.0 TB/s spec; a float4 copy reaches 6.29), and one JSON line.

    python scripts/bench_preprocess.py [--size 224] [--crop 224] [--window 0.4] [--rounds 5]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from imagescry_amd import clip, normalize_per_channel, resize, resize_center_crop  # noqa: E402
from imagescry_amd.transforms import center_crop_geometry  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, spec
SHAPES = [(256, 3, 500, 375), (64, 3, 3000, 2000)]


def support(n_in: int, n_out: int, first: int, count: int) -> tuple[int, int]:
    """[lo, hi) of the input samples the outputs first .. first + count - 1 of an axis read."""
    s = n_in / n_out
    half = 2.0 * max(s, 1.0)
    lo = max(int(s * (first + 0.5) - half + 0.5), 0)
    hi = min(int(s * (first + count - 0.5) + half + 0.5), n_in)
    return lo, hi


def window(fn, iters: int) -> float:
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
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    mean = torch.tensor(clip.IMAGE_MEAN, device=dev) * 255.0
    std = torch.tensor(clip.IMAGE_STD, device=dev) * 255.0
    mean4, std4 = mean.reshape(1, 3, 1, 1), std.reshape(1, 3, 1, 1)
    results = []
    for b, c, h, w in SHAPES:
        x = torch.randint(0, 256, (b, c, h, w), dtype=torch.uint8, device=dev)
        (h2, w2), (top, left, hc, wc) = center_crop_geometry(h, w, args.size, args.crop)
        r0, r1 = support(h, h2, top, hc)
        c0, c1 = support(w, w2, left, wc)
        bytes_a = b * c * ((r1 - r0) * (c1 - c0) + 4 * hc * wc)

        def path_a():
            return resize_center_crop(x, args.size, args.crop, channel_means=mean, channel_stds=std, quantize=True)

        def path_b():
            return normalize_per_channel(resize(x, (args.crop, args.crop)), channel_means=mean4, channel_stds=std4, eps=0.0)

        times = {"a": [], "b": []}
        iters = {}
        for name, fn in (("a", path_a), ("b", path_b)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[name] = max(10, int(args.window / window(fn, 5)) + 1)
        for _ in range(args.rounds):
            for name, fn in (("a", path_a), ("b", path_b)):
                times[name].append(window(fn, iters[name]))
        med = {k: statistics.median(v) for k, v in times.items()}
        rate = bytes_a / med["a"]
        print(f"{b} x {c} x {h} x {w} uint8 -> resize ({h2}, {w2}), crop ({top}, {left}, {hc}, {wc})")
        for k, label in (("a", "(a) checkpoint"), ("b", "(b) squash    ")):
            print(f"  {label}: median {med[k] * 1e6:9.1f} us  (min {min(times[k]) * 1e6:.1f} .. max {max(times[k]) * 1e6:.1f}, "
                  f"{args.rounds} windows of {iters[k]} calls)")
        print(f"  (a) algorithmic bytes {bytes_a / 1e6:.1f} MB (input rows {r0}..{r1}, columns {c0}..{c1}; float32 out) -> "
              f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak", flush=True)
        results.append({"shape": [b, c, h, w], "resize": [h2, w2], "crop": [top, left, hc, wc],
                        "a_us": [t * 1e6 for t in times["a"]], "b_us": [t * 1e6 for t in times["b"]],
                        "a_bytes": bytes_a, "a_bytes_per_s": rate, "a_share_of_hbm_peak": rate / HBM_PEAK})
        del x
    print(json.dumps({"bench": "preprocess", "size": args.size, "crop": args.crop, "results": results}))


if __name__ == "__main__":
    main()
