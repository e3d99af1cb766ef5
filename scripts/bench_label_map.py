"""Times the fused pixel labelling against the torch composition it replaces, on the GPU:

  (a) segmentation.label_map(scores_bhwc, (H, W))                        one launch: labels uint8 + best float32
  (b) F.interpolate(scores_bchw, (H, W), mode="bilinear").max(dim=1)     writes [B, C, H, W] float32, reads it back

in one process, alternating, with device events after a warm-up, each window `--window` seconds of back-to-back calls,
`--rounds` windows a path.  Before timing, (a)'s labels are compared with (b)'s on the same input (the two blend in
different orders: the share of pixels that differ is printed; tests/test_segment_host.py has the argument).  Prints per
shape the median call time of both with the spread (min .. max over the rounds), the bytes (a) has to store -- one uint8
and one float32 a pixel -- and the bytes/s they amount to as a share of the HBM peak (8.0 TB/s spec; a float4 copy
reaches 6.29), the prompt blends per second, and one JSON line.

    python scripts/bench_label_map.py [--window 0.5] [--rounds 5]
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

from imagescry_amd import label_map  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, spec
# (B, C, h, w, H, W): ADE20K's 150 classes on 28 x 28 patches to 448 x 448; 21 classes on 14 x 14 to 224 x 224
SHAPES = [(64, 150, 28, 28, 448, 448), (512, 21, 14, 14, 224, 224)]


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
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_map.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    results = []
    for b, c, h, w, big_h, big_w in SHAPES:
        g = torch.Generator().manual_seed(b + c)
        m = F.normalize(torch.randn(b, 64, h, w, generator=g), dim=1)
        t = F.normalize(torch.randn(c, 64, generator=g), dim=1)
        bchw = torch.einsum("behw,ce->bchw", m, t).contiguous().to(dev)
        bhwc = bchw.permute(0, 2, 3, 1).contiguous()
        pixels = b * big_h * big_w
        stored = pixels * 5

        def path_a():
            return label_map(bhwc, (big_h, big_w))

        def path_b():
            return F.interpolate(bchw, size=(big_h, big_w), mode="bilinear", align_corners=False).max(dim=1)

        ours, theirs = path_a(), path_b()
        differ = float((ours.labels.long() != theirs.indices).float().mean())
        far = float((ours.scores - theirs.values).abs().max())
        del ours, theirs
        times = {"a": [], "b": []}
        iters = {}
        for name, fn in (("a", path_a), ("b", path_b)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[name] = max(5, int(args.window / window(fn, 3)) + 1)
        for _ in range(args.rounds):
            for name, fn in (("a", path_a), ("b", path_b)):
                times[name].append(window(fn, iters[name]))
        med = {k: statistics.median(v) for k, v in times.items()}
        rate = stored / med["a"]
        print(f"{b} x {c} x {h} x {w} -> {big_h} x {big_w}: labels differ from the composition's at {100 * differ:.4f} % of "
              f"the pixels, max |best - max| = {far:.2e}")
        for k, label in (("a", "(a) label_map        "), ("b", "(b) interpolate + max")):
            print(f"  {label}: median {med[k] * 1e6:10.1f} us  (min {min(times[k]) * 1e6:.1f} .. max {max(times[k]) * 1e6:.1f}, "
                  f"{args.rounds} windows of {iters[k]} calls)")
        print(f"  (a) stores {stored / 1e6:.1f} MB -> {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8.0 TB/s HBM "
              f"peak; {pixels * c / med['a'] / 1e9:.1f} G prompt blends/s; (b) / (a) = {med['b'] / med['a']:.2f}; the "
              f"intermediate (b) writes is {pixels * c * 4 / 1e9:.2f} GB", flush=True)
        results.append({"shape": [b, c, h, w, big_h, big_w], "a_us": [x * 1e6 for x in times["a"]],
                        "b_us": [x * 1e6 for x in times["b"]], "a_stored_bytes": stored, "a_bytes_per_s": rate,
                        "a_share_of_hbm_peak": rate / HBM_PEAK, "labels_differ": differ, "max_abs_diff": far})
        del bchw, bhwc
    print(json.dumps({"bench": "label_map", "results": results}))


if __name__ == "__main__":
    main()
