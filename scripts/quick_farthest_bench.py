"""Timing of `EmbeddingBank.farthest_points` against the loop a user had to write without it (not the contract bench; see
bench.py).

Banks of unit fp16 rows, 1 M x 768 and 100 k x 768 (or the row counts given on the command line), m = 256 picks.  After one
warm-up call of each route, 5 timed calls each with device events around the public calls, the routes interleaved round by
round; the median, the minimum and the maximum are reported:
  farthest-points   `bank.farthest_points(m)`
  scores-loop       per pick `bank.scores(bank.rows(c), arange(len))` -- a [1, N] table through an N-entry row list -- then
                    `torch.maximum` into the running `near` and an `argmin` over the rows not yet picked, all on the device
                    (the index check of `rows` is the loop's one host read per pick)
The picks of the two routes are compared once.  `per_pick_ms` is the call divided by m, `per_pick_streams` that time in reads
of the packed bank (N * D * 2 B) at the 6.29 TB/s a float4 copy reaches.
Usage: python scripts/quick_farthest_bench.py [--out FILE.json] [--picks M] [N ...]"""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank  # noqa: E402

D, REPS, M = 768, 5, 256
HBM_TBPS = 6.29
args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i : i + 2]
if "--picks" in args:
    i = args.index("--picks")
    M = int(args[i + 1])
    del args[i : i + 2]
sizes = [int(a) for a in args] or [1_000_000, 100_000]
dev = torch.device("cuda:0")
out = []


def emit(line: dict) -> None:
    print(json.dumps(line), flush=True)
    out.append(line)


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for n in sizes:
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.empty((n, D), dtype=torch.float16, device=dev)
    for r0 in range(0, n, 1 << 20):
        blk = torch.randn(min(1 << 20, n - r0), D, generator=g, device=dev)
        rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
    bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
    del rows
    every = torch.arange(n, device=dev)
    stream_ms = n * D * 2 / (HBM_TBPS * 1e12) * 1e3

    def scores_loop() -> torch.Tensor:
        near = torch.full((n,), -math.inf, device=dev)
        taken = torch.zeros(n, dtype=torch.bool, device=dev)
        picks = torch.empty(M, dtype=torch.int64, device=dev)
        c = torch.zeros(1, dtype=torch.int64, device=dev)  # no centre yet: the lowest row
        for t in range(M):
            picks[t : t + 1] = c
            taken[c] = True
            near = torch.maximum(near, bank.scores(bank.rows(c), every)[0])
            c = near.masked_fill(taken, math.inf).argmin().reshape(1)
        return picks

    routes = {"farthest-points": lambda: bank.farthest_points(M)[0], "scores-loop": scores_loop}
    answers = {name: fn() for name, fn in routes.items()}  # the same answer (and the warm-up of both routes)
    torch.cuda.synchronize()
    differing = int((answers["farthest-points"] != answers["scores-loop"]).sum())
    times = {name: [] for name in routes}
    for _ in range(REPS):
        for name, fn in routes.items():
            times[name].append(timed(fn))
    med = {name: statistics.median(t) for name, t in times.items()}
    for name in routes:
        emit({"N": n, "D": D, "m": M, "route": name, "ms": round(med[name], 3), "min_ms": round(min(times[name]), 3),
              "max_ms": round(max(times[name]), 3), "per_pick_ms": round(med[name] / M, 4),
              "per_pick_streams": round(med[name] / M / stream_ms, 2)})
    emit({"N": n, "m": M, "stream_ms": round(stream_ms, 4), "picks_differing": differing,
          "speedup_over_scores_loop": round(med["scores-loop"] / med["farthest-points"], 2)})
    del bank, every
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
