"""Timing of `EmbeddingBank.assign` and one `KMeans` iteration at 1 M x 768 fp16 against the two routes to the same labels
that exist without it (not the contract bench; see bench.py).

Per C in {16, 256, 1024} (or the C given on the command line), after warm-up, the median of 20 timed calls each, the routes
interleaved round by round:
  assign-labels    `assign(centroids, return_scores=False)`
  assign-scores    `assign(centroids)`
  kmeans-iter      `assign(return_scores=False)` + `group_sums` + the centroid update (tensor ops, no host read)
  scores-argmax    chunked `scores(centroids, rows)` (a [C, chunk] float32 block per call, chunk * C <= 2^26) + argmax
  centroid-bank    a bank built from the centroids, searched with 1024-row chunks of `bank.bank` as queries at k = 1 (the
                   unpacking is NOT timed); timed over `--baseline-rows` rows and scaled to N, the passes being identical
The labels of the three routes are compared once and the rows where they differ are counted.  scores-argmax computes the same
scores and must agree; the centroid bank ranks by dot / ||row|| -- a search normalises by its QUERY -- where assign ranks by
dot / ||centroid||, so it may pick another centroid on a near tie when the stored centroids' norms differ in the last fp16
bits: it is the closest older route, not the same function.  `stream_ms` is one read of the packed bank (N * D * 2 B) at the
6.29 TB/s a float4 copy reaches.
`--exact` adds, on the same bank, the float64 passes nothing else times: `search_exhaustive` of 8 queries, `scores` of 8
queries x 65536 rows and `assign_exhaustive` of 16 centroids (the median of 20 calls each).
Usage: python scripts/quick_assign_bench.py [--out FILE.json] [--rows N] [--baseline-rows M] [--exact] [C ...]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank  # noqa: E402

N, D, REPS = 1_000_000, 768, 20
BASE_ROWS = 65536
HBM_TBPS = 6.29
args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i : i + 2]
if "--rows" in args:
    i = args.index("--rows")
    N = int(args[i + 1])
    del args[i : i + 2]
exact = "--exact" in args
if exact:
    args.remove("--exact")
if "--baseline-rows" in args:
    i = args.index("--baseline-rows")
    BASE_ROWS = int(args[i + 1])
    del args[i : i + 2]
cs = [int(a) for a in args] or [16, 256, 1024]
BASE_ROWS = min(BASE_ROWS, N)
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
rows = torch.empty((N, D), dtype=torch.float16, device=dev)
for r0 in range(0, N, 1 << 20):
    blk = torch.randn(min(1 << 20, N - r0), D, generator=g, device=dev)
    rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
out = []
stream_ms = N * D * 2 / (HBM_TBPS * 1e12) * 1e3


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


all_rows = torch.arange(N, device=dev)
for c in cs:
    cent = torch.nn.functional.normalize(torch.randn(c, D, generator=g, device=dev), dim=1)
    chunk = max(1024, min(N, (1 << 26) // c))

    def scores_argmax(upto: int = N) -> torch.Tensor:
        parts = [bank.scores(cent, all_rows[r0 : min(r0 + chunk, upto)]).argmax(dim=0) for r0 in range(0, upto, chunk)]
        return torch.cat(parts)

    cbank = EmbeddingBank(cent, dtype=torch.float16, normalize=False)

    def centroid_bank(upto: int = BASE_ROWS) -> torch.Tensor:
        parts = [cbank.search(rows[r0 : min(r0 + 1024, upto)], 1)[1][:, 0] for r0 in range(0, upto, 1024)]
        return torch.cat(parts)

    def kmeans_iter() -> torch.Tensor:
        labels, _ = bank.assign(cent, return_scores=False)
        sums, counts = bank.group_sums(labels, c)
        norm = sums.norm(dim=1, keepdim=True)
        return torch.where((counts == 0)[:, None], cent.double(), sums / norm.clamp_min(1e-300)).float()

    routes = {
        "assign-labels": lambda: bank.assign(cent, return_scores=False),
        "assign-scores": lambda: bank.assign(cent),
        "kmeans-iter": kmeans_iter,
        "scores-argmax": scores_argmax,
        "centroid-bank": centroid_bank,
    }
    scale = {name: 1.0 for name in routes}
    scale["centroid-bank"] = N / BASE_ROWS
    # the same answer (and the warm-up of every route)
    labels, _ = bank.assign(cent, return_scores=False)
    status = bank.last_assign_status.cpu()
    a = scores_argmax()
    b = centroid_bank()
    diff_a = int((labels.long() != a).sum())
    diff_b = int((labels[:BASE_ROWS].long() != b).sum())
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(REPS):
        for name, fn in routes.items():
            times[name].append(timed(fn) * scale[name])
    med = {name: statistics.median(t) for name, t in times.items()}
    best_base = min(med["scores-argmax"], med["centroid-bank"])
    for name in routes:
        emit({"C": c, "N": N, "D": D, "route": name, "ms": round(med[name], 3),
              "min_ms": round(min(times[name]), 3), "max_ms": round(max(times[name]), 3),
              "over_assign_labels": round(med[name] / med["assign-labels"], 2),
              "bank_streams": round(med[name] / stream_ms, 2)})
    emit({"C": c, "assign_labels_ms": round(med["assign-labels"], 3), "best_baseline_ms": round(best_base, 3),
          "speedup_over_best_baseline": round(best_base / med["assign-labels"], 2), "stream_ms": round(stream_ms, 3),
          "status": [int(status[0]), int(status[1]), float(status[2:3].view(torch.float32)[0]), int(status[3])],
          "rows_differing_from_scores_argmax": diff_a, "rows_differing_from_centroid_bank": diff_b,
          "centroid_bank_timed_rows": BASE_ROWS})
    del cbank
if exact:
    # the float64 passes on the same bank (csrc/exact_dots.h), interleaved round by round like the routes above
    q8 = torch.nn.functional.normalize(torch.randn(8, D, generator=g, device=dev), dim=1)
    c16 = torch.nn.functional.normalize(torch.randn(16, D, generator=g, device=dev), dim=1)
    some = torch.randperm(N, generator=g, device=dev)[: min(65536, N)]
    passes = {
        "search_exhaustive-Q8": lambda: bank.search_exhaustive(q8, 10),
        "scores-8x64K": lambda: bank.scores(q8, some),
        "assign_exhaustive-C16": lambda: bank.assign_exhaustive(c16),
    }
    for fn in passes.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in passes}
    for _ in range(REPS):
        for name, fn in passes.items():
            times[name].append(timed(fn))
    for name, t in times.items():
        emit({"N": N, "D": D, "exact_pass": name, "ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
              "max_ms": round(max(t), 3)})
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
