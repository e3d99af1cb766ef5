"""Timing of EmbeddingBank.search_range on a 10 M x 768 fp16 bank (not the contract bench; see bench.py).

Thresholds admit about 10, 1 000 and 100 000 rows per query (random unit rows: score ~ N(0, 1/768)).  Device events bracket
`iters` calls (each call synchronises the host once to size its output, so the time is end to end).  Prints one line per
case: ms per call, the end-to-end HBM fraction N * D * 2 B / t / 8 TB/s, and the ratio to `search(q, 10)` at the same Q.
Usage: python scripts/quick_range_bench.py [--out FILE.json] [Q ...]   (--out: also write the lines as one JSON list)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank  # noqa: E402

N, D = 10_000_000, 768
THRESHOLDS = {10: 0.1714, 1_000: 0.1342, 100_000: 0.0839}
args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i : i + 2]
qs = [int(a) for a in args] or [1, 16, 64, 256, 1024]
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
rows = torch.empty((N, D), dtype=torch.float16, device=dev)
for r0 in range(0, N, 1 << 20):
    blk = torch.randn(min(1 << 20, N - r0), D, generator=g, device=dev)
    rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
del rows


def timed(fn, iters: int) -> float:
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


out = []
for nq in qs:
    q = torch.randn(nq, D, generator=g, device=dev).half()
    topk_ms = timed(lambda: eb.search(q, 10), 5)
    for per_query, t in THRESHOLDS.items():
        if nq * per_query > 30_000_000:
            continue
        ms = timed(lambda: eb.search_range(q, t, max_results=1 << 28), 5)
        res = eb.search_range(q, t, max_results=1 << 28)
        line = {
            "N": N, "D": D, "Q": nq, "target_per_query": per_query, "t": t,
            "mean_results_per_query": float(res.offsets[-1]) / nq, "ms": round(ms, 4),
            "hbm_fraction": round(N * D * 2 / (ms * 1e-3) / 8e12, 4), "topk10_ms": round(topk_ms, 4),
            "ratio_to_topk10": round(ms / topk_ms, 3), "status": eb.last_range_status.tolist(),
        }
        print(json.dumps(line), flush=True)
        out.append(line)
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
