"""Timing of `EmbeddingBank.search` beyond k = 120 at 1 M x 768 fp16 (and 10 M with --rows 10000000) against the calls it is
built from and the one it replaces (not the contract bench; see bench.py).

Per (Q, k) in {1, 64, 1024} x {121, 1000, 4096} (or --q / --k), after warm-up, the median of REPS timed calls each (device
events around the call, one synchronisation per measurement), the routes interleaved round by round:
  search-k         `search(q, k)`: isc_cosine_topk_large
  search-120       `search(q, 120)` on the same queries: the code path of k <= 120, untouched
  range-at-kth     `search_range(q, t)` with t = each query's k-th score: the large call does this work plus the bound pass
  exhaustive-k     `search_exhaustive(q[:EXQ], k)`: isc_cosine_topk_exhaustive_large, timed once over at most EXQ = 8 queries
                   (nine float64 sweeps of the bank per four queries) and reported per query
Next to them: the candidates the filter kept per query in units of k (status word 3), the status words, the workspace bytes
of the large call and `stream_ms`, one read of the packed bank (N * D * 2 B) at the 6.29 TB/s a float4 copy reaches.
Usage: python scripts/quick_largek_bench.py [--out FILE.json] [--rows N] [--reps R] [--q Q ...] [--k K ...]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank, _lib  # noqa: E402

N, D, REPS, EXQ = 1_000_000, 768, 20, 8
HBM_TBPS = 6.29
args = sys.argv[1:]


def take(flag: str, many: bool = False):
    if flag not in args:
        return None
    i = args.index(flag)
    j = i + 1
    while j < len(args) and not args[j].startswith("--") and (many or j == i + 1):
        j += 1
    vals = args[i + 1 : j]
    del args[i:j]
    return vals if many else vals[0]


out_path = take("--out")
N = int(take("--rows") or N)
REPS = int(take("--reps") or REPS)
qs = [int(v) for v in (take("--q", many=True) or [1, 64, 1024])]
ks = [int(v) for v in (take("--k", many=True) or [121, 1000, 4096])]
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
rows = torch.empty((N, D), dtype=torch.float16, device=dev)
for r0 in range(0, N, 1 << 20):
    blk = torch.randn(min(1 << 20, N - r0), D, generator=g, device=dev)
    rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
del rows
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


for nq in qs:
    q = torch.nn.functional.normalize(torch.randn(nq, D, generator=g, device=dev), dim=1)
    for k in ks:
        s, i = bank.search(q, k)
        status = bank.last_status.cpu()
        kth = s[:, k - 1].contiguous()
        need = _lib.c_size_t()
        _lib.check(_lib.load().isc_cosine_topk_large_workspace_bytes(_lib.ISC_F16, N, D, nq, k, need), "workspace_bytes")
        routes = {
            "search-k": lambda: bank.search(q, k),
            "search-120": lambda: bank.search(q, 120),
            "range-at-kth": lambda: bank.search_range(q, kth),
        }
        res = bank.search_range(q, kth)
        same = all(torch.equal(res[j][1][:k], i[j]) for j in range(min(nq, 8)))
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(REPS):
            for name, fn in routes.items():
                times[name].append(timed(fn))
        med = {name: statistics.median(t) for name, t in times.items()}
        exq = min(nq, EXQ)
        bank.search_exhaustive(q[:exq], k)
        ex_ms = timed(lambda: bank.search_exhaustive(q[:exq], k))
        es, ei = bank.search_exhaustive(q[:exq], k)
        emit({"N": N, "D": D, "Q": nq, "k": k,
              **{name + "_ms": round(med[name], 3) for name in routes},
              **{name + "_min_ms": round(min(times[name]), 3) for name in routes},
              "over_range": round(med["search-k"] / med["range-at-kth"], 2),
              "over_search_120": round(med["search-k"] / med["search-120"], 2),
              "search_k_bank_streams": round(med["search-k"] / stream_ms, 2),
              "exhaustive_ms_per_query": round(ex_ms / exq, 3), "exhaustive_queries_timed": exq,
              "equals_exhaustive": bool(torch.equal(ei, i[:exq]) and torch.equal(es.view(torch.int32), s[:exq].view(torch.int32))),
              "first_k_of_range_equal": same,
              "candidates_per_query_over_k": round(int(status[3]) / (nq * k), 3),
              "status": [int(status[0]), int(status[1]), float(status[2:3].view(torch.float32)[0]), int(status[3])],
              "workspace_bytes": need.value, "stream_ms": round(stream_ms, 3), "reps": REPS})
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
