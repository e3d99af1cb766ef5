"""Timing of the collapsed search (`EmbeddingBank.search_groups(q, 10)`) on a 10 M x 768 fp16 bank (not the contract
bench; see bench.py).

Two banks of the same rows: groups of 49 adjacent rows (the cells of one 7 x 7 map), and every row its own group.  Each
query is a banked row plus noise.  For each Q the row search, the grouped row search (`exclude_group=` a label no row
carries) and `search_groups` are timed in 5 interleaved rounds (device events around `iters` calls, the median round
kept) and printed with the ratio to the row search and each call's `last_status` ([0] overflowed buffers, [1] queries
redone, [3] exhaustive sweeps).
Usage: python scripts/quick_collapse_bench.py [--out FILE.json] [Q ...]   (--out: also write the lines as one JSON list)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank  # noqa: E402

N, D, K, CELLS = 10_000_000, 768, 10, 49
args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i : i + 2]
qs = [int(a) for a in args] or [1, 64, 1024]
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
rows = torch.empty((N, D), dtype=torch.float16, device=dev)
for r0 in range(0, N, 1 << 20):
    blk = torch.randn(min(1 << 20, N - r0), D, generator=g, device=dev)
    rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
src_all = torch.randint(0, N, (max(qs),), generator=g, device=dev)
queries = (rows[src_all].float() + 0.05 * torch.randn((max(qs), D), generator=g, device=dev)).half()


def timed(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


out = []
for bank_name, labels in (("groups_of_49", torch.arange(N, device=dev) // CELLS), ("singletons", torch.arange(N, device=dev))):
    eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False, row_groups=labels)
    del labels
    head = {"bank": bank_name, "N": N, "D": D, "max_group_rows": eb._max_group_rows}
    print(json.dumps(head), flush=True)
    out.append(head)
    for nq in qs:
        q = queries[:nq].contiguous()
        none = torch.full((nq,), -1, dtype=torch.int64, device=dev)
        iters = 10 if nq <= 64 else 4
        cases = {"search": lambda: eb.search(q, K), "grouped_search": lambda: eb.search(q, K, exclude_group=none),
                 "search_groups": lambda: eb.search_groups(q, K)}
        for fn in cases.values():  # warm-up (workspaces, code objects)
            fn()
        torch.cuda.synchronize()
        rounds = {name: [] for name in cases}
        for _ in range(5):
            for name, fn in cases.items():
                rounds[name].append(timed(fn, iters))
        base = statistics.median(rounds["search"])
        for name, fn in cases.items():
            ms = statistics.median(rounds[name])
            fn()
            line = {"bank": bank_name, "Q": nq, "k": K, "call": name, "ms": round(ms, 4),
                    "ratio_to_search": round(ms / base, 4), "status": eb.last_status.tolist()}
            print(json.dumps(line), flush=True)
            out.append(line)
    del eb
    torch.cuda.empty_cache()
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
