"""Timing of the grouped top-k (`EmbeddingBank.search(q, 10, exclude_group=...)`) on a 10 M x 768 fp16 bank (not the
contract bench; see bench.py).

Rows are in groups of 49 adjacent rows (the cells of one 7 x 7 map); each query is a banked row plus noise and excludes
its row's group.  For each Q the unmasked search, the masked search with every row allowed and the grouped search are
timed in 5 interleaved rounds (device events around `iters` calls, the median round kept) and printed with the ratio to
the unmasked time and each call's `last_status` ([0] overflowed buffers, [1] queries redone, [3] exhaustive sweeps).
Usage: python scripts/quick_group_bench.py [--out FILE.json] [Q ...]   (--out: also write the lines as one JSON list)"""
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
labels = torch.arange(N, device=dev) // CELLS
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False, row_groups=labels)
e1.record()
torch.cuda.synchronize()
src_all = torch.randint(0, N, (max(qs),), generator=g, device=dev)
queries = (rows[src_all].float() + 0.05 * torch.randn((max(qs), D), generator=g, device=dev)).half()
del rows
all_rows = eb.row_filter(torch.ones(N, dtype=torch.bool, device=dev))


def timed(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


out = [{"N": N, "D": D, "group_rows": CELLS, "bank_build_with_groups_ms": round(e0.elapsed_time(e1), 2)}]
print(json.dumps(out[0]), flush=True)
for nq in qs:
    q = queries[:nq].contiguous()
    excl = labels[src_all[:nq]]
    iters = 10 if nq <= 64 else 4
    cases = {"unmasked": lambda: eb.search(q, K), "masked_all_rows": lambda: eb.search(q, K, mask=all_rows),
             "grouped": lambda: eb.search(q, K, exclude_group=excl)}
    for fn in cases.values():  # warm-up (workspaces, code objects)
        fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name in cases}
    for _ in range(5):
        for name, fn in cases.items():
            rounds[name].append(timed(fn, iters))
    base = statistics.median(rounds["unmasked"])
    for name, fn in cases.items():
        ms = statistics.median(rounds[name])
        _, idx = fn()
        line = {"Q": nq, "k": K, "search": name, "ms": round(ms, 4), "ratio_to_unmasked": round(ms / base, 4),
                "status": eb.last_status.tolist()}
        if name == "grouped":
            line["own_group_hits"] = int((idx // CELLS == excl[:, None]).sum())
        print(json.dumps(line), flush=True)
        out.append(line)
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
