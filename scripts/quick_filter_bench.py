"""Timing of the masked top-k (`EmbeddingBank.search(q, 10, mask=...)`) on a 10 M x 768 fp16 bank (not the contract
bench; see bench.py).

Masks: random with allowed fraction 1.0, 0.5, 0.01 and 1e-4, and "exclude one image" (the 64 adjacent cells of one image
disallowed).  For each Q, the unmasked search and every mask are timed in interleaved rounds (device events around
`iters` calls, the median round kept) and printed with the ratio to the unmasked time and the masked call's
`last_status` ([0] overflowed buffers, [1] queries redone, [3] queries answered by the exhaustive sweep).  The cost of
`isc_row_mask_pack` (one `row_filter` call on a device bool tensor) is printed once.
Usage: python scripts/quick_filter_bench.py [--out FILE.json] [Q ...]   (--out: also write the lines as one JSON list)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank  # noqa: E402

N, D, K = 10_000_000, 768, 10
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
eb = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
del rows


def timed(fn, iters: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


allows = {f"random_{p:g}": torch.rand(N, generator=g, device=dev) < p for p in (1.0, 0.5, 0.01, 1e-4)}
image = torch.ones(N, dtype=torch.bool, device=dev)
image[5_000_000 : 5_000_064] = False
allows["exclude_one_image"] = image
filters = {name: eb.row_filter(a) for name, a in allows.items()}
pack_ms = statistics.median(timed(lambda: eb.row_filter(allows["random_0.5"]), 5) for _ in range(3))
out = [{"N": N, "D": D, "row_filter_ms": round(pack_ms, 4)}]
print(json.dumps(out[0]), flush=True)
for nq in qs:
    q = torch.randn(nq, D, generator=g, device=dev).half()
    iters = 10 if nq <= 64 else 4
    cases = {"unmasked": lambda: eb.search(q, K)}
    for name, rf in filters.items():
        cases[name] = (lambda rf=rf: eb.search(q, K, mask=rf))
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
        fn()
        line = {"Q": nq, "k": K, "mask": name, "ms": round(ms, 4), "ratio_to_unmasked": round(ms / base, 4),
                "allowed": None if name == "unmasked" else int(filters[name].allowed_count.item()),
                "status": eb.last_status.tolist()}
        print(json.dumps(line), flush=True)
        out.append(line)
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
