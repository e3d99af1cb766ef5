"""Timing of the appendable bank (`EmbeddingBank(capacity=)`, `append`, `reserve`) at 10 M x 768 fp16 (not the contract
bench; see bench.py).

1. Append throughput: filling an empty bank of capacity C in blocks of 2^16 and 2^20 rows (`isc_bank_append`), against the
   only way a bank without reserved capacity has to take more rows -- building a fresh bank of the final size
   (`isc_bank_pack` over all rows).  Bytes are counted once read and once written (2 * rows * D * 2).
2. Search at partial fill: capacity C with C / 2, C - 1 (masked by the fill bitmap) and C rows (full: unmasked calls again)
   against the unmasked search of a fresh C-row bank, interleaved rounds, median of 5.
3. Growth: `isc_bank_repack` of C / 2 rows into an image laid out for C, against the `isc_bank_unpack` + `isc_bank_pack`
   round trip through a row-major copy it replaces.
Usage: python scripts/quick_append_bench.py [--out FILE.json] [--rows N] [Q ...]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import EmbeddingBank  # noqa: E402

C, D, K = 10_000_000, 768, 10
args = sys.argv[1:]
out_path = None
if "--out" in args:
    i = args.index("--out")
    out_path = args[i + 1]
    del args[i : i + 2]
if "--rows" in args:
    i = args.index("--rows")
    C = int(args[i + 1])
    del args[i : i + 2]
qs = [int(a) for a in args] or [1, 64, 1024]
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
rows = torch.empty((C, D), dtype=torch.float16, device=dev)
for r0 in range(0, C, 1 << 20):
    blk = torch.randn(min(1 << 20, C - r0), D, generator=g, device=dev)
    rows[r0 : r0 + blk.shape[0]] = torch.nn.functional.normalize(blk, dim=1).half()
out = []


def emit(line: dict) -> None:
    print(json.dumps(line), flush=True)
    out.append(line)


def timed(fn, iters: int = 1) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def gbs(n_rows: int, ms: float) -> float:
    return round(2 * n_rows * D * 2 / ms / 1e6, 1)


# ---- 1. append throughput
def fresh_bank() -> EmbeddingBank:
    return EmbeddingBank(rows, dtype=torch.float16, normalize=False)


def fill(block: int, upto: int = C) -> EmbeddingBank:
    eb = EmbeddingBank(rows[:0], dtype=torch.float16, normalize=False, capacity=C)
    for r0 in range(0, upto, block):
        eb.append(rows[r0 : min(r0 + block, upto)])
    return eb


fresh_bank()  # warm-up (code objects, the allocator's pool)
fresh_ms = statistics.median(timed(fresh_bank) for _ in range(3))
emit({"what": "fresh bank of C rows (isc_bank_pack, 2^20-row blocks)", "C": C, "D": D, "ms": round(fresh_ms, 2),
      "rows_per_s": round(C / fresh_ms * 1e3), "GBps": gbs(C, fresh_ms)})
for block in (1 << 16, 1 << 20):
    fill(block)
    ms = statistics.median(timed(lambda: fill(block)) for _ in range(3))
    emit({"what": "fill capacity C by appends (allocation of the empty image included)", "block": block, "ms": round(ms, 2),
          "rows_per_s": round(C / ms * 1e3), "GBps": gbs(C, ms), "ratio_to_fresh": round(ms / fresh_ms, 3)})
    eb = EmbeddingBank(rows[:0], dtype=torch.float16, normalize=False, capacity=C)
    eb.append(rows[:block])
    one = statistics.median(timed(lambda: eb._append_rows(rows[block : 2 * block], block, False, None), 5) for _ in range(3))
    emit({"what": "one isc_bank_append launch into a capacity-C image", "block": block, "ms": round(one, 4),
          "rows_per_s": round(block / one * 1e3), "GBps": gbs(block, one),
          "fresh_bank_over_one_append": round(fresh_ms / one, 1)})
    del eb

# ---- 2. search at partial fill
fresh = fresh_bank()
half = fill(1 << 20, C // 2)
most = fill(1 << 20, C - 1)
for nq in qs:
    q = torch.randn(nq, D, generator=g, device=dev).half()
    iters = 10 if nq <= 64 else 4
    cases = {"fresh C rows, unmasked": fresh, "capacity C, C/2 rows": half, "capacity C, C-1 rows": most}
    for b in cases.values():
        b.search(q, K)
    torch.cuda.synchronize()
    rounds = {name: [] for name in cases}
    for _ in range(5):
        for name, b in cases.items():
            rounds[name].append(timed(lambda b=b: b.search(q, K), iters))
    base = statistics.median(rounds["fresh C rows, unmasked"])
    for name, b in cases.items():
        ms = statistics.median(rounds[name])
        b.search(q, K)
        emit({"Q": nq, "k": K, "bank": name, "ms": round(ms, 4), "ratio_to_unmasked": round(ms / base, 4),
              "status": b.last_status.tolist()})
most.append(rows[C - 1 :])
for nq in qs:
    q = torch.randn(nq, D, generator=g, device=dev).half()
    iters = 10 if nq <= 64 else 4
    most.search(q, K), fresh.search(q, K)
    a, b = [], []
    for _ in range(5):
        a.append(timed(lambda: fresh.search(q, K), iters))
        b.append(timed(lambda: most.search(q, K), iters))
    emit({"Q": nq, "k": K, "bank": "capacity C, C rows (full: unmasked calls)", "ms": round(statistics.median(b), 4),
          "ratio_to_unmasked": round(statistics.median(b) / statistics.median(a), 4)})
del fresh, most

# ---- 3. growth
n = C // 2
src = EmbeddingBank(rows[:n], dtype=torch.float16, normalize=False)
del rows


def repack() -> None:
    packed, fill_bits, _ = src._alloc_image(C, dev, False)
    src._repack_rows(src._bank, n, None, packed, C, None, fill_bits)


def round_trip() -> None:
    EmbeddingBank(src.bank, dtype=torch.float16, normalize=False, capacity=C)


repack(), round_trip()
packed, fill_bits, _ = src._alloc_image(C, dev, False)
kernel = statistics.median(timed(lambda: src._repack_rows(src._bank, n, None, packed, C, None, fill_bits)) for _ in range(3))
del packed, fill_bits
emit({"what": "isc_bank_repack alone", "rows": n, "ms": round(kernel, 2), "GBps": gbs(n, kernel)})
a = statistics.median(timed(repack) for _ in range(3))
b = statistics.median(timed(round_trip) for _ in range(3))
emit({"what": "grow C/2 rows to capacity C: new image + isc_bank_repack", "ms": round(a, 2), "GBps": gbs(n, a)})
emit({"what": "grow C/2 rows to capacity C: isc_bank_unpack + new image + isc_bank_append", "ms": round(b, 2),
      "GBps": gbs(n, b), "ratio_to_repack": round(b / a, 2)})
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
