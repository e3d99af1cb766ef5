"""Randomised differential test of EmbeddingBank.search against search_exhaustive for 120 < k <= 4096 (the proven-bound
range search against the float64 radix select, both on the device), bit for bit.  Not part of the pytest suites; run on the
GPU:  python scripts/fuzz_largek.py [seconds] [seed]

Every case: random N around the tile (256 rows), the bucket granularities (N / 16 and N / 4 against the bucket count) and the
bucket fold, D, Q (one pass, several passes), k around the pass sizes, fp16 or fp32 bank and queries, unit or raw rows;
optionally exact copies, near-duplicates of the queries' rows, a mask=, exclude_group= and a zero / tiny query.  Prints one
JSON line per run with the counts: cases, failures, passes that overflowed, queries the last resort answered and the largest
|A - E| / eps seen."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from imagescry_amd import EmbeddingBank

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
dev = torch.device("cuda:0")
NS = [121, 255, 256, 257, 1000, 4095, 4097, 5000, 12345, 16384, 32768, 65537, 131072, 200000]
DS = [1, 3, 32, 33, 40, 64, 128, 768]
QS = [1, 2, 63, 64, 65, 129, 300, 1025]
KS = [121, 128, 255, 256, 257, 500, 1000, 1024, 2048, 2049, 4096]
t_end = time.time() + budget
cases = fails = overflowed = last_resort = 0
worst = 0.0
while time.time() < t_end:
    n = int(rng.choice(NS))
    d = int(rng.choice(DS))
    nq = int(rng.choice(QS))
    if n * d > 60_000_000:
        d = 64
    k = min(int(rng.choice(KS)), n)
    if rng.random() < 0.2:
        k = int(rng.integers(121, min(n, 4096) + 1))
    dtype = torch.float16 if rng.random() < 0.6 else torch.float32
    qdtype = torch.float16 if rng.random() < 0.5 else torch.float32
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    rows = torch.randn(n, d, generator=g)
    if rng.random() < 0.2:  # exact copies
        rows[n // 2 : n // 2 + n // 4] = rows[: n // 4].clone()
    if rng.random() < 0.7:
        rows = torch.nn.functional.normalize(rows, dim=1)
    labels = torch.arange(n) // 49
    src = torch.randint(0, n, (nq,), generator=g)
    q = rows[src] + float(rng.choice([0.0, 0.05, 0.5])) * torch.randn(nq, d, generator=g)
    if rng.random() < 0.1:
        q[0] = 0.0
    if rng.random() < 0.1:
        q[-1] *= 1e-33
    q = q.to(qdtype).to(dev)
    eb = EmbeddingBank(rows.to(dev), dtype=dtype, normalize=False, row_groups=labels)
    kw = {}
    if rng.random() < 0.3:
        kw["mask"] = (torch.rand(n, generator=g) < float(rng.choice([0.05, 0.5, 0.95]))).to(dev)
    if rng.random() < 0.3:
        kw["exclude_group"] = labels[src]
    got = eb.search(q, k, **kw)
    st = eb.last_status.cpu()
    exp = eb.search_exhaustive(q, k, **kw)
    cases += 1
    overflowed += int(st[0])
    last_resort += int(st[1])
    ratio = float(st[2:3].view(torch.float32)[0])
    worst = max(worst, ratio)
    ok = torch.equal(got[1], exp[1]) and torch.equal(got[0].view(torch.int32), exp[0].view(torch.int32)) and ratio < 1.0
    if not ok:
        fails += 1
        print(json.dumps({"FAIL": True, "n": n, "d": d, "q": nq, "k": k, "dtype": str(dtype), "qdtype": str(qdtype),
                          "mask": "mask" in kw, "exclude": "exclude_group" in kw, "status": st.tolist()}), flush=True)
    del eb
print(json.dumps({"cases": cases, "failures": fails, "passes_overflowed": overflowed, "last_resort_queries": last_resort,
                  "worst_filter_error_over_eps": round(worst, 4), "seed": seed, "seconds": budget}), flush=True)
sys.exit(1 if fails else 0)
