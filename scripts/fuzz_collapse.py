"""Randomised differential test of EmbeddingBank.search_groups against search_groups_exhaustive (the float64 sweep on the
device), bit for bit.  Not part of the pytest suites; run on the GPU:  python scripts/fuzz_collapse.py [seconds] [seed]

Every case: random N around the tile (256 rows) and level boundaries, D, Q (one pass, and two passes past 1024), k,
fp16 or fp32 bank and queries, and a group size from {1, 2, 49, 1000, N} with labels permuted; optionally near-duplicate
rows inside a group, exact copies, a mask= and exclude_group=.  Prints one JSON line per run with the counts."""
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
NS = [1, 2, 49, 255, 256, 257, 4095, 4096, 4097, 5000, 12345, 65536, 65537, 200000]
DS = [1, 3, 32, 33, 64, 96, 128, 768]
QS = [1, 2, 63, 64, 65, 128, 129, 256, 300, 1025]
KS = [1, 2, 10, 17, 64, 120]
GROUPS = [1, 2, 49, 1000, 0]  # 0: one group of every row
t_end = time.time() + budget
cases = fails = 0
redone = exhaustive = 0
while time.time() < t_end:
    n = int(rng.choice(NS))
    d = int(rng.choice(DS))
    nq = int(rng.choice(QS)) if rng.random() < 0.9 else 1025
    if n * d > 60_000_000:
        d = 64
    gs = int(rng.choice(GROUPS)) or n
    dtype = torch.float16 if rng.random() < 0.6 else torch.float32
    qdtype = torch.float16 if rng.random() < 0.5 else torch.float32
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    rows = torch.randn(n, d, generator=g)
    labels = torch.randperm(n // gs + 1, generator=g)[torch.arange(n) // gs]
    if rng.random() < 0.4:  # near-duplicate rows inside a group
        rows = rows[torch.arange(n) // gs * gs] + 0.03 * torch.randn(n, d, generator=g)
    if rng.random() < 0.2 and n > 4:  # exact copies
        rows[n // 2 : n // 2 + n // 4] = rows[: n // 4].clone()
    rows = torch.nn.functional.normalize(rows, dim=1)
    src = torch.randint(0, n, (nq,), generator=g)
    q = (rows[src] + float(rng.choice([0.0, 0.05, 0.5])) * torch.randn(nq, d, generator=g)).to(qdtype).to(dev)
    kmax = min(int(rng.choice(KS)), n)
    k = int(rng.integers(1, kmax + 1))
    eb = EmbeddingBank(rows.to(dev), dtype=dtype, normalize=False, row_groups=labels)
    kw = {}
    if rng.random() < 0.3:
        kw["mask"] = (torch.rand(n, generator=g) < 0.5).to(dev)
    if rng.random() < 0.3:
        kw["exclude_group"] = labels[src]
    got = eb.search_groups(q, k, **kw)
    st = eb.last_status.cpu().tolist()
    exp = eb.search_groups_exhaustive(q, k, **kw)
    cases += 1
    redone += st[1]
    exhaustive += st[3]
    ok = torch.equal(got[1], exp[1]) and torch.equal(got[2], exp[2]) and \
        torch.equal(got[0].view(torch.int32), exp[0].view(torch.int32))
    if not ok:
        fails += 1
        print(json.dumps({"FAIL": True, "n": n, "d": d, "q": nq, "k": k, "group": gs, "dtype": str(dtype),
                          "qdtype": str(qdtype), "mask": "mask" in kw, "exclude": "exclude_group" in kw, "status": st}),
              flush=True)
    del eb
print(json.dumps({"cases": cases, "failures": fails, "queries_redone": redone, "exhaustive_queries": exhaustive,
                  "seed": seed, "seconds": budget}), flush=True)
sys.exit(1 if fails else 0)
