"""Timing and peak memory of `PCA.fit_bank` and `EmbeddingBank.project` at 1 M x 768 fp16, K = 128, against the only route
to the same result without them (not the contract bench; see bench.py):

  packed     `PCA.fit_bank(bank)`                           then `bank.project(pca)`
  unpacked   `x = bank.bank.float()`, `PCA.fit(x)`          then `EmbeddingBank(pca.transform(x), dtype=fp16)`

One process, device events around each call (a fit ends in the host's D x D eigenproblem, which both routes share and the
events include), the median of 5 after 3 warm-ups.  `gram` is the Gram launch alone (`_gram_rows`, mean given), whose
D^2 N flops are set against the 157 TF/s the f32 matrix cores are stated to reach.  Peak memory is
`max_memory_allocated` above what was allocated before the call (the bank itself is part of the baseline).
Usage: python scripts/quick_bank_pca_bench.py [--out FILE.json] [--rows N] [--dim D] [--components K]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import PCA, EmbeddingBank  # noqa: E402

N, D, K = 1_000_000, 768, 128
WARMUP, REPS = 3, 5
F32_MATRIX_TFLOPS = 157.0
args = sys.argv[1:]
out_path = None


def take(flag: str, default):
    if flag in args:
        i = args.index(flag)
        value = args[i + 1]
        del args[i : i + 2]
        return type(default)(value)
    return default


out_path = take("--out", "")
N, D, K = take("--rows", N), take("--dim", D), take("--components", K)
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
scale = torch.linspace(2.0, 0.1, D, device=dev)
bank = EmbeddingBank(torch.empty((0, D), device=dev), dtype=torch.float16, normalize=False, capacity=N)
for r0 in range(0, N, 1 << 18):
    blk = torch.randn(min(1 << 18, N - r0), D, generator=g, device=dev) * scale + 0.5
    bank.append(blk.half())
    del blk
out = []


def emit(line: dict) -> None:
    print(json.dumps(line), flush=True)
    out.append(line)


def measure(fn, reset=lambda: None) -> tuple[float, float, object]:
    """(median ms, peak MiB above the baseline of the last run, the last result); `reset` drops what the previous run kept
    before the baseline is taken."""
    times, peak, result = [], 0.0, None
    for i in range(WARMUP + REPS):
        result = None
        reset()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        result = fn()
        e1.record()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2**20
        if i >= WARMUP:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), peak, result


def new_pca() -> PCA:
    return PCA(min_num_components=K, max_num_components=K)


packed_mib = bank._bank.numel() / 2**20
fit_ms, fit_peak, pca = measure(lambda: new_pca().fit_bank(bank))
emit({"route": "packed", "call": "fit_bank", "N": N, "D": D, "ms": round(fit_ms, 2), "peak_mib": round(fit_peak, 1)})

mean = pca.feature_means.reshape(-1).contiguous()


def gram_only():
    gram = torch.zeros((D, D), dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    bank._gram_rows(mean, bank._as_filter(None), gram, count)
    return gram


gram_ms, _, _ = measure(gram_only)
tflops = D * D * N / (gram_ms * 1e-3) / 1e12
emit({"route": "packed", "call": "gram", "ms": round(gram_ms, 3), "tflops_d2n": round(tflops, 1),
      "fraction_of_f32_matrix_peak": round(tflops / F32_MATRIX_TFLOPS, 3)})

proj_ms, proj_peak, proj = measure(lambda: bank.project(pca))
emit({"route": "packed", "call": "project", "K": K, "ms": round(proj_ms, 2), "peak_mib": round(proj_peak, 1),
      "new_bank_mib": round(proj._bank.numel() / 2**20, 1)})
del proj

held = {}


def unpacked_fit():
    held["x"] = bank.bank.float()
    return new_pca().fit(held["x"])


ufit_ms, ufit_peak, upca = measure(unpacked_fit, held.clear)
emit({"route": "unpacked", "call": "bank.bank.float() + fit", "ms": round(ufit_ms, 2), "peak_mib": round(ufit_peak, 1)})


def unpacked_project():
    return EmbeddingBank(upca.transform(held["x"]), dtype=torch.float16, normalize=True)


# `x` is kept from the fit, as a caller of the unpacked route would keep it: its 4 N D bytes are that route's to count
uproj_ms, uproj_peak, _ = measure(unpacked_project)
x_mib = held["x"].numel() * 4 / 2**20
emit({"route": "unpacked", "call": "transform + EmbeddingBank", "ms": round(uproj_ms, 2),
      "peak_mib": round(uproj_peak + x_mib, 1), "of_which_x_mib": round(x_mib, 1)})
emit({"packed_bank_mib": round(packed_mib, 1), "fit_speedup": round(ufit_ms / fit_ms, 2),
      "project_speedup": round(uproj_ms / proj_ms, 2),
      "max_abs_diff_of_explained_variance": float((pca.explained_variance - upca.explained_variance).abs().max())})
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
