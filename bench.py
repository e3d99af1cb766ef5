#!/usr/bin/env python3
"""Headline benchmark of the embed-and-search hot path on MI355X (contract: see the build prompt / DESIGN.md).

    python bench.py --gpus N --steps K --warmup W            # any N: for N > 1 without a launcher (WORLD_SIZE unset)
                                                             # it starts the N ranks itself (torch.distributed.run child)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W                 # N > 1, one rank per GPU over RCCL

Primary workload (`--workload search`, BASELINE.json config 3/4): cosine top-10 of 1024 fp16 queries against a
10,000,000 x 768 fp16 bank.  STRONG scaling: the bank is fixed -- the same rows whatever N is (every 2^20-row block
has its own seed) -- and row-sharded over the N ranks (rank r generates rows [r*N/G, (r+1)*N/G) on its device); a
step is one `EmbeddingBank.search` call -- local MFMA filter + exact re-score (+ exact redo of what the filter cannot
prove, on the device), one RCCL all-gather of the Q x k partials, merge.  `value` = queries/s.

`--workload encode` makes the encode the primary metric instead (replicas: every rank encodes its own batch of
512, weak scaling, no collective).

A plain run sets up, warms up, times exactly `--steps` steps and reports them; nothing else.  `--full` adds, after the
timed steps: the per-kernel roofline (a second, bracketed loop of the same steps), the self-check -- every rank PROVES
the merged answer on its shard (float64 on the device, "selfcheck" in the JSON line) --, the query-count / shard-size
sweeps and bank variants (N = 1), the CPU baselines, and, for `--workload search`, secondary lines on rank 0's GPU:
under "encode" ResNet-50 -> 768-d float32 `predict_step` on 512 random 224 x 224 uint8 images (BASELINE.json config 2),
images/s; under "encode_vit_b16" the same batch through the ViT-B/16 fp16 embedder (config 5); under
"encode_efficientnet_v2_s" the reference's own EfficientNetV2-S embedder.  `--no-sweep`, `--no-secondary` and
`--no-cpu-baseline` leave parts of that out.

`--dump-outputs DIR` writes what the timed path returned in its last timed step (rank 0's copy) as DIR/<name>.npy:
floating point as float32, integer indices as float64 (exact below 2^53).  The inputs are seeded, so two builds run
with the same arguments can be compared output for output.

Rank 0 prints ONE JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path


def _self_launch() -> None:
    """`python bench.py --gpus N` with N > 1 and no launcher around it (WORLD_SIZE unset): start the N ranks here, as ONE
    child `python -m torch.distributed.run ... bench.py <same arguments>`, and exit with its code.  This runs before
    torch or the HIP library is imported: the parent never touches a GPU (a process that has initialised HIP must not
    spawn the ranks' runtime), it only waits."""
    if "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    gpus = 1
    argv = sys.argv[1:]
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            gpus = int(argv[i + 1])
        elif a.startswith("--gpus="):
            gpus = int(a.split("=", 1)[1])
    if gpus <= 1:
        return
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]
    print(f"bench.py: WORLD_SIZE unset, starting {gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    raise SystemExit(subprocess.call(cmd, env=env))


if __name__ == "__main__":
    _self_launch()

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from imagescry_amd import (  # noqa: E402
    EfficientNetEmbedder, EmbeddingBank, ImageBatch, ResNet50Embedder, ViTB16Embedder, _lib, efficientnet, resnet50,
    shard_bounds, vit,
)

SEED = 1234
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16/bf16
MFMA_F32_PEAK_TFLOPS = 157.3  # f32-input MFMA == vector rate


def parse_args() -> argparse.Namespace:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["search", "encode", "pipeline"], default="search")
    ap.add_argument("--bank-rows", type=int, default=10_000_000, help="total bank rows (all ranks together)")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=512, help="encode batch (images per step per rank)")
    ap.add_argument("--pipeline-rows", type=int, default=50_000_000, help="bank rows of --workload pipeline (all ranks)")
    ap.add_argument("--no-overlap", action="store_true", help="--workload pipeline: one stream instead of two")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: roofline, self-check, sweeps, bank "
                         "variants, CPU baselines, secondary encode lines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--no-secondary", action="store_true", help="--full without the secondary encode lines")
    ap.add_argument("--no-sweep", action="store_true",
                    help="--full without the query-count / shard-size sweeps and bank variants (N = 1 only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def setup_dist(args: argparse.Namespace) -> tuple[int, int, torch.device]:
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:  # a launcher started a different number of ranks than asked for
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node must equal --gpus")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    # ISC_BENCH_BACKEND=gloo rehearses the N > 1 path on a box with fewer GPUs than ranks (ranks share devices)
    backend = os.environ.get("ISC_BENCH_BACKEND", "nccl")
    if backend == "nccl" and world > torch.cuda.device_count():
        raise SystemExit(f"--gpus {world} over RCCL needs {world} devices, {torch.cuda.device_count()} visible "
                         f"(ISC_BENCH_BACKEND=gloo rehearses the path with ranks sharing a device)")
    device = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, device


def _collective_device(device: torch.device) -> torch.device:
    return torch.device("cpu") if dist.get_backend() == "gloo" else device


def fence(world: int) -> None:
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize()


def max_over_ranks(seconds: float, world: int, device: torch.device) -> float:
    if world == 1:
        return seconds
    t = torch.tensor([seconds], dtype=torch.float64, device=_collective_device(device))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def timed_steps(step, steps: int, warmup: int, world: int, device: torch.device) -> float:
    """W untimed steps, then EXACTLY `steps` steps between barrier + synchronize; max over ranks, seconds."""
    for _ in range(warmup):
        step()
    fence(world)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    fence(world)
    return max_over_ranks(time.perf_counter() - t0, world, device)


def bracketed_kernel_ms(step, steps: int, kernel_id: int) -> tuple[float, int]:
    """(summed device ms inside the instrumented kernel, KERNEL launches) over `steps` more steps, run with the event
    brackets on -- a loop of its own, after the loop `value` was timed in."""
    torch.cuda.synchronize()
    _lib.timing_enable(True)
    _lib.timing_read(kernel_id)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    out = _lib.timing_read(kernel_id)
    _lib.timing_enable(False)
    return out


# ------------------------------------------------------------------------------------------------ search
BLOCK_ROWS = 1 << 20


def make_shard(lo: int, hi: int, dim: int, device: torch.device, seed: int = SEED) -> torch.Tensor:
    """Rows [lo, hi) of THE bank: random unit-norm fp16 rows generated on the device, block b = rows [b * 2^20,
    (b + 1) * 2^20) from seed + b -- the bank is the same whatever the number of ranks (SURVEY.md section 8d input 4
    asked for seed 1234 + rank, which makes every world size a different bank and the runs incomparable)."""
    out = torch.empty((hi - lo, dim), dtype=torch.float16, device=device)
    for b in range(lo // BLOCK_ROWS, (hi + BLOCK_ROWS - 1) // BLOCK_ROWS):
        g = torch.Generator(device=device).manual_seed(seed + b)
        blk = torch.nn.functional.normalize(torch.randn((BLOCK_ROWS, dim), generator=g, device=device), dim=1).half()
        b0 = b * BLOCK_ROWS
        s0, s1 = max(lo, b0), min(hi, b0 + BLOCK_ROWS)
        out[s0 - lo : s1 - lo] = blk[s0 - b0 : s1 - b0]
    return out


def selfcheck(shard: torch.Tensor, lo: int, queries: torch.Tensor, scores: torch.Tensor, indices: torch.Tensor,
              world: int, device: torch.device) -> dict:
    """Proof, on the device and outside the timed region, that (scores, indices) is the cosine top-k of `queries` over
    the WHOLE bank, each rank vouching for its shard (rows [lo, lo + len(shard)), row-major):
      identical      every rank holds the same merged result (min == max of a checksum over the ranks);
      scores_exact   the scores of the returned rows this rank owns equal float32(their float64 cosine) BIT FOR BIT
                     (`scores_max_abs_diff` reports the largest difference, 0.0 when exact);
      kth_is_kth     the rows of this shard that rank before the k-th entry (score desc, index asc), summed over the
                     ranks, are exactly k - 1 per query -- nothing outside the answer beats it, nothing is missing;
      sorted         every result row is ordered."""
    q, k = scores.shape
    n_local, d = shard.shape
    q64 = queries.double()
    denom = q64.norm(dim=1).clamp_min(1e-12)
    s64 = scores.double()
    sorted_ok = bool(((s64[:, :-1] > s64[:, 1:]) | ((s64[:, :-1] == s64[:, 1:]) & (indices[:, :-1] < indices[:, 1:]))).all())
    mine = (indices >= lo) & (indices < lo + n_local)
    qi, ki = mine.nonzero(as_tuple=True)
    rows = shard[indices[qi, ki] - lo].double()
    exact = ((rows * q64[qi]).sum(dim=1) / denom[qi]).float()
    exact_ok = bool(torch.equal(exact, scores[qi, ki]))  # bit for bit: the search's scores ARE float32(float64 cosine)
    max_diff = float((exact.double() - scores[qi, ki].double()).abs().max()) if exact.numel() else 0.0
    kth, kth_idx = s64[:, -1], indices[:, -1]
    ahead = torch.zeros(q, dtype=torch.int64, device=device)
    blk = 1 << 17
    for r0 in range(0, n_local, blk):
        sc = (q64 @ shard[r0 : r0 + blk].double().T / denom[:, None]).float().double()
        ridx = torch.arange(lo + r0, lo + r0 + sc.shape[1], device=device)[None, :]
        ahead += ((sc > kth[:, None]) | ((sc == kth[:, None]) & (ridx < kth_idx[:, None]))).sum(dim=1)
    w = torch.arange(1, k + 1, device=device, dtype=torch.int64)
    checksum = ((indices * w).sum() + (scores.view(torch.int32).long() * w).sum()).reshape(1)
    cmin, cmax = checksum.clone(), checksum.clone()
    flags = torch.tensor([int(sorted_ok), int(exact_ok)], dtype=torch.int64, device=device)
    diff = torch.tensor([max_diff], dtype=torch.float64, device=device)
    if world > 1:
        cd = _collective_device(device)
        ahead, cmin, cmax, flags, diff = ahead.to(cd), cmin.to(cd), cmax.to(cd), flags.to(cd), diff.to(cd)
        dist.all_reduce(ahead, op=dist.ReduceOp.SUM)
        dist.all_reduce(cmin, op=dist.ReduceOp.MIN)
        dist.all_reduce(cmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(flags, op=dist.ReduceOp.MIN)
        dist.all_reduce(diff, op=dist.ReduceOp.MAX)
    out = {
        "identical_on_all_ranks": bool((cmin == cmax).item()),
        "scores_exact": bool(flags[1].item()),
        "scores_max_abs_diff": float(diff.item()),
        "kth_is_kth": bool((ahead == k - 1).all().item()),
        "sorted": bool(flags[0].item()),
        "checksum": int(cmin.item()),
    }
    out["ok"] = all(v for v in out.values() if isinstance(v, bool))  # floats (the diff) are reported, not judged
    return out


def measured_traffic(config: dict) -> tuple[float | None, str | None, bool]:
    """HBM bytes per `k_dots_filter` launch from the newest committed PMC summary whose workload equals `config`
    (profiles/*_headline_traffic.json, written by scripts/summarize_headline_traffic.py from separate rocprofv3
    --pmc FETCH_SIZE / WRITE_SIZE passes; counters cannot be read from inside this process)."""
    keys = ("bank_rows", "dim", "queries", "k", "rows_per_gpu")
    for f in sorted((ROOT / "profiles").glob("*_headline_traffic.json"), reverse=True):
        try:
            t = json.loads(f.read_text())
        except (OSError, ValueError):
            continue
        if all(t.get("config", {}).get(k) == config.get(k) for k in keys):
            # per STEP when the summary has it (the number of launches per step is a tuning knob), else per launch
            return float(t.get("hbm_bytes_per_step", t["hbm_bytes_per_launch"])), f"profiles/{f.name}", "hbm_bytes_per_step" in t
    return None, None, False


def measured_encoder_traffic(model: str, batch: int) -> tuple[float | None, str | None, float | None]:
    """L2 <-> fabric bytes per `k_conv_f32` launch of one encoder's predict_step from the newest committed PMC summary of
    the kernel bench.py times (profiles/*_<model>_traffic.json: scripts/pmc_encoder.sh + scripts/summarize_encoder_traffic.py;
    the round-1/2 `*_encode_traffic.json` files were taken on kernels that are no longer built and are not read)."""
    for f in sorted((ROOT / "profiles").glob(f"*_{model}_traffic.json"), reverse=True):
        try:
            t = json.loads(f.read_text())
        except (OSError, ValueError):
            continue
        if t.get("config", {}).get("batch_per_gpu") == batch and t.get("config", {}).get("model") == model:
            return float(t["hbm_bytes_per_launch"]), f"profiles/{f.name}", t.get("traffic_over_algorithmic")
    return None, None, None


def measured_vit_traffic(batch: int) -> tuple[float | None, str | None, float | None]:
    """L2 <-> fabric bytes per `k_gemm_f16` launch of the ViT-B/16 step from the newest committed PMC summary
    (profiles/*_vit_traffic.json, scripts/pmc_gemm.sh): average over the four GEMM shapes of an encoder layer."""
    for f in sorted((ROOT / "profiles").glob("*_vit_traffic.json"), reverse=True):
        try:
            t = json.loads(f.read_text())
        except (OSError, ValueError):
            continue
        if t.get("config", {}).get("batch_per_gpu") == batch:
            return float(t["hbm_bytes_per_launch"]), f"profiles/{f.name}", t.get("traffic_over_algorithmic")
    return None, None, None


def search_roofline(rows: int, d: int, q: int, k: int, kernel_ms_per_step: float, launches_per_step: float) -> dict:
    """Roofline entry of k_dots_filter for one search step on one rank.  Algorithmic work:
    every local bank row is read once (2 B / element) and dotted with every query."""
    flops = 2.0 * q * rows * d
    nbytes = rows * d * 2.0 + q * d * 2.0 + q * k * 12.0
    sec = kernel_ms_per_step / 1e3
    tflops = flops / sec / 1e12
    gbs = nbytes / sec / 1e9
    # arithmetic intensity ~ q flop/byte (fp16 bank): the MFMA roofline binds above ~310 queries, HBM below
    ridge = MFMA_F16_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9)
    bound = "mfma" if flops / nbytes >= ridge else "hbm"
    return {
        "kernel": "k_dots_filter<f16>",
        "bound": bound,
        "achieved": round(tflops if bound == "mfma" else gbs, 2),
        "peak": MFMA_F16_PEAK_TFLOPS if bound == "mfma" else HBM_PEAK_GBS,
        "unit": "TFLOP/s" if bound == "mfma" else "GB/s",
        "frac": round((tflops / MFMA_F16_PEAK_TFLOPS) if bound == "mfma" else (gbs / HBM_PEAK_GBS), 4),
        "traffic": None,
        "launches_per_step": launches_per_step,
        "avg_launch_ms": round(kernel_ms_per_step / max(launches_per_step, 1e-9), 4),
        "kernel_ms_per_step": round(kernel_ms_per_step, 4),
        "algorithmic_flops_per_step": flops,
        "algorithmic_bytes_per_step": nbytes,
        "mfma_frac": round(tflops / MFMA_F16_PEAK_TFLOPS, 4),
        "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
    }


def query_sweep(bank: EmbeddingBank, rows: int, d: int, k: int, device: torch.device,
                qs: tuple[int, ...] = (1, 16, 64, 128, 256, 512, 1024)) -> list[dict]:
    """the same bank searched with 1 .. 1024 queries, so that the HBM-bound regime
    (few queries) is measured directly beside the MFMA-bound headline.  End-to-end time is taken with the per-kernel
    event brackets OFF; a second loop with them on gives the time inside k_dots_filter, and their difference is what a
    search spends outside the streaming kernel (prep, selections, exact re-score, launch gaps)."""
    out = []
    for q in qs:
        queries = torch.randn((q, d), generator=torch.Generator().manual_seed(SEED + q)).half().to(device)
        for _ in range(3):
            bank.search(queries, k)
        steps = 20 if rows * q <= 2e9 else 8
        rounds = []
        for _ in range(3):  # three rounds, the median: one host hiccup in a 5 - 40 ms window moved a row by 20 %
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                bank.search(queries, k)
            torch.cuda.synchronize()
            rounds.append((time.perf_counter() - t0) / steps)
        sec = sorted(rounds)[1]
        # the same searches as a STREAM: search i + 1 is issued before handle i is resolved, so the bank runs them on its
        # two alternating streams and the short kernels at the end of one search overlap the first kernels of the next
        for _ in range(4):
            bank.search_async(queries, k).result()
        rounds = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pending = None
            for _ in range(steps):
                h = bank.search_async(queries, k)
                if pending is not None:
                    pending.result()
                pending = h
            pending.result()
            torch.cuda.synchronize()
            rounds.append((time.perf_counter() - t0) / steps)
        sec_stream = sorted(rounds)[1]
        _lib.timing_enable(True)
        _lib.timing_read(_lib.ISC_KERNEL_DOTS_FILTER)
        for _ in range(steps):
            bank.search(queries, k)
        torch.cuda.synchronize()
        kernel_ms, launches = _lib.timing_read(_lib.ISC_KERNEL_DOTS_FILTER)
        _lib.timing_enable(False)
        r = search_roofline(rows, d, q, k, kernel_ms / steps, launches / steps)
        out.append({
            "queries": q, "rows_per_gpu": rows, "ms_per_search": round(sec * 1e3, 4),
            "queries_per_s": round(q / sec, 1),
            "bank_gb_per_s_end_to_end": round(rows * d * 2.0 / sec / 1e9, 1),
            "hbm_frac_end_to_end": round(rows * d * 2.0 / sec / 1e9 / HBM_PEAK_GBS, 4),
            "ms_per_search_streamed": round(sec_stream * 1e3, 4),
            "hbm_frac_streamed": round(rows * d * 2.0 / sec_stream / 1e9 / HBM_PEAK_GBS, 4),
            "kernel_ms": r["kernel_ms_per_step"], "us_outside_dots_filter": round((sec * 1e3 - r["kernel_ms_per_step"]) * 1e3, 1),
            "bound": r["bound"], "frac": r["frac"],
            "mfma_frac": r["mfma_frac"], "hbm_frac": r["hbm_frac"],
            "exact_pass_queries": int(bank.last_status[1].item()),
        })
    return out


def scaling_projection(sweep: list[dict], n: int) -> dict:
    """A PROJECTION, not a measurement: what the 1 -> 8 GPU strong-scaling curve of the search would be if every rank ran
    its shard as this one GPU runs a shard of that size (`q_sweep` rows with rows_per_gpu = n / G, searches issued as a
    stream) and the exchange -- one all-gather of Q x k x 12 B per rank + the merge, on the bank's exchange stream under
    the next search's local kernels -- cost nothing on the critical path.  The compute side only; the RCCL exchange has
    not been timed.  The driver's SCALE run is the measurement."""
    out = {"kind": "projection from single-GPU shard timings (exchange not included)", "rows": []}
    for q in (64, 1024):
        base = next((r for r in sweep if r["queries"] == q and r["rows_per_gpu"] == n), None)
        for g in (1, 2, 4, 8):
            r = next((r for r in sweep if r["queries"] == q and r["rows_per_gpu"] == n // g), None)
            if r is None or base is None:
                continue
            ms = r["ms_per_search_streamed"]
            out["rows"].append({"n_gpus": g, "queries": q, "ms_per_search": ms, "queries_per_s": round(q / ms * 1e3, 1),
                                "speedup_vs_1": round(base["ms_per_search_streamed"] / ms, 3),
                                "efficiency": round(base["ms_per_search_streamed"] / ms / g, 3),
                                "hbm_frac_per_gpu": r["hbm_frac_streamed"], "mfma_frac_per_gpu": r["mfma_frac"]})
    return out


def merge_us(bank: EmbeddingBank, q: int, k: int, device: torch.device, g: int = 8, reps: int = 50) -> float:
    """Device time of one `isc_topk_merge` of `g` shards' partial results ([g, q, k], what every rank of a g-GPU search
    runs behind its all-gather), microseconds, from HIP events over `reps` back-to-back launches on the current stream."""
    gen = torch.Generator().manual_seed(SEED + q)
    s = torch.randn((g, q, k), generator=gen).sort(dim=2, descending=True).values.to(device)
    i = torch.randint(0, 1 << 40, (g, q, k), generator=gen).to(device)
    for _ in range(3):
        bank._merge_topk(s, i, k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        bank._merge_topk(s, i, k)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def time_search(bank: EmbeddingBank, queries: torch.Tensor, k: int, steps: int) -> tuple[float, list[int]]:
    for _ in range(2):
        bank.search(queries, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        bank.search(queries, k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, bank.last_status.cpu().tolist()


def bank_variants(n: int, d: int, q: int, k: int, device: torch.device, iid_ms: float) -> list[dict]:
    """The same search on banks that are NOT exchangeable random rows (N = 1 only, outside the timed region of `value`):
      dup8              every row stored 8 times -- the store holds an image indexed twice, uniform patches, ... -- so the
                        k-th neighbour of every query ties with copies the filter cannot order: every query is searched
                        a second time (one more matrix-core pass for all of them together, k_final2);
      image_ordered_49  rows arrive in the reference's store order (record, h, w): 49 adjacent near-duplicate cells per
                        image (src/imagescry/storage/operations.py:135-144)."""
    out = []
    queries = torch.randn((q, d), generator=torch.Generator().manual_seed(SEED)).half().to(device)

    def run(name: str, rows: torch.Tensor, note: str) -> None:
        bank = EmbeddingBank(rows, dtype=torch.float16, normalize=False)
        del rows
        torch.cuda.empty_cache()
        sec, st = time_search(bank, queries, k, 5)
        out.append({"bank": name, "rows": n, "queries": q, "ms_per_search": round(sec * 1e3, 3),
                    "queries_per_s": round(q / sec, 1), "vs_iid": round(sec * 1e3 / iid_ms, 3),
                    "searched_again_queries": st[1], "exhaustive_pass_queries": st[3],
                    "overflowed_candidate_buffers": st[0], "note": note})
        del bank
        torch.cuda.empty_cache()

    base = make_shard(0, n // 8, d, device, seed=SEED + 1000)
    run("dup8", base.repeat(8, 1), "every row stored 8 times (original order: copy c of row r at c * N/8 + r)")
    del base
    cells = 49
    images = (n + cells - 1) // cells
    rows = torch.empty((n, d), dtype=torch.float16, device=device)
    g = torch.Generator(device=device).manual_seed(SEED + 2000)
    blk = 1 << 14  # images per block
    for i0 in range(0, images, blk):
        ni = min(blk, images - i0)
        centre = torch.randn((ni, 1, d), generator=g, device=device)
        cell = centre + 0.05 * torch.randn((ni, cells, d), generator=g, device=device)
        flat = torch.nn.functional.normalize(cell, dim=2).half().reshape(ni * cells, d)
        r0 = i0 * cells
        rows[r0 : r0 + flat.shape[0]] = flat[: n - r0]
    run("image_ordered_49", rows, "49 adjacent near-duplicate cells per image, in store order")
    return out


def bench_search(args: argparse.Namespace, rank: int, world: int, device: torch.device) -> dict:
    n, d, q, k = args.bank_rows, args.dim, args.queries, args.k
    lo, hi = shard_bounds(n, world, rank)
    shard = make_shard(lo, hi, d, device)
    queries = torch.randn((q, d), generator=torch.Generator().manual_seed(SEED)).half().to(device)
    group = dist.group.WORLD if world > 1 else None
    bank = EmbeddingBank(shard, dtype=torch.float16, normalize=False, index_base=lo, process_group=group,
                         presharded=True)

    pending: list = []

    def step() -> None:
        # a stream of searches: search i is enqueued, THEN the handle of search i - 1 is resolved on this stream, so on
        # a sharded bank the all-gather + merge of i - 1 (the bank's exchange stream) run under the local kernels of i.
        # The closing fence synchronises the whole device, i.e. the last exchange too.
        pending.append(bank.search_async(queries, k))
        if len(pending) > 1:
            pending.pop(0).result()

    # `value` is timed with the per-kernel event brackets OFF; the time inside k_dots_filter comes from a SECOND loop of
    # the same steps with them on (two extra event records per launch stretch a step by a fraction of a percent, which
    # must not sit inside the number that is quoted).  scripts/trace_headline.sh reproduces `kernel_ms_per_step` from a
    # rocprofv3 kernel trace of this same command by launch index (profiles/*_headline_trace.json).
    seconds = timed_steps(step, args.steps, args.warmup, world, device)
    scores, indices = pending.pop().result()  # the answer of the last timed step (the only handle still pending)
    rows = hi - lo
    out = {
        "metric": "queries/s cosine top-10 over N x D bank",
        "value": round(q * args.steps / seconds, 1),
        "unit": "queries/s",
        "ms_per_step": round(seconds / args.steps * 1e3, 4),
        "scaling": "strong",
        "dtype": "f16",
        "config": {
            "workload": f"cosine top-{k}: {q} fp16 queries x {n} x {d} fp16 bank (BASELINE config 4 bank; "
                        f"row-sharded {world} way{'s' if world > 1 else ''})",
            "bank_rows": n, "dim": d, "queries": q, "k": k, "rows_per_gpu": rows,
            "parallelism": f"row-shard{world}" + ("+allgather" if world > 1 else ""),
        },
        "roofline": None,
        "_outputs": {"scores": scores, "indices": indices},
    }
    if not args.full:
        return out
    _lib.timing_enable(True)
    _lib.timing_read(_lib.ISC_KERNEL_DOTS_FILTER)
    seconds_bracketed = timed_steps(step, args.steps, 0, world, device)
    while pending:
        pending.pop(0).result()
    kernel_ms, launches = _lib.timing_read(_lib.ISC_KERNEL_DOTS_FILTER)
    _lib.timing_enable(False)
    status = bank.last_status.cpu().tolist()
    scores, indices = bank.search(queries, k)
    check = selfcheck(shard, lo, queries, scores, indices, world, device)
    check["backend"] = dist.get_backend() if world > 1 else "none (single process)"
    check["world_size"] = dist.get_world_size() if world > 1 else 1
    del shard
    torch.cuda.empty_cache()

    roofline = search_roofline(rows, d, q, k, kernel_ms / args.steps, launches / args.steps)
    roofline["ms_per_step_with_brackets"] = round(seconds_bracketed / args.steps * 1e3, 4)
    roofline["search_calls_in_order"] = {"warmup": args.warmup, "timed": args.steps, "bracketed": args.steps, "selfcheck": 1}
    sweep = None
    if world == 1 and not args.no_sweep:
        sweep = query_sweep(bank, rows, d, k, device)
        # the shard one GPU holds when the same bank is split over 2 / 4 / 8 GPUs (8: what the north-star 70 %-of-HBM
        # target is about): the per-GPU work of the strong-scaling curve, measured on this one GPU
        for g in (2, 4, 8):
            shard_rows = n // g
            if shard_rows < 100_000:
                continue
            small = EmbeddingBank(make_shard(0, shard_rows, d, device), dtype=torch.float16, normalize=False)
            torch.cuda.empty_cache()
            shard_sweep = query_sweep(small, shard_rows, d, k, device, qs=(1, 16, 64, 1024) if g == 8 else (64, 1024))
            for row in shard_sweep:  # what every rank of the g-GPU search runs behind its all-gather
                row["merge_us"] = merge_us(small, row["queries"], k, device, g=g)
                row["shards"] = g
                if g == 8:
                    row["merge_us_g8"] = row["merge_us"]
            sweep += shard_sweep
            del small
            torch.cuda.empty_cache()
    variants = None
    if world == 1 and not args.no_sweep and n >= 1_000_000:
        del bank
        torch.cuda.empty_cache()
        variants = bank_variants(n, d, q, k, device, seconds / args.steps * 1e3)
        bank = None
    traffic, traffic_src, per_step = measured_traffic({"bank_rows": n, "dim": d, "queries": q, "k": k, "rows_per_gpu": rows})
    if traffic_src:
        lps = max(roofline["launches_per_step"], 1e-9)
        step_bytes = traffic if per_step else traffic * lps
        roofline["traffic"] = step_bytes / lps  # per launch, like `achieved`
        roofline["traffic_per_step"] = step_bytes
        roofline["traffic_source"] = traffic_src
        roofline["traffic_over_algorithmic"] = round(step_bytes / roofline["algorithmic_bytes_per_step"], 3)
    return {
        **out,
        "roofline": roofline,
        "selfcheck": check,
        "overflowed_candidate_buffers": status[0],
        "exact_pass_queries": status[1],  # queries the first pass could not prove (searched again on the device)
        "exhaustive_pass_queries": status[3],
        "q_sweep": sweep,
        "scaling_projection": scaling_projection(sweep, n) if sweep else None,
        "bank_variants": variants,
        "_bank": bank, "_queries": queries,
    }


def cpu_baseline_search(args: argparse.Namespace) -> dict:
    """The oracle's float32 torch expression on the host cores, on a bounded row sample of the same workload."""
    from oracle import search_oracle

    sample_rows = min(args.bank_rows, 1_000_000)
    g = torch.Generator().manual_seed(SEED)
    bank = torch.nn.functional.normalize(torch.randn((sample_rows, args.dim), generator=g), dim=1)
    queries = torch.randn((args.queries, args.dim), generator=torch.Generator().manual_seed(SEED)).half().float()
    cores = torch.get_num_threads()
    search_oracle.cosine_topk_torch_blocked(bank[: sample_rows // 8], queries, args.k)  # warm-up
    reps, t0 = 0, time.perf_counter()
    while reps < 2 or (time.perf_counter() - t0 < 8.0 and reps < 10):
        search_oracle.cosine_topk_torch_blocked(bank, queries, args.k)
        reps += 1
    per_pass = (time.perf_counter() - t0) / reps
    scaled = per_pass * args.bank_rows / sample_rows  # cost is linear in the bank rows
    return {
        "value": round(args.queries / scaled, 2),
        "unit": "queries/s",
        "cores": cores,
        "kind": "port",
        "sample_fraction": round(sample_rows / args.bank_rows, 4),
        "sample": f"oracle.search_oracle.cosine_topk_torch_blocked (float32 GEMM + topk), {args.queries} queries x "
                  f"{sample_rows} of the {args.bank_rows} rows ({100.0 * sample_rows / args.bank_rows:.0f} % sample), "
                  f"{reps} passes of {per_pass:.2f} s, scaled linearly to the full bank; a stated baseline of a stock "
                  f"torch CPU build, not a tuned CPU search -- do not quote the GPU/CPU ratio",
        "gflops": round(2.0 * args.queries * sample_rows * args.dim / per_pass / 1e9, 1),
    }


# ------------------------------------------------------------------------------------------------ encode
def bench_encode(args: argparse.Namespace, rank: int, world: int, device: torch.device, steps: int, warmup: int,
                 collective_timing: bool, full: bool) -> dict:
    b = args.batch
    model = ResNet50Embedder(seed=0).to(device)
    images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(SEED + rank)).to(device)
    batch = ImageBatch(indices=torch.arange(b, device=device), images=images)
    last: list = [None]

    def step() -> None:
        last[0] = model.predict_step(batch)

    seconds = timed_steps(step, steps, warmup, world if collective_timing else 1, device)  # brackets off
    ranks = world if collective_timing else 1
    out = {
        "metric": "images/s encode",
        "value": round(b * ranks * steps / seconds, 1),
        "unit": "images/s",
        "ms_per_step": round(seconds / steps * 1e3, 3),
        "scaling": "weak",
        "dtype": "f32",
        "config": {"workload": f"ResNet-50 (random weights) batch-{b} 224x224 uint8 -> 768-d predict_step, fp32 "
                               f"(BASELINE config 2)", "batch_per_gpu": b, "parallelism": f"replicas{ranks}"},
        "roofline": None,
        "_outputs": {"indices": last[0].indices, "embeddings": last[0].embeddings},
        "_model": model, "_images": images,
    }
    if not full:
        return out
    kernel_ms, launches = bracketed_kernel_ms(step, steps, _lib.ISC_KERNEL_CONV)
    flops = float(resnet50.conv_flops(b, 224, 224))
    tflops = flops * steps / (kernel_ms / 1e3) / 1e12
    enc_traffic, enc_traffic_src, enc_ratio = measured_encoder_traffic("resnet50", b)
    return {
        **out,
        "roofline": {
            "kernel": "k_conv_f32",
            "bound": "mfma",
            "achieved": round(tflops, 2),
            "peak": MFMA_F32_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(tflops / MFMA_F32_PEAK_TFLOPS, 4),
            "traffic": enc_traffic,
            "traffic_source": enc_traffic_src,
            "traffic_over_algorithmic": enc_ratio,
            "launches_per_step": launches / steps,
            "avg_launch_ms": round(kernel_ms / max(launches, 1), 4),
            "kernel_ms_per_step": round(kernel_ms / steps, 3),
            "algorithmic_flops_per_step": flops,
            "algorithmic_bytes_per_step": float(resnet50.conv_bytes(b, 224, 224)),
        },
    }


def bench_encode_vit(args: argparse.Namespace, device: torch.device, steps: int, warmup: int) -> dict:
    """BASELINE.json configs[4]: ViT-B/16 (random weights) -> 768-d, fp16 matrix-core arithmetic, batch 512."""
    b = args.batch
    model = ViTB16Embedder(seed=0).to(device)
    images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(SEED)).to(device)
    batch = ImageBatch(indices=torch.arange(b, device=device), images=images)
    seconds = timed_steps(lambda: model.predict_step(batch), steps, warmup, 1, device)  # brackets off
    kernel_ms, launches = bracketed_kernel_ms(lambda: model.predict_step(batch), steps, _lib.ISC_KERNEL_GEMM_F16)
    cfg = vit.VIT_B16
    t, d = cfg.tokens, cfg.dim
    gemm_flops = float(b) * (2 * (t - 1) * d * 3 * cfg.patch_size**2
                             + cfg.depth * (2 * t * d * 3 * d + 2 * t * d * d + 4 * t * d * cfg.mlp_dim))
    tflops = gemm_flops * steps / (kernel_ms / 1e3) / 1e12
    vit_traffic, vit_traffic_src, vit_ratio = measured_vit_traffic(b)
    return {
        "metric": "images/s encode",
        "value": round(b * steps / seconds, 1),
        "unit": "images/s",
        "ms_per_step": round(seconds / steps * 1e3, 3),
        "dtype": "f16",
        "config": {"workload": f"ViT-B/16 (random weights) batch-{b} 224x224 uint8 -> 768-d predict_step, fp16 operands / "
                               f"float32 accumulation (BASELINE config 5)", "batch_per_gpu": b, "parallelism": "replicas1"},
        "roofline": {
            "kernel": "k_gemm_f16",
            "bound": "mfma",
            "achieved": round(tflops, 2),
            "peak": MFMA_F16_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(tflops / MFMA_F16_PEAK_TFLOPS, 4),
            "traffic": vit_traffic,
            "traffic_source": vit_traffic_src,
            "traffic_over_algorithmic": vit_ratio,
            "launches_per_step": launches / steps,
            "avg_launch_ms": round(kernel_ms / max(launches, 1), 4),
            "kernel_ms_per_step": round(kernel_ms / steps, 3),
            "algorithmic_flops_per_step": gemm_flops,
        },
    }


def bench_encode_efficientnet(args: argparse.Namespace, device: torch.device, steps: int, warmup: int) -> dict:
    """The reference's own embedder (src/imagescry/models/embedding.py:108-183): EfficientNetV2-S features, float32,
    batch 512 at 224 x 224 -> [512, 1280, 7, 7] per-cell embeddings."""
    b = args.batch
    model = EfficientNetEmbedder(backbone_size="s", seed=0).to(device)
    images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(SEED)).to(device)
    batch = ImageBatch(indices=torch.arange(b, device=device), images=images)
    seconds = timed_steps(lambda: model.predict_step(batch), steps, warmup, 1, device)  # brackets off
    kernel_ms, launches = bracketed_kernel_ms(lambda: model.predict_step(batch), steps, _lib.ISC_KERNEL_CONV)
    flops = float(efficientnet.conv_flops("s", b, 224, 224))
    tflops = flops * steps / (kernel_ms / 1e3) / 1e12
    eff_traffic, eff_traffic_src, eff_ratio = measured_encoder_traffic("efficientnet_s", b)
    return {
        "metric": "images/s encode",
        "value": round(b * steps / seconds, 1),
        "unit": "images/s",
        "ms_per_step": round(seconds / steps * 1e3, 3),
        "dtype": "f32",
        "config": {"workload": f"EfficientNetV2-S (random weights, the reference's embedder) batch-{b} 224x224 uint8 -> "
                               f"[B,1280,7,7] predict_step, fp32", "batch_per_gpu": b, "parallelism": "replicas1"},
        "roofline": {
            "kernel": "k_conv_f32",
            "bound": "mfma",
            "achieved": round(tflops, 2),
            "peak": MFMA_F32_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(tflops / MFMA_F32_PEAK_TFLOPS, 4),
            "traffic": eff_traffic,
            "traffic_source": eff_traffic_src,
            "traffic_over_algorithmic": eff_ratio,
            "algorithmic_bytes_per_step": float(efficientnet.conv_bytes("s", b, 224, 224)),
            "launches_per_step": launches / steps,
            "avg_launch_ms": round(kernel_ms / max(launches, 1), 4),
            "kernel_ms_per_step": round(kernel_ms / steps, 3),
            "algorithmic_flops_per_step": flops,
            "note": "algorithmic FLOPs use the true channel counts, which is also what the kernel runs (24- and "
                    "48-channel stages in its packed-K mode, no padding to 32); depthwise convolutions and the "
                    "squeeze-excitation pooling (not matrix-core work) take the rest of the step",
        },
    }


def bench_pipeline(args: argparse.Namespace, rank: int, world: int, device: torch.device) -> dict:
    """BASELINE.json configs[4]: ViT-B/16 fp16 encode of 512-image batches pipelined into a row-sharded
    50 M x 768 fp16 search, encode and search on two HIP streams.  A step = every rank encodes one batch of 512 and all
    world * 512 embeddings are searched (top-10) against the whole bank.  value = images/s = queries/s, whole job."""
    from imagescry_amd import EmbedSearchPipeline

    n, d, b, k = args.pipeline_rows, args.dim, args.batch, args.k
    lo, hi = shard_bounds(n, world, rank)
    shard = make_shard(lo, hi, d, device)
    group = dist.group.WORLD if world > 1 else None
    bank = EmbeddingBank(shard, dtype=torch.float16, normalize=False, index_base=lo, process_group=group, presharded=True)
    del shard
    torch.cuda.empty_cache()
    model = ViTB16Embedder(seed=0).to(device)
    images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(SEED + rank)).to(device)
    batch = ImageBatch(indices=torch.arange(b, device=device), images=images)
    pipe = EmbedSearchPipeline(embedding_model=model, bank=bank, k=k, overlap=not args.no_overlap)
    pipe.run([batch] * max(args.warmup, 1))
    fence(world)
    t0 = time.perf_counter()
    results = pipe.run([batch] * args.steps)  # one call: batches stream through the two HIP streams back to back
    fence(world)
    seconds = max_over_ranks(time.perf_counter() - t0, world, device)
    assert len(results) == args.steps and results[-1].neighbours.shape == (b, k)
    return {
        "metric": "images/s encoded and searched (ViT-B/16 fp16 -> cosine top-10)",
        "value": round(b * world * args.steps / seconds, 1),
        "unit": "images/s",
        "ms_per_step": round(seconds / args.steps * 1e3, 3),
        "scaling": "weak",
        "dtype": "f16",
        "config": {"workload": f"ViT-B/16 fp16 encode of {b}-image batches per rank pipelined into cosine top-{k} over a "
                               f"{n} x {d} fp16 bank row-sharded {world} way(s); "
                               f"{'two HIP streams' if not args.no_overlap else 'one stream'} (BASELINE config 5)",
                   "bank_rows": n, "dim": d, "batch_per_gpu": b, "k": k, "rows_per_gpu": hi - lo,
                   "parallelism": f"encode replicas{world} + row-shard{world}" + ("+allgather" if world > 1 else "")},
        "roofline": None,
        "_outputs": {"indices": results[-1].indices, "scores": results[-1].scores,
                     "neighbours": results[-1].neighbours},
    }


def cpu_baseline_encode(args: argparse.Namespace) -> dict:
    from oracle import encoder_oracle

    sample = min(128, args.batch)
    sd = resnet50.make_state_dict(seed=0)
    images = torch.randint(0, 256, (sample, 3, 224, 224), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(SEED))
    encoder_oracle.predict_step_embeddings(images[:2], sd)
    reps, t0 = 0, time.perf_counter()
    while reps < 1 or (time.perf_counter() - t0 < 12.0 and reps < 4):
        encoder_oracle.predict_step_embeddings(images, sd)
        reps += 1
    per_pass = (time.perf_counter() - t0) / reps
    return {
        "value": round(sample / per_pass, 2),
        "unit": "images/s",
        "cores": torch.get_num_threads(),
        "kind": "port",
        "sample_fraction": round(sample / args.batch, 4),
        "sample": f"oracle.encoder_oracle.predict_step_embeddings (torch CPU float32), one batch of {sample} images "
                  f"({100.0 * sample / args.batch:.0f} % of the {args.batch}-image step; batch statistics are per sample "
                  f"batch), {reps} passes of {per_pass:.2f} s",
    }


def strip(d: dict) -> dict:
    return {k: v for k, v in d.items() if not k.startswith("_")}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: Path, outputs: dict[str, torch.Tensor]) -> None:
    """`--dump-outputs`: one DIR/<name>.npy per array the timed path returned in its last step, floating point as float32
    and integers as float64.  Above DUMP_LIMIT_BYTES in all, every array keeps a fixed, seeded sample of its rows, and
    DIR/<name>_rows.npy says which."""
    import numpy as np

    arrays = {name: (t.float() if t.is_floating_point() else t.double()).cpu().numpy() for name, t in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        frac = DUMP_LIMIT_BYTES / total / 2  # half the budget: room for the row lists
        for name in list(arrays):
            n = len(arrays[name])
            rows = np.sort(np.random.default_rng(SEED).choice(n, max(1, int(n * frac)), replace=False))
            arrays[name] = arrays[name][rows]
            arrays[f"{name}_rows"] = rows.astype(np.float64)
    out_dir.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(out_dir / f"{name}.npy", a)


def main() -> None:
    args = parse_args()
    rank, world, device = setup_dist(args)
    torch.manual_seed(SEED)
    if args.workload == "search":
        primary = bench_search(args, rank, world, device)
        primary.pop("_bank", None), primary.pop("_queries", None)
        torch.cuda.empty_cache()
        secondary = secondary_vit = secondary_eff = None
        if args.full and not args.no_secondary and rank == 0:
            secondary = bench_encode(args, rank, world, device, steps=6, warmup=2, collective_timing=False, full=True)
            secondary.pop("_model"), secondary.pop("_images")
            torch.cuda.empty_cache()
            secondary_vit = bench_encode_vit(args, device, steps=6, warmup=2)
            torch.cuda.empty_cache()
            secondary_eff = bench_encode_efficientnet(args, device, steps=6, warmup=2)
    elif args.workload == "pipeline":
        primary = bench_pipeline(args, rank, world, device)
        secondary = secondary_vit = secondary_eff = None
    else:
        primary = bench_encode(args, rank, world, device, args.steps, args.warmup, collective_timing=True,
                               full=args.full)
        secondary = secondary_vit = secondary_eff = None
    outputs = primary.pop("_outputs")
    if args.dump_outputs and rank == 0:
        dump_outputs(Path(args.dump_outputs), outputs)
    if world > 1:
        dist.barrier()
    if rank == 0:
        line = {
            "metric": primary["metric"],
            "value": primary["value"],
            "unit": primary["unit"],
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": primary["ms_per_step"],
            "higher_is_better": True,
            "scaling": primary["scaling"],
            "vs_baseline": None,  # the reference publishes no number for this metric
            "dtype": primary["dtype"],
            "data": "synthetic (seeded random unit-norm bank / random uint8 images, random-init weights)",
            "config": primary["config"],
            "roofline": primary["roofline"],
        }
        for key in ("selfcheck", "overflowed_candidate_buffers", "exact_pass_queries", "exhaustive_pass_queries"):
            if key in primary:
                line[key] = primary[key]
        if primary.get("q_sweep"):
            line["q_sweep"] = primary["q_sweep"]
        if primary.get("scaling_projection"):
            line["scaling_projection"] = primary["scaling_projection"]
        if primary.get("bank_variants"):
            line["bank_variants"] = primary["bank_variants"]
        if args.full and world == 1 and not args.no_cpu_baseline:
            if args.workload != "pipeline":
                line["cpu_baseline"] = (cpu_baseline_search(args) if args.workload == "search"
                                        else cpu_baseline_encode(args))
        if secondary is not None:
            enc = strip(secondary)
            if world == 1 and not args.no_cpu_baseline:
                enc["cpu_baseline"] = cpu_baseline_encode(args)
            line["encode"] = enc
        if secondary_vit is not None:
            line["encode_vit_b16"] = secondary_vit
        if secondary_eff is not None:
            line["encode_efficientnet_v2_s"] = secondary_eff
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
