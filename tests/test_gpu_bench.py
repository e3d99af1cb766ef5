"""`bench.py` itself, at small sizes, each run a fresh child process: the plain line carries the headline and nothing
else, `--dump-outputs` writes what the last timed step returned (checked against the oracle / the same embedder in
this process on the same seeded inputs), and `--full` still adds the roofline, the self-check and the sweeps."""

from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("selfcheck", "q_sweep", "cpu_baseline", "encode", "encode_vit_b16", "encode_efficientnet_v2_s")


def _bench(*args: str) -> dict:
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    lines = [line for line in proc.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, proc.stdout[-4000:]
    return json.loads(lines[0])


def test_plain_search_line_and_dumped_answer(tmp_path: Path, device: torch.device) -> None:
    import bench
    from oracle import search_oracle

    n, q, k, steps = 65536, 64, 10, 3
    line = _bench("--steps", str(steps), "--warmup", "1", "--bank-rows", str(n), "--queries", str(q),
                  "--dump-outputs", str(tmp_path))
    assert all(key in line for key in HEADLINE_KEYS) and line["steps"] == steps and line["ms_per_step"] > 0
    assert line["unit"] == "queries/s" and line["dtype"] == "f16" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(q * 1e3 / line["ms_per_step"], rel=5e-3)
    assert not any(key in line for key in FULL_ONLY_KEYS) and line["roofline"] is None
    assert sorted(p.name for p in tmp_path.iterdir()) == ["indices.npy", "scores.npy"]
    scores, indices = np.load(tmp_path / "scores.npy"), np.load(tmp_path / "indices.npy")
    assert scores.dtype == np.float32 and indices.dtype == np.float64 and scores.shape == indices.shape == (q, k)

    rows = bench.make_shard(0, n, line["config"]["dim"], device).cpu()
    queries = torch.randn((q, rows.shape[1]), generator=torch.Generator().manual_seed(bench.SEED)).half()
    exp_s, exp_i = search_oracle.cosine_topk(rows, queries, k)
    assert np.array_equal(indices, exp_i.astype(np.float64))
    assert np.allclose(scores, exp_s, rtol=0, atol=1e-6)


def test_plain_encode_dumped_embeddings(tmp_path: Path, device: torch.device) -> None:
    import bench
    from imagescry_amd import ImageBatch, ResNet50Embedder

    b = 8
    line = _bench("--workload", "encode", "--batch", str(b), "--steps", "2", "--warmup", "1",
                  "--dump-outputs", str(tmp_path))
    assert line["unit"] == "images/s" and line["dtype"] == "f32" and line["steps"] == 2 and line["roofline"] is None
    emb, idx = np.load(tmp_path / "embeddings.npy"), np.load(tmp_path / "indices.npy")
    assert emb.dtype == np.float32 and idx.dtype == np.float64 and emb.shape[0] == b
    assert np.array_equal(idx, np.arange(b, dtype=np.float64))

    images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(bench.SEED))
    model = ResNet50Embedder(seed=0).to(device)
    expect = model.predict_step(ImageBatch(indices=torch.arange(b), images=images).to(device)).embeddings
    assert emb.shape == tuple(expect.shape)
    assert np.allclose(emb, expect.cpu().numpy(), rtol=0, atol=1e-5)


def test_full_search_line_keeps_roofline_selfcheck_and_sweep() -> None:
    line = _bench("--full", "--no-secondary", "--no-cpu-baseline", "--steps", "2", "--warmup", "1",
                  "--bank-rows", "65536")
    assert all(key in line for key in HEADLINE_KEYS) and line["steps"] == 2
    assert line["selfcheck"]["ok"] is True
    assert line["roofline"]["kernel"] == "k_dots_filter<f16>" and line["roofline"]["kernel_ms_per_step"] > 0
    assert [r["queries"] for r in line["q_sweep"]] == [1, 16, 64, 128, 256, 512, 1024]
    assert "cpu_baseline" not in line and "encode" not in line
