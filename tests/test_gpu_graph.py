"""hipGraph capture and replay of the C ABI and of the Python calls built on it (include/imagescry_hip.h: "the functions may
be captured into a hipGraph").

Every capture here is `torch.cuda.graph` of a linear chain of launches on one stream, after one eager warm-up call, with
static input and output tensors allocated before the capture and new inputs `copy_`'d into them between replays.  A graph
replays the same launches with the same pointers and the host-side choices frozen at capture: a missed device-side reset,
a host decision that depends on data, or a hidden synchronisation shows up here.  Each replay must equal an eager call on
the same inputs bit for bit (status words included) and match the oracle."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import capi_search as cs  # noqa: E402
import cases  # noqa: E402

from oracle import search_oracle  # noqa: E402

pytestmark = pytest.mark.gpu


def _capture(fn) -> "torch.cuda.CUDAGraph":
    """One eager warm-up call of `fn` on the current stream, then its capture."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    torch.cuda.synchronize()
    return graph


def _replay(graph) -> None:
    graph.replay()
    torch.cuda.synchronize()


_TIES: dict = {}


def _ties_bank(device: torch.device):
    """test_more_ties_than_the_redo_lists_hold's bank (20 000 copies of one row among 30 000, fp16), a half-density row
    filter of it, and the copied row."""
    if not _TIES:
        g = cases.gen(71)
        rows = torch.nn.functional.normalize(torch.randn(30_000, 64, generator=g), dim=1)
        patch = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
        rows[torch.randperm(30_000, generator=g)[:20_000]] = patch
        eb = cs.bank(rows.half(), device)
        allow = torch.rand(30_000, generator=cases.gen(13)) < 0.5
        _TIES.update(eb=eb, rows=rows.half().float(), allow=allow, rf=eb.row_filter(allow.to(device)), patch=patch)
    return _TIES


def _r1(nq: int) -> torch.Tensor:
    return torch.randn(nq, 64, generator=cases.gen(nq + 1)).half()


def _r2(nq: int, patch: torch.Tensor) -> torch.Tensor:
    """Degenerate queries: every third one hits the 20 000 tied rows (redo, then the exhaustive sweep), one is zero."""
    q = torch.randn(nq, 64, generator=cases.gen(nq + 2))
    q[::3] = patch * 2.0
    if nq > 1:
        q[1] = 0
    return q.half()


_ORACLE: dict = {}


def _oracle(t: dict, q: torch.Tensor, k: int, masked: bool):
    key = (q.numpy().tobytes(), k, masked)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_uncached(t, q, k, masked)
    return _ORACLE[key]


def _oracle_uncached(t: dict, q: torch.Tensor, k: int, masked: bool):
    from oracle import c_oracle

    if not masked:
        return c_oracle.cosine_topk(t["rows"].numpy(), q.float().numpy(), k)
    idx = torch.nonzero(t["allow"]).flatten().numpy()
    s, i = c_oracle.cosine_topk(t["rows"][idx].numpy(), q.float().numpy(), k)
    return s, idx[i]


@pytest.mark.parametrize("entry", ["topk", "topk_masked", "exhaustive", "exhaustive_masked"])
@pytest.mark.parametrize("nq", [1, 100, 300, 1500])
def test_captured_search_replays_equal_eager(entry: str, nq: int, device: torch.device) -> None:
    """isc_cosine_topk[_masked] / isc_cosine_topk_exhaustive[_masked] captured once and replayed with R1 (random
    queries), R2 (queries that drive status[1] > 0 and status[3] > 0) and R1 again, then once more after the captured
    workspace was overwritten with 0xFF."""
    t = _ties_bank(device)
    eb, k = t["eb"], 10
    masked = entry.endswith("masked")
    mask = t["rf"] if masked else None
    ex = entry.startswith("exhaustive")
    q = _r1(nq).to(device)
    s, i, st = cs.zero_topk_out(nq, k, device)
    ws = torch.zeros(cs.topk_ws_bytes(eb, nq, k, exhaustive=ex), dtype=torch.uint8, device=device)

    def call(q_, s_, i_, st_, ws_):
        if ex:
            cs.exhaustive(eb, q_, k, s_, i_, ws_, mask=mask)
        else:
            cs.topk(eb, q_, k, s_, i_, st_, ws_, mask=mask)

    graph = _capture(lambda: call(q, s, i, st, ws))
    r1, r2 = _r1(nq), _r2(nq, t["patch"])
    answers = []
    for name, inp in (("R1", r1), ("R2", r2), ("R1 again", r1), ("R1 after 0xFF", r1)):
        if name == "R1 after 0xFF":
            ws.fill_(255)
        s.fill_(float("nan"))
        i.fill_(-7)
        st.fill_(-1)
        q.copy_(inp.to(device))
        _replay(graph)
        es, ei, est = cs.zero_topk_out(nq, k, device)
        call(inp.to(device), es, ei, est, torch.zeros_like(ws))
        torch.cuda.synchronize()
        cs.assert_bits_equal(s, es, f"{entry} Q={nq} {name} scores")
        cs.assert_bits_equal(i, ei, f"{entry} Q={nq} {name} indices")
        if not ex:
            cs.assert_topk_status_equal(st, est, f"{entry} Q={nq} {name}")
            if name == "R2":  # the degenerate replay took the second pass and the exhaustive sweep
                got = st.cpu().tolist()
                assert got[1] > 0 and got[3] > 0, got
        exp_s, exp_i = _oracle(t, inp, k, masked)
        np.testing.assert_array_equal(i.cpu().numpy(), exp_i, err_msg=name)
        np.testing.assert_allclose(s.cpu().numpy(), exp_s, rtol=0, atol=1e-6, err_msg=name)
        answers.append((s.clone(), i.clone(), st.clone()))
    for a, b in ((answers[0], answers[2]), (answers[0], answers[3])):
        cs.assert_bits_equal(a[0], b[0], "R1 replays")
        cs.assert_bits_equal(a[1], b[1], "R1 replays")
        if not ex:
            cs.assert_topk_status_equal(a[2], b[2], "R1 replays")


def test_captured_topk_merge_replays_equal_eager(device: torch.device) -> None:
    """isc_topk_merge of three partial lists captured, replayed with two different inputs (ties and NaN included)."""
    g, nq, kin, kout = 3, 50, 12, 20

    def parts(seed: int):
        gen = cases.gen(seed)
        sc = torch.randn(g, nq, kin, generator=gen).round(decimals=1)  # many exact ties
        sc[0, 3, :4] = float("nan")
        sc = sc.sort(dim=2, descending=True).values
        ix = torch.randint(0, 1000, (g, nq, kin), generator=gen)
        return sc, ix

    ps, pi = (x.to(device) for x in parts(1))
    os_ = torch.zeros(nq, kout, device=device)
    oi = torch.zeros(nq, kout, dtype=torch.int64, device=device)
    graph = _capture(lambda: cs.topk_merge(ps, pi, kout, os_, oi))
    for seed in (2, 3):
        sc, ix = parts(seed)
        ps.copy_(sc.to(device))
        pi.copy_(ix.to(device))
        os_.fill_(-1.0)
        oi.fill_(-1)
        _replay(graph)
        es = torch.zeros_like(os_)
        ei = torch.zeros_like(oi)
        cs.topk_merge(ps, pi, kout, es, ei)
        torch.cuda.synchronize()
        cs.assert_bits_equal(os_, es)
        cs.assert_bits_equal(oi, ei)
        exp_s, exp_i = search_oracle.topk_merge(sc.numpy(), ix.numpy(), kout)
        np.testing.assert_array_equal(oi.cpu().numpy(), exp_i)
        np.testing.assert_array_equal(os_.cpu().numpy(), exp_s)


def _range_oracle(rows: torch.Tensor, q: torch.Tensor, thr: torch.Tensor, allow: np.ndarray):
    s = search_oracle.exact_scores(rows, q.float())
    offs, sc, ix = [0], [], []
    t = thr.cpu().numpy()
    for qi in range(s.shape[0]):
        sel = np.nonzero((s[qi] >= t[qi]) & allow)[0]
        order = np.lexsort((sel, -s[qi, sel].astype(np.float64)))
        sc.append(s[qi, sel[order]])
        ix.append(sel[order].astype(np.int64))
        offs.append(offs[-1] + sel.size)
    return np.array(offs, np.int64), np.concatenate(sc).astype(np.float32), np.concatenate(ix)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nq", [64, 300, 3000])
def test_captured_range_replays_equal_eager(nq: int, masked: bool, device: torch.device) -> None:
    """isc_cosine_range[_masked] captured with a fixed capacity, replayed with three device thresholds: one whose result
    fits, one whose result does not (needed equals the eager needed, offsets all 0), one that fits again.  3000 queries
    are more segments than the point where rocPRIM's segmented sort would partition them by size and read the counts
    back to the host: the range call must stay capturable there too."""
    rows = torch.nn.functional.normalize(torch.randn(3000, 96, generator=cases.gen(41)), dim=1).half()
    eb = cs.bank(rows, device)
    allow = torch.rand(3000, generator=cases.gen(43)) < 0.5
    mask = eb.row_filter(allow.to(device)) if masked else None
    q_host = torch.randn(nq, 96, generator=cases.gen(nq)).half()
    q = q_host.to(device)
    s10 = eb.search(q, 10)[0]
    fits = [s10[:, -1].contiguous(), s10[:, 4].contiguous()]  # 10 and 5 rows per query (fewer when masked)
    over = torch.full((nq,), -2.0, device=device)  # every row of every query
    capacity = nq * 16
    thr = fits[0].clone()
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=device)
    scores = torch.zeros(capacity, device=device)
    indices = torch.zeros(capacity, dtype=torch.int64, device=device)
    needed = torch.zeros(1, dtype=torch.int64, device=device)
    status = torch.zeros(4, dtype=torch.int32, device=device)
    ws = torch.zeros(cs.range_ws_bytes(eb, nq, capacity), dtype=torch.uint8, device=device)
    graph = _capture(lambda: cs.cosine_range(eb, q, thr, capacity, offsets, scores, indices, needed, status, ws, mask=mask))
    allow_np = allow.numpy() if masked else np.ones(3000, bool)
    for name, t in (("fits", fits[0]), ("overflows", over), ("fits again", fits[1])):
        thr.copy_(t)
        offsets.fill_(-1)
        needed.fill_(-1)
        status.fill_(-1)
        _replay(graph)
        ref = (torch.zeros_like(offsets), torch.zeros_like(scores), torch.zeros_like(indices), torch.zeros_like(needed),
               torch.zeros_like(status))
        cs.cosine_range(eb, q, t, capacity, *ref, torch.zeros_like(ws), mask=mask)
        torch.cuda.synchronize()
        cs.assert_bits_equal(needed, ref[3], name)
        cs.assert_bits_equal(offsets, ref[0], name)
        if name == "overflows":
            assert int(needed) == nq * int(allow_np.sum()) > capacity
            assert not bool(offsets.any())
            continue
        cs.assert_bits_equal(status, ref[4], name)
        total = int(offsets[-1])
        cs.assert_bits_equal(scores[:total], ref[1][:total], name)
        cs.assert_bits_equal(indices[:total], ref[2][:total], name)
        exp = _range_oracle(rows, q_host, t, allow_np)
        np.testing.assert_array_equal(offsets.cpu().numpy(), exp[0])
        np.testing.assert_array_equal(indices[:total].cpu().numpy(), exp[2])
        np.testing.assert_array_equal(scores[:total].cpu().numpy(), exp[1])


@pytest.mark.parametrize("masked", [False, True])
def test_captured_bank_search_replays_equal_eager(masked: bool, device: torch.device) -> None:
    """EmbeddingBank.search (one GPU), plain and with a prebuilt RowFilter, captured and replayed."""
    t = _ties_bank(device)
    eb = t["eb"]
    mask = t["rf"] if masked else None
    q = _r1(64).to(device)
    out = {}

    def run():
        out["r"] = eb.search(q, 10, mask=mask)

    graph = _capture(run)
    for inp in (_r2(64, t["patch"]), _r1(64)):
        q.copy_(inp.to(device))
        _replay(graph)
        es, ei = eb.search(inp.to(device), 10, mask=mask)
        torch.cuda.synchronize()
        cs.assert_bits_equal(out["r"][0], es)
        cs.assert_bits_equal(out["r"][1], ei)
        exp_s, exp_i = _oracle(t, inp, 10, masked)
        np.testing.assert_array_equal(ei.cpu().numpy(), exp_i)


def test_captured_search_keeps_its_workspace_alive(device: torch.device) -> None:
    """A captured search holds the raw pointer of its workspace.  After eager searches at five other (bucket, k) keys
    -- more than the bank's workspace cache keeps -- the bank must still reference that workspace (checked on the host
    first, so that a bank that dropped it fails here instead of replaying over freed memory); tensors allocated
    afterwards of the same size must not be written by a replay."""
    t = _ties_bank(device)
    eb = t["eb"]
    q = _r1(64).to(device)
    out = {}

    def run():
        out["r"] = eb.search(q, 10)

    graph = _capture(run)
    ws_ptr = eb._workspace(64, 10).data_ptr()
    ws_bytes = cs.topk_ws_bytes(eb, 64, 10)
    for nq, k in ((1, 3), (100, 5), (300, 7), (1500, 9), (200, 11)):
        eb.search(_r1(nq).to(device), k)
    torch.cuda.synchronize()
    held = [w.data_ptr() for lane in eb._workspaces.values() for w in lane.values()]
    held += [w.data_ptr() for w in eb._captured_workspaces]
    assert ws_ptr in held
    fillers = [torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=device) for _ in range(3)]
    q.copy_(_r2(64, t["patch"]).to(device))
    _replay(graph)
    es, ei = eb.search(q, 10)
    torch.cuda.synchronize()
    cs.assert_bits_equal(out["r"][0], es)
    cs.assert_bits_equal(out["r"][1], ei)
    for f in fillers:
        assert bool((f == 0x5A).all())


def _assert_encoder_replays(model, images: list[torch.Tensor], device: torch.device) -> None:
    from imagescry_amd import ImageBatch

    idx = torch.arange(images[0].shape[0], device=device)
    static = images[0].to(device).clone()
    out = {}

    def run():
        out["e"] = model.predict_step(ImageBatch(indices=idx, images=static)).embeddings

    graph = _capture(run)
    for img in images[1:]:
        static.copy_(img.to(device))
        _replay(graph)
        eager = model.predict_step(ImageBatch(indices=idx, images=img.to(device))).embeddings
        torch.cuda.synchronize()
        assert out["e"].shape == eager.shape
        assert torch.equal(out["e"], eager)


@pytest.mark.parametrize("name", ["resnet50", "resnet50_resize", "efficientnet_s"])
def test_captured_cnn_predict_step_equals_eager(name: str, device: torch.device) -> None:
    """predict_step of the convolutional embedders (preprocess with batch statistics, the fused stem input, the
    encoder, the normalised tail) captured and replayed with two batches: bit-identical to eager.  `resnet50_resize`
    caps the long side at 80, so the (64, 96) batches take the resize branch."""
    from imagescry_amd import EfficientNetEmbedder, ResNet50Embedder

    if name == "efficientnet_s":
        model = EfficientNetEmbedder(backbone_size="s", seed=1)
    else:
        model = ResNet50Embedder(seed=1, max_side_length=80 if name == "resnet50_resize" else 640)
    model = model.to(device)
    imgs = [cases.images_u8((2, 3, 64, 96), seed=s) for s in (1, 2, 3)]
    _assert_encoder_replays(model, imgs, device)


def test_captured_vit_predict_step_equals_eager(device: torch.device) -> None:
    from imagescry_amd import ViTB16Embedder, vit

    model = ViTB16Embedder(config=vit.ViTConfig(depth=2), seed=1).to(device)
    imgs = [cases.images_u8((2, 3, 224, 224), seed=s) for s in (4, 5, 6)]
    _assert_encoder_replays(model, imgs, device)


def test_captured_pca_pipeline_predict_step_equals_eager(device: torch.device) -> None:
    """EmbeddingPCAPipeline.predict_step (the encoder, then isc_linear_centered) captured and replayed."""
    from imagescry_amd import EmbeddingPCAPipeline, ImageBatch, PCA, ResNet50Embedder

    model = ResNet50Embedder(seed=2).to(device)
    fit = model.predict_step(ImageBatch(indices=torch.arange(24), images=cases.images_u8((24, 3, 64, 64), seed=31)).to(device))
    pca = PCA(max_num_components=8, min_explained_variance=1.0).fit(fit.get_flat_vectors())
    pipe = EmbeddingPCAPipeline(embedding_model=model, pca=pca)
    imgs = [cases.images_u8((3, 3, 64, 64), seed=s) for s in (32, 33, 34)]
    idx = torch.tensor([4, 2, 9], device=device)
    static = imgs[0].to(device).clone()
    out = {}

    def run():
        out["e"] = pipe.predict_step(ImageBatch(indices=idx, images=static)).embeddings

    graph = _capture(run)
    for img in imgs[1:]:
        static.copy_(img.to(device))
        _replay(graph)
        eager = pipe.predict_step(ImageBatch(indices=idx, images=img.to(device))).embeddings
        torch.cuda.synchronize()
        assert out["e"].shape == eager.shape == (3, 8, 1, 1)
        assert torch.equal(out["e"], eager)
