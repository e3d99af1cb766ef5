"""Cost of the CLIP backbones (not the contract bench):

* the causal attention kernel -- isc_attention_f16_causal against the bidirectional isc_attention_f16 on the same packed
  operands (1024 sequences x 8 heads, T = 77: the ViT-B text tower's layer), alternated in one process;
* `encode_text` of the ViT-B/16 text tower at Q = 1024, T = 77, in texts / s;
* `predict_step` at batch 256, 224 x 224, of the ViT-B/32, ViT-B/16 and ViT-L/14 vision towers, interleaved, in images / s.

    python scripts/quick_clip_bench.py [--rounds 5] [--steps 3] [--attention-only | --models-only]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import CLIPEmbedder, ImageBatch, _lib
from imagescry_amd.vit import packed_elems


def arg(name: str, default: int) -> int:
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


dev = torch.device("cuda:0")
lib = _lib.load()
s = _lib.stream_handle(dev)
rounds, steps = arg("--rounds", 5), arg("--steps", 3)


def timed(fn, n: int) -> float:
    """milliseconds per call, device events around n calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def median(ts: list[float]) -> float:
    return sorted(ts)[len(ts) // 2]


if "--models-only" not in sys.argv:
    b, t, heads = 1024, 77, 8
    d = heads * 64
    qkv = (torch.randn(packed_elems(b * t, 3 * d), device=dev) * 0.5).half()
    out = torch.empty(packed_elems(b * t, d), dtype=torch.float16, device=dev)
    fns = {name: (lambda f=getattr(lib, name), name=name: _lib.check(
        f(qkv.data_ptr(), b, t, heads, 64, out.data_ptr(), 1, s), name))
        for name in ("isc_attention_f16", "isc_attention_f16_causal")}
    for fn in fns.values():
        timed(fn, 5)
    times = {key: [] for key in fns}
    for _ in range(max(rounds, 9)):  # alternated
        for key, fn in fns.items():
            times[key].append(timed(fn, 20))
    for key, ts in times.items():
        print(f"attention B={b} heads={heads} T={t} packed {key}: median {median(ts) * 1e3:.1f} us, min {min(ts) * 1e3:.1f}, "
              f"max {max(ts) * 1e3:.1f}", flush=True)
    ratio = median(times["isc_attention_f16_causal"]) / median(times["isc_attention_f16"])
    print(f"attention causal / bidirectional: {ratio:.3f} of the time", flush=True)
    if "--attention-only" in sys.argv:
        sys.exit(0)

q, t = 1024, 77
text_model = CLIPEmbedder("ViT-B/16").to(dev)
vocab = text_model.clip_config.text.vocab
g = torch.Generator().manual_seed(0)
ids = torch.randint(1, vocab - 1, (q, t), generator=g)
ids[torch.arange(q), torch.randint(1, t, (q,), generator=g)] = vocab - 1
ids = ids.to(dev)
timed(lambda: text_model.encode_text(ids), 2)
ts = [timed(lambda: text_model.encode_text(ids), steps) for _ in range(rounds)]
print(f"encode_text ViT-B/16 text tower Q={q} T={t}: median {median(ts):.2f} ms, min {min(ts):.2f}, max {max(ts):.2f} "
      f"-> {q / median(ts) * 1e3:.0f} texts/s ({rounds} rounds x {steps} steps, one host read a call)", flush=True)
ts = [timed(lambda: text_model.encode_text(ids, validate=False), steps) for _ in range(rounds)]
print(f"encode_text ... validate=False: median {median(ts):.2f} ms -> {q / median(ts) * 1e3:.0f} texts/s", flush=True)

b = 256
images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
batch = ImageBatch(indices=torch.arange(b), images=images).to(dev)
models = {"ViT-B/16": text_model, "ViT-B/32": CLIPEmbedder("ViT-B/32").to(dev), "ViT-L/14": CLIPEmbedder("ViT-L/14").to(dev)}
for model in models.values():
    timed(lambda: model.predict_step(batch), 2)
times = {key: [] for key in models}
for _ in range(rounds):
    for key, model in models.items():
        times[key].append(timed(lambda: model.predict_step(batch), steps))
for key, ts in times.items():
    print(f"predict_step B={b} 224x224 CLIPEmbedder {key}: median {median(ts):.2f} ms, min {min(ts):.2f}, max {max(ts):.2f} "
          f"-> {b / median(ts) * 1e3:.0f} img/s ({rounds} rounds x {steps} steps)", flush=True)
