"""Timing of isc_attention_f16_stream (not the contract bench), the numbers of DESIGN.md 4.6:

  * the kernel at B * heads = 96 * 12 and T in {197, 224, 577, 785, 1025}, row-major operands;
  * against isc_attention_f16 where that one applies (T <= 224);
  * against what a user could write in torch on the same tensors -- two matmuls and a softmax in fp16 -- and, as
    information, against torch.nn.functional.scaled_dot_product_attention;
  * ViTB16Embedder (ViT-B/16, output="patches") images per second at 14 x 14, 20 x 20, 28 x 28 and 32 x 32 patches.

Device events, warm-up, the routes of one shape interleaved, median of --samples (20) samples of --reps calls each.

    python scripts/quick_attention_stream_bench.py [--samples 20] [--reps 3] [--no-model]
"""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import ImageBatch, ViTB16Embedder, _lib, vit


def arg(name: str, default: int) -> int:
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


dev = torch.device("cuda:0")
lib = _lib.load()
s = _lib.stream_handle(dev)
samples, reps = arg("--samples", 20), arg("--reps", 3)
b, heads, hd = 96, 12, 64
d = heads * hd


def timed(fn, n: int) -> float:
    """milliseconds per call, device events around n calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def medians(routes: dict) -> dict:
    for fn in routes.values():
        timed(fn, 2)
    ts = {name: [] for name in routes}
    for _ in range(samples):
        for name, fn in routes.items():
            ts[name].append(timed(fn, reps))
    return {name: sorted(v)[len(v) // 2] for name, v in ts.items()}


for t in (197, 224, 577, 785, 1025):
    qkv = (torch.randn(b, t, 3 * d, device=dev, generator=torch.Generator(device=dev).manual_seed(t)) * 0.5).half()
    out = torch.empty(b, t, d, dtype=torch.float16, device=dev)
    q, k, v = (z.view(b, t, heads, hd).transpose(1, 2) for z in qkv.split(d, dim=-1))

    def stream() -> None:
        _lib.check(lib.isc_attention_f16_stream(qkv.data_ptr(), b, t, heads, hd, out.data_ptr(), 0, s), "stream")

    def one_shot() -> None:
        _lib.check(lib.isc_attention_f16(qkv.data_ptr(), b, t, heads, hd, out.data_ptr(), 0, s), "one-shot")

    def plain() -> torch.Tensor:
        p = torch.softmax(torch.matmul(q * 0.125, k.transpose(-1, -2)), dim=-1)
        return torch.matmul(p, v).transpose(1, 2).reshape(b, t, d)

    def sdpa() -> torch.Tensor:
        return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, t, d)

    stream()
    torch.cuda.synchronize()
    err = (out.float() - plain().float()).abs().max().item()
    routes = {"stream": stream, "torch": plain, "sdpa": sdpa}
    if t <= 224:
        routes["one-shot"] = one_shot
    ms = medians(routes)
    fl = 4.0 * t * t * hd * b * heads
    line = ", ".join(f"{name} {v * 1e3:.1f} us ({fl / v / 1e9:.0f} TFLOP/s)" for name, v in ms.items())
    ratios = ", ".join(f"{name} / stream {ms[name] / ms['stream']:.2f}" for name in ms if name != "stream")
    print(f"T={t} B*heads={b * heads}: {line}; {ratios}; max|stream - torch| {err:.2e}", flush=True)
    del qkv, out, q, k, v

if "--no-model" not in sys.argv:
    sd = vit.make_state_dict(vit.VIT_B16, seed=0)
    nb = 64
    for n in (14, 20, 28, 32):
        kw = {} if n == 14 else {"max_patches": n * n}
        model = ViTB16Embedder(state_dict=sd, output="patches", grid="aspect", **kw).to(dev)
        images = torch.randint(0, 256, (nb, 3, 16 * n, 16 * n), dtype=torch.uint8, generator=torch.Generator().manual_seed(n))
        batch = ImageBatch(indices=torch.arange(nb), images=images).to(dev)
        shape = tuple(model.predict_step(batch).embeddings.shape)
        ms = medians({"predict_step": lambda: model.predict_step(batch)})["predict_step"]
        print(f"ViT-B/16 patches {n}x{n} ({n * n + 1} tokens), batch {nb}: {ms:.2f} ms, {nb / ms * 1e3:.0f} images/s, "
              f"map {shape}", flush=True)
        del model, batch
