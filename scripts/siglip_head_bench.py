"""Timing of the SigLIP pooling head at ViT-B/16, 224 pixels (not the contract bench; see bench.py): the one-query
attention kernel against one read of its kv operand, the head's share of the image tower, and fc1 with the tanh GELU
epilogue against fc1 with the erf one.  `python scripts/siglip_head_bench.py [B]` (B = 256 by default) on a HIP device."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import SigLIPEmbedder, _lib, siglip, vit  # noqa: E402

dev = torch.device("cuda:0")
b = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cfg = siglip.PRESETS["ViT-B/16"]
cfg = siglip.SigLIPConfig(cfg.vision, siglip.SigLIPTextConfig(depth=1, vocab=1000))  # the text tower is not timed
v = cfg.vision
t, d, heads = v.tokens, v.dim, v.heads
model = SigLIPEmbedder(cfg, seed=0, max_images_per_pass=b).to(dev)
net = model._net
lib = _lib.load()
stream = _lib.stream_handle(dev)
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: the specification and a measured float4 copy (MI355X)


def median_ms(kernel_id: int, launch, buffers: int, reps: int = 40) -> float:
    """Median device time of `launch(i % buffers)`, one timing read per launch, after a warm-up of every buffer."""
    for i in range(buffers):
        launch(i)
    torch.cuda.synchronize()
    _lib.timing_enable(True)
    _lib.timing_read(kernel_id)
    times = []
    for i in range(reps):
        launch(i % buffers)
        times.append(_lib.timing_read(kernel_id)[0])
    _lib.timing_enable(False)
    return statistics.median(times)


# ---- 1. isc_attention_f16_probe against one read of kv.  Four kv operands in rotation: more bytes than the 256 MiB
# Infinity Cache holds, so every launch reads HBM.
kv_bytes = b * t * 2 * d * 2
kvs = [torch.randn(vit.packed_elems(b * t, 2 * d), device=dev).half() for _ in range(max(2, -(-(640 << 20) // kv_bytes)))]
att = torch.empty(vit.packed_elems(b, d), dtype=torch.float16, device=dev)


def probe(i: int) -> None:
    _lib.check(lib.isc_attention_f16_probe(kvs[i].data_ptr(), net.probe_q.data_ptr(), b, t, heads, 64, att.data_ptr(), 1,
                                           stream), "isc_attention_f16_probe")


ms = median_ms(_lib.ISC_KERNEL_ATTENTION_PROBE, probe, len(kvs))
print(f"probe attention B={b} T={t} heads={heads}: {ms * 1e3:.1f} us for {kv_bytes / 1e6:.1f} MB of kv = "
      f"{kv_bytes / (ms * 1e-3) / 1e12:.2f} TB/s; floor {kv_bytes / HBM_PEAK * 1e6:.1f} us at {HBM_PEAK / 1e12:.1f} TB/s "
      f"(share {kv_bytes / HBM_PEAK / (ms * 1e-3):.2f}), {kv_bytes / HBM_COPY * 1e6:.1f} us at the measured copy rate "
      f"(share {kv_bytes / HBM_COPY / (ms * 1e-3):.2f})")
del kvs

# ---- 2. the head's share of the image tower: the encoder alone and the encoder + head, alternating, device events
x = torch.randn(b, 3, v.image_size, v.image_size, device=dev)


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


grid = (v.grid, v.grid)
for _ in range(2):
    vit._encode(net.encoder, x, grid)
    siglip.forward_image(net, x)
enc, full = [], []
for _ in range(7):
    enc.append(timed(lambda: vit._encode(net.encoder, x, grid)))
    full.append(timed(lambda: siglip.forward_image(net, x)))
e, f = statistics.median(enc), statistics.median(full)
print(f"image tower B={b}: encoder {e:.2f} ms, encoder + pooling head {f:.2f} ms: the head (LayerNorm, kv GEMM, probe, "
      f"out_proj, MLP) takes {f - e:.2f} ms = {100 * (f - e) / f:.1f} % of the tower (spread of the encoder over 7 runs: "
      f"{min(enc):.2f} .. {max(enc):.2f} ms)")

# ---- 3. fc1 with the tanh and with the erf epilogue, same operands, alternating
m = b * t
a = torch.randn(vit.packed_elems(m, d), device=dev).half() * 0.5
out = torch.empty(vit.packed_elems(m, v.mlp_dim), dtype=torch.float16, device=dev)
fc1 = net.encoder.blocks[0].fc1
acts = (_lib.ISC_ACT_GELU_TANH, _lib.ISC_ACT_GELU)
per = {}
for name, act in (("tanh", acts[0]), ("erf", acts[1]), ("tanh again", acts[0]), ("erf again", acts[1])):
    per[name] = median_ms(_lib.ISC_KERNEL_GEMM_F16, lambda i: vit._gemm(a, m, fc1, out, act=act, stream=stream), 1, reps=20)
flops = 2.0 * m * d * v.mlp_dim
print(f"fc1 {m} x {d} x {v.mlp_dim}, fp16 packed out: " + ", ".join(
    f"{k} {ms_ * 1e3:.0f} us ({flops / (ms_ * 1e-3) / 1e12:.0f} TFLOP/s)" for k, ms_ in per.items()))
