"""Cost of the ViT patch-token output (not the contract bench): `predict_step` at batch 512, 224 x 224, depth 12 with
output="patches" against output="cls" (interleaved, same process), isc_vit_tokens_out alone, and isc_attention_f16 at
T = 188 (an 11 x 17 grid: the generic, fully masked form) against T = 197.

    python scripts/quick_vit_tokens_bench.py [--rounds 6] [--steps 10] [--head-only]

`--head-only` launches nothing but isc_vit_tokens_out (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagescry_amd import ImageBatch, ViTB16Embedder, _lib, vit
from imagescry_amd.vit import packed_elems


def arg(name: str, default: int) -> int:
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


dev = torch.device("cuda:0")
lib = _lib.load()
s = _lib.stream_handle(dev)
rounds, steps = arg("--rounds", 6), arg("--steps", 10)
b, d = 512, 768


def timed(fn, n: int) -> float:
    """milliseconds per call, device events around n calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


# ---- the head alone: reads B * 196 * D floats, writes as many
t = 197
tokens = torch.randn(b * t, d, device=dev)
gamma, beta = torch.rand(d, device=dev) + 0.5, torch.randn(d, device=dev)
out = torch.empty(b, d, t - 1, device=dev)
for normalize in (0, 1):
    def head() -> None:
        _lib.check(lib.isc_vit_tokens_out(tokens.data_ptr(), b, t, d, gamma.data_ptr(), beta.data_ptr(), 1e-6, normalize,
                                          1e-12, out.data_ptr(), s), "isc_vit_tokens_out")
    timed(head, 5)
    ms = min(timed(head, 50) for _ in range(3))
    gb = 2 * b * (t - 1) * d * 4 / 1e9
    print(f"isc_vit_tokens_out normalize={normalize}: {ms * 1e3:.1f} us, {gb / ms:.2f} TB/s ({gb:.3f} GB moved)", flush=True)
if "--head-only" in sys.argv:
    sys.exit(0)

# ---- attention: T = 188 against T = 197
for t in (188, 197):
    qkv = (torch.randn(packed_elems(b * t, 3 * d), device=dev) * 0.5).half()
    att = torch.empty(packed_elems(b * t, d), dtype=torch.float16, device=dev)

    def attention() -> None:
        _lib.check(lib.isc_attention_f16(qkv.data_ptr(), b, t, 12, 64, att.data_ptr(), 1, s), "isc_attention_f16")
    timed(attention, 5)
    ms = min(timed(attention, 30) for _ in range(3))
    print(f"isc_attention_f16 B=512 T={t}: {ms * 1e3:.1f} us, {4.0 * t * t * 64 * b * 12 / ms / 1e9:.1f} TFLOP/s", flush=True)
    del qkv, att

# ---- predict_step, patches against cls, interleaved
sd = vit.make_state_dict(vit.VIT_B16, seed=0)
models = {mode: ViTB16Embedder(state_dict=sd, output=mode).to(dev) for mode in ("cls", "patches")}
images = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
batch = ImageBatch(indices=torch.arange(b), images=images).to(dev)
for m in models.values():
    timed(lambda: m.predict_step(batch), 3)
times = {mode: [] for mode in models}
for _ in range(rounds):
    for mode, m in models.items():
        times[mode].append(timed(lambda: m.predict_step(batch), steps))
for mode, ts in times.items():
    print(f"predict_step B=512 224x224 depth 12 output={mode}: median {sorted(ts)[len(ts) // 2]:.3f} ms, "
          f"min {min(ts):.3f}, max {max(ts):.3f} ({rounds} rounds x {steps} steps)", flush=True)
med = {mode: sorted(ts)[len(ts) // 2] for mode, ts in times.items()}
print(f"patches - cls: {med['patches'] - med['cls']:+.3f} ms (median), {min(times['patches']) - min(times['cls']):+.3f} ms (min)")
