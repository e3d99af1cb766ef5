"""The entry points the CLIP backbones add to the C ABI (isc_attention_f16_causal, isc_text_embed,
isc_text_pool_layernorm) and the ISC_ACT_QUICK_GELU activation of isc_gemm_f16: declared in include/imagescry_hip.h,
exported by the built library, bound in the ctypes table, and their host-side argument checks.  No device is touched:
every call below has to fail its checks before a launch (a launch here would report ISC_ERR_LAUNCH or
ISC_ERR_NO_DEVICE)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_attention_f16_causal", "isc_text_embed", "isc_text_pool_layernorm")
INVALID, UNSUPPORTED, ALIGNMENT = _lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_ALIGNMENT
FAKE, ODD, ODD4 = 0x10000, 0x10008, 0x10004  # never dereferenced; ODD is 8-byte but not 16-byte aligned, ODD4 4-byte


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(_prototype(name))
    assert _prototype("isc_attention_f16_causal") == _prototype("isc_attention_f16")  # same operands, same order
    assert _prototype("isc_text_embed") == [
        "const int64_t* ids", "int B", "int T", "int vocab", "int D", "const float* table", "const float* pos",
        "float* tokens", "int32_t* bad_count", "void* stream"]
    assert _prototype("isc_text_pool_layernorm") == [
        "const float* tokens", "const int64_t* ids", "int B", "int T", "int D", "int64_t eos_id", "const float* gamma",
        "const float* beta", "float eps", "void* out", "int out_dtype", "int out_packed", "void* stream"]
    assert re.search(r"#define ISC_ACT_QUICK_GELU 5\b", HEADER.read_text()) and _lib.ISC_ACT_QUICK_GELU == 5
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive: the ABI version stays


def test_causal_attention_argument_checks() -> None:
    lib = _lib.load()

    def att(qkv=FAKE, b=2, t=77, heads=8, head_dim=64, out=FAKE, packed=1):
        return lib.isc_attention_f16_causal(qkv, b, t, heads, head_dim, out, packed, None)

    assert att(qkv=None) == INVALID and att(out=None) == INVALID
    assert att(b=0) == INVALID and att(heads=0) == INVALID
    assert att(t=0) == INVALID and att(t=-1) == INVALID
    for packed in (0, 1):
        assert att(t=129, packed=packed) == UNSUPPORTED  # a head's keys are held whole up to 128
        assert att(t=225, packed=packed) == UNSUPPORTED
        assert att(head_dim=32, packed=packed) == UNSUPPORTED and att(head_dim=128, packed=packed) == UNSUPPORTED
        assert att(qkv=ODD, packed=packed) == ALIGNMENT and att(out=ODD, packed=packed) == ALIGNMENT
        assert att(t=128, out=ODD, packed=packed) == ALIGNMENT and att(t=1, qkv=ODD, packed=packed) == ALIGNMENT


def test_text_embed_argument_checks() -> None:
    lib = _lib.load()

    def embed(ids=FAKE, b=3, t=77, vocab=1000, d=512, table=FAKE, pos=FAKE, out=FAKE, bad=FAKE):
        return lib.isc_text_embed(ids, b, t, vocab, d, table, pos, out, bad, None)

    for null in ("ids", "table", "pos", "out"):  # the counter is optional, nothing else is
        assert embed(**{null: None}) == INVALID
        assert embed(**{null: None}, bad=None) == INVALID
    assert embed(b=0) == INVALID and embed(t=0) == INVALID and embed(vocab=0) == INVALID and embed(d=0) == INVALID
    assert embed(d=6) == UNSUPPORTED and embed(d=6, bad=None) == UNSUPPORTED
    for odd in ("table", "pos", "out"):
        assert embed(**{odd: ODD}) == ALIGNMENT
    assert embed(ids=ODD4) == ALIGNMENT and embed(ids=ODD, out=ODD) == ALIGNMENT  # int64 ids: 8 bytes


def test_text_pool_layernorm_argument_checks() -> None:
    lib = _lib.load()

    def pool(tokens=FAKE, ids=FAKE, b=3, t=77, d=512, eos=49407, gamma=FAKE, beta=FAKE, eps=1e-5, out=FAKE,
             dtype=_lib.ISC_F16, packed=1):
        return lib.isc_text_pool_layernorm(tokens, ids, b, t, d, eos, gamma, beta, eps, out, dtype, packed, None)

    for null in ("tokens", "ids", "gamma", "beta", "out"):
        assert pool(**{null: None}) == INVALID
    assert pool(b=0) == INVALID and pool(t=0) == INVALID and pool(d=0) == INVALID and pool(eps=-1.0) == INVALID
    assert pool(dtype=_lib.ISC_U8) == INVALID and pool(dtype=9) == INVALID
    # the limits of isc_layernorm
    assert pool(d=6) == UNSUPPORTED and pool(d=2052) == UNSUPPORTED
    assert pool(d=132) == UNSUPPORTED  # packed output needs whole K steps of 64 ...
    assert pool(dtype=_lib.ISC_F32) == UNSUPPORTED  # ... and fp16
    for odd in ("tokens", "gamma", "beta", "out"):
        assert pool(**{odd: ODD}) == ALIGNMENT
        assert pool(**{odd: ODD}, dtype=_lib.ISC_F32, packed=0, eos=-1) == ALIGNMENT
    assert pool(ids=ODD4) == ALIGNMENT


def test_quick_gelu_is_accepted_where_gelu_is() -> None:
    """The `act` table of both GEMM entries, decided before any launch: a misaligned output pointer stands behind every
    accepted combination, so ISC_ERR_ALIGNMENT means "passed the activation checks"."""
    lib = _lib.load()
    packed = _lib.ISC_GEMM_A_PACKED | _lib.ISC_GEMM_W_PACKED
    none, gelu, quick = _lib.ISC_ACT_NONE, _lib.ISC_ACT_GELU, _lib.ISC_ACT_QUICK_GELU

    def gemm(act, dtype=_lib.ISC_F16, flags=packed, n=256, out=ODD):
        return lib.isc_gemm_f16(FAKE, 300, 128, FAKE, n, FAKE, None, act, out, dtype, flags, None)

    def scaled(act, dtype=_lib.ISC_F32, flags=packed, n=256):
        return lib.isc_gemm_f16_scaled(FAKE, 300, 128, FAKE, n, FAKE, FAKE, None, act, ODD, dtype, flags, None)

    for act in (gelu, quick):
        for dtype in (_lib.ISC_F16, _lib.ISC_F32):
            for flags, n in ((packed, 256), (packed | _lib.ISC_GEMM_TILE_128, 256), (0, 132), (packed, 384)):
                assert gemm(act, dtype, flags, n) == ALIGNMENT, (act, dtype, flags, n)
        assert gemm(act, flags=packed | _lib.ISC_GEMM_OUT_PACKED) == ALIGNMENT
        assert gemm(act, flags=packed | _lib.ISC_GEMM_TILE_256, n=256, out=FAKE) == UNSUPPORTED  # no activation epilogue there
        assert gemm(act, flags=_lib.ISC_GEMM_TILE_256, out=FAKE) == UNSUPPORTED
        for flags in (packed, 0, packed | _lib.ISC_GEMM_TILE_128):
            assert scaled(act, flags=flags) == UNSUPPORTED  # LayerScale has no activation
    assert gemm(none) == ALIGNMENT and scaled(none) == ALIGNMENT
    for act in (_lib.ISC_ACT_RELU, _lib.ISC_ACT_SILU, _lib.ISC_ACT_SIGMOID, 6, 7, -1):
        assert gemm(act) == INVALID and gemm(act, out=FAKE, flags=0) == INVALID, act
        assert scaled(act) == INVALID, act
