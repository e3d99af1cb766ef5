"""The entry points the SigLIP backbones add to the C ABI (isc_attention_f16_probe, isc_vit_assemble_plain,
isc_gemm_f16_act) and the ISC_ACT_GELU_TANH activation the last one admits: declared in include/imagescry_hip.h,
exported by the built library, bound in the ctypes table, and their host-side argument checks.  No device is touched: every call below has to fail its checks
before a launch (a launch here would report ISC_ERR_LAUNCH or ISC_ERR_NO_DEVICE)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_attention_f16_probe", "isc_vit_assemble_plain", "isc_gemm_f16_act")
INVALID, UNSUPPORTED, ALIGNMENT = _lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_ALIGNMENT
FAKE, ODD = 0x10000, 0x10008  # never dereferenced; ODD is 8-byte but not 16-byte aligned


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
    assert _prototype("isc_attention_f16_probe") == [
        "const void* kv", "const void* q", "int B", "int T", "int heads", "int head_dim", "void* out", "int packed",
        "void* stream"]
    assert _prototype("isc_vit_assemble_plain") == [
        "const float* patch_embed", "const float* pos_embed", "int B", "int P", "int D", "float* tokens", "void* stream"]
    assert _prototype("isc_gemm_f16_act") == _prototype("isc_gemm_f16")  # same operands, same order
    # the entries a class-token tower goes through take what they took
    assert _prototype("isc_vit_assemble") == [
        "const float* patch_embed", "const float* cls_token", "const float* pos_embed", "int B", "int T", "int D",
        "float* tokens", "void* stream"]
    assert re.search(r"#define ISC_ACT_GELU_TANH 6\b", HEADER.read_text()) and _lib.ISC_ACT_GELU_TANH == 6
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive: the ABI version stays
    assert re.search(r"#define ISC_ABI_VERSION 4\b", HEADER.read_text())


def test_probe_attention_argument_checks() -> None:
    lib = _lib.load()

    def att(kv=FAKE, q=FAKE, b=2, t=196, heads=12, head_dim=64, out=FAKE, packed=1):
        return lib.isc_attention_f16_probe(kv, q, b, t, heads, head_dim, out, packed, None)

    assert att(kv=None) == INVALID and att(q=None) == INVALID and att(out=None) == INVALID
    assert att(b=0) == INVALID and att(b=-1) == INVALID and att(heads=0) == INVALID
    assert att(t=0) == INVALID and att(t=-1) == INVALID
    for packed in (0, 1):
        assert att(head_dim=32, packed=packed) == UNSUPPORTED and att(head_dim=72, packed=packed) == UNSUPPORTED
        assert att(head_dim=128, packed=packed) == UNSUPPORTED
        for odd in ("kv", "q", "out"):
            assert att(**{odd: ODD}, packed=packed) == ALIGNMENT
            assert att(**{odd: ODD}, t=1, packed=packed) == ALIGNMENT and att(**{odd: ODD}, t=5000, packed=packed) == ALIGNMENT
        assert att(b=1 << 20, t=1 << 11, packed=packed) == UNSUPPORTED  # B * T = 2^31


def test_plain_assemble_argument_checks() -> None:
    lib = _lib.load()

    def asm(pe=FAKE, pos=FAKE, b=3, p=196, d=768, out=FAKE):
        return lib.isc_vit_assemble_plain(pe, pos, b, p, d, out, None)

    for null in ("pe", "pos", "out"):
        assert asm(**{null: None}) == INVALID
    assert asm(b=0) == INVALID and asm(p=0) == INVALID and asm(d=0) == INVALID and asm(p=-3) == INVALID
    assert asm(d=770) == UNSUPPORTED
    for odd in ("pe", "pos", "out"):
        assert asm(**{odd: ODD}) == ALIGNMENT


def test_gelu_tanh_is_accepted_by_the_act_entry_and_by_no_other() -> None:
    """The `act` table of isc_gemm_f16_act, decided before any launch: a misaligned output pointer stands behind every
    accepted combination, so ISC_ERR_ALIGNMENT means "passed the activation checks".  isc_gemm_f16 and
    isc_gemm_f16_scaled answer the code 6 as they always did, ISC_ERR_INVALID_ARG; for the activations isc_gemm_f16 takes
    the two entries answer alike."""
    lib = _lib.load()
    packed = _lib.ISC_GEMM_A_PACKED | _lib.ISC_GEMM_W_PACKED
    tanh = _lib.ISC_ACT_GELU_TANH

    def gemm(act=tanh, dtype=_lib.ISC_F16, flags=packed, n=256, out=ODD, entry="isc_gemm_f16_act"):
        return getattr(lib, entry)(FAKE, 300, 128, FAKE, n, FAKE, None, act, out, dtype, flags, None)

    for dtype in (_lib.ISC_F16, _lib.ISC_F32):
        for flags, n in ((packed, 256), (packed | _lib.ISC_GEMM_TILE_128, 256), (0, 132), (packed, 384)):
            assert gemm(dtype=dtype, flags=flags, n=n) == ALIGNMENT, (dtype, flags, n)
    assert gemm(flags=packed | _lib.ISC_GEMM_OUT_PACKED) == ALIGNMENT
    assert gemm(flags=packed | _lib.ISC_GEMM_TILE_256, n=256, out=FAKE) == UNSUPPORTED  # no activation epilogue there
    assert gemm(entry="isc_gemm_f16") == INVALID and gemm(entry="isc_gemm_f16", out=FAKE, flags=0) == INVALID
    for flags in (packed, 0, packed | _lib.ISC_GEMM_TILE_128):
        assert lib.isc_gemm_f16_scaled(FAKE, 300, 128, FAKE, 256, FAKE, FAKE, None, tanh, ODD, _lib.ISC_F32, flags,
                                       None) == INVALID
    for act in (_lib.ISC_ACT_NONE, _lib.ISC_ACT_GELU, _lib.ISC_ACT_QUICK_GELU):
        for kw in (dict(), dict(dtype=_lib.ISC_F32), dict(flags=packed | _lib.ISC_GEMM_TILE_256, out=FAKE), dict(n=130)):
            assert gemm(act, **kw) == gemm(act, entry="isc_gemm_f16", **kw), (act, kw)
    for other in (_lib.ISC_ACT_RELU, _lib.ISC_ACT_SILU, _lib.ISC_ACT_SIGMOID, 7, 8, -1):
        assert gemm(other) == INVALID and gemm(other, out=FAKE, flags=0) == INVALID
    assert gemm(out=None) == INVALID and gemm(n=0) == INVALID
