"""The entry points the DINOv2 backbones add to the C ABI (isc_gemm_f16_scaled, isc_patchify_f16_padded,
isc_vit_assemble_reg, isc_vit_tokens_out_skip, isc_vit_pos_resample_aa): declared in include/imagescry_hip.h, exported
by the built library, bound in the ctypes table, and their host-side argument checks.  No device is touched: every call
below has to fail its checks before a launch (a launch here would report ISC_ERR_LAUNCH or ISC_ERR_NO_DEVICE)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_gemm_f16_scaled", "isc_patchify_f16_padded", "isc_vit_assemble_reg", "isc_vit_tokens_out_skip",
         "isc_vit_pos_resample_aa")
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
    gemm = _prototype("isc_gemm_f16")  # the scaled GEMM is isc_gemm_f16 with `scale` in front of `residual`
    assert _prototype("isc_gemm_f16_scaled") == gemm[:6] + ["const float* scale"] + gemm[6:]
    patchify = _prototype("isc_patchify_f16")
    assert _prototype("isc_patchify_f16_padded") == patchify[:6] + ["int kpad"] + patchify[6:]
    assert _prototype("isc_vit_assemble_reg") == [
        "const float* patch_embed", "const float* cls_token", "const float* reg_tokens", "const float* pos_embed", "int B",
        "int T", "int R", "int D", "float* tokens", "void* stream"]
    head = _prototype("isc_vit_tokens_out")
    assert _prototype("isc_vit_tokens_out_skip") == head[:3] + ["int skip"] + head[3:]
    assert _prototype("isc_vit_pos_resample_aa") == _prototype("isc_vit_pos_resample")
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive: the ABI version stays


def test_scaled_gemm_argument_checks() -> None:
    lib = _lib.load()
    packed = _lib.ISC_GEMM_A_PACKED | _lib.ISC_GEMM_W_PACKED

    def gemm(a=FAKE, m=300, k=128, w=FAKE, n=256, bias=FAKE, scale=FAKE, res=FAKE, act=_lib.ISC_ACT_NONE, out=FAKE,
             dtype=_lib.ISC_F32, flags=packed):
        return lib.isc_gemm_f16_scaled(a, m, k, w, n, bias, scale, res, act, out, dtype, flags, None)

    for null in ("a", "w", "out", "scale"):  # the scale is not optional
        assert gemm(**{null: None}) == INVALID
    assert gemm(m=0) == INVALID and gemm(k=0) == INVALID and gemm(n=-4) == INVALID
    assert gemm(act=7) == INVALID and gemm(dtype=9) == INVALID and gemm(flags=64) == INVALID
    assert gemm(k=100) == UNSUPPORTED and gemm(n=254) == UNSUPPORTED
    # the documented unsupported forms, on either kernel's operand layout
    for flags in (packed, 0, packed | _lib.ISC_GEMM_TILE_128):
        assert gemm(dtype=_lib.ISC_F16, flags=flags) == UNSUPPORTED
        assert gemm(dtype=_lib.ISC_F16, flags=flags | _lib.ISC_GEMM_OUT_PACKED) == UNSUPPORTED
        assert gemm(flags=flags | _lib.ISC_GEMM_OUT_PACKED) == UNSUPPORTED
        assert gemm(act=_lib.ISC_ACT_GELU, flags=flags) == UNSUPPORTED
        assert gemm(flags=flags | _lib.ISC_GEMM_TILE_256) == UNSUPPORTED
    for odd in ("a", "w", "out", "scale", "bias", "res"):
        assert gemm(**{odd: ODD}) == ALIGNMENT
        assert gemm(**{odd: ODD}, n=384, flags=0) == ALIGNMENT


def test_padded_patchify_argument_checks() -> None:
    lib = _lib.load()

    def patchify(x=FAKE, b=2, c=3, h=42, w=70, patch=14, kpad=640, out=FAKE, packed=1):
        return lib.isc_patchify_f16_padded(x, b, c, h, w, patch, kpad, out, packed, None)

    assert patchify(x=None) == INVALID and patchify(out=None) == INVALID
    assert patchify(b=0) == INVALID and patchify(patch=0) == INVALID and patchify(kpad=0) == INVALID
    for packed in (0, 1):
        assert patchify(kpad=600, packed=packed) == UNSUPPORTED  # not whole K steps
        assert patchify(kpad=576, packed=packed) == UNSUPPORTED  # whole K steps, but fewer than 3 * 14 * 14 columns
        assert patchify(patch=7, h=49, packed=packed) == UNSUPPORTED  # odd patch size
        assert patchify(h=43, packed=packed) == UNSUPPORTED and patchify(w=72, packed=packed) == UNSUPPORTED
    assert patchify(x=ODD) == ALIGNMENT and patchify(out=ODD) == ALIGNMENT


def test_assemble_reg_argument_checks() -> None:
    lib = _lib.load()

    def assemble(pe=FAKE, cls=FAKE, reg=FAKE, pos=FAKE, b=2, t=8, r=4, d=384, out=FAKE):
        return lib.isc_vit_assemble_reg(pe, cls, reg, pos, b, t, r, d, out, None)

    for null in ("pe", "cls", "pos", "out", "reg"):
        assert assemble(**{null: None}) == INVALID
    assert assemble(r=-1) == INVALID
    assert assemble(t=5) == INVALID  # no patch token behind the class token and four registers
    assert assemble(b=0) == INVALID and assemble(d=0) == INVALID
    assert assemble(d=6) == UNSUPPORTED
    for odd in ("pe", "cls", "reg", "pos", "out"):
        assert assemble(**{odd: ODD}) == ALIGNMENT
    assert assemble(r=0, reg=None, t=1) == INVALID  # the limits of isc_vit_assemble when there are no registers


def test_tokens_out_skip_argument_checks() -> None:
    lib = _lib.load()

    def head(x=FAKE, b=2, t=20, skip=5, d=384, gamma=FAKE, beta=FAKE, out=FAKE):
        return lib.isc_vit_tokens_out_skip(x, b, t, skip, d, gamma, beta, 1e-6, 1, 1e-12, out, None)

    assert head(skip=0) == INVALID and head(skip=-1) == INVALID
    assert head(skip=20) == INVALID and head(skip=21) == INVALID  # nothing left behind the skipped rows
    for null in ("x", "gamma", "beta", "out"):
        assert head(**{null: None}) == INVALID
    assert head(d=6) == UNSUPPORTED and head(d=2048) == UNSUPPORTED
    for odd in ("x", "gamma", "beta", "out"):
        assert head(**{odd: ODD}) == ALIGNMENT


def test_pos_resample_aa_argument_checks() -> None:
    lib = _lib.load()
    assert lib.isc_vit_pos_resample_aa(None, 37, 16, 16, 768, FAKE, None) == INVALID
    assert lib.isc_vit_pos_resample_aa(FAKE, 37, 16, 16, 768, None, None) == INVALID
    assert lib.isc_vit_pos_resample_aa(FAKE, 0, 16, 16, 768, FAKE, None) == INVALID
    assert lib.isc_vit_pos_resample_aa(FAKE, 37, 16, 0, 768, FAKE, None) == INVALID
    assert lib.isc_vit_pos_resample_aa(FAKE, 37, 16, 16, 6, FAKE, None) == UNSUPPORTED
    assert lib.isc_vit_pos_resample_aa(FAKE, 37, 4096, 4096, 768, FAKE, None) == UNSUPPORTED
    assert lib.isc_vit_pos_resample_aa(ODD, 37, 16, 16, 768, FAKE, None) == ALIGNMENT
    assert lib.isc_vit_pos_resample_aa(FAKE, 37, 16, 16, 768, ODD, None) == ALIGNMENT
