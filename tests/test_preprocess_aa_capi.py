"""The entry points of the antialiased resize (isc_resize_aa_workspace_bytes, isc_resize_aa): declared in
include/imagescry_hip.h, exported by the built library, bound in the ctypes table, and their host-side argument checks.
No device is touched: every call below has to fail its checks before a launch (a launch here would report
ISC_ERR_LAUNCH or ISC_ERR_NO_DEVICE)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
INVALID, UNSUPPORTED, ALIGNMENT, WORKSPACE = (_lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_ALIGNMENT,
                                              _lib.ISC_ERR_WORKSPACE)
FAKE, ODD, ODD8 = 0x10000, 0x10002, 0x10008  # never dereferenced; ODD is 2-byte, ODD8 8-byte but not 16-byte aligned


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def _bytes(h1=500, w1=375, h2=341, w2=256, top=58, left=16, hc=224, wc=224):
    need = ctypes.c_size_t(0)
    return _lib.load().isc_resize_aa_workspace_bytes(h1, w1, h2, w2, top, left, hc, wc, need), need.value


def _resize(x=FAKE, dtype=_lib.ISC_U8, b=2, c=3, h1=500, w1=375, h2=341, w2=256, top=58, left=16, hc=224, wc=224,
            mean=FAKE, std=FAKE, quantize=1, y=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return _lib.load().isc_resize_aa(x, dtype, b, c, h1, w1, h2, w2, top, left, hc, wc, mean, std, quantize, y, ws,
                                     ws_bytes, None)


def test_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("isc_resize_aa_workspace_bytes", "isc_resize_aa"):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(_prototype(name))
    query = _prototype("isc_resize_aa_workspace_bytes")
    assert query == ["int H1", "int W1", "int H2", "int W2", "int top", "int left", "int Hc", "int Wc", "size_t* bytes"]
    assert not any(re.search(r"\bB\b", a) for a in query)  # the workspace does not grow with the batch
    assert _prototype("isc_resize_aa") == [
        "const void* x", "int dtype", "int B", "int C", "int H1", "int W1", "int H2", "int W2", "int top", "int left",
        "int Hc", "int Wc", "const float* mean", "const float* stdev", "int quantize", "float* y", "void* workspace",
        "size_t workspace_bytes", "void* stream"]
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4  # additive: the ABI version stays


def test_workspace_is_two_small_tables() -> None:
    st, need = _bytes()
    # 224 + 224 outputs: two ints and at most 4 s + 2 = 8 weights each, s = 375 / 256 (whole blocks of 8 weights)
    assert st == _lib.ISC_OK and 0 < need <= 448 * (2 + 8) * 4 + 512
    st, full = _bytes(top=0, left=0, hc=341, wc=256)
    assert st == _lib.ISC_OK and need < full <= 597 * (2 + 8) * 4 + 512  # the tables cover the crop only
    st, big = _bytes(h1=3000, w1=2000, h2=336, w2=224, top=56, left=0)
    assert st == _lib.ISC_OK and big <= 448 * (2 + 40) * 4 + 512  # s = 8.93: 37 taps
    st, up = _bytes(h1=20, w1=13, h2=43, w2=28, top=8, left=0, hc=28, wc=28)
    assert st == _lib.ISC_OK and up <= 56 * (2 + 8) * 4 + 512


def test_workspace_query_argument_checks() -> None:
    assert _lib.load().isc_resize_aa_workspace_bytes(500, 375, 341, 256, 58, 16, 224, 224, None) == INVALID
    for bad in (dict(h1=0), dict(w1=-1), dict(h2=0), dict(w2=0), dict(hc=0), dict(wc=-3), dict(top=-1), dict(left=-1)):
        assert _bytes(**bad)[0] == INVALID
    # the crop rectangle has to lie inside H2 x W2
    assert _bytes(top=118)[0] == INVALID and _bytes(top=117)[0] == _lib.ISC_OK
    assert _bytes(left=33)[0] == INVALID and _bytes(left=32)[0] == _lib.ISC_OK
    assert _bytes(top=2**31 - 1)[0] == INVALID and _bytes(hc=2**31 - 1)[0] == INVALID
    # limits: a downscale factor of 64 per axis, planes and crops below 2^31 elements; any upscale
    assert _bytes(h1=448, w1=470, h2=14, w2=14, top=0, left=0, hc=14, wc=14)[0] == _lib.ISC_OK  # 130+ taps
    assert _bytes(h1=896, w1=896, h2=14, w2=14, top=0, left=0, hc=14, wc=14)[0] == _lib.ISC_OK  # scale 64
    assert _bytes(h1=897, w1=896, h2=14, w2=14, top=0, left=0, hc=14, wc=14)[0] == UNSUPPORTED
    assert _bytes(h1=896, w1=911, h2=14, w2=14, top=0, left=0, hc=14, wc=14)[0] == UNSUPPORTED
    assert _bytes(h1=2, w1=3, h2=2000, w2=3000, top=0, left=0, hc=2000, wc=3000)[0] == _lib.ISC_OK
    assert _bytes(h1=65536, w1=32768, h2=2048, w2=1024, top=0, left=0, hc=224, wc=224)[0] == UNSUPPORTED  # 2^31 a plane
    assert _bytes(h1=64, w1=64, h2=65536, w2=32768, top=0, left=0, hc=65536, wc=32768)[0] == UNSUPPORTED


def test_resize_argument_checks() -> None:
    for null in ("x", "y"):
        assert _resize(**{null: None}) == INVALID
    assert _resize(mean=None) == INVALID and _resize(std=None) == INVALID  # the statistics go together
    assert _resize(dtype=_lib.ISC_F16) == INVALID and _resize(dtype=7) == INVALID
    for bad in (dict(b=0), dict(c=0), dict(h1=0), dict(w1=0), dict(h2=-1), dict(w2=0), dict(hc=0), dict(wc=0),
                dict(top=-1), dict(left=-2), dict(top=118), dict(left=33), dict(hc=342), dict(wc=257)):
        assert _resize(**bad) == INVALID
    assert _resize(h1=22000, h2=341) == UNSUPPORTED  # a downscale factor above 64
    assert _resize(h1=65536, w1=32768, h2=2048, w2=1024) == UNSUPPORTED
    # alignment: floats on 4 bytes, the workspace on 16; a uint8 image anywhere
    for odd in ("y", "mean", "std"):
        assert _resize(**{odd: ODD}) == ALIGNMENT
    assert _resize(ws=ODD8) == ALIGNMENT
    assert _resize(x=ODD, dtype=_lib.ISC_F32) == ALIGNMENT
    st, need = _bytes()
    assert _resize(x=ODD, ws=None) == WORKSPACE  # an unaligned uint8 image passes every check before the workspace's
    assert _resize(ws=None) == WORKSPACE and _resize(ws_bytes=need - 1) == WORKSPACE and _resize(ws_bytes=0) == WORKSPACE
    assert _resize(mean=None, std=None, ws_bytes=need - 1) == WORKSPACE  # without statistics: as far as the workspace
