"""The stored-row entry points of the C ABI (isc_bank_gather, isc_cosine_scores): declared in include/imagescry_hip.h,
exported by the built library, bound in the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_bank_gather", "isc_cosine_scores")


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_row_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    assert _prototype("isc_bank_gather") == [
        "const void* packed", "int dtype", "int D", "int64_t capacity", "const int64_t* rows", "int64_t m",
        "const uint32_t* fill_mask", "void* out", "int64_t ldo", "void* stream"]
    assert _prototype("isc_cosine_scores") == [
        "const void* bank", "int dtype", "int64_t capacity", "int D", "const void* queries", "int q_dtype", "int Q",
        "int64_t ldq", "const int64_t* rows", "int64_t M", "const uint32_t* fill_mask", "float* scores", "int64_t lds",
        "void* stream"]
    # 64-bit sizes and leading dimensions are bound as such
    gather, scores = _lib.SIGNATURES["isc_bank_gather"][1], _lib.SIGNATURES["isc_cosine_scores"][1]
    assert [gather[i] for i in (3, 5, 8)] == [ctypes.c_int64] * 3
    assert [scores[i] for i in (2, 7, 9, 12)] == [ctypes.c_int64] * 4


def test_the_abi_version_stays_4() -> None:
    assert _lib.load().isc_abi_version() == _lib.ISC_ABI_VERSION == 4


def test_gather_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    F16, F32 = _lib.ISC_F16, _lib.ISC_F32
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks before a launch
    odd2, odd4, odd8, odd16 = (ctypes.c_void_p(0x1000 + o) for o in (1, 2, 4, 8))

    def gather(packed=fake, dtype=F16, d=100, cap=300, rows=fake, m=10, fill=None, out=fake, ldo=100):
        return lib.isc_bank_gather(packed, dtype, d, cap, rows, m, fill, out, ldo, None)

    assert gather(packed=None) == _lib.ISC_ERR_INVALID_ARG
    assert gather(rows=None) == _lib.ISC_ERR_INVALID_ARG
    assert gather(out=None) == _lib.ISC_ERR_INVALID_ARG
    assert gather(dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert gather(dtype=7) == _lib.ISC_ERR_INVALID_ARG
    assert gather(d=0) == _lib.ISC_ERR_INVALID_ARG
    assert gather(ldo=99) == _lib.ISC_ERR_INVALID_ARG
    assert gather(m=-1) == _lib.ISC_ERR_INVALID_ARG
    assert gather(cap=0) == _lib.ISC_ERR_INVALID_ARG
    assert gather(cap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    assert gather(packed=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert gather(rows=odd8) == _lib.ISC_ERR_ALIGNMENT
    assert gather(fill=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert gather(out=odd2) == _lib.ISC_ERR_ALIGNMENT
    assert gather(dtype=F32, out=odd4) == _lib.ISC_ERR_ALIGNMENT
    # nothing to read: OK without a launch (there is no device here: a launch would fail), whatever the pointers
    assert gather(m=0) == _lib.ISC_OK
    assert gather(m=0, packed=None, rows=None, out=None) == _lib.ISC_OK
    assert gather(m=0, ldo=99) == _lib.ISC_ERR_INVALID_ARG  # ... but not whatever the shape


def test_scores_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    F16, F32 = _lib.ISC_F16, _lib.ISC_F32
    fake = ctypes.c_void_p(0x1000)
    odd2, odd4, odd8, odd16 = (ctypes.c_void_p(0x1000 + o) for o in (1, 2, 4, 8))

    def scores(bank=fake, dtype=F16, cap=300, d=100, q=fake, q_dtype=F32, nq=3, ldq=100, rows=fake, m=10, fill=None,
               out=fake, lds=10):
        return lib.isc_cosine_scores(bank, dtype, cap, d, q, q_dtype, nq, ldq, rows, m, fill, out, lds, None)

    assert scores(bank=None) == _lib.ISC_ERR_INVALID_ARG
    assert scores(q=None) == _lib.ISC_ERR_INVALID_ARG
    assert scores(rows=None) == _lib.ISC_ERR_INVALID_ARG
    assert scores(out=None) == _lib.ISC_ERR_INVALID_ARG
    assert scores(dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert scores(q_dtype=_lib.ISC_U8) == _lib.ISC_ERR_INVALID_ARG
    assert scores(d=0) == _lib.ISC_ERR_INVALID_ARG
    assert scores(ldq=99) == _lib.ISC_ERR_INVALID_ARG
    assert scores(lds=9) == _lib.ISC_ERR_INVALID_ARG
    assert scores(nq=-1) == _lib.ISC_ERR_INVALID_ARG
    assert scores(m=-1) == _lib.ISC_ERR_INVALID_ARG
    assert scores(cap=0) == _lib.ISC_ERR_INVALID_ARG
    assert scores(cap=1 << 31) == _lib.ISC_ERR_INVALID_ARG
    big = _lib.ISC_SEARCH_MAX_D + 1
    assert scores(d=big, ldq=big) == _lib.ISC_ERR_UNSUPPORTED  # the searches' limit, the searches' status
    assert scores(d=big, ldq=big, nq=0) == _lib.ISC_ERR_UNSUPPORTED
    assert scores(bank=odd16) == _lib.ISC_ERR_ALIGNMENT
    assert scores(q=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert scores(q=odd2, q_dtype=F16) == _lib.ISC_ERR_ALIGNMENT
    assert scores(rows=odd8) == _lib.ISC_ERR_ALIGNMENT
    assert scores(fill=odd4) == _lib.ISC_ERR_ALIGNMENT
    assert scores(out=odd4) == _lib.ISC_ERR_ALIGNMENT
    # nothing to score: OK without a launch
    assert scores(nq=0) == _lib.ISC_OK
    assert scores(m=0, lds=0) == _lib.ISC_OK
    assert scores(nq=0, bank=None, q=None, rows=None, out=None) == _lib.ISC_OK
    assert scores(m=0, lds=0, bank=None, q=None, rows=None, out=None) == _lib.ISC_OK
