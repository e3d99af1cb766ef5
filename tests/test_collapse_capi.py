"""The collapsed-search entry points of the C ABI: declared in include/imagescry_hip.h, exported by the built library, bound
in the ctypes table, and their host-side argument checks (no device is touched)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_cosine_topk_collapse_workspace_bytes", "isc_cosine_topk_collapse",
         "isc_cosine_topk_exhaustive_collapse_workspace_bytes", "isc_cosine_topk_exhaustive_collapse",
         "isc_topk_merge_groups")


def _prototype(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in proto.split(",")]


def test_collapse_entry_points_declared_exported_and_bound() -> None:
    build.build(verbose=False)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        params = _prototype(name)
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
    # the collapsed calls are the grouped ones plus what a group answer needs, in front of the stream
    grouped, collapse = _prototype("isc_cosine_topk_grouped"), _prototype("isc_cosine_topk_collapse")
    assert collapse == grouped[:-1] + ["int max_group_rows", "int32_t* out_codes", "void* stream"]
    grouped, collapse = _prototype("isc_cosine_topk_exhaustive_grouped"), _prototype("isc_cosine_topk_exhaustive_collapse")
    assert collapse == grouped[:-1] + ["int32_t* out_codes", "void* stream"]
    assert _lib.SIGNATURES["isc_cosine_topk_collapse"][1][:19] == _lib.SIGNATURES["isc_cosine_topk_grouped"][1][:19]


def test_collapse_argument_checks_on_the_host() -> None:
    lib = _lib.load()
    assert lib.isc_abi_version() == 4
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks before a launch
    odd = ctypes.c_void_p(0x1002)
    need = _lib.c_size_t()
    f16 = _lib.ISC_F16
    assert lib.isc_cosine_topk_collapse_workspace_bytes(f16, 1000, 64, 4, 10, 49, need) == _lib.ISC_OK and need.value > 0
    one = need.value
    assert lib.isc_cosine_topk_collapse_workspace_bytes(f16, 1000, 64, 4, 10, 1, need) == _lib.ISC_OK
    assert lib.isc_cosine_topk_collapse_workspace_bytes(f16, 1000, 64, 4, 10, 0, need) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_cosine_topk_collapse_workspace_bytes(f16, 1000, 64, 4, 121, 49, need) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_cosine_topk_collapse_workspace_bytes(f16, 5, 64, 4, 10, 1, need) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_cosine_topk_collapse_workspace_bytes(f16, 1000, 64, 4, 10, 49, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_cosine_topk_exhaustive_collapse_workspace_bytes(f16, 1000, 64, 4, 10, need) == _lib.ISC_OK
    assert lib.isc_cosine_topk_exhaustive_collapse_workspace_bytes(_lib.ISC_U8, 1000, 64, 4, 10, need) == \
        _lib.ISC_ERR_INVALID_ARG

    def topk(rm=None, rg=fake, qg=None, codes=fake, mgr=49, n=1000, k=10, ws=one):
        return lib.isc_cosine_topk_collapse(fake, f16, n, 64, fake, f16, 4, 64, k, 0, None, fake, fake, fake, fake, ws, rm,
                                            rg, qg, mgr, codes, None)

    def exhaustive(rm=None, rg=fake, qg=None, codes=fake):
        return lib.isc_cosine_topk_exhaustive_collapse(fake, f16, 1000, 64, fake, f16, 4, 64, 10, 0, fake, fake, fake,
                                                       1 << 20, rm, rg, qg, codes, None)

    for call in (topk, exhaustive):
        assert call(rg=None) == _lib.ISC_ERR_INVALID_ARG  # row codes are required
        assert call(codes=None) == _lib.ISC_ERR_INVALID_ARG  # ... and the code output
        assert call(rg=odd) == _lib.ISC_ERR_ALIGNMENT  # row codes: 16-byte vector loads
        assert call(qg=odd) == _lib.ISC_ERR_ALIGNMENT
        assert call(rm=odd) == _lib.ISC_ERR_ALIGNMENT
    assert topk(mgr=0) == _lib.ISC_ERR_INVALID_ARG
    assert topk(n=5) == _lib.ISC_ERR_INVALID_ARG  # k > N
    assert topk(k=121) == _lib.ISC_ERR_UNSUPPORTED
    assert topk(ws=one - 1) == _lib.ISC_ERR_WORKSPACE
    assert topk(codes=odd) == _lib.ISC_ERR_ALIGNMENT
    merge = lib.isc_topk_merge_groups
    assert merge(None, fake, fake, 2, 1, 10, 10, 0, 0, 0, fake, fake, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert merge(fake, fake, None, 2, 1, 10, 10, 0, 0, 0, fake, fake, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert merge(fake, fake, fake, 2, 1, 10, 21, 0, 0, 0, fake, fake, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert merge(fake, fake, fake, 2, 1, 10, 10, 5, 0, 0, fake, fake, fake, None) == _lib.ISC_ERR_INVALID_ARG
    assert merge(fake, fake, fake, 30, 1, 120, 10, 0, 0, 0, fake, fake, fake, None) == _lib.ISC_ERR_UNSUPPORTED
