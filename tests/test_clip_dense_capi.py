"""The three C-ABI entries behind the dense CLIP patch map -- isc_attention_f16_self, isc_attention_f16_self_stream,
isc_tokens_to_map -- are exported, typed and validate their arguments before anything is launched (no GPU here: every
call below returns from the host checks; the buffers are host memory that is never dereferenced)."""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest

from imagescry_amd import _lib, build

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NEW = ("isc_attention_f16_self", "isc_attention_f16_self_stream", "isc_tokens_to_map")


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def buf() -> int:
    """The address of a 16-byte aligned host buffer (kept alive by the module-level list)."""
    raw = ctypes.create_string_buffer(4096 + 16)
    _KEEP.append(raw)
    return (ctypes.addressof(raw) + 15) // 16 * 16


_KEEP: list = []


def test_symbols_are_exported_and_typed_and_the_abi_version_stays(lib):
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
        params = [" ".join(a.split()) for a in proto.split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, params)
        for p, a in zip(params, argtypes):  # int -> c_int, float -> c_float, any pointer -> c_void_p
            want = ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else ctypes.c_int
            assert a is want, (name, p, a)
        assert getattr(lib, name).argtypes == argtypes
    for name in NEW[:2]:  # `part` sits behind head_dim, in front of the output
        proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S).group(1)
        params = [" ".join(a.split()) for a in proto.split(",")]
        assert params[4] == "int head_dim" and params[5] == "int part" and params[6] == "void* out", params
    assert re.search(r"#define ISC_ATT_PART_QUERY 0\b", text) and re.search(r"#define ISC_ATT_PART_KEY 1\b", text)
    assert (_lib.ISC_ATT_PART_QUERY, _lib.ISC_ATT_PART_KEY) == (0, 1)
    assert lib.isc_abi_version() == _lib.ISC_ABI_VERSION == 4
    assert re.search(r"#define ISC_ABI_VERSION 4\b", HEADER.read_text())


@pytest.mark.parametrize("name", NEW[:2])
def test_self_attention_argument_validation(lib, buf, name):
    fn = getattr(lib, name)
    q, k = _lib.ISC_ATT_PART_QUERY, _lib.ISC_ATT_PART_KEY
    for part in (q, k):
        assert fn(None, 2, 17, 3, 64, part, buf, 0, None) == _lib.ISC_ERR_INVALID_ARG
        assert fn(buf, 2, 17, 3, 64, part, None, 0, None) == _lib.ISC_ERR_INVALID_ARG
        assert fn(buf, 0, 17, 3, 64, part, buf, 0, None) == _lib.ISC_ERR_INVALID_ARG
        assert fn(buf, 2, 0, 3, 64, part, buf, 0, None) == _lib.ISC_ERR_INVALID_ARG
        assert fn(buf, 2, 17, 0, 64, part, buf, 0, None) == _lib.ISC_ERR_INVALID_ARG
        assert fn(buf, 2, 17, 2, 96, part, buf, 0, None) == _lib.ISC_ERR_UNSUPPORTED
        assert fn(buf + 2, 2, 17, 3, 64, part, buf, 0, None) == _lib.ISC_ERR_ALIGNMENT
        assert fn(buf, 2, 17, 3, 64, part, buf + 8, 1, None) == _lib.ISC_ERR_ALIGNMENT
    for part in (2, -1, 3):  # the value columns are no choice
        assert fn(buf, 2, 17, 3, 64, part, buf, 0, None) == _lib.ISC_ERR_INVALID_ARG
        assert fn(buf, 2, 17, 3, 64, part, buf, 1, None) == _lib.ISC_ERR_INVALID_ARG
    # the limits of the entry it mirrors
    if name == "isc_attention_f16_self":
        assert fn(buf, 2, 225, 3, 64, k, buf, 0, None) == _lib.ISC_ERR_UNSUPPORTED
        assert lib.isc_attention_f16(buf, 2, 225, 3, 64, buf, 0, None) == _lib.ISC_ERR_UNSUPPORTED
    else:
        assert fn(buf, 2**20, 2**11, 1, 64, k, buf, 0, None) == _lib.ISC_ERR_UNSUPPORTED
        assert lib.isc_attention_f16_stream(buf, 2**20, 2**11, 1, 64, buf, 0, None) == _lib.ISC_ERR_UNSUPPORTED


def test_tokens_to_map_argument_validation(lib, buf):
    fn = lib.isc_tokens_to_map
    assert fn(None, 2, 26, 1, 512, 1, 1e-12, buf, None) == _lib.ISC_ERR_INVALID_ARG
    assert fn(buf, 2, 26, 1, 512, 1, 1e-12, None, None) == _lib.ISC_ERR_INVALID_ARG
    assert fn(buf, 0, 26, 1, 512, 1, 1e-12, buf, None) == _lib.ISC_ERR_INVALID_ARG
    assert fn(buf, 2, 26, 0, 512, 1, 1e-12, buf, None) == _lib.ISC_ERR_INVALID_ARG  # skip = 0
    assert fn(buf, 2, 26, 26, 512, 1, 1e-12, buf, None) == _lib.ISC_ERR_INVALID_ARG  # skip = T
    assert fn(buf, 2, 26, 27, 512, 1, 1e-12, buf, None) == _lib.ISC_ERR_INVALID_ARG
    assert fn(buf, 2, 26, 1, 512, 1, -1.0, buf, None) == _lib.ISC_ERR_INVALID_ARG
    assert fn(buf, 2, 26, 1, 1028, 1, 1e-12, buf, None) == _lib.ISC_ERR_UNSUPPORTED  # D > 1024
    assert fn(buf, 2, 26, 1, 6, 1, 1e-12, buf, None) == _lib.ISC_ERR_UNSUPPORTED  # D % 4
    assert fn(buf + 4, 2, 26, 1, 512, 0, 1e-12, buf, None) == _lib.ISC_ERR_ALIGNMENT
    assert fn(buf, 2, 26, 1, 512, 0, 1e-12, buf + 8, None) == _lib.ISC_ERR_ALIGNMENT
    # the LayerNorm head it shares a kernel with still asks for its affine
    assert lib.isc_vit_tokens_out_skip(buf, 2, 26, 1, 512, None, buf, 1e-6, 1, 1e-12, buf, None) == _lib.ISC_ERR_INVALID_ARG
    assert lib.isc_vit_tokens_out_skip(buf, 2, 26, 1, 512, buf, buf + 4, 1e-6, 1, 1e-12, buf, None) == _lib.ISC_ERR_ALIGNMENT
