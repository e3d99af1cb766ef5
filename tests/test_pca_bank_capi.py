"""Host-only calls of the bank PCA entry points (include/imagescry_hip.h: isc_bank_gram, isc_bank_project): argument
validation happens before anything is launched, so it runs without a GPU, and the workspace size is the documented one."""

from __future__ import annotations

import ctypes

import pytest

from imagescry_amd import _lib, build

OK, INVALID, UNSUPPORTED = _lib.ISC_OK, _lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED
F16, F32 = _lib.ISC_F16, _lib.ISC_F32


@pytest.fixture(scope="module")
def lib() -> ctypes.CDLL:
    build.build(verbose=False)
    return _lib.load()


def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def test_chunk_rows_is_a_multiple_of_the_tile(lib) -> None:
    chunk = lib.isc_bank_gram_chunk_rows()
    assert chunk > 0 and chunk % 256 == 0


@pytest.mark.parametrize("dtype", (F16, F32))
@pytest.mark.parametrize("n,d", ((1, 8), (256, 64), (257, 128), (700, 129), (32768, 768), (32769, 1280), (1_000_000, 768),
                                 (50_000_000, 2048)))
def test_workspace_is_the_documented_size(lib, n, d, dtype) -> None:
    chunk = lib.isc_bank_gram_chunk_rows()
    need = ctypes.c_size_t()
    assert lib.isc_bank_gram_workspace_bytes(dtype, n, d, need) == OK
    chunks = _ceil(_ceil(n, 256) * 256, chunk)
    dpad = _ceil(d, 128) * 128  # the header: D rounded up to a multiple of 128
    counts = _ceil(chunks * 8, 256) * 256  # the header: one int64 per chunk, rounded up to 256 bytes
    assert need.value == chunks * dpad * dpad * 4 + counts


def test_workspace_arguments(lib) -> None:
    need = ctypes.c_size_t()
    assert lib.isc_bank_gram_workspace_bytes(F16, 100, 2048, need) == OK
    assert lib.isc_bank_gram_workspace_bytes(F16, 100, 2049, need) == UNSUPPORTED
    assert lib.isc_bank_gram_workspace_bytes(F16, 100, 0, need) == INVALID
    assert lib.isc_bank_gram_workspace_bytes(F16, -1, 8, need) == INVALID
    assert lib.isc_bank_gram_workspace_bytes(F16, 2**31 - 1, 8, need) == INVALID
    assert lib.isc_bank_gram_workspace_bytes(_lib.ISC_U8, 100, 8, need) == INVALID
    assert lib.isc_bank_gram_workspace_bytes(F16, 100, 8, None) == INVALID


def test_gram_rejects_bad_arguments_before_any_launch(lib) -> None:
    assert lib.isc_bank_gram(None, F16, 100, 8, None, None, None, 8, None, None, 0, None) == INVALID
    assert lib.isc_bank_gram(None, F16, 100, 2049, None, None, None, 2049, None, None, 0, None) == UNSUPPORTED
    assert lib.isc_bank_gram(None, _lib.ISC_U8, 100, 8, None, None, None, 8, None, None, 0, None) == INVALID
    assert lib.isc_bank_gram(None, F16, 100, 8, None, None, None, 7, None, None, 0, None) == INVALID  # ld < D
    assert lib.isc_bank_gram(None, F16, 0, 8, None, None, None, 8, None, None, 0, None) == OK  # N == 0: no launch


def test_project_rejects_bad_arguments_before_any_launch(lib) -> None:
    def call(n=100, d=8, k=4, ldw=4, ldo=4, dtype=F16, out_dtype=F16, out_rows=None, out_packed=None):
        return lib.isc_bank_project(None, dtype, n, d, None, None, k, ldw, None, out_rows, ldo, out_packed, out_dtype, 1,
                                    1e-12, None, None)

    fake = 4096  # never dereferenced: every call below is refused, or has no row to launch for
    assert call() == INVALID  # no output, NULL bank
    assert call(out_rows=fake) == INVALID  # NULL bank, mean and w
    assert call(d=2049, k=4, out_rows=fake) == UNSUPPORTED
    assert call(k=9, ldw=9, ldo=9, out_rows=fake) == INVALID  # K > D
    assert call(k=0, out_rows=fake) == INVALID
    assert call(ldw=3, out_rows=fake) == INVALID
    assert call(ldo=3, out_rows=fake) == INVALID
    assert call(out_packed=fake, out_dtype=_lib.ISC_U8) == INVALID
    assert call(dtype=_lib.ISC_U8, out_rows=fake) == INVALID
    assert call(n=0) == INVALID  # at least one output, even for an empty bank
    assert call(n=0, out_rows=fake) == OK
