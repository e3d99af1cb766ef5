"""The PCA fit kernels at the C ABI, each against an exact reference: `isc_feature_sums` (float64 sums of values whose
sum is exact in any order), `isc_center_transpose` (the bits of torch's float32 `(x - mean).T`, exact zeros in the
padding, nothing written behind it), `isc_gram_rows` (integer rows: `torch.equal` with the float64 Gram matrix, up to
the production chunk of 32 768 samples = 1024 K steps per tile; real rows under the derived bound of
tests/matmul_bound.py), and the chunk seams of `PCA.fit` under a Weyl bound.  No tolerance here is measured."""

from __future__ import annotations

import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import matmul_bound as mb  # noqa: E402

pytestmark = pytest.mark.gpu


def _api(device):
    from imagescry_amd import _lib

    return _lib, _lib.load(), _lib.stream_handle(device)


# ----------------------------------------------------------------------------------------------------- isc_feature_sums
def run_feature_sums(device, x_dev: torch.Tensor, n: int, f: int, ldx: int) -> torch.Tensor:
    _lib, lib, stream = _api(device)
    need = _lib.c_size_t()
    _lib.check(lib.isc_feature_sums_workspace_bytes(n, f, need), "isc_feature_sums_workspace_bytes")
    assert need.value == -(-n // 1024) * f * 8
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=device)  # NaN partials unless written
    sums = torch.full((f,), float("nan"), dtype=torch.float64, device=device)
    _lib.check(lib.isc_feature_sums(x_dev.data_ptr(), n, f, ldx, sums.data_ptr(), ws.data_ptr(), ws.numel(), stream),
               "isc_feature_sums")
    return sums.cpu()


@pytest.mark.parametrize("pad", (0, 5), ids=("dense", "ldx=F+5"))
@pytest.mark.parametrize("n,f", ((1, 1), (3, 255), (1023, 256), (1024, 257), (1025, 1280), (4099, 257), (4099, 1), (1, 1280)))
def test_feature_sums_exact(n, f, pad, device: torch.device) -> None:
    """Values in [32, 64) are multiples of 2^-18 and a sum of 4099 of them stays below 2^18: 36 bits, so the float64 sum
    is exact in any order and must equal torch's."""
    g = torch.Generator().manual_seed(n * 13 + f)
    x = torch.randn(n, f + pad, generator=g) * 0.1 + 50.0
    assert float(x.min()) >= 32.0 and float(x.max()) < 64.0
    xd = x.to(device)
    got = run_feature_sums(device, xd[:, :f], n, f, f + pad)
    assert torch.equal(got, x[:, :f].double().sum(0))


def test_feature_sums_against_fsum(device: torch.device) -> None:
    """Plain randn: any-order float64 summation of n terms is within n 2^-53 sum |x| of the exact sum (first order in
    2^-53), which `math.fsum` returns correctly rounded."""
    n, f = 2500, 9
    x = torch.randn(n, f, generator=torch.Generator().manual_seed(5))
    got = run_feature_sums(device, x.to(device), n, f, f)
    for j in range(f):
        col = x[:, j].double().tolist()
        assert abs(float(got[j]) - math.fsum(col)) <= n * 2.0**-53 * math.fsum(abs(v) for v in col), j


def test_feature_sums_refusals(device: torch.device) -> None:
    _lib, lib, stream = _api(device)
    x = torch.zeros(2048, 8, device=device)
    sums = torch.zeros(8, dtype=torch.float64, device=device)
    need = _lib.c_size_t()
    _lib.check(lib.isc_feature_sums_workspace_bytes(2048, 8, need), "ws")
    ws = torch.zeros(need.value, dtype=torch.uint8, device=device)
    call = lib.isc_feature_sums
    assert call(x.data_ptr(), 2048, 8, 8, sums.data_ptr(), ws.data_ptr(), need.value - 1, stream) == _lib.ISC_ERR_WORKSPACE
    assert call(x.data_ptr(), 2048, 8, 7, sums.data_ptr(), ws.data_ptr(), need.value, stream) == _lib.ISC_ERR_INVALID_ARG
    # more row blocks than a grid's y axis holds: refused before any launch (the pointers are never read)
    assert call(x.data_ptr(), 65536 * 1024, 8, 8, sums.data_ptr(), ws.data_ptr(), need.value, stream) == _lib.ISC_ERR_UNSUPPORTED
    assert call(x.data_ptr(), 2048, 8, 8, sums.data_ptr(), ws.data_ptr(), need.value, stream) == _lib.ISC_OK
    torch.cuda.synchronize(device)
    assert torch.equal(sums.cpu(), torch.zeros(8, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------- isc_center_transpose
SENTINEL = -7.25


def check_center_transpose(device, n: int, f: int, ldx: int, fpad: int, ldn: int) -> None:
    _lib, lib, stream = _api(device)
    g = torch.Generator().manual_seed(n * 101 + f * 7 + ldx)
    x = torch.randn(n, ldx, generator=g) + 50.0
    mean = x[:, :f].mean(0) + 0.01 * torch.randn(f, generator=g)
    tail = 64
    buf = torch.full((fpad * ldn + tail,), float("nan"), device=device)
    buf[fpad * ldn :] = SENTINEL
    xd, md = x.to(device), mean.to(device)
    _lib.check(lib.isc_center_transpose(xd.data_ptr(), n, f, ldx, md.data_ptr(), buf.data_ptr(), fpad, ldn, stream),
               "isc_center_transpose")
    got = buf.cpu()
    xt = got[: fpad * ldn].reshape(fpad, ldn)
    what = f"n={n} F={f} ldx={ldx} Fpad={fpad} ldn={ldn}"
    want = (x[:, :f] - mean).T.contiguous()  # float32, one correctly rounded subtraction per element
    assert torch.equal(xt[:f, :n].contiguous().view(torch.int32), want.view(torch.int32)), what
    # exact (positive) zeros in the padding rows and columns
    assert torch.equal(xt[f:].contiguous().view(torch.int32), torch.zeros((fpad - f, ldn), dtype=torch.int32)), what
    assert torch.equal(xt[:, n:].contiguous().view(torch.int32), torch.zeros((fpad, ldn - n), dtype=torch.int32)), what
    assert torch.equal(got[fpad * ldn :], torch.full((tail,), SENTINEL)), what


@pytest.mark.parametrize("n,f", ((1, 1), (31, 3), (32, 4), (33, 33), (1000, 96), (1000, 1), (1, 96), (33, 3), (31, 33)))
def test_center_transpose_bits(n, f, device: torch.device) -> None:
    for fpad in ((f + 3) // 4 * 4, f + 32):
        for ldn in ((n + 31) // 32 * 32, (n + 31) // 32 * 32 + 64):
            check_center_transpose(device, n, f, f, fpad, ldn)


def test_center_transpose_strided_input(device: torch.device) -> None:
    check_center_transpose(device, 33, 33, 40, 36, 64)


# -------------------------------------------------------------------------------------------------------- isc_gram_rows
def run_gram(device, xt: torch.Tensor) -> torch.Tensor:
    _lib, lib, stream = _api(device)
    f, n = xt.shape
    xd = xt.contiguous().to(device)
    gram = torch.full((f, f), float("nan"), device=device)
    _lib.check(lib.isc_gram_rows(xd.data_ptr(), f, n, gram.data_ptr(), stream), "isc_gram_rows")
    return gram.cpu()


@pytest.mark.parametrize(
    "f,n",
    (
        (4, 32),  # the 32-channel tile, one K step
        (36, 64),
        (64, 4096),
        (132, 32768),  # the production chunk: 1024 K steps, ragged in both tile directions
        (768, 32768),
        (1280, 2048),  # 100 tiles, no whole round: all half tiles
    ),
)
def test_gram_rows_exact_integers(f, n, device: torch.device) -> None:
    """Rows in -3 .. 3: every partial sum is an integer of at most 9 n < 2^24, so the float32 result is the float64 Gram
    matrix whatever the order of the K steps -- and a dropped or repeated step cannot hide."""
    xt = mb.int_tensor((f, n), -3, 3, torch.Generator().manual_seed(f + n))
    mb.assert_exact_range(xt, xt)
    got = run_gram(device, xt)
    assert torch.equal(got, got.T)
    want = mb.product_f64(xt, xt)
    assert torch.equal(got.double(), want), mb.worst_ratio(got, want, torch.full_like(want, 2.0**-24))


def test_gram_rows_within_bound(device: torch.device) -> None:
    f, n = 100, 1024
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, f, generator=g) @ torch.randn(f, f, generator=g) * 0.1 + 50.0
    xt = (x - x.mean(0)).T.contiguous()
    got = run_gram(device, xt)
    ratio = mb.assert_within_bound(got, mb.product_f64(xt, xt), mb.product_bound(xt, xt), "gram 100 x 1024")
    print(f"gram_rows (100, 1024): error / bound = {ratio:.4f}")
    assert torch.equal(got, got.T)


def test_gram_rows_refusals(device: torch.device) -> None:
    _lib, lib, stream = _api(device)
    xt = torch.zeros(8, 64, device=device)
    gram = torch.zeros(8, 8, device=device)
    assert lib.isc_gram_rows(xt.data_ptr(), 8, 48, gram.data_ptr(), stream) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_gram_rows(xt.data_ptr(), 6, 64, gram.data_ptr(), stream) == _lib.ISC_ERR_UNSUPPORTED
    assert lib.isc_gram_rows(xt.data_ptr(), 8, 64, gram.data_ptr(), stream) == _lib.ISC_OK
    torch.cuda.synchronize(device)


# ------------------------------------------------------------------------------------------------ chunk seams of PCA.fit
@pytest.mark.parametrize("n,c", ((97, 32), (65, 64), (64, 32), (33, 32)))
def test_fit_chunk_seams(n, c, device: torch.device, monkeypatch: pytest.MonkeyPatch) -> None:
    """`PCA.fit` with chunks of c rows: last chunks of one row (97, 65, 33) and of a whole chunk (64).

    Reference: the float64 eigenvalues of Xc^T Xc with Xc = x - fitted float32 mean (each subtraction rounded to float32,
    as `isc_center_transpose` does).  The Gram matrix `fit` accumulates differs from Xc^T Xc by a symmetric E with
    |E| <= sum over the chunks of (c + 2) 2^-23 |Xc_chunk|^T |Xc_chunk| element-wise (tests/matmul_bound.py with K = c; the
    float64 accumulation of the chunks is far below it), so by Weyl's inequality every eigenvalue moves by at most
    ||E||_2 <= ||E||_F, and the explained-variance ratios agree within 2 ||E||_F / sum(lambda) + 2^-21 (the last term: the
    three float32 operations of the ratio).  A reference that lost its last row must lie OUTSIDE that tolerance, else the
    test could not see a lost row."""
    from imagescry_amd.decomposition import PCA

    f = 20
    g = torch.Generator().manual_seed(n * 3 + c)
    x = torch.randn(n, f, generator=g) @ torch.randn(f, f, generator=g) * 0.1 + 50.0
    assert float(x.min()) >= 32.0 and float(x.max()) < 64.0
    monkeypatch.setattr(PCA, "GRAM_CHUNK_ROWS", c)
    pca = PCA().fit(x.to(device))
    mean = pca.feature_means.cpu().reshape(f)
    assert torch.equal(mean, (x.double().sum(0) / n).float())  # sums exact (values in [32, 64)), one division, one rounding
    xc = (x - mean).double()

    def ratios(rows: torch.Tensor) -> tuple[torch.Tensor, float]:
        lam = torch.linalg.eigvalsh(rows.T @ rows).flip(0).clamp_min(0.0)
        return lam / lam.sum(), float(lam.sum())

    e = torch.zeros(f, f, dtype=torch.float64)
    for r0 in range(0, n, c):
        blk = xc[r0 : r0 + c].abs()
        e += (c + 2) * mb.U2 * (blk.T @ blk)
    want, total = ratios(xc)
    tol = 2 * float(torch.linalg.matrix_norm(e)) / total + 2.0**-21
    got = pca.explained_variance.cpu().double()
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"fit seams n={n} c={c}: max ratio error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (err, tol)
    lost, _ = ratios(xc[:-1])
    assert float((lost - got).abs().max()) > tol, "the tolerance could not tell a lost row"
