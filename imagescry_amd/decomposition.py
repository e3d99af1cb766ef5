"""Principal component analysis and spherical k-means on MI355X.

Same constructor arguments, attributes and behaviour as the reference `PCA`
(src/imagescry/models/decomposition.py:11-180).  `fit` keeps everything sample-sized on the GPU -- float64 feature sums,
centred + transposed chunks and their Gram matrices on the f32 matrix cores -- and leaves the host the `F x F`
symmetric eigenproblem, where the reference runs an SVD of the whole `[N, F]` matrix on the host.  `transform` /
`forward` -- the step the reference applies to every embedding batch right after the hot path
(src/imagescry/models/pipelines.py:76-84) -- runs in the HIP kernel behind `isc_linear_centered`:
`(x - feature_means) @ component_vectors` with the centring done before the product.
`fit_bank` fits on the rows of an `EmbeddingBank` without unpacking it (`isc_bank_gram`), and `EmbeddingBank.project`
compresses the bank the same way (`isc_bank_project`).

`KMeans` clusters the rows of an `EmbeddingBank` by cosine similarity without unpacking it: every iteration is one
`EmbeddingBank.assign` (labels only) and one `EmbeddingBank.group_sums`.
"""

from __future__ import annotations

import torch
from torch import Tensor

from imagescry_amd import _lib

__all__ = ["PCA", "KMeans"]


class PCA:
    """Linear projection to a lower dimensional space using the SVD of the centred data."""

    def __init__(
        self,
        *,
        min_num_components: int = 1,
        max_num_components: int | None = None,
        min_explained_variance: float = 0.0,
        num_features: int = 0,
        num_components: int = 0,
    ) -> None:
        # The same three argument checks as the reference constructor (decomposition.py:46-52: ValueError for each), worded
        # here; callers match on the exception type.
        if min_num_components < 1:
            raise ValueError(f"PCA needs min_num_components >= 1 (got {min_num_components})")
        if max_num_components is not None and max_num_components < min_num_components:
            raise ValueError(
                f"max_num_components={max_num_components} is below min_num_components={min_num_components}"
            )
        if not 0.0 <= min_explained_variance <= 1.0:
            raise ValueError(f"min_explained_variance is a fraction in [0, 1] (got {min_explained_variance})")
        self.min_num_components = min_num_components
        self.max_num_components = max_num_components
        self.min_explained_variance = min_explained_variance
        self.hparams: dict[str, object] = {
            "min_num_components": min_num_components,
            "max_num_components": max_num_components,
            "min_explained_variance": min_explained_variance,
        }
        self._fitted = False
        self._num_features = 0
        self._num_components = 0
        self.feature_means = torch.empty((1, num_features))
        self.explained_variance = torch.empty((num_features,))
        self.component_vectors = torch.empty((num_features, num_components))
        self._device = torch.device("cpu")
        self._packed: tuple[Tensor, Tensor] | None = None  # (mean [Fpad], weights [Kpad, Fpad]) on the device

    def __repr__(self) -> str:
        # contract string: the reference prints the two sizes, or "not fitted" for both (decomposition.py:73-76)
        shown = (self.num_features, self.num_components) if self.fitted else ("not fitted", "not fitted")
        return f"{type(self).__name__}(num_features={shown[0]}, num_components={shown[1]})"

    # ------------------------------------------------------------------ fit (device + an F x F eigenproblem)
    GRAM_CHUNK_ROWS = 32768  # samples per Gram launch: each chunk's sum is float32, the chunks are added in float64

    def fit(self, x: Tensor) -> "PCA":
        """Principal axes of the centred (not scaled) rows and how many of them the constructor arguments ask for.

        `x` is used as float32 (a float64 input is rounded once, and `feature_means` is float32 whatever the input type).
        The reference centres `x` and takes `torch.linalg.svd` of the `[N, F]` matrix on the host
        (decomposition.py:118-146).  Here everything N-sized runs on the GPU, in three kernels: per-feature sums in
        float64 (`isc_feature_sums`), the centred rows written transposed chunk by chunk (`isc_center_transpose`), and
        the `F x F` Gram matrix of every chunk on the f32 matrix cores (`isc_gram_rows`), added up in float64.  The
        eigenvectors of the Gram matrix ARE the right singular vectors, its eigenvalues the squared singular values, so
        the one thing left for the host is the `F x F` symmetric eigenproblem (LAPACK, float64).  Outputs as the
        reference: `feature_means [1, F]`, `explained_variance [min(N, F)]`, `component_vectors [F, K]`, K chosen by
        the same rule (decomposition.py:133-142).  A principal axis is defined up to its sign; the sign is fixed here by
        making each component's largest-magnitude entry positive.
        """
        if not isinstance(x, Tensor) or not x.dtype.is_floating_point or x.ndim != 2:
            raise TypeError("x must be a floating point [num_samples, num_features] tensor")
        num_samples, num_features = x.shape
        if num_samples < 2:
            raise ValueError(f"num_samples must be at least 2, got {num_samples}")
        if x.device.type != "cuda":
            # The reference is always called as `PCA(...).fit(host_samples)` (decomposition.py:94-148): a host tensor goes
            # to the model's device, or -- for a model that has not been placed yet -- to the current HIP device.  That is a
            # copy, not a CPU computation: without a HIP device the call raises below.
            if self._device.type == "cuda":
                x = x.to(self._device)
            elif torch.cuda.is_available():
                x = x.to(torch.device("cuda", torch.cuda.current_device()))
        _lib.require_device(x, "x")  # no CPU fallback
        dev = x.device
        lib = _lib.load()
        xf = x.detach().float()
        if xf.stride(1) != 1:
            xf = xf.contiguous()
        n, f = num_samples, num_features
        fpad = (f + 3) // 4 * 4
        with torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)
            need = _lib.c_size_t()
            _lib.check(lib.isc_feature_sums_workspace_bytes(n, f, need), "isc_feature_sums_workspace_bytes")
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            sums = torch.empty(f, dtype=torch.float64, device=dev)
            _lib.check(lib.isc_feature_sums(xf.data_ptr(), n, f, xf.stride(0), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                            stream), "isc_feature_sums")
            mean = (sums / n).float()  # what the reference subtracts: a float32 mean
            # rows per chunk: F * rows < 2^31 (32-bit element offsets in the kernel), whole K steps of 32 samples
            chunk = max(32, min(self.GRAM_CHUNK_ROWS, ((2**31 - 1) // fpad) // 32 * 32))
            ld = (min(chunk, n) + 31) // 32 * 32
            xt = torch.empty((fpad, ld), dtype=torch.float32, device=dev)
            gram_chunk = torch.empty((fpad, fpad), dtype=torch.float32, device=dev)
            gram = torch.zeros((fpad, fpad), dtype=torch.float64, device=dev)
            for r0 in range(0, n, chunk):
                rows = min(chunk, n - r0)
                ldn = (rows + 31) // 32 * 32
                blk = xf[r0 : r0 + rows]
                _lib.check(lib.isc_center_transpose(blk.data_ptr(), rows, f, xf.stride(0), mean.data_ptr(), xt.data_ptr(),
                                                    fpad, ldn, stream), "isc_center_transpose")
                _lib.check(lib.isc_gram_rows(xt.data_ptr(), fpad, ldn, gram_chunk.data_ptr(), stream), "isc_gram_rows")
                gram += gram_chunk.double()
        return self._finish_fit(gram[:f, :f].cpu(), n, f, mean, dev)

    def _finish_fit(self, g: Tensor, n: int, f: int, mean: Tensor, dev: torch.device) -> "PCA":
        """The host tail of `fit` and `fit_bank`: `g` is the float64 `[F, F]` Gram matrix of the `n` centred samples (host),
        `mean` the float32 `[F]` mean on `dev`.  Symmetrise, `eigh`, descending order, the sign convention, the float32
        explained variance and the choice of the component count."""
        g = (g + g.T) * 0.5
        evals, evecs = torch.linalg.eigh(g)  # ascending; float64
        evals = torch.flip(evals, dims=(0,)).clamp_min(0.0)
        evecs = torch.flip(evecs, dims=(1,))
        lead = evecs.abs().argmax(dim=0)
        evecs = evecs * torch.sign(evecs[lead, torch.arange(f)]).masked_fill_(evecs[lead, torch.arange(f)] == 0, 1.0)
        rank = min(n, f)  # the reference's SVD returns min(N, F) singular values
        # From here on in float32, as the reference computes it (s ** 2 / (n - 1), its sum, the ratio and the cumulative sum
        # are all float32 tensors there, decomposition.py:124-128): with a threshold near 1 the count of components depends
        # on the rounding of the tail of that float32 cumsum, so the same arithmetic is used.  Accuracy floor: the Gram
        # route squares the condition number, eigenvalues below ~1e-7 of the largest are rounding noise (clamped at 0).
        eigenvalues = (evals[:rank] / (n - 1)).float()
        explained = eigenvalues / torch.sum(eigenvalues)
        cumulative = torch.cumsum(explained, dim=0)
        needed = int((cumulative < self.min_explained_variance).sum().item()) + 1
        num_components = max(self.min_num_components, needed)
        if self.max_num_components is not None:
            num_components = min(self.max_num_components, num_components)
        num_components = min(num_components, f)
        self._num_features = f
        self._num_components = num_components
        self.feature_means = mean.reshape(1, f)
        self.explained_variance = explained.to(dev)
        self.component_vectors = evecs[:, :num_components].float().contiguous().to(dev)
        self._fitted = True
        self.hparams.update({"num_features": f, "num_components": num_components})
        self._device = dev
        self._packed = None
        return self

    def fit_bank(self, bank, *, mask=None) -> "PCA":
        """`fit` on the live rows of an `EmbeddingBank` (those `mask` -- a `RowFilter` or bool `[N]` -- allows, when given)
        without unpacking it: the rows are read from the packed image as stored (float16 or float32) and nothing row-sized
        is allocated.  The mean comes from `bank.group_sums` with one group -- float64 sums in a fixed order, then
        `(sums / n).float()` as in `fit` --, the centred Gram matrix from one `isc_bank_gram` (float32 partials per chunk of
        packed rows on the f32 matrix cores, added in float64 in chunk order: the same bank gives the same bits), and the
        host tail is `fit`'s.  `n` is the number of live, allowed rows (one host read); fewer than 2 raise ValueError, and
        so does a sharded bank."""
        if bank.process_group is not None:
            raise ValueError("a sharded bank (process_group=) cannot be fitted: " + bank._ROWS_ON_ONE_RANK)
        rf = bank._as_filter(mask)
        rows, f = len(bank), bank.dim
        dev = bank.device
        if rows == 0:
            raise ValueError("num_samples must be at least 2, got 0")
        live = bank.live if rf is None or rf.packed is bank._fill else bank._unpack_mask(rf.packed, rows)
        sums, counts = bank.group_sums(torch.where(live, 0, -1), 1)
        n = int(counts[0])
        if n < 2:
            raise ValueError(f"num_samples must be at least 2, got {n} live rows")
        mean = (sums[0] / n).float()  # what the reference subtracts: a float32 mean
        gram = torch.zeros((f, f), dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        bank._gram_rows(mean, rf, gram, count)
        return self._finish_fit(gram.cpu(), n, f, mean, dev)

    # ------------------------------------------------------------------ device placement
    def to(self, device: str | torch.device) -> "PCA":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.feature_means = self.feature_means.to(device)
        self.explained_variance = self.explained_variance.to(device)
        self.component_vectors = self.component_vectors.to(device)
        self._device = device
        self._packed = None
        return self

    @property
    def device(self) -> torch.device:
        return self._device

    def _kernel_operands(self) -> tuple[Tensor, Tensor]:
        """mean padded to a multiple of 32 features, components as [K padded to 4, F padded] rows (zeros in the
        padding, so padded inputs and outputs contribute nothing)."""
        if self._packed is None:
            f, k = self.num_features, self.num_components
            fpad, kpad = (f + 31) // 32 * 32, (k + 3) // 4 * 4
            mean = torch.zeros(fpad, dtype=torch.float32, device=self._device)
            mean[:f] = self.feature_means.reshape(-1).float()
            w = torch.zeros((kpad, fpad), dtype=torch.float32, device=self._device)
            w[:k, :f] = self.component_vectors.T.float()
            self._packed = (mean, w)
        return self._packed

    # ------------------------------------------------------------------ projection (device)
    def forward(self, x: Tensor) -> Tensor:
        """`(x - feature_means) @ component_vectors` (reference: decomposition.py:78-91)."""
        if not isinstance(x, Tensor) or not x.dtype.is_floating_point:
            raise TypeError("x must be a floating point tensor")
        if x.ndim != 2 or x.shape[1] != self.num_features:
            raise ValueError(f"x must have shape [num_samples, {self.num_features}], got {tuple(x.shape)}")
        _lib.require_device(x, "x")
        if self._device != x.device:
            raise ValueError(f"PCA is on {self._device} but the input is on {x.device}; call .to() first")
        n, f = x.shape
        k = self.num_components
        out_dtype = x.dtype
        mean, w = self._kernel_operands()
        fpad, kpad = w.shape[1], w.shape[0]
        xk = x.float()
        if fpad != f:
            xk = torch.nn.functional.pad(xk, (0, fpad - f))
        xk = xk.contiguous()
        out = torch.empty((n, kpad), dtype=torch.float32, device=x.device)
        if n > 0:
            lib = _lib.load()
            with torch.cuda.device(x.device):
                st = lib.isc_linear_centered(
                    xk.data_ptr(), n, fpad, mean.data_ptr(), w.data_ptr(), kpad, None, out.data_ptr(),
                    _lib.stream_handle(x.device),
                )
            _lib.check(st, "isc_linear_centered")
        return out[:, :k].to(out_dtype)

    def __call__(self, x: Tensor) -> Tensor:
        return self.forward(x)

    def transform(self, x: Tensor) -> Tensor:
        """Project the input data (reference: decomposition.py:150-165)."""
        if not self.fitted:
            raise RuntimeError("PCA model not fitted")
        return self(x)

    @property
    def fitted(self) -> bool:
        return self._fitted

    @property
    def num_features(self) -> int:
        return self._num_features

    @property
    def num_components(self) -> int:
        return self._num_components


class KMeans:
    """Spherical k-means over the rows of an `EmbeddingBank`: clusters by cosine similarity, centroids of unit length.

    Args:
        num_clusters: C >= 1.
        max_iter: most iterations (assignments) `fit` runs; the last one does not move the centroids.
        tol: `fit` stops when an update raises the objective by less than this.
        init: `"sample"` (C distinct live rows, drawn with a CPU generator seeded by `seed`), `"farthest"` (the rows of
            `bank.farthest_points(C, mask=...)`: spread out, deterministic, `seed` is ignored) or a `[C, D]` tensor that
            is used as given.
        seed: seed of the `"sample"` draw.

    After `fit`: `cluster_centers` (`[C, D]` float32 on the bank's device), `labels` (int32 `[len]`, -1 for removed or
    masked rows), `counts` (int64 `[C]`), `objective` (one float per iteration: the mean over the live rows of the winning
    score, before that iteration's update) and `num_iter`.
    """

    def __init__(self, num_clusters: int, *, max_iter: int = 25, tol: float = 1e-4,
                 init: "str | Tensor" = "sample", seed: int = 0) -> None:
        if isinstance(num_clusters, bool) or not isinstance(num_clusters, int) or num_clusters < 1:
            raise ValueError(f"num_clusters must be a positive int, got {num_clusters!r}")
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
            raise ValueError(f"max_iter must be a positive int, got {max_iter!r}")
        if not tol >= 0.0:
            raise ValueError(f"tol must be >= 0, got {tol!r}")
        if isinstance(init, str):
            if init not in ("sample", "farthest"):
                raise ValueError(f"init must be 'sample', 'farthest' or a [num_clusters, D] tensor, got {init!r}")
        elif not (isinstance(init, Tensor) and init.dtype.is_floating_point and init.ndim == 2
                  and init.shape[0] == num_clusters):
            raise ValueError(f"init must be 'sample', 'farthest' or a floating [{num_clusters}, D] tensor")
        self.num_clusters = num_clusters
        self.max_iter = max_iter
        self.tol = float(tol)
        self.init = init
        self.seed = int(seed)
        self.cluster_centers: Tensor | None = None
        self.labels: Tensor | None = None
        self.counts: Tensor | None = None
        self.objective: list[float] = []
        self.num_iter = 0

    def __repr__(self) -> str:
        return f"{type(self).__name__}(num_clusters={self.num_clusters}, num_iter={self.num_iter})"

    def _initial_centers(self, bank, live: Tensor, num_live: int, rf=None) -> Tensor:
        c = self.num_clusters
        if isinstance(self.init, Tensor):
            if self.init.shape[1] != bank.dim:
                raise ValueError(f"init must have shape [{c}, {bank.dim}], got {tuple(self.init.shape)}")
            return self.init.detach().to(device=bank.device, dtype=torch.float32).clone()
        if self.init == "farthest":  # (`fit` has checked that C live rows exist: every pick is a row)
            return bank.rows(bank.farthest_points(c, mask=rf)[0]).float()
        gen = torch.Generator().manual_seed(self.seed)
        pick = torch.randperm(num_live, generator=gen)[:c]  # distinct positions among the live rows
        rows = live.nonzero().squeeze(1).cpu()[pick] + bank.index_base
        return bank.rows(rows).float()

    def fit(self, bank, mask=None) -> "KMeans":
        """Cluster the live rows of `bank` (those `mask` allows, when given).  Per iteration: `assign` (labels only),
        `group_sums`, centroid = sum / ||sum|| in float64 (an empty cluster keeps its centroid), and the objective taken
        from the sums -- the winning score of a row is row . q_c / ||q_c||, so its sum over a cluster is sum_c . q_c /
        ||q_c|| -- with ONE host read.  Stops when no label changed, when the objective rose by less than `tol`, or after
        `max_iter` iterations.  ValueError for fewer live rows than clusters and for a sharded bank."""
        if bank.process_group is not None:
            raise ValueError("a sharded bank (process_group=) cannot be clustered: " + bank._ROWS_ON_ONE_RANK)
        rf = bank._as_filter(mask)
        c = self.num_clusters
        live = bank.live if rf is None or rf.packed is bank._fill else bank._unpack_mask(rf.packed, len(bank))
        num_live = int(live.sum())
        if num_live < c:
            raise ValueError(f"{c} clusters need at least {c} live rows, the bank has {num_live}")
        centers = self._initial_centers(bank, live, num_live, rf)
        self.objective = []
        labels = None
        for it in range(self.max_iter):
            new_labels, _ = bank.assign(centers, mask=rf, return_scores=False)
            sums, counts = bank.group_sums(new_labels, c)
            q = centers.to(bank.dtype).double()  # the centroids as `assign` scored them
            qn = q.norm(dim=1).clamp_min(1e-12)
            obj = ((sums * q).sum(dim=1) / qn).sum() / num_live
            changed = (new_labels != labels).any() if labels is not None else torch.ones((), dtype=torch.bool,
                                                                                          device=new_labels.device)
            obj_host, changed_host = torch.stack([obj, changed.double()]).tolist()  # the iteration's one host read
            labels = new_labels
            self.labels, self.counts = labels, counts
            self.objective.append(obj_host)
            self.num_iter = it + 1
            if not changed_host:
                break
            if it > 0 and obj_host - self.objective[-2] < self.tol:
                break
            if it + 1 == self.max_iter:  # no update without an assignment behind it: `labels` belong to `cluster_centers`
                break
            norm = sums.norm(dim=1, keepdim=True)
            keep = (counts == 0)[:, None] | ~(norm > 0)
            centers = torch.where(keep, centers.double(), sums / norm.clamp_min(1e-300)).float()
        self.cluster_centers = centers
        return self

    def predict(self, bank) -> Tensor:
        """The label of every row of `bank` under the fitted centroids: `bank.assign(cluster_centers)` labels."""
        if self.cluster_centers is None:
            raise RuntimeError("KMeans model not fitted")
        return bank.assign(self.cluster_centers, return_scores=False)[0]
