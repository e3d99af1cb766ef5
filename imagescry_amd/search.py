"""Brute-force cosine top-k over an embedding bank resident in HBM.

The reference stores embeddings as SQLite BLOB rows (src/imagescry/storage/models.py:73-129) and reads them
back with `get_embeddings_by_image_id` (src/imagescry/storage/operations.py:108-144); it has no search step
(SURVEY.md section 0 fact 2).  `EmbeddingBank` is the storage-flavoured object BASELINE.json's `north_star`
asks for: it keeps the `[N, D]` bank on the GPU and answers `search(queries, k)`.

Semantics (pinned by oracle/search_oracle.py, not by the reference):
`score = float32(dot_f64(q, b) / max(||q||, 1e-12))`, bank rows used as stored (L2-normalised once at build
time with the `F.normalize` formula of src/imagescry/models/embedding.py:74), results ordered by
(score descending, row index ascending).  Row ids are positions in the bank, the analogue of the reference's
DB row order (operations.py:135-144).

The matrix-core pass is a float32 filter; the candidates are re-scored in float64, a rounding-error guard proves per
query that the filter lost nothing, and what it cannot prove is searched again exactly on the device -- one call, no
host synchronisation, the result is final (csrc/cosine_topk.hip).  The bank is stored in a fixed pseudo-random row
order (`isc_bank_permutation`), so banks whose rows arrive sorted or clustered -- the reference's store returns all
cells of one image adjacent, operations.py:135-144 -- behave like shuffled ones; indices are always original rows.

Multi-GPU: one process per GPU.  The bank is row-sharded -- rank r holds rows `[r*N//G, (r+1)*N//G)` -- every
rank searches its shard with the replicated queries, one all-gather (RCCL over xGMI) exchanges the
`Q x k x 12 B` partial results and every rank merges them; the merge order is total, so the answer does not
depend on G.  The exchange is software-pipelined: the local search runs on the caller's stream, the all-gather and
the merge on the bank's own exchange stream (ordered by events, two exchange buffers), and `search_async` returns as
soon as the merge is enqueued -- in a stream of searches the exchange of search i runs under the local kernels of
search i + 1.
"""

from __future__ import annotations

import math
import weakref
from contextlib import nullcontext
from dataclasses import dataclass
from os import PathLike
from typing import Sequence

import torch
import torch.distributed as dist
from torch import Tensor

from imagescry_amd import _lib, segmentation
from imagescry_amd.data import EmbeddingBatch

__all__ = ["EmbeddingBank", "RangeResult", "RowFilter", "SearchHandle", "shard_bounds"]

_PAD_INDEX = torch.iinfo(torch.int64).max


def shard_bounds(n_rows: int, world_size: int, rank: int) -> tuple[int, int]:
    """Contiguous row range `[lo, hi)` of `rank` when `n_rows` are split over `world_size` ranks."""
    if world_size <= 0 or not 0 <= rank < world_size:
        raise ValueError(f"invalid rank {rank} for world size {world_size}")
    return rank * n_rows // world_size, (rank + 1) * n_rows // world_size


# The two streams asynchronous searches alternate between, per DEVICE and shared by every bank on it: the runtime maps
# streams onto a handful of hardware queues, and streams that share a queue wait for each other -- with a pair per bank, a
# process holding two banks ran its searches slower asynchronously than serially (0.366 against 0.321 ms at a 1.25 M-row
# shard).
_LANE_STREAMS: dict[int, tuple["torch.cuda.Stream", "torch.cuda.Stream"]] = {}


def _lane_streams(device: torch.device) -> tuple["torch.cuda.Stream", "torch.cuda.Stream"]:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    pair = _LANE_STREAMS.get(idx)
    if pair is None:
        pair = (torch.cuda.Stream(device), torch.cuda.Stream(device))
        _LANE_STREAMS[idx] = pair
    return pair


class SearchHandle:
    """Result of `EmbeddingBank.search_async`.  The tensors exist at once; their CONTENTS are final when the event
    recorded behind the merge has fired.  `result()` orders the caller's current stream behind that event (no host
    synchronisation) and returns `(scores, indices)`."""

    __slots__ = ("_scores", "_indices", "_event", "gathered_status")

    def __init__(self, scores: Tensor, indices: Tensor, event: "torch.cuda.Event | None" = None,
                 gathered_status: Tensor | None = None) -> None:
        self._scores = scores
        self._indices = indices
        self._event = event
        # [G, 4] diagnostics of every shard: a view into the gathered exchange buffers, which it keeps alive (they were
        # allocated on the exchange stream and are read only there, so nothing else has to hold them)
        self.gathered_status = gathered_status

    def result(self) -> tuple[Tensor, Tensor]:
        """May be called more than once and from different streams: EVERY call orders the then-current stream behind the
        answer and tells the allocator about that stream (events are cheap; a stream already ordered waits for nothing)."""
        if self._event is not None:
            cur = torch.cuda.current_stream(self._scores.device)
            cur.wait_event(self._event)
            for t in (self._scores, self._indices, self.gathered_status):  # allocated on another stream, used on this one
                if t is not None:
                    t.record_stream(cur)
        return self._scores, self._indices


@dataclass
class RangeResult:
    """Result of `EmbeddingBank.search_range`: query q's rows are `scores[offsets[q]:offsets[q + 1]]` /
    `indices[...]`, ordered by (score descending, row index ascending).  All three tensors live on the bank's device."""

    offsets: Tensor  # int64 [Q + 1]
    scores: Tensor  # float32 [M]
    indices: Tensor  # int64 [M]

    def __len__(self) -> int:
        return self.offsets.shape[0] - 1

    @property
    def counts(self) -> Tensor:
        """int64 [Q]: rows per query."""
        return self.offsets[1:] - self.offsets[:-1]

    def __getitem__(self, q: int) -> tuple[Tensor, Tensor]:
        n = len(self)
        if not -n <= q < n:
            raise IndexError(f"query {q} out of range for {n} queries")
        q %= n
        lo, hi = (int(v) for v in self.offsets[q : q + 2].tolist())
        return self.scores[lo:hi], self.indices[lo:hi]


def _unpad(scores: Tensor, indices: Tensor) -> tuple[Tensor, Tensor]:
    """The public form of a masked top-k: the C ABI's padding (score NaN, index INT64_MAX) becomes (-inf, -1)."""
    pad = indices == _PAD_INDEX
    return scores.masked_fill(pad, -math.inf), indices.masked_fill(pad, -1)


def _unpad_groups(scores: Tensor, indices: Tensor, labels: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """The public form of a collapsed top-k: the padding (NaN, INT64_MAX, label -1) becomes (-inf, -1, -1)."""
    pad = indices == _PAD_INDEX
    return scores.masked_fill(pad, -math.inf), indices.masked_fill(pad, -1), labels.masked_fill(pad, -1)


def _check_labels(labels: object, name: str, n: int, shape: str, got: bool = False) -> None:
    """`labels` must be an integer tensor of shape `[n]`; `shape` is how the message words that, and `got` says whether
    the type errors name what came instead."""
    if not isinstance(labels, Tensor):
        raise TypeError(f"{name} must be an integer torch.Tensor" + (f", got {type(labels).__name__}" if got else ""))
    dt = labels.dtype
    if dt.is_floating_point or dt.is_complex or dt == torch.bool:
        raise TypeError(f"{name} must be an integer tensor, got {dt}" if got else f"{name} must be an integer torch.Tensor")
    if labels.shape != (n,):
        raise ValueError(f"{name} must have shape {shape}, got {tuple(labels.shape)}")


def _exchange_layout(nq: int, k: int, with_labels: bool = False):
    """The exchange buffer of a sharded search, `[scores f32 Q*k | pad to 8 | indices i64 Q*k | (labels i64 Q*k) | status
    i32 x4]`: its size in bytes and `views(buf)`, the `(scores, indices, (labels,) status)` planes of one rank's uint8
    `[nbytes]` buffer (`[Q, k]` each, status `[4]`) or of the all-gathered `[G, nbytes]` one (`[G, Q, k]`, `[G, 4]`).  The
    search kernels write the planes in place, ONE collective gathers them and the merge kernel reads them in place."""
    n = nq * k
    off_i = (4 * n + 7) // 8 * 8
    off_s = off_i + (16 if with_labels else 8) * n

    def views(buf: Tensor) -> tuple[Tensor, ...]:
        lead = buf.shape[:-1]
        planes = [buf[..., : 4 * n].view(torch.float32).view(*lead, nq, k)]
        for lo in (off_i, off_i + 8 * n)[: 2 if with_labels else 1]:
            planes.append(buf[..., lo : lo + 8 * n].view(torch.int64).view(*lead, nq, k))
        return (*planes, buf[..., off_s:].view(torch.int32))

    return off_s + 16, views


class RowFilter:
    """A set of allowed rows of ONE bank, made by `EmbeddingBank.row_filter`: the bitmap of this rank's rows in the bank's
    packed row order (`isc_row_mask_pack`) and the number of rows it allows (int64 [1], device).  Searches given it as
    `mask=` answer as if the bank held the allowed rows only, with their indices in the whole bank.  A filter describes
    the bank as it was when the filter was made: after `EmbeddingBank.append`, `reserve`, `remove`, `replace` or `compact`
    it is refused."""

    __slots__ = ("packed", "allowed_count", "_bank", "_revision")

    def __init__(self, bank: "EmbeddingBank", packed: Tensor, allowed_count: Tensor | None) -> None:
        self.packed = packed  # int32 [isc_row_mask_words(capacity)] (uint32 bit patterns); empty for a shard with no row
        self.allowed_count = allowed_count
        self._bank = weakref.ref(bank)
        self._revision = bank._revision

    def belongs_to(self, bank: "EmbeddingBank") -> bool:
        return self._bank() is bank


class _ExchangeSlot:
    """One of the two exchange buffers of a sharded bank and the event behind the last exchange that read it."""

    __slots__ = ("buf", "done")

    def __init__(self) -> None:
        self.buf: Tensor | None = None
        self.done: "torch.cuda.Event | None" = None


class EmbeddingBank:
    """`[N, D]` embedding bank on one GPU (or one row shard of it per rank) with cosine top-k search.

    Args:
        embeddings: floating `[N, D]` tensor on a HIP device.  With `process_group` set and
            `presharded=False` it is the FULL bank (identical on every rank) and this rank keeps only its
            rows; with `presharded=True` it is this rank's shard and `index_base` is the global index of
            its first row.
        dtype: storage dtype of the bank, `torch.float16` (default) or `torch.float32`.
        normalize: L2-normalise every row before storing it (skip for rows that are already unit length,
            e.g. the output of `Embedder.predict_step`).
        index_base: global row index of local row 0 (only with `presharded=True`).
        process_group: the `torch.distributed` group the bank is sharded over (`None` = single GPU).
        row_groups: optional integer group label of every row (e.g. its image id), sharded like `embeddings`: the full
            `[N]` with `presharded=False`, the shard's `[N_local]` with `presharded=True`.  Searches given
            `exclude_group=` labels per query then skip, for each query, the rows that carry its label.
        capacity: lay the packed image out for this many rows (>= N; `embeddings` may then be `[0, D]`): `append` adds rows
            in place, one launch each, until the capacity is used up.  `None` (default): no room is reserved.
    """

    # An appendable bank (`capacity=`, `reserve`, `append`): the row count the packed image is laid out for (None: the
    # number of rows, nothing reserved), the bitmap of the filled packed positions (isc_row_mask_words(capacity) words, the
    # `mask` of every search while capacity > len) and the counter stale `RowFilter`s are told by.  Class-level defaults:
    # a bank that never reserves carries none of it.
    _capacity: int | None = None
    _fill: Tensor | None = None
    _fill_filter: RowFilter | None = None
    _group_counts: Tensor | None = None
    _revision = 0
    # the rows `remove` took out and `compact` has not closed up yet: their fill bits are 0, their indices stay reserved
    _num_removed = 0
    _GROW_BLOCK = 1 << 20  # rows per isc_bank_pack / isc_bank_append / isc_bank_repack launch
    _n_total: int | None = None  # rows of the whole sharded bank, learnt by `_global_rows`

    def __init__(
        self,
        embeddings: Tensor,
        *,
        dtype: torch.dtype = torch.float16,
        normalize: bool = True,
        index_base: int = 0,
        process_group: dist.ProcessGroup | None = None,
        presharded: bool = False,
        row_groups: Tensor | None = None,
        capacity: int | None = None,
        shadow: bool = True,
    ) -> None:
        if not isinstance(embeddings, Tensor) or not embeddings.dtype.is_floating_point:
            raise TypeError("embeddings must be a floating point torch.Tensor")
        if embeddings.ndim != 2:
            raise ValueError(f"embeddings must have shape [N, D], got {tuple(embeddings.shape)}")
        if dtype not in (torch.float16, torch.float32):
            raise ValueError(f"bank dtype must be float16 or float32, got {dtype}")
        self.process_group = process_group
        self.world_size = dist.get_world_size(process_group) if process_group is not None else 1
        self.rank = dist.get_rank(process_group) if process_group is not None else 0
        if row_groups is not None:
            n = embeddings.shape[0]
            _check_labels(row_groups, "row_groups", n, f"[{n}] (one label per row of embeddings)")
        if process_group is not None and not presharded:
            lo, hi = shard_bounds(embeddings.shape[0], self.world_size, self.rank)
            embeddings = embeddings[lo:hi]
            if row_groups is not None:
                row_groups = row_groups[lo:hi]
            index_base = lo
        elif process_group is None and index_base != 0 and not presharded:
            raise ValueError("index_base is only meaningful for a presharded bank")
        self.index_base = int(index_base)
        self.presharded = bool(presharded)
        self.dtype = dtype
        self.dim = int(embeddings.shape[1])
        self.num_local_rows = int(embeddings.shape[0])
        if self.dim == 0:
            raise ValueError("embedding dimension must be positive")
        self.normalize = bool(normalize)
        # int8 shadow of an fp16 bank (`isc_bank_quantize`, +50 % of the bank's memory): built at the first plain search
        # whose plan uses it (more than 256 queries on a bank of millions of rows), dropped by whatever changes the image
        self.shadow = bool(shadow)
        self._shadow: Tensor | None = None
        if capacity is None:
            self._bank = self._store(embeddings, normalize)
        else:
            self._check_capacity(capacity)
            self._norm_bound = torch.zeros(1, dtype=torch.float32, device=embeddings.device)
            self._capacity = capacity
            self._bank, self._fill, _ = self._alloc_image(capacity, embeddings.device, False)
            self._fill_filter = RowFilter(self, self._fill, None)
            self._append_rows(embeddings, 0, normalize, None)
        # search workspaces per LANE: -1 = the caller's stream (`search`), 0 / 1 = the two streams `search_async` alternates
        # between -- two searches in flight must not share a workspace
        self._workspaces: dict[int, dict[tuple[int, int], Tensor]] = {}
        # workspaces a stream capture has seen (`_workspace`): a captured graph replays into them, so they live as long as
        # the bank whatever the bucket cache drops
        self._captured_workspaces: list[Tensor] = []
        self._lane_next = 0
        self._slots = (_ExchangeSlot(), _ExchangeSlot())
        self._slot_next = 0
        self._xstream: "torch.cuda.Stream | None" = None
        self.last_status: Tensor | None = None
        self.last_range_status: Tensor | None = None
        self._range_ws: Tensor | None = None  # the range search's workspace, grown on demand
        self.last_gathered_status: Tensor | None = None
        self.row_origin: Tensor | None = None  # set by from_database: (image_id, h, w) of every row
        # row groups (`row_groups`): this rank's sorted distinct labels (int64 [G], device) and the int32 code -- the label's
        # position among them -- of every row in the PACKED row order (`isc_row_groups_pack`)
        self.group_labels: Tensor | None = None
        self._row_codes: Tensor | None = None
        # the most rows one group of this rank holds: the collapsed search (`search_groups`) sizes its levels with it,
        # so it is taken here, once, rather than with a host synchronisation per search
        self._max_group_rows = 0
        if row_groups is not None:
            labels = row_groups.to(device=self.device, dtype=torch.int64)
            self.group_labels, codes, counts = torch.unique(labels, sorted=True, return_inverse=True, return_counts=True)
            self._max_group_rows = int(counts.max()) if counts.numel() else 0
            self._group_counts = counts
            self._row_codes = self._pack_groups(codes.to(torch.int32).contiguous())

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_batches(cls, batches: Sequence[EmbeddingBatch], **kwargs: object) -> "EmbeddingBank":
        """Bank whose rows are `get_flat_vectors()` of every batch, in order (reference: data.py:112-118).

        `predict_step` output is already L2-normalised per location, so `normalize` defaults to False here.
        """
        if len(batches) == 0:
            raise ValueError("need at least one EmbeddingBatch")
        rows = torch.cat([b.get_flat_vectors() for b in batches], dim=0)
        kwargs.setdefault("normalize", False)
        return cls(rows, **kwargs)  # type: ignore[arg-type]

    @classmethod
    def from_database(
        cls,
        db: "str | PathLike",
        *,
        device: str | torch.device = "cuda",
        image_ids: Sequence[int] | None = None,
        **kwargs: object,
    ) -> "EmbeddingBank":
        """Bank built from the reference's SQLite store (`<dir>/imagescry.db`, table `embeddings`): every spatial
        location of every stored `[C, H, W]` map becomes one row, in (record, h, w) order.  `row_origin`
        (`int64 [N, 3]` = image_id, h, w) maps result indices back to images.  Stored maps are PCA-compressed,
        i.e. not unit length, so rows are L2-normalised unless `normalize=False` is passed.
        (reference format: storage/models.py:73-129; read order: storage/operations.py:108-144)"""
        from imagescry_amd import storage

        rows, origin = storage.flat_rows(storage.read_embeddings(db, image_ids=image_ids))
        kwargs.setdefault("row_groups", origin[:, 0])  # grouped by image: exclude_group= takes image ids
        bank = cls(rows.to(device), **kwargs)  # type: ignore[arg-type]
        bank.row_origin = origin
        return bank

    def _store(self, embeddings: Tensor, normalize: bool) -> Tensor:
        """Row-normalise / cast the rows and write them into the PACKED bank image (`isc_bank_pack`):
        `[tile of 256 rows][K step][row][128 B]`, rows permuted, the layout the search kernels stream
        (include/imagescry_hip.h).  `_norm_bound` receives an upper bound of the stored rows' norms (the search's
        rounding guard needs it)."""
        _lib.require_device(embeddings, "embeddings")
        n, d = embeddings.shape
        lib = _lib.load()
        code = _lib.dtype_code(self.dtype)
        self._norm_bound = torch.zeros(1, dtype=torch.float32, device=embeddings.device)
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=embeddings.device)
        need = _lib.c_size_t()
        _lib.check(lib.isc_bank_packed_bytes(code, n, d, need), "isc_bank_packed_bytes")
        packed = torch.empty(need.value, dtype=torch.uint8, device=embeddings.device)
        tile_bytes = need.value // ((n + 255) // 256)
        packed[-tile_bytes:].zero_()  # padding rows of the last tile (isc_bank_pack writes real rows only)
        with torch.cuda.device(embeddings.device):
            for r0, rows in self._row_blocks(embeddings):
                st = lib.isc_bank_pack(
                    rows.data_ptr(), _lib.dtype_code(rows.dtype), rows.shape[0], d, rows.stride(0), r0, n,
                    int(normalize), 1e-12, packed.data_ptr(), code, self._norm_bound.data_ptr(),
                    _lib.stream_handle(embeddings.device),
                )
                _lib.check(st, "isc_bank_pack")
        return packed

    def _row_blocks(self, embeddings: Tensor):
        """`(r0, rows)` for every `_GROW_BLOCK` rows of `embeddings` from row `r0` on, float16 or float32 with unit inner
        stride: the input of one `isc_bank_pack` / `isc_bank_append` launch."""
        if embeddings.dtype not in (torch.float16, torch.float32):
            embeddings = embeddings.float()
        for r0 in range(0, embeddings.shape[0], self._GROW_BLOCK):
            rows = embeddings[r0 : r0 + self._GROW_BLOCK]
            yield r0, rows if rows.stride(1) == 1 else rows.contiguous()

    # ------------------------------------------------------------------ reserved capacity and append
    def _check_capacity(self, capacity: object) -> None:
        if not isinstance(capacity, int) or isinstance(capacity, bool):
            raise TypeError(f"capacity must be an int, got {type(capacity).__name__}")
        if capacity < max(self.num_local_rows, 1):
            raise ValueError(f"capacity={capacity} must be at least the bank's {self.num_local_rows} rows (and positive)")
        if capacity > 0x7FFFFFFE:
            raise ValueError(f"capacity={capacity} exceeds the packed layout's limit of {0x7FFFFFFE} rows")
        if self.process_group is not None:
            raise ValueError("a sharded bank (process_group=) cannot reserve capacity or append: its global indices are "
                             "contiguous per rank and would shift")

    def _alloc_image(self, capacity: int, device: torch.device, grouped: bool) -> tuple[Tensor, Tensor, Tensor | None]:
        """The empty image of a `capacity`-row bank: (packed rows, all zero; fill bitmap, all zero; packed group codes, all
        -2, when `grouped`).  A device hook, like `_store`."""
        lib = _lib.load()
        need, words = _lib.c_size_t(), _lib.c_size_t()
        _lib.check(lib.isc_bank_packed_bytes(_lib.dtype_code(self.dtype), capacity, self.dim, need), "isc_bank_packed_bytes")
        _lib.check(lib.isc_row_mask_words(capacity, words), "isc_row_mask_words")
        packed = torch.zeros(need.value, dtype=torch.uint8, device=device)
        fill = torch.zeros(words.value, dtype=torch.int32, device=device)
        codes = torch.full(((capacity + 255) // 256 * 256,), -2, dtype=torch.int32, device=device) if grouped else None
        return packed, fill, codes

    def _append_rows(self, embeddings: Tensor, first_row: int, normalize: bool, codes: Tensor | None) -> None:
        """`isc_bank_append` of `embeddings` as rows `[first_row, first_row + m)` of the image laid out for `capacity` rows
        (one launch per 2^20 rows, on the current stream): the rows, their fill bits and -- `codes`: int32 `[m]` -- their
        group codes.  A device hook."""
        _lib.require_device(embeddings, "embeddings")
        d = embeddings.shape[1]
        lib = _lib.load()
        with torch.cuda.device(embeddings.device):
            for r0, rows in self._row_blocks(embeddings):
                cs = None if codes is None else codes[r0 : r0 + self._GROW_BLOCK]
                st = lib.isc_bank_append(
                    rows.data_ptr(), _lib.dtype_code(rows.dtype), rows.shape[0], d, rows.stride(0), first_row + r0,
                    self.capacity, int(normalize), 1e-12, self._bank.data_ptr(), _lib.dtype_code(self.dtype),
                    self._norm_bound.data_ptr(), self._fill.data_ptr(), _lib.ptr(cs),
                    None if cs is None else self._row_codes.data_ptr(), _lib.stream_handle(embeddings.device),
                )
                _lib.check(st, "isc_bank_append")

    def _repack_rows(self, src: Tensor, src_capacity: int, src_codes: Tensor | None, dst: Tensor, dst_capacity: int,
                     dst_codes: Tensor | None, dst_fill: Tensor) -> None:
        """`isc_bank_repack` of every row of the bank from the image laid out for `src_capacity` rows into the (empty) one
        laid out for `dst_capacity`, in blocks of 2^20 rows.  A device hook."""
        lib = _lib.load()
        with torch.cuda.device(dst.device):
            for r0 in range(0, self.num_local_rows, self._GROW_BLOCK):
                st = lib.isc_bank_repack(
                    src.data_ptr(), src_capacity, dst.data_ptr(), dst_capacity, _lib.dtype_code(self.dtype), self.dim, r0,
                    min(self._GROW_BLOCK, self.num_local_rows - r0), _lib.ptr(src_codes), _lib.ptr(dst_codes),
                    dst_fill.data_ptr(), _lib.stream_handle(dst.device),
                )
                _lib.check(st, "isc_bank_repack")

    def _repack_map(self, src: Tensor, src_capacity: int, src_codes: Tensor | None, dst: Tensor, dst_capacity: int,
                    dst_codes: Tensor | None, dst_fill: Tensor, new_index: Tensor) -> None:
        """`isc_bank_repack_map`: `_repack_rows` with row r landing at row `new_index[r]` (int64 `[len]`, device) of the
        destination, a negative entry moving nothing.  A device hook."""
        lib = _lib.load()
        with torch.cuda.device(dst.device):
            for r0 in range(0, self.num_local_rows, self._GROW_BLOCK):
                st = lib.isc_bank_repack_map(
                    src.data_ptr(), src_capacity, dst.data_ptr(), dst_capacity, _lib.dtype_code(self.dtype), self.dim, r0,
                    min(self._GROW_BLOCK, self.num_local_rows - r0), _lib.ptr(src_codes), _lib.ptr(dst_codes),
                    dst_fill.data_ptr(), new_index.data_ptr(), _lib.stream_handle(dst.device),
                )
                _lib.check(st, "isc_bank_repack_map")

    def _remove_rows(self, index: Tensor, removed: Tensor) -> None:
        """`isc_bank_remove` of the local rows `index` (int64 `[m]`, device, m > 0), one launch on the current stream: their
        fill bits are cleared, their group codes become -2, `_group_counts` goes down, and the number of rows that were
        still there is added to `removed` (int64 `[1]`, device).  A device hook."""
        with torch.cuda.device(self.device):
            st = _lib.load().isc_bank_remove(
                index.data_ptr(), index.numel(), self.num_local_rows, self.capacity, self._fill.data_ptr(),
                _lib.ptr(self._row_codes), _lib.ptr(self._group_counts if self._row_codes is not None else None),
                removed.data_ptr(), _lib.stream_handle(self.device),
            )
        _lib.check(st, "isc_bank_remove")

    def _replace_rows(self, embeddings: Tensor, index: Tensor, normalize: bool) -> None:
        """`isc_bank_replace`: `embeddings[i]` is stored at local row `index[i]` (int64 `[m]`, device, distinct) unless that
        row is removed; one launch per 2^20 rows on the current stream.  A device hook."""
        _lib.require_device(embeddings, "rows")
        lib = _lib.load()
        with torch.cuda.device(self.device):
            for r0, rows in self._row_blocks(embeddings):
                st = lib.isc_bank_replace(
                    rows.data_ptr(), _lib.dtype_code(rows.dtype), rows.shape[0], self.dim, rows.stride(0),
                    index[r0 : r0 + self._GROW_BLOCK].data_ptr(), self.capacity, int(normalize), 1e-12,
                    self._bank.data_ptr(), _lib.dtype_code(self.dtype), self._norm_bound.data_ptr(), _lib.ptr(self._fill),
                    _lib.stream_handle(self.device),
                )
                _lib.check(st, "isc_bank_replace")

    def _unpack_mask(self, packed: Tensor, n_rows: int) -> Tensor:
        """`isc_row_mask_unpack`: bool `[n_rows]`, the bits of the first `n_rows > 0` rows of a bitmap in this bank's packed
        row order.  A device hook."""
        allow = torch.empty(n_rows, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            st = _lib.load().isc_row_mask_unpack(packed.data_ptr(), self.capacity, n_rows, allow.data_ptr(),
                                                 _lib.stream_handle(self.device))
        _lib.check(st, "isc_row_mask_unpack")
        return allow.view(torch.bool)

    def _code_rows(self, codes: Tensor) -> Tensor:
        """The local rows (int64, device, any order) whose stored group code is one of `codes` (int32, >= 0): tensor ops on
        the packed codes, position p holding row `(mul * p) mod capacity`.  A device hook."""
        mul, inv = _lib.c_int64(), _lib.c_int64()
        _lib.check(_lib.load().isc_bank_permutation(self.capacity, mul, inv), "isc_bank_permutation")
        pos = torch.isin(self._row_codes, codes).nonzero().squeeze(1)
        return (pos * mul.value) % self.capacity

    def _stored_codes(self, index: Tensor) -> Tensor:
        """The stored int32 group codes of the local rows `index` (int64 `[m]`, device), read from the packed codes at the
        rows' packed positions `(mul_inv * row) mod capacity`: tensor ops, no label lookup, no host read.  A device hook."""
        mul, inv = _lib.c_int64(), _lib.c_int64()
        _lib.check(_lib.load().isc_bank_permutation(self.capacity, mul, inv), "isc_bank_permutation")
        return self._row_codes[(index * inv.value) % self.capacity]

    def _gather_rows(self, index: Tensor, out: Tensor) -> None:
        """`isc_bank_gather`: `out[i]` (`[m, D]` of the bank dtype, unit inner stride) receives the stored bytes of local
        row `index[i]` (int64 `[m]`, device, m > 0), zeros for a removed row; one launch on the current stream, no host
        read.  A device hook."""
        with torch.cuda.device(self.device):
            st = _lib.load().isc_bank_gather(
                self._bank.data_ptr(), _lib.dtype_code(self.dtype), self.dim, self.capacity, index.data_ptr(),
                index.numel(), _lib.ptr(self._fill), out.data_ptr(), out.stride(0), _lib.stream_handle(self.device),
            )
        _lib.check(st, "isc_bank_gather")

    def _score_rows(self, q: Tensor, index: Tensor, out: Tensor) -> None:
        """`isc_cosine_scores`: `out[i, j]` (float32 `[Q, M]`, unit inner stride) receives the score of query `q[i]`
        (prepared, Q > 0) against local row `index[j]` (int64 `[M]`, device, M > 0), -inf for a removed row; one launch on
        the current stream, no host read.  A device hook."""
        with torch.cuda.device(self.device):
            st = _lib.load().isc_cosine_scores(
                self._bank.data_ptr(), _lib.dtype_code(self.dtype), self.capacity, self.dim, q.data_ptr(),
                _lib.dtype_code(q.dtype), q.shape[0], q.stride(0), index.data_ptr(), index.numel(), _lib.ptr(self._fill),
                out.data_ptr(), out.stride(0), _lib.stream_handle(self.device),
            )
        _lib.check(st, "isc_cosine_scores")

    def _wait_for_issued(self) -> None:
        """Order the caller's current stream behind everything this bank has issued elsewhere: both lane streams of
        `search_async` and the exchange stream.  An unresolved asynchronous search then never reads a half-updated image."""
        if self.device.type != "cuda":
            return
        cur = torch.cuda.current_stream(self.device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        for stream in (*_LANE_STREAMS.get(idx, ()), self._xstream):
            if stream is not None:
                issued = torch.cuda.Event()
                issued.record(stream)
                cur.wait_event(issued)

    def _relayout(self, capacity: int, new_index: Tensor | None = None) -> None:
        """Move the bank into a fresh image laid out for `capacity` rows (`isc_bank_repack`).  `new_index` (int64 `[len]`,
        -1: the row stays behind): the rows move through it (`isc_bank_repack_map`); a bank with removed rows always moves
        that way, so a growth neither moves nor revives them."""
        old = (self._bank, self._fill, self._row_codes)
        if new_index is None and self._num_removed:
            new_index = torch.where(self.live, torch.arange(self.num_local_rows, device=self.device), -1)
        packed, fill, codes = self._alloc_image(capacity, self.device, self.group_labels is not None)
        if self.num_local_rows and new_index is None:
            self._repack_rows(self._bank, self.capacity, self._row_codes, packed, capacity, codes, fill)
        elif self.num_local_rows:
            self._repack_map(self._bank, self.capacity, self._row_codes, packed, capacity, codes, fill, new_index)
        if self._captured_workspaces:
            # a graph captured before the growth still holds the old pointers: a stale replay must read stale memory,
            # never memory the allocator has handed to somebody else
            self.__dict__.setdefault("_retired", []).append(old)
        self._bank, self._fill, self._capacity = packed, fill, capacity
        if self.group_labels is not None:
            self._row_codes = codes
        self._shadow = None
        # sized by the image's row count
        self._workspaces = {}
        self._range_ws = None

    def reserve(self, capacity: int) -> None:
        """Lay the packed image out for `capacity >= len(self)` rows, so that `append` up to it works in place.  A no-op
        when the image already holds that many; otherwise the rows move into a new image (`isc_bank_repack`: peak memory is
        the old image plus the new one), which invalidates graphs captured on this bank.  `RowFilter`s made before the
        call are refused afterwards."""
        self._check_capacity(capacity)
        if self._fill is None or capacity > self.capacity:
            self._wait_for_issued()
            self._relayout(capacity)
        self._shadow = None
        self._revision += 1
        self._fill_filter = RowFilter(self, self._fill, None)

    def append(self, rows: Tensor, *, row_groups: Tensor | None = None, row_origin: Tensor | None = None,
               normalize: bool | None = None) -> range:
        """Add `rows` (floating `[m, D]`, on the bank's device) to the bank and return the global indices they received,
        `range(index_base + len_before, index_base + len_after)`.  Searches issued afterwards see them.

        Within the reserved capacity (`capacity=`, `reserve`) this is ONE launch that touches only the new rows
        (`isc_bank_append`): the packed image, the fill bitmap and the norm bound are updated in place, no pointer and no
        size changes, so a `search` captured into a graph before the append replays over the new rows.  The bank then
        equals, bit for bit in every search, the bank built from all the rows at once: it is that bank's rows in an image
        laid out for `capacity` rows, searched through the bitmap of the filled positions.

        Past the capacity the bank first grows to `max(2 * capacity, len + m)` rows: every row moves into a new image
        (`isc_bank_repack`, byte for byte).  Peak memory during a growth is the old image plus the new one.  A growth
        invalidates graphs captured on this bank (a bank that has seen a capture keeps the old image alive, so a stale
        replay reads stale rows, not freed memory) and drops the cached search workspaces.

        `row_groups` (integer `[m]`) is required iff the bank has row groups, `row_origin` (`[m, 3]`) iff it has one;
        `normalize` defaults to the bank's own setting.  Labels not seen before are merged into the sorted `group_labels`
        (the stored codes are re-mapped on the device; a grouped append reads one group count back to the host).

        Runs on the caller's current stream, ordered behind everything the bank has issued on its own streams
        (unresolved `search_async` handles see the bank as it was).  `RowFilter`s made before the call are refused
        afterwards: make them again.  A sharded bank (`process_group=`) cannot append."""
        if self.process_group is not None:
            raise ValueError("a sharded bank (process_group=) cannot append: its global indices are contiguous per rank "
                             "and would shift")
        if not isinstance(rows, Tensor) or not rows.dtype.is_floating_point:
            raise TypeError("rows must be a floating point torch.Tensor")
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must have shape [m, {self.dim}], got {tuple(rows.shape)}")
        if rows.device != self.device:
            raise ValueError(f"rows are on {rows.device} but the bank is on {self.device}")
        m = int(rows.shape[0])
        if (row_groups is not None) != (self.group_labels is not None):
            raise ValueError("row_groups must be given iff the bank was built with row groups")
        if row_groups is not None:
            _check_labels(row_groups, "row_groups", m, f"[{m}] (one label per row)")
        if (row_origin is not None) != (self.row_origin is not None):
            raise ValueError("row_origin must be given iff the bank has one (EmbeddingBank.from_database)")
        if row_origin is not None and (not isinstance(row_origin, Tensor) or row_origin.shape != (m, 3)):
            raise ValueError(f"row_origin must be a tensor of shape [{m}, 3] (image_id, h, w)")
        first = self.num_local_rows
        if m == 0:
            return range(self.index_base + first, self.index_base + first)
        if first + m > 0x7FFFFFFE:
            raise ValueError(f"{first + m} rows exceed the packed layout's limit of {0x7FFFFFFE}")
        self._wait_for_issued()
        if self._fill is None or first + m > self.capacity:
            self._relayout(max(2 * self.capacity, first + m))
        codes = None
        if row_groups is not None:
            codes = self._merge_labels(row_groups.to(device=self.device, dtype=torch.int64))
        self._append_rows(rows, first, self.normalize if normalize is None else bool(normalize), codes)
        self.num_local_rows = first + m
        if row_origin is not None:
            self.row_origin = torch.cat([self.row_origin, row_origin.to(device=self.row_origin.device,
                                                                        dtype=self.row_origin.dtype)])
        self._shadow = None
        self._revision += 1
        self._fill_filter = RowFilter(self, self._fill, None)
        return range(self.index_base + first, self.index_base + first + m)

    # ------------------------------------------------------------------ remove, replace, compact
    def _refuse_sharded(self, what: str, why: str = "its global indices are contiguous per rank and would shift") -> None:
        if self.process_group is not None:
            raise ValueError(f"a sharded bank (process_group=) cannot {what}: {why}")

    # why the stored-row calls (`rows`, `scores`, `similarity_map`, `search_rows`) refuse a sharded bank
    _ROWS_ON_ONE_RANK = "a row is stored on one rank only, and every other rank would need it broadcast by its owner"

    def _local_index(self, index: object, name: str) -> Tensor:
        """Global row indices (an integer tensor or a sequence of ints) as a contiguous int64 `[m]` tensor of LOCAL rows
        on the bank's device; ValueError for one outside the bank (reads the extremes back to the host)."""
        r = index if isinstance(index, Tensor) else torch.as_tensor(list(index), dtype=torch.int64)
        if r.dtype.is_floating_point or r.dtype.is_complex or r.dtype == torch.bool or r.ndim != 1:
            raise ValueError(f"{name} must be a 1-D sequence of integer row indices")
        r = r.to(device=self.device, dtype=torch.int64) - self.index_base
        if r.numel() and (int(r.min()) < 0 or int(r.max()) >= self.num_local_rows):
            raise ValueError(f"{name} must lie in [{self.index_base}, {self.index_base + self.num_local_rows})")
        return r.contiguous()

    def _changed(self) -> None:
        """What every call that changes the stored rows ends with: the shadow is stale, older `RowFilter`s are refused."""
        self._shadow = None
        self._revision += 1
        self._fill_filter = None if self._fill is None else RowFilter(self, self._fill, None)

    def _counts(self) -> Tensor:
        """`_group_counts`, taken from the stored codes when nobody has kept it (a bare bank whose codes were set by hand)."""
        if self._group_counts is None:
            c = self._row_codes[self._row_codes >= 0].long()
            self._group_counts = torch.bincount(c, minlength=self.group_labels.numel())
        return self._group_counts

    @property
    def num_removed(self) -> int:
        """Rows `remove` has taken out since the bank was built or last compacted (kept on the host)."""
        return self._num_removed

    @property
    def live(self) -> Tensor:
        """bool `[len]` on the bank's device: False for the rows `remove` has taken out (unpacked from the fill bitmap,
        `isc_row_mask_unpack`)."""
        n = self.num_local_rows
        if not self._num_removed or n == 0:
            return torch.ones(n, dtype=torch.bool, device=self.device)
        return self._unpack_mask(self._fill, n)

    def remove(self, *, rows: "Tensor | Sequence[int] | None" = None, image_ids: "Tensor | Sequence[int] | None" = None,
               groups: "Tensor | Sequence[int] | None" = None) -> int:
        """Take rows out of the bank, chosen by exactly one of
        - `rows`: global row indices,
        - `image_ids`: every cell of these images (needs `row_origin`, i.e. a bank from `from_database`),
        - `groups`: every row that carries one of these `row_groups` labels (a label no row carries selects nothing),
        and return how many rows the call actually removed: duplicates and rows removed before are tolerated and counted
        once.  That count is one host read, like a grouped append's.  An index outside the bank raises ValueError before
        anything is launched.

        The selector becomes row indices with tensor ops; ONE launch (`isc_bank_remove`) then clears those rows' bits in the
        fill bitmap, which is the mask of every later search: the answers are those of the bank without the rows, bit for
        bit.  Row bytes are not touched.  Indices are stable: `len(bank)` stays the size of the index space, a removed
        index is never returned again, `append` keeps numbering from `len`, and `k` is still validated against `len` (a
        query with fewer than k rows left ends in score -inf, index -1 entries, as in any masked search).  `compact`
        closes the holes.  On a grouped bank the rows' stored codes become -2 and the per-group counts go down on the
        device; the planning figure of `search_groups` stays an upper bound until `compact`.

        A bank that never reserved capacity gains a fill bitmap of all ones first (one `isc_row_mask_pack` launch, its
        capacity is its length; the image does not move).  A `search` captured into a graph on a bank with spare capacity
        replays over the removal -- it is the masked call, and no pointer changes.  A graph captured while the bank had
        neither spare room nor holes holds the unmasked call: capture it again after the first `remove`.

        Runs on the caller's current stream, behind everything the bank has issued on its own streams (unresolved
        `search_async` handles see the bank as it was).  `RowFilter`s made before the call are refused afterwards.  A
        sharded bank (`process_group=`) cannot remove."""
        self._refuse_sharded("remove")
        if sum(x is not None for x in (rows, image_ids, groups)) != 1:
            raise ValueError("give exactly one of rows, image_ids or groups")
        if rows is not None:
            index = self._local_index(rows, "rows")
        elif image_ids is not None:
            if self.row_origin is None:
                raise ValueError("image_ids needs row_origin: build the bank with EmbeddingBank.from_database")
            if self.row_origin.shape[0] != self.num_local_rows:
                raise ValueError("row_origin does not describe the bank's rows")
            ids = image_ids if isinstance(image_ids, Tensor) else torch.as_tensor(list(image_ids), dtype=torch.int64)
            origin = self.row_origin[:, 0]
            index = torch.isin(origin, ids.to(device=origin.device, dtype=origin.dtype)).nonzero().squeeze(1).to(self.device)
        else:
            if self.group_labels is None:
                raise ValueError("groups needs row groups: build the bank with row_groups= (or from_database)")
            g = groups if isinstance(groups, Tensor) else torch.as_tensor(list(groups), dtype=torch.int64)
            _check_labels(g, "groups", g.shape[0] if g.ndim == 1 else -1, "[m]", got=True)
            codes = self._query_codes(g, g.shape[0])
            index = self._code_rows(codes[codes >= 0])
        if index.numel() == 0:
            return 0
        self._wait_for_issued()
        if self._fill is None:
            self._capacity = self.num_local_rows
            self._fill = self._pack_filter(torch.ones(self.num_local_rows, dtype=torch.bool, device=self.device)).packed
        if self._row_codes is not None:
            self._counts()
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._remove_rows(index, count)
        removed = int(count.item())
        self._num_removed += removed
        self._changed()
        return removed

    def replace(self, indices: "Tensor | Sequence[int]", rows: Tensor, *, normalize: bool | None = None) -> None:
        """Overwrite the stored vectors of the rows `indices` (global, distinct) with `rows` (floating `[m, D]`, on the
        bank's device), in place: ONE launch that touches only those rows (`isc_bank_replace`), with the arithmetic of the
        constructor and of `append` (`normalize` defaults to the bank's own setting), so the bank then equals the bank built
        with those vectors substituted.  Group and origin of a row are kept.  A removed index is skipped: the row stays
        removed.  Duplicate indices raise ValueError (found with one host read).  The norm bound the searches' rounding
        guard reads can only rise, so it stays a valid upper bound.

        No pointer changes: a captured masked `search` replays over the new vectors.  Stream order, stale `RowFilter`s and
        sharded banks: as in `remove`."""
        self._refuse_sharded("replace")
        if not isinstance(rows, Tensor) or not rows.dtype.is_floating_point:
            raise TypeError("rows must be a floating point torch.Tensor")
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must have shape [m, {self.dim}], got {tuple(rows.shape)}")
        if rows.device != self.device:
            raise ValueError(f"rows are on {rows.device} but the bank is on {self.device}")
        index = self._local_index(indices, "indices")
        if index.shape[0] != rows.shape[0]:
            raise ValueError(f"indices must name one row per vector: {index.shape[0]} indices for {rows.shape[0]} rows")
        if index.numel() == 0:
            return
        if int(torch.unique(index).numel()) != index.numel():
            raise ValueError("indices must be distinct")
        self._wait_for_issued()
        self._replace_rows(rows, index, self.normalize if normalize is None else bool(normalize))
        self._changed()

    def compact(self) -> Tensor:
        """Close the holes `remove` left: the surviving rows move, in row order, into a fresh image of the same capacity
        (`isc_bank_repack_map`, byte for byte; peak memory is the old image plus the new one).  Returns the int64
        `[len_before]` map from old to new row index (local rows, on the bank's device), -1 for the removed rows.  With no
        holes nothing happens and the identity map is returned.

        Afterwards `len` is the number of surviving rows, `row_origin` holds their rows only, `group_labels` has lost the
        labels no row carries any more (the stored codes are re-mapped) and the planning figure of `search_groups` is exact
        again: the bank equals, in everything a caller can see, the bank built from the surviving rows with `capacity=`.
        Graphs captured on the bank are invalidated exactly as by a growth (the old image is kept alive if a capture has
        seen it; the cached workspaces are dropped).  Stream order, stale `RowFilter`s and sharded banks: as in `remove`."""
        self._refuse_sharded("compact")
        n = self.num_local_rows
        if not self._num_removed:
            return torch.arange(n, dtype=torch.int64, device=self.device)
        self._wait_for_issued()
        live = self.live
        new_index = torch.where(live, torch.cumsum(live, 0) - 1, -1)
        self._relayout(self.capacity, new_index)
        self.num_local_rows = n - self._num_removed
        self._num_removed = 0
        if self.row_origin is not None:
            self.row_origin = self.row_origin[live.to(self.row_origin.device)]
        if self.group_labels is not None:
            counts = self._counts()
            keep = counts > 0
            if self.group_labels.numel():
                table = (torch.cumsum(keep, 0) - 1).to(torch.int32)
                stored = self._row_codes
                stored.copy_(torch.where(stored >= 0, table[stored.clamp(min=0).long()], stored))
            self.group_labels = self.group_labels[keep]
            self._group_counts = counts = counts[keep]
            self._max_group_rows = int(counts.max()) if counts.numel() else 0
        self._changed()
        return new_index

    def _merge_labels(self, new: Tensor) -> Tensor:
        """The int32 codes of an append's labels after merging them into `group_labels`, which stays sorted: a code is the
        label's position in it, so labels not seen before re-map the stored codes -- in place, through the old -> new
        position table, -2 kept -- before the launch.  Updates `_max_group_rows` (the one host read of a grouped append)."""
        old = self.group_labels
        merged = torch.unique(torch.cat([old, new]), sorted=True)
        counts = self._group_counts
        if counts is None:  # (a bare bank whose codes were set by hand)
            c = self._row_codes[self._row_codes >= 0].long()
            counts = torch.bincount(c, minlength=old.numel())
        if merged.numel() != old.numel():
            table = torch.searchsorted(merged, old)
            stored = self._row_codes
            if old.numel():
                stored.copy_(torch.where(stored >= 0, table.to(torch.int32)[stored.clamp(min=0).long()], stored))
            counts = torch.zeros(merged.numel(), dtype=counts.dtype, device=counts.device).index_add_(0, table, counts)
            self.group_labels = merged
        codes = torch.searchsorted(merged, new)
        counts = counts + torch.bincount(codes, minlength=merged.numel())
        self._group_counts = counts
        self._max_group_rows = int(counts.max())
        return codes.to(torch.int32).contiguous()

    # ------------------------------------------------------------------ properties
    @property
    def device(self) -> torch.device:
        return self._bank.device

    @property
    def bank(self) -> Tensor:
        """The stored rows as a row-major `[N_local, D]` tensor of the bank dtype (unpacked copy, `isc_bank_unpack`): all
        `len` slots; a removed row (`remove`) keeps the bytes it had until a growth or `reserve` moves the image: only live
        rows move, so it reads as zeros afterwards.  `rows(indices)` reads chosen rows without unpacking the rest."""
        out = torch.empty((self.num_local_rows, self.dim), dtype=self.dtype, device=self.device)
        if self.num_local_rows:
            lib = _lib.load()
            with torch.cuda.device(self.device):
                st = lib.isc_bank_unpack(
                    self._bank.data_ptr(), _lib.dtype_code(self.dtype), self.dim, self.capacity, 0,
                    self.num_local_rows, out.data_ptr(), self.dim, _lib.stream_handle(self.device),
                )
            _lib.check(st, "isc_bank_unpack")
        return out

    def __len__(self) -> int:
        return self.num_local_rows

    @property
    def capacity(self) -> int:
        """The row count the packed image is laid out for: `len(self)` unless room was reserved (`capacity=`, `reserve`,
        or the growth of an `append`)."""
        return self.num_local_rows if self._capacity is None else self._capacity

    # ------------------------------------------------------------------ row filters
    def _global_rows(self) -> int | None:
        """Rows of the whole (possibly sharded) bank; on a sharded bank the first call is a collective of every rank.
        None for a presharded bank without a process group: its shard ends at row index_base + len(self) of a bank whose
        size only the caller knows."""
        if self.process_group is None:
            return None if self.presharded else self.num_local_rows
        if self._n_total is None:
            self._n_total = self._total_rows()
        return self._n_total

    def row_filter(self, allow: Tensor | None = None, *, rows: "Tensor | Sequence[int] | None" = None,
                   image_ids: "Tensor | Sequence[int] | None" = None, exclude: bool = False) -> RowFilter:
        """A `RowFilter` of this bank for the `mask=` of its searches, from exactly one of
        - `allow`: bool `[N]` over the GLOBAL rows of the bank (True = the row may be returned),
        - `rows`: global row indices,
        - `image_ids`: the images whose cells may be returned (needs `row_origin`, i.e. a bank from `from_database`);
        `exclude=True` allows the complement instead.  Rows `remove` has taken out are never allowed.  A sharded bank keeps the bits of its own rows
        `[index_base, index_base + len(self))`; there every rank makes the filter (the first call learns the global row
        count with a collective).  A presharded bank without a process group takes an `allow` of any length that covers
        its rows.  The filter is packed on the device in one launch and belongs to this bank."""
        if sum(x is not None for x in (allow, rows, image_ids)) != 1:
            raise ValueError("give exactly one of allow, rows or image_ids")
        n_total = self._global_rows()
        hi = self.index_base + self.num_local_rows
        dev = self.device
        if allow is not None:
            ok = isinstance(allow, Tensor) and allow.dtype == torch.bool and allow.ndim == 1
            if not ok or (allow.shape[0] != n_total if n_total is not None else allow.shape[0] < hi):
                raise ValueError(f"allow must be a bool tensor of shape [{n_total if n_total is not None else 'N >= ' + str(hi)}]"
                                 " (the bank's global rows)")
            keep = allow.to(dev)
        elif rows is not None:
            r = rows if isinstance(rows, Tensor) else torch.as_tensor(list(rows), dtype=torch.int64)
            if r.dtype.is_floating_point or r.dtype == torch.bool or r.ndim != 1:
                raise ValueError("rows must be a 1-D sequence of integer row indices")
            r = r.to(torch.int64)
            if r.numel() and (int(r.min()) < 0 or (n_total is not None and int(r.max()) >= n_total)):
                raise ValueError(f"rows must lie in [0, {n_total if n_total is not None else 'N'})")
            size = n_total if n_total is not None else max(hi, int(r.max()) + 1 if r.numel() else 0)
            keep = torch.zeros(size, dtype=torch.bool, device=dev)
            keep[r.to(dev)] = True
        else:
            if self.row_origin is None:
                raise ValueError("image_ids needs row_origin: build the bank with EmbeddingBank.from_database")
            if self.row_origin.shape[0] != (n_total if n_total is not None else self.row_origin.shape[0]):
                raise ValueError("row_origin does not describe the bank's rows")
            ids = image_ids if isinstance(image_ids, Tensor) else torch.as_tensor(list(image_ids), dtype=torch.int64)
            origin = self.row_origin[:, 0]
            keep = torch.isin(origin, ids.to(device=origin.device, dtype=origin.dtype)).to(dev)
        if exclude:
            keep = ~keep
        local = keep[self.index_base : self.index_base + self.num_local_rows]
        if self._num_removed:  # a filter never allows a removed row, and `allowed_count` counts the rows it can return
            local = local & self.live
        return self._pack_filter(local)

    def _pack_filter(self, local: Tensor) -> RowFilter:
        """`isc_row_mask_pack` of this rank's bool `[N_local]` rows (zero-padded to the capacity the image is laid out for)."""
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        n = self.capacity
        if n == 0:
            return RowFilter(self, torch.empty(0, dtype=torch.int32, device=self.device), count)
        lib = _lib.load()
        words = _lib.c_size_t()
        _lib.check(lib.isc_row_mask_words(n, words), "isc_row_mask_words")
        packed = torch.empty(words.value, dtype=torch.int32, device=self.device)
        allow = local.to(torch.uint8).contiguous()
        if n > allow.shape[0]:  # the reserved room past the last row is never allowed
            allow = torch.nn.functional.pad(allow, (0, n - allow.shape[0]))
        with torch.cuda.device(self.device):
            st = lib.isc_row_mask_pack(allow.data_ptr(), n, packed.data_ptr(), count.data_ptr(),
                                       _lib.stream_handle(self.device))
        _lib.check(st, "isc_row_mask_pack")
        return RowFilter(self, packed, count)

    def _as_filter(self, mask: "RowFilter | Tensor | None") -> RowFilter | None:
        if mask is None:  # a bank with spare capacity or removed rows searches its live rows: the fill bitmap is the filter
            return self._fill_filter if self.num_local_rows < self.capacity or self._num_removed else None
        if isinstance(mask, RowFilter):
            if not mask.belongs_to(self):
                raise ValueError("this RowFilter belongs to another EmbeddingBank")
            if mask._revision != self._revision:
                raise ValueError("this RowFilter was made before the bank changed; make it again")
            return mask
        if isinstance(mask, Tensor):
            return self.row_filter(mask)
        raise TypeError(f"mask must be a RowFilter or a bool tensor, got {type(mask).__name__}")

    # ------------------------------------------------------------------ row groups
    def _pack_groups(self, codes: Tensor) -> Tensor:
        """`isc_row_groups_pack` of this rank's int32 `[N_local]` row codes: int32 `[ceil(N_local / 256) * 256]` (of the
        capacity the image is laid out for, the rows past `N_local` coded -2 like the padding)."""
        n = self.capacity
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        if n > codes.shape[0]:
            codes = torch.nn.functional.pad(codes, (0, n - codes.shape[0]), value=-2)
        packed = torch.empty((n + 255) // 256 * 256, dtype=torch.int32, device=self.device)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            st = lib.isc_row_groups_pack(codes.data_ptr(), n, packed.data_ptr(), _lib.stream_handle(self.device))
        _lib.check(st, "isc_row_groups_pack")
        return packed

    def _query_codes(self, exclude_group: Tensor | None, nq: int) -> Tensor | None:
        """The int32 `[Q]` codes of `exclude_group` labels on the bank's device: a label's position among this rank's
        `group_labels`, -1 for a label no row of the rank carries.  Tensor ops only: no host synchronisation."""
        if exclude_group is None:
            return None
        _check_labels(exclude_group, "exclude_group", nq, f"[Q] = [{nq}]", got=True)
        if self.group_labels is None:
            raise ValueError("exclude_group needs row groups: build the bank with row_groups= (or from_database)")
        x = exclude_group.to(device=self.device, dtype=torch.int64)
        labels = self.group_labels
        if labels.numel() == 0:
            return torch.full((nq,), -1, dtype=torch.int32, device=self.device)
        pos = torch.searchsorted(labels, x).clamp_(max=labels.numel() - 1)
        return torch.where(labels[pos] == x, pos, -1).to(torch.int32)

    # ------------------------------------------------------------------ search
    def _prepare_queries(self, queries: Tensor) -> Tensor:
        if not isinstance(queries, Tensor) or not queries.dtype.is_floating_point:
            raise TypeError("queries must be a floating point torch.Tensor")
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"queries must have shape [Q, {self.dim}], got {tuple(queries.shape)}")
        if queries.device != self.device:
            raise ValueError(f"queries are on {queries.device} but the bank is on {self.device}")
        # float16 and float32 queries go to the library as they are: `isc_cosine_topk` rounds them to the bank dtype while
        # it packs them (`q_dtype`; float32 -> fp16 round to nearest even, the arithmetic of `Tensor.to(float16)`), so the
        # reference-shaped call `bank.search(predict_step(batch).get_flat_vectors())` -- float32 vectors, data.py:112-118 --
        # runs no cast kernel.  Other floating types are converted here, directly to the bank dtype.
        if queries.dtype not in (torch.float16, torch.float32):
            queries = queries.to(self.dtype)
        return queries if queries.stride(1) == 1 or queries.shape[0] == 0 else queries.contiguous()

    def _workspace(self, n_queries: int, k: int, lane: int = -1, collapse: bool = False) -> Tensor:
        """The search workspace.  The C side runs a call as passes of at most `ISC_SEARCH_PASS_QUERIES` queries over
        one workspace and cuts the queries into ONE tile of 64 (Q <= 64) or 128 (Q <= 128), or tiles of 256, so the size depends on
        (padded queries of a pass, k) only: alternating batch sizes inside one bucket -- a pipeline's short last
        batch -- reuse one allocation instead of reallocating 150-300 MB per call.  One buffer per bucket and lane is kept.

        A workspace handed out while the current stream is being captured is also kept in `_captured_workspaces`, which
        the bucket cache never evicts: the graph holds its raw pointer, and a replay after the bucket had been dropped would
        write into whatever tensor the allocator had given that memory to.

        `collapse`: the workspace of the collapsed search (`isc_cosine_topk_collapse_workspace_bytes`), cached apart."""
        nq = min(n_queries, _lib.ISC_SEARCH_PASS_QUERIES)
        key = (-(-nq // 64) * 64 if nq <= 128 else -(-nq // 256) * 256, k) + (("collapse",) if collapse else ())
        cache = self._workspaces.setdefault(lane, {})
        ws = cache.get(key)
        if ws is None:
            lib = _lib.load()
            need = _lib.c_size_t()
            if k > _lib.ISC_TOPK_MAX_K:  # the large-k search (its passes shrink as k grows: O(queries per pass x k))
                st = lib.isc_cosine_topk_large_workspace_bytes(_lib.dtype_code(self.dtype), self.capacity, self.dim,
                                                               key[0], k, need)
                _lib.check(st, "isc_cosine_topk_large_workspace_bytes")
            elif collapse:
                st = lib.isc_cosine_topk_collapse_workspace_bytes(
                    _lib.dtype_code(self.dtype), self.capacity, self.dim, min(key[0], _lib.ISC_SEARCH_PASS_QUERIES),
                    k, max(self._max_group_rows, 1), need)
                _lib.check(st, "isc_cosine_topk_collapse_workspace_bytes")
            else:
                st = lib.isc_cosine_topk_workspace_bytes(
                    _lib.dtype_code(self.dtype), self.capacity, self.dim, min(key[0], _lib.ISC_SEARCH_PASS_QUERIES), k,
                    need
                )
                _lib.check(st, "isc_cosine_topk_workspace_bytes")
            ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            if len(cache) >= 4:  # bound what a bank pins: drop the oldest bucket
                cache.pop(next(iter(cache)))
            cache[key] = ws
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            if all(t.data_ptr() != ws.data_ptr() for t in self._captured_workspaces):
                self._captured_workspaces.append(ws)
        return ws

    def _shadow_for(self, nq: int, k: int) -> Tensor | None:
        """The bank's int8 shadow if a plain search of `nq` queries uses it (`isc_cosine_topk_uses_shadow`: an fp16 bank,
        more than 256 queries per pass, a plan with an int8 level -- `isc_cosine_topk_plan`), built on the current stream
        the first time and kept until `append` / `reserve` change the image.  None while the stream is being captured: the
        fp16 levels run then, with the same answer."""
        if not self.shadow or self.dtype != torch.float16 or nq <= 256 or self._fill is not None:
            return None
        if torch.cuda.is_current_stream_capturing():  # (a graph would pin a buffer that `append` / `reserve` drop)
            return None
        if self._shadow is None:
            lib = _lib.load()
            uses = _lib.c_int()
            _lib.check(lib.isc_cosine_topk_uses_shadow(_lib.ISC_F16, self.capacity, self.dim, nq, k, uses),
                       "isc_cosine_topk_uses_shadow")
            if not uses.value:
                return None
            need = _lib.c_size_t()
            _lib.check(lib.isc_bank_shadow_bytes(self.capacity, self.dim, need), "isc_bank_shadow_bytes")
            shadow = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                st = lib.isc_bank_quantize(self._bank.data_ptr(), self.capacity, self.dim, shadow.data_ptr(),
                                           shadow.numel(), _lib.stream_handle(self.device))
            _lib.check(st, "isc_bank_quantize")
            self._shadow = shadow
        return self._shadow

    def _new_out(self, nq: int, k: int) -> tuple[Tensor, Tensor, Tensor]:
        """What a local search writes when the caller gave no `out`: (scores [Q, k], indices [Q, k], status int32[4])."""
        return (torch.empty((nq, k), dtype=torch.float32, device=self.device),
                torch.empty((nq, k), dtype=torch.int64, device=self.device),
                torch.empty(4, dtype=torch.int32, device=self.device))

    def _row_search(self, base: str, args: tuple, mask: RowFilter | None, groups: Tensor | None, stream: int) -> None:
        """One row-search call of the C ABI on `stream` (a raw handle): `base` itself, `base_masked` with the row filter's
        bitmap, or -- `groups`: int32 `[Q]` query codes -- `base_grouped` with the bitmap (or NULL), the packed row codes
        and the query codes, each behind the arguments `args` the three share."""
        if groups is not None:
            name = base + "_grouped"
            args += (None if mask is None else mask.packed.data_ptr(), self._row_codes.data_ptr(), groups.data_ptr())
        elif mask is not None:
            name = base + "_masked"
            args += (mask.packed.data_ptr(),)
        else:
            name = base
        with torch.cuda.device(self.device):
            st = getattr(_lib.load(), name)(*args, stream)
        _lib.check(st, name)

    def _local_topk(
        self, queries: Tensor, k: int, out: tuple[Tensor, Tensor, Tensor] | None = None, lane: int = -1,
        stream: "torch.cuda.Stream | None" = None, mask: RowFilter | None = None, groups: Tensor | None = None,
    ) -> tuple[Tensor, Tensor]:
        """Top-k of this rank's rows: `(float32 [Q, k], int64 [Q, k])` with GLOBAL row indices, final when the stream
        has run the call.  `out` optionally supplies the (scores, indices, status int32[4]) tensors to write into (the
        exchange buffer of a sharded search); `lane` / `stream`: the workspace set and the stream of an asynchronous search
        (default: the caller's current stream).  Tensors are allocated on the caller's stream whichever stream computes.
        `mask`: search the rows of a row filter only (`isc_cosine_topk_masked`); a query with fewer than k allowed rows ends
        in the C ABI's padding (score NaN, index INT64_MAX), which the public calls map to (-inf, -1) at the very end.
        `groups`: int32 `[Q]` query codes (`_query_codes`): query q skips the rows of its group (`isc_cosine_topk_grouped`),
        with the masked search's padding."""
        nq = queries.shape[0]
        scores, indices, status = out if out is not None else self._new_out(nq, k)
        ws = self._workspace(nq, k, lane)
        large = k > _lib.ISC_TOPK_MAX_K  # isc_cosine_topk_large: one entry point for the three filters, no shadow
        shadow = self._shadow_for(nq, k) if mask is None and groups is None and not large else None
        if stream is not None:
            # every tensor this call touches was allocated on some other stream: tell the allocator the lane uses it, so
            # that nothing handed back early (a dropped handle, a dropped bank, a workspace bucket pushed out of the cache)
            # is given to somebody else before the lane's kernels have run
            for t in (scores, indices, status, ws, self._bank, self._norm_bound):
                t.record_stream(stream)
            if mask is not None:
                mask.packed.record_stream(stream)
            if groups is not None:
                groups.record_stream(stream)
                self._row_codes.record_stream(stream)
            if shadow is not None:
                # built on the caller's stream: the lane starts behind it
                built = torch.cuda.Event()
                built.record(torch.cuda.current_stream(self.device))
                stream.wait_event(built)
                shadow.record_stream(stream)
        args = (
            self._bank.data_ptr(), _lib.dtype_code(self.dtype), self.capacity, self.dim, queries.data_ptr(),
            _lib.dtype_code(queries.dtype), nq, queries.stride(0), k, self.index_base, self._norm_bound.data_ptr(),
            scores.data_ptr(), indices.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
        )
        if shadow is not None:
            args += (shadow.data_ptr(),)
        handle = stream.cuda_stream if stream is not None else _lib.stream_handle(self.device)
        if large:
            self._large_search("isc_cosine_topk_large", args, mask, groups, handle)
        else:
            self._row_search("isc_cosine_topk_shadow" if shadow is not None else "isc_cosine_topk", args, mask, groups,
                             handle)
        self.last_status = status
        return scores, indices

    def _large_search(self, name: str, args: tuple, mask: RowFilter | None, groups: Tensor | None, stream: int) -> None:
        """One large-k call of the C ABI (120 < k <= `ISC_TOPK_LARGE_MAX_K`) on `stream`: `name` takes the row filter's
        bitmap, the packed row codes and the query codes behind `args`, each NULL when the search has no such filter."""
        with torch.cuda.device(self.device):
            st = getattr(_lib.load(), name)(
                *args, None if mask is None else mask.packed.data_ptr(),
                None if groups is None else self._row_codes.data_ptr(), None if groups is None else groups.data_ptr(),
                stream)
        _lib.check(st, name)

    def search_exhaustive(self, queries: Tensor, k: int = 10, *, mask: "RowFilter | Tensor | None" = None,
                          exclude_group: Tensor | None = None) -> tuple[Tensor, Tensor]:
        """The same answer from the data-independent float64 kernel (`isc_cosine_topk_exhaustive`): every score of
        every query evaluated exactly.  Slow; the on-device reference the fast path is tested against.  `mask`,
        `exclude_group`: as in `search`.  `k` up to `ISC_TOPK_LARGE_MAX_K`: above 120 the same scores are selected by a
        radix select over the bank (`isc_cosine_topk_exhaustive_large`: nine sweeps per four queries)."""
        rf = self._as_filter(mask)
        q = self._prepare_queries(queries)
        nq = q.shape[0]
        qg = self._query_codes(exclude_group, nq)
        if self.process_group is not None:
            raise ValueError("search_exhaustive answers for one shard; merge the shards with search()")
        if not 1 <= k <= self.num_local_rows:
            raise ValueError(f"k={k} must be in [1, {self.num_local_rows}]")
        if k > _lib.ISC_TOPK_LARGE_MAX_K:
            raise ValueError(f"k must be <= {_lib.ISC_TOPK_LARGE_MAX_K}, got {k}")
        lib = _lib.load()
        code = _lib.dtype_code(self.dtype)
        need = _lib.c_size_t()
        # beyond ISC_TOPK_MAX_K: the radix-select form of the same sweep (isc_cosine_topk_exhaustive_large)
        base = "isc_cosine_topk_exhaustive" + ("_large" if k > _lib.ISC_TOPK_MAX_K else "")
        _lib.check(getattr(lib, base + "_workspace_bytes")(code, self.capacity, self.dim, nq, k, need),
                   base + "_workspace_bytes")
        ews = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        indices = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        args = (
            self._bank.data_ptr(), code, self.capacity, self.dim, q.data_ptr(), _lib.dtype_code(q.dtype), nq,
            q.stride(0), k, self.index_base, scores.data_ptr(), indices.data_ptr(), ews.data_ptr(), ews.numel(),
        )
        if k > _lib.ISC_TOPK_MAX_K:
            self._large_search(base, args, rf, qg, _lib.stream_handle(self.device))
        else:
            self._row_search(base, args, rf, qg, _lib.stream_handle(self.device))
        return (scores, indices) if rf is None and qg is None else _unpad(scores, indices)

    def _merge_topk(self, scores: Tensor, indices: Tensor, k: int) -> tuple[Tensor, Tensor]:
        """Merge `[G, Q, kin]` partial results into `[Q, k]` by (score desc, index asc) (`isc_topk_merge`).  The two
        inputs may be strided along G (views into the all-gathered exchange buffer); their `[Q, kin]` blocks are dense."""
        g, nq, kin = scores.shape
        if scores.stride(1) != kin or scores.stride(2) != 1 or indices.stride(1) != kin or indices.stride(2) != 1:
            scores, indices = scores.contiguous(), indices.contiguous()
        out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
        out_i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
        lib = _lib.load()
        with torch.cuda.device(scores.device):
            st = lib.isc_topk_merge(
                scores.data_ptr(), indices.data_ptr(), g, nq, kin, k, scores.stride(0) if g > 1 else 0,
                indices.stride(0) if g > 1 else 0, out_s.data_ptr(), out_i.data_ptr(), _lib.stream_handle(scores.device),
            )
        _lib.check(st, "isc_topk_merge")
        return out_s, out_i

    def _total_rows(self) -> int:
        if self.process_group is None:
            return self.num_local_rows
        counts = [0] * self.world_size
        dist.all_gather_object(counts, self.num_local_rows, group=self.process_group)
        return int(sum(counts))

    def search(self, queries: Tensor, k: int = 10, *, mask: "RowFilter | Tensor | None" = None,
               exclude_group: Tensor | None = None, check: bool = True) -> tuple[Tensor, Tensor]:
        """Cosine top-k of every query against the whole (possibly sharded) bank.

        Returns `(scores float32 [Q, k], indices int64 [Q, k])`, best first, ties by lower row index.  The call
        only enqueues work: no host synchronisation, and the result is final -- queries the float32 filter cannot
        prove are redone exactly on the device.  `last_status` (int32[4], device) holds diagnostics: [0] overflowed
        candidate buffers, [1] queries the first pass could not prove (searched again: one more matrix-core pass over the
        bank for all of them together), [3] queries answered by the exhaustive float64 sweep (about one bank sweep per
        four such queries: a bank with thousands of exact copies of a row pays this for queries that hit them).  `check` is accepted for compatibility with the
        first version of this API and ignored.  Everything runs on the caller's current stream (a sharded bank's
        exchange on the bank's exchange stream, ordered behind it).

        `mask` restricts the search to a set of rows: a `RowFilter` of this bank (`row_filter`), or a bool tensor of the
        bank's GLOBAL row count (True = allowed), packed for this call.  The answer is the search of the bank of the
        allowed rows alone, with indices in the whole bank, bit for bit; `k` is still bounded by the bank size, and a
        query with fewer than k allowed rows ends in score -inf, index -1 entries.  The whole bank is streamed whatever
        the filter's density (the masked filter).

        `exclude_group`: an integer `[Q]` tensor (any device) of group labels, on a bank built with `row_groups=`: query q
        skips the rows whose label equals `exclude_group[q]` ("not my own image"), on top of `mask`.  Each query's answer
        is the masked search of the rows it may return, bit for bit, padded as above; a label no row carries excludes
        nothing.  The labels become codes on the device, so a grouped search stays capturable.

        `k` may be up to `ISC_TOPK_LARGE_MAX_K` = 4096 on an unsharded bank.  Above `ISC_TOPK_MAX_K` = 120 the call is
        `isc_cosine_topk_large` ("Top-k beyond 120"): a matrix-core pass proves a lower bound of each query's
        k-th score, the range search's filter, float64 re-score and sort run behind it, and the first k rows are the
        answer -- the same contract, filters and padding, about one pass over the bank more than `search_range` at the k-th
        score.  `last_status` then holds [0] passes whose candidate buffer overflowed, [1] queries answered by the float64
        last resort (`search_exhaustive`'s kernels), [2] the largest filter error over its bound (float bits, < 1),
        [3] candidates the filter kept.  The int8 shadow is not used there.

        A world-1 `search` may be captured into a CUDA / HIP graph (`torch.cuda.graph`) and replayed.  The workspace a
        capture used stays allocated for the bank's lifetime so that replays stay valid: each distinct (query bucket, k)
        captured pins one `isc_cosine_topk_workspace_bytes` buffer -- up to a few hundred MB on a large bank -- until the
        bank is dropped.
        """
        del check
        return self._search(queries, k, lanes=False, mask=mask, exclude_group=exclude_group).result()

    def search_async(self, queries: Tensor, k: int = 10, *, mask: "RowFilter | Tensor | None" = None,
                     exclude_group: Tensor | None = None) -> SearchHandle:
        """`search` that returns as soon as everything is ENQUEUED; `handle.result()` orders the caller's current stream
        behind the answer.  The local kernels of a search of up to 128 queries run on one of TWO library-owned streams
        of the device, alternately -- the bank keeps a workspace for each -- ordered behind the caller's stream as it
        stands at the call (larger searches stay on the caller's stream); a sharded bank's exchange (all-gather + merge)
        runs on the bank's exchange stream.  A caller that issues search i + 1 before it resolves handle i
        therefore has the short kernels at the end of search i (selection, exact re-score, the empty redo launches) and
        its exchange running beside the first kernels of search i + 1 -- at a 1.25 M-row shard 20 - 25 us of a 320 us
        search (`scripts/two_stream_probe.py`).  At most two searches of one bank should be unresolved at a time (a
        third waits, on the device, for the first one).

        Ownership until `handle.result()`: the search reads `queries` on a library-owned stream (float16 / float32
        queries with unit inner stride are NOT copied), and writes `last_status` / `last_gathered_status` there -- so the
        caller must not overwrite the query tensor in place, nor read those status tensors, on its own stream before it
        has resolved the handle.  `search()` has no such window: everything it does is ordered on the caller's stream.
        `mask`, `exclude_group`: as in `search` (a `RowFilter` is read on the library's stream too: keep it until the handle
        is resolved)."""
        return self._search(queries, k, lanes=True, mask=mask, exclude_group=exclude_group)

    def _lane(self, cur: "torch.cuda.Stream", q: Tensor) -> tuple[int, "torch.cuda.Stream"]:
        """The next of the two search streams, ordered behind everything the caller's stream holds so far."""
        lane = self._lane_next
        self._lane_next ^= 1
        ls = _lane_streams(self.device)[lane]
        ready = torch.cuda.Event()
        ready.record(cur)
        ls.wait_event(ready)
        q.record_stream(ls)  # (possibly a copy made on the caller's stream: keep it until the lane has read it)
        return lane, ls

    # Searches of more queries than this run on the caller's stream even when asynchronous: their kernels fill the GPU for
    # milliseconds, there is nothing at their ends worth overlapping (measured: 1 757 -> 1 749 us at Q = 1024 on a 1.25 M-row
    # shard), and two of them sharing the GPU would stretch each other's launches.
    _LANE_MAX_QUERIES = 128

    def _search(self, queries: Tensor, k: int, lanes: bool, mask: "RowFilter | Tensor | None" = None,
                exclude_group: Tensor | None = None, query_codes: Tensor | None = None) -> SearchHandle:
        """`query_codes`: the int32 `[Q]` codes of the queries' groups themselves, in place of `exclude_group` labels
        (`search_rows` reads them from the stored codes)."""
        rf = self._as_filter(mask)
        self._check_k(k, _lib.ISC_TOPK_LARGE_MAX_K)
        if k > _lib.ISC_TOPK_MAX_K and self.process_group is not None:
            # (isc_topk_merge holds at most 4096 inputs per query: G shards of k > 120 candidates do not fit)
            raise ValueError(f"a sharded bank searches k <= {_lib.ISC_TOPK_MAX_K}, got {k}: the merge of the shards' "
                             "lists has no large-k form")
        q = self._prepare_queries(queries)
        nq = q.shape[0]
        filt = self._filter_kwargs(rf, self._query_codes(exclude_group, nq) if query_codes is None else query_codes)
        # sharded: the first search learns the bank's size with a collective of every rank
        n_rows = self.num_local_rows if self.process_group is None else self._global_rows()
        if k > n_rows:
            raise ValueError(f"k={k} exceeds the bank size {n_rows}")
        if nq == 0:
            return SearchHandle(*self._empty_topk(k))
        on_gpu = self.device.type == "cuda"
        lanes = lanes and on_gpu and nq <= self._LANE_MAX_QUERIES
        if self.process_group is None:
            lane, ls = self._lane(torch.cuda.current_stream(self.device), q) if lanes else (-1, None)
            out = self._local_topk(q, k, lane=lane, stream=ls, **filt)
            if filt:  # the padding of a filtered search becomes (-inf, -1) on the stream that computed it
                with torch.cuda.stream(ls) if ls is not None else nullcontext():
                    out = _unpad(*out)
            if ls is None:
                return SearchHandle(*out)
            done = torch.cuda.Event()
            done.record(ls)
            return SearchHandle(*out, done)

        # ---- sharded: local partial top-k -> ONE all-gather -> merge on every rank.  Every rank issues exactly one
        # collective per search whatever its shard holds, so the ranks cannot fall out of step.
        nbytes, views = _exchange_layout(nq, k)
        slot = self._slots[self._slot_next]
        self._slot_next ^= 1
        lane, ls = -1, None
        kl = min(k, self.num_local_rows)
        if on_gpu:
            cur = torch.cuda.current_stream(self.device)
            if slot.buf is None or slot.buf.numel() < nbytes:
                if slot.done is not None:  # the old buffer goes back to this stream's pool: nobody may still read it
                    cur.wait_event(slot.done)
                slot.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if lanes and kl == k:  # (a shard with fewer rows than k is padded with tensor ops on the caller's stream)
                lane, ls = self._lane(cur, q)
                cur = ls  # the stream the local kernels run on
            if slot.done is not None:  # the exchange that last read this buffer (two searches ago)
                cur.wait_event(slot.done)
        elif slot.buf is None or slot.buf.numel() < nbytes:
            slot.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        xbuf = slot.buf[:nbytes]
        part_s, part_i, status = views(xbuf)
        if kl < k:
            # (an unfiltered search pads with -inf; a filtered one with the C ABI's NaN, which ranks after the NaN-scored
            # rows of other shards too)
            self._short_shard(self._local_topk, q, kl, filt, (part_s, part_i), status, math.nan if filt else -math.inf)
        else:
            self._local_topk(q, k, out=(part_s, part_i, status), lane=lane, stream=ls, **filt)

        def exchange() -> tuple[Tensor, Tensor, Tensor]:
            all_s, all_i, gstatus = views(self._all_gather_bytes(xbuf))  # gstatus [G, 4]: every shard's diagnostics
            out = self._merge_topk(all_s, all_i, k)
            return (*(_unpad(*out) if filt else out), gstatus)

        if not on_gpu:  # CPU tensors (the gloo rehearsal of the host logic): nothing to overlap
            out_s, out_i, gstatus = exchange()
            self.last_gathered_status = gstatus
            return SearchHandle(out_s, out_i, None, gstatus)
        if self._xstream is None:
            self._xstream = torch.cuda.Stream(self.device)
        local_done = torch.cuda.Event()
        local_done.record(cur)
        with torch.cuda.stream(self._xstream):
            self._xstream.wait_event(local_done)
            xbuf.record_stream(self._xstream)  # (allocated on the caller's stream, read by the all-gather on this one)
            out_s, out_i, gstatus = exchange()
            done = torch.cuda.Event()
            done.record(self._xstream)
        slot.done = done
        self.last_gathered_status = gstatus  # valid once the handle has been resolved
        return SearchHandle(out_s, out_i, done, gstatus)

    def _short_shard(self, local, q: Tensor, kl: int, filt: dict, planes: tuple[Tensor, ...], status: Tensor,
                     pad_score: float) -> None:
        """The exchange planes of a shard with `kl` < k rows: its `local(q, kl, **filt)` answer -- `_local_topk`, or
        `_local_collapse` with a labels plane -- in the first `kl` columns, the rest entries that rank after every real
        candidate (`pad_score`, INT64_MAX, label -1); status zero."""
        for plane, pad in zip(planes, (pad_score, _PAD_INDEX, -1)):
            plane.fill_(pad)
        status.zero_()
        if kl > 0:
            for plane, part in zip(planes, local(q, kl, **filt)):
                plane[:, :kl] = part

    def _all_gather_bytes(self, xbuf: Tensor) -> Tensor:
        """`[G, nbytes]` uint8: every rank's exchange buffer (one all-gather; RCCL over xGMI on the GPUs)."""
        # a gloo group exchanges host copies (used to rehearse the multi-rank path without RCCL)
        on_host = dist.get_backend(self.process_group) == "gloo" and xbuf.device.type != "cpu"
        src = xbuf.cpu() if on_host else xbuf
        gathered = torch.empty(self.world_size * src.numel(), dtype=torch.uint8, device=src.device)
        dist.all_gather_into_tensor(gathered, src, group=self.process_group)
        return gathered.to(xbuf.device).view(self.world_size, src.numel())

    # ------------------------------------------------------------------ stored rows
    def rows(self, indices: "Tensor | Sequence[int]") -> Tensor:
        """The stored vectors of the rows `indices` (global, any order, duplicates allowed): `[m, D]` of the bank dtype,
        ONE launch that reads only those rows (`isc_bank_gather`) -- `bank.bank[indices]` bit for bit without unpacking the
        bank.  A removed row reads as zeros.  An index outside the bank raises ValueError.  Runs on the caller's current
        stream.  A sharded bank (`process_group=`) cannot read rows back."""
        self._refuse_sharded("read rows back", self._ROWS_ON_ONE_RANK)
        index = self._local_index(indices, "indices")
        out = torch.empty((index.numel(), self.dim), dtype=self.dtype, device=self.device)
        if index.numel():
            self._gather_rows(index, out)
        return out

    def scores(self, queries: Tensor, rows: "Tensor | Sequence[int]") -> Tensor:
        """The scores of `queries` (floating `[Q, D]`, as in `search`) against the rows `rows` (global, any order,
        duplicates allowed): float32 `[Q, M]`, ONE launch that reads only those rows (`isc_cosine_scores`).  Entry
        `[q, j]` has the bits `search_exhaustive` returns for that query and row -- re-rank a candidate list from elsewhere,
        or check a `search` result by hand.  The column of a removed row is -inf.  `Q == 0` or `M == 0` gives an empty
        tensor without a launch.  No host synchronisation past the index check.  A sharded bank cannot score rows."""
        self._refuse_sharded("score rows", self._ROWS_ON_ONE_RANK)
        q = self._prepare_queries(queries)
        index = self._local_index(rows, "rows")
        out = torch.empty((q.shape[0], index.numel()), dtype=torch.float32, device=self.device)
        if out.numel():
            self._score_rows(q, index, out)
        return out

    # ------------------------------------------------------------------ nearest centroid, sums per group
    def _assign_rows(self, q: Tensor, mask: RowFilter | None, labels: Tensor, scores: Tensor | None,
                     exhaustive: bool) -> None:
        """`isc_bank_assign` (`exhaustive`: `isc_bank_assign_exhaustive`): `labels` (int32 `[capacity]`) and, unless None,
        `scores` (float32 `[capacity]`) receive the best centroid of `q` (prepared, C > 0) for every row of the image in
        ORIGINAL row order, (-1, -inf) for a row `mask` (None: the fill bitmap, if the bank has one) does not allow.  On the
        current stream, no host read; the status words are left in `last_assign_status`.  A device hook."""
        lib = _lib.load()
        dev = self.device
        n = self.capacity
        code = _lib.dtype_code(self.dtype)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        rm = _lib.ptr(mask.packed) if mask is not None else _lib.ptr(self._fill)
        ws = None
        if not exhaustive:
            need = _lib.c_size_t()
            _lib.check(lib.isc_bank_assign_workspace_bytes(code, n, self.dim, q.shape[0], need),
                       "isc_bank_assign_workspace_bytes")
            if self._assign_ws is None or self._assign_ws.numel() < need.value:
                self._assign_ws = None
                self._assign_ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            ws = self._assign_ws
        with torch.cuda.device(dev):
            head = (self._bank.data_ptr(), code, n, self.dim, q.data_ptr(), _lib.dtype_code(q.dtype), q.shape[0],
                    q.stride(0))
            tail = (rm, labels.data_ptr(), _lib.ptr(scores), status.data_ptr(), _lib.ptr(ws),
                    0 if ws is None else ws.numel(), _lib.stream_handle(dev))
            if exhaustive:
                st = lib.isc_bank_assign_exhaustive(*head, *tail)
            else:
                st = lib.isc_bank_assign(*head, self._norm_bound.data_ptr(), *tail)
        _lib.check(st, "isc_bank_assign_exhaustive" if exhaustive else "isc_bank_assign")
        self.last_assign_status = status

    def _group_sums(self, rows: Tensor, offsets: Tensor, sums: Tensor, counts: Tensor) -> None:
        """`isc_bank_group_sums`: `sums[g]` (float64 `[G, D]`) and `counts[g]` (int64 `[G]`) receive the sum and the number
        of the live rows among `rows[offsets[g]:offsets[g + 1]]` (int64, device; entries past `offsets[G]` are ignored).
        On the current stream, no host read.  A device hook."""
        lib = _lib.load()
        dev = self.device
        code = _lib.dtype_code(self.dtype)
        need = _lib.c_size_t()
        _lib.check(lib.isc_bank_group_sums_workspace_bytes(code, rows.numel(), self.dim, need),
                   "isc_bank_group_sums_workspace_bytes")
        if self._sums_ws is None or self._sums_ws.numel() < need.value:
            self._sums_ws = None
            self._sums_ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        ws = self._sums_ws
        with torch.cuda.device(dev):
            st = lib.isc_bank_group_sums(
                self._bank.data_ptr(), code, self.capacity, self.dim, rows.data_ptr(), rows.numel(), offsets.data_ptr(),
                counts.numel(), _lib.ptr(self._fill), sums.data_ptr(), sums.stride(0), counts.data_ptr(), ws.data_ptr(),
                ws.numel(), _lib.stream_handle(dev),
            )
        _lib.check(st, "isc_bank_group_sums")

    _assign_ws: Tensor | None = None  # the workspaces of `assign` and `group_sums`, grown on demand like `_range_ws`
    _sums_ws: Tensor | None = None
    last_assign_status: Tensor | None = None

    def _assign(self, centroids: Tensor, mask: "RowFilter | Tensor | None", return_scores: bool,
                exhaustive: bool) -> tuple[Tensor, Tensor | None]:
        self._refuse_sharded("assign rows to centroids", self._ROWS_ON_ONE_RANK)
        q = self._prepare_queries(centroids)
        if q.shape[0] == 0:
            raise ValueError("centroids must hold at least one vector")
        if q.shape[0] > 1 << 24:
            raise ValueError(f"at most {1 << 24} centroids, got {q.shape[0]}")
        rf = self._as_filter(mask)
        n = self.num_local_rows
        labels = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
        scores = torch.empty(self.capacity, dtype=torch.float32, device=self.device) if return_scores else None
        if n:
            self._assign_rows(q, rf, labels, scores, exhaustive)
        return labels[:n], None if scores is None else scores[:n]

    def assign(self, centroids: Tensor, *, mask: "RowFilter | Tensor | None" = None,
               return_scores: bool = True) -> tuple[Tensor, Tensor | None]:
        """For EVERY stored row the nearest of `centroids` (floating `[C, D]`, C >= 1, as the queries of `search`): labels
        int32 `[len]` and, with `return_scores`, the winning scores float32 `[len]` (else None), in row order.  The score
        of a centroid against a row is the score `search` gives the centroid as a query (`scores(centroids, [r])` bit for
        bit); the best is by score descending, NaN last, ties to the lower centroid.  A removed row, and a row `mask`
        (`RowFilter` or bool `[N]`) does not allow, gets label -1 and score -inf.  The packed bank is streamed once per 64
        centroids on the matrix cores and finished exactly (`isc_bank_assign`; `last_assign_status` holds its status
        words); labels alone are cheaper than labels with scores.  Runs on the caller's current stream with no host read.
        A sharded bank cannot assign."""
        return self._assign(centroids, mask, return_scores, False)

    def assign_exhaustive(self, centroids: Tensor, *, mask: "RowFilter | Tensor | None" = None,
                          return_scores: bool = True) -> tuple[Tensor, Tensor | None]:
        """`assign` answered by the data-independent float64 kernel (`isc_bank_assign_exhaustive`): slow, the reference
        `assign` is tested against, bit for bit."""
        return self._assign(centroids, mask, return_scores, True)

    def group_sums(self, labels: Tensor, num_groups: int) -> tuple[Tensor, Tensor]:
        """Float64 sums of the stored rows per label: `sums` `[G, D]` float64 and `counts` `[G]` int64 with G =
        `num_groups`, from `labels` (integer `[len]`, e.g. the labels of `assign`).  Rows whose label is outside `[0, G)`
        and removed rows are ignored.  A stable sort of the labels lists the rows group by group; `isc_bank_group_sums`
        adds them in that order without floating-point atomics, so the same labels give the same bits.  No host read.
        A sharded bank cannot sum rows."""
        self._refuse_sharded("sum rows per group", self._ROWS_ON_ONE_RANK)
        n = self.num_local_rows
        ok = isinstance(labels, Tensor) and labels.ndim == 1 and labels.shape[0] == n
        if not ok or labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise ValueError(f"labels must be an integer tensor of shape [{n}] (one label per row)")
        if isinstance(num_groups, bool) or not isinstance(num_groups, int) or num_groups < 0:
            raise ValueError(f"num_groups must be a non-negative int, got {num_groups!r}")
        g = num_groups
        dev = self.device
        sums = torch.zeros((g, self.dim), dtype=torch.float64, device=dev)
        counts = torch.zeros(g, dtype=torch.int64, device=dev)
        if g == 0 or n == 0:
            return sums, counts
        lab = labels.to(device=dev, dtype=torch.int64)
        key = torch.where((lab >= 0) & (lab < g), lab, g)  # the rows without a group sort behind every group
        skey, order = torch.sort(key, stable=True)
        offsets = torch.searchsorted(skey, torch.arange(g + 1, dtype=torch.int64, device=dev)).to(torch.int64)
        self._group_sums(order.contiguous(), offsets.contiguous(), sums, counts)
        return sums, counts

    # ------------------------------------------------------------------ farthest-point selection
    _farthest_ws: Tensor | None = None  # the workspace of `_farthest_rows`, grown on demand like `_assign_ws`

    def _farthest_rows(self, start: Tensor, m: int, mask: RowFilter | None, out_rows: Tensor, out_cover: Tensor,
                       out_near: Tensor | None) -> None:
        """`isc_bank_farthest`: `out_rows` (int64 `[m]`, LOCAL rows, -1 past the last candidate) and `out_cover` (float32
        `[m]`) receive `m > 0` greedy picks after the centres `start` (int64 LOCAL rows on the device, possibly empty);
        `mask` (None: every live row) says which rows may be picked, the fill bitmap which are live.  `out_near`, unless
        None, is float32 `[capacity]` in ORIGINAL row order.  On the current stream, no host read.  A device hook."""
        lib = _lib.load()
        dev = self.device
        n = self.capacity
        code = _lib.dtype_code(self.dtype)
        need = _lib.c_size_t()
        _lib.check(lib.isc_bank_farthest_workspace_bytes(code, n, self.dim, need), "isc_bank_farthest_workspace_bytes")
        if self._farthest_ws is None or self._farthest_ws.numel() < need.value:
            self._farthest_ws = None
            self._farthest_ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        ws = self._farthest_ws
        rm = None if mask is None or mask.packed is self._fill else mask.packed.data_ptr()
        with torch.cuda.device(dev):
            st = lib.isc_bank_farthest(
                self._bank.data_ptr(), code, n, self.dim, start.data_ptr() if start.numel() else None, start.numel(), m,
                _lib.ptr(self._fill), rm, out_rows.data_ptr(), out_cover.data_ptr(), _lib.ptr(out_near), ws.data_ptr(),
                ws.numel(), _lib.stream_handle(dev),
            )
        _lib.check(st, "isc_bank_farthest")

    def farthest_points(self, m: int, *, start: "Tensor | Sequence[int] | None" = None,
                        mask: "RowFilter | Tensor | None" = None, return_near: bool = False) -> tuple[Tensor, ...]:
        """`m` rows that are as unlike each other as greedy farthest-point selection (k-center greedy) finds them: `idx`
        int64 `[m]` (global rows) and `cover` float32 `[m]`, and with `return_near` also `near` float32 `[len]`.

        `S(c, r)` is the score of stored row c as a query against stored row r (`scores(rows([c]), [r])` bit for bit) and
        `near(r)` the best `S(c, r)` over the centres so far, -inf with none; "best" is `search`'s order (score
        descending, NaN below every number, -0.0 equal to +0.0) and a tie keeps the earlier value.  Every live row of
        `start` (global rows; range-checked on the host like `rows`; may lie outside `mask`), in order, becomes a centre;
        a removed one is skipped.  Then, `m` times, the pick is the candidate -- a live row `mask` (`RowFilter` or bool
        `[N]`) allows that is neither picked nor in `start` -- whose `near` is LAST in that order, ties to the lower row;
        `cover[t]` is its `near` at that moment (the running worst-case similarity of the rows to the selection), and it
        becomes a centre.  When no candidate is left the remaining entries are `(-inf, -1)`.  Without `start` the first
        pick is the lowest allowed live row with cover -inf, and the answer to `m` is a prefix of the answer to any
        larger `m`.  `near` covers all centres, the last pick included, in row order; a removed row reads -inf.

        One float64 pass over the packed bank per centre (`isc_bank_farthest`), on the caller's current stream with no
        host read past the index check, so the call can be captured.  `m == 0` returns empty `idx` and `cover` without a
        launch (`near`, if asked for, is then -inf: no centre was scored).  A sharded bank cannot select."""
        self._refuse_sharded("select farthest points", self._ROWS_ON_ONE_RANK)
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= _lib.ISC_FARTHEST_MAX_PICKS:
            raise ValueError(f"m must be an int in [0, {_lib.ISC_FARTHEST_MAX_PICKS}], got {m!r}")
        index = self._local_index(start if start is not None else [], "start")
        rf = self._as_filter(mask)
        dev = self.device
        n = self.num_local_rows
        near = torch.full((self.capacity,), -math.inf, dtype=torch.float32, device=dev) if return_near else None
        if m == 0 or n == 0:
            idx = torch.full((m,), -1, dtype=torch.int64, device=dev)
            cover = torch.full((m,), -math.inf, dtype=torch.float32, device=dev)
        else:
            idx = torch.empty(m, dtype=torch.int64, device=dev)
            cover = torch.empty(m, dtype=torch.float32, device=dev)
            self._farthest_rows(index, m, rf, idx, cover, near)
            if self.index_base:
                idx = torch.where(idx >= 0, idx + self.index_base, idx)
        return (idx, cover, near[:n]) if return_near else (idx, cover)

    # ------------------------------------------------------------------ PCA on the packed image
    _gram_ws: Tensor | None = None  # the workspace of `_gram_rows`, grown on demand

    def _gram_rows(self, mean: Tensor, mask: RowFilter | None, gram: Tensor, count: Tensor) -> None:
        """`isc_bank_gram`: `gram` (float64 `[D, D]`, zeroed) receives the sum over the rows `mask` allows (None: the fill
        bitmap, if the bank has one) of `(row - mean) (row - mean)^T` with `mean` float32 `[D]`, and `count` (int64 `[1]`,
        zeroed) the number of those rows.  On the current stream, no host read.  A device hook."""
        lib = _lib.load()
        dev = self.device
        code = _lib.dtype_code(self.dtype)
        need = _lib.c_size_t()
        _lib.check(lib.isc_bank_gram_workspace_bytes(code, self.capacity, self.dim, need), "isc_bank_gram_workspace_bytes")
        if self._gram_ws is None or self._gram_ws.numel() < need.value:
            self._gram_ws = None
            self._gram_ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        ws = self._gram_ws
        rm = _lib.ptr(mask.packed) if mask is not None else _lib.ptr(self._fill)
        with torch.cuda.device(dev):
            st = lib.isc_bank_gram(
                self._bank.data_ptr(), code, self.capacity, self.dim, mean.data_ptr(), rm, gram.data_ptr(), gram.stride(0),
                count.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle(dev),
            )
        _lib.check(st, "isc_bank_gram")

    def _project_rows(self, mean: Tensor, w: Tensor, mask: RowFilter | None, out_rows: Tensor | None,
                      out_bank: "EmbeddingBank | None") -> None:
        """`isc_bank_project`: every row `mask` allows (None: the fill bitmap, if the bank has one) is projected once,
        `(row - mean) @ w` with `mean` float32 `[D]` and `w` float32 `[D, K]`, and goes to `out_rows` (float32
        `[capacity, K]`, zeros for the other rows) and / or into the packed image of `out_bank` (a K-wide bank laid out for
        the same capacity, image zeroed) with `out_bank`'s dtype, `normalize` and norm bound.  One launch on the current
        stream, no host read.  A device hook."""
        dev = self.device
        with torch.cuda.device(dev):
            st = _lib.load().isc_bank_project(
                self._bank.data_ptr(), _lib.dtype_code(self.dtype), self.capacity, self.dim, mean.data_ptr(), w.data_ptr(),
                w.shape[1], w.stride(0), _lib.ptr(mask.packed) if mask is not None else _lib.ptr(self._fill),
                _lib.ptr(out_rows), 0 if out_rows is None else out_rows.stride(0),
                None if out_bank is None else out_bank._bank.data_ptr(),
                _lib.dtype_code(self.dtype if out_bank is None else out_bank.dtype),
                0 if out_bank is None else int(out_bank.normalize), 1e-12,
                None if out_bank is None else out_bank._norm_bound.data_ptr(), _lib.stream_handle(dev),
            )
        _lib.check(st, "isc_bank_project")

    def _pca_operands(self, pca: object, what: str) -> tuple[Tensor, Tensor]:
        """(`feature_means` as float32 `[D]`, `component_vectors` as float32 `[D, K]`, unit inner stride) of a fitted PCA
        on this bank's device whose `num_features` is the bank's `dim`; ValueError otherwise."""
        self._refuse_sharded(what, self._ROWS_ON_ONE_RANK)
        if not getattr(pca, "fitted", False):
            raise ValueError("the PCA is not fitted")
        if pca.num_features != self.dim:
            raise ValueError(f"the PCA was fitted on {pca.num_features} features, the bank holds {self.dim}")
        mean, w = pca.feature_means, pca.component_vectors
        if mean.device != self.device or w.device != self.device:
            raise ValueError(f"the PCA is on {w.device} but the bank is on {self.device}; call pca.to() first")
        return mean.reshape(-1).float().contiguous(), w.float().contiguous()

    def projected_rows(self, pca: object) -> Tensor:
        """`pca.transform` of every stored row, float32 `[len, K]` in row order, read from the packed image
        (`isc_bank_project`): no unpacked copy of the bank is made.  A removed row comes back as zeros.  The centred row is
        formed in float32 from the stored value and multiplied on the f32 matrix cores.  `pca` is a fitted `PCA` on the
        bank's device with `num_features == dim` (ValueError otherwise).  Runs on the caller's current stream with no host
        read.  A sharded bank cannot project its rows."""
        mean, w = self._pca_operands(pca, "project its rows")
        n = self.num_local_rows
        out = torch.zeros((self.capacity, w.shape[1]), dtype=torch.float32, device=self.device)
        if n:
            self._project_rows(mean, w, self._as_filter(None), out, None)
        return out[:n]

    def project(self, pca: object, *, dtype: torch.dtype | None = None, normalize: bool = True) -> "EmbeddingBank":
        """The bank of the PCA-compressed rows: a new `EmbeddingBank` with `dim = pca.num_components` and `dtype` (default:
        this bank's) whose row i is `pca.transform` of this bank's row i, stored as `EmbeddingBank(rows, dtype=...,
        normalize=...)` would store it -- bit for bit: the projection kernel ends in the pack kernels' row function.  One
        launch reads the packed rows and writes the packed image of the new bank (`isc_bank_project`); neither an `[N, D]`
        nor an `[N, K]` row-major tensor exists at any time.

        The new bank has the same `len`, capacity, fill bitmap (a copy: removed rows stay removed, `num_removed` is kept),
        `row_origin`, row groups and `index_base` 0, so an index means the same row in both banks and every call works on
        it: `search`, `search_groups`, `exclude_group=`, `similarity_map`, `append`, `remove`, ...  Runs on the caller's
        current stream, behind everything this bank has issued on its own streams.  `pca`: as in `projected_rows`.  A
        sharded bank cannot be projected."""
        mean, w = self._pca_operands(pca, "be projected")
        dtype = self.dtype if dtype is None else dtype
        if dtype not in (torch.float16, torch.float32):
            raise ValueError(f"bank dtype must be float16 or float32, got {dtype}")
        k = w.shape[1]
        n = self.num_local_rows
        empty = torch.empty((0, k), dtype=torch.float32, device=self.device)
        if self.capacity == 0:
            return type(self)(empty, dtype=dtype, normalize=normalize, shadow=self.shadow)
        self._wait_for_issued()
        out = type(self)(empty, dtype=dtype, normalize=normalize, capacity=self.capacity, shadow=self.shadow)
        out.num_local_rows = n
        out._num_removed = self._num_removed
        if self._fill is None:  # nothing reserved, nothing removed: the new bank is searched without a mask too
            out._capacity = out._fill = out._fill_filter = None
        else:
            out._capacity = self._capacity
            out._fill = self._fill.clone()
            out._fill_filter = RowFilter(out, out._fill, None)
        if self.row_origin is not None:
            out.row_origin = self.row_origin.clone()
        if self.group_labels is not None:
            out.group_labels = self.group_labels.clone()
            out._row_codes = self._row_codes.clone()
            out._group_counts = None if self._group_counts is None else self._group_counts.clone()
            out._max_group_rows = self._max_group_rows
        if n:
            self._project_rows(mean, w, self._as_filter(None), None, out)
        return out

    def similarity_map(self, queries: Tensor, image_id: int) -> Tensor:
        """The score of every query against every cell of one image, on a bank with `row_origin` (`from_database`):
        float32 `[Q, H, W]` with H = the image's largest h + 1 and W = its largest w + 1; cells the bank does not hold, or
        has removed, are -inf.  An image no row of the bank belongs to raises ValueError.  Host indexing on `scores`."""
        self._refuse_sharded("map an image", self._ROWS_ON_ONE_RANK)
        if self.row_origin is None:
            raise ValueError("similarity_map needs row_origin: build the bank with EmbeddingBank.from_database")
        if self.row_origin.shape[0] != self.num_local_rows:
            raise ValueError("row_origin does not describe the bank's rows")
        q = self._prepare_queries(queries)
        origin = self.row_origin
        cells = (origin[:, 0] == int(image_id)).nonzero().squeeze(1)
        if cells.numel() == 0:
            raise ValueError(f"image_id {int(image_id)} is not in the bank")
        h, w = origin[cells, 1].to(self.device), origin[cells, 2].to(self.device)
        out = torch.full((q.shape[0], int(h.max()) + 1, int(w.max()) + 1), -math.inf, dtype=torch.float32,
                         device=self.device)
        out[:, h, w] = self.scores(q, cells + self.index_base)
        return out

    def label_map(self, vectors: Tensor, image_id: int, size: tuple[int, int], **kw: object) -> segmentation.LabelMaps:
        """Pixel labels of one stored image: `similarity_map(vectors, image_id)` upsampled to `size = (H, W)` with the arg
        max per pixel, `segmentation.label_map(similarity_map(...)[None], size, layout="bchw", **kw)` with B = 1 (`kw`:
        `class_of`, `min_score`, `return_*`).  A cell the bank does not hold, or has removed, scores -inf for every vector
        and goes through the blend as it is: a pixel with such a cell among its four scores -inf (a nonzero weight) or
        NaN (a zero weight) for every vector.  The pixels around a missing cell therefore come out `UNLABELED` under any
        finite `min_score` (pass one, e.g. -1, to mask them); with the threshold off only the NaN ones do, and the -inf
        ones carry the first vector's class with score -inf.  A sharded bank refuses the call, as it refuses
        `similarity_map`."""
        if "layout" in kw:
            raise TypeError("label_map takes no layout: similarity_map is [Q, H, W]")
        return segmentation.label_map(self.similarity_map(vectors, image_id)[None], size, layout="bchw", **kw)

    def search_rows(self, indices: "Tensor | Sequence[int]", k: int = 10, *, exclude_self: bool = True,
                    mask: "RowFilter | Tensor | None" = None,
                    exclude_group: "Tensor | str | None" = None) -> tuple[Tensor, Tensor]:
        """`search` with the stored vectors of the rows `indices` (global) as the queries -- "more cells like this stored
        cell".  The queries are gathered in the bank dtype (`isc_bank_gather`), so rounding them to the bank dtype is the
        identity and the answer is `search(rows(indices), k, ...)` bit for bit.  `mask`, `exclude_group`: as in `search`;
        in addition `exclude_group="own"` makes every query skip its own row's group ("in other images"): the query codes
        are the rows' stored codes, read on the device, so the bank must have row groups.

        `exclude_self=True` (default) keeps a query's own row out of its answer.  With `"own"` the group exclusion already
        does.  Otherwise `k + 1` entries are searched and, per query, the entry whose index is the query's own row is
        dropped, or the last entry when the own row is not among them (the mask or the group exclusion disallows it, or
        `k + 1` exact copies with lower indices precede it); the order is total, so what remains is exactly the top-k of
        the rows other than the query's own.  Then `1 <= k <= min(ISC_TOPK_MAX_K - 1, len - 1)`.

        A removed row among `indices` raises ValueError (one host read, only while `num_removed > 0`).  Everything else is
        enqueued on the caller's current stream.  A sharded bank cannot search by row."""
        self._refuse_sharded("search by row", self._ROWS_ON_ONE_RANK)
        index = self._local_index(indices, "indices")
        self._check_k(k)
        own = isinstance(exclude_group, str)
        if own and exclude_group != "own":
            raise ValueError(f"exclude_group must be a label tensor or 'own', got {exclude_group!r}")
        if own and self.group_labels is None:
            raise ValueError("exclude_group='own' needs row groups: build the bank with row_groups= (or from_database)")
        drop = bool(exclude_self) and not own
        if drop and k > min(_lib.ISC_TOPK_MAX_K, self.num_local_rows) - 1:
            raise ValueError(f"k={k} must be in [1, {min(_lib.ISC_TOPK_MAX_K, self.num_local_rows) - 1}] with "
                             "exclude_self=True: each query's own row is searched too and then dropped")
        if self._num_removed and index.numel() and not bool(self.live[index].all()):
            raise ValueError("indices name a removed row: it has no stored vector to search with")
        q = torch.empty((index.numel(), self.dim), dtype=self.dtype, device=self.device)
        if index.numel():
            self._gather_rows(index, q)
        codes = self._stored_codes(index) if own else None
        scores, found = self._search(q, k + 1 if drop else k, lanes=False, mask=mask,
                                     exclude_group=None if own else exclude_group, query_codes=codes).result()
        if not drop:
            return scores, found
        hit = found == (index + self.index_base)[:, None]  # at most one entry per query: a result names a row once
        at = torch.where(hit.any(dim=1), hit.to(torch.uint8).argmax(dim=1), k)  # the own row's position, or the last
        cols = torch.arange(k, device=found.device)[None, :]
        cols = cols + (cols >= at[:, None])
        return scores.gather(1, cols), found.gather(1, cols)

    # ------------------------------------------------------------------ collapsed search
    def _labels_of(self, codes: Tensor) -> Tensor:
        """int64 labels of int32 group codes (`group_labels[code]`); -1 for the padding's code -1.  Tensor ops only."""
        labels = self.group_labels
        if labels is None or labels.numel() == 0:
            return torch.full(codes.shape, -1, dtype=torch.int64, device=codes.device)
        return torch.where(codes >= 0, labels[codes.clamp(min=0).long()], -1)

    def _local_collapse(self, queries: Tensor, k: int, out: tuple[Tensor, Tensor, Tensor] | None = None,
                        mask: RowFilter | None = None, groups: Tensor | None = None) -> tuple[Tensor, Tensor, Tensor]:
        """The k best groups of this rank's rows (`isc_cosine_topk_collapse`): `(scores float32 [Q, k], indices int64
        [Q, k] GLOBAL rows, labels int64 [Q, k])` with the C ABI's padding (NaN, INT64_MAX, label -1), final when the stream
        has run the call.  `out`: optional (scores, indices, status int32[4]) to write into; `mask` / `groups`: as in
        `_local_topk`.  The device hook a CPU rehearsal replaces."""
        nq = queries.shape[0]
        scores, indices, status = out if out is not None else self._new_out(nq, k)
        codes = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        ws = self._workspace(nq, k, collapse=True)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            st = lib.isc_cosine_topk_collapse(
                self._bank.data_ptr(), _lib.dtype_code(self.dtype), self.capacity, self.dim, queries.data_ptr(),
                _lib.dtype_code(queries.dtype), nq, queries.stride(0), k, self.index_base, self._norm_bound.data_ptr(),
                scores.data_ptr(), indices.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                None if mask is None else mask.packed.data_ptr(), self._row_codes.data_ptr(),
                None if groups is None else groups.data_ptr(), max(self._max_group_rows, 1), codes.data_ptr(),
                _lib.stream_handle(self.device),
            )
        _lib.check(st, "isc_cosine_topk_collapse")
        self.last_status = status
        return scores, indices, self._labels_of(codes)

    def _merge_groups(self, scores: Tensor, indices: Tensor, labels: Tensor, k: int) -> tuple[Tensor, Tensor, Tensor]:
        """Merge `[G, Q, kin]` collapsed partial results into `[Q, k]` (`isc_topk_merge_groups`): the best entry per label,
        then the best k.  The inputs may be strided along G; their `[Q, kin]` blocks are dense."""
        g, nq, kin = scores.shape
        ts = (scores, indices, labels)
        if any(t.stride(1) != kin or t.stride(2) != 1 for t in ts):
            scores, indices, labels = (t.contiguous() for t in ts)
        out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
        out_i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
        out_l = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
        lib = _lib.load()
        with torch.cuda.device(scores.device):
            st = lib.isc_topk_merge_groups(
                scores.data_ptr(), indices.data_ptr(), labels.data_ptr(), g, nq, kin, k,
                scores.stride(0) if g > 1 else 0, indices.stride(0) if g > 1 else 0, labels.stride(0) if g > 1 else 0,
                out_s.data_ptr(), out_i.data_ptr(), out_l.data_ptr(), _lib.stream_handle(scores.device),
            )
        _lib.check(st, "isc_topk_merge_groups")
        return out_s, out_i, out_l

    def _check_k(self, k: int, limit: int = _lib.ISC_TOPK_MAX_K) -> None:
        """`limit`: `ISC_TOPK_MAX_K`, or `ISC_TOPK_LARGE_MAX_K` for the calls that have a large-k path."""
        if not isinstance(k, int) or isinstance(k, bool):
            raise TypeError(f"k must be an int, got {type(k).__name__}")
        if k < 1:
            raise ValueError(f"k must be >= 1, got {k}")
        if k > limit:
            raise ValueError(f"k must be <= {limit}, got {k}")

    @staticmethod
    def _filter_kwargs(rf: RowFilter | None, qg: Tensor | None) -> dict[str, object]:
        """`mask=` / `groups=` of a local search hook, each only when set (a hook without that filter need not know the
        argument).  A filtered search (non-empty) pads short answers; the grouped kernels get the query codes."""
        filt: dict[str, object] = {} if rf is None else {"mask": rf}
        if qg is not None:
            filt["groups"] = qg
        return filt

    def _empty_topk(self, k: int, labels: bool = False) -> tuple[Tensor, ...]:
        """The answer to no query: `(scores [0, k], indices [0, k])` and, with `labels`, the labels."""
        dtypes = (torch.float32, torch.int64, torch.int64) if labels else (torch.float32, torch.int64)
        return tuple(torch.empty((0, k), dtype=dt, device=self.device) for dt in dtypes)

    def search_groups(self, queries: Tensor, k: int = 10, *, mask: "RowFilter | Tensor | None" = None,
                      exclude_group: Tensor | None = None) -> tuple[Tensor, Tensor, Tensor]:
        """The k best GROUPS per query ("which images look like this region?") on a bank built with `row_groups=` (or
        `from_database`, grouped by image id).  A group's key is the best (score desc with NaN last, row asc) among the rows
        the query may return (`mask`, `exclude_group`: as in `search`); that row is the group's leader.

        Returns `(scores float32 [Q, k], indices int64 [Q, k], groups int64 [Q, k])`: per entry the leader's score, its
        global row index and the group's label, best group first.  A query with fewer than k groups it may return ends in
        padding: score -inf, index -1, label -1 (test the index: -1 can be a real label).  `1 <= k <= min(rows, 120)`.

        Exact like `search`: on a bank whose rows are each their own group the answer is `search(q, k)`, bit for bit.
        No host synchronisation, so a world-1 call may be captured into a graph.  `last_status` keeps its meaning ([1]:
        queries the first pass could not prove, [3]: queries answered by the float64 sweep).  A sharded bank all-gathers
        every rank's collapsed list with its labels and keeps the best entry per label."""
        rf = self._as_filter(mask)
        self._check_k(k)
        q = self._prepare_queries(queries)
        nq = q.shape[0]
        if self.group_labels is None:
            raise ValueError("search_groups needs row groups: build the bank with row_groups= (or from_database)")
        filt = self._filter_kwargs(rf, self._query_codes(exclude_group, nq))
        n_rows = self.num_local_rows if self.process_group is None else self._global_rows()
        if k > n_rows:
            raise ValueError(f"k={k} exceeds the bank size {n_rows}")
        if nq == 0:
            return self._empty_topk(k, labels=True)
        if self.process_group is None:
            return _unpad_groups(*self._local_collapse(q, k, **filt))

        # sharded like `_search`, but not pipelined: a fresh exchange buffer per call, the all-gather on the caller's stream
        nbytes, views = _exchange_layout(nq, k, with_labels=True)
        xbuf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        part_s, part_i, part_l, status = views(xbuf)
        kl = min(k, self.num_local_rows)
        if kl < k:
            self._short_shard(self._local_collapse, q, kl, filt, (part_s, part_i, part_l), status, math.nan)
        else:
            _, _, lab = self._local_collapse(q, k, out=(part_s, part_i, status), **filt)
            part_l.copy_(lab)
        all_s, all_i, all_l, self.last_gathered_status = views(self._all_gather_bytes(xbuf))
        return _unpad_groups(*self._merge_groups(all_s, all_i, all_l, k))

    def search_groups_exhaustive(self, queries: Tensor, k: int = 10, *, mask: "RowFilter | Tensor | None" = None,
                                 exclude_group: Tensor | None = None) -> tuple[Tensor, Tensor, Tensor]:
        """`search_groups` from the data-independent float64 kernel (`isc_cosine_topk_exhaustive_collapse`): every score
        evaluated exactly, one shard.  Slow; the on-device reference the fast path is tested against."""
        rf = self._as_filter(mask)
        self._check_k(k)
        q = self._prepare_queries(queries)
        nq = q.shape[0]
        if self.group_labels is None:
            raise ValueError("search_groups_exhaustive needs row groups: build the bank with row_groups= (or from_database)")
        qg = self._query_codes(exclude_group, nq)
        if self.process_group is not None:
            raise ValueError("search_groups_exhaustive answers for one shard; merge the shards with search_groups()")
        if not 1 <= k <= self.num_local_rows:
            raise ValueError(f"k={k} must be in [1, {self.num_local_rows}]")
        if nq == 0:
            return self._empty_topk(k, labels=True)
        lib = _lib.load()
        code = _lib.dtype_code(self.dtype)
        need = _lib.c_size_t()
        _lib.check(lib.isc_cosine_topk_exhaustive_collapse_workspace_bytes(code, self.capacity, self.dim, nq, k,
                                                                           need),
                   "isc_cosine_topk_exhaustive_collapse_workspace_bytes")
        ews = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        indices = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        codes = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            st = lib.isc_cosine_topk_exhaustive_collapse(
                self._bank.data_ptr(), code, self.capacity, self.dim, q.data_ptr(), _lib.dtype_code(q.dtype), nq,
                q.stride(0), k, self.index_base, scores.data_ptr(), indices.data_ptr(), ews.data_ptr(), ews.numel(),
                None if rf is None else rf.packed.data_ptr(), self._row_codes.data_ptr(),
                None if qg is None else qg.data_ptr(), codes.data_ptr(), _lib.stream_handle(self.device),
            )
        _lib.check(st, "isc_cosine_topk_exhaustive_collapse")
        return _unpad_groups(scores, indices, self._labels_of(codes))

    # ------------------------------------------------------------------ range search
    # Entries the first attempt of a range search reserves per query; a larger result costs one more call with the exact
    # capacity the first one reported.
    _RANGE_GUESS_PER_QUERY = 2048

    def _range_thresholds(self, min_score: "float | Tensor", nq: int) -> Tensor:
        if isinstance(min_score, Tensor):
            if min_score.shape != (nq,):
                raise ValueError(f"min_score must be a float or a [Q] = [{nq}] tensor, got shape {tuple(min_score.shape)}")
            if min_score.dtype != torch.float32:
                raise TypeError(f"min_score tensor must be float32, got {min_score.dtype}")
            if bool(torch.isnan(min_score).any()):
                raise ValueError("min_score contains NaN")
            return min_score.to(self.device).contiguous()
        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)):
            raise TypeError(f"min_score must be a float or a float32 tensor, got {type(min_score).__name__}")
        if math.isnan(min_score):
            raise ValueError("min_score is NaN")
        return torch.full((nq,), float(min_score), dtype=torch.float32, device=self.device)

    def _empty_range(self, nq: int) -> RangeResult:
        return RangeResult(torch.zeros(nq + 1, dtype=torch.int64, device=self.device),
                           torch.empty(0, dtype=torch.float32, device=self.device),
                           torch.empty(0, dtype=torch.int64, device=self.device))

    def _range_call(self, q: Tensor, thr: Tensor, capacity: int, mask: RowFilter | None = None,
                    groups: Tensor | None = None) -> tuple[int, RangeResult, Tensor]:
        """One `isc_cosine_range` call: (needed, result -- valid only when needed <= capacity --, status int32[4])."""
        lib = _lib.load()
        nq = q.shape[0]
        code = _lib.dtype_code(self.dtype)
        need = _lib.c_size_t()
        _lib.check(lib.isc_cosine_range_workspace_bytes(code, self.capacity, self.dim, nq, capacity, need),
                   "isc_cosine_range_workspace_bytes")
        if self._range_ws is None or self._range_ws.numel() < need.value:
            self._range_ws = None
            self._range_ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        ws = self._range_ws
        offsets = torch.empty(nq + 1, dtype=torch.int64, device=self.device)
        scores = torch.empty(capacity, dtype=torch.float32, device=self.device)
        indices = torch.empty(capacity, dtype=torch.int64, device=self.device)
        needed = torch.empty(1, dtype=torch.int64, device=self.device)
        status = torch.empty(4, dtype=torch.int32, device=self.device)
        args = (
            self._bank.data_ptr(), code, self.capacity, self.dim, q.data_ptr(), _lib.dtype_code(q.dtype), nq,
            q.stride(0), thr.data_ptr(), self.index_base, self._norm_bound.data_ptr(), capacity,
            offsets.data_ptr(), scores.data_ptr(), indices.data_ptr(), needed.data_ptr(), status.data_ptr(),
            ws.data_ptr(), ws.numel(),
        )
        self._row_search("isc_cosine_range", args, mask, groups, _lib.stream_handle(self.device))
        return int(needed.item()), RangeResult(offsets, scores, indices), status

    def _local_range(self, queries: Tensor, min_score: Tensor, max_results: int, mask: RowFilter | None = None,
                     groups: Tensor | None = None) -> tuple[int, RangeResult | None]:
        """Range search of this rank's rows with GLOBAL row indices: `(total, result)`; `result` is None when `total`
        exceeds `max_results` (then `total` is the exact row count, or, when even counting would need more than twice
        `max_results` entries, the filter's candidate count, an upper bound of it)."""
        nq = queries.shape[0]
        if self.num_local_rows == 0 or nq == 0:
            return 0, self._empty_range(nq)
        limit = min(max(max_results, 1), 0x7FFFFFFF)
        cap = min(max(1 << 16, self._RANGE_GUESS_PER_QUERY * nq), limit)
        grp = {} if groups is None else {"groups": groups}
        needed, res, status = self._range_call(queries, min_score, cap, mask, **grp)
        if needed > cap:
            if needed > 2 * limit or needed > 0x7FFFFFFF:
                self.last_range_status = status
                return needed, None
            needed, res, status = self._range_call(queries, min_score, needed, mask, **grp)
        self.last_range_status = status
        total = int(res.offsets[-1].item())
        if total > max_results:
            return total, None
        return total, RangeResult(res.offsets, res.scores[:total], res.indices[:total])

    def search_range(self, queries: Tensor, min_score: "float | Tensor", *, max_results: int = 1 << 26,
                     mask: "RowFilter | Tensor | None" = None, exclude_group: Tensor | None = None) -> RangeResult:
        """Every row whose cosine score against a query is >= `min_score` (a float, or a float32 `[Q]` tensor of
        per-query thresholds): a `RangeResult` whose query q holds its rows ordered by (score descending, row index
        ascending), indices global.  Exact: the scores and the membership are those of the top-k (`search`), so with
        t = the k-th score of `search(q, k)` the first k rows of `search_range(q, t)` are `search(q, k)`.  NaN scores
        are never in a result.

        The call synchronises the host to size the output (like `torch.nonzero`), so it cannot be captured into a graph
        (capture `isc_cosine_range` itself with a fixed capacity instead); a result larger than the first
        internal guess costs a second device call of the exact size.  More than `max_results` rows in all raise
        ValueError with the count.  `last_range_status` (int32[4], device) holds diagnostics: [0] filter candidates,
        [1] queries answered by the float64 sweep, [2] float bits of the largest filter error in units of its bound.
        A sharded bank searches its shard on every rank, all-gathers the per-rank totals and then the rows, and every
        rank merges them into the answer of the unsharded bank.  `mask`: as in `search` -- the result without the rows the
        filter disallows, bit for bit.  `exclude_group`: as in `search` -- query q's result without the rows of its group."""
        rf = self._as_filter(mask)
        q = self._prepare_queries(queries)
        nq = q.shape[0]
        qg = self._query_codes(exclude_group, nq)
        thr = self._range_thresholds(min_score, nq)
        if isinstance(max_results, bool) or not isinstance(max_results, int) or max_results < 0:
            raise ValueError(f"max_results must be a non-negative int, got {max_results!r}")
        if qg is not None:
            total, res = self._local_range(q, thr, max_results, rf, groups=qg)
        else:
            total, res = self._local_range(q, thr, max_results) if rf is None else self._local_range(q, thr, max_results, rf)
        if self.process_group is None:
            if res is None:
                raise ValueError(f"search_range found {total} rows, more than max_results={max_results}")
            return res
        return self._exchange_range(nq, total, res, max_results)

    def _exchange_range(self, nq: int, total: int, res: RangeResult | None, max_results: int) -> RangeResult:
        """Two all-gathers (per-rank totals, then the padded rows) and the merge into (query, score desc, index asc)
        order.  Every rank issues the same collectives whatever its shard holds."""
        g = self.world_size
        dev = self.device
        tot = torch.tensor([total, 0 if res is not None else 1], dtype=torch.int64, device=dev)
        all_tot = self._all_gather_bytes(tot.view(torch.uint8)).view(torch.int64).view(g, 2).cpu()
        merged = int(all_tot[:, 0].sum())
        if merged > max_results or bool(all_tot[:, 1].any()):
            raise ValueError(f"search_range found {merged}{'' if not all_tot[:, 1].any() else ' or more'} rows, more "
                             f"than max_results={max_results}")
        if merged == 0:
            return self._empty_range(nq)
        width = int(all_tot[:, 0].max())
        # payload of this rank: [query int64 | index int64 | score float32 (as 8 bytes)] x width, padding rows unused
        pay = torch.zeros((3, width), dtype=torch.int64, device=dev)
        if total:
            assert res is not None
            pay[0, :total] = torch.repeat_interleave(torch.arange(nq, device=dev), res.counts)
            pay[1, :total] = res.indices
            pay[2, :total] = res.scores.to(torch.float64).view(torch.int64)
        gathered = self._all_gather_bytes(pay.view(-1).view(torch.uint8)).view(torch.int64).view(g, 3, width)
        keep = torch.arange(width, device=dev)[None, :] < all_tot[:, 0].to(dev)[:, None]  # [G, width]
        qs = gathered[:, 0][keep]
        idx = gathered[:, 1][keep]
        sc = gathered[:, 2][keep].view(torch.float64).to(torch.float32)
        # ranks are gathered in row order and each rank's rows of a query come index-ascending within a score, so two
        # stable sorts -- score descending, then query -- give (query, score desc, index asc)
        order = torch.sort(sc, descending=True, stable=True).indices
        qs, idx, sc = qs[order], idx[order], sc[order]
        order = torch.sort(qs, stable=True).indices
        qs, idx, sc = qs[order], idx[order], sc[order]
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(torch.bincount(qs, minlength=nq), 0)
        return RangeResult(offsets, sc, idx)
