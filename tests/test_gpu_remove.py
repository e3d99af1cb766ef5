"""In-place `remove`, `replace` and `compact` of `EmbeddingBank` (isc_bank_remove, isc_bank_replace, isc_bank_repack_map,
isc_row_mask_unpack) on the GPU.  Every comparison is exact (`assert_array_equal`), against one of two references:

- rule 1, "remove equals mask": a bank after `remove(rows=R)` answers every search as an untouched twin bank does with
  `mask = row_filter(rows=R, exclude=True)` (ANDed with the caller's own mask);
- rule 4, "compact equals a fresh bank": after `compact()` the bank is, in everything a caller can see, the bank built from
  the surviving rows at once (and `replace` gives the bank built with the new vectors substituted).

The shapes are the boundary shapes of tests/test_gpu_append.py: D = 40 fp16 and D = 72 fp32 / fp16 with mixed input dtypes,
banks of 255 rows in capacity 257, 300 in 513, 300 filled to 512 (full) and a never-reserved bank of 300 -- a tile boundary
at 256, mask-word boundaries at 32, spare room and none -- and its (Q, k) grid, one pair per step."""

from __future__ import annotations

import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))

import cases  # noqa: E402

from oracle import search_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

QK = ((1, 1), (65, 10), (130, 120), (1, 10), (65, 120), (130, 1), (1, 120), (65, 1), (130, 10))  # Q x k, one per step
F16, F32 = torch.float16, torch.float32
# name: (D, bank dtype, input dtype, normalize, rows at the start, capacity= (None: nothing reserved), rows appended at once)
BANKS = {
    "255-257": (72, F16, F16, False, 255, 257, 0),
    "300-513": (72, F16, F32, True, 300, 513, 0),
    "300-512-full": (40, F16, F16, True, 300, 512, 212),
    "300-plain": (72, F32, F16, False, 300, None, 0),
}


def _rows(n: int, d: int, dtype: torch.dtype, seed: int, unit: bool = True) -> torch.Tensor:
    x = torch.randn(n, d, generator=cases.gen(seed))
    return (torch.nn.functional.normalize(x, dim=1) if unit else x * 3.0).to(dtype)


def _labels(n: int, seed: int) -> torch.Tensor:
    return torch.randint(2, 14, (n,), generator=cases.gen(500 + seed)) * 10  # 20, 30, ..., 130


def _queries(nq: int, d: int, dtype: torch.dtype, seed: int, device: torch.device) -> torch.Tensor:
    return torch.randn(nq, d, generator=cases.gen(1000 + seed)).to(dtype).to(device)


def _make(rows: torch.Tensor, labels: torch.Tensor | None, device: torch.device, dtype, normalize, capacity=None):
    from imagescry_amd import EmbeddingBank

    kw = {} if capacity is None else {"capacity": capacity}
    if labels is not None:
        kw["row_groups"] = labels
    return EmbeddingBank(rows.to(device), dtype=dtype, normalize=normalize, **kw)


def _data(name: str) -> tuple[torch.Tensor, torch.Tensor]:
    d, _, in_dtype, normalize, start, _, extra = BANKS[name]
    n = start + extra
    return _rows(n, d, in_dtype, 1, unit=not normalize), _labels(n, 1)


def _build(name: str, device: torch.device, grouped: bool = True):
    """The bank `name`, grouped by `_labels`: built with its start rows and, for the full one, filled by one append."""
    d, dtype, _, normalize, start, capacity, extra = BANKS[name]
    rows, labels = _data(name)
    eb = _make(rows[:start], labels[:start] if grouped else None, device, dtype, normalize, capacity)
    if extra:
        eb.append(rows[start:].to(device), **({"row_groups": labels[start:]} if grouped else {}))
        assert len(eb) == eb.capacity
    return eb


_TWINS: dict[str, object] = {}


def _twin(name: str, device: torch.device):
    """The untouched twin of bank `name`: built once, shared by every test, never changed."""
    if name not in _TWINS:
        _TWINS[name] = _build(name, device)
    return _TWINS[name]


def _same(got, exp, what: str = "") -> None:
    np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1].cpu().numpy(), err_msg=what)
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0].cpu().numpy(), err_msg=what)  # NaN == NaN here
    for g, e in zip(got[2:], exp[2:]):
        np.testing.assert_array_equal(g.cpu().numpy(), e.cpu().numpy(), err_msg=what)


def _same_range(got, exp, what: str = "") -> None:
    for field in ("offsets", "indices", "scores"):
        np.testing.assert_array_equal(getattr(got, field).cpu().numpy(), getattr(exp, field).cpu().numpy(), err_msg=what)


def _all_searches(eb, ref, step: int, device: torch.device, labels: torch.Tensor, what: str, kws) -> None:
    """`eb` against `ref` through `search` (the step's (Q, k)), `search_exhaustive`, `search_range` (thresholds = the 5th
    scores) and, on grouped banks, `search_groups`; `kws` is a list of (keywords for eb, keywords for ref) pairs.
    `exclude_group` holds 130 labels: each call takes the first Q."""
    assert len(eb) == len(ref)
    nq, k = QK[step % len(QK)]
    k = min(k, len(eb))
    q = _queries(nq, eb.dim, eb.dtype, step, device)
    q65 = _queries(65, eb.dim, eb.dtype, step + 50, device)
    k5 = min(5, len(eb))
    for kw_eb, kw_ref in kws:
        tag = f"{what} step {step} {sorted(kw_eb)}"

        def cut(kw, n):
            return {key: v[:n] if key == "exclude_group" else v for key, v in kw.items()}

        _same(eb.search(q, k, **cut(kw_eb, nq)), ref.search(q, k, **cut(kw_ref, nq)), tag + f" search Q={nq} k={k}")
        top = ref.search_exhaustive(q65, k5, **cut(kw_ref, 65))
        _same(eb.search_exhaustive(q65, k5, **cut(kw_eb, 65)), top, tag + " exhaustive")
        thr = top[0][:, -1].clamp(min=-2.0).contiguous()  # (-inf padding: every row the query may return)
        _same_range(eb.search_range(q65, thr, **cut(kw_eb, 65)), ref.search_range(q65, thr, **cut(kw_ref, 65)),
                    tag + " range")
        if eb.group_labels is not None:
            _same(eb.search_groups(q, k, **cut(kw_eb, nq)), ref.search_groups(q, k, **cut(kw_ref, nq)),
                  tag + f" groups Q={nq} k={k}")


def _removed_equals_masked(eb, twin, gone: torch.Tensor, step: int, device: torch.device, labels: torch.Tensor,
                           what: str = "") -> None:
    """Rule 1.  `gone`: bool [len], the rows removed from `eb` so far; `twin` holds the same rows, none removed."""
    n = len(eb)
    assert len(twin) == n and eb.num_removed == int(gone.sum())
    np.testing.assert_array_equal(eb.live.cpu().numpy(), (~gone).numpy(), err_msg=what)
    keep = twin.row_filter((~gone).to(device))
    assert int(keep.allowed_count) == n - int(gone.sum())
    allow = torch.rand(n, generator=cases.gen(300 + step)) < 0.5
    both = twin.row_filter((allow & ~gone).to(device))
    mine = eb.row_filter(allow.to(device))  # ANDed with `live`
    assert int(mine.allowed_count) == int(both.allowed_count) == int((allow & ~gone).sum())
    excl = labels[torch.randint(0, n, (130,), generator=cases.gen(400 + step))].clone()
    excl[3] = 12345  # a label no row carries
    _all_searches(eb, twin, step, device, labels, what,
                  [({}, {"mask": keep}), ({"mask": mine}, {"mask": both}), ({"mask": allow.to(device)}, {"mask": both}),
                   ({"exclude_group": excl}, {"mask": keep, "exclude_group": excl})])


def _rows_at_positions(capacity: int, n: int, positions) -> list[int]:
    """The rows < n that the packed positions `positions` of a bank laid out for `capacity` rows hold."""
    from imagescry_amd import _lib

    mul, inv = ctypes.c_int64(), ctypes.c_int64()
    assert _lib.load().isc_bank_permutation(capacity, mul, inv) == 0
    return [r for r in ((mul.value * p) % capacity for p in positions) if r < n]


def _removal_sets(name: str, n: int, capacity: int, labels: torch.Tensor) -> dict[str, tuple]:
    """name -> (selector keyword, its value, the rows it names, forced step or None)."""
    word = _rows_at_positions(capacity, n, range(64, capacity))[:33]  # 33 neighbours in the bitmap: two or three words
    group = int(labels[7])
    tile = sorted(set(range(250, min(n, 262))) | set(_rows_at_positions(capacity, n, range(250, 262))))
    most = list(range(n))
    for r in (3, 200, n - 1):
        most.remove(r)
    return {
        "one": ("rows", [n // 2], [n // 2], None),
        "word33": ("rows", torch.tensor(word), word, None),
        "group": ("groups", [group], torch.nonzero(labels == group).squeeze(1).tolist(), None),
        "tile-boundary": ("rows", tile, tile, None),
        "all-but-3": ("rows", torch.tensor(most, dtype=torch.int32), most, 1),  # (Q, k) = (65, 10): k pads
        "all": ("rows", range(n), list(range(n)), 1),  # every entry (-inf, -1)
        "twice": ("rows", word[:20] + word[:20], word[:20], None),
    }


@pytest.mark.parametrize("which", ["one", "word33", "group", "tile-boundary", "all-but-3", "all", "twice"])
@pytest.mark.parametrize("name", list(BANKS))
def test_remove_equals_mask(name: str, which: str, device: torch.device) -> None:
    _, labels = _data(name)
    eb, twin = _build(name, device), _twin(name, device)
    n, capacity, image = len(eb), eb.capacity, eb._bank.data_ptr()
    kw, value, named, forced = _removal_sets(name, n, capacity, labels)[which]
    step = forced if forced is not None else list(BANKS).index(name) * 2 + len(which)
    assert eb.remove(**{kw: value}) == len(set(named))
    assert len(eb) == n and eb.capacity == capacity and eb._bank.data_ptr() == image and eb._as_filter(None) is not None
    if which == "twice":
        assert eb.remove(rows=named) == 0 and eb.num_removed == len(named)
    gone = torch.zeros(n, dtype=torch.bool)
    gone[named] = True
    assert torch.equal(eb.bank.view(torch.uint8), twin.bank.view(torch.uint8))  # row bytes are not touched
    _removed_equals_masked(eb, twin, gone, step, device, labels, f"{name} {which}")
    if which == "all":
        s, i = eb.search(_queries(65, eb.dim, eb.dtype, 2, device), 10)
        assert bool((i == -1).all()) and bool(torch.isneginf(s).all())
    if which == "all-but-3":
        s, i = eb.search(_queries(65, eb.dim, eb.dtype, 2, device), 10)
        assert sorted(i[0].tolist()) == [-1] * 7 + [3, 200, n - 1] and bool(torch.isneginf(s[:, 3:]).all())
    if which == "group":  # the group is gone from the collapsed answer
        assert not bool((eb.search_groups(_queries(65, eb.dim, eb.dtype, 3, device), 5)[2] == int(labels[7])).any())


def _oracle_topk(stored: torch.Tensor, q: torch.Tensor, k: int) -> tuple[np.ndarray, np.ndarray]:
    s = search_oracle.exact_scores(stored, q.cpu().to(stored.dtype))
    idx = np.arange(s.shape[1])
    order = np.stack([np.lexsort((idx, -s[i].astype(np.float64)))[:k] for i in range(s.shape[0])])
    return np.take_along_axis(s, order, axis=1), order.astype(np.int64)


@pytest.mark.parametrize("name", ["255-257", "300-plain"])
def test_small_banks_against_the_float64_oracle(name: str, device: torch.device) -> None:
    eb = _build(name, device, grouped=False)
    n = len(eb)
    gone = torch.rand(n, generator=cases.gen(31)) < 0.3
    gone[250:] = True
    assert eb.remove(rows=torch.nonzero(gone).squeeze(1).to(device)) == int(gone.sum())
    alive = torch.nonzero(~gone).squeeze(1)
    for nq, k in ((65, 10), (130, 120), (1, 1)):
        q = _queries(nq, eb.dim, eb.dtype, 40 + nq, device)
        exp_s, exp_i = _oracle_topk(eb.bank.cpu()[alive], q, k)
        got = eb.search(q, k)
        np.testing.assert_array_equal(got[1].cpu().numpy(), alive.numpy()[exp_i])
        np.testing.assert_array_equal(got[0].cpu().numpy(), exp_s)


def _fresh_with(name: str, device: torch.device, vec: dict, normalize_new: bool, capacity: int):
    """The bank `name` built with the vectors `vec` (row -> vector, in the dtype it arrived in) in place of its own rows:
    runs of old rows and single new rows appended in row order, each stored with its own input dtype and normalisation --
    by tests/test_gpu_append.py that is the bank built from those rows at once."""
    from imagescry_amd import EmbeddingBank

    d, dtype, _, bank_norm, _, _, _ = BANKS[name]
    rows, labels = _data(name)
    n = rows.shape[0]
    fb = EmbeddingBank(torch.empty(0, d, device=device), dtype=dtype, capacity=capacity,
                       row_groups=torch.empty(0, dtype=torch.int64))
    r = 0
    while r < n:
        if r in vec:
            fb.append(vec[r][None].to(device), row_groups=labels[r : r + 1], normalize=normalize_new)
            r += 1
        else:
            hi = r
            while hi < n and hi not in vec:
                hi += 1
            fb.append(rows[r:hi].to(device), row_groups=labels[r:hi], normalize=bank_norm)
            r = hi
    return fb


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", ["300-513", "300-512-full", "300-plain"])
def test_replace_equals_the_bank_built_with_the_new_vectors(name: str, normalize: bool, device: torch.device) -> None:
    d, _, in_dtype, _, _, _, _ = BANKS[name]
    _, labels = _data(name)
    eb = _build(name, device)
    n, image, had_fill = len(eb), eb._bank.data_ptr(), eb._fill is not None
    idx = torch.cat([torch.arange(250, 262), torch.tensor([0, 31, 32, n - 1])])  # both sides of 256
    idx = idx[torch.randperm(idx.numel(), generator=cases.gen(7))]
    new = _rows(idx.numel(), d, F32 if in_dtype == F16 else F16, 77, unit=not normalize)  # the other input dtype
    if not normalize:
        new[2] *= 2.0  # raises the norm bound
    eb.replace(idx.to(device), new.to(device), normalize=normalize)
    assert eb._bank.data_ptr() == image and (eb._fill is not None) == had_fill and len(eb) == n
    vec = {int(r): new[j] for j, r in enumerate(idx.tolist())}
    fresh = _fresh_with(name, device, vec, normalize, eb.capacity)
    assert torch.equal(eb.bank.view(torch.uint8), fresh.bank.view(torch.uint8))
    assert float(eb._norm_bound) >= float(fresh._norm_bound) and (normalize or float(eb._norm_bound) > 1.9)
    gone = torch.zeros(n, dtype=torch.bool)
    if eb._as_filter(None) is None:  # full and without holes: both banks take the unmasked calls
        assert fresh._as_filter(None) is None
        _all_searches(eb, fresh, 4, device, labels, f"{name} replace", [({}, {})])
    else:
        _removed_equals_masked(eb, fresh, gone, 4, device, labels, f"{name} replace")
    # a second replacement names a removed row too: it stays removed, with the bytes it had
    assert eb.remove(rows=[255, 5]) == 2
    gone[[255, 5]] = True
    idx2 = [254, 255, 256, 6]
    new2 = _rows(4, d, in_dtype, 78, unit=not normalize)
    eb.replace(idx2, new2.to(device), normalize=normalize)
    vec.update({r: new2[j] for j, r in enumerate(idx2) if r != 255})
    fresh = _fresh_with(name, device, vec, normalize, eb.capacity)
    assert torch.equal(eb.bank.view(torch.uint8), fresh.bank.view(torch.uint8))
    assert float(eb._norm_bound) >= float(fresh._norm_bound)
    _removed_equals_masked(eb, fresh, gone, 5, device, labels, f"{name} replace with a tombstone")


def _origin(labels: torch.Tensor) -> torch.Tensor:
    n = labels.shape[0]
    return torch.stack([labels, torch.arange(n) // 4, torch.arange(n) % 4], dim=1)


def _compacted_equals_fresh(eb, rows, labels, origin, alive, step, device, what, normalize) -> None:
    """Rule 4.  `alive`: the original positions (in `rows` / `labels` / `origin`) of the rows `eb` should hold, in order."""
    fresh = _make(rows[alive], labels[alive], device, eb.dtype, normalize, eb.capacity)
    assert len(eb) == len(fresh) == alive.numel() and eb.num_removed == 0, what
    assert torch.equal(eb.bank.view(torch.uint8), fresh.bank.view(torch.uint8)), what
    assert torch.equal(eb.group_labels, fresh.group_labels) and eb._max_group_rows == fresh._max_group_rows, what
    assert torch.equal(eb.row_origin.cpu(), origin[alive]), what
    assert bool(eb.live.all())
    _all_searches(eb, fresh, step, device, labels, what, [({}, {})])
    excl = labels[alive][torch.randint(0, alive.numel(), (130,), generator=cases.gen(400 + step))]
    allow = (torch.rand(alive.numel(), generator=cases.gen(300 + step)) < 0.5).to(device)
    _all_searches(eb, fresh, step + 1, device, labels, what, [({"exclude_group": excl}, {"exclude_group": excl}),
                                                               ({"mask": allow}, {"mask": allow})])


@pytest.mark.parametrize("name", list(BANKS))
def test_compact_equals_the_bank_of_the_surviving_rows(name: str, device: torch.device) -> None:
    d, _, in_dtype, normalize, _, _, _ = BANKS[name]
    rows, labels = _data(name)
    origin = _origin(labels)
    eb = _build(name, device)
    eb.row_origin = origin.clone()
    n, capacity = len(eb), eb.capacity
    gone = torch.rand(n, generator=cases.gen(61)) < 0.4
    gone[250:258] = torch.tensor([True, False] * 4)[: min(n, 258) - 250]
    gone |= labels == int(labels[7])  # a whole group: its label leaves `group_labels`
    assert eb.remove(rows=torch.nonzero(gone).squeeze(1)) == int(gone.sum())
    old = (eb._bank.data_ptr(), eb._max_group_rows)
    index_map = eb.compact()
    alive = torch.nonzero(~gone).squeeze(1)
    assert index_map.dtype == torch.int64 and index_map.device == eb.device and index_map.shape == (n,)
    exp_map = torch.full((n,), -1, dtype=torch.int64)
    exp_map[alive] = torch.arange(alive.numel())
    assert torch.equal(index_map.cpu(), exp_map)
    assert eb.capacity == capacity and eb._bank.data_ptr() != old[0] and int(labels[7]) not in eb.group_labels.tolist()
    assert eb._max_group_rows <= old[1]
    _compacted_equals_fresh(eb, rows, labels, origin, alive, 2, device, f"{name} compact", normalize)
    assert torch.equal(eb.compact().cpu(), torch.arange(alive.numel()))  # no holes: the identity, nothing moves
    # an append after the compaction numbers from the new length and equals the fresh bank plus those rows
    m = 33
    more, more_labels = _rows(m, d, in_dtype, 62, unit=not normalize), _labels(m, 62) + 5
    got = eb.append(more.to(device), row_groups=more_labels, row_origin=_origin(more_labels))
    assert got == range(alive.numel(), alive.numel() + m)
    rows2, labels2 = torch.cat([rows, more]), torch.cat([labels, more_labels])
    origin2 = torch.cat([origin, _origin(more_labels)])
    alive2 = torch.cat([alive, torch.arange(n, n + m)])
    _compacted_equals_fresh(eb, rows2, labels2, origin2, alive2, 6, device, f"{name} compact + append", normalize)


def test_a_compacted_bank_filled_exactly_returns_to_the_unmasked_calls(device: torch.device) -> None:
    """255 rows in capacity 257: 3 removed and compacted leave 252; 5 more fill the capacity exactly with no hole left, so
    `_as_filter(None)` is None again and the bank equals the never-reserved bank of those 257 rows."""
    name = "255-257"
    d, dtype, in_dtype, normalize, _, _, _ = BANKS[name]
    rows, labels = _data(name)
    eb = _build(name, device)
    assert eb.remove(rows=[0, 128, 254]) == 3 and eb._as_filter(None) is not None
    eb.compact()
    more, more_labels = _rows(5, d, in_dtype, 63), _labels(5, 63)
    eb.append(more.to(device), row_groups=more_labels)
    assert len(eb) == eb.capacity == 257 and eb.num_removed == 0 and eb._as_filter(None) is None
    alive = torch.tensor([r for r in range(255) if r not in (0, 128, 254)])
    fresh = _make(torch.cat([rows[alive], more]), torch.cat([labels[alive], more_labels]), device, dtype, normalize)
    assert fresh._fill is None and torch.equal(eb.bank.view(torch.uint8), fresh.bank.view(torch.uint8))
    _all_searches(eb, fresh, 1, device, labels, "refilled", [({}, {})])
    assert eb.remove(rows=[256]) == 1 and eb._as_filter(None) is eb._fill_filter  # full, holed: masked again


def test_interleaved_append_remove_replace_growth_compact(device: torch.device) -> None:
    """One bank through append, remove, replace, an append past the capacity (a growth with holes in the image), remove
    and compact; after every step it equals the twin built from the same rows at once in the same capacity with the
    removed rows masked (rule 1), and at the end the bank built from the survivors (rule 4)."""
    name = "300-513"
    d, dtype, in_dtype, normalize, _, _, _ = BANKS[name]
    rows, labels = _data(name)
    eb = _build(name, device)
    eb.row_origin = _origin(labels)
    gone = torch.zeros(300, dtype=torch.bool)
    zeroed = torch.zeros(0, dtype=torch.bool)  # the rows that were removed when the image last moved

    def check(step: int) -> None:
        twin = _make(rows, labels, device, dtype, normalize, eb.capacity)
        # (a removed row keeps its bytes while the image stays; a growth moves the live rows only and leaves zeros)
        stored, expected = eb.bank.view(torch.uint8).cpu(), twin.bank.view(torch.uint8).cpu()
        kept = ~zeroed[: gone.numel()] if zeroed.numel() else torch.ones_like(gone)
        kept = torch.cat([kept, torch.ones(gone.numel() - kept.numel(), dtype=torch.bool)])
        assert torch.equal(stored[kept], expected[kept]) and not bool(stored[~kept].any())
        _removed_equals_masked(eb, twin, gone, step, device, labels, f"interleaved step {step}")

    def grow(m: int, seed: int) -> None:
        nonlocal rows, labels, gone
        more, more_labels = _rows(m, d, in_dtype, seed, unit=not normalize), _labels(m, seed)
        first = len(eb)
        assert eb.append(more.to(device), row_groups=more_labels, row_origin=_origin(more_labels)) == range(first, first + m)
        rows, labels = torch.cat([rows, more]), torch.cat([labels, more_labels])
        gone = torch.cat([gone, torch.zeros(m, dtype=torch.bool)])

    grow(31, 81)  # in place
    assert eb.capacity == 513
    assert eb.remove(rows=list(range(240, 270)) + [5, 330]) == 32
    gone[240:270] = True
    gone[[5, 330]] = True
    check(0)
    idx = torch.tensor([239, 270, 300, 6])
    new = _rows(4, d, in_dtype, 82, unit=not normalize)
    eb.replace(idx, new.to(device))
    rows[idx] = new
    check(1)
    image = eb._bank.data_ptr()
    grow(200, 83)  # 331 + 200 > 513: the image moves, the holes stay holes
    zeroed = gone.clone()
    zeroed[331:] = False
    assert eb.capacity == 1026 and eb._bank.data_ptr() != image and eb.num_removed == 32 and len(eb) == 531
    check(2)
    assert eb.remove(groups=[int(labels[400])]) > 0
    gone |= labels == int(labels[400])
    check(3)
    origin = eb.row_origin.clone()
    index_map = eb.compact()
    alive = torch.nonzero(~gone).squeeze(1)
    assert torch.equal(index_map.cpu()[alive], torch.arange(alive.numel())) and bool((index_map.cpu()[gone] == -1).all())
    _compacted_equals_fresh(eb, rows, labels, origin, alive, 4, device, "interleaved compact", normalize)


def test_captured_search_replays_over_a_removal_and_a_replacement(device: torch.device) -> None:
    """A `search` captured on a bank with spare capacity is the masked call and holds the image, the fill bitmap and the
    norm bound by pointer: `remove` and `replace` update them in place, so the next replay answers for the changed bank."""
    name = "255-257"
    d, dtype, in_dtype, normalize, _, _, _ = BANKS[name]
    rows, _ = _data(name)
    eb, twin = _build(name, device, grouped=False), _build(name, device, grouped=False)
    q = _queries(65, d, dtype, 24, device)
    out = {}

    def run():
        out["r"] = eb.search(q, 10)

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    torch.cuda.synchronize()
    q.copy_(_queries(65, d, dtype, 25, device))
    best = twin.search(q, 10)[1][:, 0].unique()  # the rows the queries like best
    assert eb.remove(rows=best) == best.numel()
    graph.replay()
    torch.cuda.synchronize()
    _same(out["r"], eb.search(q, 10))
    _same(out["r"], twin.search(q, 10, mask=twin.row_filter(rows=best, exclude=True)))
    assert not bool(torch.isin(out["r"][1], best).any())
    idx = torch.tensor([r for r in (7, 200, 254, 8, 201, 253) if r not in best.tolist()][:3])  # three live rows
    new = (q[:3].float() * 0.5).to(in_dtype)  # each becomes its query's best row, and raises the norm bound the graph reads
    eb.replace(idx, new)
    rows2 = rows.clone()
    rows2[idx] = new.cpu()
    twin2 = _make(rows2, None, device, dtype, normalize, 257)
    graph.replay()
    torch.cuda.synchronize()
    _same(out["r"], eb.search(q, 10))
    _same(out["r"], twin2.search(q, 10, mask=twin2.row_filter(rows=best, exclude=True)))
    assert out["r"][1][:3, 0].tolist() == idx.tolist() and float(eb._norm_bound) > 2.0


def test_unresolved_async_searches_see_the_bank_before_the_removal(device: torch.device) -> None:
    name = "300-513"
    eb, twin = _build(name, device, grouped=False), _twin(name, device)
    q = [_queries(65, eb.dim, eb.dtype, 18 + i, device) for i in range(3)]
    gone = torch.arange(0, 300, 2)
    torch.cuda.synchronize()
    h0 = eb.search_async(q[0], 10)
    h1 = eb.search_async(q[1], 120)
    assert eb.remove(rows=gone.to(device)) == 150
    h2 = eb.search_async(q[2], 10)
    _same(h2.result(), twin.search(q[2], 10, mask=twin.row_filter(rows=gone, exclude=True)))
    _same(h0.result(), twin.search(q[0], 10))
    _same(h1.result(), twin.search(q[1], 120))
    assert not bool((h2.result()[1] % 2 == 0).any()) and bool((h0.result()[1] % 2 == 0).any())
