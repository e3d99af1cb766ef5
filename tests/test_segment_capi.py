"""The C entry points of csrc/label_map.hip without a device: they are declared, exported and bound, the ABI version has
not moved, the geometry call answers, and every limit the header states is refused with its error code before anything
is launched (the pointers below are never dereferenced: the checks come first, and B = 0 launches nothing)."""

from __future__ import annotations

import math
import re
from pathlib import Path

from imagescry_amd import _lib, segmentation

HEADER = Path(__file__).resolve().parents[1] / "include" / "imagescry_hip.h"
NAMES = ("isc_label_map", "isc_label_map_geometry", "isc_map_class_scores")
OK, INVALID, UNSUPPORTED, ALIGNMENT = _lib.ISC_OK, _lib.ISC_ERR_INVALID_ARG, _lib.ISC_ERR_UNSUPPORTED, _lib.ISC_ERR_ALIGNMENT
P = 4096  # a 16-byte aligned non-NULL address no call reaches


def test_declared_bound_and_abi_unchanged() -> None:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        proto = re.search(rf"\bint {name}\s*\(([^;]*?)\);", text, flags=re.S)
        assert proto is not None, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name)
    assert lib.isc_abi_version() == _lib.ISC_ABI_VERSION == 4
    assert "#define ISC_ABI_VERSION 4" in HEADER.read_text()


def test_geometry() -> None:
    tw, th, chunk = segmentation.label_map_geometry()
    assert tw * th == 256 and tw % 4 == 0  # a thread a pixel; label quads do not straddle tiles
    assert 4 <= chunk <= segmentation.MAX_PROMPTS and chunk % 4 == 0
    assert _lib.load().isc_label_map_geometry(None, None, None) == INVALID


def _label_map(scores=P, b=1, h=2, w=2, c=3, ldc=3, class_of=None, big_h=4, big_w=4, min_score=-math.inf, labels=P,
               best=P, margin=None, counts=None) -> int:
    return _lib.load().isc_label_map(scores, b, h, w, c, ldc, class_of, big_h, big_w, min_score, labels, best, margin,
                                     counts, None)


def test_label_map_argument_checks() -> None:
    assert _label_map(b=0) == OK  # an empty batch: no launch
    assert _label_map(b=0, scores=None, labels=None, best=None) == OK
    assert _label_map(b=-1) == INVALID
    for kw in (dict(h=0), dict(w=0), dict(big_h=0), dict(big_w=0), dict(c=0), dict(ldc=2), dict(scores=None),
               dict(labels=None, best=None), dict(min_score=math.nan)):
        assert _label_map(**kw) == INVALID, kw
    for kw in (dict(c=1025, ldc=1025), dict(h=65536, w=32768), dict(big_h=65536, big_w=32768), dict(b=65536),
               dict(big_h=4 * 65535 + 1)):
        assert _label_map(**kw) == UNSUPPORTED, kw
    for kw in (dict(scores=P + 4), dict(best=P + 2), dict(margin=P + 1), dict(counts=P + 2), dict(class_of=P + 2)):
        assert _label_map(**kw) == ALIGNMENT, kw
    # the limits themselves are accepted (with no image in the batch nothing is launched)
    assert _label_map(b=0, c=1024, ldc=1024, big_h=4 * 65535, big_w=8192, h=46340, w=46340) == OK


def _class_scores(maps=P, b=1, e=4, s=9, vectors=P, c=3, ldv=4, out=P, ldc=3) -> int:
    return _lib.load().isc_map_class_scores(maps, b, e, s, vectors, c, ldv, out, ldc, None)


def test_map_class_scores_argument_checks() -> None:
    assert _class_scores(b=0) == OK
    assert _class_scores(b=0, maps=None, vectors=None, out=None) == OK
    for kw in (dict(b=-1), dict(e=0), dict(s=0), dict(c=0), dict(ldv=3), dict(ldc=2), dict(maps=None),
               dict(vectors=None), dict(out=None)):
        assert _class_scores(**kw) == INVALID, kw
    assert _class_scores(b=65536) == UNSUPPORTED
    for kw in (dict(maps=P + 2), dict(vectors=P + 1), dict(out=P + 3)):
        assert _class_scores(**kw) == ALIGNMENT, kw
