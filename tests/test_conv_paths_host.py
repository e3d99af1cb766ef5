"""tests/conv_paths.py pinned to the worked examples of encoder.hip's comments and of the existing convolution tests, and
the GPU case table of tests/test_gpu_conv_dma.py checked for what it has to reach -- on the CPU, so that a deleted case
or a dispatch change that moves one fails here before a GPU is involved."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import conv_paths as cp  # noqa: E402

CU_COUNTS = (256, 304)  # the table is built from the count: the part under test and one other


def test_thin_last_round_of_128_tiles() -> None:
    """563 tiles of 128 x 128 on 512 resident workgroups: 512 + 51 -> 102 halves."""
    p = cp.conv_path(5, 120, 120, 64, 128, 3, 3, 1, 1, 256)
    assert p.form == "rounds+halves" and p.tiles == (512, 102) and p.grid == (512, 102) and p.ksteps == 18
    assert p.kernels == ("conv<128,128,false,true,false>", "conv<128,64,false,true,false>")
    assert p.launches == 2 and p.walk == 1 and p.tile_base == 512


def test_thin_last_round_of_64_tiles() -> None:
    """565 tiles of 64 x 256: 512 + 53 -> 106 halves of 64 x 128."""
    p = cp.conv_path(5, 170, 170, 64, 64, 3, 3, 1, 1, 256)
    assert p.form == "rounds+halves" and p.tiles == (512, 106)
    assert p.kernels == ("conv<64,256,false,true,false>", "conv<64,128,false,true,false>")


def test_no_whole_round() -> None:
    """15 tiles of 64 x 256 as 30 half tiles."""
    p = cp.conv_path(1, 33, 35, 512, 192, 1, 1, 1, 0, 256)
    assert p.form == "halves-only" and p.tiles == (30,) and p.grid == (30,) and p.launches == 1
    assert p.kernels == ("conv<64,128,false,true,false>",)


def test_resnet50_layer3_layer4_at_batch_512() -> None:
    """1 568 and 784 tiles on 512 resident workgroups (encoder.hip, conv_launch)."""
    l3 = cp.conv_path(512, 14, 14, 256, 256, 3, 3, 1, 1, 256)
    assert l3.form == "rounds+halves" and l3.tiles == (1536, 64) and sum((l3.tiles[0], l3.tiles[1] // 2)) == 1568
    assert l3.walk == 3 and l3.ksteps == 72
    l4 = cp.conv_path(512, 7, 7, 512, 512, 3, 3, 1, 1, 256)
    assert l4.form == "rounds+halves" and l4.tiles == (512, 544) and l4.grid == (512, 544)
    assert l4.tiles[0] + l4.tiles[1] // 2 == 784


def test_short_k_layers_run_as_half_tiles() -> None:
    p = cp.conv_path(8, 130, 130, 64, 256, 1, 1, 1, 0, 256)  # ResNet layer1 expand: two K steps per tile
    assert p.form == "all-halves" and p.kernels == ("conv<128,64,false,true,false>",) and p.grid == (768,)
    # "128 x 128 tiles, nine K steps" of test_conv2d_nhwc: 264 tiles are no whole round, so 528 half tiles
    p = cp.conv_path(6, 75, 75, 32, 128, 3, 3, 1, 1, 256)
    assert p.form == "halves-only" and p.kernels == ("conv<128,64,false,true,false>",) and p.tiles == (528,) and p.walk == 1


def test_register_staged_and_dual_forms() -> None:
    p = cp.conv_path(3, 9, 9, 96, 132, 1, 1, 1, 0, 256, transformed=True)  # tests/test_gpu_conv_staged.py
    assert p.kernels == ("conv<64,256,false,false,false>",) and p.grid == p.tiles == (3,)
    p = cp.conv_path(3, 9, 9, 96, 196, 1, 1, 1, 0, 256, transformed=True)
    assert p.kernels == ("conv<128,128,false,false,false>",) and p.tiles == (4,)
    p = cp.conv_path(8, 130, 130, 64, 256, 1, 1, 1, 0, 256, cin2=64)  # tests/test_gpu_encoder.py, dual input
    assert p.kernels == ("conv<128,128,false,true,true>",) and p.ksteps == 4 and p.walk == 5
    with pytest.raises(ValueError):
        cp.conv_path(1, 8, 8, 24, 32, 1, 1, 1, 0, 256, transformed=True)
    with pytest.raises(ValueError):
        cp.conv_path(1, 8, 8, 32, 32, 3, 3, 1, 1, 256, cin2=32)


def test_halo_rule() -> None:
    """The two packed-K cases of test_conv2d_packed_k_mode that moved to the halo-tile kernel, and the "halo" cases that
    fail its LDS rule (folded weights + halo tile <= 78 KiB) and run packed-K half tiles."""
    assert cp.halo_applies(24, 24, 3, 3, 1, 1) and cp.halo_applies(8, 48, 3, 3, 2, 1)
    assert cp.conv_path(8, 150, 150, 24, 24, 3, 3, 1, 1, 256).kernels == ("halo<2>",)
    assert cp.conv_path(8, 150, 150, 8, 48, 3, 3, 2, 1, 256).kernels == ("halo<4>",)
    assert cp.halo_lds_bytes(12, 40, 5, 1) == 98304 and not cp.halo_applies(12, 40, 5, 5, 1, 2)
    assert cp.halo_lds_bytes(20, 64, 7, 2) > 270000 and not cp.halo_applies(20, 64, 7, 7, 2, 3)
    p = cp.conv_path(3, 33, 47, 12, 40, 5, 5, 1, 2, 256)
    assert p.form == "halves-only" and p.kernels == ("conv<64,128,true,true,false>",)
    p = cp.conv_path(2, 45, 31, 20, 64, 7, 7, 2, 3, 256)
    assert p.form == "halves-only" and p.kernels == ("conv<64,128,true,true,false>",)
    assert cp.halo_lds_bytes(16, 4, 3, 2) == 92160  # (2, 64, 64, 16, 4, 3, 2, 1) of the same list: 32 x 256 packed-K
    assert cp.conv_path(2, 64, 64, 16, 4, 3, 3, 2, 1, 256).kernels == ("conv<32,256,true,true,false>",)
    # the stems the kernel was written for, and what the rule leaves out
    assert cp.halo_lds_bytes(4, 64, 7, 2) == 77824 and cp.halo_applies(4, 64, 7, 7, 2, 3)
    assert cp.halo_lds_bytes(16, 32, 5, 1) == cp.HALO_LDS_LIMIT and cp.halo_applies(16, 32, 5, 5, 1, 2)
    assert not cp.halo_applies(24, 24, 3, 3, 1, 0)  # not "same" padding
    assert not cp.halo_applies(24, 24, 1, 3, 1, 1) and not cp.halo_applies(24, 24, 3, 1, 1, 1)  # not square
    assert not cp.halo_applies(32, 24, 3, 3, 1, 1) and not cp.halo_applies(24, 68, 3, 3, 1, 1)
    assert not cp.halo_applies(24, 24, 3, 3, 3, 1)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_table_reaches_every_path(cus: int) -> None:
    got: dict[tuple[str, str, bool], list[str]] = {}
    for case in cp.cases_for(cus):
        for entry in cp.reached(case, cus):
            got.setdefault(entry, []).append(case.name)
    missing = [entry for entry in cp.required_paths() if entry not in got]
    assert not missing, f"no case of the table reaches {missing} at {cus} CUs"
    # stride2 1 and 2 on both dual instantiations
    duals = {(case.path(cus).kernels[0], case.stride2) for case in cp.cases_for(cus) if case.cin2}
    assert duals == {(k, s2) for k in ("conv<64,256,false,true,true>", "conv<128,128,false,true,true>") for s2 in (1, 2)}
    # tile_base > 0 in every rounds+halves case, and its whole rounds are one tile per workgroup
    for case in cp.cases_for(cus):
        p = case.path(cus)
        if p.form == "rounds+halves":
            assert p.tile_base == 2 * cus and p.grid[0] == p.tiles[0] and p.ksteps >= 16


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_table_names_what_it_runs(cus: int) -> None:
    """A case's name states its path: tile shape, plain / packed, and how the tiles are spread."""
    names = [case.name for case in cp.cases_for(cus)]
    assert len(set(names)) == len(names)
    for case in cp.cases_for(cus):
        p = case.path(cus)
        family, *rest = case.name.split("-")
        if family.startswith("halo"):
            assert p.kernels == (f"halo<{family[4]}>",), case
            assert cp.halo_applies(*case.shape[3:])
            assert (p.walk > 1) == ("walk" in rest), case
            continue
        tap4 = "true" if "packed" in rest else "false"
        if family.startswith("dual"):
            tco = int(family[4:])
            assert p.kernels == (f"conv<{tco},{256 if tco == 64 else 128},false,true,true>",), case
        elif family.startswith("t"):
            tco = int(family[1:])
            assert p.form == "single" and p.kernels == (f"conv<{tco},{128 if tco == 128 else 256},{tap4},true,false>",), case
        else:
            tco = int(family[1:])
            assert p.kernels[-1] == f"conv<{tco},{64 if tco == 128 else 128},{tap4},true,false>", case
            form = {"all": "all-halves", "only": "halves-only", "rounds": "rounds+halves"}["all" if rest[0] == "all" else rest[-1]]
            assert p.form == form, case
        if "single" in rest:
            assert p.walk == 1, case
        if "walk" in rest or "onestep" in rest:
            assert p.walk >= 2, case


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_table_edges(cus: int) -> None:
    table = cp.cases_for(cus)
    walking = [c.path(cus) for c in table if c.path(cus).walk > 1 and not c.path(cus).kernels[0].startswith("halo")]
    ksteps = {p.ksteps for p in walking}
    assert 1 in ksteps and any(k % 2 == 0 for k in ksteps) and any(k % 2 == 1 and k > 1 for k in ksteps)
    # ... among the packed-K walkers too: the cursor reset is followed by a K step of either buffer parity
    packed = {p.ksteps % 2 for p in walking if ",true,true," in p.kernels[0]}
    assert packed == {0, 1}
    found: set[str] = set()
    for c in table:
        found |= cp.edges(c, cus)
    assert found >= {"ragged-pixel-tile", "empty-last-half", "cout-past-tile-by-4", "image-seam-in-tile"}
    # the halo kernel: an image smaller than a tile, ragged tiles both ways, three images, every window and stride
    halo = [c for c in table if c.name.startswith("halo")]
    assert any(c.shape[1] < 16 and c.shape[2] < 16 for c in halo)
    assert any(c.shape[0] == 3 and c.path(cus).walk > 1 for c in halo)
    assert {c.shape[5] for c in halo} == {3, 5, 7} and {c.shape[7] for c in halo} == {1, 2}
    assert {c.shape[3] for c in halo} >= {4, 8, 16, 24} and {c.shape[4] for c in halo} >= {4, 16, 32, 36, 64}
    for c in halo:
        ho, wo = cp.out_size(c.shape[1], c.shape[2], *c.shape[5:])
        if c.path(cus).walk > 1:
            assert ho % 16 and wo % 16, c


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_table_cost(cus: int) -> None:
    for case in cp.cases_for(cus):
        assert case.macs <= cp.MAC_CAP, f"{case.name}: {case.macs:.3g} multiply-adds for the float64 reference"
