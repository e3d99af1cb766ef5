"""Which kernel a convolution shape is MEANT to reach: a pure-Python restatement of `conv_launch` (encoder.hip) and of
`isc_conv_halo_applies` (conv_halo.hip), so that a test can say "this case walks 64 x 256 packed-K tiles" and have the
claim checked on the CPU (tests/test_conv_paths_host.py) and, through the launch count, on the GPU.  A helper, not a
conftest.

`conv_path` returns a `ConvPath`:

    kernels   one name per launch: `halo<MI>` or `conv<TCO,TPIX,TAP4,DMA,DUAL>`
    form      `single`         one launch of full tiles (or of the halo kernel)
              `all-halves`     plain layers of at most 8 K steps: every tile as two half tiles, one launch
              `halves-only`    no whole round of full tiles: the layer as half tiles, one launch
              `rounds+halves`  whole rounds of full tiles, then the remainder as half tiles (`tile_base > 0`)
    launches  len(kernels)
    tiles     tiles of each launch (half tiles where the launch computes halves)
    grid      workgroups of each launch
    walk      the largest number of tiles one workgroup of any launch walks
    ksteps    128-byte K steps of a tile

`cases_for(cus)` is the table of GPU cases of tests/test_gpu_conv_dma.py.  Pixel counts are computed from the number of
resident workgroups (2 * cus), so the table lands on the same paths on a part with another CU count; the host test
checks that at two counts.  `edges` names the tile-edge properties of a case (ragged last pixel tile, empty last half
tile, Cout past a channel tile by 4, an image seam inside a tile)."""

from __future__ import annotations

import math
from dataclasses import dataclass

HALO_LDS_LIMIT = 78 * 1024
HALVES_KSTEPS = 8  # plain layers of at most this many K steps run as half tiles throughout
SPLIT_KSTEPS = 16  # whole rounds + half-tile remainder only for tiles at least this long
MAC_CAP = 7e9  # multiply-adds of a case's float64 reference


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def out_size(h: int, w: int, r: int, s: int, stride: int, pad: int) -> tuple[int, int]:
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def halo_lds_bytes(cin: int, cout: int, r: int, stride: int) -> int:
    """LDS image of the halo-tile kernel: folded weights + one input halo tile (rounded to whole staging rounds)."""
    cin4 = cin // 4
    kq = _ceil_div(r * r * cin4, 4)
    mi = 2 if cout <= 32 else 4
    hr = 15 * stride + r
    return kq * mi * 16 * 4 * 16 + _ceil_div(hr * hr * cin4, 256) * 256 * 16


def halo_applies(cin: int, cout: int, r: int, s: int, stride: int, pad: int) -> bool:
    if r != s or r not in (3, 5, 7) or pad != r // 2 or stride not in (1, 2):
        return False
    if cin % 4 or cin % 32 == 0 or cin > 24 or cout > 64 or cout % 4:
        return False
    return halo_lds_bytes(cin, cout, r, stride) <= HALO_LDS_LIMIT


@dataclass(frozen=True)
class ConvPath:
    kernels: tuple[str, ...]
    form: str
    tiles: tuple[int, ...]
    grid: tuple[int, ...]
    ksteps: int
    tco: int  # channel tile of the layer's FULL tiles (halo: 16 * MI)
    tpix: int  # pixels of a FULL tile (halo: 256 = 16 x 16)

    @property
    def launches(self) -> int:
        return len(self.kernels)

    @property
    def walk(self) -> int:
        return max(_ceil_div(t, g) for t, g in zip(self.tiles, self.grid))

    @property
    def tile_base(self) -> int:
        return self.tiles[0] if self.form == "rounds+halves" else 0


def _name(tco: int, tpix: int, tap4: bool, dma: bool, dual: bool = False) -> str:
    return f"conv<{tco},{tpix},{str(tap4).lower()},{str(dma).lower()},{str(dual).lower()}>"


def conv_path(b: int, h: int, w: int, cin: int, cout: int, r: int, s: int, stride: int, pad: int, cus: int, cin2: int = 0,
              transformed: bool = False) -> ConvPath:
    """The launches `conv_launch` makes for this layer on a part of `cus` compute units.  `cin2`: channels of the
    K-concatenated second input (`isc_conv2d_nhwc_dual`); `transformed`: a gate or a centring vector is applied to x
    (`isc_conv2d_nhwc_gated`, `isc_linear_centered`), which selects the register-staged form."""
    if cin % 4 or cout % 4:
        raise ValueError("channels are multiples of 4")
    tap4 = cin % 32 != 0
    if transformed and tap4:
        raise ValueError("no packed-K form with a transformed operand")
    if cin2 and (tap4 or transformed or cin2 % 32 or (r, s, stride, pad) != (1, 1, 1, 0)):
        raise ValueError("the second input exists for plain 1 x 1 / 1 / 0 layers only")
    ho, wo = out_size(h, w, r, s, stride, pad)
    m = b * ho * wo
    ksteps = _ceil_div(r * s * cin, 32) if tap4 else r * s * (cin // 32)
    ksteps += cin2 // 32
    resident = 2 * cus
    if tap4 and not cin2 and halo_applies(cin, cout, r, s, stride, pad):
        mi = 2 if cout <= 32 else 4
        tiles = b * _ceil_div(ho, 16) * _ceil_div(wo, 16)
        return ConvPath((f"halo<{mi}>",), "single", (tiles,), (min(tiles, resident),), ksteps, 16 * mi, 256)
    narrow = _ceil_div(cout, 64) * 64 < _ceil_div(cout, 128) * 128
    dma = not transformed
    tile32 = cout <= 32 and dma
    if tile32:
        tco, tpix = 32, 256
    elif narrow:
        tco, tpix = 64, 256
    else:
        tco, tpix = 128, 128
    blocks = _ceil_div(m, 256) if tile32 else _ceil_div(cout, tco) * _ceil_div(m, tpix)
    grid = min(blocks, resident) if dma else blocks
    if cin2:
        return ConvPath((_name(tco, tpix, False, True, True),), "single", (blocks,), (grid,), ksteps, tco, tpix)
    half = _name(tco, tpix // 2, tap4, True)
    if dma and not tile32 and not tap4 and ksteps <= HALVES_KSTEPS:
        return ConvPath((half,), "all-halves", (2 * blocks,), (min(2 * blocks, 3 * cus),), ksteps, tco, tpix)
    if dma and not tile32:
        rounds, rem = divmod(blocks, resident)
        if rem > 0 and rem * 4 <= resident * 3 and (ksteps >= SPLIT_KSTEPS or rounds == 0):
            g2 = min(2 * rem, 3 * resident // 2)
            if rounds == 0:
                return ConvPath((half,), "halves-only", (2 * rem,), (g2,), ksteps, tco, tpix)
            return ConvPath((_name(tco, tpix, tap4, True), half), "rounds+halves", (rounds * resident, 2 * rem),
                            (resident, g2), ksteps, tco, tpix)
    return ConvPath((_name(tco, tpix, tap4, dma),), "single", (blocks,), (grid,), ksteps, tco, tpix)


# --------------------------------------------------------------------------------------------------- the GPU case table
@dataclass(frozen=True)
class Case:
    name: str
    shape: tuple[int, ...]  # (B, H, W, Cin, Cout, R, S, stride, pad)
    cin2: int = 0  # the dual entry: channels of the second input ...
    stride2: int = 1  # ... and the stride it is sampled at

    def path(self, cus: int) -> ConvPath:
        return conv_path(*self.shape, cus, cin2=self.cin2)

    @property
    def macs(self) -> int:
        b, h, w, cin, cout, r, s, stride, pad = self.shape
        ho, wo = out_size(h, w, r, s, stride, pad)
        return b * ho * wo * (r * s * cin + self.cin2) * cout


def edges(case: Case, cus: int) -> set[str]:
    """Tile-edge properties of a case of the k_conv_f32 family (not the halo kernel)."""
    b, h, w, cin, cout, r, s, stride, pad = case.shape
    p = case.path(cus)
    found: set[str] = set()
    if p.kernels[0].startswith("halo"):
        return found
    ho, wo = out_size(h, w, r, s, stride, pad)
    m = b * ho * wo
    last = m % p.tpix
    if last:
        found.add("ragged-pixel-tile")
    if p.form != "single" and 0 < last <= p.tpix // 2:
        found.add("empty-last-half")  # the last full tile is in the half-tile launch: its second half has no pixel
    if cout % p.tco == 4:
        found.add("cout-past-tile-by-4")
    if any((i * ho * wo) % p.tpix for i in range(1, b)):
        found.add("image-seam-in-tile")
    return found


def _hw(npix: int, width: int) -> tuple[int, int]:
    """An image of `width` columns with at least `npix` pixels (fewer than `width` more)."""
    return _ceil_div(npix, width), width


def _pixels(tiles: int, co_tiles: int, tpix: int, ragged: int) -> int:
    """Pixels that give at least `tiles` tiles over `co_tiles` channel tiles, the last pixel tile holding `ragged`."""
    return (_ceil_div(tiles, co_tiles) - 1) * tpix + ragged


def cases_for(cus: int) -> tuple[Case, ...]:
    res = 2 * cus  # resident workgroups of the persistent kernels
    over = 2 * res + 8  # every workgroup walks two tiles, some three
    most = 3 * res // 4 + 4  # more than three quarters of a round: one launch, one tile per workgroup
    thin = res + res // 10  # a thin second round: whole round + half-tile remainder for long tiles
    c = []

    def add(name, b, npix, width, cin, cout, r, s, stride, pad, **kw):
        h, w = _hw(npix, width) if npix else width
        c.append(Case(name, (b, h, w, cin, cout, r, s, stride, pad), **kw))

    # ---- 32 x 256 (Cout <= 32): never split
    add("t32-plain-single", 2, 0, (13, 12), 64, 24, 1, 1, 1, 0)  # two tiles, seam inside the first, ragged second
    add("t32-plain-walk", 1, _pixels(res + 3, 1, 256, 100), 509, 32, 24, 1, 1, 1, 0)  # ONE K step per tile
    add("t32-packed-single", 3, 0, (17, 17), 40, 32, 1, 1, 1, 0)
    add("t32-packed-walk", 1, _pixels(res + 3, 1, 256, 37), 363, 40, 24, 1, 1, 1, 0)  # two K steps
    # ---- 64 x 256 full tiles
    add("t64-plain-single", 1, _pixels(most, 3, 256, 60), 182, 288, 192, 1, 1, 1, 0)  # nine K steps
    add("t64-plain-walk", 1, _pixels(over, 3, 256, 200), 297, 32, 192, 3, 3, 1, 1)  # nine K steps (odd), padding taps
    add("t64-packed-single", 1, _pixels(most, 3, 256, 60), 181, 40, 192, 3, 3, 1, 1)  # twelve K steps
    add("t64-packed-walk", 1, _pixels(over, 3, 256, 200), 297, 24, 192, 3, 3, 1, 1)  # seven K steps (odd)
    # ---- 128 x 128 full tiles
    add("t128-plain-single", 1, _pixels(most, 4, 128, 60), 113, 288, 512, 1, 1, 1, 0)
    add("t128-plain-walk", 1, _pixels(over, 4, 128, 100), 182, 32, 512, 3, 3, 1, 1)  # nine K steps (odd)
    add("t128-packed-single", 1, _pixels(most, 4, 128, 60), 113, 40, 512, 3, 3, 1, 1)
    add("t128-packed-walk", 1, _pixels(over, 4, 128, 100), 182, 20, 512, 3, 3, 1, 1)  # six K steps (even)
    # ---- half tiles throughout (plain, at most 8 K steps)
    add("h64-all-single", 3, 0, (9, 11), 256, 132, 1, 1, 1, 0)  # eight K steps; 297 pixels: the last half empty; 64+64+4
    add("h64-all-walk", 2, _pixels(res + 7, 3, 256, 130) // 2, 211, 64, 192, 1, 1, 1, 0)  # two K steps
    add("h128-all-single", 2, 0, (14, 14), 64, 256, 1, 1, 1, 0)
    add("h128-all-walk", 1, _pixels(res + 6, 2, 128, 30), 211, 96, 256, 1, 1, 1, 0)  # three K steps; the last half empty
    add("h128-all-onestep", 1, _pixels(res + 6, 2, 128, 100), 199, 32, 256, 1, 1, 1, 0)  # ONE K step, walking
    # ---- no whole round: half tiles only
    add("h64-plain-only", 1, 0, (33, 35), 512, 192, 1, 1, 1, 0)  # 15 tiles as 30 halves, the last one empty
    add("h128-plain-only", 3, 0, (9, 9), 320, 256, 1, 1, 1, 0)  # 4 tiles as 8 halves, seams inside tiles
    add("h64-packed-only", 2, 0, (17, 19), 48, 192, 3, 3, 1, 1)
    add("h128-packed-only", 2, 0, (17, 19), 40, 128, 3, 3, 1, 1)
    # ---- whole round + half-tile remainder (>= 16 K steps)
    add("h64-plain-rounds", 1, _pixels(thin, 3, 256, 90), 170, 64, 192, 3, 3, 1, 1)  # 18 K steps
    add("h128-plain-rounds", 1, _pixels(thin, 4, 128, 50), 120, 64, 512, 3, 3, 1, 1)
    add("h64-packed-rounds", 1, _pixels(thin, 3, 256, 90), 170, 60, 192, 3, 3, 1, 1)  # 17 K steps (odd)
    add("h128-packed-rounds", 1, _pixels(thin, 4, 128, 50), 120, 56, 512, 3, 3, 1, 1)  # 16 K steps (even)
    # ---- the K-concatenated second input
    add("dual64-single-s1", 3, 0, (9, 9), 64, 192, 1, 1, 1, 0, cin2=64, stride2=1)
    add("dual64-walk-s2", 1, _pixels(res + 5, 3, 256, 77), 157, 32, 192, 1, 1, 1, 0, cin2=32, stride2=2)
    add("dual128-single-s2", 2, 0, (7, 9), 64, 256, 1, 1, 1, 0, cin2=96, stride2=2)
    add("dual128-walk-s1", 1, _pixels(res + 6, 4, 128, 51), 157, 32, 512, 1, 1, 1, 0, cin2=64, stride2=1)
    # ---- the halo-tile kernel
    per_image = _ceil_div(res + 6, 3)  # three images: a tile index crosses an image
    tx = math.isqrt(per_image) + 1
    ty = _ceil_div(per_image, tx)
    add("halo2-single", 1, 0, (5, 7), 24, 24, 3, 3, 1, 1)  # smaller than one 16 x 16 tile
    add("halo2-walk", 3, 0, (16 * ty - 5, 16 * tx - 3), 24, 24, 3, 3, 1, 1)  # ragged in both directions
    add("halo2-5x5", 2, 0, (33, 47), 16, 32, 5, 5, 1, 2)  # exactly at the LDS limit
    add("halo2-7x7-s2", 3, 0, (45, 31), 4, 16, 7, 7, 2, 3)  # stride 2 on odd sizes
    add("halo2-cout4-s2", 2, 0, (64, 64), 8, 4, 3, 3, 2, 1)  # stride 2 on even sizes; one of four channel groups
    add("halo4-single", 1, 0, (11, 9), 16, 36, 3, 3, 1, 1)  # 32 + 4 channels
    add("halo4-walk-s2", 3, 0, (32 * ty - 9, 32 * tx - 6), 8, 48, 3, 3, 2, 1)
    add("halo4-stem", 2, 0, (61, 50), 4, 64, 7, 7, 2, 3)  # the ResNet-50 stem's window
    add("halo4-5x5-s2", 1, 0, (40, 37), 4, 64, 5, 5, 2, 2)
    return tuple(c)


# what the table has to reach (tests/test_conv_paths_host.py): (kernel, form, walks)
def required_paths() -> list[tuple[str, str, bool]]:
    need = []
    for tco, tpix in ((32, 256), (64, 256), (128, 128)):
        for tap4 in (False, True):
            for walks in (False, True):
                need.append((_name(tco, tpix, tap4, True), "single", walks))
    for tco, tpix in ((64, 128), (128, 64)):
        need += [(_name(tco, tpix, False, True), "all-halves", False), (_name(tco, tpix, False, True), "all-halves", True)]
        for tap4 in (False, True):
            need += [(_name(tco, tpix, tap4, True), "halves-only", False), (_name(tco, tpix, tap4, True), "rounds+halves", False)]
    for tco, tpix in ((64, 256), (128, 128)):
        need += [(_name(tco, tpix, False, True, True), "single", False), (_name(tco, tpix, False, True, True), "single", True)]
    for mi in (2, 4):
        need += [(f"halo<{mi}>", "single", False), (f"halo<{mi}>", "single", True)]
    return need


def reached(case: Case, cus: int) -> list[tuple[str, str, bool]]:
    """The (kernel, form, walks) entries a case reaches, one per launch.  `walks` (a workgroup of the launch computes
    more than one tile) is told apart for the `single` and `all-halves` forms only, as the coverage list does."""
    p = case.path(cus)
    told_apart = p.form in ("single", "all-halves")
    return [(kernel, p.form, told_apart and t > g) for kernel, t, g in zip(p.kernels, p.tiles, p.grid)]
