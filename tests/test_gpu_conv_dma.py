"""The convolutions every ResNet-50 and EfficientNetV2 layer runs -- the LDS-DMA instantiations of `k_conv_f32` (full
tiles, half tiles, packed-K, the K-concatenated second input) and `k_conv_halo_f32` -- at the C ABI (`isc_conv2d_nhwc`,
`isc_conv2d_nhwc_dual`), against the two references of tests/matmul_bound.py: exact integers (`torch.equal` with the
float64 product) and the derived element-wise bound, activations by the rule of tests/conv_reference.py.  No tolerance
here is measured.

Which kernel a case runs is stated by its name and by tests/conv_paths.py, whose table (`cases_for`) is built from the
CU count of the device under test; tests/test_conv_paths_host.py checks on the CPU that the table reaches every
instantiation, single and walking, and `test_launch_count` checks on the GPU that the library made as many launches
as the restated dispatch says.  Every output is a `GuardedOutput`: canaries on both sides, NaN inside.

Exact integers.  x in -2 .. 2, w in -1 .. 1, bias and residual in -8 .. 8: every partial sum is an integer far below
2^24 (`assert_exact_range`), so any summation order gives the same bits -- tile splits, the K concatenation of the dual
entry and the chunk order of packed-K cannot excuse a difference."""

from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import conv_paths as cp  # noqa: E402
import matmul_bound as mb  # noqa: E402
from conv_reference import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, RES_AFTER, GuardedOutput, expected,  # noqa: E402
                            gemm_operands, packed_k_rows)

pytestmark = pytest.mark.gpu

CASE_NAMES = tuple(case.name for case in cp.cases_for(256))  # the names do not depend on the CU count, the shapes do
# real-valued operands: the small cases of every instantiation family, all activation / residual combinations ...
BOUND_SMALL = ("t32-plain-single", "t32-packed-single", "h64-all-single", "h128-all-single", "h64-plain-only",
               "h128-plain-only", "h64-packed-only", "h128-packed-only", "dual64-single-s1", "dual128-single-s2",
               "halo2-single", "halo2-5x5", "halo2-7x7-s2", "halo4-single", "halo4-stem")
# ... and the full tiles, which no small layer reaches, with four of them
BOUND_FULL = ("t64-plain-single", "t64-packed-single", "t128-plain-single", "t128-packed-single")
# (activation, residual: None / "inside" / "after")
COMBOS = tuple((act, where) for act in (ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_SIGMOID) for where in (None, "inside")) + tuple(
    (act, "after") for act in (ACT_GELU, ACT_SILU, ACT_SIGMOID))
COMBOS_FULL = ((ACT_NONE, "inside"), (ACT_SILU, None), (ACT_GELU, "inside"), (ACT_SIGMOID, "after"))
# (R, S, stride, pad): pad 1 under a one-row (one-column) filter gives output rows (columns) made of padding taps only
NONSQUARE = ((1, 3, 1, 1), (3, 1, 1, 1), (1, 7, 1, 1), (5, 3, 1, 1), (1, 3, 2, 1), (5, 3, 2, 2))
NONSQUARE_CHANNELS = ((32, 96), (64, 24), (24, 96), (24, 24))  # plain and packed-K, 128- and 32-channel tiles (never the halo kernel)


def device_cus(device: torch.device) -> int:
    return torch.cuda.get_device_properties(device).multi_processor_count


def table_case(name: str, device: torch.device) -> cp.Case:
    return {case.name: case for case in cp.cases_for(device_cus(device))}[name]


def _seed(case: cp.Case) -> int:
    return sum(case.shape) * 31 + sum(map(ord, case.name))


def operands(case: cp.Case, integers: bool) -> dict:
    """Host operands of a case, the weight rows as the C ABI takes them (`wdev`) and the GEMM operands `a`, `w2`."""
    b, h, w, cin, cout, r, s, stride, pad = case.shape
    g = torch.Generator().manual_seed(_seed(case))
    ho, wo = cp.out_size(h, w, r, s, stride, pad)
    k = r * s * cin + case.cin2
    if integers:
        x = mb.int_tensor((b, h, w, cin), -2, 2, g)
        wt = mb.int_tensor((cout, r, s, cin), -1, 1, g)
        bias = mb.int_tensor((cout,), -8, 8, g)
        res = mb.int_tensor((b * ho * wo, cout), -8, 8, g)
    else:
        x = torch.randn(b, h, w, cin, generator=g)
        wt = torch.randn(cout, r, s, cin, generator=g) / k**0.5
        bias = torch.randn(cout, generator=g)
        res = torch.randn(b * ho * wo, cout, generator=g)
    wdev = packed_k_rows(wt) if cin % 32 else wt
    a, w2 = gemm_operands(x, wdev, r, s, stride, pad)
    ops = dict(x=x, bias=bias, res=res, m=b * ho * wo)
    if case.cin2:
        s2 = case.stride2
        h2, w2_ = (h - 1) * s2 + 1 + (s2 > 1), (w - 1) * s2 + 1  # (h2 - 1) // s2 + 1 == h either way
        x2 = mb.int_tensor((b, h2, w2_, case.cin2), -2, 2, g) if integers else torch.randn(b, h2, w2_, case.cin2, generator=g)
        wd = mb.int_tensor((cout, case.cin2), -1, 1, g) if integers else torch.randn(cout, case.cin2, generator=g) / k**0.5
        a = torch.cat([a, x2[:, ::s2, ::s2, :].reshape(-1, case.cin2)], dim=1)  # [t | x2 sampled at stride2]
        w2 = torch.cat([w2, wd], dim=1)  # [w3 | wd]
        wdev = w2
        ops.update(x2=x2)
    ops.update(wdev=wdev.contiguous(), a=a, w2=w2)
    return ops


class Layer:
    """The operands of a case on the device, and the call."""

    def __init__(self, device: torch.device, case: cp.Case, ops: dict) -> None:
        self.device, self.case, self.m = device, case, ops["m"]
        self.x, self.w = ops["x"].contiguous().to(device), ops["wdev"].to(device)
        self.x2 = ops["x2"].contiguous().to(device) if case.cin2 else None
        self.bias, self.res = ops["bias"].to(device), ops["res"].contiguous().to(device)

    def run(self, act: int, bias: bool, res: bool, what: str) -> torch.Tensor:
        from imagescry_amd import _lib

        lib = _lib.load()
        b, h, w, cin, cout, r, s, stride, pad = self.case.shape
        out = GuardedOutput((self.m, cout), self.device)
        pb = self.bias.data_ptr() if bias else None
        pr = self.res.data_ptr() if res else None
        stream = _lib.stream_handle(self.device)
        if self.case.cin2:
            st = lib.isc_conv2d_nhwc_dual(self.x.data_ptr(), b, h, w, cin, self.x2.data_ptr(), self.x2.shape[1], self.x2.shape[2],
                                          self.case.cin2, self.case.stride2, self.w.data_ptr(), cout, pb, pr, act, out.ptr, stream)
        else:
            st = lib.isc_conv2d_nhwc(self.x.data_ptr(), b, h, w, cin, self.w.data_ptr(), cout, r, s, stride, pad, pb, pr, act,
                                     out.ptr, stream)
        _lib.check(st, what)
        return out.result(what)


def assert_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert torch.equal(got.double(), want), (what, mb.worst_ratio(got, want, torch.full_like(want, 2.0**-24)))


def check_exact(device: torch.device, case: cp.Case) -> None:
    """plain; bias + ReLU; bias + residual + ReLU; ReLU then residual -- each equal to the float64 result bit for bit."""
    ops = operands(case, integers=True)
    a, w2, bias, res = ops["a"], ops["w2"], ops["bias"], ops["res"]
    mb.assert_exact_range(a, w2, bias, res)
    pre = mb.product_f64(a, w2)
    b64, r64 = bias.double(), res.double()
    layer = Layer(device, case, ops)
    what = f"{case.name} {case.shape}"
    assert_equal(layer.run(ACT_NONE, False, False, what), pre, f"{what} plain")
    assert_equal(layer.run(ACT_RELU, True, False, what), (pre + b64).clamp_min(0.0), f"{what} bias + ReLU")
    assert_equal(layer.run(ACT_RELU, True, True, what), (pre + b64 + r64).clamp_min(0.0), f"{what} bias + residual + ReLU")
    assert_equal(layer.run(ACT_RELU | RES_AFTER, True, True, what), (pre + b64).clamp_min(0.0) + r64, f"{what} ReLU then residual")


def check_bound(device: torch.device, case: cp.Case, combos) -> float:
    """Real operands: every (activation, residual) combination within `expected()` of the float64 result."""
    ops = operands(case, integers=False)
    a, w2, bias, res = ops["a"], ops["w2"], ops["bias"], ops["res"]
    layer = Layer(device, case, ops)
    pre = {False: mb.product_f64(a, w2, bias), True: mb.product_f64(a, w2, bias, res)}
    # mb.product_bound with and without the residual, from one product: (K + 2) 2^-23 (|a| . |w|^T + |bias| [+ |residual|])
    pre_bound = {False: mb.product_bound(a, w2, bias)}
    pre_bound[True] = pre_bound[False] + (a.shape[1] + 2) * mb.U2 * res.double().abs()
    worst = 0.0
    for act, where in combos:
        what = f"{case.name} {case.shape} act {act} residual {where}"
        inside = where == "inside"
        want, bound = expected(pre[inside], pre_bound[inside], act, res.double() if where == "after" else None)
        got = layer.run(act | (RES_AFTER if where == "after" else 0), True, where is not None, what)
        ratio = mb.assert_within_bound(got, want, bound, what)
        print(f"{what}: error / bound = {ratio:.4f}")
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", CASE_NAMES)
def test_exact_integers(name: str, device: torch.device) -> None:
    case = table_case(name, device)
    if name.startswith("halo"):
        assert cp.halo_applies(*case.shape[3:])
    check_exact(device, case)


@pytest.mark.parametrize("name", BOUND_SMALL)
def test_within_bound(name: str, device: torch.device) -> None:
    case = table_case(name, device)
    if name.startswith("halo"):
        assert cp.halo_applies(*case.shape[3:])
    check_bound(device, case, COMBOS)


@pytest.mark.parametrize("name", BOUND_FULL)
def test_within_bound_full_tiles(name: str, device: torch.device) -> None:
    check_bound(device, table_case(name, device), COMBOS_FULL)


# ------------------------------------------------------------------------------------------------- non-square filters
def nonsquare_case(cin: int, cout: int, r: int, s: int, stride: int, pad: int) -> cp.Case:
    return cp.Case(f"{r}x{s}-{cin}-{cout}", (2, 9, 11, cin, cout, r, s, stride, pad))


@pytest.mark.parametrize("cin,cout", NONSQUARE_CHANNELS)
@pytest.mark.parametrize("r,s,stride,pad", NONSQUARE)
def test_nonsquare_exact_integers(r, s, stride, pad, cin, cout, device: torch.device) -> None:
    case = nonsquare_case(cin, cout, r, s, stride, pad)
    assert not cp.halo_applies(cin, cout, r, s, stride, pad)
    check_exact(device, case)
    # output rows (columns) whose every tap is padding: the bias through the activation, nothing else
    ops = operands(case, integers=True)
    ho, wo = cp.out_size(9, 11, r, s, stride, pad)
    rows = [oy for oy in range(ho) if not any(0 <= oy * stride - pad + dr < 9 for dr in range(r))]
    cols = [ox for ox in range(wo) if not any(0 <= ox * stride - pad + ds < 11 for ds in range(s))]
    assert (r, pad) != (1, 1) or rows == [0, ho - 1]
    assert (s, pad) != (1, 1) or cols == [0, wo - 1]
    if rows or cols:
        got = Layer(device, case, ops).run(ACT_RELU, True, False, f"{case.name} padding rows").reshape(2, ho, wo, cout)
        want = ops["bias"].clamp_min(0.0)
        for oy in rows:
            assert torch.equal(got[:, oy], want.expand(2, wo, cout)), f"{case.name}: output row {oy} is not relu(bias)"
        for ox in cols:
            assert torch.equal(got[:, :, ox], want.expand(2, ho, cout)), f"{case.name}: output column {ox} is not relu(bias)"


@pytest.mark.parametrize("cin,cout", NONSQUARE_CHANNELS)
@pytest.mark.parametrize("r,s,stride,pad", NONSQUARE[:4])
def test_nonsquare_within_bound(r, s, stride, pad, cin, cout, device: torch.device) -> None:
    check_bound(device, nonsquare_case(cin, cout, r, s, stride, pad), ((ACT_SILU, "after"), (ACT_GELU, "inside")))


# ------------------------------------------------------------------------------------------------------- launch count
@pytest.mark.parametrize("name", ("h64-plain-rounds", "h128-plain-rounds", "h64-packed-rounds", "h128-packed-rounds",
                                  "t64-packed-walk", "h64-plain-only", "halo2-walk"))
def test_launch_count(name: str, device: torch.device) -> None:
    """The library makes the launches tests/conv_paths.py says it makes: two for whole rounds + half-tile remainder, one
    otherwise.  Operands are zeros (the count does not depend on them); the output must be the bias."""
    import ctypes

    from imagescry_amd import _lib

    lib = _lib.load()
    cus = device_cus(device)
    ncus = ctypes.c_int()
    _lib.check(lib.isc_device_info(ncus, None, None, 0), "isc_device_info")
    assert ncus.value == cus, f"the library sizes launches for {ncus.value} CUs, torch reports {cus}"
    case = table_case(name, device)
    b, h, w, cin, cout, r, s, stride, pad = case.shape
    ho, wo = cp.out_size(h, w, r, s, stride, pad)
    x = torch.zeros((b, h, w, cin), device=device)
    wt = torch.zeros((cout, (r * s * cin + 31) // 32 * 32), device=device)
    bias = torch.arange(cout, dtype=torch.float32, device=device)
    out = GuardedOutput((b * ho * wo, cout), device)
    _lib.timing_enable(True)
    try:
        _lib.timing_read(_lib.ISC_KERNEL_CONV)  # clear
        _lib.check(lib.isc_conv2d_nhwc(x.data_ptr(), b, h, w, cin, wt.data_ptr(), cout, r, s, stride, pad, bias.data_ptr(), None,
                                       ACT_NONE, out.ptr, _lib.stream_handle(device)), name)
        _, launches = _lib.timing_read(_lib.ISC_KERNEL_CONV)
    finally:
        _lib.timing_enable(False)
    path = case.path(cus)
    assert launches == path.launches, (
        f"{name} {case.shape}: {launches} launches, tests/conv_paths.py expects {path.launches} ({path.form}: {path.kernels}) "
        f"on the {cus} CUs torch reports for this device"
    )
    assert torch.equal(out.result(name), bias.cpu().expand(b * ho * wo, cout))
