"""The split operand mode of the direct fp32 kernel (C2M_DIRECT_MATH = split: three bf16 pieces per fp32 value, six products on the
bf16 MFMA, csrc/conv_igemm.hip PREC = 2) against the fp32 MFMA mode and the fp64 CPU convolution: tails, 3-D strides, the parity
classes of a batched data gradient, K tails, 1x1, split-K, the deepest K of the model, operands spread over 80 binades, Inf / NaN.
Every case runs forward + backward once per mode (twice in split mode); the tests below only read those results."""
import ctypes
import functools
import os

import pytest
import torch

from c2m_amd import _lib, ops
from gpu_util import rel_close, rnd
from conv_route_cases import knobs
from test_gpu_conv_routes import _reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "C2M_DIRECT_MATH"
TILES, NSS = (32, 64, 128), (1, 2, 4)

# name -> (input shape, weight shape, stride, pad, reflect, knobs, variant)
CASES = {
    "1_tails": ((2, 24, 10, 14), (40, 24, 4, 4), (2, 2), (1, 1), True, {}, None),
    "2_3d_inplane_stride": ((1, 8, 4, 8, 12), (16, 8, 3, 4, 4), (1, 2, 2), (1, 1, 1), True, {}, None),
    "3_parity_classes": ((1, 8, 6, 8, 8), (16, 8, 4, 4, 4), (2, 2, 2), (1, 1, 1), True, {}, None),
    "4_k147_zero_pad": ((1, 3, 12, 20), (32, 3, 7, 7), (1, 1), (3, 3), False, {}, None),
    "5_1x1": ((2, 64, 8, 8), (128, 64, 1, 1), (1, 1), (0, 0), False, {}, None),
    "6_split_k": ((1, 512, 2, 4), (64, 512, 4, 4), (2, 2), (1, 1), False, {}, None),
    "7_k16384": ((1, 1024, 4, 4), (32, 1024, 4, 4), (2, 2), (1, 1), False, {}, None),
    "8_exponent_spread": ((2, 24, 10, 14), (40, 24, 4, 4), (2, 2), (1, 1), True, {}, "spread"),
    "9_nonfinite": ((2, 24, 10, 14), (40, 24, 4, 4), (2, 2), (1, 1), True, {}, "nonfinite"),
    # the remaining (tile, NS) instantiations: 128 rows with 8 / 3 input channels, 64 rows with 3
    "10_tile128_ns2": ((1, 8, 8, 8), (80, 8, 4, 4), (2, 2), (1, 1), True, {}, None),
    "11_tile128_ns4": ((1, 3, 8, 8), (80, 3, 7, 7), (1, 1), (3, 3), False, {}, None),
    "12_tile64_ns4": ((1, 3, 8, 8), (40, 3, 7, 7), (1, 1), (3, 3), False, {}, None),
}
FINITE = [k for k, c in CASES.items() if c[6] != "nonfinite"]


def _inputs(name):
    xs, ws, stride, pad, reflect, kn, variant = CASES[name]
    fan = 1
    for d in ws[1:]:
        fan *= d
    x, w, b = rnd(91, *xs), rnd(92, *ws, scale=(1.0 / fan) ** 0.5), rnd(93, ws[0], scale=0.1)
    if variant == "spread":       # channel c of the input times 2^e_c, e_c = -40 .. 40, the weights by the inverse: exact scalings
        e = torch.linspace(-40, 40, xs[1]).round()
        shape = (1, xs[1]) + (1,) * (len(xs) - 2)
        x, w = x * torch.exp2(e).view(shape), w * torch.exp2(-e).view(shape)
    if variant == "nonfinite":
        x[0, 3, 4, 5], x[1, 7, 2, 9] = float("inf"), float("nan")
    return x, w, b


def _run_mode(name, mode, x, w, b, go):
    """forward + backward with the knob at `mode` (None: unset).  -> y, dx, dw, db, routes, profiler (kind, tag) list, split counts."""
    xs, ws, stride, pad, reflect, kn, _ = CASES[name]
    L = _lib.lib()
    counts = (ctypes.c_int64 * 9)()
    old = os.environ.get(KNOB)
    try:
        if mode is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = mode
        with knobs(kn):
            xg, wg, bg = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
            pl = ops._plan(xg, wg, (1,) * (3 - len(stride)) + stride, (0,) * (3 - len(pad)) + pad, reflect, None)
            assert L.c2m_direct_math_counts(None, 1) == 9
            with ops.ConvProfiler() as prof:
                y = ops.conv(xg, wg, bg, stride=stride, padding=pad, padding_mode="reflect" if reflect else "zeros")
                (y * go.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            L.c2m_direct_math_counts(counts, 0)
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old
    return dict(y=y.detach().cpu(), dx=xg.grad.cpu(), dw=wg.grad.cpu(), db=bg.grad.cpu(),
                routes=(pl.fwd_route, pl.dgrad_route, pl.wgrad_route), prof=[(r[0], tuple(r[4])) for r in prof.records],
                counts=list(counts))


@functools.lru_cache(maxsize=None)
def _results(name):
    xs, ws, stride, pad, reflect, kn, variant = CASES[name]
    prev = ops.set_conv_precision("fp32")
    try:
        x, w, b = _inputs(name)
        xg, wg = x.to(DEV), w.to(DEV)
        with knobs(kn), torch.no_grad():
            yshape = ops.conv(xg, wg, None, stride=stride, padding=pad, padding_mode="reflect" if reflect else "zeros").shape
        go = rnd(94, *yshape)
        out = {m: _run_mode(name, m, x, w, b, go) for m in ("split", "fp32", None)}
        out["split_again"] = _run_mode(name, "split", x, w, b, go)
        if variant != "nonfinite":
            out["ref"] = _reference(x, w, b, (1,) * (3 - len(stride)) + stride, (0,) * (3 - len(pad)) + pad, reflect, go)
        out["go"], out["cout"] = go, ws[0]
        return out
    finally:
        ops.set_conv_precision(prev)


@pytest.mark.parametrize("mode", ["split", "fp32"])
@pytest.mark.parametrize("name", FINITE)
def test_gates(name, mode):
    r = _results(name)
    got, (yr, gxr, gwr, gbr) = r[mode], r["ref"]
    rel_close(got["y"], yr, 2e-5, "forward")
    rel_close(got["dx"], gxr, 5e-5, "data gradient")
    rel_close(got["dw"], gwr, 1e-4, "weight gradient")
    rel_close(got["db"], gbr, 1e-4, "bias gradient", floor=1e-3 * float(r["go"].abs().sum()) / r["cout"])


@pytest.mark.parametrize("name", [k for k in FINITE if int(k.split("_")[0]) <= 8])
def test_split_forward_is_five_times_under_its_gate(name):
    r = _results(name)
    err = (r["split"]["y"].double() - r["ref"][0]).abs().max().item() / r["ref"][0].abs().max().item()
    ferr = (r["fp32"]["y"].double() - r["ref"][0]).abs().max().item() / r["ref"][0].abs().max().item()
    print(f"{name}: forward error over max |ref|: split {err:.3e}, fp32 {ferr:.3e}")
    rel_close(r["split"]["y"], r["ref"][0], 2e-5 / 5, "forward, split")


@pytest.mark.parametrize("name", list(CASES))
def test_routes_and_profiler_records_do_not_depend_on_the_mode(name):
    r = _results(name)
    assert r["split"]["routes"] == r["fp32"]["routes"] == r[None]["routes"]
    assert r["split"]["prof"] == r["fp32"]["prof"] == r[None]["prof"]
    assert {k for k, _ in r["split"]["prof"]} <= {"igemm", "wgrad"}      # the direct family, under its own names
    assert sum(r["split"]["counts"]) >= 2 and sum(r["fp32"]["counts"]) == 0   # forward and data gradient ran split / none did


@pytest.mark.parametrize("name", list(CASES))
def test_split_is_bit_repeatable(name):
    r = _results(name)
    for k in ("y", "dx", "dw", "db"):
        a, b = r["split"][k], r["split_again"][k]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k      # (bit patterns: NaN == NaN)


def test_nonfinite_inputs_reach_the_output():
    r = _results("9_nonfinite")
    for k in ("y", "dw"):
        bad = ~torch.isfinite(r["fp32"][k])
        assert bad.any() and not torch.isfinite(r["split"][k][bad]).any(), k
    assert bool((~torch.isfinite(r["split"]["y"])).sum() == (~torch.isfinite(r["fp32"]["y"])).sum())


def test_fp32_mode_is_the_unset_knob_where_auto_keeps_fp32():
    """`auto` leaves the launches of the 32-row tile (M <= 32) on the fp32 MFMA (igemm_split_pays, csrc/conv_igemm.hip): in the cases
    whose forward and data gradient both have at most 32 rows (2, 3, 4) the unset knob and C2M_DIRECT_MATH=fp32 launch the same
    kernels on the same operands."""
    for name in ("2_3d_inplane_stride", "3_parity_classes", "4_k147_zero_pad"):
        r = _results(name)
        assert sum(r[None]["counts"]) == 0, name
        for k in ("y", "dx", "dw", "db"):
            assert torch.equal(r[None][k].view(torch.int32), r["fp32"][k].view(torch.int32)), (name, k)


def test_every_split_instantiation_is_reached():
    seen = [0] * 9
    for name in CASES:
        seen = [a + b for a, b in zip(seen, _results(name)["split"]["counts"])]
    missing = [(TILES[i // 3], NSS[i % 3]) for i, n in enumerate(seen) if n == 0]
    assert not missing, f"no case launches the split kernel with (tile rows, NS) = {missing}"
