"""Every conv route by name (ops._ConvPlan.fwd_route / dgrad_route / wgrad_route) on the smallest layer of the suite that takes it: the
launches a forward + backward records under ops.ConvProfiler carry the profiler kind and tag suffix ops._ROUTE_PROF lists for the
plan's route names -- the name IS what was launched --, and outputs and gradients meet the fp64 reference at the gates of
test_gpu_ops.py (fp32) and test_gpu_nc8.py / test_gpu_g8.py (bf16, with the unused NCHW storage of NC8-only gradients poisoned)."""
import pytest
import torch
import torch.nn.functional as F

from c2m_amd import ops
from gpu_util import rel_close, rnd
from conv_route_cases import TABLE, knobs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [c for c in TABLE if c[0][0] < 40]         # (the model-size rows of the table are routing statements only)


def _id(c):
    return "x".join(map(str, c[0])) + "-co%d-k%s-s%s-%s-%s-%s" % (
        c[1][0], "".join(map(str, c[1][2:])), "".join(map(str, c[2])), "reflect" if c[4] else "zeros", "bf16" if c[5] else "fp32",
        ",".join(f"{k}={v}" for k, v in c[7].items()) or "auto")


def _reference(x, w, b, stride, pad, reflect, go):
    """fp64 convolution and its gradients on the CPU."""
    nd = x.dim() - 2
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    pads = [p for q in reversed(pad[3 - nd:]) for p in (q, q)]
    xp = F.pad(xr, pads, mode="reflect") if reflect else F.pad(xr, pads)
    y = (F.conv3d if nd == 3 else F.conv2d)(xp, wr, br, stride=stride[3 - nd:])
    (y * go.double()).sum().backward()
    return y.detach(), xr.grad, wr.grad, br.grad


def _expected(pl, table, route, head):
    kind, suffix = ops._ROUTE_PROF[table][route]
    return (kind + ("_bf16" if pl.bf16 else ""), head, suffix[-1] if suffix else None)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_route_is_what_is_launched(case):
    xs, ws, stride, pad, reflect, bf16, rows, kn, want = case
    nd = len(xs) - 2
    q = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)       # bf16: representable operands, every product exact in fp32
    x, w = q(rnd(81, *xs)), q(rnd(82, *ws, scale=(1.0 / (ws[1] * ws[2] * ws[3] * (ws[4] if nd == 3 else 1))) ** 0.5))
    b = rnd(83, ws[0], scale=0.1)
    prev = ops.set_conv_precision("bf16" if bf16 else "fp32")
    poison = ops._NC8_POISON
    try:
        with knobs(kn):
            ops._NC8_POISON = bool(bf16)
            xg, wg, bg = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
            pl = ops._plan(xg, wg, stride, pad, reflect, rows)
            assert (pl.fwd_route, pl.dgrad_route, pl.wgrad_route) == want
            with ops.ConvProfiler() as prof:
                y = ops.conv(xg, wg, bg, stride=stride[3 - nd:], padding=pad[3 - nd:], padding_mode="reflect" if reflect else "zeros",
                             dgrad_channels=rows)
                go = q(rnd(84, *y.shape))
                (y.float() * go.to(DEV)).sum().backward()
            torch.cuda.synchronize()
    finally:
        ops._NC8_POISON = poison
        ops.set_conv_precision(prev)
    # ---- the name is what was launched: (kind, pass, last tag entry) of every recorded launch
    seen = {}
    for kind, _, _, _, tag, _ in prof.records:
        last = tag[-1] if isinstance(tag[-1], str) else None           # (a c2m_conv_igemm / c2m_conv_wgrad tag without suffix ends in its split count)
        seen.setdefault(tag[0], set()).add((kind, tag[0], last))
    assert seen == {"fwd": {_expected(pl, "conv", pl.fwd_route, "fwd")}, "dgrad": {_expected(pl, "conv", pl.dgrad_route, "dgrad")},
                    "wgrad": {_expected(pl, "wgrad", pl.wgrad_route, "wgrad")}}
    # ---- and it computes the convolution
    yr, gxr, gwr, gbr = _reference(x, w, b, stride, pad, reflect, go)
    assert y.dtype == (torch.bfloat16 if (bf16 and ws[0] > 4) else torch.float32)
    rel_close(y.float(), yr, 4e-3 if y.dtype == torch.bfloat16 else 2e-5, "forward")
    n = rows or xs[1]
    rel_close(xg.grad[:, :n], gxr[:, :n], 5e-5, "data gradient")
    assert rows is None or float(xg.grad[:, n:].abs().max()) == 0.0
    rel_close(wg.grad, gwr, 1e-4, "weight gradient")
    # (fp32 gate of test_gpu_ops.py: a bias gradient is a plain sum of either sign, its rounding error scales with sum |go|; the bf16
    # files gate it without that floor)
    rel_close(bg.grad, gbr, 1e-4, "bias gradient", floor=0.0 if bf16 else 1e-3 * float(go.abs().sum()) / ws[0])
