"""ops.resize_bilinear_grad: the differentiable bilinear resize of the frame sizes that are not multiples of 64 (run with -m gpu).

Forward = c2m_resize_bilinear, backward = its gather-form adjoint c2m_resize_bilinear_bwd (no float atomics).  Checked
against torch's CPU autograd of F.interpolate(mode="bilinear") in fp64 (norm-wise) and in fp32 (element-wise: the same
fp32 coordinate arithmetic, only the summation order differs)."""
import pytest
import torch
import torch.nn.functional as F

from c2m_amd import ops
from gpu_util import rel_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (input shape, output size): the model's own instances (12->13, 46->47, 184->188), 6->13, down-sampling (13->6, 47->23),
# degenerate extents (1->k, k->1) and a 5-D [B,C,T,H,W] map
SHAPES = [
    ((2, 3, 12, 12), (13, 13)),
    ((1, 4, 46, 47), (47, 52)),
    ((1, 2, 184, 352), (188, 352)),
    ((2, 3, 6, 6), (13, 13)),
    ((2, 3, 13, 13), (6, 6)),
    ((1, 5, 47, 47), (23, 23)),
    ((2, 2, 1, 1), (7, 9)),
    ((2, 2, 1, 9), (5, 9)),
    ((2, 2, 7, 9), (1, 1)),
    ((2, 2, 9, 1), (9, 4)),
    ((2, 3, 5, 12, 13), (13, 26)),
    ((1, 4, 5, 23, 11), (23, 12)),
]
IDS = [f"{'x'.join(map(str, s[-2:]))}to{o[0]}x{o[1]}_{len(s)}d" for s, o in SHAPES]


def _ref(x, size, align):
    """torch CPU autograd; 5-D maps as the reference's resize_video (fold the time axis, interpolate, unfold)."""
    if x.dim() == 5:
        B, C, T, H, W = x.shape
        y = F.interpolate(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), size=size, mode="bilinear", align_corners=align)
        return y.reshape(B, T, C, *size).permute(0, 2, 1, 3, 4)
    return F.interpolate(x, size=size, mode="bilinear", align_corners=align)


def _run(x, size, align, go, dtype=torch.float32):
    xg = x.to(DEV, dtype).requires_grad_(True)
    y = ops.resize_bilinear_grad(xg, size, align_corners=align)
    y.backward(go.to(DEV, dtype))
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape,size", SHAPES, ids=IDS)
def test_resize_grad_vs_torch(shape, size, align):
    x = rnd(11, *shape)
    out_shape = shape[:-2] + size
    go = rnd(12, *out_shape)
    y, gx = _run(x, size, align, go)
    assert y.shape == out_shape and gx.shape == shape
    # fp64 reference, norm-wise (its coordinates are fp64; ours are ATen's fp32 ones)
    x64 = x.double().requires_grad_(True)
    y64 = _ref(x64, size, align)
    y64.backward(go.double())
    for a, b, what in ((y, y64, "fwd"), (gx, x64.grad, "bwd")):
        a, b = a.cpu().double(), b.detach()
        err = float((a - b).norm() / max(float(b.norm()), 1e-30))
        assert err <= 1e-5, f"{what}: relative L2 error {err:.2e} vs fp64"
    # fp32 reference with the same coordinate arithmetic, element-wise
    x32 = x.clone().requires_grad_(True)
    y32 = _ref(x32, size, align)
    y32.backward(go)
    rel_close(y, y32, 1e-5, "fwd vs fp32 CPU")
    rel_close(gx, x32.grad, 1e-5, "bwd vs fp32 CPU")


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape,size", SHAPES, ids=IDS)
def test_resize_grad_bf16(shape, size, align):
    """bf16 I/O, fp32 arithmetic: the fp32 HIP op on the same (bf16-representable) values, then one RNE rounding."""
    x = rnd(21, *shape).bfloat16().float()
    go = rnd(22, *(shape[:-2] + size)).bfloat16().float()
    y, gx = _run(x, size, align, go)
    yb, gxb = _run(x, size, align, go, torch.bfloat16)
    assert yb.dtype == torch.bfloat16 and gxb.dtype == torch.bfloat16
    rel_close(yb.float(), y, 2 ** -8, "bf16 fwd")
    rel_close(gxb.float(), gx, 2 ** -8, "bf16 bwd")
    assert torch.equal(yb.float(), y.bfloat16().float()), "forward: fp32 result rounded once"
    assert torch.equal(gxb.float(), gx.bfloat16().float()), "backward: fp32 sum rounded once"


def test_resize_grad_repeatable_and_matches_no_grad_op():
    x = rnd(31, 2, 8, 5, 184, 352)
    go = rnd(32, 2, 8, 5, 188, 352).to(DEV)
    runs = [_run(x, (188, 352), False, go) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    x4 = x.to(DEV).reshape(16, 5, 184, 352)
    assert torch.equal(ops.resize_bilinear(x4, (188, 352)).reshape(runs[0][0].shape), runs[0][0]), \
        "forward must give the bits of ops.resize_bilinear"


def test_resize_grad_graph_replay_equals_eager():
    """Forward and backward captured into a HIP graph.  Every step runs on the capture stream (as TrainStep.capture
    arranges it): autograd work left on another stream would need cross-stream syncs inside the capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = rnd(41, 2, 4, 46, 47).to(DEV).requires_grad_(True)
        go = rnd(42, 2, 4, 47, 52).to(DEV)

        def step():
            y = ops.resize_bilinear_grad(x, (47, 52))
            gx, = torch.autograd.grad(y, x, go)
            return y, gx

        ye, ge = (t.clone() for t in step())
        step()                                        # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        yg, gg = step()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, ye) and torch.equal(gg, ge)


def test_resize_grad_same_size_returns_input():
    x = rnd(51, 1, 2, 3, 12, 13).to(DEV).requires_grad_(True)
    assert ops.resize_bilinear_grad(x, (12, 13)) is x
    assert ops.resize_bilinear_grad(x, [12, 13], align_corners=True) is x


def test_resize_grad_rejects_bad_input_and_no_grad_op_keeps_its_contract():
    with pytest.raises(ValueError):
        ops.resize_bilinear_grad(torch.zeros(3, 4, 5, device=DEV), (6, 7))
    with pytest.raises(RuntimeError):
        ops.resize_bilinear(torch.zeros(1, 1, 4, 4, device=DEV, requires_grad=True), (5, 5))
