"""L1 mean, SSIM, RoIAlign and bf16 max-pool kernels at their launch edges (run with -m gpu), against the float64 references
of loss_edges_ref.py on the same input values.  test_loss_edges_cpu.py checks those references and the input conditions.

Launch edge -> case that reaches it
  second lap of the grid-stride loop      L1 lap2-* (262500 elements > 1024 blocks x 256), SSIM (4,3,150,150) (262848 windows)
  1024 partials into final_sum_kernel     the same cases (four rounds of its 256 threads)
  masked index arithmetic                 L1 masked cases: (C, inner) = (3, 960), (5, 17500), (7, 99), (1, 2145), (1, 1)
  masked bf16                             L1 *-bf16-frac, *-bf16-binary, one-bf16-masked
  non-contiguous a, stride-0 mask         L1 odd-f32-views
  H == 3 and W == 3 planes                SSIM (1,1,3,3), (1,1,3,70), (1,2,70,3)
  C % 8 != 0, C > 8                       RoI C1-*, C9-*, C19-* (C3 in the K520 / K0 / one-row cases)
  K > 512 (box list in global memory)     RoI C3-bins7-K520
  boxes straddling and leaving the map    RoI *-K19 (the hand-written list: every border, outside, reversed, zero, sub-pixel)
  an image without boxes                  RoI: image 2 of every [3,C,10,13] case; C3-bins3x5-K0 has no box at all
  one-row / one-column maps               RoI row1x9-*, col9x1-*
  bf16 max-pool at odd extents            max-pool (2,3,7,9), (1,2,6,5), (1,1,3,2): the general (per-pixel) bf16 kernel

Bounds -- none is taken from what the kernels return, except M_SSIM, which is measured as described below
  L1 value      2e-6 relative: a thread adds at most ceil(total / 262144) + 1 = 3 terms in fp32, the rest is float64.
  L1 gradients  fp32: 1e-6 relative, no absolute term (g * sign * m / total: three roundings).  bf16: 2^-8 relative (one bf16
                rounding of that fp32 value).  Exactly 0 on the planted a == b block and wherever the mask is 0.
  SSIM          err <= M_SSIM * E32 + floor, where err is the kernel's deviation from ssim_ref(float64) and E32 that of
                ssim_ref(float32) on the same input (absolute for the loss, max abs for the gradient); floor = 1e-7 for the loss
                and 1e-6 * max|grad64| for the gradient.  M_SSIM is twice the largest ratio err / max(E32, floor) seen on the
                MI355X (table below) and must stay <= 8: above that the kernel would be less accurate than the formula is in fp32.
                `flat` (0.7 + 1e-4 noise against 0.7) is judged on the loss alone plus a finite gradient: E[x^2] - mu^2
                cancels all but one or two bits there, in the reference's own fp32 arithmetic as much as in the kernel's,
                and a third of the windows land in the clamp, where the gradient is 0 on one side and not on the other.
                `equal` (x is y) has loss 0 and gradient 0 analytically and is judged by the floors alone; its gradient
                floor takes its scale from the same x against an independent target (`rand01`), as its own is 0.
  RoIAlign      max abs err <= 1e-5 * max|ref| for the output and for d feat (an fp32 emulation of the gather is within 7e-7
                of float64 on inputs that keep every sample off the cutoff; a misplaced tap or a dropped sample shows at 1e-2).
  max-pool      bit-equal to F.max_pool2d on the fp32 copy of the bf16 values, output and input gradient: a maximum and a
                copy round nothing.

Measured on the MI355X (each test prints its figures before it asserts)
  L1       value: worst relative error 5.1e-8 (lap2-f32-frac).  Gradients: fp32 worst 1.2e-7 (c1-f32-frac), bf16 worst 3.84e-3
           = 0.98 * 2^-8 (golden-bf16-frac); zeros exact.
  SSIM     err / max(E32, floor), loss | gradient, at (2,3,33,47):
             rand01 0.30 | 0.99   rand+-1 0.15 | 1.04   near_equal 0.18 | 0.97   smooth_shift 0.49 | 0.93   anti 0.07 | 0.90
             flat 1.12 | (0.69, not judged)   equal: loss err 1.1e-8 (floor 1e-7), gradient err 2.6e-10 (floor 5.2e-10)
           rand01 and smooth_shift at the edge shapes: (1,1,3,3) 0.48 | 0.35 and 0.50 | 0.73; (1,1,3,70) 0.17 | 0.64 and
           0.65 | 0.93; (1,2,70,3) 0.19 | 0.55 and 0.26 | 1.12; (4,3,150,150) 0.19 | 0.76 and 0.41 | 0.94.
           Largest 1.12 (flat's loss; smooth_shift's gradient at (1,2,70,3)) -> M_SSIM = 2.24: the kernel is as accurate as
           the formula evaluated in fp32, no family stands out.
  RoIAlign worst out err / max|ref| 1.22e-6 (C3-bins7-K520), worst d feat err / max|ref| 7.5e-7 (C19-bins7-K19); the all-zero
           results (image 2, the boxes outside the map, K = 0) are exact.
  max-pool bit-equal.
"""
import pytest
import torch
import torch.nn.functional as F

import loss_edges_ref as R
from c2m_amd import ops
from gpu_util import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M_SSIM = 2.24
assert M_SSIM <= 8.0
L1_VALUE_RTOL, L1_GRAD_RTOL, BF16_RTOL = 2e-6, 1e-6, 2.0 ** -8
SSIM_LOSS_FLOOR, SSIM_GRAD_FLOOR = 1e-7, 1e-6
ROI_TOL = 1e-5
_refs = {}


def g(t):
    return t.to(DEV)


def _ids(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


# ----------------------------------------------------------------------------------------------- L1 mean
@pytest.mark.parametrize("case", R.L1_CASES, ids=repr)
def test_l1_mean_value_and_both_gradients(case):
    a, b, mask, same = R.l1_inputs(case)
    off, on, mpos = R.l1_separation(a, b, mask, same)
    assert off >= R.L1_SEP and on == 0.0 and mpos >= 0.05
    v64, ga64, gb64 = R.l1_ref_grads(a, b, mask, 1.7)
    md = None if mask is None else g(mask)
    if case.view:
        junk = torch.full_like(a[:, :1], 7.0)
        ad = g(torch.cat([junk, a, junk], 1))[:, 1:-1]
        base = mask[(slice(None), slice(None)) + (slice(0, 1),) * (mask.dim() - 3)].contiguous()
        md = g(base).expand(mask.shape)
        assert not ad.is_contiguous() and 0 in md.stride() and torch.equal(md.cpu(), mask)
    else:
        ad = g(a)
    ad, bd = ad.requires_grad_(True), g(b).requires_grad_(True)
    loss = ops.l1_mean(ad, bd, md)
    (loss * 1.7).backward()
    ga, gb = ad.grad.cpu(), bd.grad.cpu()
    assert loss.dtype == torch.float32 and ga.dtype == a.dtype and gb.dtype == b.dtype and ga.shape == a.shape
    verr = abs(loss.item() - v64.item()) / v64.item() if v64.item() else abs(loss.item())
    nz = ga64 != 0
    gerr = max(((t.double() - r).abs()[nz] / r.abs()[nz]).max().item() if nz.any() else 0.0 for t, r in ((ga, ga64), (gb, gb64)))
    print(f"l1 {case}: value rel err {verr:.2e}, worst gradient rel err {gerr:.2e}")
    assert verr <= L1_VALUE_RTOL
    rtol = BF16_RTOL if case.dtype == "bf16" else L1_GRAD_RTOL
    torch.testing.assert_close(ga.double(), ga64, rtol=rtol, atol=0.0)
    torch.testing.assert_close(gb.double(), gb64, rtol=rtol, atol=0.0)
    assert not ga[same].any() and not gb[same].any(), "planted a == b block: sign 0"
    if mask is not None:
        off_mask = (mask == 0).expand_as(a)
        assert not ga[off_mask].any() and not gb[off_mask].any()


# ----------------------------------------------------------------------------------------------- SSIM
def _ssim_refs(family, shape):
    key = ("ssim", family, shape)
    if key not in _refs:
        x, y = R.ssim_inputs(family, shape)
        _refs[key] = (x, y) + R.ssim_ref_grad(x, y, torch.float64) + R.ssim_ref_grad(x, y, torch.float32)
    return _refs[key]


def _ssim_run(x, y, same=False):
    xd = g(x).requires_grad_(True)
    loss = ops.ssim_loss(xd, xd.detach() if same else g(y))
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("family,shape", R.SSIM_CASES, ids=_ids)
def test_ssim_loss_and_gradient_within_the_fp32_yardstick(family, shape):
    x, y, v64, g64, v32, g32 = _ssim_refs(family, shape)
    loss, gx = _ssim_run(x, y, same=family == "equal")
    assert loss.dtype == torch.float32 and gx.dtype == torch.float32 and gx.shape == x.shape
    assert torch.isfinite(loss) and torch.isfinite(gx).all()
    e32_l, e32_g = abs(v32.item() - v64.item()), (g32 - g64).abs().max().item()
    err_l, err_g = abs(loss.item() - v64.item()), (gx.double() - g64).abs().max().item()
    gscale = g64.abs().max().item()
    if family == "equal":
        gscale = _ssim_refs("rand01", shape)[3].abs().max().item()
    fl_l, fl_g = SSIM_LOSS_FLOOR, SSIM_GRAD_FLOOR * gscale
    print(f"ssim {family} {shape}: loss {v64.item():.3e} err {err_l:.2e} E32 {e32_l:.2e} ratio {err_l / max(e32_l, fl_l):.2f}; "
          f"max|grad| {gscale:.3e} err {err_g:.2e} E32 {e32_g:.2e} ratio {err_g / max(e32_g, fl_g):.2f}")
    if family == "equal":
        assert err_l <= fl_l and err_g <= fl_g
        return
    assert err_l <= M_SSIM * e32_l + fl_l
    if family != "flat":
        assert err_g <= M_SSIM * e32_g + fl_g


def test_ssim_bf16_input_runs_the_fp32_kernel_on_the_rounded_values():
    x, y = R.ssim_inputs("smooth_shift", R.SSIM_MAIN_SHAPE)
    xb, yb = x.bfloat16(), y.bfloat16()
    xd = g(xb).requires_grad_(True)
    loss = ops.ssim_loss(xd, g(yb))
    loss.backward()
    loss32, gx32 = _ssim_run(xb.float(), yb.float())
    assert xd.grad.dtype == torch.bfloat16 and loss.dtype == torch.float32
    assert torch.equal(loss.cpu(), loss32) and torch.equal(xd.grad.cpu(), gx32.bfloat16())


def test_ssim_backward_is_bit_repeatable():
    x, y = R.ssim_inputs("rand01", R.SSIM_EDGE_SHAPES[-1])
    (l1, g1), (l2, g2) = _ssim_run(x, y), _ssim_run(x, y)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ----------------------------------------------------------------------------------------------- RoIAlign
def _roi_refs(case):
    key = ("roi", case.name)
    if key not in _refs:
        feat, gout = case.tensors()
        _refs[key] = (feat, gout) + R.roi_ref(feat, case.boxes, case.bins, R.ROI_SCALE, gout)
    return _refs[key]


@pytest.mark.parametrize("case", R.ROI_CASES, ids=repr)
def test_roi_align_forward_and_gather_backward(case):
    if case.K:
        assert R.roi_sample_margin(case.boxes, case.bins, R.ROI_SCALE, case.H, case.W) >= R.ROI_MARGIN
        assert 0 <= int(case.boxes[:, 0].min()) and int(case.boxes[:, 0].max()) < case.N
    feat, gout, out64, gfeat64 = _roi_refs(case)
    grads = []
    for _ in range(2):
        fd = g(feat).requires_grad_(True)
        out = ops.roi_align(fd, g(case.boxes), case.bins, spatial_scale=R.ROI_SCALE)
        poison(torch.cuda.current_stream(), fd)                  # d feat comes from torch.empty: the kernel writes every zero
        (out * g(gout)).sum().backward()
        grads.append(fd.grad.cpu())
    out, gfeat = out.detach().cpu(), grads[0]
    assert out.shape == out64.shape and gfeat.shape == feat.shape and out.dtype == gfeat.dtype == torch.float32
    assert torch.equal(grads[0], grads[1]), "d feat is not bit-repeatable"
    so, sg = out64.abs().max().item() if case.K else 0.0, gfeat64.abs().max().item()
    eo = (out.double() - out64).abs().max().item() if case.K else 0.0
    eg = (gfeat.double() - gfeat64).abs().max().item()
    print(f"roi {case}: out err / max|ref| {eo / so if so else 0.0:.2e}, d feat err / max|ref| {eg / sg if sg else eg:.2e}")
    assert eo <= ROI_TOL * so and eg <= ROI_TOL * sg
    if case.N == 3:
        assert not gfeat[2].any(), "image 2 has no box"
    if case.K == 19:
        outside = [k for k, b in enumerate(R.ROI_BOXES) if b[1] > 60 or b[3] < -4]
        assert len(outside) == 2 and not out[outside].any()


# ----------------------------------------------------------------------------------------------- max-pool, bf16, odd extents
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=_ids)
def test_maxpool_bf16_general_kernel_bit_equal(shape):
    x, gout = R.pool_inputs(shape)
    xr = x.float().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    (yr * gout.float()).sum().backward()
    xd = g(x).requires_grad_(True)
    y = ops.maxpool2x2(xd)
    y.backward(g(gout))
    assert y.dtype == torch.bfloat16 and xd.grad.dtype == torch.bfloat16
    assert torch.equal(y.detach().float().cpu(), yr.detach())
    assert torch.equal(xd.grad.float().cpu(), xr.grad)
