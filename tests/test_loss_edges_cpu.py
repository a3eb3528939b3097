"""No GPU: what makes test_gpu_loss_edges.py trustworthy.  The float64 references of loss_edges_ref.py reproduce the golden
vectors captured from the reference implementation; roi_ref agrees with an unpruned sample-by-sample loop written here; and
every case meets the input condition its comparison rests on (loss_edges_ref.py's docstring states them)."""
import math

import numpy as np
import pytest
import torch

import loss_edges_ref as R
from golden_io import Case


def fold_time(x):
    return torch.cat(torch.unbind(x, 2), 0)


# ----------------------------------------------------------------------------------------------- references vs golden
def test_l1_and_ssim_references_reproduce_the_golden_losses():
    c = Case("op_losses")
    i, o, gin = c.group("in"), c.group("out"), c.group("gin")
    a = i["a"].double().requires_grad_(True)
    b, m = i["b"].double(), i["mask"]
    ssim = R.ssim_ref(fold_time(a), fold_time(b), torch.float64)
    l1, l1m = R.l1_ref(a, b), R.l1_ref(a, b, m)
    (ssim * 1.5 + l1 * 0.7 + l1m * 2.0).backward()
    for name, got, want in (("ssim", ssim, o["ssim"]), ("l1", l1, o["l1"]), ("l1_masked", l1m, o["l1_masked"])):
        rel = abs(got.item() - want.item()) / abs(want.item())
        print(f"{name}: rel {rel:.2e}")
        assert rel <= 1e-6, name
    want = gin["a"].double()
    err = (a.grad - want).abs().max().item() / want.abs().max().item()
    print(f"d a: max abs err / max|grad| {err:.2e}")
    assert err <= 1e-6


def test_ssim_float32_yardstick_is_the_same_formula():
    x, y = R.ssim_inputs("rand01", R.SSIM_MAIN_SHAPE)
    v64, g64 = R.ssim_ref_grad(x, y, torch.float64, 1.3)
    v32, g32 = R.ssim_ref_grad(x, y, torch.float32, 1.3)
    assert abs(v32 - v64) <= 1e-6 * v64 and (g32 - g64).abs().max() <= 1e-5 * g64.abs().max()
    assert x.dtype == y.dtype == torch.float32


# ----------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("case", R.L1_CASES, ids=repr)
def test_l1_case_keeps_the_sign_away_from_rounding(case):
    a, b, mask, same = R.l1_inputs(case)
    assert a.shape == case.shape and a.dtype == b.dtype == (torch.bfloat16 if case.dtype == "bf16" else torch.float32)
    off, on, mpos = R.l1_separation(a, b, mask, same)
    assert off >= R.L1_SEP and on == 0.0 and mpos >= 0.05, (off, on, mpos)
    assert a.numel() == 1 or same.any()
    assert float(a.float().abs().max()) < 4.0 and float(b.float().abs().max()) < 4.0
    if case.mask is not None:
        assert mask.shape == (a.shape[0], 1) + a.shape[2:] and mask.dtype == torch.float32
        assert float(mask.min()) >= 0.0 and float(mask.max()) <= 1.0
        if case.mask == "frac":
            assert a.numel() == 1 or ((mask > 0) & (mask < 1)).any()
        if a.numel() > 1:
            assert (mask == 0).any() and (mask > 0).any()
        if not case.view and len(a.shape) > 2 and a.shape[-2] > 1:
            assert not mask[..., 0, :].any()
    _, ga, gb = R.l1_ref_grads(a, b, mask, 1.7)
    assert not ga[same].any() and not gb[same].any()          # sign 0 on the planted block
    assert torch.equal(ga, -gb)


def test_l1_cases_cover_what_the_kernel_branches_on():
    n = {c.name: math.prod(c.shape) for c in R.L1_CASES}
    assert n["lap2-f32-frac"] == 262500 > 1024 * 256               # second lap of the grid-stride loop, 1024 partials
    assert {(c.dtype, c.mask is not None) for c in R.L1_CASES} == {("f32", False), ("f32", True), ("bf16", False), ("bf16", True)}
    assert {c.mask for c in R.L1_CASES} == {None, "binary", "frac"} and any(c.view for c in R.L1_CASES)
    masked = [c for c in R.L1_CASES if c.mask]
    assert len({(c.shape[1], math.prod(c.shape[2:])) for c in masked}) >= 4          # (C, inner) pairs


@pytest.mark.parametrize("family,shape", [(f, s) for f, s in R.SSIM_CASES if f in R.SSIM_OFF_CLAMP],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_ssim_case_stays_off_the_clamp(family, shape):
    x, y = R.ssim_inputs(family, shape)
    frac = R.ssim_near_clamp_fraction(x, y)
    print(f"{family} {shape}: {100 * frac:.3f} % of the windows within {R.SSIM_CLAMP_MARGIN} of the clamp")
    assert frac < 0.01
    if family == "near_equal":
        assert frac == 0.0


def test_ssim_special_families_are_what_they_claim():
    x, y = R.ssim_inputs("equal", R.SSIM_MAIN_SHAPE)
    assert x is y
    v, gx = R.ssim_ref_grad(x, y.clone(), torch.float64)
    assert v.item() <= 1e-15 and gx.abs().max().item() <= 1e-12          # ssim == 1: a minimum of the unclamped term
    x, y = R.ssim_inputs("flat", R.SSIM_MAIN_SHAPE)
    v64 = R.ssim_ref(x, y, torch.float64).item()
    v32 = R.ssim_ref(x, y, torch.float32).item()
    print(f"flat: loss {v64:.3e} in float64, {v32:.3e} in float32")
    assert v64 < 1e-4 and abs(v32 - v64) > 0.05 * v64                    # fp32 itself is noise here
    n = R.SSIM_EDGE_SHAPES[-1]
    assert n[0] * n[1] * (n[2] - 2) * (n[3] - 2) == 262848 > 1024 * 256


@pytest.mark.parametrize("case", R.ROI_CASES, ids=repr)
def test_roi_case_keeps_every_sample_off_the_cutoff(case):
    b = case.boxes
    assert b.shape == (case.K, 5)
    if case.K:
        assert torch.equal(b[:, 1:] * 2, (b[:, 1:] * 2).round()), "half-pixel grid"
        idx = b[:, 0]
        assert float(idx.min()) >= 0 and float(idx.max()) < case.N and torch.equal(idx, idx.round())
        assert case.N < 3 or not (idx == 2).any()
        margin = R.roi_sample_margin(b, case.bins, R.ROI_SCALE, case.H, case.W)
        print(f"{case}: margin {margin:.4f}")
        assert margin >= R.ROI_MARGIN


def test_roi_box_list_holds_every_kind_of_box():
    H, W = R.ROI_MAP
    kinds = set()
    for (_, x1, y1, x2, y2) in R.ROI_BOXES:
        x1, y1, x2, y2 = (v * R.ROI_SCALE for v in (x1, y1, x2, y2))
        if x2 < x1 or y2 < y1:
            kinds.add("reversed")
        elif x2 == x1 and y2 == y1:
            kinds.add("zero")
        elif x1 > W + 1 or y1 > H + 1 or x2 < -1 or y2 < -1:
            kinds.add("outside")
        elif x1 < 0 and y1 < 0 and x2 > W and y2 > H:
            kinds.add("larger")
        elif (x1, y1, x2, y2) == (0, 0, W, H):
            kinds.add("whole")
        elif x1 < 0:
            kinds.add("left")
        elif x2 > W:
            kinds.add("right")
        elif y1 < 0:
            kinds.add("top")
        elif y2 > H:
            kinds.add("bottom")
        elif x2 - x1 < 1 and y2 - y1 < 1:
            kinds.add("subpixel")
        else:
            kinds.add("inside")
    assert kinds == {"reversed", "zero", "outside", "larger", "whole", "left", "right", "top", "bottom", "subpixel", "inside"}
    assert {c.C for c in R.ROI_CASES} >= {1, 8, 9, 19} and max(c.K for c in R.ROI_CASES) > 512


# ----------------------------------------------------------------------------------------------- roi_ref vs a plain loop
def _roi_loop(feat, boxes, bins, scale, gout):
    """RoIAlign(aligned=False, sampling_ratio=-1) one sample at a time in float64, nothing pruned and nothing vectorised:
    out [K,C,PH,PW] and d feat of sum(out * gout)."""
    feat, gout = feat.double().numpy(), gout.double().numpy()
    N, C, H, W = feat.shape
    PH, PW = bins
    out = np.zeros((len(boxes), C, PH, PW))
    gfeat = np.zeros_like(feat)

    def taps(v, S):
        if v < -1.0 or v > S:
            return None
        v = max(v, 0.0)
        lo = int(v)
        if lo >= S - 1:
            return ((S - 1, 1.0), (S - 1, 0.0))
        return ((lo, 1.0 - (v - lo)), (lo + 1, v - lo))

    for k, (n, x1, y1, x2, y2) in enumerate(boxes.tolist()):
        n = int(n)
        x1, y1, x2, y2 = x1 * scale, y1 * scale, x2 * scale, y2 * scale
        rw, rh = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
        bh, bw = rh / PH, rw / PW
        gh, gw = int(math.ceil(rh / PH)), int(math.ceil(rw / PW))
        for ph in range(PH):
            for pw in range(PW):
                for iy in range(gh):
                    ty = taps(y1 + ph * bh + (iy + 0.5) * bh / gh, H)
                    for ix in range(gw):
                        tx = taps(x1 + pw * bw + (ix + 0.5) * bw / gw, W)
                        if ty is None or tx is None:
                            continue
                        for (yy, wy) in ty:
                            for (xx, wx) in tx:
                                w = wy * wx / (gh * gw)
                                out[k, :, ph, pw] += w * feat[n, :, yy, xx]
                                gfeat[n, :, yy, xx] += w * gout[k, :, ph, pw]
    return torch.from_numpy(out), torch.from_numpy(gfeat)


@pytest.mark.parametrize("name", ["C1-bins7-K19", "C1-bins3x5-K19", "C1-bins1-K19", "row1x9-bins7", "col9x1-bins3x5"])
def test_roi_ref_agrees_with_an_unpruned_sample_loop(name):
    case = next(c for c in R.ROI_CASES if c.name == name)
    feat, gout = case.tensors()
    out, gfeat = R.roi_ref(feat, case.boxes, case.bins, R.ROI_SCALE, gout)
    lout, lgfeat = _roi_loop(feat, case.boxes, case.bins2, R.ROI_SCALE, gout)
    for what, a, b in (("out", out, lout), ("d feat", gfeat, lgfeat)):
        err = (a - b).abs().max().item() / b.abs().max().item()
        print(f"{name} {what}: {err:.2e}")
        assert err <= 1e-12, what
    if case.N == 3:
        assert not gfeat[2].any()
        outside = [k for k, b in enumerate(R.ROI_BOXES) if b[1] > 60 or b[3] < -4]
        assert len(outside) == 2 and not out[outside].any()


def test_pool_inputs_hold_the_planted_ties():
    for shape in R.POOL_SHAPES:
        x, gout = R.pool_inputs(shape)
        assert x.dtype == gout.dtype == torch.bfloat16 and x.shape == shape
        w = x[0, 0, 0:2, 0:2].float()
        assert (w == w[0, 0]).all() and (shape[2] % 2 or shape[3] % 2)          # four equal; an odd extent: the general kernel
