"""Pins the NumPy restatements of tests/resize_np.py (the reference of test_gpu_resize.py) to the libraries that define the
results: Pillow (live where importable, and a committed capture, tools/capture_resize_golden.py) and torch's F.interpolate on
the CPU; and the host tables of c2m_amd.ops to the restatement.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_np as R
from c2m_amd import _lib, build, ops
from golden_io import GOLDEN

BIG = [((1024, 2048), (128, 256)), ((1024, 2048), (188, 352))]


def test_restatement_equals_pillow_capture():
    z = np.load(os.path.join(GOLDEN, "resize_pil.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    assert len(meta["cases"]) >= 8
    for i, case in enumerate(meta["cases"]):
        x, want, size = z[f"in{i}"], z[f"out{i}"], tuple(case["size"])
        if case["filter"] == "nearest":
            got = R.np_resize_nearest(x, size)
        else:
            got = R.np_resize_u8(x.reshape(x.shape[:2] + (-1,)), size, case["filter"]).reshape(want.shape)
        assert got.dtype == want.dtype and np.array_equal(got, want), case


@pytest.mark.parametrize("shape_in,size", R.SHAPES + BIG)
def test_restatement_equals_live_pillow(shape_in, size):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    h, w = size
    for mode, C in (("RGB", 3), ("L", 1)):
        pats = R.patterns(rng, (1,) + shape_in + (C,))
        for name in ("noise", "step") if shape_in[0] > 200 else pats:
            img = pats[name][0]
            pil = Image.fromarray(img if C == 3 else img[..., 0], mode=mode)
            for filt, code in (("bicubic", Image.BICUBIC), ("bilinear", Image.BILINEAR)):
                want = np.asarray(pil.resize((w, h), code)).reshape(h, w, C)
                assert np.array_equal(R.np_resize_u8(img, size, filt), want), (mode, name, filt)
            assert np.array_equal(R.np_resize_nearest(img[..., 0], size), np.asarray(pil.getchannel(0).resize((w, h), Image.NEAREST)))
    ids = rng.integers(0, 40001, shape_in).astype(np.int32)
    want = np.asarray(Image.fromarray(ids, mode="I").resize((w, h), Image.NEAREST))
    assert np.array_equal(R.np_resize_nearest(ids, size), want)


def test_step_edge_clips_on_both_sides():
    """The step-edge pattern overshoots below 0 and above 255 before the clip: both sides of clip8 are exercised."""
    (H, W), size = R.SHAPES[0]
    img = R.patterns(np.random.default_rng(0), (1, H, W, 1))["step"][0, :, :, 0].astype(np.int64)
    row = R.coeffs_8bpc(R.precompute_coeffs(W, size[1], "bicubic"))
    acc = np.array([[(1 << 21) + sum(int(img[y, f + t]) * k for t, k in enumerate(ks)) for f, ks in row] for y in range(H)])
    assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255


def _affine(H, W, a, b, c):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return a * xx + b * yy + c


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("shape_in,size", R.SHAPES + [((75, 150), (37, 70)), ((1024, 2048), (128, 416))])
def test_flow_restatement_equals_interpolate_on_affine_fields(shape_in, size, antialias):
    """Triangle filters reproduce affine fields away from the border, so a wrong centre or support convention shows as an
    offset of a pixel fraction times the slope, far above the tolerance: torch computes source coordinates and weights in
    fp32 (error <= |slope| * extent * 2^-22 per axis), and both sides round two fp32 dot products
    (8 * n_taps * 2^-24 * max|v|, as in test_gpu_resize.py)."""
    H, W = shape_in
    a, b = (0.25, -0.125), (-0.0625, 0.5)
    field = np.stack([_affine(H, W, a[0], b[0], 3.0), _affine(H, W, a[1], b[1], -7.0)], -1).astype(np.float32)   # exact in fp32
    got = R.np_resize_flow(field, size, antialias)
    t = torch.from_numpy(field).permute(2, 0, 1)[None]
    want = F.interpolate(t, size=size, mode="bilinear", align_corners=False, antialias=antialias)[0].permute(1, 2, 0)
    want = want.double().numpy() * size[0] / H
    vmax = float(np.abs(field).max())
    tol = (max(abs(a[0]), abs(a[1])) * W + max(abs(b[0]), abs(b[1])) * H) * 2.0 ** -22 \
        + 8 * R.flow_max_taps(shape_in, size, antialias) * 2.0 ** -24 * vmax
    tol *= max(size[0] / H, 1.0)                                  # both sides carry the h / H factor
    err = float(np.abs(got - want).max())
    print(f"{shape_in}->{size} antialias={antialias}: max |restatement - interpolate| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    # the interior equals the affine field at the output's source coordinate, times h / H (a wrong centre shows here).  The
    # widened filter is sampled symmetrically about that coordinate only at whole-number ratios.
    sy, sx = H / size[0], W / size[1]
    m = int(np.ceil(2 * max(sy, sx, 1.0)))
    if size[0] > 2 * m and size[1] > 2 * m and (not antialias or (H % size[0] == 0 and W % size[1] == 0)):
        yo, xo = np.meshgrid((np.arange(size[0]) + 0.5) * sy - 0.5, (np.arange(size[1]) + 0.5) * sx - 0.5, indexing="ij")
        exact = np.stack([a[0] * xo + b[0] * yo + 3.0, a[1] * xo + b[1] * yo - 7.0], -1) * size[0] / H
        inner = (slice(m, size[0] - m), slice(m, size[1] - m))
        assert np.abs(got[inner] - exact[inner]).max() <= 1e-9 * vmax


def test_host_tables_equal_the_restatement():
    for (H, W), (h, w) in R.SHAPES + BIG:
        for n_in, n_out in ((H, h), (W, w)):
            for filt in ("bicubic", "bilinear"):
                (bounds, coef), _, ks = ops.resize_table(filt, n_in, n_out, "cpu")
                assert coef.shape == (n_out, ks) and bounds.dtype == coef.dtype == np.int32
                for i, (first, k) in enumerate(R.coeffs_8bpc(R.precompute_coeffs(n_in, n_out, filt))):
                    assert (bounds[i, 0], bounds[i, 1]) == (first, len(k)) and list(coef[i, :len(k)]) == k
                    assert not coef[i, len(k):].any()
            (idx,), _, _ = ops.resize_table("nearest", n_in, n_out, "cpu")
            assert np.array_equal(idx, R.nearest_index(n_in, n_out))
            for antialias in (False, True):
                (bounds, wt), _, ks = ops.resize_table("flow_aa" if antialias else "flow", n_in, n_out, "cpu")
                assert wt.dtype == np.float32
                for i, (first, k) in enumerate(R.flow_taps(n_in, n_out, antialias)):
                    assert (bounds[i, 0], bounds[i, 1]) == (first, len(k)) and np.array_equal(wt[i, :len(k)], np.float32(k))
    assert ops.resize_table("bicubic", 2048, 256, "cpu")[2] == 33        # 8x reduction: 33-tap windows
    assert ops.resize_table("bicubic", 2048, 256, "cpu") is ops.resize_table("bicubic", 2048, 256, "cpu"), "cached"


def test_entry_points_declared_and_built_like_data_prep():
    for name in ("c2m_resize_u8", "c2m_resize_nearest", "c2m_resize_flow"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
    assert build.SOURCES["resize.hip"] == build.SOURCES["data_prep.hip"]
    assert _lib.ABI_VERSION == 6
