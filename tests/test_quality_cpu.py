"""Host side of the frame-quality metric (no GPU): the float64 restatement (quality_np) is checked against scipy's Gaussian
filter, a direct 121-tap sum and the properties its definition promises; ops._frame_quality_plan accepts the good cases and
refuses every bad one before a launch; the entry point is declared and bound; the host arithmetic of evaluate.frame_quality,
QualityScore and quality_regions is checked on hand-made inputs."""
import math

import numpy as np
import pytest
import torch

import quality_np as Q
from c2m_amd import _lib, evaluate, ops


def frames(B=2, C=3, T=2, H=19, W=23, seed=0, noise=0.1):
    """Two float operands [B,C,T,H,W] in [0,1]: smooth structure plus noise, the second a perturbed first."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.4 * np.sin(xx / 3.0 + rng.uniform(0, 6, (B, C, T, 1, 1))) * np.cos(yy / 4.0)
    x = np.clip(base + rng.normal(0, 0.05, base.shape), 0, 1)
    y = np.clip(x + rng.normal(0, noise, x.shape), 0, 1)
    return x, y


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_taps_are_the_ops_weights_and_sum_to_one():
    w = Q.taps()
    assert w.shape == (11,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    assert np.array_equal(ops.quality_weights(), w)


def test_moments_agree_with_scipy_gaussian_filter():
    import scipy.ndimage as ndi
    x, y = frames(1, 1, 1, 27, 31, seed=1)
    for a in (x[0, 0, 0], y[0, 0, 0], x[0, 0, 0] * y[0, 0, 0]):
        want = ndi.gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")[5:-5, 5:-5]
        assert np.abs(Q.window_mean(a) - want).max() <= 1e-12


def test_moments_agree_with_the_direct_121_tap_sum():
    x, _ = frames(1, 1, 1, 14, 17, seed=2)
    a = x[0, 0, 0]
    w2 = np.outer(Q.taps(), Q.taps())
    want = np.array([[(w2 * a[i:i + 11, j:j + 11]).sum() for j in range(17 - 10)] for i in range(14 - 10)])
    assert np.abs(Q.window_mean(a) - want).max() <= 1e-12


def test_identical_frames_score_one_and_infinite_psnr():
    x, _ = frames(seed=3)
    s = Q.frame_quality_sums(x, x)
    r = evaluate.quality_from_sums(s, 3, 1.0)
    assert np.abs(r["ssim"].numpy() - 1).max() <= 1e-12
    assert torch.isinf(r["psnr"]).all() and (r["psnr"] > 0).all() and not r["mse"].any()


def test_a_constant_offset_has_its_square_as_mse():
    x, _ = frames(seed=4)
    x = x * 0.5
    d = 0.125
    r = evaluate.quality_from_sums(Q.frame_quality_sums(x, x + d), 3, 1.0)
    assert np.abs(r["mse"].numpy() - d * d).max() <= 1e-15
    assert np.abs(r["psnr"].numpy() - 10 * math.log10(1 / (d * d))).max() <= 1e-12


def test_symmetric_in_its_operands():
    x, y = frames(seed=5)
    a, b = Q.frame_quality_sums(x, y), Q.frame_quality_sums(y, x)
    assert np.array_equal(a[..., :3], b[..., :3]) and np.abs(a[..., 3] - b[..., 3]).max() <= 1e-12 * a[..., 2].max()


def to_u8_form(x):
    return np.floor(x * 255 + 0.5).astype(np.uint8).transpose(0, 2, 3, 4, 1)            # [B,T,H,W,C]


def test_uint8_form_and_its_float_form_agree():
    x, y = frames(seed=6)
    xu, yu = to_u8_form(x), to_u8_form(y)
    xf, yf = (a.astype(np.float64).transpose(0, 4, 1, 2, 3) / 255 for a in (xu, yu))
    ru = evaluate.quality_from_sums(Q.frame_quality_sums(xu, yu), 3, 255.0)
    rf = evaluate.quality_from_sums(Q.frame_quality_sums(xf, yf), 3, 1.0)
    for k in ("mse", "ssim"):
        assert np.abs(ru[k].numpy() - rf[k].numpy()).max() <= 1e-12, k
    assert np.abs(ru["psnr"].numpy() - rf["psnr"].numpy()).max() <= 1e-10            # (10 log10 of 1e-12-close numbers)


def test_a_partition_adds_up_to_the_frame():
    x, y = frames(seed=7)
    rng = np.random.default_rng(7)
    fg = rng.integers(0, 2, (2, 2, 19, 23)).astype(np.uint8)
    s = Q.frame_quality_sums(x, y, fg + 2 * (1 - fg))
    assert np.array_equal(s[:, :, 1, (0, 2)] + s[:, :, 2, (0, 2)], s[:, :, 0, (0, 2)])
    assert np.abs(s[:, :, 1] + s[:, :, 2] - s[:, :, 0]).max() <= 1e-11
    assert not s[:, :, 3:].any() and s[0, 0, 0, 0] == 19 * 23 and s[0, 0, 0, 2] == 9 * 13


# ------------------------------------------------------------------------------------------------------------ the plan
def _f(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def test_plan_accepts_both_forms_and_strided_views():
    assert ops._frame_quality_plan(_f(2, 3, 4, 11, 12), _f(2, 3, 4, 11, 12), None) == ("float", 2, 3, 4, 11, 12)
    assert ops._frame_quality_plan(_f(2, 1, 4, 16, 11, dtype=torch.bfloat16), _f(2, 1, 4, 16, 11), None)[0] == "float"
    u = _f(2, 5, 13, 17, 3, dtype=torch.uint8)
    assert ops._frame_quality_plan(u, u, _f(2, 5, 13, 17, dtype=torch.uint8)) == ("uint8", 2, 3, 5, 13, 17)
    big_u, big_f = _f(4, 7, 13, 17, 3, dtype=torch.uint8), _f(4, 3, 7, 13, 17)
    assert ops._frame_quality_plan(big_u[::2, 2:], big_u[1::2, :5], None) == ("uint8", 2, 3, 5, 13, 17)
    assert ops._frame_quality_plan(big_f[::2, :, 2:], big_f[1::2, :, 2:], None) == ("float", 2, 3, 5, 13, 17)
    x, sx = ops._quality_operand(big_f[::2, :, 2:], "float", 13, 17, 3)
    assert x.data_ptr() == big_f[::2, :, 2:].data_ptr() and tuple(sx) == (2 * 3 * 7 * 221, 7 * 221, 221)    # no copy
    x, sx = ops._quality_operand(big_u[::2, 2:], "uint8", 13, 17, 3)
    assert x.data_ptr() == big_u[::2, 2:].data_ptr() and tuple(sx) == (2 * 7 * 663, 0, 663)
    x, sx = ops._quality_operand(big_f[..., ::2], "float", 13, 9, 3)                                            # a copy
    assert x.is_contiguous() and tuple(sx) == (3 * 7 * 117, 7 * 117, 117)


BAD = {
    "forms differ": lambda: (_f(1, 3, 2, 12, 12), _f(1, 2, 12, 12, 3, dtype=torch.uint8), None),
    "dtype family": lambda: (_f(1, 3, 2, 12, 12), _f(1, 3, 2, 12, 12, dtype=torch.float64), None),
    "integer family": lambda: (_f(1, 3, 2, 12, 12, dtype=torch.int32), _f(1, 3, 2, 12, 12, dtype=torch.int32), None),
    "shapes differ": lambda: (_f(1, 3, 2, 12, 12), _f(1, 3, 2, 12, 13), None),
    "not 5-d": lambda: (_f(3, 2, 12, 12), _f(3, 2, 12, 12), None),
    "float C=2": lambda: (_f(1, 2, 2, 12, 12), _f(1, 2, 2, 12, 12), None),
    "uint8 C=4": lambda: (_f(1, 2, 12, 12, 4, dtype=torch.uint8), _f(1, 2, 12, 12, 4, dtype=torch.uint8), None),
    "H < 11": lambda: (_f(1, 3, 2, 10, 12), _f(1, 3, 2, 10, 12), None),
    "W < 11": lambda: (_f(1, 2, 12, 10, 3, dtype=torch.uint8), _f(1, 2, 12, 10, 3, dtype=torch.uint8), None),
    "regions dtype": lambda: (_f(1, 3, 2, 12, 12), _f(1, 3, 2, 12, 12), _f(1, 2, 12, 12, dtype=torch.int32)),
    "regions shape": lambda: (_f(1, 3, 2, 12, 12), _f(1, 3, 2, 12, 12), _f(1, 3, 12, 12, dtype=torch.uint8)),
    "regions 5-d": lambda: (_f(1, 3, 2, 12, 12), _f(1, 3, 2, 12, 12), _f(1, 1, 2, 12, 12, dtype=torch.uint8)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_plan_refuses(case):
    with pytest.raises(ValueError):
        ops._frame_quality_plan(*BAD[case]())


def test_host_tensors_are_refused_on_the_launch_path():
    x = _f(1, 3, 2, 12, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        ops.frame_quality(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        evaluate.frame_quality(x, x)


def test_entry_point_is_declared_and_bound():
    for name in ("c2m_frame_quality", "c2m_frame_quality_workspace_bytes"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
    assert _lib.ABI_VERSION == 6
    assert "quality.hip" in __import__("c2m_amd.build", fromlist=["SOURCES"]).SOURCES


# ------------------------------------------------------------------------------------------------- the host arithmetic
def test_quality_from_sums_by_hand():
    s = torch.zeros(1, 2, 9, 4, dtype=torch.float64)
    s[0, 0, 0] = torch.tensor([100.0, 3.0, 10.0, 9.0])
    s[0, 1, 0] = torch.tensor([100.0, 0.0, 10.0, 10.0])
    s[0, 0, 1] = torch.tensor([20.0, 6.0, 0.0, 0.0])                # a region on the border: pixels, no window centre
    r = evaluate.quality_from_sums(s, 3, 1.0, evaluate.QUALITY_REGIONS)
    assert r["mse"].tolist() == [[0.01, 0.0]] and r["ssim"].tolist() == [[0.9, 1.0]]
    assert r["psnr"][0, 0].item() == pytest.approx(20.0, abs=1e-12) and r["psnr"][0, 1].item() == math.inf
    assert r["region_mse"].shape == (1, 2, 4) and r["region_pixels"][0, 0].tolist() == [20, 0, 0, 0]
    assert r["region_mse"][0, 0, 0].item() == 0.1 and r["region_psnr"][0, 0, 0].item() == pytest.approx(10.0, abs=1e-12)
    assert math.isnan(r["region_ssim"][0, 0, 0].item())
    for k in ("region_mse", "region_psnr", "region_ssim"):
        assert torch.isnan(r[k][0, :, 1:]).all() and torch.isnan(r[k][0, 1]).all()
    u = evaluate.quality_from_sums(s * torch.tensor([1.0, 255.0 ** 2, 1.0, 1.0]), 3, 255.0)
    assert u["region_mse"].shape == (1, 2, 8)
    assert torch.allclose(u["mse"], r["mse"], rtol=1e-15, atol=0) and torch.allclose(u["psnr"][0, :1], r["psnr"][0, :1], atol=1e-12)


def _result(mse, psnr, ssim, R=4):
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    nan = torch.full(t(mse).shape + (R,), math.nan, dtype=torch.float64)
    return {"mse": t(mse), "psnr": t(psnr), "ssim": t(ssim), "region_mse": nan.clone(), "region_psnr": nan.clone(),
            "region_ssim": nan.clone(), "region_pixels": torch.zeros_like(nan)}


def test_quality_score_arithmetic(tmp_path):
    a = _result([[0.01, 0.04]], [[20.0, 14.0]], [[0.9, 0.8]])
    b = _result([[0.03, 0.0], [0.05, 0.02]], [[15.0, math.inf], [13.0, 17.0]], [[0.7, 1.0], [0.5, 0.6]])
    a["region_psnr"][0, 0, 0], a["region_ssim"][0, 0, 0], a["region_mse"][0, 0, 0] = 30.0, 0.95, 0.001
    b["region_psnr"][1, 0, 0], b["region_ssim"][1, 0, 0], b["region_mse"][1, 0, 0] = 20.0, 0.85, 0.01
    b["region_psnr"][0, 1, 2] = math.inf
    q = evaluate.QualityScore()
    assert q.region_names == evaluate.QUALITY_REGIONS == ("foreground", "background", "guided", "disoccluded")
    q.update(a)
    q.update(b)
    r = q.result()
    assert r["frames"] == 6
    assert r["mse"] == pytest.approx(0.15 / 6, abs=1e-15) and r["ssim"] == pytest.approx(4.5 / 6, abs=1e-15)
    assert r["psnr"] == pytest.approx(79.0 / 5, abs=1e-12) and r["psnr_identical"] == 1            # inf counted, not averaged
    assert r["psnr_per_frame"] == pytest.approx([48.0 / 3, 31.0 / 2], abs=1e-12)
    assert r["ssim_per_frame"] == pytest.approx([2.1 / 3, 2.4 / 3], abs=1e-15)
    assert r["mse_per_frame"] == pytest.approx([0.03, 0.02], abs=1e-15)
    assert r["foreground_psnr"] == pytest.approx(25.0) and r["foreground_ssim"] == pytest.approx(0.9)      # NaN skipped
    assert r["foreground_mse"] == pytest.approx(0.0055)
    assert r["foreground_psnr_per_frame"][0] == pytest.approx(25.0) and math.isnan(r["foreground_psnr_per_frame"][1])
    assert math.isnan(r["background_psnr"]) and r["background_psnr_identical"] == 0
    assert r["guided_psnr_identical"] == 1 and math.isnan(r["guided_psnr"])
    path = tmp_path / "metrics.txt"
    assert q.write(str(path))["frames"] == 6
    lines = path.read_text().splitlines()
    assert lines[0] == "frames 6"
    assert f"psnr {r['psnr']} psnr_identical 1" in lines and f"ssim {r['ssim']}" in lines and f"mse {r['mse']}" in lines
    assert f"foreground_ssim {r['foreground_ssim']}" in lines and "guided_psnr nan guided_psnr_identical 1" in lines
    assert "psnr_per_frame " + " ".join(str(v) for v in r["psnr_per_frame"]) in lines
    q.write(str(path))                                                                              # appends
    assert path.read_text().splitlines().count("frames 6") == 2
    with pytest.raises(ValueError):
        q.update(_result([[0.1]], [[10.0]], [[0.5]]))                                               # another T
    two = evaluate.QualityScore(region_names=("foreground", "background"))
    two.update(a)
    assert "guided_psnr" not in two.result() and two.result()["foreground_psnr"] == 30.0


def test_quality_regions_on_small_tensors():
    B, T, H, W = 2, 2, 4, 5
    fg = torch.zeros(B, 9, T, H, W)
    fg[0, 3, 0, 1, 2] = 1
    fg[1, 8, 1, :, 0] = 1
    inst = torch.zeros(B, 1, T, H, W, dtype=torch.int32)
    inst[0, 0, 0, 1, 2], inst[0, 0, 1, 0, 0], inst[1, 0, 1, 3, 0], inst[1, 0, 0, 2, 2] = 13001, 13001, 17002, 13001
    occ = torch.ones(B, 1, T, H, W)
    occ[0, 0, 1, 3, 4], occ[1, 0, 0, 0, 0] = 0.25, 0.5
    r = evaluate.quality_regions(fg, inst, [[13001], [17002, 5]], occ)
    assert r.dtype == torch.uint8 and r.shape == (B, T, H, W) and r.is_contiguous()
    want = torch.full((B, T, H, W), 2, dtype=torch.uint8)
    want[0, 0, 1, 2] = 1 + 4
    want[0, 1, 0, 0] = 2 + 4
    want[1, 1, :, 0] = 1
    want[1, 1, 3, 0] = 1 + 4
    want[0, 1, 3, 4] = 2 + 8                     # 13001 in sample 1 is not clicked there; occ == threshold is not below it
    assert torch.equal(r, want)
    assert torch.equal(evaluate.quality_regions(fg, inst[:, 0]), torch.where(want & 1 > 0, 1, 2).to(torch.uint8))
    assert torch.equal(evaluate.quality_regions(fg, inst, [[], []], occ, occ_threshold=0.6) & 8,
                       ((occ[:, 0] < 0.6) * 8).to(torch.uint8))
    with pytest.raises(ValueError):
        evaluate.quality_regions(fg, inst, [[1]])
    with pytest.raises(ValueError):
        evaluate.quality_regions(fg, inst, None, occ[:, :, :1])
    assert evaluate.QUALITY_REGIONS == ("foreground", "background", "guided", "disoccluded")
