"""Frame quality on the GPU (run with -m gpu): ops.frame_quality against the float64 restatement of tests/quality_np.py on the
same (rounded) inputs, then c2m_amd.evaluate on a prediction of the small model of test_gpu_click_to_move.py.

The kernel's tile is TH x TW = 16 x 32 pixels (pinned below through the workspace size); the shapes put H and W one below, at
and one above a tile edge and one above two tiles.

Bounds, none of them taken from the kernel's output.  n_pixels and n_windows: equal.  uint8 sse: equal (integers below 2^53).
Float sse: 1e-12 relative (only the squares and the sum round).  ssim_sum / n_windows: 1e-9 absolute -- both sides are fp64 and
differ in summation order only: a moment is off by at most about 121 * 2^-53 of the value range, the variance factor by at most
about 6e-11 relative against C2 = 9e-4, the luminance factor by about 1e-12, so one centre's SSIM is within about 1e-10.  No
pixel and no case is exempt.  Each comparison prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import quality_np as Q
from c2m_amd import _lib, data, evaluate, fullres, ops
from c2m_amd import interactive as I
from test_gpu_click_to_move import DRAGS, T_OUT, inputs, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = 16, 32
SSE_REL, SSIM_ABS = 1e-12, 1e-9
# (form, C, B, T, H, W).  One window; one extra column / row; every tile edge in each axis (with the other axis at another
# edge); W odd with C = 3 uint8 (rows that are not dword-aligned); both channel counts; both (B, T); bf16.
CASES = [("f32", 3, 1, 1, 11, 11), ("f32", 1, 1, 1, 11, 12), ("f32", 3, 1, 1, 12, 11), ("u8", 3, 1, 1, 11, 11),
         ("f32", 1, 2, 3, 15, 33), ("f32", 3, 2, 3, 16, 32), ("f32", 3, 1, 1, 17, 31), ("f32", 1, 1, 1, 33, 65),
         ("f32", 3, 1, 1, 15, 65), ("f32", 1, 2, 3, 33, 31),
         ("u8", 3, 2, 3, 17, 33), ("u8", 3, 1, 1, 33, 65), ("u8", 3, 1, 1, 16, 31), ("u8", 1, 2, 3, 15, 33), ("u8", 1, 1, 1, 32, 64),
         ("bf16", 3, 2, 3, 17, 33), ("bf16", 1, 1, 1, 16, 65),
         # more tiles than the reduce kernel has slices (16): 2 x 9 = 18 tiles, slices 0 and 1 add two; 3 x 12 = 36, slices 0..3 three
         ("f32", 1, 1, 1, 17, 257), ("u8", 3, 1, 1, 33, 353)]
_cases = {}


def operands(form, C, B, T, H, W, seed, noise=0.08):
    """pred, target (torch, host, in the form's own dtype and layout) and random region bytes (bit 6 never set, bit 7 always)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.4 * np.sin(xx / 3.0 + rng.uniform(0, 6, (B, C, T, 1, 1))) * np.cos(yy / 4.0 + rng.uniform(0, 6, (B, C, T, 1, 1)))
    x = np.clip(base + rng.normal(0, 0.03, base.shape), 0, 1)
    x[..., :H // 2, :W // 3] = 0.97 + 0.02 * rng.random(x[..., :H // 2, :W // 3].shape)       # bright and nearly flat
    y = np.clip(x + rng.normal(0, noise, x.shape), 0, 1)
    reg = (rng.integers(0, 64, (B, T, H, W)) | 128).astype(np.uint8)
    if form == "u8":
        cv = lambda a: torch.from_numpy(np.floor(a * 255 + 0.5).astype(np.uint8).transpose(0, 2, 3, 4, 1).copy())
    elif form == "bf16":
        cv = lambda a: torch.from_numpy(a).to(torch.bfloat16)
    else:
        cv = lambda a: torch.from_numpy(a.astype(np.float32))
    return cv(x), cv(y), torch.from_numpy(reg)


def host(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def case(i):
    """Inputs and float64 reference of CASES[i], computed once and never modified."""
    if i not in _cases:
        x, y, reg = operands(*CASES[i], seed=300 + i)
        _cases[i] = dict(x=x, y=y, reg=reg, ref=Q.frame_quality_sums(host(x), host(y), reg.numpy()))
    return _cases[i]


def compare(got, ref, exact_sse, what):
    """got, ref [B,T,9,4] float64: the module's bounds."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    d_sse = np.abs(got[..., 1] - ref[..., 1])
    rel = float((d_sse / np.maximum(ref[..., 1], 1e-300)).max())
    nw = np.maximum(ref[..., 2], 1)
    d_ssim = float(np.abs(got[..., 3] / nw - ref[..., 3] / nw).max())
    print(f"{what}: sse max abs diff {d_sse.max():.3e} rel {rel:.3e}; ssim mean max abs diff {d_ssim:.3e}")
    assert np.array_equal(got[..., 0], ref[..., 0]), f"{what}: n_pixels"
    assert np.array_equal(got[..., 2], ref[..., 2]), f"{what}: n_windows"
    if exact_sse:
        assert np.array_equal(got[..., 1], ref[..., 1]), f"{what}: uint8 sse"
    else:
        assert (d_sse <= SSE_REL * ref[..., 1]).all(), f"{what}: sse rel {rel:.3e}"
    assert d_ssim <= SSIM_ABS, f"{what}: ssim {d_ssim:.3e}"


def test_tile_is_the_one_the_shapes_were_chosen_for():
    for H, W in ((16, 32), (17, 33), (1024, 2048)):
        want = 2 * 3 * -(-H // TH) * -(-W // TW) * 36 * 8
        assert _lib.lib().c2m_frame_quality_workspace_bytes(2, 3, H, W) == want


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "-".join(str(v) for v in CASES[i]))
def test_sums_vs_float64(i):
    c = case(i)
    got = ops.frame_quality(c["x"].to(DEV), c["y"].to(DEV), c["reg"].to(DEV))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == tuple(c["ref"].shape)
    compare(got.cpu().numpy(), c["ref"], CASES[i][0] == "u8", str(CASES[i]))
    none = ops.frame_quality(c["x"].to(DEV), c["y"].to(DEV))
    assert torch.equal(none[:, :, 0], got[:, :, 0]) and not none[:, :, 1:].any()
    assert torch.equal(got[:, :, 8], got[:, :, 0]) and not got[:, :, 7].any()     # bit 7 everywhere, bit 6 nowhere


def test_fp32_against_bf16_is_scored_in_fp32():
    c = case(15)
    got = ops.frame_quality(c["x"].to(DEV), c["y"].to(DEV).float(), c["reg"].to(DEV))
    assert torch.equal(got, ops.frame_quality(c["x"].to(DEV), c["y"].to(DEV), c["reg"].to(DEV)))


@pytest.mark.parametrize("i", [5, 10], ids=["f32", "u8"])
def test_strided_views_go_in_without_a_copy(i, monkeypatch):
    """B- and T-strided slices of larger tensors: the same bits as the dense operands, and no .contiguous() on the way."""
    form, C, B, T, H, W = CASES[i]
    c = case(i)
    x, y, reg = c["x"].to(DEV), c["y"].to(DEV), c["reg"].to(DEV)
    want = ops.frame_quality(x, y, reg)
    tdim = 1 if form == "u8" else 2
    shape = list(x.shape)
    shape[0], shape[tdim] = 2 * B + 1, T + 3
    bx = torch.full(shape, 77, dtype=x.dtype, device=DEV)
    by = torch.full(shape, 55, dtype=x.dtype, device=DEV)
    vx, vy = bx[1::2].narrow(tdim, 2, T), by[:2 * B:2].narrow(tdim, 3, T)
    vx.copy_(x)
    vy.copy_(y)
    assert not vx.is_contiguous() and not vy.is_contiguous()
    copies = []
    orig = torch.Tensor.contiguous
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda self, *a, **k: (copies.append(self.shape), orig(self, *a, **k))[1])
    got = ops.frame_quality(vx, vy, reg)
    monkeypatch.undo()
    assert not copies and torch.equal(got, want)
    wshape = list(x.shape)                                             # rows that are not dense: the wrapper copies
    wshape[-2 if form == "u8" else -1] += 3
    wide = torch.zeros(wshape, dtype=x.dtype, device=DEV)
    wv = wide.narrow(-2 if form == "u8" else -1, 0, W)
    wv.copy_(x)
    assert torch.equal(ops.frame_quality(wv, y, reg), want)
    compare(got.cpu().numpy(), c["ref"], form == "u8", f"strided {CASES[i]}")


def test_regions_never_everywhere_and_border_only():
    form, C, B, T, H, W = "f32", 3, 2, 3, 17, 33
    x, y, _ = operands(form, C, B, T, H, W, seed=7)
    reg = np.zeros((B, T, H, W), np.uint8)
    reg |= 2                                                     # bit 1 everywhere; bit 0 never
    border = np.ones((H, W), bool)
    border[5:H - 5, 5:W - 5] = False
    reg[:, :, border] |= 4                                       # bit 2: the 5-pixel border only
    rng = np.random.default_rng(8)
    reg |= (rng.integers(0, 2, reg.shape) * 8).astype(np.uint8)  # bit 3: random
    ref = Q.frame_quality_sums(host(x), host(y), reg)
    r = evaluate.frame_quality(x.to(DEV), y.to(DEV), torch.from_numpy(reg).to(DEV), evaluate.QUALITY_REGIONS)
    w = evaluate.quality_from_sums(ref, C, 1.0, evaluate.QUALITY_REGIONS)
    assert all(not v.is_cuda and v.dtype == torch.float64 for v in r.values()) and r["region_mse"].shape == (B, T, 4)
    for k in ("region_mse", "region_psnr", "region_ssim"):
        assert torch.isnan(r[k][..., 0]).all(), k                                       # never set
    assert not r["region_pixels"][..., 0].any()
    for k in ("mse", "psnr", "ssim"):
        assert torch.equal(r["region_" + k][..., 1], r[k]), k                           # everywhere: the whole-frame row
    assert (r["region_pixels"][..., 1] == H * W).all()
    assert torch.isfinite(r["region_psnr"][..., 2]).all() and torch.isnan(r["region_ssim"][..., 2]).all()      # border
    assert (r["region_pixels"][..., 2] == H * W - (H - 10) * (W - 10)).all()
    for k in r:
        a, b = r[k].numpy(), w[k].numpy()
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        d = float(np.nanmax(np.abs(a - b), initial=0.0))
        print(f"{k}: max abs diff {d:.3e}")
        assert d <= {"ssim": SSIM_ABS, "region_ssim": SSIM_ABS, "region_pixels": 0}.get(k, 1e-9), k
        # mse: 1e-12 relative of values <= 1; psnr = 10 log10: 4.35 * 1e-12 relative -- both far inside 1e-9


def test_identical_operands_repeat_and_streams():
    c = case(5)
    x, y, reg = c["x"].to(DEV), c["y"].to(DEV), c["reg"].to(DEV)
    same = evaluate.frame_quality(x, x.clone(), reg)
    assert torch.isinf(same["psnr"]).all() and (same["psnr"] > 0).all() and (same["ssim"] - 1).abs().max() <= 1e-12
    assert not same["mse"].any()
    ok = same["region_pixels"] > 0
    assert torch.isinf(same["region_psnr"][ok]).all() and torch.isnan(same["region_psnr"][~ok]).all()
    a, b = ops.frame_quality(x, y, reg), ops.frame_quality(x, y, reg)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):
        big = big @ big * 1e-3                                    # the default stream is busy
    with torch.cuda.stream(side):
        s = ops.frame_quality(x, y, reg)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(s, a)


def test_uint8_and_float_forms_agree():
    c = case(10)
    xu, yu, reg = c["x"].to(DEV), c["y"].to(DEV), c["reg"].to(DEV)
    xf, yf = ((t.float() / 255).permute(0, 4, 1, 2, 3).contiguous() for t in (xu, yu))      # fp32 n / 255: rounded
    ru, rf = evaluate.frame_quality(xu, yu, reg), evaluate.frame_quality(xf, yf, reg)
    # The float frames are fp32 roundings of n / 255, each off by eps <= 6e-8 of its value (<= 1), so the two forms score
    # slightly different inputs.  x - y moves by at most 1.2e-7, the mse by at most 2 * 1.2e-7 / rms(x - y) relative: below 1e-5
    # for the rms of 0.05 or more that these frames have; psnr = -10 log10(mse) by 4.35 times that.  A variance moves by at most
    # 2 sigma eps against a denominator of 2 sigma^2 + C2, at most eps / sqrt(2 C2) = 1.5e-6 relative per factor: 1e-5 covers
    # numerator, denominator and the luminance factor.
    for k, tol, relative in (("mse", 1e-5, True), ("psnr", 4.35e-5, False), ("ssim", 1e-5, False),
                             ("region_mse", 1e-5, True), ("region_psnr", 4.35e-5, False), ("region_ssim", 1e-5, False)):
        a, b = ru[k].numpy(), rf[k].numpy()
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        d = float(np.nanmax(np.abs(a - b) / (np.maximum(np.abs(b), 1e-30) if relative else 1.0), initial=0.0))
        print(f"{k}: max {'rel' if relative else 'abs'} diff {d:.3e}")
        assert d <= tol, k
    assert float(np.sqrt(rf["mse"].numpy().min())) >= 0.05                          # what the mse bound assumed
    assert torch.equal(ru["region_pixels"], rf["region_pixels"])


def test_refusals_on_the_device():
    c = case(5)
    x, y, reg = c["x"].to(DEV), c["y"].to(DEV), c["reg"].to(DEV)
    with pytest.raises(ValueError):
        ops.frame_quality(x, y[..., :31])
    with pytest.raises(ValueError):
        ops.frame_quality(x, y, reg.int())
    with pytest.raises(ValueError):
        ops.frame_quality(x, case(10)["x"].to(DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        ops.frame_quality(x, y.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        ops.frame_quality(x, y, reg.cpu())
    empty = ops.frame_quality(x[:0], y[:0])
    assert tuple(empty.shape) == (0, 3, 9, 4)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def predicted():
    """A click-to-move prediction of the small model whose video comes from uint8 frames, so the ground truth has both forms."""
    B, t_in = 2, 1
    batch = inputs(B, t_in)
    frames = (batch["video"].permute(0, 2, 3, 4, 1) * 255).round().clamp(0, 255).to(torch.uint8).contiguous()
    video = data.prep_video(frames)
    model = small_model(t_in)
    z_m = torch.randn(B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(21)
    out = I.click_to_move(model, video[:, :, :t_in].contiguous(), batch["bg_mask"], batch["fg_mask"], batch["instance_mask"],
                          DRAGS, z_m=z_m)
    torch.cuda.synchronize()
    return dict(out=out, video=video, frames=frames, batch=batch, t_in=t_in)


def test_evaluate_on_a_prediction(predicted, tmp_path):
    out, video, batch, t_in = (predicted[k] for k in ("out", "video", "batch", "t_in"))
    gen, truth = out["generated"], video[:, :, t_in:]
    assert gen.shape == truth.shape == (2, 3, T_OUT, 128, 256) and not truth.is_contiguous()
    clicked = [[13001], [12005]]
    inst_t = batch["instance_mask"][:, :, t_in - 1:t_in].expand(-1, -1, T_OUT, -1, -1)      # the objects, as if they stood still
    reg = evaluate.quality_regions(batch["fg_mask"][:, :, t_in:], inst_t, clicked, out["occlusion_bw"])
    assert reg.is_cuda and reg.dtype == torch.uint8 and tuple(reg.shape) == (2, T_OUT, 128, 256)
    fg = (host(batch["fg_mask"][:, :, t_in:]) != 0).any(1)
    inst = host(inst_t[:, 0])
    guided = np.stack([np.isin(inst[b], clicked[b]) for b in range(2)])
    want_reg = fg + 2 * ~fg + 4 * guided + 8 * (host(out["occlusion_bw"][:, 0]) < 0.5)
    assert np.array_equal(reg.cpu().numpy(), want_reg.astype(np.uint8))
    got = evaluate.frame_quality(gen, truth, reg, evaluate.QUALITY_REGIONS)
    ref = Q.frame_quality_sums(host(gen), host(truth), want_reg.astype(np.uint8))
    compare(ops.frame_quality(gen, truth, reg).cpu().numpy(), ref, False, "generated vs video")
    want = evaluate.quality_from_sums(ref, 3, 1.0, evaluate.QUALITY_REGIONS)
    for k in want:
        a, b = got[k].numpy(), want[k].numpy()
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), k
        d = float(np.nanmax(np.abs(a - b), initial=0.0))
        print(f"{k}: max abs diff {d:.3e}")
        assert d <= 1e-9, k                       # ssim: the module's bound; mse, psnr: 1e-12 relative of values below 100
    # QualityScore over two updates: the means of the restatement's numbers
    half = lambda r, s: {k: v[s] for k, v in r.items()}
    score = evaluate.QualityScore()
    score.update(half(got, slice(0, 1)))
    score.update(half(got, slice(1, 2)))
    res = score.write(str(tmp_path / "quality.txt"))
    assert res["frames"] == 2 * T_OUT and res["psnr_identical"] == 0
    for k in ("mse", "psnr", "ssim"):
        w = want[k].numpy()
        assert abs(res[k] - w.mean()) <= 1e-9 and np.abs(np.array(res[k + "_per_frame"]) - w.mean(0)).max() <= 1e-9, k
        for j, name in enumerate(evaluate.QUALITY_REGIONS):
            wr = want["region_" + k].numpy()[..., j]
            if np.isfinite(wr).any():
                assert abs(res[f"{name}_{k}"] - wr[np.isfinite(wr)].mean()) <= 1e-9, (name, k)
            else:
                assert np.isnan(res[f"{name}_{k}"]), (name, k)
    assert np.isfinite(res["foreground_psnr"]) and np.isfinite(res["background_ssim"]) and np.isfinite(res["guided_ssim"])
    assert (tmp_path / "quality.txt").read_text().startswith(f"frames {2 * T_OUT}\n")


def test_evaluate_on_upscaled_uint8_frames(predicted):
    out, video, frames, t_in = (predicted[k] for k in ("out", "video", "frames", "t_in"))
    pred_u8, _ = fullres.upscale(out, video, frames[:, t_in - 1].contiguous(), t_in)
    truth_u8 = frames[:, t_in:]
    assert pred_u8.shape == truth_u8.shape == (2, T_OUT, 128, 256, 3) and not truth_u8.is_contiguous()
    got = ops.frame_quality(pred_u8, truth_u8)
    ref = Q.frame_quality_sums(pred_u8.cpu().numpy(), truth_u8.cpu().numpy())
    compare(got.cpu().numpy(), ref, True, "upscaled vs dataset frames")
    r = evaluate.frame_quality(pred_u8, truth_u8)
    w = evaluate.quality_from_sums(ref, 3, 255.0)
    assert torch.isfinite(r["psnr"]).all() and (r["ssim"] - w["ssim"]).abs().max() <= SSIM_ABS
    assert torch.equal(r["mse"], w["mse"]) and torch.equal(r["psnr"], w["psnr"])
