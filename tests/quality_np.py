"""The per-frame quality sums of ops.frame_quality restated in float64 numpy, from their definition, not from
the kernel: squared error over every pixel, and Wang et al.'s SSIM with an 11-tap Gaussian window (sigma 1.5) at every centre
whose window lies inside the frame, as skimage.metrics.structural_similarity(gaussian_weights=True,
use_sample_covariance=False, data_range=L) evaluates it, per channel and then the mean over channels."""
import numpy as np

R, SIGMA = 5, 1.5


def taps():
    i = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def window_mean(a, w=None):
    """[..., H, W] -> [..., H - 10, W - 10]: the Gaussian-weighted mean of every 11x11 window inside the frame (rows first)."""
    w = taps() if w is None else w
    a = np.asarray(a, np.float64)
    Wv = a.shape[-1] - 2 * R
    Hv = a.shape[-2] - 2 * R
    h = sum(w[k] * a[..., :, k:k + Wv] for k in range(2 * R + 1))
    return sum(w[k] * h[..., k:k + Hv, :] for k in range(2 * R + 1))


def ssim_map(x, y, L):
    """x, y [..., H, W] float64 -> the SSIM of every valid centre, [..., H - 10, W - 10]."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    ux, uy = window_mean(x), window_mean(y)
    vx = window_mean(x * x) - ux * ux
    vy = window_mean(y * y) - uy * uy
    vxy = window_mean(x * y) - ux * uy
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def canonical(a):
    """An operand of either form as float64 [B,T,C,H,W] and its data range: uint8 [B,T,H,W,C] keeps its integer levels."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.float64).transpose(0, 1, 4, 2, 3), 255.0
    return a.astype(np.float64).transpose(0, 2, 1, 3, 4), 1.0


def frame_quality_sums(pred, target, regions=None):
    """-> float64 [B,T,9,4]: (n_pixels, sse, n_windows, ssim_sum) of the whole frame and of region bits 0..7."""
    x, L = canonical(pred)
    y, Ly = canonical(target)
    assert L == Ly and x.shape == y.shape
    B, T, C, H, W = x.shape
    out = np.zeros((B, T, 9, 4), np.float64)
    se = ((x - y) ** 2).sum(2)                                   # [B,T,H,W]
    s = ssim_map(x, y, L).mean(2)                                # [B,T,H-10,W-10]
    for k in range(9):
        if k == 0:
            m = np.ones((B, T, H, W), bool)
        elif regions is None:
            continue
        else:
            m = ((np.asarray(regions) >> (k - 1)) & 1).astype(bool)
        mc = m[:, :, R:H - R, R:W - R]
        out[:, :, k, 0] = m.sum((2, 3))
        out[:, :, k, 1] = np.where(m, se, 0.0).sum((2, 3))
        out[:, :, k, 2] = mc.sum((2, 3))
        out[:, :, k, 3] = np.where(mc, s, 0.0).sum((2, 3))
    return out
