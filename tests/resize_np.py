"""NumPy restatements of the three resize operations (csrc/resize.hip), written from the public definitions: Pillow's 8-bit
resampler (src/libImaging/Resample.c) and NEAREST scaling (Geometry.c ImagingScaleAffine), and torch's bilinear interpolation
of tensors with and without antialiasing.  Shared by test_resize_cpu.py (which pins them to live Pillow / a Pillow capture /
F.interpolate, without a GPU) and test_gpu_resize.py."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# (Hin, Win) -> (Hout, Wout): down, non-integer ratio, up, one axis unchanged, and 8x (33-tap windows)
SHAPES = [((37, 53), (16, 24)), ((64, 96), (47, 88)), ((40, 60), (64, 100)), ((33, 41), (33, 20)), ((128, 256), (16, 32))]


def bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def bicubic_filter(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"bilinear": (bilinear_filter, 1.0), "bicubic": (bicubic_filter, 2.0)}


def precompute_coeffs(n_in, n_out, name):
    """Per output: (first, [normalised float64 coefficients]).  Python floats are C doubles; int() truncates like (int)."""
    filt, support = FILTERS[name]
    scale = filterscale = float(n_in) / n_out
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ss = 1.0 / filterscale
    table = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        table.append((xmin, k))
    return table


def coeffs_8bpc(table):
    scale = 1 << PRECISION_BITS
    return [(first, [int(-0.5 + w * scale) if w < 0 else int(0.5 + w * scale) for w in k]) for first, k in table]


def _pass_8bpc(img, table, axis):
    """One resampling pass along `axis` of an int64 array holding uint8 values."""
    img = np.moveaxis(img, axis, 0)
    out = np.empty((len(table),) + img.shape[1:], np.int64)
    for i, (first, k) in enumerate(table):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t, kk in enumerate(k):
            acc += img[first + t] * kk
        assert np.abs(acc).max() < 2 ** 31, "Pillow accumulates in int"
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def np_resize_u8(img, size, name="bicubic"):
    """[..., H, W, C] uint8 -> [..., h, w, C]: Image.resize((w, h), BICUBIC / BILINEAR) per image; horizontal pass first,
    rounded and clipped to uint8, then the vertical pass."""
    h, w = size
    H, W = img.shape[-3:-1]
    x = _pass_8bpc(img.astype(np.int64), coeffs_8bpc(precompute_coeffs(W, w, name)), img.ndim - 2)
    x = _pass_8bpc(x, coeffs_8bpc(precompute_coeffs(H, h, name)), img.ndim - 3)
    return x.astype(np.uint8)


def nearest_index(n_in, n_out):
    """ImagingScaleAffine's index table: a running double sum; outputs whose source is outside the image stay unwritten (-1)."""
    a = float(n_in) / n_out
    xo = a * 0.5
    idx = []
    for _ in range(n_out):
        xin = -1 if xo < 0.0 else int(xo)
        idx.append(xin if 0 <= xin < n_in else -1)
        xo += a
    return np.asarray(idx, np.int64)


def np_resize_nearest(x, size):
    """[..., H, W] -> [..., h, w]: Image.resize((w, h), NEAREST)."""
    yi, xi = nearest_index(x.shape[-2], size[0]), nearest_index(x.shape[-1], size[1])
    out = x[..., np.maximum(yi, 0)[:, None], np.maximum(xi, 0)[None, :]]
    out = np.where((yi < 0)[:, None] | (xi < 0)[None, :], np.zeros((), x.dtype), out)
    return np.ascontiguousarray(out.astype(x.dtype))


def flow_taps(n_in, n_out, antialias):
    """Per output: (first, [float64 weights]) of the triangle filter torch applies to a tensor (align_corners=False)."""
    scale = float(n_in) / n_out
    if antialias:
        return precompute_coeffs(n_in, n_out, "bilinear")        # the same window and normalisation as Pillow's
    table = []
    for i in range(n_out):
        src = max(scale * (i + 0.5) - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        lam = src - i0
        table.append((i0, [1.0 - lam, lam]) if i0 + 1 <= n_in - 1 else (i0, [1.0]))
    return table


def flow_max_taps(shape, size, antialias):
    """The longest dot product of the two passes (for the fp32 rounding bound)."""
    return max(len(k) for n_in, n_out in zip(shape, size) for _, k in flow_taps(n_in, n_out, antialias))


def np_resize_flow(flow, size, antialias=False):
    """[..., H, W, 2] -> [..., h, w, 2] in float64, times h / H on both channels (cityscapes.py:222)."""
    flow = np.asarray(flow, np.float64)
    H, W = flow.shape[-3:-1]

    def run(x, table, axis):
        x = np.moveaxis(x, axis, 0)
        out = np.stack([sum(x[first + t] * w for t, w in enumerate(k)) for first, k in table], 0)
        return np.moveaxis(out, 0, axis)

    x = run(flow, flow_taps(W, size[1], antialias), flow.ndim - 2)
    x = run(x, flow_taps(H, size[0], antialias), flow.ndim - 3)
    return x * size[0] / H


def patterns(rng, shape):
    """The uint8 inputs of the resampler tests: noise, all-255, a 0/255 checkerboard and a step edge (ringing on both clip
    sides).  shape = (N, H, W, C) -> dict of arrays."""
    N, H, W, C = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    board = (((yy + xx) % 2) * 255).astype(np.uint8)
    step = np.where(xx + yy // 3 < W // 2, 0, 255).astype(np.uint8)
    tile = lambda p: np.ascontiguousarray(np.broadcast_to(p[None, :, :, None], shape))
    return {"noise": rng.integers(0, 256, shape, dtype=np.uint8), "white": np.full(shape, 255, np.uint8),
            "checker": tile(board), "step": tile(step)}
