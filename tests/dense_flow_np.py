"""NumPy restatement of the dense inverse search flow (csrc/dense_flow.hip), stage by stage and in the dtype asked
for (float64: the yardstick; float32: the kernels' own precision, with numpy's summation order), the synthetic scenes with a
known flow, and the inputs of the GPU tests (tests/test_gpu_dense_flow.py) with the tolerance that belongs to them.

The flow is that of a -> b in pixels, channel 0 = x: a(x) ~ b(x + flow(x))."""
import numpy as np

PATCH, STRIDE, MAX_LEVELS = 8, 4, 7
DET_MIN, MAX_STEP2 = 40.96, 64.0

# 16 x the largest difference between the float32 and the float64 run of this file over the GPU tests' own stage inputs: the
# records of patch_search on every level_pair of search_cases() (patches that excluded() names left out) and the dense flows of
# densify on the float64 records rounded to float32.  Measured: 1.563e-4 (a patch of the 21 x 37, N = 3 case with the corner
# and the large motion, 12 steps from an initial flow 3 px off); tests/test_dense_flow_cpu.py recomputes the gap and asserts
# gap <= TOL / 16.  The factor 16 covers the kernels' different, but fixed, summation order.
TOL = 16 * 1.6e-4


# ------------------------------------------------------------------------------------------------ the algorithm
def pyramid_sizes(H, W, levels=None):
    sizes = [(H, W)]
    cap = MAX_LEVELS if levels is None else min(levels, MAX_LEVELS)
    while len(sizes) < cap and min(sizes[-1]) // 2 >= 16:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def origins(n):
    o = list(range(0, n - PATCH + 1, STRIDE))
    return o if o[-1] == n - PATCH else o + [n - PATCH]


def gray(img, value_range=(0, 1), dtype=np.float64):
    """img [3,H,W] -> gray [H,W] on 0..255."""
    dt = np.dtype(dtype).type
    lo, hi = value_range
    x = (np.asarray(img).astype(dtype) - dt(lo)) * dt(255.0 / (float(hi) - float(lo)))
    coef = [dt(np.float32(c)) if dtype == np.float32 else dt(c) for c in (0.299, 0.587, 0.114)]
    return (coef[0] * x[0] + coef[1] * x[1]) + coef[2] * x[2]


def down(I):
    h, w = I.shape
    y0, x0 = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    return (((I[y0][:, x0] + I[y0][:, x1]) + I[y1][:, x0]) + I[y1][:, x1]) * I.dtype.type(0.25)


def pyramid(g, levels=None):
    """gray [H,W] -> [level 0, level 1, ...]"""
    out = [g]
    for _ in pyramid_sizes(*g.shape, levels)[1:]:
        out.append(down(out[-1]))
    return out


def gradients(I):
    h, w = I.shape
    x, y = np.arange(w), np.arange(h)
    half = I.dtype.type(0.5)
    return half * (I[:, np.minimum(x + 1, w - 1)] - I[:, np.maximum(x - 1, 0)]), \
        half * (I[np.minimum(y + 1, h - 1)] - I[np.maximum(y - 1, 0)])


def sample(I, fx, fy):
    """Bilinear sample of I at (fx, fy), coordinates clamped to the image, neighbour indices min(x0 + 1, w - 1)."""
    h, w = I.shape
    dt = I.dtype.type
    fx, fy = np.clip(fx, dt(0), dt(w - 1)), np.clip(fy, dt(0), dt(h - 1))
    x0f, y0f = np.floor(fx), np.floor(fy)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = fx - x0f, fy - y0f
    one = dt(1)
    top = I[y0, x0] * (one - ax) + I[y0, x1] * ax
    bot = I[y1, x0] * (one - ax) + I[y1, x1] * ax
    return top * (one - ay) + bot * ay


def upsample(f, h, w):
    """Step 3: the coarser flow [2,hc,wc] read at level size (h, w): 2 * f[y // 2, x // 2]."""
    return f.dtype.type(2) * f[:, (np.arange(h) // 2)[:, None], (np.arange(w) // 2)[None, :]]


def _patch_grid(h, w, dt):
    oy, ox = np.asarray(origins(h)), np.asarray(origins(w))
    Y = (oy[:, None, None, None] + np.arange(PATCH)[None, None, :, None]) + np.zeros((1, len(ox), 1, PATCH), np.int64)
    X = (ox[None, :, None, None] + np.arange(PATCH)[None, None, None, :]) + np.zeros((len(oy), 1, PATCH, 1), np.int64)
    return oy, ox, Y, X


def patch_search(Ia, Ib, init=None, iters=12, dtype=np.float64, details=False):
    """Steps 1-6 on one level.  Ia, Ib [h,w]; init: the dense flow [2,h,w] AT THIS LEVEL (None: zero) -> records [npy,npx,3] =
    (u, v, mean(J) - mean(T)).  details: also det [npy,npx] and the squared displacement before the step-6 test."""
    dt = np.dtype(dtype).type
    Ia, Ib = np.asarray(Ia).astype(dtype), np.asarray(Ib).astype(dtype)
    h, w = Ia.shape
    oy, ox, Y, X = _patch_grid(h, w, dt)
    gxi, gyi = gradients(Ia)
    T, gx, gy = Ia[Y, X], gxi[Y, X], gyi[Y, X]
    s = lambda v: v.sum(axis=(2, 3), dtype=dtype)
    inv = dt(1.0 / 64.0)
    if init is None:
        u0 = v0 = np.zeros((len(oy), len(ox)), dtype)
    else:
        c = np.asarray(init).astype(dtype)[:, (oy + 3)[:, None], (ox + 3)[None, :]]
        u0, v0 = c[0], c[1]
    mT = s(T) * inv
    Tm = T - mT[..., None, None]
    a, b, c = s(gx * gx), s(gx * gy), s(gy * gy)
    det = a * c - b * b
    ok = det > dt(DET_MIN)
    sdet = np.where(ok, det, dt(1))
    Xf, Yf = X.astype(dtype), Y.astype(dtype)
    u, v = u0.copy(), v0.copy()
    for _ in range(iters):
        J = sample(Ib, Xf + u[..., None, None], Yf + v[..., None, None])
        r = (J - (s(J) * inv)[..., None, None]) - Tm
        bx, by = s(r * gx), s(r * gy)
        u = np.where(ok, u - (c * bx - b * by) / sdet, u)
        v = np.where(ok, v - (a * by - b * bx) / sdet, v)
    d2 = (u - u0) * (u - u0) + (v - v0) * (v - v0)
    far = d2 > dt(MAX_STEP2)
    u, v = np.where(far, u0, u), np.where(far, v0, v)
    J = sample(Ib, Xf + u[..., None, None], Yf + v[..., None, None])
    rec = np.stack([u, v, s(J) * inv - mT], -1)
    return (rec, det, d2) if details else rec


def densify(Ia, Ib, rec, dtype=np.float64):
    """Step 7 on one level: records [npy,npx,3] -> dense flow [2,h,w]."""
    dt = np.dtype(dtype).type
    Ia, Ib, rec = np.asarray(Ia).astype(dtype), np.asarray(Ib).astype(dtype), np.asarray(rec).astype(dtype)
    h, w = Ia.shape
    _, _, Y, X = _patch_grid(h, w, dt)
    u, v, d = (rec[..., k][..., None, None] for k in range(3))
    r = (sample(Ib, X.astype(dtype) + u, Y.astype(dtype) + v) - Ia[Y, X]) - d
    wgt = dt(1) / np.maximum(dt(1), np.abs(r))
    flat = (Y * w + X).ravel()                              # C order: ascending (oy, ox) for every pixel
    su, sv, sw = (np.zeros(h * w, dtype) for _ in range(3))
    np.add.at(su, flat, (wgt * u).ravel())
    np.add.at(sv, flat, (wgt * v).ravel())
    np.add.at(sw, flat, wgt.ravel())
    return np.stack([su / sw, sv / sw]).reshape(2, h, w)


def dense_flow(a, b, value_range=(0, 1), levels=None, finest=0, iters=12, dtype=np.float64):
    """a, b [3,H,W] -> flow [2,H,W] of a -> b."""
    pa, pb = pyramid(gray(a, value_range, dtype), levels), pyramid(gray(b, value_range, dtype), levels)
    flow = None
    for l in range(len(pa) - 1, finest - 1, -1):
        h, w = pa[l].shape
        init = None if flow is None else upsample(flow, h, w)
        flow = densify(pa[l], pb[l], patch_search(pa[l], pb[l], init, iters, dtype), dtype)
    for l in range(finest - 1, -1, -1):
        flow = upsample(flow, *pa[l].shape)
    return flow


# ------------------------------------------------------------------------------------------------ synthetic scenes
def texture(H, W, seed, channels=3):
    """Seeded 1/f texture on 0..1: the sum of Gaussian-filtered white noise at sigma = 1, 2, 4, 8, each at unit variance (equal
    energy per octave: with the bands at their own variance the sigma = 1 band dominates, the coarse levels see no structure
    and a 7.5-px shift is lost), stretched to the range."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    out = np.zeros((channels, H, W))
    for c in range(channels):
        for sigma in (1, 2, 4, 8):
            f = gaussian_filter(rng.standard_normal((H + 64, W + 64)), sigma)[32:32 + H, 32:32 + W]
            out[c] += f / f.std()
    out -= out.min()
    return (out / out.max()).astype(np.float32)


def resample(img, flow):
    """img [C,H,W] read at x + flow(x) (cubic, edge replicated): the frame a of which img is the frame b."""
    from scipy.ndimage import map_coordinates
    C, H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([map_coordinates(img[c].astype(np.float64), [yy + flow[1], xx + flow[0]], order=3, mode="nearest")
                     for c in range(C)]).astype(np.float32)


def motion_field(kind, H, W):
    """The true flow [2,H,W] of the named motion: ("shift", (u, v)) or ("zoom", fraction about the centre)."""
    name, arg = kind
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if name == "shift":
        return np.stack([np.full((H, W), float(arg[0])), np.full((H, W), float(arg[1]))])
    if name == "zoom":
        return np.stack([arg * (xx - (W - 1) / 2), arg * (yy - (H - 1) / 2)])
    raise ValueError(kind)


def pair(kind, H, W, seed=0):
    """(a, b, true flow, mask): a 1/f texture b and the frame a that the known flow makes of it; mask: >= 8 px from the border
    and the target inside the frame."""
    flow = motion_field(kind, H, W)
    b = texture(H, W, seed)
    a = resample(b, flow)
    yy, xx = np.mgrid[0:H, 0:W]
    tx, ty = xx + flow[0], yy + flow[1]
    mask = (yy >= 8) & (yy < H - 8) & (xx >= 8) & (xx < W - 8) & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
    return a, b, flow, mask


def two_layer(H, W, obj=(24, 36), motion=(3, -2), seed=0):
    """(a, b, true flow, object mask in a): an obj = (h, w) textured rectangle moving by motion = (u, v) over a static
    textured background."""
    bg, fg = texture(H, W, seed), texture(H, W, seed + 1000)
    oh, ow = obj
    y0, x0 = (H - oh) // 2, (W - ow) // 2
    u, v = motion
    a, b = bg.copy(), bg.copy()
    a[:, y0:y0 + oh, x0:x0 + ow] = fg[:, :oh, :ow]
    b[:, y0 + v:y0 + v + oh, x0 + u:x0 + u + ow] = fg[:, :oh, :ow]
    flow = np.zeros((2, H, W))
    inside = np.zeros((H, W), bool)
    inside[y0:y0 + oh, x0:x0 + ow] = True
    flow[0][inside], flow[1][inside] = u, v
    return a, b, flow, inside


def epe(flow, true, mask):
    return float(np.sqrt(((flow - true) ** 2).sum(0))[mask].mean())


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
FULL_SIZES = [(64, 128), (33, 65), (37, 70)]
MOTIONS = [("shift", (1.7, -0.9)), ("shift", (7.5, 3.25)), ("zoom", 0.04)]
FULL_CASES = [(size, m) for size in FULL_SIZES for m in MOTIONS if not (m[1] == (7.5, 3.25) and size != (64, 128))]
STAGE_SIZES = [(8, 8), (8, 9), (9, 8), (16, 16), (21, 37)]


def level_pair(h, w, n, corner, leave, seed=0):
    """Stage inputs: gray level images ia, ib [n,h,w] float32 on 0..255 and a random initial flow [n,2,h,w] with |.| <= 3.
    corner: a constant 10 x 10 corner in both (det below the threshold there); leave: a motion that takes targets near the
    border out of the frame (the step-6 reset) instead of a sub-pixel one."""
    rng = np.random.default_rng(1000 * h + 10 * w + n + 7 * seed)
    ia, ib = np.zeros((n, h, w), np.float32), np.zeros((n, h, w), np.float32)
    for i in range(n):
        shift = (4.5 - 0.5 * i, -3.25 + 0.25 * i) if leave else (0.7 - 0.2 * i, -0.4 + 0.3 * i)
        tex = texture(h + 32, w + 32, 17 * h + w + i + seed, channels=1)
        flow = motion_field(("shift", shift), h + 32, w + 32)
        ib[i] = 255.0 * tex[0, 16:16 + h, 16:16 + w]
        ia[i] = 255.0 * resample(tex, flow)[0, 16:16 + h, 16:16 + w]
        if corner:
            ia[i, :10, :10] = 97.0
            ib[i, :10, :10] = 97.0
    init = rng.uniform(-3, 3, (n, 2, h, w)).astype(np.float32)
    return ia, ib, init


def search_cases():
    return [(h, w, n, corner, leave) for (h, w) in STAGE_SIZES for n in (1, 3) for corner in (False, True)
            for leave in (False, True)]


def excluded(det, d2):
    """Patches whose float64 det is within 0.1 % of the threshold or whose squared displacement is within 0.01 of 64: either
    side of the test is a correct answer there."""
    return (np.abs(det - DET_MIN) <= 1e-3 * DET_MIN) | (np.abs(d2 - MAX_STEP2) <= 0.01)


def interior(mask, margin=STRIDE):
    """The pixels of a mask at least `margin` (one patch stride by default) from its edge."""
    from scipy.ndimage import binary_erosion
    return binary_erosion(mask, iterations=margin)


CLIP_BOXES = [(11001, 8, 10, 24, 32, (3, 0)), (12002, 38, 80, 24, 32, (0, -3))]      # id, y, x at frame 0, h, w, (dx, dy) per frame


def moving_boxes_clip(H=64, W=128, T=7, seed=0):
    """A painted clip: video [3,T,H,W] float32 on 0..1 and instance maps [T,H,W] int32 (background id 7) of two textured boxes
    moving 3 px per frame over a static textured background."""
    bg = texture(H, W, seed)
    video, inst = np.zeros((3, T, H, W), np.float32), np.full((T, H, W), 7, np.int32)
    for t in range(T):
        video[:, t] = bg
        for k, (i, y, x, h, w, (dx, dy)) in enumerate(CLIP_BOXES):
            yy, xx = y + dy * t, x + dx * t
            video[:, t, yy:yy + h, xx:xx + w] = texture(h, w, seed + 100 + k)
            inst[t, yy:yy + h, xx:xx + w] = i
    return video, inst
