"""Float64 references, input builders and case lists for the L1 / SSIM / RoIAlign / max-pool launch-edge sweeps
(test_gpu_loss_edges.py runs the kernels on them, test_loss_edges_cpu.py checks the references and the input conditions
without a GPU).  Plain torch / numpy; nothing here imports c2m_amd.

Every builder is seeded and returns host tensors whose values the device sees bit for bit (fp32, or bf16 for the bf16 cases):
the float64 reference is evaluated on `.double()` of exactly those values, so no input rounding enters an error figure.

Input conditions (asserted by the CPU module for every case, and again by the GPU module before it compares):

L1    every element has |a - b| >= L1_SEP, or a == b exactly on the planted block; mask values are 0 or >= 0.05.  Then
      |a*m - b*m| >= 5e-5 wherever it is not exactly 0, four hundred ulps of the largest operand: sign(a*m - b*m) is the same
      in fp32 and in float64, and the gradient has no discontinuity near any input.
SSIM  for every family but `equal` and `flat`, fewer than 1 % of the windows have (1 - ssim)/2 within SSIM_CLAMP_MARGIN of the
      clamp's 0 or 1 (in float64): a window on the other side of the clamp has gradient 0, so near the clamp fp32 and float64
      may legitimately disagree by the whole window.  That shapes `near_equal`: with a full-contrast y every window of
      x = y + 1e-3*noise sits about 3e-6 from the clamp (1 - ssim = var(x - y) / (var x + var y + c2), and var y is about 0.08),
      so y is a per-plane constant level plus a ripple of 1e-3 -- then c2 = 9e-4 dominates the denominator and (1 - ssim)/2 is
      about 5e-4 * var(noise) -- and the noise alternates in sign from pixel to pixel with a random amplitude in [0.7, 1.3],
      so that its 3x3 sample variance is at least 0.4 (purely random noise has windows of almost no variance: with them
      ssim_ref(float32) crosses the clamp in a few windows and its gradient error, the yardstick, grows from 2e-4 of
      max|grad| to 5e-2).  No window of this family is within the margin.  The planes are dark (levels 0.05 .. 0.15): the
      rounding of E[x^2] - mu^2 scales with the level squared, and at mid-grey the LOSS error of any fp32 evaluation is the mean of
      zero-mean per-window errors of 3e-5 -- ssim_ref(float32)'s own came out anywhere between 1.5e-8 and 9.7e-7 over twenty
      seeds, a coin flip as a yardstick; dark planes keep it under the 1e-7 floor, and `flat` is the family for that regime.
RoI   no sample coordinate lies within ROI_MARGIN of -1 or of the map's extent, where a sample is dropped: box coordinates
      are on a half-pixel grid, so that x * 0.25 and every difference of two of them is exact in fp32 and in float64 and
      ceil(roi / bins) cannot differ between the two; roi_sample_margin measures the rest.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import thirdparty

L1_SEP = 1e-3
SSIM_CLAMP_MARGIN = 1e-4
ROI_MARGIN = 1e-3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# =============================================================================================== L1 mean
def l1_ref(a, b, mask=None):
    """mean |a*m - b*m| in float64, mask [N,1,...] broadcast over dim 1 (L1MaskedLoss); a, b are used as given (float64 leaves)."""
    if mask is not None:
        mask = mask.double().expand_as(a)
        return (a * mask - b * mask).abs().mean()
    return (a - b).abs().mean()


def l1_ref_grads(a, b, mask, upstream):
    """(value, d a, d b) of upstream * l1_ref in float64 for host tensors of any float type."""
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    v = l1_ref(a64, b64, mask)
    (v * upstream).backward()
    return v.detach(), a64.grad, b64.grad


class L1Case:
    """shape of a and b; mask None | 'binary' | 'frac'; dtype 'f32' | 'bf16'; view: a is handed over as a non-contiguous channel
    slice and the mask as an expanded stride-0 view (the mask then varies along the last axis only)."""

    def __init__(self, name, shape, mask, dtype, seed, view=False):
        self.name, self.shape, self.mask, self.dtype, self.seed, self.view = name, tuple(shape), mask, dtype, seed, view

    def __repr__(self):
        return self.name


L1_CASES = [
    L1Case("one-f32", (1, 1, 1, 1), None, "f32", 100),
    L1Case("one-bf16-masked", (1, 1, 1, 1), "frac", "bf16", 122),
    L1Case("golden-f32", (2, 3, 5, 12, 16), None, "f32", 102),
    L1Case("golden-bf16", (2, 3, 5, 12, 16), None, "bf16", 103),
    L1Case("golden-f32-binary", (2, 3, 5, 12, 16), "binary", "f32", 104),
    L1Case("golden-bf16-frac", (2, 3, 5, 12, 16), "frac", "bf16", 105),
    L1Case("lap2-f32", (3, 5, 7, 50, 50), None, "f32", 106),                 # 262500 elements: second lap, 1024 partials
    L1Case("lap2-f32-frac", (3, 5, 7, 50, 50), "frac", "f32", 107),          # ... C = 5, inner = 17500
    L1Case("lap2-bf16-binary", (3, 5, 7, 50, 50), "binary", "bf16", 108),
    L1Case("odd-f32-binary", (2, 7, 9, 11), "binary", "f32", 109),
    L1Case("odd-bf16-frac", (2, 7, 9, 11), "frac", "bf16", 110),
    L1Case("odd-f32-views", (2, 7, 9, 11), "frac", "f32", 111, view=True),
    L1Case("c1-f32-frac", (4, 1, 33, 65), "frac", "f32", 112),
    L1Case("c1-bf16-binary", (4, 1, 33, 65), "binary", "bf16", 113),
]


def l1_inputs(case):
    """a, b (host, in the case's dtype), mask (fp32 [N,1,...] or None; an expanded view for a `view` case) and `same`, the
    boolean planted block on which a == b exactly.  |a - b| is at least 0.05 elsewhere (before the bf16 rounding of a, which
    moves it by at most 2^-7: the values stay below 4)."""
    g = _gen(case.seed)
    dt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    shape = case.shape
    b = (torch.randn(shape, generator=g).clamp(-2.5, 2.5)).to(dt)
    d = 0.05 + torch.rand(shape, generator=g)
    sgn = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    a = (b.float() + sgn * d).to(dt)
    same = torch.zeros(shape, dtype=torch.bool)
    if a.numel() > 1:                                      # a block that crosses a row end: part of the last rows of plane [0, -1]
        flat = same[0, -1].view(-1)
        flat[flat.numel() // 3: flat.numel() // 3 + min(37, flat.numel() // 2)] = True
        a = torch.where(same, b, a)
    mask = None
    if case.mask is not None:
        mshape = (shape[0], 1) + shape[2:]
        if case.view:                                      # varies along the last axis only: stride 0 everywhere else but dim 0
            mshape = (shape[0], 1) + (1,) * (len(shape) - 3) + shape[-1:]
        u = torch.rand(mshape, generator=g)
        if case.mask == "binary":
            mask = (u > 0.3).float()
        else:                                              # occlusion maps are fractional: exact 0, exact 1, and [0.05, 1) between
            mask = 0.05 + 0.95 * torch.rand(mshape, generator=g)
            mask = torch.where(u < 0.15, torch.zeros(()), torch.where(u > 0.85, torch.ones(()), mask))
        if not case.view and len(shape) > 2 and shape[-2] > 1:
            mask[..., 0, :] = 0.0                          # whole zero rows
            mask[0, :, ..., -1, :] = 0.0
        if case.view:
            mask = mask.expand((shape[0], 1) + shape[2:])
    return a, b, mask, same


def l1_separation(a, b, mask, same):
    """(smallest |a - b| off the planted block, largest |a - b| on it, smallest non-zero mask value) in float64."""
    d = (a.double() - b.double()).abs()
    off = d[~same].min().item() if (~same).any() else math.inf
    on = d[same].max().item() if same.any() else 0.0
    mpos = math.inf
    if mask is not None and (mask > 0).any():
        mpos = mask[mask > 0].min().item()
    return off, on, mpos


# =============================================================================================== SSIM
def ssim_unclamped(x, y):
    """(1 - ssim)/2 per 3x3 window, before the clamp, in the dtype of x and y: five avg_pool2d(3, 1), c1 = 0.01^2, c2 = 0.03^2."""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sx = F.avg_pool2d(x * x, 3, 1) - mu_x * mu_x
    sy = F.avg_pool2d(y * y, 3, 1) - mu_y * mu_y
    sxy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + c1) * (2 * sxy + c2)
    d = (mu_x * mu_x + mu_y * mu_y + c1) * (sx + sy + c2)
    return (1 - n / d) / 2


def ssim_ref(x, y, dtype=torch.float64):
    """SSIMLoss on [N,C,H,W] in `dtype`: float64 is the reference, float32 the yardstick of what the formula itself loses in
    the kernel's precision."""
    return torch.clamp(ssim_unclamped(x.to(dtype), y.to(dtype)), 0, 1).mean()


def ssim_ref_grad(x, y, dtype, upstream=1.0):
    """(loss, d loss / d x) of upstream * ssim_ref in `dtype`, returned as float64."""
    xr = x.detach().to(dtype, copy=True).requires_grad_(True)
    v = ssim_ref(xr, y, dtype)
    (v * upstream).backward()
    return v.detach().double(), xr.grad.double()


def ssim_near_clamp_fraction(x, y):
    """Share of the windows whose (1 - ssim)/2 lies within SSIM_CLAMP_MARGIN of 0 or of 1, or beyond."""
    v = ssim_unclamped(x.double(), y.double())
    return ((v < SSIM_CLAMP_MARGIN) | (v > 1 - SSIM_CLAMP_MARGIN)).double().mean().item()


SSIM_FAMILIES = ["rand01", "rand+-1", "near_equal", "smooth_shift", "anti", "equal", "flat"]
SSIM_OFF_CLAMP = [f for f in SSIM_FAMILIES if f not in ("equal", "flat")]
SSIM_MAIN_SHAPE = (2, 3, 33, 47)
SSIM_EDGE_SHAPES = [(1, 1, 3, 3), (1, 1, 3, 70), (1, 2, 70, 3), (4, 3, 150, 150)]     # the last: 262848 windows
# every family at the main shape; the edge shapes with rand01 and smooth_shift
SSIM_CASES = [(f, SSIM_MAIN_SHAPE) for f in SSIM_FAMILIES] + [(f, s) for s in SSIM_EDGE_SHAPES for f in ("rand01", "smooth_shift")]
_SSIM_SEEDS = {}                                                                       # (family, shape) -> seed, default below


def ssim_inputs(family, shape):
    """x (generated), y (target): fp32 host tensors [N,C,H,W]."""
    N, C, H, W = shape
    seed = _SSIM_SEEDS.get((family, shape), 200 + 13 * SSIM_FAMILIES.index(family) + H + 7 * W)
    g = _gen(seed)
    r = lambda: torch.rand(shape, generator=g, dtype=torch.float64)
    if family == "rand01":
        x, y = r(), r()
    elif family == "rand+-1":
        x, y = 2 * r() - 1, 2 * r() - 1
    elif family == "near_equal":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        level = 0.05 + 0.1 * torch.rand((N, C, 1, 1), generator=g, dtype=torch.float64)
        y = level + 1e-3 * torch.sin(xx / 5.0 + 40 * level) * torch.cos(yy / 7.0)
        x = y + 1e-3 * (2 * ((xx + yy) % 2) - 1) * (0.7 + 0.6 * r())          # alternating sign, random amplitude
    elif family == "smooth_shift":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W + 1, dtype=torch.float64), indexing="ij")
        ph = 6 * torch.rand((N, C, 1, 1), generator=g, dtype=torch.float64)
        base = 0.5 + 0.4 * torch.sin(xx / 1.3 + ph) * torch.cos(yy / 1.7 + 2 * ph)
        x = base[..., :, :W] + 2e-3 * torch.randn(shape, generator=g, dtype=torch.float64)
        y = base[..., :, 1:] + 2e-3 * torch.randn(shape, generator=g, dtype=torch.float64)
    elif family == "anti":
        x = r()
        y = 1 - x
    elif family == "equal":
        x = r()
        y = x
    elif family == "flat":
        x = 0.7 + 1e-4 * torch.randn(shape, generator=g, dtype=torch.float64)
        y = torch.full(shape, 0.7, dtype=torch.float64)
    else:
        raise KeyError(family)
    x = x.float()
    return x, (x if family == "equal" else y.float())


# =============================================================================================== RoIAlign
def roi_ref(feat, boxes, out_size, scale, gout=None):
    """oracle.thirdparty.roi_align on float64 copies: (out, d feat of sum(out * gout)) -- d feat is None without gout."""
    f = feat.double().requires_grad_(gout is not None)
    out = thirdparty.roi_align(f, boxes.double(), out_size, spatial_scale=scale)
    if gout is None:
        return out.detach(), None
    if out.numel():
        (out * gout.double()).sum().backward()
    return out.detach(), (f.grad if f.grad is not None else torch.zeros_like(f))


def roi_sample_coords(box, bins, scale):
    """Float64 sample coordinates (ys, xs) of one box (x1, y1, x2, y2) in image pixels, as RoIAlign(aligned=False,
    sampling_ratio=-1) places them: bins[0] * ceil(roi_h / bins[0]) rows, likewise columns."""
    x1, y1, x2, y2 = (float(v) * scale for v in box)
    out = []
    for lo, hi, nb in ((y1, y2, bins[0]), (x1, x2, bins[1])):
        roi = max(hi - lo, 1.0)
        g = int(math.ceil(roi / nb))
        b = roi / nb
        out.append(np.array([lo + p * b + (i + 0.5) * b / g for p in range(nb) for i in range(g)], np.float64))
    return out[0], out[1]


def roi_sample_margin(boxes, out_size, scale, H, W):
    """Smallest distance of any sample coordinate of any box to -1 or to the map's extent (H for rows, W for columns), where
    the sample drops out of the sum.  boxes [K,5] = (image, x1, y1, x2, y2)."""
    bins = (out_size, out_size) if isinstance(out_size, int) else tuple(out_size)
    m = math.inf
    for row in boxes.tolist():
        ys, xs = roi_sample_coords(row[1:], bins, scale)
        for v, S in ((ys, H), (xs, W)):
            m = min(m, float(np.abs(v + 1.0).min()), float(np.abs(v - S).min()))
    return m


ROI_SCALE = 0.25
ROI_MAP = (10, 13)            # a 40 x 52 image at scale 0.25
# (image, x1, y1, x2, y2) in image pixels, on the half-pixel grid.  Image 2 has no box.  The first box is the K = 1 list.
ROI_BOXES = [
    (0, 8.0, 6.0, 30.0, 26.0),          # inside
    (1, 0.0, 0.0, 52.0, 40.0),          # the whole map
    (0, -21.5, -17.5, 75.5, 60.5),      # larger than the map on all sides
    (1, -10.5, 8.0, 14.0, 30.5),        # straddles the left border
    (0, 36.5, 4.5, 66.0, 33.0),         # straddles the right border
    (1, 11.0, -12.5, 40.5, 12.0),       # straddles the top border
    (0, 6.5, 25.0, 33.5, 55.5),         # straddles the bottom border
    (1, 70.5, 60.5, 90.0, 85.5),        # entirely outside (below right): output 0, gradient 0
    (0, -40.5, 10.0, -12.5, 30.0),      # entirely outside (left)
    (1, 30.0, 10.0, 20.0, 24.0),        # x2 < x1: width clamps to one feature pixel
    (0, 24.0, 31.5, 36.0, 20.5),        # y2 < y1
    (1, 17.5, 22.5, 17.5, 22.5),        # zero size
    (0, 20.5, 12.5, 21.0, 13.0),        # sub-pixel
    (1, 0.0, 0.0, 4.0, 4.0),            # one feature pixel in the top left corner
    (0, 47.5, 35.5, 52.0, 40.0),        # ... and the bottom right corner region
    (1, 2.5, 33.5, 49.5, 38.0),         # wide and flat along the bottom rows
    (0, 44.5, 1.5, 50.0, 38.5),         # tall and thin along the right columns
    (1, 8.0, 6.0, 30.0, 26.0),          # the inside box again, on the other image
    (0, 8.0, 6.0, 30.0, 26.0),          # ... and twice on the same image: the gather must add both
]
# one-row / one-column maps ([1,3,1,9] and [1,3,9,1]; a 36 x 4 image, transposed for the column map): (image, x1, y1, x2, y2)
ROI_BOXES_ROW = [
    (0, 6.0, 0.5, 26.0, 3.5),
    (0, 0.0, 0.0, 36.0, 4.0),
    (0, -9.5, -3.5, 44.5, 9.5),
    (0, -8.5, 1.0, 9.0, 3.0),
    (0, 29.5, 0.5, 49.0, 2.5),
    (0, 50.5, 0.0, 60.0, 4.0),
    (0, 12.5, 1.5, 12.5, 1.5),
]


def roi_boxes_many(K=520):
    """K small boxes on images 0 and 1 of the ROI_MAP image (K > 512: the gather walks the list in global memory), from an integer
    formula on the half-pixel grid: 1.5 .. 6 pixels on a side (at most 1.5 feature pixels), all over the image."""
    rows = []
    for j in range(K):
        x1 = 0.5 * ((j * 37) % 92)
        y1 = 0.5 * ((j * 53) % 68)
        rows.append((j % 2, x1, y1, x1 + 1.5 + 0.5 * (j % 10), y1 + 1.5 + 0.5 * ((j // 3) % 10)))
    return rows


class RoiCase:
    def __init__(self, name, N, C, H, W, bins, boxes, seed):
        self.name, self.N, self.C, self.H, self.W, self.bins, self.seed = name, N, C, H, W, bins, seed
        self.boxes = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 5)

    def __repr__(self):
        return self.name

    @property
    def K(self):
        return self.boxes.shape[0]

    @property
    def bins2(self):
        return (self.bins, self.bins) if isinstance(self.bins, int) else tuple(self.bins)

    def tensors(self):
        """feat [N,C,H,W] and gout [K,C,PH,PW], fp32 on the host."""
        g = _gen(self.seed)
        return (torch.randn((self.N, self.C, self.H, self.W), generator=g),
                torch.randn((self.K, self.C) + self.bins2, generator=g))


def _roi_cases():
    H, W = ROI_MAP
    cases, seed = [], 300
    for C in (1, 8, 9, 19):
        for bins in (7, (3, 5), 1):
            for K in (1, 19):
                bname = bins if isinstance(bins, int) else "x".join(map(str, bins))
                cases.append(RoiCase(f"C{C}-bins{bname}-K{K}", 3, C, H, W, bins, ROI_BOXES[:K], seed))
                seed += 1
    cases.append(RoiCase("C3-bins7-K520", 3, 3, H, W, 7, roi_boxes_many(520), seed))
    cases.append(RoiCase("C3-bins3x5-K0", 3, 3, H, W, (3, 5), [], seed + 1))           # no box at all: d feat is all zeros
    col = [(i, y1, x1, y2, x2) for (i, x1, y1, x2, y2) in ROI_BOXES_ROW]
    for bins in (7, (3, 5), 1):
        bname = bins if isinstance(bins, int) else "x".join(map(str, bins))
        tb = bins if isinstance(bins, int) else (bins[1], bins[0])
        cases.append(RoiCase(f"row1x9-bins{bname}", 1, 3, 1, 9, bins, ROI_BOXES_ROW, seed + 2))
        cases.append(RoiCase(f"col9x1-bins{bname}", 1, 3, 9, 1, tb, col, seed + 3))
        seed += 2
    return cases


ROI_CASES = _roi_cases()
assert len(ROI_BOXES) == 19


# =============================================================================================== max-pool
POOL_SHAPES = [(2, 3, 7, 9), (1, 2, 6, 5), (1, 1, 3, 2)]


def pool_inputs(shape, seed=400):
    """x and gout as bf16 host tensors, with planted ties: a window of four equal values that are its maximum, a window whose
    maximum stands in two places (second row first), and a window of four equal NEGATIVE values."""
    g = _gen(seed + shape[-1])
    x = torch.randn(shape, generator=g).bfloat16()
    N, C, H, W = shape
    x[0, 0, 0:2, 0:2] = 1.5                                # four equal: the gradient goes to the first
    if W >= 4:
        x[0, 0, 0:2, 2:4] = torch.tensor([[-0.5, 0.25], [2.0, 2.0]]).bfloat16()
    if H >= 4:
        x[-1, -1, 2:4, 0:2] = -0.75
    gout = torch.randn((N, C, H // 2, W // 2), generator=g).bfloat16()
    return x, gout
