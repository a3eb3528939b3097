"""The dataset-resolution composite of c2m_amd.fullres (ops.detail_warp) restated in float64 numpy, from its definition
(DESIGN.md 4.2g), not from the kernel.  Returns the value before rounding as well as the levels, so that a test can tell
the pixels that sit on a rounding boundary."""
import numpy as np


def up_taps(n_in, n_out):
    """upsample_bilinear2d(align_corners=False) along one axis -> (i0, i1, lam, pos): pos is the source coordinate before
    the clamp at 0."""
    pos = float(n_in) / n_out * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    s = np.maximum(pos, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0, pos


def up(A, H, W):
    """[..., h, w] -> [..., H, W]."""
    A = np.asarray(A, np.float64)
    y0, y1, ly, _ = up_taps(A.shape[-2], H)
    x0, x1, lx, _ = up_taps(A.shape[-1], W)
    ly = ly[:, None]
    with np.errstate(invalid="ignore"):
        top = (1 - lx) * A[..., y0, :][..., x0] + lx * A[..., y0, :][..., x1]
        bot = (1 - lx) * A[..., y1, :][..., x0] + lx * A[..., y1, :][..., x1]
        return (1 - ly) * top + ly * bot


def source(flow, H, W):
    """flow [B,2,T,h,w] -> (IX, IY) [B,T,H,W]: where each output pixel reads the full-size frame, clamped, NaN -> 0."""
    h, w = flow.shape[-2:]
    xl = up_taps(w, W)[3][None, :]
    yl = up_taps(h, H)[3][:, None]
    f = up(flow, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        IX = (xl + f[:, 0]) * W / (w - 1) - 0.5
        IY = (yl + f[:, 1]) * H / (h - 1) - 0.5
    IX = np.where(np.isnan(IX), 0.0, np.clip(IX, 0.0, W - 1.0))
    IY = np.where(np.isnan(IY), 0.0, np.clip(IY, 0.0, H - 1.0))
    return IX, IY


def detail_warp(F, G, Wl, flow, occ=None, ids=None, occ_threshold=None, fill_id=0):
    """F uint8 [B,H,W,3]; G, Wl [B,3,T,h,w]; flow [B,2,T,h,w]; occ [B,1,T,h,w] or None; ids int32 [B,H,W] or None.
    -> dict(v float64 [B,T,H,W,3] before clip and rounding, levels uint8 [B,T,H,W,3], IX, IY [B,T,H,W], occ_up [B,T,H,W],
    ids int32 [B,T,H,W] or None)."""
    F = np.asarray(F)
    B, H, W, _ = F.shape
    T = G.shape[2]
    IX, IY = source(np.asarray(flow, np.float64), H, W)
    x0 = np.floor(IX).astype(np.int64)
    y0 = np.floor(IY).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    assert x0.min() >= 0 and x0.max() <= W - 1 and y0.min() >= 0 and y0.max() <= H - 1
    lx, ly = (IX - x0)[..., None], (IY - y0)[..., None]
    Fd = F.astype(np.float64)
    bi = np.arange(B)[:, None, None, None]
    warpF = (1 - ly) * ((1 - lx) * Fd[bi, y0, x0] + lx * Fd[bi, y0, x1]) + \
        ly * ((1 - lx) * Fd[bi, y1, x0] + lx * Fd[bi, y1, x1])                                    # [B,T,H,W,3]
    to_last = lambda a: np.moveaxis(a, 1, -1)                                                      # [B,C,T,H,W] -> [B,T,H,W,C]
    occ_up = np.ones((B, T, H, W)) if occ is None else up(occ, H, W)[:, 0]
    with np.errstate(invalid="ignore"):
        v = 255.0 * to_last(up(G, H, W)) + occ_up[..., None] * (warpF - 255.0 * to_last(up(Wl, H, W)))
        levels = np.where(np.isnan(v), 0.0, np.floor(np.clip(v, 0.0, 255.0) + 0.5)).astype(np.uint8)
    out_ids = None
    if ids is not None:
        out_ids = np.asarray(ids)[bi, np.rint(IY).astype(np.int64), np.rint(IX).astype(np.int64)].astype(np.int32)
        if occ_threshold is not None:
            with np.errstate(invalid="ignore"):
                out_ids = np.where(occ_up < occ_threshold, np.int32(fill_id), out_ids)
    return dict(v=v, levels=levels, IX=IX, IY=IY, occ_up=occ_up, ids=out_ids)


def warp_small(f, flow):
    """The working-size warp in float64 (utils.resample's coordinate rule, border padding): f [B,3,h,w] in [0, 1], flow
    [B,2,T,h,w] -> [B,3,T,h,w].  Stands in for ops.flow_warp where a test has no GPU."""
    B, _, h, w = f.shape
    F = np.moveaxis(np.asarray(f, np.float64), 1, -1)                                              # [B,h,w,3]
    IX, IY = source(np.asarray(flow, np.float64), h, w)
    x0 = np.floor(IX).astype(np.int64)
    y0 = np.floor(IY).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    lx, ly = (IX - x0)[..., None], (IY - y0)[..., None]
    bi = np.arange(B)[:, None, None, None]
    out = (1 - ly) * ((1 - lx) * F[bi, y0, x0] + lx * F[bi, y0, x1]) + ly * ((1 - lx) * F[bi, y1, x0] + lx * F[bi, y1, x1])
    return np.moveaxis(out, -1, 1)                                                                 # [B,T,h,w,3] -> [B,3,T,h,w]


def boundary_distance(v):
    """Distance of clip(v, 0, 255) from the nearest rounding boundary k + 0.5."""
    c = np.clip(np.where(np.isnan(v), 0.0, v), 0.0, 255.0)
    return np.abs(c - np.floor(c) - 0.5)


def make_case(h, w, H, W, B, T, seed):
    """The seeded inputs of the kernel tests: random uint8 detail on a smooth base, flow ~ N(0, 1.5), occ ~ U(0, 1),
    G = clip(Wl + N(0, 0.05)), block-constant ids.  Wl is the float64 working-size warp of the nearest-sampled frame rounded to
    fp32 (what the kernel is handed); every array is in the dtype the kernel takes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 70 * np.sin(xx / W * 5.0 + np.arange(3)[:, None, None]) * np.cos(yy / H * 4.0)   # [3,H,W]
    F = np.clip(base[None] + rng.integers(-40, 41, (B, 3, H, W)), 0, 255).astype(np.uint8)
    F = np.ascontiguousarray(np.moveaxis(F, 1, -1))                                                # [B,H,W,3]
    small = up_down(F, h, w)
    flow = (rng.standard_normal((B, 2, T, h, w)) * 1.5).astype(np.float32)
    occ = rng.uniform(0, 1, (B, 1, T, h, w)).astype(np.float32)
    Wl = warp_small(small, flow).astype(np.float32)
    G = np.clip(Wl + rng.standard_normal(Wl.shape) * 0.05, 0, 1).astype(np.float32)
    ids = (1000 + rng.integers(0, 50, (B, -(-H // 3), -(-W // 3)))).repeat(3, 1).repeat(3, 2)[:, :H, :W].astype(np.int32)
    return dict(F=F, G=G, Wl=Wl, flow=flow, occ=occ, ids=np.ascontiguousarray(ids))


def up_down(F, h, w):
    """A working-size stand-in for a full-size uint8 frame [B,H,W,3] -> [B,3,h,w] in [0, 1]: nearest sample (the tests need
    a plausible partner, not a particular filter)."""
    B, H, W, _ = F.shape
    ys = np.minimum(((np.arange(h) + 0.5) * H / h).astype(np.int64), H - 1)
    xs = np.minimum(((np.arange(w) + 0.5) * W / w).astype(np.int64), W - 1)
    return np.moveaxis(F[:, ys][:, :, xs].astype(np.float64) / 255.0, -1, 1)
