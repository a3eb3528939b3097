"""NumPy restatement of the segment-guided dense flow (the guided instantiations of csrc/dense_flow.hip and
csrc/flow_refine.hip) on top of tests/dense_flow_np.py and tests/flow_refine_np.py, in the dtype asked for (float64: the
yardstick; float32: the kernels' own precision, with numpy's summation order), the id maps of the GPU tests
(tests/test_gpu_guided_flow.py) and the tolerance that belongs to them.

`seg` is always the LEVEL-0 id map of frame a, int32 [H,W]; a stage on level l reads it as seg[y << l, x << l]."""
import numpy as np

import dense_flow_np as NP
import flow_refine_np as RF

# TOL: 16 x the largest difference between the float32 and the float64 run of this file over the GPU tests' own stage inputs
# (stage_cases() x MAPS): the records of patch_search (patches that excluded() names left out) and the dense flows of densify on
# the float64 records rounded to float32.  tests/test_guided_flow_cpu.py recomputes the gap and asserts gap <= TOL / 16.
# Measured: search 3.84e-4 (21 x 37, N = 3, level 0, "blobs", pair 1; the unguided figure is 1.56e-4), densify 5.8e-5.
# The level_pair seed matters: a patch of a few pixels that walks 7 px from a 3-px-off start is chaotic, and with seed 0 one
# 16-pixel patch of a "blobs" map (det = 155 x its threshold, so no conditioning rule names it) is 0.67 px apart in the two
# precisions.  STAGE_SEED = 2 has no such patch, and none that excluded() leaves out either: the excluded share is 0 in every
# case, with the two rules of the unguided test alone (no rule on small det is needed).
SEARCH_GAP = 3.9e-4
TOL = 16 * SEARCH_GAP
# REFINE_TOL[map]: 16 x the float32 - float64 gap of refine() over refine_cases() of that map (every stage size and 40 x 70, n 1
# and 3, levels 0 and 1, sor 1 and the defaults), the random level_pair flows (up to 3 px) as the initial flow.  A region that
# the cut leaves with few or no neighbours is held by the data term alone, the robust weights are steep there and the result
# itself grows (to 380 px on "checker", where every pixel is alone; 230 px on "blobs"; 8 px with one id), and so does the gap:
# one figure for all maps would loosen the check of the maps that are well conditioned.  The gap also moves with the level_pair
# seed, by an order of magnitude on the cut maps (largest per-map gap over the cases: seed 0 4.4e-2, 1 3.1e-2, 2 7.2e-2,
# 3 2.9e-2, 4 1.2e-2, 5 4.4e-2; always a 5 x 5 run at 21 x 37 or 40 x 70, never a small size).  Measured with REFINE_SEED = 4:
# constant 2.11e-3, halves 2.10e-3 (both 40 x 70, n = 3, level 0), blobs and wild 1.18e-2 (21 x 37, n = 3, level 1), stripes
# 4.49e-3 (16 x 16, n = 1, level 0), checker 1.11e-2 (40 x 70, n = 3, level 0).  These bound the distance to float64 only.  The
# sharp check of the kernel is another one: on every one of these cases and maps the GPU returns the bits of the float32 run
# of refine() (the same operations in the same order, sqrt and division correctly rounded on both sides), and the GPU test
# asserts that equality.
REFINE_GAP = {"constant": 2.2e-3, "halves": 2.2e-3, "blobs": 1.2e-2, "wild": 1.2e-2, "stripes": 4.6e-3, "checker": 1.15e-2}
REFINE_TOL = {k: 16 * v for k, v in REFINE_GAP.items()}


# ------------------------------------------------------------------------------------------------ the algorithm
def level_ids(seg, level, h, w):
    """The ids of level `level`, [h,w]: seg[y << level, x << level] (in bounds for the (h + 1) // 2 pyramid)."""
    seg = np.asarray(seg)
    assert ((h - 1) << level) < seg.shape[0] and ((w - 1) << level) < seg.shape[1]
    return seg[(np.arange(h) << level)[:, None], (np.arange(w) << level)[None, :]]


def patch_search(Ia, Ib, seg, init=None, iters=12, level=0, dtype=np.float64, details=False):
    """Steps 1-6 on one level with every patch sum masked by (id == the id of the patch centre (oy + 3, ox + 3)) -> records
    [npy,npx,4] = (u, v, mean(J) - mean(T), n).  details: also det, its threshold DET_MIN * n^2 / 4096 and the squared
    displacement before the step-6 test."""
    dt = np.dtype(dtype).type
    Ia, Ib = np.asarray(Ia).astype(dtype), np.asarray(Ib).astype(dtype)
    h, w = Ia.shape
    S = level_ids(seg, level, h, w)
    oy, ox, Y, X = NP._patch_grid(h, w, dt)
    gxi, gyi = NP.gradients(Ia)
    T, gx, gy = Ia[Y, X], gxi[Y, X], gyi[Y, X]
    m = S[Y, X] == S[(oy + 3)[:, None], (ox + 3)[None, :]][..., None, None]
    n = m.sum(axis=(2, 3))
    nf = n.astype(dtype)
    zero = dt(0)
    s = lambda v: np.where(m, v, zero).sum(axis=(2, 3), dtype=dtype)
    if init is None:
        u0 = v0 = np.zeros((len(oy), len(ox)), dtype)
    else:
        c = np.asarray(init).astype(dtype)[:, (oy + 3)[:, None], (ox + 3)[None, :]]
        u0, v0 = c[0], c[1]
    mT = s(T) / nf
    Tm = T - mT[..., None, None]
    a, b, c = s(gx * gx), s(gx * gy), s(gy * gy)
    det = a * c - b * b
    thr = dt(NP.DET_MIN) * ((n * n).astype(dtype) / dt(4096))
    ok = det > thr
    sdet = np.where(ok, det, dt(1))
    Xf, Yf = X.astype(dtype), Y.astype(dtype)
    u, v = u0.copy(), v0.copy()
    for _ in range(iters):
        J = NP.sample(Ib, Xf + u[..., None, None], Yf + v[..., None, None])
        r = (J - (s(J) / nf)[..., None, None]) - Tm
        bx, by = s(r * gx), s(r * gy)
        u = np.where(ok, u - (c * bx - b * by) / sdet, u)
        v = np.where(ok, v - (a * by - b * bx) / sdet, v)
    d2 = (u - u0) * (u - u0) + (v - v0) * (v - v0)
    far = d2 > dt(NP.MAX_STEP2)
    u, v = np.where(far, u0, u), np.where(far, v0, v)
    J = NP.sample(Ib, Xf + u[..., None, None], Yf + v[..., None, None])
    rec = np.stack([u, v, s(J) / nf - mT, nf], -1)
    return (rec, det, thr, d2) if details else rec


def densify(Ia, Ib, rec, seg, level=0, dtype=np.float64):
    """Step 7 on one level: records [npy,npx,4] -> dense flow [2,h,w].  A pixel takes the covering patches whose centre has its
    id, weight n / max(1, |r|); all covering patches, same weights, if there is none."""
    dt = np.dtype(dtype).type
    Ia, Ib, rec = np.asarray(Ia).astype(dtype), np.asarray(Ib).astype(dtype), np.asarray(rec).astype(dtype)
    h, w = Ia.shape
    S = level_ids(seg, level, h, w)
    oy, ox, Y, X = NP._patch_grid(h, w, dt)
    u, v, d, n = (rec[..., k][..., None, None] for k in range(4))
    r = (NP.sample(Ib, X.astype(dtype) + u, Y.astype(dtype) + v) - Ia[Y, X]) - d
    wgt = n / np.maximum(dt(1), np.abs(r)) + np.zeros(Y.shape, dtype)
    same = (S[Y, X] == S[(oy + 3)[:, None], (ox + 3)[None, :]][..., None, None]).ravel()
    flat = (Y * w + X).ravel()                              # C order: ascending (oy, ox) for every pixel
    sums = np.zeros((2, 3, h * w), dtype)                   # [matching, all][su, sv, sw]
    for k, val in enumerate(((wgt * u).ravel(), (wgt * v).ravel(), wgt.ravel())):
        np.add.at(sums[0, k], flat[same], val[same])
        np.add.at(sums[1, k], flat, val)
    hit = np.zeros(h * w, bool)
    hit[flat[same]] = True
    su, sv, sw = np.where(hit, sums[0], sums[1])
    return np.stack([su / sw, sv / sw]).reshape(2, h, w)


def outer_iteration(planes, S, u, v, du, dv, alpha=20.0, delta=5.0, gamma=10.0, sor=5, omega=1.6):
    """RF.outer_iteration with the smoothness cut at id borders: a forward difference toward a neighbour of another id is 0 in
    ws, and wR, wD, wL, wU are 0 across an id border.  S: the ids of this level, [h,w]."""
    Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz = planes
    dt = u.dtype.type
    assert all(a.dtype == u.dtype for a in (*planes, v, du, dv))
    alpha, delta, gamma, omega, half, zeta2, eps2 = (dt(x) for x in (alpha, delta, gamma, omega, 0.5, RF.ZETA2, RF.EPS2))
    h, w = u.shape
    sh = RF._shift
    sameR, sameD = sh(S, 0, 1) == S, sh(S, 1, 0) == S       # the clamped neighbour of the last column / row is the pixel itself
    zero = dt(0)
    U, V = u + du, v + dv
    Ux, Uy = np.where(sameR, sh(U, 0, 1) - U, zero), np.where(sameD, sh(U, 1, 0) - U, zero)
    Vx, Vy = np.where(sameR, sh(V, 0, 1) - V, zero), np.where(sameD, sh(V, 1, 0) - V, zero)
    ws = alpha / np.sqrt((((Ux * Ux + Uy * Uy) + Vx * Vx) + Vy * Vy) + eps2)
    wR, wD, wL, wU = (np.zeros((h, w), u.dtype) for _ in range(4))
    wR[:, :-1] = np.where(sameR[:, :-1], half * (ws[:, :-1] + ws[:, 1:]), zero)
    wD[:-1] = np.where(sameD[:-1], half * (ws[:-1] + ws[1:]), zero)
    wL[:, 1:], wU[1:] = wR[:, :-1], wD[:-1]
    sw = ((wL + wR) + wU) + wD
    nI, nX, nY = (Ix * Ix + Iy * Iy) + zeta2, (Ixx * Ixx + Ixy * Ixy) + zeta2, (Ixy * Ixy + Iyy * Iyy) + zeta2
    r = (Iz + Ix * du) + Iy * dv
    wd = (delta / np.sqrt((r * r) / nI + eps2)) / nI
    rx, ry = (Ixz + Ixx * du) + Ixy * dv, (Iyz + Ixy * du) + Iyy * dv
    wg = gamma / np.sqrt(((rx * rx) / nX + (ry * ry) / nY) + eps2)
    wgx, wgy = wg / nX, wg / nY
    A11 = ((wd * Ix) * Ix + (wgx * Ixx) * Ixx) + (wgy * Ixy) * Ixy
    A12 = ((wd * Ix) * Iy + (wgx * Ixx) * Ixy) + (wgy * Ixy) * Iyy
    A22 = ((wd * Iy) * Iy + (wgx * Ixy) * Ixy) + (wgy * Iyy) * Iyy
    b1 = -(((wd * Iz) * Ix + (wgx * Ixz) * Ixx) + (wgy * Iyz) * Ixy)
    b2 = -(((wd * Iz) * Iy + (wgx * Ixz) * Ixy) + (wgy * Iyz) * Iyy)
    D1, D2 = A11 + sw, A22 + sw
    om1 = dt(1) - omega
    parity = (np.arange(h)[:, None] + np.arange(w)[None, :]) & 1
    du, dv = du.copy(), dv.copy()
    for _ in range(int(sor)):
        for colour in (0, 1):
            m = parity == colour
            Uc, Vc = u + du, v + dv
            su = (((wL * sh(Uc, 0, -1) + wR * sh(Uc, 0, 1)) + wU * sh(Uc, -1, 0)) + wD * sh(Uc, 1, 0)) - sw * u
            sv = (((wL * sh(Vc, 0, -1) + wR * sh(Vc, 0, 1)) + wU * sh(Vc, -1, 0)) + wD * sh(Vc, 1, 0)) - sw * v
            # a pixel all of whose edges are cut has D = A11 (A22) alone, which is 0 where the image is flat: its du (dv) stays
            with np.errstate(divide="ignore", invalid="ignore"):
                du = np.where(m & (D1 > 0), om1 * du + omega * (((b1 + su) - A12 * dv) / D1), du)
                dv = np.where(m & (D2 > 0), om1 * dv + omega * (((b2 + sv) - A12 * du) / D2), dv)
    return du, dv


def refine(Ia, Ib, flow, seg, level=0, alpha=20.0, delta=5.0, gamma=10.0, outer=5, sor=5, omega=1.6, dtype=np.float64):
    """The refinement of one level, cut at id borders: Ia, Ib [h,w], flow [2,h,w] -> flow [2,h,w]."""
    flow = np.asarray(flow).astype(dtype)
    planes = RF.prepare(Ia, Ib, flow, dtype)
    S = level_ids(seg, level, *flow.shape[1:])
    u, v = flow[0], flow[1]
    du, dv = np.zeros_like(u), np.zeros_like(v)
    for _ in range(int(outer)):
        du, dv = outer_iteration(planes, S, u, v, du, dv, alpha, delta, gamma, sor, omega)
    return np.stack([u + du, v + dv])


def dense_flow(a, b, seg, value_range=(0, 1), levels=None, finest=0, iters=12, refine_params=None, dtype=np.float64):
    """a, b [3,H,W], seg int [H,W] (the ids of a) -> flow [2,H,W] of a -> b; refine_params as in flow_refine_np.dense_flow."""
    pa, pb = NP.pyramid(NP.gray(a, value_range, dtype), levels), NP.pyramid(NP.gray(b, value_range, dtype), levels)
    flow = None
    for l in range(len(pa) - 1, finest - 1, -1):
        h, w = pa[l].shape
        init = None if flow is None else NP.upsample(flow, h, w)
        flow = densify(pa[l], pb[l], patch_search(pa[l], pb[l], seg, init, iters, l, dtype), seg, l, dtype)
        if refine_params is not None and refine_params is not False:
            flow = refine(pa[l], pb[l], flow, seg, l, dtype=dtype, **RF.params(refine_params))
    for l in range(finest - 1, -1, -1):
        flow = NP.upsample(flow, *pa[l].shape)
    return flow


# ------------------------------------------------------------------------------------------------ the scenes of the quality bounds
SCENES = [((64, 128), (24, 36), (3, -2)), ((64, 128), (12, 12), (3, -2)), ((64, 128), (24, 36), (-5, 4)),
          ((128, 256), (50, 70), (6, -3))]


def scene(size, obj, motion):
    """(a, b, true flow, object mask, ids = the object mask as int32, background >= 8 px from the object)."""
    from scipy.ndimage import binary_dilation
    a, b, true, inside = NP.two_layer(*size, obj=obj, motion=motion)
    return a, b, true, inside, inside.astype(np.int32), ~binary_dilation(inside, iterations=8)


# ------------------------------------------------------------------------------------------------ the clip of the end-to-end test
CLIP_T_IN = 2
CLIP_BOUND = 0.1                # px, mean endpoint error of target_bw_of over a whole box of moving_boxes_clip(), band included


def clip_target_bw(video, inst, t_in, t_out, value_range=(0, 1), guided=True, **kw):
    """target_bw_of [2,t_out,H,W] of c2m_amd.flow.clip_flows in float64: the backward steps c_j+1 -> c_j, each guided by the ids of
    frame j + 1 (inst [T,H,W]; guided False: the unguided flow), chained from every predicted frame to the last input frame."""
    import flow_chain_np as C
    pair = (lambda a, b, ids: dense_flow(a, b, ids, value_range, **kw)) if guided else \
        (lambda a, b, ids: RF.dense_flow(a, b, value_range, refine_params=kw.get("refine_params")))
    first = t_in - 1
    bw = np.stack([pair(video[:, first + j + 1], video[:, first + j], inst[first + j + 1]) for j in range(t_out)])
    return C.chain(bw, "backward")[0].transpose(1, 0, 2, 3)


def clip_box_errors(target_bw, inst, t_in):
    """{(box id, k): (mean EPE over the box's pixels in frame t_in + k, over its 4-px edge band)} against the true backward flow
    -(k + 1) (dx, dy) of the boxes of moving_boxes_clip()."""
    out = {}
    for i, _, _, _, _, (dx, dy) in NP.CLIP_BOXES:
        for k in range(target_bw.shape[1]):
            inside = inst[t_in + k] == i
            true = np.zeros((2,) + inside.shape)
            true[0], true[1] = -(k + 1) * dx, -(k + 1) * dy
            out[(i, k)] = (NP.epe(target_bw[:, k], true, inside), NP.epe(target_bw[:, k], true, RF.object_masks(inside)[1]))
    return out


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
STAGE_SEED, REFINE_SEED = 2, 4  # of level_pair, for the search / densify cases and for the refinement's: see TOL, REFINE_TOL
MAPS = ["constant", "halves", "blobs", "stripes", "checker", "wild"]


def id_map(kind, H, W, seed=0, level=0):
    """A level-0 id map int32 [H,W] for a stage on level `level`.  constant: one id; halves: two ids, the border right behind a
    column of patch centres of that level (x = 4 j + 3), so that it runs through patches and their centre pixels sit on it;
    blobs: random blobs of five ids; stripes: columns of two alternating ids, 1 px wide at that level (patch centres are in odd
    columns but for a clamped last patch: every pixel of an even column falls back in densify); checker: every pixel its own
    id (n = 1 everywhere: nothing is searched, nothing is smoothed); wild: blobs with negative and large ids."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "constant":
        return np.full((H, W), 5, np.int32)
    if kind == "halves":
        wl = (W + (1 << level) - 1) >> level
        centre = 4 * (wl // 8 if wl >= 16 else 0) + 3
        return np.where(xx <= (centre << level), 3, 9).astype(np.int32)
    if kind in ("blobs", "wild"):
        from scipy.ndimage import gaussian_filter
        rng = np.random.default_rng(100 * H + W + seed)
        f = gaussian_filter(rng.standard_normal((H + 16, W + 16)), 2.5)[8:8 + H, 8:8 + W]
        k = np.digitize(f, np.quantile(f, [0.2, 0.4, 0.6, 0.8]))
        names = np.asarray([0, 1, 2, 3, 4] if kind == "blobs" else [-2 ** 31, -1, 0, 2 ** 31 - 1, 1 << 24], np.int64)
        return names[k].astype(np.int32)
    if kind == "stripes":
        return np.where((xx >> level) & 1, 21, 12).astype(np.int32)
    if kind == "checker":
        return (yy * W + xx).astype(np.int32)
    raise ValueError(kind)


def stage_cases():
    """(h, w, n, level) of the stage tests: NP.STAGE_SIZES, n in {1, 3}, levels 0 and 1; the map of a level-1 case is the
    level-0 map of size (2 h - 1, 2 w), odd and even."""
    return [(h, w, n, level) for (h, w) in NP.STAGE_SIZES for n in (1, 3) for level in (0, 1)]


def refine_cases():
    """(h, w, n, level, refinement parameters) of the iterate kernel's cases: every stage case and MULTI_TILE (six tiles with a
    ragged remainder) with n in {1, 3} and levels 0 and 1, each with sor 1 (one outer iteration) and the defaults (5 x 5)."""
    return [(h, w, n, level, kw) for (h, w) in NP.STAGE_SIZES + [RF.MULTI_TILE] for n in (1, 3) for level in (0, 1)
            for kw in (dict(outer=1, sor=1), {})]


def stage_inputs(h, w, n, level, kind, seed=STAGE_SEED):
    """(ia, ib, init, seg [n,H,W]) of a stage case: the level_pair images (the corner comes with level 1, the leaving motion with
    n = 3) and one map per pair."""
    ia, ib, init = NP.level_pair(h, w, n, bool(level), n == 3, seed=seed)
    H, W = ((h, w) if level == 0 else (2 * h - 1, 2 * w))
    seg = np.stack([id_map(kind, H, W, seed=i, level=level) for i in range(n)])
    return ia, ib, init, seg


def excluded(det, thr, d2):
    """Patches whose float64 det is within 0.1 % of their threshold or whose squared displacement is within 0.01 of 64: either
    side of the test is a correct answer there."""
    return (np.abs(det - thr) <= 1e-3 * thr) | (np.abs(d2 - NP.MAX_STEP2) <= 0.01)
