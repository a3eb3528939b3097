"""NumPy restatement of the block-matching seed of the dense flow's coarsest level (fl_patch_match_kernel in
csrc/dense_flow.hip), unguided and guided, on top of tests/dense_flow_np.py and tests/guided_flow_np.py, in the dtype asked for
(float64: the yardstick; float32: the kernel's precision, the two 64-term sums of a candidate taken serially in raster order as
the kernel takes them), the seeded dense_flow built on the stages of those files, and the inputs of the GPU tests
(tests/test_gpu_flow_seed.py) with the tolerances that belong to them.

A patch tries every integer displacement (dx, dy) in [-R, R]^2 whose 8 x 8 window lies wholly inside b's level, and takes the
one with the smallest key (cost, dx^2 + dy^2, dy, dx); cost = sum(((J - mean(J)) - (T - mean(T)))^2)."""
import numpy as np

import dense_flow_np as NP
import flow_refine_np as RF
import guided_flow_np as G

SEED_RADIUS, SEED_CAP = 4, 8
# A patch whose two lowest costs are closer than this (relative to the second) may choose either in float32: a 64-term fp32
# sum of non-negative terms carries at most 64 * 2^-24 = 3.8e-6 relative error, mJ and Tm add a few 1e-7 more per term, and
# 1e-4 leaves more than 10 x margin over both costs' errors together.
GAP_MIN = 1e-4
EXCLUDED_CAP = 0.01             # seed_excluded() may name at most this share of the patches of any case


def _serial(v, dtype):
    """Sum over the last axis (the 64 pixels of a patch in raster order), one term after the other."""
    acc = np.zeros(v.shape[:-1], dtype)
    for k in range(v.shape[-1]):
        acc = acc + v[..., k]
    return acc


def candidates(radius):
    """(dx, dy) [K] of the (2 R + 1)^2 displacements, dy-major."""
    r = np.arange(-radius, radius + 1)
    return np.tile(r, len(r)), np.repeat(r, len(r))


def patch_match(Ia, Ib, radius=SEED_RADIUS, seg=None, level=0, dtype=np.float64, details=False):
    """Ia, Ib [h,w] -> records [npy,npx,3] = (dx, dy, mean(J) - mean(T)) at the chosen displacement; with seg (the level-0 ids
    of frame a) every sum runs over the n pixels with the id of the patch centre and the records are [npy,npx,4], n last.
    details: also det, its threshold, and the relative gap (second - best) / second of the two lowest costs, windows with the
    winner's values not counted as a second (1 where the patch has one candidate or is not matched at all)."""
    if not 1 <= int(radius) <= SEED_CAP:
        raise ValueError(f"radius must be 1 .. {SEED_CAP}, got {radius}")
    dt = np.dtype(dtype).type
    Ia, Ib = np.asarray(Ia).astype(dtype), np.asarray(Ib).astype(dtype)
    h, w = Ia.shape
    oy, ox, Y, X = NP._patch_grid(h, w, dt)
    gxi, gyi = NP.gradients(Ia)
    T, gx, gy = Ia[Y, X], gxi[Y, X], gyi[Y, X]
    if seg is None:
        m = np.ones(Y.shape, bool)
    else:
        S = G.level_ids(seg, level, h, w)
        m = S[Y, X] == S[(oy + 3)[:, None], (ox + 3)[None, :]][..., None, None]
    n = m.sum(axis=(2, 3))
    nf = n.astype(dtype)
    zero = dt(0)
    s = lambda v: np.where(m, v, zero).sum(axis=(2, 3), dtype=dtype)           # step 4's sums, as the search takes them
    mT = s(T) / nf
    Tm = T - mT[..., None, None]
    a, b, c = s(gx * gx), s(gx * gy), s(gy * gy)
    det = a * c - b * b
    thr = dt(NP.DET_MIN) * ((n * n).astype(dtype) / dt(4096))
    ok = det > thr
    dx, dy = candidates(int(radius))
    K = len(dx)
    valid = ((ox[None, :, None] + dx >= 0) & (ox[None, :, None] + dx <= w - NP.PATCH) &
             (oy[:, None, None] + dy >= 0) & (oy[:, None, None] + dy <= h - NP.PATCH))            # [npy,npx,K]
    # a candidate that is skipped reads nothing; here its window is read at clipped indices and its cost thrown away
    Yc = np.clip(Y[:, :, None] + dy[None, None, :, None, None], 0, h - 1)
    Xc = np.clip(X[:, :, None] + dx[None, None, :, None, None], 0, w - 1)
    mk = np.broadcast_to(m[:, :, None], Yc.shape).reshape(*Yc.shape[:3], 64)
    J = Ib[Yc, Xc].reshape(*Yc.shape[:3], 64)
    mJ = _serial(np.where(mk, J, zero), dtype) / nf[..., None]
    d = (J - mJ[..., None]) - Tm.reshape(*Tm.shape[:2], 1, 64)
    cost = np.where(valid, _serial(np.where(mk, d * d, zero), dtype), dt(np.inf))
    d2 = np.broadcast_to(dx * dx + dy * dy, cost.shape)
    order = np.lexsort((np.broadcast_to(dx, cost.shape), np.broadcast_to(dy, cost.shape), d2, cost), axis=-1)
    best = order[..., 0]
    best = np.where(ok, best, K // 2)                                        # det <= threshold: (0, 0), the middle candidate
    pick = lambda arr: np.take_along_axis(arr, best[..., None], -1)[..., 0]
    rec = [dx[best].astype(dtype), dy[best].astype(dtype), pick(mJ) - mT]
    if seg is not None:
        rec.append(nf)
    rec = np.stack(rec, -1)
    if not details:
        return rec
    # the runner-up: the lowest cost among the candidates whose window differs from the winner's in a pixel that carries the sums.
    # Two windows with the same values (flat regions of b) have the same cost in every precision and every order of summation,
    # and the rest of the key decides between them exactly: that is no ambiguity.
    Jm = np.where(mk, J, zero)
    first = order[..., :1]
    same = (Jm == np.take_along_axis(Jm, first[..., None], 2)).all(-1)
    c0 = np.take_along_axis(cost, first, -1)[..., 0].astype(np.float64)
    c1 = np.where(same, np.inf, cost.astype(np.float64)).min(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(np.isfinite(c1), np.where(c1 > 0, (c1 - c0) / c1, 0.0), 1.0)
    return rec, det, thr, np.where(ok, gap, 1.0)


def seed_excluded(det, thr, gap):
    """Patches on which either answer is correct: det within 0.1 % of its threshold (the rule of the search), or the two lowest
    costs closer than GAP_MIN."""
    return (np.abs(det - thr) <= 1e-3 * thr) | (gap < GAP_MIN)


def seed_radius(seed):
    """None / False -> None; True -> SEED_RADIUS; an int 1 .. SEED_CAP -> that radius."""
    if seed is None or seed is False:
        return None
    return SEED_RADIUS if seed is True else int(seed)


def dense_flow(a, b, seed=True, seg=None, value_range=(0, 1), levels=None, finest=0, iters=12, refine_params=None,
               dtype=np.float64):
    """a, b [3,H,W] (seg: the int ids [H,W] of a, or None) -> flow [2,H,W] of a -> b, the coarsest level seeded: patch_match,
    the densify of its records at that level, and the search started from that dense flow.  seed None: the unseeded flow."""
    radius = seed_radius(seed)
    pa, pb = NP.pyramid(NP.gray(a, value_range, dtype), levels), NP.pyramid(NP.gray(b, value_range, dtype), levels)
    refined = refine_params is not None and refine_params is not False
    flow = None
    for l in range(len(pa) - 1, finest - 1, -1):
        h, w = pa[l].shape
        if flow is not None:
            init = NP.upsample(flow, h, w)
        elif radius is None:
            init = None
        elif seg is None:
            init = NP.densify(pa[l], pb[l], patch_match(pa[l], pb[l], radius, dtype=dtype), dtype)
        else:
            init = G.densify(pa[l], pb[l], patch_match(pa[l], pb[l], radius, seg, l, dtype), seg, l, dtype)
        if seg is None:
            flow = NP.densify(pa[l], pb[l], NP.patch_search(pa[l], pb[l], init, iters, dtype), dtype)
            if refined:
                flow = RF.refine(pa[l], pb[l], flow, dtype=dtype, **RF.params(refine_params))
        else:
            flow = G.densify(pa[l], pb[l], G.patch_search(pa[l], pb[l], seg, init, iters, l, dtype), seg, l, dtype)
            if refined:
                flow = G.refine(pa[l], pb[l], flow, seg, l, dtype=dtype, **RF.params(refine_params))
    for l in range(finest - 1, -1, -1):
        flow = NP.upsample(flow, *pa[l].shape)
    return flow


# ------------------------------------------------------------------------------------------------ the scenes of the error table
# FAST: the unseeded error must exceed FAST_MIN px and the seeded one stay within SEEDED_MAX; SMALL: unchanged to SMALL_SAME px;
# LIMITS: what the seed does not repair.  Each entry builds its case: a, b, the true flow, the mask of the error, ids, levels.
FAST_MIN, SEEDED_MAX, SMALL_SAME = 2.0, 0.1, 1e-3


def pair_case(size, kind, levels=None):
    a, b, true, mask = NP.pair(kind, *size)
    return dict(a=a, b=b, true=true, mask=mask, seg=None, levels=levels)


def object_case(size, obj, motion, guided=True, interior=False):
    a, b, true, inside = NP.two_layer(*size, obj=obj, motion=motion)
    return dict(a=a, b=b, true=true, mask=NP.interior(inside) if interior else inside,
                seg=inside.astype(np.int32) if guided else None, levels=None)


FAST = {"128x256 shift (25, 0)": lambda: pair_case((128, 256), ("shift", (25, 0))),
        "64x128 shift (14, -6)": lambda: pair_case((64, 128), ("shift", (14, -6))),
        "37x70 shift (9, 5)": lambda: pair_case((37, 70), ("shift", (9, 5))),
        "64x128 levels=2 shift (7.5, 3.25)": lambda: pair_case((64, 128), ("shift", (7.5, 3.25)), levels=2),
        "guided 64x128 12x12 (10, 4)": lambda: object_case((64, 128), (12, 12), (10, 4))}
SMALL = {"64x128 shift (1.7, -0.9)": lambda: pair_case((64, 128), ("shift", (1.7, -0.9))),
         "64x128 zoom 0.04": lambda: pair_case((64, 128), ("zoom", 0.04)),
         "128x256 shift (13.5, 6.25)": lambda: pair_case((128, 256), ("shift", (13.5, 6.25)))}
LIMITS = {"guided 64x128 24x36 (12, -5)": lambda: object_case((64, 128), (24, 36), (12, -5)),
          "guided 128x256 50x70 (20, -6)": lambda: object_case((128, 256), (50, 70), (20, -6)),
          "unguided 128x256 50x70 (20, -6) interior": lambda: object_case((128, 256), (50, 70), (20, -6), guided=False,
                                                                          interior=True),
          "128x256 shift (25, -10)": lambda: pair_case((128, 256), ("shift", (25, -10)))}


def case_errors(case, dtype=np.float64):
    """(unseeded, seeded) mean endpoint error of a case over its mask."""
    kw = dict(seg=case["seg"], levels=case["levels"], dtype=dtype)
    return tuple(NP.epe(dense_flow(case["a"], case["b"], seed=s, **kw), case["true"], case["mask"]) for s in (None, True))


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
RADII = [1, 4, 8]
GUIDED_SIZES = [(16, 16), (21, 37)]
GUIDED_MAPS = ["halves", "blobs", "wild"]
GRID_STRIDE = (64, 128, 3)      # h, w, n: 465 patches a pair, 349 workgroups
# The seed of level_pair for the stage cases.  With seed 0 one patch of the 21 x 37, n = 3 cases has its two lowest costs 2.7e-5
# apart (relative), with seeds 2, 3 and 4 several cases exceed EXCLUDED_CAP; with seed 1 the smallest gap over every stage case,
# guided ones included, is 1.3e-4 and seed_excluded() names no patch at all (the GRID_STRIDE case has one of 1395, at 7.0e-5).
STAGE_SEED = 1


def stage_cases():
    """(h, w, n, corner, leave) of the unguided stage test, each run with every radius of RADII."""
    return NP.search_cases()


def stage_inputs(h, w, n, corner, leave):
    """ia, ib [n,h,w] float32 of an unguided stage case."""
    return NP.level_pair(h, w, n, corner, leave, seed=STAGE_SEED)[:2]


def guided_stage_cases():
    """(h, w, n, level) of the guided stage test, each with every map of GUIDED_MAPS and every radius of RADII."""
    return [(h, w, n, level) for (h, w) in GUIDED_SIZES for n in (1, 3) for level in (0, 1)]


def guided_stage_inputs(h, w, n, level, kind):
    """ia, ib [n,h,w] float32 and the level-0 id maps [n,H,W] of a guided stage case."""
    ia, ib, _, seg = G.stage_inputs(h, w, n, level, kind, seed=STAGE_SEED)
    return ia, ib, seg


# the whole-flow cases of the GPU test: name -> (case builder, dense_flow keywords, EPE bound or None)
WHOLE = {"64x128 shift (14, -6)": (FAST["64x128 shift (14, -6)"], {}, SEEDED_MAX),
         "37x70 shift (9, 5)": (FAST["37x70 shift (9, 5)"], {}, SEEDED_MAX),
         "64x128 levels=2 shift (7.5, 3.25)": (FAST["64x128 levels=2 shift (7.5, 3.25)"], {}, SEEDED_MAX),
         "33x65 shift (1.7, -0.9)": (lambda: pair_case((33, 65), ("shift", (1.7, -0.9))), {}, None),
         "guided 12x12 (10, 4)": (FAST["guided 64x128 12x12 (10, 4)"], {}, SEEDED_MAX),
         "guided 12x12 (10, 4) refined": (FAST["guided 64x128 12x12 (10, 4)"], dict(refine_params=True), None)}
# WHOLE_TOL[name]: the bound on max |GPU - float64| of the whole seeded flow.  It is NP.TOL (16 x the float32 - float64 gap of
# the stage restatement) where the float32 - float64 gap of the case's whole seeded flow is within NP.TOL / 16 = 1.6e-4, else 16 x
# that case's own measured gap (WHOLE_GAP; measured 3.477e-4, 6.637e-4, 1.153e-3 and 3.842e-4: a search that starts up to
# half a pixel from its end after an integer seed, four levels deep, is further from float64 than a stage).
# tests/test_flow_seed_cpu.py recomputes every gap; DESIGN.md 4.2q records them.
WHOLE_GAP = {"64x128 shift (14, -6)": 3.5e-4, "37x70 shift (9, 5)": 6.7e-4, "64x128 levels=2 shift (7.5, 3.25)": 1.16e-3,
             "guided 12x12 (10, 4)": 3.9e-4}
WHOLE_TOL = {k: 16 * WHOLE_GAP[k] if k in WHOLE_GAP else NP.TOL for k in WHOLE}
