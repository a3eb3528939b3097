"""NumPy float64 restatement of the flow scores (csrc/flow_score.hip, c2m_amd/evaluate.py): both operators in
the kernels' operation order, flow_regions, and the host arithmetic.  Inputs are converted to float64 first (exact for fp32 and
for bf16 values held in fp32), every written operation rounds once, every threshold compares squared quantities: the counts
are then functions of + and x alone and equal the device's exactly; the sums differ from it only in the order of addition.

Flows are in pixels, channel 0 = x: a(x) ~ b(x + flow(x))."""
import numpy as np

import dense_flow_np as D

ROWS = 9
QUALITY_COLUMNS = ("n", "n_nonfinite", "sum_epe", "sum_e2", "sum_mag", "sum_ae", "n_out", "n_gt1", "n_gt3", "n_gt5")
CONSISTENCY_COLUMNS = ("n", "n_inside", "sum_photo", "sum_photo2", "sum_fb", "n_incons", "sum_photo_cons")
REGIONS = ("object", "background", "boundary", "occluded", "slow", "medium", "fast")
COUNT_Q, SUM_Q = (0, 1, 6, 7, 8, 9), (2, 3, 4, 5)
COUNT_C, SUM_C = (0, 1, 5), (2, 3, 4, 6)
QC = {k: i for i, k in enumerate(QUALITY_COLUMNS)}
CC = {k: i for i, k in enumerate(CONSISTENCY_COLUMNS)}


def _rows(mask, regions):
    """The nine row masks of one pair: `mask`, then `mask` and region bit k."""
    out = [mask]
    for k in range(8):
        out.append(mask & (((regions >> k) & 1) != 0) if regions is not None else np.zeros_like(mask))
    return out


def flow_quality_terms(pred, target, valid=None):
    """Per-pixel terms of one pair, pred / target [2,H,W]: dict of scored, nonfinite (bool), epe, e2, mag, ae (0 where not scored
    or nonfinite), out, gt1, gt3, gt5 (bool, True for a nonfinite pixel)."""
    with np.errstate(all="ignore"):
        pu, pv = np.asarray(pred[0], np.float64), np.asarray(pred[1], np.float64)
        tu, tv = np.asarray(target[0], np.float64), np.asarray(target[1], np.float64)
        scored = np.isfinite(tu) & np.isfinite(tv) & (np.abs(tu) < 1e9) & (np.abs(tv) < 1e9)
        if valid is not None:
            scored &= np.asarray(valid) != 0
        fin = scored & np.isfinite(pu) & np.isfinite(pv)
        bad = scored & ~fin
        du, dv = pu - tu, pv - tv
        e2, m2 = du * du + dv * dv, tu * tu + tv * tv
        c = ((1.0 + pu * tu) + pv * tv) / np.sqrt(((1.0 + pu * pu) + pv * pv) * (1.0 + m2))
        ae = np.arccos(np.minimum(np.maximum(c, -1.0), 1.0))
        z = lambda x: np.where(fin, x, 0.0)
        return {"scored": scored, "nonfinite": bad, "epe": z(np.sqrt(e2)), "e2": z(e2), "mag": z(np.sqrt(m2)), "ae": z(ae),
                "out": bad | (fin & (e2 > 9.0) & (e2 > 0.0025 * m2)), "gt1": bad | (fin & (e2 > 1.0)),
                "gt3": bad | (fin & (e2 > 9.0)), "gt5": bad | (fin & (e2 > 25.0))}


def flow_quality_sums(pred, target, valid=None, regions=None):
    """pred, target [N,2,H,W] -> float64 [N,9,10]."""
    N = pred.shape[0]
    out = np.zeros((N, ROWS, len(QUALITY_COLUMNS)))
    for i in range(N):
        t = flow_quality_terms(pred[i], target[i], None if valid is None else valid[i])
        for r, m in enumerate(_rows(t["scored"], None if regions is None else np.asarray(regions[i]))):
            out[i, r] = [m.sum(), (m & t["nonfinite"]).sum(), t["epe"][m].sum(), t["e2"][m].sum(), t["mag"][m].sum(),
                         t["ae"][m].sum(), (m & t["out"]).sum(), (m & t["gt1"]).sum(), (m & t["gt3"]).sum(), (m & t["gt5"]).sum()]
    return out


def _sample(img, x0, x1, y0, y1, ax, ay):
    """flow_sample.h's corner and association order, in float64."""
    top = img[y0, x0] * (1.0 - ax) + img[y0, x1] * ax
    bot = img[y1, x0] * (1.0 - ax) + img[y1, x1] * ax
    return top * (1.0 - ay) + bot * ay


def flow_consistency_terms(flow_ab, a, b, flow_ba=None, alpha1=0.01, alpha2=0.5):
    """Per-pixel terms of one pair, flows [2,H,W], a / b [C,H,W]: dict of inside, incons (bool), photo, fb (float64, NaN
    outside), fb_sum (fb where fb^2 is finite, else 0)."""
    with np.errstate(all="ignore"):
        fu, fv = np.asarray(flow_ab[0], np.float64), np.asarray(flow_ab[1], np.float64)
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        C, H, W = a.shape
        yy0, xx0 = np.mgrid[0:H, 0:W].astype(np.float64)
        yx, yy = xx0 + fu, yy0 + fv
        inside = np.isfinite(fu) & np.isfinite(fv) & (yx >= 0.0) & (yx <= W - 1.0) & (yy >= 0.0) & (yy <= H - 1.0)
        sx, sy = np.where(inside, yx, 0.0), np.where(inside, yy, 0.0)
        x0f, y0f = np.floor(sx), np.floor(sy)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        ax, ay = sx - x0f, sy - y0f
        s = np.zeros((H, W))
        for c in range(C):
            s = s + np.abs(a[c] - _sample(b[c], x0, x1, y0, y1, ax, ay))
        photo = np.where(inside, s / float(C), np.nan)
        incons, fb, fb_sum = np.zeros((H, W), bool), np.full((H, W), np.nan), np.zeros((H, W))
        if flow_ba is not None:
            gu = _sample(np.asarray(flow_ba[0], np.float64), x0, x1, y0, y1, ax, ay)
            gv = _sample(np.asarray(flow_ba[1], np.float64), x0, x1, y0, y1, ax, ay)
            su, sv = fu + gu, fv + gv
            fb2 = su * su + sv * sv
            incons = inside & ~(fb2 <= alpha1 * ((fu * fu + fv * fv) + (gu * gu + gv * gv)) + alpha2)
            fb = np.where(inside, np.sqrt(fb2), np.nan)
            fb_sum = np.where(inside & np.isfinite(fb2), np.sqrt(fb2), 0.0)
        return {"inside": inside, "incons": incons, "photo": photo, "fb": fb, "fb_sum": fb_sum}


def flow_consistency_sums(flow_ab, a, b, flow_ba=None, regions=None, alpha1=0.01, alpha2=0.5):
    """flows [N,2,H,W], a / b [N,C,H,W] -> (float64 [N,9,7], {"photo", "fb": float32 [N,H,W], "inconsistent": uint8})."""
    N, _, H, W = flow_ab.shape
    out = np.zeros((N, ROWS, len(CONSISTENCY_COLUMNS)))
    maps = {"photo": np.zeros((N, H, W), np.float32), "fb": np.zeros((N, H, W), np.float32),
            "inconsistent": np.zeros((N, H, W), np.uint8)}
    every = np.ones((H, W), bool)
    for i in range(N):
        t = flow_consistency_terms(flow_ab[i], a[i], b[i], None if flow_ba is None else flow_ba[i], alpha1, alpha2)
        p = np.where(t["inside"], t["photo"], 0.0)
        for r, m in enumerate(_rows(every, None if regions is None else np.asarray(regions[i]))):
            mi = m & t["inside"]
            out[i, r] = [m.sum(), mi.sum(), p[mi].sum(), (p * p)[mi].sum(), t["fb_sum"][mi].sum(), (m & t["incons"]).sum(),
                         p[mi & ~t["incons"]].sum()]
        if flow_ba is None:
            out[i, :, 4:] = np.nan
        with np.errstate(all="ignore"):
            maps["photo"][i], maps["fb"][i] = t["photo"].astype(np.float32), t["fb"].astype(np.float32)
        maps["inconsistent"][i] = t["incons"]
    return out, maps


# ------------------------------------------------------------------------------------------------ host arithmetic
def _div(a, b):
    with np.errstate(all="ignore"):
        return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)


def quality_from_sums(sums):
    """[...,9,10] -> {key: [...,9]} (row 0 the frame, rows 1.. the regions)."""
    n, bad, s_epe, s_e2, s_mag, s_ae, n_out, g1, g3, g5 = np.moveaxis(np.asarray(sums, np.float64), -1, 0)
    fin = n - bad
    return {"epe": _div(s_epe, fin), "rmse": np.sqrt(_div(s_e2, fin)), "ae_deg": _div(s_ae, fin) * (180.0 / np.pi),
            "magnitude": _div(s_mag, fin), "fl": _div(n_out, n), "bad1": _div(g1, n), "bad3": _div(g3, n), "bad5": _div(g5, n),
            "nonfinite": bad, "pixels": n}


def consistency_from_sums(sums):
    n, n_in, s_p, s_p2, s_fb, n_inc, s_pc = np.moveaxis(np.asarray(sums, np.float64), -1, 0)
    return {"photo": _div(s_p, n_in), "photo_rms": np.sqrt(_div(s_p2, n_in)), "photo_consistent": _div(s_pc, n_in - n_inc),
            "fb": _div(s_fb, n_in), "inconsistent": _div(n_inc, n_in), "outside": _div(n - n_in, n), "pixels": n}


# ------------------------------------------------------------------------------------------------ regions
def dilate_brute(edge, band):
    """Chebyshev dilation of a [H,W] mask by `band` px, one loop per pixel."""
    H, W = edge.shape
    out = np.zeros_like(edge)
    for y in range(H):
        for x in range(W):
            out[y, x] = edge[max(y - band, 0):y + band + 1, max(x - band, 0):x + band + 1].any()
    return out


def flow_regions(target, instance=None, occlusion=None, occ_threshold=0.5, band=4, jump=1.0, speeds=(10.0, 40.0),
                 id_range=(1000, 19000)):
    """target [N,2,H,W], instance / occlusion [N,H,W] -> uint8 [N,H,W], bits in the order of REGIONS."""
    N, _, H, W = target.shape
    out = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        with np.errstate(all="ignore"):
            u, v = np.asarray(target[i, 0], np.float64), np.asarray(target[i, 1], np.float64)
            edge = np.zeros((H, W), bool)
            for sl_p, sl_q in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))),
                               ((slice(1, None), slice(None)), (slice(None, -1), slice(None)))):
                du, dv = u[sl_p] - u[sl_q], v[sl_p] - v[sl_q]
                d = du * du + dv * dv > float(jump) * float(jump)
                if instance is not None:
                    d = d | (instance[i][sl_p] != instance[i][sl_q])
                edge[sl_p] |= d
                edge[sl_q] |= d
            obj = np.zeros((H, W), bool) if instance is None else (instance[i] >= id_range[0]) & (instance[i] < id_range[1])
            m2 = u * u + v * v
            s0, s1 = float(speeds[0]) ** 2, float(speeds[1]) ** 2
            bits = obj * 1 + (~obj) * 2 + dilate_brute(edge, band) * 4 + (m2 < s0) * 16 + ((m2 >= s0) & (m2 < s1)) * 32 + \
                (m2 >= s1) * 64
            if occlusion is not None:
                bits = bits + (np.asarray(occlusion[i]) < occ_threshold) * 8
        out[i] = bits
    return out


# ------------------------------------------------------------------------------------------------ scenes of the usefulness check
def two_layer_scene():
    """dense_flow_np.two_layer(64, 128, (24, 36), (3, -2)): (a, b, true flow a -> b, true flow b -> a, the occluded strip)."""
    H, W, (oh, ow), (u, v) = 64, 128, (24, 36), (3, -2)
    a, b, fwd, obj = D.two_layer(H, W, (oh, ow), (u, v))
    y0, x0 = (H - oh) // 2, (W - ow) // 2
    obj_b = np.zeros((H, W), bool)
    obj_b[y0 + v:y0 + v + oh, x0 + u:x0 + u + ow] = True
    bwd = np.zeros((2, H, W))
    bwd[0][obj_b], bwd[1][obj_b] = -u, -v
    return a, b, fwd, bwd, obj_b & ~obj                # the background of a that the object covers in b


def shift_scene():
    """dense_flow_np.pair(("shift", (1.7, -0.9)), 64, 128): (a, b, true flow a -> b, true flow b -> a, None)."""
    a, b, fwd, _ = D.pair(("shift", (1.7, -0.9)), 64, 128)
    return a, b, fwd, -fwd, None
