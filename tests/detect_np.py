"""NumPy float64 restatement of the detector metric after the network: preprocessing, YOLOLayer decode, candidate filter,
suppress-and-merge, matching, trajectory error and the score -- and, for every case, the MARGIN: how far every quantity that
feeds a decision is from the value at which the decision flips.  test_detect_cpu.py pins this file to the live reference's
recorded results and asserts that every planted input keeps its margins above the fp32 rounding of the kernels; the GPU tests
can then demand equal decisions with nothing excluded.

Margins and the bounds they are held against (BOUNDS):
  conf   |conf - conf_thres|                 sigmoid of one fp32 value: a few ulp of a number <= 1
  score  gap between adjacent sorted scores  product of two such numbers
  iou    |IoU - nms_thres|                   ~10 fp32 operations on pixel coordinates (areas with +1), result <= 1
  -> all three held above 64 * 2^-23 = 7.6e-6 (64 ulp of 1.0: an order of magnitude over the operation count).
  corner distance of a kept (merged) corner to the nearest integer and to 0, held above the whole fp32 error a kernel's corner
         can carry: the merge's (n + 4) * 2^-23 * max|corner| (the GPU test's tolerance for the merge alone, which it checks on
         the device's own candidate rows) PLUS the decode's DECODE_ULPS * 2^-23 * max|corner| (decode_bound below).
  area   |box area - 0.01 h w| / (0.01 h w), relative; held above 64 * 2^-23.
  Overlap and the small-object skip are integer arithmetic (2 dx dy > height width; dy dx < 0.005 w h with an integer left
  side): exact in both implementations, margin reported as the integer distance (>= 1 unless equal, which never decides
  differently)."""
import numpy as np

ULP = 2.0 ** -23
BOUNDS = {"conf": 64 * ULP, "score": 64 * ULP, "iou": 64 * ULP, "area": 64 * ULP}
YOLOV3_ANCHORS = [[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]]


# fp32 roundings on the way from a raw head value to a corner c -+ size / 2, each at most one ulp of a quantity no larger than
# |c| + size / 2 = the far corner: sigmoid (expf <= 2, add, divide) 4, + cell 1, * stride 1 -> 6 ulp of |c|;  expf <= 2, * anchor 1,
# * stride 1 -> 4 ulp of size / 2 (the halving is exact);  the final subtraction 1.  6 |c| + 4 size / 2 + (|c| + size / 2) <=
# 7 (|c| + size / 2): DECODE_ULPS = 8 leaves one for the float64 restatement's own rounding of the fp32-rounded anchor ratio.
DECODE_ULPS = 8


def corner_bound(n, row):
    """The issue's bound for a row merged from n boxes: twice the fp32 bound of a weighted mean of n terms in any order."""
    return (n + 4) * ULP * float(np.max(np.abs(row[:4])))


def decode_bound(rows):
    """Per row [.., 7] -> [.., 2]: the decode's error bound of the x corners and of the y corners (see DECODE_ULPS)."""
    rows = np.asarray(rows, np.float64)
    return DECODE_ULPS * ULP * np.stack([np.abs(rows[..., [0, 2]]).max(-1), np.abs(rows[..., [1, 3]]).max(-1)], -1)


# ------------------------------------------------------------------------------------------------------ preprocessing
def detect_scale(width):
    return 1 if width in (256, 320) else 2


def np_detect_input(frames, S=416):
    """frames [B,C,H,W] -> ([B,C,S,S], scale, (h, w)): nearest x scale, zero pad right / bottom, crop beyond S."""
    B, C, H, W = frames.shape
    s = detect_scale(W)
    up = frames.repeat(s, axis=2).repeat(s, axis=3)
    out = np.zeros((B, C, S, S), frames.dtype)
    h, w = min(S, H * s), min(S, W * s)
    out[:, :, :h, :w] = up[:, :, :h, :w]
    return out, s, (H * s, W * s)


# ------------------------------------------------------------------------------------------------------------- decode
def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def np_decode(heads, anchors, C, img_size):
    """Raw head maps [N, A*(5+C), g, g] -> [N, boxes, 5+C] float64 = (cx, cy, w, h, conf, classes...), boxes ordered head,
    anchor, row, column (YOLOLayer.forward + the concatenation of Darknet.forward)."""
    outs = []
    for head, anc in zip(heads, anchors):
        N, _, g, _ = head.shape
        A = len(anc)
        p = head.astype(np.float64).reshape(N, A, 5 + C, g, g).transpose(0, 1, 3, 4, 2)
        stride = img_size / g
        aw = np.array([np.float32(a[0] / stride) for a in anc], np.float64).reshape(1, A, 1, 1)
        ah = np.array([np.float32(a[1] / stride) for a in anc], np.float64).reshape(1, A, 1, 1)
        gx = np.arange(g, dtype=np.float64).reshape(1, 1, 1, g)
        gy = np.arange(g, dtype=np.float64).reshape(1, 1, g, 1)
        box = np.stack([(sigmoid(p[..., 0]) + gx) * stride, (sigmoid(p[..., 1]) + gy) * stride,
                        np.exp(p[..., 2]) * aw * stride, np.exp(p[..., 3]) * ah * stride], -1)
        outs.append(np.concatenate([box, sigmoid(p[..., 4:])], -1).reshape(N, A * g * g, 5 + C))
    return np.concatenate(outs, 1)


def np_candidates(pred, conf_thres=0.5):
    """One image's decoded boxes [boxes, 5+C] -> rows [n, 7] in box order, score [n], margins."""
    conf = pred[:, 4]
    keep = conf >= conf_thres
    margin = {"conf": float(np.min(np.abs(conf - conf_thres))) if conf.size else np.inf}
    p = pred[keep]
    cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    cls = np.argmax(p[:, 5:], 1) if p.size else np.zeros(0, np.int64)
    cc = p[np.arange(p.shape[0]), 5 + cls] if p.size else np.zeros(0)
    rows = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, p[:, 4], cc, cls.astype(np.float64)], 1)
    return rows, p[:, 4] * cc, margin


def iou_one_to_many(b, B):
    iw = np.clip(np.minimum(b[2], B[:, 2]) - np.maximum(b[0], B[:, 0]) + 1, 0, None)
    ih = np.clip(np.minimum(b[3], B[:, 3]) - np.maximum(b[1], B[:, 1]) + 1, 0, None)
    inter = iw * ih
    a1 = (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
    a2 = (B[:, 2] - B[:, 0] + 1) * (B[:, 3] - B[:, 1] + 1)
    return inter / (a1 + a2 - inter + 1e-16)


def np_nms(rows, score, nms_thres=0.4):
    """non_max_suppression's loop with a stable descending sort -> dets [k, 7], merged [k] (boxes merged into each row), margins."""
    order = np.argsort(-score, kind="stable")
    s = score[order]
    margin = {"score": float(np.min(-np.diff(s))) if s.size > 1 else np.inf, "iou": np.inf, "corner": np.inf}
    d = rows[order].copy()
    alive = np.ones(d.shape[0], bool)
    out, merged = [], []
    head = 0
    n = d.shape[0]
    while head < n:
        idx = head + np.flatnonzero(alive[head:])
        iou = iou_one_to_many(d[head], d[idx])
        same = d[idx, 6] == d[head, 6]
        if same.any():
            margin["iou"] = min(margin["iou"], float(np.min(np.abs(iou[same] - nms_thres))))
        inv = idx[(iou > nms_thres) & same]
        w = d[inv, 4:5]
        row = d[head].copy()
        row[:4] = (w * d[inv, :4]).sum(0) / w.sum()
        out.append(row)
        merged.append(inv.size)
        margin["corner"] = min(margin["corner"], corner_margin(row, inv.size))
        alive[inv] = False
        alive[head] = False
        rest = np.flatnonzero(alive[head:])
        head = head + rest[0] if rest.size else n
    return (np.stack(out) if out else np.zeros((0, 7))), np.array(merged, np.int64), margin


def corner_margin(row, n):
    """Distance of the row's corners to the nearest integer (and so to 0) as the RATIO distance / (merge bound + decode bound),
    so that one number covers rows of different n; margins_ok wants it above 1."""
    c = row[:4]
    dist = float(np.min(np.abs(c - np.round(c))))
    return dist / (corner_bound(n, row) + float(decode_bound(row).max()))


def np_detect(heads, anchors, C, img_size, conf_thres=0.5, nms_thres=0.4):
    """Everything after the network for a batch -> list of (dets, merged) per image and the merged margins."""
    pred = np_decode(heads, anchors, C, img_size)
    res, margin = [], {"conf": np.inf, "score": np.inf, "iou": np.inf, "corner": np.inf}
    for n in range(pred.shape[0]):
        rows, score, m1 = np_candidates(pred[n], conf_thres)
        dets, merged, m2 = np_nms(rows, score, nms_thres)
        res.append((dets, merged, rows))
        for k, v in {**m1, **m2}.items():
            margin[k] = min(margin[k], v)
    return res, margin


def margins_ok(margin):
    """The precondition of the GPU tests."""
    bad = {k: v for k, v in margin.items() if v <= (1.0 if k == "corner" else BOUNDS.get(k, 0.0))}
    return not bad, bad


# -------------------------------------------------------------------------------------------------------------- match
def _trunc(v):
    return int(np.trunc(v))


def np_best(dets, roi_int, min_area, margin):
    ymin, xmin, ymax, xmax = roi_int
    hw = (ymax - ymin + 1) * (xmax - xmin + 1)
    best, box = -1, None
    for x1, y1, x2, y2 in np.asarray(dets, np.float64)[:, :4]:
        if not (x1 > 0 and y1 > 0 and x2 > 0 and y2 > 0):
            continue
        iy1, ix1, iy2, ix2 = _trunc(y1), _trunc(x1), _trunc(y2), _trunc(x2)
        dx = min(xmax, ix2) - max(xmin, ix1)
        dy = min(ymax, iy2) - max(ymin, iy1)
        if dx < 0 or dy < 0:
            continue
        margin["overlap"] = min(margin["overlap"], abs(2 * dx * dy - hw))
        if 2 * dx * dy <= hw:
            continue
        area = (y2 - y1) * (x2 - x1)
        margin["area"] = min(margin["area"], abs(area - min_area) / min_area)
        if area < min_area:
            continue
        if dx * dy > best:
            best, box = dx * dy, [iy1, ix1, iy2, ix2]
    return box


def np_match(dets_gt, dets_pred, index, roi, x, batch, scale, size):
    """compute_detection's per-object part.  dets_gt / dets_pred: per image an [k, 7] array (k may be 0).  roi [nodes, T, 4]
    float32, x [nodes, t_in, F] float32.  Returns per-object arrays and the reference's four lists."""
    h, w = size
    margin = {"overlap": np.inf, "area": np.inf, "skip": np.inf}
    M = len(index)
    flags, boxes, err = np.zeros((M, 3), np.int32), np.zeros((M, 8), np.int32), np.zeros((M, 2))
    f32 = np.float32
    for m, i in enumerate(index):
        b = int(batch[i])
        r = (roi[i, -1].astype(f32) * f32(scale)).astype(f32)
        xmin, xmax, ymin, ymax = (_trunc(v) for v in r)
        margin["skip"] = min(margin["skip"], abs((ymax - ymin) * (xmax - xmin) - 0.005 * w * h))
        if (ymax - ymin) * (xmax - xmin) < 0.005 * w * h:
            flags[m, 0] = 1
            continue
        g = np_best(dets_gt[b], (ymin, xmin, ymax, xmax), h * w * 0.01, margin) if len(dets_gt[b]) else None
        if g is None:
            continue
        flags[m, 1] = 1
        boxes[m, :4] = g
        p = np_best(dets_pred[b], (ymin, xmin, ymax, xmax), h * w * 0.01, margin) if len(dets_pred[b]) else None
        if p is None:
            continue
        flags[m, 2] = 1
        boxes[m, 4:] = p
        xn = x[i, -1].astype(f32)
        sy = _trunc((xn[0] + f32(1)) / f32(2) * f32(h))
        sx = _trunc((xn[1] + f32(1)) / f32(2) * f32(w))
        gy, gx = (ymin + ymax) / 2, (xmin + xmax) / 2
        py, px = (p[0] + p[2]) / 2, (p[1] + p[3]) / 2
        mse = np.sqrt((py - gy) ** 2 + (px - gx) ** 2)
        nf = np.sqrt((sy - gy) ** 2 + (sx - gx) ** 2)
        nf = nf if nf > 0 else 1
        err[m] = (mse, mse / (nf + 1e-06))
    found = flags[:, 2] == 1
    lists = {"mse_batch": err[found, 0].tolist(), "mse_normalized_batch": err[found, 1].tolist(),
             "gt_detected_images": [1] * int(flags[:, 1].sum()), "pred_detected_images": [1] * int(found.sum())}
    return flags, boxes, err, lists, margin


# -------------------------------------------------------------------------------------------------------------- score
def np_score(gt_detected, pred_detected):
    """Evaluator.generate_metrics: pad, binary F1, accuracy."""
    pred = list(pred_detected) + [0] * (len(gt_detected) - len(pred_detected))
    t, p = np.asarray(gt_detected), np.asarray(pred)
    tp, fp, fn = int(((t == 1) & (p == 1)).sum()), int(((t != 1) & (p == 1)).sum()), int(((t == 1) & (p != 1)).sum())
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return f1, float((t == p).mean()) if t.size else float("nan")


# ------------------------------------------------------------------------------------------------------------ planting
def logit(p):
    return np.log(p) - np.log1p(-p)


def plant(N, C, grids, anchors, img_size, specs, background=-7.0):
    """Raw head maps holding exactly the boxes of `specs`: per image a list of dicts {box: index in box order, cx, cy, w, h
    (pixels; cx, cy inside the box's cell), conf, cls, cls_conf}.  Everything else sits at `background` (conf 0.0009).
    Values are computed in float64 and rounded to fp32 once; the restatement decodes the ROUNDED maps."""
    heads = [np.full((N, len(a) * (5 + C), g, g), background, np.float64) for g, a in zip(grids, anchors)]
    starts = np.cumsum([0] + [len(a) * g * g for g, a in zip(grids, anchors)])
    for n, boxes in enumerate(specs):
        for s in boxes:
            h = int(np.searchsorted(starts, s["box"], side="right") - 1)
            g, anc = grids[h], anchors[h]
            r = s["box"] - starts[h]
            a, gy, gx = r // (g * g), (r // g) % g, r % g
            stride = img_size / g
            v = heads[h][n, a * (5 + C):(a + 1) * (5 + C), gy, gx]
            fx, fy = s["cx"] / stride - gx, s["cy"] / stride - gy
            assert 0 < fx < 1 and 0 < fy < 1, "a planted centre lies inside its cell"
            v[0], v[1] = logit(fx), logit(fy)
            v[2], v[3] = np.log(s["w"] / anc[a][0]), np.log(s["h"] / anc[a][1])
            v[4] = logit(s["conf"])
            v[5:] = logit(0.02)
            v[5 + s["cls"]] = logit(s["cls_conf"])
    return [h.astype(np.float32) for h in heads]


def cell_of(box, grids, anchors):
    """(head, anchor, gy, gx, stride fraction helper) of a box index."""
    starts = np.cumsum([0] + [len(a) * g * g for g, a in zip(grids, anchors)])
    h = int(np.searchsorted(starts, box, side="right") - 1)
    g = grids[h]
    r = box - starts[h]
    return h, r // (g * g), (r // g) % g, r % g


def lattice_conf(n, rng, lo=0.55, hi=0.95):
    """n distinct confidences, evenly spaced and shuffled: adjacent scores differ by (hi - lo) / n times the class confidence."""
    return lo + (hi - lo) * (rng.permutation(n) + 0.5) / n


# -------------------------------------------------------------------------------------------------------- planted cases
S_SMALL = 96
GRIDS_SMALL = [3, 6, 12]                      # 27 + 108 + 432 = 567 boxes, one odd grid


def _spec(box, grids, anchors, img_size, w, h, conf, cls, frac=(0.3, 0.3), cls_conf=0.9):
    hd, a, gy, gx = cell_of(box, grids, anchors)
    stride = img_size / grids[hd]
    return {"box": int(box), "cx": (gx + frac[0]) * stride, "cy": (gy + frac[1]) * stride, "w": w, "h": h, "conf": float(conf),
            "cls": int(cls), "cls_conf": cls_conf}


def small_cases(C):
    """name -> (heads, C): B = 2 at S = 96.  Built once per C (lru-cached by the callers)."""
    A, G, S = YOLOV3_ANCHORS, GRIDS_SMALL, S_SMALL
    nb = sum(len(a) * g * g for g, a in zip(G, A))
    out = {}
    # random boxes, random classes, anchor-sized; the second image has no candidate
    rng = np.random.default_rng(130 + C)
    pick = rng.choice(nb, 120, replace=False)
    conf = lattice_conf(pick.size, rng)
    specs = []
    for b, cf in zip(pick, conf):
        hd, a, _, _ = cell_of(b, G, A)
        specs.append(_spec(b, G, A, S, A[hd][a][0] * rng.uniform(0.15, 0.5), A[hd][a][1] * rng.uniform(0.15, 0.5), cf,
                           rng.integers(C), frac=tuple(rng.uniform(0.2, 0.8, 2))))
    out["random_and_empty"] = plant(2, C, G, A, S, [specs, []])
    # every box passes; three anchors per cell share one small box: same-class anchors of a cell merge, nothing else does
    rng = np.random.default_rng(200 + C)
    conf = lattice_conf(2 * nb, rng)
    specs = [[_spec(b, G, A, S, 3.3, 3.3, conf[n * nb + b], rng.integers(min(C, 3))) for b in range(nb)] for n in range(2)]
    out["all_pass"] = plant(2, C, G, A, S, specs)
    if C != 3:
        return out
    start2 = 27 + 108                                    # first box of the stride-8 head
    at = lambda a, gy, gx: start2 + (a * 12 + gy) * 12 + gx
    # one merge of everything: 12 boxes of one class, 80 px wide, centres within 8 px | A-B-C chain (40 px boxes 16 px apart)
    rng = np.random.default_rng(300)
    conf = lattice_conf(12, rng)
    one = [_spec(at(a, gy, gx), G, A, S, 80.0, 80.0, conf[(a * 2 + gy - 5) * 2 + gx - 5], 1)
           for a in range(3) for gy in (5, 6) for gx in (5, 6)]
    chain = [_spec(at(0, 3, gx), G, A, S, 40.0, 40.0, cf, 2, frac=(0.7875, 0.7875)) for gx, cf in ((3, 0.9), (5, 0.8), (7, 0.7))]
    out["one_merge_and_chain"] = plant(2, C, G, A, S, [one, chain])
    # the same box twice with different classes (both stay), next to a same-class pair (one row) | nothing
    both = [_spec(at(0, 4, 4), G, A, S, 30.0, 30.0, 0.9, 0), _spec(at(1, 4, 4), G, A, S, 30.0, 30.0, 0.8, 1),
            _spec(at(0, 8, 8), G, A, S, 20.0, 20.0, 0.7, 2), _spec(at(1, 8, 8), G, A, S, 20.0, 20.0, 0.6, 2)]
    out["classes"] = plant(2, C, G, A, S, [both, []])
    return out


def full_case():
    """10 647 boxes at S = 416, all passing, none merging: 1.3 px boxes, the three anchors of a cell in three classes."""
    A, G, S, C = YOLOV3_ANCHORS, [13, 26, 52], 416, 3
    nb = sum(len(a) * g * g for g, a in zip(G, A))
    rng = np.random.default_rng(400)
    conf = lattice_conf(nb, rng)
    specs = [[_spec(b, G, A, S, 1.3, 1.3, conf[b], cell_of(b, G, A)[1]) for b in range(nb)]]
    return plant(1, C, G, A, S, specs), C, G, S
