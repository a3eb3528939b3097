"""The contract of evaluate.tube_quality and tracking.anchor_maps restated in numpy, and the cases the tests
and the fixture share.  A window's score is map_quality_np.image_quality -- the restatement of the reference's
pq_compute_single_core -- on the window's k frames stacked into one image of k * H rows; it is held to the reference's own
results on the stacked windows by tests/test_tube_quality_cpu.py (tests/golden/tube_quality_reference.npz)."""
import numpy as np

import map_quality_np as M

FIELDS = ("tp", "fp", "fn", "iou")


def restatement_params(params):
    return M.restatement_params(params)


def windows_of(T, k):
    return [(t0, k) for t0 in range(T - k + 1)]


def window_quality(pred, gt, **params):
    """One window, [k,H,W] maps -> tp, fp, fn int32 [C], iou float64 [C]: the k frames as one image of k * H rows."""
    k, H, W = pred.shape
    r = M.image_quality(pred.reshape(k * H, W), gt.reshape(k * H, W), **params)
    return {f: r[f] for f in FIELDS}


def clip_quality(pred, gt, k, **params):
    """[B,T,H,W] clips -> dict of arrays [B, T-k+1, C] for window length k; a window never crosses a clip."""
    B, T = pred.shape[:2]
    rows = [[window_quality(pred[b, t0:t0 + k], gt[b, t0:t0 + k], **params) for t0 in range(T - k + 1)] for b in range(B)]
    return {f: np.stack([np.stack([w[f] for w in row]) for row in rows]) for f in FIELDS}


def window_pairs(pred, gt, num_classes=19, thing_list=M.CITYSCAPES["thing_list"], label_divisor=1000, ignore_label=255):
    """The number of distinct (g, p) pairs of one window that go through the pair table: both non-void, of one class, g no crowd
    region."""
    pk = M.keys(pred, num_classes, label_divisor, ignore_label).reshape(-1)
    gk = M.keys(gt, num_classes, label_divisor, ignore_label).reshape(-1)
    ok = (pk >= 0) & (gk >= 0) & (pk // label_divisor == gk // label_divisor)
    ok &= ~(np.isin(gk // label_divisor, thing_list) & (gk % label_divisor == 0))
    return len(np.unique(gk[ok].astype(np.int64) * (num_classes * label_divisor + 1) + pk[ok]))


def id_quality(pred, gt, ids, num_classes=19, thing_list=M.CITYSCAPES["thing_list"], label_divisor=1000, ignore_label=255):
    """One window [k,H,W] and a list of map values -> (id_iou float64 [M], id_gt_area int32 [M], id_pred_area int32 [M]).
    -1.0 for padding (negative), a void value, a ground-truth crowd key and a key without ground-truth pixels in the window;
    else inter / union with inter the pixels holding the key in both maps and union = area_p + area_g - inter - void_p."""
    pk = M.keys(pred, num_classes, label_divisor, ignore_label).reshape(-1)
    gk = M.keys(gt, num_classes, label_divisor, ignore_label).reshape(-1)
    iou = np.full(len(ids), -1.0, np.float64)
    ga, pa = np.zeros(len(ids), np.int32), np.zeros(len(ids), np.int32)
    for m, v in enumerate(ids):
        if v < 0:
            continue
        g = int(M.keys(np.array([v]), num_classes, label_divisor, ignore_label)[0])
        if g < 0 or (g // label_divisor in thing_list and g % label_divisor == 0):
            continue
        ga[m], pa[m] = int((gk == g).sum()), int((pk == g).sum())
        if ga[m] == 0:
            continue
        inter = int(((gk == g) & (pk == g)).sum())
        union = int(pa[m]) + int(ga[m]) - inter - int(((pk == g) & (gk < 0)).sum())
        iou[m] = np.float64(inter) / np.float64(union)
    return iou, ga, pa


def clip_id_quality(pred, gt, ids, k, **params):
    """[B,T,H,W] clips and ids [B,M] -> id_iou, id_gt_area, id_pred_area [B, T-k+1, M]."""
    B, T = pred.shape[:2]
    rows = [[id_quality(pred[b, t0:t0 + k], gt[b, t0:t0 + k], ids[b], **params) for t0 in range(T - k + 1)] for b in range(B)]
    return tuple(np.stack([np.stack([w[i] for w in row]) for row in rows]) for i in range(3))


def relabel(maps, pairs_from, pairs_to, count, thing_list=M.CITYSCAPES["thing_list"], label_divisor=1000):
    """tracking.anchor_maps' rule per plane: maps [P,H,W]; pairs [P,n]; the first count[p] pairs of plane p hold.  A value equal
    to a `from` becomes its `to` (looked up by the OLD value only); every other thing value becomes its class's crowd id."""
    out = np.empty_like(maps)
    for p in range(maps.shape[0]):
        v = maps[p].astype(np.int64)
        cat = v // label_divisor
        res = np.where((v >= label_divisor) & np.isin(cat, thing_list), cat * label_divisor, v)
        for i in range(int(count[p])):
            res[v == int(pairs_from[p][i])] = int(pairs_to[p][i])
        out[p] = res.astype(maps.dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
def _rect(m, y, x, h, w, v):
    m[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = v


def _ground(B, T, H, W):
    """Stuff bands (road, sky, vegetation) that do not move, for both maps."""
    g = np.zeros((B, T, H, W), np.int32)
    g[:, :, : H // 4] = 10
    g[:, :, :, W - W // 5:] = 8
    return g


def clips(H=24, W=40):
    """[2,5,H,W]: objects that keep their id while they move, one property each; see the head of tests/test_gpu_tube_quality.py."""
    B, T = 2, 5
    gt = _ground(B, T, H, W)
    pred = gt.copy()
    pred[:, :, H // 4] = 10                                                   # the sky one row too deep: stuff IoU below 1
    for b in range(B):
        for t in range(T):
            # a car in every frame, the prediction one pixel off
            _rect(gt[b, t], 8, 2 + 2 * t + b, 5, 7, 13001); _rect(pred[b, t], 8, 3 + 2 * t + b, 5, 7, 13001)
            # a person that is there in frames 2.. only (an id present in some frames of a window)
            if t >= 2:
                _rect(gt[b, t], 15, 20 + t, 6, 3, 11001); _rect(pred[b, t], 15, 20 + t, 6, 3, 11001)
            # a rider the prediction does not have (id_iou 0.0) and a made-up bicycle
            _rect(gt[b, t], 16, 30, 3, 3, 12001)
            _rect(pred[b, t], 20, 1 + t, 2, 2, 18007)
    # step 4: a predicted truck, 12 pixels per frame; in frame 1 of clip 0 ten of them lie on void, so alone (k = 1) it is
    # ignored there, while over a window of two or more frames less than half of the tube is on void: it counts as fp
    for t in range(T):
        _rect(pred[0, t], 19, 10, 3, 4, 14001)
    _rect(gt[0, 1], 19, 10, 3, 4, 255); gt[0, 1, 19, 10:12] = 0
    # a ground-truth crowd region of cars in frame 3 of clip 1 only, under a predicted car of 8 pixels per frame (frames 2..4)
    for t in (2, 3, 4):
        _rect(pred[1, t], 20, 12, 2, 4, 13002)
    _rect(gt[1, 3], 20, 12, 2, 4, 13000)
    # the clip border: car 13005 is real and predicted in the LAST frame of clip 0, and only predicted, elsewhere and larger, in
    # the FIRST frame of clip 1: a window that leaked across the border would lose the match of clip 0 / add pixels to clip 1's
    _rect(gt[0, T - 1], 21, 30, 2, 4, 13005); _rect(pred[0, T - 1], 21, 30, 2, 4, 13005)
    _rect(pred[1, 0], 13, 1, 3, 6, 13005)
    return pred, gt


def id_swap(H=12, W=24, T=4, at=2):
    """Two cars of equal area that move; from frame `at` on the prediction carries each one's id on the other."""
    gt = _ground(1, T, H, W)
    pred = gt.copy()
    for t in range(T):
        a, b = (13001, 13002) if t < at else (13002, 13001)
        _rect(gt[0, t], 4, 1 + t, 3, 4, 13001); _rect(gt[0, t], 8, 10 + t, 3, 4, 13002)
        _rect(pred[0, t], 4, 1 + t, 3, 4, a); _rect(pred[0, t], 8, 10 + t, 3, 4, b)
    return pred, gt


def pair_frames(per_frame, H=4, W=8):
    """[1,T,H,W] all void but, in frame t, per_frame[t] single-pixel cars (the ids listed) at the same place in both maps: every
    one is one pair of the table."""
    T = len(per_frame)
    gt = np.full((1, T, H, W), 255, np.int32)
    for t, ids in enumerate(per_frame):
        assert len(ids) <= H * W
        gt[0, t].reshape(-1)[:len(ids)] = ids
    return gt.copy(), gt


def cases():
    """name -> dict(pred, gt [B,T,H,W], windows, params[, ids [B,M]])."""
    out = {}
    p, g = clips()
    ids = np.array([[13001, -1, 11001, 11000, 12001, 255, 13005, 14001],      # padding, crowd id, pred lacks 12001, void, absent 14001
                    [13001, 11001, 13005, 13002, -7, 18007, 12001, 0]], np.int32)
    out["clips_24x40"] = dict(pred=p, gt=g, windows=(1, 2, 3, 5), params={}, ids=ids)
    p, g = clips(23, 37)                                                       # W % 4 != 0, H * W odd
    out["odd_23x37"] = dict(pred=p[:1, :3].copy(), gt=g[:1, :3].copy(), windows=(3, 1, 2), params={}, ids=ids[:1, :5].copy())
    out["single_frame"] = dict(pred=p[:, 2:3].copy(), gt=g[:, 2:3].copy(), windows=(1,), params={})
    lab = lambda m: np.where(m >= 1000, m // 1000, m).astype(np.uint8)
    p, g = clips()
    out["labels_u8"] = dict(pred=lab(p[:1, :3]), gt=lab(g[:1, :3]), windows=(1, 3), params={})
    p, g = id_swap()
    out["id_swap"] = dict(pred=p, gt=g, windows=(1, 2, 3, 4), params={}, ids=np.array([[13001, 13002]], np.int32))
    car = lambda *n: [13000 + i for i in n]
    p, g = pair_frames([car(1, 2, 3, 4), car(5, 6, 7, 8), car(8), car(1)])   # window (0, 1) of k = 2: exactly 8 pairs
    out["pairs_exact"] = dict(pred=p, gt=g, windows=(1, 2), params=dict(max_pairs=8))
    p, g = pair_frames([car(1, 2, 3, 4), car(5, 6, 7, 8, 9), car(8), car(1)])  # ... 9 pairs: that window alone overflows
    out["pairs_over"] = dict(pred=p, gt=g, windows=(1, 2), params=dict(max_pairs=8))
    p, g = pair_frames([car(1), car(*range(1, 10)), car(2), car(3)])           # frame 1 overflows on its own
    out["pairs_frame_over"] = dict(pred=p, gt=g, windows=(1, 2, 4), params=dict(max_pairs=8))
    return out


OVERFLOW_CASES = ("pairs_over", "pairs_frame_over")


def expected_overflow(case):
    """{k: bool [B, T-k+1]}: a window overflows when it has more pairs than max_pairs or one of its frames has."""
    p = restatement_params(case["params"])
    cap = case["params"].get("max_pairs", 65536)
    B, T = case["pred"].shape[:2]
    frame = np.array([[window_pairs(case["pred"][b, t], case["gt"][b, t], **p) > cap for t in range(T)] for b in range(B)])
    out = {}
    for k in case["windows"]:
        out[k] = np.array([[window_pairs(case["pred"][b, t0:t0 + k], case["gt"][b, t0:t0 + k], **p) > cap or
                            frame[b, t0:t0 + k].any() for t0 in range(T - k + 1)] for b in range(B)])
    return out


def relabel_cases():
    """name -> dict(maps [P,H,W], pairs_from, pairs_to [P,n], count [P]) for the relabel kernel."""
    rng = np.random.default_rng(5)
    out = {}

    def plane(H, W, values):
        return rng.choice(np.array(values, np.int32), (H, W)).astype(np.int32)

    vals = [0, 7, 255, 24001, -3, 13001, 13002, 13003, 11001, 11002, 14500, 300000]
    # a swap of two ids; 13003 is unlinked and EQUALS the anchor id node 11001 maps to; 11002 unlinked; 14500 -> 14001
    m = np.stack([plane(9, 40, vals), plane(9, 40, vals)])
    out["swap_9x40"] = dict(maps=m, pairs_from=np.array([[13002, 13001, 11001, 14500], [13001, 0, 0, 0]]),
                            pairs_to=np.array([[13001, 13002, 13003, 14001], [13002, 0, 0, 0]]), count=np.array([4, 1]))
    # W % 4 != 0, more than one strip of the scalar kernel (2048 pixels), count 0 and count 64
    many = [(11 + i % 8) * 1000 + 1 + i for i in range(64)]
    m = np.stack([plane(57, 37, vals + many[:8]), plane(57, 37, many + [0, 255, 16900])])
    frm = np.array([[0] * 64, many[::-1]])
    to = np.array([[0] * 64, [(v // 1000) * 1000 + 700 + i for i, v in enumerate(many[::-1])]])
    out["odd_57x37"] = dict(maps=m, pairs_from=frm, pairs_to=to, count=np.array([0, 64]))
    # more than one strip of the vector kernel (8192 pixels) and a plane smaller than one strip
    out["strips_72x128"] = dict(maps=plane(72, 128, vals + many[:20])[None], pairs_from=np.array([many[:20]]),
                                pairs_to=np.array([many[20:40]]), count=np.array([20]))
    out["tiny_2x4"] = dict(maps=plane(2, 4, vals)[None], pairs_from=np.array([[13001, 11001]]), pairs_to=np.array([[11001, 13001]]),
                           count=np.array([2]))
    return out
