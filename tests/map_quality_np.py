"""The contract of evaluate.map_quality restated in numpy, one image at a time, and the cases the tests and
the fixture share.  The restatement follows the reference's formulation (cityscapesscripts' pq_compute_single_core and
Panoptic-DeepLab's SemanticEvaluator.update): np.unique over packed keys, sorted, then loops over the segments; it is held to
the reference's own results by tests/test_map_quality_cpu.py (tests/golden/map_quality_reference.npz)."""
import numpy as np

CITYSCAPES = dict(num_classes=19, thing_list=(11, 12, 13, 14, 15, 16, 17, 18), label_divisor=1000, ignore_label=255)


def canonical(v, num_classes, label_divisor, ignore_label):
    """Map values -> (cat, n, void).  v < label_divisor: (v, 0); else (v // label_divisor, v % label_divisor).  Void: negative,
    cat == ignore_label or cat >= num_classes."""
    v = np.asarray(v).astype(np.int64)
    low = v < label_divisor
    cat = np.where(low, v, v // label_divisor)
    n = np.where(low, 0, v % label_divisor)
    void = (v < 0) | (cat == ignore_label) | (cat >= num_classes)
    return cat, n, void


def keys(v, num_classes, label_divisor, ignore_label):
    """cat * label_divisor + n, and -1 on void."""
    cat, n, void = canonical(v, num_classes, label_divisor, ignore_label)
    return np.where(void, -1, cat * label_divisor + n)


def image_quality(pred, gt, num_classes=19, thing_list=CITYSCAPES["thing_list"], label_divisor=1000, ignore_label=255):
    """One image -> tp, fp, fn int32 [C], iou float64 [C], confusion int64 [C+1,C+1] ([pred, gt], void last)."""
    C, div = num_classes, label_divisor
    pk = keys(pred, C, div, ignore_label).reshape(-1)
    gk = keys(gt, C, div, ignore_label).reshape(-1)
    BIG = C * div + 1                                                          # void packs as 0, a key k as k + 1
    pairs, counts = np.unique((gk + 1) * BIG + (pk + 1), return_counts=True)   # sorted: g ascending, then p
    inter = {(int(k // BIG) - 1, int(k % BIG) - 1): int(c) for k, c in zip(pairs, counts)}
    area_p = {int(k): int(c) for k, c in zip(*np.unique(pk[pk >= 0], return_counts=True))}
    area_g = {int(k): int(c) for k, c in zip(*np.unique(gk[gk >= 0], return_counts=True))}
    crowd = lambda g: (g // div) in thing_list and g % div == 0
    tp, fp, fn = (np.zeros(C, np.int32) for _ in range(3))
    iou = np.zeros(C, np.float64)
    g_matched, p_matched = set(), set()
    for (g, p), it in inter.items():                                          # insertion order = sorted order
        if g < 0 or p < 0 or crowd(g) or g // div != p // div:
            continue
        union = area_p[p] + area_g[g] - it - inter.get((-1, p), 0)
        v = np.float64(it) / np.float64(union)
        if v > 0.5:
            tp[g // div] += 1
            iou[g // div] += v
            g_matched.add(g)
            p_matched.add(p)
    for g in area_g:
        if g not in g_matched and not crowd(g):
            fn[g // div] += 1
    for p, a in area_p.items():
        if p in p_matched:
            continue
        cg = (p // div) * div                                                  # the crowd region of p's class, if it is a thing
        ignored = inter.get((-1, p), 0) + (inter.get((cg, p), 0) if crowd(cg) else 0)
        if np.float64(ignored) / np.float64(a) > 0.5:
            continue
        fp[p // div] += 1
    pc = np.where(pk < 0, C, pk // div)
    gc = np.where(gk < 0, C, gk // div)
    conf = np.bincount((C + 1) * pc + gc, minlength=(C + 1) ** 2).reshape(C + 1, C + 1).astype(np.int64)
    return {"tp": tp, "fp": fp, "fn": fn, "iou": iou, "confusion": conf}


def batch_quality(pred, gt, **params):
    """[..., H, W] maps -> a list of per-image results, images in row-major order of the leading axes."""
    H, W = pred.shape[-2:]
    return [image_quality(p, g, **params) for p, g in zip(pred.reshape(-1, H, W), gt.reshape(-1, H, W))]


def to_panoptic(ins, label_divisor=1000, ignore_label=255):
    """The instance-id image -> the panoptic encoding of the same scene (stuff class * divisor, void ignore_label * divisor)."""
    ins = ins.astype(np.int64)
    return np.where(ins >= label_divisor, ins, ins * label_divisor).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- cases
STUFF = (0, 1, 2, 8, 10)
THINGS = CITYSCAPES["thing_list"]


def scene(rng, N, H, W, things=6):
    """N (gt, pred) instance-id images: stuff bands with a void patch, rectangles of thing classes numbered per class, one crowd
    region; the prediction is the ground truth moved by a few pixels per object, one object renumbered, one dropped, one made up."""
    gt = np.empty((N, H, W), np.int32)
    pred = np.empty((N, H, W), np.int32)
    for i in range(N):
        for m, (dy, dx) in ((gt, (0, 0)), (pred, (int(rng.integers(0, 2)), int(rng.integers(0, 3))))):
            bands = np.array(STUFF)[(np.arange(W) * len(STUFF) // max(W, 1) + i) % len(STUFF)]
            m[i] = np.roll(np.broadcast_to(bands, (H, W)), dx, axis=1)
            m[i, : max(H // 3, 1)] = 10                                        # sky
        gt[i, H // 2: H // 2 + max(H // 8, 1), : max(W // 5, 1)] = 255         # void patch
        if H > 4 and W > 12:
            gt[i, H - 3:, W // 2: W // 2 + 9] = 11000                          # a crowd of persons
        count = {}
        r2 = np.random.default_rng(1000 + i)
        for k in range(things):
            c = int(THINGS[int(rng.integers(0, len(THINGS)))])
            count[c] = count.get(c, 0) + 1
            h, w = int(rng.integers(1, max(H // 3, 2))), int(rng.integers(1, max(W // 4, 2)))
            y, x = int(rng.integers(0, max(H - h, 1))), int(rng.integers(0, max(W - w, 1)))
            gt[i, y:y + h, x:x + w] = c * 1000 + count[c]
            if k == 1:
                continue                                                       # dropped from the prediction
            sy, sx = int(r2.integers(-1, 2)), int(r2.integers(-2, 3))
            y2, x2 = min(max(y + sy, 0), H - 1), min(max(x + sx, 0), W - 1)
            pred[i, y2:y2 + h, x2:x2 + w] = c * 1000 + (count[c] if k != 2 else 900 + k)
        pred[i, 0:1, 0:1] = 18999                                              # made up, one pixel, the largest n
        if H > 8:
            pred[i, H // 2 + 1, 1: max(W // 6, 2)] = 255
    return pred, gt


def _rect(m, y, x, h, w, v):
    m[y:y + h, x:x + w] = v


def crafted():
    """12 x 40 images, one property each (pred, gt), in the order of the list in the head of tests/test_gpu_map_quality.py."""
    H, W = 12, 40
    P, G = [], []

    def new():
        p, g = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)         # road everywhere
        P.append(p)
        G.append(g)
        return p, g

    p, g = new()                       # 0: IoU exactly 0.5: areas 75 and 75, 50 in common, union 100 -> no match: fn 1, fp 1
    _rect(g, 0, 0, 5, 15, 13001); _rect(p, 0, 5, 5, 15, 13001)
    p, g = new()                       # 1: 76 and 76, 51 in common, union 101 -> match
    _rect(g, 0, 0, 5, 15, 13001); _rect(p, 0, 5, 5, 15, 13001); g[5, 0] = p[5, 0] = 13001
    p, g = new()                       # 2: a predicted car of 40 pixels, 20 of them on void: counted as fp
    _rect(p, 2, 2, 4, 10, 13001); _rect(g, 2, 2, 4, 5, 255)
    p, g = new()                       # 3: 21 of 40 on void: ignored
    _rect(p, 2, 2, 4, 10, 13001); _rect(g, 2, 2, 4, 5, 255); g[2, 7] = 255
    p, g = new()                       # 4: 20 of 40 on the crowd region of cars: fp
    _rect(p, 2, 2, 4, 10, 13001); _rect(g, 2, 2, 4, 5, 13000)
    p, g = new()                       # 5: 21 of 40 on the crowd region of cars: ignored
    _rect(p, 2, 2, 4, 10, 13001); _rect(g, 2, 2, 4, 5, 13000); g[2, 7] = 13000
    p, g = new()                       # 6: 30 of 40 on a crowd of PERSONS: that excuses no car -> fp
    _rect(p, 2, 2, 4, 10, 13001); _rect(g, 2, 2, 3, 10, 11)                   # 11 below the divisor: (11, 0) as well
    p, g = new()                       # 7: a predicted (13, 0) exactly on the crowd region (13, 0): no tp, no fn, no fp
    _rect(p, 2, 2, 4, 10, 13000); _rect(g, 2, 2, 4, 10, 13000)
    p, g = new()                       # 8: the same n in two classes, and n = label_divisor - 1
    _rect(g, 0, 0, 4, 6, 11001); _rect(g, 0, 10, 4, 6, 13001); _rect(g, 6, 0, 4, 6, 13999); _rect(g, 6, 10, 4, 6, 11999)
    _rect(p, 0, 0, 4, 6, 11001); _rect(p, 0, 11, 4, 6, 13001); _rect(p, 6, 0, 4, 6, 13999); _rect(p, 6, 20, 4, 6, 11999)
    p, g = new()                       # 9: all void on both sides
    p[:] = 255; g[:] = 255
    p, g = new()                       # 10: void by three routes (negative, a class past num_classes, 255000) and void under a match
    _rect(g, 0, 0, 6, 10, 14002); _rect(p, 0, 0, 6, 12, 14007); _rect(g, 0, 10, 6, 2, 255)
    p[8, :10] = -5; p[9, :10] = 19; p[10, :10] = 255000; g[8, 20:30] = 25003; g[9, 20:30] = 999
    return np.stack(P), np.stack(G)


def hash_load():
    """Three 64 x 64 frames; in the middle one every pixel is its own thing on both sides: 4096 pairs of equal class."""
    rng = np.random.default_rng(77)
    pred, gt = scene(rng, 3, 64, 64)
    i = np.arange(64 * 64)
    full = ((11 + i % 8) * 1000 + 1 + i // 8).astype(np.int32).reshape(64, 64)
    pred[1], gt[1] = full, full.copy()
    return pred, gt


def cases():
    """name -> dict(pred, gt, params): maps with the leading axes the call is made with ([N], [B,T] or [B,1,T])."""
    rng = np.random.default_rng(2024)
    out = {}
    one = np.full((1, 1, 1), 11001, np.int32)
    out["px_1x1"] = dict(pred=one, gt=one.copy(), params={})
    p, g = scene(rng, 3, 7, 300)
    out["rows_7x300"] = dict(pred=p, gt=g, params={})
    out["rows_7x300_panoptic"] = dict(pred=to_panoptic(p), gt=to_panoptic(g), params={})
    p, g = scene(rng, 6, 33, 65)
    out["clip_33x65"] = dict(pred=p.reshape(2, 3, 33, 65), gt=g.reshape(2, 3, 33, 65), params={})
    p, g = scene(rng, 3, 129, 257, things=14)
    out["clip5d_129x257"] = dict(pred=p.reshape(1, 1, 3, 129, 257), gt=g.reshape(1, 1, 3, 129, 257), params={})
    p, g = scene(rng, 1, 129, 257, things=10)
    out["single_129x257"] = dict(pred=p, gt=g, params={})
    p, g = crafted()
    out["crafted"] = dict(pred=p, gt=g, params={})
    p, g = scene(rng, 1, 33, 65)
    lab = lambda m: np.where(m >= 1000, m // 1000, m).astype(np.uint8)
    p, g = lab(p), lab(g)
    p[0, 5, 5:9] = 200                                                         # a class past num_classes: void
    out["labels_u8_33x65"] = dict(pred=p, gt=g, params={})
    p, g = hash_load()
    out["hash_64x64"] = dict(pred=p, gt=g, params=dict(max_pairs=4096))
    p, g = scene(rng, 2, 20, 31)
    small = lambda m: np.where(m == 255, 255 * 64, np.where(m >= 1000, (m // 1000) * 64 + m % 1000 % 63 + 1, m)).astype(np.int32)
    out["divisor_64"] = dict(pred=small(p), gt=small(g), params=dict(label_divisor=64, num_classes=21, thing_list=(11, 12, 13, 19),
                                                                     ignore_label=255))
    return out


def walk_cases():
    """Cases for the count kernel's tile walk, held to the restatement alone (too many frames for the fixture): the kernel
    launches at most 1024 workgroups over all frames, so with 600 frames of 33 x 65 (2145 pixels, two tiles of 2048) one
    workgroup per frame walks both tiles with one LDS pair table, and with 1100 frames the cap falls below one workgroup per
    frame and is clamped to one.  A small divisor keeps the per-frame tables small."""
    small = lambda m: np.where(m == 255, 255 * 64, np.where(m >= 1000, (m // 1000) * 64 + m % 1000 % 63 + 1, m)).astype(np.int32)
    params = dict(label_divisor=64, num_classes=21, thing_list=(11, 12, 13, 19), ignore_label=255, max_pairs=1024)
    out = {}
    p, g = scene(np.random.default_rng(600), 24, 33, 65)
    idx = np.arange(600) % 24
    p, g = small(p)[idx], small(g)[idx]
    p[np.arange(600), 32, 64] = 13 * 64 + 1 + np.arange(600) % 60             # the last pixel, in the second tile, differs per frame
    out["walk_600x33x65"] = dict(pred=p, gt=g, params=params)
    p, g = scene(np.random.default_rng(1100), 20, 3, 5, things=2)
    idx = np.arange(1100) % 20
    p, g = small(p)[idx], small(g)[idx]
    g[np.arange(1100), 0, 0] = 12 * 64 + 1 + np.arange(1100) % 50
    out["clamp_1100x3x5"] = dict(pred=p, gt=g, params=params)
    return out


def restatement_params(params):
    """The parameters image_quality takes (max_pairs belongs to the kernel's table alone)."""
    return {**CITYSCAPES, **{k: v for k, v in params.items() if k != "max_pairs"}}
