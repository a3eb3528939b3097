"""Plain numpy restatement of the Panoptic-DeepLab post-processing contract, one image at a time, written from
the contract and independent of the kernels' structure: float64 distances, a loop over the centres, np.bincount for the votes.
tests/test_panoptic_cpu.py holds it to the reference's own results (tests/golden/panoptic_reference.npz); the GPU tests hold
the kernels to it.  Also the builders of the test cases, shared by the capture tool and both test files."""
import numpy as np

CITYSCAPES = dict(thing_list=(11, 12, 13, 14, 15, 16, 17, 18), label_divisor=1000, stuff_area=2048, ignore_label=255,
                  threshold=0.1, nms_kernel=7, top_k=200)


def labels_of(semantic):
    """[C,H,W] logits -> argmax, first maximum; [H,W] labels pass through."""
    semantic = np.asarray(semantic)
    return semantic.argmax(0).astype(np.int64) if semantic.ndim == 3 else semantic.astype(np.int64)


def find_centers(score, threshold, nms_kernel, top_k):
    """[H,W] fp32 -> int64 [K,2] (y, x), row-major."""
    score = np.asarray(score, np.float32)
    H, W = score.shape
    r = nms_kernel // 2
    pad = np.full((H + 2 * r, W + 2 * r), -np.inf, np.float32)
    pad[r:r + H, r:r + W] = score
    top = np.full((H, W), -np.inf, np.float32)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            top = np.maximum(top, pad[dy:dy + H, dx:dx + W])
    cand = (score > np.float32(threshold)) & (score == top)
    if cand.sum() >= top_k:
        s_k = np.sort(score[cand])[::-1][top_k - 1]
        cand &= score > s_k
    return np.argwhere(cand).astype(np.int64)


def nearest(centers, offset, chunk=64):
    """Index of the nearest centre of every pixel's (y + dy, x + dx), float64, first of equally near ones; also the two
    smallest squared distances [2,H,W] (for the near-tie mask of the unquantised case)."""
    _, H, W = offset.shape
    yy, xx = np.mgrid[0:H, 0:W]
    py = (yy.astype(np.float32) + offset[0].astype(np.float32)).astype(np.float64)      # the fp32 point, as the contract says
    px = (xx.astype(np.float32) + offset[1].astype(np.float32)).astype(np.float64)
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    arg = np.zeros((H, W), np.int64)
    for k, (cy, cx) in enumerate(centers):
        d = (cy - py) ** 2 + (cx - px) ** 2
        closer = d < best
        second = np.where(closer, best, np.minimum(second, d))
        arg = np.where(closer, k, arg)
        best = np.where(closer, d, best)
    return arg, np.stack([best, second])


def panoptic_one(semantic, center, offset, thing_list, label_divisor, stuff_area, ignore_label, threshold, nms_kernel, top_k):
    """One image.  Returns dict(semantic uint8, panoptic int32, instance int32 [H,W], centers int64 [K,2], two [2,H,W])."""
    sem = labels_of(semantic)
    H, W = sem.shape
    void = ignore_label * label_divisor
    things = sorted(set(int(c) for c in thing_list))
    is_thing = np.isin(sem, things)
    ctr = find_centers(np.asarray(center).reshape(H, W), threshold, nms_kernel, top_k)
    two = np.full((2, H, W), np.inf)
    raw = np.zeros((H, W), np.int64)
    if len(ctr):
        arg, two = nearest(ctr, np.asarray(offset))
        raw = (arg + 1) * is_thing
    pan = np.full((H, W), void, np.int64)
    used = {}
    for k in range(1, len(ctr) + 1):
        mask = raw == k
        if not mask.any():
            continue
        cls = int(np.bincount(sem[mask]).argmax())                       # ties: the smallest class
        used[cls] = used.get(cls, 0) + 1
        pan[mask] = cls * label_divisor + used[cls]
    for cls in np.unique(sem):
        if int(cls) in things:
            continue
        mask = (sem == cls) & (raw == 0)
        if mask.sum() >= stuff_area:
            pan[mask] = int(cls) * label_divisor
    cls_of = pan // label_divisor
    ins = np.where(np.isin(cls_of, things), pan, cls_of)
    return dict(semantic=sem.astype(np.uint8), panoptic=pan.astype(np.int32), instance=ins.astype(np.int32), centers=ctr, two=two)


def panoptic_batch(semantic, center, offset, **params):
    """N images: lists of the per-image results of panoptic_one."""
    p = {**CITYSCAPES, **params}
    return [panoptic_one(semantic[n], center[n], offset[n], **p) for n in range(len(center))]


# ------------------------------------------------------------------------------------------------ test cases
# Every case is a dict: semantic (labels uint8 [N,H,W] or logits fp32 [N,C,H,W]), center fp32 [N,1,H,W], offset fp32 [N,2,H,W]
# with multiples of 1/4, params (overrides of CITYSCAPES).  Scores are distinct unless the case says otherwise.
def _scene(rng, N, H, W, n_centers, things=(11, 12, 13), stuff=(0, 1, 8), min_gap=0):
    """Random labelled blobs, offsets pointing roughly at planted centres (quantised to 1/4), distinct scores."""
    sem = np.zeros((N, H, W), np.uint8)
    ctr = np.zeros((N, 1, H, W), np.float32)
    off = np.zeros((N, 2, H, W), np.float32)
    classes = np.array(list(things) + list(stuff), np.uint8)
    for n in range(N):
        coarse = classes[rng.integers(0, len(classes), ((H + 7) // 8, (W + 7) // 8))]
        sem[n] = np.kron(coarse, np.ones((8, 8), np.uint8))[:H, :W]
        # background scores below the threshold (coarse values: the fixture compresses)
        ctr[n, 0] = (rng.integers(0, 368, (H, W)) / 4096).astype(np.float32)
        pts = set()
        while len(pts) < n_centers:
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            if all(max(abs(y - a), abs(x - b)) > min_gap for a, b in pts):
                pts.add((y, x))
        for i, (y, x) in enumerate(sorted(pts)):
            ctr[n, 0, y, x] = 0.2 + 0.7 * (i * 37 % 101 + 1) / 128 + i / 4096          # distinct, above the threshold
        off[n] = np.round(rng.normal(0, 6, (2, H, W)) * 4) / 4
    return sem, ctr, off


def cases():
    """name -> case.  Small on purpose: every case is a few thousand pixels."""
    out = {}
    rng = np.random.default_rng(20)

    # off-tile sizes, N = 3; image 1 has no candidate at all
    for name, (H, W) in (("off_tile_37x53", (37, 53)), ("off_tile_65x97", (65, 97))):
        sem, ctr, off = _scene(rng, 3, H, W, 9)
        ctr[1] = np.minimum(ctr[1], 0.05)
        out[name] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=40, nms_kernel=3))

    # centres on borders, corners, both sides of the 64 x 16 tile seams of the candidate kernel, and a 3x3 plateau
    H, W = 40, 140
    sem, ctr, off = _scene(rng, 1, H, W, 0)
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 70), (H - 1, 30), (20, 0), (9, W - 1),
           (15, 63), (16, 64), (15, 64), (16, 63), (31, 127), (32, 128), (31, 128), (32, 127), (15, 20), (16, 100), (5, 63), (25, 64)]
    for i, (y, x) in enumerate(pts):
        ctr[0, 0, y, x] = 0.3 + i / 64
    ctr[0, 0, 23:26, 40:43] = 0.875                                                       # the plateau: all nine are kept
    out["positions"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=64, nms_kernel=1, top_k=64))
    ctr7 = ctr.copy()
    out["positions_nms7"] = dict(semantic=sem, center=ctr7, offset=off, params=dict(stuff_area=64, nms_kernel=7, top_k=64))

    # top-k: 12 candidates, top_k = 8; the 8th largest score is shared by three (all three drop: 6 remain)
    H, W = 24, 70
    sem, ctr, off = _scene(rng, 1, H, W, 0)
    spots = [(2 + 5 * (i // 4), 3 + 17 * (i % 4)) for i in range(12)]
    scores = [0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.5, 0.5, 0.5, 0.4, 0.35, 0.3]
    for (y, x), s in zip(spots, scores):
        ctr[0, 0, y, x] = s
    out["topk_three_way_tie"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=30, nms_kernel=3, top_k=8))
    flat = ctr.copy()
    for (y, x) in spots:
        flat[0, 0, y, x] = 0.5                                                            # every candidate tied: none remains
    out["topk_all_tied"] = dict(semantic=sem, center=flat, offset=off, params=dict(stuff_area=30, nms_kernel=3, top_k=8))
    out["topk_one"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=30, nms_kernel=3, top_k=1))
    out["topk_minus_one"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=30, nms_kernel=3, top_k=13))
    out["topk_exact"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=30, nms_kernel=3, top_k=12))

    # many centres: nms_kernel = 1, top_k = 300 and the maximum, at 64 x 96
    sem, ctr, off = _scene(rng, 1, 64, 96, 280)
    out["many_centers_300"] = dict(semantic=sem, center=ctr, offset=off,
                                   params=dict(stuff_area=50, nms_kernel=1, top_k=300, label_divisor=2000))
    sem, ctr, off = _scene(rng, 2, 64, 96, 1100)
    ctr[1] = _scene(rng, 1, 64, 96, 1000)[1][0]
    out["many_centers_max"] = dict(semantic=sem, center=ctr, offset=off,
                                   params=dict(stuff_area=50, nms_kernel=1, top_k=1024, label_divisor=2000))

    # a score exactly at the threshold is no centre
    H, W = 20, 30
    sem, ctr, off = _scene(rng, 1, H, W, 0)
    ctr[0, 0, 5, 5], ctr[0, 0, 12, 20], ctr[0, 0, 15, 8] = np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1)), 0.6
    out["threshold"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=10, nms_kernel=3))

    # equidistant centres and offsets that point far outside the image
    H, W = 16, 33
    sem = np.full((1, H, W), 11, np.uint8)
    sem[0, :, 28:] = 0
    ctr = np.zeros((1, 1, H, W), np.float32)
    ctr[0, 0, 8, 4], ctr[0, 0, 8, 24], ctr[0, 0, 2, 14], ctr[0, 0, 14, 14] = 0.5, 0.6, 0.7, 0.8
    off = np.zeros((1, 2, H, W), np.float32)                                              # column 14 is equidistant from two
    off[0, :, 0:3, :] = 300.0                                                             # whole numbers: the fp32 sums are exact
    off[0, :, 13:16, :] = -400.0
    out["equidistant"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=10, nms_kernel=3))

    # majority vote: tie -> smaller class; a centre with stuff pixels only is skipped; 3 + 2 instances numbered per class
    H, W = 24, 56
    sem = np.zeros((1, H, W), np.uint8)
    ctr = np.zeros((1, 1, H, W), np.float32)
    off = np.zeros((1, 2, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(7):                                                                    # seven 8-pixel columns, each pointing
        ctr[0, 0, 12, 8 * i + 4] = 0.9 - i / 16                                           # exactly at its own centre
    off[0, 0], off[0, 1] = 12 - yy, (xx // 8) * 8 + 4 - xx
    for i, cls in enumerate((13, 0, 11, 13, 11, 13, 13)):                                 # 13001, skipped (stuff only), 11001, 13002,
        sem[0, :, 8 * i:8 * i + 8] = cls                                                  # 11002, 12001 (below), 13003
    sem[0, :12, 40:48] = 12                                                               # 96 pixels each of 12 and 13: the tie
    out["majority"] = dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=10, nms_kernel=3))

    # stuff area: exactly stuff_area pixels is kept, one fewer is void
    H, W = 20, 40
    sem = np.full((1, H, W), 11, np.uint8)
    sem[0, 0:5, 0:10] = 3                                                                 # 50 pixels
    sem[0, 10:17, 0:7] = 4                                                                # 49 pixels
    ctr = np.zeros((1, 1, H, W), np.float32)
    ctr[0, 0, 10, 30] = 0.5
    out["stuff_area"] = dict(semantic=sem, center=ctr, offset=np.zeros((1, 2, H, W), np.float32),
                             params=dict(stuff_area=50, nms_kernel=3))

    # logits, with an exact two-way tie on a block of pixels (the first class wins)
    H, W, C = 33, 41, 19
    sem, ctr, off = _scene(rng, 2, H, W, 7)
    logits = (rng.integers(-64, 64, (2, C, H, W)) / 8).astype(np.float32)
    logits[np.arange(2)[:, None, None], sem, np.arange(H)[None, :, None], np.arange(W)[None, None, :]] = 9.0
    logits[:, 12, 4:20, 5:30] = 11.0
    logits[:, 3, 4:20, 5:30] = 11.0                                                       # 3 and 12 tie: 3
    out["logits"] = dict(semantic=logits, center=ctr, offset=off, params=dict(stuff_area=40, nms_kernel=5))
    return out


def unquantised_case(seed=5, H=129, W=257, n_centers=150):
    """Unquantised random offsets, 150 centres: held to the float64 restatement except pixels whose two nearest distances are
    within 1e-5 relative (at most 0.1 % of the pixels)."""
    rng = np.random.default_rng(seed)
    sem, ctr, _ = _scene(rng, 1, H, W, n_centers, min_gap=3)
    off = rng.normal(0, 12, (1, 2, H, W)).astype(np.float32)
    return dict(semantic=sem, center=ctr, offset=off, params=dict(stuff_area=100, nms_kernel=7, top_k=200))


def near_tie_mask(two, rel=1e-5):
    """Pixels whose two smallest squared distances differ by less than `rel` relative IN DISTANCE (the contract's measure)."""
    d1, d2 = np.sqrt(two[0]), np.sqrt(two[1])
    return np.isfinite(d2) & (d2 - d1 < rel * np.maximum(d2, 1e-30))
