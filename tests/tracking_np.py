"""NumPy restatements of the instance-link kernels and of tracking.track_instances, and the scenes the tracking tests are built
from.  Shared by test_tracking_cpu.py (which checks the scenes with them, without a GPU) and test_gpu_tracking.py."""
import glob
import os

import numpy as np

from c2m_amd import graph as G
from golden_io import GOLDEN

TRACKS = os.path.join(GOLDEN, "scene_tracks")
LO, HI = 1000, 19000


# ------------------------------------------------------------------------------------------------ kernels, restated
def np_slots(plane, lo=LO, hi=HI, min_pixels=1):
    """One map [H,W] -> (ids ascending, boxes [n,4] pixel edges, areas [n])."""
    v = plane.astype(np.int64)
    ids, areas = np.unique(v[(v >= lo) & (v < hi)], return_counts=True)
    keep = areas >= min_pixels
    ids, areas = ids[keep], areas[keep]
    boxes = []
    for i in ids:
        ys, xs = np.nonzero(v == i)
        boxes.append([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1])
    return ids, np.asarray(boxes, np.int64).reshape(len(ids), 4), areas


def np_source(flow):
    """csrc/warp_coord.h in float32, operation by operation: flow [2,H,W] -> flat source index [H,W] (warp_source, border clamp,
    round half to even).  The GPU tests take the source from ops.label_warp instead; this one checks the scenes on the CPU."""
    f32 = np.float32
    _, H, W = flow.shape

    def lin(n):
        if n <= 1:
            return np.full(n, -1, f32)
        step = f32(2.0) / f32(n - 1)
        i = np.arange(n)
        lo = (step.astype(np.float64) * i - 1.0).astype(f32)                  # fmaf: one rounding
        hi = (-step.astype(np.float64) * (n - 1 - i) + 1.0).astype(f32)
        return np.where(i < n // 2, lo, hi)

    def coord(fl, grid, n):
        c = f32((n - 1.0) / 2.0)
        g = (grid + fl / c).astype(f32)
        i = (((g + f32(1.0)).astype(f32)).astype(np.float64) * np.float64(f32(n) / f32(2.0)) - 0.5).astype(f32)
        i = np.minimum(f32(n - 1), np.maximum(np.where(np.isnan(i), f32(0), i), f32(0)))
        return np.rint(i).astype(np.int64)

    sx = coord(flow[0].astype(f32), lin(W)[None, :], W)
    sy = coord(flow[1].astype(f32), lin(H)[:, None], H)
    return sy * W + sx


def np_pairs(ref, frame, src, ref_ids, frame_ids, M):
    """Contingency table [M+1, M+1] of two maps [H,W]; src: flat source index per frame pixel or None (the pixel itself)."""
    def slot(v, ids):
        pos = np.searchsorted(ids, v)
        hit = (pos < len(ids)) & (np.asarray(ids, np.int64)[np.minimum(pos, max(len(ids) - 1, 0))] == v) if len(ids) else \
            np.zeros(v.shape, bool)
        return np.where(hit, pos, M)

    warped = ref.reshape(-1) if src is None else ref.reshape(-1)[src.reshape(-1)]
    out = np.zeros((M + 1, M + 1), np.int64)
    np.add.at(out, (slot(warped.astype(np.int64), ref_ids), slot(frame.reshape(-1).astype(np.int64), frame_ids)), 1)
    return out


def np_match(pairs, ref_ids, frame_ids, min_iou=(1, 4), same_class=True):
    """The match rule restated: pairs [nr+1, nf+1] ("no slot" last) -> the frame slot of every ref slot or -1."""
    n = np.asarray(pairs, np.int64)
    nr, nf = len(ref_ids), len(frame_ids)
    union = n.sum(1)[:nr, None] + n.sum(0)[None, :nf] - n[:nr, :nf]
    better = lambda i, j, k, l: n[i, j] * union[k, l] > n[k, l] * union[i, j]            # IoU(i,j) > IoU(k,l), exactly
    link = np.full(nr, -1, np.int64)
    for i in range(nr):
        for j in range(nf):
            if n[i, j] > 0 and not any(n[i, l] > 0 and (better(i, l, i, j) or (l < j and not better(i, j, i, l))) for l in range(nf)) \
                    and not any(n[k, j] > 0 and (better(k, j, i, j) or (k < i and not better(i, j, k, j))) for k in range(nr)) \
                    and n[i, j] * min_iou[1] >= min_iou[0] * union[i, j] \
                    and (not same_class or ref_ids[i] // 1000 == frame_ids[j] // 1000):
                link[i] = j
    return link


def np_track(inst, t_in, target_flow=None, input_flow=None, min_pixels=1, M=64, min_iou=(1, 4), same_class=True):
    """tracking.track_instances for one sample, restated: inst [T,H,W], target_flow [2,T-t_in,H,W], input_flow [2,t_in-1,H,W]
    (or None) -> (ids [N,T], boxes [N,T,4], lost [(anchor id, frame)])."""
    T = inst.shape[0]
    a = t_in - 1
    slots = [np_slots(inst[t], min_pixels=min_pixels) for t in range(T)]
    assert all(len(s[0]) <= M for s in slots)

    def link(ref_t, t, flow):
        src = None if flow is None else np_source(flow)
        pr = np_pairs(inst[ref_t], inst[t], src, slots[ref_t][0], slots[t][0], M)
        nr, nf = len(slots[ref_t][0]), len(slots[t][0])
        sub = np.zeros((nr + 1, nf + 1), np.int64)
        sub[:nr, :nf], sub[:nr, nf], sub[nr, :nf], sub[nr, nf] = pr[:nr, :nf], pr[:nr, M], pr[M, :nf], pr[M, M]
        return np_match(sub, slots[ref_t][0], slots[t][0], min_iou, same_class)

    na = len(slots[a][0])
    slot = np.full((na, T), -1, np.int64)
    slot[:, a] = np.arange(na)
    for t in range(t_in, T):
        slot[:, t] = link(a, t, None if target_flow is None else target_flow[:, t - t_in])
    for t in range(a - 1, -1, -1):
        lk = link(t + 1, t, None if input_flow is None else input_flow[:, t])
        slot[:, t] = np.where(slot[:, t + 1] >= 0, lk[np.maximum(slot[:, t + 1], 0)] if len(lk) else -1, -1)
    keep = (slot >= 0).all(1)
    order = list(range(a - 1, -1, -1)) + list(range(t_in, T))
    lost = [(int(slots[a][0][s]), next(f for f in order if slot[s, f] < 0)) for s in np.nonzero(~keep)[0]]
    rows = np.nonzero(keep)[0]
    ids = np.array([[slots[t][0][slot[s, t]] for t in range(T)] for s in rows], np.int64).reshape(len(rows), T)
    boxes = np.array([[slots[t][1][slot[s, t]] for t in range(T)] for s in rows], np.int64).reshape(len(rows), T, 4)
    return ids, boxes, lost


# ------------------------------------------------------------------------------------------------ scenes
def fixture_boxes(prefix, T, size):
    """The tests/golden/scene_tracks boxes of one scene rounded to the pixel grid of `size`: (edges [N,T,4] int, ids [N])."""
    H, W = size
    tracks = [open(p).read().splitlines() for p in sorted(glob.glob(os.path.join(TRACKS, prefix) + "*.txt"))]
    box, ids = G.parse_tracks(tracks, T)
    x0, y0 = np.rint(box[..., 0] / 2048 * W), np.rint(box[..., 1] / 1024 * H)
    x1, y1 = np.rint((box[..., 0] + box[..., 2]) / 2048 * W), np.rint((box[..., 1] + box[..., 3]) / 1024 * H)
    edges = np.stack([x0, y0, np.maximum(x1, x0 + 1), np.maximum(y1, y0 + 1)], -1).astype(np.int64)
    return edges, ids[:, 0].copy()


def constructed_boxes(T, size, n=12, seed=0):
    """n rectangles of four classes on a grid of cells, each drifting a few pixels per frame inside its cell."""
    H, W = size
    rng = np.random.default_rng(seed)
    cols = 4
    rows = -(-n // cols)
    ch, cw = H // rows, W // cols
    edges = np.zeros((n, T, 4), np.int64)
    for k in range(n):
        cy, cx = (k // cols) * ch, (k % cols) * cw
        h, w = rng.integers(ch // 3, ch // 2), rng.integers(cw // 3, cw // 2)
        y, x = cy + rng.integers(0, ch // 4), cx + rng.integers(0, cw // 4)
        vy, vx = rng.integers(-2, 3), rng.integers(-3, 4)
        for t in range(T):
            yy = int(np.clip(y + vy * t, 0, H - h)); xx = int(np.clip(x + vx * t, 0, W - w))
            edges[k, t] = [xx, yy, xx + w, yy + h]
    ids = np.array([(11 + k % 4) * 1000 + 1 + k // 4 for k in range(n)], np.int64)
    return edges, ids


def paint_scene(edges, ids, t_in, size, seed=0, permute=True, background=(0, 7, 24001)):
    """Rectangles painted in a fixed z-order (later objects on top) with, per frame, the ids permuted among the objects of a class
    (the anchor frame keeps `ids`).  Returns dict(inst [T,H,W] int32, frame_ids [N,T] (the id object k carries in frame t),
    target_flow [2,T-t_in,H,W], input_flow [2,t_in-1,H,W] fp32: the true displacement of the object under every pixel, zero
    elsewhere), as track_instances consumes them."""
    H, W = size
    N, T = edges.shape[:2]
    rng = np.random.default_rng(seed)
    a = t_in - 1
    frame_ids = np.repeat(np.asarray(ids, np.int64)[:, None], T, 1)
    if permute:
        for t in range(T):
            if t == a:
                continue
            for c in np.unique(frame_ids[:, t] // 1000):
                rows = np.nonzero(np.asarray(ids) // 1000 == c)[0]
                pool = np.concatenate([np.asarray(ids)[rows], c * 1000 + 500 + np.arange(len(rows))])   # some ids are new
                frame_ids[rows, t] = rng.permutation(pool)[:len(rows)]
    inst = rng.choice(np.array(background, np.int32), (T, H, W)).astype(np.int32)
    owner = np.full((T, H, W), -1, np.int64)
    for t in range(T):
        for k in range(N):
            x0, y0, x1, y1 = edges[k, t]
            inst[t, y0:y1, x0:x1] = frame_ids[k, t]
            owner[t, y0:y1, x0:x1] = k
    centre = np.stack([(edges[..., 0] + edges[..., 2]) // 2, (edges[..., 1] + edges[..., 3]) // 2], -1)      # [N,T,2]

    def flow_to(t, ref_t):
        f = np.zeros((2, H, W), np.float32)
        for k in range(N):
            m = owner[t] == k
            f[0][m], f[1][m] = centre[k, ref_t, 0] - centre[k, t, 0], centre[k, ref_t, 1] - centre[k, t, 1]
        return f

    target = np.stack([flow_to(t, a) for t in range(t_in, T)], 1) if T > t_in else np.zeros((2, 0, H, W), np.float32)
    inputs = np.stack([flow_to(t, t + 1) for t in range(a)], 1) if a > 0 else np.zeros((2, 0, H, W), np.float32)
    return dict(inst=inst, frame_ids=frame_ids, target_flow=target, input_flow=inputs, owner=owner)


def painted_extents(scene):
    """What the tracker must return for a painted scene: per object and frame the id it carries and the extent of its VISIBLE
    pixels, objects in ascending anchor id order: (ids [N,T], boxes [N,T,4])."""
    inst, fid = scene["inst"], scene["frame_ids"]
    N, T = fid.shape
    boxes = np.zeros((N, T, 4), np.int64)
    for k in range(N):
        for t in range(T):
            ys, xs = np.nonzero(scene["owner"][t] == k)
            assert len(ys), f"object {k} is hidden in frame {t}"
            boxes[k, t] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
    return fid, boxes


SCENES = [("fixture", "aachen_000000_000019_", 2), ("fixture", "bonn_000001_000004_", 2), ("fixture", "aachen_000000_000019_", 1),
          ("constructed", 12, 2), ("constructed", 20, 1)]


def make_scene(kind, arg, t_in, T=7, size=(128, 256), seed=0, permute=True):
    edges, ids = fixture_boxes(arg, T, size) if kind == "fixture" else constructed_boxes(T, size, arg, seed)
    return edges, ids, paint_scene(edges, ids, t_in, size, seed, permute)
