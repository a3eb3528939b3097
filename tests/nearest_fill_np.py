"""The contract of ops.nearest_fill in numpy, brute force: for every hole pixel all hole-seed distances as int64,
the key d^2 * (H * W) + y' * W + x', argmin.  A pixel set in both masks is a hole and never a seed.  Nothing here is fast; the
shapes of the tests are small."""
import numpy as np


def sources(hole, seed):
    """hole, seed: [H, W] (nonzero = set) -> (ys, xs, src): the hole pixels and the flat index y' * W + x' of each one's source,
    or None when the image has no seed."""
    hole = np.asarray(hole) != 0
    seed = (np.asarray(seed) != 0) & ~hole
    H, W = hole.shape
    ys, xs = np.nonzero(hole)
    sy, sx = np.nonzero(seed)
    if sy.size == 0:
        return ys, xs, None
    d2 = (ys[:, None].astype(np.int64) - sy[None]) ** 2 + (xs[:, None].astype(np.int64) - sx[None]) ** 2
    key = d2 * (H * W) + (sy.astype(np.int64) * W + sx)[None]
    k = key.argmin(1) if ys.size else np.zeros(0, np.int64)
    return ys, xs, sy[k].astype(np.int64) * W + sx[k]


def nearest_fill(hole, seed, planes):
    """hole, seed [B, T, H, W]; planes: a list of arrays [B, C, T, H, W] of 32-bit items (None passes) -> (the filled copies as
    int32 words, in the same order; unfilled [B, T] int32)."""
    hole, seed = np.asarray(hole), np.asarray(seed)
    B, T, H, W = hole.shape
    outs = [None if p is None else np.ascontiguousarray(p).view(np.int32).copy() for p in planes]
    unfilled = np.zeros((B, T), np.int32)
    for b in range(B):
        for t in range(T):
            ys, xs, src = sources(hole[b, t], seed[b, t])
            if src is None:
                unfilled[b, t] = ys.size
                continue
            for o in outs:
                if o is not None and o.shape[1]:
                    flat = o[b, :, t].reshape(o.shape[1], H * W)              # a view: o is contiguous in (H, W)
                    o[b, :, t, ys, xs] = flat[:, src].T
    return outs, unfilled


def source_distance(hole, seed):
    """[H, W] float64: the Euclidean distance of every hole pixel to its chosen source, 0 elsewhere (for the comparison with
    scipy's distance transform, whose ties differ but whose distances must not)."""
    ys, xs, src = sources(hole, seed)
    H, W = np.asarray(hole).shape
    out = np.zeros((H, W))
    if src is not None:
        out[ys, xs] = np.sqrt((ys - src // W) ** 2 + (xs - src % W) ** 2)
    return out


def paint(H, W, cy, cx, seeds):
    """One hole at (cy, cx) and seeds at the given (dy, dx) offsets from it; every other pixel is neither hole nor seed
    -> (hole, seed) [H, W] uint8."""
    hole, seed = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    hole[cy, cx] = 1
    for dy, dx in seeds:
        assert 0 <= cy + dy < H and 0 <= cx + dx < W
        seed[cy + dy, cx + dx] = 1
    return hole, seed


def label_planes(rng, B, Cf, Ci, T, H, W):
    """Planes whose every word names its own place, so a wrong source shows: fp32 [B,Cf,T,H,W] and int32 [B,Ci,T,H,W]."""
    pf = rng.standard_normal((B, Cf, T, H, W)).astype(np.float32)
    pi = rng.integers(-2 ** 31, 2 ** 31, (B, Ci, T, H, W), dtype=np.int64).astype(np.int32)
    return pf, pi
