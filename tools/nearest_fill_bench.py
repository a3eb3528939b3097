"""Device-event timing of ops.nearest_fill (csrc/nearest_fill.hip: every disoccluded pixel takes its label planes from the nearest
visible background pixel) next to the only other way to get the same result, and next to the time its bytes need at the rate of a
copy.

    python tools/nearest_fill_bench.py [--iters 10] [--out FILE]

Workloads: the maps propagate_maps fills, Cf = 20 float planes and Ci = 1 id plane, at [8,.,5,128,256] and [1,.,5,1024,2048].
Holes are the crescents a moved disc leaves behind: --discs discs per frame (default 36) at random places, each moved by 2 - 12
pixels; the hole is the old support minus the new one, the new supports are things (no seeds), everything else is a seed.  One
adversarial frame per size has its whole lower half as ONE hole under an upper half of seeds: the walk of a hole pixel is then as
long as its distance to the middle row, and every row on the way is scanned over its full width.
The yardstick lives here only and is used only if scipy is importable (the package never falls back to it): masks and planes to
the host, scipy.ndimage.distance_transform_edt(return_indices=True) per frame, a gather, and the planes back to the device.  The
two are timed alternately in one process after --warmup rounds, median of --iters repetitions each, HIP events around each.  In
that alternation the call starts on an idle queue; --queue calls issued back to back between two events give the time per call
with the queue kept busy.  A fill writes only holes and reads only seeds, so repeating it on the filled planes is the same work.
The id plane holds every pixel's own index, so a filled pixel names its source: the tool checks that every source is a seed at
exactly scipy's distance (its ties differ, its distances must not).
Prints one JSON line per workload: milliseconds, the bytes the call must move (both masks once, and a read and a write of
Cf + Ci words per hole pixel) and the time those bytes take at the two ends of the range DESIGN 4.2g measured for a copy.
--out appends the lines to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops  # noqa: E402

COPY_GBPS = (3500.0, 5900.0)            # ATen strided copies on this GPU
CF, CI = 20, 1


def crescents(B, T, H, W, discs, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    hole, thing = np.zeros((B, T, H, W), bool), np.zeros((B, T, H, W), bool)
    for b in range(B):
        for t in range(T):
            for _ in range(discs):
                r = rng.integers(max(H // 32, 3), max(H // 10, 5))
                cy, cx = rng.integers(0, H), rng.integers(0, W)
                ang, s = rng.random() * 2 * np.pi, rng.integers(2, 13)
                dy, dx = s * np.sin(ang), s * np.cos(ang)
                y0, y1, x0, x1 = max(cy - r - 13, 0), min(cy + r + 14, H), max(cx - r - 13, 0), min(cx + r + 14, W)
                py, px = yy[y0:y1, x0:x1], xx[y0:y1, x0:x1]
                old = (py - cy) ** 2 + (px - cx) ** 2 <= r * r
                new = (py - cy - dy) ** 2 + (px - cx - dx) ** 2 <= r * r
                hole[b, t, y0:y1, x0:x1] |= old & ~new
                thing[b, t, y0:y1, x0:x1] |= new
    hole &= ~thing                                                     # a disc moved onto another's crescent covers it
    return hole, ~hole & ~thing


def lower_half(H, W):
    hole = np.zeros((1, 1, H, W), bool)
    hole[..., H // 2:, :] = True
    return hole, ~hole


def planes(B, T, H, W, seed=1):
    g = torch.Generator().manual_seed(seed)
    pf = torch.randn(B, CF, T, H, W, generator=g)
    pi = torch.arange(H * W, dtype=torch.int32).view(1, 1, 1, H, W).expand(B, CI, T, H, W).contiguous()
    return pf, pi


def scipy_fill(hole, seed, pf, pi):
    """The yardstick: device -> host, one distance transform per frame, gather, host -> device.  Returns the new device planes."""
    from scipy import ndimage
    h, s, f, i = hole.cpu().numpy(), seed.cpu().numpy(), pf.cpu().numpy(), pi.cpu().numpy()
    B, T = h.shape[:2]
    for b in range(B):
        for t in range(T):
            if not s[b, t].any():
                continue
            iy, ix = ndimage.distance_transform_edt(~s[b, t], return_distances=False, return_indices=True)
            ys, xs = np.nonzero(h[b, t])
            f[b, :, t, ys, xs] = f[b, :, t, iy[ys, xs], ix[ys, xs]]
            i[b, :, t, ys, xs] = i[b, :, t, iy[ys, xs], ix[ys, xs]]
    return torch.from_numpy(f).to(pf.device), torch.from_numpy(i).to(pi.device)


def median(t):
    return sorted(t)[len(t) // 2]


def timed_pair(fa, fb, iters, warmup):
    for _ in range(warmup):
        fa()
        if fb:
            fb()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in ev:
        a.record()
        fa()
        b.record()
        if fb:
            fb()
        c.record()
    torch.cuda.synchronize()
    return median([a.elapsed_time(b) for a, b, _ in ev]), (median([b.elapsed_time(c) for _, b, c in ev]) if fb else None)


def timed_queue(fn, calls, iters):
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return median(times)


def run(name, hole_np, seed_np, a, have_scipy):
    B, T, H, W = hole_np.shape
    hole, seed = torch.from_numpy(hole_np).cuda(), torch.from_numpy(seed_np).cuda()
    pf, pi = (t.cuda() for t in planes(B, T, H, W))
    kernel = lambda: ops.nearest_fill(hole, seed, pf, pi)
    stock = (lambda: scipy_fill(hole, seed, pf, pi)) if have_scipy else None
    ms_kernel, ms_stock = timed_pair(kernel, stock, a.iters, a.warmup)
    ms_queue = timed_queue(kernel, a.queue, a.iters)
    unfilled = kernel()
    holes = int(hole_np.sum())
    nbytes = 2 * hole_np.size + holes * (CF + CI) * 8
    res = {"workload": name, "shape": [B, CF + CI, T, H, W], "hole_pixels": holes, "hole_share": round(holes / hole_np.size, 4),
           "unfilled": int(unfilled.sum()), "kernel_ms": round(ms_kernel, 4), "kernel_ms_back_to_back": round(ms_queue, 4),
           "bytes_must_move": nbytes, "ms_at_copy_rate": [round(nbytes / r / 1e6, 4) for r in COPY_GBPS],
           "kernel_back_to_back_over_copy_rate": [round(ms_queue / (nbytes / r / 1e6), 1) for r in COPY_GBPS]}
    if have_scipy:
        from scipy import ndimage
        src = pi.cpu().numpy()[:, 0]
        ok = True
        for b in range(B):
            for t in range(T):
                ys, xs = np.nonzero(hole_np[b, t])
                sy, sx = src[b, t, ys, xs] // W, src[b, t, ys, xs] % W
                d2 = np.rint(ndimage.distance_transform_edt(~seed_np[b, t]) ** 2).astype(np.int64)
                ok = ok and bool(seed_np[b, t, sy, sx].all()) and bool(((sy - ys) ** 2 + (sx - xs) ** 2 == d2[ys, xs]).all())
        res.update(scipy_ms=round(ms_stock, 2), scipy_over_kernel=round(ms_stock / ms_kernel, 1), sources_at_scipys_distance=ok)
    else:
        res.update(scipy_ms="not measured (scipy is not importable)")
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queue", type=int, default=10)
    ap.add_argument("--discs", type=int, default=36)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nearest_fill_bench needs a GPU: a timing taken anywhere else says nothing about it")
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    for (B, T, H, W) in ((8, 5, 128, 256), (1, 5, 1024, 2048)):
        run(f"crescents {H}x{W}", *crescents(B, T, H, W, a.discs), a, have_scipy)
    a.iters, a.queue = min(a.iters, 5), min(a.queue, 2)                # the slow case: fewer repetitions
    for (H, W) in ((128, 256), (1024, 2048)):
        run(f"lower half one hole {H}x{W}", *lower_half(H, W), a, have_scipy)


if __name__ == "__main__":
    main()
