"""Device-event timing of evaluate.tube_quality (csrc/map_quality.hip: video panoptic quality, the pixels read once and the
per-frame tables merged per window) next to what the package offered for the same result before it: evaluate.map_quality on the
windows' frames stacked into one image each with torch.cat, one call per window length.

    python tools/tube_quality_bench.py [--iters 10] [--out FILE]

Workloads: int32 clips [8,15,128,256] and [1,15,1024,2048] with windows (1, 2, 3, 4, "all"); the ground truth a synthetic
Cityscapes-like layout (stuff bands, a void strip, numbered things that drift and keep their ids, a crowd region), the
prediction the same shifted by a few pixels.  The two are timed alternately in one process between device events, warmed up
first (two rounds), median of --iters repetitions each, and their results are checked equal (tp, fp, fn, iou bit for bit,
overflow).  Prints one JSON line per workload; --out appends them to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import evaluate  # noqa: E402

P = evaluate.MAP_QUALITY
WINDOWS = (1, 2, 3, 4, "all")
SHAPES = ((8, 15, 128, 256), (1, 15, 1024, 2048))
FIELDS = ("tp", "fp", "fn", "iou", "overflow")


def workload(B, T, H, W, things, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: int(torch.randint(lo, max(hi, lo + 1), (1,), generator=g))
    stuff = torch.tensor([0, 1, 2, 8, 10])
    gt = torch.empty(B, T, H, W, dtype=torch.int32)
    for b in range(B):
        bands = stuff[(torch.arange(W) * len(stuff) // W + b) % len(stuff)].int()
        gt[b] = bands.view(1, 1, W).expand(T, H, W)
        gt[b, :, : H // 3] = 10
        gt[b, :, -(H // 20):] = 255                                         # the ego vehicle: void
        gt[b, :, H // 2: H // 2 + H // 16, : W // 6] = 13000                # a crowd of cars
        count = {}
        for _ in range(things):
            c = int(P["thing_list"][r(0, len(P["thing_list"]))])
            count[c] = count.get(c, 0) + 1
            h, w = r(8, H // 8), r(8, W // 16)
            y, x, vy, vx = r(0, H - h), r(0, W - w), r(-2, 3), r(-4, 5)
            for t in range(T):
                yy, xx = min(max(y + vy * t, 0), H - h), min(max(x + vx * t, 0), W - w)
                gt[b, t, yy:yy + h, xx:xx + w] = c * 1000 + count[c]
    pred = torch.roll(gt, shifts=(3, 5), dims=(2, 3))
    pred[..., :5] = 255
    return pred.cuda().contiguous(), gt.cuda().contiguous()


def stacked(pred, gt, ks):
    """The parent's route: for every k, the windows' frames concatenated along the rows, then map_quality per stacked image."""
    B, T, H, W = pred.shape
    out = {}
    for k in ks:
        stack = lambda m: torch.stack([torch.cat([m[b, t] for t in range(t0, t0 + k)], 0) for b in range(B) for t0 in range(T - k + 1)])
        m = evaluate.map_quality(stack(pred), stack(gt))
        out[k] = {f: m[f].view(B, T - k + 1, *m[f].shape[1:]) for f in FIELDS}
    return out


def timed_pair(fa, fb, iters, warmup=2):
    """Median milliseconds of fa and fb, alternated."""
    for _ in range(warmup):
        fa()
        fb()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in ev:
        a.record()
        fa()
        b.record()
        fb()
        c.record()
    torch.cuda.synchronize()
    med = lambda t: sorted(t)[len(t) // 2]
    return med([a.elapsed_time(b) for a, b, _ in ev]), med([b.elapsed_time(c) for _, b, c in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tube_quality_bench needs a GPU: a timing taken anywhere else says nothing about it")
    for B, T, H, W in SHAPES:
        pred, gt = workload(B, T, H, W, things=max(H * W // 8192, 8))
        ks = tuple(T if k == "all" else k for k in WINDOWS)
        tube = lambda: evaluate.tube_quality(pred, gt, windows=WINDOWS)
        stack = lambda: stacked(pred, gt, ks)
        ms_tube, ms_stack = timed_pair(tube, stack, a.iters)
        got, want = tube(), stack()
        torch.cuda.synchronize()
        agree = all(torch.equal(got[k][f], want[k][f]) for k in ks for f in FIELDS)
        res = {"shape": [B, T, H, W], "windows": list(ks), "map_bytes": 2 * pred.numel() * 4, "tube_ms": round(ms_tube, 4),
               "stacked_ms": round(ms_stack, 4), "stacked_over_tube": round(ms_stack / ms_tube, 2),
               "tp_fp_fn_per_k": {k: [int(got[k][f].sum()) for f in ("tp", "fp", "fn")] for k in ks},
               "overflow": bool(any(got[k]["overflow"].any() for k in ks)), "results_agree_exactly": bool(agree)}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
