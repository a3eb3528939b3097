"""Times the detector metric's device work with HIP events: warm-up, then the median of --iters timed runs.

 (i)   a full YOLOv3 forward at 416 x 416, N = 16 (seeded random weights);
 (ii)  candidates + sort + suppression (ops.yolo_candidates, ops.nms_merge) on those heads, and on planted heads with about 300
       and about 7 000 candidates per image;
 (iii) the same suppression written as the reference's loop of stock torch ops on the device (one image at a time, a host round
       trip per `while` test), as the comparison.
Prints one JSON line per measurement.   python tools/detect_microbench.py [--iters 20] [--batch 16]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops  # noqa: E402
from c2m_amd.modules.networks.yolo_v3 import Darknet  # noqa: E402

ANCHORS = [[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]]


def timed(fn, iters, warmup=3, inner=1):
    """Median, and the (min, max) of the timed windows, in ms per call; a window holds `inner` calls so that a 0.1 ms call is
    measured over a window well above the event resolution."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"ms": round(float(np.median(ms)), 3), "min": round(float(min(ms)), 3), "max": round(float(max(ms)), 3), "windows": iters,
            "calls_per_window": inner}


def planted_heads(N, per_image, dev, seed=0, C=80):
    """Background far below the threshold; `per_image` random boxes pass, anchor-sized, random classes."""
    g = torch.Generator().manual_seed(seed)
    heads = [torch.full((N, 3 * (5 + C), s, s), -7.0) for s in (13, 26, 52)]
    nb = [3 * s * s for s in (13, 26, 52)]
    for n in range(N):
        pick = torch.randperm(sum(nb), generator=g)[:per_image]
        for j in pick.tolist():
            h = 0 if j < nb[0] else 1 if j < nb[0] + nb[1] else 2
            r = j - sum(nb[:h])
            s = heads[h].shape[-1]
            a, gy, gx = r // (s * s), (r // s) % s, r % s
            v = torch.randn(5 + C, generator=g)
            v[2:4] = torch.randn(2, generator=g) * 0.3
            v[4] = 0.2 + 3 * torch.rand(1, generator=g)
            heads[h][n, a * (5 + C):(a + 1) * (5 + C), gy, gx] = v
    return [h.to(dev) for h in heads]


def torch_nms(cand_rows, nms_thres=0.4):
    """non_max_suppression's loop (yolo_v3/utils/utils.py) as stock torch ops on the device, for one image's candidates."""
    score = cand_rows[:, 4] * cand_rows[:, 5]
    det = cand_rows[(-score).argsort()]
    keep = []
    while det.size(0):
        b = det[0, :4]
        iw = (torch.min(b[2], det[:, 2]) - torch.max(b[0], det[:, 0]) + 1).clamp(min=0)
        ih = (torch.min(b[3], det[:, 3]) - torch.max(b[1], det[:, 1]) + 1).clamp(min=0)
        inter = iw * ih
        iou = inter / ((b[2] - b[0] + 1) * (b[3] - b[1] + 1) + (det[:, 2] - det[:, 0] + 1) * (det[:, 3] - det[:, 1] + 1) - inter
                       + 1e-16)
        invalid = (iou > nms_thres) & (det[0, -1] == det[:, -1])
        invalid[0] = True
        w = det[invalid, 4:5]
        det[0, :4] = (w * det[invalid, :4]).sum(0) / w.sum()
        keep.append(det[0])
        det = det[~invalid]
    return torch.stack(keep) if keep else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    dev, N = "cuda:0", args.batch
    torch.manual_seed(0)
    net = Darknet().to(dev).eval()
    x = torch.rand(N, 3, 416, 416, device=dev)
    heads = net(x)
    print(json.dumps({"what": "yolov3 forward 416x416", "N": N, **timed(lambda: net(x), args.iters)}), flush=True)
    for name, hs in (("network heads", heads), ("planted ~300 / image", planted_heads(N, 300, dev)),
                     ("planted ~7000 / image", planted_heads(N, 7000, dev, seed=1))):
        cand, score, count = ops.yolo_candidates(hs, ANCHORS, 80, 416, 0.5)
        dets, kept = ops.nms_merge(cand, score, count, 0.4)
        n_c, n_k = count.float().mean().item(), kept.float().mean().item()
        row = {"what": name, "N": N, "candidates_per_image": round(n_c, 1), "kept_per_image": round(n_k, 1),
               "candidates": timed(lambda: ops.yolo_candidates(hs, ANCHORS, 80, 416, 0.5), args.iters, inner=50),
               "sort_and_nms": timed(lambda: ops.nms_merge(cand, score, count, 0.4), args.iters, inner=20 if n_c <= 1000 else 1)}
        # the stock-torch loop: all N images at a few hundred candidates; ONE image at thousands (seconds each); one warm-up run
        # and three timed ones either way
        rows = [cand[n, :int(count[n])].clone() for n in range(N if n_c <= 1000 else 1)]
        row["torch_loop_images"] = len(rows)
        row["torch_loop"] = timed(lambda: [torch_nms(r.clone()) for r in rows], 3, warmup=1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
