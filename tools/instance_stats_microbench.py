"""Device-event timing of ops.instance_stats (c2m_instance_stats: table init + per-instance statistics) and of the whole
ops.instance_boxes call (stats, compaction, one device -> host read), next to a torch copy_ of the maps' bytes.

    python tools/instance_stats_microbench.py [--planes 16] [--sizes 128x256,1024x2048] [--objects 30]

The maps are street-scene-like: stuff ids (< 1000) in horizontal bands, `--objects` ellipses with ids 11001..18999 of
random sizes on top (about a fifth of the pixels).  Prints one JSON line per size: median microseconds and the rate at
which the maps are read."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2]


def scene_maps(planes, H, W, objects, seed=0):
    g = torch.Generator().manual_seed(seed)
    ys = torch.arange(H).view(H, 1).float()
    xs = torch.arange(W).view(1, W).float()
    out = torch.empty(planes, H, W, dtype=torch.int32)
    for p in range(planes):
        m = torch.full((H, W), 23, dtype=torch.int32)                          # sky
        m[ys.view(-1) >= H * 0.35] = 11                                        # buildings
        m[ys.view(-1) >= H * 0.6] = 7                                          # road
        for k in range(objects):
            cy, cx = float(torch.rand(1, generator=g)) * H, float(torch.rand(1, generator=g)) * W
            ry = (0.02 + 0.1 * float(torch.rand(1, generator=g))) * H
            rx = ry * (0.5 + float(torch.rand(1, generator=g))) * W / H
            inside = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1
            m[inside] = 1000 * (11 + k % 8) + 1 + k
        out[p] = m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--sizes", default="128x256,1024x2048")
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        maps = scene_maps(a.planes, H, W, a.objects).to("cuda").view(a.planes, 1, H, W)   # B = planes, t_in = 1
        obj = float(((maps >= 1000) & (maps < 19000)).float().mean())
        dst = torch.empty_like(maps)
        t_stats = timed(lambda: ops.instance_stats(maps, 1), a.iters)
        t_copy = timed(lambda: dst.copy_(maps), a.iters)
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            ops.instance_boxes(maps, 1)
        t_boxes = (time.perf_counter() - t0) / n * 1e6
        nbytes = maps.numel() * 4
        print(json.dumps({"H": H, "W": W, "planes": a.planes, "object_pixel_fraction": round(obj, 3),
                          "instance_stats_us": round(t_stats, 1), "maps_read_GBps": round(nbytes / t_stats / 1e3, 1),
                          "copy_us": round(t_copy, 1), "copy_GBps": round(2 * nbytes / t_copy / 1e3, 1),
                          "instance_boxes_wall_us": round(t_boxes, 1)}))


if __name__ == "__main__":
    main()
