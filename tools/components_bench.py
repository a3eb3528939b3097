"""Device-event timing of ops.connected_components and segment.semantic_instances (csrc/components.hip) next to the two other
ways to instance ids: ops.panoptic_maps on the same number of frames (the producer that needs a network's centre and offset
heads; here on synthetic heads, labels given), and scipy.ndimage.label on the host including the copy of the labels to the host
and of the result back (if scipy is installed).

    python tools/components_bench.py [--reps 20] [--warmup 3] [--out FILE]

Workloads: 56 frames of 128 x 256 (a B = 8 clip of 7 frames), 1 and 8 frames of 1024 x 2048; each on random-blob labels (classes
in cells of 32 pixels with 0.2 % of the pixels redrawn) and on the serpentine, a one-pixel path along every second row joined
alternately at either end -- ONE component that crosses every tile seam, the worst case of the seam pass.  HIP events around
every repetition; median and min-max over --reps after --warmup rounds.  Prints one JSON line per workload; --out appends them
to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops, segment  # noqa: E402

THINGS = segment.CITYSCAPES["thing_list"]


def blob_labels(N, H, W, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    classes = torch.tensor([0, 1, 2, 8, 10, 11, 12, 13, 13, 13, 11, 18], device="cuda", dtype=torch.uint8)
    pick = lambda *s: classes[(torch.rand(*s, device="cuda", generator=g) * len(classes)).long().clamp_(max=len(classes) - 1)]
    coarse = pick(N, H // 32 + 1, W // 32 + 1)
    labels = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].contiguous()
    redraw = torch.rand(N, H, W, device="cuda", generator=g) < 0.002
    return torch.where(redraw, pick(N, H, W), labels)


def serpentine_labels(N, H, W):
    img = torch.full((H, W), 7, dtype=torch.uint8)
    img[0::2] = 11
    for i, y in enumerate(range(1, H - 1, 2)):
        img[y, W - 1 if i % 2 == 0 else 0] = 11
    return img.to("cuda").expand(N, H, W).contiguous()


def heads(N, H, W, seed=1):
    """Synthetic centre and offset heads: about 200 peaks per frame, offsets of a few pixels."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    center = torch.rand(N, 1, H, W, device="cuda", generator=g) * 0.05
    ys = (torch.rand(N, 200, device="cuda", generator=g) * H).long().clamp_(max=H - 1)
    xs = (torch.rand(N, 200, device="cuda", generator=g) * W).long().clamp_(max=W - 1)
    center[torch.arange(N, device="cuda")[:, None], 0, ys, xs] = 0.5
    return center, torch.randn(N, 2, H, W, device="cuda", generator=g) * 4


def timed(fn, reps, warmup):
    """Milliseconds of fn by HIP events: (median, min, max) over reps."""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return [round(t[len(t) // 2], 4), round(t[0], 4), round(t[-1], 4)]


def scipy_host(labels, components, reps):
    """ndimage.label of every thing class of every frame (8-connectivity) on the host, with the copy of the labels to the host
    and of the int32 result back: wall-clock milliseconds (median, min, max), and whether frame 0 splits its thing pixels into
    the same sets as `components` does.  (None, None) without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None, None
    eight = np.ones((3, 3), int)
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = labels.cpu().numpy()
        out = np.zeros(host.shape, np.int32)
        for n in range(host.shape[0]):
            for c in THINGS:
                mask = host[n] == c
                if mask.any():
                    lab, _ = ndimage.label(mask, structure=eight)
                    out[n][mask] = c * 1000 + lab[mask]
        torch.from_numpy(out).to("cuda")
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    mask = out[0] > 0
    pairs = np.unique(np.stack([components[0].cpu().numpy()[mask], out[0][mask]]), axis=1)
    same = len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))
    return [round(t[len(t) // 2], 2), round(t[0], 2), round(t[-1], 2)], bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs a GPU: a timing taken anywhere else says nothing about it")
    lines = []
    for N, H, W in ((56, 128, 256), (1, 1024, 2048), (8, 1024, 2048)):
        center, offset = heads(N, H, W)
        for kind, labels in (("blobs", blob_labels(N, H, W)), ("serpentine", serpentine_labels(N, H, W))):
            maps = segment.semantic_instances(labels)
            res = {"frames": N, "size": [H, W], "labels": kind,
                   "components_per_frame": int(torch.unique(maps["components"][0]).numel()),
                   "kept_things_per_frame": int(maps["count"][0].sum()),
                   "connected_components_ms": timed(lambda: ops.connected_components(labels, 8), a.reps, a.warmup),
                   "connected_components_4_ms": timed(lambda: ops.connected_components(labels, 4), a.reps, a.warmup),
                   "semantic_instances_ms": timed(lambda: segment.semantic_instances(labels), a.reps, a.warmup),
                   "panoptic_maps_ms": timed(lambda: segment.panoptic_maps(labels, center, offset), a.reps, a.warmup),
                   "scipy_label_host_ms": None, "frame_0_same_partition_as_scipy": None,
                   "ms_are": "median, min, max", "reps": a.reps, "warmup": a.warmup}
            res["scipy_label_host_ms"], res["frame_0_same_partition_as_scipy"] = scipy_host(labels, maps["components"], a.host_reps)
            res["Mpixel_per_ms_components"] = round(N * H * W / res["connected_components_ms"][0] / 1e6, 2)
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
