"""Device-event timing of ops.panoptic_maps (csrc/panoptic.hip: Panoptic-DeepLab's post-processing for a whole clip in one call) next
to the reference's formulation written with stock PyTorch operators on the same device.

    python tools/panoptic_bench.py [--iters 10] [--chunk 0] [--out FILE]

Workload: the heads of one clip at the size the network runs at, logits [5,19,1025,2049], about 200 centres per frame, offsets
that point at the nearest planted centre plus noise, labels in blobs.  The stock composite is the yardstick and lives here only
(the package never falls back to it): per image, argmax, threshold + max-pool NMS + top-k, the [K, H*W, 2] difference tensor
with torch.norm and argmin (--chunk K' computes it K' centres at a time with a running minimum; 0: all at once, 3.4 GB at K =
200), then the host loops over instance ids and classes with a synchronisation each.  The two are timed alternately in one
process, warmed up first, median of --iters repetitions each.  Prints one JSON line: milliseconds for both, their ratio, the
bytes the kernels must read and the rate that makes, centres per frame, and the number of pixels on which the two results
differ.  --out appends the line to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops, segment  # noqa: E402

P = segment.CITYSCAPES


def stock_one(logits, center, offset, chunk):
    """One image by stock operators, in the reference's formulation -> (semantic, panoptic, instance image) int64 [H,W]."""
    things, div, void = list(P["thing_list"]), P["label_divisor"], P["ignore_label"] * P["label_divisor"]
    sem = logits.argmax(0)
    H, W = sem.shape
    heat = F.threshold(center.reshape(1, 1, H, W), P["threshold"], -1.0)
    r = P["nms_kernel"] // 2
    heat = torch.where(heat == F.max_pool2d(heat, P["nms_kernel"], 1, r), heat, torch.full_like(heat, -1.0)).reshape(H, W)
    ctr = torch.nonzero(heat > 0)
    if ctr.shape[0] >= P["top_k"]:
        kth = torch.topk(heat.flatten(), P["top_k"])[0][-1]
        ctr = torch.nonzero(heat > kth)
    is_thing = torch.zeros_like(sem)
    for c in things:
        is_thing[sem == c] = 1
    ins = torch.zeros_like(sem)
    if ctr.shape[0]:
        yy = torch.arange(H, device=sem.device, dtype=offset.dtype).view(H, 1).expand(H, W)
        xx = torch.arange(W, device=sem.device, dtype=offset.dtype).view(1, W).expand(H, W)
        loc = (torch.stack([yy, xx]) + offset).reshape(2, H * W).t().unsqueeze(0)          # [1, HW, 2]
        step = chunk or ctr.shape[0]
        best = arg = None
        for k0 in range(0, ctr.shape[0], step):
            d = torch.norm(ctr[k0:k0 + step].unsqueeze(1) - loc, dim=-1)                   # [K', HW]
            dmin, amin = d.min(0)
            if best is None:
                best, arg = dmin, amin
            else:
                closer = dmin < best
                best, arg = torch.where(closer, dmin, best), torch.where(closer, amin + k0, arg)
        ins = (arg.reshape(H, W) + 1) * is_thing
    pan = torch.full_like(sem, void)
    used = {}
    for i in torch.unique(ins):
        if i == 0:
            continue
        mask = ins == i
        cls = int(torch.mode(sem[mask])[0].item())
        used[cls] = used.get(cls, 0) + 1
        pan[mask] = cls * div + used[cls]
    for c in torch.unique(sem):
        if c.item() in things:
            continue
        mask = (sem == c) & (ins == 0)
        if int(mask.sum().item()) >= P["stuff_area"]:
            pan[mask] = c * div
    cls_of = pan // div
    thing = torch.zeros_like(pan)
    for c in things:
        thing[cls_of == c] = 1
    return sem, pan, cls_of * (1 - thing) + pan * thing


def workload(N, C, H, W, K, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
    classes = torch.tensor([0, 1, 2, 8, 10, 11, 12, 13, 13, 13, 11, 18], device="cuda")
    coarse = classes[(rnd(N, 1, H // 32 + 1, W // 32 + 1) * len(classes)).long().clamp_(max=len(classes) - 1)]
    labels = F.interpolate(coarse.float(), size=(H, W), mode="nearest").long()[:, 0]
    logits = torch.randn(N, C, H, W, device="cuda", generator=g)
    logits.scatter_add_(1, labels.unsqueeze(1), torch.full((N, 1, H, W), 6.0, device="cuda"))
    center = rnd(N, 1, H, W) * 0.05
    offset = torch.empty(N, 2, H, W, device="cuda")
    yy = torch.arange(H, device="cuda", dtype=torch.float32).view(H, 1).expand(H, W)
    xx = torch.arange(W, device="cuda", dtype=torch.float32).view(1, W).expand(H, W)
    for n in range(N):
        gy, gx = H // 10, W // 20                                                          # one centre per cell of a 10 x 20 grid
        cy = (torch.arange(10, device="cuda").view(10, 1) * gy + 4 + (rnd(10, 20) * max(gy - 8, 1)).long()).flatten()[:K]
        cx = (torch.arange(20, device="cuda").view(1, 20) * gx + 4 + (rnd(10, 20) * max(gx - 8, 1)).long()).flatten()[:K]
        center[n, 0, cy, cx] = 0.3 + 0.6 * rnd(cy.numel())
        near = torch.cdist(torch.stack([yy, xx], -1).reshape(-1, 2), torch.stack([cy, cx], -1).float()).argmin(1)
        offset[n, 0] = cy[near].reshape(H, W) - yy
        offset[n, 1] = cx[near].reshape(H, W) - xx
    offset += torch.randn(N, 2, H, W, device="cuda", generator=g) * 1.5
    return logits, center, offset


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
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, nargs=4, default=[5, 19, 1025, 2049], metavar=("N", "C", "H", "W"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panoptic_bench needs a GPU: a timing taken anywhere else says nothing about it")
    N, C, H, W = a.shape
    logits, center, offset = workload(N, C, H, W, 200)
    params = dict(P)
    kernel = lambda: ops.panoptic_maps(logits, center, offset, **params)
    stock = lambda: [stock_one(logits[n], center[n], offset[n], a.chunk) for n in range(N)]
    ms_kernel, ms_stock = timed_pair(kernel, stock, a.iters)
    got, want = kernel(), stock()
    differ = [sum(int((g[n].long() != w).sum()) for g, w in zip((got["semantic"], got["panoptic"], got["instance"]), want[n]))
              for n in range(N)]
    nbytes = (logits.numel() + center.numel() + offset.numel()) * 4
    res = {"shape": [N, C, H, W], "centres_per_frame": got["center_count"].tolist(), "bytes_read": nbytes,
           "kernel_ms": round(ms_kernel, 3), "kernel_GBps": round(nbytes / ms_kernel / 1e6, 1), "stock_ms": round(ms_stock, 2),
           "stock_chunk": a.chunk, "stock_over_kernel": round(ms_stock / ms_kernel, 1), "pixels_differing_per_frame": differ}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
