"""Device-event timing of evaluate.map_quality (csrc/map_quality.hip: panoptic-quality counts and the confusion matrix of a whole
clip in one call) next to the reference's formulation written with stock PyTorch operators on the same device.

    python tools/map_quality_bench.py [--iters 10] [--queue 20] [--out FILE]

Workload: a pair of int32 maps [5,1025,2049], the ground truth a synthetic Cityscapes-like layout (stuff bands, a void strip, a
few hundred numbered things per frame, a crowd region) and the prediction the same shifted by a few pixels, so most things match
and some do not.  The stock composite is the yardstick and lives here only (the package never falls back to it): one image at a
time, canonical keys with tensor arithmetic, torch.unique(return_counts=True) over the packed 64-bit keys and over each side's
keys, then the reference's host loops over the pairs and segments (after one copy of the unique keys to the host), and the
confusion matrix by torch.bincount.  The two are timed alternately in one process, warmed up first (two rounds), median of
--iters repetitions each.  In that alternation the kernel's call starts on an idle queue (the stock side has just copied to the
host), so its time includes the host's work to issue the call: its allocations and four launches.  --queue calls issued back to
back between two events, divided by their number, give the time per call with the queue kept busy (kernel_ms_back_to_back).
Prints one JSON line: milliseconds for both, their ratio, the bytes the kernel must read and the rate that makes (for both
kernel timings), tp / fp / fn per frame, and whether the two results agree exactly.  --out appends the line to a file.
A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import evaluate  # noqa: E402

P = evaluate.MAP_QUALITY


def stock_one(pred, gt):
    """One image by stock operators, in the reference's formulation -> tp, fp, fn [C] lists, iou [C] list, confusion [C+1,C+1]."""
    C, div, ign, things = P["num_classes"], P["label_divisor"], P["ignore_label"], set(P["thing_list"])

    def key(v):
        v = v.long().flatten()
        low = v < div
        cat = torch.where(low, v, v // div)
        n = torch.where(low, torch.zeros_like(v), v % div)
        void = (v < 0) | (cat == ign) | (cat >= C)
        return torch.where(void, torch.full_like(v, -1), cat * div + n)

    pk, gk = key(pred), key(gt)
    BIG = C * div + 1
    pairs, cnt = torch.unique((gk + 1) * BIG + (pk + 1), return_counts=True)
    pu, pc = torch.unique(pk, return_counts=True)
    gu, gc = torch.unique(gk, return_counts=True)
    pcls = torch.where(pk < 0, torch.full_like(pk, C), pk // div)
    gcls = torch.where(gk < 0, torch.full_like(gk, C), gk // div)
    conf = torch.bincount((C + 1) * pcls + gcls, minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    pairs, cnt, pu, pc, gu, gc = (t.tolist() for t in (pairs, cnt, pu, pc, gu, gc))      # the copies to the host
    inter = {(k // BIG - 1, k % BIG - 1): c for k, c in zip(pairs, cnt)}
    area_p = {k: c for k, c in zip(pu, pc) if k >= 0}
    area_g = {k: c for k, c in zip(gu, gc) if k >= 0}
    crowd = lambda g: (g // div) in things and g % div == 0
    tp, fp, fn, iou = [0] * C, [0] * C, [0] * C, [0.0] * C
    gm, pm = set(), set()
    for (g, p), it in inter.items():
        if g < 0 or p < 0 or crowd(g) or g // div != p // div:
            continue
        v = it / (area_p[p] + area_g[g] - it - inter.get((-1, p), 0))
        if v > 0.5:
            tp[g // div] += 1
            iou[g // div] += v
            gm.add(g)
            pm.add(p)
    for g in area_g:
        if g not in gm and not crowd(g):
            fn[g // div] += 1
    for p, a in area_p.items():
        if p in pm:
            continue
        cg = (p // div) * div
        if (inter.get((-1, p), 0) + (inter.get((cg, p), 0) if crowd(cg) else 0)) / a > 0.5:
            continue
        fp[p // div] += 1
    return tp, fp, fn, iou, conf


def workload(N, H, W, things, seed=0):
    g = torch.Generator().manual_seed(seed)
    stuff = torch.tensor([0, 1, 2, 8, 10])
    gt = torch.empty(N, H, W, dtype=torch.int32)
    for n in range(N):
        bands = stuff[(torch.arange(W) * len(stuff) // W + n) % len(stuff)].int()
        gt[n] = bands.view(1, W).expand(H, W)
        gt[n, : H // 3] = 10
        gt[n, -H // 20:] = 255                                              # the ego vehicle: void
        gt[n, H // 2: H // 2 + H // 16, : W // 6] = 13000                   # a crowd of cars
        count = {}
        for k in range(things):
            c = int(P["thing_list"][int(torch.randint(0, len(P["thing_list"]), (1,), generator=g))])
            count[c] = count.get(c, 0) + 1
            h, w = int(torch.randint(8, H // 8, (1,), generator=g)), int(torch.randint(8, W // 16, (1,), generator=g))
            y, x = int(torch.randint(0, H - h, (1,), generator=g)), int(torch.randint(0, W - w, (1,), generator=g))
            gt[n, y:y + h, x:x + w] = c * 1000 + count[c]
    pred = torch.roll(gt, shifts=(3, 5), dims=(1, 2))
    pred[:, :, :5] = 255
    return pred.cuda().contiguous(), gt.cuda().contiguous()


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


def timed_queue(fn, calls, iters):
    """Median milliseconds per call of `calls` calls issued back to back."""
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
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--queue", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--things", type=int, default=300)
    ap.add_argument("--shape", type=int, nargs=3, default=[5, 1025, 2049], metavar=("N", "H", "W"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_quality_bench needs a GPU: a timing taken anywhere else says nothing about it")
    N, H, W = a.shape
    pred, gt = workload(N, H, W, a.things)
    kernel = lambda: evaluate.map_quality(pred, gt)
    stock = lambda: [stock_one(pred[n], gt[n]) for n in range(N)]
    ms_kernel, ms_stock = timed_pair(kernel, stock, a.iters)
    ms_queue = timed_queue(kernel, a.queue, a.iters)
    got, want = kernel(), stock()
    host = {k: v.cpu() for k, v in got.items()}
    agree = all(host["tp"][n].tolist() == w[0] and host["fp"][n].tolist() == w[1] and host["fn"][n].tolist() == w[2] and
                host["iou"][n].tolist() == w[3] and torch.equal(host["confusion"][n], w[4].cpu()) for n, w in enumerate(want))
    nbytes = (pred.numel() + gt.numel()) * 4
    res = {"shape": [N, H, W], "bytes_read": nbytes, "kernel_ms": round(ms_kernel, 4), "kernel_GBps": round(nbytes / ms_kernel / 1e6, 1),
           "kernel_ms_back_to_back": round(ms_queue, 4), "kernel_back_to_back_GBps": round(nbytes / ms_queue / 1e6, 1),
           "stock_ms": round(ms_stock, 2), "stock_GBps": round(nbytes / ms_stock / 1e6, 2),
           "stock_over_kernel": round(ms_stock / ms_kernel, 1), "tp_fp_fn_per_frame": [[int(host[k][n].sum()) for k in ("tp", "fp", "fn")]
                                                                                      for n in range(N)],
           "overflow": host["overflow"].tolist(), "results_agree_exactly": bool(agree)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
