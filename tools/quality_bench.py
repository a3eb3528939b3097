"""Device-event timing of ops.frame_quality (c2m_frame_quality: per-frame squared error and Gaussian-window SSIM sums, fp64) next
to the same formula assembled from stock PyTorch operators on the device.

    python tools/quality_bench.py [--iters 30] [--out FILE]

Two workloads: float [8,3,5,128,256] (a working-size batch) and uint8 [1,5,1024,2048,3] (one clip at dataset resolution), both
with region bytes.  The stock composite is the yardstick: the five moments by depthwise conv2d with the 11-tap kernels (rows,
then columns) in fp64, the SSIM map, and masked sums for the whole frame and the eight region bits; it lives here only, the
package never falls back to it.  The two are timed alternately in one process, warmed up first, median of --iters repetitions
each.  Prints one JSON line per workload: milliseconds for both, their ratio, the bytes the kernel must read (both operands and
the regions, once) and the rate that makes; the largest difference between the two results is printed too.  --out appends the
lines to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops  # noqa: E402


def stock_composite(pred, target, regions):
    """-> float64 [B,T,9,4] by stock operators, fp64 throughout."""
    if pred.dtype == torch.uint8:
        x, y, L = pred.permute(0, 1, 4, 2, 3).double(), target.permute(0, 1, 4, 2, 3).double(), 255.0      # [B,T,C,H,W]
    else:
        x, y, L = pred.permute(0, 2, 1, 3, 4).double(), target.permute(0, 2, 1, 3, 4).double(), 1.0
    B, T, C, H, W = x.shape
    w = torch.from_numpy(ops.quality_weights()).to(x.device)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    planes = torch.stack([x, y, x * x, y * y, x * y], 2).reshape(B * T, 5 * C, H, W)
    k = w.reshape(1, 1, 1, -1).expand(5 * C, 1, 1, -1)
    m = F.conv2d(F.conv2d(planes, k, groups=5 * C), k.transpose(2, 3), groups=5 * C).reshape(B, T, 5, C, H - 10, W - 10)
    ux, uy, xx, yy, xy = m.unbind(2)
    s = ((2 * ux * uy + C1) * (2 * (xy - ux * uy) + C2)) / ((ux * ux + uy * uy + C1) * (xx - ux * ux + yy - uy * uy + C2))
    s = s.mean(2)                                                                  # [B,T,H-10,W-10]
    se = ((x - y) ** 2).sum(2)                                                     # [B,T,H,W]
    bits = torch.arange(8, device=x.device).view(1, 1, 8, 1, 1)
    mask = torch.cat([torch.ones_like(regions).unsqueeze(2), (regions.unsqueeze(2) >> bits) & 1], 2).double()   # [B,T,9,H,W]
    mc = mask[..., 5:H - 5, 5:W - 5]
    return torch.stack([mask.sum((3, 4)), (mask * se.unsqueeze(2)).sum((3, 4)), mc.sum((3, 4)),
                        (mc * s.unsqueeze(2)).sum((3, 4))], -1)


def timed_pair(fa, fb, iters, warmup=3):
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


def workload(form, B, C, T, H, W):
    g = torch.Generator().manual_seed(0)
    base = F.interpolate(torch.rand(B * T, C, H // 16, W // 16, generator=g), size=(H, W), mode="bilinear")
    x = (base * 0.8 + torch.rand(B * T, C, H, W, generator=g) * 0.2).reshape(B, T, C, H, W)
    y = (x + torch.randn(x.shape, generator=g) * 0.05).clamp_(0, 1)
    regions = torch.randint(0, 16, (B, T, H, W), generator=g, dtype=torch.uint8).cuda()
    if form == "uint8":
        cv = lambda a: (a * 255).round().to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous().cuda()
    else:
        cv = lambda a: a.permute(0, 2, 1, 3, 4).contiguous().cuda()
    return cv(x), cv(y), regions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench needs a GPU: a timing taken anywhere else says nothing about it")
    for form, B, C, T, H, W in (("float", 8, 3, 5, 128, 256), ("uint8", 1, 3, 5, 1024, 2048)):
        x, y, regions = workload(form, B, C, T, H, W)
        kernel = lambda: ops.frame_quality(x, y, regions)
        stock = lambda: stock_composite(x, y, regions)
        ms_kernel, ms_stock = timed_pair(kernel, stock, a.iters)
        nbytes = x.numel() * x.element_size() * 2 + regions.numel()
        got, want = kernel(), stock()
        nw = want[..., 2].clamp(min=1)
        res = {"form": form, "shape": list(x.shape), "bytes_read": nbytes, "kernel_ms": round(ms_kernel, 4),
               "kernel_GBps": round(nbytes / ms_kernel / 1e6, 1), "stock_ms": round(ms_stock, 4),
               "stock_over_kernel": round(ms_stock / ms_kernel, 2),
               "max_abs_diff_mean_ssim": float(((got[..., 3] - want[..., 3]).abs() / nw).max()),
               "max_rel_diff_sse": float(((got[..., 1] - want[..., 1]).abs() / want[..., 1].clamp(min=1e-300)).max())}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del x, y, regions
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
