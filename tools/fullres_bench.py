"""Device-event timing of ops.detail_warp (c2m_detail_warp: predicted frames at dataset resolution, one fused pass) next to
the same composite assembled from stock PyTorch operators on the device.

    python tools/fullres_bench.py [--work 128x256] [--full 1024x2048] [--batch 1] [--frames 5] [--iters 50] [--out FILE]

Default: the workload's own factor 8, (128, 256) -> (1024, 2048), B = 1, T = 5.  The two are timed alternately in one process,
warmed up first, median of --iters repetitions each.  The stock composite is F.interpolate (bilinear) of the four working-size
tensors, F.grid_sample of the float frame on an explicit grid, and the element-wise tail down to uint8 [B,T,H,W,3]; it lives
here only, the package never falls back to it.  Prints one JSON line: milliseconds, and bytes written plus compulsory bytes
read (every input once) per second, for both -- to be read beside the 3.5-5.9 TB/s ATen's strided copies reach on this part
(profiles/r05_copy_kernel_vs_aten_microbench.txt); the two outputs' largest difference is printed too (they round
differently at ties).  --out appends the line to a file."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops  # noqa: E402
from c2m_amd.modules.layers.common import fold_time  # noqa: E402


def stock_composite(frame_u8, gen, warped, flow, occ):
    B, _, T, h, w = gen.shape
    H, W = frame_u8.shape[1:3]
    up = lambda a: F.interpolate(fold_time(a), size=(H, W), mode="bilinear", align_corners=False)      # [T*B,C,H,W]
    g, wl, fl, oc = up(gen), up(warped), up(flow), up(occ)
    xl = (torch.arange(W, device=gen.device, dtype=torch.float32) + 0.5) * (w / W) - 0.5
    yl = (torch.arange(H, device=gen.device, dtype=torch.float32) + 0.5) * (h / H) - 0.5
    ix = (xl[None, None, :] + fl[:, 0]) * (W / (w - 1)) - 0.5
    iy = (yl[None, :, None] + fl[:, 1]) * (H / (h - 1)) - 0.5
    grid = torch.stack([(ix + 0.5) * (2.0 / W) - 1.0, (iy + 0.5) * (2.0 / H) - 1.0], -1)               # [T*B,H,W,2]
    f = frame_u8.permute(0, 3, 1, 2).float().repeat(T, 1, 1, 1)                                        # frame-major, as fold_time
    wf = F.grid_sample(f, grid, mode="bilinear", padding_mode="border", align_corners=False)
    v = 255.0 * g + oc * (wf - 255.0 * wl)
    lv = (v.clamp_(0, 255) + 0.5).floor_().to(torch.uint8)                                             # [T*B,3,H,W]
    return lv.reshape(T, B, 3, H, W).permute(1, 0, 3, 4, 2).contiguous()


def timed_pair(fa, fb, iters, warmup=5):
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
    ap.add_argument("--work", default="128x256")
    ap.add_argument("--full", default="1024x2048")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fullres_bench needs a GPU: a timing taken anywhere else says nothing about it")
    h, w = (int(v) for v in a.work.split("x"))
    H, W = (int(v) for v in a.full.split("x"))
    B, T = a.batch, a.frames
    g = torch.Generator().manual_seed(0)
    base = F.interpolate(torch.rand(B, 3, H // 16, W // 16, generator=g), size=(H, W), mode="bilinear")
    frame = (base * 200 + torch.rand(B, 3, H, W, generator=g) * 55).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    flow = (torch.randn(B, 2, T, h, w, generator=g) * 1.5).cuda()
    occ = torch.rand(B, 1, T, h, w, generator=g).cuda()
    small = F.interpolate(frame.permute(0, 3, 1, 2).float() / 255, size=(h, w), mode="bilinear", antialias=True)
    rep = small.unsqueeze(0).expand(T, B, 3, h, w).reshape(T * B, 3, h, w)
    warped = ops.flow_warp(rep, fold_time(flow)).reshape(T, B, 3, h, w).permute(1, 2, 0, 3, 4).contiguous()
    gen = (warped + torch.randn(warped.shape, generator=g).cuda() * 0.05).clamp_(0, 1)
    fused = lambda: ops.detail_warp(frame, gen, warped, flow, occ)[0]
    stock = lambda: stock_composite(frame, gen, warped, flow, occ)
    ms_fused, ms_stock = timed_pair(fused, stock, a.iters)
    nbytes = B * T * H * W * 3 + frame.numel() + 4 * (gen.numel() + warped.numel() + flow.numel() + occ.numel())
    d = (fused().int() - stock().int()).abs()
    res = {"work": [h, w], "full": [H, W], "B": B, "T": T, "bytes_written_plus_compulsory_read": nbytes,
           "fused_ms": round(ms_fused, 4), "fused_GBps": round(nbytes / ms_fused / 1e6, 1),
           "stock_ms": round(ms_stock, 4), "stock_GBps": round(nbytes / ms_stock / 1e6, 1),
           "stock_over_fused": round(ms_stock / ms_fused, 2),
           "max_abs_diff_levels": int(d.max()), "values_differing": round(float((d > 0).float().mean()), 5)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
