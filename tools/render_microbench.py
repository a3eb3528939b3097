"""Times the rendering kernels (csrc/render.hip) with HIP events: warm-up, then the median of --iters timed launches.

Per kernel, at B 8 x T 15 x 128 x 256 (a three-segment rollout) and at B 2 x T 2 x 1024 x 2048: ms and TB/s of the bytes it
reads and writes, beside (a) copy_ of the same number of bytes, (b) the same sheet built from stock torch device ops
(mul / clamp / to(uint8) / permute / reshape) and, for the flow, (c) the numpy float64 route including the device -> host
copy.  Prints one JSON line per measurement.   python tools/render_microbench.py [--iters 30]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops, visual  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def torch_sheet(x, cols):
    """What a user of stock torch writes: [B,C,T,H,W] -> uint8 [T, H, B*W, C] (one row of cells)."""
    B, C, T, H, W = x.shape
    return (x * 255.0).clamp(0, 255).to(torch.uint8).permute(2, 3, 0, 4, 1).reshape(T, H, B * W, C)


def numpy_flow(flow):
    f = flow.cpu().numpy().astype(np.float64)
    B, _, T, H, W = f.shape
    u = f[:, 0].transpose(1, 2, 0, 3).reshape(T, H, B * W)
    v = f[:, 1].transpose(1, 2, 0, 3).reshape(T, H, B * W)
    rad = np.sqrt(u * u + v * v)
    m = rad.reshape(T, -1).max(1)[:, None, None]
    u, v = u / m, v / m
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * 54 + 1
    k0 = np.floor(fk).astype(int)
    return (255 * (fk - k0)).astype(np.uint8), rad                         # the blend itself left out: a lower bound of the route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = "cuda:0"
    for B, T, H, W in ((8, 15, 128, 256), (2, 2, 1024, 2048)):
        px = B * T * H * W
        g = torch.Generator().manual_seed(0)
        frames = torch.rand(B, 3, T, H, W, generator=g).to(dev)
        occ = torch.rand(B, 1, T, H, W, generator=g).to(dev)
        flow = (torch.randn(B, 2, T, H, W, generator=g) * 5).to(dev)
        ids = (torch.randint(0, 20, (B, 1, T, H // 8, W // 8), generator=g) * 1000 + 1).repeat_interleave(8, 3) \
            .repeat_interleave(8, 4).to(torch.int32).to(dev)
        size = (1, B)
        sheet = ops.render_frames(frames, size)
        pal = visual.default_palette().to(dev)
        boxes = torch.tensor([20, 30, 90, 100], dtype=torch.int32).expand(B, 8, T, 4).contiguous().to(dev)
        pres = torch.ones(B, 8, T, dtype=torch.bool, device=dev)
        bcol = torch.full((B, 8, 3), 255, dtype=torch.uint8, device=dev)
        pts = torch.tensor([[10, 10], [60, 40], [100, 90], [120, 20]], dtype=torch.int32).expand(B, 4, 2).contiguous().to(dev)
        smp = torch.arange(B, dtype=torch.int32, device=dev)
        cnt = torch.full((B, T), 4, dtype=torch.int32, device=dev)
        cases = [("render_frames C=3", lambda: ops.render_frames(frames, size), 15 * px, lambda: torch_sheet(frames, B)),
                 ("render_frames C=3 bf16", (lambda fb: lambda: ops.render_frames(fb, size))(frames.bfloat16()), 9 * px, None),
                 ("render_frames C=1", lambda: ops.render_frames(occ, size), 5 * px, lambda: torch_sheet(occ, B)),
                 ("render_flow sheet", lambda: ops.render_flow(flow, size), 19 * px, None),       # flow read twice (maximum pass)
                 ("render_flow fixed", lambda: ops.render_flow(flow, size, 3.0), 11 * px, None),
                 ("render_instances", lambda: ops.render_instances(ids, size, pal, sheet), 10 * px, None),
                 ("draw_overlays 8 boxes + 1 path", lambda: ops.draw_overlays(sheet, size, boxes, pres, bcol, pts, smp, cnt, bcol[:, 0]),
                  None, None)]
        for name, fn, nbytes, stock in cases:
            row = dict(shape=[B, T, H, W], kernel=name, ms=round(timed(fn, args.iters), 4))
            if nbytes:
                row["tb_s"] = round(nbytes / row["ms"] / 1e9, 3)
                src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                row["copy_same_bytes_ms"] = round(timed(lambda: dst.copy_(src), args.iters), 4)
            if stock:
                row["stock_torch_ms"] = round(timed(stock, args.iters), 4)
            if name == "render_flow sheet":
                t0 = time.perf_counter()
                numpy_flow(flow)
                row["numpy_float64_route_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
