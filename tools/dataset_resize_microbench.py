"""Device-event timing of data.resize_frames (c2m_resize_u8, Pillow's bicubic bit for bit) on one training step's worth of
full-resolution frames, next to the same job in Pillow on the host and a stock-torch composite on the device.

    python tools/dataset_resize_microbench.py [--frames 56] [--src 1024x2048] [--dst 128x256] [--iters 30] [--pil-frames 4]

Default: 56 frames (BASELINE configs[1]: 8 samples x 7 frames) of 1024x2048x3 -> 128x256.  (tools/resize_microbench.py times the
model's in-network bilinear resize, another kernel.)  Prints one JSON line: median microseconds, the rate at which the source
bytes are consumed, and that rate over the 8.0 TB/s HBM3E peak and over the 6.29 TB/s a float4 copy reaches on this part;
the source-sized copy_ measured here for scale; Pillow's milliseconds per frame on one host core; and the torch composite
(uint8 -> float NCHW -> F.interpolate(bicubic, antialias=True) -> round, clamp, uint8 NHWC), which is NOT bit-equal to Pillow
(its maximum difference from the kernel's output is printed)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import data  # noqa: E402

HBM_PEAK_TBPS, HBM_COPY_TBPS = 8.0, 6.29


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


def torch_composite(x, size):
    f = x.permute(0, 3, 1, 2).float()
    y = F.interpolate(f, size=size, mode="bicubic", antialias=True, align_corners=False)
    return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=56)
    ap.add_argument("--src", default="1024x2048")
    ap.add_argument("--dst", default="128x256")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--pil-frames", type=int, default=4)
    a = ap.parse_args()
    H, W = (int(v) for v in a.src.split("x"))
    h, w = (int(v) for v in a.dst.split("x"))
    g = torch.Generator().manual_seed(0)
    # smooth image + noise: like a photograph, the bicubic overshoot rarely clips
    base = F.interpolate(torch.rand(a.frames, 3, H // 16, W // 16, generator=g), size=(H, W), mode="bilinear")
    frames = (base * 200 + torch.rand(a.frames, 3, H, W, generator=g) * 55).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    x = frames.cuda()
    nbytes = x.numel()
    res = {"frames": a.frames, "src": [H, W], "dst": [h, w], "source_bytes": nbytes}
    us = timed(lambda: data.resize_frames(x, (h, w)), a.iters)
    res["resize_u8_us"] = round(us, 1)
    res["resize_u8_source_GBps"] = round(nbytes / us / 1e3, 1)
    res["fraction_of_hbm_peak"] = round(nbytes / us / 1e6 / HBM_PEAK_TBPS, 3)
    res["fraction_of_hbm_copy_rate"] = round(nbytes / us / 1e6 / HBM_COPY_TBPS, 3)
    dst = torch.empty_like(x)
    us = timed(lambda: dst.copy_(x), a.iters)
    del dst
    res["copy_us"] = round(us, 1)
    res["copy_GBps"] = round(2 * nbytes / us / 1e3, 1)
    us = timed(lambda: torch_composite(x, (h, w)), max(a.iters // 3, 3), warmup=2)
    res["torch_composite_us"] = round(us, 1)
    diff = (torch_composite(x[:2], (h, w)).int() - data.resize_frames(x[:2], (h, w)).int()).abs()
    res["torch_composite_max_abs_diff"] = int(diff.max())
    res["torch_composite_values_differing"] = round(float((diff > 0).float().mean()), 4)
    try:
        from PIL import Image
    except ImportError:
        res["pil_ms_per_frame"] = None
    else:
        t = []
        for i in range(min(a.pil_frames, a.frames)):
            im = Image.fromarray(frames[i].numpy())
            t0 = time.perf_counter()
            out = im.resize((w, h), Image.BICUBIC)
            t.append(time.perf_counter() - t0)
        res["pil_ms_per_frame"] = round(sorted(t)[len(t) // 2] * 1e3, 2)
        res["pil_ms_for_the_job_one_core"] = round(res["pil_ms_per_frame"] * a.frames, 1)
        res["bit_equal_to_pil"] = bool(np.array_equal(np.asarray(out), data.resize_frames(x[i:i + 1], (h, w))[0].cpu().numpy()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
