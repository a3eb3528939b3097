"""Times of the bf16 weight-gradient kernels (the 16-byte-load forms, conv_wgrad_wide_bf16_kernel, where the plan picks them) on
bench shapes, bf16 tensors.  usage: python tools/ab_bf16_wgrad.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(40, 256, 16, 32, 256, "reflect", 2), (40, 128, 64, 128, 128, "reflect", 2), (40, 32, 128, 256, 32, "reflect", 2),
          (40, 64, 64, 128, 128, "reflect", 2), (40, 128, 32, 64, 128, "zeros", 2), (8, 34, 128, 256, 32, "reflect", 3),
          (40, 64, 128, 256, 32, "reflect", 2), (40, 256, 32, 64, 128, "reflect", 2)]
sys.path.insert(0, ROOT)
import torch
from c2m_amd import ops
ops.set_conv_precision("bf16")
for (N, Cin, H, W, Cout, mode, nd) in SHAPES:
    xs = (N, Cin, H, W) if nd == 2 else (N, Cin, 5, H, W)
    x = torch.randn(*xs, device="cuda:0").bfloat16()
    w = (torch.randn(Cout, Cin, *([3] * nd), device="cuda:0") / (Cin * 3 ** nd) ** 0.5).requires_grad_(True)
    y = ops.conv(x, w, None, stride=1, padding=1, padding_mode=mode)
    go = torch.randn_like(y)
    with ops.ConvProfiler() as prof:
        for _ in range(30):
            y = ops.conv(x, w, None, stride=1, padding=1, padding_mode=mode)
            y.backward(go)
            w.grad = None
    for tag, n, ms, tf in prof.table():
        if tag[1] == "wgrad":
            print((N, Cin, H, W, Cout, mode, nd), f"{ms / n * 1000:.1f} us  {tf:.1f} TF/s", flush=True)
