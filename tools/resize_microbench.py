"""Device-event timing of ops.resize_bilinear_grad (c2m_resize_bilinear forward, c2m_resize_bilinear_bwd backward) on the
model's largest instance, next to a torch copy_ of the same number of bytes.

    python tools/resize_microbench.py [--planes 1280] [--hi 184 --wi 352 --ho 188 --wo 352] [--dtype f32|bf16]

Default: the generator's final resize at BASELINE width, B 8 x 5 frames x 32 channels = 1280 planes, 184x352 -> 188x352.
Prints one JSON line: median microseconds and achieved GB/s (bytes read + written once) of fwd, bwd and the copy."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops, _lib  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=1280)
    ap.add_argument("--hi", type=int, default=184)
    ap.add_argument("--wi", type=int, default=352)
    ap.add_argument("--ho", type=int, default=188)
    ap.add_argument("--wo", type=int, default=352)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.bfloat16
    dev = torch.device("cuda", 0)
    x = torch.randn(a.planes, a.hi, a.wi, device=dev).to(dt).view(1, a.planes, a.hi, a.wi)
    y = torch.empty(1, a.planes, a.ho, a.wo, device=dev, dtype=dt)
    gy = torch.randn_like(y)
    gx = torch.empty_like(x)
    L, s = _lib.lib(), ops._stream
    code = 1 if dt == torch.bfloat16 else 0

    def fwd():
        _lib.check(L.c2m_resize_bilinear(ops._p(x), ops._p(y), a.planes, a.hi, a.wi, a.ho, a.wo, 0, 0.0, code, s()), "fwd")

    def bwd():
        _lib.check(L.c2m_resize_bilinear_bwd(ops._p(gy), ops._p(gx), a.planes, a.hi, a.wi, a.ho, a.wo, 0, code, s()), "bwd")

    esz = x.element_size()
    nbytes = (x.numel() + y.numel()) * esz
    src = torch.empty((x.numel() + y.numel()) // 2, device=dev, dtype=dt)
    dst = torch.empty_like(src)
    res = {"planes": a.planes, "in": [a.hi, a.wi], "out": [a.ho, a.wo], "dtype": a.dtype, "bytes": nbytes}
    for name, fn in (("fwd", fwd), ("bwd", bwd), ("copy", lambda: dst.copy_(src))):
        us = timed(fn, a.iters)
        res[name + "_us"] = round(us, 2)
        res[name + "_GBps"] = round(nbytes / us / 1e3, 1)
    # the model's call through autograd (allocations + Python included), for scale
    xg = x.detach().requires_grad_(True)
    res["op_fwd_bwd_us"] = round(timed(lambda: ops.resize_bilinear_grad(xg, (a.ho, a.wo)).backward(gy), a.iters), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
