"""Writes tests/golden/resize_pil.npz: small inputs and what Pillow's Image.resize returns for them (bicubic, bilinear and
NEAREST; modes RGB, L and I), so that tests/test_resize_cpu.py pins the NumPy restatement of tests/resize_np.py to Pillow
without needing Pillow.

    python tools/capture_resize_golden.py

Inputs are noise with a 0/255 step edge drawn through it (the bicubic overshoot clips on both sides there)."""
import json
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "resize_pil.npz")
FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "nearest": Image.NEAREST}
# (mode, filter, (Hin, Win), (Hout, Wout))
CASES = [("RGB", "bicubic", (37, 53), (16, 24)), ("L", "bicubic", (40, 60), (64, 100)), ("RGB", "bicubic", (33, 41), (33, 20)),
         ("L", "bicubic", (64, 96), (47, 88)), ("RGB", "bilinear", (37, 53), (16, 24)), ("L", "bilinear", (40, 60), (64, 100)),
         ("L", "nearest", (37, 53), (16, 24)), ("L", "nearest", (40, 60), (64, 100)), ("I", "nearest", (33, 41), (33, 20)),
         ("I", "nearest", (64, 96), (47, 88))]


def main():
    rng = np.random.default_rng(2024)
    arrays, meta = {}, []
    for i, (mode, filt, (H, W), (h, w)) in enumerate(CASES):
        if mode == "I":
            x = rng.integers(0, 40001, (H, W)).astype(np.int32)
        else:
            x = rng.integers(0, 256, (H, W) + ((3,) if mode == "RGB" else ()), dtype=np.uint8)
            x[H // 4:H // 2, :W // 3] = 0
            x[H // 4:H // 2, W // 3:2 * W // 3] = 255
        out = np.asarray(Image.fromarray(x, mode=mode).resize((w, h), FILTERS[filt]))
        arrays[f"in{i}"], arrays[f"out{i}"] = x, out
        meta.append({"mode": mode, "filter": filt, "size": [h, w]})
    arrays["meta"] = np.frombuffer(json.dumps({"pillow": PIL.__version__, "cases": meta}).encode(), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
