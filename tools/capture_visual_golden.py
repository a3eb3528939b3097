"""Captures tests/golden/vis_reference.npz from the live reference (build container only; the fixture is data).

Seeded inputs at B 4 x T 2 x 16 x 24 and what the reference's own tensor2im (both normalize values), tensor2occ, tensor2flow
and compute_flow_color_map return for them, through oracle.ref_shims (which stands in for the absent cv2 / imageio).
Run from the repository root:  python tools/capture_visual_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shims  # noqa: E402


def main():
    ref_utils = ref_shims.install()
    ref_vis = ref_shims.import_reference("utils.utils")
    ref_ops = ref_shims.import_reference("utils.ops")
    rng = np.random.default_rng(20240607)
    B, T, H, W = 4, 2, 16, 24
    size = [2, 3]                                                   # two empty cells
    frames = rng.uniform(-0.2, 1.2, (B, 3, T, H, W)).astype(np.float32)
    frames.reshape(-1)[:256] = np.arange(256, dtype=np.float32) / np.float32(255)          # every level
    frames_pm = (frames * 2 - 1).astype(np.float32)
    occ = rng.uniform(-0.1, 1.1, (B, 1, T, H, W)).astype(np.float32)
    flow = (rng.standard_normal((B, 2, T, H, W)) * 5).astype(np.float32)
    flow[1, 0, 0, 3, 4:7] = 2e7                                     # unknown components
    flow[2, 1, 1, 5, 5] = -3e9
    flow[3, :, 1] *= 4                                              # one sample holds frame 1's maximum
    flow[0, :, 0, :2] *= 0.01                                       # radii below 1 in the fixed-scale mode
    t = torch.from_numpy
    out = dict(size=np.array(size), frames=frames, frames_pm=frames_pm, occ=occ, flow=flow,
               im=ref_vis.tensor2im(t(frames), size=size), im_normalize=ref_vis.tensor2im(t(frames_pm), normalize=True, size=size),
               occ_sheet=ref_vis.tensor2occ(t(occ), size=size), flow_sheet=ref_vis.tensor2flow(t(flow), size),
               # save_flows' call: one float32 HWC frame of one sample at a time
               flow_fixed=np.stack([np.stack([np.uint8(ref_ops.compute_flow_color_map(flow[b, :, k].transpose(1, 2, 0).copy()))
                                              for k in range(T)]) for b in range(B)]))
    for k, v in out.items():
        print(k, v.dtype, v.shape)
    path = os.path.join(ROOT, "tests", "golden", "vis_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
