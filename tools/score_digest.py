"""SHA-256 digests of the raw bytes the score kernels return (csrc/quality.hip, csrc/flow_score.hip, csrc/score_rows.h), one line
per case, for comparing two builds of the library bit for bit:

    C2M_AMD_LIB=/path/to/other/libc2m_hip.so python tools/score_digest.py > a.txt
    python tools/score_digest.py > b.txt && diff a.txt b.txt

Every result here is bit-repeatable by design (fixed summation order, no atomics), so two builds that compute the same thing
print the same lines; a line that differs means a summation order or a per-pixel operation moved.  The inputs are the tool's
own (numpy default_rng, seeded per case).  Frame quality: ops.frame_quality at the tile edges of its 16 x 32 tile and at 18 and
36 tiles per frame (more than the reduce kernel's 16 slices), with and without region bytes.  Flow scores:
evaluate.flow_quality_sums and evaluate.flow_consistency_sums (maps=True: the sums and the three maps) from 1 pixel to 18 tiles
of 1024, 1 and 3 pairs, fp32 and bf16, 1 and 3 channels, with and without valid, regions and the reverse flow.  A tool, not a
test: it carries no threshold."""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import evaluate as E, ops  # noqa: E402

DEV = "cuda:0"
# (form, C, B, T, H, W)
QUALITY_CASES = [("f32", 3, 1, 1, 11, 11), ("f32", 1, 1, 1, 11, 12), ("f32", 3, 1, 1, 12, 11), ("u8", 3, 1, 1, 11, 11),
                 ("f32", 1, 2, 3, 15, 33), ("f32", 3, 2, 3, 16, 32), ("f32", 3, 1, 1, 17, 31), ("f32", 1, 1, 1, 33, 65),
                 ("f32", 3, 1, 1, 15, 65), ("f32", 1, 2, 3, 33, 31), ("u8", 3, 2, 3, 17, 33), ("u8", 3, 1, 1, 33, 65),
                 ("u8", 3, 1, 1, 16, 31), ("u8", 1, 2, 3, 15, 33), ("u8", 1, 1, 1, 32, 64), ("bf16", 3, 2, 3, 17, 33),
                 ("bf16", 1, 1, 1, 16, 65), ("f32", 1, 1, 1, 17, 257), ("u8", 3, 1, 1, 33, 353)]
FLOW_SHAPES = [(1, 1), (8, 8), (9, 13), (21, 37), (40, 70), (130, 140)]


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def quality_operands(form, C, B, T, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((B, C, T, H, W))
    y = np.clip(x + rng.normal(0, 0.08, x.shape), 0, 1)
    reg = torch.from_numpy(rng.integers(0, 256, (B, T, H, W)).astype(np.uint8))
    if form == "u8":
        cv = lambda a: torch.from_numpy(np.floor(a * 255 + 0.5).astype(np.uint8).transpose(0, 2, 3, 4, 1).copy())
    else:
        cv = lambda a: torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16 if form == "bf16" else torch.float32)
    return cv(x).to(DEV), cv(y).to(DEV), reg.to(DEV)


def flow_operands(H, W, N, C, seed):
    """Flows that stay inside, leave the frame and are not finite; targets with the invalid marker; a sparse valid."""
    rng = np.random.default_rng(seed)

    def flow(scale):
        f = rng.uniform(-scale, scale, (N, 2, H, W)).astype(np.float32)
        f = np.where(rng.random(f.shape) < 0.05, np.float32(1e4), f)
        f = np.where(rng.random(f.shape) < 0.02, np.float32(np.nan), f)
        return np.where(rng.random(f.shape) < 0.01, np.float32(np.inf), f).astype(np.float32)

    target = np.where(rng.random((N, 2, H, W)) < 0.03, np.float32(1e10), flow(12.0)).astype(np.float32)
    pred = (target + rng.normal(0, 2, target.shape)).astype(np.float32)
    x = dict(flow_ab=flow(3.0), flow_ba=flow(3.0), target=target, pred=pred,
             a=rng.uniform(-1, 2, (N, C, H, W)).astype(np.float32), b=rng.uniform(-1, 2, (N, C, H, W)).astype(np.float32),
             valid=((rng.random((N, H, W)) < 0.7) * rng.integers(1, 256, (N, H, W))).astype(np.uint8),
             regions=rng.integers(0, 256, (N, H, W)).astype(np.uint8))
    return {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("score_digest needs a GPU: it digests what the kernels return")
    for i, case in enumerate(QUALITY_CASES):
        x, y, reg = quality_operands(*case, seed=7000 + i)
        name = "-".join(str(v) for v in case)
        print(f"frame_quality {name} regions=0 {digest(ops.frame_quality(x, y))}")
        print(f"frame_quality {name} regions=1 {digest(ops.frame_quality(x, y, reg))}")
    for j, ((H, W), N, C) in enumerate(itertools.product(FLOW_SHAPES, (1, 3), (1, 3))):
        x = flow_operands(H, W, N, C, seed=9000 + j)
        for dt, use_valid, use_reg in itertools.product((torch.float32, torch.bfloat16), (0, 1), (0, 1)):
            name = f"{H}x{W} N={N} {str(dt)[6:]} valid={use_valid} regions={use_reg}"
            if C == 1:                                         # flow quality has no image operand: once per (shape, N)
                s = E.flow_quality_sums(x["pred"].to(dt), x["target"], x["valid"] if use_valid else None,
                                        x["regions"] if use_reg else None)
                print(f"flow_quality {name} {digest(s)}")
            if not use_valid:                                  # flow consistency takes no valid
                for use_ba in (0, 1):
                    s, m = E.flow_consistency_sums(x["flow_ab"], x["a"].to(dt), x["b"].to(dt), x["flow_ba"] if use_ba else None,
                                                   x["regions"] if use_reg else None, maps=True)
                    print(f"flow_consistency {name[:name.index(' valid')]} C={C} regions={use_reg} flow_ba={use_ba} "
                          f"{digest(s, m['photo'], m['fb'], m['inconsistent'])}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
