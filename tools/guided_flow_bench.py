"""Device-event timing of the segment-guided dense flow (c2m_amd.flow.dense_flow(segments=...)) next to the
unguided call on the same frames, with the protocol of tools/dense_flow_bench.py.

    python tools/guided_flow_bench.py [--pairs 96] [--size 128 256] [--iters 20] [--warmup 3] [--unguided-only] [--out FILE]

The 96 pairs at 128 x 256 are those of a B = 8 step with 2 input and 5 predicted frames.  Frames: dense_flow_bench's 1/f texture
moved by (3, -2) px.  Ids: per pair, smooth noise cut into six labels (blobs of some tens of pixels across, so that a good share
of the patches holds an id border); `constant` is one id everywhere, the case whose result is the unguided one bit for bit.
The calls are timed alternately in one process after --warmup rounds, HIP events around each call; median, minimum and maximum
of --iters repetitions.  --unguided-only times the two unguided calls alone (it runs on a tree without `segments`, for a
before / after comparison of the unguided kernels).  Prints one JSON line; --out appends it to a file.  A tool, not a test: it
carries no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import flow as F  # noqa: E402
from dense_flow_bench import frames, timed  # noqa: E402


def blob_ids(n, H, W, labels=6, seed=1):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, 1, -(-H // 16) + 2, -(-W // 16) + 2, generator=g)
    f = torch.nn.functional.interpolate(c, scale_factor=16, mode="bicubic", align_corners=False)[:, 0, 16:16 + H, 16:16 + W].contiguous()
    cuts = torch.quantile(f.flatten(), torch.linspace(0, 1, labels + 1)[1:-1])
    return torch.bucketize(f, cuts).to(torch.int32).contiguous().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=96)
    ap.add_argument("--size", type=int, nargs=2, default=(128, 256))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--unguided-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guided_flow_bench needs a GPU: a timing taken anywhere else says nothing about it")
    H, W = a.size
    A, B = frames(a.pairs, H, W)
    names = ["dense_flow", "dense_flow_refined"]
    fns = [lambda: F.dense_flow(A, B, value_range=(-1, 1)), lambda: F.dense_flow(A, B, value_range=(-1, 1), refine=True)]
    res = {"pairs": a.pairs, "size": [H, W], "levels": len(F.pyramid_sizes(H, W)), "iters": a.iters}
    if not a.unguided_only:
        ids, one = blob_ids(a.pairs, H, W), torch.zeros(a.pairs, H, W, dtype=torch.int32, device="cuda")
        names += ["dense_flow_guided", "dense_flow_refined_guided", "dense_flow_constant_ids", "dense_flow_refined_constant_ids"]
        fns += [lambda: F.dense_flow(A, B, value_range=(-1, 1), segments=ids),
                lambda: F.dense_flow(A, B, value_range=(-1, 1), refine=True, segments=ids),
                lambda: F.dense_flow(A, B, value_range=(-1, 1), segments=one),
                lambda: F.dense_flow(A, B, value_range=(-1, 1), refine=True, segments=one)]
        res["constant_ids_bit_identical"] = bool(torch.equal(fns[4](), fns[0]()) and torch.equal(fns[5](), fns[1]()))
        # the share of 8 x 8 patches at level 0 that hold an id border
        p = ids[:, :H // 8 * 8, :W // 8 * 8].view(a.pairs, H // 8, 8, W // 8, 8)
        res["patches_with_a_border"] = round(float((p.amax((2, 4)) != p.amin((2, 4))).float().mean()), 3)
    res.update(zip(names, timed(fns, a.iters, a.warmup)))
    if not a.unguided_only:
        res["guided_over_plain"] = round(res["dense_flow_guided"]["median_ms"] / res["dense_flow"]["median_ms"], 3)
        res["guided_over_plain_refined"] = round(res["dense_flow_refined_guided"]["median_ms"] / res["dense_flow_refined"]["median_ms"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
