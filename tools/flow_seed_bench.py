"""Device-event timing of dense_flow with and without the block-matching seed of its coarsest level (c2m_amd.flow, seed=;
fl_patch_match_kernel in csrc/dense_flow.hip), by the method of tools/dense_flow_bench.py and on its workload.

    python tools/flow_seed_bench.py [--pairs 96] [--size 128 256] [--iters 20] [--warmup 3] [--out FILE]

The 96 pairs at 128 x 256 are those of a B = 8 step with 2 input and 5 predicted frames.  All variants are timed alternately in
one process after --warmup rounds, HIP events around each call; median, minimum and maximum of --iters repetitions:
`dense_flow` / `dense_flow_seeded` (radius 4) / `dense_flow_seeded_r8`, the same three with the variational refinement, and
`patch_match` / `patch_match_r8`: the match launch alone on the coarsest level of the call's pyramid.  The seed adds two launches
(the match and a densify of the coarsest level) whatever the number of pairs is.  `fast_*`: the mean endpoint error of a second
set of pairs, the same texture moved by (25, 0) px, away from the border, unseeded and seeded: the motion the seed is for.
Prints one JSON line; --out appends it to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import flow as F  # noqa: E402
from dense_flow_bench import frames, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=96)
    ap.add_argument("--size", type=int, nargs=2, default=(128, 256))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_seed_bench needs a GPU: a timing taken anywhere else says nothing about it")
    H, W = a.size
    A, B = frames(a.pairs, H, W)
    vr = dict(value_range=(-1, 1))
    _, sizes, images = F.flow_pyramid(A, B, (-1, 1))
    ia, ib = (t.clone() for t in images[-1])
    names = ["dense_flow", "dense_flow_seeded", "dense_flow_seeded_r8", "dense_flow_refined", "dense_flow_refined_seeded",
             "dense_flow_refined_seeded_r8", "patch_match", "patch_match_r8"]
    fns = [lambda: F.dense_flow(A, B, **vr), lambda: F.dense_flow(A, B, seed=True, **vr), lambda: F.dense_flow(A, B, seed=8, **vr),
           lambda: F.dense_flow(A, B, refine=True, **vr), lambda: F.dense_flow(A, B, refine=True, seed=True, **vr),
           lambda: F.dense_flow(A, B, refine=True, seed=8, **vr), lambda: F.patch_match(ia, ib), lambda: F.patch_match(ia, ib, 8)]
    t = dict(zip(names, timed(fns, a.iters, a.warmup)))
    inner = (slice(None), slice(None), slice(32, H - 32), slice(32, W - 32))

    def epe(flow, u, v):
        return round(float((flow - torch.tensor([u, v], device=flow.device).view(1, 2, 1, 1))[inner].square().sum(1).sqrt().mean()), 4)

    n_fast = min(a.pairs, 8)
    Bf = B[:n_fast]
    Af = torch.roll(Bf, shifts=-25, dims=3)                           # a(x) = b(x + (25, 0)) away from the wrap
    res = {"pairs": a.pairs, "size": [H, W], "levels": len(sizes), "coarsest": list(sizes[-1]), "iters": a.iters,
           "patches_per_pair_coarsest": len(F.patch_origins(sizes[-1][0])) * len(F.patch_origins(sizes[-1][1])),
           "launches_dense_flow": 1 + 2 * len(sizes), "launches_dense_flow_seeded": 3 + 2 * len(sizes), **t,
           "seeded_over_plain": round(t["dense_flow_seeded"]["median_ms"] / t["dense_flow"]["median_ms"], 3),
           "seeded_r8_over_plain": round(t["dense_flow_seeded_r8"]["median_ms"] / t["dense_flow"]["median_ms"], 3),
           "refined_seeded_over_refined": round(t["dense_flow_refined_seeded"]["median_ms"] / t["dense_flow_refined"]["median_ms"], 3),
           "small_motion_epe_px": epe(F.dense_flow(A, B, **vr), 3.0, -2.0),
           "small_motion_epe_px_seeded": epe(F.dense_flow(A, B, seed=True, **vr), 3.0, -2.0),
           "fast_pairs": n_fast, "fast_motion_epe_px": epe(F.dense_flow(Af, Bf, **vr), 25.0, 0.0),
           "fast_motion_epe_px_seeded": epe(F.dense_flow(Af, Bf, seed=True, **vr), 25.0, 0.0)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
