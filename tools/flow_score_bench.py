"""Device-event timing of the flow scores (c2m_amd.evaluate.flow_quality_sums / flow_consistency_sums; csrc/flow_score.hip; DESIGN
4.2r), by the method of tools/dense_flow_bench.py and on its workload.

    python tools/flow_score_bench.py [--pairs 96] [--size 128 256] [--iters 20] [--warmup 3] [--out FILE]

The 96 pairs at 128 x 256 are those of a B = 8 step with 2 input and 5 predicted frames: b a smooth-noise frame, a the frame
moved by (3, -2) px, the flows those of flow.dense_flow in both directions, the target the constant true flow.  All variants
are timed alternately in one process after --warmup rounds, HIP events around each call; median, minimum and maximum of --iters
repetitions.  `quality` / `quality_regions`: flow_quality_sums without and with a region byte; `consistency`,
`consistency_regions`, `consistency_maps`, `consistency_no_ba`: flow_consistency_sums with both flows, plus a region byte, plus
the three maps, and without the reverse flow.  `torch_quality` / `torch_consistency`: the whole-frame columns of the same
quantities (no regions, no maps) composed from torch operators in float64, as context: they are what a user would write without
the kernels, not a restatement with the same bits.  Each timed call includes its workspace and result allocations (torch's
caching allocator), as a user's call does.  `*_GBps_of_inputs`: every input byte once over the median time; the inputs of all
pairs (50 and 126 MB) fit in the last-level cache and every repetition reads the same ones, so this is a warm-cache rate, not
an HBM rate.  Prints one JSON line; --out appends it to a file.  A tool, not a test: it carries
no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import evaluate as E, flow as F  # noqa: E402
from dense_flow_bench import frames, timed  # noqa: E402


def torch_quality(pred, target):
    p, t = pred.double(), target.double()
    scored = torch.isfinite(t).all(1) & (t.abs() < 1e9).all(1)
    fin = scored & torch.isfinite(p).all(1)
    e2, m2 = (p - t).square().sum(1), t.square().sum(1)
    c = (1.0 + (p * t).sum(1)) / torch.sqrt((1.0 + p.square().sum(1)) * (1.0 + m2))
    z = lambda x: torch.where(fin, x, torch.zeros_like(x)).sum((1, 2))
    n = lambda m: m.sum((1, 2)).double()
    bad = scored & ~fin
    return torch.stack([n(scored), n(bad), z(e2.sqrt()), z(e2), z(m2.sqrt()), z(torch.acos(c.clamp(-1.0, 1.0))),
                        n(bad | (fin & (e2 > 9.0) & (e2 > 0.0025 * m2))), n(bad | (fin & (e2 > 1.0))), n(bad | (fin & (e2 > 9.0))),
                        n(bad | (fin & (e2 > 25.0)))], 1)


def torch_consistency(fab, a, b, fba, alpha1=0.01, alpha2=0.5):
    N, C, H, W = a.shape
    f = fab.double()
    yy, xx = torch.meshgrid(torch.arange(H, device=a.device, dtype=torch.float64),
                            torch.arange(W, device=a.device, dtype=torch.float64), indexing="ij")
    yx, yv = xx + f[:, 0], yy + f[:, 1]
    inside = torch.isfinite(f).all(1) & (yx >= 0) & (yx <= W - 1) & (yv >= 0) & (yv <= H - 1)
    sx, sy = torch.where(inside, yx, torch.zeros_like(yx)), torch.where(inside, yv, torch.zeros_like(yv))
    x0f, y0f = sx.floor(), sy.floor()
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    ax, ay = (sx - x0f).unsqueeze(1), (sy - y0f).unsqueeze(1)

    def sample(img):
        flat = img.double().flatten(2)
        g = lambda y, x: flat.gather(2, (y * W + x).flatten(1).unsqueeze(1).expand(-1, img.shape[1], -1)).view(N, -1, H, W)
        top = g(y0, x0) * (1.0 - ax) + g(y0, x1) * ax
        bot = g(y1, x0) * (1.0 - ax) + g(y1, x1) * ax
        return top * (1.0 - ay) + bot * ay

    p = (a.double() - sample(b)).abs().sum(1) / C
    g = sample(fba)
    fb2 = (f + g).square().sum(1)
    inc = inside & ~(fb2 <= alpha1 * (f.square().sum(1) + g.square().sum(1)) + alpha2)
    z = lambda x, m: torch.where(m, x, torch.zeros_like(x)).sum((1, 2))
    n = lambda m: m.sum((1, 2)).double()
    return torch.stack([torch.full((N,), float(H * W), device=a.device, dtype=torch.float64), n(inside), z(p, inside), z(p * p, inside),
                        z(fb2.sqrt(), inside & torch.isfinite(fb2)), n(inc), z(p, inside & ~inc)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=96)
    ap.add_argument("--size", type=int, nargs=2, default=(128, 256))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_score_bench needs a GPU: a timing taken anywhere else says nothing about it")
    H, W = a.size
    A, B = frames(a.pairs, H, W)
    fab, fba = F.dense_flow(A, B, value_range=(-1, 1)), F.dense_flow(B, A, value_range=(-1, 1))
    target = torch.tensor([3.0, -2.0], device=A.device).view(1, 2, 1, 1).expand(a.pairs, 2, H, W).contiguous()
    regions = E.flow_regions(fab)
    names = ["quality", "quality_regions", "consistency", "consistency_regions", "consistency_maps", "consistency_no_ba",
             "torch_quality", "torch_consistency"]
    fns = [lambda: E.flow_quality_sums(fab, target), lambda: E.flow_quality_sums(fab, target, None, regions),
           lambda: E.flow_consistency_sums(fab, A, B, fba), lambda: E.flow_consistency_sums(fab, A, B, fba, regions),
           lambda: E.flow_consistency_sums(fab, A, B, fba, regions, maps=True), lambda: E.flow_consistency_sums(fab, A, B),
           lambda: torch_quality(fab, target), lambda: torch_consistency(fab, A, B, fba)]
    t = dict(zip(names, timed(fns, a.iters, a.warmup)))
    q, c = E.flow_quality_sums(fab, target)[:, 0], E.flow_consistency_sums(fab, A, B, fba)[:, 0]
    tq, tc = torch_quality(fab, target), torch_consistency(fab, A, B, fba)
    rel = lambda x, y: float(((x - y).abs() / y.abs().clamp_min(1e-300)).max())
    px = a.pairs * H * W
    read_q, read_c = px * 16, px * (8 + 12 + 12 + 8)                   # every input byte once; the gathers' re-reads hit the caches
    res = {"pairs": a.pairs, "size": [H, W], "iters": a.iters, "tiles_per_pair": -(-H * W // 1024), **t,
           "quality_GBps_of_inputs": round(read_q / t["quality"]["median_ms"] / 1e6, 1),
           "consistency_GBps_of_inputs": round(read_c / t["consistency"]["median_ms"] / 1e6, 1),
           "torch_quality_over_kernel": round(t["torch_quality"]["median_ms"] / t["quality"]["median_ms"], 1),
           "torch_consistency_over_kernel": round(t["torch_consistency"]["median_ms"] / t["consistency"]["median_ms"], 1),
           "counts_equal_torch": bool(torch.equal(q[:, [0, 1, 6, 7, 8, 9]], tq[:, [0, 1, 6, 7, 8, 9]]) and torch.equal(c[:, [0, 1, 5]], tc[:, [0, 1, 5]])),
           "max_rel_sum_gap_vs_torch": max(rel(q[:, 2:6], tq[:, 2:6]), rel(c[:, [2, 3, 4, 6]], tc[:, [2, 3, 4, 6]])),
           "epe_px": round(float(q[:, 2].sum() / q[:, 0].sum()), 4), "photo": round(float(c[:, 2].sum() / c[:, 1].sum()), 5),
           "fb_px": round(float(c[:, 4].sum() / c[:, 1].sum()), 4), "inconsistent": round(float(c[:, 5].sum() / c[:, 1].sum()), 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
