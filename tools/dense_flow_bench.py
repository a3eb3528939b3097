"""Device-event timing of one train.compute_flow-sized flow call, the weight-free dense inverse search (c2m_amd.flow; csrc/dense_flow.hip)
next to the random-weight FlowNet2 pass on the same frames.

    python tools/dense_flow_bench.py [--pairs 96] [--size 128 256] [--iters 20] [--warmup 3] [--out FILE]

The 96 pairs at 128 x 256 are those of a B = 8 step with 2 input and 5 predicted frames: 2 * (t_in - 1 + t_out) * B.  Frames are a
1/f texture and the same texture moved by a smooth flow of a few pixels, so the search runs on real structure (its cost does not
depend on the data: every patch does the same number of steps).  The two are timed alternately in one process after --warmup
rounds, HIP events around each call; median, minimum and maximum of --iters repetitions.  `dense_flow` is the flow alone,
`dense_flow_refined` the same with the variational refinement (refine=True; csrc/flow_refine.hip), `classic` adds the occlusion
map (ops.occlusion_splat) as ClassicFlow returns it, `flownet2` is FlowNet(pretrained=False)(A, B), which also includes that map.
`compute_flow_direct` is train.compute_flow(ClassicFlow()) on a clip batch of --pairs / 12 clips with 2 input and 5 predicted frames
(the same 96 pairs, every target searched across its whole gap), `compute_flow_chained` the same call with ClassicFlow(chain=True)
(the consecutive pairs, chained: csrc/flow_chain.hip), `chain_backward` / `chain_forward` one chain_flows launch
on that batch's steps.  Prints one JSON line; --out appends it to a file.  A tool, not a test: it carries no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import flow as F, train  # noqa: E402
from c2m_amd.modules.third_party.flow_net.flow_net import FlowNet  # noqa: E402


def frames(n, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    b = torch.zeros(n, 3, H, W)
    for k in (2, 4, 8, 16):                                          # octaves of smooth noise, equal energy each
        c = torch.randn(n, 3, -(-H // k) + 2, -(-W // k) + 2, generator=g)
        b += torch.nn.functional.interpolate(c, scale_factor=k, mode="bicubic", align_corners=False)[..., k:k + H, k:k + W]
    b = (b - b.amin()) / (b.amax() - b.amin())
    a = torch.roll(b, shifts=(2, -3), dims=(2, 3))                   # a(x) = b(x + (3, -2)) away from the wrap
    return (a * 2 - 1).cuda(), (b * 2 - 1).cuda()


def timed(fns, iters, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(iters)]
    for row in ev:
        row[0].record()
        for k, fn in enumerate(fns):
            fn()
            row[k + 1].record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        t = sorted(row[k].elapsed_time(row[k + 1]) for row in ev)
        out.append({"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=96)
    ap.add_argument("--size", type=int, nargs=2, default=(128, 256))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_flow_bench needs a GPU: a timing taken anywhere else says nothing about it")
    H, W = a.size
    A, B = frames(a.pairs, H, W)
    classic = F.ClassicFlow()
    torch.manual_seed(0)
    net = FlowNet(pretrained=False).cuda()
    flow = F.dense_flow(A, B, value_range=(-1, 1))
    inner = (slice(None), slice(None), slice(16, H - 16), slice(16, W - 16))
    err = (flow - torch.tensor([3.0, -2.0], device=flow.device).view(1, 2, 1, 1))[inner].square().sum(1).sqrt().mean()
    refined = F.dense_flow(A, B, value_range=(-1, 1), refine=True)
    err_refined = (refined - torch.tensor([3.0, -2.0], device=flow.device).view(1, 2, 1, 1))[inner].square().sum(1).sqrt().mean()
    # the clip batch of a training step: the texture moving (3, -2) px per frame, t_in = 2, t_out = 5
    t_in, t_out, clips = 2, 5, max(1, a.pairs // 12)
    video = torch.stack([torch.roll((B[:clips] + 1) / 2, shifts=(2 * t, -3 * t), dims=(2, 3)) for t in range(t_in + t_out)], 2)
    batch, tp = {"video": video}, {"num_input_frames": t_in, "num_predicted_frames": t_out}
    chained = F.ClassicFlow(chain=True)
    steps = torch.stack([flow[:clips]] * t_out, 1).contiguous()
    fns = [lambda: F.dense_flow(A, B, value_range=(-1, 1)), lambda: F.dense_flow(A, B, value_range=(-1, 1), refine=True),
           lambda: classic(A, B), lambda: net(A, B), lambda: train.compute_flow(classic, batch, tp),
           lambda: train.compute_flow(chained, batch, tp), lambda: F.chain_flows(steps, "backward"),
           lambda: F.chain_flows(steps, "forward")]
    t_flow, t_refined, t_classic, t_net, t_direct, t_chained, t_cb, t_cf = timed(fns, a.iters, a.warmup)
    far = (slice(None), slice(None), t_out - 1, slice(32, H - 32), slice(32, W - 32))      # the last target, away from the wrap
    truth = torch.tensor([3.0 * t_out, -2.0 * t_out], device=flow.device).view(1, 2, 1, 1)
    epe_far = lambda f: round(float((f["target_bw_of"][far] - truth).square().sum(1).sqrt().mean()), 4)
    levels, rp = len(F.pyramid_sizes(H, W)), F.REFINE_DEFAULTS
    res = {"pairs": a.pairs, "size": [H, W], "levels": len(F.pyramid_sizes(H, W)), "iters": a.iters,
           "launches_dense_flow": 1 + 2 * len(F.pyramid_sizes(H, W)), "mean_epe_px_16px_from_border": round(float(err), 4),
           "launches_dense_flow_refined": 1 + (3 + rp["outer"]) * levels,
           "mean_epe_px_16px_from_border_refined": round(float(err_refined), 4),
           "dense_flow": t_flow, "dense_flow_refined": t_refined,
           "refined_over_plain": round(t_refined["median_ms"] / t_flow["median_ms"], 1), "classic": t_classic, "flownet2": t_net,
           "flownet2_over_classic": round(t_net["median_ms"] / t_classic["median_ms"], 1),
           "clips": clips, "frames": [t_in, t_out], "compute_flow_direct": t_direct, "compute_flow_chained": t_chained,
           "chained_over_direct": round(t_chained["median_ms"] / t_direct["median_ms"], 3),
           "chain_backward": t_cb, "chain_forward": t_cf,
           "last_target_epe_px_direct": epe_far(train.compute_flow(classic, batch, tp)),
           "last_target_epe_px_chained": epe_far(train.compute_flow(chained, batch, tp))}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
