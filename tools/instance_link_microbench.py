"""Device-event timing of ops.instance_overlap (c2m_instance_overlap: table zeroing + one pass over frame, flow and reference map)
and wall time of the whole tracking.track_instances call (statistics, slots, overlap, match, composition, one device -> host
read), next to a baseline made only of what the project had before the kernel: ops.label_warp of the reference map, two
torch.searchsorted for the id -> slot maps and a torch.bincount over a combined key (four passes over the pixels).

    python tools/instance_link_microbench.py [--cases 8x7x128x256,16x1x1024x2048] [--objects 30] [--iters 50]

A case is BxTxHxW: B samples of T frames, one input frame, so B * (T - 1) planes are linked to their sample's first frame
(T = 1: B planes against themselves).  The maps are the street-like maps of tools/instance_stats_microbench.py, every frame
shifted by a few pixels and the flow the matching shift.  Prints one JSON line per case: median microseconds, and the rate at
which the algorithm's 16 bytes per pixel (frame 4, flow 8, reference 4) are moved."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c2m_amd import ops, tracking  # noqa: E402
from instance_stats_microbench import scene_maps, timed  # noqa: E402


def baseline(ref, frame, flow, ref_slots, frame_slots, M):
    """pairs [P, M + 1, M + 1] from torch ops and ops.label_warp; slot lists padded with -1 as ops.instance_slots writes them."""
    P = ref.shape[0]
    warped = ops.label_warp(flow, planes_i=ref[:, None])[1].view(P, -1)
    big = torch.iinfo(torch.int32).max

    def slot(v, ids):
        ids = torch.where(ids < 0, torch.full_like(ids, big), ids)
        pos = torch.searchsorted(ids, v).clamp(max=M - 1)
        return torch.where(torch.gather(ids, 1, pos) == v, pos, torch.full_like(pos, M))

    key = (slot(warped, ref_slots) * (M + 1) + slot(frame.view(P, -1), frame_slots)
           + torch.arange(P, device=ref.device)[:, None] * (M + 1) ** 2)
    return torch.bincount(key.view(-1), minlength=P * (M + 1) ** 2).view(P, M + 1, M + 1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8x7x128x256,16x1x1024x2048")
    ap.add_argument("--objects", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instance_link_microbench needs a HIP device: nothing is measured without one")
    M = 64
    for case in a.cases.split(","):
        B, T, H, W = (int(v) for v in case.split("x"))
        base = scene_maps(B, H, W, a.objects)
        shifts = [(2 * t, t) for t in range(max(T, 2))]                                  # frame t: the scene moved by (2t, t) px
        inst = torch.stack([torch.roll(base, (dy, dx), (1, 2)) for dx, dy in shifts], 1).to("cuda")   # [B, >=2, H, W]
        n = max(T - 1, 1)
        flow = torch.zeros(B, 2, n, H, W, device="cuda")
        for k in range(n):
            flow[:, 0, k], flow[:, 1, k] = -shifts[k + 1][0], -shifts[k + 1][1]
        P = B * n
        ref = inst[:, :1].expand(B, n, H, W).reshape(P, H, W).contiguous()
        frame = inst[:, 1:1 + n].reshape(P, H, W).contiguous()
        fl = flow.permute(0, 2, 1, 3, 4).reshape(P, 2, H, W).contiguous()
        slots, _, _, count, _ = ops.instance_slots(ops.instance_stats(inst[:, :1 + n].contiguous(), 1 + n))
        pick = lambda x, lo, hi: x[:, lo:hi].reshape((P,) + tuple(x.shape[2:])).contiguous()
        rs, rc = pick(slots[:, :1].expand(B, n, M), 0, n), pick(count[:, :1].expand(B, n), 0, n)
        fs, fc = pick(slots, 1, 1 + n), pick(count, 1, 1 + n)
        got = ops.instance_overlap(ref, frame, fl, rs, rc, fs, fc)
        same = bool(torch.equal(got, baseline(ref, frame, fl, rs, fs, M)))               # faster and different is not faster
        t_kernel = timed(lambda: ops.instance_overlap(ref, frame, fl, rs, rc, fs, fc), a.iters)
        t_plain = timed(lambda: ops.instance_overlap(ref, frame, None, rs, rc, fs, fc), a.iters)
        t_base = timed(lambda: baseline(ref, frame, fl, rs, fs, M), a.iters)
        clip = inst[:, :1 + n].contiguous()
        tracking.track_instances(clip, 1, flow)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 10
        for _ in range(reps):
            tracking.track_instances(clip, 1, flow)
        t_track = (time.perf_counter() - t0) / reps * 1e6
        nbytes = 16 * P * H * W
        print(json.dumps({"B": B, "T": 1 + n, "H": H, "W": W, "planes": P, "objects_per_plane": float(count.float().mean()),
                          "equals_baseline": same, "instance_overlap_us": round(t_kernel, 1),
                          "algorithmic_GBps": round(nbytes / t_kernel / 1e3, 1),
                          "instance_overlap_no_flow_us": round(t_plain, 1), "baseline_us": round(t_base, 1),
                          "baseline_over_kernel": round(t_base / t_kernel, 2), "track_instances_wall_us": round(t_track, 1)}))


if __name__ == "__main__":
    main()
