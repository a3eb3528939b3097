"""Captures tests/golden/tube_quality_reference.npz from the LIVE reference (build container only; needs the reference checkout
that oracle.ref_shims points at).  Nothing of the reference is stored but what its programs compute.

Video panoptic quality is the reference's panoptic quality with a tube for a segment, so the oracle of a window of k frames is
cityscapesscripts' pq_compute_single_core on the k frames stacked into one image of k * H rows.  This tool stacks every window
of every case of tests/tube_quality_np.py and hands the stacks to tools/capture_map_quality_golden.py's run_case, which writes
the id-RGB PNG files and annotations the reference reads (see there for the encoding).

Recorded per case: the clips; per window length k the reference's tp / fp / fn / iou per class of every window on its own
([B, T-k+1, C]), the totals of one run over all windows of that k, and PQStat.pq_average of the totals for All / Things / Stuff
(n = 0 and NaN where the reference divides by zero).

    python tools/capture_tube_quality_golden.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import capture_map_quality_golden as CM                  # noqa: E402
import tube_quality_np as TQ                             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "tube_quality_reference.npz")
FIELDS = ("tp", "fp", "fn", "iou")


def main():
    pq, sem = CM.load_reference()
    out = {}
    for name, case in TQ.cases().items():
        pred, gt = case["pred"], case["gt"]
        B, T, H, W = pred.shape
        out[f"{name}/pred"], out[f"{name}/gt"] = pred, gt
        for k in case["windows"]:
            stack = lambda m: np.stack([m[b, t0:t0 + k].reshape(k * H, W) for b in range(B) for t0 in range(T - k + 1)])
            stacked = dict(pred=stack(pred), gt=stack(gt), params=case["params"])
            with tempfile.TemporaryDirectory() as tmp:
                p, cats, per_window, whole, _, _ = CM.run_case(pq, sem, stacked, tmp)
            C = p["num_classes"]
            rows = [CM._stat_arrays(s, C) for s in per_window]
            for i, f in enumerate(FIELDS):
                out[f"{name}/k{k}/{f}"] = np.stack([r[i] for r in rows]).reshape(B, T - k + 1, C)
                out[f"{name}/k{k}/total/{f}"] = CM._stat_arrays(whole, C)[i]
            for g, isthing in zip(CM.GROUPS, (None, True, False)):
                try:
                    avg, _ = whole.pq_average(cats, isthing=isthing)
                except ZeroDivisionError:
                    avg = {"pq": np.nan, "sq": np.nan, "rq": np.nan, "n": 0}
                out[f"{name}/k{k}/avg/{g}"] = np.array([avg[x] for x in ("pq", "sq", "rq", "n")], np.float64)
            print(name, "k", k, pred.shape, "tp/fp/fn", *(int(out[f"{name}/k{k}/total/{f}"].sum()) for f in FIELDS[:3]),
                  "All", out[f"{name}/k{k}/avg/All"].tolist())
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN))


if __name__ == "__main__":
    main()
