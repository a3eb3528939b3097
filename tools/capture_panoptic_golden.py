"""Captures tests/golden/panoptic_reference.npz from the LIVE reference (build container only; needs the reference checkout that
oracle.ref_shims points at).  Nothing of the reference is stored but what its programs compute.

The reference's two post-processing files (panoptic_deeplab/segmentation/model/post_processing/{semantic,instance}_post_processing.py)
are loaded by path under a stub package -- the package's own __init__ would import the backbones -- and run on the CPU, one image at
a time, on the cases of tests/panoptic_np.py.  Recorded per case and image: the inputs (labels instead of logits in all but the
logits case; offsets as int16 quarter-pixels), the reference's semantic / panoptic / centres, and the instance-id image computed
from its panoptic result as generate_segmentation.py:299-305 does.  For the unquantised case the inputs are regenerated from the
seed; only the reference's results are stored, plus the number of pixels where its own fp32 result leaves the float64 restatement.

    python tools/capture_panoptic_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import panoptic_np as P                                 # noqa: E402
from oracle import ref_shims                            # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "panoptic_reference.npz")
POST = os.path.join(os.path.dirname(ref_shims.REF_SRC), "panoptic_deeplab", "segmentation", "model", "post_processing")


def load_reference():
    sys.dont_write_bytecode = True
    pkg = types.ModuleType("pdl_post")
    pkg.__path__ = [POST]
    sys.modules["pdl_post"] = pkg
    mods = {}
    for name in ("semantic_post_processing", "instance_post_processing"):
        spec = importlib.util.spec_from_file_location(f"pdl_post.{name}", os.path.join(POST, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["semantic_post_processing"], mods["instance_post_processing"]


def run_reference(sem_mod, ins_mod, case):
    """The reference on every image of a case: lists of semantic, panoptic, centres, instance image."""
    p = {**P.CITYSCAPES, **case["params"]}
    res = []
    for n in range(case["center"].shape[0]):
        s = torch.from_numpy(np.ascontiguousarray(case["semantic"][n:n + 1]))
        sem = sem_mod.get_semantic_segmentation(s) if s.dim() == 4 else s.long()
        pan, ctr = ins_mod.get_panoptic_segmentation(
            sem, torch.from_numpy(case["center"][n:n + 1].copy()), torch.from_numpy(case["offset"][n:n + 1].copy()),
            thing_list=list(p["thing_list"]), label_divisor=p["label_divisor"], stuff_area=p["stuff_area"],
            void_label=p["label_divisor"] * p["ignore_label"], threshold=p["threshold"], nms_kernel=p["nms_kernel"],
            top_k=p["top_k"], foreground_mask=None)
        pan = pan.squeeze(0).numpy()
        # the instance-id image, as generate_segmentation.py:299-305 computes it from the panoptic result
        to_sem = pan // p["label_divisor"]
        thing = np.isin(to_sem, list(p["thing_list"])).astype(pan.dtype)
        ins = to_sem * (1 - thing) + pan * thing
        res.append(dict(semantic=sem.squeeze(0).numpy().astype(np.uint8), panoptic=pan.astype(np.int32),
                        instance=ins.astype(np.int32), centers=ctr.reshape(-1, 2).numpy().astype(np.int16)))
    return res


def main():
    sem_mod, ins_mod = load_reference()
    out = {}
    for name, case in P.cases().items():
        sem = case["semantic"]
        out[f"{name}/semantic_in"] = sem if sem.ndim == 3 else sem.astype(np.float16)      # logits are eighths: exact in fp16
        assert np.array_equal(out[f"{name}/semantic_in"].astype(sem.dtype), sem)
        out[f"{name}/center_in"] = case["center"]
        q = case["offset"] * 4
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2 ** 15
        out[f"{name}/offset_q4"] = q.astype(np.int16)
        for n, r in enumerate(run_reference(sem_mod, ins_mod, case)):
            for k, v in r.items():
                out[f"{name}/{n}/{k}"] = v
        print(name, [int(len(out[f"{name}/{n}/centers"])) for n in range(case["center"].shape[0])])
    u = P.unquantised_case()
    r = run_reference(sem_mod, ins_mod, u)[0]
    mine = P.panoptic_batch(u["semantic"], u["center"], u["offset"], **u["params"])[0]
    differ = r["panoptic"] != mine["panoptic"]
    near = P.near_tie_mask(mine["two"])
    out["unquantised/0/panoptic"], out["unquantised/0/centers"] = r["panoptic"], r["centers"]
    out["unquantised/ref_fp32_differs"] = np.int64(differ.sum())
    out["unquantised/ref_fp32_differs_outside_near_ties"] = np.int64((differ & ~near).sum())
    print("unquantised: centres", len(r["centers"]), "reference fp32 != float64 restatement on", int(differ.sum()), "pixels,",
          int((differ & ~near).sum()), "outside the near-tie mask of", int(near.sum()))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN))


if __name__ == "__main__":
    main()
