"""Captures tests/golden/map_quality_reference.npz from the LIVE reference (build container only; needs the reference checkout
that oracle.ref_shims points at).  Nothing of the reference is stored but what its programs compute.

Two files of the reference are loaded by path and run on the CPU on the cases of tests/map_quality_np.py:
cityscapesScripts/cityscapesscripts/evaluation/evalPanopticSemanticLabeling.py (pq_compute_single_core, PQStat.pq_average,
average_pq; `pyquaternion`, which its helpers import, is stubbed) and panoptic_deeplab/segmentation/evaluation/semantic.py
(SemanticEvaluator; `fvcore.common.file_io` and `segmentation.utils` are stubbed and np.int / np.float defined, which numpy 2
no longer has).  pq_compute_single_core reads PNG files and a `segments_info` list: every map is written as a temporary id-RGB
PNG with void as the reference's VOID = 0 and a segment (cat, n) as cat * label_divisor + n + 1 -- for the panoptic encoding
that is v + 1; it is monotone in n within a class, so the reference's order of summation is the contract's, and road (class 0)
does not collide with VOID -- and category_id, iscrowd and area are filled in from the canonical rule.  SemanticEvaluator gets
the class maps with void as num_classes (prediction) and ignore_label (ground truth).

Recorded per case: the maps and parameters; per image tp / fp / fn / iou per class and the confusion matrix (the reference run
on that image alone); and from one run over all images of the case the totals, average_pq's results and
SemanticEvaluator.evaluate's.  A group without a counted class makes the reference divide by zero: n = 0 and NaN are recorded.

    python tools/capture_map_quality_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_quality_np as M                               # noqa: E402
from oracle import ref_shims                             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "map_quality_reference.npz")
REF = os.path.dirname(ref_shims.REF_SRC)
CS_ROOT = os.path.join(REF, "cityscapesScripts")
PQ_FILE = os.path.join(CS_ROOT, "cityscapesscripts", "evaluation", "evalPanopticSemanticLabeling.py")
SEM_FILE = os.path.join(REF, "panoptic_deeplab", "segmentation", "evaluation", "semantic.py")
GROUPS = ("All", "Things", "Stuff")
SEM_KEYS = ("mIoU", "fwIoU", "mACC", "pACC")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyquaternion", types.ModuleType("pyquaternion"))
    sys.modules["pyquaternion"].Quaternion = object
    sys.path.insert(0, CS_ROOT)
    pq = _load("ref_eval_panoptic", PQ_FILE)
    for name in ("fvcore", "fvcore.common", "fvcore.common.file_io", "segmentation", "segmentation.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["fvcore.common.file_io"].PathManager = None
    sys.modules["segmentation.utils"].save_annotation = None
    if not hasattr(np, "int"):
        np.int, np.float = int, float
    sem = _load("ref_eval_semantic", SEM_FILE)
    return pq, sem


def _png(path, ids):
    ids = ids.astype(np.uint32)
    assert ids.max() < 2 ** 24
    Image.fromarray(np.stack([ids & 255, (ids >> 8) & 255, ids >> 16], -1).astype(np.uint8)).save(path)


def _annotation(name, ids, p, crowd_side):
    info = []
    for i, cnt in zip(*np.unique(ids[ids > 0], return_counts=True)):
        cat, n = (int(i) - 1) // p["label_divisor"], (int(i) - 1) % p["label_divisor"]
        info.append({"id": int(i), "category_id": cat, "area": int(cnt),
                     "iscrowd": int(crowd_side and cat in p["thing_list"] and n == 0)})
    return {"image_id": name, "file_name": name + ".png", "segments_info": info}


def run_case(pq, sem, case, tmp):
    """-> per-image PQStats, the PQStat of one run over all images, per-image confusion matrices, the evaluator of all images."""
    p = M.restatement_params(case["params"])
    C = p["num_classes"]
    cats = {c: {"id": c, "name": str(c), "isthing": int(c in p["thing_list"])} for c in range(C)}
    H, W = case["pred"].shape[-2:]
    pairs = []
    confs = []
    total = sem.SemanticEvaluator(C, ignore_label=p["ignore_label"])
    for n, (pm, gm) in enumerate(zip(case["pred"].reshape(-1, H, W), case["gt"].reshape(-1, H, W))):
        ids, classes = [], []
        for m in (pm, gm):
            cat, _, void = M.canonical(m, C, p["label_divisor"], p["ignore_label"])
            ids.append(np.where(void, 0, M.keys(m, C, p["label_divisor"], p["ignore_label"]) + 1))
            classes.append((cat, void))
        _png(os.path.join(tmp, f"pred_{n}.png"), ids[0])
        _png(os.path.join(tmp, f"gt_{n}.png"), ids[1])
        pairs.append((_annotation(f"gt_{n}", ids[1], p, True), _annotation(f"pred_{n}", ids[0], p, False)))
        pred_sem = np.where(classes[0][1], C, classes[0][0])
        gt_sem = np.where(classes[1][1], p["ignore_label"], classes[1][0])
        one = sem.SemanticEvaluator(C, ignore_label=p["ignore_label"])
        one.update(pred_sem, gt_sem)
        total.update(pred_sem, gt_sem)
        confs.append(one._conf_matrix.copy())
    with contextlib.redirect_stdout(io.StringIO()):
        per_image = [pq.pq_compute_single_core(0, [pair], tmp, tmp, cats) for pair in pairs]
        whole = pq.pq_compute_single_core(0, pairs, tmp, tmp, cats)
    return p, cats, per_image, whole, confs, total


def _stat_arrays(stat, C):
    return (np.array([stat[c].tp for c in range(C)], np.int32), np.array([stat[c].fp for c in range(C)], np.int32),
            np.array([stat[c].fn for c in range(C)], np.int32), np.array([stat[c].iou for c in range(C)], np.float64))


def main():
    pq, sem = load_reference()
    out = {}
    for name, case in M.cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            p, cats, per_image, whole, confs, total = run_case(pq, sem, case, tmp)
        C = p["num_classes"]
        out[f"{name}/pred"], out[f"{name}/gt"] = case["pred"], case["gt"]
        for n, (stat, conf) in enumerate(zip(per_image, confs)):
            out[f"{name}/{n}/tp"], out[f"{name}/{n}/fp"], out[f"{name}/{n}/fn"], out[f"{name}/{n}/iou"] = _stat_arrays(stat, C)
            out[f"{name}/{n}/confusion"] = conf.astype(np.int64)
        out[f"{name}/total/tp"], out[f"{name}/total/fp"], out[f"{name}/total/fn"], out[f"{name}/total/iou"] = _stat_arrays(whole, C)
        out[f"{name}/total/confusion"] = total._conf_matrix.astype(np.int64)
        avgs = {}
        for g, isthing in zip(GROUPS, (None, True, False)):
            try:
                avgs[g], per_class = whole.pq_average(cats, isthing=isthing)         # what average_pq calls per group
            except ZeroDivisionError:
                avgs[g], per_class = {"pq": np.nan, "sq": np.nan, "rq": np.nan, "n": 0}, None
            out[f"{name}/avg/{g}"] = np.array([avgs[g][k] for k in ("pq", "sq", "rq", "n")], np.float64)
            if g == "All":
                out[f"{name}/avg/per_class"] = np.zeros((C, 3)) if per_class is None else np.array(
                    [[per_class[c][k] for k in ("pq", "sq", "rq")] for c in range(C)], np.float64)
        if all(avgs[g]["n"] for g in GROUPS):                                        # average_pq itself, where it can run
            ref = pq.average_pq(whole, cats)
            assert all(ref[g] == avgs[g] for g in GROUPS)
        with np.errstate(all="ignore"):
            res = total.evaluate()["sem_seg"]
        out[f"{name}/avg/semantic"] = np.array([res[k] for k in SEM_KEYS], np.float64)
        print(name, case["pred"].shape, "tp/fp/fn", int(out[f"{name}/total/tp"].sum()), int(out[f"{name}/total/fp"].sum()),
              int(out[f"{name}/total/fn"].sum()), "All", out[f"{name}/avg/All"].tolist(), "semantic", out[f"{name}/avg/semantic"].tolist())
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN))


if __name__ == "__main__":
    main()
