"""Scoring of label maps on the GPU (csrc/map_quality.hip, evaluate.map_quality): every output is held to the numpy restatement
(tests/map_quality_np.py) and to the reference's own per-image results (tests/golden/map_quality_reference.npz) with exact
equality, the float64 IoU sums with torch.equal.  The cases (map_quality_np.cases()) are the smallest shapes at which the kernels
can still go wrong: 1x1, 7x300, 33x65 and 129x257 (none a multiple of the wave, of a thread's 8 pixels or of a workgroup's
2048), N = 1, 3, 6 and 11, [N], [B,T] and [B,1,T] inputs, a segment that spans several workgroups and one of a single pixel, and
in `crafted` one image per rule: IoU exactly 0.5 (50 / 100: no match) and 51 / 101 (match); a predicted segment exactly half on
void (fp) and one pixel more (ignored); the same through the crowd region of its class; a crowd region of another class; a
ground-truth crowd region under an identical prediction (no tp, no fn); the same n in two classes; n = label_divisor - 1; an
all-void image; void by every route.  Both encodings of one scene, a uint8 label map pair, another divisor and class count,
the pair table at full occupancy and past it, many frames of two tiles each (the count kernel's tile walk) and more frames
than the kernel launches workgroups."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import map_quality_np as M
import panoptic_np as P
from c2m_amd import evaluate, segment

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_quality_reference.npz")
FIELDS = ("tp", "fp", "fn", "iou", "confusion")
CASE_NAMES = sorted(M.cases())


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return M.cases()


@pytest.fixture(scope="module")
def expected(cases):
    """The restatement's per-image results of every case, computed once."""
    return {k: M.batch_quality(c["pred"], c["gt"], **M.restatement_params(c["params"])) for k, c in cases.items()}


def run(case, **over):
    m = evaluate.map_quality(torch.from_numpy(case["pred"]).to(DEV), torch.from_numpy(case["gt"]).to(DEV),
                             **{**case["params"], **over})
    torch.cuda.synchronize()
    return m


def lead_of(case):
    s = case["pred"].shape[:-2]
    return (s[0], s[-1]) if len(s) > 1 else tuple(s)


def stacked(rows, lead):
    """A list of per-image dicts -> one dict of torch tensors with the leading axes `lead`."""
    return {k: torch.from_numpy(np.stack([r[k] for r in rows]).reshape(lead + rows[0][k].shape)) for k in FIELDS}


def check(got, want, what, frames=None):
    for k in FIELDS:
        g, w = got[k].cpu(), want[k]
        if frames is not None:
            g, w = g[frames], w[frames]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (what, k, (g != w).nonzero()[:4].tolist())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_equals_restatement_and_reference(name, cases, expected, golden):
    c = cases[name]
    lead = lead_of(c)
    got = run(c)
    assert got["tp"].dtype == torch.int32 and got["iou"].dtype == torch.float64 and got["confusion"].dtype == torch.int64
    assert got["overflow"].dtype == torch.bool and got["overflow"].shape == lead and not got["overflow"].any()
    assert all(v.device.type == "cuda" for v in got.values())
    check(got, stacked(expected[name], lead), name)
    ref = [{k: golden[f"{name}/{n}/{k}"] for k in FIELDS} for n in range(len(expected[name]))]
    check(got, stacked(ref, lead), name + " (reference)")
    assert int(got["confusion"].sum()) == c["pred"].size                   # every pixel is binned once


def test_both_encodings_of_a_scene_agree(cases):
    a, b = run(cases["rows_7x300"]), run(cases["rows_7x300_panoptic"])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_batch_equals_single_calls_and_4d_equals_5d(cases):
    c = cases["clip_33x65"]
    whole = run(c)
    five = run({**c, "pred": c["pred"][:, None], "gt": c["gt"][:, None]})
    for k in whole:
        assert torch.equal(whole[k], five[k]), k
    for b in range(2):
        for t in range(3):
            one = run({**c, "pred": c["pred"][b, t][None], "gt": c["gt"][b, t][None]})
            for k in whole:
                assert torch.equal(one[k][0], whole[k][b, t]), (k, b, t)


CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import map_quality_np as M
from c2m_amd import evaluate
c = M.cases()["hash_64x64"]
pred, gt = torch.from_numpy(c["pred"]).cuda(), torch.from_numpy(c["gt"]).cuda()
out = {{}}
for tag, max_pairs in (("full", 4096), ("past", 2048)):
    m = evaluate.map_quality(pred, gt, max_pairs=max_pairs)
    torch.cuda.synchronize()
    out.update({{tag + "/" + k: v.cpu().numpy() for k, v in m.items()}})
np.savez({path!r}, **out)
"""


def test_pair_table_full_and_past_full(expected, tmp_path):
    """Frame 1 of hash_64x64 holds 4096 pairs of equal class.  The two calls run in a fresh child process under a time limit:
    that the call returns is part of what is tested (no probe loop is unbounded), and a call that did not return must not
    block the tests after this one."""
    want = stacked(expected["hash_64x64"], (3,))
    path = str(tmp_path / "hash.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    code = CHILD.format(root=os.path.dirname(here), tests=here, path=path)
    flags = ["-s"] if sys.flags.no_user_site else []
    child = subprocess.run([sys.executable] + flags + ["-c", code], capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    with np.load(path) as z:
        done = {tag: {k: torch.from_numpy(z[f"{tag}/{k}"]) for k in FIELDS + ("overflow",)} for tag in ("full", "past")}
    assert done["full"]["overflow"].tolist() == [False, False, False]     # 4096 slots: full occupancy, long probe chains
    check(done["full"], want, "4096 pairs in 4096 slots")
    assert int(done["full"]["tp"][1].sum()) == 4096
    assert done["past"]["overflow"].tolist() == [False, True, False]
    check(done["past"], want, "frames next to the overflowed one", frames=[0, 2])
    assert torch.equal(done["past"]["confusion"], want["confusion"])      # what does not go through the pair table is complete
    score = evaluate.MapScore(max_pairs=2048)
    with pytest.raises(ValueError, match="max_pairs"):
        score.update(done["past"])
    evaluate.MapScore(max_pairs=4096).update(done["full"])


@pytest.fixture(scope="module")
def walk():
    return M.walk_cases()


@pytest.mark.parametrize("name", ["walk_600x33x65", "clamp_1100x3x5"])
def test_tile_walk_and_workgroup_clamp_equal_restatement(name, walk):
    """600 frames of two tiles each: one workgroup per frame walks both with one LDS pair table; 1100 frames: the cap of 1024
    workgroups falls below one per frame and is clamped to one (map_quality_np.walk_cases)."""
    c = walk[name]
    N = c["pred"].shape[0]
    got = run(c)
    assert not got["overflow"].any()
    check(got, stacked(M.batch_quality(c["pred"], c["gt"], **M.restatement_params(c["params"])), (N,)), name)
    assert int(got["confusion"].sum()) == c["pred"].size


def test_rollout_maps_5d_against_clip_maps_4d(cases):
    c = cases["clip_33x65"]                                                # [B,T,H,W]
    whole = run(c)
    for pred, gt in ((c["pred"][:, None], c["gt"]), (c["pred"], c["gt"][:, None])):
        mixed = run({**c, "pred": pred, "gt": gt})
        for k in whole:
            assert mixed[k].shape == whole[k].shape and torch.equal(mixed[k], whole[k]), k
    with pytest.raises(ValueError, match="differ in shape"):
        run({**c, "pred": c["pred"][:, None], "gt": c["gt"][:, :2]})


def test_repeats_bit_for_bit_also_on_a_side_stream(cases):
    c = cases["clip5d_129x257"]
    a, b = run(c), run(c)
    side = torch.cuda.Stream()
    pred, gt = torch.from_numpy(c["pred"]).to(DEV), torch.from_numpy(c["gt"]).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d = evaluate.map_quality(pred, gt)
    side.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], d[k]), k


def test_map_score_takes_device_results(cases, golden):
    name = "clip_33x65"
    score = evaluate.MapScore()
    score.update(run(cases[name]))
    r = score.result()
    assert np.array_equal(score.total["tp"], golden[f"{name}/total/tp"]) and len(r["per_frame"]) == 3
    assert abs(r["All"]["pq"] - golden[f"{name}/avg/All"][0]) <= 1e-12 * golden[f"{name}/avg/All"][0]
    assert abs(r["mIoU"] - golden[f"{name}/avg/semantic"][0]) <= 1e-12 * golden[f"{name}/avg/semantic"][0]


def test_panoptic_maps_scored_against_themselves():
    c = P.cases()["off_tile_65x97"]
    heads = [torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("semantic", "center", "offset")]
    maps = segment.panoptic_maps(*heads, **c["params"])
    p = {k: c["params"][k] for k in ("thing_list", "label_divisor", "ignore_label") if k in c["params"]}
    for key in ("panoptic", "instance"):
        m = evaluate.map_quality(maps[key], maps[key], **p)
        torch.cuda.synchronize()
        assert int(m["tp"].sum()) > 0 and not m["fp"].any() and not m["fn"].any() and not m["overflow"].any()
        assert torch.equal(m["iou"], m["tp"].double())
        conf = m["confusion"]
        assert torch.equal(conf, torch.diag_embed(torch.diagonal(conf, dim1=-2, dim2=-1)))
        assert int(conf.sum()) == maps[key].numel()


def test_refusals_on_the_device(cases):
    c = cases["px_1x1"]
    pred, gt = torch.from_numpy(c["pred"]).to(DEV), torch.from_numpy(c["gt"]).to(DEV)
    with pytest.raises(ValueError, match="max_pairs"):
        evaluate.map_quality(pred, gt, max_pairs=100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.map_quality(pred.cpu(), gt.cpu())
    empty = evaluate.map_quality(pred[:0], gt[:0])
    assert empty["tp"].shape == (0, 19) and empty["confusion"].shape == (0, 20, 20) and empty["overflow"].shape == (0,)
