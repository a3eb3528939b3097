"""Video panoptic quality on the GPU (csrc/map_quality.hip: c2m_tube_quality; csrc/instance_link.hip: c2m_instance_relabel).
Counts are compared exactly and the float64 IoU sums and id_iou bit for bit (torch.equal) with the numpy restatement
(tests/tube_quality_np.py); tp / fp / fn / iou also with the reference's own results on the stacked windows
(tests/golden/tube_quality_reference.npz).  The cases (tube_quality_np.cases()) are small clips, one property each:

  clips_24x40   [2,5,24,40], k = 1, 2, 3 and T: an id that is there in frames 2.. only; a predicted truck that is mostly on void
                in one frame (ignored at k = 1) but not over a tube of two or more frames (fp; step 4); a ground-truth crowd
                region in one frame only; a car that is real in the last frame of clip 0 and only predicted in the first frame
                of clip 1, so a window that leaked across the clip border would change tp and fp; ids: padding, an absent
                object, a crowd id, a void value, an id the prediction lacks (0.0)
  odd_23x37     W % 4 != 0, windows given out of order; single_frame: T = 1; labels_u8: uint8 label maps
  id_swap       two cars whose ids swap mid-clip
  pairs_*       max_pairs = 8: a window with exactly 8 pairs (no overflow), with 9 (that window alone), and a frame that
                overflows on its own (every window that holds it)

and for the relabel kernel (tube_quality_np.relabel_cases()): a swap of two ids; an unlinked id that equals another node's anchor
id; count 0 and count 64 given unsorted; W % 4 != 0 with two strips of the scalar kernel; two strips of the vector kernel; a
plane smaller than one strip."""
import os

import numpy as np
import pytest
import torch

import tracking_np as NP
import tube_quality_np as TQ
from c2m_amd import evaluate, ops, tracking

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tube_quality_reference.npz")
CASE_NAMES = sorted(TQ.cases())


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return TQ.cases()


@pytest.fixture(scope="module")
def expected(cases):
    """The restatement's results of every case and window length, computed once."""
    out = {}
    for name, c in cases.items():
        p = TQ.restatement_params(c["params"])
        out[name] = {k: TQ.clip_quality(c["pred"], c["gt"], k, **p) for k in c["windows"]}
        if "ids" in c:
            for k in c["windows"]:
                out[name][k]["id_iou"], out[name][k]["id_gt_area"], out[name][k]["id_pred_area"] = \
                    TQ.clip_id_quality(c["pred"], c["gt"], c["ids"], k, **p)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(case, **over):
    ids = dev(case["ids"]) if "ids" in case else None
    r = evaluate.tube_quality(dev(case["pred"]), dev(case["gt"]), windows=case["windows"], ids=ids, **{**case["params"], **over})
    torch.cuda.synchronize()
    return r


def same(got, want, what, keep=None):
    g, w = got.cpu(), torch.from_numpy(np.asarray(want))
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if keep is not None:
        g, w = g[keep], w[keep]
    assert torch.equal(g, w), (what, (g != w).nonzero()[:4].tolist())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_equals_restatement_and_reference(name, cases, expected, golden):
    c = cases[name]
    B, T = c["pred"].shape[:2]
    got = run(c)
    over = TQ.expected_overflow(c)
    assert list(got) == list(c["windows"])                                  # in the order asked for
    for k in c["windows"]:
        r = got[k]
        assert r["overflow"].dtype == torch.bool and r["overflow"].shape == (B, T - k + 1)
        assert all(v.device.type == "cuda" for v in r.values())
        assert r["overflow"].cpu().tolist() == over[k].tolist(), (name, k)
        keep = torch.from_numpy(~over[k])                                   # an overflowed window's counts are incomplete
        for f in TQ.FIELDS:
            same(r[f], expected[name][k][f], (name, k, f), keep)
            same(r[f], golden[f"{name}/k{k}/{f}"], (name, k, f, "reference"), keep)
        if "ids" in c:
            for f in ("id_iou", "id_gt_area", "id_pred_area"):
                same(r[f], expected[name][k][f], (name, k, f), keep)
        else:
            assert "id_iou" not in r


def test_k1_is_map_quality(cases):
    for name in ("clips_24x40", "odd_23x37", "labels_u8", "pairs_frame_over"):
        c = cases[name]
        tube = run({**c, "windows": (1,)})[1]
        frames = evaluate.map_quality(dev(c["pred"]), dev(c["gt"]), **c["params"])
        torch.cuda.synchronize()
        for f in TQ.FIELDS + ("overflow",):
            assert tube[f].dtype == frames[f].dtype and torch.equal(tube[f], frames[f]), (name, f)


def test_the_cases_show_what_they_are_built_for(cases):
    c = cases["clips_24x40"]
    r = run(c)
    truck, car, person = 14, 13, 11
    assert r[1]["fp"][0, :, truck].tolist() == [1, 0, 1, 1, 1]              # frame 1: ten of twelve pixels on void, ignored
    assert r[2]["fp"][0, :, truck].tolist() == [1, 1, 1, 1] and r[5]["fp"][0, 0, truck].item() == 1   # never over a tube
    assert r[1]["fp"][1, :, car].tolist() == [1, 0, 1, 0, 1]                # clip 1: 13005 made up in frame 0; 13002 is on the crowd
    assert r[2]["fp"][1, :, car].tolist() == [1, 1, 1, 1]                   # region in frame 3 alone and counts over any tube
    assert r[1]["tp"][0, :, car].tolist() == [1, 1, 1, 1, 2] and r[2]["tp"][0, :, car].tolist() == [1, 1, 1, 2]   # 13005: the last
    assert r[1]["tp"][1, :, car].tolist() == [1] * 5                        # frame of clip 0 only; nothing of it in clip 1
    assert r[3]["tp"][0, :, person].tolist() == [1, 1, 1] and r[2]["tp"][0, :, person].tolist() == [0, 1, 1, 1]
    ids = r[5]["id_iou"][:, 0].cpu()
    assert ids[0, 1] == -1 and ids[0, 3] == -1 and ids[0, 5] == -1 and ids[0, 7] == -1      # padding, crowd id, void, absent
    assert ids[0, 4] == 0.0 and 0.5 < ids[0, 0] < 1 and ids[0, 2] == 1.0                     # the prediction lacks the rider
    assert r[2]["id_iou"][0, :, 6].tolist()[:3] == [-1.0] * 3 and r[2]["id_iou"][0, 3, 6].item() == 1.0
    s = run(cases["id_swap"])
    assert s[1]["tp"][0, :, car].tolist() == [2] * 4 and s[2]["fp"][0, :, car].tolist() == [0, 2, 0]
    assert s[2]["fn"][0, :, car].tolist() == [0, 2, 0] and s[4]["id_iou"][0, 0].tolist() == [24 / 72, 24 / 72]


def test_5d_against_4d_and_all(cases):
    c = cases["odd_23x37"]
    whole = run(c)
    mixed = run({**c, "pred": c["pred"][:, None], "windows": (1, 2, "all")})
    assert list(mixed) == [1, 2, 3]
    for k in whole:
        for f in whole[k]:
            assert torch.equal(whole[k][f], mixed[k][f]), (k, f)
    with pytest.raises(ValueError, match="differ in shape"):
        run({**c, "pred": c["pred"][:, None], "gt": c["gt"][:, :2]})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.tube_quality(dev(c["pred"]), dev(c["gt"]), windows=(1,), ids=torch.from_numpy(c["ids"]))
    empty = evaluate.tube_quality(dev(c["pred"])[:0], dev(c["gt"])[:0], windows=(2,))
    assert empty[2]["tp"].shape == (0, 2, 19) and empty[2]["overflow"].shape == (0, 2)


def test_repeats_bit_for_bit_also_on_a_side_stream(cases):
    c = cases["clips_24x40"]
    a, b = run(c), run(c)
    pred, gt, ids = dev(c["pred"]), dev(c["gt"]), dev(c["ids"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d = evaluate.tube_quality(pred, gt, windows=c["windows"], ids=ids)
    side.synchronize()
    for k in a:
        for f in a[k]:
            assert torch.equal(a[k][f], b[k][f]) and torch.equal(a[k][f], d[k][f]), (k, f)


def test_tube_score_takes_device_results(cases, golden):
    name = "clips_24x40"
    score = evaluate.TubeScore()
    score.update(run(cases[name]))
    r = score.result()
    for k in cases[name]["windows"]:
        assert np.array_equal(score.total[k]["tp"], golden[f"{name}/k{k}/total/tp"])
        want = golden[f"{name}/k{k}/avg/All"][0]
        assert abs(r["per_k"][k]["All"]["pq"] - want) <= 1e-12 * want
        assert 0 < r["per_k"][k]["id_iou"] < 1
    with pytest.raises(ValueError, match="max_pairs"):
        evaluate.TubeScore(max_pairs=8).update(run(cases["pairs_over"]))


@pytest.mark.parametrize("name", sorted(TQ.relabel_cases()))
def test_relabel_equals_restatement(name):
    c = TQ.relabel_cases()[name]
    maps = dev(c["maps"])
    before = maps.clone()
    got = ops.instance_relabel(maps, c["pairs_from"], c["pairs_to"], c["count"], TQ.M.CITYSCAPES["thing_list"], 1000)
    again = ops.instance_relabel(maps, c["pairs_from"], c["pairs_to"], c["count"], TQ.M.CITYSCAPES["thing_list"], 1000)
    torch.cuda.synchronize()
    want = TQ.relabel(c["maps"], c["pairs_from"], c["pairs_to"], c["count"])
    assert got.dtype == torch.int32 and got.shape == maps.shape and torch.equal(maps, before)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (got.cpu() != torch.from_numpy(want)).nonzero()[:4].tolist()
    assert torch.equal(got, again)
    if name == "swap_9x40":                                                 # the case shows what it is built for
        m, w = c["maps"][0], want[0]
        assert (w[m == 13001] == 13002).all() and (w[m == 13002] == 13001).all() and (m == 13001).any() and (m == 13002).any()
        assert (w[m == 13003] == 13000).all() and (w[m == 11001] == 13003).all() and (w[m == 11002] == 11000).all()
        assert (w[m == 300000] == 300000).all() and (w[m == 24001] == 24001).all() and (w[m == -3] == -3).all()


def test_tracked_scene_scores_one_against_its_unpermuted_painting():
    """A scene the tracking tests link completely: its frames carry permuted and partly new ids; track_instances and
    anchor_maps put them into the anchor's id space, where they must be the same scene painted without the permutation -- every
    thing tube a true positive with IoU 1 over the whole clip, and every node's own tube IoU 1."""
    t_in, T = 2, 7
    edges, ids, sc = NP.make_scene("constructed", 12, t_in)
    plain = NP.make_scene("constructed", 12, t_in, permute=False)[2]
    assert not np.array_equal(sc["inst"], plain["inst"])
    inst = dev(sc["inst"][None, None])                                      # [1,1,T,H,W]
    tr = tracking.track_instances(inst, t_in, dev(sc["target_flow"][None]), dev(sc["input_flow"][None]))
    assert tr.count.tolist() == [12] and tr.lost == [[]]
    real = tracking.anchor_maps(inst, tr, t_in)
    assert real.shape == inst.shape
    things = torch.from_numpy(sc["owner"] >= 0)                             # the backgrounds of the two paintings differ
    assert torch.equal(real[0, 0].cpu()[things], torch.from_numpy(plain["inst"])[things])
    nodes = tr.ids[:, :, t_in - 1].to(DEV)
    nodes = torch.where(torch.arange(64, device=DEV)[None] < 12, nodes, -1).int()
    r = evaluate.tube_quality(dev(plain["inst"][None]), real, windows=("all", 1), ids=nodes)
    torch.cuda.synchronize()
    full = r[T]
    th = list(TQ.M.CITYSCAPES["thing_list"])
    assert int(full["tp"][0, 0, th].sum()) == 12 and not full["fp"][0, 0, th].any() and not full["fn"][0, 0, th].any()
    assert torch.equal(full["iou"][0, 0, th], full["tp"][0, 0, th].double()) and not full["overflow"].any()
    assert (full["id_iou"][0, 0, :12] == 1.0).all() and (full["id_iou"][0, 0, 12:] == -1.0).all()
    assert (r[1]["id_iou"][0, :, :12] == 1.0).all()
