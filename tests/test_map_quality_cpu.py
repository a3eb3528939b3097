"""Scoring of label maps, the parts that need no GPU: the numpy restatement of the contract (tests/map_quality_np.py) is held to
what the reference computed (tests/golden/map_quality_reference.npz, written by tools/capture_map_quality_golden.py from
cityscapesscripts' pq_compute_single_core / pq_average and Panoptic-DeepLab's SemanticEvaluator) with exact equality per image,
the float64 IoU sums included; evaluate.MapScore's arithmetic is fed with the recorded per-image values; and the checks
evaluate.map_quality makes on the host before anything is launched.

The tolerance of the averages, relative 1e-12, is derived, not measured: MapScore adds the per-image IoU sums in the order they
arrive and the reference adds match by match, so the totals differ by the rounding of the additions only; every figure is the
result of fewer than 10^4 float64 additions and divisions, each within 2^-53 relative: 10^4 * 2^-53 = 1.1e-12."""
import os

import numpy as np
import pytest
import torch

import map_quality_np as M
from c2m_amd import evaluate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_quality_reference.npz")
FIELDS = ("tp", "fp", "fn", "iou", "confusion")
CASE_NAMES = sorted(M.cases())
RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return M.cases()


def images(case):
    return int(np.prod(case["pred"].shape[:-2]))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_holds_the_cases_inputs(name, cases, golden):
    for k in ("pred", "gt"):
        assert golden[f"{name}/{k}"].dtype == cases[name][k].dtype and np.array_equal(golden[f"{name}/{k}"], cases[name][k])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_reference_per_image(name, cases, golden):
    c = cases[name]
    got = M.batch_quality(c["pred"], c["gt"], **M.restatement_params(c["params"]))
    assert len(got) == images(c)
    for n, g in enumerate(got):
        for k in FIELDS:
            want = golden[f"{name}/{n}/{k}"]
            assert g[k].dtype == want.dtype and np.array_equal(g[k], want), (name, n, k, g[k], want)


def test_fixture_cases_crafted_images_show_what_they_are_built_for(cases):
    """A check of the cases themselves (the restatement on them), not of the package: each crafted image isolates its rule."""
    c = cases["crafted"]
    r = M.batch_quality(c["pred"], c["gt"], **M.restatement_params({}))
    car = lambda n: (int(r[n]["tp"][13]), int(r[n]["fp"][13]), int(r[n]["fn"][13]))
    assert car(0) == (0, 1, 1)                                   # IoU exactly 0.5 is no match
    assert car(1) == (1, 0, 0) and r[1]["iou"][13] == 51 / 101
    assert car(2) == (0, 1, 0) and car(3) == (0, 0, 0)           # half on void counts, one pixel more is ignored
    assert car(4) == (0, 1, 0) and car(5) == (0, 0, 0)           # the same through the crowd region of its class
    assert car(6) == (0, 1, 0)                                   # a crowd of another class excuses nothing
    assert int(r[6]["fn"][11]) == 0 and car(7) == (0, 0, 0)      # a crowd region is no fn and matches nothing
    assert (int(r[8]["tp"][11]), int(r[8]["tp"][13]), int(r[8]["fp"][11]), int(r[8]["fn"][11])) == (1, 2, 1, 1)
    assert not r[9]["tp"].any() and not r[9]["fp"].any() and not r[9]["fn"].any() and r[9]["confusion"][19, 19] == 480
    assert int(r[10]["tp"][14]) == 1 and r[10]["iou"][14] == 1.0  # the predicted pixels on void leave the union


def test_fixture_cases_hold_one_scene_in_both_encodings(cases):
    """A check of the cases themselves: the two encodings differ as arrays and mean the same scene to the restatement."""
    a, b = cases["rows_7x300"], cases["rows_7x300_panoptic"]
    assert not np.array_equal(a["pred"], b["pred"])
    for x, y in zip(M.batch_quality(a["pred"], a["gt"], **M.restatement_params({})),
                    M.batch_quality(b["pred"], b["gt"], **M.restatement_params({}))):
        for k in FIELDS:
            assert np.array_equal(x[k], y[k])


def close(got, want):
    return (np.isnan(want) and np.isnan(got)) or abs(got - want) <= RTOL * abs(want)


def score_of(name, case, golden):
    lead = case["pred"].shape[:-2]
    lead = (lead[0], lead[-1]) if len(lead) > 1 else lead
    m = {k: np.stack([golden[f"{name}/{n}/{k}"] for n in range(images(case))]).reshape(lead + golden[f"{name}/0/{k}"].shape)
         for k in FIELDS}
    m["overflow"] = np.zeros(lead, bool)
    p = M.restatement_params(case["params"])
    score = evaluate.MapScore(**p)
    score.update(m)
    return score, p


@pytest.mark.parametrize("name", CASE_NAMES)
def test_map_score_equals_reference_averages(name, cases, golden):
    score, p = score_of(name, cases[name], golden)
    for k in ("tp", "fp", "fn", "confusion"):
        assert np.array_equal(score.total[k], golden[f"{name}/total/{k}"]), k
    want_iou = golden[f"{name}/total/iou"]
    assert np.all(np.abs(score.total["iou"] - want_iou) <= RTOL * np.abs(want_iou))
    r = score.result()
    assert r["frames"] == images(cases[name])
    for g in ("All", "Things", "Stuff"):
        pq, sq, rq, n = golden[f"{name}/avg/{g}"]
        assert r[g]["n"] == int(n)
        if n == 0:                                               # the stated deviation: the reference divides by zero here
            assert (r[g]["pq"], r[g]["sq"], r[g]["rq"]) == (0.0, 0.0, 0.0)
        else:
            assert close(r[g]["pq"], pq) and close(r[g]["sq"], sq) and close(r[g]["rq"], rq), (g, r[g], pq, sq, rq)
    for c in range(p["num_classes"]):
        for i, k in enumerate(("pq", "sq", "rq")):
            assert close(r["per_class"][c][k], golden[f"{name}/avg/per_class"][c, i]), (c, k)
    for i, k in enumerate(("mIoU", "fwIoU", "mACC", "pACC")):
        assert close(r[k], golden[f"{name}/avg/semantic"][i]), (k, r[k], golden[f"{name}/avg/semantic"][i])


def test_map_score_accumulates_per_frame_index_and_writes(cases, golden, tmp_path):
    name = "clip_33x65"                                          # [B=2, T=3]
    score, p = score_of(name, cases[name], golden)
    r = score.result()
    assert len(r["per_frame"]) == 3
    for t in range(3):
        alone = evaluate.MapScore(**p)
        for b in range(2):
            n = b * 3 + t
            alone.update({**{k: golden[f"{name}/{n}/{k}"][None] for k in FIELDS}, "overflow": np.zeros(1, bool)})
        want = alone.result()
        assert "per_frame" not in want
        assert {k: v for k, v in r["per_frame"][t].items()} == {k: v for k, v in want.items() if k != "frames"}
    twice = evaluate.MapScore(**p)
    for _ in range(2):
        twice.update({**{k: np.stack([golden[f"{name}/{n}/{k}"] for n in range(6)]).reshape((2, 3) + golden[f"{name}/0/{k}"].shape)
                         for k in FIELDS}, "overflow": np.zeros((2, 3), bool)})
    assert np.array_equal(twice.total["tp"], 2 * score.total["tp"]) and twice.result()["frames"] == 12
    with pytest.raises(ValueError, match="different numbers of predicted frames"):
        twice.update({**{k: golden[f"{name}/0/{k}"][None] for k in FIELDS}, "overflow": np.zeros(1, bool)})
    path = tmp_path / "scores.txt"
    assert score.write(str(path)) == r
    score.write(str(path))                                       # appends
    text = path.read_text()
    assert text.count("frames 6\n") == 2 and f"All pq {r['All']['pq']} " in text and f"frame2_mIoU {r['per_frame'][2]['mIoU']}\n" in text


def test_map_score_refuses_an_overflowed_frame(cases, golden):
    name = "px_1x1"
    m = {**{k: golden[f"{name}/0/{k}"][None] for k in FIELDS}, "overflow": np.ones(1, bool)}
    with pytest.raises(ValueError, match="max_pairs"):
        evaluate.MapScore().update(m)


def test_host_checks_come_before_any_launch():
    a = torch.zeros(1, 2, 4, 6, dtype=torch.int32)
    with pytest.raises(TypeError, match="unknown parameter"):
        evaluate.map_quality(a, a, stuff_area=3)
    with pytest.raises(TypeError, match="unknown parameter"):
        evaluate.MapScore(top_k=3)
    with pytest.raises(ValueError, match="max_pairs"):
        evaluate.map_quality(a, a, max_pairs=3000)
    with pytest.raises(ValueError, match="num_classes"):
        evaluate.map_quality(a, a, num_classes=256)
    with pytest.raises(ValueError, match="shape"):
        evaluate.map_quality(a, a[:, :1])
    with pytest.raises(ValueError, match="dtype"):
        evaluate.map_quality(a, a.to(torch.uint8))
    with pytest.raises(ValueError, match="int32 or uint8"):
        evaluate.map_quality(a.long(), a.long())                 # a dtype that could hide negative values is refused outright
    for bad in (0, 2 ** 20):
        with pytest.raises(ValueError, match="label_divisor"):
            evaluate.map_quality(a, a, label_divisor=bad)
    with pytest.raises(ValueError, match=r"\[B,T,H,W\]"):
        evaluate.map_quality(a[0, 0], a[0, 0])
    with pytest.raises(ValueError, match="thing_list"):
        evaluate.map_quality(a, a, thing_list=(19,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # [B,1,T,H,W] against [B,T,H,W]: one clip, the checks pass
        evaluate.map_quality(a[:, None], a)
    with pytest.raises(ValueError, match="shape"):
        evaluate.map_quality(a[:, None], a[:, :1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # every check passed: a host tensor is refused, never scored
        evaluate.map_quality(a, a)


def test_both_maps_are_guarded_on_the_launch_path(monkeypatch):
    """The device guards look at every operand (a host tensor or another GPU's in any position), and map_quality hands them gt as
    well as pred."""
    from c2m_amd import ops
    monkeypatch.setattr(ops, "_cur_device", lambda: 0)
    on = lambda index: type("OnGpu", (), {"is_cuda": True, "device": type("device", (), {"index": index})()})()
    ops._on_current_device(on(0), on(0), None)
    for operands in ((on(1), on(0)), (on(0), on(1)), (None, on(0), on(1))):
        with pytest.raises(RuntimeError, match="tensor on cuda:1 but the current device is cuda:0"):
            ops._on_current_device(*operands)
    host = torch.zeros(1, 4, 6, dtype=torch.int32)
    ops._hip_only(None, None)
    for operands in ((host, None), (None, host)):
        with pytest.raises(RuntimeError, match="HIP device .no CPU fallback by design.$"):
            ops._hip_only(*operands)

    class Reached(Exception):
        pass

    seen = {}

    def on_current_device(*ts, **kw):
        seen["current"] = ts
        raise Reached

    monkeypatch.setattr(ops, "_hip_only", lambda *ts, **kw: seen.__setitem__("hip", ts))
    monkeypatch.setattr(ops, "_on_current_device", on_current_device)
    pred, gt = host, host.clone()
    with pytest.raises(Reached):
        ops.map_quality(pred, gt, 19, tuple(range(11, 19)), 1000, 255, 1 << 12)
    for guard in ("hip", "current"):
        assert any(t is pred for t in seen[guard]) and any(t is gt for t in seen[guard]), guard
