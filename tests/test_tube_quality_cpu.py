"""Video panoptic quality, the parts that need no GPU: the numpy restatement of the contract (tests/tube_quality_np.py: a window
is map_quality_np.image_quality on its frames stacked into one image) is held, window by window and with exact equality, the
float64 IoU sums included, to what the reference computed on the same stacks (tests/golden/tube_quality_reference.npz, written by
tools/capture_tube_quality_golden.py from cityscapesscripts' pq_compute_single_core / pq_average); evaluate.TubeScore's
arithmetic is fed with the recorded per-window values; the id-swap scene shows what the measure is for; and the checks
evaluate.tube_quality, tracking.anchor_maps and ops.instance_relabel make on the host before anything is launched.

The tolerance of the averages, relative 1e-12, is DESIGN 4.2j's bound for reordered float64 additions: TubeScore adds the
per-window IoU sums in the order they arrive and the reference adds match by match, so the totals differ by the rounding of the
additions only; every figure is the result of fewer than 10^4 float64 additions and divisions, each within 2^-53 relative:
10^4 * 2^-53 = 1.1e-12."""
import os

import numpy as np
import pytest
import torch

import tube_quality_np as TQ
from c2m_amd import evaluate, ops, tracking

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tube_quality_reference.npz")
CASE_NAMES = sorted(TQ.cases())
RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return TQ.cases()


def test_fixture_is_small_and_holds_the_cases_inputs(cases, golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    for name, c in cases.items():
        for k in ("pred", "gt"):
            assert golden[f"{name}/{k}"].dtype == c[k].dtype and np.array_equal(golden[f"{name}/{k}"], c[k]), (name, k)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_reference_per_window(name, cases, golden):
    c = cases[name]
    p = TQ.restatement_params(c["params"])
    B, T = c["pred"].shape[:2]
    for k in c["windows"]:
        got = TQ.clip_quality(c["pred"], c["gt"], k, **p)
        for f in TQ.FIELDS:
            want = golden[f"{name}/k{k}/{f}"]
            assert got[f].shape == (B, T - k + 1, p["num_classes"]) and got[f].dtype == want.dtype, (name, k, f)
            assert np.array_equal(got[f], want), (name, k, f)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_fit_their_pair_tables_but_the_overflow_cases(name, cases):
    """A check of the cases themselves: every window has at most max_pairs distinct same-class pairs, so its counts are
    complete; the overflow cases are the exception, and there exactly the windows they are built for."""
    over = TQ.expected_overflow(cases[name])
    if name not in TQ.OVERFLOW_CASES:
        assert not any(v.any() for v in over.values())
    elif name == "pairs_over":
        assert over[1].tolist() == [[False] * 4] and over[2].tolist() == [[True, False, False]]
    else:
        assert over[1].tolist() == [[False, True, False, False]] and over[2].tolist() == [[True, True, False]]
        assert over[4].tolist() == [[True]]
    if name == "pairs_exact":                                    # one window sits exactly at the table's size
        c = cases[name]
        assert TQ.window_pairs(c["pred"][0, 0:2], c["gt"][0, 0:2], **TQ.restatement_params(c["params"])) == c["params"]["max_pairs"]


def result_of(name, case, golden):
    B, T = case["pred"].shape[:2]
    return {k: {**{f: golden[f"{name}/k{k}/{f}"] for f in TQ.FIELDS}, "overflow": np.zeros((B, T - k + 1), bool)}
            for k in case["windows"]}


def close(got, want):
    return abs(got - want) <= RTOL * abs(want)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_tube_score_equals_reference_averages(name, cases, golden):
    c = cases[name]
    p = TQ.restatement_params(c["params"])
    score = evaluate.TubeScore(**p)
    score.update(result_of(name, c, golden))
    r = score.result()
    B, T = c["pred"].shape[:2]
    assert r["windows"] == sum(B * (T - k + 1) for k in c["windows"]) and sorted(r["per_k"]) == sorted(c["windows"])
    for k in c["windows"]:
        for f in ("tp", "fp", "fn"):
            assert np.array_equal(score.total[k][f], golden[f"{name}/k{k}/total/{f}"]), (k, f)
        want_iou = golden[f"{name}/k{k}/total/iou"]
        assert np.all(np.abs(score.total[k]["iou"] - want_iou) <= RTOL * np.abs(want_iou))
        for g in ("All", "Things", "Stuff"):
            pq, sq, rq, n = golden[f"{name}/k{k}/avg/{g}"]
            got = r["per_k"][k][g]
            assert got["n"] == int(n)
            if n == 0:                                           # the stated deviation of pq_average: the reference divides by zero
                assert (got["pq"], got["sq"], got["rq"]) == (0.0, 0.0, 0.0)
            else:
                assert close(got["pq"], pq) and close(got["sq"], sq) and close(got["rq"], rq), (k, g, got, pq, sq, rq)
    for key, g in (("vpq", "All"), ("vpq_things", "Things"), ("vpq_stuff", "Stuff")):
        per_k = [golden[f"{name}/k{k}/avg/{g}"] for k in c["windows"]]
        want = float(np.mean([a[0] if a[3] else 0.0 for a in per_k]))
        assert abs(r[key] - want) <= RTOL * abs(want), (key, r[key], want)


def test_id_swap_is_invisible_per_frame_and_costs_two_fp_and_two_fn_per_tube(cases):
    c = cases["id_swap"]
    p = TQ.restatement_params(c["params"])
    car = 13
    q = {k: TQ.clip_quality(c["pred"], c["gt"], k, **p) for k in c["windows"]}
    assert q[1]["tp"][0, :, car].tolist() == [2, 2, 2, 2] and not q[1]["fp"].any() and not q[1]["fn"].any()
    assert np.array_equal(q[1]["iou"], q[1]["tp"].astype(np.float64))           # per-frame PQ is 1, of the things as well
    straddles = {2: [False, True, False], 3: [True, True], 4: [True]}             # the ids swap between frames 1 and 2
    for k, rows in straddles.items():
        for t0, hit in enumerate(rows):
            got = tuple(int(q[k][f][0, t0, car]) for f in ("tp", "fp", "fn"))
            assert got == ((0, 2, 2) if hit else (2, 0, 0)), (k, t0, got)
    score = evaluate.TubeScore()
    score.update({k: {**q[k], "overflow": np.zeros(q[k]["tp"].shape[:2], bool)} for k in q})
    r = score.result()
    assert r["per_k"][1]["Things"]["pq"] == 1.0 and r["per_k"][4]["Things"]["pq"] == 0.0
    assert r["vpq_things"] == (1.0 + r["per_k"][2]["Things"]["pq"] + 0.0 + 0.0) / 4 and r["vpq_stuff"] == 1.0
    # the per-object figure: each id's predicted tube covers its own car only in the frames before the swap
    iou, ga, pa = TQ.clip_id_quality(c["pred"], c["gt"], c["ids"], 4, **p)
    assert iou[0, 0].tolist() == [24 / 72, 24 / 72] and ga[0, 0].tolist() == [48, 48] and pa[0, 0].tolist() == [48, 48]


def test_tube_score_sums_updates_reports_id_iou_and_writes(cases, golden, tmp_path):
    name = "clips_24x40"
    c = cases[name]
    res = result_of(name, c, golden)
    for k in res:
        res[k]["id_iou"] = np.full(res[k]["tp"].shape[:2] + (3,), -1.0)
        res[k]["id_iou"][0, 0] = [0.25, -1.0, 0.75]
    once, twice = evaluate.TubeScore(), evaluate.TubeScore()
    once.update(res)
    twice.update(res)
    twice.update(res)
    for k in res:
        assert np.array_equal(twice.total[k]["tp"], 2 * once.total[k]["tp"])
    r = twice.result()
    assert r["windows"] == 2 * once.result()["windows"]
    assert all(s["id_iou"] == 0.5 and s["id_n"] == 4 for s in r["per_k"].values())
    assert once.result()["vpq"] == sum(once.result()["per_k"][k]["All"]["pq"] for k in sorted(res)) / len(res)
    with pytest.raises(ValueError, match="different window lengths"):
        twice.update({1: res[1]})
    path = tmp_path / "tubes.txt"
    assert twice.write(str(path)) == r
    twice.write(str(path))                                       # appends
    text = path.read_text()
    assert text.count(f"windows {r['windows']}\n") == 2 and f"vpq {r['vpq']} " in text
    assert f"k5_All pq {r['per_k'][5]['All']['pq']} " in text and "k2_id_iou 0.5 n 4\n" in text
    plain = evaluate.TubeScore()
    plain.update(result_of(name, c, golden))
    assert plain.result()["per_k"][1]["id_iou"] is None


def test_tube_score_refuses_an_overflowed_window(cases, golden):
    res = result_of("pairs_exact", cases["pairs_exact"], golden)
    res[2]["overflow"][0, 1] = True
    with pytest.raises(ValueError, match="max_pairs"):
        evaluate.TubeScore(max_pairs=8).update(res)
    with pytest.raises(TypeError, match="unknown parameter"):
        evaluate.TubeScore(top_k=3)


def test_host_checks_come_before_any_launch():
    a = torch.zeros(2, 3, 4, 6, dtype=torch.int32)
    with pytest.raises(TypeError, match="unknown parameter"):
        evaluate.tube_quality(a, a, stuff_area=3)
    for bad in ((0,), (4,), (1, 1), (2, "all", 3), (), ("every",), (1.5,), (True,)):
        with pytest.raises(ValueError, match="window"):
            evaluate.tube_quality(a, a, windows=bad)
    with pytest.raises(ValueError, match="window"):              # the default (1, 2, 3, 4) in clips of three frames
        evaluate.tube_quality(a, a)
    w = dict(windows=(1, "all"))
    with pytest.raises(ValueError, match="max_pairs"):
        evaluate.tube_quality(a, a, max_pairs=3000, **w)
    with pytest.raises(ValueError, match="shape"):
        evaluate.tube_quality(a, a[:, :1], **w)
    with pytest.raises(ValueError, match="dtype"):
        evaluate.tube_quality(a, a.to(torch.uint8), **w)
    with pytest.raises(ValueError, match="int32 or uint8"):
        evaluate.tube_quality(a.long(), a.long(), **w)
    with pytest.raises(ValueError, match=r"\[B,T,H,W\]"):
        evaluate.tube_quality(a[0], a[0], **w)
    for ids in (torch.zeros(2, 3), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                torch.zeros(2, 0, dtype=torch.int32), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="ids"):
            evaluate.tube_quality(a, a, ids=ids, **w)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tube_quality(a[..., ::2], a[..., ::2], (1,), None, 19, tuple(range(11, 19)), 1000, 255, 1 << 12)
    big = torch.empty(1, 2 ** 11, 2 ** 10, 2 ** 10, dtype=torch.uint8, device="meta")   # T * H * W = 2**31, no memory behind it
    with pytest.raises(ValueError, match=r"T \* H \* W"):
        ops._tube_quality_plan(big, big, (1,), None, 19, tuple(range(11, 19)), 1000, 255, 1 << 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # [B,1,T,H,W] against [B,T,H,W]: one clip, the checks pass
        evaluate.tube_quality(a[:, None], a, ids=torch.zeros(2, 2, dtype=torch.int32), **w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # every check passed: a host tensor is refused, never scored
        evaluate.tube_quality(a, a, **w)


def test_relabel_and_anchor_maps_host_checks():
    m = torch.zeros(2, 3, 4, 6, dtype=torch.int32)
    frm, to, cnt = np.zeros((6, 2), np.int64), np.zeros((6, 2), np.int64), np.zeros(6, np.int64)
    things = tuple(range(11, 19))
    with pytest.raises(ValueError, match="int32"):
        ops.instance_relabel(m.long(), frm, to, cnt, things)
    with pytest.raises(ValueError, match="contiguous"):
        ops.instance_relabel(m[..., ::2], frm, to, cnt, things)
    with pytest.raises(ValueError, match="pairs_from"):
        ops.instance_relabel(m, frm[:5], to, cnt, things)
    with pytest.raises(ValueError, match="pairs_from"):
        ops.instance_relabel(m, np.zeros((6, 65), np.int64), np.zeros((6, 65), np.int64), cnt, things)
    with pytest.raises(ValueError, match="count"):
        ops.instance_relabel(m, frm, to, cnt + 3, things)
    with pytest.raises(ValueError, match="twice"):
        ops.instance_relabel(m, frm, to, cnt + 2, things)
    with pytest.raises(ValueError, match="label_divisor"):
        ops.instance_relabel(m, frm, to, cnt, things, label_divisor=0)
    with pytest.raises(ValueError, match="thing_list"):
        ops.instance_relabel(m, frm, to, cnt, (300,))
    pl = ops._instance_relabel_plan(m[0, :2], np.array([[9, 5, 7], [3, 1, 2]]), np.array([[90, 50, 70], [30, 10, 20]]),
                                    np.array([3, 2]), things, 1000)
    tab = pl.table
    assert tab[:3].tolist() == [5, 7, 9] and tab[128:131].tolist() == [50, 70, 90]            # sorted by `from`, `to` alongside
    assert tab[64:67].tolist() == [1, 3, 0] and tab[192:195].tolist() == [10, 30, 0] and tab[256:].tolist() == [3, 2]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.instance_relabel(m, frm, to, cnt, things)
    tr = tracking.Tracks(torch.zeros(2, 64, 3, dtype=torch.int32), torch.zeros(2, 64, 3, 4, dtype=torch.int32),
                         torch.tensor([2, 1], dtype=torch.int32))
    tr.ids[0, 0], tr.ids[0, 1], tr.ids[1, 0] = torch.tensor([13005, 13001, 13002]), torch.tensor([13001, 13002, 13001]), 11001
    frm, to, cnt = tracking.anchor_pairs(tr, 2)
    assert frm.shape == (6, 64) and cnt.tolist() == [2, 2, 2, 1, 1, 1]
    assert frm[:3, :2].tolist() == [[13005, 13001], [13001, 13002], [13002, 13001]] and to[:3, :2].tolist() == [[13001, 13002]] * 3
    with pytest.raises(TypeError, match="int32"):
        tracking.anchor_maps(m.long(), tr, 2)
    with pytest.raises(ValueError, match="frames"):
        tracking.anchor_maps(m[:, :2], tr, 2)
    with pytest.raises(ValueError, match="num_input_frames"):
        tracking.anchor_maps(m, tr, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tracking.anchor_maps(m[:, None], tr, 2)
