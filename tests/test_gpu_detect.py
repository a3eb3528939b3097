"""csrc/detect.hip, the Darknet forward and c2m_amd.evaluate on the device, against tests/detect_np.py (pinned to the live
reference's recorded results by test_detect_cpu.py, which also asserts the margins that let these tests demand EQUAL decisions)
and against tests/golden/detect_reference.npz.

Network tolerance: the reference's own fp32 forward differs from its float64 evaluation by `ref_fp32_error` (max-abs over
max-abs, 3.3e-7 on the fixture net); the test allows NET_MARGIN times that for Winograd transforms and another summation order.
Observed on an MI355X: see DESIGN §4.2f."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detect_np as D
from c2m_amd import evaluate, ops
from c2m_amd.modules.networks.yolo_v3 import Darknet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY_CFG = os.path.join(GOLDEN, "detect_tiny.cfg")
NET_MARGIN = 4


@functools.lru_cache(maxsize=None)
def _fixture():
    return dict(np.load(os.path.join(GOLDEN, "detect_reference.npz")))


@functools.lru_cache(maxsize=None)
def _cases(C):
    return D.small_cases(C)


@functools.lru_cache(maxsize=None)
def _want(C, name):
    return D.np_detect(_cases(C)[name], D.YOLOV3_ANCHORS, C, D.S_SMALL)[0]


def _run(heads, C, img_size):
    hs = [torch.from_numpy(h).to(DEV) for h in heads]
    cand, score, count = ops.yolo_candidates(hs, D.YOLOV3_ANCHORS, C, img_size, 0.5)
    dets, kept = ops.nms_merge(cand, score, count, 0.4)
    return cand.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy(), dets.cpu().numpy(), kept.cpu().numpy()


def _check_candidates(c, rows):
    """Device candidate rows against the float64 decode: class and order equal, corners within the decode's derived bound
    (detect_np.decode_bound), confidences within the sigmoid's 4 roundings (8 ulp allowed, relative)."""
    assert np.array_equal(c[:, 6], rows[:, 6]), "candidate classes / order"
    tol = D.decode_bound(rows)
    assert np.all(np.abs(c[:, [0, 2]] - rows[:, [0, 2]]) <= tol[:, :1]) and np.all(np.abs(c[:, [1, 3]] - rows[:, [1, 3]]) <= tol[:, 1:])
    np.testing.assert_allclose(c[:, 4:6], rows[:, 4:6], rtol=8 * D.ULP, atol=0)


def _check(got, want):
    """Decisions against the restatement on the planted maps; the merge itself against the restatement run on the DEVICE's own
    fp32 candidate rows and scores, with the issue's bound alone: (n + 4) * 2^-23 * max|corner|."""
    cand, score, count, dets, kept = got
    for n, (wd, merged, rows) in enumerate(want):
        assert count[n] == len(rows), f"image {n}: {count[n]} candidates, {len(rows)} expected"
        assert kept[n] == len(wd), f"image {n}: kept {kept[n]}, expected {len(wd)}"
        assert not dets[n, kept[n]:].any()
        if not len(rows):
            continue
        c = cand[n, :len(rows)].astype(np.float64)
        _check_candidates(c, rows)
        g = dets[n, :kept[n]]
        assert np.array_equal(g[:, 6], wd[:, 6]), f"image {n}: classes / order of the kept rows"
        own, own_merged, _ = D.np_nms(c, score[n, :len(rows)].astype(np.float64), 0.4)
        assert np.array_equal(own_merged, merged) and np.array_equal(own[:, 4:], g[:, 4:]), f"image {n}: rows, conf, class"
        for r in range(len(own)):
            tol = D.corner_bound(int(merged[r]), own[r])
            assert np.max(np.abs(g[r, :4] - own[r, :4])) <= tol, f"image {n} row {r} (merged from {merged[r]}): " \
                f"{g[r, :4]} vs {own[r, :4]}, tol {tol}"


# ------------------------------------------------------------------------------------------------------------- input
@pytest.mark.parametrize("shape", [(8, 12), (4, 256), (4, 224)])
def test_detect_input_equals_restatement(shape):
    rng = np.random.default_rng(1)
    x = rng.random((2, 3) + shape, dtype=np.float32)
    got, s, size = ops.detect_input(torch.from_numpy(x).to(DEV))
    want, ws, wsize = D.np_detect_input(x)
    assert (s, size) == (ws, wsize) and torch.equal(got.cpu(), torch.from_numpy(want))


def test_detect_input_reads_the_last_frame_through_strides():
    rng = np.random.default_rng(2)
    v = rng.random((2, 3, 4, 10, 14), dtype=np.float32)
    dv = torch.from_numpy(v).to(DEV)
    want = torch.from_numpy(D.np_detect_input(v[:, :, -1])[0])
    assert torch.equal(ops.detect_input(dv)[0].cpu(), want)
    perm = dv.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)        # same values, other strides
    assert torch.equal(ops.detect_input(perm)[0].cpu(), want)


# ------------------------------------------------------------------------------------------ candidates and suppression
@pytest.mark.parametrize("C,name", [(3, "random_and_empty"), (80, "random_and_empty"), (3, "all_pass"), (80, "all_pass"),
                                    (3, "one_merge_and_chain"), (3, "classes")])
def test_candidates_and_suppression_equal_restatement(C, name):
    want = _want(C, name)
    got = _run(_cases(C)[name], C, D.S_SMALL)
    _check(got, want)
    again = _run(_cases(C)[name], C, D.S_SMALL)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two runs differ"
    if name == "one_merge_and_chain":
        assert got[4].tolist() == [1, 2] and want[0][1].tolist() == [12] and want[1][1].tolist() == [2, 1]
    if name == "all_pass":
        assert got[2].tolist() == [567, 567]


def test_every_box_of_a_416_image_survives():
    heads, C, G, S = D.full_case()
    cand, score, count, dets, kept = _run(heads, C, S)
    assert count.tolist() == [10647] and kept.tolist() == [10647]
    rows, want_score, _ = D.np_candidates(D.np_decode(heads, D.YOLOV3_ANCHORS, C, S)[0])
    _check_candidates(cand[0].astype(np.float64), rows)
    order = np.argsort(-want_score, kind="stable")             # nothing merges: the result is the device's candidates, sorted
    assert np.array_equal(np.argsort(-score[0], kind="stable"), order)
    want = cand[0][order]
    assert np.array_equal(dets[0, :, 4:], want[:, 4:])
    tol = 5 * D.ULP * np.abs(want[:, :4]).max(1, keepdims=True)               # conf * corner / conf: the bound at n = 1
    assert np.all(np.abs(dets[0, :, :4] - want[:, :4]) <= tol)


# ----------------------------------------------------------------------------------------------------------- network
def _rel_err(got, want):
    return max(float(np.abs(g.double().cpu().numpy() - w).max()) for g, w in zip(got, want)) / \
        max(float(np.abs(w).max()) for w in want)


def test_tiny_net_matches_reference_float64(tmp_path):
    fx = _fixture()
    path = tmp_path / "tiny.weights"
    fx["tiny_weights"].tofile(path)
    net = Darknet(TINY_CFG)
    net.load_darknet_weights(str(path))
    net.to(DEV).eval()
    heads = net(torch.from_numpy(fx["tiny_input"]).to(DEV))
    err = _rel_err(heads, [fx[f"tiny_heads64_{i}"] for i in range(3)])
    print(f"tiny net: error {err:.3e}, reference fp32 {float(fx['ref_fp32_error']):.3e}")
    assert err <= NET_MARGIN * float(fx["ref_fp32_error"])


def _composite64(net, x):
    """The net from its state_dict with stock float64 ops on the CPU."""
    sd = {k: v.double() for k, v in net.state_dict().items()}
    outs, heads = [], []
    for i, d in enumerate(net.module_defs):
        k = d["type"]
        if k == "convolutional":
            w = sd[f"module_list.{i}.conv_{i}.weight"]
            x = F.conv2d(x, w, sd.get(f"module_list.{i}.conv_{i}.bias"), int(d["stride"]), (w.shape[-1] - 1) // 2)
            p = f"module_list.{i}.batch_norm_{i}."
            if p + "weight" in sd:
                x = F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0,
                                 1e-5)
            if d["activation"] == "leaky":
                x = F.leaky_relu(x, 0.1)
        elif k == "upsample":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        elif k == "route":
            x = torch.cat([outs[int(s)] for s in str(d["layers"]).split(",")], 1)
        elif k == "shortcut":
            x = outs[-1] + outs[int(d["from"])]
        elif k == "yolo":
            heads.append(x)
        outs.append(x)
    return heads


def test_full_net_matches_float64_composite():
    torch.manual_seed(3)
    net = Darknet().eval()
    g = torch.Generator().manual_seed(4)
    for m in net.modules():                                    # statistics away from (0, 1) so that folding is exercised
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.8, 1.6, generator=g)
            m.bias.data.uniform_(-0.2, 0.2, generator=g)
            m.running_mean.data.uniform_(-0.2, 0.2, generator=g)
            m.running_var.data.uniform_(0.5, 1.5, generator=g)
    x = torch.rand(1, 3, 96, 96, generator=g)
    want = [h.numpy() for h in _composite64(net, x.double())]
    heads = net.to(DEV)(x.to(DEV))
    assert [tuple(h.shape) for h in heads] == [(1, 255, 3, 3), (1, 255, 6, 6), (1, 255, 12, 12)]
    err = _rel_err(heads, want)
    print(f"full net: error {err:.3e}, bound {NET_MARGIN * float(_fixture()['ref_fp32_error']):.3e}")
    assert err <= NET_MARGIN * float(_fixture()["ref_fp32_error"])


# -------------------------------------------------------------------------------------------------------- end to end
def _planted(tag):
    fx = _fixture()
    H, W = (int(v) for v in fx[f"{tag}_size"])
    g = type("G", (), {})()
    g.target_frames_nodes_roi = torch.from_numpy(fx[f"{tag}_roi"]).to(DEV)
    g.x, g.batch = torch.from_numpy(fx["planted_x"]).to(DEV), torch.from_numpy(fx["planted_batch"]).to(DEV)
    video = torch.rand(2, 3, 2, H, W, device=DEV)
    heads = [torch.from_numpy(fx[f"planted_heads_{i}"]).to(DEV) for i in range(3)]
    return fx, g, video, heads, torch.from_numpy(fx["planted_index"])


@functools.lru_cache(maxsize=None)
def _plant_detector():
    blocks = [{"type": "net", "channels": 3, "height": 416}]
    anchors = ",".join(f"{w},{h}" for a in D.YOLOV3_ANCHORS[::-1] for w, h in a)
    for mask in ("6,7,8", "3,4,5", "0,1,2"):
        blocks += [{"type": "convolutional", "filters": 21, "size": 1, "stride": 1, "activation": "linear"},
                   {"type": "yolo", "mask": mask, "anchors": anchors, "classes": 2}]
    det = evaluate.Detector.__new__(evaluate.Detector)
    det.net = Darknet(blocks).eval()
    return det


@pytest.mark.parametrize("tag", ["s1", "s2"])
def test_trajectory_metric_reproduces_the_reference(tag):
    fx, g, video, heads, index = _planted(tag)
    det = _plant_detector()
    r = evaluate.trajectory_metric(det, video, video.clone(), g, index, predictions=heads)
    assert r["gt_detected_images"] == fx[f"{tag}_gt_detected"].astype(int).tolist()
    assert r["pred_detected_images"] == fx[f"{tag}_pred_detected"].astype(int).tolist()
    np.testing.assert_allclose(r["mse_batch"], fx[f"{tag}_mse"], rtol=1e-6)
    np.testing.assert_allclose(r["mse_normalized_batch"], fx[f"{tag}_mse_normalized"], rtol=1e-6)
    assert r["skipped"].tolist() == [False, False, False, True, False, False, False, False]
    assert r["gt_found"].tolist() == [True, True, False, False, True, False, False, True]
    assert r["pred_found"].tolist() == [True, False, False, False, True, False, False, False]
    r2 = evaluate.trajectory_metric(det, video, video.clone(), g, index, predictions=heads)
    assert all(torch.equal(r[k], r2[k]) for k in ("gt_box", "pred_box", "mse", "mse_normalized")), "two runs differ"
    score = evaluate.DetectionScore()
    score.update(r)
    assert score.result()["f1"] == pytest.approx(2 * 2 / (2 * 2 + 2)) and score.result()["accuracy"] == 0.5


def test_trajectory_metric_through_a_real_detector(tmp_path):
    fx, g, video, _, index = _planted("s1")
    path = tmp_path / "tiny.weights"
    fx["tiny_weights"].tofile(path)
    det = evaluate.Detector(weights=str(path), config=TINY_CFG, device=DEV)
    a = evaluate.trajectory_metric(det, video, video.flip(-1), g, index)
    b = evaluate.trajectory_metric(det, video, video.flip(-1), g, index)
    assert len(a["skipped"]) == 8 and a["skipped"].tolist()[3]
    assert all(torch.equal(a[k], b[k]) for k in ("gt_box", "pred_box", "mse", "mse_normalized", "gt_found", "pred_found"))
    with pytest.raises(FileNotFoundError):
        evaluate.Detector(weights=str(tmp_path / "missing.weights"), config=TINY_CFG, device=DEV)


def test_validation_happens_before_any_launch():
    det = _plant_detector()
    with pytest.raises(ValueError):
        det.heads(torch.zeros(1, 3, 100, 100, device=DEV))
    with pytest.raises(RuntimeError):
        ops.detect_input(torch.zeros(1, 3, 8, 8))
    fx, g, video, heads, index = _planted("s1")
    del g.x
    with pytest.raises(ValueError):
        evaluate.trajectory_metric(det, video, video, g, index, predictions=heads)
    fx, g, video, heads, index = _planted("s1")
    r = evaluate.trajectory_metric(det, video, video, g, [], predictions=heads)
    assert r["mse_batch"] == [] and len(r["skipped"]) == 0


# ------------------------------------------------------------------------------------------------ documented deviations
def _three(C=3):
    """Three far-apart 20 px boxes of three classes in the stride-8 head of a 96 px image, planted in box order 0 < 1 < 2."""
    A, G, S = D.YOLOV3_ANCHORS, D.GRIDS_SMALL, D.S_SMALL
    at = lambda a, gy, gx: 27 + 108 + (a * 12 + gy) * 12 + gx
    return [at(0, 2, 2), at(0, 6, 6), at(1, 9, 3)], A, G, S


def test_equal_scores_keep_their_box_order():
    """The tie rule: a stable sort, so equal scores come out lower box index first (the reference leaves it undefined)."""
    boxes, A, G, S = _three()
    specs = [D._spec(b, G, A, S, 20.0, 20.0, 0.8, k) for k, b in enumerate(boxes)]
    specs.insert(1, D._spec(27 + 108 + 200, G, A, S, 20.0, 20.0, 0.9, 0))          # a higher score from a LATER box goes first
    cand, score, count, dets, kept = _run(D.plant(1, 3, G, A, S, [specs]), 3, S)
    assert count.tolist() == [4] and kept.tolist() == [4]
    assert score[0, 0] == score[0, 1] == score[0, 3] < score[0, 2], "three bit-equal scores and one above them"
    assert dets[0, :4, 6].tolist() == [0.0, 0.0, 1.0, 2.0]
    assert np.array_equal(dets[0, 1:4, 4:], cand[0, [0, 1, 3], 4:]) and np.array_equal(dets[0, 0, 4:], cand[0, 2, 4:])


def test_a_non_finite_head_is_removed_and_the_loop_ends():
    """A head whose box is NaN overlaps nothing, itself included: the reference never removes it.  Here it leaves with a NaN box
    and the candidates behind it are treated as usual."""
    boxes, A, G, S = _three()
    heads = D.plant(1, 3, G, A, S, [[D._spec(boxes[0], G, A, S, 20.0, 20.0, 0.9, 1), D._spec(boxes[1], G, A, S, 20.0, 20.0, 0.8, 1),
                                     D._spec(boxes[2], G, A, S, 20.0, 20.0, 0.7, 1)]])
    hd, a, gy, gx = D.cell_of(boxes[0], G, A)
    heads[hd][0, a * 8 + 2, gy, gx] = np.nan                                       # the width of the best box
    cand, score, count, dets, kept = _run(heads, 3, S)
    assert count.tolist() == [3] and kept.tolist() == [3]
    assert np.isnan(dets[0, 0, :4]).all() and np.array_equal(dets[0, 0, 4:], cand[0, 0, 4:])
    tol = 5 * D.ULP * np.abs(cand[0, 1:3, :4]).max(1, keepdims=True)              # conf * corner / conf: the bound at n = 1
    assert np.all(np.abs(dets[0, 1:3, :4] - cand[0, 1:3, :4]) <= tol)
    assert np.array_equal(dets[0, 1:3, 4:], cand[0, 1:3, 4:])
