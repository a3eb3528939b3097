"""tests/detect_np.py against the live reference's recorded results (tests/golden/detect_reference.npz, written by
tools/capture_detect_golden.py), the margins every planted GPU case must keep, the YOLOv3 table, the weights file layout and
the score arithmetic.  No GPU.

Planted objects of part (c), in index order: 0 found in both; 1 found in the ground truth only; 2 not found; 3 under 0.5 % of
the frame (skipped); 4 two overlapping candidates of which the later, larger overlap wins; 5 a detection with a negative corner;
6 a detection under 1 % of the frame; 7 found, in an image whose predicted frame has no detection at all."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import detect_np as D
from c2m_amd.modules.networks.yolo_v3 import Darknet, parse_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY_CFG = os.path.join(GOLDEN, "detect_tiny.cfg")
TINY_ANCHORS = [[(36, 28), (44, 52), (60, 60)], [(12, 20), (20, 16), (20, 36)], [(4, 5), (6, 10), (10, 8)]]


@functools.lru_cache(maxsize=None)
def _fx():
    return dict(np.load(os.path.join(GOLDEN, "detect_reference.npz")))


def test_yolov3_table_matches_the_reference_net():
    fx = _fx()
    net = Darknet()
    assert len(net.module_defs) == 107 and len(net.heads) == 3 and net.num_classes == 80
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == json.loads(str(fx["full_state"]))
    assert sum(t.numel() for t in net._conv_tensors()) == int(fx["full_floats"])


def test_tiny_weights_round_trip_and_truncation(tmp_path):
    fx = _fx()
    src = tmp_path / "tiny.weights"
    fx["tiny_weights"].tofile(src)
    net = Darknet(TINY_CFG)
    assert net.anchors == TINY_ANCHORS
    net.load_darknet_weights(str(src))
    net.save_darknet_weights(str(tmp_path / "again.weights"))
    assert np.array_equal(np.fromfile(tmp_path / "again.weights", dtype=np.uint8), fx["tiny_weights"])
    fx["tiny_weights"][:-4].tofile(tmp_path / "short.weights")
    with pytest.raises(ValueError, match=r"holds \d+ floats, this net reads \d+"):
        net.load_darknet_weights(str(tmp_path / "short.weights"))
    np.concatenate([fx["tiny_weights"], np.zeros(4, np.uint8)]).tofile(tmp_path / "long.weights")
    with pytest.raises(ValueError):
        net.load_darknet_weights(str(tmp_path / "long.weights"))
    with pytest.raises(FileNotFoundError):
        net.load_darknet_weights(str(tmp_path / "missing.weights"))


def test_reference_keyed_state_dict_loads_strictly():
    names = json.loads(str(_fx()["full_state"]))
    sd = {k: torch.zeros(shape, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, shape in names}
    Darknet().load_state_dict(sd, strict=True)


def test_cfg_parser():
    blocks = parse_config(TINY_CFG)
    assert blocks[0]["type"] == "net" and len(blocks) == 29
    assert parse_config("[net]\nchannels = 3 # c\n[yolo]\nmask=0")[1] == {"type": "yolo", "mask": "0"}
    with pytest.raises(ValueError):
        parse_config("[convolutional]\nfilters=1\n")


def test_decode_and_suppression_reproduce_the_reference_on_the_tiny_net():
    fx = _fx()
    heads = [fx[f"tiny_heads_{i}"] for i in range(3)]
    pred = D.np_decode(heads, TINY_ANCHORS, 2, 64)
    assert pred.shape == fx["tiny_decoded"].shape == (1, 252, 7)
    np.testing.assert_allclose(pred, fx["tiny_decoded"], rtol=1e-5, atol=1e-5)
    res, margin = D.np_detect(heads, TINY_ANCHORS, 2, 64)
    dets, merged, _ = res[0]
    want = fx["tiny_nms"]
    assert dets.shape == want.shape and np.array_equal(dets[:, 6], want[:, 6])
    assert margin["conf"] > D.BOUNDS["conf"] and margin["iou"] > D.BOUNDS["iou"] and margin["score"] > D.BOUNDS["score"]
    # the merge alone, on the reference's OWN fp32 decode: its corners c -+ size / 2 and its scores are single fp32 operations on
    # fp32 values, so rounding the float64 results to fp32 gives its inputs exactly; then the issue's bound holds with nothing added
    rows, score, _ = D.np_candidates(fx["tiny_decoded"][0].astype(np.float64))
    rows[:, :4] = rows[:, :4].astype(np.float32)
    own, own_merged, _ = D.np_nms(rows, score.astype(np.float32).astype(np.float64))
    assert np.array_equal(own_merged, merged) and np.array_equal(own[:, 4:].astype(np.float32), want[:, 4:])
    for r in range(len(want)):
        assert np.max(np.abs(own[r, :4] - want[r, :4])) <= D.corner_bound(int(merged[r]), want[r])


@pytest.mark.parametrize("tag", ["s1", "s2"])
def test_matching_reproduces_compute_detection(tag):
    fx = _fx()
    heads = [fx[f"planted_heads_{i}"] for i in range(3)]
    res, margin = D.np_detect(heads, D.YOLOV3_ANCHORS, 2, 416)
    ok, bad = D.margins_ok(margin)
    assert ok, bad
    H, W = (int(v) for v in fx[f"{tag}_size"])
    s = D.detect_scale(W)
    dets = [r[0] for r in res]
    flags, boxes, err, lists, m2 = D.np_match(dets[:2], dets[2:], fx["planted_index"], fx[f"{tag}_roi"], fx["planted_x"],
                                              fx["planted_batch"], s, (H * s, W * s))
    assert lists["gt_detected_images"] == fx[f"{tag}_gt_detected"].astype(int).tolist()
    assert lists["pred_detected_images"] == fx[f"{tag}_pred_detected"].astype(int).tolist()
    assert lists["mse_batch"] == fx[f"{tag}_mse"].tolist()
    np.testing.assert_allclose(lists["mse_normalized_batch"], fx[f"{tag}_mse_normalized"], rtol=1e-12)
    assert flags[:, 0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and flags[:, 1].tolist() == [1, 1, 0, 0, 1, 0, 0, 1]
    assert m2["area"] > D.BOUNDS["area"] and m2["overlap"] >= 1 and m2["skip"] > 1e-9
    assert boxes[4, :4].tolist() == [71, 201, 119, 249], "the larger overlap wins over the higher score"


@pytest.mark.parametrize("C", [3, 80])
def test_planted_gpu_cases_keep_their_margins(C):
    for name, heads in D.small_cases(C).items():
        res, margin = D.np_detect(heads, D.YOLOV3_ANCHORS, C, D.S_SMALL)
        ok, bad = D.margins_ok(margin)
        assert ok, (name, bad)
        if name == "one_merge_and_chain":                      # A takes B; C, which overlaps B only, stays
            assert [len(r[0]) for r in res] == [1, 2] and res[0][1].tolist() == [12] and res[1][1].tolist() == [2, 1]
        if name == "classes":
            assert len(res[0][0]) == 3 and len(res[1][0]) == 0


def test_full_size_case_keeps_its_margins():
    heads, C, G, S = D.full_case()
    pred = D.np_decode(heads, D.YOLOV3_ANCHORS, C, S)[0]
    rows, score, m = D.np_candidates(pred)
    assert len(rows) == 10647 and m["conf"] > D.BOUNDS["conf"]
    assert np.min(-np.diff(np.sort(score)[::-1])) > D.BOUNDS["score"]
    for c in range(C):                                         # nothing merges: every same-class pair, in chunks
        r = rows[rows[:, 6] == c]
        for i0 in range(0, len(r), 256):
            a = r[i0:i0 + 256, None, :]
            iw = np.clip(np.minimum(a[..., 2], r[None, :, 2]) - np.maximum(a[..., 0], r[None, :, 0]) + 1, 0, None)
            ih = np.clip(np.minimum(a[..., 3], r[None, :, 3]) - np.maximum(a[..., 1], r[None, :, 1]) + 1, 0, None)
            inter = iw * ih
            area = (r[:, 2] - r[:, 0] + 1) * (r[:, 3] - r[:, 1] + 1)
            iou = inter / (area[i0:i0 + 256, None] + area[None, :] - inter + 1e-16)
            iou[np.arange(iou.shape[0]), i0 + np.arange(iou.shape[0])] = 0
            assert iou.max() < 0.4 - D.BOUNDS["iou"]
    dist = np.abs(rows[:, :4] - np.round(rows[:, :4])).min()                # corners away from integers: n = 1 merge + decode
    assert dist > 5 * D.ULP * 416 + D.decode_bound(rows).max()


def test_preprocessing_restatement_equals_torch():
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    for shape in ((8, 12), (4, 256), (4, 224)):
        x = rng.random((2, 3) + shape, dtype=np.float32)
        t = torch.from_numpy(x)
        s = D.detect_scale(shape[1])
        if s == 2:
            t = F.interpolate(t, scale_factor=2, mode="nearest")
        t = F.pad(t, (0, 416 - t.shape[-1], 0, 416 - t.shape[-2]))
        got, gs, size = D.np_detect_input(x)
        assert gs == s and size == (shape[0] * s, shape[1] * s) and np.array_equal(got, t.numpy())


def test_score_equals_sklearn_and_the_restatement():
    from c2m_amd.evaluate import DetectionScore, accuracy, binary_f1
    rng = np.random.default_rng(3)
    try:
        from sklearn.metrics import accuracy_score, f1_score
    except ImportError:
        accuracy_score = f1_score = None
    for _ in range(20):
        n = int(rng.integers(1, 30))
        t, p = rng.integers(0, 2, n).tolist(), rng.integers(0, 2, n).tolist()
        if f1_score is not None:
            assert binary_f1(t, p) == pytest.approx(f1_score(t, p)) and accuracy(t, p) == pytest.approx(accuracy_score(t, p))
        k = int(rng.integers(0, n + 1))
        sc = DetectionScore()
        sc.update(mse_batch=[1.0, 3.0], mse_normalized_batch=[0.5, 0.25], gt_detected_images=[1] * n, pred_detected_images=[1] * k)
        f1, acc = D.np_score([1] * n, [1] * k)
        r = sc.result()
        assert r["f1"] == pytest.approx(f1) and r["accuracy"] == pytest.approx(acc) and r["mse_traj"] == 2.0
        assert (r["gt_detection"], r["pred_detection"]) == (n, k)


def test_score_write(tmp_path):
    from c2m_amd.evaluate import DetectionScore
    sc = DetectionScore()
    sc.update(mse_batch=[2.0], mse_normalized_batch=[0.5], gt_detected_images=[1, 1], pred_detected_images=[1])
    sc.write(tmp_path / "results.txt")
    lines = (tmp_path / "results.txt").read_text().splitlines()
    assert lines[0].startswith("f1 score 0.666") and lines[1] == "accuracy score 0.5 gt_detection 2 pred_detection1"
    assert lines[2] == "mse_traj_loss 2.0" and lines[3] == "mse_normalized_traj_loss 0.5"


def test_fold_follows_versions_and_refold_covers_data_edits():
    net = Darknet(TINY_CFG).eval()
    w0, b0 = net._fold(0)
    assert net._fold(0)[0] is w0, "cached"
    bn = net.module_list[0][1]
    with torch.no_grad():
        bn.weight.mul_(2.0)                                    # bumps the version: refolded
    w1, _ = net._fold(0)
    assert torch.allclose(w1, 2 * w0)
    bn.weight.data.mul_(0.5)                                   # invisible to the version counter: stale until refold()
    assert net._fold(0)[0] is w1
    net.refold()
    assert torch.allclose(net._fold(0)[0], w0)
    want = net.module_list[0][0].weight.double() * (bn.weight.double() / torch.sqrt(bn.running_var.double() + 1e-5)).view(-1, 1, 1, 1)
    assert torch.equal(net._fold(0)[0], want.float())


def test_a_path_with_a_bracket_is_opened_as_a_path(tmp_path):
    d = tmp_path / "cfg[1]"
    d.mkdir()
    (d / "tiny.cfg").write_text(open(TINY_CFG).read())
    assert parse_config(str(d / "tiny.cfg")) == parse_config(TINY_CFG) == parse_config(open(TINY_CFG).read())
    with pytest.raises(FileNotFoundError):
        parse_config("[net]")
