"""Captures tests/golden/detect_reference.npz from the LIVE reference (build container only; needs the reference checkout that
oracle.ref_shims points at).  Nothing of the reference is stored but what its programs compute:

 (a) the full YOLOv3 net: state_dict names and shapes, and the float count save_darknet_weights writes;
 (b) the tiny net of tests/golden/detect_tiny.cfg (our own settings file): its darknet weights bytes, a 64 x 64 input, the raw head
     maps (fp32 and float64), the decoded output, the non_max_suppression result and the reference's own fp32-vs-float64 error;
 (c) compute_detection on planted head maps, for both scale rules; the reference's detector is replaced by a stub that decodes
     the planted maps of the image it is handed with the reference's own YOLOLayer.

    python tools/capture_detect_golden.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_np as D                                   # noqa: E402
from oracle import ref_shims                            # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY_CFG = os.path.join(GOLDEN, "detect_tiny.cfg")
PLANT_GRIDS, PLANT_C, PLANT_SIZE = [2, 4, 8], 2, 416


def planted_case():
    """Head maps for 2B = 4 images (ground truth 0, 1; predicted 2, 3), the graph and the clicked nodes: see the case list in
    tests/test_detect_cpu.py."""
    A, G = D.YOLOV3_ANCHORS, PLANT_GRIDS
    start2 = 3 * (4 + 16)

    def at(cx, cy, w, h, conf, cls, a):
        gx, gy = int(cx // 52), int(cy // 52)
        return {"box": start2 + (a * 8 + gy) * 8 + gx, "cx": cx, "cy": cy, "w": w, "h": h, "conf": conf, "cls": cls,
                "cls_conf": 0.9}

    gt0 = [at(60.45, 50.45, 38.3, 38.3, 0.90, 0, 0),            # object 0: found in both
           at(175.45, 40.45, 48.3, 38.3, 0.85, 0, 0),           # object 1: ground truth only
           at(225.45, 95.45, 48.3, 48.3, 0.70, 0, 0),           # object 4: the larger overlap, lower score ...
           at(235.45, 95.45, 40.3, 48.3, 0.95, 1, 1)]           # ... and the smaller overlap of another class, which comes first
    pr0 = [at(66.65, 53.55, 38.3, 38.3, 0.80, 0, 0), at(222.45, 93.45, 46.3, 46.3, 0.75, 0, 0)]
    gt1 = [at(18.45, 25.45, 42.3, 46.3, 0.90, 0, 0),            # object 5: x1 < 0
           at(109.95, 68.95, 17.3, 15.3, 0.80, 1, 0),           # object 6: under 1 % of the frame
           at(205.45, 60.45, 48.3, 58.3, 0.85, 0, 0)]           # object 7: found; the predicted image has no detection at all
    heads = D.plant(4, PLANT_C, G, A, PLANT_SIZE, [gt0, gt1, pr0, []])
    roi = np.zeros((10, 3, 4), np.float32)
    roi[:, -1] = [[40.4, 80.6, 30.2, 70.7], [150.3, 200.5, 20.2, 60.4], [100.2, 140.3, 80.1, 120.6], [10.1, 20.3, 100.2, 110.4],
                  [200.2, 250.4, 70.3, 120.5], [0.0, 40.5, 0.0, 50.5], [100.3, 118.6, 60.2, 76.4], [180.2, 230.4, 30.3, 90.5],
                  [5.0, 9.0, 5.0, 9.0], [5.0, 9.0, 5.0, 9.0]]
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.9, 0.9, (10, 2, 6)).astype(np.float32)
    batch = np.array([0] * 5 + [1] * 5, np.int64)
    return heads, roi, x, batch, np.arange(8, dtype=np.int64)


def capture_planted(rm, uy, out):
    heads, roi, x, batch, index = planted_case()
    layers = [rm.YOLOLayer(a, PLANT_C, PLANT_SIZE) for a in D.YOLOV3_ANCHORS]

    def stub(image):                                            # the image carries its own number in its first pixel
        n = int(round(float(image[0, 0, 0, 0]) * 8))
        return torch.cat([layer(torch.from_numpy(h[n:n + 1]), None, PLANT_SIZE)[0] for layer, h in zip(layers, heads)], 1)

    for i, h in enumerate(heads):
        out[f"planted_heads_{i}"] = h
    out["planted_x"], out["planted_batch"], out["planted_index"] = x, batch, index
    for tag, (H, W) in (("s1", (128, 256)), ("s2", (64, 128))):
        scale = 1 if W in (256, 320) else 2
        r = roi / scale
        video, gen = torch.rand(2, 3, 2, H, W), torch.rand(2, 3, 2, H, W)
        for b in range(2):
            video[b, 0, -1, 0, 0] = b / 8
            gen[b, 0, -1, 0, 0] = (2 + b) / 8
        g = type("G", (), {})()
        g.source_frames_nodes_instance_ids = torch.zeros(10, 2, dtype=torch.int64)
        g.batch, g.target_frames_nodes_roi, g.x = torch.from_numpy(batch), torch.from_numpy(r), torch.from_numpy(x)
        res = uy.compute_detection(video, gen, stub, g, ["a", "b"], "cpu", [int(i) for i in index], [["0.png", "1.png"]], "", "")
        out[f"{tag}_size"] = np.array([H, W])
        out[f"{tag}_roi"] = r
        for k, v in zip(("mse", "mse_normalized", "gt_detected", "pred_detected"), res):
            out[f"{tag}_{k}"] = np.array([float(e) for e in v], np.float64)
        print(tag, [list(map(float, v)) for v in res])


def capture_tiny(rm, out):
    torch.manual_seed(11)
    net = rm.Darknet(TINY_CFG, img_size=64)
    g = torch.Generator().manual_seed(12)
    for i, (d, m) in enumerate(zip(net.module_defs, net.module_list)):
        if d["type"] != "convolutional":
            continue
        if d["batch_normalize"]:
            bn = m[1]
            bn.weight.data.uniform_(0.5, 1.5, generator=g)
            bn.bias.data.uniform_(-0.3, 0.3, generator=g)
            bn.running_mean.data.uniform_(-0.3, 0.3, generator=g)
            bn.running_var.data.uniform_(0.5, 1.5, generator=g)
        else:                                                  # the heads: spread the confidences over (0, 1)
            m[0].weight.data.mul_(12.0)
            m[0].bias.data.uniform_(-0.5, 0.5, generator=g)
    net.eval()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.weights")
        net.save_darknet_weights(path)
        out["tiny_weights"] = np.fromfile(path, dtype=np.uint8)
    x = torch.rand(1, 3, 64, 64, generator=g)
    heads_at = [i - 1 for i, d in enumerate(net.module_defs) if d["type"] == "yolo"]

    def run(model, inp):
        got, hooks = [], [model.module_list[i].register_forward_hook(lambda m, a, o: got.append(o.detach().clone()))
                          for i in heads_at]
        with torch.no_grad():
            dec = model(inp)
        for h in hooks:
            h.remove()
        return got, dec

    h32, dec = run(net, x)
    import copy
    h64, _ = run(copy.deepcopy(net).double(), x.double())
    err = max(float((a.double() - b).abs().max()) for a, b in zip(h32, h64)) / max(float(b.abs().max()) for b in h64)
    out["tiny_input"] = x.numpy()
    for i, (a, b) in enumerate(zip(h32, h64)):
        out[f"tiny_heads_{i}"], out[f"tiny_heads64_{i}"] = a.numpy(), b.numpy()
    out["tiny_decoded"] = dec.numpy().copy()
    nms = rm.non_max_suppression(dec.clone(), 0.5, 0.4)[0]
    out["tiny_nms"] = nms.numpy()
    out["ref_fp32_error"] = np.float64(err)
    print("tiny: nms rows", tuple(nms.shape), "conf>=0.5:", int((dec[0, :, 4] >= 0.5).sum()), "fp32 error", err)


def capture_full(rm, out):
    net = rm.Darknet(os.path.join(ref_shims.REF_SRC, "modules/networks/yolo_v3/config/yolov3.cfg"))
    sd = net.state_dict()
    out["full_state"] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "full.weights")
        net.save_darknet_weights(path)
        out["full_floats"] = np.int64((os.path.getsize(path) - 20) // 4)


def main():
    ref_shims.install()
    rm = ref_shims.import_reference("modules.networks.yolo_v3.models")
    uy = ref_shims.import_reference("utils.utils_yolov3")
    uy.save_image = lambda *a, **k: None                       # writes PNGs through cv2
    torch.Tensor.cuda = lambda self, *a, **k: self             # compute_detection: torch.LongTensor([h, w]).cuda()
    out = {}
    capture_full(rm, out)
    capture_tiny(rm, out)
    capture_planted(rm, uy, out)
    np.savez_compressed(os.path.join(GOLDEN, "detect_reference.npz"), **out)
    print("wrote", os.path.join(GOLDEN, "detect_reference.npz"), os.path.getsize(os.path.join(GOLDEN, "detect_reference.npz")))


if __name__ == "__main__":
    main()
