"""The detector metric of the reference's evaluator (src/evaluator/evaluator.py, src/utils/utils_yolov3.py) on the device.

A YOLOv3 detector looks at the last ground-truth frame and the last predicted frame; the object the user moved is searched
for in both; the result is a detection F1 / accuracy and the distance between where the predicted object landed and where the
tracker says it should be.  FID and FVD are not provided (they need Inception / I3D weights and TensorFlow).

Differences from the reference, all documented in DESIGN §4.2f: the detector runs ONCE on the 2B frames instead of once per
object; candidates with equal scores keep their box order; a non-finite head box is removed instead of looping for ever."""
import ctypes
import math
import statistics
import warnings

import numpy as np
import torch

from . import _lib, ops, segment
from .modules.networks.yolo_v3 import Darknet

_GRAPH_FIELDS = ("target_frames_nodes_roi", "x", "batch")


class Detector:
    """YOLOv3 (or any darknet cfg built from the same blocks) + decode + suppression.  weights: a darknet `.weights` file
    (a missing file raises); None keeps the seeded random init and warns once."""
    _warned = False

    def __init__(self, weights=None, config=None, device="cuda"):
        self.net = Darknet(config)
        if weights is not None:
            self.net.load_darknet_weights(weights)                 # FileNotFoundError / ValueError: never a silent fallback
        elif not Detector._warned:
            Detector._warned = True
            warnings.warn("Detector(weights=None): random-weight detector; pass the path of a darknet weights file "
                          "(yolov3.weights) for a meaningful metric", stacklevel=2)
        self.net.to(device).eval()

    def heads(self, images):
        """images [N,C,S,S], S a multiple of 32, on the device -> the raw head maps [N, A*(5+classes), g, g], coarsest first."""
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[2] != images.shape[3] or \
                images.shape[2] % 32 or images.shape[2] < 32:
            raise ValueError(f"images must be [N,C,S,S] with S a multiple of 32, got "
                             f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__}")
        ops._hip_only(images)
        return self.net(images)

    def detect(self, images=None, conf_thres=0.5, nms_thres=0.4, heads=None, predictions=None, img_size=None):
        """images [N,C,S,S] -> dets [N,cap,7] = (x1, y1, x2, y2, conf, class_conf, class), kept [N] int32, on the device.
        heads= (or predictions=): precomputed raw head maps instead of images; img_size is then the input side they belong to
        (default: 32 x the coarsest grid)."""
        heads = heads if heads is not None else predictions
        if (images is None) == (heads is None):
            raise ValueError("detect() takes images or heads, one of them")
        if heads is None:
            heads, img_size = self.heads(images), images.shape[2]
        elif img_size is None:
            img_size = 32 * min(int(h.shape[-1]) for h in heads)
        cand, score, count = ops.yolo_candidates(list(heads), self.net.anchors, self.net.num_classes, img_size, conf_thres)
        return ops.nms_merge(cand, score, count, nms_thres)


def _graph_inputs(tracking_gnn, index_user_guidance):
    missing = [k for k in _GRAPH_FIELDS if not hasattr(tracking_gnn, k)]
    if missing:
        raise ValueError(f"tracking_gnn lacks {missing}")
    idx = torch.as_tensor(index_user_guidance, dtype=torch.int64).reshape(-1)
    return idx, [getattr(tracking_gnn, k) for k in _GRAPH_FIELDS]


def trajectory_metric(detector, video, generated, tracking_gnn, index_user_guidance, predictions=None, conf_thres=0.5,
                      nms_thres=0.4):
    """utils_yolov3.compute_detection.  video / generated [B,3,T,H,W] (their last frames are read), tracking_gnn and
    index_user_guidance as the model's inference returns them.  predictions: raw head maps for the 2B frames (ground truth
    first) instead of running the network.  Returns a dict with the reference's four lists (mse_batch, mse_normalized_batch,
    gt_detected_images, pred_detected_images) and the per-object tensors (skipped, gt_found, pred_found, gt_box, pred_box, mse,
    mse_normalized) on the host."""
    for name, t in (("video", video), ("generated", generated)):
        if not isinstance(t, torch.Tensor) or t.dim() != 5:
            raise ValueError(f"{name} must be [B,C,T,H,W]")
        ops._hip_only(t, name=name, where=True)
    if video.shape[0] != generated.shape[0] or video.shape[1] != generated.shape[1] or video.shape[3:] != generated.shape[3:]:
        raise ValueError(f"video {tuple(video.shape)} and generated {tuple(generated.shape)} differ in batch, channels or size")
    B = video.shape[0]
    idx, (roi, x, batch) = _graph_inputs(tracking_gnn, index_user_guidance)
    if roi.dim() != 3 or x.dim() != 3 or batch.dim() != 1 or roi.shape[-1] != 4:
        raise ValueError("tracking_gnn: target_frames_nodes_roi [nodes,T,4], x [nodes,t_in,F], batch [nodes] expected")
    empty = {"mse_batch": [], "mse_normalized_batch": [], "gt_detected_images": [], "pred_detected_images": []}
    M = idx.numel()
    if M == 0 or B == 0:
        z = torch.zeros(0, dtype=torch.int32)
        return dict(empty, skipped=z.bool(), gt_found=z.bool(), pred_found=z.bool(), gt_box=z.view(0, 4), pred_box=z.view(0, 4),
                    mse=z.double(), mse_normalized=z.double())
    dev = video.device
    if predictions is None:
        gt, scale, size = ops.detect_input(video.float())
        pr, _, _ = ops.detect_input(generated.float())
        dets, kept = detector.detect(torch.cat([gt, pr], 0), conf_thres, nms_thres)
    else:
        W = video.shape[-1]
        scale = ops.detect_scale(W)
        size = (video.shape[-2] * scale, W * scale)
        if any(h.shape[0] != 2 * B for h in predictions):
            raise ValueError(f"predictions must hold {2 * B} images (ground truth first, then predicted)")
        dets, kept = detector.detect(heads=predictions, conf_thres=conf_thres, nms_thres=nms_thres, img_size=ops.DETECT_SIZE)
    flags, boxes, err = ops.match_detections(dets, kept, idx.to(dev), roi.to(dev, torch.float32), x.to(dev, torch.float32),
                                             batch.to(dev, torch.int64), scale, size)
    packed = torch.cat([flags.double(), boxes.double(), err], 1).cpu()          # the one copy to the host
    flags, boxes, err = packed[:, :3].to(torch.int32), packed[:, 3:11].to(torch.int32), packed[:, 11:]
    if bool((flags[:, 0] < 0).any()):
        raise IndexError("index_user_guidance or tracking_gnn.batch points outside the graph / the batch")
    gt_found, pred_found = flags[:, 1] == 1, flags[:, 2] == 1
    return {"mse_batch": err[pred_found, 0].tolist(), "mse_normalized_batch": err[pred_found, 1].tolist(),
            "gt_detected_images": [1] * int(gt_found.sum()), "pred_detected_images": [1] * int(pred_found.sum()),
            "skipped": flags[:, 0] == 1, "gt_found": gt_found, "pred_found": pred_found, "gt_box": boxes[:, :4],
            "pred_box": boxes[:, 4:], "mse": err[:, 0], "mse_normalized": err[:, 1]}


def binary_f1(y_true, y_pred):
    """sklearn.metrics.f1_score for 0/1 lists (positive label 1; 0 when there is no true or predicted positive)."""
    tp = sum(1 for t, p in zip(y_true, y_pred) if t == 1 and p == 1)
    fp = sum(1 for t, p in zip(y_true, y_pred) if t != 1 and p == 1)
    fn = sum(1 for t, p in zip(y_true, y_pred) if t == 1 and p != 1)
    return 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0


def accuracy(y_true, y_pred):
    """sklearn.metrics.accuracy_score."""
    if len(y_true) != len(y_pred):
        raise ValueError("lists of different length")
    return sum(1 for t, p in zip(y_true, y_pred) if t == p) / len(y_true) if y_true else float("nan")


class DetectionScore:
    """Evaluator.compute_detection / generate_metrics / write_metrics, the detector lines."""

    def __init__(self):
        self.mse, self.mse_normalized, self.gt_detected, self.pred_detected = [], [], [], []

    def update(self, result=None, **lists):
        r = result if result is not None else lists
        self.mse.extend(r["mse_batch"])
        self.mse_normalized.extend(r["mse_normalized_batch"])
        self.gt_detected.extend(r["gt_detected_images"])
        self.pred_detected.extend(r["pred_detected_images"])

    def result(self):
        pred = self.pred_detected + [0] * (len(self.gt_detected) - len(self.pred_detected))
        mean = lambda v: statistics.mean(v) if v else float("nan")      # (the reference raises on an empty list)
        return {"f1": binary_f1(self.gt_detected, pred), "accuracy": accuracy(self.gt_detected, pred),
                "mse_traj": mean(self.mse), "mse_normalized_traj": mean(self.mse_normalized),
                "gt_detection": sum(self.gt_detected), "pred_detection": sum(pred)}

    def write(self, path):
        r = self.result()
        with open(path, "a") as f:
            f.write(f"f1 score {r['f1']}\n")
            f.write(f"accuracy score {r['accuracy']} gt_detection {r['gt_detection']} pred_detection{r['pred_detection']}\n")
            f.write(f"mse_traj_loss {r['mse_traj']}\n")
            f.write(f"mse_normalized_traj_loss {r['mse_normalized_traj']}\n\n\n")
        return r


# ------------------------------------------------------------------------------------------ frame quality: PSNR and SSIM
# What video-prediction work reports next to FID / FVD and what needs no weights: per-frame PSNR and SSIM against the real
# future frames, for the whole frame and per region.
QUALITY_REGIONS = ("foreground", "background", "guided", "disoccluded")
_NAN = float("nan")


def quality_regions(fg_mask, instance_mask, clicked_ids=None, occlusion=None, occ_threshold=0.5):
    """The region bytes of frame_quality for the scored frames -> uint8 [B,T,H,W] on the inputs' device.
    bit 0 foreground: any channel of fg_mask [B,9,T,H,W] (ground truth of the scored frames) is set; bit 1 background: the
    rest; bit 2 guided: instance_mask [B,1,T,H,W] (or [B,T,H,W]) holds one of clicked_ids[b] (a list of ids per sample);
    bit 3 disoccluded: occlusion [B,1,T,H,W] (the model's occlusion_bw) is below occ_threshold."""
    if not isinstance(fg_mask, torch.Tensor) or fg_mask.dim() != 5:
        raise ValueError("fg_mask must be [B,C,T,H,W]")
    B, _, T, H, W = fg_mask.shape
    inst = instance_mask[:, 0] if instance_mask.dim() == 5 else instance_mask
    if tuple(inst.shape) != (B, T, H, W):
        raise ValueError(f"instance_mask must be {(B, 1, T, H, W)} or {(B, T, H, W)}, got {tuple(instance_mask.shape)}")
    fg = (fg_mask != 0).any(1)
    bits = fg.to(torch.uint8) + (~fg).to(torch.uint8) * 2
    if clicked_ids is not None:
        if len(clicked_ids) != B:
            raise ValueError(f"clicked_ids must hold one list of ids per sample ({B}), got {len(clicked_ids)}")
        for b, ids in enumerate(clicked_ids):
            ids = torch.as_tensor(ids).reshape(-1).tolist()
            if ids:
                pick = torch.isin(inst[b], torch.tensor(ids, dtype=inst.dtype, device=inst.device))
                bits[b] += pick.to(torch.uint8) * 4
    if occlusion is not None:
        if tuple(occlusion.shape) != (B, 1, T, H, W):
            raise ValueError(f"occlusion must be {(B, 1, T, H, W)}, got {tuple(occlusion.shape)}")
        bits += (occlusion[:, 0] < occ_threshold).to(torch.uint8) * 8
    return bits.contiguous()


def _div(a, b):
    """a / b, NaN where b is 0."""
    return torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), torch.full_like(a, _NAN))


def _region_count(region_names):
    k = 8 if region_names is None else len(region_names)
    if not 0 <= k <= 8:
        raise ValueError("a region byte has 8 bits")
    return k


def _split_rows(values, k):
    """{key: [..., 9]} -> {key: the frame's [...], "region_" + key: [..., k]}."""
    out = {}
    for key, v in values.items():
        out[key] = v[..., 0]
        out["region_" + key] = v[..., 1:1 + k]
    return out


def _mean(v, dim):
    """Mean over `dim` of the finite entries, NaN where there is none."""
    ok = torch.isfinite(v)
    return _div(torch.where(ok, v, torch.zeros_like(v)).sum(dim), ok.sum(dim).double())


def _row_keys(k, names):
    """The result keys of quantity k, one per row: k for the frame, <region>_k for the regions."""
    return [k if i == 0 else f"{name}_{k}" for i, name in enumerate(names)]


def _put_rows(out, k, names, overall, per_t, suffix=""):
    """out[<key><suffix>] and out[<key><suffix>_per_frame] for every row key of k, from overall [1+R] and per_t [T,1+R]."""
    for i, key in enumerate(_row_keys(k, names)):
        out[key + suffix] = float(overall[i])
        out[key + suffix + "_per_frame"] = per_t[:, i].tolist()


def quality_from_sums(sums, channels, data_range, region_names=None):
    """The host arithmetic of frame_quality: sums [B,T,9,4] float64 (n_pixels, sse, n_windows, ssim_sum) -> the result dict."""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    n, sse, nw, ss = sums.unbind(-1)
    L2 = float(data_range) ** 2
    mse_raw = _div(sse, n * channels)
    with_err = sse > 0
    psnr = torch.where(with_err, 10.0 * torch.log10(L2 / torch.where(with_err, mse_raw, torch.ones_like(mse_raw))),
                       torch.where(n > 0, torch.full_like(sse, float("inf")), torch.full_like(sse, _NAN)))
    k = _region_count(region_names)
    return dict(_split_rows({"mse": mse_raw / L2, "psnr": psnr, "ssim": _div(ss, nw)}, k), region_pixels=n[..., 1:1 + k])


def frame_quality(pred, target, regions=None, region_names=None):
    """PSNR and SSIM of every predicted frame against the real one (ops.frame_quality), on the host after one copy.
    pred / target: float [B,C,T,H,W] in [0,1] (out["generated"] against video[:, :, t_in:]) or uint8 [B,T,H,W,C]
    (fullres.upscale's frames against the dataset's); regions: quality_regions(...) or None.
    Returns float64 tensors: mse (in units of L^2, so both forms agree), psnr (inf for identical frames), ssim [B,T];
    region_mse, region_psnr, region_ssim, region_pixels [B,T,8] (or len(region_names)).  NaN where a region is empty (ssim:
    where it holds no window centre)."""
    sums = ops.frame_quality(pred, target, regions).cpu()                          # the one copy to the host
    u8 = pred.dtype == torch.uint8
    return quality_from_sums(sums, pred.shape[-1] if u8 else pred.shape[1], 255.0 if u8 else 1.0, region_names)


class QualityScore:
    """Means of frame_quality results over a dataset: overall and per predicted-frame index, whole frame and per region.
    NaN entries (empty regions) are left out of their mean; inf PSNR entries (identical frames) are counted in
    psnr_identical and not averaged."""
    _KEYS = ("mse", "psnr", "ssim")

    def __init__(self, region_names=QUALITY_REGIONS):
        self.region_names = tuple(region_names)
        self.rows = {k: [] for k in self._KEYS}              # each entry [B,T,1+R]: the frame, then the regions

    def update(self, result):
        R = len(self.region_names)
        for k in self._KEYS:
            whole, reg = torch.as_tensor(result[k], dtype=torch.float64), torch.as_tensor(result["region_" + k], dtype=torch.float64)
            if reg.shape[-1] < R:
                raise ValueError(f"result holds {reg.shape[-1]} regions, the score has {R}")
            row = torch.cat([whole.unsqueeze(-1), reg[..., :R]], -1)
            if self.rows[k] and row.shape[1] != self.rows[k][0].shape[1]:
                raise ValueError("results with different numbers of predicted frames")
            self.rows[k].append(row)

    def result(self):
        names = ("frame",) + self.region_names
        out = {}
        for k in self._KEYS:
            v = torch.cat(self.rows[k], 0) if self.rows[k] else torch.zeros(0, 0, len(names), dtype=torch.float64)
            _put_rows(out, k, names, _mean(v, (0, 1)), _mean(v, 0))                   # [1+R], [T,1+R]
            if k == "psnr":
                for i, key in enumerate(_row_keys(k, names)):
                    out[key.replace("psnr", "psnr_identical")] = int(torch.isinf(v[..., i]).sum())
        out["frames"] = int(sum(r.shape[0] * r.shape[1] for r in self.rows["mse"]))
        return out

    def write(self, path):
        r = self.result()
        with open(path, "a") as f:
            f.write(f"frames {r['frames']}\n")
            for name in ("",) + tuple(n + "_" for n in self.region_names):
                f.write(f"{name}psnr {r[name + 'psnr']} {name}psnr_identical {r[name + 'psnr_identical']}\n")
                f.write(f"{name}ssim {r[name + 'ssim']}\n")
                f.write(f"{name}mse {r[name + 'mse']}\n")
                for k in self._KEYS:
                    f.write(f"{name}{k}_per_frame {' '.join(str(v) for v in r[name + k + '_per_frame'])}\n")
            f.write("\n\n")
        return r


# ------------------------------------------------------------------------------------------ map quality: mIoU and panoptic quality
# What future-segmentation work reports and what needs no weights either: the label maps a prediction carries forward (or the
# segmenter's maps of predicted frames) against the maps of the real future frames.
MAP_QUALITY = dict(num_classes=19, thing_list=segment.CITYSCAPES["thing_list"], label_divisor=segment.CITYSCAPES["label_divisor"],
                   ignore_label=segment.CITYSCAPES["ignore_label"], max_pairs=65536)
_PQ_GROUPS = (("All", None), ("Things", True), ("Stuff", False))


def _map_params(who, params):
    unknown = set(params) - set(MAP_QUALITY)
    if unknown:
        raise TypeError(f"{who} got unknown parameter(s) {sorted(unknown)}; known: {sorted(MAP_QUALITY)}")
    return {**MAP_QUALITY, **params}


def map_quality(pred_maps, gt_maps, **params):
    """Panoptic-quality counts and the confusion matrix of every predicted map against the real one (ops.map_quality), on the
    device, per frame.  pred_maps / gt_maps: int32 or uint8 [B,T,H,W], [B,1,T,H,W] or [N,H,W], of one dtype and, the channel
    axis of the 5-D form aside, one shape (a rollout's [B,1,T,H,W] maps are scored against clip_maps' [B,T,H,W] as they are): the
    instance-id image (things class * label_divisor + k, stuff the class, void ignore_label: r["instance_mask"] of a rollout,
    segment.clip_maps), the `panoptic` map of segment.panoptic_maps (void ignore_label * label_divisor) or a plain label map.
    Keyword parameters default to MAP_QUALITY: num_classes, thing_list, label_divisor, ignore_label (segment.CITYSCAPES) and
    max_pairs, the slots of a frame's pair table (a power of two).
    Returns a dict of device tensors with the leading axes [...] of the input ([B,T] or [N]): tp, fp, fn int32 [...,C]; iou
    float64 [...,C], the sum of the matched IoUs; confusion int64 [...,C+1,C+1] ([pred, gt], void last); overflow bool [...]:
    the frame had more distinct segment pairs than max_pairs and its counts are incomplete (MapScore.update refuses it)."""
    p = _map_params("map_quality", params)
    for name, t in (("pred_maps", pred_maps), ("gt_maps", gt_maps)):
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4, 5) or (t.dim() == 5 and t.shape[1] != 1):
            raise ValueError(f"{name} must be [B,T,H,W], [B,1,T,H,W] or [N,H,W], got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    pred, gt = (t[:, 0] if t.dim() == 5 else t for t in (pred_maps, gt_maps))      # [B,1,T,H,W] and [B,T,H,W] are one clip
    if pred.shape != gt.shape:
        raise ValueError(f"pred_maps {tuple(pred_maps.shape)} and gt_maps {tuple(gt_maps.shape)} differ in shape")
    lead = tuple(pred.shape[:-2])
    H, W = pred.shape[-2:]
    m = ops.map_quality(pred.reshape(-1, H, W).contiguous(), gt.reshape(-1, H, W).contiguous(), **p)
    return {k: v.view(*lead, *v.shape[1:]) for k, v in m.items()}


def pq_average(tp, fp, fn, iou, classes):
    """PQStat.pq_average over `classes`: ({"pq", "sq", "rq", "n"}, {class: {"pq", "sq", "rq"}}).  Classes with tp + fp + fn == 0
    do not count.  With no counted class the reference divides by zero; here the averages are 0.0 and n is 0."""
    pq = sq = rq = n = 0
    per_class = {}
    for c in classes:
        t, p, f, i = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        if t + p + f == 0:
            per_class[c] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
            continue
        n += 1
        pq_c = i / (t + 0.5 * p + 0.5 * f)
        sq_c = i / t if t != 0 else 0
        rq_c = t / (t + 0.5 * p + 0.5 * f)
        per_class[c] = {"pq": pq_c, "sq": sq_c, "rq": rq_c}
        pq += pq_c
        sq += sq_c
        rq += rq_c
    if n == 0:
        return {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}, per_class
    return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class


def semantic_scores(confusion):
    """SemanticEvaluator.evaluate on a [C+1,C+1] confusion matrix ([pred, gt], void last), restated as it is -- the IoU of a
    class is assigned under acc_valid (the class has ground-truth pixels), the mean divides by the classes of iou_valid."""
    conf = np.asarray(confusion, dtype=np.int64)
    C = conf.shape[0] - 1
    acc, iou = np.zeros(C, dtype=np.float64), np.zeros(C, dtype=np.float64)
    tp = conf.diagonal()[:-1].astype(np.float64)
    pos_gt = np.sum(conf[:-1, :-1], axis=0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        class_weights = pos_gt / np.sum(pos_gt)
        pos_pred = np.sum(conf[:-1, :-1], axis=1).astype(np.float64)
        acc_valid = pos_gt > 0
        acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
        iou_valid = (pos_gt + pos_pred) > 0
        union = pos_gt + pos_pred - tp
        iou[acc_valid] = tp[acc_valid] / union[acc_valid]
        macc = np.sum(acc) / np.sum(acc_valid)
        miou = np.sum(iou) / np.sum(iou_valid)
        fiou = np.sum(iou * class_weights)
        pacc = np.sum(tp) / np.sum(pos_gt)
    return {"mIoU": float(100 * miou), "fwIoU": float(100 * fiou), "mACC": float(100 * macc), "pACC": float(100 * pacc)}


def _pq_zero(C, **extra):
    """An empty tally of panoptic-quality counts over C classes, plus the caller's own entries."""
    return {"tp": np.zeros(C, np.int64), "fp": np.zeros(C, np.int64), "fn": np.zeros(C, np.int64),
            "iou": np.zeros(C, np.float64), **extra}


def _pq_host(result, keys, what, max_pairs, call):
    """The entries `keys` of a map_quality / tube_quality result as numpy arrays; refuses one with an overflow flag."""
    host = {k: (result[k].cpu().numpy() if isinstance(result[k], torch.Tensor) else np.asarray(result[k]))
            for k in tuple(keys) + ("overflow",)}
    over = host.pop("overflow").astype(bool)
    if over.any():
        raise ValueError(f"{int(over.sum())} {what} had more distinct segment pairs than max_pairs={max_pairs}: "
                         f"their counts are incomplete; call {call} with a larger max_pairs")
    return host


def _pq_tally(host, keys, lead, tallies_of):
    """Adds host[k] for k in keys, the `lead` leading axes flattened to rows, into every tally of tallies_of(i), one row at a
    time in arrival order (iou: one float64 addition per class and row).  Returns the number of rows."""
    rows = {k: host[k].reshape((-1,) + host[k].shape[lead:]) for k in keys}
    rows["iou"] = rows["iou"].astype(np.float64)
    for i in range(len(rows["tp"])):
        for acc in tallies_of(i):
            for k in keys:
                acc[k] += rows[k][i]
    return len(rows["tp"])


def _pq_scores(acc, num_classes, things):
    """PQStat.pq_average of a tally over All / Things / Stuff, and All's per-class values as "per_class"."""
    out = {}
    for name, isthing in _PQ_GROUPS:
        classes = [c for c in range(num_classes) if isthing is None or (c in things) == isthing]
        out[name], per_class = pq_average(acc["tp"], acc["fp"], acc["fn"], acc["iou"], classes)
        if name == "All":
            out["per_class"] = per_class
    return out


def _pq_params(who, params):
    """(params, num_classes, max_pairs, things) of a MapScore / TubeScore constructor."""
    p = _map_params(who, params)
    return p, int(p["num_classes"]), int(p["max_pairs"]), tuple(sorted(set(int(c) for c in p["thing_list"])))


class MapScore:
    """Sums of map_quality results over a dataset and the reference's averages of them (cityscapesscripts' PQStat.pq_average /
    average_pq and Panoptic-DeepLab's SemanticEvaluator.evaluate): overall and, where the results had a frame axis [B,T], per
    predicted-frame index.  The per-frame values are added in the order they arrive."""

    _KEYS = ("tp", "fp", "fn", "iou", "confusion")

    def __init__(self, **params):
        self.params, self.num_classes, self.max_pairs, self.things = _pq_params("MapScore", params)
        self.per_t = None                                    # None until the first update; [] for results without a frame axis
        self.total = self._zero()
        self.frames = 0

    def _zero(self):
        return _pq_zero(self.num_classes, confusion=np.zeros((self.num_classes + 1,) * 2, np.int64))

    def update(self, result):
        C = self.num_classes
        host = _pq_host(result, self._KEYS, "frame(s)", self.max_pairs, "map_quality")
        lead = host["tp"].shape[:-1]
        if host["tp"].shape[-1] != C or host["confusion"].shape[-2:] != (C + 1, C + 1) or len(lead) not in (1, 2):
            raise ValueError(f"result of {host['tp'].shape[-1]} classes with leading axes {lead}; the score has {C} classes and "
                             "takes [B,T] or [N] results")
        T = lead[1] if len(lead) == 2 else 0
        if self.per_t is None:
            self.per_t = [self._zero() for _ in range(T)]
        if len(self.per_t) != T:
            raise ValueError("results with different numbers of predicted frames")
        self.frames += _pq_tally(host, self._KEYS, len(lead),
                                 lambda i: (self.total, self.per_t[i % T]) if T else (self.total,))

    def _scores(self, acc):
        return dict(_pq_scores(acc, self.num_classes, self.things), **semantic_scores(acc["confusion"]))

    def result(self):
        out = self._scores(self.total)
        out["frames"] = self.frames
        if self.per_t:
            out["per_frame"] = [self._scores(a) for a in self.per_t]
        return out

    def write(self, path):
        r = self.result()
        rows = [("", r)] + [(f"frame{t}_", f) for t, f in enumerate(r.get("per_frame", ()))]
        with open(path, "a") as f:
            f.write(f"frames {r['frames']}\n")
            for prefix, s in rows:
                for name, _ in _PQ_GROUPS:
                    g = s[name]
                    f.write(f"{prefix}{name} pq {g['pq']} sq {g['sq']} rq {g['rq']} n {g['n']}\n")
                for k in ("mIoU", "fwIoU", "mACC", "pACC"):
                    f.write(f"{prefix}{k} {s[k]}\n")
            for c, g in sorted(r["per_class"].items()):
                f.write(f"class {c} pq {g['pq']} sq {g['sq']} rq {g['rq']}\n")
            f.write("\n\n")
        return r


# ------------------------------------------------------------------------------------------ tube quality: video panoptic quality
# Identity over time: PQ in which a segment is a tube, the pixels of one id in k consecutive frames (VPQ, Kim et al., CVPR 2020;
# DESIGN §4.2s).  Two objects of one class that swap ids are true positives in every frame and, from k = 2 on, two false
# positives and two false negatives.
TUBE_WINDOWS = (1, 2, 3, 4)
_TUBE_KEYS = ("tp", "fp", "fn", "iou")


def _tube_windows(windows, T):
    """The `windows` argument -> a tuple of distinct ints in 1..T ("all" is T)."""
    if isinstance(windows, (str, int)) or not hasattr(windows, "__iter__"):
        windows = (windows,)
    ks = []
    for k in windows:
        if isinstance(k, str):
            if k != "all":
                raise ValueError(f"windows holds {k!r}: an entry is an int in 1..T or \"all\"")
            k = T
        elif isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"windows holds {k!r}: an entry is an int in 1..T or \"all\"")
        k = int(k)
        if not 1 <= k <= T:
            raise ValueError(f"a window of {k} frames in clips of {T}: windows must lie in 1..{T}")
        if k in ks:
            raise ValueError(f"windows holds the length {k} twice")
        ks.append(k)
    if not ks:
        raise ValueError("windows is empty")
    return tuple(ks)


def tube_quality(pred_maps, gt_maps, windows=TUBE_WINDOWS, ids=None, **params):
    """Video panoptic quality counts of predicted clips against the real ones (ops.tube_quality), on the device: for every k of
    `windows` and every window of k consecutive frames of a clip, map_quality's counts with a TUBE for a segment -- the pixels
    of the window with one (cat, n), matched by tube IoU > 0.5.  pred_maps / gt_maps: int32 or uint8 [B,T,H,W] or [B,1,T,H,W]
    of one dtype and, the channel axis aside, one shape, with map_quality's encodings; both must be in ONE id space over time
    (a rollout's instance_mask against tracking.anchor_maps of the real frames).  windows: ints in 1..T or "all" (= T), no
    length twice.  ids: None or int32 [B,M] map values on the device (negative: padding), the objects whose own tube IoU is
    wanted.  Keyword parameters as map_quality's (MAP_QUALITY); max_pairs also bounds a window's pair table.
    Returns {k: dict} of device tensors: tp, fp, fn int32 [B,T-k+1,C]; iou float64 [B,T-k+1,C]; overflow bool [B,T-k+1] (a
    frame of the window or the window itself had more distinct segment pairs than max_pairs; TubeScore.update refuses it) and,
    with ids, id_iou float64 [B,T-k+1,M] -- the IoU of the predicted and the real tube of that id, not thresholded; -1.0 for
    padding, a void or crowd id and an object without real pixels in the window -- and id_gt_area, id_pred_area int32."""
    p = _map_params("tube_quality", params)
    for name, t in (("pred_maps", pred_maps), ("gt_maps", gt_maps)):
        if not isinstance(t, torch.Tensor) or t.dim() not in (4, 5) or (t.dim() == 5 and t.shape[1] != 1):
            raise ValueError(f"{name} must be [B,T,H,W] or [B,1,T,H,W], got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    pred, gt = (t[:, 0] if t.dim() == 5 else t for t in (pred_maps, gt_maps))
    if pred.shape != gt.shape:
        raise ValueError(f"pred_maps {tuple(pred_maps.shape)} and gt_maps {tuple(gt_maps.shape)} differ in shape")
    if pred.shape[1] < 1:
        raise ValueError("clips without a frame")
    ks = _tube_windows(windows, int(pred.shape[1]))
    return ops.tube_quality(pred.contiguous(), gt.contiguous(), ks, ids, **p)


class TubeScore:
    """Sums of tube_quality results over a dataset and video panoptic quality from them, as Cityscapes-VPS aggregates it: per
    window length k the counts of all windows of all updates are added and PQStat.pq_average gives PQ / SQ / RQ over All /
    Things / Stuff; `vpq` is the mean over k of the per-k PQ.  With ids, the mean id_iou over the entries >= 0 per k."""

    def __init__(self, **params):
        self.params, self.num_classes, self.max_pairs, self.things = _pq_params("TubeScore", params)
        self.total = None                                    # {k: sums}, fixed by the first update
        self.windows = 0

    def update(self, result):
        C = self.num_classes
        if not isinstance(result, dict) or not result or not all(isinstance(k, (int, np.integer)) for k in result):
            raise ValueError("a tube_quality result is a dict {k: {...}} with one entry per window length")
        if self.total is not None and set(self.total) != set(int(k) for k in result):
            raise ValueError(f"results with different window lengths: {sorted(self.total)} and {sorted(result)}")
        host = {}
        for k, r in result.items():
            h = _pq_host(r, _TUBE_KEYS + (("id_iou",) if "id_iou" in r else ()), f"window(s) of {int(k)} frame(s)",
                         self.max_pairs, "tube_quality")
            if h["tp"].ndim != 3 or h["tp"].shape[-1] != C:
                raise ValueError(f"result of shape {h['tp'].shape} for k={int(k)}; the score has {C} classes and takes [B,T-k+1,C]")
            host[int(k)] = h
        if self.total is None:
            self.total = {k: _pq_zero(C, windows=0, id_sum=0.0, id_n=0) for k in host}
        for k, h in host.items():                            # every k was checked before the first row is added
            acc = self.total[k]
            n = _pq_tally(h, _TUBE_KEYS, 2, lambda i: (acc,))
            acc["windows"] += n
            self.windows += n
            if "id_iou" in h:
                v = h["id_iou"].astype(np.float64).reshape(-1)
                for x in v[v >= 0]:
                    acc["id_sum"] += float(x)
                acc["id_n"] += int((v >= 0).sum())

    def result(self):
        out = {"windows": self.windows, "per_k": {}}
        for k, acc in sorted((self.total or {}).items()):
            s = {"windows": acc["windows"], **_pq_scores(acc, self.num_classes, self.things)}
            s["id_iou"] = acc["id_sum"] / acc["id_n"] if acc["id_n"] else None
            s["id_n"] = acc["id_n"]
            out["per_k"][k] = s
        n = len(out["per_k"])
        for name, _ in _PQ_GROUPS:
            key = "vpq" if name == "All" else f"vpq_{name.lower()}"
            out[key] = sum(s[name]["pq"] for s in out["per_k"].values()) / n if n else 0.0
        return out

    def write(self, path):
        r = self.result()
        with open(path, "a") as f:
            f.write(f"windows {r['windows']}\n")
            f.write(f"vpq {r['vpq']} vpq_things {r['vpq_things']} vpq_stuff {r['vpq_stuff']}\n")
            for k, s in r["per_k"].items():
                for name, _ in _PQ_GROUPS:
                    g = s[name]
                    f.write(f"k{k}_{name} pq {g['pq']} sq {g['sq']} rq {g['rq']} n {g['n']}\n")
                if s["id_iou"] is not None:
                    f.write(f"k{k}_id_iou {s['id_iou']} n {s['id_n']}\n")
            f.write("\n\n")
        return r


# ------------------------------------------------------------------------------------------ flow scores: endpoint error and consistency
# What optical-flow work reports (Sintel's EPE and speed buckets, KITTI's Fl, Barron's angular error) and, for clips without
# ground truth, what the flows say about themselves: the photometric error of the warp and the forward-backward distance
# (csrc/flow_score.hip).  Flows are in pixels, channel 0 = x, a(x) ~ b(x + flow(x)).
FLOW_REGIONS = ("object", "background", "boundary", "occluded", "slow", "medium", "fast")
FLOW_QUALITY_COLUMNS = ("n", "n_nonfinite", "sum_epe", "sum_e2", "sum_mag", "sum_ae", "n_out", "n_gt1", "n_gt3", "n_gt5")
FLOW_CONSISTENCY_COLUMNS = ("n", "n_inside", "sum_photo", "sum_photo2", "sum_fb", "n_incons", "sum_photo_cons")
FLOW_SCORE_ROWS = ops.SCORE_ROWS                # every counted pixel, then region bits 0..7
_FLOW_FLOATS = (torch.float32, torch.bfloat16)


def _flow_operand(name, x, channels, dtypes):
    """Type, dtype, rank and channel checks of one [N,C,H,W] / [B,C,T,H,W] operand -> (B, T, H, W, lead) with lead (N,) or (B, T)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if x.dim() not in (4, 5):
        raise ValueError(f"{name} must be [N,C,H,W] or [B,C,T,H,W], got {tuple(x.shape)}")
    if x.shape[1] not in channels:
        raise ValueError(f"{name} must have {' or '.join(str(c) for c in channels)} channels, got {x.shape[1]} in {tuple(x.shape)}")
    if x.dim() == 4:
        (N, _, H, W), T, lead = x.shape, 1, (x.shape[0],)
    else:
        (N, _, T, H, W), lead = x.shape, (x.shape[0], x.shape[2])
    if H < 1 or W < 1:
        raise ValueError(f"{name} must hold at least one pixel, got {tuple(x.shape)}")
    if H * W >= 2 ** 31:
        raise ValueError(f"one {H}x{W} frame has 2^31 pixels or more")
    return N, T, H, W, lead


def _flow_same(name, x, ref_name, ref):
    if x.dim() != ref.dim() or x.shape[0] != ref.shape[0] or x.shape[2:] != ref.shape[2:]:
        raise ValueError(f"{name} {tuple(x.shape)} and {ref_name} {tuple(ref.shape)} differ in rank, pairs or size")


def _flow_mask(name, m, lead, H, W, like):
    """A uint8 per-pixel operand (valid, regions): lead + (H, W), on the device of `like`."""
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{name} must be a uint8 tensor or None, got {type(m).__name__}")
    if m.dtype != torch.uint8:
        raise TypeError(f"{name} must be uint8, got {m.dtype}")
    if tuple(m.shape) != tuple(lead) + (H, W):
        raise ValueError(f"{name} must be {tuple(lead) + (H, W)}, got {tuple(m.shape)}")
    if m.device != like.device:
        raise ValueError(f"{name} must be on the device of the flows ({like.device}), got {m.device}")
    return m


def _flow_planes(x):
    """x with dense H x W planes and distinct channels (a copy only if they are not) and its (B, C, T) strides in elements.  A
    B- or T-strided or expanded view (flows[:, :, 1:], one frame repeated along T) goes in as it is."""
    x = x.detach()
    H, W = x.shape[-2:]
    dense = (W == 1 or x.stride(-1) == 1) and (H == 1 or x.stride(-2) == W) and (x.shape[1] == 1 or x.stride(1) >= H * W)
    if not dense:
        x = x.contiguous()
    s = x.stride()
    return x, ((s[0], s[1], s[2]) if x.dim() == 5 else (s[0], s[1], 0))


def _same_device(pairs, first):
    for name, t in pairs:
        if t is not None and t.device != first.device:
            raise ValueError(f"{name} must be on the device of the first operand ({first.device}), got {t.device}")


def flow_quality_sums(pred, target, valid=None, regions=None):
    """The error sums of the flow `pred` against `target` (csrc/flow_score.hip): float64 [N,9,10] (or [B,T,9,10]) on the device,
    row 0 the scored pixels, row 1 + k those whose `regions` byte has bit k, columns FLOW_QUALITY_COLUMNS.

    pred fp32 or bf16, target fp32: [N,2,H,W] or [B,2,T,H,W]; B-, T- and channel-strided views go in without a copy.  valid,
    regions: uint8 [N,H,W] / [B,T,H,W] or None.  A pixel is scored when valid != 0 and both target components are finite and
    below 1e9 in magnitude (KITTI's sparse ground truth, Sintel's invalid marker); a scored pixel whose pred is not finite adds
    nothing to the sums and counts in n, n_nonfinite and all four threshold counts.  All arithmetic fp64; two launches, no
    atomics, bit-repeatable, nothing read back, no autograd."""
    B, T, H, W, lead = _flow_operand("pred", pred, (2,), _FLOW_FLOATS)
    _flow_operand("target", target, (2,), (torch.float32,))
    _flow_same("target", target, "pred", pred)
    valid = _flow_mask("valid", valid, lead, H, W, pred)
    regions = _flow_mask("regions", regions, lead, H, W, pred)
    _same_device((("target", target),), pred)
    ops._hip_only(pred, target, valid, regions)
    ops._on_current_device(pred, target, valid, regions)
    pred, sp = _flow_planes(pred)
    target, st = _flow_planes(target)
    valid, regions = (None if m is None else m.contiguous() for m in (valid, regions))
    out = torch.zeros(*lead, FLOW_SCORE_ROWS, len(FLOW_QUALITY_COLUMNS), device=pred.device, dtype=torch.float64)
    if B * T:
        L = _lib.lib()
        nbytes = L.c2m_flow_quality_workspace_bytes(B, T, H, W)
        work = torch.empty(nbytes // 8, device=pred.device, dtype=torch.float64)
        _lib.check(L.c2m_flow_quality(ops._p(pred), ops._p(target), ops._p(valid), ops._p(regions), ops._dt(pred), B, T, H, W,
                                      (ctypes.c_long * 3)(*sp), (ctypes.c_long * 3)(*st), ops._p(work), nbytes, ops._p(out),
                                      ops._stream()), "flow_quality")
    return out


def flow_consistency_sums(flow_ab, a, b, flow_ba=None, regions=None, alpha1=0.01, alpha2=0.5, maps=False):
    """The ground-truth-free check of the flow a -> b (csrc/flow_score.hip): float64 [N,9,7] (or [B,T,9,7]) on the device, row 0
    every pixel of a, row 1 + k those whose `regions` byte has bit k, columns FLOW_CONSISTENCY_COLUMNS.

    flow_ab, flow_ba (the flow b -> a, or None): fp32 [N,2,H,W] or [B,2,T,H,W]; a, b: fp32 or bf16 with 1 or 3 channels, any value
    range, finite; strided views go in without a copy (a frame repeated along T too).  A pixel x is inside when its flow is finite
    and y = x + flow_ab(x) lies in the frame; there b and flow_ba are sampled bilinearly at y in fp64: photo = mean over channels
    of |a(x) - b(y)|, fb = |flow_ab(x) + flow_ba(y)|, and the pixel is inconsistent when fb^2 > alpha1 (|flow_ab(x)|^2 +
    |flow_ba(y)|^2) + alpha2 (UnFlow's occlusion test; a non-finite flow_ba(y) is inconsistent and adds nothing to sum_fb).
    Without flow_ba the last three columns are NaN.
    maps=True: returns (sums, {"photo", "fb": fp32 [N,H,W] / [B,T,H,W], NaN outside; "inconsistent": uint8}), written by the same
    launch.  Two launches, no atomics, bit-repeatable, nothing read back, no autograd."""
    for name, al in (("alpha1", alpha1), ("alpha2", alpha2)):
        if isinstance(al, bool) or not isinstance(al, (int, float)):
            raise TypeError(f"{name} must be a number, got {type(al).__name__}")
        if not math.isfinite(al) or al < 0:
            raise ValueError(f"{name} must be finite and >= 0, got {al}")
    B, T, H, W, lead = _flow_operand("flow_ab", flow_ab, (2,), (torch.float32,))
    _flow_operand("a", a, (1, 3), _FLOW_FLOATS)
    _flow_operand("b", b, (1, 3), _FLOW_FLOATS)
    _flow_same("a", a, "flow_ab", flow_ab)
    _flow_same("b", b, "flow_ab", flow_ab)
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"a has {a.shape[1]} channels and b {b.shape[1]}")
    if flow_ba is not None:
        _flow_operand("flow_ba", flow_ba, (2,), (torch.float32,))
        _flow_same("flow_ba", flow_ba, "flow_ab", flow_ab)
    regions = _flow_mask("regions", regions, lead, H, W, flow_ab)
    _same_device((("a", a), ("b", b), ("flow_ba", flow_ba)), flow_ab)
    ops._hip_only(flow_ab, a, b, flow_ba, regions)
    ops._on_current_device(flow_ab, a, b, flow_ba, regions)
    if a.dtype != b.dtype:                               # fp32 against bf16: bf16 -> fp32 is exact
        a, b = a.float(), b.float()
    C = a.shape[1]
    strides = []
    flow_ab, s = _flow_planes(flow_ab)
    strides += s
    a, s = _flow_planes(a)
    strides += s
    b, s = _flow_planes(b)
    strides += s
    if flow_ba is not None:
        flow_ba, s = _flow_planes(flow_ba)
        strides += s
    else:
        strides += (0, 0, 0)
    regions = None if regions is None else regions.contiguous()
    dev = flow_ab.device
    out = torch.zeros(*lead, FLOW_SCORE_ROWS, len(FLOW_CONSISTENCY_COLUMNS), device=dev, dtype=torch.float64)
    if flow_ba is None:
        out[..., 4:] = _NAN
    m = None
    if maps:
        m = {"photo": torch.full((*lead, H, W), _NAN, device=dev, dtype=torch.float32),
             "fb": torch.full((*lead, H, W), _NAN, device=dev, dtype=torch.float32),
             "inconsistent": torch.zeros(*lead, H, W, device=dev, dtype=torch.uint8)}
    if B * T:
        L = _lib.lib()
        nbytes = L.c2m_flow_consistency_workspace_bytes(B, T, H, W)
        work = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        mp = (None, None, None) if m is None else (ops._p(m["photo"]), ops._p(m["fb"]), ops._p(m["inconsistent"]))
        _lib.check(L.c2m_flow_consistency(ops._p(flow_ab), ops._p(a), ops._p(b), ops._p(flow_ba), ops._p(regions), ops._dt(a),
                                          B, C, T, H, W, (ctypes.c_long * 12)(*strides), float(alpha1), float(alpha2), *mp,
                                          ops._p(work), nbytes, ops._p(out), ops._stream()), "flow_consistency")
    return (out, m) if maps else out


def flow_quality_from_sums(sums, region_names=None):
    """The host arithmetic of flow_quality: sums [...,9,10] float64 (FLOW_QUALITY_COLUMNS) -> the result dict.  The means of the
    error sums are over the scored pixels with a finite pred (n - n_nonfinite), the rates over all scored pixels (n)."""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    if sums.dim() < 2 or tuple(sums.shape[-2:]) != (FLOW_SCORE_ROWS, len(FLOW_QUALITY_COLUMNS)):
        raise ValueError(f"sums must be [...,{FLOW_SCORE_ROWS},{len(FLOW_QUALITY_COLUMNS)}], got {tuple(sums.shape)}")
    n, bad, s_epe, s_e2, s_mag, s_ae, n_out, g1, g3, g5 = sums.unbind(-1)
    fin = n - bad
    v = {"epe": _div(s_epe, fin), "rmse": torch.sqrt(_div(s_e2, fin)), "ae_deg": _div(s_ae, fin) * (180.0 / math.pi),
         "magnitude": _div(s_mag, fin), "fl": _div(n_out, n), "bad1": _div(g1, n), "bad3": _div(g3, n), "bad5": _div(g5, n),
         "nonfinite": bad, "pixels": n}
    return _split_rows(v, _region_count(region_names))


def flow_consistency_from_sums(sums, region_names=None):
    """The host arithmetic of flow_consistency: sums [...,9,7] float64 (FLOW_CONSISTENCY_COLUMNS) -> the result dict: photo,
    photo_rms and fb are means over the inside pixels, photo_consistent over the inside pixels that pass the forward-backward
    test, inconsistent the share of the inside pixels that fail it, outside the share of all pixels whose target leaves the frame."""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    if sums.dim() < 2 or tuple(sums.shape[-2:]) != (FLOW_SCORE_ROWS, len(FLOW_CONSISTENCY_COLUMNS)):
        raise ValueError(f"sums must be [...,{FLOW_SCORE_ROWS},{len(FLOW_CONSISTENCY_COLUMNS)}], got {tuple(sums.shape)}")
    n, n_in, s_p, s_p2, s_fb, n_inc, s_pc = sums.unbind(-1)
    v = {"photo": _div(s_p, n_in), "photo_rms": torch.sqrt(_div(s_p2, n_in)), "photo_consistent": _div(s_pc, n_in - n_inc),
         "fb": _div(s_fb, n_in), "inconsistent": _div(n_inc, n_in), "outside": _div(n - n_in, n), "pixels": n}
    return _split_rows(v, _region_count(region_names))


def flow_quality(pred, target, valid=None, regions=None, region_names=None):
    """Endpoint error, angular error and outlier rates of the flow `pred` against `target` (flow_quality_sums), on the host after
    one copy.  Returns float64 tensors [N] (or [B,T]): epe (px), rmse (px), ae_deg (Barron's angular error, degrees), magnitude
    (mean |target|), fl (KITTI: error > 3 px and > 5 % of |target|), bad1, bad3, bad5 (error > 1, 3, 5 px), nonfinite, pixels;
    region_* [...,8] (or len(region_names)); "sums", the raw sums (what FlowScore.update takes).  NaN where a region holds no
    scored pixel."""
    sums = flow_quality_sums(pred, target, valid, regions).cpu()                   # the one copy to the host
    return dict(flow_quality_from_sums(sums, region_names), sums=sums)


def flow_consistency(flow_ab, a, b, flow_ba=None, regions=None, region_names=None, alpha1=0.01, alpha2=0.5, maps=False):
    """The ground-truth-free score of the flow a -> b (flow_consistency_sums), on the host after one copy.  Returns float64
    tensors [N] (or [B,T]): photo, photo_rms, photo_consistent, fb (px), inconsistent, outside, pixels; region_*; "sums"; with
    maps=True also the device maps photo_map, fb_map (fp32, NaN outside) and inconsistent_map (uint8).  fb, inconsistent and
    photo_consistent are NaN without flow_ba.
    What it cannot see: a textureless region has a low photometric error for any flow, and the forward-backward test flags a
    disocclusion as an error by design."""
    r = flow_consistency_sums(flow_ab, a, b, flow_ba, regions, alpha1, alpha2, maps)
    sums = (r[0] if maps else r).cpu()                                              # the one copy to the host
    out = dict(flow_consistency_from_sums(sums, region_names), sums=sums)
    if maps:
        out.update({k + "_map": v for k, v in r[1].items()})
    return out


def flow_regions(target, instance=None, occlusion=None, occ_threshold=0.5, band=4, jump=1.0, speeds=(10.0, 40.0),
                 id_range=(1000, 19000)):
    """The region bytes of flow_quality / flow_consistency for target flows [N,2,H,W] or [B,2,T,H,W] -> uint8 [N,H,W] / [B,T,H,W]
    on the target's device, bits in the order of FLOW_REGIONS:
    object: `instance` ([N,H,W] / [B,T,H,W], or with a channel axis of 1) holds an id with id_range[0] <= id < id_range[1];
    background: every other pixel (all of them without `instance`);
    boundary: within `band` px (Chebyshev) of a pixel whose target flow differs from a 4-neighbour's by more than `jump` px or,
    with `instance`, whose id differs from a 4-neighbour's;
    occluded: `occlusion` (same shapes) is below occ_threshold;
    slow / medium / fast: |target| < speeds[0], < speeds[1], >= speeds[1] (Sintel's s0-10, s10-40, s40+), decided on squares in
    float64.  Plain torch on the device."""
    if not isinstance(target, torch.Tensor) or target.dim() not in (4, 5) or target.shape[1] != 2:
        raise ValueError("target must be [N,2,H,W] or [B,2,T,H,W]")
    if not isinstance(band, int) or isinstance(band, bool) or band < 0:
        raise ValueError(f"band must be an int >= 0, got {band!r}")
    s0, s1 = (float(s) for s in speeds)
    if not (0.0 <= s0 <= s1 and math.isfinite(s1)) or not (math.isfinite(jump) and jump >= 0):
        raise ValueError(f"speeds must be two finite, ordered, non-negative values and jump finite and >= 0, got {speeds}, {jump}")
    lo, hi = (int(v) for v in id_range)
    t = target.detach().double()
    u, v = t[:, 0], t[:, 1]                                                        # [N,H,W] or [B,T,H,W]
    lead, (H, W) = tuple(u.shape[:-2]), u.shape[-2:]

    def plane(name, x):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        if x.dim() == u.dim() + 1 and x.shape[1] == 1:
            x = x[:, 0]
        if tuple(x.shape) != tuple(u.shape):
            raise ValueError(f"{name} must be {tuple(u.shape)} (or with a channel axis of 1), got {tuple(x.shape)}")
        if x.device != target.device:
            raise ValueError(f"{name} must be on the device of target ({target.device}), got {x.device}")
        return x

    def neighbours(differs):
        """differs(p, q) on the two slices of each 4-neighbour pair -> the pixels on either side of a differing pair."""
        e = torch.zeros(u.shape, dtype=torch.bool, device=u.device)
        dx = differs(lambda x: x[..., :, 1:], lambda x: x[..., :, :-1])
        e[..., :, 1:] |= dx
        e[..., :, :-1] |= dx
        dy = differs(lambda x: x[..., 1:, :], lambda x: x[..., :-1, :])
        e[..., 1:, :] |= dy
        e[..., :-1, :] |= dy
        return e

    edge = neighbours(lambda p, q: (p(u) - q(u)) * (p(u) - q(u)) + (p(v) - q(v)) * (p(v) - q(v)) > float(jump) * float(jump))
    bits = torch.zeros(u.shape, dtype=torch.uint8, device=u.device)
    if instance is not None:
        inst = plane("instance", instance)
        obj = (inst >= lo) & (inst < hi)
        edge |= neighbours(lambda p, q: p(inst) != q(inst))
    else:
        obj = torch.zeros(u.shape, dtype=torch.bool, device=u.device)
    bits += obj.to(torch.uint8) + (~obj).to(torch.uint8) * 2
    if band > 0:
        e = edge.reshape(-1, 1, H, W).to(torch.float32)
        edge = (torch.nn.functional.max_pool2d(e, 2 * band + 1, 1, band) > 0).reshape(u.shape)
    bits += edge.to(torch.uint8) * 4
    if occlusion is not None:
        bits += (plane("occlusion", occlusion) < occ_threshold).to(torch.uint8) * 8
    m2 = u * u + v * v
    bits += (m2 < s0 * s0).to(torch.uint8) * 16 + ((m2 >= s0 * s0) & (m2 < s1 * s1)).to(torch.uint8) * 32 + \
        (m2 >= s1 * s1).to(torch.uint8) * 64
    return bits.contiguous()


class FlowScore:
    """Flow scores over a dataset, shaped like QualityScore.  kind "quality" takes flow_quality results (or their raw sums),
    kind "consistency" flow_consistency results.  Every quantity is reported twice: `<key>` is the pixel-weighted figure over
    everything seen -- the sums of all pairs added, then the host arithmetic: Sintel's EPE, KITTI's Fl-all -- and `<key>_mean`
    the mean over pairs of the per-pair values (NaN entries, pairs with an empty region, left out); both overall and, as
    `_per_frame` lists, per frame index, for the whole frame and as `<region>_<key>` per region.  Sums with an [N] lead count as
    one frame index."""
    _KINDS = {"quality": (FLOW_QUALITY_COLUMNS, flow_quality_from_sums,
                          ("epe", "rmse", "ae_deg", "fl", "bad1", "bad3", "bad5", "nonfinite", "pixels")),
              "consistency": (FLOW_CONSISTENCY_COLUMNS, flow_consistency_from_sums,
                              ("photo", "photo_consistent", "fb", "inconsistent", "outside", "pixels"))}

    def __init__(self, kind="quality", region_names=FLOW_REGIONS):
        if kind not in self._KINDS:
            raise ValueError(f"kind must be one of {sorted(self._KINDS)}, got {kind!r}")
        self.kind, self.region_names = kind, tuple(region_names)
        _region_count(self.region_names)
        self.columns, self.from_sums, self.keys = self._KINDS[kind]
        self.rows = []                                   # each entry [B,T,9,K]

    def update(self, result):
        sums = result["sums"] if isinstance(result, dict) else result
        sums = torch.as_tensor(sums.cpu() if isinstance(sums, torch.Tensor) else sums, dtype=torch.float64)
        if sums.dim() not in (3, 4) or tuple(sums.shape[-2:]) != (FLOW_SCORE_ROWS, len(self.columns)):
            raise ValueError(f"a {self.kind} score takes sums [N,{FLOW_SCORE_ROWS},{len(self.columns)}] or [B,T,..], got "
                             f"{tuple(sums.shape)}")
        if sums.dim() == 3:
            sums = sums.unsqueeze(1)
        if self.rows and sums.shape[1] != self.rows[0].shape[1]:
            raise ValueError("results with different numbers of frames")
        self.rows.append(sums)

    def _flat(self, sums):
        """from_sums -> {key: [..., 1 + R]}: the frame, then the regions."""
        r = self.from_sums(sums, self.region_names)
        return {k: torch.cat([r[k].unsqueeze(-1), r["region_" + k]], -1) for k in self.keys}

    def result(self):
        names = ("frame",) + self.region_names
        K = len(self.columns)
        v = torch.cat(self.rows, 0) if self.rows else torch.zeros(0, 0, FLOW_SCORE_ROWS, K, dtype=torch.float64)
        pooled, pooled_t, each = self._flat(v.sum((0, 1))), self._flat(v.sum(0)), self._flat(v)
        out = {}
        for k in self.keys:
            _put_rows(out, k, names, pooled[k], pooled_t[k])
            _put_rows(out, k, names, _mean(each[k], (0, 1)), _mean(each[k], 0), "_mean")
        out["pairs"] = int(v.shape[0] * v.shape[1])
        return out

    def write(self, path):
        r = self.result()
        with open(path, "a") as f:
            f.write(f"{self.kind} pairs {r['pairs']}\n")
            for name in ("",) + tuple(n + "_" for n in self.region_names):
                for k in self.keys:
                    f.write(f"{name}{k} {r[name + k]} {name}{k}_mean {r[name + k + '_mean']}\n")
                    f.write(f"{name}{k}_per_frame {' '.join(str(x) for x in r[name + k + '_per_frame'])}\n")
                    f.write(f"{name}{k}_mean_per_frame {' '.join(str(x) for x in r[name + k + '_mean_per_frame'])}\n")
            f.write("\n\n")
        return r


def clip_flow_check(video, flows, num_input_frames, regions=None, region_names=None, alpha1=0.01, alpha2=0.5, maps=False):
    """Scores what train.compute_flow returned for a batch, without ground truth: video [B,C,T,H,W] (fp32 or bf16, C 1 or 3),
    flows the dict of compute_flow, num_input_frames = t_in.  Returns {"target_bw": ..., "target_fw": ..., "input": ...}, each
    a flow_consistency result with [B, frames] entries, for the entries the dict holds:
    target_bw_of[:, :, i]: a = frame t_in + i, b = frame t_in - 1, with target_fw_of as the reverse flow when it is there;
    target_fw_of[:, :, i]: a = frame t_in - 1, b = frame t_in + i, with target_bw_of as the reverse flow;
    input_of[:, :, i]: a = frame i, b = frame i + 1; no reverse flow is in the dict, so its forward-backward figures are NaN.
    The photometric figures are always given.  regions: None or a dict with the same keys of uint8 [B,frames,H,W] region bytes.
    No frame is copied: the pairs are strided views of the video.  This is how ClassicFlow() is compared with
    ClassicFlow(seed=True, refine=True, chain=True) on one's own clips: lower photo and fb on the same clip is the better flow.

    For pixel-unit flow targets only (a(x) ~ b(x + flow(x))).  The generator's dense_motion_bw follows ops.flow_warp's grid
    convention: score it with flow_quality against target_bw_of, not with this call."""
    if not isinstance(video, torch.Tensor) or video.dim() != 5:
        raise ValueError("video must be [B,C,T,H,W]")
    if not isinstance(flows, dict) or not isinstance(flows.get("target_bw_of"), torch.Tensor):
        raise ValueError("flows must be the dict of train.compute_flow (it holds target_bw_of)")
    t_in = int(num_input_frames)
    bw, fw, inp = flows["target_bw_of"], flows.get("target_fw_of"), flows.get("input_of")
    if bw.dim() != 5:
        raise ValueError(f"target_bw_of must be [B,2,T,H,W], got {tuple(bw.shape)}")
    t_out = bw.shape[2]
    if t_in < 1 or video.shape[2] < t_in + t_out:
        raise ValueError(f"video holds {video.shape[2]} frames; {t_in} input frames and {t_out} flow targets need {t_in + t_out}")
    if regions is not None and not isinstance(regions, dict):
        raise TypeError("regions must be None or a dict with the keys of the result")
    reg = regions or {}
    future = video[:, :, t_in:t_in + t_out]
    last = video[:, :, t_in - 1:t_in].expand(-1, -1, t_out, -1, -1)
    kw = dict(region_names=region_names, alpha1=alpha1, alpha2=alpha2, maps=maps)
    out = {"target_bw": flow_consistency(bw, future, last, fw, reg.get("target_bw"), **kw)}
    if fw is not None:
        out["target_fw"] = flow_consistency(fw, last, future, bw, reg.get("target_fw"), **kw)
    if inp is not None and t_in > 1:
        out["input"] = flow_consistency(inp, video[:, :, :t_in - 1], video[:, :, 1:t_in], None, reg.get("input"), **kw)
    return out
