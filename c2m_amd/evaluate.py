"""The detector metric of the reference's evaluator (src/evaluator/evaluator.py, src/utils/utils_yolov3.py) on the device.

A YOLOv3 detector looks at the last ground-truth frame and the last predicted frame; the object the user moved is searched
for in both; the result is a detection F1 / accuracy and the distance between where the predicted object landed and where the
tracker says it should be.  FID and FVD are not provided (they need Inception / I3D weights and TensorFlow).

Differences from the reference, all documented in DESIGN §4.2f: the detector runs ONCE on the 2B frames instead of once per
object; candidates with equal scores keep their box order; a non-finite head box is removed instead of looping for ever."""
import statistics
import warnings

import numpy as np
import torch

from . import ops, segment
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


def quality_from_sums(sums, channels, data_range, region_names=None):
    """The host arithmetic of frame_quality: sums [B,T,9,4] float64 (n_pixels, sse, n_windows, ssim_sum) -> the result dict."""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    n, sse, nw, ss = sums.unbind(-1)
    L2 = float(data_range) ** 2
    mse_raw = _div(sse, n * channels)
    with_err = sse > 0
    psnr = torch.where(with_err, 10.0 * torch.log10(L2 / torch.where(with_err, mse_raw, torch.ones_like(mse_raw))),
                       torch.where(n > 0, torch.full_like(sse, float("inf")), torch.full_like(sse, _NAN)))
    mse, ssim = mse_raw / L2, _div(ss, nw)
    k = 8 if region_names is None else len(region_names)
    if not 0 <= k <= 8:
        raise ValueError("a region byte has 8 bits")
    return {"mse": mse[..., 0], "psnr": psnr[..., 0], "ssim": ssim[..., 0], "region_mse": mse[..., 1:1 + k],
            "region_psnr": psnr[..., 1:1 + k], "region_ssim": ssim[..., 1:1 + k], "region_pixels": n[..., 1:1 + k]}


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

    @staticmethod
    def _mean(v, dim):
        ok = torch.isfinite(v)
        return _div(torch.where(ok, v, torch.zeros_like(v)).sum(dim), ok.sum(dim).double())

    def result(self):
        names = ("frame",) + self.region_names
        out = {}
        for k in self._KEYS:
            v = torch.cat(self.rows[k], 0) if self.rows[k] else torch.zeros(0, 0, len(names), dtype=torch.float64)
            overall, per_t = self._mean(v, (0, 1)), self._mean(v, 0)                  # [1+R], [T,1+R]
            for i, name in enumerate(names):
                key = k if i == 0 else f"{name}_{k}"
                out[key] = float(overall[i])
                out[key + "_per_frame"] = per_t[:, i].tolist()
                if k == "psnr":
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


class MapScore:
    """Sums of map_quality results over a dataset and the reference's averages of them (cityscapesscripts' PQStat.pq_average /
    average_pq and Panoptic-DeepLab's SemanticEvaluator.evaluate): overall and, where the results had a frame axis [B,T], per
    predicted-frame index.  The per-frame values are added in the order they arrive."""

    def __init__(self, **params):
        p = _map_params("MapScore", params)
        self.num_classes, self.max_pairs = int(p["num_classes"]), int(p["max_pairs"])
        self.things = tuple(sorted(set(int(c) for c in p["thing_list"])))
        self.params = p
        self.per_t = None                                    # None until the first update; [] for results without a frame axis
        self.total = self._zero()
        self.frames = 0

    def _zero(self):
        C = self.num_classes
        return {"tp": np.zeros(C, np.int64), "fp": np.zeros(C, np.int64), "fn": np.zeros(C, np.int64),
                "iou": np.zeros(C, np.float64), "confusion": np.zeros((C + 1, C + 1), np.int64)}

    @staticmethod
    def _add(acc, row):
        for k in acc:
            acc[k] += row[k]                                 # iou: one float64 addition per class and frame, in arrival order

    def update(self, result):
        C = self.num_classes
        host = {k: (result[k].cpu().numpy() if isinstance(result[k], torch.Tensor) else np.asarray(result[k]))
                for k in ("tp", "fp", "fn", "iou", "confusion", "overflow")}
        over = host.pop("overflow").astype(bool)
        if over.any():
            raise ValueError(f"{int(over.sum())} frame(s) had more distinct segment pairs than max_pairs={self.max_pairs}: "
                             f"their counts are incomplete; call map_quality with a larger max_pairs")
        lead = host["tp"].shape[:-1]
        if host["tp"].shape[-1] != C or host["confusion"].shape[-2:] != (C + 1, C + 1) or len(lead) not in (1, 2):
            raise ValueError(f"result of {host['tp'].shape[-1]} classes with leading axes {lead}; the score has {C} classes and "
                             "takes [B,T] or [N] results")
        T = lead[1] if len(lead) == 2 else 0
        if self.per_t is None:
            self.per_t = [self._zero() for _ in range(T)]
        if len(self.per_t) != T:
            raise ValueError("results with different numbers of predicted frames")
        rows = {k: v.reshape((-1,) + v.shape[len(lead):]) for k, v in host.items()}
        rows["iou"] = rows["iou"].astype(np.float64)
        for i in range(rows["tp"].shape[0]):
            row = {k: v[i] for k, v in rows.items()}
            self._add(self.total, row)
            if T:
                self._add(self.per_t[i % T], row)
            self.frames += 1

    def _scores(self, acc):
        out = {}
        for name, isthing in _PQ_GROUPS:
            classes = [c for c in range(self.num_classes) if isthing is None or (c in self.things) == isthing]
            out[name], per_class = pq_average(acc["tp"], acc["fp"], acc["fn"], acc["iou"], classes)
            if name == "All":
                out["per_class"] = per_class
        out.update(semantic_scores(acc["confusion"]))
        return out

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
