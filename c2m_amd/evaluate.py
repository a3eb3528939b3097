"""The detector metric of the reference's evaluator (src/evaluator/evaluator.py, src/utils/utils_yolov3.py) on the device.

A YOLOv3 detector looks at the last ground-truth frame and the last predicted frame; the object the user moved is searched
for in both; the result is a detection F1 / accuracy and the distance between where the predicted object landed and where the
tracker says it should be.  FID and FVD are not provided (they need Inception / I3D weights and TensorFlow).

Differences from the reference, all documented in DESIGN §4.2f: the detector runs ONCE on the 2B frames instead of once per
object; candidates with equal scores keep their box order; a non-finite head box is removed instead of looping for ever."""
import statistics
import warnings

import torch

from . import ops
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
        if not images.is_cuda:
            raise RuntimeError("c2m_amd ops need tensors on a HIP device (no CPU fallback by design)")
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
        if not t.is_cuda:
            raise RuntimeError(f"c2m_amd ops need tensors on a HIP device (no CPU fallback by design): {name}")
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
