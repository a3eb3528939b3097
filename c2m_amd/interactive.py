"""Click-to-move: predict a video from the input frames and a drag on one object, without tracker files.

The reference (src/evaluator/evaluator.py:102-115 on src/datasets/cityscapes.py:79-199) needs per-object tracker boxes of
ALL frames, and the "user guidance" is the recorded future trajectory of a drawn node.  Here the objects and their
boxes come from the instance maps of the input frames (ops.instance_boxes, HIP), and a drag becomes the future boxes of
the clicked object.  Everything after that is the tracker path's own arithmetic (graph.scene_graph_from_boxes) and the
unchanged GeneratorFullModel.inference: the clicked node's theta is replaced by its targets_theta there
(SparseMotionDecoder: loc(x) * (1 - u) + targets_theta * u).

Conventions:
  - Pixels are at the model's working size (train_params.input_size = the size of the instance maps).
  - Instance boxes are turned into the tracker convention (x, y, w, h in 2048x1024 pixels) from their pixel edges
    (x_min, y_min, x_max + 1, y_max + 1).  A mask box is tighter than a SiamRPN++ tracker box.
  - Objects that are not dragged get stationary future boxes (identity theta).  With use_gt_eval: False (the shipped
    config) those thetas are multiplied by u = 0 and never read: the GNN predicts their motion.  With use_gt_eval: True
    every node's targets_theta drives the raster, so they mean "everything else stays still".
  - Several drags in one sample guide several nodes at once.  The reference trains with exactly one guided node per
    sample, so more than one is an extrapolation of what the model has seen.
"""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .graph import collate_graphs, scene_graph_from_boxes
from .synthetic import GraphBatch

TRACKER_W, TRACKER_H = 2048, 1024


@dataclass
class Drag:
    """A click on (x, y) of sample `sample` in the last input frame, dragged to (to_x, to_y) over the predicted frames.

    Frame t of T moves the box centre by (t + 1) / T * (to - from).  `path` (T points) gives the target of the clicked
    point per frame instead; `scale` (T factors, default 1) scales the box about its centre per frame."""
    sample: int
    x: float
    y: float
    to_x: Optional[float] = None
    to_y: Optional[float] = None
    path: Optional[Sequence[Sequence[float]]] = None
    scale: Optional[Sequence[float]] = None

    def displacements(self, num_predicted_frames):
        """[T, 2] float64 displacement (dx, dy) of the box centre per predicted frame, in pixels."""
        T = num_predicted_frames
        if self.path is not None:
            path = np.asarray(self.path, dtype=np.float64)
            if path.shape != (T, 2):
                raise ValueError(f"drag path must hold {T} (x, y) points, got shape {path.shape}")
            return path - np.array([self.x, self.y], dtype=np.float64)
        if self.to_x is None or self.to_y is None:
            raise ValueError("a drag needs (to_x, to_y) or a path")
        step = np.array([self.to_x - self.x, self.to_y - self.y], dtype=np.float64)
        return np.arange(1, T + 1, dtype=np.float64)[:, None] * step / T

    def scales(self, num_predicted_frames):
        T = num_predicted_frames
        if self.scale is None:
            return np.ones(T, dtype=np.float64)
        s = np.asarray(self.scale, dtype=np.float64)
        if s.shape != (T,) or not np.all(s > 0):
            raise ValueError(f"drag scale must hold {T} positive factors, got {self.scale!r}")
        return s


def edges_to_tracker(edges, size):
    """Pixel-edge boxes [..., 4] (x_min, y_min, x_max + 1, y_max + 1) at size (H, W) -> tracker boxes [..., 4] float64
    (x, y, w, h in 2048x1024 pixels)."""
    H, W = size
    e = np.asarray(edges, dtype=np.float64)
    sx, sy = TRACKER_W / W, TRACKER_H / H
    return np.stack([e[..., 0] * sx, e[..., 1] * sy, (e[..., 2] - e[..., 0]) * sx, (e[..., 3] - e[..., 1]) * sy], -1)


def future_edges(last, displacement, scale):
    """Pixel-edge box `last` (4,) moved by displacement [T, 2] and scaled about its centre by scale [T] -> [T, 4].
    A zero displacement with scale 1 returns `last` exactly (pixel edges are integers)."""
    x0, y0, x1, y1 = (float(v) for v in last)
    cx, cy, hw, hh = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2, (y1 - y0) / 2
    ncx, ncy = cx + displacement[:, 0], cy + displacement[:, 1]
    return np.stack([ncx - hw * scale, ncy - hh * scale, ncx + hw * scale, ncy + hh * scale], -1)


def _click_ids(instance, drags, t_in):
    """Instance id under every drag's pixel in the last input frame (one device -> host read)."""
    ys = torch.tensor([int(d.y) for d in drags], dtype=torch.long)
    xs = torch.tensor([int(d.x) for d in drags], dtype=torch.long)
    bs = torch.tensor([int(d.sample) for d in drags], dtype=torch.long)
    dev = instance.device
    return instance[bs.to(dev), t_in - 1, ys.to(dev), xs.to(dev)].cpu().tolist()


def _check_drags(drags, B, H, W):
    for d in drags:
        if not 0 <= int(d.sample) < B:
            raise ValueError(f"drag on sample {d.sample}, but the batch has {B} sample(s)")
        if not (0 <= d.x < W and 0 <= d.y < H):
            raise ValueError(f"drag pixel ({d.x}, {d.y}) is outside the {H}x{W} frame")


def graph_from_boxes(ids, edges, count, drags, clicked_ids, size, num_input_frames, num_predicted_frames,
                     id_range=(1000, 19000)):
    """Host half of graph_from_instances: the results of ops.instance_boxes (ids [B, max_nodes], edges
    [B, max_nodes, t_in, 4] pixel edges, count [B]), the drags and the id under each drag's pixel -> (GraphBatch,
    click_index).  Every field comes out of graph.scene_graph_from_boxes, the tracker path's arithmetic."""
    t_in, T = int(num_input_frames), int(num_predicted_frames)
    if T < 1:
        raise ValueError("num_predicted_frames must be >= 1")
    H, W = size
    id_lo, id_hi = (int(v) for v in id_range)
    B = int(count.shape[0])
    drags = list(drags)
    _check_drags(drags, B, H, W)
    picks, chosen = {}, []                            # (sample, node of the sample) -> drag; (sample, node) per drag
    for d, cid in zip(drags, clicked_ids):
        b, cid = int(d.sample), int(cid)
        where = f"pixel (x={int(d.x)}, y={int(d.y)}) of sample {b}"
        if not id_lo <= cid < id_hi:
            raise ValueError(f"{where} holds id {cid}, outside the object id range [{id_lo}, {id_hi}) "
                             "(background or stuff)")
        row = [int(v) for v in ids[b, :int(count[b])]]
        if cid not in row:
            raise ValueError(f"{where} holds id {cid}, which is not an object of every input frame "
                             "(or has too few pixels)")
        n = row.index(cid)
        if (b, n) in picks:
            raise ValueError(f"two drags select object {cid} of sample {b}")
        picks[(b, n)] = d
        chosen.append((b, n))
    graphs, base = [], []
    for b in range(B):
        N = int(count[b])
        if N == 0:
            raise ValueError(f"sample {b} has no object with an id in [{id_lo}, {id_hi}) in every input frame")
        e = np.asarray(edges[b, :N], dtype=np.float64)                    # [N, t_in, 4] pixel edges
        fut = np.repeat(e[:, t_in - 1:t_in], T, axis=1)                   # stationary future boxes
        for n in range(N):
            d = picks.get((b, n))
            if d is not None:
                fut[n] = future_edges(e[n, t_in - 1], d.displacements(T), d.scales(T))
        box = edges_to_tracker(np.concatenate([e, fut], 1), (H, W))
        node_ids = np.repeat(np.asarray(ids[b, :N], dtype=np.int64)[:, None], t_in + T, axis=1)
        _, g = scene_graph_from_boxes(box, node_ids, (H, W), t_in, t_in + T)
        base.append(sum(gr.num_nodes for gr in graphs))
        graphs.append(g)
    click_index = torch.tensor([base[b] + n for b, n in chosen], dtype=torch.long)
    return collate_graphs(graphs), click_index


def graph_from_instances(instance_mask, drags, num_input_frames, num_predicted_frames, **box_kw):
    """Object graphs of a batch from its instance maps and the user's drags.

    instance_mask: [B,1,T,H,W] or [B,T,H,W] integer ids on the device (T >= num_input_frames; later frames are not read).
    drags: Drag per guided object (usually one per sample; more are accepted, see the module docstring).
    box_kw: id_range, min_pixels, max_nodes of ops.instance_boxes.
    Returns (GraphBatch on the host with every field of graph.collate_graphs, click_index LongTensor of the dragged nodes
    in drag order)."""
    inst = instance_mask[:, 0] if instance_mask.dim() == 5 else instance_mask
    ids, edges, count = ops.instance_boxes(instance_mask, num_input_frames, **box_kw)
    drags = list(drags)
    _check_drags(drags, inst.shape[0], inst.shape[-2], inst.shape[-1])
    clicked = _click_ids(inst, drags, num_input_frames) if drags else []
    return graph_from_boxes(ids.numpy(), edges.numpy(), count.numpy(), drags, clicked, tuple(inst.shape[-2:]),
                            num_input_frames, num_predicted_frames, box_kw.get("id_range", (1000, 19000)))


def graph_to(graph, device):
    """Every tensor field of a GraphBatch on `device` (GraphBatch.to moves the fields the model reads only)."""
    return GraphBatch(**{k: v.to(device) if torch.is_tensor(v) else v for k, v in graph.__dict__.items()})


def click_to_move(model, video, bg_mask, fg_mask, instance_mask, drags, input_of=None, input_occ=None, z_m=None,
                  **box_kw):
    """Predict the num_predicted_frames future frames from the input frames and `drags`; returns the dict of
    model.inference.

    video [B,3,T,H,W], bg_mask [B,11,T,H,W], fg_mask [B,9,T,H,W], instance_mask [B,1,T,H,W] (or [B,T,H,W]) on the model's
    device, H x W = train_params.input_size; only the first num_input_frames frames are read (T may equal it).
    input_of / input_occ: the input-frame flows when the config uses them.  z_m: [B, fc.in_features] motion code; drawn from
    N(0, 1) with the torch CPU generator when None, as the reference's evaluator does.  The trajectory latent is drawn by
    inference() itself (seed torch for repeatable runs).  box_kw: id_range, min_pixels, max_nodes (ops.instance_boxes)."""
    tp = model.train_params
    t_in, T = tp["num_input_frames"], tp["num_predicted_frames"]
    size = tuple(int(v) for v in tp["input_size"])
    if tuple(video.shape[-2:]) != size or tuple(instance_mask.shape[-2:]) != size:
        raise ValueError(f"inputs must be at the model's working size {size}, got video {tuple(video.shape[-2:])} and "
                         f"instance maps {tuple(instance_mask.shape[-2:])}")
    device = next(model.parameters()).device
    graph, click_index = graph_from_instances(instance_mask, drags, t_in, T, **box_kw)
    inst = instance_mask if instance_mask.dim() == 5 else instance_mask.unsqueeze(1)
    first = lambda x: None if x is None else x[:, :, :t_in]
    if z_m is None:
        z_m = torch.FloatTensor(video.shape[0], model.motion_encoder.fc.in_features).normal_(0, 1)
    with torch.no_grad():
        return model.inference(first(video), first(bg_mask), first(fg_mask), first(inst), input_of, input_occ,
                               graph_to(graph, device), click_index.to(device), z_m.to(device))
