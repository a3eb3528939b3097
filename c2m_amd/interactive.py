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

Continuing a prediction (propagate_maps, continue_click_to_move, rollout): the model needs the one-hot semantic channels and
the instance ids of every input frame, and nothing produces them for a frame the model generated itself (the reference gets
them from Panoptic-DeepLab and an offline tracker).  Frame t of `generated` takes pixel p from position s(p) of the last input
frame, so the labels of frame t are the labels of the last input frame gathered at the pixel nearest to s(p)
(ops.label_warp, HIP: the bilinear warp's own coordinates, nearest neighbour, nothing blended).  With them the output of
one call is a complete input of the next, an object keeps its id across segments, and ops.instance_stats on the propagated
ids gives the dragged object's boxes in the predicted frames (predicted_boxes, drag_error).  DESIGN.md, "Label propagation",
has the coordinate rule and the ghost caveat of the sparse flow.  Where an object moved away the warp gathers the labels of the
object that used to be there; occ_threshold with fill="nearest" gives such pixels the labels of the nearest visible background
pixel instead (ops.nearest_fill, HIP).
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


def _pick_nodes(ids, count, drags, clicked_ids, size, id_range):
    """The node every drag selects: [(sample, node of the sample)] in drag order; a drag on no object, or two drags on one
    object, raise ValueError."""
    H, W = size
    id_lo, id_hi = (int(v) for v in id_range)
    _check_drags(drags, int(count.shape[0]), H, W)
    chosen = []
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
        if (b, n) in chosen:
            raise ValueError(f"two drags select object {cid} of sample {b}")
        chosen.append((b, n))
    return chosen


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
    chosen = _pick_nodes(ids, count, drags, clicked_ids, size, id_range)
    picks = dict(zip(chosen, drags))                  # (sample, node of the sample) -> drag
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


def _tracked_boxes(model, inst, t_in, input_of, track, box_kw):
    """The (ids, edges, count) of ops.instance_boxes from tracking.track_instances on the input frames: an object may carry
    a different id in every input frame; `ids` are the ids of the LAST input frame, the ones the model and the drags read.
    Also returns the input-frame maps with every tracked object relabelled to that id."""
    from .tracking import track_instances
    if t_in < 2:
        raise ValueError("track= links the objects of several input frames: it needs num_input_frames > 1")
    _check_continuable(model)
    kw = dict(box_kw, **(track if isinstance(track, dict) else {}))
    tr = track_instances(inst[:, :, :t_in], t_in, None, input_of, **kw)
    # the model reads the ids of every input frame as numbers (the encoder's instance channels): an object gets its
    # last-input-frame id in the earlier frames too, as maps with stable ids would have it
    relabelled = inst[:, :, :t_in].clone()
    for b in range(inst.shape[0]):
        for n in range(int(tr.count[b])):
            for f in range(t_in - 1):
                old, new = int(tr.ids[b, n, f]), int(tr.ids[b, n, t_in - 1])
                if old != new:
                    relabelled[b, 0, f][inst[b, 0, f] == old] = new
    return tr.ids[:, :, t_in - 1].contiguous().numpy(), tr.boxes.numpy(), tr.count.numpy(), relabelled


def _predict(model, video, bg_mask, fg_mask, instance_mask, drags, input_of, input_occ, z_m, box_kw, track=None):
    """click_to_move plus what it learnt about the objects on the way: (output dict of model.inference, dict(ids, edges,
    count: ops.instance_boxes of the input frames; nodes: [(sample, node)] per drag))."""
    tp = model.train_params
    t_in, T = tp["num_input_frames"], tp["num_predicted_frames"]
    size = tuple(int(v) for v in tp["input_size"])
    if tuple(video.shape[-2:]) != size or tuple(instance_mask.shape[-2:]) != size:
        raise ValueError(f"inputs must be at the model's working size {size}, got video {tuple(video.shape[-2:])} and "
                         f"instance maps {tuple(instance_mask.shape[-2:])}")
    device = next(model.parameters()).device
    inst = instance_mask if instance_mask.dim() == 5 else instance_mask.unsqueeze(1)
    if track:
        ids, edges, count, inst = _tracked_boxes(model, inst, t_in, input_of, track, box_kw)
    else:
        ids, edges, count = (t.numpy() for t in ops.instance_boxes(inst, t_in, **box_kw))
    drags = list(drags)
    _check_drags(drags, inst.shape[0], size[0], size[1])
    clicked = _click_ids(inst[:, 0], drags, t_in) if drags else []
    id_range = box_kw.get("id_range", (1000, 19000))
    graph, click_index = graph_from_boxes(ids, edges, count, drags, clicked, size, t_in, T, id_range)
    first = lambda x: None if x is None else x[:, :, :t_in]
    if z_m is None:
        z_m = torch.FloatTensor(video.shape[0], model.motion_encoder.fc.in_features).normal_(0, 1)
    with torch.no_grad():
        out = model.inference(first(video), first(bg_mask), first(fg_mask), first(inst), input_of, input_occ,
                              graph_to(graph, device), click_index.to(device), z_m.to(device))
    return out, dict(ids=ids, edges=edges, count=count, nodes=_pick_nodes(ids, count, drags, clicked, size, id_range))


def click_to_move(model, video, bg_mask, fg_mask, instance_mask, drags, input_of=None, input_occ=None, z_m=None,
                  track=None, **box_kw):
    """Predict the num_predicted_frames future frames from the input frames and `drags`; returns the dict of
    model.inference.

    video [B,3,T,H,W], bg_mask [B,11,T,H,W], fg_mask [B,9,T,H,W], instance_mask [B,1,T,H,W] (or [B,T,H,W]) on the model's
    device, H x W = train_params.input_size; only the first num_input_frames frames are read (T may equal it).
    input_of / input_occ: the input-frame flows when the config uses them.  z_m: [B, fc.in_features] motion code; drawn from
    N(0, 1) with the torch CPU generator when None, as the reference's evaluator does.  The trajectory latent is drawn by
    inference() itself (seed torch for repeatable runs).  box_kw: id_range, min_pixels, max_nodes (ops.instance_boxes).
    track: None (the default) takes an object to be the same id in every input frame; True, or a dict of min_iou /
    same_class, links the objects of the input frames with tracking.track_instances instead (num_input_frames > 1, maps whose
    ids change from frame to frame; input_of, when given, carries the association; scale_factor != 1 is refused)."""
    return _predict(model, video, bg_mask, fg_mask, instance_mask, drags, input_of, input_occ, z_m, box_kw, track)[0]


# ------------------------------------------------------------------------------------------------ continuing a prediction
FLOW_OCC = {"dense_motion_bw": "occlusion_bw", "sparse_motion_bw": "sparse_occ_bw"}


FILLS = (None, "nearest")


def _check_fill(fill, occ_threshold):
    if fill not in FILLS:
        raise ValueError(f"fill must be one of {list(FILLS)}, got {fill!r}")
    if fill is not None and occ_threshold is None:
        raise ValueError(f"fill={fill!r} fills the pixels whose occlusion value is below occ_threshold: it needs occ_threshold")


def propagate_maps(out, bg_mask, fg_mask, instance_mask, num_input_frames, flow="dense_motion_bw", occ_threshold=None,
                   fill_id=0, fill=None, id_range=(1000, 19000)):
    """Label maps of the predicted frames: the maps of input frame num_input_frames - 1 (no other frame is read) carried
    along the backward flow out[flow] by ops.label_warp -> dict(bg_mask [B,11,T,H,W], fg_mask [B,9,T,H,W] fp32, instance_mask
    [B,1,T,H,W] int32), on the device.

    flow: "dense_motion_bw" (the default), the flow the generator drew `generated` with, so the maps line up with its
    pixels; or "sparse_motion_bw", the rasterised object motion: exact for a rigid drag, but zero off the objects' new
    supports, so an object's id also stays at its OLD place (a ghost) wherever no other object's support covers it.
    occ_threshold: instance ids become fill_id where the matching occlusion map (occlusion_bw / sparse_occ_bw) is below
    it -- a disoccluded pixel belongs to no known object.  With fill=None the semantic channels of such a pixel stay as
    gathered: they name the object that used to cover it.
    fill: "nearest" (needs occ_threshold) gives every disoccluded pixel (a hole: occ < occ_threshold) ALL its label planes, the
    20 semantic channels and the id, from the nearest pixel of the same frame that is visible and belongs to no object (a
    seed: no hole, warped id outside id_range) -- ops.nearest_fill, HIP: exact Euclidean distance, ties to the smaller row,
    then the smaller column.  A filled pixel carries its seed's stuff id, consistent with its one-hot channels; fill_id remains
    the id of the holes of a frame that has no seed.  The dict then also holds unfilled [B,T] int32 on the device: the holes
    each frame kept because it has no seed."""
    if flow not in FLOW_OCC:
        raise ValueError(f"flow must be one of {sorted(FLOW_OCC)}, got {flow!r}")
    _check_fill(fill, occ_threshold)
    last = int(num_input_frames) - 1
    inst = instance_mask if instance_mask.dim() == 5 else instance_mask.unsqueeze(1)
    for name, t in (("bg_mask", bg_mask), ("fg_mask", fg_mask), ("instance_mask", inst)):
        if t.dim() != 5 or not 0 <= last < t.shape[2]:
            raise ValueError(f"{name} must be [B,C,T,H,W] with T >= num_input_frames={num_input_frames}, got "
                             f"{tuple(t.shape)}")
    if inst.dtype.is_floating_point:
        raise ValueError(f"instance maps hold integer ids, got {inst.dtype}")
    f = out[flow]
    if tuple(f.shape[-2:]) != tuple(inst.shape[-2:]):
        raise ValueError(f"{flow} is {tuple(f.shape[-2:])} but the maps are {tuple(inst.shape[-2:])}: flows and frames "
                         "at different sizes (common_params.scale_factor != 1) are not supported yet")
    nbg = bg_mask.shape[1]
    planes_f = torch.cat([bg_mask[:, :, last], fg_mask[:, :, last]], 1).float()
    planes_i = inst[:, :, last].to(torch.int32)
    occ = None if occ_threshold is None else out[FLOW_OCC[flow]]
    with torch.no_grad():
        of, oi = ops.label_warp(f, planes_f, planes_i, occ, occ_threshold, fill_id)
        maps = dict(bg_mask=of[:, :nbg], fg_mask=of[:, nbg:], instance_mask=oi)
        if fill == "nearest":
            id_lo, id_hi = (int(v) for v in id_range)
            hole = occ[:, 0] < occ_threshold                       # the comparison label_warp's kernel makes on the same map
            ids = oi[:, 0]
            seed = ~hole & ((ids < id_lo) | (ids >= id_hi))
            maps["unfilled"] = ops.nearest_fill(hole, seed, of, oi)
    return maps


def boxes_from_stats(rows):
    """Rows of the ops.instance_stats table [..., 5] (count, x_min, x_max, y_min, y_max) -> (boxes [..., 4] pixel edges
    (x_min, y_min, x_max + 1, y_max + 1), zero where the id is absent; presence [...] bool)."""
    presence = rows[..., 0] > 0
    boxes = torch.stack([rows[..., 1], rows[..., 3], rows[..., 2] + 1, rows[..., 4] + 1], -1)
    return boxes * presence.unsqueeze(-1).to(boxes.dtype), presence


def predicted_boxes(maps_or_instance, ids=None, id_range=(1000, 19000)):
    """Boxes of the objects in every frame of an instance map on the device (the propagated one: where the flow put them).

    maps_or_instance: the dict of propagate_maps, or instance maps [B,1,T,H,W] / [B,T,H,W].  ids: [B, N] object ids per
    sample, e.g. the `ids` of ops.instance_boxes on the input frames (values outside id_range, such as its zero padding, are
    never present); None: every id of id_range that occurs in some frame, ascending, padded with -1 (one more device ->
    host read).  Returns CPU tensors: ids [B, N] int64, boxes [B, N, T, 4] int32 pixel edges (zero where absent) and
    presence [B, N, T] bool -- an object may leave the frame or be covered completely, and unlike ops.instance_boxes
    this keeps it, frame by frame.  Built on the ops.instance_stats table; one device -> host read of [B, N, T, 5]."""
    inst = maps_or_instance["instance_mask"] if isinstance(maps_or_instance, dict) else maps_or_instance
    T = inst.shape[-3]
    lo, hi = (int(v) for v in id_range)
    table = ops.instance_stats(inst, T, id_range)                       # [B, T, hi - lo, 5] on the device
    B = table.shape[0]
    if ids is None:
        seen = (table[..., 0] > 0).any(1).cpu()                         # [B, hi - lo]
        rows = [torch.nonzero(r).flatten() + lo for r in seen]
        ids = torch.full((B, max([len(r) for r in rows] + [1])), -1, dtype=torch.int64)
        for b, r in enumerate(rows):
            ids[b, :len(r)] = r
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64).reshape(B, -1)
    valid = (ids >= lo) & (ids < hi)
    col = (ids - lo).clamp(0, hi - lo - 1).to(table.device)
    rows = table[torch.arange(B, device=table.device)[:, None], :, col].cpu()        # [B, N, T, 5]
    boxes, presence = boxes_from_stats(rows)
    presence = presence & valid[:, :, None]
    return ids, boxes * presence.unsqueeze(-1).to(boxes.dtype), presence


@dataclass
class DragTarget:
    """Where a drag asks its object to be: node `node` of sample `sample` (a column of the `ids` the boxes were taken
    for), its box in the last input frame and the requested boxes of the T predicted frames, pixel edges."""
    sample: int
    node: int
    start: np.ndarray          # [4]
    edges: np.ndarray          # [T, 4]


def drag_targets(drags, nodes, edges, num_input_frames, num_predicted_frames):
    """DragTarget per drag from the nodes the drags selected ([(sample, node)], drag order) and the input-frame boxes
    `edges` [B, N, t_in, 4] of ops.instance_boxes: the boxes graph_from_boxes turns into the guided node's targets_theta."""
    t_in, T = int(num_input_frames), int(num_predicted_frames)
    out = []
    for d, (b, n) in zip(drags, nodes):
        start = np.asarray(edges[b, n, t_in - 1], dtype=np.float64)
        out.append(DragTarget(int(b), int(n), start, future_edges(start, d.displacements(T), d.scales(T))))
    return out


def _centres(e):
    e = np.asarray(e, dtype=np.float64)
    return np.stack([(e[..., 0] + e[..., 2]) / 2, (e[..., 1] + e[..., 3]) / 2], -1)


def drag_error(targets, boxes, presence):
    """How far every dragged object ended up from where its drag asked it to be, without a detector.

    targets: DragTarget list (drag_targets); boxes [B, N, T, 4], presence [B, N, T]: predicted_boxes of the PROPAGATED
    instance map for the same ids.  Returns a dict of float64 arrays:
      distance [D, T]   pixels between the centre of the requested box and the centre of the object's box, per frame; nan
                        in a frame where the object is absent (it left the frame or is covered) -- never a silent 0;
      displacement [D]  pixels between the centre of the start box and the centre of the last requested box;
      normalized [D]    distance[:, -1] / ((displacement if displacement > 0 else 1) + 1e-6): the reference's rule for
                        a zero displacement (utils_yolov3.py:130-136).
    This is the reference's mse_traj_loss / mse_normalized_traj_loss with the YOLOv3 detections replaced by the boxes of
    the propagated ids (and without its int() truncation of the box corners).  It measures the FLOW the generator used --
    where the model moved the object's pixels from -- not the rendered pixels: an object the generator paints badly at the
    right place scores 0, and the sparse flow's ghost (propagate_maps) stretches a box back to the object's old place."""
    boxes, presence = np.asarray(boxes), np.asarray(presence)
    D = len(targets)
    T = boxes.shape[2] if boxes.ndim == 4 else 0
    distance, displacement = np.full((D, T), np.nan), np.zeros(D)
    for k, g in enumerate(targets):
        want, got = _centres(g.edges), _centres(boxes[g.sample, g.node])
        if want.shape != got.shape:
            raise ValueError(f"target {k} holds {want.shape[0]} frames but the boxes hold {got.shape[0]}")
        dist = np.sqrt(((want - got) ** 2).sum(-1))
        distance[k] = np.where(presence[g.sample, g.node], dist, np.nan)
        displacement[k] = np.sqrt(((want[-1] - _centres(g.start)) ** 2).sum())
    divisor = np.where(displacement > 0, displacement, 1.0) + 1e-6
    normalized = distance[:, -1] / divisor if T else np.full(D, np.nan)
    return dict(distance=distance, displacement=displacement, normalized=normalized)


def _reads_input_flows(model):
    cp = model.model_params["common_params"]
    return model.train_params["num_input_frames"] > 1 and cp["flow_channel"] + cp["occlusion_channel"] > 0


def _check_continuable(model):
    sf = model.model_params["common_params"]["scale_factor"]
    if isinstance(sf, (list, tuple)) or sf != 1:
        raise ValueError(f"common_params.scale_factor = {sf}: flows and frames are then at different sizes; continuing "
                         "a prediction is not supported yet for scale_factor != 1")


def next_inputs(prev_inputs, out, maps, num_input_frames, flow_fn=None, needs_flows=False):
    """The inputs of the next call from the previous call: per tensor, the first num_input_frames frames of the previous
    inputs followed by the predicted frames (`generated`, `maps` of propagate_maps), of which the LAST num_input_frames
    frames are kept -> dict(video, bg_mask, fg_mask, instance_mask [B,1,t_in,H,W] int32, input_of, input_occ).

    needs_flows: the model reads the flows between consecutive input frames (num_input_frames > 1).  Nothing else
    produces them for generated frames, so the caller supplies flow_fn(frame_a, frame_b) -> (flow [B,2,H,W], occ
    [B,1,H,W]) on frames [B,3,H,W] as they are in `video`, e.g. FlowNet.compute_flow_and_conf behind the caller's
    value-range mapping.  As in train.compute_flow, input_of[:, :, i] is the flow of (i -> i + 1) and input_occ[:, :, i] the
    occlusion map of the reverse pair."""
    t_in = int(num_input_frames)
    if needs_flows and t_in > 1 and flow_fn is None:
        raise ValueError(f"the model reads the flows between its {t_in} input frames: continuing needs "
                         "flow_fn(frame_a, frame_b) -> (flow, occ), e.g. FlowNet.compute_flow_and_conf")
    inst = prev_inputs["instance_mask"]
    inst = inst if inst.dim() == 5 else inst.unsqueeze(1)
    join = lambda old, new: torch.cat([old[:, :, :t_in].to(new.dtype), new], 2)[:, :, -t_in:]
    nxt = dict(video=join(prev_inputs["video"], out["generated"]), bg_mask=join(prev_inputs["bg_mask"], maps["bg_mask"]),
               fg_mask=join(prev_inputs["fg_mask"], maps["fg_mask"]), instance_mask=join(inst, maps["instance_mask"]),
               input_of=None, input_occ=None)
    if needs_flows and t_in > 1:
        v = nxt["video"]
        nxt["input_of"] = torch.stack([flow_fn(v[:, :, i], v[:, :, i + 1])[0] for i in range(t_in - 1)], 2)
        nxt["input_occ"] = torch.stack([flow_fn(v[:, :, i + 1], v[:, :, i])[1] for i in range(t_in - 1)], 2)
    return nxt


def continue_click_to_move(model, prev_inputs, out, drags, flow_fn=None, z_m=None, flow="dense_motion_bw",
                           occ_threshold=None, fill=None, **box_kw):
    """The next prediction from the previous one: drag again from where the objects now are.

    prev_inputs: dict(video, bg_mask, fg_mask, instance_mask) of the previous call (its first num_input_frames frames are
    read); out: what that call returned.  drags: in the coordinates of the LAST generated frame; the object under a click is
    looked up in the propagated instance map, so it keeps the id it had in the first frame.  flow, occ_threshold, fill:
    propagate_maps (box_kw's id_range, when given, is also its id_range); flow_fn: next_inputs (needed when the model reads
    input-frame flows, i.e. num_input_frames > 1; not with the shipped num_input_frames: 1); z_m, box_kw: click_to_move.
    common_params.scale_factor != 1 is not supported yet (ValueError).  Returns (the dict of model.inference, the inputs it
    was called on: prev_inputs of the next call)."""
    _check_continuable(model)
    t_in = model.train_params["num_input_frames"]
    maps = propagate_maps(out, prev_inputs["bg_mask"], prev_inputs["fg_mask"], prev_inputs["instance_mask"], t_in, flow,
                          occ_threshold, fill=fill, id_range=box_kw.get("id_range", (1000, 19000)))
    with torch.no_grad():
        nxt = next_inputs(prev_inputs, out, maps, t_in, flow_fn, _reads_input_flows(model))
    return click_to_move(model, nxt["video"], nxt["bg_mask"], nxt["fg_mask"], nxt["instance_mask"], drags, nxt["input_of"],
                         nxt["input_occ"], z_m, **box_kw), nxt


def rollout(model, video, bg_mask, fg_mask, instance_mask, segments, input_of=None, input_occ=None, flow_fn=None,
            z_m=None, flow="dense_motion_bw", occ_threshold=None, fill=None, **box_kw):
    """A prediction of len(segments) * num_predicted_frames frames: click_to_move on the inputs, then
    continue_click_to_move on every result.

    segments: a list of drag lists, one per segment, each in the coordinates of the frame the segment starts from; an empty
    list guides no object (the GNN decides every motion).  z_m: None or one motion code per segment.  The other arguments:
    click_to_move and continue_click_to_move.  Returns a dict:
      generated [B,3,K*T,H,W]; bg_mask [B,11,K*T,H,W], fg_mask [B,9,K*T,H,W], instance_mask [B,1,K*T,H,W]: the
      propagated maps of every predicted frame; outputs: the K dicts of model.inference;
      ids [K][B, N]: the objects each segment started with (ops.instance_boxes); boxes [K][B, N, T, 4], presence
      [K][B, N, T]: predicted_boxes of them in the segment's frames; targets [K]: drag_targets of the segment's drags;
      drag_errors [K]: drag_error of them.
    fill="nearest" (with occ_threshold; propagate_maps): every disoccluded pixel of the propagated maps takes its labels from the
    nearest visible background pixel, so the next segment is fed maps that agree with themselves; the dict then also holds
    unfilled [B,K*T] int32 on the device, the holes each frame kept because it has no seed.
    A sample whose every object has left the frame (or is covered) ends the rollout with the "no object" ValueError of
    graph_from_boxes, prefixed with the segment.  Per segment the host reads what click_to_move reads plus the
    [B, N, T, 5] box table; frames and maps stay on the device."""
    segments = [list(s) for s in segments]
    if not segments:
        raise ValueError("rollout needs at least one segment (an empty drag list is a segment without guidance)")
    if z_m is not None and len(z_m) != len(segments):
        raise ValueError(f"z_m holds {len(z_m)} motion codes for {len(segments)} segments")
    if len(segments) > 1:
        _check_continuable(model)
    _check_fill(fill, occ_threshold)
    tp = model.train_params
    t_in, T = tp["num_input_frames"], tp["num_predicted_frames"]
    id_range = box_kw.get("id_range", (1000, 19000))
    inputs = dict(video=video, bg_mask=bg_mask, fg_mask=fg_mask, instance_mask=instance_mask, input_of=input_of,
                  input_occ=input_occ)
    res = dict(outputs=[], maps=[], ids=[], boxes=[], presence=[], targets=[], drag_errors=[])
    out = maps = None
    for k, drags in enumerate(segments):
        try:
            if k > 0:
                with torch.no_grad():
                    inputs = next_inputs(inputs, out, maps, t_in, flow_fn, _reads_input_flows(model))
            out, info = _predict(model, inputs["video"], inputs["bg_mask"], inputs["fg_mask"], inputs["instance_mask"], drags,
                                 inputs["input_of"], inputs["input_occ"], None if z_m is None else z_m[k], box_kw)
        except ValueError as e:
            raise ValueError(f"segment {k}: {e}") from e
        maps = propagate_maps(out, inputs["bg_mask"], inputs["fg_mask"], inputs["instance_mask"], t_in, flow,
                              occ_threshold, fill=fill, id_range=id_range)
        ids, boxes, presence = predicted_boxes(maps, info["ids"], id_range)
        res["outputs"].append(out)
        res["maps"].append(maps)
        res["ids"].append(ids)
        res["boxes"].append(boxes)
        res["presence"].append(presence)
        res["targets"].append(drag_targets(drags, info["nodes"], info["edges"], t_in, T))
        res["drag_errors"].append(drag_error(res["targets"][-1], boxes, presence))
    maps = res.pop("maps")
    res["generated"] = torch.cat([o["generated"] for o in res["outputs"]], 2)
    for key in ("bg_mask", "fg_mask", "instance_mask"):
        res[key] = torch.cat([m[key] for m in maps], 2)
    if fill is not None:
        res["unfilled"] = torch.cat([m["unfilled"] for m in maps], 1)
    return res
