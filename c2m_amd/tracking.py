"""Tracks from instance maps and flows: a training batch without tracker files.

The reference (src/datasets/cityscapes.py:79-199) reads one text file per object with a box and an id per frame, written by an
offline SiamRPN++ run.  Per-frame panoptic maps do not keep an object's id from frame to frame, so the boxes of "the same
object" in all num_input_frames + num_predicted_frames frames cannot be read off the maps by id.  This module associates the
objects of every frame with the objects of the ANCHOR, the last input frame, on the device (csrc/instance_link.hip):

  - target frame t is linked directly to the anchor through target_bw_of[:, :, t], the flow ops.label_warp consumes: pixel p of
    frame t came from the pixel nearest to p + flow(p) of the anchor (csrc/warp_coord.h, the same coordinates bit for bit);
  - input frame i < anchor is linked to frame i + 1 through input_of[:, :, i] (defined on frame i, pointing into i + 1) and the
    links are composed down the chain;
  - a missing flow means same-pixel overlap.

Two objects are linked when each is the other's best match by IoU of their pixel sets (the anchor's set taken through the flow),
the IoU is at least min_iou (1/4 by default: a rule, not a measurement) and, with same_class, both ids have the same id // 1000.
An anchor object is a node only if it is linked in EVERY frame (the reference refuses short tracks too); the others are listed
in `lost`.  Objects that appear after the anchor are ignored.  The nodes are the anchor's objects in ascending id order, the
order of ops.instance_boxes, so for num_input_frames = 1 they coincide with interactive.graph_from_instances.

Everything after the association is the tracker path's own arithmetic: interactive.edges_to_tracker and
graph.scene_graph_from_boxes.  DESIGN.md §4.2d has the rules in full.
"""
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np
import torch

from . import ops
from .graph import collate_graphs, scene_graph_from_boxes, tracking_mask


@dataclass
class Tracks:
    """ids [B, max_nodes, T] int32: the id of node n in every frame; boxes [B, max_nodes, T, 4] int32 pixel edges (x_min, y_min,
    x_max + 1, y_max + 1); count [B] int32 (nodes per sample; rows past it are zero); lost [B]: per sample, (anchor id, frame)
    of every anchor object that is not a node and the frame that lost it -- the input frame nearest the anchor where its chain
    broke, else the first target frame without a link.  All on the host."""
    ids: torch.Tensor
    boxes: torch.Tensor
    count: torch.Tensor
    lost: List[List[Tuple[int, int]]] = field(default_factory=list)


def match_host(pairs, ref_ids, frame_ids, min_iou=(1, 4), same_class=True):
    """The match rule of ops.instance_match for one plane, stated on the host with Python integers (the kernel's yardstick; no
    product path calls it).  pairs [nr + 1, nf + 1]: the overlap table with its "no slot" row and column last; ref_ids [nr],
    frame_ids [nf] ascending.  Returns link [nr]: the frame slot of every ref slot or -1."""
    n = [[int(v) for v in row] for row in np.asarray(pairs)]
    nr, nf = len(ref_ids), len(frame_ids)
    if len(n) != nr + 1 or any(len(row) != nf + 1 for row in n):
        raise ValueError(f"pairs must be [{nr + 1}, {nf + 1}] for {nr} and {nf} ids, got {np.asarray(pairs).shape}")
    num, den = (int(v) for v in min_iou)
    r = [sum(row) for row in n]
    a = [sum(n[i][j] for i in range(nr + 1)) for j in range(nf + 1)]

    def best(cands, cell):
        top = None                                  # (n, union) of the best so far; ties keep the earlier (lower id)
        for k in cands:
            c, u = cell(k)
            if c > 0 and (top is None or c * top[2] > top[1] * u):
                top = (k, c, u)
        return top

    best_ref = [best(range(nr), lambda i: (n[i][j], r[i] + a[j] - n[i][j])) for j in range(nf)]
    link = []
    for i in range(nr):
        top = best(range(nf), lambda j: (n[i][j], r[i] + a[j] - n[i][j]))
        ok = top is not None and best_ref[top[0]][0] == i and top[1] * den >= num * top[2]
        if ok and same_class:
            ok = int(ref_ids[i]) // 1000 == int(frame_ids[top[0]]) // 1000
        link.append(top[0] if ok else -1)
    return np.asarray(link, dtype=np.int64).reshape(nr)


def check_config(config):
    """common_params.scale_factor != 1 puts flows and frames at different sizes: refused, as in interactive.py."""
    sf = config["model_params"]["common_params"]["scale_factor"]
    if isinstance(sf, (list, tuple)) or sf != 1:
        raise ValueError(f"common_params.scale_factor = {sf}: flows and frames are then at different sizes; tracking from "
                         "instance maps is not supported yet for scale_factor != 1")


def _flow_input(name, flow, B, frames, H, W):
    """A flow argument checked before anything is launched: [B, 2, frames, H, W] fp32 on the device, or None."""
    if flow is None:
        return None
    if not isinstance(flow, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(flow).__name__}")
    if flow.dtype != torch.float32:
        raise TypeError(f"{name} must be fp32 (coordinates are never rounded), got {flow.dtype}")
    if flow.dim() != 5 or flow.shape[1] != 2:
        raise ValueError(f"{name} must be [B,2,T,H,W], got {list(flow.shape)}")
    if tuple(flow.shape[-2:]) != (H, W):
        raise ValueError(f"{name} is {tuple(flow.shape[-2:])} but the maps are {(H, W)}: flows and frames at different "
                         "sizes (common_params.scale_factor != 1) are not supported yet")
    if flow.shape[0] != B or flow.shape[2] != frames:
        raise ValueError(f"{name} must be {[B, 2, frames, H, W]} for these maps, got {list(flow.shape)}")
    ops._hip_only(flow)
    return flow.detach()


def _link_group(inst, slots, count, frames, refs, flow, min_iou, same_class):
    """link [B, len(frames), M]: for frame frames[k] of every sample, the slot in it of every slot of frame refs[k]."""
    B, _, H, W = inst.shape
    n, M = len(frames), slots.shape[-1]
    P = B * n
    pick = lambda x, idx: x[:, idx].reshape((P,) + tuple(x.shape[2:]))
    fl = None if flow is None else flow.permute(0, 2, 1, 3, 4).reshape(P, 2, H, W)
    rs, rc, fs, fc = pick(slots, refs), pick(count, refs), pick(slots, frames), pick(count, frames)
    pairs = ops.instance_overlap(pick(inst, refs), pick(inst, frames), fl, rs, rc, fs, fc)
    return ops.instance_match(pairs, rs, rc, fs, fc, min_iou, same_class).view(B, n, M)


def track_instances(instance_mask, num_input_frames, target_bw_of=None, input_of=None, id_range=(1000, 19000), min_pixels=1,
                    max_nodes=64, min_iou=(1, 4), same_class=True):
    """The objects of the last input frame followed through all T frames of per-frame instance maps -> Tracks.

    instance_mask [B,1,T,H,W] or [B,T,H,W] integer ids on the device; T >= num_input_frames (T = num_input_frames: input
    frames only, as click-to-move needs).  target_bw_of [B,2,T - num_input_frames,H,W], input_of [B,2,num_input_frames - 1,H,W]:
    fp32 pixel flows at the size of the maps, or None (same-pixel overlap).  id_range, min_pixels, max_nodes: what counts as
    an object in a frame (ops.instance_boxes); max_nodes <= 64.  min_iou = (num, den), same_class: ops.instance_match.
    A sample without a node, and a frame with more than max_nodes objects, raise ValueError.  The association runs on the
    device; the host reads ONE buffer (ids, boxes, links, counts, overflow flags) at the end."""
    t_in = int(num_input_frames)
    if not isinstance(instance_mask, torch.Tensor) or instance_mask.dim() not in (4, 5):
        raise ValueError("instance maps must be [B,1,T,H,W] or [B,T,H,W], got "
                         f"{list(getattr(instance_mask, 'shape', ()))}")
    if instance_mask.dtype.is_floating_point or instance_mask.dtype == torch.bool or instance_mask.is_complex():
        raise TypeError(f"instance maps hold integer ids, got {instance_mask.dtype}")
    B, (T, H, W) = instance_mask.shape[0], instance_mask.shape[-3:]
    id_lo, id_hi = (int(v) for v in id_range)
    if not 0 <= id_lo < id_hi:
        raise ValueError(f"id_range must satisfy 0 <= lo < hi, got {id_range}")
    if int(min_pixels) < 1 or int(max_nodes) < 1:
        raise ValueError("min_pixels and max_nodes must be >= 1")
    # every dtype and shape before the device is looked at: the messages do not depend on where the tensors are
    for name, flow, frames in (("target_bw_of", target_bw_of, T - t_in), ("input_of", input_of, t_in - 1)):
        if flow is not None and (not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or flow.dim() != 5 or
                                 tuple(flow.shape) != (B, 2, frames, H, W)):
            _flow_input(name, flow, B, frames, H, W)
    inst = ops._instance_input(instance_mask, t_in)
    M, min_pixels = ops._link_nodes(max_nodes, min_pixels)
    target_bw_of = _flow_input("target_bw_of", target_bw_of, B, T - t_in, H, W)
    input_of = _flow_input("input_of", input_of, B, t_in - 1, H, W)
    a = t_in - 1
    dev = inst.device
    with torch.no_grad():
        table = ops.instance_stats(inst, T, id_range)                                           # [B, T, nid, 5]
        slots, boxes, _, count, overflow = ops.instance_slots(table, id_range, min_pixels, M)   # [B, T, M] ...
        lane = torch.arange(M, device=dev)
        slot = torch.full((B, M, T), -1, device=dev, dtype=torch.int64)     # the slot in frame f of anchor slot s
        slot[:, :, a] = torch.where(lane[None] < count[:, a, None], lane[None], -1)
        if T > t_in:
            link = _link_group(inst, slots, count, list(range(t_in, T)), [a] * (T - t_in), target_bw_of, min_iou, same_class)
            slot[:, :, t_in:] = torch.where(slot[:, :, a:a + 1] >= 0, link.permute(0, 2, 1).long(), -1)
        if t_in > 1:
            link = _link_group(inst, slots, count, list(range(a)), list(range(1, t_in)), input_of, min_iou, same_class)
            for f in range(a - 1, -1, -1):                                  # composed down the chain, on the device
                prev = slot[:, :, f + 1]
                step = torch.gather(link[:, f].long(), 1, prev.clamp(min=0))
                slot[:, :, f] = torch.where(prev >= 0, step, -1)
        at = slot.clamp(min=0)
        ids = torch.gather(slots.permute(0, 2, 1), 1, at)                   # [B, M, T]
        edges = torch.gather(boxes.permute(0, 2, 1, 3), 1, at[..., None].expand(B, M, T, 4))
        n_ids, n_box = B * M * T, B * M * T * 4
        host = torch.cat([ids.reshape(-1), edges.reshape(-1), (slot >= 0).to(torch.int32).reshape(-1), count.reshape(-1),
                          overflow.reshape(-1)]).cpu()
    ids, edges = host[:n_ids].view(B, M, T), host[n_ids:n_ids + n_box].view(B, M, T, 4)
    valid = host[n_ids + n_box:2 * n_ids + n_box].view(B, M, T).bool()
    count = host[2 * n_ids + n_box:2 * n_ids + n_box + B * T].view(B, T)
    overflow = host[2 * n_ids + n_box + B * T:].view(B, T)
    return tracks_from_links(ids, edges, valid, count, overflow, t_in, id_range)


def tracks_from_links(ids, edges, valid, count, overflow, num_input_frames, id_range=(1000, 19000)):
    """Host half of track_instances: what the device found for every anchor slot s and frame f -- ids [B, M, T], edges
    [B, M, T, 4], valid [B, M, T] (s has a link in f), and per frame count [B, T], overflow [B, T] -- -> Tracks: the slots
    that are linked in every frame, in order; the others in `lost`.  Raises the ValueErrors of track_instances."""
    t_in = int(num_input_frames)
    B, M, T = ids.shape
    a = t_in - 1
    id_lo, id_hi = (int(v) for v in id_range)
    bad = overflow.any(1).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"sample(s) {bad} hold more than max_nodes={M} objects in a frame; the object graph is complete "
                         "(N*(N-1) edges), raise min_pixels (max_nodes is capped by the kernels)")
    out = Tracks(torch.zeros(B, M, T, dtype=torch.int32), torch.zeros(B, M, T, 4, dtype=torch.int32),
                 torch.zeros(B, dtype=torch.int32), [])
    order = list(range(a - 1, -1, -1)) + list(range(t_in, T))               # where a track is looked for first
    for b in range(B):
        n = int(count[b, a])
        keep = valid[b, :n].all(1)
        gone = []
        for s in (~keep).nonzero().flatten().tolist():
            gone.append((int(ids[b, s, a]), next(f for f in order if not valid[b, s, f])))
        out.lost.append(gone)
        k = int(keep.sum())
        if k == 0:
            raise ValueError(f"sample {b} has no object with an id in [{id_lo}, {id_hi}) that is linked in every frame"
                             + (f" (lost: {gone})" if gone else ""))
        out.ids[b, :k], out.boxes[b, :k], out.count[b] = ids[b, :n][keep], edges[b, :n][keep], k
    return out


def anchor_pairs(tracks, num_input_frames):
    """Tracks -> (from [B*T, max_nodes], to [B*T, max_nodes], count [B*T]) int64 on the host: for plane (b, t) the pairs
    (tracks.ids[b, n, t], tracks.ids[b, n, num_input_frames - 1]) of the nodes n < count[b]."""
    ids = tracks.ids.numpy().astype(np.int64)                               # [B, M, T]
    B, M, T = ids.shape
    if not 1 <= int(num_input_frames) <= T:
        raise ValueError(f"num_input_frames={num_input_frames} but the tracks have {T} frames")
    frm = ids.transpose(0, 2, 1).reshape(B * T, M)
    to = np.broadcast_to(ids[:, None, :, int(num_input_frames) - 1], (B, T, M)).reshape(B * T, M)
    count = np.repeat(tracks.count.numpy().astype(np.int64), T)
    return frm, np.ascontiguousarray(to), count


def anchor_maps(instance_mask, tracks, num_input_frames, thing_list=tuple(range(11, 19)), label_divisor=1000):
    """The instance maps of the real frames in the id space of the ANCHOR (the last input frame), on the device: what a rollout's
    maps, which carry the anchor's ids through the predicted frames, are scored against (evaluate.tube_quality).

    instance_mask [B,1,T,H,W] or [B,T,H,W] int32 on the device; tracks: track_instances' result for the same maps.  In plane
    (b, t) a value equal to tracks.ids[b, n, t] of a node n < count[b] becomes tracks.ids[b, n, num_input_frames - 1]; every
    other thing value (v >= label_divisor, v // label_divisor in thing_list) becomes its class's crowd id (v // label_divisor) *
    label_divisor -- an object the anchor does not know, or one whose track broke, neither rewards nor punishes a prediction that
    could not contain it; stuff and void stay.  The mapping is simultaneous (two objects may swap ids).  Returns a new tensor of
    the input's shape (ops.instance_relabel: one upload, one launch on the current stream)."""
    if not isinstance(instance_mask, torch.Tensor) or instance_mask.dim() not in (4, 5) or \
            (instance_mask.dim() == 5 and instance_mask.shape[1] != 1):
        raise ValueError(f"instance maps must be [B,1,T,H,W] or [B,T,H,W], got {list(getattr(instance_mask, 'shape', ()))}")
    if instance_mask.dtype != torch.int32:
        raise TypeError(f"instance maps must be int32, got {instance_mask.dtype}")
    if not isinstance(tracks, Tracks):
        raise TypeError(f"tracks must be a Tracks, got {type(tracks).__name__}")
    B, T = instance_mask.shape[0], instance_mask.shape[-3]
    if tuple(tracks.ids.shape[::2]) != (B, T) or tuple(tracks.count.shape) != (B,):
        raise ValueError(f"tracks of {tracks.ids.shape[0]} samples and {tracks.ids.shape[2]} frames for maps of {B} and {T}")
    frm, to, count = anchor_pairs(tracks, num_input_frames)
    maps = instance_mask if instance_mask.is_contiguous() else instance_mask.contiguous()
    return ops.instance_relabel(maps, frm, to, count, thing_list, label_divisor)


def scene_graphs(tr, size, num_input_frames, lambda_traj=1):
    """Tracks -> (tracking_ids [B] of [T, N] int64, graphs [B] of graph.GraphData), per sample what graph.scene_graph returns
    for tracker files with the same boxes: pixel edges become tracker boxes (interactive.edges_to_tracker), the rest is
    graph.scene_graph_from_boxes."""
    from .interactive import edges_to_tracker
    T = tr.ids.shape[2]
    tracking_ids, graphs = [], []
    for b in range(tr.ids.shape[0]):
        N = int(tr.count[b])
        if N == 0:
            raise ValueError(f"sample {b} has no object that is linked in every frame")
        box = edges_to_tracker(tr.boxes[b, :N].numpy(), size)
        t, g = scene_graph_from_boxes(box, tr.ids[b, :N].numpy().astype(np.int64), size, num_input_frames, T, lambda_traj)
        tracking_ids.append(t)
        graphs.append(g)
    return tracking_ids, graphs


def tracked_batch(frames_u8, labels_u8, instance_i32, target_occ_u8, target_flow_hwc, num_input_frames, input_occ_u8=None,
                  input_flow_hwc=None, lambda_traj=1, config=None, size=None, antialias=False, **track_kw):
    """data.assemble_batch without tracker files: its inputs minus tracking_gnn (decoded arrays on the device) plus
    num_input_frames -> the same batch dict, with `tracking_gnn` built from the instance maps and the batch's own flows
    (track_instances on instance_mask, target_bw_of and input_of), `tracking_mask` [B,1,T,H,W] (graph.tracking_mask per sample)
    and `tracks` (the Tracks).  config: the run's configuration, checked by check_config.  size, antialias: as assemble_batch
    (arrays at dataset resolution are resized on the device first).  track_kw: track_instances."""
    from .data import assemble_batch
    if config is not None:
        check_config(config)
    batch = assemble_batch(frames_u8, labels_u8, instance_i32, target_occ_u8, target_flow_hwc, None, input_occ_u8,
                           input_flow_hwc, size=size, antialias=antialias)
    inst = batch["instance_mask"]
    tr = track_instances(inst, num_input_frames, batch["target_bw_of"], batch["input_of"], **track_kw)
    tracking_ids, graphs = scene_graphs(tr, tuple(inst.shape[-2:]), num_input_frames, lambda_traj)
    batch["tracking_gnn"] = collate_graphs(graphs).to(inst.device)
    batch["tracking_mask"] = torch.stack([tracking_mask(inst[b], tracking_ids[b]) for b in range(inst.shape[0])], 0)
    batch["tracks"] = tr
    return batch
