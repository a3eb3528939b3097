"""Pictures of what the model returns, rendered on the device (csrc/render.hip): the reference's tensor2im / tensor2occ /
tensor2flow / compute_flow_color_map value rules as uint8 sheets, and `storyboard`, one call for a click_to_move or
rollout result.  Only the uint8 sheets cross to the host (a quarter of the bytes of the fp32 tensors they show).

A sheet is uint8 [T, rows*H, cols*W, C]: sample b in cell (b // cols, b % cols) of size = [rows, cols], the reference's
`merge`; one-channel sheets drop the channel axis, as `merge` does."""
import numpy as np
import torch

from . import ops

DEFAULT_SIZE = (8, 4)                       # the reference's default grid (utils/utils.py:46-72)
PANELS = ("generated", "instances", "dense_motion_bw", "occlusion_bw")
BOX_COLOR = (255, 0, 0)                     # the reference's draw_bbox colour
PATH_COLOR = (255, 255, 0)


def _size(size):
    rows, cols = DEFAULT_SIZE if size is None else size
    return int(rows), int(cols)


def _drop_single_channel(sheet):
    return sheet[..., 0] if sheet.shape[-1] == 1 else sheet


def tensor2im(x, normalize=False, size=None):
    """Frames [B,C,T,H,W] in [0, 1] (normalize: [-1, 1]) -> uint8 [T, rows*H, cols*W, C] on the device, the reference's
    tensor2im array ([T, rows*H, cols*W] for C = 1)."""
    return _drop_single_channel(ops.render_frames(x, _size(size), normalize))


def tensor2occ(x, size=None):
    """Occlusion maps [B,1,T,H,W] in [0, 1] -> uint8 [T, rows*H, cols*W] on the device, the reference's tensor2occ array."""
    return _drop_single_channel(ops.render_frames(x, _size(size), False))


def tensor2flow(x, size):
    """Flows [B,2,T,H,W] -> uint8 RGB [T, rows*H, cols*W, 3] in the Middlebury colour code, every frame's sheet normalised by
    its own largest radius over all samples: the reference's tensor2flow array."""
    return ops.render_flow(x, _size(size), None)


def flow_color_map(x, scale=3.0, size=None):
    """Flows [B,2,T,H,W] -> uint8 RGB sheet with the fixed scale of the reference's compute_flow_color_map (save_flows):
    cell b, frame t is compute_flow_color_map(x[b, :, t]).  size None: the samples side by side, [1, B]."""
    return ops.render_flow(x, (1, max(int(x.shape[0]), 1)) if size is None else _size(size), float(scale))


def default_palette(n=32):
    """n well separated RGB colours, uint8 [n, 3] (a fixed table: golden-angle hues at two brightness levels)."""
    k = np.arange(n)
    h = (k * 0.61803398875) % 1.0 * 6.0
    v = np.where(k % 2 == 0, 255.0, 170.0)
    x = v * (1 - np.abs(h % 2 - 1))
    z = np.zeros(n)
    sel = h.astype(int) % 6
    r = np.choose(sel, [v, x, z, z, x, v])
    g = np.choose(sel, [x, v, v, x, z, z])
    b = np.choose(sel, [z, z, x, v, v, x])
    return torch.from_numpy(np.stack([r, g, b], -1).astype(np.uint8))


def _as_rgb(sheet):
    return sheet if sheet.shape[-1] == 3 else sheet.expand(*sheet.shape[:-1], 3)


def _segment_overlays(targets, boxes, presence, B, T):
    """Primitive tables of one segment: the predicted boxes of the dragged objects and the requested path of every drag."""
    per_sample = [[g for g in targets if g.sample == b] for b in range(B)]
    N = max([len(p) for p in per_sample] + [1])
    bx = torch.zeros(B, N, T, 4, dtype=torch.int32)
    pr = torch.zeros(B, N, T, dtype=torch.bool)
    if boxes is not None:
        for b, tg in enumerate(per_sample):
            for n, g in enumerate(tg):
                bx[b, n] = torch.as_tensor(np.asarray(boxes[b][g.node])).to(torch.int32)
                pr[b, n] = torch.as_tensor(np.asarray(presence[b][g.node])).bool()
    D = len(targets)
    pts = np.zeros((D, T + 1, 2), np.int32)
    for d, g in enumerate(targets):
        e = np.concatenate([np.asarray(g.start, np.float64)[None], np.asarray(g.edges, np.float64)], 0)
        if e.shape[0] != T + 1:
            raise ValueError(f"targets: drag {d} holds {e.shape[0] - 1} frames but the segment holds {T}")
        pts[d, :, 0] = np.floor((e[:, 0] + e[:, 2]) / 2)
        pts[d, :, 1] = np.floor((e[:, 1] + e[:, 3]) / 2)
    count = np.tile(np.arange(2, T + 2, dtype=np.int32), (D, 1))
    sample = np.array([g.sample for g in targets], np.int32)
    return bx, pr, torch.from_numpy(pts), torch.from_numpy(sample), torch.from_numpy(count)


def storyboard(result, video=None, panels=PANELS, cols=None, maps=None, boxes=None, presence=None, targets=None, overlays=True,
               palette=None, alpha=128, id_range=(1000, 19000), box_color=BOX_COLOR, path_color=PATH_COLOR, flow_scale=None):
    """One picture per predicted frame of what interactive.click_to_move or interactive.rollout returned: the chosen
    panels stacked vertically, the samples side by side -> uint8 [frames, len(panels)*H, cols*W, 3] on the device.

    result: the dict of rollout (frames of all segments in order; its instance_mask, boxes, presence and targets are used),
    or the dict of click_to_move / model.inference with maps = the dict of propagate_maps for the "instances" panel and
    boxes / presence (predicted_boxes) and targets (drag_targets) for the overlays.  panels: keys of the output dict --
    three-channel ones are frames, one-channel ones maps in [0, 1], two-channel ones flows (normalised per frame over the
    samples; flow_scale s: fixed scale instead) -- plus "instances" (generated, the objects of id_range tinted with
    palette[id % P], their borders solid) and "source" (the first frame of `video`, repeated).  overlays: on the "generated"
    and "instances" panels the predicted boxes of the DRAGGED objects (box_color) and each drag's requested path so far
    with a marker on its current point (path_color), each segment's drags in its own frames.  cols: cells per row (B).
    Flows and frames at different sizes (common_params.scale_factor != 1) are not supported."""
    segs = result["outputs"] if "outputs" in result else [result]
    gen = result["generated"]
    B, _, F, H, W = gen.shape
    T = segs[0]["generated"].shape[2]
    cols = B if cols is None else int(cols)
    if cols < B:
        raise ValueError(f"cols = {cols} cells do not hold the B = {B} samples side by side")
    size = (1, cols)
    if "outputs" in result:
        maps = dict(instance_mask=result["instance_mask"]) if maps is None else maps
        seg_boxes, seg_presence = result.get("boxes"), result.get("presence")
        seg_targets = result.get("targets") if targets is None else targets
    else:
        seg_boxes, seg_presence = (None if boxes is None else [boxes]), (None if presence is None else [presence])
        seg_targets = None if targets is None else [targets]
    if seg_targets is not None and len(seg_targets) != len(segs):
        raise ValueError(f"targets holds {len(seg_targets)} segments, the result {len(segs)}")
    cat = lambda key: result[key] if "outputs" not in result else torch.cat([o[key] for o in segs], 2)
    base = None
    sheets = []
    for name in panels:
        if name in ("generated", "instances"):
            if base is None:
                base = ops.render_frames(gen, size)
            if name == "generated":
                sheet = base.clone() if overlays else base
            else:
                if maps is None:
                    raise ValueError("the \"instances\" panel needs maps = the dict of interactive.propagate_maps")
                inst = maps["instance_mask"]
                if tuple(inst.shape[-2:]) != (H, W):
                    raise ValueError(f"the instance maps are {tuple(inst.shape[-2:])} but the frames are {(H, W)}: flows and "
                                     "frames at different sizes (common_params.scale_factor != 1) are not supported yet")
                sheet = ops.render_instances(inst.to(torch.int32), size, default_palette() if palette is None else palette, base,
                                             id_range, alpha)
            if overlays and seg_targets is not None:
                for k, tg in enumerate(seg_targets):
                    if not tg:
                        continue
                    bx, pr, pts, smp, cnt = _segment_overlays(tg, None if seg_boxes is None else seg_boxes[k],
                                                              None if seg_presence is None else seg_presence[k], B, T)
                    ops.draw_overlays(sheet[k * T:(k + 1) * T], size, bx, pr,
                                      torch.tensor(box_color, dtype=torch.uint8).expand(B, bx.shape[1], 3).contiguous(), pts, smp,
                                      cnt, torch.tensor(path_color, dtype=torch.uint8).expand(len(tg), 3).contiguous())
        elif name == "source":
            if video is None:
                raise ValueError("the \"source\" panel needs video")
            sheet = ops.render_frames(video[:, :, :1].expand(-1, -1, F, -1, -1), size)
        else:
            x = cat(name)
            if x.dim() != 5 or x.shape[1] not in (1, 2, 3):
                raise ValueError(f"panel {name!r} is {tuple(x.shape)}: a panel is [B, C, T, H, W] with 1, 2 or 3 channels")
            if tuple(x.shape[-2:]) != (H, W):
                raise ValueError(f"panel {name!r} is {tuple(x.shape[-2:])} but the frames are {(H, W)}: flows and frames at "
                                 "different sizes (common_params.scale_factor != 1) are not supported yet")
            sheet = ops.render_flow(x, size, flow_scale) if x.shape[1] == 2 else ops.render_frames(x, size)
        sheets.append(_as_rgb(sheet))
    return torch.cat(sheets, 1)


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("c2m_amd.visual.save_png / save_gif need PIL (the Pillow package), which is not installed") from e
    return Image


def _host_u8(a, name):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError(f"{name} must be uint8, got {a.dtype}")
    return a


def save_png(path, image):
    """uint8 [H, W] or [H, W, 3] -> PNG file."""
    Image = _pil()
    image = _host_u8(image, "image")
    if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
        raise ValueError(f"image must be [H, W] or [H, W, 3], got {image.shape}")
    Image.fromarray(image).save(path, format="PNG")


def save_gif(path, frames, fps=None):
    """uint8 [T, H, W] or [T, H, W, 3] -> animated GIF; fps = len(frames) by default (the clip lasts a second), the reference's
    convention.  GIF holds 256 colours per frame: unlike save_png this is a preview, not a lossless copy."""
    Image = _pil()
    frames = _host_u8(frames, "frames")
    if frames.ndim not in (3, 4) or len(frames) == 0 or (frames.ndim == 4 and frames.shape[3] != 3):
        raise ValueError(f"frames must be [T, H, W] or [T, H, W, 3] with T >= 1, got {frames.shape}")
    fps = len(frames) if fps is None else fps
    if fps <= 0:
        raise ValueError(f"fps must be positive, got {fps}")
    ims = [Image.fromarray(f) for f in frames]
    ims[0].save(path, format="GIF", save_all=True, append_images=ims[1:], duration=max(int(round(1000.0 / fps)), 1), loop=0)
