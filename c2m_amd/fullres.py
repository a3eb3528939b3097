"""Click-to-move results at dataset resolution, on the GPU.

Inputs may arrive at dataset resolution and are resized to the model's working size on the device (data.resize_frames); this
module goes back the other way.  The model already predicts what a full-size result needs: a backward flow from every
predicted frame to the last input frame (dense_motion_bw) and where that flow is valid (occlusion_bw).  The last input frame
exists at full resolution and it is sharp, so its pixels are moved with the flow, and the generator's working-size output
supplies only what warping cannot: disoccluded regions and appearance changes (ops.detail_warp, csrc/detail_warp.hip; DESIGN.md
4.2g has the definition).

    upscale           one dict of model.inference / click_to_move  -> uint8 [B,T,H,W,3] (+ instance ids [B,T,H,W])
    upscale_rollout   the dict of interactive.rollout, every segment warped from the last full-size frame of the one before

Everything stays on the device; nothing here is differentiable."""
import torch

from . import ops
from .interactive import FLOW_OCC
from .modules.layers.common import fold_time, unfold_time


def upscale(out, video, frame_hr_u8, num_input_frames, ids_hr=None, flow="dense_motion_bw", occ_threshold=None, fill_id=0):
    """The T predicted frames of `out` at the size of frame_hr_u8.

    out: the dict of model.inference (generated, the flow and its occlusion map are read); video [B,3,T',h,w]: the model's
    input, of which frame num_input_frames - 1 is read; frame_hr_u8 [B,H,W,3] uint8: that same frame at the output size, the
    layout data.resize_frames reads; ids_hr [B,H,W] int32 or None: its instance ids, carried along unblended (fill_id where
    the enlarged occlusion map is below occ_threshold).  flow: "dense_motion_bw", the flow `generated` was drawn with, or
    "sparse_motion_bw"; the occlusion map is the one that belongs to it (interactive.FLOW_OCC).
    Returns (uint8 [B,T,H,W,3], int32 [B,T,H,W] or None)."""
    if flow not in FLOW_OCC:
        raise ValueError(f"flow must be one of {sorted(FLOW_OCC)}, got {flow!r}")
    last = int(num_input_frames) - 1
    if video.dim() != 5 or not 0 <= last < video.shape[2]:
        raise ValueError(f"video must be [B,3,T,h,w] with T >= num_input_frames={num_input_frames}, got {tuple(video.shape)}")
    gen, f = out["generated"], out[flow]
    for name, t in (("generated", gen), ("video", video)):
        if tuple(f.shape[-2:]) != tuple(t.shape[-2:]):
            raise ValueError(f"{flow} is {tuple(f.shape[-2:])} but {name} is {tuple(t.shape[-2:])}: flows and frames at "
                             "different sizes (common_params.scale_factor != 1) are not supported yet")
    T = f.shape[2]
    with torch.no_grad():
        frame = video[:, :, last]
        b, c, h, w = frame.shape
        rep = frame.unsqueeze(0).expand(T, b, c, h, w).reshape(T * b, c, h, w)          # the frame _generate warps
        warped = unfold_time(ops.flow_warp(rep, fold_time(f)), T)
        return ops.detail_warp(frame_hr_u8, gen, warped, f, out[FLOW_OCC[flow]], ids_hr, occ_threshold, fill_id)


def upscale_rollout(r, video, frame_hr_u8, num_input_frames, ids_hr=None, flow="dense_motion_bw", occ_threshold=None,
                    fill_id=0):
    """The K * T frames of interactive.rollout at the size of frame_hr_u8.

    Segment 0 is warped from frame_hr_u8 and video, as upscale does.  Segment k > 0 started from the last frame of segment
    k - 1, so it is warped from the last full-size frame this function produced for that segment, whose working-size partner
    is r["generated"][:, :, k * T - 1]; ids_hr is carried the same way.
    Returns (uint8 [B,K*T,H,W,3], int32 [B,K*T,H,W] or None)."""
    frames, ids = [], []
    for k, out in enumerate(r["outputs"]):
        if k == 0:
            fr, idk = upscale(out, video, frame_hr_u8, num_input_frames, ids_hr, flow, occ_threshold, fill_id)
        else:
            T = frames[-1].shape[1]
            fr, idk = upscale(out, r["generated"][:, :, k * T - 1:k * T], frames[-1][:, -1],
                              1, None if ids_hr is None else ids[-1][:, -1], flow, occ_threshold, fill_id)
        frames.append(fr)
        ids.append(idk)
    return torch.cat(frames, 1), None if ids_hr is None else torch.cat(ids, 1)
