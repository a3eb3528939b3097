"""Device-side batch assembly: the input-pipeline stage just upstream of the hot path.

Reference: src/datasets/cityscapes.py builds every sample on the CPU -- ToTensor of the frames (:30-33), the 20-channel
one-hot split of the label-id map (:35-41), instance ids (:43-52), occlusion PNG -> clip_mask (:212-216, 262-265), .flo
HWC -> CHW (:219-231) -- and src/train.py:23-38 collates.  Here the decoded arrays (what PIL / np.fromfile return, at
dataset resolution or already at input_size) are uploaded as they are (uint8 / int32 / float32), resized on the device
where asked (`size=`: resize_frames is Pillow's BICUBIC and resize_maps its NEAREST bit for bit, resize_flow is
transforms.Resize on the .flo tensor times size[0] / h; csrc/resize.hip) and expanded by three small kernels; the result is
the batch dict `GeneratorFullModel.forward` consumes.  Only file decoding stays on the host."""
import torch

from . import _lib
from . import ops
from .ops import _p, _stream


def _u8(t, name):
    if t.dtype != torch.uint8:
        raise TypeError(f"{name} must be uint8 (decoded image data)")
    ops._hip_only(t)
    return t.contiguous()


def prep_video(frames_u8):
    """[B,T,H,W,3] uint8 -> video [B,3,T,H,W] float32 in [0,1] (ToTensor + stack over time, cityscapes.py:30-33,59-61)."""
    frames_u8 = _u8(frames_u8, "frames")
    B, T, H, W, C = frames_u8.shape
    if C != 3:
        raise ValueError("frames must be [B,T,H,W,3]")
    out = torch.empty(B, 3, T, H, W, device=frames_u8.device, dtype=torch.float32)
    _lib.check(_lib.lib().c2m_prep_video(_p(frames_u8), _p(out), B, T, H, W, _stream()), "prep_video")
    return out


def prep_seg_onehot(labels_u8):
    """[B,T,H,W] uint8 label ids -> (bg_mask [B,11,T,H,W], fg_mask [B,9,T,H,W]) (cityscapes.py:35-41,62-70)."""
    labels_u8 = _u8(labels_u8, "labels")
    B, T, H, W = labels_u8.shape
    bg = torch.empty(B, 11, T, H, W, device=labels_u8.device, dtype=torch.float32)
    fg = torch.empty(B, 9, T, H, W, device=labels_u8.device, dtype=torch.float32)
    _lib.check(_lib.lib().c2m_prep_seg_onehot(_p(labels_u8), _p(bg), _p(fg), B, T, H, W, _stream()), "prep_seg_onehot")
    return bg, fg


def prep_flow_occ(occ_u8, flow_hwc):
    """occlusion PNGs [B,T,H,W] uint8 and .flo arrays [B,T,H,W,2] float32 -> (target_bw_occ [B,1,T,H,W],
    target_bw_of [B,2,T,H,W]) (cityscapes.py:212-231,254-265).  Either input may be None."""
    ref = occ_u8 if occ_u8 is not None else flow_hwc
    ops._hip_only(ref)
    B, T, H, W = ref.shape[:4]
    occ = flow = None
    if occ_u8 is not None:
        occ_u8 = _u8(occ_u8, "occlusion")
        occ = torch.empty(B, 1, T, H, W, device=ref.device, dtype=torch.float32)
    if flow_hwc is not None:
        ops._hip_only(flow_hwc)
        if flow_hwc.dtype != torch.float32 or tuple(flow_hwc.shape) != (B, T, H, W, 2):
            raise ValueError("flow must be float32 [B,T,H,W,2]")
        flow_hwc = flow_hwc.contiguous()
        flow = torch.empty(B, 2, T, H, W, device=ref.device, dtype=torch.float32)
    _lib.check(_lib.lib().c2m_prep_flow_occ(_p(occ_u8), _p(flow_hwc), _p(occ), _p(flow), B, T, H, W, _stream()),
               "prep_flow_occ")
    return occ, flow


def _size(size):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (h, w), got {size!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"size must be positive, got {size!r}")
    return h, w


def _resize(x, name, dtypes, tail, size, run):
    """Shared front of the three resizes: x is [..., H, W] + tail dims; checks first, then one launch on the flattened batch."""
    if not torch.is_tensor(x) or x.dtype not in dtypes:
        raise TypeError(f"{name} must be a tensor of dtype {' or '.join(str(d) for d in dtypes)}")
    ops._hip_only(x)
    h, w = _size(size)
    cut = x.dim() - len(tail)                                  # [..., H, W] ends here
    if cut < 2 or any(c not in ok for c, ok in zip(x.shape[cut:], tail)):
        raise ValueError(f"{name} must be [..., H, W{''.join(', ' + '|'.join(map(str, ok)) for ok in tail)}], got "
                         f"{tuple(x.shape)}")
    lead, (H, W), rest = x.shape[:cut - 2], x.shape[cut - 2:cut], x.shape[cut:]
    if (H, W) == (h, w):
        return x                                              # already at size: no launch
    if x.numel() == 0:
        if H < 1 or W < 1:
            raise ValueError(f"{name} has an empty image: {tuple(x.shape)}")
        return x.new_empty(*lead, h, w, *rest)
    return run(x.contiguous().reshape(-1, H, W, *rest), (h, w)).reshape(*lead, h, w, *rest)


def resize_frames(frames_u8, size, filter="bicubic"):
    """[..., H, W, C] uint8 (C in {1, 3}, HWC as PIL decodes it) -> [..., h, w, C] with size = (h, w): what
    Image.resize((w, h), BICUBIC) returns (cityscapes.py:23,33), bit for bit; filter 'bilinear' is Pillow's BILINEAR."""
    if filter not in ("bicubic", "bilinear"):
        raise ValueError(f"filter must be 'bicubic' or 'bilinear', got {filter!r} (LANCZOS is not supported)")
    return _resize(frames_u8, "frames", (torch.uint8,), ((1, 3),), size, lambda x, s: ops.resize_u8(x, s, filter))


def resize_maps(x, size):
    """[..., H, W] uint8 (label ids, occlusion) or int32 (instance ids) -> [..., h, w]: Image.resize((w, h), NEAREST)
    (cityscapes.py:26-33,211), bit for bit."""
    return _resize(x, "maps", (torch.uint8, torch.int32), (), size, ops.resize_nearest)


def resize_flow(flow_hwc, size, antialias=False):
    """[..., H, W, 2] float32 (the .flo layout) -> [..., h, w, 2]: transforms.Resize on the tensor times h / H on BOTH
    channels (cityscapes.py:220-222).  antialias=False: plain bilinear, align_corners=False (Resize on tensors in the
    torchvision of the reference's time); True: the triangle filter widened by the scale (torchvision >= 0.17)."""
    return _resize(flow_hwc, "flow", (torch.float32,), ((2,),), size, lambda x, s: ops.resize_flow(x, s, bool(antialias)))


def assemble_batch(frames_u8, labels_u8, instance_i32, target_occ_u8, target_flow_hwc, tracking_gnn,
                   input_occ_u8=None, input_flow_hwc=None, size=None, antialias=False):
    """The batch dict of model.py:124 from decoded arrays already on the device.  `instance_i32` [B,T,H,W] int32.
    size = (h, w): every array may be at dataset resolution and is resized first (resize_frames / resize_maps / resize_flow
    with `antialias`); None: the arrays are at input_size already."""
    if size is not None:
        fl = lambda t: None if t is None else resize_flow(t, size, antialias)
        mp = lambda t: None if t is None else resize_maps(t, size)
        frames_u8, labels_u8, instance_i32 = resize_frames(frames_u8, size), mp(labels_u8), mp(instance_i32.to(torch.int32))
        target_occ_u8, input_occ_u8, target_flow_hwc, input_flow_hwc = mp(target_occ_u8), mp(input_occ_u8), \
            fl(target_flow_hwc), fl(input_flow_hwc)
    bg, fg = prep_seg_onehot(labels_u8)
    occ, flow = prep_flow_occ(target_occ_u8, target_flow_hwc)
    batch = dict(video=prep_video(frames_u8), bg_mask=bg, fg_mask=fg,
                 instance_mask=instance_i32.to(torch.int32).unsqueeze(1).contiguous(), tracking_gnn=tracking_gnn,
                 target_bw_of=flow, target_bw_occ=occ, input_of=None, input_occ=None)
    if input_flow_hwc is not None:
        batch["input_occ"], batch["input_of"] = prep_flow_occ(input_occ_u8, input_flow_hwc)
    return batch
