"""Label maps and instance maps from the heads of a Panoptic-DeepLab network, on the GPU.

The reference produces the `_ssmask` and `_gtFine_instanceIds` images its loader reads with its vendored Panoptic-DeepLab
(panoptic_deeplab/tools/generate_segmentation.py): a plain-torch network emits three heads at frame size -- semantic logits,
a centre heat map and a (dy, dx) offset field -- and a post-processing step (segmentation/model/post_processing) turns them into
the two images, one frame at a time, with host loops over instances and classes.  This module is that post-processing step for
a whole clip in one call (ops.panoptic_maps, csrc/panoptic.hip; DESIGN.md 4.2i has the contract).  The network itself is
ordinary torch and is not part of this package: run it under PyTorch-ROCm and hand its `semantic`, `center` and `offset`
outputs (after its own _upsample_predictions, i.e. at frame size) to panoptic_maps.

    panoptic_maps   heads of N frames -> semantic uint8, instance int32, panoptic int32 [N,H,W], centers, center_count
    clip_maps       the same as the (labels_u8, instance_i32) pair of a [B,T] clip that tracking.tracked_batch and
                    data.assemble_batch take, cropped from the padded 32k+1 frame the network ran on

Where that network (or its checkpoint) is not to be had, instance ids come from the label maps alone -- Cityscapes gtFine, KITTI
semantic maps, the `semantic` output of any segmenter, the label maps interactive.rollout carries forward -- by connected
components of the thing classes (ops.semantic_instances, csrc/components.hip):

    semantic_instances   labels of N frames -> instance int32 [N,H,W] in the same encoding, count, dropped, components
    clip_instances       the same as the (labels_u8, instance_i32) pair of a [B,T] clip

What it cannot do: two touching objects of one class are ONE component and get one id.  The centre and offset heads can tell them
apart, connected components cannot; panoptic_maps stays the better producer wherever its network is available.

Everything stays on the device; nothing here is differentiable."""
import torch

from . import ops

# POST_PROCESSING of panoptic_deeplab/configs/cityscapes_valset.yaml + the Cityscapes meta data of the reference
CITYSCAPES = dict(thing_list=(11, 12, 13, 14, 15, 16, 17, 18), label_divisor=1000, stuff_area=2048, ignore_label=255,
                  threshold=0.1, nms_kernel=7, top_k=200)


def panoptic_maps(semantic, center, offset, **params):
    """semantic: fp32 logits [N,C,H,W], or labels already taken, uint8 / int64 [N,H,W]; center [N,1,H,W] and offset [N,2,H,W]
    (dy, dx) fp32, all at frame size.  Keyword parameters default to CITYSCAPES: thing_list, label_divisor, stuff_area,
    ignore_label (void = ignore_label * label_divisor), threshold, nms_kernel, top_k.

    Returns a dict of device tensors: "semantic" uint8 [N,H,W] (argmax, first maximum), "panoptic" int32 [N,H,W]
    (class * label_divisor + n on things, class * label_divisor on stuff of at least stuff_area pixels, void elsewhere),
    "instance" int32 [N,H,W] (the panoptic value on things, the class on stuff, ignore_label on void: the instance-id image the
    loader reads), "centers" int32 [N,top_k,2] (y, x) in row-major order, zero past "center_count" int32 [N]."""
    unknown = set(params) - set(CITYSCAPES)
    if unknown:
        raise TypeError(f"panoptic_maps got unknown parameter(s) {sorted(unknown)}; known: {sorted(CITYSCAPES)}")
    return ops.panoptic_maps(semantic, center, offset, **{**CITYSCAPES, **params})


def clip_maps(semantic, center, offset, clip, crop=None, **params):
    """The maps of a clip: heads of N = B * T frames (sample-major) -> (labels_u8 [B,T,h,w] uint8, instance_i32 [B,T,h,w] int32),
    the two arrays tracking.tracked_batch and data.assemble_batch take.  clip = (B, T); crop = (h, w) keeps the top-left h x w
    pixels AFTER the computation, as the reference does with the padded frame it runs the network on (None: the whole frame)."""
    try:
        B, T = (int(v) for v in clip)
    except (TypeError, ValueError):
        raise ValueError(f"clip must be (B, T), got {clip!r}") from None
    if not isinstance(semantic, torch.Tensor) or B < 0 or T < 0 or semantic.shape[0] != B * T:
        raise ValueError(f"clip={clip!r} needs heads of {B * T} frames, got {tuple(getattr(semantic, 'shape', ()))}")
    H, W = semantic.shape[-2:]
    h, w = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"crop={crop!r} must lie inside the {H}x{W} frame")
    m = panoptic_maps(semantic, center, offset, **params)
    return (m["semantic"].view(B, T, H, W)[:, :, :h, :w].contiguous(),
            m["instance"].view(B, T, H, W)[:, :, :h, :w].contiguous())


INSTANCE_DEFAULTS = dict(thing_list=CITYSCAPES["thing_list"], label_divisor=CITYSCAPES["label_divisor"],
                         ignore_label=CITYSCAPES["ignore_label"], connectivity=8, min_area=1)


def semantic_instances(labels, **params):
    """labels: uint8 or int64 [N,H,W], values 0..255.  Keyword parameters: thing_list, label_divisor, ignore_label (default:
    CITYSCAPES), connectivity (8; or 4), min_area (1).

    Returns a dict of device tensors.  "instance" int32 [N,H,W], in the encoding of panoptic_maps()["instance"] and the loader:
    class * label_divisor + n on a thing component that is kept, ignore_label on pixels labelled so, the class everywhere else
    (stuff, thing components of fewer than min_area pixels, thing components past the cap).  n = 1, 2, ... counts the KEPT
    components of the class in the image by ascending first raster pixel and stays below label_divisor.  "count" and "dropped"
    int32 [N, len(thing_list)]: the kept components, and those of at least min_area pixels the cap left out.  "components" int32
    [N,H,W]: ops.connected_components of the labels (at every pixel the index y * W + x of its component's first pixel).

    Two touching objects of one class are one component: connected components cannot separate them (see the module text)."""
    unknown = set(params) - set(INSTANCE_DEFAULTS)
    if unknown:
        raise TypeError(f"semantic_instances got unknown parameter(s) {sorted(unknown)}; known: {sorted(INSTANCE_DEFAULTS)}")
    return ops.semantic_instances(labels, **{**INSTANCE_DEFAULTS, **params})


def clip_instances(labels, clip, crop=None, **params):
    """The instance maps of a clip from its label maps: labels of N = B * T frames (sample-major), uint8 or int64 [N,H,W] ->
    (labels_u8 [B,T,h,w] uint8, instance_i32 [B,T,h,w] int32), the two arrays tracking.tracked_batch and data.assemble_batch
    take.  clip = (B, T); crop = (h, w) keeps the top-left h x w pixels BEFORE the labelling (None: the whole frame): there is
    no padded network frame here, and the objects are those of the visible frame."""
    try:
        B, T = (int(v) for v in clip)
    except (TypeError, ValueError):
        raise ValueError(f"clip must be (B, T), got {clip!r}") from None
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or B < 0 or T < 0 or labels.shape[0] != B * T:
        raise ValueError(f"clip={clip!r} needs labels [N,H,W] of {B * T} frames, got {tuple(getattr(labels, 'shape', ()))}")
    if labels.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"labels must be uint8 or int64, got {labels.dtype}")
    H, W = labels.shape[-2:]
    h, w = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"crop={crop!r} must lie inside the {H}x{W} frame")
    visible = labels[:, :h, :w]
    visible = (visible if visible.dtype == torch.uint8 else visible.to(torch.uint8)).contiguous()
    m = semantic_instances(visible, **params)
    return visible.view(B, T, h, w), m["instance"].view(B, T, h, w)
