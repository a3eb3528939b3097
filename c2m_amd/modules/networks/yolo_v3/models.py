"""The YOLOv3 detector of the evaluator (reference: src/modules/networks/yolo_v3/models.py), inference only.

Same attribute layout as the reference's `Darknet` -- `module_list.{i}.conv_{i}.weight`, `module_list.{i}.batch_norm_{i}.*` -- so
a state_dict moves between the two with strict=True in either direction, and the same darknet `.weights` file layout.
The architecture is restated here as a table (`yolov3_blocks`); `Darknet(config=path_or_list)` builds any net from the same
block kinds out of a darknet cfg text, read by `parse_config`.

Forward: fp32, under no_grad, convolutions on `ops.conv` with the leaky slope 0.1 fused; eval-mode batch-norm is folded into
weight and bias (float64 arithmetic, rounded to fp32 once) and refolded only when a parameter or statistic changes.  Returns the
raw head maps [N, A*(5+C), g, g]; decoding is `ops.yolo_candidates`."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import ops

YOLOV3_ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
LEAKY_SLOPE = 0.1


def _conv(filters, size, stride=1, bn=True, leaky=True):
    d = {"type": "convolutional", "filters": filters, "size": size, "stride": stride, "pad": 1,
         "activation": "leaky" if leaky else "linear"}
    if bn:
        d["batch_normalize"] = 1
    return d


def yolov3_blocks(num_classes=80, channels=3, size=416):
    """[net] block + the 107 blocks of YOLOv3: Darknet-53 (1, 2, 8, 8, 4 residual pairs behind stride-2 convolutions), then
    three detection branches at strides 32, 16, 8; the second and third start from a 1x1 convolution of the branch before,
    upsampled x2 and concatenated with the backbone's stride-16 / stride-8 output (blocks 61 and 36)."""
    blocks = [{"type": "net", "channels": channels, "height": size, "width": size}]
    blocks.append(_conv(32, 3))
    for width, repeats in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        blocks.append(_conv(width, 3, stride=2))
        for _ in range(repeats):
            blocks += [_conv(width // 2, 1), _conv(width, 3), {"type": "shortcut", "from": -3, "activation": "linear"}]
    out = 3 * (5 + num_classes)
    anchors = ",".join(f"{w},{h}" for w, h in YOLOV3_ANCHORS)
    for width, mask, skip in ((512, "6,7,8", None), (256, "3,4,5", 61), (128, "0,1,2", 36)):
        if skip is not None:
            blocks += [{"type": "route", "layers": "-4"}, _conv(width, 1), {"type": "upsample", "stride": 2},
                       {"type": "route", "layers": f"-1,{skip}"}]
        for _ in range(3):
            blocks += [_conv(width, 1), _conv(2 * width, 3)]
        blocks.append(_conv(out, 1, bn=False, leaky=False))
        blocks.append({"type": "yolo", "mask": mask, "anchors": anchors, "classes": num_classes, "num": 9})
    return blocks


def parse_config(text_or_path):
    """darknet cfg text, or the path of a file holding it -> list of blocks, the first being [net].  A string with a line break
    in it is cfg text (no cfg fits one line: it has a [net] block and a layer); anything else is a path and is opened.
    `[kind]` opens a block, `key = value` lines fill it, `#` and `;` start comments.  Values stay strings; the builder converts
    what it reads."""
    text = os.fspath(text_or_path)
    if "\n" not in text:
        with open(text, "r") as f:
            text = f.read()
    blocks = []
    for n, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith("["):
            if not line.endswith("]"):
                raise ValueError(f"cfg line {n}: unterminated block header {raw!r}")
            blocks.append({"type": line[1:-1].strip()})
        else:
            if "=" not in line or not blocks:
                raise ValueError(f"cfg line {n}: expected key=value inside a block, got {raw!r}")
            k, v = line.split("=", 1)
            blocks[-1][k.strip()] = v.strip()
    if not blocks or blocks[0]["type"] != "net":
        raise ValueError("a cfg starts with a [net] block")
    return blocks


def _ints(v):
    return [int(s) for s in str(v).split(",") if s.strip() != ""]


class _Mark(nn.Module):
    """Parameterless stand-in for the layers the forward pass runs itself (route, shortcut, upsample, maxpool, yolo, leaky)."""

    def __init__(self, **kw):
        super().__init__()
        self.__dict__.update(kw)


class Darknet(nn.Module):
    def __init__(self, config=None, img_size=416):
        super().__init__()
        blocks = yolov3_blocks() if config is None else parse_config(config) if isinstance(config, (str, os.PathLike)) \
            else [dict(b) for b in config]
        if not blocks or blocks[0].get("type") != "net":
            raise ValueError("the block list starts with a [net] block")
        self.hyperparams = dict(blocks[0])
        self.module_defs = [dict(b) for b in blocks[1:]]
        self.img_size = img_size
        self.seen = 0
        self.header_info = np.array([0, 0, 0, self.seen, 0], dtype=np.int32)
        self.module_list = nn.ModuleList()
        filters_out = []
        prev = int(self.hyperparams.get("channels", 3))
        self.heads = []                                      # (block index, anchors [(w, h)], classes)
        for i, d in enumerate(self.module_defs):
            seq, kind = nn.Sequential(), d["type"]
            if kind == "convolutional":
                bn = int(d.get("batch_normalize", 0))
                filters, k, stride = int(d["filters"]), int(d["size"]), int(d.get("stride", 1))
                act = d.get("activation", "linear")
                if act not in ("leaky", "linear"):
                    raise NotImplementedError(f"block {i}: activation {act!r}")
                seq.add_module(f"conv_{i}", nn.Conv2d(prev, filters, k, stride=stride, padding=(k - 1) // 2, bias=not bn))
                if bn:
                    seq.add_module(f"batch_norm_{i}", nn.BatchNorm2d(filters, momentum=0.9, eps=1e-5))
                if act == "leaky":
                    seq.add_module(f"leaky_{i}", _Mark())
            elif kind == "maxpool":
                k, stride = int(d["size"]), int(d["stride"])
                if k == 2 and stride == 1:
                    seq.add_module(f"_debug_padding_{i}", _Mark())
                seq.add_module(f"maxpool_{i}", _Mark(kernel=k, stride=stride))
                filters = prev
            elif kind == "upsample":
                if int(d["stride"]) != 2:
                    raise NotImplementedError(f"block {i}: upsample x{d['stride']}")
                seq.add_module(f"upsample_{i}", _Mark())
                filters = prev
            elif kind == "route":
                src = _ints(d["layers"])
                if not 1 <= len(src) <= 2:
                    raise NotImplementedError(f"block {i}: route with {len(src)} sources")
                for s in src:
                    if not -i <= s < i:
                        raise ValueError(f"block {i}: route source {s} does not exist")
                filters = sum(filters_out[s] for s in src)
                seq.add_module(f"route_{i}", _Mark())
            elif kind == "shortcut":
                s = int(d["from"])
                if not -i <= s < i:
                    raise ValueError(f"block {i}: shortcut source {s} does not exist")
                filters = filters_out[s]
                seq.add_module(f"shortcut_{i}", _Mark())
            elif kind == "yolo":
                flat = _ints(d["anchors"])
                pairs = [(flat[j], flat[j + 1]) for j in range(0, len(flat), 2)]
                anchors = [pairs[j] for j in _ints(d["mask"])]
                classes = int(d["classes"])
                if prev != len(anchors) * (5 + classes):
                    raise ValueError(f"block {i}: a yolo layer with {len(anchors)} anchors and {classes} classes reads "
                                     f"{len(anchors) * (5 + classes)} channels, the block before it gives {prev}")
                seq.add_module(f"yolo_{i}", _Mark())
                self.heads.append((i, anchors, classes))
                filters = prev
            else:
                raise NotImplementedError(f"block {i}: kind {kind!r}")
            self.module_list.append(seq)
            filters_out.append(filters)
            prev = filters
        if not self.heads:
            raise ValueError("the net has no yolo layer")
        if len({c for _, _, c in self.heads}) != 1:
            raise ValueError("the yolo layers disagree on the number of classes")
        self._folded = {}

    @property
    def num_classes(self):
        return self.heads[0][2]

    @property
    def anchors(self):
        return [a for _, a, _ in self.heads]

    # ---- darknet weights files: 5 int32, then per convolution (bn bias, weight, mean, var | conv bias), conv weight; float32
    def _conv_tensors(self, cutoff=None):
        for i, (d, m) in enumerate(zip(self.module_defs, self.module_list)):
            if cutoff is not None and i >= cutoff:
                break
            if d["type"] != "convolutional":
                continue
            conv = m[0]
            if conv.bias is None:
                bn = m[1]
                yield from (bn.bias, bn.weight, bn.running_mean, bn.running_var)
            else:
                yield conv.bias
            yield conv.weight

    def load_darknet_weights(self, weights_path):
        """Raises unless the file holds exactly the floats this net reads (a `darknet53.conv.74` backbone file fills the
        first 75 blocks and may be as long as it likes, as in the reference)."""
        with open(weights_path, "rb") as f:
            header = np.fromfile(f, dtype=np.int32, count=5)
            weights = np.fromfile(f, dtype=np.float32)
        if header.size != 5:
            raise ValueError(f"{weights_path}: shorter than the 5-int header")
        backbone = "darknet53.conv.74" in str(weights_path)
        tensors = list(self._conv_tensors(75 if backbone else None))
        need = sum(t.numel() for t in tensors)
        if weights.size < need or (weights.size != need and not backbone):
            raise ValueError(f"{weights_path}: the file holds {weights.size} floats, this net reads {need}")
        self.header_info = header
        self.seen = header[3]
        ptr = 0
        with torch.no_grad():
            for t in tensors:
                n = t.numel()
                t.copy_(torch.from_numpy(weights[ptr:ptr + n].copy()).view_as(t))
                ptr += n
        return ptr

    def save_darknet_weights(self, path, cutoff=-1):
        self.header_info[3] = self.seen
        with open(path, "wb") as fp:
            self.header_info.tofile(fp)
            stop = len(self.module_defs) + cutoff if cutoff < 0 else cutoff      # the reference's [:cutoff]: -1 drops the last
            for t in self._conv_tensors(stop):                                   # block, which is a yolo layer
                t.detach().cpu().numpy().tofile(fp)

    # ---- forward
    def refold(self):
        """Forget the folded weights; the next forward folds again.  Needed only after an edit the version counters do not see
        (see _fold)."""
        self._folded.clear()

    def _fold(self, i):
        """(weight, bias) of convolution i with its eval-mode batch-norm folded in, cached per (storage, version) of every
        tensor read.  load_state_dict, load_darknet_weights, .to(), optimizers and in-place ops on the parameter all change one
        of the two.  An in-place edit THROUGH `.data` (`bn.weight.data.mul_(2)`) changes neither -- autograd's counter belongs to
        the tensor it is called on -- and leaves a stale fold: call refold() after such an edit."""
        m = self.module_list[i]
        conv = m[0]
        if conv.bias is not None:
            return conv.weight, conv.bias
        bn = m[1]
        src = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = tuple((t.data_ptr(), t._version) for t in src)
        hit = self._folded.get(i)
        if hit is None or hit[0] != key:
            w, g, b, mu, var = (t.detach().double() for t in src)
            scale = g / torch.sqrt(var + bn.eps)
            hit = (key, (w * scale.view(-1, 1, 1, 1)).float().contiguous(), (b - mu * scale).float().contiguous())
            self._folded[i] = hit
        return hit[1], hit[2]

    def forward(self, x):
        if self.training:
            raise RuntimeError("Darknet is inference only here: call .eval() (batch-norm uses its running statistics)")
        if x.dim() != 4 or x.shape[1] != int(self.hyperparams.get("channels", 3)):
            raise ValueError(f"input must be [N,{self.hyperparams.get('channels', 3)},H,W], got {tuple(x.shape)}")
        outs, heads = [], []
        with torch.no_grad(), ops.conv_precision("fp32"):
            x = x.float()
            for i, d in enumerate(self.module_defs):
                kind = d["type"]
                if kind == "convolutional":
                    conv = self.module_list[i][0]
                    w, b = self._fold(i)
                    leaky = d.get("activation", "linear") == "leaky"
                    x = ops.conv(x, w, b, stride=conv.stride[0], padding=conv.padding[0], act="lrelu" if leaky else None,
                                 slope=LEAKY_SLOPE)
                elif kind == "upsample":
                    x = F.interpolate(x, scale_factor=2, mode="nearest")
                elif kind == "maxpool":
                    k, stride = int(d["size"]), int(d["stride"])
                    if k == 2 and stride == 1:
                        x = F.pad(x, (0, 1, 0, 1))
                    x = F.max_pool2d(x, k, stride, (k - 1) // 2)
                elif kind == "route":
                    src = _ints(d["layers"])
                    x = outs[src[0]] if len(src) == 1 else torch.cat([outs[s] for s in src], 1)
                elif kind == "shortcut":
                    x = outs[-1] + outs[int(d["from"])]
                elif kind == "yolo":
                    heads.append(x)
                outs.append(x)
        return heads
