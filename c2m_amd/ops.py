"""Host side of the HIP kernels: torch.autograd Functions over the C ABI (include/c2m_hip.h).

PyTorch is used for device memory, streams and autograd bookkeeping only; every op below launches hand-written
gfx950 kernels from libc2m_hip.so on torch's current HIP stream.  There is no CPU or eager fallback: a tensor that is
not on a HIP device raises (the oracle in oracle/ is test infrastructure and is never imported from here).
"""
import collections
import ctypes
import os
import weakref
import math

import numpy as np
import torch

from . import _lib

G, WG = _lib.GEOM, _lib.WINO_GEOM      # names of the geom[] entries (include/c2m_geom.h: one definition for kernels and host)

ACT = {None: 0, "none": 0, "relu": 1, "lrelu": 2, "sigmoid": 3}
LRELU_SLOPE = 0.2


def _stream():
    """torch's current HIP stream of the current device as a raw handle (torch.cuda.current_stream() costs ~9 us of
    Python per call -- 500 calls per step; the private raw getter is the same lookup without the Stream object)."""
    return ctypes.c_void_p(_raw_stream(_cur_device()))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)
if _raw_stream is None or _cur_device is None:          # older / newer torch without the private getters
    _raw_stream = lambda idx: torch.cuda.current_stream(idx).cuda_stream
    _cur_device = torch.cuda.current_device


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(*ts):
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            _hip_only(t)                # raises: the message is spelled there
        if t.dtype != torch.float32 and t.dtype != torch.bfloat16:
            raise RuntimeError(f"c2m_amd ops take fp32 (or, on the bf16 data path, bf16) tensors, got {t.dtype}")
        if cur is None:
            cur = _cur_device()
        if t.device.index != cur:       # kernels are launched on the CURRENT device's stream (see _stream)
            _on_current_device(t)       # raises


def _hip_only(*ts, name=None, where=False, required=False):
    """The device guard of every operator outside the training path (that one is _dev: it adds the dtype rule and reports through
    these two): refuses a tensor that is not on a HIP device.  None and values that are no tensors pass (an operator's own checks
    name those), unless `required`.  name: the argument, as a prefix of the message; with `where` appended instead, together with
    the device it is on."""
    for t in ts:
        if t.is_cuda if isinstance(t, torch.Tensor) else not required:
            continue
        msg = "c2m_amd ops need tensors on a HIP device (no CPU fallback by design)"
        if where:
            raise RuntimeError(f"{msg}: {name} is on {t.device}")
        raise RuntimeError(f"{name}: {msg}" if name else msg)


def _on_current_device(*ts, name=None):
    """Refuses a tensor (None passes) of another GPU than the current one: kernels are launched on the CURRENT device's stream
    (see _stream), where such a tensor would arrive as a bare address."""
    cur = _cur_device()
    for t in ts:
        if t is not None and t.device.index != cur:
            raise RuntimeError(f"{name + ': ' if name else 'c2m_amd ops: '}tensor on cuda:{t.device.index} but the current device "
                               f"is cuda:{cur}; call torch.cuda.set_device() (or use `with torch.cuda.device(...)`) first")


def _f(t):
    return t if t.is_contiguous() else t.contiguous()


BF16 = torch.bfloat16


def _dt(t):
    """Element-type code of the C ABI (csrc/dtype.h): 0 = fp32, 1 = bf16."""
    return 1 if t.dtype == torch.bfloat16 else 0


def _as(t, dtype):
    """t in `dtype`, contiguous (None passes through)."""
    if t is None:
        return None
    return _f(t if t.dtype == dtype else t.to(dtype))


def _thin(M, splits, npix, two_target=False, ncls=1):
    """The dispatch rule of c2m_conv_igemm for the <= 4-output-row vector-ALU kernels (conv_thin.hip): those are fp32 in,
    fp32 out in either precision mode, so the host must hand them fp32 tensors."""
    return M <= 4 and splits == 1 and npix >= 16384 and not two_target and ncls == 1


# =============================================================================================== convolution
_geom_cache = {}
_conv_bf16 = False
# minimum region fill of a Winograd data-gradient launch: the padded 18x34 domain of the 16x32 reflect layers fills 53 % of its
# 8x16 regions and still beats the gather kernel by 14-30 % (tools/run_conv.py A/B); the 10x18 domain (35 %) does not
_WINO_DFIT = 0.5
_WINO_MIN_WGS = 128   # smallest Winograd forward / dgrad grid: 160 workgroups of a 1536-deep layer still beat the gather kernel 1.5x
# reflect-padded 3x3 data gradients as interior (exact domain, Winograd) + pad ring (conv_ring.hip): "auto" (maps of >= _RING_MIN_PIX
# pixels) | "off" (padded domain + two-target epilogue + fold, rounds 1-4) | "force" (tests: every eligible layer with H, W >= 4)
_RING = os.environ.get("C2M_RING", "auto")
_RING_BUFFER = True     # ring terms through a compact buffer added by the Winograd epilogue (False, set by the tests: the first form, in place)
_RING_MIN_PIX = 1024
_RING_F2_MAX_PIX = 4096      # largest map on which an F(2x2) interior + ring beats the padded domain
_WINO4 = os.environ.get("C2M_WINO4", "auto")       # F(4x4,3x3) for the 2-D Winograd layers: "off" | "auto" (rule: _wino4_pays) | "force" (tests: every eligible 2-D Winograd launch)
_WINO = os.environ.get("C2M_WINOGRAD", "auto")      # "auto" | "off" | "force" (tests: every eligible shape)
# Winograd WEIGHT gradient (round 2: fragments built in registers from raw LDS patches): "auto" = the layers where it beats
# the direct kernel, "off", "force" (tests: every eligible shape).
_WINO_WGRAD = os.environ.get("C2M_WINOGRAD_WGRAD", "auto")      # "auto" | "off" | "force"


def set_conv_precision(precision):
    """"fp32" (default: exact fp32 MFMA, fp32 tensors) or "bf16" (BASELINE configs[2-4]): the bf16 data path.  Convolutions
    multiply bf16 operands on the bf16 MFMA with fp32 accumulation AND write bf16 activations (NCHW, as PyTorch lays them
    out); norm / activation / up-sampling / pooling / warping kernels read and write bf16 with fp32 arithmetic in registers;
    gradients of those activations are bf16 as well.  Stays fp32: weights and their gradients (the optimizer's master copy),
    norm statistics, losses, flows / occlusion / index masks (bit-exact paths), the <= 4-channel heads (flow, occlusion,
    RGB).  An fp32 tensor handed to a bf16-mode convolution is cast once (RNE), so old call sites keep working.
    Returns the previous setting."""
    global _conv_bf16
    if precision not in ("fp32", "bf16"):
        raise ValueError(f"unknown conv precision {precision!r}")
    prev = "bf16" if _conv_bf16 else "fp32"
    _conv_bf16 = precision == "bf16"
    return prev


class conv_precision:
    """Context manager form of set_conv_precision (the backward of a conv uses the precision of its forward)."""

    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        self.prev = set_conv_precision(self.precision)

    def __exit__(self, *exc):
        set_conv_precision(self.prev)


class ConvProfiler:
    """Optional HIP-event timing of every implicit-GEMM launch (bench.py roofline): events are recorded on the stream
    the kernels are launched on (torch's current stream).  Off by default; zero overhead when off."""
    active = None

    def __init__(self):
        self.records = []          # (kind, flops, start_event, end_event, tag, algorithmic bytes)
        self._pool, self._used = [], 0

    def __enter__(self):
        ConvProfiler.active = self
        return self

    def __exit__(self, *exc):
        ConvProfiler.active = None

    def __del__(self):
        try:
            L = _lib.lib()
            for e in self._pool:
                L.c2m_event_destroy(e)
        except Exception:
            pass

    def _event(self):
        """HIP timing event without the system-scope fence of torch.cuda.Event (csrc/events.hip)."""
        if self._used == len(self._pool):
            import ctypes
            h = ctypes.c_void_p(None)
            _lib.check(_lib.lib().c2m_event_create(ctypes.addressof(h)), "event_create")
            self._pool.append(h.value)
        self._used += 1
        return self._pool[self._used - 1]

    @staticmethod
    def _ms(e0, e1):
        import ctypes
        ms = ctypes.c_float(0.0)
        _lib.check(_lib.lib().c2m_event_elapsed_ms(e0, e1, ctypes.addressof(ms)), "event_elapsed")
        return float(ms.value)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, flops, e0, e1, _, nbytes in self.records:
            d = out.setdefault(kind, dict(launches=0, flops=0.0, ms=0.0, bytes=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += self._ms(e0, e1)
        return out

    def table(self):
        """Per launch-shape totals: [(tag, launches, ms, TFLOP/s)] sorted by time."""
        torch.cuda.synchronize()
        agg = {}
        for kind, flops, e0, e1, tag, _ in self.records:
            d = agg.setdefault((kind,) + tuple(tag), [0, 0.0, 0.0])
            d[0] += 1
            d[1] += self._ms(e0, e1)
            d[2] += flops
        rows = [(k, v[0], v[1], v[2] / (v[1] * 1e-3) / 1e12) for k, v in agg.items()]
        return sorted(rows, key=lambda r: -r[2])


# weight gradient on a side stream: "auto" = bf16 data path AND inside a HIP-graph capture; "1" = bf16 and fp32, eager too; "0" off.
# Measured: graph replays of the bf16 configurations 89.7 -> 86.7 ms (configs[2]), 159.4 -> 152.0 (configs[4]),
# 55.5 -> 55.2 (configs[3]).  Eager: fork / join cost the host ~25 us per conv node (events, stream switch, record_stream), which a
# host-bound eager step pays in full (configs[3] 62.0 -> 65.3 ms; configs[4], GPU-bound, 161.6 -> 155.1), and per-kernel HIP-event
# times of overlapping launches are no kernel measurements any more -- so eager steps stay on one stream.  fp32 configs[1]:
# 74.5 -> 75.3 ms (the fp32 Winograd kernels fill the CUs' LDS and registers by themselves).
_WGRAD_SIDE = os.environ.get("C2M_WGRAD_STREAM", "auto")
_side_streams = {}


def _side_stream(device):
    # (stream priorities measured, round 5: side stream high 62.9 vs 62.1 ms, low = default; the step on a prioritised non-default
    # stream 62.1 (high) / 63.9 (normal) vs 62.2 on the default stream -- nothing to gain, default priorities everywhere)
    s = _side_streams.get(device.index)
    if s is None:
        s = _side_streams[device.index] = torch.cuda.Stream(device=device)
    return s


# ---- auxiliary stream for the object branch (round 5).  The RoI head of the appearance encoder and the object GNN are ~600 launches
# of a few microseconds on [24, 1024]-sized tensors per step (Linear layers, GATv2 attention, theta losses): ~3 ms of GPU time that
# uses a sliver of the chip and, with gt thetas (use_gt_training: True), feeds nothing but the theta losses.  Run on a second stream
# they execute NEXT TO the convolutions of the motion encoders / decoder / generator instead of between them -- forward, and
# backward too: autograd runs every backward node on the stream of its forward and orders the streams itself.  No arithmetic
# changes; every kernel pairing is one the concurrency stress test covers.  C2M_AUX_STREAM=0 switches it off (A/B).
_AUX = os.environ.get("C2M_AUX_STREAM", "1")          # 1 | 0 | obj (= roi + gnn) | novgg | roi | gnn | vgg (parts: diagnosis, A/B)
_aux_streams = {}        # (device index, lane) -> stream.  Lane 0: the object branch; lane 1: the ground-truth VGG pass (losses.py)
_aux_open = {}           # (device index, lane) -> the lane has work the main stream has not joined yet


class aux_branch:
    """`with ops.aux_branch(*input_tensors): ...` -- the body's launches go to an auxiliary stream of the device, ordered behind
    everything the current stream has been given so far.  The results may only be used on the main stream after `aux_join`."""

    def __init__(self, *inputs, part="", lane=0):
        self.inputs = [t for t in inputs if torch.is_tensor(t) and t.is_cuda]
        self.ctx = None
        self.lane = lane
        self.on = _AUX == "1" or _AUX == part or (_AUX == "obj" and part in ("roi", "gnn")) or \
            (_AUX.startswith("no") and _AUX[2:] != part)
        # bench.py's per-launch HIP events time ISOLATED launches: the steps that carry them run on one stream (a kernel that shares
        # the chip with another stream's is stretched, in the events and in a rocprofv3 trace alike)
        self.on = self.on and ConvProfiler.active is None

    def __enter__(self):
        if not self.on or not self.inputs:
            if self.inputs:
                aux_join(*self.inputs, lanes=(self.lane,))    # (diagnosis mode, an earlier part on this lane: this one reads its results)
            return self
        dev = self.inputs[0].device
        key = (dev.index, self.lane)
        aux = _aux_streams.get(key)
        if aux is None:
            aux = _aux_streams[key] = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream(dev)
        if aux == main:
            return self
        aux.wait_stream(main)                     # (a second block of the same branch: aux order kept, the new dependencies added)
        for t in self.inputs:
            t.record_stream(aux)                  # allocated on the main stream's pool, read by aux-stream kernels
        _aux_open[key] = True
        self.ctx = torch.cuda.stream(aux)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# ---- deferred weight gradients (round 5): see _ConvFn.backward
_DEFER_WGRAD = os.environ.get("C2M_DEFER_WGRAD", "1") != "0"
_defer = {"on": False, "params": {}, "devs": set(), "seen": set(), "hold": collections.deque(), "grads": {}, "by_p": {}}


class deferred_wgrads:
    """`with ops.deferred_wgrads(params=conv_weights_and_biases): loss.backward()` -- the weight / bias gradients of the
    convolutions whose parameters are listed are computed on the side stream and joined once, when the block exits (on the stream
    that is current then, also when the body raises).  Listing a parameter is a promise: inside this backward its gradient is
    produced by ops.conv nodes only (no other op of the graph reads the parameter) and nobody reads it before the block exits.
    Everything the node can check for itself it does (_may_defer); a convolution whose parameters are not listed, and every case
    the checks turn down, computes its gradients on the backward's own stream as without the block."""

    def __init__(self, enabled=True, params=None):
        self.params = {id(p): p for p in (params or ())}
        self.enabled = bool(enabled) and _DEFER_WGRAD and bool(self.params)

    def __enter__(self):
        _defer["on"] = self.enabled
        _defer["params"] = self.params if self.enabled else {}
        _defer["seen"].clear()
        _defer["grads"].clear()
        _defer["by_p"].clear()
        return self

    def __exit__(self, *exc):
        _defer["on"] = False
        for idx in _defer["devs"]:
            side = _side_streams[idx]
            torch.cuda.current_stream(side.device).wait_stream(side)
        _defer["devs"].clear()
        _defer["hold"].clear()            # (the joined stream orders every later write behind the side stream's reads)
        _defer["grads"].clear()
        _defer["by_p"].clear()
        _defer["seen"].clear()
        _defer["params"] = {}
        return False


def deferred_grad_stream(grad):
    """The side stream if `grad` is a weight / bias gradient that a deferred launch of the current backward is still producing
    (ops.deferred_wgrads), else None.  For whoever touches a parameter gradient INSIDE backward (the gradient reducer's hook).
    A hook that asks this carries `_c2m_asks_grad_stream = True`: parameters with any other hook are not deferred."""
    return _defer["grads"].get(grad.data_ptr()) if _defer["grads"] else None


def deferred_grad_done(grad):
    """`grad` has been consumed on the stream deferred_grad_stream named and is about to be dropped: its address no longer stands
    for a gradient in flight (the allocator may hand the block to a tensor made on another stream)."""
    _defer["grads"].pop(grad.data_ptr(), None)


def _may_defer(p):
    """The gradient of parameter `p` may stay unjoined on the side stream until the block exits: the caller listed it, it is a
    leaf without a gradient (AccumulateGrad adopts the tensor: no kernel), this is its first gradient in this backward (a second
    one is summed by the engine on the backward's stream) and it carries no hook that would read the gradient inside backward."""
    if p is None or id(p) not in _defer["params"] or id(p) in _defer["seen"] or not p.is_leaf or p.grad is not None:
        return False
    for hooks in (p._backward_hooks, getattr(p, "_post_accumulate_grad_hooks", None)):
        if hooks and not all(getattr(h, "_c2m_asks_grad_stream", False) for h in hooks.values()):
            return False
    return True


def _record_stream_all(stream, *objs):
    """Every device tensor in objs (tensors, NC8 placeholders and their forms, dicts / tuples of them) is in use on `stream`."""
    for o in objs:
        if o is None:
            continue
        if torch.is_tensor(o):
            if o.is_cuda:
                o.record_stream(stream)
                form = getattr(o, "_c2m_nc8", None)               # (version, NC8 form) riding on the tensor object
                if form is not None and torch.is_tensor(form[1]):
                    form[1].record_stream(stream)
                ent = _nc8_only.get(o.data_ptr()) if getattr(o, "_c2m_nc8_only", False) else None
                if ent is not None and torch.is_tensor(ent[2]):
                    ent[2].record_stream(stream)
        elif isinstance(o, dict):
            _record_stream_all(stream, *o.values())
        elif isinstance(o, (tuple, list)):
            _record_stream_all(stream, *o)


def branch_streams(device):
    """The streams -- besides the one backward() is called on -- that backward nodes of this package run on (the object branch's
    auxiliary stream, the weight-gradient side stream).  Whoever consumes gradients from ANOTHER stream before backward() has
    returned (the gradient reducer's communication stream) has to wait for these as well."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return [s for (i, _), s in _aux_streams.items() if i == idx] + ([_side_streams[idx]] if idx in _side_streams else [])


def _on_aux_stream(dev):
    cur = None
    for (i, _), s in _aux_streams.items():
        if i == dev.index:
            cur = torch.cuda.current_stream(dev) if cur is None else cur
            if s == cur:
                return True
    return False


def aux_join(*outputs, lanes=None):
    """The current stream waits for the auxiliary streams' work (all lanes, or the given ones); `outputs` (tensors made there) may
    be used from here on."""
    for key, is_open in list(_aux_open.items()):
        if not is_open or (lanes is not None and key[1] not in lanes):
            continue
        aux = _aux_streams[key]
        main = torch.cuda.current_stream(aux.device)
        if aux != main:
            main.wait_stream(aux)
            _record_stream_all(main, *outputs)
        _aux_open[key] = False


def _timed(kind, flops, fn, tag=(), nbytes=0):
    prof = ConvProfiler.active
    if prof is None:
        return fn()
    L, st = _lib.lib(), _stream()
    e0, e1 = prof._event(), prof._event()
    _lib.check(L.c2m_event_record(e0, st), "event_record")
    rc = fn()
    _lib.check(L.c2m_event_record(e1, st), "event_record")
    prof.records.append((kind, flops, e0, e1, tag, nbytes))
    return rc


def _ceil(a, b):
    return (a + b - 1) // b * b


def _cdiv(a, b):
    return (a + b - 1) // b


def _triple(v, nd):
    if isinstance(v, int):
        return (1,) * (3 - nd) + (v,) * nd if nd < 3 else (v, v, v)
    v = tuple(int(a) for a in v)
    return (1,) * (3 - len(v)) + v if len(v) < 3 else v


def _pad3(v, nd):
    if isinstance(v, int):
        return (0,) * (3 - nd) + (v,) * nd
    v = tuple(int(a) for a in v)
    return (0,) * (3 - len(v)) + v


def _choose_ck(C, taps):
    """Channels per tap inside one 16-deep K-step (CK x NS = 16): the padding-minimal choice, larger CK on ties."""
    best = None
    for ck in (16, 8, 4):
        ns = 16 // ck
        cost = _ceil(C, ck) * _ceil(taps, ns) * (1.0 + 0.03 * (ns - 1))
        if best is None or cost < best[0] * 0.97:
            best = (cost, ck)
    return best[1]


class _Layer(collections.namedtuple("_Layer", "N Cin Cout Ti Hi Wi To Ho Wo kt kh kw st sh sw pt ph pw nd reflect bf16 dM in_sc osp taps")):
    """The numbers of one layer, as _ConvPlan.__init__ works them out: what the stages of a plan and the routing rules below read.
    dM: rows of the data-gradient GEMM; in_sc / osp: elements of one input / output channel; taps = kt * kh * kw.  The three
    kernel shapes with kernels of their own: 3x3 stride 1 pad 1; 4x4 stride 2 pad 1 on even extents; 3x3x3 stride 1 pad 1."""
    __slots__ = ()
    k = property(lambda ly: (ly.kt, ly.kh, ly.kw))
    stride = property(lambda ly: (ly.st, ly.sh, ly.sw))
    is_3x3_s1p1 = property(lambda ly: ly.k == (1, 3, 3) and ly.stride == (1, 1, 1) and (ly.ph, ly.pw) == (1, 1))
    is_4x4_s2p1_even = property(lambda ly: ly.k == (1, 4, 4) and ly.stride == (1, 2, 2) and (ly.ph, ly.pw) == (1, 1) and
                                ly.Hi % 2 == 0 and ly.Wi % 2 == 0)
    is_333_s1p1 = property(lambda ly: ly.k == (3, 3, 3) and ly.stride == (1, 1, 1) and (ly.pt, ly.ph, ly.pw) == (1, 1, 1))


def _rows_ok(m):
    """Rows of a Winograd forward / data gradient: 64-row tiles need >= 48 output channels to pay; 17..32 run on the 32-row variant
    (MT = 1, three workgroups per CU), which beats the direct kernels' 32-row tiles."""
    return m >= 48 or 17 <= m <= 32


def _wino_gate(regions, pixels, fit, K, M):
    """A Winograd forward / data gradient of M rows over a K-deep reduction pays: the domain's `pixels` fill at least `fit` of its
    `regions` (128 outputs each), and the grid is big enough."""
    return _WINO == "force" or (_WINO == "auto" and pixels >= fit * regions * 128 and K >= 32 and _rows_ok(M) and
                                regions * _cdiv(M, 64) >= _WINO_MIN_WGS)


def _chan16_ok(c, limit):
    """c channels as whole 16-channel chunks: at least 12, padded to at most `limit` times their number."""
    return c >= 12 and _ceil(c, 16) <= limit * c


def _tile_area(H, W, rows=8):
    return _ceil(W, 32) * _ceil(H, rows)


def _fill_ok(H, W, limit, rows=8):
    """The (rows x 32) tiles of an H x W domain cover at most `limit` times its pixels."""
    return _tile_area(H, W, rows) <= limit * W * H


def _patch_ok(C, taps3, stride, splits, Ho, Wo, M):
    """LDS-patch kernel eligibility: 3x3 (kt = 1) stride-1, whole 16-channel chunks without much padding, a grid big
    enough not to need split-K, output rows/cols that fill the (rows x 32) tile reasonably."""
    kt, kh, kw = taps3
    if (kt, kh, kw) != (1, 3, 3) or tuple(stride) != (1, 1, 1) or M <= 4:      # <= 4 rows: vector-ALU kernels
        return False
    best = _ceil(C, _choose_ck(C, 9))
    if _ceil(C, 16) > 1.10 * best:
        return False
    rows = 8 if M <= 32 else 4
    return Wo >= 32 and Ho >= rows and _fill_ok(Ho, Wo, 1.15, rows)


def _patch_bf16_ok(C, stride, Ho, Wo, M, fill_limit=None, nc8=True):
    """bf16 LDS-patch kernel (8 rows x 32 columns per workgroup): 3x3 stride-1.  Where it beats the bf16 gather kernel
    (per-shape A/B of BASELINE configs[2], gpurun_out/r02/table_cfg2*.txt): deep reductions (>= 128 channels: the weight
    image of a chunk is re-streamed per 256 pixels, which only pays with many chunks) or few output rows (<= 64), and
    tiles that do not hang far over the (padded) domain; <= 4 output rows stay on the vector-ALU kernels."""
    if tuple(stride) != (1, 1, 1) or M <= 4 or Wo < 32 or Ho < 8 or not _chan16_ok(C, 1.25):
        return False
    fill = _tile_area(Ho, Wo) / float(Wo * Ho)      # (the quotient, not _fill_ok's product: the two round differently)
    if _NC8 and nc8:      # the channel-blocked kernel (conv_nc8.hip) has no 2-byte gathers to amortise: every layer whose tiles fit
                          # (nc8: the plan can run it -- planes of whole 8-pixel groups; otherwise the NCHW kernel's own rule below)
        return fill <= (fill_limit or _NC8_FILL)      # (the padded 34x66 domain of a reflect data gradient fills 58 % of its tiles: still 1.5x the gather kernel)
    if C < 128:
        return M <= 64 and fill <= 1.2
    return fill <= _PATCH_FILL[0] or (fill <= _PATCH_FILL[1] and C >= 256)


_NC8_VARIANT = 0      # tile / buffering variant of conv_patch_nc8_kernel: 0 = the library's rule; tests set 1, 2, 4, 5 (the rule's choices)
# NC8 gather kernel (conv_gather_nc8_kernel, conv_gather.hip): every bf16 forward / data gradient the NC8 patch forms do not take
_NC8_LOG = None
_NC8_LOG_TAG = [""]          # (tools/nc8_producers.py: what made the gradient tensor a backward conversion sees)
_NC8_GRAD = os.environ.get("C2M_NC8_GRAD", "1") != "0"      # act_bwd / tap backward write NC8 only where every reader is an NC8 kernel
_NC8_POISON = os.environ.get("C2M_NC8_POISON", "0") == "1"  # debug: the unused NCHW storage of such gradients is NaN
_G8 = os.environ.get("C2M_G8", "1") != "0"
_G8_VARIANT = 0      # tile variant of conv_gather_nc8_kernel: 0 = the library's rule; tests set 1, 3, 5 (the rule's choices)
_NC8_S2_WGRAD_MIN_PIX = 16384
# padded domains of the reflect data gradients: tile waste above which the NC8 gather form takes them (kernel times on one box,
# patch kernel with the buffer-store two-target epilogue vs gather form: 66x130 domains, fill 1.34: 78 vs 111 us and 144 vs 151;
# 34x66, fill 1.71: 106 vs 87; 18x34, fill 2.5: 68 vs 45)
_NC8_DGRAD_FILL = 1.5
_NC8_S2_FILL_G8 = 1.5      # stride-2 patch forms: largest tile waste where the gather form is the alternative
_NC8_FILL = 2.6      # (18x34 padded domains of the 16x32 reflect data gradients: 2.5; still 1.5x+ the gather kernel)
_NC8 = os.environ.get("C2M_NC8", "1") != "0"        # bf16 3x3 stride-1 layers on channel-blocked input (A/B knob)
_PATCH_FILL = (1.15, 1.4)     # bf16 3x3 NCHW patch kernel: largest tile waste (any C; C >= 256), see _patch_pays


def _pack_bf16_patch(w, M, C, s_m, s_c, mode=0):
    """c2m_pack_weights_bf16_patch: contiguous native 3x3 weights -> bf16 [chunk][tap][Mpad][16]; mode 2: native 4x4 weights of a
    stride-2 layer -> [chunk][input parity][2x2 tap][Mpad][16] (conv_nc8.hip, S2)."""
    L = _lib.lib()
    nbytes = L.c2m_pack_weights_bf16_s2_bytes(M, C) if mode >= 2 else L.c2m_pack_weights_bf16_patch_bytes(M, C)
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    g = np.array([M, C, s_m, s_c, mode], dtype=np.int64)
    _lib.check(L.c2m_pack_weights_bf16_patch(_p(w), _p(out), _gp(g), _stream()), "pack_weights_bf16_patch")
    out._c2m_job = (1, g)                   # how to rebuild this pack in place (refresh_trainable_packs)
    return out


_BF16_SPLIT_DIV = 4.0      # bf16 kernels: a quarter of the fp32 rule's K splits (A/B on configs[2,3], graph mode: 1 -> 60.0 / 93.7 ms, 2 -> 58.4 / 92.5, 4 -> 58.0 / 91.2, no splits -> 65.4 / 98.2)


def _splits(L, M, nk, npix, bf16):
    """c2m_conv_igemm_splits, optionally thinned out for the bf16 kernels (every split still owns >= 1 K-step)."""
    S = L.c2m_conv_igemm_splits(M, nk, npix)
    if bf16 and _BF16_SPLIT_DIV != 1 and S > 1:
        S = max(1, int(S / _BF16_SPLIT_DIV))
        S = _cdiv(nk, _cdiv(nk, S))
    return S


def _patch_splits(L, M, C, npix, bf16=False):
    """Split-K count for the patch kernel: whole 16-channel chunks per split, every split non-empty."""
    nch = _cdiv(C, 16)
    s0 = _splits(L, M, nch * 9, npix, bf16)
    return _cdiv(nch, _cdiv(nch, s0))


_nc8_only = {}      # storage address -> (weakref(NC8-only tensor), its _version, NC8 form)


def _drop_nc8_only(key):
    ent = _nc8_only.get(key)
    if ent is not None and ent[0]() is None:
        del _nc8_only[key]


def _mark_nc8_only(t, tn):
    """`t` is an NCHW-shaped tensor object whose storage is never written: its values exist as `tn` (NC8) only."""
    t._c2m_nc8 = (t._version, tn)
    t._c2m_nc8_only = True
    key = t.data_ptr()
    _nc8_only[key] = (weakref.ref(t), t._version, tn)
    weakref.finalize(t, _drop_nc8_only, key)
    return t


def _to_nc8(x, keep=None):
    """c2m_nchw_to_nc8: contiguous bf16 [N, C, H, W] -> [N, ceil(C/8), H, W, 8] (the conv input form of conv_nc8.hip).
    The result is remembered ON the source tensor (attribute, with the tensor's `_version`: any in-place change invalidates it),
    so an activation that feeds several convolutions -- the SPADE maps, the shared conditioning features -- is converted once;
    keep: a dict that additionally pins the result per source tensor for the duration of one backward node (the data gradient and
    the weight gradient share the NC8 form of dY even when autograd hands them the gradient as a fresh tensor object)."""
    hit = getattr(x, "_c2m_nc8", None)
    if hit is not None and hit[0] == x._version and hit[1].device == x.device:
        if keep is not None:
            keep[x.data_ptr()] = (x, hit[1])       # (a tensor that exists in NC8 form only must never depend on the attribute alone)
        return hit[1]
    if keep is not None:
        hit = keep.get(x.data_ptr())
        if hit is not None and hit[0] is x:
            return hit[1]
    # NC8-only tensors: the NCHW storage of such a tensor was never written.  If the attribute did not travel with the
    # tensor object (tensor hooks, retain_grad, saved_tensors_hooks hand out another object over the same storage) the NC8 form is
    # recovered from the registry by storage address + version; a tensor tagged NC8-only without any valid form is an error, never
    # a layout pass over uninitialised memory.
    ent = _nc8_only.get(x.data_ptr())
    if ent is not None:
        src = ent[0]()
        if src is not None and src.shape == x.shape and src.dtype == x.dtype and ent[1] == x._version and ent[2].device == x.device:
            if keep is not None:
                keep[x.data_ptr()] = (x, ent[2])
            return ent[2]
    if getattr(x, "_c2m_nc8_only", False):
        raise RuntimeError("c2m_amd: a tensor that exists in NC8 form only reached a convolution without a valid NC8 form (it was "
                           "modified in place, or its single-consumer contract -- feeds= / private_input= -- was broken)")
    N, C = x.shape[0], x.shape[1]
    sp = tuple(x.shape[2:])                 # (H, W), or (T, H, W): the pixel axis of the layout pass is everything behind C
    if _NC8_LOG is not None:                # tools/nc8_producers.py: who produced the tensors that need a layout pass
        fn = x.grad_fn
        _NC8_LOG.append((type(fn).__name__ if fn is not None else ("leaf" if torch.is_grad_enabled() else "backward" + _NC8_LOG_TAG[0]), tuple(x.shape)))
    y = torch.empty((N, _cdiv(C, 8)) + sp + (8,), device=x.device, dtype=BF16)
    _lib.check(_lib.lib().c2m_nchw_to_nc8(_p(x), _p(y), N, C, int(np.prod(sp)), _stream()), "nchw_to_nc8")
    if keep is not None:
        keep[x.data_ptr()] = (x, y)
    x._c2m_nc8 = (x._version, y)
    return y


def _time_pair_table_kt(T, reflect):
    """Data gradient of a 3-tap pad-1 convolution in time: output frame t sums dY frame `to` through time tap kt for every
    (to, kt) with reflect(to + kt - 1) == t (reflect padding: the pad frames' contributions land on the frames they mirror) or
    to + kt - 1 == t (zeros).  int32 [T][11] = {npairs, (to, kt) x 5} -- c2m_conv3d_dgrad_nc8's ptab."""
    tab = np.zeros((T, 11), dtype=np.int32)
    for t in range(T):
        pairs = []
        for kt in range(3):
            for to in range(T):
                q = to + kt - 1
                if reflect:
                    q = -q if q < 0 else (2 * T - 2 - q if q >= T else q)
                if q == t:
                    pairs.append((to, kt))
        assert 1 <= len(pairs) <= 5
        tab[t, 0] = len(pairs)
        for j, (to, kt) in enumerate(pairs):
            tab[t, 1 + 2 * j], tab[t, 2 + 2 * j] = to, kt
    return tab


def _pack_bf16_k333(w, M, C, dgrad=False, cin_total=None):
    """Weights [Cout][Cin][3][3][3] of a 3x3x3 layer -> three c2m_pack_weights_bf16_patch images back to back (time tap kt = 0, 1, 2);
    rows M = output channels, reduction C = input channels -- or, for the data gradient, rows = input channels over output channels."""
    L = _lib.lib()
    nb = L.c2m_pack_weights_bf16_patch_bytes(M, C)
    out = torch.empty(3 * nb, device=w.device, dtype=torch.uint8)
    wf = w.reshape(-1)
    for kt in range(3):
        g = np.array([M, C, 27, (cin_total or M) * 27, 0] if dgrad else [M, C, C * 27, 27, 0], dtype=np.int64)
        _lib.check(L.c2m_pack_weights_bf16_patch(_p(wf[kt * 9:]), _p(out[kt * nb:]), _gp(g), _stream()), "pack_weights_bf16_patch (3-D)")
    return out


def _nc8_launch(L, A, x, dst, y2, b, geom, act, slope, keep=None):
    """One 3x3 stride-1 launch on channel-blocked input: the layout pass + c2m_conv_patch_nc8 (timed together)."""
    xn = _to_nc8(x, keep)
    geom[G.NC8_VARIANT] = _NC8_VARIANT
    return L.c2m_conv_patch_nc8(_p(A), _p(xn), _p(dst), _p(y2), _p(b), _gp(geom), act, slope, _stream())


def _pack_bf16_gather(w, M, C, kdims, stride, s_m, s_c):
    """c2m_pack_weights_bf16_gather: contiguous native weights -> prod(stride) class images [tap][16-channel chunk][half][Mpad] of
    16-byte bf16 units (the NC8 gather kernel's K order: tap-major)."""
    L = _lib.lib()
    kt, kh, kw = kdims
    st, sh, sw = stride
    g = np.array([M, C, 16, kt, kh, kw, st, sh, sw, s_m, s_c], dtype=np.int64)
    nbytes = L.c2m_pack_weights_bf16_gather_bytes(_gp(g))
    if nbytes <= 0:
        raise RuntimeError("c2m_pack_weights_bf16_gather_bytes: bad geometry")
    out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    _lib.check(L.c2m_pack_weights_bf16_gather(_p(w), _p(out), _gp(g), _stream()), "pack_weights_bf16_gather")
    out._c2m_job = (2, g)
    return out


def _g8_bm(M):
    """Row tile of conv_gather_nc8_kernel for M output rows (the rule of c2m_conv_igemm's NC8 gather form)."""
    return 32 if M <= 32 else (64 if (M <= 64 or 1 <= M % 128 <= 64) else 128)


_G8_SPLIT_WGS = 320


def _g8_splits(M, nk, npix, ncls=1):
    """K splits of an NC8 gather launch (256-pixel tiles): only launches that leave CUs empty are split, towards ~1.25 workgroups
    per CU with >= 8 K-steps per split -- at bf16 MFMA rates the fp32 slabs (4 bytes per output and split, written and read back)
    cost more than a second round of workgroups saves."""
    tiles = _cdiv(M, _g8_bm(M)) * _cdiv(npix, 256) * ncls
    if tiles >= 200 or nk < 16:
        return 1
    S = min(_cdiv(_G8_SPLIT_WGS, tiles), nk // 8, 16)
    if S < 2:
        return 1
    return _cdiv(nk, _cdiv(nk, S))


def _g8_geom(geom, C, taps, S):
    """geom of the same launch on the NC8 gather form: nk = taps * ceil(C/16) K-steps in (tap, chunk) order."""
    g = geom.copy()
    nk = taps * _cdiv(C, 16)
    g[[G.NK, G.LDA, G.NS, G.SPLITS, G.CIN, G.TAPS, G.PRECISION, G.PATCH, G.G8, G.G8_VARIANT]] = (nk, nk * 16, 1, S, C, taps, 1, 0, 1, _G8_VARIANT)
    return g


def _g8_taps(offs, device):
    t = np.zeros((len(offs), 4), dtype=np.int32)
    t[:, :3] = np.asarray(offs, dtype=np.int32).reshape(len(offs), 3)
    t[:, 3] = 1
    return torch.from_numpy(t.reshape(-1)).to(device)


def _set_patch(geom, iy0, ix0, pty, ptx):
    geom[G.PATCH] = 1
    geom[G.PATCH_IY0], geom[G.PATCH_IX0] = iy0, ix0
    geom[G.PATCH_TY:G.PATCH_TY + 3] = pty
    geom[G.PATCH_TX:G.PATCH_TX + 3] = ptx


def _tap_offsets(kt, kh, kw, off_t, off_y, off_x):
    """(dt, dy, dx) per tap in (t, y, x) row-major order."""
    return [(int(off_t[a]), int(off_y[b]), int(off_x[c])) for a in range(kt) for b in range(kh) for c in range(kw)]


def _kstep_table(C, tap_offs, chan_stride, ck, extra_groups=0, ones_group=False):
    """K-step / row-group table: [(groups), 1 + NS, 4] int32 in (channel chunk, tap group) order.
    group = header {chan_off, nvalid, 0, 0} + NS x {dt, dy, dx, valid}; optional ones group (nvalid = -2) and zero pads."""
    ns = 16 // ck
    taps = len(tap_offs)
    nch, ntg = _cdiv(C, ck), _cdiv(taps, ns)
    n = nch * ntg
    tab = np.zeros((n + (1 if ones_group else 0) + extra_groups, 1 + ns, 4), dtype=np.int32)
    offs = np.zeros((ntg * ns, 4), dtype=np.int32)
    offs[:taps, :3] = np.asarray(tap_offs, dtype=np.int32).reshape(taps, 3)
    offs[:taps, 3] = 1
    for ch in range(nch):
        tab[ch * ntg:(ch + 1) * ntg, 0, 0] = ch * ck * chan_stride
        tab[ch * ntg:(ch + 1) * ntg, 0, 1] = min(ck, C - ch * ck)
        tab[ch * ntg:(ch + 1) * ntg, 1:, :] = offs.reshape(ntg, ns, 4)
    if ones_group:
        tab[n, 0, 1] = -2
    return tab, nch, ntg


def _pack_rows(wm, ck):
    """[M, C, taps] -> contiguous [M, nk*16] in the kernel's K order (chunk, tap group, tap slot, channel)."""
    M, C, taps = wm.shape
    ns = 16 // ck
    nch, ntg = _cdiv(C, ck), _cdiv(taps, ns)
    if nch * ck != C or ntg * ns != taps:
        buf = wm.new_zeros(M, nch * ck, ntg * ns)
        buf[:, :C, :taps] = wm
        wm = buf
    # .contiguous(): in degenerate cases (one tap, one chunk) the reshape chain is a strided VIEW of the weights
    return wm.reshape(M, nch, ck, ntg, ns).permute(0, 1, 3, 4, 2).reshape(M, nch * ntg * 16).contiguous()


def _geom(**kw):
    g = np.zeros(G.LEN, dtype=np.int64)      # CLS_PO .. LEN - 1: per-class (po_t, po_y, po_x) of a class-batched launch
    idx = dict(M=G.M, nk=G.NK, lda=G.LDA, Npix=G.NPIX, To=G.TO, Ho=G.HO, Wo=G.WO, Ti=G.TI, Hi=G.HI, Wi=G.WI, st=G.ST, sh=G.SH, sw=G.SW,
               in_sn=G.IN_SN, in_st=G.IN_ST, in_sh=G.IN_SH, out_sn=G.OUT_SN, out_sc=G.OUT_SC, out_st=G.OUT_ST, out_sh=G.OUT_SH,
               out_sw=G.OUT_SW, out_off=G.OUT_OFF, reflect=G.REFLECT, is3d=G.IS3D, ns=G.NS, in_sc=G.IN_SC, splits=G.SPLITS,
               slab_stride=G.SLAB_STRIDE, Cin=G.CIN, taps=G.TAPS, ntg=G.NTG, ngroups=G.NGROUPS, x_bytes=G.X_BYTES, dy_bytes=G.DY_BYTES,
               precision=G.PRECISION)
    for k, v in kw.items():
        g[idx[k]] = v
    return g


def _wino4_pays(L, M, K, nimg, Ho, Wo):
    """F(4x4,3x3) (conv_wino4.hip: 64 rows x 16x32 outputs per 512-thread workgroup, ONE workgroup per CU) instead of F(2x2,3x3)
    for a 2-D Winograd launch with M output rows, K input channels over nimg Ho x Wo output domains.  Measured per shape on one box
    (tools/bench_wino4.py, round 3): 1.25-1.42x on grids of >= 2.5 workgroups per CU that fill their 16x32 regions, 1.08-1.12x on
    the deep 16x32 layers, 0.87-0.92x on the 320-workgroup launches of 128-row layers at 32x64."""
    if _WINO4 == "force":
        return True
    if _WINO4 != "auto":
        return False
    regions = nimg * L.c2m_wino4_regions(Ho, Wo)
    fill = nimg * Ho * Wo / float(regions * 512)
    # (the deep 16x32 layers -- 512 -> 512 / 256 -> 256, 320 / 160 workgroups -- measure 1.08x / 1.12x alone but made the step
    # slower when routed here: 67.7 -> 68.3 ms; they stay on F(2x2))
    # fill: full regions only.  The padded 66 x 130 domains of the reflect data gradients (0.67 of their 16x32 regions) measure
    # 1.06-1.24x as isolated forward grids (tools/bench_wino4.py) but routing them here made the step slower (67.8 -> 68.1 ms)
    wgs = regions * (M // 64) if M % 64 == 0 else 0
    if K < _WINO4_MIN_K or M < 64 or fill < _WINO4_MIN_FILL:
        return False
    return wgs >= _WINO4_MIN_WGS


_WINO4_MIN_K = 64
_WINO4_MIN_FILL = 0.9
_WINO4_MIN_WGS = 600      # 640 workgroups (256 -> 256 at 32x64, 40 images): 1.12x; 320: 0.8-0.95x


def _wino4_filter(w, Cout, Cin, dgrad):
    """c2m_wino4_filter_transform: native [Cout][Cin][3][3] -> packed 6x6 U = G g G^T fragments of conv_wino4_kernel."""
    L = _lib.lib()
    M, K = (Cin, Cout) if dgrad else (Cout, Cin)
    U = torch.empty(L.c2m_wino4_upack_floats(M, K), device=w.device, dtype=torch.float32)
    _lib.check(L.c2m_wino4_filter_transform(_p(w), _p(U), Cout, Cin, dgrad, _stream()), "wino4_filter_transform")
    return U


def _ring_pack(w, Cout, Cin):
    """c2m_ring_pack: native [Cout][Cin][3][3] -> the A fragments of reflect_ring_dgrad_kernel (four sides x three taps)."""
    L = _lib.lib()
    A = torch.empty(L.c2m_ring_pack_floats(Cout, Cin), device=w.device, dtype=torch.float32)
    _lib.check(L.c2m_ring_pack(_p(w), _p(A), Cout, Cin, _stream()), "ring_pack")
    return A


def _wino_geom(**kw):
    """geom[] of c2m_conv_wino from its entries by name (C2M_WG_* of include/c2m_geom.h in lower case; what is not named is 0):
    m rows, k reduction depth, nimg images; hi, wi / ho, wo: input / output extents, with strides in_sn, in_sc, in_sh / out_sn, out_sc,
    out_sh; iy0, ix0: input origin of output (0, 0); reflect; x_bytes: byte bound of the input.  Two-target epilogue (_wino_interior):
    y2_* strides, lo_* origin and ext_* extents of the interior.  3x3x3 layers: to frames, in_st / out_st, cin x nkt virtual channels,
    toff, ti input frames, treflect."""
    g = np.zeros(WG.LEN, dtype=np.int64)
    for k, v in kw.items():
        g[WG[k.upper()]] = v
    return g


def _wino_interior(ly):
    """Two-target block of a reflect data gradient's Winograd geom: the pad-1 interior of the launched domain goes straight into dX."""
    return dict(y2_sn=ly.Cin * ly.in_sc, y2_sc=ly.in_sc, y2_sh=ly.Wi, lo_y=1, lo_x=1, ext_y=ly.Hi, ext_x=ly.Wi)


def _time_pair_table(T):
    """Temporal reflect padding (pad 1, 3 taps) folded into the data gradient: output frame t of the unpadded axis sums dY
    frame `to` through time tap kt for every (to, kt) with reflect(to + kt - 1) == t.  int32 [T][11] = {npairs, (to, U block =
    2 - kt: the flipped tap order of the packed data-gradient weights) x 5} -- c2m_conv_wino geom[33]."""
    tab = np.zeros((T, 11), dtype=np.int32)
    for t in range(T):
        pairs = []
        for kt in range(3):
            for to in range(T):
                q = to + kt - 1
                q = -q if q < 0 else (2 * T - 2 - q if q >= T else q)
                if q == t:
                    pairs.append((to, 2 - kt))
        assert 2 <= len(pairs) <= 5
        tab[t, 0] = len(pairs)
        for j, (to, ub) in enumerate(pairs):
            tab[t, 1 + 2 * j], tab[t, 2 + 2 * j] = to, ub
    return tab


class _ConvPlan:
    """Everything shape-dependent for one conv layer geometry (cached): gather tables + geom arrays."""

    def __init__(self, xs, ws, stride, pad, reflect, device, bf16=False, dgrad_rows=None):
        L = _lib.lib()
        self.bf16 = bf16
        nd = len(xs) - 2
        self.is3d = 1 if nd == 3 else 0
        N, Cin = xs[0], xs[1]
        if ws[1] != Cin:
            # torch.nn.functional.conv2d raises here too.  Without the check the pack kernels read Cin * taps weights per output
            # row out of a tensor that holds ws[1] * taps: past its end -- harmless next to other cached blocks, a GPU page fault
            # when the weight sits at the end of an allocator segment (the intermittent abort of round 5's suite: a test that
            # passed a 32-channel input to a 16-channel weight)
            raise RuntimeError(f"convolution: input of shape {tuple(xs)} has {Cin} channels, weight of shape {tuple(ws)} expects "
                               f"{ws[1]} (groups are not on the C2M path)")
        Ti, Hi, Wi = (xs[2], xs[3], xs[4]) if nd == 3 else (1, xs[2], xs[3])
        Cout = ws[0]
        kt, kh, kw = (ws[2], ws[3], ws[4]) if nd == 3 else (1, ws[2], ws[3])
        st, sh, sw = stride
        pt, ph, pw = pad
        To, Ho, Wo = (Ti + 2 * pt - kt) // st + 1, (Hi + 2 * ph - kh) // sh + 1, (Wi + 2 * pw - kw) // sw + 1
        if min(To, Ho, Wo) <= 0:
            raise ValueError("empty convolution output")
        if kt * kh * kw > 128:
            raise NotImplementedError(f"conv kernels with more than 128 taps ({kt}x{kh}x{kw}) are not on the C2M path "
                                      "(c2m_pack_weights / the gather tables hold 128 tap offsets)")
        if reflect and (pt >= Ti and pt > 0 or ph >= Hi and ph > 0 or pw >= Wi and pw > 0):
            raise ValueError("reflect padding must be smaller than the input extent")
        if 4 * N * max(Cin * Ti * Hi * Wi, Cout * To * Ho * Wo) >= 2 ** 31:
            raise ValueError("tensor too large: the gather uses 32-bit byte offsets (< 2 GiB per tensor)")
        self.dims = (N, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw)
        # dgrad_rows: only the first dgrad_rows input channels need a gradient (the rest of a concatenated input is a
        # tensor without grad, e.g. the rastered sparse motion in front of final_fuse): the data-gradient GEMM then has
        # dM rows instead of Cin -- 32 instead of 34 there, which is one 32-row MFMA tile instead of a half-empty 64
        dM = self.dM = int(dgrad_rows) if dgrad_rows and tuple(stride) == (1, 1, 1) and 0 < dgrad_rows < Cin else Cin
        self.stride, self.pad, self.reflect = stride, pad, reflect
        self.out_shape = (N, Cout, To, Ho, Wo) if nd == 3 else (N, Cout, Ho, Wo)
        self.K = Cin * kt * kh * kw
        ly = _Layer(N, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw, nd, reflect, bf16, dM,
                    Ti * Hi * Wi, To * Ho * Wo, kt * kh * kw)
        self._plan_wino2d(ly, L)
        self._plan_wino3d(ly, L, device)
        self._plan_nc8(ly, device)
        offs = self._plan_forward(ly, L, device)
        self._plan_wgrad(ly, L, offs, device)
        self._plan_dgrad_classes(ly, L, device)
        self._plan_class_batching(ly, L)
        self._plan_g8(ly, offs, device)
        self._plan_routes()
        self._plan_call_constants(ly)

    def _fwd_on_patch_nc8(self):
        return self.fwd_patch and self.nc8

    def _dgrad_on_patch_nc8(self):
        """The single 3x3 stride-1 class of a bf16 layer whose dY planes are whole 8-pixel groups (a patch class is the only class)."""
        return bool(self.bf16 and _NC8 and self.classes and all(c["patch"] for c in self.classes) and not self.is3d and
                    (self.dims[7] * self.dims[8]) % 8 == 0)

    def _wino_wgrad_pays(self, ly, L, Kw, nimg):
        """Winograd weight gradient over Kw input channels (3-D: virtual (kt, ci)) and nimg images.  Sets wino_wg_splits where it pays."""
        Cout, Hi, Wi = ly.Cout, ly.Hi, ly.Wi
        wrows = 32 if Cout <= 32 else 64                      # workgroup tile: 64 (32 for Cout <= 32) output x 32 input channels
        wg_tiles = _cdiv(Kw, 32) * _cdiv(Cout, wrows)
        # A/B against the direct kernel (tools/ab_wino_wgrad.py, AB_EXTRA=1 for the marginal shapes): the Winograd form
        # wins 1.1-1.3x even on a half-empty 64-row tile as long as there are two tiles
        waste = 32.0 * wrows * wg_tiles / (Kw * Cout)
        if not (Hi % 2 == 0 and Wi % 16 == 0 and (Kw * Cout) % 4 == 0 and (_WINO_WGRAD == "force" or (
                _WINO_WGRAD == "auto" and (waste <= 1.35 or (waste <= 2.0 and wg_tiles >= 2))
                and nimg * (Hi // 2) * (Wi // 16) >= 8 * max(1, (768 if wrows == 32 else 512) // wg_tiles)))):
            return False
        self.wino_wg_splits = L.c2m_wino_wgrad_splits(Cout, Kw, nimg, Hi, Wi)
        return True

    def _plan_wino2d(self, ly, L):
        """Winograd F(2x2,3x3) / F(4x4,3x3) for the 3x3 stride-1 pad-1 2-D layers (fp32 mode): forward, weight gradient and data
        gradient.  Data gradient: zero padding -> the unpadded domain; reflect padding -> EITHER the exact H x W domain (the interior
        of the padded gradient = the zero-padded "same" data gradient, full Winograd regions) + the pad ring folded into dX
        by c2m_reflect_ring_dgrad (conv_ring.hip: four thin GEMMs, 3/9 (2H+2W)/(HW) of the layer's FLOPs -- maps of
        >= _RING_MIN_PIX pixels), OR the padded (H+2)x(W+2) domain with the two-target epilogue (interior straight into dX,
        pad ring into a scratch tensor that is then folded).
        Sets: wino_fwd, wino_dgrad, wino_wgrad, ring_dgrad, wino4_fwd, wino4_dgrad (all False unless the layer qualifies);
        wino_fwd_geom, wino_dgrad_geom, wino_wg_splits where their flag is set.  Reads: the layer only."""
        N, Cin, Cout, Hi, Wi, Ho, Wo, reflect, in_sc, osp = ly.N, ly.Cin, ly.Cout, ly.Hi, ly.Wi, ly.Ho, ly.Wo, ly.reflect, ly.in_sc, ly.osp
        self.wino_fwd = self.wino_dgrad = self.wino_wgrad = self.ring_dgrad = False
        self.wino4_fwd = self.wino4_dgrad = False         # F(4x4,3x3) instead of F(2x2,3x3) for that launch (2-D layers)
        if ly.bf16 or not ly.is_3x3_s1p1 or ly.nd != 2:
            return
        self.wino_wgrad = self._wino_wgrad_pays(ly, L, Cin, N)
        # regions per image: 8 x 16 outputs, or the th x tw tile shape c2m_conv_wino picks for a badly fitting domain
        if _wino_gate(N * L.c2m_wino_regions(Ho, Wo), N * Ho * Wo, 0.8, Cin, Cout):
            self.wino_fwd = True
            self.wino_fwd_geom = _wino_geom(m=Cout, k=Cin, nimg=N, hi=Hi, wi=Wi, ho=Ho, wo=Wo, iy0=-1, ix0=-1, reflect=int(reflect),
                                            in_sn=Cin * in_sc, in_sc=in_sc, in_sh=Wi, out_sn=Cout * osp, out_sc=osp, out_sh=Wo,
                                            x_bytes=4 * N * Cin * in_sc)
            self.wino4_fwd = _wino4_pays(L, Cout, Cin, N, Ho, Wo)
        dy = dict(m=Cin, k=Cout, nimg=N, hi=Ho, wi=Wo, in_sn=Cout * osp, in_sc=osp, in_sh=Wo, x_bytes=4 * N * Cout * osp)
        if reflect and ly.dM == Cin and _RING != "off" and Hi >= 4 and Wi >= 4 and (_RING == "force" or Hi * Wi >= _RING_MIN_PIX):
            w4e = _wino4_pays(L, Cin, Cout, N, Hi, Wi)
            # measured per shape in the step (profiles/r05_ab_ring_*): the route pays where the exact domain moves the layer to
            # F(4x4) (1.3-1.65x) and on the <= 32 x 64 maps whose padded domain wastes a third of the F(2x2) regions (1.14-1.26x);
            # F(2x2) layers on >= 64 x 128 maps (padded fill 0.8-0.9) gain less than the ring launch costs
            pays = _RING == "force" or w4e or Hi * Wi <= _RING_F2_MAX_PIX
            if pays and _wino_gate(N * L.c2m_wino_regions(Hi, Wi), N * Hi * Wi, 0.8, Cout, Cin):
                self.wino_dgrad = self.ring_dgrad = True
                self.wino_dgrad_geom = _wino_geom(ho=Hi, wo=Wi, iy0=-1, ix0=-1, out_sn=Cin * in_sc, out_sc=in_sc, out_sh=Wi, **dy)
                self.wino4_dgrad = w4e
        Hd, Wd = (Hi + 2, Wi + 2) if reflect else (Hi, Wi)
        if not self.ring_dgrad and ly.dM == Cin and _wino_gate(N * L.c2m_wino_regions(Hd, Wd), N * Hd * Wd, _WINO_DFIT, Cout, Cin):
            self.wino_dgrad = True
            o = -2 if reflect else -1
            self.wino_dgrad_geom = _wino_geom(ho=Hd, wo=Wd, iy0=o, ix0=o, out_sn=Cin * Hd * Wd, out_sc=Hd * Wd, out_sh=Wd,
                                              **dy, **_wino_interior(ly))
            self.wino4_dgrad = _wino4_pays(L, Cin, Cout, N, Hd, Wd)

    def _plan_wino3d(self, ly, L, device):
        """3x3x3 stride-1 pad-1 layers (fuse_convs, the 3-D blocks; fp32 mode): a 2-D Winograd over virtual input channels
        (time tap, channel) with image = (sample, frame) -- the K loop is three times as deep as the 2-D layer's, the
        temporal padding is a per-tap frame index (reflected, or a zero-record descriptor).  Data gradient: virtual
        channels (flipped time tap, output channel) of dY over the padded (T+2, H+2, W+2) domain (reflect; then one
        fold pass) or the unpadded one (zeros).
        Sets: wino3d, wino_wgrad3d, wino3d_pairs (always); wino_fwd, wino_dgrad, wino_wgrad, wino_fwd_geom, wino_dgrad_geom,
        wino_dgrad_target, wino_pair_tab, wino_wg_splits where the layer qualifies.  Reads: the layer only."""
        N, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, reflect, in_sc, osp = ly[:9] + (ly.reflect, ly.in_sc, ly.osp)
        self.wino3d = self.wino_wgrad3d = self.wino3d_pairs = False
        if ly.bf16 or ly.nd != 3 or not ly.is_333_s1p1:
            return
        if _wino_gate(N * To * L.c2m_wino_regions(Ho, Wo), N * To * Ho * Wo, 0.8, 3 * Cin, Cout):
            self.wino_fwd = self.wino3d = True
            self.wino_fwd_geom = _wino_geom(m=Cout, k=3 * Cin, nimg=N * To, hi=Hi, wi=Wi, ho=Ho, wo=Wo, iy0=-1, ix0=-1, reflect=int(reflect),
                                            in_sn=Cin * in_sc, in_sc=in_sc, in_sh=Wi, out_sn=Cout * osp, out_sc=osp, out_sh=Wo,
                                            x_bytes=4 * N * Cin * in_sc, to=To, in_st=Hi * Wi, out_st=Ho * Wo, cin=Cin, nkt=3, toff=-1,
                                            ti=Ti, treflect=int(reflect))
        Td, Hd, Wd = (Ti + 2, Hi + 2, Wi + 2) if reflect else (Ti, Hi, Wi)
        if _wino_gate(N * Td * L.c2m_wino_regions(Hd, Wd), N * Td * Hd * Wd, _WINO_DFIT, 3 * Cout, ly.dM):
            self.wino_dgrad = self.wino3d = True
            o = -2 if reflect else -1
            # reflect in time: launched over the Ti real frames with the pad frames' contributions as extra (frame, tap)
            # pairs of the frames they mirror onto (kernel: WinoP::ptab) -- not over Ti + 2 frames + a fold in time
            self.wino3d_pairs = bool(reflect and Cout % 8 == 0 and To == Ti and Ti >= 2)
            Tl = Ti if self.wino3d_pairs else Td
            self.wino_dgrad_target = (N, Cin, Tl, Hd, Wd)
            pairs = {}
            if self.wino3d_pairs:
                self.wino_pair_tab = torch.from_numpy(_time_pair_table(Ti).reshape(-1)).to(device)
                # every launched frame is a real one: the two-target epilogue of the 2-D layers applies per frame (interior
                # straight into dX, only the pad ring into the scratch tensor; then the border-only fold)
                pairs = dict(_wino_interior(ly), ptab=self.wino_pair_tab.data_ptr())
            self.wino_dgrad_geom = _wino_geom(m=ly.dM, k=3 * Cout, nimg=N * Tl, hi=Ho, wi=Wo, ho=Hd, wo=Wd, iy0=o, ix0=o,
                                              in_sn=Cout * osp, in_sc=osp, in_sh=Wo, out_sn=Cin * Tl * Hd * Wd, out_sc=Tl * Hd * Wd, out_sh=Wd,
                                              x_bytes=4 * N * Cout * osp, to=Tl, in_st=Ho * Wo, out_st=Hd * Wd, cin=Cout, nkt=3, toff=o,
                                              ti=To, **pairs)
        # weight gradient: the 2-D Winograd wgrad kernel over images (sample, frame) and virtual channels (kt, ci)
        self.wino_wgrad = self.wino_wgrad3d = self._wino_wgrad_pays(ly, L, 3 * Cin, N * Ti)

    def _plan_nc8(self, ly, device):
        """Which NC8 patch kernels (conv_nc8.hip, bf16 mode) can take the layer.
        Sets: nc8, k333_nc8, k333_wgrad_nc8, k333_dgrad_nc8, s2_nc8, s2_dgrad_nc8, s2_wgrad_nc8, wgrad_nc8 (always); k333_ptab
        where k333_dgrad_nc8.  Reads: the layer only."""
        N, Cin, Cout, Hi, Wi, Ho, Wo, reflect, dM = ly.N, ly.Cin, ly.Cout, ly.Hi, ly.Wi, ly.Ho, ly.Wo, ly.reflect, ly.dM
        # channel-blocked input: 2-D bf16 patch layers whose planes are whole 8-pixel groups
        self.nc8 = bool(ly.bf16 and _NC8 and ly.nd == 2 and (Hi * Wi) % 8 == 0 and (Ho * Wo) % 8 == 0)
        # ... the 3x3x3 stride-1 pad-1 layers as (sample, frame) images with (time tap, channel) chunks: forward and weight gradient
        # (channel padding up to 45 %: final_fuse has 34 input channels = three 16-channel chunks, still 2x the gather kernel)
        k333 = bool(ly.bf16 and _NC8 and ly.nd == 3 and ly.is_333_s1p1 and (Hi * Wi) % 8 == 0 and ly.Ti >= 2 and _chan16_ok(Cin, 1.45) and
                    Wo >= 32 and Ho >= 8 and _fill_ok(Ho, Wo, _NC8_FILL))
        self.k333_nc8 = k333 and Cout > 4
        self.k333_wgrad_nc8 = k333 and Cout >= 64 and Cin >= 16
        pd = 1 if reflect else 0
        self.k333_dgrad_nc8 = bool(k333 and _chan16_ok(Cout, 1.25) and dM > 4 and _fill_ok(Hi + 2 * pd, Wi + 2 * pd, _NC8_FILL))
        if self.k333_dgrad_nc8:
            self.k333_ptab = torch.from_numpy(_time_pair_table_kt(ly.Ti, bool(reflect)).reshape(-1)).to(device)
        # ... the 4x4 stride-2 pad-1 layers on the parity-plane form of the patch kernel (forward).  Half-filled tiles (8 x 16 output maps)
        # go to the NC8 gather form where it can take the layer: 40 vs 59 us on 256 -> 512 at 16x32, but 42 vs 36 us on 128 -> 256 at
        # 32x64 whose tiles are full (profiles/r04_ab_nc8.txt)
        # (only launches with >= 4096 output pixels: below that the gather form needs deep K splits -- configs[2]'s 20-image batches of
        # the same layers measured +0.7 ms with the gather form, configs[3]'s 40-image batches -0.7 ms)
        g8_in = bool(_G8 and _chan16_ok(Cin, 1.45) and ly.in_sc % 8 == 0 and N * ly.osp >= 4096)
        g8_out = bool(_G8 and _chan16_ok(Cout, 1.45) and ly.osp % 8 == 0 and N * ly.osp >= 4096)
        s2 = self.nc8 and ly.is_4x4_s2p1_even
        self.s2_nc8 = bool(s2 and Cout > 4 and Cin >= 12 and Wo >= 16 and Ho >= 4 and
                           _fill_ok(Ho, Wo, _NC8_S2_FILL_G8 if g8_in else _NC8_FILL))
        # ... their data gradient (four output parity classes over one shared dY patch, one launch)
        qh, qw = Hi // 2 + pd, Wi // 2 + pd
        self.s2_dgrad_nc8 = bool(s2 and Cin >= 8 and Cout >= 12 and qw >= 16 and dM == Cin and
                                 _fill_ok(qh, qw, _NC8_S2_FILL_G8 if (g8_out and dM > 4) else _NC8_FILL))
        self.s2_wgrad_nc8 = bool(s2 and Cout >= 64 and Cin >= 16 and
                                 N * Ho * Wo >= _NC8_S2_WGRAD_MIN_PIX)      # (the few-pixel encoder tails: one or two chunks per split, slabs dominate)
        # ... and the weight gradient of the 3x3 stride-1 pad-1 layers from the NC8 forms of X and dY (transposed LDS reads)
        self.wgrad_nc8 = bool(self.nc8 and ly.is_3x3_s1p1 and Cout >= 64 and Cin >= 16)      # (Cout = 32: half of a 64-row tile is padding -- 88 vs 145 TF/s on the NCHW kernel)

    def _plan_forward(self, ly, L, device):
        """The direct (implicit-GEMM / LDS-patch) forward launch; returns the tap offsets for the stages that share them.
        Sets: ck, fwd_patch, nk, fwd_tab, fwd_splits, fwd_geom.  Reads: nc8."""
        N, Cin, Cout, Ho, Wo, kt, kh, kw, in_sc, osp = ly.N, ly.Cin, ly.Cout, ly.Ho, ly.Wo, ly.kt, ly.kh, ly.kw, ly.in_sc, ly.osp
        self.fwd_patch = ly.k == (1, 3, 3) and (_patch_bf16_ok(Cin, ly.stride, Ho, Wo, Cout, None, self.nc8) if ly.bf16 else
                                                _patch_ok(Cin, ly.k, ly.stride, 1, Ho, Wo, Cout))
        self.ck = ck = 16 if self.fwd_patch else _choose_ck(Cin, ly.taps)
        offs = _tap_offsets(kt, kh, kw, np.arange(kt) - ly.pt, np.arange(kh) - ly.ph, np.arange(kw) - ly.pw)
        tab, nch, ntg = _kstep_table(Cin, offs, in_sc, ck)
        self.nk = nk = nch * ntg
        self.fwd_tab = torch.from_numpy(tab.reshape(-1)).to(device)
        self.fwd_splits = _patch_splits(L, Cout, Cin, N * osp, ly.bf16) if self.fwd_patch else \
            _splits(L, Cout, nk, N * osp, ly.bf16)
        self.fwd_geom = _geom(M=Cout, nk=nk, lda=nk * 16, Npix=N * osp, To=ly.To, Ho=Ho, Wo=Wo, Ti=ly.Ti, Hi=ly.Hi, Wi=ly.Wi, st=ly.st,
                              sh=ly.sh, sw=ly.sw, in_sn=Cin * in_sc, in_st=ly.Hi * ly.Wi, in_sh=ly.Wi, out_sn=Cout * osp, out_sc=osp,
                              out_st=Ho * Wo, out_sh=Wo, out_sw=1, out_off=0, reflect=int(ly.reflect), is3d=self.is3d, ns=16 // ck,
                              in_sc=in_sc, splits=self.fwd_splits, slab_stride=N * Cout * osp, x_bytes=4 * N * Cin * in_sc,
                              Cin=Cin, taps=ly.taps, ntg=ntg, precision=int(ly.bf16))      # (precision: read by c2m_conv_igemm / c2m_conv_wgrad)
        if kt == 1 and kh == kw and ly.stride == (1, 1, 1):
            self.fwd_geom[G.SQUARE_KW] = kw              # row-major square tap set, dx ascending (thin row-blocked kernel)
        if self.fwd_patch:
            _set_patch(self.fwd_geom, -ly.ph, -ly.pw, (0, 1, 2), (0, 1, 2))
            if ly.bf16:
                self.fwd_geom[G.LDA] = _ceil(Cout, 128)       # lda = padded row count of the bf16 weight image
        return offs

    def _plan_wgrad(self, ly, L, offs, device):
        """The direct weight gradient: the forward's (chunk, tap group) row order + a ones group (bias gradient) + zero groups up to
        the tile.  Sets: J, wg_tab, wg_geom, wg_splits.  Reads: ck, nk, fwd_geom."""
        N, Cout, Wi, Wo, kw, osp, nk = ly.N, ly.Cout, ly.Wi, ly.Wo, ly.kw, ly.osp, self.nk
        self.J = L.c2m_conv_wgrad_rows(Cout, nk + 1)
        wtab, _, _ = _kstep_table(ly.Cin, offs, ly.in_sc, self.ck, extra_groups=self.J // 16 - nk - 1, ones_group=True)
        self.wg_tab = torch.from_numpy(wtab.reshape(-1)).to(device)
        self.wg_geom = self.fwd_geom.copy()      # (M rows of dY with the output's strides; Cin, taps, tap groups: the forward's)
        self.wg_geom[[G.PATCH, G.NK, G.NGROUPS, G.DY_BYTES]] = (0, self.J, nk, 4 * N * Cout * osp)      # (wgrad: J rows, nk of them K-step groups)
        # bf16 data path: the 16-byte-load weight-gradient kernel (conv_wgrad_wide_bf16_kernel) takes layers whose 8-pixel
        # groups stay inside an input row up to one pad pixel: unit x stride, same-width output, |tap dx| <= 1
        self.wg_geom[G.WGRAD_WIDE] = int(ly.bf16 and ly.sw == 1 and Wi == Wo and Wo % 8 == 0 and Wi >= 8 and kw in (1, 3)
                                         and ly.pw == (kw - 1) // 2 and osp % 8 == 0)
        # ... and its stride-2 form (4-wide taps, pad 1: dx = -1 .. 2; every second element of a 16-element run)
        if ly.bf16 and ly.sw == 2 and Wi == 2 * Wo and Wo % 8 == 0 and kw == 4 and ly.pw == 1 and osp % 8 == 0:
            self.wg_geom[G.WGRAD_WIDE] = 2
        self.wg_splits = L.c2m_conv_wgrad_splits(Cout, self.J, N * osp)

    def _plan_dgrad_classes(self, ly, L, device):
        """The direct data gradient: one launch per stride-parity class, with the split count the classes share.
        Sets: dgrad_target, dgrad_needs_zero, classes (dicts: r, taps, ck, nk, npix, patch, tab, geom, offs), dgrad_splits,
        fwd_flops, dgrad_flops, dgrad_work.  Reads: K."""
        N, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw, _, reflect, bf16, dM, in_sc, osp, _ = ly
        Tp, Hp, Wp = (Ti + 2 * pt, Hi + 2 * ph, Wi + 2 * pw) if reflect else (Ti, Hi, Wi)
        self.dgrad_target = (N, Cin, Tp, Hp, Wp)
        self.dgrad_needs_zero = False
        self.classes = []

        def dim_classes(I, O, k, s, p):
            Ip = I + 2 * p if reflect else I
            out = []
            for r in range(s):
                A = len(range(r, k, s))
                if reflect:
                    qmin, qmax, off = 0, (Ip - 1 - r) // s, r
                else:
                    qmin = max(0, -((r - p) // s))      # ceil((p - r)/s)
                    qmax = (I - 1 + p - r) // s
                    off = s * qmin + r - p
                Q = qmax - qmin + 1
                if Q <= 0:
                    continue
                if A == 0:
                    self.dgrad_needs_zero = True
                    continue
                out.append((r, A, qmin, Q, off))
            return out

        tgt_numel = N * Cin * Tp * Hp * Wp
        for (rt, At, qt, Qt, offt) in dim_classes(Ti, To, kt, st, pt):
            for (ry, Ay, qy, Qy, offy) in dim_classes(Hi, Ho, kh, sh, ph):
                for (rx, Ax, qx, Qx, offx) in dim_classes(Wi, Wo, kw, sw, pw):
                    ctaps = At * Ay * Ax
                    cpatch = (At, Ay, Ax) == (1, 3, 3) and (st, sh, sw) == (1, 1, 1) and \
                        (_patch_bf16_ok(Cout, (1, 1, 1), Qy, Qx, dM, _NC8_DGRAD_FILL if (reflect and _G8) else None,
                                        not self.is3d and (Ho * Wo) % 8 == 0) if bf16 else
                         _patch_ok(Cout, (At, Ay, Ax), (1, 1, 1), 1, Qy, Qx, dM))
                    cck = 16 if cpatch else _choose_ck(Cout, ctaps)
                    coffs = _tap_offsets(At, Ay, Ax, qt - np.arange(At), qy - np.arange(Ay), qx - np.arange(Ax))
                    ctab, cnch, cntg = _kstep_table(Cout, coffs, osp, cck)
                    cnk = cnch * cntg
                    npix = N * Qt * Qy * Qx
                    geom = _geom(M=dM, nk=cnk, lda=cnk * 16, Npix=npix, To=Qt, Ho=Qy, Wo=Qx, Ti=To, Hi=Ho, Wi=Wo, st=1,
                                 sh=1, sw=1, in_sn=Cout * osp, in_st=Ho * Wo, in_sh=Wo, out_sn=Cin * Tp * Hp * Wp,
                                 out_sc=Tp * Hp * Wp, out_st=st * Hp * Wp, out_sh=sh * Wp, out_sw=sw,
                                 out_off=offt * Hp * Wp + offy * Wp + offx, reflect=0, is3d=self.is3d, ns=16 // cck,
                                 in_sc=osp, splits=1, slab_stride=tgt_numel, x_bytes=4 * N * Cout * osp,
                                 Cin=Cout, taps=ctaps, ntg=cntg, precision=int(bf16))
                    # two-target epilogue (reflect): padded coord = q*stride + r per dim; interior = [pad, pad + extent)
                    geom[G.PS_T:G.Y2_SH + 1] = (st, sh, sw, offt, offy, offx, pt, ph, pw, Ti, Hi, Wi, Cin * in_sc, in_sc, Hi * Wi, Wi)
                    if At == 1 and Ay == Ax and (st, sh, sw) == (1, 1, 1):
                        geom[G.SQUARE_KW] = -Ax            # data gradient: tap offsets run q - arange(A): dx descending
                    if cpatch:
                        _set_patch(geom, qy - 2, qx - 2, (2, 1, 0), (2, 1, 0))
                        if bf16:
                            geom[G.LDA] = _ceil(dM, 128)
                    self.classes.append(dict(r=(rt, ry, rx), taps=ctaps, ck=cck, nk=cnk, npix=npix, patch=cpatch,
                                             tab=torch.from_numpy(ctab.reshape(-1)).to(device), geom=geom, offs=coffs))
        # common split count for all classes (they share one slab set); fall back to 1 if they cannot agree
        S = min(_splits(L, dM, c["nk"], c["npix"], bf16) for c in self.classes) if self.classes else 1
        if S > 1 and any(_cdiv(c["nk"], _cdiv(c["nk"], S)) != S for c in self.classes):
            S = 1
        if any(c["patch"] for c in self.classes):        # stride-1 3x3: a single class
            S = _patch_splits(L, dM, Cout, self.classes[0]["npix"], bf16)
        self.dgrad_splits = S
        for c in self.classes:
            c["geom"][G.SPLITS] = S
        # Algorithmic FLOPs (roofline bookkeeping): the data gradient of a convolution has the MACs of its forward
        # (2 * Cout * K * output pixels -- FlopCounterMode's count).  Reflect-padded layers LAUNCH over the
        # padded domain; every launch is credited with its share of the forward count, not with the padded volume.
        self.fwd_flops = 2.0 * Cout * self.K * N * osp
        self.dgrad_flops = self.fwd_flops * dM / Cin
        self.dgrad_work = float(sum(c["taps"] * c["npix"] for c in self.classes)) or 1.0

    def _plan_class_batching(self, ly, L):
        """Class batching: the stride parity classes of a k % s == 0 conv share every dimension (same taps per class, same Q extents)
        and differ only in weights, tap table and output origin -> ONE launch (blockIdx.z = class), which fills the chip where a
        single class (1/s^d of the pixels) cannot.
        Sets: classes_packable, cls_batch (None, or a dict: groups (dicts: geom, tab, ncls, first, npix), ncls, ck, taps, nk); with
        cls_batch, dgrad_splits again.  Reads: classes, dgrad_needs_zero."""
        Cin, st, sh, sw = ly.Cin, ly.st, ly.sh, ly.sw
        self.cls_batch = None
        cl = self.classes
        ncls = st * sh * sw
        whole = len(cl) == ncls and ly.kt % st == 0 and ly.kh % sh == 0 and ly.kw % sw == 0      # every parity class, each with k / s taps per dim
        self.classes_packable = whole and len({(c["ck"], c["taps"]) for c in cl}) == 1 and \
            [c["r"] for c in cl] == [(a, b, c_) for a in range(st) for b in range(sh) for c_ in range(sw)]
        if 1 < ncls <= 8 and whole and not self.dgrad_needs_zero and not any(c["patch"] for c in cl) and \
                len({(c["nk"], c["ck"], c["taps"]) for c in cl}) == 1:
            key = lambda c: (c["npix"],) + tuple(int(v) for v in c["geom"][G.TO:G.WO + 1])
            runs, i = [], 0
            while i < ncls:                       # maximal runs of consecutive classes with identical extents
                j = i
                while j + 1 < ncls and key(cl[j + 1]) == key(cl[i]):
                    j += 1
                runs.append((i, j + 1))
                i = j + 1
            nk0, ck0 = cl[0]["nk"], cl[0]["ck"]
            SB = min(_splits(L, Cin, nk0, cl[a]["npix"] * (b - a), ly.bf16) for a, b in runs)
            groups = []
            for a, b in runs:
                g = cl[a]["geom"].copy()
                g[G.SPLITS] = SB
                g[G.NCLS], g[G.A_CLS], g[G.KTAB_CLS] = b - a, Cin * nk0 * 16, nk0 * (1 + 16 // ck0)
                assert b - a <= 8                     # C2M_G_MAX_CLS (checked against the flag entries in c2m_geom.h)
                for i in range(a, b):
                    g[G.CLS_OUT_OFF + i - a] = cl[i]["geom"][G.OUT_OFF]
                    po = G.CLS_PO + 3 * (i - a)
                    g[po:po + 3] = cl[i]["geom"][G.PO_T:G.PO_X + 1]
                groups.append(dict(geom=g, tab=torch.cat([c["tab"] for c in cl[a:b]]), ncls=b - a, first=a,
                                   npix=cl[a]["npix"]))
            if len(groups) < ncls:
                self.cls_batch = dict(groups=groups, ncls=ncls, ck=ck0, taps=cl[0]["taps"], nk=nk0)
                self.dgrad_splits = SB

    def _plan_g8(self, ly, offs, device):
        """NC8 gather form (conv_gather_nc8_kernel) of every bf16 forward / data gradient the NC8 patch forms do not take: the same
        launches (geometry, classes, two-target epilogue, split-K) with channel-blocked input, a compact tap table and bf16 weights in
        (tap, chunk) order.  Channel padding up to 45 % (34 -> 48); <= 4 output rows stay on the vector-ALU kernels.
        Sets: g8_fwd, g8_dgrad (always); g8_fwd_splits, g8_fwd_geom, g8_fwd_tab where g8_fwd; g8_a_cls, g8_dgrad_splits and, on every
        class and batch group, "g8" and "g8tab" where g8_dgrad.  Reads: the NC8 flags, fwd_patch, fwd_geom, classes, classes_packable,
        cls_batch; offs: the forward's tap offsets."""
        N, Cin, Cout, dM, osp, taps, cl = ly.N, ly.Cin, ly.Cout, ly.dM, ly.osp, ly.taps, self.classes
        g8 = bool(ly.bf16 and _NC8 and _G8)
        self.g8_fwd = bool(g8 and not (self.k333_nc8 or self.s2_nc8 or self._fwd_on_patch_nc8()) and Cout > 4 and _chan16_ok(Cin, 1.45)
                           and ly.in_sc % 8 == 0 and taps <= 64)
        if self.g8_fwd:
            self.g8_fwd_splits = _g8_splits(Cout, taps * _cdiv(Cin, 16), N * osp)
            self.g8_fwd_geom = _g8_geom(self.fwd_geom, Cin, taps, self.g8_fwd_splits)
            self.g8_fwd_tab = _g8_taps(offs, device)
        self.g8_dgrad = bool(g8 and cl and not (self.k333_dgrad_nc8 or self.s2_dgrad_nc8 or self._dgrad_on_patch_nc8()) and dM > 4
                             and _chan16_ok(Cout, 1.45) and osp % 8 == 0 and self.classes_packable and max(c["taps"] for c in cl) <= 64 and
                             not any(c["patch"] for c in cl))      # (a patch class off the 8-pixel grid: the NCHW patch kernel)
        if self.g8_dgrad:
            ctaps = cl[0]["taps"]
            nk8 = ctaps * _cdiv(Cout, 16)
            self.g8_a_cls = nk8 * 2 * _ceil(dM, 128) * 16          # bytes of one class image
            S8 = min(_g8_splits(dM, nk8, grp["npix"], grp["ncls"]) for grp in self.cls_batch["groups"]) if self.cls_batch is not None else \
                min(_g8_splits(dM, nk8, c["npix"]) for c in cl)
            if S8 > 1 and _cdiv(nk8, _cdiv(nk8, S8)) != S8:
                S8 = 1
            self.g8_dgrad_splits = S8
            for c in cl:
                c["g8"] = _g8_geom(c["geom"], Cout, ctaps, S8)
                c["g8tab"] = _g8_taps(c["offs"], device)
            for grp in (self.cls_batch["groups"] if self.cls_batch else ()):
                grp["g8"] = _g8_geom(grp["geom"], Cout, ctaps, S8)
                grp["g8"][G.A_CLS], grp["g8"][G.KTAB_CLS] = 0, 0
                grp["g8tab"] = torch.cat([c["g8tab"] for c in cl[grp["first"]:grp["first"] + grp["ncls"]]])

    def _plan_routes(self):
        """The kernel each pass of this layer runs on, by name (_ROUTE_PROF lists them).  The eligibility flags are read HERE only, in
        order of precedence (the NC8 flags hold `bf16` themselves, the Winograd ones `not bf16`); dispatch, the NC8-only predicates
        and the NC8 keep decisions read the names.  Knobs (_NC8, _G8, _WINO, ...) are fixed when the plan is built.
        Sets: fwd_route, dgrad_route, wgrad_route, keep_x_nc8, keep_dy_nc8.  Reads: every eligibility flag, cls_batch, classes."""
        self.fwd_route = (("wino3d" if self.wino3d else "wino4" if self.wino4_fwd else "wino") if self.wino_fwd else
                          "k333_nc8" if self.k333_nc8 else "s2_nc8" if self.s2_nc8 else "g8" if self.g8_fwd else
                          "patch_nc8" if self._fwd_on_patch_nc8() else "igemm")
        self.dgrad_route = (("wino3d" if self.wino3d else ("wino4" if self.wino4_dgrad else "wino") + ("_ring" if self.ring_dgrad else ""))
                            if self.wino_dgrad else
                            "k333_nc8" if self.k333_dgrad_nc8 else "s2_nc8" if self.s2_dgrad_nc8 else "g8" if self.g8_dgrad else
                            "igemm_batched" if self.cls_batch is not None else "patch_nc8" if self._dgrad_on_patch_nc8() else "igemm")
        self.wgrad_route = ("k333_nc8" if self.k333_wgrad_nc8 else "nc8" if self.wgrad_nc8 else "s2_nc8" if self.s2_wgrad_nc8 else
                            "wino3d" if self.wino_wgrad3d else "wino" if self.wino_wgrad else "igemm")
        # X in NC8 form goes from the forward launch to the weight gradient (ctx.nc8_keep); dY in NC8 form is shared by the two gradients
        # of a backward node (`keep`)
        self.keep_x_nc8 = self.fwd_route in _NC8_KEEPS_X and self.wgrad_route in _NC8_WGRADS
        self.keep_dy_nc8 = self.dgrad_route in _NC8_CONVS or self.wgrad_route in _NC8_WGRADS

    def _plan_call_constants(self, ly):
        """What is the same for every call.  bf16 data path: bf16 in, bf16 out, except the <= 4-channel heads (flow, occlusion, RGB):
        fp32 out, and fp32 in on the vector-ALU kernels when the launch is big enough for them (_thin).
        Sets: fwd_xdt, fwd_ydt, in_shape, dgrad_route_splits, dgrad_folded, dgrad_two_target, "thin" on every class, fwd_prof,
        dgrad_prof, wgrad_prof.  Reads: the routes, fwd_splits, g8_fwd_splits, dgrad_splits, g8_dgrad_splits, wg_splits,
        dgrad_needs_zero, cls_batch, classes, dims, stride, pad, K."""
        N, Cin, Cout, bf16, osp = ly.N, ly.Cin, ly.Cout, ly.bf16, ly.osp
        thin = bool(bf16 and _thin(Cout, self.fwd_splits, N * osp))
        self.fwd_xdt = BF16 if (bf16 and not thin) else torch.float32
        self.fwd_ydt = BF16 if (bf16 and not thin and Cout > 4) else torch.float32
        self.in_shape = (N, Cin, ly.Ti, ly.Hi, ly.Wi) if ly.nd == 3 else (N, Cin, ly.Hi, ly.Wi)
        S = self.dgrad_route_splits = self.g8_dgrad_splits if self.dgrad_route == "g8" else self.dgrad_splits
        self.dgrad_folded = bool(ly.reflect and any(self.pad))
        self.dgrad_two_target = self.dgrad_folded and S == 1 and not self.dgrad_needs_zero
        for c in self.classes:        # (a <= 4-channel input: such launches are fp32 in, fp32 out, and then the layer's target is fp32)
            c["thin"] = bool(bf16 and self.cls_batch is None and _thin(ly.dM, S, c["npix"], self.dgrad_two_target))
        def prof(table, route, splits, *head):         # (profiler kind, tag) -- the data gradient's tag: its tail, per launch
            kind, sfx = _ROUTE_PROF[table][route]
            return kind + ("_bf16" if bf16 else ""), head + (self.dims[9:12], self.stride, ly.reflect) + tuple(splits if v is None else v for v in sfx)
        self.fwd_prof = prof("conv", self.fwd_route, self.g8_fwd_splits if self.g8_fwd else self.fwd_splits, "fwd", Cout, self.K, N * osp)
        self.dgrad_prof = prof("conv", self.dgrad_route, S)
        self.wgrad_prof = prof("wgrad", self.wgrad_route, self.wg_splits, "wgrad", Cout, self.K, N * osp)


# route -> (profiler kind, tag suffix; None = the launch's split count): what bench.py (sums by kind) and the tools (read tag positions)
# see of a route.  Launches of a bf16 plan are kind + "_bf16" (the NC8 routes exist in bf16 only, the Winograd ones in fp32 only).
_ROUTE_PROF = {
    "conv": {       # forward and data gradient (*_ring, igemm_batched: data gradient only)
        "wino3d": ("wino", ("wino",)), "wino4": ("wino4", ("wino4",)), "wino": ("wino", ("wino",)),
        "wino4_ring": ("wino4", ("wino4", "ring")), "wino_ring": ("wino", ("wino", "ring")),
        "k333_nc8": ("igemm", ("nc8",)), "s2_nc8": ("igemm", ("nc8",)), "g8": ("igemm", (None, "nc8g")),
        "patch_nc8": ("igemm", (None, "nc8")), "igemm_batched": ("igemm", (None,)), "igemm": ("igemm", (None,))},
    "wgrad": {
        "k333_nc8": ("wgrad", ("nc8",)), "nc8": ("wgrad", ("nc8",)), "s2_nc8": ("wgrad", ("nc8",)),
        "wino3d": ("wino_wgrad", ("wino",)), "wino": ("wino_wgrad", ("wino",)), "igemm": ("wgrad", (None,))},
}
_NC8_CONVS = frozenset(("k333_nc8", "s2_nc8", "g8", "patch_nc8"))      # forward: reads X as NC8 only; data gradient: reads dY as NC8 only
_NC8_KEEPS_X = _NC8_CONVS - {"g8"}                                      # ... and hands its NC8 X on (the gather form converts for itself)
_NC8_WGRADS = frozenset(("k333_nc8", "nc8", "s2_nc8"))                  # weight gradient: reads X and dY as NC8 only


def _bwd_reads_only_nc8(pl, need_x, need_w):
    """True when every kernel of this bf16 layer's backward reads the output gradient in its NC8 form (conv_nc8.hip / the NC8 gather
    form): the gradient then need not exist in NCHW at all (`_virtual_grad`)."""
    if not (pl.bf16 and _NC8 and _NC8_GRAD and (pl.dims[6] * pl.dims[7] * pl.dims[8]) % 8 == 0):
        return False
    return not (need_x and pl.dgrad_route not in _NC8_CONVS) and not (need_w and pl.wgrad_route not in _NC8_WGRADS)


def _fwd_reads_only_nc8(pl, need_w):
    """True when the forward AND the weight gradient of this bf16 layer read the input in its NC8 form only (the data gradient never
    reads the input): an activation whose single consumer is this layer need not exist in NCHW (`feeds=` of the norm ops)."""
    if not (pl.bf16 and _NC8 and _NC8_GRAD and (pl.dims[3] * pl.dims[4] * pl.dims[5]) % 8 == 0):
        return False
    return pl.fwd_route in _NC8_CONVS and not (need_w and pl.wgrad_route not in _NC8_WGRADS)


def _consumer_reads_only_nc8(like, feeds):
    """`feeds` = conv_consumer(...) and `like` a tensor of the consumer's input shape / dtype: True when that convolution will read
    its input through NC8 kernels only AND in one piece -- `conv()` runs tensors past 2 GiB as batch chunks, i.e. on VIEWS of its
    input, which do not carry the NC8 form."""
    cw, cstride, cpad, cmode = feeds[:4]
    cb = feeds[4] if len(feeds) > 4 else None
    nd = like.dim() - 2
    stride3, pad3 = _triple(cstride, nd), _pad3(cpad, nd)
    if _chunks_for_2gib(like.shape, cw.shape, stride3, pad3) > 1:
        return False
    cpl = _plan(like, _f(cw), stride3, pad3, cmode == "reflect" and any(pad3), None)
    # (a frozen weight with a trainable bias still runs _ConvFn._wgrad -- the bias gradient comes out of the weight-gradient kernel)
    return _fwd_reads_only_nc8(cpl, cw.requires_grad or (cb is not None and cb.requires_grad))


def conv_consumer(conv_w, stride=1, padding=0, padding_mode="zeros", conv_b=None):
    """`feeds=` argument of batch_norm_act / instance_norm_act / spade_norm_act: the ONE convolution that consumes the op's result
    (the caller guarantees nothing else reads it -- `out = norm(x); out = conv(out)` inside a block).  Where that layer's forward and
    weight gradient run on NC8 kernels the result is produced in NC8 form only."""
    return (conv_w, stride, padding, padding_mode, conv_b)


def _virtual_grad(like, gn):
    """A gradient that exists in NC8 form only: a tensor object of the NCHW shape that carries `gn` for `_to_nc8` and whose own
    storage is never written or read (C2M_NC8_POISON=1 fills it with NaN -- the tests run the steps that way: a kernel that read
    it would poison the losses)."""
    g = torch.empty_like(like)
    if _NC8_POISON:
        g.fill_(float("nan"))
    return _mark_nc8_only(g, gn)


def _plan_for(xs, ws, stride, pad, reflect, device, dgrad_rows=None):
    """The cached plan of the convolution of an input of shape `xs` with a weight of shape `ws` in the current precision."""
    key = (xs, ws, stride, pad, reflect, device.index, _conv_bf16, dgrad_rows)
    pl = _geom_cache.get(key)
    if pl is None:
        pl = _geom_cache[key] = _ConvPlan(xs, ws, stride, pad, reflect, device, _conv_bf16, dgrad_rows)
    return pl


def _plan(x, w, stride, pad, reflect, dgrad_rows=None):
    return _plan_for(tuple(x.shape), tuple(w.shape), stride, pad, reflect, x.device, dgrad_rows)


def _gp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _wino_filter(w, Cout, Cin, dgrad):
    """c2m_wino_filter_transform: native [Cout][Cin][3][3] -> packed U = G g G^T fragments (dgrad: transposed, rotated)."""
    L = _lib.lib()
    M, K = (Cin, Cout) if dgrad else (Cout, Cin)
    U = torch.empty(L.c2m_wino_upack_floats(M, K), device=w.device, dtype=torch.float32)
    _lib.check(L.c2m_wino_filter_transform(_p(w), _p(U), Cout, Cin, dgrad, _stream()), "wino_filter_transform")
    return U


def _pack_native(w, M, C, ck, kdims, stride, s_m, s_c):
    """c2m_pack_weights: contiguous native weights -> [ncls*M, nk*16] packed rows (ncls = prod(stride))."""
    kt, kh, kw = kdims
    st, sh, sw = stride
    ns = 16 // ck
    taps = (kt // st) * (kh // sh) * (kw // sw)
    out = torch.empty(st * sh * sw * M, _cdiv(C, ck) * _cdiv(taps, ns) * 16, device=w.device, dtype=torch.float32)
    g = np.array([M, C, ck, kt, kh, kw, st, sh, sw, s_m, s_c], dtype=np.int64)
    _lib.check(_lib.lib().c2m_pack_weights(_p(w), _p(out), _gp(g), _stream()), "pack_weights")
    out._c2m_job = (0, g)                   # how to rebuild this pack in place (refresh_trainable_packs)
    return out


_frozen_pack_cache = {}       # (id(w), kind) -> (weakref(w), w._version, w.data_ptr(), packed)   [name kept from round 1]
_PACK_CACHE_LIMIT = 4096


def _packed(w, frozen, kind, build):
    """Packed weight matrix (K-order rows, Winograd U fragments, bf16 patch image ...), built once per weight VALUE: cached
    while the SAME tensor object is alive and unmodified (weak reference + `_version` + data pointer: a new tensor that
    happens to reuse a freed allocation never hits).  Frozen weights (the VGG-19 of the perceptual loss) are packed once per
    run; trainable weights once per optimizer step -- `c2m_amd.optim.Adam.step` (and every in-place torch update) bumps
    `_version` -- instead of once per call: the discriminators run three times per step, every layer's forward and data
    gradient layouts were rebuilt on every use (pack_weights 76 + wino_filter 94 launches per step in round 2).
    Under a HIP-graph capture trainable weights are re-packed INSIDE the graph and never cached: the graph is replayed after
    eager optimizer steps, and a pack tensor from the graph's private pool must not leak into eager code."""
    key = (id(w), kind)
    hit = _frozen_pack_cache.get(key)
    fresh = hit is not None and hit[0]() is w and hit[1] == w._version and hit[2] == w.data_ptr()
    if not frozen and w.is_cuda and torch.cuda.is_current_stream_capturing():
        # a pack that is kept fresh from outside the graph (refresh_trainable_packs after every optimizer step: same buffer,
        # new contents) is used as it is -- the graph then holds no pack kernels; pinned, because the graph keeps its address
        if fresh and key in _pack_jobs and _pack_jobs[key][3] is hit[3]:
            _capture_pins[id(hit[3])] = hit[3]
            return hit[3]
        return build()
    if fresh:
        return hit[3]
    # A registered pack of this very tensor that has gone stale outside the optimizer (load_state_dict, .copy_, a torch
    # optimizer): rebuild it IN PLACE.  A captured graph may hold the buffer's address (_capture_pins); a fresh allocation here
    # would leave that graph replaying the old weights for ever.
    job = _pack_jobs.get(key)
    if job is not None and hit is not None and job[0]() is w and hit[0]() is w and job[3] is hit[3] and \
            hit[2] == w.data_ptr():
        refresh_trainable_packs([w])
        return job[3]
    if len(_frozen_pack_cache) > _PACK_CACHE_LIMIT:
        for k in [k for k, v in _frozen_pack_cache.items() if v[0]() is None]:       # owners that died (e.g. the
            del _frozen_pack_cache[k]                                                  # per-forward spectral-norm weight)
        if len(_frozen_pack_cache) > _PACK_CACHE_LIMIT:
            _frozen_pack_cache.clear()
    A = build()
    _frozen_pack_cache[key] = (weakref.ref(w), w._version, w.data_ptr(), A)
    job = getattr(A, "_c2m_job", None)
    # (leaf tensors only: a weight derived per forward -- spectral norm's w / sigma -- dies with its step, and registering it would
    # throw the device tables away every step: +2-3 ms of host time per eager step when that was tried)
    if not frozen and job is not None and w.is_leaf and A.data_ptr() != w.data_ptr():
        _pack_jobs[key] = (weakref.ref(w), job[0], job[1], A)
        _pack_tables.clear()          # device job tables are keyed on (key, pointers): a new tensor may reuse both with another geometry
    return A


_pack_jobs = {}          # (id(w), kind) -> (weakref(w), job type, g, packed tensor): packs of trainable weights we know how to rebuild
_pack_tables = {}        # signature of a stale set -> (device job table, njobs, total workgroups)
_capture_pins = {}       # id -> pack whose address a captured graph holds (one entry per pack, however many captures)


def refresh_trainable_packs(params=None):
    """Rebuild, in ONE launch (c2m_pack_multi), every cached pack of a trainable weight whose weight has changed since it was
    packed -- called by c2m_amd.optim.Adam.step and before a HIP-graph replay.  The packs keep their buffers, so the ~195 pack
    launches a full G + D step used to spend on its first use of every layer after the optimizer step (1.3 ms of GPU time, more
    host time than that) become one, and a captured graph needs no pack kernels at all.  Returns the number of packs rebuilt."""
    if not _pack_jobs:
        return 0
    stale = []
    if params is None:
        items = list(_pack_jobs.items())
    else:                                   # the optimizer's own parameters only (host time: ~1.5 us per registered pack)
        ids = {id(p) for p in params}
        items = [(k, v) for k, v in _pack_jobs.items() if k[0] in ids]
    for key, (wref, typ, g, A) in items:
        w = wref()
        hit = _frozen_pack_cache.get(key)
        if w is None or hit is None or hit[3] is not A or hit[0]() is not w or hit[2] != w.data_ptr():
            del _pack_jobs[key]
            continue
        if hit[1] != w._version:
            stale.append((key, w, typ, g, A))
    if not stale:
        return 0
    L = _lib.lib()
    sig = tuple(id(A) for _, _, _, _, A in stale)         # packs stay alive while registered; tables die with any new registration
    tab = _pack_tables.get(sig)
    if tab is None:
        nb = L.c2m_pack_job_bytes()
        host = (ctypes.c_ubyte * (nb * len(stale)))()
        first = 0
        btab = []
        for i, (_, w, typ, g, A) in enumerate(stale):
            n = L.c2m_pack_job_fill(ctypes.addressof(host) + i * nb, typ, _p(w), _p(A), _gp(g), first)
            if n <= 0:
                raise RuntimeError("c2m_pack_job_fill: bad pack geometry")
            first += n
            btab.append(np.stack([np.full(n, i, dtype=np.int32), np.arange(n, dtype=np.int32)], 1))
        device = stale[0][1].device
        dev = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device)
        bdev = torch.from_numpy(np.concatenate(btab, 0)).to(device)
        if len(_pack_tables) > 16:
            _pack_tables.clear()
        tab = _pack_tables[sig] = (dev, len(stale), first, bdev)
    _lib.check(L.c2m_pack_multi(_p(tab[0]), _p(tab[3]), tab[1], tab[2], _stream()), "pack_multi")
    for key, w, _, _, A in stale:
        hit = _frozen_pack_cache[key]
        _frozen_pack_cache[key] = (hit[0], w._version, hit[2], A)
    return len(stale)


def _set_io(geom, x, ydt):
    """Per-call element types / bounds of a c2m_conv_igemm geom: X bytes (buffer range check), X type, Y type."""
    geom[G.X_BYTES] = x.numel() * x.element_size()
    geom[G.X_TYPE] = _dt(x)
    geom[G.Y_TYPE] = 1 if ydt == BF16 else 0
    return geom


def _dgrad_tag(pl, taps, npix):
    """(kind, tag) of one data-gradient launch: `taps` weights per (input, output) channel pair over `npix` pixels."""
    return pl.dgrad_prof[0], ("dgrad", pl.dims[1], pl.dims[2] * taps, npix) + pl.dgrad_prof[1]


def _dgrad_wino3d(pl, w, gy, frozen_w, out_dtype, keep):
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    Ti, Hi, Wi = pl.dims[3:6]
    dM = pl.dM
    # virtual channels (flipped time tap, output channel): a "native" [3*Cout][dM][3][3] weight for the 2-D transform
    U = _packed(w, frozen_w, ("wino-dgrad3d", dM), lambda: _wino_filter(
        w[:, :dM].flip(2).permute(2, 0, 1, 3, 4).reshape(3 * Cout, dM, 3, 3).contiguous(), 3 * Cout, dM, 1))
    gx = torch.empty(pl.in_shape, device=gy.device, dtype=torch.float32)
    tgt = torch.empty(pl.wino_dgrad_target, device=gy.device, dtype=torch.float32) if pl.reflect else gx
    g3 = pl.wino_dgrad_geom
    two = pl.reflect and pl.wino3d_pairs
    kind, tag = _dgrad_tag(pl, 27, int(g3[WG.NIMG] * g3[WG.HO] * g3[WG.WO]))
    _lib.check(_timed(kind, pl.dgrad_flops,
                      lambda: L.c2m_conv_wino(_p(U), _p(gy), _p(tgt), _p(gx) if two else None, None, _gp(g3), 0, 0.0, _stream()), tag,
                      4 * (gy.numel() + w.numel() + gx.numel())), "conv_wino dgrad 3-D")
    if pl.reflect:
        if two:
            _lib.check(L.c2m_reflect_border_add(_p(tgt), _p(gx), N * Cin, Ti, Hi, Wi, 0, 1, 1, 0, _stream()), "reflect border add 3-D")
        else:
            _lib.check(L.c2m_reflect_fold(_p(tgt), _p(gx), N * Cin, Ti, Hi, Wi, 1, 1, 1, 0, _stream()), "reflect fold 3-D")
    return gx


def _dgrad_wino(pl, w, gy, frozen_w, out_dtype, keep):
    """Routes wino / wino4 (zeros: the unpadded domain; reflect: the padded domain with the two-target epilogue) and wino_ring /
    wino4_ring (reflect: the exact domain + the pad ring, conv_ring.hip)."""
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    Ti, Hi, Wi = pl.dims[3:6]
    dev = gy.device
    g_ = pl.wino_dgrad_geom
    if pl.dgrad_route in ("wino4", "wino4_ring"):
        U, conv_wino = _packed(w, frozen_w, ("wino4-dgrad",), lambda: _wino4_filter(w, Cout, Cin, 1)), L.c2m_conv_wino4
    else:
        U, conv_wino = _packed(w, frozen_w, ("wino-dgrad",), lambda: _wino_filter(w, Cout, Cin, 1)), L.c2m_conv_wino
    gx = torch.empty(pl.in_shape, device=dev, dtype=torch.float32)
    kind, tag = _dgrad_tag(pl, 9, int(g_[WG.NIMG] * g_[WG.HO] * g_[WG.WO]))
    nbytes = 4 * (gy.numel() + w.numel() + gx.numel())
    if pl.dgrad_route in ("wino_ring", "wino4_ring"):
        # the interior term straight into gx, then the pad ring added in place -- both launches inside the timed region of this
        # layer's data gradient
        Ar = _packed(w, frozen_w, ("ring-dgrad",), lambda: _ring_pack(w, Cout, Cin))
        if _RING_BUFFER:
            # buffer form: the ring launch WRITES its terms (coalesced, no read-modify-write of dX, no corner part) and the
            # Winograd launch behind it adds them in its epilogue
            r_l = _ceil(max(Hi, Wi), 4)
            R = torch.empty(N * Cin * 4 * r_l, device=dev, dtype=torch.float32)

            def run_ring():
                rc = L.c2m_reflect_ring_buffer(_p(Ar), _p(gy), _p(R), N, Cout, Cin, Hi, Wi, r_l, _stream())
                g_[WG.RING], g_[WG.RING_L] = R.data_ptr(), r_l
                try:
                    return rc or conv_wino(_p(U), _p(gy), _p(gx), None, None, _gp(g_), 0, 0.0, _stream())
                finally:
                    g_[WG.RING], g_[WG.RING_L] = 0, 0
        else:
            def run_ring():
                rc = conv_wino(_p(U), _p(gy), _p(gx), None, None, _gp(g_), 0, 0.0, _stream())
                return rc or L.c2m_reflect_ring_dgrad(_p(Ar), _p(w), _p(gy), _p(gx), N, Cout, Cin, Hi, Wi, _stream())
        _lib.check(_timed(kind, pl.fwd_flops, run_ring, tag, nbytes), "conv_wino dgrad + reflect ring")
        return gx
    # reflect: ring of the padded domain -> tgt (only the ring is ever written or read), interior -> gx
    tgt = torch.empty(pl.dgrad_target, device=dev, dtype=torch.float32) if pl.reflect else gx
    _lib.check(_timed(kind, pl.fwd_flops,
                      lambda: conv_wino(_p(U), _p(gy), _p(tgt), _p(gx) if pl.reflect else None, None, _gp(g_), 0, 0.0, _stream()), tag,
                      nbytes), "conv_wino dgrad")
    if pl.reflect:
        _lib.check(L.c2m_reflect_border_add(_p(tgt), _p(gx), N * Cin, Ti, Hi, Wi, 0, 1, 1, 0, _stream()), "reflect border add")
    return gx


def _dgrad_nc8(pl, w, gy, frozen_w, out_dtype, keep):
    """Routes k333_nc8 (3x3x3 layers: (sample, frame) images, frame t summing its (dY frame, time tap) pairs) and s2_nc8 (4x4 stride-2
    layers: all four output parity classes in one launch) on the NC8 form of dY (conv_nc8.hip); reflect: spatially padded target + fold."""
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    Ti, Hi, Wi = pl.dims[3:6]
    gy_b = _as(gy, BF16)
    kdt = BF16 if out_dtype == BF16 else torch.float32
    gx = torch.empty(pl.in_shape, device=gy.device, dtype=kdt)
    if pl.dgrad_route == "k333_nc8":
        dM = pl.dM
        A = _packed(w, frozen_w, ("dgrad-bf16-k333", dM), lambda: _pack_bf16_k333(w, dM, Cout, dgrad=True, cin_total=Cin))
        tgt = torch.empty((N, Cin, Ti, Hi + 2, Wi + 2), device=gy.device, dtype=kdt) if pl.reflect else gx
        taps, what = 27, "conv3d_dgrad_nc8"

        def run():
            gyn = _to_nc8(gy_b, keep)
            return L.c2m_conv3d_dgrad_nc8(_p(A), _p(gyn), _p(tgt), _p(pl.k333_ptab), dM, Cin, Cout, N, Ti, Hi, Wi, int(pl.reflect),
                                          _dt(tgt), _stream())
    else:
        Ho, Wo = pl.dims[7:9]
        A = _packed(w, frozen_w, ("dgrad-bf16-s2", pl.reflect), lambda: _pack_bf16_patch(w, Cin, Cout, 16, Cin * 16, 4 if pl.reflect else 3))
        tgt = torch.empty(pl.dgrad_target, device=gy.device, dtype=kdt) if pl.reflect else gx
        taps, what = 16, "conv_s2_dgrad_nc8"

        def run():
            gyn = _to_nc8(gy_b, keep)
            return L.c2m_conv_s2_dgrad_nc8(_p(A), _p(gyn), _p(tgt), Cin, Cout, N, Ho, Wo, int(pl.reflect), _dt(tgt), _stream())
    kind, tag = _dgrad_tag(pl, taps, int(N * Ti * Hi * Wi))
    _lib.check(_timed(kind, pl.dgrad_flops, run, tag, 2 * (gy.numel() + gx.numel()) + 4 * w.numel()), what)
    if pl.reflect:
        _lib.check(L.c2m_reflect_fold(_p(tgt), _p(gx), N * Cin, Ti, Hi, Wi, 0, 1, 1, _dt(tgt), _stream()), "reflect fold (NC8, spatial)")
    return gx


def _dgrad_igemm(pl, w, gy, frozen_w, out_dtype, keep):
    """Routes igemm and patch_nc8 (one c2m_conv_igemm / c2m_conv_patch_nc8 launch per stride-parity class), igemm_batched (one per
    group of classes) and g8 (either, on the NC8 gather form): shared target, split-K slabs, reduction and reflect fold."""
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    route, S, two_target, cb = pl.dgrad_route, pl.dgrad_route_splits, pl.dgrad_two_target, pl.cls_batch
    alloc = torch.zeros if pl.dgrad_needs_zero else torch.empty
    dev = gy.device
    # bf16 data path: the bf16 kernels gather gy as bf16 and write `kdt`; the <= 4-row vector-ALU kernels (c["thin"]) are fp32 in,
    # fp32 out -- if any launch of this layer is one of those, the layer's target is fp32
    gy_b = gy_f = None
    kdt = torch.float32
    if pl.bf16:
        thin = [c["thin"] for c in pl.classes]
        kdt = BF16 if (out_dtype == BF16 and not any(thin)) else torch.float32
        if not all(thin):
            gy_b = _as(gy, BF16)
        if any(thin):
            gy_f = _as(gy, torch.float32)
    tgt = alloc(pl.dgrad_target, device=dev, dtype=kdt)
    gx = torch.empty(pl.in_shape, device=dev, dtype=kdt) if pl.dgrad_folded else tgt.view(pl.in_shape)
    gx2 = gx if two_target else None
    dst = tgt if S == 1 else alloc(S * tgt.numel(), device=dev, dtype=torch.float32)
    xnumel = gx.numel()
    kdims = kt, kh, kw = pl.dims[9:12]
    pack_all = (Cout, kdims, pl.stride, kt * kh * kw, Cin * kt * kh * kw)        # (every class image of the weights in one pack)
    kind = pl.dgrad_prof[0]
    if route == "g8":
        A8 = _packed(w, frozen_w, ("dgrad-bf16-g8", pl.dM, pl.stride), lambda: _pack_bf16_gather(w, pl.dM, *pack_all))
        launches = [(grp["g8"], grp["g8tab"], grp["first"], cb["taps"] * grp["npix"] * grp["ncls"], grp["npix"] * grp["ncls"])
                    for grp in cb["groups"]] if cb is not None else \
                   [(c["g8"], c["g8tab"], ci, c["taps"] * c["npix"], c["npix"]) for ci, c in enumerate(pl.classes)]
        for geom8, tab8, first, work, npix in launches:
            Ag = A8[first * pl.g8_a_cls:]

            def run_g8d():
                gyn = _to_nc8(gy_b, keep)
                _set_io(geom8, gyn, kdt)
                return L.c2m_conv_igemm(_p(Ag), _p(gyn), _p(dst), _p(gx2), None, _p(tab8), _gp(geom8), 0, 0.0, _stream())
            _lib.check(_timed(kind, pl.dgrad_flops * work / pl.dgrad_work, run_g8d, _dgrad_tag(pl, pl.classes[0]["taps"], npix)[1],
                              (2 * (gy.numel() + xnumel) + 4 * w.numel()) * work // int(pl.dgrad_work)),
                       "conv_igemm dgrad (NC8 gather)")
    elif route == "igemm_batched":
        A = _packed(w, frozen_w, ("dgrad-all", cb["ck"], pl.stride), lambda: _pack_native(w, Cin, Cout, cb["ck"], *pack_all[1:]))
        gin = gy_b if pl.bf16 else gy
        for grp in cb["groups"]:
            Ag = A[grp["first"] * Cin:]
            _set_io(grp["geom"], gin, kdt)
            _lib.check(_timed(kind, pl.dgrad_flops * cb["taps"] * grp["npix"] * grp["ncls"] / pl.dgrad_work,
                              lambda: L.c2m_conv_igemm(_p(Ag), _p(gin), _p(dst), _p(gx2), None, _p(grp["tab"]), _gp(grp["geom"]), 0, 0.0,
                                                       _stream()), _dgrad_tag(pl, cb["taps"], grp["npix"] * grp["ncls"])[1],
                              4 * (gy.numel() * grp["ncls"] // cb["ncls"] + w.numel() + xnumel * grp["ncls"] // cb["ncls"])),
                       "conv_igemm dgrad (batched classes)")
    else:
        st, sh, sw = pl.stride
        w5 = w if pl.is3d else w.unsqueeze(2)
        Aall = None
        if pl.classes_packable and not (pl.bf16 and all(c["patch"] for c in pl.classes)):
            Aall = _packed(w, frozen_w, ("dgrad-all", pl.classes[0]["ck"], pl.stride), lambda: _pack_native(
                w, Cin, Cout, pl.classes[0]["ck"], *pack_all[1:]))
        for ci, c in enumerate(pl.classes):
            rt, ry, rx = c["r"]
            A = _packed(w, frozen_w, ("dgrad-bf16-patch", pl.dM), lambda: _pack_bf16_patch(
                w, pl.dM, Cout, 9, Cin * 9)) if (c["patch"] and pl.bf16) else \
                Aall[ci * Cin:] if Aall is not None else _packed(
                w, frozen_w, ("dgrad", c["ck"], pl.stride, c["r"]), lambda: _pack_rows(
                    w5[:, :, rt::st, ry::sh, rx::sw].reshape(Cout, Cin, c["taps"]).transpose(0, 1), c["ck"]))
            gin = (gy_f if c["thin"] else gy_b) if pl.bf16 else gy
            _set_io(c["geom"], gin, torch.float32 if c["thin"] else kdt)
            _lib.check(_timed(kind, pl.dgrad_flops * c["taps"] * c["npix"] / pl.dgrad_work,
                              (lambda: _nc8_launch(L, A, gin, dst, gx2, None, c["geom"], 0, 0.0, keep)) if route == "patch_nc8" else
                              (lambda: L.c2m_conv_igemm(_p(A), _p(gin), _p(dst), _p(gx2), None, _p(c["tab"]), _gp(c["geom"]), 0, 0.0,
                                                        _stream())), _dgrad_tag(pl, c["taps"], c["npix"])[1],
                              4 * (gy.numel() + w.numel() + xnumel) // len(pl.classes)), "conv_igemm dgrad")
    if S > 1:
        _lib.check(L.c2m_splitk_reduce(_p(dst), _p(tgt), None, tgt.numel(), S, 1, 1, 0, 0.0, _dt(tgt), _stream()),
                   "splitk_reduce dgrad")
    if pl.dgrad_folded:
        Ti, Hi, Wi = pl.dims[3:6]
        fold = L.c2m_reflect_border_add if two_target else L.c2m_reflect_fold
        _lib.check(fold(_p(tgt), _p(gx), N * Cin, Ti, Hi, Wi, pl.pad[0], pl.pad[1], pl.pad[2], _dt(tgt), _stream()),
                   "reflect fold")
    return gx


_DGRAD = {"wino3d": _dgrad_wino3d, "wino4": _dgrad_wino, "wino": _dgrad_wino, "wino4_ring": _dgrad_wino, "wino_ring": _dgrad_wino,
          "k333_nc8": _dgrad_nc8, "s2_nc8": _dgrad_nc8, "g8": _dgrad_igemm, "igemm_batched": _dgrad_igemm, "patch_nc8": _dgrad_igemm,
          "igemm": _dgrad_igemm}


def _conv_dgrad(pl, w, gy, frozen_w, out_dtype=torch.float32, keep=None):
    """Data gradient of the convolution described by plan `pl` (= the transposed convolution of gy with w): shared by
    _ConvFn.backward and conv_transpose2d.  gy contiguous [N, Cout, (To,) Ho, Wo]; returns [N, Cin, (Ti,) Hi, Wi] in
    `out_dtype` (the dtype of the forward input: bf16 on the bf16 data path, fp32 for fp32 inputs)."""
    if not pl.bf16:
        gy = _as(gy, torch.float32)
    gx = _DGRAD[pl.dgrad_route](pl, w, gy, frozen_w, out_dtype, keep)
    if pl.dM < pl.dims[1]:
        gx[:, pl.dM:].zero_()            # channels declared gradient-free by the caller (dgrad_rows); their planes were never written
    return gx if gx.dtype == out_dtype else gx.to(out_dtype)


def _fwd_timed(pl, run, x, w, y, what):
    _lib.check(_timed(pl.fwd_prof[0], pl.fwd_flops, run, pl.fwd_prof[1],
                      x.element_size() * x.numel() + 4 * w.numel() + y.element_size() * y.numel()), what)


def _fwd_wino(pl, x, w, b, y, act, slope, frozen_w, keep):
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    conv_wino = L.c2m_conv_wino
    if pl.fwd_route == "wino3d":      # virtual channels (kt, ci): [Cout][3*Cin][3][3]
        U = _packed(w, frozen_w, ("wino-fwd3d",), lambda: _wino_filter(
            w.permute(0, 2, 1, 3, 4).reshape(Cout, 3 * Cin, 3, 3).contiguous(), Cout, 3 * Cin, 0))
    elif pl.fwd_route == "wino4":     # F(4x4,3x3): its own roofline family (executed = algorithmic / 4)
        U, conv_wino = _packed(w, frozen_w, ("wino4-fwd",), lambda: _wino4_filter(w, Cout, Cin, 0)), L.c2m_conv_wino4
    else:
        U = _packed(w, frozen_w, ("wino-fwd",), lambda: _wino_filter(w, Cout, Cin, 0))
    _fwd_timed(pl, lambda: conv_wino(_p(U), _p(x), _p(y), None, _p(b), _gp(pl.wino_fwd_geom), act, slope, _stream()), x, w, y,
               "conv_wino fwd")


def _fwd_nc8(pl, x, w, b, y, act, slope, frozen_w, keep):
    """Routes k333_nc8 (3x3x3: (sample, frame) images, (time tap, channel) chunks) and s2_nc8 (4x4 stride 2: input parity planes)."""
    L = _lib.lib()
    N, Cin, Cout, Ti, Hi, Wi = pl.dims[0:6]
    if pl.fwd_route == "k333_nc8":
        A = _packed(w, frozen_w, ("fwd-bf16-k333",), lambda: _pack_bf16_k333(w, Cout, Cin))
        run = lambda: L.c2m_conv3d_nc8(_p(A), _p(_to_nc8(x, keep)), _p(y), _p(b), Cout, Cin, N, Ti, Hi, Wi, int(pl.reflect), 1, act, slope,
                                       _stream())
    else:
        A = _packed(w, frozen_w, ("fwd-bf16-s2",), lambda: _pack_bf16_patch(w, Cout, Cin, pl.K, 16, 2))
        run = lambda: L.c2m_conv_s2_nc8(_p(A), _p(_to_nc8(x, keep)), _p(y), _p(b), Cout, Cin, N, Hi, Wi, int(pl.reflect), 1, act, slope,
                                        _stream())
    _fwd_timed(pl, run, x, w, y, "conv_nc8 fwd")


def _fwd_igemm(pl, x, w, b, y, act, slope, frozen_w, keep):
    """Routes igemm, patch_nc8 (c2m_conv_patch_nc8 on channel-blocked input) and g8 (the NC8 gather form: channel-blocked input, bf16
    weights in (tap, chunk) order -- conv_gather_nc8_kernel), each with its split-K reduction."""
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    route = pl.fwd_route
    S = pl.g8_fwd_splits if route == "g8" else pl.fwd_splits
    dst = y if S == 1 else torch.empty(S * y.numel(), device=x.device, dtype=torch.float32)
    if route == "g8":
        A = _packed(w, frozen_w, ("fwd-bf16-g8",), lambda: _pack_bf16_gather(w, Cout, Cin, pl.dims[9:12], (1, 1, 1), pl.K, pl.K // Cin))

        def run():
            xn = _to_nc8(x)
            _set_io(pl.g8_fwd_geom, xn, BF16)
            return L.c2m_conv_igemm(_p(A), _p(xn), _p(dst), None, _p(b), _p(pl.g8_fwd_tab), _gp(pl.g8_fwd_geom), act, slope, _stream())
    else:
        if pl.bf16 and pl.fwd_geom[G.PATCH]:       # (the patch kernels of the bf16 path read their own weight image)
            A = _packed(w, frozen_w, ("fwd-bf16-patch",), lambda: _pack_bf16_patch(w, Cout, Cin, pl.K, 9))
        else:
            A = _packed(w, frozen_w, ("fwd", pl.ck), lambda: _pack_native(w, Cout, Cin, pl.ck, pl.dims[9:12], (1, 1, 1), pl.K, pl.K // Cin))
        _set_io(pl.fwd_geom, x, y.dtype)
        if route == "patch_nc8":
            run = lambda: _nc8_launch(L, A, x, dst, None, b, pl.fwd_geom, act, slope, keep)
        else:
            run = lambda: L.c2m_conv_igemm(_p(A), _p(x), _p(dst), None, _p(b), _p(pl.fwd_tab), _gp(pl.fwd_geom), act, slope, _stream())
    _fwd_timed(pl, run, x, w, y, "conv_igemm fwd (NC8 gather)" if route == "g8" else "conv_igemm fwd")
    if S > 1:
        _lib.check(L.c2m_splitk_reduce(_p(dst), _p(y), _p(b), y.numel(), S, int(pl.fwd_geom[G.OUT_SC]), Cout, act, slope, _dt(y),
                                       _stream()), "splitk_reduce")


_FWD = {"wino3d": _fwd_wino, "wino4": _fwd_wino, "wino": _fwd_wino, "k333_nc8": _fwd_nc8, "s2_nc8": _fwd_nc8,
        "g8": _fwd_igemm, "patch_nc8": _fwd_igemm, "igemm": _fwd_igemm}


def _wgrad_timed(pl, run, nbytes, what):
    _lib.check(_timed(pl.wgrad_prof[0], pl.fwd_flops, run, pl.wgrad_prof[1], nbytes), what)


def _wgrad_nc8(pl, x, w, gy, keep, x_keep):
    """Routes nc8 (3x3 stride 1), s2_nc8 (4x4 stride 2) and k333_nc8 (3x3x3, one launch per time tap): both operands in NC8 form -- X
    from the forward launch (x_keep = ctx.nc8_keep) or converted now, dY shared with the data gradient (keep)."""
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    gyn = _to_nc8(_as(gy, BF16), keep)
    xn = next(iter(x_keep.values()))[1] if x_keep else _to_nc8(_as(x, BF16))
    gw = torch.empty_like(w)
    gb = torch.empty(Cout, device=x.device, dtype=torch.float32)
    if pl.wgrad_route == "k333_nc8":
        Ti, Hi, Wi = pl.dims[3:6]
        slab = torch.empty(L.c2m_conv_wgrad_nc8_slab_floats(Cout, Cin, N * Ti, Hi, Wi, 0), device=x.device, dtype=torch.float32)
        what = "conv_wgrad3d_nc8"
        run = lambda: L.c2m_conv_wgrad3d_nc8(_p(gyn), _p(xn), _p(slab), _p(gw), _p(gb), Cout, Cin, N, Ti, Hi, Wi, int(pl.reflect), _stream())
    else:
        s2 = int(pl.wgrad_route == "s2_nc8")
        Ho, Wo = pl.dims[7:9]                  # the dY map
        slab = torch.empty(L.c2m_conv_wgrad_nc8_slab_floats(Cout, Cin, N, Ho, Wo, s2), device=x.device, dtype=torch.float32)
        what = "conv_wgrad_nc8"
        run = lambda: L.c2m_conv_wgrad_nc8(_p(gyn), _p(xn), _p(slab), _p(gw), _p(gb), Cout, Cin, N, Ho, Wo, int(pl.reflect), s2, _stream())
    _wgrad_timed(pl, run, 2 * (gyn.numel() + xn.numel()) + 4 * w.numel(), what)
    return gw, gb


def _wgrad_wino(pl, x, w, gy, keep, x_keep):
    """Routes wino and wino3d (the 2-D kernel over (sample, frame) images and virtual channels (time tap, channel))."""
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    Ti, Hi, Wi = pl.dims[3:6]
    S = pl.wino_wg_splits
    nbytes = 4 * (gy.numel() + x.numel() + w.numel())
    slab = torch.empty((S + 1) * 16 * Cout * pl.dims[9] * Cin, device=x.device, dtype=torch.float32)
    dbslab = torch.empty(S * Cout, device=x.device, dtype=torch.float32)
    gb = torch.empty(Cout, device=x.device, dtype=torch.float32)
    if pl.wgrad_route == "wino3d":
        gw3 = torch.empty(Cout, 3, Cin, 3, 3, device=x.device, dtype=torch.float32)      # (time tap, channel) order
        _wgrad_timed(pl, lambda: L.c2m_conv_wino_wgrad3d(_p(gy), _p(x), _p(slab), _p(dbslab), _p(gw3), _p(gb), Cout, Cin, N, Ti, Hi, Wi,
                                                         int(pl.reflect), _stream()), nbytes, "conv_wino_wgrad3d")
        return gw3.permute(0, 2, 1, 3, 4).contiguous(), gb
    gw = torch.empty_like(w)
    _wgrad_timed(pl, lambda: L.c2m_conv_wino_wgrad(_p(gy), _p(x), _p(slab), _p(dbslab), _p(gw), _p(gb), Cout, Cin, N, Hi, Wi,
                                                   int(pl.reflect), _stream()), nbytes, "conv_wino_wgrad")
    return gw, gb


def _wgrad_igemm(pl, x, w, gy, keep, x_keep):
    L = _lib.lib()
    N, Cin, Cout = pl.dims[0:3]
    slab = torch.empty(pl.wg_splits * Cout * pl.J, device=x.device, dtype=torch.float32)
    gw = torch.empty_like(w)
    gb = torch.empty(Cout, device=x.device, dtype=torch.float32)
    # bf16 data path: the MFMA kernel gathers bf16 dY and X; the <= 4-output-channel heads run on the fp32 vector-ALU
    # kernels (c2m_conv_wgrad's own rule: M <= 4 and >= 16384 pixels)
    wdt = BF16 if (pl.bf16 and not (Cout <= 4 and int(pl.wg_geom[G.NPIX]) >= 16384)) else torch.float32
    xg, gyw = _as(x, wdt), _as(gy, wdt)
    pl.wg_geom[G.X_BYTES], pl.wg_geom[G.DY_BYTES] = xg.numel() * xg.element_size(), gyw.numel() * gyw.element_size()
    pl.wg_geom[G.X_TYPE] = _dt(xg)
    _wgrad_timed(pl, lambda: L.c2m_conv_wgrad(_p(gyw), _p(xg), _p(slab), _p(gw), _p(gb), _p(pl.wg_tab), _gp(pl.wg_geom), _stream()),
                 xg.element_size() * (gyw.numel() + xg.numel()) + 4 * w.numel(), "conv_wgrad")
    return gw, gb


_WGRAD = {"k333_nc8": _wgrad_nc8, "nc8": _wgrad_nc8, "s2_nc8": _wgrad_nc8, "wino3d": _wgrad_wino, "wino": _wgrad_wino,
          "igemm": _wgrad_igemm}


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, reflect, act, dgrad_rows=None, slope=LRELU_SLOPE):
        _dev(x, w, b)
        ctx.slope = slope = float(slope)
        # the caller's weight and bias objects, for backward's deferral checks (weak: the node keeps no parameter alive)
        ctx.wb_refs = (weakref.ref(w), weakref.ref(b) if b is not None else None)
        x, w = _f(x), _f(w)
        pl = _plan(x, w, stride, pad, reflect, dgrad_rows)
        if b is not None and b.numel() != pl.dims[2]:
            raise RuntimeError(f"convolution: bias of {b.numel()} elements for {pl.dims[2]} output channels")
        ctx.frozen_w = not ctx.needs_input_grad[1]
        ctx.x_dtype = x.dtype
        ctx.nc8_keep = {} if (pl.keep_x_nc8 and ctx.needs_input_grad[1]) else None      # X in NC8 form, for the weight gradient
        x = _as(x, pl.fwd_xdt)             # (the fp32 kernels are fp32 in, fp32 out; bf16 path: an fp32 input is cast once)
        y = torch.empty(pl.out_shape, device=x.device, dtype=pl.fwd_ydt)
        _FWD[pl.fwd_route](pl, x, w, b, y, ACT[act], slope, ctx.frozen_w, ctx.nc8_keep)
        ctx.pl, ctx.act, ctx.has_bias = pl, act, b is not None
        ctx.save_for_backward(x, w, y if ACT[act] else None)
        # an output whose gradient this layer's backward will read through NC8 kernels only (no fused activation: act_bwd reads the
        # incoming gradient in NCHW): a norm op told that it is the output's ONLY consumer (`private_input=True`) then hands its dx back
        # in NC8 form alone
        if pl.bf16 and not ACT[act] and y.dtype == BF16 and _bwd_reads_only_nc8(
                pl, ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])):
            y._c2m_bwd_nc8 = True
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        pl, L = ctx.pl, _lib.lib()
        gy = _f(gy)
        if _NC8_LOG is not None:
            _NC8_LOG_TAG[0] = " (own act_bwd)" if ACT[ctx.act] else " (incoming gradient)"
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        if ACT[ctx.act]:
            gy = _as(gy, y.dtype)
            if y.dtype == BF16 and _bwd_reads_only_nc8(pl, ctx.needs_input_grad[0], need_w):
                # the masked gradient in NC8 form only: its readers below are all NC8 kernels (no NCHW write, no layout pass)
                Nn, Cc = y.shape[0], y.shape[1]
                gn = torch.empty((Nn, _cdiv(Cc, 8)) + tuple(y.shape[2:]) + (8,), device=y.device, dtype=BF16)
                _lib.check(L.c2m_grad_to_nc8(0, _p(y), None, _p(gy), None, _p(gn), Nn, Cc, y.numel() // (Nn * Cc), 0, ACT[ctx.act],
                                             ctx.slope, _stream()), "grad_to_nc8 (act_bwd)")
                gy = _virtual_grad(y, gn)
            else:
                g = torch.empty_like(gy)
                _lib.check(L.c2m_act_bwd(_p(y), _p(gy), _p(g), gy.numel(), ACT[ctx.act], ctx.slope, _dt(y), _stream()), "act_bwd")
                gy = g
        N, Cin, Cout = pl.dims[0:3]
        gx = gw = gb = None
        # The weight gradient and the data gradient of a layer are independent: with both wanted, the weight gradient (and its
        # split reductions) is issued on a side stream and joined at the end of this node, so the two launches share the chip
        # -- the tail of one (e.g. 1440 workgroups on 512 slots) is filled by the other and the ~10 us reductions disappear
        # behind MFMA kernels.  Fork / join are events, so a HIP-graph capture records the same parallel branches.
        # (inside a capture for both precisions: fp32 configs[1] as a replay 66.6 -> 66.1 ms on one box, `bench.py --graph`)
        side_on = _WGRAD_SIDE == "1" or (_WGRAD_SIDE == "auto" and torch.cuda.is_current_stream_capturing())
        # (not from the auxiliary stream of the object branch: its one small convolution gains nothing, and a side stream that two
        # captured streams fork into and join from takes capture_end down on ROCm 7.2 -- tools/aux_capture_probe.py)
        side = _side_stream(x.device) if (side_on and need_w and ctx.needs_input_grad[0] and not _on_aux_stream(x.device)) else None
        # NC8 form of dY: one layout pass shared by the data gradient and the weight gradient of this node (made on the main
        # stream BEFORE a fork, so the side stream's launch is ordered behind it)
        keep = {} if pl.keep_dy_nc8 else None
        if need_w and pl.wgrad_route in _NC8_WGRADS:
            gy = _as(gy, BF16)
            _to_nc8(gy, keep)
        # (not while capturing a HIP graph: the graph executor runs the long side branch worse than the per-node fork + join below --
        # replays of configs[3] / configs[2]: 42.7 / 63.9 ms deferred, 42.4 / 63.5 per node, 43.8 / 66.4 deferred without the object
        # branch -- and a capture would have to hold every dY until its end)
        if need_w and _defer["on"] and not torch.cuda.is_current_stream_capturing():
            # `with ops.deferred_wgrads(params=...):` around backward (TrainStep): the weight / bias gradient of LISTED leaf
            # parameters that have no gradient yet goes to the side stream and is NOT joined here -- nothing reads it before the
            # optimizer (AccumulateGrad adopts the tensor, no kernel) -- so its split reductions and its tail run under the
            # data-gradient chain of the layers below.  The context's exit joins.  The gradients stay unjoined only when nothing on
            # this stream can touch them before that (_may_defer, asked for the weight AND the bias): a parameter that already has a
            # gradient (a second backward: AccumulateGrad sums with a kernel on this stream), that is not a leaf, that got a
            # gradient earlier in this backward (a weight applied twice -- the sparse-feature encoder with use_fw_of --, a bias
            # shared by two convolutions: the engine sums the two on this stream) or that carries a hook joins first and takes the
            # ordinary path.  A parameter that ALSO feeds a non-convolution op of the graph cannot be seen from here: that is
            # what the caller's list vouches for, and an unlisted parameter is never deferred.
            w0, b0 = (r() if r is not None else None for r in ctx.wb_refs)
            defer_ok = (not ctx.needs_input_grad[1] or _may_defer(w0)) and \
                (not (ctx.has_bias and ctx.needs_input_grad[2]) or _may_defer(b0))
            for p in (w0, b0):
                if p is not None:
                    _defer["seen"].add(id(p))
            if defer_ok and ConvProfiler.active is None and not _on_aux_stream(x.device):
                main = torch.cuda.current_stream(x.device)
                dside = _side_stream(x.device)
                dside.wait_stream(main)
                _record_stream_all(dside, x, gy, keep, ctx.nc8_keep)    # freed by autograd right after this node; still being read
                with torch.cuda.stream(dside):
                    gw, gb = _ConvFn._wgrad(ctx, pl, x, w, gy, keep)
                for p, t in ((w0, gw), (b0, gb)):
                    if t is not None:
                        t.record_stream(main)
                        _defer["grads"][t.data_ptr()] = dside
                        if p is not None:
                            _defer["by_p"][id(p)] = t.data_ptr()
                _defer["devs"].add(x.device.index)
                # dY may be shared with the identity path of a residual block (AddBackward hands ONE tensor to both branches): the
                # engine sums the other branch's gradient into it IN PLACE once nobody else holds it -- while the side stream still
                # reads it (found by test_branch_streams_do_not_change_a_step: conv2 of the residual blocks).  A second owner makes
                # that sum out of place; the reference is dropped when the side stream has passed this launch.
                ev = torch.cuda.Event()
                ev.record(dside)
                hold = _defer["hold"]
                hold.append((ev, gy))
                while hold and hold[0][0].query():
                    hold.popleft()
                if ctx.needs_input_grad[0]:
                    gx = _conv_dgrad(pl, w, gy, ctx.frozen_w, ctx.x_dtype, keep)
                return gx, gw, gb, None, None, None, None, None, None
            if x.device.index in _defer["devs"]:
                torch.cuda.current_stream(x.device).wait_stream(_side_stream(x.device))
                for p in (w0, b0):                      # a first gradient is summed with this one on THIS stream:
                    ptr = _defer["by_p"].pop(id(p), None) if p is not None else None
                    if ptr is not None:
                        _defer["grads"].pop(ptr, None)  # no longer "being produced on the side stream"
        if side is not None:
            main = torch.cuda.current_stream(x.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                gw, gb = _ConvFn._wgrad(ctx, pl, x, w, gy, keep)
            gx = _conv_dgrad(pl, w, gy, ctx.frozen_w, ctx.x_dtype, keep)
            main.wait_stream(side)
            for t in (gw, gb):
                if t is not None:
                    t.record_stream(main)       # allocated in the side stream's pool, consumed (and freed) on the main stream
            return gx, gw, gb, None, None, None, None, None, None
        if ctx.needs_input_grad[0]:
            gx = _conv_dgrad(pl, w, gy, ctx.frozen_w, ctx.x_dtype, keep)
        if need_w:
            gw, gb = _ConvFn._wgrad(ctx, pl, x, w, gy, keep)
        return gx, gw, gb, None, None, None, None, None, None

    @staticmethod
    def _wgrad(ctx, pl, x, w, gy, keep=None):
        if not (ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])):
            return None, None
        if not pl.bf16:
            gy = _as(gy, torch.float32)
        gw, gb = _WGRAD[pl.wgrad_route](pl, x, w, gy, keep, ctx.nc8_keep)
        return gw, (gb if ctx.has_bias else None)


def conv(x, w, b=None, stride=1, padding=0, padding_mode="zeros", act=None, dgrad_channels=None, slope=LRELU_SLOPE):
    """conv2d (4-D x) / conv3d (5-D x) with zero or reflect padding folded into the gather; bias + activation fused.
    dgrad_channels: the caller guarantees that only x[:, :dgrad_channels] needs a gradient (x is a concatenation whose tail
    carries no grad); the data gradient of the tail is returned as zeros instead of being computed."""
    nd = x.dim() - 2
    stride3, pad3 = _triple(stride, nd), _pad3(padding, nd)
    reflect = padding_mode == "reflect" and any(pad3)
    if padding_mode not in ("zeros", "reflect"):
        raise NotImplementedError(f"padding_mode {padding_mode}")
    # The kernels address each tensor with 32-bit byte offsets (< 2 GiB).  Larger activations (40 folded frames x 128
    # channels at 256x512 = 2.7 GB) are run as batch chunks: images are independent in the forward pass and the data
    # gradient, and autograd sums the chunks' weight gradients.
    n = x.shape[0]
    k = _chunks_for_2gib(x.shape, w.shape, stride3, pad3)
    if k > 1:
        size = _cdiv(n, k)
        return torch.cat([_ConvFn.apply(xc, w, b, stride3, pad3, reflect, act, dgrad_channels, slope) for xc in x.split(size)], 0)
    return _ConvFn.apply(x, w, b, stride3, pad3, reflect, act, dgrad_channels, slope)


class _ConvReluTapFn(torch.autograd.Function):
    """y = relu(conv3x3(x; frozen w, b)) together with the L1 tap mean|y - t| it feeds (a perceptual-loss tap of the frozen
    VGG-19, losses.py:60-65): backward folds the L1 gradient, its sum with the next conv's data gradient and the ReLU mask
    into ONE element-wise pass (c2m_relu_tap_bwd) in front of the data gradient -- autograd ran three (9 tensor passes instead
    of 4 over the largest tensors of the step).  Same fp32 arithmetic, so values and gradients are bit-identical to
    conv(act='relu') + l1_mean."""

    @staticmethod
    def forward(ctx, x, w, b, t, pad3):
        y = _ConvFn.apply(x, w, b, (1, 1, 1), pad3, False, "relu", None, LRELU_SLOPE)       # (grad mode is off in here)
        t = _as(t, y.dtype)
        l = _L1MeanFn.apply(y, t, None)
        ctx.pl = _plan(_f(x), _f(w), (1, 1, 1), pad3, False, None)
        ctx.x_dtype = x.dtype
        ctx.save_for_backward(w, y, t)
        ctx.set_materialize_grads(False)
        return y, l

    @staticmethod
    def backward(ctx, gy, gl):
        if gy is None and gl is None:
            return None, None, None, None, None
        w, y, t = ctx.saved_tensors
        if gl is None:
            gl = torch.zeros((), device=y.device, dtype=torch.float32)
        gl = _f(gl.reshape(1).float())
        gy = None if gy is None else _as(gy, y.dtype)
        if y.dtype == BF16 and _bwd_reads_only_nc8(ctx.pl, True, False):
            Nn, Cc = y.shape[0], y.shape[1]
            gn = torch.empty((Nn, _cdiv(Cc, 8)) + tuple(y.shape[2:]) + (8,), device=y.device, dtype=BF16)
            _lib.check(_lib.lib().c2m_grad_to_nc8(1, _p(y), _p(t), _p(gy), _p(gl), _p(gn), Nn, Cc, y.numel() // (Nn * Cc), y.numel(),
                                                  0, 0.0, _stream()), "grad_to_nc8 (relu_tap_bwd)")
            return _conv_dgrad(ctx.pl, w, _virtual_grad(y, gn), True, ctx.x_dtype), None, None, None, None
        g = torch.empty_like(y)
        _lib.check(_lib.lib().c2m_relu_tap_bwd(_p(y), _p(t), _p(gy), _p(gl), _p(g), y.numel(), _dt(y), _stream()), "relu_tap_bwd")
        if _NC8_LOG is not None:
            _NC8_LOG_TAG[0] = " (relu_tap_bwd)"
        return _conv_dgrad(ctx.pl, w, g, True, ctx.x_dtype), None, None, None, None


def conv_relu_tap(x, w, b, target, padding=1):
    """(y, mean|y - target|) for y = relu(conv(x, w, b)) with a FROZEN w / b (the VGG-19 of the perceptual loss) and a target
    without gradient: conv(act='relu') + l1_mean with a fused backward (see _ConvReluTapFn).  Falls back to the two ops where
    the fused form does not apply (weights that need gradients, batches that run as 2 GiB chunks)."""
    nd = x.dim() - 2
    pad3 = _pad3(padding, nd)
    if w.requires_grad or (b is not None and b.requires_grad) or target.requires_grad or not x.requires_grad or \
            not torch.is_grad_enabled() or _chunks_for_2gib(x.shape, w.shape, (1, 1, 1), pad3) > 1:
        y = conv(x, w, b, stride=1, padding=padding, padding_mode="zeros", act="relu")
        return y, l1_mean(y, target)
    return _ConvReluTapFn.apply(x, w, b, target, pad3)


class _ConvReluPoolFn(torch.autograd.Function):
    """maxpool2x2(relu(conv3x3(x; frozen w, b))) as one node (layers/vgg.py: the conv -> ReLU -> MaxPool2d runs of the frozen
    VGG-19 whose ReLU output nobody else reads): the pool backward applies the ReLU mask on the value it already holds
    (c2m_maxpool2x2_relu_bwd), so the activation-backward pass over the full-resolution tensor disappears.  Same arithmetic ->
    bit-identical to conv(act='relu') + maxpool2x2."""

    @staticmethod
    def forward(ctx, x, w, b, pad3):
        y = _ConvFn.apply(x, w, b, (1, 1, 1), pad3, False, "relu", None, LRELU_SLOPE)
        p = _MaxPool2Fn.apply(y)
        ctx.pl = _plan(_f(x), _f(w), (1, 1, 1), pad3, False, None)
        ctx.x_dtype = x.dtype
        ctx.save_for_backward(w, y)
        return p

    @staticmethod
    def backward(ctx, gp):
        w, y = ctx.saved_tensors
        N, C, H, W = y.shape
        g = torch.empty_like(y)
        _lib.check(_lib.lib().c2m_maxpool2x2_relu_bwd(_p(y), _p(_as(gp, y.dtype)), _p(g), N * C, H, W, _dt(y), _stream()),
                   "maxpool_relu_bwd")
        return _conv_dgrad(ctx.pl, w, g, True, ctx.x_dtype), None, None, None


def conv_relu_pool(x, w, b, padding=1):
    """maxpool2x2(relu(conv(x, w, b))) for a FROZEN w / b, with the ReLU backward folded into the pool backward; the unfused
    ops where that does not apply (trainable weights, no gradient wanted, 2 GiB batch chunks, odd extents)."""
    nd = x.dim() - 2
    pad3 = _pad3(padding, nd)
    if nd != 2 or w.requires_grad or (b is not None and b.requires_grad) or not x.requires_grad or not torch.is_grad_enabled() or \
            _chunks_for_2gib(x.shape, w.shape, (1, 1, 1), pad3) > 1:
        return maxpool2x2(conv(x, w, b, stride=1, padding=padding, padding_mode="zeros", act="relu"))
    return _ConvReluPoolFn.apply(x, w, b, pad3)


def conv_transpose2d(x, w, b=None, stride=2, padding=1, act=None, slope=LRELU_SLOPE):
    """nn.ConvTranspose2d(x; w [Cin, Cout, kh, kw], stride, padding) (+ bias, activation) for frozen, no-grad use (FlowNet2's
    `deconv` / `upsampled_flow` layers, flownet2/networks/submodules.py:75-80): a transposed convolution IS the data gradient
    of the convolution with the same weight tensor, so it runs on the stride-parity-class data-gradient kernels (no
    zero-stuffed MACs).  Output size (H - 1) * stride - 2 * padding + k."""
    _dev(x, w, b)
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)):
        raise RuntimeError("conv_transpose2d is forward-only (frozen flow network under no_grad)")
    x, w = _f(x), _f(w)
    N, Ci, H, W = x.shape
    Co, kh, kw = w.shape[1], w.shape[2], w.shape[3]
    s3, p3 = _triple(stride, 2), _pad3(padding, 2)
    Ho, Wo = (H - 1) * s3[1] - 2 * p3[1] + kh, (W - 1) * s3[2] - 2 * p3[2] + kw
    # the forward convolution whose data gradient this is: input [N, Co, Ho, Wo] (x of the plan), weight [Ci, Co, kh, kw]
    pl = _plan_for((N, Co, Ho, Wo), tuple(w.shape), s3, p3, False, x.device)
    if pl.out_shape != (N, Ci, H, W):
        raise ValueError(f"conv_transpose2d: inconsistent geometry {tuple(x.shape)} vs {pl.out_shape}")
    with torch.no_grad():
        y = _conv_dgrad(pl, w, x, True, x.dtype)
        if b is not None or ACT[act]:
            y = _as(y, torch.float32)
            _lib.check(_lib.lib().c2m_bias_act(_p(y), _p(b), N, Co, Ho * Wo, ACT[act], float(slope), _stream()), "bias_act")
    return y


_MAX_TENSOR_BYTES = int(0.9 * 2 ** 31)      # 10 % margin: the Winograd data gradient rounds its padded domain up to whole tiles


def _chunks_for_2gib(xs, ws, stride, pad):
    """Number of batch chunks that keeps the input (incl. its padded data-gradient domain) and the output of one
    launch under 2 GiB; 1 for everything the bench configurations use at 128x256."""
    n, cin, cout = xs[0], xs[1], ws[0]
    sp_in = [d for d in xs[2:]]
    k3 = list(ws[2:])
    nd = len(sp_in)
    padded, out = 1, 1
    for d in range(nd):
        padded *= sp_in[d] + 2 * pad[3 - nd + d]
        out *= max((sp_in[d] + 2 * pad[3 - nd + d] - k3[d]) // stride[3 - nd + d] + 1, 1)
    per_image = 4 * max(cin * padded, cout * out)
    if n * per_image < _MAX_TENSOR_BYTES:
        return 1
    fit = (_MAX_TENSOR_BYTES - 1) // per_image
    if fit < 1:
        raise ValueError("tensor too large: one image exceeds the 32-bit byte offsets of the gather (< 2 GiB)")
    return _cdiv(n, fit)


# =============================================================================================== norm + act
class _NormActFn(torch.autograd.Function):
    """y = act(norm(x) * scale + shift); mode 0 instance / 1 batch statistics; gb = SPADE [N,2C,...] map or None."""

    @staticmethod
    def forward(ctx, x, gamma, beta, gb, running_mean, running_var, mode, act, eps, momentum, feeds=None, private_input=False, rep=1):
        _dev(x, gamma, beta, gb)
        rep = int(rep)
        if rep < 1 or (rep != 1 and mode != 1):
            raise ValueError(f"norm: replication count {rep} (batch statistics only, >= 1)")
        x = _f(x)
        ctx.gb_dtype = gb.dtype if gb is not None else None
        gb = _as(gb, x.dtype)                   # the SPADE map shares the activation type (bf16 on the bf16 data path)
        dt = _dt(x)
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        # the kernels index these by channel: sizes checked here (torch's norm layers raise on the same mistakes)
        for name, t, want in (("gamma", gamma, C), ("beta", beta, C), ("running_mean", running_mean, C), ("running_var", running_var, C),
                              ("SPADE map", gb, 2 * x.numel())):
            if t is not None and t.numel() != want:
                raise RuntimeError(f"norm: {name} has {t.numel()} elements, expected {want} for an input of shape {tuple(x.shape)}")
        L = _lib.lib()
        nstat = N * C if mode == 0 else C
        mean = torch.empty(nstat, device=x.device, dtype=torch.float32)
        invstd = torch.empty_like(mean)
        ws = torch.empty(L.c2m_norm_workspace_floats(N, C, S), device=x.device, dtype=torch.float32)
        y = torch.empty_like(x)
        # `feeds`: the result's only consumer is one convolution whose forward and weight gradient read NC8 -> NC8 is the ONLY output
        # (writing both layouts measured slower than the layout passes it saved: 47.7 vs 47.05 ms, 71.5 vs 70.7 ms per bf16 step)
        only = False
        if feeds is not None and dt == 1 and S % 8 == 0:
            only = _consumer_reads_only_nc8(x, feeds)
        yn = torch.empty((N, _cdiv(C, 8)) + tuple(x.shape[2:]) + (8,), device=x.device, dtype=BF16) if only else None
        if yn is None:
            # statistics + apply in one call: instance-norm planes of <= 32768 elements run as ONE launch (norm_inst_fused_kernel)
            _lib.check(L.c2m_norm_fwd_rep(_p(x), _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(ws), _p(gamma), _p(beta), _p(gb),
                                          _p(y), N, C, S, mode, eps, momentum, rep, ACT[act], LRELU_SLOPE, dt, _stream()), "norm_fwd")
        else:
            _lib.check(L.c2m_norm_stats_rep(_p(x), _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(ws), N, C, S, mode,
                                            eps, momentum, rep, dt, _stream()), "norm_stats")
            _lib.check(L.c2m_norm_apply(_p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(gb), None, _p(yn), N, C, S,
                                        mode, ACT[act], LRELU_SLOPE, dt, _stream()), "norm_apply")
        if only and _NC8_POISON:
            y.fill_(float("nan"))
        ctx.cfg = (N, C, S, mode, act)
        # x is the output of a convolution whose backward reads its gradient in NC8 only, and this op is x's only consumer (the
        # caller's promise): dx is produced in NC8 form alone
        ctx.dx_nc8_only = bool(private_input and _NC8_GRAD and dt == 1 and S % 8 == 0 and getattr(x, "_c2m_bwd_nc8", False))
        ctx.save_for_backward(x, gamma, beta, gb, mean, invstd)
        if yn is None:
            return y, None
        ctx.mark_non_differentiable(yn)
        return y, yn

    @staticmethod
    def backward(ctx, gy, _gyn=None):
        x, gamma, beta, gb, mean, invstd = ctx.saved_tensors
        N, C, S, mode, act = ctx.cfg
        L = _lib.lib()
        gy = _as(gy, x.dtype)
        only = ctx.dx_nc8_only
        dx = torch.empty_like(x)
        dxn = torch.empty((N, _cdiv(C, 8)) + tuple(x.shape[2:]) + (8,), device=x.device, dtype=BF16) if only else None
        ggb = torch.empty_like(gb) if gb is not None else None
        dgamma = torch.empty_like(gamma) if gamma is not None else None
        dbeta = torch.empty_like(beta) if gamma is not None else None
        ws = torch.empty(L.c2m_norm_workspace_floats(N, C, S), device=x.device, dtype=torch.float32)
        _lib.check(L.c2m_norm_bwd(_p(x), _p(gy), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(gb), _p(ggb), _p(dgamma),
                                  _p(dbeta), None if only else _p(dx), _p(dxn), _p(ws), N, C, S, mode, ACT[act], LRELU_SLOPE, _dt(x),
                                  _stream()),
                   "norm_bwd")
        if only and _NC8_POISON:
            dx.fill_(float("nan"))
        if only:
            _mark_nc8_only(dx, dxn)               # autograd hands this very tensor object to the convolution's backward (see _to_nc8)
        if ggb is not None and ggb.dtype != ctx.gb_dtype:
            ggb = ggb.to(ctx.gb_dtype)
        return dx, dgamma, dbeta, ggb, None, None, None, None, None, None, None, None, None


def _norm_act(*args, rep=1):
    y, yn = _NormActFn.apply(*args, rep)
    if yn is not None:                            # NC8 is the only output (`only` in _NormActFn.forward)
        _mark_nc8_only(y, yn)                     # y's NCHW storage was never written
    return y


def batch_norm_act(x, gamma, beta, running_mean, running_var, act=None, eps=1e-5, momentum=0.1, feeds=None, private_input=False, rep=1):
    """private_input: x is a convolution's output that NOTHING else reads (`y = conv(..); y = norm(y)` inside a block) -- where that
    convolution's backward runs on NC8 kernels, dx is handed back in NC8 form only (no NCHW write, no layout pass).
    rep: x stands for `rep` identical copies of itself (the generator encodes a source frame once for its T predicted frames); the
    running variance is updated as the copied batch would have updated it, everything else is the batch's own."""
    return _norm_act(x, gamma, beta, None, running_mean, running_var, 1, act, eps, momentum, feeds, private_input, rep=rep)


def instance_norm_act(x, gamma=None, beta=None, act=None, eps=1e-5, feeds=None, private_input=False):
    return _norm_act(x, gamma, beta, None, None, None, 0, act, eps, 0.1, feeds, private_input)


def spade_norm_act(x, gamma_beta, act=None, eps=1e-5, feeds=None, private_input=False):
    """InstanceNorm(affine=False)(x) * (1 + gamma) + beta with [gamma, beta] = gamma_beta.chunk(2, 1), then act.
    feeds (all three ops): `conv_consumer(...)` of the one convolution that reads the result, see there."""
    return _norm_act(x, None, None, gamma_beta, None, None, 0, act, eps, 0.1, feeds, private_input)


# =============================================================================================== warping / resampling
class _FlowWarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, flow, occ):
        _dev(img, flow, occ)
        ctx.flow_dtype = flow.dtype
        img, flow = _f(img), _as(flow, torch.float32)        # coordinates are never rounded to bf16
        occ = _as(occ, torch.float32)
        N, C, H, W = img.shape
        assert flow.shape == (N, 2, H, W), f"flow {tuple(flow.shape)} vs image {tuple(img.shape)}"
        assert occ is None or occ.shape == (N, 1, H, W)
        out = torch.empty_like(img)
        _lib.check(_lib.lib().c2m_flow_warp_fwd(_p(img), _p(flow), _p(occ), _p(out), N, C, H, W, _dt(img), _stream()),
                   "flow_warp")
        ctx.save_for_backward(img, flow, occ)
        return out

    @staticmethod
    def backward(ctx, gout):
        img, flow, occ = ctx.saved_tensors
        N, C, H, W = img.shape
        L = _lib.lib()
        gimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        gflow = torch.empty_like(flow) if ctx.needs_input_grad[1] else None
        if gimg is not None or gflow is not None:
            ws = torch.empty(L.c2m_flow_warp_bwd_workspace_bytes(N, C, H, W, int(gimg is not None), int(gflow is not None)),
                             device=img.device, dtype=torch.uint8)
            _lib.check(L.c2m_flow_warp_bwd(_p(img), _p(flow), _p(occ), _p(_as(gout, img.dtype)), _p(gimg), _p(gflow), N, C, H,
                                           W, _p(ws), _dt(img), _stream()), "flow_warp_bwd")
        if gflow is not None and gflow.dtype != ctx.flow_dtype:
            gflow = gflow.to(ctx.flow_dtype)
        return gimg, gflow, None


def flow_warp(img, flow, occ=None):
    """utils.resample(img, flow) [* occ]: backward warp with pixel-unit flow (reference coordinate quirk included)."""
    return _FlowWarpFn.apply(img, flow, occ)


def resample2d(img, flow):
    """FlowNet2 Resample2d (kernel_size 1, bilinear): img [N,C,H,W] sampled at (x + flow[:,0], y + flow[:,1]), taps clamped to
    the border (third_party/resample2d/src/resample2d_kernel.cu:16-75).  Forward only."""
    _dev(img, flow)
    img, flow = _as(img.detach(), torch.float32), _as(flow.detach(), torch.float32)     # fp32-only kernel (bf16 conv outputs are cast)
    N, C, H, W = img.shape
    assert flow.shape == (N, 2, H, W)
    out = torch.empty_like(img)
    _lib.check(_lib.lib().c2m_resample2d_fwd(_p(img), _p(flow), _p(out), N, C, H, W, _stream()), "resample2d")
    return out


def channelnorm(x):
    """FlowNet2 ChannelNorm: sqrt(sum_c x^2) -> [N,1,H,W] (third_party/channelnorm/src/channelnorm_kernel.cu:19-62)."""
    _dev(x)
    x = _as(x.detach(), torch.float32)                   # fp32-only kernel
    N, C, H, W = x.shape
    out = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().c2m_channelnorm_fwd(_p(x), _p(out), N, C, H, W, _stream()), "channelnorm")
    return out


def correlation(a, b, pad_size=20, kernel_size=1, max_displacement=20, stride1=1, stride2=2):
    """FlowNetC cost volume (third_party/correlation/src/correlation_cuda_kernel.cu:47-147; defaults = flownet_c.py:44-46):
    [N,C,H,W] x [N,C,H,W] -> [N, (2*(max_displacement//stride2)+1)^2, oH, oW]."""
    _dev(a, b)
    a, b = _as(a.detach(), torch.float32), _as(b.detach(), torch.float32)      # fp32-only kernel: a bf16 pointer would be read as floats
    assert a.shape == b.shape
    N, C, H, W = a.shape
    L = _lib.lib()
    D = 2 * (max_displacement // stride2) + 1
    oH = L.c2m_correlation_out_size(H, pad_size, kernel_size, max_displacement, stride1)
    oW = L.c2m_correlation_out_size(W, pad_size, kernel_size, max_displacement, stride1)
    out = torch.empty(N, D * D, oH, oW, device=a.device, dtype=torch.float32)
    _lib.check(L.c2m_correlation_fwd(_p(a), _p(b), _p(out), N, C, H, W, pad_size, kernel_size, max_displacement, stride1,
                                     stride2, _stream()), "correlation")
    return out


class _Upsample2xFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, feeds=None):
        _dev(x)
        x = _f(x)
        N, C, H, W = x.shape
        y = torch.empty(N, C, 2 * H, 2 * W, device=x.device, dtype=x.dtype)
        ctx.shape = (N, C, H, W)
        if feeds is not None and x.dtype == BF16 and (H * W) % 8 == 0:
            # the result's only reader is one convolution whose forward and weight gradient read NC8: NC8 -> NC8, no NCHW result
            if _consumer_reads_only_nc8(y, feeds):
                xn = _to_nc8(x)
                yn = torch.empty((N, _cdiv(C, 8), 2 * H, 2 * W, 8), device=x.device, dtype=BF16)
                _lib.check(_lib.lib().c2m_upsample2x_nc8(_p(xn), _p(yn), N * _cdiv(C, 8), H, W, _stream()), "upsample2x_nc8")
                if _NC8_POISON:
                    y.fill_(float("nan"))
                _Upsample2xFn.last_form = yn      # read by upsample2x() right behind apply(): tags y as NC8-only
                return y
        _Upsample2xFn.last_form = None
        _lib.check(_lib.lib().c2m_upsample2x_fwd(_p(x), _p(y), N * C, H, W, _dt(x), _stream()), "upsample2x")
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W = ctx.shape
        gy = _f(gy)
        gx = torch.empty(N, C, H, W, device=gy.device, dtype=gy.dtype)
        _lib.check(_lib.lib().c2m_upsample2x_bwd(_p(gy), _p(gx), N * C, H, W, _dt(gy), _stream()), "upsample2x_bwd")
        return gx, None


def upsample2x(x, feeds=None):
    """nn.Upsample(scale_factor=2, mode='bilinear').  feeds: `conv_consumer(...)` of the ONE convolution that reads the result (the up
    block): where that layer reads NC8 only, the up-sampled map -- the largest tensors of the decoder -- is produced in NC8 alone."""
    y = _Upsample2xFn.apply(x, feeds)
    if _Upsample2xFn.last_form is not None:
        _mark_nc8_only(y, _Upsample2xFn.last_form)
        _Upsample2xFn.last_form = None
    return y


def resize_bilinear(x, size, align_corners=False):
    """F.interpolate(x, size, mode='bilinear') for no-grad tensors (sparse flow / occlusion pyramids)."""
    _dev(x)
    if x.requires_grad:
        raise RuntimeError("resize_bilinear has no backward; use upsample2x for the differentiable x2 case")
    x = _f(x)
    N, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=x.dtype)
    _lib.check(_lib.lib().c2m_resize_bilinear(_p(x), _p(y), N * C, H, W, Ho, Wo, 1 if align_corners else 0, 0.0,
                                              _dt(x), _stream()), "resize_bilinear")
    return y


class _ResizeBilinearFn(torch.autograd.Function):
    """Every leading dimension is a plane: a contiguous [B,C,T,H,W] is B*C*T planes, so the reference's fold -> interpolate
    -> unfold (utils.resize_video) is this one launch with no permute copies."""

    @staticmethod
    def forward(ctx, x, Ho, Wo, align):
        x = _f(x)
        H, W = x.shape[-2:]
        planes = x.numel() // max(H * W, 1)
        y = torch.empty(x.shape[:-2] + (Ho, Wo), device=x.device, dtype=x.dtype)
        ctx.meta = (x.shape, planes, H, W, Ho, Wo, align)
        _lib.check(_lib.lib().c2m_resize_bilinear(_p(x), _p(y), planes, H, W, Ho, Wo, align, 0.0, _dt(x), _stream()),
                   "resize_bilinear")
        return y

    @staticmethod
    def backward(ctx, gy):
        shape, planes, H, W, Ho, Wo, align = ctx.meta
        gy = _f(gy)
        gx = torch.empty(shape, device=gy.device, dtype=gy.dtype)
        _lib.check(_lib.lib().c2m_resize_bilinear_bwd(_p(gy), _p(gx), planes, H, W, Ho, Wo, align, _dt(gy), _stream()),
                   "resize_bilinear_bwd")
        return gx, None, None, None


def resize_bilinear_grad(x, size, align_corners=False):
    """Differentiable F.interpolate(x, size, mode='bilinear') of a 4-D [N,C,H,W] or 5-D [B,C,T,H,W] tensor (each H x W
    plane resized).  The forward is c2m_resize_bilinear (the same bits as resize_bilinear), the backward its gather-form
    adjoint c2m_resize_bilinear_bwd (no atomics: repeatable bit for bit).  Returns x itself when the size already matches."""
    _dev(x)
    if x.dim() not in (4, 5):
        raise ValueError(f"resize_bilinear_grad takes 4-D or 5-D tensors, got {x.dim()}-D")
    Ho, Wo = int(size[0]), int(size[1])
    if Ho < 1 or Wo < 1:
        raise ValueError(f"resize_bilinear_grad: output size {Ho}x{Wo}")
    if tuple(x.shape[-2:]) == (Ho, Wo):
        return x
    return _ResizeBilinearFn.apply(x, Ho, Wo, 1 if align_corners else 0)


class _MaxPool2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _dev(x)
        x = _f(x)
        N, C, H, W = x.shape
        y = torch.empty(N, C, H // 2, W // 2, device=x.device, dtype=x.dtype)
        _lib.check(_lib.lib().c2m_maxpool2x2_fwd(_p(x), _p(y), N * C, H, W, _dt(x), _stream()), "maxpool")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        N, C, H, W = x.shape
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().c2m_maxpool2x2_bwd(_p(x), _p(_as(gy, x.dtype)), _p(gx), N * C, H, W, _dt(x), _stream()),
                   "maxpool_bwd")
        return gx


def maxpool2x2(x):
    return _MaxPool2Fn.apply(x)


class _RoiAlignFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, boxes, ph, pw, scale):
        _dev(feat, boxes)
        ctx.feat_dtype = feat.dtype
        feat, boxes = _as(feat, torch.float32), _as(boxes, torch.float32)      # a [B,64,32,64] map: fp32 kernel, cast once
        N, C, H, W = feat.shape
        K = boxes.shape[0]
        out = torch.empty(K, C, ph, pw, device=feat.device, dtype=torch.float32)
        _lib.check(_lib.lib().c2m_roi_align_fwd(_p(feat), _p(boxes), _p(out), K, C, H, W, ph, pw, scale, _stream()),
                   "roi_align")
        ctx.cfg = (N, C, H, W, K, ph, pw, scale)
        ctx.save_for_backward(boxes)
        return out

    @staticmethod
    def backward(ctx, gout):
        (boxes,) = ctx.saved_tensors
        N, C, H, W, K, ph, pw, scale = ctx.cfg
        gfeat = torch.empty(N, C, H, W, device=gout.device, dtype=torch.float32)
        _lib.check(_lib.lib().c2m_roi_align_bwd(_p(boxes), _p(_as(gout, torch.float32)), _p(gfeat), N, K, C, H, W, ph, pw,
                                                scale, _stream()), "roi_align_bwd")
        return gfeat if gfeat.dtype == ctx.feat_dtype else gfeat.to(ctx.feat_dtype), None, None, None, None


def roi_align(feat, boxes, output_size, spatial_scale=1.0):
    """torchvision.ops.roi_align(feat, boxes[K,5], output_size, spatial_scale) with aligned=False, sampling_ratio=-1."""
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    return _RoiAlignFn.apply(feat, boxes.to(torch.float32), int(ph), int(pw), float(spatial_scale))


# =============================================================================================== object GNN
class _GatDenseFn(torch.autograd.Function):
    """Attention of a GATv2 layer on a dense graph of <= 64 nodes (csrc/gnn.hip): one launch forward, two backward."""

    @staticmethod
    def forward(ctx, xl, xr, att, A, slope):
        _dev(xl, xr, att, A)
        xl, xr, att, A = (_as(t, torch.float32) for t in (xl, xr, att, A))
        N, H, C = xl.shape
        assert xr.shape == (N, H, C) and att.shape == (H, C) and A.shape == (N, N)
        out = torch.empty(N, C, device=xl.device, dtype=torch.float32)
        alpha = torch.empty(N, N, H, device=xl.device, dtype=torch.float32)
        _lib.check(_lib.lib().c2m_gat_dense_fwd(_p(xl), _p(xr), _p(att), _p(A), _p(out), _p(alpha), N, H, C, float(slope), _stream()),
                   "gat_dense_fwd")
        ctx.slope = float(slope)
        ctx.save_for_backward(xl, xr, att, alpha)
        return out

    @staticmethod
    def backward(ctx, g):
        xl, xr, att, alpha = ctx.saved_tensors
        N, H, C = xl.shape
        L = _lib.lib()
        dxl, dxr, datt = torch.empty_like(xl), torch.empty_like(xr), torch.empty_like(att)
        ws = torch.empty(L.c2m_gat_dense_bwd_workspace_floats(N, H, C), device=xl.device, dtype=torch.float32)
        _lib.check(L.c2m_gat_dense_bwd(_p(xl), _p(xr), _p(att), _p(alpha), _p(_as(g, torch.float32)), _p(dxl), _p(dxr), _p(datt), _p(ws),
                                       N, H, C, ctx.slope, _stream()), "gat_dense_bwd")
        return dxl, dxr, datt, None, None


GAT_DENSE_MAX_NODES, GAT_DENSE_MAX_CHANNELS = 64, 1024
_GAT_FUSED = True


def gatv2_dense_ok(xl, N, C):
    return _GAT_FUSED and xl.is_cuda and xl.dtype == torch.float32 and N <= GAT_DENSE_MAX_NODES and C <= GAT_DENSE_MAX_CHANNELS


def gatv2_dense(xl, xr, att, A, negative_slope=0.2):
    """mean over heads of softmax_j(att . lrelu(xl[j] + xr[i]); weights A[i, j]) applied to xl -- the message passing of
    GATv2Conv(concat=False, add_self_loops=False) for all ordered node pairs (thirdparty.GATv2Conv adds the bias).  xl, xr [N, H, C],
    att [H, C], A [N, N] edge multiplicities; returns [N, C]."""
    return _GatDenseFn.apply(xl, xr, att, A, negative_slope)


# =============================================================================================== index / mask path
def sparse_raster(instance, obj_id, obj_batch, thetas):
    """instance [B,H,W] float ids, obj_id/obj_batch [K], thetas [K,T,6] -> (bw [B,2,T,H,W], fw, bin [B,1,T,H,W])."""
    _dev(instance, thetas)
    instance, thetas = _as(instance, torch.float32), _as(thetas.detach(), torch.float32)
    B, H, W = instance.shape
    K, T = thetas.shape[0], thetas.shape[1]
    oid = obj_id.to(device=instance.device, dtype=torch.int32).contiguous()
    ob = obj_batch.to(device=instance.device, dtype=torch.int32).contiguous()
    bw = torch.empty(B, 2, T, H, W, device=instance.device, dtype=torch.float32)
    fw = torch.empty_like(bw)
    binm = torch.empty(B, 1, T, H, W, device=instance.device, dtype=torch.float32)
    _lib.check(_lib.lib().c2m_sparse_raster(_p(instance), _p(oid), _p(ob), _p(thetas), _p(bw), _p(fw), _p(binm), B, K, T,
                                            H, W, _stream()), "sparse_raster")
    return bw, fw, binm


def _instance_input(instance, num_input_frames):
    """[B,1,T,H,W] or [B,T,H,W] integer ids on the device -> contiguous int32 [B,T,H,W] (no copy for an int32 input)."""
    _hip_only(instance)
    if instance.dim() == 5:
        if instance.shape[1] != 1:
            raise ValueError(f"instance maps must be [B,1,T,H,W] or [B,T,H,W], got {tuple(instance.shape)}")
        instance = instance[:, 0]
    if instance.dim() != 4:
        raise ValueError(f"instance maps must be [B,1,T,H,W] or [B,T,H,W], got {tuple(instance.shape)}")
    if instance.dtype.is_floating_point or instance.dtype == torch.bool or instance.is_complex():
        raise TypeError(f"instance maps hold integer ids, got {instance.dtype}")
    if not 1 <= num_input_frames <= instance.shape[1]:
        raise ValueError(f"num_input_frames={num_input_frames} but the maps have {instance.shape[1]} frames")
    _on_current_device(instance)
    return _f(instance if instance.dtype == torch.int32 else instance.to(torch.int32))


def _id_range(id_range):
    id_lo, id_hi = (int(v) for v in id_range)
    if not 0 <= id_lo < id_hi:
        raise ValueError(f"id_range must satisfy 0 <= lo < hi, got {id_range}")
    return id_lo, id_hi


def _node_limits(min_pixels, max_nodes):
    min_pixels, max_nodes = int(min_pixels), int(max_nodes)
    if min_pixels < 1 or max_nodes < 1:
        raise ValueError("min_pixels and max_nodes must be >= 1")
    return min_pixels, max_nodes


def instance_stats(instance, num_input_frames, id_range=(1000, 19000)):
    """Per-instance pixel statistics of the first `num_input_frames` frames: int32 [B, t_in, id_hi - id_lo, 5] on the device,
    (count, x_min, x_max, y_min, y_max) of every id in [id_lo, id_hi) (an absent id: count 0, x_min = y_min = 2**31 - 1,
    x_max = y_max = -1).  Integer atomics only: the table is the same on every run."""
    inst = _instance_input(instance, num_input_frames)
    id_lo, id_hi = _id_range(id_range)
    B, T, H, W = inst.shape
    table = torch.empty(B, num_input_frames, id_hi - id_lo, 5, device=inst.device, dtype=torch.int32)
    _lib.check(_lib.lib().c2m_instance_stats(_p(inst), _p(table), B, T, num_input_frames, H, W, id_lo, id_hi, _stream()),
               "instance_stats")
    return table


def instance_boxes(instance, num_input_frames, id_range=(1000, 19000), min_pixels=1, max_nodes=64):
    """The objects of every sample: ids in `id_range` that cover >= `min_pixels` pixels in EACH of the first
    `num_input_frames` frames, in ascending id order, with their pixel boxes per input frame.

    instance: [B,1,T,H,W] or [B,T,H,W] integer ids on the device.  The default range is the rule of
    graph.scene_graph: class id // 1000 < 19, ids below 1000 are stuff / background.
    Returns CPU tensors (one device -> host read; the graph size depends on the data):
      ids [B, max_nodes] int32, boxes [B, max_nodes, t_in, 4] int32 (x_min, y_min, x_max + 1, y_max + 1: pixel edges),
      count [B] int32; slots past count[b] are zero.  More than `max_nodes` objects in a sample raises ValueError."""
    t_in = int(num_input_frames)
    min_pixels, max_nodes = _node_limits(min_pixels, max_nodes)
    table = instance_stats(instance, t_in, id_range)
    B, nid = table.shape[0], table.shape[2]
    n_ids, n_box = B * max_nodes, B * max_nodes * t_in * 4
    out = torch.empty(n_ids + n_box + 2 * B, device=table.device, dtype=torch.int32)
    ids, boxes = out[:n_ids], out[n_ids:n_ids + n_box]
    count, overflow = out[n_ids + n_box:n_ids + n_box + B], out[n_ids + n_box + B:]
    if B:
        _lib.check(_lib.lib().c2m_instance_compact(_p(table), _p(ids), _p(boxes), _p(count), _p(overflow), B, t_in, nid,
                                                   int(id_range[0]), min_pixels, max_nodes, _stream()), "instance_compact")
    host = out.cpu()
    ids, boxes = host[:n_ids].view(B, max_nodes), host[n_ids:n_ids + n_box].view(B, max_nodes, t_in, 4)
    count, overflow = host[n_ids + n_box:n_ids + n_box + B], host[n_ids + n_box + B:]
    bad = overflow.nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"sample(s) {bad} hold more than max_nodes={max_nodes} objects; the object graph is complete "
                         "(N*(N-1) edges), raise max_nodes or min_pixels")
    return ids, boxes, count


# ---- linking the objects of two instance maps (csrc/instance_link.hip; c2m_amd.tracking is the public interface) ------------
def _link_nodes(max_nodes, min_pixels=1):
    min_pixels, max_nodes = _node_limits(min_pixels, max_nodes)
    cap = _lib.lib().c2m_instance_link_max_nodes()
    if max_nodes > cap:
        raise ValueError(f"max_nodes={max_nodes} is above the kernel cap of {cap} (one wave holds a plane's objects)")
    return max_nodes, min_pixels


def _link_i32(name, t, shape):
    """An int32 device tensor of exactly `shape` on the current device, contiguous."""
    _hip_only(t, required=True)
    if t.dtype != torch.int32:
        raise TypeError(f"{name} must be int32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    _on_current_device(t)
    return _f(t)


def instance_slots(table, id_range=(1000, 19000), min_pixels=1, max_nodes=64):
    """Per plane of an instance_stats table [..., id_hi - id_lo, 5], the ids with count >= min_pixels in ascending order; an
    id's position in that list is its slot.  Unlike instance_boxes every plane (sample, frame) is compacted on its own.

    Returns device tensors, int32, with the table's leading dimensions [...]: slot_ids [..., max_nodes] (-1 past count),
    boxes [..., max_nodes, 4] pixel edges (x_min, y_min, x_max + 1, y_max + 1) and areas [..., max_nodes] (zero past count),
    count [...], overflow [...] (1: the plane holds more than max_nodes such ids; the rest is dropped).  Nothing is read back."""
    max_nodes, min_pixels = _link_nodes(max_nodes, min_pixels)
    id_lo, id_hi = _id_range(id_range)
    _hip_only(table, required=True)
    if table.dim() < 2 or tuple(table.shape[-2:]) != (id_hi - id_lo, 5):
        raise ValueError(f"table must be [..., {id_hi - id_lo}, 5] for id_range {id_range}, got {list(table.shape)}")
    lead = tuple(table.shape[:-2])
    table = _link_i32("table", table, table.shape)
    planes = 1
    for n in lead:
        planes *= n
    dev = table.device
    slot_ids = torch.empty(lead + (max_nodes,), device=dev, dtype=torch.int32)
    boxes = torch.empty(lead + (max_nodes, 4), device=dev, dtype=torch.int32)
    areas = torch.empty(lead + (max_nodes,), device=dev, dtype=torch.int32)
    count = torch.empty(lead, device=dev, dtype=torch.int32)
    overflow = torch.empty(lead, device=dev, dtype=torch.int32)
    if planes:
        _lib.check(_lib.lib().c2m_instance_slots(_p(table), _p(slot_ids), _p(boxes), _p(areas), _p(count), _p(overflow), planes,
                                                 id_hi - id_lo, id_lo, min_pixels, max_nodes, _stream()), "instance_slots")
    return slot_ids, boxes, areas, count, overflow


def instance_overlap(ref, frame, flow, ref_slots, ref_count, frame_slots, frame_count):
    """Contingency table of two instance maps: pairs [P, max_nodes + 1, max_nodes + 1] int32 on the device, pairs[p, i, j] = the
    number of pixels q of frame[p] whose id is frame_slots[p, j] and whose source pixel in ref[p] holds ref_slots[p, i]; the last
    row / column count the pixels without a slot (background, stuff, below min_pixels).

    ref, frame [P,H,W] int32; flow [P,2,H,W] fp32 in pixels, defined on the frame's pixels and pointing into ref -- the source
    pixel is the one label_warp reads (same coordinates, border clamp, ties to even) -- or None: the source pixel is q itself
    (plain overlap; no coordinate is computed).  ref_slots / frame_slots [P, max_nodes] and ref_count /
    frame_count [P]: instance_slots of the two maps.  One pass over the pixels, int32 atomics only: bit-repeatable."""
    if not isinstance(ref, torch.Tensor) or ref.dim() != 3:
        raise ValueError(f"ref must be [P,H,W], got {list(getattr(ref, 'shape', ()))}")
    P, H, W = ref.shape
    if not isinstance(ref_slots, torch.Tensor) or ref_slots.dim() != 2:
        raise ValueError(f"ref_slots must be [P, max_nodes], got {list(getattr(ref_slots, 'shape', ()))}")
    M, _ = _link_nodes(ref_slots.shape[1])
    ref, frame = _link_i32("ref", ref, (P, H, W)), _link_i32("frame", frame, (P, H, W))
    ref_slots, frame_slots = _link_i32("ref_slots", ref_slots, (P, M)), _link_i32("frame_slots", frame_slots, (P, M))
    ref_count, frame_count = _link_i32("ref_count", ref_count, (P,)), _link_i32("frame_count", frame_count, (P,))
    if H * W >= 2 ** 31:
        raise ValueError(f"a plane of {H}x{W} pixels is too large (H * W must be below 2**31)")
    if flow is not None:
        _hip_only(flow)
        if flow.dtype != torch.float32:
            raise TypeError(f"flow must be fp32 (coordinates are never rounded), got {flow.dtype}")
        if tuple(flow.shape) != (P, 2, H, W):
            raise ValueError(f"flow must be {[P, 2, H, W]} (at the size of the maps), got {list(flow.shape)}")
        _on_current_device(flow)
        flow = _f(flow.detach())
    pairs = torch.empty(P, M + 1, M + 1, device=ref.device, dtype=torch.int32)
    if P:
        _lib.check(_lib.lib().c2m_instance_overlap(_p(ref), _p(frame), _p(flow), _p(ref_slots), _p(ref_count), _p(frame_slots),
                                                   _p(frame_count), _p(pairs), P, H, W, M, _stream()), "instance_overlap")
    return pairs


def instance_match(pairs, ref_slots, ref_count, frame_slots, frame_count, min_iou=(1, 4), same_class=True):
    """Mutual best match of an instance_overlap table: link [P, max_nodes] int32 on the device, the frame slot of every ref slot
    or -1.  With r_i / a_j the row / column sums of pairs[p] and IoU(i, j) = n_ij / (r_i + a_j - n_ij), frame slot j is linked to
    ref slot i iff i has the largest IoU in column j, j has the largest IoU in row i (cells with n = 0 never count, ties go to the
    lower id), IoU >= min_iou = (num, den), exactly equal passing, and -- with same_class -- both ids have the same id // 1000.
    Integer arithmetic throughout (64-bit cross-multiplication)."""
    if not isinstance(ref_slots, torch.Tensor) or ref_slots.dim() != 2:
        raise ValueError(f"ref_slots must be [P, max_nodes], got {list(getattr(ref_slots, 'shape', ()))}")
    P = ref_slots.shape[0]
    M, _ = _link_nodes(ref_slots.shape[1])
    try:
        num, den = (int(v) for v in min_iou)
    except (TypeError, ValueError):
        raise ValueError(f"min_iou must be a rational (num, den) of two integers, got {min_iou!r}") from None
    if tuple(min_iou) != (num, den) or not (0 <= num <= den and 1 <= den < 2 ** 31):
        raise ValueError(f"min_iou must be a rational (num, den) of two integers with 0 <= num <= den, got {min_iou!r}")
    pairs = _link_i32("pairs", pairs, (P, M + 1, M + 1))
    ref_slots, frame_slots = _link_i32("ref_slots", ref_slots, (P, M)), _link_i32("frame_slots", frame_slots, (P, M))
    ref_count, frame_count = _link_i32("ref_count", ref_count, (P,)), _link_i32("frame_count", frame_count, (P,))
    link = torch.empty(P, M, device=pairs.device, dtype=torch.int32)
    if P:
        _lib.check(_lib.lib().c2m_instance_match(_p(pairs), _p(ref_slots), _p(ref_count), _p(frame_slots), _p(frame_count),
                                                 _p(link), P, M, num, den, 1 if same_class else 0, _stream()), "instance_match")
    return link


_RelabelPlan = collections.namedtuple("_RelabelPlan", "P HW table things label_divisor")


def _instance_relabel_plan(maps, pairs_from, pairs_to, count, thing_list, label_divisor):
    """Every check of instance_relabel, made before anything is launched (host tensors pass: the device is the launch path's
    check), and the host half of it: each plane's pairs sorted by `from` and padded to the kernel's 64 -> table, flat int32:
    from [P, 64] | to [P, 64] | count [P]."""
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.int32 or maps.dim() < 3:
        raise ValueError("maps must be an int32 tensor [..., H, W] with at least one leading axis, got "
                         f"{(maps.dtype, tuple(maps.shape)) if isinstance(maps, torch.Tensor) else type(maps).__name__}")
    if not maps.is_contiguous():
        raise ValueError("maps must be contiguous")
    H, W = maps.shape[-2:]
    P = int(np.prod(maps.shape[:-2]))
    if H * W >= 2 ** 31 or P >= 2 ** 24:
        raise ValueError(f"{P} planes of {H}x{W} pixels: too many planes or too large a plane (H * W must be below 2**31)")
    try:
        label_divisor = int(label_divisor)
        things = tuple(sorted(set(int(c) for c in thing_list)))
    except (TypeError, ValueError):
        raise ValueError("label_divisor must be an integer and thing_list a list of class ids") from None
    if not 1 <= label_divisor < 2 ** 31:
        raise ValueError(f"label_divisor must be in 1..2**31-1, got {label_divisor}")
    if any(not 0 <= c <= 255 for c in things):
        raise ValueError(f"thing_list must lie in 0..255, got {list(thing_list)}")
    cap = 64                                                      # c2m_instance_link_max_nodes(): one LDS list per plane
    frm, to, cnt = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in (pairs_from, pairs_to, count))
    if frm.ndim != 2 or frm.shape != to.shape or frm.shape[0] != P or frm.shape[1] > cap or cnt.shape != (P,) or \
            any(a.dtype.kind not in "iu" for a in (frm, to, cnt)):
        raise ValueError(f"pairs_from and pairs_to must be integer [P={P}, n <= {cap}] and count [P={P}], got {frm.shape}, "
                         f"{to.shape} and {cnt.shape}")
    n = frm.shape[1]
    if cnt.size and (cnt.min() < 0 or cnt.max() > n):
        raise ValueError(f"count must lie in 0..{n}")
    live = np.arange(n)[None] < cnt[:, None]                      # also the live entries after the sort: padding sorts last
    frm, to = frm.astype(np.int64), to.astype(np.int64)
    for a in (frm, to):
        if live.any() and (a[live].min() < -2 ** 31 or a[live].max() >= 2 ** 31 - 1):
            raise ValueError("pair values must be int32 below 2**31 - 1 (the list's padding)")
    key = np.where(live, frm, 2 ** 31 - 1)
    order = np.argsort(key, axis=1, kind="stable")
    key = np.take_along_axis(key, order, 1)
    if n > 1 and ((key[:, 1:] == key[:, :-1]) & live[:, 1:]).any():
        raise ValueError("a plane lists one `from` value twice: the mapping must be a function")
    table = np.zeros((2, P, cap), np.int32)
    table[0, :, :n] = np.where(live, key, 0)
    table[1, :, :n] = np.where(live, np.take_along_axis(to, order, 1), 0)
    table = np.concatenate([table.reshape(-1), cnt.astype(np.int32)])
    return _RelabelPlan(P, H * W, table, things, label_divisor)


def instance_relabel(maps, pairs_from, pairs_to, count, thing_list, label_divisor=1000):
    """Every plane of int32 maps [..., H, W] rewritten through its own list of (from, to) pairs (csrc/instance_link.hip:
    c2m_instance_relabel; the contract is in include/c2m_hip.h): a value equal to a `from` becomes its `to`, all at once (two ids
    may swap); every other thing value (v >= label_divisor, v // label_divisor in thing_list) becomes its class's crowd id
    (v // label_divisor) * label_divisor; stuff and void stay.  pairs_from, pairs_to: host integers [P, n <= 64], count [P] (the
    pairs of plane p are the first count[p]; any order).  Returns a new tensor of the shape of maps; one upload and one launch on
    the current stream."""
    pl = _instance_relabel_plan(maps, pairs_from, pairs_to, count, thing_list, label_divisor)
    _hip_only(maps)
    _on_current_device(maps)
    maps = maps.detach()
    out = torch.empty_like(maps)
    if pl.P and pl.HW:
        thing, _ = _panoptic_tables(pl.things, maps.device)
        tab = torch.from_numpy(pl.table).to(maps.device)
        n = pl.P * 64
        _lib.check(_lib.lib().c2m_instance_relabel(_p(maps), _p(out), _p(tab[:n]), _p(tab[n:2 * n]), _p(tab[2 * n:]), _p(thing),
                                                   pl.P, pl.HW, pl.label_divisor, _stream()), "instance_relabel")
    return out


def occlusion_splat(flow, want_map=True, want_clip=False):
    """get_occlusion_map for [B,2,H,W] or, frame-batched, [B,2,T,H,W] flows -> ([B,1,(T,)H,W] map, clip_mask) ."""
    _dev(flow)
    flow = _as(flow.detach(), torch.float32)
    five = flow.dim() == 5
    if five:
        B, _, T, H, W = flow.shape
        sb, sc, st = 2 * T * H * W, T * H * W, H * W
        oshape = (B, 1, T, H, W)
    else:
        B, _, H, W = flow.shape
        T, sb, sc, st = 1, 2 * H * W, H * W, 0
        oshape = (B, 1, H, W)
    L = _lib.lib()
    ws = torch.empty(L.c2m_occlusion_splat_workspace_bytes(B * T, H, W), device=flow.device, dtype=torch.uint8)
    occ = torch.empty(oshape, device=flow.device, dtype=torch.float32) if want_map else None
    clip = torch.empty(oshape, device=flow.device, dtype=torch.float32) if want_clip else None
    _lib.check(L.c2m_occlusion_splat(_p(flow), sb, sc, st, B, T, H, W, _p(occ), _p(clip), _p(ws), _stream()),
               "occlusion_splat")
    return occ, clip


def _label_warp_plan(flow, planes_f, planes_i, occ, threshold):
    """Shapes and dtypes of label_warp, checked before anything is launched: (B, T, H, W, Cf, Ci)."""
    if flow.dim() not in (4, 5) or flow.shape[1] != 2:
        raise ValueError(f"flow must be [B,2,T,H,W] or [B,2,H,W], got {tuple(flow.shape)}")
    if flow.dtype != torch.float32:
        raise ValueError(f"flow must be fp32 (coordinates are never rounded), got {flow.dtype}")
    B, (H, W) = flow.shape[0], flow.shape[-2:]
    T = flow.shape[2] if flow.dim() == 5 else 1
    if planes_f is None and planes_i is None:
        raise ValueError("label_warp needs planes_f or planes_i")
    chans = []
    for name, t, dtype in (("planes_f", planes_f, torch.float32), ("planes_i", planes_i, torch.int32)):
        if t is None:
            chans.append(0)
            continue
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[-2:]) != (H, W):
            raise ValueError(f"{name} must be [{B},C,{H},{W}] for flow {tuple(flow.shape)}, got {tuple(t.shape)}")
        chans.append(t.shape[1])
    if occ is not None:
        if threshold is None:
            raise ValueError("occ needs a threshold")
        if occ.dtype != torch.float32:
            raise ValueError(f"occ must be fp32, got {occ.dtype}")
        want = (B, 1, T, H, W) if flow.dim() == 5 else (B, 1, H, W)
        if tuple(occ.shape) != want:
            raise ValueError(f"occ must be {want} for flow {tuple(flow.shape)}, got {tuple(occ.shape)}")
    elif threshold is not None:
        raise ValueError("a threshold needs occ")
    return B, T, H, W, chans[0], chans[1]


def label_warp(flow, planes_f=None, planes_i=None, occ=None, threshold=None, fill_id=0):
    """Label maps of one frame carried along a backward flow, nearest neighbour: out[b, c, t, y, x] = planes[b, c, sy, sx] with
    (sx, sy) the pixel nearest (ties to even) to the position flow_warp reads for (x, y) under flow[b, :, t] -- the same
    coordinates, after the border clamp (csrc/warp_coord.h).  Nothing is blended: ids stay ids, one-hot stays one-hot.

    flow [B,2,T,H,W] fp32 in pixels (a view with dense rows is read in place) or [B,2,H,W] (T = 1); planes_f [B,Cf,H,W] fp32,
    planes_i [B,Ci,H,W] int32, either may be None or have 0 channels.  occ [B,1,T,H,W] (or [B,1,H,W]) with `threshold`: where
    occ < threshold the INTEGER outputs are `fill_id`; float planes are not touched there, so they name the object that used to
    cover the pixel: nearest_fill (below) fills all planes of such pixels from the nearest visible background pixel.
    Returns (out_f [B,Cf,T,H,W] fp32 or None, out_i [B,Ci,T,H,W] int32 or None).  One launch, no atomics, no autograd."""
    _hip_only(flow, planes_f, planes_i, occ)
    B, T, H, W, Cf, Ci = _label_warp_plan(flow, planes_f, planes_i, occ, threshold)
    if not -2 ** 31 <= int(fill_id) < 2 ** 31:
        raise ValueError(f"fill_id must be an int32 value, got {fill_id}")
    _on_current_device(flow, planes_f, planes_i, occ)
    flow = flow.detach()
    if flow.stride(-1) != 1 or flow.stride(-2) != W:
        flow = flow.contiguous()
    sb, sc = flow.stride(0), flow.stride(1)
    st = flow.stride(2) if flow.dim() == 5 else 0
    dev = flow.device
    out_f = None if planes_f is None else torch.empty(B, Cf, T, H, W, device=dev, dtype=torch.float32)
    out_i = None if planes_i is None else torch.empty(B, Ci, T, H, W, device=dev, dtype=torch.int32)
    pf = _f(planes_f.detach()) if Cf else None
    pi = _f(planes_i) if Ci else None
    occ = None if occ is None else _f(occ.detach())
    if B * T * H * W and Cf + Ci:
        _lib.check(_lib.lib().c2m_label_warp(_p(flow), sb, sc, st, _p(occ), float(threshold or 0.0), int(fill_id), _p(pf), Cf,
                                             _p(pi), Ci, B, T, H, W, _p(out_f) if Cf else None, _p(out_i) if Ci else None,
                                             _stream()), "label_warp")
    return out_f, out_i


NEAREST_FILL_MAX_SIDE = 32768       # d^2 of two pixels then fits the upper half of the kernel's 64-bit key


def _nearest_fill_plan(hole, seed, planes_f, planes_i):
    """Every check of nearest_fill, made before anything is launched (host tensors pass: the device is the launch path's
    check, all tensors on ONE device is checked here): (B, T, H, W, Cf, Ci)."""
    for name, t in (("hole", hole), ("seed", seed)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{name} must be a uint8 or bool mask, got {t.dtype}")
        if t.dim() not in (3, 4):
            raise ValueError(f"{name} must be [B,T,H,W] or [B,H,W], got {tuple(t.shape)}")
    if hole.shape != seed.shape:
        raise ValueError(f"hole {tuple(hole.shape)} and seed {tuple(seed.shape)} differ in shape")
    B, (H, W) = hole.shape[0], hole.shape[-2:]
    T = hole.shape[1] if hole.dim() == 4 else 1
    if H > NEAREST_FILL_MAX_SIDE or W > NEAREST_FILL_MAX_SIDE or H * W >= 2 ** 31 or B * T >= 2 ** 31:
        raise ValueError(f"{B * T} frames of {H}x{W} pixels: H and W must be at most {NEAREST_FILL_MAX_SIDE}, H * W and B * T "
                         "below 2**31")
    if planes_f is None and planes_i is None:
        raise ValueError("nearest_fill needs planes_f or planes_i")
    chans = []
    for name, t, dtype in (("planes_f", planes_f, torch.float32), ("planes_i", planes_i, torch.int32)):
        if t is None:
            chans.append(0)
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"{name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if t.dim() != 5 or (t.shape[0], t.shape[2], t.shape[3], t.shape[4]) != (B, T, H, W):
            raise ValueError(f"{name} must be [{B},C,{T},{H},{W}] for masks {tuple(hole.shape)}, got {tuple(t.shape)}")
        if t.numel() and ((W > 1 and t.stride(4) != 1) or (H > 1 and t.stride(3) != W)):
            raise ValueError(f"{name} must have dense rows (strides {W}, 1 of H, W), got strides {tuple(t.stride())}")
        if any(t.shape[d] > 1 and t.stride(d) == 0 for d in (0, 1, 2)):
            raise ValueError(f"{name} is filled in place: an expanded view (stride 0) would be written through several indices")
        if t.device != hole.device:
            raise ValueError(f"{name} is on {t.device} but the masks are on {hole.device}")
        chans.append(t.shape[1])
    if sum(chans) == 0:
        raise ValueError("nearest_fill needs at least one plane (planes_f and planes_i have 0 channels)")
    if seed.device != hole.device:
        raise ValueError(f"hole and seed must be on one device, got {hole.device} and {seed.device}")
    return B, T, H, W, chans[0], chans[1]


def nearest_fill(hole, seed, planes_f=None, planes_i=None):
    """Every hole pixel takes all its label words from the nearest seed pixel of the same image, IN PLACE (csrc/nearest_fill.hip;
    DESIGN.md 4.2k).  For a hole pixel (y, x) of image (b, t) the source is the seed pixel (y', x') of that image with the
    smallest ((y - y')**2 + (x - x')**2, y', x'), compared as integers -- exact Euclidean distance, ties to the smaller row, then
    to the smaller column -- and planes[b, c, t, y, x] = planes[b, c, t, y', x'] for every plane c.  Pixels that are no holes
    are never written, pixels that are no seeds are never read as sources.

    hole, seed: [B,T,H,W] uint8 or bool on the device ([B,H,W]: T = 1), nonzero = set.  A pixel set in BOTH is an error of the
    caller that the host cannot see: the kernel treats it as a hole and never as a seed.  planes_f [B,Cf,T,H,W] fp32, planes_i
    [B,Ci,T,H,W] int32 (what label_warp returns): views with any batch, channel and frame strides and dense rows; either may be
    None or have 0 channels, not both.  Planes are moved as 32-bit words, so every bit pattern survives (NaN payloads, negative
    ids).  Returns unfilled [B,T] int32 on the device: the hole pixels of an image left untouched because the image has no seed.
    Two zero-fills and two launches on the current stream; nothing is copied to the host and nothing synchronises."""
    _hip_only(hole, seed, planes_f, planes_i)
    B, T, H, W, Cf, Ci = _nearest_fill_plan(hole, seed, planes_f, planes_i)
    _on_current_device(hole, seed, planes_f, planes_i)
    dev = hole.device
    as_u8 = lambda m: _f(m.detach().view(torch.uint8) if m.dtype == torch.bool else m.detach())
    hole, seed = as_u8(hole), as_u8(seed)
    unfilled = torch.empty(B, T, device=dev, dtype=torch.int32)
    if B * T:
        L = _lib.lib()
        nbytes = L.c2m_nearest_fill_workspace_bytes(B, T, H, W)
        if nbytes < 0:
            raise ValueError(f"nearest_fill: sizes out of range (B={B}, T={T}, H={H}, W={W})")
        work = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.int64)
        pf = planes_f.detach() if Cf else None
        pi = planes_i.detach() if Ci else None
        fs = (pf.stride(0), pf.stride(1), pf.stride(2)) if Cf else (0, 0, 0)
        si = (pi.stride(0), pi.stride(1), pi.stride(2)) if Ci else (0, 0, 0)
        _lib.check(L.c2m_nearest_fill(_p(hole), _p(seed), _p(pf), *fs, Cf, _p(pi), *si, Ci, B, T, H, W, _p(unfilled), _p(work),
                                      nbytes, _stream()), "nearest_fill")
    return unfilled


# ============================================================================ dataset-resolution output (csrc/detail_warp.hip)
def _detail_warp_plan(frame_u8, generated, warped, flow, occ, ids, occ_threshold):
    """Shapes and dtypes of detail_warp, checked before anything is launched: (B, T, h, w, H, W)."""
    if generated.dim() != 5 or generated.shape[1] != 3:
        raise ValueError(f"generated must be [B,3,T,h,w], got {tuple(generated.shape)}")
    B, _, T, h, w = generated.shape
    if h < 2 or w < 2:
        raise ValueError(f"the working size must be at least 2x2 (the flow's coordinate rule divides by h - 1, w - 1), got {h}x{w}")
    for name, t, c, dtypes in (("generated", generated, 3, (torch.float32, torch.bfloat16)),
                               ("warped", warped, 3, (torch.float32, torch.bfloat16)),
                               ("flow", flow, 2, (torch.float32,)), ("occ", occ, 1, (torch.float32, torch.bfloat16))):
        if t is None and name == "occ":
            continue
        if tuple(t.shape) != (B, c, T, h, w):
            raise ValueError(f"{name} must be {(B, c, T, h, w)} for generated {tuple(generated.shape)}, got {tuple(t.shape)}")
        if t.dtype not in dtypes:
            raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}"
                             f"{' (coordinates are never rounded)' if name == 'flow' else ''}, got {t.dtype}")
    if frame_u8.dtype != torch.uint8:
        raise ValueError(f"frame_u8 must be uint8, got {frame_u8.dtype}")
    if frame_u8.dim() != 4 or frame_u8.shape[0] != B or frame_u8.shape[3] != 3:
        raise ValueError(f"frame_u8 must be [{B},H,W,3], got {tuple(frame_u8.shape)}")
    H, W = frame_u8.shape[1:3]
    if H < h or W < w:
        raise ValueError(f"the output size {H}x{W} is below the working size {h}x{w}: down-scaling is not supported")
    if H * W * 3 >= 2 ** 31:
        raise ValueError(f"one {H}x{W} frame has 2^31 bytes or more")
    if ids is not None:
        if ids.dtype != torch.int32:
            raise ValueError(f"ids must be int32, got {ids.dtype}")
        if tuple(ids.shape) != (B, H, W):
            raise ValueError(f"ids must be {(B, H, W)} for frame_u8 {tuple(frame_u8.shape)}, got {tuple(ids.shape)}")
    if occ_threshold is not None:
        if ids is None:
            raise ValueError("occ_threshold marks disoccluded ids: it needs ids")
        if occ is None:
            raise ValueError("a threshold needs occ")
    return B, T, h, w, H, W


def detail_warp(frame_u8, generated, warped, flow, occ=None, ids=None, occ_threshold=None, fill_id=0):
    """Predicted frames at the size of `frame_u8`: its sharp pixels moved along the working-size backward flow, the generator's
    output supplying the rest.  With up() the bilinear enlargement (align_corners=False) and warpF the bilinear value of
    frame_u8 where the working-size warp reads, mapped to the large grid (csrc/warp_coord.h, border clamp included):
        level = floor(clip(255 up(generated) + up(occ) * (warpF - 255 up(warped)), 0, 255) + 0.5)

    frame_u8 [B,H,W,3] uint8: the last input frame at the output size; generated, warped [B,3,T,h,w] (fp32 or bf16), warped =
    flow_warp of the working-size frame by `flow`, no occlusion; flow [B,2,T,h,w] fp32 in working-size pixels; occ [B,1,T,h,w]
    or None (1 everywhere); 2 <= h <= H, 2 <= w <= W.  ids [B,H,W] int32: carried to the nearest pixel of the same position, never
    blended; with occ_threshold, fill_id where up(occ) < occ_threshold.
    Returns (uint8 [B,T,H,W,3], int32 [B,T,H,W] or None).  One launch, no atomics, no autograd."""
    ts = (frame_u8, generated, warped, flow, occ, ids)
    _hip_only(*ts)
    B, T, h, w, H, W = _detail_warp_plan(frame_u8, generated, warped, flow, occ, ids, occ_threshold)
    if not -2 ** 31 <= int(fill_id) < 2 ** 31:
        raise ValueError(f"fill_id must be an int32 value, got {fill_id}")
    _on_current_device(*ts)
    frame_u8, ids = _f(frame_u8), None if ids is None else _f(ids)
    generated, warped = _as(generated.detach(), torch.float32), _as(warped.detach(), torch.float32)
    flow, occ = _f(flow.detach()), None if occ is None else _as(occ.detach(), torch.float32)
    out = torch.empty(B, T, H, W, 3, device=frame_u8.device, dtype=torch.uint8)
    out_ids = None if ids is None else torch.empty(B, T, H, W, device=frame_u8.device, dtype=torch.int32)
    if B * T:
        thr = float("-inf") if occ_threshold is None else float(occ_threshold)
        _lib.check(_lib.lib().c2m_detail_warp(_p(frame_u8), _p(generated), _p(warped), _p(flow), _p(occ), _p(ids), thr,
                                              int(fill_id), B, T, h, w, H, W, _p(out), _p(out_ids), _stream()), "detail_warp")
    return out, out_ids


# ====================================================================================== frame quality (csrc/quality.hip)
QUALITY_TAPS = 11
QUALITY_SIGMA = 1.5
SCORE_ROWS = 9              # csrc/score_rows.h: the whole frame, then region bits 0..7; every score kernel writes [..., 9, K]
QUALITY_ROWS = SCORE_ROWS


def quality_weights():
    """The eleven taps of the SSIM window, float64: exp(-i^2 / (2 sigma^2)), i = -5..5, normalised to sum 1."""
    i = np.arange(QUALITY_TAPS, dtype=np.float64) - QUALITY_TAPS // 2
    w = np.exp(-(i * i) / (2.0 * QUALITY_SIGMA * QUALITY_SIGMA))
    return w / w.sum()


_QUALITY_FLOATS = (torch.float32, torch.bfloat16)


def _frame_quality_plan(pred, target, regions=None):
    """Forms, dtypes and shapes of frame_quality, checked before anything is launched: (form, B, C, T, H, W) with form "float"
    ([B,C,T,H,W] fp32 / bf16, L = 1) or "uint8" ([B,T,H,W,C], L = 255)."""
    for name, t in (("pred", pred), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.dim() != 5:
            raise ValueError(f"{name} must be a 5-d tensor: float [B,C,T,H,W] or uint8 [B,T,H,W,C]")
        if t.dtype != torch.uint8 and t.dtype not in _QUALITY_FLOATS:
            raise ValueError(f"{name} must be fp32, bf16 or uint8, got {t.dtype}")
    if (pred.dtype == torch.uint8) != (target.dtype == torch.uint8):
        raise ValueError(f"pred and target must have the same form (both float [B,C,T,H,W] or both uint8 [B,T,H,W,C]), got "
                         f"{pred.dtype} and {target.dtype}")
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pred.dtype == torch.uint8:
        form, (B, T, H, W, C) = "uint8", pred.shape
    else:
        form, (B, C, T, H, W) = "float", pred.shape
    if C not in (1, 3):
        raise ValueError(f"{form} frames must have 1 or 3 channels, got {C} in {tuple(pred.shape)}")
    if H < QUALITY_TAPS or W < QUALITY_TAPS:
        raise ValueError(f"a frame must hold one {QUALITY_TAPS}x{QUALITY_TAPS} SSIM window, got {H}x{W}")
    if H * W * C >= 2 ** 31:
        raise ValueError(f"one {H}x{W}x{C} frame has 2^31 elements or more")
    if regions is not None:
        if not isinstance(regions, torch.Tensor) or regions.dtype != torch.uint8:
            raise ValueError(f"regions must be a uint8 tensor, got {getattr(regions, 'dtype', type(regions).__name__)}")
        if tuple(regions.shape) != (B, T, H, W):
            raise ValueError(f"regions must be {(B, T, H, W)} for frames {tuple(pred.shape)}, got {tuple(regions.shape)}")
    return form, B, C, T, H, W


def _quality_operand(x, form, H, W, C):
    """x with dense inner dims (a copy only if they are not) and its (B, C, T) strides in elements."""
    s = x.stride()
    if form == "uint8":
        if s[2:] != (W * C, C, 1) or min(s[0], s[1]) < H * W * C:
            x = x.contiguous()
        return x, (x.stride(0), 0, x.stride(1))
    if s[3:] != (W, 1) or min(s[:3]) < H * W:
        x = x.contiguous()
    return x, x.stride()[:3]


def frame_quality(pred, target, regions=None):
    """Per-frame squared error and SSIM sums of `pred` against `target`: float64 [B,T,9,4] on the device, row 0 the whole frame,
    row 1 + k the pixels whose `regions` byte has bit k; columns (n_pixels, sse, n_windows, ssim_sum).

    Both operands float [B,C,T,H,W] (fp32 or bf16, nominal range [0,1], L = 1, not clamped) or both uint8 [B,T,H,W,C] (L = 255,
    on the integer levels); C 1 or 3; H, W >= 11.  B- and T-strided views (frames[:, t_in:], video[:, :, t_in:]) go in without a
    copy.  regions: uint8 [B,T,H,W] or None.  sse counts every pixel; ssim_sum the centres whose 11x11 Gaussian window (sigma
    1.5) lies inside the frame, SSIM as skimage's structural_similarity(gaussian_weights=True, use_sample_covariance=False)
    computes it, in fp64.  Two launches, no atomics, bit-repeatable, no autograd."""
    _hip_only(pred, target, regions)
    form, B, C, T, H, W = _frame_quality_plan(pred, target, regions)
    _on_current_device(pred, target, regions)
    pred, target = pred.detach(), target.detach()
    if pred.dtype != target.dtype:                       # fp32 against bf16: bf16 -> fp32 is exact
        pred, target = pred.float(), target.float()
    pred, sp = _quality_operand(pred, form, H, W, C)
    target, st = _quality_operand(target, form, H, W, C)
    regions = None if regions is None else _f(regions)
    out = torch.zeros(B, T, QUALITY_ROWS, 4, device=pred.device, dtype=torch.float64)
    if B * T:
        L = _lib.lib()
        nbytes = L.c2m_frame_quality_workspace_bytes(B, T, H, W)
        work = torch.empty(nbytes // 8, device=pred.device, dtype=torch.float64)
        code = 2 if form == "uint8" else _dt(pred)
        w = quality_weights()
        _lib.check(L.c2m_frame_quality(_p(pred), _p(target), _p(regions), code, B, C, T, H, W, (ctypes.c_long * 3)(*sp),
                                       (ctypes.c_long * 3)(*st), w.ctypes.data_as(ctypes.c_void_p),
                                       255.0 if form == "uint8" else 1.0, _p(work), nbytes, _p(out), _stream()), "frame_quality")
    return out


# =============================================================================================== rendering (csrc/render.hip)
def _sheet_plan(name, x, channels, size, dtypes=(torch.float32, torch.bfloat16)):
    """Checks of one [B,C,T,H,W] device tensor that becomes a sheet -> (B, C, T, H, W, rows, cols)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if x.dim() != 5 or x.shape[1] not in channels:
        raise ValueError(f"{name} must be [B, C, T, H, W] with C in {tuple(channels)}, got {tuple(x.shape)}")
    rows, cols = (int(v) for v in size)
    if rows < 1 or cols < 1 or x.shape[0] > rows * cols:
        raise ValueError(f"{name}: B = {x.shape[0]} samples do not fit size = {rows} x {cols} cells")
    _hip_only(x, name=name)             # after the shape checks: those are the same with or without a device
    _on_current_device(x, name=name)
    B, C, T, H, W = x.shape
    return B, C, T, H, W, rows, cols


def render_frames(x, size, normalize=False):
    """Frames or one-channel maps [B,C,T,H,W] (C in {1, 3}, fp32 or bf16) -> uint8 sheet [T, rows*H, cols*W, C]; sample b in
    cell (b // cols, b % cols) of size = (rows, cols), the other cells zero.  Level = trunc(clip(x * 255, 0, 255)), with
    normalize (x + 1) / 2 * 255: the reference's tensor2im / tensor2occ bit for bit; NaN -> 0.  One launch."""
    B, C, T, H, W, rows, cols = _sheet_plan("x", x, (1, 3), size)
    with torch.no_grad():
        x = _f(x.detach())
        out = torch.empty(T, rows * H, cols * W, C, device=x.device, dtype=torch.uint8)
        if out.numel():
            _lib.check(_lib.lib().c2m_render_frames(_p(x), _dt(x), B, C, T, H, W, rows, cols, int(bool(normalize)), _p(out),
                                                    _stream()), "render_frames")
    return out


def render_flow(flow, size, scale=None):
    """Flow [B,2,T,H,W] in pixels -> uint8 RGB sheet [T, rows*H, cols*W, 3] in the Middlebury colour code.  scale None: every
    frame's sheet is normalised by its largest radius over ALL samples (the reference's tensor2flow; |component| > 1e7 is
    unknown = black, an all-zero sheet is black); scale s: u * s, v * s without normalisation (compute_flow_color_map, s = 3).
    Empty cells hold zero flow (near-white / white).  NaN components -> black."""
    B, _, T, H, W, rows, cols = _sheet_plan("flow", flow, (2,), size)
    with torch.no_grad():
        flow = _f(flow.detach())
        out = torch.empty(T, rows * H, cols * W, 3, device=flow.device, dtype=torch.uint8)
        if out.numel():
            L = _lib.lib()
            ws = None if scale is not None else torch.empty(max(L.c2m_render_flow_workspace_bytes(T) // 8, 1), device=flow.device,
                                                            dtype=torch.int64)
            _lib.check(L.c2m_render_flow(_p(flow), _dt(flow), B, T, H, W, rows, cols, 0 if scale is None else 1,
                                         float(scale or 0.0), _p(out), _p(ws), _stream()), "render_flow")
    return out


def _u8_table(name, t, device, last=3):
    t = torch.as_tensor(t)
    if t.dtype != torch.uint8 or t.dim() < 1 or t.shape[-1] != last:
        raise ValueError(f"{name} must be uint8 [..., {last}], got {t.dtype} {tuple(t.shape)}")
    return _f(t.to(device))


def render_instances(ids, size, palette, base=None, id_range=(1000, 19000), alpha=128):
    """Instance ids [B,1,T,H,W] int32 -> uint8 RGB sheet: pixels with lo <= id < hi tinted with palette[id % P]
    ((c * (256 - alpha) + p * alpha) >> 8), instance borders (id differs from a 4-neighbour inside the frame, the reference's
    get_edges) in the solid palette colour of the larger id.  base: an RGB sheet to draw onto (not modified), None = black."""
    B, _, T, H, W, rows, cols = _sheet_plan("ids", ids, (1,), size, dtypes=(torch.int32,))
    lo, hi = (int(v) for v in id_range)
    if lo < 0 or hi < lo:
        raise ValueError(f"id_range must be 0 <= lo <= hi, got {id_range}")
    if not 0 <= int(alpha) <= 256:
        raise ValueError(f"alpha must be in 0..256, got {alpha}")
    palette = _u8_table("palette", palette, ids.device)
    if palette.dim() != 2 or palette.shape[0] < 1:
        raise ValueError(f"palette must be uint8 [P, 3] with P >= 1, got {tuple(palette.shape)}")
    shape = (T, rows * H, cols * W, 3)
    if base is not None:
        if not base.is_cuda or base.dtype != torch.uint8 or tuple(base.shape) != shape:
            raise ValueError(f"base must be a uint8 HIP tensor of shape {shape}, got {base.dtype} {tuple(base.shape)} on {base.device}")
        base = _f(base)
    with torch.no_grad():
        ids = _f(ids)
        out = torch.empty(shape, device=ids.device, dtype=torch.uint8)
        if out.numel():
            _lib.check(_lib.lib().c2m_render_instances(_p(ids), B, T, H, W, rows, cols, _p(base), _p(palette), palette.shape[0], lo,
                                                       hi, int(alpha), _p(out), _stream()), "render_instances")
    return out


def draw_overlays(sheet, size, boxes=None, presence=None, box_colors=None, points=None, point_sample=None, point_count=None,
                  line_colors=None):
    """Draws box outlines and drag paths onto an RGB sheet [T, rows*H, cols*W, 3] uint8 IN PLACE and returns it.

    boxes [B,N,T,4] int32 pixel edges (x0, y0, x1, y1) in cell coordinates and presence [B,N,T] bool (what
    interactive.predicted_boxes returns; CPU tensors are copied over): the 1-pixel outline of [x0, x1-1] x [y0, y1-1] of every
    present box, colour box_colors [B,N,3] uint8; N <= 64.  points [D,P,2] int32 (x, y), point_sample [D] (the sample a path
    belongs to), point_count [D,T] (frame t shows the first point_count[d, t] points and a 3x3 marker on the last of them),
    line_colors [D,3] uint8.  Per pixel the last covering primitive wins: boxes in node order, then paths in order; nothing is
    drawn outside a sample's own cell."""
    _hip_only(sheet, name="sheet", required=True)
    _on_current_device(sheet, name="sheet")
    if sheet.dtype != torch.uint8 or sheet.dim() != 4 or sheet.shape[-1] != 3 or not sheet.is_contiguous():
        raise ValueError(f"sheet must be a contiguous uint8 [T, rows*H, cols*W, 3] tensor, got {sheet.dtype} {tuple(sheet.shape)}")
    rows, cols = (int(v) for v in size)
    T = sheet.shape[0]
    if rows < 1 or cols < 1 or sheet.shape[1] % rows or sheet.shape[2] % cols:
        raise ValueError(f"size = {rows} x {cols} does not divide the sheet {tuple(sheet.shape)}")
    H, W = sheet.shape[1] // rows, sheet.shape[2] // cols
    dev = sheet.device
    as_i32 = lambda t: _f(torch.as_tensor(t).to(device=dev, dtype=torch.int32))
    B = N = D = P = 0
    if boxes is not None:
        boxes = torch.as_tensor(boxes)
        if boxes.dim() != 4 or boxes.shape[2] != T or boxes.shape[3] != 4 or boxes.dtype.is_floating_point:
            raise ValueError(f"boxes must be integer [B, N, {T}, 4], got {boxes.dtype} {tuple(boxes.shape)}")
        B, N = boxes.shape[:2]
        if N > _lib.lib().c2m_draw_overlays_max_boxes():
            raise ValueError(f"boxes: N = {N} nodes per sample, the overlay kernel keeps at most "
                             f"{_lib.lib().c2m_draw_overlays_max_boxes()} (the cap of ops.instance_boxes)")
        presence = torch.ones(B, N, T, dtype=torch.bool) if presence is None else torch.as_tensor(presence)
        if tuple(presence.shape) != (B, N, T):
            raise ValueError(f"presence must be [B, N, T] = {(B, N, T)}, got {tuple(presence.shape)}")
        presence = _f((presence != 0).to(device=dev, dtype=torch.uint8))
        if box_colors is None:
            raise ValueError("box_colors [B, N, 3] uint8 is needed with boxes")
        box_colors = _u8_table("box_colors", box_colors, dev)
        if tuple(box_colors.shape) != (B, N, 3):
            raise ValueError(f"box_colors must be uint8 [B, N, 3] = {(B, N, 3)}, got {tuple(box_colors.shape)}")
        boxes = as_i32(boxes)
    if points is not None:
        points = torch.as_tensor(points)
        if points.dim() != 3 or points.shape[2] != 2 or points.dtype.is_floating_point:
            raise ValueError(f"points must be integer [D, P, 2], got {points.dtype} {tuple(points.shape)}")
        D, P = points.shape[:2]
        if point_sample is None or point_count is None or line_colors is None:
            raise ValueError("point_sample [D], point_count [D, T] and line_colors [D, 3] are needed with points")
        point_sample, point_count = torch.as_tensor(point_sample), torch.as_tensor(point_count)
        if tuple(point_sample.shape) != (D,) or tuple(point_count.shape) != (D, T):
            raise ValueError(f"point_sample must be [{D}] and point_count [{D}, {T}], got {tuple(point_sample.shape)} and "
                             f"{tuple(point_count.shape)}")
        line_colors = _u8_table("line_colors", line_colors, dev)
        if tuple(line_colors.shape) != (D, 3):
            raise ValueError(f"line_colors must be uint8 [D, 3] = {(D, 3)}, got {tuple(line_colors.shape)}")
        if D and (int(point_sample.min()) < 0 or int(point_sample.max()) >= rows * cols):
            raise ValueError(f"point_sample holds a sample outside the {rows} x {cols} cells")
        B = max(B, int(point_sample.max()) + 1) if D else B
        points, point_sample, point_count = as_i32(points), as_i32(point_sample), as_i32(point_count)
    if B > rows * cols:
        raise ValueError(f"boxes: B = {B} samples do not fit size = {rows} x {cols} cells")
    if B * T >= 65536:
        raise ValueError(f"sheet: B * T = {B * T} cells, the overlay launch takes fewer than 65536")
    if boxes is not None and boxes.shape[0] < B:            # paths of samples past the boxes' batch: pad with absent boxes
        pad = B - boxes.shape[0]
        boxes = torch.cat([boxes, boxes.new_zeros(pad, N, T, 4)])
        presence = torch.cat([presence, presence.new_zeros(pad, N, T)])
        box_colors = torch.cat([box_colors, box_colors.new_zeros(pad, N, 3)])
    if sheet.numel() and B and (N or D * P):
        with torch.no_grad():
            _lib.check(_lib.lib().c2m_draw_overlays(_p(sheet), B, T, H, W, rows, cols, _p(boxes) if N else None,
                                                    _p(presence) if N else None, _p(box_colors) if N else None, N,
                                                    _p(points) if D * P else None, _p(point_sample) if D * P else None,
                                                    _p(point_count) if D * P else None, _p(line_colors) if D * P else None,
                                                    D if P else 0, P, _stream()), "draw_overlays")
    return sheet


# =============================================================================================== losses
class _L1MeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mask):
        _dev(a, b, mask)
        ctx.b_dtype = b.dtype
        a = _f(a)
        b = _as(b, a.dtype)
        assert a.shape == b.shape
        C, inner = 1, 1
        if mask is not None:
            mask = _as(mask, torch.float32)
            assert mask.shape[0] == a.shape[0] and mask.shape[1] == 1 and mask.shape[2:] == a.shape[2:]
            C, inner = a.shape[1], a[0, 0].numel()
        out = torch.empty((), device=a.device, dtype=torch.float32)
        ws = torch.empty(1024, device=a.device, dtype=torch.float64)
        _lib.check(_lib.lib().c2m_l1_mean_fwd(_p(a), _p(b), _p(mask), _p(out), a.numel(), C, inner, _p(ws), _dt(a), _stream()),
                   "l1_mean")
        ctx.cfg = (C, inner)
        ctx.save_for_backward(a, b, mask)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, mask = ctx.saved_tensors
        C, inner = ctx.cfg
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        g = _f(g.reshape(1).float())
        _lib.check(_lib.lib().c2m_l1_mean_bwd(_p(a), _p(b), _p(mask), _p(g), _p(ga), _p(gb), a.numel(), C, inner,
                                              _dt(a), _stream()), "l1_mean_bwd")
        if gb is not None and gb.dtype != ctx.b_dtype:
            gb = gb.to(ctx.b_dtype)
        return ga, gb, None


def l1_mean(a, b, mask=None):
    """F.l1_loss(a*mask, b*mask) with mask [B,1,...] broadcast over channels (L1MaskedLoss), or plain L1 mean."""
    return _L1MeanFn.apply(a, b, mask)


class _SsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        _dev(x, y)
        ctx.x_dtype = x.dtype
        x, y = _as(x, torch.float32), _as(y, torch.float32)
        N, C, H, W = x.shape
        out = torch.empty((), device=x.device, dtype=torch.float32)
        ws = torch.empty(1024, device=x.device, dtype=torch.float64)
        _lib.check(_lib.lib().c2m_ssim_fwd(_p(x), _p(y), _p(out), N * C, H, W, _p(ws), _stream()), "ssim")
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        N, C, H, W = x.shape
        gx = torch.empty_like(x)
        coef = torch.empty(N * C * (H - 2) * (W - 2) * 3, device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().c2m_ssim_bwd(_p(x), _p(y), _p(_f(g.reshape(1).float())), _p(gx), _p(coef), N * C, H, W,
                                           _stream()), "ssim_bwd")
        return gx if gx.dtype == ctx.x_dtype else gx.to(ctx.x_dtype), None


def ssim_loss(x, y):
    """SSIMLoss.ssim on [N,C,H,W] (x = generated, differentiable; y = target)."""
    return _SsimFn.apply(x, y)


def norm_apply_eval(x, mean, invstd, gamma, beta, act=None):
    """Inference-mode BatchNorm (+act): per-channel affine with given statistics. No autograd."""
    _dev(x, mean, invstd, gamma, beta)
    x = _f(x)
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    y = torch.empty_like(x)
    _lib.check(_lib.lib().c2m_norm_apply(_p(x), _p(_f(mean)), _p(_f(invstd)), _p(gamma), _p(beta), None, _p(y), None, N, C, S, 1,
                                         ACT[act], LRELU_SLOPE, _dt(x), _stream()), "norm_apply(eval)")
    return y


# ------------------------------------------------------------------ dataset resolution -> input_size (csrc/resize.hip)
# Per-axis tables, built in float64 exactly as the library that defines the result builds them, cached per (in, out, filter)
# and per device.  Pillow (src/libImaging/Resample.c precompute_coeffs / normalize_coeffs_8bpc, Geometry.c ImagingScaleAffine) for
# uint8 images and maps; torch's upsample_bilinear2d (align_corners=False) and its antialiased form for flow fields.
_RESIZE_FILTERS = {"bilinear": 1.0, "bicubic": 2.0}
_resize_tables = {}


def _resize_filter_value(name, x):
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _resize_coeffs(n_in, n_out, name):
    """precompute_coeffs: bounds [out,2] int32 (first, count) and normalised float64 coefficients [out,ks]."""
    scale = float(n_in) / n_out
    filterscale = max(scale, 1.0)
    support = _RESIZE_FILTERS[name] * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)            # (int): towards zero, as astype
    count = np.minimum((center + support + 0.5).astype(np.int64), n_in) - first
    x = np.arange(ks, dtype=np.int64)[None, :]
    w = _resize_filter_value(name, ((x + first[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(x < count[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                             # the running sum `ww += w`, in tap order
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    return np.ascontiguousarray(np.stack([first, count], 1).astype(np.int32)), k, ks


def _resize_bilinear_taps(n_in, n_out):
    """upsample_bilinear2d, align_corners=False: source = scale * (dst + 0.5) - 0.5 clamped at 0, the two neighbours."""
    scale = float(n_in) / n_out
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    lam = src - i0
    two = i0 + 1 <= n_in - 1
    bounds = np.stack([i0, np.where(two, 2, 1)], 1).astype(np.int32)
    k = np.stack([np.where(two, 1.0 - lam, 1.0), np.where(two, lam, 0.0)], 1)
    return np.ascontiguousarray(bounds), k, 2


def _resize_nearest_index(n_in, n_out):
    """ImagingScaleAffine: xo = 0.5 * a; index = (int)xo; xo += a, a running double sum; outside the image: -1."""
    a = float(n_in) / n_out
    xo = np.cumsum(np.concatenate([[0.5 * a], np.full(n_out - 1, a)]))
    idx = xo.astype(np.int64)
    return np.ascontiguousarray(np.where((xo < 0.0) | (idx >= n_in), -1, idx).astype(np.int32))


def resize_table(kind, n_in, n_out, device):
    """(host arrays, device tensors, ks) of one axis.  kind: 'bicubic' / 'bilinear' (Pillow 8-bit: bounds + int32 coefficients),
    'nearest' (index), 'flow' / 'flow_aa' (bounds + fp32 weights)."""
    key = (kind, int(n_in), int(n_out), torch.device(device))
    tab = _resize_tables.get(key)
    if tab is None:
        if kind in _RESIZE_FILTERS:
            bounds, k, ks = _resize_coeffs(n_in, n_out, kind)
            q = k * (1 << 22)
            host = (bounds, np.ascontiguousarray(np.where(k < 0, -0.5 + q, 0.5 + q).astype(np.int32)))
        elif kind == "nearest":
            host, ks = (_resize_nearest_index(n_in, n_out),), 1
        elif kind in ("flow", "flow_aa"):
            bounds, k, ks = _resize_coeffs(n_in, n_out, "bilinear") if kind == "flow_aa" else _resize_bilinear_taps(n_in, n_out)
            host = (bounds, np.ascontiguousarray(k.astype(np.float32)))
        else:
            raise ValueError(f"unknown resize table {kind!r}")
        tab = _resize_tables[key] = (host, tuple(torch.from_numpy(h).to(device) for h in host), ks)
    return tab


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def resize_u8(x, size, filter="bicubic"):
    """[N,Hin,Win,C] uint8 (C in {1, 3}), contiguous, on the device -> [N,h,w,C]: Pillow's Image.resize, bit for bit."""
    N, Hin, Win, C = x.shape
    h, w = size
    (bxh, _), (bx, kx), ksx = resize_table(filter, Win, w, x.device)
    (byh, _), (by, ky), ksy = resize_table(filter, Hin, h, x.device)
    out = torch.empty(N, h, w, C, device=x.device, dtype=torch.uint8)
    _lib.check(_lib.lib().c2m_resize_u8(_p(x), _p(out), N, Hin, Win, h, w, C, _hp(bxh), _p(bx), _p(kx), ksx, _hp(byh), _p(by),
                                        _p(ky), ksy, _stream()), "resize_u8")
    return out


def resize_nearest(x, size):
    """[N,Hin,Win] uint8 or int32, contiguous, on the device -> [N,h,w]: Pillow's Image.resize(NEAREST)."""
    N, Hin, Win = x.shape
    h, w = size
    (xh,), (xi,), _ = resize_table("nearest", Win, w, x.device)
    (yh,), (yi,), _ = resize_table("nearest", Hin, h, x.device)
    out = torch.empty(N, h, w, device=x.device, dtype=x.dtype)
    _lib.check(_lib.lib().c2m_resize_nearest(_p(x), _p(out), x.element_size(), N, Hin, Win, h, w, _hp(xh), _p(xi), _hp(yh),
                                             _p(yi), _stream()), "resize_nearest")
    return out


def resize_flow(x, size, antialias=False):
    """[N,Hin,Win,2] float32, contiguous, on the device -> [N,h,w,2]: triangle filter, then * h / Hin on both channels."""
    N, Hin, Win, _ = x.shape
    h, w = size
    kind = "flow_aa" if antialias else "flow"
    (bxh, _), (bx, kx), ksx = resize_table(kind, Win, w, x.device)
    (byh, _), (by, ky), ksy = resize_table(kind, Hin, h, x.device)
    out = torch.empty(N, h, w, 2, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().c2m_resize_flow(_p(x), _p(out), N, Hin, Win, h, w, _hp(bxh), _p(bx), _p(kx), ksx, _hp(byh), _p(by),
                                          _p(ky), ksy, _stream()), "resize_flow")
    return out


# ========================================================================================== detector metric (csrc/detect.hip)
DETECT_SIZE = 416
_DET_MAX_HEADS, _DET_MAX_ANCHORS = 4, 8


def _det_check(name, t, dtype, dim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    _hip_only(t, name=name, where=True)
    _on_current_device(t, name=name)
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"{name} must have {dim} dimensions, got {tuple(t.shape)}")


def detect_scale(width):
    """The reference's rule (utils_yolov3.py:69): frames 256 or 320 wide go in as they are, every other width doubled."""
    return 1 if width in (256, 320) else 2


def detect_input(frames, size=DETECT_SIZE):
    """frames [B,C,H,W] fp32, or a video [B,C,T,H,W] whose LAST time index is read through its strides (no copy) ->
    ([B,C,size,size], scale, (h, w)): nearest x scale, zeros to the right and below -- and a crop where the scaled frame is
    larger than `size`, as F.pad with a negative pad does.  (h, w) is the scaled, unpadded frame size.  One launch."""
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
        raise ValueError("frames must be a [B,C,H,W] or [B,C,T,H,W] tensor")
    _det_check("frames", frames, torch.float32)
    v = frames.detach()
    if v.dim() == 5:
        if v.shape[2] < 1:
            raise ValueError("the video has no frame")
        v = v[:, :, -1]
    B, C, H, W = v.shape
    if min(C, H, W) < 1:
        raise ValueError(f"empty frame {tuple(v.shape)}")
    if any(s < 0 for s in v.stride()):
        v = v.contiguous()
    s = detect_scale(W)
    out = torch.empty(B, C, size, size, device=v.device, dtype=torch.float32)
    if B:
        _lib.check(_lib.lib().c2m_detect_input(_p(v), _p(out), B, C, H, W, v.stride(0), v.stride(1), v.stride(2), v.stride(3), s,
                                               size, _stream()), "detect_input")
    return out, s, (H * s, W * s)


def _yolo_plan(heads, anchors, num_classes, img_size):
    if not isinstance(heads, (list, tuple)) or not 1 <= len(heads) <= _DET_MAX_HEADS:
        raise ValueError(f"heads must be a list of 1..{_DET_MAX_HEADS} head maps")
    if len(anchors) != len(heads):
        raise ValueError(f"{len(heads)} heads but {len(anchors)} anchor sets")
    C = int(num_classes)
    if C < 1:
        raise ValueError("num_classes must be >= 1")
    N = None
    grid, na, boxes = [], [], 0
    for i, (h, a) in enumerate(zip(heads, anchors)):
        _det_check(f"heads[{i}]", h, torch.float32, 4)
        if not 1 <= len(a) <= _DET_MAX_ANCHORS or any(len(p) != 2 for p in a):
            raise ValueError(f"anchors[{i}] must be 1..{_DET_MAX_ANCHORS} (w, h) pairs")
        n, ch, gy, gx = h.shape
        if N is None:
            N = n
        if n != N or gy != gx or gy < 1 or ch != len(a) * (5 + C):
            raise ValueError(f"heads[{i}] must be [{N},{len(a) * (5 + C)},g,g] for {len(a)} anchors and {C} classes, "
                             f"got {tuple(h.shape)}")
        grid.append(gy)
        na.append(len(a))
        boxes += len(a) * gy * gy
    if img_size < 1:
        raise ValueError("img_size must be positive")
    return N, C, grid, na, boxes


def yolo_candidates(heads, anchors, num_classes, img_size, conf_thres=0.5):
    """YOLOLayer decode + confidence filter + class arg-max of every head of every image.  heads: raw maps [N, A*(5+C), g, g];
    anchors: per head a list of (w, h) in pixels; img_size: the side of the detector's input.  Returns cand [N,cap,7] =
    (x1, y1, x2, y2, conf, class_conf, class) compacted in box order (head, anchor, row, column), score [N,cap] = conf *
    class_conf with -inf in the unused slots, count [N] int32.  cap = every box: nothing is dropped."""
    N, C, grid, na, boxes = _yolo_plan(heads, anchors, num_classes, img_size)
    dev = heads[0].device
    cap = boxes
    cand = torch.zeros(N, cap, 7, device=dev, dtype=torch.float32)
    score = torch.full((N, cap), float("-inf"), device=dev, dtype=torch.float32)
    count = torch.zeros(N, device=dev, dtype=torch.int32)
    if N == 0:
        return cand, score, count
    hs = [_f(h.detach()) for h in heads]
    nh = len(hs)
    ptrs = (ctypes.c_void_p * nh)(*[h.data_ptr() for h in hs])
    stride = [img_size / g for g in grid]                                      # YOLOLayer.compute_grid_offsets: a Python float
    anc = np.zeros((nh, _DET_MAX_ANCHORS, 2), np.float32)
    for i, a in enumerate(anchors):
        for j, (w, h) in enumerate(a):
            anc[i, j] = (w / stride[i], h / stride[i])                         # FloatTensor([(a_w / stride, a_h / stride)])
    g_arr, na_arr = (ctypes.c_int * nh)(*grid), (ctypes.c_int * nh)(*na)
    st_arr = (ctypes.c_float * nh)(*stride)
    ws = torch.empty(N * _cdiv(boxes, 256), device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().c2m_yolo_candidates(ptrs, g_arr, na_arr, st_arr, _hp(anc), _DET_MAX_ANCHORS, nh, N, C,
                                              float(conf_thres), cap, _p(ws), _p(cand), _p(score), _p(count), _stream()),
               "yolo_candidates")
    return cand, score, count


def nms_merge(cand, score, count, nms_thres=0.4):
    """The reference's suppress-and-merge loop for every image in one launch.  Candidates are ordered by descending score with a
    STABLE sort (ties: lower box index first).  Returns dets [N,cap,7] (rows >= kept[n] are zero) and kept [N] int32."""
    _det_check("cand", cand, torch.float32, 3)
    _det_check("score", score, torch.float32, 2)
    _det_check("count", count, torch.int32, 1)
    N, cap, seven = cand.shape
    if seven != 7 or tuple(score.shape) != (N, cap) or tuple(count.shape) != (N,) or cap < 1:
        raise ValueError(f"need cand [N,cap,7], score [N,cap], count [N]; got {tuple(cand.shape)}, {tuple(score.shape)}, "
                         f"{tuple(count.shape)}")
    dets = torch.zeros(N, cap, 7, device=cand.device, dtype=torch.float32)
    kept = torch.zeros(N, device=cand.device, dtype=torch.int32)
    if N == 0:
        return dets, kept
    order = torch.sort(score, dim=1, descending=True, stable=True).indices
    srt = torch.gather(_f(cand), 1, order.unsqueeze(-1).expand(N, cap, 7))
    _lib.check(_lib.lib().c2m_nms_merge(_p(srt), _p(_f(count)), N, cap, float(nms_thres), _p(dets), _p(kept), _stream()),
               "nms_merge")
    return dets, kept


def match_detections(dets, kept, index, roi, x, batch, scale, size):
    """find_best_detection + the trajectory error for every clicked object in one launch.  dets [2B,cap,7] / kept [2B]: ground
    truth images first, predicted second; index [M] int64 node indices; roi [nodes,T,4], x [nodes,t_in,F] fp32 and batch [nodes]
    int64 from the graph; size = (h, w) of the scaled, unpadded frame.  Returns flags [M,3] int32 (skipped, gt_found,
    pred_found; skipped = -1 marks an index outside the graph), boxes [M,8] int32, err [M,2] float64."""
    _det_check("dets", dets, torch.float32, 3)
    _det_check("kept", kept, torch.int32, 1)
    _det_check("index", index, torch.int64, 1)
    _det_check("roi", roi, torch.float32, 3)
    _det_check("x", x, torch.float32, 3)
    _det_check("batch", batch, torch.int64, 1)
    N2, cap, seven = dets.shape
    nodes = batch.shape[0]
    if seven != 7 or N2 % 2 or N2 < 2 or kept.shape[0] != N2 or cap < 1:
        raise ValueError(f"need dets [2B,cap,7] and kept [2B], got {tuple(dets.shape)} and {tuple(kept.shape)}")
    if roi.shape[0] != nodes or roi.shape[2] != 4 or roi.shape[1] < 1:
        raise ValueError(f"roi must be [{nodes},T,4], got {tuple(roi.shape)}")
    if x.shape[0] != nodes or x.shape[1] < 1 or x.shape[2] < 2:
        raise ValueError(f"x must be [{nodes},t_in,F>=2], got {tuple(x.shape)}")
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or scale < 1:
        raise ValueError("size and scale must be positive")
    M = index.shape[0]
    dev = dets.device
    flags = torch.zeros(M, 3, device=dev, dtype=torch.int32)
    boxes = torch.zeros(M, 8, device=dev, dtype=torch.int32)
    err = torch.zeros(M, 2, device=dev, dtype=torch.float64)
    if M:
        roi, x = _f(roi.detach()), _f(x.detach())
        _lib.check(_lib.lib().c2m_match_detections(_p(_f(dets)), _p(_f(kept)), cap, N2 // 2, _p(_f(index)), M, _p(roi), roi.shape[1],
                                                   _p(x), x.shape[1], x.shape[2], _p(_f(batch)), nodes, int(scale), h, w,
                                                   0.005 * w * h, h * w * 0.01, _p(flags), _p(boxes), _p(err), _stream()),
                   "match_detections")
    return flags, boxes, err


# =============================================================================================== Panoptic-DeepLab post-processing
# (csrc/panoptic.hip; c2m_amd.segment is the public interface)
PANOPTIC_MAX_TOP_K = 1024       # c2m_panoptic_max_top_k(): the grouping kernel stages a frame's centres whole in LDS
_PanopticPlan = collections.namedtuple(
    "_PanopticPlan", "form N C H W things threshold nms_kernel top_k label_divisor stuff_area ignore_label")
_PANOPTIC_CLASSES = {}


def _panoptic_plan(semantic, center, offset, thing_list, label_divisor, stuff_area, ignore_label, threshold, nms_kernel, top_k):
    """Every check of panoptic_maps, made before anything is launched (host tensors pass: the device is the launch path's
    check).  semantic: fp32 logits [N,C,H,W] (form "logits") or uint8 / int64 labels [N,H,W] (form "labels")."""
    for name, t in (("semantic", semantic), ("center", center), ("offset", offset)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if semantic.dim() == 4 and semantic.dtype == torch.float32:
        form, (N, C, H, W) = "logits", semantic.shape
        if not 1 <= C <= 256:
            raise ValueError(f"semantic logits must have 1..256 classes (labels are uint8), got {C}")
    elif semantic.dim() == 3 and semantic.dtype in (torch.uint8, torch.int64):
        form, C, (N, H, W) = "labels", 256, semantic.shape
    else:
        raise ValueError("semantic must be fp32 logits [N,C,H,W] or uint8 / int64 labels [N,H,W], got "
                         f"{semantic.dtype} {tuple(semantic.shape)}")
    for name, t, ch in (("center", center, 1), ("offset", offset, 2)):
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be fp32, got {t.dtype}")
        if tuple(t.shape) != (N, ch, H, W):
            raise ValueError(f"{name} must be {(N, ch, H, W)} for semantic {tuple(semantic.shape)}, got {tuple(t.shape)}")
    for name, t in (("semantic", semantic), ("center", center), ("offset", offset)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device != semantic.device:
            raise ValueError(f"the heads must be on one device, got {semantic.device} and {t.device} ({name})")
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"a frame of {H}x{W} pixels is empty or too large (H * W must be below 2**31)")
    try:
        nms_kernel, top_k, label_divisor, stuff_area, ignore_label = (
            int(v) for v in (nms_kernel, top_k, label_divisor, stuff_area, ignore_label))
        threshold = float(threshold)
        things = tuple(sorted(set(int(c) for c in thing_list)))
    except (TypeError, ValueError):
        raise ValueError("nms_kernel, top_k, label_divisor, stuff_area, ignore_label must be integers, threshold a number and "
                         "thing_list a list of class ids") from None
    if not (1 <= nms_kernel <= 15 and nms_kernel % 2 == 1):
        raise ValueError(f"nms_kernel must be odd and in 1..15, got {nms_kernel}")
    if top_k is None or not 1 <= top_k <= PANOPTIC_MAX_TOP_K:
        raise ValueError(f"top_k is required and must be in 1..{PANOPTIC_MAX_TOP_K}, got {top_k}")
    if not threshold >= 0:                      # a candidate's score is then positive: the radix select orders by the float bits
        raise ValueError(f"threshold must be >= 0, got {threshold}")
    hi = C - 1 if form == "logits" else 254
    if any(not 0 <= c <= min(hi, 254) for c in things):
        raise ValueError(f"thing_list must lie in 0..{min(hi, 254)} for this input, got {list(thing_list)}")
    if label_divisor <= top_k:
        raise ValueError(f"label_divisor={label_divisor} must be above top_k={top_k}: the instance number must fit below it")
    if 256 * label_divisor >= 2 ** 31:
        raise ValueError(f"label_divisor={label_divisor} is too large: class * label_divisor must stay below 2**31")
    if not 0 <= ignore_label <= 255 or ignore_label in things:
        raise ValueError(f"ignore_label must be in 0..255 and no thing class, got {ignore_label}")
    return _PanopticPlan(form, N, C, H, W, things, threshold, nms_kernel, top_k, label_divisor, stuff_area, ignore_label)


def _panoptic_tables(things, device):
    """Device tables of a thing list: uint8 [256] (0: no thing, else 1 + position) and int32 [len] (the classes, ascending)."""
    key = (things, device.index)
    if key not in _PANOPTIC_CLASSES:
        _PANOPTIC_CLASSES[key] = torch.tensor(list(things) or [0], dtype=torch.int32, device=device)
    return _thing_table(things, device), _PANOPTIC_CLASSES[key]


def panoptic_maps(semantic, center, offset, thing_list, label_divisor, stuff_area, ignore_label, threshold, nms_kernel, top_k):
    """Panoptic-DeepLab's post-processing for N frames in one call (csrc/panoptic.hip; the contract is in include/c2m_hip.h and
    DESIGN.md 4.2i).  semantic: fp32 logits [N,C,H,W] or uint8 / int64 labels [N,H,W] with values in 0..255; center [N,1,H,W],
    offset [N,2,H,W] (dy, dx) fp32.  Returns device tensors: semantic uint8, instance int32, panoptic int32 [N,H,W], centers
    int32 [N,top_k,2] (y, x; zero past the count) and center_count int32 [N].  Six launches on the current stream; nothing is read
    back and nothing synchronises."""
    _hip_only(semantic, center, offset)
    pl = _panoptic_plan(semantic, center, offset, thing_list, label_divisor, stuff_area, ignore_label, threshold, nms_kernel, top_k)
    _on_current_device(semantic, center, offset)
    L = _lib.lib()
    assert L.c2m_panoptic_max_top_k() == PANOPTIC_MAX_TOP_K
    dev = semantic.device
    semantic, center, offset = semantic.detach(), center.detach(), offset.detach()
    logits = semantic if pl.form == "logits" else None
    labels = None if pl.form == "logits" else (semantic if semantic.dtype == torch.uint8 else semantic.to(torch.uint8))
    table, classes = _panoptic_tables(pl.things, dev)
    N, H, W = pl.N, pl.H, pl.W
    sem = torch.empty(N, H, W, device=dev, dtype=torch.uint8)
    ins = torch.empty(N, H, W, device=dev, dtype=torch.int32)
    pan = torch.empty(N, H, W, device=dev, dtype=torch.int32)
    centers = torch.empty(N, pl.top_k, 2, device=dev, dtype=torch.int32)
    count = torch.empty(N, device=dev, dtype=torch.int32)
    if N:
        nbytes = L.c2m_panoptic_workspace_bytes(N, H, W, pl.top_k, len(pl.things))
        if nbytes < 0:
            raise ValueError(f"panoptic_maps: sizes out of range (N={N}, {H}x{W}, top_k={pl.top_k})")
        work = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
        _lib.check(L.c2m_panoptic_maps(_p(logits), _p(labels), pl.C, _p(center), _p(offset), _p(table), _p(classes),
                                       len(pl.things), _p(sem), _p(ins), _p(pan), _p(centers), _p(count), _p(work), nbytes, N, H,
                                       W, pl.threshold, pl.nms_kernel, pl.top_k, pl.label_divisor, pl.stuff_area,
                                       pl.ignore_label, _stream()), "panoptic_maps")
    return {"semantic": sem, "instance": ins, "panoptic": pan, "centers": centers, "center_count": count}


# ------------------------------------------------------------------------------------------ scoring of label maps
# (csrc/map_quality.hip; c2m_amd.evaluate.map_quality is the public interface)
MAP_QUALITY_MAX_KEYS = 1 << 20      # num_classes * label_divisor: the per-image tables are addressed by class * divisor + n
MAP_QUALITY_MAX_PAIRS = 1 << 22
_MapQualityPlan = collections.namedtuple("_MapQualityPlan", "N H W u8 num_classes things label_divisor ignore_label max_pairs")


def _map_quality_plan(pred, gt, num_classes, thing_list, label_divisor, ignore_label, max_pairs):
    """Every check of map_quality, made before anything is launched (host tensors pass: the device is the launch path's
    check).  pred, gt: [N,H,W], both int32 or both uint8 -- no other dtype, so a negative value can only be an int32 the
    kernel reads as void."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype not in (torch.int32, torch.uint8):
            raise ValueError(f"{name} must be an int32 or uint8 label map, got {t.dtype}")
        if t.dim() != 3:
            raise ValueError(f"{name} must be [N,H,W], got {tuple(t.shape)}")
    if pred.dtype != gt.dtype:
        raise ValueError(f"pred and gt must have one dtype, got {pred.dtype} and {gt.dtype}")
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if pred.device != gt.device:
        raise ValueError(f"pred and gt must be on one device, got {pred.device} and {gt.device}")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError("pred and gt must be contiguous")
    N, H, W = pred.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31 or N >= 2 ** 24:
        raise ValueError(f"{N} frames of {H}x{W} pixels: a frame is empty or too large (H * W must be below 2**31)")
    try:
        num_classes, label_divisor, ignore_label, max_pairs = (int(v) for v in (num_classes, label_divisor, ignore_label, max_pairs))
        things = tuple(sorted(set(int(c) for c in thing_list)))
    except (TypeError, ValueError):
        raise ValueError("num_classes, label_divisor, ignore_label and max_pairs must be integers and thing_list a list of "
                         "class ids") from None
    if not 1 <= num_classes <= 255:
        raise ValueError(f"num_classes must be in 1..255, got {num_classes}")
    if label_divisor < 1 or num_classes * label_divisor > MAP_QUALITY_MAX_KEYS:
        raise ValueError(f"label_divisor={label_divisor} is out of range: it must be at least 1 and num_classes * label_divisor "
                         f"at most {MAP_QUALITY_MAX_KEYS}")
    if max_pairs < 1 or max_pairs > MAP_QUALITY_MAX_PAIRS or max_pairs & (max_pairs - 1):
        raise ValueError(f"max_pairs must be a power of two in 1..{MAP_QUALITY_MAX_PAIRS}, got {max_pairs}")
    if ignore_label < 0 or ignore_label >= 2 ** 31:
        raise ValueError(f"ignore_label must be in 0..2**31-1, got {ignore_label}")
    if any(not 0 <= c < num_classes for c in things) or ignore_label in things:
        raise ValueError(f"thing_list must lie in 0..{num_classes - 1} and leave out ignore_label, got {list(thing_list)}")
    return _MapQualityPlan(N, H, W, pred.dtype == torch.uint8, num_classes, things, label_divisor, ignore_label, max_pairs)


def map_quality(pred, gt, num_classes, thing_list, label_divisor, ignore_label, max_pairs):
    """Panoptic-quality counts and the confusion matrix of N predicted label maps against N ground-truth ones, per frame
    (csrc/map_quality.hip; the contract is in include/c2m_hip.h and DESIGN.md 4.2j).  pred, gt: int32 or uint8 [N,H,W].
    Returns device tensors: tp, fp, fn int32 [N,C], iou float64 [N,C], confusion int64 [N,C+1,C+1] ([pred, gt], void last),
    overflow bool [N].  A zero-fill and three launches on the current stream; nothing is read back and nothing synchronises."""
    pl = _map_quality_plan(pred, gt, num_classes, thing_list, label_divisor, ignore_label, max_pairs)
    _hip_only(pred, gt)
    _on_current_device(pred, gt)
    L = _lib.lib()
    dev, N, C = pred.device, pl.N, pl.num_classes
    pred, gt = pred.detach(), gt.detach()
    table, _ = _panoptic_tables(pl.things, dev)
    tp, fp, fn = (torch.zeros(N, C, device=dev, dtype=torch.int32) for _ in range(3))
    iou = torch.zeros(N, C, device=dev, dtype=torch.float64)
    conf = torch.zeros(N, C + 1, C + 1, device=dev, dtype=torch.int64)
    over = torch.zeros(N, device=dev, dtype=torch.uint8)
    if N:
        nbytes = L.c2m_map_quality_workspace_bytes(N, C, pl.label_divisor, pl.max_pairs)
        if nbytes < 0:
            raise ValueError(f"map_quality: sizes out of range (N={N}, num_classes={C}, label_divisor={pl.label_divisor}, "
                             f"max_pairs={pl.max_pairs})")
        work = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.int64)
        _lib.check(L.c2m_map_quality(_p(pred), _p(gt), int(pl.u8), _p(table), _p(tp), _p(fp), _p(fn), _p(iou), _p(conf),
                                     _p(over), _p(work), nbytes, N, pl.H, pl.W, C, pl.label_divisor, pl.ignore_label,
                                     pl.max_pairs, _stream()), "map_quality")
    return {"tp": tp, "fp": fp, "fn": fn, "iou": iou, "confusion": conf, "overflow": over.view(torch.bool)}


# ------------------------------------------------------------------------------------------ scoring of label maps over time
# (csrc/map_quality.hip; c2m_amd.evaluate.tube_quality is the public interface)
_TubeQualityPlan = collections.namedtuple("_TubeQualityPlan", "B T H W windows M mq")


def _tube_quality_plan(pred, gt, windows, ids, num_classes, thing_list, label_divisor, ignore_label, max_pairs):
    """Every check of tube_quality, made before anything is launched (host tensors pass: the device is the launch path's
    check).  pred, gt: [B,T,H,W], both int32 or both uint8; windows: distinct ints in 1..T; ids: None or int32 [B,M]."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dim() != 4:
            raise ValueError(f"{name} must be [B,T,H,W], got {tuple(t.shape)}")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError("pred and gt must be contiguous")
    B, T, H, W = pred.shape
    if T < 1:
        raise ValueError(f"clips of {T} frames: a clip needs at least one frame")
    frames = lambda t: t.view(t.shape[0] * t.shape[1], t.shape[2], t.shape[3])
    mq = _map_quality_plan(frames(pred), frames(gt), num_classes, thing_list, label_divisor, ignore_label, max_pairs)
    try:
        ks = tuple(int(k) for k in windows)
        if any(isinstance(k, (bool, float)) for k in windows):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"windows must be a sequence of frame counts, got {windows!r}") from None
    if not ks:
        raise ValueError("windows is empty")
    for k in ks:
        if not 1 <= k <= T:
            raise ValueError(f"a window of {k} frames in clips of {T}: windows must lie in 1..{T}")
    if len(set(ks)) != len(ks):
        raise ValueError(f"windows holds a length twice: {list(ks)}")
    if T * H * W >= 2 ** 31:
        raise ValueError(f"clips of {T} frames of {H}x{W} pixels: a tube's pixel counts are int32 (T * H * W must be below 2**31)")
    M = 0
    if ids is not None:
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1:
            raise ValueError(f"ids must be an int32 tensor [B={B}, M >= 1], got "
                             f"{(ids.dtype, tuple(ids.shape)) if isinstance(ids, torch.Tensor) else type(ids).__name__}")
        M = int(ids.shape[1])
    return _TubeQualityPlan(B, T, H, W, ks, M, mq)


def tube_quality(pred, gt, windows, ids, num_classes, thing_list, label_divisor, ignore_label, max_pairs):
    """Video panoptic quality counts of B predicted clips against B ground-truth ones, per window of k consecutive frames, for
    every k of `windows` (csrc/map_quality.hip; the contract is in include/c2m_hip.h and DESIGN.md 4.2s).  pred, gt: int32 or
    uint8 [B,T,H,W]; ids: None or int32 [B,M] map values (negative: padding).  Returns {k: dict} of device tensors: tp, fp, fn
    int32 [B,T-k+1,C], iou float64 [B,T-k+1,C], overflow bool [B,T-k+1] and, with ids, id_iou float64 and id_gt_area,
    id_pred_area int32 [B,T-k+1,M].  The pixels are read once; everything runs on the current stream, nothing is read back."""
    pl = _tube_quality_plan(pred, gt, windows, ids, num_classes, thing_list, label_divisor, ignore_label, max_pairs)
    _hip_only(pred, gt, ids)
    _on_current_device(pred, gt, ids)
    L = _lib.lib()
    dev, B, T, C, M, mq = pred.device, pl.B, pl.T, pl.mq.num_classes, pl.M, pl.mq
    pred, gt = pred.detach(), gt.detach()
    ids = None if ids is None else _f(ids.detach())
    table, _ = _panoptic_tables(mq.things, dev)
    counts = [B * (T - k + 1) for k in pl.windows]
    total = sum(counts)
    tp, fp, fn = (torch.zeros(total, C, device=dev, dtype=torch.int32) for _ in range(3))
    iou = torch.zeros(total, C, device=dev, dtype=torch.float64)
    over = torch.zeros(total, device=dev, dtype=torch.uint8)
    id_iou = torch.full((total, M), -1.0, device=dev, dtype=torch.float64) if M else None
    id_ga, id_pa = (torch.zeros(total, M, device=dev, dtype=torch.int32) if M else None for _ in range(2))
    if B:
        nbytes = L.c2m_tube_quality_workspace_bytes(B, T, C, mq.label_divisor, mq.max_pairs)
        if nbytes < 0:
            raise ValueError(f"tube_quality: sizes out of range (B={B}, T={T}, num_classes={C}, label_divisor={mq.label_divisor}, "
                             f"max_pairs={mq.max_pairs})")
        work = torch.empty(nbytes // 8 + 1, device=dev, dtype=torch.int64)
        ks = (ctypes.c_int32 * len(pl.windows))(*pl.windows)
        _lib.check(L.c2m_tube_quality(_p(pred), _p(gt), int(mq.u8), _p(table), ks, len(pl.windows), _p(tp), _p(fp), _p(fn), _p(iou),
                                      _p(over), _p(ids), M, _p(id_iou), _p(id_ga), _p(id_pa), _p(work), nbytes, B, T, pl.H, pl.W, C,
                                      mq.label_divisor, mq.ignore_label, mq.max_pairs, _stream()), "tube_quality")
    out, off = {}, 0
    for k, n in zip(pl.windows, counts):
        lead = (B, T - k + 1)
        r = {"tp": tp[off:off + n].view(*lead, C), "fp": fp[off:off + n].view(*lead, C), "fn": fn[off:off + n].view(*lead, C),
             "iou": iou[off:off + n].view(*lead, C), "overflow": over[off:off + n].view(torch.bool).view(*lead)}
        if M:
            r.update(id_iou=id_iou[off:off + n].view(*lead, M), id_gt_area=id_ga[off:off + n].view(*lead, M),
                     id_pred_area=id_pa[off:off + n].view(*lead, M))
        out[k] = r
        off += n
    return out


# =============================================================================================== connected components, instances
# (csrc/components.hip; c2m_amd.segment.semantic_instances is the public interface of the second)
COMPONENTS_TILE = (16, 64)          # c2m_components_tile_h/w(): the tile labelled in LDS; larger frames are merged across its seams
SEMANTIC_INSTANCES_MAX_THINGS = 32
_ComponentsPlan = collections.namedtuple("_ComponentsPlan", "N H W key_bytes stride_n stride_y connectivity")
_InstancesPlan = collections.namedtuple("_InstancesPlan", "N H W things label_divisor ignore_label connectivity min_area")
_THING_TABLES = {}


def _components_plan(keys, connectivity):
    """Every check of connected_components, made before anything is launched (host tensors pass: the device is the launch path's
    check).  keys: uint8 or int32 [N,H,W] whose rows are dense (stride 1 along x); the other two strides are free."""
    if not isinstance(keys, torch.Tensor):
        raise ValueError(f"keys must be a tensor, got {type(keys).__name__}")
    if keys.dtype not in (torch.uint8, torch.int32):
        raise ValueError(f"keys must be uint8 or int32, got {keys.dtype}")
    if keys.dim() != 3:
        raise ValueError(f"keys must be [N,H,W], got {tuple(keys.shape)}")
    N, H, W = keys.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31 or N * H * W >= 2 ** 31:
        raise ValueError(f"{N} images of {H}x{W} pixels: an image is empty or too large (H * W and N * H * W must be below 2**31)")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    sn, sy, sx = keys.stride()
    if (W > 1 and sx != 1) or (H > 1 and sy < 0) or (N > 1 and sn < 0):
        raise ValueError(f"keys must have dense rows (stride 1 along x) and no negative stride, got strides {keys.stride()}")
    return _ComponentsPlan(N, H, W, keys.element_size(), sn if N > 1 else 0, sy if H > 1 else W, int(connectivity))


def _components_workspace(workspace, nbytes, dev, what):
    """The int32 workspace of a call: a fresh block, or the caller's (tests hand in a poisoned one) if it is large enough."""
    if workspace is None:
        return torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
    if not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.int32 and workspace.is_contiguous()
            and workspace.device == dev and workspace.numel() * 4 >= nbytes):
        raise ValueError(f"{what}: workspace must be a contiguous int32 tensor of at least {nbytes} bytes on {dev}")
    return workspace


def connected_components(keys, connectivity=8, workspace=None):
    """Connected components of N key maps (csrc/components.hip; the contract is in include/c2m_hip.h and DESIGN.md 4.2o).
    keys: uint8 or int32 [N,H,W] on the device, a view with dense rows is fine.  Two pixels belong to one component when they are
    4- or 8-neighbours and carry the same key; there is no background.  Returns int32 [N,H,W]: at every pixel the index y * W + x
    of its component's first pixel in raster order (scipy.ndimage.label up to renumbering).  Three launches on the current stream
    whatever N is; nothing is read back and nothing synchronises; bit-repeatable; an image does not depend on the others."""
    pl = _components_plan(keys, connectivity)
    _hip_only(keys)
    _on_current_device(keys)
    L = _lib.lib()
    assert (L.c2m_components_tile_h(), L.c2m_components_tile_w()) == COMPONENTS_TILE
    keys = keys.detach()
    out = torch.empty(pl.N, pl.H, pl.W, device=keys.device, dtype=torch.int32)
    if pl.N:
        nbytes = L.c2m_components_workspace_bytes(pl.N, pl.H, pl.W)
        if nbytes < 0:
            raise ValueError(f"connected_components: sizes out of range (N={pl.N}, {pl.H}x{pl.W})")
        work = _components_workspace(workspace, nbytes, keys.device, "connected_components")
        _lib.check(L.c2m_connected_components(_p(keys), pl.key_bytes, pl.stride_n, pl.stride_y, _p(out), _p(work), nbytes, pl.N,
                                              pl.H, pl.W, pl.connectivity, _stream()), "connected_components")
    return out


def _instances_plan(labels, thing_list, label_divisor, ignore_label, connectivity, min_area):
    """Every check of semantic_instances, made before anything is launched (host tensors pass: the device is the launch path's
    check).  labels: uint8 or int64 [N,H,W] with values in 0..255."""
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"labels must be a tensor, got {type(labels).__name__}")
    if labels.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"labels must be uint8 or int64, got {labels.dtype}")
    if labels.dim() != 3:
        raise ValueError(f"labels must be [N,H,W], got {tuple(labels.shape)}")
    N, H, W = labels.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31 or N * H * W >= 2 ** 31:
        raise ValueError(f"{N} frames of {H}x{W} pixels: a frame is empty or too large (H * W and N * H * W must be below 2**31)")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    try:
        label_divisor, ignore_label, min_area = (int(v) for v in (label_divisor, ignore_label, min_area))
        things = tuple(int(c) for c in thing_list)
    except (TypeError, ValueError):
        raise ValueError("label_divisor, ignore_label and min_area must be integers and thing_list a list of class ids") from None
    if len(things) > SEMANTIC_INSTANCES_MAX_THINGS:
        raise ValueError(f"thing_list holds {len(things)} classes, at most {SEMANTIC_INSTANCES_MAX_THINGS} are supported")
    if len(set(things)) != len(things):
        raise ValueError(f"thing_list must hold distinct classes, got {list(things)}")
    if not 0 <= ignore_label <= 255:
        raise ValueError(f"ignore_label must be in 0..255, got {ignore_label}")
    if any(not 0 <= c <= 255 for c in things) or ignore_label in things:
        raise ValueError(f"thing_list must lie in 0..255 and leave out ignore_label={ignore_label}, got {list(things)}")
    if label_divisor < 1 or 256 * label_divisor >= 2 ** 31:
        raise ValueError(f"label_divisor={label_divisor} is out of range: class * label_divisor + n must stay below 2**31")
    if min_area < 1:
        raise ValueError(f"min_area must be at least 1, got {min_area}")
    return _InstancesPlan(N, H, W, things, label_divisor, ignore_label, int(connectivity), min_area)


def _thing_table(things, device):
    """Device uint8 [256] of a thing list in the order given: 0 for no thing, else 1 + the position in the list."""
    key = (things, device.index)
    if key not in _THING_TABLES:
        tab = np.zeros(256, np.uint8)
        for i, c in enumerate(things):
            tab[c] = i + 1
        _THING_TABLES[key] = torch.from_numpy(tab).to(device)
    return _THING_TABLES[key]


def semantic_instances(labels, thing_list, label_divisor, ignore_label, connectivity=8, min_area=1, workspace=None):
    """Instance ids of N label maps by connected components of the thing classes (csrc/components.hip; the contract is in
    include/c2m_hip.h and DESIGN.md 4.2o).  labels: uint8 or int64 [N,H,W] with values in 0..255.  Returns device tensors:
    instance int32 [N,H,W] (class * label_divisor + n on a kept thing component, n = 1, 2, ... per class and image by ascending
    first raster pixel; the label everywhere else), count and dropped int32 [N, len(thing_list)], components int32 [N,H,W].  A
    zero-fill and eight launches on the current stream; nothing is read back and nothing synchronises."""
    pl = _instances_plan(labels, thing_list, label_divisor, ignore_label, connectivity, min_area)
    _hip_only(labels)
    _on_current_device(labels)
    L = _lib.lib()
    dev, N, H, W, T = labels.device, pl.N, pl.H, pl.W, len(pl.things)
    labels = labels.detach()
    labels = _f(labels if labels.dtype == torch.uint8 else labels.to(torch.uint8))
    ins = torch.empty(N, H, W, device=dev, dtype=torch.int32)
    comp = torch.empty(N, H, W, device=dev, dtype=torch.int32)
    count = torch.empty(N, T, device=dev, dtype=torch.int32)
    dropped = torch.empty(N, T, device=dev, dtype=torch.int32)
    if N:
        nbytes = L.c2m_semantic_instances_workspace_bytes(N, H, W, T)
        if nbytes < 0:
            raise ValueError(f"semantic_instances: sizes out of range (N={N}, {H}x{W}, {T} thing classes)")
        work = _components_workspace(workspace, nbytes, dev, "semantic_instances")
        table = _thing_table(pl.things, dev)
        _lib.check(L.c2m_semantic_instances(_p(labels), _p(table), T, _p(ins), _p(comp), _p(count), _p(dropped), _p(work), nbytes,
                                            N, H, W, pl.connectivity, pl.min_area, pl.label_divisor, _stream()),
                   "semantic_instances")
    return {"instance": ins, "count": count, "dropped": dropped, "components": comp}
