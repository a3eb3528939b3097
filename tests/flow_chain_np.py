"""NumPy restatement of the flow chain (csrc/flow_chain.hip) in the dtype asked for (float64: the yardstick;
float32: the kernel's own precision and association order), the clip flows built on it with tests/dense_flow_np.py, the scenes
of the error table, and the inputs of the GPU tests (tests/test_gpu_flow_chain.py) with the tolerances that belong to them.

Flows are in pixels, channel 0 = x, a(x) ~ b(x + flow(x)).  Frames c_0 .. c_K; order "backward": steps[j] is the flow
c_{j+1} -> c_j and out[k] the flow c_{k+1} -> c_0; order "forward": steps[j] is c_j -> c_{j+1} and out[k] is c_0 -> c_{k+1}."""
import functools

import numpy as np

import dense_flow_np as NP

K_CAP = 16                      # the launcher's cap on the number of steps
EDGE_EPS = 1e-3                 # `valid` may differ where a float64 hop ends this close to the frame edge

# TOL_CHAIN is 16 x the largest difference between the float32 and the float64 run of chain() over the finite stage_cases()
# with uniform steps (+-3 px, and +-12 px where walks leave the frame), both orders; tests/test_flow_chain_cpu.py recomputes the
# gap and asserts that it is within a factor 2 of MEASURED_GAP.  The gap is NOT small: a field of independent uniform values
# has a slope of up to 6 px per px (24 in the "leave" case), every hop multiplies the distance between two walks by up to that
# slope, and after a handful of hops the float32 walk has left the float64 one altogether.  Measured per case, +-3 px steps:
# K = 1: 0 (exact), K = 3: 8.4e-6, K = 5: 9.4e-4, K = 16: 9.03 px; +-12 px steps at K = 5: 9.8e-2.  TOL_CHAIN, as defined,
# therefore bounds nothing at K = 16, and the tests do not rest on it:
#   - the GPU result is compared with the float32 restatement bit for bit (the kernel evaluates the same expressions in the
#     same order), and with float64 within 16 x the gap OF ITS OWN CASE (case_gap), which is at most TOL_CHAIN;
#   - the "smooth" stage cases (steps whose slope is below 0.7 px per px, like those of a real clip) keep a chain of 16 hops
#     comparable with float64: their gap is 1.7e-5 px;
#   - the end-to-end test uses TOL_CLIP = 16 x the gap of the chain on the float64 step flows of moving_boxes_clip() itself
#     (rounded to float32), measured 3.84e-5 px, in TOL_CHAIN's place.
MEASURED_GAP = 9.1
TOL_CHAIN = 16 * MEASURED_GAP
MEASURED_GAP_CLIP = 3.9e-5
TOL_CLIP = 16 * MEASURED_GAP_CLIP


# ------------------------------------------------------------------------------------------------ the algorithm
def _nan_to_zero(c):
    """What fl_sample's fmaxf(c, 0) does to a NaN coordinate before the clamp."""
    return np.where(np.isnan(c), c.dtype.type(0), c)


def gather_indices(px, py, H, W):
    """(x0, x1, y0, y1) that the sample at (px, py) reads, as dense_flow_np.sample forms them after the NaN rule."""
    dt = px.dtype.type
    fx, fy = np.clip(_nan_to_zero(px), dt(0), dt(W - 1)), np.clip(_nan_to_zero(py), dt(0), dt(H - 1))
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    return x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1)


def _walk(steps, js, dtype):
    """One walk over the steps js from every pixel: d = 0; per hop p = pixel + d, d += steps[j] sampled at p.  Yields after
    every hop (dx, dy, ok, (px, py), (ex, ey)): ok: every pixel + d so far inside the frame; p: where the hop read; e: pixel + d
    after it."""
    K, _, H, W = steps.shape
    dt = np.dtype(dtype).type
    xx = np.broadcast_to(np.arange(W).astype(dtype)[None, :], (H, W))
    yy = np.broadcast_to(np.arange(H).astype(dtype)[:, None], (H, W))
    dx, dy = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
    ok = np.ones((H, W), bool)
    for j in js:
        px, py = xx + dx, yy + dy
        sx, sy = _nan_to_zero(px), _nan_to_zero(py)
        dx, dy = dx + NP.sample(steps[j, 0], sx, sy), dy + NP.sample(steps[j, 1], sx, sy)
        ex, ey = xx + dx, yy + dy
        ok = ok & (ex >= dt(0)) & (ex <= dt(W - 1)) & (ey >= dt(0)) & (ey <= dt(H - 1))
        yield dx, dy, ok, (px, py), (ex, ey)


def chain(steps, order="backward", dtype=np.float64, details=False):
    """steps [K,2,H,W] -> (out [K,2,H,W], valid [K,H,W] bool).  details: also, per k, the list over the hops of the walk behind
    out[k] of ((px, py), (ex, ey)): where the hop read and where the pixel stood after it."""
    if order not in ("backward", "forward"):
        raise ValueError(f"order must be 'backward' or 'forward', got {order!r}")
    steps = np.asarray(steps).astype(dtype)
    K, two, H, W = steps.shape
    assert two == 2 and K >= 1
    out, valid, hops = np.zeros((K, 2, H, W), dtype), np.zeros((K, H, W), bool), [[] for _ in range(K)]
    if order == "forward":                                            # one walk, d written after every hop
        for k, (dx, dy, ok, p, e) in enumerate(_walk(steps, range(K), dtype)):
            out[k, 0], out[k, 1], valid[k] = dx, dy, ok
            for later in hops[k:]:
                later.append((p, e))
    else:                                                             # a walk of its own from every c_{k+1}
        for k in range(K):
            for dx, dy, ok, p, e in _walk(steps, range(k, -1, -1), dtype):
                hops[k].append((p, e))
            out[k, 0], out[k, 1], valid[k] = dx, dy, ok
    return (out, valid, hops) if details else (out, valid)


def undecided(steps, order, rounding=False):
    """[K,H,W] bool: the pixels whose `valid` may come out either way: a hop of the float64 walk ends within EDGE_EPS px of the
    frame edge (or is a NaN).  rounding: also within 16 x the distance between the float32 and the float64 walk at that hop
    (for the uniform steps at K = 16, where rounding moves a walk by pixels)."""
    K, _, H, W = np.asarray(steps).shape
    _, _, h64 = chain(steps, order, np.float64, details=True)
    h32 = chain(steps, order, np.float32, details=True)[2] if rounding else h64
    und = np.zeros((K, H, W), bool)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            for (_, (ex, ey)), (_, (fx, fy)) in zip(h64[k], h32[k]):
                edge = np.minimum(np.minimum(np.abs(ex), np.abs(ex - (W - 1))), np.minimum(np.abs(ey), np.abs(ey - (H - 1))))
                apart = np.maximum(np.abs(ex - fx), np.abs(ey - fy))
                und[k] |= ~(edge >= np.maximum(EDGE_EPS, 16 * apart))
    return und


def case_gap(steps, order):
    """The largest |float32 - float64| of chain() on steps [N,K,2,H,W], NaN results (which must coincide) left out."""
    gap = 0.0
    for s in steps:
        o64, o32 = chain(s, order)[0], chain(s, order, np.float32)[0]
        assert o32.dtype == np.float32 and np.array_equal(np.isnan(o64), np.isnan(o32))
        gap = max(gap, float(np.nanmax(np.abs(o64 - o32))))
    return gap


def clip_steps(video, first, K, value_range=(0, 1), dtype=np.float64, **kw):
    """(backward, forward) step flows [K,2,H,W] of the frames first .. first + K of video [3,T,H,W], by dense_flow_np."""
    fr = lambda t: video[:, t]
    bw = np.stack([NP.dense_flow(fr(first + j + 1), fr(first + j), value_range, dtype=dtype, **kw) for j in range(K)])
    fw = np.stack([NP.dense_flow(fr(first + j), fr(first + j + 1), value_range, dtype=dtype, **kw) for j in range(K)])
    return bw, fw


def clip_flows(video, t_in, t_out, value_range=(0, 1), dtype=np.float64, **kw):
    """The flows of c2m_amd.flow.clip_flows (no occlusion maps): input_of [2,t_in-1,H,W] or None, target_bw_of and target_fw_of
    [2,t_out,H,W], and the step flows they were chained from.  video [3,T,H,W]."""
    bw, fw = clip_steps(video, t_in - 1, t_out, value_range, dtype, **kw)
    inp = [NP.dense_flow(video[:, i], video[:, i + 1], value_range, dtype=dtype, **kw) for i in range(t_in - 1)]
    return {"input_of": np.stack(inp, 1) if inp else None, "steps_bw": bw, "steps_fw": fw,
            "target_bw_of": chain(bw, "backward", dtype)[0].transpose(1, 0, 2, 3),
            "target_fw_of": chain(fw, "forward", dtype)[0].transpose(1, 0, 2, 3)}


# ------------------------------------------------------------------------------------------------ the scenes of the error table
def shift_clip(H, W, per_frame, T=6, seed=0, margin=32):
    """video [3,T,H,W] on 0..1 of a 1/f texture under a global shift: the backward flow c_{t+1} -> c_t, which the targets of
    training are made of, is per_frame = (u, v) everywhere: c_{t+1}(x) = c_t(x + (u, v)), so c_g -> c_0 is g (u, v) and c_0 -> c_g
    is -g (u, v).  Cut from a texture `margin` px larger on every side, so nothing of the resampling's border reaches the frames."""
    big = NP.texture(H + 2 * margin, W + 2 * margin, seed)
    u, v = per_frame
    assert (T - 1) * max(abs(u), abs(v)) + 2 <= margin
    frames = [NP.resample(big, NP.motion_field(("shift", (t * u, t * v)), H + 2 * margin, W + 2 * margin))
              [:, margin:margin + H, margin:margin + W] for t in range(T)]
    return np.stack(frames, 1)


def shift_mask(H, W, flow):
    """dense_flow_np.pair's mask for a constant flow (u, v): >= 8 px from the border and the target inside the frame."""
    yy, xx = np.mgrid[0:H, 0:W]
    tx, ty = xx + flow[0], yy + flow[1]
    return (yy >= 8) & (yy < H - 8) & (xx >= 8) & (xx < W - 8) & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)


def constant_flow(H, W, flow):
    return np.stack([np.full((H, W), float(flow[0])), np.full((H, W), float(flow[1]))])


CLIP_T_IN, CLIP_OBJECT, CLIP_SPEED = 2, 11001, (3, 0)               # the end-to-end scene: moving_boxes_clip(), its first box


@functools.lru_cache(maxsize=None)
def boxes_reference():
    """(video, inst, float64 clip_flows of moving_boxes_clip() with t_in = 2, t_out = 5), computed once and left unchanged.  The
    frames go through the map of train.compute_flow first (v * 2 - 1 in float32, value range (-1, 1))."""
    video, inst = NP.moving_boxes_clip()
    ref = clip_flows(video * np.float32(2) - np.float32(1), CLIP_T_IN, video.shape[1] - CLIP_T_IN, value_range=(-1, 1))
    for v in ref.values():
        v.setflags(write=False)
    return video, inst, ref


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
STAGE_SHAPES = [(8, 8, 1, 1), (9, 13, 3, 1), (21, 37, 5, 1), (21, 37, 5, 3), (40, 70, K_CAP, 2)]      # H, W, K, N
LEAVE_SHAPE = (21, 37, 5, 3)
NAN_SHAPE = (21, 37, 5, 1)
SMOOTH_SHAPES = [(21, 37, 5, 3), (40, 70, K_CAP, 2)]
KIND_AMP = {"plain": 3.0, "leave": 12.0, "nan": 3.0, "smooth": 3.0}


def stage_cases():
    """(H, W, K, N, kind): "plain" +-3 px uniform steps at every stage shape; "leave" +-12 px uniform steps, whose walks exit
    the frame; "nan" +-3 px steps with one NaN entry; "smooth" +-3 px steps of slope < 0.5 px per px."""
    return [s + ("plain",) for s in STAGE_SHAPES] + [LEAVE_SHAPE + ("leave",), NAN_SHAPE + ("nan",)] + \
        [s + ("smooth",) for s in SMOOTH_SHAPES]


def chaotic(K, kind):
    """The cases whose float32 walk leaves the float64 one by pixels: independent uniform steps followed for 16 hops."""
    return kind != "smooth" and K == K_CAP


def stage_steps(H, W, K, N, kind="plain"):
    """Seeded step flows [N,K,2,H,W] float32: independent uniform values, or ("smooth") uniform values on a grid of 8-px cells,
    interpolated linearly: a slope of at most 2 * 3 / 8 px per px along an axis."""
    amp = KIND_AMP[kind]
    rng = np.random.default_rng(100000 * H + 1000 * W + 10 * K + N + sorted(KIND_AMP).index(kind))
    if kind == "smooth":
        from scipy.ndimage import zoom
        coarse = rng.uniform(-amp, amp, (N, K, 2, H // 8 + 2, W // 8 + 2))
        return np.ascontiguousarray(zoom(coarse, (1, 1, 1, 8, 8), order=1)[..., :H, :W]).astype(np.float32)
    steps = rng.uniform(-amp, amp, (N, K, 2, H, W)).astype(np.float32)
    if kind == "nan":
        steps[0, K // 2, 0, H // 2, W // 2] = np.nan
    return steps
