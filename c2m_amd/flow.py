"""Optical flow without a checkpoint: dense inverse search on the GPU (csrc/dense_flow.hip).

`dense_flow(a, b)` is the flow a -> b in pixels, channel 0 = x, with a(x) ~ b(x + flow(x)): the convention of
`ops.occlusion_splat`, of FlowNet2's output and of `train.compute_flow`, whose `target_bw_of` is the flow of (target frame ->
last input frame) and is read by `ops.label_warp` and `tracking.track_instances` as "pixel p came from p + flow(p)".
`ClassicFlow` has the call surface of `modules.third_party.flow_net.FlowNet` (4-, 5- and 6-D inputs, `compute_flow_and_conf`), so
it drops into `train.compute_flow`, into `tracking.tracked_batch`'s inputs and into `interactive.rollout(flow_fn=...)`.

The algorithm is a coarse-to-fine inverse search over 8 x 8 patches at stride 4 (one wave64 per patch), a fixed number of steps
per patch and a weighted average of the patches that cover a pixel.  `refine=True` adds a variational refinement of every level's
flow (csrc/flow_refine.hip; off by default).  A motion of more than about 8 px at the coarsest level (25 px at
128 x 256, four levels) is out of range of ONE search that starts at zero flow.  `seed=` starts the coarsest level's search
from the best of the integer displacements within a radius (4 by default, at most 8) of every patch, found by block matching
(`patch_match`; DESIGN.md 4.2q, with the measured limits; off by default): fast motion between two consecutive frames.
Frames of a clip that are further apart get their flow from the flows between consecutive frames, chained (`chain_flows`,
`clip_flows`, `ClassicFlow(chain=True)`; csrc/flow_chain.hip).  `segments=` (the int32 instance ids of frame a)
keeps the motion of one id out of the estimate of another: patch sums, the average over patches and the refinement's
smoothness stop at id borders.  Nothing here has weights; nothing is differentiated.  There is no CPU path: a
tensor that is not on a HIP device raises.
"""
import torch
import torch.nn as nn

from . import _lib, ops

PATCH, STRIDE, MAX_LEVELS = 8, 4, 7
REFINE_DEFAULTS = dict(alpha=20., delta=5., gamma=10., outer=5, sor=5, omega=1.6)      # OpenCV's DIS defaults; images on 0..255
SOR_CAP = 5                                                   # the iterate kernel's tile has a halo of 2 * sor <= 10 pixels
CHAIN_CAP = 16                                                # the most steps one chain_flows call follows
SEED_RADIUS, SEED_CAP = 4, 8                                  # block matching at the coarsest level: default and largest radius


def pyramid_sizes(H, W, levels=None):
    """[(h, w)] of every level: level l + 1 is ((h + 1) // 2, (w + 1) // 2), added while min(h, w) // 2 >= 16, at most
    `levels` (and at most 7, what the pyramid kernel's tile holds)."""
    if levels is not None and int(levels) < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    sizes = [(int(H), int(W))]
    cap = MAX_LEVELS if levels is None else min(int(levels), MAX_LEVELS)
    while len(sizes) < cap and min(sizes[-1]) // 2 >= 16:
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def patch_origins(n):
    """Patch origins along an axis of n >= 8 pixels: 0, 4, 8, ... <= n - 8, plus n - 8 if that is not one of them."""
    if n < PATCH:
        raise ValueError(f"an axis of {n} pixels holds no {PATCH}-pixel patch")
    o = list(range(0, n - PATCH + 1, STRIDE))
    return o if o[-1] == n - PATCH else o + [n - PATCH]


def _pair(a, b):
    """The checks of an image pair, before the device is looked at: (N, H, W)."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"{name} must be a [N,3,H,W] tensor, got {list(getattr(t, 'shape', ()))}")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{name} must be fp32 or bf16, got {t.dtype}")
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError(f"a and b must have one shape and dtype, got {list(a.shape)} {a.dtype} and {list(b.shape)} {b.dtype}")
    N, _, H, W = a.shape
    if H < PATCH or W < PATCH:
        raise ValueError(f"dense_flow needs H, W >= {PATCH}, got {H} x {W}")
    if not (a.is_cuda and b.is_cuda):
        raise ValueError("dense_flow needs tensors on a HIP device (no CPU fallback by design)")
    ops._on_current_device(a, b)
    return N, H, W


def _level_images(ia, ib):
    if not all(isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.float32 for t in (ia, ib)) or ia.shape != ib.shape:
        raise ValueError("level images must be two fp32 [N,h,w] tensors of one shape")
    if ia.shape[1] < PATCH or ia.shape[2] < PATCH:
        raise ValueError(f"a level needs h, w >= {PATCH}, got {ia.shape[1]} x {ia.shape[2]}")
    ops._hip_only(ia, ib)
    ops._on_current_device(ia, ib)
    return ia.detach().contiguous(), ib.detach().contiguous()


def _segment_ids(segments, N, h, w, level, device):
    """The checks of a guide: int32 [N,H,W] on `device`, the ids of frame a at level 0, which a stage on level `level` with
    [N,h,w] images reads at (y << level, x << level).  None stays None."""
    if segments is None:
        return None
    level = int(level)
    if not isinstance(segments, torch.Tensor) or segments.dtype != torch.int32 or segments.dim() != 3 or segments.shape[0] != N:
        raise ValueError(f"segments must be an int32 [{N},H,W] tensor, got {getattr(segments, 'dtype', None)} "
                         f"{list(getattr(segments, 'shape', ()))}")
    if segments.device != device:
        raise ValueError(f"segments must be on the device of the images ({device}), got {segments.device}")
    H, W = segments.shape[1:]
    if not 0 <= level < MAX_LEVELS or ((h - 1) << level) >= H or ((w - 1) << level) >= W:
        raise ValueError(f"segments {[H, W]} is not the level-0 map of a level-{level} image of {[h, w]}")
    return segments.detach().contiguous()


def flow_pyramid(a, b, value_range=(0, 1), levels=None):
    """Gray pyramids of both frames of N pairs in one launch -> (workspace, sizes, images): `workspace` is the fp32 buffer of
    one dense_flow call (c2m_flow_workspace_bytes), sizes = pyramid_sizes, images[l] = (a_l, b_l), [N,h,w] views of it."""
    N, H, W = _pair(a, b)
    lo, hi = (float(v) for v in value_range)
    if not hi > lo:
        raise ValueError(f"value_range must be (lo, hi) with lo < hi, got {value_range}")
    sizes = pyramid_sizes(H, W, levels)
    L, n = _lib.lib(), len(sizes)
    nbytes = L.c2m_flow_workspace_bytes(N, H, W, n)
    if nbytes < 0:
        raise ValueError(f"dense_flow: sizes out of range (N={N}, H={H}, W={W}, levels={n})")
    work = torch.empty(nbytes // 4, device=a.device, dtype=torch.float32)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    _lib.check(L.c2m_flow_pyramid(ops._p(a), ops._p(b), int(a.dtype == torch.bfloat16), lo, hi, N, H, W, n, ops._p(work), nbytes,
                                  ops._stream()), "flow_pyramid")
    images = []
    for l, (h, w) in enumerate(sizes):
        o = L.c2m_flow_workspace_offset(N, H, W, n, 0, l)
        images.append((work[o:o + N * h * w].view(N, h, w), work[o + N * h * w:o + 2 * N * h * w].view(N, h, w)))
    return work, sizes, images


def patch_search(ia, ib, init=None, iters=12, out=None, segments=None, level=0):
    """Steps 1-6 for one level: ia, ib [N,h,w] fp32 -> records [N,npy,npx,3] = (u, v, mean(J) - mean(T)) per patch.  init: None
    (zero flow), the dense flow [N,2,h,w] of this level, or that of the coarser level [N,2,(h+1)//2,(w+1)//2], which is read as
    2 * init[y // 2, x // 2].  segments: int32 [N,H,W], the ids of frame a at level 0 (ia is level `level` of it): every patch
    sum runs over the pixels with the id of the patch centre, and the records are [N,npy,npx,4], the count n last."""
    ia, ib = _level_images(ia, ib)
    N, h, w = ia.shape
    segments = _segment_ids(segments, N, h, w, level, ia.device)
    shift = 0
    if init is not None:
        coarse = (N, 2, (h + 1) // 2, (w + 1) // 2)
        if not isinstance(init, torch.Tensor) or init.dtype != torch.float32 or tuple(init.shape) not in ((N, 2, h, w), coarse):
            raise ValueError(f"init must be fp32 {[N, 2, h, w]} or {list(coarse)}, got {list(getattr(init, 'shape', ()))}")
        ops._hip_only(init)
        shift = int(tuple(init.shape) != (N, 2, h, w))
        init = init.detach().contiguous()
    npy, npx = len(patch_origins(h)), len(patch_origins(w))
    rec = torch.empty(N, npy, npx, 3 if segments is None else 4, device=ia.device, dtype=torch.float32) if out is None else out
    if segments is not None:
        _lib.check(_lib.lib().c2m_flow_patch_search_guided(
            ops._p(ia), ops._p(ib), ia.numel(), ops._p(init), 0 if init is None else init.numel(), shift, ops._p(rec), rec.numel(),
            N, h, w, int(iters), ops._p(segments), segments.numel(), int(level), segments.shape[1], segments.shape[2],
            ops._stream()), "flow_patch_search_guided")
        return rec
    _lib.check(_lib.lib().c2m_flow_patch_search(ops._p(ia), ops._p(ib), ia.numel(), ops._p(init), 0 if init is None else init.numel(),
                                                shift, ops._p(rec), rec.numel(), N, h, w, int(iters), ops._stream()),
               "flow_patch_search")
    return rec


def patch_match(ia, ib, radius=SEED_RADIUS, out=None, segments=None, level=0):
    """The block-matching seed of one level: ia, ib [N,h,w] fp32 -> records [N,npy,npx,3] = (dx, dy, mean(J) -
    mean(T)) per patch, (dx, dy) the integer displacement in [-radius, radius]^2 (1 <= radius <= SEED_CAP) with the smallest
    (cost, dx^2 + dy^2, dy, dx) among those whose 8 x 8 window lies inside ib; `densify` takes them.  segments, level: as in
    patch_search, records [N,npy,npx,4].  ONE launch on the current stream."""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= SEED_CAP:
        raise ValueError(f"radius must be an int 1 .. {SEED_CAP}, got {radius!r}")
    ia, ib = _level_images(ia, ib)
    N, h, w = ia.shape
    segments = _segment_ids(segments, N, h, w, level, ia.device)
    npy, npx = len(patch_origins(h)), len(patch_origins(w))
    rec = torch.empty(N, npy, npx, 3 if segments is None else 4, device=ia.device, dtype=torch.float32) if out is None else out
    if segments is not None:
        _lib.check(_lib.lib().c2m_flow_patch_match_guided(
            ops._p(ia), ops._p(ib), ia.numel(), ops._p(rec), rec.numel(), N, h, w, radius, ops._p(segments), segments.numel(),
            int(level), segments.shape[1], segments.shape[2], ops._stream()), "flow_patch_match_guided")
        return rec
    _lib.check(_lib.lib().c2m_flow_patch_match(ops._p(ia), ops._p(ib), ia.numel(), ops._p(rec), rec.numel(), N, h, w, radius,
                                               ops._stream()), "flow_patch_match")
    return rec


def seed_radius(seed):
    """None / False -> None (no seed); True -> SEED_RADIUS; an int 1 .. SEED_CAP -> that radius; anything else raises."""
    if seed is None or seed is False:
        return None
    if seed is True:
        return SEED_RADIUS
    if not isinstance(seed, int) or not 1 <= seed <= SEED_CAP:
        raise ValueError(f"seed must be None, a bool or an int 1 .. {SEED_CAP} (the radius), got {seed!r}")
    return seed


def densify(ia, ib, records, shift=0, out_size=None, out=None, segments=None, level=0):
    """Step 7 for one level: the dense flow [N,2,h,w] from the patch records [N,npy,npx,3].  shift, out_size: write
    2**shift * flow[y >> shift, x >> shift] at out_size = (Ho, Wo) instead (a coarser level brought to level 0).  segments (as
    in patch_search, with its records [N,npy,npx,4]): a pixel is averaged over the patches whose centre has its id."""
    ia, ib = _level_images(ia, ib)
    N, h, w = ia.shape
    segments = _segment_ids(segments, N, h, w, level, ia.device)
    npy, npx, width = len(patch_origins(h)), len(patch_origins(w)), 3 if segments is None else 4
    if not isinstance(records, torch.Tensor) or records.dtype != torch.float32 or tuple(records.shape) != (N, npy, npx, width):
        raise ValueError(f"records must be fp32 {[N, npy, npx, width]}, got {list(getattr(records, 'shape', ()))}")
    ops._hip_only(records)
    records = records.detach().contiguous()
    Ho, Wo = (h, w) if out_size is None else (int(v) for v in out_size)
    flow = torch.empty(N, 2, Ho, Wo, device=ia.device, dtype=torch.float32) if out is None else out
    if segments is not None:
        _lib.check(_lib.lib().c2m_flow_densify_guided(
            ops._p(ia), ops._p(ib), ia.numel(), ops._p(records), records.numel(), ops._p(flow), flow.numel(), N, h, w, int(shift),
            Ho, Wo, ops._p(segments), segments.numel(), int(level), segments.shape[1], segments.shape[2], ops._stream()),
            "flow_densify_guided")
        return flow
    _lib.check(_lib.lib().c2m_flow_densify(ops._p(ia), ops._p(ib), ia.numel(), ops._p(records), records.numel(), ops._p(flow),
                                           flow.numel(), N, h, w, int(shift), Ho, Wo, ops._stream()), "flow_densify")
    return flow


def refine_params(refine):
    """None / False -> None (no refinement); True -> REFINE_DEFAULTS; a dict overrides them, an unknown key raises.  The values
    are checked here, on the host: outer >= 1, 1 <= sor <= SOR_CAP, 0 < omega < 2, alpha, delta, gamma > 0."""
    if refine is None or refine is False:
        return None
    p = dict(REFINE_DEFAULTS)
    if refine is not True:
        if not isinstance(refine, dict):
            raise ValueError(f"refine must be None, a bool or a dict of {sorted(p)}, got {type(refine).__name__}")
        unknown = sorted(set(refine) - set(p))
        if unknown:
            raise ValueError(f"refine: unknown parameters {unknown} (known: {sorted(p)})")
        p.update(refine)
    for k in ("alpha", "delta", "gamma"):
        p[k] = float(p[k])
        if not 0 < p[k] < float("inf"):
            raise ValueError(f"refine: {k} must be a positive weight, got {p[k]}")
    p["omega"], p["outer"], p["sor"] = float(p["omega"]), int(p["outer"]), int(p["sor"])
    if not 0 < p["omega"] < 2:
        raise ValueError(f"refine: omega must be in (0, 2), got {p['omega']}")
    if not 1 <= p["outer"] <= 1024:
        raise ValueError(f"refine: outer must be 1 .. 1024, got {p['outer']}")
    if not 1 <= p["sor"] <= SOR_CAP:
        raise ValueError(f"refine: sor must be 1 .. {SOR_CAP} (the halo of the iterate kernel's tile), got {p['sor']}")
    return p


def _refine_workspace(N, h, w, device):
    nbytes = _lib.lib().c2m_flow_refine_workspace_bytes(N, h, w)
    if nbytes < 0:
        raise ValueError(f"refine_flow: sizes out of range (N={N}, h={h}, w={w})")
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32)


def _level_inputs(ia, ib, flow):
    """The checks of a level's images and its dense flow [N,2,h,w]."""
    ia, ib = _level_images(ia, ib)
    N, h, w = ia.shape
    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or tuple(flow.shape) != (N, 2, h, w):
        raise ValueError(f"flow must be fp32 {[N, 2, h, w]}, got {list(getattr(flow, 'shape', ()))}")
    ops._hip_only(flow)
    return ia, ib, flow.detach().contiguous()


def refine_planes(ia, ib, flow, work=None):
    """The eight planes (Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz) [8,N,h,w] of one level (a view of the workspace), ONE launch."""
    ia, ib, flow = _level_inputs(ia, ib, flow)
    N, h, w = ia.shape
    work = _refine_workspace(N, h, w, ia.device) if work is None else work
    _lib.check(_lib.lib().c2m_flow_refine_prepare(ops._p(ia), ops._p(ib), ia.numel(), ops._p(flow), flow.numel(), ops._p(work),
                                                  work.numel() * 4, N, h, w, ops._stream()), "flow_refine_prepare")
    return work[:8 * N * h * w].view(8, N, h, w)


def _refine_level(ia, ib, flow, p, work, out, shift=0, segments=None, level=0):
    """prepare + p['outer'] iterate launches; flow [N,2,h,w] contiguous; the last iteration writes `out` [N,2,Ho,Wo].  segments
    (checked by the caller): the smoothness is cut at the id borders of level `level`."""
    N, h, w = ia.shape
    refine_planes(ia, ib, flow, work)
    L, nbytes = _lib.lib(), work.numel() * 4
    for k in range(p["outer"]):
        last = k == p["outer"] - 1
        if segments is not None:
            _lib.check(L.c2m_flow_refine_iterate_guided(
                ops._p(flow), flow.numel(), ops._p(work), nbytes, N, h, w, k, p["sor"], p["alpha"], p["delta"], p["gamma"],
                p["omega"], ops._p(out) if last else None, out.numel() if last else 0, int(shift), out.shape[2], out.shape[3],
                ops._p(segments), segments.numel(), int(level), segments.shape[1], segments.shape[2], ops._stream()),
                "flow_refine_iterate_guided")
            continue
        _lib.check(L.c2m_flow_refine_iterate(ops._p(flow), flow.numel(), ops._p(work), nbytes, N, h, w, k, p["sor"], p["alpha"],
                                             p["delta"], p["gamma"], p["omega"], ops._p(out) if last else None,
                                             out.numel() if last else 0, int(shift), out.shape[2], out.shape[3], ops._stream()),
                   "flow_refine_iterate")
    return out


def refine_flow(ia, ib, flow, alpha=20., delta=5., gamma=10., outer=5, sor=5, omega=1.6, out=None, segments=None, level=0):
    """Variational refinement of one level: ia, ib [N,h,w] fp32 gray on 0..255 and the level's dense flow
    [N,2,h,w] -> the refined flow [N,2,h,w].  `outer` fixed-point iterations of `sor` (<= SOR_CAP) red-black SOR sweeps with
    relaxation omega; alpha, delta, gamma weigh smoothness, brightness and gradient constancy.  1 + outer launches on the
    current stream, no synchronisation; bit-repeatable and independent of N.  segments: int32 [N,H,W], the ids of frame a at
    level 0 (ia is level `level` of it): no smoothness couples two ids."""
    p = refine_params(dict(alpha=alpha, delta=delta, gamma=gamma, outer=outer, sor=sor, omega=omega))
    ia, ib, flow = _level_inputs(ia, ib, flow)
    N, h, w = ia.shape
    segments = _segment_ids(segments, N, h, w, level, ia.device)
    if out is None:
        out = torch.empty_like(flow)
    elif out.data_ptr() == flow.data_ptr():
        raise ValueError("refine_flow: out must not be the input flow (a tile reads its neighbours' input)")
    return _refine_level(ia, ib, flow, p, _refine_workspace(N, h, w, ia.device), out, segments=segments, level=level)


def dense_flow(a, b, value_range=(0, 1), levels=None, finest=0, iters=12, refine=None, segments=None, seed=None):
    """Flow a -> b of N image pairs -> [N,2,H,W] fp32 pixels (channel 0 = x; a(x) ~ b(x + flow(x))).

    a, b [N,3,H,W] fp32 or bf16 on the device, H, W >= 8, values in value_range = (lo, hi).  levels: at most that many pyramid
    levels (by default levels are added while min(h, w) // 2 >= 16).  finest: the last level searched; its flow is brought to
    level 0 by 2 * f[y // 2, x // 2] per level.  iters: search steps per patch and level, the same for every patch.
    refine: None / False: the densified patch flow; True: the variational refinement of DESIGN.md 4.2m after the densify of
    every searched level, with REFINE_DEFAULTS; a dict overrides those (see refine_params).
    segments: None, or the int32 ids [N,H,W] of frame a (instance ids; any integer is an id): the patch sums, the average over
    patches and the refinement's smoothness stop at id borders, which keeps the motion edge of an object sharp (DESIGN.md 4.2p;
    the same number of launches).  One id everywhere gives the bits of segments=None.
    seed: None / False: the coarsest level's search starts at zero flow; True, or an int 1 .. SEED_CAP: from the densified
    result of `patch_match` with radius SEED_RADIUS (that radius), which brings a motion of up to the radius at the coarsest
    level (32 px at 128 x 256 with the default) into range; the 8 px of the search's reset then count from the seed (DESIGN.md
    4.2q has what it recovers and what it does not).
    1 + 2 * (levels - finest) launches on the current stream whatever N is (1 + (3 + outer) * (levels - finest) with refinement;
    two more with a seed), no synchronisation, no copy to the host; the result is bit-repeatable and that of a pair does not
    depend on the other pairs of the call.  No gradient flows through it."""
    rp, radius = refine_params(refine), seed_radius(seed)
    if segments is not None:
        N, H, W = _pair(a, b)
        segments = _segment_ids(segments, N, H, W, 0, a.device)
        if tuple(segments.shape) != (N, H, W):
            raise ValueError(f"segments must be an int32 {[N, H, W]} tensor, got {list(segments.shape)}")
    with torch.no_grad():
        work, sizes, images = flow_pyramid(a, b, value_range, levels)
        N, (H, W), n = a.shape[0], sizes[0], len(sizes)
        finest, iters = int(finest), int(iters)
        if not 0 <= finest < n:
            raise ValueError(f"finest must be a level of the pyramid (0 .. {n - 1}), got {finest}")
        if not 0 <= iters <= 1024:
            raise ValueError(f"iters must be 0 .. 1024, got {iters}")
        L = _lib.lib()
        rec0 = L.c2m_flow_workspace_offset(N, H, W, n, 3, 0)
        out = torch.empty(N, 2, H, W, device=a.device, dtype=torch.float32)
        flow = None
        guide = {}
        if segments is not None:                                      # records of 4 floats: a buffer of their own
            hf, wf = sizes[finest]
            grec = torch.empty(4 * N * len(patch_origins(hf)) * len(patch_origins(wf)), device=a.device)
        if rp is not None:                                            # the refinement's own buffers, sized for the finest level
            hf, wf = sizes[finest]
            rwork, patchflow = _refine_workspace(N, hf, wf, a.device), torch.empty(2 * N * hf * wf, device=a.device)
        for l in range(n - 1, finest - 1, -1):
            (h, w), (ia, ib) = sizes[l], images[l]
            npy, npx = len(patch_origins(h)), len(patch_origins(w))
            if segments is None:
                rec = work[rec0:rec0 + N * npy * npx * 3].view(N, npy, npx, 3)
            else:
                rec, guide = grec[:N * npy * npx * 4].view(N, npy, npx, 4), dict(segments=segments, level=l)
            if radius is not None and l == n - 1:                     # the seed: match, densify at this level, search from it
                o = L.c2m_flow_workspace_offset(N, H, W, n, 2, l)     # this level's flow slot; level 0 has none
                flow = work[o:o + 2 * N * h * w] if l else torch.empty(2 * N * h * w, device=a.device)
                flow = densify(ia, ib, patch_match(ia, ib, radius, out=rec, **guide), out=flow.view(N, 2, h, w), **guide)
            rec = patch_search(ia, ib, flow, iters, out=rec, **guide)
            if rp is not None:                                        # densify -> refine -> the place the plain flow would go to
                dense = densify(ia, ib, rec, out=patchflow[:2 * N * h * w].view(N, 2, h, w), **guide)
                if l == finest:
                    return _refine_level(ia, ib, dense, rp, rwork, out, shift=l, **guide)
                o = L.c2m_flow_workspace_offset(N, H, W, n, 2, l)
                flow = _refine_level(ia, ib, dense, rp, rwork, work[o:o + 2 * N * h * w].view(N, 2, h, w), **guide)
                continue
            if l == finest:
                return densify(ia, ib, rec, shift=l, out_size=(H, W), out=out, **guide)
            o = L.c2m_flow_workspace_offset(N, H, W, n, 2, l)
            flow = densify(ia, ib, rec, out=work[o:o + 2 * N * h * w].view(N, 2, h, w), **guide)


def chain_flows(steps, order="backward", return_valid=False):
    """The flows across 1 .. K frames of N clips from the K flows between consecutive frames: steps
    [N,K,2,H,W] fp32 on the device -> [N,K,2,H,W].  Frames c_0 .. c_K.  order "backward": steps[:, j] is the flow c_{j+1} -> c_j
    and out[:, k] the flow c_{k+1} -> c_0; "forward": steps[:, j] is c_j -> c_{j+1} and out[:, k] is c_0 -> c_{k+1}.  Every pixel
    is followed through the steps: its displacement d starts at 0 and each hop adds the step sampled at pixel + d (bilinear,
    the coordinate clamped to the frame for the read only).  out[:, 0] is steps[:, 0].  return_valid: also a uint8 [N,K,H,W],
    1 where pixel + d stayed inside the frame after every hop.  1 <= K <= CHAIN_CAP.  ONE launch on the current stream
    whatever N and K are, no synchronisation; bit-repeatable, and the result of a clip does not depend on the others."""
    if order not in ("backward", "forward"):
        raise ValueError(f"order must be 'backward' or 'forward', got {order!r}")
    if not isinstance(steps, torch.Tensor) or steps.dim() != 5 or steps.shape[2] != 2 or steps.dtype != torch.float32:
        raise ValueError(f"steps must be a fp32 [N,K,2,H,W] tensor, got {getattr(steps, 'dtype', None)} "
                         f"{list(getattr(steps, 'shape', ()))}")
    N, K, _, H, W = steps.shape
    if not 1 <= K <= CHAIN_CAP or H < 1 or W < 1:
        raise ValueError(f"chain_flows needs 1 <= K <= {CHAIN_CAP} and H, W >= 1, got K={K}, H={H}, W={W}")
    if steps.numel() >= 1 << 31:
        raise ValueError(f"chain_flows: N * K * 2 * H * W must be below 2^31, got {steps.numel()}")
    ops._hip_only(steps)
    ops._on_current_device(steps)
    with torch.no_grad():
        steps = steps.detach().contiguous()
        out = torch.empty_like(steps)
        valid = torch.empty(N, K, H, W, device=steps.device, dtype=torch.uint8) if return_valid else None
        _lib.check(_lib.lib().c2m_flow_chain(ops._p(steps), steps.numel(), ops._p(out), out.numel(), ops._p(valid),
                                             0 if valid is None else valid.numel(), N, K, H, W, int(order == "forward"),
                                             ops._stream()), "flow_chain")
    return (out, valid) if return_valid else out


def clip_flows(video, num_input_frames, num_predicted_frames, use_fw_of=False, value_range=(0, 1), segments=None, **dense_flow_kw):
    """The dict of train.compute_flow for video [B,3,T,H,W] (T >= t_in + t_out; values in value_range), with the flows between
    the last input frame and the predicted frames CHAINED through the frames in between instead of searched across up to t_out
    frames: `target_bw_of` [B,2,t_out,H,W] is the backward chain from the last input frame, `target_bw_occ` [B,1,t_out,H,W] is
    ops.occlusion_splat of the forward chain; with use_fw_of, `target_fw_of` is the forward chain and `target_fw_occ` the map of
    the backward one.  `input_of` / `input_occ` (None for t_in = 1) are the consecutive flows themselves, as compute_flow has
    them, and so is the first target frame.  ONE dense_flow call over the 2 (t_in - 1 + t_out) B consecutive pairs (both
    directions; dense_flow_kw: levels, finest, iters, refine, seed), two chain launches, the splats and the copies that bring the
    results into compute_flow's layout: a number of launches that does not depend on B.
    segments: the int32 ids [B,T,H,W] of every frame of the video: the pair (c_j -> c_j+1) is guided by the ids of frame j, the
    pair (c_j+1 -> c_j) by those of frame j + 1 (dense_flow's `segments`, still ONE call)."""
    t_in, t_out = int(num_input_frames), int(num_predicted_frames)
    if t_in < 1 or not 1 <= t_out <= CHAIN_CAP:
        raise ValueError(f"clip_flows needs num_input_frames >= 1 and 1 <= num_predicted_frames <= {CHAIN_CAP}, got {t_in}, {t_out}")
    if not isinstance(video, torch.Tensor) or video.dim() != 5 or video.shape[1] != 3 or video.shape[2] < t_in + t_out:
        raise ValueError(f"video must be a [B,3,T,H,W] tensor with T >= {t_in + t_out}, got {list(getattr(video, 'shape', ()))}")
    B, _, _, H, W = video.shape
    n, n_in = t_in + t_out - 1, t_in - 1                              # consecutive pairs of a clip; those between input frames
    if segments is not None:
        if not isinstance(segments, torch.Tensor) or segments.dtype != torch.int32 or segments.dim() != 4 or \
                segments.shape[0] != B or segments.shape[1] < n + 1 or tuple(segments.shape[2:]) != (H, W):
            raise ValueError(f"segments must be an int32 [B,T,H,W] tensor with the video's B, H, W and T >= {n + 1}, got "
                             f"{getattr(segments, 'dtype', None)} {list(getattr(segments, 'shape', ()))}")
        if segments.device != video.device:
            raise ValueError(f"segments must be on the device of the video ({video.device}), got {segments.device}")
    with torch.no_grad():
        frames = video.detach()[:, :, :n + 1].transpose(1, 2)         # [B,T,3,H,W]
        f0, f1 = frames[:, :-1].reshape(B * n, 3, H, W), frames[:, 1:].reshape(B * n, 3, H, W)
        if segments is not None:                                      # the ids of the first frame of every pair
            ids = segments.detach()[:, :n + 1]
            dense_flow_kw["segments"] = torch.cat([ids[:, :-1].reshape(B * n, H, W), ids[:, 1:].reshape(B * n, H, W)])
        flows = dense_flow(torch.cat([f0, f1]), torch.cat([f1, f0]), value_range, **dense_flow_kw).view(2, B, n, 2, H, W)
        fw, bw = flows[0], flows[1]                                   # [:, j]: c_j -> c_{j+1} and c_{j+1} -> c_j
        fw_chain, bw_chain = chain_flows(fw[:, n_in:], "forward"), chain_flows(bw[:, n_in:], "backward")
        layout = lambda f: f.transpose(1, 2).contiguous()             # [B,K,2,H,W] -> [B,2,K,H,W]
        out = {"input_of": layout(fw[:, :n_in]) if n_in else None,
               "input_occ": ops.occlusion_splat(layout(bw[:, :n_in]))[0] if n_in else None}
        fw_chain, bw_chain = layout(fw_chain), layout(bw_chain)
        out["target_bw_of"], out["target_bw_occ"] = bw_chain, ops.occlusion_splat(fw_chain)[0]
        if use_fw_of:
            out["target_fw_of"], out["target_fw_occ"] = fw_chain, ops.occlusion_splat(bw_chain)[0]
    return out


class ClassicFlow(nn.Module):
    """dense_flow behind FlowNet's call surface: `flow, conf = ClassicFlow()(A, B)` for 4-D [N,3,H,W], 5-D [b,n,3,H,W] and 6-D
    [b,t,n,3,H,W] inputs, with conf = ops.occlusion_splat(flow)[0] as FlowNet computes it.  value_range defaults to (-1, 1),
    where train.compute_flow puts the frames; ClassicFlow(value_range=(0, 1)).compute_flow_and_conf is the `flow_fn` of
    interactive.rollout.  refine, seed: as in dense_flow (None: off).  No weights, no resize to multiples of 64: any size >= 8.
    chain=True: train.compute_flow takes its targets from `clip_flows` (the consecutive flows of the clip, chained) instead of
    searching each (last input frame, predicted frame) pair directly; the call surface above is the same either way.
    segments: forward, compute_flow_and_conf and clip_flows take the int32 ids of the first frame of every pair (of every frame
    of the clip) and pass them to dense_flow; train.compute_flow(..., segments=) hands them over."""

    takes_segments = True                                             # train.compute_flow asks before it passes `segments`

    def __init__(self, value_range=(-1, 1), levels=None, finest=0, iters=12, refine=None, chain=False, seed=None):
        super().__init__()
        self.value_range, self.levels, self.finest, self.iters = tuple(value_range), levels, finest, iters
        refine_params(refine)                                         # a bad parameter raises here, not at the first call
        seed_radius(seed)
        self.refine, self.chain, self.seed = refine, bool(chain), seed

    def clip_flows(self, train_batch, train_params, segments=None):
        """train.compute_flow's dict for a batch, by `clip_flows`; the frames go to [-1, 1] first, as compute_flow puts them.
        segments: the int32 ids [B,T,H,W] of every frame."""
        return clip_flows(train_batch["video"] * 2 - 1, train_params["num_input_frames"], train_params["num_predicted_frames"],
                          train_params.get("use_fw_of", False), self.value_range, levels=self.levels, finest=self.finest,
                          iters=self.iters, refine=self.refine, seed=self.seed,
                          **({} if segments is None else dict(segments=segments)))

    def forward(self, input_A, input_B, segments=None):
        size = input_A.size()
        if len(size) not in (4, 5, 6):
            raise ValueError(f"ClassicFlow takes [N,3,H,W], [b,n,3,H,W] or [b,t,n,3,H,W], got {list(size)}")
        if segments is not None and (not isinstance(segments, torch.Tensor) or
                                     tuple(segments.shape) != tuple(size[:-3]) + tuple(size[-2:])):
            raise ValueError(f"segments must be an int32 {list(size[:-3]) + list(size[-2:])} tensor (the ids of input_A), got "
                             f"{list(getattr(segments, 'shape', ()))}")
        if len(size) == 4:
            return self.compute_flow_and_conf(input_A, input_B, segments)
        c, h, w = size[-3:]
        flow, conf = self.compute_flow_and_conf(input_A.contiguous().view(-1, c, h, w), input_B.contiguous().view(-1, c, h, w),
                                                None if segments is None else segments.contiguous().view(-1, h, w))
        return flow.view(*size[:-3], 2, h, w), conf.view(*size[:-3], 1, h, w)

    def compute_flow_and_conf(self, im1, im2, segments=None):
        flow = dense_flow(im1, im2, self.value_range, self.levels, self.finest, self.iters, self.refine, segments, self.seed)
        with torch.no_grad():
            conf = ops.occlusion_splat(flow)[0]
        return flow, conf
