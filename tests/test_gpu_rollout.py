"""Label propagation and rollouts on the GPU (run with -m gpu): ops.label_warp against exact constructions and against
torch's nearest grid_sample on the CPU, then propagate_maps / predicted_boxes / drag_error / continue_click_to_move /
rollout on the small model and the rectangle scene of test_gpu_click_to_move.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from c2m_amd import interactive as I
from c2m_amd import ops
from test_gpu_click_to_move import DRAGS, RECTS, T_OUT, drag_step, inputs, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(128, 256), (94, 176), (188, 352), (256, 512)]
IDS = np.array([0, 7, 999, 1000, 11001, 13001, 18999, 24000, 33001, -5, 2 ** 31 - 1, -2 ** 31])


# ------------------------------------------------------------------------------------------------ helpers
def planes(B, Cf, Ci, H, W, seed):
    """One-hot float planes [B,Cf,H,W] and int32 id planes [B,Ci,H,W] that change from pixel to pixel."""
    g = torch.Generator().manual_seed(seed)
    pf = F.one_hot(torch.randint(0, max(Cf, 1), (B, H, W), generator=g), max(Cf, 1)).permute(0, 3, 1, 2).float()[:, :Cf]
    pi = torch.from_numpy(IDS)[torch.randint(0, len(IDS), (B, Ci, H, W), generator=g)].to(torch.int32)
    return pf.contiguous(), pi.contiguous()


def coords64(flow):
    """The source position (ix, iy) of every output pixel in float64, after the border clamp: a linspace(-1, 1) grid plus
    flow / ((n - 1) / 2), un-normalised as grid_sample(align_corners=False) does.  flow [B,2,T,H,W]."""
    H, W = flow.shape[-2:]
    f = flow.double()
    gx = torch.linspace(-1, 1, W, dtype=torch.float64) + f[:, 0] / ((W - 1) / 2)
    gy = torch.linspace(-1, 1, H, dtype=torch.float64)[:, None] + f[:, 1] / ((H - 1) / 2)
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    return ix.clamp(0, W - 1), iy.clamp(0, H - 1)


def torch_nearest(flow, pl):
    """The restatement with public torch calls, fp32 on the CPU: flow [B,2,T,H,W], pl [B,C,H,W] float -> [B,C,T,H,W]."""
    B, _, T, H, W = flow.shape
    gx = torch.linspace(-1, 1, W)[None, None, None, :] + flow[:, 0] / ((W - 1) / 2)
    gy = torch.linspace(-1, 1, H)[None, None, :, None] + flow[:, 1] / ((H - 1) / 2)
    grid = torch.stack([gx, gy], -1)                                                  # [B,T,H,W,2]
    out = [F.grid_sample(pl, grid[:, t], mode="nearest", padding_mode="border", align_corners=False) for t in range(T)]
    return torch.stack(out, 2)


def constructed(B, T, H, W, seed):
    """Flows whose source position is an integer pixel (up to 20 px outside every border) plus an offset in [-0.4, 0.4]:
    (flow fp32 [B,2,T,H,W], sx, sy int64 [B,T,H,W] clamped into the frame).  The coordinate formula is inverted in float64."""
    g = torch.Generator().manual_seed(seed)
    sx = torch.randint(-20, W + 20, (B, T, H, W), generator=g)
    sy = torch.randint(-20, H + 20, (B, T, H, W), generator=g)
    sx[:, :, :, :4], sx[:, :, :, -4:] = -20, W + 19                                   # both extremes, in every row
    sy[:, :, :4], sy[:, :, -4:] = H + 19, -20
    off = torch.rand((2, B, T, H, W), generator=g, dtype=torch.float64) * 0.8 - 0.4
    ix, iy = sx + off[0], sy + off[1]
    gx = torch.linspace(-1, 1, W, dtype=torch.float64)
    gy = torch.linspace(-1, 1, H, dtype=torch.float64)[:, None]
    fx = ((2 * ix + 1) / W - 1 - gx) * ((W - 1) / 2)
    fy = ((2 * iy + 1) / H - 1 - gy) * ((H - 1) / 2)
    return torch.stack([fx, fy], 1).float(), sx.clamp(0, W - 1), sy.clamp(0, H - 1)


def gather(pl, sx, sy):
    """pl [B,C,H,W], sx / sy [B,T,H,W] -> [B,C,T,H,W]: the plain integer gather."""
    B, C, H, W = pl.shape
    idx = (sy * W + sx).reshape(B, 1, -1).expand(B, C, -1)
    return pl.reshape(B, C, H * W).gather(2, idx).reshape(B, C, *sx.shape[1:])


def run(flow, pf=None, pi=None, **kw):
    d = lambda t: None if t is None else t.to(DEV)
    of, oi = ops.label_warp(d(flow), d(pf), d(pi), **{k: d(v) if torch.is_tensor(v) else v for k, v in kw.items()})
    torch.cuda.synchronize()
    return (None if of is None else of.cpu()), (None if oi is None else oi.cpu())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("size", SIZES)
def test_zero_flow_is_the_identity(size):
    """Not trivial: under the reference's coordinate quirk a zero flow is not the identity of the bilinear warp; the offset
    x / (W - 1) - 0.5 stays inside (-0.5, 0.5] and its one tie, at the last column, is clamped."""
    H, W = size
    B, T = 2, 3
    pf, pi = planes(B, 20, 1, H, W, seed=H)
    pf[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -0.0, 1e-42])            # words are copied, not computed on
    of, oi = run(torch.zeros(B, 2, T, H, W), pf, pi)
    assert of.shape == (B, 20, T, H, W) and of.dtype == torch.float32
    assert oi.shape == (B, 1, T, H, W) and oi.dtype == torch.int32
    assert same_bits(of, pf.unsqueeze(2).expand(B, 20, T, H, W))
    assert torch.equal(oi, pi.unsqueeze(2).expand(B, 1, T, H, W))
    of4, oi4 = run(torch.zeros(B, 2, H, W), pf, pi)                                      # [B,2,H,W] is T = 1
    assert same_bits(of4, pf.unsqueeze(2)) and torch.equal(oi4, pi.unsqueeze(2))


@pytest.mark.parametrize("size", SIZES + [(33, 61)])
def test_constructed_sources_are_gathered_exactly(size):
    """No tolerance: the source is at least 0.1 px from a rounding tie, the formula's fp32 error is orders of magnitude
    below that.  61 columns: the one-pixel-per-thread form of the kernel."""
    H, W = size
    B, T = 2, 5
    flow, sx, sy = constructed(B, T, H, W, seed=W)
    pf, pi = planes(B, 20, 1, H, W, seed=W + 1)
    of, oi = run(flow, pf, pi)
    assert same_bits(of, gather(pf, sx, sy))
    assert torch.equal(oi, gather(pi, sx, sy))


@pytest.mark.parametrize("sigma", [2.0, 12.0])
@pytest.mark.parametrize("size", SIZES)
def test_random_flows_vs_torch_nearest_on_the_cpu(size, sigma):
    H, W = size
    B, T = 1, 3
    g = torch.Generator().manual_seed(int(H * 7 + sigma))
    flow = torch.randn(B, 2, T, H, W, generator=g) * sigma
    ids = torch.randint(0, 2 ** 20, (B, 3, H, W), generator=g, dtype=torch.int32)    # exact in fp32 for grid_sample
    want = torch_nearest(flow, ids.float()).to(torch.int32)
    of, oi = run(flow, ids.float(), ids)
    ix, iy = coords64(flow)
    tie = lambda v: ((v - torch.floor(v)) - 0.5).abs() <= 1e-3
    excluded = (tie(ix) | tie(iy)).unsqueeze(1)                                         # [B,1,T,H,W]
    share = excluded.float().mean().item()
    bad_i = ((oi != want) & ~excluded).sum().item()
    bad_f = ((of.to(torch.int32) != want) & ~excluded).sum().item()
    print(f"{H}x{W} sigma {sigma}: excluded share {share:.5f}, mismatches outside {bad_i} / {bad_f}, inside "
          f"{((oi != want) & excluded).sum().item()}")
    assert share < 0.01, share
    assert bad_i == 0 and bad_f == 0


def test_properties():
    H, W = 128, 256
    B, T = 2, 5
    g = torch.Generator().manual_seed(4)
    flow = torch.randn(B, 2, T, H, W, generator=g) * 6
    pf, pi = planes(B, 20, 1, H, W, seed=9)
    of, oi = run(flow, pf, pi)
    assert torch.equal(of.sum(1), torch.ones(B, T, H, W)) and ((of == 0) | (of == 1)).all()       # still one-hot
    again = run(flow, pf, pi)
    assert same_bits(of, again[0]) and torch.equal(oi, again[1])                                  # bit-repeatable
    # occ: integer outputs are fill_id exactly where occ < threshold; float planes are not touched
    occ = torch.rand(B, 1, T, H, W, generator=g)
    occ[0, 0, 0, 0, :4] = torch.tensor([0.5, float("nan"), 0.49999997, 0.0])
    ff, fi = run(flow, pf, pi, occ=occ, threshold=0.5, fill_id=-7)
    assert same_bits(ff, of)
    assert torch.equal(fi, torch.where(occ < 0.5, torch.full_like(oi, -7), oi))
    assert 0.3 < (fi == -7).float().mean() < 0.7
    # a strided 5-D flow (frame-batched view of a larger tensor) and its contiguous copy
    big = torch.randn(B, 2, T + 3, H, W, generator=g).to(DEV) * 6
    view = big[:, :, 2:2 + T]
    assert not view.is_contiguous()
    a = ops.label_warp(view, pf.to(DEV), pi.to(DEV))
    b = ops.label_warp(view.contiguous(), pf.to(DEV), pi.to(DEV))
    assert same_bits(a[0].cpu(), b[0].cpu()) and torch.equal(a[1], b[1])
    rows = torch.randn(B, 2, T, H, 2 * W, generator=g).to(DEV)[..., ::2]                # rows not dense: copied by the op
    c = ops.label_warp(rows, pf.to(DEV), pi.to(DEV))
    d = ops.label_warp(rows.contiguous(), pf.to(DEV), pi.to(DEV))
    assert same_bits(c[0].cpu(), d[0].cpu()) and torch.equal(c[1], d[1])
    # Cf = 0 or Ci = 0
    only_i = run(flow, None, pi)
    assert only_i[0] is None and torch.equal(only_i[1], oi)
    only_f = run(flow, pf, None)
    assert only_f[1] is None and same_bits(only_f[0], of)
    e = run(flow, pf[:, :0], pi)
    assert e[0].shape == (B, 0, T, H, W) and torch.equal(e[1], oi)
    e = run(flow, pf, pi[:, :0])
    assert e[1].shape == (B, 0, T, H, W) and same_bits(e[0], of)
    many = run(flow, pf[:, :3], pi.expand(B, 6, H, W).contiguous())
    assert all(torch.equal(many[1][:, c], oi[:, 0]) for c in range(6))


def test_arguments_are_checked_before_any_launch():
    H, W = 16, 32
    flow, pf, pi = torch.zeros(2, 2, 3, H, W), torch.zeros(2, 4, H, W), torch.zeros(2, 1, H, W, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.label_warp(flow, pf, pi)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.label_warp(flow.to(DEV), pf, pi.to(DEV))
    f, a, b = flow.to(DEV), pf.to(DEV), pi.to(DEV)
    bad = [dict(flow=f[:, :1]), dict(flow=f[0]), dict(flow=f.double()), dict(planes_f=a[:1]), dict(planes_f=a[..., :-1]),
           dict(planes_f=a.half()), dict(planes_i=b.long()), dict(planes_i=b[:, 0]), dict(planes_i=b.float()),
           dict(planes_f=None, planes_i=None), dict(occ=torch.zeros(2, 1, 3, H, W, device=DEV)),
           dict(occ=torch.zeros(2, 1, 2, H, W, device=DEV), threshold=0.5), dict(threshold=0.5),
           dict(occ=torch.zeros(2, 1, 3, H, W, device=DEV), threshold=0.5, fill_id=2 ** 31)]
    for kw in bad:
        args = dict(flow=f, planes_f=a, planes_i=b)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.label_warp(**args)


@pytest.mark.parametrize("size", [(128, 256), (94, 176)])
def test_same_coordinates_as_the_bilinear_warp(size):
    """A two-channel image of each pixel's own (x, y): flow_warp returns the clamped (ix, iy) it read, label_warp the pixel
    it picked.  On the constructed flows they differ by the 0.4 px offset plus fp32 slack at most -- one coordinate formula."""
    H, W = size
    B, T = 2, 5
    flow, sx, sy = constructed(B, T, H, W, seed=H + 3)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.stack([xs, ys], 0).expand(B, 2, H, W).contiguous().to(DEV)
    picked = ops.label_warp(flow.to(DEV), img)[0]                                      # [B,2,T,H,W]
    for t in range(T):
        read = ops.flow_warp(img, flow[:, :, t].contiguous().to(DEV))
        diff = (read - picked[:, :, t]).abs().amax(dim=(0, 2, 3)).tolist()
        print(f"{H}x{W} frame {t}: max |bilinear - nearest| = {diff}")
        assert max(diff) <= 0.41, (t, diff)
    assert torch.equal(picked[:, 0].cpu(), sx.float()) and torch.equal(picked[:, 1].cpu(), sy.float())


# ------------------------------------------------------------------------------------------------ session level
def _rect_mask(x0, y0, x1, y1, dx=0, dy=0):
    m = torch.zeros(128, 256, dtype=torch.bool)
    m[y0 + dy:y1 + dy, x0 + dx:x1 + dx] = True
    return m


def test_the_drag_moves_the_object_and_its_id():
    t_in = 2
    batch = inputs(1, t_in)
    model = small_model(t_in, use_gt_eval=True)
    torch.manual_seed(0)
    out = I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], DRAGS[:1],
                          batch["input_of"], batch["input_occ"])
    maps = I.propagate_maps(out, batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], t_in, flow="sparse_motion_bw")
    assert maps["bg_mask"].shape == (1, 11, T_OUT, 128, 256) and maps["fg_mask"].shape == (1, 9, T_OUT, 128, 256)
    assert maps["instance_mask"].shape == (1, 1, T_OUT, 128, 256) and maps["instance_mask"].dtype == torch.int32
    assert all(v.is_cuda for v in maps.values())
    inst = maps["instance_mask"][0, 0].cpu()
    binm = out["sparse_motion_bin"][0, 0].cpu()
    sx, sy = drag_step(DRAGS[0])
    ids_in, edges_in, count = ops.instance_boxes(batch["instance_mask"], t_in)
    assert ids_in[0, :3].tolist() == [11001, 13001, 18999] and int(count[0]) == 3
    ids, boxes, presence = I.predicted_boxes(maps, ids_in)
    assert presence[0, :3].all() and not presence[0, 3:].any() and not boxes[0, 3:].any()
    moved = next(r for r in RECTS[0] if r[0] == 13001)
    for t in range(T_OUT):
        inside = _rect_mask(*moved[1:], sx * (t + 1), sy * (t + 1)) & (binm[t] == 1)
        assert inside.sum() > 0 and (inst[t][inside] == 13001).all(), t             # the id moved with the support
        ys, xs = torch.nonzero(inside, as_tuple=True)
        bx = boxes[0, 1, t].tolist()
        assert bx[0] <= int(xs.min()) and bx[1] <= int(ys.min()) and bx[2] > int(xs.max()) and bx[3] > int(ys.max()), (t, bx)
        for n in (0, 2):                                                              # the others stay where they were
            assert torch.equal(boxes[0, n, t], edges_in[0, n, t_in - 1]), (n, t)
    # the one-hot channels went the same way as the ids
    sem = torch.cat([maps["bg_mask"], maps["fg_mask"]], 1)
    assert torch.equal(sem.sum(1), torch.ones_like(sem[:, 0]))
    # the same ids without being given them; padded with -1
    ids2, boxes2, presence2 = I.predicted_boxes(maps["instance_mask"])
    assert ids2[0].tolist() == [11001, 13001, 18999] and torch.equal(boxes2[0], boxes[0, :3])
    # drag_error on a hand-built, ghost-free map with the rectangle at the requested place: 0.0 in every frame
    clean = torch.full((1, 1, T_OUT, 128, 256), 7, dtype=torch.int32)
    for t in range(T_OUT):
        for r in RECTS[0]:
            dx, dy = (sx * (t + 1), sy * (t + 1)) if r[0] == 13001 else (0, 0)
            clean[0, 0, t][_rect_mask(*r[1:], dx, dy)] = r[0]
    _, cboxes, cpres = I.predicted_boxes(clean.to(DEV), ids_in)
    targets = I.drag_targets(DRAGS[:1], [(0, 1)], edges_in.numpy(), t_in, T_OUT)
    err = I.drag_error(targets, cboxes, cpres)
    assert err["distance"].tolist() == [[0.0] * T_OUT] and err["normalized"].tolist() == [0.0]
    assert abs(err["displacement"][0] - np.hypot(10, 5)) < 1e-12
    # on the propagated map the ghost keeps the box's near edge at the old place: the error is what that geometry gives
    got = I.drag_error(targets, boxes, presence)
    print("sparse-flow drag error per frame (ghost included):", got["distance"].tolist(), got["normalized"].tolist())
    assert np.isfinite(got["distance"]).all()


def _second_drags(maps, t_in, B):
    """A drag per sample on an object of the last t_in propagated frames, found on the host."""
    inst = maps["instance_mask"][:, :, -t_in:].contiguous()
    ids, _, count = ops.instance_boxes(inst, t_in)
    assert (count > 0).all(), f"precondition: every sample keeps an object after the first segment, got {count.tolist()}"
    drags = []
    for b in range(B):
        ys, xs = torch.nonzero(inst[b, 0, -1].cpu() == int(ids[b, 0]), as_tuple=True)
        x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
        drags.append(I.Drag(b, x, y, min(max(x + 10 - 20 * b, 0), 255), min(max(y + 5, 0), 127)))
    return drags


def _stub_flow(a, b):
    return (b - a)[:, :2] * 3.0, (a.mean(1, keepdim=True) > b.mean(1, keepdim=True)).float()


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("t_in", [1, 2])
def test_a_continuation_equals_the_hand_built_second_call(t_in):
    B = 2
    batch = inputs(B, t_in)
    model = small_model(t_in)
    zs = torch.randn(2, B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(11)
    out1 = I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], DRAGS,
                           batch["input_of"], batch["input_occ"], z_m=zs[0])
    maps = I.propagate_maps(out1, batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], t_in)
    drags2 = _second_drags(maps, t_in, B)
    flow_fn = _stub_flow if t_in > 1 else None
    if t_in > 1:
        with pytest.raises(ValueError, match="flow_fn"):
            I.continue_click_to_move(model, batch, out1, drags2, z_m=zs[1])
    torch.manual_seed(13)
    got, nxt = I.continue_click_to_move(model, batch, out1, drags2, flow_fn=flow_fn, z_m=zs[1])
    # by hand
    last = lambda x: x[:, :, -t_in:]
    video = last(out1["generated"])
    graph, click = I.graph_from_instances(last(maps["instance_mask"]), drags2, t_in, T_OUT)
    of = occ = None
    if t_in > 1:
        of = torch.stack([_stub_flow(video[:, :, i], video[:, :, i + 1])[0] for i in range(t_in - 1)], 2)
        occ = torch.stack([_stub_flow(video[:, :, i + 1], video[:, :, i])[1] for i in range(t_in - 1)], 2)
    torch.manual_seed(13)
    with torch.no_grad():
        want = model.inference(video, last(maps["bg_mask"]), last(maps["fg_mask"]), last(maps["instance_mask"]), of, occ,
                               I.graph_to(graph, DEV), click.to(DEV), zs[1].to(DEV))
    torch.cuda.synchronize()
    _same_outputs(got, want)
    assert torch.equal(nxt["video"], video) and torch.equal(nxt["instance_mask"], last(maps["instance_mask"]))
    assert got["generated"].shape == (B, 3, T_OUT, 128, 256) and torch.isfinite(got["generated"]).all()
    assert got["index_user_guidance"].numel() == B


def test_rollout_over_three_segments():
    B, t_in = 2, 1
    batch = inputs(B, t_in)
    model = small_model(t_in)
    zs = torch.randn(3, B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(8))
    args = [batch[k] for k in ("video", "bg_mask", "fg_mask", "instance_mask")]
    # step by step (the last segment's clicks are found on the way), then the same in one call
    torch.manual_seed(21)
    out1 = I.click_to_move(model, *args, DRAGS, z_m=zs[0])
    out2, in2 = I.continue_click_to_move(model, batch, out1, [], z_m=zs[1])
    maps2 = I.propagate_maps(out2, in2["bg_mask"], in2["fg_mask"], in2["instance_mask"], t_in)
    drags3 = _second_drags(maps2, t_in, B)
    out3, in3 = I.continue_click_to_move(model, in2, out2, drags3, z_m=zs[2])
    segments = [DRAGS, [], drags3]
    torch.manual_seed(21)
    r = I.rollout(model, *args, segments, z_m=zs)
    torch.cuda.synchronize()
    assert r["generated"].shape == (B, 3, 3 * T_OUT, 128, 256) and torch.isfinite(r["generated"]).all()
    assert r["bg_mask"].shape == (B, 11, 15, 128, 256) and r["fg_mask"].shape == (B, 9, 15, 128, 256)
    assert r["instance_mask"].shape == (B, 1, 15, 128, 256) and r["instance_mask"].dtype == torch.int32
    for k, o in enumerate((out1, out2, out3)):
        assert torch.equal(r["generated"][:, :, k * T_OUT:(k + 1) * T_OUT], o["generated"]), k
        _same_outputs(r["outputs"][k], o)
    assert torch.equal(r["instance_mask"][:, :, T_OUT:2 * T_OUT], maps2["instance_mask"])
    assert out2["index_user_guidance"].numel() == 0 and out3["index_user_guidance"].numel() == B
    # ids never change value: nothing but the ids of the first frame, every later frame
    first = set(batch["instance_mask"][:, :, t_in - 1].unique().tolist())
    assert set(r["instance_mask"].unique().tolist()) <= first
    sem = torch.cat([r["bg_mask"], r["fg_mask"]], 1)
    assert torch.equal(sem.sum(1), torch.ones_like(sem[:, 0]))
    # boxes and errors per segment
    assert len(r["boxes"]) == len(r["presence"]) == len(r["drag_errors"]) == 3
    for k in range(3):
        N = r["ids"][k].shape[1]
        assert r["boxes"][k].shape == (B, N, T_OUT, 4) and r["presence"][k].shape == (B, N, T_OUT)
        assert r["drag_errors"][k]["distance"].shape == (len(segments[k]), T_OUT)
    assert r["ids"][0][0, :3].tolist() == [11001, 13001, 18999] and r["ids"][0][1, :2].tolist() == [12005, 17002]
    # the same seeds again: the same bits
    torch.manual_seed(21)
    again = I.rollout(model, *args, segments, z_m=zs)
    assert torch.equal(again["generated"], r["generated"]) and torch.equal(again["instance_mask"], r["instance_mask"])
    assert all(torch.equal(a, b) for a, b in zip(again["boxes"], r["boxes"]))
    # a sample without objects ends the rollout with the "no object" error, naming segment and sample
    empty = batch["instance_mask"].clone()
    empty[1] = 7
    with pytest.raises(ValueError, match=r"segment 0: sample 1 has no object"):
        I.rollout(model, args[0], args[1], args[2], empty, [[DRAGS[0]], []], z_m=zs[:2])


def test_scale_factor_other_than_one_is_refused():
    t_in = 1
    batch = inputs(1, t_in)
    model = small_model(t_in)
    model.model_params["common_params"]["scale_factor"] = 0.5
    with pytest.raises(ValueError, match="scale_factor"):
        I.continue_click_to_move(model, batch, {}, [])
    with pytest.raises(ValueError, match="scale_factor"):
        I.rollout(model, batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], [[], []])
