"""The rendering kernels on the GPU (run with -m gpu): ops.render_frames / render_flow / render_instances / draw_overlays
and c2m_amd.visual against the numpy restatement and painters of tests/test_visual_cpu.py and the fixture captured from
the live reference, then `storyboard` on a two-segment rollout of the small model of test_gpu_click_to_move.py.

Bounds.  Frames, occlusion maps, instances and overlays: bit-equal.  Flows: every pixel within 1 level and at most 1e-5 of
the pixels different at all; both sides are float64 and only atan2 is not correctly rounded on both.  Each flow test
prints its share before it asserts."""
import numpy as np
import pytest
import torch

from c2m_amd import interactive as I
from c2m_amd import ops, visual
from test_gpu_click_to_move import DRAGS, T_OUT, inputs, small_model
from test_gpu_rollout import IDS
from test_visual_cpu import GOLDEN, np_flow_fixed, np_flow_sheet, np_frames, np_instances, np_overlays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(128, 256), (94, 176), (188, 352)]
GRIDS = {1: (1, 2), 5: (2, 3), 8: (3, 3)}                 # B -> grid with empty cells


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def frame_values(B, C, T, H, W, seed):
    """Every k / 255, values below 0 and above 1, NaN and infinities among uniform noise."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.3, 1.3, (B, C, T, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    flat[:256] = np.arange(256, dtype=np.float32) / np.float32(255)
    flat[256:262] = [np.nan, np.inf, -np.inf, -0.0, 1.0, 255.5 / 255]
    flat[-256:] = np.nextafter(np.arange(256, dtype=np.float32) / np.float32(255), np.float32(-1))
    return x


def flow_close(got, want, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    share = (d > 0).any(-1).mean()
    print(f"{what}: {int((d > 0).any(-1).sum())} of {d[..., 0].size} pixels differ (share {share:.3g}), max {d.max()} levels")
    assert got.shape == want.shape and got.dtype == np.uint8
    assert d.max() <= 1, what
    assert share <= 1e-5, what


# ------------------------------------------------------------------------------------------------ frames / occlusion
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("size", SIZES)
def test_frames_and_occlusion_maps_are_bit_equal(size, B, dtype):
    H, W = size
    T = 2
    for C, normalize in ((3, False), (3, True), (1, False)):
        x = torch.from_numpy(frame_values(B, C, T, H, W, seed=H + B + C))
        if normalize:
            x = x * 2 - 1
        x = x.to(dtype)
        keep = x.clone()
        xd = x.to(DEV)
        got = ops.render_frames(xd, GRIDS[B], normalize)
        assert got.dtype == torch.uint8 and got.shape == (T, GRIDS[B][0] * H, GRIDS[B][1] * W, C) and got.is_cuda
        want = np_frames(x.float().numpy(), GRIDS[B], normalize)
        assert np.array_equal(host(got), want), (C, normalize)
        assert torch.equal(xd.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           keep.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))       # input not modified
        assert torch.equal(ops.render_frames(xd, GRIDS[B], normalize), got)                              # the same bits again
    occ = visual.tensor2occ(xd, GRIDS[B])
    assert occ.shape == (T, GRIDS[B][0] * H, GRIDS[B][1] * W) and np.array_equal(host(occ), want[..., 0])


def test_odd_width_and_strided_input():
    x = torch.from_numpy(frame_values(3, 3, 2, 33, 61, seed=9))
    assert np.array_equal(host(ops.render_frames(x.to(DEV), (2, 2))), np_frames(x.numpy(), (2, 2)))
    big = torch.from_numpy(frame_values(3, 3, 4, 32, 64, seed=10)).to(DEV)
    view = big[:, :, 1:3]                                                        # not contiguous
    assert np.array_equal(host(ops.render_frames(view, (1, 3))), np_frames(view.cpu().numpy(), (1, 3)))
    f = torch.randn(2, 2, 1, 33, 61, generator=torch.Generator().manual_seed(0)) * 5
    flow_close(host(ops.render_flow(f.to(DEV), (1, 3))), np_flow_sheet(f.numpy(), (1, 3)), "sheet mode, 61 columns")
    flow_close(host(ops.render_flow(f.to(DEV), (1, 3), 3.0)), np_flow_fixed(f.numpy(), (1, 3)), "fixed scale, 61 columns")


def test_the_golden_fixture_of_the_live_reference():
    g = np.load(GOLDEN)
    size = [int(v) for v in g["size"]]
    d = lambda k: torch.from_numpy(g[k]).to(DEV)
    assert np.array_equal(host(visual.tensor2im(d("frames"), size=size)), g["im"])
    assert np.array_equal(host(visual.tensor2im(d("frames_pm"), normalize=True, size=size)), g["im_normalize"])
    assert np.array_equal(host(visual.tensor2occ(d("occ"), size=size)), g["occ_sheet"])
    assert np.array_equal(host(visual.tensor2im(d("frames").bfloat16(), size=size)),
                          np_frames(d("frames").bfloat16().float().cpu().numpy(), size))
    flow_close(host(visual.tensor2flow(d("flow"), size)), g["flow_sheet"], "tensor2flow vs the reference")
    fixed = host(visual.flow_color_map(d("flow")))                               # [T, H, B*W, 3]
    B, W = g["flow"].shape[0], g["flow"].shape[-1]
    want = np.concatenate([g["flow_fixed"][b] for b in range(B)], 2)
    flow_close(fixed, want, "flow_color_map vs the reference")
    # default grid [8, 4]
    assert visual.tensor2im(d("frames")).shape == (2, 8 * 16, 4 * 24, 3)


# ------------------------------------------------------------------------------------------------ flows
def flows(kind, B, T, H, W, seed):
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((B, 2, T, H, W)) * 5).astype(np.float32)
    if kind == "unknown":
        idx = rng.integers(0, f.size, 200)
        f.reshape(-1)[idx] = rng.choice(np.array([2e7, -5e8, np.inf, 1.5e7], np.float32), 200)
        f[0, 0, 0, 0, :8] = 1e7                                                   # not above the threshold: known, and the maximum
    elif kind == "zero":
        f[:, :, 0] = 0                                                            # frame 0: an all-zero sheet
    elif kind == "one_sample_max":
        f[B - 1, :, :, 5, 7] = 400.0                                              # the sheet's maximum sits in the last sample
        f[:, :, :, :4] *= 0.02                                                    # small radii
    return f


@pytest.mark.parametrize("kind", ["normal", "unknown", "zero", "one_sample_max"])
@pytest.mark.parametrize("size,B", [((128, 256), 8), ((94, 176), 5), ((188, 352), 1)])
def test_flows_in_both_modes(size, B, kind):
    H, W = size
    T = 3
    f = flows(kind, B, T, H, W, seed=H + B)
    fd = torch.from_numpy(f).to(DEV)
    got = ops.render_flow(fd, GRIDS[B])
    want = np_flow_sheet(f, GRIDS[B])
    flow_close(host(got), want, f"sheet mode {kind} {size} B={B}")
    if kind == "zero":
        assert (host(got)[0] == 0).all() and host(got)[1].max() > 0                # 0 / 0: black, frame 0 only
    if kind == "unknown":
        assert (host(got).reshape(-1, 3).max(1) == 0).sum() >= 100
    if kind == "one_sample_max" and B > 1:
        # per sheet, not per sample: rendering sample 0 alone normalises by another maximum
        alone = host(ops.render_flow(fd[:1], (1, 1)))
        assert not np.array_equal(alone[:, :, :, :], host(got)[:, :H, :W])
    fixed = ops.render_flow(fd, GRIDS[B], 3.0)
    flow_close(host(fixed), np_flow_fixed(f, GRIDS[B]), f"fixed scale {kind} {size} B={B}")
    assert torch.equal(ops.render_flow(fd, GRIDS[B]), got) and torch.equal(ops.render_flow(fd, GRIDS[B], 3.0), fixed)
    assert np.array_equal(fd.cpu().numpy().view(np.int32), f.view(np.int32))
    # bf16 flows are widened first
    fb = fd.bfloat16()
    flow_close(host(ops.render_flow(fb, GRIDS[B])), np_flow_sheet(fb.float().cpu().numpy(), GRIDS[B]), "sheet mode bf16")


def test_nan_flow_is_black_and_python_max_rule():
    f = flows("normal", 2, 2, 32, 64, seed=1)
    f[0, 0, 1, 3, 3] = np.nan
    got = host(ops.render_flow(torch.from_numpy(f).to(DEV), (1, 2)))
    flow_close(got, np_flow_sheet(f, (1, 2)), "sheet mode with a NaN")            # frame 1: maxrad = max(-1, nan) = -1
    assert (got[1, 3, 3] == 0).all()
    fixed = host(ops.render_flow(torch.from_numpy(f).to(DEV), (1, 2), 3.0))
    assert (fixed[1, 3, 3] == 0).all()


# ------------------------------------------------------------------------------------------------ instances / overlays
def id_maps(B, T, H, W, seed, block=8):
    rng = np.random.default_rng(seed)
    bh, bw = -(-H // block), -(-W // block)
    ids = IDS[rng.integers(0, len(IDS), (B, 1, T, bh, bw))]
    ids = np.repeat(np.repeat(ids, block, 3), block, 4)[..., :H, :W].copy()
    noise = rng.random(ids.shape) < 0.02
    ids[noise] = IDS[rng.integers(0, len(IDS), int(noise.sum()))]
    return ids.astype(np.int32)


@pytest.mark.parametrize("size,B", [((128, 256), 5), ((94, 176), 8), ((33, 61), 1)])
def test_instances_are_bit_equal(size, B):
    H, W = size
    T = 2
    ids = id_maps(B, T, H, W, seed=W)
    pal = visual.default_palette(7).numpy()
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (T, GRIDS[B][0] * H, GRIDS[B][1] * W, 3), dtype=np.uint8)
    idd, based = torch.from_numpy(ids).to(DEV), torch.from_numpy(base).to(DEV)
    for alpha in (0, 100, 256):
        got = ops.render_instances(idd, GRIDS[B], torch.from_numpy(pal), based, alpha=alpha)
        assert np.array_equal(host(got), np_instances(ids, GRIDS[B], pal, base, alpha=alpha)), alpha
    assert np.array_equal(host(based), base) and np.array_equal(host(idd), ids)
    black = ops.render_instances(idd, GRIDS[B], torch.from_numpy(pal), None, id_range=(0, 12000))
    assert np.array_equal(host(black), np_instances(ids, GRIDS[B], pal, None, id_range=(0, 12000)))
    assert torch.equal(ops.render_instances(idd, GRIDS[B], torch.from_numpy(pal), None, id_range=(0, 12000)), black)


def overlay_case(B, T, H, W, seed):
    rng = np.random.default_rng(seed)
    N = 9
    boxes = np.zeros((B, N, T, 4), np.int32)
    presence = np.ones((B, N, T), bool)
    fixed = [(0, 0, W, H), (-5, -7, 20, 30), (W - 10, H - 12, W + 9, H + 4), (W - 1, 0, W, H), (0, H - 1, W, H),
             (10, 10, 11, 11), (-30, 5, -2, 40), (W, 3, W + 20, 20)]             # touching / crossing every border, 1 pixel, outside
    for n, bx in enumerate(fixed):
        boxes[:, n] = bx
    boxes[:, 8] = (15, 8, 40, 35)                                                 # overlaps box 1: the later node wins
    boxes[:, 8, 1:] += np.arange(1, T)[:, None] * 3
    presence[:, 2, ::2] = False
    presence[B - 1, 0] = False
    colors = rng.integers(1, 256, (B, N, 3), dtype=np.uint8)
    octants = [(30, 0), (30, 11), (30, 30), (11, 30), (0, 30), (-11, 30), (-30, 30), (-30, 11), (-30, 0), (-30, -11), (-30, -30),
               (-11, -30), (0, -30), (11, -30), (30, -30), (30, -11)]
    D = len(octants) + 3
    P = 4
    points = np.zeros((D, P, 2), np.int32)
    count = np.full((D, T), 2, np.int32)
    for d, (dx, dy) in enumerate(octants):
        points[d, 0] = (W // 2, H // 2)
        points[d, 1] = (W // 2 + dx, H // 2 + dy)
    d = len(octants)
    points[d] = [(5, 5), (5, 5), (W + 15, 20), (-40, H + 9)]                      # repeated point, points outside the cell
    count[d] = np.minimum(np.arange(T) + 1, 6)                                   # 1 point (marker only) ... past P
    points[d + 1] = [(W - 1, H - 1), (0, 0), (0, 0), (0, 0)]                     # a single point in the corner: clipped marker
    count[d + 1] = 1
    points[d + 2] = [(3, H - 2), (W - 3, 2), (W // 3, H // 2), (W // 3, H // 2)]
    count[d + 2] = np.arange(T) % 5                                              # 0 shows nothing
    sample = (np.arange(D) % B).astype(np.int32)
    lines = rng.integers(1, 256, (D, 3), dtype=np.uint8)
    return boxes, presence, colors, points, sample, count, lines


@pytest.mark.parametrize("size,B", [((128, 256), 5), ((94, 176), 8), ((33, 61), 1)])
def test_overlays_are_bit_equal(size, B):
    H, W = size
    T = 5
    grid = GRIDS[B]
    rng = np.random.default_rng(H)
    sheet = rng.integers(0, 256, (T, grid[0] * H, grid[1] * W, 3), dtype=np.uint8)
    boxes, presence, colors, points, sample, count, lines = overlay_case(B, T, H, W, seed=B)
    want = np_overlays(sheet, grid, boxes, presence, colors, points, sample, count, lines)
    t = torch.from_numpy
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                                              # a non-default stream
        sd = t(sheet).to(DEV)
        got = ops.draw_overlays(sd, grid, t(boxes), t(presence), t(colors), t(points), t(sample), t(count), t(lines))
        assert got.data_ptr() == sd.data_ptr()                                   # in place
        f = ops.render_frames(torch.from_numpy(frame_values(B, 3, 1, H, W, seed=2)).to(DEV), grid)
        fl = ops.render_flow(torch.zeros(B, 2, 1, H, W, device=DEV), grid, 3.0)
    stream.synchronize()
    assert np.array_equal(host(got), want)
    assert np.array_equal(host(f), np_frames(frame_values(B, 3, 1, H, W, seed=2), grid)) and (host(fl) == 255).all()
    changed = (want != sheet).any(-1)
    assert changed.any()
    for b in range(B, grid[0] * grid[1]):                                        # nothing in a cell without a sample
        assert not changed[:, (b // grid[1]) * H:(b // grid[1] + 1) * H, (b % grid[1]) * W:(b % grid[1] + 1) * W].any()
    # boxes alone, paths alone, and the same bits twice
    only_b = ops.draw_overlays(t(sheet).to(DEV), grid, t(boxes), t(presence), t(colors))
    assert np.array_equal(host(only_b), np_overlays(sheet, grid, boxes, presence, colors))
    only_p = ops.draw_overlays(t(sheet).to(DEV), grid, points=t(points), point_sample=t(sample), point_count=t(count),
                               line_colors=t(lines))
    assert np.array_equal(host(only_p), np_overlays(sheet, grid, None, None, None, points, sample, count, lines))
    again = ops.draw_overlays(t(sheet).to(DEV), grid, t(boxes), t(presence), t(colors), t(points), t(sample), t(count), t(lines))
    assert torch.equal(again, got)
    with pytest.raises(ValueError, match="boxes: N = 65"):
        ops.draw_overlays(t(sheet).to(DEV), grid, torch.zeros(B, 65, T, 4, dtype=torch.int32), None, torch.zeros(B, 65, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ end to end
def test_storyboard_of_a_two_segment_rollout():
    B, t_in = 2, 1
    batch = inputs(B, t_in)
    model = small_model(t_in)
    zs = torch.randn(2, B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(8))
    args = [batch[k] for k in ("video", "bg_mask", "fg_mask", "instance_mask")]
    torch.manual_seed(21)
    r = I.rollout(model, *args, [DRAGS[:1], []], z_m=zs)                          # one drag, in sample 0, first segment only
    H, W = 128, 256
    board = visual.storyboard(r, batch["video"])
    assert board.shape == (2 * T_OUT, 4 * H, B * W, 3) and board.dtype == torch.uint8 and board.is_cuda
    plain = visual.storyboard(r, batch["video"], overlays=False)
    gen = visual.tensor2im(r["generated"], size=[1, B])
    assert torch.equal(plain[:, :H], gen)
    assert torch.equal(plain[:, 2 * H:3 * H], visual.tensor2flow(torch.cat([o["dense_motion_bw"] for o in r["outputs"]], 2), [1, B]))
    assert torch.equal(plain[:, 3 * H:, :, 0], visual.tensor2occ(torch.cat([o["occlusion_bw"] for o in r["outputs"]], 2), [1, B]))
    assert torch.equal(board[:, 2 * H:], plain[:, 2 * H:])                        # overlays only on the frame panels
    inst = ops.render_instances(r["instance_mask"], (1, B), visual.default_palette(), gen)
    assert torch.equal(plain[:, H:2 * H], inst)
    # the outline colour: at the corners of every present predicted box of the dragged object, nowhere in sample 1's cell
    tg = r["targets"][0][0]
    assert (tg.sample, len(r["targets"][1])) == (0, 0)
    red = (host(board) == np.array(visual.BOX_COLOR, np.uint8)).all(-1)           # [frames, 4H, B*W]
    seen = 0
    for t in range(T_OUT):
        if not bool(r["presence"][0][0, tg.node, t]):
            continue
        x0, y0, x1, y1 = (int(v) for v in r["boxes"][0][0, tg.node, t])
        for panel in (0, 1):
            for x, y in ((x0, y0), (x1 - 1, y0), (x0, y1 - 1), (x1 - 1, y1 - 1)):
                assert red[t, panel * H + y, x], (t, panel, x, y)
        seen += 1
    assert seen > 0
    plain_red = (host(plain) == np.array(visual.BOX_COLOR, np.uint8)).all(-1)
    assert not (red & ~plain_red)[:, :, W:].any()                                 # sample 1 has no drag: nothing drawn there
    assert not (red & ~plain_red)[T_OUT:].any()                                   # the second segment has no drag either
    assert torch.equal(board[T_OUT:], plain[T_OUT:])
    # a plain click_to_move result, a custom panel list, and the scale_factor refusal
    out = r["outputs"][0]
    single = visual.storyboard(out, panels=("generated", "occlusion_bw"))
    assert single.shape == (T_OUT, 2 * H, B * W, 3) and torch.equal(single[:, :H], gen[:T_OUT])
    with pytest.raises(ValueError, match="maps"):
        visual.storyboard(out)
    small = dict(out, dense_motion_bw=out["dense_motion_bw"][..., ::2, ::2])
    with pytest.raises(ValueError, match="scale_factor"):
        visual.storyboard(small, panels=("generated", "dense_motion_bw"))
