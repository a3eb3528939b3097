"""Click-to-move on the GPU (run with -m gpu): the instance-box kernels against a NumPy restatement, the graph from
instance maps against the tracker-file graph, and click_to_move against model.inference on that graph."""
import copy

import numpy as np
import pytest
import torch

from c2m_amd import graph as G
from c2m_amd import interactive as I
from c2m_amd import ops
from c2m_amd.config import default_config, normalize_config
from c2m_amd.modules.model import GeneratorFullModel
from c2m_amd.synthetic import make_batch, batch_to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = np.iinfo(np.int32).max
FIELDS = ("x", "y", "source_frames_nodes_roi", "source_frames_nodes_roi_padded", "target_frames_nodes_roi",
          "source_frames_nodes_instance_ids", "target_frames_nodes_instance_ids", "targets_barycenter",
          "targets_displacement", "targets_theta", "num_real_nodes", "edge_index", "batch", "ptr")


# ------------------------------------------------------------------------------------------------ kernel vs NumPy
def np_stats(inst, t_in, lo, hi):
    """inst [B,T,H,W] -> [B, t_in, hi - lo, 5] (count, x_min, x_max, y_min, y_max; absent: 0, BIG, -1, BIG, -1)."""
    B, _, H, W = inst.shape
    out = np.zeros((B, t_in, hi - lo, 5), np.int64)
    out[..., 1] = out[..., 3] = BIG
    out[..., 2] = out[..., 4] = -1
    ys, xs = np.divmod(np.arange(H * W), W)
    for b in range(B):
        for t in range(t_in):
            v = inst[b, t].reshape(-1).astype(np.int64)
            m = (v >= lo) & (v < hi)
            k, x, y = v[m] - lo, xs[m], ys[m]
            o = out[b, t]
            o[:, 0] = np.bincount(k, minlength=hi - lo)
            np.minimum.at(o[:, 1], k, x)
            np.maximum.at(o[:, 2], k, x)
            np.minimum.at(o[:, 3], k, y)
            np.maximum.at(o[:, 4], k, y)
    return out


def np_boxes(table, lo, min_pixels, max_nodes):
    B, t_in = table.shape[:2]
    ids = np.zeros((B, max_nodes), np.int64)
    boxes = np.zeros((B, max_nodes, t_in, 4), np.int64)
    count = np.zeros(B, np.int64)
    for b in range(B):
        keep = np.nonzero((table[b, :, :, 0] >= min_pixels).all(0))[0]
        assert len(keep) <= max_nodes
        count[b] = len(keep)
        ids[b, :len(keep)] = keep + lo
        e = table[b][:, keep]                                            # [t_in, n, 5]
        boxes[b, :len(keep)] = np.stack([e[..., 1], e[..., 3], e[..., 2] + 1, e[..., 4] + 1], -1).transpose(1, 0, 2)
    return ids, boxes, count


POOL = np.array([0, 7, 500, 999, 1000, 11001, 11002, 11003, 12001, 12002, 13001, 13002, 14001, 15001, 15002, 16001,
                 17001, 17002, 18001, 18002, 18999, 19000, 24000, 26001, 33001])


def blocky(B, T, H, W, seed, block=16, pool=POOL):
    """Random block-constant id maps with the edge cases placed on top."""
    rng = np.random.default_rng(seed)
    bh, bw = -(-H // block), -(-W // block)
    inst = pool[rng.integers(0, len(pool), (B, T, bh, bw))]
    inst = inst.repeat(block, 2).repeat(block, 3)[:, :, :H, :W].astype(np.int32)
    inst[:, :, 0, 0] = 1500                    # corners and borders
    inst[:, :, H - 1, W - 1] = 1501
    inst[:, :, 0, W // 2:W // 2 + 7] = 1502
    inst[:, :, H // 3:H // 3 + 5, W - 1] = 1503
    inst[:, :, 10:12, 20:22] = 1000            # both ends of the id range
    inst[:, :, 20:22, 40:44] = 18999
    inst[:, :, H // 2, W // 3] = 17777         # one-pixel instances
    inst[:, :, H - 1, 0] = 17778
    inst[:, 0, 5:9, 5:9] = 16666               # only in frame 0: dropped when t_in = 2
    inst[:, -1] = 14444                        # a frame past the input frames: never read
    return inst


@pytest.mark.parametrize("size", [(128, 256), (188, 352), (1024, 2048)])
@pytest.mark.parametrize("B,t_in", [(1, 1), (3, 2), (1, 2), (3, 1)])
def test_instance_boxes_vs_numpy(size, B, t_in):
    H, W = size
    inst = blocky(B, t_in + 1, H, W, seed=H + B * 10 + t_in)
    lo, hi = 1000, 19000
    want_tab = np_stats(inst, t_in, lo, hi)
    d = torch.from_numpy(inst).to(DEV)
    tab = ops.instance_stats(d, t_in).cpu()
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (B, t_in, hi - lo, 5)
    assert np.array_equal(tab.numpy(), want_tab)
    assert torch.equal(ops.instance_stats(d.unsqueeze(1), t_in).cpu(), tab)      # [B,1,T,H,W] too; bit-repeatable
    for min_pixels in (1, 2, 40):
        ids, boxes, count = ops.instance_boxes(d, t_in, min_pixels=min_pixels)
        w_ids, w_boxes, w_count = np_boxes(want_tab, lo, min_pixels, 64)
        assert np.array_equal(ids.numpy(), w_ids) and np.array_equal(count.numpy(), w_count)
        assert np.array_equal(boxes.numpy(), w_boxes)
        again = ops.instance_boxes(d, t_in, min_pixels=min_pixels)
        assert all(torch.equal(a, b) for a, b in zip((ids, boxes, count), again))
    ids, boxes, count = ops.instance_boxes(d, t_in)
    row = ids[0, :int(count[0])].tolist()
    assert {1000, 1500, 1501, 1502, 1503, 17777, 17778, 18999} <= set(row)
    assert not {0, 7, 500, 999, 14444, 19000, 24000, 26001, 33001} & set(row)
    assert (16666 in row) == (t_in == 1)
    n = row.index(17777)
    assert boxes[0, n, 0].tolist() == [W // 3, H // 2, W // 3 + 1, H // 2 + 1]
    n = row.index(1501)
    assert boxes[0, n, 0].tolist() == [W - 1, H - 1, W, H]


def test_instance_boxes_overflow_and_id_range():
    H, W = 64, 320
    inst = np.zeros((2, 1, H, W), np.int32)
    for k in range(100):                                  # 100 objects in sample 1, 3 in sample 0
        inst[1, 0, (k // 20) * 8:(k // 20) * 8 + 4, (k % 20) * 16:(k % 20) * 16 + 8] = 11000 + k
    inst[0, 0, :4, :4], inst[0, 0, 10:12, 10:30], inst[0, 0, 40:, 300:] = 11001, 12001, 13001
    d = torch.from_numpy(inst).to(DEV)
    with pytest.raises(ValueError, match=r"\[1\].*max_nodes=64"):
        ops.instance_boxes(d, 1)
    ids, boxes, count = ops.instance_boxes(d, 1, max_nodes=128)
    assert count.tolist() == [3, 100] and ids[1, :100].tolist() == list(range(11000, 11100))
    assert ids[0, :3].tolist() == [11001, 12001, 13001] and not ids[0, 3:].any() and not boxes[0, 3:].any()
    ids, boxes, count = ops.instance_boxes(d, 1, id_range=(12000, 13002), max_nodes=4)   # the others are ignored
    assert count.tolist() == [2, 0] and ids[0, :2].tolist() == [12001, 13001]
    assert boxes[0, 0, 0].tolist() == [10, 10, 30, 12] and boxes[0, 1, 0].tolist() == [300, 40, 320, 64]
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.instance_boxes(torch.from_numpy(inst), 1)
    with pytest.raises(ValueError):
        ops.instance_boxes(d, 2)                          # only one frame


def test_instance_boxes_small_maps_many_objects():
    """8 x 96 maps, three input frames, ids in [1000, 1600) at the first and last lane of a wave and of a 256-id chunk: 70
    objects in sample 0 (max_nodes = 128: more than one wave of slots), the every-frame rule and the one-over-the-limit case."""
    lo, hi, t_in, H, W = 1000, 1600, 3, 8, 96
    rng = np.random.default_rng(9)
    edges = [0, 63, 64, 255, 256, 257, 511, 512, 599]
    gone, thin = 300, 301                                 # absent in frame 1; two pixels in frame 1 only
    rest = np.setdiff1d(np.arange(hi - lo), edges + [gone, thin])
    objects = [np.concatenate([edges, rng.choice(rest, 70 - len(edges), replace=False), [gone, thin]]), np.array([599, 5, 256])]
    inst = np.array([0, 7, 999, 1600], np.int32)[rng.integers(0, 4, (2, t_in, H, W))]     # ids outside the range: ignored
    for b, offs in enumerate(objects):
        for cell, off in zip(rng.permutation(96), offs):  # 2 x 4 cells; frame t keeps 4 - t columns: 8, 6 and 4 pixels
            r0, c0 = (cell // 24) * 2, (cell % 24) * 4
            for t in range(t_in):
                inst[b, t, r0:r0 + 2, c0:c0 + 4] = 0
                if off == gone and t == 1:
                    continue
                inst[b, t, r0:r0 + (1 if off == thin and t == 1 else 2), c0:c0 + (2 if off == thin and t == 1 else 4 - t)] = lo + off
    table = np_stats(inst, t_in, lo, hi)
    d = torch.from_numpy(inst).to(DEV)
    assert np.array_equal(ops.instance_stats(d, t_in, id_range=(lo, hi)).cpu().numpy(), table)
    for min_pixels, kept in ((1, [71, 3]), (3, [70, 3])):
        ids, boxes, count = ops.instance_boxes(d, t_in, id_range=(lo, hi), min_pixels=min_pixels, max_nodes=128)
        w_ids, w_boxes, w_count = np_boxes(table, lo, min_pixels, 128)
        assert w_count.tolist() == kept and np.array_equal(count.numpy(), w_count)
        assert np.array_equal(ids.numpy(), w_ids) and np.array_equal(boxes.numpy(), w_boxes)
        row = ids[0, :kept[0]].tolist()
        assert lo + gone not in row and (lo + thin in row) == (min_pixels == 1)
        assert set(lo + np.array(edges)) <= set(row) and ids[1, :3].tolist() == [lo + 5, lo + 256, lo + 599]
    ids, boxes, count = ops.instance_boxes(d, t_in, id_range=(lo, hi), min_pixels=3, max_nodes=70)      # exactly at the limit
    assert count.tolist() == [70, 3] and np.array_equal(ids.numpy(), np_boxes(table, lo, 3, 70)[0])
    with pytest.raises(ValueError, match=r"\[0\].*max_nodes=69"):
        ops.instance_boxes(d, t_in, id_range=(lo, hi), min_pixels=3, max_nodes=69)                       # one over


# ------------------------------------------------------------------------------------------------ the tracker path
# last-input-frame rectangles (id, x0, y0, x1, y1) at 128x256; input frame t sits (t_in - 1 - t) px further left
RECTS = [[(11001, 20, 30, 60, 60), (13001, 100, 40, 130, 90), (18999, 180, 70, 220, 100)],
         [(12005, 30, 20, 70, 50), (17002, 150, 60, 200, 110)]]
DRAGS = [I.Drag(0, 110, 60, 120, 55), I.Drag(1, 40, 30, 25, 35)]       # per frame (2, -1) and (-3, 1) pixels
T_OUT = 5


def scene(B, t_in, T_total, seed=0):
    rng = np.random.default_rng(seed)
    inst = rng.choice(np.array([0, 7, 24001], np.int32), (B, 1, T_total, 128, 256))
    inst[:, :, :t_in] = 7
    for b in range(B):
        for t in range(t_in):
            for i, x0, y0, x1, y1 in RECTS[b]:
                s = t_in - 1 - t
                inst[b, 0, t, y0:y1, x0 - s:x1 - s] = i
    return inst


def drag_step(drag):
    return (drag.to_x - drag.x) // T_OUT, (drag.to_y - drag.y) // T_OUT


def tracker_graph(B, t_in, drags):
    """The same scene as tracker text lines (boxes x 8 = 2048x1024 pixels, exact), sorted by id -> scene_graph."""
    graphs = []
    for b in range(B):
        tracks = []
        for i, x0, y0, x1, y1 in RECTS[b]:
            lines = [(x0 - (t_in - 1 - t), y0, x1 - (t_in - 1 - t), y1) for t in range(t_in)]
            d = next((d for d in drags if d.sample == b and x0 <= d.x < x1 and y0 <= d.y < y1), None)
            sx, sy = drag_step(d) if d is not None else (0, 0)
            lines += [(x0 + sx * (t + 1), y0 + sy * (t + 1), x1 + sx * (t + 1), y1 + sy * (t + 1)) for t in range(T_OUT)]
            tracks.append([f"{a * 8},{c * 8},{(e - a) * 8},{(f - c) * 8},0.9,{i}" for a, c, e, f in lines])
        graphs.append(G.scene_graph(tracks, (128, 256), t_in, t_in + T_OUT)[1])
    return G.collate_graphs(graphs)


def small_model(t_in, use_gt_eval=False, seed=0):
    cfg = normalize_config(default_config(num_input_frames=t_in, block_expansion=4, max_expansion=32, h_dim=32, z_dim=16,
                                          out_channel=16, ndf=4, use_image_discriminator=False,
                                          use_video_discriminator=False))
    cfg["train_params"]["use_gt_eval"] = use_gt_eval
    torch.manual_seed(seed)
    model = GeneratorFullModel(train_params=copy.deepcopy(cfg["train_params"]),
                               model_params=copy.deepcopy(cfg["model_params"]), dataset="cityscapes", is_inference=True)
    return model.to(DEV).eval()


def inputs(B, t_in, seed=0):
    batch = batch_to(make_batch(B, 128, 256, t_in, seed=seed), DEV)
    batch["instance_mask"] = torch.from_numpy(scene(B, t_in, t_in + T_OUT, seed)).to(DEV)
    return batch


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("t_in", [1, 2])
def test_graph_and_outputs_equal_the_tracker_path(t_in):
    B = 2
    batch = inputs(B, t_in)
    g, click = I.graph_from_instances(batch["instance_mask"], DRAGS, t_in, T_OUT)
    ref = tracker_graph(B, t_in, DRAGS)
    for k in FIELDS:
        x, y = getattr(g, k), getattr(ref, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
    assert g.num_nodes == ref.num_nodes and click.tolist() == [1, 3]
    model = small_model(t_in)
    z_m = torch.randn(B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(11)
    got = I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], DRAGS,
                          batch["input_of"], batch["input_occ"], z_m=z_m)
    torch.manual_seed(11)
    with torch.no_grad():
        want = model.inference(batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"],
                               batch["input_of"], batch["input_occ"], ref.to(DEV), click.to(DEV), z_m.to(DEV))
    torch.cuda.synchronize()
    _same_outputs(got, want)
    assert got["generated"].shape == (B, 3, T_OUT, 128, 256) and torch.isfinite(got["generated"]).all()


def test_the_future_is_not_read():
    B, t_in = 2, 2
    batch = inputs(B, t_in)
    model = small_model(t_in)
    z_m = torch.randn(B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(6))
    cut = lambda x: None if x is None else x[:, :, :t_in].contiguous()
    torch.manual_seed(3)
    a = I.click_to_move(model, cut(batch["video"]), cut(batch["bg_mask"]), cut(batch["fg_mask"]),
                        cut(batch["instance_mask"]), DRAGS, batch["input_of"], batch["input_occ"], z_m=z_m)
    gen = torch.Generator().manual_seed(99)
    noisy = {k: batch[k].clone() for k in ("video", "bg_mask", "fg_mask", "instance_mask")}
    noisy["video"][:, :, t_in:] = torch.rand(noisy["video"][:, :, t_in:].shape, generator=gen).to(DEV)
    noisy["bg_mask"][:, :, t_in:] = (torch.rand(noisy["bg_mask"][:, :, t_in:].shape, generator=gen) > 0.5).float().to(DEV)
    noisy["instance_mask"][:, :, t_in:] = torch.randint(11000, 12000, noisy["instance_mask"][:, :, t_in:].shape,
                                                        generator=gen, dtype=torch.int32).to(DEV)
    torch.manual_seed(3)
    b = I.click_to_move(model, noisy["video"], noisy["bg_mask"], noisy["fg_mask"], noisy["instance_mask"], DRAGS,
                        batch["input_of"], batch["input_occ"], z_m=z_m)
    torch.cuda.synchronize()
    _same_outputs(a, b)


def _raster_flow(x, dx_pix, n):
    """sparse_motion_bw of a pure translation by dx_pix pixels at pixel column x of an n-wide frame, as the raster defines
    it (reference dense_motion.py warp: affine_grid(align_corners=False) minus a linspace grid, times (n - 1) / 2):
    ((lx (n-1)/n - 2 dx_pix / n) - lx) (n-1)/2 with lx = -1 + 2x/(n-1) = -dx_pix (n-1)/n plus a sub-pixel offset
    that the identity theta has as well."""
    lx = -1.0 + 2.0 * x / (n - 1)
    return (lx * (n - 1) / n - 2.0 * dx_pix / n - lx) * (n - 1) / 2


def test_the_drag_moves_the_object():
    t_in = 2
    batch = inputs(1, t_in)
    model = small_model(t_in, use_gt_eval=True)
    torch.manual_seed(0)
    out = I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], DRAGS[:1],
                          batch["input_of"], batch["input_occ"])
    bw, binm = out["sparse_motion_bw"][0].cpu().double(), out["sparse_motion_bin"][0, 0].cpu()
    ys, xs = torch.meshgrid(torch.arange(128, dtype=torch.float64), torch.arange(256, dtype=torch.float64), indexing="ij")
    sx, sy = drag_step(DRAGS[0])
    for t in range(T_OUT):
        covered = torch.zeros(128, 256, dtype=torch.bool)
        for i, x0, y0, x1, y1 in RECTS[0]:
            dx, dy = (sx * (t + 1), sy * (t + 1)) if i == 13001 else (0, 0)
            rect = torch.zeros(128, 256, dtype=torch.bool)
            rect[y0 + dy:y1 + dy, x0 + dx:x1 + dx] = True
            inside = rect & (binm[t] == 1)
            assert inside.sum() >= 0.5 * rect.sum(), (i, t, int(inside.sum()), int(rect.sum()))   # the support moved
            ex, ey = _raster_flow(xs, dx, 256), _raster_flow(ys, dy, 128)
            assert (bw[0, t][inside] - ex[inside]).abs().max() <= 1e-4, (i, t)
            assert (bw[1, t][inside] - ey[inside]).abs().max() <= 1e-4, (i, t)
            if i != 13001:      # unclicked: no motion beyond the identity theta's sub-pixel grid offset (< 0.5 px)
                assert bw[:, t][:, inside].abs().max() < 0.5
            covered |= rect
        assert not (binm[t].bool() & ~covered).any(), t                   # no support anywhere else
        assert not bw[:, t][:, binm[t] == 0].any(), t                      # and zero flow off the supports


def test_two_drags_in_one_sample():
    t_in = 2
    batch = inputs(1, t_in)
    drags = [I.Drag(0, 110, 60, 120, 55), I.Drag(0, 200, 80, 190, 90)]
    g, click = I.graph_from_instances(batch["instance_mask"], drags, t_in, T_OUT)
    assert click.tolist() == [1, 2]
    for n, (sx, sy) in zip(click.tolist(), [(2, -1), (-2, 2)]):
        for t in range(T_OUT):
            want = [1, 0, -2 * sx * (t + 1) / 256, 0, 1, -2 * sy * (t + 1) / 128]
            assert np.allclose(g.targets_theta[n, t].double().numpy(), want, atol=1e-7, rtol=0)
    assert torch.equal(g.targets_theta[0], torch.tensor([1, 0, 0, 0, 1, 0.]).expand(T_OUT, 6))
    model = small_model(t_in)
    torch.manual_seed(0)
    out = I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], drags,
                          batch["input_of"], batch["input_occ"])
    assert out["index_user_guidance"].tolist() == [1, 2]
    for t in range(T_OUT):
        th = out[f"theta_{t}"].cpu()
        assert torch.equal(th[click], g.targets_theta[click, t]), t
