"""Tracking from instance maps on the GPU (run with -m gpu): the instance-link kernels against NumPy restatements (the overlap
table through ops.label_warp, which is pinned to the oracle), known tracks recovered from painted scenes, behaviour under
trouble, and the tracked batch through the model against the tracker-file batch."""
import copy

import numpy as np
import pytest
import torch

from c2m_amd import data as D
from c2m_amd import graph as G
from c2m_amd import interactive as I
from c2m_amd import ops
from c2m_amd import tracking as TR
from c2m_amd.config import default_config, normalize_config
from c2m_amd.modules.model import GeneratorFullModel
from c2m_amd.synthetic import make_batch, make_step_rng, batch_to
import gpu_util
import tracking_np as NP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = 64
FIELDS = ("x", "y", "source_frames_nodes_roi", "source_frames_nodes_roi_padded", "target_frames_nodes_roi",
          "source_frames_nodes_instance_ids", "target_frames_nodes_instance_ids", "targets_barycenter",
          "targets_displacement", "targets_theta", "num_real_nodes", "edge_index")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------ inputs
def random_maps(P, H, W, seed, n_ids=40, pool_seed=None):
    """Block-constant maps, about 40 % object pixels on at most n_ids ids, with per-pixel speckle on top.  pool_seed: the seed
    the ids are drawn with (maps with the same pool_seed share their n_ids ids); the map's own seed by default."""
    rng = np.random.default_rng(seed)
    pool = rng if pool_seed is None else np.random.default_rng(pool_seed)
    ids = np.sort(pool.choice(np.arange(11000, 19000), n_ids, replace=False))
    bh, bw = -(-H // 8), -(-W // 8)
    obj = rng.random((P, bh, bw)) < 0.4
    blocks = np.where(obj, ids[rng.integers(0, n_ids, (P, bh, bw))], np.array([0, 7, 24001])[rng.integers(0, 3, (P, bh, bw))])
    maps = blocks.repeat(8, 1).repeat(8, 2)[:, :H, :W].astype(np.int32)
    speckle = rng.random((P, H, W)) < 0.02
    maps[speckle] = ids[rng.integers(0, n_ids, int(speckle.sum()))]
    return maps


def random_flow(P, H, W, seed, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == "pixel":
        f = 6.0 * torch.randn(P, 2, H, W, generator=g)
        f[:, :, :2] = float("nan")                             # the border clamp and the NaN rule are part of the coordinate
        f[:, :, 2:4] = 1.0e9
        return f
    coarse = 8.0 * torch.randn(P, 2, -(-H // 16) + 1, -(-W // 16) + 1, generator=g)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).contiguous()


def slot_lists(maps, min_pixels=1):
    P = maps.shape[0]
    slots, count = np.full((P, M), -1, np.int32), np.zeros(P, np.int32)
    for p in range(P):
        ids = NP.np_slots(maps[p], min_pixels=min_pixels)[0]
        assert len(ids) <= M
        slots[p, :len(ids)], count[p] = ids, len(ids)
    return slots, count


def expected_pairs(ref, frame, flow, rs, rc, fs, fc):
    P, H, W = ref.shape
    warped = ref if flow is None else ops.label_warp(flow, planes_i=dev(ref)[:, None])[1].cpu().numpy().reshape(P, H, W)
    out = np.zeros((P, M + 1, M + 1), np.int64)
    for p in range(P):
        out[p] = NP.np_pairs(warped[p], frame[p], None, rs[p, :rc[p]].astype(np.int64), fs[p, :fc[p]].astype(np.int64), M)
    return out


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("P,size", [(3, (128, 256)), (3, (128, 416)), (2, (93, 187)), (2, (1024, 2048)), (1, (128, 256)),
                                    (40, (128, 256))])
@pytest.mark.parametrize("kind", ["smooth", "pixel", None])
def test_overlap_table_bit_for_bit(P, size, kind):
    H, W = size
    ref, frame = random_maps(P, H, W, 1 + H + P, pool_seed=77), random_maps(P, H, W, 2 + W + P, pool_seed=77)
    frame[:, H // 2:] = ref[:, H // 2:]                          # half of every frame really is the reference (one pool of 40 ids)
    flow = None if kind is None else random_flow(P, H, W, 3 + H, kind).to(DEV)
    (rs, rc), (fs, fc) = slot_lists(ref), slot_lists(frame, min_pixels=3)
    want = expected_pairs(ref, frame, flow, rs, rc, fs, fc)
    args = (dev(ref), dev(frame), flow, dev(rs), dev(rc), dev(fs), dev(fc))
    got = ops.instance_overlap(*args)
    assert got.dtype == torch.int32 and tuple(got.shape) == (P, M + 1, M + 1)
    assert int(got.sum()) == P * H * W
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.instance_overlap(*args), got)          # bit-repeatable


def test_overlap_without_flow_is_same_pixel_overlap():
    P, H, W = 1, 64, 96
    ref = random_maps(P, H, W, 5)
    (rs, rc) = slot_lists(ref)
    args = (dev(ref), dev(ref), dev(rs), dev(rc), dev(rs), dev(rc))
    plain = ops.instance_overlap(args[0], args[1], None, *args[2:]).cpu()
    off = plain[0, :M, :M] - torch.diag(torch.diagonal(plain[0, :M, :M]))
    assert not off.any() and not plain[0, M, :M].any() and not plain[0, :M, M].any()      # a map overlaps itself exactly
    assert int(plain.sum()) == H * W
    # a zero flow goes through the warp's coordinates like any other flow: whatever label_warp reads, the table counts
    zero = torch.zeros(P, 2, H, W, device=DEV)
    got = ops.instance_overlap(args[0], args[1], zero, *args[2:]).cpu().numpy()
    assert np.array_equal(got, expected_pairs(ref, ref, zero, rs, rc, rs, rc))


@pytest.mark.parametrize("size,B,T", [((128, 256), 3, 3), ((188, 352), 2, 2)])
def test_slots_vs_numpy_and_instance_boxes(size, B, T):
    H, W = size
    inst = random_maps(B * T, H, W, 11, n_ids=30).reshape(B, T, H, W)
    inst[:, :, 0, 0], inst[:, :, H - 1, W - 1], inst[:, :, 5, 7:9] = 1000, 18999, 17777
    d = dev(inst)
    table = ops.instance_stats(d, T)
    for min_pixels in (1, 2, 40):
        slots, boxes, areas, count, overflow = (t.cpu().numpy() for t in ops.instance_slots(table, min_pixels=min_pixels))
        assert slots.shape == (B, T, M) and boxes.shape == (B, T, M, 4) and not overflow.any()
        for b in range(B):
            for t in range(T):
                ids, bx, ar = NP.np_slots(inst[b, t], min_pixels=min_pixels)
                n = len(ids)
                assert count[b, t] == n and np.array_equal(slots[b, t, :n], ids) and (slots[b, t, n:] == -1).all()
                assert np.array_equal(boxes[b, t, :n], bx) and not boxes[b, t, n:].any()
                assert np.array_equal(areas[b, t, :n], ar) and not areas[b, t, n:].any()
        for t in range(T):          # one input frame: every id of the plane is "present in all input frames"
            ids, bx, cnt = ops.instance_boxes(d[:, t:t + 1].contiguous(), 1, min_pixels=min_pixels)
            for b in range(B):
                n = int(cnt[b])
                assert n == count[b, t] and np.array_equal(ids[b, :n].numpy(), slots[b, t, :n])
                assert np.array_equal(bx[b, :n, 0].numpy(), boxes[b, t, :n])
    with pytest.raises(ValueError, match="kernel cap"):
        ops.instance_slots(table, max_nodes=65)
    with pytest.raises(ValueError, match="min_pixels"):
        ops.instance_slots(table, min_pixels=0)
    with pytest.raises(ValueError, match="table must be"):
        ops.instance_slots(table, id_range=(1000, 18000))
    with pytest.raises(TypeError, match="int32"):
        ops.instance_slots(table.long())


def test_slots_on_a_table_at_wave_and_chunk_edges():
    """A hand-made table of 600 ids (chunks of 256, 256 and 88 entries for the 256-thread workgroup) with qualifying ids at the
    first and last lane of a wave and of a chunk; counts of 2 sit next to them, so min_pixels = 3 leaves them out."""
    lo, nid, big = 1000, 600, np.iinfo(np.int32).max
    edges = [0, 63, 64, 255, 256, 257, 511, 512, 599]
    twos = [1, 62, 65, 254, 258, 510, 513, 598]
    rng = np.random.default_rng(5)
    rest = np.setdiff1d(np.arange(nid), edges + twos)
    table = np.zeros((3, nid, 5), np.int32)
    table[..., 1], table[..., 2], table[..., 3], table[..., 4] = big, -1, big, -1        # absent ids, as instance_stats leaves them
    for p, n in ((0, 64), (1, 65)):                                  # plane 2 stays empty
        big_ids = np.concatenate([edges, rng.choice(rest, n - len(edges), replace=False)])
        table[p, big_ids, 0] = rng.integers(3, 900, n)
        table[p, twos, 0] = 2
        present = table[p, :, 0] > 0
        k = int(present.sum())
        x0, y0 = rng.integers(0, 100, k), rng.integers(0, 50, k)
        table[p, present, 1], table[p, present, 2] = x0, x0 + rng.integers(0, 30, k)
        table[p, present, 3], table[p, present, 4] = y0, y0 + rng.integers(0, 30, k)
    d = dev(table)
    for min_pixels in (1, 3):
        slots, boxes, areas, count, overflow = (t.cpu().numpy() for t in
                                                ops.instance_slots(d, id_range=(lo, lo + nid), min_pixels=min_pixels))
        assert slots.shape == (3, M) and boxes.shape == (3, M, 4) and areas.shape == (3, M) and count.shape == (3,)
        for p in range(3):
            found = np.nonzero(table[p, :, 0] >= min_pixels)[0]      # ascending
            keep = found[:M]
            n, e = len(keep), table[p, keep].astype(np.int64)
            assert count[p] == n and overflow[p] == (len(found) > M), (p, min_pixels)
            assert np.array_equal(slots[p, :n], keep + lo) and (slots[p, n:] == -1).all()
            assert np.array_equal(boxes[p, :n], np.stack([e[:, 1], e[:, 3], e[:, 2] + 1, e[:, 4] + 1], -1))
            assert np.array_equal(areas[p, :n], e[:, 0]) and not boxes[p, n:].any() and not areas[p, n:].any()
        if min_pixels == 3:
            assert count.tolist() == [64, 64, 0] and overflow.tolist() == [0, 1, 0]
            assert set(lo + np.array(edges)) <= set(slots[0].tolist()) and not set(lo + np.array(twos)) & set(slots[0].tolist())
            assert slots[1, 0] == lo and slots[1, -1] < lo + 599     # the 65th id, the last of the table, is the one dropped
        else:
            assert count.tolist() == [64, 64, 0] and overflow.tolist() == [1, 1, 0]       # 72 and 73 ids


def test_match_kernel_vs_host_rule():
    rng = np.random.default_rng(3)
    P = 48
    pairs = np.zeros((P, M + 1, M + 1), np.int32)
    rs, fs = np.full((P, M), -1, np.int32), np.full((P, M), -1, np.int32)
    rc, fc = rng.integers(0, 9, P).astype(np.int32), rng.integers(0, 9, P).astype(np.int32)
    rc[0], fc[1], rc[2], fc[2] = 0, 0, M, M
    for p in range(P):
        rs[p, :rc[p]] = np.sort(rng.choice(np.arange(11000, 14000, 40), rc[p], replace=False))
        fs[p, :fc[p]] = np.sort(rng.choice(np.arange(11000, 14000, 40), fc[p], replace=False))
        big = 1 if p % 3 else 300000                             # products beyond 32 bits
        sub = rng.integers(0, 6, (rc[p] + 1, fc[p] + 1)) * rng.integers(0, 2, (rc[p] + 1, fc[p] + 1)) * big
        pairs[p, :rc[p], :fc[p]], pairs[p, :rc[p], M], pairs[p, M, :fc[p]], pairs[p, M, M] = \
            sub[:-1, :-1], sub[:-1, -1], sub[-1, :-1], sub[-1, -1]
    for kw in (dict(), dict(min_iou=(1, 2)), dict(same_class=False), dict(min_iou=(0, 1), same_class=False)):
        got = ops.instance_match(dev(pairs), dev(rs), dev(rc), dev(fs), dev(fc), **kw).cpu().numpy()
        for p in range(P):
            nr, nf = rc[p], fc[p]
            sub = np.zeros((nr + 1, nf + 1), np.int64)
            sub[:nr, :nf], sub[:nr, nf], sub[nr, :nf], sub[nr, nf] = pairs[p, :nr, :nf], pairs[p, :nr, M], pairs[p, M, :nf], pairs[p, M, M]
            assert np.array_equal(got[p, :nr], TR.match_host(sub, rs[p, :nr], fs[p, :nf], **kw)), (p, kw)
            assert (got[p, nr:] == -1).all()
    with pytest.raises(ValueError, match="min_iou"):
        ops.instance_match(dev(pairs), dev(rs), dev(rc), dev(fs), dev(fc), min_iou=0.25)
    with pytest.raises(ValueError, match="min_iou"):
        ops.instance_match(dev(pairs), dev(rs), dev(rc), dev(fs), dev(fc), min_iou=(3, 2))
    with pytest.raises(ValueError, match="pairs must be"):
        ops.instance_match(dev(pairs[:, :M]), dev(rs), dev(rc), dev(fs), dev(fc))


def test_ops_run_in_stream_order():
    """On a non-default current stream, right after their producers, with the producers held back: no host sync anywhere."""
    P, H, W = 4, 128, 256
    ref, frame = random_maps(P, H, W, 21), random_maps(P, H, W, 22)
    flow = random_flow(P, H, W, 23, "smooth")
    (rs, rc), (fs, fc) = slot_lists(ref), slot_lists(frame)
    want = expected_pairs(ref, frame, flow.to(DEV), rs, rc, fs, fc)
    both = dev(np.stack([ref, frame], 1))                        # [P, 2, H, W]: the two frames of P samples
    host = [t.pin_memory() for t in (torch.from_numpy(np.stack([ref, frame], 1)), flow)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, flow.to(DEV))
        junk = [torch.full_like(both, -1) for _ in range(2)]       # (the helper fills NaN: float tensors only)
        del junk
        gpu_util.stretch(side, 20.0)
        maps = host[0].to(DEV, non_blocking=True)                # the producers: queued behind the delay
        fl = host[1].to(DEV, non_blocking=True)
        table = ops.instance_stats(maps, 2)
        slots, _, _, count, _ = ops.instance_slots(table)
        a = (slots[:, 0].contiguous(), count[:, 0].contiguous(), slots[:, 1].contiguous(), count[:, 1].contiguous())
        pairs = ops.instance_overlap(maps[:, 0].contiguous(), maps[:, 1].contiguous(), fl, *a)
        link = ops.instance_match(pairs, *a)
    side.synchronize()
    assert np.array_equal(pairs.cpu().numpy(), want)
    for p in range(P):
        nr, nf = rc[p], fc[p]
        sub = np.zeros((nr + 1, nf + 1), np.int64)
        sub[:nr, :nf], sub[:nr, nf], sub[nr, :nf], sub[nr, nf] = want[p, :nr, :nf], want[p, :nr, M], want[p, M, :nf], want[p, M, M]
        assert np.array_equal(link[p, :nr].cpu().numpy(), TR.match_host(sub, rs[p, :nr], fs[p, :nf]))


# ------------------------------------------------------------------------------------------------ known tracks
def run_tracker(scenes, t_in, **kw):
    inst = dev(np.stack([s["inst"] for s in scenes])[:, None])
    tf = dev(np.stack([s["target_flow"] for s in scenes]))
    inf = dev(np.stack([s["input_flow"] for s in scenes])) if t_in > 1 else None
    return TR.track_instances(inst, t_in, tf, inf, **kw)


@pytest.mark.parametrize("kind,arg,t_in", NP.SCENES)
def test_recovers_known_tracks(kind, arg, t_in):
    size, T = (128, 256), 7
    edges, ids, sc = NP.make_scene(kind, arg, t_in)
    tr = run_tracker([sc], t_in)
    want_ids, want_boxes = NP.painted_extents(sc)
    order = np.argsort(ids)
    n = len(ids)
    assert tr.count.tolist() == [n] and tr.lost == [[]]                       # every object, nothing left out
    assert np.array_equal(tr.ids[0, :n].numpy(), want_ids[order]) and not tr.ids[0, n:].any()
    assert np.array_equal(tr.boxes[0, :n].numpy(), want_boxes[order]) and not tr.boxes[0, n:].any()
    tids, graphs = TR.scene_graphs(tr, size, t_in)
    w_ids, want = G.scene_graph_from_boxes(I.edges_to_tracker(want_boxes[order], size), want_ids[order], size, t_in, T)
    assert torch.equal(tids[0], w_ids)
    for k in FIELDS:
        x, y = getattr(graphs[0], k), getattr(want, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
    np_ids, np_boxes, np_lost = NP.np_track(sc["inst"], t_in, sc["target_flow"], sc["input_flow"])
    assert np.array_equal(tr.ids[0, :n].numpy(), np_ids) and np.array_equal(tr.boxes[0, :n].numpy(), np_boxes)
    if t_in == 1:      # the nodes of graph_from_instances
        b_ids, b_edges, b_count = ops.instance_boxes(dev(sc["inst"][None, None]), 1)
        assert int(b_count[0]) == n and torch.equal(b_ids[0, :n], tr.ids[0, :n, 0])
        assert torch.equal(b_edges[0, :n, 0], tr.boxes[0, :n, 0])


def test_a_batch_of_scenes_and_a_perturbed_flow():
    t_in = 2
    made = [NP.make_scene("constructed", 12, t_in, seed=s) for s in (0, 1, 2)]
    scenes = [m[2] for m in made]
    tr = run_tracker(scenes, t_in)
    assert tr.count.tolist() == [12, 12, 12] and tr.lost == [[], [], []]
    for b, (edges, ids, sc) in enumerate(made):
        want_ids, want_boxes = NP.painted_extents(sc)
        order = np.argsort(ids)
        assert np.array_equal(tr.ids[b, :12].numpy(), want_ids[order]) and np.array_equal(tr.boxes[b, :12].numpy(), want_boxes[order])
    rng = np.random.default_rng(9)
    for s in scenes:                                              # +-1 px on every component: the same links
        s["target_flow"] = s["target_flow"] + rng.integers(-1, 2, s["target_flow"].shape).astype(np.float32)
        s["input_flow"] = s["input_flow"] + rng.integers(-1, 2, s["input_flow"].shape).astype(np.float32)
    again = run_tracker(scenes, t_in)
    assert torch.equal(again.ids, tr.ids) and torch.equal(again.boxes, tr.boxes) and again.lost == tr.lost
    same = run_tracker(scenes, t_in)
    assert torch.equal(same.ids, again.ids) and torch.equal(same.boxes, again.boxes)


def test_a_removed_object_is_lost_and_the_others_stay():
    t_in = 2
    edges, ids, sc = NP.make_scene("constructed", 12, t_in)
    order = np.argsort(ids)
    k, t = int(order[4]), 5                                        # the fifth node disappears from target frame 5
    sc["inst"][t][sc["owner"][t] == k] = 7
    tr = run_tracker([sc], t_in)
    want_ids, want_boxes = NP.painted_extents(NP.make_scene("constructed", 12, t_in)[2])
    rest = [i for i in order if i != k]
    assert tr.count.tolist() == [11] and tr.lost == [[(int(ids[k]), t)]]
    assert np.array_equal(tr.ids[0, :11].numpy(), want_ids[rest]) and np.array_equal(tr.boxes[0, :11].numpy(), want_boxes[rest])
    k0 = int(order[0])                                             # ... and another one from input frame 0
    sc["inst"][0][sc["owner"][0] == k0] = 7
    tr = run_tracker([sc], t_in)
    assert tr.count.tolist() == [10] and tr.lost == [[(int(ids[k0]), 0), (int(ids[k]), t)]]


def test_same_class_and_zero_nodes():
    H, W = 64, 96
    inst = np.zeros((1, 1, 3, H, W), np.int32)
    inst[0, 0, 0, 10:30, 10:40], inst[0, 0, 1:, 10:30, 10:40] = 11001, 12001          # same place, another class later
    inst[0, 0, :, 40:60, 50:90] = 13002
    d = dev(inst)
    tr = TR.track_instances(d, 1)
    assert tr.count.tolist() == [1] and tr.ids[0, 0].tolist() == [13002] * 3 and tr.lost == [[(11001, 1)]]
    tr = TR.track_instances(d, 1, same_class=False)
    assert tr.count.tolist() == [2] and tr.ids[0, 0].tolist() == [11001, 12001, 12001] and tr.lost == [[]]
    assert tr.boxes[0, 0].tolist() == [[10, 10, 40, 30]] * 3
    with pytest.raises(ValueError, match=r"sample 0 has no object with an id in \[11000, 12000\)"):
        TR.track_instances(d, 1, id_range=(11000, 12000))
    with pytest.raises(ValueError, match=r"sample 0 has no object"):
        TR.track_instances(torch.zeros(1, 1, 3, H, W, dtype=torch.int32, device=DEV), 1)
    with pytest.raises(ValueError, match="scale_factor"):
        TR.track_instances(d, 1, target_bw_of=torch.zeros(1, 2, 2, H // 2, W // 2, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        TR.track_instances(d, 1, target_bw_of=torch.zeros(1, 2, 2, H, W))


def test_more_than_64_objects_in_a_plane():
    H, W = 64, 320
    inst = np.zeros((2, 1, 2, H, W), np.int32)
    inst[:, 0, :, :4, :4] = 11001
    for k in range(70):                                           # 70 objects in target frame 1 of sample 1 only
        inst[1, 0, 1, 8 + (k // 20) * 8:12 + (k // 20) * 8, (k % 20) * 16:(k % 20) * 16 + 8] = 12000 + k
    with pytest.raises(ValueError, match=r"\[1\].*max_nodes=64"):
        TR.track_instances(dev(inst), 1)
    tr = TR.track_instances(dev(inst[:1]), 1)
    assert tr.count.tolist() == [1]
    with pytest.raises(ValueError, match="kernel cap"):
        TR.track_instances(dev(inst), 1, max_nodes=128)


# ------------------------------------------------------------------------------------------------ through the model
# last-input-frame rectangles (id, x0, y0, x1, y1) at 128x256; frame t sits (t - anchor) * step px away
RECTS = [[(11001, 20, 30, 60, 60, (2, 0)), (11004, 100, 40, 130, 90, (-1, 1)), (18999, 180, 70, 220, 100, (0, -2))],
         [(12005, 30, 20, 70, 50, (3, 1)), (17002, 150, 60, 200, 110, (-2, 0))]]
T_IN, T_OUT, SIZE = 2, 5, (128, 256)


def rect_at(r, t):
    i, x0, y0, x1, y1, (sx, sy) = r
    d = t - (T_IN - 1)
    return x0 + sx * d, y0 + sy * d, x1 + sx * d, y1 + sy * d


def raw_inputs(B, seed=0):
    """Decoded arrays as data.assemble_batch takes them, with consistently painted instance maps and the true flows."""
    rng = np.random.default_rng(seed)
    H, W = SIZE
    T = T_IN + T_OUT
    inst = rng.choice(np.array([0, 7, 24001], np.int32), (B, T, H, W))
    tflow, iflow = np.zeros((B, T_OUT, H, W, 2), np.float32), np.zeros((B, T_IN - 1, H, W, 2), np.float32)
    for b in range(B):
        for t in range(T):
            for r in RECTS[b]:
                x0, y0, x1, y1 = rect_at(r, t)
                inst[b, t, y0:y1, x0:x1] = r[0]
                sx, sy = r[5]
                if t >= T_IN:
                    tflow[b, t - T_IN, y0:y1, x0:x1] = (-sx * (t - T_IN + 1), -sy * (t - T_IN + 1))
                elif t < T_IN - 1:
                    iflow[b, t, y0:y1, x0:x1] = (sx, sy)
    return dict(frames=rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8), labels=rng.integers(0, 20, (B, T, H, W), dtype=np.uint8),
                inst=inst, tocc=rng.integers(0, 256, (B, T_OUT, H, W), dtype=np.uint8), tflow=tflow,
                iocc=rng.integers(0, 256, (B, T_IN - 1, H, W), dtype=np.uint8), iflow=iflow)


def tracker_file_graphs(B):
    """The same scene as tracker text lines (boxes x 8 = 2048x1024 pixels, exact), sorted by id -> scene_graph."""
    out = []
    for b in range(B):
        tracks = []
        for r in sorted(RECTS[b]):
            lines = [rect_at(r, t) for t in range(T_IN + T_OUT)]
            tracks.append([f"{a * 8},{c * 8},{(e - a) * 8},{(f - c) * 8},0.9,{r[0]}" for a, c, e, f in lines])
        out.append(G.scene_graph(tracks, SIZE, T_IN, T_IN + T_OUT))
    return out


def small_model(train, seed=0):
    cfg = normalize_config(default_config(num_input_frames=T_IN, block_expansion=4, max_expansion=32, h_dim=32, z_dim=16,
                                          out_channel=16, ndf=4, use_image_discriminator=False,
                                          use_video_discriminator=False))
    torch.manual_seed(seed)
    model = GeneratorFullModel(train_params=copy.deepcopy(cfg["train_params"]), model_params=copy.deepcopy(cfg["model_params"]),
                               dataset="cityscapes", is_inference=not train)
    return (model.to(DEV).train() if train else model.to(DEV).eval()), cfg


def test_tracked_batch_equals_the_tracker_file_batch_through_the_model():
    B = 2
    raw = {k: dev(v) for k, v in raw_inputs(B).items()}
    model, cfg = small_model(train=True)
    files = tracker_file_graphs(B)
    ref_graph = G.collate_graphs([g for _, g in files])
    want = D.assemble_batch(raw["frames"], raw["labels"], raw["inst"], raw["tocc"], raw["tflow"], ref_graph.to(DEV), raw["iocc"],
                            raw["iflow"])
    got = TR.tracked_batch(raw["frames"], raw["labels"], raw["inst"], raw["tocc"], raw["tflow"], T_IN, raw["iocc"], raw["iflow"],
                           config=cfg)
    assert got["tracks"].count.tolist() == [3, 2] and got["tracks"].lost == [[], []]
    for k in FIELDS + ("batch", "ptr"):
        x, y = getattr(got["tracking_gnn"], k), getattr(ref_graph, k)
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y), k
    mask = torch.stack([G.tracking_mask(want["instance_mask"][b], files[b][0]) for b in range(B)], 0)
    assert torch.equal(got["tracking_mask"], mask) and mask.any() and tuple(mask.shape) == (B, 1, T_IN + T_OUT, *SIZE)
    for k in ("video", "bg_mask", "fg_mask", "instance_mask", "target_bw_of", "target_bw_occ", "input_of", "input_occ"):
        assert torch.equal(got[k], want[k]), k
    rng = {k: v.to(DEV) for k, v in make_step_rng(want, z_dim=16, latent_dim=32, seed=0).items()}
    outs = []
    for batch in (want, got):
        batch = dict(batch, rng=rng)
        with torch.no_grad():
            out, losses, _, _ = model(batch)
        torch.cuda.synchronize()
        outs.append((out, losses))
    assert set(outs[0][1]) == set(outs[1][1]) and outs[0][1]
    for k in outs[0][1]:
        assert torch.equal(torch.as_tensor(outs[0][1][k]), torch.as_tensor(outs[1][1][k])), k
    for k in ("generated", "sparse_motion_bin", "sparse_motion_bw"):
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k


def test_click_to_move_with_ids_that_change_between_the_input_frames():
    B = 2
    batch = batch_to(make_batch(B, 128, 256, T_IN, seed=0), DEV)
    raw = raw_inputs(B)
    steady = raw["inst"][:, None, :T_IN].copy()
    swapped = steady.copy()
    f0 = steady[:, 0, 0]
    swapped[:, 0, 0][f0 == 11001], swapped[:, 0, 0][f0 == 11004] = 11004, 11001         # two objects trade ids in frame 0
    swapped[:, 0, 0][f0 == 17002] = 17950                                               # and one carries a new id there
    drags = [I.Drag(0, 110, 60, 120, 55), I.Drag(1, 40, 30, 25, 35)]
    model, _ = small_model(train=False)
    z_m = torch.randn(B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(5))
    iof = dev(raw["iflow"]).permute(0, 4, 1, 2, 3).contiguous()                          # [B,2,t_in-1,H,W]: the true motion
    runs = []
    for maps, kw in ((steady, dict()), (swapped, dict(track=True)), (steady, dict(track=dict(min_iou=(1, 3))))):
        torch.manual_seed(11)
        runs.append(I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], dev(maps), drags, iof,
                                    batch["input_occ"], z_m=z_m, **kw))
        torch.cuda.synchronize()
    for other in runs[1:]:
        assert set(other) == set(runs[0])
        for k in runs[0]:
            assert torch.equal(other[k], runs[0][k]), k
    with pytest.raises(ValueError, match="not an object of every input frame"):          # without it the swapped ids are refused
        I.click_to_move(model, batch["video"], batch["bg_mask"], batch["fg_mask"], dev(swapped), [I.Drag(1, 160, 70, 150, 80)],
                        iof, batch["input_occ"], z_m=z_m)
