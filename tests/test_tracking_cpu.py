"""Host side of tracking from instance maps (c2m_amd.tracking): the match rule against a NumPy restatement, scene_graphs against
the tracker-file arithmetic, the refusals, and the scenes of the GPU tests checked with the NumPy pipeline.  No GPU needed."""
import numpy as np
import pytest
import torch

from c2m_amd import _lib, graph as G, interactive as I, ops, tracking as TR
from c2m_amd.config import default_config, normalize_config
import tracking_np as NP

FIELDS = ("x", "y", "source_frames_nodes_roi", "source_frames_nodes_roi_padded", "target_frames_nodes_roi",
          "source_frames_nodes_instance_ids", "target_frames_nodes_instance_ids", "targets_barycenter",
          "targets_displacement", "targets_theta", "num_real_nodes", "edge_index")


# ------------------------------------------------------------------------------------------------ the match rule
def _both(pairs, ref_ids, frame_ids, **kw):
    got = TR.match_host(pairs, ref_ids, frame_ids, **kw)
    assert np.array_equal(got, NP.np_match(pairs, np.asarray(ref_ids), np.asarray(frame_ids), **kw))
    return got.tolist()


def test_match_rule_plain_and_empty():
    # two objects that swapped ids; the last row / column are the pixels without a slot
    assert _both([[90, 2, 8], [0, 50, 10], [5, 5, 1000]], [11001, 11002], [11001, 11002]) == [0, 1]
    assert _both([[0, 0, 9], [0, 0, 4], [3, 7, 100]], [11001, 11002], [11001, 11002]) == [-1, -1]       # nothing overlaps
    assert _both([[500]], [], []) == []                                                                 # an empty plane
    assert _both([[0, 0, 500]], [], [11001, 11002]) == []
    assert _both([[7], [500]], [11001], []) == [-1]


def test_match_rule_tie_goes_to_the_lower_id():
    # ref 0 overlaps frame 0 and frame 1 with the same IoU (30 / (60 + 40 - 30)); ref 1 and frame 1 are left to each other
    pairs = [[30, 30, 0], [0, 5, 35], [10, 5, 0]]
    assert _both(pairs, [11001, 11002], [11001, 11002]) == [0, -1]
    # mirrored: two refs tie for one frame object, the lower ref wins and the other ref stays unlinked
    pairs = [[30, 0, 10], [30, 5, 5], [0, 35, 0]]
    assert _both(pairs, [11001, 11002], [11001, 11002], min_iou=(1, 100)) == [0, -1]


def test_match_rule_class_mismatch():
    pairs = [[80, 0, 0], [0, 60, 0], [0, 0, 10]]
    assert _both(pairs, [11001, 12001], [11007, 13001]) == [0, -1]
    assert _both(pairs, [11001, 12001], [11007, 13001], same_class=False) == [0, 1]


def test_match_rule_best_but_not_mutual():
    # frame 0 is ref 1's best, but frame 0's best is ref 0; ref 1 does not fall back to its second choice
    pairs = [[60, 0, 0], [30, 8, 12], [0, 2, 0]]
    assert _both(pairs, [11001, 11002], [11001, 11002], min_iou=(1, 100)) == [0, -1]


def test_match_rule_min_iou_boundary():
    pairs = [[25, 35], [40, 0]]                       # n = 25, r = 60, a = 65: IoU = 25 / 100 exactly
    assert _both(pairs, [11001], [11001], min_iou=(1, 4)) == [0]
    assert _both(pairs, [11001], [11001], min_iou=(26, 100)) == [-1]
    assert _both(pairs, [11001], [11001], min_iou=(25, 100)) == [0]
    assert _both([[24, 36], [40, 0]], [11001], [11001], min_iou=(1, 4)) == [-1]


def test_match_rule_random_tables():
    rng = np.random.default_rng(0)
    for k in range(40):
        nr, nf = rng.integers(0, 7, 2)
        pairs = rng.integers(0, 6, (nr + 1, nf + 1)) * rng.integers(0, 2, (nr + 1, nf + 1))      # many zeros and ties
        ref_ids = np.sort(rng.choice(np.arange(11000, 13000, 250), nr, replace=False))
        frame_ids = np.sort(rng.choice(np.arange(11000, 13000, 250), nf, replace=False))
        _both(pairs, ref_ids, frame_ids, min_iou=(1, 4), same_class=bool(k % 2))


# ------------------------------------------------------------------------------------------------ track-file equivalence
@pytest.mark.parametrize("t_in", [1, 2])
@pytest.mark.parametrize("lambda_traj", [1, 3])
def test_scene_graphs_equal_the_track_file_arithmetic(t_in, lambda_traj):
    size, T = (128, 256), 7
    scenes = [NP.fixture_boxes(p, T, size) for p in ("aachen_000000_000019_", "bonn_000001_000004_")]
    M = 64
    tr = TR.Tracks(torch.zeros(2, M, T, dtype=torch.int32), torch.zeros(2, M, T, 4, dtype=torch.int32),
                   torch.zeros(2, dtype=torch.int32), [[], []])
    for b, (edges, ids) in enumerate(scenes):
        n = len(ids)
        tr.ids[b, :n] = torch.from_numpy(np.repeat(ids[:, None], T, 1) + np.arange(T)[None])      # an id per frame
        tr.boxes[b, :n] = torch.from_numpy(edges)
        tr.count[b] = n
    tids, graphs = TR.scene_graphs(tr, size, t_in, lambda_traj)
    for b, (edges, ids) in enumerate(scenes):
        want_ids, want = G.scene_graph_from_boxes(I.edges_to_tracker(edges, size), np.repeat(ids[:, None], T, 1) + np.arange(T)[None],
                                                  size, t_in, T, lambda_traj)
        assert torch.equal(tids[b], want_ids)
        for k in FIELDS:
            x, y = getattr(graphs[b], k), getattr(want, k)
            assert x.dtype == y.dtype and torch.equal(x, y), k


# ------------------------------------------------------------------------------------------------ the scenes of the GPU tests
@pytest.mark.parametrize("kind,arg,t_in", NP.SCENES)
def test_numpy_pipeline_recovers_every_object_of_the_scenes(kind, arg, t_in):
    edges, ids, sc = NP.make_scene(kind, arg, t_in)
    got_ids, got_boxes, lost = NP.np_track(sc["inst"], t_in, sc["target_flow"], sc["input_flow"])
    want_ids, want_boxes = NP.painted_extents(sc)
    order = np.argsort(ids)
    assert lost == [] and len(got_ids) == len(ids)
    assert np.array_equal(got_ids, want_ids[order]) and np.array_equal(got_boxes, want_boxes[order])
    if kind == "constructed":
        assert (sc["frame_ids"] != sc["frame_ids"][:, t_in - 1:t_in]).any()      # the ids do change from frame to frame


def test_numpy_pipeline_under_trouble():
    edges, ids, sc = NP.make_scene("constructed", 12, 2)
    want = NP.np_track(sc["inst"], 2, sc["target_flow"], sc["input_flow"])
    rng = np.random.default_rng(1)
    jitter = lambda f: f + rng.integers(-1, 2, f.shape).astype(np.float32)
    got = NP.np_track(sc["inst"], 2, jitter(sc["target_flow"]), jitter(sc["input_flow"]))
    assert got[2] == [] and np.array_equal(got[0], want[0])


# ------------------------------------------------------------------------------------------------ refusals
def test_abi_declares_and_binds_the_link_entries():
    for name in ("c2m_instance_link_max_nodes", "c2m_instance_slots", "c2m_instance_overlap", "c2m_instance_match"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS


def test_no_cpu_path_and_dtypes():
    inst = torch.zeros(1, 3, 8, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        TR.track_instances(inst, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.instance_slots(torch.zeros(1, 18000, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.instance_overlap(torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8, dtype=torch.int32), None,
                             torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                             torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.instance_match(torch.zeros(1, 65, 65, dtype=torch.int32), torch.zeros(1, 64, dtype=torch.int32),
                           torch.zeros(1, dtype=torch.int32), torch.zeros(1, 64, dtype=torch.int32),
                           torch.zeros(1, dtype=torch.int32))


def test_scale_factor_is_refused():
    cfg = normalize_config(default_config(num_input_frames=2))
    TR.check_config(cfg)
    cfg["model_params"]["common_params"]["scale_factor"] = 0.5
    with pytest.raises(ValueError, match="scale_factor = 0.5"):
        TR.check_config(cfg)
    with pytest.raises(ValueError, match="scale_factor = 0.5"):           # before anything touches the (CPU) arrays
        TR.tracked_batch(None, None, None, None, None, 2, config=cfg)


def test_zero_nodes_is_refused_by_scene_graphs():
    tr = TR.Tracks(torch.zeros(2, 4, 7, dtype=torch.int32), torch.zeros(2, 4, 7, 4, dtype=torch.int32),
                   torch.tensor([1, 0], dtype=torch.int32), [[], [(11001, 3)]])
    tr.ids[0, 0], tr.boxes[0, 0] = 11001, torch.tensor([2, 2, 10, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="sample 1 has no object"):
        TR.scene_graphs(tr, (128, 256), 2)


def _links(B=2, M=4, T=3):
    ids = torch.zeros(B, M, T, dtype=torch.int32)
    edges = torch.zeros(B, M, T, 4, dtype=torch.int32)
    valid = torch.zeros(B, M, T, dtype=torch.bool)
    count, overflow = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, T, dtype=torch.int32)
    for b in range(B):
        for s in range(2):
            ids[b, s] = torch.tensor([11001 + s, 11005 + s, 11009 - s])
            edges[b, s] = torch.tensor([4 * s, 2, 4 * s + 3, 9])
            valid[b, s] = True
        count[b] = 2
    return ids, edges, valid, count, overflow


def test_lost_objects_zero_nodes_and_overflow():
    ids, edges, valid, count, overflow = _links()
    tr = TR.tracks_from_links(ids, edges, valid, count, overflow, 2)
    assert tr.count.tolist() == [2, 2] and tr.lost == [[], []]
    assert torch.equal(tr.ids[:, :2], ids[:, :2]) and not tr.ids[:, 2:].any() and torch.equal(tr.boxes[:, :2], edges[:, :2])
    valid[1, 0, 2] = False                                    # sample 1 loses its first object in target frame 2
    valid[0, 1, 0] = False                                    # sample 0 loses its second object in input frame 0
    tr = TR.tracks_from_links(ids, edges, valid, count, overflow, 2)
    assert tr.count.tolist() == [1, 1] and tr.lost == [[(11006, 0)], [(11005, 2)]]
    assert tr.ids[0, 0].tolist() == [11001, 11005, 11009] and tr.ids[1, 0].tolist() == [11002, 11006, 11008]
    assert not tr.ids[:, 1:].any() and not tr.boxes[:, 1:].any()
    valid[1, 1, 1] = False                                    # nothing is left of sample 1 (frame 1 is the anchor's own)
    valid[1, 1, 2] = False
    with pytest.raises(ValueError, match=r"sample 1 has no object with an id in \[1000, 19000\)"):
        TR.tracks_from_links(ids, edges, valid, count, overflow, 2)
    overflow[1, 2] = 1
    with pytest.raises(ValueError, match=r"\[1\].*max_nodes=4"):
        TR.tracks_from_links(ids, edges, valid, count, overflow, 2)


def test_wrong_dtypes_and_flows_not_at_frame_size():
    inst = torch.zeros(2, 1, 7, 16, 32, dtype=torch.int32)
    with pytest.raises(TypeError, match="integer ids"):
        TR.track_instances(inst.float(), 2)
    with pytest.raises(ValueError, match=r"target_bw_of is \(8, 16\) but the maps are \(16, 32\).*scale_factor"):
        TR.track_instances(inst, 2, target_bw_of=torch.zeros(2, 2, 5, 8, 16))
    with pytest.raises(ValueError, match=r"input_of is \(8, 16\) but the maps are \(16, 32\)"):
        TR.track_instances(inst, 2, input_of=torch.zeros(2, 2, 1, 8, 16))
    with pytest.raises(TypeError, match="target_bw_of must be fp32"):
        TR.track_instances(inst, 2, target_bw_of=torch.zeros(2, 2, 5, 16, 32, dtype=torch.float64))
    with pytest.raises(ValueError, match="input_of must be"):
        TR.track_instances(inst, 2, input_of=torch.zeros(2, 2, 3, 16, 32))
    with pytest.raises(ValueError, match="min_pixels and max_nodes"):
        TR.track_instances(inst, 2, min_pixels=0)
    with pytest.raises(RuntimeError, match="HIP device"):      # everything else is in order: only the device is wrong
        TR.track_instances(inst, 2, torch.zeros(2, 2, 5, 16, 32), torch.zeros(2, 2, 1, 16, 32))
