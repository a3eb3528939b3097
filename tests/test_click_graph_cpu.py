"""Host side of click-to-move (c2m_amd.interactive): the tracker-file graph split into parse_tracks +
scene_graph_from_boxes, the drag -> future-box conversion and the validation errors.  No GPU needed."""
import glob
import os

import numpy as np
import pytest
import torch

from c2m_amd import graph as G
from c2m_amd import interactive as I
from golden_io import GOLDEN

TRACKS = os.path.join(GOLDEN, "scene_tracks")
FIELDS = ("x", "y", "source_frames_nodes_roi", "source_frames_nodes_roi_padded", "target_frames_nodes_roi",
          "source_frames_nodes_instance_ids", "target_frames_nodes_instance_ids", "targets_barycenter",
          "targets_displacement", "targets_theta", "num_real_nodes", "edge_index")


def _prefixes():
    names = sorted({os.path.basename(p).rsplit("_", 1)[0] + "_" for p in glob.glob(os.path.join(TRACKS, "*.txt"))})
    assert names, "no committed track fixtures"
    return names


def _tracks(prefix):
    return [open(p).read().splitlines() for p in sorted(glob.glob(os.path.join(TRACKS, prefix) + "*.txt"))]


def _same_graph(a, b):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k


@pytest.mark.parametrize("t_in", [1, 2])
@pytest.mark.parametrize("lambda_traj", [1, 3])
def test_scene_graph_from_boxes_is_scene_graph(t_in, lambda_traj):
    for prefix in _prefixes():
        tracks = _tracks(prefix)
        ids_a, a = G.scene_graph(tracks, (128, 256), t_in, 7, lambda_traj)
        box, ids = G.parse_tracks(tracks, 7)
        ids_b, b = G.scene_graph_from_boxes(box, ids, (128, 256), t_in, 7, lambda_traj)
        assert torch.equal(ids_a, ids_b)
        _same_graph(a, b)


def test_scene_graph_from_boxes_checks_shapes():
    box = np.zeros((2, 7, 4))
    with pytest.raises(ValueError):
        G.scene_graph_from_boxes(box, np.zeros((2, 6), np.int64), (128, 256), 2, 7)
    with pytest.raises(ValueError):
        G.scene_graph_from_boxes(box, np.zeros((2, 7), np.int64), (128, 256), 2, 6)
    with pytest.raises(ValueError):
        G.scene_graph_from_boxes(np.zeros((0, 7, 4)), np.zeros((0, 7), np.int64), (128, 256), 2, 7)


def test_linear_drag_displacements():
    d = I.Drag(0, 10, 20, 20, 15)
    got = d.displacements(5)
    want = np.array([[2, -1], [4, -2], [6, -3], [8, -4], [10, -5]], dtype=np.float64)
    assert np.array_equal(got, want)
    assert np.array_equal(d.scales(5), np.ones(5))


def test_path_and_scale():
    path = [(11, 20), (13, 21), (13, 23), (12, 25), (10, 26)]
    d = I.Drag(0, 10, 20, path=path, scale=[1, 1.5, 2, 1, 0.5])
    assert np.array_equal(d.displacements(5), np.asarray(path, np.float64) - [10, 20])
    fut = I.future_edges([4, 8, 12, 16], d.displacements(5), d.scales(5))
    # centre (8, 12), half size (4, 4): frame 1 moves by (3, 1) and scales by 1.5
    assert np.array_equal(fut[1], [11 - 6, 13 - 6, 11 + 6, 13 + 6])
    assert np.array_equal(fut[4], [8 - 2, 18 - 2, 8 + 2, 18 + 2])


def _one_sample(ids=(11001, 12002), last_edges=((10, 20, 30, 40), (100, 50, 120, 70)), t_in=2):
    N = len(ids)
    edges = np.zeros((1, 4, t_in, 4), np.int32)
    for n, e in enumerate(last_edges):
        edges[0, n, :] = e
    idv = np.zeros((1, 4), np.int32)
    idv[0, :N] = ids
    return idv, edges, np.array([N], np.int32)


def test_zero_drag_is_identity_theta():
    ids, edges, count = _one_sample()
    drag = I.Drag(0, 15, 25, 15, 25)
    g, click = I.graph_from_boxes(ids, edges, count, [drag], [11001], (128, 256), 2, 5)
    assert click.tolist() == [0]
    ident = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32).expand(2, 5, 6)
    assert torch.equal(g.targets_theta, ident)
    assert torch.equal(g.targets_displacement, torch.zeros(2, 5, 2))


def test_drag_theta_and_graph_fields():
    ids, edges, count = _one_sample()
    g, click = I.graph_from_boxes(ids, edges, count, [I.Drag(0, 110, 60, 90, 70)], [12002], (128, 256), 2, 5)
    assert click.tolist() == [1] and g.num_nodes == 2 and g.edge_index.tolist() == [[0, 1], [1, 0]]
    th = g.targets_theta.double()
    assert torch.equal(g.targets_theta[0], torch.tensor([1, 0, 0, 0, 1, 0.]).expand(5, 6))   # the other object stays
    for t in range(5):
        dx, dy = -20 * (t + 1) / 5, 10 * (t + 1) / 5
        want = [1, 0, -2 * dx / 256, 0, 1, -2 * dy / 128]                 # bary(last) - bary(t), in [-1, 1] units
        assert np.allclose(th[1, t].numpy(), want, atol=1e-7, rtol=0), t
    # boxes at the working size: [x_l, x_r, y_t, y_b]
    assert g.source_frames_nodes_roi[1, 1].tolist() == [100, 120, 50, 70]
    assert g.target_frames_nodes_roi[1, 4].tolist() == [80, 100, 60, 80]
    assert g.source_frames_nodes_instance_ids[:, 0].tolist() == [11001, 12002]
    assert g.target_frames_nodes_instance_ids.shape == (2, 5)


def test_scale_theta():
    ids, edges, count = _one_sample()
    drag = I.Drag(0, 15, 25, 15, 25, scale=[2] * 5)
    g, _ = I.graph_from_boxes(ids, edges, count, [drag], [11001], (128, 256), 2, 5)
    assert torch.equal(g.targets_theta[0], torch.tensor([0.5, 0, 0, 0, 0.5, 0]).expand(5, 6))


def test_two_samples_and_two_drags():
    ids, edges, count = _one_sample()
    ids2, edges2, count2 = np.concatenate([ids, ids]), np.concatenate([edges, edges]), np.concatenate([count, count])
    drags = [I.Drag(1, 110, 60, 100, 60), I.Drag(1, 15, 25, 20, 25), I.Drag(0, 15, 25, 15, 30)]
    g, click = I.graph_from_boxes(ids2, edges2, count2, drags, [12002, 11001, 11001], (128, 256), 2, 5)
    assert click.tolist() == [3, 2, 0] and g.batch.tolist() == [0, 0, 1, 1]


def test_single_object_keeps_the_self_edge():
    ids, edges, count = _one_sample(ids=(11001,), last_edges=((10, 20, 30, 40),))
    g, _ = I.graph_from_boxes(ids, edges, count, [I.Drag(0, 15, 25, 20, 25)], [11001], (128, 256), 2, 5)
    assert g.edge_index.tolist() == [[0], [0]]


def test_validation_errors():
    ids, edges, count = _one_sample()
    args = ((128, 256), 2, 5)
    with pytest.raises(ValueError, match=r"pixel \(x=3, y=4\).*id 0"):                      # background
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 3, 4, 10, 10)], [0], *args)
    with pytest.raises(ValueError, match=r"id 26001.*outside"):                            # class 26 is not an object class
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 3, 4, 10, 10)], [26001], *args)
    with pytest.raises(ValueError, match="id 13003"):                                     # in range, not in every frame
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 3, 4, 10, 10)], [13003], *args)
    with pytest.raises(ValueError, match="path"):
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 15, 25, path=[(1, 1)] * 4)], [11001], *args)
    with pytest.raises(ValueError, match="sample 1"):
        I.graph_from_boxes(ids, edges, count, [I.Drag(1, 15, 25, 10, 10)], [11001], *args)
    with pytest.raises(ValueError, match="outside"):
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 256, 25, 10, 10)], [11001], *args)
    with pytest.raises(ValueError, match="scale"):
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 15, 25, 10, 10, scale=[1, 1, 0, 1, 1])], [11001], *args)
    with pytest.raises(ValueError, match="two drags"):
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 15, 25, 10, 10), I.Drag(0, 12, 22, 1, 1)], [11001, 11001],
                           *args)
    with pytest.raises(ValueError, match="to_x"):
        I.graph_from_boxes(ids, edges, count, [I.Drag(0, 15, 25)], [11001], *args)


def test_instance_boxes_has_no_cpu_path():
    from c2m_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.instance_boxes(torch.zeros(1, 2, 8, 8, dtype=torch.int32), 2)
