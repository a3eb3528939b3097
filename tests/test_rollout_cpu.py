"""Host logic of the rollout (no GPU): the drag-error arithmetic, the box table, the input assembly of a continuation on CPU
tensors with the warp stubbed, argument validation, and the C ABI entry of the label warp."""
import types

import numpy as np
import pytest
import torch

from c2m_amd import _lib, interactive as I, ops

T = 5


def _target(start, to, sample=0, node=0):
    d = I.Drag(sample, (start[0] + start[2]) / 2, (start[1] + start[3]) / 2, to[0], to[1])
    return I.drag_targets([d], [(sample, node)], np.asarray(start, np.float64).reshape(1, 1, 1, 4).repeat(sample + 1, 0)
                          .repeat(node + 1, 1), 1, T)[0]


def test_drag_targets_are_the_boxes_the_graph_is_built_from():
    t = _target((100, 40, 130, 90), (125, 60))                       # centre (115, 65) -> (125, 60)
    assert t.start.tolist() == [100, 40, 130, 90]
    assert t.edges.tolist() == [[100 + 2 * k, 40 - k, 130 + 2 * k, 90 - k] for k in range(1, T + 1)]
    d = I.Drag(0, 1, 1, 2, 2, scale=[1, 1, 1, 1, 2])
    e = I.drag_targets([d], [(0, 0)], np.array([[[[0, 0, 10, 20]]]]), 1, T)[0].edges
    assert e[-1].tolist() == [6 - 10, 11 - 20, 6 + 10, 11 + 20]


def test_drag_error_arithmetic():
    tg = _target((100, 40, 130, 90), (125, 60), node=1)
    boxes = np.zeros((1, 2, T, 4), np.int64)
    presence = np.ones((1, 2, T), bool)
    boxes[0, 1] = tg.edges                                            # exactly where it was asked to be
    err = I.drag_error([tg], boxes, presence)
    assert err["distance"].tolist() == [[0.0] * T] and err["normalized"].tolist() == [0.0]
    assert err["displacement"][0] == np.sqrt(125.0)
    boxes[0, 1] = tg.edges + np.array([3, 4, 3, 4])                   # 5 px off in every frame
    boxes[0, 1, 2] = tg.edges[2] + np.array([0, 0, 12, 0])            # 12 px wider: the centre is 6 px off
    err = I.drag_error([tg], boxes, presence)
    assert err["distance"].tolist() == [[5.0, 5.0, 6.0, 5.0, 5.0]]
    assert err["normalized"][0] == 5.0 / (np.sqrt(125.0) + 1e-6)
    # torch tensors are accepted as well (predicted_boxes returns them)
    err_t = I.drag_error([tg], torch.from_numpy(boxes), torch.from_numpy(presence))
    assert err_t["distance"].tolist() == err["distance"].tolist()


def test_drag_error_zero_displacement_and_absent_object():
    still = _target((10, 10, 20, 30), (15, 20))                       # dragged onto its own centre: displacement 0
    boxes = np.zeros((1, 1, T, 4), np.int64)
    boxes[0, 0] = still.edges + np.array([0, 2, 0, 2])
    presence = np.ones((1, 1, T), bool)
    err = I.drag_error([still], boxes, presence)
    assert err["displacement"].tolist() == [0.0]
    assert err["normalized"][0] == 2.0 / (1 + 1e-6)                   # divisor 1 when the displacement is 0, plus 1e-6
    presence[0, 0, 1] = presence[0, 0, -1] = False                    # gone in two frames: nan there, never 0
    err = I.drag_error([still], boxes, presence)
    assert np.isnan(err["distance"][0, [1, 4]]).all() and err["distance"][0, [0, 2, 3]].tolist() == [2.0, 2.0, 2.0]
    assert np.isnan(err["normalized"][0])
    assert I.drag_error([], boxes, presence)["distance"].shape == (0, T)
    with pytest.raises(ValueError, match="frames"):
        I.drag_error([still], boxes[:, :, :3], presence[:, :, :3])


def test_boxes_from_stats():
    big = 2 ** 31 - 1
    rows = torch.tensor([[[12, 3, 9, 4, 7], [0, big, -1, big, -1]], [[1, 0, 0, 5, 5], [2, 254, 255, 0, 127]]], dtype=torch.int32)
    boxes, presence = I.boxes_from_stats(rows)
    assert presence.tolist() == [[True, False], [True, True]]
    assert boxes.tolist() == [[[3, 4, 10, 8], [0, 0, 0, 0]], [[0, 5, 1, 6], [254, 0, 256, 128]]]
    assert boxes.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ the continuation
def _fake_model(t_in, scale_factor=1, flow_channel=2):
    return types.SimpleNamespace(
        train_params=dict(num_input_frames=t_in, num_predicted_frames=T, input_size=[8, 16]),
        model_params=dict(common_params=dict(scale_factor=scale_factor, flow_channel=flow_channel, occlusion_channel=1)))


def _prev(B, t_total, H=8, W=16):
    """Inputs whose every frame can be told apart: frame t of the video is t everywhere, the id map holds 11000 + t."""
    frames = torch.arange(t_total, dtype=torch.float32).view(1, 1, t_total, 1, 1)
    sem = torch.zeros(B, 20, t_total, H, W)
    sem[:, 3] = 1.0
    return dict(video=frames.expand(B, 3, t_total, H, W).clone(), bg_mask=sem[:, :11].clone(), fg_mask=sem[:, 11:].clone(),
                instance_mask=(11000 + frames).expand(B, 1, t_total, H, W).to(torch.int64))


def _stub_label_warp(calls):
    def label_warp(flow, planes_f=None, planes_i=None, occ=None, threshold=None, fill_id=0):
        calls.append(dict(flow=flow, planes_f=planes_f, planes_i=planes_i, occ=occ, threshold=threshold, fill_id=fill_id))
        Tn = flow.shape[2]
        step = torch.arange(Tn).view(1, 1, Tn, 1, 1)
        return planes_f.unsqueeze(2).repeat(1, 1, Tn, 1, 1), planes_i.unsqueeze(2) + 100 * (step + 1).to(torch.int32)
    return label_warp


def _out(B, H=8, W=16):
    gen = 100 + torch.arange(T, dtype=torch.float32).view(1, 1, T, 1, 1)
    return dict(generated=gen.expand(B, 3, T, H, W).clone(), dense_motion_bw=torch.zeros(B, 2, T, H, W),
                sparse_motion_bw=torch.ones(B, 2, T, H, W), occlusion_bw=torch.full((B, 1, T, H, W), 0.25),
                sparse_occ_bw=torch.full((B, 1, T, H, W), 0.75))


@pytest.mark.parametrize("t_in", [1, 2, 7])
def test_input_assembly_of_a_continuation(monkeypatch, t_in):
    B = 2
    calls = []
    monkeypatch.setattr(ops, "label_warp", _stub_label_warp(calls))
    prev, out = _prev(B, t_in + 3), _out(B)                            # frames past t_in are never read
    maps = I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], t_in)
    c = calls[0]
    assert c["flow"] is out["dense_motion_bw"] and c["occ"] is None and c["threshold"] is None
    assert c["planes_f"].shape == (B, 20, 8, 16) and c["planes_f"][:, 3].eq(1).all() and c["planes_f"].sum() == B * 8 * 16
    assert c["planes_i"].dtype == torch.int32 and c["planes_i"].eq(11000 + t_in - 1).all()      # the LAST input frame only
    assert maps["bg_mask"].shape == (B, 11, T, 8, 16) and maps["fg_mask"].shape == (B, 9, T, 8, 16)
    assert maps["instance_mask"].shape == (B, 1, T, 8, 16) and maps["instance_mask"].dtype == torch.int32
    I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"][:, 0], t_in, flow="sparse_motion_bw",
                     occ_threshold=0.5, fill_id=3)
    c = calls[1]
    assert c["flow"] is out["sparse_motion_bw"] and c["occ"] is out["sparse_occ_bw"] and c["threshold"] == 0.5 and c["fill_id"] == 3
    I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], t_in, occ_threshold=0.1)
    assert calls[2]["occ"] is out["occlusion_bw"]

    seen = []
    flow_fn = lambda a, b: (seen.append((float(a.mean()), float(b.mean()))) or torch.full((B, 2, 8, 16), float(b.mean() - a.mean())),
                            torch.full((B, 1, 8, 16), float(a.mean())))
    nxt = I.next_inputs(prev, out, maps, t_in, flow_fn if t_in > 1 else None, needs_flows=t_in > 1)
    # the last t_in frames of (the t_in input frames, then the T predicted ones)
    seq = [float(t) for t in range(t_in)] + [100.0 + t for t in range(T)]
    ids = [11000 + t for t in range(t_in)] + [11000 + t_in - 1 + 100 * (t + 1) for t in range(T)]
    assert nxt["video"].shape == (B, 3, t_in, 8, 16) and nxt["video"][0, 0, :, 0, 0].tolist() == seq[-t_in:]
    assert nxt["instance_mask"].shape == (B, 1, t_in, 8, 16) and nxt["instance_mask"].dtype == torch.int32
    assert nxt["instance_mask"][1, 0, :, 0, 0].tolist() == ids[-t_in:]                            # ids persist as values
    assert nxt["bg_mask"].shape == (B, 11, t_in, 8, 16) and nxt["fg_mask"].shape == (B, 9, t_in, 8, 16)
    assert nxt["bg_mask"][:, 3].eq(1).all()
    if t_in == 1:
        assert nxt["input_of"] is None and nxt["input_occ"] is None and not seen
    else:
        s = seq[-t_in:]
        assert nxt["input_of"].shape == (B, 2, t_in - 1, 8, 16) and nxt["input_occ"].shape == (B, 1, t_in - 1, 8, 16)
        # flow of (i -> i + 1), occlusion of the reverse pair
        assert nxt["input_of"][0, 0, :, 0, 0].tolist() == [s[i + 1] - s[i] for i in range(t_in - 1)]
        assert nxt["input_occ"][0, 0, :, 0, 0].tolist() == [s[i + 1] for i in range(t_in - 1)]
        with pytest.raises(ValueError, match="flow_fn"):
            I.next_inputs(prev, out, maps, t_in, None, needs_flows=True)
        assert I.next_inputs(prev, out, maps, t_in, None, needs_flows=False)["input_of"] is None


def test_continue_calls_click_to_move_on_the_assembled_inputs(monkeypatch):
    B, t_in = 1, 2
    monkeypatch.setattr(ops, "label_warp", _stub_label_warp([]))
    got = {}

    def click_to_move(model, video, bg_mask, fg_mask, instance_mask, drags, input_of=None, input_occ=None, z_m=None, **kw):
        got.update(video=video, instance_mask=instance_mask, drags=drags, input_of=input_of, z_m=z_m, kw=kw)
        return "out"
    monkeypatch.setattr(I, "click_to_move", click_to_move)
    prev, out = _prev(B, t_in), _out(B)
    flow_fn = lambda a, b: (torch.zeros(B, 2, 8, 16), torch.ones(B, 1, 8, 16))
    drags = [I.Drag(0, 1, 1, 2, 2)]
    res, nxt = I.continue_click_to_move(_fake_model(t_in), prev, out, drags, flow_fn=flow_fn, z_m="z", min_pixels=4)
    assert res == "out" and got["video"] is nxt["video"] and got["instance_mask"] is nxt["instance_mask"]
    assert got["drags"] is drags and got["z_m"] == "z" and got["kw"] == dict(min_pixels=4)
    assert got["input_of"].shape == (B, 2, 1, 8, 16)
    assert got["video"][0, 0, :, 0, 0].tolist() == [103.0, 104.0]
    with pytest.raises(ValueError, match="flow_fn"):
        I.continue_click_to_move(_fake_model(t_in), prev, out, drags)
    # a model that was built without flow channels reads no input-frame flows
    I.continue_click_to_move(_fake_model(t_in, flow_channel=-1), prev, out, drags)
    assert got["input_of"] is None


def test_argument_validation():
    prev, out = _prev(1, 1), _out(1)
    for sf in (0.5, 2, [64, 128]):
        with pytest.raises(ValueError, match="scale_factor"):
            I.continue_click_to_move(_fake_model(1, scale_factor=sf), prev, out, [])
        with pytest.raises(ValueError, match="scale_factor"):
            I.rollout(_fake_model(1, scale_factor=sf), prev["video"], prev["bg_mask"], prev["fg_mask"], prev["instance_mask"],
                      [[], []])
    with pytest.raises(ValueError, match="at least one segment"):
        I.rollout(_fake_model(1), prev["video"], prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], [])
    with pytest.raises(ValueError, match="motion codes"):
        I.rollout(_fake_model(1), prev["video"], prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], [[], []], z_m=[None])
    with pytest.raises(ValueError, match="flow must be one of"):
        I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], 1, flow="occlusion_bw")
    with pytest.raises(ValueError, match="num_input_frames"):
        I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], 2)
    with pytest.raises(ValueError, match="integer ids"):
        I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"].float(), 1)
    small = dict(out, dense_motion_bw=torch.zeros(1, 2, T, 4, 8))
    with pytest.raises(ValueError, match="different sizes"):
        I.propagate_maps(small, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], 1)
    # the op itself: CPU tensors are refused before anything else, like every other op
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.label_warp(torch.zeros(1, 2, T, 8, 16), prev["bg_mask"][:, :, 0], prev["instance_mask"][:, :, 0].int())
    with pytest.raises(RuntimeError, match="HIP device"):
        I.propagate_maps(out, prev["bg_mask"], prev["fg_mask"], prev["instance_mask"], 1)


def test_label_warp_plan_checks_shapes_and_dtypes():
    f, a, b = torch.zeros(2, 2, 3, 8, 16), torch.zeros(2, 4, 8, 16), torch.zeros(2, 1, 8, 16, dtype=torch.int32)
    assert ops._label_warp_plan(f, a, b, None, None) == (2, 3, 8, 16, 4, 1)
    assert ops._label_warp_plan(f[:, :, 0], None, b, torch.zeros(2, 1, 8, 16), 0.5) == (2, 1, 8, 16, 0, 1)
    assert ops._label_warp_plan(f, a[:, :0], None, None, None) == (2, 3, 8, 16, 0, 0)
    bad = [(f[:, :1], a, b, None, None), (f.double(), a, b, None, None), (f, a[:1], b, None, None),
           (f, a, b.long(), None, None), (f, a.int(), b, None, None), (f, a, b[..., :8], None, None), (f, None, None, None, None),
           (f, a, b, torch.zeros(2, 1, 3, 8, 16), None), (f, a, b, None, 0.5), (f, a, b, torch.zeros(2, 1, 8, 16), 0.5),
           (f, a, b, torch.zeros(2, 1, 3, 8, 16).double(), 0.5)]
    for args in bad:
        with pytest.raises(ValueError):
            ops._label_warp_plan(*args)


def test_label_warp_is_declared_bound_and_exported():
    assert "c2m_label_warp" in _lib.declared_symbols() and "c2m_label_warp" in _lib._SIGS
    L = _lib.lib()
    assert hasattr(L, "c2m_label_warp")
    # host-side argument checks of the launcher run without a device: nothing to do is success, a negative size is refused
    assert L.c2m_label_warp(None, 0, 0, 0, None, 0.0, 0, None, 0, None, 0, 0, 5, 8, 16, None, None, None) == 0
    assert L.c2m_label_warp(None, 0, 0, 0, None, 0.0, 0, None, 0, None, 0, 2, 5, 8, 16, None, None, None) == 0
    assert L.c2m_label_warp(None, 0, 0, 0, None, 0.0, 0, None, 3, None, 1, 2, 5, -8, 16, None, None, None) != 0
    assert L.c2m_label_warp(None, 0, 0, 0, None, 0.0, 0, None, 3, None, 1, 2, 5, 8, 16, None, None, None) != 0   # no flow
