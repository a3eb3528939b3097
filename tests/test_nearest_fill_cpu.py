"""Host side of the nearest-seed fill (no GPU): the numpy oracle against scipy's distance transform, the checks made before any
launch, the C ABI, and how propagate_maps / rollout build the masks and pass `fill` through, with the operators stubbed."""
import types

import numpy as np
import pytest
import torch

import nearest_fill_np as NF
from c2m_amd import _lib, interactive as I, ops

T = 5


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_ties_go_to_the_smaller_row_then_column():
    for seeds, want in (([(0, 5), (0, -5)], (0, -5)), ([(5, 0), (-5, 0)], (-5, 0)), ([(0, 5), (-3, 4), (4, 3)], (-3, 4)),
                        ([(0, 5), (4, 3)], (0, 5)), ([(0, 5), (-5, 0)], (-5, 0)), ([(3, -4), (4, 3)], (3, -4))):
        hole, seed = NF.paint(16, 16, 8, 8, seeds)
        _, _, src = NF.sources(hole, seed)
        assert (src[0] // 16 - 8, src[0] % 16 - 8) == want, seeds
    hole, seed = NF.paint(4, 4, 1, 1, [(0, 1)])
    seed[1, 1] = 1                                                     # set in both: a hole, never a seed
    assert NF.sources(hole, seed)[2].tolist() == [1 * 4 + 2]
    assert NF.sources(hole, np.zeros_like(seed))[2] is None


def test_oracle_distances_equal_scipys_distance_transform():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for H, W, ph, ps in ((33, 300, 0.3, 0.02), (7, 65, 0.6, 0.05), (1, 70, 0.5, 0.1), (40, 40, 0.9, 0.003)):
        hole = rng.random((H, W)) < ph
        seed = (rng.random((H, W)) < ps) & ~hole
        seed[rng.integers(H), rng.integers(W)] = True                  # at least one
        hole &= ~seed
        edt = ndimage.distance_transform_edt(~seed)                    # distance of every pixel to the nearest seed
        got = NF.source_distance(hole, seed)
        assert np.array_equal(got[hole], edt[hole])                    # both are sqrt of the same integer


# ------------------------------------------------------------------------------------------------ checks before any launch
def test_plan_accepts_and_refuses():
    z = lambda *s, dtype=torch.uint8: torch.zeros(*s, dtype=dtype)
    h, s = z(2, 5, 8, 16), z(2, 5, 8, 16, dtype=torch.bool)
    pf, pi = z(2, 20, 5, 8, 16, dtype=torch.float32), z(2, 1, 5, 8, 16, dtype=torch.int32)
    assert ops._nearest_fill_plan(h, s, pf, pi) == (2, 5, 8, 16, 20, 1)
    assert ops._nearest_fill_plan(h[:, 0], s[:, 0], None, pi[:, :, :1]) == (2, 1, 8, 16, 0, 1)
    assert ops._nearest_fill_plan(h, s, pf, pi[:, :0]) == (2, 5, 8, 16, 20, 0)
    big = z(3, 30, 7, 8, 16, dtype=torch.float32)
    assert ops._nearest_fill_plan(h, s, big[:2, 3:23, 1:6], None) == (2, 5, 8, 16, 20, 0)           # any outer strides
    assert ops._nearest_fill_plan(z(1, 1, 1, 1), z(1, 1, 1, 1), None, z(1, 1, 1, 1, 1, dtype=torch.int32)) == (1, 1, 1, 1, 0, 1)
    wider = z(2, 20, 5, 8, 32, dtype=torch.float32)
    bad = [(h[0, 0], s[0, 0], pf, pi), (h.float(), s, pf, pi), (h, s.int(), pf, pi), (h, s[:1], pf, pi), (h, s, None, None),
           (h, s, pf[:, :0], pi[:, :0]), (h, s, pf[:, :0], None), (h, s, pf.double(), pi), (h, s, pf, pi.long()),
           (h, s, pf[:1], pi), (h, s, pf[:, :, :4], pi), (h, s, pf[:, 0], pi), (h, s, pf, pi[..., :8]),
           (h, s, wider[..., ::2], pi), (h, s, wider[..., :16], pi),                                      # rows not dense
           (h, s, pf[:, :1].expand(2, 20, 5, 8, 16), pi)]                                                 # written through 20 indices
    for args in bad:
        with pytest.raises(ValueError):
            ops._nearest_fill_plan(*args)
    one, word = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)                      # sizes only: no memory
    for shape in ((1, 1, 1, 32769), (1, 1, 32769, 1), (1, 1, 32768, 32768 * 2)):
        with pytest.raises(ValueError, match="at most 32768"):
            ops._nearest_fill_plan(one.expand(shape), one.expand(shape), None, word.expand(shape[:1] + (1,) + shape[1:]))
    with pytest.raises(RuntimeError, match="HIP device"):               # the op itself refuses host tensors first
        ops.nearest_fill(h, s, pf, pi)


def test_entry_points_are_declared_bound_and_exported():
    for name in ("c2m_nearest_fill", "c2m_nearest_fill_workspace_bytes"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
    L = _lib.lib()
    wb = L.c2m_nearest_fill_workspace_bytes
    assert wb(8, 5, 128, 256) == 40 * 128 * 4 * 8 + 20 * 8              # 4 KB of bits per frame, then the seed counters
    assert wb(1, 1, 1, 1) == 8 + 8 and wb(1, 3, 2, 65) == 3 * 2 * 2 * 8 + 2 * 8 and wb(0, 5, 8, 16) == 0
    assert wb(1, 1, 32768, 32768) > 0 and wb(1, 1, 32769, 1) == -1 and wb(1, 1, 1, 32769) == -1 and wb(1, -1, 8, 8) == -1
    nf = L.c2m_nearest_fill
    # host-side argument checks of the launcher run without a device: nothing to do is success, bad sizes are refused
    assert nf(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 1, 0, 5, 8, 16, None, None, 0, None) == 0
    assert nf(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 1, 2, 5, -8, 16, None, None, 0, None) != 0
    assert nf(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 1, 2, 5, 8, 32769, None, None, 0, None) != 0
    assert nf(None, None, None, 0, 0, 0, 0, None, 0, 0, 0, 1, 2, 5, 8, 16, None, None, 0, None) != 0        # no unfilled


# ------------------------------------------------------------------------------------------------ the interface
def _maps(B, H=8, W=16):
    sem = torch.zeros(B, 20, 1, H, W)
    sem[:, 3] = 1.0
    inst = torch.full((B, 1, 1, H, W), 7, dtype=torch.int64)           # stuff
    inst[:, :, :, 2:5, 3:9] = 11000                                    # a thing
    inst[:, :, :, 6, 10] = 18999                                       # the last thing id
    inst[:, :, :, 6, 11] = 19000                                       # the first id above the range: no thing
    inst[:, :, :, 6, 12] = 999
    return sem[:, :11], sem[:, 11:], inst


def _out(B, H=8, W=16):
    occ = torch.ones(B, 1, T, H, W)
    occ[:, :, :, 1:4, 2:6] = 0.25                                      # disoccluded, partly on the thing
    occ[:, :, 1] = 0.5                                                 # exactly the threshold: not below it
    occ[:, :, 2] = float("nan")                                        # compares false, as in the kernel
    return dict(dense_motion_bw=torch.zeros(B, 2, T, H, W), occlusion_bw=occ, generated=torch.zeros(B, 3, T, H, W))


def _stubs(monkeypatch):
    calls = dict(warp=[], fill=[])

    def label_warp(flow, planes_f=None, planes_i=None, occ=None, threshold=None, fill_id=0):
        calls["warp"].append(dict(occ=occ, threshold=threshold, fill_id=fill_id))
        Tn = flow.shape[2]
        return planes_f.unsqueeze(2).repeat(1, 1, Tn, 1, 1), planes_i.unsqueeze(2).repeat(1, 1, Tn, 1, 1)

    def nearest_fill(hole, seed, planes_f=None, planes_i=None):
        calls["fill"].append(dict(hole=hole, seed=seed, planes_f=planes_f, planes_i=planes_i))
        return torch.arange(hole.shape[0] * hole.shape[1], dtype=torch.int32).view(hole.shape[:2])

    monkeypatch.setattr(ops, "label_warp", label_warp)
    monkeypatch.setattr(ops, "nearest_fill", nearest_fill)
    return calls


def test_fill_needs_a_threshold_and_a_known_name(monkeypatch):
    calls = _stubs(monkeypatch)
    bg, fg, inst = _maps(1)
    with pytest.raises(ValueError, match="(?s)fill.*occ_threshold"):
        I.propagate_maps(_out(1), bg, fg, inst, 1, fill="nearest")
    for fill in ("linear", "", True, 0):
        with pytest.raises(ValueError, match="fill must be one of"):
            I.propagate_maps(_out(1), bg, fg, inst, 1, occ_threshold=0.5, fill=fill)
    model = types.SimpleNamespace(train_params=dict(num_input_frames=1, num_predicted_frames=T, input_size=[8, 16]),
                                  model_params=dict(common_params=dict(scale_factor=1, flow_channel=2, occlusion_channel=1)))
    prev = dict(video=torch.zeros(1, 3, 1, 8, 16), bg_mask=bg, fg_mask=fg, instance_mask=inst)
    for kw in (dict(fill="nearest"), dict(fill="edt", occ_threshold=0.5)):
        with pytest.raises(ValueError, match="fill"):
            I.continue_click_to_move(model, prev, _out(1), [], **kw)
        with pytest.raises(ValueError, match="fill"):
            I.rollout(model, prev["video"], bg, fg, inst, [[]], **kw)
    assert not calls["warp"] and not calls["fill"]                     # refused before anything ran


def test_propagate_maps_builds_hole_and_seed(monkeypatch):
    calls = _stubs(monkeypatch)
    B = 2
    bg, fg, inst = _maps(B)
    out = _out(B)
    maps = I.propagate_maps(out, bg, fg, inst, 1, occ_threshold=0.5, fill_id=3, fill="nearest")
    assert calls["warp"] == [dict(occ=out["occlusion_bw"], threshold=0.5, fill_id=3)]           # label_warp's call is unchanged
    (c,) = calls["fill"]
    hole, seed = c["hole"], c["seed"]
    assert hole.shape == seed.shape == (B, T, 8, 16) and hole.dtype == seed.dtype == torch.bool
    want = torch.zeros(B, T, 8, 16, dtype=torch.bool)
    want[:, :, 1:4, 2:6] = True
    want[:, 1:3] = False                                               # occ == threshold and NaN are no holes
    assert torch.equal(hole, want)
    ids = inst[:, 0].expand(B, T, 8, 16)
    thing = (ids >= 1000) & (ids < 19000)
    assert not (seed & thing).any() and not (seed & hole).any()        # a thing pixel is never a seed, a hole is never a seed
    assert torch.equal(seed, ~hole & ~thing)
    assert seed[0, 0, 6, 11] and seed[0, 0, 6, 12] and not seed[0, 0, 6, 10] and not seed[0, 0, 2, 6]
    # one call covers the 20 float planes and the id plane, and the maps returned are views of what it filled
    assert c["planes_f"].shape == (B, 20, T, 8, 16) and c["planes_i"].shape == (B, 1, T, 8, 16)
    assert maps["bg_mask"].data_ptr() == c["planes_f"].data_ptr() and maps["instance_mask"] is c["planes_i"]
    assert maps["fg_mask"].shape == (B, 9, T, 8, 16) and maps["fg_mask"]._base is c["planes_f"]
    assert maps["unfilled"].tolist() == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]
    # another id range moves the seeds with it
    I.propagate_maps(out, bg, fg, inst, 1, occ_threshold=0.5, fill="nearest", id_range=(5, 8))
    seed2 = calls["fill"][1]["seed"]
    assert torch.equal(seed2, ~hole & (ids != 7))


def test_fill_none_is_todays_behaviour(monkeypatch):
    calls = _stubs(monkeypatch)
    bg, fg, inst = _maps(1)
    for kw in ({}, dict(occ_threshold=0.5), dict(occ_threshold=0.5, fill=None)):
        maps = I.propagate_maps(_out(1), bg, fg, inst, 1, **kw)
        assert sorted(maps) == ["bg_mask", "fg_mask", "instance_mask"]
    assert len(calls["warp"]) == 3 and not calls["fill"]


def test_rollout_passes_fill_through_and_returns_unfilled(monkeypatch):
    calls = _stubs(monkeypatch)
    B, K = 2, 3
    bg, fg, inst = _maps(B)
    model = types.SimpleNamespace(train_params=dict(num_input_frames=1, num_predicted_frames=T, input_size=[8, 16]),
                                  model_params=dict(common_params=dict(scale_factor=1, flow_channel=2, occlusion_channel=1)))
    info = dict(ids=np.zeros((B, 1), np.int64), edges=np.zeros((B, 1, 1, 4)), count=np.zeros(B, np.int64), nodes=[])
    monkeypatch.setattr(I, "_predict", lambda *a, **k: (_out(B), info))
    monkeypatch.setattr(I, "predicted_boxes", lambda maps, ids, id_range: (torch.zeros(B, 1), torch.zeros(B, 1, T, 4),
                                                                           torch.zeros(B, 1, T, dtype=torch.bool)))
    video = torch.zeros(B, 3, 1, 8, 16)
    res = I.rollout(model, video, bg, fg, inst, [[]] * K, occ_threshold=0.5, fill="nearest", id_range=(5, 8))
    assert len(calls["fill"]) == K and res["unfilled"].shape == (B, K * T) and res["unfilled"].dtype == torch.int32
    assert res["unfilled"][1].tolist() == [5, 6, 7, 8, 9] * K          # concatenated over the segments, frame order
    assert not calls["fill"][0]["seed"][0, 0, 0, 0]                    # id 7 is a thing of id_range (5, 8): box_kw's range is used
    assert res["instance_mask"].shape == (B, 1, K * T, 8, 16)
    calls["fill"].clear()
    res = I.rollout(model, video, bg, fg, inst, [[]] * K, occ_threshold=0.5)
    assert "unfilled" not in res and not calls["fill"]

    got = {}
    monkeypatch.setattr(I, "click_to_move", lambda *a, **k: got.update(k) or "out")
    prev = dict(video=video, bg_mask=bg, fg_mask=fg, instance_mask=inst)
    I.continue_click_to_move(model, prev, _out(B), [], occ_threshold=0.5, fill="nearest", min_pixels=4)
    assert len(calls["fill"]) == 1 and got == dict(min_pixels=4)       # fill is not one of click_to_move's box keywords
