"""Host side of the dataset-resolution output (no GPU): the float64 restatement of the composite checks itself against the
properties its definition promises, ops._detail_warp_plan refuses every bad shape and dtype before a launch, the entry
point is declared, bound and exported, and the op and c2m_amd.fullres fail loudly on CPU tensors."""
import numpy as np
import pytest
import torch

import fullres_np as R
from c2m_amd import _lib, fullres, ops


def case(h, w, H, W, B=2, T=2, seed=0):
    return R.make_case(h, w, H, W, B, T, seed)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_taps_are_those_of_the_resize_tables():
    for n_in, n_out in ((13, 13), (13, 40), (9, 37), (6, 15), (16, 128)):
        i0, i1, lam, _ = R.up_taps(n_in, n_out)
        bounds, k, _ = ops._resize_bilinear_taps(n_in, n_out)
        assert np.array_equal(bounds[:, 0], i0)
        two = bounds[:, 1] == 2
        assert np.array_equal(two, i1 > i0)
        assert np.array_equal(k[:, 1], np.where(two, lam, 0.0)) and np.array_equal(k[:, 0], np.where(two, 1 - lam, 1.0))


def test_scale_one_is_the_generator_output():
    """H = h, W = w and F = 255 f: the full-size warp IS the working-size warp, so v = 255 G wherever the flow points."""
    c = case(9, 13, 9, 13, seed=1)
    f = np.moveaxis(c["F"].astype(np.float64) / 255.0, -1, 1)
    Wl = R.warp_small(f, c["flow"])                                   # float64, not rounded
    G = np.clip(Wl + np.random.default_rng(2).standard_normal(Wl.shape) * 0.05, 0, 1)
    r = R.detail_warp(c["F"], G, Wl, c["flow"], c["occ"])
    assert np.abs(r["v"] - 255.0 * np.moveaxis(G, 1, -1)).max() <= 1e-9
    assert np.array_equal(r["levels"], np.floor(255.0 * np.moveaxis(G, 1, -1) + 0.5).astype(np.uint8))


def test_occlusion_zero_is_the_plain_enlargement():
    c = case(9, 13, 37, 53, seed=3)
    r = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], np.zeros_like(c["occ"]))
    assert np.array_equal(r["v"], 255.0 * np.moveaxis(R.up(c["G"], 37, 53), 1, -1))


def test_a_constant_frame_adds_nothing():
    c = case(6, 10, 15, 25, seed=4)
    F = np.empty_like(c["F"])
    F[...] = (51, 102, 204)
    Wl = np.broadcast_to(np.array([0.2, 0.4, 0.8])[None, :, None, None, None], c["Wl"].shape)
    r = R.detail_warp(F, c["G"], Wl, c["flow"], c["occ"])
    assert np.abs(r["v"] - 255.0 * np.moveaxis(R.up(c["G"], 15, 25), 1, -1)).max() <= 1e-9


def test_occlusion_none_is_one_everywhere():
    c = case(9, 13, 9, 40, seed=5)
    a = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], None)
    b = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], np.ones_like(c["occ"]))
    assert np.array_equal(a["v"], b["v"])


def test_wild_flows_index_in_bounds():
    c = case(8, 16, 64, 128, seed=6)
    flow = c["flow"].copy()
    flow[0, 0, 0, 2, 3], flow[0, 1, 0, 5, 9], flow[1, 0, 1, 1, 1], flow[1, 1, 1, 6, 12] = np.nan, np.inf, -np.inf, 1e30
    flow[1, 0, 0, 4, 4], flow[1, 0, 0, 4, 5] = np.inf, -np.inf        # neighbours: inf - inf inside the enlargement
    r = R.detail_warp(c["F"], c["G"], c["Wl"], flow, c["occ"], c["ids"], 0.3, -7)
    for k, n in (("IX", 128), ("IY", 64)):
        assert np.isfinite(r[k]).all() and r[k].min() >= 0 and r[k].max() <= n - 1
    assert np.isfinite(r["v"]).all()                                  # the clamped coordinates read real pixels
    assert r["IX"][0, 0, 16:24, 24:32].min() == 0.0                   # the NaN's footprint reads column 0
    assert r["IX"][1, 1].min() == 0.0 and r["IY"][0, 0].max() == 63.0 and r["IY"][1, 1].max() == 63.0
    assert set(np.unique(r["ids"])) <= set(np.unique(c["ids"])) | {-7}


def test_ids_are_gathered_not_blended_and_filled_below_the_threshold():
    c = case(9, 13, 37, 53, seed=7)
    r = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], c["occ"], c["ids"], 0.4, -1)
    plain = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], c["occ"], c["ids"])["ids"]
    low = r["occ_up"] < 0.4
    assert low.any() and not low.all()
    assert (r["ids"][low] == -1).all() and np.array_equal(r["ids"][~low], plain[~low])
    assert set(np.unique(plain)) <= set(np.unique(c["ids"]))
    zero = R.detail_warp(c["F"], c["G"], c["Wl"], np.zeros_like(c["flow"]), None, c["ids"])
    assert np.array_equal(zero["ids"][:, 0], zero["ids"][:, 1])


# ------------------------------------------------------------------------------------------------ the plan
def tensors(B=2, T=3, h=8, w=16, H=32, W=48):
    return dict(frame_u8=torch.zeros(B, H, W, 3, dtype=torch.uint8), generated=torch.zeros(B, 3, T, h, w),
                warped=torch.zeros(B, 3, T, h, w), flow=torch.zeros(B, 2, T, h, w), occ=torch.zeros(B, 1, T, h, w),
                ids=torch.zeros(B, H, W, dtype=torch.int32), occ_threshold=0.5)


def test_plan_accepts_the_good_shapes():
    t = tensors()
    assert ops._detail_warp_plan(**t) == (2, 3, 8, 16, 32, 48)
    assert ops._detail_warp_plan(**dict(t, occ=None, occ_threshold=None)) == (2, 3, 8, 16, 32, 48)
    assert ops._detail_warp_plan(**dict(t, ids=None, occ_threshold=None)) == (2, 3, 8, 16, 32, 48)
    assert ops._detail_warp_plan(**dict(t, occ_threshold=None)) == (2, 3, 8, 16, 32, 48)          # ids without a fill
    assert ops._detail_warp_plan(**dict(t, generated=t["generated"].bfloat16(), warped=t["warped"].bfloat16(),
                                        occ=t["occ"].bfloat16())) == (2, 3, 8, 16, 32, 48)
    s = tensors(H=8, W=16)                                                                         # scale 1
    assert ops._detail_warp_plan(**s) == (2, 3, 8, 16, 8, 16)
    m = tensors(h=2, w=2, H=2, W=3)
    assert ops._detail_warp_plan(**m) == (2, 3, 2, 2, 2, 3)


BAD = {
    "h < 2": lambda t: tensors(h=1, H=32),
    "w < 2": lambda t: tensors(w=1),
    "H < h": lambda t: tensors(H=7),
    "W < w": lambda t: tensors(W=15),
    "generated is not 5-d": lambda t: dict(t, generated=t["generated"][:, :, 0]),
    "generated has 4 channels": lambda t: dict(t, generated=torch.zeros(2, 4, 3, 8, 16)),
    "generated is fp64": lambda t: dict(t, generated=t["generated"].double()),
    "flow at another size": lambda t: dict(t, flow=torch.zeros(2, 2, 3, 8, 15)),
    "flow with another T": lambda t: dict(t, flow=torch.zeros(2, 2, 2, 8, 16)),
    "flow with 3 channels": lambda t: dict(t, flow=torch.zeros(2, 3, 3, 8, 16)),
    "flow in bf16": lambda t: dict(t, flow=t["flow"].bfloat16()),
    "occ at another size": lambda t: dict(t, occ=torch.zeros(2, 1, 3, 4, 8)),
    "occ with 2 channels": lambda t: dict(t, occ=torch.zeros(2, 2, 3, 8, 16)),
    "occ in fp64": lambda t: dict(t, occ=t["occ"].double()),
    "warped at another size": lambda t: dict(t, warped=torch.zeros(2, 3, 3, 9, 16)),
    "warped of another batch": lambda t: dict(t, warped=torch.zeros(1, 3, 3, 8, 16)),
    "warped in fp16": lambda t: dict(t, warped=t["warped"].half()),
    "frame is float": lambda t: dict(t, frame_u8=t["frame_u8"].float()),
    "frame is channels-first": lambda t: dict(t, frame_u8=torch.zeros(2, 3, 32, 48, dtype=torch.uint8)),
    "frame of another batch": lambda t: dict(t, frame_u8=torch.zeros(1, 32, 48, 3, dtype=torch.uint8)),
    "frame without a batch": lambda t: dict(t, frame_u8=torch.zeros(32, 48, 3, dtype=torch.uint8)),
    "ids in int64": lambda t: dict(t, ids=t["ids"].long()),
    "ids at the working size": lambda t: dict(t, ids=torch.zeros(2, 8, 16, dtype=torch.int32)),
    "ids with a channel axis": lambda t: dict(t, ids=torch.zeros(2, 1, 32, 48, dtype=torch.int32)),
    "a threshold without ids": lambda t: dict(t, ids=None),
    "a threshold without occ": lambda t: dict(t, occ=None),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_plan_refuses(what):
    with pytest.raises(ValueError):
        ops._detail_warp_plan(**BAD[what](tensors()))


# ------------------------------------------------------------------------------------------------ ABI, fail-loud
def test_detail_warp_is_declared_bound_and_exported():
    assert "c2m_detail_warp" in _lib.declared_symbols() and "c2m_detail_warp" in _lib._SIGS
    L = _lib.lib()
    assert hasattr(L, "c2m_detail_warp")
    # host-side argument checks of the launcher run without a device: nothing to do is success, bad sizes are refused
    call = lambda B, T, h, w, H, W: L.c2m_detail_warp(None, None, None, None, None, None, 0.0, 0, B, T, h, w, H, W, None,
                                                       None, None)
    assert call(0, 5, 8, 16, 64, 128) == 0 and call(2, 0, 8, 16, 64, 128) == 0
    assert call(2, 5, 1, 16, 64, 128) != 0 and call(2, 5, 8, 1, 64, 128) != 0
    assert call(2, 5, 8, 16, 7, 128) != 0 and call(2, 5, 8, 16, 64, 15) != 0
    assert call(2, 5, 8, 16, 64, 128) != 0                                                          # no tensors
    assert call(-1, 5, 8, 16, 64, 128) != 0


def test_cpu_tensors_fail_loudly():
    t = tensors()
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.detail_warp(t["frame_u8"], t["generated"], t["warped"], t["flow"])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.detail_warp(**t)
    out = dict(generated=t["generated"], dense_motion_bw=t["flow"], occlusion_bw=t["occ"])
    video = torch.zeros(2, 3, 1, 8, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        fullres.upscale(out, video, t["frame_u8"], 1)


def test_upscale_checks_its_arguments_first():
    t = tensors()
    out = dict(generated=t["generated"], dense_motion_bw=t["flow"], occlusion_bw=t["occ"])
    video = torch.zeros(2, 3, 1, 8, 16)
    with pytest.raises(ValueError, match="flow must be one of"):
        fullres.upscale(out, video, t["frame_u8"], 1, flow="occlusion_bw")
    with pytest.raises(ValueError, match="num_input_frames"):
        fullres.upscale(out, video, t["frame_u8"], 2)
    small = dict(out, dense_motion_bw=torch.zeros(2, 2, 3, 4, 8))                # a scale_factor != 1 model
    with pytest.raises(ValueError, match="different sizes"):
        fullres.upscale(small, video, t["frame_u8"], 1)
