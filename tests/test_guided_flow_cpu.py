"""Host side of the segment-guided dense flow (no GPU): what the float64 restatement (tests/guided_flow_np.py) gains at the edge of
a moving object, that constant ids are the unguided algorithm, the float32-against-float64 gap of the restatement on the GPU
tests' own inputs (from which their tolerance is derived), the C ABI and the launchers' refusals, and the argument checks of
c2m_amd.flow and train.compute_flow."""
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as NP
import flow_refine_np as RF
import guided_flow_np as G
from c2m_amd import _lib, flow as F, train


# ------------------------------------------------------------------------------------------------ the reference earns its keep
@functools.lru_cache(maxsize=None)
def scene_errors(size, obj, motion):
    """Mean EPE on (object, its 4-px band, background >= 8 px away) of the plain, guided, plain refined and guided refined flow."""
    a, b, true, inside, ids, far = G.scene(size, obj, motion)
    band = RF.object_masks(inside)[1]
    flows = dict(plain=NP.dense_flow(a, b), guided=G.dense_flow(a, b, ids), plain_refined=RF.dense_flow(a, b),
                 guided_refined=G.dense_flow(a, b, ids, refine_params=True))
    return {k: tuple(NP.epe(f, true, m) for m in (inside, band, far)) for k, f in flows.items()}


@pytest.mark.parametrize("size,obj,motion", G.SCENES)
def test_guided_reference_recovers_the_object_up_to_its_edge(size, obj, motion):
    """float64, ids = two_layer's object mask; mean endpoint error on the object's pixels (band: its 4-px edge band; background:
    >= 8 px from the object).  Measured, object (band) / background:
                                      plain            guided            plain refined    guided refined
      64 x 128, 24 x 36, (3, -2)      0.1847 / 0.0024  0.0064 (0.0105) / 0.0020  0.1761 / 0.0001  0.00016 / 0.0001
      64 x 128, 12 x 12, (3, -2)      1.0565 / 0.0006  0.00004 / 0.0006          1.1641 / 0.0001  0.00016 / 0.0001
      64 x 128, 24 x 36, (-5, 4)      0.2399 / 0.0026  0.0869 / 0.0025           0.4406 / 0.0003  0.00039 / 0.0002
      128 x 256, 50 x 70, (6, -3)     0.3785 / 0.0062  0.1931 / 0.0057           0.2266 / 0.0006  0.0170  / 0.0004
    The unrefined guided flow of the last two scenes still has patches of the band that end between the two motions at a coarse
    level (max error 6 and 11 px); the cut refinement repairs them, the uncut one cannot."""
    e = scene_errors(size, obj, motion)
    for k, v in e.items():
        print(size, obj, motion, f"{k:15s} object {v[0]:.5f} band {v[1]:.5f} background {v[2]:.5f}")
    if (obj, motion) == ((24, 36), (3, -2)):
        assert e["guided"][0] <= 0.03 and e["guided"][1] <= 0.05
    if obj == (12, 12):
        assert e["guided"][0] <= 0.01
    if size == (64, 128):
        assert e["guided_refined"][0] <= 0.005
    else:
        assert e["guided_refined"][0] <= 0.05 and e["guided_refined"][0] < 0.25 * e["plain_refined"][0]
    assert e["guided"][2] <= e["plain"][2] + 0.005 and e["guided_refined"][2] <= e["plain_refined"][2] + 0.005


def test_clip_reference_meets_the_bound_and_the_unguided_one_does_not():
    """float64, moving_boxes_clip(), t_in = 2, five predicted frames, frames on [-1, 1]; mean EPE of target_bw_of over each box in
    each predicted frame against the true -(k + 1) (dx, dy).  Measured, largest over boxes and frames: guided 0.0875 px whole box
    (band 0.157), guided and refined 0.0080 (band 0.0153); unguided: whole box 0.093 .. 1.03, band 0.184 .. 2.02 (the SMALLEST band
    figure is 0.184); unguided and refined: band 0.266 .. 2.78."""
    video, inst = NP.moving_boxes_clip()
    tp = dict(num_input_frames=G.CLIP_T_IN, num_predicted_frames=video.shape[1] - G.CLIP_T_IN)
    v = video * np.float32(2) - np.float32(1)
    t_in, t_out = tp["num_input_frames"], tp["num_predicted_frames"]
    guided = G.clip_box_errors(G.clip_target_bw(v, inst, t_in, t_out, (-1, 1)), inst, t_in)
    plain = G.clip_box_errors(G.clip_target_bw(v, inst, t_in, t_out, (-1, 1), guided=False), inst, t_in)
    print("guided", max(x[0] for x in guided.values()), "unguided band", min(x[1] for x in plain.values()))
    assert max(x[0] for x in guided.values()) <= G.CLIP_BOUND < min(x[1] for x in plain.values())


# ------------------------------------------------------------------------------------------------ constant ids
@pytest.mark.parametrize("refine", [None, True])
def test_constant_ids_are_the_unguided_algorithm(refine):
    """float64: n = 64, the threshold factor is 1, the densify weights are scaled by 64 (a power of two) and no edge is cut."""
    a, b, _, inside = NP.two_layer(64, 128)
    ids = np.full(inside.shape, -7, np.int32)
    want = RF.dense_flow(a, b, refine_params=refine)
    assert np.array_equal(G.dense_flow(a, b, ids, refine_params=refine), want)
    assert np.array_equal(G.dense_flow(a, b, ids, refine_params=refine, finest=1), RF.dense_flow(a, b, refine_params=refine, finest=1))
    assert not np.array_equal(G.dense_flow(a, b, inside.astype(np.int32), refine_params=refine), want)
    ia, ib, init = NP.level_pair(21, 37, 1, True, True)
    for level, shape in ((0, (21, 37)), (1, (41, 74))):
        seg = np.zeros(shape, np.int32)
        rec = G.patch_search(ia[0], ib[0], seg, init[0], level=level)
        assert np.array_equal(rec[..., :3], NP.patch_search(ia[0], ib[0], init[0])) and (rec[..., 3] == 64).all()
        assert np.array_equal(G.densify(ia[0], ib[0], rec, seg, level), NP.densify(ia[0], ib[0], rec[..., :3]))
        assert np.array_equal(G.refine(ia[0], ib[0], init[0], seg, level), RF.refine(ia[0], ib[0], init[0]))


def test_the_id_maps_reach_every_branch():
    """halves: the border runs through patch centres; stripes: pixels that fall back in densify; checker: n = 1 everywhere;
    wild: the extremes of int32; level 1 reads (y << 1, x << 1)."""
    for level in (0, 1):
        h, w = 21, 37
        H, W = (h, w) if level == 0 else (2 * h - 1, 2 * w)
        ia, ib, init = NP.level_pair(h, w, 1, False, False)
        n = {k: G.patch_search(ia[0], ib[0], G.id_map(k, H, W, level=level), init[0], level=level, details=True) for k in G.MAPS}
        assert (n["constant"][0][..., 3] == 64).all() and (n["checker"][0][..., 3] == 1).all()
        assert set(np.unique(n["halves"][0][..., 3])) == {32, 64} and set(np.unique(n["stripes"][0][..., 3])) == {32}
        assert len(np.unique(n["blobs"][0][..., 3])) > 3
        _, det, thr, _ = n["checker"]
        assert not (det > thr).any()
        S = G.level_ids(G.id_map("stripes", H, W, level=level), level, h, w)
        assert (S[:, ::2] == 12).all() and (S[:, 1::2] == 21).all()
        wild = G.id_map("wild", H, W)
        assert wild.min() == -2 ** 31 and wild.max() == 2 ** 31 - 1 and wild.dtype == np.int32
    # checker: nothing is searched (the records are the initial flow at the patch centres), nothing is smoothed
    ia, ib, init = NP.level_pair(16, 16, 1, False, False)
    seg = G.id_map("checker", 16, 16)
    rec = G.patch_search(ia[0], ib[0], seg, init[0])
    assert np.array_equal(rec[..., 0], init[0, 0][3::4, 3::4][:3, :3]) and np.array_equal(rec[..., 1], init[0, 1][3::4, 3::4][:3, :3])
    cut, smooth = G.refine(ia[0], ib[0], init[0], seg, outer=1, sor=1), RF.refine(ia[0], ib[0], init[0], outer=1, sor=1)
    assert not np.array_equal(cut, smooth)


# ------------------------------------------------------------------------------------------------ the GPU tests' tolerance
def test_tolerance_is_sixteen_times_the_float32_gap_of_the_guided_reference():
    """Search and densify over stage_cases() x MAPS; the excluded share of every case is within 10 % (it is 0)."""
    search = dens = 0.0
    share = {}
    for h, w, n, level in G.stage_cases():
        for kind in G.MAPS:
            ia, ib, init, seg = G.stage_inputs(h, w, n, level, kind)
            left = total = 0
            for i in range(n):
                r64, det, thr, d2 = G.patch_search(ia[i], ib[i], seg[i], init[i], level=level, details=True)
                r32 = G.patch_search(ia[i], ib[i], seg[i], init[i], level=level, dtype=np.float32)
                assert r32.dtype == np.float32
                keep = ~G.excluded(det, thr, d2)
                left, total = left + int((~keep).sum()), total + keep.size
                if keep.any():
                    search = max(search, float(np.abs(r64 - r32)[keep].max()))
                rec = r64.astype(np.float32)
                f32 = G.densify(ia[i], ib[i], rec, seg[i], level, dtype=np.float32)
                assert f32.dtype == np.float32
                dens = max(dens, float(np.abs(G.densify(ia[i], ib[i], rec, seg[i], level) - f32).max()))
            share[(h, w, n, level, kind)] = left / total
    worst = max(share, key=share.get)
    print(f"float32 - float64 gap: search {search:.3e} densify {dens:.3e} (TOL {G.TOL:.3e}); largest excluded share "
          f"{share[worst]:.3f} at {worst}")
    assert 0 < dens <= search <= G.SEARCH_GAP == G.TOL / 16
    assert search >= 0.5 * G.SEARCH_GAP                               # the constant is the measurement, not a loose bound
    assert G.TOL <= 10 * NP.TOL                                       # of use without a rule on badly conditioned patches
    assert all(s <= 0.10 for s in share.values()), worst


@pytest.mark.parametrize("kind", G.MAPS)
def test_refinement_tolerance_is_sixteen_times_the_float32_gap_of_its_map(kind):
    gap = 0.0
    for h, w, n, level, kw in G.refine_cases():
        ia, ib, init, seg = G.stage_inputs(h, w, n, level, kind, G.REFINE_SEED)
        for i in range(n):
            r32 = G.refine(ia[i], ib[i], init[i], seg[i], level, dtype=np.float32, **kw)
            assert r32.dtype == np.float32 and np.isfinite(r32).all()
            gap = max(gap, float(np.abs(G.refine(ia[i], ib[i], init[i], seg[i], level, **kw) - r32).max()))
    print(kind, f"float32 - float64 gap of refine {gap:.3e} (REFINE_TOL {G.REFINE_TOL[kind]:.3e})")
    assert 0.5 * G.REFINE_GAP[kind] <= gap <= G.REFINE_GAP[kind] == G.REFINE_TOL[kind] / 16


def test_a_pixel_without_neighbours_on_a_flat_image_keeps_its_flow():
    """All edges cut and no image gradient: D = A11 = 0 and b = 0; the pixel's du stays 0 and no NaN reaches its neighbours
    through 0 * NaN.  (With one id D > 0 everywhere: the rule never acts, and constant ids stay the unguided bits.)"""
    flat = np.full((16, 16), 97.0)
    flow = np.random.default_rng(0).uniform(-1, 1, (2, 16, 16))
    got = G.refine(flat, flat, flow, G.id_map("checker", 16, 16))
    assert np.array_equal(got, flow)
    one = np.zeros((16, 16), np.int32)
    one[5, 5] = 1
    got = G.refine(flat, flat, flow, one)
    assert np.isfinite(got).all() and np.array_equal(got[:, 5, 5], flow[:, 5, 5]) and not np.array_equal(got, flow)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_exported():
    for name in ("c2m_flow_patch_search_guided", "c2m_flow_densify_guided", "c2m_flow_refine_iterate_guided"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
        assert hasattr(_lib.lib(), name)
    plain, guided = _lib._SIGS["c2m_flow_patch_search"][1], _lib._SIGS["c2m_flow_patch_search_guided"][1]
    assert guided[:len(plain) - 1] == plain[:-1] and len(guided) == len(plain) + 5     # segments, elems, level, H, W before stream
    assert _lib.lib().c2m_abi_version() == _lib.ABI_VERSION                            # purely additive


def test_launcher_checks():
    """Host-side checks run without a device: nothing to do is success; bad sizes, a missing map and a level whose shifted index
    would pass the map are refused."""
    L = _lib.lib()

    def search(N=0, h=8, w=8, iters=12, shift=0, seg=None, elems=0, level=0, H=8, W=8):
        return L.c2m_flow_patch_search_guided(None, None, 0, None, 0, shift, None, 0, N, h, w, iters, seg, elems, level, H, W, None)

    def dens(N=0, h=8, w=8, shift=0, Ho=8, Wo=8, seg=None, elems=0, level=0, H=8, W=8):
        return L.c2m_flow_densify_guided(None, None, 0, None, 0, None, 0, N, h, w, shift, Ho, Wo, seg, elems, level, H, W, None)

    def iterate(N=0, h=8, w=8, sor=5, seg=None, elems=0, level=0, H=8, W=8, out=None, Ho=8):
        return L.c2m_flow_refine_iterate_guided(None, 0, None, 0, N, h, w, 0, sor, 20.0, 5.0, 10.0, 1.6, out, 0, 0, Ho, 8, seg, elems,
                                                level, H, W, None)

    ids = torch.zeros(64, dtype=torch.int32)
    for fn in (search, dens, iterate):
        assert fn() == 0                                              # N = 0
        assert fn(level=1, H=15, W=15) == 0 and fn(level=1, H=16, W=30) == 0          # (8 - 1) << 1 = 14 < 15
        assert fn(level=1, H=14, W=15) != 0 and fn(level=1, H=15, W=14) != 0          # row / column 14 of a 14-row map
        assert fn(level=1) != 0 and fn(level=-1) != 0 and fn(level=7) != 0
        assert fn(h=9) != 0 and fn(w=9) != 0 and fn(H=0) != 0 and fn(h=7, H=8) != 0
        assert fn(N=1) != 0                                           # no map
        assert fn(N=1, seg=ids.data_ptr(), elems=63) != 0             # a map that is too short
        assert fn(N=1, seg=ids.data_ptr(), elems=64) != 0             # a map, but no images
        assert fn(N=1, seg=ids.data_ptr() + 2, elems=64) != 0         # misaligned
    assert search(iters=1025) != 0 and search(shift=2) != 0
    assert dens(Ho=9) != 0 and dens(shift=1, Ho=16, Wo=16) == 0
    assert iterate(sor=6) != 0 and iterate(out=ids.data_ptr(), Ho=9) != 0 and iterate(out=ids.data_ptr()) == 0
    # the unguided launchers are what they were
    assert L.c2m_flow_patch_search(None, None, 0, None, 0, 0, None, 0, 0, 8, 8, 12, None) == 0
    assert L.c2m_flow_patch_search(None, None, 0, None, 0, 0, None, 0, 1, 8, 8, 12, None) != 0
    assert L.c2m_flow_densify(None, None, 0, None, 0, None, 0, 0, 8, 8, 0, 9, 8, None) != 0
    assert L.c2m_flow_workspace_bytes(3, 33, 65, 2) == 4 * (2 * 3 * (33 * 65 + 17 * 33) + 3 * 8 * 16 * 3 + 2 * 3 * 17 * 33)


# ------------------------------------------------------------------------------------------------ the interface
def test_argument_errors_are_raised_before_any_launch():
    a = torch.zeros(2, 3, 16, 24)
    seg = torch.zeros(2, 16, 24, dtype=torch.int32)
    with pytest.raises(ValueError, match="HIP device"):              # the images are checked first, as without segments
        F.dense_flow(a, a, segments=seg)
    cf = F.ClassicFlow()
    assert cf.takes_segments
    for shape, sshape in (((2, 3, 16, 24), (2, 16, 24)), ((1, 2, 3, 16, 24), (1, 2, 16, 24)), ((1, 1, 2, 3, 16, 24), (1, 1, 2, 16, 24))):
        with pytest.raises(ValueError, match="HIP device"):
            cf(torch.zeros(shape), torch.zeros(shape), segments=torch.zeros(sshape, dtype=torch.int32))
        with pytest.raises(ValueError, match="segments must be"):
            cf(torch.zeros(shape), torch.zeros(shape), segments=torch.zeros(sshape[1:], dtype=torch.int32))
    video = torch.zeros(1, 3, 4, 16, 24)
    for bad in (torch.zeros(1, 4, 16, 24), torch.zeros(1, 3, 16, 24, dtype=torch.int32), torch.zeros(2, 4, 16, 24, dtype=torch.int32),
                torch.zeros(1, 4, 16, 25, dtype=torch.int32), torch.zeros(4, 16, 24, dtype=torch.int32), "ids"):
        with pytest.raises(ValueError, match="segments must be"):
            F.clip_flows(video, 2, 2, segments=bad)
    # a flow module that takes no segments says so; without segments nothing changes for it
    tp = dict(num_input_frames=2, num_predicted_frames=2)
    calls = []

    def stub(A, B):
        calls.append(A.shape[0])
        return torch.zeros(A.shape[0], 2, 16, 24), torch.zeros(A.shape[0], 1, 16, 24)

    ids = torch.zeros(1, 4, 16, 24, dtype=torch.int32)
    with pytest.raises(ValueError, match="segments"):
        train.compute_flow(stub, dict(video=video), tp, segments=ids)
    assert calls == [] and train.compute_flow(stub, dict(video=video), tp)["target_bw_of"].shape == (1, 2, 2, 16, 24)
    with pytest.raises(ValueError, match="segments must be"):
        train.compute_flow(cf, dict(video=video), tp, segments=ids[:, :3])
    got = []

    class Takes(torch.nn.Module):
        takes_segments = True

        def forward(self, A, B, segments=None):
            got.append(segments)
            return stub(A, B)

    marked = torch.arange(4, dtype=torch.int32).view(1, 4, 1, 1).expand(1, 4, 16, 24)
    train.compute_flow(Takes(), dict(video=video), tp, segments=marked)
    assert got[0].shape == (6, 16, 24) and got[0][:, 0, 0].tolist() == [0, 1, 1, 2, 1, 3]     # the first frame of every pair
    train.compute_flow(Takes(), dict(video=video), tp)
    assert got[1] is None
    for bad in (marked.long(), marked[:, :3], marked[..., :23], marked[0], "ids"):      # refused before the module is called
        with pytest.raises(ValueError, match="segments must be"):
            train.compute_flow(Takes(), dict(video=video), tp, segments=bad)
    assert len(got) == 2
