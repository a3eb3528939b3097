"""Segment-guided dense flow on the GPU (run with -m gpu): the guided instantiations of the patch search, the densify and the
refinement's iterate kernel against the float64 restatement (tests/guided_flow_np.py) within the tolerances that
tests/test_guided_flow_cpu.py derives from the restatement's own float32 error; constant ids against segments=None bit for bit;
repeatability, independence of the batch, stream order; the quality bounds at the edge of a moving object; clip_flows and
ClassicFlow(chain=True) with the instance maps of a painted clip; argument errors."""
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as NP
import flow_refine_np as RF
import gpu_util
import guided_flow_np as G
from c2m_amd import flow as F
from c2m_amd import train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the stages
@pytest.mark.parametrize("h,w,n,level", G.stage_cases())
def test_patch_search_and_densify_vs_float64(h, w, n, level):
    """Every map of guided_flow_np.MAPS; densify on the float64 records rounded to float32."""
    npy, npx = len(NP.origins(h)), len(NP.origins(w))
    for kind in G.MAPS:
        ia, ib, init, seg = G.stage_inputs(h, w, n, level, kind)
        got = F.patch_search(dev(ia), dev(ib), dev(init), segments=dev(seg), level=level).cpu().numpy()
        assert got.shape == (n, npy, npx, 4)
        want = [G.patch_search(ia[i], ib[i], seg[i], init[i], level=level, details=True) for i in range(n)]
        left_out = 0
        for i, (rec, det, thr, d2) in enumerate(want):
            keep = ~G.excluded(det, thr, d2)
            left_out += int((~keep).sum())
            err = np.abs(got[i] - rec)[keep]
            print(f"{kind} pair {i}: search max |gpu - float64| = {err.max() if err.size else 0:.3e} (TOL {G.TOL:.3e})")
            assert (err <= G.TOL).all(), kind
            assert np.array_equal(got[i, ..., 3], rec[..., 3]), kind                     # the count is exact
            if kind == "checker":                                     # n = 1: nothing is searched, the initial flow bit for bit
                cy, cx = np.asarray(NP.origins(h)) + 3, np.asarray(NP.origins(w)) + 3
                assert np.array_equal(got[i, ..., :2], init[i][:, cy[:, None], cx[None, :]].transpose(1, 2, 0))
        assert left_out <= 0.10 * n * npy * npx
        rec = np.stack([r[0] for r in want]).astype(np.float32)
        flow = F.densify(dev(ia), dev(ib), dev(rec), segments=dev(seg), level=level).cpu().numpy()
        assert flow.shape == (n, 2, h, w)
        for i in range(n):
            err = np.abs(flow[i] - G.densify(ia[i], ib[i], rec[i], seg[i], level)).max()
            print(f"{kind} pair {i}: densify max |gpu - float64| = {err:.3e} (TOL {G.TOL:.3e})")
            assert err <= G.TOL, kind
        if kind == "halves" and level == 1:                           # a coarser level written at a larger size: 2 * f[y // 2, x // 2]
            big = F.densify(dev(ia), dev(ib), dev(rec), shift=1, out_size=(2 * h - 1, 2 * w), segments=dev(seg), level=level)
            yy, xx = np.arange(2 * h - 1)[:, None] // 2, np.arange(2 * w)[None] // 2
            assert np.array_equal(big.cpu().numpy(), 2 * flow[:, :, yy, xx])


@pytest.mark.parametrize("h,w,n,level,kw", G.refine_cases())
def test_refine_flow_vs_float64(h, w, n, level, kw):
    """The cut iterate kernel on every map, every stage size (at 8 x 8 every pixel is on the image border, and a level-1 case
    reads the last row of an odd-sized map) and six tiles (40 x 70), n 1 and 3, levels 0 and 1, sor 1 and 5, from the random
    level_pair flows.  Against float64 within the tolerance of the map, and against the float32 run of the restatement bit for
    bit: the same operations in the same order, sqrt and division correctly rounded on both sides, whatever tile computed a
    pixel.  The second is the sharp check where the cut makes the float64 tolerance wide."""
    for kind in G.MAPS:
        ia, ib, init, seg = G.stage_inputs(h, w, n, level, kind, G.REFINE_SEED)
        got = F.refine_flow(dev(ia), dev(ib), dev(init), segments=dev(seg), level=level, **kw).cpu().numpy()
        assert got.shape == (n, 2, h, w)
        for i in range(n):
            err = np.abs(got[i] - G.refine(ia[i], ib[i], init[i], seg[i], level, **kw)).max()
            print(f"{kind} pair {i}: max |gpu - float64| = {err:.3e} (TOL {G.REFINE_TOL[kind]:.3e})")
            assert err <= G.REFINE_TOL[kind], kind
            assert np.array_equal(got[i], G.refine(ia[i], ib[i], init[i], seg[i], level, dtype=np.float32, **kw)), (kind, i)
        if kind == "constant":                                        # no edge is cut: the unguided kernel's bits
            assert torch.equal(dev(got), F.refine_flow(dev(ia), dev(ib), dev(init), **kw))


def test_a_pixel_without_neighbours_on_a_flat_image_keeps_its_flow():
    flat = np.full((1, 16, 16), 97.0, np.float32)
    flow = np.random.default_rng(0).uniform(-1, 1, (1, 2, 16, 16)).astype(np.float32)
    got = F.refine_flow(dev(flat), dev(flat), dev(flow), segments=dev(G.id_map("checker", 16, 16)[None]))
    assert torch.equal(got, dev(flow))


# ------------------------------------------------------------------------------------------------ the whole call
@functools.lru_cache(maxsize=None)
def batch():
    """Three pairs at 37 x 70 (two levels) with their id maps: a moving object with its mask, blobs, and negative / large ids."""
    a0, b0, _, inside = NP.two_layer(37, 70, obj=(16, 24), motion=(2, -1))
    a1, b1, _, _ = NP.pair(NP.MOTIONS[0], 37, 70)
    a2, b2, _, _ = NP.pair(NP.MOTIONS[2], 37, 70)
    seg = np.stack([inside.astype(np.int32), G.id_map("blobs", 37, 70), G.id_map("wild", 37, 70)])
    return np.stack([a0, a1, a2]), np.stack([b0, b1, b2]), seg


@pytest.mark.parametrize("refine", [None, True])
def test_constant_ids_are_segments_none_bit_for_bit(refine):
    a, b, seg = batch()
    a, b = dev(a), dev(b)
    want = F.dense_flow(a, b, refine=refine)
    for value in (0, -5, 2 ** 31 - 1):
        ids = torch.full((3, 37, 70), value, device=DEV, dtype=torch.int32)
        assert torch.equal(F.dense_flow(a, b, refine=refine, segments=ids), want), value
    ids = torch.zeros(3, 37, 70, device=DEV, dtype=torch.int32)
    assert torch.equal(F.dense_flow(a, b, refine=refine, finest=1, segments=ids), F.dense_flow(a, b, refine=refine, finest=1))
    assert torch.equal(F.dense_flow(a.bfloat16(), b.bfloat16(), refine=refine, segments=ids),
                       F.dense_flow(a.bfloat16(), b.bfloat16(), refine=refine))
    assert not torch.equal(F.dense_flow(a, b, refine=refine, segments=dev(seg)), want)


@pytest.mark.parametrize("refine", [None, True])
def test_guided_flow_is_repeatable_independent_of_the_batch_and_close_to_float64(refine):
    a, b, seg = batch()
    da, db, ds = dev(a), dev(b), dev(seg)
    first = F.dense_flow(da, db, refine=refine, segments=ds)
    assert first.shape == (3, 2, 37, 70) and first.dtype == torch.float32 and torch.isfinite(first).all()
    assert torch.equal(F.dense_flow(da, db, refine=refine, segments=ds), first)            # bit for bit
    for i in range(3):
        assert torch.equal(F.dense_flow(da[i:i + 1], db[i:i + 1], refine=refine, segments=ds[i:i + 1])[0], first[i]), i
    # a map that is a non-contiguous view is the same call on its values
    wide = torch.cat([ds, ds], 2)
    assert torch.equal(F.dense_flow(da, db, refine=refine, segments=wide[:, :, :70]), first)
    # pair 0 (an object and its mask) against float64: the whole-flow condition of the unguided tests
    want = G.dense_flow(a[0], b[0], seg[0], refine_params=refine)
    diff = np.abs(first[0].cpu().numpy() - want).max(0)
    print(f"refine {refine}: max {diff.max():.3e}, pixels beyond 1e-3 px: {(diff > 1e-3).mean():.4%}")
    assert (diff > 1e-3).mean() <= 0.01
    coarse = F.dense_flow(da, db, refine=refine, finest=1, segments=ds)[0].cpu().numpy()
    diff = np.abs(coarse - G.dense_flow(a[0], b[0], seg[0], refine_params=refine, finest=1)).max(0)
    assert (diff > 1e-3).mean() <= 0.01


@pytest.mark.parametrize("refine", [None, True])
def test_guided_flow_runs_in_stream_order(refine):
    """On a side stream, right behind the producers of its inputs on that stream, with the producers held back."""
    a, b, seg = batch()
    want = F.dense_flow(dev(a), dev(b), refine=refine, segments=dev(seg))
    host = [torch.from_numpy(x).pin_memory() for x in (a, b, seg)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, want, dev(a))
        gpu_util.stretch(side, 20.0)
        da, db, ds = (h.to(DEV, non_blocking=True) for h in host)     # the producers: queued behind the delay
        got = F.dense_flow(da, db, refine=refine, segments=ds)
    side.synchronize()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ quality at the object's edge
@pytest.mark.parametrize("size,obj,motion", G.SCENES)
def test_guided_flow_recovers_the_object_up_to_its_edge(size, obj, motion):
    """The bounds of tests/test_guided_flow_cpu.py (its docstring has the float64 figures) on the GPU's flows."""
    a, b, true, inside, ids, far = G.scene(size, obj, motion)
    band = RF.object_masks(inside)[1]
    da, db, ds = dev(a)[None], dev(b)[None], dev(ids)[None]
    flows = dict(plain=F.dense_flow(da, db), guided=F.dense_flow(da, db, segments=ds), plain_refined=F.dense_flow(da, db, refine=True),
                 guided_refined=F.dense_flow(da, db, refine=True, segments=ds))
    e = {k: tuple(NP.epe(f[0].cpu().numpy().astype(np.float64), true, m) for m in (inside, band, far)) for k, f in flows.items()}
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


# ------------------------------------------------------------------------------------------------ a clip with its instance maps
@functools.lru_cache(maxsize=None)
def clip():
    video, inst = NP.moving_boxes_clip()
    return video, inst, dict(num_input_frames=G.CLIP_T_IN, num_predicted_frames=video.shape[1] - G.CLIP_T_IN, use_fw_of=True)


@pytest.mark.parametrize("refine", [None, True])
def test_clip_flows_and_chained_classic_flow_take_the_instance_maps(refine):
    """With the instance maps target_bw_of is within 0.1 px (mean endpoint error) of the truth over each whole box, band
    included, in every predicted frame (3 .. 15 px from the last input frame); without them the band alone exceeds that.
    tests/test_guided_flow_cpu.py checks the same on the float64 restatement and has its figures."""
    video, inst, tp = clip()
    t_in, t_out = tp["num_input_frames"], tp["num_predicted_frames"]
    batch_, ids = dict(video=dev(video)[None]), dev(inst)[None]
    cf = F.ClassicFlow(chain=True, refine=refine)
    guided = train.compute_flow(cf, batch_, tp, segments=ids)
    plain = train.compute_flow(cf, batch_, tp)
    assert guided.keys() == plain.keys()
    for k, v in plain.items():
        assert guided[k].shape == v.shape and guided[k].dtype == v.dtype and torch.isfinite(guided[k]).all(), k
    direct = F.clip_flows(dev(video)[None] * 2 - 1, t_in, t_out, True, (-1, 1), refine=refine, segments=ids)
    for k, v in guided.items():
        assert torch.equal(direct[k], v), k
    eg = G.clip_box_errors(guided["target_bw_of"][0].cpu().numpy().astype(np.float64), inst, t_in)
    ep = G.clip_box_errors(plain["target_bw_of"][0].cpu().numpy().astype(np.float64), inst, t_in)
    print("guided whole box", {k: round(v[0], 4) for k, v in eg.items()})
    print("unguided band", {k: round(v[1], 4) for k, v in ep.items()})
    assert max(v[0] for v in eg.values()) <= G.CLIP_BOUND
    assert min(v[1] for v in ep.values()) > G.CLIP_BOUND
    # constant ids are the unguided clip, bit for bit; one clip of a batch of two is the single clip
    const = train.compute_flow(cf, batch_, tp, segments=torch.zeros_like(ids))
    assert all(torch.equal(const[k], plain[k]) for k in plain)
    two = F.clip_flows(torch.cat([dev(video)[None], dev(video)[None].flip(3)]) * 2 - 1, t_in, t_out, True, (-1, 1), refine=refine,
                       segments=torch.cat([ids, ids.flip(2)]))
    assert all(torch.equal(two[k][0], guided[k][0]) for k in guided)


def test_unchained_compute_flow_guides_every_pair_by_its_first_frame():
    video, inst, tp = clip()
    t_in, t_out = tp["num_input_frames"], tp["num_predicted_frames"]
    v, ids = dev(video)[None], dev(inst)[None]
    got = train.compute_flow(F.ClassicFlow(), dict(video=v), tp, segments=ids)
    frame = lambda i: v[:, :, i] * 2 - 1
    # target_bw_of[k]: (target frame k -> last input frame), guided by the target frame's ids; target_fw_of: by the last input's
    for k in range(t_out):
        bw = F.dense_flow(frame(t_in + k), frame(t_in - 1), (-1, 1), segments=ids[:, t_in + k])
        fw = F.dense_flow(frame(t_in - 1), frame(t_in + k), (-1, 1), segments=ids[:, t_in - 1])
        assert torch.equal(got["target_bw_of"][:, :, k], bw) and torch.equal(got["target_fw_of"][:, :, k], fw), k
    assert torch.equal(got["input_of"][:, :, 0], F.dense_flow(frame(0), frame(1), (-1, 1), segments=ids[:, 0]))
    f5, c5 = F.ClassicFlow()(torch.stack([frame(0), frame(1)], 1), torch.stack([frame(1), frame(2)], 1), segments=ids[:, :2])
    assert f5.shape == (1, 2, 2, 64, 128) and c5.shape == (1, 2, 1, 64, 128) and torch.equal(f5[:, 0], got["input_of"][:, :, 0])


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    a = torch.zeros(2, 3, 16, 24, device=DEV)
    ids = torch.zeros(2, 16, 24, device=DEV, dtype=torch.int32)
    ia, fl = torch.zeros(2, 16, 24, device=DEV), torch.zeros(2, 2, 16, 24, device=DEV)
    bads = (ids.long(), ids.float(), ids[:1], ids[:, :15], ids[:, :, :23], ids[0], ids.cpu(), torch.zeros(2, 17, 24, device=DEV,
            dtype=torch.int32), "ids")
    for bad in bads:
        with pytest.raises(ValueError, match="segments"):
            F.dense_flow(a, a, segments=bad)
        with pytest.raises(ValueError, match="segments"):
            F.ClassicFlow()(a, a, segments=bad)
    for bad in (ids.long(), ids[:1], ids[:, :15], ids.cpu(), ids[0]):
        with pytest.raises(ValueError, match="segments"):
            F.patch_search(ia, ia, segments=bad)
        with pytest.raises(ValueError, match="segments"):
            F.densify(ia, ia, torch.zeros(2, 3, 5, 4, device=DEV), segments=bad)
        with pytest.raises(ValueError, match="segments"):
            F.refine_flow(ia, ia, fl, segments=bad)
    for level, shape in ((1, (2, 30, 47)), (1, (2, 31, 46)), (7, (2, 16, 24)), (-1, (2, 16, 24))):
        with pytest.raises(ValueError, match="segments"):            # (16 - 1) << 1 = 30 is past a map of 30 rows
            F.patch_search(ia, ia, segments=torch.zeros(shape, device=DEV, dtype=torch.int32), level=level)
    assert F.patch_search(ia, ia, segments=torch.zeros(2, 31, 47, device=DEV, dtype=torch.int32), level=1).shape == (2, 3, 5, 4)
    with pytest.raises(ValueError, match="records must be"):         # a guided densify wants records of 4 floats
        F.densify(ia, ia, torch.zeros(2, 3, 5, 3, device=DEV), segments=ids)
    video = torch.zeros(1, 3, 4, 16, 24, device=DEV)
    for bad in (torch.zeros(1, 4, 16, 24, device=DEV), torch.zeros(1, 3, 16, 24, device=DEV, dtype=torch.int32),
                torch.zeros(1, 4, 16, 24, dtype=torch.int32)):
        with pytest.raises(ValueError, match="segments"):
            F.clip_flows(video, 2, 2, segments=bad)
        for chain in (False, True):                                   # compute_flow checks them itself, before it queues anything
            with pytest.raises(ValueError, match="segments must be"):
                train.compute_flow(F.ClassicFlow(chain=chain), dict(video=video), dict(num_input_frames=2, num_predicted_frames=2),
                                   segments=bad)
    # a flow module that takes no segments: FlowNet
    from c2m_amd.modules.third_party.flow_net.flow_net import FlowNet
    with pytest.raises(ValueError, match="segments"):
        train.compute_flow(FlowNet(pretrained=False), dict(video=video), dict(num_input_frames=2, num_predicted_frames=2),
                           segments=torch.zeros(1, 4, 16, 24, device=DEV, dtype=torch.int32))
