"""Results at dataset resolution on the GPU (run with -m gpu): ops.detail_warp against the float64 restatement of
tests/fullres_np.py, then c2m_amd.fullres on a two-segment rollout of the small model of test_gpu_click_to_move.py.

Bounds.  Levels: a pixel whose float64 clip(v) lies within 0.02 levels of a rounding boundary k + 0.5 may differ by one level,
every other pixel is equal; 0.02 covers fp32 evaluation at these sizes (a coordinate ulp times a neighbour step of the frame is
about 2e-3 levels).  The exempt share is measured on the reference alone and must stay at or below 6 % (a uniform fractional part
gives 4 %).  Ids: equal except where the float64 IX or IY is within 1e-3 of a half-integer (a rounding tie of the nearest
pixel) or the enlarged occlusion map within 1e-6 of the threshold, at most 2 % of the pixels, again measured on the reference
alone; fill_id below the threshold is exact.  Each test prints its shares before it asserts."""
import numpy as np
import pytest
import torch

import fullres_np as R
from c2m_amd import data, fullres, ops
from c2m_amd import interactive as I
from test_gpu_click_to_move import DRAGS, T_OUT, inputs, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIE, TIE_SHARE = 0.02, 0.06
ID_TIE, ID_TIE_SHARE = 1e-3, 0.02
# (h, w) -> (H, W), B, T.  The first five: scale 1; one axis enlarged only; ragged tiles in both axes; factor 2.5; factor 8, the
# workload's own.  A tile is 4 rows of 256 pixels and a thread owns 4 of them, stored as dwords when W % 4 == 0 and as bytes
# otherwise: the last two span three tiles in x, one per store form.
SHAPES = [((9, 13), (9, 13), 2, 2), ((9, 13), (9, 40), 1, 1), ((9, 13), (37, 53), 2, 2), ((6, 10), (15, 25), 1, 2),
          ((8, 16), (64, 128), 2, 2), ((6, 70), (11, 530), 1, 2), ((6, 70), (9, 520), 2, 1)]
_cases = {}


def case(i):
    """Inputs and float64 reference of SHAPES[i], computed once and never modified."""
    if i not in _cases:
        (h, w), (H, W), B, T = SHAPES[i]
        c = R.make_case(h, w, H, W, B, T, seed=100 + i)
        c["ref"] = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], c["occ"], c["ids"], 0.35, -3)
        _cases[i] = c
    return _cases[i]


def dev(c, *keys):
    return [None if k is None else torch.from_numpy(c[k]).to(DEV) for k in keys]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def levels_close(got, ref, what):
    assert got.shape == ref["levels"].shape and got.dtype == np.uint8, what
    d = np.abs(got.astype(np.int64) - ref["levels"].astype(np.int64))
    near = R.boundary_distance(ref["v"]) <= TIE
    print(f"{what}: {int((d > 0).sum())} of {d.size} values differ, max {d.max()} levels; exempt share {near.mean():.4f}, "
          f"differing outside it {int((d[~near] > 0).sum())}")
    assert near.mean() <= TIE_SHARE, what
    assert d.max() <= 1, what
    assert not d[~near].any(), what


def ids_close(got, ref, what, threshold=None):
    assert got.shape == ref["ids"].shape and got.dtype == np.int32, what
    tie = lambda a: np.abs(a - np.floor(a) - 0.5) <= ID_TIE
    near = tie(ref["IX"]) | tie(ref["IY"])
    if threshold is not None:               # up(occ) is a convex combination of values in [0, 1]: fp32 is within 1e-6 of it
        near |= np.abs(ref["occ_up"] - threshold) <= 1e-6
    bad = got != ref["ids"]
    print(f"{what}: {int(bad.sum())} of {bad.size} ids differ; exempt share {near.mean():.4f}, differing outside it "
          f"{int(bad[~near].sum())}")
    assert near.mean() <= ID_TIE_SHARE, what
    assert not bad[~near].any(), what


# ------------------------------------------------------------------------------------------------ kernel vs float64
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b, _, _ in SHAPES])
def test_kernel_vs_float64(i):
    c = case(i)
    (h, w), (H, W), B, T = SHAPES[i]
    F, G, Wl, flow, occ, ids = dev(c, "F", "G", "Wl", "flow", "occ", "ids")
    keep = [t.clone() for t in (F, G, Wl, flow, occ, ids)]
    out, oid = ops.detail_warp(F, G, Wl, flow, occ, ids, 0.35, -3)
    assert out.shape == (B, T, H, W, 3) and out.dtype == torch.uint8 and out.is_cuda
    assert oid.shape == (B, T, H, W) and oid.dtype == torch.int32
    levels_close(host(out), c["ref"], f"{SHAPES[i]}")
    ids_close(host(oid), c["ref"], f"{SHAPES[i]} ids", 0.35)
    low = c["ref"]["occ_up"] < 0.35 - 1e-5                          # fill_id under the threshold is exact
    assert low.any() and (host(oid)[low] == -3).all()
    assert all(torch.equal(a, b) for a, b in zip(keep, (F, G, Wl, flow, occ, ids)))          # inputs not modified
    # the same bits again, and on another stream
    again, again_id = ops.detail_warp(F, G, Wl, flow, occ, ids, 0.35, -3)
    assert torch.equal(again, out) and torch.equal(again_id, oid)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, other_id = ops.detail_warp(F, G, Wl, flow, occ, ids, 0.35, -3)
    side.synchronize()
    assert torch.equal(other, out) and torch.equal(other_id, oid)
    # frames alone; ids without a threshold
    alone, none = ops.detail_warp(F, G, Wl, flow, occ)
    assert none is None and torch.equal(alone, out)
    _, plain = ops.detail_warp(F, G, Wl, flow, occ, ids)
    ids_close(host(plain), R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], c["occ"], c["ids"]), f"{SHAPES[i]} ids, no fill")


def test_occ_none_bf16_and_strided_inputs():
    c = case(2)
    F, G, Wl, flow, occ = dev(c, "F", "G", "Wl", "flow", "occ")
    ref = R.detail_warp(c["F"], c["G"], c["Wl"], c["flow"], None)
    levels_close(host(ops.detail_warp(F, G, Wl, flow)[0]), ref, "occ=None")
    Gb, Wb, ob = G.bfloat16(), Wl.bfloat16(), occ.bfloat16()
    assert torch.equal(ops.detail_warp(F, Gb, Wb, flow, ob)[0], ops.detail_warp(F, Gb.float(), Wb.float(), flow, ob.float())[0])
    wide = torch.zeros(2, 3, 4, 9, 13, device=DEV)
    wide[:, :, 1:3] = G
    assert torch.equal(ops.detail_warp(F, wide[:, :, 1:3], Wl, flow, occ)[0], ops.detail_warp(F, G, Wl, flow, occ)[0])


def test_wild_flows_read_in_bounds_and_match_the_definition():
    """NaN, +inf, -inf and 1e30 in a few flow elements, at factor 8 where the taps of the enlargement are exact in fp32 as in
    float64, so a non-finite tap spreads to the same output pixels on both sides."""
    c = dict(case(4))
    flow = c["flow"].copy()
    flow[0, 0, 0, 2, 3], flow[0, 1, 0, 5, 9], flow[1, 0, 1, 1, 1], flow[1, 1, 1, 6, 12] = np.nan, np.inf, -np.inf, 1e30
    flow[1, 0, 0, 4, 4], flow[1, 0, 0, 4, 5] = np.inf, -np.inf
    flow[0, 0, 1, 0, 0], flow[0, 1, 1, 7, 15] = -1e30, np.nan
    c["flow"] = flow
    ref = R.detail_warp(c["F"], c["G"], c["Wl"], flow, c["occ"], c["ids"], 0.35, -3)
    F, G, Wl, fl, occ, ids = dev(c, "F", "G", "Wl", "flow", "occ", "ids")
    out, oid = ops.detail_warp(F, G, Wl, fl, occ, ids, 0.35, -3)
    levels_close(host(out), ref, "wild flows")
    ids_close(host(oid), ref, "wild flows, ids", 0.35)


def test_offsets_past_2_31():
    """2.2e9 output bytes: the last frame equals the same frame computed alone."""
    B, T, h, w, H, W = 1, 44, 16, 16, 4096, 4096
    g = torch.Generator().manual_seed(3)
    F = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    G, Wl = torch.rand(B, 3, T, h, w, generator=g).to(DEV), torch.rand(B, 3, T, h, w, generator=g).to(DEV)
    flow, occ = (torch.randn(B, 2, T, h, w, generator=g) * 1.5).to(DEV), torch.rand(B, 1, T, h, w, generator=g).to(DEV)
    out, _ = ops.detail_warp(F, G, Wl, flow, occ)
    assert out.numel() > 2 ** 31
    for t in (0, T - 1):
        s = slice(t, t + 1)
        one, _ = ops.detail_warp(F, G[:, :, s], Wl[:, :, s], flow[:, :, s], occ[:, :, s])
        assert torch.equal(out[:, t], one[:, 0]), t
    assert not torch.equal(out[:, 0], out[:, T - 1])


def test_arguments_are_checked_before_any_launch():
    c = case(0)
    F, G, Wl, flow, occ, ids = dev(c, "F", "G", "Wl", "flow", "occ", "ids")
    with pytest.raises(ValueError):
        ops.detail_warp(F, G, Wl, flow[..., :12], occ)
    with pytest.raises(ValueError):
        ops.detail_warp(F.float(), G, Wl, flow, occ)
    with pytest.raises(ValueError):
        ops.detail_warp(F, G, Wl, flow, None, ids, 0.5)
    with pytest.raises(ValueError):
        ops.detail_warp(F, G, Wl, flow, occ, ids, 0.5, fill_id=2 ** 31)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.detail_warp(F.cpu(), G, Wl, flow, occ)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def rolled():
    """A two-segment rollout of the small model whose video comes from uint8 frames through data.prep_video, so f = F / 255."""
    B, t_in = 2, 1
    batch = inputs(B, t_in)
    frames = (batch["video"].permute(0, 2, 3, 4, 1) * 255).round().clamp(0, 255).to(torch.uint8).contiguous()
    video = data.prep_video(frames)
    model = small_model(t_in)
    zs = torch.randn(2, B, model.motion_encoder.fc.in_features, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(21)
    r = I.rollout(model, video, batch["bg_mask"], batch["fg_mask"], batch["instance_mask"], [DRAGS, []], z_m=zs)
    g = torch.Generator().manual_seed(5)
    big = frames[:, t_in - 1].repeat_interleave(2, 1).repeat_interleave(2, 2).to(torch.int16)
    big = (big + torch.randint(-30, 31, big.shape, generator=g, dtype=torch.int16).to(DEV)).clamp(0, 255).to(torch.uint8)
    ids_big = batch["instance_mask"][:, 0, t_in - 1].repeat_interleave(2, 1).repeat_interleave(2, 2).to(torch.int32).contiguous()
    torch.cuda.synchronize()
    return dict(r=r, video=video, frames=frames, t_in=t_in, big=big.contiguous(), ids_big=ids_big)


def test_upscale_at_the_working_size_is_the_generator_output(rolled):
    """H = h, W = w and f = F / 255: the full-size warp reads what the working-size warp read, so nothing is added."""
    out, t_in = rolled["r"]["outputs"][0], rolled["t_in"]
    got, none = fullres.upscale(out, rolled["video"], rolled["frames"][:, t_in - 1].contiguous(), t_in)
    assert none is None and got.shape == (2, T_OUT, 128, 256, 3)
    v = 255.0 * host(out["generated"]).astype(np.float64).transpose(0, 2, 3, 4, 1)
    ref = dict(v=v, levels=np.floor(np.clip(v, 0, 255) + 0.5).astype(np.uint8))
    levels_close(host(got), ref, "upscale at 128x256")


def test_upscale_at_twice_the_size_is_detail_warp_by_hand(rolled):
    out, t_in, video = rolled["r"]["outputs"][0], rolled["t_in"], rolled["video"]
    got, gid = fullres.upscale(out, video, rolled["big"], t_in, rolled["ids_big"], occ_threshold=0.5, fill_id=-1)
    assert got.shape == (2, T_OUT, 256, 512, 3) and gid.shape == (2, T_OUT, 256, 512)
    flow = out["dense_motion_bw"]
    warped = torch.stack([ops.flow_warp(video[:, :, t_in - 1].contiguous(), flow[:, :, t].contiguous())
                          for t in range(T_OUT)], 2)
    want, wid = ops.detail_warp(rolled["big"], out["generated"], warped, flow, out["occlusion_bw"], rolled["ids_big"], 0.5, -1)
    assert torch.equal(got, want) and torch.equal(gid, wid)
    sparse, _ = fullres.upscale(out, video, rolled["big"], t_in, flow="sparse_motion_bw")
    warped = torch.stack([ops.flow_warp(video[:, :, t_in - 1].contiguous(), out["sparse_motion_bw"][:, :, t].contiguous())
                          for t in range(T_OUT)], 2)
    want, _ = ops.detail_warp(rolled["big"], out["generated"], warped, out["sparse_motion_bw"], out["sparse_occ_bw"])
    assert torch.equal(sparse, want) and not torch.equal(sparse, got)


def test_upscale_rollout_chains_the_segments(rolled):
    r, t_in, video, big, ids_big = (rolled[k] for k in ("r", "t_in", "video", "big", "ids_big"))
    got, gid = fullres.upscale_rollout(r, video, big, t_in, ids_big, occ_threshold=0.5, fill_id=-1)
    assert got.shape == (2, 2 * T_OUT, 256, 512, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert gid.shape == (2, 2 * T_OUT, 256, 512) and gid.dtype == torch.int32
    a, aid = fullres.upscale(r["outputs"][0], video, big, t_in, ids_big, occ_threshold=0.5, fill_id=-1)
    partner = r["generated"][:, :, T_OUT - 1:T_OUT]
    b, bid = fullres.upscale(r["outputs"][1], partner, a[:, -1].contiguous(), 1, aid[:, -1].contiguous(), occ_threshold=0.5,
                             fill_id=-1)
    assert torch.equal(got[:, :T_OUT], a) and torch.equal(gid[:, :T_OUT], aid)
    assert torch.equal(got[:, T_OUT:], b) and torch.equal(gid[:, T_OUT:], bid)
    broken, _ = fullres.upscale(r["outputs"][1], partner, big, 1)                   # warped from the original frame instead
    assert not torch.equal(got[:, T_OUT:], broken)
    frames_only, none = fullres.upscale_rollout(r, video, big, t_in)
    assert none is None and torch.equal(frames_only, got)
