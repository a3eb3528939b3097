"""The block-matching seed of the dense flow on the GPU (run with -m gpu): fl_patch_match_kernel, unguided and guided, against the
float64 restatement (tests/flow_seed_np.py): the chosen displacement exactly, outside the few patches on which float32 may
choose otherwise (tests/test_flow_seed_cpu.py holds their share within the cap; it is zero on these inputs); dense_flow(seed=)
against the seeded float64 flow within the tolerances that the CPU test derives, and within the endpoint errors it asserts;
seed=None against the call without the argument bit for bit; repeatability, independence of the batch, stream order, bf16;
ClassicFlow(seed=) and clip_flows(seed=) through train.compute_flow; the launchers' refusals."""
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as NP
import flow_seed_np as S
import gpu_util
from c2m_amd import _lib, flow as F
from c2m_amd import train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the stage
def check_records(got, ia, ib, radius, seg=None, level=0):
    """got [n,npy,npx,3 or 4] of the GPU against float64: (dx, dy) exact outside seed_excluded, the third field within NP.TOL, n
    exact; the excluded patches within the cap."""
    n, (h, w) = len(ia), ia.shape[1:]
    assert got.shape == (n, len(NP.origins(h)), len(NP.origins(w)), 3 if seg is None else 4)
    left = 0
    for i in range(n):
        rec, det, thr, gap = S.patch_match(ia[i], ib[i], radius, None if seg is None else seg[i], level, details=True)
        keep = ~S.seed_excluded(det, thr, gap)
        left += int((~keep).sum())
        assert np.array_equal(got[i][keep][:, :2], rec[keep][:, :2]), (i, radius)
        err = np.abs(got[i][keep][:, 2] - rec[keep][:, 2])
        print(f"radius {radius} pair {i}: third field max |gpu - float64| = {err.max() if err.size else 0:.3e} (TOL {NP.TOL:.3e}); "
              f"smallest gap {gap.min():.2e}")
        assert (err <= NP.TOL).all()
        if seg is not None:
            assert np.array_equal(got[i][..., 3], rec[..., 3])
    assert left <= S.EXCLUDED_CAP * got[..., 0].size


@pytest.mark.parametrize("h,w,n,corner,leave", S.stage_cases())
def test_patch_match_vs_float64(h, w, n, corner, leave):
    ia, ib = S.stage_inputs(h, w, n, corner, leave)
    for radius in S.RADII:
        check_records(F.patch_match(dev(ia), dev(ib), radius).cpu().numpy(), ia, ib, radius)
    if (h, w) == (8, 8):                                              # one window fits: nothing moves
        assert not F.patch_match(dev(ia), dev(ib), 8)[..., :2].any()


@pytest.mark.parametrize("h,w,n,level", S.guided_stage_cases())
def test_guided_patch_match_vs_float64(h, w, n, level):
    for kind in S.GUIDED_MAPS:
        ia, ib, seg = S.guided_stage_inputs(h, w, n, level, kind)
        for radius in S.RADII:
            got = F.patch_match(dev(ia), dev(ib), radius, segments=dev(seg), level=level)
            check_records(got.cpu().numpy(), ia, ib, radius, seg, level)
    # one id everywhere: the bits of the unguided kernel, n = 64
    one = torch.full(seg.shape, -7, device=DEV, dtype=torch.int32)
    for radius in S.RADII:
        got, plain = F.patch_match(dev(ia), dev(ib), radius, segments=one, level=level), F.patch_match(dev(ia), dev(ib), radius)
        assert torch.equal(got[..., :3], plain) and (got[..., 3] == 64).all()


def test_patch_match_on_many_workgroups():
    """N = 3 at 64 x 128: 1395 patches, 349 workgroups, the last one with three live waves of four."""
    h, w, n = S.GRID_STRIDE
    ia, ib = S.stage_inputs(h, w, n, False, True)
    got = F.patch_match(dev(ia), dev(ib))
    check_records(got.cpu().numpy(), ia, ib, S.SEED_RADIUS)
    assert torch.equal(F.patch_match(dev(ia), dev(ib)), got)
    for i in range(n):                                                # a pair does not depend on the others
        assert torch.equal(F.patch_match(dev(ia[i:i + 1]), dev(ib[i:i + 1]))[0], got[i])
    out = torch.full((n, 15, 31, 3), float("nan"), device=DEV)
    assert F.patch_match(dev(ia), dev(ib), out=out) is out and torch.equal(out, got)


@pytest.mark.parametrize("first,second,winner", [((-5, 0), (4, 0), (4, 0)), ((5, -5), (-5, 5), (5, -5)),
                                                 ((5, 0), (-5, 0), (-5, 0))])
def test_equal_costs_are_decided_by_the_rest_of_the_key(first, second, winner):
    """Two exact copies of the patch in b (tests/test_flow_seed_cpu.py): equal costs in two lanes of the wave."""
    ia = (255 * NP.texture(24, 24, 3, channels=1)[0]).astype(np.float32)
    ib = np.full((24, 24), 100.0, np.float32)
    for dx, dy in (first, second):
        ib[8 + dy:16 + dy, 8 + dx:16 + dx] = ia[8:16, 8:16]
    got = F.patch_match(dev(ia)[None], dev(ib)[None], 8)[0, 2, 2].tolist()
    assert tuple(got[:2]) == winner and abs(got[2]) <= 1e-3
    assert tuple(S.patch_match(ia, ib, 8)[2, 2, :2]) == winner


# ------------------------------------------------------------------------------------------------ the whole flow
@functools.lru_cache(maxsize=None)
def whole(name):
    """(case, float64 seeded flow) of a whole-flow case, computed once."""
    build, kw, _ = S.WHOLE[name]
    c = build()
    return c, S.dense_flow(c["a"], c["b"], seg=c["seg"], levels=c["levels"], **kw)


@pytest.mark.parametrize("name", list(S.WHOLE))
def test_seeded_dense_flow_vs_float64(name):
    c, want = whole(name)
    kw = dict(levels=c["levels"], refine=S.WHOLE[name][1].get("refine_params"))
    if c["seg"] is not None:
        kw["segments"] = dev(c["seg"])[None]
    got = F.dense_flow(dev(c["a"])[None], dev(c["b"])[None], seed=True, **kw)
    assert got.shape == (1, 2) + c["a"].shape[1:] and got.dtype == torch.float32
    got = got[0].cpu().numpy().astype(np.float64)
    err, e = np.abs(got - want).max(), NP.epe(got, c["true"], c["mask"])
    print(f"{name}: max |gpu - float64| = {err:.3e} (TOL {S.WHOLE_TOL[name]:.3e}); EPE {e:.4f}")
    assert err <= S.WHOLE_TOL[name]
    if S.WHOLE[name][2] is not None:
        assert e <= S.WHOLE[name][2]
    assert torch.equal(F.dense_flow(dev(c["a"])[None], dev(c["b"])[None], seed=S.SEED_RADIUS, **kw)[0], dev(got.astype(np.float32)))


def test_seeded_dense_flow_recovers_25_px_at_128_x_256():
    c = S.FAST["128x256 shift (25, 0)"]()
    a, b = dev(c["a"])[None], dev(c["b"])[None]
    seeded, plain = (NP.epe(F.dense_flow(a, b, seed=s)[0].cpu().numpy().astype(np.float64), c["true"], c["mask"])
                     for s in (True, None))
    print(f"128 x 256 shift (25, 0): unseeded {plain:.3f} seeded {seeded:.3f}")
    assert seeded <= S.SEEDED_MAX and plain > S.FAST_MIN


# ------------------------------------------------------------------------------------------------ the other properties
@functools.lru_cache(maxsize=None)
def batch():
    """Three pairs at 37 x 70 (two levels): a fast shift, a fast object with its mask, a small motion."""
    a0, b0 = (S.FAST["37x70 shift (9, 5)"]()[k] for k in ("a", "b"))
    a1, b1, _, inside = NP.two_layer(37, 70, obj=(12, 12), motion=(7, 3))
    a2, b2, _, _ = NP.pair(NP.MOTIONS[0], 37, 70)
    seg = np.stack([np.zeros((37, 70), np.int32), inside.astype(np.int32), np.full((37, 70), 3, np.int32)])
    return np.stack([a0, a1, a2]), np.stack([b0, b1, b2]), seg


@pytest.mark.parametrize("refine", [None, True])
@pytest.mark.parametrize("guided", [False, True])
def test_seed_none_is_the_call_without_it_and_a_seed_is_repeatable_and_batch_independent(refine, guided):
    a, b, seg = batch()
    da, db = dev(a), dev(b)
    kw = dict(refine=refine, **(dict(segments=dev(seg)) if guided else {}))
    want = F.dense_flow(da, db, **kw)
    for off in (None, False):
        assert torch.equal(F.dense_flow(da, db, seed=off, **kw), want)
    first = F.dense_flow(da, db, seed=True, **kw)
    assert first.shape == (3, 2, 37, 70) and torch.isfinite(first).all() and not torch.equal(first, want)
    assert torch.equal(F.dense_flow(da, db, seed=True, **kw), first) and torch.equal(F.dense_flow(da, db, seed=4, **kw), first)
    for i in range(3):
        one = {k: (v[i:i + 1] if k == "segments" else v) for k, v in kw.items()}
        assert torch.equal(F.dense_flow(da[i:i + 1], db[i:i + 1], seed=True, **one)[0], first[i]), i
    # one level (the coarsest level is level 0, which has no flow slot in the workspace) and a search that stops at level 1
    for extra in (dict(levels=1), dict(finest=1)):
        again = F.dense_flow(da, db, seed=True, **extra, **kw)
        assert torch.equal(F.dense_flow(da, db, seed=True, **extra, **kw), again) and torch.isfinite(again).all()
        assert torch.equal(F.dense_flow(da[1:2], db[1:2], seed=True, **extra,
                                        **{k: (v[1:2] if k == "segments" else v) for k, v in kw.items()})[0], again[1])
    if guided:                                                        # one id everywhere: the bits of the unguided seeded flow
        ids = torch.full((3, 37, 70), 9, device=DEV, dtype=torch.int32)
        assert torch.equal(F.dense_flow(da, db, seed=True, refine=refine, segments=ids),
                           F.dense_flow(da, db, seed=True, refine=refine))
    # bf16 frames are the same call on their fp32 values
    assert torch.equal(F.dense_flow(da.bfloat16(), db.bfloat16(), seed=True, **kw),
                       F.dense_flow(da.bfloat16().float(), db.bfloat16().float(), seed=True, **kw))


def test_one_level_seeded_flow_vs_float64():
    """levels = 1: the seed's dense flow lives in a buffer of the host's."""
    c = S.pair_case((33, 65), ("shift", (3.0, -2.0)), levels=1)
    got = F.dense_flow(dev(c["a"])[None], dev(c["b"])[None], levels=1, seed=True)[0].cpu().numpy()
    diff = np.abs(got - S.dense_flow(c["a"], c["b"], levels=1)).max(0)
    print(f"max {diff.max():.3e}, pixels beyond 1e-3 px: {(diff > 1e-3).mean():.4%}")
    assert (diff > 1e-3).mean() <= 0.01


def test_seeded_flow_runs_in_stream_order():
    """On a side stream, right behind the producers of its inputs on that stream, with the producers held back."""
    a, b, seg = batch()
    want = F.dense_flow(dev(a), dev(b), seed=True, segments=dev(seg))
    host = [torch.from_numpy(x).pin_memory() for x in (a, b, seg)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, want, dev(a))
        gpu_util.stretch(side, 20.0)
        da, db, ds = (h.to(DEV, non_blocking=True) for h in host)     # the producers: queued behind the delay
        got = F.dense_flow(da, db, seed=True, segments=ds)
    side.synchronize()
    assert torch.equal(got, want)


def test_classic_flow_and_clip_flows_take_the_seed():
    """moving_boxes_clip with every second frame dropped: the boxes move 6 px a frame, 1.5 px at the coarsest level."""
    video, inst = NP.moving_boxes_clip()
    video, inst = video[:, ::2], inst[::2]
    tp = dict(num_input_frames=2, num_predicted_frames=2, use_fw_of=True)
    v, ids = dev(video)[None], dev(inst)[None]
    for chain in (False, True):
        cf = F.ClassicFlow(chain=chain, seed=True)
        got = train.compute_flow(cf, dict(video=v), tp, segments=ids)
        plain = train.compute_flow(F.ClassicFlow(chain=chain), dict(video=v), tp, segments=ids)
        assert got.keys() == plain.keys()
        for k in plain:
            assert got[k].shape == plain[k].shape and torch.isfinite(got[k]).all(), k
        assert not torch.equal(got["target_bw_of"], plain["target_bw_of"])
        frame = lambda i: v[:, :, i] * 2 - 1
        assert torch.equal(got["input_of"][:, :, 0], F.dense_flow(frame(0), frame(1), (-1, 1), segments=ids[:, 0], seed=True))
    direct = F.clip_flows(v * 2 - 1, 2, 2, True, (-1, 1), segments=ids, seed=True)
    assert all(torch.equal(direct[k], got[k]) for k in got)
    flow, conf = F.ClassicFlow(seed=2)(v[:, :, 0] * 2 - 1, v[:, :, 1] * 2 - 1)
    assert torch.equal(flow, F.dense_flow(v[:, :, 0] * 2 - 1, v[:, :, 1] * 2 - 1, (-1, 1), seed=2))
    assert conf.shape == (1, 1, 64, 128)


# ------------------------------------------------------------------------------------------------ refusals
def test_launcher_refuses_before_any_launch():
    L = _lib.lib()
    ia = torch.rand(1, 16, 16, device=DEV) * 255
    rec = torch.full((3 * 3 * 3 + 1,), -1.0, device=DEV)

    def match(radius=4, a=ia.data_ptr(), b=ia.data_ptr(), elems=256, r=rec.data_ptr(), relems=27, N=1, h=16, w=16):
        return L.c2m_flow_patch_match(a, b, elems, r, relems, N, h, w, radius, None)

    for rc in (match(radius=0), match(radius=9), match(elems=255), match(relems=26), match(a=ia.data_ptr() + 2),
               match(b=ia.data_ptr() + 2), match(r=rec.data_ptr() + 2), match(a=None), match(r=None), match(h=7), match(N=-1)):
        assert rc != 0
    assert match(N=0) == 0
    torch.cuda.synchronize()
    assert (rec == -1).all()                                          # nothing was launched
    assert match() == 0
    torch.cuda.synchronize()
    assert (rec[:27] != -1).any() and rec[27] == -1
    a = torch.zeros(2, 3, 16, 24, device=DEV)
    for bad in (0, 9, 4.0, "4"):
        with pytest.raises(ValueError, match="seed must be"):
            F.dense_flow(a, a, seed=bad)
    for bad in (0, 9, True, 4.0):
        with pytest.raises(ValueError, match="radius"):
            F.patch_match(a[:, 0], a[:, 0], bad)
    with pytest.raises(ValueError, match="segments"):
        F.patch_match(a[:, 0], a[:, 0], segments=torch.zeros(2, 16, 24, device=DEV))
