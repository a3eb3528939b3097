"""Dense inverse search flow on the GPU (run with -m gpu): every kernel of csrc/dense_flow.hip against the numpy restatement
(tests/dense_flow_np.py), within the tolerance that tests/test_dense_flow_cpu.py derives from the reference's own float32 error;
repeatability, independence of the batch, stream order; ClassicFlow behind FlowNet's call surface; and frames -> flow -> tracks
with a computed flow."""
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as NP
import gpu_util
import tracking_np
from c2m_amd import flow as F
from c2m_amd import ops, tracking, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def full_case(size, motion):
    """(a, b, float64 reference flow) of a full-flow case, computed once and left unchanged."""
    a, b, _, _ = NP.pair(motion, *size)
    ref = NP.dense_flow(a, b)
    ref.setflags(write=False)
    return a, b, ref


# ------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("size", [(8, 8), (9, 13), (33, 65), (37, 70)])
@pytest.mark.parametrize("dtype,value_range", [(torch.float32, (0, 1)), (torch.float32, (-1, 1)), (torch.bfloat16, (0, 1))])
def test_pyramid_vs_numpy(size, dtype, value_range):
    H, W = size
    N = 2
    lo, hi = value_range
    rng = np.random.default_rng(H * W)
    a = torch.from_numpy((lo + (hi - lo) * rng.random((N, 3, H, W))).astype(np.float32)).to(dtype)
    b = torch.from_numpy((lo + (hi - lo) * rng.random((N, 3, H, W))).astype(np.float32)).to(dtype)
    work, sizes, images = F.flow_pyramid(a.to(DEV), b.to(DEV), value_range)
    assert sizes == NP.pyramid_sizes(H, W) and len(images) == len(sizes) == (2 if H > 32 else 1)
    for which, src in enumerate((a, b)):
        for n in range(N):
            want = NP.pyramid(NP.gray(src[n].float().numpy(), value_range, np.float32))
            for l, (h, w) in enumerate(sizes):
                got = images[l][which][n].cpu().numpy()
                assert got.shape == (h, w) == want[l].shape
                np.testing.assert_allclose(got, want[l], rtol=1e-6, atol=0)


def test_pyramid_level_cap_and_a_tile_edge():
    """Three levels at a size that is no multiple of the 64-pixel tile (two tiles a side), and the `levels` cap."""
    H, W, N = 70, 130, 1
    rng = np.random.default_rng(5)
    a, b = (torch.from_numpy(rng.random((N, 3, H, W)).astype(np.float32)) for _ in range(2))
    _, sizes, images = F.flow_pyramid(a.to(DEV), b.to(DEV))
    assert sizes == [(70, 130), (35, 65), (18, 33)]
    want = NP.pyramid(NP.gray(b[0].numpy(), (0, 1), np.float32))
    for l in range(3):
        np.testing.assert_allclose(images[l][1][0].cpu().numpy(), want[l], rtol=1e-6, atol=0)
    assert F.flow_pyramid(a.to(DEV), b.to(DEV), levels=2)[1] == sizes[:2]


# ------------------------------------------------------------------------------------------------ patch search, densify
@pytest.mark.parametrize("h,w,n,corner,leave", NP.search_cases())
def test_patch_search_vs_float64(h, w, n, corner, leave):
    ia, ib, init = NP.level_pair(h, w, n, corner, leave)
    got = F.patch_search(dev(ia), dev(ib), dev(init)).cpu().numpy()
    npy, npx = len(NP.origins(h)), len(NP.origins(w))
    assert got.shape == (n, npy, npx, 3)
    left_out = 0
    for i in range(n):
        want, det, d2 = NP.patch_search(ia[i], ib[i], init[i], details=True)
        keep = ~NP.excluded(det, d2)
        left_out += int((~keep).sum())
        err = np.abs(got[i] - want)[keep]
        print(f"pair {i}: max |gpu - float64| = {err.max() if err.size else 0:.3e} (TOL {NP.TOL:.3e})")
        assert (err <= NP.TOL).all()
        if corner:                                                   # det = 0 exactly: the patch keeps its initial flow, bit for bit
            assert got[i, 0, 0, 0] == init[i, 0, 3, 3] and got[i, 0, 0, 1] == init[i, 1, 3, 3]
    assert left_out <= 0.02 * n * npy * npx


def test_patch_search_initial_flow_forms():
    """No initial flow is a zero flow; a coarser flow is read as 2 * f[y // 2, x // 2], the up-sampling fused into the read."""
    h, w, n = 21, 37, 2
    ia, ib, _ = NP.level_pair(h, w, n, False, False)
    zero = F.patch_search(dev(ia), dev(ib), torch.zeros(n, 2, h, w, device=DEV))
    assert torch.equal(F.patch_search(dev(ia), dev(ib)), zero)
    coarse = np.random.default_rng(2).uniform(-1.5, 1.5, (n, 2, 11, 19)).astype(np.float32)
    up = np.stack([NP.upsample(coarse[i], h, w) for i in range(n)])
    assert torch.equal(F.patch_search(dev(ia), dev(ib), dev(coarse)), F.patch_search(dev(ia), dev(ib), dev(up)))
    with pytest.raises(ValueError, match="init must be"):
        F.patch_search(dev(ia), dev(ib), torch.zeros(n, 2, 10, 19, device=DEV))
    few = F.patch_search(dev(ia), dev(ib), iters=0).cpu().numpy()
    assert not few[..., :2].any()                                     # no steps: the initial flow


@pytest.mark.parametrize("h,w", NP.STAGE_SIZES)
@pytest.mark.parametrize("n", [1, 3])
def test_densify_vs_numpy(h, w, n):
    ia, ib, init = NP.level_pair(h, w, n, True, True)
    rec = np.stack([NP.patch_search(ia[i], ib[i], init[i]) for i in range(n)]).astype(np.float32)
    got = F.densify(dev(ia), dev(ib), dev(rec)).cpu().numpy()
    assert got.shape == (n, 2, h, w)
    for i in range(n):
        err = np.abs(got[i] - NP.densify(ia[i], ib[i], rec[i])).max()
        print(f"pair {i}: max |gpu - float64| = {err:.3e} (TOL {NP.TOL:.3e})")
        assert err <= NP.TOL
    # a coarser level written at the size of level 0: 2 * f[y // 2, x // 2], exactly
    big = F.densify(dev(ia), dev(ib), dev(rec), shift=1, out_size=(2 * h - 1, 2 * w)).cpu().numpy()
    yy, xx = np.arange(2 * h - 1)[:, None] // 2, np.arange(2 * w)[None] // 2
    assert np.array_equal(big, 2 * got[:, :, yy, xx])


# ------------------------------------------------------------------------------------------------ the whole flow
@pytest.mark.parametrize("size,motion", NP.FULL_CASES)
def test_dense_flow_vs_float64(size, motion):
    a, b, ref = full_case(size, motion)
    got = F.dense_flow(dev(a)[None], dev(b)[None])
    assert got.shape == (1, 2) + size and got.dtype == torch.float32
    diff = np.abs(got[0].cpu().numpy() - ref).max(0)
    print(f"max {diff.max():.3e}, pixels beyond 1e-3 px: {(diff > 1e-3).mean():.4%}")
    assert (diff > 1e-3).mean() <= 0.01


def test_dense_flow_is_repeatable_and_independent_of_the_batch():
    size = (37, 70)
    cases = [full_case(size, m) for m in NP.MOTIONS if (size, m) in NP.FULL_CASES] + [full_case(size, NP.MOTIONS[0])[1::-1]]
    a, b = dev(np.stack([c[0] for c in cases])), dev(np.stack([c[1] for c in cases]))
    assert a.shape[0] == 3
    first = F.dense_flow(a, b)
    assert torch.equal(F.dense_flow(a, b), first)                    # bit for bit
    for i in range(3):
        assert torch.equal(F.dense_flow(a[i:i + 1], b[i:i + 1])[0], first[i]), i
    # bf16 frames are the same call on their fp32 values; finest = 1 stops one level early
    assert torch.equal(F.dense_flow(a.bfloat16(), b.bfloat16()), F.dense_flow(a.bfloat16().float(), b.bfloat16().float()))
    want = np.stack([NP.dense_flow(c[0], c[1], finest=1) for c in cases])
    diff = np.abs(F.dense_flow(a, b, finest=1).cpu().numpy() - want).max(1)
    assert (diff > 1e-3).mean() <= 0.01
    with pytest.raises(ValueError, match="finest"):
        F.dense_flow(a, b, finest=2)


def test_dense_flow_runs_in_stream_order():
    """On a side stream, right behind the producer of its inputs on that stream, with the producer held back."""
    size = (64, 128)
    a, b, _ = full_case(size, NP.MOTIONS[1])
    want = F.dense_flow(dev(a)[None], dev(b)[None])
    host = [torch.from_numpy(x)[None].pin_memory() for x in (a, b)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, want, dev(a)[None])
        gpu_util.stretch(side, 20.0)
        da, db = (h.to(DEV, non_blocking=True) for h in host)         # the producers: queued behind the delay
        got = F.dense_flow(da, db)
    side.synchronize()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ ClassicFlow
def test_classic_flow_input_forms_and_conf():
    a, b, _ = full_case((33, 65), NP.MOTIONS[0])
    A = dev(np.stack([a, b, a, b]) * 2 - 1)
    B = dev(np.stack([b, a, b, b]) * 2 - 1)
    cf = F.ClassicFlow()
    flow, conf = cf(A, B)
    assert flow.shape == (4, 2, 33, 65) and conf.shape == (4, 1, 33, 65)
    assert torch.equal(flow, F.dense_flow(A, B, value_range=(-1, 1)))
    assert torch.equal(conf, ops.occlusion_splat(flow)[0])
    f5, c5 = cf(A.view(2, 2, 3, 33, 65), B.view(2, 2, 3, 33, 65))
    assert torch.equal(f5, flow.view(2, 2, 2, 33, 65)) and torch.equal(c5, conf.view(2, 2, 1, 33, 65))
    f6, c6 = cf(A.view(1, 2, 2, 3, 33, 65), B.view(1, 2, 2, 3, 33, 65))
    assert torch.equal(f6, flow.view(1, 2, 2, 2, 33, 65)) and torch.equal(c6, conf.view(1, 2, 2, 1, 33, 65))
    g, c = F.ClassicFlow(value_range=(0, 1)).compute_flow_and_conf((A + 1) / 2, (B + 1) / 2)      # the flow_fn of rollout
    assert g.shape == flow.shape and c.shape == conf.shape
    assert float(((g - flow).abs().amax(1) > 1e-3).float().mean()) <= 0.01      # the same frames through another affine map
    assert not torch.equal(flow[2], flow[3]) and float(flow[3].abs().max()) < 1e-3                 # b -> b does not move


@pytest.mark.parametrize("t_in", [1, 2])
@pytest.mark.parametrize("use_fw_of", [False, True])
def test_compute_flow_takes_classic_flow(t_in, use_fw_of):
    B, H, W, t_out = 1, 32, 64, 3
    video = dev(NP.texture(H, W * (t_in + t_out), 3)).view(3, H, t_in + t_out, W).permute(0, 2, 1, 3)[None].contiguous()
    tp = dict(num_input_frames=t_in, num_predicted_frames=t_out, use_fw_of=use_fw_of)
    calls = []

    def stub(A, Bm):                                                  # FlowNet's 4-D result shapes
        calls.append(tuple(A.shape))
        return torch.zeros(A.shape[0], 2, H, W, device=DEV), torch.zeros(A.shape[0], 1, H, W, device=DEV)

    want = train.compute_flow(stub, dict(video=video), tp)
    got = train.compute_flow(F.ClassicFlow(), dict(video=video), tp)
    assert calls == [(2 * (t_in - 1 + t_out), 3, H, W)]              # one batched call, nothing else of the flow net is used
    assert set(got) == set(want) == {"input_of", "input_occ", "target_bw_of", "target_bw_occ"} | \
        ({"target_fw_of", "target_fw_occ"} if use_fw_of else set())
    for k, v in want.items():
        if v is None:
            assert got[k] is None and t_in == 1, k
        else:
            assert got[k].shape == v.shape and got[k].dtype == v.dtype and torch.isfinite(got[k]).all(), k
    assert got["target_bw_of"].shape == (B, 2, t_out, H, W) and got["target_bw_occ"].shape == (B, 1, t_out, H, W)


# ------------------------------------------------------------------------------------------------ frames -> flow -> tracks
def test_tracks_from_frames_alone():
    """A painted clip of two boxes moving 3 px per frame: the flows come from ClassicFlow, and track_instances on them links
    both objects through all seven frames.  The last frame is 15 px from the anchor: without flows one object is lost."""
    t_in, T = 2, 7
    video, inst = NP.moving_boxes_clip()
    flows = train.compute_flow(F.ClassicFlow(), dict(video=dev(video)[None]), dict(num_input_frames=t_in, num_predicted_frames=T - t_in))
    maps = dev(inst)[None, None]
    tr = tracking.track_instances(maps, t_in, flows["target_bw_of"], flows["input_of"])
    assert tr.count.tolist() == [2] and tr.lost == [[]]
    for k, (i, y, x, h, w, (dx, dy)) in enumerate(NP.CLIP_BOXES):
        assert tr.ids[0, k].tolist() == [i] * T
        assert tr.boxes[0, k].tolist() == [[x + dx * t, y + dy * t, x + dx * t + w, y + dy * t + h] for t in range(T)]
    ids, _, lost = tracking_np.np_track(inst, t_in, flows["target_bw_of"][0].cpu().numpy(), flows["input_of"][0].cpu().numpy())
    assert lost == [] and ids[:, 0].tolist() == [11001, 12002]
    bare = tracking.track_instances(maps, t_in)
    assert bare.lost != [[]]                                          # same-pixel overlap does not reach that far
