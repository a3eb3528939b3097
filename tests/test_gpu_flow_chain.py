"""The flow chain on the GPU (run with -m gpu): csrc/flow_chain.hip against the numpy restatement (tests/flow_chain_np.py), bit for
bit in float32 and within the tolerances that tests/test_flow_chain_cpu.py derives against float64; the launcher's refusals;
repeatability, independence of the batch, stream order; train.compute_flow with ClassicFlow(chain=True) end to end."""
import numpy as np
import pytest
import torch

import dense_flow_np as NP
import flow_chain_np as C
import gpu_util
from c2m_amd import _lib, flow as F
from c2m_amd import ops, tracking, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ORDERS = ("backward", "forward")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the stage
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("H,W,K,N,kind", C.stage_cases())
def test_chain_flows_vs_the_restatement(H, W, K, N, kind, order):
    """Against float64 within 16 x the float32 gap of the case itself (at most TOL_CHAIN; 0 for one hop), and against the
    float32 restatement bit for bit: flows and `valid`.  `valid` against float64 outside the pixels flow_chain_np.undecided
    names."""
    steps = C.stage_steps(H, W, K, N, kind)
    flow, valid = F.chain_flows(dev(steps), order, return_valid=True)
    assert flow.shape == (N, K, 2, H, W) and flow.dtype == torch.float32 and valid.shape == (N, K, H, W) and valid.dtype == torch.uint8
    assert torch.equal(F.chain_flows(dev(steps), order).view(torch.int32), flow.view(torch.int32))      # without the map; NaN == NaN
    got, ok = flow.cpu().numpy(), valid.cpu().numpy()
    assert set(np.unique(ok)) <= {0, 1}
    gap = C.case_gap(steps, order)
    assert 16 * gap <= C.TOL_CHAIN
    for i in range(N):
        o64, v64 = C.chain(steps[i], order)
        o32, v32 = C.chain(steps[i], order, np.float32)
        assert np.array_equal(np.isnan(got[i]), np.isnan(o64)) and np.isnan(o64).any() == (kind == "nan")
        err = float(np.nanmax(np.abs(got[i] - o64)))
        same = np.array_equal(got[i], o32, equal_nan=True)
        und = C.undecided(steps[i], order, rounding=C.chaotic(K, kind))
        print(f"clip {i}: max |gpu - float64| = {err:.3e} (16 x gap {16 * gap:.3e}), float32 bits {'equal' if same else 'DIFFER'}, "
              f"valid differs from float64 at {int((ok[i].astype(bool) != v64).sum())} pixels, {int(und.sum())} undecided")
        assert err <= 16 * gap
        assert same and np.array_equal(ok[i].astype(bool), v32)
        assert not ((ok[i].astype(bool) != v64) & ~und).any()
    if K == 1:                                                        # a one-hop chain is the step
        assert np.array_equal(got.view(np.uint32), steps.view(np.uint32))
    assert np.array_equal(got[:, 0][~np.isnan(got[:, 0])], steps[:, 0][~np.isnan(got[:, 0])])


def test_launcher_refuses_bad_sizes_and_short_buffers():
    fc = _lib.lib().c2m_flow_chain
    N, K, H, W = 2, 3, 9, 13
    steps, out, valid = torch.zeros(N, K, 2, H, W, device=DEV), torch.full((N, K, 2, H, W), 7.0, device=DEV), torch.full((N, K, H, W), 7, device=DEV, dtype=torch.uint8)
    total = steps.numel()

    def call(K=K, se=total, oe=total, ve=total // 2, out=out, forward=0):
        return fc(ops._p(steps), se, ops._p(out), oe, ops._p(valid), ve, N, K, H, W, forward, ops._stream())

    for bad in (dict(K=0), dict(K=17), dict(se=total - 1), dict(oe=total - 1), dict(ve=total // 2 - 1), dict(out=steps), dict(forward=2)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and int(valid.min()) == 7          # nothing was launched
    assert call() == 0 and call(forward=1) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and int(valid.min()) == 1   # zero steps: nothing moves, everything stays inside
    with pytest.raises(ValueError, match="chain_flows needs"):
        F.chain_flows(torch.zeros(1, 17, 2, 8, 8, device=DEV))


# ------------------------------------------------------------------------------------------------ call properties
@pytest.mark.parametrize("order", ORDERS)
def test_chain_flows_is_repeatable_and_independent_of_the_batch(order):
    H, W, K, N = 21, 37, 5, 3
    steps = dev(C.stage_steps(H, W, K, N, "leave"))
    first, valid = F.chain_flows(steps, order, return_valid=True)
    again, valid2 = F.chain_flows(steps, order, return_valid=True)
    assert torch.equal(again, first) and torch.equal(valid2, valid)  # bit for bit
    for i in range(N):
        one, v = F.chain_flows(steps[i:i + 1], order, return_valid=True)
        assert torch.equal(one[0], first[i]) and torch.equal(v[0], valid[i]), i
    # a view that is not contiguous is the same call on its values
    wide = torch.cat([steps, steps.flip(1)], 1)
    assert torch.equal(F.chain_flows(wide[:, :K], order), first)
    assert not torch.equal(F.chain_flows(steps, ORDERS[order == "backward"]), first)


@pytest.mark.parametrize("order", ORDERS)
def test_chain_flows_runs_in_stream_order(order):
    """On a side stream, right behind the producer of its input on that stream, with the producer held back."""
    H, W, K, N = C.STAGE_SHAPES[-1]
    steps = C.stage_steps(H, W, K, N, "smooth")
    want, want_valid = F.chain_flows(dev(steps), order, return_valid=True)
    host = torch.from_numpy(steps).pin_memory()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, want, want)                             # the input's and the result's blocks
        gpu_util.stretch(side, 20.0)
        got, got_valid = F.chain_flows(host.to(DEV, non_blocking=True), order, return_valid=True)      # queued behind the delay
    side.synchronize()
    assert torch.equal(got, want) and torch.equal(got_valid, want_valid)


# ------------------------------------------------------------------------------------------------ end to end
def test_compute_flow_with_chained_targets():
    """moving_boxes_clip(), t_in = 2, five predicted frames.  The search decisions are dense_flow's, so the chained flows are
    within dense_flow_np.TOL + TOL_CLIP (TOL_CHAIN's counterpart on this clip's own steps, and far below it) of the float64
    restatement on at least 99 % of the pixels; on the interior of object 11001, 12 and 15 px from the last input frame, they
    are as good as the restatement's, where the direct search is lost."""
    video, inst, ref = C.boxes_reference()
    t_in, t_out = C.CLIP_T_IN, video.shape[1] - C.CLIP_T_IN
    batch, tp = dict(video=dev(video)[None]), dict(num_input_frames=t_in, num_predicted_frames=t_out, use_fw_of=True)
    chained = train.compute_flow(F.ClassicFlow(chain=True), batch, tp)
    direct = train.compute_flow(F.ClassicFlow(), batch, tp)
    assert chained.keys() == direct.keys()
    for k, v in direct.items():
        assert chained[k].shape == v.shape and chained[k].dtype == v.dtype and chained[k].is_contiguous() and torch.isfinite(chained[k]).all(), k
    tol = NP.TOL + C.TOL_CLIP
    assert tol <= NP.TOL + C.TOL_CHAIN
    for k in ("input_of", "target_bw_of", "target_fw_of"):
        diff = np.abs(chained[k][0].cpu().numpy() - ref[k]).max(0)    # [frames, H, W]
        print(f"{k}: max {diff.max():.3e}, beyond {tol:.2e} px: {(diff > tol).mean():.4%}; per frame",
              [f"{(d > tol).mean():.4%}" for d in diff])
        assert (diff > tol).mean() <= 0.01
    # what the chain is for: the far targets on the object
    dx, dy = C.CLIP_SPEED
    for g in (4, 5):
        for key, mask, true in (("target_bw_of", inst[t_in - 1 + g] == C.CLIP_OBJECT, (-g * dx, -g * dy)),
                                ("target_fw_of", inst[t_in - 1] == C.CLIP_OBJECT, (g * dx, g * dy))):
            mask, true = NP.interior(mask), C.constant_flow(64, 128, true)
            e_gpu, e_ref = NP.epe(chained[key][0, :, g - 1].cpu().numpy(), true, mask), NP.epe(ref[key][:, g - 1], true, mask)
            e_direct = NP.epe(direct[key][0, :, g - 1].cpu().numpy(), true, mask)
            print(f"{key} gap {g}: chained {e_gpu:.4f} (float64 restatement {e_ref:.4f}), direct {e_direct:.4f}")
            assert e_gpu <= e_ref + tol and e_direct > 5
    # nothing else moves: the input frames and the first target frame are the direct call's, bit for bit
    assert torch.equal(chained["input_of"], direct["input_of"]) and torch.equal(chained["input_occ"], direct["input_occ"])
    for k in ("target_bw_of", "target_bw_occ", "target_fw_of", "target_fw_occ"):
        assert torch.equal(chained[k][:, :, 0], direct[k][:, :, 0]), k
        assert not torch.equal(chained[k][:, :, -1], direct[k][:, :, -1]), k
    assert torch.equal(chained["target_bw_occ"], ops.occlusion_splat(chained["target_fw_of"])[0])
    assert torch.equal(chained["target_fw_occ"], ops.occlusion_splat(chained["target_bw_of"])[0])
    # the tracks of the painted clip are found on the chained flows
    tr = tracking.track_instances(dev(inst)[None, None], t_in, chained["target_bw_of"], chained["input_of"])
    assert tr.count.tolist() == [2] and tr.lost == [[]]


def test_clip_flows_batch_keys_and_a_single_input_frame():
    video, _, _ = C.boxes_reference()
    clips = dev(np.stack([video, video[:, ::-1], video[:, :, ::-1]]))                # the clip, reversed in time, upside down
    both = F.clip_flows(clips, 2, 5, use_fw_of=True)
    assert torch.equal(F.clip_flows(clips, 2, 5, use_fw_of=True)["target_bw_of"], both["target_bw_of"])
    for i in range(3):
        one = F.clip_flows(clips[i:i + 1], 2, 5, use_fw_of=True)
        for k, v in one.items():
            assert torch.equal(v[0], both[k][i]), (i, k)
    assert torch.equal(both["target_bw_of"][1], both["target_bw_of"][0]) is False
    # a ClassicFlow(chain=True) call on frames in [0, 1] mapped to [-1, 1] is clip_flows on them with that range
    cf = F.ClassicFlow(chain=True, iters=8)
    got = cf.clip_flows(dict(video=clips), dict(num_input_frames=2, num_predicted_frames=5))
    want = F.clip_flows(clips * 2 - 1, 2, 5, value_range=(-1, 1), iters=8)
    assert sorted(got) == ["input_occ", "input_of", "target_bw_occ", "target_bw_of"]
    assert all(torch.equal(got[k], want[k]) for k in got)
    assert not torch.equal(got["target_bw_of"], F.ClassicFlow(chain=True).clip_flows(dict(video=clips), dict(num_input_frames=2, num_predicted_frames=5))["target_bw_of"])
    # t_in = 1: no input flows; more frames than t_in + t_out are not looked at
    single = F.clip_flows(clips, 1, 3)
    assert single["input_of"] is None and single["input_occ"] is None and single["target_bw_of"].shape == (3, 2, 3, 64, 128)
    assert torch.equal(single["target_bw_of"], F.clip_flows(clips[:, :, :4], 1, 3)["target_bw_of"])
    # frame 1 -> frame 0 is the first target of t_in = 1 and the reverse of the input pair of t_in = 2: one consecutive flow
    assert torch.equal(single["target_bw_of"][:, :, 0], F.clip_flows(clips, 1, 1)["target_bw_of"][:, :, 0])
    assert torch.equal(ops.occlusion_splat(single["target_bw_of"][:, :, :1].contiguous())[0], both["input_occ"])
