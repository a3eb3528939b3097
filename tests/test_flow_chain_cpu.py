"""Host side of the flow chain (no GPU): the C ABI and the launcher's refusals, the argument checks of c2m_amd.flow and the
delegation of train.compute_flow, the properties of the restatement (tests/flow_chain_np.py): exact sums, a one-hop chain is the
step, no read out of bounds whatever the steps hold, forward against backward; the error table of DESIGN.md 4.2n (direct search
against chained consecutive flows); and the float32-against-float64 gaps from which the GPU tests' tolerances are derived."""
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as NP
import flow_chain_np as C
from c2m_amd import _lib, build, flow as F, train

ORDERS = ("backward", "forward")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_point_is_declared_bound_and_exported():
    assert "c2m_flow_chain" in _lib.declared_symbols() and "c2m_flow_chain" in _lib._SIGS
    assert hasattr(_lib.lib(), "c2m_flow_chain")
    assert _lib.ABI_VERSION == 6 and _lib.lib().c2m_abi_version() == 6                 # purely additive
    assert build.SOURCES["flow_chain.hip"] == build.SOURCES["dense_flow.hip"]         # -ffp-contract=off, no SLP vectoriser
    assert F.CHAIN_CAP == C.K_CAP == 16


def test_launcher_checks():
    """Host-side checks run without a device: nothing to do is success; bad sizes and short extents are refused before a launch."""
    fc = _lib.lib().c2m_flow_chain
    ptr = torch.zeros(1).data_ptr()                                   # never read: every call below ends before the launch

    def call(N=0, K=1, H=8, W=8, forward=0, steps=None, out=None, valid=None, se=0, oe=0, ve=0):
        return fc(steps, se, out, oe, valid, ve, N, K, H, W, forward, None)

    assert call() == 0 and call(K=C.K_CAP, forward=1) == 0 and call(H=1, W=1) == 0
    for bad in (dict(K=0), dict(K=C.K_CAP + 1), dict(K=-1), dict(H=0), dict(W=0), dict(N=-1), dict(forward=2), dict(forward=-1),
                dict(N=1 << 20, K=16, H=8, W=8),                      # N K 2 H W = 2^31
                dict(N=1, K=1, H=1 << 16, W=1 << 15), dict(H=1 << 30, W=1 << 30)):
        assert call(**bad) != 0, bad
    assert call(N=(1 << 20) - 1, K=16, H=8, W=8, steps=ptr, out=ptr + 4) != 0          # in range, but no extents
    total = 2 * 3 * 5 * 7
    ok = dict(N=2, K=3, H=5, W=7, steps=ptr, out=ptr + 4, valid=ptr + 8, se=total, oe=total, ve=total // 2)
    for bad in (dict(steps=None), dict(out=None), dict(se=total - 1), dict(oe=total - 1), dict(ve=total // 2 - 1), dict(out=ptr),
                dict(steps=ptr + 1)):
        assert call(**dict(ok, **bad)) != 0, bad


# ------------------------------------------------------------------------------------------------ the interface
def test_argument_errors_are_raised_before_the_device_is_touched():
    s = torch.zeros(2, 3, 2, 8, 12)
    with pytest.raises(ValueError, match="order"):
        F.chain_flows(s, order="both")
    for bad in (s[0], s[:, :, :1], s.double(), s.numpy(), torch.zeros(2, 0, 2, 8, 12), torch.zeros(1, F.CHAIN_CAP + 1, 2, 8, 12)):
        with pytest.raises(ValueError, match="steps must be|chain_flows needs"):
            F.chain_flows(bad)
    for order in ORDERS:
        with pytest.raises(RuntimeError, match="HIP"):                # no CPU path
            F.chain_flows(s, order=order, return_valid=True)
    video = torch.zeros(1, 3, 7, 16, 24)
    with pytest.raises(ValueError, match="HIP device"):
        F.clip_flows(video, 2, 5)
    for bad in (dict(num_input_frames=0, num_predicted_frames=5), dict(num_input_frames=2, num_predicted_frames=0),
                dict(num_input_frames=1, num_predicted_frames=F.CHAIN_CAP + 1)):
        with pytest.raises(ValueError, match="clip_flows needs"):
            F.clip_flows(video, **bad)
    for bad in (video[0], video[:, :2], video[:, :, :6]):
        with pytest.raises(ValueError, match="video must be"):
            F.clip_flows(bad, 2, 5)
    with pytest.raises(ValueError, match="sor"):
        F.clip_flows(video, 2, 5, refine=dict(sor=0))
    assert F.ClassicFlow().chain is False and F.ClassicFlow(chain=True).chain is True
    with pytest.raises(ValueError, match="HIP device"):
        F.ClassicFlow(chain=True).clip_flows(dict(video=video), dict(num_input_frames=2, num_predicted_frames=5))


def test_compute_flow_delegates_only_to_a_chaining_flow_module():
    video = torch.rand(1, 3, 3, 8, 8)
    tp = dict(num_input_frames=1, num_predicted_frames=2)

    class Stub:
        def __init__(self, chain=None):
            self.calls = []
            if chain is not None:
                self.chain = chain

        def clip_flows(self, batch, params):
            self.calls.append("clip")
            return {"target_bw_of": "chained"}

        def __call__(self, A, B):
            self.calls.append("pairs")
            return torch.zeros(A.shape[0], 2, 8, 8), torch.ones(A.shape[0], 1, 8, 8)

    on = Stub(chain=True)
    assert train.compute_flow(on, dict(video=video), tp) == {"target_bw_of": "chained"} and on.calls == ["clip"]
    for off in (Stub(chain=False), Stub()):                           # FlowNet has no such attribute
        got = train.compute_flow(off, dict(video=video), tp)
        assert off.calls == ["pairs"] and got["target_bw_of"].shape == (1, 2, 2, 8, 8) and got["input_of"] is None


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", ORDERS)
def test_chains_of_constant_steps_are_the_sum_exactly(order, dtype):
    """Constants with few bits: every product of the bilinear weights is exact, and so is every sum."""
    H, W, consts = 11, 17, [(1.5, -0.25), (-2.25, 1.0), (0.5, 0.75), (3.0, -1.5)]
    steps = np.stack([C.constant_flow(H, W, c) for c in consts])
    out, valid = C.chain(steps, order, dtype)
    assert out.dtype == dtype
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(len(consts)):
        walk = consts[:k + 1][::-1] if order == "backward" else consts[:k + 1]
        total, inside = np.zeros(2), np.ones((H, W), bool)
        for c in walk:
            total += c
            inside &= (xx + total[0] >= 0) & (xx + total[0] <= W - 1) & (yy + total[1] >= 0) & (yy + total[1] <= H - 1)
        assert np.array_equal(out[k], C.constant_flow(H, W, total)), k
        assert np.array_equal(valid[k], inside) and 0 < inside.sum() < inside.size, k


@pytest.mark.parametrize("order", ORDERS)
def test_a_one_hop_chain_returns_the_bits_of_the_step(order):
    steps = C.stage_steps(21, 37, 5, 1, "leave")[0]
    out, _ = C.chain(steps, order, np.float32)
    assert out.dtype == np.float32 and np.array_equal(out[0].view(np.uint32), steps[0].view(np.uint32))
    one, valid = C.chain(steps[3:4], order, np.float32)
    assert np.array_equal(one[0].view(np.uint32), steps[3].view(np.uint32))
    yy, xx = np.mgrid[0:21, 0:37]
    ex, ey = xx + steps[3, 0], yy + steps[3, 1]                       # float32 + int64 -> float64: exact
    assert np.array_equal(valid[0], (ex.astype(np.float32) >= 0) & (ex.astype(np.float32) <= 36) & (ey.astype(np.float32) >= 0)
                          & (ey.astype(np.float32) <= 20))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", ORDERS)
def test_wild_steps_read_nothing_out_of_bounds(order, dtype):
    """NaN, +-1e6 and infinite entries: every index of every hop's gather lies inside the plane, the indices are those
    dense_flow_np.sample reads with, and `valid` is 0 wherever the displacement is not finite or has left the frame."""
    H, W, K = 13, 19, 4
    steps = C.stage_steps(H, W, K, 1, "plain")[0].copy()
    steps[1, 0, 4, 5], steps[1, 1, 6, 7], steps[2, 0, 2, 3], steps[0, 1, 9, 11] = np.nan, 1e6, -1e6, np.nan
    steps[2, 1, 10, 15], steps[3, 0, 1, 1] = np.inf, -np.inf
    with np.errstate(invalid="ignore"):                               # 0 * inf and inf - inf: NaN, as on the device
        out, valid, hops = C.chain(steps, order, dtype, details=True)
    assert np.isnan(out).any() and (np.abs(out[np.isfinite(out)]) > 1e5).any()
    hop_count = 0
    for k in range(K):
        assert len(hops[k]) == k + 1
        for h, ((px, py), _) in enumerate(hops[k]):
            x0, x1, y0, y1 = C.gather_indices(px, py, H, W)
            assert x0.min() >= 0 and x1.max() <= W - 1 and y0.min() >= 0 and y1.max() <= H - 1 and (x0 <= x1).all() and (y0 <= y1).all()
            hop_count += 1
            # the same indices give dense_flow_np.sample's value (on a finite plane)
            plane = np.arange(H * W, dtype=dtype).reshape(H, W)
            fx = np.clip(np.where(np.isnan(px), 0, px), 0, W - 1).astype(dtype)
            fy = np.clip(np.where(np.isnan(py), 0, py), 0, H - 1).astype(dtype)
            ax, ay = fx - np.floor(fx), fy - np.floor(fy)
            top, bot = plane[y0, x0] * (1 - ax) + plane[y0, x1] * ax, plane[y1, x0] * (1 - ax) + plane[y1, x1] * ax
            assert np.array_equal(top * (1 - ay) + bot * ay, NP.sample(plane, np.where(np.isnan(px), 0, px).astype(dtype),
                                                                       np.where(np.isnan(py), 0, py).astype(dtype)))
    assert hop_count == K * (K + 1) // 2
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore"):
        ex, ey = xx + out[:, 0], yy + out[:, 1]
        assert not (valid & ~((ex >= 0) & (ex <= W - 1) & (ey >= 0) & (ey <= H - 1))).any()
    assert not valid[np.isnan(out).any(1)].any()


@functools.lru_cache(maxsize=None)
def shift_case(H, W, per_frame):
    """(video, backward steps, forward steps, backward chain, forward chain) of a pure-shift clip of six frames, float64."""
    video = C.shift_clip(H, W, per_frame)
    bw, fw = C.clip_steps(video, 0, 5)
    return video, bw, fw, C.chain(bw, "backward")[0], C.chain(fw, "forward")[0]


def test_forward_and_backward_chains_agree_on_a_pure_shift():
    """On a global shift the forward chain is minus the backward one.  tests/test_dense_flow_cpu.py allows the restatement a mean
    endpoint error of E = 0.25 px on a pair with a known motion; a chain of g hops adds up g such errors, so each chain is within
    g E of the truth and the two agree within 2 g E, in the mean over dense_flow_np.pair's mask of both flows.  (A chain with the
    wrong sign, or one hop short, is 3.8 px or more off.)  Measured at 64 x 128, (3.5, -1.5) px per frame, g = 1 .. 5: single
    consecutive flows 0.016 .. 0.021; backward 0.016 / 0.034 / 0.051 / 0.077 / 0.097, forward 0.018 / 0.050 / 0.096 / 0.093 /
    0.108, |forward + backward| 0.026 / 0.068 / 0.124 / 0.141 / 0.169."""
    H, W, s, E = 64, 128, (3.5, -1.5), 0.25
    _, bw, fw, cb, cf = shift_case(H, W, s)
    for g in range(1, 6):
        tb, tf = (g * s[0], g * s[1]), (-g * s[0], -g * s[1])
        m = C.shift_mask(H, W, tb) & C.shift_mask(H, W, tf)
        eb, ef = NP.epe(cb[g - 1], C.constant_flow(H, W, tb), m), NP.epe(cf[g - 1], C.constant_flow(H, W, tf), m)
        agree = NP.epe(cf[g - 1], -cb[g - 1], m)
        print(f"gap {g}: backward {eb:.4f} forward {ef:.4f} |forward + backward| {agree:.4f} (bounds {g * E:.2f}, {2 * g * E:.2f})")
        assert m.mean() > 0.3 and eb <= g * E and ef <= g * E and agree <= 2 * g * E


# ------------------------------------------------------------------------------------------------ the error table
def table_row(direct, chained, true, mask):
    return NP.epe(direct, true, mask), NP.epe(chained, true, mask)


@pytest.mark.parametrize("size,per_frame", [((64, 128), (3.5, -1.5)), ((128, 256), (5.0, -2.0))])
def test_chained_flow_on_a_global_shift(size, per_frame):
    """Mean endpoint error (px) of the backward flow c_g -> c_0 = g * per_frame over dense_flow_np.pair's mask, direct search
    against the chain of the consecutive flows, float64.  Measured, gap 3 / 4 / 5, direct then chained:
    (3.5, -1.5) px per frame at 64 x 128: 2.95 / 8.99 / 9.36 and 0.051 / 0.075 / 0.096;
    (5, -2) px per frame at 128 x 256: 0.333 / 0.099 / 11.8 and 0.025 / 0.040 / 0.041 (the direct search at gap 4 finds the
    20 px there; at gap 5 it does not)."""
    H, W = size
    video, _, _, cb, _ = shift_case(H, W, per_frame)
    for g in (3, 4, 5):
        true = (g * per_frame[0], g * per_frame[1])
        direct, chained = table_row(NP.dense_flow(video[:, g], video[:, 0]), cb[g - 1], C.constant_flow(H, W, true), C.shift_mask(H, W, true))
        print(f"{size} {per_frame} gap {g}: direct {direct:.4f} chained {chained:.4f} ratio {chained / direct:.4f}")
        if size == (64, 128) and g >= 4:
            assert direct > 5 and chained < direct / 20


@pytest.mark.parametrize("order", ORDERS)
def test_chained_flow_on_the_moving_boxes(order):
    """Object 11001 of moving_boxes_clip() (3 px per frame), t_in = 2, its interior (4 px from its edge), float64.  Measured, gap
    3 / 4 / 5, direct then chained: backward (target frame -> last input frame) 0.354 / 13.2 / 12.8 and 0.028 / 0.042 / 0.042;
    forward 1.92 / 15.2 / 15.8 and 0.022 / 0.027 / 0.035."""
    video, inst, ref = C.boxes_reference()
    first, (dx, dy) = C.CLIP_T_IN - 1, C.CLIP_SPEED
    for g in (3, 4, 5):
        if order == "backward":
            mask, true = NP.interior(inst[first + g] == C.CLIP_OBJECT), (-g * dx, -g * dy)
            direct, chained = NP.dense_flow(video[:, first + g], video[:, first]), ref["target_bw_of"][:, g - 1]
        else:
            mask, true = NP.interior(inst[first] == C.CLIP_OBJECT), (g * dx, g * dy)
            direct, chained = NP.dense_flow(video[:, first], video[:, first + g]), ref["target_fw_of"][:, g - 1]
        d, c = table_row(direct, chained, C.constant_flow(64, 128, true), mask)
        print(f"{order} gap {g}: direct {d:.4f} chained {c:.4f} ratio {c / d:.4f}")
        assert mask.sum() == 16 * 24
        if g >= 4:
            assert d > 5 and c < d / 20
    # the first target frame and the input frames are the consecutive flows themselves
    assert np.array_equal(ref["target_bw_of"][:, 0], ref["steps_bw"][0]) and np.array_equal(ref["target_fw_of"][:, 0], ref["steps_fw"][0])


# ------------------------------------------------------------------------------------------------ the GPU tests' tolerances
def test_tolerance_is_sixteen_times_the_float32_gap_of_the_restatement():
    """TOL_CHAIN as flow_chain_np defines it, over the uniform stage inputs; the chain through such fields is chaotic at K = 16 (see
    flow_chain_np), which this test shows per case; the smooth cases are not."""
    gap, smooth = 0.0, 0.0
    for H, W, K, N, kind in C.stage_cases():
        steps = C.stage_steps(H, W, K, N, kind)
        for order in ORDERS:
            g = C.case_gap(steps, order)
            print(f"{H} x {W}, K = {K}, N = {N}, {kind}, {order}: float32 - float64 gap {g:.3e}")
            if kind == "smooth":
                smooth = max(smooth, g)
            elif kind != "nan":
                gap = max(gap, g)
            if K == 1:
                assert g == 0                                         # one hop is exact
    print("gap", gap, "TOL_CHAIN", C.TOL_CHAIN, "smooth", smooth)
    assert C.TOL_CHAIN == 16 * C.MEASURED_GAP and 0.5 * C.MEASURED_GAP <= gap <= 2 * C.MEASURED_GAP
    assert 0 < smooth <= 1e-4                                         # a long chain through a smooth field is well conditioned


def test_clip_tolerance_is_sixteen_times_the_gap_on_the_clip_s_own_steps():
    _, _, ref = C.boxes_reference()
    gap = max(C.case_gap(ref[name].astype(np.float32)[None], order) for name, order in (("steps_bw", "backward"), ("steps_fw", "forward")))
    print("float32 - float64 gap of the chain on the clip's steps", gap, "TOL_CLIP", C.TOL_CLIP)
    assert C.TOL_CLIP == 16 * C.MEASURED_GAP_CLIP and 0.5 * C.MEASURED_GAP_CLIP <= gap <= 2 * C.MEASURED_GAP_CLIP
    assert C.TOL_CLIP <= C.TOL_CHAIN


@pytest.mark.parametrize("H,W,K,N,kind", C.stage_cases())
def test_valid_of_the_stage_seeds(H, W, K, N, kind):
    """The pixels within EDGE_EPS of the frame edge are at most 1 % of every case, and outside them the float32 restatement's
    `valid` is the float64 one's -- except for the uniform steps at K = 16, where rounding moves a walk by pixels (36 to 55
    pixels of a clip's 44 800 differ outside the band): there the two agree outside undecided(rounding=True), 6.2 % of the case."""
    steps = C.stage_steps(H, W, K, N, kind)
    chaotic = C.chaotic(K, kind)
    for order in ORDERS:
        band = np.stack([C.undecided(s, order) for s in steps])
        v64 = np.stack([C.chain(s, order)[1] for s in steps])
        v32 = np.stack([C.chain(s, order, np.float32)[1] for s in steps])
        und = np.stack([C.undecided(s, order, rounding=True) for s in steps]) if chaotic else band
        print(f"{order}: band {band.mean():.4%}, left out {und.mean():.4%}, valid {v64.mean():.3f}, differ outside the band {int(((v64 != v32) & ~band).sum())}")
        assert band.mean() <= 0.01 and und.mean() <= 0.1
        assert not ((v64 != v32) & ~und).any()
        assert 0.2 < v64.mean() < 0.9                                 # walks leave the frame, and walks stay
        if kind == "leave":
            assert v64.mean() < 0.5
