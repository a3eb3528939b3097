"""Host side of the variational refinement of the dense flow (no GPU): the C ABI and the launchers' refusals, the argument checks
of c2m_amd.flow, what the float64 restatement (tests/flow_refine_np.py) gains over the plain flow on scenes with a known flow,
that an iteration restricted to a tile plus its halo equals the global iteration bit for bit (what fr_iterate_kernel rests on),
and the float32-against-float64 gap of the restatement, from which the GPU tests' tolerance is derived."""
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as NP
import flow_refine_np as R
from c2m_amd import _lib, build, flow as F

BIG_CASES = [((128, 256), ("zoom", 0.05)), ((128, 256), ("shift", (13.5, 6.25)))]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_exported():
    for name in ("c2m_flow_refine_workspace_bytes", "c2m_flow_refine_prepare", "c2m_flow_refine_iterate"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
        assert hasattr(_lib.lib(), name)
    assert build.SOURCES["flow_refine.hip"] == build.SOURCES["dense_flow.hip"]        # -ffp-contract=off, no SLP vectoriser
    assert F.REFINE_DEFAULTS == R.DEFAULTS and F.SOR_CAP == R.SOR_CAP


def test_workspace_query_and_launcher_checks():
    L = _lib.lib()
    wb = L.c2m_flow_refine_workspace_bytes
    assert wb(3, 33, 65) == 4 * 12 * 3 * 33 * 65 and wb(0, 8, 8) == 0 and wb(1, 8, 8) == 4 * 12 * 64
    for bad in ((1, 7, 8), (1, 8, 7), (-1, 8, 8), (1, 32769, 8), (1 << 24, 8, 8)):
        assert wb(*bad) == -1, bad
    # the dense flow's own workspace is what it was
    assert L.c2m_flow_workspace_bytes(3, 33, 65, 2) == 4 * (2 * 3 * (33 * 65 + 17 * 33) + 3 * 8 * 16 * 3 + 2 * 3 * 17 * 33)
    # host-side checks run without a device: nothing to do is success, bad sizes, extents and parameters are refused
    prep, it = L.c2m_flow_refine_prepare, L.c2m_flow_refine_iterate
    assert prep(None, None, 0, None, 0, None, 0, 0, 8, 8, None) == 0
    assert prep(None, None, 0, None, 0, None, 0, 1, 8, 8, None) != 0                    # no tensors
    assert prep(None, None, 0, None, 0, None, 0, 0, 7, 8, None) != 0

    def iterate(N=0, h=8, w=8, iteration=0, sor=5, alpha=20.0, delta=5.0, gamma=10.0, omega=1.6, shift=0, Ho=8, Wo=8, out=None):
        return it(None, 0, None, 0, N, h, w, iteration, sor, alpha, delta, gamma, omega, out, 0, shift, Ho, Wo, None)

    assert iterate() == 0
    assert iterate(N=1) != 0                                                            # no tensors
    for bad in (dict(h=7), dict(w=7), dict(sor=0), dict(sor=6), dict(iteration=-1), dict(iteration=1024), dict(alpha=0.0),
                dict(delta=-1.0), dict(gamma=float("nan")), dict(alpha=float("inf")), dict(omega=0.0), dict(omega=2.0),
                dict(omega=float("nan"))):
        assert iterate(**bad) != 0, bad
    # an output is checked like c2m_flow_densify's: no output row or column past the level
    out = (torch.zeros(1).data_ptr())
    assert iterate(out=out) == 0 and iterate(out=out, shift=1, Ho=16, Wo=16) == 0
    assert iterate(out=out, Ho=9) != 0 and iterate(out=out, shift=1, Ho=17, Wo=16) != 0 and iterate(out=out, shift=7) != 0
    assert iterate(out=out, Ho=0) != 0


# ------------------------------------------------------------------------------------------------ the interface
def test_argument_errors_are_raised_before_the_device_is_touched():
    a = torch.zeros(2, 3, 16, 24)
    ia, fl = torch.zeros(2, 16, 24), torch.zeros(2, 2, 16, 24)
    for bad, match in ((dict(sor=0), "sor"), (dict(sor=F.SOR_CAP + 1), "sor"), (dict(outer=0), "outer"), (dict(omega=0), "omega"),
                       (dict(omega=2.0), "omega"), (dict(alpha=0), "alpha"), (dict(delta=-1), "delta"),
                       (dict(gamma=float("nan")), "gamma")):
        with pytest.raises(ValueError, match=match):
            F.refine_flow(ia, ia, fl, **bad)
        with pytest.raises(ValueError, match=match):
            F.dense_flow(a, a, refine=bad)
        with pytest.raises(ValueError, match=match):
            F.ClassicFlow(refine=bad)
    with pytest.raises(ValueError, match="unknown parameters"):
        F.dense_flow(a, a, refine=dict(sigma=1))
    with pytest.raises(ValueError, match="refine must be"):
        F.dense_flow(a, a, refine="yes")
    for refine in (True, dict(sor=2), None, False):
        with pytest.raises(ValueError, match="HIP device"):
            F.dense_flow(a, a, refine=refine)
        with pytest.raises(ValueError, match="HIP device"):
            F.ClassicFlow(refine=refine)(a, a)
    with pytest.raises(ValueError, match="h, w >= 8"):
        F.refine_flow(ia[:, :7], ia[:, :7], fl[:, :, :7])
    with pytest.raises(ValueError, match="level images"):
        F.refine_flow(ia.double(), ia.double(), fl)
    with pytest.raises(ValueError, match="level images"):
        F.refine_flow(ia, ia[:1], fl)
    with pytest.raises(RuntimeError, match="HIP"):
        F.refine_flow(ia, ia, fl)
    assert F.refine_params(None) is None and F.refine_params(False) is None and F.refine_params(True) == F.REFINE_DEFAULTS
    assert F.refine_params(dict(sor=2, omega=1)) == dict(F.REFINE_DEFAULTS, sor=2, omega=1.0)
    assert F.ClassicFlow().refine is None and F.ClassicFlow(refine=True).refine is True


# ------------------------------------------------------------------------------------------------ what the refinement gains
@functools.lru_cache(maxsize=None)
def errors(size, motion):
    a, b, true, mask = NP.pair(motion, *size)
    return NP.epe(NP.dense_flow(a, b), true, mask), NP.epe(R.dense_flow(a, b), true, mask)


@pytest.mark.parametrize("size,motion", NP.FULL_CASES + BIG_CASES)
def test_refinement_gains_on_smooth_motion_and_loses_nowhere(size, motion):
    """float64, mean endpoint error over dense_flow_np.pair's mask.  Measured, plain / refined: 4 % zoom 0.0630 / 0.0272 (64 x 128),
    0.0647 / 0.0257 (33 x 65), 0.0636 / 0.0275 (37 x 70); 5 % zoom at 128 x 256 0.0774 / 0.0308; shift (1.7, -0.9) 0.0222 / 0.0197,
    0.0192 / 0.0185, 0.0199 / 0.0156; (7.5, 3.25) at 64 x 128 0.0212 / 0.0274, the one case that loses; (13.5, 6.25) at 128 x 256
    0.0211 / 0.0172."""
    plain, refined = errors(size, motion)
    print(size, motion, f"plain {plain:.4f} refined {refined:.4f} ratio {refined / plain:.3f}")
    if motion[0] == "zoom":
        assert refined <= 0.6 * plain
    assert refined <= plain + 0.01


@pytest.mark.parametrize("size,obj,motion,whole,band,core", [((128, 256), (50, 70), (6, -3), 0.75, 0.8, 0.5),
                                                              ((64, 128), (24, 36), (3, -2), 1.0, None, 0.5)])
def test_refinement_on_a_moving_object(size, obj, motion, whole, band, core):
    """The whole object, its 4-px edge band and the object eroded by 4.  Measured, plain / refined: 128 x 256, 50 x 70 moving
    (6, -3): 0.3785 / 0.2266, 1.3329 / 0.8731, 0.0501 / 0.0042; 64 x 128, 24 x 36 moving (3, -2): 0.1847 / 0.1761,
    0.3734 / 0.3633 (the band of the small object is NOT repaired), 0.0095 / 0.0023."""
    a, b, true, inside = NP.two_layer(*size, obj=obj, motion=motion)
    plain, refined = NP.dense_flow(a, b), R.dense_flow(a, b)
    for name, mask, cap in zip(("whole", "band", "eroded"), R.object_masks(inside), (whole, band, core)):
        p, r = NP.epe(plain, true, mask), NP.epe(refined, true, mask)
        print(size, name, f"plain {p:.4f} refined {r:.4f} ratio {r / p:.3f}")
        assert cap is None or r <= cap * p, name


def test_refinement_off_is_the_plain_flow_and_finest_follows_the_step_3_rule():
    a, b, _, _ = NP.pair(("zoom", 0.04), 33, 65)
    assert np.array_equal(R.dense_flow(a, b, refine_params=None), NP.dense_flow(a, b))
    assert np.array_equal(R.dense_flow(a, b, refine_params=False, finest=1), NP.dense_flow(a, b, finest=1))
    pa, pb = NP.pyramid(NP.gray(a)), NP.pyramid(NP.gray(b))
    lvl1 = R.refine(pa[1], pb[1], NP.densify(pa[1], pb[1], NP.patch_search(pa[1], pb[1])))
    assert np.array_equal(R.dense_flow(a, b, finest=1), 2 * lvl1[:, np.arange(33)[:, None] // 2, np.arange(65)[None] // 2])
    with pytest.raises(ValueError, match="unknown"):
        R.dense_flow(a, b, refine_params=dict(sigma=1))


# ------------------------------------------------------------------------------------------------ tiling is exact
@pytest.mark.parametrize("sor", [1, 3, R.SOR_CAP])
def test_an_iteration_on_a_tile_and_its_halo_is_the_global_iteration_bit_for_bit(sor):
    """float32, 40 x 70, every 32 x 32 tile position (image corners included).  The crop is the tile plus 2 sor pixels (the
    distance the red-black half-sweeps carry a value) plus the 2 pixels the smoothness weights of the outermost of those read;
    at the crop's own border the weights are those of an image border, i.e. wrong, and 2 sor half-sweeps carry that error to
    within one pixel of the tile, not into it.  From du = dv = 0 (the first iteration) and from the result of that (the second)."""
    h, w = R.MULTI_TILE
    th, tw = R.TILE
    ia, ib, init = NP.level_pair(h, w, 1, True, False)
    flow = init[0]
    planes = R.prepare(ia[0], ib[0], flow, np.float32)
    zero = np.zeros((h, w), np.float32)
    first = R.outer_iteration(planes, flow[0], flow[1], zero, zero, sor=sor)
    second = R.outer_iteration(planes, flow[0], flow[1], *first, sor=sor)
    assert first[0].dtype == np.float32 and np.abs(first[0]).max() > 0.1 and not np.array_equal(first[0], second[0])
    margin = 2 * sor + 2
    for (du, dv), want in (((zero, zero), first), (first, second)):
        for ty in range(0, h, th):
            for tx in range(0, w, tw):
                y0, y1, x0, x1 = max(ty - margin, 0), min(ty + th + margin, h), max(tx - margin, 0), min(tx + tw + margin, w)
                crop = lambda A: np.ascontiguousarray(A[y0:y1, x0:x1])
                got = R.outer_iteration([crop(P) for P in planes], crop(flow[0]), crop(flow[1]), crop(du), crop(dv), sor=sor,
                                        origin=(y0, x0))
                for g, wnt in zip(got, want):
                    assert np.array_equal(g[ty - y0:ty - y0 + th, tx - x0:tx - x0 + tw], wnt[ty:ty + th, tx:tx + tw]), (ty, tx)
    # one pixel less is not enough at the cap: the property is not vacuous
    if sor == R.SOR_CAP:
        m, ty, tx = 2 * sor - 2, 0, 32
        x0, x1, y1 = tx - m, min(tx + tw + m, w), th + m
        got = R.outer_iteration([P[:y1, x0:x1] for P in planes], flow[0][:y1, x0:x1], flow[1][:y1, x0:x1], zero[:y1, x0:x1],
                                zero[:y1, x0:x1], sor=sor, origin=(0, x0))
        assert not np.array_equal(got[0][:th, m:m + tw], first[0][:th, tx:tx + tw])


# ------------------------------------------------------------------------------------------------ the GPU tests' tolerance
def test_tolerance_is_sixteen_times_the_float32_gap_of_the_restatement():
    gap = 0.0
    for h, w, n, corner, leave in R.stage_cases():
        ia, ib, init = NP.level_pair(h, w, n, corner, leave)
        for i in range(n):
            for kw in ({}, dict(outer=1, sor=1)):
                r32 = R.refine(ia[i], ib[i], init[i], dtype=np.float32, **kw)
                assert r32.dtype == np.float32
                gap = max(gap, float(np.abs(R.refine(ia[i], ib[i], init[i], **kw) - r32).max()))
    print("float32 - float64 gap of refine", gap, "TOL", R.TOL)
    assert 0 < gap <= R.MEASURED_GAP == R.TOL / 16
    assert gap >= 0.5 * R.MEASURED_GAP                                # the constant is the measurement, not a loose bound


def test_whole_refined_flow_in_float32_is_far_inside_the_whole_flow_condition():
    """The GPU tests allow 1 % of the pixels of a whole flow beyond 1e-3 px of float64.  The restatement's own float32 run has
    none (measured: at most 3.0e-4 px, on the (7.5, 3.25) shift at 64 x 128; 1.2e-4 px on the two-layer scene)."""
    worst = 0.0
    pairs = [NP.pair(m, *size)[:2] for size, m in NP.FULL_CASES] + [NP.two_layer(64, 128)[:2]]
    for a, b in pairs:
        diff = np.abs(R.dense_flow(a, b) - R.dense_flow(a, b, dtype=np.float32)).max(0)
        worst = max(worst, float(diff.max()))
        assert (diff > 1e-3).mean() == 0
    print("whole refined flow, float32 - float64: max", worst)
