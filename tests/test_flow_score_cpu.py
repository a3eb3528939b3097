"""Flow scores without a GPU: closed forms of the float64 restatement (tests/flow_score_np.py), the counting
rules for NaN / Inf / invalid pixels, flow_regions against a brute-force loop, the host arithmetic and FlowScore of
c2m_amd.evaluate, the argument checks that come before any launch, and the usefulness check: in float64 the ground-truth-free
score ranks the true flow, the searched flow and the zero flow as the ground-truth score does."""
import math

import numpy as np
import pytest
import torch

import dense_flow_np as D
import flow_score_np as S
from c2m_amd import _lib, build, evaluate

QC, CC = S.QC, S.CC


def test_symbols_columns_and_build_flags():
    for name in ("c2m_flow_quality", "c2m_flow_quality_workspace_bytes", "c2m_flow_consistency",
                 "c2m_flow_consistency_workspace_bytes"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
    assert build.SOURCES["flow_score.hip"] == build.SOURCES["quality.hip"]          # -ffp-contract=off, no SLP vectoriser
    assert evaluate.FLOW_QUALITY_COLUMNS == S.QUALITY_COLUMNS and evaluate.FLOW_CONSISTENCY_COLUMNS == S.CONSISTENCY_COLUMNS
    assert evaluate.FLOW_REGIONS == S.REGIONS and evaluate.FLOW_SCORE_ROWS == S.ROWS


# ------------------------------------------------------------------------------------------------ closed forms: quality
def _const(u, v, H=6, W=7):
    return np.stack([np.full((H, W), float(u)), np.full((H, W), float(v))])[None].astype(np.float32)


def test_equal_flows_have_no_error():
    rng = np.random.default_rng(0)
    t = rng.integers(-20, 20, (2, 2, 6, 7)).astype(np.float32)
    s = S.flow_quality_sums(t, t)[:, 0]
    assert (s[:, QC["n"]] == 42).all()
    for k in ("n_nonfinite", "sum_epe", "sum_e2", "sum_ae", "n_out", "n_gt1", "n_gt3", "n_gt5"):
        assert (s[:, QC[k]] == 0).all(), k


def test_three_four_five():
    n = 42
    s = S.flow_quality_sums(_const(13, 4), _const(10, 0))[0, 0]
    assert s[QC["n"]] == n and s[QC["sum_epe"]] == 5 * n and s[QC["sum_e2"]] == 25 * n and s[QC["sum_mag"]] == 10 * n
    assert s[QC["n_gt1"]] == n and s[QC["n_gt3"]] == n
    assert s[QC["n_gt5"]] == 0                      # 25 > 25 is false
    assert s[QC["n_out"]] == n                      # 25 > 9 and 25 > 0.25
    s = S.flow_quality_sums(_const(203, 4), _const(200, 0))[0, 0]
    assert s[QC["sum_epe"]] == 5 * n and s[QC["n_gt3"]] == n
    assert s[QC["n_out"]] == 0                      # 25 > 100 is false


def test_nonfinite_and_invalid_pixels_follow_the_rule():
    pred, target = _const(13, 4), _const(10, 0)
    valid = np.ones((1, 6, 7), np.uint8)
    pred[0, 0, 0, 0] = np.nan                       # nonfinite: counted in n and in every threshold count, in no sum
    pred[0, 1, 0, 1] = np.inf
    target[0, 0, 1, 0] = 1e10                       # not scored
    target[0, 1, 1, 1] = np.nan                     # not scored
    target[0, 0, 1, 2] = np.inf                     # not scored
    valid[0, 2, 2] = 0                              # not scored
    pred[0, 0, 2, 2] = np.nan                       # ... whatever pred holds there
    s = S.flow_quality_sums(pred, target, valid)[0, 0]
    n = 42 - 4
    assert s[QC["n"]] == n and s[QC["n_nonfinite"]] == 2
    assert s[QC["sum_epe"]] == 5 * (n - 2) and s[QC["sum_e2"]] == 25 * (n - 2) and s[QC["sum_mag"]] == 10 * (n - 2)
    assert np.isfinite(s).all()
    assert s[QC["n_gt1"]] == n and s[QC["n_gt3"]] == n and s[QC["n_out"]] == n
    assert s[QC["n_gt5"]] == 2                      # only the two nonfinite pixels
    r = S.quality_from_sums(s[None])
    assert r["epe"][0] == 5.0 and r["bad5"][0] == 2 / n and r["nonfinite"][0] == 2


def test_region_rows_select_their_bit():
    pred, target = _const(13, 4), _const(10, 0)
    regions = np.zeros((1, 6, 7), np.uint8)
    regions[0, :2] = 1 | 128
    regions[0, 2:3] = 4
    s = S.flow_quality_sums(pred, target, None, regions)[0]
    assert s[:, QC["n"]].tolist() == [42, 14, 0, 7, 0, 0, 0, 0, 14]
    assert s[3, QC["sum_epe"]] == 35 and s[2, QC["sum_epe"]] == 0
    assert (S.flow_quality_sums(pred, target)[0, 1:] == 0).all()


def test_angular_error_of_orthogonal_unit_flows():
    s = S.flow_quality_sums(_const(1, 0), _const(0, 1))[0, 0]             # cos = 1 / (sqrt 2 sqrt 2) = 1/2
    assert abs(s[QC["sum_ae"]] / 42 - math.pi / 3) < 1e-14


# ------------------------------------------------------------------------------------------------ closed forms: consistency
@pytest.mark.parametrize("dx,dy", [(0, 0), (2, -1), (-3, 2), (7, 5)])
@pytest.mark.parametrize("C", [1, 3])
def test_integer_shift_with_true_flows(dx, dy, C):
    H, W = 9, 13
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, (C, H + 20, W + 20)).astype(np.float32)
    b = big[:, 10:10 + H, 10:10 + W][None]
    a = big[:, 10 + dy:10 + dy + H, 10 + dx:10 + dx + W][None]             # a(x) = b(x + (dx, dy))
    s, maps = S.flow_consistency_sums(_const(dx, dy, H, W), a, b, _const(-dx, -dy, H, W))
    s = s[0, 0]
    assert s[CC["n"]] == H * W and s[CC["n_inside"]] == (W - abs(dx)) * (H - abs(dy))
    assert s[CC["sum_photo"]] == 0 and s[CC["sum_photo2"]] == 0 and s[CC["sum_fb"]] == 0 and s[CC["n_incons"]] == 0
    assert s[CC["sum_photo_cons"]] == 0
    assert int(np.isnan(maps["photo"][0]).sum()) == H * W - (W - abs(dx)) * (H - abs(dy))
    s0, _ = S.flow_consistency_sums(_const(dx, dy, H, W), a, b)
    assert np.isnan(s0[0, :, 4:]).all() and (s0[0, 0, :4] == s[:4]).all()


def test_half_pixel_sample_and_nonfinite_flows():
    H, W = 4, 5
    b = np.arange(H * W, dtype=np.float32).reshape(1, 1, H, W)             # b(x, y) = 5 y + x: bilinear is exact
    a = b + 0.5 + 2.5                                                      # a(x) = b(x + (0.5, 0.5))
    f = _const(0.5, 0.5, H, W)
    f[0, 0, 0, 0] = np.nan
    f[0, 1, 0, 1] = np.inf
    f[0, 0, 1, 1] = 1e30
    s, maps = S.flow_consistency_sums(f, a, b, _const(-0.5, -0.5, H, W))
    inside = (W - 1) * (H - 1) - 3
    assert s[0, 0, CC["n_inside"]] == inside and s[0, 0, CC["sum_photo"]] == 0 and s[0, 0, CC["n_incons"]] == 0
    assert np.isnan(maps["photo"][0, 0, 0]) and np.isnan(maps["fb"][0, 1, 1]) and maps["inconsistent"].sum() == 0
    ba = _const(-0.5, -0.5, H, W)
    ba[0, 0, 2, 2] = np.nan                                                # read by the four pixels around it: inconsistent there
    s, maps = S.flow_consistency_sums(f, a, b, ba)
    assert s[0, 0, CC["n_incons"]] == maps["inconsistent"].sum() > 0 and np.isfinite(s[0, 0]).all()


# ------------------------------------------------------------------------------------------------ regions
def _region_case():
    rng = np.random.default_rng(5)
    N, H, W = 2, 20, 27
    target = np.zeros((N, 2, H, W), np.float32)
    target[:, 0, 5:12, 6:15] = 12.0
    target[1, 1, 14:18, 2:9] = -45.0
    target[0, 0, 19, 26] = 0.9                      # below the jump: no edge
    inst = np.full((N, H, W), 7, np.int32)
    inst[:, 5:12, 6:15] = 11001
    inst[1, 0:3, 20:27] = 19000                     # outside the id range, still an id border
    occ = rng.uniform(0, 1, (N, H, W)).astype(np.float32)
    return target, inst, occ


@pytest.mark.parametrize("band", [0, 1, 4])
@pytest.mark.parametrize("with_ids", [False, True])
def test_flow_regions_match_the_brute_force_restatement(band, with_ids):
    target, inst, occ = _region_case()
    want = S.flow_regions(target, inst if with_ids else None, occ, band=band)
    got = evaluate.flow_regions(torch.from_numpy(target), torch.from_numpy(inst) if with_ids else None,
                                torch.from_numpy(occ)[:, None], band=band).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    obj, bg = (got & 1) != 0, (got & 2) != 0
    assert np.array_equal(obj, ~bg) and obj.any() == with_ids
    speed = ((got >> 4) & 1).astype(int) + ((got >> 5) & 1) + ((got >> 6) & 1)
    assert (speed == 1).all()                       # the buckets partition the (finite) pixels
    assert ((got >> 4) & 7).max() == 4 and ((got & 32) != 0).any()
    assert ((got & 4) != 0).any() and not ((got & 4) != 0)[0, 15:, 20:].any()      # the 0.9 px step is no edge
    five = evaluate.flow_regions(torch.from_numpy(target).unsqueeze(2), None, None, band=band)          # [B=2,2,T=1,H,W]
    assert five.shape == (2, 1, 20, 27) and np.array_equal(five[:, 0].numpy(), S.flow_regions(target, band=band))


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_host_dicts_from_hand_made_sums():
    sums = np.zeros((2, 9, 10))
    sums[0, 0] = [100, 4, 96 * 2.0, 96 * 5.0, 96 * 3.0, 96 * math.pi / 6, 10, 50, 20, 8]
    sums[0, 2] = [10, 10, 0, 0, 0, 0, 10, 10, 10, 10]                      # a region of nonfinite pixels only
    sums[1, 0] = [7, 0, 7.0, 7.0, 0, 0, 0, 0, 0, 0]
    r = evaluate.flow_quality_from_sums(sums, region_names=("a", "b", "c"))
    assert r["epe"].tolist() == [2.0, 1.0] and r["rmse"][0] == math.sqrt(5.0) and abs(float(r["ae_deg"][0]) - 30.0) < 1e-12
    assert r["fl"].tolist() == [0.1, 0.0] and r["bad1"][0] == 0.5 and r["bad3"][0] == 0.2 and r["bad5"][0] == 0.08
    assert r["nonfinite"].tolist() == [4, 0] and r["pixels"].tolist() == [100, 7]
    assert r["region_epe"].shape == (2, 3) and torch.isnan(r["region_epe"]).all()             # empty, or no finite pixel
    assert r["region_fl"][0, 1] == 1.0 and torch.isnan(r["region_fl"][0, 0]) and torch.isnan(r["region_fl"][1]).all()
    want = S.quality_from_sums(sums)
    for k, v in want.items():
        assert np.array_equal(r[k].numpy(), v[:, 0], equal_nan=True) and np.array_equal(r["region_" + k].numpy(), v[:, 1:4],
                                                                                        equal_nan=True), k
    cs = np.zeros((1, 9, 7))
    cs[0, 0] = [200, 100, 50.0, 30.0, 25.0, 20, 16.0]
    c = evaluate.flow_consistency_from_sums(cs)
    assert c["photo"][0] == 0.5 and c["photo_consistent"][0] == 0.2 and c["fb"][0] == 0.25 and c["inconsistent"][0] == 0.2
    assert c["outside"][0] == 0.5 and c["region_photo"].shape == (1, 8) and torch.isnan(c["region_photo"]).all()
    cs[0, :, 4:] = np.nan                                                  # no reverse flow
    c = evaluate.flow_consistency_from_sums(cs)
    assert c["photo"][0] == 0.5 and all(torch.isnan(c[k][0]) for k in ("fb", "inconsistent", "photo_consistent"))
    want = S.consistency_from_sums(cs)
    for k, v in want.items():
        assert np.array_equal(c[k].numpy(), v[:, 0], equal_nan=True), k
    with pytest.raises(ValueError):
        evaluate.flow_quality_from_sums(cs)
    with pytest.raises(ValueError):
        evaluate.flow_quality_from_sums(sums, region_names=tuple("abcdefghi"))


def test_flow_score_two_updates_equal_the_concatenation(tmp_path):
    rng = np.random.default_rng(11)
    pred = rng.normal(0, 4, (6, 2, 12, 16)).astype(np.float32)
    target = rng.normal(0, 4, (6, 2, 12, 16)).astype(np.float32)
    regions = rng.integers(0, 128, (6, 12, 16)).astype(np.uint8)
    regions[:, :, :] &= ~np.uint8(8)                                        # an empty region
    sums = S.flow_quality_sums(pred, target, None, regions).reshape(3, 2, 9, 10)            # [B=3,T=2]
    one, two = evaluate.FlowScore(), evaluate.FlowScore()
    one.update(torch.from_numpy(sums))
    two.update({"sums": torch.from_numpy(sums[:1])})
    two.update(sums[1:])
    r1, r2 = one.result(), two.result()
    assert r1.keys() == r2.keys() and r1["pairs"] == 6
    for k in r1:
        assert np.array_equal(np.asarray(r1[k], np.float64), np.asarray(r2[k], np.float64), equal_nan=True), k
    q = S.quality_from_sums(sums)
    assert abs(r1["epe"] - S.quality_from_sums(sums.sum((0, 1)))["epe"][0]) < 1e-12         # pixel-weighted: Sintel's EPE
    assert abs(r1["epe_mean"] - q["epe"][..., 0].mean()) < 1e-12                           # mean over pairs
    assert np.allclose(r1["fl_mean_per_frame"], q["fl"][..., 0].mean(0), rtol=1e-12, atol=0)
    assert np.allclose(r1["boundary_bad1_per_frame"], S.quality_from_sums(sums.sum(0))["bad1"][:, 3], rtol=1e-12, atol=0)
    assert math.isnan(r1["occluded_epe"]) and math.isnan(r1["occluded_epe_mean"]) and r1["occluded_pixels"] == 0
    assert len(r1["epe_per_frame"]) == 2 and r1["pixels"] == 6 * 12 * 16
    path = tmp_path / "flow.txt"
    assert one.write(str(path)).keys() == r1.keys() and "fast_epe" in path.read_text()
    with pytest.raises(ValueError):
        two.update(torch.zeros(2, 3, 9, 10))                               # another number of frames
    with pytest.raises(ValueError):
        evaluate.FlowScore("consistency").update(torch.zeros(2, 9, 10))
    cons = evaluate.FlowScore("consistency", region_names=())
    cons.update(torch.ones(4, 9, 7))
    assert cons.result()["photo"] == 1.0 and cons.result()["pairs"] == 4


# ------------------------------------------------------------------------------------------------ checks before any launch
def test_argument_errors_come_before_the_device_is_touched():
    f, img = torch.zeros(2, 2, 4, 5), torch.zeros(2, 3, 4, 5)
    u8 = torch.zeros(2, 4, 5, dtype=torch.uint8)
    Q, C = evaluate.flow_quality_sums, evaluate.flow_consistency_sums
    for bad in (lambda: Q(f.double(), f), lambda: Q(f, f.bfloat16()), lambda: Q(None, f), lambda: Q(f, f, u8.float()),
                lambda: Q(f, f, None, u8.bool()), lambda: C(f.bfloat16(), img, img), lambda: C(f, img.half(), img),
                lambda: C(f, img, img, alpha1="1"), lambda: C(f, img, img, f.double())):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: Q(f[0], f[0]), lambda: Q(f, f[:1]), lambda: Q(f, f[..., :4]), lambda: Q(img, img),
                lambda: Q(f, f, u8[:1]), lambda: Q(f, f, None, u8[:, :3]), lambda: Q(f, f.reshape(1, 2, 2, 4, 5)),
                lambda: C(f, img[:, :2], img[:, :2]), lambda: C(f, img, img[:, :1]), lambda: C(f, img, img[:1]),
                lambda: C(f, img, img, f[:1]), lambda: C(f, img, img, alpha1=-0.1), lambda: C(f, img, img, alpha2=float("nan")),
                lambda: C(f, img, img, alpha2=float("inf")), lambda: C(f, img, img, regions=u8[..., :2]),
                lambda: evaluate.clip_flow_check(torch.zeros(1, 3, 3, 4, 5), {"target_bw_of": torch.zeros(1, 2, 2, 4, 5)}, 2),
                lambda: evaluate.flow_regions(f, band=-1), lambda: evaluate.flow_regions(f, instance=u8[:1])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ usefulness, in float64
def ranking(a, b, fwd, bwd):
    """(photo, fb, epe) of the true flow, the searched flow and the zero flow a -> b, each checked against the reverse flow of
    its own kind; the zero flow also against the searched reverse flow (a pair of zero flows cancels by construction)."""
    found_ab, found_ba = D.dense_flow(a, b), D.dense_flow(b, a)
    zero = np.zeros_like(fwd)
    out = {}
    for name, f, g in (("true", fwd, bwd), ("found", found_ab, found_ba), ("zero", zero, found_ba), ("zero_zero", zero, zero)):
        s, _ = S.flow_consistency_sums(f[None], a[None], b[None], g[None])
        c = S.consistency_from_sums(s)
        q = S.quality_from_sums(S.flow_quality_sums(f[None], fwd[None]))
        out[name] = (float(c["photo"][0, 0]), float(c["fb"][0, 0]), float(q["epe"][0, 0]))
    return out


@pytest.fixture(scope="module")
def rankings():
    return {"two_layer": ranking(*S.two_layer_scene()[:4]), "shift": ranking(*S.shift_scene()[:4])}


@pytest.mark.parametrize("scene", ["two_layer", "shift"])
def test_the_ground_truth_free_score_ranks_like_the_endpoint_error(rankings, scene):
    """Scenes: dense_flow_np.two_layer(64, 128, (24, 36), (3, -2)) and pair(("shift", (1.7, -0.9)), 64, 128), both at seed 0.
    photo and fb order true < found < zero strictly, as the endpoint error does.  The zero flow's fb is taken against the found
    reverse flow: against a zero reverse flow it is 0 by construction, which the last assertion records (what the
    check cannot see)."""
    r = rankings[scene]
    for i, name in enumerate(("photo", "fb", "epe")):
        t, f, z = r["true"][i], r["found"][i], r["zero"][i]
        print(f"{scene} {name}: true {t:.6g} found {f:.6g} zero {z:.6g}  margins {f - t:.6g} {z - f:.6g}")
        assert t < f < z, (scene, name, t, f, z)
    assert r["zero_zero"][1] == 0.0 and r["zero_zero"][0] == r["zero"][0]


def test_inconsistent_covers_the_occluded_strip():
    a, b, fwd, bwd, occluded = S.two_layer_scene()
    assert occluded.sum() > 0
    _, maps = S.flow_consistency_sums(fwd[None], a[None], b[None], bwd[None])
    inc = maps["inconsistent"][0] != 0
    assert inc[occluded].all()                          # fb^2 = 13 > 0.01 * 13 + 0.5 there
    assert np.array_equal(inc, occluded)                # and nowhere else: the true flows cancel everywhere else
    regions = occluded.astype(np.uint8)[None] * 8
    s, _ = S.flow_consistency_sums(fwd[None], a[None], b[None], bwd[None], regions)
    c = S.consistency_from_sums(s)
    print(f"two_layer true flows: photo {c['photo'][0, 0]:.6g}, consistent only {c['photo_consistent'][0, 0]:.6g}, "
          f"occluded strip {c['photo'][0, 4]:.6g}")
    assert c["inconsistent"][0, 4] == 1.0 and c["photo_consistent"][0, 0] == 0.0 and c["photo"][0, 4] > 0.01
