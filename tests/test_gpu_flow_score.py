"""The flow scores on the GPU (run with -m gpu): csrc/flow_score.hip against the float64 restatement (tests/flow_score_np.py).
Counts and the `inconsistent` map are equal; the photo / fb maps are within one fp32 ulp (a double-rounded sqrt), NaN in the same
places; a non-negative sum of n float64 terms is within n * 2^-52 relative (both sides add correctly rounded terms and differ in
the order alone); sum_ae within 1e-9 relative (device and numpy acos may differ by a few ulp per term: a bound, the largest gap
seen is printed).  Then bit identity across calls, batches, maps, regions and streams; the launcher's refusals; end to end on
train.compute_flow's dict; and the ordering of the usefulness check of tests/test_flow_score_cpu.py with flow.dense_flow."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dense_flow_np as D
import flow_score_np as S
import gpu_util
from c2m_amd import _lib, evaluate, flow as F, ops, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (8, 8), (9, 13), (21, 37), (40, 70)]
# The tile kernels hand one partial per 1024 pixels to a reduce kernel of 1024 threads = 8 slices x 128 value slots; slice s adds
# the tiles s, s + 8, ...  130 x 140 = 18,200 pixels are 18 tiles: 18 x 90 = 1,620 (18 x 63 = 1,134) partial values, more than
# the 1024 threads, and every slice runs a second lap (slices 0 and 1 a third).
LARGE = (130, 140)
EPS = 2.0 ** -52
QC, CC = S.QC, S.CC
ae_gap = [0.0]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # a copy: the cached inputs are read-only


def as_dtype(x, dtype):
    """(device tensor in `dtype`, the float32 numpy array of exactly those values)."""
    t = dev(x).to(dtype)
    return t, t.float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(H, W, N, C, seed=0):
    """Flows with an exact-integer part, a half-pixel part, a part that lands exactly on the last row / column and half a pixel
    before it (the corners x1 = min(x0 + 1, W - 1)), large values that leave the frame, NaN and Inf; targets with NaN, Inf and
    1e10; errors on the thresholds themselves (e2 = 1, 9, 25 exactly); a sparse `valid`; random region bytes."""
    rng = np.random.default_rng(1000 * H + 10 * W + N + 7 * C + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    kind = rng.integers(0, 8, (N, H, W))
    whole = rng.integers(-2, 3, (N, 2, H, W)).astype(np.float32)
    smooth = rng.uniform(-3, 3, (N, 2, H, W)).astype(np.float32)
    last = np.stack([W - 1 - xx, H - 1 - yy])[None].repeat(N, 0)

    def mix(k0):
        f = np.where(kind[:, None] == k0 % 8, whole, smooth)
        f = np.where(kind[:, None] == (k0 + 1) % 8, whole + 0.5, f)
        f = np.where(kind[:, None] == (k0 + 2) % 8, last, f)
        f = np.where(kind[:, None] == (k0 + 3) % 8, last - 0.5, f)
        f = np.where((kind[:, None] == (k0 + 4) % 8) & (rng.random((N, 1, H, W)) < 0.3), np.float32(1e4), f)
        f = np.where((kind[:, None] == (k0 + 4) % 8) & (rng.random((N, 2, H, W)) < 0.1), np.float32(-1e30), f)
        f = np.where(rng.random((N, 2, H, W)) < 0.02, np.float32(np.nan), f)
        return np.where(rng.random((N, 2, H, W)) < 0.01, np.float32(np.inf), f).astype(np.float32)

    flow_ab, flow_ba = mix(0), mix(1)
    if H * W == 1:
        flow_ab[0] = 0.0                                  # one pair whose only pixel stays inside
    target = (mix(2) * 4).astype(np.float32)
    target = np.where(rng.random((N, 2, H, W)) < 0.03, np.float32(1e10), target)
    step = np.array([0, 1, -1, 3, -3, 4, 5, 0.5], np.float32)[rng.integers(0, 8, (N, 2, H, W))]
    pred = np.where(kind[:, None] < 5, target + step, target + rng.normal(0, 2, (N, 2, H, W)).astype(np.float32)).astype(np.float32)
    pred = np.where(rng.random((N, 2, H, W)) < 0.02, np.float32(np.nan), pred)
    pred = np.where(rng.random((N, 2, H, W)) < 0.01, np.float32(-np.inf), pred).astype(np.float32)
    a = rng.uniform(-1, 2, (N, C, H, W)).astype(np.float32)
    b = rng.uniform(-1, 2, (N, C, H, W)).astype(np.float32)
    valid = (rng.random((N, H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (N, H, W)).astype(np.uint8)
    regions = rng.integers(0, 256, (N, H, W)).astype(np.uint8)
    out = dict(flow_ab=flow_ab, flow_ba=flow_ba, target=target, pred=pred, a=a, b=b, valid=valid, regions=regions)
    for v in out.values():
        v.setflags(write=False)
    return out


def region_variants(x):
    """(name, valid, regions): both absent, both present, every bit, no bit."""
    return [("absent", None, None), ("present", x["valid"], x["regions"]), ("every bit", x["valid"], np.full_like(x["regions"], 255)),
            ("no bit", None, np.zeros_like(x["regions"]))]


def check_sums(got, want, count_cols, sum_terms, ae_col=None, what=""):
    """got / want [N,9,K]; count_cols equal; sum_terms {column: [N,9] number of terms} within terms * 2^-52 relative."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float64, what
    for c in count_cols:
        assert np.array_equal(got[..., c], want[..., c]), (what, "count column", c, got[..., c], want[..., c])
    for c, terms in sum_terms.items():
        if np.isnan(want[..., c]).all():
            assert np.isnan(got[..., c]).all(), (what, c)
            continue
        gap = np.abs(got[..., c] - want[..., c])
        assert (got[..., c] >= 0).all() and (gap <= terms * EPS * want[..., c]).all(), (what, "sum column", c, gap.max())
    if ae_col is not None:
        gap = np.abs(got[..., ae_col] - want[..., ae_col])
        rel = float((gap / np.maximum(want[..., ae_col], 1e-300)).max())
        ae_gap[0] = max(ae_gap[0], rel)
        assert (gap <= 1e-9 * want[..., ae_col]).all(), (what, "sum_ae", rel)


def quality_terms(want):
    fin = want[..., QC["n"]] - want[..., QC["n_nonfinite"]]
    return {c: fin for c in (QC["sum_epe"], QC["sum_e2"], QC["sum_mag"])}


def consistency_terms(want):
    n_in = want[..., CC["n_inside"]]
    return {CC["sum_photo"]: n_in, CC["sum_photo2"]: n_in, CC["sum_fb"]: n_in,
            CC["sum_photo_cons"]: n_in - np.nan_to_num(want[..., CC["n_incons"]])}


def ulps(got, want):
    """Largest distance in fp32 steps between two non-negative float32 arrays with NaN in the same places."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0
    return int(np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64)).max())


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES + [LARGE])
def test_flow_quality_sums_vs_the_restatement(H, W, N, dtype):
    x = inputs(H, W, N, 1)
    pred, pred_np = as_dtype(x["pred"], dtype)
    target = dev(x["target"])
    for name, valid, regions in region_variants(x):
        got = evaluate.flow_quality_sums(pred, target, None if valid is None else dev(valid), None if regions is None else dev(regions))
        want = S.flow_quality_sums(pred_np, x["target"], valid, regions)
        assert got.shape == (N, 9, 10) and got.dtype == torch.float64 and got.device == pred.device
        check_sums(got, want, S.COUNT_Q, quality_terms(want), QC["sum_ae"], what=(H, W, N, name))
        if name == "every bit":
            assert torch.equal(got[:, 1:], got[:, :1].expand(-1, 8, -1))
        if name in ("absent", "no bit"):
            assert float(got[:, 1:].abs().max()) == 0.0
    print(f"largest relative sum_ae gap so far: {ae_gap[0]:.3e} (bound 1e-9)")
    if H * W > 1:
        assert want[:, 0, QC["n_nonfinite"]].sum() > 0 and want[:, 0, QC["n"]].sum() < N * H * W


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES + [LARGE])
def test_flow_consistency_sums_vs_the_restatement(H, W, N, C, dtype):
    x = inputs(H, W, N, C)
    (a, a_np), (b, b_np) = as_dtype(x["a"], dtype), as_dtype(x["b"], dtype)
    fab, fba = dev(x["flow_ab"]), dev(x["flow_ba"])
    worst = 0
    for name, _, regions in region_variants(x):
        for ba, ba_np in ((fba, x["flow_ba"]), (None, None)):
            got, maps = evaluate.flow_consistency_sums(fab, a, b, ba, None if regions is None else dev(regions), maps=True)
            want, want_maps = S.flow_consistency_sums(x["flow_ab"], a_np, b_np, ba_np, regions)
            assert got.shape == (N, 9, 7) and maps["photo"].shape == (N, H, W) and maps["photo"].dtype == torch.float32
            assert maps["inconsistent"].dtype == torch.uint8 and maps["fb"].shape == (N, H, W)
            counts = S.COUNT_C if ba is not None else (0, 1)
            check_sums(got, want, counts, consistency_terms(want), what=(H, W, N, C, name, ba is not None))
            assert np.array_equal(maps["inconsistent"].cpu().numpy(), want_maps["inconsistent"])
            worst = max(worst, ulps(maps["photo"].cpu().numpy(), want_maps["photo"]), ulps(maps["fb"].cpu().numpy(), want_maps["fb"]))
            if ba is None:
                assert torch.isnan(got[..., 4:]).all() and torch.isnan(maps["fb"]).all() and int(maps["inconsistent"].max()) == 0
    print(f"photo / fb maps: at most {worst} fp32 ulp from float64")
    assert worst <= 1
    assert want[:, 0, CC["n_inside"]].sum() > 0
    if H * W > 1:
        assert want[:, 0, CC["n_inside"]].sum() < N * H * W


def test_strided_five_d_views_go_in_as_they_are():
    """[B,2,T,H,W] as flows[:, :, 1:] of a larger tensor (B-, C- and T-strided), against the restatement on the copied pairs,
    and against the call on a contiguous copy bit for bit; a frame repeated along T by expand() (stride 0) likewise."""
    Bn, T, H, W = 2, 3, 21, 37
    x = inputs(H, W, Bn * (T + 1), 3)
    five = lambda k, c: dev(x[k]).reshape(Bn, T + 1, c, H, W).transpose(1, 2)       # [B,c,T+1,H,W], not contiguous
    flat = lambda t: t.transpose(1, 2).reshape(Bn * T, -1, H, W).cpu().numpy()
    pred, target, fab, fba, a, b = (five(k, c)[:, :, 1:] for k, c in (("pred", 2), ("target", 2), ("flow_ab", 2), ("flow_ba", 2),
                                                                     ("a", 3), ("b", 3)))
    valid, regions = (dev(x[k]).reshape(Bn, T + 1, H, W)[:, 1:] for k in ("valid", "regions"))
    assert not pred.is_contiguous() and not a.is_contiguous()
    got = evaluate.flow_quality_sums(pred, target, valid, regions)
    assert got.shape == (Bn, T, 9, 10)
    want = S.flow_quality_sums(flat(pred), flat(target), valid.reshape(-1, H, W).cpu().numpy(), regions.reshape(-1, H, W).cpu().numpy())
    check_sums(got.reshape(Bn * T, 9, 10), want, S.COUNT_Q, quality_terms(want), QC["sum_ae"])
    assert torch.equal(got, evaluate.flow_quality_sums(pred.contiguous(), target.contiguous(), valid, regions))
    got, maps = evaluate.flow_consistency_sums(fab, a, b, fba, regions, maps=True)
    assert got.shape == (Bn, T, 9, 7) and maps["fb"].shape == (Bn, T, H, W)
    want, want_maps = S.flow_consistency_sums(flat(fab), flat(a), flat(b), flat(fba), regions.reshape(-1, H, W).cpu().numpy())
    check_sums(got.reshape(Bn * T, 9, 7), want, S.COUNT_C, consistency_terms(want))
    assert np.array_equal(maps["inconsistent"].reshape(-1, H, W).cpu().numpy(), want_maps["inconsistent"])
    again = evaluate.flow_consistency_sums(fab.contiguous(), a.contiguous(), b.contiguous(), fba.contiguous(), regions)
    assert torch.equal(got, again)
    one = b[:, :, :1].expand(-1, -1, T, -1, -1)                                     # the same frame b for every t
    assert one.stride(2) == 0
    assert torch.equal(evaluate.flow_consistency_sums(fab, a, one, fba), evaluate.flow_consistency_sums(fab, a, one.contiguous(), fba))


# ------------------------------------------------------------------------------------------------ bit identity
def test_sums_are_repeatable_and_independent_of_batch_maps_and_regions():
    H, W, N = 21, 37, 3
    x = inputs(H, W, N, 3)
    pred, target, valid, regions, fab, fba, a, b = (dev(x[k]) for k in ("pred", "target", "valid", "regions", "flow_ab", "flow_ba", "a", "b"))
    q = evaluate.flow_quality_sums(pred, target, valid, regions)
    c = evaluate.flow_consistency_sums(fab, a, b, fba, regions)
    same = lambda u, v: torch.equal(u.view(torch.int64), v.view(torch.int64))         # NaN == NaN
    assert same(evaluate.flow_quality_sums(pred, target, valid, regions), q)
    assert same(evaluate.flow_consistency_sums(fab, a, b, fba, regions), c)
    for i in range(N):
        s = slice(i, i + 1)
        assert same(evaluate.flow_quality_sums(pred[s], target[s], valid[s], regions[s])[0], q[i]), i
        assert same(evaluate.flow_consistency_sums(fab[s], a[s], b[s], fba[s], regions[s])[0], c[i]), i
    with_maps, maps = evaluate.flow_consistency_sums(fab, a, b, fba, regions, maps=True)
    assert same(with_maps, c)
    none, zero = evaluate.flow_quality_sums(pred, target, valid), evaluate.flow_quality_sums(pred, target, valid, torch.zeros_like(regions))
    assert same(none, zero) and same(none[:, 0], q[:, 0])
    none, zero = evaluate.flow_consistency_sums(fab, a, b, fba), evaluate.flow_consistency_sums(fab, a, b, fba, torch.zeros_like(regions))
    assert same(none, zero) and same(none[:, 0], c[:, 0])
    no_ba = evaluate.flow_consistency_sums(fab, a, b)
    assert same(no_ba[..., :4], none[..., :4])
    r = evaluate.flow_consistency(fab, a, b, fba, regions, region_names=evaluate.FLOW_REGIONS, maps=True)
    assert same(r["sums"], c.cpu()) and torch.equal(r["inconsistent_map"], maps["inconsistent"]) and r["region_photo"].shape == (N, 7)
    assert same(evaluate.flow_quality(pred, target, valid, regions)["sums"], q.cpu())


def test_scores_run_in_stream_order():
    """On a side stream, right behind the producers of their inputs on that stream, with the producers held back."""
    H, W, N = LARGE[0], LARGE[1], 2
    x = inputs(H, W, N, 3)
    keys = ("pred", "target", "flow_ab", "flow_ba", "a", "b", "regions")
    want_q = evaluate.flow_quality_sums(dev(x["pred"]), dev(x["target"]), None, dev(x["regions"]))
    want_c, want_m = evaluate.flow_consistency_sums(*(dev(x[k]) for k in ("flow_ab", "a", "b", "flow_ba", "regions")), maps=True)
    host = {k: torch.from_numpy(np.array(x[k])).pin_memory() for k in keys}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, want_q, want_c, want_m["photo"], want_m["fb"], *(dev(x[k]) for k in keys[:-1]))   # the float blocks
        gpu_util.stretch(side, 20.0)
        d = {k: v.to(DEV, non_blocking=True) for k, v in host.items()}            # queued behind the delay
        got_q = evaluate.flow_quality_sums(d["pred"], d["target"], None, d["regions"])
        got_c, got_m = evaluate.flow_consistency_sums(d["flow_ab"], d["a"], d["b"], d["flow_ba"], d["regions"], maps=True)
    side.synchronize()
    assert torch.equal(got_q, want_q) and torch.equal(got_c, want_c)
    for k in want_m:
        assert torch.equal(got_m[k].view(torch.int32) if got_m[k].dtype == torch.float32 else got_m[k],
                           want_m[k].view(torch.int32) if want_m[k].dtype == torch.float32 else want_m[k]), k


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_come_before_any_launch(monkeypatch):
    monkeypatch.setattr(evaluate._lib, "lib", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(evaluate.ops, "_stream", lambda: pytest.fail("a stream was asked for"))
    f, img = torch.zeros(2, 2, 4, 5, device=DEV), torch.zeros(2, 3, 4, 5, device=DEV)
    u8 = torch.zeros(2, 4, 5, dtype=torch.uint8, device=DEV)
    Q, C = evaluate.flow_quality_sums, evaluate.flow_consistency_sums
    for bad in (lambda: Q(f.double(), f), lambda: Q(f, f.bfloat16()), lambda: Q(f, f, u8.int()), lambda: Q(f, f, None, u8.float()),
                lambda: C(f.bfloat16(), img, img), lambda: C(f, img.half(), img), lambda: C(f, img, img.double()),
                lambda: C(f, img, img, f.half()), lambda: C(f, img, img, alpha2=None)):
        with pytest.raises(TypeError):
            bad()
    four = torch.zeros(2, 4, 4, 5, device=DEV)
    for bad in (lambda: Q(f[0], f[0]), lambda: Q(f, f[:1]), lambda: Q(f, f[..., :4]), lambda: Q(f, f, u8[:1]),
                lambda: Q(f, f, None, u8[:, :3]), lambda: Q(f, f, u8.cpu()), lambda: Q(f, f, None, u8.cpu()), lambda: Q(f, f.cpu()),
                lambda: C(f, four, four), lambda: C(f, img[:, :2], img[:, :2]), lambda: C(f, img, img[:, :1]), lambda: C(f, img[:1], img),
                lambda: C(f, img, img, f[:, :, :3]), lambda: C(f, img, img, regions=u8.cpu()), lambda: C(f, img.cpu(), img),
                lambda: C(f, img, img, alpha1=-1e-9), lambda: C(f, img, img, alpha1=float("inf")), lambda: C(f, img, img, alpha2=float("nan"))):
        with pytest.raises(ValueError):
            bad()


def test_launchers_refuse_bad_arguments():
    L = _lib.lib()
    B, T, H, W = 2, 1, 9, 13
    f, img = torch.zeros(B, 2, H, W, device=DEV), torch.zeros(B, 3, H, W, device=DEV)
    out_q, out_c = torch.full((B, 9, 10), 7.0, device=DEV, dtype=torch.float64), torch.full((B, 9, 7), 7.0, device=DEV, dtype=torch.float64)
    nq, nc = L.c2m_flow_quality_workspace_bytes(B, T, H, W), L.c2m_flow_consistency_workspace_bytes(B, T, H, W)
    assert nq == B * 1 * 90 * 8 and nc == B * 1 * 63 * 8 and L.c2m_flow_quality_workspace_bytes(1, 1, 130, 140) == 18 * 90 * 8
    assert L.c2m_flow_quality_workspace_bytes(1, 1, 0, 4) == -1 and L.c2m_flow_consistency_workspace_bytes(-1, 1, 4, 4) == -1
    work = torch.zeros(nq // 8, device=DEV, dtype=torch.float64)
    dense = (2 * H * W, H * W, 0)

    def quality(dt=0, H=H, sp=dense, nbytes=nq, out=out_q, pred=f):
        return L.c2m_flow_quality(ops._p(pred), ops._p(f), None, None, dt, B, T, H, W, (ctypes.c_long * 3)(*sp), (ctypes.c_long * 3)(*dense),
                                  ops._p(work), nbytes, ops._p(out), ops._stream())

    def consistency(C=3, dt=0, a1=0.01, a2=0.5, nbytes=nc, s1=H * W, maps=(None, None, None)):
        st = dense + (3 * H * W, s1, 0) + (3 * H * W, H * W, 0) + (0, 0, 0)
        return L.c2m_flow_consistency(ops._p(f), ops._p(img), ops._p(img), None, None, dt, B, C, T, H, W, (ctypes.c_long * 12)(*st), a1, a2,
                                      *maps, ops._p(work), nbytes, ops._p(out_c), ops._stream())

    for bad in (dict(dt=2), dict(H=0), dict(sp=(2 * H * W, H * W - 1, 0)), dict(sp=(-1, H * W, 0)), dict(nbytes=nq - 8), dict(out=None),
                dict(pred=None)):
        assert quality(**bad) != 0, bad
    for bad in (dict(C=2), dict(C=4), dict(dt=-1), dict(a1=-0.5), dict(a2=float("nan")), dict(a1=float("inf")), dict(nbytes=nc - 8),
                dict(s1=H * W - 1), dict(maps=(ops._p(out_c), None, None))):
        assert consistency(**bad) != 0, bad
    torch.cuda.synchronize()
    assert float(out_q.min()) == 7.0 and float(out_c.min()) == 7.0            # nothing was launched
    assert quality() == 0 and consistency() == 0
    torch.cuda.synchronize()
    assert out_q[:, 0, 0].tolist() == [H * W] * B and out_c[:, 0, 1].tolist() == [H * W] * B and bool(torch.isnan(out_c[..., 4:]).all())
    empty = evaluate.flow_quality_sums(f[:0], f[:0])
    assert empty.shape == (0, 9, 10) and evaluate.flow_consistency_sums(f[:0], img[:0], img[:0]).shape == (0, 9, 7)


# ------------------------------------------------------------------------------------------------ end to end
def test_clip_flow_check_and_flow_score_on_compute_flow():
    """train.compute_flow(ClassicFlow(), use_fw_of) on dense_flow_np.moving_boxes_clip(): clip_flow_check against the restatement
    on the same device flows; flow_quality of target_bw_of against the clip's known motion through flow_regions and FlowScore."""
    video, inst = D.moving_boxes_clip()
    t_in, t_out = 2, video.shape[1] - 2
    H, W = video.shape[2:]
    vid = dev(video)[None]
    flows = train.compute_flow(F.ClassicFlow(), dict(video=vid), dict(num_input_frames=t_in, num_predicted_frames=t_out, use_fw_of=True))
    check = evaluate.clip_flow_check(vid, flows, t_in, maps=True)
    assert set(check) == {"target_bw", "target_fw", "input"}
    host = {k: v[0].cpu().numpy() for k, v in flows.items()}                       # [2,frames,H,W]
    frames = lambda idx: np.stack([video[:, i] for i in idx])
    future, last = frames(range(t_in, t_in + t_out)), frames([t_in - 1] * t_out)
    pairs = {"target_bw": (host["target_bw_of"], future, last, host["target_fw_of"]),
             "target_fw": (host["target_fw_of"], last, future, host["target_bw_of"]),
             "input": (host["input_of"], frames(range(t_in - 1)), frames(range(1, t_in)), None)}
    for k, (f, a, b, g) in pairs.items():
        want, want_maps = S.flow_consistency_sums(f.transpose(1, 0, 2, 3), a, b, None if g is None else g.transpose(1, 0, 2, 3))
        got = check[k]["sums"]
        assert got.shape == (1, len(a), 9, 7)
        check_sums(got[0].numpy(), want, S.COUNT_C if g is not None else (0, 1), consistency_terms(want), what=k)
        assert np.array_equal(check[k]["inconsistent_map"][0].cpu().numpy(), want_maps["inconsistent"])
        ref = S.consistency_from_sums(want)
        for key in ("photo", "photo_consistent", "fb", "inconsistent", "outside"):
            assert np.allclose(check[k][key][0].numpy(), ref[key][:, 0], rtol=1e-12, atol=0, equal_nan=True), (k, key)
        print(k, {key: [round(float(v), 4) for v in check[k][key][0]] for key in ("photo", "fb", "inconsistent")})
    assert torch.isnan(check["input"]["fb"]).all() and not torch.isnan(check["target_bw"]["fb"]).any()

    # the known motion: box k moves (dx, dy) per frame, so target_bw_of[:, :, i] is -(i + 1) (dx, dy) on the box in frame t_in + i
    truth = np.zeros((t_out, 2, H, W), np.float32)
    for i in range(t_out):
        for (ident, _, _, _, _, (dx, dy)) in D.CLIP_BOXES:
            m = inst[t_in + i] == ident
            truth[i, 0][m], truth[i, 1][m] = -(i + 1) * dx, -(i + 1) * dy
    truth_d = dev(truth.transpose(1, 0, 2, 3))[None]                               # [1,2,T,H,W]
    ids = dev(inst[t_in:t_in + t_out])[None]
    regions = evaluate.flow_regions(truth_d, instance=ids)
    assert np.array_equal(regions[0].cpu().numpy(), S.flow_regions(truth, inst[t_in:t_in + t_out]))
    r = evaluate.flow_quality(flows["target_bw_of"], truth_d, regions=regions, region_names=evaluate.FLOW_REGIONS)
    want = S.flow_quality_sums(host["target_bw_of"].transpose(1, 0, 2, 3), truth, None, regions[0].cpu().numpy())
    check_sums(r["sums"][0].numpy(), want, S.COUNT_Q, quality_terms(want), QC["sum_ae"])
    score = evaluate.FlowScore()
    score.update(r)
    out = score.result()
    area = sum(h * w for (_, _, _, h, w, _) in D.CLIP_BOXES)
    assert out["pairs"] == t_out and out["pixels"] == t_out * H * W and out["nonfinite"] == 0
    assert out["object_pixels_per_frame"] == [area] * t_out and out["background_pixels"] == t_out * (H * W - area)
    assert out["slow_pixels_per_frame"] == [H * W] * 3 + [H * W - area] * 2        # 3, 6, 9 px, then 12 and 15 px
    assert out["medium_pixels_per_frame"] == [0] * 3 + [area] * 2 and out["fast_pixels"] == 0 and out["occluded_pixels"] == 0
    ref = S.quality_from_sums(want.sum(0))
    assert abs(out["epe"] - ref["epe"][0]) <= 1e-12 * ref["epe"][0] and abs(out["object_fl"] - ref["fl"][1]) <= 1e-12
    print("object epe per frame", out["object_epe_per_frame"], "background", out["background_epe_per_frame"])
    # a search from zero flow reaches 3 px and loses 15 px, and the static background is easier than the boxes
    assert out["object_epe_per_frame"][0] < out["object_epe_per_frame"][-1] and out["background_epe"] < out["object_epe"]


@pytest.mark.parametrize("scene", ["two_layer", "shift"])
def test_ordering_of_the_usefulness_check_with_the_gpu_search(scene):
    """The scenes and the assertion of tests/test_flow_score_cpu.py, with flow.dense_flow as the search and the GPU scores."""
    a, b, fwd, bwd = (S.two_layer_scene() if scene == "two_layer" else S.shift_scene())[:4]
    A, B_ = dev(a)[None], dev(b)[None]
    true_ab, true_ba = dev(fwd.astype(np.float32))[None], dev(bwd.astype(np.float32))[None]
    found_ab, found_ba = F.dense_flow(A, B_), F.dense_flow(B_, A)
    zero = torch.zeros_like(true_ab)
    r = {}
    for name, f, g in (("true", true_ab, true_ba), ("found", found_ab, found_ba), ("zero", zero, found_ba), ("zero_zero", zero, zero)):
        c, q = evaluate.flow_consistency(f, A, B_, g), evaluate.flow_quality(f, true_ab)
        r[name] = (float(c["photo"][0]), float(c["fb"][0]), float(q["epe"][0]))
    for i, name in enumerate(("photo", "fb", "epe")):
        t, f, z = r["true"][i], r["found"][i], r["zero"][i]
        print(f"{scene} {name}: true {t:.6g} found {f:.6g} zero {z:.6g}  margins {f - t:.6g} {z - f:.6g}")
        assert t < f < z, (scene, name, t, f, z)
    assert r["zero_zero"][1] == 0.0
