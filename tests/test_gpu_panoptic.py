"""Panoptic-DeepLab post-processing on the GPU (csrc/panoptic.hip, c2m_amd.segment): held to the numpy restatement
(tests/panoptic_np.py) and to the reference's own results (tests/golden/panoptic_reference.npz) with exact equality of semantic,
instance, panoptic, centers[:count] and center_count, on the cases of panoptic_np.cases(): offsets are multiples of 1/4 and
distances stay small enough for fp32 to be exact, so no tolerance and no excluded pixel is needed.  The one unquantised case
leaves out the pixels whose two nearest float64 distances are within 1e-5 relative (at most 0.1 % of the pixels)."""
import os

import numpy as np
import pytest
import torch

import panoptic_np as P
from c2m_amd import data, ops, segment

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panoptic_reference.npz")
CASE_NAMES = sorted(P.cases())


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return P.cases()


@pytest.fixture(scope="module")
def expected(cases):
    """The restatement's result of every case, computed once."""
    return {k: P.panoptic_batch(c["semantic"], c["center"], c["offset"], **c["params"]) for k, c in cases.items()}


def run(case, **over):
    heads = [torch.from_numpy(np.ascontiguousarray(case[k])).to(DEV) for k in ("semantic", "center", "offset")]
    m = segment.panoptic_maps(*heads, **{**case["params"], **over})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in m.items()}


def check(got, want, what):
    """got: the maps of N images; want: a list of N per-image dicts (restatement or fixture)."""
    top_k = got["centers"].shape[1]
    for n, w in enumerate(want):
        cnt = int(got["center_count"][n])
        assert cnt == len(w["centers"]), (what, n, cnt, len(w["centers"]))
        assert np.array_equal(got["centers"][n, :cnt], np.asarray(w["centers"], np.int64).reshape(-1, 2)), (what, n)
        assert not got["centers"][n, cnt:].any() and cnt <= top_k
        for key in ("semantic", "panoptic", "instance"):
            bad = got[key][n] != w[key]
            assert not bad.any(), (what, n, key, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_equals_restatement_and_reference(name, cases, expected, golden):
    got = run(cases[name])
    assert got["semantic"].dtype == np.uint8 and got["panoptic"].dtype == np.int32 and got["instance"].dtype == np.int32
    check(got, expected[name], name)
    N = cases[name]["center"].shape[0]
    ref = [{k: golden[f"{name}/{n}/{k}"] for k in ("semantic", "panoptic", "instance", "centers")} for n in range(N)]
    check(got, ref, name + " (reference)")


@pytest.mark.parametrize("name", ["off_tile_37x53", "off_tile_65x97", "many_centers_max"])
def test_batch_equals_single_calls(name, cases):
    c = cases[name]
    whole = run(c)
    for n in range(c["center"].shape[0]):
        one = run({k: (v[n:n + 1] if k != "params" else v) for k, v in c.items()})
        for key, v in one.items():
            assert np.array_equal(v[0], whole[key][n]), (name, n, key)


def test_image_without_candidates_keeps_stuff_only(cases):
    c = cases["off_tile_65x97"]
    got = run(c)
    sem = c["semantic"][1]
    assert got["center_count"].tolist() == [9, 0, 9]
    assert np.all(got["instance"][1][np.isin(sem, (11, 12, 13))] == 255) and np.all(got["panoptic"][1][sem == 8] == 8000)


def test_labels_uint8_int64_and_logits_agree(cases, expected):
    c = cases["logits"]
    from_logits = run(c)
    labels = np.stack([e["semantic"] for e in expected["logits"]])
    assert np.all(labels[:, 4:20, 5:30] == 3)                            # the exact two-way tie took the first class
    for dtype in (np.uint8, np.int64):
        from_labels = run({**c, "semantic": labels.astype(dtype)})
        for key, v in from_logits.items():
            assert np.array_equal(v, from_labels[key]), (dtype, key)


def test_unquantised_offsets_against_float64(golden):
    u = P.unquantised_case()
    want = P.panoptic_batch(u["semantic"], u["center"], u["offset"], **u["params"])[0]
    got = run(u)
    assert int(got["center_count"][0]) == 150 and np.array_equal(got["centers"][0, :150], want["centers"])
    near = P.near_tie_mask(want["two"])
    assert near.mean() <= 1e-3
    for key in ("semantic", "panoptic", "instance"):
        bad = (got[key][0] != want[key]) & ~near
        print(key, "differs on", int((got[key][0] != want[key]).sum()), "pixels,", int(bad.sum()), "outside", int(near.sum()),
              "near ties")
        assert not bad.any(), (key, int(bad.sum()))
    assert not ((got["panoptic"][0] != golden["unquantised/0/panoptic"]) & ~near).any()


def test_clip_maps_feed_assemble_batch_and_instance_boxes(cases):
    c = cases["off_tile_65x97"]
    B, T, h, w = 2, 3, 64, 96
    order = [0, 2, 1, 2, 0, 1]                                             # the frame without a centre is each sample's last
    heads = [torch.from_numpy(np.ascontiguousarray(c[k][order])).to(DEV) for k in ("semantic", "center", "offset")]
    labels, inst = segment.clip_maps(*heads, clip=(B, T), crop=(h, w), **c["params"])
    assert labels.shape == (B, T, h, w) and labels.dtype == torch.uint8 and labels.is_contiguous()
    assert inst.shape == (B, T, h, w) and inst.dtype == torch.int32 and inst.is_contiguous()
    whole = segment.panoptic_maps(*heads, **c["params"])
    assert torch.equal(inst, whole["instance"].view(B, T, 65, 97)[:, :, :h, :w])         # crop slices after the computation
    frames = torch.zeros(B, T, h, w, 3, dtype=torch.uint8, device=DEV)
    occ = torch.zeros(B, T - 2, h, w, dtype=torch.uint8, device=DEV)
    flow = torch.zeros(B, T - 2, h, w, 2, device=DEV)
    batch = data.assemble_batch(frames, labels, inst, occ, flow, None, size=(32, 48))
    im = batch["instance_mask"]
    assert im.shape == (B, 1, T, 32, 48) and batch["fg_mask"].shape == (B, 9, T, 32, 48)
    ids, boxes, count = ops.instance_boxes(im, 2)
    v = im.cpu().numpy()[:, 0]
    for b in range(B):
        things = [set(np.unique(f[(f > 1000) & (f < 19000)]).tolist()) for f in v[b, :2]]
        assert all(1000 < i < 19000 for s in things for i in s) and things[0] | things[1]
        assert int(count[b]) == len(things[0] & things[1])
        assert set(ids[b, :int(count[b])].tolist()) == things[0] & things[1]
    assert not np.isin(v, np.arange(256, 1001)).any()                      # everything else is a class or 255


def test_repeats_bit_for_bit_on_a_side_stream(cases):
    c = cases["many_centers_max"]
    heads = [torch.from_numpy(c[k]).to(DEV) for k in ("semantic", "center", "offset")]
    a = segment.panoptic_maps(*heads, **c["params"])
    side = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):
        big = big @ big * 1e-3                                             # the default stream is busy
    with torch.cuda.stream(side):
        b = segment.panoptic_maps(*heads, **c["params"])
        d = segment.panoptic_maps(*heads, **c["params"])
    side.synchronize()
    torch.cuda.synchronize()
    for key in a:
        assert torch.equal(a[key], b[key]) and torch.equal(b[key], d[key]), key


def test_refusals_on_the_device(cases):
    c = cases["threshold"]
    heads = [torch.from_numpy(c[k]).to(DEV) for k in ("semantic", "center", "offset")]
    with pytest.raises(ValueError, match="nms_kernel"):
        segment.panoptic_maps(*heads, nms_kernel=2)
    with pytest.raises(ValueError, match="label_divisor"):
        segment.panoptic_maps(*heads, top_k=1000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        segment.panoptic_maps(heads[0].cpu(), heads[1], heads[2])
    empty = segment.panoptic_maps(heads[0][:0], heads[1][:0], heads[2][:0])
    assert empty["semantic"].shape == (0, 20, 30) and empty["center_count"].shape == (0,)
