"""Panoptic-DeepLab post-processing without a GPU: the numpy restatement (tests/panoptic_np.py) is held to what the reference's
own post-processing computed for every case (tests/golden/panoptic_reference.npz, written by tools/capture_panoptic_golden.py),
with exact equality on every array; the stored inputs are the ones the case builders produce today; ops._panoptic_plan accepts
the good inputs and refuses every bad one before a launch; the entry points are declared and bound."""
import os

import numpy as np
import pytest
import torch

import panoptic_np as P
from c2m_amd import _lib, ops, segment

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panoptic_reference.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return P.cases()


CASE_NAMES = sorted(P.cases())


def test_the_fixture_holds_every_case(golden, cases):
    assert sorted({k.split("/")[0] for k in golden} - {"unquantised"}) == CASE_NAMES
    assert os.path.getsize(GOLDEN) < 2 ** 20


@pytest.mark.parametrize("name", CASE_NAMES)
def test_inputs_are_the_recorded_ones(golden, cases, name):
    c = cases[name]
    assert np.array_equal(golden[f"{name}/semantic_in"].astype(c["semantic"].dtype), c["semantic"])
    assert np.array_equal(golden[f"{name}/center_in"], c["center"])
    assert np.array_equal(golden[f"{name}/offset_q4"].astype(np.float32) / 4, c["offset"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_the_reference(golden, cases, name):
    c = cases[name]
    got = P.panoptic_batch(c["semantic"], c["center"], c["offset"], **c["params"])
    for n, r in enumerate(got):
        for key in ("semantic", "panoptic", "instance"):
            assert np.array_equal(r[key], golden[f"{name}/{n}/{key}"]), (name, n, key)
        assert np.array_equal(r["centers"], golden[f"{name}/{n}/centers"].astype(np.int64).reshape(-1, 2)), (name, n)


def test_cases_show_what_they_are_named_for(cases):
    res = {k: P.panoptic_batch(c["semantic"], c["center"], c["offset"], **c["params"]) for k, c in cases.items()}
    n = lambda k, i=0: len(res[k][i]["centers"])
    assert (n("topk_three_way_tie"), n("topk_all_tied"), n("topk_one"), n("topk_minus_one"), n("topk_exact")) == (6, 0, 0, 12, 11)
    assert n("positions") == 29 and n("many_centers_300") == 280 and (n("many_centers_max"), n("many_centers_max", 1)) == (1023, 1000)
    assert n("threshold") == 2 and [5, 5] not in res["threshold"][0]["centers"].tolist()
    for k in ("off_tile_37x53", "off_tile_65x97"):                       # image 1: no centre, things void, stuff kept
        r, sem = res[k][1], cases[k]["semantic"][1]
        assert n(k, 1) == 0 and np.all(r["instance"][np.isin(sem, (11, 12, 13))] == 255)
        assert set(np.unique(r["instance"])) == {0, 1, 8, 255}
    plateau = {(y, x) for y in range(23, 26) for x in range(40, 43)}
    for k in ("positions", "positions_nms7"):
        assert plateau <= {tuple(p) for p in res[k][0]["centers"].tolist()}
    assert np.unique(res["majority"][0]["panoptic"]).tolist() == [0, 11001, 11002, 12001, 13001, 13002, 13003]
    assert np.unique(res["stuff_area"][0]["panoptic"]).tolist() == [3000, 11001, 255000]
    eq = res["equidistant"][0]["panoptic"]
    assert eq[8, 14] == 11001 and eq[8, 3] == 11002                       # equally near centres: the lower index
    lg = res["logits"][0]["semantic"]
    assert np.all(lg[4:20, 5:30] == 3)


def test_unquantised_case_against_the_reference(golden):
    u = P.unquantised_case()
    r = P.panoptic_batch(u["semantic"], u["center"], u["offset"], **u["params"])[0]
    assert len(r["centers"]) == 150 and np.array_equal(r["centers"], golden["unquantised/0/centers"].astype(np.int64))
    near = P.near_tie_mask(r["two"])
    assert near.mean() <= 1e-3                                            # the pixels a GPU test may leave out
    differ = r["panoptic"] != golden["unquantised/0/panoptic"]
    assert not (differ & ~near).any()
    # what the capture saw: the reference's own fp32 result left the float64 restatement on no pixel of this seed
    assert int(golden["unquantised/ref_fp32_differs"]) == int(differ.sum()) == 0


# ------------------------------------------------------------------------------------------------ the plan
def _heads(N=2, C=19, H=9, W=11, labels=False, dtype=torch.uint8):
    sem = torch.zeros(N, H, W, dtype=dtype) if labels else torch.zeros(N, C, H, W)
    return sem, torch.zeros(N, 1, H, W), torch.zeros(N, 2, H, W)


def _plan(heads, **kw):
    return ops._panoptic_plan(*heads, **{**segment.CITYSCAPES, **kw})


def test_plan_accepts_logits_and_labels():
    pl = _plan(_heads())
    assert (pl.form, pl.N, pl.C, pl.H, pl.W, pl.top_k, pl.things) == ("logits", 2, 19, 9, 11, 200, tuple(range(11, 19)))
    assert _plan(_heads(labels=True)).form == "labels" and _plan(_heads(labels=True, dtype=torch.int64)).form == "labels"
    assert _plan(_heads(), top_k=ops.PANOPTIC_MAX_TOP_K, label_divisor=2000).top_k == 1024
    assert _plan(_heads(), nms_kernel=15).nms_kernel == 15 and _plan(_heads(), nms_kernel=1).nms_kernel == 1
    assert _plan(_heads(labels=True), thing_list=(254,)).things == (254,)
    assert segment.CITYSCAPES == P.CITYSCAPES


def _bad_shape(i, shape):
    h = list(_heads())
    h[i] = torch.zeros(*shape)
    return h


BAD = {
    "center_shape": lambda: (_bad_shape(1, (2, 1, 9, 12)), {}),
    "offset_channels": lambda: (_bad_shape(2, (2, 3, 9, 11)), {}),
    "batch_differs": lambda: (_bad_shape(1, (3, 1, 9, 11)), {}),
    "fp64_logits": lambda: ((torch.zeros(2, 19, 9, 11, dtype=torch.float64),) + _heads()[1:], {}),
    "int32_labels": lambda: (_heads(labels=True, dtype=torch.int32), {}),
    "fp16_center": lambda: ((_heads()[0], torch.zeros(2, 1, 9, 11, dtype=torch.float16), _heads()[2]), {}),
    "not_contiguous": lambda: ((_heads()[0], _heads()[1], torch.zeros(2, 2, 11, 9).transpose(2, 3)), {}),
    "too_many_classes": lambda: (_heads(C=257), {}),
    "even_nms": lambda: (_heads(), dict(nms_kernel=4)),
    "nms_17": lambda: (_heads(), dict(nms_kernel=17)),
    "nms_0": lambda: (_heads(), dict(nms_kernel=0)),
    "top_k_none": lambda: (_heads(), dict(top_k=None)),
    "top_k_0": lambda: (_heads(), dict(top_k=0)),
    "top_k_above_bound": lambda: (_heads(), dict(top_k=1025, label_divisor=4000)),
    "thing_outside_logits": lambda: (_heads(C=12), {}),
    "thing_255_labels": lambda: (_heads(labels=True), dict(thing_list=(255,), ignore_label=0)),
    "negative_thing": lambda: (_heads(), dict(thing_list=(-1,))),
    "divisor_not_above_top_k": lambda: (_heads(), dict(label_divisor=200)),
    "divisor_overflows": lambda: (_heads(), dict(label_divisor=2 ** 23)),
    "ignore_is_a_thing": lambda: (_heads(), dict(ignore_label=11)),
    "negative_threshold": lambda: (_heads(), dict(threshold=-0.5)),
    "nan_threshold": lambda: (_heads(), dict(threshold=float("nan"))),
    "not_a_tensor": lambda: ((None,) + _heads()[1:], {}),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_plan_refuses(case):
    heads, kw = BAD[case]()
    with pytest.raises(ValueError):
        _plan(heads, **kw)


def test_host_tensors_are_refused_on_the_launch_path():
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        segment.panoptic_maps(*_heads())
    with pytest.raises(TypeError, match="unknown parameter"):
        segment.panoptic_maps(*_heads(), topk=3)
    with pytest.raises(ValueError, match="clip"):
        segment.clip_maps(*_heads(), clip=(3, 1))
    with pytest.raises(ValueError, match="crop"):
        segment.clip_maps(*_heads(), clip=(1, 2), crop=(10, 11))


def test_entry_points_are_declared_and_bound():
    for name in ("c2m_panoptic_maps", "c2m_panoptic_workspace_bytes", "c2m_panoptic_max_top_k"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS
    assert _lib.ABI_VERSION == 6                                          # additive: no geom[] entry moved


class _OnGpu:
    """Stands for a tensor on GPU `index`: what the current-device guard reads of one."""
    is_cuda = True

    def __init__(self, index):
        self.device = type("device", (), {"index": index})()


def test_every_head_is_guarded_on_the_launch_path(monkeypatch):
    """The two device guards (ops._hip_only, ops._on_current_device) look at every operand, and panoptic_maps hands them all three
    heads: center and offset on another GPU would otherwise reach the kernel as bare addresses."""
    monkeypatch.setattr(ops, "_cur_device", lambda: 0)
    here, there, host = _OnGpu(0), _OnGpu(1), torch.zeros(1)
    ops._on_current_device(here, None, here)
    for operands in ((there, here, here), (here, there, None), (here, None, there)):
        with pytest.raises(RuntimeError, match="tensor on cuda:1 but the current device is cuda:0"):
            ops._on_current_device(*operands)
    ops._hip_only(None, "no tensor", None)
    for operands in ((host, None, None), (None, host), (None, "no tensor", host)):
        with pytest.raises(RuntimeError, match=r"^c2m_amd ops need tensors on a HIP device \(no CPU fallback by design\)$"):
            ops._hip_only(*operands)
    with pytest.raises(RuntimeError, match=r"^offset: c2m_amd ops need tensors on a HIP device \(no CPU fallback by design\)$"):
        ops._hip_only(None, host, name="offset")
    with pytest.raises(RuntimeError, match="HIP device"):
        ops._hip_only(None, required=True)

    class Reached(Exception):
        pass

    seen = {}

    def on_current_device(*ts, **kw):
        seen["current"] = ts
        raise Reached

    monkeypatch.setattr(ops, "_hip_only", lambda *ts, **kw: seen.__setitem__("hip", ts))
    monkeypatch.setattr(ops, "_on_current_device", on_current_device)
    heads = _heads()
    with pytest.raises(Reached):
        segment.panoptic_maps(*heads)
    for guard in ("hip", "current"):
        assert all(any(t is h for t in seen[guard]) for h in heads), guard
