"""Connected components and instances from label maps on the GPU (csrc/components.hip; ops.connected_components,
segment.semantic_instances): held to the restatement (tests/components_np.py) with exact equality on every pixel and every
counter -- everything is integer, so there is no tolerance and no excluded pixel.  The serpentine, the diagonal contacts at a
corner of four tiles and the poisoned workspace are the cases a wrong seam pass or a missing zero-fill fails."""
import ctypes

import numpy as np
import pytest
import torch

import components_np as C
import gpu_util
from c2m_amd import _lib, ops, segment, tracking

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASE_NAMES = sorted(C.cases())
KEYS = ("instance", "count", "dropped", "components")


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def expected(cases):
    """The restatement's results, each computed once on first use and never changed: (name, connectivity) -> labels [N,H,W];
    name -> the outputs of semantic_instances with the case's parameters."""
    memo = {}

    def get(name, connectivity=None):
        key = (name, connectivity)
        if key not in memo:
            c = cases[name]
            memo[key] = C.instances_batch(c["keys"], **c["params"]) if connectivity is None else \
                C.components_batch(c["keys"], connectivity)
            for v in (memo[key].values() if connectivity is None else [memo[key]]):
                v.setflags(write=False)
        return memo[key]

    return get


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # a copy: the shared expectations are read-only


def differing(got, want):
    bad = np.asarray(got) != np.asarray(want)
    return int(bad.sum()), np.argwhere(bad)[:4].tolist()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_components_equal_the_restatement(name, cases, expected):
    keys = cases[name]["keys"]
    for connectivity in (4, 8):
        want = expected(name, connectivity)
        for dtype in (torch.uint8, torch.int32):
            k = dev(keys).to(dtype)
            if dtype == torch.int32:
                k = k * 16777259 - 2147483000                         # keys beyond a byte, negative ones among them
            got = ops.connected_components(k, connectivity)
            assert got.dtype == torch.int32 and got.shape == keys.shape
            assert differing(got.cpu().numpy(), want) == (0, []), (name, connectivity, dtype)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_instances_equal_the_restatement(name, cases, expected):
    c, want = cases[name], expected(name)
    for labels in (dev(c["keys"]), dev(c["keys"]).long()):
        got = segment.semantic_instances(labels, **c["params"])
        assert sorted(got) == sorted(KEYS)
        for k in KEYS:
            assert got[k].dtype == torch.int32 and got[k].shape == want[k].shape, k
            assert differing(got[k].cpu().numpy(), want[k]) == (0, []), (name, k)


def test_the_cap_leaves_the_class_on_the_pixels_past_it(cases):
    c = cases["checkerboard_cap_40x80"]
    got = segment.semantic_instances(dev(c["keys"]), **c["params"])
    assert got["count"].tolist() == [[999]] and got["dropped"].tolist() == [[601]]
    things = got["instance"][0].cpu().numpy()[c["keys"][0] == 13]
    assert things[:999].tolist() == list(range(13001, 14000)) and np.all(things[999:] == 13)
    small = cases["checkerboard_40x40"]
    got = segment.semantic_instances(dev(small["keys"]), **small["params"])
    assert got["count"].tolist() == [[800]] and got["dropped"].tolist() == [[0]]
    assert len(torch.unique(ops.connected_components(dev(small["keys"]), 8))) == 2
    assert len(torch.unique(ops.connected_components(dev(small["keys"]), 4))) == 1600


@pytest.mark.parametrize("name", ["random_97x131", "random_33x65"])
def test_batch_equals_single_calls(name, cases):
    keys = dev(cases[name]["keys"])
    assert keys.shape[0] == 3 and not torch.equal(keys[0], keys[1]) and not torch.equal(keys[1], keys[2])
    for connectivity in (4, 8):
        whole = ops.connected_components(keys, connectivity)
        maps = segment.semantic_instances(keys, connectivity=connectivity, min_area=3)
        for n in range(3):
            assert torch.equal(ops.connected_components(keys[n:n + 1], connectivity)[0], whole[n]), (n, connectivity)
            one = segment.semantic_instances(keys[n:n + 1], connectivity=connectivity, min_area=3)
            for k in KEYS:
                assert torch.equal(one[k][0], maps[k][n]), (n, connectivity, k)
    empty = segment.semantic_instances(keys[:0])
    assert empty["instance"].shape == (0, *keys.shape[1:]) and empty["count"].shape == (0, 8)
    assert ops.connected_components(keys[:0]).shape == (0, *keys.shape[1:])


def test_repeats_bit_for_bit_also_on_a_side_stream(cases):
    keys = dev(np.concatenate([cases["serpentine_65x67"]["keys"], cases["spiral_67x67"]["keys"][:, :65]]))
    first = segment.semantic_instances(keys)
    again = segment.semantic_instances(keys)
    side = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    for _ in range(8):
        big = big @ big * 1e-3                                          # the default stream is busy
    with torch.cuda.stream(side):
        third = segment.semantic_instances(keys)
        comp = ops.connected_components(keys, 8)
    side.synchronize()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], third[k]), k
    assert torch.equal(comp, first["components"])


def test_runs_in_stream_order_behind_its_producer(cases, expected):
    """On a side stream, right behind the producer of its input on that stream, with the producer held back: a host
    synchronisation or a read outside the stream's order would see the poison."""
    name = "random_64x128"
    want = expected(name)
    host = torch.from_numpy(cases[name]["keys"]).pin_memory()
    like = {k: dev(want[k]) for k in KEYS}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gpu_util.poison(side, like["instance"].float(), like["components"].float())
        gpu_util.stretch(side, 20.0)
        labels = host.to(DEV, non_blocking=True)                        # the producer: queued behind the delay
        got = segment.semantic_instances(labels)
    side.synchronize()
    for k in KEYS:
        assert torch.equal(got[k], like[k]), k


def test_a_dense_row_view_is_taken_as_it_is(cases, expected):
    name = "random_37x70"
    keys = cases[name]["keys"]
    N, H, W = keys.shape
    for dtype in (torch.uint8, torch.int32):
        frame = torch.full((N, H + 5, W + 9), 11, device=DEV, dtype=dtype)          # the surroundings carry a key of the image
        view = frame[:, 2:2 + H, 4:4 + W]
        view.copy_(dev(keys))
        assert not view.is_contiguous() and view.stride(2) == 1
        for connectivity in (4, 8):
            got = ops.connected_components(view, connectivity)
            assert got.is_contiguous() and differing(got.cpu().numpy(), expected(name, connectivity)) == (0, [])
    with pytest.raises(ValueError, match="dense rows"):
        ops.connected_components(dev(keys).transpose(1, 2), 8)


def test_a_poisoned_workspace_changes_nothing(cases, expected):
    """Nothing may rely on a zero (or anything else) that the call did not write itself."""
    L = _lib.lib()
    for name in ("serpentine_65x67", "semantic_mix", "random_97x131"):
        c = cases[name]
        labels = dev(c["keys"])
        N, H, W = labels.shape
        params = {**segment.INSTANCE_DEFAULTS, **c["params"]}
        nbytes = L.c2m_semantic_instances_workspace_bytes(N, H, W, len(params["thing_list"]))
        work = torch.full((nbytes // 4 + 3,), -1, device=DEV, dtype=torch.int32)    # 0xFF in every byte
        got = ops.semantic_instances(labels, workspace=work, **params)
        for k in KEYS:
            assert differing(got[k].cpu().numpy(), expected(name)[k]) == (0, []), (name, k)
        assert torch.all(work[nbytes // 4:] == -1)                                  # and nothing is written past its size
        nbytes = L.c2m_components_workspace_bytes(N, H, W)
        work = torch.full((nbytes // 4 + 3,), -1, device=DEV, dtype=torch.int32)
        got = ops.connected_components(labels, 4, workspace=work)
        assert differing(got.cpu().numpy(), expected(name, 4)) == (0, []) and torch.all(work[nbytes // 4:] == -1)
        with pytest.raises(ValueError, match="workspace"):
            ops.connected_components(labels, 4, workspace=work[:nbytes // 4 - 1])


def _nodes(stream):
    """The number of nodes the capture on `stream` holds so far."""
    n = ctypes.c_long(-1)
    _lib.check(_lib.lib().c2m_capture_node_count(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(n)), "capture_node_count")
    return n.value


def _captured(fn):
    """fn() captured into a graph on a side stream (a synchronisation, a copy to the host or an allocation by the runtime fails
    the capture) and replayed once.  Returns what fn returned, the graph, and the number of nodes fn added to it."""
    fn()                                                                # warm: the tables and the allocator
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        before = _nodes(side)
        out = fn()
        added = _nodes(side) - before
    g.replay()
    torch.cuda.synchronize()
    return out, g, added


def test_no_synchronisation_and_a_launch_count_independent_of_n(cases, expected):
    """The whole call is captured into a graph -- a host synchronisation, a copy to the host or a runtime allocation would fail the
    capture -- and the replay, on fresh contents of the same buffers, gives the new result.  One image and three put the same
    number of nodes on the stream: a zero-fill and eight kernels, and three kernels for the operator alone."""
    name = "random_33x65"
    keys = cases[name]["keys"]
    counts = {}
    for N in (1, 3):
        labels = torch.zeros(N, *keys.shape[1:], device=DEV, dtype=torch.uint8)
        maps, g, n_si = _captured(lambda: segment.semantic_instances(labels))
        assert not maps["count"].any()
        labels.copy_(dev(keys[:N]))
        g.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert differing(maps[k].cpu().numpy(), expected(name)[k][:N]) == (0, []), (N, k)
        comp, _, n_cc = _captured(lambda: ops.connected_components(labels, 4))
        assert differing(comp.cpu().numpy(), expected(name, 4)[:N]) == (0, [])
        counts[N] = (n_si, n_cc)
    print("graph nodes (semantic_instances, connected_components) for N = 1, 3:", counts)
    assert counts[1] == counts[3] == (9, 3)


def test_refusals_on_the_device(cases):
    keys = dev(cases["random_33x65"]["keys"])
    with pytest.raises(ValueError, match="connectivity"):
        ops.connected_components(keys, 6)
    with pytest.raises(ValueError, match="uint8 or int32"):
        ops.connected_components(keys.long())
    with pytest.raises(ValueError, match="thing_list"):
        segment.semantic_instances(keys, thing_list=(11, 11))
    with pytest.raises(TypeError, match="unknown parameter"):
        segment.semantic_instances(keys, top_k=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        segment.semantic_instances(keys.cpu())


# ------------------------------------------------------------------------------------------------ downstream
def test_clip_instances_feed_instance_boxes_and_track_instances():
    """Two frames, frame 1 = frame 0 moved up by 6 pixels.  Rectangle A of class 13 begins above rectangle B of the same class
    and to its right; moved up, both begin in row 0, so B is first in raster order there: their numbers swap.  A rectangle of
    class 11 keeps its number."""
    H, W, up = 48, 96, 6
    rects = dict(A=(13, 2, 30, 60, 80), B=(13, 4, 34, 10, 30), C=(11, 36, 44, 40, 56))      # class, y0, y1, x0, x1
    clip = np.zeros((2, H, W), np.int64)
    clip[:] = 7
    for cls, y0, y1, x0, x1 in rects.values():
        clip[0, y0:y1, x0:x1] = cls
        clip[1, max(y0 - up, 0):y1 - up, x0:x1] = cls
    labels, inst = segment.clip_instances(dev(clip), clip=(1, 2))
    assert labels.shape == (1, 2, H, W) and labels.dtype == torch.uint8 and inst.shape == (1, 2, H, W) and inst.dtype == torch.int32
    v = inst[0].cpu().numpy()
    assert v[0, 3, 61] == 13001 and v[0, 5, 11] == 13002 and v[1, 3, 61] == 13002 and v[1, 5, 11] == 13001     # swapped
    assert v[0, 37, 41] == v[1, 31, 41] == 11001 and np.all(v[clip == 7] == 7)
    box = lambda r, t: [r[3], max(r[1] - up * t, 0), r[4], r[2] - up * t]                   # x_min, y_min, x_max + 1, y_max + 1
    ids, boxes, count = ops.instance_boxes(inst, 2)
    assert int(count[0]) == 3 and ids[0, :3].tolist() == [11001, 13001, 13002]
    assert boxes[0, 0].tolist() == [box(rects["C"], 0), box(rects["C"], 1)]
    assert boxes[0, 1].tolist() == [box(rects["A"], 0), box(rects["B"], 1)]                 # an id is not an object ...
    assert boxes[0, 2].tolist() == [box(rects["B"], 0), box(rects["A"], 1)]
    flow = torch.zeros(1, 2, 1, H, W, device=DEV)
    flow[:, 1] = float(up)                                              # pixel p of frame 1 came from p + (0, up) of frame 0
    tr = tracking.track_instances(inst, 1, target_bw_of=flow)
    assert int(tr.count[0]) == 3 and tr.lost == [[]]
    assert tr.ids[0, :3].tolist() == [[11001, 11001], [13001, 13002], [13002, 13001]]       # ... the track is
    assert tr.boxes[0, 0].tolist() == [box(rects["C"], 0), box(rects["C"], 1)]
    assert tr.boxes[0, 1].tolist() == [box(rects["A"], 0), box(rects["A"], 1)]
    assert tr.boxes[0, 2].tolist() == [box(rects["B"], 0), box(rects["B"], 1)]
    # a crop is applied before the labelling: the objects are those of the visible frame
    lab_c, inst_c = segment.clip_instances(dev(clip), clip=(1, 2), crop=(40, 70))
    assert lab_c.shape == (1, 2, 40, 70) and torch.equal(lab_c, labels[:, :, :40, :70])
    assert torch.equal(inst_c[0, 0], segment.semantic_instances(dev(clip[:1, :40, :70]))["instance"][0])
