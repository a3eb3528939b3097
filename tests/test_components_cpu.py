"""Connected components and instances from label maps without a GPU: the restatement (tests/components_np.py) is held to
scipy.ndimage.label where scipy is installed (the same partition, and the first-pixel rule); the cases show what they are named
for; ops._components_plan / ops._instances_plan refuse every bad input before a launch; the workspace functions and the launchers
refuse sizes out of range; the entry points are declared and bound; segment.clip_instances crops BEFORE it labels."""
import numpy as np
import pytest
import torch

import components_np as C
from c2m_amd import _lib, build, ops, segment


@pytest.fixture(scope="module")
def cases():
    return C.cases()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_scipy_label(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    rng = np.random.default_rng(5)
    for h, w, values, cell, noise in ((23, 31, 2, 1, 0.0), (40, 57, 3, 4, 0.05), (64, 64, 5, 8, 0.02), (1, 50, 2, 1, 0.0),
                                      (50, 1, 3, 1, 0.0)):
        keys = C.blobs(h, w, rng.choice(256, values, replace=False), cell, noise, int(rng.integers(1 << 30)))
        got = C.connected_components(keys, connectivity)
        # scipy labels the foreground of ONE key at a time; offset the numbers so that the union is a labelling of all pixels
        want, base = np.zeros((h, w), np.int64), 0
        for v in np.unique(keys):
            lab, n = ndimage.label(keys == v, structure=structure)
            want[keys == v] = lab[keys == v] + base
            base += n
        assert C.same_partition(got, want), (h, w, values, connectivity)
        first = {}
        for i, l in enumerate(got.reshape(-1).tolist()):
            first.setdefault(l, i)
        assert all(l == i for l, i in first.items())                   # the label IS the index of the first pixel
        assert len(first) == base


def test_same_partition_tells_partitions_apart():
    a = np.array([[0, 0, 2], [3, 3, 2]])
    assert C.same_partition(a, a * 7 + 1) and C.same_partition(a, np.array([[5, 5, 1], [9, 9, 1]]))
    assert not C.same_partition(a, np.array([[0, 0, 2], [0, 0, 2]])) and not C.same_partition(a, np.array([[0, 1, 2], [3, 3, 2]]))


def test_cases_show_what_they_are_named_for(cases):
    comps = lambda name, conn, n=0: len(np.unique(C.connected_components(cases[name]["keys"][n], conn)))
    th, tw = C.TILE_H, C.TILE_W
    assert (th, tw) == ops.COMPONENTS_TILE
    for h, w in ((1, 1), (1, 70), (70, 1), (33, 65), (37, 70), (64, 128), (97, 131), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1)):
        assert cases[f"random_{h}x{w}"]["keys"].shape == (3, h, w)
    assert comps("random_97x131", 4, 0) > 2000 and comps("random_97x131", 8, 2) < 60        # specks, and a few large blobs
    for name in ("serpentine_65x67", "serpentine_67x65_transposed"):
        k = cases[name]["keys"][0]
        lab = C.connected_components(k, 4)
        assert (k == 11).sum() == 33 * 67 + 32 and len(np.unique(lab[k == 11])) == 1 and lab[0, 0] == 0
    sp = cases["spiral_67x67"]["keys"][0]
    assert len(np.unique(C.connected_components(sp, 8)[sp == 13])) == 1 and (sp == 13).sum() > 2000
    cb = cases["combs_40x70"]["keys"][0]
    lab = C.connected_components(cb, 8)
    assert len(np.unique(lab[cb == 11])) == 1 and len(np.unique(lab[cb == 12])) == 1
    assert comps("checkerboard_40x40", 8) == 2 and comps("checkerboard_40x40", 4) == 1600
    cap = C.instances_batch(cases["checkerboard_cap_40x80"]["keys"], **cases["checkerboard_cap_40x80"]["params"])
    assert cap["count"].tolist() == [[999]] and cap["dropped"].tolist() == [[601]]
    inst = cap["instance"][0].reshape(-1)
    things = inst[cases["checkerboard_cap_40x80"]["keys"][0].reshape(-1) == 13]
    assert things[:999].tolist() == list(range(13001, 14000)) and np.all(things[999:] == 13)     # past the cap: the class
    for name in ("diagonal_main", "diagonal_anti"):
        k = cases[name]["keys"][0]
        ys, xs = np.nonzero(k == 11)
        assert sorted(ys.tolist()) == [th - 1, th] and sorted(xs.tolist()) == [tw - 1, tw]      # the corner of four tiles
        assert comps(name, 8) == 2 and comps(name, 4) == 3
    assert not C.connected_components(cases["constant_37x70"]["keys"][0], 4).any()
    ig = C.instances_batch(cases["all_ignore_33x65"]["keys"])
    assert np.all(ig["instance"] == 255) and not ig["count"].any() and not ig["dropped"].any()


def test_semantic_cases(cases):
    mix = C.instances_batch(cases["semantic_mix"]["keys"], **cases["semantic_mix"]["params"])
    inst, lab = mix["instance"][0], cases["semantic_mix"]["keys"][0]
    assert mix["count"][0].tolist() == [3, 3, 3, 0, 0, 0, 0, 0] and not mix["dropped"].any()
    assert inst[5, 5] == 11001 and inst[5, 20] == 11002 and inst[5, 15] == 255              # the ignore stripe splits the car
    assert inst[25, 6] == 12001 and inst[25, 16] == 12002 and inst[25, 12] == 7             # stuff between the riders
    assert inst[14, 41] == 13 and inst[17, 41] == 13001                                     # below / at min_area
    assert inst[27, 69] == 13002 and inst[31, 60] == inst[43, 70] == inst[31, 79] == 13003  # the enclosed bar comes first
    assert inst[35, 90] == 11003 and inst[42, 95] == 12003
    assert np.array_equal(inst[(lab != 11) & (lab != 12) & (lab != 13)], lab[(lab != 11) & (lab != 12) & (lab != 13)])
    other = C.instances_batch(cases["other_classes"]["keys"], **cases["other_classes"]["params"])
    v = other["instance"][0]
    assert other["count"].shape == (1, 3) and other["count"].min() >= 1
    assert set(np.unique(v // 256).tolist()) <= {0, 1, 3, 200} and v[15, 65] // 256 == 200
    for t, cls in enumerate((3, 200, 1)):                              # the columns follow the thing list as given
        assert len(np.unique(v[v // 256 == cls])) == other["count"][0, t]


# ------------------------------------------------------------------------------------------------ the host checks
def _sizes_only(shape, dtype):
    return torch.zeros(1, dtype=dtype).expand(shape)                    # no memory behind it


def test_components_plan():
    pl = ops._components_plan(torch.zeros(2, 5, 7, dtype=torch.uint8), 8)
    assert (pl.N, pl.H, pl.W, pl.key_bytes, pl.stride_n, pl.stride_y, pl.connectivity) == (2, 5, 7, 1, 35, 7, 8)
    view = torch.zeros(3, 9, 20, dtype=torch.int32)[:, 2:7, 4:11]       # a dense-row view
    pl = ops._components_plan(view, 4)
    assert (pl.key_bytes, pl.stride_n, pl.stride_y) == (4, 180, 20)
    assert ops._components_plan(torch.zeros(0, 5, 7, dtype=torch.uint8), 8).N == 0
    bad = [(torch.zeros(2, 5, 7), 8), (torch.zeros(2, 5, 7, dtype=torch.int64), 8), (torch.zeros(5, 7, dtype=torch.uint8), 8),
           (torch.zeros(1, 2, 5, 7, dtype=torch.uint8), 8), (torch.zeros(2, 0, 7, dtype=torch.uint8), 8),
           (torch.zeros(2, 5, 0, dtype=torch.uint8), 8), (torch.zeros(2, 5, 7, dtype=torch.uint8), 6),
           (torch.zeros(2, 5, 7, dtype=torch.uint8), True), (torch.zeros(2, 5, 7, dtype=torch.uint8), None),
           (torch.zeros(2, 7, 5, dtype=torch.uint8).transpose(1, 2), 8), (torch.zeros(2, 5, 14, dtype=torch.uint8)[:, :, ::2], 8),
           (_sizes_only((1, 1 << 16, 1 << 15), torch.uint8), 8), (_sizes_only((3, 1 << 15, 1 << 15), torch.int32), 8),
           (np.zeros((2, 5, 7), np.uint8), 8)]
    for keys, conn in bad:
        with pytest.raises(ValueError):
            ops._components_plan(keys, conn)
    with pytest.raises(ValueError, match="connectivity"):               # the checks come before the device guard
        ops.connected_components(torch.zeros(2, 5, 7, dtype=torch.uint8), connectivity=5)
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        ops.connected_components(torch.zeros(2, 5, 7, dtype=torch.uint8))


GOOD = dict(thing_list=(11, 12), label_divisor=1000, ignore_label=255, connectivity=8, min_area=1)
BAD_INSTANCES = {
    "fp32_labels": (torch.zeros(2, 5, 7), {}),
    "int32_labels": (torch.zeros(2, 5, 7, dtype=torch.int32), {}),
    "four_dims": (torch.zeros(2, 1, 5, 7, dtype=torch.uint8), {}),
    "empty_frame": (torch.zeros(2, 0, 7, dtype=torch.uint8), {}),
    "frame_too_large": (_sizes_only((1, 1 << 16, 1 << 15), torch.uint8), {}),
    "batch_too_large": (_sizes_only((3, 1 << 15, 1 << 15), torch.uint8), {}),
    "not_a_tensor": (None, {}),
    "connectivity_6": (None, dict(connectivity=6)),
    "too_many_things": (None, dict(thing_list=tuple(range(33)))),
    "thing_256": (None, dict(thing_list=(256,))),
    "negative_thing": (None, dict(thing_list=(-1,))),
    "thing_twice": (None, dict(thing_list=(11, 12, 11))),
    "thing_is_ignore": (None, dict(thing_list=(11, 255))),
    "things_not_a_list": (None, dict(thing_list=11)),
    "ignore_256": (None, dict(ignore_label=256)),
    "divisor_0": (None, dict(label_divisor=0)),
    "divisor_overflows": (None, dict(label_divisor=2 ** 23)),
    "min_area_0": (None, dict(min_area=0)),
    "min_area_text": (None, dict(min_area="large")),
}


@pytest.mark.parametrize("case", sorted(BAD_INSTANCES))
def test_instances_plan_refuses(case):
    labels, kw = BAD_INSTANCES[case]
    if labels is None and case != "not_a_tensor":
        labels = torch.zeros(2, 5, 7, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops._instances_plan(labels, **{**GOOD, **kw})


def test_instances_plan_accepts_and_the_interface_refuses():
    pl = ops._instances_plan(torch.zeros(2, 5, 7, dtype=torch.int64), **{**GOOD, "thing_list": (12, 3, 200), "connectivity": 4})
    assert (pl.N, pl.H, pl.W, pl.things, pl.connectivity, pl.min_area) == (2, 5, 7, (12, 3, 200), 4, 1)
    assert ops._instances_plan(torch.zeros(1, 5, 7, dtype=torch.uint8), **{**GOOD, "thing_list": tuple(range(32))}).things[-1] == 31
    assert ops._instances_plan(torch.zeros(1, 5, 7, dtype=torch.uint8), **{**GOOD, "thing_list": ()}).things == ()
    assert {k: segment.INSTANCE_DEFAULTS[k] for k in ("thing_list", "label_divisor", "ignore_label")} == \
        {k: segment.CITYSCAPES[k] for k in ("thing_list", "label_divisor", "ignore_label")}
    assert segment.INSTANCE_DEFAULTS == C.CITYSCAPES_INSTANCES
    labels = torch.zeros(2, 5, 7, dtype=torch.uint8)
    with pytest.raises(TypeError, match="unknown parameter"):
        segment.semantic_instances(labels, minarea=3)
    with pytest.raises(TypeError, match="unknown parameter"):
        segment.semantic_instances(labels, stuff_area=3)                # a panoptic_maps parameter, not one of these
    with pytest.raises(ValueError, match="min_area"):
        segment.semantic_instances(labels, min_area=0)
    with pytest.raises(RuntimeError, match="no CPU fallback by design"):
        segment.semantic_instances(labels)
    with pytest.raises(ValueError, match="clip"):
        segment.clip_instances(labels, clip=(3, 1))
    with pytest.raises(ValueError, match="crop"):
        segment.clip_instances(labels, clip=(1, 2), crop=(6, 7))
    with pytest.raises(ValueError, match="uint8 or int64"):
        segment.clip_instances(labels.float(), clip=(1, 2))


def test_entry_points_are_declared_bound_and_refuse_bad_sizes():
    names = ("c2m_connected_components", "c2m_components_workspace_bytes", "c2m_semantic_instances",
             "c2m_semantic_instances_workspace_bytes", "c2m_components_tile_w", "c2m_components_tile_h")
    for name in names:
        assert name in _lib.declared_symbols() and name in _lib._SIGS
    import ctypes
    V, I, L_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS["c2m_connected_components"] == (I, [V, I, L_, L_, V, V, L_, I, I, I, I, V])
    assert _lib._SIGS["c2m_semantic_instances"] == (I, [V, V, I, V, V, V, V, V, L_] + [I] * 6 + [V])
    assert _lib._SIGS["c2m_components_workspace_bytes"] == (L_, [I, I, I])
    assert _lib._SIGS["c2m_semantic_instances_workspace_bytes"] == (L_, [I, I, I, I])
    assert _lib.ABI_VERSION == 6                                        # additive: no geom[] entry moved
    assert build.SOURCES["components.hip"] == build.NOSLP               # integer kernels: no other flag
    L = _lib.lib()
    assert (L.c2m_components_tile_h(), L.c2m_components_tile_w()) == ops.COMPONENTS_TILE
    wb = L.c2m_components_workspace_bytes
    assert wb(3, 5, 7) == 3 * 35 * 4 and wb(0, 5, 7) == 0 and wb(1, 1, 1) == 4
    assert wb(1, 0, 7) == -1 and wb(1, 5, 0) == -1 and wb(-1, 5, 7) == -1
    assert wb(1, 1 << 16, 1 << 15) == -1 and wb(3, 1 << 15, 1 << 15) == -1 and wb(1, 1 << 15, (1 << 16) - 1) > 0
    sb = L.c2m_semantic_instances_workspace_bytes
    chunks = -(-97 * 131 // 1024)
    assert sb(2, 97, 131, 8) == (2 * 2 * 97 * 131 + 2 * 2 * 8 * chunks) * 4 and sb(0, 5, 7, 8) == 0
    assert sb(1, 5, 7, 33) == -1 and sb(1, 5, 7, -1) == -1 and sb(1, 0, 7, 8) == -1 and sb(1, 1 << 16, 1 << 15, 8) == -1
    assert sb(1, 5, 7, 0) > 0 and sb(1, 5, 7, 32) > 0
    # the launchers' own checks run without a device: nothing to do is success, anything out of range is an error code
    cc, si = L.c2m_connected_components, L.c2m_semantic_instances
    assert cc(None, 1, 0, 7, None, None, 0, 0, 5, 7, 8, None) == 0
    assert cc(None, 1, 0, 7, None, None, 0, 2, 5, 7, 8, None) != 0      # no pointers
    assert cc(None, 1, 0, 7, None, None, 0, 0, 5, 7, 6, None) != 0      # connectivity
    assert cc(None, 2, 0, 7, None, None, 0, 0, 5, 7, 8, None) != 0      # key size
    assert cc(None, 1, 0, 7, None, None, 0, 0, 0, 7, 8, None) != 0 and cc(None, 1, 0, -7, None, None, 0, 0, 5, 7, 8, None) != 0
    assert cc(None, 1, 0, 7, None, None, 0, 0, 1 << 16, 1 << 15, 8, None) != 0
    assert si(None, None, 8, None, None, None, None, None, 0, 0, 5, 7, 8, 1, 1000, None) == 0
    assert si(None, None, 8, None, None, None, None, None, 0, 2, 5, 7, 8, 1, 1000, None) != 0
    assert si(None, None, 33, None, None, None, None, None, 0, 0, 5, 7, 8, 1, 1000, None) != 0
    assert si(None, None, 8, None, None, None, None, None, 0, 0, 5, 7, 8, 0, 1000, None) != 0
    assert si(None, None, 8, None, None, None, None, None, 0, 0, 5, 7, 8, 1, 0, None) != 0
    assert si(None, None, 8, None, None, None, None, None, 0, 0, 5, 7, 8, 1, 1 << 23, None) != 0
    assert si(None, None, 8, None, None, None, None, None, 0, 0, 5, 7, 5, 1, 1000, None) != 0


# ------------------------------------------------------------------------------------------------ clip_instances
def test_clip_instances_crops_before_it_labels(monkeypatch):
    """Without a device: ops.semantic_instances is stood in for by the restatement.  A bar of class 13 that leaves the crop and
    comes back is ONE object of the whole frame and TWO of the visible one."""
    calls = []

    def stand_in(labels, **params):
        calls.append(tuple(labels.shape))
        assert labels.dtype == torch.uint8 and labels.is_contiguous()
        got = C.instances_batch(labels.numpy(), **params)
        return {k: torch.from_numpy(v) for k, v in got.items()}

    monkeypatch.setattr(ops, "semantic_instances", stand_in)
    B, T, H, W, h, w = 2, 3, 20, 30, 16, 24
    frame = np.zeros((H, W), np.int64)
    frame[4:6, 2:28] = 13
    frame[4:12, 26:28] = 13                                             # the bridge lies outside the crop (x >= 24)
    frame[10:12, 2:28] = 13
    labels = torch.from_numpy(np.stack([np.roll(frame, s, 0) for s in range(B * T)]))
    lab, inst = segment.clip_instances(labels, clip=(B, T), crop=(h, w))
    assert calls == [(B * T, h, w)]
    assert lab.shape == (B, T, h, w) and lab.dtype == torch.uint8 and lab.is_contiguous()
    assert inst.shape == (B, T, h, w) and inst.dtype == torch.int32 and inst.is_contiguous()
    assert torch.equal(lab.view(-1, h, w).long(), labels[:, :h, :w])
    assert sorted(np.unique(inst[0, 0].numpy()).tolist()) == [0, 13001, 13002]
    whole_lab, whole = segment.clip_instances(labels.to(torch.uint8), clip=(B, T))
    assert whole.shape == (B, T, H, W) and sorted(np.unique(whole[0, 0].numpy()).tolist()) == [0, 13001]
    assert torch.equal(whole_lab.view(-1, H, W).long(), labels)
    empty = segment.clip_instances(labels[:0], clip=(0, 3), crop=(h, w))
    assert empty[0].shape == (0, 3, h, w) and empty[1].shape == (0, 3, h, w)
