"""CPU-only checks of the rendering layer (c2m_amd.visual, csrc/render.hip): the C ABI surface, a numpy restatement of the
reference's value rules held against a fixture captured from the live reference (tools/capture_visual_golden.py), the
file writers, and argument validation.  The restatement and the numpy painters here are what tests/test_gpu_visual.py
holds the kernels to.

Number formats of the restatement: tensor2im / tensor2occ multiply a float32 array by a Python scalar, which numpy keeps in
float32 (a float64 product gives the same levels: test below); the flows are float64 throughout.  For tensor2flow that is
the reference exactly (merge() copies into a float64 sheet).  compute_flow_color_map is handed float32 frames, so in the
reference u * 3, the radius, arctan2 and the wheel position are numpy float32 and only the blend and the colour float64;
numpy's float32 arctan2 is not correctly rounded (it differs from the rounded float64 value on 38 % of a normal flow's
pixels), so no other implementation can follow its last bit.  The float64 statement used here reproduces the fixture bit
for bit and differs from the live reference on 1.9e-5 of 4 M pixels of a normal flow (sigma 5) by one level; a statement
that keeps the float32 steps but rounds a float64 arctan2 once: 6.4e-6, also one level."""
import os

import numpy as np
import pytest
import torch

from c2m_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_reference.npz")
SYMBOLS = ("c2m_render_frames", "c2m_render_flow", "c2m_render_instances", "c2m_draw_overlays")


# ------------------------------------------------------------------------------------------------ the restatement
def merge(cells, size, fill=0):
    """cells [B, ..., H, W, C] -> sheet [..., rows*H, cols*W, C]; sample b in cell (b // cols, b % cols)."""
    rows, cols = size
    B, H, W, C = cells.shape[0], cells.shape[-3], cells.shape[-2], cells.shape[-1]
    out = np.full(cells.shape[1:-3] + (rows * H, cols * W, C), fill, cells.dtype)
    for b in range(B):
        j, i = b // cols, b % cols
        out[..., j * H:(j + 1) * H, i * W:(i + 1) * W, :] = cells[b]
    return out


def levels(x, normalize=False):
    """float32 array -> uint8 levels; NaN -> 0 (numpy leaves that conversion undefined)."""
    x = np.asarray(x, np.float32)
    v = (x + 1) / 2.0 * 255.0 if normalize else x * 255.0
    assert v.dtype == np.float32
    v = np.clip(v, 0, 255)
    return np.where(np.isnan(v), 0, v).astype(np.uint8)


def np_frames(x, size, normalize=False):
    """[B,C,T,H,W] float32 -> [T, rows*H, cols*W, C] uint8."""
    return merge(levels(x, normalize).transpose(0, 2, 3, 4, 1), size)


def wheel():
    """The Middlebury colour wheel from its definition: six ramps of 15/6/4/11/13/6 entries, one channel full, one moving."""
    w = np.zeros((55, 3))
    k = 0
    for n, full, ramp, up in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True),
                              (6, 0, 2, False)):
        r = np.floor(255 * np.arange(n) / n)
        w[k:k + n, full] = 255
        w[k:k + n, ramp] = r if up else 255 - r
        k += n
    return w


def colour(u, v):
    """The colour rule in the dtype of u, v (float64, or float32 where numpy keeps it) -> uint8 [..., 3]."""
    nan = np.isnan(u) | np.isnan(v)
    u, v = np.where(nan, 0, u).astype(u.dtype), np.where(nan, 0, v).astype(u.dtype)
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * 54 + 1
    assert rad.dtype == u.dtype and fk.dtype == u.dtype
    k0 = np.floor(fk).astype(np.int64)
    k1 = np.where(k0 + 1 == 56, 1, k0 + 1)
    f = fk - k0
    assert f.dtype == np.float64
    W = wheel()
    out = np.zeros(u.shape + (3,), np.uint8)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            col = (1 - f) * (W[k0 - 1, c] / 255) + f * (W[k1 - 1, c] / 255)
            col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
            out[..., c] = np.floor(255 * col * (1 - nan)).astype(np.uint8)
    return out


def np_flow_sheet(flow, size):
    """tensor2flow: [B,2,T,H,W] float32 -> [T, rows*H, cols*W, 3]; float64, normalised per frame over the whole sheet."""
    sheet = merge(np.asarray(flow, np.float32).astype(np.float64).transpose(0, 2, 3, 4, 1), size)        # [T, RH, CW, 2]
    out = []
    for s in sheet:
        u, v = s[..., 0].copy(), s[..., 1].copy()
        unknown = (np.abs(u) > 1e7) | (np.abs(v) > 1e7)
        u[unknown] = v[unknown] = 0
        maxrad = max(-1, np.max(np.sqrt(u * u + v * v)))
        with np.errstate(invalid="ignore", divide="ignore"):
            img = colour(u / maxrad + np.finfo(float).eps, v / maxrad + np.finfo(float).eps)
        img[unknown] = 0
        out.append(img)
    return np.stack(out)


def np_flow_fixed(flow, size, scale=3.0):
    """compute_flow_color_map per cell: [B,2,T,H,W] float32 -> [T, rows*H, cols*W, 3]; empty cells hold zero flow."""
    sheet = merge(np.asarray(flow, np.float32).astype(np.float64).transpose(0, 2, 3, 4, 1), size)
    with np.errstate(over="ignore", invalid="ignore"):
        return colour(sheet[..., 0] * float(scale), sheet[..., 1] * float(scale))


def np_instances(ids, size, palette, base=None, id_range=(1000, 19000), alpha=128):
    """ids [B,1,T,H,W] -> RGB sheet: borders (id differs from a 4-neighbour in the frame) solid in the colour of the largest
    id among the pixel and its neighbours when that id is in range, else in-range ids tinted in integers."""
    ids = np.asarray(ids).astype(np.int64)[:, 0]                                       # [B,T,H,W]
    B, T, H, W = ids.shape
    lo, hi = id_range
    P = len(palette)
    pal = np.asarray(palette).astype(np.int64)
    m, edge = ids.copy(), np.zeros(ids.shape, bool)
    for a, b in ((np.s_[..., 1:], np.s_[..., :-1]), (np.s_[..., 1:, :], np.s_[..., :-1, :])):
        for p, q in ((a, b), (b, a)):
            m[p] = np.maximum(m[p], ids[q])
            edge[p] |= ids[p] != ids[q]
    out = np.zeros((T, size[0] * H, size[1] * W, 3), np.int64) if base is None else np.asarray(base).astype(np.int64)
    for b in range(B):
        j, i = b // size[1], b % size[1]
        cell = out[:, j * H:(j + 1) * H, i * W:(i + 1) * W]
        solid = edge[b] & (m[b] >= lo) & (m[b] < hi)
        tint = ~solid & (ids[b] >= lo) & (ids[b] < hi)
        cell[tint] = (cell[tint] * (256 - alpha) + pal[ids[b][tint] % P] * alpha) >> 8
        cell[solid] = pal[m[b][solid] % P]
    return out.astype(np.uint8)


def segment_pixels(a, b):
    """The pixels of the segment a -> b by the stated rule."""
    (ax, ay), (bx, by) = (int(v) for v in a), (int(v) for v in b)
    dx, dy = bx - ax, by - ay
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(ax, ay)]
    sign = lambda v: (v > 0) - (v < 0)
    if abs(dx) >= abs(dy):
        return [(ax + sign(dx) * i, ay + (2 * i * dy + n) // (2 * n)) for i in range(n + 1)]
    return [(ax + (2 * i * dx + n) // (2 * n), ay + sign(dy) * i) for i in range(n + 1)]


def np_overlays(sheet, size, boxes=None, presence=None, box_colors=None, points=None, sample=None, count=None,
                line_colors=None):
    """Painter in scatter form, primitive by primitive in the stated order, clipped to the sample's own cell."""
    out = np.array(sheet, copy=True)
    T = out.shape[0]
    H, W = out.shape[1] // size[0], out.shape[2] // size[1]

    def put(b, t, x, y, c):
        if 0 <= x < W and 0 <= y < H:
            out[t, (b // size[1]) * H + y, (b % size[1]) * W + x] = c

    nb = 0 if boxes is None else len(boxes)
    nd = 0 if points is None else len(points)
    for b in range(max([nb] + [int(s) + 1 for s in (sample if nd else [])])):
        for t in range(T):
            for n in range(boxes.shape[1] if b < nb else 0):
                if not presence[b, n, t]:
                    continue
                x0, y0, x1, y1 = (int(v) for v in boxes[b, n, t])
                x1, y1 = x1 - 1, y1 - 1
                if x1 < x0 or y1 < y0:
                    continue
                for x in range(max(x0, 0), min(x1, W - 1) + 1):
                    put(b, t, x, y0, box_colors[b, n]), put(b, t, x, y1, box_colors[b, n])
                for y in range(max(y0, 0), min(y1, H - 1) + 1):
                    put(b, t, x0, y, box_colors[b, n]), put(b, t, x1, y, box_colors[b, n])
            for d in range(nd):
                if int(sample[d]) != b:
                    continue
                c = min(int(count[d, t]), points.shape[1])
                if c <= 0:
                    continue
                for j in range(c - 1):
                    for x, y in segment_pixels(points[d, j], points[d, j + 1]):
                        put(b, t, x, y, line_colors[d])
                px, py = (int(v) for v in points[d, c - 1])
                for yy in range(py - 1, py + 2):
                    for xx in range(px - 1, px + 2):
                        put(b, t, xx, yy, line_colors[d])
    return out


# ------------------------------------------------------------------------------------------------ tests
def test_abi_declares_and_binds_the_render_symbols():
    declared = _lib.declared_symbols()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/c2m_hip.h"
        assert s in _lib._SIGS, f"{s} has no ctypes signature"
    assert _lib.ABI_VERSION == 6
    L = _lib.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.c2m_render_flow_workspace_bytes(5) == 40 and L.c2m_draw_overlays_max_boxes() == 64


def test_restatement_reproduces_the_live_reference_bit_for_bit():
    g = np.load(GOLDEN)
    size = tuple(int(v) for v in g["size"])
    assert np.array_equal(np_frames(g["frames"], size), g["im"])
    assert np.array_equal(np_frames(g["frames_pm"], size, normalize=True), g["im_normalize"])
    assert np.array_equal(np_frames(g["occ"], size)[..., 0], g["occ_sheet"])
    assert np.array_equal(np_flow_sheet(g["flow"], size), g["flow_sheet"])
    B, T = g["flow"].shape[0], g["flow"].shape[2]
    fixed = np_flow_fixed(g["flow"], (1, B))                                          # cell b = sample b
    W = g["flow"].shape[-1]
    for b in range(B):
        assert np.array_equal(fixed[:, :, b * W:(b + 1) * W], g["flow_fixed"][b]), b
    # the fixture exercises what it should: every level, both clip sides, unknown flow, radii on both sides of 1
    assert set(np.unique(g["im"])) == set(range(256)) and (g["frames"] < 0).any() and (g["frames"] > 1).any()
    assert (np.abs(g["flow"]) > 1e7).sum() == 4 and (g["flow_sheet"].reshape(-1, 3).max(1) == 0).sum() >= 4
    rad = np.sqrt((g["flow"][:, 0] * 3) ** 2 + (g["flow"][:, 1] * 3) ** 2)
    assert (rad <= 1).any() and (rad > 1).any()
    # empty cells: zero flow is near-white in the sheet mode (the added epsilon), white in the fixed-scale mode
    H = g["flow"].shape[-2]
    assert g["flow_sheet"][:, H:, W:].min() >= 254
    assert (np_flow_fixed(g["flow"], size)[:, H:, W:] == 255).all()


def test_frame_levels_in_float32_equal_the_float64_levels():
    """numpy keeps float32 for `array * 255.0`, and so does the kernel; a float64 product truncates to the same level (the
    float32 product never rounds up onto an integer the exact product is below), so either statement of the rule holds."""
    x = np.random.default_rng(0).uniform(-0.1, 1.1, 1 << 22).astype(np.float32)
    f64 = np.clip(x.astype(np.float64) * 255.0, 0, 255).astype(np.uint8)
    assert np.array_equal(levels(x), f64)


def test_all_zero_and_nan_sheets():
    z = np.zeros((2, 2, 1, 4, 8), np.float32)
    assert (np_flow_sheet(z, (1, 2)) == 0).all()                                      # 0 / 0 = NaN = black
    assert (np_flow_fixed(z, (1, 2)) == 255).all()
    z[0, 0, 0, 1, 1] = np.nan
    assert (np_flow_fixed(z, (1, 2))[0, 1, 1] == 0).all()
    assert levels(np.array([np.nan, -1, 0.5, 2], np.float32)).tolist() == [0, 0, 127, 255]


def test_segment_rule_is_symmetric_enough_to_draw_with():
    for b in [(5, 0), (5, 2), (2, 5), (0, 5), (-2, 5), (-5, 2), (-5, 0), (-5, -2), (-2, -5), (0, -5), (2, -5), (5, -2), (5, 5), (-4, 4)]:
        px = segment_pixels((10, 10), (10 + b[0], 10 + b[1]))
        assert px[0] == (10, 10) and px[-1] == (10 + b[0], 10 + b[1]) and len(px) == max(abs(b[0]), abs(b[1])) + 1
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1 for p, q in zip(px, px[1:]))       # 8-connected
    assert segment_pixels((3, 4), (3, 4)) == [(3, 4)]


def test_save_png_and_gif_round_trip(tmp_path):
    from PIL import Image
    from c2m_amd import visual
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (5, 12, 20, 3), dtype=np.uint8)
    visual.save_png(str(tmp_path / "a.png"), frames[0])
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "a.png"))), frames[0])
    visual.save_png(str(tmp_path / "g.png"), torch.from_numpy(frames[1, :, :, 0].copy()))
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "g.png"))), frames[1, :, :, 0])
    visual.save_gif(str(tmp_path / "a.gif"), frames)
    im = Image.open(str(tmp_path / "a.gif"))
    assert im.n_frames == 5 and im.size == (20, 12) and im.info["duration"] == 200          # fps = len(frames)
    visual.save_gif(str(tmp_path / "b.gif"), frames[:3, :, :, 0], fps=10)
    im = Image.open(str(tmp_path / "b.gif"))
    assert im.n_frames == 3 and im.size == (20, 12) and im.info["duration"] == 100
    with pytest.raises(ValueError, match="image"):
        visual.save_png(str(tmp_path / "x.png"), frames[0].astype(np.float32))
    with pytest.raises(ValueError, match="frames"):
        visual.save_gif(str(tmp_path / "x.gif"), frames[0, 0])


def test_argument_validation_names_the_argument():
    from c2m_amd import ops, visual
    x = torch.zeros(5, 3, 2, 8, 8)
    with pytest.raises(ValueError, match=r"x: B = 5 samples do not fit"):
        ops.render_frames(x, (2, 2))
    with pytest.raises(ValueError, match=r"x must be \[B, C, T, H, W\] with C in"):
        visual.tensor2im(torch.zeros(1, 2, 2, 8, 8))
    with pytest.raises(ValueError, match=r"flow must be \[B, C, T, H, W\] with C in \(2,\)"):
        visual.tensor2flow(x, [8, 4])
    with pytest.raises(ValueError, match="flow: B = 5"):
        visual.flow_color_map(torch.zeros(5, 2, 1, 8, 8), size=[1, 4])
    with pytest.raises(TypeError, match="ids must be torch.int32"):
        ops.render_instances(torch.zeros(1, 1, 2, 8, 8), (1, 1), torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match="x must be"):
        ops.render_frames(x.double(), (8, 4))
    for call in (lambda: visual.tensor2im(x), lambda: visual.tensor2occ(x[:, :1]), lambda: visual.tensor2flow(x[:, :2], [8, 4]),
                 lambda: visual.flow_color_map(x[:, :2])):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(RuntimeError, match="ids: .*HIP device"):
        ops.render_instances(torch.zeros(1, 1, 2, 8, 8, dtype=torch.int32), (1, 1), torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="sheet: .*HIP device"):
        ops.draw_overlays(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (1, 1))
