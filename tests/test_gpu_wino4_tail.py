"""F(4x4,3x3) Winograd kernel (conv_wino4.hip) outside its K loop: the patch source offsets each lane computes in registers (reflect,
out-of-image, partial regions) and the two-pass inverse transform (32 output channels per pass, all eight waves writing, every
thread inverting one item per 32-row half) -- at the smallest shapes that reach each of their paths, against a float64 convolution
and its autograd on the CPU at the conv tests' gates (forward 2e-5, data gradient 5e-5, weight gradient 1e-4 of the tensor scale),
every launch twice with the same bits."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from c2m_amd import _lib, ops
from gpu_util import rel_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}          # float64 references, computed once per case and left unchanged


def _ref(xs, cout, mode, bias):
    """Inputs (fp32, CPU) and the float64 reference: pre-activation output, data and weight gradient for a fixed dY."""
    key = (xs, cout, mode, bias)
    if key not in _REF:
        seed = zlib.crc32(("wino4tail" + str(key)).encode()) % 10000
        x = rnd(seed, *xs)
        w = rnd(seed + 1, cout, xs[1], 3, 3, scale=(1.0 / (xs[1] * 9) ** 0.5))
        b = rnd(seed + 2, cout, scale=0.1) if bias else None
        go = rnd(seed + 3, xs[0], cout, xs[2], xs[3])
        xr, wr = (t.double().requires_grad_(True) for t in (x, w))
        xp = F.pad(xr, (1, 1, 1, 1), mode="reflect") if mode == "reflect" else F.pad(xr, (1, 1, 1, 1))
        y = F.conv2d(xp, wr, None if b is None else b.double())
        (y * go.double()).sum().backward()
        _REF[key] = (x, w, b, go, y.detach(), xr.grad, wr.grad)
    return _REF[key]


def _force(monkeypatch, ring):
    monkeypatch.setattr(ops, "_WINO", "force")
    monkeypatch.setattr(ops, "_WINO4", "force")
    monkeypatch.setattr(ops, "_RING", ring)
    monkeypatch.setattr(ops, "_RING_BUFFER", True)
    ops._geom_cache.clear()


def _fwd_bwd(xs, cout, mode, bias, ring):
    """One forward + backward through the forced F(4x4) route: (y, dX, dW) on the CPU."""
    x, w, b, go = _ref(xs, cout, mode, bias)[:4]
    xg, wg = (t.to(DEV).requires_grad_(True) for t in (x, w))
    bg = None if b is None else b.to(DEV)
    y = ops.conv(xg, wg, bg, stride=1, padding=1, padding_mode=mode)
    pl = ops._plan(xg, wg, (1, 1, 1), (0, 1, 1), mode == "reflect")
    assert pl.wino_fwd and pl.wino_dgrad and pl.wino4_fwd and pl.wino4_dgrad
    assert bool(pl.ring_dgrad) == (ring == "force")
    (y * go.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), xg.grad.cpu(), wg.grad.cpu()


def _check(xs, cout, mode, bias=True, ring="off"):
    yr, dxr, dwr = _ref(xs, cout, mode, bias)[4:]
    a, b2 = _fwd_bwd(xs, cout, mode, bias, ring), _fwd_bwd(xs, cout, mode, bias, ring)
    rel_close(a[0], yr, 2e-5, "F(4x4,3x3) fwd")
    rel_close(a[1], dxr, 5e-5, "F(4x4,3x3) dgrad")
    rel_close(a[2], dwr, 1e-4, "wgrad next to the F(4x4,3x3) launches")
    for u, v, what in zip(a, b2, ("fwd", "dgrad", "wgrad")):
        assert torch.equal(u, v), f"{what}: the same launch twice must give the same bits"
    return a


# one region and one chunk: Cout 64 = all four (wm, hf) groups live; 16 = only (0, 0); 33 = (1, 0) with ONE live row and (1, 1) dead
# (also (0, 1) full); 48 = (1, 1) dead; 80 = two M tiles, the second with 16 live rows.  The data gradients of these have M = 8 / 16.
@pytest.mark.parametrize("xs,cout", [((1, 8, 16, 32), 64), ((1, 8, 16, 32), 16), ((1, 8, 16, 32), 33), ((1, 8, 16, 32), 48),
                                     ((1, 16, 16, 32), 80)], ids=lambda v: str(v).replace(" ", ""))
def test_wino4_tail_row_groups(xs, cout, monkeypatch):
    _force(monkeypatch, "off")
    try:
        _check(xs, cout, "zeros")
    finally:
        ops._geom_cache.clear()


def test_wino4_tail_partial_regions_reflect(monkeypatch):
    """18 x 34: partial regions on both axes (2 x 2 regions of 16 x 32, the second ones with 2 live rows / columns), reflected source
    offsets at all four borders, K = 24; the data gradient runs over the padded 20 x 36 domain whose last 4-pixel group crosses Wo."""
    _force(monkeypatch, "off")
    try:
        _check((2, 24, 18, 34), 64, "reflect")
    finally:
        ops._geom_cache.clear()


def test_wino4_tail_odd_k_zero_pad(monkeypatch):
    """K = 17 (the last chunk re-reads the last channel against zero U rows) with out-of-image offsets on a 20 x 40 map (partial regions)."""
    _force(monkeypatch, "off")
    try:
        _check((1, 17, 20, 40), 64, "zeros")
    finally:
        ops._geom_cache.clear()


@pytest.mark.parametrize("ring", ["off", "force"])
@pytest.mark.parametrize("xs,cout", [((2, 64, 16, 32), 64), ((2, 40, 6, 10), 24)], ids=lambda v: str(v).replace(" ", ""))
def test_wino4_tail_reflect_dgrad(xs, cout, ring, monkeypatch):
    """Reflect data gradients: ring "off" = two-target stores over the padded domain (Y_interior + pad ring, per-pixel groups at the
    interior's edge); "force" = exact domain, the ring terms of the compact buffer added in the epilogue (rows 1 / H-2, columns 1 / W-2)."""
    _force(monkeypatch, ring)
    try:
        a = _check(xs, cout, "reflect", bias=False, ring=ring)
        dxr = _ref(xs, cout, "reflect", False)[5]
        H, W = xs[2], xs[3]
        for sl in ((slice(None), slice(None), [1, H - 2], slice(None)), (slice(None), slice(None), slice(None), [1, W - 2])):
            rel_close(a[1][sl], dxr[sl], 5e-5, "reflect dgrad, ring targets")
    finally:
        ops._geom_cache.clear()


@pytest.mark.parametrize("act", ["lrelu", "sigmoid"])
def test_wino4_tail_activation(act, monkeypatch):
    """Bias + activation inside the inverse-transform pass (80 output channels: both M tiles, a partial one)."""
    _force(monkeypatch, "off")
    try:
        xs, cout = (1, 16, 16, 32), 80
        x, w, b, _, yr = _ref(xs, cout, "zeros", True)[:5]
        ref = F.leaky_relu(yr, 0.2) if act == "lrelu" else torch.sigmoid(yr)
        with torch.no_grad():
            ya = ops.conv(x.to(DEV), w.to(DEV), b.to(DEV), stride=1, padding=1, padding_mode="zeros", act=act)
            yb = ops.conv(x.to(DEV), w.to(DEV), b.to(DEV), stride=1, padding=1, padding_mode="zeros", act=act)
        rel_close(ya, ref, 2e-5, f"F(4x4,3x3) fwd + {act}")
        assert torch.equal(ya, yb)
    finally:
        ops._geom_cache.clear()


def test_wino4_tail_strided_output_stays_inside():
    """One C-ABI launch with M = 80 into a larger NaN-filled buffer through out_sn / out_sc / out_sh / out_off: every element outside the
    [N][80][H][W] view is still NaN (no store of a dead row group, a dead M-tile row or a partial region lands anywhere), every element
    inside is finite and right."""
    L = _lib.lib()
    G = _lib.WINO_GEOM
    N, Cin, H, W, M = 2, 16, 18, 34, 80
    x, w, b, _, yr = _ref((N, Cin, H, W), M, "zeros", True)[:5]
    xg, wg, bg = (t.to(DEV).contiguous() for t in (x, w, b))
    sh, sc, sn, off = W + 5, (H + 3) * (W + 5) + 7, (M + 9) * ((H + 3) * (W + 5) + 7) + 11, 1234
    buf = torch.full((off + N * sn + 4321,), float("nan"), device=DEV)
    g = np.zeros(G.LEN, dtype=np.int64)
    for k, v in dict(M=M, K=Cin, NIMG=N, HI=H, WI=W, HO=H, WO=W, IY0=-1, IX0=-1, REFLECT=0, IN_SN=Cin * H * W, IN_SC=H * W, IN_SH=W,
                     OUT_SN=sn, OUT_SC=sc, OUT_SH=sh, OUT_OFF=off, X_BYTES=4 * N * Cin * H * W).items():
        g[getattr(G, k)] = v
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    U = torch.empty(L.c2m_wino4_upack_floats(M, Cin), device=DEV)
    assert L.c2m_wino4_filter_transform(p(wg), p(U), M, Cin, 0, st) == 0
    outs = []
    for _ in range(2):
        buf.fill_(float("nan"))
        assert L.c2m_conv_wino4(p(U), p(xg), p(buf), None, p(bg), g.ctypes.data_as(ctypes.c_void_p), 0, 0.0, st) == 0
        torch.cuda.synchronize()
        outs.append(buf.cpu())
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    inside.as_strided((N, M, H, W), (sn, sc, sh, 1), off).fill_(True)
    assert int(inside.sum()) == N * M * H * W
    got = outs[0]
    assert torch.isnan(got[~inside]).all(), f"{int((~torch.isnan(got[~inside])).sum())} elements outside the output view were written"
    assert torch.isfinite(got[inside]).all()
    rel_close(got.as_strided((N, M, H, W), (sn, sc, sh, 1), off), yr, 2e-5, "F(4x4,3x3) fwd through the C ABI")
    assert torch.equal(outs[0][inside], outs[1][inside])
