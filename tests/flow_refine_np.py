"""NumPy restatement of the variational refinement of the dense flow (csrc/flow_refine.hip) in the dtype asked for
(float64: the yardstick; float32: the kernels' own precision and association order), dense_flow with refinement on top of
tests/dense_flow_np.py, the tolerance of the GPU tests (tests/test_gpu_flow_refine.py) and their inputs.

Every expression below is written with ONE association order, the one the kernels use (compiled with -ffp-contract=off)."""
import numpy as np

import dense_flow_np as NP

ZETA2, EPS2 = 0.01, 1e-6
DEFAULTS = dict(alpha=20.0, delta=5.0, gamma=10.0, outer=5, sor=5, omega=1.6)
SOR_CAP = 5                     # the halo of fr_iterate_kernel is 2 * sor <= 10 pixels
TILE = (32, 32)                 # the tile of fr_iterate_kernel
MULTI_TILE = (40, 70)           # two tiles an axis (three along x) with a ragged remainder

# 16 x the largest difference between the float32 and the float64 run of refine() over stage_cases() (level_pair inputs with
# their random initial flows of up to 3 px, which the refinement has to smooth out: far rougher than a densified flow).
# Measured: 1.456e-3 px (the 40 x 70, N = 1 case whose motion leaves the frame, default parameters; 1.381e-3 at 21 x 37);
# tests/test_flow_refine_cpu.py recomputes the gap and asserts gap <= TOL / 16.  The factor 16 is the convention of
# dense_flow_np.TOL: it covers a different, but fixed, order of the operations.
MEASURED_GAP = 1.5e-3
TOL = 16 * MEASURED_GAP


def params(refine):
    """True or a dict of overrides -> the full parameter dict."""
    p = dict(DEFAULTS)
    if isinstance(refine, dict):
        unknown = set(refine) - set(p)
        if unknown:
            raise ValueError(f"unknown refinement parameters {sorted(unknown)}")
        p.update(refine)
    return p


# ------------------------------------------------------------------------------------------------ the algorithm
def prepare(Ia, Ib, flow, dtype=np.float64):
    """Once per level: Ia, Ib [h,w], flow [2,h,w] -> (Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz)."""
    dt = np.dtype(dtype).type
    Ia, Ib, flow = np.asarray(Ia).astype(dtype), np.asarray(Ib).astype(dtype), np.asarray(flow).astype(dtype)
    h, w = Ia.shape
    xx, yy = np.arange(w).astype(dtype)[None, :], np.arange(h).astype(dtype)[:, None]
    J = NP.sample(Ib, xx + flow[0], yy + flow[1])
    Iz = J - Ia
    Ix, Iy = NP.gradients(dt(0.5) * (J + Ia))
    Ixx, Ixy = NP.gradients(Ix)
    Iyy = NP.gradients(Iy)[1]
    Ixz, Iyz = NP.gradients(Iz)
    return Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz


def _shift(A, dy, dx):
    """A read at (y + dy, x + dx), indices clamped to the array."""
    h, w = A.shape
    return A[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


def outer_iteration(planes, u, v, du, dv, alpha=20.0, delta=5.0, gamma=10.0, sor=5, omega=1.6, origin=(0, 0)):
    """One fixed-point iteration: weights and linear system from (du, dv), then `sor` red-black sweeps -> (du, dv).  The dtype is
    that of the arrays.  origin: the level coordinates (y, x) of element [0, 0], for the colour of a pixel (a crop of a level)."""
    Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz = planes
    dt = u.dtype.type
    assert all(a.dtype == u.dtype for a in (*planes, v, du, dv))
    alpha, delta, gamma, omega, half, zeta2, eps2 = (dt(x) for x in (alpha, delta, gamma, omega, 0.5, ZETA2, EPS2))
    h, w = u.shape
    # smoothness
    U, V = u + du, v + dv
    Ux, Uy, Vx, Vy = _shift(U, 0, 1) - U, _shift(U, 1, 0) - U, _shift(V, 0, 1) - V, _shift(V, 1, 0) - V
    ws = alpha / np.sqrt((((Ux * Ux + Uy * Uy) + Vx * Vx) + Vy * Vy) + eps2)
    wR, wD, wL, wU = (np.zeros((h, w), u.dtype) for _ in range(4))
    wR[:, :-1] = half * (ws[:, :-1] + ws[:, 1:])
    wD[:-1] = half * (ws[:-1] + ws[1:])
    wL[:, 1:], wU[1:] = wR[:, :-1], wD[:-1]
    sw = ((wL + wR) + wU) + wD
    # data
    nI, nX, nY = (Ix * Ix + Iy * Iy) + zeta2, (Ixx * Ixx + Ixy * Ixy) + zeta2, (Ixy * Ixy + Iyy * Iyy) + zeta2
    r = (Iz + Ix * du) + Iy * dv
    wd = (delta / np.sqrt((r * r) / nI + eps2)) / nI
    rx, ry = (Ixz + Ixx * du) + Ixy * dv, (Iyz + Ixy * du) + Iyy * dv
    wg = gamma / np.sqrt(((rx * rx) / nX + (ry * ry) / nY) + eps2)
    wgx, wgy = wg / nX, wg / nY
    # system
    A11 = ((wd * Ix) * Ix + (wgx * Ixx) * Ixx) + (wgy * Ixy) * Ixy
    A12 = ((wd * Ix) * Iy + (wgx * Ixx) * Ixy) + (wgy * Ixy) * Iyy
    A22 = ((wd * Iy) * Iy + (wgx * Ixy) * Ixy) + (wgy * Iyy) * Iyy
    b1 = -(((wd * Iz) * Ix + (wgx * Ixz) * Ixx) + (wgy * Iyz) * Ixy)
    b2 = -(((wd * Iz) * Iy + (wgx * Ixz) * Ixy) + (wgy * Iyz) * Iyy)
    D1, D2 = A11 + sw, A22 + sw
    # red-black SOR
    om1 = dt(1) - omega
    parity = ((np.arange(h)[:, None] + origin[0]) + (np.arange(w)[None, :] + origin[1])) & 1
    du, dv = du.copy(), dv.copy()
    for _ in range(int(sor)):
        for colour in (0, 1):
            m = parity == colour
            Uc, Vc = u + du, v + dv
            su = (((wL * _shift(Uc, 0, -1) + wR * _shift(Uc, 0, 1)) + wU * _shift(Uc, -1, 0)) + wD * _shift(Uc, 1, 0)) - sw * u
            sv = (((wL * _shift(Vc, 0, -1) + wR * _shift(Vc, 0, 1)) + wU * _shift(Vc, -1, 0)) + wD * _shift(Vc, 1, 0)) - sw * v
            du = np.where(m, om1 * du + omega * (((b1 + su) - A12 * dv) / D1), du)
            dv = np.where(m, om1 * dv + omega * (((b2 + sv) - A12 * du) / D2), dv)
    return du, dv


def refine(Ia, Ib, flow, alpha=20.0, delta=5.0, gamma=10.0, outer=5, sor=5, omega=1.6, dtype=np.float64):
    """The refinement of one level: Ia, Ib [h,w], flow [2,h,w] -> flow [2,h,w]."""
    flow = np.asarray(flow).astype(dtype)
    planes = prepare(Ia, Ib, flow, dtype)
    u, v = flow[0], flow[1]
    du, dv = np.zeros_like(u), np.zeros_like(v)
    for _ in range(int(outer)):
        du, dv = outer_iteration(planes, u, v, du, dv, alpha, delta, gamma, sor, omega)
    return np.stack([u + du, v + dv])


def dense_flow(a, b, value_range=(0, 1), levels=None, finest=0, iters=12, refine_params=True, dtype=np.float64):
    """dense_flow_np.dense_flow with the refinement after the densify of every searched level (refine_params None / False: off)."""
    pa, pb = NP.pyramid(NP.gray(a, value_range, dtype), levels), NP.pyramid(NP.gray(b, value_range, dtype), levels)
    flow = None
    for l in range(len(pa) - 1, finest - 1, -1):
        h, w = pa[l].shape
        init = None if flow is None else NP.upsample(flow, h, w)
        flow = NP.densify(pa[l], pb[l], NP.patch_search(pa[l], pb[l], init, iters, dtype), dtype)
        if refine_params is not None and refine_params is not False:
            flow = refine(pa[l], pb[l], flow, dtype=dtype, **params(refine_params))
    for l in range(finest - 1, -1, -1):
        flow = NP.upsample(flow, *pa[l].shape)
    return flow


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
STAGE_SIZES = NP.STAGE_SIZES + [MULTI_TILE]


def stage_cases():
    """(h, w, n, corner, leave) of the refine_flow tests: every stage size with n in {1, 3}; the corner and the leaving motion
    alternate so that both occur at every n."""
    return [(h, w, n, bool((i + n) & 1), bool((i + (n >> 1)) & 1)) for i, (h, w) in enumerate(STAGE_SIZES) for n in (1, 3)]


def object_masks(inside, band=4):
    """(whole object, its `band`-px edge band, the object eroded by `band`)."""
    core = NP.interior(inside, band)
    return inside, inside & ~core, core
