"""The route table shared by tests/test_conv_routes_cpu.py (what each plan says) and tests/test_gpu_conv_routes.py (what is launched):
layer geometries and knob settings with the route each pass takes, written down from the if-chains the route names replaced."""
import contextlib
import itertools

from c2m_amd import ops

S1, S2, P2, P3 = (1, 1, 1), (1, 2, 2), (0, 1, 1), (1, 1, 1)
FORCE = dict(_WINO="force", _WINO_WGRAD="force", _RING="off")
# (the small maps of tests/test_gpu_nc8.py: weight gradient on the NC8 kernel below its pixel threshold, half-filled stride-2 tiles
# and padded data-gradient domains on the patch forms)
NC8T = dict(_NC8_S2_WGRAD_MIN_PIX=0, _NC8_S2_FILL_G8=2.6, _NC8_DGRAD_FILL=2.6)

# input shape, weight shape, stride, pad, reflect, bf16, dgrad_rows, knobs -> (fwd_route, dgrad_route, wgrad_route)
TABLE = [
    # fp32: Winograd F(2x2) / F(4x4), the reflect data gradient over the padded domain or as interior + ring, 3x3x3 as 2-D Winograd
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, True, False, None, FORCE, ("wino", "wino", "wino")),
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, False, False, None, dict(FORCE, _WINO4="force"), ("wino4", "wino4", "wino")),
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, True, False, None, dict(_WINO="force", _RING="force", _WINO4="off"), ("wino", "wino_ring", "igemm")),
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, True, False, None, dict(_WINO="force", _RING="force", _WINO4="force"), ("wino4", "wino4_ring", "igemm")),
    ((2, 12, 3, 16, 32), (40, 12, 3, 3, 3), S1, P3, False, False, None, FORCE, ("wino3d", "wino3d", "wino3d")),
    ((1, 16, 2, 16, 32), (16, 16, 3, 3, 3), S1, P3, True, False, None, FORCE, ("wino3d", "wino3d", "wino3d")),
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, True, False, None, dict(_WINO="off"), ("igemm", "igemm", "igemm")),
    ((2, 32, 16, 16), (64, 32, 4, 4), S2, P2, True, False, None, {}, ("igemm", "igemm_batched", "igemm")),
    ((2, 32, 17, 17), (48, 32, 4, 4), S2, P2, False, False, None, {}, ("igemm", "igemm", "igemm")),      # classes of different extents
    # fp32, the auto rules at model size (tests/test_wino4_cpu.py::test_routing_rule)
    ((40, 128, 64, 128), (128, 128, 3, 3), S1, P2, True, False, None, {}, ("wino4", "wino4_ring", "wino")),
    ((40, 128, 64, 128), (128, 128, 3, 3), S1, P2, False, False, None, {}, ("wino4", "wino4", "wino")),
    ((40, 128, 32, 64), (128, 128, 3, 3), S1, P2, True, False, None, {}, ("wino", "wino_ring", "wino")),
    ((40, 32, 128, 256), (32, 32, 3, 3), S1, P2, True, False, None, {}, ("wino", "wino", "wino")),
    ((40, 256, 16, 32), (256, 256, 3, 3), S1, P2, True, False, None, {}, ("wino", "wino", "wino")),
    ((40, 128, 64, 128), (128, 128, 3, 3), S1, P2, True, False, None, dict(_RING="off"), ("wino4", "wino", "wino")),
    ((40, 128, 64, 128), (128, 128, 3, 3), S1, P2, True, True, None, {}, ("patch_nc8", "patch_nc8", "nc8")),
    # bf16: the NC8 patch kernels (3x3, 4x4 stride 2, 3x3x3), the NC8 gather form of what they do not take, the NCHW kernels
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, False, True, None, {}, ("patch_nc8", "patch_nc8", "nc8")),
    ((2, 16, 20, 40), (32, 16, 3, 3), S1, P2, True, True, None, NC8T, ("patch_nc8", "patch_nc8", "igemm")),
    ((1, 72, 36, 96), (24, 72, 3, 3), S1, P2, False, True, None, NC8T, ("patch_nc8", "g8", "igemm")),
    ((2, 16, 32, 128), (64, 16, 4, 4), S2, P2, True, True, None, NC8T, ("s2_nc8", "s2_nc8", "s2_nc8")),
    ((3, 64, 24, 128), (32, 64, 4, 4), S2, P2, True, True, None, NC8T, ("s2_nc8", "s2_nc8", "igemm")),
    ((1, 32, 3, 16, 64), (64, 32, 3, 3, 3), S1, P3, True, True, None, NC8T, ("k333_nc8", "k333_nc8", "k333_nc8")),
    ((1, 16, 2, 8, 96), (24, 16, 3, 3, 3), S1, P3, True, True, None, NC8T, ("k333_nc8", "g8", "igemm")),
    ((1, 34, 3, 16, 64), (32, 34, 3, 3, 3), S1, P3, True, True, 32, NC8T, ("k333_nc8", "k333_nc8", "igemm")),
    ((2, 32, 16, 16), (64, 32, 4, 4), S2, P2, True, True, None, {}, ("g8", "g8", "igemm")),               # batched parity classes
    ((2, 64, 8, 16), (32, 64, 1, 1), S1, (0, 0, 0), False, True, None, {}, ("g8", "g8", "igemm")),
    ((2, 32, 17, 17), (48, 32, 4, 4), S2, P2, False, True, None, {}, ("igemm", "g8", "igemm")),            # input planes off the 8-pixel grid
    ((1, 24, 4, 8, 16), (64, 24, 4, 4, 4), (2, 2, 2), P3, True, True, None, {}, ("g8", "g8", "igemm")),
    ((2, 32, 16, 16), (64, 32, 4, 4), S2, P2, True, True, None, dict(_G8=False), ("igemm", "igemm_batched", "igemm")),
    ((2, 32, 16, 32), (64, 32, 3, 3), S1, P2, False, True, None, dict(_NC8=False), ("igemm", "igemm", "igemm")),
    ((2, 32, 15, 33), (64, 32, 3, 3), S1, P2, True, True, None, {}, ("igemm", "igemm", "igemm")),
    ((1, 32, 128, 128), (3, 32, 3, 3), S1, P2, False, True, None, {}, ("igemm", "igemm", "igemm")),        # fp32 head: thin forward
    ((1, 3, 128, 128), (32, 3, 3, 3), S1, P2, True, True, None, {}, ("igemm", "igemm", "igemm")),          # ... thin data gradient
    ((2, 48, 20, 40), (34, 48, 3, 3), S1, P2, True, True, 46, {}, ("patch_nc8", "g8", "igemm")),
]
FWD_ROUTES = {"wino3d", "wino4", "wino", "k333_nc8", "s2_nc8", "g8", "patch_nc8", "igemm"}
DGRAD_ROUTES = FWD_ROUTES | {"wino4_ring", "wino_ring", "igemm_batched"}
WGRAD_ROUTES = {"k333_nc8", "nc8", "s2_nc8", "wino3d", "wino", "igemm"}


def sweep():
    """(input shape, weight shape, stride, pad, reflect, bf16, dgrad_rows) of ~20 000 layer geometries for the default knobs: every
    route name of every pass is reached (tools/conv_plan_digest.py hashes their plans; tests/test_conv_routes_cpu.py reads them)."""
    sizes = ((8, 16), (16, 32), (32, 64), (64, 128), (128, 256), (15, 33), (120, 250))
    chans = (3, 16, 32, 34, 64, 128, 256)
    flags = list(itertools.product((False, True), repeat=2))
    k2d = (((1, 1), S1, (0, 0, 0)), ((3, 3), S1, P2), ((4, 4), S2, P2), ((7, 7), S1, (0, 3, 3)))
    for N, Cin, Cout, hw, (k, stride, pad), (reflect, bf16) in itertools.product((1, 8, 40), chans, chans, sizes, k2d, flags):
        yield (N, Cin) + hw, (Cout, Cin) + k, stride, pad, reflect, bf16, 32 if Cin == 34 else None
    k3d = (((3, 3, 3), S1, P3), ((4, 4, 4), (2, 2, 2), P3), ((1, 3, 3), S1, P2))
    for N, T, Cin, Cout, hw, (k, stride, pad), (reflect, bf16) in itertools.product((1, 8), (2, 3, 6), (16, 34, 64), (3, 32, 64), sizes[:5],
                                                                                    k3d, flags):
        yield (N, Cin, T) + hw, (Cout, Cin) + k, stride, pad, reflect, bf16, 32 if Cin == 34 else None


@contextlib.contextmanager
def knobs(settings):
    """The routing knobs are module globals read when a plan is built: set, build, restore (and drop the cached plans both times)."""
    old = {k: getattr(ops, k) for k in settings}
    for k, v in settings.items():
        setattr(ops, k, v)
    ops._geom_cache.clear()
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
        ops._geom_cache.clear()
