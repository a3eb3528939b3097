"""The route names of a convolution plan (ops._ConvPlan.fwd_route / dgrad_route / wgrad_route; no GPU): the literal table of
tests/conv_route_cases.py -- layer geometries and knob settings with the route each pass takes --, the operand
precision every geom array of a plan carries, and the NC8-only predicates against their former spelling over the eligibility flags
(both over the table's plans and the ~20 000 of conv_route_cases.sweep()).
tests/test_gpu_conv_routes.py runs the small cases of the same table and ties each name to what is launched."""
import itertools

import torch

from c2m_amd import ops
from conv_route_cases import DGRAD_ROUTES, FWD_ROUTES, TABLE, WGRAD_ROUTES, knobs, sweep


def _plans(with_sweep=True):
    """(plan, bf16, routes the table expects or None): the table's rows, each built and read under its knobs, then the ~20 000
    geometries of conv_route_cases.sweep() under the default knobs."""
    for xs, ws, stride, pad, reflect, bf16, rows, kn, want in TABLE:
        with knobs(kn):
            yield ops._ConvPlan(xs, ws, stride, pad, reflect, torch.device("cpu"), bf16, rows), bf16, want
    for xs, ws, stride, pad, reflect, bf16, rows in sweep() if with_sweep else ():
        yield ops._ConvPlan(xs, ws, stride, pad, reflect, torch.device("cpu"), bf16, rows), bf16, None


def test_route_table():
    seen = [set(), set(), set()]
    for pl, _, want in _plans(with_sweep=False):
        assert (pl.fwd_route, pl.dgrad_route, pl.wgrad_route) == want, (pl.dims, pl.bf16)
        for s, r in zip(seen, want):
            s.add(r)
    assert seen == [FWD_ROUTES, DGRAD_ROUTES, WGRAD_ROUTES], "every route name of every pass must appear in the table"
    assert set(ops._FWD) == FWD_ROUTES and set(ops._DGRAD) == DGRAD_ROUTES and set(ops._WGRAD) == WGRAD_ROUTES
    assert set(ops._ROUTE_PROF["conv"]) == DGRAD_ROUTES and set(ops._ROUTE_PROF["wgrad"]) == WGRAD_ROUTES


def test_every_geom_carries_the_plan_precision():
    P = ops.G.PRECISION
    for pl, bf16, _ in _plans():
        geoms = [pl.fwd_geom, pl.wg_geom] + [c["geom"] for c in pl.classes] + \
            [grp["geom"] for grp in (pl.cls_batch["groups"] if pl.cls_batch else ())]
        assert all(int(g[P]) == int(bf16) for g in geoms), pl.dims
        g8 = ([pl.g8_fwd_geom] if pl.g8_fwd else []) + [c["g8"] for c in pl.classes if "g8" in c] + \
            [grp["g8"] for grp in (pl.cls_batch["groups"] if pl.cls_batch else ()) if "g8" in grp]
        assert all(int(g[P]) == 1 for g in g8) and bool(g8) == bool(pl.g8_fwd or pl.g8_dgrad), pl.dims


def _flags_bwd_reads_only_nc8(pl, need_x, need_w):
    """ops._bwd_reads_only_nc8 as it was spelled over the eligibility flags."""
    if not (pl.bf16 and ops._NC8 and ops._NC8_GRAD and (pl.dims[6] * pl.dims[7] * pl.dims[8]) % 8 == 0):
        return False
    if need_x:
        patch_nc8 = bool(pl.classes) and all(c["patch"] for c in pl.classes) and not pl.is3d and (pl.dims[7] * pl.dims[8]) % 8 == 0
        if not (pl.k333_dgrad_nc8 or pl.s2_dgrad_nc8 or pl.g8_dgrad or patch_nc8):
            return False
    if need_w and not (pl.k333_wgrad_nc8 or pl.wgrad_nc8 or pl.s2_wgrad_nc8):
        return False
    return True


def _flags_fwd_reads_only_nc8(pl, need_w):
    """ops._fwd_reads_only_nc8 as it was spelled over the eligibility flags."""
    if not (pl.bf16 and ops._NC8 and ops._NC8_GRAD and (pl.dims[3] * pl.dims[4] * pl.dims[5]) % 8 == 0):
        return False
    if not (pl.k333_nc8 or pl.s2_nc8 or (pl.fwd_patch and pl.nc8) or pl.g8_fwd):
        return False
    if need_w and not (pl.k333_wgrad_nc8 or pl.wgrad_nc8 or pl.s2_wgrad_nc8):
        return False
    return True


def test_nc8_only_predicates_follow_the_flags():
    said_yes = 0
    for pl, bf16, _ in _plans():       # (the predicates read _NC8 / _NC8_GRAD themselves: evaluated under the plan's knobs)
        for need_x, need_w in itertools.product((False, True), repeat=2):
            got = ops._bwd_reads_only_nc8(pl, need_x, need_w)
            assert got == _flags_bwd_reads_only_nc8(pl, need_x, need_w), (pl.dims, bf16, need_x, need_w)
            said_yes += got
        for need_w in (False, True):
            got = ops._fwd_reads_only_nc8(pl, need_w)
            assert got == _flags_fwd_reads_only_nc8(pl, need_w), (pl.dims, bf16, need_w)
            said_yes += got
    assert said_yes > 20          # (the table holds layers of both kinds)
