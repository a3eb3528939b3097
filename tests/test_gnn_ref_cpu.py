"""No GPU: what makes test_gpu_gnn.py trustworthy.  gat_ref(float64) agrees with the independent edge-list derivation on every
case; every judged quantity of every case is well conditioned (the fp32 evaluation of the formula itself is within 1e-5 of the
float64 one); the inputs are what their family and graph claim; and the case list reaches every launch edge of csrc/gnn.hip
(gnn_ref.py's docstring states the conditions)."""
import pytest
import torch

import gnn_ref as R

TWO_FORMS_TOL = 1e-12          # of each tensor's maximum: two float64 derivations of one formula
CONDITION_TOL = 1e-5           # E32 / max|ref64| of every judged quantity


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_dense_reference_agrees_with_the_edge_list_form(case):
    r = R.refs(case)
    xl, xr, att, A, gout = r["inputs"]
    edges = dict(zip(R.QUANTITIES, R.gat_ref_edges(xl, xr, att, A, gout, case.slope)))
    for q in R.QUANTITIES:
        a, b = r["ref64"][q], edges[q]
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float64
        err = (a - b).abs().max().item()
        print(f"{case} {q}: two float64 forms differ by {err:.2e}, max|ref| {r['scale'][q]:.3e}")
        if q in r["zero"]:
            continue
        assert err <= TWO_FORMS_TOL * r["scale"][q], q


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_every_judged_quantity_is_well_conditioned(case):
    r = R.refs(case)
    for q in R.QUANTITIES:
        if q in r["zero"]:
            continue
        scale, e32 = r["scale"][q], r["e32"][q]
        print(f"{case} {q}: E32 {e32:.2e} = {e32 / scale:.2e} of max|ref64| {scale:.3e}")
        assert scale > 0 and e32 <= CONDITION_TOL * scale, q


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_inputs_are_what_the_case_claims(case):
    r = R.refs(case)
    xl, xr, att, A, gout = r["inputs"]
    N, H, C = case.N, case.H, case.C
    assert xl.shape == xr.shape == (N, H, C) and att.shape == (H, C) and A.shape == (N, N) and gout.shape == (N, C)
    assert all(t.dtype == torch.float32 for t in (xl, xr, att, A, gout))
    assert N * N * H * C <= R.MAX_WORK
    assert torch.equal(A, A.round()) and float(A.min()) >= 0 and A.any()
    src = R.sources(A)
    alpha = r["ref64"]["alpha"]
    # planted ties
    n_ties = R.count_ties(xl, xr, A)
    assert n_ties == len(r["ties"])
    if case.family == "plain" and N >= 2 and C >= 2:
        assert n_ties == R.TIES
        for (i, j, h, c) in r["ties"]:
            assert A[i, j] != 0 and (xl[j, h, c] + xr[i, h, c]).item() == 0.0 and xl[j, h, c].item() != 0.0
    # graphs
    if case.graph == "random":
        assert float(A.max()) >= 5
    if case.graph == "dense":
        assert bool((A == 1).all())
    if case.graph == "empty":
        rows = R.empty_rows_of(case)
        assert not A[rows].any() and (N < 5 or int((src == 0).sum()) >= 3)
    if case.graph == "single":
        row = N // 3
        assert int(src[row]) == 1 and float(A[row].max()) == 3.0
    # families
    if case.family == "sharp":
        assert N > 3, "alpha saturates at N <= 3: d xr and d att are pure cancellation there"
        rows = src >= 2
        peak = alpha.max(dim=1).values[rows].mean().item()
        print(f"{case}: mean row maximum of alpha {peak:.4f}")
        assert peak >= 0.9
    if case.family == "flat":
        assert not att.any()
        want = A.double() / A.double().sum(1, keepdim=True).clamp(min=1.0)
        assert (alpha - want.unsqueeze(-1)).abs().max().item() <= 1e-15
        assert not r["ref64"]["dxr"].any()
    # closed forms
    sums = alpha.sum(1)                                                       # [N, H]
    assert (src > 0).any() and (sums[src > 0] - 1.0).abs().max().item() <= 1e-14
    assert not alpha[src == 0].any() and not r["ref64"]["out"][src == 0].any()
    assert not alpha[(A == 0)].any()
    one = src == 1
    if one.any():                                                             # single-source rows: alpha is one-hot
        assert bool((alpha[one].max(dim=1).values == 1.0).all())
        assert r["ref64"]["dxr"][one].abs().max().item() <= 1e-12 * max(r["scale"]["dxr"], 1e-300)
    if "datt" in r["zero"]:
        assert r["ref64"]["datt"].abs().max().item() <= 1e-12 * r["scale"]["dxl"]


def test_case_list_reaches_every_launch_edge():
    assert 50 <= len(R.CASES) <= 70 and len({repr(c) for c in R.CASES}) == len(R.CASES)
    every = R.CASES
    sharp = [c for c in every if c.family == "sharp"]
    assert {c.C for c in every} >= set(R.EDGE_C) and {c.N for c in every} >= set(R.EDGE_N) and {c.H for c in every} >= set(R.EDGE_H)
    assert {c.C for c in sharp} >= set(R.EDGE_C) - {1}
    assert {c.N for c in sharp} >= {n for n in R.EDGE_N if n > 3}
    assert {c.H for c in sharp} >= set(R.EDGE_H) - {1}
    assert all(c.family != "sharp" for c in every if c.N <= 3)
    # the kernel instantiations: NS = 1, 2, 4 (ns = 3 and 4), 8, 16
    assert {min(n for n in (1, 2, 4, 8, 16) if n >= (c.C + 63) // 64) for c in every} == {1, 2, 4, 8, 16}
    assert {(c.C + 63) // 64 for c in every} >= {3, 4}
    for fam in R.FAMILIES:
        assert any((c.N, c.H, c.C) == R.MODEL_SHAPE and c.family == fam for c in every)
        assert {c.graph for c in every if c.family == fam} == set(R.GRAPHS)
    assert {c.slope for c in every if c.family == "plain"} == {0.0, 0.01, 0.2}
    assert all(c.slope == 0.2 for c in every if c.family != "plain")
    assert any((c.N, c.H, c.C) == (64, 8, 257) for c in every) and any((c.N, c.H, c.C) == (64, 1, 1023) for c in every)
    assert any(c.N == 1 for c in every) and all(c.graph == "dense" for c in every if c.N == 1)


def test_float32_yardstick_is_the_same_formula():
    case = next(c for c in R.CASES if (c.N, c.H, c.C) == R.MODEL_SHAPE and c.family == "plain" and c.graph == "random")
    xl, xr, att, A, gout = R.refs(case)["inputs"]
    r32 = R.gat_ref(xl, xr, att, A, gout, case.slope, torch.float32)
    assert all(t.dtype == torch.float32 for t in r32)
    assert [t.shape for t in r32] == [t.shape for t in R.refs(case)["ref64"].values()]
