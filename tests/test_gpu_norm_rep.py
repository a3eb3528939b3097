"""c2m_norm_fwd_rep / c2m_norm_stats_rep: train-mode BatchNorm of a batch that stands for `rep` identical copies of itself
(run with -m gpu).  Reference: float64 torch.nn.functional.batch_norm on the PHYSICALLY replicated tensor.

  * running_mean / running_var: the error against float64 is at most twice the error the existing entry (c2m_norm_fwd, rep = 1)
    shows on the replicated tensor, with a floor of 1e-6 relative (max abs error / max abs reference);
  * y, mean and invstd are those of c2m_norm_fwd on the distinct tensor, bit for bit.
Shapes (N, C, S): (2, 5, 24) the one-launch kernel, (2, 3, 6144) and (3, 2, 16384) the three launches with the one-thread finalize
(one and two chunks per plane), (16, 3, 600) the three launches with the wave finalize (N * chunks >= 16)."""
import pytest
import torch

from c2m_amd import _lib, ops
from gpu_util import rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOMENTUM = 1e-5, 0.1
SHAPES = [(2, 5, 24), (2, 3, 6144), (3, 2, 16384), (16, 3, 600)]


def _case(N, C, S):
    x = (rnd(N * 1000 + C, N, C, S) * (1.0 + rnd(7, 1, C, 1).abs()) + 3.0 * rnd(8, 1, C, 1)).to(DEV).contiguous()
    gamma, beta = (1.0 + 0.3 * rnd(1, C)).to(DEV), rnd(2, C).to(DEV)
    rm0, rv0 = rnd(3, C).to(DEV), (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(4))).to(DEV)
    return x, gamma, beta, rm0, rv0


def _run(entry, x, gamma, beta, rm0, rv0, rep=None, apply=True):
    """One call of c2m_norm_fwd (rep None), c2m_norm_fwd_rep or (apply=False) c2m_norm_stats_rep on fresh copies of the buffers."""
    L = _lib.lib()
    N, C, S = x.shape
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm, rv = rm0.clone(), rv0.clone()
    ws = torch.empty(L.c2m_norm_workspace_floats(N, C, S), device=DEV)
    y = torch.empty_like(x)
    p, rep_arg = ops._p, () if rep is None else (rep,)
    if apply:
        rc = getattr(L, entry)(p(x), p(mean), p(invstd), p(rm), p(rv), p(ws), p(gamma), p(beta), None, p(y), N, C, S, 1, EPS, MOMENTUM,
                               *rep_arg, ops.ACT["lrelu"], ops.LRELU_SLOPE, 0, ops._stream())
    else:
        rc = getattr(L, entry)(p(x), p(mean), p(invstd), p(rm), p(rv), p(ws), N, C, S, 1, EPS, MOMENTUM, *rep_arg, 0, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{entry}: hipError_t {rc}"
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv)


def _relerr(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("rep", [1, 5])
@pytest.mark.parametrize("N,C,S", SHAPES)
def test_norm_fwd_rep_vs_float64_on_the_replicated_tensor(N, C, S, rep):
    x, gamma, beta, rm0, rv0 = _case(N, C, S)
    xr = x.repeat(rep, 1, 1).contiguous()
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    torch.nn.functional.batch_norm(xr.double(), rm64, rv64, gamma.double(), beta.double(), True, MOMENTUM, EPS)
    old = _run("c2m_norm_fwd", xr, gamma, beta, rm0, rv0)                  # the existing entry on the replicated tensor
    new = _run("c2m_norm_fwd_rep", x, gamma, beta, rm0, rv0, rep)
    for k, ref in (("rm", rm64), ("rv", rv64)):
        e_old, e_new = _relerr(old[k], ref), _relerr(new[k], ref)
        print(f"({N},{C},{S}) rep {rep} {k}: error vs float64 {e_new:.2e} (existing entry on the replicated tensor {e_old:.2e})")
        assert e_new <= max(2.0 * e_old, 1e-6), f"{k}: {e_new:.3e} vs existing entry {e_old:.3e}"
    # the replication count touches nothing but the running variance
    base = _run("c2m_norm_fwd", x, gamma, beta, rm0, rv0)
    for k in ("y", "mean", "invstd", "rm"):
        assert torch.equal(new[k], base[k]), k
    assert torch.equal(new["rv"], base["rv"]) == (rep == 1)
    # the statistics-only entry (the path that also writes the channel-blocked layout uses it) updates the buffers the same way
    fused_old = _lib.lib().c2m_norm_set_fused(0)
    try:
        three = _run("c2m_norm_fwd_rep", x, gamma, beta, rm0, rv0, rep)
    finally:
        _lib.lib().c2m_norm_set_fused(fused_old)
    st = _run("c2m_norm_stats_rep", x, gamma, beta, rm0, rv0, rep, apply=False)
    for k in ("mean", "invstd", "rm", "rv"):
        assert torch.equal(st[k], three[k]), k
    for k, ref in (("rm", rm64), ("rv", rv64)):
        assert _relerr(three[k], ref) <= max(2.0 * _relerr(old[k], ref), 1e-6), k


def test_norm_rep_rejects_what_it_cannot_mean():
    x, gamma, beta, rm0, rv0 = _case(2, 5, 24)
    L = _lib.lib()
    N, C, S = x.shape
    mean, invstd, y = torch.empty(N * C, device=DEV), torch.empty(N * C, device=DEV), torch.empty_like(x)
    ws = torch.empty(L.c2m_norm_workspace_floats(N, C, S), device=DEV)
    p = ops._p
    for mode, rep in ((1, 0), (0, 5)):          # no copies at all; instance statistics have no batch to replicate
        rc = L.c2m_norm_fwd_rep(p(x), p(mean), p(invstd), p(rm0), p(rv0), p(ws), p(gamma), p(beta), None, p(y), N, C, S, mode, EPS,
                                MOMENTUM, rep, 0, ops.LRELU_SLOPE, 0, ops._stream())
        assert rc != 0
    with pytest.raises(ValueError):
        ops.batch_norm_act(x, gamma, beta, rm0.clone(), rv0.clone(), rep=0)
