"""Float64 references, input builders and the case list for the launch-edge sweep of the one-launch GATv2 attention kernels
(csrc/gnn.hip).  test_gpu_gnn.py runs the kernels on them; test_gnn_ref_cpu.py checks the references and the input conditions
without a GPU.  Plain torch; nothing here imports c2m_amd.

Two independent derivations of the same layer (GATv2Conv(concat=False, add_self_loops=False) without the bias, on given
xl = lin_l(x), xr = lin_r(x)):
  gat_ref        all ordered pairs, the edge-multiplicity matrix A[i, j] (edges j -> i) as mask and weight of the softmax;
                 evaluated at float64 (the reference) and at float32 (the yardstick: what the formula itself loses in fp32);
  gat_ref_edges  the edge list with every edge repeated by its multiplicity, scatter_reduce / index_add over the target node, as
                 oracle/thirdparty.py::gatv2_conv does it; float64 only.

Every builder is seeded per case and returns fp32 host tensors that the device sees bit for bit; the float64 reference runs on
`.double()` of exactly those values, so no input rounding enters an error figure.

Input conditions (asserted by the CPU module for every case):
  ties    `plain` cases with N >= 2 and C >= 2 carry planted (i, j, h, c) with A[i, j] != 0 and xr[i,h,c] = -xl[j,h,c]: the sum is
          exactly 0 in fp32 and in float64.  Everywhere else an fp32 sum of two fp32 values is correctly rounded and has the sign
          of the float64 sum, so the LeakyReLU kink is never crossed between precisions; at the ties both sides take value 0 and
          derivative `slope` (torch's x > 0 ? 1 : slope, and the kernel's).
  sharp   att = 30 * N(0, 1/C): the mean row maximum of alpha is >= 0.9, exp underflows for most sources.  Not used at N <= 3,
          where alpha saturates and d xr, d att are pure cancellation (fp32 itself is 1e-2 of a near-zero maximum there).
  flat    att = 0: alpha = A / sum A, and d xr = 0.
  every judged quantity of every case has E32 <= 1e-5 * max|ref64|: the comparison never rests on an ill-conditioned figure.
Quantities that are analytically zero are `designated`: d xr where att = 0 or no row has two distinct sources, d att where no
row has two distinct sources (d logit = alpha * (d alpha - sum alpha d alpha) = 1 * (x - x)).  They get exact checks, no bound.
"""
import torch
import torch.nn.functional as F

QUANTITIES = ("out", "alpha", "dxl", "dxr", "datt")
SHARP_GAIN = 30.0
TIES = 6                    # planted per case where the case allows them
_cache = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# =============================================================================================== the two references
def gat_ref(xl, xr, att, A, gout, slope, dtype):
    """Dense form at `dtype`: (out [N,C], alpha [N,N,H], d xl, d xr [N,H,C], d att [H,C]) for the upstream gradient gout."""
    xl, xr, att = (t.detach().to(dtype).requires_grad_(True) for t in (xl, xr, att))
    A, gout = A.to(dtype), gout.to(dtype)
    e = F.leaky_relu(xl.unsqueeze(0) + xr.unsqueeze(1), slope)                 # [i, j, H, C]
    logit = (e * att).sum(-1)                                                  # [i, j, H]
    logit = logit.masked_fill(A.unsqueeze(-1) == 0, float("-inf"))
    mx = logit.max(dim=1).values
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx).detach()       # rows without edges
    ex = (logit - mx.unsqueeze(1)).exp() * A.unsqueeze(-1)
    alpha = ex / (ex.sum(1, keepdim=True) + 1e-16)
    out = torch.einsum("ijh,jhc->ihc", alpha, xl).mean(dim=1)
    out.backward(gout)
    return out.detach(), alpha.detach(), xl.grad, xr.grad, att.grad


def edge_list(A):
    """(src, dst) with edge j -> i repeated A[i, j] times."""
    nz = A.nonzero()
    rep = A[nz[:, 0], nz[:, 1]].long()
    dst, src = nz[:, 0].repeat_interleave(rep), nz[:, 1].repeat_interleave(rep)
    return src, dst


def gat_ref_edges(xl, xr, att, A, gout, slope):
    """Edge-list form in float64: the same five results, alpha as the per-edge alphas summed per (i, j) pair."""
    xl, xr, att = (t.detach().double().requires_grad_(True) for t in (xl, xr, att))
    N, H, C = xl.shape
    src, dst = edge_list(A)
    e = F.leaky_relu(xl[src] + xr[dst], slope)
    logit = (e * att).sum(-1)                                                  # [E, H]
    mx = torch.full((N, H), float("-inf"), dtype=torch.float64)
    mx = mx.scatter_reduce(0, dst[:, None].expand(-1, H), logit, reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    ex = (logit - mx[dst].detach()).exp()
    den = torch.zeros((N, H), dtype=torch.float64).index_add(0, dst, ex)
    alpha = ex / (den[dst] + 1e-16)
    out = torch.zeros((N, H, C), dtype=torch.float64).index_add(0, dst, xl[src] * alpha.unsqueeze(-1)).mean(dim=1)
    out.backward(gout.double())
    pair = torch.zeros((N, N, H), dtype=torch.float64).index_put_((dst, src), alpha.detach(), accumulate=True)
    return out.detach(), pair, xl.grad, xr.grad, att.grad


# =============================================================================================== cases and inputs
class GatCase:
    def __init__(self, N, H, C, family, graph, slope=0.2):
        self.N, self.H, self.C, self.family, self.graph, self.slope = N, H, C, family, graph, slope
        self.seed = 7000 + 131 * N + 17 * H + C + 1009 * FAMILIES.index(family) + 3001 * GRAPHS.index(graph) + int(slope * 1000)

    def __repr__(self):
        s = "" if self.slope == 0.2 else f"-slope{self.slope:g}"
        return f"N{self.N}-H{self.H}-C{self.C}-{self.family}-{self.graph}{s}"


FAMILIES = ("plain", "sharp", "flat")
GRAPHS = ("random", "empty", "dense", "single")
MODEL_SHAPE = (24, 4, 512)


def _c(N, H, C, family, graph, slope=0.2):
    return GatCase(N, H, C, family, graph, slope)


CASES = [
    # every channel-slot edge in `plain` ...
    _c(5, 2, 1, "plain", "random"), _c(13, 3, 63, "plain", "empty"), _c(24, 4, 64, "plain", "random"),
    _c(4, 5, 65, "plain", "dense"), _c(63, 2, 128, "plain", "single"), _c(13, 9, 129, "plain", "random"),
    _c(5, 8, 193, "plain", "empty"), _c(64, 4, 256, "plain", "random"), _c(24, 3, 257, "plain", "single"),
    _c(24, 4, 512, "plain", "random"), _c(13, 5, 513, "plain", "empty"), _c(64, 1, 1023, "plain", "random"),
    _c(63, 2, 1024, "plain", "dense"),
    # ... and in `sharp` (C = 1 exempt), with every N >= 4 and every H >= 2 of the table among them
    _c(13, 4, 63, "sharp", "random"), _c(5, 3, 64, "sharp", "dense"), _c(24, 2, 65, "sharp", "empty"),
    _c(4, 4, 128, "sharp", "random"), _c(63, 5, 129, "sharp", "single"), _c(24, 8, 193, "sharp", "random"),
    _c(13, 9, 256, "sharp", "empty"), _c(64, 8, 257, "sharp", "dense"), _c(24, 4, 512, "sharp", "random"),
    _c(24, 4, 513, "sharp", "single"), _c(64, 1, 1023, "sharp", "random"), _c(64, 2, 1024, "sharp", "random"),
    # `flat`
    _c(24, 4, 512, "flat", "random"), _c(1, 4, 64, "flat", "dense"), _c(2, 3, 129, "flat", "dense"),
    _c(3, 5, 257, "flat", "random"), _c(13, 9, 193, "flat", "empty"), _c(64, 2, 65, "flat", "single"),
    _c(5, 1, 1, "flat", "random"), _c(63, 8, 63, "flat", "dense"),
    # N < GAT_JB (`plain` and `flat` only) and the batch tail
    _c(1, 1, 1, "plain", "dense"), _c(1, 4, 512, "plain", "dense"), _c(1, 9, 193, "plain", "dense"),
    _c(2, 4, 512, "plain", "dense"), _c(2, 2, 63, "plain", "random"), _c(3, 8, 128, "plain", "random"),
    _c(3, 3, 1023, "plain", "single"), _c(4, 9, 257, "plain", "empty"), _c(4, 1, 64, "plain", "single"),
    # other slopes
    _c(13, 4, 96, "plain", "random", 0.0), _c(13, 4, 96, "plain", "random", 0.01),
    # the model's shape on the other graphs; the largest launches; graphs x families not met above
    _c(24, 4, 512, "plain", "empty"), _c(24, 4, 512, "sharp", "empty"), _c(24, 4, 512, "plain", "single"),
    _c(24, 4, 512, "sharp", "dense"), _c(64, 4, 512, "plain", "dense"), _c(64, 9, 193, "sharp", "random"),
    _c(63, 3, 256, "sharp", "empty"), _c(24, 5, 1024, "sharp", "empty"), _c(13, 8, 1023, "plain", "single"),
    _c(64, 3, 129, "plain", "empty"), _c(13, 2, 193, "sharp", "single"), _c(5, 9, 64, "plain", "single"),
    _c(13, 1, 257, "sharp", "random"), _c(64, 5, 63, "sharp", "single"),
]

# the table of edges every list must reach (test_gnn_ref_cpu.py asserts it), in any family and in `sharp`
EDGE_C = (1, 63, 64, 65, 128, 129, 193, 256, 257, 512, 513, 1023, 1024)
EDGE_N = (1, 2, 3, 4, 5, 13, 24, 63, 64)
EDGE_H = (1, 2, 3, 4, 5, 8, 9)
MAX_WORK = 9e6              # N * N * H * C: a float64 reference in well under a second


def empty_rows_of(case):
    return sorted({0, case.N // 2, case.N - 1}) if case.graph == "empty" else []


def graph(case, g):
    """A [N, N] fp32 edge multiplicities (edges j -> i at A[i, j]) and the planted single-source row (or None)."""
    N = case.N
    if case.graph == "dense":
        return torch.ones(N, N), None
    E = 5 * N
    dst, src = torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
    A = torch.zeros(N, N).index_put_((dst, src), torch.ones(E), accumulate=True)
    A[int(dst[0]), int(src[0])] = 5.0
    row = None
    if case.graph == "empty":
        A[empty_rows_of(case)] = 0.0
    if case.graph == "single":
        row = N // 3
        A[row] = 0.0
        A[row, (2 * N) // 3] = 3.0
    return A, row


def inputs(case):
    """(xl, xr [N,H,C], att [H,C], A [N,N], gout [N,C], ties): fp32 host tensors; ties = the planted (i, j, h, c)."""
    g = _gen(case.seed)
    N, H, C = case.N, case.H, case.C
    xl, xr = torch.randn(N, H, C, generator=g), torch.randn(N, H, C, generator=g)
    att = torch.randn(H, C, generator=g) / C ** 0.5
    gout = torch.randn(N, C, generator=g)
    A, _ = graph(case, g)
    if case.family == "sharp":
        att = att * SHARP_GAIN
    elif case.family == "flat":
        att = torch.zeros(H, C)
    ties = []
    if case.family == "plain" and N >= 2 and C >= 2:
        nz = A.nonzero().tolist()
        chans = [0, C - 1, C // 2, 63 % C, 64 % C, (C - 1) // 64 * 64]           # first / last channel, slot borders
        used = set()
        for k in range(200):
            if len(ties) == TIES or not nz:
                break
            i, j = nz[int(torch.randint(0, len(nz), (1,), generator=g))]
            h, c = k % H, chans[k % len(chans)]
            if (i, h, c) in used:
                continue
            used.add((i, h, c))
            xr[i, h, c] = -xl[j, h, c]
            ties.append((i, j, h, c))
    return xl, xr, att, A, gout, ties


def count_ties(xl, xr, A):
    """Number of (i, j, h, c) with an edge j -> i and xl[j,h,c] + xr[i,h,c] == 0 in fp32."""
    z = (xl.unsqueeze(0) + xr.unsqueeze(1)) == 0
    return int((z & (A != 0)[:, :, None, None]).sum())


def sources(A):
    """Distinct sources per target row."""
    return (A != 0).sum(1)


def designated_zero(case, A):
    """{quantity} that is analytically exactly 0 for the case (exact checks instead of a relative bound)."""
    z = set()
    if int(sources(A).max()) <= 1:
        z |= {"dxr", "datt"}
    if case.family == "flat":
        z.add("dxr")
    return z


def refs(case):
    """dict(inputs, ref64, ref32, e32 {q: max abs}, scale {q: max|ref64|}), computed once per case and shared by every test."""
    key = repr(case)
    if key not in _cache:
        xl, xr, att, A, gout, ties = inputs(case)
        r64 = gat_ref(xl, xr, att, A, gout, case.slope, torch.float64)
        r32 = gat_ref(xl, xr, att, A, gout, case.slope, torch.float32)
        e32 = {q: (b.double() - a).abs().max().item() for q, a, b in zip(QUANTITIES, r64, r32)}
        scale = {q: a.abs().max().item() for q, a in zip(QUANTITIES, r64)}
        _cache[key] = dict(inputs=(xl, xr, att, A, gout), ties=ties, ref64=dict(zip(QUANTITIES, r64)), e32=e32, scale=scale,
                           zero=designated_zero(case, A))
    return _cache[key]
