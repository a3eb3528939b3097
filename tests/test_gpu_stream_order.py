"""Stream ordering of the branch streams, made to fail every time it is wrong.

A training step runs on up to four kinds of stream: the backward's own, the weight-gradient side stream (ops.deferred_wgrads; the
per-node fork of C2M_WGRAD_STREAM), the auxiliary lanes (ops.aux_branch / ops.aux_join) and the gradient reducer's communication
stream.  A missing wait_stream / record_stream between them shows at natural timing only when the race happens to be lost.  Here
the forked stream is STRETCHED: a bounded delay (gpu_util.stretch, torch.cuda._sleep calibrated with HIP events) is enqueued in
front of every side-stream weight gradient and right after aux_branch has switched streams, so a consumer that does not wait is
certain to run first -- and finds NaN (gpu_util.poison fills and frees NaN blocks of the results' sizes in the forked stream's
allocator pool) or memory the main stream has scribbled over (gpu_util.scribble_after_conv_nodes), never the right bits of an
earlier run (every stretched run draws a fresh seed).  A lost race gives wrong numbers, nothing else: no unallocated memory is
read and every delay is at most 50 ms.

Reference of every test: the same graph with the streams OFF (deferred_wgrads(enabled=False), _AUX = "0", _WGRAD_SIDE = "0") and
no delay, compared with torch.equal -- the schemes are scheduling only.  test_reference_run_matches_float64_conv2d pins that
reference itself against F.conv2d in float64 on the CPU.

Delays: each test times its own reference run with HIP events -- the whole forward + backward + gradient reads on the main stream,
an upper bound of the segment from any fork in it to the first consumer of the forked result -- and delays by ten times that
(gpu_util.stretch_ms_for: floor 1 ms, cap 50 ms).  Measured on one MI355X (printed by every test, `pytest -s`):
    op-level convolution chains (2-3 layers, fp32 16 channels at 16 x 32; bf16 64 channels): segment 0.66 - 1.39 ms -> delay 6.6 - 13.9 ms
    auxiliary-branch graphs (two or three small GEMMs):                                     segment 0.11 - 0.84 ms -> delay 1.1 - 8.3 ms
    whole tiny step: a fixed small delay instead of the ten-fold rule (about a hundred delayed launches per step): 0.2 ms in front
    of every side-stream weight gradient and 2 ms per auxiliary block
"""
import contextlib
import copy
import itertools
import types

import pytest
import torch
import torch.nn.functional as F

from c2m_amd import ops
from c2m_amd.ddp import GradientReducer
from gpu_util import (rel_close, rnd, stretch_ms_for, poison, stretch_wgrads, stretch_aux, scribble_after_conv_nodes,
                      MAX_STRETCH_MS)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_seeds = itertools.count(41000, 100)       # a fresh seed for every stretched run of the process


def _side():
    return ops._side_stream(torch.device(DEV))


def _make(seed, layers=3, C=16, shape=(2, 16, 16, 32)):
    """Leaf tensors of a chain of `layers` 3x3 convolutions C -> C on `shape`, and the output gradient."""
    P = types.SimpleNamespace()
    P.x = rnd(seed, *shape).to(DEV).requires_grad_(True)
    P.w = [rnd(seed + 1 + 2 * i, C, C, 3, 3, scale=(1.0 / (C * 9)) ** 0.5).to(DEV).requires_grad_(True) for i in range(layers)]
    P.b = [rnd(seed + 2 + 2 * i, C, scale=0.1).to(DEV).requires_grad_(True) for i in range(layers)]
    P.go = rnd(seed + 50, *shape).to(DEV)
    P.aux = rnd(seed + 51, C, scale=0.05).to(DEV)
    P.after_backward = lambda: None
    return P


def _cv(x, w, b, act="lrelu", mode="reflect"):
    return ops.conv(x, w, b, stride=1, padding=1, padding_mode=mode, act=act)


def _chain(P, n=None):
    y = P.x
    for w, b in list(zip(P.w, P.b))[:n]:
        y = _cv(y, w, b)
    return y


def _params(P):
    return [t for pair in zip(P.w, P.b) for t in pair]


def _grads(P):
    """Read every gradient on the current stream, right away (the consumer of the forked results)."""
    out = {"x": P.x.grad}
    for i, (w, b) in enumerate(zip(P.w, P.b)):
        out[f"w{i}"], out[f"b{i}"] = w.grad, b.grad
    return {k: v.detach().clone() for k, v in out.items() if v is not None}


@contextlib.contextmanager
def _streams(monkeypatch, on, side="0"):
    with monkeypatch.context() as m:
        m.setattr(ops, "_AUX", "1" if on else "0")
        m.setattr(ops, "_WGRAD_SIDE", side if on else "0")
        m.setattr(ops, "_DEFER_WGRAD", bool(on))
        yield


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _reference(monkeypatch, scenario, make, seed, what):
    """The streams-off run (after one warm-up on another seed: plans, packs, allocator) and the delay its duration asks for."""
    with _streams(monkeypatch, False):
        scenario(make(seed - 1), False)
        P = make(seed)
        ref, seg = _timed(lambda: scenario(P, False))
    ms = stretch_ms_for(seg)
    print(f"[stream-order] {what}: main-stream segment {seg:.3f} ms -> delay {ms:.1f} ms")
    assert ms >= 10.0 * seg or ms == MAX_STRETCH_MS
    return ref, ms


def _same(ref, got, what):
    torch.cuda.synchronize()
    assert ref.keys() == got.keys(), f"{what}: {sorted(ref)} vs {sorted(got)}"
    bad = [k for k in ref if not torch.equal(ref[k], got[k])]
    assert not bad, f"{what}: differ from the streams-off run: {bad}"
    assert all(bool(torch.isfinite(v).all()) for v in ref.values()), f"{what}: the reference is not finite"


def _check_deferred(monkeypatch, scenario, what, make=_make, deferred=None, scribble=False):
    """`scenario(P, on)` builds a graph over the leaves P and runs its backward inside `with ops.deferred_wgrads(enabled=on, ...)`;
    the stretched run must give the bits of the streams-off run.  deferred: how many weight gradients must really have gone to
    the (stretched) side stream."""
    seed = next(_seeds)
    ref, ms = _reference(monkeypatch, scenario, make, seed, what)
    P = make(seed)
    with _streams(monkeypatch, True), monkeypatch.context() as m:
        st = stretch_wgrads(m, ops, ms)
        if scribble:
            sc = scribble_after_conv_nodes(m, ops)
            P.after_backward = sc.flush
        poison(_side(), *ref.values())
        got = scenario(P, True)
        _same(ref, got, what)
    if deferred is not None:
        assert st.stretched == deferred, f"{what}: {st.stretched} of {st.calls} weight gradients ran on the side stream, expected {deferred}"
    assert not ops._defer["on"] and not ops._defer["devs"] and not ops._defer["grads"] and not ops._defer["hold"]
    return st


def _backward_in_block(P, on, loss, params=None):
    with ops.deferred_wgrads(enabled=on, params=_params(P) if params is None else params):
        loss.backward()
        P.after_backward()
    return _grads(P)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_run_matches_float64_conv2d(monkeypatch):
    """The streams-off run every other test compares with, against F.conv2d in float64 on the CPU (two layers, no activation:
    the gates of test_conv_fwd_bwd)."""
    seed = next(_seeds)
    P = _make(seed, layers=2)
    with _streams(monkeypatch, False):
        y = _cv(_cv(P.x, P.w[0], P.b[0], act=None, mode="zeros"), P.w[1], P.b[1], act=None, mode="zeros")
        got = _backward_in_block(P, False, (y * P.go).sum())
    R = _make(seed, layers=2)
    x, w, b = R.x.detach().cpu().double().requires_grad_(True), [t.detach().cpu().double().requires_grad_(True) for t in R.w], \
        [t.detach().cpu().double().requires_grad_(True) for t in R.b]
    yr = F.conv2d(F.conv2d(x, w[0], b[0], padding=1), w[1], b[1], padding=1)
    go = R.go.cpu().double()
    (yr * go).sum().backward()
    rel_close(y, yr, 2e-5, "conv chain fwd")
    rel_close(got["x"], x.grad, 5e-5, "conv chain dgrad")
    for i in range(2):
        rel_close(got[f"w{i}"], w[i].grad, 1e-4, f"conv chain wgrad {i}")
    rel_close(got["b1"], b[1].grad, 1e-4, "conv chain bias grad 1", floor=1e-3 * float(go.abs().sum()) / 16)
    # (bias 0 sums the data gradient of layer 1: its rounding scale is that gradient's absolute sum)
    gh = F.conv_transpose2d(go, w[1].detach(), padding=1)
    rel_close(got["b0"], b[0].grad, 1e-4, "conv chain bias grad 0", floor=1e-3 * float(gh.abs().sum()) / 16)


# ------------------------------------------------------------------------------------------------ deferred weight gradients
def test_deferred_chain_gradients_read_right_after_the_block(monkeypatch):
    _check_deferred(monkeypatch, lambda P, on: _backward_in_block(P, on, (_chain(P) * P.go).sum()), "deferred chain", deferred=3)


def test_deferred_chain_bf16_nc8_forms(monkeypatch):
    """bf16 data path, 64 channels: the weight gradient reads the NC8 forms riding on x and dY (_record_stream_all), on the side
    stream; the main stream scribbles over everything each node lets go of."""
    def make(seed):
        return _make(seed, layers=2, C=64, shape=(2, 64, 16, 32))
    with ops.conv_precision("bf16"):
        st = _check_deferred(monkeypatch, lambda P, on: _backward_in_block(P, on, (_chain(P).float() * P.go).sum()),
                             "deferred chain bf16", make=make, deferred=2, scribble=True)
    assert st.nc8 == 2, "the case must run the NC8 weight-gradient kernel"


def test_deferred_residual_block_temporaries_freed_under_the_side_stream(monkeypatch):
    """y = conv2(conv1(h)) + h: x / dY of every node are freed by autograd while the side stream still sleeps -- and the main
    stream allocates and overwrites tensors of their sizes at once (record_stream on x, dY); AddBackward hands ONE dY to conv2 and
    to the identity path, where the engine sums conv1's data gradient into it in place unless somebody holds it (the hold queue)."""
    def scenario(P, on):
        h = _cv(P.x, P.w[0], P.b[0])
        y = _cv(_cv(h, P.w[1], P.b[1]), P.w[2], P.b[2], act=None) + h
        return _backward_in_block(P, on, (y * P.go).sum())
    _check_deferred(monkeypatch, scenario, "deferred residual block", deferred=3, scribble=True)


def test_deferred_bias_with_a_gradient_weight_without(monkeypatch):
    """Case 1: b.grad is preset (AccumulateGrad runs b.grad += gb on the backward's stream), w.grad is None."""
    def scenario(P, on):
        P.b[1].grad = P.aux.clone()
        return _backward_in_block(P, on, (_chain(P, 2) * P.go).sum())
    _check_deferred(monkeypatch, scenario, "bias has a gradient", make=lambda s: _make(s, layers=2), deferred=1)


def test_deferred_bias_shared_by_two_convolutions(monkeypatch):
    """Case 2: the engine sums the two bias gradients on the backward's stream; both weights are seen for the first time."""
    def scenario(P, on):
        P.b[1] = P.b[0]
        return _backward_in_block(P, on, (_chain(P, 2) * P.go).sum())
    _check_deferred(monkeypatch, scenario, "shared bias", make=lambda s: _make(s, layers=2), deferred=1)


def test_deferred_weight_with_a_gradient_second_backward_and_micro_batches(monkeypatch):
    """w.grad exists from the second backward on: retain_graph = True and a second micro-batch inside ONE block."""
    def scenario(P, on):
        la = (_chain(P, 2) * P.go).sum()
        P.x2 = (P.x.detach() * 0.5 + 0.25).requires_grad_(True)
        lb = (_cv(_cv(P.x2, P.w[0], P.b[0]), P.w[1], P.b[1]) * P.go).sum()
        with ops.deferred_wgrads(enabled=on, params=_params(P)):
            la.backward(retain_graph=True)
            la.backward()
            lb.backward()
        out = _grads(P)
        out["x2"] = P.x2.grad.detach().clone()
        return out
    _check_deferred(monkeypatch, scenario, "accumulation", make=lambda s: _make(s, layers=2), deferred=2)


def test_deferred_weight_applied_twice_in_one_graph(monkeypatch):
    def scenario(P, on):
        y = _cv(_cv(_cv(P.x, P.w[0], P.b[0]), P.w[1], P.b[1]), P.w[0], P.b[2])
        return _backward_in_block(P, on, (y * P.go).sum())
    _check_deferred(monkeypatch, scenario, "weight applied twice", deferred=2)


def test_deferred_non_leaf_weight(monkeypatch):
    """w = w0 / |w0| (the spectral-norm shape): DivBackward reads the weight gradient on the backward's stream."""
    def scenario(P, on):
        y = _cv(_cv(P.x, P.w[0], P.b[0]), P.w[1] / P.w[1].norm(), P.b[1])
        return _backward_in_block(P, on, (y * P.go).sum())
    _check_deferred(monkeypatch, scenario, "non-leaf weight", make=lambda s: _make(s, layers=2), deferred=1)


def test_deferred_tensor_hook_on_the_weight(monkeypatch):
    """Case 3: a gradient-clipping tensor hook reads the weight gradient inside backward."""
    def scenario(P, on):
        h = P.w[1].register_hook(lambda g: g.clamp(-0.5, 0.5))
        try:
            return _backward_in_block(P, on, (_chain(P, 2) * P.go).sum())
        finally:
            h.remove()
    _check_deferred(monkeypatch, scenario, "tensor hook", make=lambda s: _make(s, layers=2), deferred=1)


def test_deferred_post_accumulate_hook_reading_the_gradient(monkeypatch):
    """Case 3: a post-accumulate hook (not the reducer's) scales p.grad in place inside backward, on the weight and on the bias."""
    def scenario(P, on):
        def halve(p):
            p.grad.mul_(0.5)
        hs = [p.register_post_accumulate_grad_hook(halve) for p in (P.w[1], P.b[0])]
        try:
            return _backward_in_block(P, on, (_chain(P, 2) * P.go).sum())
        finally:
            for h in hs:
                h.remove()
    _check_deferred(monkeypatch, scenario, "post-accumulate hook", make=lambda s: _make(s, layers=2), deferred=0)


def test_deferred_weight_that_also_feeds_a_penalty_term(monkeypatch):
    """Case 4: loss = conv(...).sum() + w.square().sum() -- the engine sums the two gradients of w on the backward's stream, which
    the convolution node cannot see.  Deferral is opt-in per parameter: the caller lists the parameters whose
    gradients come from convolution nodes alone, and leaves this weight out."""
    def scenario(P, on):
        loss = (_chain(P, 2) * P.go).sum() + P.w[1].square().sum()
        return _backward_in_block(P, on, loss, params=[P.w[0], P.b[0], P.b[1]])
    _check_deferred(monkeypatch, scenario, "weight penalty", make=lambda s: _make(s, layers=2), deferred=1)


def test_deferred_block_without_a_parameter_list_defers_nothing(monkeypatch):
    """A direct user of ops.conv who vouched for no parameter gets the joined path, penalty term and all."""
    def scenario(P, on):
        loss = (_chain(P, 2) * P.go).sum() + P.w[1].square().sum() + P.b[0].square().sum()
        with ops.deferred_wgrads(enabled=on):
            loss.backward()
        return _grads(P)
    _check_deferred(monkeypatch, scenario, "no parameter list", make=lambda s: _make(s, layers=2), deferred=0)


def test_deferred_autograd_grad_inside_the_block(monkeypatch):
    def scenario(P, on):
        loss = (_chain(P, 2) * P.go).sum()
        with ops.deferred_wgrads(enabled=on, params=_params(P)):
            gx, gw, gb, gw1 = torch.autograd.grad(loss, [P.x, P.w[0], P.b[0], P.w[1]])
        return {k: v.detach().clone() for k, v in (("x", gx), ("w0", gw), ("b0", gb), ("w1", gw1))}
    _check_deferred(monkeypatch, scenario, "autograd.grad", make=lambda s: _make(s, layers=2), deferred=2)


class _Boom(Exception):
    pass


def test_deferred_block_joins_when_its_body_raises(monkeypatch):
    """The block's exit joins the side stream on the way out of an exception and leaves the bookkeeping clean for the next block."""
    def scenario(P, on):
        loss = (_chain(P) * P.go).sum()
        try:
            with ops.deferred_wgrads(enabled=on, params=_params(P)):
                loss.backward()
                raise _Boom()
        except _Boom:
            pass
        return _grads(P)
    _check_deferred(monkeypatch, scenario, "exception in the block", deferred=3)
    assert not ops._defer["seen"] and not ops._defer.get("by_p") and not ops._defer.get("params")
    _check_deferred(monkeypatch, lambda P, on: _backward_in_block(P, on, (_chain(P) * P.go).sum()), "block after the exception",
                    deferred=3)


# ------------------------------------------------------------------------------------------------ with the gradient reducer
class _At:
    """Stands for a new tensor that the allocator placed at a given address."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def _reducer_run(monkeypatch, P, ref_ms, in_block):
    """One step of a one-bucket reducer that adopts every parameter, no process group; `in_block(red, asked, query)` runs inside
    the block, after backward (asked: what deferred_grad_stream answered the hook, per address; query: deferred_grad_stream).
    Returns the reducer and `asked`."""
    params = _params(P)
    red = GradientReducer(params, adopt_params=params)
    assert len(red.buckets) == 1
    asked = []
    orig = ops.deferred_grad_stream

    def spy(grad):
        s = orig(grad)
        asked.append((grad.data_ptr(), s))
        return s

    with _streams(monkeypatch, True), monkeypatch.context() as m:
        m.setattr(ops, "deferred_grad_stream", spy)
        st = stretch_wgrads(m, ops, ref_ms)
        poison(_side(), *params)
        red.zero_grad()
        red.arm()
        loss = (_chain(P) * P.go).sum()
        with ops.deferred_wgrads(params=params):
            loss.backward()
            in_block(red, asked, orig)
    assert st.stretched == len(P.w), "the reducer's own hook must not switch the deferral off"
    return red, asked


def test_reducer_hook_unregisters_an_adopted_gradient(monkeypatch):
    """Case 5: once the hook has copied an adopted gradient into the bucket and dropped it, its address no longer stands for a
    gradient in flight on the side stream -- asked on the bookkeeping, whatever the allocator does with the block."""
    seed = next(_seeds)
    ref, ms = _reference(monkeypatch, lambda P, on: _backward_in_block(P, on, (_chain(P) * P.go).sum()), _make, seed, "reducer")
    P = _make(seed)
    answers = []

    def in_block(red, asked, query):            # backward is over, the block still open: a new tensor at a moved gradient's address
        answers.extend(query(_At(ptr)) for ptr, s in asked if s is not None)

    red, asked = _reducer_run(monkeypatch, P, ms, in_block)
    assert len(answers) == 2 * len(P.w), "every weight and bias gradient is moved into the bucket on the side stream"
    red.finish()
    _same(ref, _grads(P), "reducer, adopted gradients")
    assert all(a is None for a in answers), "addresses of dropped gradients are still registered as made on the side stream"
    red.remove()


def test_reducer_launch_waits_for_the_branch_streams(monkeypatch):
    """GradientReducer._launch, called while the side stream still produces the adopted gradients (inside the block: nothing but
    its own waits orders the communication stream behind ops.branch_streams): what the collective would send is the final bucket."""
    seed = next(_seeds)
    ref, ms = _reference(monkeypatch, lambda P, on: _backward_in_block(P, on, (_chain(P) * P.go).sum()), _make, seed,
                         "reducer launch")
    P = _make(seed)
    sent = []

    def in_block(red, asked, query):
        red.collectives = True                                # one process, no group: the collective is a snapshot of its input
        red._collective = lambda b: sent.append(b.flat.clone())
        red.finish()

    red, _ = _reducer_run(monkeypatch, P, ms, in_block)
    torch.cuda.synchronize()
    names = {id(p): k for k, p in [(f"w{i}", w) for i, w in enumerate(P.w)] + [(f"b{i}", b) for i, b in enumerate(P.b)]}
    want = torch.cat([ref[names[id(p)]].reshape(-1) for p in red.buckets[0].params])
    assert len(sent) == 1 and torch.equal(sent[0], want), "the bucket went out before the side stream had filled it"
    red.remove()


# ------------------------------------------------------------------------------------------------ per-node fork and join
def test_per_node_side_stream_gradients_consumed_at_once(monkeypatch):
    """C2M_WGRAD_STREAM = 1: fork and join inside every node; the weight gradients are consumed on the main stream right after
    backward, without any block."""
    def scenario(P, on):
        (_chain(P) * P.go).sum().backward()
        return _grads(P)
    seed = next(_seeds)
    ref, ms = _reference(monkeypatch, scenario, _make, seed, "per-node fork")
    P = _make(seed)
    with _streams(monkeypatch, True, side="1"), monkeypatch.context() as m:
        st = stretch_wgrads(m, ops, ms)
        poison(_side(), *ref.values())
        _same(ref, scenario(P, True), "per-node fork")
    assert st.stretched == 3


# ------------------------------------------------------------------------------------------------ auxiliary branches
def _aux_stream(monkeypatch, lane):
    if (0, lane) not in ops._aux_streams:
        with _streams(monkeypatch, True):
            with ops.aux_branch(torch.zeros(8, device=DEV), lane=lane):
                pass
            ops.aux_join()
    return ops._aux_streams[(0, lane)]


def _make_aux(seed):
    P = types.SimpleNamespace()
    P.x = rnd(seed, 64, 256).to(DEV).requires_grad_(True)
    P.A = rnd(seed + 1, 256, 256, scale=1.0 / 16).to(DEV).requires_grad_(True)
    P.B = rnd(seed + 2, 256, 256, scale=1.0 / 16).to(DEV).requires_grad_(True)
    P.go = rnd(seed + 3, 64, 256).to(DEV)
    return P


def _aux_grads(P, **more):
    out = {"x": P.x.grad, "A": P.A.grad, "B": P.B.grad}
    out.update(more)
    return {k: v.detach().clone() for k, v in out.items() if v is not None}


def _check_aux(monkeypatch, scenario, what, lanes=(0,), blocks=None):
    seed = next(_seeds)
    ref, ms = _reference(monkeypatch, scenario, _make_aux, seed, what)
    streams = [_aux_stream(monkeypatch, lane) for lane in lanes]
    P = _make_aux(seed)
    with _streams(monkeypatch, True), monkeypatch.context() as m:
        st = stretch_aux(m, ops, ms)
        for s in streams:
            poison(s, P.x, P.A, *ref.values())
        _same(ref, scenario(P, True), what)
    if blocks is not None:
        assert st.stretched == blocks, f"{what}: {st.stretched} blocks ran on an auxiliary stream, expected {blocks}"
    assert not any(ops._aux_open.values())
    return st


def test_aux_branch_result_used_after_the_join(monkeypatch):
    """Forward and backward: autograd runs the branch's backward on the auxiliary stream."""
    def scenario(P, on):
        h = P.x * 2.0
        with ops.aux_branch(h, part="roi"):
            z = torch.tanh(h @ P.A)
        m = torch.sigmoid(h @ P.B)
        ops.aux_join(z)
        out = z * m
        (out * P.go).sum().backward()
        return _aux_grads(P, out=out)
    _check_aux(monkeypatch, scenario, "aux branch", blocks=1)


def test_aux_second_block_on_the_lane_reads_the_first_blocks_result(monkeypatch):
    def scenario(P, on):
        h = P.x * 2.0
        with ops.aux_branch(h, part="roi"):
            z1 = torch.tanh(h @ P.A)
        m = torch.sigmoid(h @ P.B)
        with ops.aux_branch(z1, m, part="gnn"):
            z2 = torch.tanh(z1 @ P.B) + m
        ops.aux_join(z2)
        (z2 * P.go).sum().backward()
        return _aux_grads(P, z2=z2)
    _check_aux(monkeypatch, scenario, "two blocks on a lane", blocks=2)


def test_aux_two_lanes_joined_one_at_a_time(monkeypatch):
    state = {}

    def scenario(P, on):
        h = P.x * 2.0
        with ops.aux_branch(h, part="roi", lane=0):
            z0 = torch.tanh(h @ P.A)
        with ops.aux_branch(h, part="vgg", lane=1):
            z1 = torch.sigmoid(h @ P.B)
        ops.aux_join(z1, lanes=(1,))
        state["open"] = dict(ops._aux_open)
        u = z1 * 3.0                              # lane 1's result, lane 0 still open
        ops.aux_join(z0)
        out = u + z0
        (out * P.go).sum().backward()
        return _aux_grads(P, u=u, out=out)
    _check_aux(monkeypatch, scenario, "two lanes", lanes=(0, 1), blocks=2)
    assert state["open"][(0, 0)] is True and state["open"][(0, 1)] is False


def test_aux_branch_without_tensor_inputs_is_a_no_op(monkeypatch):
    with _streams(monkeypatch, True):
        main = torch.cuda.current_stream(torch.device(DEV))
        before = dict(ops._aux_open)
        with ops.aux_branch(None, 3, "no tensors here") as br:
            assert br.ctx is None and torch.cuda.current_stream(torch.device(DEV)) == main
        assert dict(ops._aux_open) == before


def test_aux_input_freed_and_overwritten_while_the_lane_reads_it(monkeypatch):
    """t.record_stream(aux): the input's block goes back to the main stream's pool while the (stretched) lane has not read it."""
    def scenario(P, on):
        with torch.no_grad():
            h = P.x * 2.0
            with ops.aux_branch(h, part="roi"):
                z = torch.tanh(h @ P.A)
            shape = h.shape
            del h
            junk = [torch.full(shape, 3.0e4, device=DEV) for _ in range(4)]
            del junk
            ops.aux_join(z)
            return {"z": z.clone()}
    _check_aux(monkeypatch, scenario, "aux input freed", blocks=1)


def test_aux_branches_are_off_under_the_conv_profiler(monkeypatch):
    def scenario(P, on):
        h = P.x * 2.0
        main = torch.cuda.current_stream(torch.device(DEV))
        with ops.aux_branch(h, part="roi") as br:
            assert br.ctx is None and torch.cuda.current_stream(torch.device(DEV)) == main
            z = torch.tanh(h @ P.A)
        ops.aux_join(z)
        (z * P.go).sum().backward()
        return _aux_grads(P, z=z)
    monkeypatch.setattr(ops.ConvProfiler, "active", object())
    _check_aux(monkeypatch, scenario, "aux under the profiler", blocks=0)


# ------------------------------------------------------------------------------------------------ whole steps
def _tiny_step_run(monkeypatch, on, precision, steps=2):
    from c2m_amd.modules.model import GeneratorFullModel
    from c2m_amd.synthetic import make_batch, make_step_rng, batch_to
    from c2m_amd.train import TrainStep
    from test_gpu_optim import _tiny_cfg
    cfg = _tiny_cfg()
    tp = cfg["train_params"]
    with _streams(monkeypatch, on), ops.conv_precision(precision):
        torch.manual_seed(0)
        model = GeneratorFullModel(train_params=copy.deepcopy(tp), model_params=copy.deepcopy(cfg["model_params"]),
                                   dataset="cityscapes").to(DEV).train()
        step = TrainStep(model, run_optimizers=True, distributed=False)
        totals, grads = [], None
        for it in range(steps):
            batch = batch_to(make_batch(2, 128, 256, 2, seed=60 + it), DEV)
            rng = make_step_rng(batch, z_dim=16, latent_dim=32, seed=it)
            batch["rng"] = {k: v.to(DEV) for k, v in rng.items()}
            _, lg, _ = step(batch)
            totals.append(float(lg["total_gen"].detach()))
            if it == 0:
                grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
        return totals, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whole_step_with_both_stream_kinds_stretched(precision, monkeypatch):
    """The tiny configuration of test_branch_streams_do_not_change_a_step, two steps with optimizers, every side-stream weight
    gradient and every auxiliary block delayed a little: bit-identical to the streams off."""
    t0, g0, w0 = _tiny_step_run(monkeypatch, False, precision)
    with monkeypatch.context() as m:
        sw, sa = stretch_wgrads(m, ops, 0.2), stretch_aux(m, ops, 2.0)
        t1, g1, w1 = _tiny_step_run(m, True, precision)
    assert sw.stretched > 20 and sa.stretched >= 2, (sw.stretched, sa.stretched)
    assert t0 == t1, f"losses differ: {t0} vs {t1}"
    assert g0.keys() == g1.keys()
    bad = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not bad, f"gradients differ with the stretched branch streams: {bad[:5]}"
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])]
    assert not bad, f"weights differ after 2 steps: {bad[:5]}"


DEFERRED_PER_CONFIG1_STEP = 88       # of 89 weight-gradient launches; counted by this test before the fail-safe checks, and after


def test_configs1_step_defers_as_many_weight_gradients_as_before(monkeypatch):
    """The fail-safe checks must not change the shipped step: the number of weight gradients a BASELINE configs[1] step leaves
    unjoined on the side stream, counted here, is the number counted the same way before the checks existed."""
    import bench
    from c2m_amd.modules.model import GeneratorFullModel
    from c2m_amd.synthetic import make_stream_batch, make_step_rng, batch_to
    from c2m_amd.train import TrainStep
    c = bench.CONFIGS[1]
    cfg = bench.bench_config(c["height"], c["width"], c["full_step"])
    tp = cfg["train_params"]
    with _streams(monkeypatch, True), monkeypatch.context() as m:
        st = stretch_wgrads(m, ops, 0.0)
        torch.manual_seed(0)
        model = GeneratorFullModel(train_params=copy.deepcopy(tp), model_params=copy.deepcopy(cfg["model_params"]),
                                   dataset="cityscapes").to(DEV).train()
        step = TrainStep(model, run_optimizers=c["full_step"], distributed=False)
        batch = batch_to(make_stream_batch(c["batch"], c["windows"], c["height"], c["width"], 2, seed=0), DEV)
        rng = make_step_rng(batch, z_dim=1024, latent_dim=1024, seed=0)
        batch["rng"] = {k: v.to(DEV) for k, v in rng.items()}
        step(batch)
        torch.cuda.synchronize()
    print(f"[stream-order] configs[1] step: {st.stretched} of {st.calls} weight gradients deferred")
    assert st.stretched == DEFERRED_PER_CONFIG1_STEP
