import torch


def close(a, b, rtol=1e-5, atol=1e-6, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def rel_close(a, b, tol, what="", floor=0.0):
    """Norm-wise relative error (GEMM accumulation order differs between CPU and MFMA).  `floor` is a lower bound for
    the scale: gradients that are analytically zero (a conv bias in front of a BatchNorm) are pure rounding noise."""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), floor, 1e-30)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def rnd(seed, *shape, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale


# ---- stream stretching (test_gpu_stream_order.py): make a missing stream dependency lose its race every time -----------------
MAX_STRETCH_MS = 50.0          # one delay is a timing aid, never a hang
_sleep_rate = {}               # device index -> ("sleep", cycles per ms) | ("mm", matrices, products per ms)


def _calibrate(device):
    """Once per process and device: what one millisecond of torch.cuda._sleep (or of a chain of matrix products) is, by HIP events."""
    idx = device if isinstance(device, int) else (torch.device(device).index or 0)
    if idx in _sleep_rate:
        return _sleep_rate[idx]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.cuda.device(idx):
        torch.cuda.synchronize()
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)                                  # (first launch: module load)
            lo, hi = 1_000_000, 11_000_000
            t_lo, t_hi = timed(lambda: torch.cuda._sleep(lo)), timed(lambda: torch.cuda._sleep(hi))
            rate = ("sleep", (hi - lo) / max(t_hi - t_lo, 1e-3))     # the difference drops the launch overhead
        else:
            a = torch.ones(2048, 2048, device=f"cuda:{idx}")
            torch.mm(a, a)
            n = 32
            t = timed(lambda: [torch.mm(a, a) for _ in range(n)])
            rate = ("mm", a, n / max(t, 1e-3))
    _sleep_rate[idx] = rate
    return rate


def stretch(stream, ms):
    """Enqueue a delay of about `ms` milliseconds (at most MAX_STRETCH_MS) on `stream`: work queued behind it starts that much
    later, so a consumer on another stream that fails to wait for it is certain to run first.  Returns the delay asked for."""
    ms = min(float(ms), MAX_STRETCH_MS)
    if ms <= 0:
        return 0.0
    rate = _calibrate(stream.device)
    with torch.cuda.stream(stream):
        if rate[0] == "sleep":
            torch.cuda._sleep(int(ms * rate[1]))
        else:
            for _ in range(max(1, int(ms * rate[2]))):
                torch.mm(rate[1], rate[1])
    return ms


def stretch_ms_for(segment_ms, floor=1.0):
    """The delay for a fork whose main-stream segment (fork -> first consumer, measured with the streams off) took `segment_ms`:
    ten times the segment, at least `floor`, capped at MAX_STRETCH_MS."""
    return min(MAX_STRETCH_MS, max(10.0 * segment_ms, floor))


def poison(stream, *like):
    """Fill and free NaN tensors of the given tensors' sizes and types in `stream`'s allocator pool: a block that is read before
    its producer on that stream has run holds NaN, not the right bits of an earlier run."""
    with torch.cuda.stream(stream):
        junk = [torch.full_like(t, float("nan")) for t in like for _ in range(2)]
    del junk


class _Stretcher:
    def __init__(self, ms):
        self.ms, self.calls, self.stretched, self.nc8 = ms, 0, 0, 0
        if ms > 0:
            _calibrate(torch.cuda.current_device())      # (not from inside a backward node)


def stretch_wgrads(monkeypatch, ops, ms):
    """A delay in front of every _ConvFn._wgrad that runs on the weight-gradient side stream instead of the node's own (the
    deferred path and the per-node fork).  The returned object counts all calls (.calls) and the delayed ones (.stretched)."""
    st = _Stretcher(ms)
    orig = ops._ConvFn._wgrad

    def wgrad(ctx, pl, x, w, gy, keep=None):
        st.calls += 1
        cur = torch.cuda.current_stream(x.device)
        if any(cur == s for s in ops._side_streams.values()):
            st.stretched += 1
            st.nc8 += pl.wgrad_route in ops._NC8_WGRADS      # (NC8 operands riding on x / dY)
            stretch(cur, st.ms)
        return orig(ctx, pl, x, w, gy, keep)

    monkeypatch.setattr(ops._ConvFn, "_wgrad", staticmethod(wgrad))
    return st


def stretch_aux(monkeypatch, ops, ms):
    """A delay right after aux_branch.__enter__ has switched to the auxiliary stream (counted in .stretched)."""
    st = _Stretcher(ms)
    orig = ops.aux_branch.__enter__

    def enter(self):
        st.calls += 1
        out = orig(self)
        if self.ctx is not None:
            st.stretched += 1
            stretch(torch.cuda.current_stream(self.inputs[0].device), st.ms)
        return out

    monkeypatch.setattr(ops.aux_branch, "__enter__", enter)
    return st


class _Scribbler:
    def __init__(self):
        self.pending, self.nodes = [], 0

    def flush(self):
        """Allocate and overwrite, on the current stream, tensors of the sizes the last convolution node has just let go of."""
        junk = [torch.full(shape, 3.0e4, device=dev, dtype=dt) for (shape, dt, dev) in self.pending for _ in range(3)]
        self.pending = []
        del junk


def scribble_after_conv_nodes(monkeypatch, ops):
    """After every _ConvFn.backward node (at the start of the next one, and at .flush()) the backward's stream allocates and
    overwrites tensors of the sizes of the node's x and dY -- which autograd has freed by then.  Memory that went back to the
    allocator while another stream still reads it is handed out again here and changes that stream's result."""
    sc = _Scribbler()
    orig = ops._ConvFn.backward

    def backward(ctx, gy):
        sc.flush()
        sc.nodes += 1
        x = ctx.saved_tensors[0]
        sc.pending = [(tuple(t.shape), dt, t.device) for t in (x, gy) for dt in {t.dtype, torch.bfloat16 if ctx.pl.bf16 else t.dtype}]
        return orig(ctx, gy)

    monkeypatch.setattr(ops._ConvFn, "backward", staticmethod(backward))
    return sc
