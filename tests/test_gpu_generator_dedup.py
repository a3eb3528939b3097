"""OcclusionAwareGenerator.forward(..., source_repeats=T): the B distinct source frames are encoded once and the features repeated
where flow and occlusion enter, instead of encoding T identical copies (run with -m gpu).

Small generator (block_expansion 8, max_expansion 64, 32x64 frames, B = 2, T = 5, train mode), both use_spade settings:
  * source_repeats=1 on the replicated frames is bit-identical to the forward this change replaced (kept below as _parent_forward);
  * source_repeats=5 on the distinct frames against source_repeats=1 on the replicated ones -- two fp32 evaluations of one function
    that differ in summation order only (batch statistics over N instead of 5N planes, the gradient of a value used five times
    summed once instead of inside every layer's reduction) -- within the gates of test_gpu_model.test_full_width_step_vs_oracle:
    output 2e-4 of its scale, gradients norm-wise 1e-2 at worst and 2e-3 in the median;
  * the BatchNorm buffers after one forward equal the replicated path's: the running variance counts the copies (rep).
Measured on MI355X (printed by the tests): DESIGN 4.9."""
import copy

import pytest
import torch

from c2m_amd import ops
from c2m_amd.config import default_config, normalize_config
from c2m_amd.modules.generator.generator import OcclusionAwareGenerator
from c2m_amd.modules.layers.common import conv_module
from gpu_util import close, rel_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, B, T = 32, 64, 2, 5
MOMENTUM = 0.1


def _generator(use_spade):
    cfg = normalize_config(default_config(height=H, width=W, block_expansion=8, max_expansion=64, use_spade=use_spade))
    mp = cfg["model_params"]
    torch.manual_seed(3)
    mod = OcclusionAwareGenerator(copy.deepcopy(mp["generator"]), copy.deepcopy(mp["flow_embedder"]), input_channel=3,
                                  dataset="cityscapes")
    return mod.to(DEV).train()


def _inputs(b=B, t=T, seed=11):
    frame = torch.rand((b, 3, H, W), generator=torch.Generator().manual_seed(seed)).to(DEV)
    flow = rnd(seed + 1, t * b, 2, H, W, scale=2.0).to(DEV)
    occ = torch.sigmoid(rnd(seed + 2, t * b, 1, H, W)).to(DEV)
    return frame, flow, occ


def _replicate(frame, t):
    return frame.unsqueeze(0).expand(t, *frame.shape).reshape(t * frame.shape[0], *frame.shape[1:]).contiguous()


def _parent_forward(self, first_frame, flow, occlusion_map):
    """The forward before source_repeats existed (cityscapes branch), on the same containers."""
    nd = self.num_down_blocks
    if self.use_spade:
        img_warp = ops.flow_warp(first_frame, flow)
        cond = self.get_cond_maps(torch.cat([img_warp, flow, occlusion_map], dim=1))
    out = self.first(first_frame)
    for blk in self.down_blocks:
        out = blk(out)
    if not self.use_spade:
        out = self.apply_optical(input_ref=out, optical_flow=flow, occlusion_map=occlusion_map)
    for blk in self.middle:
        out = blk(out)
    for i, blk in enumerate(self.up_blocks):
        if self.use_spade:
            c = cond[nd - i]
            if out.shape[-2:] != c[0].shape[-2:]:
                out = ops.resize_bilinear_grad(out, c[0].shape[-2:])
            out = ops.upsample2x(blk(out, *c))
        else:
            out = blk(out)
    if out.shape[-2:] != first_frame.shape[-2:]:
        out = ops.resize_bilinear_grad(out, first_frame.shape[-2:])
    return conv_module(out, self.final[0], act="sigmoid")


def _step(mod, frame, flow, occ, repeats):
    """One forward + backward of sum(y * fixed weights) on a private copy of the module: output, gradients, buffers."""
    mod = copy.deepcopy(mod)
    flow, occ = flow.clone().requires_grad_(True), occ.clone().requires_grad_(True)
    y = mod(frame, flow, occ, source_repeats=repeats)
    (y * rnd(5, *y.shape).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
    return dict(y=y.detach(), grads=grads, dflow=flow.grad, docc=occ.grad, bufs=dict(mod.named_buffers()), mod=mod)


_cache = {}


def _pair(use_spade):
    """(deduplicated, replicated) steps from the same weights and inputs; computed once per use_spade, never modified."""
    if use_spade not in _cache:
        mod = _generator(use_spade)
        frame, flow, occ = _inputs()
        _cache[use_spade] = (_step(mod, frame, flow, occ, T), _step(mod, _replicate(frame, T), flow, occ, 1))
    return _cache[use_spade]


@pytest.mark.parametrize("use_spade", [True, False])
def test_source_repeats_1_is_the_parent_forward(use_spade):
    mod = _generator(use_spade)
    frame, flow, occ = _inputs()
    rep = _replicate(frame, T)
    with torch.no_grad():
        want = _parent_forward(copy.deepcopy(mod), rep, flow, occ)
        got = copy.deepcopy(mod)(rep, flow, occ)
        got_kw = copy.deepcopy(mod)(rep, flow, occ, source_repeats=1)
    assert torch.equal(got, want) and torch.equal(got_kw, want)


@pytest.mark.parametrize("use_spade", [True, False])
def test_dedup_output_and_gradients_vs_replicated(use_spade):
    a, b = _pair(use_spade)
    err = (a["y"] - b["y"]).abs().max().item() / b["y"].abs().max().item()
    print(f"use_spade={use_spade}: output max abs err / scale {err:.2e}")
    rel_close(a["y"], b["y"], 2e-4, "generated")
    assert set(a["grads"]) == set(b["grads"])
    ga = dict(a["grads"], **{"<flow>": a["dflow"], "<occlusion>": a["docc"]})
    gb = dict(b["grads"], **{"<flow>": b["dflow"], "<occlusion>": b["docc"]})
    rms = sorted(gb[k].double().norm().item() / gb[k].numel() ** 0.5 for k in gb)
    noise = 1e-3 * rms[len(rms) // 2]               # analytically-zero gradients (conv biases in front of a norm) are rounding noise
    rel = []
    for k in gb:
        x, r = ga[k].double(), gb[k].double()
        e = (x - r).norm().item()
        rel.append((e / (1e-2 * r.norm().item() + noise * r.numel() ** 0.5), k, e / max(r.norm().item(), 1e-30)))
    rel.sort(reverse=True)
    real = sorted(r for _, k, r in rel if gb[k].double().norm().item() > 10 * noise * gb[k].numel() ** 0.5)
    print(f"use_spade={use_spade}: gradient relative L2 error worst {real[-1]:.2e} median {real[len(real) // 2]:.2e} "
          f"({len(real)} of {len(rel)} above the noise floor); worst error / allowance {rel[0][0]:.3f} ({rel[0][1]})")
    assert len(real) > 20 and real[len(real) // 2] < 2e-3, f"median relative gradient error {real[len(real) // 2]:.2e}"
    assert rel[0][0] <= 1.0, f"worst gradients (error / allowance, key, relative error): {rel[:5]}"


def _norm_counts(mod):
    """{BatchNorm buffer prefix: elements per channel on the DISTINCT batch} of the layers that run on the B source frames."""
    n, h, w = {}, H, W
    for i in range(len(mod.down_blocks)):
        h, w = h // 2, w // 2
        n[f"down_blocks.{i}.norm"] = B * h * w
    if mod.use_spade:
        for i in range(len(mod.middle)):
            n[f"middle.{i}.norm1"] = n[f"middle.{i}.norm2"] = B * h * w
    return n


@pytest.mark.parametrize("use_spade", [True, False])
def test_batchnorm_buffers_match_the_replicated_path(use_spade):
    """Both paths see the same statistics up to fp32 summation order (eps 6e-8 through at most 11 layers: 2e-5 with room to
    spare); a running variance updated WITHOUT the replication count is off by momentum * var * (n/(n-1) - 5n/(5n-1)) -- about
    1e-3 of the buffer at the 4x8 maps (n = 64) -- which this tolerance must and does reject."""
    a, b = _pair(use_spade)
    names = [k for k in b["bufs"] if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert len(names) >= 9 and set(a["bufs"]) == set(b["bufs"])
    worst = 0.0
    for k in names:
        if k.endswith("num_batches_tracked"):
            assert torch.equal(a["bufs"][k], b["bufs"][k]) and int(b["bufs"][k]) == 1, k
            continue
        close(a["bufs"][k], b["bufs"][k], 2e-5, 2e-6, k)
        if k.endswith("running_var"):
            worst = max(worst, ((a["bufs"][k] - b["bufs"][k]).abs() / b["bufs"][k]).max().item())
    print(f"use_spade={use_spade}: running_var worst relative difference {worst:.2e}")
    seen = 0
    for pre, n in _norm_counts(b["mod"]).items():
        rv = b["bufs"][pre + ".running_var"].double()
        unbiased = (rv - (1.0 - MOMENTUM)) / MOMENTUM                         # of the 5n replicated elements
        without = (1.0 - MOMENTUM) + MOMENTUM * unbiased * (T * n - 1) / (T * n) * n / (n - 1)
        shift = ((without - rv).abs() / rv).max().item()
        if n <= 64:
            print(f"{pre}: without the replication count running_var would be off by {shift:.1e}")
            assert not torch.allclose(without, rv, rtol=2e-5, atol=2e-6), pre
            seen += 1
    assert seen == (9 if use_spade else 1)


@pytest.mark.parametrize("use_spade", [True, False])
@pytest.mark.parametrize("b,t", [(1, 5), (2, 1), (1, 1)])
def test_single_frame_and_single_clip_run(use_spade, b, t):
    mod = _generator(use_spade)
    frame, flow, occ = _inputs(b, t)
    r = _step(mod, frame, flow, occ, t)
    assert r["y"].shape == (t * b, 3, H, W) and torch.isfinite(r["y"]).all()
    assert all(torch.isfinite(g).all() for g in r["grads"].values()) and torch.isfinite(r["dflow"]).all()
    with pytest.raises(ValueError):
        mod(frame, flow, occ, source_repeats=t + 1)


@pytest.mark.parametrize("use_spade", [True, False])
def test_two_identical_steps_give_identical_gradients(use_spade):
    mod = _generator(use_spade)
    frame, flow, occ = _inputs()
    r0, r1 = _step(mod, frame, flow, occ, T), _step(mod, frame, flow, occ, T)
    assert torch.equal(r0["y"], r1["y"]) and torch.equal(r0["dflow"], r1["dflow"]) and torch.equal(r0["docc"], r1["docc"])
    bad = [k for k in r0["grads"] if not torch.equal(r0["grads"][k], r1["grads"][k])]
    assert not bad, f"{len(bad)} gradients differ between two runs of the same step: {bad[:6]}"
