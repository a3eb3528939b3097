"""Frame sizes that are not multiples of 64 (128x416, the KITTI aspect ratio, and 188x352), end to end on the GPU (-m gpu).

At those sizes the up-sampled path and its skip disagree by a pixel at five sites, where the reference bilinear-resizes
and we call ops.resize_bilinear_grad.  The fixtures (tests/golden/anysize_*.npz, tools/capture_anysize_golden.py) come
from the live reference; the acceptance logic is test_gpu_model.py's, restated with the frame size taken from the meta.
The new extents (47, 23, 13, 11, 5, ...) also put every convolution route on shapes the 128x256 suite never builds:
test_conv_problems_of_odd_frame_sizes checks each distinct problem of a step against fp64 torch."""
import copy
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from c2m_amd import ops
from c2m_amd.config import default_config, normalize_config
from c2m_amd.modules.model import GeneratorFullModel
from c2m_amd.synthetic import make_batch, make_step_rng, batch_to
from c2m_amd.train import TrainStep
from oracle import c2m_oracle as O
from oracle.golden_util import synth_state, summarize, synth_input, check_compact
from golden_io import Case, names
from gpu_util import close, rel_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ZERO_GRAD_BIASES = {
    "appearance_encoder.roi_align_blocks.2.bias", "appearance_encoder.roi_align_regressor.bias",
    "appearance_encoder.fuse_appearance_roi.bias", "motion_encoder.sparse_motion_estimator.x_encoder.2.bias",
    "motion_encoder.sparse_motion_estimator.encode_scene_features.0.bias",
    "motion_encoder.sparse_motion_estimator.encode_scene_features.3.bias"}
MASKS = ("sparse_motion_bin", "sparse_occ_bw", "sparse_occ_fw")
E2E = [n for n in names("anysize_e2e_") if "fullwidth" not in n]


def _model_and_batch(c, device=DEV):
    m = c.meta
    cfg = normalize_config(m["cfg"])
    model = GeneratorFullModel(train_params=cfg["train_params"], model_params=cfg["model_params"], dataset="cityscapes")
    model.load_state_dict(synth_state(m["spec"], m["seed"]), strict=True)
    model.to(device).train()
    batch = batch_to(make_batch(m["batch_size"], m["H"], m["W"], m["t_in"], seed=m["seed"]), device)
    rng = c.group("rng")
    batch["rng"] = dict(latent_traj=rng["latent_traj"].to(device), eps=rng["eps"].to(device),
                        click_index=rng["click_index"].long().to(device))
    return cfg, model, batch


def test_fixtures_cover_both_sizes_and_every_site():
    sizes = {(Case(n).meta["H"], Case(n).meta["W"]) for n in names("anysize_")}
    assert sizes == {(128, 416), (188, 352)}
    assert len(E2E) == 3 and len(names("anysize_inf_")) == 1 and len(names("anysize_mod_")) == 3


@pytest.mark.parametrize("name", E2E)
def test_train_step_vs_golden(name):
    """test_gpu_model.test_train_step_vs_golden's acceptance logic for gt-theta fixtures (bit-exact masks)."""
    c = Case(name)
    assert c.meta["use_gt_training"]
    cfg, model, batch = _model_and_batch(c)
    out, lg, ld = TrainStep(model, run_optimizers=False, distributed=False)(batch)
    torch.cuda.synchronize()
    ref_l = c.group("loss")
    assert [k for k in lg] == [k for k in ref_l], "loss dict keys / order"
    for k, v in lg.items():
        close(v, ref_l[k], 1e-4 if k != "perceptual" else 2e-4, 1e-6, f"loss {k}")
    ref_di, ref_dv = c.group("loss_d_image"), c.group("loss_d_video")
    if ref_di:
        close(ld["total_image_dis"], (ref_di["d_real"] + ref_di["d_fake"]) * 0.5, 1e-4, 1e-6)
        close(ld["total_video_dis"], (ref_dv["d_real"] + ref_dv["d_fake"]) * 0.5, 1e-4, 1e-6)
    for k in MASKS:
        mism = int((out[k].cpu() != c.mask(k)).sum())
        assert mism == 0, f"{k} must be bit-exact ({mism} pixels differ)"
    for k, ref in c.group("sub.out").items():
        close(out[k][:, :, :, ::16, ::16], ref, 1e-3, 1e-4, f"out {k}")
    for k, ref in c.group("out").items():
        close(out[k], ref, 1e-3, 1e-4, f"out {k}")
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    ref_g = c.group("sum.grad")
    assert set(got) == set(ref_g), f"grad key set differs: {sorted(set(got) ^ set(ref_g))[:6]}"
    numel = {k: max(p.numel(), 1) for k, p in model.named_parameters()}
    per_elem = sorted(ref_g[k][1].item() / numel[k] for k in ref_g)
    noise = 1e-3 * per_elem[len(per_elem) // 2]
    gtol, bad = 5e-3, []
    for k, ref in ref_g.items():
        s = summarize(got[k].cpu())
        assert np.all(np.isfinite(s)), f"non-finite gradient {k}"
        if k in ZERO_GRAD_BIASES:
            assert s[1] <= 10 * max(ref[1].item(), noise * numel[k]), f"{k}: {s[1]} vs reference noise {ref[1].item()}"
            continue
        if not (abs(s[1] - ref[1].item()) <= gtol * abs(ref[1].item()) + noise * numel[k] and
                abs(s[2] - ref[2].item()) <= 2 * gtol * abs(ref[2].item()) + noise * noise * numel[k]):
            bad.append((k, s[1], ref[1].item()))
    # step-function derivatives (LeakyReLU, L1 sign, max-pool) flip within rounding of 0: the same allowance as test_gpu_model
    worse = [b for b in bad if abs(b[1] - b[2]) > 5e-2 * abs(b[2]) + noise * numel[b[0]]]
    assert len(bad) <= max(4, len(ref_g) // 10) and not worse, f"{len(bad)} gradients off: {bad[:5]}"
    nograd = sorted(k for k, p in model.named_parameters() if p.requires_grad and p.grad is None)
    assert nograd == sorted(c.json("nograd")), "set of trainable params that never get a gradient"
    bufs = dict(model.named_buffers())
    for k, ref in c.group("sum.buf").items():
        np.testing.assert_allclose(summarize(bufs[k].cpu()), ref.numpy(), rtol=1e-3, atol=1e-5, err_msg=f"buf {k}")


@pytest.mark.parametrize("name", names("anysize_inf_"))
def test_inference_vs_golden(name):
    c = Case(name)
    m = c.meta
    cfg = normalize_config(m["cfg"])
    model = GeneratorFullModel(train_params=cfg["train_params"], model_params=cfg["model_params"], dataset="cityscapes")
    model.load_state_dict(synth_state(m["spec"], m["seed"]), strict=True)
    model.to(DEV).train(not m["eval_mode"])
    batch = batch_to(make_batch(m["batch_size"], m["H"], m["W"], m["t_in"], seed=m["seed"]), DEV)
    rng = c.group("rng")
    torch.manual_seed(m["seed"])
    with torch.no_grad():
        out = model.inference(batch["video"], batch["bg_mask"], batch["fg_mask"], batch["instance_mask"],
                              batch.get("input_of"), batch.get("input_occ"), batch["tracking_gnn"],
                              rng["click_index"].long().to(DEV), c.group("in")["z_m"].to(DEV))
    torch.cuda.synchronize()
    exact = m["use_gt_eval"]
    for k in MASKS:
        mism = int((out[k].cpu() != c.mask(k)).sum())
        if exact:
            assert mism == 0, f"{k} must be bit-exact ({mism} pixels differ)"
        else:
            assert mism <= 0.06 * float(c.mask("sparse_motion_bin").sum()), f"{k}: {mism} pixels differ"
    ref_out = c.group("out")
    assert torch.equal(out["index_user_guidance"].cpu(), ref_out.pop("index_user_guidance"))
    for k, ref in ref_out.items():
        close(out[k], ref, 1e-3, 1e-4, f"out {k}")
    if exact:
        for k, ref in c.group("sub.out").items():
            close(out[k][:, :, :, ::8, ::8], ref, 2e-3, 2e-4, f"out {k}")
    tol = 1e-3 if exact else 3e-2
    for k, ref in c.group("sum.out").items():
        got = summarize(out[k].cpu())
        assert abs(got[1] - ref[1].item()) <= tol * abs(ref[1].item()) + 1e-4, f"|{k}| sum {got[1]} vs {ref[1].item()}"
    assert set(out) == set(c.group("sum.out")) | set(c.group("out")) | set(MASKS), "output key surface"
    bufs = dict(model.named_buffers())
    for k, ref in c.group("sum.buf").items():
        close(torch.from_numpy(summarize(bufs[k].cpu())), ref, 1e-6, 1e-7, f"buf {k}")


def _product_module(c):
    from c2m_amd.modules.generator.generator import OcclusionAwareGenerator
    from c2m_amd.modules.generator.flowembedder import FlowEmbedder
    from c2m_amd.modules.motion_estimator.motion_autoencoder import DenseMotionDecoder
    m = c.meta
    if m["module"] == "generator":
        mod = OcclusionAwareGenerator(copy.deepcopy(m["generator"]), copy.deepcopy(m["flow_embedder"]), input_channel=3,
                                      dataset="cityscapes")
        return mod, (lambda i: {"y": mod(i["first_frame"], i["flow"], i["occlusion_map"])}), \
            ("first_frame", "flow", "occlusion_map")
    if m["module"] == "flowembedder":
        mod = FlowEmbedder(copy.deepcopy(m["flow_embedder"]))
        return mod, (lambda i: {f"y{j}": v for j, v in enumerate(mod(i["x"]))}), ("x",)
    mod = DenseMotionDecoder(copy.deepcopy(m["decoder"]))

    def call(i):
        app = {k[4:]: v for k, v in i.items() if k.startswith("app.")}
        sp = {k[7:]: v for k, v in i.items() if k.startswith("sparse.")}
        return mod(app, sp, i["sparse_motion"], i["sparse_occlusion"], i["z"])
    return mod, call, tuple(k for k in m["inputs"] if k not in ("sparse_motion", "sparse_occlusion"))


@pytest.mark.parametrize("name", names("anysize_mod_"))
def test_module_vs_golden(name):
    """DenseMotionDecoder (both _match sites), FlowEmbedder (decoder skip) and the SPADE generator (conditioning size and
    final size): test_gpu_model.test_standalone_module_vs_golden's tolerances."""
    c = Case(name)
    seed = c.meta["seed"]
    mod, call, gin = _product_module(c)
    mod.load_state_dict(synth_state(c.meta["spec"], seed), strict=True)
    mod.to(DEV).train()
    inp = {k: synth_input(v).to(DEV) for k, v in c.meta["inputs"].items()}
    for k in gin:
        inp[k].requires_grad_(True)
    outs = call(inp)
    total = 0
    for j, (k, v) in enumerate(sorted(outs.items())):
        total = total + (v * rnd(seed + 100 + j, *v.shape).to(DEV)).sum()
    total.backward()
    for k, v in outs.items():
        check_compact(c.arr, "out", k, v, 2e-4, f"{name} out.{k}")
    # the SPADE generator at 188x352: the reference's own input gradients move by up to 5.7e-2 (max) / 5.7e-3 (norm-wise) of
    # their scale between fp32 and fp64 evaluation (LeakyReLU slopes flipped within rounding of 0); 2e-2 on a subsample
    gtol = 2e-2 if c.meta["module"] == "generator" else 5e-3
    for k in gin:
        check_compact(c.arr, "gin", k, inp[k].grad, gtol, f"{name} d{k}")
    got = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
    ref_keys = {k.split(".", 1)[1] for k in c.arr if k.startswith(("grad.", "sumgrad."))}
    assert set(got) == ref_keys, f"params with grads differ: {sorted(set(got) ^ ref_keys)[:6]}"
    gscale = max(float(np.abs(c.arr[k]).max()) for k in c.arr if k.startswith(("grad.", "subgrad.")))
    for k in sorted(ref_keys):
        check_compact(c.arr, "grad", k, got[k], 5e-3, f"{name} grad.{k}", floor=1e-2 * gscale)
    nograd = sorted(k for k, p in mod.named_parameters() if p.requires_grad and p.grad is None)
    assert nograd == sorted(c.json("nograd"))
    bufs = dict(mod.named_buffers())
    for k in {k.split(".", 1)[1] for k in c.arr if k.startswith(("buf.", "sumbuf."))}:
        check_compact(c.arr, "buf", k, bufs[k].float(), 1e-3, f"{name} buf.{k}", floor=1e-3)


def test_full_width_step_188x352():
    """BASELINE widths, t_in 2, B 1, generator only, at 188x352: losses, masks and sub-sampled outputs against the
    reference's fingerprints; every gradient (but the analytically zero ones) against the CPU oracle on the same weights and draws under the project's fp32
    gate (worst <= 1e-2 norm-wise with the analytically-zero noise floor, median <= 2e-3)."""
    import os
    c = Case("anysize_e2e_fullwidth_188x352")
    m = c.meta
    cfg, model, batch = _model_and_batch(c)
    out, lg, _ = TrainStep(model, run_optimizers=False, distributed=False)(batch)
    torch.cuda.synchronize()
    ref_l = c.group("loss")
    assert [k for k in lg] == [k for k in ref_l]
    for k, v in lg.items():
        close(v, ref_l[k], 2e-4, 1e-6, f"loss {k}")
    for k in MASKS:
        assert torch.equal(out[k].cpu(), c.mask(k)), k
    for k, ref in c.group("sub.out").items():
        close(out[k][:, :, :, ::16, ::16], ref, 1e-3, 1e-4, f"out {k}")
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    S = O.State(synth_state(m["spec"], m["seed"]))
    ob = make_batch(m["batch_size"], m["H"], m["W"], m["t_in"], seed=m["seed"])
    r = c.group("rng")
    olg = O.forward(S, cfg, ob, dict(latent_traj=r["latent_traj"], eps=r["eps"], click_index=r["click_index"].long()))[1]
    O.train_step_backward(cfg, olg, {}, {})
    og = S.grads()
    gg = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(og) == set(gg) == set(c.group("sum.grad"))
    rms = sorted((og[k].double().norm().item() / og[k].numel() ** 0.5) for k in og)
    noise = 1e-3 * rms[len(rms) // 2]
    rel = []
    for k in og:
        a, b = gg[k].cpu().double(), og[k].double()
        if k in ZERO_GRAD_BIASES:          # analytically zero: rounding residue of a cancelling sum, same order only
            assert a.norm().item() <= 10 * max(b.norm().item(), noise * b.numel() ** 0.5), f"{k}: {a.norm()} vs {b.norm()}"
            continue
        err = (a - b).norm().item()
        rel.append((err / (1e-2 * b.norm().item() + noise * b.numel() ** 0.5), k, err / max(b.norm().item(), 1e-30)))
    rel.sort(reverse=True)
    real = sorted(r for _, k, r in rel if og[k].double().norm().item() > 10 * noise * og[k].numel() ** 0.5)
    assert len(real) > 100 and real[len(real) // 2] < 2e-3, f"median relative gradient error {real[len(real) // 2]:.2e}"
    assert rel[0][0] <= 1.0, f"worst gradients (error / allowance, key, relative error): {rel[:5]}"


def test_step_is_deterministic_188x352():
    c = Case("anysize_e2e_tin2_spade_full_188x352")
    losses, grads = [], []
    for _ in range(2):
        cfg, model, batch = _model_and_batch(c)
        out, lg, ld = TrainStep(model, run_optimizers=False, distributed=False)(batch)
        losses.append(float(lg["total_gen"].detach()))
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert losses[0] == losses[1]
    bad = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not bad, f"{len(bad)} gradients differ between two runs of the same step: {bad[:6]}"


def _tiny_cfg(H, W):
    cfg = normalize_config(default_config(height=H, width=W, num_input_frames=2, block_expansion=4, max_expansion=32, h_dim=32,
                                          z_dim=16, out_channel=16, ndf=4))
    cfg["train_params"]["use_gt_training"] = True
    return cfg


def test_graph_replay_matches_eager_128x416():
    """TrainStep.capture at 128x416: the resize launches are legal inside a HIP-graph capture, replays equal the eager step."""
    cfg = _tiny_cfg(128, 416)
    tp = cfg["train_params"]

    def run(graph):
        torch.manual_seed(0)
        model = GeneratorFullModel(train_params=copy.deepcopy(tp), model_params=copy.deepcopy(cfg["model_params"]),
                                   dataset="cityscapes").to(DEV).train()
        step = TrainStep(model, run_optimizers=True, distributed=False)
        batch = batch_to(make_batch(1, 128, 416, 2, seed=61), DEV)
        rng = make_step_rng(batch, z_dim=16, latent_dim=32, seed=0)
        batch["rng"] = {k: v.to(DEV) for k, v in rng.items()}
        if graph:
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            step.capture(batch)
            model.load_state_dict(sd)
        totals = []
        for _ in range(3):
            _, lg, _ = step(batch)
            totals.append(float(lg["total_gen"].detach()))
        torch.cuda.synchronize()
        return totals, model.generator.first.conv.weight.detach().clone()

    te, we = run(False)
    tg, wg = run(True)
    assert te == tg, f"losses differ: eager {te} vs graph {tg}"
    assert torch.equal(we, wg)


def test_bf16_mode_step_188x352():
    """configs[2-4]'s bf16 operand mode at 188x352: every gradient finite, losses within 2e-2 of the fp32 HIP step."""
    cfg = _tiny_cfg(188, 352)
    tp = cfg["train_params"]
    torch.manual_seed(0)
    sd = GeneratorFullModel(train_params=copy.deepcopy(tp), model_params=copy.deepcopy(cfg["model_params"]),
                            dataset="cityscapes").state_dict()
    batch = batch_to(make_batch(1, 188, 352, 2, seed=71), DEV)
    rng = make_step_rng(batch, z_dim=16, latent_dim=32, seed=0)
    batch["rng"] = {k: v.to(DEV) for k, v in rng.items()}
    res = []
    for prec in ("fp32", "bf16"):
        model = GeneratorFullModel(train_params=copy.deepcopy(tp), model_params=copy.deepcopy(cfg["model_params"]),
                                   dataset="cityscapes")
        model.load_state_dict(sd)
        model.to(DEV).train()
        with ops.conv_precision(prec):
            _, lg, _ = TrainStep(model, run_optimizers=False, distributed=False)(batch)
        torch.cuda.synchronize()
        res.append(({k: float(v.detach()) for k, v in lg.items()}, model))
    (l32, _), (l16, m16) = res
    for k, ref in l32.items():
        assert np.isfinite(l16[k]) and abs(l16[k] - ref) <= 2e-2 * abs(ref) + 1e-4, f"bf16 loss {k}: {l16[k]} vs fp32 {ref}"
    bad = [k for k, p in m16.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    assert not bad, f"non-finite bf16-mode gradients: {bad[:6]}"


# ------------------------------------------------------------------------------------- every conv route at odd extents
def _record_conv_problems(monkeypatch, cfg, B, H, W, dims):
    """Distinct (x shape, w shape, stride, padding, padding mode, bias) of one training step, through a wrapper around
    ops.conv installed for this step only."""
    seen = {}
    real = ops.conv

    def rec(x, w, b=None, stride=1, padding=0, padding_mode="zeros", *a, **kw):
        key = (tuple(x.shape), tuple(w.shape), stride if isinstance(stride, int) else tuple(stride),
               padding if isinstance(padding, int) else tuple(padding), padding_mode, b is not None)
        seen.setdefault(key, None)
        return real(x, w, b, stride, padding, padding_mode, *a, **kw)
    monkeypatch.setattr(ops, "conv", rec)
    tp = cfg["train_params"]
    torch.manual_seed(0)
    model = GeneratorFullModel(train_params=copy.deepcopy(tp), model_params=copy.deepcopy(cfg["model_params"]),
                               dataset="cityscapes").to(DEV).train()
    batch = batch_to(make_batch(B, H, W, tp["num_input_frames"], seed=81), DEV)
    rng = make_step_rng(batch, z_dim=dims[0], latent_dim=dims[1], seed=0)
    batch["rng"] = {k: v.to(DEV) for k, v in rng.items()}
    TrainStep(model, run_optimizers=False, distributed=False)(batch)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "conv", real)
    return list(seen)


def _ref_conv(x, w, b, stride, pad, mode):
    nd = x.dim() - 2
    pads = (pad,) * nd if isinstance(pad, int) else tuple(pad)
    if mode == "reflect" and any(pads):
        tup = []
        for p in reversed(pads):
            tup += [p, p]
        x = F.pad(x, tuple(tup), mode="reflect")
        pads = (0,) * nd
    return (F.conv2d if nd == 2 else F.conv3d)(x, w, b, stride=stride, padding=pads)


def _sizes_problems(monkeypatch):
    probs = set()
    for H, W in ((128, 416), (188, 352)):
        probs.update(_record_conv_problems(monkeypatch, _tiny_cfg(H, W), 2, H, W, (16, 32)))
    full = normalize_config(default_config(height=188, width=352, num_input_frames=2, use_image_discriminator=False,
                                           use_video_discriminator=False))
    for p in _record_conv_problems(monkeypatch, full, 1, 188, 352, (1024, 1024)):
        xs, ws = p[0], p[1]
        out_px = int(np.prod(xs[2:]))
        if out_px * ws[0] * int(np.prod(ws[1:])) * xs[0] <= 2e8:      # fp64 CPU reference affordable
            probs.add(p)
    return sorted(probs)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_conv_problems_of_odd_frame_sizes(precision, monkeypatch):
    """Forward, data gradient and weight gradient of every distinct convolution of a step at 128x416 and 188x352 (tiny
    widths, plus the affordable problems of the full-width generator) against fp64 torch on the CPU, with the tolerances of
    test_gpu_ops' conv tests for the same mode (bf16 mode: bf16-representable operands, as test_conv_bf16_mode)."""
    probs = _sizes_problems(monkeypatch)
    odd = [p for p in probs if any(e % 2 for e in p[0][-2:])]
    assert len(odd) >= 10, f"only {len(odd)} problems with an odd spatial extent"
    bad = []
    for xs, ws, stride, pad, mode, has_b in probs:
        seed = zlib.crc32(str((xs, ws, stride, pad, mode)).encode()) % 10000
        x = rnd(seed, *xs)
        w = rnd(seed + 1, *ws, scale=(1.0 / int(np.prod(ws[1:]))) ** 0.5)
        b = rnd(seed + 2, ws[0], scale=0.1) if has_b else None
        if precision == "bf16":
            x, w = x.bfloat16().float(), w.bfloat16().float()
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        yr = _ref_conv(xr, wr, None if b is None else b.double(), stride, pad, mode)
        go = rnd(seed + 3, *yr.shape)
        if precision == "bf16":
            go = go.bfloat16().float()
        (yr * go.double()).sum().backward()
        xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        with ops.conv_precision(precision):
            y = ops.conv(xg, wg, None if b is None else b.to(DEV), stride=stride, padding=pad, padding_mode=mode)
            (y.float() * go.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        ftol = 4e-3 if precision == "bf16" and ws[0] > 4 else 2e-5
        what = f"{precision} x{list(xs)} w{list(ws)} s{stride} p{pad} {mode}"
        for a, r, tol, part in ((y.float(), yr, ftol, "fwd"), (xg.grad, xr.grad, 5e-5, "dgrad"), (wg.grad, wr.grad, 1e-4, "wgrad")):
            try:
                rel_close(a, r.detach(), tol, f"{what} {part}")
            except AssertionError as e:
                bad.append(str(e))
    assert not bad, f"{len(bad)} of {3 * len(probs)} checks failed: {bad[:6]}"
