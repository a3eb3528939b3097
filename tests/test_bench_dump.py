"""bench.py's --dump-outputs writer on the host: names, dtypes, the size budget and seeded samples that repeat."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _step_result():
    """A train step's (generated, generator losses, D losses) and a model whose gradients it left, all on the host."""
    g = torch.Generator().manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 300), torch.nn.Linear(300, 5), torch.nn.Linear(5, 5))
    x = torch.randn(7, 64, generator=g)
    loss = model[1](model[0](x)).square().mean()
    loss.backward()                                          # model[2] keeps grad None
    generated = {"generated": torch.randn(2, 3, 5, 64, 64, generator=g), "mask": torch.rand(2, 1, 8, 8, generator=g) > 0.5,
                 "idx": torch.arange(12), "theta": [torch.randn(3, generator=g), None], "unused": None}
    return (generated, {"kl": loss, "total_gen": loss * 2}, {}), model


def test_dump_outputs_budget_dtypes_and_repeatable_samples(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 256 << 10)
    monkeypatch.setattr(bench, "DUMP_GRAD_SAMPLE", 4096)
    result, model = _step_result()
    files = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        written = bench.dump_outputs(str(d), result, model)
        got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert sum(a.nbytes for a in got.values()) == written <= 256 << 10
        files.append(got)
    a, b = files
    assert sorted(a) == ["grad_norms", "grad_sample", "loss.kl", "loss.total_gen", "out.generated", "out.idx", "out.mask",
                         "out.theta.0"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    gen = result[0]["generated"].reshape(-1)
    assert 0 < a["out.generated"].size < gen.numel()                  # larger than its share: a sample of the tensor's values
    assert np.isin(a["out.generated"], gen.numpy()).all()
    np.testing.assert_array_equal(a["out.idx"], np.arange(12, dtype=np.float64))
    assert a["out.idx"].dtype == np.float64 and a["out.mask"].dtype == np.float32
    np.testing.assert_array_equal(a["loss.total_gen"], np.float32(float(result[1]["total_gen"].detach())))
    norms = a["grad_norms"]
    params = list(model.parameters())
    assert norms.shape == (len(params) - 2,)                            # model[2] has no gradient: not listed
    np.testing.assert_allclose(norms, [float(p.grad.double().norm()) for p in params[:-2]], rtol=1e-12)
    grads = torch.cat([p.grad.reshape(-1) for p in params[:-2]]).numpy()
    assert a["grad_sample"].size == 4096 and np.isin(a["grad_sample"], grads).all()
