"""Drop-in boundary: `c2m_amd.install_as_reference_layout()` makes the reference's src/train.py and Trainer run on
c2m_amd without edits.  Runs in child processes because it re-binds the top-level names `modules`, `losses`, `utils`.

The reference's own sources are not part of this repository, so the "patched" mode is checked against a stand-in `utils`
package written into the test's temporary directory: the layout the reference's src/utils has (a package whose __init__
star-imports `.ops` and `.utils`), with its own functions of the hot-path names and of names the trainer needs untouched.
"""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_STANDIN = {
    "utils/__init__.py": "from .ops import *\nfrom .utils import *\n",
    "utils/ops.py": "".join(f"def {n}(*a, **k):\n    return 'stand-in'\n" for n in
                            ("resample", "get_grid", "get_occlusion_map", "grid_sample", "get_corresponding_map", "tensor2im")),
    "utils/utils.py": "".join(f"def {n}(*a, **k):\n    return 'stand-in'\n" for n in
                              ("resize_flow", "resize_video", "isnan", "dist_all_reduce_tensor", "dist_all_gather_tensor",
                               "save_parameters", "set_random_seed", "init_cudnn")),
}

_CHILD = r'''
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, STANDIN)
import torch
import c2m_amd
assert c2m_amd.install_as_reference_layout() == "patched"

# --- the reference-side utils package stays in place, with only the hot-path functions replaced
import utils, utils.ops, utils.utils
assert utils.__file__.startswith(STANDIN), utils.__file__
import c2m_amd.utils as ours
for name in ("resample", "get_grid", "get_occlusion_map", "resize_flow", "resize_video", "isnan"):
    assert getattr(utils, name) is getattr(ours, name), name
assert utils.ops.resample is ours.resample and utils.utils.resize_flow is ours.resize_flow
for name in ("dist_all_reduce_tensor", "dist_all_gather_tensor", "save_parameters", "tensor2im", "grid_sample",
             "get_corresponding_map", "set_random_seed", "init_cudnn"):
    assert getattr(utils, name).__module__.startswith("utils."), name     # untouched reference-side code

# --- train.py's imports (`from modules.model import GeneratorFullModel`, `from torch_geometric.data import Batch, Data`)
from modules.model import GeneratorFullModel
import losses.losses
import c2m_amd.modules.model as ours_model
assert GeneratorFullModel is ours_model.GeneratorFullModel
assert losses.losses.__name__.startswith("c2m_amd.")
from torch_geometric.data import Batch, Data
assert hasattr(Batch, "from_data_list") and hasattr(Batch, "pin_memory")

# --- the update step reaches the first HIP op, which refuses host tensors loudly (no fallback)
from c2m_amd.config import default_config, normalize_config
from c2m_amd.synthetic import make_batch
from c2m_amd.train import TrainStep
cfg = normalize_config(default_config(num_input_frames=1, block_expansion=4, max_expansion=32, h_dim=32, z_dim=16,
                                      out_channel=16, ndf=4, height=32, width=64))
c2m = GeneratorFullModel(train_params=cfg["train_params"], model_params=cfg["model_params"], dataset="cityscapes")
try:
    TrainStep(c2m, distributed=False)(make_batch(2, 32, 64, 1, seed=0))
except RuntimeError as e:
    assert "HIP device" in str(e), e
    import traceback
    assert any("/c2m_amd/ops.py" in f.filename for f in traceback.extract_tb(e.__traceback__))
else:
    raise AssertionError("the update step ran without a GPU: a CPU fallback exists on the product path")
print("PATCHED-OK")
'''


def test_layout_patches_a_reference_utils_package_in_place(tmp_path):
    standin = tmp_path / "ref_src"
    for rel, text in _STANDIN.items():
        (standin / rel).parent.mkdir(parents=True, exist_ok=True)
        (standin / rel).write_text(text)
    code = f"ROOT = {ROOT!r}\nSTANDIN = {str(standin)!r}\n" + textwrap.dedent(_CHILD)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PATCHED-OK" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-4000:]


def test_layout_without_reference_aliases_utils(tmp_path):
    """Stand-alone use (no reference on sys.path): `utils` resolves to c2m_amd.utils with the trainer-facing helpers."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import c2m_amd
        assert c2m_amd.install_as_reference_layout() == "aliased"
        import utils
        from utils.utils import set_random_seed, init_cudnn
        for n in ("resample", "get_occlusion_map", "resize_flow", "resize_video", "dist_all_reduce_tensor",
                  "dist_all_gather_tensor", "get_world_size", "is_master"):
            assert hasattr(utils, n), n
        from torch_geometric.data import Batch, Data
        assert hasattr(Batch, "from_data_list") and hasattr(Batch, "pin_memory")
        import torch
        t = torch.ones(3)
        assert utils.dist_all_gather_tensor(t) is t and utils.dist_all_reduce_tensor(t) is t
        print("ALIAS-OK")
    """)
    r = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALIAS-OK" in r.stdout, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
