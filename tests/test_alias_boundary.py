"""SURVEY.md 8(b) "Registry API": the reference's UNCHANGED callers against the alias package.

They import more than the registries (`segdino3d.utils`, `segdino3d.datasets.dataset`, `segdino3d.models.module`,
`segdino3d.gtypes`); the alias owns the model side and falls through to the reference checkout for the rest
(segdino3d_amd/install.py).  The first test replays the callers' exact import lines against a stub tree laid out like the
reference (its files are written here: a few lines each, no reference source), in fresh interpreters, for both ways in -
this repository first on PYTHONPATH, and a script started from the reference checkout through `python -m segdino3d_amd.run`.
The last one checks that the fall-through submodules are the checkout's own files, found from another directory."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the import lines of the reference's callers, verbatim (file:line in the comment)
CALLER_LINES = """
from segdino3d import build_architecture                                          # train_3d.py:18
from segdino3d.utils import get_rank, init_distributed_mode, is_main_process      # train_3d.py:19
from segdino3d.utils import is_main_process, get_rank                             # evaluation/evaluate_3d.py:9
from segdino3d.datasets.dataset import ScanNet200InstanceSeg3D                    # evaluation/evaluate_3d.py:14
from segdino3d.datasets.dataset import ScanNetInstanceSeg3D                       # evaluation/evaluate_3d.py:15
from segdino3d import build_dataset                                               # utils/dataset_utils.py:6
from segdino3d.models.module import NestedTensor, nested_tensor_from_tensor_list  # utils/dataset_utils.py:7
from segdino3d.utils import get_world_size, is_main_process                       # utils/train_utils.py:4
"""

BUILD_AND_CHECK = """
import segdino3d, segdino3d_amd
assert segdino3d.__file__.startswith(REPO), segdino3d.__file__
from segdino3d_amd.configs import scannet200_model_cfg, scannetv2_model_cfg
model = build_architecture(scannet200_model_cfg(query_num=200))
assert type(model) is segdino3d_amd.Baseline3D and type(model.backbone) is segdino3d_amd.Res16UNet34C
assert type(build_architecture(scannetv2_model_cfg()).backbone) is segdino3d_amd.SpConvUNet
ds = build_dataset(dict(type="ScanNet200InstanceSeg3D", split="val"))             # registered by the fall-through datasets
assert type(ds) is ScanNet200InstanceSeg3D and ds.target_type is segdino3d_amd.GD3DTarget
assert segdino3d.datasets_import_error is None
from segdino3d.models.backbone import Res16UNet34C, SpConvUNet
from segdino3d.models.decoder import ScanNetQueryDecoder
from segdino3d.models.architecture import Baseline3D
from segdino3d.models.loss import ScanNetUnifiedCriterion
from segdino3d.builder import ARCHITECTURES, build_from_cfg
assert ARCHITECTURES.get("Baseline3D") is Baseline3D
print("ALIAS-OK", get_rank(), is_main_process(), NestedTensor.__module__)
"""


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(textwrap.dedent(text))


def _stub_reference(root):
    """A tree laid out like the reference checkout; every file a stand-in of a few lines with the same import lines."""
    pkg = os.path.join(root, "segdino3d")
    # the reference's own package __init__ imports MinkowskiEngine / spconv through models.backbone: must never run
    _write(os.path.join(pkg, "__init__.py"), "raise ImportError('reference segdino3d/__init__.py executed (needs MinkowskiEngine)')\n")
    _write(os.path.join(pkg, "utils", "__init__.py"),
           "from .dist_utils import get_rank, is_main_process, init_distributed_mode, get_world_size, is_dist_avail_and_initialized\n")
    _write(os.path.join(pkg, "utils", "dist_utils.py"), """
        def get_rank(): return 0
        def get_world_size(): return 1
        def is_main_process(): return True
        def is_dist_avail_and_initialized(): return False
        def init_distributed_mode(args): args.distributed = False
        """)
    _write(os.path.join(pkg, "models", "__init__.py"), "raise ImportError('reference segdino3d/models/__init__.py executed')\n")
    _write(os.path.join(pkg, "models", "module", "__init__.py"), "from .nested_tensor import NestedTensor, nested_tensor_from_tensor_list\n")
    _write(os.path.join(pkg, "models", "module", "nested_tensor.py"), """
        class NestedTensor:
            def __init__(self, tensors, mask): self.tensors, self.mask = tensors, mask
        def nested_tensor_from_tensor_list(ts): return NestedTensor(ts, None)
        """)
    # datasets/ has no __init__.py in the reference (namespace package); dataset/, preparer/, transform/ do
    _write(os.path.join(pkg, "datasets", "dataset", "__init__.py"),
           "from .scannet200 import ScanNet200InstanceSeg3D\nfrom .scannet import ScanNetInstanceSeg3D\n")
    for mod, cls in (("scannet200", "ScanNet200InstanceSeg3D"), ("scannet", "ScanNetInstanceSeg3D")):
        _write(os.path.join(pkg, "datasets", "dataset", mod + ".py"), f"""
            from segdino3d import DATASETS, build_transform          # {mod}.py:12-13
            from segdino3d.gtypes import GD3DTarget                  # {mod}.py:13-14
            @DATASETS.register_module()
            class {cls}:
                target_type = GD3DTarget
                def __init__(self, split): self.split = split
            """)
    _write(os.path.join(pkg, "datasets", "preparer", "__init__.py"), "from .instance_seg_3d_preparer import InstanceSeg3DDataPreparer\n")
    _write(os.path.join(pkg, "datasets", "preparer", "instance_seg_3d_preparer.py"), """
        from segdino3d import PREPARERS                              # instance_seg_3d_preparer.py:6
        @PREPARERS.register_module()
        class InstanceSeg3DDataPreparer: pass
        """)
    _write(os.path.join(pkg, "datasets", "transform", "__init__.py"), "from .segment_3d_transforms import Segment3DTransform\n")
    _write(os.path.join(pkg, "datasets", "transform", "segment_3d_transforms.py"), """
        from segdino3d import (TRANSFORMS, build_preparer, build_transform)     # segment_3d_transforms.py:4
        @TRANSFORMS.register_module()
        class Segment3DTransform: pass
        """)
    _write(os.path.join(root, "train_3d.py"), "REPO = %r\n" % ROOT + CALLER_LINES + BUILD_AND_CHECK)
    return root


def _run(cmd, cwd, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "SEGDINO3D_REFERENCE_ROOT")}
    env["PYTHONPATH"] = ROOT
    env.update(extra_env or {})
    return subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_script_started_from_the_reference_checkout(tmp_path):
    """`python -m segdino3d_amd.run train_3d.py` from the checkout: the script's directory precedes PYTHONPATH, the launcher
    installs the alias first; the stub's own `segdino3d/__init__.py` (which raises) is never executed."""
    ref = _stub_reference(str(tmp_path / "SegDINO3D"))
    r = _run([sys.executable, "-m", "segdino3d_amd.run", "train_3d.py"], cwd=ref)
    assert r.returncode == 0 and "ALIAS-OK 0 True segdino3d.models.module.nested_tensor" in r.stdout, r.stdout + r.stderr
    # without the launcher the reference's package wins (this is why the launcher exists)
    r2 = _run([sys.executable, "train_3d.py"], cwd=ref)
    assert r2.returncode != 0 and "reference segdino3d/__init__.py executed" in r2.stderr


def test_repository_first_on_sys_path(tmp_path):
    """`python -c` / `-m` / pytest with this repository first on PYTHONPATH: plain `import segdino3d` is the alias; the
    checkout is located through SEGDINO3D_REFERENCE_ROOT (or found on sys.path / in the working directory)."""
    ref = _stub_reference(str(tmp_path / "SegDINO3D"))
    code = "REPO = %r\n" % ROOT + CALLER_LINES + BUILD_AND_CHECK
    r = _run([sys.executable, "-c", code], cwd=str(tmp_path), extra_env={"SEGDINO3D_REFERENCE_ROOT": ref})
    assert r.returncode == 0 and "ALIAS-OK" in r.stdout, r.stdout + r.stderr
    # no checkout anywhere: the model side still works, the reference-only submodules are simply absent
    code2 = ("import segdino3d\nfrom segdino3d import build_architecture, DATASETS\nfrom segdino3d.gtypes import GD3DTarget\n"
             "import importlib.util as u\nassert u.find_spec('segdino3d.utils') is None\nprint('MODEL-ONLY-OK')")
    r = _run([sys.executable, "-c", code2], cwd=str(tmp_path))
    assert r.returncode == 0 and "MODEL-ONLY-OK" in r.stdout, r.stdout + r.stderr


def test_checkout_submodules_fall_through(tmp_path):
    """The checkout found through SEGDINO3D_REFERENCE_ROOT from an unrelated working directory: `segdino3d.utils` and
    `segdino3d.models.module` are the checkout's own files, executed in place; the registries they would register into and
    `build_architecture` are the AMD ones."""
    ref = _stub_reference(str(tmp_path / "SegDINO3D"))
    code = "REF = %r\n" % ref + textwrap.dedent("""
        import os
        from segdino3d import build_architecture
        from segdino3d.utils import get_rank, init_distributed_mode, is_main_process
        from segdino3d.utils import get_world_size, is_dist_avail_and_initialized
        from segdino3d.models.module import NestedTensor, nested_tensor_from_tensor_list
        import segdino3d, segdino3d.utils, segdino3d.models.module as mm
        assert segdino3d.utils.__file__.startswith(REF + os.sep), segdino3d.utils.__file__
        assert mm.__file__.startswith(REF + os.sep), mm.__file__
        assert get_rank() == 0 and is_main_process() and get_world_size() == 1 and not is_dist_avail_and_initialized()
        assert isinstance(nested_tensor_from_tensor_list([]), NestedTensor)
        from segdino3d_amd.configs import scannet200_model_cfg
        import segdino3d_amd
        assert type(build_architecture(scannet200_model_cfg())) is segdino3d_amd.Baseline3D
        print("FALLTHROUGH-OK")
        """)
    elsewhere = tmp_path / "elsewhere"
    elsewhere.mkdir()
    r = _run([sys.executable, "-c", code], cwd=str(elsewhere), extra_env={"SEGDINO3D_REFERENCE_ROOT": ref})
    assert r.returncode == 0 and "FALLTHROUGH-OK" in r.stdout, r.stdout + r.stderr
