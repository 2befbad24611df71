"""lion_amd.shim.install(): the advertised zero-edit drop-in.  After it, the REFERENCE's autograd wrappers
(third_party/pvcnn/functional/*.py, PyTorchEMD/emd.py, ChamferDistancePytorch) must resolve their native module to
liblion_hip.so's operator objects.  Wiring only (no GPU here): run in a fresh interpreter (python -B) over a stand-in
of the reference's package tree written by this test -- the same module names, each wrapper importing its native
module the way the reference's does (``from third_party.pvcnn.functional.backend import _backend``, ``from
third_party.PyTorchEMD.backend import emd_cuda_dynamic as emd_cuda``), and a Chamfer module that would JIT-build."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PVCNN_WRAPPERS = {   # module -> (function the package exports, backend call it makes)
    "voxelization": ("avg_voxelize", "avg_voxelize_forward"),
    "devoxelization": ("trilinear_devoxelize", "trilinear_devoxelize_forward"),
    "ball_query": ("ball_query", "ball_query"),
    "grouping": ("grouping", "grouping_forward"),
    "sampling": ("furthest_point_sample", "furthest_point_sampling"),
    "interpolatation": ("nearest_neighbor_interpolate", "three_nearest_neighbors_interpolate_forward"),
}


def _stand_in_tree(root):
    """the reference's package layout with its import edges; every wrapper forwards its arguments to the backend"""
    def write(rel, text):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    for pkg in ("third_party", "third_party/pvcnn", "third_party/PyTorchEMD", "third_party/ChamferDistancePytorch",
                "third_party/ChamferDistancePytorch/chamfer3D"):
        write(pkg + "/__init__.py", "")
    init = []
    for mod, (fn, call) in PVCNN_WRAPPERS.items():
        write(f"third_party/pvcnn/functional/{mod}.py",
              "from third_party.pvcnn.functional.backend import _backend\n\n\n"
              f"def {fn}(*args):\n    return _backend.{call}(*args)\n")
        init.append(f"from third_party.pvcnn.functional.{mod} import {fn}\n")
    write("third_party/pvcnn/functional/__init__.py", "".join(init))
    write("third_party/pvcnn/functional/backend.py", "raise ImportError('the native extension would be JIT-built here')\n")
    write("third_party/PyTorchEMD/emd.py", "from third_party.PyTorchEMD.backend import emd_cuda_dynamic as emd_cuda\n")
    write("third_party/PyTorchEMD/backend.py", "raise ImportError('the native extension would be JIT-built here')\n")
    write("third_party/ChamferDistancePytorch/chamfer3D/dist_chamfer_3D.py",
          "raise ImportError('the native extension would be JIT-built here')\n")


SCRIPT = r'''
import os, sys, torch
import lion_amd.shim
REF = os.environ["LION_SHIM_TREE"] + "/"
m, c, e = lion_amd.shim.install()
from lion_amd.functional.backend import _backend as ours
from lion_amd import chamfer3d, emd

# 1. the reference's package: every wrapper module pulled OUR _backend (bindings.cpp:10-37 names)
import third_party.pvcnn.functional as F
assert F.__file__.startswith(REF), F.__file__
# (the package rebinds names like `ball_query` / `grouping` to the functions: fetch the modules from sys.modules)
for short in ("voxelization", "devoxelization", "ball_query", "grouping", "sampling", "interpolatation"):
    mod = sys.modules["third_party.pvcnn.functional." + short]
    assert mod.__file__.startswith(REF), mod.__file__
    assert mod._backend is ours, mod.__name__
for name in ("gather_features_forward", "gather_features_backward", "furthest_point_sampling", "ball_query",
             "grouping_forward", "grouping_backward", "three_nearest_neighbors_interpolate_forward",
             "three_nearest_neighbors_interpolate_backward", "trilinear_devoxelize_forward",
             "trilinear_devoxelize_backward", "avg_voxelize_forward", "avg_voxelize_backward"):
    assert callable(getattr(ours, name)), name

# 2. calling the reference's wrapper reaches our operator: CPU tensors -> our "no CPU path" error
try:
    F.avg_voxelize(torch.zeros(1, 2, 4), torch.zeros(1, 3, 4, dtype=torch.int32), 4)
except RuntimeError as ex:
    assert "lion_amd" in str(ex), ex
else:
    raise AssertionError("the reference wrapper did not reach lion_amd's backend")

# 3. EMD: the reference's autograd Function binds emd_ext
import third_party.PyTorchEMD.emd as ref_emd
assert ref_emd.__file__.startswith(REF)
assert ref_emd.emd_cuda is emd.emd_ext
for name in ("approxmatch_forward", "matchcost_forward", "matchcost_backward"):
    assert callable(getattr(ref_emd.emd_cuda, name))

# 4. Chamfer: importing the reference's module path yields ours (no JIT build, no write into the tree)
from third_party.ChamferDistancePytorch.chamfer3D.dist_chamfer_3D import chamfer_3DDist
assert chamfer_3DDist is chamfer3d.chamfer_3DDist
print("WIRED")
'''


def test_install_rewires_the_reference_wrappers(tmp_path):
    tree = str(tmp_path / "reference")
    _stand_in_tree(tree)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, tree])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    env["LION_SHIM_TREE"] = tree
    out = subprocess.run([sys.executable, "-B", "-c", SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "WIRED" in out.stdout
