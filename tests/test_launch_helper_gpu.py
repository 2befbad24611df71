"""-m gpu: the one thing csrc/common.h's lion_launch owns besides the launch itself -- the dynamic-LDS limit of a kernel,
one slot per kernel instantiation, which only grows.  hipFuncSetAttribute state is per process, so the sequence runs in a
fresh child: the same vox_scatter_kernel instantiation is launched with a small request, then a large one, then the small
one again, and every result must be bit-identical to the path that computes the same thing with another kernel.  The
affine devoxelise runs the same sequence of channel counts; its ring kernel asks for one constant size, so there the
sequence checks that a slot already raised is left alone."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import numpy as np
import torch
from lion_amd import fused_ops as fo
from lion_amd.functional.backend import _backend as bk

B, N, r = 1, 2048, 32
rng = np.random.default_rng(2048)
co = torch.from_numpy(rng.standard_normal((B, 3, N)).astype(np.float32)).cuda()

# lion_voxel_index once, then lion_voxel_scatter at C = 1 (tens of KiB of LDS), C = 64 (the 160-KiB arena), C = 1 again:
# each against lion_voxelize_points_forward (the fused kernel; bit-identical by
# test_hip_parity_gpu.py::test_voxel_index_then_scatter_equals_fused_and_oracle)
plan = bk.voxel_index(co, r, True, 0.0)
assert plan is not None
for C in (1, 64, 1):
    feat = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32)).cuda()
    out = bk.voxel_scatter(feat, plan)
    ref, norm, ind, cnt = bk.voxelize_points_forward(feat, co, r, True, 0.0)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()), ("voxel_scatter", C)
    assert torch.equal(ind, plan["ind"]) and torch.equal(cnt, plan["cnt"]) and torch.equal(norm, plan["norm"])
    assert bool(out.abs().sum() > 0)
    print("scatter C=%d ok" % C)

# the affine devoxelise: lion_trilinear_devoxelize_affine_forward against lion_trilinear_devoxelize_plan +
# ..._planned_forward (documented bit-identical), same sequence of channel counts
vc = plan["norm"].contiguous()
dplan = fo.devoxelize_plan(vc, r)
assert dplan is not None
for C in (1, 64, 1):
    grid = torch.from_numpy(rng.standard_normal((B, C, r, r, r)).astype(np.float32)).cuda()
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, (B, C)).astype(np.float32)).cuda()
    shift = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).cuda()
    one = fo.devoxelize_affine(grid, vc, r, scale, shift)
    two = fo.devoxelize_affine(grid, vc, r, scale, shift, plan=dplan)
    torch.cuda.synchronize()
    assert np.array_equal(one.cpu().numpy(), two.cpu().numpy()), ("devoxelize_affine", C)
    assert bool(one.abs().sum() > 0)
    print("devox C=%d ok" % C)
print("DONE")
"""


def test_dynamic_lds_limit_grows_and_is_kept_per_kernel():
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.run([sys.executable, "-B", "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split()
    assert out.stdout.count(" ok") == 6 and lines[-1] == "DONE", out.stdout[-2000:]
