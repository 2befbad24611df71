"""Chamfer distance operator module -- replaces the reference's JIT-built ``chamfer_3D``
extension and mirrors third_party/ChamferDistancePytorch/chamfer3D/dist_chamfer_3D.py:41-133.

``chamfer_3D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2) -> int`` and
``chamfer_3D.backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2) -> int``
keep the reference's "caller pre-allocates the outputs" contract (chamfer_cuda.cpp:17-33)."""
import torch
from torch import nn
from torch.autograd import Function
from torch.amp import custom_fwd, custom_bwd

from . import _lib

__all__ = ["chamfer_3D", "chamfer_3DFunction", "chamfer_3DDist", "chamfer_3DFunction_noGrad",
           "chamfer_3DDist_nograd"]


class _Chamfer3DModule:
    """Same two entry points as the pybind module built from chamfer_cuda.cpp."""

    @staticmethod
    def forward(xyz1, xyz2, dist1, dist2, idx1, idx2):
        _lib.require_cuda(xyz1, xyz2, dist1, dist2, idx1, idx2)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        _lib.call("lion_chamfer_forward", xyz1, xyz2, b, n, m, dist1, dist2, idx1, idx2)
        return 1

    @staticmethod
    def backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2):
        _lib.require_cuda(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        _lib.call("lion_chamfer_backward", xyz1, xyz2, graddist1, graddist2, idx1, idx2, b, n, m, gradxyz1, gradxyz2)
        return 1


chamfer_3D = _Chamfer3DModule()


def _alloc(xyz1, xyz2):
    b, n, dim = xyz1.size()
    assert dim == 3, "Wrong last dimension for the chamfer distance 's input! Check with .size()"
    _, m, dim = xyz2.size()
    assert dim == 3, "Wrong last dimension for the chamfer distance 's input! Check with .size()"
    dev = xyz1.device
    return (torch.empty(b, n, device=dev), torch.empty(b, m, device=dev),
            torch.empty(b, n, device=dev, dtype=torch.int32),
            torch.empty(b, m, device=dev, dtype=torch.int32))


class chamfer_3DFunction(Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, xyz1, xyz2):
        dist1, dist2, idx1, idx2 = _alloc(xyz1, xyz2)
        chamfer_3D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.empty_like(xyz2)
        chamfer_3D.backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1.contiguous(),
                            graddist2.contiguous(), idx1, idx2)
        return gradxyz1, gradxyz2


class chamfer_3DDist(nn.Module):
    def forward(self, input1, input2):
        return chamfer_3DFunction.apply(input1.contiguous(), input2.contiguous())


class chamfer_3DFunction_noGrad(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        dist1, dist2, idx1, idx2 = _alloc(xyz1, xyz2)
        chamfer_3D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2)
        return dist1, dist2, idx1, idx2


class chamfer_3DDist_nograd(nn.Module):
    def forward(self, input1, input2):
        return chamfer_3DFunction_noGrad.apply(input1.contiguous(), input2.contiguous())
