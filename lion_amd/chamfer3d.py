"""Chamfer distance operator module -- replaces the reference's JIT-built ``chamfer_3D``
extension and mirrors third_party/ChamferDistancePytorch/chamfer3D/dist_chamfer_3D.py:41-133.

``chamfer_3D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2) -> int`` and
``chamfer_3D.backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2) -> int``
keep the reference's "caller pre-allocates the outputs" contract (chamfer_cuda.cpp:17-33).

``chamfer_loss`` / ``ChamferLossFunction`` are the reconstruction losses built on it (utils/model_helper.py:43-52,
``ddpm.loss_type`` 'chamfer' and 'cd_sum'): the forward launch, one reduction launch and a gather-form gradient without
atomics (csrc/chamfer.hip) -- the same bits on every run, capturable, no vendor-library launch in between."""
import torch
from torch import nn
from torch.autograd import Function
from torch.amp import custom_fwd, custom_bwd

from . import _lib

__all__ = ["chamfer_3D", "chamfer_3DFunction", "chamfer_3DDist", "chamfer_3DFunction_noGrad",
           "chamfer_3DDist_nograd", "ChamferLossFunction", "chamfer_loss"]


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


class ChamferLossFunction(Function):
    """(pred [B,N,3], target [B,M,3], s1, s2) -> loss [B] = s1 * sum_j dist1[:, j] + s2 * sum_k dist2[:, k], dist1 / dist2 being
    chamfer_3DFunction's squared nearest-neighbour distances pred -> target and target -> pred.  Three launches of the library
    in all (lion_chamfer_forward, lion_chamfer_loss_reduce; lion_chamfer_loss_backward), every output a torch.empty buffer that
    its kernel writes in full, no host synchronisation.  The gradient (expression order: include/lion_hip.h) has no atomics."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, target, s1, s2):
        _lib.require_cuda(pred, target)
        dist1, dist2, idx1, idx2 = _alloc(pred, target)
        b, n, _ = pred.shape
        m = target.shape[1]
        loss = torch.empty(b, device=pred.device)
        _lib.call("lion_chamfer_forward", pred, target, b, n, m, dist1, dist2, idx1, idx2)
        _lib.call("lion_chamfer_loss_reduce", dist1, dist2, b, n, m, s1, s2, loss)
        ctx.save_for_backward(pred, target, idx1, idx2)
        ctx.scales = (s1, s2)
        return loss

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, gloss):
        pred, target, idx1, idx2 = ctx.saved_tensors
        b, n, _ = pred.shape
        m = target.shape[1]
        # the VAE needs the prediction's gradient only: a direction nobody asked for is a NULL pointer and is not launched
        gpred = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        gtarget = torch.empty_like(target) if ctx.needs_input_grad[1] else None
        _lib.call("lion_chamfer_loss_backward", pred, target, idx1, idx2, gloss.contiguous(), b, n, m, *ctx.scales,
                  gpred, gtarget)
        return gpred, gtarget, None, None


def chamfer_loss(pred, target, reduction="mean"):
    """Chamfer reconstruction loss per sample, [B]: "mean" = dist1.mean(1) + dist2.mean(1) (model_helper.py:49-52, 'chamfer'),
    "sum" = dist1.sum(1) + dist2.sum(1) (:43-47, 'cd_sum'); pred [B,N,3], target [B,M,3]."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"chamfer_loss: reduction must be 'mean' or 'sum', got {reduction!r}")
    n, m = pred.shape[1], target.shape[1]
    s1, s2 = (1.0 / n, 1.0 / m) if reduction == "mean" else (1.0, 1.0)
    return ChamferLossFunction.apply(pred.contiguous(), target.contiguous(), s1, s2)
