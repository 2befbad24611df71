"""Approximate earth mover's distance -- replaces the reference's JIT-built ``emd_ext`` module
(third_party/PyTorchEMD/cuda/emd.cpp:23-27) and mirrors emd.py:6-51 / emd_nograd.py:6-44."""
import torch
from torch.amp import custom_fwd, custom_bwd

from . import _lib

__all__ = ["emd_ext", "emd_cuda", "earth_mover_distance", "earth_mover_distance_nograd",
           "EarthMoverDistanceFunction", "EarthMoverDistanceFunctionNoGrad", "EmdLossFunction", "emd_loss"]


def _ws(b, n, m, dev):
    nbytes = _lib.load().lion_emd_workspace_bytes(b, n, m)
    return torch.empty((nbytes,), device=dev, dtype=torch.uint8), nbytes


class _EmdModule:
    """approxmatch_forward / matchcost_forward / matchcost_backward, xyz point-major [B,N,3]."""

    @staticmethod
    def approxmatch_forward(xyz1, xyz2):
        _lib.require_cuda(xyz1, xyz2)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        match = torch.empty((b, m, n), device=xyz1.device, dtype=torch.float32)
        ws, nbytes = _ws(b, n, m, xyz1.device)
        _lib.call("lion_emd_approxmatch", xyz1, xyz2, b, n, m, match, ws, nbytes)
        return match

    @staticmethod
    def matchcost_forward(xyz1, xyz2, match):
        _lib.require_cuda(xyz1, xyz2, match)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        cost = torch.empty((b,), device=xyz1.device, dtype=torch.float32)
        ws, nbytes = _ws(b, n, m, xyz1.device)
        _lib.call("lion_emd_matchcost", xyz1, xyz2, match, b, n, m, cost, ws, nbytes)
        return cost

    @staticmethod
    def matchcost_backward(grad_cost, xyz1, xyz2, match):
        _lib.require_cuda(grad_cost, xyz1, xyz2, match)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        g1 = torch.empty((b, n, 3), device=xyz1.device, dtype=torch.float32)
        g2 = torch.empty((b, m, 3), device=xyz1.device, dtype=torch.float32)
        _lib.call("lion_emd_matchcost_backward", grad_cost, xyz1, xyz2, match, b, n, m, g1, g2)
        return [g1, g2]


emd_ext = emd_cuda = _EmdModule()


class EarthMoverDistanceFunction(torch.autograd.Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, xyz1, xyz2):
        xyz1 = xyz1.contiguous()
        xyz2 = xyz2.contiguous()
        assert xyz1.is_cuda and xyz2.is_cuda, "Only support cuda currently."
        match = emd_ext.approxmatch_forward(xyz1, xyz2)
        cost = emd_ext.matchcost_forward(xyz1, xyz2, match)
        ctx.save_for_backward(xyz1, xyz2, match)
        return cost

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_cost):
        xyz1, xyz2, match = ctx.saved_tensors
        g1, g2 = emd_ext.matchcost_backward(grad_cost.contiguous(), xyz1, xyz2, match)
        return g1, g2


class EarthMoverDistanceFunctionNoGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1 = xyz1.contiguous()
        xyz2 = xyz2.contiguous()
        assert xyz1.is_cuda and xyz2.is_cuda, "Only support cuda currently."
        # no gradient needed: the fused path never materialises the [B,N,M] match matrix
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        cost = torch.empty((b,), device=xyz1.device, dtype=torch.float32)
        ws, nbytes = _ws(b, n, m, xyz1.device)
        _lib.call("lion_emd_cost", xyz1, xyz2, b, n, m, cost, ws, nbytes)
        return cost


class EmdLossFunction(torch.autograd.Function):
    """(pred [B,N,3], target [B,M,3]) -> loss [B] = matchcost / N on lion_emd_approxmatch's auction, the match held constant
    in the gradient (EarthMoverDistanceFunction's value and semantics) -- without the [B,M,N] match matrix: one call of
    lion_emd_loss_forward accumulates the cost and, for the inputs that need a gradient, d(N * loss)/d(input) level by
    level; those [B,N,3] / [B,M,3] buffers are what is saved, and the backward is one elementwise launch.  Every output is a
    torch.empty buffer its kernel writes in full; no atomics, no host synchronisation (orders: include/lion_hip.h)."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, target):
        _lib.require_cuda(pred, target)
        b, n, _ = pred.shape
        m = target.shape[1]
        loss = torch.empty((b,), device=pred.device, dtype=torch.float32)
        g1u = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        g2u = torch.empty_like(target) if ctx.needs_input_grad[1] else None
        ws, nbytes = _ws(b, n, m, pred.device)
        _lib.call("lion_emd_loss_forward", pred, target, b, n, m, loss, g1u, g2u, ws, nbytes)
        ctx.save_for_backward(g1u, g2u)
        ctx.dims = (b, n, m)
        return loss

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, gloss):
        g1u, g2u = ctx.saved_tensors
        gpred = None if g1u is None else torch.empty_like(g1u)
        gtarget = None if g2u is None else torch.empty_like(g2u)
        _lib.call("lion_emd_loss_backward", gloss.contiguous(), g1u, g2u, *ctx.dims, gpred, gtarget)
        return gpred, gtarget


def emd_loss(pred, target):
    """EMD reconstruction loss per sample, [B] (utils/model_helper.py:82-96: earth_mover_distance(pred, target,
    transpose=False)); pred [B,N,3], target [B,M,3].  Without grad mode no gradient buffer is allocated or accumulated."""
    if not torch.is_grad_enabled():   # a Function's needs_input_grad ignores the grad mode
        pred, target = pred.detach(), target.detach()
    return EmdLossFunction.apply(pred.contiguous(), target.contiguous())


def _prep(xyz1, xyz2, transpose):
    if xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    if transpose:
        xyz1 = xyz1.transpose(1, 2)
        xyz2 = xyz2.transpose(1, 2)
    assert xyz1.shape[-1] == 3, f'require it to be B,N,3; get: {xyz1.shape}'
    return xyz1, xyz2


def earth_mover_distance(xyz1, xyz2, transpose=True):
    """(b,3,n)|(b,n,3) clouds -> per-pair cost / n  (emd.py:31-51)."""
    xyz1, xyz2 = _prep(xyz1, xyz2, transpose)
    return EarthMoverDistanceFunction.apply(xyz1, xyz2) / float(xyz1.shape[1])


def earth_mover_distance_nograd(xyz1, xyz2, transpose=True):
    """emd_nograd.py:19-44."""
    xyz1, xyz2 = _prep(xyz1, xyz2, transpose)
    return EarthMoverDistanceFunctionNoGrad.apply(xyz1, xyz2) / float(xyz1.shape[1])
