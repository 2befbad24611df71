"""CPU suite: the Chamfer reconstruction losses ('chamfer', 'cd_sum' of utils/model_helper.py:43-52) are wired through every
layer -- header, ctypes table, library, lion_amd.chamfer3d, loss_fn -- and, like every other operator, have no CPU path."""
import os

import pytest
import torch

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lion_chamfer_loss_reduce", "lion_chamfer_loss_backward")


def test_both_symbols_are_declared_bound_and_exported():
    from lion_amd import _lib, chamfer3d
    abi_check.declared_bound_and_exported(NEW)
    assert "ChamferLossFunction" in chamfer3d.__all__ and "chamfer_loss" in chamfer3d.__all__
    # bad arguments are refused on the host, before any launch: NULL pointers, empty clouds, both gradients NULL
    l = _lib.load()
    assert l.lion_chamfer_loss_reduce(None, None, 1, 4, 4, 1.0, 1.0, None, None) == -1
    assert l.lion_chamfer_loss_backward(None, None, None, None, None, 1, 4, 4, 1.0, 1.0, None, None, None) == -1


@pytest.mark.parametrize("loss_type", ["chamfer", "cd_sum"])
def test_chamfer_loss_types_reach_the_kernels_and_have_no_cpu_path(loss_type):
    from lion_amd.models.vae_adain import loss_fn
    B = 2
    pred, target = torch.rand(B, 8, 3), torch.rand(B, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_fn(pred, target, loss_type, 3, B)


def test_chamfer_loss_rejects_an_unknown_reduction():
    from lion_amd.chamfer3d import chamfer_loss
    with pytest.raises(ValueError, match="reduction"):
        chamfer_loss(torch.rand(1, 4, 3), torch.rand(1, 4, 3), "max")


@pytest.mark.parametrize("loss_type", ["emd", "chamfer_emd", "cd1_sum_emd", "cd1_sum", "dcd", "l1_cd"])
def test_other_loss_types_stay_unimplemented(loss_type):
    from lion_amd.models.vae_adain import loss_fn
    with pytest.raises(NotImplementedError):
        loss_fn(torch.rand(2, 8, 3), torch.rand(2, 8, 3), loss_type, 3, 2)
