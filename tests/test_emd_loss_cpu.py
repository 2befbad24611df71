"""CPU suite: the EMD reconstruction losses ('emd', 'chamfer_emd' of utils/model_helper.py:82-96) are wired through every
layer -- header, ctypes table, library, lion_amd.emd, loss_fn, the config default -- and, like every other operator, have no
CPU path.  The suites that scan the whole library (tests/test_cabi_cpu.py: header <-> ctypes table; test_launch_sites_cpu.py;
test_isa_cpu.py) cover the new entry points and kernels as they stand."""
import inspect

import pytest
import torch

import abi_check

NEW = ("lion_emd_loss_forward", "lion_emd_loss_backward")
EINVAL, EWORKSPACE = -1, -3


def test_both_symbols_are_declared_bound_and_exported():
    from lion_amd import emd
    abi_check.declared_bound_and_exported(NEW)
    assert "EmdLossFunction" in emd.__all__ and "emd_loss" in emd.__all__
    assert callable(emd.emd_loss) and issubclass(emd.EmdLossFunction, torch.autograd.Function)


def test_bad_arguments_are_refused_on_the_host():
    """NULL inputs, non-positive sizes, no workspace: each returns before any launch (there is no device here to launch on);
    the pointers that pass the NULL test are never dereferenced on the host"""
    from lion_amd import _lib
    l = _lib.load()
    p = 4096                                                         # any non-NULL value
    big = 1 << 20
    assert l.lion_emd_loss_forward(None, p, 1, 4, 4, p, None, None, p, big, None) == EINVAL
    assert l.lion_emd_loss_forward(p, None, 1, 4, 4, p, None, None, p, big, None) == EINVAL
    assert l.lion_emd_loss_forward(p, p, 1, 4, 4, None, p, p, p, big, None) == EINVAL
    for b, n, m in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert l.lion_emd_loss_forward(p, p, b, n, m, p, None, None, p, big, None) == EINVAL
        assert l.lion_emd_loss_backward(p, p, None, b, n, m, p, None, None) == EINVAL
    need = l.lion_emd_workspace_bytes(2, 65, 63)
    assert l.lion_emd_loss_forward(p, p, 2, 65, 63, p, None, None, p, need - 1, None) == EWORKSPACE
    assert l.lion_emd_loss_forward(p, p, 2, 65, 63, p, None, None, None, need, None) == EWORKSPACE
    # backward: no gloss; neither direction; half a pair
    assert l.lion_emd_loss_backward(None, p, None, 1, 4, 4, p, None, None) == EINVAL
    assert l.lion_emd_loss_backward(p, None, None, 1, 4, 4, None, None, None) == EINVAL
    assert l.lion_emd_loss_backward(p, p, None, 1, 4, 4, None, None, None) == EINVAL
    assert l.lion_emd_loss_backward(p, None, p, 1, 4, 4, p, None, None) == EINVAL


@pytest.mark.parametrize("loss_type", ["emd", "chamfer_emd"])
def test_emd_loss_types_have_no_cpu_path(loss_type):
    from lion_amd.models.vae_adain import loss_fn
    assert inspect.signature(loss_fn).parameters["loss_weight_emd"].default == 0.02
    pred, target = torch.rand(2, 8, 3), torch.rand(2, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_fn(pred, target, loss_type, 3, 2)
    with pytest.raises(NotImplementedError, match=f"{loss_type}: no CPU path"):
        loss_fn(pred, target, loss_type, 3, 2, loss_weight_emd=0.5)


def test_emd_loss_itself_refuses_cpu_tensors():
    from lion_amd.emd import emd_loss
    with pytest.raises(RuntimeError, match="no CPU path"):
        emd_loss(torch.rand(1, 4, 3, requires_grad=True), torch.rand(1, 4, 3))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        emd_loss(torch.rand(1, 4, 3), torch.rand(1, 4, 3))


@pytest.mark.parametrize("loss_type", ["cd1_sum_emd", "cd1_sum", "dcd", "l1_cd"])
def test_the_remaining_loss_types_stay_unimplemented(loss_type):
    from lion_amd.models.vae_adain import loss_fn
    with pytest.raises(NotImplementedError) as e:
        loss_fn(torch.rand(2, 8, 3), torch.rand(2, 8, 3), loss_type, 3, 2, loss_weight_emd=0.02)
    assert "no CPU path" not in str(e.value)


def test_config_default_and_get_loss_forward_the_weight():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models import vae_adain
    assert released_prior_cfg().ddpm.loss_weight_emd == 0.02
    assert "loss_weight_emd" in inspect.getsource(vae_adain.Model.get_loss)
