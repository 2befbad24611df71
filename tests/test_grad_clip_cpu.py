"""CPU side of gradient clipping: lion_amd.optim.get_opt maps a `trainer.opt` config onto the optimizer the way the Adam branch of
the reference's utils/utils.py:115-138 does -- `grad_clip` included, which no code read before -- and the three C entry points
refuse bad arguments before anything is launched."""
import ctypes

import pytest
import torch


def _cfgopt(**over):
    from lion_amd.config import released_prior_cfg
    c = released_prior_cfg().trainer.opt.clone()
    c.merge(over)
    return c


def _params():
    return [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5))]


def test_get_opt_reads_the_config():
    from lion_amd.optim import Adam, get_opt
    opt = get_opt(_params(), _cfgopt(lr=2e-4, beta1=0.8, beta2=0.95, weight_decay=3e-4))
    assert type(opt) is Adam
    g = opt.param_groups[0]
    assert g["lr"] == 2e-4 and g["betas"] == (0.8, 0.95) and g["weight_decay"] == 3e-4 and g["eps"] == 1e-8
    assert opt.ema_decay == 0.0 and opt.grad_norm is None


def test_get_opt_grad_clip():
    from lion_amd.optim import get_opt
    assert _cfgopt().grad_clip == -1.0                                     # the released configs: no clipping
    assert get_opt(_params(), _cfgopt()).max_grad_norm is None
    assert get_opt(_params(), _cfgopt(grad_clip=1.0)).max_grad_norm == 1.0
    # the explicit argument (the prior trainers' cfg.sde.grad_clip_max_norm) overrides the config, both ways
    assert get_opt(_params(), _cfgopt(grad_clip=1.0), grad_clip=0.5).max_grad_norm == 0.5
    assert get_opt(_params(), _cfgopt(grad_clip=1.0), grad_clip=-1.0).max_grad_norm is None
    assert get_opt(_params(), _cfgopt(), grad_clip=2).max_grad_norm == 2.0
    c = _cfgopt()
    del c["grad_clip"]                                                      # a config without the key
    assert get_opt(_params(), c).max_grad_norm is None


def test_adam_max_grad_norm_argument():
    from lion_amd.optim import Adam
    assert Adam(_params()).max_grad_norm is None
    assert Adam(_params(), max_grad_norm=None).max_grad_norm is None
    assert Adam(_params(), max_grad_norm=0).max_grad_norm is None
    assert Adam(_params(), max_grad_norm=-1.0).max_grad_norm is None
    assert Adam(_params(), max_grad_norm=0.25).max_grad_norm == 0.25
    with pytest.raises(ValueError, match="max_grad_norm"):
        Adam(_params(), max_grad_norm=float("nan"))


def test_get_opt_use_ema_wraps_and_hands_the_decay_over():
    from lion_amd.optim import Adam, get_opt
    from lion_amd.training import EMA
    opt = get_opt(_params(), _cfgopt(grad_clip=1.0), use_ema=True)
    assert isinstance(opt, EMA) and isinstance(opt.optimizer, Adam) and opt._folded
    assert opt.ema_decay == 0.9999 and opt.optimizer.ema_decay == 0.9999
    assert opt.optimizer.max_grad_norm == 1.0 and opt.grad_norm is None
    assert get_opt(_params(), _cfgopt(ema_decay=0.99), use_ema=True).optimizer.ema_decay == 0.99
    c = _cfgopt()
    del c["ema_decay"]
    assert get_opt(_params(), c, use_ema=True).optimizer.ema_decay == 0.9999    # the reference's constant
    assert EMA(torch.optim.SGD(_params(), lr=0.1), 0.5).grad_norm is None


@pytest.mark.parametrize("kind", ["sgd", "adamax", "lion", None])
def test_get_opt_other_types_raise(kind):
    from lion_amd.optim import get_opt
    c = _cfgopt(type=kind)
    with pytest.raises(NotImplementedError):
        get_opt(_params(), c)


def test_entry_points_refuse_bad_arguments_before_launching():
    from lion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)                                               # never dereferenced: every call returns first
    EINVAL = -1
    assert lib.lion_grad_sqnorm_partials(None, a, a, 1, a, None) == EINVAL
    assert lib.lion_grad_sqnorm_partials(a, a, a, 1, None, None) == EINVAL
    assert lib.lion_grad_sqnorm_partials(a, a, a, 0, a, None) == EINVAL
    assert lib.lion_grad_clip_coef(None, 1, 1.0, a, None) == EINVAL
    assert lib.lion_grad_clip_coef(a, 1, 1.0, None, None) == EINVAL
    assert lib.lion_grad_clip_coef(a, 0, 1.0, a, None) == EINVAL
    assert lib.lion_grad_clip_coef(a, 1, 0.0, a, None) == EINVAL
    assert lib.lion_grad_clip_coef(a, 1, float("nan"), a, None) == EINVAL
    assert lib.lion_adam_step_scaled(None, a, a, 1, 1, a, 0.9, 0.99, 1e-8, 0.0, 0.0, a, None) == EINVAL
    assert lib.lion_adam_step_scaled(a, a, a, 1, 1, a, 1.0, 0.99, 1e-8, 0.0, 0.0, a, None) == EINVAL
    assert lib.lion_adam_step_scaled(a, a, a, 1, 1, a, 0.9, 0.99, 1e-8, 0.0, 1.5, a, None) == EINVAL
