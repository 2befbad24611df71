"""The precision policy of the voxel convolutions (conv_ops.PRECISION, lion_amd.conv_precision) without a GPU: which
shapes the single-product kernel takes, the default, the chain's policy key, the context manager, the C binding."""
import inspect

import pytest
import torch


def test_half_supported_and_use_half_truth_table():
    from lion_amd import conv_ops
    rows = [((64, 64, 8), False),     # r = 8 stays on the three-product kernel
            ((4, 64, 32), False),     # Cin % 16
            ((64, 48, 32), False),    # Cout % 32
            ((64, 64, 32), True), ((128, 128, 16), True), ((16, 32, 16), True)]
    for args, want in rows:
        assert conv_ops.half_supported(*args) is want, args
        assert conv_ops.use_half(*args) is False, args          # the default policy never selects it
        with conv_ops.conv_precision("half"):
            assert conv_ops.use_half(*args) is want, args
    assert all(conv_ops.split_supported(*a) for a, w in rows if w)   # it only ever replaces a split launch


def test_half_is_inference_only():
    from lion_amd import conv_ops
    x = torch.zeros(1, 64, 2, 2, 2, requires_grad=True)
    with conv_ops.conv_precision("half"):
        assert not conv_ops.use_half(64, 64, 32, x)             # grad enabled, input requires grad: policy ignored
        with torch.no_grad():
            assert conv_ops.use_half(64, 64, 32, x)
        assert conv_ops.use_half(64, 64, 32, x.detach())
    src = inspect.getsource(conv_ops._Conv3dK3.forward) + inspect.getsource(conv_ops.conv3d_k3_dgrad)
    assert src.count("half=False") == 2                         # the training ops never take it


def test_default_is_fp32_and_the_public_keyword_defaults_to_it():
    import os
    import lion_amd
    from lion_amd import conv_ops, sampling
    from lion_amd.diffusion import DiffusionDiscretized
    from lion_amd.diffusion_continuous import DiffusionVPSDE
    from lion_amd.models.lion import LION
    assert conv_ops.PRECISION == os.environ.get("LION_CONV_PRECISION", "fp32")   # "fp32" unless the environment asks
    assert 'os.environ.get("LION_CONV_PRECISION", "fp32")' in inspect.getsource(conv_ops)
    for fn in (sampling.generate_samples_vada_2prior, DiffusionDiscretized.run_ddim,
               DiffusionDiscretized.run_denoising_diffusion, DiffusionVPSDE.sample_model_ode, LION.sample):
        assert inspect.signature(fn).parameters["conv_precision"].default == "fp32", fn
    with pytest.raises(ValueError):
        with lion_amd.conv_precision("bf16"):
            pass
    with pytest.raises(ValueError):
        conv_ops.requested_precision("fp16")


def test_policy_key_differs_between_the_settings():
    import lion_amd
    from lion_amd import chain
    base = chain.policy_key()
    with lion_amd.conv_precision("half"):
        half = chain.policy_key()
    assert base != half and chain.policy_key() == base
    with lion_amd.conv_precision("fp32"):
        assert chain.policy_key() == base


def test_context_manager_restores_the_previous_value_on_exception():
    import lion_amd
    from lion_amd import conv_ops
    assert conv_ops.PRECISION == "fp32"
    with pytest.raises(KeyError):
        with lion_amd.conv_precision("half"):
            assert conv_ops.PRECISION == "half"
            with conv_ops.requested_precision("fp32"):          # a sampler's default keyword leaves the ambient setting
                assert conv_ops.PRECISION == "half"
            raise KeyError("boom")
    assert conv_ops.PRECISION == "fp32"
    with conv_ops.requested_precision("half"):
        assert conv_ops.PRECISION == "half"
    assert conv_ops.PRECISION == "fp32"


def test_the_symbol_is_bound_with_the_split_entrys_signature():
    from lion_amd import _lib
    assert _lib.SIGNATURES["lion_conv3d_k3_half_forward"] == _lib.SIGNATURES["lion_conv3d_k3_split_forward"]
    lib = _lib.load()
    assert lib.lion_conv3d_k3_half_forward.argtypes == lib.lion_conv3d_k3_split_forward.argtypes
