"""CPU suite of per-shape seeds (noise addressed by sample, not by batch position): the keyed C entry points are declared,
bound, exported and refuse bad arguments before any launch; sampling.shape_seeds addresses the SplitMix64 sequence in O(1);
the `seeds` keyword's refusals fire before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from abi_check import declared_bound_and_exported

NEW = ("lion_philox_normal_keyed", "lion_chain_update_noise_keyed", "lion_chain_update_noise_cm_keyed",
       "lion_chain_update_multistep_noise_keyed", "lion_chain_update_multistep_noise_cm_keyed", "lion_chain_diffuse_keyed")
EINVAL = -1


def test_symbols_declared_bound_and_exported():
    import os
    import re
    from lion_amd import chain
    declared_bound_and_exported(NEW)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "lion_hip.h")).read()
    words = {name: int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+)u" % name, txt).group(1), 16)
             for name in ("LION_START_STEP_WORD", "LION_DIFFUSE_STEP_WORD")}
    assert words == {"LION_START_STEP_WORD": 0xFFFFFFFE, "LION_DIFFUSE_STEP_WORD": 0xFFFFFFFF}
    assert (chain.START_STEP_WORD, chain.DIFFUSE_STEP_WORD) == (0xFFFFFFFE, 0xFFFFFFFF)
    assert min(words.values()) > 2 ** 31 - 1               # a step's word is its row index, an int: no step can have either


def test_entry_points_refuse_bad_arguments_before_launching():
    from lion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15                  # 16-byte aligned, never dereferenced: every call returns first
    # name -> a call with keys, B, n (N for the channel-major forms) left open
    calls = {
        "lion_philox_normal_keyed": lambda k, B, n: lib.lion_philox_normal_keyed(k, B, n, 5, 0, a, None),
        "lion_chain_update_noise_keyed": lambda k, B, n: lib.lion_chain_update_noise_keyed(0, a, a, B, n, a, k, 0, a, a, None),
        "lion_chain_update_noise_cm_keyed": lambda k, B, n: lib.lion_chain_update_noise_cm_keyed(1, a, a, B, n, a, k, 0, a, None,
                                                                                                 None),
        "lion_chain_update_multistep_noise_keyed":
            lambda k, B, n: lib.lion_chain_update_multistep_noise_keyed(a, a, a, B, n, a, a, k, 0, a, a, None, None),
        "lion_chain_update_multistep_noise_cm_keyed":
            lambda k, B, n: lib.lion_chain_update_multistep_noise_cm_keyed(a, a, a, B, n, a, a, k, 0, a, a, a, None),
        "lion_chain_diffuse_keyed": lambda k, B, n: lib.lion_chain_diffuse_keyed(a, B, n, 0.5, 0.5, k, 1, a, None, None),
    }
    assert set(calls) == set(NEW)
    for name, f in calls.items():
        cm = "_cm_" in name
        assert f(None, 2, 8) == EINVAL, name                # NULL keys
        assert f(a, 0, 8) == EINVAL and f(a, -1, 8) == EINVAL, name   # B <= 0
        assert f(a, 2, 0) == EINVAL and f(a, 2, -4) == EINVAL, name   # n <= 0 / N <= 0
        if not cm:                                          # a channel-major sample holds 4*N elements: always whole quads
            for n in (1, 2, 3, 5, 6, 1022):
                assert f(a, 2, n) == EINVAL, (name, n)      # a quad would straddle two samples
        assert f(a, 65536, 8) == EINVAL, name               # more samples than the grid's y dimension holds
    # the other required pointers, the mode, the alignment
    assert lib.lion_philox_normal_keyed(a, 2, 8, 5, 0, None, None) == EINVAL
    assert lib.lion_philox_normal_keyed(a, 2, 8, 5, 0, a + 4, None) == EINVAL
    for mode in (-1, 2):
        assert lib.lion_chain_update_noise_keyed(mode, a, a, 2, 8, a, a, 0, a, None, None) == EINVAL
        assert lib.lion_chain_update_noise_cm_keyed(mode, a, a, 2, 2, a, a, 0, a, None, None) == EINVAL
    assert lib.lion_chain_update_noise_keyed(0, None, a, 2, 8, a, a, 0, a, None, None) == EINVAL
    assert lib.lion_chain_update_noise_keyed(0, a, None, 2, 8, a, a, 0, a, None, None) == EINVAL
    assert lib.lion_chain_update_noise_keyed(0, a, a, 2, 8, None, a, 0, a, None, None) == EINVAL
    assert lib.lion_chain_update_noise_keyed(0, a, a, 2, 8, a, a, 0, None, None, None) == EINVAL
    assert lib.lion_chain_update_noise_keyed(0, a + 4, a, 2, 8, a, a, 0, a, None, None) == EINVAL
    assert lib.lion_chain_update_noise_cm_keyed(0, a, a, 2, 2, a, a, 0, a, a + 8, None) == EINVAL
    assert lib.lion_chain_update_multistep_noise_keyed(a, a, None, 2, 8, a, a, a, 0, a, a, None, None) == EINVAL   # hist
    assert lib.lion_chain_update_multistep_noise_keyed(a, a, a, 2, 8, a, None, a, 0, a, a, None, None) == EINVAL   # table
    assert lib.lion_chain_update_multistep_noise_cm_keyed(a, a, a, 2, 2, None, a, a, 0, a, a, None, None) == EINVAL   # cur
    assert lib.lion_chain_update_multistep_noise_cm_keyed(a, a, a, 2, 2, a, a, a, 0, a, None, None, None) == EINVAL   # hist_out
    assert lib.lion_chain_diffuse_keyed(None, 2, 8, 0.5, 0.5, a, 1, a, None, None) == EINVAL
    assert lib.lion_chain_diffuse_keyed(a, 2, 8, 0.5, 0.5, a, 1, None, None, None) == EINVAL


def test_shape_seeds_address_the_splitmix_sequence():
    from lion_amd.chain import split_seed
    from lion_amd.editing import _split_seed
    from lion_amd.sampling import shape_seeds
    assert _split_seed is split_seed                        # one splitter for editing and sampling
    # SplitMix64's published first outputs from state 0 (Steele, Lea, Flood 2014; the reference implementation's test vector)
    assert split_seed(0, 3) == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for b in (0, 1, 0x1234567890ABCDEF, 2 ** 64 - 1, 2 ** 64 + 5, -3):
        assert shape_seeds(b, 0, 6) == shape_seeds(b, 0, 3) + shape_seeds(b, 3, 3)
        assert shape_seeds(b, 0, 6) == split_seed(b, 6)
        assert shape_seeds(b, 4, 2) == split_seed(b, 6)[4:]
        assert shape_seeds(b, 7, 0) == []
        assert all(0 <= s < 2 ** 64 for s in shape_seeds(b, 0, 6))
    assert shape_seeds(10 ** 12, 10 ** 9, 1) == shape_seeds(10 ** 12, 10 ** 9 - 1, 2)[1:]      # O(1): no walk from 0
    one, two = shape_seeds(7, 0, 64), shape_seeds(8, 0, 64)
    assert len(set(one)) == 64 and len(set(two)) == 64 and not set(one) & set(two)
    with pytest.raises(ValueError):
        shape_seeds(7, -1, 2)


def test_sample_keys_and_key_words():
    from lion_amd.chain import key_words, sample_keys
    assert sample_keys([1, -1, 2 ** 64 + 3], 3) == [1, 2 ** 64 - 1, 3]
    assert sample_keys(torch.tensor([5, -2], dtype=torch.int64), 2) == [5, 2 ** 64 - 2]
    assert sample_keys(np.array([5, 6]), 2) == [5, 6]
    for bad, n in (([1, 2], 3), ([], 1), (torch.arange(4), 3), (7, 1)):
        with pytest.raises(ValueError):
            sample_keys(bad, n)
    w = key_words([0x1122334455667788, 2 ** 64 - 1])
    assert w.dtype == torch.int32 and tuple(w.shape) == (2, 2)
    assert w.numpy().view(np.uint32).tolist() == [[0x55667788, 0x11223344], [0xFFFFFFFF, 0xFFFFFFFF]]


def test_split_sample_seeds_order():
    from lion_amd.chain import split_seed
    from lion_amd.editing import SUBKEYS
    from lion_amd.sampling import SAMPLE_SUBKEYS, split_sample_seeds
    assert SAMPLE_SUBKEYS == ("start_global", "chain_global", "start_local", "chain_local")
    assert SUBKEYS == ("vae", "diffuse_global", "chain_global", "diffuse_local", "chain_local")
    sub = split_sample_seeds([3, 2 ** 64 + 9], 2)
    assert sub["seeds"] == [3, 9] and set(sub) == set(SAMPLE_SUBKEYS) | {"seeds"}
    for j, name in enumerate(SAMPLE_SUBKEYS):
        assert sub[name] == [split_seed(3, 4)[j], split_seed(9, 4)[j]]


# ---- refusals: ValueError before the "no CPU path" error, on CPU tensors ---------------------------------------------------------
def _diffusion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    return DiffusionDiscretized(None, None, released_prior_cfg(), device="cpu")


class _Vae:
    def latent_shape(self):
        return [[128, 1, 1], [8192, 1, 1]]


def test_sampler_refusals_come_before_any_launch():
    d = _diffusion()
    model, B, shape = torch.nn.Identity(), 2, [128, 1, 1]
    x = torch.zeros([B] + shape)
    noise = (x, [x] * 4)
    bad = [
        lambda: d.run_denoising_diffusion(model, B, shape, seeds=[1]),
        lambda: d.run_denoising_diffusion(model, B, shape, seeds=[1, 2, 3]),
        lambda: d.run_denoising_diffusion(model, B, shape, seeds=[1, 2], given_noise=noise),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, 4, x, seeds=[1]),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, 4, x, seeds=[1, 2], seed=5),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, 4, x, seeds=[1, 2], given_noise=noise),
        lambda: d.run_ddim(model, B, shape, ddim_step=4, seeds=torch.tensor([1, 2, 3])),
        lambda: d.run_ddim(model, B, shape, ddim_step=4, seeds=[1, 2], given_noise=noise),
        lambda: d.run_ddim(model, B, shape, ddim_step=4, seeds=[1, 2], noise='cpu'),
        lambda: d.run_dpm_solver(model, B, shape, steps=4, stochastic=True, seeds=[1]),
        lambda: d.run_dpm_solver(model, B, shape, steps=4, stochastic=True, seeds=[1, 2], seed=5),
        lambda: d.run_dpm_solver(model, B, shape, steps=4, seeds=[1, 2], seed=5),
        lambda: d.diffuse(x, 10, seeds=[1]),
        lambda: d.diffuse(x, 10, seeds=[1, 2], seed=5),
        lambda: d.diffuse(x, 10, seeds=[1, 2], noise=x),
    ]
    for f in bad:
        with pytest.raises(ValueError, match="seeds"):
            f()
    good = [
        lambda: d.run_denoising_diffusion(model, B, shape, seeds=[1, 2]),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, 4, x, seeds=[1, 2]),
        lambda: d.run_ddim(model, B, shape, ddim_step=4, seeds=[1, 2]),
        lambda: d.run_dpm_solver(model, B, shape, steps=4, stochastic=True, seeds=[1, 2]),
        lambda: d.diffuse(x, 10, seeds=[1, 2]),
    ]
    for f in good:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_driver_refusals_come_before_any_launch():
    from lion_amd.editing import diffuse_denoise
    from lion_amd.sampling import generate_samples_vada_2prior
    d, vae = _diffusion(), _Vae()
    dae = [torch.nn.Identity(), torch.nn.Identity()]
    sh = vae.latent_shape()
    for kw in (dict(seeds=[1]), dict(seeds=[1, 2, 3]), dict(seeds=[1, 2], noise='cpu'), dict(seeds=[1, 2], ode_sample=1),
               dict(seeds=[1, 2], given_noise=[None, None])):
        with pytest.raises(ValueError, match="seeds"):
            generate_samples_vada_2prior(sh, dae, d, vae, 2, dpm_step=4, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        generate_samples_vada_2prior(sh, dae, d, vae, 2, dpm_step=4, seeds=[1, 2])
    x = torch.zeros(2, 2048, 3)
    for kw in (dict(seeds=[1]), dict(seeds=[1, 2], seed=5)):
        with pytest.raises(ValueError, match="seeds"):
            diffuse_denoise(vae, dae, d, x, 200, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffuse_denoise(vae, dae, d, x, 200, seeds=[1, 2])


def test_keyed_chain_construction_refusals():
    from lion_amd import chain
    for mode in (chain.DPMPP, chain.ENCODE):
        with pytest.raises(ValueError, match="keyed"):
            chain.GraphedChain(torch.nn.Identity(), 2, [128, 1, 1], None, None, "cpu", mode, 8, keyed=True)
    with pytest.raises(ValueError, match="multiple of 4"):
        chain.GraphedChain(torch.nn.Identity(), 2, [6, 1, 1], None, None, "cpu", chain.DDIM, 8, keyed=True)
    assert chain.KEYED_MODES == (chain.DDIM, chain.DDPM, chain.SDE_DPMPP)
