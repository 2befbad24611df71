"""CPU suite of diffuse-denoise (lion_amd/editing.py, DiffusionDiscretized.diffuse / run_denoising_diffusion_from_t /
ddpm_table, lion_chain_diffuse): the C ABI agrees across header, ctypes table and library and refuses bad arguments on the
host; the tail's schedule table is the whole chain's, cut; out-of-range steps are ValueErrors; CPU tensors are refused."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _diffusion(T=1000):
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    cfg = released_prior_cfg()
    cfg.ddpm.num_steps = T
    return DiffusionDiscretized(None, None, cfg, device="cpu")


def test_chain_diffuse_is_declared_bound_and_exported():
    from lion_amd import _lib
    txt = abi_check.header()
    found = re.findall(r"\bint\s+lion_chain_diffuse\s*\(([^)]*)\)\s*;", txt)
    assert len(found) == 1, "lion_chain_diffuse: one prototype in include/lion_hip.h"
    params = [" ".join(p.split()) for p in found[0].split(",")]
    kinds = ["*" if "*" in p else [w for w in re.findall(r"\w+", p) if w != "const"][0] for p in params]
    assert kinds == ["*", "*", "size_t", "float", "float", "*", "uint32_t", "*", "*", "lionStream_t"]
    ctype = {"*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32,
             "lionStream_t": ctypes.c_void_p}
    res, args = _lib.SIGNATURES["lion_chain_diffuse"]
    assert res is ctypes.c_int and len(args) == len(kinds)
    assert all(a is ctype[k] for a, k in zip(args, kinds))
    abi_check.declared_bound_and_exported(["lion_chain_diffuse"])
    # the step word of the draw's counter is stated in the header, and no chain step can have it (a step index is an int)
    word = re.search(r"#define\s+LION_DIFFUSE_STEP_WORD\s+(0x[0-9A-Fa-f]+)u?\b", open(os.path.join(ROOT, "include", "lion_hip.h")).read())
    assert word and int(word.group(1), 16) > 0x7FFFFFFF


def test_chain_diffuse_refuses_bad_arguments_on_the_host():
    """-1 before any launch (no GPU here: a launch would be a HIP error, a positive code)"""
    from lion_amd import _lib
    fn = _lib.load().lion_chain_diffuse
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert fn(None, p, 8, 1.0, 0.5, p, 1, p, None, None) == -1          # x0
    assert fn(p, p, 8, 1.0, 0.5, p, 1, None, None, None) == -1          # out
    assert fn(p, None, 8, 1.0, 0.5, None, 1, p, None, None) == -1       # no noise and no seed to draw it with
    assert fn(p, p, 0, 1.0, 0.5, p, 1, p, None, None) == -1             # numel


def _parent_table(d, temp=1.0, noise_scale=None):
    """the loop run_denoising_diffusion had before ddpm_table existed, from ddpm_coefficients"""
    T = d._diffusion_steps
    table = np.zeros((T, 8), np.float32)
    for i, t in enumerate(reversed(range(T))):
        is0, k_outer, k_a, k_b, scale = d.ddpm_coefficients(t)
        if noise_scale is not None and not is0:
            scale = float(noise_scale(t))
        table[i] = (t + 1, k_outer, k_a, k_b, scale, temp, 1.0 if is0 else 0.0, 0.0)
    return table


@pytest.mark.parametrize("T", [1000, 12])
def test_ddpm_table_is_the_whole_chains_table_and_its_tails(T):
    d = _diffusion(T)
    full = d.ddpm_table(T)
    assert full.dtype == np.float32 and full.shape == (T, 8)
    assert full.tobytes() == _parent_table(d).tobytes()
    scale = lambda t: 0.01 + 1e-5 * t
    assert d.ddpm_table(T, 0.7, scale).tobytes() == _parent_table(d, 0.7, scale).tobytes()
    for k in (1, 2, T - 1):
        tail = d.ddpm_table(k)
        assert tail.shape == (k, 8) and tail.tobytes() == full[T - k:].tobytes()
        assert tail[0, 0] == k and tail[-1, 0] == 1 and tail[-1, 6] == 1.0
    for bad in (0, -1, T + 1):
        with pytest.raises(ValueError):
            d.ddpm_table(bad)


def test_out_of_range_steps_are_value_errors():
    d = _diffusion(12)
    x = torch.zeros(2, 4, 1, 1)
    for t in (-1, 12):
        with pytest.raises(ValueError):
            d.diffuse(x, t)
    for ts in (-1, 13):
        with pytest.raises(ValueError):
            d.run_denoising_diffusion_from_t(None, 2, [4, 1, 1], ts, x)
    from lion_amd.editing import diffuse_denoise
    for ts in (-1, 12, (0, 12), (1, 2, 3)):
        with pytest.raises(ValueError):
            diffuse_denoise(None, [None, None], d, torch.zeros(2, 16, 3), ts)


def test_time_start_zero_needs_no_device():
    d = _diffusion(12)
    x = torch.randn(2, 4, 1, 1)
    out, states = d.run_denoising_diffusion_from_t(None, 2, [4, 1, 1], 0, x)
    assert out is x and states == []


def test_no_cpu_path():
    from lion_amd import diffusion_ops
    from lion_amd.editing import diffuse_denoise
    d = _diffusion(12)
    x = torch.zeros(2, 4, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffusion_ops.diffuse(x, 0.9, 0.1, seed=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.diffuse(x, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.diffuse(x, 3, noise=torch.zeros_like(x))
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.run_denoising_diffusion_from_t(None, 2, [4, 1, 1], 3, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffuse_denoise(None, [None, None], d, torch.zeros(2, 16, 3), 3)
