"""Fused denoiser-step updates (D1) over the C ABI: lion_ddim_update / lion_ddpm_update, the multistep solver
step lion_dpmpp_update and its stochastic form lion_sde_dpmpp_update, the deterministic encoder's row lion_ddim_encode_update,
the forward-process draw lion_chain_diffuse, and the per-sample-key draws lion_philox_normal_keyed / lion_chain_diffuse_keyed /
lion_chain_diffuse_keyed_at."""
import numpy as np
import torch

from . import _lib
from .chain import key_words, sample_keys

__all__ = ["ddim_update", "ddpm_update", "dpmpp_update", "sde_dpmpp_update", "ddim_encode_update", "diffuse",
           "diffuse_at", "philox_normal_keyed"]


def ddim_update(x, eps, z, s, c, sigma, out=None):
    """out = x*s + (c*eps + sigma*z)   (utils/diffusion_pvd.py:451-467); z may be None if sigma==0."""
    _lib.require_cuda(x, eps, z)
    out = torch.empty_like(x) if out is None else out
    _lib.call("lion_ddim_update", x, eps, z, x.numel(), float(s), float(c), float(sigma), out)
    return out


def seed_words(seed, device):
    """the 64-bit Philox key as the two 32-bit words (lo, hi) the chain kernels read from device memory"""
    words = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(words).to(device)


def _device_keys(keys, num_samples, device, who):
    """per-sample keys as the device words the keyed kernels read: an int32[B, 2] device tensor passes (a loop uploads its keys
    once), anything else goes through chain.sample_keys (ValueError on a wrong count)"""
    if isinstance(keys, torch.Tensor) and keys.dtype == torch.int32 and keys.dim() == 2:
        if tuple(keys.shape) != (num_samples, 2):
            raise ValueError(f"{who}: key words {tuple(keys.shape)} for {num_samples} samples")
        return keys
    return key_words(sample_keys(keys, num_samples, who), device)


def philox_normal_keyed(keys, num_samples, shape, step, stream_id=0, device="cuda", out=None):
    """z [num_samples] + shape with z[b] ~ N(0, 1) drawn by the chain's Philox generator under the 64-bit key keys[b] at counter
    (quad within the sample, `step`, stream_id) (lion_philox_normal_keyed): what a keyed chain draws for sample b at that step
    word, and what the single-seed kernels draw for ONE sample of this shape under seed keys[b] -- whatever num_samples, b and
    the other keys are.  keys: num_samples ints (a sequence or tensor), or their device words (chain.key_words).  The
    elements of one sample must be a multiple of 4.  step = chain.START_STEP_WORD is the start latent of a keyed chain."""
    size = [int(num_samples)] + list(shape)
    n = int(np.prod(shape))
    if n <= 0 or n % 4 != 0:
        raise ValueError(f"philox_normal_keyed: {n} elements per sample, must be a positive multiple of 4")
    out = torch.empty(size, device=device) if out is None else out
    _lib.require_cuda(out)
    words = _device_keys(keys, num_samples, out.device, "philox_normal_keyed")
    _lib.call("lion_philox_normal_keyed", words, int(num_samples), n, int(step), int(stream_id), out)
    return out


def diffuse(x0, m, s, noise=None, seed=None, stream_id=1, out=None, return_noise=False, seeds=None):
    """out = m*x0 + s*z, the forward-process draw (utils/diffusion_pvd.py:105-113).  z = `noise` if given, else N(0, 1) drawn
    in the kernel by the chain's Philox generator under the 64-bit `seed` (lion_chain_diffuse; stream_id 1 keeps the draw apart
    from every step's noise of a chain run under the same seed, which uses stream 0).  out may be x0.
    seeds (instead of noise / seed): one key per sample x0[b]; sample b's z is drawn under seeds[b] at counters within the sample
    (lion_chain_diffuse_keyed), so it does not depend on the batch it sits in."""
    if seeds is not None:
        if noise is not None or seed is not None:
            raise ValueError("diffuse: seeds excludes noise and seed")
        B = x0.shape[0]
        words = _device_keys(seeds, B, x0.device, "diffuse")
        _lib.require_cuda(x0, out)
        n = x0.numel() // max(B, 1)
        if n <= 0 or n % 4 != 0:
            raise ValueError(f"diffuse: {n} elements per sample, keyed noise needs a positive multiple of 4")
        out = torch.empty_like(x0) if out is None else out
        z_out = torch.empty_like(x0) if return_noise else None
        _lib.call("lion_chain_diffuse_keyed", x0, B, n, float(m), float(s), words, int(stream_id), out, z_out)
        return (out, z_out) if return_noise else out
    _lib.require_cuda(x0, noise, out)
    if noise is None and seed is None:
        raise ValueError("diffuse: either noise or seed")
    if noise is not None and noise.shape != x0.shape:
        raise ValueError(f"diffuse: noise {tuple(noise.shape)} for x0 {tuple(x0.shape)}")
    out = torch.empty_like(x0) if out is None else out
    z_out = torch.empty_like(x0) if return_noise else None
    _lib.call("lion_chain_diffuse", x0, noise, x0.numel(), float(m), float(s),
              None if noise is not None else seed_words(int(seed), x0.device), int(stream_id), out, z_out)
    return (out, z_out) if return_noise else out


def diffuse_at(x0, ms, seeds, stream_id=1, out=None, return_noise=False):
    """diffuse(seeds=...) with its two scalars per sample (lion_chain_diffuse_keyed_at): ms is B pairs (m_b, s_b) of host floats,
    and sample b is diffuse's keyed draw with (m_b, s_b) bit for bit.  A sample with (1, 0) is copied bit for bit and draws
    nothing; its z is 0.  out may be x0."""
    B = x0.shape[0]
    pairs = np.asarray(ms, dtype=np.float32)
    if pairs.shape != (B, 2):
        raise ValueError(f"diffuse_at: ms {pairs.shape} for {B} samples")
    _lib.require_cuda(x0, out)
    words = _device_keys(seeds, B, x0.device, "diffuse_at")
    n = x0.numel() // max(B, 1)
    if n <= 0 or n % 4 != 0:
        raise ValueError(f"diffuse_at: {n} elements per sample, keyed noise needs a positive multiple of 4")
    out = torch.empty_like(x0) if out is None else out
    z_out = torch.empty_like(x0) if return_noise else None
    _lib.call("lion_chain_diffuse_keyed_at", x0, B, n, torch.from_numpy(pairs).to(x0.device), words, int(stream_id), out, z_out)
    return (out, z_out) if return_noise else out


def dpmpp_update(x, eps, hist, a0, a1, a2, a3, a4, a5, out=None, hist_out=None):
    """One DPM-Solver++(2M) step (lion_dpmpp_update; coefficients: DiffusionDiscretized.dpm_solver_table):
    x0 = a0*(x - a1*eps);  D = a4*x0 (+ a5*hist where a5 != 0);  out = a2*x + a3*D;  hist_out = x0.  hist, the previous step's
    x0, is not read when a5 == 0 and may then be None.  out may be x and hist_out may be hist.  Returns (out, hist_out)."""
    _lib.require_cuda(x, eps, hist, out, hist_out)
    if hist is None and float(a5) != 0.0:
        raise ValueError("dpmpp_update: a second-order row (a5 != 0) needs hist")
    out = torch.empty_like(x) if out is None else out
    hist_out = torch.empty_like(x) if hist_out is None else hist_out
    _lib.call("lion_dpmpp_update", x, eps, hist, x.numel(), float(a0), float(a1), float(a2), float(a3), float(a4), float(a5),
              out, hist_out)
    return out, hist_out


def sde_dpmpp_update(x, eps, hist, a0, a1, a2, a3, a4, a5, a6, noise=None, seed=None, step=0, stream_id=0, out=None,
                     hist_out=None, return_noise=False):
    """One SDE-DPM-Solver++(2M) step (lion_sde_dpmpp_update; coefficients: dpm_solver_table(stochastic=True), a6 its
    column 7): dpmpp_update's x0, D and hist_out, then out = (a2*x + a3*D) + a6*z where a6 != 0, else out = a2*x + a3*D.
    z = `noise` if given, else N(0, 1) drawn in the kernel by the chain's Philox generator at counter (element/4, `step`,
    stream_id) under `seed`: a 64-bit int, or the device words of seed_words() (a loop uploads them once) -- what step `step`
    of a captured chain (chain.SDE_DPMPP) under that seed draws.  Neither is needed when a6 == 0: nothing is drawn.
    return_noise: (out, hist_out, z), z the noise that was used, zeros when a6 == 0."""
    _lib.require_cuda(x, eps, hist, noise, out, hist_out)
    if hist is None and float(a5) != 0.0:
        raise ValueError("sde_dpmpp_update: a second-order row (a5 != 0) needs hist")
    if noise is None and seed is None and float(a6) != 0.0:
        raise ValueError("sde_dpmpp_update: a noisy row (a6 != 0) needs noise or seed")
    if noise is not None and noise.shape != x.shape:
        raise ValueError(f"sde_dpmpp_update: noise {tuple(noise.shape)} for x {tuple(x.shape)}")
    out = torch.empty_like(x) if out is None else out
    hist_out = torch.empty_like(x) if hist_out is None else hist_out
    z_out = torch.empty_like(x) if return_noise else None
    if noise is not None or seed is None:
        words = None
    else:
        words = seed if isinstance(seed, torch.Tensor) else seed_words(int(seed), x.device)
    _lib.call("lion_sde_dpmpp_update", x, eps, hist, noise, x.numel(), float(a0), float(a1), float(a2), float(a3), float(a4),
              float(a5), float(a6), words, int(step), int(stream_id), out, hist_out, z_out)
    return (out, hist_out, z_out) if return_noise else (out, hist_out)


def ddim_encode_update(base, eps, s, c, commit, out=None, base_out=None):
    """One row of the refined DDIM inversion (lion_ddim_encode_update; coefficients: DiffusionDiscretized.encode_table):
    out = s*base + c*eps, and base_out = out where `commit` (the last row of a leg).  base_out is neither written nor allocated
    without commit.  out may be base or the tensor the model read, base_out may be base.  Returns (out, base_out), base_out None
    where nothing was committed and none was given."""
    _lib.require_cuda(base, eps, out, base_out)
    if eps.shape != base.shape:
        raise ValueError(f"ddim_encode_update: eps {tuple(eps.shape)} for base {tuple(base.shape)}")
    out = torch.empty_like(base) if out is None else out
    if commit and base_out is None:
        base_out = torch.empty_like(base)
    _lib.call("lion_ddim_encode_update", base, eps, base.numel(), float(s), float(c), 1.0 if commit else 0.0, out, base_out)
    return out, base_out


def ddpm_update(x, eps, z, t_is_zero, k_outer, k_a, k_b, scale, temp, out=None):
    """DDPM ancestral step (utils/diffusion_pvd.py:283-296, :475-486)."""
    _lib.require_cuda(x, eps, z)
    out = torch.empty_like(x) if out is None else out
    _lib.call("lion_ddpm_update", x, eps, z, x.numel(), int(bool(t_is_zero)), float(k_outer), float(k_a), float(k_b),
              float(scale), float(temp), out)
    return out
