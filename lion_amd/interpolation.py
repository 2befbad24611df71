"""Shape interpolation in the ODE's noise space (the paper's interpolation results): the noise-mixing rules of the
reference's ``trainers/interpolate_latent.py:24-59``, its ``generate_samples`` (:120-170), and encode -> interpolate ->
decode as in ``trainers/encode_interp_interp.py:229-293``.  Every latent is [B, D, 1, 1]; row 0 and row B-1 are the two
ends, rows 1..B-2 are replaced (in place, as the reference does) and the ends are left untouched.
On the discrete diffusion the same recipe runs on its few-step pair instead of the ODE: ``encode_noise`` (refined DDIM inversion,
DiffusionDiscretized.run_ddim_forward) and ``decode_noise`` (the order-1 solver over the same schedule)."""
from __future__ import annotations

import math

import torch


def _fill(noise, rule):
    a, b = noise[0].clone(), noise[-1].clone()
    B = noise.shape[0]
    for k in range(1, B - 1):
        noise[k] = rule(k / B, a, b)      # p = k / B: 1/B .. (B-2)/B
    return noise


def interpolate_noise(noise):
    """variance-preserving: sqrt(p) * end + sqrt(1 - p) * start"""
    return _fill(noise, lambda p, a, b: math.sqrt(p) * b + math.sqrt(1 - p) * a)


def linear_interpolate_noise(noise):
    """p * end + (1 - p) * start"""
    return _fill(noise, lambda p, a, b: p * b + (1 - p) * a)


def subtract_noise(noise):
    """latent arithmetic on a batch of at least 16: rows 0..5 become n12, n15, n9, n10, n9 + (n12 - n15),
    n10 + (n12 - n15)"""
    if noise.shape[0] < 16:
        raise ValueError("subtract_noise needs at least 16 rows")
    a, b, c, d = (noise[i].clone() for i in (12, 15, 9, 10))
    delta = a - b
    noise[:6] = torch.stack([a, b, c, d, c + delta, d + delta])
    return noise


def freeze_noise(noise):
    """every row takes row 0 (the 'freeze' mode: one local latent for all samples)"""
    noise[1:] = noise[0]
    return noise


MODES = {'interpolate': interpolate_noise, 'linear_interpolate': linear_interpolate_noise,
         'subtract': subtract_noise, 'freeze': freeze_noise}


@torch.no_grad()
def generate_samples(shape, dae, diffusion, vae, num_samples, enable_autocast=False, ode_eps=1e-5, ode_solver_tol=1e-5,
                     temp=1.0, generate_mode_global='interpolate', generate_mode_local='freeze', graph=True):
    """interpolate_latent.py:120-170: fresh noise per prior, mixed by the prior's mode, integrated by the PF-ODE, the
    global latent conditioning the local prior (through vae.global2style, as the samplers do), decoded.
    Returns (points [B, N, 3], {'nfe': [per prior], 'seconds': [per prior]})."""
    condition_input = None
    latents, nfe, seconds = [], [], []
    for i, mode in enumerate((generate_mode_global, generate_mode_local)[:len(dae)]):
        noise = torch.randn(size=[num_samples] + list(shape[i]), device=diffusion.device)
        noise = MODES[mode](noise) if mode in MODES else noise
        eps, n, s = diffusion.sample_model_ode(dae[i], num_samples, shape[i], ode_eps, ode_solver_tol, enable_autocast,
                                               temp, noise, condition_input=condition_input, graph=graph)
        condition_input = vae.global2style(eps) if i == 0 else eps
        latents.append(eps)
        nfe.append(n)
        seconds.append(s)
    eps = vae.compose_eps(latents)
    points = vae.sample(num_samples=num_samples, decomposed_eps=vae.decompose_eps(eps.view(num_samples, -1)))
    return points, {'nfe': nfe, 'seconds': seconds}


def _vae_latents(vae, clouds, latents):
    """the two VAE latents as [B] + latent_shape tensors, from the clouds or from the given flat ``latents``"""
    shapes = vae.latent_shape()
    if latents is None:
        latents = vae.decompose_eps(vae.encode(clouds)[0])
    B = latents[0].shape[0]
    return [latents[i].reshape([B] + list(shapes[i])).contiguous() for i in range(2)]


@torch.no_grad()
def encode_noise(vae, dae, diffusion, clouds=None, latents=None, steps=20, refine=1, skip_type='logsnr', graph=True):
    """clouds [B, N, 3] (or ``latents`` [global [B, Dg], local [B, Dl]]) -> [z_global, z_local], the noise of each prior that
    ``decode_noise`` maps back: ``DiffusionDiscretized.run_ddim_forward`` per prior over ``solver_schedule(steps, skip_type)``
    with ``refine`` corrector evaluations per leg, the local prior conditioned on vae.global2style of the encoded global
    latent, as the ODE path of encode_interpolate does."""
    if clouds is None and latents is None:
        raise ValueError("encode_noise: either clouds or latents")
    eg, el = _vae_latents(vae, clouds, latents)
    zg, _ = diffusion.run_ddim_forward(dae[0], eg, steps, skip_type, refine=refine, graph=graph)
    zl, _ = diffusion.run_ddim_forward(dae[1], el, steps, skip_type, condition_input=vae.global2style(eg), refine=refine,
                                       graph=graph)
    return [zg, zl]


@torch.no_grad()
def decode_noise(vae, dae, diffusion, noise, steps=20, skip_type='logsnr', graph=True):
    """[z_global, z_local] -> the latents [global, local] ([B] + latent_shape each): the order-1 solver
    (run_dpm_solver(order=1), DDIM with kappa = 0) per prior over the schedule encode_noise walked, the local prior conditioned
    on vae.global2style of the DECODED global latent.  vae.sample(num_samples=B, decomposed_eps=[g.view(B, -1), l.view(B, -1)])
    turns them into points."""
    zg, zl = noise
    B = zg.shape[0]
    shapes = vae.latent_shape()
    g, _ = diffusion.run_dpm_solver(dae[0], B, shapes[0], steps=steps, order=1, skip_type=skip_type, x_noisy=zg,
                                    keep_trajectory=False, graph=graph)
    l, _ = diffusion.run_dpm_solver(dae[1], B, shapes[1], steps=steps, order=1, skip_type=skip_type, x_noisy=zl,
                                    condition_input=vae.global2style(g), keep_trajectory=False, graph=graph)
    return [g, l]


@torch.no_grad()
def encode_interpolate(vae, dae, diffusion, clouds, ode_eps=1e-5, ode_solver_tol=1e-5, temp=1.0, mode='interpolate',
                       latents=None, graph=True, steps=20, refine=1, skip_type='logsnr'):
    """clouds [B, N, 3] -> VAE latents (or the given ``latents`` [global [B, Dg], local [B, Dl]]) -> noise by the ODE
    (compute_ode_nll) per prior -> rows 1..B-2 interpolated between the first and the last cloud's noise -> back by the
    ODE (sample_model_ode) -> decoded.  Returns (points [B, N, 3], info) with info['latents'] the encoded latents and
    info['nfe'] the evaluations of the four solves.
    With a DiffusionDiscretized the two maps are its few-step pair instead: run_ddim_forward(steps, skip_type, refine) into
    the noise and run_dpm_solver(order=1) over the same schedule back (encode_noise / decode_noise, prior by prior);
    ode_eps, ode_solver_tol and temp are unused there, the same info keys come back, info['nfe'] holds the four replay
    counts -- legs*(1 + refine) per encoder, legs per decoder -- and info['noise'] the mixed noise [global, local]."""
    from .diffusion import DiffusionDiscretized
    if isinstance(diffusion, DiffusionDiscretized):
        return _encode_interpolate_discrete(vae, dae, diffusion, clouds, mode, latents, graph, steps, refine, skip_type)
    B = clouds.shape[0]
    shapes = vae.latent_shape()
    if latents is None:
        latents = vae.decompose_eps(vae.encode(clouds)[0])
    eg, el = (latents[i].reshape([B] + list(shapes[i])).contiguous() for i in range(2))
    mix = MODES[mode]
    nfe = []
    zg = mix(diffusion.compute_ode_nll(dae[0], eg, ode_eps, ode_solver_tol, graph=graph).contiguous())
    nfe.append(diffusion.last_ode["nfe"])
    g_new, n, _ = diffusion.sample_model_ode(dae[0], B, shapes[0], ode_eps, ode_solver_tol, False, temp, zg,
                                             graph=graph)
    nfe.append(n)
    zl = mix(diffusion.compute_ode_nll(dae[1], el, ode_eps, ode_solver_tol, condition_input=vae.global2style(eg),
                                       graph=graph).contiguous())
    nfe.append(diffusion.last_ode["nfe"])
    l_new, n, _ = diffusion.sample_model_ode(dae[1], B, shapes[1], ode_eps, ode_solver_tol, False, temp, zl,
                                             condition_input=vae.global2style(g_new), graph=graph)
    nfe.append(n)
    points = vae.sample(num_samples=B, decomposed_eps=[g_new.view(B, -1), l_new.view(B, -1)])
    return points, {'latents': [eg, el], 'nfe': nfe, 'interpolated': [g_new, l_new]}


def _encode_interpolate_discrete(vae, dae, diffusion, clouds, mode, latents, graph, steps, refine, skip_type):
    """encode_interpolate on the discrete diffusion: per prior, encoder -> MODES[mode] -> order-1 decoder; the solves in the ODE
    path's order (global in, global out, local in, local out)"""
    eg, el = _vae_latents(vae, clouds, latents)
    B = eg.shape[0]
    shapes = vae.latent_shape()
    mix = MODES[mode]
    legs = len(diffusion.solver_schedule(steps, skip_type))
    back = dict(steps=steps, order=1, skip_type=skip_type, keep_trajectory=False, graph=graph)
    zg = mix(diffusion.run_ddim_forward(dae[0], eg, steps, skip_type, refine=refine, graph=graph)[0])
    g_new, _ = diffusion.run_dpm_solver(dae[0], B, shapes[0], x_noisy=zg, **back)
    zl = mix(diffusion.run_ddim_forward(dae[1], el, steps, skip_type, condition_input=vae.global2style(eg), refine=refine,
                                        graph=graph)[0])
    l_new, _ = diffusion.run_dpm_solver(dae[1], B, shapes[1], x_noisy=zl, condition_input=vae.global2style(g_new), **back)
    points = vae.sample(num_samples=B, decomposed_eps=[g_new.view(B, -1), l_new.view(B, -1)])
    return points, {'latents': [eg, el], 'nfe': [legs * (1 + refine), legs, legs * (1 + refine), legs],
                    'interpolated': [g_new, l_new], 'noise': [zg, zl]}
