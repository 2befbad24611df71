"""Two-prior sampling driver -- mirror of ``generate_samples_vada_2prior``
(trainers/train_2prior.py:50-127): global prior -> style -> local prior -> VAE decode, and the
multi-GPU sharding of a generation job (independent shapes, no data-path collective; the reference
splits iterations over ranks but reseeds every rank identically, base_trainer.py:447-463 -- here either
every shape of the job has a seed of its own, ``shape_seeds``, whatever rank draws it, or the rank is
folded into the seed, ``rank_seed``)."""
from __future__ import annotations

import torch

from . import chain as _chain
from . import diffusion_ops

# the keys one shape's seed is split into (chain.split_seed, in this order): the start latent and the chain of each prior
SAMPLE_SUBKEYS = ("start_global", "chain_global", "start_local", "chain_local")


def split_sample_seeds(seeds, num_samples, names=SAMPLE_SUBKEYS, who="seeds"):
    """per-shape seeds -> {'seeds': [s_0, ...], name: [the sub-key `name` of s_0, ...], ...}: shape b's seed is split with
    SplitMix64 (chain.split_seed) into len(names) keys, in the order of `names`.  ValueError on a wrong count."""
    keys = _chain.sample_keys(seeds, num_samples, who)
    split = [_chain.split_seed(k, len(names)) for k in keys]
    out = {name: [sp[j] for sp in split] for j, name in enumerate(names)}
    out["seeds"] = keys
    return out


@torch.no_grad()
def generate_samples_vada_2prior(shape, dae, diffusion, vae, num_samples, enable_autocast=False,
                                 temp=1.0, ddim_step=0, clip_feat=None, ddim_skip_type='uniform',
                                 ddim_kappa=1.0, noise='device', step_callback=None, graph=True, given_noise=None,
                                 state_hook=None, ode_sample=0, ode_eps=1e-5, ode_solver_tol=1e-5, start_noise=None,
                                 conv_precision="fp32", dpm_step=0, dpm_order=2, dpm_skip_type='logsnr',
                                 dpm_stochastic=False, seeds=None):
    """shape: vae.latent_shape(); dae: [global prior, local prior].  Returns (points [B,N,3], info).
    graph=True (default): every chain is replayed from one captured hipGraph per prior (lion_amd/chain.py);
    graph=False: the eager per-step loop; noise='cpu' draws the start and every step's noise from torch's CPU generator
    (one seed = one chain on any device: what the sampler-level parity test runs on the GPU and on the host);
    given_noise = [(start, [z per step]) per prior] replays recorded draws through the eager loop (DDIM only).
    state_hook(prior_index, step_index, x): may overwrite a chain's latent in place before a model evaluation (DDIM only;
    device-side launches, no host synchronisation).
    ode_sample=1 (train_2prior.py:58-75): each prior integrates the probability-flow ODE of a continuous diffusion
    (diffusion_continuous.DiffusionVPSDE) from t = 1 to ode_eps at tolerance ode_solver_tol, starting from
    start_noise[i] if given (else fresh N(0, I) draws); info['nfe'] lists the evaluations per prior.
    dpm_step > 0: each prior runs DPM-Solver++(2M) with at most dpm_step evaluations (DiffusionDiscretized.run_dpm_solver,
    order dpm_order, spacing dpm_skip_type): deterministic after the start draw; state_hook applies, noise / given_noise do
    not.  dpm_stochastic=True: the stochastic form of that solver (SDE-DPM-Solver++(2M), run_dpm_solver(stochastic=True)):
    fresh noise enters at every step but the last, from the chain's generator under a key drawn with chain.draw_seed().
    Precedence: ode_sample == 1, then dpm_step > 0, then ddim_step > 0, then the ancestral chain.
    conv_precision="half": the supported reduced-precision mode -- the denoiser evaluations of every chain run their voxel
    convolutions at r = 16 / 32 with one fp16 product per operand pair, inside the captured chain (conv_ops.PRECISION,
    DESIGN.md 4.3); the VAE decode stays fp32-accurate.  enable_autocast is unrelated and keeps its behaviour (it leaves
    the captured chain for the vendor libraries).
    seeds: num_samples ints (a sequence or an int64 tensor, each taken mod 2^64), one per shape: shape b is addressed by
    seeds[b].  Each seed is split (SplitMix64) into SAMPLE_SUBKEYS = (start_global, chain_global, start_local, chain_local);
    a prior's start latent is the keyed draw under start_* at LION_START_STEP_WORD and its chain runs under chain_* (the
    samplers' `seeds`).  No draw of the call touches torch's global generators, and the NOISE a shape receives depends on its
    seed alone -- not on num_samples, its position, or its batchmates -- so a shape can be regenerated, or run under another
    sampler from the same start.  The resulting points are promised bit-equal only at equal num_samples: other batch sizes
    select other kernel plans (the split 1x1 convolution from B*L >= 8192 columns, the conv tile plans).  info['seeds']
    reports the seeds and their sub-keys.  ValueError before any launch: len(seeds) != num_samples, seeds with given_noise,
    with noise='cpu', or with ode_sample=1 (the ODE path has no keyed form)."""
    sub = None
    if seeds is not None:
        sub = split_sample_seeds(seeds, num_samples, who="generate_samples_vada_2prior")
        if given_noise is not None or noise == 'cpu' or ode_sample == 1:
            raise ValueError("generate_samples_vada_2prior: seeds cannot be combined with given_noise, noise='cpu' or ode_sample=1")
    keyed = [{}, {}] if sub is None else [
        dict(seeds=sub["chain_" + w], x_noisy=diffusion_ops.philox_normal_keyed(
            sub["start_" + w], num_samples, shape[i], _chain.START_STEP_WORD, device=diffusion.device))
        for i, w in enumerate(("global", "local"))]
    condition_input = None
    all_eps = []
    nfes = []
    for i in range(len(dae)):
        if ode_sample == 1:
            if not hasattr(diffusion, 'sample_model_ode'):
                raise TypeError('ODE-based sampling requires a continuous diffusion (diffusion_continuous.make_diffusion)')
            eps, nfe, _ = diffusion.sample_model_ode(dae[i], num_samples, shape[i], ode_eps, ode_solver_tol,
                                                     enable_autocast, temp,
                                                     None if start_noise is None else start_noise[i],
                                                     condition_input=condition_input, clip_feat=clip_feat, graph=graph,
                                                     conv_precision=conv_precision)
            nfes.append(nfe)
        elif dpm_step > 0:
            eps, _ = diffusion.run_dpm_solver(dae[i], num_samples, shape[i], steps=dpm_step, order=dpm_order,
                                              skip_type=dpm_skip_type, condition_input=condition_input, clip_feat=clip_feat,
                                              enable_autocast=enable_autocast, keep_trajectory=False, graph=graph,
                                              state_hook=None if state_hook is None else
                                              (lambda k, x, _i=i: state_hook(_i, k, x)), conv_precision=conv_precision,
                                              stochastic=dpm_stochastic, **keyed[i])
        elif ddim_step > 0:
            eps, _ = diffusion.run_ddim(dae[i], num_samples, shape[i], temp, enable_autocast,
                                        is_image=False, ddim_step=ddim_step,
                                        condition_input=condition_input, clip_feat=clip_feat,
                                        skip_type=ddim_skip_type, kappa=ddim_kappa, noise=noise,
                                        keep_trajectory=False, graph=graph,
                                        given_noise=None if given_noise is None else given_noise[i],
                                        state_hook=None if state_hook is None else
                                        (lambda k, x, _i=i: state_hook(_i, k, x)), conv_precision=conv_precision,
                                        **keyed[i])
        else:
            eps, _ = diffusion.run_denoising_diffusion(dae[i], num_samples, shape[i], temp,
                                                       enable_autocast, is_image=False,
                                                       condition_input=condition_input,
                                                       clip_feat=clip_feat, graph=graph, keep_trajectory=False,
                                                       conv_precision=conv_precision, **keyed[i])
        condition_input = eps
        if i == 0:
            condition_input = vae.global2style(condition_input)
        all_eps.append(eps)
        if step_callback is not None:
            step_callback(i)
    eps = vae.compose_eps(all_eps)
    info = {'print/sample_mean_global': eps.view(num_samples, -1).mean(-1).mean(),
            'print/sample_var_global': eps.view(num_samples, -1).var(-1).mean()}
    if ode_sample == 1:
        info['nfe'] = nfes
    if sub is not None:
        info['seeds'] = sub
    points = vae.sample(num_samples=num_samples, decomposed_eps=vae.decompose_eps(eps))
    return points, info


def shard_batch(total: int, rank: int, world: int) -> int:
    """shapes this rank generates: contiguous split, remainder to the low ranks."""
    return total // world + (1 if rank < total % world else 0)


def rank_seed(base_seed: int, rank: int, iteration: int = 0) -> int:
    """one seed per (rank, iteration) for the call-level generators: the sample SET of a job then depends on the world size"""
    return int(base_seed) + 1000003 * int(rank) + int(iteration)


def shape_seeds(base_seed: int, start: int, count: int):
    """the seeds of the job's shapes start ... start+count-1: shape k's seed is output k of the SplitMix64 sequence from state
    base_seed, so shape_seeds(b, start, count)[j] == chain.split_seed(b, start + count)[start + j], each in O(1).  A rank takes
    its slice (shard_batch) and passes it as `seeds`: the set of shapes a job produces then does not depend on the world
    size, as long as every call uses the same batch size."""
    M = 0xFFFFFFFFFFFFFFFF
    if start < 0 or count < 0:
        raise ValueError(f"shape_seeds: start = {start}, count = {count}")
    out = []
    for k in range(int(start), int(start) + int(count)):
        z = ((int(base_seed) & M) + (k + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        out.append(z ^ (z >> 31))
    return out


def gather_samples(local_points: torch.Tensor, world: int):
    """all_gather of [B_local, N, 3] samples at the end of a generation job
    (trainers/base_trainer.py:484-487); the only communication of the sampling path."""
    import torch.distributed as dist
    if world == 1 or not dist.is_initialized():
        return local_points
    sizes = [torch.zeros(1, dtype=torch.int64, device=local_points.device) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([local_points.shape[0]], dtype=torch.int64, device=local_points.device))
    mx = int(max(s.item() for s in sizes))
    pad = torch.zeros((mx,) + tuple(local_points.shape[1:]), dtype=local_points.dtype, device=local_points.device)
    pad[: local_points.shape[0]] = local_points
    bufs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad)
    return torch.cat([b[: int(s.item())] for b, s in zip(bufs, sizes)], dim=0)
