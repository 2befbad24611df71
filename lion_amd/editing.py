"""Diffuse-denoise -- the two-latent recipe of the reference's ``trainers/denoise_pts.py:101-156``: encode a shape, push
its latents part of the way into the forward process, run the reverse chain from there, decode.  Shape variation, denoising
of noisy or voxelised inputs, editing.

Per latent the device work is one forward draw (``DiffusionDiscretized.diffuse``: lion_chain_diffuse, noise on the chip) and
``time_start`` replays of the prior's captured ancestral step (``run_denoising_diffusion_from_t``) -- the chain a sampling
call of the same batch shape captured is the one replayed here.  ``time_start`` is one index per latent for the whole batch, as
in the reference, or one per latent AND sample (per-sample start steps, DESIGN.md 4.6.9: one keyed forward draw and
max(time_start) replays of the per-sample-start capture, each sample held until its own first row).  With
``keep=mask`` the local latent's tail is region-preserving: the marked latent points are kept, the rest is
re-drawn conditioned on them, in the same number of replays; ``resample=`` adds RePaint's resampling jumps to that tail (DESIGN.md
4.6.11: more replays, and a re-drawn part that agrees with the kept one).  With ``solver_steps=S``
the tail is instead at most S replays of the few-step solver's captured step (``run_dpm_solver(t_start=...)``, by default its stochastic form: fresh noise re-enters during the tail, as in the recipe).

``voxel_guided`` is the recipe on the surface of the input's voxelisation (``perturb.voxel_surface_points``);
``voxel_grid_guided`` starts from a voxel grid instead of a cloud.  Both can report the voxel IoU of input and output.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import chain as _chain
from . import diffusion_ops
from .chain import split_seed as _split_seed   # SplitMix64: one seed -> a key per draw (shared with sampling.py)

_MASK64 = 0xFFFFFFFFFFFFFFFF
SUBKEYS = ("vae", "diffuse_global", "chain_global", "diffuse_local", "chain_local")   # the order a seed is split in


@torch.no_grad()
def diffuse_denoise(vae, dae, diffusion, x, time_start, *, temp=1.0, clip_feat=None, keep_first=False, graph=True,
                    conv_precision="fp32", seed=None, solver_steps=None, stochastic=True, seeds=None, keep=None,
                    resample=None):
    """x [B, N, 3] -> (points [B, N, 3], info).  vae: models.vae_adain.Model (in the mode the caller wants: eval() for
    inference); dae: [global prior, local prior]; diffusion: DiffusionDiscretized.

    Sequence (denoise_pts.py:101-156): encode_global -> sample -> [diffuse -> denoise on dae[0]] -> global2style ->
    encode_local(x, style) -> sample -> [diffuse -> denoise on dae[1], conditioned on the edited global latent] -> decode.

    time_start: an int, or a (global, local) pair, each in 0 ... T-1.  As in the reference, the latent is diffused with the
    schedule INDEX time_start (alpha_bar[time_start], the marginal of the model's timestep time_start + 1) while denoising
    begins with the step at index time_start - 1: the chain runs time_start steps and treats its start as one step less noisy
    than it was drawn.  That off-by-one is the reference's and is kept.  0 skips diffusion for that latent; with both at 0
    the result is the VAE's reconstruction from its sampled latents.
    Per-sample start steps: time_start itself (a 1-D integer tensor or numpy array), or either element of the pair (there a
    list or tuple too), may be B indices, one per sample -- a strength sweep of one shape, or a batch of scans that each need
    their own amount of denoising, in ONE call.  A top-level tuple or list of length 2 is always the (global, local) pair.
    Sample b of the call is, bit for bit at equal B and equal `seeds`, sample b of the call with the ints (g[b], l[b]); a
    sample with 0 keeps that latent.  The latent costs max(time_start) prior evaluations of the whole batch.  The draws are
    always keyed: under `seed` each draw's key is split once more into one key per sample.  ValueError: a wrong count, bool
    entries, an index outside 0 ... T-1, or per-sample indices with solver_steps.
    keep_first: sample 0 keeps its own latents (the reference's ``eps[0:1] = eps_ori[0:1]``), so the batch shows the input's
    reconstruction next to its variations.
    seed: makes the whole call repeatable and leaves torch's global generators alone; None draws one from torch's CPU
    generator (chain.draw_seed), so torch.manual_seed governs the call.
    The local prior's condition_input is vae.global2style(edited global latent), as the samplers and the training of this
    package pass it; the reference's recipe passes the latent itself, which is the same tensor whenever style_mlp is '' (every
    released configuration).
    info: 'global_original', 'global_edited', 'local_original', 'local_edited' (the four latents, [B] + latent_shape()),
    'condition_input' (what the local prior was conditioned on), 'time_start' (the pair that ran: ints, or tuples of B ints),
    'seeds' (the call's seed and the key of every draw derived from it) and 'tail_steps' (per latent the list of schedule
    indices its tail evaluated the prior at, in order: max(time_start) - 1 ... 0; [] where time_start is 0).
    solver_steps: None (default) is the ancestral tail above.  An int S >= 2 runs each latent's tail with the few-step solver,
    run_dpm_solver(steps=S, t_start=time_start[i], stochastic=stochastic, seed=seeds['chain_*']): at most S evaluations of the
    prior, at the indices solver_schedule(S, 'logsnr', time_start[i]), instead of time_start[i].  The solver tail STARTS AT
    index time_start, the marginal the latent was actually drawn from: it does not reproduce the reference's off-by-one,
    which stays with the ancestral tail.  stochastic=True (default) is SDE-DPM-Solver++(2M), whose steps draw fresh noise
    as the ancestral steps do; False is the deterministic solver, which only transports the perturbation of the forward draw.
    keep_first, conv_precision, graph and time_start = 0 behave as in the ancestral tail; temp scales the ancestral steps'
    noise only, the solver has no such knob.
    seeds: B ints (a sequence or an int64 tensor, each mod 2^64) in place of `seed`, one per sample: "variation #5 again".
    Sample b's seed is split (SplitMix64) into the five keys of SUBKEYS, and every draw of sample b -- the two
    reparameterisation draws (streams 0 and 1 of lion_philox_normal_keyed under 'vae'), the two forward draws, the two tails'
    per-step noise -- comes from its own keys at counters within the sample: it depends on neither B, nor b, nor the other
    samples' seeds, and torch's generators are not touched.  The output for a seed is promised bit-equal at equal B only
    (other batch sizes select other kernel plans).  info['seeds'] then holds 'seeds' (the list) and a list per sub-key.
    ValueError before any launch: len(seeds) != B, or seeds with seed.
    keep: a bool tensor or array [B, N] or [N] (one mask for every sample) over the INPUT points, True = keep that point's latent
    point ("keep the legs, give me other backs").  The local latent is point-wise -- latent point i is the
    latent_shape()[1] / N consecutive floats behind input point i -- and its tail runs region-preserving,
    run_denoising_diffusion_from_t(known=(sampled local encoding, keep)): the kept latent points of 'local_edited' are those of
    'local_original' bit for bit, the others are re-drawn conditioned on them.  The global latent follows time_start as without
    keep; (0, t) leaves it alone.  keep_first, seeds, per-sample time_start and conv_precision combine with it.  The decoder
    mixes neighbouring latent points, so the decoded kept points are NOT promised equal to the input points.  info['keep'] is
    the mask that ran ([B, N] bool; None without keep).  ValueError before any launch: another dtype or shape, or keep with
    solver_steps.
    resample (with keep): RePaint's resampling jumps on the region-preserving tail, an int n_resample (jump
    length 10) or a pair (jump_length, n_resample), as run_denoising_diffusion_from_t(resample=) takes it.  In a single pass the
    re-drawn points only ever see independent noisy copies of the kept ones and stay close to the input at small time_start;
    walking back up and down n_resample times at every anchor lets them follow the kept points.  It applies where `known` is
    passed, the local latent's tail.  info['resample'] is (jump_length, n_resample) (None without it) and info['tail_rows']
    the replay count per latent: time_start for the global latent, the length of resample_walk(time_start, jump_length,
    n_resample) for the local one.  'tail_steps' stays the plain descending list.  ValueError before any launch: resample
    without keep, with solver_steps or with per-sample time_start."""
    T = diffusion._diffusion_steps
    B = x.shape[0]
    pair = tuple(time_start) if isinstance(time_start, (tuple, list)) else (time_start, time_start)
    if len(pair) != 2:
        raise ValueError(f"diffuse_denoise: time_start = {time_start!r}: an int or a (global, local) pair in [0, {T - 1}]")
    # per latent: an int, or (per-sample start steps) a tuple of B ints -- inside the pair a list is one too
    inside = isinstance(time_start, (tuple, list))
    starts = [diffusion.per_sample_indices("diffuse_denoise: time_start", t, B, 0, T - 1, lists=inside) for t in pair]
    if any(s is None and (isinstance(t, bool) or not isinstance(t, numbers.Integral) or not 0 <= t <= T - 1)
           for s, t in zip(starts, pair)):
        raise ValueError(f"diffuse_denoise: time_start = {time_start!r}: an int or a (global, local) pair in [0, {T - 1}], "
                         f"each an int or {B} per-sample indices")
    pair = tuple(int(t) if s is None else tuple(s) for s, t in zip(starts, pair))
    if solver_steps is not None and (isinstance(solver_steps, bool) or not isinstance(solver_steps, numbers.Integral)
                                     or solver_steps < 2):
        raise ValueError(f"diffuse_denoise: solver_steps = {solver_steps!r}: None or an int >= 2")
    if solver_steps is not None and any(isinstance(t, tuple) for t in pair):
        raise ValueError("diffuse_denoise: per-sample time_start cannot be combined with solver_steps (a per-sample solver "
                         "schedule would need per-sample timesteps)")
    if keep is not None:
        if solver_steps is not None:
            raise ValueError("diffuse_denoise: keep cannot be combined with solver_steps (the solver tails have no known-region "
                             "form)")
        keep = _keep_mask(keep, B, x.shape[1], vae.latent_shape()[1])
    if resample is not None:
        resample = diffusion.resample_pair("diffuse_denoise", resample)
        if keep is None:
            raise ValueError("diffuse_denoise: resample needs keep: without kept points there is nothing to agree with")
        if solver_steps is not None:
            raise ValueError("diffuse_denoise: resample cannot be combined with solver_steps")
        if any(isinstance(t, tuple) for t in pair):
            raise ValueError("diffuse_denoise: resample cannot be combined with per-sample time_start (a sample's own walk "
                             "would differ from the walk of its uniform call)")
        if pair[1] > 0:
            diffusion.resample_walk(pair[1], *resample)     # a walk that is too long is refused here
    visited, rows = [[], []], [0, 0]
    names = SUBKEYS
    keyed = seeds is not None
    if keyed:
        if seed is not None:
            raise ValueError("diffuse_denoise: seeds cannot be combined with seed")
        per_sample = _chain.sample_keys(seeds, x.shape[0], "diffuse_denoise")
    if not x.is_cuda:
        raise RuntimeError("lion_amd: expected a CUDA(HIP) tensor; there is no CPU path")
    B, shapes = x.shape[0], vae.latent_shape()
    if keyed:
        split = [_split_seed(k, len(names)) for k in per_sample]
        seeds = {name: [sp[j] for sp in split] for j, name in enumerate(names)}
        seeds["seeds"] = per_sample
        vae_words = _chain.key_words(seeds["vae"], x.device)
        draws = iter((0, 1))

        def sample(dist):   # Normal.sample() on each sample's own key: stream 0 for the global latent, 1 for the local
            rho = diffusion_ops.philox_normal_keyed(vae_words, B, list(dist.mu.shape[1:]), _chain.START_STEP_WORD,
                                                    stream_id=next(draws), device=dist.mu.device)
            return dist.sample_given_rho(rho.to(dist.mu.dtype))
    else:
        base = _chain.draw_seed() if seed is None else int(seed) & _MASK64
        seeds = dict(zip(names, _split_seed(base, len(names))), seed=base)
        gen = torch.Generator(device=x.device).manual_seed(seeds["vae"] & 0x7FFFFFFFFFFFFFFF)

        def sample(dist):   # Normal.sample() on a generator of this call
            return dist.sample_given_rho(torch.randn(dist.mu.shape, device=dist.mu.device, dtype=dist.mu.dtype, generator=gen))

    def key(name):   # the call's key of that draw, or (seeds) every sample's
        return {"seeds" if keyed else "seed": seeds[name]}

    def edit(i, eps_ori, condition_input):
        if pair[i] == 0:
            return eps_ori
        which = ("global", "local")[i]
        known = {"known": (eps_ori, keep)} if keep is not None and i == 1 else {}
        if known and resample is not None:
            known["resample"] = resample
        if isinstance(pair[i], tuple):   # per-sample starts: one keyed forward draw, max(start) replays of the from-rows capture
            top = max(pair[i])
            if top == 0:
                return eps_ori
            visited[i] = list(range(top - 1, -1, -1))
            rows[i] = top
            at = torch.tensor([t if t > 0 else -1 for t in pair[i]], dtype=torch.int64)   # start 0: neither diffused nor denoised
            eps_t = diffusion.diffuse(eps_ori, at, **key("diffuse_" + which))
            eps, _ = diffusion.run_denoising_diffusion_from_t(dae[i], B, shapes[i], torch.tensor(pair[i], dtype=torch.int64),
                                                              eps_t, temp=temp, condition_input=condition_input,
                                                              clip_feat=clip_feat, graph=graph, keep_trajectory=False,
                                                              conv_precision=conv_precision, **key("chain_" + which), **known)
            if keep_first:
                eps[0:1] = eps_ori[0:1]
            return eps.contiguous()
        eps_t = diffusion.diffuse(eps_ori, pair[i], **key("diffuse_" + which))
        if solver_steps is not None:
            visited[i] = diffusion.solver_schedule(int(solver_steps), 'logsnr', pair[i])
            rows[i] = len(visited[i])
            eps, _ = diffusion.run_dpm_solver(dae[i], B, shapes[i], steps=int(solver_steps), x_noisy=eps_t,
                                              condition_input=condition_input, clip_feat=clip_feat, keep_trajectory=False,
                                              graph=graph, conv_precision=conv_precision, stochastic=stochastic,
                                              t_start=pair[i], **key("chain_" + which))
        else:
            visited[i] = list(range(pair[i] - 1, -1, -1))
            rows[i] = len(diffusion.resample_walk(pair[i], *resample)) if "resample" in known else pair[i]
            eps, _ = diffusion.run_denoising_diffusion_from_t(dae[i], B, shapes[i], pair[i], eps_t, temp=temp,
                                                              condition_input=condition_input, clip_feat=clip_feat, graph=graph,
                                                              keep_trajectory=False, conv_precision=conv_precision,
                                                              **key("chain_" + which), **known)
        if keep_first:
            eps[0:1] = eps_ori[0:1]
        return eps.contiguous()

    eps = sample(vae.encode_global(x))
    flat_shape = eps.shape
    global_ori = eps.view([B] + shapes[0]).contiguous()
    global_new = edit(0, global_ori, None)
    style = vae.global2style(global_new.view(flat_shape))
    condition_input = vae.global2style(global_new)

    eps = sample(vae.encode_local(x, style))
    flat_shape = eps.shape
    local_ori = eps.view([B] + shapes[1]).contiguous()
    local_new = edit(1, local_ori, condition_input)
    points = vae.decoder(None, beta=None, context=local_new.view(flat_shape), style=style)
    info = {"global_original": global_ori, "global_edited": global_new, "local_original": local_ori,
            "local_edited": local_new, "condition_input": condition_input, "time_start": pair, "seeds": seeds,
            "tail_steps": (visited[0], visited[1]), "keep": keep, "resample": resample, "tail_rows": (rows[0], rows[1])}
    return points, info


def _keep_mask(keep, B, n_points, local_shape):
    """diffuse_denoise's `keep` as a bool tensor [B, n_points] (on the device it came from; an array: the host); ValueError on
    another dtype or shape, or a local latent that is not a whole number of quads per point.  Host work only."""
    if not isinstance(keep, torch.Tensor):
        try:
            keep = torch.from_numpy(np.asarray(keep))
        except TypeError as e:
            raise ValueError(f"diffuse_denoise: keep is a bool tensor or array, got {type(keep).__name__}") from e
    if keep.dtype != torch.bool or tuple(keep.shape) not in ((B, n_points), (n_points,)):
        raise ValueError(f"diffuse_denoise: keep is a bool mask [{B}, {n_points}] or [{n_points}], got {keep.dtype} "
                         f"{tuple(keep.shape)}")
    per_sample = int(np.prod(local_shape))
    if per_sample % n_points != 0 or (per_sample // n_points) % 4 != 0:
        raise ValueError(f"diffuse_denoise: keep needs a local latent of whole quads per point, got {per_sample} floats for "
                         f"{n_points} points")
    return (keep if keep.dim() == 2 else keep.unsqueeze(0).expand(B, n_points)).contiguous()


@torch.no_grad()
def voxel_guided(vae, dae, diffusion, x, resolution, time_start, *, iou=False, **diffuse_denoise_kwargs):
    """Voxel-guided synthesis: x [B, N, 3] -> (points [B, N, 3], info).  The input is replaced by N points on the surface of
    its voxelisation at `resolution` (perturb.voxel_surface_points) and that cloud goes through diffuse_denoise(vae, dae,
    diffusion, ., time_start, **diffuse_denoise_kwargs), which is not changed (`keep` and `resample` go through with the
    rest).  `seeds` (or `seed`) of the keyword arguments address both: sample b's voxel points are drawn under seeds[b] at LION_VOXEL_STEP_WORD, a step word no draw of
    diffuse_denoise uses, so the two never share a counter.  info is diffuse_denoise's with 'input' (the voxel-surface cloud
    that was denoised) and 'faces' (int32[B], the exposed faces per cloud).
    iou=True adds the paper's measure of the experiment, the voxel IoU between the input's voxels and the voxelised output in
    the input's frame: 'input grid' and 'frame' (perturb.voxel_occupancy(x, resolution)), 'iou' (float32[B]) and 'iou_counts'
    (int32[B, 2]: intersection, union) -- three more launches; the default issues none and adds no key."""
    from . import perturb
    pts, made = perturb.voxel_surface_points(x, resolution, x.shape[1], seeds=diffuse_denoise_kwargs.get("seeds"),
                                             seed=diffuse_denoise_kwargs.get("seed"))
    points, info = diffuse_denoise(vae, dae, diffusion, pts, time_start, **diffuse_denoise_kwargs)
    info["input"], info["faces"] = pts, made["faces"]
    if iou:
        grid, occ = perturb.voxel_occupancy(x, resolution)
        _add_iou(info, grid, occ["frame"], points)
    return points, info


def _add_iou(info, grid, frame, points):
    """info['iou'], ['iou_counts'], ['input grid'], ['frame']: the output `points` against the input's grid, in its frame"""
    from . import metrics
    value, m = metrics.voxel_iou(grid, points, frame=frame)
    info["input grid"], info["frame"], info["iou"] = grid, frame, value
    info["iou_counts"] = m["counts"]


@torch.no_grad()
def voxel_grid_guided(vae, dae, diffusion, grid, time_start, frame=None, num_points=2048, iou=False,
                      **diffuse_denoise_kwargs):
    """Voxel-guided synthesis from voxels: grid [B, r, r, r] (bool or uint8, r <= 32; an editor's, a scan's, a coarse shape's)
    -> (points [B, num_points, 3], info).  num_points points are drawn on the exposed faces of the grid, placed in `frame`
    (perturb.voxel_surface_points_from_grid; None: the cube [-1, 1]^3), and that cloud goes through diffuse_denoise(vae, dae,
    diffusion, ., time_start, **diffuse_denoise_kwargs) under the same `seeds` / `seed`, as in voxel_guided.  info is
    diffuse_denoise's with 'input' (the cloud that was denoised), 'faces' (int32[B]), 'input grid' and 'frame' (float32[B, 4]
    on the device).  iou=True adds 'iou' (float32[B]: the voxel IoU of the input grid and the output voxelised in the same
    frame, metrics.voxel_iou) and 'iou_counts' (int32[B, 2]: intersection, union)."""
    from . import perturb
    pts, made = perturb.voxel_surface_points_from_grid(grid, frame, num_points, seeds=diffuse_denoise_kwargs.get("seeds"),
                                                       seed=diffuse_denoise_kwargs.get("seed"))
    points, info = diffuse_denoise(vae, dae, diffusion, pts, time_start, **diffuse_denoise_kwargs)
    info["input"], info["faces"], info["input grid"], info["frame"] = pts, made["faces"], grid, made["frame"]
    if iou:
        _add_iou(info, grid, made["frame"], points)
    return points, info
