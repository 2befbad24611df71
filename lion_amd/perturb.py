"""Perturbed inputs for guided synthesis: the clouds ``editing.diffuse_denoise`` denoises and ``training.vae_forward_backward(...,
noisy_input=)`` fine-tunes the encoder on -- points on the surface of a cloud's voxelisation, and the three corruptions of the
paper's denoising experiments (normal noise, uniform noise, outliers).  Made on the device from clouds resident in HBM
(csrc/perturb.hip), one launch each, nothing synchronises with the host.  The voxelisation is also an
object of its own: ``voxel_occupancy`` returns a cloud's grid and frame, ``voxel_surface_points_from_grid``
starts from a grid that is given (an editor's, a scan's), ``metrics.voxel_iou`` compares grids.

Every sample is addressed by its own 64-bit key: sample b's output under seeds[b] is the same bits alone, first
or last of a batch and beside any batchmates.  The draws come from the chain's Philox generator at reserved step words of their
own, so a key shared with a sampler or with diffuse_denoise repeats none of their noise.
"""
from __future__ import annotations

import numbers

import torch

from . import _lib, diffusion_ops
from . import chain as _chain

__all__ = ["voxel_surface_points", "voxel_occupancy", "voxel_surface_points_from_grid", "add_noise", "KINDS", "MAX_RESOLUTION",
           "UNIT_FRAME"]

# the step words of include/lion_hip.h: beside chain.START_STEP_WORD / DIFFUSE_STEP_WORD, above every chain step's row index
VOXEL_STEP_WORD, PERTURB_STEP_WORD = 0xFFFFFFFD, 0xFFFFFFFC
KINDS = ("normal", "uniform", "outlier")
MAX_RESOLUTION = 32
_MODE = {"uniform": 0, "outlier": 1}


def _cloud_shape(x, who):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[-1] < 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: x is [B, N, 3] (or [B, N, D], D > 3), got {tuple(getattr(x, 'shape', ()))!r}")
    if x.dtype != torch.float32:
        raise ValueError(f"{who}: x is float32, got {x.dtype}")
    return int(x.shape[0]), int(x.shape[1])


def _keys(seeds, seed, B, who):
    """the call's keys: `seeds` as B ints mod 2^64 (or their int32[B, 2] device words, which pass as they are: a loop or a
    captured region uploads its keys once).  seed: one int, expanded with sampling.shape_seeds(seed, 0, B).  Neither: one base
    seed from torch's CPU generator (chain.draw_seed), expanded the same way.  Host work only."""
    if seeds is not None:
        if seed is not None:
            raise ValueError(f"{who}: seeds cannot be combined with seed")
        if isinstance(seeds, torch.Tensor) and seeds.dtype == torch.int32 and seeds.dim() == 2:
            if tuple(seeds.shape) != (B, 2):
                raise ValueError(f"{who}: key words {tuple(seeds.shape)} for {B} samples")
            return seeds
        return _chain.sample_keys(seeds, B, who)
    from .sampling import shape_seeds
    return shape_seeds(_chain.draw_seed() if seed is None else int(seed), 0, B)


def _xyz(x):
    _lib.require_cuda(x)
    return x[..., :3].contiguous()


@torch.no_grad()
def voxel_surface_points(x, resolution, num_points=None, *, seeds=None, seed=None, stream_id=0):
    """x [B, N, 3] (or [B, N, D], D > 3: xyz is read) -> (points [B, K, 3], info): K = num_points (default N) points drawn
    uniformly over the exposed faces of the cloud's voxelisation at `resolution` (1 ... 32) -- the cube around the middle of the
    cloud's bounding box, its side the box's longest, cut into resolution^3 voxels; a face is exposed when the voxel holds a
    point and its neighbour across the face holds none or lies outside the grid.  Exact arithmetic: include/lion_hip.h,
    lion_voxel_surface_points_keyed.  Every cloud is handled on its own.
    seeds: B ints (a sequence or an int64 tensor, each mod 2^64) or their int32[B, 2] device words (chain.key_words), one key
    per sample: point k of sample b is the Philox draw under seeds[b] at counter (k, LION_VOXEL_STEP_WORD, stream_id), whatever
    B, b and the other seeds are, and torch's generators are not touched.  seed: one int for the batch, expanded with
    sampling.shape_seeds(seed, 0, B).  Neither: a base seed is drawn from torch's CPU generator (torch.manual_seed governs it).
    info: 'faces' (int32[B] on the device: the exposed faces of each cloud) and 'seeds' (as given, or the expanded list).
    One launch, no host synchronisation; with device key words the call can be captured.
    ValueError before the device is touched: resolution outside 1 ... 32, num_points < 1, a wrong seed count, seeds with seed,
    x not a float32 [B, N, >= 3] tensor."""
    who = "voxel_surface_points"
    B, N = _cloud_shape(x, who)
    r = _resolution(resolution, who)
    K = N if num_points is None else num_points
    if isinstance(K, bool) or not isinstance(K, numbers.Integral) or K < 1:
        raise ValueError(f"{who}: num_points = {num_points!r}: None or an int >= 1")
    K = int(K)
    keys = _keys(seeds, seed, B, who)
    xyz = _xyz(x)
    words = diffusion_ops._device_keys(keys, B, xyz.device, who)
    out = torch.empty((B, K, 3), device=xyz.device, dtype=torch.float32)
    faces = torch.empty((B,), device=xyz.device, dtype=torch.int32)
    ws_bytes = int(_lib.load().lion_voxel_surface_workspace_bytes(B, N, r, K))
    ws = torch.empty((ws_bytes,), device=xyz.device, dtype=torch.uint8) if ws_bytes else None
    _lib.call("lion_voxel_surface_points_keyed", xyz, B, N, r, words, int(stream_id), K, out, faces, ws, ws_bytes)
    return out, {"faces": faces, "seeds": keys}


def _resolution(resolution, who):
    if isinstance(resolution, bool) or not isinstance(resolution, numbers.Integral) or not 1 <= resolution <= MAX_RESOLUTION:
        raise ValueError(f"{who}: resolution = {resolution!r}: an int in [1, {MAX_RESOLUTION}]")
    return int(resolution)


def _grid_shape(grid, who):
    """(B, r) of an occupancy grid: a bool or uint8 [B, r, r, r] tensor, 1 <= r <= 32"""
    if not isinstance(grid, torch.Tensor) or grid.dim() != 4 or grid.shape[0] < 1 or len(set(grid.shape[1:])) != 1:
        raise ValueError(f"{who}: a grid is [B, r, r, r], got {tuple(getattr(grid, 'shape', ()))!r}")
    if grid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: a grid is bool or uint8 (non-zero: occupied), got {grid.dtype}")
    if not 1 <= grid.shape[1] <= MAX_RESOLUTION:
        raise ValueError(f"{who}: grid resolution {grid.shape[1]}: in [1, {MAX_RESOLUTION}]")
    return int(grid.shape[0]), int(grid.shape[1])


def _host_frame(frame, B, who):
    """None, a device f32[B, 4] tensor (passed on: the host cannot vet it), or a host frame -- 4 numbers for the whole batch or
    B x 4, a sequence or a CPU tensor -- validated here (finite, side > 0) and returned as a CPU f32[B, 4] tensor to upload"""
    if frame is None:
        return None
    if isinstance(frame, torch.Tensor) and frame.is_cuda:
        if frame.dtype != torch.float32 or tuple(frame.shape) != (B, 4):
            raise ValueError(f"{who}: a device frame is float32 [{B}, 4], got {frame.dtype} {tuple(frame.shape)}")
        return frame
    try:
        f = torch.as_tensor(frame, dtype=torch.float64, device="cpu")
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{who}: frame = {frame!r}: (lo_x, lo_y, lo_z, side), one for the batch or one per sample") from e
    if tuple(f.shape) == (4,):
        f = f.expand(B, 4)
    if tuple(f.shape) != (B, 4):
        raise ValueError(f"{who}: frame of shape {tuple(f.shape)}: 4 numbers or [{B}, 4]")
    f = f.to(torch.float32)
    if not bool(torch.isfinite(f).all()) or not bool((f[:, 3] > 0).all()):
        raise ValueError(f"{who}: a frame is finite with side > 0, got {f.tolist()!r}")
    return f.contiguous()


def _device_frame(frame, device):
    return frame if frame is None or frame.is_cuda else frame.to(device)


@torch.no_grad()
def voxel_occupancy(x, resolution, frame=None):
    """x [B, N, 3] (or [B, N, D], D > 3: xyz is read) -> (grid bool [B, r, r, r], info): the voxels of every cloud at r =
    `resolution` (1 ... 32), indexed [x, y, z].  A frame is (lo_x, lo_y, lo_z, side), the cube the grid covers.  frame=None: every
    cloud in its OWN frame, the box of voxel_surface_points -- the grid is then exactly the occupancy that function builds.
    Otherwise a device float32 [B, 4] tensor (used as it is; the host cannot vet it, and whatever it holds no access leaves
    its range), or a host frame: 4 numbers (one frame for the batch) or B x 4, a sequence or a CPU tensor, validated here
    (finite, side > 0) and uploaded.  A point's voxel index is ALWAYS clamped to 0 ... r-1, so points outside a given frame land
    in its boundary voxels.  Exact arithmetic: include/lion_hip.h, lion_voxel_occupancy.
    info: 'frame' (float32 [B, 4] on the device: the frame that was used) and 'clamped' (int32 [B] on the device: the points of
    each cloud whose index the clamp changed on at least one axis).
    One launch, no host synchronisation; with frame None or a device frame the call can be captured.
    ValueError before the device is touched: resolution outside 1 ... 32, x not a float32 [B, N, >= 3] tensor, a host frame of
    another shape, not finite, or with side <= 0, a device frame that is not float32 [B, 4]."""
    who = "voxel_occupancy"
    B, N = _cloud_shape(x, who)
    r = _resolution(resolution, who)
    frame = _host_frame(frame, B, who)
    xyz = _xyz(x)
    frame = _device_frame(frame, xyz.device)
    grid = torch.empty((B, r, r, r), device=xyz.device, dtype=torch.bool)
    used = torch.empty((B, 4), device=xyz.device, dtype=torch.float32)
    clamped = torch.empty((B,), device=xyz.device, dtype=torch.int32)
    _lib.call("lion_voxel_occupancy", xyz, B, N, r, frame, grid, used, clamped)
    return grid, {"frame": used, "clamped": clamped}


UNIT_FRAME = (-1.0, -1.0, -1.0, 2.0)   # the cube [-1, 1]^3: the frame of a grid that comes without one


@torch.no_grad()
def voxel_surface_points_from_grid(grid, frame=None, num_points=2048, *, seeds=None, seed=None, stream_id=0):
    """grid [B, r, r, r] (bool, or uint8 where any non-zero byte is an occupied voxel; indexed [x, y, z], r <= 32) ->
    (points [B, K, 3], info): K = num_points points drawn uniformly over the exposed faces of the grid, placed in `frame` --
    voxel_surface_points for a voxelisation that is given, not made from a cloud.  frame: as in voxel_occupancy; None is the
    cube [-1, 1]^3, i.e. (-1, -1, -1, 2) (UNIT_FRAME).  With the grid and info['frame'] that voxel_occupancy(x, r) returns, the
    points are voxel_surface_points(x, r, K)'s under the same seeds, bit for bit.  An empty grid has no face: its 'faces' entry
    is 0 and all its K points are the frame's centre.  Exact arithmetic: include/lion_hip.h,
    lion_voxel_surface_points_grid_keyed.
    seeds / seed / neither, stream_id: as in voxel_surface_points (counter (k, LION_VOXEL_STEP_WORD, stream_id) under seeds[b]).
    info: 'faces' (int32 [B] on the device), 'seeds' (as given, or the expanded list) and 'frame' (float32 [B, 4] on the device).
    One launch, no host synchronisation; with device key words and a device frame the call can be captured.
    ValueError before the device is touched: grid not a bool / uint8 [B, r, r, r] tensor with 1 <= r <= 32, num_points < 1, a
    wrong seed count, seeds with seed, a bad frame (voxel_occupancy)."""
    who = "voxel_surface_points_from_grid"
    B, r = _grid_shape(grid, who)
    K = num_points
    if isinstance(K, bool) or not isinstance(K, numbers.Integral) or K < 1:
        raise ValueError(f"{who}: num_points = {num_points!r}: an int >= 1")
    K = int(K)
    frame = _host_frame(UNIT_FRAME if frame is None else frame, B, who)
    keys = _keys(seeds, seed, B, who)
    _lib.require_cuda(grid)
    frame = _device_frame(frame, grid.device)
    words = diffusion_ops._device_keys(keys, B, grid.device, who)
    out = torch.empty((B, K, 3), device=grid.device, dtype=torch.float32)
    faces = torch.empty((B,), device=grid.device, dtype=torch.int32)
    _lib.call("lion_voxel_surface_points_grid_keyed", grid, frame, B, r, words, int(stream_id), K, out, faces)
    return out, {"faces": faces, "seeds": keys, "frame": frame}


@torch.no_grad()
def add_noise(x, kind, amount, *, seeds=None, seed=None):
    """x [B, N, 3] (or [B, N, D], D > 3: only xyz is perturbed, the other channels are copied) -> the corrupted cloud, same shape.
      'normal'   x + amount*z, z ~ N(0, 1): DiffusionDiscretized.diffuse's keyed draw (lion_chain_diffuse_keyed, m = 1,
                 s = amount), bit for bit; a sample's 3*N coordinates must be a multiple of 4 there (N % 4 == 0)
      'uniform'  x + amount*(2u - 1), u uniform on [0, 1) per coordinate
      'outlier'  each point is replaced, with probability amount (0 ... 1), by a uniform draw inside the cloud's own per-axis
                 bounding box; the others are copied bit for bit
    Exact arithmetic of the last two: include/lion_hip.h, lion_perturb_points_keyed (counter (point index,
    LION_PERTURB_STEP_WORD, 0) under the sample's key).  seeds / seed / neither: as in voxel_surface_points.
    ValueError before the device is touched: an unknown kind, a negative (or NaN) amount, an outlier fraction > 1, a wrong seed
    count, seeds with seed, 'normal' with N % 4 != 0, x not a float32 [B, N, >= 3] tensor."""
    who = "add_noise"
    B, N = _cloud_shape(x, who)
    if kind not in KINDS:
        raise ValueError(f"{who}: kind = {kind!r}: one of {KINDS}")
    if isinstance(amount, bool) or not isinstance(amount, numbers.Real) or not amount >= 0:
        raise ValueError(f"{who}: amount = {amount!r}: a number >= 0")
    if kind == "outlier" and amount > 1:
        raise ValueError(f"{who}: outlier fraction {amount!r} > 1")
    if kind == "normal" and N % 4 != 0:
        raise ValueError(f"{who}: normal noise is drawn a quad at a time: N = {N} is not a multiple of 4")
    keys = _keys(seeds, seed, B, who)
    xyz = _xyz(x)
    words = diffusion_ops._device_keys(keys, B, xyz.device, who)
    if kind == "normal":
        out = diffusion_ops.diffuse(xyz, 1.0, float(amount), seeds=words)
    else:
        out = torch.empty_like(xyz)
        _lib.call("lion_perturb_points_keyed", _MODE[kind], xyz, B, N, float(amount), words, 0, out)
    if x.shape[-1] == 3:
        return out
    full = x.clone()
    full[..., :3] = out
    return full
