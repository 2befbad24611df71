"""-m gpu: the small-grid (r <= 20) voxelize / devoxelize launches, bit for bit against the CPU oracle.

devox_slab_kernel's single-slab form (csrc/devoxelize.hip, every even r <= 20) loads a point's coordinates once, does
without the point sort and the row bitmap, and fetches every row of its channel grids unconditionally from kernel entry on.
r in (2, 6, 8, 10, 16, 20) covers every LD (1, 4, 9) and the CI values 16, 9, 2, 1, with rows of 4k + 2 floats (r = 2, 6, 10:
16-byte pieces that straddle two z-rows) and of 4k; N in (1 .. 1024) the empty, partial and full point slots of a 256-thread
workgroup; C = 17 crosses the CI / CT boundaries.  The voxelisations of the same sizes (r = 8, 16: vox_fused_kernel /
vox_scatter_kernel with one point per thread, all loads of the scatter's prologue in one round trip) are checked the same
way, at r = 16 also through the reader-aware scatter; N = 1 is normalised with eps = 1e-3 (with eps = 0 it is 0 / 0).  The
scatter launcher's coarsened channel split needs 256 workgroups and so a batch of 32: three cases at the step's own shapes.

Every devoxelize case runs twice with a launch on another grid of the same shape in between: the second run finds other
bytes in LDS and must give the same result -- stale LDS is never read."""
import numpy as np
import pytest
import torch

import geometry_cases as gc
from conftest import gaussian_cloud

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 255, 256, 257, 1024)
CS = (1, 9, 16, 17, 128)
DEVOX_RS = (2, 6, 8, 10, 16, 20)
DEVOX_CLOUDS = ("gauss", "one-voxel", "integer", "outside", "sparse")
VOX_RS = (8, 16)
VOX_CLOUDS = ("gauss", "one-voxel", "clump")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def bk():
    from lion_amd.functional.backend import _backend
    _backend.lib  # loads the .so, raises if missing
    return _backend


def same(got, want, what):
    got = host(got) if torch.is_tensor(got) else got
    bad = got != want
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def batch_of(ni, ci):
    """B in (1, 3), alternating over the (N, C) table so that every N and every C meets both"""
    return 1 if (ni + ci) % 2 == 0 else 3


def devox_cloud(kind, r, B, N, rng):
    """-> (coords [B,3,N] for the kernel, coords for the oracle, outside [B,N] bool).  The oracle (like the reference) would
    read out of bounds for a point outside the grid: it gets the cloud with that point moved inside, and the kernel's
    columns of the outside points must be 0."""
    e = float(r - 1)
    outside = np.zeros((B, N), bool)
    if kind == "gauss":
        co = gc.devox_cloud("dense", r, B, N, r, rng)
    elif kind == "one-voxel":
        cell = rng.integers(0, r - 1, (B, 3, 1)).astype(np.float32)
        co = (cell + rng.uniform(0.05, 0.95, (B, 3, N))).astype(np.float32)
    elif kind == "integer":
        co = gc.devox_cloud("lattice", r, B, N, r, rng)
        co[:, :, 0] = e                                       # the r - 1 corner: every "hi" equals its "lo"
    elif kind == "sparse":
        co = gc.devox_cloud("sparse", r, B, N, r, rng)
    else:
        co = gc.devox_cloud("dense", r, B, N, r, rng)
    ref_co = co
    if kind == "outside":
        co = co.copy()
        for b in range(B):
            i, axis = (N // 2 + b) % N, b % 3
            co[b, axis, i] = (r + 0.25, -0.75, float(r))[b % 3]
            outside[b, i] = True
    return co, ref_co, outside


@pytest.fixture(scope="module")
def devox_grids():
    """one grid, one other grid and one scale / shift pair per r, at the largest (B, C); the cases take leading slices"""
    made = {}

    def get(r):
        if r not in made:
            rng = np.random.default_rng(1000 + r)
            made[r] = (rng.standard_normal((3, max(CS), r ** 3), dtype=np.float32),
                       rng.standard_normal((3, max(CS), r ** 3), dtype=np.float32) * 3.0 + 5.0,
                       rng.uniform(0.5, 1.5, (3, max(CS))).astype(np.float32),
                       rng.standard_normal((3, max(CS))).astype(np.float32))
        return made[r]
    return get


@pytest.mark.parametrize("kind", DEVOX_CLOUDS)
@pytest.mark.parametrize("r", DEVOX_RS)
def test_single_slab_devoxelize_equals_oracle(bk, orc, devox_grids, r, kind):
    from lion_amd.fused_ops import devoxelize_affine
    g_all, g_other, sc_all, sh_all = devox_grids(r)
    rng = np.random.default_rng(gc.seed_of(f"small-devox-{r}-{kind}"))
    for ni, N in enumerate(NS):
        for ci, C in enumerate(CS):
            B = batch_of(ni, ci)
            assert gc.devox_path(B, C, N, r)["kernel"] == "slab" and gc.devox_path(B, C, N, r)["XS"] == 1
            co, ref_co, outside = devox_cloud(kind, r, B, N, rng)
            grid, other = np.ascontiguousarray(g_all[:B, :C]), np.ascontiguousarray(g_other[:B, :C])
            scale, shift = np.ascontiguousarray(sc_all[:B, :C]), np.ascontiguousarray(sh_all[:B, :C])
            o_out, o_inds, o_wgts = orc.trilinear_devoxelize_forward(r, True, ref_co, grid)
            o_aff = gc.devox_affine_expect(o_out, o_wgts, scale, shift)
            o_out[np.broadcast_to(outside[:, None, :], o_out.shape)] = 0.0
            o_aff[np.broadcast_to(outside[:, None, :], o_aff.shape)] = 0.0
            d_co, d_grid, d_other, d_sc, d_sh = dev(co), dev(grid), dev(other), dev(scale), dev(shift)
            what = f"B={B} C={C} N={N}"
            for run in (0, 1):
                plain, _, _ = bk.trilinear_devoxelize_forward(r, False, d_co, d_grid)
                same(plain, o_out, f"plain, run {run}, {what}")
                aff = devoxelize_affine(d_grid, d_co, r, d_sc, d_sh)
                same(aff, o_aff, f"affine, run {run}, {what}")
                devoxelize_affine(d_other, d_co, r, d_sh, d_sc)          # leaves another grid's bytes in LDS
            if kind != "outside":
                out, inds, wgts = bk.trilinear_devoxelize_forward(r, True, d_co, d_grid)
                same(inds, o_inds, f"inds, {what}")
                same(wgts, o_wgts, f"wgts, {what}")
                same(out, o_out, f"out (training), {what}")


def vox_cloud(kind, B, N, rng):
    co = gaussian_cloud(rng, B, N)
    if kind == "clump":
        co[:, :, : int(N * 0.98)] *= 0.08
    if kind == "one-voxel":
        co[:, :, 1:] = co[:, :, 1:] * 1e-4 + 0.3
    return co


def check_voxelize(bk, orc, r, co, feat, eps, what):
    """index plan, scatter, fused form and (r = 16) reader-aware scatter of one (cloud, features) pair against the oracle"""
    from lion_amd import _lib, fused_ops as fo
    lib = _lib.load()
    B, C, N = feat.shape
    o_nc, o_vc = orc.voxelize_coords(co, r, True, eps)
    o_out, o_ind, o_cnt = orc.avg_voxelize_forward(feat, o_vc, r)
    d_co, d_feat = dev(co), dev(feat)
    plan = bk.voxel_index(d_co, r, True, eps)
    assert plan is not None
    same(plan["norm"], o_nc, f"norm, {what}")
    same(plan["ind"], o_ind, f"ind, {what}")
    same(plan["cnt"], o_cnt, f"cnt, {what}")
    same(bk.voxel_scatter(d_feat, plan), o_out, f"scatter, {what}")
    f_out, f_nc, f_ind, f_cnt = bk.voxelize_points_forward(d_feat, d_co, r, True, eps)
    same(f_out, o_out, f"fused out, {what}")
    same(f_nc, o_nc, f"fused norm, {what}")
    same(f_ind, o_ind, f"fused ind, {what}")
    same(f_cnt, o_cnt, f"fused cnt, {what}")
    if r == 16:                                                   # the reader-aware scatter: equal where the reader stages
        occ1, _ = fo.conv3d_occupancy(plan["cnt"], r, 64, B)
        out = torch.full((B, C, r ** 3), -7.5, device="cuda")
        ws = plan["ws"]
        _lib.check(lib.lion_voxel_scatter_read(_lib.ptr(d_feat), _lib.ptr(ws), ws.numel(), B, C, N, r, _lib.ptr(occ1),
                                               _lib.ptr(out), _lib.stream_ptr(d_feat.device)), "voxel_scatter_read")
        nt = (r // 4) * (r // 4)
        occ_t = ((occ1[:B * nt] & 0xf) != 0).view(B, 1, r // 4, r // 4).float()
        rows = occ_t.repeat_interleave(4, 2).repeat_interleave(4, 3)
        need = torch.nn.functional.max_pool2d(rows, 3, 1, 1)[:, 0].bool()
        need_v = host(need.view(B, 1, r, r, 1).expand(B, C, r, r, r).reshape(B, C, r ** 3))
        got = host(out)
        same(got[need_v], o_out[need_v], f"reader-aware scatter, {what}")
        assert (got[~need_v] == -7.5).all(), f"reader-aware scatter wrote outside the reader's rows, {what}"


@pytest.mark.parametrize("kind", VOX_CLOUDS)
@pytest.mark.parametrize("r", VOX_RS)
def test_small_grid_voxelize_equals_oracle(bk, orc, r, kind):
    """N = 1 (one occupied voxel, every clamp of the scatter's prologue at 0) is normalised with eps = 1e-3: with eps = 0 the
    normalisation is 0 / 0, in the reference too"""
    rng = np.random.default_rng(gc.seed_of(f"small-vox-{r}-{kind}"))
    f_all = rng.standard_normal((3, max(CS), max(NS)), dtype=np.float32)
    for ni, N in enumerate(NS):
        for ci, C in enumerate(CS):
            B = batch_of(ni, ci)
            co = vox_cloud(kind, B, N, rng)
            feat = np.ascontiguousarray(f_all[:B, :C, :N])
            check_voxelize(bk, orc, r, co, feat, 1e-3 if N == 1 else 0.0, f"B={B} C={C} N={N}")


def scatter_channel_ranges(B, C, N, r):
    """(channel ranges per slab before, after the coarsening) of voxel_scatter_impl for N <= 1024 (csrc/voxelize.hip)"""
    r3, S = r ** 3, 1
    while S < 16 and B * S < 512 and r3 // (S * 2) >= 512 and r3 % (S * 2 * 4) == 0:
        S *= 2
    SV, CS0 = r3 // S, 1
    while B * S * CS0 < 512 and C // (CS0 * 2) >= 8:
        CS0 *= 2
    CS1 = CS0
    while CS1 > 1 and SV * gc.cdiv(C, CS1) < 8192 and B * S * (CS1 // 2) >= 256:
        CS1 //= 2
    return CS0, CS1


@pytest.mark.parametrize("kind", ("gauss", "clump"))
@pytest.mark.parametrize("C,N,r,split", [(128, 256, 8, (16, 8)), (192, 64, 8, (16, 8)), (128, 1024, 16, (2, 2))])
def test_scatter_channel_split_at_the_step_batch(bk, orc, C, N, r, split, kind):
    """B = 32, the batch of the sampling step: the r = 8 scatters take the coarsened channel split (16 ranges -> 8, which a
    batch below 32 never reaches), the r = 16 scatter keeps its two ranges"""
    B = 32
    assert scatter_channel_ranges(B, C, N, r) == split
    rng = np.random.default_rng(gc.seed_of(f"split-{C}-{N}-{r}-{kind}"))
    co = vox_cloud(kind, B, N, rng)
    feat = rng.standard_normal((B, C, N), dtype=np.float32)
    check_voxelize(bk, orc, r, co, feat, 0.0, f"B={B} C={C} N={N}")
