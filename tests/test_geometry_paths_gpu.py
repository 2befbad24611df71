"""-m gpu: the point-geometry kernels -- devoxelize, furthest point sampling, ball query, 3-NN interpolation, grouping and
their backward scatters -- on every branch of their launchers and at the tile edges inside the kernels, one test function
per kernel path.  The cases, their builders and the reasons behind the shapes are in tests/geometry_cases.py;
tests/test_geometry_cases_cpu.py shows on the CPU that every case reaches the path and has the property it is named for.

Integer outputs and every forward float output: bit-equal to the CPU oracle (one IEEE rounding per written operation, in the
oracle's order).  Ball query: the oracle and a NumPy float32 restatement of the distance test.  Backward scatters (order of
the sum free): |got - float64 sum| <= (k + 1) 2^-24 sum|w g| per bin of k entries (geometry_cases.scatter_ref)."""
import numpy as np
import pytest
import torch

import geometry_cases as gc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def bk():
    from lion_amd.functional.backend import _backend
    _backend.lib  # loads the .so, raises if missing
    return _backend


def ids(cases):
    return [c.id for c in cases]


def of_path(cases, *paths):
    sel = [c for c in cases if c.path in paths]
    return pytest.mark.parametrize("case", sel, ids=ids(sel))


def same(got, want, what):
    got = host(got) if torch.is_tensor(got) else got
    bad = got != want
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


# ---- devoxelize forward: lion_trilinear_devoxelize_forward (training 0 / 1) and fused_ops.devoxelize_affine -------------------

def run_devox_forward(bk, orc, case):
    from lion_amd.fused_ops import devoxelize_affine
    p = case.p
    r = p["r"]
    co, grid, scale, shift = gc.devox_inputs(case)
    o_out, o_inds, o_wgts = orc.trilinear_devoxelize_forward(r, True, co, grid)
    d_co = dev(co)
    if p["aligned"]:
        d_grid = dev(grid)
    else:                                                   # a contiguous view that starts 4 bytes into a larger buffer
        buf = torch.empty(grid.size + 1, device="cuda")
        d_grid = buf[1:].view(grid.shape)
        d_grid.copy_(torch.from_numpy(grid))
    assert d_grid.is_contiguous() and d_grid.data_ptr() % 16 == (0 if p["aligned"] else 4)
    out, inds, wgts = bk.trilinear_devoxelize_forward(r, True, d_co, d_grid)
    same(inds, o_inds, "inds")
    same(wgts, o_wgts, "wgts")
    same(out, o_out, "out (training)")
    out_e, _, _ = bk.trilinear_devoxelize_forward(r, False, d_co, d_grid)
    same(out_e, o_out, "out (eval)")
    got = devoxelize_affine(d_grid, d_co, r, dev(scale), dev(shift))
    same(got, gc.devox_affine_expect(o_out, o_wgts, scale, shift), "affine")


@of_path(gc.DEVOX_FWD, "slab1")
def test_devox_slab_kernel_single_slab(bk, orc, case):
    """devox_slab_kernel with CI whole channel grids per LDS buffer: r = 2, 6, 10 have rows of 4k + 2 floats, whose 16-byte
    pieces straddle two z-rows (the `sparse` and `plane` clouds need an odd row and not the row before it)"""
    run_devox_forward(bk, orc, case)


@of_path(gc.DEVOX_FWD, "slabx")
def test_devox_slab_kernel_multi_slab(bk, orc, case):
    """devox_slab_kernel walking XS > 1 slabs of PX planes + 1 halo plane: points sorted by slab, bitmap offset by the slab"""
    run_devox_forward(bk, orc, case)


@of_path(gc.DEVOX_FWD, "gather")
def test_devox_gather_kernel_by_shape(bk, orc, case):
    """devox_fwd_kernel for odd r, r >= 68 and N > 2048"""
    run_devox_forward(bk, orc, case)


@of_path(gc.DEVOX_FWD, "misaligned")
def test_devox_gather_kernel_misaligned_grid(bk, orc, case):
    run_devox_forward(bk, orc, case)


@of_path(gc.DEVOX_FWD, "ct")
def test_devox_gather_kernel_channel_tiles(bk, orc, case):
    """devox_fwd_kernel<16 | 8 | 4 | 2>"""
    run_devox_forward(bk, orc, case)


# ---- devoxelize backward: lion_trilinear_devoxelize_backward ----------------------------------------------------------

def run_devox_backward(bk, orc, case):
    p = case.p
    co, gy = gc.devox_bwd_inputs(case)
    _, inds, wgts = orc.trilinear_devoxelize_forward(p["r"], True, co, np.zeros((p["B"], 1, p["r"] ** 3), np.float32))
    ref, bound = gc.scatter_ref(gy, inds.reshape(p["B"], -1), wgts.reshape(p["B"], -1), p["r"] ** 3)
    gx = host(bk.trilinear_devoxelize_backward(dev(gy), dev(inds), dev(wgts), p["r"]))
    err = np.abs(gx - ref)
    assert np.all(err <= bound), f"{np.count_nonzero(err > bound)} bins outside the bound, worst {err.max():.3g}"


@of_path(gc.DEVOX_BWD, "atomic")
def test_devox_backward_atomic_kernel(bk, orc, case):
    """devox_bwd_atomic_kernel: r^3 % 4 != 0 (r = 5), r^3 * 4 > 128 KiB (r = 34)"""
    run_devox_backward(bk, orc, case)


@of_path(gc.DEVOX_BWD, "lds")
def test_devox_backward_lds_kernel(bk, orc, case):
    """devox_bwd_lds_kernel: 256 threads and one part (r = 6), 1024 threads and two parts (r = 26)"""
    run_devox_backward(bk, orc, case)


def test_devox_backward_entry_off_the_cubes():
    """lion_trilinear_devoxelize_backward handed r3 itself.  16388 = 4 * 4097 floats lie above 64 KiB, where a slab is cut
    into two parts, but are no multiple of 8: the launcher goes back to ONE part (1024 threads, 65552 bytes of LDS) -- no
    cube reaches that branch.  729 = 9^3 is odd: the atomic fallback.  Indices over the whole range, both ends crowded and
    some out of range (clamped); same reference and bound as the cases above (geometry_cases.scatter_ref)."""
    from lion_amd import _lib
    assert gc.devox_bwd_path(9) == {"kernel": "atomic"} and 16388 * 4 > 64 * 1024 and 16388 % 4 == 0 and 16388 % 8 != 0
    B, C, N = 1, 2, 64
    for r3 in (16388, 729):
        rng = np.random.default_rng(gc.seed_of(f"devox-bwd-r3-{r3}"))
        inds = rng.integers(0, r3, (B, 8, N)).astype(np.int32)
        inds[:, :, :6] = r3 - 1
        inds[:, :, 6:12] = 0
        inds[:, 0, 12:14] = (-3, r3 + 5)
        wgts = rng.uniform(0, 1, (B, 8, N)).astype(np.float32)
        gy = rng.standard_normal((B, C, N), dtype=np.float32)
        ref, bound = gc.scatter_ref(gy, inds.reshape(B, -1), wgts.reshape(B, -1), r3)
        gx = torch.full((B, C, r3), float("nan"), device="cuda")
        _lib.call("lion_trilinear_devoxelize_backward", dev(gy), dev(inds), dev(wgts), B, C, N, r3, gx)
        err = np.abs(host(gx) - ref)
        assert np.all(err <= bound), f"r3 = {r3}: {np.count_nonzero(err > bound)} bins outside the bound, worst {err.max():.3g}"


# ---- furthest point sampling ------------------------------------------------------------------------------------------

def run_fps(bk, orc, case):
    co = gc.fps_cloud(case)
    same(bk.furthest_point_sampling(dev(co), case.p["M"]), orc.furthest_point_sampling(co, case.p["M"]), "idx")


@of_path(gc.FPS, "reg")
def test_fps_register_kernel(bk, orc, case):
    """fps_reg_kernel<1 | 2 | 4 | 8 | 16, 4> on both sides of every threshold; clouds with fewer distinct points than
    samples, where every remaining distance is 0 and the tie-break word alone decides (padding lanes take part)"""
    run_fps(bk, orc, case)


@of_path(gc.FPS, "lds")
def test_fps_lds_kernel(bk, orc, case):
    run_fps(bk, orc, case)


def test_fps_n32769_raises_and_leaves_idx_untouched(bk):
    from lion_amd import _lib
    N, M = 32769, 4
    assert gc.fps_path(N)[0] == "unsupported"
    co = torch.zeros(1, 3, N, device="cuda")
    idx = torch.full((1, M), -7, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError):
        _lib.call("lion_furthest_point_sampling", co, 1, N, M, idx)
    torch.cuda.synchronize()
    assert bool((idx == -7).all())
    with pytest.raises(RuntimeError):
        bk.furthest_point_sampling(co, M)


# ---- ball query -------------------------------------------------------------------------------------------------------

@of_path(gc.BQ, "placed")
def test_ball_query_placed_hits(bk, orc, case):
    """N = 4200 = 2048 + 2048 + 104: hits placed by index among filler points far from every centre"""
    U = case.p["U"]
    ctr, pts, radius, plan = gc.bq_placed_inputs(case)
    got = host(bk.ball_query(dev(ctr), dev(pts), radius, U))
    want = gc.bq_brute(ctr, pts, radius, U)
    for b in range(gc.BQ_B):
        for j, (name, _) in enumerate(plan[b]):
            assert np.array_equal(got[b, j], want[b, j]), f"cloud {b} centre {j} ({name}): {got[b, j][:8]} != {want[b, j][:8]}"
    same(got, orc.ball_query(ctr, pts, radius, U), "idx against the oracle")


@of_path(gc.BQ, "gauss")
def test_ball_query_gaussian_filler(bk, orc, case):
    U = case.p["U"]
    ctr, pts, radius = gc.bq_gauss_inputs(case)
    got = host(bk.ball_query(dev(ctr), dev(pts), radius, U))
    same(got, gc.bq_brute(ctr, pts, radius, U), "idx against the float32 restatement")
    same(got, orc.ball_query(ctr, pts, radius, U), "idx against the oracle")


# ---- 3-NN search and interpolation ------------------------------------------------------------------------------------

def run_nn(bk, orc, case):
    pts, ctr, cf = gc.nn_inputs(case)
    o_out, o_idx, o_w = orc.three_nn_interpolate_forward(pts, ctr, cf)
    out, idx, w = bk.three_nearest_neighbors_interpolate_forward(dev(pts), dev(ctr), dev(cf))
    same(idx, o_idx, "idx")
    same(w, o_w, "weights")
    same(out, o_out, "out")


@of_path(gc.NN, "search")
def test_three_nn_search(bk, orc, case):
    """three_nn_kernel: fewer centres than lanes of a quad / than the 16-centre unrolled step, one centre more or less than
    an LDS tile, a third tile; one point, one more than a wave of points; Gaussian centres and lattice centres with ties"""
    run_nn(bk, orc, case)


@of_path(gc.NN_CT, "interp")
def test_three_nn_interp_channel_tiles(bk, orc, case):
    """three_nn_interp_kernel<16 | 8 | 4 | 2>"""
    run_nn(bk, orc, case)


def test_three_nn_interp_cat_seams_inside_one_tile(bk, orc):
    """three_nn_interp_cat_kernel<16>: C1 = 1000 and C1 + C2 = 1005 fall into the channel tile 992..1007"""
    case = gc.NN_CAT
    p = case.p
    pts, ctr, cf = gc.nn_inputs(case)
    rng = np.random.default_rng(gc.seed_of(case.id) + 1)
    temb = rng.standard_normal((p["B"], p["C2"]), dtype=np.float32)
    skip = rng.standard_normal((p["B"], p["C3"], p["N"]), dtype=np.float32)
    both = np.concatenate([cf, np.broadcast_to(temb[:, :, None], (p["B"], p["C2"], p["M"]))], 1)
    o_out, o_idx, o_w = orc.three_nn_interpolate_forward(pts, ctr, both)
    out, idx, w = bk.three_nearest_neighbors_interpolate_cat_forward(dev(pts), dev(ctr), dev(cf), dev(temb), p["C2"], dev(skip))
    same(idx, o_idx, "idx")
    same(w, o_w, "weights")
    same(out, np.concatenate([o_out, skip], 1), "out")


# ---- grouping forward -------------------------------------------------------------------------------------------------

def run_group(bk, orc, case):
    from lion_amd import fused_ops as fo
    p = case.p
    feat, idx, co, ctr = gc.group_inputs(case)
    d_idx = dev(idx)
    want = orc.grouping_forward(feat, idx)
    if p["centers"]:
        rel = (orc.grouping_forward(co, idx) - ctr[:, :, :, None]).astype(np.float32)
        same(fo.group_points(dev(co), dev(ctr), dev(feat), d_idx), np.concatenate([rel, want], 1), "coords - centres ; features")
        same(fo.group_points(dev(co), dev(ctr), None, d_idx), rel, "coords - centres")
    else:
        same(bk.grouping_forward(dev(feat), d_idx), want, "out")


@of_path(gc.GROUP_STRADDLE, "quad")
def test_grouping_quads_straddle_centres(bk, orc, case):
    """grouping_fwd_kernel, 16-byte path (M U % 4 == 0) with U = 3, 6, 5, 1: the four slots of a lane belong to two, three or
    four centres; with `centers` (lion_group_points_forward) the four centre indices differ"""
    run_group(bk, orc, case)


def test_grouping_clipped_indices(bk, orc):
    """indices -3 and N + 5 read rows 0 and N - 1: the oracle on the clipped indices"""
    case = gc.GROUP_CLIP
    N = case.p["N"]
    feat, idx, _, _ = gc.group_inputs(case)
    idx[:, 0, 0], idx[:, 1, 1] = 0, N - 1
    r = np.where(idx == 0, -3, np.where(idx == N - 1, N + 5, idx)).astype(np.int32)
    assert (r == -3).any() and (r == N + 5).any()
    want = orc.grouping_forward(feat, np.clip(r, 0, case.p["N"] - 1))
    same(bk.grouping_forward(dev(feat), dev(r)), want, "out")


@of_path(gc.GROUP_CT, "ct")
def test_grouping_channel_tiles(bk, orc, case):
    """grouping_fwd_kernel<16 | 8 | 4 | 2> with a last, shorter channel tile"""
    run_group(bk, orc, case)


# ---- the legacy scatters of the C ABI: LDS rows with CT = 8 and CT = 5 channels, and their global-atomic fallbacks ----------------

def run_scatter(orc, case):
    from lion_amd import _lib
    p = case.p
    B, C, bins = p["B"], p["C"], p["bins"]
    gy, idx, w = gc.scatter_inputs(case)
    flat = idx.reshape(B, -1)
    ref, bound = gc.scatter_ref(gy.reshape(B, C, -1), flat, None if w is None else w.reshape(B, -1), bins)
    d_gy, d_idx = dev(gy), dev(idx)
    gx = torch.full((B, C, bins), float("nan"), device="cuda")
    lib, st = _lib.load(), _lib.stream_ptr(d_gy.device)
    if p["op"] == "group":
        M, U = idx.shape[1:]
        _lib.check(lib.lion_grouping_backward(_lib.ptr(d_gy), _lib.ptr(d_idx), B, C, bins, M, U, _lib.ptr(gx), st), case.id)
    elif p["op"] == "nn":
        d_w = dev(w)
        _lib.check(lib.lion_three_nn_interpolate_backward(_lib.ptr(d_gy), _lib.ptr(d_idx), _lib.ptr(d_w), B, C, idx.shape[2], bins,
                                                          _lib.ptr(gx), st), case.id)
    else:
        _lib.check(lib.lion_gather_features_backward(_lib.ptr(d_gy), _lib.ptr(d_idx), B, C, bins, idx.shape[1], _lib.ptr(gx), st),
                   case.id)
    got = host(gx)
    assert np.isfinite(got).all(), "bins left unwritten"
    err = np.abs(got - ref)
    assert np.all(err <= bound), f"{np.count_nonzero(err > bound)} bins outside the bound, worst {err.max():.3g}"


@of_path([c for c in gc.SCATTER if c.p["op"] == "group"], "lds")
def test_scatter_rows_lds_kernel(orc, case):
    run_scatter(orc, case)


@of_path([c for c in gc.SCATTER if c.p["op"] != "nn"], "atomic")
def test_scatter_rows_atomic_kernel(orc, case):
    """lion_grouping_backward and lion_gather_features_backward beyond 16384 bins"""
    run_scatter(orc, case)


@of_path([c for c in gc.SCATTER if c.p["op"] == "nn"], "lds")
def test_three_nn_interp_grad_kernel(orc, case):
    run_scatter(orc, case)


@of_path([c for c in gc.SCATTER if c.p["op"] == "nn"], "atomic")
def test_three_nn_interp_grad_atomic_kernel(orc, case):
    run_scatter(orc, case)


def test_no_case_is_left_out():
    """every case of the tables is a parameter of exactly one test above"""
    import sys
    mod = sys.modules[__name__]
    used = []
    for name in dir(mod):
        fn = getattr(mod, name)
        for m in getattr(fn, "pytestmark", []) if name.startswith("test_") else []:
            if m.name == "parametrize":
                used += [c.id for c in m.args[1]]
    table = [c.id for c in gc.DEVOX_FWD + gc.DEVOX_BWD + gc.FPS + gc.BQ + gc.NN + gc.NN_CT + gc.GROUP_STRADDLE + gc.GROUP_CT + gc.SCATTER]
    assert sorted(used) == sorted(table) and len(set(table)) == len(table)
