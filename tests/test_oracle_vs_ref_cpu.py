"""Pins oracle/lion_oracle.c against the reference's OWN kernel bodies executed on the CPU
(oracle/_ref/libref.so, built by oracle/ref_build.py from the reference tree with a fiber-based CUDA
execution shim).  Index / integer outputs and every atomics-free float output must be identical;
outputs the reference accumulates with atomicAdd are order-dependent there, so they are compared
bit-exactly only where one thread owns one point (n <= 512) and with 1e-6 otherwise.

The reference's outputs of every call are recorded in tests/golden/oracle_vs_ref.npz, with a digest of the inputs they
were computed from: the suite needs neither the reference tree nor libref.so.  Where libref.so is built, re-record with
    LION_RECORD_REF=1 python -m pytest tests/test_oracle_vs_ref_cpu.py"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, gaussian_cloud, surface_cloud, voxel_coords

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref.so")
GOLD = os.path.join(GOLDEN, "oracle_vs_ref.npz")
RECORD = os.environ.get("LION_RECORD_REF") == "1"
_RECORDED = {}

fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    if RECORD:
        np.savez_compressed(GOLD, **_RECORDED)


@pytest.fixture()
def ref(request):
    """ref(name, scalars, inputs, outputs): the reference kernel `name` of libref.so, called as
    name(*scalars, *inputs, *outputs) with the arrays as pointers; fills `outputs` in place.  Replays the recorded
    outputs unless LION_RECORD_REF=1, which runs libref.so and records them."""
    lib = C.CDLL(SO) if RECORD else None
    gold = None if RECORD else np.load(GOLD)
    n = [0]

    def call(name, scalars, inputs, outputs):
        tag = f"{request.node.name}/{n[0]}/{name}"
        n[0] += 1
        inputs = [np.ascontiguousarray(a) for a in inputs]
        assert all(a.dtype in (np.float32, np.int32) for a in inputs + list(outputs))
        dig = _digest(inputs)
        if RECORD:
            ptrs = [a.ctypes.data_as(fp if a.dtype == np.float32 else ip) for a in inputs + list(outputs)]
            getattr(lib, name)(*scalars, *ptrs)
            _RECORDED[tag + "/inputs"] = np.array(dig)
            for j, o in enumerate(outputs):
                _RECORDED[f"{tag}/out{j}"] = o.copy()
        else:
            assert str(gold[tag + "/inputs"]) == dig, f"{tag}: inputs differ from the ones the outputs were recorded for"
            for j, o in enumerate(outputs):
                o[...] = gold[f"{tag}/out{j}"]
    yield call
    if gold is not None:
        gold.close()


@pytest.mark.parametrize("C_,N,r", [(5, 300, 8), (3, 512, 16), (6, 256, 8), (4, 2048, 32), (2, 1300, 16)])
def test_voxelize(ref, orc, C_, N, r):
    rng = np.random.default_rng(N)
    B = 2
    vc = np.rint(voxel_coords(rng, B, N, r, "surface")).astype(np.int32)
    feat = rng.standard_normal((B, C_, N)).astype(np.float32)
    o_out, o_ind, o_cnt = orc.avg_voxelize_forward(feat, vc, r)
    out = np.empty_like(o_out); ind = np.empty_like(o_ind); cnt = np.empty_like(o_cnt)
    ref("ref_avg_voxelize_forward", (B, C_, N, r), (vc, feat), (ind, cnt, out))
    assert np.array_equal(ind, o_ind) and np.array_equal(cnt, o_cnt)
    if N <= 512 and (N & (N - 1)) == 0:  # one point per thread: accumulation order == point order
        assert np.array_equal(out, o_out)
    else:
        np.testing.assert_allclose(out, o_out, rtol=1e-6, atol=1e-6)
    gy = rng.standard_normal((B, C_, r ** 3)).astype(np.float32)
    gx = np.empty((B, C_, N), np.float32)
    ref("ref_avg_voxelize_backward", (B, C_, N, r ** 3), (gy, ind, cnt), (gx,))
    assert np.array_equal(gx, orc.avg_voxelize_backward(gy, o_ind, o_cnt))


@pytest.mark.parametrize("C_,N,r", [(6, 400, 8), (4, 512, 8), (3, 1500, 16)])
def test_devoxelize(ref, orc, C_, N, r):
    rng = np.random.default_rng(N + 1)
    B = 2
    co = voxel_coords(rng, B, N, r)
    co[:, :, :3] = np.array([[0.0, r - 1.0, 2.0]] * 3, np.float32)
    feat = rng.standard_normal((B, C_, r ** 3)).astype(np.float32)
    o_out, o_i, o_w = orc.trilinear_devoxelize_forward(r, True, co, feat)
    out = np.empty_like(o_out); inds = np.empty_like(o_i); wgts = np.empty_like(o_w)
    ref("ref_trilinear_devoxelize_forward", (B, C_, N, r, 1), (co, feat), (inds, wgts, out))
    assert np.array_equal(inds, o_i) and np.array_equal(wgts, o_w) and np.array_equal(out, o_out)
    gy = rng.standard_normal((B, C_, N)).astype(np.float32)
    gx = np.empty((B, C_, r ** 3), np.float32)
    ref("ref_trilinear_devoxelize_backward", (B, C_, N, r ** 3), (gy, inds, wgts), (gx,))
    o_gx = orc.trilinear_devoxelize_backward(gy, o_i, o_w, r)
    if N <= 512 and (N & (N - 1)) == 0:
        assert np.array_equal(gx, o_gx)
    else:
        np.testing.assert_allclose(gx, o_gx, rtol=1e-5, atol=1e-5)


def test_ball_query_grouping_gather(ref, orc):
    rng = np.random.default_rng(3)
    B, N, M, U, C_ = 2, 700, 90, 16, 5
    pts = (gaussian_cloud(rng, B, N) * 0.4).astype(np.float32)
    ctr = pts[:, :, :M].copy()
    for radius in (0.15, 0.4, 5.0, 1e-6):
        idx = np.empty((B, M, U), np.int32)
        ref("ref_ball_query", (B, N, M, C.c_float(radius), U), (ctr, pts), (idx,))
        assert np.array_equal(idx, orc.ball_query(ctr, pts, radius, U)), radius
    feat = rng.standard_normal((B, C_, N)).astype(np.float32)
    out = np.empty((B, C_, M, U), np.float32)
    ref("ref_grouping_forward", (B, C_, N, M, U), (feat, idx), (out,))
    assert np.array_equal(out, orc.grouping_forward(feat, idx))
    gy = rng.standard_normal((B, C_, M, U)).astype(np.float32)
    gx = np.empty((B, C_, N), np.float32)
    ref("ref_grouping_backward", (B, C_, N, M, U), (gy, idx), (gx,))
    np.testing.assert_allclose(gx, orc.grouping_backward(gy, idx, N), rtol=1e-5, atol=1e-5)
    i1 = np.ascontiguousarray(idx[:, :, 0])
    o = np.empty((B, C_, M), np.float32)
    ref("ref_gather_features_forward", (B, C_, N, M), (feat, i1), (o,))
    assert np.array_equal(o, orc.gather_features_forward(feat, i1))


@pytest.mark.parametrize("N,M", [(300, 64), (1300, 100), (2048, 256)])
def test_fps_including_tie_break(ref, orc, N, M):
    rng = np.random.default_rng(N)
    B = 2
    co = gaussian_cloud(rng, B, N)
    co[1, :, N // 2:] = co[1, :, : N - N // 2]  # exact duplicates -> exact distance ties
    idx = np.empty((B, M), np.int32)
    ref("ref_furthest_point_sampling", (B, N, M), (co,), (idx,))
    assert np.array_equal(idx, orc.furthest_point_sampling(co, M))


def test_fps_lattice_ties(ref, orc):
    g3 = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), 0).reshape(3, -1)
    co = np.concatenate([g3, g3, g3, g3], 1)[None].astype(np.float32)  # 864 points, heavy ties, N > 512
    rng = np.random.default_rng(0)
    co = np.ascontiguousarray(co[:, :, rng.permutation(co.shape[2])])
    idx = np.empty((1, 150), np.int32)
    ref("ref_furthest_point_sampling", (1, co.shape[2], 150), (co,), (idx,))
    assert np.array_equal(idx, orc.furthest_point_sampling(co, 150))


@pytest.mark.parametrize("N,M", [(500, 40), (200, 2), (64, 16)])
def test_three_nn(ref, orc, N, M):
    rng = np.random.default_rng(M)
    B, C_ = 2, 6
    pts, ctr = gaussian_cloud(rng, B, N), gaussian_cloud(rng, B, M)
    cf = rng.standard_normal((B, C_, M)).astype(np.float32)
    o_out, o_idx, o_w = orc.three_nn_interpolate_forward(pts, ctr, cf)
    idx = np.empty_like(o_idx); w = np.empty_like(o_w); out = np.empty_like(o_out)
    ref("ref_three_nn_interpolate_forward", (B, C_, M, N), (pts, ctr, cf), (idx, w, out))
    assert np.array_equal(idx, o_idx) and np.array_equal(w, o_w) and np.array_equal(out, o_out)
    gy = rng.standard_normal((B, C_, N)).astype(np.float32)
    gx = np.empty((B, C_, M), np.float32)
    ref("ref_three_nn_interpolate_backward", (B, C_, N, M), (gy, idx, w), (gx,))
    np.testing.assert_allclose(gx, orc.three_nn_interpolate_backward(gy, o_idx, o_w, M), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("B,N,M", [(4, 100, 200), (2, 700, 1300)])
def test_chamfer(ref, orc, B, N, M):
    rng = np.random.default_rng(N)
    x1, x2 = rng.random((B, N, 3)).astype(np.float32), rng.random((B, M, 3)).astype(np.float32)
    x2[0, 5] = x2[0, 600 % M]  # duplicate targets across 512-tiles: tie -> lowest index
    o = orc.chamfer_forward(x1, x2)
    d1 = np.empty((B, N), np.float32); d2 = np.empty((B, M), np.float32)
    i1 = np.empty((B, N), np.int32); i2 = np.empty((B, M), np.int32)
    ref("ref_chamfer_forward", (B, N, M), (x1, x2), (d1, d2, i1, i2))
    assert np.array_equal(i1, o[2]) and np.array_equal(i2, o[3])
    assert np.array_equal(d1, o[0]) and np.array_equal(d2, o[1])
    g1, g2 = rng.standard_normal((B, N)).astype(np.float32), rng.standard_normal((B, M)).astype(np.float32)
    gx1 = np.empty((B, N, 3), np.float32); gx2 = np.empty((B, M, 3), np.float32)
    ref("ref_chamfer_backward", (B, N, M), (x1, x2, g1, g2, i1, i2), (gx1, gx2))
    og1, og2 = orc.chamfer_backward(x1, x2, g1, g2, i1, i2)
    np.testing.assert_allclose(gx1, og1, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gx2, og2, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("B,N,M", [(2, 96, 96), (1, 200, 120), (33, 16, 16)])
def test_emd(ref, orc, B, N, M):
    """approxmatch (10 levels x 3 passes) and matchcost (512-thread partial sums + tree) bit for bit;
    B=33 exercises the reference's `for i = blockIdx.x; i < b; i += gridDim.x` loop over 32 blocks."""
    rng = np.random.default_rng(N + M)
    x1, x2 = rng.random((B, N, 3)).astype(np.float32), rng.random((B, M, 3)).astype(np.float32)
    o_match = orc.approxmatch(x1, x2)
    match = np.empty_like(o_match)
    ref("ref_approxmatch", (B, N, M), (x1, x2), (match,))
    assert np.array_equal(match, o_match)
    cost = np.empty((B,), np.float32)
    ref("ref_matchcost", (B, N, M), (x1, x2, match), (cost,))
    assert np.array_equal(cost, orc.matchcost(x1, x2, o_match))
    gc = rng.standard_normal((B,)).astype(np.float32)
    g1 = np.empty((B, N, 3), np.float32); g2 = np.empty((B, M, 3), np.float32)
    ref("ref_matchcost_backward", (B, N, M), (gc, x1, x2, match), (g1, g2))
    og1, og2 = orc.matchcost_backward(gc, x1, x2, o_match)
    assert np.array_equal(g1, og1)
    np.testing.assert_allclose(g2, og2, rtol=1e-5, atol=1e-6)
