"""The case tables of tests/geometry_cases.py, checked without a GPU: every builder runs against the CPU oracle, the
launcher's choice (recomputed from the formulas of the .hip files) is the one a case is filed under, and a constructed
cloud has the property it is named for.  tests/test_geometry_paths_gpu.py runs exactly these cases on the device; none is
skipped or filtered there."""
import ctypes

import numpy as np
import pytest

import geometry_cases as gc


def ids(cases):
    return [c.id for c in cases]


# ---- devoxelize forward -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from lion_amd import _lib
    return _lib.load()


DEVOX_KINDS = ("ring", "slab", "gather")


def assert_devox_path_equals_library(lib, B, C, N, r, aligned):
    """gc.devox_path against lion_internal_devoxelize_path {kind, PX, XS, CI, ld, CT or ct, LDS bytes, grid.x}, field for
    field; the grid's x (not among the restatement's fields) is the workgroups over the channels, or over the points"""
    out = (ctypes.c_int32 * 8)()
    assert lib.lion_internal_devoxelize_path(B, C, N, r, int(aligned), out, None) == 0
    kind, PX, XS, CI, ld, ct, lds, gx = out
    want = gc.devox_path(B, C, N, r, aligned)
    assert DEVOX_KINDS[kind] == want["kernel"], (B, C, N, r, aligned, list(out), want)
    if want["kernel"] == "slab":
        assert dict(kernel="slab", PX=PX, XS=XS, CI=CI, ld=ld, CT=ct) == want, (B, C, N, r, list(out), want)
        assert gx == gc.cdiv(C, ct) and 2 * ld * 4096 < lds <= 160 * 1024
    elif want["kernel"] == "gather":
        assert (PX, XS, CI, ld, ct, lds, gx) == (0, 0, 0, 0, want["ct"], 0, gc.cdiv(N, 256)), (B, C, N, r, list(out), want)
    else:
        assert (PX, XS, CI, ld) == (0, 0, 0, 0) and gx == gc.cdiv(C, ct) and 144 * 1024 < lds <= 160 * 1024


@pytest.mark.parametrize("case", gc.DEVOX_FWD, ids=ids(gc.DEVOX_FWD))
def test_devox_path_equals_the_library_on_the_case_table(lib, case):
    p = case.p
    assert_devox_path_equals_library(lib, p["B"], p["C"], p["N"], p["r"], p["aligned"])


@pytest.mark.parametrize("r", sorted(set(range(2, 51, 2)) | {9, 15, 33}))
def test_devox_path_equals_the_library_across_every_threshold(lib, r):
    """ring (r = 32), slab (r^2 % 4 == 0, r^2 <= 4608, N <= 2048: one slab up to r = 20, LD 1 / 2 / 4 / 9, CI 16 .. 1, CT by
    B x C) and gather (odd r, N > 2048, unaligned; ct by B x C x N)"""
    for B in (1, 2, 8, 32, 64):
        for C in (1, 8, 17, 64, 128):
            for N in (1, 7, 1024, 1025, 2048, 2049, 4096, 8192, 8193):
                for aligned in (True, False):
                    assert_devox_path_equals_library(lib, B, C, N, r, aligned)


def test_devox_path_query_refuses_bad_arguments(lib):
    out = (ctypes.c_int32 * 8)()
    for args in ((0, 8, 64, 8, 1), (1, 0, 64, 8, 1), (1, 8, 0, 8, 1), (1, 8, 64, 0, 1)):
        assert lib.lion_internal_devoxelize_path(*args, out, None) == -1, args
    assert lib.lion_internal_devoxelize_path(1, 8, 64, 8, 1, None, None) == -1


def _paths(group):
    return [(c, gc.devox_path(c.p["B"], c.p["C"], c.p["N"], c.p["r"], c.p["aligned"])) for c in gc.DEVOX_FWD if c.path == group]


def test_devox_table_covers_what_it_claims():
    one = _paths("slab1")
    assert all(p["kernel"] == "slab" and p["XS"] == 1 for _, p in one)
    assert {c.p["r"] for c, _ in one} == {2, 6, 10, 12, 20}
    assert {p["CI"] for _, p in one} == {16, 9, 5, 1}          # r = 2 and 6: 16, r = 10: 9, r = 12: 5, r = 20: 1
    assert {p["ld"] for _, p in one} == {1, 4, 9}              # LD = 4 is r = 6 alone
    assert all(p["CT"] == p["CI"] and c.p["C"] % p["CI"] for c, p in one if p["CI"] > 1)  # a last, shorter channel group
    many = _paths("slabx")
    assert all(p["kernel"] == "slab" and p["XS"] > 1 and p["CI"] == 1 and p["ld"] == 9 for _, p in many)
    assert {(c.p["r"], p["PX"], p["XS"]) for c, p in many} == {(22, 18, 2), (24, 15, 2), (40, 4, 10), (66, 1, 66)}
    assert {c.p["kind"] for c, _ in many} == set(gc.KINDS) | {"slab-edges"}
    by_shape = _paths("gather")
    assert all(p["kernel"] == "gather" for _, p in by_shape)
    assert {(c.p["r"], c.p["N"] > 2048) for c, _ in by_shape} == {(5, False), (33, False), (68, False), (32, True), (16, True)}
    mis = _paths("misaligned")
    assert {c.p["r"] for c, _ in mis} == {16, 32} and all(p["kernel"] == "gather" for _, p in mis)
    assert all(gc.devox_path(c.p["B"], c.p["C"], c.p["N"], c.p["r"], True)["kernel"] != "gather" for c, _ in mis)
    tiles = _paths("ct")
    assert all(p["kernel"] == "gather" and p["ct"] == gc.DEVOX_CT_OF_C[c.p["C"]] for c, p in tiles)
    assert {p["ct"] for _, p in tiles} == {16, 8, 4, 2}
    assert all(c.p["C"] % 2 for c in gc.DEVOX_FWD if c.path != "ct")   # C no multiple of any channel tile (16, 8, 4, 2)
    assert {c.p["C"] for c, _ in tiles} == {1021, 512, 256, 7}
    for group in ("slab1", "slabx", "gather", "misaligned", "ct"):
        assert {c.p["kind"] for c, _ in _paths(group)} >= set(gc.KINDS)
    assert len({c.id for c in gc.DEVOX_FWD}) == len(gc.DEVOX_FWD)


@pytest.mark.parametrize("case", gc.DEVOX_FWD, ids=ids(gc.DEVOX_FWD))
def test_devox_cloud_is_what_its_name_says(orc, case):
    p = case.p
    r, B, N, kind = p["r"], p["B"], p["N"], p["kind"]
    co, grid, scale, shift = gc.devox_inputs(case)
    assert co.dtype == np.float32 and co.shape == (B, 3, N) and co.min() >= 0 and co.max() <= r - 1   # the contract
    if kind == "sparse":
        assert np.unique(co[0].T, axis=0).shape[0] <= 8
        assert any(np.array_equal(co[0, :, i], np.array([0, 1, .5], np.float32)) for i in range(N))
    if kind == "plane":
        for b in range(B):
            ys = np.unique(co[b, 1])
            assert np.unique(co[b, 0]).size == 1 and ys.size == 2 and ys[1] - ys[0] == 1
    if kind == "lattice":
        assert np.array_equal(co, np.floor(co))
    if kind == "edges":
        assert np.all(((co == 0) | (co == r - 1)).any(axis=1))
        assert np.unique(co[0, :, :8].T, axis=0).shape[0] == 8 and np.all((co[0, :, :8] == 0) | (co[0, :, :8] == r - 1))
        for a in range(3):
            assert (co[:, a] == 0).any() and (co[:, a] == r - 1).any()
    if kind == "slab-edges":
        PX, XS = p["PX"], gc.cdiv(r, p["PX"])
        for k in range(1, XS):
            assert {np.float32(k * PX - 2.0 ** -10), np.float32(k * PX), np.float32(min(k * PX + 0.5, r - 1))} <= set(co[0, 0])
    if kind in ("sparse", "plane") and r % 4 == 2:
        need = gc.devox_needed_rows(co[0], r)
        assert np.any(need[1:] & ~need[:-1]), "no needed z-row behind a row nobody needs"
        if kind == "sparse" or r > 2:   # (a plane of two adjacent y at r = 2 is rows 2 and 3: no odd row stands alone)
            assert gc.devox_reads_split_piece(co[0], r)
    out, inds, wgts = orc.trilinear_devoxelize_forward(r, True, co, grid)
    assert inds.min() >= 0 and inds.max() < r ** 3
    assert np.abs(wgts.sum(1) - 1).max() < 1e-6 and np.isfinite(out).all()
    # the oracle itself against the interpolation written out in float64 from its indices and weights
    b, c = B - 1, p["C"] - 1
    ref = (grid[b, c].astype(np.float64)[inds[b]] * wgts[b]).sum(0)
    mag = (np.abs(grid[b, c].astype(np.float64)[inds[b]]) * wgts[b]).sum(0)
    assert np.all(np.abs(out[b, c] - ref) <= 9 * gc.U32 * mag + 1e-30)
    assert np.isfinite(gc.devox_affine_expect(out, wgts, scale, shift)).all()


# ---- devoxelize backward ------------------------------------------------------------------------------------

def test_devox_bwd_table_covers_what_it_claims():
    assert gc.devox_bwd_path(5) == {"kernel": "atomic"} and 5 ** 3 % 4                      # by divisibility
    assert gc.devox_bwd_path(34) == {"kernel": "atomic"} and 34 ** 3 % 4 == 0               # by size
    assert gc.devox_bwd_path(6) == {"kernel": "lds", "parts": 1, "nt": 256}
    assert gc.devox_bwd_path(26) == {"kernel": "lds", "parts": 2, "nt": 1024}
    assert {(c.p["r"], c.p["kind"]) for c in gc.DEVOX_BWD} == {(r, k) for r in (5, 34, 6, 26) for k in ("surface", "hub")}


def test_devox_bwd_affine_refusals(lib):
    """lion_trilinear_devoxelize_backward_affine refuses, before any launch, a slab above 128 KiB (r = 34), r3 % 8 != 0
    (r = 6: 216 is a multiple of 8, r = 5 and the plain entry's r3 = 16388 are not) and a misaligned x or dx; null pointers
    and empty shapes are LION_EINVAL.  (Host pointers: every call returns before it would touch them.)"""
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    f = lib.lion_trilinear_devoxelize_backward_affine
    call = lambda r3, x=ok, dx=ok, gy=ok: f(gy, ok, ok, x, ok, ok, ok, 1, 2, 64, r3, dx, None)
    assert call(34 ** 3) == -2 and call(125) == -2 and call(16388) == -2 and call(8 * 4096 + 4) == -2
    assert call(512, x=off) == -2 and call(512, dx=off) == -2
    assert call(512, gy=None) == -1 and call(0) == -1 and call(-8) == -1
    assert lib.lion_trilinear_devoxelize_backward(None, ok, ok, 1, 2, 64, 512, ok, None) == -1


@pytest.mark.parametrize("case", gc.DEVOX_BWD, ids=ids(gc.DEVOX_BWD))
def test_devox_bwd_oracle_is_inside_the_bound(orc, case):
    p = case.p
    co, gy = gc.devox_bwd_inputs(case)
    assert co.min() >= 0 and co.max() <= p["r"] - 1
    if p["kind"] == "hub":
        assert np.unique(np.floor(co).reshape(p["B"], 3, -1).transpose(1, 0, 2).reshape(3, -1).T, axis=0).shape[0] == 1
    _, inds, wgts = orc.trilinear_devoxelize_forward(p["r"], True, co, np.zeros((p["B"], 1, p["r"] ** 3), np.float32))
    ref, bound = gc.scatter_ref(gy, inds.reshape(p["B"], -1), wgts.reshape(p["B"], -1), p["r"] ** 3)
    if p["kind"] == "hub":
        assert np.count_nonzero(ref[0, 0]) == 8                 # the 8 corners of one cell, N entries each
    assert gc.within(orc.trilinear_devoxelize_backward(gy, inds, wgts, p["r"]), ref, bound)


# ---- legacy scatters ----------------------------------------------------------------------------------------

def scatter_oracle(orc, case, gy, idx, w):
    p = case.p
    ix = np.clip(idx, 0, p["bins"] - 1)                         # the oracle does not clamp; the kernels do
    if p["op"] == "group":
        return orc.grouping_backward(gy, ix, p["bins"])
    if p["op"] == "nn":
        return orc.three_nn_interpolate_backward(gy, ix, w, p["bins"])
    return orc.gather_features_backward(gy, ix, p["bins"])


@pytest.mark.parametrize("case", gc.SCATTER, ids=ids(gc.SCATTER))
def test_scatter_case_and_oracle(orc, case):
    p = case.p
    gy, idx, w = gc.scatter_inputs(case)
    B, bins = p["B"], p["bins"]
    assert gc.scatter_lds_ct(B, p["C"], bins) == p["ct"]
    assert (case.path == "atomic") == (bins > 16384)
    if p["ct"] == 8:
        assert p["C"] % 8                                       # a last, shorter channel group
    flat = idx.reshape(B, -1)
    if p["var"] == "hub":
        assert np.bincount(flat[0], minlength=bins).max() >= flat.shape[1] // 2
    else:
        assert (flat < 0).any() and (flat >= bins).any()
    g3 = gy.reshape(B, p["C"], -1)
    ref, bound = gc.scatter_ref(g3, flat, None if w is None else w.reshape(B, -1), bins)
    assert gc.within(scatter_oracle(orc, case, gy, idx, w), ref, bound)


def test_scatter_table_covers_what_it_claims():
    assert {(c.p["op"], c.p["ct"]) for c in gc.SCATTER} == {("group", 8), ("group", 5), ("group", 0), ("nn", 8), ("nn", 5),
                                                            ("nn", 0), ("gather", 0)}
    assert all({c.p["var"] for c in gc.SCATTER if c.p["op"] == op} == {"hub", "clamp"} for op in ("group", "nn", "gather"))


# ---- furthest point sampling --------------------------------------------------------------------------------

def test_fps_table_covers_what_it_claims():
    assert {gc.fps_path(c.p["N"]) for c in gc.FPS} == {("reg", 1), ("reg", 2), ("reg", 4), ("reg", 8), ("reg", 16), ("lds", 0)}
    assert all(gc.fps_path(c.p["N"])[0] == c.path for c in gc.FPS)
    for edge in (256, 512, 1024, 2048, 4096):                    # both sides of every threshold
        ns = {c.p["N"] for c in gc.FPS}
        assert ns & {edge - 1, edge} and edge + 1 in ns
    assert gc.fps_path(32768) == ("lds", 0) and gc.fps_path(32769) == ("unsupported", 0)


@pytest.mark.parametrize("case", gc.FPS, ids=ids(gc.FPS))
def test_fps_cloud_and_oracle(orc, case):
    p = case.p
    co = gc.fps_cloud(case)
    assert co.shape == (gc.FPS_B, 3, p["N"]) and co.dtype == np.float32
    distinct = [gc.distinct_points(co[b]) for b in range(gc.FPS_B)]
    if p["kind"] == "mixed":
        assert distinct[0] <= p["N"] // 2 and distinct[1] == p["N"]      # lattice with duplicates; Gaussian
    else:
        assert max(distinct) < p["M"]                                    # every remaining distance reaches 0
        assert distinct == ([1] * 3 if p["kind"] == "identical" else [5] * 3)
    idx = orc.furthest_point_sampling(co, p["M"])
    assert idx.min() >= 0 and idx.max() < p["N"] and np.all(idx[:, 0] == 0)
    for b in range(gc.FPS_B):                                            # as many distinct points as there are to take
        assert gc.distinct_points(co[b][:, idx[b]]) == min(p["M"], distinct[b])


# ---- ball query ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in gc.BQ if c.path == "placed"], ids=ids([c for c in gc.BQ if c.path == "placed"]))
def test_bq_placed_centres_have_their_patterns(orc, case):
    U, T = case.p["U"], gc.BQ_TILE
    ctr, pts, radius, plan = gc.bq_placed_inputs(case)
    assert pts.shape == (gc.BQ_B, 3, gc.BQ_N) and ctr.shape == (gc.BQ_B, 3, gc.BQ_M) and gc.BQ_N == 2 * T + 104
    seen = set()
    for b in range(gc.BQ_B):
        hit = gc.bq_hits(ctr[b], pts[b], radius)
        for j, (name, hits) in enumerate(plan[b]):
            assert np.flatnonzero(hit[j]).tolist() == hits, (b, j, name)
            h = np.array(hits)
            seen.add(name)
            if name == "straddle":
                assert (h < T).any() and (h >= T).any() and h.size > U
                assert U == 1 or np.count_nonzero(h < T) < U             # the count is carried into the second tile
            elif name == "last-only":
                assert hits == [gc.BQ_N - 1]
            elif name == "first64":
                assert h.size == min(U + 4, 64) and h.max() < 64
            elif name == "none":
                assert hits == []
            elif name == "exact-tile-end":
                assert h.size == U and h[-1] % T == T - 1
            elif name == "cut-in-step":
                assert h.size > U and (h[U - 1] % T) // 64 == (h[U] % T) // 64
            elif name == "at-radius":
                d2 = gc.sqdist3_f32(ctr[b, :, j], pts[b, :, gc.BQ_AT_RADIUS_POINT])
                assert d2 == np.float32(radius) * np.float32(radius) and gc.BQ_AT_RADIUS_POINT not in hits
                assert np.all(ctr[b, :, j] == 0) and min(hits) > gc.BQ_AT_RADIUS_POINT
            elif name == "later-tile-first":
                assert h.min() >= 2 * T
            elif name == "partial-last-step":
                assert h.min() >= 2 * T + 64 and gc.BQ_N - (2 * T + 64) < 64
    assert {"straddle", "last-only", "first64", "none", "exact-tile-end", "cut-in-step", "at-radius"} <= seen
    assert np.array_equal(orc.ball_query(ctr, pts, radius, U), gc.bq_brute(ctr, pts, radius, U))


@pytest.mark.parametrize("case", [c for c in gc.BQ if c.path == "gauss"], ids=ids([c for c in gc.BQ if c.path == "gauss"]))
def test_bq_gauss_oracle_equals_brute_force(orc, case):
    U = case.p["U"]
    ctr, pts, radius = gc.bq_gauss_inputs(case)
    hit = gc.bq_hits(ctr[0], pts[0], radius)
    assert hit.any(axis=1).all()                                         # a centre is a point of the cloud
    tiles = [np.unique(np.flatnonzero(h)[:U] // gc.BQ_TILE).size for h in hit]
    assert U == 1 or max(tiles) > 1                                      # some list is filled from more than one tile
    assert np.array_equal(orc.ball_query(ctr, pts, radius, U), gc.bq_brute(ctr, pts, radius, U))


def test_bq_table_covers_what_it_claims():
    assert {(c.path, c.p["U"]) for c in gc.BQ} == {(k, U) for k in ("placed", "gauss") for U in (1, 8, 64, 65, 100)}


# ---- 3-NN ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gc.NN + gc.NN_CT + [gc.NN_CAT], ids=ids(gc.NN + gc.NN_CT + [gc.NN_CAT]))
def test_nn_case_and_oracle(orc, case):
    p = case.p
    pts, ctr, cf = gc.nn_inputs(case)
    assert pts.shape == (p["B"], 3, p["N"]) and ctr.shape == (p["B"], 3, p["M"])
    out, idx, w = orc.three_nn_interpolate_forward(pts, ctr, cf)
    assert idx.min() >= 0 and idx.max() < p["M"] and np.isfinite(out).all()
    if p["M"] >= 3:
        assert np.abs(w.sum(1) - 1).max() < 1e-5
        d = np.sort(gc.sqdist3_f32(pts[0][:, :, None], ctr[0][:, None, :]), axis=1)   # [N, M]
        got = np.sort(gc.sqdist3_f32(pts[0][:, None, :], ctr[0][:, idx[0]]), axis=0)   # [3, N]
        assert np.array_equal(got.T, d[:, :3])                           # the three smallest distances, whatever the ties
        if p["kind"] == "lattice" and p["M"] >= 4 and p["N"] >= 65:
            assert np.any(d[:, 2] == d[:, 3])                            # a tie across the cut
    if case.path == "interp":
        assert gc.interp_ct(p["B"], p["C"], p["N"]) == gc.DEVOX_CT_OF_C[p["C"]]
    if case.path == "cat":
        C1, C12 = p["C"], p["C"] + p["C2"]
        assert gc.interp_ct(p["B"], C12 + p["C3"], p["N"]) == 16
        assert C1 % 16 and C12 % 16 and C1 // 16 == C12 // 16           # both seams inside one channel tile


def test_nn_table_covers_what_it_claims():
    assert {(c.p["M"], c.p["N"], c.p["kind"]) for c in gc.NN} == {(M, N, k) for M in (1, 2, 3, 4, 5, 15, 16, 17, 2047, 2048, 2049, 4100)
                                                                 for N in (1, 65, 300) for k in ("gauss", "lattice")}
    assert {gc.interp_ct(c.p["B"], c.p["C"], c.p["N"]) for c in gc.NN_CT} == {16, 8, 4, 2}


# ---- grouping forward ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gc.GROUP_STRADDLE + [gc.GROUP_CLIP] + gc.GROUP_CT,
                         ids=ids(gc.GROUP_STRADDLE + [gc.GROUP_CLIP] + gc.GROUP_CT))
def test_group_case_and_oracle(orc, case):
    p = case.p
    feat, idx, co, ctr = gc.group_inputs(case)
    MU, U = p["M"] * p["U"], p["U"]
    assert MU % 4 == 0                                                   # the 16-byte path
    assert any(e // U != (e + 3) // U for e in range(0, MU, 4))          # a quad of slots reaches into the next centre
    if case.path == "ct":
        assert gc.group_ct(p["B"], p["C"], p["M"], U) == p["ct"] and p["C"] % p["ct"]
    out = orc.grouping_forward(feat, idx)
    assert out.shape == (p["B"], p["C"], p["M"], U)
    assert np.array_equal(out[1, 2, 3], feat[1, 2][idx[1, 3]])


def test_group_table_covers_what_it_claims():
    assert {(c.p["U"], c.p["M"], c.p["centers"]) for c in gc.GROUP_STRADDLE} == {(U, M, k) for U, M in ((3, 8), (6, 10), (5, 4), (1, 64))
                                                                                 for k in (False, True)}
    assert {gc.group_ct(c.p["B"], c.p["C"], c.p["M"], c.p["U"]) for c in gc.GROUP_CT} == {16, 8, 4, 2}
