"""CPU suite of the guided-synthesis inputs: tests/perturb_ref.py -- the oracle the GPU tests hold csrc/perturb.hip to -- against
properties that do not depend on it (occupancy recomputed with np.unique on integer indices, face counts known in closed form),
the C entry points' refusals, which return before any launch, and the Python API's ValueErrors, which fire before a device is
touched."""
import ctypes

import numpy as np
import pytest
import torch

import perturb_ref as ref
from abi_check import declared_bound_and_exported

EINVAL = -1
SEED = 0x1234567890ABCDEF          # the seed of the "every face is hit" case; checked here on the CPU, reused on the GPU
NEW = ("lion_voxel_surface_workspace_bytes", "lion_voxel_surface_points_keyed", "lion_perturb_points_keyed")
TWO_VOXELS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32)      # two x-adjacent voxels at r = 2


def _occupied(x, r):
    """the occupied voxels of cloud x as a set of (ix, iy, iz), from float64 arithmetic on the box the reference reports and
    np.unique on the integer indices -- valid for clouds whose points sit well inside their cells or are clamped"""
    lo, s, _ = ref.box(x, r)
    idx = np.clip(np.floor((np.asarray(x, np.float64) - lo.astype(np.float64)) / float(s)).astype(np.int64), 0, r - 1)
    return {tuple(v) for v in np.unique(idx, axis=0)}


def _check_on_exposed_faces(x, r, K, seed, strict=True):
    """every point lies on a face of an occupied voxel whose neighbour across it is empty or outside the grid: exact in index
    arithmetic.  The grid coordinate along the face's axis is the integer i or i + 1; along the other two the real i + u lies
    in [i, i + 1) and its float32 rounding in [i, i + 1] (strict: the upper end is not reached under this seed)."""
    pts, F, aux = ref.voxel_surface_points(x, r, K, seed)
    occ = _occupied(x, r)
    for k in range(K):
        v, f, t = tuple(int(c) for c in aux["voxel"][k]), int(aux["face"][k]), aux["grid"][k]
        assert v in occ, (k, v)
        a, d = f >> 1, (1 if f & 1 else -1)
        nb = list(v)
        nb[a] += d
        assert not (0 <= nb[a] < r) or tuple(nb) not in occ, (k, v, f)
        assert float(t[a]) == v[a] + (f & 1), (k, t, v, f)
        for b in range(3):
            if b != a:
                assert v[b] <= float(t[b]) <= v[b] + 1 and (not strict or float(t[b]) < v[b] + 1), (k, t, v)
    # the points are the grid coordinates mapped through the box, one product and one sum
    want = (aux["lo"].astype(np.float64) + aux["grid"].astype(np.float64) * float(aux["s"]))
    assert np.abs(pts.astype(np.float64) - want).max() <= 2.0 ** -22 * max(1.0, np.abs(want).max())
    return pts, F, aux


# ---- the restatement against independent properties --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", [("gauss", 8), ("gauss", 32), ("shell", 16), ("shell", 1), ("boundary", 8), ("gauss7", 2)])
def test_points_lie_on_exposed_faces(name, r):
    x = {"gauss": ref.gaussian_cloud(64, 1), "gauss7": ref.gaussian_cloud(7, 2), "shell": ref.shell_cloud(2048, 3),
         "boundary": ref.boundary_cloud(r)}[name]
    if name == "boundary":      # points ON cell boundaries: float64 and float32 floors agree because 2/r and r/2 are exact here
        assert {tuple(v) for v in ref.voxel_indices(x, r)} == _occupied(x, r)
        assert ref.voxel_indices(x, r).max() == r - 1 and np.floor((x.max() + 1.0) * r / 2.0) == r     # the clamp is exercised
    _, F, aux = _check_on_exposed_faces(x, r, 300, SEED + r)
    assert F >= 6
    assert len(np.unique(aux["face"])) == 6 or r > 1 or F == 6


def test_face_counts_in_closed_form():
    one = np.array([[0.3, -1.2, 2.5]], dtype=np.float32)
    for x in (one, np.repeat(one, 7, axis=0)):                      # h = 0: the box is the cube of half-side 1 around the point
        for r in (1, 2, 5, 32):
            pts, F, aux = _check_on_exposed_faces(x, r, 64, SEED)
            assert F == 6 and len({tuple(v) for v in aux["voxel"]}) == 1
            lo, s, _ = ref.box(x, r)
            assert np.array_equal(lo, one[0] - np.float32(1.0)) and s == np.float32(2.0) / np.float32(r)
    _, F, _ = _check_on_exposed_faces(ref.grid_cloud(2), 2, 256, SEED)            # a full 2 x 2 x 2
    assert F == 24
    _, F, _ = _check_on_exposed_faces(TWO_VOXELS, 2, 256, SEED)                   # two face-adjacent voxels
    assert F == 10


def test_solid_block_never_yields_its_centre():
    """A solid 3 x 3 x 3 block has 54 exposed faces and its centre voxel none.  The grid is the cube around the cloud's own
    bounding box, so the occupied voxels always reach both ends of the grid along the longest axis: a 3-wide block cannot lie
    strictly inside an 8-wide grid with nothing else in it.  Two forms of the case therefore: the block as the whole grid
    (r = 3, F = 54), and the block inside r = 8 together with the two corner voxels that pin the box (they touch nothing:
    F = 54 + 2 * 6)."""
    _, F, aux = _check_on_exposed_faces(ref.grid_cloud(3), 3, 2048, SEED)
    assert F == 54 and not (aux["voxel"] == 1).all(1).any()
    x = ref.lattice_cloud(8, ref.block_cells(2, 3))
    assert _occupied(x, 8) == {tuple(c) for c in ref.block_cells(2, 3)} | {(0, 0, 0), (7, 7, 7)}
    _, F, aux = _check_on_exposed_faces(x, 8, 2048, SEED)
    assert F == 66 and not (aux["voxel"] == 3).all(1).any()
    inner = (aux["voxel"] >= 2).all(1) & (aux["voxel"] <= 4).all(1)
    assert abs(inner.mean() - 54 / 66) < 0.05                      # faces are drawn uniformly: 54 of 66 lie on the block


def test_every_face_of_two_voxels_is_hit():
    _, F, aux = ref.voxel_surface_points(TWO_VOXELS, 2, 4096, SEED)
    assert F == 10
    hit = {(tuple(v), int(f)) for v, f in zip(aux["voxel"], aux["face"])}
    assert len(hit) == 10
    assert ((0, 1, 1), 1) not in hit and ((1, 1, 1), 0) not in hit  # the shared face is not exposed from either side
    counts = np.bincount(ref.exposed_faces(TWO_VOXELS, 2).searchsorted(aux["voxel"] @ [24, 12, 6] + aux["face"]), minlength=10)
    assert counts.min() > 4096 / 10 * 0.8                           # and uniformly: 410 expected, sd 19


def test_uniform_noise_restatement():
    x = ref.gaussian_cloud(2048, 5)
    out, _ = ref.perturb_points(x, 0, 0.05, SEED)
    d = out.astype(np.float64) - x
    assert np.abs(d).max() <= 0.05 + 1e-6 and np.abs(d).max() > 0.049
    assert abs(d.mean()) < 5 * 0.05 / np.sqrt(3 * 6144) and abs(d.std() - 0.05 / np.sqrt(3)) < 1e-3
    assert np.array_equal(ref.perturb_points(x, 0, 0.0, SEED)[0], x)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_outlier_restatement(p):
    x = ref.gaussian_cloud(2048, 6)
    out, hit = ref.perturb_points(x, 1, p, SEED)
    w3 = ref.point_words(len(x), ref.PERTURB_STEP_WORD, 0, SEED)[:, 3].astype(np.int64)
    thr = min(int(np.floor(float(np.float32(p)) * 2.0 ** 32)), 2 ** 32 - 1)
    assert ref.outlier_threshold(p) == thr
    assert int(hit.sum()) == int((w3 < thr).sum())                  # the replaced fraction is that count, exactly
    assert np.array_equal(out[~hit].view(np.int32), x[~hit].view(np.int32))       # untouched points: bit-equal
    mn, mx = x.min(0), x.max(0)
    assert (out[hit] >= mn).all() and (out[hit] <= mx).all()        # replaced points: inside the clean bounding box
    moved = (out != x).any(1)
    assert not (moved & ~hit).any()
    if p == 0.0:
        assert not hit.any()
    elif p == 1.0:
        assert hit.all()
    else:
        assert abs(hit.mean() - p) < 5 * np.sqrt(p * (1 - p) / len(x))


def test_streams_do_not_share_words():
    a = ref.point_words(64, ref.VOXEL_STEP_WORD, 0, SEED)
    assert not np.array_equal(a, ref.point_words(64, ref.PERTURB_STEP_WORD, 0, SEED))
    assert not np.array_equal(a, ref.point_words(64, ref.VOXEL_STEP_WORD, 1, SEED))
    assert not np.array_equal(a, ref.point_words(64, ref.VOXEL_STEP_WORD, 0, SEED + 1))
    assert np.array_equal(a[:16], ref.point_words(16, ref.VOXEL_STEP_WORD, 0, SEED))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_exported_and_step_words_reserved():
    import os
    import re
    from lion_amd import chain, perturb
    declared_bound_and_exported(NEW[:1], returns="size_t")
    declared_bound_and_exported(NEW[1:])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "lion_hip.h")).read()
    words = {name: int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+)u" % name, txt).group(1), 16)
             for name in ("LION_VOXEL_STEP_WORD", "LION_PERTURB_STEP_WORD", "LION_START_STEP_WORD", "LION_DIFFUSE_STEP_WORD")}
    assert len(set(words.values())) == 4 and min(words.values()) > 2 ** 31 - 1     # no chain step (an int row index) has one
    assert (perturb.VOXEL_STEP_WORD, perturb.PERTURB_STEP_WORD) == (words["LION_VOXEL_STEP_WORD"], words["LION_PERTURB_STEP_WORD"])
    assert (ref.VOXEL_STEP_WORD, ref.PERTURB_STEP_WORD) == (perturb.VOXEL_STEP_WORD, perturb.PERTURB_STEP_WORD)
    assert (chain.START_STEP_WORD, chain.DIFFUSE_STEP_WORD) == (words["LION_START_STEP_WORD"], words["LION_DIFFUSE_STEP_WORD"])


def einval_cases(lib):
    """[(what, return code)]: every refusal the header lists for the two entry points; no call gets as far as a launch, so the
    pointers are never dereferenced"""
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    need = lib.lion_voxel_surface_workspace_bytes(2, 64, 8, 64)

    def vox(x=a, B=2, N=64, r=8, keys=a, K=64, out=a, faces=a, ws=None, ws_bytes=need):
        return lib.lion_voxel_surface_points_keyed(x, B, N, r, keys, 0, K, out, faces, ws, ws_bytes, None)

    def per(mode=0, x=a, B=2, N=64, p0=0.5, keys=a, out=a):
        return lib.lion_perturb_points_keyed(mode, x, B, N, p0, keys, 0, out, None)

    cases = [("x", vox(x=None)), ("keys", vox(keys=None)), ("out", vox(out=None)), ("B = 0", vox(B=0)), ("B < 0", vox(B=-1)),
             ("B > 65535", vox(B=65536)), ("N = 0", vox(N=0)), ("N < 0", vox(N=-5)), ("K = 0", vox(K=0)), ("K < 0", vox(K=-1)),
             ("r = 0", vox(r=0)), ("r < 0", vox(r=-2)), ("r = 33", vox(r=33)),
             ("perturb x", per(x=None)), ("perturb keys", per(keys=None)), ("perturb out", per(out=None)),
             ("perturb B = 0", per(B=0)), ("perturb B > 65535", per(B=65536)), ("perturb N = 0", per(N=0)),
             ("perturb mode 2", per(mode=2)), ("perturb mode -1", per(mode=-1)), ("perturb p0 < 0", per(p0=-0.1)),
             ("perturb p0 nan", per(p0=float("nan"))), ("outlier p0 > 1", per(mode=1, p0=1.5))]
    if need:                                                        # a workspace is asked for: too small, or missing
        cases += [("ws too small", vox(ws=a, ws_bytes=need - 1)), ("ws NULL", vox(ws=None, ws_bytes=need))]
    return cases


def test_entry_points_refuse_bad_arguments_before_launching():
    from lion_amd import _lib
    lib = _lib.load()
    cases = einval_cases(lib)
    assert len(cases) >= 24
    for what, rc in cases:
        assert rc == EINVAL, what
    for shape in ((1, 1, 1, 1), (32, 2048, 32, 2048), (65535, 1 << 20, 32, 1 << 20)):
        assert lib.lion_voxel_surface_workspace_bytes(*shape) == 0  # every table of r <= 32 lives in LDS


# ---- the Python API: ValueError before a device is touched ---------------------------------------------------------------------------
def test_api_refuses_bad_arguments_without_a_device():
    from lion_amd import editing, perturb
    x = torch.zeros(3, 8, 3)                                        # a CPU tensor: anything past the checks would raise RuntimeError
    for bad in (0, 33, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="resolution"):
            perturb.voxel_surface_points(x, bad, seeds=[1, 2, 3])
    for seeds in ([1, 2], [1, 2, 3, 4], torch.zeros(2, 2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            perturb.voxel_surface_points(x, 8, seeds=seeds)
        with pytest.raises(ValueError):
            perturb.add_noise(x, "uniform", 0.1, seeds=seeds)
    with pytest.raises(ValueError, match="seeds cannot be combined"):
        perturb.voxel_surface_points(x, 8, seeds=[1, 2, 3], seed=4)
    with pytest.raises(ValueError, match="seeds cannot be combined"):
        perturb.add_noise(x, "outlier", 0.1, seeds=[1, 2, 3], seed=4)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_points"):
            perturb.voxel_surface_points(x, 8, bad, seeds=[1, 2, 3])
    for kind in ("gaussian", "", None, 0):
        with pytest.raises(ValueError, match="kind"):
            perturb.add_noise(x, kind, 0.1, seeds=[1, 2, 3])
    for kind in perturb.KINDS:
        for amount in (-0.1, float("nan")):
            with pytest.raises(ValueError, match="amount"):
                perturb.add_noise(x, kind, amount, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="outlier fraction"):
        perturb.add_noise(x, "outlier", 1.01, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="multiple of 4"):
        perturb.add_noise(torch.zeros(3, 7, 3), "normal", 0.1, seeds=[1, 2, 3])
    for shape in ((8, 3), (3, 8, 2), (3, 0, 3)):
        with pytest.raises(ValueError):
            perturb.voxel_surface_points(torch.zeros(shape), 8, seed=1)
    with pytest.raises(ValueError, match="float32"):
        perturb.add_noise(x.double(), "uniform", 0.1, seed=1)
    with pytest.raises(ValueError, match="resolution"):             # the wrapper's refusals are the wrapped functions'
        editing.voxel_guided(None, None, None, x, 64, 3, seeds=[1, 2, 3])
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="no CPU path"):          # good arguments reach the device check: there is no CPU path
        perturb.voxel_surface_points(x, 8, seeds=[1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        perturb.add_noise(x, "uniform", 0.1, seed=5)
    assert torch.equal(state, torch.get_rng_state())                # seeded calls leave torch's generator alone
