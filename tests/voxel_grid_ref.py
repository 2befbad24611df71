"""numpy float32 restatement of the voxel-grid entry points of csrc/perturb.hip (the arithmetic stated in include/lion_hip.h:
lion_voxel_occupancy, lion_voxel_surface_points_grid_keyed, lion_voxel_iou).  numpy on the CPU; imports
tests/perturb_ref.py (the Philox words, the fractions) and nothing from lion_amd.  Every operation on a coordinate is one
float32 numpy operation; faces are found by listing them, counts by counting.  tests/test_voxel_grid_reference_cpu.py holds this
file to perturb_ref and to hand-counted cases; tests/test_voxel_grid_gpu.py holds the kernels to this file, bit for bit."""
import numpy as np

import perturb_ref as pref

F32 = np.float32
UNIT_FRAME = np.array([-1.0, -1.0, -1.0, 2.0], dtype=F32)


def own_frame(x):
    """f32 [4] = (lo_x, lo_y, lo_z, side): the cube around the middle of cloud x's bounding box, its side the box's longest
    (1 + 1 where the box is a point) -- the box rule of perturb_ref.box, with the side kept instead of s and inv"""
    mn, mx = pref.bounds(x)
    c = (mn + mx) * F32(0.5)
    h = ((mx - mn) * F32(0.5)).max()
    if h == 0:
        h = F32(1.0)
    lo = c - h
    side = F32(2.0) * h
    out = np.array([lo[0], lo[1], lo[2], side], dtype=F32)
    assert lo.dtype == F32 and np.asarray(side).dtype == F32
    return out


def occupancy(x, r, frame=None):
    """one cloud x [N, 3] -> (grid bool [r, r, r] indexed [x, y, z], frame f32 [4], clamped): every point's voxel in `frame`
    (None: the cloud's own), i = floor((p - lo) * inv) per axis with inv = r / side, ALWAYS clamped to 0 ... r-1; clamped is the
    number of points whose index the clamp changed on at least one axis"""
    frame = own_frame(x) if frame is None else np.asarray(frame, dtype=F32)
    lo, inv = frame[:3], F32(r) / frame[3]
    t = (np.asarray(x, dtype=F32) - lo) * inv
    assert t.dtype == F32
    raw = np.floor(t).astype(np.int64)
    idx = np.clip(raw, 0, r - 1)
    grid = np.zeros((r, r, r), dtype=bool)
    grid[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    return grid, frame, int((raw != idx).any(1).sum())


def exposed_faces(grid):
    """int64 [F]: the exposed faces of the grid as 6 * (flat voxel id) + f, ascending; f = 0..5 = -x, +x, -y, +y, -z, +z is
    exposed when the neighbour across it is empty or outside the grid.  Any non-zero entry is an occupied voxel."""
    occ = np.asarray(grid) != 0
    r = occ.shape[0]
    assert occ.shape == (r, r, r)
    pad = np.zeros((r + 2, r + 2, r + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = occ
    exposed = np.zeros((r, r, r, 6), dtype=bool)
    for f in range(6):
        a, d = f >> 1, (1 if f & 1 else -1)
        sl = [slice(1, r + 1)] * 3
        sl[a] = slice(1 + d, r + 1 + d)
        exposed[..., f] = occ & ~pad[tuple(sl)]
    return np.flatnonzero(exposed.reshape(-1))


def surface_points_from_grid(grid, frame, K, seed, stream_id=0):
    """one grid [r, r, r] in frame f32 [4] -> (points f32 [K, 3], F): point k on face (uint64(w0) * F) >> 32, its grid
    coordinate t as in perturb_ref.voxel_surface_points, out = lo + t * s with s = side / r.  F = 0 (an empty grid): every
    point is the frame's centre lo + side * 0.5."""
    frame = np.asarray(frame, dtype=F32)
    r = np.asarray(grid).shape[0]
    lo, side = frame[:3], frame[3]
    s = side / F32(r)
    faces = exposed_faces(grid)
    F = len(faces)
    if F == 0:
        centre = lo + side * F32(0.5)
        assert centre.dtype == F32
        return np.repeat(centre[None, :], K, axis=0), 0
    w = pref.point_words(K, pref.VOXEL_STEP_WORD, stream_id, seed)
    j = ((w[:, 0].astype(np.uint64) * np.uint64(F)) >> np.uint64(32)).astype(np.int64)
    v, f = faces[j] // 6, faces[j] % 6
    vox = np.stack([v // (r * r), (v // r) % r, v % r], 1)
    axis, plus = f >> 1, f & 1
    frac = np.stack([pref.u24(w[:, 1]), pref.u24(w[:, 2])], 1)
    t = np.empty((K, 3), dtype=F32)
    first = np.where(axis == 0, 1, 0)                            # the lower tangential axis takes u(w1), the other u(w2)
    for a in range(3):
        tang = vox[:, a].astype(F32) + np.where(a == first, frac[:, 0], frac[:, 1])
        t[:, a] = np.where(axis == a, (vox[:, a] + plus).astype(F32), tang)
    pts = lo[None, :] + t * s
    assert pts.dtype == F32
    return pts, F


def iou(a, b):
    """two grids [r, r, r] -> (iou f32, inter, union): counts of the voxels occupied in both / in either; iou = inter / union
    as one float32 division of the two counts (exact in float32: at most 32^3), 1 where the union is empty"""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    inter, union = int((a & b).sum()), int((a | b).sum())
    return (F32(1.0) if union == 0 else F32(inter) / F32(union)), inter, union


# ---- the grids of the tests (host-made, seeded) -------------------------------------------------------------------------------------

def random_grid(r, seed, density=0.3):
    return np.random.default_rng(seed).random((r, r, r)) < density


def corner_grid(r, c):
    """a single voxel, at corner c = 0 ... 7 (bit 2: x, bit 1: y, bit 0: z at r - 1): F = 6"""
    g = np.zeros((r, r, r), dtype=bool)
    g[(r - 1) * (c >> 2 & 1), (r - 1) * (c >> 1 & 1), (r - 1) * (c & 1)] = True
    return g


def checkerboard_grid(r):
    """voxels with even x + y + z: no two share a face, so every face of every occupied voxel is exposed"""
    i = np.arange(r)
    return (i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0
