"""numpy float32 restatement of csrc/perturb.hip (the arithmetic stated in include/lion_hip.h: lion_voxel_surface_points_keyed,
lion_perturb_points_keyed), and the clouds the tests run it on.  numpy on the CPU; imports nothing from lion_amd.  Every
operation on a coordinate is one float32 numpy operation (one IEEE rounding, as the kernels' *_rn helpers); faces are found by
listing them, not by the kernel's prefix sums and searches.  tests/test_perturb_reference_cpu.py holds this file to properties
that do not depend on it; tests/test_perturb_gpu.py holds the kernels to this file, bit for bit."""
import numpy as np

VOXEL_STEP_WORD, PERTURB_STEP_WORD = 0xFFFFFFFD, 0xFFFFFFFC
F32 = np.float32
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32-valued [n, 4], key (k0, k1) -> uint32 [n, 4]  (Salmon et al. 2011, ten rounds; as tests/train_norm_ref.py)"""
    c = np.asarray(ctr).astype(np.uint64)
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[:, 0]
        p1 = np.uint64(0xCD9E8D57) * c[:, 2]
        c = np.stack([((p1 >> s32) ^ c[:, 1] ^ k0) & _M32, p1 & _M32, ((p0 >> s32) ^ c[:, 3] ^ k1) & _M32, p0 & _M32], 1)
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c.astype(np.uint32)


def point_words(count, step_word, stream_id, seed):
    """uint32 [count, 4]: the Philox words of points 0 ... count-1 under the 64-bit `seed` at counter (point, 0, step word,
    stream_id) -- the counter layout of every keyed entry point"""
    n = np.arange(count, dtype=np.uint64)
    ctr = np.stack([n & _M32, n >> np.uint64(32), np.full(count, step_word, np.uint64), np.full(count, stream_id, np.uint64)], 1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def u24(w):
    """(w >> 8) * 2^-24 in float32: exact"""
    return (w >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def bounds(x):
    """per-axis min and max of x [N, 3]"""
    x = np.asarray(x, dtype=F32)
    return x.min(0), x.max(0)


def box(x, r):
    """(lo [3], s, inv) of the voxel grid of cloud x [N, 3] at resolution r"""
    mn, mx = bounds(x)
    c = (mn + mx) * F32(0.5)
    h = ((mx - mn) * F32(0.5)).max()
    if h == 0:
        h = F32(1.0)
    lo = c - h
    side = F32(2.0) * h
    return lo, side / F32(r), F32(r) / side


def voxel_indices(x, r):
    """int64 [N, 3]: the voxel of every point"""
    lo, _, inv = box(x, r)
    t = (np.asarray(x, dtype=F32) - lo) * inv
    assert t.dtype == F32
    return np.clip(np.floor(t).astype(np.int64), 0, r - 1)


def exposed_faces(x, r):
    """int64 [F]: the exposed faces of the voxelisation as 6 * (flat voxel id) + f, ascending"""
    idx = voxel_indices(x, r)
    occ = np.zeros((r, r, r), dtype=bool)
    occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    pad = np.zeros((r + 2, r + 2, r + 2), dtype=bool)         # outside the grid: empty
    pad[1:-1, 1:-1, 1:-1] = occ
    exposed = np.zeros((r, r, r, 6), dtype=bool)
    for f in range(6):
        a, d = f >> 1, (1 if f & 1 else -1)
        sl = [slice(1, r + 1)] * 3
        sl[a] = slice(1 + d, r + 1 + d)
        exposed[..., f] = occ & ~pad[tuple(sl)]
    return np.flatnonzero(exposed.reshape(-1))


def voxel_surface_points(x, r, K, seed, stream_id=0):
    """one cloud x [N, 3] -> (points f32 [K, 3], F, aux); aux: 'voxel' int64 [K, 3], 'face' int64 [K], 'grid' f32 [K, 3] (the
    grid coordinate t of every point), 'lo', 's'"""
    lo, s, _ = box(x, r)
    faces = exposed_faces(x, r)
    F = len(faces)
    w = point_words(K, VOXEL_STEP_WORD, stream_id, seed)
    j = ((w[:, 0].astype(np.uint64) * np.uint64(F)) >> np.uint64(32)).astype(np.int64)
    v, f = faces[j] // 6, faces[j] % 6
    vox = np.stack([v // (r * r), (v // r) % r, v % r], 1)
    axis, plus = f >> 1, f & 1
    frac = np.stack([u24(w[:, 1]), u24(w[:, 2])], 1)
    t = np.empty((K, 3), dtype=F32)
    for a in range(3):
        first = np.where(axis == 0, 1, 0)                        # the lower tangential axis takes u(w1), the other u(w2)
        tang = vox[:, a].astype(F32) + np.where(a == first, frac[:, 0], frac[:, 1])
        t[:, a] = np.where(axis == a, (vox[:, a] + plus).astype(F32), tang)
    pts = lo[None, :] + t * s
    assert pts.dtype == F32 and t.dtype == F32
    return pts, F, {"voxel": vox, "face": f, "grid": t, "lo": lo, "s": s}


def outlier_threshold(p0):
    """floor(p0 * 2^32) in double from the float32 p0, saturated at 2^32 - 1"""
    t = float(F32(p0)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def perturb_points(x, mode, p0, seed, stream_id=0):
    """one cloud x [N, 3] -> (out f32 [N, 3], replaced bool [N]); mode 0: uniform noise of half-width p0, mode 1: outliers with
    probability p0"""
    x = np.asarray(x, dtype=F32)
    w = point_words(len(x), PERTURB_STEP_WORD, stream_id, seed)
    u = np.stack([u24(w[:, a]) for a in range(3)], 1)
    if mode == 0:
        out = x + F32(p0) * (F32(2.0) * u - F32(1.0))
        assert out.dtype == F32
        return out, np.zeros(len(x), dtype=bool)
    mn, mx = bounds(x)
    hit = w[:, 3].astype(np.int64) < outlier_threshold(p0)
    repl = mn[None, :] + u * (mx - mn)[None, :]
    assert repl.dtype == F32
    return np.where(hit[:, None], repl, x), hit


# ---- the clouds of the tests (seeded, host-made, float32) -------------------------------------------------------------------------

def lattice_cloud(r, cells):
    """the centres of the given voxels (x, y, z) of an r^3 grid on [-1, 1]^3, plus the grid's two far corners so that the box
    is exactly that cube whatever the cells are -- corners that fall into voxels (0, 0, 0) and (r-1, r-1, r-1)"""
    cells = np.asarray(cells, dtype=np.float64)
    pts = -1.0 + (cells + 0.5) * (2.0 / r)
    return np.concatenate([pts, [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]]).astype(F32)


def block_cells(lo, n):
    """the voxels (x, y, z) of the solid n^3 block that starts at (lo, lo, lo)"""
    g = np.arange(n) + lo
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def grid_cloud(n):
    """the n^3 integer lattice 0 ... n-1 (n >= 2): its box is the lattice's own bounding cube, and at resolution n every voxel
    holds exactly one point (coordinate k lands at k*n/(n-1): inside cell k, the last one by the clamp)"""
    return block_cells(0, n).astype(F32)


def gaussian_cloud(N, seed):
    return np.random.default_rng(seed).standard_normal((N, 3)).astype(F32)


def shell_cloud(N, seed):
    """points on a sphere of radius 0.5, quantised to multiples of 1/8: many points per voxel and many equal points"""
    z = np.random.default_rng(seed).standard_normal((N, 3))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    return (np.round(z * 0.5 * 8) / 8).astype(F32)


def boundary_cloud(r):
    """points exactly on cell boundaries of the r^3 grid on [-1, 1]^3 (box: min -1, max 1, h = 1, s = 2/r exact for the r used)
    and on the box's max face, where floor gives r and the clamp brings it back to r - 1"""
    k = np.arange(r + 1, dtype=np.float64)
    edge = -1.0 + k * (2.0 / r)                                   # every boundary, the max face included
    pts = [np.stack([edge, np.full_like(edge, -1.0), np.full_like(edge, 1.0)], 1),
           np.stack([np.full_like(edge, 1.0), edge, edge[::-1]], 1),
           np.stack([edge, edge, edge], 1)]
    return np.concatenate(pts).astype(F32)
