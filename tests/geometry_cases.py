"""Case tables, cloud builders and references for the point-geometry kernels (csrc/devoxelize.hip, sampling.hip,
ball_query.hip, interpolate.hip, grouping.hip): every dispatch branch of their launchers and the tile edges inside the
kernels.  tests/test_geometry_paths_gpu.py runs the cases on the device; tests/test_geometry_cases_cpu.py runs every builder
against the CPU oracle and asserts that a case has the property it is named for (the launcher's choice recomputed from its
formulas, the hit pattern of a ball-query centre, the needed z-rows of a devoxelize cloud), so that a GPU test cannot pass
for the wrong reason.  NumPy only; imports nothing from lion_amd.

u = 2^-24 is the unit roundoff of fp32."""
from collections import namedtuple

import numpy as np

from conftest import gaussian_cloud, surface_cloud, voxel_coords

U32 = 2.0 ** -24

Case = namedtuple("Case", "id path p")   # p: dict of the case's parameters


def cdiv(a, b):
    return -(-a // b)


def seed_of(text):
    import zlib
    return zlib.crc32(text.encode()) & 0x7fffffff


# =============================================================================================================
# devoxelize forward: devox_plan of csrc/devoxelize.hip, line for line (lion_internal_devoxelize_path asks the library)
# =============================================================================================================

def devox_path(B, C, N, r, aligned=True):
    r2 = r * r
    if r == 32 and N <= 2048 and aligned:
        return {"kernel": "ring"}
    if r2 % 4 == 0 and N <= 2048 and r2 <= 4608 and aligned:
        planes_max = 9216 // r2
        PX = r if planes_max >= r else planes_max - 1
        XS = cdiv(r, PX)
        CI = min(9216 // (r2 * r), 16) if XS == 1 else 1
        ld0 = cdiv((CI * r2 * r if XS == 1 else (PX + 1) * r2) // 4, 256)
        ld = 1 if ld0 <= 1 else 2 if ld0 <= 2 else 4 if ld0 <= 4 else 9
        CT = 4 * CI
        while CT > CI and B * cdiv(C, CT) < 512:
            CT >>= 1
        return {"kernel": "slab", "PX": PX, "XS": XS, "CI": CI, "ld": ld, "CT": CT}
    pt, ct = cdiv(N, 256), 16
    while ct > 2 and B * pt * cdiv(C, ct) < 2048:
        ct >>= 1
    return {"kernel": "gather", "ct": ct}


KINDS = ("dense", "sparse", "plane", "lattice", "edges")
KIND_N = {"dense": 777, "sparse": 8, "plane": 300, "lattice": 300, "edges": 64}   # where the path does not fix N


def _sparse_points(r, b):
    """<= 8 hand-placed points per batch element.  Element 0 holds (0, 1, 0.5) and points like it only: integer x, odd
    integer y, z in [0, 1] -- each reads the first two floats of ONE odd z-row whose even neighbour nobody needs.  The
    permutations of (0, 1, 0.5) are in element 1 (they need row 0), corners and far cells in element 2."""
    e = float(r - 1)
    if b == 0:
        pts = [(0, 1, .5), (0, 1, 0), (0, 1, 1)]
        if r >= 6:
            pts += [(2, 3, .5), (e - 1, e, .25), (r // 2, 1, .75)]
    elif b == 1:
        pts = [(1, 0, .5), (.5, 0, 1), (.5, 1, 0), (0, .5, 1), (1, .5, 0), (0, 0, 0), (1, 1, .5), (.5, .5, .5)]
    else:
        pts = [(e, e, e), (e, 0, max(e - .5, 0)), (0, e, .25), (max(e - .5, 0), 1, .5), (e, e, 0), (0, 0, e),
               (e / 2, e / 2, e / 2)]
    a = np.array(pts, np.float32).T                       # [3, n]
    return np.clip(a, 0, e)


def devox_cloud(kind, r, B, N, PX, rng):
    """float32 [B, 3, N] voxel coordinates in [0, r - 1] (what Voxelization.forward hands to devoxelize)"""
    e = float(r - 1)
    if kind == "dense":
        return voxel_coords(rng, B, N, r)
    co = np.empty((B, 3, N), np.float32)
    for b in range(B):
        if kind == "sparse":
            a = _sparse_points(r, b % 3)
            co[b] = a[:, np.arange(N) % a.shape[1]]       # padded by repetition (a path that fixes N tiles the pattern)
        elif kind == "plane":                             # one integer x, two adjacent integer y (the lower one odd)
            x0 = (0, r // 2, r - 1)[b % 3] if r > 2 else 1
            y0 = 1 + 2 * (b % max(1, (r - 2) // 2)) if r > 2 else 0
            co[b, 0] = x0
            co[b, 1] = y0 + rng.integers(0, 2, N)
            co[b, 2] = rng.uniform(0, e, N)
            co[b, 1, :2] = y0
            co[b, 2, :2] = (0.5, 1.0) if r > 2 else (0.5, 0.25)
        elif kind == "lattice":                           # every fraction is 0: "hi = lo" on all three axes
            co[b] = rng.integers(0, r, (3, N))
        elif kind == "edges":                             # 0 and r - 1 on every axis: the 8 grid corners, then mixtures
            c = np.array([[(q >> 2) & 1, (q >> 1) & 1, q & 1] for q in range(8)], np.float32).T * e
            co[b] = rng.uniform(0, e, (3, N))
            pick = rng.integers(0, 3, (3, N))             # 0: keep, 1: -> 0, 2: -> r - 1
            pick[rng.integers(0, 3, N), np.arange(N)] = rng.integers(1, 3, N)   # at least one axis on an edge
            co[b][pick == 1] = 0
            co[b][pick == 2] = e
            co[b][:, :8] = c
        elif kind == "slab-edges":                        # x just below, on and half a cell above every slab's first plane
            XS = cdiv(r, PX)
            x = np.array([k * PX + d for k in range(XS) for d in (-2.0 ** -10, 0.0, 0.5)], np.float32)
            assert N == x.size
            co[b, 0] = x
            co[b, 1:] = rng.uniform(0, e, (2, N))
            co[b, 1:, ::5] = np.floor(co[b, 1:, ::5])
        else:
            raise ValueError(kind)
    return np.clip(co, 0, e).astype(np.float32)


def _devox_cases():
    cases = []

    def add(path, r, C, B=3, N=None, aligned=True, tag=""):
        pth = devox_path(B, C, N or 8, r, aligned)
        kinds = KINDS + (("slab-edges",) if pth.get("XS", 1) > 1 else ())
        for kind in kinds:
            n = N or (3 * pth["XS"] if kind == "slab-edges" else KIND_N[kind])
            cases.append(Case(f"devox-{path}-r{r}{tag}-{kind}", path,
                              dict(r=r, C=C, B=B, N=n, aligned=aligned, kind=kind, PX=pth.get("PX", r))))

    for r in (2, 6, 10, 12, 20):
        add("slab1", r, 37)
    for r, C, B in ((22, 7, 3), (24, 7, 3), (40, 7, 3), (66, 3, 2)):
        add("slabx", r, C, B)
    for r, C, B, N in ((5, 37, 3, None), (33, 7, 3, None), (68, 7, 2, None), (32, 7, 3, 2049), (16, 7, 3, 2500)):
        add("gather", r, C, B, N, tag=f"-n{N}" if N else "")
    for r in (16, 32):
        add("misaligned", r, 7, aligned=False)
    for C in (1021, 512, 256, 7):
        add("ct", 8, C, 2, 4096, tag=f"-c{C}")
    return cases


DEVOX_FWD = _devox_cases()
DEVOX_CT_OF_C = {1021: 16, 512: 8, 256: 4, 7: 2}


def devox_inputs(case):
    """coords [B,3,N], grid [B,C,r^3], scale / shift [B,C] of a forward case"""
    p = case.p
    rng = np.random.default_rng(seed_of(case.id))
    co = devox_cloud(p["kind"], p["r"], p["B"], p["N"], p["PX"], rng)
    grid = rng.standard_normal((p["B"], p["C"], p["r"] ** 3), dtype=np.float32)
    scale = rng.uniform(0.5, 1.5, (p["B"], p["C"])).astype(np.float32)
    shift = rng.standard_normal((p["B"], p["C"])).astype(np.float32)
    return co, grid, scale, shift


def devox_affine_expect(o_out, o_wgts, scale, shift):
    """scale * interp + shift * sum(w) in float32, the corner weights added in ascending order (the kernel's order)"""
    wsum = o_wgts[:, 0].copy()
    for k in range(1, 8):
        wsum = (wsum + o_wgts[:, k]).astype(np.float32)
    return ((o_out * scale[:, :, None]).astype(np.float32) + (shift[:, :, None] * wsum[:, None, :]).astype(np.float32)).astype(np.float32)


def devox_needed_rows(co_b, r):
    """bool [r*r]: the z-rows (x * r + y) a cloud [3, N] reads, with the reference's "hi = lo when the fraction is 0" rule"""
    need = np.zeros(r * r, bool)
    x0, y0 = np.floor(co_b[0]).astype(int), np.floor(co_b[1]).astype(int)
    x1 = np.minimum(x0 + (co_b[0] > x0), r - 1)
    y1 = np.minimum(y0 + (co_b[1] > y0), r - 1)
    for xa in (x0, x1):
        for ya in (y0, y1):
            need[xa * r + ya] = True
    return need


def devox_reads_split_piece(co_b, r):
    """r = 4k + 2: some point reads z = 0 or 1 of an odd z-row -- the two floats that share a 16-byte piece with the end of
    the row before -- while nobody needs that row before"""
    need = devox_needed_rows(co_b, r)
    x0, y0, z0 = (np.floor(co_b[a]).astype(int) for a in range(3))
    row = x0 * r + y0                                     # the (x_lo, y_lo) row of every point is always read at z_lo
    return bool(np.any((row % 2 == 1) & ~need[row - 1] & (z0 < 2)))


# ---- devoxelize backward: lion_trilinear_devoxelize_backward with devox_bwd_plan -------------------------------

def devox_bwd_path(r):
    r3 = r ** 3
    if r3 * 4 <= 128 * 1024 and r3 % 4 == 0:
        parts = 2 if r3 * 4 > 64 * 1024 else 1
        if r3 % (4 * parts):
            parts = 1
        return {"kernel": "lds", "parts": parts, "nt": 1024 if r3 >= 16384 else 256}
    return {"kernel": "atomic"}


DEVOX_BWD = [Case(f"devox-bwd-r{r}-{kind}", devox_bwd_path(r)["kernel"], dict(r=r, kind=kind, B=2, C=5, N=600))
             for r in (5, 34, 6, 26) for kind in ("surface", "hub")]


def devox_bwd_inputs(case):
    """coords [B,3,N] (surface cloud, or every point inside one voxel) and gy [B,C,N]; inds / wgts come from the oracle"""
    p = case.p
    rng = np.random.default_rng(seed_of(case.id))
    if p["kind"] == "hub":
        co = (np.float32(p["r"] // 2) + rng.uniform(0.05, 0.95, (p["B"], 3, p["N"]))).astype(np.float32)
    else:
        co = voxel_coords(rng, p["B"], p["N"], p["r"], "surface")
    gy = rng.standard_normal((p["B"], p["C"], p["N"]), dtype=np.float32)
    return co, gy


# =============================================================================================================
# scatter-add reference where the order of the sum is free
# =============================================================================================================

def scatter_ref(gy, idx, w, bins):
    """gy [B,C,S], idx int [B,E], w [B,E] or None; entry e adds w[e] * gy[:, e mod S] into bin clip(idx[e]).
    -> (float64 sum [B,C,bins], bound [B,C,bins]) with bound = (k + 1) u sum|w g| per bin of k entries: the worst-case
    error of k rounded fp32 products added in fp32 in any order (k - 1 additions, one rounding per product, and room for
    the second-order terms), so it needs no measurement."""
    B, C, S = gy.shape
    E = idx.shape[1]
    ref = np.zeros((B, C, bins))
    mag = np.zeros((B, C, bins))
    k = np.zeros((B, bins))
    src = np.arange(E) % S
    for b in range(B):
        ix = np.clip(idx[b], 0, bins - 1)
        t = gy[b].astype(np.float64)[:, src]
        if w is not None:
            t = t * w[b].astype(np.float64)[None, :]
        np.add.at(ref[b], (slice(None), ix), t)
        np.add.at(mag[b], (slice(None), ix), np.abs(t))
        np.add.at(k[b], ix, 1)
    return ref, (k[:, None, :] + 1) * U32 * mag


def within(got, ref, bound):
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= bound))


def scatter_lds_ct(B, C, bins):
    """channels per workgroup of scatter_rows / lion_three_nn_interpolate_backward; 0: the global-atomic fallback"""
    if bins * 4 > 64 * 1024:
        return 0
    ct = min((64 * 1024) // (bins * 4), 8, C)
    while ct > 1 and B * cdiv(C, ct) < 1024:
        ct >>= 1
    return ct


# (name, B, C, bins, expected channel tile); the entry counts are small: the tile choice does not depend on them
SCATTER_SHAPES = [("ct8", 4, 2050, 64, 8), ("ct5", 4, 1300, 3000, 5), ("atomic", 2, 3, 16400, 0)]
SCATTER = ([Case(f"scatter-group-{n}-{v}", "atomic" if ct == 0 else "lds", dict(op="group", B=B, C=C, bins=bins, ct=ct, var=v))
            for n, B, C, bins, ct in SCATTER_SHAPES for v in ("hub", "clamp")]
           + [Case(f"scatter-nn-{n}-{v}", "atomic" if ct == 0 else "lds", dict(op="nn", B=B, C=C, bins=bins, ct=ct, var=v))
              for n, B, C, bins, ct in SCATTER_SHAPES for v in ("hub", "clamp")]
           + [Case(f"scatter-gather-n16400-{v}", "atomic", dict(op="gather", B=2, C=3, bins=16400, ct=0, var=v))
              for v in ("hub", "clamp")])


def scatter_inputs(case):
    """group: gy [B,C,M,U], idx [B,M,U];  nn: gy [B,C,N], idx [B,3,N], w [B,3,N];  gather: gy [B,C,M], idx [B,M]
    -> (gy, idx, w or None).  hub: half of all entries fall into one bin; clamp: indices from -3 to bins + 2."""
    p = case.p
    rng = np.random.default_rng(seed_of(case.id))
    B, C, bins = p["B"], p["C"], p["bins"]
    shape = {"group": (B, 16, 5), "nn": (B, 3, 30), "gather": (B, 500)}[p["op"]]
    if p["bins"] >= 3000:
        shape = {"group": (B, 40, 10), "nn": (B, 3, 130), "gather": (B, 500)}[p["op"]]
    if p["var"] == "hub":
        idx = rng.integers(0, bins, shape)
        flat = idx.reshape(B, -1)
        flat[:, rng.permutation(flat.shape[1])[: flat.shape[1] // 2]] = bins - 3
    else:
        idx = rng.integers(-3, bins + 3, shape)
        idx.reshape(B, -1)[:, :4] = (-3, -1, bins, bins + 2)
    idx = idx.astype(np.int32)
    S = idx.reshape(B, -1).shape[1] // (3 if p["op"] == "nn" else 1)
    gy = rng.standard_normal((B, C, S), dtype=np.float32)
    w = rng.uniform(0.05, 1.0, shape).astype(np.float32) if p["op"] == "nn" else None
    if p["op"] == "group":
        gy = gy.reshape(B, C, shape[1], shape[2])
    return gy, idx, w


# =============================================================================================================
# furthest point sampling: lion_furthest_point_sampling of csrc/sampling.hip
# =============================================================================================================

def fps_path(N):
    for lim, ppt in ((256, 1), (512, 2), (1024, 4), (2048, 8), (4096, 16)):
        if N <= lim:
            return ("reg", ppt)
    return ("lds", 0) if N <= 32768 else ("unsupported", 0)


FPS = ([Case(f"fps-n{N}-m40", fps_path(N)[0], dict(N=N, M=40, kind="mixed"))
        for N in (255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2049, 4095, 4097)]
       + [Case("fps-n300-m300", "reg", dict(N=300, M=300, kind="mixed")),
          Case("fps-n4097-m300", "lds", dict(N=4097, M=300, kind="mixed")),
          Case("fps-n32768-m48", "lds", dict(N=32768, M=48, kind="mixed")),
          Case("fps-identical-n300-m10", "reg", dict(N=300, M=10, kind="identical")),
          Case("fps-five-distinct-n700-m12", "reg", dict(N=700, M=12, kind="five"))])
FPS_B = 3


def fps_cloud(case):
    """[3, 3, N].  mixed: element 0 a shuffled integer lattice with duplicates, 1 and 2 Gaussian; identical: one point
    N times (another one per element); five: five distinct points among N"""
    p = case.p
    N = p["N"]
    rng = np.random.default_rng(seed_of(case.id))
    co = gaussian_cloud(rng, FPS_B, N)
    if p["kind"] == "mixed":
        side = max(2, int((N / 2) ** (1 / 3)))            # side^3 <= N / 2 cells: at least half the points are duplicates
        co[0] = rng.integers(0, side, (3, N))
    elif p["kind"] == "identical":
        co[:] = co[:, :, :1].copy()
        co[1] = 0.0
    else:
        five = rng.standard_normal((FPS_B, 3, 5)).astype(np.float32)
        pick = rng.integers(0, 5, (FPS_B, N))
        pick[:, :5] = np.arange(5)
        for b in range(FPS_B):
            co[b] = five[b][:, pick[b]]
    return np.ascontiguousarray(co, np.float32)


def distinct_points(co_b):
    return np.unique(co_b.T, axis=0).shape[0]


# =============================================================================================================
# ball query: csrc/ball_query.hip -- tiles of 2048 points, steps of 64, first U hits in ascending index
# =============================================================================================================

BQ_N, BQ_M, BQ_B, BQ_RADIUS = 4200, 21, 2, 0.5
BQ_TILE = 2048
BQ_US = (1, 8, 64, 65, 100)
BQ_AT_RADIUS_POINT = 100     # the point at exactly the radius of the "at-radius" centre
BQ = ([Case(f"bq-placed-u{U}", "placed", dict(U=U)) for U in BQ_US]
      + [Case(f"bq-gauss-u{U}", "gauss", dict(U=U)) for U in BQ_US])
BQ_GAUSS_RADIUS = 0.08


def bq_patterns(U, rng):
    """21 (name, ascending hit indices), pairwise disjoint.  The first seven are the named ones.
    "first64" asks for U + 4 hits inside the first 64-point step; a step has 64 points, so from U = 61 on it is all 64."""
    hb = max(1, U // 2)
    pats = [("straddle", sorted([2047 - 2 * i for i in range(hb)] + [2048 + 2 * i for i in range(U)])),
            ("last-only", [BQ_N - 1]),
            ("first64", list(range(min(U + 4, 64)))),
            ("none", []),
            ("exact-tile-end", sorted(4095 - 2 * i for i in range(U))),
            ("cut-in-step", list(range(2693, 2693 + U + 20))),
            ("at-radius", [200, 4100]),
            ("later-tile-first", [4097, 4101, 4130]),
            ("second-tile-only", [2051 + 6 * i for i in range(5)]),
            ("partial-last-step", list(range(4160, 4199))),
            ("second-step-first", [64]),
            ("all-tiles-few", [70, 2300, 4150])]
    used = {BQ_AT_RADIUS_POINT}
    for _, h in pats:
        assert not used & set(h)
        used |= set(h)
    free = np.array(sorted(set(range(BQ_N)) - used))
    free = free[rng.permutation(free.size)]
    at = 0
    for i, n in enumerate([1, 3, U - 1, U, U + 1, 2 * U, 5, 40, 130]):
        pats.append((f"random{i}-{n}", sorted(int(v) for v in free[at:at + n])))
        at += n
    assert len(pats) == BQ_M
    return pats


def bq_placed_inputs(case):
    """-> centres [B,3,M], points [B,3,N], radius, per batch element the (name, hits) of every centre slot.
    Filler points are ~1000 away from every centre; centre pattern p sits at (10 (p + 1), 0, 0), "at-radius" at the
    origin; a hit is its centre plus an offset of length 0.05 .. 0.45 (radius 0.5)."""
    U = case.p["U"]
    rng = np.random.default_rng(seed_of(case.id))
    pats = bq_patterns(U, rng)
    ctr = np.zeros((BQ_B, 3, BQ_M), np.float32)
    pts = (rng.uniform(-1, 1, (BQ_B, 3, BQ_N)) + np.array([0, 1000.0, 0])[None, :, None]).astype(np.float32)
    plan = []
    for b in range(BQ_B):
        slots = []
        for j in range(BQ_M):
            pi = (j + 5 * b) % BQ_M                       # another wave / centre slot per batch element
            name, hits = pats[pi]
            pos = np.array([0.0 if name == "at-radius" else 10.0 * (pi + 1), 0.0, 0.0])
            ctr[b, :, j] = pos
            if hits:
                d = rng.standard_normal((3, len(hits)))
                d *= rng.uniform(0.05, 0.45, len(hits)) / np.linalg.norm(d, axis=0)
                pts[b][:, hits] = (pos[:, None] + d).astype(np.float32)
            if name == "at-radius":
                pts[b, :, BQ_AT_RADIUS_POINT] = (0.5, 0.0, 0.0)
            slots.append((name, hits))
        plan.append(slots)
    return ctr, pts, BQ_RADIUS, plan


def bq_gauss_inputs(case):
    rng = np.random.default_rng(seed_of(case.id))
    pts = (gaussian_cloud(rng, BQ_B, BQ_N) * 0.35).astype(np.float32)
    ctr = np.ascontiguousarray(pts[:, :, rng.permutation(BQ_N)[:BQ_M]])
    return ctr, pts, BQ_GAUSS_RADIUS


def sqdist3_f32(a, b):
    """common.h sqdist3 in NumPy float32, one rounding per operation: (dx dx + dy dy) + dz dz.  a [3, ...], b [3, ...]"""
    d = a.astype(np.float32) - b.astype(np.float32)
    q = d * d
    return (q[0] + q[1]) + q[2]


def bq_hits(ctr_b, pts_b, radius):
    """bool [M, N]: d2 < r2 with the strict '<' and r2 = radius * radius in float32"""
    r2 = np.float32(radius) * np.float32(radius)
    return sqdist3_f32(ctr_b[:, :, None], pts_b[:, None, :]) < r2


def bq_brute(ctr, pts, radius, U):
    """first U hits in ascending point index, the rest of a list repeats the first hit, no hit at all: zeros"""
    B, _, M = ctr.shape
    out = np.zeros((B, M, U), np.int32)
    for b in range(B):
        hit = bq_hits(ctr[b], pts[b], radius)
        for j in range(M):
            h = np.flatnonzero(hit[j])
            if h.size:
                out[b, j] = h[0]
                out[b, j, :min(U, h.size)] = h[:U]
    return out


# =============================================================================================================
# 3-NN search and interpolation: csrc/interpolate.hip
# =============================================================================================================

NN_MS = (1, 2, 3, 4, 5, 15, 16, 17, 2047, 2048, 2049, 4100)    # centres: quad split, 16-centre unroll, 2048-centre LDS tile
NN_NS = (1, 65, 300)                                            # points: 64 per workgroup
NN = [Case(f"nn-m{M}-n{N}-{kind}", "search", dict(M=M, N=N, kind=kind, B=2, C=5))
      for M in NN_MS for N in NN_NS for kind in ("gauss", "lattice")]
NN_CT = [Case(f"nn-interp-c{C}", "interp", dict(M=8, N=4096, kind="gauss", B=2, C=C)) for C in (1021, 512, 256, 7)]
NN_CAT = Case("nn-cat-c1000+5+16", "cat", dict(M=8, N=4096, kind="gauss", B=2, C=1000, C2=5, C3=16))


def interp_ct(B, C, N):
    pt, ct = cdiv(N, 256), 16
    while ct > 2 and B * pt * cdiv(C, ct) < 2048:
        ct >>= 1
    return ct


def nn_inputs(case):
    """points [B,3,N], centres [B,3,M], centre features [B,C,M].  lattice: integer centres (many coincide) and points on
    or half-way between lattice sites: most of the three nearest distances are exact ties"""
    p = case.p
    rng = np.random.default_rng(seed_of(case.id))
    B, N, M = p["B"], p["N"], p["M"]
    if p["kind"] == "gauss":
        pts, ctr = gaussian_cloud(rng, B, N), gaussian_cloud(rng, B, M)
    else:
        side = min(16, max(2, int(round(M ** (1 / 3)))))
        ctr = rng.integers(0, side, (B, 3, M)).astype(np.float32)
        pts = rng.integers(-1, side + 1, (B, 3, N)).astype(np.float32)
        pts[:, :, ::3] += 0.5
    cf = rng.standard_normal((B, p["C"], M), dtype=np.float32)
    return pts, ctr, cf


# =============================================================================================================
# grouping forward: grouping_launch / grouping_fwd_kernel of csrc/grouping.hip
# =============================================================================================================

def group_ct(B, C, M, U):
    et, ct = cdiv(cdiv(M * U, 4), 256), 16
    while ct > 1 and B * et * cdiv(C, ct) < 2048:
        ct >>= 1
    return ct


GROUP_STRADDLE = [Case(f"group-u{U}-m{M}-{'centers' if ctr else 'plain'}", "quad", dict(U=U, M=M, centers=ctr, B=2, C=5, N=37))
                  for U, M in ((3, 8), (6, 10), (5, 4), (1, 64)) for ctr in (False, True)]
GROUP_CLIP = Case("group-clipped-indices", "quad", dict(U=3, M=8, centers=False, B=2, C=5, N=37))
# C from the launcher's rule at (B, M, U) = (2, 8, 3): one workgroup column, so B * ceil(C / ct) >= 2048 decides
GROUP_CT = [Case(f"group-ct{ct}-c{C}", "ct", dict(U=3, M=8, centers=False, B=2, C=C, N=16, ct=ct))
            for ct, C in ((16, 16370), (8, 8190), (4, 4094), (2, 2047))]


def group_inputs(case):
    """feat [B,C,N] (coords [B,3,N] and centres [B,3,M] as well when the case has centres), idx int32 [B,M,U]"""
    p = case.p
    rng = np.random.default_rng(seed_of(case.id))
    B, C, N, M, U = p["B"], p["C"], p["N"], p["M"], p["U"]
    feat = rng.standard_normal((B, C, N), dtype=np.float32)
    idx = rng.integers(0, N, (B, M, U)).astype(np.int32)
    co = gaussian_cloud(rng, B, N)
    ctr = gaussian_cloud(rng, B, M)
    return feat, idx, co, ctr
