"""Case tables, cloud builders and references for the voxelisation kernels (csrc/voxelize.hip): every plan of vox_plan
(fused and scatter), the run-length edges of phase B2's double-buffered ordered sum, the wave-aggregated LDS counters, the
chunk adoption of the NP >= 2 scatter, the three fallback kernels and the backward.  tests/test_voxelize_paths_gpu.py runs
the cases on the device; tests/test_voxelize_cases_cpu.py runs every builder against the CPU oracle and asserts that a case
has the plan and the property it is named for, so that a GPU test cannot pass for the wrong reason.  NumPy only; imports
nothing from lion_amd.

The launcher arithmetic is restated line for line (each function names the function of lion_amd/csrc/voxelize.hip it
restates); the host calls lion_internal_voxelize_plan / lion_voxel_plan_bytes / lion_avg_voxelize_workspace_bytes check the
restatement in the CPU suite.

u = 2^-24 is the unit roundoff of fp32."""
from collections import namedtuple

import numpy as np

from conftest import gaussian_cloud

U32 = 2.0 ** -24

Case = namedtuple("Case", "id path p")   # p: dict of the case's parameters

VT = 1024                     # voxelize.hip: VT
MAXP = 8                      # MAXP
LDS_LIMIT = 160 * 1024        # LDS_LIMIT
PREFETCH_PAD = 2 * 16 * 4     # PREFETCH_PAD
CH_CAP = 64                   # CH_CAP
OUT_CAP_BYTES = 64 << 20      # the largest output grid of any case


def cdiv(a, b):
    return -(-a // b)


def align4(x):
    return (x + 3) & ~3


def seed_of(text):
    import zlib
    return zlib.crc32(text.encode()) & 0x7fffffff


# =============================================================================================================
# the launchers, line for line
# =============================================================================================================

def vox_plan(B, C, N, r):
    """vox_plan(kind = VOX_FUSED) of voxelize.hip.  `why` names the first reason a shape is not fast (None when it is)."""
    r3 = r * r * r
    two_per_cu = N <= VT
    wgs = 512 if two_per_cu else 256
    lds_limit = (LDS_LIMIT // 2 if two_per_cu else LDS_LIMIT) - PREFETCH_PAD
    S = 1
    while S < 16 and B * S < wgs and r3 // (S * 2) >= 512 and r3 % (S * 2 * 4) == 0:
        S *= 2
    CS = 1
    while B * S * CS < wgs and C // (CS * 2) >= 8:
        CS *= 2
    SV = r3 // S
    n_words = align4(N)
    NP = 1 if N <= VT else 2 if N <= 2 * VT else 4 if N <= 4 * VT else 8
    svp = ((SV + (SV >> 5) + 3) & ~3) + 4
    fixed = (svp + n_words + 64 + 32) * 4
    need_a = (svp + n_words) * 4
    nocc = min(N, SV)
    want = max((N + 1 + nocc) * (C if C > 0 else 1) * 4, need_a)
    avail = lds_limit - fixed if fixed < lds_limit else 0
    arena = min(want, avail)
    arena_words = arena // 4
    why = None                                                                  # in the order written there
    if r3 > (1 << 17):
        why = "r3"
    elif r3 % 4 or SV % 4:
        why = "odd"
    elif N > MAXP * VT or N < 1:
        why = "n"
    elif arena < need_a or arena_words < N + 1 + nocc:
        why = "lds"
    return dict(S=S, CS=CS, SV=SV, NP=NP, n_words=n_words, arena_words=arena_words, fast=why is None, two_per_cu=two_per_cu,
                why=why, lds=fixed + arena_words * 4 + PREFETCH_PAD, ws_bytes=(B * 3 * N * 4 + 255) & ~255)


def plan_bytes(B, N, r):
    """lion_voxel_plan_bytes with vox_plan_words"""
    p = vox_plan(B, 0, N, r)
    return B * (2 * N + p["S"] * (4 + 2 * align4(N))) * 4 if p["fast"] else 0


def slabs_of_plan_bytes(nbytes, B, N):
    """S recovered from plan_bytes / 4 = B (2 N + S (4 + 2 align4(N)))"""
    w, rem = divmod(nbytes // 4 - B * 2 * N, B * (4 + 2 * align4(N)))
    assert rem == 0 and nbytes % 4 == 0
    return w


def scatter_plan(B, C, N, r, read=False):
    """vox_plan(kind = VOX_SCATTER / VOX_SCATTER_READ) of voxelize.hip as voxel_scatter_impl asks for it -> dict(S, CS, SV, NP, n_words, arena_words) or None (LION_EUNSUPPORTED)"""
    p0 = vox_plan(B, C, N, r)
    if not p0["fast"]:
        return None
    S, CS, SV = p0["S"], p0["CS"], p0["SV"]
    two_per_cu = N <= VT
    if two_per_cu:
        CS = 1
        while B * S * CS < 512 and C // (CS * 2) >= 8:
            CS *= 2
        while CS > 1 and SV * cdiv(C, CS) < 8192 and B * S * (CS // 2) >= 256:
            CS //= 2
    lds_limit = (LDS_LIMIT // 2 if two_per_cu else LDS_LIMIT) - PREFETCH_PAD - (1024 + 64 if read else 0)
    fixed = (SV + p0["n_words"] + 64) * 4
    nocc = min(N, SV)
    want = (N + 1 + nocc) * C * 4
    avail = lds_limit - fixed if fixed < lds_limit else 0
    arena = min(want, avail)
    if arena // 4 < N + 1 + nocc:
        return None
    return dict(S=S, CS=CS, SV=SV, NP=p0["NP"], n_words=p0["n_words"], arena_words=arena // 4)


def ch_max_of(arena_words, pts, occ, C):
    """channels per chunk of a slab: ch_max of vox_means_and_store (and l_chm of vox_scatter_kernel)"""
    return min(CH_CAP, min(C, arena_words // ((pts | 1) + occ)) if pts > 0 else C)


def chunking(plan, pts, occ, C, cs=0):
    """The header block and the greedy adoption loop of vox_scatter_kernel for channel range `cs` of
    one cloud.  pts / occ: per slab.  -> (chm [S], nc [S], moves [(adopter, slab, chunk)], rem [S]: chunks left with the owner)"""
    S, CS = plan["S"], plan["CS"]
    c_per = cdiv(C, CS)
    cg_lo = cs * c_per
    cg_hi = min(C, cg_lo + c_per)
    chm = [ch_max_of(plan["arena_words"], pts[s], occ[s], C) for s in range(S)]
    nc = [cdiv(cg_hi - cg_lo, chm[s]) if pts[s] > 0 else 1 for s in range(S)]
    lanes = 16                                                                  # the xor butterfly spans lanes 0..15
    rem = [nc[s] if s < S else 0 for s in range(lanes)]                         # (l_nc = 0 in the lanes past S)
    ld2 = [1 if s < S and pts[s] == 0 else 0x7fffff for s in range(lanes)]
    taken = [0] * lanes
    moves = []
    if plan["NP"] >= 2 and any(pts[s] == 0 for s in range(S)):
        for _ in range(5 * 16):
            km = max((rem[s] << 8) | (63 - s) for s in range(lanes))
            ka = min((ld2[s] << 8) | s for s in range(lanes))
            smax, nmax, a_, la = 63 - (km & 0xff), km >> 8, ka & 0xff, ka >> 8
            if nmax < 2 or nmax > 256 or la + 2 >= 2 * nmax:
                break
            rem[smax] -= 1
            ld2[a_] += 2
            taken[a_] += 1
            if taken[a_] == 5:
                ld2[a_] = 0x7fffff
            moves.append((a_, smax, nmax - 1))
    return chm, nc, moves, rem[:S]


def slab_headers(vox_ids, plan):
    """per slab (points, occupied voxels) of one cloud from its voxel ids [N] (hdr of the index plan, written by vox_fused_kernel)"""
    r3 = plan["S"] * plan["SV"]
    v = np.clip(np.asarray(vox_ids, np.int64), 0, r3 - 1)
    pts, occ = [], []
    for s in range(plan["S"]):
        m = v[(v >= s * plan["SV"]) & (v < (s + 1) * plan["SV"])]
        pts.append(int(m.size))
        occ.append(int(np.unique(m).size))
    return pts, occ


def vox_ids(vox, r):
    """voxel ids [B, N] from integer coordinates [B, 3, N] (vox_fused_kernel without P1)"""
    v = vox.astype(np.int64)
    return v[:, 0] * r * r + v[:, 1] * r + v[:, 2]


def balanced_cloud(rest, r):
    """rest: voxel ids [N - 1] -> (voxel ids [N], float32 [3, N] raw coordinates that Voxelization.forward with normalize =
    False puts on them).  The forward subtracts the cloud's mean, so a cloud lands on chosen voxels only if the mean of its
    voxel coordinates is r / 2 on every axis: the first N - 1 points sit on the voxel centres 2 q / r - 1 of `rest`, and
    the LAST point is placed where it makes the mean r / 2 exactly -- usually far outside the grid, where it is clamped to
    a border voxel (x = 0 or r - 1: the first or the last slab).  The CPU suite checks the landing voxels against the oracle."""
    rest = np.asarray(rest, np.int64)
    N = rest.size + 1
    q = np.stack([rest // (r * r), (rest // r) % r, rest % r]).astype(np.float64)
    last = N * r / 2.0 - q.sum(1)
    u = np.concatenate([q, last[:, None]], 1)
    land = np.clip(np.rint(last), 0, r - 1).astype(np.int64)
    ids = np.concatenate([rest, [land[0] * r * r + land[1] * r + land[2]]])
    return ids, np.ascontiguousarray(2.0 * u / r - 1.0, np.float32)


def fill_slabs(spec, SV, N, rng):
    """voxel ids [N] of a cloud with spec[s] = (points, distinct voxels) in slab s, the point order shuffled"""
    ids = []
    for s, (pts, occ) in enumerate(spec):
        if pts == 0:
            continue
        assert 1 <= occ <= min(pts, SV)
        vs = s * SV + rng.permutation(SV)[:occ]
        ids.append(np.concatenate([vs, vs[rng.integers(0, occ, pts - occ)]]))
    ids = np.concatenate(ids)
    assert ids.size == N, (ids.size, N)
    return ids[rng.permutation(N)]


# =============================================================================================================
# A / B: the plans.  (B, C, N, r, cloud kind); a case is named S{S}-CS{CS}-NP{NP} and the shape it has them at
# =============================================================================================================

PLAN_SHAPES = [
    (3, 64, 2048, 32, "gauss"),          # S = 16
    (32, 16, 2048, 32, "clump"),         # S = 8, CS = 1: the plan of the workload's (32, 64, 2048, 32) on a 64-MiB grid
    (64, 2, 1200, 32, "gauss"),          # S = 4
    (128, 2, 64, 16, "gauss"),
    (128, 2, 1200, 32, "gauss"),         # S = 2
    (256, 2, 64, 16, "gauss"),
    (512, 2, 64, 16, "gauss"),           # S = 1 at r = 16
    (1, 8, 64, 12, "gauss"),             # S = 2 by divisibility
    (1, 8, 64, 14, "gauss"),
    (1, 8, 2048, 30, "gauss"),
    (1, 8, 64, 20, "gauss"),             # S = 8, SV = 1000
    (1, 8, 64, 24, "gauss"),             # S = 16, SV = 864
    (1, 8, 2048, 36, "gauss"),           # S = 16, SV = 2916
    (9, 8, 64, 8, "gauss"),              # 7 idle cloud slots of the second 8-group
    (1, 24, 3000, 16, "gauss"),          # NP = 4, ragged N
    (1, 40, 5000, 16, "clump"),          # NP = 8, ragged N
    (1, 8, 8192, 44, "gauss"),
    (2, 5, 1023, 8, "gauss"), (2, 5, 1024, 8, "gauss"), (2, 5, 1025, 8, "gauss"),
    (2, 5, 2048, 8, "gauss"), (2, 5, 2049, 8, "gauss"), (2, 5, 4096, 8, "gauss"), (2, 5, 4097, 8, "gauss"),
    (1, 64, 8192, 16, "oneslab"),        # ch_max < c_per: ~3 channels per chunk
    (1, 3, 8192, 48, "oneslab"),         # 1 channel per chunk
    (1, 17, 300, 16, "clump"),           # C % CS != 0, C no multiple of 16 / NP: NP = 1
    (2, 37, 1500, 16, "clump"),          # NP = 2
    (1, 7, 3000, 16, "gauss"),           # NP = 4
    (1, 3, 5000, 16, "gauss"),           # NP = 8
    (1, 1, 1, 2, "gauss"), (2, 5, 100, 2, "gauss"), (2, 5, 100, 4, "gauss"), (2, 5, 100, 6, "gauss"),
    (32, 128, 256, 8, "clump"),          # scatter: CS 16 -> 8
    (32, 192, 64, 8, "gauss"),
]


def _plan_cases():
    out = []
    for B, C, N, r, kind in PLAN_SHAPES:
        p = vox_plan(B, C, N, r)
        out.append(Case(f"S{p['S']}-CS{p['CS']}-NP{p['NP']}-b{B}c{C}n{N}r{r}-{kind}", "fused" if p["fast"] else "fallback",
                        dict(B=B, C=C, N=N, r=r, kind=kind, feat="normal")))
    return out


PLANS = _plan_cases()


# =============================================================================================================
# C: adoption (NP >= 2 scatter).  p["slabs"]: per slab (points, distinct voxels) of the first N - 1 points, the same for
# every cloud of the batch; the balancing point (balanced_cloud) lands in slab p["lands"] and makes it one point more.
# p["moves"]: what chunking() has to give for every channel range
# =============================================================================================================

def _adoption_cases():
    few = (40, 30)
    table = [
        # one crowded slab (2047 points in 512 voxels: 14 channels per chunk, 5 chunks), 6 empty slabs: four adopters
        ("many-adopters", 32, 64, 2048, 16, [(2047, 512)] + [(0, 0)] * 7, 7,
         [(1, 0, 4), (2, 0, 3), (3, 0, 2), (4, 0, 1)]),
        # one adopter (slab 14), 6 chunks in slab 15: it takes three
        ("one-adopter-three-chunks", 8, 64, 4096, 32, [(79, 60)] * 3 + [(78, 60)] * 11 + [(0, 0), (3000, 2048)], 0,
         [(14, 15, 5), (14, 15, 4), (14, 15, 3)]),
        # C < 16 -> CS = 1; 15 chunks of one channel in slab 15, one adopter (slab 14): it stops at five
        ("cap-of-five", 1, 15, 8192, 48, [(0, 0)] + [(1, 1)] * 13 + [(0, 0), (8178, 4800)], 0,
         [(14, 15, 14 - k) for k in range(5)]),
        # two crowded slabs (3 chunks each) with empties between
        ("two-crowded", 4, 12, 8192, 32, [(4000, 2048), (0, 0), (0, 0), few, (4071, 2048), (0, 0)] + [few] * 2 + [(0, 0)] * 8, 15,
         [(1, 0, 2), (2, 4, 2), (5, 0, 1), (8, 4, 1)]),
        # c_per = 30, 14 channels per chunk: chunks of 14 / 14 / 2, the 2-channel chunk is adopted first
        ("partial-last-chunk", 8, 120, 2048, 16, [(2047, 512)] + [(0, 0)] * 7, 7, [(1, 0, 2), (2, 0, 1)]),
        # no empty slab: nobody moves
        ("no-empty-slab", 8, 120, 2048, 16, [(1767, 512)] + [few] * 7, 7, []),
    ]
    out = []
    for name, B, C, N, r, slabs, lands, moves in table:
        assert sum(s[0] for s in slabs) == N - 1
        out.append(Case(f"adopt-{name}", "adopt", dict(B=B, C=C, N=N, r=r, kind="slabs", slabs=slabs, lands=lands, moves=moves,
                                                       feat="normal")))
    return out


ADOPT = _adoption_cases()


# =============================================================================================================
# D: run lengths of phase B2.  One slab holds voxels of exactly 1, 2, ..., 3 PW + 3 points (PW = 8 for NP 1 / 8, 16 for
# NP 2 / 4: every edge n = 8 / 9, PW, PW + 1, PW + 2, 2 PW + 1, 3 PW + 1 is among them), fillers elsewhere
# =============================================================================================================

def pw_of(NP):
    return 16 if NP in (2, 4) else 8                                            # PW of vox_means_and_store


def run_edges(NP):
    PW = pw_of(NP)
    return sorted({8, 9, PW, PW + 1, PW + 2, 2 * PW + 1, 3 * PW + 1})


RUNS = ([Case(f"runs-staircase-NP{NP}", "runs", dict(B=1, C=5, N=N, r=16, kind="staircase", top=3 * pw_of(NP) + 3, long=0,
                                                    feat="wide"))
         for NP, N in ((1, 1024), (2, 2048), (4, 4096), (8, 8192))]
        + [Case("runs-long-NP8", "runs", dict(B=1, C=3, N=8192, r=16, kind="staircase", top=0, long=8191, feat="wide")),
           Case("runs-long-NP2", "runs", dict(B=1, C=5, N=2048, r=16, kind="staircase", top=9, long=1900, feat="wide"))])
STAIR_SLAB = 3


def staircase_ids(p, rng):
    """slab 3: voxels of 1 .. top points (and one of `long` points); the rest of the first N - 1 points in the slabs behind
    it, so that the balancing point lands in slab 0"""
    plan = vox_plan(p["B"], p["C"], p["N"], p["r"])
    SV, S = plan["SV"], plan["S"]
    counts = list(range(1, p["top"] + 1)) + ([p["long"]] if p["long"] else [])
    vs = STAIR_SLAB * SV + rng.permutation(SV)[:len(counts)]
    ids = np.repeat(vs, counts)
    rest = p["N"] - 1 - ids.size
    assert rest >= 0 and S > STAIR_SLAB + 1
    other = np.arange(STAIR_SLAB + 1, S)
    fill = other[rng.integers(0, other.size, rest)] * SV + rng.integers(0, SV, rest)
    ids = np.concatenate([ids, fill])
    return ids[rng.permutation(ids.size)], dict(zip(vs.tolist(), counts))


# =============================================================================================================
# E: the wave-aggregated LDS counters.  Wave w of point slot p holds points 1024 p + 64 w .. + 63
# =============================================================================================================

# (pattern name, distinct voxels, layout): "even": lane l -> voxel l mod k (every group has >= 2 lanes for k <= 32);
# "singles": lanes 0 and 1 alone on a voxel each (the peel loop stops after two singleton groups), the rest over k - 2
WAVE_PATTERNS = [("all-one", 1, "even"), ("two", 2, "even"), ("eight", 8, "even"), ("nine", 9, "even"), ("ten", 10, "even"),
                 ("own", 64, "even"), ("eight-singles", 8, "singles"), ("nine-singles", 9, "singles"),
                 ("ten-singles", 10, "singles")]
COUNTERS = [Case(f"counters-NP{NP}", "counters", dict(B=2, C=3, N=N, r=16, kind="waves", feat="normal"))
            for NP, N in ((1, 1024), (2, 2048))]


def wave_first(N):
    return N // 64 - len(WAVE_PATTERNS) - 1


def wave_ids(p, rng, b):
    """9 waves of the cloud's last point slot carry WAVE_PATTERNS, each inside one slab; the others are random (the last
    wave holds the balancing point)"""
    plan = vox_plan(p["B"], p["C"], p["N"], p["r"])
    SV, S, N = plan["SV"], plan["S"], p["N"]
    ids = rng.integers(0, S * SV, N - 1)
    first = wave_first(N)
    for j, (_, k, layout) in enumerate(WAVE_PATTERNS):
        slab = (j + b) % S
        vs = slab * SV + rng.permutation(SV)[:k]
        lane = np.arange(64)
        which = lane % k if layout == "even" else np.where(lane < 2, lane, 2 + lane % (k - 2))
        ids[(first + j) * 64:(first + j + 1) * 64] = vs[which]
    return ids


# =============================================================================================================
# F: the fallbacks
# =============================================================================================================

FALLBACK_SHAPES = [("odd", 2, 8, 100, 5), ("odd", 2, 8, 100, 7), ("lds", 1, 8, 2048, 34), ("r3", 1, 4, 64, 52),
                   ("s1", 256, 2, 1200, 32), ("n", 2, 5, 8193, 8)]
FALLBACK_WHY = {"s1": "lds"}     # S = 1 at r = 32 fails the LDS test: one slab of 32768 voxels
FALLBACKS = ([Case(f"fallback-{why}-b{B}c{C}n{N}r{r}", "fallback", dict(B=B, C=C, N=N, r=r, kind="clump", feat="normal", why=why))
              for why, B, C, N, r in FALLBACK_SHAPES]
             + [Case(f"fallback-misaligned-{which}", "misaligned", dict(B=3, C=9, N=700, r=16, kind="clump", feat="normal", which=which))
                for which in ("out", "cnt")])


def fallback_bound(feat, ind, cnt):
    """feat [B,C,N], ind [B,N], cnt [B,r3] -> (float64 sum [B,C,r3] of the fp32 terms t_i = fl(f_i * fl(1 / cnt)), bound
    [B,C,r3]).  bound = (k + 1) u sum|t_i| for a voxel of k points: k - 1 fp32 additions in any order, and room for the
    second-order terms -- derived, not measured (as geometry_cases.scatter_ref)."""
    B, C, N = feat.shape
    r3 = cnt.shape[1]
    ref = np.zeros((B, C, r3))
    mag = np.zeros((B, C, r3))
    for b in range(B):
        pos = np.clip(ind[b], 0, r3 - 1)
        inv = (np.float32(1.0) / cnt[b][pos].astype(np.float32)).astype(np.float32)
        t = (feat[b] * inv[None, :]).astype(np.float32).astype(np.float64)
        np.add.at(ref[b], (slice(None), pos), t)
        np.add.at(mag[b], (slice(None), pos), np.abs(t))
    return ref, (cnt[:, None, :].astype(np.float64) + 1) * U32 * mag


def within(got, ref, bound):
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= bound))


# =============================================================================================================
# G: backward
# =============================================================================================================

GRAD_CS, GRAD_NS = (1, 8, 9, 17), (1, 255, 256, 257, 1000)
GRAD = [Case(f"grad-r{r}-b{B}", "grad", dict(r=r, B=B)) for r in (4, 16) for B in (1, 3)]


def grad_ref(gy, ind, cnt):
    """vox_grad_kernel's two expressions (voxelize.hip) in NumPy float32: a clamped index, 0 where the count is 0"""
    B, C, r3 = gy.shape
    gx = np.zeros((B, C, ind.shape[1]), np.float32)
    for b in range(B):
        pos = np.clip(ind[b], 0, r3 - 1)
        cur = cnt[b][pos]
        inv = np.where(cur > 0, np.float32(1.0) / np.maximum(cur, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        gx[b] = np.where(cur[None, :] > 0, (gy[b][:, pos] * inv[None, :]).astype(np.float32), np.float32(0))
    return gx


# =============================================================================================================
# inputs of a forward case
# =============================================================================================================

ALL_FORWARD = PLANS + ADOPT + RUNS + COUNTERS + FALLBACKS


def canonical(case):
    """(normalize, eps) under which the case's cloud has the property it is named for"""
    if case.p["kind"] in ("gauss", "clump"):
        return True, (1e-3 if case.p["N"] == 1 else 0.0)
    return False, 0.0


def forward_ids(case):
    """-> (intended voxel ids [B, N], raw coordinates [B, 3, N]) of a cloud built from ids, else None"""
    p = case.p
    if p["kind"] in ("gauss", "clump"):
        return None
    rng = np.random.default_rng(seed_of(case.id) + 1)
    plan = vox_plan(p["B"], p["C"], p["N"], p["r"])
    out = []
    for b in range(p["B"]):
        if p["kind"] == "oneslab":                      # every point in slab 0, over as many voxels as it has
            ids = rng.permutation(np.arange(p["N"] - 1) % plan["SV"])
        elif p["kind"] == "slabs":
            ids = fill_slabs(p["slabs"], plan["SV"], p["N"] - 1, rng)
        elif p["kind"] == "staircase":
            ids, _ = staircase_ids(p, rng)
        elif p["kind"] == "waves":
            ids = wave_ids(p, rng, b)
        else:
            raise ValueError(p["kind"])
        out.append(balanced_cloud(ids, p["r"]))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def forward_inputs(case):
    """-> (raw coordinates float32 [B,3,N], features float32 [B,C,N])"""
    p = case.p
    rng = np.random.default_rng(seed_of(case.id))
    B, C, N = p["B"], p["C"], p["N"]
    built = forward_ids(case)
    if built is None:
        co = gaussian_cloud(rng, B, N)
        if p["kind"] == "clump":                        # most points within a few voxels, a sparse shell around them
            co[:, :, : int(N * 0.9)] *= 0.05
    else:
        co = built[1]
    feat = rng.standard_normal((B, C, N), dtype=np.float32)
    if p["feat"] == "wide":                             # magnitudes over six decades: the order of a sum shows in its bits
        feat = (feat * 10.0 ** rng.uniform(-3, 3, (B, C, N))).astype(np.float32)
    return co, feat


def order_sensitive_fraction(feat_b, ids_b):
    """one cloud: among the voxels of >= 3 points, the fraction whose fp32 sum of t_i = fl(f_i * fl(1 / cnt)) has other bits
    in descending than in ascending point order (in some channel)"""
    vs, inverse, counts = np.unique(ids_b, return_inverse=True, return_counts=True)
    inv = (np.float32(1.0) / counts.astype(np.float32)).astype(np.float32)
    hit = tot = 0
    for u in np.flatnonzero(counts >= 3):
        pts = np.flatnonzero(inverse == u)                                  # ascending point index
        t = (feat_b[:, pts] * inv[u]).astype(np.float32)
        up = np.cumsum(t, axis=1, dtype=np.float32)[:, -1]
        down = np.cumsum(t[:, ::-1], axis=1, dtype=np.float32)[:, -1]
        hit += bool(np.any(up.view(np.int32) != down.view(np.int32)))
        tot += 1
    return hit / max(tot, 1)
