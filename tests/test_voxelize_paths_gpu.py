"""-m gpu: the voxelisation kernels of csrc/voxelize.hip -- vox_fused_kernel (integer coordinates and the fused P1),
vox_scatter_kernel (plain and reader-aware, with its chunk adoption), the three fallback kernels and vox_grad_kernel -- on
every plan of their launchers, one test function per path.  The cases, their builders and the reasons behind the shapes are in
tests/voxelize_cases.py; tests/test_voxelize_cases_cpu.py shows on the CPU that every case reaches the plan and has the
property it is named for.

Fast path: norm_coords, ind, cnt and out bit-equal to the CPU oracle (the kernel's contract).  Fallback: ind, cnt and
norm_coords bit-equal; out is a sum in free order of the exactly known fp32 terms t_i = fl(f_i fl(1 / cnt)):
|out - sum64 t_i| <= (k + 1) 2^-24 sum|t_i| for a voxel of k points (voxelize_cases.fallback_bound).  Backward: bit-equal to
the oracle, the documented edge inputs (count 0, index outside the grid) bit-equal to a NumPy float32 restatement.

Every output lies inside a larger sentinel-filled buffer whose bands before and after it must stay intact; every fast-path
case runs twice with launches of other shapes in between: the second run finds other bytes in LDS and must give the same."""
import numpy as np
import pytest
import torch

import voxelize_cases as vc
from conftest import gaussian_cloud

pytestmark = pytest.mark.gpu

EUNSUPPORTED, EWORKSPACE = -2, -3
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
SENTINEL = {F32: -7.5, I32: -77, U8: 0xA5}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ids(cases):
    return [c.id for c in cases]


def of_path(cases, *paths, keep=lambda c: True):
    sel = [c for c in cases if c.path in paths and keep(c)]
    return pytest.mark.parametrize("case", sel, ids=ids(sel))


@pytest.fixture(scope="module")
def bk():
    from lion_amd.functional.backend import _backend
    _backend.lib  # loads the .so, raises if missing
    return _backend


@pytest.fixture(scope="module")
def lib(bk):
    return bk.lib


def ptr(t):
    from lion_amd import _lib
    return _lib.ptr(t)


def stream():
    from lion_amd import _lib
    return _lib.stream_ptr(torch.device("cuda"))


class Band:
    """a contiguous tensor `view` of `shape` that starts 256 bytes (+ `offset` elements) into a sentinel-filled buffer and
    ends 256 bytes or more before its end"""

    def __init__(self, shape, dtype, offset=0):
        self.n = int(np.prod(shape))
        self.s = SENTINEL[dtype]
        self.lo = 256 // torch.empty((), dtype=dtype).element_size() + offset
        self.buf = torch.full((self.lo + self.n + self.lo,), self.s, dtype=dtype, device="cuda")
        self.view = self.buf[self.lo:self.lo + self.n].view(shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (4 * offset) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == self.s).all()) and bool((self.buf[self.lo + self.n:] == self.s).all())

    def untouched(self):
        return bool((self.buf == self.s).all())


def same(got, want, what):
    """bit-equal (floats compared as their 32-bit patterns)"""
    want = dev(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype == F32:
        got, want = got.contiguous().view(I32), want.view(I32)
    if torch.equal(got, want):
        return
    bad = host(got != want)
    raise AssertionError(f"{what}: {np.count_nonzero(bad)} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}")


class Oracle:
    """the case's inputs and the oracle's outputs under one (normalize, eps), computed once and left unchanged"""
    _last = (None, None)

    def __init__(self, orc, case, normalize, eps):
        p = case.p
        self.co, self.feat = vc.forward_inputs(case)
        self.nc, self.vox = orc.voxelize_coords(self.co, p["r"], normalize, eps)
        self.out, self.ind, self.cnt = orc.avg_voxelize_forward(self.feat, self.vox, p["r"])
        self.normalize, self.eps = normalize, eps

    @classmethod
    def of(cls, orc, case, normalize=None, eps=None):
        if normalize is None:
            normalize, eps = vc.canonical(case)
        key = (case.id, normalize, eps)
        if cls._last[0] != key:
            cls._last = (None, None)                         # (drop the previous case's grids first)
            cls._last = (key, cls(orc, case, normalize, eps))
        return cls._last[1]


@pytest.fixture(scope="module")
def disturb(bk):
    """launches of other shapes through all four fast kernels (NP = 1 and 2, fused and scatter): they leave their bytes in
    the LDS the next launch of the case finds"""
    rng = np.random.default_rng(99)
    sets = [(dev(gaussian_cloud(rng, 3, n)), dev(rng.standard_normal((3, 7, n), dtype=np.float32) * 100 + 50), r)
            for n, r in ((1500, 16), (300, 8))]

    def go():
        for co, feat, r in sets:
            bk.voxelize_points_forward(feat, co, r)
            bk.voxel_scatter(feat, bk.voxel_index(co, r))
    return go


# ---- the entry points, every output inside a band ----------------------------------------------------------------------

class Fused:
    def __init__(self, lib, p, feat, coords, is_int, normalize=False, eps=0.0, off_out=0, off_cnt=0, ws_bytes=None):
        B, C, N, r = p["B"], p["C"], p["N"], p["r"]
        r3 = r ** 3
        self.out = Band((B, C, r3), F32, off_out) if feat is not None else None
        self.nc = None if is_int else Band((B, 3, N), F32)
        self.ind, self.cnt = Band((B, N), I32), Band((B, r3), I32, off_cnt)
        need = lib.lion_avg_voxelize_workspace_bytes(B, max(C, 1), N, r)
        self.ws = Band((need,), U8)
        ws_bytes = need if ws_bytes is None else ws_bytes
        o = ptr(self.out.view) if feat is not None else None
        c = C if feat is not None else 0
        if is_int:
            self.rc = lib.lion_avg_voxelize_forward(ptr(feat), ptr(coords), B, c, N, r, o, ptr(self.ind.view), ptr(self.cnt.view),
                                                    ptr(self.ws.view), ws_bytes, stream())
        else:
            self.rc = lib.lion_voxelize_points_forward(ptr(feat), ptr(coords), B, c, N, r, int(normalize), float(eps), o,
                                                       ptr(self.nc.view), ptr(self.ind.view), ptr(self.cnt.view),
                                                       ptr(self.ws.view), ws_bytes, stream())
        torch.cuda.synchronize()

    def bands(self):
        return [b for b in (self.out, self.nc, self.ind, self.cnt, self.ws) if b is not None]

    def check(self, o, what, out_exact=True):
        assert self.rc == 0, f"{what}: returned {self.rc}"
        if self.nc is not None:
            same(self.nc.view, o.nc, f"{what}: norm_coords")
        same(self.ind.view, o.ind, f"{what}: ind")
        same(self.cnt.view, o.cnt, f"{what}: cnt")
        if self.out is not None and out_exact:
            same(self.out.view, o.out, f"{what}: out")
        assert all(b.intact() for b in self.bands()), f"{what}: wrote outside an output"

    def untouched(self):
        return all(b.untouched() for b in self.bands())


class Index:
    def __init__(self, lib, p, co, normalize, eps, off_cnt=0, plan_bytes=None):
        B, N, r = p["B"], p["N"], p["r"]
        self.need = lib.lion_voxel_plan_bytes(B, N, r)
        self.plan = Band((max(self.need, 1024),), U8)
        self.nc, self.ind, self.cnt = Band((B, 3, N), F32), Band((B, N), I32), Band((B, r ** 3), I32, off_cnt)
        self.bytes = self.plan.n if plan_bytes is None else plan_bytes
        self.rc = lib.lion_voxel_index(ptr(co), B, N, r, int(normalize), float(eps), ptr(self.nc.view), ptr(self.ind.view),
                                       ptr(self.cnt.view), ptr(self.plan.view), self.bytes, stream())
        torch.cuda.synchronize()

    def bands(self):
        return [self.plan, self.nc, self.ind, self.cnt]

    def check(self, o, what):
        assert self.rc == 0, f"{what}: returned {self.rc}"
        same(self.nc.view, o.nc, f"{what}: norm_coords")
        same(self.ind.view, o.ind, f"{what}: ind")
        same(self.cnt.view, o.cnt, f"{what}: cnt")
        assert all(b.intact() for b in self.bands()), f"{what}: wrote outside an output or past the plan"

    def untouched(self):
        return all(b.untouched() for b in self.bands())


class Scatter:
    def __init__(self, lib, p, feat, index, occ=None, off_out=0, plan_bytes=None):
        B, C, N, r = p["B"], p["C"], p["N"], p["r"]
        self.out = Band((B, C, r ** 3), F32, off_out)
        nbytes = index.bytes if plan_bytes is None else plan_bytes
        if occ is None:
            self.rc = lib.lion_voxel_scatter(ptr(feat), ptr(index.plan.view), nbytes, B, C, N, r, ptr(self.out.view), stream())
        else:
            self.rc = lib.lion_voxel_scatter_read(ptr(feat), ptr(index.plan.view), nbytes, B, C, N, r, ptr(occ),
                                                  ptr(self.out.view), stream())
        torch.cuda.synchronize()


def needed_rows(index, p):
    """bool [B, C, r^3]: the z-rows the sparse convolution stages -- within one voxel (in d and h) of a tile with a point
    within one voxel (the row rule of test_voxel_scatter_for_the_sparse_reader) -- and the margin-1 flags themselves"""
    from lion_amd import fused_ops as fo
    B, C, r = p["B"], p["C"], p["r"]
    occ1, _ = fo.conv3d_occupancy(index.cnt.view, r, 64, B)
    td, th = (2, 4) if r == 32 else (4, 4)
    nt = (r // td) * (r // th)
    occ_t = ((occ1[:B * nt] & 0xf) != 0).view(B, 1, r // td, r // th).float()
    rows = occ_t.repeat_interleave(td, 2).repeat_interleave(th, 3)
    need = torch.nn.functional.max_pool2d(rows, 3, 1, 1)[:, 0].bool()
    return occ1, need.view(B, 1, r, r, 1).expand(B, C, r, r, r).reshape(B, C, r ** 3)


def run_fused(lib, orc, disturb, case, is_int, variants):
    p = case.p
    for normalize, eps in variants:
        o = Oracle.of(orc, case, normalize, eps)
        feat, coords = dev(o.feat), dev(o.vox if is_int else o.co)
        for run in (0, 1):
            Fused(lib, p, feat, coords, is_int, normalize, eps).check(o, f"{case.id} normalize={normalize} eps={eps} run {run}")
            disturb()


def run_two_step(lib, orc, disturb, case, read=False, fused_too=True):
    p = case.p
    o = Oracle.of(orc, case)
    feat, co = dev(o.feat), dev(o.co)
    want = dev(o.out)
    for run in (0, 1):
        index = Index(lib, p, co, o.normalize, o.eps)
        index.check(o, f"{case.id} index, run {run}")
        sc = Scatter(lib, p, feat, index)
        assert sc.rc == 0
        same(sc.out.view, o.out, f"{case.id} scatter, run {run}")
        assert sc.out.intact() and index.plan.intact()
        if read:
            occ1, need = needed_rows(index, p)
            rd = Scatter(lib, p, feat, index, occ=occ1)
            assert rd.rc == 0
            got = rd.out.view
            assert torch.equal(got[need].view(I32), want[need].view(I32)), f"{case.id} reader-aware scatter, run {run}"
            assert bool((got[~need] == SENTINEL[F32]).all()), f"{case.id}: wrote rows without a reader"
            assert bool((want[~need] == 0).all()) and rd.out.intact()
        disturb()
    if fused_too:                                             # the two-step result equals the fused entry point's
        fu = Fused(lib, p, feat, co, False, o.normalize, o.eps)
        fu.check(o, f"{case.id} fused")
        assert torch.equal(fu.out.view.view(I32), sc.out.view.view(I32))


def p1_variants(case):
    if case.p["N"] == 1:                                      # normalised with eps = 0 it is 0 / 0, in the reference too
        return [(True, 1e-3), (False, 0.0)]
    return [(True, 0.0), (True, 1e-3), (False, 0.0)]


# ---- A: vox_fused_kernel on every plan ----------------------------------------------------------------------------------

@of_path(vc.PLANS, "fused")
def test_fused_kernel_integer_coordinates(lib, orc, disturb, case):
    """vox_fused_kernel<false, NP> through lion_avg_voxelize_forward"""
    run_fused(lib, orc, disturb, case, True, [vc.canonical(case)])


@of_path(vc.PLANS, "fused")
def test_fused_kernel_with_p1(lib, orc, disturb, case):
    """vox_fused_kernel<true, NP> through lion_voxelize_points_forward: normalize on with eps 0 and 1e-3, and off"""
    run_fused(lib, orc, disturb, case, False, p1_variants(case))


def test_fused_kernel_index_only(lib, orc):
    """features == NULL: norm_coords, ind and cnt only (the kernel returns after the count slab)"""
    case = next(c for c in vc.PLANS if c.id.startswith("S8-CS2-NP4"))
    o = Oracle.of(orc, case)
    Fused(lib, case.p, None, dev(o.co), False, o.normalize, o.eps).check(o, case.id)


# ---- B: the plan-driven scatter ----------------------------------------------------------------------------------------

@of_path(vc.PLANS, "fused")
def test_index_then_scatter(lib, orc, disturb, case):
    """lion_voxel_index + lion_voxel_scatter (vox_scatter_kernel<NP, false>, the NP = 1 one-round-trip prologue included):
    bit-equal to the oracle and to the fused entry point"""
    run_two_step(lib, orc, disturb, case)


@of_path(vc.PLANS + vc.RUNS + vc.COUNTERS, "fused", "runs", "counters", keep=lambda c: c.p["r"] in (16, 32))
def test_scatter_read(lib, orc, disturb, case):
    """lion_voxel_scatter_read (vox_scatter_kernel<NP, true>): the rows with a reader bit-equal, the others left alone"""
    run_two_step(lib, orc, disturb, case, read=True, fused_too=False)


# ---- C: adoption --------------------------------------------------------------------------------------------------------

@of_path(vc.ADOPT, "adopt")
def test_adoption(lib, orc, disturb, case):
    """the NP >= 2 scatter with empty slabs adopting chunks of crowded ones (the moves: test_voxelize_cases_cpu.py)"""
    run_two_step(lib, orc, disturb, case, read=case.p["r"] in (16, 32))


# ---- D: the run lengths of phase B2 -------------------------------------------------------------------------------------

@of_path(vc.RUNS, "runs")
def test_run_lengths(lib, orc, disturb, case):
    """voxels of 1 .. 3 PW + 3 points and one long chain, features over six decades: the order of every sum shows"""
    run_fused(lib, orc, disturb, case, False, [vc.canonical(case)])
    run_fused(lib, orc, disturb, case, True, [vc.canonical(case)])
    run_two_step(lib, orc, disturb, case, fused_too=False)


# ---- E: the wave-aggregated counters -----------------------------------------------------------------------------------

@of_path(vc.COUNTERS, "counters")
def test_counters(lib, orc, disturb, case):
    """waves whose lanes hit 1, 2, 8, 9, 10 and 64 distinct voxels: counts, ids and means"""
    run_fused(lib, orc, disturb, case, False, [vc.canonical(case)])
    run_fused(lib, orc, disturb, case, True, [vc.canonical(case)])
    run_two_step(lib, orc, disturb, case, fused_too=False)


# ---- F: the fallbacks ---------------------------------------------------------------------------------------------------

def offsets(case):
    return dict(off_out=int(case.p.get("which") == "out"), off_cnt=int(case.p.get("which") == "cnt"))


def check_fallback_out(fu, o, what):
    ref, bound = vc.fallback_bound(o.feat, o.ind, o.cnt)
    got = host(fu.out.view)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bound), f"{what}: out misses the bound at {np.count_nonzero(err > bound)} voxels, largest excess {np.max(err - bound)}"
    assert np.all(got[np.broadcast_to(o.cnt[:, None, :] == 0, got.shape)] == 0)


@of_path(vc.FALLBACKS, "fallback", "misaligned")
def test_fallback_p1_kernel(lib, orc, case):
    """p1_kernel + vox_index_atomic_kernel (features == NULL): norm_coords, ind, cnt"""
    for normalize, eps in p1_variants(case):
        o = Oracle.of(orc, case, normalize, eps)
        Fused(lib, case.p, None, dev(o.co), False, normalize, eps, **offsets(case)).check(o, f"{case.id} {normalize} {eps}")


@of_path(vc.FALLBACKS, "fallback", "misaligned")
def test_fallback_index_atomic_kernel(lib, orc, case):
    """vox_index_atomic_kernel from integer coordinates: ind, cnt"""
    o = Oracle.of(orc, case)
    Fused(lib, case.p, dev(o.feat), dev(o.vox), True, **offsets(case)).check(o, case.id, out_exact=False)


@of_path(vc.FALLBACKS, "fallback", "misaligned")
def test_fallback_scatter_atomic_kernel(lib, orc, case):
    """vox_scatter_atomic_kernel behind both entry points: out within the derived bound of the float64 sum of its terms"""
    o = Oracle.of(orc, case)
    feat = dev(o.feat)
    for is_int in (True, False):
        fu = Fused(lib, case.p, feat, dev(o.vox if is_int else o.co), is_int, o.normalize, o.eps, **offsets(case))
        fu.check(o, case.id, out_exact=False)
        check_fallback_out(fu, o, f"{case.id} int={is_int}")


# ---- refusals -----------------------------------------------------------------------------------------------------------

@of_path(vc.FALLBACKS, "fallback")
def test_refusals_of_shapes_without_a_plan(lib, orc, case):
    """lion_voxel_plan_bytes == 0; index and scatter return LION_EUNSUPPORTED and write nothing"""
    p = case.p
    assert lib.lion_voxel_plan_bytes(p["B"], p["N"], p["r"]) == 0
    co, feat = (dev(a) for a in vc.forward_inputs(case))
    index = Index(lib, p, co, True, 0.0)
    assert index.rc == EUNSUPPORTED and index.untouched()
    for occ in (None,) + ((torch.zeros(4096, dtype=I32, device="cuda"),) if p["r"] in (16, 32) else ()):
        sc = Scatter(lib, p, feat, index, occ=occ)
        assert sc.rc == EUNSUPPORTED and sc.out.untouched() and index.plan.untouched()
    fu = Fused(lib, p, feat, co, False, True, 0.0, ws_bytes=lib.lion_avg_voxelize_workspace_bytes(p["B"], p["C"], p["N"], p["r"]) - 1)
    assert fu.rc == EWORKSPACE and fu.untouched()


@of_path(vc.FALLBACKS, "misaligned")
def test_refusals_on_a_fast_shape(lib, orc, case):
    """a fast shape: a cnt / out that starts 4 bytes into a 16-byte piece is LION_EUNSUPPORTED, a short plan_bytes or
    workspace LION_EWORKSPACE; nothing is written"""
    p = case.p
    o = Oracle.of(orc, case)
    co, feat = dev(o.co), dev(o.feat)
    need = lib.lion_voxel_plan_bytes(p["B"], p["N"], p["r"])
    assert need > 0
    good = Index(lib, p, co, o.normalize, o.eps)
    good.check(o, case.id)
    if p["which"] == "cnt":
        bad = Index(lib, p, co, o.normalize, o.eps, off_cnt=1)
        assert bad.rc == EUNSUPPORTED and bad.untouched()
        short = Index(lib, p, co, o.normalize, o.eps, plan_bytes=need - 1)
        assert short.rc == EWORKSPACE and short.untouched()
    else:
        occ1, _ = needed_rows(good, p)
        for occ in (None, occ1):
            bad = Scatter(lib, p, feat, good, occ=occ, off_out=1)
            assert bad.rc == EUNSUPPORTED and bad.out.untouched()
            short = Scatter(lib, p, feat, good, occ=occ, plan_bytes=need - 1)
            assert short.rc == EWORKSPACE and short.out.untouched()
        sc = Scatter(lib, p, feat, good)                    # (the plan the refusals were handed is still whole)
        assert sc.rc == 0
        same(sc.out.view, o.out, case.id)
    ws = lib.lion_avg_voxelize_workspace_bytes(p["B"], p["C"], p["N"], p["r"])
    for is_int in (True, False):
        fu = Fused(lib, p, feat, dev(o.vox) if is_int else co, is_int, o.normalize, o.eps, ws_bytes=ws - 1)
        assert fu.rc == EWORKSPACE and fu.untouched()


# ---- G: backward --------------------------------------------------------------------------------------------------------

def run_grad(lib, gy, ind, cnt, want, what):
    B, C, r3 = gy.shape
    N = ind.shape[1]
    gx = Band((B, C, N), F32)
    d_gy, d_ind, d_cnt = dev(gy), dev(ind), dev(cnt)
    rc = lib.lion_avg_voxelize_backward(ptr(d_gy), ptr(d_ind), ptr(d_cnt), B, C, N, r3, ptr(gx.view), stream())
    torch.cuda.synchronize()
    assert rc == 0
    same(gx.view, want, what)
    assert gx.intact(), f"{what}: wrote outside gx"


@of_path(vc.GRAD, "grad")
def test_backward(lib, orc, case):
    """vox_grad_kernel: C across CT = 8 with and without a remainder, N across its 256-point workgroups; ind and cnt from
    a forward of a Gaussian cloud, of a cloud inside one voxel, and the documented edge inputs"""
    r, B = case.p["r"], case.p["B"]
    r3 = r ** 3
    rng = np.random.default_rng(vc.seed_of(case.id))
    for C in vc.GRAD_CS:
        for N in vc.GRAD_NS:
            gy = rng.standard_normal((B, C, r3), dtype=np.float32)
            for kind in ("gauss", "one-voxel", "edges"):
                _, vox = orc.voxelize_coords(gaussian_cloud(rng, B, N), r, True, 1e-3)
                if kind == "one-voxel":
                    vox = np.broadcast_to(np.array([r - 1, 1, r // 2], np.int32)[None, :, None], (B, 3, N)).copy()
                _, ind, cnt = orc.avg_voxelize_forward(np.zeros((B, 1, N), np.float32), vox, r)
                if kind == "one-voxel":
                    assert cnt.max() == N and np.count_nonzero(cnt) == B
                what = f"{case.id} C={C} N={N} {kind}"
                if kind == "edges":                              # count 0 under the index, indices below 0 and from r^3 on
                    ind, cnt = ind.copy(), cnt.copy()
                    ind[:, ::7] = r3 + np.arange(ind[:, ::7].shape[1], dtype=np.int32)
                    ind[:, 3::7] = -1 - np.arange(ind[:, 3::7].shape[1], dtype=np.int32)
                    for b in range(B):
                        cnt[b, np.clip(ind[b, 1::5], 0, r3 - 1)] = 0
                    want = vc.grad_ref(gy, ind, cnt)
                    if N >= 255:
                        assert (want == 0).any() and (want != 0).any()
                else:
                    want = orc.avg_voxelize_backward(gy, ind, cnt)
                    assert np.array_equal(want.view(np.int32), vc.grad_ref(gy, ind, cnt).view(np.int32))
                run_grad(lib, gy, ind, cnt, want, what)
