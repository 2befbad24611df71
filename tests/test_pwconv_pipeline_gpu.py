"""-m gpu: the schedule of pwconv_kernel (csrc/pwconv.hip) -- a workgroup walks several column tiles with the operand one
group of k-steps ahead -- through lion_internal_pwconv_walk, which runs that kernel at any L with a cap on the workgroups
per (sample, channel tile) and the weights forced through LDS or read from L2.  A few hundred to 2600 columns, B = 2:
  1. the walk (cap 1 and 2) == one workgroup per tile, bit for bit: y, every tile of the sums, the OUT = 2 maxima;
  2. exact on small integers under the walk, which pins the tile index of every sum;
  3. within the float64 bounds of tests/pwconv_ref.py under the walk;
  4. a NaN in the last column / the last channel changes only what depends on it.
T = columns of a tile (512, 512, 256, 128 for CB = 1, 2, 4, 8), G = 32 / VB k-steps of a group (8, 8, 16, 32)."""
import math

import pytest
import torch

import pwconv_ref as pw

pytestmark = pytest.mark.gpu

NAN = float("nan")
B = 2
N_PTS, U = 96, 32            # the gathered operand: 96 points, 32 neighbours per centre
COUTS = (32, 48, 64, 128, 256)   # 48: padded channel rows


def geometry(cout, cin):
    cb, vb = pw.pw_plan(cout, cin)
    return cb, 4 * vb * 32, 32 // vb     # CB, T, G


def cins(cout):
    g = geometry(cout, 3)[2]
    out = (3, 2 * g - 1, 2 * g, 2 * g + 1, 4 * g + 3)   # one group, the group edge, three groups; odd and even
    assert all(geometry(cout, c)[2] == g for c in out)
    return out


CASES = [(cout, cin) for cout in COUTS for cin in cins(cout)]


def pack(w):
    from lion_amd import fused_ops
    return fused_ops._pw_pack(w)


def walk(x, w, bias, pro=None, out=None, gather=None, y=True, stats=True, cap=0, wlds=-1):
    """lion_internal_pwconv_walk -> (y | ymax | None, sums | None); outputs start as NaN, so an element nobody wrote
    compares unequal to everything.  x f32[B, Cin, L], or gather = (coords, centers, feat | None, idx) with L = M * U."""
    from lion_amd import _lib
    cout, cin = w.shape
    if gather is None:
        L = x.shape[2]
        ga = (None, None, None, None, 0, 0)
    else:
        coords, centers, feat, idx = gather
        L = idx.shape[1] * idx.shape[2]
        ga = (coords, centers, feat, idx, coords.shape[2], idx.shape[2])
    tiles = math.ceil(L / geometry(cout, cin)[1])
    pa, pb = (None, None) if pro is None else pro
    oa, ob = (None, None) if out is None else out
    yt = None
    if out is not None:
        yt = torch.full((B, cout, L // 32), NAN, device="cuda")
    elif y:
        yt = torch.full((B, cout, L), NAN, device="cuda")
    st = torch.full((B, cout, tiles, 2), NAN, device="cuda") if stats else None
    _lib.call("lion_internal_pwconv_walk", x, pack(w), bias, B, cin, cout, L, pa, pb, oa, ob, *ga, yt, st, cap, wlds)
    return yt, st


def data(cout, cin, L, seed, kind="unit"):
    return pw.make_data(kind, cin, cout, L, B, seed, device="cuda")


def gather_data(cin, L, seed, integers=False):
    """(coords, centers, feat | None, idx) and the [B, Cin, L] tensor they stand for; idx holds 0, N - 1 and values
    outside [0, N), which the kernel clamps as the grouping kernel does"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    M, C = L // U, cin - 3

    def rnd(*s):
        if integers:
            return torch.randint(-4, 5, s, generator=g, device="cuda").float()
        return torch.randn(*s, generator=g, device="cuda")

    coords, centers = rnd(B, 3, N_PTS), rnd(B, 3, M)
    feat = rnd(B, C, N_PTS) if C else None
    idx = torch.randint(-3, N_PTS + 3, (B, M, U), generator=g, device="cuda", dtype=torch.int32)
    idx[:, 0, 0], idx[:, 0, 1], idx[:, -1, -1], idx[:, -1, 0] = 0, N_PTS - 1, -7, N_PTS + 5
    ic = idx.long().clamp(0, N_PTS - 1).view(B, 1, L)
    x = torch.gather(coords, 2, ic.expand(B, 3, L)) - centers.repeat_interleave(U, 2)
    if C:
        x = torch.cat([x, torch.gather(feat, 2, ic.expand(B, C, L))], 1)
    return (coords, centers, feat, idx), x.contiguous()


def out_scalars(cout, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, cout, generator=g, device="cuda") * 0.5 + 1.0, torch.randn(B, cout, generator=g, device="cuda") * 0.3)


# ---- 1. walk == no walk ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout,cin", CASES)
def test_walk_equals_one_workgroup_per_tile(cout, cin):
    """cap 1 (one workgroup walks every tile) and cap 2 against the cap at the tile count: torch.equal on y, every tile of
    the sums and the OUT = 2 maxima; ragged L = 3 T + 37, L = T - 1, and 3 T + 32 for the max form and the gathered operand;
    prologue and statistics on and off; weights through LDS and from L2"""
    _, T, _ = geometry(cout, cin)
    for L in (3 * T + 37, T - 1):
        tiles = math.ceil(L / T)
        x, w, bias, pro = data(cout, cin, L, 7 * cin + cout + L)
        for p in (None, pro):
            for st in (True, False):
                for wlds in (1, 0):
                    y0, s0 = walk(x, w, bias, p, stats=st, cap=tiles, wlds=wlds)
                    assert not bool(torch.isnan(y0).any()) and (s0 is None or not bool(torch.isnan(s0).any()))
                    for cap in (1, 2):
                        y1, s1 = walk(x, w, bias, p, stats=st, cap=cap, wlds=wlds)
                        assert torch.equal(y1, y0), (L, p is not None, st, wlds, cap)
                        assert s0 is None or torch.equal(s1, s0), (L, p is not None, st, wlds, cap)
                # the weights' route changes nothing either
                assert torch.equal(walk(x, w, bias, p, stats=st, cap=1, wlds=1)[0], walk(x, w, bias, p, stats=st, cap=2, wlds=0)[0])
    L = 3 * T + 32
    tiles = math.ceil(L / T)
    x, w, bias, pro = data(cout, cin, L, 11 * cin + cout)
    out = out_scalars(cout, cin + cout)
    for p in (None, pro):
        for wlds in (1, 0):
            y0, s0 = walk(x, w, bias, p, cap=tiles, wlds=wlds)
            _, q0 = walk(x, w, bias, p, y=False, cap=tiles, wlds=wlds)
            m0, _ = walk(x, w, bias, p, out=out, stats=False, cap=tiles, wlds=wlds)
            assert torch.equal(q0, s0) and not bool(torch.isnan(m0).any())
            for cap in (1, 2):
                _, q1 = walk(x, w, bias, p, y=False, cap=cap, wlds=wlds)
                m1, _ = walk(x, w, bias, p, out=out, stats=False, cap=cap, wlds=wlds)
                assert torch.equal(q1, s0) and torch.equal(m1, m0), (p is not None, wlds, cap)
    ga, xg = gather_data(cin, L, 13 * cin + cout)
    for st in (True, False):
        for wlds in (1, 0):
            y0, s0 = walk(xg, w, bias, stats=st, cap=tiles, wlds=wlds)          # the tensor the gather stands for
            for cap in (tiles, 1, 2):
                y1, s1 = walk(None, w, bias, gather=ga, stats=st, cap=cap, wlds=wlds)
                assert torch.equal(y1, y0) and (s0 is None or torch.equal(s1, s0)), (st, wlds, cap)


# ---- 2. exact on small integers -------------------------------------------------------------------------------------------

def int_data(cout, cin, L, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def ri(*s):
        return torch.randint(-4, 5, s, generator=g, device="cuda").float()

    return ri(B, cin, L), ri(cout, cin), ri(cout)


def check_exact(x, w, bias, y, st, T):
    ref, _ = pw.pwconv64(x, w, bias)
    assert y is None or torch.equal(y.double(), ref)
    s, _ = pw.tile_stats64(ref, torch.zeros_like(ref), T)
    sa, _ = pw.tile_stats64(ref.abs(), torch.zeros_like(ref), T)
    assert sa.max().item() < pw.EXACT_MAX     # the data keeps its promise: every partial sum is an fp32 integer
    assert torch.equal(st.double(), s)


@pytest.mark.parametrize("cout,cin", CASES)
def test_integers_are_exact_under_the_walk(cout, cin):
    """operands in [-4, 4]: y and EVERY tile sum equal integer arithmetic with one workgroup walking all tiles and with
    two, plain and gathered, stored and sums-only -- a sum in the slot of the workgroup instead of the tile would show"""
    _, T, _ = geometry(cout, cin)
    L = 3 * T + 37
    x, w, bias = int_data(cout, cin, L, 3 * cin + cout)
    assert pw.exact_ok(x, w, bias)
    for cap in (1, 2):
        for wlds in (1, 0):
            check_exact(x, w, bias, *walk(x, w, bias, cap=cap, wlds=wlds), T)
    L = 3 * T + 32
    ga, xg = gather_data(cin, L, 5 * cin + cout, integers=True)
    assert pw.exact_ok(xg, w, bias)
    for cap in (1, 2):
        check_exact(xg, w, bias, *walk(None, w, bias, gather=ga, cap=cap, wlds=cap - 1), T)
        check_exact(xg, w, bias, *walk(xg, w, bias, y=False, cap=cap, wlds=2 - cap), T)


# ---- 3. float64 under the derived bounds ------------------------------------------------------------------------------------

def ratio(got, ref, bound):
    assert bool(torch.isfinite(got).all())
    return float(((got.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("cout,cin", CASES)
def test_against_float64_under_the_walk(cout, cin):
    """y per element, s1 / s2 per tile and the activated maximum within pwconv64 / tile_stats64 / max64 of
    tests/pwconv_ref.py, with and without the prologue, one workgroup walking all tiles (and two, from L2)"""
    _, T, _ = geometry(cout, cin)
    L = 3 * T + 32
    x, w, bias, pro = data(cout, cin, L, 17 * cin + cout)
    out = out_scalars(cout, cin)
    for p in (None, pro):
        ref, bound = pw.pwconv64(x, w, bias, p)
        s64, sb = pw.tile_stats64(ref, bound, T)
        m64, mb = pw.max64(ref, bound, *out)
        for cap, wlds in ((1, 1), (2, 0)):
            y, st = walk(x, w, bias, p, cap=cap, wlds=wlds)
            m, _ = walk(x, w, bias, p, out=out, stats=False, cap=cap, wlds=wlds)
            r = {"y": ratio(y, ref, bound), "s1": ratio(st[..., 0], s64[..., 0], sb[..., 0]),
                 "s2": ratio(st[..., 1], s64[..., 1], sb[..., 1]), "max": ratio(m, m64, mb)}
            print(f"{cin}->{cout} pro={p is not None} cap={cap}: worst error / bound " + ", ".join(f"{k} = {v:.3f}" for k, v in r.items()))
            assert all(v <= 1.0 for v in r.values()), r
    ga, xg = gather_data(cin, L, 19 * cin + cout)
    ref, bound = pw.pwconv64(xg, w, bias)
    s64, sb = pw.tile_stats64(ref, bound, T)
    y, st = walk(None, w, bias, gather=ga, cap=1, wlds=0)
    r = {"y": ratio(y, ref, bound), "s1": ratio(st[..., 0], s64[..., 0], sb[..., 0]), "s2": ratio(st[..., 1], s64[..., 1], sb[..., 1])}
    print(f"{cin}->{cout} gathered: worst error / bound " + ", ".join(f"{k} = {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


# ---- 4. NaN containment -------------------------------------------------------------------------------------------------------

def same_or_nan(got, clean, nan_mask):
    return bool(torch.isnan(got)[nan_mask].all()) and torch.equal(got[~nan_mask], clean[~nan_mask])


@pytest.mark.parametrize("cout,cin", CASES)
def test_nan_is_contained_under_the_walk(cout, cin):
    """a NaN in column L - 1 (the column every masked lane of the last tile reads, clamped) of sample 0 and one in channel
    Cin - 1 (the row the odd-Cin half-wave reads, clamped) of sample 1, in tile 1: NaN in exactly those two columns of y and
    those two tiles of the sums, in the one maximum that holds the column; every other value bit for bit the clean run's"""
    _, T, _ = geometry(cout, cin)
    for L in (3 * T + 37, 3 * T + 32):
        x, w, bias, pro = data(cout, cin, L, 23 * cin + cout + L)
        dirty = x.clone()
        c1 = T + 5
        dirty[0, 0, L - 1] = NAN
        dirty[1, cin - 1, c1] = NAN
        ymask = torch.zeros(B, cout, L, dtype=torch.bool, device="cuda")
        ymask[0, :, L - 1] = True
        ymask[1, :, c1] = True
        smask = torch.zeros(B, cout, math.ceil(L / T), 2, dtype=torch.bool, device="cuda")
        smask[0, :, (L - 1) // T] = True
        smask[1, :, c1 // T] = True
        for p in (None, pro):
            for cap, wlds in ((1, 1), (2, 0)):
                y0, s0 = walk(x, w, bias, p, cap=cap, wlds=wlds)
                y1, s1 = walk(dirty, w, bias, p, cap=cap, wlds=wlds)
                assert same_or_nan(y1, y0, ymask) and same_or_nan(s1, s0, smask), (L, p is not None, cap)
                if L % 32 == 0:
                    out = out_scalars(cout, cin)
                    m0, _ = walk(x, w, bias, p, out=out, stats=False, cap=cap, wlds=wlds)
                    m1, _ = walk(dirty, w, bias, p, out=out, stats=False, cap=cap, wlds=wlds)
                    mmask = ymask.view(B, cout, L // 32, 32).any(-1)
                    # a maximum over a NaN: the kernel's comparison chain may keep or drop it, as lion_affine_swish_max's does
                    assert torch.equal(m1[~mmask], m0[~mmask]), (L, p is not None, cap)
