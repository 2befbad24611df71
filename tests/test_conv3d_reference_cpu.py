"""CPU: the tile plan, case table, float64 references and bounds of tests/conv3d_ref.py.  The plan against what the library
reports (pure host calls), the references against an explicit 27-tap sum, and the bounds against an fp32 numpy emulation of
conv3d_k3_kernel's own arithmetic (csrc/conv3d.hip) -- so they are known to be satisfiable before any GPU run -- and against
the mistakes they are there to catch."""
import numpy as np
import pytest
import torch

import conv3d_ref as cr


def ratio(got, ref, bound):
    err = (torch.as_tensor(np.asarray(got)).double() - ref).abs()
    assert bool((bound > 0).all())
    return float((err / bound).max())


def data(cin, cout, r, B, seed):
    """seeded normal input, nn.Conv3d's default weights and bias, prologue scalars A = rand + 0.5, Bs = 0.5 randn"""
    torch.manual_seed(seed)
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1)
    x = torch.randn(B, cin, r, r, r)
    pro = (torch.rand(B, cin) + 0.5, torch.randn(B, cin) * 0.5)
    return x, conv.weight.detach(), conv.bias.detach(), pro


# ---- the plan ------------------------------------------------------------------------------------------------------------

def test_plan_mirror_equals_the_librarys_host_calls():
    """conv3d_ref.conv_plan against lion_conv3d_stat_tiles and lion_conv3d_occupancy_ints over r x Cout x B = 1..64 x sparse.
    The tile count pins VB (r^3 / (128 VB)).  The channel tile COT cannot be observed from outside the library: the five-line
    restatement is checked against conv_plan of csrc/conv3d.hip by eye."""
    from lion_amd import _lib
    lib = _lib.load()
    for r in (8, 16, 32):
        for cout in (32, 64, 96, 128, 256, 512):
            for B in range(1, 65):
                for sparse in (False, True):
                    vb, cot, tiles = cr.conv_plan(r, cout, B, sparse)
                    assert lib.lion_conv3d_stat_tiles(r, cout, B, int(sparse)) == tiles, (r, cout, B, sparse)
                    assert tiles == r ** 3 // (128 * vb) and cout % cot == 0
                    td, th, tw = cr.tile_dims(r, vb)
                    assert td * th * tw == 128 * vb and tw == r and r % td == 0 and r % th == 0
                if r in (16, 32):
                    assert lib.lion_conv3d_occupancy_ints(r, cout, B) == 2 * B * cr.conv_plan(r, cout, B, True)[2] + 4
    assert lib.lion_conv3d_stat_tiles(7, 64, 2, 0) == 0 and cr.conv_plan(8, 48, 2, False) == (0, 0, 0)
    assert lib.lion_conv3d_stat_tiles(8, 48, 2, 0) == 0


def test_case_table_reaches_every_tile_of_launch_conv():
    seen = set()
    for name, ((r, B, cout, sparse), want) in cr.PLAN_CASES.items():
        vb, cot, tiles = cr.conv_plan(r, cout, B, sparse)
        assert (vb, cot) == want, name
        assert (r, vb, cot) in cr.LAUNCH_TILES, name
        seen.add((r, vb, cot))
        if sparse:
            assert vb == 2 and r >= 16, name
    assert seen == cr.LAUNCH_TILES and len(seen) == 10
    # the rows "just under": one more sample moves them to the 64-channel tile
    assert cr.conv_plan(32, 64, 4, False)[:2] == (2, 64) and cr.conv_plan(8, 512, 32, False)[:2] == (2, 64)
    # the sparse 64-channel rows hold more items than two workgroups per CU of a 256-CU device
    for name in ("r32-vb2-cot64-sparse", "r16-vb2-cot64-sparse"):
        (r, B, cout, _), _ = cr.PLAN_CASES[name]
        assert B * cr.conv_plan(r, cout, B, True)[2] * (cout // 64) > 512
    assert len(cr.DENSE_CASES) == 10 and len(cr.SPARSE_CASES) == 4


# ---- the references ------------------------------------------------------------------------------------------------------

def taps64(z, w, bias):
    """the convolution written out: 27 shifted products summed in float64"""
    B, cin, r = z.shape[:3]
    zp = torch.zeros(B, cin, r + 2, r + 2, r + 2, dtype=torch.float64)
    zp[:, :, 1:-1, 1:-1, 1:-1] = z
    out = torch.zeros(B, w.shape[0], r, r, r, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                out += torch.einsum("oc,bcdhw->bodhw", w[:, :, kd, kh, kw].double(), zp[:, :, kd:kd + r, kh:kh + r, kw:kw + r])
    return out + bias.double()[None, :, None, None, None]


@pytest.mark.parametrize("use_pro", [False, True])
def test_conv64_is_the_written_out_sum(use_pro):
    x, w, bias, pro = data(5, 6, 8, 2, 3)
    ref, bound = cr.conv64(x, w, bias, pro if use_pro else None)
    z = x.double()
    if use_pro:
        t = z * pro[0].double()[:, :, None, None, None] + pro[1].double()[:, :, None, None, None]
        z = t * torch.sigmoid(t)
    want = taps64(z, w, bias)
    assert (ref - want).abs().max().item() <= 1e-14 * want.abs().max().item()
    k = (27 * 8 + 2) * cr.U32
    mag = taps64(z.abs(), w.abs(), bias.abs())
    if not use_pro:
        assert torch.allclose(bound, k * mag, rtol=1e-12, atol=0)
    else:
        assert bool((bound > k * mag).all()) and bool((bound < 3 * k * mag).all())
    assert cr.k_products(3) == cr.k_products(4) == 108 and cr.k_products(12) == 324 and cr.k_products(5) == 216


def test_tile_stats_follow_the_tile_geometry():
    for r, vb in ((8, 1), (8, 2), (16, 2), (16, 4), (32, 2), (32, 4)):
        td, th, _ = cr.tile_dims(r, vb)
        y = torch.randn(1, 2, r, r, r)
        s, b = cr.tile_stats64(y, r, vb)
        T = (r // td) * (r // th)
        assert tuple(s.shape) == (1, 2, T, 2) and T == r ** 3 // (128 * vb)
        for dt, ht in ((0, 0), (r // td - 1, min(1, r // th - 1)), (1, r // th - 1)):
            blk = y[:, :, dt * td:(dt + 1) * td, ht * th:(ht + 1) * th, :].double()
            t = dt * (r // th) + ht
            assert torch.allclose(s[:, :, t, 0], blk.sum((2, 3, 4)), rtol=1e-13, atol=1e-13)
            assert torch.allclose(s[:, :, t, 1], blk.square().sum((2, 3, 4)), rtol=1e-13)
            assert torch.allclose(b[:, :, t, 0], 128 * vb * cr.U32 * blk.abs().sum((2, 3, 4)), rtol=1e-13)
    names = [n for n, _ in cr.border_regions(8)]
    assert len(set(names)) == 26
    m = torch.zeros(8, 8, 8)
    for _, idx in cr.border_regions(8):
        m[idx] += 1
    assert m[1:-1, 1:-1, 1:-1].sum() == 0 and m[0, 3, 3] == 1 and m[0, 0, 3] == 3 and m[0, 0, 0] == 7


# ---- the bounds are satisfiable ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin", [4, 12])
def test_bounds_hold_for_the_kernels_own_arithmetic(cin):
    """the emulated fma chain in the kernel's order and in the reverse order, plain and behind the prologue (argument as two
    roundings and as one fma), and serial fp32 tile sums of the emulated output in both directions"""
    x, w, bias, pro = data(cin, 32, 8, 1, 10 + cin)
    pn = (pro[0].numpy(), pro[1].numpy())
    worst = {}
    for p, fused in ((None, False), (pro, False), (pro, True)):
        ref, bound = cr.conv64(x, w, bias, p)
        for rev in (False, True):
            y = cr.emulate_conv32(x.numpy(), w.numpy(), bias.numpy(), None if p is None else pn, reverse=rev, fused_arg=fused)
            assert np.all(np.isfinite(y))
            worst[(p is not None, fused, rev)] = ratio(y, ref, bound)
            for vb in (1, 2):
                sref, sbound = cr.tile_stats64(torch.as_tensor(y), 8, vb)
                st = cr.emulate_tile_stats32(y, 8, vb, reverse=rev)
                assert ratio(st, sref, sbound) <= 1.0
    print("emulation, worst error / bound:", worst)
    assert all(0.0 < v <= 1.0 for v in worst.values()), worst


def test_prologue_bound_holds_for_saturated_and_cancelling_arguments():
    """prologue scalars away from the tests' own: large slopes (|t| up to ~40: swish at its limits), and shifts that cancel
    the product or dominate it"""
    x, w, bias, _ = data(4, 32, 8, 1, 7)
    for a, b in ((10.0, 0.0), (1.0, -2.2), (1e-3, -2.2), (0.05, 3.0), (-8.0, 8.0)):
        pro = (torch.full((1, 4), a), torch.full((1, 4), b))
        ref, bound = cr.conv64(x, w, bias, pro)
        for fused in (False, True):
            y = cr.emulate_conv32(x.numpy(), w.numpy(), bias.numpy(), (pro[0].numpy(), pro[1].numpy()), fused_arg=fused)
            assert ratio(y, ref, bound) <= 1.0, (a, b, fused)


# ---- the bounds catch what they are there to catch -----------------------------------------------------------------------

def test_bounds_tell_the_mistakes_apart():
    """each mistake a tile variant of the kernel could make moves the result by far more than its bound"""
    r = 8
    x, w, bias, pro = data(12, 64, r, 2, 1)
    ref, bound = cr.conv64(x, w, bias)

    def off(wrong, sel=Ellipsis):
        return float(((wrong - ref).abs() / bound)[sel].median())

    # one tap reads the voxel next to its own
    w2 = w.clone()
    w2[:, :, 0, 1, 1] += w[:, :, 0, 1, 2]
    w2[:, :, 0, 1, 2] = 0
    assert off(cr.conv64(x, w2, bias)[0]) > 100
    # two input channels swapped
    perm = list(range(12))
    perm[4], perm[5] = 5, 4
    assert off(cr.conv64(x[:, perm], w, bias)[0]) > 100
    # zero padding replaced by edge clamping: every border voxel, nothing inside
    xc = torch.nn.functional.pad(x.double(), (1,) * 6, mode="replicate")
    clamped = torch.nn.functional.conv3d(xc, w.double(), bias.double())
    for name, idx in cr.border_regions(r):
        assert off(clamped, idx) > 100, name
    assert off(clamped, (Ellipsis, slice(1, -1), slice(1, -1), slice(1, -1))) < 1e-3
    # the two 32-channel row blocks of a 64-channel tile swapped
    assert off(torch.cat([ref[:, 32:], ref[:, :32]], 1)) > 100
    # the bias of the other channel tile
    shift = (torch.cat([bias[32:], bias[:32]]) - bias).double()[None, :, None, None, None]
    assert off(ref + shift) > 100
    # the same behind the prologue: a swapped pair of prologue scalars
    refp, boundp = cr.conv64(x, w, bias, pro)
    pa = pro[0].clone()
    pa[:, [0, 1]] = pa[:, [1, 0]]
    assert float(((cr.conv64(x, w, bias, (pa, pro[1]))[0] - refp).abs() / boundp).median()) > 100
    # statistics of the neighbouring tile
    y = ref.float()
    for vb in (1, 2):
        s, b = cr.tile_stats64(y, r, vb)
        assert float(((s.roll(1, 2) - s).abs() / b).median()) > 100
