"""-m gpu: conv3d_k3_kernel, the exact-fp32 MFMA 3x3x3 convolution of csrc/conv3d.hip, in every tile shape conv_plan can
choose -- the 64-channel tiles that only a large batch reaches included -- and in its four forms (prologue on / off x tile
sums on / off), against float64 under the derived elementwise bounds of tests/conv3d_ref.py; the sparse (work queue) and
constant-plus-delta launches with more items than resident workgroups; the edges of Cin; and one sparse launch of the split
kernel whose persistent grid is smaller than its item count.  Every launch goes through fused_ops.conv3d_fused or
conv_ops.conv3d_k3 with split=False (the last test: split=True).  The float64 side runs on the device."""
import pytest
import torch

import conv3d_ref as cr

pytestmark = pytest.mark.gpu

SPLIT_BOUND = 5e-6   # BOUND of test_conv_split_gpu.py


def make(cin, cout, r, B, seed):
    """seeded normal input, nn.Conv3d's default weights and bias, prologue scalars A = rand + 0.5, Bs = 0.5 randn"""
    torch.manual_seed(seed)
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1).cuda()
    x = torch.randn(B, cin, r, r, r, device="cuda")
    pro = (torch.rand(B, cin, device="cuda") + 0.5, torch.randn(B, cin, device="cuda") * 0.5)
    return conv, x, pro


def fused(x, conv, pro=None, want_stats=True, occ=None, prev_conv=None, split=False):
    from lion_amd import fused_ops
    with torch.no_grad():
        return fused_ops.conv3d_fused(x, conv, pro, want_stats, occ, prev_conv=prev_conv, split=split)


def ref_of(x, conv, pro=None):
    with torch.no_grad():
        return cr.conv64(x, conv.weight.detach(), conv.bias.detach(), pro)


def hold_output(y, ref, bound, what):
    """the whole output inside its elementwise bound, then each face, edge and corner by name; returns the worst ratio"""
    assert bool(torch.isfinite(y).all()), what
    q = (y.double() - ref).abs() / bound
    worst = float(q.max())
    print(f"{what}: worst error / bound y = {worst:.4f}")
    assert worst <= 1.0, (what, worst)
    for name, idx in cr.border_regions(y.shape[-1]):
        assert float(q[idx].max()) <= 1.0, (what, name)
    return worst


def hold_stats(st, y, ref, r, vb, what):
    """each tile's sums against the kernel's own output under the per-tile bounds; the totals over the tiles against the
    float64 reference with the tolerances of test_conv_split_gpu.py::test_split_prologue_and_groupnorm_sums"""
    B, cout = y.shape[:2]
    assert tuple(st.shape) == (B, cout, r ** 3 // (128 * vb), 2), (what, tuple(st.shape))
    assert bool(torch.isfinite(st).all()), what
    s, b = cr.tile_stats64(y, r, vb)
    q = (st.double() - s).abs() / b
    w1, w2 = float(q[..., 0].max()), float(q[..., 1].max())
    print(f"{what}: worst error / bound s1 = {w1:.4f}, s2 = {w2:.4f}")
    assert w1 <= 1.0 and w2 <= 1.0, (what, w1, w2)
    sums = st.double().sum(2)
    scale = ref.abs().max().item()
    assert torch.allclose(sums[..., 0], ref.flatten(2).sum(-1), rtol=1e-4, atol=1e-5 * scale * (r ** 3) ** 0.5), what
    assert torch.allclose(sums[..., 1], ref.flatten(2).square().sum(-1), rtol=1e-4), what


def four_forms(r, B, cin, cout, want_tile, seed):
    """plain, tile sums only, prologue only, prologue with tile sums: outputs and sums of each form held to their bounds"""
    from lion_amd import _lib, conv_ops
    vb, cot, tiles = cr.conv_plan(r, cout, B, False)
    assert (vb, cot) == want_tile
    assert _lib.load().lion_conv3d_stat_tiles(r, cout, B, 0) == tiles
    conv, x, pro = make(cin, cout, r, B, seed)
    what = f"conv3d r={r} B={B} {cin}->{cout} <vb {vb}, cot {cot}>"
    ref, bound = ref_of(x, conv)
    with torch.no_grad():
        y = conv_ops.conv3d_k3(x, conv.weight, conv.bias, split=False)
    hold_output(y, ref, bound, what + " plain")
    y, st = fused(x, conv)
    hold_output(y, ref, bound, what + " stats")
    hold_stats(st, y, ref, r, vb, what + " stats")
    del ref, bound
    if cin % 4:
        return      # the prologue takes Cin % 4 == 0 only (the wrapper pads the plain form)
    ref, bound = ref_of(x, conv, pro)
    y, st = fused(x, conv, pro, want_stats=False)
    assert st is None
    hold_output(y, ref, bound, what + " prologue")
    y, st = fused(x, conv, pro)
    hold_output(y, ref, bound, what + " prologue+stats")
    hold_stats(st, y, ref, r, vb, what + " prologue+stats")


# ---- 1. every dense tile, four forms --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cr.DENSE_CASES)
def test_dense_tiles_against_float64(case):
    """Cin = 12: three K chunks, so both weight buffers are used and the first is used again"""
    (r, B, cout, _), tile = cr.PLAN_CASES[case]
    four_forms(r, B, 12, cout, tile, seed=r + B + cout)


# ---- 2. the edges of Cin --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,cin", [("r32-vb2-cot64", 4), ("r8-vb1-cot32", 4), ("r8-vb1-cot32", 3)])
def test_single_chunk_and_padded_cin(case, cin):
    """Cin = 4: a single chunk, the load of a next chunk never issues (a 64- and a 32-channel tile); Cin = 3: through the
    wrappers' zero channel"""
    (r, B, cout, _), tile = cr.PLAN_CASES[case]
    four_forms(r, B, cin, cout, tile, seed=100 + cin + r)


@pytest.mark.parametrize("case,cin", [("r8-vb1-cot32", 64), ("r8-vb1-cot32", 68), ("r8-vb1-cot32", 256), ("r32-vb2-cot64", 68)])
def test_prologue_tables_at_their_edges(case, cin):
    """the prologue's LDS tables hold (Cin + 63) & ~63 scalars: Cin = 64 and 68 sit on either side of a step, 256 is the
    maximum; Cin = 68 on a 64-channel tile moves the arrays carved out behind the 64-wide tables"""
    (r, B, cout, _), (vb, cot) = cr.PLAN_CASES[case]
    assert cr.conv_plan(r, cout, B, False)[:2] == (vb, cot)
    conv, x, pro = make(cin, cout, r, B, seed=cin + r)
    ref, bound = ref_of(x, conv, pro)
    what = f"conv3d r={r} B={B} {cin}->{cout} <vb {vb}, cot {cot}> prologue+stats"
    y, st = fused(x, conv, pro)
    hold_output(y, ref, bound, what)
    hold_stats(st, y, ref, r, vb, what)


def test_prologue_beyond_256_channels_is_refused_on_the_host():
    from lion_amd import _lib, conv_ops
    r, B, cout, cin = 8, 2, 32, 260
    conv, x, pro = make(cin, cout, r, B, seed=260)
    with pytest.raises(RuntimeError, match="LION_EUNSUPPORTED"):
        fused(x, conv, pro)
    y = torch.full((B, cout, r, r, r), -7.5, device="cuda")
    st = torch.full((B, cout, 4, 2), -7.5, device="cuda")
    with pytest.raises(RuntimeError, match="LION_EUNSUPPORTED"):
        _lib.call("lion_conv3d_k3_fused_forward", x, conv_ops.packed_weight(conv.weight), conv.bias.detach(), B, cin, cout, r,
                  pro[0], pro[1], None, None, y, st, None)
    torch.cuda.synchronize()
    assert bool((y == -7.5).all()) and bool((st == -7.5).all())
    # without the prologue the same shape runs
    ref, bound = ref_of(x, conv)
    hold_output(fused(x, conv, None, want_stats=False)[0], ref, bound, "conv3d 260->32 plain")


# ---- 3. sparse launches ---------------------------------------------------------------------------------------------------

CLOUD_SEED = 7   # of the CPU generator: at every (r, B, N) used here the flat cloud leaves empty AND partly occupied tiles


def voxelised(kind, B, c, r, n):
    """a grid [B, c, r, r, r] from a cloud and its point counts: `flat` = normal coordinates scaled by (1, 0.2, 0.6), drawn
    on the CPU so that the cloud does not depend on the device; `one-point` = a centre point and the two corner points
    that pin the normalisation"""
    from lion_amd.functional.backend import _backend
    gen = torch.Generator().manual_seed(CLOUD_SEED)
    if kind == "one-point":
        coords = torch.zeros(B, 3, 3)
        coords[:, :, 1], coords[:, :, 2] = 1.0, -1.0
    else:
        coords = torch.randn(B, 3, n, generator=gen) * torch.tensor([1.0, 0.2, 0.6]).view(1, 3, 1)
    feat = torch.randn(B, c, coords.shape[2], generator=gen)
    out, _, _, cnt = _backend.voxelize_points_forward(feat.cuda(), coords.cuda().contiguous(), r, True, 0.0)
    return out.view(B, c, r, r, r), cnt


def queue_words(occ, B, nt):
    return occ[2 * B * nt:2 * B * nt + 2].tolist()


def totals_agree(s_a, s_b, rtol, atol_rel):
    ta, tb = s_a.sum(2), s_b.sum(2)
    return torch.allclose(ta, tb, rtol=rtol, atol=atol_rel * tb.abs().max().item())


@pytest.mark.parametrize("case,kind", [(c, "flat") for c in cr.SPARSE_CASES] + [("r32-vb2-cot64-sparse", "one-point")])
def test_sparse_and_delta_launches(case, kind):
    """conv1 (8 -> 32 on the voxelised grid, work queue, empty tiles skipped) and conv2 (32 -> Cout of the row, prologue,
    constant + delta) of a PVConv at the row's batch.  The delta form is held to cr.DELTA_RTOL of max |ref| (see
    conv3d_ref: no derived bound), everything else to its derived bound or to bit equality."""
    from lion_amd import fused_ops as fo
    (r, B, cout, _), (vb, cot) = cr.PLAN_CASES[case]
    assert cr.conv_plan(r, cout, B, True)[:2] == (vb, cot) and vb == 2
    grid, cnt = voxelised(kind, B, 8, r, 2048 if r == 32 else 512)
    torch.manual_seed(r * B + cout)
    conv1 = torch.nn.Conv3d(8, 32, 3, padding=1).cuda()
    conv2 = torch.nn.Conv3d(32, cout, 3, padding=1).cuda()
    pro = (torch.rand(B, 32, device="cuda") + 0.5, torch.randn(B, 32, device="cuda") * 0.5)
    occ1, occ2 = fo.conv3d_occupancy(cnt, r, cout, B)
    nt = cr.conv_plan(r, cout, B, True)[2]
    assert occ1.numel() == occ2.numel() == 2 * B * nt + 4 and cr.conv_plan(r, 32, B, True)[2] == nt
    for occ in (occ1, occ2):
        flags = occ[:B * nt] & 0xf
        assert bool((flags == 0).any())                                    # some tile is skipped
        if kind == "flat":
            assert bool(((flags != 0) & (flags != 0xf)).any())             # some tile runs with idle waves
    if cot == 64:       # more items than resident workgroups (two per CU): workgroups take more than one item
        assert B * nt * (cout // 64) > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    what = f"sparse r={r} B={B} {kind}"
    # conv1
    y_d, s_d = fused(grid, conv1)
    y_s, s_s = fused(grid, conv1, occ=occ1)
    assert queue_words(occ1, B, nt) == [0, 0]
    assert torch.equal(y_d, y_s), what
    ref, bound = ref_of(grid, conv1)
    hold_output(y_s, ref, bound, what + " conv1 8->32")
    assert totals_agree(s_s, s_d, 1e-4, 1e-5), what
    y_s2, s_s2 = fused(grid, conv1, occ=occ1)                              # the same buffer again
    assert torch.equal(y_s, y_s2) and torch.equal(s_s, s_s2), what
    assert queue_words(occ1, B, nt) == [0, 0]
    del y_d, y_s2, ref, bound
    # conv2
    dense, sd = fused(y_s, conv2, pro)
    sparse, ss = fused(y_s, conv2, pro, occ=occ2, prev_conv=conv1)
    assert queue_words(occ2, B, nt) == [0, 0]
    ref, bound = ref_of(y_s, conv2, pro)
    hold_output(dense, ref, bound, what + f" conv2 32->{cout} dense")
    assert bool(torch.isfinite(sparse).all())
    tol = cr.DELTA_RTOL * ref.abs().max().item()
    err = (sparse.double() - ref).abs()
    print(f"{what} conv2 32->{cout} delta: worst error / (1e-5 max|ref|) = {float(err.max()) / tol:.4f}")
    assert float(err.max()) < tol, what
    for name, idx in cr.border_regions(r):
        assert float(err[idx].max()) < tol, (what, name)
    assert totals_agree(ss, sd, 1e-3, 1e-4), what
    sparse2, ss2 = fused(y_s, conv2, pro, occ=occ2, prev_conv=conv1)
    assert torch.equal(sparse, sparse2) and torch.equal(ss, ss2), what
    assert queue_words(occ2, B, nt) == [0, 0]


# ---- 4. the split kernel's persistent grid --------------------------------------------------------------------------------

def test_split_sparse_grid_smaller_than_its_items():
    """conv3d_split_kernel, sparse conv1 at r = 32, 64 -> 64, B = 10: 1280 items for the two resident workgroups per CU"""
    from lion_amd import fused_ops as fo
    r, B, c = 32, 10, 64
    grid, cnt = voxelised("flat", B, c, r, 2048)
    torch.manual_seed(10)
    conv = torch.nn.Conv3d(c, c, 3, padding=1).cuda()
    occ1, _ = fo.conv3d_occupancy(cnt, r, c, B)
    nt = (occ1.numel() - 4) // 2 // B
    assert B * nt == 1280 and B * nt > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    flags = occ1[:B * nt] & 0xf
    assert bool((flags == 0).any()) and bool(((flags != 0) & (flags != 0xf)).any())
    y_d, s_d = fused(grid, conv, split=True)
    y_s, s_s = fused(grid, conv, occ=occ1, split=True)
    assert queue_words(occ1, B, nt) == [0, 0]
    assert torch.equal(y_d, y_s)
    y_s2, s_s2 = fused(grid, conv, occ=occ1, split=True)
    assert torch.equal(y_s, y_s2) and torch.equal(s_s, s_s2) and queue_words(occ1, B, nt) == [0, 0]
    del y_d, y_s2
    ref, _ = ref_of(grid, conv)
    err = float((y_s.double() - ref).abs().max()) / ref.abs().max().item()
    print(f"split sparse r=32 B=10 64->64: error / max|ref| = {err:.3e}")
    assert err < SPLIT_BOUND
