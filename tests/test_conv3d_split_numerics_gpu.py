"""-m gpu: the split-operand voxel convolution -- conv3d_split_pipe_kernel (r = 8) and conv3d_split_kernel<P = 2> (r = 16 / 32)
of csrc/conv3d_split.hip / conv3d_split_kernel.h -- on every plan, in its four forms, at the edges of Cin, on adversarial
dynamic ranges and at the three consumer-aware sparse levels, against float64 under the derived elementwise bounds of
tests/conv3d_split_ref.py (accumulation + representation + floor + prologue; tile sums against the kernel's own output).
A. every plan x four forms at Cin = 48;  B. Cin = 16 / 32 (the one- and two-chunk walks), 256 behind the prologue, 272 (the
<PRO = false, STATS = true> instantiation of the CB = 2 tile; refused behind a prologue);  C. dynamic range, exact scale
invariance and non-finite inputs on the r = 8 kernel and the CB = 1 tile;  D. hand-built count grids at aware levels 0 / 1 / 2,
the conv on the grid and the constant + delta conv behind it, per tile.
Launches go through conv_ops.conv3d_k3(split=True) and fused_ops.conv3d_fused(split=True); section D and the refusals call the
C entry points (as conv3d_fused marshals them), because they need an output buffer prefilled with NaN to show what a launch
leaves unwritten.  The float64 side runs on the device.

Worst error / bound ratios MEASURED on the MI355X (information only: the bounds stay the derived ones; each test prints its
own).  The bounds are worst-case dot-product bounds, linear in K = 27 Cin, so a kernel whose roundings cancel sits far inside:
  A  every plan, Cin = 48:        output 0.0010;  tile sums s1 0.0090, s2 0.0109
  B  Cin = 16 / 32 / 256 / 272:   output 0.0027 (Cin = 16, r16-CB2, prologue);  s1 0.0075, s2 0.0101
  C  dynamic range:               output 0.0030 (nine-decades on the CB = 1 tile), rising 0.0005, falling 0.0014;
                                  per-sample error / max |ref| 8.5e-7 (falling on the r = 8 kernel; BOUND 5e-6)
  D  sparse levels:               dense conv1 output 0.0014, s1 0.0088, s2 0.0154;  delta 0.060 of DELTA_RTOL max |ref|;
                                  every bit-equality, NaN-prefill and queue assertion held at the three levels.
Nothing asked for a wider constant than the assumed 2^-23 per accumulated product of v_mfma_f32_32x32x16_f16."""
import pytest
import torch

import conv3d_ref as cr
import conv3d_split_ref as sr

pytestmark = pytest.mark.gpu

BOUND = 5e-6     # test_conv_split_gpu.py: max error / max |ref|, here per sample
SPLIT, HALF = "lion_conv3d_k3_split_forward", "lion_conv3d_k3_half_forward"


def make(cin, cout, r, B, seed, bias=True):
    """seeded normal input, nn.Conv3d's default weights and bias, prologue scalars A = rand + 0.5, Bs = 0.5 randn"""
    torch.manual_seed(seed)
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1, bias=bias).cuda()
    x = torch.randn(B, cin, r, r, r, device="cuda")
    pro = (torch.rand(B, cin, device="cuda") + 0.5, torch.randn(B, cin, device="cuda") * 0.5)
    return conv, x, pro


def plain(x, w, bias):
    from lion_amd import conv_ops
    with torch.no_grad():
        return conv_ops.conv3d_k3(x, w, bias, split=True)


def fused(x, conv, pro=None, want_stats=True):
    from lion_amd import fused_ops
    with torch.no_grad():
        return fused_ops.conv3d_fused(x, conv, pro, want_stats, None, split=True)


def ref_of(x, conv, pro=None):
    with torch.no_grad():
        return sr.conv64(x, conv.weight.detach(), None if conv.bias is None else conv.bias.detach(), pro)


def hold_output(y, ref, bound, what, mask=None):
    """the output inside its elementwise bound, then each face, edge and corner by name; returns the worst ratio"""
    q = (y.double() - ref).abs() / bound
    if mask is not None:
        q = torch.where(mask, q, torch.zeros_like(q))
    else:
        assert bool(torch.isfinite(y).all()), what
    worst = float(q.max())
    print(f"{what}: worst error / bound y = {worst:.4f}")
    assert worst <= 1.0, (what, worst)
    for name, idx in cr.border_regions(y.shape[-1]):
        assert float(q[idx].max()) <= 1.0, (what, name)
    return worst


def hold_stats(st, y, ref, r, what):
    """each tile's sums against the kernel's own output under the per-tile bounds, then the totals over the tiles against the
    float64 reference (tolerances of test_conv_split_gpu.py::test_split_prologue_and_groupnorm_sums)"""
    B, cout = y.shape[:2]
    assert tuple(st.shape) == (B, cout, 2 if r == 8 else r ** 3 // 256, 2), (what, tuple(st.shape))
    assert bool(torch.isfinite(st).all()), what
    s, b = sr.tile_stats64(y, r)
    q = (st.double() - s).abs() / b
    w1, w2 = float(q[..., 0].max()), float(q[..., 1].max())
    print(f"{what}: worst error / bound s1 = {w1:.4f}, s2 = {w2:.4f}")
    assert w1 <= 1.0 and w2 <= 1.0, (what, w1, w2)
    sums = st.double().sum(2)
    scale = ref.abs().max().item()
    assert torch.allclose(sums[..., 0], ref.flatten(2).sum(-1), rtol=1e-4, atol=1e-5 * scale * (r ** 3) ** 0.5), what
    assert torch.allclose(sums[..., 1], ref.flatten(2).square().sum(-1), rtol=1e-4), what


def four_forms(shape, want, seed):
    """plain, tile sums only, prologue only, prologue with tile sums: outputs and sums of each form held to their bounds"""
    from lion_amd import _lib
    r, B, cin, cout = shape
    p = sr.split_plan(r, cin, cout)
    assert (p["kernel"], p["cb"], p["grid"][1]) == want
    assert _lib.load().lion_conv3d_split_stat_tiles(r, cout) == p["stat_tiles"]
    conv, x, pro = make(cin, cout, r, B, seed)
    what = f"split r={r} B={B} {cin}->{cout} <{p['kernel']}, cb {p['cb']}>"
    ref, bound = ref_of(x, conv)
    hold_output(plain(x, conv.weight, conv.bias), ref, bound, what + " plain")
    y, st = fused(x, conv)
    hold_output(y, ref, bound, what + " stats")
    hold_stats(st, y, ref, r, what + " stats")
    del ref, bound
    ref, bound = ref_of(x, conv, pro)
    y, st = fused(x, conv, pro, want_stats=False)
    assert st is None
    hold_output(y, ref, bound, what + " prologue")
    y, st = fused(x, conv, pro)
    hold_output(y, ref, bound, what + " prologue+stats")
    hold_stats(st, y, ref, r, what + " prologue+stats")


# ---- A. every plan, four forms --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(sr.DENSE_CASES))
def test_dense_plans_against_float64(case):
    """Cin = 48: three chunks, so both plane buffers and every weight-ring slot are used again"""
    shape, want = sr.DENSE_CASES[case]
    four_forms(shape, want, seed=sum(shape))


# ---- B. the edges of Cin --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(sr.CIN_FOUR_FORMS))
def test_one_and_two_chunk_walks(case):
    """Cin = 16: a single chunk -- `more` is never true, the counted waits take their `nothing behind` branches, the ring is
    filled once; Cin = 32: two chunks -- one refill"""
    shape, want = sr.CIN_FOUR_FORMS[case]
    four_forms(shape, want, seed=100 + sum(shape))


@pytest.mark.parametrize("case", list(sr.CIN_SINGLE_FORMS))
def test_cin_at_and_beyond_the_prologue_tables(case):
    """Cin = 256 behind the prologue (the tables' maximum); Cin = 272 without one: statistics on the CB = 2 tile run on the real
    <PRO = false, STATS = true> instantiation (up to 256 channels launch_split_t re-routes them to the PRO one)"""
    (r, B, cin, cout), use_pro, stats, inst = sr.CIN_SINGLE_FORMS[case]
    assert sr.split_plan(r, cin, cout, pro=use_pro, stats=stats)["inst"] == inst
    conv, x, pro = make(cin, cout, r, B, seed=cin + r)
    pro = pro if use_pro else None
    ref, bound = ref_of(x, conv, pro)
    what = f"split r={r} B={B} {cin}->{cout} {case}"
    if stats:
        y, st = fused(x, conv, pro)
        hold_output(y, ref, bound, what)
        hold_stats(st, y, ref, r, what)
    else:
        hold_output(plain(x, conv.weight, conv.bias), ref, bound, what)


@pytest.mark.parametrize("case", list(sr.REFUSED))
def test_prologue_beyond_256_channels_is_refused(case):
    from lion_amd import _lib, conv_ops
    r, B, cin, cout = sr.REFUSED[case]
    conv, x, pro = make(cin, cout, r, B, seed=cin)
    wp = conv_ops.split_packed_weight(conv.weight)
    y = torch.full((B, cout, r, r, r), float("nan"), device="cuda")
    st = torch.full((B, cout, sr.split_plan(r, cin, cout)["stat_tiles"], 2), float("nan"), device="cuda")
    with pytest.raises(RuntimeError, match="LION_EUNSUPPORTED"):
        _lib.call(SPLIT, x, wp, conv.bias.detach(), B, cin, cout, r, pro[0], pro[1], None, None, y, st, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(st).all())
    with pytest.raises(RuntimeError, match="LION_EUNSUPPORTED"):
        fused(x, conv, pro)


# ---- C. dynamic range on the r = 8 kernel and the CB = 1 tile -------------------------------------------------------------

@pytest.mark.parametrize("case", sr.RANGE_CASES)
@pytest.mark.parametrize("shape", list(sr.RANGE_SHAPES))
def test_dynamic_range(shape, case):
    r, B, cin, cout = sr.range_shape(shape, case)
    assert sr.split_plan(r, cin, cout)["cb"] == 1
    conv, x, _ = make(cin, cout, r, B, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        x, w, bias = sr.range_case(case, x, conv.weight.detach(), conv.bias.detach(), gen)
        if case == "rising":
            assert sr.rescales(x, r) == 3 * B * sr.split_plan(r, cin, cout)["stat_tiles"]
        if case == "falling":
            assert sr.rescales(x, r) == 0
        ref, bound = sr.conv64(x, w, bias)
        got = plain(x, w, bias)
    what = f"split {shape} {cin}->{cout} {case}"
    hold_output(got, ref, bound, what)
    # the yardstick of test_conv_split_gpu.py as well, per sample on every case: behind 64 channels the elementwise bound (linear
    # in K) is wider than a lost lo piece (test_conv3d_split_reference_cpu.py), which this measure still sees
    e = sr.per_sample_err(got, ref)
    print(f"{what}: per-sample error / max |ref| = {e:.3e}")
    assert e < BOUND, (what, e)


@pytest.mark.parametrize("shape", list(sr.RANGE_SHAPES))
def test_scale_invariance_is_exact(shape):
    """conv(x 2^k) == conv(x) 2^k and conv_{w 2^k}(x) == conv_w(x) 2^k bit for bit, no bias"""
    r, B, cin, cout = sr.RANGE_SHAPES[shape]
    conv, x, _ = make(cin, cout, r, B, seed=0, bias=False)
    base = plain(x, conv.weight, None)
    assert bool(torch.isfinite(base).all())
    with torch.no_grad():
        for k in (-80, -40, -17, 9, 16, 40, 80):
            f = 2.0 ** k
            assert torch.equal(plain(x * f, conv.weight, None), base * f), k
            assert torch.equal(plain(x, (conv.weight * f).contiguous(), None), base * f), k


@pytest.mark.parametrize("shape", list(sr.RANGE_SHAPES))
def test_nonfinite_inputs_propagate(shape):
    """an inf / nan activation poisons the outputs of its 3x3x3 neighbourhood and nothing else: everything outside is inside the
    bound of the input without the poison (non-finite values do not enter the tile's scale)"""
    r, B, cin, cout = sr.RANGE_SHAPES[shape]
    conv, x, _ = make(cin, cout, r, B, seed=1)
    hi = r - 3
    x[0, 3, 2, 2, 2] = float("inf")
    x[B - 1, 7, hi, hi, hi] = float("nan")
    xc = x.clone()
    xc[0, 3, 2, 2, 2] = 0.0
    xc[B - 1, 7, hi, hi, hi] = 0.0
    got = plain(x, conv.weight, conv.bias)
    assert not bool(torch.isfinite(got[0, :, 2, 2, 2]).any()) and not bool(torch.isfinite(got[B - 1, :, hi, hi, hi]).any())
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[0, :, 1:4, 1:4, 1:4] = False
    mask[B - 1, :, hi - 1:hi + 2, hi - 1:hi + 2, hi - 1:hi + 2] = False
    assert bool(torch.isfinite(got[mask]).all())
    ref, bound = ref_of(xc, conv)
    hold_output(got, ref, bound, f"split {shape} non-finite, outside the neighbourhoods", mask=mask)


# ---- D. sparse levels on hand-built grids ---------------------------------------------------------------------------------

def entry_launch(entry, x, conv, r, pro=None, prev_conv=None, occ=None):
    """one launch through the C entry point, marshalled as fused_ops.conv3d_fused does, into NaN-prefilled y and sums"""
    from lion_amd import _lib, conv_ops, fused_ops
    B, cin = x.shape[:2]
    cout = conv.out_channels
    wp = conv_ops.split_packed_weight(conv.weight)
    bias = conv.bias.detach()
    pa = pb = pbias = tconst = None
    if pro is not None:
        pa, pb = pro
        if prev_conv is not None:
            pbias = prev_conv.bias.detach()
            tconst = torch.empty((B, 27, cout), device="cuda")
            _lib.call("lion_conv3d_const_response", fused_ops.border_weight_sums(conv.weight), bias, pbias, pa, pb, B, cin, cout,
                      tconst)
    y = torch.full((B, cout, r, r, r), float("nan"), device="cuda")
    st = torch.full((B, cout, r ** 3 // 256, 2), float("nan"), device="cuda")
    _lib.call(entry, x.contiguous(), wp, bias, B, cin, cout, r, pa, pb, pbias, tconst, y, st, occ)
    return y, st


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def twice(entry, x, conv, r, occ, nt, pro=None, prev_conv=None):
    """a sparse launch run twice on the same occupancy buffer: equal bits, and the queue words zero after either (re-armed)"""
    B = x.shape[0]
    y, st = entry_launch(entry, x, conv, r, pro, prev_conv, occ)
    assert occ[2 * B * nt:2 * B * nt + 2].tolist() == [0, 0]
    y2, st2 = entry_launch(entry, x, conv, r, pro, prev_conv, occ)
    assert occ[2 * B * nt:2 * B * nt + 2].tolist() == [0, 0]
    assert same_bits(y, y2) and same_bits(st, st2)
    return y, st


@pytest.mark.parametrize("kind", sr.CLOUDS)
@pytest.mark.parametrize("r,c", sr.SPARSE_SHAPES)
def test_sparse_levels_per_tile(r, c, kind):
    """conv1 (c -> c on a grid that is non-zero exactly at the counted voxels, no prologue) and conv2 (c -> c, prologue,
    constant + delta, reading conv1's output of the same level with its unwritten tiles still NaN) at consumer_aware 0, 1, 2"""
    from lion_amd import fused_ops as fo
    B = 2
    cnt_cpu = sr.cloud_counts(kind, r, B)
    cnt = cnt_cpu.cuda()
    torch.manual_seed(r + c)
    conv1 = torch.nn.Conv3d(c, c, 3, padding=1).cuda()
    conv2 = torch.nn.Conv3d(c, c, 3, padding=1).cuda()
    x = torch.randn(B, c, r, r, r, device="cuda") * (cnt.view(B, 1, r, r, r) > 0)
    pro = (torch.rand(B, c, device="cuda") + 0.5, torch.randn(B, c, device="cuda") * 0.5)
    nt = r ** 3 // 256
    what = f"sparse r={r} {c}->{c} {kind}"
    vox = lambda m: sr.tiles_to_voxels(m, r).cuda().expand(B, c, r, r, r)       # [B, T] tile mask -> voxels
    til = lambda m: m.cuda()[:, None, :, None].expand(B, c, nt, 2)              # ... -> the layout of the sums
    with torch.no_grad():
        # the dense launches and the float64 side, once for the three levels
        dense1 = {e: entry_launch(e, x, conv1, r) for e in (SPLIT, HALF)}
        ref1, bound1 = ref_of(x, conv1)
        hold_output(dense1[SPLIT][0], ref1, bound1, what + " conv1 dense")
        hold_stats(dense1[SPLIT][1], dense1[SPLIT][0], ref1, r, what + " conv1 dense")
        del ref1, bound1
        y1_d = dense1[SPLIT][0]
        y2_d, _ = entry_launch(SPLIT, y1_d, conv2, r, pro)
        ref2 = cr._conv64(cr.operand64(y1_d, pro)[0], conv2.weight.double(), conv2.bias.double())
        tol = sr.DELTA_RTOL * sr.per_sample_max(ref2)                            # [B, 1, 1, 1, 1]
        s2_ref, s2_bound = sr.tile_stats64(y2_d, r)
        abs2 = cr.tile_view(y2_d.double().abs(), r, sr.VB).sum(-1)               # [B, c, T]: sum |y| per tile
        tol_t = tol.view(B, 1, 1)
        # unstored tiles of the delta conv: the tile-sum bound, plus DELTA_RTOL max |ref| on each of the 256 terms of the sum:
        #   s1: 256 tol;   s2: sum ((y + e)^2 - y^2) <= 2 tol sum |y| + 256 tol^2
        allow2 = s2_bound + torch.stack([256 * tol_t.expand_as(abs2), 2 * tol_t * abs2 + 256 * tol_t ** 2], -1)
        for level in sr.LEVELS:
            fl = sr.tile_flags(cnt_cpu, r, level)
            occ1, occ2 = fo.conv3d_occupancy(cnt, r, c, B, consumer_aware=level)
            assert occ1.numel() == occ2.numel() == 2 * B * nt + 4 and int(occ1[2 * B * nt + 2]) == level
            assert torch.equal(occ1[:B * nt].view(B, nt).cpu().long(), fl["word1"]), (what, level)
            assert torch.equal(occ2[:B * nt].view(B, nt).cpu().long(), fl["word2"]), (what, level)
            # conv1: sparse against the dense launch of the same kernel, on the split and on the single-product kernel
            occupied, stored = fl["mask1"] != 0, fl["stored1"]
            for entry in (SPLIT, HALF):
                y_d, s_d = dense1[entry]
                y_s, s_s = twice(entry, x, conv1, r, occ1, nt)
                w = (what, level, entry)
                assert same_bits(torch.where(vox(stored), y_s, 0.0), torch.where(vox(stored), y_d, 0.0)), w
                assert bool(torch.isnan(y_s[vox(~stored)]).all()), w
                empty_written = vox(stored & ~occupied)
                assert bool((y_s == conv1.bias.view(1, c, 1, 1, 1))[empty_written].all()), w
                assert same_bits(torch.where(til(occupied), s_s, 0.0), torch.where(til(occupied), s_d, 0.0)), w
                sref, sbound = sr.tile_stats64(y_d, r)
                q = torch.where(til(~occupied), (s_s.double() - sref).abs() / sbound, 0.0)
                assert bool(torch.isfinite(s_s).all()) and float(q.max()) <= 1.0, (w, float(q.max()))
                if entry == SPLIT:
                    y1_s = y_s
            # conv2: constant + delta on conv1's output of this level
            stored2 = fl["stored2"]
            y2, s2 = twice(SPLIT, y1_s, conv2, r, occ2, nt, pro, conv1)
            w = (what, level, "delta")
            m = vox(stored2)
            assert bool(torch.isfinite(y2[m]).all()), w                          # nothing the producer skipped was loaded
            assert bool(torch.isnan(y2[~m]).all()), w
            err = torch.where(m, (y2.double() - ref2).abs() / tol, 0.0)
            print(f"{what} level {level} delta: worst error / (1e-5 max|ref| per sample) = {float(err.max()):.4f}")
            assert float(err.max()) < 1.0, (w, float(err.max()))
            assert bool(torch.isfinite(s2).all()), w
            own, own_b = sr.tile_stats64(torch.where(m, y2, 0.0), r)
            q = torch.where(til(stored2), (s2.double() - own).abs() / own_b, 0.0)
            assert float(q.max()) <= 1.0, (w, float(q.max()))
            q = torch.where(til(~stored2), (s2.double() - s2_ref).abs() / allow2, 0.0)
            assert float(q.max()) <= 1.0, (w, float(q.max()))
