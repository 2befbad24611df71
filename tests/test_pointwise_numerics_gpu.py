"""-m gpu: the inference AdaGN / pointwise kernels (csrc/pointwise.hip, gn_fold_kernel / gn_fold_se_kernel of
csrc/conv3d.hip), each on its own against the float64 references and derived bounds of tests/pointwise_ref.py, at the
lengths, channel counts and row counts where their code takes another path.  Every case is a few MB at the most."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointwise_ref as pr

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def within(got, ref, bound, what):
    """every element of |got - ref| <= bound; prints the worst ratio first"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    worst = float((err / bound).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert np.all(np.isfinite(np.asarray(got))), what
    assert worst <= 1.0, f"{what}: {worst:.3f} x the bound at flat index {int((err / bound).argmax())}"


def make_gn(G, C, seed):
    gn = torch.nn.GroupNorm(G, C).cuda()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        gn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        gn.bias.copy_(torch.rand(C, generator=g) - 0.5)
    return gn


def make_se(C, H, seed):
    """what fused_ops reads of an SE3d, with a free hidden width: fc = Linear(C, H), ReLU, Linear(H, C), Sigmoid"""
    torch.manual_seed(seed)
    fc = torch.nn.Sequential(torch.nn.Linear(C, H, bias=False), torch.nn.ReLU(), torch.nn.Linear(H, C, bias=False),
                             torch.nn.Sigmoid()).cuda()
    return SimpleNamespace(fc=fc)


def tile_data(B, C, T, n, seed, mean=0.2, std=0.7):
    """x f32 [B, C, T, n] and its tile sums [B, C, T, 2]: float64 sums rounded to fp32"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, C, T, n)) * std + mean).astype(np.float32)
    d = x.astype(np.float64)
    stats = np.stack([d.sum(-1), (d * d).sum(-1)], -1).astype(np.float32)
    return x, stats


def projection(B, C, seed):
    """the [B, 2C] style projection whose two strided halves are fac and gbias"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 2 * C, generator=g) * 0.3 + torch.cat([torch.ones(C), torch.zeros(C)])).cuda()


# ---- a. lion_row_stats ------------------------------------------------------------------------------------------------

def check_row_stats(rows, L, seed):
    from lion_amd import fused_ops
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, 1, L)) * 1.5 + 3.0).astype(np.float32)
    got = host(fused_ops.row_stats(dev(x)))
    assert got.shape == (rows, 2)
    d = x.astype(np.float64).reshape(rows, L)
    g = pr.row_sum_gamma(L)
    within(got[:, 0], d.sum(-1), g * np.abs(d).sum(-1), f"row_stats s1 rows={rows} L={L}")
    within(got[:, 1], (d * d).sum(-1), g * (d * d).sum(-1), f"row_stats s2 rows={rows} L={L}")


@pytest.mark.parametrize("L", [1, 3, 4, 5, 255, 256, 1023, 1024, 1028, 4097, 32768])
def test_row_stats_against_float64_sums(L):
    """float4 (L % 4 == 0) and scalar path, rows shorter than one pass and than one wave, a ragged last pass; data with a
    non-zero mean so that a dropped or doubled element shows in both sums"""
    for rows in (1, 3, 130):
        check_row_stats(rows, L, 1000 * rows + L)


def test_row_stats_of_70000_rows():
    check_row_stats(70000, 4, 7)


# ---- b. lion_groupnorm_fold -------------------------------------------------------------------------------------------

def check_fold(B, C, G, T, fac, gb, seed):
    from lion_amd import fused_ops
    n = 64
    x, stats = tile_data(B, C, T, n, seed)
    gn = make_gn(G, C, seed)
    A, Bs, cm = fused_ops.groupnorm_fold(dev(stats), gn, fac, gb, T * n)
    A64, B64, cm64 = pr.adagn_fold64(x, G, gn.weight, gn.bias, fac, gb, gn.eps)
    d = torch.from_numpy(x).double().reshape(B, C, -1)
    ref = d * A64[:, :, None] + B64[:, :, None]
    got = d * A.double().cpu()[:, :, None] + Bs.double().cpu()[:, :, None]
    tag = f"fold B={B} C={C} G={G} T={T}"
    within(got.numpy(), ref.numpy(), pr.FOLD_RTOL * ref.abs().max().item(), tag + " x*A+Bs")
    within(host(cm), cm64.numpy(), pr.FOLD_RTOL * cm64.abs().max().item(), tag + " chmean")


@pytest.mark.parametrize("C,G,T", [(8, 8, 1), (8, 8, 300), (16, 8, 5), (24, 8, 7), (40, 8, 77), (512, 8, 3), (64, 1, 130)])
def test_groupnorm_fold_against_group_norm_of_the_data(C, G, T):
    """channels per group 1 and 2 (one channel spans several waves: the LDS combine), 3 and 5 (idle channel slots), 64 (the
    declared limit); fewer tiles than lanes per channel and more; fac / gbias as the strided halves of a projection"""
    for B in (1, 3):
        fac, gb = projection(B, C, C + T + B).chunk(2, 1)
        assert fac.stride(0) == 2 * C
        check_fold(B, C, G, T, fac, gb, 100 * C + T + B)


def test_groupnorm_fold_with_one_row_expanded_over_the_batch():
    B, C, G, T = 3, 24, 8, 7
    fac, gb = projection(1, C, 5).chunk(2, 1)
    check_fold(B, C, G, T, fac.expand(B, C), gb.expand(B, C), 11)


def test_groupnorm_fold_rejects_more_than_64_channels_per_group():
    from lion_amd import fused_ops
    B, C, G, T = 1, 130, 2, 3
    _, stats = tile_data(B, C, T, 64, 0)
    fac, gb = projection(B, C, 0).chunk(2, 1)
    with pytest.raises(RuntimeError, match="lion_groupnorm_fold"):
        fused_ops.groupnorm_fold(dev(stats), make_gn(G, C, 0), fac, gb, T * 64)
    torch.cuda.synchronize()


# ---- c. lion_groupnorm_fold_se, lion_se_gate --------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("C,G,H", [(4, 1, 1), (5, 5, 2), (12, 4, 3), (100, 4, 12), (256, 8, 128)])
def test_groupnorm_fold_se_against_group_norm_and_gate_of_the_data(C, G, H, T):
    from lion_amd import fused_ops
    B, n = 3, 64
    x, stats = tile_data(B, C, T, n, 10 * C + T)
    gn = make_gn(G, C, C + T)
    se = make_se(C, H, C + H)
    fac, gb = projection(B, C, C + H + T).chunk(2, 1)
    merged = fused_ops.groupnorm_fold_se(dev(stats), gn, fac, gb, T * n, se)
    assert merged is not None
    A64, B64, cm64 = pr.adagn_fold64(x, G, gn.weight, gn.bias, fac, gb, gn.eps)
    A2, B2 = pr.se_gate64(A64, B64, cm64, se.fc[0].weight, se.fc[2].weight)
    tag = f"fold_se C={C} G={G} H={H} T={T}"
    within(host(merged[0]), A2.numpy(), pr.FOLD_RTOL * A2.abs().max().item(), tag + " A")
    within(host(merged[1]), B2.numpy(), pr.FOLD_RTOL * B2.abs().max().item(), tag + " Bs")


def gate_case(C, H, seed):
    rng = np.random.default_rng(seed)
    B = 3
    A = (rng.standard_normal((B, C)) * 0.8).astype(np.float32)
    Bs = (rng.standard_normal((B, C)) * 0.5).astype(np.float32)
    cm = (rng.standard_normal((B, C)) * 0.7 + 0.2).astype(np.float32)
    se = make_se(C, H, seed)
    return A, Bs, cm, se, pr.se_gate64(A, Bs, cm, se.fc[0].weight, se.fc[2].weight)


@pytest.mark.parametrize("C,H", [(4, 1), (65, 8), (1000, 125), (1024, 128)])
def test_se_gate_against_float64(C, H):
    from lion_amd import fused_ops
    A, Bs, cm, se, (A2, B2) = gate_case(C, H, C + H)
    dA, dB = dev(A), dev(Bs)
    gA, gB = fused_ops.se_gate_(dA, dB, dev(cm), se)
    assert gA.data_ptr() == dA.data_ptr() and gB.data_ptr() == dB.data_ptr()      # the kernel works in place
    within(host(gA), A2.numpy(), pr.FOLD_RTOL * A2.abs().max().item(), f"se_gate C={C} H={H} A")
    within(host(gB), B2.numpy(), pr.FOLD_RTOL * B2.abs().max().item(), f"se_gate C={C} H={H} Bs")


@pytest.mark.parametrize("C,H", [(1025, 8), (64, 129)])
def test_se_gate_beyond_the_kernels_range_falls_back_with_the_same_result(C, H):
    """C > 1024 or H > 128 does not fit the kernel's LDS arrays: se_gate_ evaluates the gate with torch, out of place"""
    from lion_amd import fused_ops
    A, Bs, cm, se, (A2, B2) = gate_case(C, H, C + H)
    dA, dB = dev(A), dev(Bs)
    with torch.no_grad():
        gA, gB = fused_ops.se_gate_(dA, dB, dev(cm), se)
    assert np.array_equal(host(dA), A) and np.array_equal(host(dB), Bs)
    within(host(gA), A2.numpy(), pr.FOLD_RTOL * A2.abs().max().item(), f"se_gate fallback C={C} H={H} A")
    within(host(gB), B2.numpy(), pr.FOLD_RTOL * B2.abs().max().item(), f"se_gate fallback C={C} H={H} Bs")


# ---- d. conditioning of the one-pass variance -------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [0.0, 8.0, 64.0])
def test_inference_fold_conditioning_against_the_one_pass_formula_in_fp32(ratio):
    """var = E[x^2] - mean^2 from fp32 sums loses about (mean/std)^2 u of A.  The yardstick is the same formula on the CPU
    (pointwise_ref.onepass_fold_a32: fp32 tile sums, float64 combine); the kernels -- row_stats then groupnorm_fold over
    whole rows of L = 4096, and over the 512-element tile sums a convolution emits, summed by row_stats -- must stay
    within 4x its error in A (relative to max |A|), the 4 for the different summation order.

    Measured (B = 2, C = 16, G = 8, unit std), error of A relative to max |A|, CPU formula / kernels:
        mean/std    rows of 4096: CPU    kernel        tiles of 512: CPU    kernel
        0                   8.66e-08   8.66e-08              7.81e-08   7.81e-08
        8                   3.97e-06   2.85e-06              1.50e-06   1.47e-06
        64                  1.47e-04   2.09e-04              7.51e-05   7.47e-05
    """
    from lion_amd import fused_ops
    B, C, G, L = 2, 16, 8, 4096
    rng = np.random.default_rng(int(ratio) + 3)
    x = (rng.standard_normal((B, C, L)) + ratio).astype(np.float32)
    gn = make_gn(G, C, int(ratio))
    fac, gb = projection(B, C, int(ratio) + 1).chunk(2, 1)
    A64 = pr.adagn_fold64(x, G, gn.weight, gn.bias, fac, gb, gn.eps)[0].numpy()
    scale = np.abs(A64).max()
    dx = dev(x)
    for tile in (L, 512):
        T = L // tile
        stats = fused_ops.row_stats(dx.view(B, C * T, tile)).view(B, C, T, 2)
        A = host(fused_ops.groupnorm_fold(stats, gn, fac, gb, L)[0])
        a32 = pr.onepass_fold_a32(x, tile, G, host(gn.weight), host(fac), gn.eps)
        e_ref = np.abs(a32.astype(np.float64) - A64).max() / scale
        e_ker = np.abs(A.astype(np.float64) - A64).max() / scale
        print(f"conditioning mean/std={ratio:g} tile={tile}: CPU one-pass {e_ref:.3e}  kernel {e_ker:.3e}")
        assert e_ker <= 4 * e_ref, (ratio, tile, e_ref, e_ker)


# ---- e. lion_affine_swish, lion_affine_swish_add ----------------------------------------------------------------------

def check_swish(x, a, b, add, tag):
    """x [rows, L], a / b [rows] (fp32 numpy) through fused_ops.affine_swish as [rows, 1, L]"""
    from lion_amd import fused_ops
    rows, L = x.shape
    t = pr.affine_arg32(x, a[:, None], b[:, None])
    ref = pr.swish64(t)
    dx, dA, dB = dev(x.reshape(rows, 1, L)), dev(a.reshape(rows, 1)), dev(b.reshape(rows, 1))
    got = host(fused_ops.affine_swish(dx, dA, dB)).reshape(rows, L)
    within(got, ref, pr.swish_bound(t, ref), tag + " swish")
    if add is not None:
        got = host(fused_ops.affine_swish(dx, dA, dB, add=dev(add.reshape(rows, 1, L)))).reshape(rows, L)
        within(got, ref + add.astype(np.float64), pr.swish_add_bound(t, add), tag + " swish_add")


def swish_case(rows, L, seed, sign=1.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, L)) * 3).astype(np.float32)
    a = (sign * rng.uniform(0.5, 1.5, rows) * np.where(np.arange(rows) % 2, -1.0, 1.0)).astype(np.float32)
    b = rng.standard_normal(rows).astype(np.float32)
    add = rng.standard_normal((rows, L)).astype(np.float32)
    return x, a, b, add


@pytest.mark.parametrize("L", [1, 3, 4, 5, 1023, 1024, 1025, 1028, 2049])
def test_affine_swish_and_add_against_float64(L):
    """one float4 per lane when L % 4 == 0, else four scalars; rows that end inside the first, at the end of a, and inside a
    later workgroup of 1024 elements; a scale of either sign in every row position"""
    for rows in (1, 5):
        for sign in (1.0, -1.0):
            check_swish(*swish_case(rows, L, 10 * L + rows, sign), f"rows={rows} L={L} sign={sign:+g}")


@pytest.mark.parametrize("pad", [0, 3])
def test_affine_swish_extreme_arguments_stay_finite(pad):
    """t in {0, -0.0, +-1e-30, +-20, +-100} exactly (a = 1; b = +0 and b = -0, which is what keeps x = -0.0 at t = -0.0):
    exp overflows at t = -100 and underflows at +100, the reciprocal meets infinity, and nothing may come out but a finite
    number within the bound.  pad = 3 makes L = 12: the float4 path"""
    vals = [0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0, 5.0] + [50.0, -50.0, -5.0][:pad]
    x = np.array([vals, vals], dtype=np.float32)
    a = np.array([1.0, 1.0], dtype=np.float32)
    b = np.array([0.0, -0.0], dtype=np.float32)
    t = pr.affine_arg32(x, a[:, None], b[:, None])
    assert np.array_equal(t[0, 2:], x[0, 2:]) and np.signbit(t[1, 1]) and not np.signbit(t[0, 1])
    add = np.full_like(x, 0.25)
    check_swish(x, a, b, add, f"extremes L={x.shape[1]}")


# ---- f. lion_affine_swish_max -----------------------------------------------------------------------------------------

def max_case(rows, M, U, seed):
    """x [rows, M, U] whose activated maximum of centre m sits at u = m % U: arguments t in [-6, 2] (across the minimum of
    swish) everywhere else, in [6, 8] at the planted place; every fifth centre lies left of the minimum instead, t in
    [-6, -0.5] with [-14, -10] planted, where the SMALLEST argument has the largest swish; a of both signs"""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(0.5, 1.5, rows) * np.where(np.arange(rows) % 2, -1.0, 1.0)).astype(np.float32)
    b = rng.standard_normal(rows).astype(np.float32)
    t = rng.uniform(-6, 2, (rows, M, U))
    m = np.arange(M)
    left = m % 5 == 4
    t[:, left, :] = rng.uniform(-6, -0.5, (rows, int(left.sum()), U))
    t[:, m, m % U] = np.where(left, rng.uniform(-14, -10, (rows, M)), rng.uniform(6, 8, (rows, M)))
    x = ((t - b[:, None, None]) / a[:, None, None]).astype(np.float32)
    return x, a, b


def check_swish_max(rows, M, U, seed):
    from lion_amd import fused_ops
    x, a, b = max_case(rows, M, U, seed)
    t = pr.affine_arg32(x, a[:, None, None], b[:, None, None])
    s = pr.swish64(t)
    assert np.array_equal(s.argmax(-1), np.broadcast_to(np.arange(M) % U, (rows, M)))
    dx, dA, dB = dev(x.reshape(rows, 1, M, U)), dev(a.reshape(rows, 1)), dev(b.reshape(rows, 1))
    got = fused_ops.affine_swish(dx, dA, dB, reduce_max=True)
    assert tuple(got.shape) == (rows, 1, M)
    within(host(got).reshape(rows, M), s.max(-1), pr.swish_bound(t, s).max(-1), f"swish_max rows={rows} M={M} U={U}")
    # the same arithmetic, stored and reduced by torch: a difference here is indexing, not rounding
    assert torch.equal(got, torch.amax(fused_ops.affine_swish(dx, dA, dB), dim=-1))


@pytest.mark.parametrize("U", [16, 32, 64])
def test_affine_swish_max_cooperative_kernels(U):
    """U / 4 lanes per centre, P = 4 * (64 / LPM) * 8 centres per workgroup: a workgroup's last centre, its first, a
    clamped tail, several workgroups"""
    P = 4 * (64 // (U // 4)) * 8
    assert P == {16: 512, 32: 256, 64: 128}[U]
    for M in (1, 7, P - 1, P, P + 1, 2 * P + 3):
        check_swish_max(6, M, U, 100 * U + M)


@pytest.mark.parametrize("U", [8, 128, 1, 3, 5])
def test_affine_swish_max_generic_kernel(U):
    """one lane per centre: float4 reads for U % 4 == 0 outside the cooperative widths, scalar reads otherwise"""
    for M in (1, 255, 256, 257):
        check_swish_max(6, M, U, 100 * U + M)


# ---- g. lion_timestep_embedding ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1000.0, 1.0])
@pytest.mark.parametrize("B,half,D", [(1, 32, 64), (5, 32, 65), (33, 3, 6), (7, 100, 200), (300, 1, 3)])
def test_timestep_embedding_against_float64_of_the_fp32_angle(B, half, D, scale):
    from lion_amd import _lib
    rng = np.random.default_rng(B + D)
    t = np.concatenate([[1.0, 0.0, 1e-5, 0.5], rng.uniform(0, 1, B)]).astype(np.float32)[:B]
    row = pr.frequency_row(half) if half > 1 else np.array([0.37], dtype=np.float32)
    emb = torch.full((B, D), float("nan"), device="cuda")
    _lib.call("lion_timestep_embedding", dev(t), dev(row), float(scale), B, half, D, emb)
    got = host(emb)
    within(got, pr.timestep_embedding64(t, row, scale, D), pr.TIMESTEP_ATOL, f"timestep B={B} half={half} D={D}")
    if D > 2 * half:
        assert np.all(got[:, 2 * half:] == 0.0)


# ---- h. more rows than one grid dimension holds -----------------------------------------------------------------------

def test_affine_swish_and_add_of_more_than_65535_rows():
    """B x C > 65535 (batch 128 at the 512 channels of the last set-abstraction MLP): the row rides on blockIdx.y, so the
    rows past the 65535 of one launch go out in a second one on offset pointers"""
    check_swish(*swish_case(65539, 5, 1), "rows=65539 L=5")


@pytest.mark.parametrize("U", [4, 16])
def test_affine_swish_max_of_more_than_65535_rows(U):
    check_swish_max(65539, 3, U, U)
