"""CPU: the float64 references of tests/pointwise_ref.py against the module arithmetic they stand for, in float64, and
their error bounds against an fp32 numpy emulation of the kernels' arithmetic (csrc/pointwise.hip)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointwise_ref as pr


@pytest.mark.parametrize("B,C,G,L", [(1, 8, 8, 5), (3, 24, 8, 77), (2, 64, 1, 130), (2, 40, 8, 33)])
def test_adagn_fold64_is_group_norm_times_factor_plus_bias(B, C, G, L):
    g = torch.Generator().manual_seed(C + L)
    x = torch.randn(B, C, L, generator=g, dtype=torch.float64) * 1.7 + 0.8
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    fac = torch.randn(B, C, generator=g, dtype=torch.float64)
    gb = torch.randn(B, C, generator=g, dtype=torch.float64)
    A, Bs, cm = pr.adagn_fold64(x, G, gamma, beta, fac, gb, 1e-5)
    want = torch.nn.functional.group_norm(x, G, gamma, beta, 1e-5) * fac[:, :, None] + gb[:, :, None]
    got = x * A[:, :, None] + Bs[:, :, None]
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert (cm - x.mean(-1)).abs().max().item() <= 1e-14
    # a single [1, C] row of fac / gbias serves every sample
    A1, B1, _ = pr.adagn_fold64(x, G, gamma, beta, fac[:1], gb[:1], 1e-5)
    want1 = torch.nn.functional.group_norm(x, G, gamma, beta, 1e-5) * fac[:1, :, None] + gb[:1, :, None]
    assert (x * A1[:, :, None] + B1[:, :, None] - want1).abs().max().item() <= 1e-12 * want1.abs().max().item()


@pytest.mark.parametrize("C", [8, 64, 1000])
def test_se_gate64_is_se3d_on_the_mean_of_the_normalised_grid(C):
    from lion_amd.models.pvcnn2_ada import SE3d
    torch.manual_seed(C)
    se = SE3d(C).double()
    B, V = 3, 50
    y = torch.randn(B, C, V, dtype=torch.float64) + 0.3
    A = torch.randn(B, C, dtype=torch.float64)
    Bs = torch.randn(B, C, dtype=torch.float64)
    with torch.no_grad():
        gate = se.fc((y * A[:, :, None] + Bs[:, :, None]).mean(-1))
    A2, B2 = pr.se_gate64(A, Bs, y.mean(-1), se.fc[0].weight.detach(), se.fc[2].weight.detach())
    assert (A2 - A * gate).abs().max().item() <= 1e-13
    assert (B2 - Bs * gate).abs().max().item() <= 1e-13


@pytest.mark.parametrize("D,scale", [(64, 1000.0), (65, 1000.0), (6, 1.0), (200, 1000.0)])
def test_timestep_embedding64_is_the_eager_branch(D, scale):
    """the eager branch of get_timestep_embedding forms the same two fp32 products; its fp32 sin / cos of that angle are
    within an ulp or two of the float64 ones"""
    from lion_amd.models.latent_points_ada import PVCNN2Unet
    t = torch.tensor([0.0, 1e-5, 0.5, 1.0, 0.123, 0.987], dtype=torch.float32)
    me = SimpleNamespace(embed_dim=D, time_emb_scales=scale)
    eager = PVCNN2Unet.get_timestep_embedding(me, t, torch.device("cpu"))
    row = pr.frequency_row(D // 2)
    assert np.array_equal(row, me._freq_cache[torch.device("cpu")].numpy())
    ref = pr.timestep_embedding64(t.numpy(), row, scale, D)
    assert tuple(eager.shape) == ref.shape == (6, D)
    assert np.abs(eager.double().numpy() - ref).max() <= pr.TIMESTEP_ATOL
    if D % 2:
        assert np.all(ref[:, -1] == 0.0) and np.all(eager[:, -1].numpy() == 0.0)
    # not the float64 angle: at t * scale * row ~ 1000 one fp32 rounding of the angle moves sin by far more than the bound
    if scale == 1000.0:
        exact = np.sin(np.float64(0.987) * scale * row.astype(np.float64))
        assert np.abs(exact - ref[5, :D // 2]).max() > 4 * pr.TIMESTEP_ATOL


def test_swish64_limits_and_symmetry():
    t = np.array([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0, 800.0, -800.0])
    s = pr.swish64(t)
    assert np.all(np.isfinite(s))
    naive = t[:8] / (1.0 + np.exp(-t[:8]))
    assert np.allclose(s[:8], naive, rtol=1e-15, atol=0)
    assert s[8] == 800.0 and s[9] == 0.0
    x = np.linspace(-30, 30, 601)
    assert np.allclose(pr.swish64(x) - pr.swish64(-x), x, rtol=1e-14, atol=1e-14)   # swish(t) - swish(-t) = t


def _row_sums32(x, float4):
    """row_stats_kernel's arithmetic in fp32 numpy: 256 lanes, each serial over its strided elements (float4: the pair
    sums first), then the xor-butterfly over the 64 lanes of a wave and the pairwise sum of the 4 waves"""
    f = np.float32
    L = x.shape[0]
    s1, s2 = np.zeros(256, f), np.zeros(256, f)
    if float4:
        for i0 in range(0, L, 1024):
            blk = np.zeros(1024, f)
            n = min(1024, L - i0)
            blk[:n] = x[i0:i0 + n]
            v = blk.reshape(256, 4)
            q = (v * v).astype(f)
            s1 = (s1 + ((v[:, 0] + v[:, 1]).astype(f) + (v[:, 2] + v[:, 3]).astype(f)).astype(f)).astype(f)
            s2 = (s2 + ((q[:, 0] + q[:, 1]).astype(f) + (q[:, 2] + q[:, 3]).astype(f)).astype(f)).astype(f)
    else:
        for i0 in range(0, L, 256):
            blk = np.zeros(256, f)
            n = min(256, L - i0)
            blk[:n] = x[i0:i0 + n]
            s1 = (s1 + blk).astype(f)
            s2 = (s2 + (blk * blk).astype(f)).astype(f)
    out = []
    for s in (s1, s2):
        w = s.reshape(4, 64)
        for m in (1, 2, 4, 8, 16, 32):
            w = (w + w[:, np.arange(64) ^ m]).astype(f)
        out.append(f(f(w[0, 0] + w[1, 0]) + f(w[2, 0] + w[3, 0])))
    return out


@pytest.mark.parametrize("L", [1, 5, 255, 1023, 1028, 4097, 32768])
def test_row_sum_bound_holds_for_the_kernels_summation_order(L):
    rng = np.random.default_rng(L)
    x = (rng.standard_normal(L) * 1.5 + 3.0).astype(np.float32)
    s1, s2 = _row_sums32(x, L % 4 == 0)
    d = x.astype(np.float64)
    g = pr.row_sum_gamma(L)
    assert abs(float(s1) - d.sum()) <= g * np.abs(d).sum()
    assert abs(float(s2) - (d * d).sum()) <= g * (d * d).sum()


def test_swish_bound_holds_for_fp32_arithmetic():
    """t * (1 / (1 + exp(-t))) with every operation rounded to fp32 (numpy's expf is within an ulp, as v_exp_f32)"""
    f = np.float32
    rng = np.random.default_rng(0)
    t = np.concatenate([rng.standard_normal(20000) * 6, rng.uniform(-80, 80, 20000),
                        [0.0, -0.0, 1e-30, -1e-30, 20, -20, 100, -100]]).astype(f)
    with np.errstate(over="ignore"):
        e = np.exp(-t).astype(f)
        got = (t * (f(1) / (f(1) + e).astype(f)).astype(f)).astype(f)
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(np.float64) - pr.swish64(t))
    assert np.all(err <= pr.swish_bound(t))
    add = rng.standard_normal(t.shape[0]).astype(f)
    err = np.abs((got + add).astype(f).astype(np.float64) - (pr.swish64(t) + add.astype(np.float64)))
    assert np.all(err <= pr.swish_add_bound(t, add))
    # the bound separates neighbours: a value taken from the next element of a ramp is outside it
    ramp = np.linspace(-4, 4, 101).astype(f)
    assert np.all(np.abs(pr.swish64(ramp[1:]) - pr.swish64(ramp[:-1]))[np.abs(ramp[1:] + 1.278) > 0.2]
                  > pr.swish_bound(ramp[1:])[np.abs(ramp[1:] + 1.278) > 0.2])


def test_affine_arg32_rounds_product_then_sum():
    x, a, b = np.float32(1.0000001), np.float32(1.0000001), np.float32(-1.0)
    t = pr.affine_arg32(x, a, b)
    assert t.dtype == np.float32
    assert t == np.float32(np.float32(x * a) + b)
    assert float(t) != float(x) * float(a) + float(b)      # a fused multiply-add would keep the low bits of the product


def test_timestep_bound_holds_for_fp32_sin_cos():
    rng = np.random.default_rng(1)
    t = rng.uniform(0, 1, 64).astype(np.float32)
    row = pr.frequency_row(100)
    ref = pr.timestep_embedding64(t, row, 1000.0, 200)
    ang = ((t * np.float32(1000.0)).astype(np.float32)[:, None] * row[None, :]).astype(np.float32)
    got = np.concatenate([np.sin(ang), np.cos(ang)], 1)
    assert got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - ref).max() <= pr.TIMESTEP_ATOL


@pytest.mark.parametrize("C,H", [(65, 8), (1024, 128)])
def test_gate_bound_holds_for_fp32_dot_products(C, H):
    rng = np.random.default_rng(C)
    f = np.float32
    B = 3
    A, Bs, cm = (rng.standard_normal((B, C)).astype(f) for _ in range(3))
    w1 = (rng.standard_normal((H, C)) / np.sqrt(C)).astype(f)
    w2 = (rng.standard_normal((C, H)) / np.sqrt(H)).astype(f)
    s = ((A * cm).astype(f) + Bs).astype(f)
    h = np.zeros((B, H), f)
    for c in range(C):                     # serial fp32 accumulation: the worst order the bound has to cover
        h = (h + (w1[:, c][None, :] * s[:, c][:, None]).astype(f)).astype(f)
    h = np.maximum(h, 0)
    acc = np.zeros((B, C), f)
    for j in range(H):
        acc = (acc + (w2[:, j][None, :] * h[:, j][:, None]).astype(f)).astype(f)
    g32 = (f(1) / (f(1) + np.exp(-acc).astype(f)).astype(f)).astype(f)
    A64, _ = pr.se_gate64(A, Bs, cm, w1, w2)
    g64 = (A64 / torch.from_numpy(A).double()).numpy()
    bound = pr.gate_bound(A, Bs, cm, w1, w2).numpy()
    assert np.all(np.abs(g32.astype(np.float64) - g64) <= bound)
    assert bound.max() < (1e-4 if C == 65 else 1e-2)   # a worst case: orders above what a random sum loses


@pytest.mark.parametrize("ratio", [0.0, 8.0, 64.0])
def test_onepass_fold_stays_within_the_worst_case_of_its_conditioning(ratio):
    """the fp32 one-pass emulation (the yardstick of the conditioning test in tests/test_pointwise_numerics_gpu.py) against
    adagn_fold64.  Worst case: numpy's fp32 sum nests at most ~24 additions (16 serial per accumulator, then the trees),
    + 1 for the squaring: g = 25u relative on sum x and sum x^2; var = E[x^2] - mean^2 then errs by at most
    g (E[x^2] + 2 mean^2) <= 3 g (1 + r^2) var with r = mean/std; A ~ var^-1/2 takes half of that relatively: 38 (1 + r^2) u,
    plus the three fp32 roundings of rstd * gamma * fac."""
    rng = np.random.default_rng(int(ratio))
    B, C, G, L = 2, 16, 8, 4096
    x = (rng.standard_normal((B, C, L)) + ratio).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    fac = rng.uniform(0.5, 1.5, (B, C)).astype(np.float32)
    A64, _, _ = pr.adagn_fold64(x, G, gamma, np.zeros(C), fac, np.zeros((B, C)), 1e-5)
    for tile in (L, 512):
        a32 = pr.onepass_fold_a32(x, tile, G, gamma, fac, 1e-5)
        rel = np.abs(a32.astype(np.float64) - A64.numpy()).max() / A64.abs().max().item()
        assert rel <= (38 * (1 + ratio * ratio) + 3) * pr.U32
