"""Float64 references of the inference AdaGN / pointwise kernels (csrc/pointwise.hip, gn_fold_kernel / gn_fold_se_kernel of
csrc/conv3d.hip) and the error bounds their fp32 arithmetic is held to.  numpy / torch on the CPU; imports nothing from
lion_amd (tests/test_pointwise_reference_cpu.py ties every function to the module arithmetic it stands for).

u = 2^-24 is the unit roundoff of fp32: one correctly rounded operation errs by at most u relative, a "1 ulp" hardware
function (v_exp_f32, v_rcp_f32) by at most 2u."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24


def _f64(a):
    return a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=torch.float64)


def adagn_fold64(x, G, gamma, beta, fac, gbias, eps):
    """x [B, C, ...] -> float64 (A, Bs, chmean), each [B, C], with AdaGN(x)[b, c] == x[b, c] * A[b, c] + Bs[b, c]:
        A = rstd_g * gamma_c * f_bc,  Bs = (beta_c - mean_g * rstd_g * gamma_c) * f_bc + g_bc
    (the comment above gn_fold_kernel), mean_g / rstd_g from the DATA of the group (two-pass, biased variance, as
    GroupNorm), chmean the mean of the channel."""
    x = _f64(x)
    B, C = x.shape[:2]
    x = x.reshape(B, C, -1)
    gamma, beta, fac, gbias = (_f64(v) for v in (gamma, beta, fac, gbias))
    cpg = C // G
    xg = x.reshape(B, G, -1)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1)
    rstd = (var + eps).rsqrt().repeat_interleave(cpg, 1)
    mean = mean[..., 0].repeat_interleave(cpg, 1)
    fac, gbias = fac.expand(B, C), gbias.expand(B, C)
    A = rstd * gamma * fac
    Bs = (beta - mean * rstd * gamma) * fac + gbias
    return A, Bs, x.mean(-1)


def se_gate64(A, Bs, chmean, w1, w2):
    """the SE3d gate on the folded scalars (se_gate_kernel): the mean over the grid of AdaGN(y) is A * chmean + Bs, so
    g = sigmoid(W2 relu(W1 (A * chmean + Bs))) and (A, Bs) <- (A * g, Bs * g).  w1 [H, C], w2 [C, H] (nn.Linear layouts)."""
    A, Bs, chmean, w1, w2 = (_f64(v) for v in (A, Bs, chmean, w1, w2))
    h = torch.relu((A * chmean + Bs) @ w1.t())
    g = torch.sigmoid(h @ w2.t())
    return A * g, Bs * g


def swish64(t):
    """t * sigmoid(t) in float64 without overflow for any finite fp32 t"""
    t = np.asarray(t, dtype=np.float64)
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, t / (1.0 + e), t * e / (1.0 + e))


def affine_arg32(x, a, b):
    """the fp32 argument of the activation exactly as the kernels form it without contraction: round(round(x * a) + b)"""
    x, a, b = (np.asarray(v, dtype=np.float32) for v in (x, a, b))
    return ((x * a).astype(np.float32) + b).astype(np.float32)


def timestep_embedding64(t, row, scale, D):
    """[B, D] float64: sin | cos of the fp32 angle mul_rn(mul_rn(t, scale), row) (timestep_embedding_kernel; the eager
    branch of get_timestep_embedding rounds the same two products), evaluated in float64; an odd D has a zero last column."""
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    row = np.asarray(row, dtype=np.float32).reshape(-1)
    ts = (t * np.float32(scale)).astype(np.float32)
    ang = (ts[:, None] * row[None, :]).astype(np.float32).astype(np.float64)
    emb = np.zeros((t.shape[0], D), dtype=np.float64)
    half = row.shape[0]
    emb[:, :half] = np.sin(ang)
    emb[:, half:2 * half] = np.cos(ang)
    return emb


def frequency_row(half):
    """the row of get_timestep_embedding: 10000^(-i / (half - 1)) in float64, cast to fp32"""
    return np.exp(np.arange(0, half) * -(np.log(10000) / (half - 1))).astype(np.float32)


def onepass_fold_a32(x, tile, G, gamma, fac, eps):
    """A of the inference fold by the kernel's own ONE-PASS formula on the CPU: fp32 sums of x and of round(x * x) per tile
    of `tile` consecutive elements, tiles and channels combined in float64, var = E[x^2] - mean^2, then
    rstd -> fp32, * gamma, * fac in fp32 (gn_fold_kernel).  Its error against adagn_fold64 is what the formula costs at a
    given mean/std whatever the summation order: the yardstick of the kernel's conditioning."""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape[:2]
    xt = x.reshape(B, C, -1, tile)
    s1 = xt.sum(-1, dtype=np.float32).astype(np.float64).sum(-1)
    s2 = (xt * xt).astype(np.float32).sum(-1, dtype=np.float32).astype(np.float64).sum(-1)
    return fold_a_from_sums(s1, s2, xt.shape[2] * tile, G, gamma, fac, eps)


def fold_a_from_sums(s1, s2, count, G, gamma, fac, eps):
    """the tail of onepass_fold_a32 from float64 channel totals s1, s2 [B, C] over `count` elements per channel"""
    B, C = s1.shape
    cpg = C // G
    n = float(count) * cpg
    mean = s1.reshape(B, G, cpg).sum(-1) / n
    var = np.maximum(s2.reshape(B, G, cpg).sum(-1) / n - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + float(np.float32(eps)))).astype(np.float32).repeat(cpg, 1)
    a0 = (rstd * np.asarray(gamma, dtype=np.float32)[None, :]).astype(np.float32)
    return (a0 * np.broadcast_to(np.asarray(fac, dtype=np.float32), (B, C))).astype(np.float32)


# ---- error bounds -----------------------------------------------------------------------------------------------------

def row_sum_gamma(L):
    """|s1 - sum x| <= gamma * sum |x| and |s2 - sum x^2| <= gamma * sum x^2 for row_stats_kernel: a lane adds at most
    ceil(L / 256) terms serially (the scalar path; the float4 path a quarter of that), then the fixed tree of 4 DPP steps,
    2 shuffles and 2 LDS adds; the squaring and the pair sums inside a float4 take the rest of the 12."""
    return (math.ceil(L / 256) + 12) * U32


def swish_bound(t, ref=None):
    """bound of |swish_fast(t) - swish64(t)| for the SAME fp32 t: (|t| + 8) u |swish64(t)| + 1e-35.
    |t| u: the rounded product -t * log2(e) in front of v_exp_f32 moves e^-t by that much relatively; 8 u: v_exp_f32
    (1 ulp = 2u), the rounding of 1 + e (u), v_rcp_f32 (2u), the final product (u), and slack for the rounded constant.
    1e-35: results below the normal range, where the hardware may flush to zero."""
    t = np.asarray(t, dtype=np.float64)
    ref = swish64(t) if ref is None else np.asarray(ref, dtype=np.float64)
    return (np.abs(t) + 8.0) * U32 * np.abs(ref) + 1e-35


def swish_add_bound(t, addend):
    """swish_bound plus the one rounding of the sum with the addend"""
    s = swish64(t)
    add = np.asarray(addend, dtype=np.float64)
    b = swish_bound(t, s)
    return b + U32 * (np.abs(s + add) + b)


TIMESTEP_ATOL = 4 * U32   # values in [-1, 1]: the spacing of fp32 there is <= u, device sinf / cosf are specified to a couple of ulp

FOLD_RTOL = 1e-5          # of the largest reference magnitude (tests/test_fold_se_gpu.py, same arithmetic), mean/std <= 1


def gate_bound(A, Bs, chmean, w1, w2, n1=None, n2=None):
    """bound of the fp32 gate's error |g32 - g64| per (batch, channel), propagated: every entry of the first dot product
    (additions nested n1 deep -- C for a serial sum, ceil(C / 64) + 6 for se_gate_kernel's lane-strided sum and butterfly --
    inputs rounded thrice) errs by at most (n1 + 4) u sum|w1 s|, relu is 1-Lipschitz, the second dot product (n2 deep, H
    serially) adds (n2 + 1) u sum|w2 h| and carries the first error through |w2|, sigmoid is 1/4-Lipschitz; + 4u for expf,
    the sum and the division."""
    A, Bs, chmean, w1, w2 = (_f64(v) for v in (A, Bs, chmean, w1, w2))
    n1 = w1.shape[1] if n1 is None else n1
    n2 = w1.shape[0] if n2 is None else n2
    s = A * chmean + Bs
    sa = (A * chmean).abs() + Bs.abs()
    e1 = (n1 + 4) * U32 * (sa @ w1.abs().t())
    h = torch.relu(s @ w1.t())
    e2 = (n2 + 1) * U32 * ((h + e1) @ w2.abs().t()) + e1 @ w2.abs().t()
    return 0.25 * e2 + 4 * U32
